"""A signature is written once: the public entry points in include/iunet.h, the internal launchers in csrc/launchers.h (common.h includes
both, so the compiler checks every definition and every call against them).  This test reads source text only and keeps hand-copied
forward declarations from coming back: no other file under csrc/ declares an iunet_* function.  A declaration is a statement outside
every function body that starts with a return type, names an iunet_* function and ends in `;`; definitions (the inline helpers of
common.h among them) are not."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'interactive-unet_amd', 'csrc')
COMMENT = re.compile(r'/\*.*?\*/|//[^\n]*', re.S)
STRING = re.compile(r'"(?:\\.|[^"\\\n])*"|\'(?:\\.|[^\'\\\n])*\'')
PREPROCESSOR = re.compile(r'^[ \t]*#(?:[^\n]*\\\n)*[^\n]*', re.M)
OPEN_SCOPE = re.compile(r'(?:extern\s*"C"|namespace(?:\s+\w+)?)$')          # braces that open no body
DECLARATION = re.compile(r'(?:extern\s*"C"\s*)?(?:[A-Za-z_][\w:<>]*[\s*&]+)+(iunet_\w+)\s*\(')


def declarations(text):
    """[(line, name)] of the iunet_* function declarations of a source text."""
    blank = lambda m: re.sub(r'[^\n]', ' ', m.group(0))
    text = COMMENT.sub(blank, text)
    text = STRING.sub(lambda m: m.group(0) if m.group(0) == '"C"' else blank(m), text)
    text = PREPROCESSOR.sub(blank, text)
    found, scopes, start, parens = [], [], 0, 0
    for i, ch in enumerate(text):
        if ch in '()':
            parens += 1 if ch == '(' else -1
        elif ch in '{}':
            if ch == '{':
                scopes.append(bool(OPEN_SCOPE.match(text[start:i].strip())))
            else:
                scopes.pop()
            start = i + 1
        elif ch == ';' and parens == 0:
            stmt = text[start:i]
            m = DECLARATION.match(stmt.strip()) if all(scopes) else None
            if m:
                found.append((text.count('\n', 0, i - len(stmt.lstrip())) + 1, m.group(1)))
            start = i + 1
    assert not scopes and parens == 0, 'unbalanced source text'
    return found


def test_the_scan_finds_declarations_and_only_them():
    """A slip in the scan must not pass silently."""
    text = '''
    #include "common.h"
    #define M(x) do { int iunet_in_macro(int); } while (0)
    // int iunet_in_comment(int);
    extern "C" {
    int iunet_a(int, const void*,
                long long);
    long long iunet_b(void);          /* int iunet_c(int); */
    }
    extern "C" int iunet_d(void* slab, int n);
    const char* iunet_e(void);
    namespace {
    int iunet_f(int nd, hipStream_t stream, int out8 = 0);
    inline int iunet_defined(int x) { int iunet_local(int); return iunet_a(x, nullptr, 0); }
    }
    typedef void (*iunet_hook)(void* ctx, int stage);
    static int g = iunet_call(3);
    int iunet_g(int x) {
      const char* s = "int iunet_in_string(int);";
      return iunet_b() ? iunet_d(nullptr, x) : 0;
    }
    '''
    assert declarations(text) == [(6, 'iunet_a'), (8, 'iunet_b'), (10, 'iunet_d'), (11, 'iunet_e'), (13, 'iunet_f')]


def test_launchers_h_alone_declares_iunet_functions():
    hits, seen = [], 0
    for f in sorted(os.listdir(CSRC)):
        if f.endswith(('.hip', '.h')):
            seen += 1
            found = declarations(open(os.path.join(CSRC, f)).read())
            if f == 'launchers.h':
                names = [n for _, n in found]
                assert len(names) >= 30 and len(set(names)) == len(names), 'each launcher is declared exactly once'
            else:
                hits += [f'csrc/{f}:{line}: {name}' for line, name in found]
    assert seen > 25, seen
    assert not hits, '\n'.join(hits)
