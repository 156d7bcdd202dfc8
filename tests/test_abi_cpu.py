"""CPU-side checks of the drop-in boundary: libiunet.so loads and exports every symbol
include/iunet.h declares; argument validation works without a GPU."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _lib():
    from interactive_unet import _native
    if not os.path.isfile(_native.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _native, ctypes.CDLL(_native.LIB_PATH)


def _header():
    """include/iunet.h without comments and preprocessor lines."""
    text = open(os.path.join(ROOT, 'include', 'iunet.h')).read()
    return re.sub(r'^[ \t]*#.*$', '', re.sub(r'/\*.*?\*/|//[^\n]*', ' ', text, flags=re.S), flags=re.M)


def test_library_exports_every_declared_symbol():
    """The library's unmangled iunet_* symbols, the header's functions and the bound names are ONE set."""
    nv, lib = _lib()
    declared = set(re.findall(r'\b(iunet_[a-z0-9_A-Z]+)\s*\(', _header()))
    assert len(declared) >= 15
    for name in declared:
        assert hasattr(lib, name), f'{name} declared in include/iunet.h but not exported'
    nm = shutil.which('nm') or shutil.which('llvm-nm')
    assert nm, 'nm is needed to list the symbols libiunet.so defines'
    out = subprocess.run([nm, '-D', '--defined-only', nv.LIB_PATH], capture_output=True, text=True, check=True).stdout
    defined = {line.split()[-1] for line in out.splitlines() if line.split()}
    exported = {n for n in defined if re.fullmatch(r'iunet_\w+', n)}          # C linkage; the internal launchers are mangled (_Z...)
    assert exported == declared, (sorted(exported - declared), sorted(declared - exported))
    assert set(nv.exported_symbols()) == declared and len(nv.exported_symbols()) == len(declared)


def test_every_declaration_of_the_header_is_mapped():
    """A prototype the parser's pattern skips silently would leave a function with ctypes' default (int) signature."""
    from interactive_unet import _native as nv
    assert len(nv.parse_header(open(os.path.join(ROOT, 'include', 'iunet.h')).read())) == len(re.findall(r'iunet_\w+\s*\(', _header())) > 200


def test_derived_signatures_match_the_pinned_ones():
    """restype / argtypes as read off include/iunet.h by hand, for functions that together hold every type class of the mapping."""
    from interactive_unet import _native as nv
    I, L, F, D, V, S = ctypes.c_int, ctypes.c_longlong, ctypes.c_float, ctypes.c_double, ctypes.c_void_p, ctypes.c_char_p
    PI, PL, PD, PV = (ctypes.POINTER(t) for t in (I, L, D, V))
    pinned = {
        'iunet_conv3_fwd': (I, [I, I, V, L, V, L, V, V, V, I, I, I, I, I, I, I, I, V]),
        'iunet_bn_finalize': (I, [V, I, I, D, V, V, V, V, F, F, V, V, V, V, V]),
        'iunet_zoom_nearest_u8': (I, [V, PI, PL, V, PL, PI, V, V]),                       # tables: const int* on the DEVICE -> an address
        'iunet_bn_relu_sum_bwd': (I, [I, I, I, PV, PL, V, L, V, L, V, L, V, V, V, V, V, V, V, V, V, I, I, I, I, I, V]),
        'iunet_net_create': (I, [I, I, I, I, I, I, F, PV]),
        'iunet_net_param': (I, [V, I, S, I, PL, PL]),
        'iunet_train_forward_backward_hooks': (I, [V, V, I, PL, V, V, I, I, I, I, I, V, V, V, V, V]),
        'iunet_train_bind': (I, [V, V, V, V, V, PV, V, V, V]),                            # void* const*
        'iunet_slice_gather': (I, [V, I, I, I, PD, PI, PI, I, I, I, V, V]),               # const double*
        'iunet_conv3_plan': (I, [I] * 10 + [PI]),                                         # int* (an output)
        'iunet_net_workspace_bytes': (L, [V, I, I, I, I]),
        'iunet_net_destroy': (None, [V]),
        'iunet_last_error': (S, []),
    }
    sigs = nv.signatures()
    for name, (restype, argtypes) in pinned.items():
        assert sigs[name][0] is restype, name
        assert len(sigs[name][1]) == len(argtypes) and all(a is b for a, b in zip(sigs[name][1], argtypes)), name
    l = _lib()[0].lib()                                                                   # and they are what the loaded library carries
    for name, (restype, argtypes) in pinned.items():
        assert getattr(l, name).restype is restype and list(getattr(l, name).argtypes) == argtypes, name


def test_the_parser_refuses_a_type_it_does_not_know():
    from interactive_unet import _native as nv
    with pytest.raises(nv.NativeError, match=r'iunet_odd\b.*short n'):
        nv.parse_header('int iunet_fine(int a, const void* p);\nint iunet_odd(int a, short n, void* stream);\n')
    with pytest.raises(nv.NativeError, match='iunet_ret'):
        nv.parse_header('unsigned iunet_ret(void);\n')
    with pytest.raises(nv.NativeError, match='iunet_ptr'):
        nv.parse_header('int iunet_ptr(float* p);\n')                                     # no float arrays cross the ABI: not guessed
    assert nv.parse_header('void iunet_ok(void);\n') == {'iunet_ok': (None, [])}


def test_error_reporting_without_gpu():
    nv, _ = _lib()
    l = nv.lib()
    assert l.iunet_abi_version() >= 1
    # argument validation happens before any HIP call: bad dtype -> error code + message
    rc = l.iunet_pack_conv3(7, None, None, None, 32, 32, 9, 0, None)
    assert rc < 0 and b'dtype' in l.iunet_last_error()
    with pytest.raises(nv.NativeError):
        nv.check(rc)
    # the retired kernel structures are refused by name, after the checks above and before any launch
    buf = (nv.c_int * 16)()
    for lay in (0, 1):
        rc = l.iunet_conv3_fwd(0, 3, buf, 0, buf, 0, buf, None, None, 1, 4, 4, 4, 32, 32, 0, lay, None)
        assert rc < 0 and b'layout' in l.iunet_last_error(), lay
    rc = l.iunet_pack_conv3(0, buf, None, buf, 32, 32, 9, 0, None)
    assert rc < 0 and b'mode' in l.iunet_last_error()


def test_zoom_table_host_function_matches_oracle():
    """iunet_zoom_nearest_table / _len are host-only arithmetic (no GPU): identical to the oracle's table (itself pinned
    against scipy.ndimage.zoom in test_oracle_golden.py), and bad arguments are refused."""
    import numpy as np
    from oracle import multiscale_ref as mr
    nv, _ = _lib()
    l = nv.lib()
    for n in list(range(1, 200)) + [255, 256, 257, 384, 512, 1000, 1024]:
        for zoom in (0.5, 0.25, 0.3, 0.75):
            want = mr.zoom_table(n, zoom)
            m = l.iunet_zoom_nearest_len(n, zoom)
            assert m == len(want), (n, zoom)
            if m == 0:
                continue
            t = (nv.c_int * m)()
            assert l.iunet_zoom_nearest_table(n, zoom, t, m) == 0
            assert np.array_equal(np.frombuffer(t, dtype=np.int32), want), (n, zoom)
    t = (nv.c_int * 4)()
    assert l.iunet_zoom_nearest_table(8, 0.5, t, 3) < 0 and b'n_out' in l.iunet_last_error()
    assert l.iunet_zoom_nearest_len(0, 0.5) == 0
