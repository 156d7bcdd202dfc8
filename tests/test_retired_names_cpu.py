"""The 3^d stage conv keeps one forward kernel (conv3_v4.hip, layouts 2 / 3) and one weight-gradient form per dimension.  The kernels it
had before, and the environment switches that chose between them and their successors, are gone; this test reads source text only and
keeps them from coming back through a copied snippet.  (The names are spelled in pieces so that this file does not name them.)"""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SWITCHES = ['IUNET_' + s for s in ('CONV_' + 'V1', 'CONV_' + 'V2_ALL', 'CONV_' + 'V3', 'V2_' + 'DBG', 'WGRAD_' + 'V1', 'WGRAD2D_' + 'V1',
                                   'NO_' + 'COMPACT2D', 'NO_' + 'COMPACT2D_BW', 'NO_' + 'COMPACT')]
KERNELS = ['conv3_' + 'mfma_kernel', 'conv3_' + 'v2_kernel', 'conv3_' + 'wgrad_kernel']
# what went with them: source files, launchers, parameter structs, the layout-0 pack kernel, the selection helpers
OTHER = ['conv3_' + 'mfma.hip', 'conv3_' + 'v2.hip', 'iunet_conv3_' + 'v2_launch', 'pack_' + 'conv3_kernel', 'launch_' + 'conv3', 'launch_' + 'v2',
         'launch_' + 'wgrad', 'Conv3' + 'Params', 'ConvV2' + 'Params', 'Wgrad' + 'Params', 'Tile' + '2', 'W' + 'Tile', 'wgrad_' + 'use_v2',
         'iunet_conv3_' + 'mi', 'iunet_conv3_' + 'pick']
NAMES = SWITCHES + KERNELS + OTHER
# whole identifiers only: a longer identifier that contains one (the first conv's weight-gradient parameters, the exported
# layout query) is another, living name
RETIRED = re.compile(r'(?<![A-Za-z0-9_])(?:' + '|'.join(re.escape(n) for n in sorted(NAMES, key=len, reverse=True)) + r')(?![A-Za-z0-9_])')
TEXT = ('.py', '.hip', '.h', '.inc', '.sh', '.md', '.txt', '.cpp', '.c', '.json', '.cfg', '.toml')


def test_the_pattern_matches_every_retired_name():
    """A slip in the pattern must not pass silently: each name is found alone, as a template instantiation, in a call, in a getenv
    string and in a shell assignment; the living names that contain one are not."""
    assert len(SWITCHES) == 9 and len(KERNELS) == 3
    for n in NAMES:
        for text in (n, f'{n}<T, 3>(p)', f'({n})', f'getenv("{n}")', f'{n}=1 python', f'`{n}`', f'x = {n};'):
            m = RETIRED.search(text)
            assert m and m.group(0) == n, (n, text)
    for alive in ('First' + 'Wgrad' + 'Params', 'iunet_conv3_' + 'pick' + '_layout', 'conv3_' + 'wgrad_v2_kernel', 'pack_' + 'conv3_k16_kernel',
                  'conv3_' + 'v4_kernel', 'launch_' + 'conv3x'):
        assert not RETIRED.search(alive), alive


def test_no_source_names_a_retired_conv_kernel_or_switch():
    hits, seen = [], 0
    for top in ('interactive-unet_amd', 'tests', 'tools'):
        for base, dirs, files in os.walk(os.path.join(ROOT, top)):
            dirs[:] = [d for d in dirs if d not in ('__pycache__', 'obj', 'lib', 'golden')]
            for f in files:
                if not f.endswith(TEXT):
                    continue
                path = os.path.join(base, f)
                seen += 1
                for i, line in enumerate(open(path, errors='replace'), 1):
                    m = RETIRED.search(line)
                    if m:
                        hits.append(f'{os.path.relpath(path, ROOT)}:{i}: {m.group(0)}')
    assert seen > 100, seen
    assert not hits, '\n'.join(hits)
