"""ctypes binding of libiunet.so (the C ABI declared in include/iunet.h).

The library is pure HIP (no torch types in its signatures): tensors cross the boundary
as raw device pointers + sizes + the HIP stream to order the work on.  There is NO CPU
fallback: if the shared library is missing or a call fails, this module raises.
"""
import ctypes
import os
import re

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('IUNET_LIB') or os.path.join(os.path.dirname(_HERE), 'lib', 'libiunet.so')   # IUNET_LIB: A/B builds

_lib = None
_sigs = None

c_void_p, c_int, c_ll, c_float = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong, ctypes.c_float


class NativeError(RuntimeError):
    pass


# ---- the bindings come from include/iunet.h, the one place a public signature is written.  C type (const dropped) -> ctypes:
_SCALAR = {'int': c_int, 'long long': c_ll, 'float': c_float, 'double': ctypes.c_double}
_POINTEE = ('int', 'long long', 'double')               # host arrays: POINTER(scalar)
_OPAQUE = ('void', 'iunet_net', 'iunet_train')          # T* crosses as a raw address, T** / T* const* as an array of them
# the header says `const int* tables`, but it is a DEVICE pointer: Python passes an address, not a host int array
_OVERRIDE = {('iunet_zoom_nearest_u8', 'tables'): c_void_p}
_PROTO = re.compile(r'([\w\s*]*?)\b(iunet_\w+)\s*\(([^()]*)\)\s*;')


def _ctype(spelled, ret=False):
    base, stars = ' '.join(re.sub(r'\bconst\b|\*', ' ', spelled).split()), spelled.count('*')
    if stars == 0:
        if ret and base == 'void':
            return None
        return c_void_p if base == 'iunet_train_hook' and not ret else _SCALAR[base]
    if base in _OPAQUE and stars <= 2:
        return c_void_p if stars == 1 else ctypes.POINTER(c_void_p)
    if stars == 1 and base == 'char':
        return ctypes.c_char_p
    if stars == 1 and base in _POINTEE and not ret:
        return ctypes.POINTER(_SCALAR[base])
    raise KeyError(spelled)


def parse_header(text):
    """{name: (restype, argtypes)} of every prototype of the header text (every parameter named, as include/iunet.h writes them).  A
    type the mapping above does not know raises NativeError with the function and the parameter: nothing is guessed."""
    text = re.sub(r'/\*.*?\*/|//[^\n]*', ' ', text, flags=re.S)
    text = re.sub(r'^[ \t]*#.*$', '', text, flags=re.M)
    sigs = {}
    for ret, name, params in _PROTO.findall(text):
        try:
            where = 'return type'
            restype, argtypes = _ctype(ret, ret=True), []
            for where in [' '.join(p.split()) for p in params.split(',') if p.split() not in ([], ['void'])]:
                spelled, pname = re.fullmatch(r'(.*?)(\w+)', where).groups()
                argtypes.append(_OVERRIDE.get((name, pname)) or _ctype(spelled))
        except (KeyError, AttributeError):
            raise NativeError(f'iunet.h: {name}: no ctypes mapping for `{where}`') from None
        sigs[name] = (restype, argtypes)
    return sigs


def signatures():
    """The parsed header, read once: $IUNET_HEADER, else the checkout's include/iunet.h, else the copy beside the library (overlay install)."""
    global _sigs
    if _sigs is None:
        found = [p for p in (os.path.join(_HERE, '..', '..', 'include', 'iunet.h'), os.path.join(_HERE, '..', 'lib', 'iunet.h')) if os.path.isfile(p)]
        path = os.environ.get('IUNET_HEADER') or (found[0] if found else None)
        if path is None or not os.path.isfile(path):
            raise NativeError(f'iunet.h is missing ({path or "include/iunet.h of the checkout, lib/iunet.h beside the library"}); IUNET_HEADER names another')
        _sigs = parse_header(open(path).read())
    return _sigs


def lib():
    """Load libiunet.so once; raise (never fall back) if it is not there."""
    global _lib
    if _lib is None:
        if not os.path.isfile(LIB_PATH):
            raise NativeError(f'{LIB_PATH} is missing: build it with __graft_entry__.build() '
                              f'(interactive-unet_amd/csrc/build.sh); there is no CPU fallback')
        l = ctypes.CDLL(LIB_PATH)
        for name, (restype, argtypes) in signatures().items():
            fn = getattr(l, name)          # AttributeError here = header/library mismatch
            fn.restype, fn.argtypes = restype, argtypes
        _lib = l
    return _lib


def exported_symbols():
    return list(signatures())


def check(status):
    if status != 0:
        raise NativeError(f'libiunet error {status}: {lib().iunet_last_error().decode()}')


def answer(value):
    """A non-negative answer of the library as it is; NativeError where it refused the arguments (negative)."""
    if value < 0:
        check(value)
    return value


def call(name, *args):
    check(getattr(lib(), name)(*args))


def pack_conv3_elems(cout, cin, taps, mode):
    return int(lib().iunet_pack_conv3_elems(cout, cin, taps, mode))


class PackDesc(ctypes.Structure):
    """One layer of iunet_pack_batch (mirror of csrc/pack_batch.hip: PackDesc)."""
    _fields_ = [('w', c_void_p), ('gamma', c_void_p), ('beta', c_void_p), ('mean', c_void_p), ('var', c_void_p),
                ('bias_out', c_void_p), ('dst', c_void_p), ('total', c_ll), ('Cout', c_int), ('Cin', c_int),
                ('taps', c_int), ('kind', c_int), ('dgrad', c_int), ('dtype', c_int), ('eps', c_float), ('pad_', c_int),
                ('qscale', c_void_p)]


def make_desc(w, dst, cout, cin, taps, kind, dtype, dgrad=0, bn=None, bias_out=None, eps=1e-5, qscale=None):
    if kind not in range(1, 7):
        raise NativeError(f'pack descriptor kind {kind}: the kinds are 1 .. 6 (csrc/pack_desc.h)')
    d = PackDesc()
    d.w, d.dst, d.total = w.data_ptr(), dst.data_ptr(), dst.numel()
    d.Cout, d.Cin, d.taps, d.kind, d.dgrad, d.dtype, d.eps = cout, cin, taps, kind, int(dgrad), DTYPE_CODE[dtype], eps
    if bn is not None:
        d.gamma, d.beta, d.mean, d.var = [t.data_ptr() for t in bn]
        d.bias_out = None if bias_out is None else bias_out.data_ptr()
    d.qscale = None if qscale is None else qscale.data_ptr()
    return d


class PackTable:
    """Descriptor table of iunet_pack_batch in device memory; `sources` keeps the tensors whose addresses it holds."""

    def __init__(self, descs, device, sources=()):
        assert lib().iunet_pack_desc_bytes() == ctypes.sizeof(PackDesc), 'PackDesc layout mismatch with libiunet'
        arr = (PackDesc * len(descs))(*descs)
        host = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8)
        self.dev = host.to(device)
        self.n = len(descs)
        self.sources = list(sources)
        self.quant_max_cout = max([d.Cout for d in descs if d.qscale] + [0])

    def run(self):
        call('iunet_pack_batch', ptr(self.dev), self.n, self.quant_max_cout, stream())


class X2PrepDesc(ctypes.Structure):
    """One operator of iunet_x2_prep_batch / iunet_x2m_prep_batch (mirror of csrc/x2_prep_desc.h)."""
    _fields_ = [('w', c_void_p), ('out', c_void_p), ('w8', c_void_p), ('oscale', c_void_p), ('bias_out', c_void_p), ('gamma', c_void_p),
                ('beta', c_void_p), ('mean', c_void_p), ('var', c_void_p), ('bias_in', c_void_p), ('eps', c_float), ('act_in', c_float),
                ('act_out', c_float), ('Cout', c_int), ('Cin', c_int), ('taps', c_int), ('kind', c_int), ('kc', c_int), ('row0', c_int)]


def make_x2_prep_desc(w, out, oscale, bias_out, cout, cin, taps, kind, kc, act_in, act_out, bn=None, bias_in=None, w8=None, eps=1e-5):
    d = X2PrepDesc()
    d.w, d.out, d.oscale, d.bias_out = w.data_ptr(), out.data_ptr(), oscale.data_ptr(), bias_out.data_ptr()
    d.w8 = None if w8 is None else w8.data_ptr()
    if bn is not None:
        d.gamma, d.beta, d.mean, d.var = [t.data_ptr() for t in bn]
    d.bias_in = None if bias_in is None else bias_in.data_ptr()
    d.eps, d.act_in, d.act_out = eps, act_in, act_out
    d.Cout, d.Cin, d.taps, d.kind, d.kc = cout, cin, taps, kind, kc
    return d


class X2PrepTable:
    """Descriptor table of iunet_x2_prep_batch (x2m=False) / iunet_x2m_prep_batch (x2m=True) in device memory."""

    def __init__(self, descs, device, x2m):
        assert lib().iunet_x2_prep_desc_bytes() == ctypes.sizeof(X2PrepDesc), 'X2PrepDesc layout mismatch with libiunet'
        rows = 0
        for d in descs:
            d.row0 = rows
            rows += d.Cout
        arr = (X2PrepDesc * len(descs))(*descs)
        self.dev = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(device)
        self.n, self.rows = len(descs), rows
        self.fn = 'iunet_x2m_prep_batch' if x2m else 'iunet_x2_prep_batch'

    def run(self):
        call(self.fn, ptr(self.dev), self.n, self.rows, stream())


class PackedConv:
    """A stage conv's weights in the fragment orders its launches may need: the padded K16 order (layout 2) always, the compact one
    (layout 3) where iunet_conv3_packs_compact says a launch can use it.  `dgrad`: the data-gradient operator (roles of cin / cout
    swapped).  The only place on the Python side that knows which operators are packed and which launch gets which (the rules
    themselves: csrc/capi.hip, iunet_conv3_plan)."""
    MODE = {2: 2, 3: 6}          # layout -> iunet_pack_conv3 mode
    KIND = {2: 1, 3: 6}          # layout -> iunet_pack_batch descriptor kind

    def __init__(self, cout, cin, taps, dtype, device, dgrad=False):
        self.cout, self.cin, self.taps, self.dg = cout, cin, taps, int(bool(dgrad))
        self.out_ch, self.in_ch = (cin, cout) if dgrad else (cout, cin)
        self.dt = DTYPE_CODE[dtype]
        lays = (2, 3) if answer(lib().iunet_conv3_packs_compact(taps, self.in_ch)) else (2,)
        self.buf = {lay: torch.empty(pack_conv3_elems(cout, cin, taps, self.MODE[lay] | self.dg), dtype=dtype, device=device) for lay in lays}
        self._plans = {}

    def pack(self, w, scale=None):
        for lay, b in self.buf.items():
            call('iunet_pack_conv3', self.dt, ptr(w), ptr(scale), ptr(b), self.cout, self.cin, self.taps, self.MODE[lay] | self.dg, stream())

    def descs(self, w, bn=None, bias_out=None, eps=1e-5, qscale=None):
        """Descriptors of all layouts for iunet_pack_batch (the first one also writes the folded bias)."""
        return [make_desc(w, b, self.cout, self.cin, self.taps, self.KIND[lay], b.dtype, self.dg, bn, bias_out if k == 0 else None, eps, qscale)
                for k, (lay, b) in enumerate(sorted(self.buf.items(), reverse=True))]

    def pick(self, nd, N, D, H, W, act=False, bw=False):
        """(layout, buffer, fused) of a launch on this grid.  act: the launch wants a fused input activation (iunet_conv3_fwd_act);
        bw: it wants to accumulate the BatchNorm- / GroupNorm-backward sums (iunet_conv3_dgrad_bnstats_lay / _sample_bnstats).  fused:
        the launch has what was asked for; False (where something was asked for): it runs plain, the caller applies the activation /
        reduces the sums in a pass of its own."""
        key = (nd, N, D, H, W, bool(act), bool(bw))
        plan = self._plans.get(key)          # the answer depends on the key alone: a step asks the library once per shape, not per launch
        if plan is None:
            fused = c_int(0)
            lay = answer(lib().iunet_conv3_plan(nd, N, D, H, W, self.in_ch, self.out_ch, int(key[5]), int(key[6]), int(3 in self.buf), ctypes.byref(fused)))
            plan = self._plans[key] = (lay, self.buf[lay], bool(fused.value))
        return plan


def ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def ll_array(vals):
    return (c_ll * len(vals))(*[int(v) for v in vals])


def int_array(vals):
    return (c_int * len(vals))(*[int(v) for v in vals])


DTYPE_CODE = {torch.float16: 0, torch.bfloat16: 1}
IN_DTYPE_CODE = {torch.float32: 0, torch.float16: 1, torch.uint8: 2, torch.bfloat16: 3}


def ptr_array(vals):
    """A C array of pointers (tensors, raw addresses or None) for the `const void* const*` arguments."""
    return (c_void_p * len(vals))(*[None if v is None else (v.data_ptr() if hasattr(v, 'data_ptr') else int(v)) for v in vals])
