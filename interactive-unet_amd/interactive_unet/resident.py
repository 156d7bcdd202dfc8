"""What components.py, morphology.py, propose.py and geodesic.py check and compute alike: a uint8 volume or an int32 map on the device (a
CUDA tensor) or on the host (a numpy array), their small integer arguments, and the host path's class maps.  Every check raises ValueError before any GPU work."""
import numpy as np
import torch

MAX_VOXELS = 2 ** 31 - 1


def check_bytes(name, v, dev):
    """v is uint8 and contiguous, as a CUDA tensor (dev) or a numpy array."""
    if v.dtype != (torch.uint8 if dev else np.uint8):
        raise ValueError(f'{name} must be uint8, got {v.dtype}')
    if not (v.is_contiguous() if dev else v.flags['C_CONTIGUOUS']):
        raise ValueError(f'{name} must be contiguous')


def check_volume(src, max_sq=None):
    """Validated (on_device, Z, Y, X, C) of a class map [Z, Y, X] (C = 1) or a predicted volume [Z, Y, X, C], 2 <= C <= 16; max_sq: the
    largest squared diagonal the caller's int32 distances hold."""
    dev = torch.is_tensor(src)
    if not (dev or isinstance(src, np.ndarray)):
        raise ValueError('src must be a CUDA uint8 tensor or a numpy uint8 array')
    if dev and not src.is_cuda:
        raise ValueError('a resident volume must be a CUDA tensor (a host volume goes in as a numpy array)')
    check_bytes('src', src, dev)
    if src.ndim not in (3, 4) or min(src.shape) < 1 or (src.ndim == 4 and not 2 <= src.shape[3] <= 16):
        raise ValueError(f'src must be a class map [Z, Y, X] or a predicted volume [Z, Y, X, C] with 2 <= C <= 16, got {tuple(src.shape)}')
    Z, Y, X = (int(n) for n in src.shape[:3])
    if Z * Y * X > MAX_VOXELS:
        raise ValueError(f'volume {Z} x {Y} x {X}: more than 2^31 - 1 voxels')
    if max_sq is not None and (Z - 1) ** 2 + (Y - 1) ** 2 + (X - 1) ** 2 > max_sq:
        raise ValueError(f'volume {Z} x {Y} x {X}: its squared diagonal passes 2^31 - 2')
    return dev, Z, Y, X, (1 if src.ndim == 3 else int(src.shape[3]))


def check_map(m, name, beside=None):
    """Validated (on_device, Z, Y, X) of an int32 map [Z, Y, X]; beside = (on_device, Z, Y, X): on that side (device or host) and of that
    shape."""
    dev = torch.is_tensor(m)
    if not (dev or isinstance(m, np.ndarray)):
        raise ValueError(f'{name} must be a CUDA int32 tensor or a numpy int32 array')
    if dev and not m.is_cuda:
        raise ValueError(f'resident {name} must be a CUDA tensor (a host map goes in as a numpy array)')
    if beside is not None and dev != beside[0]:
        raise ValueError(f'{name} must be a CUDA tensor beside a resident volume, a numpy array beside a host volume')
    if m.dtype != (torch.int32 if dev else np.int32):
        raise ValueError(f'{name} must be int32, got {m.dtype}')
    if not (m.is_contiguous() if dev else m.flags['C_CONTIGUOUS']):
        raise ValueError(f'{name} must be contiguous')
    if m.ndim != 3 or min(m.shape) < 1:
        raise ValueError(f'{name} must be [Z, Y, X], got {tuple(m.shape)}')
    Z, Y, X = (int(n) for n in m.shape)
    if beside is not None and (Z, Y, X) != tuple(beside[1:]):
        raise ValueError(f'{name} must be {tuple(beside[1:])}, got {(Z, Y, X)}')
    if Z * Y * X > MAX_VOXELS:
        raise ValueError(f'volume {Z} x {Y} x {X}: more than 2^31 - 1 voxels')
    return dev, Z, Y, X


def is_int(value):
    return isinstance(value, (int, np.integer)) and not isinstance(value, bool)


def check_byte(value, name):
    if not is_int(value) or not 0 <= value <= 255:
        raise ValueError(f'{name} {value!r} outside 0 .. 255')
    return int(value)


def check_count(value, name, what='an int >= 0'):
    if not is_int(value) or value < 0:
        raise ValueError(f'{name} {value!r}: {what}')
    return int(value)


def host_maps(src):
    """(cls, has) of a numpy src: the class of every voxel (the first of equal bytes) and whether it was ever predicted (a byte above 0)."""
    if src.ndim == 3:
        return src.copy(), np.ones(src.shape, dtype=bool)
    return src.argmax(axis=-1).astype(np.uint8), src.max(axis=-1) > 0
