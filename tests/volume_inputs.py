"""Inputs the tests of the resident-volume kernels share (slab, propose, tta, components, morphology, volume scale): written once, so a
seed names the same bytes in every file."""
import numpy as np


def random_pred(shape, C, seed):
    """A predicted volume uint8 [*shape, C]: random bytes, about a tenth of the voxels all-zero and a tenth with a tie at the top."""
    rng = np.random.default_rng(seed)
    pred = rng.integers(0, 256, tuple(shape) + (C,), dtype=np.uint8)
    pick = rng.random(shape)
    pred[pick < 0.1] = 0
    tie = (pick >= 0.1) & (pick < 0.2)
    top = pred.max(axis=-1)
    ch = rng.integers(0, C, shape)
    for c in range(C):
        pred[..., c] = np.where(tie & ((ch == c) | (ch == (c + 1) % C)), top, pred[..., c])
    return pred


def random_slicer(shape, seed):
    """A Slicer of the volume `shape` at a random orientation, its origin within a voxel of the volume's centre."""
    from interactive_unet.slicer import Slicer
    np.random.seed(seed)
    s = Slicer(list(shape))
    s.randomize()
    s.origin = np.array(shape) / 2 + np.random.uniform(-1, 1, 3)
    return s


def offset_copy(a, by):
    """A copy of the device tensor a that starts `by` bytes behind the (16-byte aligned) start of an allocation of its own."""
    import torch
    n = by // a.element_size()
    view = torch.empty(a.numel() + n, dtype=a.dtype, device=a.device)[n:].view(a.shape).copy_(a)
    assert view.data_ptr() % 16 == by
    return view
