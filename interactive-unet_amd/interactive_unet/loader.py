"""Drop-in for interactive_unet/loader.py ("Batch producer"): `load_annotations`,
`get_data_loader`, `UNetDataset` with the reference's names and arguments.  The annotations stay uint8 and live on the GPU;
every batch -- normalisation (loader.py:32-42), RandomHorizontalFlip / RandomVerticalFlip / RandomRotation(NEAREST) /
RandomResizedCrop((512, 512), NEAREST) (loader.py:125-133) and the float16 conversion (loader.py:150-152) -- is ONE gather
launch (libiunet: iunet_augment_batch).  The random parameters are drawn on the host from torch's generator in the order
torchvision's v2 transforms draw them (flip, flip, angle, crop box); the reference runs the same chain per sample on the CPU
with num_workers=0 (loader.py:95-99).  The three transforms the reference's authors switch on and off (loader.py:115-123:
ElasticTransform, ColorJitter, RandomChoice([GaussianBlur(5), GaussianNoise()])) are keywords of `UNetDataset` / `get_data_loader`,
off by default; switched on, `draw_extra` draws their parameters after each sample's four and the batch goes through
iunet_augment_batch_extra's short pipeline instead, still without a copy to the host.

File reading (TIFF / PNG through PIL) and `colored_to_categorical` are caller-side format code; `annotations_from_arrays`
takes arrays directly.  `reslice=True` (load_resliced_annotations, dead code in the reference: trainer.py:18) is not provided.

The 3-D producer is the 3-D form of VolumeData.sample + load_resliced_annotations (volumedata.py:68-80,
loader.py:48-82) for the dim = 3 network: `load_volume_annotations` / `volume_annotations_from_arrays` keep the image, mask and
weight VOLUMES as uint8 on the GPU, `VolumeDataset` draws random oblique patches around annotated voxels (`patch_candidates`,
`draw_patch_params`) and every batch -- image at spline order 1, mask and weight at order 0, one-hot, dark rule, fp16 -- is ONE
gather launch (libiunet: iunet_patch_batch).  `get_volume_loader` wraps it in the same `DeviceLoader`.  The same three further
transforms are keywords of `VolumeDataset` / `get_volume_loader`, off by default: switched on, `draw_extra`
draws their parameters after each sample's `draw()` and the batch goes through iunet_patch_batch_extra's pipeline -- the elastic
displacement is added to the patch coordinate before the one gather, the intensity transforms follow it -- without a copy to the host.
"""
import ctypes
import functools
import glob
import math
import os

import numpy as np
import torch

from . import _native as nv

OUT_SIZE = 512                      # RandomResizedCrop(size=(512, 512)) ignores input_size (loader.py:128)
COLORS = np.array([[0, 0, 0], [230, 25, 75], [60, 180, 75], [255, 225, 25], [0, 130, 200], [245, 130, 48], [145, 30, 180],
                   [70, 240, 240], [240, 50, 230], [210, 245, 60], [170, 255, 195]], dtype=np.uint8)      # utils.py:304-306


class AugDesc(ctypes.Structure):
    """Mirror of csrc/augment.hip: AugDesc."""
    _fields_ = [('image', ctypes.c_void_p), ('mask', ctypes.c_void_p), ('weight', ctypes.c_void_p), ('xg', ctypes.c_void_p),
                ('yg', ctypes.c_void_p), ('H', ctypes.c_int), ('W', ctypes.c_int), ('hflip', ctypes.c_int), ('vflip', ctypes.c_int),
                ('kind', ctypes.c_int), ('ci', ctypes.c_int), ('cj', ctypes.c_int), ('ch', ctypes.c_int), ('cw', ctypes.c_int),
                ('r', ctypes.c_float * 6), ('keep_dark', ctypes.c_int)]


USE_ELASTIC, USE_JITTER, USE_BLUR, USE_NOISE = 1, 2, 4, 8      # iunet_augment_batch_extra's `use` bits; AugExtraDesc.flags has the first two


def _extra_fields(blur_name, blur_len):
    """The fields of the two producers' extended descriptors: the same around the blur coefficients."""
    return [('flags', ctypes.c_int), ('kind', ctypes.c_int), ('ekey', ctypes.c_uint * 2), ('a2', ctypes.c_float),
            ('brightness', ctypes.c_float), ('contrast', ctypes.c_float), ('contrast_first', ctypes.c_int),
            (blur_name, ctypes.c_float * blur_len), ('nkey', ctypes.c_uint * 2), ('sigma_n', ctypes.c_float)]


class AugExtraDesc(ctypes.Structure):
    """Mirror of csrc/augment.hip: AugExtraDesc (36 four-byte fields, no padding)."""
    _fields_ = _extra_fields('w2', 25)


def colored_to_categorical(colored_mask):
    """utils.py:308-349: one-hot x 255 over the palette colours present in the mask (first match), background channel split
    off as weight = 255 - background."""
    flat = colored_mask.reshape(-1, 3).astype(np.uint32)
    keys = flat[:, 0] << 16 | flat[:, 1] << 8 | flat[:, 2]
    ckeys = COLORS[:, 0].astype(np.uint32) << 16 | COLORS[:, 1].astype(np.uint32) << 8 | COLORS[:, 2]
    present = ckeys[np.isin(ckeys, keys)]
    mask = np.zeros(colored_mask.shape[:2] + (len(present),), dtype=np.uint8)
    todo = np.ones(len(keys), bool)
    for k, key in enumerate(present):
        hit = todo & (keys == key)
        mask.reshape(-1, len(present))[hit, k] = 255
        todo &= ~hit
    return mask[:, :, 1:], 255 - mask[:, :, 0]


def _imread(path):
    from PIL import Image
    return np.asarray(Image.open(path))


def annotations_from_arrays(samples, device='cuda'):
    """samples: iterable of (image uint8 [H, W] or [H, W, ch], mask uint8 [H, W, C] one-hot x 255, weight uint8 [H, W]).
    Returns the annotation list the dataset works on: uint8 tensors resident on the GPU (normalisation happens in the batch
    kernel, so nothing is expanded to float32 here as loader.py:37-39 does)."""
    out = []
    for image, mask, weight in samples:
        image = np.asarray(image)
        image = image[:, :, None] if image.ndim == 2 else image
        t = [torch.from_numpy(np.array(a, dtype=np.uint8, order='C')).to(device) for a in (image, mask, weight)]
        if t[1].shape[:2] != t[0].shape[:2] or t[2].shape != t[0].shape[:2]:
            raise ValueError(f'annotation shapes differ: image {tuple(t[0].shape)}, mask {tuple(t[1].shape)}, weight {tuple(t[2].shape)}')
        out.append(t)
    return out


def load_annotations(set_type='train', device='cuda'):
    """loader.py:15-46: data/{train,val}/{images,masks,weights}/* in sorted order."""
    folder = os.path.join('data', 'train' if set_type == 'train' else 'val')
    names = [np.sort(glob.glob(os.path.join(folder, sub, '*'))) for sub in ('images', 'masks', 'weights')]
    samples = []
    for fi, fm, fw in zip(*names):
        mask, _ = colored_to_categorical(_imread(fm))
        samples.append((_imread(fi), mask, _imread(fw)))
    return annotations_from_arrays(samples, device)


# ---- random parameters, in the order torchvision's v2 transforms draw them ------------------------------------------------
def _uniform(a, b, gen):
    return torch.empty(1).uniform_(a, b, generator=gen).item()


def resized_crop_params(H, W, gen, scale=(0.3, 1.0), ratio=(3.0 / 4.0, 4.0 / 3.0)):
    """RandomResizedCrop.make_params: (top, left, height, width)."""
    area = H * W
    log_ratio = (math.log(ratio[0]), math.log(ratio[1]))
    for _ in range(10):
        target_area = area * _uniform(scale[0], scale[1], gen)
        aspect_ratio = math.exp(_uniform(log_ratio[0], log_ratio[1], gen))
        w = int(round(math.sqrt(target_area * aspect_ratio)))
        h = int(round(math.sqrt(target_area / aspect_ratio)))
        if 0 < w <= W and 0 < h <= H:
            i = torch.randint(0, H - h + 1, size=(1,), generator=gen).item()
            j = torch.randint(0, W - w + 1, size=(1,), generator=gen).item()
            return i, j, h, w
    in_ratio = float(W) / float(H)
    if in_ratio < min(ratio):
        w = W
        h = int(round(w / min(ratio)))
    elif in_ratio > max(ratio):
        h = H
        w = int(round(h * max(ratio)))
    else:
        w, h = W, H
    return (H - h) // 2, (W - w) // 2, h, w


def draw_params(H, W, gen=None):
    """One sample's (hflip, vflip, angle, crop) for the chain of loader.py:125-129."""
    hflip = bool(torch.rand(1, generator=gen).item() < 0.5)
    vflip = bool(torch.rand(1, generator=gen).item() < 0.5)
    angle = _uniform(-360.0, 360.0, gen)
    return hflip, vflip, angle, resized_crop_params(H, W, gen)


def _key(gen):
    """A 64-bit Philox key: one randint(0, 2^32, (2,)), low word first."""
    lo, hi = torch.randint(0, 2 ** 32, (2,), generator=gen).tolist()
    return lo | hi << 32


def draw_extra(gen=None, elastic=False, color_jitter=False, blur_or_noise=False, elastic_alpha=50.0, noise_sigma=0.1):
    """One sample's parameters of the three further transforms of loader.py:115-123, drawn after the four
    draws of `draw_params`, each transform only where it is switched on: elastic: the key; color_jitter: rand < 0.5 -> contrast
    first, brightness ~ U(0.75, 1.25), contrast ~ U(0.5, 2.0); blur_or_noise: randint(0, 2): 0 blur, then sigma ~ U(0.1, 2.0);
    1 noise, then the key.  Returns the dict `UNetDataset.batch(extra=...)` takes per sample (a missing entry = off); with
    everything off nothing is drawn."""
    extra = {}
    if elastic:
        extra['elastic'] = {'key': _key(gen), 'alpha': float(elastic_alpha)}
    if color_jitter:
        contrast_first = bool(torch.rand(1, generator=gen).item() < 0.5)
        brightness = _uniform(0.75, 1.25, gen)
        extra['color_jitter'] = {'brightness': brightness, 'contrast': _uniform(0.5, 2.0, gen), 'contrast_first': contrast_first}
    if blur_or_noise:
        if torch.randint(0, 2, (1,), generator=gen).item() == 0:
            extra['blur_or_noise'] = {'kind': 'blur', 'sigma': _uniform(0.1, 2.0, gen)}
        else:
            extra['blur_or_noise'] = {'kind': 'noise', 'key': _key(gen), 'sigma': float(noise_sigma)}
    return extra


def gaussian_taps(sigma, K=None):
    """The normalised Gaussian taps, float64 rounded to float32; K = int(8 sigma + 1) made odd unless given."""
    if K is None:
        K = int(8 * sigma + 1)
        K += 1 - K % 2
    x = np.arange(K, dtype=np.float64) - (K - 1) / 2
    g = np.exp(-0.5 * (x / float(sigma)) ** 2)
    return (g / g.sum()).astype(np.float32)


def _fill_shared(d, extra, write_blur):
    """One extended descriptor (AugExtraDesc, PatchExtraDesc) from a sample's dict; `write_blur(d, k)` stores the blur's
    coefficients from its five taps k.  Returns the sample's `use` bits."""
    use = 0
    if 'elastic' in extra:
        e = extra['elastic']
        d.flags |= USE_ELASTIC
        d.ekey[0], d.ekey[1] = int(e['key']) & 0xFFFFFFFF, (int(e['key']) >> 32) & 0xFFFFFFFF
        d.a2 = float(e['alpha']) / 2
        use |= USE_ELASTIC
    if 'color_jitter' in extra:
        cj = extra['color_jitter']
        d.flags |= USE_JITTER
        d.brightness, d.contrast, d.contrast_first = float(cj['brightness']), float(cj['contrast']), int(bool(cj['contrast_first']))
        use |= USE_JITTER
    bn = extra.get('blur_or_noise')
    if bn is not None:
        if bn['kind'] == 'blur':
            d.kind = 1
            write_blur(d, gaussian_taps(bn['sigma'], 5))
            use |= USE_BLUR
        elif bn['kind'] == 'noise':
            d.kind = 2
            d.nkey[0], d.nkey[1] = int(bn['key']) & 0xFFFFFFFF, (int(bn['key']) >> 32) & 0xFFFFFFFF
            d.sigma_n = float(bn['sigma'])
            use |= USE_NOISE
        else:
            raise ValueError(f"blur_or_noise kind {bn['kind']!r}: 'blur' or 'noise'")
    return use


def _aug_blur(d, k):
    d.w2[:] = (k[:, None] * k[None, :]).reshape(-1).tolist()          # float32 products


_fill_extra = functools.partial(_fill_shared, write_blur=_aug_blur)      # (d, extra): one AugExtraDesc from a sample's dict -> its `use` bits


def _upload_extras(ds, descs, extra, desc_type, fill, size_fn, ws_fn, ws_args, dev):
    """The tail both datasets' `batch` share on the extended path: the per-sample dicts `extra` into `desc_type` descriptors by
    `fill`, the layout checked against the library's `size_fn()`, the elastic taps and the workspace (`ws_fn(*ws_args)` bytes) from
    the caches on `ds`, and ONE upload of `descs` with the new descriptors behind them (both are multiples of 8 bytes).
    Returns (the uploaded buffer, the pointer to its second part, the batch's `use` bits, taps, workspace)."""
    B = len(descs)
    extra = list(extra)
    if len(extra) != B:
        raise ValueError(f'extra: {len(extra)} entries for a batch of {B}')
    extras = (desc_type * B)()
    use = 0
    for d, e in zip(extras, extra):
        use |= fill(d, e or {})
    assert size_fn() == ctypes.sizeof(desc_type), f'{desc_type.__name__} layout mismatch with libiunet'
    if ds._taps is None or ds._taps[0] != (ds.elastic_sigma, dev):
        ds._taps = ((ds.elastic_sigma, dev), torch.from_numpy(gaussian_taps(ds.elastic_sigma)).to(dev))
    need = nv.answer(ws_fn(*ws_args))
    if ds._ws is None or ds._ws.device != dev or ds._ws.numel() < need:
        ds._ws = torch.empty(need, dtype=torch.uint8, device=dev)
    raw = torch.frombuffer(bytearray(bytes(descs) + bytes(extras)), dtype=torch.uint8).to(dev)
    return raw, ctypes.c_void_p(raw.data_ptr() + ctypes.sizeof(descs)), use, ds._taps[1], ds._ws


def _rotation(angle, H, W):
    """(kind, r[6]) of torchvision's rotate(angle, NEAREST, expand=False, center=None): the fast paths for multiples of 90
    degrees, else theta^T / (W/2, H/2) of the inverse rotation about the centre, formed in float32 as _affine_grid does."""
    a = angle % 360
    if a == 0:
        return 1, [0.0] * 6
    if a == 180:
        return 2, [0.0] * 6
    if H == W and a in (90, 270):
        return (3 if a == 90 else 4), [0.0] * 6
    rot = math.radians(-angle)
    m = [math.cos(rot), math.sin(rot), 0.0, -math.sin(rot), math.cos(rot), 0.0]           # [d, -b, 0, -c, a, 0] of the inverse matrix
    theta = torch.tensor(m, dtype=torch.float32).reshape(1, 2, 3)
    r = theta.transpose(1, 2).div(torch.tensor([0.5 * W, 0.5 * H], dtype=torch.float32))[0]     # [3][2]
    return 0, [float(r[0, 0]), float(r[1, 0]), float(r[2, 0]), float(r[0, 1]), float(r[1, 1]), float(r[2, 1])]


class UNetDataset:
    """loader.py:103-154.  `annotations`: the list from load_annotations / annotations_from_arrays."""

    def __init__(self, annotations, resliced_annotations=None, reslice=False, reslice_factor=2, augment=False, generator=None,
                 out_size=OUT_SIZE, keep_dark=False, elastic=False, color_jitter=False, blur_or_noise=False, elastic_alpha=50.0,
                 elastic_sigma=5.0, noise_sigma=0.1):
        if reslice:
            raise NotImplementedError('reslice=True (load_resliced_annotations) is not provided; the reference never enables it')
        if (elastic or color_jitter or blur_or_noise) and not augment:
            raise ValueError('elastic / color_jitter / blur_or_noise are augmentations: they need augment=True')
        self.annotations = annotations
        self.resliced_annotations = resliced_annotations
        self.reslice, self.reslice_factor, self.augment = reslice, reslice_factor, augment
        self.generator = generator
        # out_size: the augmented output (the reference's loader: 512 x 512 always); keep_dark: do not zero mask / weight where
        # the image is 0 (the Suggestor's tensors, suggestor.py:60-65, carry no such masking)
        self.out_size = (out_size, out_size) if isinstance(out_size, int) else tuple(out_size)
        self.keep_dark = bool(keep_dark)
        # the three further transforms of loader.py:115-123, off by default: nothing more is drawn or launched
        self.elastic, self.color_jitter, self.blur_or_noise = bool(elastic), bool(color_jitter), bool(blur_or_noise)
        self.elastic_alpha, self.elastic_sigma, self.noise_sigma = float(elastic_alpha), float(elastic_sigma), float(noise_sigma)
        self._grids, self._lut = {}, None
        self._lut32 = self._taps = self._ws = None

    def __len__(self):
        return len(self.annotations)

    def _grid(self, n, device):
        key = (n, str(device))
        if key not in self._grids:
            self._grids[key] = torch.linspace((1.0 - n) * 0.5, (n - 1.0) * 0.5, steps=n).to(device)
        return self._grids[key]

    def batch(self, indices, params=None, extra=None):
        """The batch loader.py's DataLoader would collate from __getitem__(i) for i in indices.  `params`: optional list of
        (hflip, vflip, angle, crop) per sample (drawn from the generator when None).  `extra`: optional list, per sample, of the
        dict `draw_extra` returns ('elastic': {key, alpha}, 'color_jitter': {brightness, contrast, contrast_first},
        'blur_or_noise': {kind: 'blur', sigma} or {kind: 'noise', key, sigma}; a missing entry = off), drawn after each sample's
        `params` when None and a transform is switched on.  With the three transforms off and no `extra` the batch is ONE gather
        launch (iunet_augment_batch); else the pipeline of iunet_augment_batch_extra."""
        ann = [self.annotations[i] for i in indices]
        dev = ann[0][0].device
        ch, C = int(ann[0][0].shape[2]), int(ann[0][1].shape[2])
        extras_on = self.elastic or self.color_jitter or self.blur_or_noise
        if extra is not None and not self.augment:
            raise ValueError('extra: the further transforms need augment=True')
        if self.augment:
            OH, OW = self.out_size
        else:
            OH, OW = int(ann[0][0].shape[0]), int(ann[0][0].shape[1])
        descs = (AugDesc * len(ann))()
        drawn = []
        for k, (image, mask, weight) in enumerate(ann):
            H, W = int(image.shape[0]), int(image.shape[1])
            if int(image.shape[2]) != ch or int(mask.shape[2]) != C or (not self.augment and (H, W) != (OH, OW)):
                raise RuntimeError('stack expects each tensor to be equal size')      # what default_collate raises in the reference
            if self.augment:
                hflip, vflip, angle, crop = params[k] if params is not None else draw_params(H, W, self.generator)
                kind, r = _rotation(angle, H, W)
                if extra is None and extras_on:
                    drawn.append(draw_extra(self.generator, self.elastic, self.color_jitter, self.blur_or_noise, self.elastic_alpha,
                                            self.noise_sigma))
            else:
                hflip, vflip, kind, r, crop = False, False, 1, [0.0] * 6, (0, 0, H, W)
            d = descs[k]
            d.image, d.mask, d.weight = image.data_ptr(), mask.data_ptr(), weight.data_ptr()
            d.xg, d.yg = self._grid(W, dev).data_ptr(), self._grid(H, dev).data_ptr()
            d.H, d.W, d.hflip, d.vflip, d.kind = H, W, int(hflip), int(vflip), kind
            d.ci, d.cj, d.ch, d.cw = [int(v) for v in crop]
            d.keep_dark = int(self.keep_dark)
            for q in range(6):
                d.r[q] = r[q]
        if self._lut is None or self._lut.device != dev:
            self._lut = torch.from_numpy((np.arange(256) / 255).astype('float32')).to(torch.float16).to(dev)   # loader.py:37-39, :150
        B = len(ann)
        X = torch.empty((B, ch, OH, OW), dtype=torch.float16, device=dev)
        y = torch.empty((B, C, OH, OW), dtype=torch.float16, device=dev)
        w = torch.empty((B, C, OH, OW), dtype=torch.float16, device=dev)
        if extra is None and not drawn:
            raw = torch.frombuffer(bytearray(bytes(descs)), dtype=torch.uint8).to(dev)
            with torch.cuda.device(dev):
                nv.call('iunet_augment_batch', nv.ptr(raw), B, ch, C, OH, OW, nv.ptr(self._lut), nv.ptr(X), nv.ptr(y), nv.ptr(w), nv.stream())
            return X, y, w
        raw, extras, use, taps, ws = _upload_extras(self, descs, drawn if extra is None else extra, AugExtraDesc, _fill_extra,
                                                    nv.lib().iunet_augment_extra_desc_bytes, nv.lib().iunet_augment_extra_ws_bytes,
                                                    (B, ch, OH, OW), dev)
        if self._lut32 is None or self._lut32.device != dev:
            self._lut32 = torch.from_numpy((np.arange(256) / 255).astype('float32')).to(dev)
        with torch.cuda.device(dev):
            nv.call('iunet_augment_batch_extra', nv.ptr(raw), extras, use, B, ch, C, OH, OW,
                    nv.ptr(self._lut), nv.ptr(self._lut32), nv.ptr(taps), int(taps.numel()), nv.ptr(ws),
                    int(ws.numel()), nv.ptr(X), nv.ptr(y), nv.ptr(w), nv.stream())
        return X, y, w

    def __getitem__(self, idx):
        X, y, w = self.batch([idx])
        return X[0], y[0], w[0]


class DeviceLoader:
    """What DataLoader(dataset, batch_size, shuffle, num_workers=0) yields (loader.py:95-99), produced on the device."""

    def __init__(self, dataset, batch_size=1, shuffle=False, generator=None):
        self.dataset, self.batch_size, self.shuffle, self.generator = dataset, int(batch_size), shuffle, generator

    def __len__(self):
        return -(-len(self.dataset) // self.batch_size)

    def __iter__(self):
        n = len(self.dataset)
        order = torch.randperm(n, generator=self.generator).tolist() if self.shuffle else list(range(n))
        for s in range(0, n, self.batch_size):
            yield self.dataset.batch(order[s:s + self.batch_size])


def get_data_loader(set_type='train', num_classes=2, batch_size=2, reslice=False, reslice_factor=2, augment=True, shuffle=True,
                    annotations=None, generator=None, elastic=False, color_jitter=False, blur_or_noise=False):
    """loader.py:84-101 (`annotations`: skip the file read and use these; elastic / color_jitter / blur_or_noise: the three
    transforms of loader.py:115-123 the reference's authors switch on and off, at its parameters)."""
    if annotations is None:
        annotations = load_annotations(set_type=set_type)
    dataset = UNetDataset(annotations, None, reslice=reslice, reslice_factor=reslice_factor, augment=augment, generator=generator,
                          elastic=elastic, color_jitter=color_jitter, blur_or_noise=blur_or_noise)
    return DeviceLoader(dataset, batch_size=batch_size, shuffle=shuffle, generator=generator)


# ---- the 3-D producer: random oblique patches of annotation volumes ----------------------------------
class PatchDesc(ctypes.Structure):
    """Mirror of csrc/patch_gather.h: PatchDesc."""
    _fields_ = [('image', ctypes.c_void_p), ('mask', ctypes.c_void_p), ('weight', ctypes.c_void_p), ('wstride', ctypes.c_int),
                ('Z', ctypes.c_int), ('Y', ctypes.c_int), ('X', ctypes.c_int), ('m', ctypes.c_float * 9), ('c', ctypes.c_float * 3),
                ('keep_dark', ctypes.c_int)]


class PatchExtraDesc(ctypes.Structure):
    """Mirror of csrc/patch_augment.hip: PatchExtraDesc (16 four-byte fields, no padding)."""
    _fields_ = _extra_fields('taps', 5)


def _patch_blur(d, k):
    d.taps[:] = k.tolist()


_fill_patch_extra = functools.partial(_fill_shared, write_blur=_patch_blur)      # (d, extra): one PatchExtraDesc from a sample's dict -> its `use` bits


def volume_annotations_from_arrays(volumes, device='cuda'):
    """volumes: iterable of (image uint8 [Z, Y, X] or [Z, Y, X, ch], mask uint8 [Z, Y, X] class ids, weight uint8 [Z, Y, X] or
    [Z, Y, X, 2]: what VolumeData.build_annotation_volumes / Slicer.update_volume produce).  Returns the list VolumeDataset works
    on: uint8 tensors resident on `device`, the image as [Z, Y, X, ch]."""
    out = []
    for image, mask, weight in volumes:
        t = [a.to(device=device, dtype=torch.uint8).contiguous() if torch.is_tensor(a)
             else torch.from_numpy(np.array(a, dtype=np.uint8, order='C')).to(device) for a in (image, mask, weight)]
        if t[0].dim() == 3:
            t[0] = t[0][..., None]
        _check_volume(*t)
        out.append(t)
    return out


def _check_volume(image, mask, weight):
    ok = image.dim() == 4 and 1 <= image.shape[3] <= 4 and mask.shape == image.shape[:3] and weight.shape[:3] == image.shape[:3] \
        and (weight.dim() == 3 or (weight.dim() == 4 and weight.shape[3] == 2))
    if not ok or any(t.dtype != torch.uint8 or not t.is_contiguous() for t in (image, mask, weight)):
        raise ValueError(f'annotation volumes: image {tuple(image.shape)} (uint8 [Z, Y, X, 1..4]), mask {tuple(mask.shape)} ([Z, Y, X]), '
                         f'weight {tuple(weight.shape)} ([Z, Y, X] or [Z, Y, X, 2]) must be contiguous uint8 over one grid')


def load_volume_annotations(device='cuda'):
    """What VolumeData(f, annotations=True) reads (volumedata.py:24-30), for every data/image_volumes/<name>.zarr in sorted
    order: level '0' of the image, data/mask_volumes/<name>.npy, data/weight_volumes/<name>.npy."""
    from . import multiscale
    volumes = []
    for f in sorted(glob.glob(os.path.join('data', 'image_volumes', '*.zarr'))):
        name = os.path.splitext(os.path.basename(f))[0]
        image = multiscale.read_volume(f, 0).to_device(device)
        volumes.append((image, np.load(os.path.join('data', 'mask_volumes', f'{name}.npy')),
                        np.load(os.path.join('data', 'weight_volumes', f'{name}.npy'))))
    return volume_annotations_from_arrays(volumes, device)


def patch_candidates(mask, weight):
    """Slicer.get_origin_candidates (slicer.py:67-72) over the ANNOTATED voxels (weight > 0) of a class-id volume: per class
    present there its voxel indices (int64 [n, 3] tensors, row-major order) and the class probabilities max(count) / count,
    normalised.  Torch ops on the tensors' device, once per volume."""
    annotated = weight > 0
    classes = torch.unique(mask[annotated])
    candidates = [torch.nonzero((mask == c) & annotated) for c in classes]
    counts = torch.tensor([c.shape[0] for c in candidates], dtype=torch.float64)
    if len(candidates) == 0:
        return candidates, counts
    weights = counts.max() / counts
    return candidates, weights / weights.sum()


def _random_rotation(gen):
    """Rotation by a uniform angle about a uniformly random unit axis (normals, normalised: slicer.py:40-44), by Rodrigues' formula."""
    while True:
        k = torch.randn(3, generator=gen, dtype=torch.float64).numpy()
        if np.linalg.norm(k) >= 0.0001:
            break
    k = k / np.linalg.norm(k)
    angle = _uniform(0.0, 2.0 * math.pi, gen)
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + math.sin(angle) * K + (1.0 - math.cos(angle)) * (K @ K)


def draw_patch_params(shape, patch, candidates, gen=None, sampling_mode='random', scale=(0.5, 1.0), augment=True):
    """One sample's (m[9], c[3]) of iunet_patch_batch for a volume of `shape` and a patch (SZ, SY, SX): patch voxel t (centred
    coordinates) reads source coordinate m t + c.  'random': a random rotation times an isotropic scale from `scale` (source
    voxels per output voxel) times three independent flips; 'grid' (the app's "Axially-aligned" mode): a uniformly chosen signed
    permutation, scale 1; augment=False: the identity.  The centre puts a drawn candidate voxel (class by `candidates`'
    probabilities, then uniform among its voxels, as Slicer.randomize) exactly on a uniformly drawn voxel of the patch, so the
    patch holds an annotation without the reference's draw-again loop (loader.py:62-68).  In the two axis-aligned forms every
    source coordinate is then an integer (even patch sizes) and the patch is moved inside the volume where it fits."""
    cands, probs = candidates
    if len(cands) == 0:
        raise ValueError('no annotated voxel (weight > 0) to centre a patch on')
    aligned = not augment or sampling_mode == 'grid'
    if not augment:
        M = np.eye(3)
    elif sampling_mode == 'grid':
        perm = torch.randperm(3, generator=gen).tolist()
        sign = torch.randint(0, 2, (3,), generator=gen).tolist()
        M = np.zeros((3, 3))
        for a in range(3):
            M[a, perm[a]] = 1.0 - 2.0 * sign[a]
    elif sampling_mode == 'random':
        R = _random_rotation(gen)
        s = _uniform(scale[0], scale[1], gen)
        flips = 1.0 - 2.0 * torch.randint(0, 2, (3,), generator=gen).double().numpy()
        M = s * R * flips[None, :]
    else:
        raise ValueError('sampling_mode must be either "random" or "grid".')
    cum = np.cumsum(np.asarray(probs, dtype=np.float64))
    k = min(int(np.searchsorted(cum, torch.rand(1, generator=gen, dtype=torch.float64).item(), side='right')), len(cands) - 1)
    voxel = np.array(cands[k][torch.randint(0, int(cands[k].shape[0]), (1,), generator=gen).item()].tolist(), dtype=np.float64)
    half = (np.array(patch, dtype=np.float64) - 1.0) / 2.0
    t = np.array([torch.randint(0, int(S), (1,), generator=gen).item() for S in patch], dtype=np.float64) - half
    c = voxel - M @ t
    if aligned:                                       # source box of axis a: c[a] -+ half[j] of the patch axis j it runs along
        for a in range(3):
            h, n = half[int(np.argmax(np.abs(M[a])))], int(shape[a])
            if 2 * h + 1 <= n:
                c[a] = min(max(c[a], h), n - 1 - h)
    return [float(v) for v in M.reshape(-1)], [float(v) for v in c]


class VolumeDataset:
    """`count` random patches per epoch of the volumes of load_volume_annotations / volume_annotations_from_arrays (the 3-D form
    of load_resliced_annotations, loader.py:48-82: a uniformly drawn volume per sample, VolumeData.sample's orders -- image
    `order`, mask and weight 0).  augment=True: new patches at every call; augment=False: `count` axis-aligned patches drawn once
    here from `generator`, the same every epoch.  elastic / color_jitter / blur_or_noise: the three further transforms (DESIGN.md
    section 18), off by default -- nothing more is drawn or launched; they need augment=True."""

    def __init__(self, volumes, num_classes, patch_size=64, count=100, weight_channel=0, augment=True, sampling_mode='random', order=1,
                 generator=None, keep_dark=False, elastic=False, color_jitter=False, blur_or_noise=False, elastic_alpha=50.0,
                 elastic_sigma=5.0, noise_sigma=0.1):
        if (elastic or color_jitter or blur_or_noise) and not augment:
            raise ValueError('elastic / color_jitter / blur_or_noise are augmentations: they need augment=True')
        self.volumes = [tuple(v) for v in volumes]
        if not self.volumes:
            raise ValueError('no annotation volumes')
        for v in self.volumes:
            _check_volume(*v)
        if len({int(v[0].shape[3]) for v in self.volumes}) != 1:
            raise ValueError('annotation volumes differ in their number of image channels')
        self.patch = (int(patch_size),) * 3 if isinstance(patch_size, int) else tuple(int(s) for s in patch_size)
        if len(self.patch) != 3 or min(self.patch) < 1 or (sampling_mode == 'grid' or not augment) and any(s % 2 for s in self.patch):
            raise ValueError(f'patch_size {patch_size}: an int or (SZ, SY, SX), even for the axis-aligned forms')
        if order not in (0, 1) or sampling_mode not in ('random', 'grid'):
            raise ValueError(f'order {order} (0 or 1), sampling_mode {sampling_mode!r} ("random" or "grid")')
        self.num_classes, self.count, self.weight_channel = int(num_classes), int(count), int(weight_channel)
        self.augment, self.sampling_mode, self.order, self.generator, self.keep_dark = augment, sampling_mode, int(order), generator, bool(keep_dark)
        self.candidates = []                    # per volume, on the host: drawing from them costs no device round trip
        for image, mask, weight in self.volumes:
            cands, probs = patch_candidates(mask, self._weight(weight))
            self.candidates.append(([c.cpu() for c in cands], probs))
        self.elastic, self.color_jitter, self.blur_or_noise = bool(elastic), bool(color_jitter), bool(blur_or_noise)
        self.elastic_alpha, self.elastic_sigma, self.noise_sigma = float(elastic_alpha), float(elastic_sigma), float(noise_sigma)
        self._lut = self._taps = self._ws = None
        self._fixed = None if augment else [self.draw() for _ in range(self.count)]

    def _weight(self, weight):
        return weight if weight.dim() == 3 else weight[..., self.weight_channel]

    def __len__(self):
        return self.count

    def draw(self):
        """(volume index, m, c) of one sample, from the generator."""
        vi = torch.randint(0, len(self.volumes), (1,), generator=self.generator).item()
        m, c = draw_patch_params(tuple(self.volumes[vi][1].shape), self.patch, self.candidates[vi], self.generator,
                                 sampling_mode=self.sampling_mode, augment=self.augment)
        return vi, m, c

    def descriptors(self, params):
        descs = (PatchDesc * len(params))()
        for d, (vi, m, c) in zip(descs, params):
            image, mask, weight = self.volumes[vi]
            d.image, d.mask = image.data_ptr(), mask.data_ptr()
            d.weight, d.wstride = (weight.data_ptr(), 1) if weight.dim() == 3 else (weight.data_ptr() + self.weight_channel, int(weight.shape[3]))
            d.Z, d.Y, d.X = [int(s) for s in mask.shape]
            d.keep_dark = int(self.keep_dark)
            for q in range(9):
                d.m[q] = m[q]
            for q in range(3):
                d.c[q] = c[q]
        return descs

    def batch(self, indices, params=None, extra=None):
        """(X [B, ch, SZ, SY, SX], y, w [B, C, SZ, SY, SX]) fp16 for len(indices) samples.  `params`: optional list of (volume index,
        m[9], c[3]) per sample; else drawn from the generator (augment=True) or the fixed set's entries `indices`.  `extra`: optional
        list, per sample, of the dict `draw_extra` returns (a missing entry = off), drawn after each sample's `draw()` when None and
        a transform is switched on.  With the three transforms off and no `extra` the batch is ONE launch (iunet_patch_batch); else
        the pipeline of iunet_patch_batch_extra."""
        extras_on = self.elastic or self.color_jitter or self.blur_or_noise
        if extra is not None and not self.augment:
            raise ValueError('extra: the further transforms need augment=True')
        drawn = None
        if extra is None and extras_on:
            given, params, drawn = params, [], []
            for k in range(len(indices)):                              # per sample: draw(), then draw_extra
                params.append(given[k] if given is not None else self.draw())
                drawn.append(draw_extra(self.generator, self.elastic, self.color_jitter, self.blur_or_noise, self.elastic_alpha,
                                        self.noise_sigma))
        elif params is None:
            params = [self.draw() for _ in indices] if self.augment else [self._fixed[i] for i in indices]
        dev = self.volumes[0][0].device
        assert nv.lib().iunet_patch_desc_bytes() == ctypes.sizeof(PatchDesc), 'PatchDesc layout mismatch with libiunet'
        if self._lut is None:
            self._lut = torch.from_numpy((np.arange(256) / 255).astype('float32')).to(torch.float16).to(dev)
        descs = self.descriptors(params)
        B, ch, C = len(params), int(self.volumes[0][0].shape[3]), self.num_classes
        X = torch.empty((B, ch) + self.patch, dtype=torch.float16, device=dev)
        y = torch.empty((B, C) + self.patch, dtype=torch.float16, device=dev)
        w = torch.empty((B, C) + self.patch, dtype=torch.float16, device=dev)
        if extra is None and drawn is None:
            raw = torch.frombuffer(bytearray(bytes(descs)), dtype=torch.uint8).to(dev)
            with torch.cuda.device(dev):
                nv.call('iunet_patch_batch', nv.ptr(raw), B, ch, C, *self.patch, self.order, nv.ptr(self._lut), nv.ptr(X), nv.ptr(y), nv.ptr(w),
                        nv.stream())
            return X, y, w
        raw, extras, use, taps, ws = _upload_extras(self, descs, drawn if extra is None else extra, PatchExtraDesc, _fill_patch_extra,
                                                    nv.lib().iunet_patch_extra_desc_bytes, nv.lib().iunet_patch_extra_ws_bytes,
                                                    (B, ch) + self.patch, dev)
        with torch.cuda.device(dev):
            nv.call('iunet_patch_batch_extra', nv.ptr(raw), extras, use, B, ch, C, *self.patch,
                    self.order, nv.ptr(self._lut), nv.ptr(taps), int(taps.numel()), nv.ptr(ws), int(ws.numel()), nv.ptr(X),
                    nv.ptr(y), nv.ptr(w), nv.stream())
        return X, y, w


def get_volume_loader(set_type='train', num_classes=2, batch_size=2, patch_size=64, count=100, augment=True, shuffle=True, volumes=None,
                      generator=None, elastic=False, color_jitter=False, blur_or_noise=False, elastic_alpha=50.0, elastic_sigma=5.0,
                      noise_sigma=0.1):
    """The 3-D counterpart of get_data_loader: `count` patches per epoch from the annotation volumes (`volumes`: skip the file read
    and use these).  set_type 'train' reads weight channel 0, anything else channel 1 (loader.py:56-59).  elastic / color_jitter /
    blur_or_noise: the three further transforms, off by default; trainer.train_model(dim=3) takes such a
    loader as `train_loader`."""
    if volumes is None:
        volumes = load_volume_annotations()
    dataset = VolumeDataset(volumes, num_classes, patch_size=patch_size, count=count, weight_channel=0 if set_type == 'train' else 1,
                            augment=augment, generator=generator, elastic=elastic, color_jitter=color_jitter, blur_or_noise=blur_or_noise,
                            elastic_alpha=elastic_alpha, elastic_sigma=elastic_sigma, noise_sigma=noise_sigma)
    return DeviceLoader(dataset, batch_size=batch_size, shuffle=shuffle, generator=generator)
