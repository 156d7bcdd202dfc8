"""What the canonical networks look like, stated once for every engine: stage names, stage channel counts, transposed convs, parameter
names, level grids and the constructors' limits.  Pure Python: no device, no library.

A stage is 2 x [conv 3^d -> norm -> ReLU] with parameters `{prefix}.conv{1,2}.weight` and `{prefix}.bn{1,2}.{BN_KEYS}`.  U-Net: enc{l}
for l = 0 .. L-1, then dec{l} for l = L-2 .. 0, each behind the transposed conv `dec{l}.up` ch[l+1] -> ch[l].  U-Net++: the same encoder,
then the node dec{i}_{j} for (i, j) in unet.nested_nodes(L), each behind `dec{i}_{j}.up` ch[i+1] -> ch[i].  The encoder-only
architectures (LinkNet, DeepLabV3, Segformer) keep enc{l} and name their decoder's parameters themselves.  unet.param_shapes is the
independent statement of the same names and shapes (tests/test_topology_cpu.py holds the two against each other).
"""
BN_KEYS = ('weight', 'bias', 'running_mean', 'running_var')


def _vox(dims):
    return dims[0] * dims[1] * dims[2]


def channels(base, levels):
    return [base * 2 ** l for l in range(levels)]


def encoder_names(levels):
    return [f'enc{l}' for l in range(levels)]


def stage_names(levels):
    return encoder_names(levels) + [f'dec{l}' for l in range(levels - 2, -1, -1)]


def up_convs(levels):
    """(prefix, level l) of every transposed conv ch[l+1] -> ch[l], in parameter order."""
    return [(f'dec{l}', l) for l in range(levels - 2, -1, -1)]


def _nodes(levels):
    from .unet import nested_nodes          # (unet imports the engines, which import this module)
    return nested_nodes(levels)


def nested_stage_names(levels):
    return encoder_names(levels) + [f'dec{i}_{j}' for i, j in _nodes(levels)]


def nested_up_convs(levels):
    return [(f'dec{i}_{j}', i) for i, j in _nodes(levels)]


def stage_io(prefix, cin, ch):
    """(input channels, output channels, level) of the stage enc{l}, dec{l} (reads concat(skip, up)) or dec{i}_{j} (reads X^{i,0..j-1}
    and up(X^{i+1,j-1}))."""
    if '_' in prefix:
        i, j = (int(t) for t in prefix[3:].split('_'))
        return (j + 1) * ch[i], ch[i], i
    l = int(prefix[3:])
    if prefix.startswith('enc'):
        return (cin if l == 0 else ch[l - 1]), ch[l], l
    return 2 * ch[l], ch[l], l


def stage_param_names(prefix):
    return [n for j in (1, 2) for n in [f'{prefix}.conv{j}.weight'] + [f'{prefix}.bn{j}.{k}' for k in BN_KEYS]]


def param_names(stages, ups):
    """Every parameter of a network of `stages` whose transposed convs are `ups`, in unet.param_shapes' order: each decoder stage behind
    its transposed conv, the head last."""
    up = {prefix for prefix, _ in ups}
    names = []
    for prefix in stages:
        if prefix in up:
            names += [f'{prefix}.up.weight', f'{prefix}.up.bias']
        names += stage_param_names(prefix)
    return names + ['head.weight', 'head.bias']


def level_dims(dim, levels, D, H, W):
    return [((D >> l) if dim == 3 else 1, H >> l, W >> l) for l in range(levels)]


def check_spatial(dim, levels, D, H, W):
    """Every level halves the grid: H, W (and D in 3-D) must be divisible by 2^(levels-1), and D == 1 in 2-D."""
    f = 2 ** (levels - 1)
    if H % f or W % f or (dim == 3 and D % f) or (dim == 2 and D != 1):
        raise ValueError(f'spatial size {(D, H, W)} must be divisible by {f} (and D == 1 in 2-D)')


def check_limits(dim, base, cin, ncls, norm='batch', groups=8):
    """The limits of the native U-Net's constructors (cin None: no limit on the input channels)."""
    if dim not in (2, 3):
        raise ValueError('dim must be 2 or 3')
    if base % 32 != 0:
        raise NotImplementedError('native U-Net needs base channels to be a multiple of 32')
    if cin is not None and not (1 <= cin <= 4):
        raise NotImplementedError('native U-Net supports 1..4 input channels')
    if not (2 <= ncls <= 10):
        raise NotImplementedError('native U-Net supports 2..10 classes (app.py:162)')
    if norm not in ('batch', 'group'):
        raise ValueError("norm must be 'batch' or 'group'")
    if norm == 'group' and base % groups:
        raise ValueError(f'{groups} groups do not divide {base} channels')
