"""Host mirror of where the fused DLA backbone kernels run a launch, for a device with `cus` CUs (MI355X: 256).

- conv64_root (conv64_root.hip, the level tail): `total` = B * (H / 8) * (W / 32) work items of 8 x 32 pixels on the INPUT map;
  launch_conv64_root picks the template instance <POOL, S2D, NORM> from which outputs exist (NORM = 0: no ordinary copy of the
  root output, only the space-to-depth one).  persistent_grid (common.h): min(total, cus) workgroups; `single` when total <= cus
  (workgroup b runs item b, no tickets), else each workgroup's first draw takes three consecutive items and later draws one.
- conv32s2_fused (conv32s2_fused.hip, the level entry): `total` = B * (Ho / 8) * (Wo / 32) items on the half-resolution OUTPUT
  map, the same ticket regimes.
- stem_fused (conv_stem_fused.hip): one 256-thread workgroup per 16 x 32 full-resolution tile, B * (H / 16) * (W / 32); the
  two-layer form (base_layer + level0, 16 channels at full resolution) or the three-layer form (+ level1, 32 channels at half).
- maxpool_s2d (maxpool_kernel with ksize 0): one thread per (pixel, 8 channels), B * Ho * Wo * C / 8 threads in 256-thread
  blocks; the threads of the last block past the total return at once."""

ROOT_INSTANCES = ((1, 1, 0), (0, 1, 0), (1, 1, 1), (1, 0, 1), (0, 1, 1), (0, 0, 1))     # launch_conv64_root's order
STEM_NAMES = {2: 'stem7x7+conv3x3_fused', 3: 'stem7x7+3x3+3x3s2_fused'}


def cdiv(a, b):
    return -(-a // b)


def _persistent(total, cus):
    grid, single = min(total, cus), total <= cus
    return {'total': total, 'grid': grid, 'single': single,
            # ticket regime: the first draw of each workgroup takes items 3 t .. 3 t + 2; who gets any, and the last draw's share
            'first_draw_busy': None if single else min(grid, cdiv(total, 3)),
            'mod3': None if single else total % 3}


def root_instance(pool, s2d, out):
    """launch_conv64_root's template instance (POOL, S2D, NORM) for the outputs a launch has."""
    if not out and not s2d:
        raise ValueError('conv64_root: no root output and no space-to-depth copy')
    return (int(bool(pool)), int(bool(s2d)), int(bool(out)))


def root_name(pool, s2d):
    """The op name rtm3d_op_conv64_root records."""
    return ('conv3x3_c64+root1x1+pool_fused' if pool else 'conv3x3_c64+root1x1_fused') + ('+s2d' if s2d else '')


def conv64_root(B, H, W, pool, s2d, out=True, cus=256):
    """A level-tail launch over B images of an H x W input map."""
    assert H % 8 == 0 and W % 32 == 0
    r = _persistent(B * (H // 8) * (W // 32), cus)
    r['instance'] = root_instance(pool, s2d, out)
    return r


def conv32s2(B, Ho, Wo, cus=256):
    """A level-entry launch over B images of an Ho x Wo OUTPUT map (input 2 Ho x 2 Wo)."""
    assert Ho % 8 == 0 and Wo % 32 == 0
    return _persistent(B * (Ho // 8) * (Wo // 32), cus)


def stem(B, H, W, layers):
    """A fused stem launch over B images of H x W pixels: two or three layers."""
    assert H % 16 == 0 and W % 32 == 0 and layers in (2, 3)
    return {'layers': layers, 'grid': B * (H // 16) * (W // 32), 'out_scale': 2 if layers == 3 else 1, 'out_channels': 16 * (layers - 1)}


def maxpool_s2d(B, Ho, Wo, C):
    assert C % 8 == 0
    threads = B * Ho * Wo * (C // 8)
    blocks = cdiv(threads, 256)
    return {'threads': threads, 'blocks': blocks, 'idle': blocks * 256 - threads}


def regime_key(kind, single=None, instance=None, conv_relu=None, root_relu=None, layers=None, channels=None, idle=None):
    """The regime a fused launch exercises: what the GPU cases must cover for every launch of the product plans."""
    if kind == 'conv64_root':
        return (kind, tuple(instance), bool(single), bool(conv_relu), bool(root_relu))
    if kind == 'conv32s2_fused':
        return (kind, bool(single))
    if kind == 'stem_fused':
        return (kind, layers)
    if kind == 'maxpool_s2d':
        return (kind, channels, bool(idle))
    raise ValueError('not a fused launch kind: %r' % kind)
