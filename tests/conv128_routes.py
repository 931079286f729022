"""Host mirror of where the 128-pixel conv kernels (conv_mfma.hip) and the three halo kernels (conv64_halo.hip, conv128_halo.hip,
conv64s2_halo.hip) run a launch, for an 8-XCD device with `cus` CUs (MI355X: 256).

- admit_mfma128 (runtime.hip): BN-channel tiles (cout padded to BN), MT = ceil(M / 128) pixel tiles, NT channel tiles,
  wgs = MT * NT * groups.  An NCHW fp32 output or BN 16 / 32 runs the one-stage kernel (conv_mfma_kernel); otherwise a launch
  of at most `cus` workgroups runs conv_mfma_deep_kernel ('deep'), and K is split over ks = min(cus // wgs, ksteps // 4, 16)
  ranges ('deep_splitk') when ks >= 2, wgs * 2 <= cus, wgs <= SPLIT_CTRS and ksteps >= 8.  Split z covers k-steps
  [z * ksteps // ks, (z + 1) * ksteps // ks); the partial tiles take ks * wgs * 128 * BN floats of slab.
- grid (mt8 * NT, groups, ks), mt8 = MT rounded up to 8: workgroup x serves pixel tile xcd * chunk + j // NT (xcd = x & 7,
  j = x >> 3, chunk = ceil(MT / 8)) and returns at once when that tile is past MT.
- halo kernels: `total` work items (8 x 32 pixel tiles per image, times cout / 128 for conv128; 4 x 32 output tiles for the
  stride-2 conv64s2), persistent_grid (common.h): min(total, cus) workgroups; `single` when total <= cus (workgroup b runs item
  b, no tickets), else each workgroup's first draw takes three consecutive items and later draws one."""

XCDS = 8
SPLIT_CTRS = 256
MFMA128_BASES = ('conv1x1_mfma', 'deconv4x4_phase_mfma', 'conv3x3_mfma')
HALO_NAMES = {'conv3x3_c64_halo': 'c64_halo', 'conv3x3_c128_halo': 'c128_halo', 'conv3x3s2_c64_halo': 'c64s2_halo'}
MFMA128_ROUTES = ('one_stage', 'deep', 'deep_splitk')


def cdiv(a, b):
    return -(-a // b)


def route_of(name):
    """Route of a conv op from its recorded name: admit_mfma128's bare base name, '_deep' or '_deep_splitk', or the halo kernels'
    fixed names.  Anything else (the conv256 names among them) raises."""
    if name in HALO_NAMES:
        return HALO_NAMES[name]
    for b in MFMA128_BASES:
        if name == b:
            return 'one_stage'
        if name.startswith(b + '_') and name[len(b) + 1:] in ('deep', 'deep_splitk'):
            return name[len(b) + 1:]
    raise ValueError('not a 128-pixel or halo conv op name: %r' % name)


def admit_mfma128(M, cin, cout, ntaps, groups=1, bn=64, nchw=False, cus=256):
    """admit_mfma128 and launch_conv_mfma[_deep] for M output pixels per group (all images), cout channels per group."""
    assert bn in (16, 32, 64, 128) and cin % 64 == 0 and cus % XCDS == 0
    assert nchw or cout % bn == 0
    cout_pad = cdiv(cout, bn) * bn
    cpt = cin // 64
    ksteps = ntaps * cpt
    MT, NT = cdiv(M, 128), cout_pad // bn
    wgs = MT * NT * groups
    ks = 1
    if nchw or bn not in (64, 128) or wgs > cus:
        route = 'one_stage'
    else:
        route = 'deep'
        if wgs * 2 <= cus and wgs <= SPLIT_CTRS and ksteps >= 8:
            ks = min(cus // wgs, ksteps // 4, 16)
            if ks >= 2:
                route = 'deep_splitk'
            else:
                ks = 1
    chunk = cdiv(MT, XCDS)
    mt8 = chunk * XCDS
    grid = (mt8 * NT, groups, ks)
    idle = sum(1 for x in range(mt8 * NT) if (x & 7) * chunk + (x >> 3) // NT >= MT)
    return {'route': route, 'bn': bn, 'cout_pad': cout_pad, 'cpt': cpt, 'ksteps': ksteps, 'MT': MT, 'NT': NT, 'wgs': wgs, 'ks': ks,
            'ranges': [(z * ksteps // ks, (z + 1) * ksteps // ks) for z in range(ks)],
            'slab_floats': ks * wgs * 128 * bn if ks > 1 else 0,
            'chunk': chunk, 'grid': grid, 'idle': idle * groups * ks,
            'empty_xcds': sum(1 for x in range(XCDS) if x * chunk >= MT)}


def halo(kernel, B, Hm, Wm, cout=None, cus=256):
    """Work items and ticket regime of a halo kernel launch over B images of an Hm x Wm OUTPUT map."""
    if kernel == 'c64s2_halo':
        assert Hm % 4 == 0 and Wm % 32 == 0
        total = B * (Hm // 4) * (Wm // 32)
    else:
        assert Hm % 8 == 0 and Wm % 32 == 0
        total = B * (Hm // 8) * (Wm // 32) * (cout // 128 if kernel == 'c128_halo' else 1)
    grid, single = min(total, cus), total <= cus
    return {'total': total, 'grid': grid, 'single': single,
            # ticket regime: the first draw of each workgroup takes items 3 t .. 3 t + 2; who gets any, and the last draw's share
            'first_draw_busy': None if single else min(grid, cdiv(total, 3)),
            'mod3': None if single else total % 3}


def regime_key(kernel, route, bn=None, ks=1, nchw=False, res=False, s2d='', grouped=False, tap_dc=False, stride=1, out_scale=1,
               single=None):
    """The regime a conv launch exercises: what the GPU cases must cover for every launch of the product plans."""
    return (kernel, route, bn, ks, 'nchw' if nchw else 'nhwc', bool(res), s2d, bool(grouped), bool(tap_dc), stride, out_scale, single)
