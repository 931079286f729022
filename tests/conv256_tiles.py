"""Host mirror of how the 256 x 256 conv kernels (conv_mfma256.hip, conv_mfma256_halo.hip, conv_mfma256_lattice.hip) split a
launch into tiles and hand the tiles out, for an 8-XCD device with `cus` CUs (MI355X: 256).

- one-tile route (conv_mfma256_kernel): one workgroup per (pixel tile, channel tile, group), no tickets.
- generic persistent and halo routes: cus workgroups; a launch with at most `cus` tiles draws from ONE list (one_list), otherwise
  XCD x draws from its own list: pixel tiles [x * chunk, (x + 1) * chunk), chunk = ceil(MT / 8), times NT channel tiles times
  the groups.  Workgroup b serves the list of XCD b & 7: cus / 8 workgroups per list.
- lattice route: always the per-XCD lists (no one_list).  The kernel's 16-slot halo-row ring moves on by 10 slots per 64-channel
  chunk, counted across the tiles a workgroup runs: its k-th tile starts at ring base 10 * cpt * k mod 16.

`run` is the longest run of consecutive tiles some workgroup is guaranteed to execute: a list of L tiles drained by w
workgroups gives one of them at least ceil(L / w) (pigeonhole)."""

ROUTES = ('1tile', 'persistent', 'halo', 'lattice')
RING = 16
XCDS = 8


def cdiv(a, b):
    return -(-a // b)


def route_of(name):
    """Route of a conv256 op from its recorded name (admit_mfma256: '_1tile', '', '_halo' or '_lattice' behind the base name)."""
    base = ('conv1x1_mfma256', 'deconv4x4_phase_mfma256', 'conv3x3_mfma256')
    for b in base:
        if name == b:
            return 'persistent'
        if name.startswith(b + '_') and name[len(b) + 1:] in ('1tile', 'halo', 'lattice'):
            return name[len(b) + 1:]
    raise ValueError('not a conv256 op name: %r' % name)


def tiles(route, M, cout, groups=1, cin=64, cus=256):
    """Tile lists of a conv256 launch over M output pixels per group, cout output channels per group."""
    assert route in ROUTES and cout % 256 == 0 and cin % 64 == 0 and cus % XCDS == 0
    MT, NT, cpt = cdiv(M, 256), cout // 256, cin // 64
    total = MT * NT * groups
    r = {'route': route, 'MT': MT, 'NT': NT, 'groups': groups, 'cpt': cpt, 'total': total}
    if route == '1tile':
        r.update(one_list=None, chunk=cdiv(MT, XCDS), lists=None, empty=0, run=1, bases=None)
        return r
    one_list = route != 'lattice' and total <= cus
    if one_list:
        chunk, lists, wgs = MT, [total], cus
    else:
        chunk, wgs = cdiv(MT, XCDS), cus // XCDS
        lists = [min(max(MT - x * chunk, 0), chunk) * NT * groups for x in range(XCDS)]
    assert sum(lists) == total
    run = max(cdiv(L, wgs) for L in lists)
    r.update(one_list=one_list, chunk=chunk, lists=lists, empty=sum(1 for L in lists if L == 0), run=run,
             bases=sorted({10 * cpt * k % RING for k in range(run)}) if route == 'lattice' else None)
    return r


def reachable_bases(cpt):
    """Every ring base a lattice tile of cpt chunks can start at."""
    return sorted({10 * cpt * k % RING for k in range(RING)})
