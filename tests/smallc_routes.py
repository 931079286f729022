"""Host mirror of which instance of the register-direct small-channel conv kernels (conv_smallc.hip) runs a launch of
rtm3d_op_conv kernel 3, with which grid, and which of the kernel's edges the launch touches.

- launch_conv_smallc: a stride-1, out_scale-1 launch with cout 16 and cin 4 (49 taps) or cin 16 in the 6-k-step packing runs
  conv_smallc_rows_kernel<CIN, NCT, KR, SPR, R = 32> ('rows'): a wave owns a 16-pixel-wide column strip of 32 output rows;
  nwaves = B * strips_y * tiles_x, four waves to a block.  Everything else runs conv_smallc_kernel<CIN, NCT, S, TPW = 8>
  ('tile'): a wave owns 8 consecutive 16-pixel tiles of the M = B * Hm * Wm output pixels, a block 512 pixels; grid.y = 2
  for the 3x3 32 -> 64 instance (two 32-channel halves).  Instances with an even NCT store 16 bytes per lane, the others 8.
- admit_smallc names the op 'stem7x7_regmfma' for cin 4 and 'conv_smallc_regmfma' otherwise.
- nchw_to_nhwc4_kernel: one thread per pixel, 256 to a block."""

TILE_INSTANCES = {        # (cin, cout, ntaps) -> ((CIN, NCT, S, TPW), grid.y)
    (16, 16, 9): ((16, 1, 5, 8), 1),
    (16, 32, 9): ((16, 2, 5, 8), 1),
    (32, 64, 9): ((32, 2, 9, 8), 2),
    (32, 64, 1): ((32, 4, 1, 8), 1),
    (4, 16, 49): ((4, 1, 7, 8), 1),
    (4, 64, 49): ((4, 4, 7, 8), 1),
}
ROWS_INSTANCES = {        # (cin, cout, ntaps) -> (CIN, NCT, KR, SPR, R)
    (4, 16, 49): (4, 1, 7, 1, 32),
    (16, 16, 9): (16, 1, 3, 2, 32),
}
INSTANCES = [('tile',) + v[0] for v in TILE_INSTANCES.values()] + [('rows',) + v for v in ROWS_INSTANCES.values()]


def cdiv(a, b):
    return -(-a // b)


def op_name(cin):
    return 'stem7x7_regmfma' if cin == 4 else 'conv_smallc_regmfma'


def instance(cin, cout, ntaps, stride=1, out_scale=1, rows_packing=False):
    """('rows', CIN, NCT, KR, SPR, R) or ('tile', CIN, NCT, S, TPW) of a launch; rows_packing: the cin = 16 weight blob holds 6
    k-steps (plan.pack_smallc_weights(rows=True)), which admit_smallc tells from the 5-step one by its size."""
    key = (cin, cout, ntaps)
    if key not in TILE_INSTANCES:
        raise ValueError('conv_smallc.hip has no kernel for cin=%d cout=%d ntaps=%d' % key)
    if rows_packing and not (key == (16, 16, 9) and stride == 1 and out_scale == 1):
        raise ValueError('the 6-k-step packing is admitted for stride-1 16 -> 16 launches only')
    if stride == 1 and out_scale == 1 and key in ROWS_INSTANCES and (cin == 4 or rows_packing):
        return ('rows',) + ROWS_INSTANCES[key]
    return ('tile',) + TILE_INSTANCES[key][0]


def ksteps(inst):
    """MFMA K-steps (of 32 products) per output of an instance."""
    return inst[3] * inst[4] if inst[0] == 'rows' else inst[3]


def launch(B, H, W, cin, cout, ntaps, stride=1, out_scale=1, rows_packing=False):
    """The launch over B images of an H x W INPUT map (iteration domain Hm = (H - 1) // stride + 1, likewise Wm)."""
    Hm, Wm = (H - 1) // stride + 1, (W - 1) // stride + 1
    inst = instance(cin, cout, ntaps, stride, out_scale, rows_packing)
    r = {'instance': inst, 'op': op_name(cin), 'Hm': Hm, 'Wm': Wm, 'ksteps': ksteps(inst)}
    if inst[0] == 'rows':
        R = inst[5]
        tiles_x, strips_y = cdiv(Wm, 16), cdiv(Hm, R)
        nwaves = B * strips_y * tiles_x
        r.update(grid=(cdiv(nwaves, 4), 1), tiles_x=tiles_x, w_mod16=Wm % 16, strips_y=strips_y, h_mod32=Hm % R,
                 last_rows=Hm - (strips_y - 1) * R, nwaves=nwaves, nwaves_mod4=nwaves % 4, store_bytes=8)
        return r
    NCT, TPW = inst[2], inst[4]
    M = B * Hm * Wm
    ntiles = cdiv(M, 16)
    grid_x = cdiv(ntiles, 4 * TPW)
    row = img = 0
    for t in range(ntiles):
        first, last = t * 16, min(t * 16 + 15, M - 1)
        row += first // Wm != last // Wm
        img += first // (Hm * Wm) != last // (Hm * Wm)
    r.update(grid=(grid_x, TILE_INSTANCES[(cin, cout, ntaps)][1]), M=M, ntiles=ntiles, m_mod16=M % 16, ntiles_mod8=ntiles % TPW,
             idle_waves=grid_x * 4 - cdiv(ntiles, TPW), row_straddles=row, image_straddles=img, grid_y=TILE_INSTANCES[(cin, cout, ntaps)][1],
             store_bytes=16 if NCT % 2 == 0 else 8)
    return r


def regime_key(r, relu):
    """What a launch exercises, as the coverage guard compares GPU cases with the product plans' launches."""
    if r['instance'][0] == 'rows':
        return (r['instance'], bool(relu), r['w_mod16'] != 0, r['h_mod32'] != 0, r['nwaves_mod4'] != 0)
    return (r['instance'], bool(relu), r['m_mod16'] != 0, r['ntiles_mod8'] != 0, r['idle_waves'] > 0, r['row_straddles'] > 0,
            r['image_straddles'] > 0)


def nchw_to_nhwc4(B, H, W):
    threads = B * H * W
    blocks = cdiv(threads, 256)
    return {'threads': threads, 'blocks': blocks, 'idle': blocks * 256 - threads}
