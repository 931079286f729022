"""Host mirror of what the launch code decides for the tail of the forward path, for a device with `cus` CUs (MI355X: 256).

- softmax_fuse (rtm3d_op_softmax_fuse in runtime.hip, launch_softmax_fuse in pool_softmax.hip): the reduce pass runs one workgroup
  per (operand, image, chunk of rows), one row per chunk while `small` (B * ceil(H / 2) < 2 * cus), else two; it is skipped when
  the producers' epilogues wrote the partials (partial_chunks > 0, stat_chunks 128-pixel runs per image).  The combine pass folds
  chunk k on part k % 16.  The apply pass cuts each row into `xsplit` column segments of `seg_w` pixels (rounded up to 8, so the
  last segments can be short or empty); a workgroup walks its segment 16 pixels at a time, two pixels (x, x + 8) per lane.
- headout (rtm3d_op_headout, conv_headout.hip): 16-row tiles once B * ceil(H / 16) * ceil(W / 32) * nheads >= 4 * cus, else 8-row
  tiles; 32-pixel tile columns; grid (B * tiles_y * tiles_x, nheads); workgroup b takes tile xcd_contiguous_index(b, grid x).
- maxpool (the k x k form of maxpool_kernel): one thread per (output pixel, 8 channels) in 256-thread blocks.
- peak patches (sparse_heads.hip): patch pixel (r, c) of a 15 x 15 patch holds z at the peak + patch_cell(r, c); the mask op
  clears the window positions of a slot that lie outside the image."""

PATCH = 15
COMBINE_PARTS = 16


def cdiv(a, b):
    return -(-a // b)


def stat_chunks(groups, Hm, Wm):
    """128-pixel runs per image a halo-route producer emits partials for: two per 8 x 32 tile and group."""
    assert Hm % 8 == 0 and Wm % 32 == 0
    return groups * (Hm // 8) * (Wm // 32) * 2


def softmax_fuse(B, H, W, n_u, cus=256, partial_chunks=0):
    assert 1 <= n_u <= 3
    small = B * cdiv(H, 2) < 2 * cus
    rpc = 1 if small else 2
    chunks = cdiv(H, rpc)
    xsplit = 1
    while xsplit < 4 and W // (xsplit * 2) >= 64:
        xsplit *= 2
    while B * H * xsplit < 2 * cus and xsplit < 8 and W // (xsplit * 2) >= 32:
        xsplit *= 2
    seg_w = cdiv(cdiv(W, xsplit), 8) * 8
    widths = [max(0, min((s + 1) * seg_w, W) - s * seg_w) for s in range(xsplit)]
    reduce_runs = partial_chunks <= 0
    folded = chunks if reduce_runs else partial_chunks
    return {'small': small, 'rows_per_chunk': rpc, 'chunks': chunks, 'last_chunk_rows': H - (chunks - 1) * rpc,
            'xsplit': xsplit, 'seg_w': seg_w, 'apply_chunks': H * xsplit, 'seg_widths': widths, 'last_seg_w': widths[-1],
            'reduce_runs': reduce_runs, 'reduce_grid': (chunks, B, n_u) if reduce_runs else None,
            'combine_grid': (B, n_u, 4), 'apply_grid': (H * xsplit, B, 1),
            'combine_chunks': folded, 'parts_busy': min(COMBINE_PARTS, folded),
            # a lane of the reduce pass takes pixels x, x + 8, x + 16, x + 24 of every 32: a tail when W % 32 != 0
            'reduce_tail': W % 32 != 0,
            # the apply pass takes x, x + 8 of every 16 of a segment: the second pixel is dropped (`break`) in a segment whose
            # width leaves 1..8 pixels over
            'apply_tail': any(0 < w % 16 <= 8 for w in widths)}


def headout(B, H, W, nheads, cus=256, in_P=1):
    assert 1 <= nheads <= 4 and in_P >= 1
    count = B * cdiv(H, 16) * cdiv(W, 32) * nheads
    rows = 16 if count >= 4 * cus else 8
    tx, ty = cdiv(W, 32), cdiv(H, rows)
    y0, x0 = (ty - 1) * rows, (tx - 1) * 32
    return {'switch_count': count, 'tile_rows': rows, 'tiles_x': tx, 'tiles_y': ty, 'grid': (B * ty * tx, nheads),
            'last_rows': H - y0, 'last_cols': W - x0,
            # halo rows y0 - 1 .. y0 + rows (columns x0 - 1 .. x0 + 32) of the last tiles that lie past the border's last
            # row (column) H + in_P - 1: clamped onto it by the staging code
            'halo_rows_past': max(0, y0 + rows + 1 - (H + in_P)), 'halo_cols_past': max(0, x0 + 33 - (W + in_P))}


def xcd_contiguous_index(b, n):
    q, r, xcd, k = n >> 3, n & 7, b & 7, b >> 3
    return xcd * q + (xcd if xcd < r else r) + k


def maxpool(B, Ho, Wo, C):
    assert C % 8 == 0
    threads = B * Ho * Wo * (C // 8)
    blocks = cdiv(threads, 256)
    return {'threads': threads, 'blocks': blocks, 'idle': blocks * 256 - threads}


def patch_cell(r, c):
    """(dy, dx): patch pixel (r, c) holds z(py + dy, px + dx)."""
    assert 0 <= r < PATCH and 0 <= c < PATCH
    return (r % 5 - 2 + 6 * (r // 5 - 1), c % 5 - 2 + 6 * (c // 5 - 1))


def mask_zeroed(py, px, S, origin, img_H, img_W):
    """Window positions (i, j) of an S x S window the mask op clears for a slot whose peak is (py, px); none for py < 0."""
    if py < 0:
        return set()
    return {(i, j) for i in range(S) for j in range(S)
            if not (0 <= py + i - origin < img_H and 0 <= px + j - origin < img_W)}


def _parts_class(chunks):
    if chunks < COMBINE_PARTS:
        return 'lt16'
    if chunks == COMBINE_PARTS:
        return 'eq16'
    return 'gt16_mult' if chunks % COMBINE_PARTS == 0 else 'gt16_ragged'


def regime_key(kind, **k):
    """The regime a launch exercises: what the GPU cases must cover for every launch of the product plans."""
    if kind == 'softmax_fuse':
        r = softmax_fuse(k['B'], k['H'], k['W'], k['n_u'], k.get('cus', 256), k.get('partial_chunks', 0))
        last = 'full' if r['last_seg_w'] == r['seg_w'] else ('empty' if r['last_seg_w'] == 0 else 'short')
        # rows_per_chunk is read by the reduce pass alone
        rows = (r['rows_per_chunk'], r['last_chunk_rows'] != r['rows_per_chunk']) if r['reduce_runs'] else (None, None)
        return (kind, k['n_u'], 'reduce' if r['reduce_runs'] else 'partials') + rows + (
            _parts_class(r['combine_chunks']), r['xsplit'], last, k['W'] % 8 != 0)
    if kind == 'stat_producer':
        return (kind, k['ntaps'], bool(k['one_list']))
    if kind == 'headout':
        r = headout(k['B'], k['H'], k['W'], k['nheads'], k.get('cus', 256), k.get('in_P', 1))
        return (kind, r['tile_rows'], k['nheads'], tuple(k['couts']), r['last_rows'] != r['tile_rows'], r['last_cols'] != 32)
    if kind == 'maxpool':
        return (kind, k['k'], k['stride'], k['pad'], bool(maxpool(k['B'], k['Ho'], k['Wo'], k['C'])['idle']))
    if kind == 'patch_mask':
        return (kind, k['S'], k['origin'])
    raise ValueError('not a tail launch kind: %r' % kind)
