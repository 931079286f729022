"""hipEvent times of the validation loss on one MI355X at B = 32, 3 x 96 x 320 maps (the 384 x 1280 input of the benchmark),
about 10 objects per image: the fused path (rtm3d_loss_eval: the target is formed inside the focal reduction, two launches;
through the Python wrapper and through the C entry point with preallocated outputs) next to what a user would otherwise write
on the device - the target map materialised (rtm3d_loss_heatmap) and the rule of include/rtm3d_hip.h, "validation loss", in
torch ops on it: elementwise focal terms and their sums, the three L1 terms through index tensors built with nonzero(), which
synchronises.  rtm3d_loss_objects (once per batch of labels) is timed on its own.
Median (min) of 20 timed groups of 10 calls after a warm-up.  The two paths are checked against each other before timing.
Prints the table; with an argument, also appends it to that file (profiles/loss.txt holds its output)."""
import ctypes
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

B, C, H, W, PER_IMAGE, GROUPS, PER = 32, 3, 96, 320, 10, 20, 10


def torch_focal(hm_logit, target, alpha, beta):
    """main term of the rule on a materialised target: -(pos + neg) / num_pos, or -neg when there is no positive."""
    import torch
    prob = torch.sigmoid(hm_logit).clamp(1e-4, 1 - 1e-4)
    is_pos = target == 1
    term = torch.where(is_pos, prob.log() * (1 - prob) ** alpha, (1 - prob).log() * prob ** alpha * (1 - target) ** beta)
    return -term.sum(dtype=torch.float64) / is_pos.sum().clamp(min=1)


def torch_loss(pred, t, alpha=2.0, beta=4.0, w=(1.0, 1.0, 0.5, 0.5)):
    """The five items of the rule in torch ops, from the target fields of build_targets."""
    import torch
    hm_logit, vc_logit, mo_logit, vo_logit = pred
    B, _, H, W = hm_logit.shape
    main = torch_focal(hm_logit, t['m_hm'], alpha, beta)
    x, y = t['m_proj'].unbind(1)
    obj = torch.nonzero(t['mask'] & ~t['noise_mask'] & (x >= 0) & (x < W) & (y >= 0) & (y < H)).squeeze(1)
    main_off = (torch.sigmoid(mo_logit[t['img_id'][obj], :, y[obj], x[obj]]) - t['m_off'][obj].float()).abs().mean()
    obj = obj[t['mask_3d'][obj]]
    o, v = torch.nonzero(t['v_mask'][obj]).unbind(1)                    # (object, vertex) pairs that take part
    obj = obj[o]
    img = t['img_id'][obj]
    ver_coor = (vc_logit.view(B, 8, 2, H, W)[img, v, :, y[obj], x[obj]] - t['v_coor_off'][obj, v].float()).abs().mean()
    vx, vy = t['v_proj'][obj, v].unbind(1)
    vertex_off = (torch.sigmoid(vo_logit[img, :, vy, vx]) - t['v_off'][obj, v].float()).abs().mean()
    items = torch.stack([main.float() * w[0], ver_coor * w[1], main_off * w[2], vertex_off * w[3]])
    return torch.cat([items, items.sum().view(1)])


def main():
    import numpy as np
    import torch
    from rtm3d_amd import _lib, loss as L
    from tests import loss_cases as lc
    dev = torch.device('cuda', 0)
    lib = _lib.load()
    rng = np.random.default_rng(11)
    objs = sum([lc._scene(rng, b, PER_IMAGE, H, W) for b in range(B)], [])
    case = lc._case(B, H, W, objs)
    batch = lc.batch(case).to(dev)
    pred = [(torch.randn(B, ch, H, W, device=dev) * 2).contiguous() for ch in (C, 16, 2, 2)]
    pred[0] -= 3.0
    fn = L.RTM3DLoss()
    tg = L.build_targets(batch, H, W)
    fused = fn(pred, batch)[1]
    plain = torch_loss(pred, tg)
    torch.cuda.synchronize()
    rel = ((fused - plain).abs() / plain.abs()).max().item()
    assert rel < 1e-4, (fused, plain)
    stream = _lib.stream_ptr(dev)
    tab, rows, K, start = batch.table(H, W), batch._dev[0], batch._dev[1], batch._dev[2]
    hm = tg['m_hm']

    def timed(f):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        for _ in range(5):
            f()
        t = []
        for _ in range(GROUPS):
            e0.record()
            for _ in range(PER):
                f()
            e1.record()
            e1.synchronize()
            t.append(e0.elapsed_time(e1) * 1000.0 / PER)
        return float(np.median(t)), float(min(t))

    items, counts = torch.empty(5, dtype=torch.float32, device=dev), torch.empty(5, dtype=torch.int32, device=dev)
    ws = torch.empty(int(lib.rtm3d_loss_workspace_bytes(B, C, H, W)), dtype=torch.uint8, device=dev)

    def f_eval_c():
        _lib.check(lib.rtm3d_loss_eval(stream, B, C, H, W, pred[0].data_ptr(), pred[1].data_ptr(), pred[2].data_ptr(), pred[3].data_ptr(),
                                       start.data_ptr(), tab.data_ptr(), batch.N, ctypes.byref(fn._params), ws.data_ptr(), items.data_ptr(),
                                       counts.data_ptr(), None))

    def f_objects():
        _lib.check(lib.rtm3d_loss_objects(stream, batch.N, B, rows.data_ptr(), K.data_ptr(), 4.0, H, W, tab.data_ptr()))

    def f_heatmap():
        _lib.check(lib.rtm3d_loss_heatmap(stream, B, C, H, W, start.data_ptr(), tab.data_ptr(), batch.N, hm.data_ptr()))

    def f_focal_torch():
        return torch_focal(pred[0], hm, 2.0, 4.0)

    res = [('RTM3DLoss(pred, batch): fused target + focal + L1 (2 launches) through the Python wrapper', timed(lambda: fn(pred, batch))),
           ('rtm3d_loss_eval through the C entry point, preallocated outputs', timed(f_eval_c)),
           ('rtm3d_loss_objects (1 launch, once per label batch)', timed(f_objects)),
           ('rtm3d_loss_heatmap, the target materialised (1 launch)', timed(f_heatmap)),
           ('torch focal term on the materialised target (no L1, no sync)', timed(f_focal_torch)),
           ('torch loss on the materialised target (focal + 3 L1 through index tensors)', timed(lambda: torch_loss(pred, tg)))]
    lines = ['validation loss, us per call: median (min) of %d groups of %d back-to-back calls, hipEvent' % (GROUPS, PER),
             'B=%d, %d x %d x %d maps, %d objects (%.1f per image), num_pos %d; fused vs torch items agree to %.1e relative'
             % (B, C, H, W, batch.N, batch.N / B, int(fn.counts[0].item()), rel)]
    lines += ['  %-92s %9.1f (%.1f)' % (n + ':', m, lo) for n, (m, lo) in res]
    other = res[3][1][0] + res[5][1][0]
    lines.append('  fused %.1f us against target + torch %.1f us: %s' % (res[0][1][0], other, 'the fused path is %.1fx faster' % (other / res[0][1][0])
                                                                      if other > res[0][1][0] else 'the fused path is NOT faster'))
    print('\n'.join(lines))
    if len(sys.argv) > 1:
        with open(sys.argv[1], 'a') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
