"""Case tables of the track-drawing tests (tests/test_draw_tracks_cpu.py checks their conditions on the CPU,
tests/test_gpu_draw_tracks.py runs them on the device against tests/draw_tracks_ref.py).  A case = dict(name, hw, rec (B, topk, 32)
fp32, ids (B, topk) int32, K or None, state (B, 8 + 24 T) fp64 or None, params = keywords of draw_tracks_ref.draw /
TrackDrawParams, seed of the background, expect = the statistics of the yardstick that must be non-zero).  Frames are the small
ragged ones of tests/draw_cases.py; the sizes that matter are the kernel's: 64 x 16 tiles, rounds of 256 items, 29 label items and
14 track items per slot."""
import numpy as np

from tests import draw_cases as dc
from tests import draw_tracks_ref as ref

PALETTE3 = [(250, 250, 250), (10, 20, 200), (255, 208, 0)]          # white-ish (black ink), dark blue (white ink), yellow
NAMES = [b'Car', b'pedestrian', b'cy~l-st']                          # lower case, more than 7 bytes, a byte outside the set
LABEL_STATS = ('label_bg', 'label_glyph', ref.FACE, ref.BOX2D, ref.WIREFRAME, ref.KEYPOINT)      # every label case paints the frame layers too


def backgrounds(case):
    rng = np.random.Generator(np.random.PCG64(case['seed']))
    imgs = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in case['hw']]
    bev = None
    if case['params']['layers'] & (ref.BEV | ref.TRACK_BEV):
        bh, bw = case['params']['bev_hw']
        bev = rng.integers(1, 64, (len(imgs), bh, bw, 3), dtype=np.uint8)
    return imgs, bev


def _params(**kw):
    p = dict(layers=dc.ALL_FRAME | ref.LABEL, colors=dc.COLORS, palette=PALETTE3, names=NAMES, label_fields=15, font_scale=1)
    p.update(kw)
    return p


def _flat(x, y, cls, flag, score=0.9, z=12.34):
    """A record whose box has its corner (x1, y1) at (x, y); the cuboid sits below and right of it."""
    r = dc.record(cls, (x + 9.5, y + 7.5), dc.cuboid(x + 10, y + 8, 6, 4, 3, -2), (x, y, x + 20.5, y + 15.5), flag, score=score)
    r[24:31] = (1.5, 1.6, 3.9, 1.0, 1.2, z, 0.3)
    return r


def _labels_tiny():
    """37 x 53, the records of draw_cases' tiny: slot 0's corner at (-5, 3) - a negative anchor and too little room above, so the
    label goes inside; slot 1's box off the frame; slot 2's x2 = 9000 leaves the anchor alone.  A confirmed, a tentative and an
    untracked slot."""
    t = [c for c in dc.cases() if c['name'] == 'tiny'][0]
    return dict(name='labels_tiny', hw=t['hw'], rec=t['rec'], ids=np.array([[3, -5, 0]], np.int32), K=None, state=None, seed=21,
                params=_params(thickness=2), expect=LABEL_STATS)


def _scale3_cross():
    """101 x 223: a scale-3 label above a box at (40, 30): rows 3..29 cross the tile row 16, columns 40.. cross the tile column 64."""
    rec = np.stack([_flat(40.7, 30.2, 1, 2), _flat(120.2, 70.9, 0, 1)])[None]
    return dict(name='scale3_cross', hw=[(101, 223)], rec=rec, ids=np.array([[12, -1]], np.int32), K=None, state=None, seed=22,
                params=_params(font_scale=3, label_fields=3), expect=LABEL_STATS)


def _two_rounds():
    """topk = 10: the label pass has 290 items; slot 1 (the ninth painted) owns items 232..260, so its 26 characters straddle
    item 256 - characters 0..22 in the first round, 23..25 in the second."""
    rec = np.stack([_flat(10.5 + 17 * (s % 3), 12.5 + 9 * s, s % 3, 2, score=0.5 + 0.04 * s, z=10.0 + s) for s in range(10)])[None]
    ids = np.array([[5, 1234567, -3, 0, 8, 9, -10, 11, 12, 9999999]], np.int32)
    rec[0, 1, 0] = 1.0                                   # PEDESTR: '#1234567 PEDESTR 54% 11.0M'
    return dict(name='two_rounds', hw=[(101, 223)], rec=rec, ids=ids, K=None, state=None, seed=23, params=_params(), expect=LABEL_STATS)


def _clipped():
    """37 x 53 at scale 4 (labels 36 rows high): corners at (-7, 20) - left edge, inside, cut by the bottom edge; (40, 12) - right
    edge; (10, -5) - a negative row, cut by the top edge."""
    rec = np.stack([_flat(-7.5, 20.5, 0, 2), _flat(40.5, 12.5, 1, 1), _flat(10.5, -5.5, 2, 2)])[None]
    return dict(name='clipped', hw=[(37, 53)], rec=rec, ids=np.array([[1, 2, -3]], np.int32), K=None, state=None, seed=24,
                params=_params(font_scale=4, label_fields=1), expect=LABEL_STATS)


def _ids_mix():
    """draw_cases' ragged with every frame layer, labels and the RECORD-driven panel: ids beyond npal = 3 (wrap), negative ids
    (dimmed, '?'), id 0 beside tracked slots, an empty slot."""
    t = [c for c in dc.cases() if c['name'] == 'ragged'][0]
    ids = np.array([[7, -2, 0, 40, 0], [0, 3, -33, 0, 0]], np.int32)
    p = dict(t['params'], layers=dc.ALL_FRAME | ref.BEV | ref.LABEL, palette=PALETTE3, names=NAMES, label_fields=7, font_scale=2)
    return dict(name='ids_mix', hw=t['hw'], rec=t['rec'], ids=ids, K=t['K'], state=None, seed=25, params=p,
                expect=LABEL_STATS + (ref.BEV,))


def track_slot(tid, box, vel=(0.0, 0.0, 0.0), hits=3, misses=0, cls=0):
    s = np.zeros(ref.SLOT)
    s[0], s[1], s[2], s[3], s[4], s[5], s[6] = tid, cls, 5, hits, misses, 0.8, -1 if misses else 0
    s[7:14] = box
    s[14:17] = vel
    s[17:22] = (1.0, 0.1, 2.0, 0.5, 0.5)
    return s


def track_margins_ok(slot, bev_hw, m, vel_horizon):
    pts = ref.track_points(slot, bev_hw, m, vel_horizon if vel_horizon > 0 else 1.0).ravel()
    pts = pts[np.isfinite(pts) & (np.abs(pts) < 1e6)]
    return bool(np.all(np.abs(pts - np.round(pts)) >= dc.MARGIN))


def _track_table(rng, bev_hw, m, vh, specs):
    """(8 + 24 T,) table: specs = per slot None (free) or dict(id, hits, misses, vel or 'nan'); boxes redrawn until every mapped
    coordinate keeps the margin (met by construction)."""
    out = np.zeros(ref.HEADER + ref.SLOT * len(specs))
    out[0], out[1] = 50, 9
    for t, sp in enumerate(specs):
        if sp is None:
            continue
        while True:
            box = np.array([rng.uniform(1.3, 1.9), rng.uniform(1.5, 1.9), rng.uniform(3.2, 4.6), rng.uniform(-14, 14), rng.uniform(0.8, 1.6),
                            rng.uniform(4, 30), rng.uniform(-3.1, 3.1)])
            vel = np.array([rng.uniform(-3, 3), 0.0, rng.uniform(-3, 3)])
            s = track_slot(sp['id'], box, vel, sp['hits'], sp['misses'])
            if track_margins_ok(s, bev_hw, m, vh):
                break
        if sp.get('vel') == 'nan':
            s[14] = np.nan
        out[ref.HEADER + ref.SLOT * t:ref.HEADER + ref.SLOT * (t + 1)] = s
    return out


def _track_panel(name, **kw):
    """Two streams, T = 5, a hand-made table: slot 2 free between live ones; slot 1 coasting (misses 1, hits 0: tentative, no record
    of this frame); slot 3's velocity NaN (its mark is skipped, its footprint drawn); stream 1 differs.  The 70 x 200 panel has 20
    tiles, most of them untouched.  The records are the two flat boxes of every frame case: the panel does not read them."""
    rng = np.random.Generator(np.random.PCG64(31))
    bev_hw, m = (70, 200), 0.4
    vh = kw.get('vel_horizon', 2.0)
    specs0 = [dict(id=4, hits=3, misses=0), dict(id=17, hits=0, misses=1), None, dict(id=2, hits=6, misses=0, vel='nan'), dict(id=1234567, hits=1, misses=0)]
    specs1 = [None, dict(id=9, hits=0, misses=2), dict(id=3, hits=2, misses=0), None, None]
    state = np.stack([_track_table(rng, bev_hw, m, vh, specs0), _track_table(rng, bev_hw, m, vh, specs1)])
    rec = np.stack([np.stack([_flat(8.5, 14.5, 0, 2), _flat(20.5, 20.5, 1, 1)])] * 2)
    p = _params(layers=ref.BOX2D | ref.TRACK_BEV, bev_hw=bev_hw, bev_m_per_px=m, vel_horizon=2.0, label_fields=1)
    p.update(kw)
    expect = ['track_box', 'track_head'] + (['track_vel'] if p['vel_horizon'] > 0 else []) + (['track_text'] if p['label_fields'] & 1 else []) \
        + ([ref.BOX2D] if p['layers'] & ref.BOX2D else [])
    return dict(name=name, hw=[(37, 53), (37, 53)], rec=rec, ids=np.array([[4, 0], [0, -3]], np.int32), K=None, state=state, seed=26,
                params=p, expect=tuple(expect))


def cases():
    return [_labels_tiny(), _scale3_cross(), _two_rounds(), _clipped(), _ids_mix(), _track_panel('track_panel'),
            _track_panel('track_no_velocity', vel_horizon=0.0), _track_panel('track_fade', bev_fade=200),
            _track_panel('track_only', layers=ref.TRACK_BEV, label_fields=0, font_scale=2)]
