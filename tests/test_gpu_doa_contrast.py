"""Contrast SRP-PHAT on the MI355X: feature.event_doa with sed.DOA(..., contrast=sed.Contrast(...)) and
feature.event_contrast_frames — the selection against the integer rule from both entries, the plain detector's bits, the
fallback's bits, the contrasted maps against float64, the invariances, the track form and the detector.

One table of rows per recording and time factor (n_classes = 5; the recording has 97 or 99 feature frames, 13 output frames at
time_factor 8).  Row 0 is isolated; row 1 follows row 0 in its class; row 2 lies inside row 3 of another class, which is longer
than max_frames; row 4 starts near the start of the recording; row 5 follows row 6, an activity of its class that is longer than
the search; row 7 has a class the table does not count; row 8 is clipped at the end; row 9 lies beyond the end (it is not
located and, as every row that is not, marks no activity: a row with frames is located by this entry).

Measured on an MI355X over the 54 cases of test_selection_bits_and_maps (contrasted map / its frames against float64): kernel
error 2.1e-8 .. 4.0e-6, kernel / float32 yardstick 0.23 .. 3.47 of the 8 allowed (worst: C = 3, frames 1, hop 1001, oversample 1); no
yardstick was degenerate.  Block maps of the three track cases: 0.55 .. 2.38.  det.localize on the +10 dB scene: the plain dir 2.0
degrees from the interferer, the contrasted dir 2.0 degrees from the target, doa_power 0.113.  """
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import contrast_ref as cr  # noqa: E402
import doa_ref  # noqa: E402
import doa_track_ref as trk  # noqa: E402
from test_gpu_tdoa import DEGENERATE, _bits, _events, _planar, sed  # noqa: E402,F401

pytestmark = pytest.mark.gpu
SR = 44100
N = 96 * 1024 + 300
N_CLASSES = 5
SEARCH = 70
MF = 12
TF_HOP = [(8, 1024), (1, 1024), (1, 1001)]
FRAMES_GUARD = [(1, 0), (8, 2), (33, 1)]
# (onset, offset, peak_frame) in output frames, and the class of every row
ROWS = {1: [(40, 46, 42), (48, 54, 50), (60, 66, 61), (50, 80, 70), (3, 6, 4), (86, 90, 87), (0, 85, 10), (20, 24, 21), (94, 120, 95), (200, 210, 205)],
        8: [(5, 6, 5), (7, 8, 7), (8, 9, 8), (6, 10, 8), (1, 2, 1), (11, 12, 11), (0, 11, 2), (3, 4, 3), (12, 20, 12), (30, 31, 30)]}
CLS = [0, 0, 1, 2, 3, 4, 4, 5, 1, 0]
ISOLATED, AFTER, COVERED, LONG, START, BLOCKED, ACTIVITY, UNCOUNTED, CLIPPED, BEYOND = range(10)


def _array(C):
    return {2: doa_ref.line(2, 0.06), 3: doa_ref.line(3, 0.05), 4: doa_ref.tetrahedron(0.06), 8: doa_ref.line(8, 0.02)}[C]


_REC = {}


def _recording(C, hop, seed=0):
    """(x [N, C], Pk float64, Pk float32) of two far-field sources, computed once per (C, hop)"""
    if (C, seed) not in _REC:
        _REC[C, seed] = doa_ref.far_field(N - 2048 * seed, _array(C), doa_ref.unit(2.2), SR, seed=70 + C + seed) \
            + 0.5 * doa_ref.far_field(N - 2048 * seed, _array(C), doa_ref.unit(-0.7), SR, seed=90 + C + seed)
    x = _REC[C, seed]
    if (C, seed, hop) not in _REC:
        Pk = doa_ref.whitened(x, hop)
        Pk.setflags(write=False)
        _REC[C, seed, hop] = (Pk, doa_ref.whitened_f32(x, hop))
    return (x,) + _REC[C, seed, hop]


def _table(tf, rec=None):
    ev = _events(ROWS[tf], rec)
    ev["cls"] = torch.tensor(CLS, dtype=torch.int32, device="cuda")
    return ev


def _doa(sed, C, Q, ct, mf=MF, track=None):
    return sed.DOA(_array(C), sed.DirectionGrid.ring(24), max_frames=mf, oversample=Q, contrast=ct, track=track)


def _np(got):
    return {k: v.cpu().numpy() for k, v in got.items()}


def _min_frames(frames):
    return min(frames, 2)


def test_the_tables_hold_the_cases_the_rule_has():
    """(host only) what every row of the tables is there for, by the reference's selection"""
    import sed_crnn_amd as s
    for tf, hop in TF_HOP:
        for frames, guard in FRAMES_GUARD:
            ct = s.Contrast(frames, SEARCH, guard, 1)
            bg, sel = cr.frames_of(ROWS[tf], CLS, N, tf, hop, MF, ct, N_CLASSES)
            first = int(hop < 1024 and guard == 0)                          # (candidate 0 then reaches into the event itself)
            assert bg[ISOLATED] == frames and sel[ISOLATED].tolist() == list(range(first, first + frames))[::-1], (tf, hop, frames, guard)
            assert bg[AFTER] == frames and (sel[AFTER, 0] > first + frames - 1 or frames == 1)       # it stepped past the frames of row 0
            alone = cr.frames_of([ROWS[tf][COVERED]], [CLS[COVERED]], N, tf, hop, MF, ct, N_CLASSES)
            assert bg[COVERED] == alone[0][0] == frames and np.array_equal(sel[COVERED], alone[1][0])
            assert 0 < bg[START] and (bg[START] < frames or frames == 1)
            assert cr.frames_of(ROWS[tf], CLS, N, tf, hop, MF, s.Contrast(frames, SEARCH, guard, frames), N_CLASSES)[0][START] == (frames == 1)
            assert bg[BLOCKED] == 0 and bg[ACTIVITY] == 0 and bg[UNCOUNTED] == 0 and bg[BEYOND] == 0 and bg[CLIPPED] == frames


@pytest.mark.parametrize("Q", [1, 8])
@pytest.mark.parametrize("tf,hop", TF_HOP)
@pytest.mark.parametrize("frames,guard", FRAMES_GUARD)
@pytest.mark.parametrize("C", [2, 3, 8])
def test_selection_bits_and_maps(sed, C, frames, guard, tf, hop, Q):
    """the selection from both entries is the rule's; lag, strength, loc_frames and acc are the plain call's bits; a fallback
    event's dir, doa_power and map too; the contrasted maps / frames are within 8 x the float32 yardstick's error of float64 and
    dir is the reference's wherever its two largest values differ by more than that"""
    from sed_crnn_amd import feature
    x, Pk64, Pk32 = _recording(C, hop)
    pcm, clips = _planar(x)
    rows, ev = ROWS[tf], _table(tf)
    ct = sed.Contrast(frames, SEARCH, guard, _min_frames(frames))
    doa = _doa(sed, C, Q, ct)
    kw = dict(sr=SR, hop=hop, return_curve=True, return_map=True)
    plain = _np(feature.event_doa(pcm, clips, C, ev, tf, _doa(sed, C, Q, None), **kw))
    got = _np(feature.event_doa(pcm, clips, C, ev, tf, doa, n_classes=N_CLASSES, **kw))
    assert set(got) == set(plain) | {"bg_frames", "bg_sel"}
    ml, J, _ = doa.plan(SR)
    J = J.astype(np.int64)
    ref = cr.event_doa(Pk64, rows, CLS, N, tf, hop, J, ml, Q, MF, ct, N_CLASSES)
    yard = cr.event_doa(Pk32, rows, CLS, N, tf, hop, J, ml, Q, MF, ct, N_CLASSES, f32=True)
    # the selection, from both entries
    assert got["bg_frames"].dtype == np.int32 and got["bg_sel"].dtype == np.int32 and got["bg_sel"].shape == (len(rows), frames)
    assert np.array_equal(got["bg_frames"], ref["bg_frames"]) and np.array_equal(got["bg_sel"], ref["bg_sel"]), (got["bg_sel"], ref["bg_sel"])
    for M in (ct.min_frames, frames):
        alone = _np(feature.event_contrast_frames(clips, C, ev, tf, _doa(sed, C, Q, sed.Contrast(frames, SEARCH, guard, M)), N_CLASSES, hop=hop))
        want = cr.frames_of(rows, CLS, N, tf, hop, MF, sed.Contrast(frames, SEARCH, guard, M), N_CLASSES)
        assert np.array_equal(alone["bg_frames"], want[0]) and np.array_equal(alone["bg_sel"], want[1]), M
    # the plain detector's bits
    for k in ("lag", "strength", "loc_frames", "acc"):
        assert np.array_equal(got[k].view(np.int32), plain[k].view(np.int32)), k
    assert got["loc_frames"].tolist() == ref["loc_frames"].tolist() and got["loc_frames"][LONG] == MF and got["loc_frames"][BEYOND] == 0
    fallback = got["bg_frames"] == 0
    assert fallback[[BLOCKED, ACTIVITY, UNCOUNTED, BEYOND]].all() and not fallback[[ISOLATED, AFTER, COVERED, LONG, CLIPPED]].any()
    for k in ("dir", "doa_power", "srp"):
        assert np.array_equal(got[k][fallback].view(np.int32), plain[k][fallback].view(np.int32)), k
    assert (got["srp"][~fallback] != plain["srp"][~fallback]).any()
    # against float64
    nf = np.maximum(ref["loc_frames"], 1).astype(np.float64)[:, None]
    live = ref["loc_frames"] > 0
    e_yard = np.abs(yard["srp"].astype(np.float64) / nf - ref["srp"] / nf)[live].max()
    e_kernel = np.abs(got["srp"].astype(np.float64) / nf - ref["srp"] / nf)[live].max()
    assert e_yard >= DEGENERATE, e_yard
    print(f"C={C} frames={frames} guard={guard} tf={tf} hop={hop} Q={Q}: yardstick {e_yard:.2e}  kernel {e_kernel:.2e}  ratio {e_kernel / e_yard:.2f}")
    assert e_kernel <= 8.0 * e_yard, (e_kernel, e_yard)
    P = J.shape[1]
    for e in np.nonzero(live)[0]:
        top = np.sort(ref["srp"][e])[-2:]
        if top[1] - top[0] > 8.0 * e_yard * nf[e, 0]:
            assert got["dir"][e] == ref["dir"][e], (e, got["dir"][e], ref["dir"][e])
        d = got["dir"][e]
        assert abs(float(got["doa_power"][e]) - ref["srp"][e, d] / (P * nf[e, 0])) <= 8.0 * e_yard / P + 2.0 ** -23, e


@pytest.mark.parametrize("C,frames,guard,tf,hop,Q", [(2, 33, 1, 8, 1024, 8), (3, 8, 2, 1, 1001, 1), (8, 1, 0, 1, 1024, 8)])
def test_batch_permutation_workspace_and_foreign_samples_change_no_bit(sed, C, frames, guard, tf, hop, Q):
    from sed_crnn_amd import _lib, feature
    ct = sed.Contrast(frames, SEARCH, guard, _min_frames(frames))
    doa = _doa(sed, C, Q, ct)
    kw = dict(sr=SR, hop=hop, return_curve=True, return_map=True, n_classes=N_CLASSES)
    waves = [_recording(C, hop)[0], _recording(C, hop, seed=1)[0]]
    singles = []
    for w in waves:
        pcm, clips = _planar(w)
        singles.append(feature.event_doa(pcm, clips, C, _table(tf), tf, doa, **kw))
    pieces, clips, at = [], [], 0
    for r, w in enumerate(waves):                                                   # odd offsets, NaN sentinels between the channels
        for c in range(C):
            lead = (-at) % 4 + (3 if r == 1 else 0) + 4
            pieces.append(np.full(lead, np.nan, np.float32))
            at += lead
            clips.append((at, w.shape[0]))
            pieces.append(np.ascontiguousarray(w[:, c]))
            at += w.shape[0]
    pieces.append(np.full(5, np.nan, np.float32))
    buf = torch.from_numpy(np.concatenate(pieces)).cuda()
    E1 = len(CLS)
    ev = {k: torch.cat([v, v]) for k, v in _table(tf).items()}
    ev["rec"] = torch.tensor([0] * E1 + [1] * E1, dtype=torch.int32, device="cuda")
    batch = feature.event_doa(buf, clips, C, ev, tf, doa, **kw)
    for k in batch:                                                                 # the batch is the per-recording calls
        for r in range(2):
            assert np.array_equal(_bits(batch[k][r * E1:(r + 1) * E1]), _bits(singles[r][k])), (k, r)
    perm = torch.from_numpy(np.random.default_rng(5).permutation(2 * E1)).cuda()
    shuffled = feature.event_doa(buf, clips, C, {k: v[perm] for k, v in ev.items()}, tf, doa, **kw)
    for k in batch:                                                                 # a permuted table gives permuted outputs
        assert np.array_equal(_bits(shuffled[k]), _bits(batch[k][perm])), k
    frames_all = int(sum(w.shape[0] // (tf * hop) + 1 for w in waves))
    one = _lib.lib().sed_event_doa_contrast_workspace_bytes(2, C, 1, N, hop, MF, frames_all, frames)
    assert 0 < one < _lib.lib().sed_event_doa_contrast_workspace_bytes(2, C, 2 * E1, N, hop, MF, frames_all, frames)
    small = feature.event_doa(buf, clips, C, ev, tf, doa, max_workspace_bytes=one, **kw)
    for k in batch:                                                                 # the workspace can shrink to one event
        assert np.array_equal(_bits(small[k]), _bits(batch[k])), k
    # every sample outside the events' frames and their selected frames changes no bit
    used = [np.zeros(w.shape[0], bool) for w in waves]
    got = _np(batch)
    for e in range(2 * E1):
        r, (on, off, pk) = e // E1, ROWS[tf][e % E1]
        n = waves[r].shape[0]
        f0, f1 = sed.event_frames(on, off, pk, tf, 1 + n // hop, MF)
        fr = list(range(f0, f1)) + [on * tf - guard - 1 - int(q) for q in got["bg_sel"][e, :got["bg_frames"][e]]]
        for f in fr:
            used[r][max(f * hop - 1024, 0):min(f * hop + 1024, n)] = True
    assert all(u.sum() >= 2048 for u in used) and sum(int((~u).sum()) for u in used) >= 4096     # (33 frames an event can cover a recording)
    noisy = buf.clone()
    rng = np.random.default_rng(9)
    for r, w in enumerate(waves):
        for c in range(C):
            o = clips[r * C + c][0]
            seg = noisy[o:o + w.shape[0]]
            seg[torch.from_numpy(~used[r]).cuda()] = torch.from_numpy(rng.standard_normal(int((~used[r]).sum())).astype(np.float32)).cuda()
    other = feature.event_doa(noisy, clips, C, ev, tf, doa, **kw)
    for k in batch:
        assert np.array_equal(_bits(other[k]), _bits(batch[k])), k


@pytest.mark.parametrize("C,frames,guard,tf,hop,step", [(2, 33, 1, 1, 1001, 30), (4, 8, 2, 1, 1024, None), (8, 8, 2, 8, 1024, 30)])
def test_track_maps_and_path(sed, C, frames, guard, tf, hop, step):
    """with a track (max_frames = 80: up to three blocks of one chunk): the sibling's bits, every contrasted block map / its
    frames within the bound, and the path the float32 restatement run on the device's own maps, exactly"""
    from sed_crnn_amd import feature
    Q, mf, W = 8, 80, 1
    x, Pk64, Pk32 = _recording(C, hop)
    pcm, clips = _planar(x)
    rows = list(ROWS[tf])
    rows[LONG] = (8, 90, 40) if tf == 1 else (1, 11, 5)                             # 80 frames: three blocks
    cls = list(CLS)
    cls[ACTIVITY] = N_CLASSES                                                       # (its class would block the long event's candidates)
    ev = _events(rows)
    ev["cls"] = torch.tensor(cls, dtype=torch.int32, device="cuda")
    ct = sed.Contrast(frames, SEARCH, guard, _min_frames(frames))
    track = sed.DirectionTrack(W, step)
    doa = _doa(sed, C, Q, ct, mf, track)
    kw = dict(sr=SR, hop=hop, return_curve=True, return_map=True)
    got = _np(feature.event_doa(pcm, clips, C, ev, tf, doa, n_classes=N_CLASSES, **kw))
    flat = _np(feature.event_doa(pcm, clips, C, ev, tf, _doa(sed, C, Q, ct, mf), n_classes=N_CLASSES, **kw))
    plain = _np(feature.event_doa(pcm, clips, C, ev, tf, _doa(sed, C, Q, None, mf, track), **kw))
    for k in flat:                                                                  # the entry without a track, bit for bit
        assert np.array_equal(got[k].view(np.int32), flat[k].view(np.int32)), k
    fallback = got["bg_frames"] == 0
    assert fallback.any() and not fallback.all() and got["trk_len"][LONG] == 3 and not fallback[LONG]
    for k in ("trk_len", "trk_raw", "trk_dir", "trk_power", "trk_map"):
        assert np.array_equal(got[k][fallback].view(np.int32), plain[k][fallback].view(np.int32)), k
    ml, J, _ = doa.plan(SR)
    J = J.astype(np.int64)
    table = doa.neighbours() or (None, None)
    e_kernel = e_yard = 0.0
    for e, (on, off, pk) in enumerate(rows):
        f0, f1 = sed.event_frames(on, off, pk, tf, Pk64.shape[0], mf)
        nb, sel = int(got["bg_frames"][e]), got["bg_sel"][e]
        ref, raw, power = cr.block_maps(Pk64, f0, f1 - f0, W, J, ml, Q, on, tf, ct, nb, sel)
        yard, _, _ = cr.block_maps(Pk32, f0, f1 - f0, W, J, ml, Q, on, tf, ct, nb, sel)
        T = len(raw)
        assert got["trk_len"][e] == T
        if T:
            per = np.array([n for _, n in trk.blocks(f1 - f0, W)], np.float64)[:, None]
            e_yard = max(e_yard, np.abs(yard.astype(np.float64) / per - ref / per).max())
            e_kernel = max(e_kernel, np.abs(got["trk_map"][e, :T].astype(np.float64) / per - ref / per).max())
        want = trk.track_dir(got["trk_map"][e, :T], got["trk_raw"][e, :T], *table)
        assert np.array_equal(got["trk_dir"][e, :T], want), (e, got["trk_dir"][e, :T], want)
        assert np.array_equal(got["trk_raw"][e, :T], got["trk_map"][e, :T].argmax(1)) or f1 == f0
    assert e_yard >= DEGENERATE
    print(f"C={C} frames={frames} tf={tf} hop={hop}: block maps: yardstick {e_yard:.2e}  kernel {e_kernel:.2e}  ratio {e_kernel / e_yard:.2f}")
    assert e_kernel <= 8.0 * e_yard, (e_kernel, e_yard)


def test_detector_localize_on_the_scene(sed):
    """det.localize on the +10 dB scene at C = 4: dir within 5 degrees of the target, the plain detector's within 5 of the
    interferer; with extract=sed.DelaySum() the audio is that of a detector handed that dir, bit for bit; res.bg_frames"""
    from sed_crnn_amd import feature
    from sed_crnn_amd.detect import DetectionResult, plan_windows
    net = sed.LightningTimePooledCRNN(dropout=0.0, in_channels=4, n_mels=40).cuda().eval()
    tf = net.time_factor
    target = (24, 24 + 12 * tf // math.gcd(12, tf)) if 12 % tf else cr.TARGET       # the target ends on an output frame
    tg, ot = cr.PAIRS_DEG[0]
    x = cr.scene(tg, ot, 10.0, 100, target=target)
    grid = sed.DirectionGrid.ring(cr.RING)
    ct = sed.Contrast(frames=16, search=64, guard=2, min_frames=8)
    beam = sed.DelaySum()

    def detector(contrast, extract=None):
        doa = sed.DOA(doa_ref.tetrahedron(cr.EDGE), grid, oversample=cr.Q, contrast=contrast)
        return sed.EventDetector(net, mean=np.zeros(160, np.float32), std=np.ones(160, np.float32), localize=doa, extract=extract), doa

    def result():
        K = net.dense[-1]
        ev = {"cls": torch.zeros(1, dtype=torch.int32, device="cuda"), "onset": torch.tensor([target[0] // tf], dtype=torch.int32, device="cuda"),
              "offset": torch.tensor([target[1] // tf], dtype=torch.int32, device="cuda"), "peak": torch.ones(1, device="cuda"),
              "peak_frame": torch.tensor([target[0] // tf], dtype=torch.int32, device="cuda")}
        n_feat = 1 + x.shape[0] // cr.HOP
        plan = plan_windows(n_feat, tf, det.seq_len, det.hop, det.trim)
        return DetectionResult(torch.zeros(plan.n_out, K, device="cuda"), ev, det.frame_seconds, plan)

    det, doa = detector(ct, beam)
    assert det.sr == cr.SR and det.hop_length == cr.HOP and target[0] % tf == 0 and target[1] % tf == 0
    res = det.localize(result(), x, channels=4)
    plain = detector(None)[0].localize(result(), x, channels=4)
    units = grid.unit_vectors
    off = lambda d, deg: math.degrees(doa_ref.angle_between(units[int(d)], doa_ref.unit(math.radians(deg))))      # noqa: E731
    print(f"plain dir {off(plain.events['dir'][0], ot):.1f} deg from the interferer, contrasted dir {off(res.events['dir'][0], tg):.1f} deg from "
          f"the target; doa_power {float(res.events['doa_power'][0]):.3f}, bg_frames {res.bg_frames.tolist()}")
    assert off(plain.events["dir"][0], ot) <= 5.0 and off(res.events["dir"][0], tg) <= 5.0
    assert res.bg_frames is res.events["bg_frames"] and res.bg_frames.tolist() == [16] and res.events["bg_sel"].shape == (1, 16)
    with pytest.raises(AttributeError, match="bg_frames"):
        plain.bg_frames
    # the audio is that of a detector handed that dir
    pcm, clips = _planar(x)
    handed = feature.event_beamform(pcm, clips, 4, res.events, tf, doa, beam, sr=cr.SR, hop=cr.HOP)
    assert res.audio.numel() > 0 and np.array_equal(_bits(res.audio), _bits(handed["audio"]))
    with pytest.raises(NotImplementedError, match="follow-up"):
        det.stream(1, history_frames="min", emit_audio=True)
