"""The PSDS sweep on the MI355X (sed_crnn_amd/tune.py, csrc/psds.hip) against the interval-list restatement of
tests/psds_ref.py and against the real decoder.  Counts and cross triggers are integers: every comparison of them is exact
equality; the score is compared to 1e-12 relative (two float64 sums of at most a few thousand terms).

The data: R = 5 recordings of 1, 63, 64, 65 and 700 output frames (a one-frame recording, both sides of a word boundary), a
seeded smooth random track, and in the long recording classes 0 and 1 written by hand (0.9 on, 0.1 off) so that setting 0
(median 1, threshold 0.5, no gap merge, no minimum length) detects exactly the planted events of ``PLANTED``."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import detect_ref  # noqa: E402
import psds_ref  # noqa: E402
import tune_ref  # noqa: E402

pytestmark = pytest.mark.gpu

LENGTHS = (1, 63, 64, 65, 700)
LONG = 4                                                               # the recording that carries the planted events
CRITERIA = ((700, 700, 0), (100, 100, 300), (1000, 1, 1000))           # (dtc, gtc, cttc) in thousandths
TAIL = [(460 + 3 * i, 462 + 3 * i) for i in range(70)]                 # 70 short reference events: past the 64 staged in LDS
PLANTED = dict(
    # class 0 detections of the long recording under setting 0
    det0=[(10, 20), (30, 40), (53, 60), (74, 80), (90, 100), (110, 120), (130, 140), (150, 160), (170, 180), (182, 188), (199, 200),
          (220, 222), (230, 240), (244, 254), (260, 310), (325, 334), (338, 350), (365, 380), (400, 410), (500, 530), (559, 561),
          (600, 640), (650, 652)],
    # class 0 reference events.  Ties, passing at the boundary / failing one frame short:
    #   dtc 700: [10,20) ∩ [13,20) = 7 of 10 / [30,40) ∩ [34,40) = 6       dtc 100: [90,100) ∩ [99,100) = 1 / [110,120): 0
    #   dtc 1000: [150,160) = the event / [170,180) ∩ [171,180) = 9
    #   gtc 700: [50,60) covered by [53,60): 7 of 10 / [70,80) by [74,80): 6
    #   gtc 100 and 1: [190,200) covered by [199,200): 1 of 10 / [210,220) touched by [220,222): 0
    # [260,310) spans four reference events (two of them touching), 46 of its 50 frames; [330,370) is reached by three
    # detections with 4 of 9, 12 of 12 and 5 of 15 frames inside: only some are relevant at dtc 700 and 1000, all at 100;
    # [385,390) is reached by nothing, [400,410) reaches nothing
    ref0=[(13, 20), (34, 40), (50, 60), (70, 80), (99, 100), (150, 160), (171, 180), (190, 200), (210, 220), (260, 272), (272, 280),
          (282, 294), (296, 310), (330, 370), (385, 390)] + TAIL,
    # class 1 (K >= 3): the cross-trigger ties of the class-0 false positives
    #   cttc 300: [110,120) ∩ [117,120) = 3 of 10 / [130,140) ∩ [138,140) = 2
    #   cttc 1000: [170,180) whole / [182,188) ∩ [182,187) = 5 of 6        cttc 700: [230,240): 7 of 10 / [244,254): 6 of 10
    ref1=[(117, 120), (138, 140), (170, 180), (182, 187), (233, 240), (248, 254)],
    det1=[(52, 58)])                                                   # inside class 0's [50,60): a cross trigger 1 -> 0


@pytest.fixture(scope="module")
def sed():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    import sed_crnn_amd as s
    return s


def _grid(sed):
    """G = 12: medians {1, 5} x min_gap {0, 2} x min_len {1, 3} at threshold 0.5, then medians x min_gap with hysteresis"""
    sets = [dict(threshold=0.5, median=m, min_gap=g, min_len=n) for m in (1, 5) for g in (0, 2) for n in (1, 3)]
    sets += [dict(threshold=0.6, low=0.5, median=m, min_gap=g, min_len=1) for m in (1, 5) for g in (0, 2)]
    grid = sed.DecoderGrid.from_settings(sets)
    assert len(grid) == 12 and grid[0] == dict(threshold=0.5, low=0.5, median=1, min_gap=0, min_len=1)
    return grid


def _smooth(rng, n, K, scale=0.12):
    """a slow random track around the thresholds; six frames far below them every 80 keep every event under 80 frames"""
    walk = np.cumsum(rng.standard_normal((n, K)) * scale, 0) + rng.uniform(0, 6.28, K)
    p = ((1 / (1 + np.exp(-np.sin(walk)))) * 0.6 + 0.2).astype(np.float32)
    for a in range(74, n, 80):
        p[a:a + 6] = 0.05
    return p


_CASES, _WANT = {}, {}


def _case(sed, K):
    """(tracks, ref lists, grid, decoded events per setting) of K classes, built once"""
    if K in _CASES:
        return _CASES[K]
    rng = np.random.default_rng(40 + K)
    grid = _grid(sed)
    tracks = [_smooth(rng, n, K) for n in LENGTHS]
    hand = min(K, 2)                                                   # the classes of the long recording written by hand
    tracks[LONG][:, :hand] = 0.1
    for k, name in ((0, "det0"), (1, "det1"))[:hand]:
        for a, b in PLANTED[name]:
            tracks[LONG][a:b, k] = 0.9
    # reference events: the decode of a perturbed copy (matches, near misses and misses all occur) ...
    ref = []
    for t in tracks:
        p = np.roll(t, int(rng.integers(-2, 3)), 0) + rng.standard_normal(t.shape).astype(np.float32) * 0.03
        ref.append(tune_ref.events_to_ref([detect_ref.decode(p.astype(np.float32), lo=0.45, hi=0.55, median=3, min_gap=1)], K)[0])
    ref[1] = [[] for _ in range(K)]                                    # ... a recording with no reference
    ref[2][0] = [(0, LENGTHS[2])]                                      # one event covering a whole recording
    ref[LONG][0] = list(PLANTED["ref0"])
    if K >= 3:
        ref[LONG][1] = list(PLANTED["ref1"])
        for r in range(len(ref)):
            ref[r][K - 1] = []                                         # a class with no reference at all
    probs, out_off = np.ascontiguousarray(np.concatenate(tracks), np.float32), np.concatenate([[0], np.cumsum(LENGTHS)]).tolist()
    decoded = [tune_ref.decode_all(probs, out_off, s) for s in grid]
    # the data is what the module docstring says it is
    got = psds_ref.by_class(decoded[0][LONG], K)
    assert got[0] == PLANTED["det0"] and (K < 3 or got[1] == PLANTED["det1"])
    assert len(ref[LONG][0]) > 64 and (272, 280) in ref[LONG][0] and (260, 272) in ref[LONG][0]
    lengths = [b - a for per_rec in decoded for ev in per_rec for a, b in zip(ev["onset"], ev["offset"])]
    print(f"K={K}: events of {min(lengths)} to {max(lengths)} frames")
    assert min(lengths) == 1 and 50 <= max(lengths) <= 80, (min(lengths), max(lengths))
    _CASES[K] = (tracks, ref, grid, decoded, probs, out_off)
    return _CASES[K]


def _want(sed, K, crit):
    """the reference's (counts [G, K, 4], ct [G, K, K]), computed once per (K, criteria) and never changed"""
    if (K, crit) not in _WANT:
        _, ref, grid, decoded, _, _ = _case(sed, K)
        both = [psds_ref.counts(ev, ref, K, *crit) for ev in decoded]
        c, ct = np.stack([b[0] for b in both]), np.stack([b[1] for b in both])
        c.setflags(write=False)
        ct.setflags(write=False)
        _WANT[K, crit] = (c, ct)
    return _WANT[K, crit]


def _criteria(sed, crit):
    return sed.PSDSCriteria(crit[0] / 1000, crit[1] / 1000, crit[2] / 1000 if crit[2] else None)


def _sweep(sed, K, crit, order=None, **kw):
    tracks, ref, grid, _, _, _ = _case(sed, K)
    order = list(range(len(tracks))) if order is None else order
    probs = np.ascontiguousarray(np.concatenate([tracks[i] for i in order]), np.float32)
    out_off = np.concatenate([[0], np.cumsum([LENGTHS[i] for i in order])]).tolist()
    robj = sed.ReferenceEvents([ref[i] for i in order], [LENGTHS[i] for i in order], K)
    return sed.psds_sweep((torch.from_numpy(probs).cuda(), out_off), robj, grid, _criteria(sed, crit), 0.16, **kw)


# ───────────── 1. counts and cross triggers against the reference ─────────────
@pytest.mark.parametrize("crit", CRITERIA + ((700, 700, 700),), ids=lambda c: "-".join(map(str, c)))
@pytest.mark.parametrize("K", [1, 3, 32])
def test_counts_and_cross_triggers_equal_the_reference(sed, K, crit):
    want_c, want_ct = _want(sed, K, crit)
    res = _sweep(sed, K, crit)
    got_c, got_ct = res.table()
    assert got_c.dtype == np.int64 and got_c.shape == (12, K, 4) and got_ct.dtype == np.int64 and got_ct.shape == (12, K, K)
    for g in range(12):
        print(f"K={K} {crit} setting {g}: counts {got_c[g].sum(0).tolist()} want {want_c[g].sum(0).tolist()}, ct {int(got_ct[g].sum())} want "
              f"{int(want_ct[g].sum())}")
    np.testing.assert_array_equal(got_c, want_c)
    np.testing.assert_array_equal(got_ct, want_ct)
    assert res.n_slices == 1 and res.n_tracks == 4                       # medians (1 | 5) x thresholds (0.5 | 0.6)
    # every kind of outcome occurs: hits, misses, false positives and, with a criterion and another class, cross triggers
    assert (want_c[..., 0] > 0).any() and (want_c[..., 0] < want_c[..., 1]).any() and (want_c[..., 3] > 0).any()
    assert (want_c[..., 3] < want_c[..., 2]).any() and (np.diagonal(want_ct, axis1=1, axis2=2) == 0).all()
    assert (want_ct > 0).any() == (crit[2] > 0 and K > 1)
    if K >= 3:
        assert (want_c[:, K - 1, 1] == 0).all() and (want_c[:, K - 1, 2] > 0).any()      # detections, but no reference at all


def test_the_planted_ties_fall_on_the_side_the_definition_says(sed):
    """setting 0 on the long recording, class 0 (and class 1 as the cross-trigger target): hand-derived from PLANTED"""
    _, ref, _, decoded, _, _ = _case(sed, 3)
    sys0, ref_long = psds_ref.by_class(decoded[0][LONG], 3), ref[LONG]
    # (700, 700, 700).  Relevant: [10,20) [53,60) [74,80) [150,160) [170,180) [199,200) [260,310) [338,350) [559,561); true
    # positives: [13,20) [50,60) (7 of 10) [150,160) [171,180), the four under [260,310), [559,561) -> 9; not [70,80) (6 of 10),
    # [190,200) (1 of 10), [330,370) (12 of 40).  14 false positives; cross triggers 0 -> 1: [170,180) is relevant here, so
    # [182,188) (5 of 6) and [230,240) (7 of 10), not [244,254) (6 of 10)
    c, ct = psds_ref.counts_one(sys0, ref_long, 700, 700, 700)
    assert c[0] == [9, 85, 23, 14] and ct[0] == [0, 2, 0] and ct[1] == [1, 0, 0]
    # (1000, 1, 1000): relevant are the detections inside the reference: [53,60) [74,80) [150,160) [199,200) [338,350) [559,561)
    c, ct = psds_ref.counts_one(sys0, ref_long, 1000, 1, 1000)
    assert c[0] == [6, 85, 23, 17] and ct[0] == [0, 1, 0] and ct[1] == [1, 0, 0]        # 0 -> 1: [170,180) whole, [182,188) one short
    # (100, 100, 300): [110,120) [130,140) [182,188) [220,222) [230,240) [244,254) [400,410) stay false positives
    c, ct = psds_ref.counts_one(sys0, ref_long, 100, 100, 300)
    assert c[0][3] == 7 and ct[0] == [0, 4, 0]                           # [110,120) 3 of 10, [182,188), [230,240), [244,254); not [130,140)
    for crit in ((700, 700, 700), (1000, 1, 1000), (100, 100, 300)):
        got_c, got_ct = _sweep(sed, 3, crit, order=[LONG]).table()
        want_c, want_ct = psds_ref.counts_one(sys0, ref_long, *crit)
        assert got_c[0].tolist() == want_c and got_ct[0].tolist() == want_ct, crit


# ───────────── 2. invariances ─────────────
def test_equal_counts_for_a_permuted_recording_order_and_for_one_or_three_grid_slices(sed):
    from sed_crnn_amd._lib import lib
    K, crit = 3, (100, 100, 300)
    want_c, want_ct = _want(sed, K, crit)
    for order in ([4, 2, 0, 3, 1], [1, 0, 3, 4, 2]):
        got_c, got_ct = _sweep(sed, K, crit, order=order).table()
        np.testing.assert_array_equal(got_c, want_c, err_msg=str(order))
        np.testing.assert_array_equal(got_ct, want_ct, err_msg=str(order))
    # settings 0..3 read (1, 0.5), 4..7 (5, 0.5), 8..11 two tracks each, four in all: a budget of 3 tracks cuts after setting 7
    # (the ninth setting's 16 bytes no longer fit) and after setting 9 (a fourth track)
    budget = lib().sed_psds_workspace_bytes(sum(LENGTHS), K, len(LENGTHS), 3, 4)
    res = _sweep(sed, K, crit, max_workspace_bytes=budget)
    assert res.n_slices == 3 and res.workspace_bytes <= budget
    np.testing.assert_array_equal(res.table()[0], want_c)
    np.testing.assert_array_equal(res.table()[1], want_ct)
    again = _sweep(sed, K, crit)
    assert again.n_slices == 1 and torch.equal(again.counts.cpu(), res.counts.cpu()) and torch.equal(again.ct.cpu(), res.ct.cpu())


def test_ct_is_untouched_without_a_cross_trigger_criterion(sed):
    from sed_crnn_amd._lib import TuneSetting, check, lib, ptr, stream_ptr
    K = 3
    _, ref, grid, _, probs, out_off = _case(sed, K)
    L = lib()
    robj = sed.ReferenceEvents(ref, LENGTHS, K)
    d_off, d_on, d_offs = robj.device("cuda")
    dprobs = torch.from_numpy(probs).cuda()
    n_out = np.ascontiguousarray(np.asarray(LENGTHS, np.int64))
    arr = (TuneSetting * 12)(*[TuneSetting(s["median"], s["low"], s["threshold"], s["min_gap"], s["min_len"]) for s in grid])
    ws = torch.empty(L.sed_psds_workspace_bytes(sum(LENGTHS), K, len(LENGTHS), grid.n_tracks(), 12), dtype=torch.uint8, device="cuda")
    counts = torch.full((12, K, 4), -7, dtype=torch.int64, device="cuda")        # counts are cleared by the call, ct is not
    ct = torch.full((12, K, K), -7, dtype=torch.int64, device="cuda")

    def call(cttc, ct_arg):
        check(L.sed_psds_sweep(ptr(dprobs), C.c_void_p(n_out.ctypes.data), len(LENGTHS), K, C.cast(arr, C.c_void_p), 12, ptr(d_off),
                               ptr(d_on), ptr(d_offs), 700, 700, cttc, ptr(ws), ws.numel(), ptr(counts), ct_arg, stream_ptr()),
              "sed_psds_sweep")
        torch.cuda.synchronize()

    call(0, ptr(ct))
    assert (ct == -7).all()
    np.testing.assert_array_equal(counts.cpu().numpy(), _want(sed, K, (700, 700, 0))[0])
    call(0, None)                                                        # and it may be NULL
    np.testing.assert_array_equal(counts.cpu().numpy(), _want(sed, K, (700, 700, 0))[0])
    call(700, ptr(ct))                                                   # with a criterion it is cleared and written
    np.testing.assert_array_equal(ct.cpu().numpy(), _want(sed, K, (700, 700, 700))[1])
    np.testing.assert_array_equal(counts.cpu().numpy(), _want(sed, K, (700, 700, 700))[0])


# ───────────── 3. the public path and the real decoder ─────────────
@pytest.mark.parametrize("scenario", ["scenario1", "scenario2"])
def test_detector_psds_is_the_reference_score_of_the_real_decoders_events(sed, scenario):
    """the criteria of the two presets with e_max = 5000 per hour: the five recordings last under three minutes, so ONE false
    positive is already 22 per hour and e_max = 100 would leave the area almost empty"""
    K = 3
    _, ref, _, _, probs, out_off = _case(sed, K)
    model = sed.LightningTimePooledCRNN(dropout=0.0, n_classes=K).cuda().eval()
    det = sed.EventDetector(model, median=5, min_gap=2, min_len=2)
    preset = getattr(sed.PSDSCriteria, scenario)()
    crit = sed.PSDSCriteria(preset.dtc, preset.gtc, preset.cttc, preset.alpha_ct, preset.alpha_st, e_max=5000.0)
    robj = sed.ReferenceEvents(ref, LENGTHS, K)
    dprobs = torch.from_numpy(probs).cuda()
    thresholds = np.linspace(0.3, 0.7, 9)
    res = det.psds((dprobs, out_off), robj, thresholds=thresholds, criteria=crit)
    assert len(res) == 9 and res.grid[3] == dict(threshold=float(thresholds[3]), low=float(thresholds[3]), median=5, min_gap=2, min_len=2)
    tf = model.time_factor
    bp = sed.plan_batch([tf * n for n in LENGTHS], tf, K)                # decode_many takes R and out_off from it
    assert list(bp.out_off) == out_off
    want_c, want_ct = [], []
    for g in range(len(res)):
        ev, offs = det.with_decoder(**res.grid[g]).decode_many(dprobs, bp)
        ev = {k: v.cpu().numpy() for k, v in ev.items()}
        per_rec = [{k: ev[k][offs[r]:offs[r + 1]] for k in ("cls", "onset", "offset")} for r in range(len(LENGTHS))]
        c, ct = psds_ref.counts(per_rec, ref, K, crit.dtc_milli, crit.gtc_milli, crit.cttc_milli)
        want_c.append(c)
        want_ct.append(ct)
    got_c, got_ct = res.table()
    np.testing.assert_array_equal(got_c, np.stack(want_c))
    np.testing.assert_array_equal(got_ct, np.stack(want_ct))
    want = psds_ref.score(got_c, got_ct, LENGTHS, ref, det.frame_seconds, crit.cttc_milli, crit.alpha_ct, crit.alpha_st, crit.e_max)
    print(f"{scenario}: PSDS {res.psds()!r}, reference {want['psds']!r}")
    assert want["psds"] > 0.05 and len(want["e"]) >= 8 and abs(res.psds() - want["psds"]) <= 1e-12 * abs(want["psds"])
    e, mean, std, etpr = res.curve()
    np.testing.assert_allclose(e, want["e"], rtol=1e-12, atol=0)
    np.testing.assert_allclose(etpr, want["etpr"], rtol=1e-12, atol=1e-15)
    assert res.kept_classes().tolist() == want["kept"] == [0, 1]          # class 2 has no reference
    # the default is 50 thresholds and scenario 1; an explicit grid overrides the thresholds
    if scenario == "scenario1":
        default = det.psds((dprobs, out_off), robj)
        assert len(default) == 50 and default.criteria.dtc_milli == 700 and default.criteria.e_max == 100.0
        explicit = det.psds((dprobs, out_off), robj, thresholds=3, grid=res.grid)
        assert torch.equal(explicit.counts, res.counts)


def test_the_decoder_sweep_still_returns_its_reference_on_the_same_inputs(sed):
    """tune_refblocks_k and the track pool moved into tune_shared.h: sed_tune_sweep is served by the hoisted code"""
    K = 3
    _, ref, grid, _, probs, out_off = _case(sed, K)
    det = sed.EventDetector(sed.LightningTimePooledCRNN(dropout=0.0, n_classes=K).cuda().eval())
    robj = sed.ReferenceEvents(ref, LENGTHS, K)
    dprobs = torch.from_numpy(probs).cuda()
    for sc in (dict(collar=1, block=5, offset_collar=2), dict(collar=0, block=1), dict(collar=3, block=64, offset_percent=0.2)):
        got = det.sweep((dprobs, out_off), robj, grid, **sc).table()
        np.testing.assert_array_equal(got, tune_ref.sweep(probs, out_off, ref, grid, **sc), err_msg=str(sc))
