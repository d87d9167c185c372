"""The decoder sweep on the MI355X (sed_crnn_amd/tune.py, csrc/tune.hip) against the numpy restatement of tests/tune_ref.py
and against the real decoder.  Every comparison is exact integer equality: the counts are integers and the system events of a
setting are by definition those of sed_detect_events_batch."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import detect_ref  # noqa: E402
import tune_ref  # noqa: E402

pytestmark = pytest.mark.gpu

SCORINGS = (dict(collar=0, block=1),
            dict(collar=1, block=5, offset_collar=2),
            dict(collar=31, block=10 ** 6, offset_percent=0.5),                     # a block larger than any recording
            dict(collar=1, block=5, offset_collar=1, offset_percent=0.2))


@pytest.fixture(scope="module")
def sed():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    import sed_crnn_amd as s
    return s


@pytest.fixture(scope="module")
def det(sed):
    return sed.EventDetector(sed.LightningTimePooledCRNN(dropout=0.0).cuda().eval())


def _every_median_grid(sed):
    """24 settings: every median width 1..31, lo = hi and lo < hi, several gaps and lengths"""
    sets = []
    for i, m in enumerate(range(1, 32, 2)):
        hi = (0.5, 0.6, 0.7)[i % 3]
        sets.append(dict(threshold=hi, low=(None, 0.3, 0.45)[(i // 2) % 3], median=m, min_gap=(0, 1, 3, 17)[i % 4],
                         min_len=(1, 2, 5)[(i // 3) % 3]))
    for i in range(8):
        sets.append(dict(threshold=0.4 + 0.05 * i, low=0.4 if i % 2 else None, median=(1, 3)[i % 2], min_gap=i % 3, min_len=1 + i % 4))
    return sed.DecoderGrid.from_settings(sets)


def _smooth(rng, n, K, scale=0.15):
    walk = np.cumsum(rng.standard_normal((n, K)) * scale, 0)
    return ((1 / (1 + np.exp(-np.sin(walk)))) * 0.6 + 0.2).astype(np.float32)


def _perturbed_ref(rng, tracks, K, **kw):
    """reference events = the decode of a perturbed copy of every track (so that matches, near misses and misses all occur)"""
    kw = dict(dict(lo=0.45, hi=0.55, median=3, min_gap=1), **kw)
    evs = []
    for t in tracks:
        p = np.roll(t, int(rng.integers(-2, 3)), 0) + rng.standard_normal(t.shape).astype(np.float32) * 0.03
        evs.append(detect_ref.decode(p.astype(np.float32), **kw))
    return tune_ref.events_to_ref(evs, K)


def _pack(tracks):
    out_off = np.concatenate([[0], np.cumsum([len(t) for t in tracks])]).tolist()
    return np.ascontiguousarray(np.concatenate(tracks), np.float32), out_off


def _check(sed, det, tracks, ref_lists, grid, scorings=SCORINGS, what=""):
    """sweep on the device == decode in numpy per (recording, setting), then score, for every scoring"""
    K = tracks[0].shape[1]
    probs, out_off = _pack(tracks)
    n_out = np.diff(out_off).tolist()
    ref = sed.ReferenceEvents(ref_lists, n_out, K)
    dprobs = torch.from_numpy(probs).cuda()
    decoded = [tune_ref.decode_all(probs, out_off, s) for s in grid]
    total = None
    for sc in scorings:
        got = det.sweep((dprobs, out_off), ref, grid, **sc).table()
        want = np.stack([tune_ref.score(ev, ref_lists, n_out, K, **sc) for ev in decoded])
        assert got.dtype == np.int64 and got.shape == (len(grid), K, 6)
        np.testing.assert_array_equal(got, want, err_msg=f"{what} {sc}")
        total = want if total is None else total + want
    return total


# ───────────── 1. against the numpy reference ─────────────
@pytest.mark.parametrize("K", [1, 3, 6])
def test_sweep_matches_the_reference_on_random_and_smooth_tracks(sed, det, K):
    rng = np.random.default_rng(100 + K)
    grid = _every_median_grid(sed)
    lengths = {1: [1, 63, 64, 65, 300], 3: [1, 63, 64, 65] + rng.integers(1, 400, 26).tolist(), 6: [200, 1, 65, 500]}[K]
    tracks = [rng.random((n, K)).astype(np.float32) for n in lengths]
    t = _check(sed, det, tracks, _perturbed_ref(rng, tracks, K, median=1), grid, what=f"random K={K}")
    assert (t[..., 0] > 0).any() and (t[..., 3] > 0).any()
    tracks = [_smooth(rng, n, K) for n in lengths]
    t = _check(sed, det, tracks, _perturbed_ref(rng, tracks, K), grid, what=f"smooth K={K}")
    assert (t[..., 0] > 0).any() and (t[..., 0] < t[..., 1]).any()                   # matches and misses both occur
    if K == 1:                                                                     # R = 1
        one = [_smooth(rng, 900, 1)]
        _check(sed, det, one, _perturbed_ref(rng, one, 1), grid, what="R=1")
    # tune_ref.sweep is the same composition
    probs, out_off = _pack(tracks)
    ref_lists = _perturbed_ref(rng, tracks, K)
    small = sed.DecoderGrid([0.5, 0.6], [0.4], [1, 5], [0, 2])
    got = det.sweep((torch.from_numpy(probs).cuda(), out_off), sed.ReferenceEvents(ref_lists, np.diff(out_off), K), small, collar=2,
                    block=7).table()
    np.testing.assert_array_equal(got, tune_ref.sweep(probs, out_off, ref_lists, small, collar=2, block=7))


def test_sweep_runs_across_every_word_and_chunk_boundary(sed, det):
    rng = np.random.default_rng(3)
    n = 3 * 4096 + 500
    p = np.full((n, 2), 0.1, np.float32)
    for b in range(64, n, 64):                                  # every word boundary of the bit tracks
        p[b - 3: b + 2, 0] = 0.8
    for b in range(4096, n, 4096):                              # every chunk boundary of the walk
        p[b - 100: b + 100, 1] = 0.7
        p[b, 1] = 0.9
    p[60:4100, 1] = 0.6                                         # a run over the first chunk boundary
    tracks = [_smooth(rng, 130, 2), p, _smooth(rng, 64, 2)]
    grid = sed.DecoderGrid.from_settings([dict(threshold=0.5), dict(threshold=0.65, low=0.5, min_gap=60), dict(threshold=0.5, median=5),
                                          dict(threshold=0.75, low=0.65, median=3, min_len=4)])
    ref_lists = _perturbed_ref(rng, tracks, 2, median=1, min_gap=0)
    t = _check(sed, det, tracks, ref_lists, grid, what="boundaries")
    assert t[0, 0, 1] > 190 and t[0, 0, 0] > 0


# ───────────── 2. tie to the real decoder ─────────────
def test_every_row_is_the_score_of_the_real_decoders_events(sed, det):
    rng = np.random.default_rng(21)
    K = 3
    tracks = [_smooth(rng, n, K) for n in (500, 1, 64, 65, 1200, 77)]
    probs, out_off = _pack(tracks)
    n_out = np.diff(out_off).tolist()
    ref_lists = _perturbed_ref(rng, tracks, K)
    ref = sed.ReferenceEvents(ref_lists, n_out, K)
    grid = sed.DecoderGrid([0.5, 0.6], [0.45, 0.5], [1, 3, 7], [0, 2], [1, 3])
    dprobs = torch.from_numpy(probs).cuda()
    bp = sed.plan_batch([8 * n for n in n_out], 8, K)                                # decode_many takes R and out_off from it
    assert list(bp.out_off) == out_off
    sc = dict(collar=2, block=5, offset_collar=3, offset_percent=0.2)
    table = det.sweep((dprobs, out_off), ref, grid, **sc).table()
    for g in range(len(grid)):
        ev, offs = det.with_decoder(**grid[g]).decode_many(dprobs, bp)
        ev = {k: v.cpu().numpy() for k, v in ev.items()}
        per_rec = [{k: ev[k][offs[r]:offs[r + 1]] for k in ("cls", "onset", "offset")} for r in range(len(tracks))]
        np.testing.assert_array_equal(table[g], tune_ref.score(per_rec, ref_lists, n_out, K, **sc), err_msg=f"setting {g}")
        np.testing.assert_array_equal(table[g, :, 1], np.bincount(ev["cls"], minlength=K), err_msg=f"n_sys of setting {g}")


# ───────────── 3. edge cases ─────────────
def test_edge_cases_all_off_all_on_at_threshold_and_empty_sides(sed, det):
    rng = np.random.default_rng(4)
    K = 2
    grid = sed.DecoderGrid([0.5, 0.7], None, [1, 3], [0, 2])
    some = [[[(2, 9), (9, 12), (50, 90)], [(0, 1)]], [[], [(10, 20)]], [[(0, 1)], []]]
    none = [[[], []], [[], []], [[], []]]
    off = [np.zeros((100, K), np.float32), np.zeros((64, K), np.float32), np.zeros((1, K), np.float32)]
    on = [np.full((100, K), 0.9, np.float32), np.full((64, K), 0.9, np.float32), np.full((1, K), 0.9, np.float32)]
    at = [np.full((100, K), 0.5, np.float32), np.full((64, K), 0.7, np.float32), np.full((1, K), 0.5, np.float32)]
    t = _check(sed, det, off, some, grid, what="all off")
    assert (t[..., 1] == 0).all() and (t[..., 2] > 0).all()                          # a reference but no detections
    t = _check(sed, det, on, some, grid, what="all on")
    assert (t[..., 1] == 3 * len(SCORINGS)).all()
    t = _check(sed, det, at, some, grid, what="at the threshold")                    # p > threshold is strict
    assert (t[:4, :, 1] == len(SCORINGS)).all() and (t[4:, :, 1] == 0).all()         # only 0.7 > 0.5 counts
    t = _check(sed, det, on, none, grid, what="empty reference")                     # detections but no reference
    assert (t[..., 2] == 0).all() and (t[..., 0] == 0).all() and (t[..., 5] == 0).all() and (t[..., 4] > 0).all()
    mixed = [_smooth(rng, 100, K), np.zeros((64, K), np.float32), _smooth(rng, 1, K)]
    _check(sed, det, mixed, [some[0], some[1], none[2]], grid, what="mixed")
    _check(sed, det, mixed, [none[0], some[1], some[2]], grid, what="mixed, the reverse")
    empty = det.sweep((torch.from_numpy(mixed[0]).cuda(), [0, 100]), sed.ReferenceEvents([some[0]], [100], K),
                      sed.DecoderGrid.from_settings([]))
    assert empty.table().shape == (0, K, 6)


# ───────────── 4. invariances ─────────────
def _case(sed, rng, K=3, lengths=(300, 65, 1, 640, 129, 64, 900, 33)):
    tracks = [_smooth(rng, n, K) for n in lengths]
    return tracks, _perturbed_ref(rng, tracks, K)


def test_result_is_independent_of_the_grid_split(sed, det):
    from sed_crnn_amd._lib import lib
    rng = np.random.default_rng(31)
    tracks, ref_lists = _case(sed, rng)
    probs, out_off = _pack(tracks)
    K, R, n_total = 3, len(tracks), len(probs)
    ref = sed.ReferenceEvents(ref_lists, np.diff(out_off), K)
    dprobs = torch.from_numpy(probs).cuda()
    sc = dict(collar=1, block=5, offset_collar=2)
    grid = sed.DecoderGrid(np.linspace(0.4, 0.7, 5), [0.3, 0.35], [1, 5], [0, 3])      # every setting reads two tracks
    whole = det.sweep((dprobs, out_off), ref, grid, **sc)
    assert whole.n_slices == 1 and whole.n_tracks == grid.n_tracks() == 14
    ones = det.sweep((dprobs, out_off), ref, grid, max_workspace_bytes=lib().sed_tune_workspace_bytes(n_total, K, R, 2, 1), **sc)
    assert ones.n_slices == len(grid) == 40
    np.testing.assert_array_equal(ones.table(), whole.table())
    flat = sed.DecoderGrid(np.linspace(0.3, 0.75, 30))                               # lo = hi, all distinct: one track each
    whole = det.sweep((dprobs, out_off), ref, flat, **sc)
    sevens = det.sweep((dprobs, out_off), ref, flat, max_workspace_bytes=lib().sed_tune_workspace_bytes(n_total, K, R, 7, 7), **sc)
    assert sevens.n_slices == 5 and sevens.n_tracks == 7 and whole.n_slices == 1
    np.testing.assert_array_equal(sevens.table(), whole.table())
    np.testing.assert_array_equal(whole.table(), tune_ref.sweep(probs, out_off, ref_lists, flat, **sc))
    with pytest.raises(ValueError, match="does not hold a single setting"):
        det.sweep((dprobs, out_off), ref, flat, max_workspace_bytes=1000, **sc)


def test_result_is_independent_of_recording_order_and_bitwise_repeatable(sed, det):
    rng = np.random.default_rng(32)
    tracks, ref_lists = _case(sed, rng)
    grid = _every_median_grid(sed)
    sc = dict(collar=3, block=4, offset_percent=0.3)

    def run(order):
        probs, out_off = _pack([tracks[i] for i in order])
        ref = sed.ReferenceEvents([ref_lists[i] for i in order], np.diff(out_off), 3)
        return det.sweep((torch.from_numpy(probs).cuda(), out_off), ref, grid, **sc)

    base = run(range(len(tracks)))
    for _ in range(3):
        perm = rng.permutation(len(tracks)).tolist()
        np.testing.assert_array_equal(run(perm).table(), base.table(), err_msg=str(perm))
    again = run(range(len(tracks)))
    assert torch.equal(again.counts, base.counts)
    ref = sed.ReferenceEvents(ref_lists, [len(t) for t in tracks], 3)
    sel = [4, 0, 6]
    assert ref.select(sel).events(1, 2) == ref.events(0, 2)


# ───────────── 5. the public path with a net ─────────────
def _net_case(sed, seed, lengths):
    """a net whose track straddles 0.5, features of several recordings, and quantiles of the stitched track: the untrained net's
    output moves in a narrow band, so thresholds that cut it are taken from the track itself (test data, not a tolerance)"""
    from test_gpu_detect import _centre_on_threshold, _features, _nets
    r, m = _nets(sed, "lightning", seed)
    mels = [_features(N, 10 * seed + i) for i, N in enumerate(lengths)]
    _centre_on_threshold(r, m, mels[0])
    det = sed.EventDetector(m, hop=32)
    p = det.from_features_many(mels).probs.cpu().numpy()
    return det, mels, lambda *qs: [float(np.float32(v)) for v in np.quantile(p, qs)]


def test_end_to_end_tune_then_detect_reproduces_the_best_row(sed):
    # from scaled features (from_features_many), not PCM: everything after the log-mel front end is the path of detect_many, and
    # test_gpu_detect_many.py pins detect_many == from_features_many on the front end's output bit for bit
    det, mels, q = _net_case(sed, 5, (6000, 3000, 64, 9000, 130))
    lows, his = q(0.2, 0.35), q(0.4, 0.5, 0.6)
    truth = det.with_decoder(threshold=his[1], low=lows[1], median=5, min_gap=2, min_len=2)
    ref = sed.ReferenceEvents.from_result(truth.from_features_many(mels))
    assert len(ref) > 8
    res = det.from_features_many(mels)
    grid = sed.DecoderGrid(his, lows, [1, 5, 9], [0, 2], [1, 2])
    sweep = det.sweep(res, ref, grid, collar=1, offset_collar=1)
    g, best, score = sweep.best()
    g_truth = [grid[i] for i in range(len(grid))].index(truth.decoder_settings())    # the setting that made the reference
    assert grid[g] == best and g <= g_truth                                          # ties go to the lowest g
    np.testing.assert_array_equal(sweep.table()[g], sweep.table()[g_truth])
    row = sweep.table()[g]
    assert (row[:, 0] == row[:, 1]).all() and (row[:, 1] == row[:, 2]).all() and score > 0.999
    assert (sweep.f1_event()[1] <= score).all() and sweep.f1_event()[1].min() < 0.999
    tuned, sweep2 = sed.tune_decoder(det, res, ref, grid, collar=1, offset_collar=1)
    assert tuned.decoder_settings() == best and tuned.model is det.model and torch.equal(sweep2.counts, sweep.counts)
    res2 = tuned.from_features_many(mels)
    sc = tuned.score(res2, ref, collar=1, offset_collar=1)
    np.testing.assert_array_equal(sc.table()[0], row)
    np.testing.assert_array_equal(row[:, 1], np.bincount(res2.events["cls"].cpu().numpy(), minlength=row.shape[0]))
    # block defaults to round(1 / frame_seconds) output frames
    assert sweep.block == round(1 / det.frame_seconds) == sc.block


def test_score_is_the_one_setting_sweep_and_a_single_result_is_the_one_recording_batch(sed):
    det, mels, q = _net_case(sed, 6, (3000, 1000, 4000))
    lo, mid, hi = q(0.35, 0.5, 0.6)
    det = det.with_decoder(threshold=hi, low=mid, median=3, min_gap=1)
    res = det.from_features_many(mels)
    ref = sed.ReferenceEvents.from_result(det.with_decoder(threshold=mid, median=7).from_features_many(mels))
    assert len(ref) > 3 and res.n_events > 3
    kw = dict(collar=2, offset_percent=0.5, block=3)
    one = sed.DecoderGrid.from_settings([det.decoder_settings()])
    np.testing.assert_array_equal(det.score(res, ref, **kw).table(), det.sweep(res, ref, one, **kw).table())
    probs = res.probs.cpu().numpy()
    np.testing.assert_array_equal(det.score(res, ref, **kw).table(),
                                  tune_ref.sweep(probs, res.out_offsets, [[ref.events(i, 0)] for i in range(3)], one, **kw))
    grid = sed.DecoderGrid([mid, hi], [lo], [1, 3])
    total = 0
    for i in range(len(mels)):
        ref_i = ref.select([i])
        for single in (det.from_features(mels[i]), res[i]):                        # DetectionResults: the path's own, a batch's view
            a = det.sweep(single, ref_i, grid, **kw).table()
            b = det.sweep((single.probs, [0, single.probs.shape[0]]), ref_i, grid, **kw).table()
            np.testing.assert_array_equal(a, b)
            np.testing.assert_array_equal(det.score(single, ref_i, **kw).table()[0, :, 1], [len(single)])
        total = total + a
    np.testing.assert_array_equal(total, det.sweep(res, ref, grid, **kw).table())    # counts add over recordings
