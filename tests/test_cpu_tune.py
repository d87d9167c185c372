"""Event scoring and the decoder sweep without a GPU: the numpy reference of tests/tune_ref.py against independent yardsticks
(scipy's maximum bipartite matching, metrics.f1_overall_1sec), DecoderGrid, the ReferenceEvents constructors and their
refusals, and the argument checks of sed_tune_sweep, which validates its host tables before anything is uploaded or launched."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import detect_ref  # noqa: E402
import tune_ref  # noqa: E402

FAKE = C.c_void_p(4096)          # a non-null device address: every call below returns before anything is uploaded or launched


def _err():
    from sed_crnn_amd._lib import lib
    return lib().sed_last_error_string().decode()


def _random_events(rng, n_out, max_events, max_len=9, max_gap=6):
    """a sorted, pairwise disjoint event list inside [0, n_out) (touching events included)"""
    ev, at = [], int(rng.integers(0, max_gap + 1))
    for _ in range(int(rng.integers(0, max_events + 1))):
        b = at + int(rng.integers(1, max_len + 1))
        if b > n_out:
            break
        ev.append((at, b))
        at = b + int(rng.integers(0, max_gap + 1))
    return ev


# ───────────── the reference against independent yardsticks ─────────────
def test_onset_only_greedy_is_a_maximum_bipartite_matching():
    from scipy.sparse import csr_matrix
    from scipy.sparse.csgraph import maximum_bipartite_matching
    import sed_crnn_amd as sed
    rng = np.random.default_rng(7)
    nonzero = 0
    for case in range(1500):
        n_out = int(rng.integers(5, 120))
        sys_ev, ref_ev = _random_events(rng, n_out, 14, 5, 3), _random_events(rng, n_out, 14, 5, 3)
        collar = int(rng.choice([0, 1, 2, 3, 7, 31]))
        got = tune_ref.match_events(sys_ev, ref_ev, collar, [-1] * len(ref_ev))
        if not sys_ev or not ref_ev:
            assert got == 0
            continue
        adj = np.array([[abs(a - ra) <= collar for ra, _ in ref_ev] for a, _ in sys_ev], np.int8)
        want = int((maximum_bipartite_matching(csr_matrix(adj), perm_type="column") >= 0).sum())
        assert got == want, (case, collar, sys_ev, ref_ev)
        nonzero += want > 0
        # the product's packing keeps exactly these lists (and accepts them: sorted, disjoint, inside the recording)
        packed = sed.ReferenceEvents([[ref_ev], [sys_ev]], [n_out, n_out], 1)
        assert packed.events(0, 0) == ref_ev and packed.events(1, 0) == sys_ev
    assert nonzero > 500


def test_segment_counts_reproduce_f1_overall_1sec_on_the_event_masks():
    import sed_crnn_amd as sed
    from sed_crnn_amd import metrics
    rng = np.random.default_rng(9)
    partial = 0
    for case in range(60):
        K = int(rng.integers(1, 5))
        n_out = int(rng.integers(1, 200))
        block = int(rng.choice([1, 2, 5, 7, 50, 300]))
        partial += n_out % block != 0
        sys_k, ref_k = [_random_events(rng, n_out, 10) for _ in range(K)], [_random_events(rng, n_out, 10) for _ in range(K)]
        ev = {"cls": [k for k in range(K) for _ in sys_k[k]], "onset": [a for k in range(K) for a, _ in sys_k[k]],
              "offset": [b for k in range(K) for _, b in sys_k[k]]}
        rv = {"cls": [k for k in range(K) for _ in ref_k[k]], "onset": [a for k in range(K) for a, _ in ref_k[k]],
              "offset": [b for k in range(K) for _, b in ref_k[k]]}
        c = tune_ref.score([ev], [ref_k], [n_out], K, block=block).sum(0)
        tp, nsys, nref = float(c[3]), float(c[4]), float(c[5])
        prec, rec = tp / (nsys + metrics.eps), tp / (nref + metrics.eps)
        got = 2 * prec * rec / (prec + rec + metrics.eps)
        want = metrics.f1_overall_1sec(detect_ref.event_mask(ev, n_out, K), detect_ref.event_mask(rv, n_out, K), block)
        assert got == want, (case, K, n_out, block)
        # the event mask as frame labels gives the merged events back (touching events become one run)
        lab = sed.ReferenceEvents.from_labels_out([detect_ref.event_mask(rv, n_out, K)])
        assert tune_ref.score([ev], [[lab.events(0, k) for k in range(K)]], [n_out], K, block=block)[:, 3:].sum(0).tolist() == c[3:].tolist()
    assert partial > 10


def test_offset_tolerances_and_the_greedy_order():
    ref = [(10, 20), (22, 30), (40, 100)]
    assert tune_ref.tolerances(ref) == [-1, -1, -1]
    assert tune_ref.tolerances(ref, offset_collar=3) == [3, 3, 3]
    assert tune_ref.tolerances(ref, offset_percent=0.2) == [2, 1, 12]
    assert tune_ref.tolerances(ref, offset_collar=2, offset_percent=0.2) == [2, 2, 12]
    # the product computes the same integers for the device (float64, then int)
    import sed_crnn_amd as sed
    rng = np.random.default_rng(13)
    for case in range(300):
        evs = _random_events(rng, 4000, 30, 400, 50)
        oc = [None, 0, 1, 7][case % 4]
        pc = [None, 0.2, 0.5, float(rng.random())][(case // 4) % 4]
        got = sed.ReferenceEvents([[evs]], [4000], 1).tolerances(oc, pc)
        assert got.dtype == np.int32 and got.tolist() == tune_ref.tolerances(evs, oc, pc), (case, oc, pc)
    # the first system event takes the FIRST reference event in reach, the second the next
    assert tune_ref.match_events([(9, 20), (10, 21)], [(10, 20), (11, 22)], 1, [-1, -1]) == 2
    # with offsets: the first reference event's offset is out of reach, so the system event goes to the second
    assert tune_ref.match_events([(10, 30)], [(10, 20), (11, 30)], 1, [0, 0]) == 1
    assert tune_ref.match_events([(10, 30)], [(10, 20), (12, 30)], 1, [0, 0]) == 0


# ───────────── DecoderGrid ─────────────
def test_decoder_grid_order_low_none_and_dropped_pairs():
    import sed_crnn_amd as sed
    g = sed.DecoderGrid(threshold=[0.3, 0.6], low=[0.2, 0.5], median=[1, 5], min_gap=[0, 2], min_len=[1])
    # 0.3 x {0.2} and 0.6 x {0.2, 0.5}: low = 0.5 > threshold = 0.3 is dropped
    assert len(g) == 3 * 2 * 2
    assert g[0] == dict(threshold=0.3, low=0.2, median=1, min_gap=0, min_len=1)
    assert g[1] == dict(threshold=0.3, low=0.2, median=1, min_gap=2, min_len=1)      # min_gap / min_len fastest
    assert g[2] == dict(threshold=0.3, low=0.2, median=5, min_gap=0, min_len=1)
    assert g[4]["threshold"] == 0.6 and g[4]["low"] == 0.2 and g[8]["low"] == 0.5    # threshold slowest, then low
    assert all(s["low"] <= s["threshold"] for s in g)
    assert g.n_tracks() == 2 * 4                                                    # {0.3, 0.6, 0.2, 0.5} x two medians
    same = sed.DecoderGrid(threshold=[0.4, 0.5, 0.7])
    assert len(same) == 3 and [s["low"] for s in same] == [0.4, 0.5, 0.7] and same.n_tracks() == 3
    assert same[1] == dict(threshold=0.5, low=0.5, median=1, min_gap=0, min_len=1)
    big = sed.DecoderGrid(threshold=np.linspace(0.3, 0.65, 8), low=[0.1, 0.2, 0.25], median=[1, 3, 5, 7, 9])
    assert len(big) == 120 and big.n_tracks() == 55                                 # the pool of tracks, not 120 pairs
    ex = sed.DecoderGrid.from_settings([dict(threshold=0.5), dict(threshold=0.7, low=0.2, median=3, min_gap=4, min_len=2)])
    assert ex[0] == dict(threshold=0.5, low=0.5, median=1, min_gap=0, min_len=1) and ex[1]["min_gap"] == 4
    # a setting is a set of EventDetector keyword arguments
    det = sed.EventDetector(sed.LightningTimePooledCRNN(dropout=0.0).eval(), **ex[1])
    assert det.decoder_settings() == ex[1]
    d2 = det.with_decoder(**g[8])
    assert d2.decoder_settings() == g[8] and d2.model is det.model and d2.seq_len == det.seq_len
    assert det.with_decoder(threshold=0.9).decoder_settings()["low"] == 0.9
    with pytest.raises(ValueError, match="setting 1: median"):
        sed.DecoderGrid.from_settings([dict(threshold=0.5), dict(threshold=0.5, median=4)])
    with pytest.raises(ValueError, match="setting 0: low"):
        sed.DecoderGrid.from_settings([dict(threshold=0.5, low=0.6)])
    with pytest.raises(TypeError, match="decoder settings only"):
        det.with_decoder(hop=8)


# ───────────── ReferenceEvents ─────────────
def test_reference_from_labels_pools_and_drops_the_ragged_tail():
    import sed_crnn_amd as sed
    lab = np.zeros((43, 2), np.float32)                      # tf = 8 -> 5 output frames, 3 ragged input frames dropped
    lab[7, 0] = 1                                            # last input frame of output frame 0
    lab[8:17, 0] = 1                                         # frames 1 and 2 (one input frame into 2)
    lab[30, 1] = 1                                           # output frame 3
    lab[40:43, 1] = 1                                        # the ragged tail: dropped
    ref = sed.ReferenceEvents.from_labels([lab, lab[:16]], 8)
    assert ref.R == 2 and ref.K == 2 and ref.n_out == (5, 2)
    assert ref.events(0, 0) == [(0, 3)] and ref.events(0, 1) == [(3, 4)]
    assert ref.events(1, 0) == [(0, 2)] and ref.events(1, 1) == []
    assert ref.off.tolist() == [0, 1, 2, 3, 3] and ref.off.dtype == np.int32
    out = sed.ReferenceEvents.from_labels_out([np.array([[1, 0], [1, 0], [0, 0], [1, 1]])])
    assert out.events(0, 0) == [(0, 2), (3, 4)] and out.events(0, 1) == [(3, 4)] and len(out) == 3
    with pytest.raises(ValueError, match="recording 1: 5 frames are shorter"):
        sed.ReferenceEvents.from_labels([lab, lab[:5]], 8)
    assert out.tolerances().tolist() == [-1, -1, -1]
    assert out.tolerances(offset_collar=1, offset_percent=0.5).tolist() == [1, 1, 1]
    assert sed.ReferenceEvents.from_events([[(0, 0, 50)]], [60], 1).tolerances(offset_percent=0.2).tolist() == [10]


def test_reference_from_intervals_rounds_clips_and_merges():
    import sed_crnn_amd as sed
    fs = 0.5
    ref = sed.ReferenceEvents.from_intervals(
        [[(0, 0.6, 1.2), (0, 1.5, 2.0), (0, 3.1, 3.2), (1, 4.0, 99.0), (0, 2.0, 2.4)], []], fs, [10, 4], K=2)
    # [1, 3) and [3, 4) touch and [4, 5) touches again -> one event; [6, 7) stays; class 1 is clipped to n_out
    assert ref.events(0, 0) == [(1, 5), (6, 7)]
    assert ref.events(0, 1) == [(8, 10)]
    assert ref.events(1, 0) == [] and ref.n_out == (10, 4)
    assert sed.ReferenceEvents.from_intervals([[(2, 0.0, 0.1)]], fs, [3]).K == 3
    with pytest.raises(ValueError, match="recording 0, class 0, event 0"):
        sed.ReferenceEvents.from_intervals([[(0, 7.0, 8.0)]], fs, [10])            # starts past the end: nothing left after the clip


def test_reference_refusals_name_the_offender():
    import sed_crnn_amd as sed
    ok = [(0, 2, 5), (0, 5, 9), (1, 0, 3)]                                         # touching is fine
    assert sed.ReferenceEvents.from_events([ok], [9], 2).events(0, 0) == [(2, 5), (5, 9)]
    with pytest.raises(ValueError, match="recording 1, class 0, event 1.*overlaps or precedes"):
        sed.ReferenceEvents.from_events([ok, [(0, 2, 5), (0, 4, 9)]], [9, 9], 2)     # overlapping
    with pytest.raises(ValueError, match="recording 0, class 1, event 1.*overlaps or precedes"):
        sed.ReferenceEvents.from_events([[(1, 6, 8), (1, 1, 3)]], [9], 2)            # unsorted
    with pytest.raises(ValueError, match="recording 1, class 0, event 0.*ends past the recording's 9"):
        sed.ReferenceEvents.from_events([ok, [(0, 5, 10)]], [9, 9], 2)
    with pytest.raises(ValueError, match="recording 0, class 0, event 0.*offset > onset"):
        sed.ReferenceEvents.from_events([[(0, 4, 4)]], [9], 1)
    with pytest.raises(ValueError, match="recording 0, class 0, event 0.*offset > onset"):
        sed.ReferenceEvents.from_events([[(0, -1, 4)]], [9], 1)
    with pytest.raises(ValueError, match="K=33"):
        sed.ReferenceEvents.from_events([[]], [9], 33)
    with pytest.raises(ValueError, match="K=33"):
        sed.ReferenceEvents.from_labels_out([np.zeros((4, 33))])
    with pytest.raises(ValueError, match="recording 0, event 0: class 2"):
        sed.ReferenceEvents.from_events([[(2, 0, 1)]], [9], 2)
    # the sweep checks the reference against the track before it touches the device
    import torch
    det = sed.EventDetector(sed.LightningTimePooledCRNN(dropout=0.0).eval())
    ref = sed.ReferenceEvents.from_events([ok], [9], 2)
    grid = sed.DecoderGrid([0.5])
    with pytest.raises(ValueError, match="recording 0: the reference was built for 9"):
        det.sweep((torch.zeros(10, 2), [0, 10]), ref, grid)
    with pytest.raises(ValueError, match="1 recordings of 2 classes"):
        det.sweep((torch.zeros(9, 3), [0, 9]), ref, grid)
    with pytest.raises(ValueError, match="collar"):
        det.sweep((torch.zeros(9, 2), [0, 9]), ref, grid, collar=32)
    with pytest.raises(sed.SedHipError, match="must be on the GPU"):
        det.sweep((torch.zeros(9, 2), [0, 9]), ref, grid)


def test_sweep_result_scores_and_best_from_a_table():
    import torch
    import sed_crnn_amd as sed
    from sed_crnn_amd import metrics
    grid = sed.DecoderGrid([0.3, 0.5, 0.7])
    t = np.zeros((3, 2, 6), np.int64)
    t[0] = [[5, 10, 8, 4, 9, 6], [0, 0, 3, 0, 0, 2]]
    t[1] = [[7, 8, 8, 5, 6, 6], [2, 3, 3, 2, 2, 2]]
    t[2] = [[7, 8, 8, 5, 6, 6], [2, 3, 3, 2, 2, 2]]                                 # a tie with g = 1
    res = sed.SweepResult(torch.from_numpy(t), grid, 1, 5)
    cw, micro = res.f1_event()
    assert cw.shape == (3, 2) and micro.shape == (3,)
    p, r = 5 / (10 + metrics.eps), 5 / (8 + metrics.eps)
    assert cw[0, 0] == 2 * p * r / (p + r + metrics.eps) and cw[0, 1] == 0.0
    p, r = 9 / (11 + metrics.eps), 9 / (11 + metrics.eps)
    assert micro[1] == 2 * p * r / (p + r + metrics.eps)
    er_cw, er = res.er_segment()
    assert er_cw[0, 0] == ((6 - 4) + (9 - 4)) / 6 and er[0] == ((6 - 4) + (9 - 4) + 2) / 8
    assert res.f1_segment()[1][1] > res.f1_segment()[1][0]
    assert res.best() == (1, grid[1], float(micro[1]))                              # the lowest g of the tie
    assert res.best("er_segment")[0] == 1 and res.best("f1_segment", "macro")[0] == 1
    with pytest.raises(ValueError, match="metric"):
        res.best("accuracy")


# ───────────── the C entries ─────────────
def test_lib_lists_the_tune_symbols():
    from sed_crnn_amd import _lib
    assert "sed_tune_sweep" in _lib.SIGNATURES and "sed_tune_workspace_bytes" in _lib.SIGNATURES
    assert C.sizeof(_lib.TuneSetting) == 20
    L = _lib.lib()
    assert L.sed_tune_workspace_bytes(1000, 3, 4, 2, 1) > 0
    # grows with the number of bit tracks, by K words per frame/64 + R
    a, b = L.sed_tune_workspace_bytes(6400, 3, 4, 5, 5), L.sed_tune_workspace_bytes(6400, 3, 4, 8, 5)
    assert b - a == 3 * 3 * (6400 // 64 + 4) * 8                     # (the threshold table is padded to 16 bytes: 32 for both)
    for bad in ((0, 1, 1, 1, 1), (5, 1, 6, 1, 1), (100, 0, 1, 1, 1), (100, 33, 1, 1, 1), (100, 1, 1, 0, 1), (100, 1, 1, 3, 1),
                (100, 1, 1, 1, 0), (2 ** 31 - 1, 2, 1, 1, 1), (100, 1, 1, 1, 2 ** 21)):
        assert L.sed_tune_workspace_bytes(*bad) == 0, bad


def test_tune_sweep_refuses_bad_input_without_a_launch():
    from sed_crnn_amd._lib import TuneSetting, lib
    L = lib()
    n_out = [100, 1, 64, 65]
    K = 3
    good = [(1, 0.5, 0.5, 0, 1), (3, 0.3, 0.6, 2, 2)]
    need = L.sed_tune_workspace_bytes(sum(n_out), K, 4, 3, 2)      # (1, 0.5), (3, 0.3), (3, 0.6)
    assert need > 0

    def call(n=n_out, sets=good, ws=need, collar=1, block=5, probs=FAKE, counts=FAKE, G=None, settings=True):
        n = np.ascontiguousarray(np.asarray(n, np.int64))
        arr = (TuneSetting * max(len(sets), 1))(*[TuneSetting(*s) for s in sets])
        return L.sed_tune_sweep(probs, C.c_void_p(n.ctypes.data), n.size, K, C.cast(arr, C.c_void_p) if settings else None,
                                len(sets) if G is None else G, FAKE, FAKE, FAKE, FAKE, collar, block, FAKE, ws, counts, None)

    assert call(ws=need - 1) != 0 and "workspace" in _err() and "3 bit tracks" in _err()
    assert call(collar=32) != 0 and "collar" in _err()
    assert call(collar=-1) != 0 and "collar" in _err()
    assert call(sets=[good[0], (4, 0.5, 0.5, 0, 1)]) != 0 and "setting 1: median" in _err()
    assert call(sets=[(33, 0.5, 0.5, 0, 1)]) != 0 and "setting 0: median" in _err()
    assert call(sets=[good[0], good[1], (1, 0.6, 0.5, 0, 1)]) != 0 and "setting 2: need hi >= lo" in _err()
    assert call(sets=[(1, 0.5, 0.5, -1, 1)]) != 0 and "min_gap" in _err()
    assert call(sets=[(1, 0.5, 0.5, 0, 0)]) != 0 and "min_len" in _err()
    assert call(block=0) != 0 and "block" in _err()
    assert call(block=-3) != 0 and "block" in _err()
    assert call(n=[100, -5, 64, 65]) != 0 and "recording 1 has -5 output frames" in _err()
    assert call(n=[100, 0, 64, 65]) != 0 and "recording 1" in _err()
    assert call(n=[2 ** 30, 2 ** 30]) != 0 and "2^31" in _err()
    assert call(probs=None) != 0 and "null pointer" in _err()
    assert call(counts=None) != 0 and "null pointer" in _err()
    assert call(settings=False) != 0 and "null pointer" in _err()
    assert call(G=-1) != 0 and "G=-1" in _err()
    # G = 0: a clean no-op (nothing to upload, nothing to launch), but the recording table is still checked
    assert call(sets=[], ws=0) == 0
    assert call(sets=[], ws=0, n=[100, -5]) != 0 and "recording 1" in _err()
