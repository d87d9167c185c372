"""The polyphonic sound detection score without a GPU: PSDSCriteria and its refusals, the header and the exports of
the two entries, the host-side refusals of sed_psds_sweep (it validates everything before anything is uploaded or launched),
the score arithmetic of PSDSResult on hand-made integer tables and against tests/psds_ref.py, the grid slicing shared with the
decoder sweep, and the kernel's one-accumulator merge walk restated in Python against the pairwise definition."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import psds_ref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = C.c_void_p(4096)          # a non-null device address: every call below returns before anything is uploaded or launched


def _err():
    from sed_crnn_amd._lib import lib
    return lib().sed_last_error_string().decode()


def _result(sed, counts, ct=None, criteria=None, total_seconds=3600.0, class_seconds=None, thresholds=None):
    counts = np.asarray(counts, np.int64)
    G, K = counts.shape[:2]
    ct = np.zeros((G, K, K), np.int64) if ct is None else np.asarray(ct, np.int64)
    grid = sed.DecoderGrid(np.linspace(0.1, 0.9, G) if thresholds is None else thresholds)
    return sed.PSDSResult(torch.from_numpy(counts), torch.from_numpy(ct), grid, criteria or sed.PSDSCriteria.scenario1(), total_seconds,
                          np.ones(K) if class_seconds is None else class_seconds)


# ───────────── criteria ─────────────
def test_criteria_presets_thousandths_and_refusals():
    import sed_crnn_amd as sed
    s1, s2 = sed.PSDSCriteria.scenario1(), sed.PSDSCriteria.scenario2()
    assert (s1.dtc_milli, s1.gtc_milli, s1.cttc_milli, s1.alpha_ct, s1.alpha_st, s1.e_max) == (700, 700, 0, 0.0, 1.0, 100.0)
    assert (s2.dtc_milli, s2.gtc_milli, s2.cttc_milli, s2.alpha_ct, s2.alpha_st, s2.e_max) == (100, 100, 300, 0.5, 1.0, 100.0)
    assert s1.cttc is None and s2.cttc == 0.3 and s2.dtc == 0.1
    d = sed.PSDSCriteria()
    assert (d.dtc_milli, d.gtc_milli, d.cttc_milli, d.alpha_ct, d.alpha_st, d.e_max) == (700, 700, 0, 0.0, 1.0, 100.0)
    # every multiple of 0.001 survives the float, whatever its rounding
    for m in range(1, 1001):
        assert sed.PSDSCriteria(dtc=m / 1000, gtc=m * 0.001, cttc=m / 1000.0).cttc_milli == m
    assert sed.PSDSCriteria(dtc=1, gtc=1.0).dtc_milli == 1000
    for bad in (dict(dtc=0.7005), dict(gtc=0.12345), dict(cttc=0.3001), dict(dtc=0.0), dict(gtc=0), dict(cttc=0.0), dict(dtc=1.001),
                dict(gtc=-0.1), dict(cttc=2), dict(dtc=float("nan"))):
        with pytest.raises(ValueError, match=next(iter(bad))):
            sed.PSDSCriteria(**bad)
    with pytest.raises(ValueError, match="alpha_ct=0.5 needs a cross-trigger criterion"):
        sed.PSDSCriteria(alpha_ct=0.5)
    with pytest.raises(ValueError, match="negative"):
        sed.PSDSCriteria(alpha_st=-1.0)
    with pytest.raises(ValueError, match="e_max"):
        sed.PSDSCriteria(e_max=0.0)
    assert sed.PSDSCriteria(cttc=0.3).alpha_ct == 0.0                    # a criterion without a weight is allowed


# ───────────── the C entries ─────────────
def test_header_table_and_library_list_the_psds_entries():
    from sed_crnn_amd import _lib
    from sed_crnn_amd.build import EXTRA_FLAGS, NO_SCRATCH_KERNELS, SOURCES
    import sed_crnn_amd as sed
    header = open(os.path.join(ROOT, "include", "sedcrnn.h")).read()
    L = _lib.lib()
    for name in ("sed_psds_workspace_bytes", "sed_psds_sweep"):
        assert name in _lib.SIGNATURES and f" {name}(" in header and hasattr(L, name)
    res, args = _lib.SIGNATURES["sed_psds_sweep"]
    assert res is C.c_int and len(args) == 17 and args[9:12] == [C.c_int] * 3 and args[13] is C.c_size_t
    assert _lib.SIGNATURES["sed_psds_workspace_bytes"] == _lib.SIGNATURES["sed_tune_workspace_bytes"]
    assert "int dtc_milli, int gtc_milli, int cttc_milli" in header and "long* counts, long* ct, void* stream" in header
    # the workspace is the decoder sweep's (the prefix is per frame: block = 1 fills all of its region)
    for a in ((1000, 3, 4, 2, 1), (6400, 3, 4, 8, 5), (833, 32, 5, 4, 12)):
        assert L.sed_psds_workspace_bytes(*a) == L.sed_tune_workspace_bytes(*a) > 0
    n_total, K, R, n_tracks, G = 6400, 3, 4, 8, 5
    al = lambda b: (b + 15) & ~15  # noqa: E731
    assert L.sed_psds_workspace_bytes(n_total, K, R, n_tracks, G) == (al(12 * (R + 1)) + al(16 * G) + al(4 * n_tracks) +
                                                                      al(4 * K * (n_total + R)) + 8 * n_tracks * K * (n_total // 64 + R))
    for bad in ((0, 1, 1, 1, 1), (5, 1, 6, 1, 1), (100, 0, 1, 1, 1), (100, 33, 1, 1, 1), (100, 1, 1, 0, 1), (100, 1, 1, 3, 1),
                (100, 1, 1, 1, 0), (2 ** 31 - 1, 2, 1, 1, 1), (100, 1, 1, 1, 2 ** 21)):
        assert L.sed_psds_workspace_bytes(*bad) == 0, bad
    assert "psds.hip" in SOURCES and set(NO_SCRATCH_KERNELS["psds.hip"]) == {"psds_walk_k"}
    assert "-Rpass-analysis=kernel-resource-usage" in EXTRA_FLAGS["psds.hip"]      # without it the guard sees no remark
    src = open(os.path.join(ROOT, "sed_crnn_amd", "csrc", "psds.hip")).read()
    assert "launch_bits_seg(" in src and "tune_refblocks_k<<<" in src and "detect_walk_body(" in src      # shared, not copied
    assert "tune_refblocks_k<<<" in open(os.path.join(ROOT, "sed_crnn_amd", "csrc", "tune.hip")).read()
    for name in ("PSDSCriteria", "PSDSResult", "psds_sweep"):
        assert hasattr(sed, name)
    assert callable(sed.EventDetector.psds)


def test_psds_sweep_refuses_bad_input_without_a_launch():
    from sed_crnn_amd._lib import TuneSetting, lib
    L = lib()
    n_out = [100, 1, 64, 65]
    K = 3
    good = [(1, 0.5, 0.5, 0, 1), (3, 0.3, 0.6, 2, 2)]
    need = L.sed_psds_workspace_bytes(sum(n_out), K, 4, 3, 2)      # (1, 0.5), (3, 0.3), (3, 0.6)
    assert need > 0

    def call(n=n_out, sets=good, ws=need, crit=(700, 700, 0), probs=FAKE, counts=FAKE, ct=None, G=None, settings=True, work=FAKE):
        n = np.ascontiguousarray(np.asarray(n, np.int64))
        arr = (TuneSetting * max(len(sets), 1))(*[TuneSetting(*s) for s in sets])
        return L.sed_psds_sweep(probs, C.c_void_p(n.ctypes.data), n.size, K, C.cast(arr, C.c_void_p) if settings else None,
                                len(sets) if G is None else G, FAKE, FAKE, FAKE, crit[0], crit[1], crit[2], work, ws, counts, ct, None)

    assert call(ws=need - 1) != 0 and _err().startswith("psds_sweep:") and "workspace" in _err() and f"{need} needed" in _err()
    assert "3 bit tracks" in _err()
    for crit, word in (((0, 700, 0), "dtc"), ((1001, 700, 0), "dtc"), ((-5, 700, 0), "dtc"), ((700, 0, 0), "gtc"), ((700, 1001, 0), "gtc"),
                       ((700, 700, -1), "cttc"), ((700, 700, 1001), "cttc")):
        assert call(crit=crit) != 0 and _err().startswith("psds_sweep:") and word in _err(), crit
    assert call(crit=(100, 100, 300), ct=None) != 0 and "null pointer (ct" in _err()        # cross triggers need somewhere to go
    assert call(sets=[good[0], (4, 0.5, 0.5, 0, 1)]) != 0 and "psds_sweep: setting 1: median" in _err()
    assert call(sets=[good[0], good[1], (1, 0.6, 0.5, 0, 1)]) != 0 and "setting 2: need hi >= lo" in _err()
    assert call(sets=[(1, 0.5, 0.5, -1, 1)]) != 0 and "min_gap" in _err()
    assert call(n=[100, -5, 64, 65]) != 0 and "psds_sweep: recording 1 has -5 output frames" in _err()
    assert call(n=[2 ** 30, 2 ** 30]) != 0 and "2^31" in _err()
    assert call(probs=None) != 0 and "null pointer" in _err()
    assert call(counts=None) != 0 and "null pointer" in _err()
    assert call(work=None) != 0 and "null pointer (workspace)" in _err()
    assert call(settings=False) != 0 and "null pointer" in _err()
    assert call(G=-1) != 0 and "G=-1" in _err()
    # G = 0: a clean no-op (nothing to upload, nothing to launch), but the recording table is still checked
    assert call(sets=[], ws=0) == 0
    assert call(sets=[], ws=0, n=[100, -5]) != 0 and "recording 1" in _err()


# ───────────── the score arithmetic on hand-made tables ─────────────
def test_perfect_detector_scores_one_and_no_detections_zero():
    import sed_crnn_amd as sed
    n_ref = [4, 9, 1]
    perfect = [[[n, n, n, 0] for n in n_ref] for _ in range(5)]
    res = _result(sed, perfect)
    assert res.psds() == 1.0
    e, mean, std, etpr = res.curve()
    assert e.tolist() == [0.0, 100.0] and mean.tolist() == [1.0, 1.0] and std.tolist() == [0.0, 0.0] and etpr.tolist() == [1.0, 1.0]
    assert res.per_class_auc().tolist() == [1.0, 1.0, 1.0]
    silent = [[[0, n, 0, 0] for n in n_ref] for _ in range(5)]
    assert _result(sed, silent).psds() == 0.0
    assert _result(sed, silent, criteria=sed.PSDSCriteria.scenario2()).psds() == 0.0


def test_two_point_roc_has_the_hand_computed_area():
    import sed_crnn_amd as sed
    # one hour, one class with 4 reference events: (TPR, FPR/h) = (0.25, 10) and (0.75, 50); e_max = 100
    res = _result(sed, [[[1, 4, 11, 10]], [[3, 4, 53, 50]]])
    tpr, fpr, ctr, efpr = res.rates()
    assert tpr[:, 0].tolist() == [0.25, 0.75] and fpr[:, 0].tolist() == [10.0, 50.0] and efpr.tolist() == fpr.tolist()
    e, tk = res.roc(0)
    assert e.tolist() == [10.0, 50.0] and tk.tolist() == [0.25, 0.75]
    assert res.curve()[0].tolist() == [10.0, 50.0, 100.0]
    assert res.psds() == (0.25 * 40 + 0.75 * 50) / 100 == 0.475          # 0 before e = 10, left-constant after
    # half an hour of audio doubles the rates: the second point moves to e = 100, the first to 20
    assert _result(sed, [[[1, 4, 11, 10]], [[3, 4, 53, 50]]], total_seconds=1800.0).psds() == 0.25 * 80 / 100
    # a point beyond e_max is outside the area; a worse setting at a higher rate does not lower the step function
    assert _result(sed, [[[1, 4, 11, 10]], [[3, 4, 200, 101]]]).psds() == 0.25 * 90 / 100
    assert _result(sed, [[[3, 4, 11, 10]], [[1, 4, 53, 50]]]).psds() == 0.75 * 90 / 100
    # e_max itself as a point: the axis repeats it, the interval has no width
    assert _result(sed, [[[1, 4, 11, 10]], [[3, 4, 103, 100]]]).psds() == 0.25 * 90 / 100


def test_alpha_st_lowers_the_score_by_exactly_the_std_term():
    import sed_crnn_amd as sed
    table = [[[4, 4, 4, 0], [1, 2, 1, 0]]]                               # TPR 1.0 and 0.5 at eFPR 0: mean 0.75, std 0.25
    base = _result(sed, table, criteria=sed.PSDSCriteria(alpha_st=0.0)).psds()
    assert base == 0.75
    for a in (0.5, 1.0, 2.0):
        res = _result(sed, table, criteria=sed.PSDSCriteria(alpha_st=a))
        assert res.psds() == base - a * 0.25
        assert res.curve()[2].tolist() == [0.25, 0.25]
    assert res.per_class_auc().tolist() == [1.0, 0.5]


def test_cross_triggers_enter_the_effective_rate_only_with_a_criterion_and_reference_time():
    import sed_crnn_amd as sed
    counts = [[[2, 4, 9, 6], [1, 2, 3, 2], [0, 0, 5, 5]]]
    ct = [[[0, 3, 7], [4, 0, 9], [1, 2, 0]]]
    secs = np.array([1800.0, 900.0, 0.0])                                # class 2 has no reference time: never a column
    res = _result(sed, counts, ct, sed.PSDSCriteria.scenario2(), 7200.0, secs)
    tpr, fpr, ctr, efpr = res.rates()
    assert fpr[0].tolist() == [3.0, 1.0, 2.5] and ctr[0, 0, 1] == 3 / 0.25 and ctr[0, 1, 0] == 4 / 0.5
    assert efpr[0].tolist() == [3.0 + 0.5 * 12.0, 1.0 + 0.5 * 8.0, 2.5 + 0.5 * (2.0 + 8.0) / 2]
    assert np.isnan(tpr[0, 2]) and res.kept_classes().tolist() == [0, 1]
    # without the criterion (or with alpha_ct = 0) the table of cross triggers is ignored
    assert _result(sed, counts, ct, sed.PSDSCriteria.scenario1(), 7200.0, secs).rates()[3].tolist() == fpr.tolist()
    assert _result(sed, counts, ct, sed.PSDSCriteria(cttc=0.3), 7200.0, secs).rates()[3].tolist() == fpr.tolist()
    # a single class has no other class: the term is 0
    one = _result(sed, [[[1, 2, 3, 2]]], [[[0]]], sed.PSDSCriteria.scenario2(), 3600.0, np.array([100.0]))
    assert one.rates()[3].tolist() == [[2.0]]


def test_a_class_without_reference_is_skipped_and_none_left_raises():
    import sed_crnn_amd as sed
    with_empty = _result(sed, [[[1, 4, 11, 10], [0, 0, 7, 7]], [[3, 4, 53, 50], [0, 0, 90, 90]]])
    alone = _result(sed, [[[1, 4, 11, 10]], [[3, 4, 53, 50]]])
    assert with_empty.psds() == alone.psds() == 0.475
    auc = with_empty.per_class_auc()
    assert auc[0] == 0.475 and np.isnan(auc[1])
    with pytest.raises(ValueError, match="no class has a reference event"):
        _result(sed, [[[0, 0, 3, 3], [0, 0, 7, 7]]]).psds()
    with pytest.raises(ValueError, match="empty grid"):
        _result(sed, np.zeros((0, 2, 4), np.int64), thresholds=[]).psds()


def test_result_formulas_match_the_reference_on_random_tables():
    import sed_crnn_amd as sed
    rng = np.random.default_rng(5)
    for case in range(60):
        G, K, R = int(rng.integers(1, 40)), int(rng.integers(1, 7)), 3
        n_out = rng.integers(50, 4000, R).tolist()
        ref = [[[(int(a), int(a) + int(rng.integers(1, 9))) for a in np.sort(rng.choice(np.arange(0, n_out[r] - 10, 10), int(rng.integers(0, 4)),
                                                                                         replace=False))] for _ in range(K)] for r in range(R)]
        if case % 5 == 0:
            ref = [[[] if k == K - 1 and K > 1 else ref[r][k] for k in range(K)] for r in range(R)]
        n_ref = np.array([sum(len(ref[r][k]) for r in range(R)) for k in range(K)])
        if not n_ref.any():
            continue
        counts = np.zeros((G, K, 4), np.int64)
        counts[..., 1] = n_ref
        counts[..., 0] = rng.integers(0, n_ref + 1, (G, K))
        counts[..., 3] = rng.integers(0, 40, (G, K)) * (rng.random((G, K)) < 0.8)   # ties and zeros among the rates
        counts[..., 2] = counts[..., 3] + rng.integers(0, 9, (G, K))
        ct = rng.integers(0, 6, (G, K, K)) * (1 - np.eye(K, dtype=np.int64))
        fs = float(rng.choice([0.02, 0.16, 1.0]))
        crit = [sed.PSDSCriteria.scenario1(), sed.PSDSCriteria.scenario2(),
                sed.PSDSCriteria(0.5, 0.5, 0.2, alpha_ct=1.0, alpha_st=0.3, e_max=float(rng.choice([20.0, 100.0, 5000.0])))][case % 3]
        ref_obj = sed.ReferenceEvents(ref, n_out, K)
        secs = np.array([sum(b - a for r in range(R) for a, b in ref_obj.events(r, k)) for k in range(K)]) * fs
        res = sed.PSDSResult(torch.from_numpy(counts), torch.from_numpy(ct), sed.DecoderGrid(np.linspace(0.1, 0.9, G)), crit,
                             sum(n_out) * fs, secs)
        want = psds_ref.score(counts, ct, n_out, ref, fs, crit.cttc_milli, crit.alpha_ct, crit.alpha_st, crit.e_max)
        e, mean, std, etpr = res.curve()
        np.testing.assert_allclose(e, want["e"], rtol=1e-12, atol=0)
        np.testing.assert_allclose(mean, want["mean"], rtol=1e-12, atol=1e-15)
        np.testing.assert_allclose(std, want["std"], rtol=1e-12, atol=1e-15)
        np.testing.assert_allclose(res.rates()[3], want["efpr"], rtol=1e-12, atol=0)
        assert abs(res.psds() - want["psds"]) <= 1e-12 * max(abs(want["psds"]), 1e-300), (case, res.psds(), want["psds"])
        auc = res.per_class_auc()
        assert res.kept_classes().tolist() == want["kept"]
        for k, v in want["per_class_auc"].items():
            assert abs(auc[k] - v) <= 1e-12 * max(abs(v), 1e-300)


# ───────────── slicing: shared with the decoder sweep, the same rows for every split ─────────────
def test_slices_by_workspace_give_the_same_rows(monkeypatch):
    import sed_crnn_amd as sed
    from sed_crnn_amd import _lib, tune
    real = _lib.lib()
    calls = []

    class Fake:
        sed_psds_workspace_bytes = staticmethod(real.sed_psds_workspace_bytes)
        sed_last_error_string = staticmethod(real.sed_last_error_string)

        @staticmethod
        def sed_psds_sweep(probs, n_out, R, K, settings, G, off, on, offs, dtc, gtc, cttc, ws, ws_bytes, counts, ct, stream):
            sets = C.cast(settings, C.POINTER(_lib.TuneSetting))
            tracks = {(sets[g].median, sets[g].lo) for g in range(G)} | {(sets[g].median, sets[g].hi) for g in range(G)}
            assert ws_bytes >= real.sed_psds_workspace_bytes(833, K, R, len(tracks), G) > 0
            out = C.cast(counts, C.POINTER(C.c_long))
            cto = C.cast(ct, C.POINTER(C.c_long)) if ct else None
            assert (cto is not None) == (cttc > 0)
            for g in range(G):                                           # rows that depend on the setting alone
                for k in range(K):
                    for j in range(4):
                        out[(g * K + k) * 4 + j] = int(round(sets[g].hi * 1000)) * 100 + sets[g].median * 10 + k * 4 + j
                    for c in range(K if cto is not None else 0):
                        cto[(g * K + k) * K + c] = int(round(sets[g].hi * 1000)) + k * K + c
            calls.append(G)
            return 0

    monkeypatch.setattr(tune, "lib", lambda: Fake)
    monkeypatch.setattr(tune, "_on_gpu", lambda p: p.contiguous().float())
    monkeypatch.setattr(tune, "stream_ptr", lambda: None)
    n_out, K = [1, 63, 64, 65, 640], 2
    ref = sed.ReferenceEvents([[[(0, 1)], []]] + [[[(2, 9)], [(0, 5), (5, 7)]]] * 4, n_out, K)
    track = (torch.zeros(sum(n_out), K), np.concatenate([[0], np.cumsum(n_out)]).tolist())
    grid = sed.DecoderGrid(np.linspace(0.2, 0.7, 6), median=[3])          # lo = hi, all distinct: one bit track per setting
    size = lambda t, g: real.sed_psds_workspace_bytes(sum(n_out), K, len(n_out), t, g)  # noqa: E731
    tables = {}
    for crit in (sed.PSDSCriteria.scenario1(), sed.PSDSCriteria.scenario2()):
        for budget, n_slices in ((1 << 30, 1), (size(3, 3), 2), (size(1, 1), 6)):
            calls.clear()
            res = tune.psds_sweep(track, ref, grid, crit, 0.16, max_workspace_bytes=budget)
            assert len(calls) == n_slices == res.n_slices and sum(calls) == len(grid), (budget, calls)
            assert res.workspace_bytes <= budget and res.n_tracks == max(calls)
            tables.setdefault(crit.cttc_milli, []).append(res.table())
            assert res.total_seconds == sum(n_out) * 0.16 and res.class_seconds.tolist() == [(1 + 4 * 7) * 0.16, 4 * 7 * 0.16]
        a = tables[crit.cttc_milli]
        for b in a[1:]:
            np.testing.assert_array_equal(a[0][0], b[0])
            np.testing.assert_array_equal(a[0][1], b[1])
        assert a[0][0][:, 0, 0].tolist() == [int(round(float(np.float32(v)) * 1000)) * 100 + 30 for v in np.linspace(0.2, 0.7, 6)]
        assert (a[0][1] != 0).any() == (crit.cttc_milli > 0)
    with pytest.raises(ValueError, match="does not hold a single setting"):
        tune.psds_sweep(track, ref, grid, sed.PSDSCriteria.scenario1(), 0.16, max_workspace_bytes=1000)
    # the decoder sweep slices with the same function
    assert tune._grid_slices(grid, sum(n_out), K, len(n_out), size(3, 3), real.sed_tune_workspace_bytes, "x") == \
        [(0, 3, size(3, 3), 3), (3, 6, size(3, 3), 3)]


def test_public_path_checks_before_it_touches_the_device():
    import sed_crnn_amd as sed
    K = 6
    det = sed.EventDetector(sed.LightningTimePooledCRNN(dropout=0.0, n_classes=K).eval(), median=5, min_gap=2, min_len=3)
    ref = sed.ReferenceEvents.from_events([[(0, 2, 5), (0, 5, 9), (1, 0, 3)]], [9], K)
    cpu = (torch.zeros(9, K), [0, 9])
    with pytest.raises(ValueError, match="recording 0: the reference was built for 9"):
        det.psds((torch.zeros(10, K), [0, 10]), ref)
    with pytest.raises(ValueError, match="1 recordings of 6 classes"):
        det.psds((torch.zeros(9, 3), [0, 9]), ref)
    with pytest.raises(TypeError, match="criteria must be a PSDSCriteria"):
        det.psds(cpu, ref, criteria=dict(dtc=0.5))
    with pytest.raises(TypeError, match="grid must be a DecoderGrid"):
        det.psds(cpu, ref, grid=[dict(threshold=0.5)])
    with pytest.raises(sed.SedHipError, match="must be on the GPU"):
        det.psds(cpu, ref)
    with pytest.raises(ValueError, match="frame_seconds"):
        sed.psds_sweep(cpu, ref, sed.DecoderGrid([0.5]), sed.PSDSCriteria(), 0.0)
    cw = det.with_decoder(median=[1, 3, 5, 1, 3, 5])
    assert cw.classwise
    with pytest.raises(ValueError, match="class-wise detector has no single median"):
        cw.psds(cpu, ref)
    with pytest.raises(sed.SedHipError, match="must be on the GPU"):       # with a grid it goes as far as the device
        cw.psds(cpu, ref, grid=sed.DecoderGrid([0.5]))


def test_threshold_settings_of_the_detector(monkeypatch):
    import sed_crnn_amd as sed
    from sed_crnn_amd import tune
    det = sed.EventDetector(sed.LightningTimePooledCRNN(dropout=0.0).eval(), median=5, min_gap=2, min_len=3)
    seen = []
    monkeypatch.setattr(tune, "psds_sweep", lambda *a: seen.append(a))
    det.psds("track", "ref")
    det.psds("track", "ref", thresholds=[0.25, 0.5], criteria=sed.PSDSCriteria.scenario2(), max_workspace_bytes=123)
    explicit = sed.DecoderGrid([0.4], median=[9])
    det.psds("track", "ref", thresholds=7, grid=explicit)
    grid = seen[0][2]
    assert len(grid) == 50 and [s["threshold"] for s in grid] == np.linspace(0.01, 0.99, 50).tolist()
    assert all(s == dict(threshold=s["threshold"], low=s["threshold"], median=5, min_gap=2, min_len=3) for s in grid)
    assert seen[0][3].cttc_milli == 0 and seen[0][3].dtc_milli == 700 and seen[0][4] == det.frame_seconds and seen[0][5] == 1 << 30
    assert [s["threshold"] for s in seen[1][2]] == [0.25, 0.5] and seen[1][3].cttc_milli == 300 and seen[1][5] == 123
    assert seen[2][2] is explicit


# ───────────── the reference itself, on cases small enough to do by hand ─────────────
def test_reference_ties_pass_at_the_boundary_and_fail_one_frame_short():
    one = lambda D, G, *crit: psds_ref.counts_one([D], [G], *crit)[0][0]  # noqa: E731
    # dtc: 1000 · 7 == 700 · 10 is relevant (and covers all of its reference event), 6 of 10 is a false positive
    assert one([(10, 20)], [(13, 20)], 700, 700, 0) == [1, 1, 1, 0]
    assert one([(10, 20)], [(14, 20)], 700, 700, 0) == [0, 1, 1, 1]
    # gtc: a reference event of 10 frames covered by 7 / by 6 (the detections lie inside it: always relevant)
    assert one([(53, 60)], [(50, 60)], 700, 700, 0) == [1, 1, 1, 0]
    assert one([(54, 60)], [(50, 60)], 700, 700, 0) == [0, 1, 1, 0]
    # coverage adds up over the relevant detections only: 4 + 3 = 7 of 10; the third lies mostly outside and is not relevant
    assert one([(50, 54), (56, 59)], [(50, 60)], 700, 700, 0) == [1, 1, 2, 0]
    assert one([(50, 54), (56, 58), (59, 70)], [(50, 60)], 700, 700, 0) == [0, 1, 3, 1]
    assert one([(50, 54), (56, 58), (59, 70)], [(50, 60)], 50, 700, 0) == [1, 1, 3, 0]
    # cttc: a false positive of class 0 with 3 / 2 of its 10 frames on the reference of class 1; never on its own class
    c, ct = psds_ref.counts_one([[(10, 20)], []], [[], [(17, 20)]], 700, 700, 300)
    assert c == [[0, 0, 1, 1], [0, 1, 0, 0]] and ct == [[0, 1], [0, 0]]
    assert psds_ref.counts_one([[(10, 20)], []], [[], [(18, 20)]], 700, 700, 300)[1] == [[0, 0], [0, 0]]
    assert psds_ref.counts_one([[(10, 20)], []], [[], [(17, 20)]], 700, 700, 0)[1] == [[0, 0], [0, 0]]
    # a relevant detection is no cross trigger, however much of another class it covers
    assert psds_ref.counts_one([[(10, 20)], []], [[(10, 20)], [(10, 20)]], 700, 700, 300)[1] == [[0, 0], [0, 0]]


# ───────────── the kernel's method, restated: one open accumulator and a pointer ─────────────
def _merge_walk(D, refs, k, dtc, gtc, cttc):
    """PsdsEmit of csrc/psds.hip in Python: frame prefixes for |d ∩ G_c|, one coverage sum for the open reference event"""
    K = len(refs)
    n = max([b for evs in refs for _, b in evs] + [b for _, b in D] + [1])
    A = np.zeros((K, n + 1), np.int64)
    for c in range(K):
        m = np.zeros(n, np.int64)
        for a, b in refs[c]:
            m[a:b] = 1
        A[c, 1:] = np.cumsum(m)
    G = refs[k]
    jp, cov, tp, fp, ct = 0, 0, 0, 0, [0] * K
    for on, off in D:
        if 1000 * int(A[k, off] - A[k, on]) >= dtc * (off - on):
            while jp < len(G):
                a, b = G[jp]
                if a >= off:
                    break
                if b > on:
                    cov += min(b, off) - max(a, on)
                if b > off:
                    break
                tp += 1000 * cov >= gtc * (b - a)
                cov, jp = 0, jp + 1
            continue
        fp += 1
        for c in range(K if cttc else 0):
            if c != k and 1000 * int(A[c, off] - A[c, on]) >= cttc * (off - on):
                ct[c] += 1
    if jp < len(G):
        tp += 1000 * cov >= gtc * (G[jp][1] - G[jp][0])
    return [tp, len(G), len(D), fp], ct


def test_one_accumulator_merge_walk_is_the_pairwise_definition():
    rng = np.random.default_rng(11)

    def events(n_out, max_events, max_len, max_gap):
        ev, at = [], int(rng.integers(0, max_gap + 1))
        for _ in range(int(rng.integers(0, max_events + 1))):
            b = at + int(rng.integers(1, max_len + 1))
            if b > n_out:
                break
            ev.append((at, b))
            at = b + int(rng.integers(0, max_gap + 1))
        return ev

    seen_tp = seen_ct = 0
    for case in range(1500):
        K = int(rng.integers(1, 4))
        n_out = int(rng.integers(5, 150))
        refs = [events(n_out, 12, int(rng.choice([3, 12, 40])), int(rng.choice([0, 2, 9]))) for _ in range(K)]
        sys_ = [events(n_out, 12, int(rng.choice([3, 12, 40])), int(rng.choice([1, 2, 9]))) for _ in range(K)]
        dtc, gtc, cttc = [(700, 700, 0), (100, 100, 300), (1000, 1, 1000), (500, 900, 1)][case % 4]
        want_c, want_ct = psds_ref.counts_one(sys_, refs, dtc, gtc, cttc)
        for k in range(K):
            got_c, got_ct = _merge_walk(sys_[k], refs, k, dtc, gtc, cttc)
            assert got_c == want_c[k] and got_ct == want_ct[k], (case, k, sys_[k], refs, dtc, gtc, cttc)
            seen_tp += got_c[0]
            seen_ct += sum(got_ct)
    assert seen_tp > 1000 and seen_ct > 300
