"""Whole-recording detection without a GPU: the float64 numpy decoder of tests/detect_ref.py on hand-built cases, the window
planner of sed_crnn_amd/detect.py, and the argument checks of the sed_detect_* entries."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import detect_ref as ref  # noqa: E402


def _ev(d):
    return [(int(k), int(a), int(b)) for k, a, b in zip(d["cls"], d["onset"], d["offset"])]


def test_reference_decoder_thresholds_are_strict():
    p = np.array([[0.5], [0.6], [0.5], [0.7], [0.7], [0.4]], np.float32)
    assert _ev(ref.decode(p, lo=0.5, hi=0.5)) == [(0, 1, 2), (0, 3, 5)]            # p == lo is off
    # double threshold: a run whose maximum EQUALS hi is dropped
    p = np.array([[0.3], [0.6], [0.8], [0.6], [0.3], [0.6], [0.7], [0.2]], np.float32)
    assert _ev(ref.decode(p, lo=0.5, hi=0.7)) == [(0, 1, 4)]
    assert _ev(ref.decode(p, lo=0.5, hi=0.69)) == [(0, 1, 4), (0, 5, 7)]


def test_reference_decoder_runs_touching_both_ends_and_peaks():
    p = np.array([[0.9, 0.1], [0.8, 0.2], [0.2, 0.9], [0.95, 0.9], [0.95, 0.8]], np.float32)
    d = ref.decode(p)
    assert _ev(d) == [(0, 0, 2), (0, 3, 5), (1, 2, 5)]
    np.testing.assert_array_equal(d["peak"], np.float32([0.9, 0.95, 0.9]))
    np.testing.assert_array_equal(d["peak_frame"], [0, 3, 2])                       # first arg-max
    assert _ev(ref.decode(np.ones((7, 1), np.float32))) == [(0, 0, 7)]
    assert _ev(ref.decode(np.zeros((7, 1), np.float32))) == []


def test_reference_decoder_merges_gaps_before_dropping_short_events():
    p = np.zeros((20, 1), np.float32)
    p[2:4] = 0.9                                   # two frames
    p[6:8] = 0.9                                   # two frames, gap 2
    p[15] = 0.9                                    # one frame
    assert _ev(ref.decode(p, min_len=3)) == []
    assert _ev(ref.decode(p, min_gap=2, min_len=3)) == [(0, 2, 8)]                  # merged first, then long enough
    assert _ev(ref.decode(p, min_gap=1, min_len=3)) == []
    d = ref.decode(p, min_gap=7)
    assert _ev(d) == [(0, 2, 16)]
    p[10] = 0.95                                   # a run of its own inside the span: merged in, and the peak is there
    assert ref.decode(p, min_gap=7)["peak_frame"].tolist() == [10]


def test_reference_median_matches_scipy():
    from scipy import ndimage
    rng = np.random.default_rng(0)
    p = rng.random((300, 3)).astype(np.float32)
    p[100:140] = 0.5                               # ties
    for w in (1, 3, 5, 9, 31):
        np.testing.assert_array_equal(ref.median_nearest(p, w), ndimage.median_filter(p, size=(w, 1), mode="nearest"))


def test_window_planner_covers_every_output_frame():
    from sed_crnn_amd.detect import plan_windows
    for tf in (4, 8):
        for L in (tf * 4, 64):
            for hop in sorted({tf, L // 4 // tf * tf or tf, L // 2, L}):
                for N in list(range(tf, 3 * L)) + [10_000, 10_007]:
                    pl = plan_windows(N, tf, L, hop)
                    s, wl = ref.window_starts(N, tf, L, hop)
                    assert list(pl.starts) == s and pl.win_len == wl and pl.n_out == N // tf
                    cov = np.zeros(pl.n_out, int)
                    for st in pl.starts:
                        assert st % tf == 0 and st + pl.win_len <= N
                        cov[st // tf: st // tf + pl.win_out] += 1
                    assert (cov > 0).all(), (tf, L, hop, N)
                    assert pl.starts[-1] + pl.win_len == tf * pl.n_out                 # the last window is aligned to the end
                    if N < L:
                        assert pl.n_win == 1 and pl.win_len == tf * (N // tf)
                    # the kernel's start rule: min(w * hop_out, last_start_out)
                    assert [min(w * pl.hop_out, pl.last_start_out) for w in range(pl.n_win)] == [x // tf for x in pl.starts]


def test_window_planner_refuses_bad_arguments():
    from sed_crnn_amd.detect import plan_windows
    with pytest.raises(ValueError, match="time factor"):
        plan_windows(100, 8, 60, 32)
    with pytest.raises(ValueError, match="hop"):
        plan_windows(100, 8, 64, 12)
    with pytest.raises(ValueError, match="hop"):
        plan_windows(100, 8, 64, 72)
    with pytest.raises(ValueError, match="shorter than one output frame"):
        plan_windows(7, 8, 64, 32)
    plan_windows(8, 8, 64, 32)
    with pytest.raises(ValueError, match="uncovered"):
        plan_windows(1000, 8, 64, 32, trim=3)                  # 8 frames every 4: at most 2 trimmed per side
    plan_windows(1000, 8, 64, 32, trim=2)
    plan_windows(40, 8, 64, 32, trim=5)                        # one window touches both ends: nothing is trimmed


def test_detector_arguments_are_checked_without_a_gpu():
    import sed_crnn_amd as sed
    m = sed.LightningTimePooledCRNN(dropout=0.0)
    with pytest.raises(ValueError, match="median"):
        sed.EventDetector(m, median=4)
    with pytest.raises(ValueError, match="low"):
        sed.EventDetector(m, threshold=0.5, low=0.6)
    with pytest.raises(ValueError, match="combine"):
        sed.EventDetector(m, combine="sum")
    with pytest.raises(ValueError, match="uncovered"):
        sed.EventDetector(m, trim=3)
    with pytest.raises(TypeError):
        sed.EventDetector(object())
    det = sed.EventDetector(m)
    assert det.frame_seconds == pytest.approx(8 * 1024 / 44100)
    with pytest.raises(RuntimeError, match="eval"):
        det.from_features(np.zeros((100, 40), np.float32))


def test_detector_refuses_a_model_left_on_the_cpu_before_any_launch():
    """the kernels take raw device pointers: an eval() model that was never moved to the GPU must be refused up front (the
    features would otherwise stay on the host and reach sed_window_batch as host pointers)"""
    import sed_crnn_amd as sed
    det = sed.EventDetector(sed.LightningTimePooledCRNN(dropout=0.0).eval())
    for call in (lambda: det.from_features(np.zeros((100, 40), np.float32)), lambda: det(np.zeros(44_100, np.float32)),
                 lambda: sed.detect_events(det.model, np.zeros((100, 40), np.float32))):
        with pytest.raises(sed.SedHipError, match="move the module to the GPU first"):
            call()


def test_detect_entries_refuse_bad_sizes_without_a_gpu():
    import ctypes as C
    from sed_crnn_amd import _lib
    L = _lib.lib()
    assert L.sed_detect_workspace_bytes(466_000, 32, 0) == 2 * 32 * (466_000 // 64 + 1) * 8 + 2 * 32 * 4
    for bad in ((0, 1, 0), (-5, 1, 0), (100, 0, 0), (100, 33, 0), (100, 1, -1), (2**31, 1, 0), (2**30, 4, 0)):
        assert L.sed_detect_workspace_bytes(*bad) == 0, bad
    buf = (C.c_float * 64)()
    ws = (C.c_char * 4096)()
    cnt = C.c_int()
    a = C.cast(buf, C.c_void_p)
    # stitch: grid that does not end at n_out, trim that uncovers frames, bad combine
    for args, msg in (((a, 3, 8, 1, 4, 8, 17, 0, 0, a, None), b"end"),
                      ((a, 3, 8, 1, 4, 8, 16, 0, 3, a, None), b"uncovered"),
                      ((a, 3, 8, 1, 4, 8, 16, 2, 0, a, None), b"combine"),
                      ((a, 3, 8, 1, 4, 3, 11, 0, 0, a, None), b"last start"),
                      ((None, 3, 8, 1, 4, 8, 16, 0, 0, a, None), b"null")):
        assert L.sed_detect_stitch(*args) < 0, msg
        assert msg in L.sed_last_error_string(), (msg, L.sed_last_error_string())
    wsp, cp = C.cast(ws, C.c_void_p), C.cast(C.pointer(cnt), C.c_void_p)
    base = [a, 64, 1, 1, 0.5, 0.5, 0, 1, 0, wsp, 4096, None, None, None, None, None, cp, None]
    for i, v, msg in ((2, 33, b"bad sizes"), (3, 4, b"odd"), (3, 33, b"odd"), (4, 0.6, b"hi >= lo"), (6, -1, b"min_gap"),
                      (7, 0, b"min_len"), (8, 5, b"null output"), (10, 8, b"workspace")):
        args = list(base)
        args[i] = v
        assert L.sed_detect_events(*args) < 0, msg
        assert msg in L.sed_last_error_string(), (msg, L.sed_last_error_string())
