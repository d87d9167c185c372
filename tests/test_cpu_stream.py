"""Live streams without a GPU: the schedule arithmetic of sed_crnn_amd/stream.py against plan_windows, the numpy restatement of
tests/stream_ref.py against the offline restatement of tests/detect_ref.py (union of emissions, final rows, emission timing), the
refusals of StreamDetector, and the argument checks of the sed_stream_* entries (they validate before touching the device)."""
import ctypes as C
import itertools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import detect_ref as ref  # noqa: E402
import stream_ref  # noqa: E402

FAKE = C.c_void_p(4096)          # a non-null device address: every call below is refused before anything is uploaded or launched


def _err():
    from sed_crnn_amd._lib import lib
    return lib().sed_last_error_string().decode()


def _chunks(rng, total, how):
    """a chunking of ``total`` items: 'one' at a time, 'all' at once, or random pieces (some empty)"""
    if how == "all":
        return [total]
    if how == "one":
        return [1] * total
    out = []
    while sum(out) < total:
        out.append(min(int(rng.choice([0, 1, 2, 3, 5, 8, 13, 40])), total - sum(out)))
    return out


# ───────────── 1. schedule ─────────────
def test_schedule_runs_every_window_of_the_offline_plan_once():
    import sed_crnn_amd as sed
    rng = np.random.default_rng(0)
    tf, L = 8, 64
    lengths = [8, 9, 15, 63, 64, 65, 71, 72, 96, 127, 128, 129, 1000, 1003, 2048] + [int(n) for n in rng.integers(8, 3000, 12)]
    for hop in (tf, L // 4, L // 2, L):
        for N in lengths:
            for how in ("one", "all", "random"):
                sc = sed.StreamSchedule(tf, L, hop, median=5)
                starts, frontier = [], 0
                for c in _chunks(rng, N, how):
                    starts += sc.advance(c)
                    assert sc.final_frames >= frontier
                    frontier = sc.final_frames
                    assert frontier == max(0, sc.N // tf - L // tf) and sc.decided == max(0, frontier - 2)
                    assert sc.keep_from() <= min([sc.n_win * hop] + ([((sc.N - L) // tf) * tf] if sc.N >= L else [0]))
                    assert sc.N - sc.keep_from() < L + tf
                extra, win_len, plan = sc.finish()
                want = sed.plan_windows(N, tf, L, hop)
                assert tuple(starts + extra) == want.starts and win_len == want.win_len, (hop, N, how)
                assert plan.n_out == N // tf >= frontier
    for N in (0, 1, 7):
        sc = sed.StreamSchedule(tf, L, 32)
        sc.advance(N)
        with pytest.raises(ValueError, match=f"a recording of {N} frames is shorter than one output frame"):
            sc.finish()
    with pytest.raises(ValueError, match="hop=12 must be a positive multiple"):
        sed.StreamSchedule(8, 64, 12)


# ───────────── 2. stream_ref against detect_ref ─────────────
def _feed_windows(rng, logits, starts_out, n_out, win_out, hop_out, how, **kw):
    """one StreamRef fed the offline grid's logits as n_out grows by ``how`` -> (events per step, rows per step, finals)"""
    K = logits.shape[2]
    st = stream_ref.StreamRef(K, win_out, hop_out, **kw)
    evs, rows, finals, given, now = [], [], [], 0, 0
    for c in _chunks(rng, n_out, how) + ["end"]:
        end = c == "end"
        now = n_out if end else now + c
        upto = len(starts_out) if end else stream_ref.regular_windows(now, win_out, hop_out)
        ev, r, f = st.step([logits[w][:min(win_out, n_out)] for w in range(given, upto)], now, end)
        given = upto
        evs.append(ev); rows.append(r); finals.append(f)
        assert f == (n_out if end else max(0, now - win_out))
    return evs, rows, finals


def _union(evs):
    ev = {k: np.concatenate([e[k] for e in evs]) for k in evs[0]}
    order = np.lexsort((ev["onset"], ev["cls"]))
    return {k: v[order] for k, v in ev.items()}


def _same(got, want, what):
    for k in ("cls", "onset", "offset", "peak_frame"):
        np.testing.assert_array_equal(got[k], want[k], err_msg=f"{what} {k}")
    np.testing.assert_array_equal(got["peak"].view(np.int32), want["peak"].view(np.int32), err_msg=f"{what} peak")


def test_stream_ref_equals_the_offline_reference_on_random_window_logits():
    rng = np.random.default_rng(1)
    win_out = 8
    grid = list(itertools.product(("mean", "max"), (0, 1), (1, 5, 31), (0, 2, 9), (1, 3)))
    n_events = 0
    for i, (combine, trim, median, min_gap, min_len) in enumerate(grid):
        hop_out = (1, 2, 4, 8)[i % 4]
        if hop_out + 2 * trim > win_out:
            hop_out = 2
        n_out = int(rng.choice([3, 7, 8, 9, 12, 16, 17, 40, 97, 203]))
        starts, Lw = ref.window_starts(n_out, 1, win_out, hop_out)
        K = 1 + i % 3
        walk = np.cumsum(rng.standard_normal((n_out + win_out, K)) * 0.9, 0)
        logits = np.stack([3 * np.sin(walk[s:s + win_out]) + 0.5 * rng.standard_normal((win_out, K)) for s in starts]).astype(np.float32)
        lo, hi = (0.5, 0.5) if i % 2 else (0.35, 0.7)
        track = ref.stitch(logits[:, :Lw], starts, n_out, combine, trim)
        want = ref.decode(track, lo, hi, median, min_gap, min_len)
        for how in ("one", "all", "random"):
            evs, rows, _ = _feed_windows(rng, logits, starts, n_out, win_out, hop_out, how, combine=combine, trim=trim, lo=lo, hi=hi,
                                         median=median, min_gap=min_gap, min_len=min_len)
            assert np.array_equal(np.concatenate(rows), track), (i, how)        # float64 on both sides, same order of additions
            _same(_union(evs), want, f"case {i} {how}")
        n_events += len(want["cls"])
    assert n_events > 100


def _feed_track(rng, p, how, win_out=8, **kw):
    """DecodeRef fed a track the way the stream releases it: n_out grows by ``how``, rows below n_out - win_out are final"""
    d = stream_ref.DecodeRef(p.shape[1], **kw)
    evs, given, now = [], 0, 0
    for c in _chunks(rng, len(p), how) + ["end"]:
        end = c == "end"
        now = len(p) if end else now + c
        upto = len(p) if end else max(0, now - win_out)
        evs.append(d.step(p[given:upto], end))
        given = upto
    return evs


def test_stream_ref_equals_the_offline_reference_on_random_and_smooth_tracks():
    rng = np.random.default_rng(2)
    tracks = [rng.random((1500, 2)).astype(np.float32)]
    walk = np.cumsum(rng.standard_normal((2500, 3)) * 0.15, 0)
    tracks.append((1 / (1 + np.exp(-np.sin(walk)))).astype(np.float32) * 0.6 + 0.2)
    tracks.append(np.repeat(rng.random((300, 2)), 5, 0).astype(np.float32))      # plateaus: ties inside the median windows
    for t, p in enumerate(tracks):
        for median, min_gap, min_len in itertools.product((1, 5, 31), (0, 2, 9), (1, 3)):
            for lo, hi in ((0.5, 0.5), (0.4, 0.62)):
                kw = dict(lo=lo, hi=hi, median=median, min_gap=min_gap, min_len=min_len)
                want = ref.decode(p, **kw)
                how = ("one", "random", "all")[(median + min_gap + min_len + t) % 3]
                _same(_union(_feed_track(rng, p, how, **kw)), want, f"track {t} {kw} {how}")


def test_the_pinned_timing_example():
    """median=1, min_gap=2, on-frames 10..14 with one above hi: (10, 15) is emitted in the step in which G first reaches 18"""
    p = np.full((40, 1), 0.1, np.float32)
    p[10:15] = 0.6
    p[12] = 0.9
    d = stream_ref.DecodeRef(1, lo=0.5, hi=0.8, median=1, min_gap=2)
    for g in range(40):
        ev = d.step(p[g:g + 1])
        assert d.decided == g + 1
        if g + 1 == 18:
            assert ev["onset"].tolist() == [10] and ev["offset"].tolist() == [15] and ev["peak_frame"].tolist() == [12]
        else:
            assert len(ev["cls"]) == 0, g
        assert d.active() == ([(0, 10)] if 12 <= g < 15 else []), g               # open from the frame that makes the run kept
    # a run that begins inside the gap holds the event back until it closes; kept -> merged, with the gap in the peak
    p[17:22] = 0.55
    p[20] = 0.95
    d = stream_ref.DecodeRef(1, lo=0.5, hi=0.8, median=1, min_gap=2)
    for g in range(40):
        ev = d.step(p[g:g + 1])
        if g + 1 == 25:                                                           # offset 22, G > 22 + 2
            assert (ev["onset"].tolist(), ev["offset"].tolist(), ev["peak_frame"].tolist()) == ([10], [22], [20])
        else:
            assert len(ev["cls"]) == 0, g
        if 20 <= g < 22:
            assert d.active() == [(0, 10)]                                        # the pending event's onset: they will merge


def test_one_run_of_50000_frames_fed_4_at_a_time():
    n = 50_000
    p = np.full((n + 10, 1), 0.9, np.float32)
    p[n:] = 0.1
    p[31_337] = p[40_000] = 0.97
    d = stream_ref.DecodeRef(1, lo=0.5, hi=0.95, median=1, min_gap=3)
    got = []
    for g in range(0, n + 10, 4):
        ev = d.step(p[g:g + 4])
        if len(ev["cls"]):
            got.append((d.decided, ev))
        if g == 31_336:
            assert d.active() == [(0, 0)]                                         # kept from the step that holds frame 31 337
        elif g == 31_332:
            assert d.active() == []
    ev = d.step(p[:0], end=True)
    assert len(ev["cls"]) == 0
    assert len(got) == 1
    G, ev = got[0]
    assert G == 50_004                                                            # the first step with G > 50 000 + 3
    assert (ev["onset"][0], ev["offset"][0], ev["peak_frame"][0], ev["peak"][0]) == (0, n, 31_337, np.float32(0.97))


# ───────────── 3. StreamDetector refuses before anything runs ─────────────
def test_stream_detector_arguments_and_refusals_without_a_gpu():
    import torch
    import sed_crnn_amd as sed
    m = sed.LightningTimePooledCRNN(dropout=0.0).eval()
    with pytest.raises(ValueError, match="median must be odd"):
        sed.StreamDetector(m, 2, median=4)
    with pytest.raises(ValueError, match="low=0.9 must not exceed"):
        sed.StreamDetector(m, 2, low=0.9)
    with pytest.raises(ValueError, match="hop=12 must be a positive multiple"):
        sed.EventDetector(m).stream(2) and sed.StreamDetector(m, 2, hop=12)
    with pytest.raises(ValueError, match="n_streams"):
        sed.StreamDetector(m, 0)
    st = sed.EventDetector(m, median=5, min_gap=2).stream(n_streams=3)
    assert st.det.median == 5 and st.S == 3
    a = st.state_bytes
    assert a == sed.StreamDetector(m, 3, median=5).state_bytes > 0               # sizes only: nothing is allocated yet
    with pytest.raises(ValueError, match="expected 3 waveform pieces"):
        st.push([np.zeros(10, np.float32)])
    with pytest.raises(ValueError, match="stream 1: expected a mono 1-D waveform"):
        st.push([None, np.zeros((2, 500), np.float32), None])
    with pytest.raises(ValueError, match=r"stream 2: expected features \[N, 40\]"):
        st.push_features([None, None, np.zeros((5, 41), np.float32)])
    with pytest.raises(sed.SedHipError, match="move the module to the GPU"):
        st.push([np.zeros(5000, np.float32)] * 3)                                # valid input, CPU model
    with pytest.raises(sed.SedHipError, match="move the module to the GPU"):
        st.push_features([torch.zeros(9, 40)] * 3)
    assert st._state is None and st.state_bytes == a and not st.sched.N.any()
    m.train()
    with pytest.raises(RuntimeError, match="needs model.eval"):
        st.push([np.zeros(5000, np.float32)] * 3)
    stereo = sed.TimePooledCRNN(conv_channels=32, dropout=0.0, in_channels=2, gru_hidden=32).eval()
    with pytest.raises(ValueError, match="use push_features"):
        sed.StreamDetector(stereo, 1).push([np.zeros(10, np.float32)])


# ───────────── 4. the library entries ─────────────
def test_stream_state_bytes_depends_on_its_arguments_only():
    from sed_crnn_amd._lib import lib
    L = lib()
    a = L.sed_stream_state_bytes(7, 3, 8, 4, 5, 4)
    WR, TR = 2 * 2 + 4 + 2, 4 + 8 + 5 * 4 + 2
    track = 7 * WR * 8 * 3 * 4 + 7 * TR * 3 * 4
    assert a == (track + 63) // 64 * 64 + 7 * 3 * 64
    assert L.sed_stream_state_bytes(7, 3, 8, 4, 5, 4) == a
    assert L.sed_stream_state_bytes(8, 3, 8, 4, 5, 4) > a and L.sed_stream_state_bytes(7, 3, 8, 4, 7, 4) > a
    for bad in ((0, 1, 8, 4, 1, 1), (1, 33, 8, 4, 1, 1), (1, 0, 8, 4, 1, 1), (1, 1, 8, 4, 4, 1), (1, 1, 8, 4, 33, 1), (1, 1, 8, 9, 1, 1),
                (1, 1, 8, 0, 1, 1), (1, 1, 0, 1, 1, 1), (1, 1, 8, 4, 1, 0), (70_000, 1, 8, 4, 1, 1)):
        assert L.sed_stream_state_bytes(*bad) == 0, bad
    assert L.sed_stream_step_workspace_bytes(0, 1, 4) == 0 and L.sed_stream_step_workspace_bytes(2, 33, 4) == 0
    assert L.sed_stream_append_workspace_bytes(0) == 0 and L.sed_stream_append_workspace_bytes(3) == 3 * 56


def _step_call(table, S=2, K=2, win_out=8, hop_out=4, median=3, max_new=2, state=None, ws=None, max_dg=16, logits_len=10_000,
               cap=64, outs=FAKE, trim=0, lo=0.5, hi=0.5, probs=None, probs_rows=0):
    from sed_crnn_amd._lib import lib
    L = lib()
    t = np.ascontiguousarray(np.asarray(table, np.int64).reshape(-1, 8))
    state = L.sed_stream_state_bytes(S, K, win_out, hop_out, median, max_new) if state is None else state
    ws = L.sed_stream_step_workspace_bytes(S, K, max_dg) if ws is None else ws
    return L.sed_stream_step(FAKE, state, S, K, win_out, hop_out, median, max_new, 0, trim, lo, hi, 0, 1, FAKE, logits_len,
                             C.c_void_p(t.ctypes.data), max_dg, probs, probs_rows, cap, outs, outs, outs, outs, outs, outs, FAKE, FAKE,
                             ws, None)


def test_stream_step_refuses_bad_arguments_without_a_gpu():
    idle = [0, 0, 0, 0, 0, 0, 8, 0]
    # a stream at n_out 8 -> 13: windows 0 (complete before) .. 1 (start 4, ends 12)
    good = [1, 0, 1, 8, 13, 0, 8, 0]
    assert _step_call([good, idle], K=33) != 0 and "K=33" in _err()
    assert _step_call([good, idle], median=4) != 0 and "median=4" in _err()
    assert _step_call([good, idle], state=100) != 0 and "state of 100 bytes" in _err()
    assert _step_call([good, idle], ws=8) != 0 and "workspace" in _err()
    assert _step_call([[0, 0, 1, 8, 7, 0, 8, 0], idle]) != 0 and "n_out goes backwards (7 after 8)" in _err()
    assert _step_call([good, idle], outs=None) != 0 and "null output pointer" in _err()
    assert _step_call([[0, 0, 1, 8, 13, 0, 8, 0], idle]) != 0 and "new windows" in _err()          # window 1 is due and missing
    assert _step_call([[2, 0, 1, 8, 13, 0, 8, 0], idle]) != 0 and "new windows" in _err()          # window 2 is not complete
    assert _step_call([[1, 0, 0, 8, 13, 0, 8, 0], idle]) != 0 and "windows done do not match" in _err()
    assert _step_call([good, idle], logits_len=15) != 0 and "leave the buffer" in _err()
    assert _step_call([[3, 0, 1, 8, 21, 0, 8, 0], idle]) != 0 and "at most 2 per step" in _err()
    assert _step_call([good, idle], max_dg=0) != 0 and "decides" in _err()
    assert _step_call([good, idle], trim=3) != 0 and "uncovered" in _err()
    assert _step_call([good, idle], lo=0.6) != 0 and "hi >= lo" in _err()
    assert _step_call([good, idle], probs=FAKE, probs_rows=4) != 0 and "leave probs" in _err()
    # the end: 13 frames -> the grid 0, 4, and one end-aligned window at 5; a stream that ends below win_out: one window of n_out
    assert _step_call([[1, 0, 1, 8, 13, 1, 8, 0], idle]) != 0 and "new windows" in _err()
    assert _step_call([[1, 0, 0, 0, 5, 1, 8, 0], idle]) != 0 and "new windows" in _err()           # must be 5 frames long
    assert _step_call([[0, 0, 0, 0, 0, 1, 8, 0], idle]) != 0 and "ends without one output frame" in _err()
    from sed_crnn_amd._lib import lib
    L = lib()
    need = L.sed_stream_state_bytes(2, 2, 8, 4, 3, 2)
    assert L.sed_stream_init(None, need, 2, 2, 8, 4, 3, 2, None) != 0 and "null pointer" in _err()
    assert L.sed_stream_init(FAKE, need - 1, 2, 2, 8, 4, 3, 2, None) != 0 and "bytes" in _err()
    bad = (C.c_int * 1)(2)
    assert L.sed_stream_reset(FAKE, need, 2, 2, 8, 4, 3, 2, bad, 1, None) != 0 and "stream 2 of 2" in _err()


def test_stream_append_refuses_bad_tables_without_a_gpu():
    from sed_crnn_amd._lib import lib
    L = lib()

    def call(table, S=2, stride=100, buf_len=200, fresh_len=50, work=FAKE, work_len=300, ws=None):
        t = np.ascontiguousarray(np.asarray(table, np.int64).reshape(-1, 7))
        ws = L.sed_stream_append_workspace_bytes(S) if ws is None else ws
        return L.sed_stream_append(FAKE, buf_len, stride, FAKE, fresh_len, work, work_len, C.c_void_p(t.ctypes.data), S, FAKE, ws, None)

    idle = [0] * 7
    assert call([[0, 30, 0, 20, 0, 50, 40], idle], ws=8) != 0 and "workspace" in _err()
    assert call([[0, 30, 0, 20, 0, 50, 40], idle], stride=101) != 0 and "bad sizes" in _err()
    assert call([[80, 30, 0, 20, 0, 0, 40], idle]) != 0 and "kept floats leave its region" in _err()
    assert call([[0, 30, 0, 20, 0, 70, 40], idle]) != 0 and "tail leaves its region" in _err()
    assert call([[0, 30, 0, 20, 0, 20, 40], idle]) != 0 and "overlap" in _err()
    assert call([[0, 30, 40, 20, 0, 50, 40], idle]) != 0 and "new floats leave" in _err()
    assert call([[0, 30, 0, 20, 0, 50, 60], idle]) != 0 and "bad counts" in _err()
    assert call([[0, 30, 0, 20, 0, 50, 40], [100, 10, 20, 5, 40, 150, 5]]) != 0 and "work floats" in _err()
    assert call([[0, 30, 0, 20, 0, 50, 40], idle], work_len=49) != 0 and "work floats" in _err()
    assert call([idle, [0, 30, 0, 20, 0, 150, 40]]) != 0 and "kept floats leave its region" in _err()   # another stream's floats
