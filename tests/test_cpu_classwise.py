"""Class-wise decoder settings without a GPU: the argument handling of EventDetector / with_decoder,
SweepResult.best_per_class on a hand-made table, the three *_classwise symbols and their refusals (every check comes before the
first launch), the sizing of a class-wise stream, and the consistency of tests/classwise_ref.py's streaming restatement with
its offline definition."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import classwise_ref as cw  # noqa: E402
import detect_ref  # noqa: E402

FAKE = C.c_void_p(4096)          # a non-null device address: every call below is refused before anything is uploaded or launched
NAMES = ("sed_detect_events_classwise", "sed_detect_events_batch_classwise", "sed_stream_step_classwise")


def _err():
    from sed_crnn_amd._lib import lib
    return lib().sed_last_error_string().decode()


def _net(K=6):
    import sed_crnn_amd as sed
    return sed.LightningTimePooledCRNN(dropout=0.0, n_classes=K).eval()


# ───────────── 1. arguments ─────────────
def test_scalars_broadcast_and_any_sequence_makes_the_detector_classwise():
    import sed_crnn_amd as sed
    m = _net(6)
    scalar = sed.EventDetector(m, threshold=0.6, low=0.4, median=5, min_gap=2, min_len=3)
    assert scalar.classwise is False
    assert scalar.decoder_settings() == dict(threshold=0.6, low=0.4, median=5, min_gap=2, min_len=3)
    assert scalar.class_settings() == [scalar.decoder_settings()] * 6
    kw = cw.det_kwargs(cw.EXAMPLE)
    for as_seq in (list, tuple, np.asarray, torch.tensor):
        det = sed.EventDetector(m, **{k: as_seq(v) for k, v in kw.items()})
        assert det.classwise is True
        got = det.class_settings()
        assert [r["median"] for r in got] == kw["median"] and [r["min_gap"] for r in got] == kw["min_gap"]
        assert [r["min_len"] for r in got] == kw["min_len"]
        np.testing.assert_allclose([r["threshold"] for r in got], kw["threshold"], rtol=1e-6)      # a float32 tensor rounds
        np.testing.assert_allclose([r["low"] for r in got], kw["low"], rtol=1e-6)
        assert all(type(v) is list and len(v) == 6 for v in det.decoder_settings().values())
        assert det.median_max == 31
    # one sequence is enough, the scalars broadcast; equal entries are still class-wise
    det = sed.EventDetector(m, threshold=0.55, median=[3] * 6, min_gap=4)
    assert det.classwise and det.class_settings() == [dict(threshold=0.55, low=0.55, median=3, min_gap=4, min_len=1)] * 6
    # low=None: low_k = threshold_k, also entry by entry
    det = sed.EventDetector(m, threshold=[.3, .4, .5, .6, .7, .8])
    assert det.decoder_settings()["low"] == [.3, .4, .5, .6, .7, .8]
    det = sed.EventDetector(m, threshold=[.3, .4, .5, .6, .7, .8], low=[None, .1, None, .2, .3, None])
    assert det.decoder_settings()["low"] == [.3, .1, .5, .2, .3, .8]
    det = sed.EventDetector(m, threshold=0.5, low=[.1, .2, .3, .4, .5, .5])
    assert det.decoder_settings()["threshold"] == [0.5] * 6
    assert sed.EventDetector(_net(1), median=[7]).classwise


def test_wrong_lengths_and_bad_entries_name_the_class_and_the_argument():
    import sed_crnn_amd as sed
    m = _net(6)
    for name in ("threshold", "low", "median", "min_gap", "min_len"):
        with pytest.raises(ValueError, match=f"{name} has 5 entries, the net has 6 classes"):
            sed.EventDetector(m, **{name: [1] * 5})
    with pytest.raises(ValueError, match="median has 2 entries"):
        sed.EventDetector(m, median=np.ones((2, 3), np.int64))
    with pytest.raises(ValueError, match="class 3: median must be odd, 1..31, got 4"):
        sed.EventDetector(m, median=[1, 3, 5, 4, 7, 9])
    with pytest.raises(ValueError, match="class 5: median must be odd, 1..31, got 33"):
        sed.EventDetector(m, median=[1, 3, 5, 7, 7, 33])
    with pytest.raises(ValueError, match="class 2: low=0.7 must not exceed threshold=0.6"):
        sed.EventDetector(m, threshold=0.6, low=[.1, .6, .7, .2, .2, .2])
    with pytest.raises(ValueError, match="class 0: low=0.5 must not exceed threshold=0.4"):
        sed.EventDetector(m, threshold=[.4, .6, .6, .6, .6, .6], low=0.5)
    with pytest.raises(ValueError, match="class 4: min_gap must be >= 0, got -1"):
        sed.EventDetector(m, min_gap=[0, 0, 0, 0, -1, 0])
    with pytest.raises(ValueError, match="class 1: min_len must be >= 1, got 0"):
        sed.EventDetector(m, min_len=[1, 0, 1, 1, 1, 1])
    with pytest.raises(ValueError, match="class 1: median must be an integer, got 3.5"):
        sed.EventDetector(m, median=[1, 3.5, 1, 1, 1, 1])
    det = sed.EventDetector(m, median=[1, 3, 5, 7, 9, 11])
    with pytest.raises(ValueError, match="class 0: median"):
        det.with_decoder(median=[2, 3, 5, 7, 9, 11])
    with pytest.raises(ValueError, match="the track has 3 classes, the detector has settings for 6"):
        det._class_table(3)


def test_with_decoder_round_trips_both_kinds():
    import sed_crnn_amd as sed
    m = _net(6)
    scalar = sed.EventDetector(m, threshold=0.6, low=0.45, median=7, min_gap=1, min_len=2, hop=32, trim=1)
    again = scalar.with_decoder(**scalar.decoder_settings())
    assert not again.classwise and again.decoder_settings() == scalar.decoder_settings() and again.hop == 32 and again.trim == 1
    det = scalar.with_decoder(**cw.det_kwargs(cw.EXAMPLE))
    assert det.classwise and det.model is m and det.hop == 32 and det.trim == 1
    again = det.with_decoder(**det.decoder_settings())
    assert again.classwise and again.decoder_settings() == det.decoder_settings() and again.class_settings() == det.class_settings()
    assert [dict(lo=r["low"], hi=r["threshold"], median=r["median"], min_gap=r["min_gap"], min_len=r["min_len"])
            for r in det.class_settings()] == cw.EXAMPLE
    # one argument replaced: the rest stays class-wise; threshold without low resets low
    moved = det.with_decoder(min_gap=2)
    assert moved.classwise and moved.decoder_settings()["min_gap"] == [2] * 6 and moved.decoder_settings()["median"] == det.median
    assert det.with_decoder(threshold=0.7).decoder_settings()["low"] == [0.7] * 6
    back = det.with_decoder(**scalar.decoder_settings())
    assert not back.classwise and back.decoder_settings() == scalar.decoder_settings()
    with pytest.raises(TypeError, match="decoder settings only"):
        det.with_decoder(hop=16)


# ───────────── 2. best_per_class ─────────────
def _result(table):
    import sed_crnn_amd as sed
    table = np.asarray(table, np.int64)
    grid = sed.DecoderGrid.from_settings([dict(threshold=0.3 + 0.1 * g, median=1 + 2 * g, min_gap=g, min_len=1 + g)
                                          for g in range(table.shape[0])])
    res = sed.SweepResult(None, grid, 1, 5)
    res._table = table
    return res, grid


def test_best_per_class_on_a_hand_made_table():
    # columns: ev_tp, n_sys, n_ref, seg_tp, seg_sys, seg_ref; G = 4 settings, K = 4 classes
    t = np.zeros((4, 4, 6), np.int64)
    # class 0: event F1 best at g = 2 alone; segment F1 perfect at g = 1 and g = 3, ER 0 at both: the ties go to g = 1
    t[:, 0] = [[1, 4, 4, 2, 4, 4], [2, 4, 4, 4, 4, 4], [4, 4, 4, 3, 4, 4], [3, 4, 4, 4, 4, 4]]
    # class 1: the same counts in every setting -> ties everywhere -> g = 0
    t[:, 1] = [2, 3, 4, 2, 3, 4]
    # class 2: no reference at all: F1 = 0 everywhere, ER = x / 0 -> NaN or inf -> g = 0
    t[:, 2] = [[0, 0, 0, 0, 0, 0], [0, 1, 0, 0, 1, 0], [0, 2, 0, 0, 2, 0], [0, 0, 0, 0, 0, 0]]
    # class 3: ties between g = 1 and g = 3 only
    t[:, 3] = [[1, 5, 5, 1, 5, 5], [4, 5, 5, 4, 5, 5], [2, 5, 5, 2, 5, 5], [4, 5, 5, 4, 5, 5]]
    res, grid = _result(t)
    for metric, want in (("f1_event", [2, 0, 0, 1]), ("f1_segment", [1, 0, 0, 1]), ("er_segment", [1, 0, 0, 1])):
        g, sets, scores = res.best_per_class(metric)
        assert g.tolist() == want, metric
        cwise, _ = getattr(res, metric)()
        pick = np.where(np.isnan(cwise), np.inf, cwise) if metric == "er_segment" else -cwise
        for k in range(4):                                      # the definition: the first arg-best of the class's column
            assert g[k] == int(np.flatnonzero(pick[:, k] == pick[:, k].min())[0]), (metric, k)
            assert scores[k] == cwise[g[k], k] or (np.isnan(scores[k]) and np.isnan(cwise[g[k], k]))
        assert set(sets) == {"threshold", "low", "median", "min_gap", "min_len"}
        for k in range(4):
            assert {n: v[k] for n, v in sets.items()} == grid[int(g[k])], (metric, k)
    assert np.isnan(res.er_segment()[0][0, 2])                  # 0 / 0: counted as +inf, the class takes g = 0
    assert res.best_per_class()[0].tolist() == res.best_per_class("f1_event")[0].tolist()
    with pytest.raises(ValueError, match="metric must be"):
        res.best_per_class("accuracy")
    with pytest.raises(ValueError, match="empty grid"):
        _result(np.zeros((0, 4, 6)))[0].best_per_class()


def test_tune_decoder_per_class_builds_the_classwise_detector(monkeypatch):
    import sed_crnn_amd as sed
    t = np.zeros((3, 6, 6), np.int64)
    t[..., 1] = t[..., 2] = 4
    for k in range(6):
        t[k % 3, k, 0] = 4                                      # class k is perfect at g = k mod 3
    res, grid = _result(t)
    det = sed.EventDetector(_net(6), hop=32)
    monkeypatch.setattr(sed.EventDetector, "sweep", lambda self, track, ref, g, **kw: res)
    tuned, got = sed.tune_decoder(det, None, None, grid, per_class=True, average="macro")       # average is ignored
    assert got is res and tuned.classwise and tuned.hop == 32
    assert tuned.class_settings() == [grid[k % 3] for k in range(6)]
    one, _ = sed.tune_decoder(det, None, None, grid)
    assert not one.classwise and one.decoder_settings() == grid[0]
    assert "ignored" in sed.tune_decoder.__doc__


# ───────────── 3. symbols and refusals ─────────────
def test_symbols_are_in_the_library_the_header_and_the_signature_table():
    from sed_crnn_amd._lib import SIGNATURES, lib
    header = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "sedcrnn.h")).read()
    for name in NAMES:
        assert name in SIGNATURES and hasattr(lib(), name)
        assert re.search(rf"\bint {name}\(", header), name
    # the class-wise entries take the scalar entries' arguments with ONE table in place of the five decoder values
    for name in NAMES:                                           # (the stream entry keeps `median`: it sizes the state)
        scalar = SIGNATURES[name[:-len("_classwise")]][1]
        assert len(SIGNATURES[name][1]) == len(scalar) - (3 if "stream" in name else 4), name
    assert re.search(r"typedef sed_tune_setting sed_decoder_setting;", header)


def _table(rows):
    from sed_crnn_amd._lib import TuneSetting
    arr = (TuneSetting * len(rows))(*[TuneSetting(*r) for r in rows])
    return arr, C.cast(arr, C.c_void_p)


GOOD = [(1, .5, .5, 0, 1), (31, .4, .6, 17, 5), (3, .45, .45, 1, 2)]


def _bad_rows():
    """(rows, what the message says): one bad row each, in class 2, 0 and 1"""
    yield GOOD[:2] + [(4, .5, .5, 0, 1)], "class 2: median width must be odd"
    yield [(33, .5, .5, 0, 1)] + GOOD[1:], "class 0: median width must be odd"
    yield GOOD[:1] + [(3, .6, .5, 0, 1)] + GOOD[2:], "class 1: need hi >= lo"
    yield GOOD[:2] + [(3, .5, .5, -1, 1)], "class 2: min_gap >= 0 and min_len >= 1"
    yield GOOD[:2] + [(3, .5, .5, 0, 0)], "class 2: min_gap >= 0 and min_len >= 1"


def test_single_and_batch_entries_refuse_bad_tables_and_small_workspaces():
    from sed_crnn_amd._lib import lib
    L = lib()
    K, cap, n = 3, 10, 1000
    keep, good = _table(GOOD)
    need = L.sed_detect_workspace_bytes(n, K, cap)

    def single(tab=good, n_out=n, ws=need, k=K, outs=FAKE, max_events=cap, probs=FAKE, count=FAKE):
        return L.sed_detect_events_classwise(probs, n_out, k, tab, max_events, FAKE, ws, outs, outs, outs, outs, outs, count, None)

    for rows, msg in _bad_rows():
        hold, tab = _table(rows)
        assert single(tab) != 0 and f"detect_events_classwise: {msg}" in _err(), msg
    assert single(None) != 0 and "null pointer" in _err()
    assert single(probs=None) != 0 and "null pointer" in _err()
    assert single(count=None) != 0 and "null pointer" in _err()
    assert single(ws=need - 1) != 0 and "workspace" in _err()
    assert single(n_out=0) != 0 and "bad sizes" in _err()
    assert single(k=33) != 0 and "K=33" in _err()
    assert single(k=0) != 0 and "bad sizes" in _err()
    assert single(outs=None) != 0 and "null output pointer" in _err()
    assert single(max_events=-1) != 0 and "bad sizes" in _err()

    n_out = np.asarray([100, 1, 64, 65], np.int64)
    need = L.sed_detect_batch_workspace_bytes(int(n_out.sum()), K, 4, cap)

    def batch(tab=good, n=n_out, ws=need, rec=FAKE, k=K, event_off=FAKE):
        n = np.ascontiguousarray(np.asarray(n, np.int64))
        return L.sed_detect_events_batch_classwise(FAKE, C.c_void_p(n.ctypes.data), n.size, k, tab, cap, FAKE, ws, rec, FAKE, FAKE, FAKE,
                                                   FAKE, FAKE, event_off, None)

    for rows, msg in _bad_rows():
        hold, tab = _table(rows)
        assert batch(tab) != 0 and f"detect_events_batch_classwise: {msg}" in _err(), msg
    assert batch(None) != 0 and "null pointer" in _err()
    assert batch(event_off=None) != 0 and "null pointer" in _err()
    assert batch(n=[100, 0, 64, 65]) != 0 and "recording 1 has 0 output frames" in _err()
    assert batch(ws=need - 1) != 0 and "workspace" in _err()
    assert batch(rec=None) != 0 and "null output pointer" in _err()
    assert batch(k=33) != 0 and "K=33" in _err()
    assert batch(n=[2 ** 30, 2 ** 30]) != 0 and "2^31" in _err()
    assert L.sed_detect_events_batch_classwise(FAKE, None, 4, K, good, cap, FAKE, need, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE,
                                               None) != 0 and "null pointer" in _err()
    del keep


def test_stream_step_classwise_refuses_bad_tables_and_a_state_sized_for_another_width():
    from sed_crnn_amd._lib import lib
    L = lib()
    S, K, win_out, hop_out, max_new, max_dg = 2, 3, 8, 4, 2, 16
    keep, good = _table(GOOD)
    idle = [0, 0, 0, 0, 0, 0, 8, 0]
    step = [1, 0, 1, 8, 13, 0, 8, 0]

    def call(tab=good, median=31, table=(step, idle), state=None, ws=None, outs=FAKE, k=K, trim=0):
        t = np.ascontiguousarray(np.asarray(table, np.int64).reshape(-1, 8))
        state = L.sed_stream_state_bytes(S, k, win_out, hop_out, median, max_new) if state is None else state
        ws = L.sed_stream_step_workspace_bytes(S, k, max_dg) if ws is None else ws
        return L.sed_stream_step_classwise(FAKE, state, S, k, win_out, hop_out, median, max_new, 0, trim, tab, FAKE, 10_000,
                                           C.c_void_p(t.ctypes.data), max_dg, None, 0, 64, outs, outs, outs, outs, outs, outs, FAKE, FAKE,
                                           ws, None)

    for rows, msg in _bad_rows():
        hold, tab = _table(rows)
        assert call(tab) != 0 and f"stream_step_classwise: {msg}" in _err(), msg
    assert call(None) != 0 and "null pointer" in _err()
    # the state, the rings and the frontier belong to the WIDEST median of the classes: any other width is refused
    assert call(median=15) != 0 and "median=15 must be the widest median of the classes (31)" in _err()
    hold, narrow = _table([(1, .5, .5, 0, 1), (3, .5, .5, 0, 1), (5, .5, .5, 0, 1)])
    assert call(narrow, median=31) != 0 and "must be the widest median of the classes (5)" in _err()
    # ... and with it, the scalar entry's checks follow, under this entry's name
    assert call(state=100) != 0 and "stream_step_classwise: state of 100 bytes" in _err()
    assert call(ws=8) != 0 and "stream_step_classwise: workspace" in _err()
    assert call(outs=None) != 0 and "stream_step_classwise: null output pointer" in _err()
    assert call(k=33) != 0 and "K=33" in _err()
    assert call(trim=3) != 0 and "uncovered" in _err()
    assert call(table=([0, 0, 1, 8, 7, 0, 8, 0], idle)) != 0 and "stream_step_classwise: stream 0: n_out goes backwards" in _err()
    assert call(table=([3, 0, 1, 8, 21, 0, 8, 0], idle)) != 0 and "at most 2 per step" in _err()
    del keep


# ───────────── 4. a class-wise stream is sized with the widest median ─────────────
def test_stream_schedule_and_state_use_the_widest_median():
    import sed_crnn_amd as sed
    from sed_crnn_amd._lib import lib
    m = _net(6)
    det = sed.EventDetector(m, **cw.det_kwargs(cw.EXAMPLE))
    st = det.stream(n_streams=3)
    assert st.sched.r == 15 and st._dims == (3, 6, 8, 4, 31, 4)
    assert st._core_bytes == lib().sed_stream_state_bytes(3, 6, 8, 4, 31, 4) > lib().sed_stream_state_bytes(3, 6, 8, 4, 15, 4)
    wide = sed.EventDetector(m, median=31).stream(n_streams=3)
    assert st.state_bytes == wide.state_bytes and st.sched.r == wide.sched.r
    st.sched.advance(np.array([64 + 8 * 40, 64, 0]))
    assert st.sched.final_frames.tolist() == [40, 0, 0] and st.sched.decided.tolist() == [25, 0, 0]
    one = sed.EventDetector(m, median=[1, 1, 3, 1, 1, 1]).stream(n_streams=1)
    assert one.sched.r == 1 and one._dims[4] == 3
    with pytest.raises(sed.SedHipError, match="move the module to the GPU"):
        st.push_features([np.zeros((64, 40), np.float32)] * 3)


# ───────────── 5. the streaming restatement against its offline definition ─────────────
def _chunks(rng, n, how):
    if how == "all":
        return [n]
    out, left = [], n
    while left:
        c = 1 if how == "one" else int(min(left, rng.choice([1, 2, 3, 8, 40, 300])))
        out.append(c)
        left -= c
    return out


def _feed(rng, p, settings, how, win_out=8):
    """ClasswiseDecodeRef fed a track the way the stream releases it: rows below n_out - win_out are final"""
    d = cw.ClasswiseDecodeRef(settings)
    evs, given, now = [], 0, 0
    for c in _chunks(rng, len(p), how) + ["end"]:
        end = c == "end"
        now = len(p) if end else now + c
        upto = len(p) if end else max(0, now - win_out)
        evs.append(d.step(p[given:upto], end))
        if not end:
            assert d.decided == max(0, upto - d.R)
            for k, a in d.active():                              # an open kept run starts at or after its class's last emission
                assert 0 <= a < d.decided
        given = upto
    assert d.rows.shape[0] == 0 and d.active() == []             # the end restarts the feed
    return evs


def _union(evs):
    ev = {k: np.concatenate([e[k] for e in evs]) for k in cw.EVENT_KEYS}
    order = np.lexsort((ev["onset"], ev["cls"]))
    return {k: v[order] for k, v in ev.items()}


def _same(got, want, what):
    for k in ("cls", "onset", "offset", "peak_frame"):
        np.testing.assert_array_equal(got[k], want[k], err_msg=f"{what} {k}")
    np.testing.assert_array_equal(got["peak"].view(np.int32), want["peak"].view(np.int32), err_msg=f"{what} peak")


def test_classwise_reference_is_the_per_class_restriction_of_the_scalar_reference():
    rng = np.random.default_rng(7)
    p = cw.smooth(rng, 4097, 6)
    ev = cw.decode(p, cw.EXAMPLE)
    assert (np.diff(ev["cls"]) >= 0).all()
    for k, s in enumerate(cw.EXAMPLE):
        full = detect_ref.decode(p, **s)
        _same(cw.only(ev, k), {n: v[full["cls"] == k] for n, v in full.items()}, f"class {k}")


@pytest.mark.parametrize("seed", [7, 8])
def test_the_checked_example_tells_the_rows_apart(seed):
    for n in (4097, 4200, 8300):
        p = cw.smooth(np.random.default_rng(seed), n, 6)
        assert 0.36 < p.min() and p.max() < 0.64
        assert cw.example_is_discriminating(p), (seed, n)


def test_stream_restatement_equals_the_offline_classwise_reference_over_a_feeds_life():
    rng = np.random.default_rng(2)
    tracks = [rng.random((1200, 6)).astype(np.float32), cw.smooth(rng, 2500, 6),
              np.repeat(rng.random((300, 6)), 5, 0).astype(np.float32)]                  # plateaus: ties inside the median windows
    mixed = [dict(lo=.5, hi=.5, median=31, min_gap=0, min_len=1), dict(lo=.4, hi=.62, median=1, min_gap=9, min_len=3),
             dict(lo=.5, hi=.5, median=5, min_gap=2, min_len=1), dict(lo=.45, hi=.55, median=1, min_gap=0, min_len=1),
             dict(lo=.3, hi=.7, median=9, min_gap=40, min_len=2), dict(lo=.5, hi=.6, median=3, min_gap=1, min_len=4)]
    n = 0
    for t, p in enumerate(tracks):
        for s, settings in enumerate((cw.EXAMPLE, mixed, [mixed[2]] * 6)):
            want = cw.decode(p, settings)
            how = ("one", "random", "all")[(t + s) % 3]
            _same(_union(_feed(rng, p, settings, how)), want, f"track {t} settings {s} {how}")
            n += len(want["cls"])
    assert n > 1000
    # a short feed: shorter than the widest filter, shorter than a window
    for length in (1, 5, 20):
        p = cw.smooth(rng, length, 6)
        _same(_union(_feed(rng, p, cw.EXAMPLE, "one")), cw.decode(p, cw.EXAMPLE), f"{length} frames")


def test_a_narrow_class_waits_for_the_common_frontier():
    """class 0 (median 1, min_gap 0) next to a class with median 31: its event [10, 15) would be final with 16 decided frames,
    and it is — but frames are decided R = 15 later than class 0 alone would decide them"""
    p = np.full((80, 2), 0.1, np.float32)
    p[10:15, 0] = 0.9
    settings = [dict(lo=.5, hi=.5, median=1, min_gap=0, min_len=1), dict(lo=.5, hi=.5, median=31, min_gap=0, min_len=1)]
    d = cw.ClasswiseDecodeRef(settings)
    alone = cw.ClasswiseDecodeRef(settings[:1])
    first = first_alone = None
    for j in range(80):
        if len(d.step(p[j:j + 1])["cls"]) and first is None:
            first = j + 1                                        # rows held when the event came out
        if len(alone.step(p[j:j + 1, :1])["cls"]) and first_alone is None:
            first_alone = j + 1
    assert first_alone == 16 and first == 16 + 15
