"""Localising live streams on the MI355X: feature.ring_write + feature.event_tdoa_ring against feature.event_tdoa on
the linear prefix, bit for bit, wherever the ring wraps; the ring path once against float64; and the localising StreamDetector
end to end against the offline call.

The rings of the bitwise test are 8192, 10244 (no multiple of either hop: the wrap point moves through the frames) and 34820
samples per lane: an event of 33 frames needs 32 hops + 2048 samples in the ring, which only the third holds at either hop.
The recording is written in the pieces 1, 2047, 5000, 9000 and the rest; a ring takes at most its capacity per call, so the rest
goes in calls of at most 6000 samples, two of which end where a frame's first sample is exactly the oldest kept sample and one
sample later.  The event table runs after every call.

Measured on an MI355X, ring path against float64 (C = 2, hop 1024, cap 8192, 40000 samples, every frame in the ring as a
one-frame event; the newest of the 7 reads beyond the samples received): kernel error 5.68e-08, float32 yardstick 7.24e-08,
ratio 0.78 of the 8 allowed.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tdoa_ref  # noqa: E402
from test_gpu_detect import _assert_events_equal  # noqa: E402
from test_gpu_multichannel import _stereo, det2  # noqa: E402,F401
from test_gpu_resample import _feed  # noqa: E402
from test_gpu_spatial import _stereo16, det3  # noqa: E402,F401
from test_gpu_tdoa import DEGENERATE, DELAYS, _bits, _events, _reference, sed  # noqa: E402,F401

pytestmark = pytest.mark.gpu
N, N1 = 40000, 30000                                # samples of feed 0 and of feed 1
PIECES = (1, 2047, 5000, 9000)                      # ... then the rest
SUB = 6000                                          # the rest goes in calls of at most this many samples
MF, LAT, HIST = 40, 3, 45                           # max_frames, lat_frames, history_frames: every event of <= 40 frames passes the rule
KEYS = ("lag", "strength", "loc_frames", "acc")


def _stops(cap, hop):
    """the sample counts of feed 0 after every ring_write call, and the frame whose first sample is the oldest kept one at
    the stop ``exact`` (and one sample too old at ``exact + 1``)"""
    base = np.cumsum(PIECES).tolist()
    f = next(f for f in range(1, 400) if f * hop > 1024 and f * hop - 1024 + cap > base[-1] + 1)
    exact = f * hop - 1024 + cap
    assert exact + 1 < N
    marks = sorted(set(base + [exact, exact + 1, N]))
    stops, at = [], 0
    for m in marks:
        while m - at > min(SUB, cap):
            at += min(SUB, cap)
            stops.append(at)
        stops.append(m)
        at = m
    return stops, f, exact


def _wraps(f0, f1, hop, cap):
    """whether the samples of the frames [f0, f1) cross a multiple of cap (a wrap point of the ring)"""
    lo, hi = max(0, f0 * hop - 1024), (f1 - 1) * hop + 1024
    return lo // cap != (hi - 1) // cap


def _table(n, cap, hop, f_exact, exact):
    """[(kind, (onset, offset, peak_frame))] for a feed with n samples received"""
    n_feat, kept = 1 + n // hop, max(0, n - cap)
    last = n_feat - 1
    f_old = 0 if kept == 0 else -(-(kept + 1024) // hop)             # the oldest frame whose samples are all kept
    ev = [("frame0", (0, 1, 0)), ("last", (last, last + 1, last)), ("empty", (last, last, last)),
          ("beyond", (n_feat + 3, n_feat + 5, n_feat + 3)), ("negative", (-2, 3, 0)), ("rule_only", (last, last + 60, last))]
    if f_old <= last:
        ev += [("oldest", (f_old, f_old + 1, f_old)), ("multi", (f_old, n_feat, (f_old + last) // 2)),
               ("rule_only", (f_old, f_old + 100, f_old))]
        straddle = [f for f in range(f_old, n_feat) if f * hop >= 1024 and (f * hop - 1024) % cap + 2048 > cap]
        ev += [("straddle", (f, f + 1, f)) for f in straddle[:2]]
        if last - f_old + 1 >= 33 and _wraps(last - 32, last + 1, hop, cap):      # the newest 33 frames: two chunks, across the wrap
            ev.append(("long33", (last - 32, last + 1, last - 5)))
    if f_old > 0:
        ev.append(("too_old", (f_old - 1, f_old, f_old - 1)))
    if n == exact:
        assert f_exact * hop - 1024 == kept and f_exact == f_old
        ev.append(("exact", (f_exact, f_exact + 1, f_exact)))
    if n == exact + 1:
        assert f_exact * hop - 1024 == kept - 1
        ev.append(("one_older", (f_exact, f_exact + 1, f_exact)))
    return ev


def _located(row, n, cap, hop):
    """the host's statement of sed_event_tdoa_ring's range: (located, f0, f1, what refused it)"""
    from sed_crnn_amd.localize import event_frames, stream_locates
    a, b, pk = row
    n_feat = 1 + n // hop
    f0, f1 = event_frames(a, b, pk, 1, n_feat, MF)
    if f1 == f0:
        return False, 0, 0, "range"
    if not stream_locates(a, b, pk, 1, n_feat, MF, LAT, HIST):
        return False, 0, 0, "rule"
    if max(0, f0 * hop - 1024) < n - cap:
        return False, 0, 0, "memory"
    return True, f0, f1, None


def _ring_io(C, cap):
    """two feeds of C lanes: (signals, ring, linear planar buffer, clip offsets)"""
    x = [tdoa_ref.broadband(N, DELAYS[:C], seed=N + C), tdoa_ref.broadband(N1, DELAYS[:C][::-1], seed=N1 + C)]
    ring = torch.full((2 * C * cap,), float("nan"), device="cuda")           # a read of an unwritten entry would show
    lin = torch.from_numpy(np.concatenate([np.ascontiguousarray(s.T).reshape(-1) for s in x])).cuda()
    offs = [c * N for c in range(C)] + [C * N + c * N1 for c in range(C)]
    return x, ring, lin, offs


def _write(feature, ring, cap, x, have, upto, ws):
    """feed s from have[s] to upto[s] samples: one ring_write call over all 2 C lanes"""
    C = x[0].shape[1]
    pieces, table, at = [], [], 0
    for s in range(2):
        for c in range(C):
            p = x[s][have[s]:upto[s], c]
            table.append((at, len(p), have[s]))
            pieces.append(p)
            at += len(p)
    src = torch.from_numpy(np.concatenate(pieces)).cuda() if at else None
    return feature.ring_write(ring, cap, src, table, ws)


@pytest.mark.parametrize("cap", [8192, 10244, 34820])
@pytest.mark.parametrize("hop", [1024, 441])
@pytest.mark.parametrize("C", [2, 3, 5])
def test_ring_equals_linear_bit_for_bit(sed, C, hop, cap):
    from sed_crnn_amd import feature
    x, ring, lin, offs = _ring_io(C, cap)
    stops, f_exact, exact = _stops(cap, hop)
    kw = dict(max_lag=24, max_frames=MF, hop=hop, return_curve=True)
    rkw = dict(lat_frames=LAT, history_frames=HIST, **kw)
    have, ws, seen = [0, 0], None, {}
    for n in stops:
        upto = [n, min(N1, 1 + 3 * n // 4)]
        assert all(0 <= u - h <= cap for u, h in zip(upto, have))
        ws = _write(feature, ring, cap, x, have, upto, ws)
        have = upto
        # feed 0's table, three events of feed 1, and two that name no feed
        rows = _table(n, cap, hop, f_exact, exact)
        rec = [0] * len(rows)
        last1 = have[1] // hop
        rows += [("feed1", (0, 1, 0)), ("feed1", (last1, last1 + 1, last1)), ("feed1", (max(0, last1 - 3), last1 + 1, last1)),
                 ("rec_out", (0, 1, 0)), ("rec_out", (0, 1, 0))]
        rec += [1, 1, 1, 2, -1]
        want = [_located(r, have[q], cap, hop) if q in (0, 1) else (False, 0, 0, "rec") for (_, r), q in zip(rows, rec)]
        loc = np.array([w[0] for w in want])
        for (kind, _), w in zip(rows, want):
            seen.setdefault(kind, set()).add(w[3] or "located")
        assert loc.sum() >= 3 and (~loc).sum() >= 2, (n, rows, want)      # (on the host, before the launch)
        ev = _events([r for _, r in rows], rec)
        got = feature.event_tdoa_ring(ring, cap, have, C, ev, 1, **rkw)
        clips = [(o, have[0]) for o in offs[:C]] + [(o, have[1]) for o in offs[C:]]
        ref = feature.event_tdoa(lin, clips, C, ev, 1, **kw)
        assert np.array_equal(got["loc_frames"].cpu().numpy(), [w[2] - w[1] for w in want]), (n, rows)
        idx = torch.from_numpy(np.nonzero(loc)[0]).cuda()
        out = torch.from_numpy(np.nonzero(~loc)[0]).cuda()
        for k in KEYS:
            assert np.array_equal(_bits(got[k][idx]), _bits(ref[k][idx])), (C, hop, cap, n, k)
            assert not got[k][out].any() and torch.isfinite(got[k]).all(), (C, hop, cap, n, k)
        assert (ref["loc_frames"][idx] > 0).all()
        if n in (exact, N):
            # a permuted table gives permuted outputs (the feed column under the name a stream gives it)
            perm = np.random.default_rng(n).permutation(len(rows))
            shuffled = _events([rows[i][1] for i in perm], [rec[i] for i in perm])
            shuffled["stream"] = shuffled.pop("rec")
            sh = feature.event_tdoa_ring(ring, cap, have, C, shuffled, 1, **rkw)
            for k in KEYS:
                assert np.array_equal(_bits(sh[k]), _bits(got[k][torch.from_numpy(perm).cuda()])), (n, k)
            # two feeds with different n in one call: each equals its single-feed call on its own rings
            for q in (0, 1):
                sel = [i for i, r in enumerate(rec) if r == q]
                one = feature.event_tdoa_ring(ring[q * C * cap:(q + 1) * C * cap], cap, [have[q]], C, _events([rows[i][1] for i in sel]), 1, **rkw)
                for k in KEYS:
                    assert np.array_equal(_bits(one[k]), _bits(got[k][torch.tensor(sel).cuda()])), (n, q, k)
    assert have == [N, N1]
    # what the tables held over the run
    assert seen["frame0"] == {"located", "memory"}                        # with left zero padding while n <= cap; gone afterwards
    assert seen["exact"] == {"located"} and seen["one_older"] == {"memory"} and seen["too_old"] == {"memory"}
    assert seen["rule_only"] == {"rule"} and seen["rec_out"] == {"rec"} and seen["negative"] == seen["beyond"] == {"range"}
    assert "located" in seen["straddle"] and "located" in seen["multi"] and "located" in seen["feed1"]
    assert ("long33" in seen) == (cap == 34820) and seen.get("long33", {"located"}) == {"located"}
    # no events: empty tensors, nothing launched
    none = feature.event_tdoa_ring(ring, cap, have, C, _events(np.zeros((0, 3)), []), 1, max_lag=5, return_curve=True)
    P = C * (C - 1) // 2
    assert none["lag"].shape == (0, P) and none["loc_frames"].shape == (0,) and none["acc"].shape == (0, P, 13)
    assert none["loc_frames"].dtype == torch.int32 and none["lag"].is_cuda


def test_ring_write_refuses_more_than_the_ring_holds(sed):
    from sed_crnn_amd import feature
    ring = torch.zeros(2 * 4096, device="cuda")
    with pytest.raises(ValueError, match="0 to cap=4096"):
        feature.ring_write(ring, 4096, torch.zeros(5000, device="cuda"), [(0, 4097, 0), (0, 0, 0)])
    with pytest.raises(ValueError, match="do not fit"):
        feature.ring_write(ring, 4098, None, [(0, 0, 0), (0, 0, 0)])
    # a lane that wraps: samples 4000 .. 4199 of lane 1 land at 4000 .. 4095 and 0 .. 103; lane 0 and the rest stay as they were
    src = torch.arange(1, 201, device="cuda", dtype=torch.float32)
    feature.ring_write(ring, 4096, src, [(0, 0, 0), (0, 200, 4000)])
    got = ring.cpu().numpy()
    want = np.zeros(2 * 4096, np.float32)
    want[4096 + 4000:] = np.arange(1, 97)
    want[4096:4096 + 104] = np.arange(97, 201)
    assert np.array_equal(got, want)


def test_ring_path_against_float64(sed):
    """acc of every frame in the ring (one-frame events), C = 2, hop 1024, cap 8192 after the last piece, against
    tdoa_ref.frame_curves; bound: the project's 8 x the float32 torch.fft yardstick (test_gpu_tdoa's _reference)"""
    from sed_crnn_amd import feature
    C, hop, cap, max_lag = 2, 1024, 8192, 24
    x, c64, c32 = _reference(N, C, hop, "constant", DELAYS)
    c64, c32 = tdoa_ref.narrow(c64, max_lag), tdoa_ref.narrow(c32, max_lag)
    ring = torch.full((C * cap,), float("nan"), device="cuda")
    at, ws = 0, None
    while at < N:
        m = min(SUB, N - at)
        src = torch.from_numpy(np.concatenate([x[at:at + m, c] for c in range(C)])).cuda()
        ws = feature.ring_write(ring, cap, src, [(c * m, m, at) for c in range(C)], ws)
        at += m
    n_feat = 1 + N // hop
    f_old = -(-(N - cap + 1024) // hop)
    frames = list(range(f_old, n_feat))
    assert len(frames) == 7 and frames[-1] * hop + 1024 > N                  # the last one reads beyond the samples received
    got = feature.event_tdoa_ring(ring, cap, [N], C, _events([(f, f + 1, f) for f in frames]), 1, max_lag=max_lag, max_frames=8, hop=hop,
                                  return_curve=True)
    assert got["loc_frames"].tolist() == [1] * len(frames)
    acc = got["acc"].cpu().numpy().astype(np.float64)
    e_kernel, e_yard = np.abs(acc - c64[frames]).max(), np.abs(c32[frames].astype(np.float64) - c64[frames]).max()
    assert e_yard >= DEGENERATE
    print(f"ring path: kernel {e_kernel:.2e}  yardstick {e_yard:.2e}  ratio {e_kernel / e_yard:.2f}")
    assert e_kernel <= 8.0 * e_yard, (e_kernel, e_yard)


# ───────────── the detector ─────────────
SIZES = [1, 1, 159, 997, 0, 60_000, 3]              # test_stereo_streams_are_bitwise_the_offline_call's
COARSE = [30_000, 7, 100_001]
LOC_KEYS = ("lag", "strength", "loc_frames")


def _by_feed(outs, S):
    """the calls of one run -> per feed its events in (class, onset) order, as host arrays"""
    res = []
    for s in range(S):
        parts = [{k: v[o.event_offsets[s]:o.event_offsets[s + 1]].cpu().numpy() for k, v in o.events.items()} for o in outs]
        ev = {k: np.concatenate([p[k] for p in parts]) for k in parts[0]}
        assert (ev.pop("stream") == s).all()
        order = np.lexsort((ev["onset"], ev["cls"]))
        res.append({k: v[order] for k, v in ev.items()})
    return res


def _run(st, recs, second, sizes):
    """both feeds in pieces; feed 1 ends early and starts a second recording while feed 0 waits; then everything ends ->
    (events of the recordings, events of the second recording)"""
    outs = _feed(st, recs, sizes) + [st.flush([1])]
    later = _feed(st, [recs[0][:0], second], sizes) + [st.flush()]
    for o in outs + later:
        assert set(o.events) == {"stream", "cls", "onset", "offset", "peak", "peak_frame"} | set(LOC_KEYS)
        assert o.events["lag"].shape == (len(o), 1) and o.tdoa().shape == (len(o), 1) and o.sr == st.det.sr
        assert np.array_equal(o.tdoa(1), o.tdoa()[o.event_offsets[1]:o.event_offsets[2]])
    a, b = _by_feed(outs, 2), _by_feed(later, 2)
    first = [{k: np.concatenate([a[0][k], b[0][k]]) for k in a[0]}, a[1]]
    order = np.lexsort((first[0]["onset"], first[0]["cls"]))
    first[0] = {k: v[order] for k, v in first[0].items()}
    return first, b[1]


def _check(sed, det, st, got, w, what, everything=False):
    """one feed's streamed events against det(w): the five keys; lag / strength / loc_frames bit for bit where the rule locates
    the event, zeros elsewhere; -> (events, located)"""
    from sed_crnn_amd.localize import stream_locates
    one = det(w, sr=48000, channels=2)
    want = {k: v.cpu().numpy() for k, v in one.events.items()}
    five = ("cls", "onset", "offset", "peak", "peak_frame")
    _assert_events_equal({k: got[k] for k in five}, {k: want[k] for k in five}, what)
    n = sed.resample(w, 48000, channels=2, keep_channels=True).shape[1]
    tf, n_feat = det.model.time_factor, 1 + n // det.hop_length
    loc = np.array([stream_locates(a, b, p, tf, n_feat, det.localize_settings.max_frames, st.lat, st.history_frames)
                    for a, b, p in zip(want["onset"], want["offset"], want["peak_frame"])], bool).reshape(-1)
    assert (want["loc_frames"] > 0).all()
    assert (got["loc_frames"][loc] > 0).all(), what                         # the capacity proof, on the device: accepted = still in the ring
    for k in LOC_KEYS:
        assert np.array_equal(got[k][loc].view(np.int32), want[k][loc].view(np.int32)), (what, k)
        assert not got[k][~loc].any(), (what, k)
    assert not everything or loc.all(), what
    return len(loc), int(loc.sum())


def _stream_end_to_end(sed, plain, spatial, make):
    t = sed.TDOA(max_lag=12, max_frames=8)
    kw = dict(max_batch=1, median=3, mean=plain.mean, std=plain.std, spatial=spatial, localize=t)
    det = sed.EventDetector(plain.model, **kw)
    recs, second = [make(48000 * 8, 10), make(48000 * 8 + 4001, 11)], make(130_003, 20)
    tf = det.model.time_factor

    def run(d, history, sizes, what, everything=False):
        st = d.stream(2, history_frames=history, max_new_windows=1, input_sr=48000)
        first, again = _run(st, recs, second, sizes)
        n_ev = n_loc = 0
        for got, w, name in ((first[0], recs[0], "feed 0"), (first[1], recs[1], "feed 1"), (again, second, "feed 1, second recording")):
            e, l = _check(sed, d, st, got, w, f"{what}: {name}", everything)
            n_ev, n_loc = n_ev + e, n_loc + l
        print(f"{what}: lat {st.lat}, history {st.history_frames} frames, ring {st.cap} samples; {n_loc} of {n_ev} events located")
        return st, (first, again), n_ev, n_loc

    st, small, n_ev, n_loc = run(det, "min", SIZES, "history 'min'")
    assert st.lat == (0 + 1 + det.seq_len // tf + 1) * tf and st.history_frames == 8 + st.lat
    assert 2 * st.cap < recs[0].shape[0] * det.sr // 48000                  # the ring wraps at least twice
    assert n_loc >= 1
    with pytest.raises(ValueError, match="takes audio"):
        st.push_features([None, None])
    # a history that covers the whole recording: every event as offline
    whole = 1 + (48000 * 8 + 4001) // det.hop_length + st.lat
    _, big, n_ev2, n_loc2 = run(det, whole, SIZES, "history = the recording", everything=True)
    assert n_ev2 == n_ev == n_loc2
    # a second, coarser chunking: identical results
    for history, ref in (("min", small), (whole, big)):
        _, other, _, _ = run(det, history, COARSE, f"history {history}, coarse pieces")
        for a, b in zip(ref[0] + [ref[1]], other[0] + [other[1]]):
            assert set(a) == set(b)
            for k in a:
                assert np.array_equal(a[k].view(np.int32), b[k].view(np.int32)), (history, k)
    # class-wise settings: lat follows the largest min_gap
    K = det.model.dense[-1]
    cw = sed.EventDetector(plain.model, min_gap=[0, 2] + [0] * (K - 2) if K >= 2 else [2], **kw)     # (a one-class net: its own list)
    st, _, n_ev3, n_loc3 = run(cw, "min", SIZES, "class-wise")
    assert cw.classwise and st.lat == (2 + 1 + det.seq_len // tf + 1) * tf and n_ev3 >= 1


def test_localising_stream_of_a_two_channel_net(sed, det2):
    plain, _ = det2
    _stream_end_to_end(sed, plain, None, lambda n, seed: _stereo(n, 48000, seed))


def test_localising_stream_of_a_spatial_net(sed, det3):
    plain, _ = det3
    _stream_end_to_end(sed, plain, "gcc_phat", _stereo16)
