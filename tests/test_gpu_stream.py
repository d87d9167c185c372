"""Live streams on the MI355X (sed_crnn_amd/stream.py, csrc/stream.hip): the step kernel against the offline kernels (bitwise) and
the per-step numpy restatement of tests/stream_ref.py (emission timing), the streamed log-mel against feature.mbe (bitwise), and
the whole path against EventDetector on the concatenated input."""
import ctypes as C
import itertools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import detect_ref as ref  # noqa: E402
import stream_ref  # noqa: E402
from test_gpu_detect import _assert_events_equal, _decode_gpu  # noqa: E402
from test_gpu_detect_many import LENGTHS, _centre_on_threshold, _features, _nets  # noqa: E402

pytestmark = pytest.mark.gpu
KEYS = ("stream", "cls", "onset", "offset", "peak", "peak_frame")


@pytest.fixture(scope="module")
def sed():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    import sed_crnn_amd as s
    return s


def _bits(t):
    return t.cpu().numpy().view(np.int32)


def _np_events(ev, e0=0, e1=None):
    return {k: v[e0:e1].cpu().numpy() for k, v in ev.items() if k != "stream"}


def _union(evs):
    ev = {k: np.concatenate([e[k] for e in evs]) for k in ("cls", "onset", "offset", "peak", "peak_frame")}
    order = np.lexsort((ev["onset"], ev["cls"]))
    return {k: v[order] for k, v in ev.items()}


# ───────────── 1. the step kernel on synthetic window logits ─────────────
class _Driver:
    """sed_stream_step on its own: S streams in output frames (tf = 1), the caller supplies the logits of every window"""

    def __init__(self, sed, S, K, win_out, hop_out, max_new, combine, trim, lo, hi, median, min_gap, min_len):
        from sed_crnn_amd._lib import check, lib, ptr, stream_ptr
        self.S, self.K, self.win_out = S, K, win_out
        self.dims = (S, K, win_out, hop_out, median, max_new)
        self.args = ({"mean": 0, "max": 1}[combine], trim, lo, hi, min_gap, min_len)
        self.sched = [sed.StreamSchedule(1, win_out, hop_out, trim, median) for _ in range(S)]
        self.state = torch.empty(lib().sed_stream_state_bytes(*self.dims), dtype=torch.uint8, device="cuda")
        check(lib().sed_stream_init(ptr(self.state), self.state.numel(), *self.dims, stream_ptr()), "sed_stream_init")

    def step(self, advance, windows_of, ending=()):
        """advance [S] new output frames; windows_of(s, first, n, length) -> logits [n, length, K] of windows first..first+n-1
        -> per stream (events, rows, final frames, the new windows)"""
        from sed_crnn_amd._lib import check, lib, ptr, stream_ptr
        S, K = self.S, self.K
        table = np.zeros((S, 8), np.int64)
        flat, new, at, rows_n, dg, cap = [], [], 0, [], 0, 0
        for s, sc in enumerate(self.sched):
            prev, F0, G0, w0 = sc.n_out, sc.final_frames, sc.decided, sc.n_win
            starts = sc.advance(advance[s])
            Lw, end = self.win_out, s in ending
            if end:
                extra, Lw, _ = sc.finish()
                starts = starts + extra
            lg = windows_of(s, w0, len(starts), Lw)
            new.append([lg[i] for i in range(len(starts))])
            flat.append(lg.reshape(-1))
            F1, G1 = (sc.n_out, sc.n_out) if end else (sc.final_frames, sc.decided)
            table[s] = (len(starts), at, w0, prev, sc.n_out, int(end), Lw, sum(rows_n))
            at += lg.size
            rows_n.append(F1 - F0)
            dg = max(dg, G1 - G0)
            cap += K * ((G1 - G0) // 2 + 2)
        logits = torch.from_numpy(np.concatenate(flat + [np.zeros(1, np.float32)])).cuda()
        ws = torch.empty(lib().sed_stream_step_workspace_bytes(S, K, dg), dtype=torch.uint8, device="cuda")
        ev = torch.full((6, cap), -7, dtype=torch.int32, device="cuda")
        off = torch.zeros(S + 1, dtype=torch.int32, device="cuda")
        probs = torch.full((sum(rows_n) + 1, K), -1.0, device="cuda")
        check(lib().sed_stream_step(ptr(self.state), self.state.numel(), *self.dims, *self.args, ptr(logits), at,
                                    C.c_void_p(table.ctypes.data), dg, ptr(probs), sum(rows_n), cap, *(ptr(ev[i]) for i in range(6)),
                                    ptr(off), ptr(ws), ws.numel(), stream_ptr()), "sed_stream_step")
        offs = off.cpu().tolist()
        assert offs[-1] <= cap
        ev = ev.cpu().numpy()
        assert (ev[0, :offs[-1]] == np.repeat(np.arange(S), np.diff(offs))).all()
        assert (probs[-1] == -1.0).all()
        probs = probs.cpu().numpy()
        out, r0 = [], 0
        for s, sc in enumerate(self.sched):
            e = {k: (ev[i, offs[s]:offs[s + 1]].view(np.float32) if k == "peak" else ev[i, offs[s]:offs[s + 1]])
                 for i, k in enumerate(KEYS) if k != "stream"}
            final = sc.n_out if s in ending else sc.final_frames
            out.append((e, probs[r0:r0 + rows_n[s]], final, new[s]))
            r0 += rows_n[s]
            if s in ending:
                sc.reset()
        return out


def _stitch_offline(logits, plan, combine, trim):
    from sed_crnn_amd._lib import check, lib, ptr, stream_ptr
    lg = torch.from_numpy(np.ascontiguousarray(logits)).cuda()
    out = torch.empty(plan.n_out, logits.shape[2], device="cuda")
    check(lib().sed_detect_stitch(ptr(lg), plan.n_win, plan.win_out, logits.shape[2], plan.hop_out, plan.last_start_out, plan.n_out,
                                  {"mean": 0, "max": 1}[combine], trim, ptr(out), stream_ptr()), "sed_detect_stitch")
    return out.cpu().numpy()


def _run_step_case(sed, rng, K, hop_out, combine, trim, lo, hi, median, min_gap, min_len, what):
    win_out, max_new, S = 8, 3, 7
    # stream -> its recordings, one after another (stream 3 is flushed and restarted; 5 is shorter than a window; 6 gets
    # nothing in many calls)
    recs = {0: [203], 1: [97], 2: [16], 3: [40, 57], 4: [131], 5: [5], 6: [64]}
    kw = dict(combine=combine, trim=trim, lo=lo, hi=hi, median=median, min_gap=min_gap, min_len=min_len)
    drv = _Driver(sed, S, K, win_out, hop_out, max_new, **kw)
    refs = [stream_ref.StreamRef(K, win_out, hop_out, **kw) for _ in range(S)]
    plans, grids, idx, got = {}, {}, [0] * S, {}

    def grid(s):
        key = (s, idx[s])
        if key not in grids:
            n = recs[s][idx[s]]
            plans[key] = sed.plan_windows(n, 1, win_out, hop_out, trim)
            walk = np.cumsum(rng.standard_normal((n + win_out, K)) * 0.9, 0)
            grids[key] = np.stack([3 * np.sin(walk[st:st + plans[key].win_len]) + 0.4 * rng.standard_normal((plans[key].win_len, K))
                                   for st in plans[key].starts]).astype(np.float32)
        return grids[key]

    def windows_of(s, first, n, length):
        if n == 0:
            return np.zeros((0, length, K), np.float32)
        g = grid(s)
        assert g.shape[1] == length
        return g[first:first + n]

    left = {s: recs[s][0] for s in range(S)}
    calls = 0
    while any(idx[s] < len(recs[s]) for s in range(S)):
        adv, ending = [0] * S, set()
        for s in range(S):
            if idx[s] >= len(recs[s]) or (s == 6 and calls % 3) or (s == 1 and calls % 5 == 4):
                continue
            adv[s] = min(left[s], int(rng.choice([0, 1, 2, 3, hop_out, max_new * hop_out])))
            left[s] -= adv[s]
            if left[s] == 0:
                ending.add(s)
        out = drv.step(adv, windows_of, ending)
        calls += 1
        for s in range(S):
            e, rows, final, new = out[s]
            if idx[s] >= len(recs[s]):
                assert len(e["cls"]) == 0 and len(rows) == 0
                continue
            n_now = recs[s][idx[s]] - left[s]
            want_ev, want_rows, want_final = refs[s].step(new, n_now, s in ending, rows=rows)
            assert final == want_final, (what, s, calls)
            assert np.abs(rows - want_rows).max(initial=0) < 1e-6, (what, s, calls)
            _assert_events_equal(e, want_ev, f"{what} stream {s} call {calls}")
            got.setdefault((s, idx[s]), []).append((e, rows))
            if s in ending:
                idx[s] += 1
                if idx[s] < len(recs[s]):
                    left[s] = recs[s][idx[s]]
    for key, parts in got.items():
        track = np.concatenate([p[1] for p in parts])
        want = _stitch_offline(grids[key], plans[key], combine, trim)
        assert np.array_equal(track.view(np.int32), want.view(np.int32)), (what, key)
        c, ev = _decode_gpu(track, lo=lo, hi=hi, median=median, min_gap=min_gap, min_len=min_len)
        _assert_events_equal(_union([p[0] for p in parts]), ev, f"{what} {key} union")
    return sum(len(p[0]["cls"]) for parts in got.values() for p in parts)


def test_step_kernel_is_exact_against_the_offline_kernels_and_the_per_step_reference(sed):
    rng = np.random.default_rng(7)
    n = 0
    for i, (combine, trim, median, min_gap, min_len) in enumerate(itertools.product(("mean", "max"), (0, 1), (1, 5, 31), (0, 2, 9),
                                                                                  (1, 3))):
        hop_out = (1, 2, 4, 8)[i % 4]
        if hop_out + 2 * trim > 8:
            hop_out = 2
        lo, hi = (0.5, 0.5) if i % 2 else (0.35, 0.7)
        n += _run_step_case(sed, rng, 1 + i % 3, hop_out, combine, trim, lo, hi, median, min_gap, min_len,
                            f"{combine} trim {trim} median {median} gap {min_gap} len {min_len} hop {hop_out}")
    assert n > 100                                                    # the cases are not vacuous
    assert _run_step_case(sed, rng, 32, 4, "mean", 0, 0.4, 0.6, 3, 1, 1, "K=32") > 50


@pytest.mark.parametrize("median", range(1, 32, 2))
def test_step_kernel_every_median_width(sed, median):
    """every instantiation of the step's median (one per width the decoder accepts) against the per-step reference, the
    offline stitch (bitwise) and the offline decoder; at least 10 events per width, so that no width passes on nothing"""
    n = _run_step_case(sed, np.random.default_rng(11), K=2, hop_out=4, combine="mean", trim=0, lo=0.5, hi=0.5, median=median,
                       min_gap=0, min_len=1, what=f"median {median}")
    print(f"median {median}: {n} events")
    assert n >= 10


def test_step_kernel_pinned_timing_and_a_run_of_50000_frames(sed):
    """(10, 15) with min_gap 2 leaves in the step in which G first reaches 18; one run of 50 000 frames fed 4 at a time is ONE
    event, with the first arg-max, in the step the rule gives — the peak is a running value in the state"""
    big = 30.0

    def run(track_logit, n, feed, min_gap, lo, hi, stop_at=None):
        drv = _Driver(sed, 1, 1, 8, 8, 4, "mean", 0, lo, hi, 1, min_gap, 1)
        seen, now = [], 0

        def windows_of(s, first, cnt, length):
            if cnt == 0:
                return np.zeros((0, length, 1), np.float32)
            return np.stack([track_logit[(first + i) * 8:(first + i) * 8 + 8] for i in range(cnt)]).reshape(cnt, 8, 1).astype(np.float32)
        while now < n:
            a = min(feed, n - now)
            now += a
            (e, rows, final, _), = drv.step([a], windows_of)
            if len(e["cls"]):
                seen.append((final, e))
        return seen
    x = np.full(80, -big, np.float32)
    x[10:15] = 0.5
    x[12] = 3.0
    seen = run(x, 80, 1, 2, 0.5, 0.8)
    assert len(seen) == 1 and seen[0][0] == 18                        # median 1: G = the final frames
    assert (seen[0][1]["onset"][0], seen[0][1]["offset"][0], seen[0][1]["peak_frame"][0]) == (10, 15, 12)
    n = 50_000
    x = np.full(n + 40, 2.0, np.float32)
    x[n:] = -big
    x[31_337] = x[40_000] = 4.0
    seen = run(x, n + 40, 4, 3, 0.5, 0.95)
    assert len(seen) == 1
    G, e = seen[0]
    assert G == 50_004                                                # final frames are multiples of 4 here: the first G > 50 003
    assert (e["onset"][0], e["offset"][0], e["peak_frame"][0]) == (0, n, 31_337)
    assert abs(float(e["peak"][0]) - 1.0 / (1.0 + np.exp(-4.0))) < 1e-6


# ───────────── 2. log-mel over pushes ─────────────
def test_streamed_logmel_rows_are_bitwise_the_offline_rows(sed):
    from sed_crnn_amd import data, feature
    rng = np.random.default_rng(3)
    m = sed.LightningTimePooledCRNN(dropout=0.0).cuda().eval()
    lengths = [44_100 * 2 + 17, 1, 1023, 1024, 1025, 2048, 30_000, 5 * 1024]
    waves = [(0.3 * rng.standard_normal(n)).astype(np.float32) for n in lengths]
    mean, std = data.standard_scaler_fit(feature.mbe(torch.from_numpy(waves[0]).cuda()))
    for scaler in (False, True):
        kw = dict(mean=mean, std=std) if scaler else {}
        st = sed.StreamDetector(m, len(waves), **kw)
        st._ready()
        got, at = [[] for _ in waves], [0] * len(waves)
        sizes = [1, 3, 1000, 1023, 1024, 1025, 2047, 4097, 0, 777, 20_001, 5, 1]
        call = 0
        while any(a < n for a, n in zip(at, lengths)):
            takes = [min(n - a, sizes[(call + 3 * s) % len(sizes)]) for s, (a, n) in enumerate(zip(at, lengths))]
            parts = [torch.from_numpy(w[a:a + t]) for w, a, t in zip(waves, at, takes) if t]
            fresh = torch.cat(parts).cuda() if parts else None
            mel, row0, rows = st._logmel_round(fresh, takes, np.zeros(len(waves), bool))
            for s in range(len(waves)):
                if rows[s]:
                    got[s].append(mel[row0[s]:row0[s] + rows[s]])
                assert st._fdone[s] == (at[s] + takes[s]) // 1024
            at = [a + t for a, t in zip(at, takes)]
            call += 1
        mel, row0, rows = st._logmel_round(None, [0] * len(waves), np.ones(len(waves), bool))
        for s, w in enumerate(waves):
            got[s].append(mel[row0[s]:row0[s] + rows[s]])
            want = feature.mbe(torch.from_numpy(w).cuda(), **kw)
            assert np.array_equal(_bits(torch.cat(got[s])), _bits(want)), (scaler, s)


# ───────────── 3. end to end ─────────────
def _collect(outs, S):
    """the calls of one run -> per stream (track rows, events in order of emission)"""
    tracks, evs = [[] for _ in range(S)], [[] for _ in range(S)]
    for o in outs:
        for s in range(S):
            tracks[s].append(o.probs[o.prob_offsets[s]:o.prob_offsets[s + 1]])
            evs[s].append(_np_events(o.events, o.event_offsets[s], o.event_offsets[s + 1]))
            assert (o.events["stream"][o.event_offsets[s]:o.event_offsets[s + 1]] == s).all()
    return [torch.cat(t) for t in tracks], [_union(e) for e in evs]


def _check_against_offline(det, track, ev, one, what):
    d = (track - one.probs).abs().max().item()
    print(f"{what}: max |dp| streamed vs offline {d:.2e}, {len(ev['cls'])} events")
    assert track.shape == one.probs.shape and d <= 2e-6, (what, d)
    _assert_events_equal(ev, {k: v.cpu().numpy() for k, v in det.decode(track).items()}, f"{what} vs decode(streamed track)")
    assert det.lo == det.hi and det.min_gap == 0 and det.min_len == 1      # then an event frame is a frame with p' > threshold
    p = ref.median_nearest(one.probs.cpu().numpy(), det.median)
    sure = (np.abs(p - np.float32(det.lo)) > 1e-5) & (np.abs(p - np.float32(det.hi)) > 1e-5)
    mg = ref.event_mask(ev, one.plan.n_out, p.shape[1])
    mo = ref.event_mask({k: v.cpu().numpy() for k, v in one.events.items()}, one.plan.n_out, p.shape[1])
    assert np.array_equal(mg[sure], mo[sure]), what
    return d


def _push_all(st, pieces_of, sizes, push):
    """feed every stream its input in pieces of the given sizes (cycled, shifted per stream), then flush"""
    S = st.S
    at, outs, call = [0] * S, [], 0
    total = [len(pieces_of(s)) for s in range(S)]
    while any(a < n for a, n in zip(at, total)):
        takes = [min(total[s] - at[s], sizes[(call + s) % len(sizes)]) for s in range(S)]
        outs.append(push([pieces_of(s)[at[s]:at[s] + t] if t or (call + s) % 2 else None for s, t in enumerate(takes)]))
        at = [a + t for a, t in zip(at, takes)]
        call += 1
        for s in range(S):
            assert outs[-1].final_frames[s] == st.sched.final_frames[s]
    outs.append(st.flush())
    return outs


@pytest.mark.parametrize("which", ["lightning", "timepooled", "stereo"])
def test_stream_end_to_end_equals_the_offline_detector(sed, which):
    r, m = _nets(sed, which, seed=21)
    F = 40 * m.in_channels
    lengths = [LENGTHS[i] for i in (6, 2, 5, 9, 0)]                   # 10 007, 63, 1000, 3001, 8
    mels = [_features(N, seed=30 + i, F=F) for i, N in enumerate(lengths)]
    _centre_on_threshold(r, m, mels[0])
    det = sed.EventDetector(m, median=3)
    st = det.stream(n_streams=5, keep_probs=True)
    outs = _push_all(st, lambda s: mels[s], [32, 1, 7, 500, 64, 0, 33], st.push_features)
    tracks, evs = _collect(outs, 5)
    assert outs[-1].final_frames == [N // 8 for N in lengths]
    n = 0
    for s, x in enumerate(mels):
        one = det.from_features(torch.from_numpy(x).cuda())
        _check_against_offline(det, tracks[s], evs[s], one, f"{which} features stream {s}")
        n += len(evs[s]["cls"])
        assert len(outs[-1].intervals(s, 0)) == int((outs[-1].events["cls"][outs[-1].event_offsets[s]:outs[-1].event_offsets[s + 1]] == 0).sum())
    assert n > 0
    if m.in_channels != 1:
        return
    from sed_crnn_amd import data, feature
    rng = np.random.default_rng(5)
    samples = [44_100 * 20 + 17, 63 * 1024 + 1000, 8 * 1024, 300_000, 1024 * 200 - 1]
    t = [np.arange(n) / 44_100 for n in samples]
    waves = [(0.1 * rng.standard_normal(n) + np.sin(2 * np.pi * 800 * tt) * (np.sin(2 * np.pi * 0.3 * tt) > 0)).astype(np.float32)
             for n, tt in zip(samples, t)]
    mean, std = data.standard_scaler_fit(feature.mbe(torch.from_numpy(waves[0]).cuda()))
    det = sed.EventDetector(m, mean=mean, std=std, median=3)
    st = det.stream(n_streams=5, keep_probs=True)
    outs = _push_all(st, lambda s: waves[s], [32_768, 1, 1000, 0, 100_000, 1023, 4097], st.push)
    tracks, evs = _collect(outs, 5)
    for s, w in enumerate(waves):
        _check_against_offline(det, tracks[s], evs[s], det(w), f"{which} waves stream {s}")
    # host and device pieces, everything at once: the same
    st2 = det.stream(n_streams=5, keep_probs=True)
    o = [st2.push([torch.from_numpy(w).cuda() for w in waves]), st2.flush()]
    tracks2, evs2 = _collect(o, 5)
    for s in range(5):
        assert (tracks2[s] - tracks[s]).abs().max().item() <= 2e-6
        _assert_events_equal(evs2[s], {k: v.cpu().numpy() for k, v in det.decode(tracks2[s]).items()}, f"at once {s}")


def test_1024_feeds_pushed_together_equal_the_offline_detector(sed):
    """the README's live-stream headline: 1024 feeds per push.  Every push hands the eval forward a few thousand windows, which
    run in chunks of max_batch = 1024 — the GRU's four-row batch tile, which nothing smaller reaches.  Feeds of 200..499 feature
    frames (every length different from its neighbours'), pushed in three calls and a flush; 16 sampled feeds (the first, the
    last and 14 spread between) against the offline detector on the same features, the final frame count of all 1024."""
    S = 1024
    r, m = _nets(sed, "lightning", seed=21)
    lengths = [200 + (s * 37) % 300 for s in range(S)]
    mels = [_features(N, seed=500 + s) for s, N in enumerate(lengths)]
    _centre_on_threshold(r, m, _features(10_007, seed=30))
    det = sed.EventDetector(m, median=3)
    assert det.max_batch == 1024
    st = det.stream(n_streams=S, keep_probs=True)
    outs = _push_all(st, lambda s: mels[s], [200, 150, 300], st.push_features)
    assert len(outs) <= 4                                            # three pushes at the most, and the flush
    assert outs[-1].final_frames == [N // 8 for N in lengths]
    tracks, evs = _collect(outs, S)
    sample = sorted({0, S - 1} | {(s * 73 + 5) % S for s in range(14)})
    assert len(sample) == 16
    n = 0
    for s in sample:
        one = det.from_features(torch.from_numpy(mels[s]).cuda())
        _check_against_offline(det, tracks[s], evs[s], one, f"1024 feeds, feed {s} ({lengths[s]} frames)")
        n += len(evs[s]["cls"])
    assert n > 0
    assert all(t.shape[0] == N // 8 for t, N in zip(tracks, lengths))


def test_stream_is_bitwise_the_offline_track_at_the_same_chunk_sizes(sed):
    """one stream pushed one window hop at a time runs every window at batch 1, like the offline detector with max_batch=1"""
    r, m = _nets(sed, "lightning", seed=4)
    mel = _features(1_003, seed=8)
    _centre_on_threshold(r, m, mel)
    det = sed.EventDetector(m, max_batch=1, min_gap=1)
    st = det.stream(n_streams=1, keep_probs=True)
    outs = [st.push_features([mel[a:a + 32]]) for a in range(0, len(mel), 32)] + [st.flush()]
    tracks, evs = _collect(outs, 1)
    one = det.from_features(torch.from_numpy(mel).cuda())
    assert torch.equal(tracks[0], one.probs)
    _assert_events_equal(evs[0], {k: v.cpu().numpy() for k, v in one.events.items()}, "batch 1")
    assert len(evs[0]["cls"]) > 0


def test_neighbours_do_not_matter_and_runs_repeat_bitwise(sed):
    r, m = _nets(sed, "lightning", seed=6)
    mel = _features(2_000, seed=11)
    _centre_on_threshold(r, m, mel)
    others = [_features(700 + 13 * i, seed=100 + i) for i in range(65)]       # slot `where` is replaced
    det = sed.EventDetector(m, median=5)

    def run(S, where):
        st = det.stream(n_streams=S, keep_probs=True)
        outs = []
        for a in range(0, len(mel), 96):
            pieces = [others[i][a:a + 96] if a < len(others[i]) else None for i in range(S)]
            pieces[where] = mel[a:a + 96]
            outs.append(st.push_features(pieces))
        outs.append(st.flush())
        tracks, evs = _collect(outs, S)
        return tracks[where], evs[where]
    alone, ev_alone = run(1, 0)
    among, ev_among = run(65, 40)
    again, ev_again = run(65, 40)
    assert torch.equal(among, again)
    _assert_events_equal(ev_among, ev_again, "repeat")
    d = (alone - among).abs().max().item()
    print(f"alone vs among 64: max |dp| {d:.2e}")
    assert d <= 2e-6
    pf = ref.median_nearest(alone.cpu().numpy(), 5)
    sure = np.abs(pf - np.float32(det.lo)) > 1e-5
    ma, mb = ref.event_mask(ev_alone, len(pf), 1), ref.event_mask(ev_among, len(pf), 1)
    assert np.array_equal(ma[sure], mb[sure]) and 0 < ma.sum() < ma.size


def test_long_life_holds_constant_memory_and_an_always_on_class_is_one_event(sed):
    r, m = _nets(sed, "lightning", seed=9)
    sd = m.state_dict()
    key = [k for k in sd if k.endswith(".bias")][-1]
    sd[key] = sd[key] + 40.0                                          # the class is on in every frame
    m.load_state_dict(sd)
    m = m.cuda().eval()
    st = sed.StreamDetector(m, 2, min_gap=1)
    mel = torch.from_numpy(_features(32 * 50, seed=1)).cuda()
    size = st.state_bytes
    mem = None
    for i in range(2_000):
        a = (i % 50) * 32
        out = st.push_features([mel[a:a + 32], mel[a:a + 32] if i % 2 else None])
        assert len(out) == 0
        # stream 0: N = 32 (i+1); final frames = 4 (i+1) - 8; the run is kept from the first decided frame
        assert st.active()[:1] == ([(0, 0, 0)] if 4 * (i + 1) - 8 > 0 else []), i
        if i == 9:
            del out
            torch.cuda.synchronize()
            mem = torch.cuda.memory_allocated()
    del out
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated() == mem and st.state_bytes == size
    assert st.active() == [(0, 0, 0), (1, 0, 0)]
    out = st.flush()
    assert out.event_offsets == [0, 1, 2] and st.active() == []
    assert out.events["onset"].tolist() == [0, 0] and out.events["offset"].tolist() == [2_000 * 4, 1_000 * 4]
    assert out.final_frames == [8_000, 4_000]
    assert len(out.intervals(1)) == 1 and out.intervals(1)[0][1] == pytest.approx(4_000 * 8 * 1024 / 44_100)


def test_flush_and_reuse(sed):
    r, m = _nets(sed, "lightning", seed=12)
    mels = [_features(N, seed=40 + i) for i, N in enumerate((900, 333, 500))]
    _centre_on_threshold(r, m, mels[0])
    det = sed.EventDetector(m, median=3, min_gap=4)

    def feed(st, upto=None, streams=(0, 1, 2)):
        outs = []
        for a in range(0, 900 if upto is None else upto, 50):
            outs.append(st.push_features([mels[s][a:a + 50] if s in streams and a < len(mels[s]) else None for s in range(3)]))
        return outs
    fresh = det.stream(3, keep_probs=True)
    want_t, want_e = _collect(feed(fresh) + [fresh.flush()], 3)
    st = det.stream(3, keep_probs=True)
    first = feed(st) + [st.flush()]
    assert st.flush().event_offsets == [0, 0, 0, 0]                   # nothing received since: nothing to end
    second = feed(st) + [st.flush()]
    for outs in (first, second):
        t, e = _collect(outs, 3)
        for s in range(3):
            assert torch.equal(t[s], want_t[s])
            _assert_events_equal(e[s], want_e[s], f"reuse {s}")
    # reset(): what the streams held is dropped without an event, and they start again at frame 0
    feed(st, upto=450)
    st.reset(streams=[1])
    assert all(s != 1 for s, _, _ in st.active()) and st.sched.N.tolist() == [450, 0, 450]
    st.reset()
    assert st.active() == [] and not st.sched.N.any()
    t, e = _collect(feed(st) + [st.flush()], 3)
    for s in range(3):
        assert torch.equal(t[s], want_t[s])
        _assert_events_equal(e[s], want_e[s], f"after reset {s}")
    # flush(streams=[2]) in the middle: streams 0 and 1 go on as if stream 2 had simply stopped sending
    def tail(st, outs):
        for a in range(300, 900, 50):
            outs.append(st.push_features([mels[s][a:a + 50] if a < len(mels[s]) else None for s in (0, 1)] + [None]))
        outs.append(st.flush(streams=[0, 1]))
        outs.append(st.flush())
        return _collect(outs, 3)
    st = det.stream(3, keep_probs=True)
    outs = feed(st, upto=300)
    mid = st.flush(streams=[2])
    assert mid.event_offsets[2] == mid.event_offsets[0] == 0 and mid.final_frames[2] == 300 // 8
    t, e = tail(st, outs + [mid])
    quiet = det.stream(3, keep_probs=True)
    t2, e2 = tail(quiet, feed(quiet, upto=300))
    for s in (0, 1):
        assert torch.equal(t[s], t2[s]) and (t[s] - want_t[s]).abs().max().item() <= 2e-6
        _assert_events_equal(e[s], e2[s], f"flush([2]) leaves {s}")
    one = det.from_features(torch.from_numpy(mels[2][:300]).cuda())
    assert (t[2] - one.probs).abs().max().item() <= 2e-6 and (t2[2] - one.probs).abs().max().item() <= 2e-6


def test_refusals_leave_the_device_state_unchanged(sed):
    r, m = _nets(sed, "lightning", seed=13)
    st = sed.StreamDetector(m, 3, keep_probs=True)
    mel = _features(200, seed=2)
    st.push_features([mel, mel[:100], None])
    torch.cuda.synchronize()
    snap = (st._state.clone(), st._feat.clone(), st._pcm.clone(), st.sched.N.tolist())

    def unchanged():
        torch.cuda.synchronize()
        return (torch.equal(st._state, snap[0]) and torch.equal(st._feat, snap[1]) and torch.equal(st._pcm, snap[2]) and
                st.sched.N.tolist() == snap[3])
    with pytest.raises(ValueError, match="expected 3 feature pieces"):
        st.push_features([mel])
    assert unchanged()
    with pytest.raises(ValueError, match="stream 0: expected a mono 1-D waveform"):
        st.push([np.zeros((2, 100), np.float32), None, None])
    assert unchanged()
    with pytest.raises(ValueError, match=r"stream 1: expected features \[N, 40\]"):
        st.push_features([None, np.zeros((4, 39), np.float32), None])
    assert unchanged()
    m.train()
    with pytest.raises(RuntimeError, match="needs model.eval"):
        st.push_features([mel, None, None])
    m.eval()
    assert unchanged()
    st.push_features([None, None, mel[:5]])                            # 5 frames: shorter than one output frame
    snap = (st._state.clone(), st._feat.clone(), st._pcm.clone(), st.sched.N.tolist())
    with pytest.raises(ValueError, match="stream 2: a recording of 5 frames is shorter than one output frame"):
        st.flush()
    assert unchanged()
    _, stereo = _nets(sed, "stereo", seed=1)
    with pytest.raises(ValueError, match="use push_features"):
        sed.StreamDetector(stereo, 1).push([np.zeros(10, np.float32)])
    out = st.flush(streams=[0, 1])                                     # the streams that can end still do
    assert out.final_frames[:2] == [25, 12]


def test_stream_follows_the_bf16_inference_plan(sed):
    r, m = _nets(sed, "timepooled", seed=21)
    mels = [_features(N, seed=60 + i) for i, N in enumerate((3_001, 200, 1_000))]
    _centre_on_threshold(r, m, mels[0])
    det = sed.EventDetector(m, max_batch=64)
    f32 = det.from_features(torch.from_numpy(mels[0]).cuda()).probs
    m.set_inference_precision("bf16")
    try:
        st = det.stream(n_streams=3, keep_probs=True)
        outs = _push_all(st, lambda s: mels[s], [32, 64, 5, 300], st.push_features)
        tracks, evs = _collect(outs, 3)
        assert (tracks[0] - f32).abs().max().item() > 1e-6            # the bf16 plan ran, not the fp32 one
        for s, x in enumerate(mels):
            _check_against_offline(det, tracks[s], evs[s], det.from_features(torch.from_numpy(x).cuda()), f"bf16 stream {s}")
    finally:
        m.set_inference_precision("f32")
