"""Class-wise decoder settings on the MI355X: the three *_classwise entries through EventDetector, decode_many and
StreamDetector against tests/classwise_ref.py, against the scalar kernels they must agree with, and through tune_decoder / score.
Every comparison is exact: integers for events and counts, bit patterns for peaks."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import classwise_ref as cw  # noqa: E402
import detect_ref  # noqa: E402
import tune_ref  # noqa: E402

pytestmark = pytest.mark.gpu
KEYS = cw.EVENT_KEYS


@pytest.fixture(scope="module")
def sed():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    import sed_crnn_amd as s
    return s


_NETS = {}


def _net(sed, K):
    """an untrained Lightning net with K classes: the decoder tests only need its class count"""
    if K not in _NETS:
        _NETS[K] = sed.LightningTimePooledCRNN(dropout=0.0, n_classes=K).cuda().eval()
    return _NETS[K]


def _det(sed, settings, **kw):
    return sed.EventDetector(_net(sed, len(settings)), **cw.det_kwargs(settings), **kw)


def _scalar(sed, K, s, **kw):
    return sed.EventDetector(_net(sed, K), threshold=s["hi"], low=s["lo"], median=s["median"], min_gap=s["min_gap"],
                             min_len=s["min_len"], **kw)


def _np(ev, e0=0, e1=None):
    return {k: ev[k][e0:e1].cpu().numpy() for k in KEYS}


def _same(got, want, what=""):
    for k in ("cls", "onset", "offset", "peak_frame"):
        np.testing.assert_array_equal(got[k], want[k], err_msg=f"{what} {k}")
    np.testing.assert_array_equal(got["peak"].view(np.int32), want["peak"].view(np.int32), err_msg=f"{what} peak")


def _bitwise(a, b, keys, what=""):
    for k in keys:
        assert a[k].dtype == b[k].dtype and torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)), (what, k)


def _features(N, seed, F=40):
    rng = np.random.default_rng(seed)
    t = np.arange(N)[:, None]
    return (rng.standard_normal((N, F)) + 1.5 * np.sin(t / 37.0 + np.arange(F) / 7.0)).astype(np.float32)


def _wide_net(sed, K=6):
    """a net whose track swings through the example's thresholds: the output layer of an untrained net is rescaled per class so
    that, on a sample recording, the logits have median 0 and standard deviation 0.45 (probabilities mostly in 0.35..0.65)"""
    if ("wide", K) in _NETS:
        return _NETS[("wide", K)]
    torch.manual_seed(5)
    m = sed.LightningTimePooledCRNN(dropout=0.0, n_classes=K)
    sd = m.state_dict()
    wkey = [k for k in sd if k.endswith(".weight") and sd[k].dim() == 2 and sd[k].shape[0] == K][-1]
    bkey = wkey[:-len("weight")] + "bias"
    with torch.no_grad():
        sd[wkey] = torch.randn_like(sd[wkey])                            # every class its own direction
        m.load_state_dict(sd)
        p = sed.EventDetector(m.cuda().eval()).from_features(_features(4000, seed=1)).probs.double().cpu()
        z = torch.log(p / (1 - p))
        g = (0.45 / z.std(0)).float()
        sd[bkey] = (sd[bkey].cpu() - z.median(0).values.float()) * g
        sd[wkey] = sd[wkey].cpu() * g[:, None]
    m = sed.LightningTimePooledCRNN(dropout=0.0, n_classes=K)
    m.load_state_dict(sd)
    _NETS[("wide", K)] = m.cuda().eval()
    return _NETS[("wide", K)]


def _track_settings(p):
    """class-wise settings whose thresholds cut THIS track (quantiles of its own columns: test data, not a tolerance), with the
    example's filter widths, gaps and lengths"""
    return [dict(hi=float(np.float32(np.quantile(p[:, k], 0.55))), lo=float(np.float32(np.quantile(p[:, k], 0.45))),
                 median=s["median"], min_gap=s["min_gap"], min_len=s["min_len"]) for k, s in enumerate(cw.EXAMPLE)]


# ───────────── 1. decode against the reference ─────────────
@pytest.mark.parametrize("n_out", [1, 63, 64, 65, 4095, 4097, 8300])
def test_decode_matches_the_reference_with_the_example_settings(sed, n_out):
    det = _det(sed, cw.EXAMPLE)
    assert det.classwise
    for seed in (7, 8):
        p = cw.smooth(np.random.default_rng(seed), n_out, 6)
        if n_out >= 4097:                                                # the example tells the six rows apart on these tracks
            assert cw.example_is_discriminating(p), (seed, n_out)
        want = cw.decode(p, cw.EXAMPLE)
        got = det.decode(torch.from_numpy(p).cuda())
        assert len(got["cls"]) == len(want["cls"]), (seed, n_out)
        _same(_np(got), want, f"seed {seed} n_out {n_out}")


def test_decode_with_one_class_and_with_32_classes_of_every_median_width(sed):
    rng = np.random.default_rng(9)
    p = cw.smooth(rng, 4097, 1)
    for s in (cw.EXAMPLE[1], cw.EXAMPLE[4]):
        want = cw.decode(p, [s])
        assert len(want["cls"]) >= 4
        _same(_np(_det(sed, [s]).decode(torch.from_numpy(p).cuda())), want, f"K=1 {s}")
    # K = 32: every width 1..31 twice, thresholds across the track's range, class 5 never on, class 20 always on
    settings = [dict(hi=0.44 + 0.004 * k, lo=0.44 + 0.004 * k - (0.03 if k % 3 else 0.0), median=1 + 2 * (k % 16), min_gap=k % 5,
                     min_len=1 + k % 3) for k in range(32)]
    assert sorted(s["median"] for s in settings) == sorted(2 * list(range(1, 32, 2)))
    p = cw.smooth(rng, 4200, 32)
    p[:, 5] = 0.1
    p[:, 20] = 0.9
    want = cw.decode(p, settings)
    per = np.bincount(want["cls"], minlength=32)
    assert per[5] == 0 and per[20] == 1 and (np.delete(per, [5, 20]) >= 2).all()
    got = _det(sed, settings).decode(torch.from_numpy(p).cuda())
    _same(_np(got), want, "K=32")
    on = cw.only(_np(got), 20)
    assert (on["onset"][0], on["offset"][0]) == (0, 4200)


# ───────────── 2. K equal rows are the scalar path, bit for bit ─────────────
EQUAL = dict(hi=0.55, lo=0.45, median=7, min_gap=3, min_len=2)


def test_equal_rows_decode_bitwise_like_the_scalar_detector_single_and_batch(sed):
    rng = np.random.default_rng(12)
    scalar, same = _scalar(sed, 6, EQUAL), _det(sed, [EQUAL] * 6)
    assert same.classwise and not scalar.classwise
    for n in (1, 64, 4097):
        p = torch.from_numpy(cw.smooth(rng, n, 6)).cuda()
        a, b = scalar.decode(p), same.decode(p)
        assert len(a["cls"]) == len(b["cls"]) and (n < 4097 or len(a["cls"]) > 20)
        _bitwise(a, b, KEYS, f"single {n}")
    lengths = [1, 64, 130, 4200]
    tracks = [cw.smooth(rng, n, 6) for n in lengths]
    bp = sed.plan_batch([8 * n for n in lengths], 8, 6)
    probs = torch.from_numpy(np.concatenate(tracks)).cuda()
    (a, offs_a), (b, offs_b) = scalar.decode_many(probs, bp), same.decode_many(probs, bp)
    assert offs_a == offs_b and offs_a[-1] > 20
    _bitwise(a, b, ("rec",) + KEYS, "batch")


def _push_both(sts, mels, piece):
    """the same pieces into every StreamDetector of ``sts``, then a flush -> per detector the list of StreamEvents"""
    outs = [[] for _ in sts]
    longest = max(len(x) for x in mels)
    for a in range(0, longest, piece):
        pieces = [x[a:a + piece] if a < len(x) else None for x in mels]
        for o, st in zip(outs, sts):
            o.append(st.push_features(pieces))
    for o, st in zip(outs, sts):
        o.append(st.flush())
    return outs


def test_equal_rows_stream_the_same_events_out_of_the_same_pushes(sed):
    m = _wide_net(sed)
    kw = dict(threshold=0.55, low=0.45, median=7, min_gap=3, min_len=2)
    scalar = sed.EventDetector(m, **kw)
    same = sed.EventDetector(m, **dict(kw, median=[7] * 6))
    assert same.classwise and same.median_max == scalar.median
    mels = [_features(N, seed=20 + i) for i, N in enumerate((2500, 900, 1300))]
    n = 0
    for piece in (32, 416):
        sa, sb = scalar.stream(3, keep_probs=True), same.stream(3, keep_probs=True)
        assert sa._dims == sb._dims and sa.state_bytes == sb.state_bytes
        for i, (a, b) in enumerate(zip(*_push_both([sa, sb], mels, piece))):
            assert a.event_offsets == b.event_offsets and a.final_frames == b.final_frames, (piece, i)
            _bitwise(a.events, b.events, ("stream",) + KEYS, f"piece {piece} push {i}")
            assert torch.equal(a.probs, b.probs)
            n += len(a)
        assert sa.active() == sb.active() == []
    assert n > 40


# ───────────── 3. class k of the class-wise decode is class k of the scalar decode with row k ─────────────
def test_every_class_is_the_scalar_kernels_decode_with_its_own_row(sed):
    p = cw.smooth(np.random.default_rng(8), 8300, 6)
    assert cw.example_is_discriminating(p)
    dp = torch.from_numpy(p).cuda()
    got = _np(_det(sed, cw.EXAMPLE).decode(dp))
    scalar = [_np(_scalar(sed, 6, s).decode(dp)) for s in cw.EXAMPLE]
    for k in range(6):
        mine = cw.only(got, k)
        assert 4 <= len(mine["cls"]) <= 178
        _same(mine, cw.only(scalar[k], k), f"class {k}")
        for j in range(6):                                               # and no other row gives these events
            assert j == k or cw.pairs(cw.only(scalar[j], k)) != cw.pairs(mine), (k, j)


# ───────────── 4. batch ─────────────
def test_decode_many_keeps_recordings_apart_and_grows_its_buffers(sed):
    rng = np.random.default_rng(7)
    lengths = [1, 64, 130, 4200]
    tracks = [cw.smooth(rng, n, 6) for n in lengths]
    assert cw.example_is_discriminating(tracks[3])
    want = [cw.decode(t, cw.EXAMPLE) for t in tracks]
    det = _det(sed, cw.EXAMPLE)

    def run(order, det=det):
        bp = sed.plan_batch([8 * lengths[i] for i in order], 8, 6)
        probs = torch.from_numpy(np.concatenate([tracks[i] for i in order])).cuda()
        ev, offs = det.decode_many(probs, bp)
        for r, i in enumerate(order):
            assert (ev["rec"][offs[r]:offs[r + 1]] == r).all()
            _same(_np(ev, offs[r], offs[r + 1]), want[i], f"order {order} recording {i}")
        return ev, offs

    ev, offs = run([0, 1, 2, 3])
    assert offs[-1] == sum(len(w["cls"]) for w in want) > 100
    for order in ([3, 2, 1, 0], [2, 0, 3, 1]):                           # permuting the recordings permutes the results
        run(order)
    # buffers below the total: the decode runs again with buffers of the true total, like the scalar path
    small = _det(sed, cw.EXAMPLE)
    small.max_events = 3
    ev2, offs2 = run([0, 1, 2, 3], small)
    assert offs2 == offs and small.max_events == offs[-1]
    _bitwise(ev, ev2, ("rec",) + KEYS, "grown")
    scalar = _scalar(sed, 6, cw.EXAMPLE[0])
    scalar.max_events = 3
    probs = torch.from_numpy(np.concatenate(tracks)).cuda()
    _, offs_s = scalar.decode_many(probs, sed.plan_batch([8 * n for n in lengths], 8, 6))
    assert scalar.max_events == offs_s[-1] > 3
    one = _det(sed, cw.EXAMPLE)
    one.max_events = 2
    _same(_np(one.decode(torch.from_numpy(tracks[3]).cuda())), want[3], "single, grown")
    assert one.max_events == len(want[3]["cls"])


# ───────────── 5. streams ─────────────
def _union(evs):
    ev = {k: np.concatenate([e[k] for e in evs]) for k in KEYS}
    order = np.lexsort((ev["onset"], ev["cls"]))
    return {k: v[order] for k, v in ev.items()}


class _FeedRef:
    """classwise_ref's streaming rule for one feed of a StreamDetector fed features: the host arithmetic of which rows are final
    after every STEP (a push is split into steps of ``step_frames`` feature frames), the rule on the kernel's own rows"""

    def __init__(self, st, settings):
        self.tf, self.win_out, self.step_frames = st.det.model.time_factor, st.win_out, st.step_frames
        self.dec = cw.ClasswiseDecodeRef(settings)
        self.N = self.final = 0

    def push(self, n_frames, rows):
        """``n_frames`` new feature frames whose newly final track rows are ``rows`` -> the events of the push"""
        evs, at = [], 0
        for a in range(0, n_frames, self.step_frames):
            self.N += min(self.step_frames, n_frames - a)
            final = max(0, self.N // self.tf - self.win_out)
            evs.append(self.dec.step(rows[at:at + final - self.final]))
            at += final - self.final
            self.final = final
        assert at == len(rows)
        return _union(evs) if evs else cw.no_events()

    def flush(self, rows):
        ev = self.dec.step(rows, end=True)
        self.N = self.final = 0
        return ev


def _bad_step(sed, st):
    """sed_stream_step_classwise on the live state with a bad row for class 2 and an otherwise valid idle table"""
    from sed_crnn_amd._lib import TuneSetting, lib, ptr, stream_ptr
    rows = [TuneSetting(r["median"], r["low"], r["threshold"], r["min_gap"], r["min_len"]) for r in st.det.class_settings()]
    rows[2] = TuneSetting(rows[2].median, 0.6, 0.5, 0, 1)
    tab = (TuneSetting * len(rows))(*rows)
    n_out = st.sched.n_out
    table = np.ascontiguousarray(np.stack([np.zeros(st.S, np.int64), np.zeros(st.S, np.int64), st.sched.n_win, n_out, n_out,
                                           np.zeros(st.S, np.int64), np.full(st.S, st.win_out), np.zeros(st.S, np.int64)], 1))
    ws = torch.empty(lib().sed_stream_step_workspace_bytes(st.S, st.K, 0), dtype=torch.uint8, device="cuda")
    ev = torch.zeros(6, 8, dtype=torch.int32, device="cuda")
    off = torch.zeros(st.S + 1, dtype=torch.int32, device="cuda")
    rc = lib().sed_stream_step_classwise(ptr(st._state), st._state.numel(), *st._dims, st.det._combine_id, st.det.trim,
                                         C.cast(tab, C.c_void_p), None, 0, C.c_void_p(table.ctypes.data), 0, None, 0, 8,
                                         *(ptr(ev[i]) for i in range(6)), ptr(off), ptr(ws), ws.numel(), stream_ptr())
    return rc, lib().sed_last_error_string().decode()


def test_stream_emits_what_the_rule_says_step_by_step_and_the_offline_decode_over_a_life(sed):
    m = _wide_net(sed)
    det = sed.EventDetector(m, **cw.det_kwargs(cw.EXAMPLE))
    S, lengths = 3, (5000, 3001, 1500)
    mels = [_features(N, seed=40 + i) for i, N in enumerate(lengths)]
    offline = [det.from_features(x) for x in mels]
    per_class = np.zeros(6, np.int64)
    st = det.stream(S, keep_probs=True)
    assert st.step_frames == 128                                         # 4 windows per step: pushes of 37 windows are split
    lives = []
    for life, piece in enumerate((32, 128, 37 * 32, max(lengths), 128)):  # 1, 4, 37 windows, all at once; then the feeds reused
        refs = [_FeedRef(st, cw.EXAMPLE) for _ in range(S)]
        got, tracks = [[] for _ in range(S)], [[] for _ in range(S)]
        calls = list(range(0, max(lengths), piece)) + ["flush"]
        for call, a in enumerate(calls):
            flush = a == "flush"
            out = st.flush() if flush else st.push_features([x[a:a + piece] if a < len(x) else None for x in mels])
            for s in range(S):
                rows = out.probs[out.prob_offsets[s]:out.prob_offsets[s + 1]].cpu().numpy()
                e = _np(out.events, out.event_offsets[s], out.event_offsets[s + 1])
                assert (out.events["stream"][out.event_offsets[s]:out.event_offsets[s + 1]] == s).all()
                want = refs[s].flush(rows) if flush else refs[s].push(max(0, min(piece, lengths[s] - a)), rows)
                _same(e, want, f"piece {piece} call {call} feed {s}")
                got[s].append(e)
                tracks[s].append(rows)
            want_active = sorted((s, k, a0) for s in range(S) for k, a0 in refs[s].dec.active())
            assert sorted(st.active()) == want_active, (piece, call)
            if piece == 37 * 32 and call == 1:                           # a refused step leaves the state as it was
                torch.cuda.synchronize()
                snap = st._state.clone()
                rc, msg = _bad_step(sed, st)
                assert rc != 0 and "stream_step_classwise: class 2: need hi >= lo" in msg, msg
                torch.cuda.synchronize()
                assert torch.equal(st._state, snap)
        for s in range(S):
            track = np.concatenate(tracks[s])
            assert track.shape == tuple(offline[s].probs.shape)
            assert np.abs(track - offline[s].probs.cpu().numpy()).max() <= 2e-6
            life_ev = _union(got[s])
            _same(life_ev, cw.decode(track, cw.EXAMPLE), f"piece {piece} feed {s} vs the reference on the streamed track")
            _same(life_ev, _np(det.decode(torch.from_numpy(track).cuda())), f"piece {piece} feed {s} vs the offline class-wise decode")
            if life == 0:
                per_class += np.bincount(life_ev["cls"], minlength=6)
        lives.append([_union(g) for g in got])
    print("stream events per class:", per_class.tolist())
    assert (per_class >= 2).all()                                        # every class, so every row of the table, is exercised
    for s in range(S):                                                   # flushed and reused: the fifth life repeats the second
        _same(lives[4][s], lives[1][s], f"reuse feed {s}")


# ───────────── 6. end to end ─────────────
def test_waveforms_features_and_batches_reach_the_classwise_decoder(sed):
    m = _wide_net(sed)
    mels = [_features(N, seed=60 + i) for i, N in enumerate((3000, 64, 130, 1000))]
    det = sed.EventDetector(m, **cw.det_kwargs(cw.EXAMPLE))
    n = 0
    for x in mels:
        res = det.from_features(x)
        want = cw.decode(res.probs.cpu().numpy(), cw.EXAMPLE)
        _same(_np(res.events), want, "from_features")
        n += len(want["cls"])
    assert n > 20
    many = det.from_features_many(mels)
    for i in range(len(mels)):
        _same(_np(many[i].events), cw.decode(many[i].probs.cpu().numpy(), cw.EXAMPLE), f"from_features_many {i}")
    # one-shot functions: a list for ONE argument is enough to take the class-wise path
    medians = [s["median"] for s in cw.EXAMPLE]
    res = sed.detect_events(m, mels[0], median=medians, min_gap=[s["min_gap"] for s in cw.EXAMPLE])
    rows = [dict(lo=0.5, hi=0.5, median=s["median"], min_gap=s["min_gap"], min_len=1) for s in cw.EXAMPLE]
    want = cw.decode(res.probs.cpu().numpy(), rows)
    assert len(want["cls"]) > 10 and len({s["median"] for s in rows}) > 1
    _same(_np(res.events), want, "detect_events(median=[...])")
    assert cw.pairs(want) != cw.pairs(detect_ref.decode(res.probs.cpu().numpy()))          # not the scalar defaults
    res = sed.detect_events_many(m, mels, threshold=[s["hi"] for s in cw.EXAMPLE], low=[s["lo"] for s in cw.EXAMPLE], median=medians)
    rows = [dict(lo=s["lo"], hi=s["hi"], median=s["median"], min_gap=0, min_len=1) for s in cw.EXAMPLE]
    for i in range(len(mels)):
        _same(_np(res[i].events), cw.decode(res[i].probs.cpu().numpy(), rows), f"detect_events_many {i}")
    # waveforms: the thresholds are taken from the track itself (the log-mel of these clips is not what the net was centred on)
    rng = np.random.default_rng(3)
    samples = [44_100 * 60 + 17, 63 * 1024 + 1000, 300_000]
    t = [np.arange(k) / 44_100 for k in samples]
    waves = [(0.1 * rng.standard_normal(k) + np.sin(2 * np.pi * 800 * tt) * (np.sin(2 * np.pi * 0.3 * tt) > 0)).astype(np.float32)
             for k, tt in zip(samples, t)]
    from sed_crnn_amd import data, feature
    mean, std = data.standard_scaler_fit(feature.mbe(torch.from_numpy(waves[0]).cuda()))
    first = sed.EventDetector(m, mean=mean, std=std)(waves[0])
    settings = _track_settings(first.probs.cpu().numpy())
    det = sed.EventDetector(m, mean=mean, std=std, **cw.det_kwargs(settings))
    res = det(waves[0])
    assert torch.equal(res.probs, first.probs)
    want = cw.decode(res.probs.cpu().numpy(), settings)
    assert len(want["cls"]) > 5
    _same(_np(res.events), want, "det(waveform)")
    many = det.detect_many(waves)
    assert many.n_events > 5
    for i in range(len(waves)):
        _same(_np(many[i].events), cw.decode(many[i].probs.cpu().numpy(), settings), f"detect_many {i}")


# ───────────── 7. tuning ─────────────
def _every_median_grid(sed):
    """the 24 settings of test_gpu_tune: every median width 1..31, lo = hi and lo < hi, several gaps and lengths"""
    sets = []
    for i, m in enumerate(range(1, 32, 2)):
        hi = (0.5, 0.6, 0.7)[i % 3]
        sets.append(dict(threshold=hi, low=(None, 0.3, 0.45)[(i // 2) % 3], median=m, min_gap=(0, 1, 3, 17)[i % 4],
                         min_len=(1, 2, 5)[(i // 3) % 3]))
    for i in range(8):
        sets.append(dict(threshold=0.4 + 0.05 * i, low=0.4 if i % 2 else None, median=(1, 3)[i % 2], min_gap=i % 3, min_len=1 + i % 4))
    return sed.DecoderGrid.from_settings(sets)


REF_ROWS = [dict(lo=0.45, hi=0.55, median=m, min_gap=g, min_len=1) for m, g in ((1, 0), (3, 1), (7, 3), (15, 1), (5, 0), (31, 17))]


def _perturbed_ref(rng, tracks, K):
    """reference events = the decode of a perturbed copy of every track, as in test_gpu_tune (matches, near misses and misses
    all occur), here with another annotator per class, so that the classes want different settings"""
    evs = []
    for t in tracks:
        p = np.roll(t, int(rng.integers(-2, 3)), 0) + rng.standard_normal(t.shape).astype(np.float32) * 0.03
        evs.append(cw.decode(p.astype(np.float32), REF_ROWS))
    return tune_ref.events_to_ref(evs, K)


def test_tune_decoder_per_class_scores_what_the_sweep_promised(sed):
    rng = np.random.default_rng(41)
    K, lengths = 6, (500, 65, 1200, 300)
    tracks = [cw.smooth(rng, n, K) for n in lengths]
    ref_lists = _perturbed_ref(rng, tracks, K)
    out_off = np.concatenate([[0], np.cumsum(lengths)]).tolist()
    probs_np = np.concatenate(tracks)
    probs = torch.from_numpy(probs_np).cuda()
    ref = sed.ReferenceEvents(ref_lists, lengths, K)
    grid = _every_median_grid(sed)
    det = sed.EventDetector(_net(sed, K))
    sc = dict(collar=2, block=5, offset_collar=3, offset_percent=0.2)
    for metric in ("f1_event", "f1_segment", "er_segment"):
        det2, res = sed.tune_decoder(det, (probs, out_off), ref, grid, metric=metric, per_class=True, **sc)
        g, sets, scores = res.best_per_class(metric)
        assert det2.classwise and det2.decoder_settings() == sets and det2.class_settings() == [grid[int(i)] for i in g]
        assert len(set(g.tolist())) > 1                                  # the classes do not all want the same setting
        bp = sed.plan_batch([8 * n for n in lengths], 8, K)
        ev, offs = det2.decode_many(probs, bp)
        table = det2.score((probs, out_off), ref, **sc).table()
        assert table.shape == (1, K, 6) and table.dtype == np.int64
        for k in range(K):
            np.testing.assert_array_equal(table[0, k], res.table()[g[k], k], err_msg=f"{metric} class {k}")
        # ... and those counts are the score of the events the class-wise decode really writes
        ev = {n: v.cpu().numpy() for n, v in ev.items()}
        per_rec = [{n: ev[n][offs[r]:offs[r + 1]] for n in ("cls", "onset", "offset")} for r in range(len(lengths))]
        np.testing.assert_array_equal(table[0], tune_ref.score(per_rec, ref_lists, list(lengths), K, **sc))
        np.testing.assert_array_equal(table[0], cw.score(probs_np, out_off, ref_lists, det2.class_settings(), **sc))
        # per-class tuning cannot lose to the best single setting on the mean class-wise score: it maximises every term of the mean
        tuned = getattr(det2.score((probs, out_off), ref, **sc), metric)()[0][0]
        _, _, best_macro = res.best(metric, average="macro")
        if metric == "er_segment":
            assert tuned.mean() <= best_macro
        else:
            assert tuned.mean() >= best_macro
        np.testing.assert_array_equal(tuned, scores)
