"""Whole-recording detection on the MI355X (sed_crnn_amd/detect.py, csrc/detect.hip) against the numpy / float64 restatement of
tests/detect_ref.py and the CPU oracle nets: the stitch kernel, the event decoder (exact), the whole path end to end, the
waveform front end, chunking invariance, recordings shorter than a window and the bf16 inference plan."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import detect_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def sed():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    import sed_crnn_amd as s
    return s


def _stitch_gpu(sed, logits, plan, combine, trim):
    from sed_crnn_amd._lib import check, lib, ptr, stream_ptr
    lg = torch.from_numpy(logits).cuda()
    out = torch.empty(plan.n_out, logits.shape[2], device="cuda")
    check(lib().sed_detect_stitch(ptr(lg), plan.n_win, plan.win_out, logits.shape[2], plan.hop_out, plan.last_start_out,
                                  plan.n_out, combine, trim, ptr(out), stream_ptr()), "sed_detect_stitch")
    return out.cpu().numpy()


def _decode_gpu(probs, lo=0.5, hi=0.5, median=1, min_gap=0, min_len=1, max_events=None):
    """the decode entry on its own -> (true count, dict of the written events)"""
    from sed_crnn_amd._lib import check, lib, ptr, stream_ptr
    p = torch.from_numpy(np.ascontiguousarray(probs, np.float32)).cuda()
    n, K = p.shape
    cap = n * K // 2 + 2 if max_events is None else max_events
    ws = torch.empty(lib().sed_detect_workspace_bytes(n, K, cap), dtype=torch.uint8, device="cuda")
    keys = ("cls", "onset", "offset", "peak", "peak_frame")
    out = {k: torch.full((max(cap, 1),), -7, dtype=torch.float32 if k == "peak" else torch.int32, device="cuda") for k in keys}
    cnt = torch.zeros(1, dtype=torch.int32, device="cuda")
    check(lib().sed_detect_events(ptr(p), n, K, median, lo, hi, min_gap, min_len, cap, ptr(ws), ws.numel(),
                                  *(ptr(out[k]) for k in keys), ptr(cnt), stream_ptr()), "sed_detect_events")
    c = int(cnt.item())
    return c, {k: v[:min(c, cap)].cpu().numpy() for k, v in out.items()}


def _assert_events_equal(got, want, what=""):
    for k in ("cls", "onset", "offset", "peak_frame"):
        np.testing.assert_array_equal(got[k], want[k], err_msg=f"{what} {k}")
    np.testing.assert_array_equal(got["peak"].view(np.int32), want["peak"].view(np.int32), err_msg=f"{what} peak")


def _check_decode(probs, what="", **kw):
    want = ref.decode(probs, **kw)
    c, got = _decode_gpu(probs, **kw)
    assert c == len(want["cls"]), (what, c, len(want["cls"]))
    _assert_events_equal(got, want, what)
    return c


# ───────────── 1. stitch ─────────────
def test_stitch_matches_float64_and_is_bitwise_repeatable(sed):
    rng = np.random.default_rng(11)
    tf, L = 8, 64
    for K in (1, 3, 6):
        for hop in (L // 4, L // 2, L):
            N = 1003 + 37 * K                                   # not on the grid: the extra end-aligned window
            for trim in (0, 1, 2):
                try:
                    plan = sed.plan_windows(N, tf, L, hop, trim)
                except ValueError:
                    assert hop // tf + 2 * trim > L // tf
                    continue
                logits = (rng.standard_normal((plan.n_win, plan.win_out, K)) * 3).astype(np.float32)
                for combine, name in ((0, "mean"), (1, "max")):
                    got = _stitch_gpu(sed, logits, plan, combine, trim)
                    want = ref.stitch(logits, [s // tf for s in plan.starts], plan.n_out, name, trim)
                    np.testing.assert_allclose(got, want, atol=1e-6, rtol=0, err_msg=f"K={K} hop={hop} trim={trim} {name}")
                    again = _stitch_gpu(sed, logits, plan, combine, trim)
                    assert np.array_equal(got.view(np.int32), again.view(np.int32))


# ───────────── 2. decode: exact against the reference ─────────────
def test_decode_random_and_smooth_tracks(sed):
    rng = np.random.default_rng(5)
    for K in (1, 3):
        p = rng.random((5000, K)).astype(np.float32)
        for kw in (dict(), dict(lo=0.3, hi=0.8), dict(median=5, min_gap=2, min_len=3), dict(lo=0.4, hi=0.6, min_gap=9)):
            assert _check_decode(p, f"random K={K} {kw}", **kw) > 0
    walk = np.cumsum(rng.standard_normal((20000, 4)) * 0.15, 0)
    p = (1 / (1 + np.exp(-np.sin(walk)))).astype(np.float32) * 0.6 + 0.2
    for kw in (dict(), dict(median=9, min_gap=4, min_len=6), dict(lo=0.45, hi=0.62, median=3)):
        assert _check_decode(p, f"smooth {kw}", **kw) > 0


def test_decode_all_off_all_on_and_every_median_width(sed):
    assert _check_decode(np.zeros((10000, 2), np.float32), "off") == 0
    assert _check_decode(np.full((10000, 2), 0.5, np.float32), "at threshold") == 0
    on = np.full((10000, 2), 0.9, np.float32)
    on[1234, 1] = 0.97
    assert _check_decode(on, "on") == 2
    rng = np.random.default_rng(8)
    p = np.repeat(rng.random((600, 2)), 5, 0).astype(np.float32)       # plateaus: ties inside the median windows
    for m in range(1, 32, 2):
        _check_decode(p, f"median {m}", median=m, min_len=2)
    for gap in (0, 1, 3, 17):
        for ml in (1, 2, 5, 40):
            _check_decode(p, f"gap {gap} len {ml}", min_gap=gap, min_len=ml, lo=0.4, hi=0.7)
    _check_decode(rng.random((2000, 32)).astype(np.float32), "K=32", median=3)


def test_decode_runs_across_tile_boundaries_and_one_run_of_466k_frames(sed):
    n = 3 * 4096 + 500
    p = np.full((n, 2), 0.1, np.float32)
    for b in range(64, n, 64):                                  # every word boundary of the bit tracks
        p[b - 3: b + 2, 0] = 0.8
    for b in range(4096, n, 4096):                              # every chunk boundary of the walk
        p[b - 100: b + 100, 1] = 0.7
        p[b, 1] = 0.9
    p[60:4100, 1] = 0.6                                         # a run over the first chunk boundary
    _check_decode(p, "boundaries")
    _check_decode(p, "boundaries, merged", min_gap=60, lo=0.5, hi=0.65)
    n = 466_000
    p = np.full((n, 1), 0.9, np.float32)
    p[300_001, 0] = 0.95
    p[300_002, 0] = 0.95
    c, got = _decode_gpu(p)
    assert c == 1 and got["onset"][0] == 0 and got["offset"][0] == n and got["peak_frame"][0] == 300_001
    assert got["peak"][0] == np.float32(0.95)


def test_decode_24_hours_of_output_frames(sed):
    rng = np.random.default_rng(24)
    n = 466_000                                                 # 24 h at 0.186 s per output frame
    walk = np.cumsum(rng.standard_normal((n, 2)) * 0.08, 0)
    p = (1 / (1 + np.exp(-3 * np.sin(walk)))).astype(np.float32)
    c = _check_decode(p, "24 h", median=5, min_gap=2, min_len=3, lo=0.4, hi=0.7)
    assert c > 100
    print(f"24 h track: {c} events")


def test_decode_max_events_smaller_than_the_count(sed):
    rng = np.random.default_rng(3)
    p = rng.random((4000, 3)).astype(np.float32)
    want = ref.decode(p, median=3)
    total = len(want["cls"])
    assert total > 50
    for cap in (0, 1, 17):
        c, got = _decode_gpu(p, median=3, max_events=cap)
        assert c == total
        _assert_events_equal(got, {k: v[:cap] for k, v in want.items()}, f"cap {cap}")
    det = sed.EventDetector(sed.LightningTimePooledCRNN(dropout=0.0).cuda().eval(), median=3)
    det.max_events = 4
    ev = det.decode(torch.from_numpy(p).cuda())
    assert det.max_events == total
    _assert_events_equal({k: v.cpu().numpy() for k, v in ev.items()}, want, "EventDetector retry")


# ───────────── 3-7. the whole path ─────────────
def _nets(sed, which, seed):
    from oracle import crnn_ref
    if which == "lightning":
        r, m = crnn_ref.LightningNetRef(dropout=0.0), sed.LightningTimePooledCRNN(dropout=0.0)
    elif which == "stereo":                                     # two input channels: feature columns [c*F, (c+1)*F)
        kw = dict(conv_channels=32, dropout=0.0, in_channels=2, gru_hidden=32)
        r, m = crnn_ref.SedNetRef(**kw), sed.TimePooledCRNN(**kw)
    else:
        r, m = crnn_ref.SedNetRef(dropout=0.0, gru_hidden=32), sed.TimePooledCRNN(dropout=0.0, gru_hidden=32)
    sd = crnn_ref.rs_state_dict(r, seed)                       # running statistics away from 0 / 1
    r.load_state_dict(sd)
    m.load_state_dict(sd)
    return r.eval(), m.cuda().eval()


def _centre_on_threshold(r, m, mel, L=64):
    """shift the output bias of both nets so that the median logit over a sample of windows is 0: the track then has frames
    on both sides of 0.5 (only the bias moves; both nets get the same state)"""
    C = mel.shape[1] // 40
    xs = np.stack([mel[s:s + L].reshape(L, C, 40).transpose(1, 2, 0) for s in range(0, min(len(mel) - L, 64 * 40), 64)])
    with torch.no_grad():
        med = float(r(torch.from_numpy(xs)).median())
    sd = r.state_dict()
    key = [k for k in sd if k.endswith(".bias")][-1]            # the last dense layer's bias
    sd[key] = sd[key] - med
    r.load_state_dict(sd)
    m.load_state_dict(sd)


def _features(N, seed, F=40):
    rng = np.random.default_rng(seed)
    t = np.arange(N)[:, None]
    return (rng.standard_normal((N, F)) + 1.5 * np.sin(t / 37.0 + np.arange(F) / 7.0)).astype(np.float32)


def _oracle_probs(r, mel, plan):
    """the reference net on the same windows on the CPU, stitched in numpy float64 (mean, no trim)"""
    C = mel.shape[1] // 40
    xs = np.stack([mel[s:s + plan.win_len].reshape(plan.win_len, C, 40).transpose(1, 2, 0) for s in plan.starts])  # [n_win, C, F, L]
    with torch.no_grad():
        lg = torch.cat([r(torch.from_numpy(xs[i:i + 256])) for i in range(0, len(xs), 256)]).double().numpy()
    return ref.stitch(lg, [s // plan.tf for s in plan.starts], plan.n_out, "mean", 0)


@pytest.mark.parametrize("which", ["lightning", "timepooled", "stereo"])
def test_end_to_end_matches_the_cpu_oracle(sed, which):
    r, m = _nets(sed, which, seed=21)
    mel = _features(10_007, seed=2, F=40 * m.in_channels)
    _centre_on_threshold(r, m, mel)
    det = sed.EventDetector(m)
    res = det.from_features(torch.from_numpy(mel).cuda())
    want = _oracle_probs(r, mel, res.plan)
    got = res.probs.cpu().double().numpy()
    assert got.shape == want.shape == (10_007 // 8, 1)
    err = np.abs(got - want).max()
    print(f"{which}: max |dp| vs oracle {err:.2e}, {len(res)} events")
    assert err < 1e-4
    mask = ref.event_mask({k: v.cpu().numpy() for k, v in res.events.items()}, res.plan.n_out, 1)
    sure = np.abs(want - 0.5) > 1e-3
    assert np.array_equal(mask[sure], (want > 0.5)[sure])
    assert 0 < mask.sum() < mask.size                           # the synthetic track has both states
    iv = res.intervals(0)
    assert len(iv) == len(res) and all(b > a for a, b, _ in iv)
    assert iv[0][0] == pytest.approx(int(res.events["onset"][0]) * 8 * 1024 / 44100)


def test_waveform_equals_features_path_bitwise(sed):
    from sed_crnn_amd import data, feature
    _, m = _nets(sed, "lightning", seed=4)
    rng = np.random.default_rng(9)
    n = 44_100 * 30
    t = np.arange(n) / 44_100
    w = (0.1 * rng.standard_normal(n) + np.sin(2 * np.pi * 800 * t) * (np.sin(2 * np.pi * 0.2 * t) > 0)).astype(np.float32)
    wc = torch.from_numpy(w).cuda()
    mean, std = data.standard_scaler_fit(feature.mbe(wc))
    det = sed.EventDetector(m, mean=mean, std=std, median=3)
    a = det(w)
    b = det.from_features(feature.mbe(wc, mean=mean, std=std))
    assert torch.equal(a.probs, b.probs)
    for k in a.events:
        assert torch.equal(a.events[k], b.events[k]), k
    c = sed.detect_events(m, w, mean=mean.cpu().numpy(), std=std.cpu().numpy(), median=3)
    assert torch.equal(c.probs, a.probs)


def test_chunking_is_bitwise_invariant(sed):
    _, m = _nets(sed, "lightning", seed=5)
    mel = torch.from_numpy(_features(3_001, seed=6)).cuda()
    a = sed.EventDetector(m, max_batch=7, min_gap=1).from_features(mel)
    b = sed.EventDetector(m, max_batch=1024, min_gap=1).from_features(mel)
    assert a.plan.n_win > 7 * 3
    assert torch.equal(a.probs, b.probs)
    for k in a.events:
        assert torch.equal(a.events[k], b.events[k]), k


LONG_N = 20_500           # 639 windows on the hop grid and the end-aligned one: 640
LONG_CHUNKS = (7, 255, 256, 1024)


def test_chunking_is_bitwise_invariant_across_the_gru_batch_tiles(sed):
    """a recording of 640 windows through the Lightning net: max_batch = 1024 runs the GRU's four-row tile (one chunk of 640),
    256 the two-row tile (256, 256) and tile 1 (128), 255 and 7 tile 1 only.  The input projections have K = 640 < 1024, so no
    chunk takes a split-K plan: tracks and events must be bitwise the same whatever the chunking."""
    r, m = _nets(sed, "lightning", seed=5)
    mel_h = _features(LONG_N, seed=6)
    _centre_on_threshold(r, m, mel_h)
    mel = torch.from_numpy(mel_h).cuda()
    res = [sed.EventDetector(m, max_batch=mb, min_gap=1).from_features(mel) for mb in LONG_CHUNKS]
    assert res[0].plan.n_win == 640 and len(res[0]) > 0
    for mb, b in zip(LONG_CHUNKS[1:], res[1:]):
        assert torch.equal(res[0].probs, b.probs), f"max_batch 7 vs {mb}: max |dp| {(res[0].probs - b.probs).abs().max().item():.2e}"
        for k in b.events:
            assert torch.equal(res[0].events[k], b.events[k]), (mb, k)


def test_chunking_of_the_128_channel_net_is_invariant_to_rounding_and_bitwise_between_large_chunks(sed):
    """the 128-channel net's first input projection has K = 5120: a chunk of at most 56 windows (M = 8 rows per window, fewer
    than 96 64x64 output blocks) sums K in up to 21 slices, a larger one in two (csrc/gemm.hip, gemm_plan policy 1), so the
    logits depend on the chunk size by rounding — DESIGN 2 bounds that by 2e-6, asserted here between every two of
    max_batch = 7, 255, 256, 1024.  The recording has 640 windows so that the chunks of 255 (255, 255, 130), of 256 (256, 256,
    128) and of 1024 (640) all have at least 57 windows, the last one included: those three run one GEMM plan and differ in
    the GRU batch tile alone (1; 2 and 1; 2), and their logits, tracks and events must be bitwise equal.  max_batch = 7 ends in
    a chunk of 3 and is held to the 2e-6 only; its events must agree wherever the track is further than 1e-5 from the threshold."""
    from oracle import crnn_ref
    kw = dict(conv_channels=128, dropout=0.0, gru_hidden=128)
    r, m = crnn_ref.SedNetRef(**kw), sed.TimePooledCRNN(**kw)
    sd = crnn_ref.rs_state_dict(r, 5)
    r.load_state_dict(sd)
    m.load_state_dict(sd)
    r.eval()
    m.cuda().eval()
    mel_h = _features(LONG_N, seed=6)
    _centre_on_threshold(r, m, mel_h)
    mel = torch.from_numpy(mel_h).cuda()
    dets = [sed.EventDetector(m, max_batch=mb) for mb in LONG_CHUNKS]
    plan = dets[0]._prepare(mel)[1]
    assert plan.n_win == 640
    for mb in (255, 256, 1024):
        assert min(min(mb, plan.n_win - b0) for b0 in range(0, plan.n_win, mb)) >= 57
    with torch.no_grad():
        logits = [d.window_logits(mel, plan) for d in dets]
    res = [d.from_features(mel) for d in dets]
    worst = 0.0
    for i in range(len(dets)):
        for j in range(i + 1, len(dets)):
            d = (logits[i] - logits[j]).abs().max().item()
            worst = max(worst, d)
            print(f"128-channel net, max_batch {LONG_CHUNKS[i]} vs {LONG_CHUNKS[j]}: max |dlogit| {d:.2e}")
            assert d <= 2e-6, (LONG_CHUNKS[i], LONG_CHUNKS[j], d)
    assert worst > 0, "max_batch = 7 must take the many-slice projection (did the GEMM plan change?)"
    for i in (2, 3):                                            # 256 and 1024 against 255
        assert torch.equal(logits[1], logits[i]), (LONG_CHUNKS[i], (logits[1] - logits[i]).abs().max().item())
        assert torch.equal(res[1].probs, res[i].probs)
        for k in res[1].events:
            assert torch.equal(res[1].events[k], res[i].events[k]), (LONG_CHUNKS[i], k)
    p = res[1].probs.cpu().numpy()
    sure = np.abs(p - np.float32(0.5)) > 1e-5
    masks = [ref.event_mask({k: v.cpu().numpy() for k, v in x.events.items()}, plan.n_out, 1) for x in res]
    assert np.array_equal(masks[0][sure], masks[1][sure]) and 0 < masks[1].sum() < masks[1].size


@pytest.mark.parametrize("N", [8, 15, 50, 63])
def test_short_recordings_run_as_one_sequence(sed, N):
    r, m = _nets(sed, "lightning", seed=7)
    mel = _features(N, seed=N)
    res = sed.EventDetector(m).from_features(mel)
    assert res.plan.n_win == 1 and res.plan.win_len == 8 * (N // 8)
    want = _oracle_probs(r, mel, res.plan)
    assert np.abs(res.probs.cpu().double().numpy() - want).max() < 1e-4


def test_bf16_inference_plan_stays_in_its_band(sed):
    """the detector follows the model's inference precision: under "bf16" the track must MOVE away from the fp32 track (the
    bf16 plan ran, not the fp32 one) and stay inside the band of DESIGN 5e against the oracle"""
    r, m = _nets(sed, "timepooled", seed=21)
    mel = _features(6_000, seed=3)
    det = sed.EventDetector(m, max_batch=64)
    f32 = det.from_features(mel).probs.cpu().double().numpy()
    m.set_inference_precision("bf16")
    try:
        assert "bf16" in m.inference_plan(64, 64)["conv"]
        res = det.from_features(mel)
    finally:
        m.set_inference_precision("f32")
    bf = res.probs.cpu().double().numpy()
    want = _oracle_probs(r, mel, res.plan)
    err, err32, moved = np.abs(bf - want).max(), np.abs(f32 - want).max(), np.abs(bf - f32).max()
    print(f"bf16 plan: max |dp| vs the fp32 oracle {err:.2e} (fp32 plan {err32:.2e}), bf16 vs fp32 track {moved:.2e}")
    assert err32 < 1e-4
    assert moved > 1e-6                                         # bf16 rounding shows (measured ~4e-5); fp32 would give <= 2e-7
    assert err < 5e-4                                            # 2.6e-5 .. 5.5e-5 measured on the forward
