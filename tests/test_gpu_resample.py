"""The resampling front end on the MI355X (sed_crnn_amd/resample.py, csrc/resample.hip): the kernel against the float64
restatement of tests/resample_ref.py, packed batches, sample formats and downmix, absolute indices past 2^31 and 2^33, the
identity, and the detectors (offline, batch, streams) fed at another rate against the same detectors fed the resampled audio."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import resample_ref as ref  # noqa: E402
from test_gpu_detect import _assert_events_equal, _centre_on_threshold, _nets  # noqa: E402
from test_gpu_stream import _collect  # noqa: E402

pytestmark = pytest.mark.gpu
TILE = 1024
RATES = (48000, 16000, 96000, 22050, 88200)


@pytest.fixture(scope="module")
def sed():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    import sed_crnn_amd as s
    return s


def _bits(t):
    return t.cpu().numpy().view(np.int32)


def _lengths(sr):
    """1; half - 1; half; 2 half + 1; the input lengths around one workgroup tile of outputs; three tiles + 7"""
    L, M, half, _ = ref.design(sr)
    return [1, half - 1, half, 2 * half + 1] + sorted({t * M // L + d for t in (TILE - 1, TILE, TILE + 1) for d in (0, 1)}) + \
        [(3 * TILE + 7) * M // L + 1]


def _bound(x32, sr):
    """(float64 reference, 4 x the float32 reference variant's own error against it on the same input)"""
    y64 = ref.resample64(x32, sr)
    return y64, 4.0 * np.abs(ref.resample32(x32, sr).astype(np.float64) - y64).max()


# ───────────── 1. the kernel ─────────────
@pytest.mark.parametrize("sr", RATES)
def test_kernel_matches_the_float64_reference(sed, sr):
    rng = np.random.default_rng(sr)
    L, M, half, _ = ref.design(sr)
    waves = [(0.5 * rng.standard_normal(n)).astype(np.float32) for n in _lengths(sr)]
    worst = 0.0
    for w in waves:
        got = sed.resample(w, sr).cpu().numpy()
        y64, bound = _bound(w, sr)
        err = np.abs(got.astype(np.float64) - y64).max()
        worst = max(worst, err / (bound / 4.0) if bound else 0.0)
        print(f"{sr} Hz, {len(w)} samples -> {len(got)}: max error {err:.3e}, float32 reference error {bound / 4:.3e}")
        assert got.dtype == np.float32 and len(got) == ref.n_out(len(w), L, M) and err <= bound, (sr, len(w), err, bound)
    print(f"{sr} Hz: worst kernel error / float32 reference error = {worst:.2f} (bound 4)")
    assert {TILE - 1, TILE, TILE + 1} & {ref.n_out(len(w), L, M) for w in waves}


def test_packed_batch_is_bitwise_the_single_clip_call(sed):
    rng = np.random.default_rng(1)
    for sr in (48000, 16000):
        waves = [(0.5 * rng.standard_normal(n)).astype(np.float32) for n in (1117, 1, 29, 2 * TILE + 301, 58)]
        buf, clips = sed.resample_many(waves, sr)
        assert all(o % 4 == 0 for o, _ in clips)
        assert any((o + n) % 4 for o, n in clips)                       # clips that do not end on a boundary
        for w, (o, n) in zip(waves, clips):
            assert np.array_equal(_bits(buf[o:o + n]), _bits(sed.resample(w, sr))), (sr, len(w))
        # and the packed buffer is what the log-mel batch takes: clips of 1 .. a few thousand samples
        from sed_crnn_amd import feature
        mel, rows = feature.mbe_packed(buf, clips)
        one, _ = feature.mbe_many(waves, input_sr=sr)
        assert np.array_equal(_bits(mel), _bits(one)) and rows[-1] == mel.shape[0]
        for i, w in enumerate(waves):
            assert np.array_equal(_bits(mel[rows[i]:rows[i + 1]]), _bits(feature.mbe(w, input_sr=sr)))


def _downmix(x):
    """int16 [N, C] -> mono float32 the way the kernel's load does it: every sample times 1/32768 (exact), summed in channel
    order, times the float32 1/C"""
    acc = x[:, 0].astype(np.float32) / np.float32(32768)
    for c in range(1, x.shape[1]):
        acc = acc + x[:, c].astype(np.float32) / np.float32(32768)
    return acc if x.shape[1] == 1 else acc * (np.float32(1) / np.float32(x.shape[1]))


@pytest.mark.parametrize("channels", [1, 2, 3])
def test_int16_and_interleaved_channels(sed, channels):
    from sed_crnn_amd.resample import _device_taps, build_rows, launch
    rng = np.random.default_rng(channels)
    sr = 48000
    for N in (TILE + 77, 2 * TILE + 1):                                   # odd lengths: no multiple of any load width
        x = rng.integers(-32768, 32768, size=(N, channels), dtype=np.int16)
        mono = _downmix(x)
        torch_mono = ((torch.from_numpy(x).float() / 32768).reshape(N, channels).sum(1) * (1.0 / channels)).numpy()
        assert np.abs(mono - torch_mono).max() <= 2.0 ** -23                # the same signal up to the order of a 3-term sum
        want = sed.resample(mono, sr)
        y64, bound = _bound(torch_mono, sr)
        xin = x[:, 0] if channels == 1 else x
        for view in (xin, torch.from_numpy(xin).cuda()):
            got = sed.resample(view, sr, channels=channels)
            err = np.abs(got.cpu().numpy().astype(np.float64) - y64).max()
            print(f"int16 x {channels}, {N} frames: max error {err:.3e}, bound {bound:.3e}")
            assert err <= bound, (channels, N, err, bound)
            assert np.array_equal(_bits(got), _bits(want)), (channels, N)   # guaranteed: the same sums in the same order
        xf = x.astype(np.float32) / np.float32(32768)                     # float32 interleaved: the same values
        got = sed.resample(xf[:, 0] if channels == 1 else xf, sr, channels=channels)
        assert np.array_equal(_bits(got), _bits(want))
        # the same frames from a buffer that starts 2 bytes off a 4-byte boundary (stereo then loads sample by sample)
        taps, L, M, half = _device_taps(sr, 44100, 0)
        flat = torch.from_numpy(np.concatenate([np.zeros(1, np.int16), x.reshape(-1)])).cuda()[1:]
        assert flat.data_ptr() % 4 == 2
        rows, _, n_buf = build_rows([N], None, None, [len(y64)])
        out = torch.empty(n_buf, device="cuda")
        launch(flat, 1, channels, None, taps, L, M, half, rows, out)
        assert np.array_equal(_bits(out[:len(y64)]), _bits(want))
    # int16 / interleaved input at the detector's own rate is converted, not resampled
    got = sed.resample(xin, 44100, channels=channels)
    assert np.array_equal(_bits(got), mono.view(np.int32))


@pytest.mark.parametrize("sr", [48000, 96000])
def test_absolute_indices_past_2_31_and_2_33(sed, sr):
    """a feed that has been running for hours: the launch sees history + fresh samples at a huge absolute base.  A base
    that differs by a multiple of M has the same phase sequence, so the result must be bit for bit the small-base result
    (m*M leaves int32 long before the base does), and that one is checked against the float64 reference"""
    from sed_crnn_amd.resample import ResamplePlan, _device_taps, build_rows, launch
    plan = ResamplePlan(sr)
    L, M, half, CR = plan.L, plan.M, plan.half, plan.carry
    rng = np.random.default_rng(9)
    b, n_in = 3 * M + 7, 2 * TILE * M // L + 333
    hist = (0.5 * rng.standard_normal(CR)).astype(np.float32)
    fresh = (0.5 * rng.standard_normal(n_in)).astype(np.float32)
    m0, m1 = plan.n_final(b), plan.n_final(b + n_in)
    taps, *_ = _device_taps(sr, 44100, 0)
    outs = []
    for d in (0, (2 ** 31 - 1000) // M, (2 ** 33 + 12345) // M, (2 ** 40) // M):
        rows, _, n_buf = build_rows([n_in], [b + d * M], [m0 + d * L], [m1 - m0], [CR], [3], [-1])
        out = torch.full((n_buf,), np.nan, device="cuda")
        h = torch.cat([torch.zeros(3), torch.from_numpy(hist)]).cuda()
        launch(torch.from_numpy(fresh).cuda(), 0, 1, h, taps, L, M, half, rows, out)
        outs.append(out[:m1 - m0])
        assert (m0 + d * L) * M >= 2 ** 31 or d == 0
    for o in outs[1:]:
        assert np.array_equal(_bits(o), _bits(outs[0]))
    whole = np.concatenate([np.zeros(b - CR, np.float32), hist, fresh])
    y64, bound = _bound(whole, sr)
    assert np.abs(outs[0].cpu().numpy().astype(np.float64) - y64[m0:m1]).max() <= bound


def test_identity_rate_passes_through(sed):
    rng = np.random.default_rng(2)
    y = torch.from_numpy((0.5 * rng.standard_normal(5001)).astype(np.float32))
    assert np.array_equal(_bits(sed.resample(y, 44100)), y.numpy().view(np.int32))
    yd = y.cuda()
    assert sed.resample(yd, 44100).data_ptr() == yd.data_ptr()             # no kernel, no copy
    buf, clips = sed.resample_many([y, y[:77]], 44100)
    assert clips == [(0, 5001), (5004, 77)] and np.array_equal(_bits(buf[5004:5081]), y[:77].numpy().view(np.int32))


# ───────────── 2. the detectors ─────────────
def _wave(n, sr, seed):
    rng = np.random.default_rng(seed)
    t = np.arange(n) / sr
    return (0.1 * rng.standard_normal(n) + 0.5 * np.sin(2 * np.pi * 800 * t) * (np.sin(2 * np.pi * 1.3 * t) > 0)).astype(np.float32)


def _int16(w):
    return np.clip(np.round(w * 32768 * 0.5), -32768, 32767).astype(np.int16)


@pytest.fixture(scope="module")
def det1(sed):
    """a detector whose windows all run at batch 1 (max_batch=1): its track is then bit for bit the same however the windows
    are grouped, which is what lets streams and batches be compared with the offline call exactly"""
    from sed_crnn_amd import feature
    r, m = _nets(sed, "lightning", seed=4)
    mel = feature.mbe(sed.resample(_wave(48000 * 3, 48000, 0), 48000)).cpu().numpy()
    mel = np.concatenate([mel] * 2)
    _centre_on_threshold(r, m, mel)
    return sed.EventDetector(m, max_batch=1, median=3)


def _same(a, b, what):
    assert torch.equal(a.probs, b.probs), what
    _assert_events_equal({k: v.cpu().numpy() for k, v in a.events.items()}, {k: v.cpu().numpy() for k, v in b.events.items()}, what)


def test_detector_at_another_rate_equals_the_detector_on_the_resampled_clip(sed, det1):
    w48 = _wave(48000 * 3 + 11, 48000, 1)
    a = det1(w48, sr=48000)
    _same(a, det1(sed.resample(w48, 48000)), "48 kHz")
    assert len(a) > 0 and a.probs.shape[0] == (1 + sed.ResamplePlan(48000).n_out(len(w48)) // 1024) // 8
    w441 = _wave(44100 * 2 + 5, 44100, 2)
    _same(det1(w441, sr=44100), det1(w441), "the detector's own rate")
    st = np.stack([_int16(w48), _int16(w48[::-1].copy())], 1)
    _same(det1(st, sr=48000, channels=2), det1(sed.resample(st, 48000, channels=2)), "stereo int16")
    _same(sed.detect_events(det1.model, w48, input_sr=48000, max_batch=1, median=3), a, "detect_events")
    # a batch of three rates equals the per-clip loop
    waves = [w48, w441, _wave(16000 * 2 + 3, 16000, 3)]
    rates = [48000, 44100, 16000]
    res = det1.detect_many(waves, sr=rates)
    for i, (w, r) in enumerate(zip(waves, rates)):
        _same(res[i], det1(w, sr=r), f"detect_many clip {i}")
    res16 = det1.detect_many([_int16(w48), _int16(waves[2])], sr=[48000, 16000])
    _same(res16[1], det1(_int16(waves[2]), sr=16000), "detect_many int16")


def _feed(st, recs, sizes):
    """push every feed its recording in pieces of the given sizes (cycled, shifted per feed; None while a feed has a gap or
    is done) -> the calls' StreamEvents"""
    S = st.S
    at, outs, call = [0] * S, [], 0
    while any(a < len(r) for a, r in zip(at, recs)):
        takes = [min(len(recs[s]) - at[s], sizes[(call + 2 * s) % len(sizes)]) for s in range(S)]
        outs.append(st.push([recs[s][at[s]:at[s] + t] if t else None for s, t in enumerate(takes)]))
        at = [a + t for a, t in zip(at, takes)]
        call += 1
    return outs


def test_streams_at_another_rate_are_bitwise_the_offline_call(sed, det1):
    M = 160
    sizes = [1, 1, M - 1, 997, 0, 60_000, 1, 0, 4099, M, 12_345]          # 60 000 input samples exceed one step (31 744 outputs)
    recs = [_int16(_wave(n, 48000, 10 + i)) for i, n in enumerate((48000 * 3 + 1, 105_001, 48000 * 2 + 777))]
    st = det1.stream(3, keep_probs=True, max_new_windows=1, input_sr=48000)
    st.keep_pcm = True
    assert st.step_frames == 32 and st.state_bytes > 0
    outs = _feed(st, recs, sizes)
    # feed 1 ends early and starts a second recording while the others wait; then everything ends
    second = _int16(_wave(70_003, 48000, 20))
    early = [st.flush([1])]
    pcm1 = torch.cat(st.pcm_log[1])
    st.pcm_log[1] = []
    later = _feed(st, [recs[0][:0], second, recs[2][:0]], sizes) + [st.flush()]
    tracks, evs = _collect(outs + early, 3)
    tracks2, evs2 = _collect(later, 3)
    n_events = 0
    for s, w in enumerate(recs):
        one = det1(w, sr=48000)
        n_events += len(one)
        track = tracks[s] if s == 1 else torch.cat([tracks[s], tracks2[s]])
        ev = evs[s] if s == 1 else {k: np.concatenate([evs[s][k], evs2[s][k]]) for k in evs[s]}
        assert torch.equal(track, one.probs), s
        _assert_events_equal(ev, {k: v.cpu().numpy() for k, v in one.events.items()}, f"feed {s}")
        pcm = pcm1 if s == 1 else torch.cat(st.pcm_log[s])
        assert np.array_equal(_bits(pcm), _bits(sed.resample(w, 48000))), s
    assert n_events > 0
    one = det1(second, sr=48000)
    assert torch.equal(tracks2[1], one.probs)
    _assert_events_equal(evs2[1], {k: v.cpu().numpy() for k, v in one.events.items()}, "feed 1, second recording")
    assert np.array_equal(_bits(torch.cat(st.pcm_log[1])), _bits(sed.resample(second, 48000)))
    # reset in the middle of a recording, then a fresh one
    st.pcm_log = [[] for _ in range(3)]
    st.push([recs[0][:50_000], None, recs[2][:7]])
    st.reset([0, 2])
    o = _feed(st, [recs[2], recs[2][:0], recs[2][:0]], [33_333, 1, 997]) + [st.flush()]
    t, e = _collect(o, 3)
    one = det1(recs[2], sr=48000)
    assert torch.equal(t[0], one.probs)
    _assert_events_equal(e[0], {k: v.cpu().numpy() for k, v in one.events.items()}, "after reset")


def test_stereo_int16_stream_through_a_second_detector(sed, det1):
    left, right = _int16(_wave(48000 * 2 + 19, 48000, 30)), _int16(_wave(48000 * 2 + 19, 48000, 31))
    rec = np.stack([left, right], 1)
    det2 = det1.with_decoder(median=5)
    st = det2.stream(1, keep_probs=True, input_sr=48000, input_channels=2)
    st.keep_pcm = True
    outs = _feed(st, [rec], [1, 159, 997, 50_000, 0, 3]) + [st.flush()]
    tracks, evs = _collect(outs, 1)
    one = det2(rec, sr=48000, channels=2)
    assert torch.equal(tracks[0], one.probs)
    _assert_events_equal(evs[0], {k: v.cpu().numpy() for k, v in one.events.items()}, "stereo feed")
    assert np.array_equal(_bits(torch.cat(st.pcm_log[0])), _bits(sed.resample(rec, 48000, channels=2)))
    # stereo int16 at the detector's own rate: converted and downmixed only
    st = det2.stream(1, keep_probs=True, input_channels=2)
    rec441 = rec[:44100 + 3]
    outs = _feed(st, [rec441], [1, 4097, 20_000]) + [st.flush()]
    tracks, evs = _collect(outs, 1)
    one = det2(rec441, sr=44100, channels=2)
    assert torch.equal(tracks[0], one.probs)
    _assert_events_equal(evs[0], {k: v.cpu().numpy() for k, v in one.events.items()}, "stereo feed at 44.1 kHz")
