"""Multichannel audio in on the MI355X: the resampler keeping channels, the log-mel kernel writing channel c into
columns [c*F, (c+1)*F), and the detector / batch / live-stream paths of a 2-channel net fed [N, 2] interleaved PCM.  Every
yardstick is the pinned mono path on the de-interleaved channel and every comparison is bit for bit: a channel runs exactly
the arithmetic the mono call runs."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_gpu_detect import _assert_events_equal, _centre_on_threshold, _nets  # noqa: E402
from test_gpu_resample import _feed, _int16, _wave  # noqa: E402
from test_gpu_stream import _collect  # noqa: E402

pytestmark = pytest.mark.gpu
F = 40
LENGTHS = (1, 1023, 1024, 1025, 2049, 5000, 25 * 1024 + 3)      # odd / even frame counts, a half-filled last pair, > 1 workgroup


@pytest.fixture(scope="module")
def sed():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    import sed_crnn_amd as s
    return s


def _bits(t):
    return t.cpu().numpy().view(np.int32)


def _pcm(n, C, dtype, seed):
    rng = np.random.default_rng(seed)
    x = 0.3 * rng.standard_normal((n, C)).astype(np.float32)
    return np.clip(np.round(x * 32768), -32768, 32767).astype(np.int16) if dtype == np.int16 else x


# ───────────── 1. the resampler keeps channels ─────────────
@pytest.mark.parametrize("sr", [48000, 44100])
def test_resampler_keeps_channels(sed, sr):
    for C in (2, 3):
        for dtype in (np.int16, np.float32):
            for n in (1024 + 77, 2 * 1024 + 1):
                x = _pcm(n, C, dtype, seed=n + C)
                got = sed.resample(x, sr, channels=C, keep_channels=True)
                assert got.shape == (C, sed.ResamplePlan(sr).n_out(n)) and got.dtype == torch.float32
                for c in range(C):
                    want = sed.resample(x[:, c].copy(), sr)
                    assert np.array_equal(_bits(got[c]), _bits(want)), (sr, C, dtype, n, c)
                    assert got[c].data_ptr() % 16 == 0


@pytest.mark.parametrize("sr", [48000, 44100])
def test_resampler_keeps_channels_of_a_misaligned_stereo_int16_buffer(sed, sr):
    n = 2 * 1024 + 1
    x = _pcm(n, 2, np.int16, seed=5)
    buf = torch.zeros(2 * n + 1, dtype=torch.int16, device="cuda")
    buf[1:] = torch.from_numpy(x).reshape(-1).cuda()
    view = buf[1:].view(n, 2)
    assert view.data_ptr() % 4 == 2
    got = sed.resample(view, sr, channels=2, keep_channels=True)
    for c in range(2):
        assert np.array_equal(_bits(got[c]), _bits(sed.resample(x[:, c].copy(), sr))), (sr, c)


def test_resample_many_keeps_channels_and_equals_the_single_calls(sed):
    clips = [_pcm(3000, 2, np.int16, 1), _pcm(1024 + 77, 2, np.int16, 2), _pcm(2 * 1024 + 1, 2, np.float32, 3)]
    rates = [48000, 44100, 48000]
    buf, where = sed.resample_many(clips, rates, channels=2, keep_channels=True)
    assert len(where) == 6
    for r, (x, sr) in enumerate(zip(clips, rates)):
        one = sed.resample(x, sr, channels=2, keep_channels=True)
        for c in range(2):
            o, n = where[2 * r + c]
            assert o % 4 == 0 and n == one.shape[1]
            assert np.array_equal(_bits(buf[o:o + n]), _bits(one[c])), (r, c)
            assert np.array_equal(_bits(buf[o:o + n]), _bits(sed.resample(x[:, c].copy(), sr))), (r, c)


def test_one_row_with_history_and_fresh_samples_equals_the_whole_clip(sed):
    import importlib
    rs = importlib.import_module("sed_crnn_amd.resample")              # (the package exports the function under this name)
    N, n0, C = 5000, 3001, 2
    x = _pcm(N, C, np.int16, seed=8)
    whole = sed.resample(x, 48000, channels=C, keep_channels=True)
    plan = rs.plan_for(48000)
    taps, L, M, half = rs._device_taps(48000, 44100, 0)
    CR = plan.carry
    m0, total = plan.n_final(n0), plan.n_out(N)
    assert 0 < m0 < total
    # per channel: the CR mono float32 samples before frame n0 (what a stream's carry holds), then the fresh interleaved frames
    hist = torch.cat([torch.from_numpy(x[n0 - CR:n0, c].astype(np.float32) * np.float32(1.0 / 32768.0)) for c in range(C)]).cuda()
    rows, _, n_outbuf = rs.build_rows([N - n0] * C, [n0] * C, [m0] * C, [total - m0] * C, [CR] * C, [c * CR for c in range(C)])
    rows[:, 0] = 0                                                        # both rows read the same frames
    rows = rs.with_channels(rows, np.arange(C))
    rs.check_rows(rows, N - n0, hist.numel(), n_outbuf, L, M, half, channels=C)
    out = torch.empty(n_outbuf, device="cuda")
    rs.launch(torch.from_numpy(x[n0:]).cuda().reshape(-1), 1, C, hist, taps, L, M, half, rows, out)
    for c in range(C):
        o = int(rows[c, 5])
        assert np.array_equal(_bits(out[o:o + total - m0]), _bits(whole[c, m0:])), c


# ───────────── 2. log-mel into columns ─────────────
@pytest.fixture(scope="module")
def planar4(sed):
    """[max length, 4] float32 at the detector's own rate: channel c of a clip of n samples is x[:n, c]"""
    rng = np.random.default_rng(11)
    t = np.arange(max(LENGTHS))[:, None]
    x = 0.2 * rng.standard_normal((max(LENGTHS), 4)) + 0.4 * np.sin(t * (0.05 + 0.03 * np.arange(4)))
    return torch.from_numpy(x.astype(np.float32)).cuda()


def _scaler(n_mels, seed=3):
    """width 4 * n_mels, every channel's slice different; a C-channel call takes the first C * n_mels entries"""
    rng = np.random.default_rng(seed)
    return torch.from_numpy(rng.standard_normal(4 * n_mels) - 8.0), torch.from_numpy(0.5 + rng.random(4 * n_mels))


def _bank(name):
    """(n_mels, tables or None).  librosa's banks of 40 and of 128 bands both take the two-band plan and 12 waves per workgroup
    (their tables are 38 064 and 37 424 bytes); the third bank (40 overlapping bands of 100 bins: 4 000 non-zeros) is a list plan
    whose table leaves room for 8 waves, which is the double-buffered variant of the kernel"""
    from sed_crnn_amd import feature
    if name != "list-40":
        return int(name.split("-")[1]), None
    rng = np.random.RandomState(7)
    fb = np.zeros((40, 1025), np.float32)
    for m in range(40):
        fb[m, 23 * m: 23 * m + 100] = rng.rand(100).astype(np.float32) + 0.1
    tb = feature.build_tables(feature.hann_periodic(), fb, "cuda")
    assert int(tb[5]) == 0 and tb.numel() * 4 + 12 * 9728 > 160 * 1024 - 1280 >= tb.numel() * 4 + 8 * 9728
    return 40, tb


@pytest.mark.parametrize("pad_mode", ["constant", "reflect"])
@pytest.mark.parametrize("bank", ["slaney-40", "slaney-128", "list-40"])
def test_logmel_writes_every_channel_into_its_columns(sed, planar4, bank, pad_mode):
    from sed_crnn_amd import feature
    n_mels, tables = _bank(bank)
    mean, std = _scaler(n_mels)
    for scaled in (False, True):
        want = {}
        for n in LENGTHS:
            for c in range(4):
                sl = slice(c * n_mels, (c + 1) * n_mels)
                kw = dict(mean=mean[sl], std=std[sl]) if scaled else {}
                want[n, c] = feature.mbe(planar4[:n, c].contiguous(), n_mels=n_mels, pad_mode=pad_mode, tables=tables, **kw)
        for C in (1, 2, 3, 4):
            kw = dict(mean=mean[:C * n_mels], std=std[:C * n_mels]) if scaled else {}
            for n in LENGTHS:
                got = feature.mbe(planar4[:n, :C], n_mels=n_mels, pad_mode=pad_mode, channels=C, keep_channels=True, tables=tables, **kw)
                assert got.shape == (1 + n // 1024, C * n_mels)
                for c in range(C):
                    assert np.array_equal(_bits(got[:, c * n_mels:(c + 1) * n_mels]), _bits(want[n, c])), (scaled, C, n, c)
            if C == 3:                                                    # all lengths in one launch
                many, off = feature.mbe_many([planar4[:n, :C] for n in LENGTHS], n_mels=n_mels, pad_mode=pad_mode, channels=C,
                                             keep_channels=True, tables=tables, **kw)
                assert off == np.concatenate([[0], np.cumsum([1 + n // 1024 for n in LENGTHS])]).tolist()
                for i, n in enumerate(LENGTHS):
                    for c in range(C):
                        assert np.array_equal(_bits(many[off[i]:off[i + 1], c * n_mels:(c + 1) * n_mels]), _bits(want[n, c])), (n, c)


def test_logmel_multi_walks_past_the_first_tile_of_its_persistent_workgroups(sed):
    """two recordings x 4 channels x 1 000 000 samples: 8 x 489 = 3 912 frame pairs against the 256 x 12 = 3 072 of one resident
    launch at 12 waves"""
    from sed_crnn_amd import feature
    g = torch.Generator(device="cuda").manual_seed(4)
    recs = [torch.randn(1_000_000, 4, device="cuda", generator=g) * 0.3 for _ in range(2)]
    mean, std = _scaler(F)
    got, off = feature.mbe_many(recs, channels=4, keep_channels=True, mean=mean, std=std)
    assert off == [0, 977, 1954] and got.shape == (1954, 4 * F)
    for r, x in enumerate(recs):
        for c in range(4):
            want = feature.mbe(x[:, c].contiguous(), mean=mean[c * F:(c + 1) * F], std=std[c * F:(c + 1) * F])
            assert np.array_equal(_bits(got[off[r]:off[r + 1], c * F:(c + 1) * F]), _bits(want)), (r, c)


def test_one_channel_through_logmel_multi_equals_logmel_batch(sed, planar4):
    from sed_crnn_amd import feature
    pcm, clips = feature.pack_clips([planar4[:n, 0] for n in LENGTHS], "cuda")
    mean, std = _scaler(F)
    for kw in ({}, dict(mean=mean[:F], std=std[:F])):
        a, ra = feature.mbe_planar(pcm, clips, 1, **kw)
        b, rb = feature.mbe_packed(pcm, clips, **kw)
        assert ra == rb and np.array_equal(_bits(a), _bits(b))


# ───────────── 3. the detector ─────────────
def _stereo(n, sr, seed):
    return np.stack([_int16(_wave(n, sr, seed)), _int16(_wave(n, sr, seed + 100)[::-1].copy())], 1)


def _loop_features(sed, x, sr, mean=None, std=None):
    """the hand-written loop the new path replaces: per channel resample + mbe with the sliced scaler, joined by columns"""
    from sed_crnn_amd import feature
    cols = []
    for c in range(x.shape[1]):
        kw = {} if mean is None else dict(mean=mean[c * F:(c + 1) * F], std=std[c * F:(c + 1) * F])
        cols.append(feature.mbe(sed.resample(x[:, c].copy(), sr), **kw))
    return torch.cat(cols, 1)


@pytest.fixture(scope="module")
def det2(sed):
    """the stereo net of test_gpu_detect centred on the threshold, a scaler of width 2 * 40 whose channel slices differ, and
    max_batch=1 (every window runs at batch 1: tracks are then bit for bit the same however the windows are grouped)"""
    from sed_crnn_amd import data
    r, m = _nets(sed, "stereo", seed=4)
    x = _stereo(48000 * 3, 48000, 0)
    mean, std = data.standard_scaler_fit(_loop_features(sed, x, 48000))
    assert mean.numel() == 2 * F
    mel = _loop_features(sed, x, 48000, mean, std).cpu().numpy()
    _centre_on_threshold(r, m, np.concatenate([mel] * 2))
    return sed.EventDetector(m, max_batch=1, median=3, mean=mean, std=std), x


def _same(a, b, what):
    assert torch.equal(a.probs, b.probs), what
    _assert_events_equal({k: v.cpu().numpy() for k, v in a.events.items()}, {k: v.cpu().numpy() for k, v in b.events.items()}, what)


def test_detector_takes_stereo_pcm_for_a_two_channel_net(sed, det2):
    det, x = det2
    a = det(x, sr=48000, channels=2)
    _same(a, det.from_features(_loop_features(sed, x, 48000, det.mean, det.std)), "stereo int16 at 48 kHz")
    assert len(a) > 0
    clips = [x, _stereo(44100 * 2 + 5, 44100, 2), _stereo(16000 * 2 + 3, 16000, 3)]
    rates = [48000, 44100, 16000]
    res = det.detect_many(clips, sr=rates, channels=2)
    for i, (w, sr) in enumerate(zip(clips, rates)):
        _same(res[i], det(w, sr=sr, channels=2), f"detect_many clip {i}")
    _same(res[1], det.from_features(_loop_features(sed, clips[1], 44100, det.mean, det.std)), "the detector's own rate")
    one = sed.detect_events(det.model, x, input_sr=48000, channels=2, max_batch=1, median=3, mean=det.mean, std=det.std)
    _same(one, a, "detect_events")
    many = sed.detect_events_many(det.model, clips[:2], input_sr=rates[:2], channels=2, max_batch=1, median=3, mean=det.mean, std=det.std)
    _same(many[1], res[1], "detect_events_many")
    with pytest.raises(ValueError, match="2-channel net.*channels=1"):
        det(x[:, 0].copy(), sr=48000)


# ───────────── 4. live feeds ─────────────
def test_stereo_streams_are_bitwise_the_offline_call(sed, det2):
    det, _ = det2
    sizes = [1, 1, 159, 997, 0, 60_000, 3]
    recs = [_stereo(48000 * 3 + 1, 48000, 10), _stereo(105_001, 48000, 11)]
    st = det.stream(2, keep_probs=True, max_new_windows=1, input_sr=48000)
    assert st.input_channels == 2 and st.C == 2 and st.state_bytes > 0
    st.keep_pcm = True
    outs = _feed(st, recs, sizes)
    # feed 1 ends early and starts a second recording while feed 0 waits; then everything ends
    second = _stereo(70_003, 48000, 20)
    early = [st.flush([1])]
    pcm1 = torch.cat(st.pcm_log[1], 1)
    st.pcm_log[1] = []
    later = _feed(st, [recs[0][:0], second], sizes) + [st.flush()]
    tracks, evs = _collect(outs + early, 2)
    tracks2, evs2 = _collect(later, 2)
    n_events = 0
    for s, w in enumerate(recs):
        one = det(w, sr=48000, channels=2)
        n_events += len(one)
        track = tracks[s] if s == 1 else torch.cat([tracks[s], tracks2[s]])
        ev = evs[s] if s == 1 else {k: np.concatenate([evs[s][k], evs2[s][k]]) for k in evs[s]}
        assert torch.equal(track, one.probs), s
        _assert_events_equal(ev, {k: v.cpu().numpy() for k, v in one.events.items()}, f"feed {s}")
        pcm = pcm1 if s == 1 else torch.cat(st.pcm_log[s], 1)
        assert np.array_equal(_bits(pcm), _bits(sed.resample(w, 48000, channels=2, keep_channels=True))), s
    assert n_events > 0
    one = det(second, sr=48000, channels=2)
    assert torch.equal(tracks2[1], one.probs)
    _assert_events_equal(evs2[1], {k: v.cpu().numpy() for k, v in one.events.items()}, "feed 1, second recording")
    assert np.array_equal(_bits(torch.cat(st.pcm_log[1], 1)), _bits(sed.resample(second, 48000, channels=2, keep_channels=True)))
    # reset in the middle of a recording, then a fresh one
    st.push([recs[0][:50_000], recs[1][:7]])
    st.reset([0, 1])
    o = _feed(st, [recs[1], recs[1][:0]], [33_333, 1, 997]) + [st.flush()]
    t, e = _collect(o, 2)
    one = det(recs[1], sr=48000, channels=2)
    assert torch.equal(t[0], one.probs)
    _assert_events_equal(e[0], {k: v.cpu().numpy() for k, v in one.events.items()}, "after reset")


def test_stereo_stream_at_the_detectors_own_rate_runs_the_copy_filter(sed, det2):
    det, _ = det2
    rec = _stereo(44100 * 2 + 3, 44100, 30)
    st = sed.StreamDetector(det.model, 1, keep_probs=True, max_batch=1, median=3, mean=det.mean, std=det.std)
    assert st.input_channels == 2 and st._rs is not None and st._rs.identity
    st.keep_pcm = True
    outs = _feed(st, [rec], [1, 4097, 20_000]) + [st.flush()]
    tracks, evs = _collect(outs, 1)
    one = det(rec, sr=44100, channels=2)
    assert torch.equal(tracks[0], one.probs)
    _assert_events_equal(evs[0], {k: v.cpu().numpy() for k, v in one.events.items()}, "stereo feed at 44.1 kHz")
    assert np.array_equal(_bits(torch.cat(st.pcm_log[0], 1)), _bits(sed.resample(rec, 44100, channels=2, keep_channels=True)))
