"""PCEN on the MI355X: sed_pcen against the float64 definition (tests/pcen_ref.py: scipy.signal.lfilter as librosa
composes it), chunking / batching / untouched columns / restarts bit for bit, digital silence, and the package paths — feature.mbe
with ``compress``, the detector, the batch and live streams.

Bound of the float64 comparison: ALLOWED x the error of the same definition evaluated in float32 numpy on the same input (the
yardstick), both taken as the largest absolute difference from float64 over the case's output.

Measured on an MI355X over the 126 cases of test_pcen_matches_the_float64_definition and the ragged batch: yardstick error
8.1e-8 .. 2.9e-5, kernel error 1.1e-7 .. 2.4e-5, 0.47 .. 2.46 times the yardstick's (worst per width: 1.86 at W = 40, 2.46 at W = 7, 1.59 at W = 160); no
yardstick was exact.  ALLOWED = 5 is about twice the worst ratio."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pcen_ref  # noqa: E402
from test_gpu_detect import _assert_events_equal, _centre_on_threshold, _nets  # noqa: E402
from test_gpu_resample import _feed, _wave  # noqa: E402
from test_gpu_stream import _collect  # noqa: E402

pytestmark = pytest.mark.gpu
F = 40
ALLOWED = 5.0                                       # x the float32 yardstick's own error (module docstring)


@pytest.fixture(scope="module")
def sed():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    import sed_crnn_amd as s
    return s


def _L():
    from sed_crnn_amd import feature
    return feature.PCEN_BLOCK


def _bits(t):
    return t.cpu().numpy().view(np.int32)


def _settings(sed):
    """the defaults; gain = 1 and power = 1 with a short time constant and a large eps; the defaults on int32-scaled energies"""
    return [sed.PCEN(), sed.PCEN(gain=1.0, bias=1.0, power=1.0, time_constant=0.06, eps=1e-3), sed.PCEN(scale=2.0 ** 31)]


def _kw(p, sr=44100, hop=1024):
    return dict(b=p.smoothing(sr, hop), gain=p.gain, bias=p.bias, power=p.power, eps=p.eps, scale=p.scale)


def _logmel_like(T, W, seed):
    """[T, W] float32 log-mel-like values around -6 +- 2 with a slow swell; from 3 blocks up, a 60 dB step up at a third and down
    again at two thirds and a stretch of -inf (digital silence) in the middle; from 2 rows up, column 0 STARTS silent and
    column 1 has one silent frame"""
    L = _L()
    rng = np.random.default_rng(seed)
    t, c = np.arange(T)[:, None], np.arange(W)[None, :]
    x = -6.0 + 2.0 * rng.standard_normal((T, W)) + 1.5 * np.sin(t / 23.0 + c / 5.0)
    if T >= 3 * L:
        x[T // 3:2 * T // 3] += np.log(1e6)
        x[T // 2:T // 2 + L // 2 + 3] = -np.inf
    if T >= 2:
        x[0, 0] = -np.inf
        x[1, 1 % W] = -np.inf
    return x.astype(np.float32)


def _scaler(W, seed=3):
    rng = np.random.default_rng(seed)
    return torch.from_numpy(0.3 + 0.2 * rng.standard_normal(W)), torch.from_numpy(0.1 + 0.5 * rng.random(W))


_REF = {}


def _reference(T, W, si, p):
    """(input, float64 reference, float32 yardstick) of a case: computed once, shared, never modified"""
    key = (T, W, si)
    if key not in _REF:
        x = _logmel_like(T, W, seed=1000 * si + 7 * T + W)
        want, yard = pcen_ref.pcen(x, **_kw(p)), pcen_ref.pcen_f32(x, **_kw(p))
        for a in (x, want, yard):
            a.setflags(write=False)
        _REF[key] = (x, want, yard)
    return _REF[key]


def _compare(got, want, yard, mean, std, what):
    """kernel and yardstick against float64, with the scaler applied to both sides where given; -> the ratio.  A yardstick that
    is EXACT (error 0: e.g. a one-row case, where M[0] = E[0] needs no arithmetic) is replaced by 2^-24 of the largest value,
    half an ulp of what a float32 result is rounded to"""
    g = got.cpu().numpy().astype(np.float64)
    w, y = want, yard.astype(np.float64)
    if mean is not None:
        mu64, is64 = mean.numpy(), 1.0 / std.numpy()
        mu32, is32 = mu64.astype(np.float32), is64.astype(np.float32)
        w, y = (want - mu64) * is64, ((yard - mu32) * is32).astype(np.float64)
    assert g.shape == w.shape and np.isfinite(g).all(), what
    e_yard, e_kernel = np.abs(y - w).max(), np.abs(g - w).max()
    exact = e_yard == 0.0
    if exact:
        e_yard = 2.0 ** -24 * np.abs(w).max()
    ratio = e_kernel / e_yard if e_yard > 0 else (0.0 if e_kernel == 0 else np.inf)
    print(f"{what}: yardstick {e_yard:.2e}{' (exact: replaced)' if exact else ''}  kernel {e_kernel:.2e}  ratio {ratio:.2f}")
    assert e_kernel <= ALLOWED * e_yard, (what, e_kernel, e_yard)
    return ratio


# ───────────── 1. against float64 ─────────────
@pytest.mark.parametrize("W", [40, 7, 160])
def test_pcen_matches_the_float64_definition(sed, W):
    """rows per recording 1, 2, L-1, L, L+1, 3L+5 and 40L+17 (block ends, the first carry, many carries), three settings, with
    and without a scaler; the input has a 60 dB step, a silent stretch, a silent start and a single silent frame"""
    from sed_crnn_amd import feature
    L = _L()
    mean, std = _scaler(W)
    worst = 0.0
    for si, p in enumerate(_settings(sed)):
        for T in (1, 2, L - 1, L, L + 1, 3 * L + 5, 40 * L + 17):
            x, want, yard = _reference(T, W, si, p)
            xd = torch.tensor(x, device="cuda")
            for scaled in (False, True):
                kw = dict(mean=mean, std=std) if scaled else {}
                got = feature.pcen(xd, p, **kw)
                worst = max(worst, _compare(got, want, yard, mean if scaled else None, std, f"W={W} setting {si} T={T} scaled={scaled}"))
            assert np.array_equal(_bits(xd), x.view(np.int32))               # feature.pcen returns a new tensor
    print(f"W={W}: worst kernel / yardstick ratio {worst:.2f}")


def test_a_ragged_batch_matches_the_float64_definition(sed):
    """five recordings in one call, one of them a single row, one empty: every recording starts its own smoother"""
    from sed_crnn_amd import feature
    L, W = _L(), 40
    p = sed.PCEN()
    lens = [L + 3, 1, 3 * L + 5, 0, 2, 2 * L]
    parts = [_reference(T, W, 0, p) for T in lens if T]
    x = np.concatenate([q[0] for q in parts])
    want, yard = np.concatenate([q[1] for q in parts]), np.concatenate([q[2] for q in parts])
    off = np.concatenate([[0], np.cumsum(lens)]).tolist()
    mean, std = _scaler(W)
    for scaled in (False, True):
        got = feature.pcen(torch.tensor(x, device="cuda"), p, rows=off, **(dict(mean=mean, std=std) if scaled else {}))
        _compare(got, want, yard, mean if scaled else None, std, f"ragged batch scaled={scaled}")


# ───────────── 2. bit for bit ─────────────
def test_pieces_with_the_state_carried_equal_one_call(sed):
    from sed_crnn_amd import feature
    L, W = _L(), 40
    T = 8 * L + 11
    mean, std = _scaler(W)
    for si, p in enumerate(_settings(sed)):
        x = torch.from_numpy(_logmel_like(T, W, seed=50 + si)).cuda()
        whole = feature.pcen(x, p, mean=mean, std=std)
        pieces = [1, L - 1, 1, L, L + 1, 2 * L - 3]
        pieces.append(T - sum(pieces))
        assert pieces[-1] > L
        state = torch.full((1, W, 2), float("nan"), device="cuda")          # never read before it is written: frame 0 ignores it
        at, out = 0, []
        for n in pieces:
            out.append(feature.pcen(x[at:at + n], p, mean=mean, std=std, state=state, start=[at]))
            at += n
        assert np.array_equal(_bits(torch.cat(out)), _bits(whole)), si
        assert torch.isfinite(state).all()
        # another chunking, every piece off the block grid, ends in the same state
        state2 = torch.zeros(1, W, 2, device="cuda")
        at, out2 = 0, []
        for n in [L + 7] * (T // (L + 7)) + [T % (L + 7)]:
            out2.append(feature.pcen(x[at:at + n], p, mean=mean, std=std, state=state2, start=[at]))
            at += n
        assert np.array_equal(_bits(torch.cat(out2)), _bits(whole)) and np.array_equal(_bits(state2), _bits(state)), si


def test_a_batch_equals_the_per_recording_calls(sed):
    from sed_crnn_amd import feature
    L = _L()
    p = sed.PCEN(gain=0.8, time_constant=0.2)
    for W in (40, 7, 160):
        lens = [L + 3, 1, 3 * L + 5, 0, 2, 5 * L]
        off = np.concatenate([[0], np.cumsum(lens)]).tolist()
        x = torch.from_numpy(_logmel_like(off[-1], W, seed=W)).cuda()
        mean, std = _scaler(W)
        many = feature.pcen(x, p, rows=off, mean=mean, std=std)
        for i, n in enumerate(lens):
            one = feature.pcen(x[off[i]:off[i + 1]], p, mean=mean, std=std)
            assert np.array_equal(_bits(many[off[i]:off[i + 1]]), _bits(one)), (W, i)
        # pieces of a batch: recordings advance by different amounts per call, some by nothing
        state = torch.zeros(len(lens), W, 2, device="cuda")
        done, got = [0] * len(lens), [[] for _ in lens]
        rng = np.random.default_rng(W)
        while any(d < n for d, n in zip(done, lens)):
            take = [min(n - d, int(rng.integers(0, L + 9))) for d, n in zip(done, lens)]
            rows = torch.cat([x[off[i] + done[i]:off[i] + done[i] + t] for i, t in enumerate(take)])
            o = np.concatenate([[0], np.cumsum(take)]).tolist()
            y = feature.pcen(rows, p, rows=o, mean=mean, std=std, state=state, start=done)
            for i in range(len(lens)):
                got[i].append(y[o[i]:o[i + 1]])
            done = [d + t for d, t in zip(done, take)]
        assert np.array_equal(_bits(torch.cat([torch.cat(g) for g in got])), _bits(many)), W


def test_columns_outside_the_range_keep_their_bits(sed):
    from sed_crnn_amd import feature
    L = _L()
    x = torch.from_numpy(_logmel_like(2 * L + 9, 100, seed=8)).cuda()
    x[3, 0], x[5, 99] = float("nan"), float("-inf")                          # any bit pattern outside the range survives
    p = sed.PCEN()
    mean, std = _scaler(40)
    got = feature.pcen(x, p, columns=(30, 40), mean=mean, std=std)
    assert np.array_equal(_bits(got[:, :30]), _bits(x[:, :30])) and np.array_equal(_bits(got[:, 70:]), _bits(x[:, 70:]))
    assert np.array_equal(_bits(got[:, 30:70]), _bits(feature.pcen(x[:, 30:70].contiguous(), p, mean=mean, std=std)))


def test_a_restart_at_frame_zero_ignores_the_old_state(sed):
    from sed_crnn_amd import feature
    L, W = _L(), 40
    p = sed.PCEN()
    a = torch.from_numpy(_logmel_like(2 * L + 5, W, seed=1)).cuda()
    b = torch.from_numpy(_logmel_like(L + 9, W, seed=2)).cuda()
    used, fresh = torch.zeros(1, W, 2, device="cuda"), torch.zeros(1, W, 2, device="cuda")
    feature.pcen(a, p, state=used, start=[0])
    assert used.abs().sum() > 0
    y_used = feature.pcen(b, p, state=used, start=[0])                       # the feed restarts: no reset call in between
    y_fresh = feature.pcen(b, p, state=fresh, start=[0])
    assert np.array_equal(_bits(y_used), _bits(y_fresh)) and np.array_equal(_bits(used), _bits(fresh))
    assert np.array_equal(_bits(y_used), _bits(feature.pcen(b, p)))           # and without a state buffer


# ───────────── 3. silence ─────────────
def test_an_all_zero_clip_gives_the_scaled_zero(sed):
    from sed_crnn_amd import feature
    mean, std = _scaler(F)
    for p in _settings(sed) + [sed.PCEN(gain=12.0)]:                         # gain 12: eps^-gain overflows float32
        got = feature.mbe(torch.zeros(70_000, device="cuda"), compress=p, mean=mean, std=std).cpu()
        assert got.shape == (69, F) and torch.isfinite(got).all()
        m32, i32 = feature._scaler(mean, std, "cpu")
        assert np.array_equal(_bits(got), _bits(((0.0 - m32) * i32).expand(69, F).contiguous()))
        assert not feature.mbe(torch.zeros(70_000, device="cuda"), compress=p).any()


# ───────────── 4. through the package ─────────────
def _stereo(n, seed):
    return np.stack([_wave(n, 44100, seed), _wave(n, 44100, seed + 100)], 1)


def test_mbe_with_compress_is_the_kernel_on_the_log_mel(sed):
    from sed_crnn_amd import feature
    p = sed.PCEN(gain=0.9)
    y = torch.from_numpy(_wave(44100 * 2 + 321, 44100, 3)).cuda()
    mean, std = _scaler(F)
    assert np.array_equal(_bits(feature.mbe(y, compress=p)), _bits(feature.pcen(feature.mbe(y), p)))
    assert np.array_equal(_bits(feature.mbe(y, compress=p, mean=mean, std=std)), _bits(feature.pcen(feature.mbe(y), p, mean=mean, std=std)))
    assert np.array_equal(_bits(feature.mbe(y, hop=441, compress=p)), _bits(feature.pcen(feature.mbe(y, hop=441), p, hop=441)))
    # keep_channels, C = 2: each of the 2 * 40 mel columns is its own chain
    y2 = torch.from_numpy(_stereo(44100 + 77, 4)).cuda()
    mean2, std2 = _scaler(2 * F)
    kw = dict(channels=2, keep_channels=True)
    assert np.array_equal(_bits(feature.mbe(y2, compress=p, mean=mean2, std=std2, **kw)),
                          _bits(feature.pcen(feature.mbe(y2, **kw), p, mean=mean2, std=std2)))
    one = feature.mbe(y2[:, 1].contiguous(), compress=p, mean=mean2[F:], std=std2[F:])
    assert np.array_equal(_bits(feature.mbe(y2, compress=p, mean=mean2, std=std2, **kw)[:, F:]), _bits(one))
    # spatial: the GCC columns are what they are without compress, scaled by their own entries
    mean3, std3 = _scaler(3 * F)
    kw = dict(channels=2, keep_channels=True, spatial="gcc_phat")
    for scaled in (False, True):
        sc = dict(mean=mean3, std=std3) if scaled else {}
        sc_mel = dict(mean=mean3[:2 * F], std=std3[:2 * F]) if scaled else {}
        got, plain = feature.mbe(y2, compress=p, **kw, **sc), feature.mbe(y2, **kw, **sc)
        assert np.array_equal(_bits(got[:, 2 * F:]), _bits(plain[:, 2 * F:])), scaled
        assert np.array_equal(_bits(got), _bits(feature.pcen(feature.mbe(y2, **kw, **(dict(
            mean=torch.cat([torch.zeros(2 * F, dtype=torch.float64), mean3[2 * F:]]),
            std=torch.cat([torch.ones(2 * F, dtype=torch.float64), std3[2 * F:]])) if scaled else {})), p, columns=(0, 2 * F), **sc_mel))), scaled
    # a batch is the per-clip calls
    waves = [torch.from_numpy(_wave(n, 44100, 9 + n % 7)).cuda() for n in (30_000, 1, 70_001, 1500)]
    many, off = feature.mbe_many(waves, compress=p, mean=mean, std=std)
    for i, w in enumerate(waves):
        assert np.array_equal(_bits(many[off[i]:off[i + 1]]), _bits(feature.mbe(w, compress=p, mean=mean, std=std))), i
    assert np.array_equal(_bits(many), _bits(feature.pcen(feature.mbe_many(waves)[0], p, rows=off, mean=mean, std=std)))


@pytest.fixture(scope="module")
def detp(sed):
    """the Lightning net centred on the threshold on PCEN features, a scaler fitted on such features, max_batch=1 (tracks are
    then bit for bit the same however the windows are grouped)"""
    from sed_crnn_amd import data, feature
    p = sed.PCEN()
    r, m = _nets(sed, "lightning", seed=4)
    w = _wave(44100 * 3, 44100, 0)
    raw = feature.mbe(torch.from_numpy(w).cuda(), compress=p)
    mean, std = data.standard_scaler_fit(raw)
    mel = feature.mbe(torch.from_numpy(w).cuda(), compress=p, mean=mean, std=std)
    _centre_on_threshold(r, m, np.concatenate([mel.cpu().numpy()] * 2))
    return sed.EventDetector(m, max_batch=1, median=3, mean=mean, std=std, compress=p), p


def _same(a, b, what):
    assert torch.equal(a.probs, b.probs), what
    _assert_events_equal({k: v.cpu().numpy() for k, v in a.events.items()}, {k: v.cpu().numpy() for k, v in b.events.items()}, what)


def test_detector_with_compress_equals_the_detector_on_its_features(sed, detp):
    from sed_crnn_amd import feature
    det, p = detp
    w = _wave(44100 * 3 + 11, 44100, 1)
    a = det(w)
    mel = feature.mbe(torch.from_numpy(w).cuda(), compress=p, mean=det.mean, std=det.std)
    _same(a, det.from_features(mel), "det(wave)")
    assert len(a) > 0
    plain = sed.EventDetector(det.model, max_batch=1, median=3, mean=det.mean, std=det.std)
    assert not torch.equal(plain(w).probs, a.probs)                           # the switch does something
    _same(det.with_decoder(median=3)(w), a, "with_decoder keeps compress")
    _same(sed.detect_events(det.model, w, max_batch=1, median=3, mean=det.mean, std=det.std, compress=p), a, "detect_events")
    # another rate goes through the resampler first
    w48 = _wave(48000 * 2 + 5, 48000, 2)
    _same(det(w48, sr=48000), det(sed.resample(w48, 48000)), "48 kHz")


def test_detect_many_with_compress_equals_the_loop(sed, detp):
    det, p = detp
    clips = [_wave(n, 44100, 20 + i) for i, n in enumerate((44100 * 2 + 5, 70_001, 44100 * 3, 66_000))]
    res = det.detect_many(clips)
    n = 0
    for i, w in enumerate(clips):
        _same(res[i], det(w), f"detect_many clip {i}")
        n += len(res[i])
    assert n > 0
    many = sed.detect_events_many(det.model, clips, max_batch=1, median=3, mean=det.mean, std=det.std, compress=p)
    for i in range(len(clips)):
        _same(many[i], res[i], f"detect_events_many clip {i}")


def test_streams_with_compress_are_bitwise_the_offline_call(sed, detp):
    """two feeds pushed in seeded random pieces (some empty, some longer than one step), flushed, then pushed again: the
    smoother's state is carried on the device from push to push and starts afresh after the flush without a reset"""
    det, p = detp
    rng = np.random.default_rng(5)
    st = det.stream(2, keep_probs=True, max_new_windows=1)
    plain_bytes = sed.EventDetector(det.model, max_batch=1, median=3).stream(2, keep_probs=True, max_new_windows=1).state_bytes
    assert st.state_bytes == plain_bytes + 2 * F * 2 * 4
    n_events = 0
    for phase in range(2):
        recs = [_wave(n, 44100, 30 + 2 * phase + i) for i, n in enumerate((44100 * 3 + 1, 100_001))]
        sizes = [int(v) for v in rng.integers(0, 40_000, size=9)] + [1, 0, 1023]
        outs = _feed(st, recs, sizes) + [st.flush()]
        tracks, evs = _collect(outs, 2)
        for s, w in enumerate(recs):
            one = det(w)
            n_events += len(one)
            assert torch.equal(tracks[s], one.probs), (phase, s)
            _assert_events_equal(evs[s], {k: v.cpu().numpy() for k, v in one.events.items()}, f"phase {phase} feed {s}")
    assert n_events > 0
    # finished features go in as they are: push_features applies nothing
    from sed_crnn_amd import feature
    w = _wave(44100 * 2, 44100, 40)
    mel = feature.mbe(torch.from_numpy(w).cuda(), compress=p, mean=det.mean, std=det.std)
    st2 = det.stream(1, keep_probs=True)
    outs = [st2.push_features([mel[:50]]), st2.push_features([mel[50:]]), st2.flush()]
    tracks, _ = _collect(outs, 1)
    assert torch.equal(tracks[0], det(w).probs)


def test_spatial_streams_with_compress_are_bitwise_the_offline_call(sed):
    """a 3-input-channel net fed stereo int16 at 48 kHz with spatial="gcc_phat" and compress: per feed 2 * 40 PCEN chains, the
    GCC columns scaled by their own entries in the GCC launch (identity on the mel columns), the mel columns in the PCEN call"""
    from oracle import crnn_ref
    from sed_crnn_amd import data, feature
    from test_gpu_spatial import _stereo16
    p = sed.PCEN()
    r, m = crnn_ref.LightningNetRef(dropout=0.0, in_channels=3), sed.LightningTimePooledCRNN(dropout=0.0, in_channels=3)
    sd = crnn_ref.rs_state_dict(r, 4)
    r.load_state_dict(sd)
    m.load_state_dict(sd)
    r, m = r.eval(), m.cuda().eval()
    kw = dict(input_sr=48000, channels=2, keep_channels=True, spatial="gcc_phat", device="cuda", compress=p)
    x = _stereo16(48000 * 3, 0)
    mean, std = data.standard_scaler_fit(feature.mbe(x, **kw))
    assert mean.numel() == 3 * F
    _centre_on_threshold(r, m, np.concatenate([feature.mbe(x, mean=mean, std=std, **kw).cpu().numpy()] * 2))
    det = sed.EventDetector(m, max_batch=1, median=3, mean=mean, std=std, spatial="gcc_phat", compress=p)
    _same(det(x, sr=48000, channels=2), det.from_features(feature.mbe(x, mean=mean, std=std, **kw)), "spatial det(wave)")
    recs = [_stereo16(48000 * 3 + 1, 10), _stereo16(105_001, 11)]
    st = det.stream(2, keep_probs=True, max_new_windows=1, input_sr=48000)
    assert st.PW == 2 * F and st.CF == 3 * F
    outs = _feed(st, recs, [1, 1, 159, 997, 0, 60_000, 3]) + [st.flush()]
    tracks, evs = _collect(outs, 2)
    n_events = 0
    for s, w in enumerate(recs):
        one = det(w, sr=48000, channels=2)
        n_events += len(one)
        assert torch.equal(tracks[s], one.probs), s
        _assert_events_equal(evs[s], {k: v.cpu().numpy() for k, v in one.events.items()}, f"feed {s}")
    assert n_events > 0
