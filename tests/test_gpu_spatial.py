"""GCC-PHAT spatial features on the MI355X: sed_logmel_gcc against the float64 definition (tests/spatial_ref.py),
digital silence, the mel columns and the batch bit for bit, the detector / batch / live-stream paths of a 3-input-channel net fed
stereo PCM, and nets with 3 and 10 input channels against the CPU oracle.

Measured on an MI355X over the 144 cases of test_gcc_columns_match_the_float64_definition: kernel error 1.5e-8 .. 1.4e-7 with
constant padding (yardstick as measured 1.7e-8 .. 1.1e-7), up to 7.3e-6 with reflect padding (yardstick 2.2e-5 there); worst
kernel / measured yardstick ratio 3.6 of the 8 allowed; the yardstick was degenerate (1e-16, replaced) only for the one-sample
clip at C = 2.  C = 6 and 8: ratios 0.6 .. 1.7."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import spatial_ref  # noqa: E402
from test_gpu_detect import _assert_events_equal, _centre_on_threshold  # noqa: E402
from test_gpu_resample import _feed  # noqa: E402
from test_gpu_stream import _collect  # noqa: E402

pytestmark = pytest.mark.gpu
F = 40                                              # n_mels = n_lags
LENGTHS = (1, 700, 2047, 2048, 5000, 9000)          # one frame; < n_fft/2; around n_fft; odd frame counts; several frames
DELAYS = (0, 7, -3, 12, 5, -9, 2, 15)               # channel c = the common source delayed by DELAYS[c] samples, plus its own noise
DEGENERATE = 1e-9                                   # a float32 yardstick below this is exact arithmetic, not float32 rounding


@pytest.fixture(scope="module")
def sed():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    import sed_crnn_amd as s
    return s


def _bits(t):
    return t.cpu().numpy().view(np.int32)


def _broadband(n, C, seed):
    """[n, C] float32: a white source that reaches channel c with delay DELAYS[c], plus independent white noise per channel —
    every bin of every channel carries energy, so PHAT's division is well conditioned"""
    rng = np.random.default_rng(seed)
    src = rng.standard_normal(n + 64)
    x = np.stack([src[32 - DELAYS[c]: 32 - DELAYS[c] + n] + 0.5 * rng.standard_normal(n) for c in range(C)], 1)
    return (0.3 * x).astype(np.float32)


def _scaler(C, seed=3):
    """width (C+P)*F: mel columns around -8 +- 1, GCC columns around 0 +- 0.05, every column different"""
    rng = np.random.default_rng(seed)
    P = C * (C - 1) // 2
    mean = np.concatenate([rng.standard_normal(C * F) - 8.0, 0.02 * rng.standard_normal(P * F)])
    std = np.concatenate([0.5 + rng.random(C * F), 0.03 + 0.04 * rng.random(P * F)])
    return torch.from_numpy(mean), torch.from_numpy(std)


# ───────────── 1. against float64 ─────────────
def _against_float64(C, hop, pad_mode, lengths):
    """bound: 8 x the error of the same definition evaluated in float32 with torch.fft on the CPU (the yardstick, computed here on
    the same input); with a scaler both sides are scaled.  Only a DEGENERATE yardstick is replaced: on a clip of ONE sample
    every frame is an impulse and torch's float32 transforms of it can be exact (1e-16 measured for C = 2), and 8 x that would
    ask a float32 kernel for float64 results.  Where the unscaled yardstick is below 1e-9 it is taken as 2^-24, half an ulp of
    the peak value 1 that a float32 result is rounded to (times the column's 1/sigma with a scaler, added to the scaling's own
    rounding); everywhere else the bound is 8 x the yardstick as measured."""
    from sed_crnn_amd import feature
    P = C * (C - 1) // 2
    mean, std = _scaler(C)
    mu64, is64 = mean.numpy()[C * F:], 1.0 / std.numpy()[C * F:]
    mu32, is32 = mu64.astype(np.float32), is64.astype(np.float32)
    worst, worst_ratio = 0.0, 0.0
    for n in lengths:
        x = _broadband(n, C, seed=n + C)
        want, zeroed = spatial_ref.gcc_phat(x, hop=hop, n_lags=F, pad_mode=pad_mode)
        assert zeroed == 0, (n, zeroed)                                   # the reference dropped no bin: no empty bins in the input
        yard = spatial_ref.gcc_phat_f32(x, hop=hop, n_lags=F, pad_mode=pad_mode)
        assert want.shape == (1 + n // hop, P * F) and np.abs(want).max() <= 1.0 + 1e-9
        for scaled in (False, True):
            kw = dict(mean=mean, std=std) if scaled else {}
            got = feature.mbe(torch.from_numpy(x).cuda(), hop=hop, pad_mode=pad_mode, channels=C, keep_channels=True,
                              spatial="gcc_phat", **kw)
            assert got.shape == (1 + n // hop, (C + P) * F)
            g = got[:, C * F:].cpu().numpy().astype(np.float64)
            w, y = (want, yard) if not scaled else ((want - mu64) * is64, ((yard - mu32) * is32).astype(np.float64))
            e_yard, e_kernel = np.abs(y - w).max(), np.abs(g - w).max()
            degenerate = np.abs(yard - want).max() < DEGENERATE
            if degenerate:
                e_yard = 2.0 ** -24 if not scaled else e_yard + (2.0 ** -24 * is64).max()
            print(f"C={C} hop={hop} {pad_mode} n={n} scaled={scaled}: yardstick {e_yard:.2e}{' (degenerate: replaced)' if degenerate else ''}"
                  f"  kernel {e_kernel:.2e}  ratio {e_kernel / e_yard:.2f}")
            assert np.isfinite(g).all() and e_kernel <= 8.0 * e_yard, (n, scaled, e_kernel, e_yard)
            worst_ratio = max(worst_ratio, e_kernel / e_yard)
            if not scaled:
                worst = max(worst, e_kernel)
                assert np.abs(g).max() <= 1.0 + 1e-6
    print(f"C={C} hop={hop} {pad_mode}: worst kernel error {worst:.2e}, worst kernel / yardstick {worst_ratio:.2f}")


@pytest.mark.parametrize("pad_mode", ["constant", "reflect"])
@pytest.mark.parametrize("hop", [1024, 441])
@pytest.mark.parametrize("C", [2, 3, 4])
def test_gcc_columns_match_the_float64_definition(sed, C, hop, pad_mode):
    _against_float64(C, hop, pad_mode, LENGTHS)


@pytest.mark.parametrize("C", [6, 8])
def test_gcc_columns_of_many_channels_in_batches_of_pairs(sed, C):
    """C = 6 and 8: the 15 / 28 cross spectra do not fit LDS at once and are made 9 / 7 pairs at a time (the loop over pair
    batches of the kernel, its largest launch at C = 8); same reference, same bound"""
    _against_float64(C, 1024, "constant", (1, 5000))
    _against_float64(C, 441, "reflect", (2047,))


def test_a_delay_peaks_at_minus_d(sed):
    from sed_crnn_amd import feature
    x = _broadband(9000, 3, seed=5)
    got = feature.mbe(torch.from_numpy(x).cuda(), channels=3, keep_channels=True, spatial="gcc_phat")[:, 3 * F:].cpu().numpy()
    for p, (i, j) in enumerate(spatial_ref.pairs(3)):
        d = DELAYS[j] - DELAYS[i]                                         # channel j lags channel i by d samples
        assert (got[1:-1, p * F:(p + 1) * F].argmax(1) == F // 2 - d).all(), (i, j)


# ───────────── 2. silence ─────────────
def test_a_silent_channel_gives_exact_zeros(sed):
    from sed_crnn_amd import feature
    x = _broadband(5000, 3, seed=9)
    x[:, 1] = 0.0
    mean, std = _scaler(3)
    got = feature.mbe(torch.from_numpy(x).cuda(), channels=3, keep_channels=True, spatial="gcc_phat")[:, 3 * F:].cpu().numpy()
    assert np.isfinite(got).all()
    assert not got[:, :F].any() and not got[:, 2 * F:].any() and got[:, F:2 * F].any()      # pairs (0,1) and (1,2) hold the silent channel
    sc = feature.mbe(torch.from_numpy(x).cuda(), channels=3, keep_channels=True, spatial="gcc_phat", mean=mean, std=std)[:, 3 * F:]
    m32, i32 = feature._scaler(mean, std, "cpu")
    rest = (-m32[3 * F:]) * i32[3 * F:]
    sc = sc.cpu()
    assert torch.isfinite(sc).all()
    for p in (0, 2):
        assert np.array_equal(_bits(sc[:, p * F:(p + 1) * F]), _bits(rest[p * F:(p + 1) * F].expand(sc.shape[0], F).contiguous()))
    allz = feature.mbe(torch.zeros(3000, 2, device="cuda"), channels=2, keep_channels=True, spatial="gcc_phat")[:, 2 * F:]
    assert not allz.any()


# ───────────── 3. the mel columns, bit for bit ─────────────
@pytest.mark.parametrize("C", [2, 4])
def test_mel_columns_are_bitwise_the_multichannel_log_mel(sed, C):
    from sed_crnn_amd import feature
    mean, std = _scaler(C)
    for pad_mode, hop in (("constant", 1024), ("reflect", 441)):
        for n in (1, 2047, 5000):
            x = torch.from_numpy(_broadband(n, C, seed=n)).cuda()
            for scaled in (False, True):
                kw = dict(mean=mean, std=std) if scaled else {}
                kw_mel = dict(mean=mean[:C * F], std=std[:C * F]) if scaled else {}
                got = feature.mbe(x, hop=hop, pad_mode=pad_mode, channels=C, keep_channels=True, spatial="gcc_phat", **kw)
                mel = feature.mbe(x, hop=hop, pad_mode=pad_mode, channels=C, keep_channels=True, **kw_mel)
                assert np.array_equal(_bits(got[:, :C * F]), _bits(mel)), (pad_mode, hop, n, scaled)


# ───────────── 4. batch against loop ─────────────
def test_batch_equals_the_per_recording_calls(sed):
    from sed_crnn_amd import feature
    C = 3
    mean, std = _scaler(C)
    waves = [torch.from_numpy(_broadband(n, C, seed=n)).cuda() for n in (5000, 1, 9000)]
    many, off = feature.mbe_many(waves, channels=C, keep_channels=True, spatial="gcc_phat", mean=mean, std=std)
    assert off == [0, 5, 6, 15] and many.shape == (15, 6 * F)
    singles = [feature.mbe(w, channels=C, keep_channels=True, spatial="gcc_phat", mean=mean, std=std) for w in waves]
    for i, one in enumerate(singles):
        assert np.array_equal(_bits(many[off[i]:off[i + 1]]), _bits(one)), i
    # the same recordings as planar clips of one buffer, the last one starting at an unaligned sample offset
    # (4-byte aligned only: its frames take the guarded load path and must give the same bits)
    pieces, clips, at = [], [], 0
    for r, w in enumerate(waves):
        lead = (-at) % 4 + (3 if r == 2 else 0)
        pieces.append(torch.zeros(lead, device="cuda"))
        at += lead
        for c in range(C):
            clips.append((at, w.shape[0]))
            pieces.append(w[:, c].contiguous())
            at += w.shape[0]
            if r == 0:                                                    # keep recording 0's channels on 16-byte boundaries
                pad = (-at) % 4
                pieces.append(torch.zeros(pad, device="cuda"))
                at += pad
    buf = torch.cat(pieces)
    assert all(clips[6 + c][0] % 2 == 1 for c in range(C))
    planar, off2 = feature.mbe_planar(buf, clips, C, spatial="gcc_phat", mean=mean, std=std)
    assert off2 == off and np.array_equal(_bits(planar), _bits(many))


# ───────────── 5. the detector, batches and live feeds ─────────────
def _stereo16(n, seed):
    x = _broadband(n, 2, seed)
    env = (np.sin(2 * np.pi * 1.3 * np.arange(n) / 48000) > 0)[:, None]    # bursts, so that the track crosses the threshold
    return np.clip(np.round(x * (0.2 + 0.8 * env) * 32768 * 0.5), -32768, 32767).astype(np.int16)


@pytest.fixture(scope="module")
def det3(sed):
    """a Lightning-size net with 3 input channels (2 mel images + 1 GCC image) centred on the threshold, a scaler of width
    3 * 40 fitted on spatial features, max_batch=1 (tracks are then bit for bit the same however the windows are grouped)"""
    from oracle import crnn_ref
    from sed_crnn_amd import data, feature
    r, m = crnn_ref.LightningNetRef(dropout=0.0, in_channels=3), sed.LightningTimePooledCRNN(dropout=0.0, in_channels=3)
    sd = crnn_ref.rs_state_dict(r, 4)
    r.load_state_dict(sd)
    m.load_state_dict(sd)
    r, m = r.eval(), m.cuda().eval()
    x = _stereo16(48000 * 3, 0)
    raw = feature.mbe(x, input_sr=48000, channels=2, keep_channels=True, spatial="gcc_phat", device="cuda")
    mean, std = data.standard_scaler_fit(raw)
    assert mean.numel() == 3 * F
    mel = feature.mbe(x, input_sr=48000, channels=2, keep_channels=True, spatial="gcc_phat", device="cuda", mean=mean, std=std)
    _centre_on_threshold(r, m, np.concatenate([mel.cpu().numpy()] * 2))
    return sed.EventDetector(m, max_batch=1, median=3, mean=mean, std=std, spatial="gcc_phat"), x


def _same(a, b, what):
    assert torch.equal(a.probs, b.probs), what
    _assert_events_equal({k: v.cpu().numpy() for k, v in a.events.items()}, {k: v.cpu().numpy() for k, v in b.events.items()}, what)


def test_detector_takes_stereo_pcm_for_a_three_input_channel_net(sed, det3):
    from sed_crnn_amd import feature
    det, x = det3
    a = det(x, sr=48000, channels=2)
    mel = feature.mbe(x, input_sr=48000, channels=2, keep_channels=True, spatial="gcc_phat", device="cuda", mean=det.mean, std=det.std)
    assert mel.shape[1] == 3 * F
    _same(a, det.from_features(mel), "stereo int16 at 48 kHz")
    assert len(a) > 0
    clips, rates = [x, _stereo16(44100 * 2 + 5, 2), _stereo16(16000 * 2 + 3, 3)], [48000, 44100, 16000]
    res = det.detect_many(clips, sr=rates, channels=2)
    for i, (w, sr) in enumerate(zip(clips, rates)):
        _same(res[i], det(w, sr=sr, channels=2), f"detect_many clip {i}")
    _same(det.with_decoder(median=3)(x, sr=48000, channels=2), a, "with_decoder keeps the spatial switch")
    with pytest.raises(ValueError, match="reads 2 audio channels.*got channels=3"):
        det(np.zeros((5000, 3), np.int16), sr=48000, channels=3)


def test_spatial_streams_are_bitwise_the_offline_call(sed, det3):
    det, _ = det3
    sizes = [1, 1, 159, 997, 0, 60_000, 3]
    recs = [_stereo16(48000 * 3 + 1, 10), _stereo16(105_001, 11)]
    st = det.stream(2, keep_probs=True, max_new_windows=1, input_sr=48000)
    assert st.input_channels == 2 and st.C == 2 and st.CF == 3 * F
    outs = _feed(st, recs, sizes) + [st.flush()]
    tracks, evs = _collect(outs, 2)
    n_events = 0
    for s, w in enumerate(recs):
        one = det(w, sr=48000, channels=2)
        n_events += len(one)
        assert torch.equal(tracks[s], one.probs), s
        _assert_events_equal(evs[s], {k: v.cpu().numpy() for k, v in one.events.items()}, f"feed {s}")
    assert n_events > 0


# ───────────── 6. nets with 3 and 10 input channels ─────────────
@pytest.mark.parametrize("cin,conv", [(3, 8), (3, 16), (10, 8), (10, 16)])
def test_nets_with_spatial_input_channel_counts_vs_oracle(sed, cin, conv):
    """in_channels = 3 (2 microphones) takes the first block's Cin == 3 code, 10 (4 microphones) the generic first conv: one
    training step (loss, every gradient) and one eval forward against the CPU oracle, with the tolerances of the small-net
    oracle tests (test_gpu_model._oracle_vs_hip)"""
    from oracle import crnn_ref
    from test_gpu_model import _oracle_vs_hip
    torch.manual_seed(40 + cin + conv)
    ref = crnn_ref.SedNetRef(conv_channels=conv, dropout=0.0, in_channels=cin, n_mels=F, gru_hidden=16)
    m = sed.TimePooledCRNN(conv_channels=conv, dropout=0.0, in_channels=cin, n_mels=F, gru_hidden=16)
    x, y = crnn_ref.synthetic_batch(4, cin, F, 32, 4, seed=cin)
    _oracle_vs_hip(sed, ref, m, x, y)


@pytest.mark.parametrize("cin", [3, 10])
def test_lightning_nets_with_spatial_input_channel_counts_vs_oracle(sed, cin):
    from oracle import crnn_ref
    from test_gpu_model import _oracle_vs_hip
    torch.manual_seed(50 + cin)
    ref = crnn_ref.LightningNetRef(dropout=0.0, in_channels=cin)
    m = sed.LightningTimePooledCRNN(dropout=0.0, in_channels=cin)
    x, y = crnn_ref.synthetic_batch(4, cin, F, 32, 4, seed=cin + 1)
    _oracle_vs_hip(sed, ref, m, x, y, loss="focal")
