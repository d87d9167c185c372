"""Per-event TDOA without a GPU: the rule that picks an event's frames against hand-worked cases, the float64
reference (tests/tdoa_ref.py) on synthetic delays, the settings object, the geometry helpers and the host-only argument checks
of EventDetector and sed_event_tdoa."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import spatial_ref  # noqa: E402
import tdoa_ref  # noqa: E402

DELAYS = (0, 7, -3, 12)


# ───────────── 1. the frames of an event ─────────────
@pytest.mark.parametrize("event,tf,n_feat,max_frames,want", [
    ((3, 7, 5), 1, 100, 256, (3, 7)),                 # a short event, tf = 1
    ((2, 5, 3), 4, 100, 256, (8, 20)),                # tf = 4: output frame j covers feature frames [4j, 4j + 4)
    ((20, 30, 22), 4, 103, 256, (80, 103)),           # cut at the recording's end: 30 * 4 = 120 > 103 feature frames
    ((20, 26, 22), 4, 103, 256, (80, 103)),           # the ragged tail: offset * tf = 104 is one frame beyond the last
    ((10, 50, 10), 1, 100, 8, (10, 18)),              # longer than max_frames, peak at the start: clamped to the onset
    ((10, 50, 30), 1, 100, 8, (26, 34)),              # ... in the middle: centred, 30 - 8 // 2
    ((10, 50, 49), 1, 100, 8, (42, 50)),              # ... at the end: clamped to offset - max_frames
    ((10, 50, 10), 4, 300, 8, (40, 48)),              # tf = 4: c = 40 + 2 - 4 = 38 -> 40
    ((10, 50, 30), 4, 300, 8, (118, 126)),            # c = 120 + 2 - 4
    ((10, 50, 49), 4, 300, 8, (192, 200)),            # c = 196 + 2 - 4 = 194 -> 200 - 8
    ((10, 50, 49), 4, 190, 8, (182, 190)),            # the same event cut at 190 frames: clamped to the cut end
    ((10, 50, 30), 1, 100, 5, (28, 33)),              # an odd max_frames: 30 - 5 // 2
    ((10, 18, 12), 1, 100, 8, (10, 18)),              # exactly max_frames frames: all of them
    ((10, 19, 18), 1, 100, 8, (11, 19)),              # one more
    ((5, 5, 5), 2, 100, 256, (10, 11)),               # an empty event (no decoder emits one): the single frame a
    ((60, 70, 65), 2, 100, 256, (0, 0)),              # wholly beyond the recording: no frames
    ((-1, 3, 0), 2, 100, 256, (0, 0)),                # a negative onset: no frames
])
def test_event_frames_against_hand_worked_cases(event, tf, n_feat, max_frames, want):
    import sed_crnn_amd as sed
    from sed_crnn_amd.localize import event_frames
    assert sed.event_frames is event_frames
    got = event_frames(*event, tf, n_feat, max_frames)
    assert got == want and all(isinstance(v, int) for v in got)


def test_event_frames_refuses_bad_sizes():
    from sed_crnn_amd.localize import event_frames
    for bad in (dict(time_factor=0, n_feat=10), dict(time_factor=1, n_feat=0), dict(time_factor=1, n_feat=10, max_frames=0)):
        with pytest.raises(ValueError, match="event_frames needs"):
            event_frames(0, 1, 0, **bad)


# ───────────── 2. the float64 reference on synthetic delays ─────────────
@pytest.mark.parametrize("n", [2048, 9000, 40000])
def test_reference_finds_integer_delays(n):
    """channel c = a white source delayed by DELAYS[c] plus 0.5 x its own noise; lag = -(DELAYS[j] - DELAYS[i]) within half a
    sample (the peak is the nearest integer and the parabola moves it by less than half a sample), and no other searched lag
    comes within half the peak (measured: 0.22 at most), so that arg-max comparisons against a float32 kernel are never near-ties"""
    hop, max_lag = 1024, 24
    x = tdoa_ref.broadband(n, DELAYS, seed=n)
    curves, zeroed = tdoa_ref.frame_curves(x, hop, max_lag)
    n_feat = 1 + n // hop
    assert zeroed == 0 and curves.shape == (n_feat, 6, 2 * max_lag + 3)
    ref = tdoa_ref.event_tdoa(curves, [(0, n_feat, 0), (1, 4, 2)], 1)
    assert ref["ranges"] == [(0, n_feat), (1, min(4, n_feat))]
    for e in range(2):
        for p, (i, j) in enumerate(spatial_ref.pairs(4)):
            d = DELAYS[j] - DELAYS[i]
            print(f"n={n} event {e} pair {(i, j)}: lag {ref['lag'][e, p]:+.3f} (true {-d:+d}) strength {ref['strength'][e, p]:.3f} "
                  f"second/peak {ref['second'][e, p]:.3f}")
            assert abs(ref["lag"][e, p] + d) <= 0.5 and ref["t"][e, p] == -d
            assert ref["second"][e, p] < 0.5
            assert 0.0 < ref["strength"][e, p] <= 1.0


def test_reference_accumulation_is_the_synthesis_of_the_summed_spectra():
    """acc, defined through S[k] = sum_f Pk_f[k], against the sum of the per-frame curves that tdoa_ref uses (linearity)"""
    hop, max_lag = 441, 5
    x = tdoa_ref.broadband(3000, DELAYS[:2], seed=1)
    curves, _ = tdoa_ref.frame_curves(x, hop, max_lag)
    spec = [np.fft.rfft(spatial_ref.frames_of(x[:, c], hop).astype(np.float64), axis=1) for c in range(2)]
    G = spec[0] * np.conj(spec[1])
    S = (G / np.abs(G))[2:6].sum(0)
    S[0], S[-1] = S[0].real, S[-1].real
    tau = np.arange(-(max_lag + 1), max_lag + 2)
    k = np.arange(1, 1024)
    acc = (S[0].real + (-1.0) ** tau * S[-1].real + 2.0 * (S[None, 1:-1] * np.exp(2j * np.pi * k[None, :] * tau[:, None] / 2048)).real.sum(1)) / 2048
    np.testing.assert_allclose(tdoa_ref.event_tdoa(curves, [(2, 6, 3)], 1)["acc"][0, 0], acc, rtol=0, atol=1e-12)


def test_reference_on_silence_and_parabola():
    assert tdoa_ref.peak(np.zeros(9), 4)[:3] == (0.0, 0.0, 0)
    acc = np.array([0.0, 0.1, 0.5, 1.0, 0.5, 0.1, 0.0])                 # max_lag 2, symmetric around tau = 0
    assert tdoa_ref.peak(acc, 2)[:3] == (0.0, 0.5, 0)
    acc = np.array([0.0, 0.0, 0.2, 1.0, 0.6, 0.0, 0.0])                 # l = 0.2, m = 1, r = 0.6: 0.5 * (-0.4) / (-1.2)
    lag, strength, t, second = tdoa_ref.peak(acc, 1)
    assert t == 0 and abs(lag - 1.0 / 6.0) < 1e-15 and strength == 1.0 and second == 0.0
    acc = np.array([9.0, 1.0, 1.0, 0.0, 1.0, 1.0, 9.0])                 # ties: the FIRST maximum, and the unsearched ends do not count
    assert tdoa_ref.peak(acc, 1)[2] == -2


# ───────────── 3. settings and geometry ─────────────
def test_tdoa_settings_are_validated():
    import sed_crnn_amd as sed
    t = sed.TDOA()
    assert (t.max_lag, t.max_frames) == (24, 256) and sed.TDOA(max_lag=np.int64(7), max_frames=1) == sed.TDOA(7, 1)
    for bad in (dict(max_lag=0), dict(max_lag=128), dict(max_lag=2.5), dict(max_lag=True), dict(max_frames=0), dict(max_frames="8")):
        with pytest.raises(ValueError, match="TDOA"):
            sed.TDOA(**bad)
    with pytest.raises(Exception):
        t.max_lag = 3                                                   # frozen


def test_geometry_helpers():
    import sed_crnn_amd as sed
    assert sed.max_lag_for(0.2, 44100) == math.ceil(0.2 * 44100 / 343.0) == 26
    assert sed.max_lag_for(0.343, 1000, c=343.0) == 1 and sed.max_lag_for(0.05, 16000) == 3
    with pytest.raises(ValueError):
        sed.max_lag_for(0.0, 44100)
    d = 0.2
    az = sed.tdoa_to_azimuth(np.array([0.0, d / 343.0, -d / 343.0, 2 * d / 343.0, -1.0, 0.5 * d / 343.0]), d)
    np.testing.assert_allclose(az, [0.0, np.pi / 2, -np.pi / 2, np.pi / 2, -np.pi / 2, np.pi / 6], rtol=0, atol=1e-12)
    assert float(sed.tdoa_to_azimuth(0.0, 0.1)) == 0.0
    with pytest.raises(ValueError):
        sed.tdoa_to_azimuth(0.0, -1.0)


def _net(cin):
    import sed_crnn_amd as sed
    return sed.LightningTimePooledCRNN(dropout=0.0, in_channels=cin, n_mels=40).eval()


def test_detector_argument_checks():
    import sed_crnn_amd as sed
    with pytest.raises(ValueError, match="reads 1"):
        sed.EventDetector(_net(1), localize=sed.TDOA())
    with pytest.raises(ValueError, match="reads 10"):
        sed.EventDetector(_net(10), localize=sed.TDOA())                # ten plain channels: more than the 8 that pairs are made of
    with pytest.raises(TypeError, match="TDOA"):
        sed.EventDetector(_net(2), localize=dict(max_lag=3))
    det = sed.EventDetector(_net(2), localize=sed.TDOA(5, 16))
    assert det.localize_settings == sed.TDOA(5, 16) and det.with_decoder(threshold=0.3).localize_settings == sed.TDOA(5, 16)
    assert sed.EventDetector(_net(10), spatial="gcc_phat", localize=sed.TDOA()).audio_channels == 4
    assert sed.EventDetector(_net(2)).localize_settings is None
    with pytest.raises(NotImplementedError, match="live feeds"):
        det.stream(1)
    with pytest.raises(NotImplementedError, match="live feeds"):
        sed.StreamDetector(_net(2), 1, localize=sed.TDOA())
    with pytest.raises(ValueError, match="no localisation settings"):
        sed.EventDetector(_net(2)).localize(None, None)
    with pytest.raises(ValueError, match="holds no lags"):
        sed.DetectionResult(None, {"cls": None}, 0.1, None).tdoa()


def test_c_entry_checks_its_arguments_on_the_host():
    from sed_crnn_amd import _lib
    L = _lib.lib()
    row = 1026 * 8
    assert L.sed_event_tdoa_workspace_bytes(1, 2, 0, 5000, 1024, 256) == 32                       # sample_off [2], n_samples [1], to 16
    assert L.sed_event_tdoa_workspace_bytes(1, 2, 3, 5000, 1024, 256) == 32 + 3 * 1 * 1 * row     # 5 frames: one chunk, one pair
    assert L.sed_event_tdoa_workspace_bytes(2, 4, 10, 100 * 1024, 1024, 40) == 80 + 10 * 2 * 6 * row   # 40 frames: two chunks
    for bad in ((0, 2, 1, 5000, 1024, 8), (1, 1, 1, 5000, 1024, 8), (1, 9, 1, 5000, 1024, 8), (1, 2, -1, 5000, 1024, 8),
                (1, 2, 1, 0, 1024, 8), (1, 2, 1, 5000, 0, 8), (1, 2, 1, 5000, 1024, 0)):
        assert L.sed_event_tdoa_workspace_bytes(*bad) == 0, bad
    FAKE, blob = C.c_void_p(0x1000), (8 + 2048 + 2048 + 1028) * 4

    def call(clips, channels=2, pcm_len=20000, E=1, max_lag=24, max_frames=8, ws=1 << 20, rec=None, R=1, tf=1, hop=1024, pad=0):
        t = np.asarray(clips, dtype=np.int64)
        return L.sed_event_tdoa(FAKE, pcm_len, C.c_void_p(t.ctypes.data), R, channels, FAKE, blob, rec, FAKE, FAKE, FAKE, E, tf, hop,
                                pad, max_lag, max_frames, FAKE, FAKE, FAKE, None, FAKE, ws, None)

    def err():
        return L.sed_last_error_string().decode()
    good = [(0, 5000), (8000, 5000)]
    assert call(good, channels=1) != 0 and "channels" in err()
    assert call(good, max_lag=0) != 0 and "max_lag" in err()
    assert call(good, max_lag=128) != 0 and "max_lag" in err()
    assert call(good, max_frames=0) != 0 and "max_frames" in err()
    assert call(good, tf=0) != 0 and "bad sizes" in err()
    assert call(good, pad=2) != 0 and "pad_mode" in err()
    assert call([(0, 5000), (18000, 5000)]) != 0 and "not inside the PCM buffer" in err()
    assert call([(0, 5000), (8000, 4000)]) != 0 and "equal length" in err()
    assert call(good + good, R=2) != 0 and "need ev_rec" in err()
    assert call(good, ws=32 + row - 16) != 0 and "workspace" in err()
    assert call(good, E=0, ws=0) == 0                                   # no events: nothing is launched, nothing is needed


def test_build_guards_the_new_kernels_against_scratch():
    from sed_crnn_amd.build import EXTRA_FLAGS, NO_SCRATCH_KERNELS, SOURCES
    assert "tdoa.hip" in SOURCES and set(NO_SCRATCH_KERNELS["tdoa.hip"]) == {"tdoa_accum_k", "tdoa_finish_k"}
    assert EXTRA_FLAGS["tdoa.hip"] == EXTRA_FLAGS["gcc.hip"]
