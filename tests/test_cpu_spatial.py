"""GCC-PHAT spatial features without a GPU: the float64 reference's own properties, the channel arithmetic, the
argument checks of feature.mbe / EventDetector / StreamDetector and the host-only checks of sed_logmel_gcc."""
import ctypes as C

import numpy as np
import pytest

import spatial_ref

FAKE = C.c_void_p(4096)          # a non-null device address: every call below is refused before anything is uploaded or launched


def _err():
    from sed_crnn_amd._lib import lib
    return lib().sed_last_error_string().decode()


def test_reference_finds_a_delay_of_seven_samples():
    rs = np.random.RandomState(1)
    n = rs.randn(9000).astype(np.float32)
    d, L = 7, 40
    x = np.stack([n, np.concatenate([np.zeros(d, np.float32), n[:-d]])], 1)       # channel 1 = channel 0 delayed by d
    cc, zeroed = spatial_ref.gcc_phat(x, hop=1024, n_lags=L)
    assert cc.shape == (1 + 9000 // 1024, L) and zeroed == 0
    inner = cc[1:-1]                                                              # frames that lie inside the recording
    assert (inner.argmax(1) == L // 2 - d).all() and (inner.max(1) > 0.9).all()
    assert np.abs(cc).max() <= 1.0 + 1e-12


def test_reference_on_identical_channels_is_a_unit_pulse_at_lag_zero():
    rs = np.random.RandomState(2)
    n = rs.randn(5000).astype(np.float32)
    L = 40
    cc, zeroed = spatial_ref.gcc_phat(np.stack([n, n], 1), hop=1024, n_lags=L)
    assert zeroed == 0
    assert np.abs(cc[:, L // 2] - 1.0).max() < 1e-12
    assert np.abs(np.delete(cc, L // 2, axis=1)).max() < 1e-12


def test_reference_pair_order_and_silence():
    rs = np.random.RandomState(3)
    x = rs.randn(3000, 3).astype(np.float32)
    cc, _ = spatial_ref.gcc_phat(x, n_lags=8)
    assert spatial_ref.pairs(4) == [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)]
    for p, (i, j) in enumerate(spatial_ref.pairs(3)):
        one, _ = spatial_ref.gcc_phat(x[:, [i, j]], n_lags=8)
        assert np.array_equal(cc[:, 8 * p:8 * p + 8], one)
    x[:, 1] = 0.0                                                                 # digital silence: zeros, and the count says so
    cc, zeroed = spatial_ref.gcc_phat(x, n_lags=8)
    assert zeroed == 2 * cc.shape[0] * 1025 and np.isfinite(cc).all()
    assert not cc[:, :8].any() and not cc[:, 16:].any() and cc[:, 8:16].any()


def test_spatial_channels():
    from sed_crnn_amd import feature
    assert [feature.spatial_channels(c) for c in (2, 3, 4, 8)] == [3, 6, 10, 36]
    assert [feature.audio_channels_of(n) for n in (3, 6, 10, 36)] == [2, 3, 4, 8]
    assert all(feature.audio_channels_of(n) is None for n in (1, 2, 4, 5, 45))


def test_feature_argument_checks():
    from sed_crnn_amd import feature
    x = np.zeros((5000, 2), np.float32)
    with pytest.raises(ValueError, match="needs keep_channels=True"):
        feature.mbe(x, channels=2, spatial="gcc_phat")
    with pytest.raises(ValueError, match="needs keep_channels=True"):
        feature.mbe_many([x], channels=2, spatial="gcc_phat")
    for call in (lambda: feature.mbe(x[:, 0], channels=1, keep_channels=True, spatial="gcc_phat"),
                 lambda: feature.mbe_many([x[:, :1]], channels=1, keep_channels=True, spatial="gcc_phat"),
                 lambda: feature.mbe_planar(None, [(0, 10)], 1, spatial="gcc_phat")):
        with pytest.raises(ValueError, match="needs 2 to 8 audio channels.*got channels=1"):
            call()
    with pytest.raises(ValueError, match="got channels=9"):
        feature.mbe(np.zeros((100, 9), np.float32), channels=9, keep_channels=True, spatial="gcc_phat")
    with pytest.raises(ValueError, match="spatial must be None or 'gcc_phat'"):
        feature.mbe(x, channels=2, keep_channels=True, spatial="srp")


def _net(cin, n_mels=40):
    import sed_crnn_amd as sed
    return sed.LightningTimePooledCRNN(dropout=0.0, in_channels=cin, n_mels=n_mels).eval()


def test_detector_argument_checks():
    import sed_crnn_amd as sed
    x = np.zeros((50_000, 2), np.int16)
    with pytest.raises(ValueError, match=r"in_channels = C \+ C\(C-1\)/2.*the net has in_channels=4"):
        sed.EventDetector(_net(4), spatial="gcc_phat")
    with pytest.raises(ValueError, match="spatial must be None or 'gcc_phat'"):
        sed.EventDetector(_net(3), spatial="phat")
    with pytest.raises(ValueError, match=r"\(C\+P\)\*n_mels = 3\*40 = 120, got 80 / 80"):
        sed.EventDetector(_net(3), spatial="gcc_phat", mean=np.zeros(80), std=np.ones(80))
    det = sed.EventDetector(_net(3), spatial="gcc_phat", mean=np.zeros(120), std=np.ones(120), threshold=0.4)
    assert det.audio_channels == 2 and det.spatial == "gcc_phat"
    d2 = det.with_decoder(threshold=0.7)
    assert d2.spatial == "gcc_phat" and d2.audio_channels == 2 and d2.hi == 0.7
    for bad in (1, 3):                                                            # both numbers are named
        for call in (lambda: det(x, sr=48000, channels=bad), lambda: det.detect_many([x], sr=48000, channels=bad)):
            with pytest.raises(ValueError, match=rf"in_channels=3 reads 2 audio channels.*got channels={bad}"):
                call()
    with pytest.raises(sed.SedHipError, match="move the module to the GPU first"):
        det(x, sr=48000, channels=2)                                              # valid input, model left on the CPU
    assert sed.EventDetector(_net(10), spatial="gcc_phat").audio_channels == 4
    # without `spatial` a 3-channel net is what it was: three audio channels
    plain = sed.EventDetector(_net(3))
    assert plain.spatial is None and plain.audio_channels == 3
    with pytest.raises(ValueError, match=r"a 3-channel net takes \[N, 3\].*got channels=2"):
        plain(x, sr=48000, channels=2)
    # a spatial stream carries C audio lanes per feed and CF = (C+P)*n_mels feature columns
    st = det.stream(2, input_sr=48000)
    assert st.C == 2 and st.input_channels == 2 and st.CF == 120
    with pytest.raises(ValueError, match="input_channels must be 2, got 3"):
        det.stream(2, input_channels=3)


def test_logmel_gcc_host_checks_without_a_gpu_call():
    from sed_crnn_amd._lib import lib
    L = lib()
    assert L.sed_logmel_gcc_workspace_bytes(3, 2) >= L.sed_logmel_multi_workspace_bytes(3, 2) + (3 + 1 + 6 + 3) * 8
    for bad in ((3, 1), (3, 9), (0, 2), (-1, 2), (3, 0)):
        assert L.sed_logmel_gcc_workspace_bytes(*bad) == 0, bad
    blob = 16 * 2400

    def call(clips, channels=2, n_lags=40, pcm_len=10_000, rows=None, ws=None, R=None):
        t = np.ascontiguousarray(np.asarray(clips, np.int64).reshape(-1, 2))
        R = t.shape[0] // max(channels, 1) if R is None else R
        rows = int((1 + t[::max(channels, 1), 1] // 1024).sum()) if rows is None else rows
        ws = L.sed_logmel_gcc_workspace_bytes(R, channels) if ws is None else ws
        return L.sed_logmel_gcc(FAKE, pcm_len, C.c_void_p(t.ctypes.data), R, channels, FAKE, blob, None, None, FAKE, rows, 2048, 1024,
                                40, n_lags, 0, FAKE, ws, None)

    good = [(0, 3000), (3000, 3000), (6000, 500), (6500, 500)]                    # two recordings x two channels
    for ch in (1, 9, 0, -2):
        assert call(good, channels=ch, R=2, ws=1 << 20) != 0 and f"2 to 8 channels, got {ch}" in _err()
    for nl in (39, 1, 0, 130, -2):
        assert call(good, n_lags=nl) != 0 and f"n_lags must be even and in [2,128], got {nl}" in _err()
    assert call([(0, 3000), (3000, 2999), (6000, 500), (6500, 500)]) != 0
    assert "recording 0" in _err() and "equal length" in _err()
    assert call([(0, 3000), (3000, 3000), (6000, 500), (6500, 501)]) != 0 and "recording 1" in _err() and "equal length" in _err()
    assert call([(0, 3000), (3000, 3000), (6000, 500), (9600, 500)]) != 0 and "recording 1, channel 1" in _err()
    want_rows = (1 + 3000 // 1024) + (1 + 500 // 1024)
    assert call(good, rows=want_rows + 1) != 0 and "rows" in _err()
    assert call(good, ws=L.sed_logmel_gcc_workspace_bytes(2, 2) - 16) != 0 and "workspace" in _err()
    assert L.sed_logmel_gcc(FAKE, 100, None, 1, 2, FAKE, blob, None, None, FAKE, 1, 2048, 1024, 40, 40, 0, FAKE, 1 << 20, None) != 0
    assert "null pointer" in _err()
