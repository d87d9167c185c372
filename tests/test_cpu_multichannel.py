"""Multichannel audio in, without a GPU: the host validators of sed_logmel_multi and sed_resample_select, which
refuse a bad table before anything is uploaded or launched, and the argument checks of the detector and the live-stream
detector for nets with more than one input channel."""
import ctypes as C

import numpy as np
import pytest

FAKE = C.c_void_p(4096)          # a non-null device address: every call below is refused before anything is uploaded or launched


def _err():
    from sed_crnn_amd._lib import lib
    return lib().sed_last_error_string().decode()


def test_logmel_multi_refuses_bad_tables_without_a_gpu_call():
    from sed_crnn_amd._lib import lib
    L = lib()
    assert L.sed_logmel_multi_workspace_bytes(3, 2) == (5 * 3 * 2 + 1) * 8
    for bad in ((0, 2), (3, 0), (3, 65), (-1, 1), (1 << 26, 2)):
        assert L.sed_logmel_multi_workspace_bytes(*bad) == 0, bad
    blob = 16 * 2400                                                  # the size of a 40-band table: the checks never read it

    def call(clips, channels=2, pcm_len=10_000, rows=None, ws=None, R=None, mu=None, tables_bytes=blob, n_mels=40):
        t = np.ascontiguousarray(np.asarray(clips, np.int64).reshape(-1, 2))
        R = t.shape[0] // max(channels, 1) if R is None else R
        rows = int((1 + t[::max(channels, 1), 1] // 1024).sum()) if rows is None else rows
        ws = L.sed_logmel_multi_workspace_bytes(R, channels) if ws is None else ws
        return L.sed_logmel_multi(FAKE, pcm_len, C.c_void_p(t.ctypes.data), R, channels, FAKE, tables_bytes, mu, mu, FAKE, rows, 2048,
                                  1024, n_mels, 0, FAKE, ws, None)

    good = [(0, 3000), (3000, 3000), (6000, 500), (6500, 500)]        # two recordings x two channels
    # (a good table passes every host check; it would go on to the upload, which needs a GPU, so it is not called here)
    assert call([(0, 3000), (3000, 2999), (6000, 500), (6500, 500)]) != 0
    assert "recording 0" in _err() and "equal length" in _err()
    assert call([(0, 3000), (3000, 3000), (6000, 500), (6500, 501)]) != 0 and "recording 1" in _err()
    assert call([(0, 3000), (3000, 3000), (6000, 500), (9600, 500)]) != 0
    assert "recording 1, channel 1" in _err() and "is not inside the PCM buffer" in _err()
    assert call([(0, 3000), (-8, 3000), (6000, 500), (6500, 500)]) != 0 and "recording 0, channel 1" in _err()
    want_rows = (1 + 3000 // 1024) + (1 + 500 // 1024)
    assert call(good, rows=want_rows + 1) != 0 and "rows" in _err()
    assert call(good, rows=want_rows - 1) != 0 and "rows" in _err()
    assert call(good, channels=0, R=2) != 0 and "channels" in _err()
    assert call(good, channels=-2, R=2) != 0 and "channels" in _err()
    assert call(good, ws=L.sed_logmel_multi_workspace_bytes(2, 2) - 8) != 0 and "workspace" in _err()
    # the scaler stays in LDS: 64 channels x 128 bands x 2 x 4 B = 64 KiB beside a 100 000-byte table leave no room for the FFT
    # scratch of even 2 waves (19 456 B) in 160 KiB; the same table without a scaler, or with 4 channels, passes that check
    wide = [(64 * i, 64) for i in range(64)]
    assert call(wide, channels=64, mu=FAKE, tables_bytes=100_000, n_mels=128, rows=2) != 0
    assert "scaler of 65536 bytes" in _err() and "160 KiB" in _err()
    assert call(wide, channels=64, mu=None, tables_bytes=100_000, n_mels=128, rows=2) != 0 and "rows" in _err()
    assert call(wide[:4], channels=4, mu=FAKE, tables_bytes=100_000, n_mels=128, rows=2) != 0 and "rows" in _err()
    assert L.sed_logmel_multi(FAKE, 100, None, 1, 1, FAKE, blob, None, None, FAKE, 1, 2048, 1024, 40, 0, FAKE, 1024, None) != 0
    assert "null pointer" in _err()


def test_resample_select_validator_refuses_channels_outside_the_frames():
    from sed_crnn_amd import _lib
    from sed_crnn_amd.resample import ResamplePlan, build_keep_rows, build_rows, check_rows, with_channels
    L = _lib.lib()
    assert L.sed_resample_select_workspace_bytes(0) == 0 and L.sed_resample_select_workspace_bytes(5) == 5 * 80 + 24
    plan = ResamplePlan(48000)
    a = (plan.L, plan.M, plan.half)
    # the table resample_many(keep_channels=True) builds: three clips x three channels
    n_in = [1000, 1, 77]
    rows, x_frames, out_len = build_keep_rows(n_in, [plan.n_out(n) for n in n_in], 3)
    assert rows.shape == (9, 10) and x_frames == 1078 and (rows[:, 5] % 4 == 0).all()
    assert rows[:, 9].tolist() == [0, 1, 2] * 3 and rows[:, 0].tolist() == [0] * 3 + [1000] * 3 + [1001] * 3
    check_rows(rows, x_frames, 0, out_len, *a, channels=3)
    one, _, n1 = build_rows([100], None, None, [92])
    for ch in (-1, 0, 2):                                              # -1: today's downmix
        check_rows(with_channels(one, [ch]), 100, 0, n1, *a, channels=3)
    for ch, C_in in ((3, 3), (1, 1), (-2, 3), (64, 64)):
        with pytest.raises(_lib.SedHipError, match="channel"):
            check_rows(with_channels(one, [ch]), 100, 0, n1, *a, channels=C_in)
    with pytest.raises(_lib.SedHipError, match="channels"):
        check_rows(with_channels(one, [0]), 100, 0, n1, *a, channels=65)
    bad = with_channels(one, [0])
    bad[0, 1] = 101                                                    # the checks of sed_resample_check_table still hold
    with pytest.raises(_lib.SedHipError, match="not inside the input buffer"):
        check_rows(bad, 100, 0, n1, *a, channels=3)
    # the launch itself refuses the same things before it touches a GPU
    r = with_channels(one, [2])
    args = lambda ch=2, ws=L.sed_resample_select_workspace_bytes(1): (FAKE, 100, 1, ch, None, 0, FAKE, plan.taps.size, *a,   # noqa: E731
                                                                      C.c_void_p(r.ctypes.data), 1, FAKE, n1, FAKE, ws, None)
    assert L.sed_resample_select(*args()) != 0 and "channel 2 is outside [-1, 2)" in _err()
    assert L.sed_resample_select(*args(ch=3, ws=80)) != 0 and "workspace" in _err()


def _stereo_net():
    import sed_crnn_amd as sed
    return sed.TimePooledCRNN(conv_channels=32, dropout=0.0, in_channels=2, gru_hidden=32).eval()


def test_detector_checks_for_a_two_channel_net_without_a_gpu():
    import sed_crnn_amd as sed
    m = _stereo_net()
    det = sed.EventDetector(m, mean=np.zeros(80), std=np.ones(80))
    x = np.zeros((50_000, 2), np.int16)
    # valid input, model left on the CPU: the existing refusal, before anything else
    for call in (lambda: det(x, sr=48000, channels=2), lambda: det.detect_many([x, x], sr=48000, channels=2),
                 lambda: sed.detect_events(m, x, input_sr=48000, channels=2),
                 lambda: sed.detect_events_many(m, [x], input_sr=48000, channels=2)):
        with pytest.raises(sed.SedHipError, match="move the module to the GPU first"):
            call()
    # channels must be the net's own count: both numbers are named, and nothing is mixed down or duplicated
    for bad in (1, 4):
        for call in (lambda: det(x, sr=48000, channels=bad), lambda: det.detect_many([x], sr=48000, channels=bad),
                     lambda: sed.detect_events(m, x, input_sr=48000, channels=bad)):
            with pytest.raises(ValueError, match=rf"a 2-channel net takes \[N, 2\].*got channels={bad}"):
                call()
    with pytest.raises(ValueError, match="a 2-channel net"):
        det(np.zeros(50_000, np.float32))                              # a mono waveform is not duplicated
    with pytest.raises(ValueError, match=r"recording 1: expected a waveform of shape \[N, 2\]"):
        det.detect_many([x, np.zeros(50_000, np.int16)], sr=48000, channels=2)
    with pytest.raises(ValueError, match="recording 1: a recording of 1 frames"):
        det.detect_many([x, x[:100]], sr=48000, channels=2)
    # the scaler has one entry per feature column
    with pytest.raises(ValueError, match=r"2-channel net.*2\*40 = 80.*got 40 / 40"):
        sed.EventDetector(m, mean=np.zeros(40), std=np.ones(40))
    sed.EventDetector(m)                                               # no scaler is fine
    # a 1-channel net keeps downmixing: channels=2 is not refused for it (the CPU model is)
    mono = sed.EventDetector(sed.LightningTimePooledCRNN(dropout=0.0).eval())
    with pytest.raises(sed.SedHipError, match="move the module to the GPU first"):
        mono(x, sr=48000, channels=2)


def test_stream_detector_checks_for_a_two_channel_net_without_a_gpu():
    import sed_crnn_amd as sed
    m = _stereo_net()
    st = sed.StreamDetector(m, 3, input_sr=48000)
    assert st.input_channels == 2 and st.C == 2 and st._rs is not None
    own = sed.EventDetector(m).stream(2)                               # the detector's own rate: the copy filter, always on
    assert own.input_channels == 2 and own._rs is not None and own._rs.identity
    for bad in (1, 4):
        with pytest.raises(ValueError, match=rf"a 2-channel net.*input_channels must be 2, got {bad}"):
            sed.StreamDetector(m, 3, input_channels=bad)
    sed.StreamDetector(m, 65535 // 2)                                  # 65 534 lanes fit
    with pytest.raises(ValueError, match="65536 lanes"):
        sed.StreamDetector(m, 32768)
    # the larger carries are counted: per feed two lanes of PCM carry and of resampler carry
    mono = sed.StreamDetector(sed.TimePooledCRNN(conv_channels=32, dropout=0.0, gru_hidden=32).eval(), 3, input_sr=48000)
    assert st._core_bytes == mono._core_bytes and st.CC == mono.CC and st._rCR == mono._rCR
    assert st.state_bytes - mono.state_bytes == 4 * 3 * 2 * (st.FC * 40 + st.CC + st._rCR)
    with pytest.raises(ValueError, match="expected 3 waveform pieces"):
        st.push([np.zeros((10, 2), np.int16)])
    with pytest.raises(ValueError, match=r"stream 1: expected a waveform of shape \[N, 2\].*use push_features"):
        st.push([None, np.zeros(500, np.int16), None])
    with pytest.raises(sed.SedHipError, match="move the module to the GPU"):
        st.push([np.zeros((5000, 2), np.int16)] * 3)                   # valid input, CPU model
    assert st._state is None and not st.sched.N.any()
