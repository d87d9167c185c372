"""PCEN without a GPU: the float64 reference's own properties, the settings object, the argument checks of the
feature / detector entry points and the host-only checks of sed_pcen."""
import ctypes as C

import numpy as np
import pytest

import pcen_ref

FAKE = C.c_void_p(4096)          # a non-null device address: every call below is refused before anything is uploaded or launched


def _err():
    from sed_crnn_amd._lib import lib
    return lib().sed_last_error_string().decode()


# ───────────── the reference ─────────────
def _b():
    """the coefficient the package hands to the kernel for the default settings: the reference is exercised with it"""
    import sed_crnn_amd as sed
    return sed.PCEN().smoothing(44100, 1024)


def test_reference_smoother_starts_at_the_first_energy():
    rng = np.random.default_rng(0)
    x = rng.standard_normal((50, 3)) * 2.0 - 6.0
    b = _b()
    M = pcen_ref.smooth(np.exp(x), b)
    np.testing.assert_allclose(M[0], np.exp(x[0]), rtol=1e-15)
    want = np.exp(x[0])
    for t in range(1, 50):                                                    # and follows the recurrence of the definition
        want = (1 - b) * want + b * np.exp(x[t])
        np.testing.assert_allclose(M[t], want, rtol=1e-13)


def test_reference_constant_input_gives_constant_output():
    b = _b()
    x = np.full((300, 4), -3.25)
    out = pcen_ref.pcen(x, b)
    assert np.abs(out - out[0]).max() < 1e-14
    e = np.exp(-3.25)
    np.testing.assert_allclose(out[0], (e * (1e-6 + e) ** -0.98 + 2.0) ** 0.5 - 2.0 ** 0.5, rtol=1e-13)
    y32 = pcen_ref.pcen_f32(x, b)
    assert np.abs(y32 - out).max() < 1e-6


def test_reference_is_robust_to_gain_where_the_log_is_not():
    rng = np.random.default_rng(1)
    x = rng.standard_normal((400, 5)) - 5.0
    b = _b()
    kw = dict(gain=1.0, eps=1e-12)
    quiet, loud = pcen_ref.pcen(x, b, **kw), pcen_ref.pcen(x + np.log(100.0), b, **kw)
    assert np.log(100.0) > 4.6                                                 # what the log-mel moves by
    assert np.abs(loud - quiet).max() < 1e-6                                  # E / M does not move at all; eps is all that is left


def test_default_smoothing_coefficient():
    assert f"{pcen_ref.smoothing():.6f}" == "0.056389"
    import sed_crnn_amd as sed
    p = sed.PCEN()
    assert f"{p.smoothing(44100, 1024):.6f}" == "0.056389" and p.smoothing() == pcen_ref.smoothing()
    assert sed.PCEN(time_constant=0.1).smoothing(16000, 160) == pcen_ref.smoothing(0.1, 16000, 160)
    assert (p.gain, p.bias, p.power, p.time_constant, p.eps, p.scale) == tuple(pcen_ref.DEFAULTS[k] for k in
                                                                               ("gain", "bias", "power", "time_constant", "eps", "scale"))


def test_silence_in_the_reference_is_zero_not_nan():
    x = np.full((20, 2), -np.inf)
    assert not pcen_ref.pcen(x, _b()).any()
    assert not pcen_ref.pcen_f32(x, _b()).any()


# ───────────── the settings object and the Python argument checks ─────────────
def test_pcen_settings_refuse_bad_values():
    import dataclasses
    import sed_crnn_amd as sed
    from sed_crnn_amd import feature
    assert sed.PCEN is feature.PCEN
    for bad in (dict(gain=0.0), dict(gain=-1.0), dict(bias=-0.1), dict(power=0.0), dict(eps=0.0), dict(eps=-1e-6),
                dict(time_constant=0.0), dict(scale=0.0), dict(scale=-2.0), dict(gain=float("nan")), dict(power=float("inf")),
                dict(bias="2")):
        with pytest.raises(ValueError):
            sed.PCEN(**bad)
    p = sed.PCEN(gain=1, bias=0, power=1.0, scale=2 ** 31)                    # bias = 0 is allowed; ints become floats
    assert p.bias == 0.0 and isinstance(p.gain, float) and p == sed.PCEN(gain=1.0, bias=0.0, power=1.0, scale=2.0 ** 31)
    with pytest.raises(dataclasses.FrozenInstanceError):
        p.gain = 0.5
    with pytest.raises(ValueError):
        p.smoothing(0, 1024)
    assert hash(p) == hash(sed.PCEN(gain=1.0, bias=0.0, power=1.0, scale=2.0 ** 31))


def test_compress_argument_checks():
    import sed_crnn_amd as sed
    from sed_crnn_amd import feature
    x = np.zeros(5000, np.float32)
    for call in (lambda: feature.mbe(x, compress="pcen"), lambda: feature.mbe_many([x], compress=0.98),
                 lambda: feature.mbe_packed(None, [(0, 10)], compress=dict(gain=1.0)),
                 lambda: feature.mbe_planar(None, [(0, 10)], 1, compress=True)):
        with pytest.raises(TypeError, match="compress must be None or a PCEN"):
            call()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        feature.pcen(np.zeros((4, 40), np.float32), sed.PCEN())
    net = sed.LightningTimePooledCRNN(dropout=0.0).eval()
    with pytest.raises(TypeError, match="compress must be None or a PCEN"):
        sed.EventDetector(net, compress="pcen")
    p = sed.PCEN(gain=0.8)
    det = sed.EventDetector(net, compress=p, threshold=0.4)
    assert det.compress is p and det.with_decoder(threshold=0.7).compress is p
    assert sed.EventDetector(net).compress is None
    with pytest.raises(sed.SedHipError, match="move the module to the GPU first"):
        det(x)                                                                # valid input, model left on the CPU
    st, plain = det.stream(3), sed.EventDetector(net).stream(3)
    assert st.PW == 40 and st.state_bytes == plain.state_bytes + 3 * 40 * 2 * 4      # two floats per feed and mel column
    det2 = sed.EventDetector(sed.LightningTimePooledCRNN(dropout=0.0, in_channels=3).eval(), spatial="gcc_phat", compress=p)
    assert det2.stream(2).PW == 80 and det2.stream(2).CF == 120


# ───────────── sed_pcen's host checks ─────────────
def _call(recs, rows=100, stride=40, col0=0, W=40, state=FAKE, mu=None, inv=None, ws=None, b=0.05, x=FAKE, wsp=FAKE, gain=0.98):
    from sed_crnn_amd._lib import lib
    L = lib()
    t = np.ascontiguousarray(np.asarray(recs, np.int64).reshape(-1, 3))
    R = t.shape[0]
    ws = L.sed_pcen_workspace_bytes(rows, R, W) if ws is None else ws
    return L.sed_pcen(x, rows, stride, col0, W, C.c_void_p(t.ctypes.data), R, state, b, gain, 2.0, 0.5, 1e-6, 1.0, mu, inv, wsp, ws, None)


def test_pcen_workspace_query():
    from sed_crnn_amd._lib import lib
    L = lib()
    # tables, then block ends and carries of rows/64 + 2R blocks and the starting values of R recordings, W wide
    assert L.sed_pcen_workspace_bytes(1000, 3, 40) >= (3 + 1 + 9) * 8 + (2 * (1000 // 64 + 6) + 3) * 40 * 4
    assert L.sed_pcen_workspace_bytes(0, 0, 1) > 0
    for bad in ((-1, 1, 40), (2 ** 31, 1, 40), (100, -1, 40), (100, 2 ** 24 + 1, 40), (100, 1, 0), (100, 1, -3), (100, 1, 65537)):
        assert L.sed_pcen_workspace_bytes(*bad) == 0, bad


def test_pcen_refuses_overlapping_rows():
    assert _call([(0, 60, 0), (50, 40, 0)]) != 0
    assert "recording 1" in _err() and "overlaps" in _err()
    assert _call([(50, 40, 0), (0, 50, 0)]) != 0 and "increasing order" in _err()


def test_pcen_refuses_rows_outside_the_matrix():
    assert _call([(0, 60, 0), (60, 41, 0)]) != 0
    assert "recording 1" in _err() and "not inside the matrix of 100 rows" in _err()
    assert _call([(-1, 5, 0)]) != 0 and "not inside the matrix" in _err()
    assert _call([(0, -5, 0)]) != 0 and "not inside the matrix" in _err()
    assert _call([(101, 0, 0)]) != 0 and "not inside the matrix" in _err()


def test_pcen_refuses_a_column_range_outside_the_stride():
    assert _call([(0, 100, 0)], stride=40, col0=1, W=40, ws=1 << 20) != 0
    assert "columns [1, 1 + 40) are not inside a row of 40 floats" in _err()
    assert _call([(0, 100, 0)], col0=-1, W=4, ws=1 << 20) != 0 and "not inside a row" in _err()
    assert _call([(0, 100, 0)], W=0, ws=1 << 20) != 0 and "not inside a row" in _err()


def test_pcen_refuses_half_a_scaler():
    assert _call([(0, 100, 0)], mu=FAKE) != 0 and "both mu and inv_sigma" in _err()
    assert _call([(0, 100, 0)], inv=FAKE) != 0 and "both mu and inv_sigma" in _err()


def test_pcen_refuses_a_negative_absolute_index():
    assert _call([(0, 50, 0), (50, 50, -1)]) != 0
    assert "recording 1" in _err() and "absolute index" in _err() and "-1" in _err()


def test_pcen_refuses_a_workspace_that_is_too_small():
    from sed_crnn_amd._lib import lib
    need = lib().sed_pcen_workspace_bytes(100, 2, 40)
    assert _call([(0, 50, 0), (50, 50, 7)], ws=need - 4) != 0
    assert "workspace" in _err() and str(need) in _err()
    assert _call([(0, 50, 0)], wsp=C.c_void_p(4100)) != 0 and "8-byte aligned" in _err()


def test_pcen_refuses_the_rest():
    assert _call([(0, 50, 0)], x=None) != 0 and "null pointer" in _err()
    assert _call([(0, 50, 0), (50, 50, 7)], state=None) != 0 and "recording 1 continues at frame 7 and needs the state" in _err()
    for b in (0.0, -0.1, 1.5, float("nan")):
        assert _call([(0, 50, 0)], b=b) != 0 and "smoothing coefficient" in _err()
    for g in (0.0, -1.0, float("inf"), float("nan")):
        assert _call([(0, 50, 0)], gain=g) != 0 and "gain > 0" in _err()
    assert _call(np.zeros((0, 3)), rows=0) == 0                                # no recordings, nothing to do: no launch
    assert _call([(0, 0, 0), (100, 0, 5)], state=None) == 0                    # empty recordings only


def test_pcen_kernels_are_guarded_against_scratch():
    from sed_crnn_amd.build import NO_SCRATCH_KERNELS, SOURCES
    assert "pcen.hip" in SOURCES and set(NO_SCRATCH_KERNELS["pcen.hip"]) == {"pcen_pass_k", "pcen_carry_k"}
