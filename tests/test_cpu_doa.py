"""Per-event direction of arrival without a GPU: the steering lags against hand-worked cases and against the sign
of tdoa_ref, the grid builders, every validation error, the host-only argument checks of sed_event_doa / sed_event_doa_ring, the
build guard of doa.hip, the angle table against the log-mel blob's, and the float64 reference (tests/doa_ref.py) on synthetic
far-field sources.

The reference's own angular error, measured when this test was written (degrees; 8 sources per case, 13 frames of a white burst
with 0.2 x independent noise per channel, 44.1 kHz; ``cover`` = the grid's covering radius, doa_ref.covering_radius):
    array            grid          cover    worst error Q = 1   worst error Q = 8
    tetrahedron 6cm  ring 72        2.50         5.64                2.00
    tetrahedron 6cm  sphere 200    10.58         8.32                7.60
    tetrahedron 6cm  sphere 2562    2.80         6.69                1.91
    square 20cm      ring 72        2.50         2.00                2.00
    square 20cm      sphere 2562    2.80         5.50                2.58        (up to the mirror image in the array's plane)
On the 6 cm array the whole range is +-8 samples: at Q = 1 the steering is quantised to whole samples and the error exceeds the
grid's covering radius by up to 3.9 degrees; at Q = 8 it is within the covering radius.  A grid must be fine enough for the
aperture: with a covering radius theta the nearest direction is up to max_lag sin(theta) samples off in a pair, and a PHAT peak
is one sample wide — the 20 cm square (max_lag 26) finds nothing on sphere(200) (10.6 degrees: 4.8 samples; errors of 100+
degrees were measured), so that combination is not a case here."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import doa_ref  # noqa: E402
import spatial_ref  # noqa: E402
import tdoa_ref  # noqa: E402

SR = 44100


# ───────────── 1. steering lags ─────────────
def test_steering_lags_against_hand_worked_cases():
    import sed_crnn_amd as sed
    az = np.array([0.0, np.pi / 3, np.pi / 2, np.pi, -np.pi / 3])
    grid = sed.DirectionGrid(np.stack([np.cos(az), np.sin(az), np.zeros(5)], 1))
    tau = sed.steering_lags([[0, 0, 0], [0.343, 0, 0]], grid, 1000, c=343.0)       # 0.343 m on x at 1 kHz: one sample end to end
    assert tau.shape == (5, 1) and tau.dtype == np.float64
    np.testing.assert_allclose(tau[:, 0], np.cos(az), rtol=0, atol=1e-15)
    # three microphones: the pairs are (0,1), (0,2), (1,2) and tau is linear in the baseline
    pos = np.array([[0, 0, 0], [0.343, 0, 0], [0, 0.686, 0.343]])
    g = sed.DirectionGrid([[0, 0, 1.0], [0, 1.0, 0], [0.6, 0, 0.8]])
    np.testing.assert_allclose(sed.steering_lags(pos, g, 1000, 343.0), [[0, 1, 1], [0, 2, 2], [0.6, 0.8, 0.2]], rtol=0, atol=1e-15)
    np.testing.assert_allclose(sed.steering_lags(pos, g, 2000, 686.0), sed.steering_lags(pos, g, 1000, 343.0), rtol=0, atol=1e-15)
    tau_ref, J, ml = doa_ref.steering(pos, g.unit_vectors, 1000, 4)
    assert np.array_equal(tau_ref, sed.steering_lags(pos, g, 1000)) and ml == 3     # |r_2 - r_1| = 0.343 sqrt 6 m: ceil(2.45)
    d = sed.DOA(pos, g, oversample=4)
    assert d.max_lag(1000) == 3 and np.array_equal(d.plan(1000)[1], J) and d.plan(1000)[1].dtype == np.int32
    assert d.tdoa(1000) == sed.TDOA(3, 256)
    # round half to even: tau Q = 0.5, 1.5, 2.5 -> 0, 2, 2
    h = sed.DOA([[0, 0, 0], [0.343, 0, 0]], sed.DirectionGrid([[0.25, 0, math.sqrt(1 - 0.0625)], [0.75, 0, math.sqrt(1 - 0.5625)],
                                                            [-0.625, 0, math.sqrt(1 - 0.390625)]]), oversample=2)
    assert h.plan(1000)[1].ravel().tolist() == [0, 2, -1] and h.plan(1000)[0] == 1


def test_steering_sign_is_the_sign_of_event_tdoa():
    """a source on +x reaches the microphone at +x first: channel 1 leads, channel 0 = channel 1 delayed by 3 samples, which
    tdoa_ref (channel j delayed by n gives -n) calls lag +3; steering_lags says +3 for that direction"""
    import sed_crnn_amd as sed
    pos = np.array([[0.0, 0, 0], [3 * 0.343, 0, 0]])
    grid = sed.DirectionGrid([[1.0, 0, 0], [-1.0, 0, 0]])
    tau = sed.steering_lags(pos, grid, 1000, 343.0)
    np.testing.assert_allclose(tau[:, 0], [3.0, -3.0], rtol=0, atol=1e-12)
    x = tdoa_ref.broadband(9000, (3, 0), seed=3)                                   # channel 0 delayed by 3
    curves, _ = tdoa_ref.frame_curves(x, 1024, 8)
    assert tdoa_ref.event_tdoa(curves, [(0, 9, 4)], 1)["t"][0, 0] == 3
    y = doa_ref.far_field(9000, pos, grid.unit_vectors[0], 1000, seed=4)           # the generator agrees
    curves, _ = tdoa_ref.frame_curves(y, 1024, 8)
    assert tdoa_ref.event_tdoa(curves, [(0, 9, 4)], 1)["t"][0, 0] == 3


# ───────────── 2. grids ─────────────
def test_grid_builders():
    import sed_crnn_amd as sed
    r = sed.DirectionGrid.ring(72)
    assert len(r) == 72 and r.unit_vectors.shape == (72, 3)
    np.testing.assert_allclose(np.linalg.norm(r.unit_vectors, axis=1), 1.0, rtol=0, atol=1e-15)
    want = 2 * np.pi * np.arange(72) / 72
    np.testing.assert_allclose(np.mod(r.azimuth, 2 * np.pi), want, rtol=0, atol=1e-12)
    assert (r.azimuth > -np.pi - 1e-12).all() and (r.azimuth <= np.pi).all() and np.abs(r.elevation).max() < 1e-15
    up = sed.DirectionGrid.ring(8, elevation=0.5)
    np.testing.assert_allclose(up.elevation, 0.5, rtol=0, atol=1e-15)
    np.testing.assert_allclose(up.unit_vectors[2], [0, math.cos(0.5), math.sin(0.5)], rtol=0, atol=1e-15)
    s = sed.DirectionGrid.sphere(200)
    assert len(s) == 200
    np.testing.assert_allclose(np.linalg.norm(s.unit_vectors, axis=1), 1.0, rtol=0, atol=1e-15)
    np.testing.assert_allclose(s.unit_vectors[:, 2], 1 - (2 * np.arange(200) + 1) / 200, rtol=0, atol=1e-15)
    assert np.abs(s.unit_vectors.mean(0)).max() < 0.01                            # evenly spread: no preferred direction
    assert doa_ref.covering_radius(s.unit_vectors) < 1.2 * math.sqrt(4 * math.pi / 200)
    np.testing.assert_allclose(s.unit_vectors, np.stack([np.cos(s.elevation) * np.cos(s.azimuth), np.cos(s.elevation) * np.sin(s.azimuth),
                                                         np.sin(s.elevation)], 1), rtol=0, atol=1e-15)
    assert len(sed.DirectionGrid.sphere(16384)) == 16384 and len(sed.DirectionGrid.ring(1)) == 1
    with pytest.raises(ValueError):
        r.unit_vectors[0, 0] = 2.0                                                  # read-only


# ───────────── 3. every validation error ─────────────
def test_settings_are_validated():
    import sed_crnn_amd as sed
    ok = np.array([[1.0, 0, 0], [0, 1.0, 0]])
    for bad, what in ((np.zeros((0, 3)), "unit_vectors must be"), (np.zeros((4, 2)), "unit_vectors must be"), (np.zeros(3), "unit_vectors must be"),
                      (np.tile(ok, (8193, 1)), "unit_vectors must be"), ([[np.nan, 0, 0]], "finite"), ([[np.inf, 0, 0]], "finite"),
                      ([[1.0, 0.1, 0]], "unit norm"), ([[0.0, 0, 0]], "unit norm")):
        with pytest.raises(ValueError, match=what):
            sed.DirectionGrid(bad)
    for bad in (dict(n_az=0), dict(n_az=16385), dict(n_az=8, elevation=2.0)):
        with pytest.raises(ValueError, match="DirectionGrid.ring"):
            sed.DirectionGrid.ring(**bad)
    for bad in (0, 16385):
        with pytest.raises(ValueError, match="DirectionGrid.sphere"):
            sed.DirectionGrid.sphere(bad)
    grid, pos = sed.DirectionGrid(ok), doa_ref.tetrahedron(0.06)
    d = sed.DOA(pos, grid)
    assert (d.max_frames, d.oversample, d.c, d.channels) == (256, 8, 343.0, 4) and abs(d.aperture - 0.06) < 1e-15
    assert d.max_lag(SR) == math.ceil(0.06 * SR / 343.0) == 8 and "4 microphones" in repr(d)
    for bad, what in ((dict(positions=pos[:1]), "positions must be"), (dict(positions=np.zeros((9, 3))), "positions must be"),
                      (dict(positions=pos[:, :2]), "positions must be"), (dict(positions=pos * np.nan), "finite"),
                      (dict(positions=pos[[0, 1, 1, 2]]), "microphones 1 and 2 are at the same position"),
                      (dict(max_frames=0), "max_frames"), (dict(max_frames=2.5), "max_frames"), (dict(max_frames=True), "max_frames"),
                      (dict(oversample=3), "oversample"), (dict(oversample=32), "oversample"), (dict(oversample=0), "oversample"),
                      (dict(oversample=8.0), "oversample"), (dict(c=0.0), "speed of sound"), (dict(c=float("nan")), "speed of sound"),
                      (dict(c="fast"), "speed of sound")):
        with pytest.raises(ValueError, match=what):
            sed.DOA(**{**dict(positions=pos, grid=grid), **bad})
    with pytest.raises(TypeError, match="DirectionGrid"):
        sed.DOA(pos, ok)
    with pytest.raises(TypeError, match="DirectionGrid"):
        sed.steering_lags(pos, ok, SR)
    with pytest.raises(ValueError, match="sr > 0"):
        sed.steering_lags(pos, grid, 0)
    # the aperture: 1 m at 44.1 kHz is 129 samples, more than the 127 that are searched; at 16 kHz it is 47
    wide = sed.DOA([[0, 0, 0], [1.0, 0, 0]], grid)
    with pytest.raises(ValueError, match="aperture of 1 m is 129 samples"):
        wide.plan(SR)
    assert wide.max_lag(16000) == 47 and np.abs(wide.plan(16000)[1]).max() <= 47 * 8
    # every |J| <= max_lag Q, on a dense grid
    full = sed.DOA(doa_ref.square(0.2), sed.DirectionGrid.sphere(4000), oversample=16)
    ml, J, trig = full.plan(SR)
    assert ml == 37 and np.abs(J).max() <= ml * 16 and J.shape == (4000, 6) and trig.shape == (512 * 16 + 1, 2) and trig.dtype == np.float32


def _net(cin):
    import sed_crnn_amd as sed
    return sed.LightningTimePooledCRNN(dropout=0.0, in_channels=cin, n_mels=40).eval()


def test_detector_accepts_doa_settings_and_checks_them():
    import sed_crnn_amd as sed
    grid = sed.DirectionGrid.ring(8)
    doa = sed.DOA(doa_ref.tetrahedron(0.06), grid, max_frames=16)
    det = sed.EventDetector(_net(4), localize=doa)
    assert det.localize_settings is doa and det.locates_directions and det.localize_tdoa == sed.TDOA(8, 16)
    assert det.with_decoder(threshold=0.3).localize_settings is doa
    plain = sed.EventDetector(_net(4), localize=sed.TDOA(8, 16))
    assert not plain.locates_directions and plain.localize_tdoa == sed.TDOA(8, 16) and not sed.EventDetector(_net(4)).locates_directions
    with pytest.raises(ValueError, match="4 microphone positions, the net reads 2"):
        sed.EventDetector(_net(2), localize=doa)
    with pytest.raises(ValueError, match="aperture"):
        sed.EventDetector(_net(2), localize=sed.DOA([[0, 0, 0], [1.0, 0, 0]], grid))
    sed.EventDetector(_net(2), localize=sed.DOA([[0, 0, 0], [1.0, 0, 0]], grid), sr=16000)
    with pytest.raises(TypeError, match="TDOA"):
        sed.EventDetector(_net(4), localize=grid)
    with pytest.raises(NotImplementedError, match="live feeds"):
        det.stream(1)
    with pytest.raises(ValueError, match="holds no directions"):
        sed.DetectionResult(None, {"cls": None, "lag": None}, 0.1, None, sr=SR).doa()
    with pytest.raises(ValueError, match="hold no directions"):
        sed.StreamEvents({"cls": None}, [0, 0], [0], 0.1).doa()


def test_result_doa_maps_directions_to_angles_on_the_host():
    import torch
    import sed_crnn_amd as sed
    grid = sed.DirectionGrid.ring(4, elevation=0.25)
    ev = {"cls": torch.tensor([0, 1, 0, 1], dtype=torch.int32), "dir": torch.tensor([2, -1, 0, 3], dtype=torch.int32),
          "doa_power": torch.tensor([0.5, 0.0, 0.25, 0.125])}
    got = sed.DetectionResult(None, ev, 0.1, None, sr=SR, grid=grid).doa()
    assert got.shape == (4, 3) and np.isnan(got[1]).all()
    np.testing.assert_allclose(got[[0, 2, 3]], [[np.pi, 0.25, 0.5], [0.0, 0.25, 0.25], [-np.pi / 2, 0.25, 0.125]], rtol=0, atol=1e-12)
    assert sed.DetectionResult(None, ev, 0.1, None, sr=SR, grid=grid).doa(1).shape == (2, 3)
    st = sed.StreamEvents(ev, [0, 1, 4], [0, 0], 0.1, sr=SR, grid=grid)
    assert st.doa(1).shape == (3, 3) and np.array_equal(st.doa()[2:], got[2:])


# ───────────── 4. the C entries ─────────────
def test_c_entries_check_their_arguments_on_the_host():
    from sed_crnn_amd import _lib
    L = _lib.lib()
    for args in ((1, 2, 3, 5000, 1024, 256), (2, 4, 10, 100 * 1024, 1024, 40), (0, 2, 1, 5000, 1024, 8), (1, 9, 1, 5000, 1024, 8)):
        assert L.sed_event_doa_workspace_bytes(*args) == L.sed_event_tdoa_workspace_bytes(*args), args
    for args in ((3, 2, 3, 8192, 1024, 256), (2, 4, 10, 100 * 1024, 1024, 40), (1, 2, 1, 100, 1024, 8)):
        assert L.sed_event_doa_ring_workspace_bytes(*args) == L.sed_event_tdoa_ring_workspace_bytes(*args), args
    FAKE, blob = C.c_void_p(0x1000), (8 + 2048 + 2048 + 1028) * 4

    def call(clips=((0, 5000), (8000, 5000)), channels=2, E=1, max_lag=24, max_frames=8, ws=1 << 20, J=FAKE, D=72, Q=8, trig=FAKE, dir_=FAKE,
             power=FAKE, srp=None, pad=0):
        t = np.asarray(clips, dtype=np.int64)
        return L.sed_event_doa(FAKE, 20000, C.c_void_p(t.ctypes.data), 1, channels, FAKE, blob, None, FAKE, FAKE, FAKE, E, 1, 1024, pad,
                               max_lag, max_frames, FAKE, FAKE, FAKE, None, J, D, Q, trig, dir_, power, srp, FAKE, ws, None)

    def ring(channels=2, E=1, max_lag=24, J=FAKE, D=72, Q=8, trig=FAKE, dir_=FAKE, power=FAKE, cap=8192, hist=20):
        n = np.asarray([9000], dtype=np.int64)
        return L.sed_event_doa_ring(FAKE, 1 << 20, cap, C.c_void_p(n.ctypes.data), 1, channels, FAKE, blob, None, FAKE, FAKE, FAKE, E, 1, 1024,
                                    max_lag, 8, 10, hist, FAKE, FAKE, FAKE, None, J, D, Q, trig, dir_, power, None, FAKE, 1 << 20, None)

    def err():
        return L.sed_last_error_string().decode()
    for fn, who in ((call, "event_doa:"), (ring, "event_doa_ring:")):
        for bad, what in ((dict(J=None), "null pointer"), (dict(trig=None), "null pointer"), (dict(dir_=None), "null pointer"),
                          (dict(power=None), "null pointer"), (dict(D=0), "1 to 16384 directions"), (dict(D=16385), "1 to 16384 directions"),
                          (dict(Q=3), "oversample must be 1, 2, 4, 8 or 16"), (dict(Q=0), "oversample"), (dict(Q=32), "oversample"),
                          (dict(max_lag=0), "max_lag"), (dict(max_lag=128), "max_lag"), (dict(trig=C.c_void_p(0x1004)), "8-byte aligned"),
                          (dict(channels=1), "channels"), (dict(channels=9), "channels")):
            assert fn(**bad) != 0 and what in err() and err().startswith(who), (who, bad, err())
        assert fn(E=0) == 0                                                         # no events: nothing is launched
        assert fn(E=0, Q=16, D=16384, max_lag=127) == 0                             # the largest plan fits LDS
    # what sed_event_tdoa checks, with this entry's name
    assert call(max_frames=0) != 0 and "event_doa: max_frames" in err()
    assert call(pad=2) != 0 and "pad_mode" in err()
    assert call(clips=((0, 5000), (18000, 5000))) != 0 and "event_doa: recording 0, channel 1" in err() and "not inside the PCM buffer" in err()
    assert call(ws=32 + 1026 * 8 - 16) != 0 and "workspace" in err()
    assert ring(cap=100) != 0 and "event_doa_ring: a ring holds" in err()
    assert ring(hist=0) != 0 and "history_frames" in err()


def test_build_guards_the_steering_kernel_against_scratch():
    from sed_crnn_amd.build import EXTRA_FLAGS, NO_SCRATCH_KERNELS, SOURCES
    assert "doa.hip" in SOURCES and set(NO_SCRATCH_KERNELS["doa.hip"]) == {"doa_steer_k"}
    assert EXTRA_FLAGS["doa.hip"] == EXTRA_FLAGS["tdoa.hip"]


def test_angle_table_at_q1_is_the_log_mel_blob_table():
    """the Q = 1 bit equality of the kernel rests on this: (cos, sin)(2 pi k / 2048) of localize.trig_table are the floats of the
    blob's pairing twiddles pw[k] = (cos, -sin)"""
    import torch
    from sed_crnn_amd import feature
    from sed_crnn_amd.localize import trig_table
    blob = feature.build_tables(feature.hann_periodic(2048), feature.slaney_mel_basis(SR, 2048, 40), torch.device("cpu"))
    pw = blob.numpy().view(np.float32)[8 + 4096: 8 + 4096 + 2 * 513].reshape(513, 2)
    t = trig_table(1)
    assert t.shape == (513, 2) and np.array_equal(t[:, 0], pw[:, 0]) and np.array_equal(t[:, 1], -pw[:, 1])
    for Q in (2, 16):                                                               # every Q-th entry of a finer table is a coarser one's
        fine = trig_table(Q)
        assert fine.shape == (512 * Q + 1, 2) and np.array_equal(fine[::Q], t)
        want = 2 * np.pi * np.arange(512 * Q + 1) / (2048 * Q)
        assert np.abs(fine[:, 0] - np.cos(want)).max() <= 2.0 ** -24 and np.abs(fine[:, 1] - np.sin(want)).max() <= 2.0 ** -24


# ───────────── 5. the reference on synthetic sources ─────────────
def test_reference_fine_curve_at_q1_is_tdoa_refs_curve():
    x = tdoa_ref.broadband(9000, (0, 7, -3), seed=2)
    curves, _ = tdoa_ref.frame_curves(x, 1024, 12)
    acc = tdoa_ref.event_tdoa(curves, [(2, 6, 3)], 1)["acc"][0]
    Pk = doa_ref.whitened(x)
    np.testing.assert_allclose(doa_ref.fine_curves(Pk[2:6].sum(0), 12, 1), acc[:, 1:-1], rtol=0, atol=1e-12)
    # ... and every Q-th column of a finer curve is that curve; the columns between are the band-limited interpolation
    fine = doa_ref.fine_curves(Pk[2:6].sum(0), 12, 8)
    np.testing.assert_allclose(fine[:, ::8], acc[:, 1:-1], rtol=0, atol=1e-12)
    y32 = doa_ref.fine_curves_f32(doa_ref.whitened_f32(x)[2:6].sum(0), 12, 8)
    assert y32.dtype == np.float32 and np.abs(y32 - fine).max() < 1e-5


_RNG = np.random.default_rng(7)
IN_PLANE = [doa_ref.unit(a) for a in _RNG.uniform(0, 2 * np.pi, 8)]
ANYWHERE = _RNG.standard_normal((8, 3))
ANYWHERE = list(ANYWHERE / np.linalg.norm(ANYWHERE, axis=1, keepdims=True))
# (array, grid, sources in the array's plane, mirror) -> the measured excess over the covering radius at Q = 1 and Q = 8, degrees,
# rounded up to 0.1 (module docstring)
CASES = {("tetrahedron", "ring72"): (3.2, 0.0), ("tetrahedron", "sphere200"): (0.0, 0.0), ("tetrahedron", "sphere2562"): (3.9, 0.0),
         ("square", "ring72"): (0.0, 0.0), ("square", "sphere2562"): (2.7, 0.0)}
_ERR = {}


def _worst_error(array, gridname, Q):
    import sed_crnn_amd as sed
    key = (array, gridname, Q)
    if key not in _ERR:
        pos = doa_ref.tetrahedron(0.06) if array == "tetrahedron" else doa_ref.square(0.20)
        grid = sed.DirectionGrid.ring(72) if gridname == "ring72" else sed.DirectionGrid.sphere(int(gridname[6:]))
        sources = IN_PLANE if gridname == "ring72" else ANYWHERE
        doa = sed.DOA(pos, grid, oversample=Q)
        ml, J, _ = doa.plan(SR)
        errs = []
        for s, u in enumerate(sources):
            Pk = doa_ref.whitened(doa_ref.far_field(12 * 1024, pos, u, SR, seed=100 + s))
            r = doa_ref.event_doa(Pk, [(0, 13, 6)], 1, J.astype(np.int64), ml, Q)
            assert r["loc_frames"][0] == 13 and 0 < r["doa_power"][0] <= 1.0
            g = grid.unit_vectors[r["dir"][0]]
            e = doa_ref.angle_between(g, u)
            if array == "square" and gridname != "ring72":                          # a planar array cannot tell up from down
                e = min(e, doa_ref.angle_between(g * np.array([1.0, 1.0, -1.0]), u))
            errs.append(e)
        cover = doa_ref.covering_radius(grid.unit_vectors, in_plane=gridname == "ring72")
        _ERR[key] = (math.degrees(max(errs)), math.degrees(cover))
        print(f"{array} {gridname} Q={Q}: worst error {_ERR[key][0]:.2f} deg, covering radius {_ERR[key][1]:.2f} deg")
    return _ERR[key]


@pytest.mark.parametrize("array,gridname", sorted(CASES))
def test_reference_finds_the_synthetic_sources(array, gridname):
    for Q, excess in zip((1, 8), CASES[(array, gridname)]):
        err, cover = _worst_error(array, gridname, Q)
        assert err <= cover + excess, (array, gridname, Q, err, cover)


@pytest.mark.parametrize("gridname", ["ring72", "sphere200", "sphere2562"])
def test_oversampling_is_not_worse_on_the_small_array(gridname):
    assert _worst_error("tetrahedron", gridname, 8)[0] <= _worst_error("tetrahedron", gridname, 1)[0]
