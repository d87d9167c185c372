"""Per-event audio by an adaptive (MVDR) beam, the host side: what the float64 reference (tests/mvdr_ref.py) does to
identical channels, to a two-source scene and to an empty bin; the settings, the detector's acceptance and refusals, the C
entries' argument checks and the build guards.  No GPU."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import beam_ref  # noqa: E402
import doa_ref  # noqa: E402
import mvdr_ref  # noqa: E402

SR, HOP = 44100, 1024
SIR_MARGIN_DB = 10.0                                # what loading = 1e-2 must gain over loading = 1e6 on the two-source scene


@pytest.fixture(scope="module")
def sed():
    import sed_crnn_amd as s
    return s


# ───────────── the reference ─────────────
def test_the_reference_reproduces_equal_channels():
    """identical channels, zero delays: every w is 1/C, Y = X and the windows overlap-add to 1 — an unaligned event of 5 blocks
    and 77 samples, a single block, and one shorter than a block, each to 1e-12 (measured 1.3e-15)"""
    x = np.random.default_rng(0).standard_normal((20 * HOP, 4))
    x[:] = x[:, :1]
    for s0, length in ((3 * HOP + 5, 5 * HOP + 77), (2 * HOP, HOP), (7, 300)):
        y, _ = mvdr_ref.event(x, s0, length, np.zeros(4), 1e-2)
        assert y.shape == (length,) and np.abs(y - x[s0:s0 + length, 0]).max() <= 1e-12


def test_the_reference_suppresses_a_second_source():
    """6 cm tetrahedron at 44.1 kHz, 12 blocks, a source at (az 2.2, el 0.4) band-limited to 0.8 Nyquist, a second source at
    (az -0.7, el -0.2) 10 dB stronger, sensor noise at -30 dB (input SIR -10.0 dB).  The three go through the weights of the
    mix one by one.  Measured with this reference: output SIR -5.34 dB at loading = 1e6 (the plain steered average), +10.07 dB
    at loading = 1e-2: 15.4 dB more, of which 10 are required; the target changes by a relative RMS of 1.9e-2"""
    pos = doa_ref.tetrahedron(0.06)
    xs, xi, xn = mvdr_ref.scene(20 * HOP, pos, SR)
    tau, _ = beam_ref.delays(pos, doa_ref.unit(*mvdr_ref.TARGET)[None, :], SR, 1)
    s0, length = 4 * HOP, 12 * HOP
    sir = {}
    for loading in (1e6, 1e-2):
        y, (ys, yi, yn) = mvdr_ref.event(xs + xi + xn, s0, length, tau[0], loading, through=(xs, xi, xn))
        assert np.abs(y - (ys + yi + yn)).max() < 1e-6              # linear once the weights are fixed
        sir[loading] = mvdr_ref.db(ys, yi)
        if loading == 1e6:
            fixed = ys
    print(f"input SIR {mvdr_ref.db(xs[s0:s0 + length, 0], xi[s0:s0 + length, 0]):.2f} dB; output SIR {sir[1e6]:.2f} dB at loading 1e6, "
          f"{sir[1e-2]:.2f} dB at 1e-2; target change {np.sqrt(np.mean((ys - fixed) ** 2) / np.mean(fixed ** 2)):.2e}")
    assert sir[1e-2] - sir[1e6] >= SIR_MARGIN_DB
    assert np.sqrt(np.mean((ys - fixed) ** 2) / np.mean(fixed ** 2)) < 0.05      # distortionless: the target passes


def test_the_weights_are_distortionless_and_fall_back_on_an_empty_bin():
    rng = np.random.default_rng(3)
    for C in (2, 3, 4, 8):
        X = rng.standard_normal((6, C, 1025)) + 1j * rng.standard_normal((6, C, 1025))
        X[:, :, 7] = 0.0                                             # a bin without energy: R = 0
        R = mvdr_ref.covariance(X)
        tau = rng.uniform(-4.0, 4.0, C)
        d = mvdr_ref.steering(tau)
        for loading in (1e-6, 1e-2, 1e2, 1e6):
            w = mvdr_ref.weights(R, tau, loading)
            assert np.abs(np.einsum("kc,kc->k", w.conj(), d) - 1.0).max() <= 1e-12      # w^H d = 1
            assert np.array_equal(w[7], d[7] / C)
        assert np.abs(mvdr_ref.weights(R, tau, 1e6) - d / C).max() < 1e-5               # infinite loading: the steered average


def test_the_yardstick_is_the_same_sum_in_float32():
    pos = doa_ref.tetrahedron(0.06)
    xs, xi, xn = mvdr_ref.scene(12 * HOP, pos, SR)
    tau, _ = beam_ref.delays(pos, doa_ref.unit(*mvdr_ref.TARGET)[None, :], SR, 1)
    rows, dirs, nf = [(2, 7, 4), (9, 10, 9)], [0, 0], [5, 1]
    y = mvdr_ref.beamform(xs + xi + xn, rows, dirs, nf, 1, HOP, 12, tau, 1e-2)
    y32 = mvdr_ref.beamform(xs + xi + xn, rows, dirs, nf, 1, HOP, 12, tau, 1e-2, f32=True)
    assert y["audio"].shape == (6 * HOP,) and y32["audio"].dtype == np.float32 and y["audio_start"].tolist() == [0, 5 * HOP]
    assert 0 < np.abs(y32["audio"] - y["audio"]).max() < 1e-5


# ───────────── settings and wiring ─────────────
def test_mvdr_validation(sed):
    m = sed.MVDR()
    assert m.loading == 1e-2 and m == sed.MVDR(0.01) and hash(m) == hash(sed.MVDR(1e-2)) and isinstance(sed.MVDR(1).loading, float)
    assert sed.MVDR(1e-6).loading == 1e-6 and sed.MVDR(np.float32(1e6)).loading == 1e6
    with pytest.raises(Exception):
        m.loading = 1.0                                              # frozen
    for bad in (0, 9e-7, 1.1e6, -1.0, float("nan"), float("inf"), "1e-2", None, True):
        with pytest.raises(ValueError, match="loading"):
            sed.MVDR(bad)
    from sed_crnn_amd.localize import mvdr_window
    w = mvdr_window()
    assert w.dtype == np.float32 and w.shape == (2048,) and not w.flags.writeable
    assert np.array_equal(w, mvdr_ref.window(f32=True)) and w[0] == 0.0 and w[1024] == 1.0
    assert np.abs(mvdr_ref.window()[:1024] ** 2 + mvdr_ref.window()[1024:] ** 2 - 1.0).max() < 1e-15


def test_the_steering_table(sed):
    grid = sed.DirectionGrid.sphere(50)
    doa = sed.DOA(doa_ref.tetrahedron(0.06), grid)
    t = doa.steering(SR)
    assert t.dtype == np.float64 and t.shape == (50, 4) and t.flags.c_contiguous and doa.steering(SR) is t
    assert np.array_equal(t, sed.steering_delays(doa.positions, grid, SR)) and np.array_equal(np.rint(t * 16).astype(np.int32), doa.delays(SR, 16))


def _net(cin):
    import sed_crnn_amd as sed
    return sed.LightningTimePooledCRNN(dropout=0.0, in_channels=cin, n_mels=40).eval()


def test_detector_takes_an_mvdr_only_with_a_doa(sed):
    doa = sed.DOA(doa_ref.tetrahedron(0.06), sed.DirectionGrid.ring(12), max_frames=16)
    mv = sed.MVDR(0.1)
    det = sed.EventDetector(_net(4), localize=doa, extract=mv)
    assert det.extract_settings is mv and det.with_decoder(threshold=0.3).extract_settings is mv
    assert isinstance(sed.EventDetector(_net(4), localize=doa, extract=sed.DelaySum(8, 8)).extract_settings, sed.DelaySum)
    with pytest.raises(ValueError, match="extract=MVDR"):
        sed.EventDetector(_net(4), extract=mv)
    with pytest.raises(ValueError, match="extract=MVDR"):
        sed.EventDetector(_net(4), localize=sed.TDOA(8, 16), extract=mv)
    with pytest.raises(ValueError, match="extract=DelaySum"):
        sed.EventDetector(_net(4), extract=sed.DelaySum())
    with pytest.raises(TypeError, match="DelaySum"):
        sed.EventDetector(_net(4), localize=doa, extract=1e-2)
    with pytest.raises(NotImplementedError, match="extract"):
        det.stream(1, history_frames="min")


def test_event_mvdr_checks_its_settings_before_the_device(sed):
    """(the PCM check comes first: without a GPU there is nothing else to reach)"""
    from sed_crnn_amd import feature
    with pytest.raises(RuntimeError, match="event_mvdr needs a 1-D CUDA"):
        feature.event_mvdr(np.zeros(8, np.float32), [(0, 4), (4, 4)], 2, {}, 1, None, sed.MVDR())


# ───────────── the C entries ─────────────
def test_c_entries_check_their_arguments_on_the_host():
    """every refusal is made before anything is enqueued: the pointers are never followed (they point nowhere)"""
    import ctypes as C
    from sed_crnn_amd import _lib
    L = _lib.lib()
    row = 1026 * 8
    assert L.sed_event_mvdr_workspace_bytes(1, 2, 8, 1024) == 32 + (1 * 3 + 2) * row              # 9 frames: one chunk
    assert L.sed_event_mvdr_workspace_bytes(2, 4, 256, 1024) == 80 + (9 * 10 + 4) * row           # 257 frames: nine chunks
    assert L.sed_event_mvdr_workspace_bytes(1, 8, 31, 1024) == 80 + (1 * 36 + 8) * row            # 32 frames
    assert L.sed_event_mvdr_workspace_bytes(1, 8, 32, 1024) == 80 + (2 * 36 + 8) * row            # 33 frames
    assert L.sed_event_mvdr_workspace_bytes(1, 2, 3, 512) == 32 + 5 * row                         # 1536 samples: 2 blocks, 3 frames
    for bad in ((0, 2, 8, 1024), (1, 1, 8, 1024), (1, 9, 8, 1024), (1, 2, 0, 1024), (1, 2, 8, 0), (1, 2, 1 << 22, 1024)):
        assert L.sed_event_mvdr_workspace_bytes(*bad) == 0
    FAKE = C.c_void_p(0x1000)

    def mvdr(clips=((0, 5000), (8000, 5000)), channels=2, E=1, tf=1, hop=1024, max_frames=8, D=72, dir_=FAKE, loc=FAKE, tau=FAKE, loading=1e-2,
             tables=FAKE, tables_bytes=5132 * 4, alen=FAKE, audio=FAKE, total=100, ws=FAKE, ws_bytes=0, pcm=FAKE):
        t = np.asarray(clips, dtype=np.int64)
        return L.sed_event_mvdr(pcm, 20000, C.c_void_p(t.ctypes.data), 1, channels, None, FAKE, FAKE, FAKE, dir_, loc, E, tf, hop, max_frames,
                                tau, D, loading, tables, tables_bytes, alen, FAKE, audio, total, ws, ws_bytes, None)

    def err():
        return L.sed_last_error_string().decode()
    for bad, what in ((dict(channels=1), "channels"), (dict(channels=9), "channels"), (dict(max_frames=0), "max_frames"), (dict(tf=0), "bad sizes"),
                      (dict(hop=0), "bad sizes"), (dict(E=-1), "bad sizes"), (dict(D=0), "at least one direction"),
                      (dict(dir_=None), "null pointer"), (dict(loc=None), "null pointer"), (dict(max_frames=1 << 22), "exceed 2^31 - 1"),
                      (dict(pcm=None), "null pointer (the samples)"), (dict(pcm=C.c_void_p(0x1002)), "4-byte aligned"),
                      (dict(clips=((0, 5000), (18000, 5000))), "not inside the PCM buffer"), (dict(clips=((0, 5000), (8000, 4000))), "equal length"),
                      (dict(loading=0.0), "loading"), (dict(loading=9e-7), "loading"), (dict(loading=2e6), "loading"),
                      (dict(loading=float("nan")), "loading"), (dict(tau=None), "null pointer (tau"), (dict(alen=None), "null pointer (tau"),
                      (dict(audio=None), "null output buffer"), (dict(total=-1), "a total of -1"), (dict(tables=None), "table blob"),
                      (dict(tables_bytes=5128 * 4), "table blob"), (dict(tables_bytes=5132 * 4 + 8), "table blob"),
                      (dict(ws=None), "16-byte aligned"), (dict(ws=C.c_void_p(0x1008)), "16-byte aligned"),
                      (dict(), "workspace of 0 bytes"), (dict(ws_bytes=32 + 5 * 1026 * 8 - 1), "at least 41072 needed")):
        assert mvdr(**bad) != 0 and what in err() and err().startswith("mvdr:"), (bad, err())
    assert mvdr(E=0) == 0 and mvdr(total=0, audio=None) == 0             # no events, or nothing to extract: nothing is launched


def test_the_header_the_signatures_and_the_exports_agree(sed):
    from sed_crnn_amd import _lib
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "sedcrnn.h")).read()
    for name in ("sed_event_mvdr", "sed_event_mvdr_workspace_bytes"):
        assert name in _lib.SIGNATURES and f" {name}(" in header and hasattr(_lib.lib(), name)
    assert len(_lib.SIGNATURES["sed_event_mvdr"][1]) == 27 and sed.MVDR is __import__("sed_crnn_amd.localize").localize.MVDR


def test_build_guards_the_mvdr_kernels_against_scratch():
    from sed_crnn_amd.build import EXTRA_FLAGS, NO_SCRATCH_KERNELS, SOURCES
    assert "mvdr.hip" in SOURCES and {"mvdr_cov_k", "mvdr_apply_k"} <= set(NO_SCRATCH_KERNELS["mvdr.hip"])
    assert {"-fno-slp-vectorize", "-Rpass-analysis=kernel-resource-usage"} <= set(EXTRA_FLAGS["mvdr.hip"])
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "sed_crnn_amd", "csrc", "mvdr.hip")).read()
    import re
    kernels = set(re.findall(r"__global__[^\n]*?void (\w+)\(", src))
    assert kernels == set(NO_SCRATCH_KERNELS["mvdr.hip"])            # every kernel of the file is guarded: a new one has to be listed
