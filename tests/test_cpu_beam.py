"""Per-event audio by a steered delay-and-sum beam, the host side: the settings, the filter, the delays, the sample
rule, and what the float64 reference (tests/beam_ref.py) does to a synthetic source and to noise.  No GPU."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import beam_ref  # noqa: E402
import doa_ref  # noqa: E402

SR, HOP = 44100, 1024


@pytest.fixture(scope="module")
def sed():
    import sed_crnn_amd as s
    return s


def test_delaysum_validation(sed):
    d = sed.DelaySum()
    assert (d.oversample, d.half_width, d.beta) == (16, 16, 10.0) and d == sed.DelaySum(np.int64(16), 16, 10)
    assert isinstance(sed.DelaySum(beta=3).beta, float) and hash(d) == hash(sed.DelaySum())
    with pytest.raises(Exception):
        d.oversample = 8                                                  # frozen
    for Q in (1, 2, 4, 8, 16, 32, 64):
        assert sed.DelaySum(oversample=Q).oversample == Q
    for bad in (0, 3, 128, -1, 2.0, True, "8"):
        with pytest.raises(ValueError, match="oversample"):
            sed.DelaySum(oversample=bad)
    assert sed.DelaySum(half_width=1).half_width == 1 and sed.DelaySum(half_width=32).half_width == 32
    for bad in (0, 33, -4, 1.5, True):
        with pytest.raises(ValueError, match="half_width"):
            sed.DelaySum(half_width=bad)
    assert sed.DelaySum(beta=0).beta == 0.0
    for bad in (-0.1, float("nan"), float("inf"), "10", None, True):
        with pytest.raises(ValueError, match="beta"):
            sed.DelaySum(beta=bad)


@pytest.mark.parametrize("Q,H,beta", [(1, 1, 10.0), (4, 4, 6.0), (16, 16, 10.0), (64, 32, 10.0), (8, 3, 0.0)])
def test_taps(sed, Q, H, beta):
    t = sed.DelaySum(Q, H, beta).taps
    want32, want64 = beam_ref.taps(Q, H, beta)
    assert t.dtype == np.float32 and t.shape == (Q, 2 * H) and not t.flags.writeable
    assert np.array_equal(t.view(np.int32), want32.view(np.int32))
    impulse = np.zeros(2 * H, np.float32)
    impulse[H - 1] = 1.0
    assert np.array_equal(t[0], impulse)                                  # row 0 is the exact unit impulse
    assert np.abs(want64.sum(1) - 1.0).max() <= 4 * np.finfo(np.float64).eps          # unit float64 sum before the rounding
    assert np.abs(t.astype(np.float64).sum(1) - 1.0).max() <= 2 * H * 2.0 ** -24
    from sed_crnn_amd.resample import design_taps
    raw = design_taps(Q, H, 1.0, beta)
    assert np.allclose(want64[1:] * raw[1:].sum(1, keepdims=True), raw[1:], rtol=1e-14, atol=0)


@pytest.mark.parametrize("C,Q", [(2, 1), (3, 4), (4, 16), (8, 64)])
def test_delays(sed, C, Q):
    pos = {2: doa_ref.line(2, 0.06), 3: doa_ref.line(3, 0.04), 4: doa_ref.tetrahedron(0.06), 8: doa_ref.line(8, 0.012)}[C]
    grid = sed.DirectionGrid.sphere(200)
    doa = sed.DOA(pos, grid, oversample=8)
    M = doa.delays(SR, Q)
    tau, want = beam_ref.delays(pos, grid.unit_vectors, SR, Q)
    assert M.dtype == np.int32 and M.shape == (200, C) and np.array_equal(M, want) and doa.delays(SR, Q) is M
    assert np.allclose(sed.steering_delays(pos, grid, SR), tau, rtol=0, atol=1e-12)
    assert np.abs(tau.sum(1)).max() < 1e-9                                # the delays of a direction sum to 0 ...
    assert np.abs(M.sum(1)).max() <= C / 2                                # ... and so, within the rounding, do the integers
    assert np.abs(M).max() <= doa.max_lag(SR) * Q
    ml, J, _ = doa.plan(SR)
    pairs = [(i, j) for i in range(C) for j in range(i + 1, C)]
    lags = sed.steering_lags(pos, grid, SR)
    for p, (i, j) in enumerate(pairs):                                    # tau_j - tau_i is the pair's lag
        assert np.abs((tau[:, j] - tau[:, i]) - lags[:, p]).max() < 1e-9
        assert np.abs((M[:, j] - M[:, i]) - J[:, p] * (Q / doa.oversample)).max() <= 1 + 0.5 * Q / doa.oversample


def test_event_samples_on_the_edge_rows(sed):
    n, mf = beam_ref.EDGE_FRAMES * HOP, beam_ref.EDGE_MAX_FRAMES
    got = []
    for (on, off, pk), rec, located in beam_ref.EDGE_ROWS:
        f0, f1 = sed.event_frames(on, off, pk, 1, 1 + n // HOP, mf) if rec == 0 else (0, 0)
        d = 3 if located else -1
        s0, s1 = sed.event_samples(on, off, pk, 1, n, HOP, mf, d, f1 - f0)
        got.append((s0, s1))
        if located and f0 * HOP < n:
            assert (s0, s1) == (f0 * HOP, min(f1 * HOP, n)) and s1 > s0
        else:                                                             # not extracted, or (row 11) a frame that starts at sample n
            assert (s0, s1) == (0, 0)
    assert got[:5] == [(3 * HOP, 4 * HOP), (10 * HOP, 15 * HOP), (14 * HOP, 26 * HOP), (0, 3 * HOP), (38 * HOP, 40 * HOP)]
    assert got[11] == (0, 0) and sed.event_frames(40, 41, 40, 1, 41, mf) == (40, 41)   # located on frame 40, which starts at sample n
    assert sed.event_samples(40, 41, 40, 1, n, HOP, mf, 0, 1) == (0, 0)
    assert sed.event_samples(40, 41, 40, 1, n + 5, HOP, mf, 0, 1) == (40 * HOP, n + 5)
    assert sed.event_samples(3, 9, 5, 1, n, HOP, mf, 0, 2) == (3 * HOP, 5 * HOP)       # fewer frames than the range: as located
    assert sed.event_samples(3, 9, 5, 1, n, HOP, mf, 0, 99) == (3 * HOP, 9 * HOP)      # never more than the range
    assert sed.event_samples(3, 9, 5, 2, n, HOP, mf, 0, 12) == (6 * HOP, 18 * HOP)
    s0, lens, starts = beam_ref.spans([r for r, _, _ in beam_ref.EDGE_ROWS], [3 if ok else -1 for _, _, ok in beam_ref.EDGE_ROWS],
                                      [sed.event_frames(*r, 1, 41, mf)[1] - sed.event_frames(*r, 1, 41, mf)[0] if rec == 0 else 0
                                       for r, rec, _ in beam_ref.EDGE_ROWS], 1, n, HOP, mf)
    assert [(int(a), int(a + b)) if b else (0, 0) for a, b in zip(s0, lens)] == got
    assert np.array_equal(starts, np.concatenate([[0], np.cumsum(lens)[:-1]]))
    with pytest.raises(ValueError):
        sed.event_samples(0, 1, 0, 1, n, 0, mf, 0, 1)


def test_the_reference_points(sed):
    """6 cm tetrahedron, a source band-limited to 0.8 Nyquist from a direction that is a grid row, Q = 16, H = 16, beta = 10: the
    float64 reference reproduces the source to a relative RMS error of 1.3e-4 (bound 5e-4) and brings independent white noise
    in 4 channels to 0.235 of its power (bounds 0.2 .. 0.27; 0.25 is the plain average, the fractional-delay filters take the
    rest near Nyquist)"""
    pos, u = doa_ref.tetrahedron(0.06), doa_ref.unit(2.2, 0.4)
    Q, H = 16, 16
    tap32, _ = beam_ref.taps(Q, H, 10.0)
    _, M = beam_ref.delays(pos, u[None, :], SR, Q)
    assert np.abs(M).max() > Q                                            # more than a sample: a real steering
    n = 40 * HOP
    rows, dirs, nf = [(4, 16, 10)], [0], [12]
    x, s = beam_ref.source(n, pos, u, SR, seed=5, band=0.8)
    y = beam_ref.beamform(x, rows, dirs, nf, 1, HOP, 12, M, tap32, Q)["audio"]
    want = s[4 * HOP: 16 * HOP]
    err = np.sqrt(np.mean((y - want) ** 2) / np.mean(want ** 2))
    print(f"source: relative RMS error {err:.3g}")
    assert err <= 5e-4
    one = np.sqrt(np.mean((x[4 * HOP: 16 * HOP, 0] - want) ** 2) / np.mean(want ** 2))
    assert one > 0.1                                                      # (a single channel is not the source: it is delayed)
    w = (0.3 * np.random.default_rng(6).standard_normal((n, 4))).astype(np.float32)
    yn = beam_ref.beamform(w, rows, dirs, nf, 1, HOP, 12, M, tap32, Q)["audio"]
    ratio = np.mean(yn ** 2) / np.mean(w[4 * HOP: 16 * HOP].astype(np.float64) ** 2)
    print(f"noise: power ratio {ratio:.3g}")
    assert 0.2 <= ratio <= 0.27
    y32 = beam_ref.beamform(x, rows, dirs, nf, 1, HOP, 12, M, tap32, Q, f32=True)["audio"]
    assert y32.dtype == np.float32 and 0 < np.abs(y32 - y).max() < 1e-5   # the yardstick is the same sum, in float32


def _net(cin):
    import sed_crnn_amd as sed
    return sed.LightningTimePooledCRNN(dropout=0.0, in_channels=cin, n_mels=40).eval()


def test_detector_takes_extract_only_with_a_doa(sed):
    grid = sed.DirectionGrid.ring(12)
    doa = sed.DOA(doa_ref.tetrahedron(0.06), grid, max_frames=16)
    beam = sed.DelaySum(8, 8)
    det = sed.EventDetector(_net(4), localize=doa, extract=beam)
    assert det.extract_settings is beam and det.with_decoder(threshold=0.3).extract_settings is beam
    assert sed.EventDetector(_net(4), localize=doa).extract_settings is None
    with pytest.raises(ValueError, match="extract=DelaySum"):
        sed.EventDetector(_net(4), extract=beam)
    with pytest.raises(ValueError, match="extract=DelaySum"):
        sed.EventDetector(_net(4), localize=sed.TDOA(8, 16), extract=beam)
    with pytest.raises(TypeError, match="DelaySum"):
        sed.EventDetector(_net(4), localize=doa, extract=doa)
    with pytest.raises(NotImplementedError, match="extract"):
        det.stream(1, history_frames="min")


def test_c_entries_check_their_arguments_on_the_host():
    """every refusal is made before anything is enqueued: the pointers are never followed (they point nowhere)"""
    import ctypes as C
    from sed_crnn_amd import _lib
    L = _lib.lib()
    assert L.sed_event_beam_workspace_bytes(1, 2) == 32 and L.sed_event_beam_workspace_bytes(2, 4) == 80
    assert L.sed_event_beam_workspace_bytes(0, 2) == 0 and L.sed_event_beam_workspace_bytes(1, 9) == 0 and L.sed_event_beam_workspace_bytes(1, 1) == 0
    assert L.sed_event_beam_ring_workspace_bytes(3) == 32 and L.sed_event_beam_ring_workspace_bytes(0) == 0
    FAKE = C.c_void_p(0x1000)

    def clips_of(clips):
        t = np.asarray(clips, dtype=np.int64)
        return t, C.c_void_p(t.ctypes.data)

    def spans(clips=((0, 5000), (8000, 5000)), channels=2, E=1, tf=1, hop=1024, max_frames=8, D=72, dir_=FAKE, loc=FAKE, out=FAKE, total=FAKE, ws=0):
        t, p = clips_of(clips)
        return L.sed_event_beam_spans(20000, p, 1, channels, None, FAKE, FAKE, FAKE, dir_, loc, E, tf, hop, max_frames, D, out, FAKE, total,
                                      FAKE, ws, None)

    def spans_ring(channels=2, E=1, tf=1, hop=1024, max_frames=8, D=72, dir_=FAKE, loc=FAKE, out=FAKE, total=FAKE, ws=0, n=9000):
        t = np.asarray([n], dtype=np.int64)
        return L.sed_event_beam_spans_ring(C.c_void_p(t.ctypes.data), 1, channels, None, FAKE, FAKE, FAKE, dir_, loc, E, tf, hop, max_frames, D,
                                           out, FAKE, total, FAKE, ws, None)

    def beam(clips=((0, 5000), (8000, 5000)), channels=2, E=1, tf=1, hop=1024, max_frames=8, D=72, dir_=FAKE, loc=FAKE, M=FAKE, Q=16, H=16,
             taps=FAKE, alen=FAKE, audio=FAKE, total=100, ws=0, pcm=FAKE):
        t, p = clips_of(clips)
        return L.sed_event_beamform(pcm, 20000, p, 1, channels, None, FAKE, FAKE, FAKE, dir_, loc, E, tf, hop, max_frames, M, D, Q, H, taps,
                                    alen, FAKE, audio, total, FAKE, ws, None)

    def beam_ring(channels=2, E=1, tf=1, hop=1024, max_frames=8, D=72, dir_=FAKE, loc=FAKE, M=FAKE, Q=16, H=16, taps=FAKE, alen=FAKE,
                  audio=FAKE, total=100, ws=0, cap=8192, n=9000, pcm=FAKE):
        t = np.asarray([n], dtype=np.int64)
        return L.sed_event_beamform_ring(pcm, 1 << 20, cap, C.c_void_p(t.ctypes.data), 1, channels, None, FAKE, FAKE, FAKE, dir_, loc, E, tf, hop,
                                         max_frames, M, D, Q, H, taps, alen, FAKE, audio, total, FAKE, ws, None)

    def err():
        return L.sed_last_error_string().decode()
    shared = ((dict(channels=1), "channels"), (dict(channels=9), "channels"), (dict(max_frames=0), "max_frames"), (dict(tf=0), "bad sizes"),
              (dict(hop=0), "bad sizes"), (dict(E=-1), "bad sizes"), (dict(D=0), "at least one direction"), (dict(dir_=None), "null pointer"),
              (dict(loc=None), "null pointer"), (dict(max_frames=1 << 22, hop=1024), "exceed 2^31 - 1"), (dict(), "workspace of 0 bytes"))
    for fn, who in ((spans, "event_beam_spans:"), (spans_ring, "event_beam_spans_ring:"), (beam, "event_beamform:"),
                    (beam_ring, "event_beamform_ring:")):
        for bad, what in shared:
            assert fn(**bad) != 0 and what in err() and err().startswith(who), (who, bad, err())
    for fn in (spans, spans_ring):
        assert fn(out=None) != 0 and "null pointer (an output)" in err()
        assert fn(total=None) != 0 and "null pointer (an output)" in err()
    for fn, who in ((beam, "event_beamform:"), (beam_ring, "event_beamform_ring:")):
        for bad, what in ((dict(Q=3), "oversample"), (dict(Q=0), "oversample"), (dict(Q=128), "oversample"), (dict(H=0), "half_width"),
                          (dict(H=33), "half_width"), (dict(M=None), "null pointer"), (dict(taps=None), "null pointer"),
                          (dict(alen=None), "null pointer"), (dict(audio=None), "null output buffer"), (dict(total=-1), "a total of -1"),
                          (dict(pcm=C.c_void_p(0x1004)), "16-byte aligned"), (dict(pcm=None), "null pointer")):
            assert fn(**bad) != 0 and what in err() and err().startswith(who), (who, bad, err())
        assert fn(E=0) == 0 and fn(total=0, audio=None) == 0              # no events, or nothing to extract: nothing is launched
    for fn in (spans, beam):
        assert fn(clips=((0, 5000), (18000, 5000))) != 0 and "recording 0, channel 1" in err() and "not inside the PCM buffer" in err()
        assert fn(clips=((0, 5000), (8000, 4000))) != 0 and "equal length" in err()
    for fn in (spans_ring, beam_ring):
        assert fn(n=-1) != 0 and "samples received" in err()
    assert beam_ring(cap=100) != 0 and "event_beamform_ring: a ring holds" in err()
    assert beam_ring(cap=1 << 20) != 0 and "leave the buffer" in err()


def test_build_guards_the_beam_kernels_against_scratch():
    from sed_crnn_amd.build import EXTRA_FLAGS, NO_SCRATCH_KERNELS, SOURCES
    assert "beam.hip" in SOURCES and set(NO_SCRATCH_KERNELS["beam.hip"]) == {"beam_sum_k", "beam_spans_k"}
    assert "-Rpass-analysis=kernel-resource-usage" in EXTRA_FLAGS["beam.hip"]


def test_results_hand_out_the_audio_of_an_event():
    import torch
    import sed_crnn_amd as sed
    ev = {"cls": torch.tensor([0, 1, 0], dtype=torch.int32), "audio_start": torch.tensor([0, 4, 4]), "audio_len": torch.tensor([4, 0, 3], dtype=torch.int32)}
    audio = torch.arange(7.0)
    r = sed.DetectionResult(None, ev, 0.1, None, sr=SR, audio=audio)
    assert r.event_audio(0).tolist() == [0, 1, 2, 3] and r.event_audio(1).numel() == 0 and r.event_audio(-1).tolist() == [4, 5, 6]
    assert r.event_audio(2).data_ptr() == audio[4:].data_ptr()             # a slice, not a copy
    with pytest.raises(IndexError):
        r.event_audio(3)
    with pytest.raises(ValueError, match="holds no audio"):
        sed.DetectionResult(None, ev, 0.1, None, sr=SR).event_audio(0)
    with pytest.raises(ValueError, match="holds no audio"):
        sed.DetectionResult(None, {"cls": ev["cls"]}, 0.1, None, audio=audio).event_audio(0)
