"""The MVDR beam with its covariance taken from before the onset, the host side: the settings, the C entries'
argument checks and workspace sizes, the build guard, the detector's and the stream's rules, localize.stream_extracts against
the ring's capacity, and what the float64 reference (tests/mvdr_noise_ref.py) does on the scene the feature was made for: an
event that begins in the middle of a recording, steered with the error of a direction grid.  No GPU.

Measured with the reference (6 cm tetrahedron at 44.1 kHz unless said, event of 12 blocks, Kn = 8, G = 1, loading 1e-2;
target level out / in and output SIR, own frames | pre-onset frames):
    0 rad      -0.00 dB | 0.00 dB     10.11 dB | 15.44 dB
    0.05 rad   -3.94 dB | -0.02 dB     8.33 dB | 15.40 dB
    0.10 rad   -6.90 dB | -0.88 dB     6.65 dB | 14.55 dB
    18 cm, 0.05 rad   -8.16 dB | +0.14 dB     7.22 dB | 19.17 dB
    an event of 2 blocks, 0 rad: SIR 4.03 dB | 11.67 dB"""
import ctypes as C
import itertools
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import doa_ref  # noqa: E402
import mvdr_noise_ref  # noqa: E402
import mvdr_ref  # noqa: E402

B = 1024
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def sed():
    import sed_crnn_amd as s
    return s


def _net(cin=4):
    import sed_crnn_amd as sed
    return sed.LightningTimePooledCRNN(dropout=0.0, in_channels=cin, n_mels=40).eval()


def _doa(sed):
    return sed.DOA(doa_ref.tetrahedron(0.06), sed.DirectionGrid.ring(12), max_frames=16)


# ───────────── 1. the settings ─────────────
def test_mvdr_validates_the_noise_settings(sed):
    m = sed.MVDR()
    assert (m.loading, m.noise_blocks, m.noise_guard) == (1e-2, 0, 1) and m == sed.MVDR(1e-2, 0, 1) and hash(m) == hash(sed.MVDR(0.01, 0, 1))
    assert sed.MVDR(0.5) == sed.MVDR(loading=0.5) and sed.MVDR(0.5).noise_blocks == 0             # what they meant before
    n = sed.MVDR(noise_blocks=np.int64(8), noise_guard=np.int32(0))
    assert type(n.noise_blocks) is int and type(n.noise_guard) is int and (n.noise_blocks, n.noise_guard) == (8, 0) and n != m
    assert sed.MVDR(noise_blocks=256, noise_guard=64).noise_lead_blocks == 321 and sed.MVDR(noise_blocks=8).noise_lead_blocks == 10
    assert m.noise_lead_blocks == 0
    with pytest.raises(Exception):
        n.noise_blocks = 1                                                   # frozen
    for name in ("noise_blocks", "noise_guard"):
        most = 256 if name == "noise_blocks" else 64
        for bad in (-1, most + 1, True, False, 1.0, 8.5, "8", None, float("nan")):
            with pytest.raises(ValueError, match=f"MVDR: {name}"):
                sed.MVDR(**{name: bad})
    with pytest.raises(ValueError, match="MVDR: loading"):
        sed.MVDR(0, noise_blocks=8)


# ───────────── 2. the C entries ─────────────
def test_the_header_the_signatures_and_the_exports_agree():
    from sed_crnn_amd import _lib
    L, sig = _lib.lib(), _lib.SIGNATURES
    header = open(os.path.join(ROOT, "include", "sedcrnn.h")).read()
    for name in ("sed_event_mvdr_noise", "sed_event_mvdr_noise_ring", "sed_event_mvdr_noise_workspace_bytes",
                 "sed_event_mvdr_noise_ring_workspace_bytes"):
        assert name in sig and f" {name}(" in header and hasattr(L, name), name
    i, p = C.c_int, C.c_void_p
    for old, new in (("sed_event_mvdr", "sed_event_mvdr_noise"), ("sed_event_mvdr_ring", "sed_event_mvdr_noise_ring")):
        (res, args), (nres, nargs) = sig[old], sig[new]
        at = args.index(C.c_double) + 1                                      # the settings follow loading; the output precedes the workspace
        assert nres == res and nargs == args[:at] + [i, i] + args[at:-3] + [p] + args[-3:] and len(nargs) == len(args) + 3
        assert sig[new + "_workspace_bytes"] == (C.c_size_t, sig[old + "_workspace_bytes"][1] + [i])
        assert re.search(r"int %s\([^;]*double loading, int noise_blocks, int noise_guard, [^;]*long audio_total, int\* noise_frames_out,\s+"
                         r"void\* workspace, size_t workspace_bytes, void\* stream\);" % new, header)
    assert len(sig["sed_event_mvdr"][1]) == 27 and len(sig["sed_event_mvdr_ring"][1]) == 28      # the old entries are what they were


@pytest.mark.parametrize("Kn,slots", [(1, 1), (32, 1), (33, 2), (256, 8)])
def test_workspace_sizes(Kn, slots):
    """per event max(the own frames' chunks, ceil(Kn / 32)) chunk slots of C(C+1)/2 rows, then the C rows of w"""
    from sed_crnn_amd import _lib
    L = _lib.lib()
    row = 1026 * 8
    assert -(-Kn // 32) == slots
    for Cn in (2, 4, 8):
        T = Cn * (Cn + 1) // 2
        assert L.sed_event_mvdr_noise_workspace_bytes(1, Cn, 8, 1024, Kn) == L.sed_event_beam_workspace_bytes(1, Cn) + (slots * T + Cn) * row
        assert L.sed_event_mvdr_noise_ring_workspace_bytes(3, Cn, 8, 1024, Kn) == L.sed_event_beam_ring_workspace_bytes(3) + (slots * T + Cn) * row
    # 257 own frames are nine chunks: more than any Kn needs
    assert L.sed_event_mvdr_noise_workspace_bytes(2, 4, 256, 1024, Kn) == L.sed_event_mvdr_workspace_bytes(2, 4, 256, 1024)
    assert L.sed_event_mvdr_noise_workspace_bytes(2, 4, 12, 1024, 0) == L.sed_event_mvdr_workspace_bytes(2, 4, 12, 1024)
    for bad in ((0, 2, 8, 1024, Kn), (1, 1, 8, 1024, Kn), (1, 9, 8, 1024, Kn), (1, 2, 0, 1024, Kn), (1, 2, 8, 0, Kn), (1, 2, 8, 1024, -1),
                (1, 2, 8, 1024, 257)):
        assert L.sed_event_mvdr_noise_workspace_bytes(*bad) == 0 and L.sed_event_mvdr_noise_ring_workspace_bytes(*bad) == 0


def test_c_entries_check_their_arguments_on_the_host():
    """every refusal is made before anything is enqueued: the pointers are never followed (they point nowhere)"""
    from sed_crnn_amd import _lib
    L = _lib.lib()
    FAKE = C.c_void_p(0x1000)
    row = 1026 * 8

    def linear(clips=((0, 5000), (8000, 5000)), channels=2, E=1, tf=1, hop=1024, max_frames=8, D=72, dir_=FAKE, loc=FAKE, tau=FAKE, loading=1e-2,
               Kn=8, G=1, tables=FAKE, tables_bytes=5132 * 4, alen=FAKE, audio=FAKE, total=100, used=FAKE, ws=FAKE, ws_bytes=0, pcm=FAKE):
        t = np.asarray(clips, dtype=np.int64)
        return L.sed_event_mvdr_noise(pcm, 20000, C.c_void_p(t.ctypes.data), 1, channels, None, FAKE, FAKE, FAKE, dir_, loc, E, tf, hop,
                                      max_frames, tau, D, loading, Kn, G, tables, tables_bytes, alen, FAKE, audio, total, used, ws, ws_bytes, None)

    def ring(channels=2, E=1, hop=1024, max_frames=8, D=72, loading=1e-2, Kn=8, G=1, tables=FAKE, tb=1 << 16, alen=FAKE, audio=FAKE, total=100,
             used=FAKE, ws=FAKE, ws_bytes=0, cap=8192, n=9000, ring_=FAKE, tau=FAKE):
        t = np.asarray([n], dtype=np.int64)
        return L.sed_event_mvdr_noise_ring(ring_, 1 << 20, cap, C.c_void_p(t.ctypes.data), 1, channels, None, FAKE, FAKE, FAKE, FAKE, FAKE, E, 1,
                                           hop, max_frames, tau, D, loading, Kn, G, tables, tb, alen, FAKE, audio, total, used, ws, ws_bytes, None)

    def err():
        return L.sed_last_error_string().decode()
    for bad, what in ((dict(channels=1), "channels"), (dict(channels=9), "channels"), (dict(max_frames=0), "max_frames"), (dict(tf=0), "bad sizes"),
                      (dict(hop=0), "bad sizes"), (dict(E=-1), "bad sizes"), (dict(D=0), "at least one direction"),
                      (dict(dir_=None), "null pointer"), (dict(loc=None), "null pointer"), (dict(max_frames=1 << 22), "exceed 2^31 - 1"),
                      (dict(pcm=None), "null pointer (the samples)"), (dict(pcm=C.c_void_p(0x1002)), "4-byte aligned"),
                      (dict(clips=((0, 5000), (18000, 5000))), "not inside the PCM buffer"), (dict(clips=((0, 5000), (8000, 4000))), "equal length"),
                      (dict(loading=0.0), "loading"), (dict(loading=float("nan")), "loading"),
                      (dict(Kn=-1), "noise_blocks"), (dict(Kn=257), "noise_blocks"), (dict(G=-1), "noise_guard"), (dict(G=65), "noise_guard"),
                      (dict(used=None), "null pointer (noise_frames_out)"),
                      (dict(tau=None), "null pointer (tau"), (dict(alen=None), "null pointer (tau"),
                      (dict(audio=None), "null output buffer"), (dict(total=-1), "a total of -1"), (dict(tables=None), "table blob"),
                      (dict(tables_bytes=5128 * 4), "table blob"), (dict(ws=None), "16-byte aligned"), (dict(ws=C.c_void_p(0x1008)), "16-byte aligned"),
                      (dict(), "workspace of 0 bytes"), (dict(ws_bytes=32 + 5 * row - 1), "at least 41072 needed"),
                      (dict(Kn=33, ws_bytes=32 + 5 * row), f"at least {32 + 8 * row} needed")):        # two chunk slots of 3 rows, and w
        assert linear(**bad) != 0 and what in err() and err().startswith("mvdr_noise:"), (bad, err())
    assert linear(E=0) == 0 and linear(total=0, audio=None) == 0 and linear(E=0, used=None) == 0   # nothing is launched
    for bad, what in ((dict(channels=9), "channels"), (dict(max_frames=0), "max_frames"), (dict(hop=0), "bad sizes"), (dict(D=0), "at least one direction"),
                      (dict(ring_=None), "null pointer (the rings)"), (dict(cap=100), "a ring holds"), (dict(cap=8190), "a ring holds"),
                      (dict(cap=1 << 20), "leave the buffer"), (dict(n=-1), "samples received"), (dict(loading=0.0), "loading"),
                      (dict(Kn=257), "noise_blocks"), (dict(G=65), "noise_guard"), (dict(used=None), "null pointer (noise_frames_out)"),
                      (dict(total=-1), "a total of -1"), (dict(tau=None), "null pointer"), (dict(audio=None), "null output buffer"),
                      (dict(tables=None), "table blob"), (dict(tb=64), "table blob"), (dict(ring_=C.c_void_p(0x1002)), "4-byte aligned"),
                      (dict(), "workspace of 0 bytes")):
        assert ring(**bad) != 0 and what in err() and err().startswith("mvdr_noise_ring:"), (bad, err())
    assert ring(E=0) == 0 and ring(total=0, audio=None) == 0
    # the device compares s0 with (G + Kn + 1) B in whole blocks and 32 bits: with Kn > 0 a feed has fewer than 2^42 samples
    assert ring(hop=1 << 20, n=1 << 42) != 0 and "fewer than 2^42" in err()
    assert ring(hop=1 << 20, n=(1 << 42) - 1) != 0 and "workspace of 0 bytes" in err()
    assert ring(hop=1 << 20, n=1 << 42, Kn=0) != 0 and "workspace of 0 bytes" in err()


def test_build_guards_the_noise_kernels_against_scratch():
    from sed_crnn_amd.build import NO_SCRATCH_KERNELS
    assert {"mvdr_noise_k", "mvdr_ring_noise_k"} <= set(NO_SCRATCH_KERNELS["mvdr.hip"])
    for name in ("mvdr_noise_k", "mvdr_ring_noise_k"):                       # tests/test_cpu_mvdr_isa.py finds its kernels by substring
        assert "mvdr_cov_k" not in name and "mvdr_apply_k" not in name


# ───────────── 3. the detector and the stream ─────────────
def test_the_detector_and_the_stream_constructor(sed):
    from sed_crnn_amd.localize import stream_noise_frames
    doa = _doa(sed)
    mv = sed.MVDR(noise_blocks=8)
    det = sed.EventDetector(_net(), localize=doa, extract=mv)
    assert det.extract_settings is mv and det.with_decoder(threshold=0.3).extract_settings is mv
    with pytest.raises(ValueError, match="extract=MVDR"):
        sed.EventDetector(_net(), extract=mv)
    with pytest.raises(NotImplementedError, match="emit_audio=True"):
        det.stream(1, history_frames="min")
    own = sed.EventDetector(_net(), localize=doa, extract=sed.MVDR()).stream(3, history_frames="min", emit_audio=True)
    st = det.stream(3, history_frames="min", emit_audio=True)
    nf = stream_noise_frames(det.hop_length, 8, 1)
    assert nf == -(-10 * 1024 // det.hop_length) and own.noise_frames == 0 and st.noise_frames == nf
    assert st.lat == own.lat and own.history_frames == doa.max_frames + own.lat and st.history_frames == own.history_frames + nf
    # state_bytes grows through the larger ring alone
    assert st.cap > own.cap and st.state_bytes - own.state_bytes == 4 * 3 * 4 * (st.cap - own.cap)
    least = doa.max_frames + st.lat
    with pytest.raises(ValueError, match="less than the minimum max_frames \\+ lat"):
        det.stream(1, history_frames=least - 1, emit_audio=True)
    small = det.stream(3, history_frames=least, emit_audio=True)            # accepted: its noise events come without audio
    assert small.history_frames == least and small.cap == own.cap and small.noise_frames == nf
    assert stream_noise_frames(512, 8, 1) == 20 and stream_noise_frames(1500, 8, 1) == 7 and stream_noise_frames(1500, 0, 1) == 0
    assert stream_noise_frames(1024, 1, 0) == 2 and stream_noise_frames(1000, 33, 1) == 36
    # a result without the column has no such attribute
    import torch
    ev = {"cls": torch.zeros(2, dtype=torch.int32)}
    assert not hasattr(sed.DetectionResult(None, ev, 0.1, None), "noise_frames")
    with_col = sed.DetectionResult(None, {**ev, "noise_frames": torch.tensor([8, 0], dtype=torch.int32)}, 0.1, None)
    assert with_col.noise_frames.tolist() == [8, 0]


@pytest.mark.parametrize("hop_length", [512, 1024, 1500])
def test_stream_extracts_and_the_ring(sed, hop_length):
    """localize.stream_extracts over the grid of tests/test_cpu_stream_extract.py and (Kn, G): with the LEAST history that accepts
    an event whose weights come from before its onset, the ring of stream_ring_samples holds s0 - (G + Kn + 1) B at the least n
    the event is emitted with and at the largest (n < (b tf + lat + step_frames) hop + n_fft / 2); one frame less
    history refuses the audio and keeps the location; an event near the feed's start needs what stream_locates asks."""
    from sed_crnn_amd.localize import (event_frames, stream_extracts, stream_latency_frames, stream_locates, stream_noise_frames,
                                       stream_ring_samples)
    checked = fallbacks = 0
    for tf, seq_len, median, min_gap, MF, (Kn, G) in itertools.product((1, 4, 8), (8, 64, 256), (1, 5), (0, 3), (1, 8, 64),
                                                                        ((1, 0), (8, 1), (33, 1), (256, 64))):
        if seq_len < tf:
            continue
        lat = stream_latency_frames(tf, seq_len, median, min_gap)
        nf = stream_noise_frames(hop_length, Kn, G)
        assert (nf - 1) * hop_length < (G + Kn + 1) * B <= nf * hop_length
        for a, length, pk in ((0, 1, 0), (0, 40, 39), (3, 2, 4), (7, 100, 50), (1000, 17, 1005)):
            b = a + length
            N = b * tf + lat                                                 # the least count of final frames at emission
            n = (N - 1) * hop_length + 1024                                  # the least n the stream locates with
            f0, f1 = event_frames(a, b, pk, tf, 1 + n // hop_length, MF)
            s0 = f0 * hop_length
            base = b * tf + lat - f0                                         # the least history that locates the event
            args = (a, b, pk, tf, 1 + n // hop_length, MF, lat)
            assert stream_locates(*args, base) and not stream_locates(*args, base - 1)
            assert stream_extracts(*args, base, hop_length) and not stream_extracts(*args, base - 1, hop_length)       # Kn = 0
            if s0 < (G + Kn + 1) * B:                                        # falls back: no more history than the location needs
                assert stream_extracts(*args, base, hop_length, Kn, G) and not stream_extracts(*args, base - 1, hop_length, Kn, G)
                fallbacks += 1
                continue
            assert stream_extracts(*args, base + nf, hop_length, Kn, G) and not stream_extracts(*args, base + nf - 1, hop_length, Kn, G)
            first = s0 - (G + Kn + 1) * B
            for step_frames in (1, 4 * seq_len):
                cap = stream_ring_samples(base + nf, step_frames, hop_length, 2048)
                for n_now in (n, (N + step_frames) * hop_length + 1024 - 1):
                    assert first >= max(0, n_now - cap), (tf, seq_len, MF, Kn, G, a, b, step_frames, n_now, cap)
            checked += 1
    assert checked >= 400 and fallbacks >= 400


# ───────────── 4. the float64 reference on the scene ─────────────
@pytest.fixture(scope="module")
def table():
    rows = {(sp, err): mvdr_noise_ref.measure(sp, err) for sp, err in ((0.06, 0.0), (0.06, 0.05), (0.06, 0.10), (0.18, 0.05))}
    print("array, steering error: target level out/in own | pre-onset; output SIR own | pre-onset (dB)")
    for (sp, err), m in rows.items():
        print(f"  {sp * 100:.0f} cm, {err:.2f} rad: {m['own'][0]:+.2f} | {m['pre'][0]:+.2f}   {m['own'][1]:.2f} | {m['pre'][1]:.2f}")
    return rows


def test_the_reference_gains_sir_without_a_steering_error(table):
    """6 cm, 12 blocks, Kn = 8, G = 1: the pre-onset covariance gains at least 3 dB of output SIR over the own frames (measured
    5.3: the interferer's statistics are not diluted by the target), and the target passes as through the plain average"""
    m = table[(0.06, 0.0)]
    assert m["pre"][1] - m["own"][1] >= 3.0
    pos, xs, xi, xn = mvdr_noise_ref.onset_scene(0.06)
    tau = mvdr_noise_ref.steered(pos)
    s0, length = mvdr_noise_ref.EVENT[0] * B, 12 * B
    ys = {}
    for loading in (1e6, 1e-2):
        y, (ys[loading], yi, yn), used = mvdr_noise_ref.event(xs + xi + xn, s0, length, tau, loading, 8, 1, through=(xs, xi, xn))
        assert used == 8 and np.abs(y - (ys[loading] + yi + yn)).max() < 1e-6
    change = np.sqrt(np.mean((ys[1e-2] - ys[1e6]) ** 2) / np.mean(ys[1e6] ** 2))
    print(f"target change against loading 1e6: {change:.2e}")
    assert change < 0.05
    short = mvdr_noise_ref.measure(0.06, 0.0, blocks=2)                     # fewer frames than microphones
    print(f"2 blocks: SIR {short['own'][1]:.2f} | {short['pre'][1]:.2f} dB")
    assert short["pre"][1] - short["own"][1] >= 3.0


def test_the_reference_keeps_the_target_under_a_steering_error(table):
    """0.05 rad of azimuth error — the covering radius of the 2 562-point sphere: the own-frames beam takes the target for
    interference and removes 3.94 dB of it; the pre-onset beam has never seen the target (-0.02 dB)"""
    m = table[(0.06, 0.05)]
    assert abs(m["pre"][0]) <= 0.5 and m["own"][0] < -2.0


def test_the_noise_weights_are_distortionless_and_fall_back_on_a_silent_bin():
    rng = np.random.default_rng(5)
    x = rng.standard_normal((16 * B, 4))
    tau = rng.uniform(-4.0, 4.0, 4)
    d = mvdr_ref.steering(tau)
    for Kn, G in ((1, 0), (8, 1), (33, 1)):
        s0 = (G + Kn + 1) * B + 37
        if s0 + B > x.shape[0]:
            x = rng.standard_normal((s0 + 2 * B, 4))
        X = mvdr_noise_ref.noise_spectra(x, s0, Kn, G)
        assert X.shape == (Kn, 4, 1025)
        X[:, :, 7] = 0.0                                                     # a silent pre-onset bin
        Rn = mvdr_noise_ref.covariance(X)
        assert np.allclose(Rn, np.einsum("qck,qdk->kcd", X, X.conj()), rtol=1e-12, atol=1e-9)
        for loading in (1e-6, 1e-2, 1e2):
            w = mvdr_ref.weights(Rn, tau, loading)
            assert np.abs(np.einsum("kc,kc->k", w.conj(), d) - 1.0).max() <= 1e-12
            assert np.array_equal(w[7], d[7] / 4)


@pytest.mark.parametrize("hop", [1024, 1001, 512])
def test_an_event_too_near_the_start_is_the_own_frames_beam_exactly(hop):
    """s0 = (G + Kn + 1) B - hop falls back to mvdr_ref.event, bit for bit; s0 = (G + Kn + 1) B does not"""
    Kn, G = 8, 1
    pos = doa_ref.tetrahedron(0.06)
    x, tau = sum(mvdr_ref.scene(16 * B, pos, mvdr_noise_ref.SR)), mvdr_noise_ref.steered(pos, 0.05)
    need = (G + Kn + 1) * B
    for f32 in (False, True):
        y, _, used = mvdr_noise_ref.event(x, need - hop, 3 * B, tau, 1e-2, Kn, G, f32)
        assert used == 0 and np.array_equal(y, mvdr_ref.event(x, need - hop, 3 * B, tau, 1e-2, f32)[0])
        y, _, used = mvdr_noise_ref.event(x, need, 3 * B, tau, 1e-2, Kn, G, f32)
        assert used == Kn and not np.array_equal(y, mvdr_ref.event(x, need, 3 * B, tau, 1e-2, f32)[0])
    rows, dirs, loc = [(9, 12, 9), (10, 13, 10), (40, 41, 40)], [0, 0, -1], [3, 3, 1]
    if hop == 1024:
        out = mvdr_noise_ref.beamform(x, rows, dirs, loc, 1, hop, 12, tau[None, :], 1e-2, Kn, G)
        assert out["noise_frames"].tolist() == [0, Kn, 0] and out["noise_frames"].dtype == np.int32 and out["audio"].shape == (6 * B,)
        assert np.array_equal(out["audio"][:3 * B], mvdr_ref.event(x, 9 * B, 3 * B, tau, 1e-2)[0])
