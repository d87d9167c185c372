"""Live feeds emit each located event's audio, the host side: the constructor's rules, the merge of the steps of one
push, the margins the proof of bit equality rests on, and the two new C entries' signatures.  No GPU."""
import ctypes as C
import itertools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import doa_ref  # noqa: E402

SR, HOP, NFFT = 44100, 1024, 2048
BEAM_REACH = 32 + 127 + 1            # half_width <= 32 taps and |delay| <= 127 samples either side of an output sample, rounded up


@pytest.fixture(scope="module")
def sed():
    import sed_crnn_amd as s
    return s


def _net(cin=4):
    import sed_crnn_amd as sed
    return sed.LightningTimePooledCRNN(dropout=0.0, in_channels=cin, n_mels=40).eval()


def _doa(sed):
    return sed.DOA(doa_ref.tetrahedron(0.06), sed.DirectionGrid.ring(12), max_frames=16)


# ───────────── 1. the constructor ─────────────
def test_emit_audio_needs_a_detector_that_extracts(sed):
    det = sed.EventDetector(_net(), localize=_doa(sed))
    with pytest.raises(ValueError, match="emit_audio"):
        det.stream(1, history_frames="min", emit_audio=True)
    with pytest.raises(ValueError, match="emit_audio"):
        sed.StreamDetector(_net(), 1, localize=_doa(sed), history_frames="min", emit_audio=True)
    with pytest.raises(ValueError, match="emit_audio"):
        sed.EventDetector(_net()).stream(1, emit_audio=True)


@pytest.mark.parametrize("beam", ["DelaySum", "MVDR"])
def test_an_extracting_detector_streams_only_with_emit_audio(sed, beam):
    det = sed.EventDetector(_net(), localize=_doa(sed), extract=getattr(sed, beam)())
    for kw in (dict(history_frames="min"), dict(), dict(history_frames="min", emit_audio=False)):
        with pytest.raises(NotImplementedError, match="extract") as e:
            det.stream(1, **kw)
        assert "emit_audio=True" in str(e.value)
    with pytest.raises(NotImplementedError, match="live feeds"):             # the ring comes first, as for any localising stream
        det.stream(1, emit_audio=True)


@pytest.mark.parametrize("beam", ["DelaySum", "MVDR"])
def test_emit_audio_constructs_and_holds_no_more_state(sed, beam):
    doa = _doa(sed)
    det = sed.EventDetector(_net(), localize=doa, extract=getattr(sed, beam)())
    st = det.stream(3, history_frames="min", emit_audio=True)
    plain = sed.EventDetector(_net(), localize=doa).stream(3, history_frames="min")
    assert st.emit_audio and not plain.emit_audio
    assert st.state_bytes == plain.state_bytes and st.cap == plain.cap and st.lat == plain.lat
    st2 = sed.StreamDetector(_net(), 3, localize=doa, extract=getattr(sed, beam)(), history_frames="min", emit_audio=True)
    assert st2.state_bytes == plain.state_bytes


# ───────────── 2. the steps of one push ─────────────
def _slices_cover(start, length, total):
    """the slices [start, start + length) with length > 0 are disjoint and cover [0, total)"""
    iv = sorted((int(s), int(s) + int(n)) for s, n in zip(start, length) if n > 0)
    at = 0
    for a, b in iv:
        if a != at:
            return False
        at = b
    return at == total and all(0 <= int(s) <= total for s in start)


def test_merge_step_audio_offsets_every_step_by_the_running_total(sed):
    from sed_crnn_amd.stream import merge_step_audio
    i64, i32 = torch.int64, torch.int32
    parts = [(torch.arange(0.0, 7.0), torch.tensor([0, 4, 4], dtype=i64), torch.tensor([4, 0, 3], dtype=i32)),
             (torch.empty(0), torch.tensor([0], dtype=i64), torch.tensor([0], dtype=i32)),                      # a step that located nothing
             (torch.arange(100.0, 105.0), torch.tensor([3, 0], dtype=i64), torch.tensor([2, 3], dtype=i32)),    # (not in order of start)
             (torch.empty(0), torch.empty(0, dtype=i64), torch.empty(0, dtype=i32)),                            # a step without events
             (torch.arange(200.0, 201.0), torch.tensor([0, 1], dtype=i64), torch.tensor([1, 0], dtype=i32))]
    audio, start, length = merge_step_audio(parts)
    assert audio.dtype == torch.float32 and start.dtype == i64 and length.dtype == i32
    assert start.tolist() == [0, 4, 4, 7, 10, 7, 12, 13] and length.tolist() == [4, 0, 3, 0, 2, 3, 1, 0]
    assert audio.tolist() == list(range(7)) + list(range(100, 105)) + [200.0]
    assert _slices_cover(start, length, audio.numel())
    at = 0
    for a, s, n in parts:                                                    # every event keeps its samples
        for e in range(len(s)):
            got = audio[int(start[at]):int(start[at]) + int(length[at])]
            assert torch.equal(got, a[int(s[e]):int(s[e]) + int(n[e])])
            at += 1
    one = merge_step_audio(parts[:1])
    assert all(torch.equal(x, y) for x, y in zip(one, parts[0]))
    # through StreamEvents: the shared accessor and its error text
    ev = {"cls": torch.zeros(8, dtype=i32), "audio_start": start, "audio_len": length}
    o = sed.stream.StreamEvents(ev, [0, 8], [0], 0.1, audio=audio)
    assert o.event_audio(4).tolist() == [103.0, 104.0] and o.event_audio(1).numel() == 0 and o.event_audio(-2).tolist() == [200.0]
    with pytest.raises(IndexError):
        o.event_audio(8)
    with pytest.raises(ValueError, match="holds no audio"):
        sed.stream.StreamEvents(ev, [0, 8], [0], 0.1).event_audio(0)


# ───────────── 3. the margins of the proof ─────────────
@pytest.mark.parametrize("hop_length", [512, 1024, 1500])
def test_an_emitted_event_lies_half_a_frame_inside_what_was_received(sed, hop_length):
    """A live feed emits [a, b) only with N >= b*tf + lat final feature frames (stream_latency_frames), and a stream refuses
    to locate unless n >= (N - 1)*hop_length + n_fft/2.  With the LEAST such n: the event's samples end at least n_fft/2 = 1024
    samples before n — so s1 is what any later n gives, the offline one included — and the delay-and-sum beam's reach beyond
    [s0, s1) stays below 1024 on both sides: the received samples on the right, what the ring rule keeps (f0*hop - 1024) on the
    left."""
    from sed_crnn_amd.localize import event_frames, event_samples, stream_latency_frames
    assert BEAM_REACH < NFFT // 2
    checked = 0
    for tf, seq_len, median, min_gap, MF in itertools.product((1, 4, 8), (8, 64, 256), (1, 5), (0, 3), (1, 8, 64)):
        if seq_len < tf:
            continue
        lat = stream_latency_frames(tf, seq_len, median, min_gap)
        for a, length, pk in ((0, 1, 0), (0, 40, 39), (3, 2, 4), (7, 100, 50), (1000, 17, 1005)):
            b = a + length
            N = b * tf + lat                                                 # the least count of final frames at emission
            assert N // tf - seq_len // tf - median // 2 > b + min_gap       # ... it is: more than b + min_gap frames are decided
            assert (N - tf) // tf - seq_len // tf - median // 2 <= b + min_gap
            n = (N - 1) * hop_length + NFFT // 2                             # the least n the stream locates with
            f0, f1 = event_frames(a, b, pk, tf, 1 + n // hop_length, MF)
            assert f1 <= b * tf < N and f1 - f0 == min(length * tf, MF)
            s0, s1 = event_samples(a, b, pk, tf, n, hop_length, MF, 0, f1 - f0)
            assert (s0, s1) == (f0 * hop_length, f1 * hop_length)            # not clipped by n
            assert n - s1 >= NFFT // 2 > BEAM_REACH
            for later in (n + 1, n + hop_length, 10 * n):                    # the final n of the feed
                assert event_frames(a, b, pk, tf, 1 + later // hop_length, MF) == (f0, f1)
                assert event_samples(a, b, pk, tf, later, hop_length, MF, 0, f1 - f0) == (s0, s1)
            assert s0 - BEAM_REACH > f0 * hop_length - NFFT // 2             # the left reach is inside what the ring rule keeps
            checked += 1
    assert checked >= 400


# ───────────── 4. the C entries ─────────────
def test_lib_exposes_the_ring_entries_of_the_mvdr_beam():
    from sed_crnn_amd import _lib
    L = _lib.lib()
    sig = _lib.SIGNATURES
    assert sig["sed_event_mvdr_ring_workspace_bytes"] == sig["sed_event_mvdr_workspace_bytes"]
    res, args = sig["sed_event_mvdr_ring"]
    lin_res, lin_args = sig["sed_event_mvdr"]
    ring_res, ring_args = sig["sed_event_beamform_ring"]
    # (ring, ring_len, cap, n_host) in place of (pcm, pcm_len, clips_host): as sed_event_beamform_ring relates to sed_event_beamform
    assert res == lin_res == ring_res and args[:4] == ring_args[:4] and args[4:] == lin_args[3:] and len(args) == 28
    assert L.sed_event_mvdr_ring.argtypes == args and L.sed_event_mvdr_ring_workspace_bytes.restype == C.c_size_t
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "sedcrnn.h")) as f:
        header = f.read()
    assert "size_t sed_event_mvdr_ring_workspace_bytes(int R, int channels, int max_frames, int hop);" in header
    assert "int sed_event_mvdr_ring(const float* ring, long ring_len, long cap, const long* n_host, int R, int channels," in header
    # the table of R sample counts (rounded up to 16 bytes) in place of the linear call's R*C + R entries; the events' rows are the same
    for R, Cn, MF, hop in ((1, 2, 8, 1024), (3, 4, 36, 1024), (2, 8, 256, 512), (5, 3, 1, 1500)):
        ring, lin = L.sed_event_mvdr_ring_workspace_bytes(R, Cn, MF, hop), L.sed_event_mvdr_workspace_bytes(R, Cn, MF, hop)
        assert ring > 0 and lin - ring == L.sed_event_beam_workspace_bytes(R, Cn) - L.sed_event_beam_ring_workspace_bytes(R)
    J = -(-36 * 1024 // 1024)                                               # 36 output blocks: 37 frames, two chunks of 32
    rows = 2 * (4 * 5 // 2) + 4
    assert L.sed_event_mvdr_ring_workspace_bytes(3, 4, 36, 1024) == 32 + rows * 1026 * 8 and -(-(J + 1) // 32) == 2
    for bad in ((0, 2, 8, 1024), (1, 1, 8, 1024), (1, 9, 8, 1024), (1, 2, 0, 1024), (1, 2, 8, 0), (1, 2, 1 << 22, 1024)):
        assert L.sed_event_mvdr_ring_workspace_bytes(*bad) == 0


def test_mvdr_ring_entry_checks_its_arguments_on_the_host():
    """every refusal is made before anything is enqueued: the pointers are never followed (they point nowhere)"""
    from sed_crnn_amd import _lib
    L = _lib.lib()
    FAKE = C.c_void_p(0x1000)

    def call(channels=2, E=1, hop=1024, max_frames=8, D=72, loading=1e-2, tables=FAKE, tb=1 << 16, alen=FAKE, audio=FAKE, total=100, ws=0,
             cap=8192, n=9000, ring=FAKE, tau=FAKE):
        t = np.asarray([n], dtype=np.int64)
        return L.sed_event_mvdr_ring(ring, 1 << 20, cap, C.c_void_p(t.ctypes.data), 1, channels, None, FAKE, FAKE, FAKE, FAKE, FAKE, E, 1,
                                     hop, max_frames, tau, D, loading, tables, tb, alen, FAKE, audio, total, FAKE, ws, None)

    def err():
        return L.sed_last_error_string().decode()
    for bad, what in ((dict(channels=1), "channels"), (dict(channels=9), "channels"), (dict(max_frames=0), "max_frames"), (dict(hop=0), "bad sizes"),
                      (dict(D=0), "at least one direction"), (dict(ring=None), "null pointer (the rings)"), (dict(cap=100), "a ring holds"),
                      (dict(cap=8190), "a ring holds"), (dict(cap=1 << 20), "leave the buffer"), (dict(n=-1), "samples received"),
                      (dict(loading=0.0), "loading"), (dict(total=-1), "a total of -1"), (dict(tau=None), "null pointer"),
                      (dict(alen=None), "null pointer"), (dict(audio=None), "null output buffer"), (dict(tables=None), "table blob"),
                      (dict(tb=64), "table blob"), (dict(ring=C.c_void_p(0x1002)), "4-byte aligned"), (dict(), "workspace of 0 bytes")):
        assert call(**bad) != 0 and what in err() and err().startswith("mvdr_ring:"), (bad, err())
    assert call(E=0) == 0 and call(total=0, audio=None) == 0                 # no events, or nothing to extract: nothing is launched


def test_build_guards_the_ring_kernels_against_scratch():
    from sed_crnn_amd.build import NO_SCRATCH_KERNELS
    assert {"mvdr_ring_cov_k", "mvdr_ring_apply_k"} <= set(NO_SCRATCH_KERNELS["mvdr.hip"])
