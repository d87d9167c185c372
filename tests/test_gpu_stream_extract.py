"""Live feeds emit each located event's audio, on the MI355X: feature.event_mvdr_ring against feature.event_mvdr on the
linear prefix bit for bit — across the ring's wrap, with an odd hop, across the covariance chunks and the apply runs, sliced, and
with 8 channels — and a StreamDetector with emit_audio=True, through either beam, against the offline call in two chunkings and
in one push of many steps."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import doa_ref  # noqa: E402
from test_gpu_beam import _located  # noqa: E402
from test_gpu_doa import _array  # noqa: E402
from test_gpu_multichannel import _stereo, det2  # noqa: E402,F401
from test_gpu_resample import _feed  # noqa: E402
from test_gpu_stream_tdoa import COARSE, SIZES  # noqa: E402
from test_gpu_tdoa import _bits, _events, sed  # noqa: E402,F401

pytestmark = pytest.mark.gpu
SR = 44100


def _ring_of(x, cap, pieces, feeds=1):
    """x [n, C] written through feature.ring_write in the given pieces into the rings of feed 0 of ``feeds``; the rest stays NaN: a
    read of an entry that was never written would show"""
    from sed_crnn_amd import feature
    C = x.shape[1]
    ring = torch.full((feeds * C * cap,), float("nan"), device="cuda")
    at, ws = 0, None
    for m in pieces:
        src = torch.from_numpy(np.concatenate([x[at:at + m, c] for c in range(C)])).cuda()
        ws = feature.ring_write(ring, cap, src, [(c * m, m, at) for c in range(C)], ws)
        at += m
    assert at == x.shape[0]
    return ring


def _linear(x):
    n, C = x.shape
    return torch.from_numpy(np.ascontiguousarray(x.T).reshape(-1)).cuda(), [(c * n, n) for c in range(C)]


def _same_tables(got, ref):
    for k in ("audio", "audio_start", "audio_len"):
        assert got[k].dtype == ref[k].dtype and got[k].shape == ref[k].shape, k
    assert torch.equal(got["audio_len"], ref["audio_len"]) and torch.equal(got["audio_start"], ref["audio_start"])
    assert np.array_equal(_bits(got["audio"]), _bits(ref["audio"]))
    assert torch.isfinite(got["audio"]).all()


# ───────────── 1. the ring against the linear call ─────────────
@pytest.mark.parametrize("hop", [1024, 1001])
def test_mvdr_ring_equals_linear_bit_for_bit(sed, hop):
    """test_gpu_stream_doa's scene: C = 3, a ring of 12292 samples written in uneven pieces up to 30000 samples (it has wrapped
    twice), a second feed that stays NaN.  The events event_doa_ring located — one frame, several frames across the wrap point,
    the newest frame — carry the bits of event_mvdr on the linear samples; those it refused have dir = -1 and length 0.  With
    hop = 1001 an event on an odd frame starts on an odd sample: every frame of it takes the guarded loads."""
    from sed_crnn_amd import feature
    from sed_crnn_amd.localize import event_frames, stream_locates
    C, cap, n, MF, LAT, HIST = 3, 12292, 30000, 8, 3, 14
    pos = doa_ref.line(C, 0.04)
    x = doa_ref.far_field(n, pos, doa_ref.unit(1.0, 0.3), SR, seed=5)
    doa = sed.DOA(pos, sed.DirectionGrid.sphere(200), max_frames=MF, oversample=8)
    mv = sed.MVDR(1e-2)
    ring = _ring_of(x, cap, (1, 2047, 5000, 9000, 6000, 6000, 1952), feeds=2)
    last = n // hop
    wrap = next(f for f in range(22, last) if (f * hop - 1024) // cap != (f * hop + 1023) // cap)
    rows = [(last, last + 1, last), (22, 23, 22), (wrap - 1, wrap + 2, wrap), (23, 29, 25), (21, 29, 28),
            (19, 20, 19), (18, 19, 18), (24, 24 + 60, 24), (0, 1, 0), (22, 23, 22)]
    rec = [0] * 9 + [3]
    n_feat = 1 + n // hop
    want = []
    for (a, b, pk), r in zip(rows, rec):
        f0, f1 = event_frames(a, b, pk, 1, n_feat, MF)
        want.append(r == 0 and stream_locates(a, b, pk, 1, n_feat, MF, LAT, HIST) and max(0, f0 * hop - 1024) >= n - cap)
    assert want == [True, True, True, True, True, True, False, False, False, False]
    ev = _events(rows, rec)
    located = feature.event_doa_ring(ring, cap, [n, 0], C, ev, 1, doa, sr=SR, hop=hop, lat_frames=LAT, history_frames=HIST)
    d = located["dir"].cpu().numpy()
    assert (d >= 0).tolist() == want
    ev = {**ev, "dir": located["dir"], "loc_frames": located["loc_frames"]}
    got = feature.event_mvdr_ring(ring, cap, [n, 0], C, ev, 1, doa, mv, sr=SR, hop=hop)
    pcm, clips = _linear(x)
    lin_ev = {**_events(rows, [0] * 10), "dir": located["dir"], "loc_frames": located["loc_frames"]}
    ref = feature.event_mvdr(pcm, clips, C, lin_ev, 1, doa, mv, sr=SR, hop=hop)
    _same_tables(got, ref)
    lens = got["audio_len"].cpu().numpy()
    spans = [sed.event_samples(*r, 1, n, hop, MF, int(d[e]), int(located["loc_frames"][e])) for e, r in enumerate(rows)]
    assert lens.tolist() == [s1 - s0 for s0, s1 in spans] and (lens[:6] > 0).all() and not lens[6:].any()
    assert lens[0] == n - last * hop and lens[3] == 6 * hop
    assert sum(1 for s0, s1 in spans if s1 > s0 and s0 // cap != (s1 - 1) // cap) >= 1       # an extracted event wraps the ring
    if hop % 2:
        assert any(s1 > s0 and s0 % 2 for s0, s1 in spans)                                    # ... and one starts on an odd sample
    none = feature.event_mvdr_ring(ring, cap, [n, 0], C, {**_events(np.zeros((0, 3)), []), "dir": located["dir"][:0],
                                                          "loc_frames": located["loc_frames"][:0]}, 1, doa, mv, sr=SR, hop=hop)
    assert none["audio"].shape == (0,) and none["audio_len"].shape == (0,) and none["audio_start"].dtype == torch.int64


def test_mvdr_ring_chunks_runs_and_slices_across_the_wrap(sed):
    """C = 2, a ring of 40004 samples after 100000: an event of 36 frames — 37 transform frames, so two covariance chunks of 32
    and three apply runs of 16 blocks — whose samples contain the wrap point 2 cap, one of its frames straddling it, and an
    event of one (cut) frame at the end.  The bits are the linear call's, and they stay when the workspace holds one event."""
    from sed_crnn_amd import _lib, feature
    C, cap, n, MF, hop = 2, 40004, 100000, 36, 1024
    pos = doa_ref.line(C, 0.08)
    x = doa_ref.far_field(n, pos, doa_ref.unit(0.7, 0.0), SR, seed=8)
    doa = sed.DOA(pos, sed.DirectionGrid.ring(72), max_frames=MF, oversample=8)
    mv = sed.MVDR(1e-2)
    ring = _ring_of(x, cap, (40004, 1, 29995, 30000))
    rows, dirs, loc = [(60, 96, 70), (97, 98, 97)], [5, 40], [36, 1]
    s0, s1 = sed.event_samples(*rows[0], 1, n, hop, MF, dirs[0], loc[0])
    assert (s0, s1) == (60 * hop, 96 * hop) and s0 >= n - cap and s0 < 2 * cap < s1
    assert any(a < 2 * cap < a + 2048 for a in range(s0, s1 - 2048 + 1, 1024))               # a whole frame straddles the wrap point
    assert -(-(s1 - s0) // 1024) == 36 and -(-37 // 32) == 2 and -(-36 // 16) == 3
    ev = _located(rows, [0, 0], dirs, loc)
    got = feature.event_mvdr_ring(ring, cap, [n], C, ev, 1, doa, mv, sr=SR, hop=hop)
    pcm, clips = _linear(x)
    ref = feature.event_mvdr(pcm, clips, C, ev, 1, doa, mv, sr=SR, hop=hop)
    _same_tables(got, ref)
    assert got["audio_len"].tolist() == [36 * hop, n - 97 * hop]
    one = _lib.lib().sed_event_mvdr_ring_workspace_bytes(1, C, MF, hop)
    sliced = feature.event_mvdr_ring(ring, cap, [n], C, ev, 1, doa, mv, sr=SR, hop=hop, max_workspace_bytes=one)
    _same_tables(sliced, ref)


def test_mvdr_ring_with_eight_channels(sed):
    """C = 8: the covariance kernel holds a batch of the 36 entries at a time and transforms the chunk's frames again for every
    batch.  Two events of 2 and 5 frames, the longer one across the wrap point."""
    from sed_crnn_amd import feature
    C, cap, n, MF, hop = 8, 12292, 30000, 8, 1024
    pos = _array(C)
    x = doa_ref.far_field(n, pos, doa_ref.unit(-0.4, 0.2), SR, seed=9)
    doa = sed.DOA(pos, sed.DirectionGrid.sphere(200), max_frames=MF, oversample=8)
    mv = sed.MVDR(1e-2)
    ring = _ring_of(x, cap, (7001, 12292, 10707))
    rows, dirs, loc = [(27, 29, 27), (22, 27, 24)], [17, 150], [2, 5]
    spans = [sed.event_samples(*r, 1, n, hop, MF, d, lf) for r, d, lf in zip(rows, dirs, loc)]
    assert spans == [(27 * hop, 29 * hop), (22 * hop, 27 * hop)] and min(s0 for s0, _ in spans) >= n - cap
    assert spans[1][0] < 2 * cap < spans[1][1]
    ev = _located(rows, [0, 0], dirs, loc)
    got = feature.event_mvdr_ring(ring, cap, [n], C, ev, 1, doa, mv, sr=SR, hop=hop)
    pcm, clips = _linear(x)
    ref = feature.event_mvdr(pcm, clips, C, ev, 1, doa, mv, sr=SR, hop=hop)
    _same_tables(got, ref)
    assert got["audio_len"].tolist() == [2 * hop, 5 * hop]


# ───────────── 2. the stream ─────────────
def _covers(o):
    """the slices of one StreamEvents are disjoint and cover its audio"""
    start, length = o.events["audio_start"].cpu().numpy(), o.events["audio_len"].cpu().numpy()
    assert o.events["audio_start"].dtype == torch.int64 and o.events["audio_len"].dtype == torch.int32 and o.audio.dtype == torch.float32
    assert start.shape == length.shape == (len(o),)
    at = 0
    for a, b in sorted((int(s), int(s) + int(m)) for s, m in zip(start, length) if m > 0):
        assert a == at
        at = b
    assert at == o.audio.numel() and ((start >= 0) & (start <= o.audio.numel())).all()


def _audio_by_event(outs, S):
    """the calls of one run -> {(feed, class, onset): (dir, the bits of the event's audio)}"""
    res = {}
    for o in outs:
        _covers(o)
        ev = {k: v.cpu().numpy() for k, v in o.events.items()}
        for e in range(len(o)):
            key = (int(ev["stream"][e]), int(ev["cls"][e]), int(ev["onset"][e]))
            assert key not in res and 0 <= key[0] < S
            a = o.event_audio(e)
            assert a.numel() == ev["audio_len"][e]
            res[key] = (int(ev["dir"][e]), _bits(a))
    return res


def _extracting(sed, det2, beam):
    plain, _ = det2
    doa = sed.DOA(doa_ref.line(2, 0.08), sed.DirectionGrid.ring(72), max_frames=8, oversample=8)
    return sed.EventDetector(plain.model, max_batch=1, median=3, mean=plain.mean, std=plain.std, localize=doa,
                             extract=getattr(sed, beam)())


def _check_against_offline(sed, det, st, got, offline, recs):
    """every emitted event that the stream's rule accepts has the offline event's audio, the others none -> (events, extracted)"""
    from sed_crnn_amd.localize import stream_locates
    tf, n_ev, n_audio = det.model.time_factor, 0, 0
    for s, (one, w) in enumerate(zip(offline, recs)):
        want = {k: v.cpu().numpy() for k, v in one.events.items()}
        n = sed.resample(w, 48000, channels=2, keep_channels=True).shape[1]
        mine = {k: v for k, v in got.items() if k[0] == s}
        assert sorted((c, a) for _, c, a in mine) == sorted(zip(want["cls"].tolist(), want["onset"].tolist()))
        for e in range(len(one)):
            a, b, p = int(want["onset"][e]), int(want["offset"][e]), int(want["peak_frame"][e])
            d, bits = mine[(s, int(want["cls"][e]), a)]
            if stream_locates(a, b, p, tf, 1 + n // det.hop_length, 8, st.lat, st.history_frames):
                assert d == want["dir"][e] and np.array_equal(bits, _bits(one.event_audio(e))), (s, e)
                n_audio += int(bits.size > 0)
            else:
                assert d == -1 and bits.size == 0, (s, e)
            n_ev += 1
    return n_ev, n_audio


@pytest.mark.parametrize("beam", ["DelaySum", "MVDR"])
def test_stream_carries_the_offline_audio(sed, det2, beam):
    """two feeds, history "min" (the rings wrap several times), in fine and in coarse pieces, through either beam: where
    localize.stream_locates accepts an emitted event its audio is the offline call's bit for bit, where it refuses the event
    has no audio; the slices of every StreamEvents are disjoint and cover its buffer; the chunking changes no bit"""
    det = _extracting(sed, det2, beam)
    recs = [_stereo(48000 * 8, 48000, 10), _stereo(48000 * 8 + 4001, 48000, 11)]
    offline = [det(w, sr=48000, channels=2) for w in recs]
    runs = []
    for sizes in (SIZES, COARSE):
        st = det.stream(2, history_frames="min", max_new_windows=1, input_sr=48000, emit_audio=True)
        assert 2 * st.cap < recs[0].shape[0] * det.sr // 48000               # the ring wraps at least twice
        outs = _feed(st, recs, sizes) + [st.flush()]
        for o in outs:
            assert {"audio_start", "audio_len", "dir", "loc_frames"} <= set(o.events) and o.audio is not None
        got = _audio_by_event(outs, 2)
        n_ev, n_audio = _check_against_offline(sed, det, st, got, offline, recs)
        print(f"{beam}, pieces {sizes[:3]}..: {n_audio} of {n_ev} events came with audio")
        assert n_audio >= 1
        runs.append(got)
    assert set(runs[0]) == set(runs[1])
    for k in runs[0]:                                                         # the chunking changes no bit
        assert runs[0][k][0] == runs[1][k][0] and np.array_equal(runs[0][k][1], runs[1][k][1]), k
    empty = det.stream(2, history_frames="min", max_new_windows=1, input_sr=48000, emit_audio=True).push([None, None])
    assert len(empty) == 0 and empty.audio.shape == (0,) and empty.audio.dtype == torch.float32
    assert empty.events["audio_start"].dtype == torch.int64 and empty.events["audio_len"].dtype == torch.int32
    assert empty.events["audio_start"].shape == empty.events["audio_len"].shape == (0,)


@pytest.mark.parametrize("beam", ["DelaySum", "MVDR"])
def test_one_push_of_many_steps_carries_the_same_audio(sed, det2, beam):
    """one feed's whole recording in a single push, then flush: the push is split into steps, every step that emits events
    extracts them and the steps' buffers are merged; every event's audio is the fine-chunked run's — and the offline call's"""
    det = _extracting(sed, det2, beam)
    rec = _stereo(48000 * 8, 48000, 10)
    offline = det(rec, sr=48000, channels=2)
    st = det.stream(1, history_frames="min", max_new_windows=1, input_sr=48000, emit_audio=True)
    n = sed.resample(rec, 48000, channels=2, keep_channels=True).shape[1]
    assert n > 3 * (st.step_frames - 1) * det.hop_length                      # more than three steps
    whole = [st.push([rec]), st.flush()]
    assert len(whole[0]) >= 2
    start = whole[0].events["audio_start"].cpu().numpy()
    print(f"{beam}: {len(whole[0])} events in one push, audio_start {start.tolist()}")
    got = _audio_by_event(whole, 1)
    fine = _audio_by_event(_feed(st, [rec], SIZES) + [st.flush()], 1)         # (the flush restarted the feed)
    assert set(got) == set(fine)
    for k in got:
        assert got[k][0] == fine[k][0] and np.array_equal(got[k][1], fine[k][1]), k
    n_ev, n_audio = _check_against_offline(sed, det, st, got, [offline], [rec])
    assert n_audio >= 1
