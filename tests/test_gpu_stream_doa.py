"""Direction of arrival on live feeds, on the MI355X: feature.event_doa_ring against feature.event_doa on the linear
prefix bit for bit across the ring's wrap, with events the stream's rule and the ring's depth refuse; and a StreamDetector with
localize=DOA(...) in two chunkings against the offline call."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import doa_ref  # noqa: E402
from test_gpu_detect import _assert_events_equal  # noqa: E402
from test_gpu_multichannel import _stereo, det2  # noqa: E402,F401
from test_gpu_resample import _feed  # noqa: E402
from test_gpu_stream_tdoa import COARSE, SIZES, _by_feed  # noqa: E402
from test_gpu_tdoa import _bits, _events, sed  # noqa: E402,F401

pytestmark = pytest.mark.gpu
SR, HOP = 44100, 1024
KEYS = ("lag", "strength", "loc_frames", "acc", "dir", "doa_power", "srp")
DOA_KEYS = ("lag", "strength", "loc_frames", "dir", "doa_power")


def test_ring_equals_linear_bit_for_bit(sed):
    """C = 3, a ring of 12292 samples (no multiple of the hop) written in pieces up to 30000 samples: it has wrapped twice.
    Located events — one frame, several frames across the wrap point, the newest frame — carry the bits of the linear call;
    an event the rule refuses, one whose first sample has left the ring and one that names no feed have dir = -1, power 0."""
    from sed_crnn_amd import feature
    from sed_crnn_amd.localize import event_frames, stream_locates
    C, cap, n, MF, LAT, HIST = 3, 12292, 30000, 8, 3, 14
    pos = doa_ref.line(C, 0.04)
    x = doa_ref.far_field(n, pos, doa_ref.unit(1.0, 0.3), SR, seed=5)
    doa = sed.DOA(pos, sed.DirectionGrid.sphere(200), max_frames=MF, oversample=8)
    ring = torch.full((2 * C * cap,), float("nan"), device="cuda")          # two feeds (the second stays empty); a read of an unwritten entry would show
    at, ws = 0, None
    for m in (1, 2047, 5000, 9000, 6000, 6000, 1952):
        src = torch.from_numpy(np.concatenate([x[at:at + m, c] for c in range(C)])).cuda()
        ws = feature.ring_write(ring, cap, src, [(c * m, m, at) for c in range(C)], ws)
        at += m
    assert at == n
    last = n // HOP                                                          # frame 29; kept samples from 17708: frames >= 19 are whole
    wrap = next(f for f in range(22, last) if (f * HOP - 1024) // cap != (f * HOP + 1023) // cap)
    rows = [(last, last + 1, last), (22, 23, 22), (wrap - 1, wrap + 2, wrap), (23, 29, 25), (21, 29, 28),
            (19, 20, 19), (18, 19, 18), (24, 24 + 60, 24), (0, 1, 0), (22, 23, 22)]
    rec = [0] * 9 + [3]
    n_feat = 1 + n // HOP
    want = []
    for (a, b, pk), r in zip(rows, rec):
        f0, f1 = event_frames(a, b, pk, 1, n_feat, MF)
        want.append(r == 0 and stream_locates(a, b, pk, 1, n_feat, MF, LAT, HIST) and max(0, f0 * HOP - 1024) >= n - cap)
    assert want == [True, True, True, True, True, True, False, False, False, False]
    ev = _events(rows, rec)
    kw = dict(sr=SR, hop=HOP, return_curve=True, return_map=True)
    got = feature.event_doa_ring(ring, cap, [n, 0], C, ev, 1, doa, lat_frames=LAT, history_frames=HIST, **kw)
    lin = torch.from_numpy(np.ascontiguousarray(x.T).reshape(-1)).cuda()
    ref = feature.event_doa(lin, [(c * n, n) for c in range(C)], C, _events(rows, [0] * 10), 1, doa, **kw)
    assert set(got) == set(KEYS) == set(ref)
    loc = torch.tensor(want).cuda()
    for k in KEYS:
        assert np.array_equal(_bits(got[k][loc]), _bits(ref[k][loc])), k
        assert torch.isfinite(got[k]).all(), k
    assert (got["dir"][loc] >= 0).all() and (got["doa_power"][loc] > 0.1).all() and (got["loc_frames"][loc] > 0).all()
    assert (got["dir"][~loc] == -1).all() and not got["doa_power"][~loc].any() and not got["srp"][~loc].any() and not got["loc_frames"][~loc].any()
    # the TDOA keys are event_tdoa_ring's
    t = feature.event_tdoa_ring(ring, cap, [n, 0], C, ev, 1, max_lag=doa.max_lag(SR), max_frames=MF, hop=HOP, lat_frames=LAT,
                                history_frames=HIST, return_curve=True)
    for k in t:
        assert np.array_equal(_bits(got[k]), _bits(t[k])), k
    none = feature.event_doa_ring(ring, cap, [n, 0], C, _events(np.zeros((0, 3)), []), 1, doa, **kw)
    assert none["dir"].shape == (0,) and none["srp"].shape == (0, 200) and none["lag"].shape == (0, 3)


def test_doa_stream_carries_the_offline_directions(sed, det2):
    """two feeds, history "min" (the rings wrap several times), in fine and in coarse pieces: every emitted event has the five
    event keys of det(w); where localize.stream_locates accepts it, lag, strength, loc_frames, dir and doa_power are the
    offline call's bit for bit; where it refuses, dir = -1 and the others are 0"""
    from sed_crnn_amd.localize import stream_locates
    plain, _ = det2
    doa = sed.DOA(doa_ref.line(2, 0.08), sed.DirectionGrid.ring(72), max_frames=8, oversample=8)
    det = sed.EventDetector(plain.model, max_batch=1, median=3, mean=plain.mean, std=plain.std, localize=doa)
    recs = [_stereo(48000 * 8, 48000, 10), _stereo(48000 * 8 + 4001, 48000, 11)]
    offline = [det(w, sr=48000, channels=2) for w in recs]
    tf = det.model.time_factor
    runs = []
    for sizes in (SIZES, COARSE):
        st = det.stream(2, history_frames="min", max_new_windows=1, input_sr=48000)
        assert 2 * st.cap < recs[0].shape[0] * det.sr // 48000               # the ring wraps at least twice
        outs = _feed(st, recs, sizes) + [st.flush()]
        for o in outs:
            assert set(o.events) == {"stream", "cls", "onset", "offset", "peak", "peak_frame"} | set(DOA_KEYS)
            assert o.grid is doa.grid and o.doa().shape == (len(o), 3) and np.array_equal(o.doa(1), o.doa()[o.event_offsets[1]:o.event_offsets[2]], equal_nan=True)
            d = o.events["dir"].cpu().numpy()
            assert np.array_equal(np.isnan(o.doa()[:, 0]), d < 0) and np.array_equal(o.doa()[d >= 0, 0], doa.grid.azimuth[d[d >= 0]])
        feeds = _by_feed(outs, 2)
        n_ev = n_loc = 0
        for got, one, w in zip(feeds, offline, recs):
            want = {k: v.cpu().numpy() for k, v in one.events.items()}
            five = ("cls", "onset", "offset", "peak", "peak_frame")
            _assert_events_equal({k: got[k] for k in five}, {k: want[k] for k in five}, "the event keys")
            n = sed.resample(w, 48000, channels=2, keep_channels=True).shape[1]
            loc = np.array([stream_locates(a, b, p, tf, 1 + n // det.hop_length, 8, st.lat, st.history_frames)
                            for a, b, p in zip(want["onset"], want["offset"], want["peak_frame"])], bool).reshape(-1)
            assert (want["dir"] >= 0).all() and (got["dir"][loc] >= 0).all()
            for k in DOA_KEYS:
                assert np.array_equal(got[k][loc].view(np.int32), want[k][loc].view(np.int32)), k
            assert (got["dir"][~loc] == -1).all() and not got["doa_power"][~loc].any() and not got["loc_frames"][~loc].any()
            n_ev, n_loc = n_ev + len(loc), n_loc + int(loc.sum())
        print(f"pieces {sizes[:3]}..: lat {st.lat}, history {st.history_frames}, ring {st.cap} samples; {n_loc} of {n_ev} events located")
        assert n_loc >= 1
        runs.append(feeds)
    for a, b in zip(*runs):                                                   # the chunking changes no bit
        assert set(a) == set(b)
        for k in a:
            assert np.array_equal(a[k].view(np.int32), b[k].view(np.int32)), k
