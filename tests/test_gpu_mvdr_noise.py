"""The MVDR beam with its covariance taken from before the onset, on the MI355X: feature.event_mvdr with
sed.MVDR(noise_blocks=Kn, noise_guard=G) against the float64 definition (tests/mvdr_noise_ref.py); the events that fall back, the
batch, a permuted table, the slicing and every sample outside an event's two ranges bit for bit; the ring entry against the
linear one; the detector's entry points and a live feed against det(wave); and the purpose — the output SIR of the scene of
tests/test_cpu_mvdr_noise.py against the reference's and against the own-frames beam's.

Measured on an MI355X over the 18 cases of test_audio_matches_the_float64_definition (audio against float64): kernel error
2.4e-7 .. 2.0e-6, float32 yardstick 2.2e-7 .. 2.8e-6, kernel / yardstick 0.69 .. 1.23 of the 8 allowed (worst: C = 2, Kn = 33,
hop 1024: kernel 3.02e-7, yardstick 2.46e-7); no yardstick was degenerate.  test_it_keeps_the_suppression_the_reference_has:
output SIR 15.442 dB from the kernel and from the float64 reference with Kn = 8, 10.111 dB from both with Kn = 0.  The stream:
5 of 7 emitted events come with audio, all 5 from the noise covariance, 1 is refused by the extended rule alone.  """
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import doa_ref  # noqa: E402
import mvdr_noise_ref  # noqa: E402
import mvdr_ref  # noqa: E402
from test_gpu_beam import _located, _np, _slices  # noqa: E402
from test_gpu_doa import _array  # noqa: E402
from test_gpu_multichannel import _stereo, det2  # noqa: E402,F401
from test_gpu_resample import _feed  # noqa: E402
from test_gpu_stream_extract import _audio_by_event, _linear, _ring_of  # noqa: E402
from test_gpu_stream_tdoa import COARSE, SIZES  # noqa: E402
from test_gpu_tdoa import DEGENERATE, _bits, _planar  # noqa: E402

pytestmark = pytest.mark.gpu
SR, B = 44100, 1024
N = 48 * B + 300                                    # 48 blocks and a cut one
MAX_FRAMES = 12
SETTINGS = [(1, 0), (8, 1), (33, 1)]                # (Kn, G); 33 frames are two chunks


@pytest.fixture(scope="module")
def sed():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    import sed_crnn_amd as s
    return s


_X = {}


def _recording(C, n=N, seed=0):
    """x [n, C] float32: two far-field sources and sensor noise, made once"""
    key = (C, n, seed)
    if key not in _X:
        pos = _array(C)
        x = doa_ref.far_field(n, pos, doa_ref.unit(2.2, 0.4), SR, seed=60 + C + seed)
        x = x + 0.7 * doa_ref.far_field(n, pos, doa_ref.unit(-0.7, -0.2), SR, seed=70 + C + seed)
        x = (x + 0.05 * np.random.default_rng(80 + C + seed).standard_normal(x.shape)).astype(np.float32)
        x.setflags(write=False)
        _X[key] = x
    return _X[key]


def _rows(Kn, G, hop, n=N):
    """the event rows of one recording at time_factor 1, and which of them are given a direction: the first frame whose event
    uses the noise covariance (hop 1024: its first noise frame starts at sample 0), the frame before it (falls back), an
    unlocated event, one longer than max_frames (the 12 frames around its peak start after that first frame), one on an odd
    frame, one that is clipped at n and one at the recording's start"""
    edge = -(-(G + Kn + 1) * B // hop)
    last = n // hop
    rows = [(edge, edge + 3, edge), (edge - 1, edge + 1, edge - 1), (edge + 2, edge + 4, edge + 2),
            (max(edge - 4, 0), edge + 16, edge + 9), (41, 44, 42), (last, last + 2, last), (1, 2, 1)]
    located = [True, True, False, True, True, True, True]
    return rows, located, edge


def _loc(rows, located, n, hop):
    from sed_crnn_amd.localize import event_frames
    return [(lambda f: f[1] - f[0])(event_frames(*r, 1, 1 + n // hop, MAX_FRAMES)) if ok else 0 for r, ok in zip(rows, located)]


def _table(Kn, G, hop, D, seed, n=N):
    rows, located, edge = _rows(Kn, G, hop, n)
    rng = np.random.default_rng(seed)
    dirs = [int(rng.integers(0, D)) if ok else -1 for ok in located]
    return rows, dirs, _loc(rows, located, n, hop), edge


# ───────────── 1. against float64 ─────────────
@pytest.mark.parametrize("hop", [1024, 1001])
@pytest.mark.parametrize("Kn,G", SETTINGS)
@pytest.mark.parametrize("C", [2, 4, 8])
def test_audio_matches_the_float64_definition(sed, C, Kn, G, hop):
    """max |audio - float64| within 8 x the float32 yardstick's (mvdr_noise_ref.beamform with f32=True; a yardstick below 1e-9
    is degenerate and fails); noise_frames, audio_start and audio_len exact.  hop 1001: events on odd samples, whose noise
    frames take the guarded loads."""
    from sed_crnn_amd import feature
    doa = sed.DOA(_array(C), sed.DirectionGrid.sphere(200), max_frames=MAX_FRAMES)
    x = _recording(C)
    rows, dirs, loc, edge = _table(Kn, G, hop, 200, seed=C)
    pcm, clips = _planar(x)
    mv = sed.MVDR(1e-2, noise_blocks=Kn, noise_guard=G)
    got = _np(feature.event_mvdr(pcm, clips, C, _located(rows, None, dirs, loc), 1, doa, mv, sr=SR, hop=hop))
    assert got["audio"].dtype == np.float32 and got["noise_frames"].dtype == np.int32 and got["noise_frames"].shape == (len(rows),)
    tau = doa.steering(SR)
    ref = mvdr_noise_ref.beamform(x, rows, dirs, loc, 1, hop, MAX_FRAMES, tau, 1e-2, Kn, G)
    yard = mvdr_noise_ref.beamform(x, rows, dirs, loc, 1, hop, MAX_FRAMES, tau, 1e-2, Kn, G, f32=True)
    assert np.array_equal(ref["audio_len"], got["audio_len"]) and np.array_equal(ref["audio_start"], got["audio_start"])
    assert np.array_equal(ref["noise_frames"], got["noise_frames"])
    s0 = ref["s0"]
    assert got["noise_frames"].tolist() == [Kn, 0, 0, Kn, Kn, Kn, 0] and s0[3] >= edge * hop and loc[3] == MAX_FRAMES
    assert got["audio_len"][5] == N - (N // hop) * hop and got["audio_len"][2] == 0 and got["audio_len"][1] == 2 * hop
    for e, (r, d, lf) in enumerate(zip(rows, dirs, loc)):
        a, b = sed.event_samples(*r, 1, N, hop, MAX_FRAMES, d, lf)
        assert got["audio_len"][e] == b - a and (b == a or s0[e] == a)
    if hop == 1024:
        assert s0[0] == (G + Kn + 1) * B                                     # the first noise frame starts at sample 0
    else:
        assert s0[4] % 2 == 1 and got["noise_frames"][4] == Kn               # an event on an odd sample
    assert got["audio"].shape == ref["audio"].shape and np.isfinite(got["audio"]).all()
    e_yard = np.abs(yard["audio"].astype(np.float64) - ref["audio"]).max()
    e_kernel = np.abs(got["audio"].astype(np.float64) - ref["audio"]).max()
    print(f"C={C} Kn={Kn} G={G} hop={hop}: yardstick {e_yard:.2e}  kernel {e_kernel:.2e}  ratio {e_kernel / max(e_yard, 1e-300):.2f}")
    assert e_yard >= DEGENERATE, ("degenerate yardstick", e_yard)
    assert e_kernel <= 8.0 * e_yard, (C, Kn, G, hop, e_kernel, e_yard)


# ───────────── 2. invariances ─────────────
def test_fallbacks_batch_permutation_slices_and_the_outside_change_no_bit(sed):
    from sed_crnn_amd import _lib, feature
    C, Kn, G, hop = 3, 8, 1, 1024
    need = (G + Kn + 1) * B
    doa = sed.DOA(_array(C), sed.DirectionGrid.sphere(200), max_frames=MAX_FRAMES)
    mv, own = sed.MVDR(1e-2, noise_blocks=Kn, noise_guard=G), sed.MVDR(1e-2)
    waves = [_recording(C), _recording(C, 21000, seed=1), _recording(C, 12 * B, seed=2)]
    tables = [_table(Kn, G, hop, 200, seed=1)[:3], ([(12, 15, 13), (3, 9, 5), (19, 25, 20)], [5, 60, 110], [3, 6, 2]),
              ([(10, 12, 10), (9, 12, 9)], [7, 9], [2, 3])]
    kw = dict(sr=SR, hop=hop)
    singles, plain = [], []
    for w, (rows, d, lf) in zip(waves, tables):
        pcm, clips = _planar(w)
        singles.append(feature.event_mvdr(pcm, clips, C, _located(rows, None, d, lf), 1, doa, mv, **kw))
        plain.append(feature.event_mvdr(pcm, clips, C, _located(rows, None, d, lf), 1, doa, own, **kw))
        assert "noise_frames" not in plain[-1] and torch.equal(singles[-1]["audio_len"], plain[-1]["audio_len"])
    used = [s["noise_frames"].tolist() for s in singles]
    assert used == [[Kn, 0, 0, Kn, Kn, Kn, 0], [Kn, 0, Kn], [Kn, 0]]
    assert singles[1]["audio_len"].tolist() == [3 * B, 6 * B, 21000 - 19 * B]
    n_fall = n_noise = 0
    for s, p, u in zip(singles, plain, used):                                        # a fallback is the own-frames beam, bit for bit
        for a, b, k in zip(_slices(s), _slices(p), u):
            if a.size:
                assert np.array_equal(a, b) == (k == 0)
                n_fall, n_noise = n_fall + (k == 0), n_noise + (k != 0)
    assert n_fall == 4 and n_noise == 7
    pieces, clips, at, first = [], [], 0, {}
    for r, w in enumerate(waves):                                                    # channels start at odd samples between sentinels
        for c in range(C):
            lead = (-at) % 4 + (3 if r == 1 else 1 if c == 1 else 0)
            pieces.append(np.full(lead, 7.0, np.float32))                           # (a read outside a clip would show)
            at += lead
            clips.append((at, w.shape[0]))
            first[(r, c)] = at
            pieces.append(np.ascontiguousarray(w[:, c]))
            at += w.shape[0]
    pieces.append(np.full(5, 7.0, np.float32))
    host = np.concatenate(pieces)
    buf = torch.from_numpy(host).cuda()
    rows = [r for t in tables for r in t[0]]
    rec = [i for i, t in enumerate(tables) for _ in t[0]]
    d_all, l_all = [v for t in tables for v in t[1]], [v for t in tables for v in t[2]]
    many = feature.event_mvdr(buf, clips, C, _located(rows, rec, d_all, l_all), 1, doa, mv, **kw)
    want = [p for one in singles for p in _slices(one)]
    got = _slices(many)
    assert len(got) == len(want) == len(rows) and many["noise_frames"].tolist() == [k for u in used for k in u]
    for e, (a, b) in enumerate(zip(got, want)):                                      # the batch and the clip's place in the buffer
        assert np.array_equal(a, b), ("batch", e)
    perm = np.random.default_rng(0).permutation(len(rows))
    shuffled = feature.event_mvdr(buf, clips, C, _located([rows[i] for i in perm], [rec[i] for i in perm], [d_all[i] for i in perm],
                                                          [l_all[i] for i in perm]), 1, doa, mv, **kw)
    assert shuffled["noise_frames"].tolist() == [many["noise_frames"].tolist()[i] for i in perm]
    for j, p in enumerate(_slices(shuffled)):
        assert np.array_equal(p, got[perm[j]]), ("permuted", j)
    tab = _lib.lib().sed_event_beam_workspace_bytes(len(waves), C)                   # 1 and 5 events per workspace
    per_event = _lib.lib().sed_event_mvdr_noise_workspace_bytes(len(waves), C, MAX_FRAMES, hop, Kn) - tab
    for n_ev in (1, 5):
        sliced = feature.event_mvdr(buf, clips, C, _located(rows, rec, d_all, l_all), 1, doa, mv, max_workspace_bytes=tab + n_ev * per_event, **kw)
        assert torch.equal(sliced["noise_frames"], many["noise_frames"])
        for e, p in enumerate(_slices(sliced)):
            assert np.array_equal(p, got[e]), ("slices of", n_ev, e)
    # event 4 of recording 0, frames [41, 44): every sample of its recording outside [s0 - (G+Kn+1)B, s0 - G B) and [s0, s1) is
    # replaced, the guard [s0 - G B, s0) included
    s0, s1 = sed.event_samples(*rows[4], 1, N, hop, MAX_FRAMES, d_all[4], l_all[4])
    assert (s0, s1) == (41 * hop, 44 * hop) and many["noise_frames"][4] == Kn
    other = host.copy()
    for c in range(C):
        o = first[(0, c)]
        other[o:o + s0 - need] = 5.0
        other[o + s0 - G * B:o + s0] = -2.0
        other[o + s1:o + N] = -3.0
    alone = _slices(feature.event_mvdr(torch.from_numpy(other).cuda(), clips, C, _located(rows, rec, d_all, l_all), 1, doa, mv, **kw))
    assert np.array_equal(alone[4], got[4]) and not np.array_equal(alone[0], got[0]) and not np.array_equal(alone[5], got[5])
    inside = host.copy()
    inside[first[(0, 1)] + s0 - G * B - 512] += 0.5                                  # a sample of the last block the noise frames read
    moved = _slices(feature.event_mvdr(torch.from_numpy(inside).cuda(), clips, C, _located(rows, rec, d_all, l_all), 1, doa, mv, **kw))
    assert not np.array_equal(moved[4], got[4])
    none = feature.event_mvdr(buf, clips, C, _located(np.zeros((0, 3)), [], [], []), 1, doa, mv, **kw)
    assert none["audio"].shape == (0,) and none["noise_frames"].shape == (0,) and none["noise_frames"].dtype == torch.int32
    nothing = feature.event_mvdr(buf, clips, C, _located(rows, rec, [-1] * len(rows), l_all), 1, doa, mv, **kw)
    assert nothing["audio"].shape == (0,) and not nothing["audio_len"].any() and not nothing["noise_frames"].any()


# ───────────── 3. the ring ─────────────
@pytest.mark.parametrize("hop", [1024, 1001])
def test_ring_equals_linear_bit_for_bit(sed, hop):
    """C = 3, a ring of 12292 samples written in uneven pieces up to 30000 samples (it has wrapped twice; the wrap point 24584
    lies in what it holds), a second feed that stays NaN, Kn = 4, G = 1.  The noise frames of the event at frame 27 straddle
    the wrap point, those of the event at frame 24 do not; the last event is cut at n.  hop 1001: the event at frame 27 starts
    on an odd sample.  Audio and noise_frames are event_mvdr's on the linear samples."""
    from sed_crnn_amd import _lib, feature
    C, cap, n, MF, Kn, G = 3, 12292, 30000, 8, 4, 1
    pos = doa_ref.line(C, 0.04)
    x = doa_ref.far_field(n, pos, doa_ref.unit(1.0, 0.3), SR, seed=5)
    x = (x + 0.5 * doa_ref.far_field(n, pos, doa_ref.unit(-1.2, 0.0), SR, seed=6)).astype(np.float32)
    doa = sed.DOA(pos, sed.DirectionGrid.sphere(200), max_frames=MF, oversample=8)
    mv = sed.MVDR(1e-2, noise_blocks=Kn, noise_guard=G)
    ring = _ring_of(x, cap, (1, 2047, 5000, 9000, 6000, 6000, 1952), feeds=2)
    last = n // hop
    rows, rec = [(27, 29, 27), (24, 26, 24), (last, last + 1, last), (25, 26, 25), (26, 27, 26)], [0, 0, 0, 0, 1]
    dirs, loc = [17, 150, 3, -1, 40], [2, 2, 1, 1, 1]
    need, kept, wrap = (G + Kn + 1) * B, n - cap, 2 * cap
    spans = [sed.event_samples(*r, 1, n, hop, MF, d, lf) for r, d, lf in zip(rows, dirs, loc)]
    assert all(s0 - need >= kept for s0, s1 in spans[:3]) and kept < wrap < n
    lo = spans[0][0] - need
    assert any(lo + q * B < wrap < lo + q * B + 2048 for q in range(Kn))     # a noise frame straddles the wrap point
    assert spans[1][0] - G * B <= wrap                                       # ... and the noise frames of event 1 end before it
    if hop % 2:
        assert spans[0][0] % 2 == 1
    ev = _located(rows, rec, dirs, loc)
    got = feature.event_mvdr_ring(ring, cap, [n, 0], C, ev, 1, doa, mv, sr=SR, hop=hop)
    pcm, clips = _linear(x)
    lin = _located(rows, [0] * 5, dirs[:4] + [-1], loc)
    ref = feature.event_mvdr(pcm, clips, C, lin, 1, doa, mv, sr=SR, hop=hop)
    for k in ("audio", "audio_start", "audio_len", "noise_frames"):
        assert got[k].dtype == ref[k].dtype and got[k].shape == ref[k].shape, k
    assert torch.equal(got["audio_len"], ref["audio_len"]) and torch.equal(got["noise_frames"], ref["noise_frames"])
    assert np.array_equal(_bits(got["audio"]), _bits(ref["audio"])) and torch.isfinite(got["audio"]).all()
    assert got["noise_frames"].tolist() == [Kn, Kn, Kn, 0, 0] and got["audio_len"].tolist() == [2 * hop, 2 * hop, n - last * hop, 0, 0]
    one = _lib.lib().sed_event_mvdr_noise_ring_workspace_bytes(2, C, MF, hop, Kn)
    sliced = feature.event_mvdr_ring(ring, cap, [n, 0], C, ev, 1, doa, mv, sr=SR, hop=hop, max_workspace_bytes=one)
    assert np.array_equal(_bits(sliced["audio"]), _bits(ref["audio"])) and torch.equal(sliced["noise_frames"], ref["noise_frames"])
    own = feature.event_mvdr_ring(ring, cap, [n, 0], C, ev, 1, doa, sed.MVDR(1e-2), sr=SR, hop=hop)
    assert "noise_frames" not in own and not np.array_equal(_bits(own["audio"]), _bits(got["audio"]))


# ───────────── 4. the purpose ─────────────
def test_it_keeps_the_suppression_the_reference_has(sed):
    """the scene of tests/test_cpu_mvdr_noise.py: a 6 cm tetrahedron, the target sounds in blocks [20, 32) only, Kn = 8, G = 1,
    no steering error.  The kernel is given the mix; its interferer part is its output minus the target and the noise as the
    float64 reference passes them through the reference's weights.  Its output SIR is the reference's within 0.1 dB (the bound
    of tests/test_gpu_mvdr.py) and at least 3 dB above the own-frames beam's (Kn = 0) on the same event."""
    from sed_crnn_amd import feature
    C, Kn, G = 4, 8, 1
    pos, xs, xi, xn = mvdr_noise_ref.onset_scene(0.06)
    u = doa_ref.unit(*mvdr_ref.TARGET)
    grid = sed.DirectionGrid(np.concatenate([sed.DirectionGrid.sphere(50).unit_vectors, u[None, :]]))
    doa = sed.DOA(pos, grid, max_frames=MAX_FRAMES)
    mix = xs + xi + xn
    f0, f1 = mvdr_noise_ref.EVENT
    rows, dirs, loc = [(f0, f1, f0 + 6)], [50], [12]
    tau = doa.steering(mvdr_noise_ref.SR)
    pcm, clips = _planar(mix)
    sir = {}
    for kn in (Kn, 0):
        y_ref, (ys, yi, yn), used = mvdr_noise_ref.event(mix, f0 * B, 12 * B, tau[50], 1e-2, kn, G, through=(xs, xi, xn))
        out = feature.event_mvdr(pcm, clips, C, _located(rows, None, dirs, loc), 1, doa, sed.MVDR(1e-2, noise_blocks=kn, noise_guard=G),
                                 sr=mvdr_noise_ref.SR, hop=B)
        y = out["audio"].cpu().numpy()
        assert y.shape == (12 * B,) and used == kn and (kn == 0 or out["noise_frames"].tolist() == [kn])
        sir[kn] = (mvdr_ref.db(ys, y.astype(np.float64) - ys - yn), mvdr_ref.db(ys, yi))
        print(f"Kn={kn}: output SIR kernel {sir[kn][0]:.3f} dB, float64 reference {sir[kn][1]:.3f} dB; max |kernel - reference| "
              f"{np.abs(y - y_ref).max():.2e}")
        assert abs(sir[kn][0] - sir[kn][1]) <= 0.1
    assert sir[Kn][0] - sir[0][0] >= 3.0


# ───────────── 5. the detector and the live feed ─────────────
def _noise_detector(sed, det2, max_frames, **kw):
    plain, _ = det2
    doa = sed.DOA(doa_ref.line(2, 0.08), sed.DirectionGrid.ring(72), max_frames=max_frames, oversample=8)
    return sed.EventDetector(plain.model, max_batch=1, median=3, mean=plain.mean, std=plain.std, localize=doa, **kw), doa


def test_detector_entry_points_carry_the_audio_and_noise_frames(sed, det2):
    """det(wave), detect_many, res[i], with_decoder and from_features + det.localize of a detector with MVDR(noise_blocks=8): audio,
    audio_start, audio_len and noise_frames are feature.event_mvdr's on the kept PCM, bit for bit; a detector with Kn = 0
    returns what it did"""
    from sed_crnn_amd import feature
    from sed_crnn_amd.resample import resample_many
    plain, x = det2
    mv = sed.MVDR(0.1, noise_blocks=8)
    det, doa = _noise_detector(sed, det2, 48, extract=mv)
    before, _ = _noise_detector(sed, det2, 48)
    own, _ = _noise_detector(sed, det2, 48, extract=sed.MVDR(0.1))
    a, b, o = det(x, sr=48000, channels=2), before(x, sr=48000, channels=2), own(x, sr=48000, channels=2)
    assert len(b) > 0 and set(a.events) == set(b.events) | {"audio_start", "audio_len", "noise_frames"}
    assert set(o.events) == set(b.events) | {"audio_start", "audio_len"} and not hasattr(o, "noise_frames") and not hasattr(b, "noise_frames")
    pcm, clips = resample_many([x], 48000, det.sr, 2, "cuda", keep_channels=True)
    want = feature.event_mvdr(pcm, clips, 2, b.events, det.model.time_factor, doa, mv, sr=det.sr, hop=det.hop_length)
    assert want["audio"].numel() > 0 and np.array_equal(_bits(a.audio), _bits(want["audio"]))
    for k in ("audio_start", "audio_len", "noise_frames"):
        assert torch.equal(a.events[k], want[k]), k
    assert a.noise_frames is a.events["noise_frames"] and a.noise_frames.dtype == torch.int32
    assert set(a.noise_frames.tolist()) <= {0, 8} and 8 in a.noise_frames.tolist()
    assert torch.equal(o.events["audio_len"], a.events["audio_len"]) and not torch.equal(o.audio, a.audio)
    again = det.with_decoder(median=3)(x, sr=48000, channels=2)
    assert np.array_equal(_bits(again.audio), _bits(a.audio)) and torch.equal(again.noise_frames, a.noise_frames)

    def same(r, one, what):
        assert set(r.events) == set(one.events), what
        for k in one.events:
            if k != "audio_start":
                assert np.array_equal(_bits(r.events[k]), _bits(one.events[k])), (what, k)
        for e in range(len(one)):
            assert np.array_equal(_bits(r.event_audio(e)), _bits(one.event_audio(e))), (what, e)

    waves = [x, _stereo(48000 * 2 + 5, 48000, 2), _stereo(30000, 48000, 3)]
    res = det.detect_many(waves, sr=[48000] * 3, channels=2)
    assert res.noise_frames.shape == res.events["cls"].shape
    for i, w in enumerate(waves):
        same(res[i], det(w, sr=48000, channels=2), f"detect_many clip {i}")
        assert torch.equal(res[i].noise_frames, res.noise_frames[res.event_offsets[i]:res.event_offsets[i + 1]])
    mel = feature.mbe(x, input_sr=48000, channels=2, keep_channels=True, device="cuda", mean=det.mean, std=det.std)
    bare = det.from_features(mel)
    assert "noise_frames" not in bare.events and not hasattr(bare, "noise_frames")
    same(det.localize(plain.from_features(mel), x, sr=48000, channels=2), a, "localize after from_features")
    empty = det.detect_many([], channels=2)
    assert empty.noise_frames.shape == (0,) and empty.noise_frames.dtype == torch.int32


def test_stream_carries_the_offline_audio_and_noise_frames(sed, det2):
    """two feeds, history "min" (max_frames + lat + nf; the rings wrap), in fine and in coarse pieces, MVDR(noise_blocks=8): every
    event that comes with audio carries the audio and the noise_frames of det(wave), bit for bit; localize.stream_extracts says
    which do.  Among the emitted events at least one uses the noise covariance and at least one is located but refused by the
    extended rule alone (it keeps its dir and has no audio); the chunking changes no bit"""
    from sed_crnn_amd.localize import stream_extracts, stream_locates
    mv = sed.MVDR(noise_blocks=8)
    det, doa = _noise_detector(sed, det2, 8, extract=mv)
    recs = [_stereo(48000 * 8, 48000, 10), _stereo(48000 * 8 + 4001, 48000, 11)]
    offline = [det(w, sr=48000, channels=2) for w in recs]
    tf, hop, runs = det.model.time_factor, det.hop_length, []
    for sizes in (SIZES, COARSE):
        st = det.stream(2, history_frames="min", max_new_windows=1, input_sr=48000, emit_audio=True)
        assert st.history_frames == 8 + st.lat + st.noise_frames and st.noise_frames == -(-10 * 1024 // hop)
        assert 2 * st.cap < recs[0].shape[0] * det.sr // 48000               # the ring wraps at least twice
        outs = _feed(st, recs, sizes) + [st.flush()]
        used = {}
        for o in outs:
            assert {"audio_start", "audio_len", "dir", "noise_frames"} <= set(o.events) and o.noise_frames.dtype == torch.int32
            ev = {k: v.cpu().numpy() for k, v in o.events.items()}
            for e in range(len(o)):
                used[(int(ev["stream"][e]), int(ev["cls"][e]), int(ev["onset"][e]))] = int(ev["noise_frames"][e])
        got = _audio_by_event(outs, 2)
        n_audio = n_noise = n_refused = 0
        for s, (one, w) in enumerate(zip(offline, recs)):
            want = {k: v.cpu().numpy() for k, v in one.events.items()}
            n_feat = 1 + sed.resample(w, 48000, channels=2, keep_channels=True).shape[1] // hop
            assert sorted((c, a) for f, c, a in got if f == s) == sorted(zip(want["cls"].tolist(), want["onset"].tolist()))
            for e in range(len(one)):
                a, b, p = int(want["onset"][e]), int(want["offset"][e]), int(want["peak_frame"][e])
                key = (s, int(want["cls"][e]), a)
                d, bits = got[key]
                args = (a, b, p, tf, n_feat, 8, st.lat, st.history_frames)
                if stream_extracts(*args, hop, mv.noise_blocks, mv.noise_guard):
                    assert d == want["dir"][e] and np.array_equal(bits, _bits(one.event_audio(e))), (s, e)
                    assert used[key] == want["noise_frames"][e]
                    n_audio += int(bits.size > 0)
                    n_noise += int(bits.size > 0 and used[key] == 8)
                elif stream_locates(*args):                                  # refused by the extended rule alone: the dir stays
                    assert d == want["dir"][e] and d >= 0 and bits.size == 0 and used[key] == 0 and want["noise_frames"][e] == 8, (s, e)
                    n_refused += 1
                else:
                    assert d == -1 and bits.size == 0 and used[key] == 0, (s, e)
        print(f"pieces {sizes[:3]}..: {n_audio} events with audio, {n_noise} of them from the noise covariance, {n_refused} refused by "
              f"the extended rule alone")
        assert n_noise >= 1 and n_refused >= 1
        runs.append((got, used))
    assert set(runs[0][0]) == set(runs[1][0]) and runs[0][1] == runs[1][1]
    for k in runs[0][0]:                                                      # the chunking changes no bit
        assert runs[0][0][k][0] == runs[1][0][k][0] and np.array_equal(runs[0][0][k][1], runs[1][0][k][1]), k
    empty = det.stream(2, history_frames="min", max_new_windows=1, input_sr=48000, emit_audio=True).push([None, None])
    assert len(empty) == 0 and empty.audio.shape == (0,) and empty.noise_frames.shape == (0,) and empty.noise_frames.dtype == torch.int32
