"""Per-event audio by a steered delay-and-sum beam on the MI355X: feature.event_beamform against the float64
definition (tests/beam_ref.py), whole-sample delays bit for bit against shifted channels added on the CPU, the batch / a permuted
table / the clip's place / an unlocated neighbour bit for bit, the ring entry against the linear one across the wrap, the
detector's entry points, and the SNR gain on a synthetic source against the reference's.

Measured on an MI355X over the 16 cases of test_audio_matches_the_float64_definition (audio against float64): kernel error
4.8e-8 .. 2.6e-7, float32 yardstick 4.8e-8 .. 2.6e-7, kernel / yardstick 0.80 .. 1.09 of the 8 allowed (worst: C = 8, Q = 64,
H = 32: kernel 1.59e-7, yardstick 1.45e-7; at Q = 1 the kernel IS the yardstick, ratio 1.00); no yardstick was degenerate.  The
SNR gain of test_it_points: kernel 6.3090 dB, float64 reference 6.3090 dB.  """
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import beam_ref  # noqa: E402
import doa_ref  # noqa: E402
from test_gpu_doa import _array, _buffers  # noqa: E402
from test_gpu_multichannel import _stereo, det2  # noqa: E402,F401
from test_gpu_tdoa import DEGENERATE, _bits, _events, _planar  # noqa: E402

pytestmark = pytest.mark.gpu
SR, HOP = 44100, 1024
N = beam_ref.EDGE_FRAMES * HOP                      # 41 feature frames
MAX_FRAMES = beam_ref.EDGE_MAX_FRAMES
QUIET = (20 * HOP, 24 * HOP)
ROWS = [r for r, _, _ in beam_ref.EDGE_ROWS]
REC = [rec for _, rec, _ in beam_ref.EDGE_ROWS]
LOCATED = [ok for _, _, ok in beam_ref.EDGE_ROWS]
SOURCE = doa_ref.unit(2.2, 0.4)


@pytest.fixture(scope="module")
def sed():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    import sed_crnn_amd as s
    return s


_X = {}


def _recording(C):
    """x [N, C]: a far-field burst with a stretch of digital silence, made once"""
    if C not in _X:
        x = doa_ref.far_field(N, _array(C), SOURCE, SR, seed=40 + C)
        x[QUIET[0]:QUIET[1]] = 0.0
        x.setflags(write=False)
        _X[C] = x
    return _X[C]


def _frames(rows, rec, n, max_frames=MAX_FRAMES):
    from sed_crnn_amd.localize import event_frames
    return [(lambda f: f[1] - f[0])(event_frames(*r, 1, 1 + n // HOP, max_frames)) if k == 0 else 0 for r, k in zip(rows, rec)]


def _located(rows, rec, dirs, loc, extra=None):
    """the event table with the two columns event_doa adds, set by hand"""
    ev = _events(rows, rec)
    ev["dir"] = torch.from_numpy(np.asarray(dirs, np.int32)).cuda()
    ev["loc_frames"] = torch.from_numpy(np.asarray(loc, np.int32)).cuda()
    return ev


def _edge_table(D, seed=0):
    """the edge rows, a direction drawn for every located one (-1 for the others) and the frames they are located on"""
    rng = np.random.default_rng(seed)
    dirs = [int(rng.integers(0, D)) if ok else -1 for ok in LOCATED]
    return dirs, _frames(ROWS, REC, N)


def _np(out):
    return {k: v.cpu().numpy() for k, v in out.items()}


def _slices(out):
    """the per-event pieces of a result, as int32 bit patterns"""
    o = _np(out)
    return [o["audio"][s:s + n].view(np.int32) for s, n in zip(o["audio_start"], o["audio_len"])]


# ───────────── 1. against float64 ─────────────
@pytest.mark.parametrize("Q,H", [(1, 1), (4, 4), (16, 16), (64, 32)])
@pytest.mark.parametrize("C", [2, 3, 4, 8])
def test_audio_matches_the_float64_definition(sed, C, Q, H):
    """max |audio - float64| within 8 x the float32 yardstick's (beam_ref.beamform with f32=True; one below 1e-9 is replaced by
    2^-24, test_gpu_tdoa's rule) over all edge rows; audio_start and audio_len are localize.event_samples'"""
    from sed_crnn_amd import feature
    doa = sed.DOA(_array(C), sed.DirectionGrid.sphere(200), max_frames=MAX_FRAMES)
    beam = sed.DelaySum(Q, H, 10.0)
    x = _recording(C)
    dirs, loc = _edge_table(200, seed=C)
    pcm, clips = _buffers(x)
    got = _np(feature.event_beamform(pcm, clips, C, _located(ROWS, REC, dirs, loc), 1, doa, beam, sr=SR, hop=HOP))
    assert got["audio"].dtype == np.float32 and got["audio_start"].dtype == np.int64 and got["audio_len"].dtype == np.int32
    want_len = []
    for r, k, d, lf in zip(ROWS, REC, dirs, loc):
        s0, s1 = sed.event_samples(*r, 1, N, HOP, MAX_FRAMES, d if k == 0 else -1, lf)
        want_len.append(s1 - s0)
    assert got["audio_len"].tolist() == want_len and want_len[:8] == [HOP, 5 * HOP, 12 * HOP, 3 * HOP, 2 * HOP, 0, 0, 0]
    assert got["audio_start"].tolist() == np.concatenate([[0], np.cumsum(want_len)[:-1]]).tolist()
    assert got["audio"].shape == (sum(want_len),) and np.isfinite(got["audio"]).all()
    M, taps = doa.delays(SR, Q).astype(np.int64), beam.taps
    rows = [r if k == 0 else (99, 100, 99) for r, k in zip(ROWS, REC)]                # (the reference takes one recording)
    ref = beam_ref.beamform(x, rows, dirs, loc, 1, HOP, MAX_FRAMES, M, taps, Q)
    yard = beam_ref.beamform(x, rows, dirs, loc, 1, HOP, MAX_FRAMES, M, taps, Q, f32=True)
    assert np.array_equal(ref["audio_len"], got["audio_len"]) and np.array_equal(ref["audio_start"], got["audio_start"])
    e_yard = np.abs(yard["audio"].astype(np.float64) - ref["audio"]).max()
    e_kernel = np.abs(got["audio"].astype(np.float64) - ref["audio"]).max()
    degenerate = e_yard < DEGENERATE
    if degenerate:
        e_yard = 2.0 ** -24
    print(f"C={C} Q={Q} H={H}: yardstick {e_yard:.2e}{' (degenerate: replaced)' if degenerate else ''}  kernel {e_kernel:.2e}  "
          f"ratio {e_kernel / e_yard:.2f}")
    assert e_kernel <= 8.0 * e_yard, (C, Q, H, e_kernel, e_yard)


# ───────────── 2. whole-sample delays ─────────────
@pytest.mark.parametrize("C,Q", [(3, 1), (3, 16), (4, 8), (4, 64)])
def test_integer_delays_are_exact(sed, C, Q):
    """microphones on a line along the source direction, whole samples apart: only the impulse row of the filter is read, and
    audio is (((x_0 + x_1) + ...) * float32(1/C)) of the shifted channels bit for bit, whatever Q"""
    from sed_crnn_amd import feature
    k = {3: [-2, 0, 2], 4: [-3, -1, 1, 3]}[C]
    u = doa_ref.unit(0.9, -0.3)
    pos = beam_ref.line_along(u, np.asarray(k) * doa_ref.C_SOUND / SR)
    grid = sed.DirectionGrid(np.stack([doa_ref.unit(0.0), u, doa_ref.unit(-2.0, 0.5)]))
    doa = sed.DOA(pos, grid, max_frames=MAX_FRAMES)
    assert doa.delays(SR, Q)[1].tolist() == [Q * v for v in k]
    x = np.random.default_rng(C).standard_normal((N, C)).astype(np.float32)
    dirs = [1 if ok else -1 for ok in LOCATED]
    loc = _frames(ROWS, REC, N)
    pcm, clips = _buffers(x)
    got = feature.event_beamform(pcm, clips, C, _located(ROWS, REC, dirs, loc), 1, doa, sed.DelaySum(Q, 5, 7.0), sr=SR, hop=HOP)
    pieces = _slices(got)
    pad = np.concatenate([np.zeros((8, C), np.float32), x, np.zeros((8, C), np.float32)])
    n_checked = 0
    for e, (r, rec, ok) in enumerate(beam_ref.EDGE_ROWS):
        s0, s1 = sed.event_samples(*r, 1, N, HOP, MAX_FRAMES, dirs[e] if rec == 0 else -1, loc[e])
        assert pieces[e].shape == (s1 - s0,)
        if s1 == s0:
            continue
        y = np.zeros(s1 - s0, np.float32)
        for c in range(C):
            y = y + pad[8 + s0 - k[c]: 8 + s1 - k[c], c]                            # channel c hears s[n + k_c]: undo it
        y = y * np.float32(1.0 / C)
        assert np.array_equal(pieces[e], y.view(np.int32)), (C, Q, e)
        n_checked += 1
    assert n_checked == 9


# ───────────── 3. invariances ─────────────
def test_batch_permutation_place_and_neighbours_change_no_bit(sed):
    from sed_crnn_amd import feature
    C = 3
    doa = sed.DOA(_array(C), sed.DirectionGrid.sphere(200), max_frames=MAX_FRAMES)
    beam = sed.DelaySum(16, 16)
    waves = [_recording(C), doa_ref.far_field(9000, _array(C), doa_ref.unit(-1.0, -0.2), SR, seed=3), _recording(C)[:1]]
    tables = [[r for r, k in zip(ROWS, REC) if k == 0], [(0, 9, 4), (2, 3, 2), (0, 99, 1)], [(0, 1, 0)]]
    rng = np.random.default_rng(1)
    dirs = [[int(rng.integers(0, 200)) for _ in t] for t in tables]
    dirs[0][1] = -1                                                                  # an unlocated event between located ones
    locs = [_frames(t, [0] * len(t), w.shape[0]) for t, w in zip(tables, waves)]
    kw = dict(sr=SR, hop=HOP)
    singles = []
    for w, rows, d, lf in zip(waves, tables, dirs, locs):
        pcm, clips = _planar(w)
        singles.append(feature.event_beamform(pcm, clips, C, _located(rows, None, d, lf), 1, doa, beam, **kw))
    assert singles[2]["audio_len"].tolist() == [1] and singles[1]["audio_len"].tolist() == [8 * HOP + 9000 % HOP, HOP, 9000]
    pieces, clips, at = [], [], 0
    for r, w in enumerate(waves):                                                    # the second recording's channels start at odd samples
        for c in range(C):
            lead = (-at) % 4 + (3 if r == 1 else 0)
            pieces.append(np.full(lead, 7.0, np.float32))                           # (a read outside a clip would show)
            at += lead
            clips.append((at, w.shape[0]))
            pieces.append(np.ascontiguousarray(w[:, c]))
            at += w.shape[0]
    buf = torch.from_numpy(np.concatenate(pieces)).cuda()
    rows = [r for t in tables for r in t]
    rec = [i for i, t in enumerate(tables) for _ in t]
    d_all, l_all = [v for d in dirs for v in d], [v for lf in locs for v in lf]
    many = feature.event_beamform(buf, clips, C, _located(rows, rec, d_all, l_all), 1, doa, beam, **kw)
    want = [p for one in singles for p in _slices(one)]
    got = _slices(many)
    assert len(got) == len(want) == len(rows)
    for e, (a, b) in enumerate(zip(got, want)):                                      # the batch and the clip's place in the buffer
        assert np.array_equal(a, b), ("batch", e)
    assert many["audio_start"].tolist() == np.concatenate([[0], np.cumsum(many["audio_len"].cpu().numpy())[:-1]]).tolist()
    perm = np.random.default_rng(0).permutation(len(rows))
    shuffled = feature.event_beamform(buf, clips, C, _located([rows[i] for i in perm], [rec[i] for i in perm], [d_all[i] for i in perm],
                                                              [l_all[i] for i in perm]), 1, doa, beam, **kw)
    for j, p in enumerate(_slices(shuffled)):
        assert np.array_equal(p, got[perm[j]]), ("permuted", j)
    d_one = list(d_all)
    d_one[4] = -1                                                                    # one more event loses its direction ...
    fewer = _slices(feature.event_beamform(buf, clips, C, _located(rows, rec, d_one, l_all), 1, doa, beam, **kw))
    assert fewer[4].size == 0 and fewer[1].size == 0 and got[4].size > 0
    for e in range(len(rows)):                                                       # ... and no other event changes
        assert e == 4 or np.array_equal(fewer[e], got[e]), ("neighbour", e)
    none = feature.event_beamform(buf, clips, C, _located(np.zeros((0, 3)), [], [], []), 1, doa, beam, **kw)
    assert none["audio"].shape == (0,) and none["audio"].dtype == torch.float32 and none["audio_start"].shape == (0,)
    assert none["audio_start"].dtype == torch.int64 and none["audio_len"].dtype == torch.int32
    nothing = feature.event_beamform(buf, clips, C, _located(rows, rec, [-1] * len(rows), l_all), 1, doa, beam, **kw)
    assert nothing["audio"].shape == (0,) and not nothing["audio_len"].any() and not nothing["audio_start"].any()


# ───────────── 4. the ring ─────────────
def test_ring_equals_linear_bit_for_bit(sed):
    """C = 3, a ring of 12292 samples (no multiple of the hop) written in uneven pieces up to 30000 samples: it has wrapped twice.
    The events event_doa_ring located — one frame, several frames across the wrap point, the newest frame — carry the bits of
    event_beamform on the linear samples; those it refused (the stream's rule, a first sample that has left the ring, no such
    feed) come with dir = -1 and have length 0"""
    from sed_crnn_amd import feature
    from sed_crnn_amd.localize import stream_ring_samples
    C, n, MF, LAT, HIST = 3, 30000, 8, 3, 14
    cap = stream_ring_samples(8, 2, HOP, n_fft=2052)
    assert cap == 12292
    pos = doa_ref.line(C, 0.04)
    x = doa_ref.far_field(n, pos, doa_ref.unit(1.0, 0.3), SR, seed=5)
    doa = sed.DOA(pos, sed.DirectionGrid.sphere(200), max_frames=MF, oversample=8)
    beam = sed.DelaySum(16, 16)
    ring = torch.full((2 * C * cap,), float("nan"), device="cuda")          # two feeds (the second stays empty); a read of an unwritten entry would show
    at, ws = 0, None
    for m in (1, 2047, 5000, 9000, 6000, 6000, 1952):
        src = torch.from_numpy(np.concatenate([x[at:at + m, c] for c in range(C)])).cuda()
        ws = feature.ring_write(ring, cap, src, [(c * m, m, at) for c in range(C)], ws)
        at += m
    assert at == n
    last = n // HOP
    wrap = next(f for f in range(22, last) if (f * HOP - 1024) // cap != (f * HOP + 1023) // cap)
    rows = [(last, last + 1, last), (22, 23, 22), (wrap - 1, wrap + 2, wrap), (23, 29, 25), (21, 29, 28),
            (19, 20, 19), (18, 19, 18), (24, 24 + 60, 24), (0, 1, 0), (22, 23, 22)]
    rec = [0] * 9 + [3]
    ev = _events(rows, rec)
    located = feature.event_doa_ring(ring, cap, [n, 0], C, ev, 1, doa, sr=SR, hop=HOP, lat_frames=LAT, history_frames=HIST)
    d = located["dir"].cpu().numpy()
    assert (d >= 0).tolist() == [True, True, True, True, True, True, False, False, False, False]
    ev = {**ev, "dir": located["dir"], "loc_frames": located["loc_frames"]}
    got = feature.event_beamform_ring(ring, cap, [n, 0], C, ev, 1, doa, beam, sr=SR, hop=HOP)
    lin = torch.from_numpy(np.ascontiguousarray(x.T).reshape(-1)).cuda()
    lin_ev = {**_events(rows, [0] * 10), "dir": located["dir"], "loc_frames": located["loc_frames"]}
    ref = feature.event_beamform(lin, [(c * n, n) for c in range(C)], C, lin_ev, 1, doa, beam, sr=SR, hop=HOP)
    for k in ("audio", "audio_start", "audio_len"):
        assert got[k].dtype == ref[k].dtype and torch.equal(got[k], ref[k]) and (k != "audio" or np.array_equal(_bits(got[k]), _bits(ref[k]))), k
    assert torch.isfinite(got["audio"]).all()
    lens = got["audio_len"].cpu().numpy()
    assert (lens[:6] > 0).all() and not lens[6:].any() and lens[0] == n - last * HOP and lens[3] == 6 * HOP
    spans = [sed.event_samples(*r, 1, n, HOP, MF, int(d[e]), int(located["loc_frames"][e])) for e, r in enumerate(rows)]
    assert sum(1 for s0, s1 in spans if s1 > s0 and s0 // cap != (s1 - 1) // cap) >= 1       # an extracted event wraps the ring
    none = feature.event_beamform_ring(ring, cap, [n, 0], C, {**_events(np.zeros((0, 3)), []), "dir": located["dir"][:0],
                                                               "loc_frames": located["loc_frames"][:0]}, 1, doa, beam, sr=SR, hop=HOP)
    assert none["audio"].shape == (0,) and none["audio_len"].shape == (0,)


# ───────────── 5. the detector ─────────────
def test_detector_entry_points_carry_the_audio(sed, det2):
    """det(wave), detect_many and from_features + det.localize: audio, audio_start and audio_len are feature.event_beamform's on
    the kept PCM, bit for bit; without extract= the events are those of before and hold no audio keys; det.stream refuses"""
    from sed_crnn_amd import feature
    from sed_crnn_amd.resample import resample_many
    plain, x = det2
    doa = sed.DOA(doa_ref.line(2, 0.08), sed.DirectionGrid.ring(72), max_frames=48, oversample=8)
    beam = sed.DelaySum(8, 8)
    kw = dict(max_batch=1, median=3, mean=plain.mean, std=plain.std, localize=doa)
    det, before = sed.EventDetector(plain.model, extract=beam, **kw), sed.EventDetector(plain.model, **kw)
    a, b = det(x, sr=48000, channels=2), before(x, sr=48000, channels=2)
    assert len(b) > 0 and set(a.events) == set(b.events) | {"audio_start", "audio_len"} and b.audio is None
    assert "audio_start" not in b.events and "audio_len" not in b.events
    for k in b.events:
        assert np.array_equal(_bits(a.events[k]), _bits(b.events[k])), k
    with pytest.raises(ValueError, match="holds no audio"):
        b.event_audio(0)
    pcm, clips = resample_many([x], 48000, det.sr, 2, "cuda", keep_channels=True)
    want = feature.event_beamform(pcm, clips, 2, b.events, det.model.time_factor, doa, beam, sr=det.sr, hop=det.hop_length)
    assert want["audio"].numel() > 0 and np.array_equal(_bits(a.audio), _bits(want["audio"]))
    assert torch.equal(a.events["audio_start"], want["audio_start"]) and torch.equal(a.events["audio_len"], want["audio_len"])
    starts, lens = want["audio_start"].tolist(), want["audio_len"].tolist()
    for e in range(len(a)):
        assert torch.equal(a.event_audio(e), want["audio"][starts[e]:starts[e] + lens[e]])
    with pytest.raises(IndexError):
        a.event_audio(len(a))

    def same(r, one, what):
        assert set(r.events) == set(one.events), what
        for k in one.events:
            if k != "audio_start":
                assert np.array_equal(_bits(r.events[k]), _bits(one.events[k])), (what, k)
        for e in range(len(one)):
            assert np.array_equal(_bits(r.event_audio(e)), _bits(one.event_audio(e))), (what, e)

    waves = [x, _stereo(48000 * 2 + 5, 48000, 2), _stereo(30000, 48000, 3)]
    res = det.detect_many(waves, sr=[48000] * 3, channels=2)
    singles = [det(w, sr=48000, channels=2) for w in waves]
    assert res.audio.numel() == sum(s.audio.numel() for s in singles) and res.audio.data_ptr() == res[1].audio.data_ptr()
    for i, one in enumerate(singles):
        same(res[i], one, f"detect_many clip {i}")
    assert torch.equal(res.event_audio(res.event_offsets[1]), singles[1].event_audio(0)) if len(singles[1]) else True
    mel = feature.mbe(x, input_sr=48000, channels=2, keep_channels=True, device="cuda", mean=det.mean, std=det.std)
    bare = det.from_features(mel)
    assert "audio_start" not in bare.events and "dir" not in bare.events and bare.audio is None
    later = det.localize(plain.from_features(mel), x, sr=48000, channels=2)
    same(later, a, "localize after from_features")
    assert torch.equal(later.events["audio_start"], a.events["audio_start"])
    same(det.localize(plain.from_features_many([mel, mel]), [x, x], sr=48000)[1], a, "localize of a batch")
    empty = det.detect_many([], channels=2)
    assert empty.audio.shape == (0,) and empty.events["audio_start"].shape == (0,) and empty.events["audio_len"].dtype == torch.int32
    with pytest.raises(NotImplementedError, match="extract"):
        det.stream(1, history_frames="min")


# ───────────── 6. physical ─────────────
def test_it_points(sed):
    """a source band-limited to 0.8 Nyquist from a direction that is a grid row, and independent noise in every channel of a 6 cm
    tetrahedron: the SNR gain of the beam over channel 0 — the beam is linear, so the source and the noise go through it one
    after the other — is the float64 reference's on the same input within 0.1 dB (and more than 5 dB)"""
    from sed_crnn_amd import feature
    C, Q, H = 4, 16, 16
    pos, u = doa_ref.tetrahedron(0.06), SOURCE
    grid = sed.DirectionGrid(np.concatenate([sed.DirectionGrid.sphere(50).unit_vectors, u[None, :]]))
    doa = sed.DOA(pos, grid, max_frames=MAX_FRAMES)
    beam = sed.DelaySum(Q, H, 10.0)
    xs, _ = beam_ref.source(N, pos, u, SR, seed=8, band=0.8)
    xn = (0.3 * np.random.default_rng(9).standard_normal((N, C))).astype(np.float32)
    rows, dirs, loc = [(4, 16, 10), (20, 30, 22)], [50, 50], [12, 10]
    M = doa.delays(SR, Q).astype(np.int64)

    def power(v):
        return float(np.mean(np.asarray(v, np.float64) ** 2))

    gains = {}
    for who in ("kernel", "reference"):
        out = []
        for x in (xs, xn):
            if who == "kernel":
                pcm, clips = _planar(x)
                out.append(feature.event_beamform(pcm, clips, C, _located(rows, None, dirs, loc), 1, doa, beam, sr=SR, hop=HOP)["audio"].cpu().numpy())
            else:
                out.append(beam_ref.beamform(x, rows, dirs, loc, 1, HOP, MAX_FRAMES, M, beam.taps, Q)["audio"])
        assert out[0].shape == (22 * HOP,)
        seg = np.r_[4 * HOP:16 * HOP, 20 * HOP:30 * HOP]
        snr_in = power(xs[seg, 0]) / power(xn[seg, 0])
        gains[who] = 10.0 * np.log10(power(out[0]) / power(out[1]) / snr_in)
    print(f"SNR gain over channel 0: kernel {gains['kernel']:.4f} dB, float64 reference {gains['reference']:.4f} dB")
    assert abs(gains["kernel"] - gains["reference"]) <= 0.1 and gains["reference"] > 5.0
