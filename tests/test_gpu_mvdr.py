"""Per-event audio by an adaptive (MVDR) beam on the MI355X: feature.event_mvdr against the float64 definition
(tests/mvdr_ref.py), identical channels reproduced, the batch / a permuted table / a neighbour / the slicing / the samples outside
the event bit for bit, the suppression of a second source against the reference's and against the delay-and-sum beam's, and the
detector's entry points.

Measured on an MI355X over the 8 cases of test_audio_matches_the_float64_definition (audio against float64): kernel error
1.5e-7 .. 9.8e-7, float32 yardstick 1.2e-7 .. 9.8e-7, kernel / yardstick 0.93 .. 1.30 of the 8 allowed (worst: C = 2, loading
1e2: kernel 2.46e-7, yardstick 1.89e-7); no yardstick was degenerate.  test_identical_channels_come_back: 0.67 .. 2.00 over the 9
extracted events (2.00 on an event of one block: kernel 2.4e-7, yardstick 1.2e-7).  test_it_suppresses_a_second_source: output
SIR 10.075 dB from the kernel, 10.075 dB from the float64 reference, -5.315 dB from the delay-and-sum beam.  """
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import beam_ref  # noqa: E402
import doa_ref  # noqa: E402
import mvdr_ref  # noqa: E402
from test_cpu_mvdr import SIR_MARGIN_DB  # noqa: E402
from test_gpu_beam import HOP, LOCATED, MAX_FRAMES, N, REC, ROWS, SR, _edge_table, _frames, _located, _np, _recording, _slices  # noqa: E402
from test_gpu_doa import _array, _buffers  # noqa: E402
from test_gpu_multichannel import _stereo, det2  # noqa: E402,F401
from test_gpu_tdoa import DEGENERATE, _bits, _planar  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def sed():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    import sed_crnn_amd as s
    return s


def _one_recording(rows, rec):
    return [r if k == 0 else (99, 100, 99) for r, k in zip(rows, rec)]          # (the reference takes one recording)


# ───────────── 1. against float64 ─────────────
@pytest.mark.parametrize("loading", [1e-2, 1e2])
@pytest.mark.parametrize("C", [2, 3, 4, 8])
def test_audio_matches_the_float64_definition(sed, C, loading):
    """max |audio - float64| within 8 x the float32 yardstick's (mvdr_ref.beamform with f32=True; one below 1e-9 is replaced by
    2^-24, test_gpu_tdoa's rule) over all edge rows; audio_start and audio_len are localize.event_samples'"""
    from sed_crnn_amd import feature
    doa = sed.DOA(_array(C), sed.DirectionGrid.sphere(200), max_frames=MAX_FRAMES)
    x = _recording(C)
    dirs, loc = _edge_table(200, seed=C)
    pcm, clips = _buffers(x)
    got = _np(feature.event_mvdr(pcm, clips, C, _located(ROWS, REC, dirs, loc), 1, doa, sed.MVDR(loading), sr=SR, hop=HOP))
    assert got["audio"].dtype == np.float32 and got["audio_start"].dtype == np.int64 and got["audio_len"].dtype == np.int32
    want_len = []
    for r, k, d, lf in zip(ROWS, REC, dirs, loc):
        s0, s1 = sed.event_samples(*r, 1, N, HOP, MAX_FRAMES, d if k == 0 else -1, lf)
        want_len.append(s1 - s0)
    assert got["audio_len"].tolist() == want_len and want_len[:8] == [HOP, 5 * HOP, 12 * HOP, 3 * HOP, 2 * HOP, 0, 0, 0]
    assert got["audio_start"].tolist() == np.concatenate([[0], np.cumsum(want_len)[:-1]]).tolist()
    assert got["audio"].shape == (sum(want_len),) and np.isfinite(got["audio"]).all()
    tau = doa.steering(SR)
    rows = _one_recording(ROWS, REC)
    ref = mvdr_ref.beamform(x, rows, dirs, loc, 1, HOP, MAX_FRAMES, tau, loading)
    yard = mvdr_ref.beamform(x, rows, dirs, loc, 1, HOP, MAX_FRAMES, tau, loading, f32=True)
    assert np.array_equal(ref["audio_len"], got["audio_len"]) and np.array_equal(ref["audio_start"], got["audio_start"])
    e_yard = np.abs(yard["audio"].astype(np.float64) - ref["audio"]).max()
    e_kernel = np.abs(got["audio"].astype(np.float64) - ref["audio"]).max()
    degenerate = e_yard < DEGENERATE
    if degenerate:
        e_yard = 2.0 ** -24
    print(f"C={C} loading={loading:g}: yardstick {e_yard:.2e}{' (degenerate: replaced)' if degenerate else ''}  kernel {e_kernel:.2e}  "
          f"ratio {e_kernel / e_yard:.2f}")
    assert e_kernel <= 8.0 * e_yard, (C, loading, e_kernel, e_yard)


# ───────────── 2. reconstruction ─────────────
def test_identical_channels_come_back(sed):
    """4 identical channels on a line along x, grid row 0 along y: every tau is 0, every w is 1/C, and every extracted event is
    its own input samples — the windows overlap-add to 1 and the segment is zero outside, so an event of one frame is covered
    too — to 8 x the error the float32 yardstick has on the same input, event by event"""
    from sed_crnn_amd import feature
    C = 4
    pos = beam_ref.line_along(np.array([1.0, 0.0, 0.0]), [-0.06, -0.02, 0.02, 0.06])
    grid = sed.DirectionGrid(np.array([[0.0, 1.0, 0.0], [1.0, 0.0, 0.0]]))
    doa = sed.DOA(pos, grid, max_frames=MAX_FRAMES)
    tau = doa.steering(SR)
    assert not tau[0].any() and tau[1].any()
    x = np.repeat((0.3 * np.random.default_rng(21).standard_normal((N, 1))).astype(np.float32), C, axis=1)
    dirs, loc = [0 if ok else -1 for ok in LOCATED], _frames(ROWS, REC, N)
    pcm, clips = _buffers(x)
    got = feature.event_mvdr(pcm, clips, C, _located(ROWS, REC, dirs, loc), 1, doa, sed.MVDR(1e-2), sr=SR, hop=HOP)
    yard = mvdr_ref.beamform(x, _one_recording(ROWS, REC), dirs, loc, 1, HOP, MAX_FRAMES, tau, 1e-2, f32=True)
    o, n_checked = _np(got), 0
    for e, (s, n) in enumerate(zip(o["audio_start"], o["audio_len"])):
        if n == 0:
            continue
        s0, s1 = sed.event_samples(*ROWS[e], 1, N, HOP, MAX_FRAMES, dirs[e], loc[e])
        want = x[s0:s1, 0].astype(np.float64)
        e_yard = np.abs(yard["audio"][s:s + n].astype(np.float64) - want).max()
        e_kernel = np.abs(o["audio"][s:s + n].astype(np.float64) - want).max()
        e_yard = 2.0 ** -24 if e_yard < DEGENERATE else e_yard
        print(f"event {e} ({n} samples): yardstick {e_yard:.2e}  kernel {e_kernel:.2e}  ratio {e_kernel / e_yard:.2f}")
        assert e_kernel <= 8.0 * e_yard, (e, e_kernel, e_yard)
        n_checked += 1
    assert n_checked == 9 and HOP in o["audio_len"].tolist()


# ───────────── 3. invariances ─────────────
def test_batch_permutation_neighbours_slices_and_the_outside_change_no_bit(sed):
    from sed_crnn_amd import _lib, feature
    C = 3
    doa = sed.DOA(_array(C), sed.DirectionGrid.sphere(200), max_frames=MAX_FRAMES)
    mv = sed.MVDR(1e-2)
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
        singles.append(feature.event_mvdr(pcm, clips, C, _located(rows, None, d, lf), 1, doa, mv, **kw))
    assert singles[2]["audio_len"].tolist() == [1] and singles[1]["audio_len"].tolist() == [8 * HOP + 9000 % HOP, HOP, 9000]
    # the digital silence of recording 0 (row 6 of its table: frames [22, 23)) is located here: R = 0 in every bin, w = d / C, audio 0
    quiet = [r for r, k in zip(ROWS, REC) if k == 0].index((22, 23, 22))
    silent = _slices(singles[0])[quiet].view(np.float32)
    assert dirs[0][quiet] >= 0 and silent.size == HOP and not silent.any()          # (+0 or -0)
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
    host = np.concatenate(pieces)
    buf = torch.from_numpy(host).cuda()
    rows = [r for t in tables for r in t]
    rec = [i for i, t in enumerate(tables) for _ in t]
    d_all, l_all = [v for d in dirs for v in d], [v for lf in locs for v in lf]
    many = feature.event_mvdr(buf, clips, C, _located(rows, rec, d_all, l_all), 1, doa, mv, **kw)
    want = [p for one in singles for p in _slices(one)]
    got = _slices(many)
    assert len(got) == len(want) == len(rows)
    for e, (a, b) in enumerate(zip(got, want)):                                      # the batch and the clip's place in the buffer
        assert np.array_equal(a, b), ("batch", e)
    assert many["audio_start"].tolist() == np.concatenate([[0], np.cumsum(many["audio_len"].cpu().numpy())[:-1]]).tolist()
    perm = np.random.default_rng(0).permutation(len(rows))
    shuffled = feature.event_mvdr(buf, clips, C, _located([rows[i] for i in perm], [rec[i] for i in perm], [d_all[i] for i in perm],
                                                          [l_all[i] for i in perm]), 1, doa, mv, **kw)
    for j, p in enumerate(_slices(shuffled)):
        assert np.array_equal(p, got[perm[j]]), ("permuted", j)
    d_one = list(d_all)
    d_one[4] = -1                                                                    # one more event loses its direction ...
    fewer = _slices(feature.event_mvdr(buf, clips, C, _located(rows, rec, d_one, l_all), 1, doa, mv, **kw))
    assert fewer[4].size == 0 and fewer[1].size == 0 and got[4].size > 0
    for e in range(len(rows)):                                                       # ... and no other event changes
        assert e == 4 or np.array_equal(fewer[e], got[e]), ("neighbour", e)
    # 1 and 5 events per workspace
    tab = _lib.lib().sed_event_beam_workspace_bytes(len(waves), C)
    per_event = _lib.lib().sed_event_mvdr_workspace_bytes(len(waves), C, MAX_FRAMES, HOP) - tab
    for n_ev in (1, 5):
        sliced = feature.event_mvdr(buf, clips, C, _located(rows, rec, d_all, l_all), 1, doa, mv, max_workspace_bytes=tab + n_ev * per_event, **kw)
        for e, p in enumerate(_slices(sliced)):
            assert np.array_equal(p, got[e]), ("slices of", n_ev, e)
    # the samples outside [s0, s1) of event 2 (recording 0, frames [14, 26)): every other sample of its recording is replaced
    s0, s1 = sed.event_samples(*rows[2], 1, N, HOP, MAX_FRAMES, d_all[2], l_all[2])
    assert (s0, s1) == (14 * HOP, 26 * HOP)
    other = host.copy()
    for c in range(C):
        o = first[(0, c)]
        other[o:o + s0] = 5.0
        other[o + s1:o + N] = -3.0
    alone = _slices(feature.event_mvdr(torch.from_numpy(other).cuda(), clips, C, _located(rows, rec, d_all, l_all), 1, doa, mv, **kw))
    assert np.array_equal(alone[2], got[2]) and not np.array_equal(alone[3], got[3])
    none = feature.event_mvdr(buf, clips, C, _located(np.zeros((0, 3)), [], [], []), 1, doa, mv, **kw)
    assert none["audio"].shape == (0,) and none["audio"].dtype == torch.float32 and none["audio_start"].shape == (0,)
    assert none["audio_start"].dtype == torch.int64 and none["audio_len"].dtype == torch.int32
    nothing = feature.event_mvdr(buf, clips, C, _located(rows, rec, [-1] * len(rows), l_all), 1, doa, mv, **kw)
    assert nothing["audio"].shape == (0,) and not nothing["audio_len"].any() and not nothing["audio_start"].any()


# ───────────── 4. the purpose ─────────────
def test_it_suppresses_a_second_source(sed):
    """the two-source scene of test_cpu_mvdr on a 6 cm tetrahedron, the event's 12 blocks.  The weights are a function of the
    mix and live on the device, so the kernel is given the mix; its interferer part is its output minus the signal and the
    noise as the float64 reference passes them through the reference's weights (the beam is linear once they are fixed), and its
    output SIR — the reference's signal part over that — is the reference's within 0.1 dB.  The delay-and-sum beam has fixed
    weights: the three go through feature.event_beamform one by one, and the MVDR beam's output SIR is at least SIR_MARGIN_DB above"""
    from sed_crnn_amd import feature
    C = 4
    pos, u = doa_ref.tetrahedron(0.06), doa_ref.unit(*mvdr_ref.TARGET)
    grid = sed.DirectionGrid(np.concatenate([sed.DirectionGrid.sphere(50).unit_vectors, u[None, :]]))
    doa = sed.DOA(pos, grid, max_frames=MAX_FRAMES)
    xs, xi, xn = mvdr_ref.scene(20 * HOP, pos, SR)
    mix = xs + xi + xn
    rows, dirs, loc = [(4, 16, 10)], [50], [12]
    tau = doa.steering(SR)
    y_ref, (ys, yi, yn) = mvdr_ref.event(mix, 4 * HOP, 12 * HOP, tau[50], 1e-2, through=(xs, xi, xn))
    pcm, clips = _planar(mix)
    y = feature.event_mvdr(pcm, clips, C, _located(rows, None, dirs, loc), 1, doa, sed.MVDR(1e-2), sr=SR, hop=HOP)["audio"].cpu().numpy()
    assert y.shape == (12 * HOP,)
    sir_ref, sir_kernel = mvdr_ref.db(ys, yi), mvdr_ref.db(ys, y.astype(np.float64) - ys - yn)
    fixed = []
    for part in (xs, xi):
        pcm, clips = _planar(part)
        fixed.append(feature.event_beamform(pcm, clips, C, _located(rows, None, dirs, loc), 1, doa, sed.DelaySum(16, 16), sr=SR, hop=HOP)["audio"].cpu().numpy())
    sir_das = mvdr_ref.db(fixed[0], fixed[1])
    print(f"output SIR: kernel {sir_kernel:.3f} dB, float64 reference {sir_ref:.3f} dB, delay-and-sum {sir_das:.3f} dB; "
          f"max |kernel - reference| {np.abs(y - y_ref).max():.2e}")
    assert abs(sir_kernel - sir_ref) <= 0.1
    assert sir_kernel - sir_das >= SIR_MARGIN_DB


# ───────────── 5. the detector ─────────────
def test_detector_entry_points_carry_the_audio(sed, det2):
    """det(wave), detect_many and from_features + det.localize of an MVDR detector: audio, audio_start and audio_len are
    feature.event_mvdr's on the kept PCM, bit for bit; res[i] shares the batch buffer; det.stream refuses"""
    from sed_crnn_amd import feature
    from sed_crnn_amd.resample import resample_many
    plain, x = det2
    doa = sed.DOA(doa_ref.line(2, 0.08), sed.DirectionGrid.ring(72), max_frames=48, oversample=8)
    mv = sed.MVDR(0.1)
    kw = dict(max_batch=1, median=3, mean=plain.mean, std=plain.std, localize=doa)
    det, before = sed.EventDetector(plain.model, extract=mv, **kw), sed.EventDetector(plain.model, **kw)
    a, b = det(x, sr=48000, channels=2), before(x, sr=48000, channels=2)
    assert len(b) > 0 and set(a.events) == set(b.events) | {"audio_start", "audio_len"} and b.audio is None
    for k in b.events:
        assert np.array_equal(_bits(a.events[k]), _bits(b.events[k])), k
    pcm, clips = resample_many([x], 48000, det.sr, 2, "cuda", keep_channels=True)
    want = feature.event_mvdr(pcm, clips, 2, b.events, det.model.time_factor, doa, mv, sr=det.sr, hop=det.hop_length)
    assert want["audio"].numel() > 0 and np.array_equal(_bits(a.audio), _bits(want["audio"]))
    assert torch.equal(a.events["audio_start"], want["audio_start"]) and torch.equal(a.events["audio_len"], want["audio_len"])
    other = feature.event_beamform(pcm, clips, 2, b.events, det.model.time_factor, doa, sed.DelaySum(8, 8), sr=det.sr, hop=det.hop_length)
    assert torch.equal(other["audio_len"], want["audio_len"]) and not torch.equal(other["audio"], want["audio"])   # the same samples, another beam
    starts, lens = want["audio_start"].tolist(), want["audio_len"].tolist()
    for e in range(len(a)):
        assert torch.equal(a.event_audio(e), want["audio"][starts[e]:starts[e] + lens[e]])

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
    mel = feature.mbe(x, input_sr=48000, channels=2, keep_channels=True, device="cuda", mean=det.mean, std=det.std)
    bare = det.from_features(mel)
    assert "audio_start" not in bare.events and bare.audio is None
    later = det.localize(plain.from_features(mel), x, sr=48000, channels=2)
    same(later, a, "localize after from_features")
    assert torch.equal(later.events["audio_start"], a.events["audio_start"])
    empty = det.detect_many([], channels=2)
    assert empty.audio.shape == (0,) and empty.events["audio_start"].shape == (0,) and empty.events["audio_len"].dtype == torch.int32
    with pytest.raises(NotImplementedError, match="extract"):
        det.stream(1, history_frames="min")
