"""Per-event direction of arrival on the MI355X: feature.event_doa at Q = 1 against event_tdoa's own curve bit for
bit, the TDOA outputs unchanged, Q = 2, 8, 16 against the float64 definition (tests/doa_ref.py), the batch / a permuted table /
workspace slices / the detector's entry points bit for bit, and the direction of synthetic far-field sources.

Measured on an MI355X over the 12 cases of test_srp_matches_the_float64_definition (srp / loc_frames against float64): kernel
error 9.8e-8 .. 1.8e-6, float32 yardstick 6.3e-8 .. 1.1e-6, kernel / yardstick 0.52 .. 1.95 of the 8 allowed (worst: C = 3,
D = 200, Q = 2: kernel 3.6e-7, yardstick 1.9e-7); no yardstick was degenerate.  """
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import doa_ref  # noqa: E402
from test_gpu_detect import _assert_events_equal  # noqa: E402
from test_gpu_multichannel import _stereo, det2  # noqa: E402,F401
from test_gpu_tdoa import _bits, _events, _planar  # noqa: E402

pytestmark = pytest.mark.gpu
SR, HOP = 44100, 1024
N = 40 * HOP                                        # 41 feature frames
MAX_FRAMES = 36
DEGENERATE = 1e-9                                   # test_gpu_tdoa's: a float32 yardstick below this is exact arithmetic
QUIET = (20 * HOP, 24 * HOP)                        # samples set to 0: frame 22 reads nothing else
# (onset, offset, peak_frame), rec — at time_factor 1
ROWS = [(3, 4, 3),                                  # one frame
        (2, 35, 10),                                # 33 frames: two chunks
        (0, 41, 30),                                # 41 frames, more than max_frames: the 36 around the peak
        (50, 60, 55),                               # beyond the recording: no frames
        (5, 12, 8),                                 # ... and this one names a recording that does not exist (rec below)
        (22, 23, 22),                               # digital silence
        (5, 12, 8), (30, 50, 31), (0, 1, 0), (40, 41, 40), (8, 40, 39), (5, 12, 8)]
REC = [0, 0, 0, 0, 7, 0, 0, 0, 0, 0, 0, 0]
UNLOCATED, SILENT = (3, 4), 5
SOURCE = doa_ref.unit(2.2, 0.4)


@pytest.fixture(scope="module")
def sed():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    import sed_crnn_amd as s
    return s


def _array(C):
    return {2: doa_ref.line(2, 0.06), 3: doa_ref.line(3, 0.04), 4: doa_ref.tetrahedron(0.06), 5: doa_ref.line(5, 0.02),
            8: doa_ref.line(8, 0.012)}[C]


def _grid(sed, D):
    return sed.DirectionGrid.ring(72) if D == 72 else sed.DirectionGrid.sphere(D)


_REF = {}


def _recording(C, seed=0, u=SOURCE):
    """(x [N, C], Pk float64, Pk float32) of a far-field burst with a stretch of digital silence, computed once"""
    key = (C, seed)
    if key not in _REF:
        x = doa_ref.far_field(N, _array(C), u, SR, seed=10 * C + seed)
        x[QUIET[0]:QUIET[1]] = 0.0
        Pk = doa_ref.whitened(x, HOP)
        Pk.setflags(write=False)
        _REF[key] = (x, Pk, doa_ref.whitened_f32(x, HOP))
    return _REF[key]


def _buffers(x):
    """x [n, C] as recording 0 of two (the event that names recording 7 needs a rec column, which one recording does not read);
    recording 1 is 64 samples of silence per channel"""
    pcm, clips = _planar(np.concatenate([x, np.zeros((64, x.shape[1]), np.float32)]))
    return pcm, [(o, x.shape[0]) for o, _ in clips] + [(o + x.shape[0], 64) for o, _ in clips]


def _run(sed, C, D, Q, x=None, rows=ROWS, rec=REC, **kw):
    from sed_crnn_amd import feature
    doa = sed.DOA(_array(C), _grid(sed, D), max_frames=MAX_FRAMES, oversample=Q)
    pcm, clips = _buffers(_recording(C)[0] if x is None else x)
    got = feature.event_doa(pcm, clips, C, _events(rows, rec), 1, doa, sr=SR, hop=HOP, return_curve=True, return_map=True, **kw)
    return doa, got


def _check_unlocated(got, nf):
    d, pw, srp = got["dir"].cpu().numpy(), got["doa_power"].cpu().numpy(), got["srp"].cpu().numpy()
    assert d.dtype == np.int32 and np.isfinite(pw).all() and np.isfinite(srp).all()
    for e in UNLOCATED:
        assert nf[e] == 0 and d[e] == -1 and pw[e] == 0.0 and not srp[e].any()
    assert nf[SILENT] == 1 and d[SILENT] == -1 and pw[SILENT] == 0.0 and not srp[SILENT].any()
    located = np.setdiff1d(np.arange(len(d)), UNLOCATED + (SILENT,))
    assert (d[located] >= 0).all() and (d[located] < srp.shape[1]).all() and (np.abs(pw) <= 1.0 + 1e-6).all()
    return located


# ───────────── 1. Q = 1 is event_tdoa's curve, and 2. the TDOA keys are event_tdoa's ─────────────
@pytest.mark.parametrize("C,D", [(2, 72), (3, 200), (4, 72), (4, 200), (5, 200), (8, 72)])
def test_q1_steers_on_the_bits_of_event_tdoa(sed, C, D):
    """srp = sum_p acc[e, p, J + max_lag + 1] in fp32 adds in ascending p, bit for bit, with acc from event_tdoa; dir its first
    maximum; doa_power the double quotient rounded once.  C = 5 and 8: the pairs are accumulated in batches."""
    from sed_crnn_amd import feature
    doa, got = _run(sed, C, D, 1)
    ml, J, _ = doa.plan(SR)
    pcm, clips = _buffers(_recording(C)[0])
    want = feature.event_tdoa(pcm, clips, C, _events(ROWS, REC), 1, max_lag=ml, max_frames=MAX_FRAMES, hop=HOP, return_curve=True)
    for k in want:
        assert np.array_equal(_bits(got[k]), _bits(want[k])), k
    nf = want["loc_frames"].cpu().numpy()
    assert nf.tolist() == [1, 33, 36, 0, 0, 1, 7, 11, 1, 1, 32, 7]
    acc, Jd, P = want["acc"], torch.from_numpy(J.astype(np.int64)).cuda() + ml + 1, J.shape[1]
    srp = acc[:, 0, :][:, Jd[:, 0]]
    for p in range(1, P):
        srp = srp + acc[:, p, :][:, Jd[:, p]]
    assert np.array_equal(_bits(got["srp"]), _bits(srp))
    located = _check_unlocated(got, nf)
    s = srp.cpu().numpy()
    assert np.array_equal(got["dir"].cpu().numpy()[located], s[located].argmax(1))   # numpy's argmax is the first maximum
    best = s[located].max(1).astype(np.float64) / (P * nf[located].astype(np.float64))
    assert np.array_equal(got["doa_power"].cpu().numpy()[located].view(np.int32), best.astype(np.float32).view(np.int32))


@pytest.mark.parametrize("Q", [2, 8, 16])
def test_tdoa_keys_do_not_depend_on_the_steering(sed, Q):
    from sed_crnn_amd import feature
    C = 4
    doa, got = _run(sed, C, 200, Q)
    pcm, clips = _buffers(_recording(C)[0])
    want = feature.event_tdoa(pcm, clips, C, _events(ROWS, REC), 1, max_lag=doa.max_lag(SR), max_frames=MAX_FRAMES, hop=HOP, return_curve=True)
    assert set(got) == set(want) | {"dir", "doa_power", "srp"}
    for k in want:
        assert np.array_equal(_bits(got[k]), _bits(want[k])), k
    plain = feature.event_doa(pcm, clips, C, _events(ROWS, REC), 1, doa, sr=SR, hop=HOP)
    assert set(plain) == {"lag", "strength", "loc_frames", "dir", "doa_power"}
    for k in plain:
        assert np.array_equal(_bits(plain[k]), _bits(got[k])), k


# ───────────── 3. against float64 ─────────────
@pytest.mark.parametrize("Q", [2, 8, 16])
@pytest.mark.parametrize("C,D", [(2, 72), (3, 200), (4, 200), (5, 72)])
def test_srp_matches_the_float64_definition(sed, C, D, Q):
    """srp / loc_frames within 8 x the float32 yardstick's error (doa_ref.event_doa with f32=True; one below 1e-9 is replaced by
    2^-24, test_gpu_tdoa's rule), and the direction the kernel picks is, in float64, within that bound of the best: for EVERY
    located event"""
    doa, got = _run(sed, C, D, Q)
    ml, J, _ = doa.plan(SR)
    _, Pk64, Pk32 = _recording(C)
    rows = [r if rec == 0 else (99, 100, 99) for r, rec in zip(ROWS, REC)]           # (the reference takes one recording)
    ref = doa_ref.event_doa(Pk64, rows, 1, J.astype(np.int64), ml, Q, MAX_FRAMES)
    yard = doa_ref.event_doa(Pk32, rows, 1, J.astype(np.int64), ml, Q, MAX_FRAMES, f32=True)
    nf = ref["loc_frames"]
    assert np.array_equal(got["loc_frames"].cpu().numpy(), nf)
    located = _check_unlocated(got, nf)
    assert ref["dir"][SILENT] == -1 and (ref["dir"][list(UNLOCATED)] == -1).all()
    per = np.maximum(nf, 1)[:, None].astype(np.float64)
    srp = got["srp"].cpu().numpy().astype(np.float64)
    e_yard = np.abs(yard["srp"].astype(np.float64) / per - ref["srp"] / per).max()
    e_kernel = np.abs(srp / per - ref["srp"] / per).max()
    degenerate = e_yard < DEGENERATE
    if degenerate:
        e_yard = 2.0 ** -24
    print(f"C={C} D={D} Q={Q}: yardstick {e_yard:.2e}{' (degenerate: replaced)' if degenerate else ''}  kernel {e_kernel:.2e}  "
          f"ratio {e_kernel / e_yard:.2f}")
    assert e_kernel <= 8.0 * e_yard, (C, D, Q, e_kernel, e_yard)
    d = got["dir"].cpu().numpy()
    for e in located:
        assert ref["srp"][e, d[e]] >= ref["srp"][e].max() - 8.0 * e_yard * per[e, 0], (C, D, Q, e, d[e], ref["dir"][e])
        assert abs(float(got["doa_power"][e]) - ref["srp"][e, d[e]] / (J.shape[1] * nf[e])) <= 8.0 * e_yard + 2.0 ** -23


# ───────────── 4. bit for bit ─────────────
def _same_outputs(a, b, what, rows=slice(None)):
    assert set(a) == set(b)
    for k in a:
        assert np.array_equal(_bits(a[k][rows]), _bits(b[k])), (what, k)


def test_batch_permutation_and_slices_change_no_bit(sed):
    from sed_crnn_amd import feature
    C, Q = 3, 8
    doa = sed.DOA(_array(C), _grid(sed, 200), max_frames=MAX_FRAMES, oversample=Q)
    waves = [_recording(C)[0], _recording(C, 1, doa_ref.unit(-1.0, -0.2))[0][:9000], _recording(C)[0][:1]]
    tables = [[r for r, rec in zip(ROWS, REC) if rec == 0], [(0, 9, 4), (2, 3, 2), (0, 99, 1)], [(0, 1, 0)]]
    kw = dict(sr=SR, hop=HOP, return_curve=True, return_map=True)
    singles = []
    for w, rows in zip(waves, tables):
        pcm, clips = _planar(w)
        singles.append(feature.event_doa(pcm, clips, C, _events(rows), 1, doa, **kw))
    pieces, clips, at = [], [], 0
    for r, w in enumerate(waves):                                                   # the second recording's channels start at odd samples
        for c in range(C):
            lead = (-at) % 4 + (3 if r == 1 else 0)
            pieces.append(np.zeros(lead, np.float32))
            at += lead
            clips.append((at, w.shape[0]))
            pieces.append(np.ascontiguousarray(w[:, c]))
            at += w.shape[0]
    buf = torch.from_numpy(np.concatenate(pieces)).cuda()
    rows = [r for t in tables for r in t]
    rec = [i for i, t in enumerate(tables) for _ in t]
    many = feature.event_doa(buf, clips, C, _events(rows, rec), 1, doa, **kw)
    at = 0
    for i, one in enumerate(singles):
        _same_outputs({k: v for k, v in many.items()}, one, f"recording {i} of the batch", slice(at, at + len(tables[i])))
        at += len(tables[i])
    assert (many["dir"] >= 0).sum().item() == len(rows) - 2                          # all but the silent one and the one outside
    perm = np.random.default_rng(0).permutation(len(rows))
    shuffled = feature.event_doa(buf, clips, C, _events([rows[i] for i in perm], [rec[i] for i in perm]), 1, doa, **kw)
    for k in many:
        assert np.array_equal(_bits(shuffled[k]), _bits(many[k][torch.from_numpy(perm).cuda()])), k
    tiny = feature.event_doa(buf, clips, C, _events(rows, rec), 1, doa, max_workspace_bytes=1, **kw)
    _same_outputs(tiny, many, "one event per slice")
    few = feature.event_doa(buf, clips, C, _events(rows, rec), 1, doa, max_workspace_bytes=5 * 2 * 3 * 1026 * 8 + 4096, **kw)
    _same_outputs(few, many, "five events per slice")
    none = feature.event_doa(buf, clips, C, _events(np.zeros((0, 3)), []), 1, doa, **kw)
    assert none["dir"].shape == (0,) and none["dir"].dtype == torch.int32 and none["doa_power"].shape == (0,) and none["srp"].shape == (0, 200)


def _same(a, b, what):
    assert torch.equal(a.probs, b.probs), what
    _assert_events_equal({k: v.cpu().numpy() for k, v in a.events.items()}, {k: v.cpu().numpy() for k, v in b.events.items()}, what)
    assert set(a.events) == set(b.events), what
    for k in ("lag", "strength", "loc_frames", "dir", "doa_power"):
        assert np.array_equal(_bits(a.events[k]), _bits(b.events[k])), (what, k)


def test_detector_entry_points_agree(sed, det2):
    """det(wave), detect_many and from_features + det.localize: the same events, lags and directions, bit for bit; the TDOA keys
    are those of a TDOA detector; result.doa() maps them to angles"""
    from sed_crnn_amd import feature
    from sed_crnn_amd.resample import resample_many
    plain, x = det2
    doa = sed.DOA(doa_ref.line(2, 0.08), sed.DirectionGrid.ring(72), max_frames=48, oversample=8)
    det = sed.EventDetector(plain.model, max_batch=1, median=3, mean=plain.mean, std=plain.std, localize=doa)
    tdet = sed.EventDetector(plain.model, max_batch=1, median=3, mean=plain.mean, std=plain.std, localize=doa.tdoa(det.sr))
    a, b, t = det(x, sr=48000, channels=2), plain(x, sr=48000, channels=2), tdet(x, sr=48000, channels=2)
    assert len(b) > 0 and set(a.events) == set(b.events) | {"lag", "strength", "loc_frames", "dir", "doa_power"}
    for k in t.events:
        assert np.array_equal(_bits(a.events[k]), _bits(t.events[k])), k
    pcm, clips = resample_many([x], 48000, det.sr, 2, "cuda", keep_channels=True)
    want = feature.event_doa(pcm, clips, 2, b.events, det.model.time_factor, doa, sr=det.sr, hop=det.hop_length)
    for k in want:
        assert np.array_equal(_bits(a.events[k]), _bits(want[k])), k
    ang = a.doa()
    d = a.events["dir"].cpu().numpy()
    assert ang.shape == (len(a), 3) and (d >= 0).all() and np.array_equal(ang[:, 0], doa.grid.azimuth[d]) and not ang[:, 1].any()
    assert np.array_equal(ang[:, 2], a.events["doa_power"].cpu().numpy().astype(np.float64)) and a.doa(0).shape == (len(b.intervals(0)), 3)
    waves = [x, _stereo(48000 * 2 + 5, 48000, 2), _stereo(30000, 48000, 3)]
    res = det.detect_many(waves, sr=[48000] * 3, channels=2)
    assert res.grid is doa.grid
    for i, w in enumerate(waves):
        _same(res[i], det(w, sr=48000, channels=2), f"detect_many clip {i}")
    assert np.array_equal(res[0].doa(), ang)
    mel = feature.mbe(x, input_sr=48000, channels=2, keep_channels=True, device="cuda", mean=det.mean, std=det.std)
    assert "dir" not in det.from_features(mel).events
    _same(det.localize(plain.from_features(mel), x, sr=48000, channels=2), a, "localize after from_features")
    _same(det.localize(plain.from_features_many([mel, mel]), [x, x], sr=48000)[1], a, "localize of a batch")
    empty = det.detect_many([], channels=2)
    assert empty.events["dir"].shape == (0,) and empty.events["doa_power"].shape == (0,) and empty.grid is doa.grid


# ───────────── 5. physical ─────────────
@pytest.mark.parametrize("C,D,Q", [(4, 200, 8), (4, 72, 1), (3, 200, 16)])
def test_direction_of_a_synthetic_source_is_the_references(sed, C, D, Q):
    """the kernel's direction is the float64 reference's, or one whose float64 srp equals the reference's best within the
    bound of test 3; on the tetrahedron it lies within the covering radius (plus the Q = 1 excess of test_cpu_doa) of the source"""
    u = doa_ref.unit(0.7) if D == 72 else doa_ref.unit(-2.0, 0.5)
    x = doa_ref.far_field(N, _array(C), u, SR, seed=77)
    doa, got = _run(sed, C, D, Q, x=x, rows=[(0, 41, 20), (3, 4, 3), (10, 30, 12)], rec=[0, 0, 0])
    ml, J, _ = doa.plan(SR)
    rows = [(0, 41, 20), (3, 4, 3), (10, 30, 12)]
    ref = doa_ref.event_doa(doa_ref.whitened(x, HOP), rows, 1, J.astype(np.int64), ml, Q, MAX_FRAMES)
    yard = doa_ref.event_doa(doa_ref.whitened_f32(x, HOP), rows, 1, J.astype(np.int64), ml, Q, MAX_FRAMES, f32=True)
    per = ref["loc_frames"][:, None].astype(np.float64)
    bound = 8.0 * max(np.abs(yard["srp"].astype(np.float64) / per - ref["srp"] / per).max(), 2.0 ** -24)
    d = got["dir"].cpu().numpy()
    for e in range(3):
        assert d[e] == ref["dir"][e] or ref["srp"][e, d[e]] >= ref["srp"][e].max() - bound * per[e, 0], (e, d[e], ref["dir"][e])
        assert got["doa_power"][e].item() > 0.1
    if C == 4:
        cover = doa_ref.covering_radius(doa.grid.unit_vectors, in_plane=D == 72) + np.radians(3.2 if Q == 1 else 0.0)
        assert doa_ref.angle_between(doa.grid.unit_vectors[d[0]], u) <= cover, np.degrees(doa_ref.angle_between(doa.grid.unit_vectors[d[0]], u))
