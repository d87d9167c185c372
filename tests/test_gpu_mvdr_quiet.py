"""The MVDR beam with its noise frames picked where the event's class is silent, on the MI355X: feature.event_mvdr and
feature.event_quiet_frames with sed.MVDR(noise_select="quiet") against the numpy restatement of the rule and the float64
definition (tests/mvdr_quiet_ref.py); the bit identities — an isolated event is the fixed stretch's, a fallback the own-frames
beam's, the batch, a permuted table, the slicing, every sample outside the events and their selected frames —; the purpose on
the scene of tests/test_cpu_mvdr_quiet.py; and the detector's entry points.

One table per recording (_table) holds: an isolated event; an event right after a same-class event that ends inside the fixed
stretch; an event longer than max_frames, whose s0 lies inside itself; an event near the start that finds fewer than Kn
candidates; an event whose pre-onset frames an other-class event covers; an unlocated row that still marks activity; an event
behind an activity longer than S blocks; an event clipped at n; a row of a class the table does not count.

Measured on an MI355X over the 27 cases of test_frames_are_the_rules_and_audio_matches_the_float64_definition (audio against
float64): kernel error 3.1e-7 .. 5.4e-6, float32 yardstick 3.0e-7 .. 5.2e-6, kernel / yardstick 0.74 .. 1.16 of the 8 allowed
(worst: C = 3, Kn = 33, tf 8, hop 1024: kernel 5.91e-7, yardstick 5.11e-7); no yardstick was degenerate.
test_it_keeps_the_target_of_a_source_that_sounds_twice: output SIR 15.5965 dB from the kernel and from the float64 reference
with the selected frames, 12.5837 dB from both with the fixed stretch; target level -0.02 dB against -1.22 dB.  The detector's
one event of the stereo test clip finds all 8 frames.  """
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import doa_ref  # noqa: E402
import mvdr_noise_ref  # noqa: E402
import mvdr_quiet_ref  # noqa: E402
import mvdr_ref  # noqa: E402
from test_gpu_beam import _located, _np, _slices  # noqa: E402
from test_gpu_doa import _array  # noqa: E402
from test_gpu_multichannel import _stereo, det2  # noqa: E402,F401
from test_gpu_mvdr_noise import _noise_detector, _recording  # noqa: E402
from test_gpu_tdoa import DEGENERATE, _bits, _planar  # noqa: E402

pytestmark = pytest.mark.gpu
SR, B = 44100, 1024
N = 96 * B + 300                                    # 96 blocks and a cut one
MAX_FRAMES, S, K = 12, 70, 8                        # S: more than one wave of candidates; K classes
SETTINGS = [(1, 0), (8, 1), (33, 1)]                # (Kn, G); 33 frames are two chunks
GRIDS = [(8, 1024), (1, 1024), (1, 1001)]           # (time_factor, hop); 1001 puts events and frames on odd samples
NAMES = ("isolated", "earlier", "after", "long", "start", "covered", "cover", "marker", "marked", "wall", "behind", "clipped", "uncounted")


@pytest.fixture(scope="module")
def sed():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    import sed_crnn_amd as s
    return s


def _table(Kn, G, tf, hop, D, seed, n=N):
    """-> (rows [(onset, offset, peak)] in output frames, cls, dirs (-1: not located), loc_frames, {name: row index})"""
    from sed_crnn_amd.localize import event_frames
    H, lead = tf * hop, (G + Kn + 1) * B
    d = 1 if tf > 1 else 3                                                   # an ordinary event, in output frames
    F0 = -(-lead // H) + 1                                                   # every candidate of the fixed stretch exists from here on
    long_ = -(-(MAX_FRAMES + 8) // tf)
    Fd = max(1, lead // 2 // H)
    Fg = -(-(S + 2 * G + 6) * B // H)
    last = n // H
    spec = {"isolated": ((F0, F0 + d, F0), 0, True),
            "earlier": ((F0 + 2 - d, F0 + 2, F0 + 2 - d), 1, True), "after": ((F0 + 2, F0 + 2 + d, F0 + 2), 1, True),
            "long": ((F0, F0 + long_, F0 + long_ // 2), 2, True),
            "start": ((Fd, Fd + d, Fd), 3, True),
            "covered": ((F0 + 1, F0 + 1 + d, F0 + 1), 4, True), "cover": ((0, F0 + 1, 0), 5, False),
            "marker": ((F0 + 3 - d, F0 + 3, F0 + 3 - d), 6, False), "marked": ((F0 + 3, F0 + 3 + d, F0 + 3), 6, True),
            "wall": ((0, Fg, 1), 7, False), "behind": ((Fg, Fg + d, Fg), 7, True),
            "clipped": ((last, last + 2, last), 0, True),
            "uncounted": ((F0, F0 + d, F0), K, True)}
    assert tuple(spec) == NAMES
    rng = np.random.default_rng(seed)
    rows = [spec[k][0] for k in NAMES]
    cls = [spec[k][1] for k in NAMES]
    dirs = [int(rng.integers(0, D)) if spec[k][2] else -1 for k in NAMES]
    loc = [(lambda f: f[1] - f[0])(event_frames(*r, tf, 1 + n // hop, MAX_FRAMES)) if dr >= 0 else 0 for r, dr in zip(rows, dirs)]
    return rows, cls, dirs, loc, {k: i for i, k in enumerate(NAMES)}


def _ev(rows, rec, cls, dirs, loc):
    ev = _located(rows, rec, dirs, loc)
    ev["cls"] = torch.from_numpy(np.asarray(cls, np.int32)).cuda()
    return ev


def _mv(sed, Kn, G, M=1, exclude="same", loading=1e-2):
    return sed.MVDR(loading, noise_blocks=Kn, noise_guard=G, noise_select="quiet", noise_search=S, noise_min=M, noise_exclude=exclude)


def _scenarios_hold(ref, at, Kn, G, tf, hop, exclude, M):
    """the table does what its docstring says, by the reference's own selection"""
    used, sel, s0 = ref["noise_frames"], ref["noise_sel"], ref["s0"]
    full = list(range(Kn - 1, -1, -1))
    assert s0[at["long"]] > _table(Kn, G, tf, hop, 2, 0)[0][at["long"]][0] * tf * hop               # s0 lies inside the event
    assert used[at["wall"]] == used[at["cover"]] == used[at["marker"]] == used[at["uncounted"]] == 0
    assert ref["audio_len"][at["uncounted"]] > 0 and ref["audio_len"][at["marker"]] == 0
    assert ref["audio_len"][at["clipped"]] == N - (N // (tf * hop)) * tf * hop
    assert used[at["behind"]] == 0 and ref["audio_len"][at["behind"]] > 0                           # nothing within S blocks: the fallback
    if exclude == "same":
        assert sel[at["isolated"]].tolist() == full and sel[at["covered"]].tolist() == full
        assert 0 not in sel[at["after"]].tolist() and 0 not in sel[at["marked"]].tolist() and 0 not in sel[at["long"]].tolist()
        if Kn > 1:                                                           # fewer candidates than Kn exist: partial use, or the fallback
            assert used[at["start"]] == 0 if M == Kn else 0 < used[at["start"]] < Kn
        if M == 1:
            assert used[at["after"]] > 0 and used[at["long"]] > 0
    else:
        assert used[at["covered"]] == 0                                      # the other class covers every candidate


def _reference(x, rows, cls, dirs, loc, tf, hop, tau, Kn, G, M, exclude, f32=False, loading=1e-2):
    return mvdr_quiet_ref.beamform(x, rows, cls, dirs, loc, tf, hop, MAX_FRAMES, tau, loading, Kn, G, S, M, exclude, K, f32)


def _frames_equal(got, ref, what):
    for k in ("noise_frames", "noise_sel") + (("audio_start", "audio_len") if "audio_len" in got else ()):
        g = got[k].cpu().numpy() if isinstance(got[k], torch.Tensor) else got[k]
        assert g.shape == ref[k].shape and np.array_equal(g, ref[k]), (what, k, g.tolist(), ref[k].tolist())
    assert got["noise_frames"].dtype in (torch.int32, np.int32) and got["noise_sel"].dtype in (torch.int32, np.int32)


# ───────────── 1. the selection, 2. the audio against float64 ─────────────
@pytest.mark.parametrize("tf,hop", GRIDS)
@pytest.mark.parametrize("Kn,G", SETTINGS)
@pytest.mark.parametrize("C", [2, 3, 8])
def test_frames_are_the_rules_and_audio_matches_the_float64_definition(sed, C, Kn, G, tf, hop):
    """noise_frames, noise_sel, audio_start and audio_len equal the reference exactly, from event_mvdr and from event_quiet_frames
    alike (the latter also with noise_min = Kn and with noise_exclude="any"); max |audio - float64| within 8 x the float32
    yardstick's (mvdr_quiet_ref.beamform with f32=True; a yardstick below 1e-9 is degenerate and fails)"""
    from sed_crnn_amd import feature
    doa = sed.DOA(_array(C), sed.DirectionGrid.sphere(200), max_frames=MAX_FRAMES)
    x = _recording(C, N)
    rows, cls, dirs, loc, at = _table(Kn, G, tf, hop, 200, seed=C)
    pcm, clips = _planar(x)
    ev = _ev(rows, None, cls, dirs, loc)
    tau = doa.steering(SR)
    got = feature.event_mvdr(pcm, clips, C, ev, tf, doa, _mv(sed, Kn, G), sr=SR, hop=hop, n_classes=K)
    ref = _reference(x, rows, cls, dirs, loc, tf, hop, tau, Kn, G, 1, "same")
    _scenarios_hold(ref, at, Kn, G, tf, hop, "same", 1)
    _frames_equal(got, ref, "event_mvdr")
    assert got["noise_sel"].shape == (len(rows), Kn) and got["audio"].dtype == torch.float32
    for M, exclude in ((1, "same"), (Kn, "same"), (1, "any")):
        want = mvdr_quiet_ref.frames_of(rows, cls, dirs, loc, tf, N, hop, MAX_FRAMES, Kn, G, S, M, exclude, K)
        _scenarios_hold(want, at, Kn, G, tf, hop, exclude, M)
        _frames_equal(feature.event_quiet_frames(clips, C, ev, tf, doa, _mv(sed, Kn, G, M, exclude), K, hop=hop), want, (M, exclude))
    if hop % 2:
        assert any(int(s) % 2 for s, n in zip(ref["s0"], ref["noise_frames"]) if n)                 # frames on odd samples
    yard = _reference(x, rows, cls, dirs, loc, tf, hop, tau, Kn, G, 1, "same", f32=True)
    audio = got["audio"].cpu().numpy()
    assert audio.shape == ref["audio"].shape and np.isfinite(audio).all()
    e_yard = np.abs(yard["audio"].astype(np.float64) - ref["audio"]).max()
    e_kernel = np.abs(audio.astype(np.float64) - ref["audio"]).max()
    print(f"C={C} Kn={Kn} G={G} tf={tf} hop={hop}: yardstick {e_yard:.2e}  kernel {e_kernel:.2e}  ratio {e_kernel / max(e_yard, 1e-300):.2f}")
    assert e_yard >= DEGENERATE, ("degenerate yardstick", e_yard)
    assert e_kernel <= 8.0 * e_yard, (C, Kn, G, tf, hop, e_kernel, e_yard)


# ───────────── 3. bit identities ─────────────
def test_fixed_fallbacks_batch_permutation_slices_and_the_outside_change_no_bit(sed):
    from sed_crnn_amd import _lib, feature
    C, Kn, G, tf, hop = 3, 8, 1, 1, 1024
    doa = sed.DOA(_array(C), sed.DirectionGrid.sphere(200), max_frames=MAX_FRAMES)
    quiet, fixed, own = _mv(sed, Kn, G), sed.MVDR(1e-2, noise_blocks=Kn, noise_guard=G), sed.MVDR(1e-2)
    waves = [_recording(C, N), _recording(C, 21000, seed=1), _recording(C, 12 * B, seed=2)]
    t0 = _table(Kn, G, tf, hop, 200, seed=1)
    tables = [t0[:4], ([(12, 15, 13), (3, 9, 5), (19, 25, 20)], [0, 0, 1], [5, 60, 110], [3, 6, 2]),
              ([(10, 12, 10), (9, 12, 9)], [2, 2], [7, 9], [2, 3])]
    at = t0[4]
    kw = dict(sr=SR, hop=hop)
    singles = []
    n_fixed = n_fall = n_other = 0
    full = list(range(Kn - 1, -1, -1))
    for w, (rows, cls, d, lf) in zip(waves, tables):
        pcm, clips = _planar(w)
        ev = _ev(rows, None, cls, d, lf)
        one = feature.event_mvdr(pcm, clips, C, ev, tf, doa, quiet, n_classes=K, **kw)
        f, o = feature.event_mvdr(pcm, clips, C, ev, tf, doa, fixed, **kw), feature.event_mvdr(pcm, clips, C, ev, tf, doa, own, **kw)
        assert "noise_sel" not in f and "noise_frames" not in o and torch.equal(one["audio_len"], f["audio_len"])
        used, sel = one["noise_frames"].tolist(), one["noise_sel"].tolist()
        for e, (a, b, c) in enumerate(zip(_slices(one), _slices(f), _slices(o))):
            if not a.size:
                continue
            if sel[e] == full:                                               # the Kn nearest candidates: the fixed stretch, bit for bit
                assert f["noise_frames"][e] == Kn and np.array_equal(a, b) and not np.array_equal(a, c), e
                n_fixed += 1
            elif used[e] == 0:                                               # a fallback is the own-frames beam, bit for bit
                assert np.array_equal(a, c), e
                n_fall += 1
            else:
                assert not np.array_equal(a, b) and not np.array_equal(a, c), e
                n_other += 1
        singles.append(one)
    assert n_fixed >= 3 and n_fall >= 2 and n_other >= 3, (n_fixed, n_fall, n_other)
    # noise_min = Kn and noise_exclude = "any" on the first recording: more fallbacks, each the own-frames beam's bits
    pcm, clips = _planar(waves[0])
    rows, cls, d, lf = tables[0]
    o = _slices(feature.event_mvdr(pcm, clips, C, _ev(rows, None, cls, d, lf), tf, doa, own, **kw))
    base = singles[0]["noise_frames"].tolist()
    for M, exclude in ((Kn, "same"), (1, "any")):
        var = feature.event_mvdr(pcm, clips, C, _ev(rows, None, cls, d, lf), tf, doa, _mv(sed, Kn, G, M, exclude), n_classes=K, **kw)
        want = mvdr_quiet_ref.frames_of(rows, cls, d, lf, tf, N, hop, MAX_FRAMES, Kn, G, S, M, exclude, K)
        _frames_equal(var, want, (M, exclude))
        fell = [e for e, (u, v) in enumerate(zip(base, var["noise_frames"].tolist())) if u > 0 and v == 0 and o[e].size]
        assert fell and at["start" if M == Kn else "covered"] in fell
        for e, a in enumerate(_slices(var)):
            if var["noise_frames"][e] == 0:
                assert np.array_equal(a, o[e]), (M, exclude, e)
    # the batch: channels start at odd samples between sentinels (a read outside a clip would show)
    pieces, clips, pos, first = [], [], 0, {}
    for r, w in enumerate(waves):
        for c in range(C):
            lead = (-pos) % 4 + (3 if r == 1 else 1 if c == 1 else 0)
            pieces.append(np.full(lead, 7.0, np.float32))
            pos += lead
            clips.append((pos, w.shape[0]))
            first[(r, c)] = pos
            pieces.append(np.ascontiguousarray(w[:, c]))
            pos += w.shape[0]
    pieces.append(np.full(5, 7.0, np.float32))
    host = np.concatenate(pieces)
    buf = torch.from_numpy(host).cuda()
    rows = [r for t in tables for r in t[0]]
    rec = [i for i, t in enumerate(tables) for _ in t[0]]
    c_all, d_all, l_all = ([v for t in tables for v in t[k]] for k in (1, 2, 3))
    ev = _ev(rows, rec, c_all, d_all, l_all)
    many = feature.event_mvdr(buf, clips, C, ev, tf, doa, quiet, n_classes=K, **kw)
    want = [p for one in singles for p in _slices(one)]
    got = _slices(many)
    assert len(got) == len(want) == len(rows)
    assert torch.equal(many["noise_frames"], torch.cat([s["noise_frames"] for s in singles]))
    assert torch.equal(many["noise_sel"], torch.cat([s["noise_sel"] for s in singles]))
    for e, (a, b) in enumerate(zip(got, want)):
        assert np.array_equal(a, b), ("batch", e)
    frames_only = feature.event_quiet_frames(clips, C, ev, tf, doa, quiet, K, hop=hop)
    assert torch.equal(frames_only["noise_frames"], many["noise_frames"]) and torch.equal(frames_only["noise_sel"], many["noise_sel"])
    perm = np.random.default_rng(0).permutation(len(rows))
    shuffled = feature.event_mvdr(buf, clips, C, _ev(*([v[i] for i in perm] for v in (rows, rec, c_all, d_all, l_all))), tf, doa, quiet,
                                  n_classes=K, **kw)
    assert torch.equal(shuffled["noise_frames"].cpu(), many["noise_frames"].cpu()[perm])
    assert torch.equal(shuffled["noise_sel"].cpu(), many["noise_sel"].cpu()[perm])
    for j, p in enumerate(_slices(shuffled)):
        assert np.array_equal(p, got[perm[j]]), ("permuted", j)
    # 1 and 5 events per workspace: the activity still comes from the whole table
    frames = sum(w.shape[0] // (tf * hop) + 1 for w in waves)
    tab = _lib.lib().sed_event_quiet_frames_workspace_bytes(len(waves), C, frames, Kn)
    per_event = _lib.lib().sed_event_mvdr_quiet_workspace_bytes(len(waves), C, MAX_FRAMES, hop, Kn, frames) - tab
    assert tab > 0 and per_event == _lib.lib().sed_event_mvdr_noise_workspace_bytes(len(waves), C, MAX_FRAMES, hop, Kn) - \
        _lib.lib().sed_event_beam_workspace_bytes(len(waves), C)
    for n_ev in (1, 5):
        sliced = feature.event_mvdr(buf, clips, C, ev, tf, doa, quiet, max_workspace_bytes=tab + n_ev * per_event, n_classes=K, **kw)
        assert torch.equal(sliced["noise_frames"], many["noise_frames"]) and torch.equal(sliced["noise_sel"], many["noise_sel"])
        for e, p in enumerate(_slices(sliced)):
            assert np.array_equal(p, got[e]), ("slices of", n_ev, e)
    # every sample outside the events and their selected frames is NaN: no bit changes
    keep = np.zeros(host.shape[0], bool)
    used, sel = many["noise_frames"].tolist(), many["noise_sel"].tolist()
    for e, (r, row) in enumerate(zip(rec, rows)):
        n = waves[r].shape[0]
        s0, s1 = sed.event_samples(*row, tf, n, hop, MAX_FRAMES, d_all[e], l_all[e])
        for c in range(C):
            keep[first[(r, c)] + s0:first[(r, c)] + s1] = True
            for q in sel[e][:used[e]]:
                a = s0 - (G + 2 + q) * B
                assert 0 <= a and a + 2048 <= n
                keep[first[(r, c)] + a:first[(r, c)] + a + 2048] = True
    assert 0.2 < keep.mean() < 0.9
    holes = torch.from_numpy(np.where(keep, host, np.float32("nan"))).cuda()
    alone = feature.event_mvdr(holes, clips, C, ev, tf, doa, quiet, n_classes=K, **kw)
    holes.zero_()                                                            # (no NaN is left behind in memory that others will be given)
    assert torch.isfinite(alone["audio"]).all()
    for e, p in enumerate(_slices(alone)):
        assert np.array_equal(p, got[e]), ("outside", e)
    e = at["after"]                                                          # ... and a sample inside a selected frame changes it
    s0 = sed.event_samples(*rows[e], tf, N, hop, MAX_FRAMES, d_all[e], l_all[e])[0]
    inside = host.copy()
    inside[first[(0, 1)] + s0 - (G + 2 + sel[e][0]) * B + 700] += 0.5
    moved = _slices(feature.event_mvdr(torch.from_numpy(inside).cuda(), clips, C, ev, tf, doa, quiet, n_classes=K, **kw))
    assert not np.array_equal(moved[e], got[e])
    none = feature.event_mvdr(buf, clips, C, _ev(np.zeros((0, 3)), [], [], [], []), tf, doa, quiet, n_classes=K, **kw)
    assert none["audio"].shape == (0,) and none["noise_frames"].shape == (0,) and none["noise_sel"].shape == (0, Kn)
    nothing = feature.event_mvdr(buf, clips, C, _ev(rows, rec, c_all, [-1] * len(rows), l_all), tf, doa, quiet, n_classes=K, **kw)
    assert nothing["audio"].shape == (0,) and not nothing["noise_frames"].any() and (nothing["noise_sel"] == -1).all()
    with pytest.raises(ValueError, match="n_classes"):
        feature.event_mvdr(buf, clips, C, ev, tf, doa, quiet, **kw)
    with pytest.raises(ValueError, match="'cls'"):
        feature.event_mvdr(buf, clips, C, {k: v for k, v in ev.items() if k != "cls"}, tf, doa, quiet, n_classes=K, **kw)


# ───────────── 4. the purpose ─────────────
def test_it_keeps_the_target_of_a_source_that_sounds_twice(sed):
    """the scene of tests/test_cpu_mvdr_quiet.py: a 6 cm tetrahedron, the target sounds in blocks [8, 16) and [24, 40), the event
    is the second burst, steered 0.05 rad off, Kn = 8, G = 1.  The kernel is given the mix; its interferer part is its output
    minus the target and the noise as the float64 reference passes them through the reference's weights.  Its output SIR equals
    the reference's to 3 decimals, and the selected frames' exceeds the fixed stretch's by the 2.5 dB of the CPU test."""
    from sed_crnn_amd import feature
    C, Kn, G = 4, 8, 1
    pos, xs, xi, xn = mvdr_quiet_ref.twice_scene(0.06)
    az, el = mvdr_ref.TARGET
    grid = sed.DirectionGrid(np.concatenate([sed.DirectionGrid.sphere(50).unit_vectors, doa_ref.unit(az + 0.05, el)[None, :]]))
    doa = sed.DOA(pos, grid, max_frames=16)
    mix = xs + xi + xn
    rows, cls, dirs, loc = mvdr_quiet_ref.ROWS, mvdr_quiet_ref.CLS, [-1, 50], [0, 16]
    tau = doa.steering(mvdr_quiet_ref.SR)
    s0, length = mvdr_quiet_ref.EVENT[0] * B, mvdr_quiet_ref.EVENT[1] * B
    pcm, clips = _planar(mix)
    ev = _ev(rows, None, cls, dirs, loc)
    sir = {}
    for name, mv, qs in (("quiet", sed.MVDR(1e-2, noise_blocks=Kn, noise_guard=G, noise_select="quiet"), [18, 17, 16, 4, 3, 2, 1, 0]),
                         ("fixed", sed.MVDR(1e-2, noise_blocks=Kn, noise_guard=G), list(range(Kn - 1, -1, -1)))):
        y_ref, (ys, yi, yn) = mvdr_quiet_ref.event(mix, s0, length, tau[50], 1e-2, G, qs, through=(xs, xi, xn))
        out = feature.event_mvdr(pcm, clips, C, ev, mvdr_quiet_ref.TF, doa, mv, sr=mvdr_quiet_ref.SR, hop=mvdr_quiet_ref.HOP, n_classes=2)
        y = out["audio"].cpu().numpy()
        assert y.shape == (length,) and out["noise_frames"].tolist() == [0, Kn]
        if name == "quiet":
            assert out["noise_sel"].tolist() == [[-1] * Kn, qs]
        sir[name] = (mvdr_ref.db(ys, y.astype(np.float64) - ys - yn), mvdr_ref.db(ys, yi))
        print(f"{name}: output SIR kernel {sir[name][0]:.4f} dB, float64 reference {sir[name][1]:.4f} dB; target level "
              f"{mvdr_ref.db(ys, xs[s0:s0 + length, 0]):+.2f} dB; max |kernel - reference| {np.abs(y - y_ref).max():.2e}")
        assert abs(sir[name][0] - sir[name][1]) < 5e-4
    assert sir["quiet"][0] - sir["fixed"][0] >= 2.5


# ───────────── 5. the detector ─────────────
def test_detector_entry_points_carry_the_audio_and_the_selection(sed, det2):
    """det(wave), detect_many, res[i] and from_features + det.localize of a detector with MVDR(noise_select="quiet"): audio,
    audio_start, audio_len, noise_frames and noise_sel are feature.event_mvdr's on the kept PCM with the model's class count"""
    from sed_crnn_amd import feature
    from sed_crnn_amd.resample import resample_many
    plain, x = det2
    Kn = 8
    mv = sed.MVDR(0.1, noise_blocks=Kn, noise_select="quiet", noise_search=256)
    det, doa = _noise_detector(sed, det2, 48, extract=mv)
    before, _ = _noise_detector(sed, det2, 48)
    fixed, _ = _noise_detector(sed, det2, 48, extract=sed.MVDR(0.1, noise_blocks=Kn))
    a, b, f = det(x, sr=48000, channels=2), before(x, sr=48000, channels=2), fixed(x, sr=48000, channels=2)
    assert len(b) > 0 and set(a.events) == set(b.events) | {"audio_start", "audio_len", "noise_frames", "noise_sel"}
    assert set(f.events) == set(a.events) - {"noise_sel"}
    pcm, clips = resample_many([x], 48000, det.sr, 2, "cuda", keep_channels=True)
    n_classes = det.model.dense[-1]
    want = feature.event_mvdr(pcm, clips, 2, b.events, det.model.time_factor, doa, mv, sr=det.sr, hop=det.hop_length, n_classes=n_classes)
    assert want["audio"].numel() > 0 and np.array_equal(_bits(a.audio), _bits(want["audio"]))
    for k in ("audio_start", "audio_len", "noise_frames", "noise_sel"):
        assert torch.equal(a.events[k], want[k]), k
    assert a.noise_frames is a.events["noise_frames"] and a.events["noise_sel"].shape == (len(a), Kn) and a.events["noise_sel"].dtype == torch.int32
    ev = {k: v.cpu().numpy() for k, v in a.events.items()}                   # ... and the rule's, on the detector's own table
    rule = mvdr_quiet_ref.frames_of(list(zip(ev["onset"], ev["offset"], ev["peak_frame"])), ev["cls"], ev["dir"], ev["loc_frames"],
                                    det.model.time_factor, clips[0][1], det.hop_length, 48, Kn, mv.noise_guard, 256, 1, "same", n_classes)
    _frames_equal(want, rule, "the detector's table")
    print(f"{len(a)} events {list(zip(ev['cls'].tolist(), ev['onset'].tolist(), ev['offset'].tolist()))}: noise_frames "
          f"{a.noise_frames.tolist()}; the fixed stretch's {f.noise_frames.tolist()}")

    def same(r, one, what):
        assert set(r.events) == set(one.events), what
        for k in one.events:
            if k != "audio_start":
                assert np.array_equal(_bits(r.events[k]), _bits(one.events[k])), (what, k)
        for e in range(len(one)):
            assert np.array_equal(_bits(r.event_audio(e)), _bits(one.event_audio(e))), (what, e)

    waves = [x, _stereo(48000 * 2 + 5, 48000, 2), _stereo(30000, 48000, 3)]
    res = det.detect_many(waves, sr=[48000] * 3, channels=2)
    assert res.events["noise_sel"].shape == (res.events["cls"].shape[0], Kn)
    for i, w in enumerate(waves):
        same(res[i], det(w, sr=48000, channels=2), f"detect_many clip {i}")
        assert torch.equal(res[i].events["noise_sel"], res.events["noise_sel"][res.event_offsets[i]:res.event_offsets[i + 1]])
        assert torch.equal(res[i].noise_frames, res.noise_frames[res.event_offsets[i]:res.event_offsets[i + 1]])
    mel = feature.mbe(x, input_sr=48000, channels=2, keep_channels=True, device="cuda", mean=det.mean, std=det.std)
    same(det.localize(plain.from_features(mel), x, sr=48000, channels=2), a, "localize after from_features")
    empty = det.detect_many([], channels=2)
    assert empty.noise_frames.shape == (0,) and empty.events["noise_sel"].shape == (0, Kn) and empty.events["noise_sel"].dtype == torch.int32
