"""Direction tracks on the MI355X: feature.event_doa with sed.DOA(..., track=sed.DirectionTrack(...)) — the block rule,
the sibling's outputs bit for bit, one block = the event's own direction, every block = event_doa on the sub-event, the block
maps against float64, the path against its float32 restatement, the invariances, the ring entry, a source that moves, the
detector's entry points and a live stream.

The tables: with time_factor 1 the events are located on 1, 31, 32, 33, 47 and 48 frames, on more than max_frames, on 13 frames
clipped at the end of the recording, on none (beyond the end), on 48 frames of a recording of zeros and on 96 frames.  With
time_factor 8 an event's frames are a multiple of 8 unless it is empty or clipped, so 31, 33 and 47 cannot occur: 1 (an empty
event), 32, 8, 40, 48, 96, more than max_frames, 13 clipped, none, 48 of zeros and 96 again.

Measured on an MI355X over the 12 cases of test_block_maps_match_the_float64_definition (block map / its frames against float64):
kernel error 8.8e-8 .. 4.5e-7, float32 yardstick 5.4e-8 .. 4.7e-7, kernel / yardstick 0.68 .. 2.29 of the 8 allowed (worst: C = 2,
hop 1001, max_frames 40); no yardstick was degenerate.  The moving source through the kernels gives the reference's angles
(tests/test_cpu_doa_track.py): raw 0 0 0 0 120 0 0 0 degrees off, smoothed 0 0 0 0 5 0 0 0.  """
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import doa_ref  # noqa: E402
import doa_track_ref as trk  # noqa: E402
from test_gpu_detect import _assert_events_equal  # noqa: E402
from test_gpu_multichannel import _stereo, det2  # noqa: E402,F401
from test_gpu_resample import _feed  # noqa: E402
from test_gpu_stream_extract import _linear, _ring_of  # noqa: E402
from test_gpu_stream_tdoa import COARSE, SIZES  # noqa: E402
from test_gpu_tdoa import _bits, _events, _planar, sed  # noqa: E402,F401

pytestmark = pytest.mark.gpu
SR = 44100
N = 100 * 1024 + 300                                # samples of recording 0
N_ZERO = 48 * 1024                                  # ... and of recording 1, which is digital silence
DEGENERATE = 1e-9                                   # test_gpu_tdoa's: a float32 yardstick below this is exact arithmetic
SOURCE = doa_ref.unit(2.2, 0.0)
TF_HOP = [(8, 1024), (1, 1001)]
MF_W = [(40, 1), (96, 2), (256, 8), (256, 1)]
# (onset, offset, peak_frame) in output frames; row 9 is of recording 1, row 10 is located on 96 frames
ROWS = {1: [(3, 4, 3), (2, 33, 10), (5, 37, 6), (0, 33, 1), (10, 57, 20), (20, 68, 30), (0, 300, 60), (90, 120, 95), (150, 160, 155), (0, 48, 1), (4, 100, 50)],
        8: [(3, 3, 3), (1, 5, 2), (6, 7, 6), (2, 7, 3), (4, 10, 5), (0, 12, 5), (0, 40, 6), (11, 14, 12), (20, 22, 21), (0, 6, 1), (0, 12, 6)]}
REC = [0] * 9 + [1, 0]
LONG, CLIPPED, BEYOND, SILENT = 6, 7, 8, 9
STEPS = (15, 180, None)                             # max_step_deg


def _array(C):
    return {2: doa_ref.line(2, 0.06), 4: doa_ref.tetrahedron(0.06)}[C]


def _grid(sed, name):
    return sed.DirectionGrid.ring(24) if name == "ring24" else sed.DirectionGrid.sphere(1)      # (the smallest sphere: one direction)


_REC = {}


def _recording(C, hop):
    """(x [N, C], Pk float64, Pk float32) of a far-field burst, computed once per (C, hop)"""
    if (C, 0) not in _REC:
        _REC[C, 0] = doa_ref.far_field(N, _array(C), SOURCE, SR, seed=40 + C)
    x = _REC[C, 0]
    if (C, hop) not in _REC:
        Pk = doa_ref.whitened(x, hop)
        Pk.setflags(write=False)
        _REC[C, hop] = (Pk, doa_ref.whitened_f32(x, hop))
    return (x,) + _REC[C, hop]


def _buffers(x):
    """recording 0 = x, recording 1 = N_ZERO samples of zeros per channel"""
    pcm, clips = _planar(np.concatenate([x, np.zeros((N_ZERO, x.shape[1]), np.float32)]))
    return pcm, [(o, x.shape[0]) for o, _ in clips] + [(o + x.shape[0], N_ZERO) for o, _ in clips]


def _doa(sed, C, gridname, Q, mf, W, step, track=True):
    return sed.DOA(_array(C), _grid(sed, gridname), max_frames=mf, oversample=Q, track=sed.DirectionTrack(W, step) if track else None)


def _frames(rows, rec, tf, hop, mf):
    """the host's statement of the located frames -> [(f0, nf)]"""
    n_feat = {0: 1 + N // hop, 1: 1 + N_ZERO // hop}
    out = []
    for (a, b, pk), r in zip(rows, rec):
        f0, f1 = sed_frames(a, b, pk, tf, n_feat[r], mf)
        out.append((f0, f1 - f0))
    return out


def sed_frames(*a):
    from sed_crnn_amd.localize import event_frames
    return event_frames(*a)


def _np(got):
    return {k: v.cpu().numpy() for k, v in got.items()}


def _same_outputs(a, b, what, rows=slice(None)):
    assert set(a) == set(b), what
    for k in a:
        assert np.array_equal(_bits(a[k][rows]), _bits(b[k])), (what, k)


# ───────────── 1, 2, 3, 4, 6: the rule, the sibling's bits, one block, every block, the path ─────────────
@pytest.mark.parametrize("mf,W", MF_W)
@pytest.mark.parametrize("tf,hop", TF_HOP)
@pytest.mark.parametrize("Q", [1, 8])
@pytest.mark.parametrize("gridname", ["ring24", "sphere1"])
@pytest.mark.parametrize("C", [2, 4])
def test_track_columns(sed, C, gridname, Q, tf, hop, mf, W):
    from sed_crnn_amd import feature
    x, _, _ = _recording(C, hop)
    pcm, clips = _buffers(x)
    rows = ROWS[tf]
    ev = _events(rows, REC)
    kw = dict(sr=SR, hop=hop, return_curve=True, return_map=True)
    plain = feature.event_doa(pcm, clips, C, ev, tf, _doa(sed, C, gridname, Q, mf, W, None, track=False), **kw)
    runs = {step: feature.event_doa(pcm, clips, C, ev, tf, _doa(sed, C, gridname, Q, mf, W, step), **kw) for step in STEPS}
    D, Tm = len(_grid(sed, gridname)), trk.max_blocks(mf, W)
    want_frames = _frames(rows, REC, tf, hop, mf)
    if (tf, mf) == (1, 256):
        assert [nf for _, nf in want_frames] == [1, 31, 32, 33, 47, 48, 103, 13, 0, 48, 96]
    if (tf, mf) == (8, 256):
        assert [nf for _, nf in want_frames] == [1, 32, 8, 40, 48, 96, 101, 13, 0, 48, 96]
    assert want_frames[LONG][1] == min(mf, 1 + N // hop) and want_frames[BEYOND][1] == 0
    first = _np(runs[15])
    for step, got in runs.items():
        # 2. every TDOA and DOA output is event_doa's
        assert set(got) == set(plain) | {"trk_len", "trk_raw", "trk_dir", "trk_power", "trk_map"}
        for k in plain:
            assert np.array_equal(_bits(got[k]), _bits(plain[k])), (step, k)
        g = _np(got)
        assert g["trk_len"].dtype == np.int32 and g["trk_raw"].dtype == np.int32 and g["trk_dir"].dtype == np.int32
        assert g["trk_raw"].shape == g["trk_dir"].shape == g["trk_power"].shape == (len(rows), Tm) and g["trk_map"].shape == (len(rows), Tm, D)
        assert np.isfinite(g["trk_power"]).all() and np.isfinite(g["trk_map"]).all()
        # 1. the rule, and -1 / 0 behind it
        assert g["loc_frames"].tolist() == [nf for _, nf in want_frames]
        for e, (_, nf) in enumerate(want_frames):
            T = len(trk.blocks(nf, W))
            assert g["trk_len"][e] == T <= Tm, (e, nf)
            assert (g["trk_raw"][e, T:] == -1).all() and (g["trk_dir"][e, T:] == -1).all() and not g["trk_power"][e, T:].any() \
                and not g["trk_map"][e, T:].any(), (step, e)
            located = e not in (BEYOND, SILENT)
            assert ((g["trk_raw"][e, :T] >= 0) == located).all() and ((g["trk_power"][e, :T] != 0) == located).all(), (step, e)
            assert (g["trk_raw"][e, :T] < D).all() and (np.abs(g["trk_power"][e]) <= 1.0 + 1e-6).all()
            if located:
                assert np.array_equal(g["trk_raw"][e, :T], g["trk_map"][e, :T].argmax(1))     # numpy's argmax is the first maximum
        assert g["trk_len"][SILENT] >= 1 and not g["trk_map"][SILENT].any() and g["trk_len"][BEYOND] == 0
        # what does not depend on the smoothing is the same in the three calls
        for k in ("trk_len", "trk_raw", "trk_power", "trk_map"):
            assert np.array_equal(g[k].view(np.int32), first[k].view(np.int32)), (step, k)
        # 6. the path: the float32 restatement on the kernel's own maps, exactly
        table = _doa(sed, C, gridname, Q, mf, W, step).neighbours() or (None, None)
        for e in range(len(rows)):
            T = g["trk_len"][e]
            want = trk.track_dir(g["trk_map"][e, :T], g["trk_raw"][e, :T], *table)
            assert np.array_equal(g["trk_dir"][e, :T], want), (step, e, g["trk_dir"][e, :T], want)
        if step is None:
            assert np.array_equal(g["trk_dir"], g["trk_raw"])
    g = first
    # 3. one block: the event's own direction
    if 32 * W >= mf:
        assert Tm == 1
        assert np.array_equal(g["trk_raw"][:, 0], g["dir"]) and np.array_equal(g["trk_power"][:, 0].view(np.int32), g["doa_power"].view(np.int32))
        assert np.array_equal(g["trk_map"][:, 0].view(np.int32), g["srp"].view(np.int32))
    one = [e for e in range(len(rows)) if g["trk_len"][e] == 1]
    assert np.array_equal(g["trk_raw"][one, 0], g["dir"][one]) and np.array_equal(g["trk_map"][one, 0].view(np.int32), g["srp"][one].view(np.int32))
    # 4. every block of an event not longer than max_frames: event_doa on the expanded table of sub-events
    assert (32 * W) % tf == 0
    sub, where = [], []
    for e, ((a, b, pk), (f0, nf)) in enumerate(zip(rows, want_frames)):
        if nf == 0 or max(b - a, 0) * tf > mf:
            continue
        assert f0 == a * tf
        for blk, (start, n) in enumerate(trk.blocks(nf, W)):
            on = (f0 + start) // tf
            sub.append((on, on, pk) if b <= a else (on, -(-(f0 + start + n) // tf), on))
            where.append((e, blk))
    assert len(where) >= 5 and any(blk > 0 for _, blk in where) == (mf > 40 and Tm > 1)     # (40 frames are one block: the tail joins)
    wide = sed.DOA(_array(C), _grid(sed, gridname), max_frames=48 * W, oversample=Q)     # (takes the merged last block)
    ex = _np(feature.event_doa(pcm, clips, C, _events(sub, [REC[e] for e, _ in where]), tf, wide, sr=SR, hop=hop, return_map=True))
    for k, (e, blk) in enumerate(where):
        assert ex["loc_frames"][k] == trk.blocks(want_frames[e][1], W)[blk][1], (e, blk)
        assert ex["dir"][k] == g["trk_raw"][e, blk] and ex["doa_power"][k].view(np.int32) == g["trk_power"][e, blk].view(np.int32), (e, blk)
        assert np.array_equal(ex["srp"][k].view(np.int32), g["trk_map"][e, blk].view(np.int32)), (e, blk)


# ───────────── 5. against float64 ─────────────
@pytest.mark.parametrize("mf,W", [(40, 1), (256, 1), (96, 2)])
@pytest.mark.parametrize("tf,hop", TF_HOP)
@pytest.mark.parametrize("C", [2, 4])
def test_block_maps_match_the_float64_definition(sed, C, tf, hop, mf, W):
    """every block map / its frames within 8 x the float32 yardstick's error (doa_track_ref.block_maps with f32=True); a
    degenerate yardstick fails the test"""
    from sed_crnn_amd import feature
    Q = 8
    x, Pk64, Pk32 = _recording(C, hop)
    pcm, clips = _buffers(x)
    doa = _doa(sed, C, "ring24", Q, mf, W, 15)
    ml, J, _ = doa.plan(SR)
    J = J.astype(np.int64)
    rows = ROWS[tf]
    got = _np(feature.event_doa(pcm, clips, C, _events(rows, REC), tf, doa, sr=SR, hop=hop, return_map=True))
    e_kernel = e_yard = 0.0
    blocks = 0
    for e, (f0, nf) in enumerate(_frames(rows, REC, tf, hop, mf)):
        if REC[e] != 0 or nf == 0:
            continue
        ref, raw, power = trk.block_maps(Pk64, f0, nf, W, J, ml, Q)
        yard, _, _ = trk.block_maps(Pk32, f0, nf, W, J, ml, Q, f32=True)
        per = np.array([n for _, n in trk.blocks(nf, W)], np.float64)[:, None]
        T = len(per)
        assert got["trk_len"][e] == T
        e_yard = max(e_yard, np.abs(yard.astype(np.float64) / per - ref / per).max())
        e_kernel = max(e_kernel, np.abs(got["trk_map"][e, :T].astype(np.float64) / per - ref / per).max())
        blocks += T
    assert e_yard >= DEGENERATE, e_yard
    print(f"C={C} tf={tf} hop={hop} max_frames={mf} W={W}: {blocks} blocks, yardstick {e_yard:.2e}  kernel {e_kernel:.2e}  ratio {e_kernel / e_yard:.2f}")
    assert e_kernel <= 8.0 * e_yard, (e_kernel, e_yard)
    # the kernel's directions are, in float64, within that bound of the best; its power is the float64 power
    for e, (f0, nf) in enumerate(_frames(rows, REC, tf, hop, mf)):
        if REC[e] != 0 or nf == 0:
            continue
        ref, raw, power = trk.block_maps(Pk64, f0, nf, W, J, ml, Q)
        for b, (_, n) in enumerate(trk.blocks(nf, W)):
            d = got["trk_raw"][e, b]
            assert ref[b, d] >= ref[b].max() - 8.0 * e_yard * n, (e, b, d, raw[b])
            assert abs(float(got["trk_power"][e, b]) - ref[b, d] / (J.shape[1] * n)) <= 8.0 * e_yard + 2.0 ** -23


# ───────────── 7. bit for bit ─────────────
@pytest.mark.parametrize("C,gridname,Q,tf,hop,mf,W", [(4, "ring24", 8, 1, 1001, 256, 1), (2, "ring24", 1, 8, 1024, 96, 2), (2, "sphere1", 8, 1, 1001, 40, 1)])
def test_batch_permutation_workspaces_and_foreign_samples_change_no_bit(sed, C, gridname, Q, tf, hop, mf, W):
    from sed_crnn_amd import _lib, feature
    doa = _doa(sed, C, gridname, Q, mf, W, 15)
    x = _recording(C, hop)[0]
    waves = [x, doa_ref.far_field(50 * 1024 + 7, _array(C), doa_ref.unit(-1.0), SR, seed=3), np.zeros((N_ZERO, C), np.float32)]
    rows = ROWS[tf]
    short = [(0, 60, 20), (3, 4, 3), (10, 43, 11)] if tf == 1 else [(0, 7, 2), (3, 3, 3), (1, 6, 2)]
    tables = [rows[:SILENT] + rows[SILENT + 1:], short, rows[SILENT:SILENT + 1]]
    kw = dict(sr=SR, hop=hop, return_curve=True, return_map=True)
    singles = []
    for w, t in zip(waves, tables):
        pcm, clips = _planar(w)
        singles.append(feature.event_doa(pcm, clips, C, _events(t), tf, doa, **kw))
    pieces, clips, at = [], [], 0
    for r, w in enumerate(waves):                                                   # odd offsets, NaN sentinels between the channels
        for c in range(C):
            lead = (-at) % 4 + (3 if r == 1 else 1 if r == 2 else 0) + 4
            pieces.append(np.full(lead, np.nan, np.float32))
            at += lead
            clips.append((at, w.shape[0]))
            pieces.append(np.ascontiguousarray(w[:, c]))
            at += w.shape[0]
    pieces.append(np.full(5, np.nan, np.float32))
    buf = torch.from_numpy(np.concatenate(pieces)).cuda()
    table = [r for t in tables for r in t]
    rec = [i for i, t in enumerate(tables) for _ in t]
    many = feature.event_doa(buf, clips, C, _events(table, rec), tf, doa, **kw)
    assert torch.isfinite(many["trk_map"]).all() and torch.isfinite(many["srp"]).all()
    at = 0
    for i, one in enumerate(singles):
        _same_outputs(dict(many), one, f"recording {i} of the batch", slice(at, at + len(tables[i])))
        at += len(tables[i])
    assert bool((many["trk_len"] > 1).any()) == (mf > 40)
    perm = np.random.default_rng(0).permutation(len(table))
    shuffled = feature.event_doa(buf, clips, C, _events([table[i] for i in perm], [rec[i] for i in perm]), tf, doa, **kw)
    for k in many:
        assert np.array_equal(_bits(shuffled[k]), _bits(many[k][torch.from_numpy(perm).cuda()])), k
    # workspaces that hold one event (the least) and five
    sizes = [3, C, 0, max(w.shape[0] for w in waves), hop, mf, len(doa.grid), W, 1]
    for n_ev in (1, 5):
        sizes[2] = n_ev
        ws = _lib.lib().sed_event_doa_track_workspace_bytes(*sizes)
        assert ws > 0
        _same_outputs(feature.event_doa(buf, clips, C, _events(table, rec), tf, doa, max_workspace_bytes=ws, **kw), many, f"{n_ev} events a slice")
    _same_outputs(feature.event_doa(buf, clips, C, _events(table, rec), tf, doa, max_workspace_bytes=1, **kw), many, "the least workspace")
    # a workspace whose TDOA slice (58 events) is walked in two sub-slices (57 and 1), on the table six times over
    sizes[2] = 58
    ws = _lib.lib().sed_event_doa_track_workspace_bytes(*sizes) - 16
    six = feature.event_doa(buf, clips, C, _events(table * 6, rec * 6), tf, doa, max_workspace_bytes=ws, **kw)
    for k in many:
        assert np.array_equal(_bits(six[k]), _bits(torch.cat([many[k]] * 6))), k
    # NaN over every sample that no located frame of a reduced table reads
    few = [table[2], table[4], table[CLIPPED]]
    pcm, clips1 = _planar(x)
    clean = feature.event_doa(pcm, clips1, C, _events(few), tf, doa, **kw)
    keep = np.zeros(N, bool)
    for (a, b, pk) in few:
        f0, f1 = sed_frames(a, b, pk, tf, 1 + N // hop, mf)
        keep[max(0, f0 * hop - 1024):min(N, (f1 - 1) * hop + 1024)] = True
    assert 0 < keep.sum() < N
    dirty = x.copy()
    dirty[~keep] = np.nan
    pcm, clips1 = _planar(dirty)
    _same_outputs(feature.event_doa(pcm, clips1, C, _events(few), tf, doa, **kw), clean, "NaN outside the events' frames")
    none = feature.event_doa(buf, clips, C, _events(np.zeros((0, 3)), []), tf, doa, **kw)
    Tm = trk.max_blocks(mf, W)
    assert none["trk_len"].shape == (0,) and none["trk_raw"].shape == none["trk_dir"].shape == none["trk_power"].shape == (0, Tm)
    assert none["trk_map"].shape == (0, Tm, len(doa.grid)) and none["trk_dir"].dtype == torch.int32


# ───────────── 8. the ring ─────────────
@pytest.mark.parametrize("step", [15, None])
def test_ring_entry_equals_the_linear_one(sed, step):
    """C = 2, hop 1001: a ring of 51348 samples after 102700 has wrapped twice; the newest 48 frames make two blocks, the second
    one across the wrap point at sample 102696; the second feed stays NaN"""
    from sed_crnn_amd import feature
    from sed_crnn_amd.localize import stream_locates
    C, hop, cap, mf, W, LAT, HIST = 2, 1001, 51348, 256, 1, 3, 60
    x = _recording(C, hop)[0]
    doa = _doa(sed, C, "ring24", 8, mf, W, step)
    ring = _ring_of(x, cap, (1, 2047, 30000, 40000, 30652), feeds=2)
    n_feat = 1 + N // hop
    last = n_feat - 1
    assert 2 * cap <= N and (last * hop - 1024) // cap != (last * hop + 1023) // cap          # the newest frame straddles the wrap
    rows = [(last - 47, n_feat, last - 3), (last, n_feat, last), (last - 40, last - 7, last - 20), (last - 51, n_feat, last), (10, 20, 12),
            (last - 30, last + 40, last), (last - 3, n_feat, last)]
    rec = [0] * 6 + [1]
    want = []
    for (a, b, pk), r in zip(rows, rec):
        f0, f1 = sed_frames(a, b, pk, 1, n_feat, mf)
        want.append(r == 0 and stream_locates(a, b, pk, 1, n_feat, mf, LAT, HIST) and max(0, f0 * hop - 1024) >= N - cap)
    assert want == [True, True, True, False, False, False, False]
    ev = _events(rows, rec)
    kw = dict(sr=SR, hop=hop, return_curve=True, return_map=True)
    got = feature.event_doa_ring(ring, cap, [N, 0], C, ev, 1, doa, lat_frames=LAT, history_frames=HIST, **kw)
    pcm, clips = _linear(x)
    ref = feature.event_doa(pcm, clips, C, _events(rows[:3]), 1, doa, **kw)
    assert set(got) == set(ref) and ref["trk_len"].tolist() == [2, 1, 1]
    for k in ref:
        assert np.array_equal(_bits(got[k][:3]), _bits(ref[k])), k
        assert torch.isfinite(got[k].float()).all(), k
    assert not got["trk_len"][3:].any() and (got["trk_raw"][3:] == -1).all() and (got["trk_dir"][3:] == -1).all()
    assert not got["trk_power"][3:].any() and not got["trk_map"][3:].any() and (got["dir"][3:] == -1).all()
    plain = feature.event_doa_ring(ring, cap, [N, 0], C, ev, 1, _doa(sed, C, "ring24", 8, mf, W, None, track=False), lat_frames=LAT,
                                   history_frames=HIST, **kw)
    for k in plain:
        assert np.array_equal(_bits(got[k]), _bits(plain[k])), k


# ───────────── 9. a source that moves ─────────────
def test_kernel_follows_a_moving_source_past_a_louder_one(sed):
    """tests/test_cpu_doa_track.py's scene and its three assertions, through the kernels"""
    from sed_crnn_amd import feature
    pos, grid = doa_ref.tetrahedron(0.06), sed.DirectionGrid.ring(72)
    doa = sed.DOA(pos, grid, oversample=8, track=sed.DirectionTrack(1, 15))
    pcm, clips = _planar(trk.scene(pos, SR))
    got = _np(feature.event_doa(pcm, clips, 4, _events([(0, 256, 128)]), 1, doa, sr=SR, hop=1024, return_map=True))
    assert got["loc_frames"][0] == 256 and got["trk_len"][0] == 8
    truth = [doa_ref.unit(a) for a in trk.scene_truth()]
    u = grid.unit_vectors
    near = doa_ref.covering_radius(u, in_plane=True) + math.radians(5.0)
    e0, e7 = (math.degrees(doa_ref.angle_between(u[got["dir"][0]], truth[b])) for b in (0, 7))
    print(f"single direction {got['dir'][0]}: {e0:.2f} deg from the source in block 0, {e7:.2f} deg in block 7")
    assert max(e0, e7) > 15.0
    err = [doa_ref.angle_between(u[d], t) for d, t in zip(got["trk_raw"][0], truth)]
    print("raw track, degrees off:", np.round(np.degrees(err), 2).tolist())
    assert all(e <= near for b, e in enumerate(err) if b != 4) and err[4] > math.radians(60.0)
    err = [doa_ref.angle_between(u[d], t) for d, t in zip(got["trk_dir"][0], truth)]
    print("smoothed track, degrees off:", np.round(np.degrees(err), 2).tolist())
    assert all(e <= near for e in err)
    assert np.array_equal(got["trk_dir"][0], trk.track_dir(got["trk_map"][0], got["trk_raw"][0], *doa.neighbours()))


# ───────────── 10. the detector ─────────────
TRACK_KEYS = ("trk_len", "trk_raw", "trk_dir", "trk_power")


def _same(a, b, what):
    assert torch.equal(a.probs, b.probs), what
    _assert_events_equal({k: v.cpu().numpy() for k, v in a.events.items()}, {k: v.cpu().numpy() for k, v in b.events.items()}, what)
    assert set(a.events) == set(b.events), what
    for k in ("lag", "strength", "loc_frames", "dir", "doa_power") + TRACK_KEYS:
        assert np.array_equal(_bits(a.events[k]), _bits(b.events[k])), (what, k)


def test_detector_entry_points_carry_the_track(sed, det2):
    from sed_crnn_amd import feature
    from sed_crnn_amd.resample import resample_many
    plain, x = det2
    doa = sed.DOA(doa_ref.line(2, 0.08), sed.DirectionGrid.ring(72), max_frames=96, oversample=8, track=sed.DirectionTrack(1, 15))
    bare = sed.DOA(doa_ref.line(2, 0.08), sed.DirectionGrid.ring(72), max_frames=96, oversample=8)
    kw = dict(max_batch=1, median=3, mean=plain.mean, std=plain.std)
    det, ddet = sed.EventDetector(plain.model, localize=doa, **kw), sed.EventDetector(plain.model, localize=bare, **kw)
    a, b, d = det(x, sr=48000, channels=2), plain(x, sr=48000, channels=2), ddet(x, sr=48000, channels=2)
    assert len(b) > 0 and set(a.events) == set(d.events) | set(TRACK_KEYS) and a.track == (doa.track, 96, det.model.time_factor, det.hop_length)
    for k in d.events:
        assert np.array_equal(_bits(a.events[k]), _bits(d.events[k])), k
    pcm, clips = resample_many([x], 48000, det.sr, 2, "cuda", keep_channels=True)
    want = feature.event_doa(pcm, clips, 2, b.events, det.model.time_factor, doa, sr=det.sr, hop=det.hop_length)
    for k in want:
        assert np.array_equal(_bits(a.events[k]), _bits(want[k])), k
    assert a.events["trk_raw"].shape == (len(a), 3)
    T = a.events["trk_len"].cpu().numpy()
    nf = a.events["loc_frames"].cpu().numpy()
    assert (T >= 1).all() and T.tolist() == [len(trk.blocks(n, 1)) for n in nf]
    print(f"{len(a)} events, located on {nf.tolist()} frames, blocks {T.tolist()}")
    for e in range(len(a)):
        t = a.doa_track(e)
        assert t.shape == (T[e], 4)
        dirs = a.events["trk_dir"][e, :T[e]].cpu().numpy()
        assert (dirs >= 0).all() and np.array_equal(t[:, 1], doa.grid.azimuth[dirs]) and not t[:, 2].any()
        assert np.array_equal(t[:, 3], a.events["trk_power"][e, :T[e]].cpu().numpy().astype(np.float64))
        f0 = sed_frames(int(a.events["onset"][e]), int(a.events["offset"][e]), int(a.events["peak_frame"][e]), det.model.time_factor,
                        1 + clips[0][1] // det.hop_length, 96)[0]
        centre = [(f0 + s + (n - 1) / 2.0) * det.hop_length / det.sr for s, n in trk.blocks(int(nf[e]), 1)]
        np.testing.assert_allclose(t[:, 0], centre, rtol=0, atol=1e-12)
    with pytest.raises(ValueError, match="track="):
        d.doa_track(0)
    waves = [x, _stereo(48000 * 2 + 5, 48000, 2), _stereo(30000, 48000, 3)]
    res = det.detect_many(waves, sr=[48000] * 3, channels=2)
    assert res.grid is doa.grid and res.track == a.track
    for i, w in enumerate(waves):
        _same(res[i], det(w, sr=48000, channels=2), f"detect_many clip {i}")
    assert np.array_equal(res[0].doa_track(0), a.doa_track(0), equal_nan=True) and np.array_equal(res.doa_track(0), a.doa_track(0), equal_nan=True)
    mel = feature.mbe(x, input_sr=48000, channels=2, keep_channels=True, device="cuda", mean=det.mean, std=det.std)
    assert "trk_len" not in det.from_features(mel).events
    _same(det.localize(plain.from_features(mel), x, sr=48000, channels=2), a, "localize after from_features")
    _same(det.localize(plain.from_features_many([mel, mel]), [x, x], sr=48000)[1], a, "localize of a batch")
    _same(det.with_decoder(median=3)(x, sr=48000, channels=2), a, "with_decoder")
    empty = det.detect_many([], channels=2)
    assert empty.events["trk_len"].shape == (0,) and empty.events["trk_dir"].shape == (0, 3) and empty.track == a.track


# ───────────── 11. a live stream ─────────────
def _stream_run(sed, det, offline, recs, sizes):
    """two feeds through det.stream with history "min" in pieces of ``sizes`` -> ({(feed, class, onset): the track columns},
    located, refused), checked against the offline results"""
    from sed_crnn_amd.localize import stream_locates
    tf, mf = det.model.time_factor, det.localize_settings.max_frames
    Tm = det.localize_settings.track.max_blocks(mf)
    st = det.stream(2, history_frames="min", max_new_windows=1, input_sr=48000)
    outs = _feed(st, recs, sizes) + [st.flush()]
    got = {}
    for o in outs:
        assert set(TRACK_KEYS) <= set(o.events) and o.track == offline[0].track and o.events["trk_dir"].shape == (len(o), Tm)
        ev = _np(o.events)
        for e in range(len(o)):
            got[(int(ev["stream"][e]), int(ev["cls"][e]), int(ev["onset"][e]))] = ({k: ev[k][e] for k in TRACK_KEYS + ("dir", "loc_frames")},
                                                                                     o.doa_track(e))
    n_loc = n_ref = 0
    for s, (one, w) in enumerate(zip(offline, recs)):
        want = _np(one.events)
        n = sed.resample(w, 48000, channels=2, keep_channels=True).shape[1]
        assert sorted((c, a) for q, c, a in got if q == s) == sorted(zip(want["cls"].tolist(), want["onset"].tolist()))
        for e in range(len(one)):
            a, b, p = int(want["onset"][e]), int(want["offset"][e]), int(want["peak_frame"][e])
            mine, track = got[(s, int(want["cls"][e]), a)]
            if stream_locates(a, b, p, tf, 1 + n // det.hop_length, mf, st.lat, st.history_frames):
                for k in mine:
                    assert np.array_equal(np.asarray(mine[k]).view(np.int32), np.asarray(want[k][e]).view(np.int32)), (s, e, k)
                assert np.array_equal(track, one.doa_track(e), equal_nan=True) and len(track) == want["trk_len"][e] >= 1
                n_loc += 1
            else:                                                                   # refused by the history rule
                assert mine["trk_len"] == 0 and (mine["trk_raw"] == -1).all() and (mine["trk_dir"] == -1).all() and not mine["trk_power"].any()
                assert mine["dir"] == -1 and mine["loc_frames"] == 0 and track.shape == (0, 4) and want["trk_len"][e] >= 1
                n_ref += 1
    print(f"max_frames {mf}, pieces {sizes[:3]}..: history {st.history_frames} frames; {n_loc} events located, {n_ref} refused")
    return got, n_loc, n_ref


def test_stream_carries_the_offline_track(sed, det2):
    """two feeds, history "min", in fine and in coarse pieces: where localize.stream_locates accepts an emitted event its track
    columns are det(w)'s bit for bit and the chunking changes no bit (max_frames 96: events of up to three blocks, all located);
    an event the history rule refuses has trk_len = 0 (max_frames 8: the history is too short for the longer events)"""
    plain, _ = det2
    recs = [_stereo(48000 * 8, 48000, 10), _stereo(48000 * 8 + 4001, 48000, 11)]
    dets = {}
    for mf in (96, 8):
        doa = sed.DOA(doa_ref.line(2, 0.08), sed.DirectionGrid.ring(72), max_frames=mf, oversample=8, track=sed.DirectionTrack(1, 15))
        det = sed.EventDetector(plain.model, max_batch=1, median=3, mean=plain.mean, std=plain.std, localize=doa)
        dets[mf] = (det, [det(w, sr=48000, channels=2) for w in recs])
    fine, n_loc, _ = _stream_run(sed, *dets[96], recs, SIZES)
    coarse, n_loc2, _ = _stream_run(sed, *dets[96], recs, COARSE)
    assert n_loc == n_loc2 >= 1 and any(len(t) > 1 for _, t in fine.values())      # a track of more than one block came through
    assert set(fine) == set(coarse)
    for k in fine:
        for name in fine[k][0]:
            assert np.array_equal(np.asarray(fine[k][0][name]).view(np.int32), np.asarray(coarse[k][0][name]).view(np.int32)), (k, name)
    _, n_loc, n_ref = _stream_run(sed, *dets[8], recs, COARSE)
    assert n_loc >= 1 and n_ref >= 1
    empty = dets[96][0].stream(2, history_frames="min", max_new_windows=1, input_sr=48000).push([None, None])
    assert len(empty) == 0 and empty.events["trk_len"].shape == (0,) and empty.events["trk_raw"].shape == (0, 3)
