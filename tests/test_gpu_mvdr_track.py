"""The MVDR beam steered along the event's direction track on the MI355X: feature.event_mvdr with
sed.MVDR(follow_track=True) against the float64 definition (tests/mvdr_track_ref.py); a track that stays at ``dir`` against the
untracked kernels, bit for bit; the batch, a permuted table, the slicing and the samples outside the events; the ring entry across
the wrap point; the moving-source scene; the detector's entry points and a live stream.

The track columns are made BY THE TEST — a different row per block, a silent block, a row outside the grid, a trk_len of 0 and one
larger than Tm — so that nothing here leans on the track kernels.

Measured on an MI355X (30 cases in 5 s): audio against float64, kernel error / float32 yardstick 0.96 .. 1.21 of the 8 allowed over the
17 accuracy cases (own frames 0.96 .. 1.21, Kn = 8 1.05 .. 1.21, quiet 1.18; worst: C = 4, hop 1001, max_frames 96, W = 2); no
yardstick was degenerate.  Every bit identity with the untracked kernels held.  The scene: one dir -3.787 dB / SIR 8.577 dB (last
block -8.337 / 4.704), tracked -0.024 / 12.991 (last block -0.001 / 13.886), the float64 reference's to the third decimal.  The
streams: 7 events with audio, 2 of them on more than one block, in fine and in coarse pieces, Kn = 0 and 8.  """
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import doa_ref  # noqa: E402
import mvdr_quiet_ref  # noqa: E402
import mvdr_ref  # noqa: E402
import mvdr_track_ref as ref  # noqa: E402
from test_gpu_beam import _located, _np, _slices  # noqa: E402
from test_gpu_doa import _array  # noqa: E402
from test_gpu_multichannel import _stereo, det2  # noqa: E402,F401
from test_gpu_resample import _feed  # noqa: E402
from test_gpu_stream_extract import _audio_by_event, _linear, _ring_of, _same_tables  # noqa: E402
from test_gpu_stream_tdoa import COARSE, SIZES  # noqa: E402
from test_gpu_tdoa import DEGENERATE, _bits, _planar  # noqa: E402

pytestmark = pytest.mark.gpu
SR, B = 44100, 1024
N = 100 * 1024 + 300                                # samples of recording 0
N_ZERO = 48 * 1024                                  # ... and of recording 1, which is digital silence
D = 24                                              # a ring of 24 directions
GARBAGE = 7777                                      # behind trk_len: never read
# (onset, offset, peak_frame) in output frames and the frames the event is located on (at most; max_frames and the recording cut it)
ROWS = {1: [((3, 4, 3), 1), ((20, 53, 25), 33), ((15, 62, 20), 47), ((0, 48, 1), 48), ((4, 100, 50), 96), ((0, 300, 60), 999),
            ((90, 120, 95), 999), ((10, 20, 12), 10), ((0, 48, 1), 48)],
        8: [((3, 4, 3), 1), ((2, 7, 3), 33), ((6, 12, 6), 47), ((0, 6, 1), 48), ((0, 12, 6), 96), ((0, 40, 6), 999),
            ((11, 14, 12), 999), ((2, 3, 2), 8), ((0, 6, 1), 48)]}
REC = [0] * 8 + [1]
LONG, CLIPPED, UNLOCATED, SILENT = 5, 6, 7, 8
CASES = [(C, tf, hop, mf, W, 0) for C in (2, 4) for tf, hop in ((8, 1024), (1, 1001)) for mf, W in ((40, 1), (96, 1), (96, 2))] + \
        [(8, 1, 1001, 96, 2, 0), (4, 8, 1024, 96, 1, 8), (2, 1, 1001, 40, 1, 8), (4, 1, 1001, 96, 2, 8)]


@pytest.fixture(scope="module")
def sed():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    import sed_crnn_amd as s
    return s


_X = {}


def _recording(C):
    if C not in _X:
        x = doa_ref.far_field(N, _array(C), doa_ref.unit(2.2, 0.0), SR, seed=40 + C)
        x.setflags(write=False)
        _X[C] = x
    return _X[C]


def _buffers(x):
    """recording 0 = x, recording 1 = N_ZERO samples of zeros per channel"""
    pcm, clips = _planar(np.concatenate([x, np.zeros((N_ZERO, x.shape[1]), np.float32)]))
    return pcm, [(o, x.shape[0]) for o, _ in clips] + [(o + x.shape[0], N_ZERO) for o, _ in clips]


def _doa(sed, C, mf, W):
    return sed.DOA(_array(C), sed.DirectionGrid.ring(D), max_frames=mf, track=sed.DirectionTrack(W))


def _table(sed, tf, hop, mf, W, seed, constant=False):
    """-> rows, dirs [E], loc [E], trk_len [E], trk_dir [E, Tm]: the table above with a track made here.  ``constant``: every
    row that names a direction names the event's ``dir``"""
    from sed_crnn_amd.localize import event_frames
    rng = np.random.default_rng(seed)
    rows = [r for r, _ in ROWS[tf]]
    Tm = -(-(-(-mf // 32)) // W)
    dirs, loc, tlen = [], [], []
    tdir = np.full((len(rows), Tm), GARBAGE, np.int32)
    for e, ((a, b, pk), nf) in enumerate(ROWS[tf]):
        f0, f1 = event_frames(a, b, pk, tf, 1 + (N if REC[e] == 0 else N_ZERO) // hop, mf)
        loc.append(min(nf, f1 - f0))
        dirs.append(-1 if e == UNLOCATED else int(rng.integers(0, D)))
        T = sed.track_blocks(loc[-1], W)[0]
        tlen.append(T)
        tdir[e, :T] = dirs[-1] if constant else rng.permutation(D)[:T]        # a different row per block
    assert loc[:5] == [min(n, mf) for n in (1, 33, 47, 48, 96)] and loc[LONG] == min(mf, 1 + N // hop) and 0 < loc[CLIPPED] < 32
    tlen[0] = 0                                                               # an event without a track: steered at dir
    tdir[0] = GARBAGE
    tlen[4] = Tm + 3                                                          # more blocks than the columns hold: clamped to Tm
    tdir[4] = dirs[4] if constant else rng.permutation(D)[:Tm]
    tdir[2, 0] = -1                                                           # a silent block: dir
    tdir[3, -1 if tlen[3] == Tm else tlen[3] - 1] = D + 5                     # a row outside the grid: dir
    tdir[LONG, 0] = -7
    return rows, dirs, loc, np.asarray(tlen, np.int32), tdir


def _ev(rows, rec, dirs, loc, tlen, tdir, cls=None):
    ev = _located(rows, rec, dirs, loc)
    ev["trk_len"] = torch.from_numpy(np.ascontiguousarray(tlen, dtype=np.int32)).cuda()
    ev["trk_dir"] = torch.from_numpy(np.ascontiguousarray(tdir, dtype=np.int32)).cuda()
    if cls is not None:
        ev["cls"] = torch.from_numpy(np.asarray(cls, np.int32)).cuda()
    return ev


def _one_recording(rows):
    return [r if k == 0 else (9999, 10000, 9999) for r, k in zip(rows, REC)]   # (the reference takes one recording)


def _compare(sed, got, want, yard, rows, dirs, loc, tf, hop, mf, what):
    """the spans are localize.event_samples'; the events of recording 0 against the float64 reference under the project's rule for
    these kernels (8 x the float32 yardstick's error, one below 1e-9 replaced by 2^-24); the event on zeros is zeros -> ratio"""
    g = _np(got)
    lens = []
    for e, r in enumerate(rows):
        s0, s1 = sed.event_samples(*r, tf, N if REC[e] == 0 else N_ZERO, hop, mf, dirs[e], loc[e])
        lens.append(s1 - s0)
    assert g["audio_len"].tolist() == lens and lens[UNLOCATED] == 0 and lens[SILENT] > 0 and lens[CLIPPED] % hop != 0
    assert g["audio_start"].tolist() == np.concatenate([[0], np.cumsum(lens)[:-1]]).tolist() and g["audio"].shape == (sum(lens),)
    assert np.isfinite(g["audio"]).all()
    assert want["audio_len"][:SILENT].tolist() == lens[:SILENT]
    worst = 0.0
    for e in range(SILENT):
        if lens[e] == 0:
            continue
        a, w = g["audio"][g["audio_start"][e]:][:lens[e]].astype(np.float64), want["audio"][want["audio_start"][e]:][:lens[e]]
        y = yard["audio"][want["audio_start"][e]:][:lens[e]].astype(np.float64)
        e_yard, e_kernel = np.abs(y - w).max(), np.abs(a - w).max()
        if e_yard < DEGENERATE:
            e_yard = 2.0 ** -24
        worst = max(worst, e_kernel / e_yard)
        assert e_kernel <= 8.0 * e_yard, (what, e, e_kernel, e_yard)
    assert not g["audio"][g["audio_start"][SILENT]:][:lens[SILENT]].any()     # R = 0 in every bin: w = d / C, audio 0
    return worst


# ───────────── 1. against float64 ─────────────
@pytest.mark.parametrize("C,tf,hop,mf,W,Kn", CASES)
def test_audio_matches_the_float64_definition(sed, C, tf, hop, mf, W, Kn):
    """own frames (Kn = 0) and Kn = 8, G = 1; the worst ratio of every case is printed (module docstring)"""
    from sed_crnn_amd import feature
    doa = _doa(sed, C, mf, W)
    x = _recording(C)
    rows, dirs, loc, tlen, tdir = _table(sed, tf, hop, mf, W, seed=C + mf + W)
    pcm, clips = _buffers(x)
    mv = sed.MVDR(1e-2, Kn, 1, follow_track=True)
    got = feature.event_mvdr(pcm, clips, C, _ev(rows, REC, dirs, loc, tlen, tdir), tf, doa, mv, sr=SR, hop=hop)
    assert set(got) == {"audio", "audio_start", "audio_len"} | ({"noise_frames"} if Kn else set())
    plain = feature.event_mvdr(pcm, clips, C, _located(rows, REC, dirs, loc), tf, doa, sed.MVDR(1e-2, Kn, 1), sr=SR, hop=hop)
    assert torch.equal(got["audio_len"], plain["audio_len"]) and torch.equal(got["audio_start"], plain["audio_start"])   # the spans
    assert not torch.equal(got["audio"], plain["audio"])
    if Kn:
        assert torch.equal(got["noise_frames"], plain["noise_frames"]) and int((got["noise_frames"] == Kn).sum()) >= 3
    tau = doa.steering(SR)
    one = _one_recording(rows)
    want = ref.beamform(x, one, dirs, loc, tlen, tdir, W, tf, hop, mf, tau, 1e-2, Kn, 1)
    yard = ref.beamform(x, one, dirs, loc, tlen, tdir, W, tf, hop, mf, tau, 1e-2, Kn, 1, f32=True)
    worst = _compare(sed, got, want, yard, rows, dirs, loc, tf, hop, mf, (C, tf, hop, mf, W, Kn))
    print(f"C={C} tf={tf} hop={hop} max_frames={mf} W={W} Kn={Kn}: worst kernel / yardstick {worst:.2f} of the 8 allowed")


def _quiet_case(sed, constant):
    C, tf, hop, mf, W, Kn, G, K = 4, 8, 1024, 96, 1, 8, 1, 3
    rows, dirs, loc, tlen, tdir = _table(sed, tf, hop, mf, W, seed=77, constant=constant)
    cls = [0, 1, 0, 2, 2, 2, 1, 2, 0]                                          # the rows that cover the recording do not silence the others
    mv = dict(loading=1e-2, noise_blocks=Kn, noise_guard=G, noise_select="quiet", noise_search=32)
    return C, tf, hop, mf, W, Kn, G, K, rows, dirs, loc, tlen, tdir, cls, mv


def test_quiet_audio_matches_the_float64_definition(sed):
    """the quiet selection with the tracked weights: the selection is the untracked call's (and the reference's), the audio the
    reference's under the same rule"""
    from sed_crnn_amd import feature
    C, tf, hop, mf, W, Kn, G, K, rows, dirs, loc, tlen, tdir, cls, mv = _quiet_case(sed, False)
    doa = _doa(sed, C, mf, W)
    x = _recording(C)
    pcm, clips = _buffers(x)
    got = feature.event_mvdr(pcm, clips, C, _ev(rows, REC, dirs, loc, tlen, tdir, cls), tf, doa, sed.MVDR(follow_track=True, **mv), sr=SR, hop=hop,
                             n_classes=K)
    one = _one_recording(rows)
    sel = mvdr_quiet_ref.frames_of(one, cls, dirs, loc, tf, N, hop, mf, Kn, G, 32, 1, "same", K)
    g = _np(got)
    assert np.array_equal(g["noise_frames"][:SILENT], sel["noise_frames"][:SILENT]) and np.array_equal(g["noise_sel"][:SILENT], sel["noise_sel"][:SILENT])
    assert (sel["noise_frames"] > 0).sum() >= 3 and (sel["noise_frames"][[e for e in range(SILENT) if e != UNLOCATED]] == 0).any()
    tau = doa.steering(SR)
    quiet = (sel["noise_frames"], sel["noise_sel"])
    want = ref.beamform(x, one, dirs, loc, tlen, tdir, W, tf, hop, mf, tau, 1e-2, Kn, G, quiet=quiet)
    yard = ref.beamform(x, one, dirs, loc, tlen, tdir, W, tf, hop, mf, tau, 1e-2, Kn, G, quiet=quiet, f32=True)
    worst = _compare(sed, got, want, yard, rows, dirs, loc, tf, hop, mf, "quiet")
    print(f"quiet, C={C} tf={tf} hop={hop} max_frames={mf} W={W} Kn={Kn}: worst kernel / yardstick {worst:.2f} of the 8 allowed")


# ───────────── 2. a track that stays at dir: the untracked kernels' bits ─────────────
@pytest.mark.parametrize("C,tf,hop,mf,W,Kn", [(2, 1, 1001, 96, 1, 0), (4, 8, 1024, 96, 2, 0), (8, 1, 1001, 40, 1, 0), (4, 1, 1001, 96, 1, 8),
                                              (2, 8, 1024, 40, 1, 8)])
def test_a_track_at_dir_gives_the_untracked_bits(sed, C, tf, hop, mf, W, Kn):
    """every used row equals dir — or is silent, outside the grid, or behind a trk_len of 0: own and fixed-stretch covariance"""
    from sed_crnn_amd import feature
    doa = _doa(sed, C, mf, W)
    rows, dirs, loc, tlen, tdir = _table(sed, tf, hop, mf, W, seed=5, constant=True)
    assert (tdir == GARBAGE).any() and (tdir == -1).any() and (tdir == D + 5).any() and tlen[0] == 0 and tlen[4] > tdir.shape[1]
    pcm, clips = _buffers(_recording(C))
    got = feature.event_mvdr(pcm, clips, C, _ev(rows, REC, dirs, loc, tlen, tdir), tf, doa, sed.MVDR(1e-2, Kn, 1, follow_track=True), sr=SR, hop=hop)
    plain = feature.event_mvdr(pcm, clips, C, _located(rows, REC, dirs, loc), tf, doa, sed.MVDR(1e-2, Kn, 1), sr=SR, hop=hop)
    assert set(got) == set(plain)
    for k in plain:
        assert np.array_equal(_bits(got[k].float()) if k == "audio" else got[k].cpu().numpy(),
                              _bits(plain[k].float()) if k == "audio" else plain[k].cpu().numpy()), k
    assert got["audio"].numel() > 96 * hop and torch.isfinite(got["audio"]).all()


def test_a_track_at_dir_gives_the_untracked_bits_quiet(sed):
    from sed_crnn_amd import feature
    C, tf, hop, mf, W, Kn, G, K, rows, dirs, loc, tlen, tdir, cls, mv = _quiet_case(sed, True)
    doa = _doa(sed, C, mf, W)
    pcm, clips = _buffers(_recording(C))
    got = feature.event_mvdr(pcm, clips, C, _ev(rows, REC, dirs, loc, tlen, tdir, cls), tf, doa, sed.MVDR(follow_track=True, **mv), sr=SR, hop=hop,
                             n_classes=K)
    plain = feature.event_mvdr(pcm, clips, C, _ev(rows, REC, dirs, loc, tlen, tdir, cls), tf, doa, sed.MVDR(**mv), sr=SR, hop=hop, n_classes=K)
    assert set(got) == set(plain) == {"audio", "audio_start", "audio_len", "noise_frames", "noise_sel"}
    for k in plain:
        assert torch.equal(got[k], plain[k]) and (k != "audio" or np.array_equal(_bits(got[k]), _bits(plain[k]))), k
    assert int((got["noise_frames"] > 0).sum()) >= 3


# ───────────── 3. invariances ─────────────
def test_batch_permutation_slices_and_the_outside_change_no_bit(sed):
    """three recordings at odd offsets between NaN sentinels against the single calls; a permuted table with its track rows;
    workspaces of one and of five events; NaN over every sample outside one event and its noise frames"""
    from sed_crnn_amd import _lib, feature
    C, tf, hop, mf, W, Kn, G = 3, 1, 1001, 96, 1, 8, 1
    doa = _doa(sed, C, mf, W)
    mv = sed.MVDR(1e-2, Kn, G, follow_track=True)
    Tm = doa.track.max_blocks(mf)
    waves = [doa_ref.far_field(N, _array(C), doa_ref.unit(2.2, 0.0), SR, seed=43),
             doa_ref.far_field(50 * 1001 + 9, _array(C), doa_ref.unit(-1.0, -0.2), SR, seed=3), _recording(4)[:1, :C].copy()]
    tables = [[(20, 53, 25), (3, 4, 3), (4, 100, 50), (15, 62, 20), (90, 120, 95)], [(0, 48, 4), (12, 13, 12), (0, 99, 1)], [(0, 1, 0)]]
    rng = np.random.default_rng(1)
    kw = dict(sr=SR, hop=hop)

    def track(rows, n):
        from sed_crnn_amd.localize import event_frames
        d, lf, tl, td = [], [], [], np.full((len(rows), Tm), GARBAGE, np.int32)
        for e, r in enumerate(rows):
            f0, f1 = event_frames(*r, tf, 1 + n // hop, mf)
            lf.append(f1 - f0)
            d.append(int(rng.integers(0, D)))
            T = sed.track_blocks(lf[-1], W)[0]
            tl.append(T)
            td[e, :T] = rng.permutation(D)[:T]
        return d, lf, np.asarray(tl, np.int32), td
    tr = [track(t, w.shape[0]) for t, w in zip(tables, waves)]
    tr[0][0][1] = -1                                                                 # an unlocated event between located ones
    singles = []
    for w, rows, (d, lf, tl, td) in zip(waves, tables, tr):
        pcm, clips = _planar(w)
        singles.append(feature.event_mvdr(pcm, clips, C, _ev(rows, None, d, lf, tl, td), tf, doa, mv, **kw))
    assert singles[0]["noise_frames"].tolist() == [Kn, 0, 0, Kn, Kn] and singles[2]["audio_len"].tolist() == [1]
    pieces, clips, at, first = [], [], 0, {}
    for r, w in enumerate(waves):                                                    # channels start at odd samples between sentinels
        for c in range(C):
            lead = (-at) % 4 + (3 if r == 1 else 1 if c == 1 else 0)
            pieces.append(np.full(lead, np.nan, np.float32))                        # (a read outside a clip would show)
            at += lead
            clips.append((at, w.shape[0]))
            first[(r, c)] = at
            pieces.append(np.ascontiguousarray(w[:, c]))
            at += w.shape[0]
    pieces.append(np.full(5, np.nan, np.float32))
    host = np.concatenate(pieces)
    buf = torch.from_numpy(host).cuda()
    rows = [r for t in tables for r in t]
    rec = [i for i, t in enumerate(tables) for _ in t]
    d_all, l_all = [v for t in tr for v in t[0]], [v for t in tr for v in t[1]]
    tl_all, td_all = np.concatenate([t[2] for t in tr]), np.concatenate([t[3] for t in tr])
    many = feature.event_mvdr(buf, clips, C, _ev(rows, rec, d_all, l_all, tl_all, td_all), tf, doa, mv, **kw)
    want = [p for one in singles for p in _slices(one)]
    got = _slices(many)
    assert len(got) == len(want) == len(rows) and torch.isfinite(many["audio"]).all()
    for e, (a, b) in enumerate(zip(got, want)):
        assert np.array_equal(a, b), ("batch", e)
    assert many["noise_frames"].tolist() == [v for one in singles for v in one["noise_frames"].tolist()]
    perm = np.random.default_rng(0).permutation(len(rows))
    shuffled = feature.event_mvdr(buf, clips, C, _ev([rows[i] for i in perm], [rec[i] for i in perm], [d_all[i] for i in perm],
                                                     [l_all[i] for i in perm], tl_all[perm], td_all[perm]), tf, doa, mv, **kw)
    for j, p in enumerate(_slices(shuffled)):
        assert np.array_equal(p, got[perm[j]]), ("permuted", j)
    L = _lib.lib()
    tab = L.sed_event_beam_workspace_bytes(len(waves), C)
    per_event = L.sed_event_mvdr_track_workspace_bytes(len(waves), C, mf, hop, Kn, Tm) - tab
    assert per_event > L.sed_event_mvdr_noise_workspace_bytes(len(waves), C, mf, hop, Kn) - tab
    for n_ev in (1, 5):
        sliced = feature.event_mvdr(buf, clips, C, _ev(rows, rec, d_all, l_all, tl_all, td_all), tf, doa, mv, max_workspace_bytes=tab + n_ev * per_event,
                                    **kw)
        for e, p in enumerate(_slices(sliced)):
            assert np.array_equal(p, got[e]), ("slices of", n_ev, e)
    # event 3 (recording 0, frames [15, 62)): NaN over every sample of its recording outside it and its noise frames
    s0, s1 = sed.event_samples(*rows[3], tf, N, hop, mf, d_all[3], l_all[3])
    assert (s0, s1) == (15 * hop, 62 * hop) and s0 >= (G + Kn + 1) * B and tl_all[3] >= 1
    other = host.copy()
    for c in range(C):
        o = first[(0, c)]
        other[o:o + s0 - (G + Kn + 1) * B] = np.nan
        other[o + s0 - G * B:o + s0] = np.nan
        other[o + s1:o + N] = np.nan
    alone = _slices(feature.event_mvdr(torch.from_numpy(other).cuda(), clips, C, _ev(rows, rec, d_all, l_all, tl_all, td_all), tf, doa, mv, **kw))
    assert np.array_equal(alone[3], got[3]) and not np.array_equal(alone[2], got[2])
    none = feature.event_mvdr(buf, clips, C, _ev(np.zeros((0, 3)), [], [], [], np.zeros(0, np.int32), np.zeros((0, Tm), np.int32)), tf, doa, mv, **kw)
    assert none["audio"].shape == (0,) and none["audio_start"].dtype == torch.int64 and none["noise_frames"].shape == (0,)


# ───────────── 4. the ring ─────────────
@pytest.mark.parametrize("Kn", [0, 8])
def test_ring_entry_equals_the_linear_one(sed, Kn):
    """C = 2, hop 1001: a ring of 51348 samples after 102700 has wrapped twice.  Event 0 starts at frame 69: its frame 32, the
    first of track block 1, holds the samples [100813, 102861) across the wrap point 102696.  The bits are the linear call's,
    also when the workspace holds one event"""
    from sed_crnn_amd import _lib, feature
    C, hop, cap, mf, W = 2, 1001, 51348, 96, 1
    x = _recording(C)
    doa = _doa(sed, C, mf, W)
    mv = sed.MVDR(1e-2, Kn, 1, follow_track=True)
    ring = _ring_of(x, cap, (1, 2047, 30000, 40000, 30652), feeds=2)
    rows, dirs, loc = [(69, 103, 80), (63, 99, 70), (100, 103, 101)], [5, 17, 9], [34, 36, 3]
    tlen, tdir = np.asarray([2, 2, 1], np.int32), np.asarray([[3, 20, GARBAGE], [-1, 11, GARBAGE], [D, GARBAGE, GARBAGE]], np.int32)
    s0, s1 = sed.event_samples(*rows[0], 1, N, hop, mf, dirs[0], loc[0])
    blocks = sed.mvdr_frame_blocks(s1 - s0, hop, W, 2)
    j = int(np.argmax(blocks))                                                        # the first frame of block 1
    assert 2 * cap <= N and s1 == N and blocks[j - 1] == 0 and s0 + (j - 1) * B < 2 * cap < s0 + (j + 1) * B and s0 - 11 * B >= N - cap
    ev = _ev(rows, [0, 0, 0], dirs, loc, tlen, tdir)
    got = feature.event_mvdr_ring(ring, cap, [N, 0], C, ev, 1, doa, mv, sr=SR, hop=hop)
    pcm, clips = _linear(x)
    want = feature.event_mvdr(pcm, clips, C, _ev(rows, None, dirs, loc, tlen, tdir), 1, doa, mv, sr=SR, hop=hop)
    _same_tables(got, want)
    assert got["audio_len"].tolist() == [N - 69 * hop, 36 * hop, N - 100 * hop]
    if Kn:
        assert got["noise_frames"].tolist() == want["noise_frames"].tolist() == [Kn] * 3
    one = _lib.lib().sed_event_mvdr_track_ring_workspace_bytes(2, C, mf, hop, Kn, 3)
    _same_tables(feature.event_mvdr_ring(ring, cap, [N, 0], C, ev, 1, doa, mv, sr=SR, hop=hop, max_workspace_bytes=one), want)
    still = feature.event_mvdr(pcm, clips, C, _located(rows, None, dirs, loc), 1, doa, sed.MVDR(1e-2, Kn, 1), sr=SR, hop=hop)
    assert torch.equal(still["audio_len"], want["audio_len"]) and not torch.equal(still["audio"], want["audio"])


# ───────────── 5. the purpose ─────────────
def test_the_kernels_follow_a_moving_source(sed):
    """the scene of tests/test_cpu_mvdr_track.py on the 6 cm array, own frames.  The weights are a function of the mix and live on
    the device, so the kernel is given the mix; its target part is its output minus the interferer and the noise as the float64
    reference passes them through the reference's weights (the beam is linear once they are fixed).  Target level and SIR, over
    the whole event and over the last block, equal the reference's to 0.01 dB, tracked and with one dir"""
    from sed_crnn_amd import feature
    pos, xs, xi, xn, s = ref.moving_scene(0.06)
    tau = ref.scene_tau(pos)
    import doa_ref as dr
    units = np.stack([dr.unit(ref.azimuth(b)) for b in range(ref.BLOCKS)] + [dr.unit(np.radians(ref.ONE_DIR_AZ))])
    doa = sed.DOA(pos, sed.DirectionGrid(units), max_frames=256, track=sed.DirectionTrack(1))
    assert np.abs(doa.steering(ref.SR) - tau).max() < 1e-12
    mix = xs + xi + xn
    s0, length = ref.LEAD * B, ref.BLOCKS * ref.BLOCK_FRAMES * B
    last = slice(length - ref.BLOCK_FRAMES * B, length)
    rows, tlen, tdir = [(ref.LEAD, ref.LEAD + 256, 100)], np.asarray([8], np.int32), np.arange(8, dtype=np.int32)[None, :]
    pcm, clips = _planar(mix)
    src = s[s0:s0 + length]
    for name, track, mv in (("one dir", [], sed.MVDR(1e-2)), ("tracked", list(range(8)), sed.MVDR(1e-2, follow_track=True))):
        y = feature.event_mvdr(pcm, clips, 4, _ev(rows, None, [8], [256], tlen, tdir), 1, doa, mv, sr=ref.SR, hop=ref.HOP)["audio"].cpu().numpy()
        assert y.shape == (length,)
        y_ref, (ys, yi, yn) = ref.event(mix, s0, length, tau, track, 8, 1, ref.HOP, 1e-2, through=(xs, xi, xn))
        mine_s, mine_i = y.astype(np.float64) - yi - yn, y.astype(np.float64) - ys - yn
        for what, sl in (("whole event", slice(0, length)), ("last block", last)):
            lv_ref, lv = mvdr_ref.db(ys[sl], src[sl]), mvdr_ref.db(mine_s[sl], src[sl])
            sir_ref, sir = mvdr_ref.db(ys[sl], yi[sl]), mvdr_ref.db(ys[sl], mine_i[sl])
            print(f"{name}, {what}: target out / in {lv:.3f} dB (reference {lv_ref:.3f}), SIR {sir:.3f} dB (reference {sir_ref:.3f}); "
                  f"max |kernel - reference| {np.abs(y - y_ref).max():.2e}")
            assert abs(lv - lv_ref) <= 0.01 and abs(sir - sir_ref) <= 0.01, (name, what)


# ───────────── 6. the detector and a live stream ─────────────
def _tracking(sed, det2, mf=96, **mv):
    plain, _ = det2
    doa = sed.DOA(doa_ref.line(2, 0.08), sed.DirectionGrid.ring(72), max_frames=mf, oversample=8, track=sed.DirectionTrack(1, 15))
    kw = dict(max_batch=1, median=3, mean=plain.mean, std=plain.std, localize=doa)
    return sed.EventDetector(plain.model, extract=sed.MVDR(0.1, follow_track=True, **mv), **kw), sed.EventDetector(plain.model, **kw), doa


def test_detector_entry_points_carry_the_tracked_audio(sed, det2):
    """det(wave), detect_many, from_features + det.localize and res[i] of a tracking, extracting detector: the audio is
    feature.event_mvdr's on the detector's own table, bit for bit"""
    from sed_crnn_amd import feature
    from sed_crnn_amd.resample import resample_many
    plain, x = det2
    det, before, doa = _tracking(sed, det2)
    a, b = det(x, sr=48000, channels=2), before(x, sr=48000, channels=2)
    assert len(b) > 0 and set(a.events) == set(b.events) | {"audio_start", "audio_len"} and "trk_dir" in b.events and b.audio is None
    for k in b.events:
        assert np.array_equal(_bits(a.events[k].float()), _bits(b.events[k].float())), k
    pcm, clips = resample_many([x], 48000, det.sr, 2, "cuda", keep_channels=True)
    want = feature.event_mvdr(pcm, clips, 2, b.events, det.model.time_factor, doa, det.extract_settings, sr=det.sr, hop=det.hop_length)
    assert want["audio"].numel() > 0 and np.array_equal(_bits(a.audio), _bits(want["audio"]))
    assert torch.equal(a.events["audio_start"], want["audio_start"]) and torch.equal(a.events["audio_len"], want["audio_len"])
    still = feature.event_mvdr(pcm, clips, 2, b.events, det.model.time_factor, doa, sed.MVDR(0.1), sr=det.sr, hop=det.hop_length)
    assert torch.equal(still["audio_len"], want["audio_len"])
    moved = bool((b.events["trk_len"] > 1).any()) and not torch.equal(still["audio"], want["audio"])
    print(f"{len(a)} events, blocks {b.events['trk_len'].tolist()}; the track changes the audio: {moved}")
    with pytest.raises(ValueError, match="track="):
        feature.event_mvdr(pcm, clips, 2, {k: v for k, v in b.events.items() if k != "trk_dir"}, det.model.time_factor, doa, det.extract_settings,
                           sr=det.sr, hop=det.hop_length)

    def same(r, one, what):
        assert set(r.events) == set(one.events), what
        for k in one.events:
            if k != "audio_start":
                assert np.array_equal(_bits(r.events[k].float()), _bits(one.events[k].float())), (what, k)
        for e in range(len(one)):
            assert np.array_equal(_bits(r.event_audio(e)), _bits(one.event_audio(e))), (what, e)

    waves = [x, _stereo(48000 * 2 + 5, 48000, 2), _stereo(30000, 48000, 3)]
    res = det.detect_many(waves, sr=[48000] * 3, channels=2)
    singles = [det(w, sr=48000, channels=2) for w in waves]
    assert res.audio.numel() == sum(s.audio.numel() for s in singles) and res.audio.data_ptr() == res[1].audio.data_ptr()
    for i, one in enumerate(singles):
        same(res[i], one, f"detect_many clip {i}")
    mel = feature.mbe(x, input_sr=48000, channels=2, keep_channels=True, device="cuda", mean=det.mean, std=det.std)
    later = det.localize(plain.from_features(mel), x, sr=48000, channels=2)
    same(later, a, "localize after from_features")
    same(det.with_decoder(median=3)(x, sr=48000, channels=2), a, "with_decoder")
    empty = det.detect_many([], channels=2)
    assert empty.audio.shape == (0,) and empty.events["audio_start"].shape == (0,) and empty.events["trk_dir"].shape == (0, 3)


@pytest.mark.parametrize("Kn", [0, 8])
def test_stream_carries_the_offline_tracked_audio(sed, det2, Kn):
    """two feeds, history "min", in fine and in coarse pieces: where the stream's rule accepts an emitted event its audio is
    det(w)'s bit for bit; a refused one has dir = -1, trk_len = 0 and no audio; the chunking changes no bit"""
    from sed_crnn_amd.localize import stream_extracts
    det, _, doa = _tracking(sed, det2, noise_blocks=Kn)
    recs = [_stereo(48000 * 8, 48000, 10), _stereo(48000 * 8 + 4001, 48000, 11)]
    offline = [det(w, sr=48000, channels=2) for w in recs]
    tf, mf, runs = det.model.time_factor, 96, []
    for sizes in (SIZES, COARSE):
        st = det.stream(2, history_frames="min", max_new_windows=1, input_sr=48000, emit_audio=True)
        outs = _feed(st, recs, sizes) + [st.flush()]
        lens = {}
        for o in outs:
            assert {"audio_start", "audio_len", "trk_len", "trk_dir"} <= set(o.events) and o.audio is not None
            for e in range(len(o)):
                lens[(int(o.events["stream"][e]), int(o.events["cls"][e]), int(o.events["onset"][e]))] = int(o.events["trk_len"][e])
        got = _audio_by_event(outs, 2)
        n_audio = n_moving = 0
        for s, (one, w) in enumerate(zip(offline, recs)):
            want = {k: v.cpu().numpy() for k, v in one.events.items()}
            n = sed.resample(w, 48000, channels=2, keep_channels=True).shape[1]
            assert sorted((c, a) for q, c, a in got if q == s) == sorted(zip(want["cls"].tolist(), want["onset"].tolist()))
            for e in range(len(one)):
                a, b, p = int(want["onset"][e]), int(want["offset"][e]), int(want["peak_frame"][e])
                key = (s, int(want["cls"][e]), a)
                d, bits = got[key]
                if stream_extracts(a, b, p, tf, 1 + n // det.hop_length, mf, st.lat, st.history_frames, det.hop_length, Kn, 1):
                    assert d == want["dir"][e] and lens[key] == want["trk_len"][e] and np.array_equal(bits, _bits(one.event_audio(e))), (s, e)
                    n_audio += int(bits.size > 0)
                    n_moving += int(want["trk_len"][e] > 1 and bits.size > 0)
                else:
                    assert bits.size == 0, (s, e)
        print(f"Kn={Kn}, pieces {sizes[:3]}..: {n_audio} events came with audio, {n_moving} of them on more than one block")
        assert n_audio >= 1 and n_moving >= 1
        runs.append(got)
    assert set(runs[0]) == set(runs[1])
    for k in runs[0]:
        assert runs[0][k][0] == runs[1][k][0] and np.array_equal(runs[0][k][1], runs[1][k][1]), k
