"""Direction tracks without a GPU: the settings and their refusals, the neighbour table against a brute-force count,
the block rule at its edges, the C boundary (header, binding, exports, workspace sizes, host-side refusals of both entries, the
scratch guard of doatrack.hip), the result accessors on the host, and the float64 reference (tests/doa_track_ref.py) on a source
that moves.

The scene, measured when this test was written (degrees; tetrahedron of 6 cm, ring of 72 directions: covering radius 2.50; Q = 8;
8 blocks of 32 frames, the source at 20 + 10 b degrees, in block 4 a second source 120 degrees further round and 10 dB stronger):
    the single direction of the whole event     30: 10 from the source in block 0, 60 from the source in block 7
    raw track, error per block                   0  0  0  0  120  0  0  0
    smoothed track (max_step_deg = 15)           0  0  0  0    5  0  0  0     (float64 and the float32 restatement alike)"""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import doa_ref  # noqa: E402
import doa_track_ref as trk  # noqa: E402

SR = 44100


# ───────────── 1. settings ─────────────
def test_track_settings_are_validated():
    import sed_crnn_amd as sed
    t = sed.DirectionTrack()
    assert (t.block_chunks, t.max_step_deg) == (1, None) and sed.DirectionTrack(64, 180).max_step_deg == 180.0
    assert sed.DirectionTrack(np.int64(3), np.float32(7.5)) == sed.DirectionTrack(3, 7.5) and hash(t) == hash(sed.DirectionTrack(1))
    with pytest.raises(Exception):
        t.block_chunks = 2                                                          # frozen
    for bad in (0, 65, -1, 1.0, True, "2", None):
        with pytest.raises(ValueError, match="block_chunks"):
            sed.DirectionTrack(block_chunks=bad)
    for bad in (0, 0.0, -5, 180.5, float("nan"), float("inf"), True, "15"):
        with pytest.raises(ValueError, match="max_step_deg"):
            sed.DirectionTrack(max_step_deg=bad)
    assert [sed.DirectionTrack(w).max_blocks(mf) for w, mf in ((1, 256), (8, 256), (2, 96), (1, 40), (3, 1), (64, 100000))] == [8, 1, 2, 2, 1, 49]


def test_doa_takes_a_track_and_is_unchanged_without_one():
    import sed_crnn_amd as sed
    pos, grid = doa_ref.tetrahedron(0.06), sed.DirectionGrid.ring(36)
    plain = sed.DOA(pos, grid)
    assert plain.track is None and plain.neighbours() is None
    assert repr(plain) == "DOA(4 microphones, aperture 0.06 m, 36 directions, max_frames=256, oversample=8, c=343)"
    assert sorted(k for k in vars(plain) if k.startswith("_")) == ["_beam_device", "_delays", "_device", "_plans", "_steering", "_steering_device"]
    t = sed.DirectionTrack(2, 15)
    d = sed.DOA(pos, grid, max_frames=96, oversample=4, track=t)
    assert d.track is t and repr(d) == ("DOA(4 microphones, aperture 0.06 m, 36 directions, max_frames=96, oversample=4, c=343, "
                                        "track=DirectionTrack(block_chunks=2, max_step_deg=15.0))")
    assert d.plan(SR)[0] == plain.plan(SR)[0] and d.tdoa(SR) == sed.TDOA(8, 96)
    off, idx = d.neighbours()
    assert d.neighbours()[0] is off and d.neighbours()[1] is idx                    # cached
    want = sed.track_neighbours(grid, 15)
    assert np.array_equal(off, want[0]) and np.array_equal(idx, want[1])
    assert sed.DOA(pos, grid, track=sed.DirectionTrack(4)).neighbours() is None     # no smoothing: no table
    with pytest.raises(TypeError, match="DirectionTrack"):
        sed.DOA(pos, grid, track=15)
    sed.DOA(pos, grid, max_frames=256 * 32, track=sed.DirectionTrack(1))            # Tm = 256
    with pytest.raises(ValueError, match="257 blocks"):
        sed.DOA(pos, grid, max_frames=256 * 32 + 1, track=sed.DirectionTrack(1))
    sed.DOA(pos, grid, max_frames=256 * 32 + 1, track=sed.DirectionTrack(2))


# ───────────── 2. the neighbour table ─────────────
@pytest.mark.parametrize("gridname,step", [("ring36", 15), ("ring36", 10), ("ring36", 9.99), ("ring36", 180), ("sphere150", 15), ("sphere150", 40),
                                           ("sphere1", 5)])
def test_track_neighbours(gridname, step):
    import sed_crnn_amd as sed
    grid = sed.DirectionGrid.ring(36) if gridname == "ring36" else sed.DirectionGrid.sphere(int(gridname[6:]))
    D = len(grid)
    off, idx = sed.track_neighbours(grid, step)
    assert off.dtype == np.int32 and idx.dtype == np.int32 and off.shape == (D + 1,) and off[0] == 0 and off[-1] == idx.shape[0]
    want_off, want_idx = trk.neighbours(grid.unit_vectors, step)
    assert np.array_equal(off, want_off) and np.array_equal(idx, want_idx)
    near = np.zeros((D, D), bool)
    for d in range(D):
        row = idx[off[d]:off[d + 1]]
        assert d in row and (np.diff(row) > 0).all() and row.min() >= 0 and row.max() < D     # self-containing, ascending
        near[d, row] = True
    assert np.array_equal(near, near.T)                                             # symmetric
    ang = np.arccos(np.clip(grid.unit_vectors @ grid.unit_vectors.T, -1.0, 1.0))
    assert np.array_equal(np.diff(off), ((ang <= math.radians(step) + 1e-9) | np.eye(D, dtype=bool)).sum(1))
    if gridname == "ring36":                                                        # 10 degrees apart: the bound is inclusive
        assert (np.diff(off) == {15: 3, 10: 3, 9.99: 1, 180: 36}[step]).all()


def test_track_neighbours_refusals():
    import sed_crnn_amd as sed
    with pytest.raises(TypeError, match="DirectionGrid"):
        sed.track_neighbours(np.eye(3), 15)
    for bad in (0, -1, 181, float("nan"), None, True):
        with pytest.raises(ValueError, match="max_step_deg"):
            sed.track_neighbours(sed.DirectionGrid.ring(4), bad)


# ───────────── 3. the block rule ─────────────
@pytest.mark.parametrize("nf,W,sizes", [(0, 1, []), (1, 1, [1]), (31, 1, [31]), (32, 1, [32]), (33, 1, [33]), (47, 1, [47]), (48, 1, [32, 16]),
                                        (96, 2, [64, 32]), (95, 2, [95]), (256, 8, [256]), (256, 1, [32] * 8), (240, 1, [32] * 7 + [16]),
                                        (239, 1, [32] * 6 + [47]), (40, 1, [40]), (65, 2, [65]), (129, 2, [64, 65]), (2048 + 1023, 64, [3071]),
                                        (2048 + 1024, 64, [2048, 1024])])
def test_track_blocks_edge_cases(nf, W, sizes):
    import sed_crnn_amd as sed
    T, first, n = sed.track_blocks(nf, W)
    assert T == len(sizes) and n.tolist() == sizes and first.tolist() == [32 * W * b for b in range(T)]
    assert trk.blocks(nf, W) == list(zip(first.tolist(), n.tolist()))               # the reference states the same rule
    assert int(n.sum()) == nf and (T == 0 or (n[:-1] == 32 * W).all())
    if T > 1:
        assert n[-1] >= 16 * W                                                      # no short tail is left on its own


def test_track_blocks_over_a_range_and_refusals():
    import sed_crnn_amd as sed
    for W in (1, 2, 3, 8, 64):
        for nf in list(range(0, 300)) + [32 * W * 5 + k for k in (-1, 0, 1, 16 * W - 1, 16 * W)]:
            T, first, n = sed.track_blocks(nf, W)
            assert trk.blocks(nf, W) == list(zip(first.tolist(), n.tolist()))
            assert T <= trk.max_blocks(max(nf, 1), W) == sed.DirectionTrack(W).max_blocks(max(nf, 1))
    for bad in ((-1, 1), (10, 0), (10, 65)):
        with pytest.raises(ValueError, match="track_blocks"):
            sed.track_blocks(*bad)


# ───────────── 4. the boundary ─────────────
def test_track_entries_are_declared_bound_and_exported():
    import sed_crnn_amd as sed
    from sed_crnn_amd import _lib
    from sed_crnn_amd.events import _ENTRY
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "sedcrnn.h")).read()
    doc = open(os.path.join(root, "INTEGRATION.md")).read()
    L = C.CDLL(_lib.LIB_PATH)
    for name in ("sed_event_doa_track", "sed_event_doa_track_ring", "sed_event_doa_track_workspace_bytes", "sed_event_doa_track_ring_workspace_bytes"):
        assert name + "(" in header and name in _lib.SIGNATURES and hasattr(L, name), name
    assert "sed_event_doa_track.argtypes" in doc and "sed_event_doa_track_workspace_bytes.argtypes" in doc
    # the sibling's arguments, then 8 more behind srp_out
    for ring in ("", "_ring"):
        sib, got = _lib.SIGNATURES["sed_event_doa" + ring][1], _lib.SIGNATURES["sed_event_doa_track" + ring][1]
        assert got[:len(sib) - 3] == sib[:-3] and got[-3:] == sib[-3:] and len(got) == len(sib) + 8
        assert got[len(sib) - 3] is C.c_int and all(a is C.c_void_p for a in got[len(sib) - 2:-3])
    assert _ENTRY["doa_track", False] == "sed_event_doa_track" and _ENTRY["doa_track", True] == "sed_event_doa_track_ring"
    for name in ("DirectionTrack", "track_neighbours", "track_blocks"):
        assert hasattr(sed, name)


def test_track_workspace_sizes():
    from sed_crnn_amd import _lib
    L = _lib.lib()
    row = 1026 * 8
    for (R, ch, E, n, hop, mf), D, W in (((1, 2, 3, 5000, 1024, 256), 72, 1), ((2, 4, 10, 100 * 1024, 1024, 40), 200, 1),
                                         ((2, 4, 10, 100 * 1024 + 300, 1024, 96), 24, 2), ((1, 4, 1, 3600 * 48000, 1024, 256), 2562, 1),
                                         ((1, 3, 7, 100 * 1024, 1001, 256), 16384, 8), ((1, 2, 5, 100 * 1024, 1024, 256), 1, 64)):
        td = L.sed_event_tdoa_workspace_bytes(R, ch, E, n, hop, mf)
        cpe = -(-min(1 + n // hop, mf) // 32)
        assert td == ((R * ch + R) * 8 + 15) // 16 * 16 + E * cpe * (ch * (ch - 1) // 2) * row
        Tw = -(-cpe // W)
        assert L.sed_event_doa_track_workspace_bytes(R, ch, E, n, hop, mf, D, W, 0) == td            # no smoothing: nothing is kept
        assert L.sed_event_doa_track_workspace_bytes(R, ch, E, n, hop, mf, D, W, 1) == td + E * ((Tw * D * 6 + 15) // 16 * 16)
        cap = 65536
        tr = L.sed_event_tdoa_ring_workspace_bytes(R, ch, E, cap, hop, mf)
        cpe = -(-min(1 + cap // hop, mf) // 32)
        assert L.sed_event_doa_track_ring_workspace_bytes(R, ch, E, cap, hop, mf, D, W, 0) == tr > 0
        assert L.sed_event_doa_track_ring_workspace_bytes(R, ch, E, cap, hop, mf, D, W, 1) == tr + E * ((-(-cpe // W) * D * 6 + 15) // 16 * 16)
    ok = (1, 4, 2, 5000, 1024, 256, 72, 1, 1)
    assert L.sed_event_doa_track_workspace_bytes(*ok) > 0
    for i, bad in ((0, 0), (1, 1), (1, 9), (2, -1), (3, 0), (4, 0), (5, 0), (6, 0), (6, 16385), (7, 0), (7, 65)):
        args = list(ok)
        args[i] = bad
        assert L.sed_event_doa_track_workspace_bytes(*args) == 0, args
        if i != 3:
            args[3] = 8192
            assert L.sed_event_doa_track_ring_workspace_bytes(*args) == 0, args
    assert L.sed_event_doa_track_ring_workspace_bytes(1, 4, 2, 100, 1024, 256, 72, 1, 1) == 0        # a ring shorter than a frame
    assert L.sed_event_doa_track_workspace_bytes(1, 4, 2, 5000, 1024, 256 * 32 + 1, 72, 1, 1) == 0   # 257 blocks
    assert L.sed_event_doa_track_workspace_bytes(1, 4, 2, 5000, 1024, 256 * 32, 72, 1, 1) > 0


def test_track_entries_check_their_arguments_on_the_host():
    from sed_crnn_amd import _lib
    L = _lib.lib()
    FAKE, blob = C.c_void_p(0x1000), (8 + 2048 + 2048 + 1028) * 4

    def call(clips=((0, 5000), (8000, 5000)), channels=2, E=1, max_lag=24, max_frames=8, ws=1 << 20, J=FAKE, D=72, Q=8, trig=FAKE, dir_=FAKE,
             power=FAKE, pad=0, W=1, off=FAKE, idx=FAKE, tlen=FAKE, raw=FAKE, tdir=FAKE, tpow=FAKE, tmap=None, wsp=FAKE):
        t = np.asarray(clips, dtype=np.int64)
        return L.sed_event_doa_track(FAKE, 20000, C.c_void_p(t.ctypes.data), 1, channels, FAKE, blob, None, FAKE, FAKE, FAKE, E, 1, 1024, pad,
                                     max_lag, max_frames, FAKE, FAKE, FAKE, None, J, D, Q, trig, dir_, power, None, W, off, idx, tlen, raw,
                                     tdir, tpow, tmap, wsp, ws, None)

    def ring(channels=2, E=1, max_lag=24, max_frames=8, ws=1 << 20, J=FAKE, D=72, Q=8, trig=FAKE, dir_=FAKE, power=FAKE, cap=8192, hist=20,
             W=1, off=FAKE, idx=FAKE, tlen=FAKE, raw=FAKE, tdir=FAKE, tpow=FAKE, tmap=None, wsp=FAKE):
        n = np.asarray([9000], dtype=np.int64)
        return L.sed_event_doa_track_ring(FAKE, 1 << 20, cap, C.c_void_p(n.ctypes.data), 1, channels, FAKE, blob, None, FAKE, FAKE, FAKE, E, 1,
                                          1024, max_lag, max_frames, 10, hist, FAKE, FAKE, FAKE, None, J, D, Q, trig, dir_, power, None, W, off,
                                          idx, tlen, raw, tdir, tpow, tmap, wsp, ws, None)

    def err():
        return L.sed_last_error_string().decode()
    for fn, who in ((call, "event_doa_track:"), (ring, "event_doa_track_ring:")):
        for bad, what in ((dict(J=None), "null pointer"), (dict(trig=None), "null pointer"), (dict(dir_=None), "null pointer"),
                          (dict(power=None), "null pointer"), (dict(tlen=None), "null pointer"), (dict(raw=None), "null pointer"),
                          (dict(tdir=None), "null pointer"), (dict(tpow=None), "null pointer"), (dict(wsp=None), "null pointer"),
                          (dict(D=0), "1 to 16384 directions"), (dict(D=16385), "1 to 16384 directions"),
                          (dict(Q=3), "oversample must be 1, 2, 4, 8 or 16"), (dict(Q=0), "oversample"), (dict(Q=32), "oversample"),
                          (dict(max_lag=0), "max_lag"), (dict(max_lag=128), "max_lag"), (dict(trig=C.c_void_p(0x1004)), "8-byte aligned"),
                          (dict(W=0), "block_chunks must be in [1,64]"), (dict(W=65), "block_chunks"), (dict(off=None), "both nbr_off and nbr_idx"),
                          (dict(idx=None), "both nbr_off and nbr_idx"), (dict(max_frames=256 * 32 + 1), "257 blocks"),
                          (dict(max_frames=0), "max_frames"), (dict(channels=1), "channels"), (dict(channels=9), "channels")):
            assert fn(**bad) != 0 and what in err() and err().startswith(who), (who, bad, err())
        assert fn(E=0) == 0                                                         # no events: nothing is launched
        assert fn(E=0, off=None, idx=None) == 0 and fn(E=0, Q=16, D=16384, max_lag=127, W=64) == 0
    # the least workspace takes one event; one byte less is refused, with this entry's name, before anything is enqueued
    least = L.sed_event_doa_track_workspace_bytes(1, 2, 1, 5000, 1024, 8, 72, 1, 1)
    assert least == 32 + 1026 * 8 + 72 * 6 and call(ws=least - 16) != 0 and "event_doa_track: workspace" in err() and "one event" in err()
    assert call(ws=32 + 1026 * 8 - 16, off=None, idx=None) != 0 and "event_doa_track: workspace" in err()
    least = L.sed_event_doa_track_ring_workspace_bytes(1, 2, 1, 8192, 1024, 8, 72, 1, 1)
    assert least == 16 + 1026 * 8 + 72 * 6 and ring(ws=least - 16) != 0 and "event_doa_track_ring: workspace" in err()
    # what the siblings check, with these entries' names
    assert call(pad=2) != 0 and "event_doa_track: pad_mode" in err()
    assert call(clips=((0, 5000), (18000, 5000))) != 0 and "event_doa_track: recording 0, channel 1" in err()
    assert ring(cap=100) != 0 and "event_doa_track_ring: a ring holds" in err()
    assert ring(hist=0) != 0 and "history_frames" in err()


def test_build_guards_both_track_kernels_against_scratch():
    from sed_crnn_amd.build import EXTRA_FLAGS, NO_SCRATCH_KERNELS, SOURCES
    assert "doatrack.hip" in SOURCES and set(NO_SCRATCH_KERNELS["doatrack.hip"]) == {"doa_track_steer_k", "doa_track_path_k"}
    assert EXTRA_FLAGS["doatrack.hip"] == EXTRA_FLAGS["doa.hip"]
    assert set(NO_SCRATCH_KERNELS["doa.hip"]) == {"doa_steer_k"}                    # the sibling's guard is its own still


# ───────────── 5. the accessors, on the host ─────────────
def _net(cin):
    import sed_crnn_amd as sed
    return sed.LightningTimePooledCRNN(dropout=0.0, in_channels=cin, n_mels=40).eval()


def test_detector_carries_the_track_settings():
    import sed_crnn_amd as sed
    grid = sed.DirectionGrid.ring(8)
    t = sed.DirectionTrack(2, 50)
    doa = sed.DOA(doa_ref.tetrahedron(0.06), grid, max_frames=96, track=t)
    det = sed.EventDetector(_net(4), localize=doa)
    assert det.localize_settings is doa and det.locates_directions and det._track_info() == (t, 96, det.model.time_factor, det.hop_length)
    assert det.with_decoder(threshold=0.3)._track_info() == det._track_info()
    assert sed.EventDetector(_net(4), localize=sed.DOA(doa_ref.tetrahedron(0.06), grid))._track_info() is None
    assert sed.EventDetector(_net(4), localize=sed.TDOA(8, 16))._track_info() is None and sed.EventDetector(_net(4))._track_info() is None


def test_result_doa_track_maps_blocks_to_times_and_angles_on_the_host():
    import torch
    import sed_crnn_amd as sed
    grid = sed.DirectionGrid.ring(4, elevation=0.25)
    i32 = dict(dtype=torch.int32)
    ev = {"cls": torch.tensor([0, 1, 0], **i32), "onset": torch.tensor([2, 0, 5], **i32), "offset": torch.tensor([12, 200, 6], **i32),
          "peak_frame": torch.tensor([3, 100, 5], **i32), "loc_frames": torch.tensor([80, 96, 0], **i32), "dir": torch.tensor([1, 2, -1], **i32),
          "doa_power": torch.tensor([0.5, 0.25, 0.0]), "trk_len": torch.tensor([3, 3, 0], **i32),
          "trk_raw": torch.tensor([[1, 3, 0], [2, -1, 0], [-1, -1, -1]], **i32), "trk_dir": torch.tensor([[1, 2, 0], [2, -1, 3], [-1, -1, -1]], **i32),
          "trk_power": torch.tensor([[0.5, 0.25, 0.125], [0.125, 0.0, 0.75], [0.0, 0.0, 0.0]])}
    info = (sed.DirectionTrack(1, 30), 96, 8, 1024)
    res = sed.DetectionResult(None, ev, 0.1, None, sr=SR, grid=grid, track=info)
    a = res.doa_track(0)                                                            # frames [16, 96): blocks of 32, 32 and 16
    assert a.shape == (3, 4)
    np.testing.assert_allclose(a[:, 0], [(16 + 15.5) * 1024 / SR, (48 + 15.5) * 1024 / SR, (80 + 7.5) * 1024 / SR], rtol=0, atol=1e-12)
    np.testing.assert_allclose(a[:, 1:], [[np.pi / 2, 0.25, 0.5], [np.pi, 0.25, 0.25], [0.0, 0.25, 0.125]], rtol=0, atol=1e-12)
    b = res.doa_track(1)                                                            # 1600 frames: the 96 around the peak, from 100*8 + 4 - 48
    assert b.shape == (3, 4) and np.isnan(b[1, 1:3]).all() and b[1, 3] == 0.0
    np.testing.assert_allclose(b[:, 0], [(756 + 32 * k + 15.5) * 1024 / SR for k in range(3)], rtol=0, atol=1e-12)
    np.testing.assert_allclose(b[[0, 2], 1:], [[np.pi, 0.25, 0.125], [-np.pi / 2, 0.25, 0.75]], rtol=0, atol=1e-12)
    assert res.doa_track(2).shape == (0, 4) and np.array_equal(res.doa_track(-3), a)
    with pytest.raises(IndexError):
        res.doa_track(3)
    st = sed.StreamEvents(ev, [0, 1, 3], [0, 0], 0.1, sr=SR, grid=grid, track=info)
    assert np.array_equal(st.doa_track(0), a) and np.array_equal(st.doa_track(1), b, equal_nan=True)
    batch = sed.BatchDetectionResult(None, {**ev, "rec": torch.tensor([0, 0, 1], **i32)}, 0.1, (None, None), [0, 0, 0], [0, 2, 3], sr=SR, grid=grid,
                                     track=info)
    assert np.array_equal(batch.doa_track(1), b, equal_nan=True)
    for plain in (sed.DetectionResult(None, {k: v for k, v in ev.items() if not k.startswith("trk_")}, 0.1, None, sr=SR, grid=grid),
                  sed.DetectionResult(None, ev, 0.1, None, sr=SR, grid=grid),
                  sed.StreamEvents({"cls": None, "dir": None}, [0, 0], [0], 0.1, sr=SR, grid=grid)):
        with pytest.raises(ValueError, match="track="):
            plain.doa_track(0)


# ───────────── 6. the reference on a source that moves ─────────────
def test_path_restatements_agree_and_follow_the_rules():
    rng = np.random.default_rng(3)
    import sed_crnn_amd as sed
    grid = sed.DirectionGrid.ring(24)
    off, idx = sed.track_neighbours(grid, 15)                                       # d - 1, d, d + 1
    maps = rng.standard_normal((6, 24)).astype(np.float32)
    p32, p64 = trk.path_f32(maps, off, idx), trk.path_f64(maps.astype(np.float64), off, idx)
    assert np.array_equal(p32, p64)
    step = np.abs(np.diff(p32))
    assert (np.minimum(step, 24 - step) <= 1).all()                                 # one grid step a block at most
    # brute force over every path of a small problem: the recurrence finds the best one
    small = rng.standard_normal((4, 6))
    o6, i6 = trk.neighbours(sed.DirectionGrid.ring(6).unit_vectors, 60)
    best, arg = -np.inf, None
    for code in range(6 ** 4):
        p = [(code // 6 ** k) % 6 for k in range(4)]
        if all(p[k] in i6[o6[p[k + 1]]:o6[p[k + 1] + 1]] for k in range(3)):
            v = sum(small[k, p[k]] for k in range(4))
            if v > best:
                best, arg = v, p
    assert trk.path_f64(small, o6, i6).tolist() == arg
    # with every direction a neighbour of every other the path is the raw track; ties go to the first maximum
    full = trk.neighbours(grid.unit_vectors, 180)
    assert np.array_equal(trk.path_f32(maps, *full), maps.argmax(1))
    flat = np.zeros((3, 24), np.float32)
    assert trk.path_f32(flat, off, idx).tolist() == [0, 0, 0]
    flat[1, 5] = 1.0
    assert trk.path_f32(flat, off, idx).tolist() == [4, 5, 4]                       # the first of the neighbours, in ascending j
    assert trk.track_dir(maps, [3, -1, 4, 5, -1, 0], off, idx).tolist() == [p32[0], -1, p32[2], p32[3], -1, p32[5]]
    assert trk.track_dir(maps, [3, -1, 4, 5, -1, 0]).tolist() == [3, -1, 4, 5, -1, 0]
    assert trk.path_f32(maps[:1], off, idx).tolist() == [int(maps[0].argmax())]


def test_reference_follows_a_moving_source_past_a_louder_one():
    import sed_crnn_amd as sed
    pos, grid, Q = doa_ref.tetrahedron(0.06), sed.DirectionGrid.ring(72), 8
    doa = sed.DOA(pos, grid, oversample=Q, track=sed.DirectionTrack(1, 15))
    ml, J, _ = doa.plan(SR)
    J = J.astype(np.int64)
    Pk = doa_ref.whitened(trk.scene(pos, SR))
    truth = [doa_ref.unit(a) for a in trk.scene_truth()]
    u = grid.unit_vectors
    near = doa_ref.covering_radius(u, in_plane=True) + math.radians(5.0)
    single = doa_ref.event_doa(Pk, [(0, 256, 128)], 1, J, ml, Q)
    assert single["loc_frames"][0] == 256
    e0, e7 = (math.degrees(doa_ref.angle_between(u[single["dir"][0]], truth[b])) for b in (0, 7))
    print(f"single direction {single['dir'][0]}: {e0:.2f} deg from the source in block 0, {e7:.2f} deg in block 7")
    assert max(e0, e7) > 15.0
    maps, raw, power = trk.block_maps(Pk, 0, 256, 1, J, ml, Q)
    assert maps.shape == (8, 72) and (raw >= 0).all() and (power > 0).all()
    err = [doa_ref.angle_between(u[d], t) for d, t in zip(raw, truth)]
    print("raw track, degrees off:", np.round(np.degrees(err), 2).tolist())
    assert all(e <= near for b, e in enumerate(err) if b != 4) and err[4] > math.radians(60.0)
    for f32 in (False, True):
        path = trk.track_dir(maps.astype(np.float32) if f32 else maps, raw, *doa.neighbours(), f32=f32)
        err = [doa_ref.angle_between(u[d], t) for d, t in zip(path, truth)]
        print("smoothed track, degrees off:", np.round(np.degrees(err), 2).tolist())
        assert all(e <= near for e in err)
