"""Batched detection without a GPU: the batch planner of sed_crnn_amd/detect.py against plan_windows, the refusals of
EventDetector.from_features_many / detect_many, and the argument checks of the batch entries (sed_logmel_batch,
sed_detect_stitch_batch, sed_detect_events_batch), which validate their host tables before touching the device."""
import ctypes as C

import numpy as np
import pytest


def _err():
    from sed_crnn_amd._lib import lib
    return lib().sed_last_error_string().decode()


FAKE = C.c_void_p(4096)          # a non-null device address: every call below is refused before anything is uploaded or launched


def test_batch_plan_reproduces_plan_windows_and_packs_every_window_once():
    import sed_crnn_amd as sed
    lengths = [8, 15, 63, 64, 65, 1000, 10_007, 200, 200, 9, 56, 127, 128, 129]
    for tf, K, hop, trim in ((8, 1, 32, 0), (8, 3, 16, 1), (4, 2, 64, 0), (2, 6, 8, 2)):
        bp = sed.plan_batch(lengths, tf, K, 64, hop, trim)
        assert bp.row_off == tuple(np.concatenate([[0], np.cumsum(lengths)]).tolist())
        want = [sed.plan_windows(N, tf, 64, hop, trim) for N in lengths]
        assert bp.plans == tuple(want)
        assert bp.out_off == tuple(np.concatenate([[0], np.cumsum([p.n_out for p in want])]).tolist())
        # every window of every recording exactly once, at its absolute row, with its own length
        expect = sorted((bp.row_off[r] + s, p.win_len) for r, p in enumerate(want) for s in p.starts)
        got = sorted([(s, 64) for s in bp.full_starts] + [(s, Lw) for Lw, ss in bp.groups for s in ss])
        assert got == expect
        assert len(bp.groups) <= 64 // tf - 1 and [g[0] for g in bp.groups] == sorted(g[0] for g in bp.groups)
        # the logits of the recordings tile the flat buffer without gaps or overlaps
        ext = sorted((o, o + p.n_win * p.win_out * K) for o, p in zip(bp.logit_off, want))
        assert ext[0][0] == 0 and ext[-1][1] == bp.n_logits
        assert all(a[1] == b[0] for a, b in zip(ext, ext[1:]))
        table = bp.stitch_table()
        assert table.shape == (len(lengths), 6) and table.dtype == np.int64
        assert (table[:, 2] * table[:, 1] * K == [p.n_win * p.win_out * K for p in want]).all()
    empty = sed.plan_batch([], 8, 1)
    assert empty.plans == () and empty.out_off == (0,) and empty.n_logits == 0


def test_batch_refusals_name_the_recording():
    import torch
    import sed_crnn_amd as sed
    with pytest.raises(ValueError, match="recording 2: a recording of 7 frames"):
        sed.plan_batch([100, 8, 7, 50], 8, 1)
    det = sed.EventDetector(sed.LightningTimePooledCRNN(dropout=0.0).eval())      # on the CPU: refused later, if at all
    with pytest.raises(ValueError, match="recording 1: a recording of 5 frames"):
        det.from_features_many([np.zeros((80, 40), np.float32), np.zeros((5, 40), np.float32)])
    with pytest.raises(ValueError, match=r"recording 1: expected features \[N, 40\]"):
        det.from_features_many([np.zeros((80, 40), np.float32), np.zeros((80, 41), np.float32)])
    with pytest.raises(ValueError, match="recording 0: expected a mono 1-D waveform"):
        det.detect_many([np.zeros((2, 5000), np.float32)])
    with pytest.raises(ValueError, match="recording 1: a recording of 1 frames"):
        det.detect_many([np.zeros(50_000, np.float32), np.zeros(100, np.float32)])
    with pytest.raises(sed.SedHipError, match="move the module to the GPU"):
        det.from_features_many([torch.zeros(80, 40)])                      # valid input, CPU model: refused before a launch


def test_logmel_batch_refuses_bad_clip_tables():
    from sed_crnn_amd._lib import lib
    L = lib()
    ws_bytes = L.sed_logmel_batch_workspace_bytes(3)
    assert ws_bytes == (4 * 3 + 1) * 8
    for bad in (0, -1, 1 << 27):
        assert L.sed_logmel_batch_workspace_bytes(bad) == 0
    blob = 16 * 2000                                                  # a plausible table size: the checks never read it

    def call(clips, pcm_len=10_000, rows=None, ws=ws_bytes, R=None):
        t = np.ascontiguousarray(np.asarray(clips, np.int64).reshape(-1, 2))
        R = t.shape[0] if R is None else R
        rows = int((1 + t[:, 1] // 1024).sum()) if rows is None else rows
        return L.sed_logmel_batch(FAKE, pcm_len, C.c_void_p(t.ctypes.data), R, FAKE, blob, None, None, FAKE, rows, 2048, 1024,
                                  40, 0, FAKE, ws, None)

    assert call([(0, 100), (9_000, 1_001), (200, 5)]) != 0 and "is not inside the PCM buffer" in _err()
    assert call([(0, 100), (200, 0), (300, 5)]) != 0 and "clip 1" in _err()
    assert call([(0, 100), (-4, 10), (300, 5)]) != 0 and "clip 1" in _err()
    assert call([(0, 100), (100, 10), (300, 5)], rows=7) != 0 and "rows" in _err()
    assert call([(0, 100), (100, 10), (300, 5)], ws=ws_bytes - 8) != 0 and "workspace" in _err()
    t = np.zeros((1, 2), np.int64)
    assert L.sed_logmel_batch(FAKE, 100, None, 1, FAKE, blob, None, None, FAKE, 1, 2048, 1024, 40, 0, FAKE, ws_bytes, None) != 0
    assert "null pointer" in _err()
    assert L.sed_logmel_batch(FAKE, 100, C.c_void_p(t.ctypes.data), 1, FAKE, blob, None, None, FAKE, 1, 2048, 1024, 40, 0, None,
                              ws_bytes, None) != 0 and "null pointer" in _err()


def _stitch_call(recs, K=2, trim=0, logits_len=None, n_total=None, ws=None, combine=0):
    from sed_crnn_amd._lib import lib
    L = lib()
    t = np.ascontiguousarray(np.asarray(recs, np.int64).reshape(-1, 6))
    R = t.shape[0]
    n_total = int(t[:, 5].sum()) if n_total is None else n_total
    logits_len = int(max(t[:, 0] + t[:, 1] * t[:, 2] * K)) if logits_len is None else logits_len
    need = L.sed_detect_batch_workspace_bytes(n_total, K, R, 0)
    ws = need if ws is None else ws
    return L.sed_detect_stitch_batch(FAKE, logits_len, C.c_void_p(t.ctypes.data), R, K, combine, trim, FAKE, n_total, FAKE, ws, None)


def test_stitch_batch_refuses_bad_recording_tables():
    K = 2
    a = [0, 3, 8, 4, 8, 16]                        # 3 windows of 8 every 4: 0, 4, 8 -> ends at 16
    b = [3 * 8 * K, 1, 5, 5, 0, 5]                 # one short window
    assert _stitch_call([a, [3 * 8 * K, 1, 5, 5, 0, 6]], K) != 0 and "must end at the recording's end" in _err()
    assert _stitch_call([[0, 3, 8, 4, 4, 12], b], K) != 0 and "is not the last start" in _err()    # a fourth window missing
    assert _stitch_call([a, [3 * 8 * K - 2, 1, 5, 5, 0, 5]], K) != 0 and "overlap" in _err()
    assert _stitch_call([[48, 1, 5, 5, 0, 5], [40, 3, 8, 4, 8, 16]], K) != 0 and "overlap" in _err()     # any order
    assert _stitch_call([a, b], K, logits_len=3 * 8 * K + 5 * K - 1) != 0 and "leave the buffer" in _err()
    assert _stitch_call([a, b], K, trim=3) != 0 and "uncovered" in _err()                        # hop 4 + 2*3 > 8
    assert _stitch_call([a, b], K, n_total=20) != 0 and "output frames" in _err()
    from sed_crnn_amd._lib import lib
    need = lib().sed_detect_batch_workspace_bytes(21, K, 2, 0)
    assert _stitch_call([a, b], K, ws=need - 1) != 0 and "workspace" in _err()
    assert _stitch_call([a, b], K, combine=2) != 0 and "combine" in _err()
    t = np.asarray([a], np.int64)
    assert lib().sed_detect_stitch_batch(None, 100, C.c_void_p(t.ctypes.data), 1, K, 0, 0, FAKE, 16, FAKE, need, None) != 0
    assert "null pointer" in _err()
    assert lib().sed_detect_stitch_batch(FAKE, 100, None, 1, K, 0, 0, FAKE, 16, FAKE, need, None) != 0 and "null" in _err()


def test_events_batch_refuses_bad_tables_and_small_workspaces():
    from sed_crnn_amd._lib import lib
    L = lib()
    n_out = np.asarray([100, 1, 64, 65], np.int64)
    K, cap = 3, 10
    need = L.sed_detect_batch_workspace_bytes(int(n_out.sum()), K, 4, cap)
    assert need > 0
    for args in ((0, 1, 1, 0), (5, 1, 6, 0), (100, 0, 1, 0), (100, 33, 1, 0), (100, 1, 1, -1), (2 ** 31 - 1, 2, 1, 0)):
        assert L.sed_detect_batch_workspace_bytes(*args) == 0, args

    def call(n, ws=need, max_events=cap, rec=FAKE, median=1, lo=0.5, hi=0.5):
        n = np.ascontiguousarray(np.asarray(n, np.int64))
        return L.sed_detect_events_batch(FAKE, C.c_void_p(n.ctypes.data), n.size, K, median, lo, hi, 0, 1, max_events, FAKE, ws,
                                         rec, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, None)

    assert call([100, 0, 64, 65]) != 0 and "recording 1 has 0 output frames" in _err()
    assert call([100, -5, 64, 65]) != 0 and "recording 1" in _err()
    assert call(n_out, ws=need - 1) != 0 and "workspace" in _err()
    assert call(n_out, rec=None) != 0 and "null output pointer" in _err()
    assert call(n_out, median=4) != 0 and "median" in _err()
    assert call(n_out, lo=0.6, hi=0.5) != 0 and "hi >= lo" in _err()
    assert call([2 ** 30, 2 ** 30]) != 0 and "2^31" in _err()
    assert L.sed_detect_events_batch(FAKE, None, 4, K, 1, 0.5, 0.5, 0, 1, cap, FAKE, need, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE,
                                     None) != 0 and "null pointer" in _err()
    assert L.sed_detect_events_batch(FAKE, C.c_void_p(n_out.ctypes.data), 4, K, 1, 0.5, 0.5, 0, 1, cap, FAKE, need, FAKE, FAKE,
                                     FAKE, FAKE, FAKE, FAKE, None, None) != 0 and "null pointer" in _err()
