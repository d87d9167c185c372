"""Batched detection on the MI355X (EventDetector.detect_many / from_features_many, feature.mbe_many, the sed_*_batch entries of
csrc/logmel.hip and csrc/detect.hip) against the single-recording path, the numpy restatement of tests/detect_ref.py and the
CPU oracle nets."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import detect_ref as ref  # noqa: E402
from test_gpu_detect import _assert_events_equal, _centre_on_threshold, _features, _nets, _oracle_probs  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def sed():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    import sed_crnn_amd as s
    return s


def _bits(t):
    return t.cpu().numpy().view(np.int32)


# ───────────── 1. log-mel ─────────────
def test_mbe_many_equals_per_clip_mbe_bitwise(sed):
    from sed_crnn_amd import data, feature
    rng = np.random.default_rng(1)
    lengths = [1, 100, 1023, 1024, 1025, 2047, 2048, 3 * 44_100 + 17, 5000]
    waves = [torch.from_numpy((0.3 * rng.standard_normal(n)).astype(np.float32)).cuda() for n in lengths]
    mean, std = data.standard_scaler_fit(feature.mbe(waves[-2]))
    for pad_mode in ("constant", "reflect"):
        for scaler in (False, True):
            kw = dict(pad_mode=pad_mode, mean=mean if scaler else None, std=std if scaler else None)
            got, rows = feature.mbe_many(waves, **kw)
            want = [feature.mbe(w, **kw) for w in waves]
            assert rows == list(np.concatenate([[0], np.cumsum([len(w) for w in want])]))
            assert np.array_equal(_bits(got), _bits(torch.cat(want))), (pad_mode, scaler)
    # host clips, one launch for all
    got, _ = feature.mbe_many([w.cpu().numpy() for w in waves[:4]])
    assert np.array_equal(_bits(got), _bits(torch.cat([feature.mbe(w) for w in waves[:4]])))


def test_mbe_packed_at_odd_offsets_and_custom_tables(sed):
    """caller-packed clips at odd sample offsets take the guarded loads: the same values; a custom blob (list plan)"""
    from sed_crnn_amd import feature
    rng = np.random.default_rng(2)
    buf = torch.from_numpy((0.2 * rng.standard_normal(400_000)).astype(np.float32)).cuda()
    clips = [(3, 1025), (1031, 70_001), (71_033, 1), (71_035, 2048), (73_085, 100_000), (200_001, 4095)]
    win = feature.hann_periodic() ** 2
    fb = feature.slaney_mel_basis(n_mels=64)
    fb[:, ::3] *= 0.5                                                 # still a two-band bank; and one that is not:
    dense = np.abs(rng.standard_normal((24, 1025))).astype(np.float32) * (rng.random((24, 1025)) < 0.2)
    for tables in (None, feature.build_tables(win, fb, "cuda"), feature.build_tables(win, dense, "cuda")):
        for pad_mode in ("constant", "reflect"):
            got, rows = feature.mbe_packed(buf, clips, pad_mode=pad_mode, tables=tables)
            want = torch.cat([feature.mbe(buf[o:o + n].clone(), pad_mode=pad_mode, tables=tables) for o, n in clips])
            assert np.array_equal(_bits(got), _bits(want)), pad_mode
            assert rows[-1] == want.shape[0]


# ───────────── 2. stitch ─────────────
def _stitch_single(logits, plan, combine, trim):
    from sed_crnn_amd._lib import check, lib, ptr, stream_ptr
    out = torch.empty(plan.n_out, logits.shape[2], device="cuda")
    check(lib().sed_detect_stitch(ptr(logits), plan.n_win, plan.win_out, logits.shape[2], plan.hop_out, plan.last_start_out,
                                  plan.n_out, combine, trim, ptr(out), stream_ptr()), "sed_detect_stitch")
    return out


def test_stitch_batch_equals_single_stitch_bitwise(sed):
    rng = np.random.default_rng(11)
    tf, L = 8, 64
    lengths = [64, 8, 1003, 65, 15, 4000, 63, 64, 200, 129]
    for K in (1, 4):
        m = sed.LightningTimePooledCRNN(dropout=0.0, n_classes=K).cuda().eval()
        for trim in (0, 1, 2):
            for combine in ("mean", "max"):
                bp = sed.plan_batch(lengths, tf, K, L, 32, trim)
                det = sed.EventDetector(m, hop=32, trim=trim, combine=combine)
                logits = torch.from_numpy((rng.standard_normal(bp.n_logits) * 3).astype(np.float32)).cuda()
                probs = det.stitch_many(logits, bp)
                for r, p in enumerate(bp.plans):
                    o = bp.logit_off[r]
                    lg = logits[o:o + p.n_win * p.win_out * K].view(p.n_win, p.win_out, K)
                    one = _stitch_single(lg, p, {"mean": 0, "max": 1}[combine], trim)
                    seg = probs[bp.out_off[r]:bp.out_off[r + 1]]
                    assert np.array_equal(_bits(seg), _bits(one)), (K, trim, combine, r)
                    want = ref.stitch(lg.cpu().numpy(), [s // tf for s in p.starts], p.n_out, combine, trim)
                    assert np.abs(seg.cpu().numpy() - want).max() < 1e-6


# ───────────── 3. decode ─────────────
def _decode_batch(sed, tracks, max_events=None, **kw):
    """tracks: list of [n_r, K] float32 -> (true total, events dict, event offsets)"""
    K = tracks[0].shape[1]
    m = sed.LightningTimePooledCRNN(dropout=0.0, n_classes=K).cuda().eval()
    det = sed.EventDetector(m, threshold=kw.pop("hi", 0.5), low=kw.pop("lo", None), **kw)
    bp = sed.plan_batch([8 * len(t) for t in tracks], 8, K)
    probs = torch.from_numpy(np.ascontiguousarray(np.concatenate(tracks), np.float32)).cuda()
    if max_events is not None:
        det.max_events = max_events
        from sed_crnn_amd._lib import check, lib, ptr, stream_ptr
        import ctypes as C
        n_out = np.asarray([len(t) for t in tracks], np.int64)
        ws = det._batch_workspace(probs.shape[0], K, len(tracks))
        keys = ("rec", "cls", "onset", "offset", "peak", "peak_frame")
        out = {k: torch.full((max(max_events, 1),), -7, dtype=torch.float32 if k == "peak" else torch.int32, device="cuda")
               for k in keys}
        off = torch.zeros(len(tracks) + 1, dtype=torch.int32, device="cuda")
        check(lib().sed_detect_events_batch(ptr(probs), C.c_void_p(n_out.ctypes.data), len(tracks), K, det.median, det.lo, det.hi,
                                            det.min_gap, det.min_len, max_events, ptr(ws), ws.numel(), *(ptr(out[k]) for k in keys),
                                            ptr(off), stream_ptr()), "sed_detect_events_batch")
        offs = off.cpu().tolist()
        return offs[-1], {k: v[:min(offs[-1], max_events)].cpu().numpy() for k, v in out.items()}, offs
    ev, offs = det.decode_many(probs, bp)
    return offs[-1], {k: v.cpu().numpy() for k, v in ev.items()}, offs


def _check_batch_decode(sed, tracks, what="", **kw):
    total, got, offs = _decode_batch(sed, tracks, **dict(kw))
    want_n = 0
    for r, t in enumerate(tracks):
        want = ref.decode(t, **{k: v for k, v in kw.items()})
        e0, e1 = offs[r], offs[r + 1]
        assert e1 - e0 == len(want["cls"]), (what, r)
        _assert_events_equal({k: got[k][e0:e1] for k in want}, want, f"{what} rec {r}")
        assert (got["rec"][e0:e1] == r).all()
        want_n += e1 - e0
    assert total == want_n
    return total


def test_decode_batch_matches_reference_per_recording(sed):
    rng = np.random.default_rng(5)
    lengths = [1, 5, 63, 64, 65, 128, 4097, 3, 900, 31, 30, 2]
    for K in (1, 3):
        tracks = [(1 / (1 + np.exp(-np.sin(np.cumsum(rng.standard_normal((n, K)) * 0.4, 0)) * 3))).astype(np.float32)
                  for n in lengths]
        for kw in (dict(), dict(lo=0.3, hi=0.8), dict(median=5, min_gap=2, min_len=3)):
            _check_batch_decode(sed, tracks, f"K={K} {kw}", **kw)
        for m in (1, 3, 15, 31):                                      # widths beyond the short recordings' lengths
            _check_batch_decode(sed, tracks, f"median {m}", median=m, lo=0.4, hi=0.6)


def test_decode_batch_keeps_recordings_apart(sed):
    """a recording ending 'on' followed by one starting 'on': two events, and min_gap does not merge them"""
    a = np.full((70, 1), 0.1, np.float32)
    a[60:] = 0.9
    b = np.full((40, 1), 0.9, np.float32)
    b[5:] = 0.1
    c = np.full((64, 1), 0.9, np.float32)
    for kw in (dict(), dict(min_gap=50), dict(median=9, min_gap=20)):
        total = _check_batch_decode(sed, [a, b, c, a], f"apart {kw}", **kw)
        assert total == 4 or kw.get("median")


def test_decode_batch_max_events_below_the_total(sed):
    rng = np.random.default_rng(3)
    tracks = [rng.random((n, 2)).astype(np.float32) for n in (300, 1, 77, 1000)]
    total, full, _ = _decode_batch(sed, tracks, median=3)
    assert total > 50
    for cap in (0, 1, 17, total - 1):
        t, got, offs = _decode_batch(sed, tracks, max_events=cap, median=3)
        assert t == total and offs[-1] == total
        for k in got:
            np.testing.assert_array_equal(got[k], full[k][:cap], err_msg=f"cap {cap} {k}")
    m = sed.LightningTimePooledCRNN(dropout=0.0, n_classes=2).cuda().eval()
    det = sed.EventDetector(m, median=3)
    det.max_events = 4                                                # the detector grows its buffers and reruns the decode
    ev, offs = det.decode_many(torch.from_numpy(np.concatenate(tracks)).cuda(), sed.plan_batch([8 * len(t) for t in tracks], 8, 2))
    assert det.max_events == total and offs[-1] == total
    for k in full:
        np.testing.assert_array_equal(ev[k].cpu().numpy(), full[k], err_msg=k)


def test_decode_batch_scan_over_3000_recordings(sed):
    rng = np.random.default_rng(9)
    tracks = [rng.random((int(n), 4)).astype(np.float32) for n in rng.integers(1, 40, 3_100)]
    total = _check_batch_decode(sed, tracks, "3100 x 4", lo=0.6, hi=0.7)
    assert total > 3_000


# ───────────── 4-7. the whole path ─────────────
LENGTHS = [8, 15, 63, 64, 65, 1000, 10_007, 200, 200, 3_001, 129, 500]


@pytest.mark.parametrize("which", ["lightning", "timepooled", "stereo"])
def test_batch_end_to_end_matches_single_path_and_oracle(sed, which):
    r, m = _nets(sed, which, seed=21)
    F = 40 * m.in_channels
    mels = [_features(N, seed=30 + i, F=F) for i, N in enumerate(LENGTHS)]
    _centre_on_threshold(r, m, mels[6])
    det = sed.EventDetector(m)
    res = det.from_features_many([torch.from_numpy(x).cuda() for x in mels])
    assert len(res) == len(LENGTHS) and res.out_offsets[-1] == res.probs.shape[0]
    assert int(res.events["rec"].numel()) == res.event_offsets[-1]
    worst = 0.0
    for i, x in enumerate(mels):
        one = det.from_features(torch.from_numpy(x).cuda())
        got = res[i]
        assert got.plan == one.plan
        d = (got.probs - one.probs).abs().max().item()
        assert d <= 2e-6, (i, d)
        p = one.probs.cpu().numpy()
        sure = (np.abs(p - det.lo) > 1e-5) & (np.abs(p - det.hi) > 1e-5)      # lo == hi, no filter: the mask is p > 0.5
        K = p.shape[1]
        mg = ref.event_mask({k: v.cpu().numpy() for k, v in got.events.items()}, got.plan.n_out, K)
        mo = ref.event_mask({k: v.cpu().numpy() for k, v in one.events.items()}, one.plan.n_out, K)
        assert np.array_equal(mg[sure], mo[sure]), i
        want = _oracle_probs(r, x, got.plan)
        worst = max(worst, np.abs(got.probs.cpu().double().numpy() - want).max())
        assert len(got.intervals(0)) == int((got.events["cls"] == 0).sum())
    print(f"{which}: max |dp| vs oracle {worst:.2e}, {res.n_events} events")
    assert worst < 1e-4


def test_detect_many_equals_features_path_bitwise(sed):
    from sed_crnn_amd import data, feature
    _, m = _nets(sed, "lightning", seed=4)
    rng = np.random.default_rng(9)
    lengths = [44_100 * 30, 8 * 1024, 100_000, 44_100 * 3 + 17, 7 * 1024 + 5]
    waves = [torch.from_numpy((0.1 * rng.standard_normal(n)).astype(np.float32)).cuda() for n in lengths]
    mean, std = data.standard_scaler_fit(feature.mbe(waves[0]))
    det = sed.EventDetector(m, mean=mean, std=std, median=3)
    a = det.detect_many(waves)
    b = det.from_features_many([feature.mbe(w, mean=mean, std=std) for w in waves])
    assert torch.equal(a.probs, b.probs)
    for k in a.events:
        assert torch.equal(a.events[k], b.events[k]), k
    c = sed.detect_events_many(m, [w.cpu().numpy() for w in waves], mean=mean, std=std, median=3)
    assert torch.equal(c.probs, a.probs) and c.event_offsets == a.event_offsets


def test_batch_chunking_and_repeatability(sed):
    _, m = _nets(sed, "lightning", seed=5)
    mels = [torch.from_numpy(_features(N, seed=N)).cuda() for N in (3_001, 40, 700, 56, 64, 2_000)]
    a = sed.EventDetector(m, max_batch=7, min_gap=1).from_features_many(mels)
    b = sed.EventDetector(m, max_batch=1024, min_gap=1).from_features_many(mels)
    c = sed.EventDetector(m, max_batch=1024, min_gap=1).from_features_many(mels)
    assert (a.probs - b.probs).abs().max().item() <= 2e-6
    assert torch.equal(b.probs, c.probs)
    for k in b.events:
        assert torch.equal(b.events[k], c.events[k]), k


def test_empty_batch_launches_nothing(sed):
    _, m = _nets(sed, "lightning", seed=6)
    det = sed.EventDetector(m)
    torch.cuda.synchronize()
    res = det.from_features_many([])
    assert len(res) == 0 and res.probs.shape == (0, 1) and res.event_offsets == [0] and res.n_events == 0
    assert det._bws is None and det._zlab is None                      # no workspace, no window buffer: nothing ran
    res = sed.detect_events_many(m, [])
    assert len(res) == 0 and list(res) == []
