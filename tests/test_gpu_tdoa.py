"""Per-event TDOA on the MI355X: feature.event_tdoa against the float64 definition (tests/tdoa_ref.py), integer delays
coming back, the batch / a permuted table / the guarded load path / workspace slices bit for bit, silence and junk events, and
the localising detector end to end.

Measured on an MI355X over the cases of test_event_tdoa_matches_the_float64_definition and the C = 8 test (acc / loc_frames
against float64): kernel error 1.5e-8 .. 1.4e-7 with constant padding, up to 7.6e-6 with reflect padding on the 2047-sample clip
(one-frame event on an end frame; yardstick 2.3e-5 there); worst kernel / yardstick ratio 5.59 of the 8 allowed (C = 2, hop 441,
reflect, 5000 samples, max_lag 1: kernel 2.7e-7, yardstick 4.8e-8), with constant padding 4.16 (C = 3, hop 1024, 2047 samples,
max_lag 1, yardstick 1.4e-8); the yardstick was degenerate (below 1e-9, replaced by 2^-24) only on one-sample clips at C = 2
and 3.  lag and strength against the float64 formula on the kernel's own curve: at most 0.50 x eps32 max(1, |lag|) —
the kernel evaluates the formula in double and rounds once — so LAG_BOUND is twice that, 1.0.  C = 8: ratios 0.48 .. 1.03.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import spatial_ref  # noqa: E402
import tdoa_ref  # noqa: E402
from test_gpu_detect import _assert_events_equal  # noqa: E402
from test_gpu_multichannel import _stereo, det2  # noqa: E402,F401
from test_gpu_spatial import _stereo16, det3  # noqa: E402,F401

pytestmark = pytest.mark.gpu
DELAYS = (0, 7, -3, 12, 5, -9, 2, 15)               # test_gpu_spatial's: every pair of the first 4 within 24 samples, of all 8 too
NEAR = (0, 1, 0, 1, 1, 0, 1, 0)                     # for max_lag = 1: every pair's delay is -1, 0 or 1
LENGTHS = (1, 2047, 5000, 9000, 40000)
CHUNK = 32                                          # tdoa.hip: TD_CHUNK
DEGENERATE = 1e-9                                   # test_gpu_spatial's: a float32 yardstick below this is exact arithmetic
EPS32 = 2.0 ** -23
LAG_BOUND = 1.0                                     # x EPS32 max(1, |lag|): twice the measured 0.5 (the one rounding to float32)


@pytest.fixture(scope="module")
def sed():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    import sed_crnn_amd as s
    return s


def _bits(t):
    return t.cpu().numpy().view(np.int32)


def _planar(x, lead=0):
    """[n, C] -> (one device buffer with the C planar channels, each starting 16-byte aligned plus ``lead`` samples, clips)"""
    pieces, clips, at = [], [], 0
    for c in range(x.shape[1]):
        pad = (-at) % 4 + lead
        pieces.append(np.zeros(pad, np.float32))
        at += pad
        clips.append((at, x.shape[0]))
        pieces.append(np.ascontiguousarray(x[:, c], dtype=np.float32))
        at += x.shape[0]
    return torch.from_numpy(np.concatenate(pieces)).cuda(), clips


def _events(rows, rec=None):
    """[(onset, offset, peak_frame), ...] -> the dict of int32 device tensors the decoders return"""
    a = np.asarray(rows, dtype=np.int32).reshape(-1, 3)
    ev = {k: torch.from_numpy(np.ascontiguousarray(a[:, i])).cuda() for i, k in enumerate(("onset", "offset", "peak_frame"))}
    ev["cls"] = torch.zeros(len(a), dtype=torch.int32, device="cuda")
    ev["peak"] = torch.ones(len(a), device="cuda")
    if rec is not None:
        ev["rec"] = torch.from_numpy(np.asarray(rec, dtype=np.int32)).cuda()
    return ev


def _tables(n_feat, pad_mode="constant", impulse=False):
    """(time_factor, max_frames, events, indices of the events whose arg-max may be a tie) x 2 for a recording of n_feat feature
    frames.  With reflect padding frame 0, centred on sample 0, is exactly symmetric about its centre: cc[+d] = cc[-d], a tie by
    construction — and the last frame holds up to half a frame of mirrored samples (a second peak of 0.55 of the first was seen).
    With reflect padding the one-frame events whose arg-max is compared therefore sit one frame further in, and one-frame events
    on frame 0 and on the last frame are run as well, flagged: everything is checked on them, and the arg-max wherever the
    reference itself is no near-tie.  ``impulse``: a clip of one sample, whose frames are impulses — cc = sign(x_i x_j) at lag 0
    and rounding noise elsewhere, so with a negative sign the maximum is left to that noise: every event is flagged."""
    last = n_feat - 1
    first = 1 if pad_mode == "reflect" and n_feat > 1 else 0
    one = last - 1 if pad_mode == "reflect" and n_feat > 2 else last
    a = [(first, first + 1, first), (one, one + 1, one),             # one-frame events: the first and the last frame
         (0, n_feat, n_feat // 2),                                    # the whole clip
         (0, n_feat + 7, 1),                                          # an offset beyond the last frame
         (last // 2, n_feat, last), (last // 2, n_feat, last)]        # two identical events
    if n_feat > CHUNK:
        a += [(n_feat - CHUNK - 1, n_feat, 0), (1, CHUNK + 1, 3)]     # chunk length + 1 frames (two chunks), exactly one chunk
    ties = set()
    if pad_mode == "reflect" and n_feat > 1:
        ties = {len(a), len(a) + 1}
        a += [(0, 1, 0), (last, last + 1, last)]                      # the mirror-symmetric end frames on their own
    tf = 2
    n_out = max(1, n_feat // tf)
    b = [(0, n_out, 0), (0, n_out, n_out - 1), (0, n_out, n_out // 2),   # longer than max_frames = 8 where the clip is: peak at either end
         (0, n_out + 3, n_out - 1),                                       # ... and the ragged tail beyond the last output frame
         (n_out - 1, n_out, n_out - 1), (0, 1, 0)]
    return [(1, 256, a, set(range(len(a))) if impulse else ties), (tf, 8, b, set(range(len(b))) if impulse else set())]


_REF = {}


def _reference(n, C, hop, pad_mode, delays):
    """per-frame curves at max_lag = 127 in float64 and float32 (the narrower ranges are columns of them), computed once"""
    key = (n, C, hop, pad_mode, delays)
    if key not in _REF:
        x = tdoa_ref.broadband(n, delays[:C], seed=n + C)
        c64, zeroed = tdoa_ref.frame_curves(x, hop, 127, pad_mode)
        assert zeroed == 0, (key, zeroed)                                  # the reference dropped no bin
        c64.setflags(write=False)
        _REF[key] = (x, c64, tdoa_ref.frame_curves_f32(x, hop, 127, pad_mode))
    return _REF[key]


def _against_float64(C, hop, pad_mode, lengths, max_lags=(1, 24, 127)):
    from sed_crnn_amd import feature
    worst_ratio, worst_lag, worst_kernel = 0.0, 0.0, 0.0
    for max_lag in max_lags:
        for n in lengths:
            x, c64, c32 = _reference(n, C, hop, pad_mode, NEAR if max_lag == 1 else DELAYS)
            c64, c32 = tdoa_ref.narrow(c64, max_lag), tdoa_ref.narrow(c32, max_lag)
            pcm, clips = _planar(x)
            for tf, max_frames, rows, ties in _tables(c64.shape[0], pad_mode, impulse=n == 1):
                ref = tdoa_ref.event_tdoa(c64, rows, tf, max_frames)
                nf = ref["loc_frames"]
                assert (nf > 0).all()
                # on these inputs no other searched lag comes within half the peak: the arg-max comparison is no near-tie
                # (only the flagged events — ties by construction, see _tables — may be, and only there is a pair left out)
                clear = ref["second"] < 0.5
                flagged = np.isin(np.arange(len(rows)), sorted(ties))
                assert clear[~flagged].all(), (C, hop, pad_mode, max_lag, n, float(ref["second"][~flagged].max()))
                # (a flagged event's peak at the level of float32 rounding, 1e-6 per frame, is no peak to compare either)
                clear = clear & (~flagged[:, None] | (ref["strength"] > 1e-6))
                got = feature.event_tdoa(pcm, clips, C, _events(rows), tf, max_lag=max_lag, max_frames=max_frames, hop=hop,
                                         pad_mode=pad_mode, return_curve=True)
                assert np.array_equal(got["loc_frames"].cpu().numpy(), nf)
                acc, lag, strength = (got[k].cpu().numpy() for k in ("acc", "lag", "strength"))
                assert acc.shape == ref["acc"].shape and np.isfinite(acc).all() and np.isfinite(lag).all() and np.isfinite(strength).all()
                assert np.array_equal(np.floor(lag.astype(np.float64) + 0.5).astype(np.int64)[clear], ref["t"][clear]), (C, hop, pad_mode, max_lag, n)
                per = nf[:, None, None].astype(np.float64)
                yard = tdoa_ref.yardstick_acc(c32, ref["ranges"]).astype(np.float64)
                e_yard, e_kernel = np.abs(yard / per - ref["acc"] / per).max(), np.abs(acc / per - ref["acc"] / per).max()
                degenerate = e_yard < DEGENERATE
                if degenerate:
                    e_yard = 2.0 ** -24
                # lag and strength: the formula in float64 on the kernel's own curve; only that formula's rounding may differ
                e_lag = 0.0
                for e in range(len(rows)):
                    for p in range(acc.shape[1]):
                        l64, s64, _, _ = tdoa_ref.peak(acc[e, p], int(nf[e]))
                        e_lag = max(e_lag, abs(float(lag[e, p]) - l64) / (EPS32 * max(1.0, abs(l64))),
                                    abs(float(strength[e, p]) - s64) / EPS32)
                print(f"C={C} hop={hop} {pad_mode} max_lag={max_lag} n={n} tf={tf}: yardstick {e_yard:.2e}{' (degenerate: replaced)' if degenerate else ''}"
                      f"  kernel {e_kernel:.2e}  ratio {e_kernel / e_yard:.2f}  lag/strength rounding {e_lag:.2f} eps")
                worst_ratio, worst_lag, worst_kernel = max(worst_ratio, e_kernel / e_yard), max(worst_lag, e_lag), max(worst_kernel, e_kernel)
                assert e_kernel <= 8.0 * e_yard, (C, hop, pad_mode, max_lag, n, tf, e_kernel, e_yard)
                assert e_lag <= LAG_BOUND, (C, hop, pad_mode, max_lag, n, tf, e_lag)
                assert np.abs(strength).max() <= 1.0 + 1e-6
    print(f"C={C} hop={hop} {pad_mode}: worst kernel error {worst_kernel:.2e}, worst kernel / yardstick {worst_ratio:.2f}, "
          f"worst lag / strength rounding {worst_lag:.2f} eps")


# ───────────── 1. against float64 ─────────────
@pytest.mark.parametrize("pad_mode", ["constant", "reflect"])
@pytest.mark.parametrize("hop", [1024, 441])
@pytest.mark.parametrize("C", [2, 3, 4])
def test_event_tdoa_matches_the_float64_definition(sed, C, hop, pad_mode):
    """loc_frames exact; round(lag) the reference's t* for every event and pair; acc / loc_frames within 8 x the float32
    yardstick's error (spatial_ref.gcc_phat_f32 rows summed in float32 in frame order; a yardstick below 1e-9 is exact arithmetic
    and is replaced by 2^-24, test_gpu_spatial's rule); lag and strength within LAG_BOUND roundings of the float64 formula on
    the kernel's own curve."""
    _against_float64(C, hop, pad_mode, LENGTHS)


def test_event_tdoa_of_eight_channels_in_batches_of_pairs(sed):
    """C = 8: the 28 accumulators do not fit LDS beside the spectra, so the pairs go 5 at a time and the frames are transformed
    again for every batch; same reference, same bounds"""
    _against_float64(8, 1024, "constant", (1, 40000), (24,))
    _against_float64(8, 441, "reflect", (5000,), (24,))


# ───────────── 2. physical ─────────────
def test_integer_delays_come_back(sed):
    from sed_crnn_amd import feature
    C, max_lag = 4, 8
    x = tdoa_ref.broadband(9000, DELAYS[:C], seed=5)
    pcm, clips = _planar(x)
    got = feature.event_tdoa(pcm, clips, C, _events([(0, 9, 4), (1, 4, 2), (2, 3, 2)]), 1, max_lag=max_lag)
    lag = got["lag"].cpu().numpy()
    inside = 0
    for p, (i, j) in enumerate(spatial_ref.pairs(C)):
        d = DELAYS[j] - DELAYS[i]                                         # channel j lags channel i by d samples: lag = -d
        if abs(d) <= max_lag:
            inside += 1
            assert (np.abs(lag[:, p] + d) <= 0.5).all(), (i, j, lag[:, p])
        else:
            assert (np.abs(lag[:, p]) <= max_lag + 0.5).all(), (i, j, lag[:, p])
    assert inside == 3 and (got["strength"].cpu().numpy()[:, [0, 1, 4]] > 0.3).all()


# ───────────── 3. bit for bit ─────────────
def _same_outputs(a, b, what, rows=slice(None)):
    for k in a:
        assert np.array_equal(_bits(a[k][rows]), _bits(b[k])), (what, k)


@pytest.mark.parametrize("hop", [1024, 441])
def test_batch_permutation_alignment_and_slices_change_no_bit(sed, hop):
    """hop 1024: in the single-recording calls every channel is 16-byte aligned and the interior frames take the plain 8-byte loads
    (the kernel's fast path needs an even hop, an 8-byte-aligned channel and a frame inside the clip); in the batch the last
    recording's channels start at odd samples, so the same frames go through the guarded loads.  hop 441: every frame is on the
    guarded path either way."""
    from sed_crnn_amd import feature
    C, lengths = 3, (45000, 1, 9000)
    waves = [tdoa_ref.broadband(n, DELAYS[:C], seed=n) for n in lengths]
    tables = [_tables(1 + n // hop)[0][2] + [(0, 999, 0)] for n in lengths]
    assert hop != 1024 or sum(f * hop >= 1024 and f * hop + 1024 <= 9000 for f in range(1 + 9000 // hop)) == 7   # interior frames
    kw = dict(max_lag=24, max_frames=40, hop=hop, return_curve=True)
    singles = []
    for w, rows in zip(waves, tables):
        pcm, clips = _planar(w)
        singles.append(feature.event_tdoa(pcm, clips, C, _events(rows), 1, **kw))
    # the three recordings in one buffer; every channel of the last one starts at an odd sample: guarded loads for all its frames
    pieces, clips, at = [], [], 0
    for r, w in enumerate(waves):
        for c in range(C):
            lead = (-at) % 4 + (3 if r == 2 else 0)
            pieces.append(np.zeros(lead, np.float32))
            at += lead
            clips.append((at, w.shape[0]))
            pieces.append(np.ascontiguousarray(w[:, c]))
            at += w.shape[0]
    assert all(clips[2 * C + c][0] % 2 == 1 for c in range(C)) and all(clips[c][0] % 4 == 0 for c in range(C))
    buf = torch.from_numpy(np.concatenate(pieces)).cuda()
    rows = [r for t in tables for r in t]
    rec = [i for i, t in enumerate(tables) for _ in t]
    many = feature.event_tdoa(buf, clips, C, _events(rows, rec), 1, **kw)
    at = 0
    for i, one in enumerate(singles):
        _same_outputs(many, one, f"recording {i} of the batch", slice(at, at + len(tables[i])))
        at += len(tables[i])
    assert singles[2]["loc_frames"].max() == 1 + 9000 // hop and singles[0]["loc_frames"].max() == 40      # whole and capped events ran
    # a permuted event table gives permuted outputs
    perm = np.random.default_rng(0).permutation(len(rows))
    shuffled = feature.event_tdoa(buf, clips, C, _events([rows[i] for i in perm], [rec[i] for i in perm]), 1, **kw)
    for k in many:
        assert np.array_equal(_bits(shuffled[k]), _bits(many[k][torch.from_numpy(perm).cuda()])), k
    # a workspace of one event at a time (as many slices as events) against all at once
    tiny = feature.event_tdoa(buf, clips, C, _events(rows, rec), 1, max_workspace_bytes=1, **kw)
    _same_outputs(tiny, many, "one event per slice")
    few = feature.event_tdoa(buf, clips, C, _events(rows, rec), 1, max_workspace_bytes=5 * 2 * 3 * 1026 * 8 + 4096, **kw)
    _same_outputs(few, many, "five events per slice")


# ───────────── 4. silence and junk ─────────────
def test_silence_and_junk_events(sed):
    from sed_crnn_amd import feature
    C = 3
    pcm, clips = _planar(np.zeros((5000, C), np.float32))
    got = feature.event_tdoa(pcm, clips, C, _events([(0, 5, 2), (1, 2, 1)]), 1, return_curve=True)
    assert got["loc_frames"].tolist() == [5, 1]
    for k in ("lag", "strength", "acc"):
        assert not got[k].any() and torch.isfinite(got[k]).all(), k
    x = tdoa_ref.broadband(5000, DELAYS[:C], seed=9)
    x[:, 1] = 0.0                                                          # one silent channel: its two pairs are silent
    pcm, clips = _planar(x)
    got = feature.event_tdoa(pcm, clips, C, _events([(0, 5, 2)]), 1)
    assert got["lag"][0].tolist()[0] == 0.0 and got["lag"][0].tolist()[2] == 0.0 and abs(got["lag"][0, 1].item() - 3.0) <= 0.5
    assert got["strength"][0].tolist()[0] == 0.0 and got["strength"][0, 1].item() > 0.3
    # junk: a recording that does not exist, events beyond the recording's end, a negative onset — between two good events
    x2 = tdoa_ref.broadband(3000, DELAYS[:C], seed=10)
    buf, cl = _planar(np.concatenate([x, np.zeros((1, C), np.float32), x2]))
    cl = [(o, 5000) for o, _ in cl] + [(o + 5001, 3000) for o, _ in cl]
    rows = [(0, 5, 2), (0, 5, 2), (0, 5, 2), (5, 9, 6), (1000000000, 1000000001, 3), (-2, 3, 0), (0, 3, 1)]
    rec = [0, 2, -1, 0, 1, 1, 1]
    got = feature.event_tdoa(buf, cl, C, _events(rows, rec), 1, return_curve=True)
    assert got["loc_frames"].tolist() == [5, 0, 0, 0, 0, 0, 3]
    for k in ("lag", "strength", "acc"):
        assert not got[k][1:6].any(), k
    assert got["strength"][6, 1].item() > 0.3
    # no events: empty tensors, nothing launched
    got = feature.event_tdoa(buf, cl, C, _events(np.zeros((0, 3)), []), 1, max_lag=5, return_curve=True)
    assert got["lag"].shape == (0, 3) and got["strength"].shape == (0, 3) and got["loc_frames"].shape == (0,) and got["acc"].shape == (0, 3, 13)
    assert got["loc_frames"].dtype == torch.int32 and got["lag"].is_cuda


# ───────────── 5. the detector ─────────────
def _same(a, b, what, keys=("lag", "strength", "loc_frames")):
    assert torch.equal(a.probs, b.probs), what
    _assert_events_equal({k: v.cpu().numpy() for k, v in a.events.items()}, {k: v.cpu().numpy() for k, v in b.events.items()}, what)
    assert not keys or set(a.events) == set(b.events), what
    for k in keys:
        assert np.array_equal(_bits(a.events[k]), _bits(b.events[k])), (what, k)


def _end_to_end(sed, plain, x, other_clips, C, spatial):
    from sed_crnn_amd import feature
    from sed_crnn_amd.resample import resample_many
    t = sed.TDOA(max_lag=12, max_frames=48)
    det = sed.EventDetector(plain.model, max_batch=1, median=3, mean=plain.mean, std=plain.std, spatial=spatial, localize=t)
    a, b = det(x, sr=48000, channels=C), plain(x, sr=48000, channels=C)
    assert len(b) > 0 and set(b.events) == {"cls", "onset", "offset", "peak", "peak_frame"}
    _same(a, b, "the five event keys and the track with and without localize", keys=())
    assert set(a.events) == set(b.events) | {"lag", "strength", "loc_frames"}
    P = C * (C - 1) // 2
    assert a.events["lag"].shape == (len(a), P) and a.events["loc_frames"].shape == (len(a),)
    pcm, clips = resample_many([x], 48000, det.sr, C, "cuda", keep_channels=True)
    want = feature.event_tdoa(pcm, clips, C, b.events, det.model.time_factor, max_lag=12, max_frames=48, hop=det.hop_length)
    for k in want:
        assert np.array_equal(_bits(a.events[k]), _bits(want[k])), k
    tf = det.model.time_factor
    on, off = b.events["onset"].cpu().numpy(), b.events["offset"].cpu().numpy()
    assert np.array_equal(a.events["loc_frames"].cpu().numpy(), np.minimum((off - on) * tf, 48))
    assert np.array_equal(a.tdoa(), a.events["lag"].cpu().numpy().astype(np.float64) / det.sr) and a.tdoa(0).shape == (len(b.intervals(0)), P)
    # batches: 48 kHz int16 interleaved input, res[i] against the single calls
    waves, rates = [x] + other_clips, [48000] * (1 + len(other_clips))
    res = det.detect_many(waves, sr=rates, channels=C)
    assert "lag" not in plain.detect_many(waves, sr=rates, channels=C).events
    for i, w in enumerate(waves):
        _same(res[i], det(w, sr=48000, channels=C), f"detect_many clip {i}")
    # from_features leaves the events un-located; det.localize adds the same bits
    mel = feature.mbe(x, input_sr=48000, channels=C, keep_channels=True, spatial=spatial, device="cuda", mean=det.mean, std=det.std)
    bare = det.from_features(mel)
    assert "lag" not in bare.events
    _same(det.localize(plain.from_features(mel), x, sr=48000, channels=C), a, "localize after from_features")
    many = det.localize(plain.from_features_many([mel, mel]), [x, x], sr=48000)
    _same(many[1], a, "localize of a batch")
    with pytest.raises(ValueError, match="feature frames"):
        det.localize(plain.from_features(mel), x[:-5000], sr=48000)
    with pytest.raises(NotImplementedError):
        det.stream(1)


def test_localising_detector_of_a_two_channel_net(sed, det2):
    plain, x = det2
    _end_to_end(sed, plain, x, [_stereo(48000 * 2 + 5, 48000, 2), _stereo(30000, 48000, 3)], 2, None)


def test_localising_detector_of_a_spatial_net(sed, det3):
    plain, x = det3
    _end_to_end(sed, plain, x, [_stereo16(48000 * 2 + 5, 2), _stereo16(30000, 3)], 2, "gcc_phat")
