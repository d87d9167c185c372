#!/usr/bin/env python3
"""Per-event TDOA (csrc/tdoa.hip sed_event_tdoa).  --seconds (one hour) of 48 kHz 4-channel int16, device-resident,
resampled once to the detector's rate; synthetic event tables of --events (1 000 and 20 000) events of 5 to 200 output frames
(time factor 8), two ways:
  event_tdoa   feature.event_tdoa(pcm, clips, 4, events, 8, max_lag, max_frames) -> lag, strength, loc_frames
  features     the only route to these numbers without it: feature.mbe_planar(..., spatial="gcc_phat") with n_mels = 2 (max_lag + 2)
               (every frame's GCC at the lags -(max_lag+2) .. max_lag+1), then torch index-sums of the GCC columns over each
               event's rows (gather + index_add_, in slices of at most 2^20 rows; the row and event indices are made outside
               the timing).  `features_cumsum` is the same front end followed by one float64 prefix sum over the rows and a
               difference per event instead of the index-sums (reported; its sums are not those of the frames in order).
The accumulated curves of the two routes are compared (max abs difference per frame).  Then the cost that ``localize=`` adds to
``det(...)`` (--det-seconds of 4-channel audio) and ``detect_many(...)`` (8 clips of a minute) of a 4-channel net, against the
same detector without it.  Every figure is a median over --reps repetitions after a warm-up; the alternatives alternate in one
process.  One JSON line at the end.  Exits non-zero when event_tdoa is slower than the features route for an event table.
python tools/tdoa_bench.py [--seconds 3600] [--events 1000 20000] [--max-lag 24] [--max-frames 256] [--reps 10]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import sed_crnn_amd as sed
from sed_crnn_amd import feature
from sed_crnn_amd.resample import resample_many

C, TF = 4, 8
P = C * (C - 1) // 2


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def med(fns, reps):
    """alternate the callables ``reps`` times -> their median wall times in ms"""
    for fn in fns:
        fn()
    ts = [[] for _ in fns]
    for _ in range(reps):
        for t, fn in zip(ts, fns):
            t.append(wall(fn)[0])
    return [float(np.median(t)) for t in ts]


def event_table(E, n_feat, rng):
    """E events of 5..200 output frames anywhere in the recording, peak anywhere inside -> host int32 [E, 3]"""
    n_out = n_feat // TF
    dur = rng.integers(5, min(200, n_out) + 1, E)
    on = (rng.random(E) * (n_out - dur + 1)).astype(np.int64)
    pk = on + (rng.random(E) * dur).astype(np.int64)
    return np.stack([on, on + dur, pk], 1).astype(np.int32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=int, default=3600)
    ap.add_argument("--events", type=int, nargs="+", default=[1000, 20000])
    ap.add_argument("--max-lag", type=int, default=24)
    ap.add_argument("--max-frames", type=int, default=256)
    ap.add_argument("--det-seconds", type=int, default=600)
    ap.add_argument("--reps", type=int, default=10)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tdoa_bench needs the GPU: nothing is measured without one")
    if not 1 <= a.max_lag <= 62:
        raise SystemExit("the features route holds n_mels = 2 (max_lag + 2) <= 128 lags: max_lag <= 62")
    gen = torch.Generator(device="cuda").manual_seed(0)
    rng = np.random.default_rng(0)
    x = torch.randint(-8000, 8000, (48000 * a.seconds, C), device="cuda", generator=gen, dtype=torch.int16)
    pcm, clips = resample_many([x], 48000, feature.SR, C, "cuda", keep_channels=True)
    n_feat = 1 + clips[0][1] // feature.HOP
    L, W = 2 * (a.max_lag + 2), 2 * a.max_lag + 3
    out = {"tool": "tdoa_bench", "seconds": a.seconds, "channels": C, "pairs": P, "time_factor": TF, "max_lag": a.max_lag,
           "max_frames": a.max_frames, "feature_frames": n_feat, "tables": {}}
    slower = []
    with torch.no_grad():
        for E in a.events:
            rows = event_table(E, n_feat, rng)
            ev = {k: torch.from_numpy(np.ascontiguousarray(rows[:, i])).cuda() for i, k in enumerate(("onset", "offset", "peak_frame"))}
            rng_f = np.array([sed.event_frames(*r, TF, n_feat, a.max_frames) for r in rows.tolist()], dtype=np.int64)
            nf = rng_f[:, 1] - rng_f[:, 0]
            # the features route's indices: per slice of events, the rows to gather and the event each one belongs to
            slices, e0 = [], 0
            while e0 < E:
                e1 = e0 + max(1, int(np.searchsorted(np.cumsum(nf[e0:]), 1 << 20, side="right")))
                e1 = min(e1, E)
                r = np.concatenate([np.arange(f0, f1) for f0, f1 in rng_f[e0:e1]])
                who = np.repeat(np.arange(e0, e1), nf[e0:e1])
                slices.append((torch.from_numpy(r).cuda(), torch.from_numpy(who).cuda()))
                e0 = e1
            f0_d, f1_d = torch.from_numpy(rng_f[:, 0]).cuda(), torch.from_numpy(rng_f[:, 1]).cuda()

            def new(curve=False):
                return feature.event_tdoa(pcm, clips, C, ev, TF, max_lag=a.max_lag, max_frames=a.max_frames, return_curve=curve)

            def gcc_columns():
                feat, _ = feature.mbe_planar(pcm, clips, C, n_mels=L, spatial="gcc_phat")
                return feat[:, C * L:]

            def features():
                g = gcc_columns()
                acc = torch.zeros(E, P * L, device="cuda")
                for r, who in slices:
                    acc.index_add_(0, who, g[r])
                return acc

            def features_cumsum():
                cs = torch.cumsum(gcc_columns(), 0, dtype=torch.float64)
                cs = torch.cat([torch.zeros(1, P * L, device="cuda", dtype=torch.float64), cs])
                return (cs[f1_d] - cs[f0_d]).float()

            got = new(curve=True)
            assert np.array_equal(got["loc_frames"].cpu().numpy(), nf)
            old = features().view(E, P, L)[:, :, 1:]
            per = torch.from_numpy(nf).cuda().view(E, 1, 1).float()
            diff = float(((got["acc"] - old) / per).abs().max())
            del old, got
            t_new, t_old, t_cs = med([new, features, features_cumsum], a.reps)
            out["tables"][str(E)] = {"located_frames": int(nf.sum()), "event_tdoa_ms": round(t_new, 4), "features_ms": round(t_old, 4),
                                     "features_cumsum_ms": round(t_cs, 4), "acc_max_abs_diff_per_frame": diff}
            print(f"{E} events ({int(nf.sum())} located frames of a recording of {n_feat}): event_tdoa {t_new:.3f} ms, features + "
                  f"index-sums {t_old:.3f} ms ({t_old / t_new:.2f}x), features + float64 prefix sums {t_cs:.3f} ms; curves differ by at "
                  f"most {diff:.2e} per frame", flush=True)
            if t_new > t_old:
                slower.append(f"{E} events: event_tdoa {t_new:.3f} ms is slower than the features route {t_old:.3f} ms")
        del pcm, x
        # ── what localize= adds to the detector ──
        m = sed.LightningTimePooledCRNN(dropout=0.0, in_channels=C).cuda().eval()
        one = torch.randint(-8000, 8000, (48000 * a.det_seconds, C), device="cuda", generator=gen, dtype=torch.int16)
        # an untrained net: the threshold goes to the median of its track, so that there are events to locate
        thr = float(sed.EventDetector(m)(one, sr=48000, channels=C).probs.median())
        plain = sed.EventDetector(m, median=3, threshold=thr)
        loc = sed.EventDetector(m, median=3, threshold=thr, localize=sed.TDOA(a.max_lag, a.max_frames))
        many = [one[i * 48000 * 60:(i + 1) * 48000 * 60] for i in range(min(8, a.det_seconds // 60))]
        t_p, t_l = med([lambda: plain(one, sr=48000, channels=C), lambda: loc(one, sr=48000, channels=C)], a.reps)
        out["detector"] = {"seconds": a.det_seconds, "events": len(loc(one, sr=48000, channels=C)), "plain_ms": round(t_p, 4),
                           "localize_ms": round(t_l, 4)}
        print(f"det(...) on {a.det_seconds} s: {t_p:.3f} ms, with localize= {t_l:.3f} ms (+{t_l - t_p:.3f} ms for {out['detector']['events']} events)", flush=True)
        if many:
            t_p, t_l = med([lambda: plain.detect_many(many, sr=48000, channels=C), lambda: loc.detect_many(many, sr=48000, channels=C)], a.reps)
            out["detect_many"] = {"clips": len(many), "events": loc.detect_many(many, sr=48000, channels=C).n_events,
                                  "plain_ms": round(t_p, 4), "localize_ms": round(t_l, 4)}
            print(f"detect_many(...) on {len(many)} clips of 60 s: {t_p:.3f} ms, with localize= {t_l:.3f} ms (+{t_l - t_p:.3f} ms for "
                  f"{out['detect_many']['events']} events)", flush=True)
    print(json.dumps(out))
    if slower:
        raise SystemExit("; ".join(slower))


if __name__ == "__main__":
    main()
