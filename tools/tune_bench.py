#!/usr/bin/env python3
"""Tuning the event decoder: one ``det.sweep`` over a grid of settings against a loop of bare ``det.decode_many`` calls, one per
setting, with NO host-side scoring at all (which favours the loop: it would still have to copy and match every event).
Synthetic smooth tracks (sigmoid of a sine of a random walk), about --hours of output frames split into --recordings
recordings of uneven length, K classes; the reference events are the decode of a perturbed copy of the track.  Both paths
alternate in one process; host wall clock around work that ends in a synchronise, after a warm-up; median of --reps.
n_sys of every setting is checked against the real decoder's event count.  One JSON line at the end; the tool FAILS when the
sweep is slower than the loop.
python tools/tune_bench.py [--hours 10] [--recordings 300] [--classes 6] [--reps 20]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import sed_crnn_amd as sed


def make_tracks(rng, n_total, R, K):
    cuts = np.sort(rng.choice(np.arange(1, n_total), R - 1, replace=False))
    out_off = np.concatenate([[0], cuts, [n_total]]).tolist()
    walk = np.cumsum(rng.standard_normal((n_total, K)) * 0.08, 0)
    probs = (1 / (1 + np.exp(-3 * np.sin(walk)))).astype(np.float32)
    return probs, out_off


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--hours", type=float, default=10.0)
    ap.add_argument("--recordings", type=int, default=300)
    ap.add_argument("--classes", type=int, default=6)
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    rng = np.random.default_rng(0)
    K, R = a.classes, a.recordings
    m = sed.LightningTimePooledCRNN(dropout=0.0, n_classes=K).cuda().eval()
    det = sed.EventDetector(m)
    n_total = int(a.hours * 3600 / det.frame_seconds)
    probs_h, out_off = make_tracks(rng, n_total, R, K)
    probs = torch.from_numpy(probs_h).cuda()
    tf = m.time_factor
    bp = sed.plan_batch([tf * n for n in np.diff(out_off)], tf, K)         # decode_many takes R and out_off from it
    assert list(bp.out_off) == out_off
    # the reference: the decode of a perturbed copy
    noisy = torch.from_numpy(np.clip(probs_h + rng.standard_normal(probs_h.shape).astype(np.float32) * 0.05, 0, 1)).cuda()
    truth = det.with_decoder(threshold=0.55, low=0.45, median=5, min_gap=2, min_len=3)
    ev, offs = truth.decode_many(noisy, bp)
    ref = sed.ReferenceEvents.from_result(sed.BatchDetectionResult(noisy, ev, det.frame_seconds, bp.plans, out_off, offs))
    grid = sed.DecoderGrid(threshold=np.linspace(0.4, 0.75, 8), low=[0.3, 0.4, 0.45], median=[1, 3, 5, 9, 15], min_gap=[0, 2, 5],
                           min_len=[1, 3])
    kw = dict(collar=1, offset_collar=1, offset_percent=0.2)
    dets = [det.with_decoder(**grid[g]) for g in range(len(grid))]      # each keeps its own workspace and event buffers

    def run_sweep():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = det.sweep((probs, out_off), ref, grid, **kw)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, res

    def run_loop():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        n = [d.decode_many(probs, bp)[1][-1] for d in dets]        # each call reads its R+1 event offsets: synchronises
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, n

    _, res = run_sweep()                                 # warm-up of both paths
    _, n_events = run_loop()
    table = res.table()
    agree = all(int(table[g, :, 1].sum()) == n_events[g] for g in range(len(grid)))
    sweeps, loops = [], []
    for _ in range(a.reps):                              # alternate the two paths
        sweeps.append(run_sweep()[0])
        loops.append(run_loop()[0])
    sm, lm = float(np.median(sweeps)), float(np.median(loops))
    g, best, score = res.best()
    out = {"tool": "tune_bench", "hours": a.hours, "output_frames": n_total, "recordings": R, "classes": K, "settings": len(grid),
           "bit_tracks": res.n_tracks, "slices": res.n_slices, "workspace_bytes": res.workspace_bytes, "reference_events": len(ref),
           "reps": a.reps, "sweep_ms": round(sm, 3), "loop_ms": round(lm, 3), "ratio": round(lm / sm, 2),
           "loop_ms_per_setting": round(lm / len(grid), 4), "n_sys_equals_decoder_counts": bool(agree), "best_g": g, "best": best,
           "best_f1_event": round(score, 6)}
    print(f"{len(grid)} settings ({res.n_tracks} bit tracks, {res.workspace_bytes / 2 ** 20:.1f} MiB workspace) on {n_total} frames in "
          f"{R} recordings, K={K}: sweep {sm:.2f} ms, loop of decode_many {lm:.2f} ms ({lm / len(grid):.3f} ms per setting), "
          f"x{lm / sm:.1f}; n_sys == decoder counts for every setting: {agree}", flush=True)
    print(json.dumps(out))
    if not agree:
        sys.exit("n_sys of a setting differs from the decoder's event count")
    if sm > lm:                                          # the requirement: one sweep is no slower than the loop it replaces
        sys.exit(f"the sweep ({sm:.2f} ms) is slower than the loop of decode_many ({lm:.2f} ms)")


if __name__ == "__main__":
    main()
