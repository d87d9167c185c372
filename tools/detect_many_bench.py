#!/usr/bin/env python3
"""Detection over many recordings: a loop of ``det(wave_r)`` against one ``det.detect_many(waves)``.
R synthetic mono clips of S seconds at 44.1 kHz (default 240 x 30 s = 2 h), resident on the device, for both nets
(LightningTimePooledCRNN and TimePooledCRNN(conv_channels=128)); the two paths alternate in one process.  Host wall clock
around work that ends in a synchronise, after a warm-up; median of --reps.  Also the per-phase device times of the batch
(hip events: log-mel, gather, forward, stitch, decode), the agreement of the two paths and one JSON line.
python tools/detect_many_bench.py [--clips 240] [--seconds 30] [--reps 5] [--hop 32] [--precision f32|bf16]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import sed_crnn_amd as sed
from sed_crnn_amd import data, feature

PHASES = ("logmel", "gather", "forward", "stitch", "decode")


def loop(det, waves):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = [det(w) for w in waves]                        # each call reads its event count: synchronises
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, res


def batch(det, waves):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = det.detect_many(waves)                         # reads the R+1 event offsets once: synchronises
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, res


def batch_phases(det, waves):
    """the batch path phase by phase, hip events around each (marks per launch for the windowed forward)"""
    m = det.model
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(5)]
    marks = []
    with torch.no_grad():
        bp = sed.plan_batch([1 + w.numel() // det.hop_length for w in waves], m.time_factor, m.dense[-1], det.seq_len, det.hop,
                            det.trim)
        ev[0].record()
        mel, _ = feature.mbe_many(waves, hop=det.hop_length, n_mels=m.n_mels, mean=det.mean, std=det.std)
        ev[1].record()
        logits = det.window_logits_many(mel, bp, marks)
        ev[2].record()
        probs = det.stitch_many(logits, bp)
        ev[3].record()
        det.decode_many(probs, bp)
        ev[4].record()
    torch.cuda.synchronize()
    gather = sum(a.elapsed_time(b) for name, a, b in marks if name == "gather")
    forward = sum(a.elapsed_time(b) for name, a, b in marks if name == "forward")
    return [ev[0].elapsed_time(ev[1]), gather, forward, ev[2].elapsed_time(ev[3]), ev[3].elapsed_time(ev[4])], \
        ev[1].elapsed_time(ev[2]), len(bp.full_starts) + sum(len(g[1]) for g in bp.groups)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=240)
    ap.add_argument("--seconds", type=float, default=30.0)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--hop", type=int, default=32)
    ap.add_argument("--max-batch", type=int, default=1024)
    ap.add_argument("--precision", choices=("f32", "bf16"), default="f32")
    a = ap.parse_args()
    torch.manual_seed(0)
    rng = np.random.default_rng(0)
    n = int(a.seconds * feature.SR)
    t = np.arange(n, dtype=np.float64) / feature.SR
    waves = []
    for r in range(a.clips):                            # a burst of a few seconds somewhere in every clip
        hits = (np.sin(2 * np.pi * (0.05 + 0.01 * (r % 7)) * t + r) > 0.9).astype(np.float32)
        w = (0.05 * rng.standard_normal(n) + hits * np.sin(2 * np.pi * 2000 * t)).astype(np.float32)
        waves.append(torch.from_numpy(w).cuda())
    mean, std = data.standard_scaler_fit(feature.mbe(waves[0]))
    out = {"tool": "detect_many_bench", "clips": a.clips, "seconds": a.seconds, "hop": a.hop, "max_batch": a.max_batch,
           "precision": a.precision, "nets": {}}
    for name, m in (("lightning", sed.LightningTimePooledCRNN()), ("timepooled128", sed.TimePooledCRNN(conv_channels=128))):
        m = m.cuda().eval().set_inference_precision(a.precision)
        det = sed.EventDetector(m, hop=a.hop, max_batch=a.max_batch, median=3, mean=mean, std=std)
        with torch.no_grad():
            _, one = loop(det, waves)                       # warm-up of both paths: workspaces, tables, buffer sizes
            _, many = batch(det, waves)
            loops, batches = [], []
            for _ in range(a.reps):                          # alternate the two paths
                loops.append(loop(det, waves)[0])
                batches.append(batch(det, waves)[0])
        dp = max((many[i].probs - one[i].probs).abs().max().item() for i in range(a.clips))
        n_loop, n_batch = sum(len(r) for r in one), many.n_events
        ph = [batch_phases(det, waves) for _ in range(a.reps)]
        med = [float(np.median([p[0][i] for p in ph])) for i in range(len(PHASES))]
        windows_span = float(np.median([p[1] for p in ph]))
        lm, bm = float(np.median(loops)), float(np.median(batches))
        out["nets"][name] = {"loop_ms": round(lm, 3), "batch_ms": round(bm, 3), "speedup": round(lm / bm, 3),
                             "loop_ms_per_clip": round(lm / a.clips, 4), "batch_ms_per_clip": round(bm / a.clips, 4),
                             "batch_phase_ms": {p: round(v, 4) for p, v in zip(PHASES, med)},
                             "batch_windows_span_ms": round(windows_span, 4), "windows": ph[0][2],
                             "max_abs_dp": dp, "events_loop": n_loop, "events_batch": n_batch}
        print(f"{name}: loop {lm:.2f} ms ({lm / a.clips:.3f} ms/clip), batch {bm:.2f} ms ({bm / a.clips:.3f} ms/clip), "
              f"x{lm / bm:.2f}; batch phases " + ", ".join(f"{p} {v:.3f}" for p, v in zip(PHASES, med)) +
              f" ms (gather+forward span {windows_span:.3f} ms); agreement: max |dp| {dp:.2e}, events {n_loop} vs {n_batch}",
              flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
