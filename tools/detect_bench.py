#!/usr/bin/env python3
"""Whole-recording detection (sed_crnn_amd.EventDetector) on one hour of synthetic mono audio at 44.1 kHz, per phase:
log-mel (fused scaler), window gather and eval forward (per chunk of max_batch windows, summed over the chunks), stitch,
decode — hip events around each phase / launch, median of --reps runs after a warm-up.
Nets: LightningTimePooledCRNN and TimePooledCRNN(conv_channels=128).
python tools/detect_bench.py [--seconds 3600] [--reps 5] [--hop 32] [--precision f32|bf16]   -> one JSON line"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import sed_crnn_amd as sed
from sed_crnn_amd import data, feature

PHASES = ("logmel", "gather", "forward", "stitch", "decode")


def run_once(det, wave, mean, std):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
    marks = []
    with torch.no_grad():
        ev[0].record()
        mel = feature.mbe(wave, mean=mean, std=std)
        ev[1].record()
        mel, plan = det._prepare(mel)
        logits = det.window_logits(mel, plan, marks)     # gather and forward alternate per chunk: timed launch by launch
        probs = det.stitch(logits, plan)
        ev[2].record()
        events = det.decode(probs)                       # reads the event count: synchronises
        ev[3].record()
    torch.cuda.synchronize()
    gather = sum(a.elapsed_time(b) for name, a, b in marks if name == "gather")
    forward = sum(a.elapsed_time(b) for name, a, b in marks if name == "forward")
    stitch_ms = marks[-1][2].elapsed_time(ev[2])          # from the last forward's end to the stitch's end
    return ([ev[0].elapsed_time(ev[1]), gather, forward, stitch_ms, ev[2].elapsed_time(ev[3])], plan, len(events["cls"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=3600.0)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--hop", type=int, default=32)
    ap.add_argument("--max-batch", type=int, default=1024)
    ap.add_argument("--precision", choices=("f32", "bf16"), default="f32")
    a = ap.parse_args()
    torch.manual_seed(0)
    rng = np.random.default_rng(0)
    n = int(a.seconds * feature.SR)
    t = np.arange(n, dtype=np.float64) / feature.SR
    hits = (np.sin(2 * np.pi * 0.05 * t) > 0.95).astype(np.float32)           # a burst every 20 s
    wave = (0.05 * rng.standard_normal(n) + hits * np.sin(2 * np.pi * 2000 * t)).astype(np.float32)
    wave = torch.from_numpy(wave).cuda()
    mean, std = data.standard_scaler_fit(feature.mbe(wave))
    out = {"tool": "detect_bench", "seconds": a.seconds, "hop": a.hop, "max_batch": a.max_batch, "precision": a.precision,
           "nets": {}}
    for name, m in (("lightning", sed.LightningTimePooledCRNN()), ("timepooled128", sed.TimePooledCRNN(conv_channels=128))):
        m = m.cuda().eval().set_inference_precision(a.precision)
        det = sed.EventDetector(m, hop=a.hop, max_batch=a.max_batch, median=3)
        run_once(det, wave, mean, std)                                         # warm-up: workspaces, tables
        runs = [run_once(det, wave, mean, std) for _ in range(a.reps)]
        med = [float(np.median([r[0][i] for r in runs])) for i in range(len(PHASES))]
        plan = runs[0][1]
        out["nets"][name] = {"ms": {p: round(v, 4) for p, v in zip(PHASES, med)}, "total_ms": round(sum(med), 4),
                             "frames": plan.n_frames, "out_frames": plan.n_out, "windows": plan.n_win, "events": runs[0][2]}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
