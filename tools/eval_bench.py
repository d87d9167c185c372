#!/usr/bin/env python3
"""Eval-mode forward (run_epoch with optim=None, sed.py:128-141) of BASELINE config 2 (or 5) on a resident batch:
python tools/eval_bench.py [--reps 30] [--precision f32|bf16] [--config 2|5]
(under rocprofv3 --kernel-trace --stats: the per-kernel split of the inference path)"""
import argparse, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import sed_crnn_amd as sed

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=30)
ap.add_argument("--B", type=int, default=None)
ap.add_argument("--T", type=int, default=None)
ap.add_argument("--precision", choices=("f32", "bf16"), default="f32", help="model.set_inference_precision (bf16: DESIGN 5e)")
ap.add_argument("--config", type=int, choices=(2, 5), default=2, help="2: mono 40 mel, BiGRU 2x128; 5: 4-ch 128 mel, BiGRU 2x256")
a = ap.parse_args()
torch.manual_seed(0)
if a.config == 2:
    a.B, a.T = a.B or 128, a.T or 256
    m = sed.TimePooledCRNN(conv_channels=128, dropout=0.5, gru_hidden=128)
    x = torch.randn(a.B, 1, 40, a.T).cuda()
else:
    a.B, a.T = a.B or 16, a.T or 512
    m = sed.TimePooledCRNN(conv_channels=128, dropout=0.5, in_channels=4, n_mels=128, gru_hidden=256)
    x = torch.randn(a.B, 4, 128, a.T).cuda()
m = m.cuda().eval().set_inference_precision(a.precision)
with torch.no_grad():
    for _ in range(5):
        m(x)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(a.reps + 1)]
    ev[0].record()
    for i in range(a.reps):
        m(x)
        ev[i + 1].record()
    torch.cuda.synchronize()
ms = sorted(ev[i].elapsed_time(ev[i + 1]) for i in range(a.reps))
med = ms[len(ms) // 2]
print(f"eval forward config {a.config} {a.precision} B={a.B} T={a.T} plan {m.inference_plan(a.B, a.T)}: median {med:.3f} ms  ({a.B * a.T / med / 1e3:.2f} M frames/s), min {ms[0]:.3f}")
