#!/usr/bin/env python3
"""Multichannel audio in (csrc/resample.hip sed_resample_select, csrc/logmel.hip sed_logmel_multi).  Two
measurements, device-resident input:
  features    --seconds (one hour) of 48 kHz 4-channel int16 -> scaled features [N, 4*40] through
              feature.mbe(..., channels=4, keep_channels=True), next to the hand-written loop it replaces: per channel
              sed.resample(x[:, c], 48000) + feature.mbe with the sliced scaler, then torch.cat(dim=1).  The two results are
              compared bit for bit at the timed size first.  Algorithmic bytes: the interleaved frames once + the features;
              the per-channel staging of the first version reads the frames once per channel (what_it_reads).
  streams     one push of 0.74 s to each of --streams stereo int16 feeds of a 2-channel net at 48 kHz, next to the same push
              of mono feeds to the same net with one input channel (host wall clock to the push's blocking read).
Every figure is a median over --reps repetitions after a warm-up; alternatives alternate in one process.  One JSON line at
the end.  Exits non-zero when the new path is slower than the loop it replaces, or differs from it.
python tools/multichannel_bench.py [--seconds 3600] [--reps 10] [--streams 1024]"""
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
from sed_crnn_amd.resample import ResamplePlan

C, F = 4, feature.NB_MEL


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=int, default=3600)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--streams", type=int, default=1024)
    ap.add_argument("--pushes", type=int, default=20)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("multichannel_bench needs the GPU: nothing is measured without one")
    gen = torch.Generator(device="cuda").manual_seed(0)
    plan = ResamplePlan(48000)
    n_in = 48000 * a.seconds
    n_out = plan.n_out(n_in)
    rows = 1 + n_out // feature.HOP
    out = {"tool": "multichannel_bench", "seconds": a.seconds, "channels": C}
    x = torch.randint(-8000, 8000, (n_in, C), device="cuda", generator=gen, dtype=torch.int16)
    mean = torch.randn(C * F, device="cuda", generator=gen, dtype=torch.float64) - 8.0
    std = torch.rand(C * F, device="cuda", generator=gen, dtype=torch.float64) + 0.5

    def new_path():
        return feature.mbe(x, input_sr=48000, channels=C, keep_channels=True, mean=mean, std=std)

    def loop():
        return torch.cat([feature.mbe(sed.resample(x[:, c], 48000), mean=mean[c * F:(c + 1) * F], std=std[c * F:(c + 1) * F])
                          for c in range(C)], 1)

    with torch.no_grad():
        same = torch.equal(new_path(), loop())
        t_new, t_loop = med([new_path, loop], a.reps)
        need = n_in * C * 2 + rows * C * F * 4                      # the frames once + the features
        reads = n_in * C * 2 * C                                    # every (clip, channel) row stages its own tile of the frames
        out["features"] = {"rows": rows, "new_ms": round(t_new, 4), "loop_ms": round(t_loop, 4), "bitwise_equal": bool(same),
                           "algorithmic_GBps": round(need / t_new / 1e6, 1), "frame_bytes_requested": reads, "frame_bytes": n_in * C * 2}
        print(f"{a.seconds} s of 48 kHz {C}-channel int16 -> features [{rows}, {C * F}]: new path {t_new:.3f} ms "
              f"({need / t_new / 1e6:.0f} GB/s algorithmic), per-channel loop {t_loop:.3f} ms, ratio {t_loop / t_new:.2f}x, "
              f"bit for bit equal: {same}; the per-channel rows request the interleaved frames {C} times "
              f"({reads / 1e9:.2f} GB for {n_in * C * 2 / 1e9:.2f} GB)", flush=True)
        del x
        # streams: 0.74 s per feed and push (one window hop at the output rate)
        S = a.streams
        n48 = 32 * 1024 * 160 // 147 + 1
        dets = [sed.EventDetector(sed.LightningTimePooledCRNN(in_channels=ch).cuda().eval(), median=3) for ch in (2, 1)]
        p2 = [torch.randint(-8000, 8000, (S, n48, 2), device="cuda", generator=gen, dtype=torch.int16) for _ in range(2)]
        p1 = [torch.randint(-8000, 8000, (S, n48), device="cuda", generator=gen, dtype=torch.int16) for _ in range(2)]
        st2, st1 = dets[0].stream(S, input_sr=48000), dets[1].stream(S, input_sr=48000)
        for i in range(6):
            st2.push(list(p2[i % 2]))
            st1.push(list(p1[i % 2]))
        w2, w1 = [], []
        for i in range(a.pushes):
            w2.append(wall(lambda: st2.push(list(p2[i % 2])))[0])
            w1.append(wall(lambda: st1.push(list(p1[i % 2])))[0])
        out["streams"] = {"S": S, "push_stereo_ms": round(float(np.median(w2)), 4), "push_mono_ms": round(float(np.median(w1)), 4),
                          "state_bytes_per_stream": [st2.state_bytes // S, st1.state_bytes // S]}
        print(f"S={S}: push of {n48 / 48000:.2f} s at 48 kHz int16, stereo feeds of a 2-channel net {np.median(w2):.3f} ms, mono feeds "
              f"of a 1-channel net {np.median(w1):.3f} ms; state per feed {st2.state_bytes // S} vs {st1.state_bytes // S} B", flush=True)
    print(json.dumps(out))
    if not same:
        raise SystemExit("the new path differs from the loop it replaces")
    if t_new > t_loop:
        raise SystemExit(f"the new path ({t_new:.3f} ms) is slower than the loop it replaces ({t_loop:.3f} ms)")


if __name__ == "__main__":
    main()
