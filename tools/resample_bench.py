#!/usr/bin/env python3
"""Resampling front end (sed_crnn_amd/resample.py, csrc/resample.hip).  Three measurements, device-resident input:
  kernel      one hour of 48 kHz stereo int16 -> 44.1 kHz mono float32: time, algorithmic GB/s (bytes read + written) and
              multiply-adds per second, next to the same hour as mono float32;
  front end   the same hour through resample + log-mel, next to log-mel alone on an hour that already is 44.1 kHz mono;
  streams     one push of 0.74 s to each of --streams feeds at 48 kHz int16, next to the same push at 44.1 kHz float
              (host wall clock to the push's blocking read, and the device time of the resample launch).
Every figure is a median over --reps repetitions after a warm-up; alternatives alternate in one process.  One JSON line at
the end.  python tools/resample_bench.py [--seconds 3600] [--reps 10] [--streams 1024]"""
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
        raise SystemExit("resample_bench needs the GPU: nothing is measured without one")
    gen = torch.Generator(device="cuda").manual_seed(0)
    plan = ResamplePlan(48000)
    n_in = 48000 * a.seconds
    n_out = plan.n_out(n_in)
    out = {"tool": "resample_bench", "seconds": a.seconds, "taps": plan.K, "phases": plan.L}
    stereo16 = torch.randint(-8000, 8000, (n_in, 2), device="cuda", generator=gen, dtype=torch.int16)
    mono32 = torch.randn(n_in, device="cuda", generator=gen) * 0.1
    at441 = torch.randn(n_out, device="cuda", generator=gen) * 0.1
    with torch.no_grad():
        t16, t32 = med([lambda: sed.resample(stereo16, 48000, channels=2), lambda: sed.resample(mono32, 48000)], a.reps)
        macs = n_out * plan.K
        for name, t, nbytes in (("stereo_int16", t16, n_in * 4 + n_out * 4), ("mono_float32", t32, n_in * 4 + n_out * 4)):
            out[name] = {"ms": round(t, 4), "GBps": round(nbytes / t / 1e6, 1), "GMACps": round(macs / t / 1e6, 1)}
            print(f"{a.seconds} s of 48 kHz {name} -> 44.1 kHz mono: {t:.3f} ms, {nbytes / t / 1e6:.0f} GB/s algorithmic "
                  f"({nbytes / t / 1e6 / 8000 * 100:.1f} % of 8 TB/s), {macs / t / 1e6:.0f} G multiply-adds/s "
                  f"({2 * macs / t / 1e9 / 157.3 * 100:.1f} % of 157.3 TFLOP/s fp32 vector)", flush=True)
        both, alone = med([lambda: feature.mbe(stereo16, input_sr=48000, channels=2), lambda: feature.mbe(at441)], a.reps)
        out["front_end"] = {"resample_logmel_ms": round(both, 4), "logmel_alone_ms": round(alone, 4)}
        print(f"the same hour through resample + log-mel: {both:.3f} ms; log-mel alone on 44.1 kHz mono: {alone:.3f} ms", flush=True)
        del stereo16, mono32, at441
        # streams: 0.74 s per feed and push (one window hop at the output rate)
        S = a.streams
        m = sed.LightningTimePooledCRNN().cuda().eval()
        det = sed.EventDetector(m, median=3)
        n48, n441 = 32 * 1024 * 160 // 147 + 1, 32 * 1024
        p48 = [torch.randint(-8000, 8000, (S, n48), device="cuda", generator=gen, dtype=torch.int16) for _ in range(2)]
        p441 = [torch.randn(S, n441, device="cuda", generator=gen) * 0.1 for _ in range(2)]
        st48, st441 = det.stream(S, input_sr=48000), det.stream(S)
        for i in range(6):
            st48.push(list(p48[i % 2]))
            st441.push(list(p441[i % 2]))
        w48, w441, dev = [], [], []
        for i in range(a.pushes):
            st48.marks = []
            w48.append(wall(lambda: st48.push(list(p48[i % 2])))[0])
            dev.append(sum(x.elapsed_time(y) for n, x, y in st48.marks if n == "resample"))
            st48.marks = None
            w441.append(wall(lambda: st441.push(list(p441[i % 2])))[0])
        out["streams"] = {"S": S, "push_48k_int16_ms": round(float(np.median(w48)), 4), "push_44k1_float_ms": round(float(np.median(w441)), 4),
                          "resample_device_ms": round(float(np.median(dev)), 4),
                          "state_bytes_per_stream": [st48.state_bytes // S, st441.state_bytes // S]}
        print(f"S={S}: push of {n48 / 48000:.2f} s at 48 kHz int16 {np.median(w48):.3f} ms (resample launch {np.median(dev):.3f} ms on the "
              f"device), at 44.1 kHz float {np.median(w441):.3f} ms; state per feed {st48.state_bytes // S} vs {st441.state_bytes // S} B",
              flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
