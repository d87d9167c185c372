#!/usr/bin/env python3
"""Class-wise decoder settings: what one class-wise call costs next to what it replaces.
  decode      --hours of output frames (synthetic smooth tracks: sigmoid of a sine of a random walk), K = 6 classes with six
              different settings.  ONE class-wise ``det.decode`` against the loop of six scalar ``det.decode`` calls, one per
              distinct setting, that a user had to run before (keeping one class of each; the loop is timed WITHOUT that
              selection, which favours it).  The tool FAILS when the class-wise call is the slower one.
  equal rows  on the same build, class-wise decode with six EQUAL rows over the scalar decode with that setting: what the
              by-value table and the per-width launches cost when nothing differs.  Reported, no pass mark.
  push        one steady-state ``StreamDetector.push`` of --streams feeds (one window hop of audio each, resident on the
              device; the setting of tools/stream_bench.py, Lightning net), class-wise against scalar with the widest median.
The paths alternate in one process; device events around every call and a host wall clock around work that ends in a
synchronise, after a warm-up; medians of --reps.  The class-wise events are checked against the six scalar decodes class by
class.  One JSON line at the end.
python tools/classwise_bench.py [--hours 24] [--streams 1024] [--reps 20] [--pushes 40]"""
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

# (threshold, low, median, min_gap, min_len) per class
SETTINGS = ((.5, .5, 1, 0, 1), (.6, .4, 31, 17, 5), (.45, .45, 3, 1, 2), (.55, .5, 15, 3, 1), (.5, .42, 7, 0, 9), (.58, .52, 1, 40, 1))
NAMES = ("threshold", "low", "median", "min_gap", "min_len")


def timed(fn):
    """-> (device ms between two events, host wall ms around fn and a synchronise, fn's result)"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), (time.perf_counter() - t0) * 1e3, out


def med(xs, i):
    return float(np.median([x[i] for x in xs]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--hours", type=float, default=24.0)
    ap.add_argument("--streams", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--pushes", type=int, default=40)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("classwise_bench needs the GPU: there is nothing to measure without one")
    rng = np.random.default_rng(0)
    K = len(SETTINGS)
    m = sed.LightningTimePooledCRNN(dropout=0.0, n_classes=K).cuda().eval()
    base = sed.EventDetector(m)
    n = int(a.hours * 3600 / base.frame_seconds)
    walk = np.cumsum(rng.standard_normal((n, K)) * 0.15, 0)
    probs = torch.from_numpy(((1 / (1 + np.exp(-np.sin(walk)))) * 0.6 + 0.2).astype(np.float32)).cuda()
    cols = {name: [s[i] for s in SETTINGS] for i, name in enumerate(NAMES)}
    cw = base.with_decoder(**cols)
    scalars = [base.with_decoder(**dict(zip(NAMES, s))) for s in SETTINGS]     # each keeps its own workspace and event buffers
    equal = base.with_decoder(**{name: [SETTINGS[3][i]] * K for i, name in enumerate(NAMES)})
    assert cw.classwise and equal.classwise and not scalars[3].classwise

    run_cw = lambda: cw.decode(probs)                                          # noqa: E731
    run_loop = lambda: [d.decode(probs) for d in scalars]                      # noqa: E731
    run_eq = lambda: equal.decode(probs)                                       # noqa: E731
    run_one = lambda: scalars[3].decode(probs)                                 # noqa: E731
    for fn in (run_cw, run_loop, run_eq, run_one, run_cw, run_loop, run_eq, run_one):       # warm-up: buffers grown, code loaded
        fn()
    ev, per = run_cw(), run_loop()
    agree = all(torch.equal(ev[key][ev["cls"] == k].view(torch.int32), per[k][key][per[k]["cls"] == k].view(torch.int32))
                for k in range(K) for key in ev)
    eq, one = run_eq(), run_one()
    agree_eq = all(torch.equal(eq[key].view(torch.int32), one[key].view(torch.int32)) for key in eq)
    t = {name: [] for name in ("cw", "loop", "eq", "one")}
    for _ in range(a.reps):                                                    # alternate the paths
        for name, fn in (("cw", run_cw), ("loop", run_loop), ("eq", run_eq), ("one", run_one)):
            t[name].append(timed(fn)[:2])
    out = {"tool": "classwise_bench", "hours": a.hours, "output_frames": n, "classes": K, "reps": a.reps,
           "events": int(ev["cls"].numel()), "events_equal_the_scalar_decodes": bool(agree),
           "equal_rows_bitwise_the_scalar_decode": bool(agree_eq)}
    for name in t:
        out[f"{name}_device_ms"], out[f"{name}_wall_ms"] = round(med(t[name], 0), 4), round(med(t[name], 1), 4)
    out["loop_over_classwise"] = round(out["loop_wall_ms"] / out["cw_wall_ms"], 3)
    out["equal_rows_over_scalar"] = round(out["eq_wall_ms"] / out["one_wall_ms"], 3)
    out["equal_rows_over_scalar_device"] = round(out["eq_device_ms"] / out["one_device_ms"], 3)
    print(f"{n} frames x {K} classes, {out['events']} events: class-wise decode {out['cw_wall_ms']:.3f} ms wall "
          f"({out['cw_device_ms']:.3f} device), loop of {K} scalar decodes {out['loop_wall_ms']:.3f} ms ({out['loop_device_ms']:.3f}), "
          f"x{out['loop_over_classwise']:.2f}; equal rows {out['eq_wall_ms']:.3f} ms against scalar {out['one_wall_ms']:.3f} ms, "
          f"ratio {out['equal_rows_over_scalar']:.3f} (device {out['equal_rows_over_scalar_device']:.3f})", flush=True)

    # one steady-state push of S feeds, class-wise against scalar (the widest median: the same state and frontier)
    S, hop = a.streams, 32
    gen = torch.Generator(device="cuda").manual_seed(0)
    hop_samples = hop * feature.HOP
    pcm = 0.05 * torch.randn(2, S, hop_samples, device="cuda", generator=gen)
    pcm[1] += torch.sin(2 * np.pi * 2000 * torch.arange(hop_samples, device="cuda") / feature.SR)
    mean, std = data.standard_scaler_fit(feature.mbe(pcm[:, 0].reshape(-1)))
    pieces = [[pcm[i, s] for s in range(S)] for i in range(2)]
    widest = max(cols["median"])
    dets = {"classwise": sed.EventDetector(m, hop=hop, mean=mean, std=std, **cols),
            "scalar": sed.EventDetector(m, hop=hop, mean=mean, std=std, median=widest)}
    sts = {name: d.stream(n_streams=S) for name, d in dets.items()}
    push = {name: [] for name in sts}
    with torch.no_grad():
        for i in range(6):                                                     # warm-up: every feed past its first window
            for st in sts.values():
                st.push(pieces[i % 2])
        for i in range(a.pushes):                                              # alternate the two detectors
            for name, st in sts.items():
                st.marks = []
                _, wall, _ = timed(lambda: st.push(pieces[i % 2]))
                step = sum(x.elapsed_time(y) for n_, x, y in st.marks if n_ == "step")
                st.marks = None
                push[name].append((step, wall))
    for name in sts:
        out[f"push_{name}_wall_ms"], out[f"push_{name}_step_device_ms"] = round(med(push[name], 1), 4), round(med(push[name], 0), 4)
    out["streams"] = S
    out["push_classwise_over_scalar"] = round(out["push_classwise_wall_ms"] / out["push_scalar_wall_ms"], 3)
    print(f"push of {S} feeds: class-wise {out['push_classwise_wall_ms']:.3f} ms wall (step {out['push_classwise_step_device_ms']:.3f} "
          f"device), scalar median {widest} {out['push_scalar_wall_ms']:.3f} ms (step {out['push_scalar_step_device_ms']:.3f}), ratio "
          f"{out['push_classwise_over_scalar']:.3f}", flush=True)
    print(json.dumps(out))
    if not (agree and agree_eq):
        sys.exit("the class-wise events differ from the scalar decodes'")
    if out["cw_wall_ms"] > out["loop_wall_ms"]:                                # the requirement: it replaces the loop, so it is no slower
        sys.exit(f"the class-wise decode ({out['cw_wall_ms']:.3f} ms) is slower than the loop of {K} scalar decodes "
                 f"({out['loop_wall_ms']:.3f} ms)")


if __name__ == "__main__":
    main()
