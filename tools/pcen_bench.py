#!/usr/bin/env python3
"""PCEN front end (csrc/pcen.hip sed_pcen).  Three workloads, each with and without ``compress=sed.PCEN()``:
  mono     --seconds (one hour) of 44.1 kHz mono float32, device-resident: feature.mbe(y, mean, std)
  four     the same length of 48 kHz 4-channel int16: feature.mbe(x, input_sr=48000, channels=4, keep_channels=True, mean, std)
  push     --hop (32) frames = 0.74 s of new audio to each of --streams (1024) live feeds: StreamDetector.push
and, for each, the route that the device path replaces: the unscaled log-mel features to the host, scipy.signal.lfilter (with
lfilter_zi, per recording / per feed with its carried filter state) plus numpy for the compression and the scaler, and the result
back to the device.  ``*_pcen_ms`` is what PCEN adds: for mono / four the difference of the two front-end calls, for push the
sed_pcen call on the round's [streams * hop, 40] rows with the state carried (the push itself is reported with and without).
Every figure is a median over --reps repetitions after a warm-up; the alternatives alternate in one process.  One JSON line at the
end.  Exits non-zero when the device path is slower than the host route in any of the three.
python tools/pcen_bench.py [--seconds 3600] [--streams 1024] [--hop 32] [--reps 10]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from scipy import signal

import sed_crnn_amd as sed
from sed_crnn_amd import data, feature

F = feature.NB_MEL


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


def host_pcen(x, p, b, zi=None):
    """[.., T, W] float32 host log-mel -> (PCEN float32, the filter's final state): lfilter along T, numpy for the rest"""
    E = np.float32(p.scale) * np.exp(x)
    if zi is None:
        zi = signal.lfilter_zi([b], [1.0, b - 1.0]).reshape((1,) * (E.ndim - 2) + (1, 1)) * E[..., :1, :]
    M, zf = signal.lfilter([b], [1.0, b - 1.0], E, zi=zi, axis=-2)
    M = M.astype(np.float32)
    return (E * (np.float32(p.eps) + M) ** np.float32(-p.gain) + np.float32(p.bias)) ** np.float32(p.power) - np.float32(p.bias) ** np.float32(p.power), zf


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=int, default=3600)
    ap.add_argument("--streams", type=int, default=1024)
    ap.add_argument("--hop", type=int, default=32)
    ap.add_argument("--reps", type=int, default=10)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("pcen_bench needs the GPU: nothing is measured without one")
    gen = torch.Generator(device="cuda").manual_seed(0)
    p = sed.PCEN()
    b = p.smoothing()
    out = {"tool": "pcen_bench", "seconds": a.seconds, "streams": a.streams, "hop": a.hop}
    slower = []

    def offline(name, x, kw, width):
        mean = torch.randn(width, device="cuda", generator=gen, dtype=torch.float64) * 0.2 + 0.3
        std = torch.rand(width, device="cuda", generator=gen, dtype=torch.float64) * 0.5 + 0.1
        mu32, is32 = (t.cpu().numpy() for t in feature._scaler(mean, std, x.device))

        def log():
            return feature.mbe(x, mean=mean, std=std, **kw)

        def pcen():
            return feature.mbe(x, mean=mean, std=std, compress=p, **kw)

        def host():
            y, _ = host_pcen(feature.mbe(x, **kw).cpu().numpy(), p, b)
            return torch.from_numpy((y - mu32) * is32).cuda()

        with torch.no_grad():
            got = pcen()
            rows, d = got.shape[0], float((got - host()).abs().max())
            del got
            t_log, t_pcen, t_host = med([log, pcen, host], a.reps)
        out[name] = {"rows": rows, "width": width, "log_ms": round(t_log, 4), "pcen_ms": round(t_pcen, 4),
                     "added_ms": round(t_pcen - t_log, 4), "host_route_ms": round(t_host, 4), "max_abs_diff_vs_host": d}
        print(f"{name}: {a.seconds} s -> [{rows}, {width}]: log front end {t_log:.3f} ms, with PCEN {t_pcen:.3f} ms (+{t_pcen - t_log:.3f}); "
              f"host route (log front end, lfilter + numpy, copies) {t_host:.3f} ms; device and host differ by at most {d:.2e}", flush=True)
        if t_pcen > t_host:
            slower.append(f"{name}: {t_pcen:.3f} ms on the device, {t_host:.3f} ms through the host")

    y = 0.1 * torch.randn(44100 * a.seconds, device="cuda", generator=gen)
    offline("mono", y, {}, F)
    del y
    x4 = torch.randint(-8000, 8000, (48000 * a.seconds, 4), device="cuda", generator=gen, dtype=torch.int16)
    offline("four", x4, dict(input_sr=48000, channels=4, keep_channels=True), 4 * F)
    del x4

    # live feeds
    S, hop_samples = a.streams, a.hop * feature.HOP
    m = sed.LightningTimePooledCRNN().cuda().eval()
    pcm = 0.05 * torch.randn(2, S, hop_samples, device="cuda", generator=gen)
    mean, std = data.standard_scaler_fit(feature.mbe(pcm[:, 0].reshape(-1), compress=p))
    pieces = [[pcm[i, s] for s in range(S)] for i in range(2)]
    sts = [sed.EventDetector(m, hop=a.hop, median=3, mean=mean, std=std, compress=c).stream(n_streams=S) for c in (None, p)]
    rows = torch.randn(S * a.hop, F, device="cuda", generator=gen) - 6.0
    state = torch.zeros(S, F, 2, device="cuda")
    frame = [0]
    mu32d, is32d = feature._scaler(mean, std, rows.device)
    mu32, is32 = mu32d.cpu().numpy(), is32d.cpu().numpy()
    zi = [None]

    def kernel():
        work = rows.clone()
        recs = np.stack([np.arange(S) * a.hop, np.full(S, a.hop), np.full(S, frame[0])], 1)
        feature._pcen_launch(work, p, b, recs, 0, F, mu32d, is32d, state)
        frame[0] += a.hop
        return work

    def clone_only():
        return rows.clone()

    def host():
        yy, zi[0] = host_pcen(rows.cpu().numpy().reshape(S, a.hop, F), p, b, zi[0])
        return torch.from_numpy(((yy - mu32) * is32).reshape(S * a.hop, F)).cuda()

    with torch.no_grad():
        for i in range(6):
            for st in sts:
                st.push(pieces[i % 2])
        k = [0]

        def push(st):
            def run():
                k[0] += 1
                return st.push(pieces[k[0] % 2])
            return run
        t_plain, t_comp, t_kernel, t_clone, t_host = med([push(sts[0]), push(sts[1]), kernel, clone_only, host], a.reps * 4)
    out["push"] = {"push_log_ms": round(t_plain, 4), "push_pcen_ms": round(t_comp, 4), "sed_pcen_call_ms": round(t_kernel - t_clone, 4),
                   "host_route_ms": round(t_host, 4), "state_bytes_per_stream": sts[1].state_bytes // S,
                   "state_bytes_per_stream_log": sts[0].state_bytes // S}
    print(f"push: {a.hop} frames to {S} feeds: {t_plain:.3f} ms with the log, {t_comp:.3f} ms with PCEN; sed_pcen on the round's "
          f"[{S * a.hop}, {F}] rows {t_kernel - t_clone:.3f} ms, the host route for them {t_host:.3f} ms", flush=True)
    if t_kernel - t_clone > t_host:
        slower.append(f"push: sed_pcen {t_kernel - t_clone:.3f} ms, {t_host:.3f} ms through the host")
    print(json.dumps(out))
    if slower:
        raise SystemExit("the device path is slower than the route it replaces: " + "; ".join(slower))


if __name__ == "__main__":
    main()
