#!/usr/bin/env python3
"""GCC-PHAT spatial features (csrc/gcc.hip sed_logmel_gcc).  --seconds (one hour) of 48 kHz 4-channel int16,
device-resident, three ways:
  spatial      feature.mbe(..., channels=4, keep_channels=True, spatial="gcc_phat") -> scaled features [N, (4+6)*40]
  mel_only     the same call without ``spatial`` -> [N, 4*40]: what the six GCC images cost on top of the mel images
  composition  what the spatial call replaces: the mel-only call, then on the resampled planar PCM torch.stft, the complex
               products and the whitening of every pair, torch.fft.irfft, the 40 lags around 0, the scaler, torch.cat
               (skipped with a message if torch.fft does not run on the device).  Its GCC columns are compared with the new
               path's first (max and mean abs difference; they are two float32 evaluations of one definition, and the
               resampler's stop band leaves a few bins below the Nyquist frequency with nothing but rounding noise, whose
               PHAT phase is arbitrary in both: one such bin moves a lag by up to 2/2048).
Every figure is a median over --reps repetitions after a warm-up; the alternatives alternate in one process.  One JSON line at
the end.  Exits non-zero when the new path is slower than the composition it replaces.
python tools/spatial_bench.py [--seconds 3600] [--reps 10]"""
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

C, F = 4, feature.NB_MEL
PAIRS = [(i, j) for i in range(C) for j in range(i + 1, C)]
W = feature.spatial_channels(C) * F


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
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("spatial_bench needs the GPU: nothing is measured without one")
    gen = torch.Generator(device="cuda").manual_seed(0)
    n_in = 48000 * a.seconds
    x = torch.randint(-8000, 8000, (n_in, C), device="cuda", generator=gen, dtype=torch.int16)
    mean = torch.cat([torch.randn(C * F, device="cuda", generator=gen, dtype=torch.float64) - 8.0,
                      0.02 * torch.randn(len(PAIRS) * F, device="cuda", generator=gen, dtype=torch.float64)])
    std = torch.cat([torch.rand(C * F, device="cuda", generator=gen, dtype=torch.float64) + 0.5,
                     0.04 * torch.rand(len(PAIRS) * F, device="cuda", generator=gen, dtype=torch.float64) + 0.03])
    win = torch.from_numpy(feature.hann_periodic()).cuda()
    mu32, is32 = feature._scaler(mean, std, x.device)

    def spatial():
        return feature.mbe(x, input_sr=48000, channels=C, keep_channels=True, spatial="gcc_phat", mean=mean, std=std)

    def mel_only():
        return feature.mbe(x, input_sr=48000, channels=C, keep_channels=True, mean=mean[:C * F], std=std[:C * F])

    def composition():
        cols = [mel_only()]
        pcm = sed.resample(x, 48000, channels=C, keep_channels=True)                  # [C, n] planar float32
        S = torch.stft(pcm, feature.NFFT, feature.HOP, window=win, center=True, pad_mode="constant", return_complex=True)
        for p, (i, j) in enumerate(PAIRS):
            G = S[i] * torch.conj(S[j])                                               # [1025, frames]
            m2 = G.real ** 2 + G.imag ** 2
            Pk = torch.where(m2 >= 1e-30, G * torch.rsqrt(m2.clamp_min(1e-30)), torch.zeros_like(G))
            cc = torch.fft.irfft(Pk, n=feature.NFFT, dim=0)                           # [2048, frames], cc[tau] at tau mod 2048
            cc = torch.cat([cc[feature.NFFT - F // 2:], cc[:F // 2]]).t()
            sl = slice((C + p) * F, (C + p + 1) * F)
            cols.append((cc - mu32[sl]) * is32[sl])
        return torch.cat(cols, 1)

    out = {"tool": "spatial_bench", "seconds": a.seconds, "channels": C, "pairs": len(PAIRS), "n_lags": F}
    with torch.no_grad():
        got = spatial()
        rows = got.shape[0]
        assert got.shape == (rows, W)
        try:
            ref = composition()
            have_fft = True
        except RuntimeError as e:                                                     # no FFT library for this device, and only that:
            msg = str(e).lower()                                                      # running out of memory or a bug must not pass as it
            if "out of memory" in msg or not any(w in msg for w in ("fft", "stft")):
                raise
            have_fft, ref = False, None
            print(f"torch.fft / torch.stft do not run on this device ({str(e).splitlines()[0]}): the composition is skipped", flush=True)
        fns = [spatial, mel_only] + ([composition] if have_fft else [])
        if have_fft:
            same_mel = torch.equal(got[:, :C * F], ref[:, :C * F])
            d = ((got[:, C * F:] - ref[:, C * F:]) / is32[C * F:]).abs()
            out.update(mel_columns_bitwise_equal=bool(same_mel), gcc_max_abs_diff=float(d.max()), gcc_mean_abs_diff=float(d.mean()))
            del d
            del ref
        del got
        ts = med(fns, a.reps)
    t_sp, t_mel = ts[0], ts[1]
    need = n_in * C * 2 + rows * W * 4                                                # the frames once + the features
    out.update(rows=rows, spatial_ms=round(t_sp, 4), mel_only_ms=round(t_mel, 4), algorithmic_GBps=round(need / t_sp / 1e6, 1))
    print(f"{a.seconds} s of 48 kHz {C}-channel int16 -> features [{rows}, {W}]: spatial front end {t_sp:.3f} ms, mel-only "
          f"multichannel front end {t_mel:.3f} ms ({t_sp / t_mel:.2f}x)", flush=True)
    if have_fft:
        out["composition_ms"] = round(ts[2], 4)
        print(f"torch.stft + complex ops + torch.fft.irfft composition {ts[2]:.3f} ms ({ts[2] / t_sp:.2f}x the new path); GCC columns "
              f"differ by at most {out['gcc_max_abs_diff']:.2e} (mean {out['gcc_mean_abs_diff']:.2e}), mel columns bit for bit equal: {out['mel_columns_bitwise_equal']}", flush=True)
    print(json.dumps(out))
    if have_fft and t_sp > ts[2]:
        raise SystemExit(f"the new path ({t_sp:.3f} ms) is slower than the composition it replaces ({ts[2]:.3f} ms)")


if __name__ == "__main__":
    main()
