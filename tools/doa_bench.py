#!/usr/bin/env python3
"""Per-event direction of arrival (csrc/doa.hip sed_event_doa).  --seconds (one hour) of 48 kHz 4-channel int16,
device-resident, resampled once to the detector's rate; a synthetic table of --events (1 000) events of 5 to 200 output frames
(time factor 8); a tetrahedron of 18 cm (max_lag 24 at 44.1 kHz); a ring of 360 and a sphere of 2 562 directions; oversample 8.
Three ways:
  event_doa    feature.event_doa(pcm, clips, 4, events, 8, doa) -> lag, strength, loc_frames, dir, doa_power
  event_tdoa   feature.event_tdoa with the same max_lag and max_frames: what the steering launch adds is the difference
  torch        the only other device route to these numbers: torch.stft per channel, whitened cross spectra per pair, index_add_
               of every event's rows (the row and event indices are made outside the timing), torch.fft.irfft(S, n = 2048 Q),
               gather at the steering lags and sum over the pairs, arg-max
The steered maps of event_doa and torch are compared (max abs difference per frame) and the directions counted that differ.
Every figure is a median over --reps repetitions after a warm-up; the alternatives alternate in one process.  One JSON line at
the end.  Exits non-zero when event_doa is slower than the torch route for a grid.
python tools/doa_bench.py [--seconds 3600] [--events 1000] [--oversample 8] [--max-frames 256] [--reps 10]"""
import argparse
import json
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import sed_crnn_amd as sed
from sed_crnn_amd import feature
from sed_crnn_amd.resample import resample_many
from tools.tdoa_bench import C, P, TF, event_table, med

EDGE = 0.18                                          # metres: every pair of the tetrahedron


def tetrahedron(edge):
    v = np.array([[1.0, 1.0, 1.0], [1.0, -1.0, -1.0], [-1.0, 1.0, -1.0], [-1.0, -1.0, 1.0]])
    return v * (edge / (2.0 * math.sqrt(2.0)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=int, default=3600)
    ap.add_argument("--events", type=int, default=1000)
    ap.add_argument("--oversample", type=int, default=8)
    ap.add_argument("--max-frames", type=int, default=256)
    ap.add_argument("--reps", type=int, default=10)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("doa_bench needs the GPU: nothing is measured without one")
    gen = torch.Generator(device="cuda").manual_seed(0)
    rng = np.random.default_rng(0)
    x = torch.randint(-8000, 8000, (48000 * a.seconds, C), device="cuda", generator=gen, dtype=torch.int16)
    pcm, clips = resample_many([x], 48000, feature.SR, C, "cuda", keep_channels=True)
    del x
    n_feat = 1 + clips[0][1] // feature.HOP
    E, Q = a.events, a.oversample
    rows = event_table(E, n_feat, rng)
    ev = {k: torch.from_numpy(np.ascontiguousarray(rows[:, i])).cuda() for i, k in enumerate(("onset", "offset", "peak_frame"))}
    rng_f = np.array([sed.event_frames(*r, TF, n_feat, a.max_frames) for r in rows.tolist()], dtype=np.int64)
    nf = rng_f[:, 1] - rng_f[:, 0]
    r_idx = torch.from_numpy(np.concatenate([np.arange(f0, f1) for f0, f1 in rng_f])).cuda()
    who = torch.from_numpy(np.repeat(np.arange(E), nf)).cuda()
    chans = [pcm[o:o + n] for o, n in clips]
    win = torch.hann_window(feature.NFFT, periodic=True, device="cuda")
    pairs = [(i, j) for i in range(C) for j in range(i + 1, C)]
    out = {"tool": "doa_bench", "seconds": a.seconds, "channels": C, "pairs": P, "time_factor": TF, "events": E, "oversample": Q,
           "max_frames": a.max_frames, "feature_frames": n_feat, "located_frames": int(nf.sum()), "grids": {}}
    slower = []
    with torch.no_grad():
        for name, grid in (("ring360", sed.DirectionGrid.ring(360)), ("sphere2562", sed.DirectionGrid.sphere(2562))):
            doa = sed.DOA(tetrahedron(EDGE), grid, max_frames=a.max_frames, oversample=Q)
            ml, J, _ = doa.plan(feature.SR)
            idx = torch.from_numpy(np.mod(J.astype(np.int64), feature.NFFT * Q)).cuda()            # lag j of the inverse transform: j mod 2048 Q

            def new(full=False):
                return feature.event_doa(pcm, clips, C, ev, TF, doa, return_map=full)

            def tdoa():
                return feature.event_tdoa(pcm, clips, C, ev, TF, max_lag=ml, max_frames=a.max_frames)

            def torch_route(full=False):
                spec = [torch.stft(ch, feature.NFFT, hop_length=feature.HOP, window=win, center=True, pad_mode="constant",
                                   return_complex=True).T for ch in chans]                          # [frames, 1025]
                S = torch.zeros(E, P, feature.NFFT // 2 + 1, 2, device="cuda")
                for p, (i, j) in enumerate(pairs):
                    G = spec[i][r_idx] * spec[j][r_idx].conj()                                      # only the rows some event reads
                    m2 = G.real ** 2 + G.imag ** 2
                    Pk = torch.where(m2 >= 1e-30, G * torch.rsqrt(m2.clamp_min(1e-30)), torch.zeros_like(G))
                    S[:, p].index_add_(0, who, torch.view_as_real(Pk))
                S = torch.view_as_complex(S)
                S[..., 0], S[..., -1] = S[..., 0].real + 0j, 0.5 * S[..., -1].real + 0j             # real DC; bin 1024 is interior now: counted twice
                fine = torch.fft.irfft(S, n=feature.NFFT * Q, dim=-1) * Q                           # [E, P, 2048 Q]
                srp = fine[:, 0][:, idx[:, 0]]
                for p in range(1, P):
                    srp = srp + fine[:, p][:, idx[:, p]]
                best, at = srp.max(1)
                return (srp if full else None), at, best / (P * torch.from_numpy(nf).cuda())

            got = new(full=True)
            assert np.array_equal(got["loc_frames"].cpu().numpy(), nf)
            srp_t, at_t, _ = torch_route(full=True)
            per = torch.from_numpy(nf).cuda().view(E, 1).float()
            diff = float(((got["srp"] - srp_t) / per).abs().max())
            other = int((got["dir"].long() != at_t).sum())
            del got, srp_t
            t_new, t_tdoa, t_torch = med([new, tdoa, torch_route], a.reps)
            out["grids"][name] = {"directions": len(grid), "max_lag": ml, "event_doa_ms": round(t_new, 4), "event_tdoa_ms": round(t_tdoa, 4),
                                  "torch_ms": round(t_torch, 4), "srp_max_abs_diff_per_frame": diff, "directions_that_differ": other}
            print(f"{name}: {E} events ({int(nf.sum())} located frames), max_lag {ml}, Q = {Q}: event_doa {t_new:.3f} ms, event_tdoa alone "
                  f"{t_tdoa:.3f} ms (steering adds {t_new - t_tdoa:.3f} ms), torch route {t_torch:.3f} ms ({t_torch / t_new:.2f}x); maps "
                  f"differ by at most {diff:.2e} per frame, {other} directions differ", flush=True)
            if t_new > t_torch:
                slower.append(f"{name}: event_doa {t_new:.3f} ms is slower than the torch route {t_torch:.3f} ms")
    print(json.dumps(out))
    if slower:
        raise SystemExit("; ".join(slower))


if __name__ == "__main__":
    main()
