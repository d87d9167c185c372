#!/usr/bin/env python3
"""Contrast SRP-PHAT (csrc/contrast.hip, sed_event_doa_contrast) on the workload of tools/doa_bench.py: --seconds (one
hour) of 48 kHz 4-channel int16, device-resident, resampled once to the detector's rate; a synthetic table of --events (1 000)
events of 5 to 200 output frames (time factor 8) of --classes (10) classes; a tetrahedron of 18 cm (max_lag 24 at 44.1 kHz); a
sphere of 2 562 directions; oversample 8; sed.Contrast() (32 frames of 256 candidates, guard 2, at least 8).  Three ways:
  contrast     feature.event_doa with sed.DOA(..., contrast=sed.Contrast()): the activity, the selection, the background's chunks
               and the steer launch that subtracts them
  event_doa    feature.event_doa without contrast: what the contrast costs is the difference
  torch        the only other device route to the same numbers: torch.stft per channel, whitened cross spectra per pair,
               index_add_ of every event's rows and of the rows of the same background lists (the lists and indices are made
               outside the timing, from the kernel's own bg_sel), S - w Sb, torch.fft.irfft(S', n = 2048 Q), gather at the steering
               lags and sum over the pairs, arg-max
The maps of the first and the last way are compared (max abs difference per frame) and the directions counted that differ; the
events that found at least min_frames background frames are counted.  Every figure is a median over --reps (5) repetitions after a
warm-up, with the smallest and the largest beside it; the alternatives alternate in one process.  One JSON line at the end.
Exits non-zero when the contrast call is slower than the torch route.
python tools/doa_contrast_bench.py [--seconds 3600] [--events 1000] [--classes 10] [--reps 5]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import sed_crnn_amd as sed
from sed_crnn_amd import feature
from sed_crnn_amd.resample import resample_many
from tools.doa_bench import EDGE, tetrahedron
from tools.doa_track_bench import spread
from tools.tdoa_bench import C, P, TF, event_table


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=int, default=3600)
    ap.add_argument("--events", type=int, default=1000)
    ap.add_argument("--classes", type=int, default=10)
    ap.add_argument("--oversample", type=int, default=8)
    ap.add_argument("--max-frames", type=int, default=256)
    ap.add_argument("--directions", type=int, default=2562)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("doa_contrast_bench needs the GPU: nothing is measured without one")
    gen = torch.Generator(device="cuda").manual_seed(0)
    rng = np.random.default_rng(0)
    x = torch.randint(-8000, 8000, (48000 * a.seconds, C), device="cuda", generator=gen, dtype=torch.int16)
    pcm, clips = resample_many([x], 48000, feature.SR, C, "cuda", keep_channels=True)
    del x
    n_feat = 1 + clips[0][1] // feature.HOP
    E, Q, K = a.events, a.oversample, a.classes
    rows = event_table(E, n_feat, rng)
    ev = {k: torch.from_numpy(np.ascontiguousarray(rows[:, i])).cuda() for i, k in enumerate(("onset", "offset", "peak_frame"))}
    ev["cls"] = torch.from_numpy(rng.integers(0, K, E).astype(np.int32)).cuda()
    ct = sed.Contrast()
    grid = sed.DirectionGrid.sphere(a.directions)
    doa = sed.DOA(tetrahedron(EDGE), grid, max_frames=a.max_frames, oversample=Q, contrast=ct)
    plain = sed.DOA(tetrahedron(EDGE), grid, max_frames=a.max_frames, oversample=Q)
    ml, J, _ = doa.plan(feature.SR)
    idx = torch.from_numpy(np.mod(J.astype(np.int64), feature.NFFT * Q)).cuda()                    # lag j of the inverse transform: j mod 2048 Q
    rng_f = np.array([sed.event_frames(*r, TF, n_feat, a.max_frames) for r in rows.tolist()], dtype=np.int64)
    nf = rng_f[:, 1] - rng_f[:, 0]
    r_idx = torch.from_numpy(np.concatenate([np.arange(f0, f1) for f0, f1 in rng_f])).cuda()
    who = torch.from_numpy(np.repeat(np.arange(E), nf)).cuda()
    chans = [pcm[o:o + n] for o, n in clips]
    win = torch.hann_window(feature.NFFT, periodic=True, device="cuda")
    pairs = [(i, j) for i in range(C) for j in range(i + 1, C)]

    def new(full=False):
        return feature.event_doa(pcm, clips, C, ev, TF, doa, return_map=full, n_classes=K)

    def doa_alone():
        return feature.event_doa(pcm, clips, C, ev, TF, plain)

    with torch.no_grad():
        got = new(full=True)
        assert np.array_equal(got["loc_frames"].cpu().numpy(), nf)
        nb = got["bg_frames"].cpu().numpy().astype(np.int64)
        sel = got["bg_sel"].cpu().numpy()
        # the torch route's lists: the rows of every event's background frames, and w per event
        b_idx = torch.from_numpy(np.concatenate([rows[e, 0] * TF - ct.guard - 1 - sel[e, :nb[e]].astype(np.int64) for e in range(E)] +
                                                [np.zeros(0, np.int64)])).cuda()
        b_who = torch.from_numpy(np.repeat(np.arange(E), nb)).cuda()
        w = torch.from_numpy(np.where(nb > 0, ct.weight * nf / np.maximum(nb, 1), 0.0).astype(np.float32)).cuda().view(E, 1, 1)

        def torch_route(full=False):
            spec = [torch.stft(ch, feature.NFFT, hop_length=feature.HOP, window=win, center=True, pad_mode="constant",
                               return_complex=True).T for ch in chans]                          # [frames, 1025]
            S = torch.zeros(E, P, feature.NFFT // 2 + 1, 2, device="cuda")
            Sb = torch.zeros(E, P, feature.NFFT // 2 + 1, 2, device="cuda")
            for p, (i, j) in enumerate(pairs):
                for acc, rws, ids in ((S, r_idx, who), (Sb, b_idx, b_who)):
                    G = spec[i][rws] * spec[j][rws].conj()                                      # only the rows some event reads
                    m2 = G.real ** 2 + G.imag ** 2
                    Pk = torch.where(m2 >= 1e-30, G * torch.rsqrt(m2.clamp_min(1e-30)), torch.zeros_like(G))
                    acc[:, p].index_add_(0, ids, torch.view_as_real(Pk))
            S = torch.view_as_complex(S) - w * torch.view_as_complex(Sb)
            S[..., 0], S[..., -1] = S[..., 0].real + 0j, 0.5 * S[..., -1].real + 0j             # real DC; bin 1024 is interior now: counted twice
            fine = torch.fft.irfft(S, n=feature.NFFT * Q, dim=-1) * Q                           # [E, P, 2048 Q]
            srp = fine[:, 0][:, idx[:, 0]]
            for p in range(1, P):
                srp = srp + fine[:, p][:, idx[:, p]]
            best, at = srp.max(1)
            return (srp if full else None), at, best / (P * torch.from_numpy(nf).cuda())

        srp_t, at_t, _ = torch_route(full=True)
        per = torch.from_numpy(nf).cuda().view(E, 1).float()
        diff = float(((got["srp"] - srp_t) / per).abs().max())
        other = int((got["dir"].long() != at_t).sum())
        moved = int((got["dir"] != doa_alone()["dir"]).sum())
        del got, srp_t
        (t_new, lo_new, hi_new), (t_doa, lo_doa, hi_doa), (t_torch, lo_torch, hi_torch) = spread([new, doa_alone, torch_route], a.reps)
    found = int((nb >= ct.min_frames).sum())
    out = {"tool": "doa_contrast_bench", "seconds": a.seconds, "channels": C, "pairs": P, "time_factor": TF, "events": E, "classes": K,
           "oversample": Q, "max_frames": a.max_frames, "directions": len(grid), "max_lag": ml, "located_frames": int(nf.sum()),
           "background_frames": int(nb.sum()), "events_with_background": found,
           "contrast_ms": [round(v, 4) for v in (t_new, lo_new, hi_new)], "event_doa_ms": [round(v, 4) for v in (t_doa, lo_doa, hi_doa)],
           "torch_ms": [round(v, 4) for v in (t_torch, lo_torch, hi_torch)], "extra_over_event_doa_ms": round(t_new - t_doa, 4),
           "srp_max_abs_diff_per_frame": diff, "directions_that_differ": other, "directions_the_contrast_moved": moved}
    print(f"{E} events of {K} classes ({int(nf.sum())} located frames, {int(nb.sum())} background frames; {found} events found at least "
          f"{ct.min_frames}), {len(grid)} directions, Q = {Q}: contrast {t_new:.3f} ms ({lo_new:.3f} .. {hi_new:.3f}), event_doa alone {t_doa:.3f} ms "
          f"({lo_doa:.3f} .. {hi_doa:.3f}): the contrast adds {t_new - t_doa:.3f} ms; torch route {t_torch:.3f} ms ({lo_torch:.3f} .. "
          f"{hi_torch:.3f}), {t_torch / t_new:.2f}x; maps differ by at most {diff:.2e} per frame, {other} directions differ; the contrast "
          f"moved {moved} directions", flush=True)
    print(json.dumps(out))
    if t_new > t_torch:
        raise SystemExit(f"the contrast call {t_new:.3f} ms is slower than the torch route {t_torch:.3f} ms")


if __name__ == "__main__":
    main()
