#!/usr/bin/env python3
"""Per-event audio by an MVDR beam whose covariance comes from before the onset (csrc/mvdr.hip sed_event_mvdr_noise).
tools/mvdr_bench.py's workload: --seconds (one hour) of 48 kHz 4-channel int16, device-resident, resampled once; --events (1 000)
events located once with feature.event_doa outside the timing; MVDR(--loading 1e-2, noise_blocks=--noise-blocks 8, noise_guard=1).
Three figures:
  event_mvdr (Kn)   feature.event_mvdr with the noise settings: the span launch, one 8-byte read, four launches per slice
  event_mvdr (0)    the same call with noise_blocks = 0 on the same build: for scale only, it computes something else
  torch             the only other device route to the same numbers: per event torch.stft of the pre-onset stretch (no padding:
                    exactly Kn frames) and of the zero-padded segment, the einsum covariance of the former — of the latter for
                    an event that falls back — torch.linalg.solve in float64, the combine and torch.istft
The buffers of the first and the last are compared (max abs difference).  Medians over --reps repetitions after a warm-up, the
alternatives alternating in one process.  One JSON line at the end.  Exits non-zero when the kernel route is the slower one.

--parent DIR (a checkout of the parent commit with its library built): also runs DIR/tools/mvdr_bench.py and this tree's
tools/mvdr_bench.py --rounds times each, alternating processes, to show what noise_blocks = 0 costs against the parent: the
medians of event_mvdr_ms and each side's own spread (max - min), to be judged against the run-to-run spread of one build
(0.18 ms), not a percentage.  (A whole checkout and not SED_CRNN_LIB alone: this package binds the new entries at
load time, which the parent's library does not export.)
python tools/mvdr_noise_bench.py [--seconds 3600] [--events 1000] [--noise-blocks 8] [--noise-guard 1] [--parent DIR] [--rounds 3]"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

import sed_crnn_amd as sed
from sed_crnn_amd import feature
from sed_crnn_amd.localize import mvdr_window
from sed_crnn_amd.resample import resample_many
from tools.doa_bench import EDGE, tetrahedron
from tools.tdoa_bench import C, TF, event_table, med

N, B = 2048, 1024


def against_parent(parent, rounds, passthrough):
    """-> {"this": [event_mvdr_ms, ...], "parent": [...]}: tools/mvdr_bench.py of both trees, one process each, alternating"""
    got = {"this": [], "parent": []}
    for _ in range(rounds):
        for name, tree in (("parent", parent), ("this", ROOT)):
            env = {k: v for k, v in os.environ.items() if k != "SED_CRNN_LIB"}
            p = subprocess.run([sys.executable, os.path.join(tree, "tools", "mvdr_bench.py")] + passthrough, cwd=tree, env=env,
                               capture_output=True, text=True)
            if p.returncode != 0:
                raise SystemExit(f"{tree}/tools/mvdr_bench.py failed:\n{p.stdout[-2000:]}\n{p.stderr[-2000:]}")
            got[name].append(json.loads(p.stdout.strip().splitlines()[-1])["event_mvdr_ms"])
    return got


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=int, default=3600)
    ap.add_argument("--events", type=int, default=1000)
    ap.add_argument("--loading", type=float, default=1e-2)
    ap.add_argument("--noise-blocks", type=int, default=8)
    ap.add_argument("--noise-guard", type=int, default=1)
    ap.add_argument("--max-frames", type=int, default=256)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--parent", default=None)
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mvdr_noise_bench needs the GPU: nothing is measured without one")
    Kn, G = a.noise_blocks, a.noise_guard
    need = (G + Kn + 1) * B
    gen = torch.Generator(device="cuda").manual_seed(0)
    rng = np.random.default_rng(0)
    x = torch.randint(-8000, 8000, (48000 * a.seconds, C), device="cuda", generator=gen, dtype=torch.int16)
    pcm, clips = resample_many([x], 48000, feature.SR, C, "cuda", keep_channels=True)
    del x
    n = clips[0][1]
    E = a.events
    rows = event_table(E, 1 + n // feature.HOP, rng)
    ev = {k: torch.from_numpy(np.ascontiguousarray(rows[:, i])).cuda() for i, k in enumerate(("onset", "offset", "peak_frame"))}
    doa = sed.DOA(tetrahedron(EDGE), sed.DirectionGrid.sphere(2562), max_frames=a.max_frames)
    noise, own = sed.MVDR(a.loading, noise_blocks=Kn, noise_guard=G), sed.MVDR(a.loading)
    with torch.no_grad():
        ev.update(feature.event_doa(pcm, clips, C, ev, TF, doa))
        dirs, loc = ev["dir"].cpu().numpy(), ev["loc_frames"].cpu().numpy()
        spans = [sed.event_samples(*r, TF, n, feature.HOP, a.max_frames, int(d), int(lf)) for r, d, lf in zip(rows.tolist(), dirs, loc)]
        lens = np.array([s1 - s0 for s0, s1 in spans], np.int64)
        starts = np.concatenate([[0], np.cumsum(lens)[:-1]])
        total = int(lens.sum())
        win = torch.from_numpy(mvdr_window().copy()).cuda()
        k = torch.arange(B + 1, device="cuda", dtype=torch.float64)[:, None]
        tau = torch.from_numpy(doa.steering(feature.SR)).cuda()
        eye = torch.eye(C, device="cuda", dtype=torch.complex128)
        chans = [pcm[o:o + m] for o, m in clips]
        plan = [(int(starts[e]), spans[e][0], int(lens[e]), int(dirs[e])) for e in range(E) if lens[e] > 0]
        uses = np.array([Kn if lens[e] > 0 and spans[e][0] >= need else 0 for e in range(E)], np.int32)

        def new():
            return feature.event_mvdr(pcm, clips, C, ev, TF, doa, noise)

        def scale_only():
            return feature.event_mvdr(pcm, clips, C, ev, TF, doa, own)

        def torch_route():
            out = torch.empty(total, device="cuda")
            for start, s0, ln, d in plan:
                J = -(-ln // B)
                seg = torch.nn.functional.pad(torch.stack([ch[s0:s0 + ln] for ch in chans]), (0, J * B - ln))
                X = torch.stft(seg, N, B, window=win, center=True, pad_mode="constant", return_complex=True)      # [C, 1025, J + 1]
                Xn = X
                if s0 >= need:                                                                                    # [C, 1025, Kn]
                    Xn = torch.stft(torch.stack([ch[s0 - need:s0 - G * B] for ch in chans]), N, B, window=win, center=False, return_complex=True)
                R = torch.einsum("ckj,dkj->kcd", Xn, Xn.conj())
                trace = torch.einsum("kcc->k", R).real
                ok = trace > 0
                dv = torch.exp(2j * torch.pi * k * tau[d][None, :] / N)                                            # [1025, C]
                A = torch.where(ok[:, None, None], R.to(torch.complex128) + (a.loading / C) * trace.double()[:, None, None] * eye, eye)
                v = torch.linalg.solve(A, dv[:, :, None])[:, :, 0]
                w = torch.where(ok[:, None], v / (dv.conj() * v).sum(1, keepdim=True), dv / C).to(torch.complex64)
                Y = torch.einsum("kc,ckj->kj", w.conj(), X)
                out[start:start + ln] = torch.istft(Y, N, B, window=win, center=True, length=J * B)[:ln]
            return out

        got = new()
        assert np.array_equal(got["audio_len"].cpu().numpy(), lens) and np.array_equal(got["audio_start"].cpu().numpy(), starts)
        assert np.array_equal(got["noise_frames"].cpu().numpy(), uses)
        diff = float((got["audio"] - torch_route()).abs().max())
        scale = float(got["audio"].abs().max())
        del got
        t_new, t_own, t_torch = med([new, scale_only, torch_route], a.reps)
    out = {"tool": "mvdr_noise_bench", "seconds": a.seconds, "channels": C, "time_factor": TF, "events": E, "extracted_events": len(plan),
           "noise_events": int((uses > 0).sum()), "loading": a.loading, "noise_blocks": Kn, "noise_guard": G, "max_frames": a.max_frames,
           "samples": total, "event_mvdr_noise_ms": round(t_new, 4), "event_mvdr_own_ms": round(t_own, 4), "torch_ms": round(t_torch, 4),
           "max_abs_diff": diff, "max_abs_audio": scale}
    print(f"{E} events ({len(plan)} extracted, {out['noise_events']} from the noise covariance, {total} samples = {total / feature.SR:.1f} s), "
          f"Kn = {Kn}, G = {G}: event_mvdr {t_new:.3f} ms, with noise_blocks = 0 (another beam, for scale) {t_own:.3f} ms, torch route "
          f"{t_torch:.3f} ms ({t_torch / t_new:.1f}x); the buffers differ by at most {diff:.2e} (largest sample {scale:.3g})", flush=True)
    if a.parent:
        torch.cuda.empty_cache()
        ab = against_parent(os.path.abspath(a.parent), a.rounds, ["--seconds", str(a.seconds), "--events", str(a.events), "--loading",
                                                                   str(a.loading), "--max-frames", str(a.max_frames), "--reps", str(a.reps)])
        for name, v in ab.items():
            out[f"mvdr_bench_{name}_ms"] = v
            print(f"tools/mvdr_bench.py, {name} tree: event_mvdr {v} ms, median {float(np.median(v)):.3f}, spread {max(v) - min(v):.3f}", flush=True)
    print(json.dumps(out))
    if t_new > t_torch:
        raise SystemExit(f"event_mvdr {t_new:.3f} ms is slower than the torch route {t_torch:.3f} ms")


if __name__ == "__main__":
    main()
