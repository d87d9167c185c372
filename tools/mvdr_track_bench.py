#!/usr/bin/env python3
"""Per-event audio by an MVDR beam steered along the event's direction track (csrc/mvdr.hip sed_event_mvdr_track).
tools/doa_track_bench.py's workload: --seconds (one hour) of 48 kHz 4-channel int16, device-resident, resampled once; --events
(1 000) events located once with feature.event_doa and track=DirectionTrack(--block-chunks 1, --max-step-deg 15) outside the
timing, an 18 cm tetrahedron, a sphere of 2 562 directions; MVDR(--loading 1e-2).  For noise_blocks = 0 and --noise-blocks (8):
  tracked      feature.event_mvdr with follow_track=True: the span launch, one 8-byte read, the covariance launches, the tracked
               weight and apply kernels per slice
  untracked    the same call without follow_track on the same build: what the extra solves and weight rows cost
and for noise_blocks = 0:
  torch        the only other device route to the same numbers: per event torch.stft of the zero-padded segment, the einsum
               covariance, ONE float64 torch.linalg.solve per track block, the combine with per-frame weights and torch.istft
The buffers of the tracked call and the torch route are compared (max abs difference).  Medians over --reps repetitions after a
warm-up, the alternatives alternating in one process, with the smallest and the largest time of each.  One JSON line at the end.
Exits non-zero when the kernel route is the slower one.
python tools/mvdr_track_bench.py [--seconds 3600] [--events 1000] [--noise-blocks 8] [--block-chunks 1] [--max-step-deg 15]"""
import argparse
import json
import os
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
from tools.tdoa_bench import C, TF, event_table, wall

N, B = 2048, 1024


def timed(fns, reps):
    """alternate the callables ``reps`` times after a warm-up -> [(median, smallest, largest)] of their wall times in ms"""
    for fn in fns:
        fn()
    ts = [[] for _ in fns]
    for _ in range(reps):
        for t, fn in zip(ts, fns):
            t.append(wall(fn)[0])
    return [(float(np.median(t)), float(min(t)), float(max(t))) for t in ts]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=int, default=3600)
    ap.add_argument("--events", type=int, default=1000)
    ap.add_argument("--loading", type=float, default=1e-2)
    ap.add_argument("--noise-blocks", type=int, default=8)
    ap.add_argument("--noise-guard", type=int, default=1)
    ap.add_argument("--max-frames", type=int, default=256)
    ap.add_argument("--block-chunks", type=int, default=1)
    ap.add_argument("--max-step-deg", type=float, default=15.0)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mvdr_track_bench needs the GPU: nothing is measured without one")
    Kn, G, W = a.noise_blocks, a.noise_guard, a.block_chunks
    gen = torch.Generator(device="cuda").manual_seed(0)
    rng = np.random.default_rng(0)
    x = torch.randint(-8000, 8000, (48000 * a.seconds, C), device="cuda", generator=gen, dtype=torch.int16)
    pcm, clips = resample_many([x], 48000, feature.SR, C, "cuda", keep_channels=True)
    del x
    n = clips[0][1]
    E = a.events
    rows = event_table(E, 1 + n // feature.HOP, rng)
    ev = {k: torch.from_numpy(np.ascontiguousarray(rows[:, i])).cuda() for i, k in enumerate(("onset", "offset", "peak_frame"))}
    doa = sed.DOA(tetrahedron(EDGE), sed.DirectionGrid.sphere(2562), max_frames=a.max_frames, track=sed.DirectionTrack(W, a.max_step_deg))
    D = len(doa.grid)
    with torch.no_grad():
        ev.update(feature.event_doa(pcm, clips, C, ev, TF, doa))
        dirs, loc = ev["dir"].cpu().numpy(), ev["loc_frames"].cpu().numpy()
        tlen, tdir = ev["trk_len"].cpu().numpy(), ev["trk_dir"].cpu().numpy()
        spans = [sed.event_samples(*r, TF, n, feature.HOP, a.max_frames, int(d), int(lf)) for r, d, lf in zip(rows.tolist(), dirs, loc)]
        lens = np.array([s1 - s0 for s0, s1 in spans], np.int64)
        starts = np.concatenate([[0], np.cumsum(lens)[:-1]])
        total = int(lens.sum())
        win = torch.from_numpy(mvdr_window().copy()).cuda()
        k = torch.arange(B + 1, device="cuda", dtype=torch.float64)[:, None]
        tau = torch.from_numpy(doa.steering(feature.SR)).cuda()
        eye = torch.eye(C, device="cuda", dtype=torch.complex128)
        chans = [pcm[o:o + m] for o, m in clips]
        plan = []
        for e in range(E):
            if lens[e] > 0:
                T = int(min(max(tlen[e], 0), tdir.shape[1]))
                per_block = [int(t) if 0 <= t < D else int(dirs[e]) for t in tdir[e, :T]] or [int(dirs[e])]
                frame_block = torch.from_numpy(sed.mvdr_frame_blocks(int(lens[e]), feature.HOP, W, T)).cuda()
                plan.append((int(starts[e]), spans[e][0], int(lens[e]), per_block, frame_block))
        calls = {(follow, kn): sed.MVDR(a.loading, noise_blocks=kn, noise_guard=G, follow_track=follow) for follow in (True, False) for kn in (0, Kn)}

        def run(follow, kn):
            return lambda: feature.event_mvdr(pcm, clips, C, ev, TF, doa, calls[follow, kn])

        def torch_route():
            out = torch.empty(total, device="cuda")
            for start, s0, ln, per_block, frame_block in plan:
                J = -(-ln // B)
                seg = torch.nn.functional.pad(torch.stack([ch[s0:s0 + ln] for ch in chans]), (0, J * B - ln))
                X = torch.stft(seg, N, B, window=win, center=True, pad_mode="constant", return_complex=True)      # [C, 1025, J + 1]
                R = torch.einsum("ckj,dkj->kcd", X, X.conj())
                trace = torch.einsum("kcc->k", R).real
                ok = trace > 0
                A = torch.where(ok[:, None, None], R.to(torch.complex128) + (a.loading / C) * trace.double()[:, None, None] * eye, eye)
                ws = []
                for d in per_block:                                                                               # a solve per block
                    dv = torch.exp(2j * torch.pi * k * tau[d][None, :] / N)                                        # [1025, C]
                    v = torch.linalg.solve(A, dv[:, :, None])[:, :, 0]
                    ws.append(torch.where(ok[:, None], v / (dv.conj() * v).sum(1, keepdim=True), dv / C).to(torch.complex64))
                w = torch.stack(ws)[frame_block]                                                                  # [J + 1, 1025, C]
                Y = torch.einsum("jkc,ckj->kj", w.conj(), X)
                out[start:start + ln] = torch.istft(Y, N, B, window=win, center=True, length=J * B)[:ln]
            return out

        got = run(True, 0)()
        assert np.array_equal(got["audio_len"].cpu().numpy(), lens) and np.array_equal(got["audio_start"].cpu().numpy(), starts)
        diff = float((got["audio"] - torch_route()).abs().max())
        scale = float(got["audio"].abs().max())
        still = float((got["audio"] - run(False, 0)()["audio"]).abs().max())
        del got
        (t_trk, t_own, t_trk_n, t_own_n, t_torch) = timed([run(True, 0), run(False, 0), run(True, Kn), run(False, Kn), torch_route], a.reps)
    blocks = int(sum(len(p[3]) for p in plan))
    fmt = lambda t: {"median": round(t[0], 4), "min": round(t[1], 4), "max": round(t[2], 4)}       # noqa: E731
    out = {"tool": "mvdr_track_bench", "seconds": a.seconds, "channels": C, "time_factor": TF, "events": E, "extracted_events": len(plan),
           "blocks": blocks, "block_chunks": W, "max_step_deg": a.max_step_deg, "directions": D, "loading": a.loading, "noise_blocks": Kn,
           "noise_guard": G, "max_frames": a.max_frames, "samples": total, "tracked_own_ms": fmt(t_trk), "untracked_own_ms": fmt(t_own),
           "tracked_noise_ms": fmt(t_trk_n), "untracked_noise_ms": fmt(t_own_n), "torch_ms": fmt(t_torch), "max_abs_diff": diff,
           "max_abs_audio": scale, "max_abs_change_by_the_track": still}
    print(f"{E} events ({len(plan)} extracted, {blocks} track blocks, {total} samples = {total / feature.SR:.1f} s): own frames, tracked "
          f"{t_trk[0]:.3f} ms [{t_trk[1]:.3f}, {t_trk[2]:.3f}] against {t_own[0]:.3f} ms [{t_own[1]:.3f}, {t_own[2]:.3f}] untracked; Kn = {Kn}, "
          f"tracked {t_trk_n[0]:.3f} ms [{t_trk_n[1]:.3f}, {t_trk_n[2]:.3f}] against {t_own_n[0]:.3f} ms [{t_own_n[1]:.3f}, {t_own_n[2]:.3f}]; "
          f"torch route {t_torch[0]:.3f} ms [{t_torch[1]:.3f}, {t_torch[2]:.3f}] ({t_torch[0] / t_trk[0]:.1f}x); the buffers differ by at most "
          f"{diff:.2e} (largest sample {scale:.3g}; the track changes a sample by up to {still:.3g})", flush=True)
    print(json.dumps(out))
    if t_trk[0] > t_torch[0]:
        raise SystemExit(f"event_mvdr {t_trk[0]:.3f} ms is slower than the torch route {t_torch[0]:.3f} ms")


if __name__ == "__main__":
    main()
