#!/usr/bin/env python3
"""Per-event audio by an adaptive (MVDR) beam (csrc/mvdr.hip sed_event_mvdr).  --seconds (one hour) of 48 kHz 4-channel
int16, device-resident, resampled once to the detector's rate; a synthetic table of --events (1 000) events of 5 to 200 output
frames (time factor 8), located once with feature.event_doa (a tetrahedron of 18 cm, a sphere of 2 562 directions) outside the
timing; MVDR(--loading 1e-2).  Three figures:
  event_mvdr      feature.event_mvdr(pcm, clips, 4, events, 8, doa, mvdr): the span launch, one 8-byte read, three launches per
                  slice of the event table
  event_beamform  feature.event_beamform with DelaySum(16, 16) on the same events: for scale only, it computes something else
  torch           the only other device route to the same numbers: per event torch.stft of the zero-padded segment (sqrt-Hann
                  window, hop 1024), einsum covariances, torch.linalg.solve in float64, the combine and torch.istft, written to
                  the event's place in the packed buffer (spans, directions, delays and the window are made outside the timing)
The buffers of event_mvdr and the torch route are compared (max abs difference).  Every figure is a median over --reps
repetitions after a warm-up; the alternatives alternate in one process.  One JSON line at the end.  Exits non-zero when
event_mvdr is slower than the torch route.
python tools/mvdr_bench.py [--seconds 3600] [--events 1000] [--loading 1e-2] [--max-frames 256] [--reps 5]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import sed_crnn_amd as sed
from sed_crnn_amd import feature
from sed_crnn_amd.localize import mvdr_window
from sed_crnn_amd.resample import resample_many
from tools.doa_bench import EDGE, tetrahedron
from tools.tdoa_bench import C, TF, event_table, med

N, B = 2048, 1024


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=int, default=3600)
    ap.add_argument("--events", type=int, default=1000)
    ap.add_argument("--loading", type=float, default=1e-2)
    ap.add_argument("--max-frames", type=int, default=256)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mvdr_bench needs the GPU: nothing is measured without one")
    gen = torch.Generator(device="cuda").manual_seed(0)
    rng = np.random.default_rng(0)
    x = torch.randint(-8000, 8000, (48000 * a.seconds, C), device="cuda", generator=gen, dtype=torch.int16)
    pcm, clips = resample_many([x], 48000, feature.SR, C, "cuda", keep_channels=True)
    del x
    n = clips[0][1]
    n_feat = 1 + n // feature.HOP
    E = a.events
    rows = event_table(E, n_feat, rng)
    ev = {k: torch.from_numpy(np.ascontiguousarray(rows[:, i])).cuda() for i, k in enumerate(("onset", "offset", "peak_frame"))}
    doa = sed.DOA(tetrahedron(EDGE), sed.DirectionGrid.sphere(2562), max_frames=a.max_frames)
    mvdr, beam = sed.MVDR(a.loading), sed.DelaySum(16, 16)
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

        def new():
            return feature.event_mvdr(pcm, clips, C, ev, TF, doa, mvdr)

        def fixed():
            return feature.event_beamform(pcm, clips, C, ev, TF, doa, beam)

        def torch_route():
            out = torch.empty(total, device="cuda")
            for start, s0, ln, d in plan:
                J = -(-ln // B)
                seg = torch.nn.functional.pad(torch.stack([ch[s0:s0 + ln] for ch in chans]), (0, J * B - ln))
                X = torch.stft(seg, N, B, window=win, center=True, pad_mode="constant", return_complex=True)      # [C, 1025, J + 1]
                R = torch.einsum("ckj,dkj->kcd", X, X.conj())
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
        diff = float((got["audio"] - torch_route()).abs().max())
        scale = float(got["audio"].abs().max())
        del got
        t_new, t_fixed, t_torch = med([new, fixed, torch_route], a.reps)
    frames = int(sum(-(-ln // B) + 1 for _, _, ln, _ in plan))
    out = {"tool": "mvdr_bench", "seconds": a.seconds, "channels": C, "time_factor": TF, "events": E, "extracted_events": len(plan),
           "loading": a.loading, "max_frames": a.max_frames, "samples": total, "frames": frames, "event_mvdr_ms": round(t_new, 4),
           "event_beamform_ms": round(t_fixed, 4), "torch_ms": round(t_torch, 4), "max_abs_diff": diff, "max_abs_audio": scale}
    print(f"{E} events ({len(plan)} extracted, {frames} frames, {total} samples = {total / feature.SR:.1f} s), loading = {a.loading:g}: "
          f"event_mvdr {t_new:.3f} ms ({t_new * 1e6 / max(frames, 1):.0f} ns per frame), event_beamform (another beam, for scale) {t_fixed:.3f} ms, "
          f"torch route {t_torch:.3f} ms ({t_torch / t_new:.1f}x); the buffers differ by at most {diff:.2e} (largest sample {scale:.3g})", flush=True)
    print(json.dumps(out))
    if t_new > t_torch:
        raise SystemExit(f"event_mvdr {t_new:.3f} ms is slower than the torch route {t_torch:.3f} ms")


if __name__ == "__main__":
    main()
