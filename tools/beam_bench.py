#!/usr/bin/env python3
"""Per-event audio by a steered delay-and-sum beam (csrc/beam.hip sed_event_beamform).  --seconds (one hour) of 48 kHz
4-channel int16, device-resident, resampled once to the detector's rate; a synthetic table of --events (1 000) events of 5 to 200
output frames (time factor 8), located once with feature.event_doa (a tetrahedron of 18 cm, a sphere of 2 562 directions) outside
the timing; DelaySum(--oversample 16, --half-width 16).  Two ways to the same samples:
  event_beamform  feature.event_beamform(pcm, clips, 4, events, 8, doa, beam): two launches and one 8-byte read
  torch           the only other device route: per event, a gather of the C channel slices shifted by the whole samples of their
                  delays, torch.nn.functional.conv1d with the C tap rows of their fractions (groups = C), the sum over the channels
                  times 1/C, written to the event's place in the packed buffer (spans, directions, delays and the zero-padded
                  channels are made outside the timing)
The two buffers are compared (max abs difference).  Every figure is a median over --reps repetitions after a warm-up; the
alternatives alternate in one process.  One JSON line at the end.  Exits non-zero when event_beamform is the slower one.
python tools/beam_bench.py [--seconds 3600] [--events 1000] [--oversample 16] [--half-width 16] [--max-frames 256] [--reps 10]"""
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
from tools.tdoa_bench import C, TF, event_table, med


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=int, default=3600)
    ap.add_argument("--events", type=int, default=1000)
    ap.add_argument("--oversample", type=int, default=16)
    ap.add_argument("--half-width", type=int, default=16)
    ap.add_argument("--max-frames", type=int, default=256)
    ap.add_argument("--reps", type=int, default=10)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("beam_bench needs the GPU: nothing is measured without one")
    gen = torch.Generator(device="cuda").manual_seed(0)
    rng = np.random.default_rng(0)
    x = torch.randint(-8000, 8000, (48000 * a.seconds, C), device="cuda", generator=gen, dtype=torch.int16)
    pcm, clips = resample_many([x], 48000, feature.SR, C, "cuda", keep_channels=True)
    del x
    n = clips[0][1]
    n_feat = 1 + n // feature.HOP
    E, Q, H = a.events, a.oversample, a.half_width
    rows = event_table(E, n_feat, rng)
    ev = {k: torch.from_numpy(np.ascontiguousarray(rows[:, i])).cuda() for i, k in enumerate(("onset", "offset", "peak_frame"))}
    doa = sed.DOA(tetrahedron(EDGE), sed.DirectionGrid.sphere(2562), max_frames=a.max_frames)
    beam = sed.DelaySum(Q, H)
    with torch.no_grad():
        ev.update(feature.event_doa(pcm, clips, C, ev, TF, doa))
        dirs, loc = ev["dir"].cpu().numpy(), ev["loc_frames"].cpu().numpy()
        spans = [sed.event_samples(*r, TF, n, feature.HOP, a.max_frames, int(d), int(lf)) for r, d, lf in zip(rows.tolist(), dirs, loc)]
        lens = np.array([s1 - s0 for s0, s1 in spans], np.int64)
        starts = np.concatenate([[0], np.cumsum(lens)[:-1]])
        M = doa.delays(feature.SR, Q).astype(np.int64)
        taps = torch.from_numpy(beam.taps.copy()).cuda()
        reach = H + int(np.abs(M).max()) // Q + 2
        padded = [torch.nn.functional.pad(pcm[o:o + m], (reach, reach)) for o, m in clips]       # samples outside the recording read as 0
        plan = []                                                                                  # per event: (start, s0, len, whole delays, tap rows)
        for e in range(E):
            if lens[e] > 0:
                q = -M[dirs[e]]
                ic = q // Q
                plan.append((int(starts[e]), spans[e][0], int(lens[e]), ic.tolist(), taps[torch.from_numpy(q - Q * ic).cuda()].unsqueeze(1).contiguous()))
        total = int(lens.sum())

        def new():
            return feature.event_beamform(pcm, clips, C, ev, TF, doa, beam)

        def torch_route():
            out = torch.empty(total, device="cuda")
            for start, s0, ln, ic, w in plan:
                seg = torch.stack([padded[c][reach + s0 + ic[c] - H + 1: reach + s0 + ic[c] + H + ln] for c in range(C)])
                y = torch.nn.functional.conv1d(seg.unsqueeze(0), w, groups=C)[0]                 # [C, ln]: a_c
                out[start:start + ln] = y.sum(0) * (1.0 / C)
            return out

        got = new()
        assert np.array_equal(got["audio_len"].cpu().numpy(), lens) and np.array_equal(got["audio_start"].cpu().numpy(), starts)
        diff = float((got["audio"] - torch_route()).abs().max())
        scale = float(got["audio"].abs().max())
        del got
        t_new, t_torch = med([new, torch_route], a.reps)
    out = {"tool": "beam_bench", "seconds": a.seconds, "channels": C, "time_factor": TF, "events": E, "extracted_events": len(plan),
           "oversample": Q, "half_width": H, "max_frames": a.max_frames, "samples": total, "event_beamform_ms": round(t_new, 4),
           "torch_ms": round(t_torch, 4), "max_abs_diff": diff, "max_abs_audio": scale}
    print(f"{E} events ({len(plan)} extracted, {total} samples = {total / feature.SR:.1f} s), Q = {Q}, H = {H}: event_beamform {t_new:.3f} ms "
          f"({total * (C + 1) * 4 / t_new / 1e6:.1f} GB/s of samples read and written), torch route {t_torch:.3f} ms "
          f"({t_torch / t_new:.1f}x); the buffers differ by at most {diff:.2e} (largest sample {scale:.3g})", flush=True)
    print(json.dumps(out))
    if t_new > t_torch:
        raise SystemExit(f"event_beamform {t_new:.3f} ms is slower than the torch route {t_torch:.3f} ms")


if __name__ == "__main__":
    main()
