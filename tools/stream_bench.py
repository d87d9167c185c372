#!/usr/bin/env python3
"""Live streams: the cost of one steady-state push (``StreamDetector.push``) for S synthetic feeds, next to what a user had
before.  Every push hands each feed one window hop of audio (32 feature frames = 32 768 samples = 0.74 s), resident on the
device, so each feed completes exactly one window per push.  Both reference nets, fp32 plan.  Per S in {1, 64, 1024}:
  push        host wall clock of one push (it ends in its one blocking read), median over --pushes pushes after a warm-up,
              and the device time of its phases (hip events: log-mel, gather, forward, step);
  forward     ``det.window_logits`` alone on the same S windows: the irreducible forward (wall, then synchronise);
  trailing    ``det.detect_many`` on S trailing buffers of seq_len + hop frames: how live audio had to be approximated.
The three alternate in one process.  One JSON line at the end.
python tools/stream_bench.py [--streams 1 64 1024] [--pushes 40] [--reps 7]"""
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

PHASES = ("logmel", "gather", "forward", "step")


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, nargs="+", default=[1, 64, 1024])
    ap.add_argument("--pushes", type=int, default=40)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--hop", type=int, default=32)
    a = ap.parse_args()
    torch.manual_seed(0)
    gen = torch.Generator(device="cuda").manual_seed(0)
    hop_samples = a.hop * feature.HOP
    out = {"tool": "stream_bench", "hop": a.hop, "push_seconds": round(hop_samples / feature.SR, 4), "nets": {}}
    for name, m in (("lightning", sed.LightningTimePooledCRNN()), ("timepooled128", sed.TimePooledCRNN(conv_channels=128))):
        m = m.cuda().eval()
        out["nets"][name] = {}
        for S in a.streams:
            # two pushes' worth of audio per feed: noise with a tone that comes and goes
            pcm = 0.05 * torch.randn(2, S, hop_samples, device="cuda", generator=gen)
            t = torch.arange(hop_samples, device="cuda") / feature.SR
            pcm[1] += torch.sin(2 * np.pi * 2000 * t)
            mean, std = data.standard_scaler_fit(feature.mbe(pcm[:, 0].reshape(-1)))
            det = sed.EventDetector(m, hop=a.hop, median=3, mean=mean, std=std)
            st = det.stream(n_streams=S)
            pieces = [[pcm[i, s] for s in range(S)] for i in range(2)]
            # what a user had: the forward of the same S windows, and detect_many on S trailing buffers
            mel = torch.randn(a.hop * (S - 1) + det.seq_len, m.n_mels, device="cuda", generator=gen)
            plan = sed.plan_windows(mel.shape[0], m.time_factor, det.seq_len, a.hop)
            assert plan.n_win == S
            trailing = [torch.cat([pcm[i % 2, s] for i in range(det.seq_len // a.hop + 1)]) for s in range(S)]
            with torch.no_grad():
                for i in range(6):                                  # warm-up: tables, workspaces, every feed past its first window
                    st.push(pieces[i % 2])
                det.window_logits(mel, plan)
                det.detect_many(trailing)
                walls, fwd, trail, phases, events = [], [], [], [], 0
                for rep in range(a.reps):                           # alternate the three
                    for i in range(a.pushes):
                        st.marks = []
                        ms, res = wall(lambda: st.push(pieces[i % 2]))
                        walls.append(ms)
                        events += len(res)
                        phases.append([sum(x.elapsed_time(y) for n, x, y in st.marks if n == p) for p in PHASES])
                        st.marks = None
                    fwd.append(wall(lambda: det.window_logits(mel, plan))[0])
                    trail.append(wall(lambda: det.detect_many(trailing))[0])
            med = [float(np.median([p[i] for p in phases])) for i in range(len(PHASES))]
            w, f, tr = float(np.median(walls)), float(np.median(fwd)), float(np.median(trail))
            out["nets"][name][str(S)] = {"push_ms": round(w, 4), "push_p90_ms": round(float(np.percentile(walls, 90)), 4),
                                         "phase_ms": {p: round(v, 4) for p, v in zip(PHASES, med)},
                                         "forward_alone_ms": round(f, 4), "push_over_forward": round(w / f, 3),
                                         "detect_many_trailing_ms": round(tr, 4), "events": events,
                                         "state_bytes_per_stream": st.state_bytes // S}
            print(f"{name} S={S}: push {w:.3f} ms (p90 {np.percentile(walls, 90):.3f}); device phases " +
                  ", ".join(f"{p} {v:.3f}" for p, v in zip(PHASES, med)) + f" ms; forward alone {f:.3f} ms (push / forward "
                  f"{w / f:.2f}); detect_many on trailing buffers {tr:.3f} ms; {st.state_bytes // S} state bytes per feed", flush=True)
            del st, pcm, pieces, trailing, mel
    print(json.dumps(out))


if __name__ == "__main__":
    main()
