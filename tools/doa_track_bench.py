#!/usr/bin/env python3
"""Direction tracks (csrc/doatrack.hip sed_event_doa_track) on the workload of tools/doa_bench.py: --seconds (one hour)
of 48 kHz 4-channel int16, device-resident, resampled once to the detector's rate; a synthetic table of --events (1 000) events of
5 to 200 output frames (time factor 8); a tetrahedron of 18 cm (max_lag 24 at 44.1 kHz); a sphere of 2 562 directions;
oversample 8; blocks of --block-chunks (1) chunks of 32 frames; max_step_deg = --max-step-deg (15).  Four ways:
  track        feature.event_doa with sed.DOA(..., track=sed.DirectionTrack(W, step)): dir and the smoothed track in one call
  track_raw    the same without max_step_deg: what the path kernel (and keeping the maps for it) adds is the difference
  event_doa    feature.event_doa without a track: what the tracks cost is the difference
  torch        the only other device route to the same numbers: event_doa for dir, event_doa(return_map=True) on the table of
               sub-events (one per block, at time factor 1: every block's frames are transformed a second time), and the path
               in torch ops over a padded neighbour matrix (the tables and indices are made outside the timing)
The tracks of the first and the last way are compared.  Every figure is a median over --reps repetitions after a warm-up, with
the smallest and the largest beside it; the alternatives alternate in one process.  One JSON line at the end.  Exits non-zero
when the track call is slower than the torch route.
python tools/doa_track_bench.py [--seconds 3600] [--events 1000] [--block-chunks 1] [--max-step-deg 15] [--reps 10]"""
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
from tools.tdoa_bench import C, TF, event_table, wall


def spread(fns, reps):
    """alternate the callables ``reps`` times after a warm-up -> per callable (median, smallest, largest) wall time in ms"""
    for fn in fns:
        fn()
    ts = [[] for _ in fns]
    for _ in range(reps):
        for t, fn in zip(ts, fns):
            t.append(wall(fn)[0])
    return [(float(np.median(t)), float(np.min(t)), float(np.max(t))) for t in ts]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=int, default=3600)
    ap.add_argument("--events", type=int, default=1000)
    ap.add_argument("--oversample", type=int, default=8)
    ap.add_argument("--max-frames", type=int, default=256)
    ap.add_argument("--block-chunks", type=int, default=1)
    ap.add_argument("--max-step-deg", type=float, default=15.0)
    ap.add_argument("--directions", type=int, default=2562)
    ap.add_argument("--reps", type=int, default=10)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("doa_track_bench needs the GPU: nothing is measured without one")
    gen = torch.Generator(device="cuda").manual_seed(0)
    rng = np.random.default_rng(0)
    x = torch.randint(-8000, 8000, (48000 * a.seconds, C), device="cuda", generator=gen, dtype=torch.int16)
    pcm, clips = resample_many([x], 48000, feature.SR, C, "cuda", keep_channels=True)
    del x
    n_feat = 1 + clips[0][1] // feature.HOP
    E, Q, W, MF = a.events, a.oversample, a.block_chunks, a.max_frames
    rows = event_table(E, n_feat, rng)
    ev = {k: torch.from_numpy(np.ascontiguousarray(rows[:, i])).cuda() for i, k in enumerate(("onset", "offset", "peak_frame"))}
    grid = sed.DirectionGrid.sphere(a.directions)
    D = len(grid)
    pos = tetrahedron(EDGE)
    track = sed.DOA(pos, grid, max_frames=MF, oversample=Q, track=sed.DirectionTrack(W, a.max_step_deg))
    track_raw = sed.DOA(pos, grid, max_frames=MF, oversample=Q, track=sed.DirectionTrack(W))
    plain = sed.DOA(pos, grid, max_frames=MF, oversample=Q)
    wide = sed.DOA(pos, grid, max_frames=48 * W, oversample=Q)                            # (takes a merged last block)
    Tm = track.track.max_blocks(MF)
    # the torch route's tables: the sub-events in feature frames, their slots, the padded neighbour matrix
    sub, slot, T_host = [], [], np.zeros(E, np.int64)
    for e, r in enumerate(rows.tolist()):
        f0, f1 = sed.event_frames(*r, TF, n_feat, MF)
        T, first, n = sed.track_blocks(f1 - f0, W)
        T_host[e] = T
        for b in range(T):
            sub.append((f0 + first[b], f0 + first[b] + n[b], f0 + first[b]))
            slot.append(e * Tm + b)
    sub = np.asarray(sub, np.int32)
    sub_ev = {k: torch.from_numpy(np.ascontiguousarray(sub[:, i])).cuda() for i, k in enumerate(("onset", "offset", "peak_frame"))}
    slot = torch.from_numpy(np.asarray(slot, np.int64)).cuda()
    off, idx = track.neighbours()
    K = int(np.diff(off).max())
    nbr = np.repeat(np.arange(D)[:, None], K, 1)                                          # padded with the row's own direction
    for d in range(D):
        nbr[d, :off[d + 1] - off[d]] = idx[off[d]:off[d + 1]]
    nbr = torch.from_numpy(nbr).cuda()
    T_dev = torch.from_numpy(T_host).cuda().view(E, 1)
    own = torch.arange(D, device="cuda").view(1, D).expand(E, D)

    def new():
        return feature.event_doa(pcm, clips, C, ev, TF, track)

    def new_raw():
        return feature.event_doa(pcm, clips, C, ev, TF, track_raw)

    def doa_alone():
        return feature.event_doa(pcm, clips, C, ev, TF, plain)

    def torch_route():
        one = feature.event_doa(pcm, clips, C, ev, TF, plain)
        blocks = feature.event_doa(pcm, clips, C, sub_ev, 1, wide, return_map=True)
        maps = torch.zeros(E * Tm, D, device="cuda")
        maps[slot] = blocks["srp"]
        maps = maps.view(E, Tm, D)
        raw = torch.full((E * Tm,), -1, dtype=torch.int32, device="cuda")
        raw[slot] = blocks["dir"]
        s, backs = maps[:, 0], []
        for b in range(1, Tm):
            best, arg = s[:, nbr].max(2)                                                  # [E, D, K] -> [E, D]
            live = T_dev > b
            s = torch.where(live, maps[:, b] + best, s)
            backs.append(torch.where(live, nbr[own, arg], own))
        at = s.argmax(1)
        path = [at]
        for bk in reversed(backs):
            at = bk.gather(1, at.view(E, 1)).squeeze(1)
            path.append(at)
        dirs = torch.stack(path[::-1], 1).to(torch.int32)
        return one["dir"], torch.where(raw.view(E, Tm) < 0, torch.full_like(dirs, -1), dirs)

    with torch.no_grad():
        got = new()
        assert np.array_equal(got["trk_len"].cpu().numpy(), T_host)
        d_t, trk_t = torch_route()
        differ = int((got["trk_dir"] != trk_t).sum())
        moved = int((got["trk_dir"] != got["trk_raw"]).sum())
        assert torch.equal(got["dir"], d_t)
        del got, d_t, trk_t
        (t_new, lo_new, hi_new), (t_raw, lo_raw, hi_raw), (t_doa, lo_doa, hi_doa), (t_torch, lo_torch, hi_torch) = \
            spread([new, new_raw, doa_alone, torch_route], a.reps)
    extra = t_new - t_doa
    share = (t_new - t_raw) / extra if extra > 0 else float("nan")
    out = {"tool": "doa_track_bench", "seconds": a.seconds, "channels": C, "time_factor": TF, "events": E, "oversample": Q, "max_frames": MF,
           "block_chunks": W, "max_step_deg": a.max_step_deg, "directions": D, "neighbours_most": K, "blocks": int(T_host.sum()),
           "track_ms": [round(v, 4) for v in (t_new, lo_new, hi_new)], "track_raw_ms": [round(v, 4) for v in (t_raw, lo_raw, hi_raw)],
           "event_doa_ms": [round(v, 4) for v in (t_doa, lo_doa, hi_doa)], "torch_ms": [round(v, 4) for v in (t_torch, lo_torch, hi_torch)],
           "extra_over_event_doa_ms": round(extra, 4), "path_share_of_extra": round(share, 4), "track_cells_that_differ": differ,
           "cells_the_path_moved": moved}
    print(f"{E} events, {int(T_host.sum())} blocks of {32 * W} frames, {D} directions (at most {K} neighbours within {a.max_step_deg:g} deg), "
          f"Q = {Q}: track {t_new:.3f} ms ({lo_new:.3f} .. {hi_new:.3f}), without the path {t_raw:.3f} ms ({lo_raw:.3f} .. {hi_raw:.3f}), "
          f"event_doa alone {t_doa:.3f} ms ({lo_doa:.3f} .. {hi_doa:.3f}): the tracks add {extra:.3f} ms, {100 * share:.0f} % of it the path; "
          f"torch route {t_torch:.3f} ms ({lo_torch:.3f} .. {hi_torch:.3f}), {t_torch / t_new:.2f}x; {differ} track cells differ, the path "
          f"moved {moved} cells", flush=True)
    print(json.dumps(out))
    if t_new > t_torch:
        raise SystemExit(f"the track call {t_new:.3f} ms is slower than the torch route {t_torch:.3f} ms")


if __name__ == "__main__":
    main()
