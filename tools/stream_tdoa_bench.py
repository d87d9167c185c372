#!/usr/bin/env python3
"""Localising live streams (csrc/tdoa.hip sed_stream_ring_write, sed_event_tdoa_ring).  --streams (1 024) four-channel
feeds at the detector's rate, Lightning-size net; every push hands each feed one window hop of audio (32 feature frames =
32 768 samples = 0.74 s), resident on the device.
  (a) push      host wall clock of one steady-state push (it ends in the step's blocking read) of a localising stream
                (``det.stream(S, history_frames=...)``: ring write per round, one event_tdoa_ring call per step that emits) next
                to the same detector without ``localize=``; the two streams take the same pieces and alternate push by push.
                The net is untrained: the threshold sits at the median of its track, so that pushes emit events.
  (b) locate    the ring route, ``feature.event_tdoa_ring`` on the stream's rings, against the only other route to the same
                numbers: linearise the rings with torch (index_select of the feeds that have events, one roll to put the
                oldest sample first), then ``feature.event_tdoa`` on that planar buffer with the event table moved to its
                frames.  Two event tables: two recent events in every feed (every ring is linearised), and one event in each
                of 64 feeds (only those are).  The history is rounded up so that the oldest kept sample starts an output
                frame — otherwise the linear route could not give the same frames at all; both routes must return the same
                bits.
Every figure is a median over --reps repetitions (of --pushes pushes) after a warm-up; the alternatives alternate in one process.
One JSON line at the end.  Exits non-zero when the ring route is the slower one for an event table.
python tools/stream_tdoa_bench.py [--streams 1024] [--pushes 20] [--reps 5] [--max-lag 24] [--max-frames 256]"""
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

C, HOP_FRAMES = 4, 32


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=1024)
    ap.add_argument("--pushes", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--max-lag", type=int, default=24)
    ap.add_argument("--max-frames", type=int, default=256)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("stream_tdoa_bench needs the GPU: nothing is measured without one")
    S = a.streams
    gen = torch.Generator(device="cuda").manual_seed(0)
    rng = np.random.default_rng(0)
    n_push = HOP_FRAMES * feature.HOP
    m = sed.LightningTimePooledCRNN(dropout=0.0, in_channels=C).cuda().eval()
    tf = m.time_factor
    # two pushes' worth of audio per feed: noise, and noise with a tone that comes and goes
    pcm = 0.05 * torch.randn(2, S, n_push, C, device="cuda", generator=gen)
    pcm[1] += torch.sin(2 * np.pi * 2000 * torch.arange(n_push, device="cuda") / feature.SR)[None, :, None]
    pieces = [[pcm[i, s] for s in range(S)] for i in range(2)]
    with torch.no_grad():
        thr = float(sed.EventDetector(m, hop=HOP_FRAMES)(torch.cat([pcm[i % 2, 0] for i in range(8)]), sr=feature.SR, channels=C).probs.median())
        plain = sed.EventDetector(m, hop=HOP_FRAMES, median=3, threshold=thr)
        loc = sed.EventDetector(m, hop=HOP_FRAMES, median=3, threshold=thr, localize=sed.TDOA(a.max_lag, a.max_frames))
        st_p = plain.stream(S)
        least = loc.stream(1, history_frames="min").history_frames
        # cap = (history + step_frames) * hop_length + n_fft: a whole number of output frames, so that the linear route exists
        hist = next(h for h in range(least, least + tf) if (h + 4 * HOP_FRAMES + feature.NFFT // feature.HOP) % tf == 0)
        st_l = loc.stream(S, history_frames=hist)
        cap = st_l.cap
        assert cap % (tf * feature.HOP) == 0 and st_l.step_frames == 4 * HOP_FRAMES
        out = {"tool": "stream_tdoa_bench", "streams": S, "channels": C, "push_seconds": round(n_push / feature.SR, 4),
               "max_lag": a.max_lag, "max_frames": a.max_frames, "lat_frames": st_l.lat, "history_frames": hist, "ring_samples": cap,
               "ring_bytes_per_feed": 4 * C * cap, "state_bytes_per_feed": {"plain": st_p.state_bytes // S, "localising": st_l.state_bytes // S}}
        # ── (a) the push ──
        warm = -(-cap // n_push) + 6                                        # until the rings have wrapped and every feed emits
        for st in (st_p, st_l):                                             # the copy filter holds one sample back: one sample first,
            st.push([pcm[0, s, :1] for s in range(S)])                      # and every push ends on a whole window hop
        for i in range(warm):
            st_p.push(pieces[i % 2])
            st_l.push(pieces[i % 2])
        t_p, t_l, t_loc, events, located = [], [], [], 0, 0
        for rep in range(a.reps):
            for i in range(a.pushes):
                t_p.append(wall(lambda: st_p.push(pieces[i % 2]))[0])
                st_l.marks = []
                ms, res = wall(lambda: st_l.push(pieces[i % 2]))
                t_l.append(ms)
                t_loc.append(sum(x.elapsed_time(y) for n, x, y in st_l.marks if n == "locate"))
                st_l.marks = None
                events += len(res)
                located += int((res.events["loc_frames"] > 0).sum())
        mp, ml, mloc = float(np.median(t_p)), float(np.median(t_l)), float(np.median(t_loc))
        out["push"] = {"plain_ms": round(mp, 4), "localising_ms": round(ml, 4), "locate_device_ms": round(mloc, 4),
                       "events_per_push": round(events / len(t_l), 2), "located_per_push": round(located / len(t_l), 2)}
        print(f"S={S}: push {mp:.3f} ms, with history_frames={hist} {ml:.3f} ms (+{ml - mp:.3f} ms; event_tdoa_ring on the device "
              f"{mloc:.3f} ms for {events / len(t_l):.1f} events per push, {located / len(t_l):.1f} located); ring {4 * C * cap / 1e6:.2f} MB "
              f"per feed", flush=True)
        # ── (b) the ring route against linearise + event_tdoa ──
        ring, n = st_l._ring, st_l._n.copy()
        n0 = int(n[0])
        assert (n == n0).all() and n0 > cap and (n0 - cap) % (tf * feature.HOP) == 0
        shift_out = (n0 - cap) // (tf * feature.HOP)                        # the linear buffer's frame 0, in output frames
        n_out = (1 + n0 // feature.HOP) // tf
        slower = []
        out["locate"] = {}
        for name, feeds, per_feed in (("every feed", np.arange(S), 2), ("64 feeds", np.sort(rng.choice(S, min(64, S), replace=False)), 1)):
            F = len(feeds)
            dur = rng.integers(1, a.max_frames // tf + 1, (F, per_feed))     # at most max_frames frames: the rule accepts every one
            off = n_out - rng.integers(0, 6, (F, per_feed))                 # the events a step emits are recent
            on = off - dur
            pk = on + (rng.random((F, per_feed)) * dur).astype(np.int64)
            who = np.repeat(feeds, per_feed)
            col = lambda x: torch.from_numpy(np.ascontiguousarray(x.reshape(-1).astype(np.int32))).cuda()    # noqa: E731
            ev = {"stream": col(who), "onset": col(on), "offset": col(off), "peak_frame": col(pk)}
            ev_lin = {"rec": col(np.repeat(np.arange(F), per_feed)), "onset": col(on - shift_out), "offset": col(off - shift_out),
                      "peak_frame": col(pk - shift_out)}
            sel = torch.from_numpy(feeds).cuda()
            clips = [(i * cap, cap) for i in range(F * C)]
            kw = dict(max_lag=a.max_lag, max_frames=a.max_frames)

            def via_ring():
                return feature.event_tdoa_ring(ring, cap, n, C, ev, tf, lat_frames=st_l.lat, history_frames=hist, **kw)

            def via_linear():
                lanes = ring.view(S, C * cap) if F == S else ring.view(S, C * cap).index_select(0, sel)
                lin = torch.roll(lanes.view(F * C, cap), -(n0 % cap), 1)    # the oldest kept sample first
                return feature.event_tdoa(lin.view(-1), clips, C, ev_lin, tf, **kw)

            r, l = via_ring(), via_linear()
            n_loc = int((r["loc_frames"] > 0).sum())
            same = all(torch.equal(r[k].view(torch.int32), l[k].view(torch.int32)) for k in ("lag", "strength", "loc_frames"))
            if n_loc != r["loc_frames"].numel() or not same:
                raise SystemExit(f"{name}: the two routes disagree ({n_loc} of {r['loc_frames'].numel()} located, equal bits: {same})")
            del r, l
            ts = [[], []]
            for _ in range(a.reps * 4):
                for t, fn in zip(ts, (via_ring, via_linear)):
                    t.append(wall(fn)[0])
            tr, tl = float(np.median(ts[0])), float(np.median(ts[1]))
            out["locate"][name] = {"events": int(who.size), "located_frames": int(feature_frames(on, off, pk, tf, n0, a.max_frames)),
                                   "ring_ms": round(tr, 4), "linearise_event_tdoa_ms": round(tl, 4)}
            print(f"{name}: {who.size} events, event_tdoa_ring {tr:.3f} ms, roll + event_tdoa {tl:.3f} ms ({tl / tr:.2f}x); same bits",
                  flush=True)
            if tr > tl:
                slower.append(f"{name}: event_tdoa_ring {tr:.3f} ms is slower than linearise + event_tdoa {tl:.3f} ms")
    print(json.dumps(out))
    if slower:
        raise SystemExit("; ".join(slower))


def feature_frames(on, off, pk, tf, n, max_frames):
    n_feat = 1 + n // feature.HOP
    return sum(f1 - f0 for f0, f1 in (sed.event_frames(a, b, p, tf, n_feat, max_frames)
                                      for a, b, p in zip(on.reshape(-1).tolist(), off.reshape(-1).tolist(), pk.reshape(-1).tolist())))


if __name__ == "__main__":
    main()
