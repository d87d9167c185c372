#!/usr/bin/env python3
"""Live streams that emit each located event's audio (csrc/mvdr.hip sed_event_mvdr_ring, csrc/beam.hip
sed_event_beamform_ring).  --streams (1 024) four-channel feeds at the detector's rate, Lightning-size net, a tetrahedron of 18 cm
and a sphere of 642 directions; every push hands each feed one window hop of audio (32 feature frames = 32 768 samples = 0.74 s),
resident on the device.
  (a) push      host wall clock of one steady-state push (it ends in the step's blocking reads) of a stream with
                ``emit_audio=True`` — one per beam, ``extract=sed.MVDR(...)`` and ``extract=sed.DelaySum(...)`` — next to the same
                detector without ``extract=`` (it locates, and emits no audio); the streams take the same pieces and alternate
                push by push.  The net is untrained: the threshold sits at the median of its track, so that pushes emit events.
  (b) extract   the ring route, ``feature.event_mvdr_ring`` / ``feature.event_beamform_ring`` on the stream's rings, against the only
                other route to the same bits: linearise the rings with torch (index_select of the feeds that have events, one
                roll to put the oldest sample first), then ``feature.event_mvdr`` / ``feature.event_beamform`` on that planar buffer
                with the event table moved to its frames.  Two event tables: two recent events in every feed (every ring is
                linearised), and one event in each of 64 feeds (only those are).  The events are located by hand (a drawn
                direction, all their frames) and start at least one output frame after the oldest kept sample, so that the
                delay-and-sum beam's reach to the left is inside both buffers; the history is rounded up so that the oldest kept
                sample starts an output frame.  Both routes must return the same bits.
Every figure is a median over --reps repetitions (of --pushes pushes) after a warm-up; the alternatives alternate in one process.
One JSON line at the end.  Exits non-zero when a ring route is the slower one for an event table.
python tools/stream_extract_bench.py [--streams 1024] [--pushes 20] [--reps 5] [--max-frames 64] [--loading 1e-2]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import sed_crnn_amd as sed
from sed_crnn_amd import feature
from tools.doa_bench import EDGE, tetrahedron
from tools.stream_tdoa_bench import HOP_FRAMES, C, wall


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=1024)
    ap.add_argument("--pushes", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--max-frames", type=int, default=64)
    ap.add_argument("--loading", type=float, default=1e-2)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("stream_extract_bench needs the GPU: nothing is measured without one")
    S = a.streams
    gen = torch.Generator(device="cuda").manual_seed(0)
    rng = np.random.default_rng(0)
    n_push = HOP_FRAMES * feature.HOP
    m = sed.LightningTimePooledCRNN(dropout=0.0, in_channels=C).cuda().eval()
    tf = m.time_factor
    pcm = 0.05 * torch.randn(2, S, n_push, C, device="cuda", generator=gen)
    pcm[1] += torch.sin(2 * np.pi * 2000 * torch.arange(n_push, device="cuda") / feature.SR)[None, :, None]
    pieces = [[pcm[i, s] for s in range(S)] for i in range(2)]
    doa = sed.DOA(tetrahedron(EDGE), sed.DirectionGrid.sphere(642), max_frames=a.max_frames)
    beams = {"mvdr": sed.MVDR(a.loading), "delaysum": sed.DelaySum(16, 16)}
    with torch.no_grad():
        thr = float(sed.EventDetector(m, hop=HOP_FRAMES)(torch.cat([pcm[i % 2, 0] for i in range(8)]), sr=feature.SR, channels=C).probs.median())
        kw = dict(hop=HOP_FRAMES, median=3, threshold=thr, localize=doa)
        located = sed.EventDetector(m, **kw)
        least = located.stream(1, history_frames="min").history_frames
        # cap = (history + step_frames) * hop_length + n_fft: a whole number of output frames, so that the linear route exists
        hist = next(h for h in range(least, least + tf) if (h + 4 * HOP_FRAMES + feature.NFFT // feature.HOP) % tf == 0)
        streams = {"located": located.stream(S, history_frames=hist)}
        for name, beam in beams.items():
            streams[name] = sed.EventDetector(m, extract=beam, **kw).stream(S, history_frames=hist, emit_audio=True)
        st0 = streams["located"]
        cap = st0.cap
        assert cap % (tf * feature.HOP) == 0 and all(st.cap == cap and st.state_bytes == st0.state_bytes for st in streams.values())
        out = {"tool": "stream_extract_bench", "streams": S, "channels": C, "push_seconds": round(n_push / feature.SR, 4),
               "max_frames": a.max_frames, "loading": a.loading, "lat_frames": st0.lat, "history_frames": hist, "ring_samples": cap,
               "state_bytes_per_feed": st0.state_bytes // S}
        # ── (a) the push ──
        warm = -(-cap // n_push) + 6                                        # until the rings have wrapped and every feed emits
        for st in streams.values():                                         # the copy filter holds one sample back: one sample first,
            st.push([pcm[0, s, :1] for s in range(S)])                      # and every push ends on a whole window hop
        for i in range(warm):
            for st in streams.values():
                st.push(pieces[i % 2])
        t = {k: [] for k in streams}
        dev = {k: [] for k in beams}
        events = {k: 0 for k in streams}
        samples = {k: 0 for k in beams}
        for rep in range(a.reps):
            for i in range(a.pushes):
                for name, st in streams.items():
                    st.marks = [] if name in beams else None
                    ms, res = wall(lambda: st.push(pieces[i % 2]))
                    t[name].append(ms)
                    events[name] += len(res)
                    if name in beams:
                        dev[name].append(sum(x.elapsed_time(y) for n, x, y in st.marks if n == "extract"))
                        samples[name] += int(res.audio.numel())
                        st.marks = None
        n_t = len(t["located"])
        base = float(np.median(t["located"]))
        out["push"] = {"located_ms": round(base, 4), "events_per_push": round(events["located"] / n_t, 2)}
        for name in beams:
            ms, d = float(np.median(t[name])), float(np.median(dev[name]))
            out["push"][name] = {"ms": round(ms, 4), "extract_ms": round(d, 4), "audio_seconds_per_push": round(samples[name] / n_t / feature.SR, 3)}
            print(f"S={S}: push {base:.3f} ms without extract=, {ms:.3f} ms with {name} and emit_audio=True (+{ms - base:.3f} ms; the "
                  f"extract call {d:.3f} ms for {events[name] / n_t:.1f} events per push, {samples[name] / n_t / feature.SR:.1f} s of audio)",
                  flush=True)
        # ── (b) the ring routes against linearise + the linear entries ──
        st = streams["mvdr"]
        ring, n = st._ring, st._n.copy()
        n0 = int(n[0])
        assert (n == n0).all() and n0 > cap and (n0 - cap) % (tf * feature.HOP) == 0
        shift_out = (n0 - cap) // (tf * feature.HOP)                        # the linear buffer's frame 0, in output frames
        n_out = (1 + n0 // feature.HOP) // tf
        slower = []
        out["extract"] = {}
        for name, feeds, per_feed in (("every feed", np.arange(S), 2), ("64 feeds", np.sort(rng.choice(S, min(64, S), replace=False)), 1)):
            F = len(feeds)
            dur = rng.integers(1, a.max_frames // tf + 1, (F, per_feed))     # at most max_frames frames: all of them are extracted
            off = n_out - rng.integers(0, 6, (F, per_feed))                 # the events a step emits are recent
            on = off - dur
            assert (on > shift_out).all()                                   # one output frame or more after the oldest kept sample
            pk = on + (rng.random((F, per_feed)) * dur).astype(np.int64)
            who = np.repeat(feeds, per_feed)
            col = lambda x: torch.from_numpy(np.ascontiguousarray(x.reshape(-1).astype(np.int32))).cuda()    # noqa: E731
            loc = {"dir": col(rng.integers(0, len(doa.grid), (F, per_feed))), "loc_frames": col(dur * tf)}
            ev = {"stream": col(who), "onset": col(on), "offset": col(off), "peak_frame": col(pk), **loc}
            ev_lin = {"rec": col(np.repeat(np.arange(F), per_feed)), "onset": col(on - shift_out), "offset": col(off - shift_out),
                      "peak_frame": col(pk - shift_out), **loc}
            sel = torch.from_numpy(feeds).cuda()
            clips = [(i * cap, cap) for i in range(F * C)]
            out["extract"][name] = {"events": int(who.size)}
            for bname, beam in beams.items():
                ring_entry, lin_entry = ((feature.event_mvdr_ring, feature.event_mvdr) if bname == "mvdr" else
                                         (feature.event_beamform_ring, feature.event_beamform))

                def via_ring():
                    return ring_entry(ring, cap, n, C, ev, tf, doa, beam)

                def via_linear():
                    lanes = ring.view(S, C * cap) if F == S else ring.view(S, C * cap).index_select(0, sel)
                    lin = torch.roll(lanes.view(F * C, cap), -(n0 % cap), 1)    # the oldest kept sample first
                    return lin_entry(lin.view(-1), clips, C, ev_lin, tf, doa, beam)

                r, l = via_ring(), via_linear()
                total = int(r["audio"].numel())
                same = all(torch.equal(r[k], l[k]) for k in ("audio_len", "audio_start")) and \
                    torch.equal(r["audio"].view(torch.int32), l["audio"].view(torch.int32))
                if total != int((dur * tf * feature.HOP).sum()) or not same:
                    raise SystemExit(f"{name}, {bname}: the two routes disagree ({total} samples, equal bits: {same})")
                del r, l
                ts = [[], []]
                for _ in range(a.reps * 4):
                    for tt, fn in zip(ts, (via_ring, via_linear)):
                        tt.append(wall(fn)[0])
                tr, tl = float(np.median(ts[0])), float(np.median(ts[1]))
                out["extract"][name][bname] = {"samples": total, "ring_ms": round(tr, 4), "linearise_ms": round(tl, 4)}
                print(f"{name}, {bname}: {who.size} events ({total / feature.SR:.1f} s of audio), the ring entry {tr:.3f} ms, roll + the "
                      f"linear entry {tl:.3f} ms ({tl / tr:.2f}x); same bits", flush=True)
                if tr > tl:
                    slower.append(f"{name}, {bname}: the ring entry {tr:.3f} ms is slower than linearise + the linear entry {tl:.3f} ms")
    print(json.dumps(out))
    if slower:
        raise SystemExit("; ".join(slower))


if __name__ == "__main__":
    main()
