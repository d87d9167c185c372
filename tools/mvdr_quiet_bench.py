#!/usr/bin/env python3
"""Per-event audio by an MVDR beam whose noise frames are picked where the event's class is silent (csrc/mvdr.hip
sed_event_mvdr_quiet).  tools/mvdr_noise_bench.py's workload: --seconds (one hour) of 48 kHz 4-channel int16, device-resident,
resampled once; --events (1 000) events of --classes (10) classes drawn at random, located once with feature.event_doa outside
the timing; MVDR(--loading 1e-2, noise_blocks=--noise-blocks 8, noise_guard=1, noise_select="quiet").  Figures:
  event_mvdr (quiet)    feature.event_mvdr: the span launch, one 8-byte read, the activity and the selection launch, four launches
                        per slice
  quiet_frames          feature.event_quiet_frames alone: what the activity and the selection cost (a workspace, a memset, an
                        upload and the two launches)
  event_mvdr (fixed)    the same call with noise_select="fixed" and with noise_blocks = 0 on the same build, for scale
  torch                 the only other device route to the same numbers: per event torch.stft of the zero-padded segment and of the
                        selected frames — the host hands it the lists the selection made, read back outside the timing —, the einsum
                        covariance, torch.linalg.solve in float64, the combine and torch.istft
The buffers of the first and the last are compared (max abs difference).  Medians over --reps repetitions after a warm-up, the
alternatives alternating in one process.  One JSON line at the end.  Exits non-zero when the kernel route is the slower one.

--parent DIR (a checkout of the parent commit with its library built): also runs DIR/tools/mvdr_noise_bench.py and this tree's
--rounds times each, alternating processes, to show what noise_select="fixed" costs against the parent with Kn = 8 and Kn = 0:
the medians and each side's own spread (max - min), to be judged against the run-to-run spread of one build (0.18 ms).
(A whole checkout and not SED_CRNN_LIB alone: this package binds the new entries at load time, which the parent's library does
not export.)
python tools/mvdr_quiet_bench.py [--seconds 3600] [--events 1000] [--classes 10] [--noise-blocks 8] [--parent DIR] [--rounds 3]"""
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
    """-> {tree: {"Kn": [ms, ...], "0": [...]}}: tools/mvdr_noise_bench.py of both trees, one process each, alternating"""
    got = {"this": {"Kn": [], "0": []}, "parent": {"Kn": [], "0": []}}
    for _ in range(rounds):
        for name, tree in (("parent", parent), ("this", ROOT)):
            env = {k: v for k, v in os.environ.items() if k != "SED_CRNN_LIB"}
            p = subprocess.run([sys.executable, os.path.join(tree, "tools", "mvdr_noise_bench.py")] + passthrough, cwd=tree, env=env,
                               capture_output=True, text=True)
            if p.returncode != 0:
                raise SystemExit(f"{tree}/tools/mvdr_noise_bench.py failed:\n{p.stdout[-2000:]}\n{p.stderr[-2000:]}")
            line = json.loads(p.stdout.strip().splitlines()[-1])
            got[name]["Kn"].append(line["event_mvdr_noise_ms"])
            got[name]["0"].append(line["event_mvdr_own_ms"])
    return got


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=int, default=3600)
    ap.add_argument("--events", type=int, default=1000)
    ap.add_argument("--classes", type=int, default=10)
    ap.add_argument("--loading", type=float, default=1e-2)
    ap.add_argument("--noise-blocks", type=int, default=8)
    ap.add_argument("--noise-guard", type=int, default=1)
    ap.add_argument("--max-frames", type=int, default=256)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--parent", default=None)
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mvdr_quiet_bench needs the GPU: nothing is measured without one")
    Kn, G, K = a.noise_blocks, a.noise_guard, a.classes
    gen = torch.Generator(device="cuda").manual_seed(0)
    rng = np.random.default_rng(0)
    x = torch.randint(-8000, 8000, (48000 * a.seconds, C), device="cuda", generator=gen, dtype=torch.int16)
    pcm, clips = resample_many([x], 48000, feature.SR, C, "cuda", keep_channels=True)
    del x
    n = clips[0][1]
    E = a.events
    rows = event_table(E, 1 + n // feature.HOP, rng)
    ev = {k: torch.from_numpy(np.ascontiguousarray(rows[:, i])).cuda() for i, k in enumerate(("onset", "offset", "peak_frame"))}
    ev["cls"] = torch.from_numpy(rng.integers(0, K, E).astype(np.int32)).cuda()
    doa = sed.DOA(tetrahedron(EDGE), sed.DirectionGrid.sphere(2562), max_frames=a.max_frames)
    quiet = sed.MVDR(a.loading, noise_blocks=Kn, noise_guard=G, noise_select="quiet")
    fixed, own = sed.MVDR(a.loading, noise_blocks=Kn, noise_guard=G), sed.MVDR(a.loading)
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

        def new():
            return feature.event_mvdr(pcm, clips, C, ev, TF, doa, quiet, n_classes=K)

        def frames_only():
            return feature.event_quiet_frames(clips, C, ev, TF, doa, quiet, K)

        def fixed_route():
            return feature.event_mvdr(pcm, clips, C, ev, TF, doa, fixed)

        def own_route():
            return feature.event_mvdr(pcm, clips, C, ev, TF, doa, own)

        got = new()
        assert np.array_equal(got["audio_len"].cpu().numpy(), lens) and np.array_equal(got["audio_start"].cpu().numpy(), starts)
        only = frames_only()
        assert torch.equal(only["noise_frames"], got["noise_frames"]) and torch.equal(only["noise_sel"], got["noise_sel"])
        used, sel = got["noise_frames"].cpu().numpy(), got["noise_sel"].cpu().numpy()            # the lists the torch route is handed
        plan = [(int(starts[e]), spans[e][0], int(lens[e]), int(dirs[e]), [spans[e][0] - (G + 2 + int(q)) * B for q in sel[e][:used[e]]])
                for e in range(E) if lens[e] > 0]

        def torch_route():
            out = torch.empty(total, device="cuda")
            for start, s0, ln, d, firsts in plan:
                J = -(-ln // B)
                seg = torch.nn.functional.pad(torch.stack([ch[s0:s0 + ln] for ch in chans]), (0, J * B - ln))
                X = torch.stft(seg, N, B, window=win, center=True, pad_mode="constant", return_complex=True)      # [C, 1025, J + 1]
                Xn = X
                if firsts:                                                                                        # [C, 1025, n_e]
                    fr = torch.stack([torch.stack([ch[f:f + N] for f in firsts]) for ch in chans])
                    Xn = torch.fft.rfft(fr * win, dim=-1).transpose(1, 2)
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

        diff = float((got["audio"] - torch_route()).abs().max())
        scale = float(got["audio"].abs().max())
        same_as_fixed = int(((sel == np.arange(Kn - 1, -1, -1)[None, :]).all(1) & (lens > 0)).sum())
        del got, only
        t_new, t_sel, t_fixed, t_own, t_torch = med([new, frames_only, fixed_route, own_route, torch_route], a.reps)
    out = {"tool": "mvdr_quiet_bench", "seconds": a.seconds, "channels": C, "time_factor": TF, "events": E, "classes": K,
           "extracted_events": len(plan), "noise_events": int(((used > 0) & (lens > 0)).sum()), "partial_events": int(((used > 0) & (used < Kn)).sum()),
           "fixed_stretch_events": same_as_fixed, "loading": a.loading, "noise_blocks": Kn, "noise_guard": G, "noise_search": quiet.noise_search,
           "max_frames": a.max_frames, "samples": total, "event_mvdr_quiet_ms": round(t_new, 4), "quiet_frames_ms": round(t_sel, 4),
           "event_mvdr_fixed_ms": round(t_fixed, 4), "event_mvdr_own_ms": round(t_own, 4), "torch_ms": round(t_torch, 4),
           "max_abs_diff": diff, "max_abs_audio": scale}
    print(f"{E} events of {K} classes ({len(plan)} extracted, {out['noise_events']} from selected frames — {out['partial_events']} from fewer "
          f"than {Kn}, {same_as_fixed} from the fixed stretch's —, {total} samples = {total / feature.SR:.1f} s), Kn = {Kn}, G = {G}, "
          f"S = {quiet.noise_search}: event_mvdr {t_new:.3f} ms, of which event_quiet_frames alone {t_sel:.3f} ms; noise_select='fixed' "
          f"{t_fixed:.3f} ms, noise_blocks = 0 {t_own:.3f} ms; torch route {t_torch:.3f} ms ({t_torch / t_new:.1f}x); the buffers differ by "
          f"at most {diff:.2e} (largest sample {scale:.3g})", flush=True)
    if a.parent:
        torch.cuda.empty_cache()
        ab = against_parent(os.path.abspath(a.parent), a.rounds, ["--seconds", str(a.seconds), "--events", str(a.events), "--loading",
                                                                   str(a.loading), "--noise-blocks", str(Kn), "--noise-guard", str(G),
                                                                   "--max-frames", str(a.max_frames), "--reps", str(a.reps)])
        for name, both in ab.items():
            for which, v in both.items():
                out[f"fixed_{name}_kn{which if which == '0' else Kn}_ms"] = v
                print(f"noise_select='fixed', noise_blocks = {0 if which == '0' else Kn}, {name} tree: event_mvdr {v} ms, median "
                      f"{float(np.median(v)):.3f}, spread {max(v) - min(v):.3f}", flush=True)
    print(json.dumps(out))
    if t_new > t_torch:
        raise SystemExit(f"event_mvdr {t_new:.3f} ms is slower than the torch route {t_torch:.3f} ms")


if __name__ == "__main__":
    main()
