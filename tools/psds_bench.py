#!/usr/bin/env python3
"""The polyphonic sound detection score: one ``det.psds`` over a sweep of thresholds against the route it replaces — a loop of
``det.decode_many`` per threshold with every event table read back to the host — and, reported SEPARATELY, the host interval
arithmetic that route still needs afterwards (``tests/psds_ref.py`` on the copied events).  ``tools/tune_bench.py``'s workload:
synthetic smooth tracks, about --hours of output frames split into --recordings recordings of uneven length, K classes; the
reference events are the decode of a perturbed copy of the track.  Both scenarios; the two device paths alternate in one
process; host wall clock around work that ends in a synchronise, after a warm-up; median of --reps.  The host arithmetic is
timed once per scenario (it does not touch the device) on --host-settings evenly spread thresholds and scaled to all of them;
its counts are checked against the sweep's.  One JSON line at the
end; the tool FAILS when the sweep is slower than the decode loop alone.
python -m tools.psds_bench [--hours 10] [--recordings 300] [--classes 6] [--thresholds 50] [--reps 20] [--host-settings 10]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

import sed_crnn_amd as sed
from tools.tune_bench import make_tracks


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--hours", type=float, default=10.0)
    ap.add_argument("--recordings", type=int, default=300)
    ap.add_argument("--classes", type=int, default=6)
    ap.add_argument("--thresholds", type=int, default=50)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--host-settings", type=int, default=10, help="thresholds, evenly spread, whose events go through the host "
                    "arithmetic: it is timed once on those and scaled to all of them")
    ap.add_argument("--scenarios", nargs="+", default=["scenario1", "scenario2", "scenario2_no_ct"],
                    help="which criteria to time; scenario2_no_ct is scenario 2 without its cross-trigger criterion: the difference "
                    "to scenario2 is the cross-trigger work alone (scenario 1 judges other detections non-relevant)")
    a = ap.parse_args()
    import psds_ref
    rng = np.random.default_rng(0)
    K, R = a.classes, a.recordings
    m = sed.LightningTimePooledCRNN(dropout=0.0, n_classes=K).cuda().eval()
    det = sed.EventDetector(m, median=5, min_gap=2, min_len=3)
    n_total = int(a.hours * 3600 / det.frame_seconds)
    probs_h, out_off = make_tracks(rng, n_total, R, K)
    probs = torch.from_numpy(probs_h).cuda()
    tf = m.time_factor
    bp = sed.plan_batch([tf * n for n in np.diff(out_off)], tf, K)         # decode_many takes R and out_off from it
    assert list(bp.out_off) == out_off
    noisy = torch.from_numpy(np.clip(probs_h + rng.standard_normal(probs_h.shape).astype(np.float32) * 0.05, 0, 1)).cuda()
    truth = det.with_decoder(threshold=0.55, low=0.45, median=5, min_gap=2, min_len=3)
    ev, offs = truth.decode_many(noisy, bp)
    ref = sed.ReferenceEvents.from_result(sed.BatchDetectionResult(noisy, ev, det.frame_seconds, bp.plans, out_off, offs))
    ref_lists = [[ref.events(r, k) for k in range(K)] for r in range(R)]
    thresholds = np.linspace(0.01, 0.99, a.thresholds)
    dets = [det.with_decoder(threshold=float(v)) for v in thresholds]      # each keeps its own workspace and event buffers
    known = {"scenario1": sed.PSDSCriteria.scenario1(), "scenario2": sed.PSDSCriteria.scenario2(),
             "scenario2_no_ct": sed.PSDSCriteria(0.1, 0.1)}
    scenarios = {n: known[n] for n in a.scenarios}

    def run_sweep(crit):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = det.psds((probs, out_off), ref, thresholds=thresholds, criteria=crit)
        res.table()                                          # the one host read: [G, K, 4] and [G, K, K] integers
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, res

    def run_loop():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        tables = []
        for d in dets:
            e, o = d.decode_many(probs, bp)
            tables.append(({k: e[k].cpu().numpy() for k in ("cls", "onset", "offset")}, o))      # the event table, read back
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, tables

    results = {n: run_sweep(c)[1] for n, c in scenarios.items()}         # warm-up of both paths
    _, tables = run_loop()
    times = {n: [] for n in scenarios}
    loops = []
    for _ in range(a.reps):                              # alternate the paths
        for n, c in scenarios.items():
            times[n].append(run_sweep(c)[0])
        loops.append(run_loop()[0])
    sm = {n: float(np.median(t)) for n, t in times.items()}
    lm = float(np.median(loops))
    # the host arithmetic of the replaced route, on the events it read back: timed once, checked against the sweep
    host, agree = {}, True
    picked = np.unique(np.linspace(0, a.thresholds - 1, min(a.host_settings, a.thresholds)).round().astype(int))
    for n, c in scenarios.items():
        t0 = time.perf_counter()
        for g in picked:
            e, o = tables[g]
            per_rec = [{k: e[k][o[r]:o[r + 1]] for k in e} for r in range(R)]
            cnt, ct = psds_ref.counts(per_rec, ref_lists, K, c.dtc_milli, c.gtc_milli, c.cttc_milli)
            got_c, got_ct = results[n].table()
            agree = agree and np.array_equal(cnt, got_c[g]) and np.array_equal(ct, got_ct[g])
        host[n] = (time.perf_counter() - t0) * 1e3 * a.thresholds / len(picked)
    res = next(iter(results.values()))
    out = {"tool": "psds_bench", "hours": a.hours, "output_frames": n_total, "recordings": R, "classes": K, "settings": len(res),
           "bit_tracks": res.n_tracks, "slices": res.n_slices, "workspace_bytes": res.workspace_bytes, "reference_events": len(ref),
           "reps": a.reps, "loop_ms": round(lm, 3), "loop_ms_min_max": [round(min(loops), 3), round(max(loops), 3)],
           "loop_ms_per_setting": round(lm / len(res), 4), "host_settings_timed": int(len(picked)),
           "counts_equal_host_arithmetic": bool(agree)}
    for n in scenarios:
        out.update({f"sweep_ms_{n}": round(sm[n], 3), f"sweep_ms_min_max_{n}": [round(min(times[n]), 3), round(max(times[n]), 3)],
                    f"ratio_{n}": round(lm / sm[n], 2), f"host_arithmetic_ms_{n}": round(host[n], 1),
                    f"psds_{n}": round(results[n].psds(), 6)})
    if "scenario2" in sm and "scenario2_no_ct" in sm:
        out["cross_trigger_ms"] = round(sm["scenario2"] - sm["scenario2_no_ct"], 3)
    if "scenario2" in sm and "scenario1" in sm:
        out["scenario2_minus_scenario1_ms"] = round(sm["scenario2"] - sm["scenario1"], 3)
    print(f"G = {len(res)} thresholds ({res.n_tracks} bit tracks, {res.workspace_bytes} workspace bytes = {res.workspace_bytes / 2 ** 20:.1f} MiB) "
          f"on {n_total} frames in {R} recordings, K={K}: sweep " + ", ".join(f"{sm[n]:.2f} ms ({n})" for n in scenarios) +
          f"; loop of decode_many with the event tables read back {lm:.2f} ms ({lm / len(res):.3f} ms per threshold); host interval "
          "arithmetic on top of the loop " + ", ".join(f"{host[n]:.0f} ms ({n})" for n in scenarios) +
          f" (timed on {len(picked)} thresholds, scaled to {len(res)}); counts == host arithmetic: {agree}", flush=True)
    print(json.dumps(out))
    if not agree:
        sys.exit("the sweep's counts differ from the host arithmetic on the decoder's events")
    worst = max(sm.values())
    if worst > lm:                                       # the requirement: the sweep is no slower than the decode loop ALONE
        sys.exit(f"the sweep ({worst:.2f} ms) is slower than the loop of decode_many ({lm:.2f} ms)")


if __name__ == "__main__":
    main()
