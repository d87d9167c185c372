"""Independent restatement of the polyphonic sound detection score (sed_crnn_amd/tune.py, csrc/psds.hip) for the
tests: Python integers and float64, written from the definition on interval lists with explicit pairwise overlaps — no prefix
arrays, no merge walk, no sorting tricks; clarity, not speed.

All positions are output frames local to a recording, offsets exclusive.  ``ref[r][k]`` = sorted, pairwise disjoint list of
(onset, offset); ``sys_events[r]`` = dict of arrays cls / onset / offset as ``detect_ref.decode`` returns them.  Criteria are
integers in thousandths (``cttc = 0``: no cross triggers).  Counts per class: (tp, n_ref, n_sys, fp), summed over recordings;
``ct[k][c]`` = cross triggers of detections of class k on the reference of class c."""
import numpy as np

import tune_ref


def overlap(x, y):
    """frames that the intervals x and y share"""
    return max(0, min(x[1], y[1]) - max(x[0], y[0]))


def covered(x, events):
    """|x ∩ G|: frames of x covered by the (disjoint) events"""
    return sum(overlap(x, t) for t in events)


def counts_one(sys_by_class, ref_by_class, dtc, gtc, cttc):
    """one recording: sys_by_class[k], ref_by_class[k] lists of (onset, offset) -> (counts [K][4], ct [K][K]) of Python ints"""
    K = len(ref_by_class)
    counts = [[0, 0, 0, 0] for _ in range(K)]
    ct = [[0] * K for _ in range(K)]
    for k in range(K):
        D, Gk = [tuple(d) for d in sys_by_class[k]], [tuple(t) for t in ref_by_class[k]]
        relevant = [d for d in D if 1000 * covered(d, Gk) >= dtc * (d[1] - d[0])]
        counts[k][0] = sum(1 for t in Gk if 1000 * sum(overlap(d, t) for d in relevant) >= gtc * (t[1] - t[0]))
        counts[k][1] = len(Gk)
        counts[k][2] = len(D)
        for d in D:
            if d in relevant:
                continue
            counts[k][3] += 1
            if cttc > 0:
                for c in range(K):
                    if c != k and 1000 * covered(d, [tuple(t) for t in ref_by_class[c]]) >= cttc * (d[1] - d[0]):
                        ct[k][c] += 1
    return counts, ct


def by_class(ev, K):
    """decoded events (dict of arrays) -> [K] lists of (onset, offset)"""
    cls, on, off = np.asarray(ev["cls"]), np.asarray(ev["onset"]), np.asarray(ev["offset"])
    return [list(zip(on[cls == k].tolist(), off[cls == k].tolist())) for k in range(K)]


def counts(sys_events, ref, K, dtc, gtc, cttc):
    """all recordings of one setting -> (int64 [K, 4], int64 [K, K])"""
    c_sum, ct_sum = np.zeros((K, 4), np.int64), np.zeros((K, K), np.int64)
    for r, ev in enumerate(sys_events):
        c, ct = counts_one(by_class(ev, K), ref[r], dtc, gtc, cttc)
        c_sum += np.asarray(c, np.int64)
        ct_sum += np.asarray(ct, np.int64)
    return c_sum, ct_sum


def sweep(probs, out_off, ref, grid, dtc, gtc, cttc):
    """-> (int64 [G, K, 4], int64 [G, K, K]): detect_ref.decode per recording and setting, then the criteria"""
    probs = np.asarray(probs, np.float32)
    K = probs.shape[1]
    both = [counts(tune_ref.decode_all(probs, out_off, s), ref, K, dtc, gtc, cttc) for s in grid]
    if not both:
        return np.zeros((0, K, 4), np.int64), np.zeros((0, K, K), np.int64)
    return np.stack([b[0] for b in both]), np.stack([b[1] for b in both])


def score(counts, ct, n_out, ref, frame_seconds, cttc, alpha_ct, alpha_st, e_max):
    """the score from the integers: -> dict(psds, e, etpr, mean, std, tpr [G][K], fpr, efpr, kept, per_class_auc {k: area})"""
    counts, ct = np.asarray(counts), np.asarray(ct)
    G, K = counts.shape[0], counts.shape[1]
    fs = float(frame_seconds)
    T = float(sum(int(n) for n in n_out)) * fs
    T_c = [float(sum(b - a for rec in ref for a, b in rec[c])) * fs for c in range(K)]
    kept = [k for k in range(K) if G and int(counts[0, k, 1]) > 0]
    if not kept:
        raise ValueError("no class has a reference event")
    tpr = [[int(counts[g, k, 0]) / int(counts[g, k, 1]) if int(counts[g, k, 1]) else float("nan") for k in range(K)] for g in range(G)]
    fpr = [[int(counts[g, k, 3]) / (T / 3600.0) for k in range(K)] for g in range(G)]
    efpr = [[fpr[g][k] for k in range(K)] for g in range(G)]
    if cttc > 0 and alpha_ct > 0:
        for g in range(G):
            for k in range(K):
                ctr = [int(ct[g, k, c]) / (T_c[c] / 3600.0) for c in range(K) if c != k and T_c[c] > 0]
                if ctr:
                    efpr[g][k] = fpr[g][k] + alpha_ct * (sum(ctr) / len(ctr))
    e = sorted({efpr[g][k] for g in range(G) for k in kept if efpr[g][k] <= e_max}) + [float(e_max)]

    def tpr_k(k, x):
        best = 0.0
        for g in range(G):
            if efpr[g][k] <= x and tpr[g][k] > best:
                best = tpr[g][k]
        return best

    mean, std, etpr = [], [], []
    for x in e:
        v = [tpr_k(k, x) for k in kept]
        m = sum(v) / len(v)
        s = (sum((y - m) ** 2 for y in v) / len(v)) ** 0.5
        mean.append(m); std.append(s); etpr.append(m - alpha_st * s)
    psds = sum(etpr[i] * (e[i + 1] - e[i]) for i in range(len(e) - 1)) / e_max
    auc = {k: sum(tpr_k(k, e[i]) * (e[i + 1] - e[i]) for i in range(len(e) - 1)) / e_max for k in kept}
    return dict(psds=psds, e=e, etpr=etpr, mean=mean, std=std, tpr=tpr, fpr=fpr, efpr=efpr, kept=kept, per_class_auc=auc)
