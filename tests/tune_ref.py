"""Independent numpy restatement of event scoring and the decoder sweep (sed_crnn_amd/tune.py, csrc/tune.hip) for the tests,
written with plain loops for clarity, not speed.

All positions are output frames local to a recording, offsets exclusive.  ``ref[r][k]`` = sorted, pairwise disjoint list of
(onset, offset); ``sys_events[r]`` = dict of arrays cls / onset / offset as ``detect_ref.decode`` returns them (sorted by class,
then onset).  Counts per class: (ev_tp, n_sys, n_ref, seg_tp, seg_sys, seg_ref), summed over recordings."""
import math

import numpy as np

import detect_ref


def tolerances(ref_events, offset_collar=None, offset_percent=None):
    """per reference event: -1 for onset-only scoring, else max(offset_collar, floor(offset_percent * length)) in float64"""
    if offset_collar is None and offset_percent is None:
        return [-1] * len(ref_events)
    oc = 0 if offset_collar is None else int(offset_collar)
    pc = 0.0 if offset_percent is None else float(offset_percent)
    return [max(oc, int(math.floor(np.float64(pc) * np.float64(b - a)))) for a, b in ref_events]


def match_events(sys_events, ref_events, collar, tol):
    """the greedy of the definition: system events in order, each to the first unmatched reference event that satisfies the
    onset condition and (tol >= 0) the offset condition -> number of matches"""
    taken = [False] * len(ref_events)
    tp = 0
    for a, b in sys_events:
        for j, (ra, rb) in enumerate(ref_events):
            if taken[j] or abs(a - ra) > collar:
                continue
            if tol[j] >= 0 and abs(b - rb) > tol[j]:
                continue
            taken[j] = True
            tp += 1
            break
    return tp


def active_blocks(events, n_out, block):
    n_blk = -(-n_out // block)
    act = np.zeros(n_blk, bool)
    for a, b in events:
        for j in range(a, b):
            act[j // block] = True
    return act


def score(sys_events, ref, n_out, K, collar=1, offset_collar=None, offset_percent=None, block=1):
    """-> int64 [K, 6]"""
    out = np.zeros((K, 6), np.int64)
    for r, ev in enumerate(sys_events):
        for k in range(K):
            sel = np.asarray(ev["cls"]) == k
            sys_k = list(zip(np.asarray(ev["onset"])[sel].tolist(), np.asarray(ev["offset"])[sel].tolist()))
            ref_k = list(ref[r][k])
            tol = tolerances(ref_k, offset_collar, offset_percent)
            s_act, r_act = active_blocks(sys_k, n_out[r], block), active_blocks(ref_k, n_out[r], block)
            out[k] += (match_events(sys_k, ref_k, collar, tol), len(sys_k), len(ref_k), int((s_act & r_act).sum()), int(s_act.sum()),
                       int(r_act.sum()))
    return out


def decode_all(probs, out_off, setting):
    """detect_ref.decode of every recording for one setting dict (threshold, low, median, min_gap, min_len)"""
    return [detect_ref.decode(probs[out_off[r]:out_off[r + 1]], lo=setting["low"], hi=setting["threshold"], median=setting["median"],
                              min_gap=setting["min_gap"], min_len=setting["min_len"]) for r in range(len(out_off) - 1)]


def sweep(probs, out_off, ref, grid, collar=1, offset_collar=None, offset_percent=None, block=1):
    """-> int64 [G, K, 6]: detect_ref.decode per recording and setting, then score"""
    probs = np.asarray(probs, np.float32)
    K = probs.shape[1]
    n_out = np.diff(out_off).tolist()
    return np.stack([score(decode_all(probs, out_off, s), ref, n_out, K, collar, offset_collar, offset_percent, block) for s in grid]
                    ) if len(grid) else np.zeros((0, K, 6), np.int64)


def events_to_ref(events, K):
    """decoded events of the recordings -> ref[r][k] lists"""
    return [[list(zip(np.asarray(ev["onset"])[np.asarray(ev["cls"]) == k].tolist(),
                      np.asarray(ev["offset"])[np.asarray(ev["cls"]) == k].tolist())) for k in range(K)] for ev in events]
