"""Independent numpy / float64 restatement of whole-recording detection (sed_crnn_amd/detect.py, csrc/detect.hip) for the
tests: the window grid, the stitch of per-window logits and the event decoder, written for clarity, not speed."""
import numpy as np


def window_starts(N, tf, L, hop):
    """window starts in input frames, and the window length (module docstring of sed_crnn_amd/detect.py)"""
    n_out = N // tf
    if N < L:
        return [0], tf * n_out
    starts = list(range(0, N - L + 1, hop))
    last = ((N - L) // tf) * tf
    if starts[-1] != last:
        starts.append(last)
    return starts, L


def stitch(logits, starts_out, n_out, combine="mean", trim=0):
    """logits [n_win, win_out, K] at output-frame starts -> float64 probs [n_out, K]"""
    logits = np.asarray(logits, np.float64)
    n_win, win_out, K = logits.shape
    p = 1.0 / (1.0 + np.exp(-logits))
    acc = np.zeros((n_out, K)) if combine == "mean" else np.full((n_out, K), -np.inf)
    cnt = np.zeros(n_out, np.int64)
    for w, s in enumerate(starts_out):
        lo = trim if s > 0 else 0
        hi = win_out - (trim if s + win_out < n_out else 0)
        seg = p[w, lo:hi]
        if combine == "mean":
            acc[s + lo:s + hi] += seg
        else:
            acc[s + lo:s + hi] = np.maximum(acc[s + lo:s + hi], seg)
        cnt[s + lo:s + hi] += 1
    assert (cnt > 0).all(), "uncovered output frame"
    return acc / cnt[:, None] if combine == "mean" else acc


def median_nearest(p, width):
    """scipy.ndimage.median_filter(p, size=(width, 1), mode='nearest') restated: the middle element of each window"""
    p = np.asarray(p)
    if width == 1:
        return p.copy()
    r = width // 2
    pad = np.concatenate([np.repeat(p[:1], r, 0), p, np.repeat(p[-1:], r, 0)], 0)
    win = np.stack([pad[d:d + p.shape[0]] for d in range(width)], -1)
    return np.sort(win, -1)[..., r]


def decode(probs, lo=0.5, hi=0.5, median=1, min_gap=0, min_len=1):
    """probs [n_out, K] float32 -> dict of arrays cls, onset, offset (exclusive), peak (float32), peak_frame, sorted by
    (class, onset).  Comparisons in float32 like the kernel: a frame is on iff p' > lo, a run is kept iff max p' > hi."""
    probs = np.asarray(probs, np.float32)
    lo, hi = np.float32(lo), np.float32(hi)
    pf = median_nearest(probs, median)
    out = {k: [] for k in ("cls", "onset", "offset", "peak", "peak_frame")}
    n = probs.shape[0]
    for k in range(probs.shape[1]):
        on = pf[:, k] > lo
        runs, j = [], 0
        while j < n:
            if not on[j]:
                j += 1
                continue
            a = j
            while j < n and on[j]:
                j += 1
            if (pf[a:j, k] > hi).any():
                runs.append([a, j])
        merged = []
        for a, b in runs:
            if merged and a - merged[-1][1] <= min_gap:
                merged[-1][1] = b
            else:
                merged.append([a, b])
        for a, b in merged:
            if b - a < min_len:
                continue
            seg = probs[a:b, k]
            out["cls"].append(k); out["onset"].append(a); out["offset"].append(b)
            out["peak"].append(seg.max()); out["peak_frame"].append(a + int(np.argmax(seg)))
    res = {k: np.asarray(v, np.int32) for k, v in out.items() if k != "peak"}
    res["peak"] = np.asarray(out["peak"], np.float32)
    return res


def event_mask(ev, n_out, K):
    m = np.zeros((n_out, K), bool)
    for k, a, b in zip(ev["cls"], ev["onset"], ev["offset"]):
        m[a:b, k] = True
    return m
