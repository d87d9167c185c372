"""Independent numpy restatement of the streaming stitch and decode (sed_crnn_amd/stream.py, csrc/stream.hip),
written for clarity, not speed.  One ``step()`` per push, so that the TIMING of every emission is checkable, not only the union.

Frames are output frames.  With ``n_out`` output frames received, regular window w starts at ``w * hop_out`` and is complete iff
``w * hop_out + win_out <= n_out``; track frame j is final iff ``j < n_out - win_out``; filtered frame g is decided iff track
frame ``g + median // 2`` is final; at the end everything is final and the 'nearest' clamp applies on the right.  The decoder
keeps the WHOLE history and re-derives the events from it at every step: nothing here is a running value.
"""
import numpy as np


def regular_windows(n_out, win_out, hop_out):
    return (n_out - win_out) // hop_out + 1 if n_out >= win_out else 0


class StitchRef:
    """window logits in, final track rows out (float64; the mean adds the covering windows in increasing window order, like
    detect_ref.stitch)"""

    def __init__(self, K, win_out, hop_out, combine="mean", trim=0):
        self.K, self.win_out, self.hop_out, self.combine, self.trim = K, win_out, hop_out, combine, trim
        self.wins = []              # (start, sigmoid [len, K]) of the windows that can still cover a frame to come
        self.seen = 0               # windows so far
        self.n_out = 0
        self.final = 0

    def step(self, new_windows, n_out, end=False):
        """``new_windows``: the logits [len, K] of the windows that completed, in window order -> the newly final rows"""
        assert n_out >= self.n_out
        n_reg = regular_windows(n_out, self.win_out, self.hop_out)
        for lg in new_windows:
            lg = np.asarray(lg, np.float64)
            w = self.seen
            self.seen += 1
            if w < n_reg:
                start = w * self.hop_out
                assert lg.shape[0] == self.win_out
            else:                                               # the offline grid's last window: aligned to the end
                assert end and w == n_reg
                start = n_out - lg.shape[0]
                assert lg.shape[0] == min(self.win_out, n_out)
            self.wins.append((start, 1.0 / (1.0 + np.exp(-lg))))
        assert self.seen >= n_reg, "a complete window is missing"
        self.n_out = n_out
        upto = n_out if end else max(0, n_out - self.win_out)
        rows = np.zeros((upto - self.final, self.K))
        for j in range(self.final, upto):
            acc, cnt = None, 0
            for start, p in self.wins:
                lo = start + (self.trim if start > 0 else 0)
                right_edge = end and start + p.shape[0] == n_out    # before the end no window touches the recording's end
                hi = start + p.shape[0] - (0 if right_edge else self.trim)
                if lo <= j < hi:
                    v = p[j - start]
                    acc = v.copy() if acc is None else (acc + v if self.combine == "mean" else np.maximum(acc, v))
                    cnt += 1
            assert cnt > 0, "uncovered output frame"
            rows[j - self.final] = acc / cnt if self.combine == "mean" else acc
        self.final = upto
        self.wins = [(st, p) for st, p in self.wins if st + p.shape[0] > upto]
        return rows


class DecodeRef:
    """final track rows in, events out — each in the step the emission rule gives.  Comparisons in float32 like the kernel."""

    def __init__(self, K, lo=0.5, hi=0.5, median=1, min_gap=0, min_len=1):
        self.K, self.lo, self.hi = K, np.float32(lo), np.float32(hi)
        self.median, self.min_gap, self.min_len = median, min_gap, min_len
        self.track = np.zeros((0, K), np.float32)
        self.filt = np.zeros((0, K), np.float32)               # decided filtered frames
        self.ended = False
        self.scan_from = [0] * K                                # everything before it is emitted or can never be an event

    @property
    def decided(self):
        return self.filt.shape[0]

    def _runs(self, k):
        """(closed kept runs merged across gaps, the open run or None) over the decided frames from scan_from[k]"""
        a0 = self.scan_from[k]
        pf = self.filt[a0:, k]
        on = np.concatenate([[False], pf > self.lo, [False]])
        edges = np.flatnonzero(on[1:] != on[:-1])
        merged, open_run = [], None
        for a, b in zip(edges[0::2], edges[1::2]):
            kept = bool((pf[a:b] > self.hi).any())
            a, b = int(a) + a0, int(b) + a0
            if b == self.decided and not self.ended:
                open_run = (a, kept)
                break
            if not kept:
                continue
            if merged and a - merged[-1][1] <= self.min_gap:
                merged[-1][1] = b
            else:
                merged.append([a, b])
        return merged, open_run

    def step(self, rows, end=False):
        """the newly final track rows (and whether the stream ends) -> dict of arrays cls, onset, offset, peak, peak_frame of the
        events emitted by this step, sorted by (class, onset)"""
        rows = np.asarray(rows, np.float32).reshape(-1, self.K)
        self.track = np.concatenate([self.track, rows])
        self.ended = end
        n, r = self.track.shape[0], self.median // 2
        upto = n if end else max(0, n - r)
        new = np.zeros((max(0, upto - self.decided), self.K), np.float32)
        for g in range(self.decided, upto):
            idx = np.clip(np.arange(g - r, g + r + 1), 0, n - 1)  # before the end g + r < n: only the left edge clamps
            new[g - self.decided] = np.sort(self.track[idx], 0)[r]
        self.filt = np.concatenate([self.filt, new])
        G = self.decided
        out = {k: [] for k in ("cls", "onset", "offset", "peak", "peak_frame")}
        for k in range(self.K):
            merged, open_run = self._runs(k)
            for a, b in merged:
                final = end or (G > b + self.min_gap and not (open_run is not None and open_run[0] <= b + self.min_gap))
                if not final:
                    break
                self.scan_from[k] = b
                if b - a < self.min_len:
                    continue
                seg = self.track[a:b, k]
                out["cls"].append(k); out["onset"].append(a); out["offset"].append(b)
                out["peak"].append(seg.max()); out["peak_frame"].append(a + int(np.argmax(seg)))
        res = {k: np.asarray(v, np.int32) for k, v in out.items() if k != "peak"}
        res["peak"] = np.asarray(out["peak"], np.float32)
        return res

    def active(self):
        """[(cls, onset)] of the runs that are open and known to be kept (the pending event's onset when they will merge)"""
        self.ended = False
        out = []
        for k in range(self.K):
            merged, open_run = self._runs(k)
            if open_run is None or not open_run[1]:
                continue
            a = open_run[0]
            if merged and a - merged[-1][1] <= self.min_gap:
                a = merged[-1][0]
            out.append((k, a))
        return out


class StreamRef:
    """one stream: StitchRef then DecodeRef.  ``step(new_windows, n_out, end, rows=None)``: with ``rows`` the decoder runs on
    those (e.g. the float32 rows of the kernel under test) instead of the float64 stitch, so that events compare exactly."""

    def __init__(self, K, win_out, hop_out, combine="mean", trim=0, lo=0.5, hi=0.5, median=1, min_gap=0, min_len=1):
        self.args = (K, win_out, hop_out, combine, trim, lo, hi, median, min_gap, min_len)
        self.reset()

    def reset(self):
        K, win_out, hop_out, combine, trim, lo, hi, median, min_gap, min_len = self.args
        self.stitch = StitchRef(K, win_out, hop_out, combine, trim)
        self.decode = DecodeRef(K, lo, hi, median, min_gap, min_len)

    def step(self, new_windows, n_out, end=False, rows=None):
        """-> (events of this step, the newly final float64 rows, final frames after the step).  After ``end`` the stream
        restarts at frame 0."""
        mine = self.stitch.step(new_windows, n_out, end)
        ev = self.decode.step(mine if rows is None else rows, end)
        final = self.stitch.final
        if end:
            self.reset()
        return ev, mine, final
