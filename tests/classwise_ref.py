"""Class-wise decoder settings restated for the tests by COMPOSING the existing references — detect_ref, stream_ref
and tune_ref are used as they are, nothing of them is repeated here.

Definition: class k's events under class-wise settings are the class-k events of ``detect_ref.decode(probs, **settings[k])``.
``detect_ref.decode`` treats the columns of a track independently, so that is the decode of column k alone, relabelled k.

Streaming rule: ONE frontier per feed.  Filtered frame g of every class is decided once track frame ``g + R`` is final,
``R = max_k median_k // 2``; a pending event [a, b) of class k is emitted in the first step in which more than
``b + min_gap_k`` frames are decided and no run of class k that began at or before ``b + min_gap_k`` is still open.
``stream_ref.DecodeRef`` decides frame g once it HOLDS track frame ``g + median // 2``; handing class k's one-class DecodeRef
the final rows ``R - median_k // 2`` frames late (all of them at the end) therefore gives exactly the common frontier, with the
emission rule, the peaks and ``active()`` unchanged.
"""
import numpy as np

import detect_ref
import stream_ref
import tune_ref

EVENT_KEYS = ("cls", "onset", "offset", "peak", "peak_frame")

# the checked example, K = 6: (hi, lo, median, min_gap, min_len)
EXAMPLE = [dict(hi=hi, lo=lo, median=m, min_gap=g, min_len=n) for hi, lo, m, g, n in
           ((.5, .5, 1, 0, 1), (.6, .4, 31, 17, 5), (.45, .45, 3, 1, 2), (.55, .5, 15, 3, 1), (.5, .42, 7, 0, 9), (.58, .52, 1, 40, 1))]


def smooth(rng, n, K, scale=0.15):
    """the track generator of test_gpu_tune (``_smooth``), copied: values in [0.361, 0.639]"""
    walk = np.cumsum(rng.standard_normal((n, K)) * scale, 0)
    return ((1 / (1 + np.exp(-np.sin(walk)))) * 0.6 + 0.2).astype(np.float32)


def det_kwargs(settings):
    """K dicts in detect_ref's names (hi, lo, ...) -> the EventDetector / with_decoder keyword arguments, as K-lists"""
    return dict(threshold=[s["hi"] for s in settings], low=[s["lo"] for s in settings], median=[s["median"] for s in settings],
                min_gap=[s["min_gap"] for s in settings], min_len=[s["min_len"] for s in settings])


def no_events():
    ev = {k: np.zeros(0, np.int32) for k in EVENT_KEYS}
    ev["peak"] = np.zeros(0, np.float32)
    return ev


def _cat(parts):
    """per-class event dicts, class by class -> one dict sorted by (class, onset)"""
    if not parts:
        return no_events()
    return {k: np.concatenate([p[k] for p in parts]).astype(np.float32 if k == "peak" else np.int32) for k in EVENT_KEYS}


def class_events(probs, k, setting):
    """the class-k events of ``detect_ref.decode(probs, **setting)``"""
    ev = detect_ref.decode(np.asarray(probs, np.float32)[:, k:k + 1], **setting)
    ev["cls"] = np.full_like(ev["cls"], k)
    return ev


def decode(probs, settings):
    """probs [n_out, K], settings: K dicts (lo, hi, median, min_gap, min_len) -> events sorted by (class, onset)"""
    assert np.asarray(probs).shape[1] == len(settings)
    return _cat([class_events(probs, k, s) for k, s in enumerate(settings)])


def only(ev, k):
    sel = ev["cls"] == k
    return {n: v[sel] for n, v in ev.items() if n in EVENT_KEYS}


def pairs(ev):
    return list(zip(ev["onset"].tolist(), ev["offset"].tolist()))


def example_is_discriminating(probs, settings=EXAMPLE, lo=4, hi=178):
    """the two properties of the checked example: every class has lo..hi events under its own row, and for every pair j != k
    class k's events under row j differ from those under row k — so a kernel that applies the wrong row is caught"""
    K = len(settings)
    mine = [pairs(class_events(probs, k, settings[k])) for k in range(K)]
    if not all(lo <= len(m) <= hi for m in mine):
        return False
    return all(pairs(class_events(probs, k, settings[j])) != mine[k] for k in range(K) for j in range(K) if j != k)


class ClasswiseDecodeRef:
    """``stream_ref.DecodeRef`` per class behind one frontier: final track rows in, each step's events out"""

    def __init__(self, settings):
        self.settings = [dict(s) for s in settings]
        self.K = len(settings)
        self.R = max(s["median"] for s in settings) // 2
        self.reset()

    def reset(self):
        self.refs = [stream_ref.DecodeRef(1, **s) for s in self.settings]
        self.rows = np.zeros((0, self.K), np.float32)
        self.given = [0] * self.K

    @property
    def decided(self):
        return max(0, self.rows.shape[0] - self.R)

    def step(self, rows, end=False):
        self.rows = np.concatenate([self.rows, np.asarray(rows, np.float32).reshape(-1, self.K)])
        n, parts = self.rows.shape[0], []
        for k, (ref, s) in enumerate(zip(self.refs, self.settings)):
            upto = n if end else max(self.given[k], n - (self.R - s["median"] // 2))
            ev = ref.step(self.rows[self.given[k]:upto, k:k + 1], end)
            self.given[k] = upto
            assert end or ref.decided == self.decided, "one frontier per feed"
            ev["cls"] = np.full_like(ev["cls"], k)
            parts.append(ev)
        if end:
            self.reset()
        return _cat(parts)

    def active(self):
        """[(cls, onset)] as ``DecodeRef.active``, every class merging with its own min_gap"""
        return [(k, a) for k, ref in enumerate(self.refs) for _, a in ref.active()]


def score(probs, out_off, ref_lists, settings, **scoring):
    """[K, 6] counts of the class-wise decode: class k's row of ``tune_ref.sweep`` with setting k (detector key names)"""
    K = len(settings)
    table = tune_ref.sweep(probs, out_off, ref_lists, settings, **scoring)          # [K settings, K classes, 6]
    return np.stack([table[k, k] for k in range(K)])
