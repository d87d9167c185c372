"""Where the quiet-frame MVDR and the contrast SRP-PHAT must pick the same frames, on the two numpy
references (tests/mvdr_quiet_ref.py, tests/contrast_ref.py).  No GPU.

Both rules are one walk (csrc/activity_shared.h) over the candidates q = 0 .. S-1 of an event: candidate q exists iff
origin - lead - q stride >= 0 and is tested on the samples [origin - before - q stride, origin + after - q stride), the low end
clamped to 0, against the output frames lo // H .. min(ceil(hi / H), L) - 1 of the activity mask; the first N eligible ones are
kept, none where they are fewer than M, and listed in descending q:

                 origin                   stride  before          after  lead
    quiet MVDR   s0                       1024    (2 G + 2) 1024  0      (G + 2) 1024
    contrast     (onset tf - G - 1) hop   hop     1024            1024   0

At hop = 1024, both guards 0 and noise_exclude = "same", an event that is no longer than max_frames (s0 = onset tf hop), fully
located and has a = onset tf >= S + 1 is tested on [(a - 2 - q) 1024, (a - q) 1024) by both rows, and all S candidates exist in
both: the two selections are equal.  Over the table below (2 recordings x 12 events, three settings) that is 61 compared
event-settings cases at time factor 1, 51 of them with a non-empty selection, and 72 at time factor 8, 64 of them non-empty.
tests/test_gpu_activity_shared.py asks the same of the two device entries on the same table."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import contrast_ref  # noqa: E402
import mvdr_quiet_ref  # noqa: E402

from sed_crnn_amd.localize import event_frames  # noqa: E402

HOP, B, MAX_FRAMES, N_CLASSES, EVENTS = 1024, 1024, 40, 3, 12
FRAMES, TAILS = (190, 120), (300, 777)              # output frames of the two recordings and their ragged tails, in samples
TFS = (1, 8)
SETTINGS = [(8, 3, 1), (70, 33, 2), (16, 16, 16)]   # (search, N, min): 70 crosses the 64-candidate batch, 33 the 32-entry chunk, 16 of 16 the cut


def table(tf, seed=5):
    """-> [(n samples, rows [(onset, offset, peak)], cls, loc_frames)] per recording: twelve events of 1 to 5 output frames and
    three classes each, every one located on all of its frames (at most 5 tf <= MAX_FRAMES)"""
    rng = np.random.default_rng(seed + tf)
    recs = []
    for frames, tail in zip(FRAMES, TAILS):
        n = frames * tf * HOP + tail
        on = rng.integers(0, frames, EVENTS)
        dur = rng.integers(1, 6, EVENTS)
        rows = [(int(a), int(a + d), int(a + d // 2)) for a, d in zip(on, dur)]
        cls = [int(k) for k in rng.integers(0, N_CLASSES, EVENTS)]
        loc = [(lambda f: f[1] - f[0])(event_frames(*r, tf, 1 + n // HOP, MAX_FRAMES)) for r in rows]
        assert all(0 < lf <= MAX_FRAMES for lf in loc)
        recs.append((n, rows, cls, loc))
    return recs


def references(tf, S, N, M):
    """-> (quiet frames [E], quiet sel [E, N], contrast frames [E], contrast sel [E, N], compared [E]) over both recordings"""
    import sed_crnn_amd as sed
    ct = sed.Contrast(frames=N, search=S, guard=0, min_frames=M)
    out = [[], [], [], [], []]
    for n, rows, cls, loc in table(tf):
        q = mvdr_quiet_ref.frames_of(rows, cls, [0] * len(rows), loc, tf, n, HOP, MAX_FRAMES, N, 0, S, M, "same", N_CLASSES)
        bg, sel = contrast_ref.frames_of(rows, cls, n, tf, HOP, MAX_FRAMES, ct, N_CLASSES)
        for k, v in enumerate((q["noise_frames"], q["noise_sel"], bg, sel, np.asarray([r[0] * tf >= S + 1 for r in rows]))):
            out[k].append(v)
    return tuple(np.concatenate(v) for v in out)


def agree(qf, qs, cf, cs, compared):
    """the two selections are equal over the compared events -> (how many those are, how many of them have a selection)"""
    assert np.array_equal(qf[compared], cf[compared]) and np.array_equal(qs[compared], cs[compared])
    return int(compared.sum()), int((qf[compared] > 0).sum())


def walk(mask, H, origin, stride, before, after, lead, N, S, M, excl):
    """the one walk, as the header states it -> (count, sel [N])"""
    L, kept = len(mask), []
    for q in range(S):
        at = origin - q * stride
        if at - lead < 0:
            break
        lo, hi = max(at - before, 0), at + after
        if not any(int(mask[t]) & excl for t in range(lo // H, min(-(-hi // H), L))):
            kept.append(q)
    kept = kept[:N]
    sel = np.full(N, -1, np.int32)
    if len(kept) < M:
        return 0, sel
    sel[:len(kept)] = kept[::-1]
    return len(kept), sel


@pytest.mark.parametrize("tf", TFS)
def test_each_rule_is_the_walk_with_its_row_of_the_table(tf):
    """for every event, and with guards that are not 0 too"""
    import sed_crnn_amd as sed
    for S, N, M in SETTINGS:
        for G in (0, 2):
            ct =sed.Contrast(frames=N, search=S, guard=G, min_frames=M)
            for n, rows, cls, loc in table(tf):
                H = tf * HOP
                mask = mvdr_quiet_ref.activity(rows, cls, n, H, N_CLASSES)
                q = mvdr_quiet_ref.frames_of(rows, cls, [0] * len(rows), loc, tf, n, HOP, MAX_FRAMES, N, G, S, M, "same", N_CLASSES)
                bg, sel = contrast_ref.frames_of(rows, cls, n, tf, HOP, MAX_FRAMES, ct, N_CLASSES)
                for e, (r, k) in enumerate(zip(rows, cls)):
                    s0 = r[0] * tf * HOP                                     # (no event is longer than MAX_FRAMES)
                    cnt, want = walk(mask, H, s0, B, (2 * G + 2) * B, 0, (G + 2) * B, N, S, M, 1 << k)
                    assert (q["noise_frames"][e], q["noise_sel"][e].tolist()) == (cnt, want.tolist()), ("quiet", S, N, M, G, e)
                    cnt, want = walk(mask, H, (r[0] * tf - G - 1) * HOP, HOP, 1024, 1024, 0, N, S, M, 1 << k)
                    assert (bg[e], sel[e].tolist()) == (cnt, want.tolist()), ("contrast", S, N, M, G, e)


def not_vacuous(compared, chosen):
    """at least a quarter of the compared events have a selection, and at least one has none"""
    return 4 * chosen >= compared and chosen < compared


@pytest.mark.parametrize("tf,figures", [(1, (61, 51)), (8, (72, 64))])
def test_the_two_rules_coincide_where_their_windows_do(tf, figures):
    compared = chosen = 0
    for S, N, M in SETTINGS:
        c, k = agree(*references(tf, S, N, M))
        print(f"tf {tf}, search {S}, N {N}, min {M}: {c} compared events, {k} with a selection")
        compared, chosen = compared + c, chosen + k
    assert not_vacuous(compared, chosen) and (compared, chosen) == figures   # the docstring's
