"""The one selection walk behind the quiet-frame MVDR and the contrast SRP-PHAT, on the MI355X:
feature.event_quiet_frames and feature.event_contrast_frames on ONE table (tests/test_cpu_activity_rules.py: 2 recordings of
different length, 2 channels, hop 1024, twelve events of 1 to 5 output frames and three classes per recording, every one located
on all of its frames in direction 0), both guards 0, noise_exclude="same".  Each result equals its numpy reference for all
events, and over the events with onset tf >= search + 1 — whose candidates both rules test on the same samples — the two device
results are equal.  No sample is read: the entries take the lengths of the recordings alone.

The event loops of the two select kernels and of the activity kernel take a second trip only beyond 2^20 events; that is not
tested here or elsewhere."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import doa_ref  # noqa: E402
from test_cpu_activity_rules import HOP, MAX_FRAMES, N_CLASSES, SETTINGS, TFS, agree, not_vacuous, references, table  # noqa: E402

pytestmark = pytest.mark.gpu
C = 2


@pytest.fixture(scope="module")
def sed():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    import sed_crnn_amd as s
    return s


def _inputs(tf):
    """-> (clips, the located event table with cls on the device)"""
    clips, cols, at = [], {k: [] for k in ("onset", "offset", "peak_frame", "rec", "cls", "dir", "loc_frames")}, 0
    for r, (n, rows, cls, loc) in enumerate(table(tf)):
        clips += [(at + c * n, n) for c in range(C)]
        at += C * n
        for (on, off, peak), k, lf in zip(rows, cls, loc):
            for key, v in zip(cols, (on, off, peak, r, k, 0, lf)):
                cols[key].append(v)
    return clips, {k: torch.tensor(v, dtype=torch.int32, device="cuda") for k, v in cols.items()}


@pytest.mark.parametrize("tf", TFS)
def test_the_two_entries_agree_where_their_windows_coincide_and_each_equals_its_reference(sed, tf):
    from sed_crnn_amd import feature
    pos = doa_ref.line(C, 0.06)
    grid = sed.DirectionGrid.ring(8)
    clips, ev = _inputs(tf)
    compared = chosen = 0
    for S, N, M in SETTINGS:
        mv = sed.MVDR(noise_blocks=N, noise_guard=0, noise_select="quiet", noise_search=S, noise_min=M, noise_exclude="same")
        quiet = feature.event_quiet_frames(clips, C, ev, tf, sed.DOA(pos, grid, max_frames=MAX_FRAMES), mv, N_CLASSES, hop=HOP)
        ct = sed.DOA(pos, grid, max_frames=MAX_FRAMES, contrast=sed.Contrast(frames=N, search=S, guard=0, min_frames=M))
        bg = feature.event_contrast_frames(clips, C, ev, tf, ct, N_CLASSES, hop=HOP)
        qf, qs, cf, cs, take = references(tf, S, N, M)
        got = [v.cpu().numpy() for v in (quiet["noise_frames"], quiet["noise_sel"], bg["bg_frames"], bg["bg_sel"])]
        for name, g, want in zip(("noise_frames", "noise_sel", "bg_frames", "bg_sel"), got, (qf, qs, cf, cs)):
            assert g.dtype == np.int32 and g.shape == want.shape and np.array_equal(g, want), (S, N, M, name, g.tolist(), want.tolist())
        c, k = agree(*got, take)
        print(f"tf {tf}, search {S}, N {N}, min {M}: {c} compared events, {k} with a selection")
        compared, chosen = compared + c, chosen + k
    assert not_vacuous(compared, chosen), (compared, chosen)
