"""The GRU dispatch (csrc/gru.hip: gru_bt + GRU_DISPATCH, reported by sed_gru_seq_variant) against the case table of
tests/test_gpu_gru_variants.py: every (batch tile, weight placement) class a call can reach must have a GPU case, so moving a
threshold or adding an instantiation fails here instead of silently losing coverage.  Host only, no GPU needed."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_gpu_gru_variants as gv  # noqa: E402

from sed_crnn_amd import ops  # noqa: E402

BATCHES = (1, 255, 256, 511, 512, 4096)


def test_case_table_covers_every_reachable_variant_class():
    reachable = {}
    for H in range(4, 341, 4):
        for B in BATCHES:
            reachable.setdefault(ops.gru_seq_variant(B, H), (B, H))
    covered = {cls for _, _, cls in gv.CASE_LIST}
    missing = {cls: first for cls, first in reachable.items() if cls not in covered}
    assert not missing, f"variant classes (bt, hreg, hlds) without a GPU case, with a (B, H) that reaches each: {missing}"
    # the table names nothing that cannot be reached either (a stale row would test a class twice and claim another)
    assert covered <= set(reachable), covered - set(reachable)
    # about twenty instantiations: 4 register sizes x 3 tiles, <128, 1|2>, streamed x 3 tiles, the hybrid
    assert len(reachable) == 18


def test_every_case_runs_the_class_its_row_names():
    for group, (B, T, H), cls in gv.CASE_LIST:
        assert ops.gru_seq_variant(B, H) == cls, (group, B, T, H)
        bt, hreg, hlds = cls
        assert bt in (1, 2, 4) and (hreg in (0, H) or hlds > 0)
    # the rows the issue's table lists under each heading are of that heading's kind
    for (B, T, H), (bt, hreg, hlds) in gv.CASES["tile 2, registers"]:
        assert bt == 2 and hreg == H
    for (B, T, H), (bt, hreg, hlds) in gv.CASES["tile 4, registers"]:
        assert bt == 4 and hreg == H
    for (B, T, H), (bt, hreg, hlds) in gv.CASES["streamed"]:
        assert bt in (2, 4) and hreg == 0 and hlds == 0
    assert {cls[0] for _, cls in gv.CASES["streamed"]} == {2, 4}
    for (B, T, H), (bt, hreg, hlds) in gv.CASES["hybrid"]:
        assert bt == 1 and 0 < hreg < H and hlds > 0 and hreg + hlds < H


def test_ragged_tiles_and_prefetch_edges_are_in_the_table():
    shapes = [s for _, s, _ in gv.CASE_LIST]
    classes = {s: c for _, s, c in gv.CASE_LIST}
    # a ragged last tile (B % tile != 0) for tile 2 and tile 4, register-resident and streamed
    for bt, reg in ((2, True), (4, True), (2, False), (4, False)):
        assert any(classes[s][0] == bt and (classes[s][1] > 0) == reg and s[0] % bt for s in shapes), (bt, reg)
    # sequences shorter than the prefetch distance (T = 1, 2) on a two-ahead, the one-ahead <0,4> and the hybrid variant
    assert any(s[1] == 1 and classes[s] == (4, 0, 0) for s in shapes)
    assert any(s[1] <= 2 and classes[s][0] == 2 for s in shapes)
    assert any(s[1] == 1 and classes[s][2] > 0 for s in shapes) and any(s[1] == 2 and classes[s][2] > 0 for s in shapes)


def test_variant_query_rejects_sizes_the_kernels_reject():
    from sed_crnn_amd._lib import SedHipError
    for B, H in ((4, 6), (4, 344), (0, 32)):
        with pytest.raises(SedHipError):
            ops.gru_seq_variant(B, H)
