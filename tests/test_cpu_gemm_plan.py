"""The shapes test_gpu_gemm_tiles.py runs really are on the tile, the FULL / guarded path, the K-loop phase and the split-K rule
their rows claim: every row of gemm_cases.py is held against sed_gemm_f32_plan (the plan the launches read), and the table as a
whole must cover the five tiles x {all-FULL, ragged} and the three split rules on the 64x64 tile and on a larger one.  No GPU."""
import pytest

import gemm_cases as gc  # noqa: E402


@pytest.fixture(scope="module")
def ops():
    from sed_crnn_amd import ops as o
    return o


def _rule(ops, M, N, K, policy):
    """which split rule a (shape, policy) is under, from the query and the rules' own conditions"""
    splits = [ops.gemm_plan(M, N, K, p)[2] for p in (0, 1, 2)]
    assert splits[0] == 1, "policy 0 never splits"
    if splits[policy] == 1:
        return None
    small_output = gc.cdiv(M, 64) * gc.cdiv(N, 64) < 96 and K >= 1024
    if small_output:
        assert splits[1] == splits[2]
        return "small"
    assert splits[policy] == 2
    if policy == 1:
        assert K >= 4096 and N <= 1024
        return "fwd2"
    return "wgrad2"


@pytest.mark.parametrize("name", gc.NAMES)
def test_row_is_in_the_regime_it_claims(ops, name):
    c = gc.case(name)
    (M, N, K), policy, want = c["shape"], c["policy"], c["claims"]
    bm, bn, splits, k_len = ops.gemm_plan(M, N, K, policy)
    assert (bm, bn) in gc.TILES
    facts = dict(tile=(bm, bn), splits=splits, k_len=k_len, nsteps=gc.nsteps(K, splits, k_len),
                 mult8=(gc.cdiv(M, bm) * gc.cdiv(N, bn)) % 8 == 0, rule=_rule(ops, M, N, K, policy))
    classes = gc.full_classes(M, N, K, bm, bn, splits, k_len)
    facts["full"] = classes[0] if len(set(classes)) == 1 else classes
    for key, claim in want.items():
        assert facts[key] == claim, f"row {name} ({M}x{N}x{K}, {gc.POLICY_NAME[policy]}): {key} is {facts[key]}, the row claims {claim}"
    # the tile does not depend on the entry, and policy 0 runs the row in one slice
    for p in (0, 1, 2):
        assert ops.gemm_plan(M, N, K, p)[:2] == (bm, bn), (name, p)
    assert ops.gemm_plan(M, N, K, 0)[2:] == (1, K)
    if name in gc.OTHER_POLICY:
        other = 2 if policy == 1 else 1
        assert ops.gemm_plan(M, N, K, other)[2:] == gc.OTHER_POLICY[name], (name, other)
    # the exactness precondition of the integer test: operands, bias and prior out in [-3, 3]
    assert gc.exactness_bound(K) == 9 * K + 6 < 2 ** 24
    # a call costs a fraction of a millisecond: at most 26 GFLOP (the boundary row of the forward rule)
    assert 2 * M * N * K <= 26e9


@pytest.mark.parametrize("name", gc.NAMES)
def test_workspace_query_is_the_larger_of_the_two_split_plans(ops, name):
    M, N, K = gc.case(name)["shape"]
    most = max(ops.gemm_plan(M, N, K, p)[2] for p in (1, 2))
    assert ops.lib().sed_gemm_f32_workspace_bytes(M, N, K) == (4 * M * N * most if most > 1 else 0)
    # every slice is non-empty, starts on a K-step and the slices cover K
    for p in (1, 2):
        _, _, splits, k_len = ops.gemm_plan(M, N, K, p)
        assert (splits == 1 and k_len == K) or (k_len % gc.GM_BK == 0 and (splits - 1) * k_len < K <= splits * k_len)


def test_the_table_covers_every_tile_path_and_split_rule():
    cover = {(c["claims"]["tile"], c["claims"]["full"]) for c in gc.CASES if c["claims"]["splits"] == 1}
    want = {(t, f) for t in gc.TILES for f in ("all", "none")}
    assert want <= cover, f"tile x path without an unsplit row: {sorted(want - cover)}"
    # all-FULL rows of 1, 2 and 3 K-steps on every tile: the prologue alone, the two-step tail alone, one turn of the steady loop
    for t in gc.TILES:
        steps = {c["claims"]["nsteps"] for c in gc.CASES if c["claims"]["tile"] == t and c["claims"]["full"] == "all" and c["policy"] == 0}
        assert {(1,), (2,), (3,)} <= steps, (t, steps)
    for rule in ("small", "fwd2", "wgrad2"):
        tiles = {c["claims"]["tile"] for c in gc.CASES if c["claims"]["rule"] == rule}
        if rule == "small":
            assert tiles == {(64, 64)}               # the rule IS the 64x64 tile; its larger-output neighbours are the rows below
        else:
            assert (64, 64) in tiles and tiles - {(64, 64)}, (rule, tiles)
    # ... so every split row of a larger tile is listed, and all four larger tiles have one
    assert {gc.case(n)["claims"]["tile"] for n in gc.SPLIT_ROWS} == set(gc.TILES)
    # a launch whose slices take different paths, a short last slice, a tile count off the multiple of 8 on a small and a large tile
    assert any("some" in c["claims"]["full"] for c in gc.CASES if isinstance(c["claims"]["full"], tuple))
    assert any(len(set(c["claims"]["nsteps"])) > 1 for c in gc.CASES)
    assert {c["claims"]["tile"] for c in gc.CASES if not c["claims"]["mult8"]} >= {(128, 128), (64, 128), (64, 64)}
    # the K >= 1024 threshold of the small-output rule and the N <= 1024 boundary of the forward rule, from both sides
    assert gc.case("small_k1024")["claims"]["splits"] > 1 and gc.case("small_k1023_not_split")["claims"]["splits"] == 1
    assert gc.case("wgrad2_128x96_not_fwd2")["shape"][1] > 1024 and gc.OTHER_POLICY["wgrad2_128x96_not_fwd2"][0] == 1
    assert gc.case("fwd2_128x64")["shape"][1] == 1024
    assert len(set(gc.NAMES)) == len(gc.NAMES)


def test_small_output_threshold_and_forward_rule_boundary(ops):
    assert ops.gemm_plan(64, 64, 1024, 1) == (64, 64, 8, 128) and ops.gemm_plan(64, 64, 1023, 1) == (64, 64, 1, 1023)
    assert ops.gemm_plan(2048, 1536, 4096, 2)[2:] == (2, 2048) and ops.gemm_plan(2048, 1536, 4096, 1)[2:] == (1, 4096)
    # the forward rule looks at N and K alone: a chunk of a policy-1 row keeps its slices from 384 rows up, whatever tile it
    # gets (with 16 column blocks the small-output rule takes over at 5 row blocks, 320 rows)
    for name in gc.FWD2_ROWS:
        M, N, K = gc.case(name)["shape"]
        want = ops.gemm_plan(M, N, K, 1)[2:]
        assert ops.gemm_plan(384, N, K, 1)[2:] == want and ops.gemm_plan(M - 1, N, K, 1)[2:] == want
        assert ops.gemm_plan(320, N, K, 1)[2] > 2
    # a 64 x 64 block of any row runs on the 64x64 tile in one slice under policy 0
    assert all(ops.gemm_plan(64, 64, K, 0) == (64, 64, 1, K) for K in (32, 70, 2048, 4100))
    assert all(ops.gemm_plan(m, n, 70, 0)[:2] == (64, 64) for m in (1, 36, 64) for n in (1, 52, 64))


def test_plan_query_rejects_bad_arguments(ops):
    from sed_crnn_amd._lib import SedHipError
    for args in ((0, 4, 4, 0), (4, 0, 4, 0), (4, 4, 0, 0), (4, 4, 4, 3), (4, 4, 4, -1)):
        with pytest.raises(SedHipError):
            ops.gemm_plan(*args)


def test_xcd_remap_visits_every_tile_once():
    """the restated remap (the GPU test's failure report relies on it) is a permutation for every grid of the table, and hands
    each XCD a contiguous row-major run"""
    grids = {(gc.cdiv(c["shape"][1], c["claims"]["tile"][1]), gc.cdiv(c["shape"][0], c["claims"]["tile"][0])) for c in gc.CASES}
    for gx, gy in sorted(grids):
        tiles = gc.xcd_remap(gx, gy)
        assert sorted(tiles) == [(y, x) for y in range(gy) for x in range(gx)], (gx, gy)
        for xcd in range(8):
            run = [y * gx + x for y, x in tiles[xcd::8]]
            assert run == list(range(run[0], run[0] + len(run))) if run else True


def test_differing_blocks_tells_a_tile_from_a_quadrant_from_a_k_step():
    import torch
    ref = torch.arange(200 * 300, dtype=torch.float32).view(200, 300)
    assert gc.differing_blocks(ref.clone(), ref) == []
    got = ref.clone()
    got[128:200, 128:256] = float("nan")                     # a 128-wide tile on the ragged lower edge, never written
    blocks = gc.differing_blocks(got, ref)
    assert blocks == [(r, c) for r in (4, 5, 6) for c in (4, 5, 6, 7)]
    assert "row-blocks [4, 5, 6], col-blocks [4, 5, 6, 7]" in gc.describe_blocks(blocks, 200, 300)
    got = ref.clone()
    got[32:64, 64:96] += 1                                   # one wave quadrant
    assert gc.differing_blocks(got, ref) == [(1, 2)]
    assert "all of them" in gc.describe_blocks(gc.differing_blocks(ref + 1, ref), 200, 300)
