"""The case table of the fp32 GEMM (csrc/gemm.hip), shared by test_cpu_gemm_plan.py (which asks sed_gemm_f32_plan and proves
that every row is in the regime it claims) and test_gpu_gemm_tiles.py (which runs the rows).  The plan is never restated here:
the library's query is the authority, and a retuned gemm_plan fails the CPU test with the name of the row that moved.  What IS
restated is what the kernel does with a plan: the FULL predicate of gemm_f32_k, the K loop's step count and the XCD remap.

A row: name, (M, N, K), the policy it is about (0 = gemm, 1 = gemm_ws, 2 = gemm_ws(wgrad=True)) and its claims:
  tile    (bm, bn) of the block tile
  splits  number of K-slices under the row's policy, k_len the k extent of a slice
  full    "all" / "some" / "none": which workgroups take the unguarded FULL path; a string holds for all four layouts, a 4-tuple
          gives the class per layout in the order of LAYOUTS (the leading stride of an operand decides whether it is read in
          float4, and FULL needs both)
  nsteps  K-steps of 32 per slice (a tuple, one entry per slice)
  mult8   whether the tile count is a multiple of 8 (the XCD remap deals q or q + 1 tiles to an XCD otherwise)
  rule    None, or the split rule that applies: "small" (small output), "fwd2" (policy 1, K >= 4096 and N <= 1024), "wgrad2"
"""
import math

GM_BK = 32
TILES = ((128, 128), (128, 96), (128, 64), (64, 128), (64, 64))
# (ta, tb): A stored [K][M] (contiguous along i) / B stored [N][K] (contiguous along k), as test_gemm_f32_layouts builds them
LAYOUTS = ((False, False), (False, True), (True, False), (True, True))
POLICY_NAME = {0: "gemm", 1: "gemm_ws", 2: "gemm_ws(wgrad)"}


def cdiv(a, b):
    return -(-a // b)


def _row(name, M, N, K, policy, tile, full, nsteps, mult8, splits=1, k_len=None, rule=None):
    return dict(name=name, shape=(M, N, K), policy=policy,
                claims=dict(tile=tile, splits=splits, k_len=K if k_len is None else k_len, full=full, nsteps=nsteps, mult8=mult8, rule=rule))


def _tile_rows():
    rows = []
    # all-FULL: every extent a multiple of its tile, K of 1, 2 and 3 steps (prologue only, the two-step tail only, one turn of
    # the steady-state loop); ragged: M and N off the tile, K = 70 (not a multiple of 4: three steps, the last of 6)
    for tile, (Mf, Nf), (Mr, Nr), m8f, m8r in (((128, 128), (2048, 2048), (1700, 2100), True, False),      # 256 / 238 tiles
                                               ((128, 96), (2048, 1536), (2000, 1500), True, True),
                                               ((128, 64), (2048, 1024), (2040, 1000), True, True),
                                               ((64, 128), (960, 2176), (950, 2170), False, False),       # 255 tiles
                                               ((64, 64), (128, 128), (130, 70), False, False)):
        for K in (32, 64, 96):
            rows.append(_row(f"full_{tile[0]}x{tile[1]}_k{K}", Mf, Nf, K, 0, tile, "all", (K // 32,), m8f))
        rows.append(_row(f"ragged_{tile[0]}x{tile[1]}", Mr, Nr, 70, 0, tile, "none", (3,), m8r))
    return rows


CASES = _tile_rows() + [
    # K a multiple of 4 but not of 32 with ragged M, N: the float4 reads of the guarded path next to the edge (leading stride 68)
    _row("ragged_128x128_k68", 1700, 2100, 68, 0, (128, 128), "none", (3,), False),
    # vectors (some operand has both strides 1: "prefer k-contiguous")
    _row("vector_row", 1, 300, 70, 0, (64, 64), "none", (3,), False),
    _row("vector_col", 300, 1, 70, 0, (64, 64), "none", (3,), False),
    _row("vector_k1", 200, 200, 1, 0, (64, 64), "none", (1,), True),
    # small-output rule (policies 1 and 2 alike; the rows run under both)
    _row("small_13_slices", 100, 30, 2000, 1, (64, 64), "none", (5,) * 12 + (3,), False, splits=13, k_len=160, rule="small"),
    _row("small_16_slices", 96, 32, 2048, 1, (64, 64), "none", (4,) * 16, False, splits=16, k_len=128, rule="small"),
    # (96 x 32 has no whole 64 x 64 tile, so its workgroups are all guarded; the all-FULL many-slice row is 128 x 64)
    _row("small_all_full", 128, 64, 2048, 1, (64, 64), "all", (4,) * 16, False, splits=16, k_len=128, rule="small"),
    _row("small_k1024", 64, 64, 1024, 1, (64, 64), "all", (4,) * 8, False, splits=8, k_len=128, rule="small"),
    _row("small_k1023_not_split", 64, 64, 1023, 1, (64, 64), "none", (32,), False),
    # forward two-slice rule (policy 1)
    _row("fwd2_64x64", 384, 1024, 4096, 1, (64, 64), "all", (64, 64), True, splits=2, k_len=2048, rule="fwd2"),
    # M = 390: A stored [K][M] has a leading stride that is no multiple of 4, so only the layouts with A stored [M][K] read it in
    # float4; there the first slice (2080) runs its interior tiles FULL and the second (2020) is guarded, in one launch
    _row("fwd2_ragged", 390, 1000, 4100, 1, (64, 64), ("some", "some", "none", "none"), (65, 64), True, splits=2, k_len=2080, rule="fwd2"),
    _row("fwd2_128x64", 2048, 1024, 4096, 1, (128, 64), "all", (64, 64), True, splits=2, k_len=2048, rule="fwd2"),
    # weight-gradient two-slice rule (policy 2)
    _row("wgrad2_64x64", 1024, 1024, 2048, 2, (64, 64), "all", (32, 32), True, splits=2, k_len=1024, rule="wgrad2"),
    # K = 2050: an operand stored along k has leading stride 2050, no float4; with both stored along m / n the first slice (1056)
    # runs its interior tiles FULL and the second (994) guarded
    _row("wgrad2_ragged_128x64", 1000, 1100, 2050, 2, (128, 64), ("none", "none", "some", "none"), (33, 32), True, splits=2, k_len=1056,
         rule="wgrad2"),
    _row("wgrad2_128x128", 2048, 2048, 2048, 2, (128, 128), "all", (32, 32), True, splits=2, k_len=1024, rule="wgrad2"),
    _row("wgrad2_64x128", 960, 2176, 2048, 2, (64, 128), "all", (32, 32), False, splits=2, k_len=1024, rule="wgrad2"),
    # boundary of the forward rule: N > 1024 splits under policy 2 only
    _row("wgrad2_128x96_not_fwd2", 2048, 1536, 4096, 2, (128, 96), "all", (64, 64), True, splits=2, k_len=2048, rule="wgrad2"),
]
# what the OTHER split-capable policy does with a split row: {name: (splits, k_len)} (tile as claimed above)
OTHER_POLICY = {
    "small_13_slices": (13, 160), "small_16_slices": (16, 128), "small_all_full": (16, 128), "small_k1024": (8, 128),
    "small_k1023_not_split": (1, 1023),
    "fwd2_64x64": (1, 4096), "fwd2_ragged": (1, 4100), "fwd2_128x64": (2, 2048),
    "wgrad2_64x64": (1, 2048), "wgrad2_ragged_128x64": (1, 2050), "wgrad2_128x128": (1, 2048), "wgrad2_64x128": (1, 2048),
    "wgrad2_128x96_not_fwd2": (1, 4096),
}
NAMES = [c["name"] for c in CASES]
TILE_ROWS = [c["name"] for c in CASES if c["policy"] == 0]
SPLIT_ROWS = [c["name"] for c in CASES if c["claims"]["splits"] > 1]
LARGE_TILE_ROWS = [c["name"] for c in CASES if c["claims"]["tile"] != (64, 64)]
FWD2_ROWS = [c["name"] for c in CASES if c["claims"]["rule"] == "fwd2"]


def case(name):
    return next(c for c in CASES if c["name"] == name)


def exactness_bound(K):
    """largest |partial sum| of the integer test: operands, bias and the prior out in [-3, 3]"""
    return 9 * K + 6


def operand_vec(lead_stride, aligned=True):
    """gemm_impl's a_vec / b_vec: the operand may be read in float4 (16-byte aligned base, leading stride a multiple of 4)"""
    return bool(aligned and lead_stride % 4 == 0)


def layout_vecs(M, N, K, ta, tb, aligned=True):
    """(a_vec, b_vec) of a row whose operands are dense in layout (ta, tb)"""
    return operand_vec(M if ta else K, aligned), operand_vec(K if tb else N, aligned)


def slices(K, splits, k_len):
    """[(kb, k_end)] of the launch's blockIdx.z"""
    out = [(z * k_len, min((z + 1) * k_len, K)) for z in range(splits)]
    assert out[-1][1] == K and all(b > a for a, b in out)
    return out


def full_count(M, N, K, bm, bn, splits, k_len, a_vec, b_vec):
    """-> (workgroups on the FULL path, workgroups): the predicate of gemm_f32_k, `a_vec && b_vec && m0 + BM <= M && n0 + BN <= N
    && (K - kb) % 32 == 0` with K the end of the workgroup's slice"""
    total = cdiv(M, bm) * cdiv(N, bn) * splits
    if not (a_vec and b_vec):
        return 0, total
    interior = (M // bm) * (N // bn)
    return sum(interior for kb, ke in slices(K, splits, k_len) if (ke - kb) % GM_BK == 0), total


def full_class(M, N, K, bm, bn, splits, k_len, a_vec, b_vec):
    n, total = full_count(M, N, K, bm, bn, splits, k_len, a_vec, b_vec)
    return "all" if n == total else "some" if n else "none"


def full_classes(M, N, K, bm, bn, splits, k_len):
    return tuple(full_class(M, N, K, bm, bn, splits, k_len, *layout_vecs(M, N, K, ta, tb)) for ta, tb in LAYOUTS)


def nsteps(K, splits, k_len):
    return tuple(cdiv(ke - kb, GM_BK) for kb, ke in slices(K, splits, k_len))


def xcd_remap(gx, gy):
    """launch index -> (by, bx) of the tile it computes, as gemm_f32_k maps it: every XCD (launch index mod 8) walks a contiguous
    run of tiles in row-major order, the first total % 8 XCDs one tile more"""
    total = gx * gy
    q, rr = total >> 3, total & 7
    out = []
    for idx in range(total):
        xcd, seq = idx & 7, idx >> 3
        v = xcd * (q + 1) + seq if xcd < rr else rr * (q + 1) + (xcd - rr) * q + seq
        out.append((v // gx, v % gx))
    return out


def differing_blocks(got, ref, block=32):
    """the 32 x 32 blocks of two equally shaped 2-D tensors that differ anywhere (NaN counts as different), as sorted
    (row-block, col-block) pairs: a dropped 64- or 128-wide tile, a 32 x 32 wave quadrant and a K-step (every block) look different"""
    import torch
    bad = ~(got.double() == ref.double())
    M, N = bad.shape
    pad = torch.zeros(cdiv(M, block) * block, cdiv(N, block) * block, dtype=torch.bool, device=bad.device)
    pad[:M, :N] = bad
    blocks = pad.view(cdiv(M, block), block, cdiv(N, block), block).any(dim=3).any(dim=1)
    return [tuple(rc) for rc in blocks.nonzero().tolist()]


def describe_blocks(blocks, M, N, block=32, limit=48):
    total = cdiv(M, block) * cdiv(N, block)
    if not blocks:
        return "no block differs"
    head = f"{len(blocks)} of {total} 32x32 blocks differ (row-block, col-block): "
    if len(blocks) == total:
        return head + "all of them (a K-step or an operand, not a tile)"
    rows, cols = sorted({r for r, _ in blocks}), sorted({c for _, c in blocks})
    return head + f"{blocks[:limit]}{' ...' if len(blocks) > limit else ''}; row-blocks {rows[:limit]}, col-blocks {cols[:limit]}"


def tolerance(K, beta=0.0):
    """(atol, rtol) of test_gemm_f32_layouts for this kernel: 8e-5 sqrt(K), doubled where the prior out is added"""
    return 8e-5 * math.sqrt(K) * (2.0 if beta else 1.0), 1e-4
