"""gemm_f32_k (csrc/gemm.hip) on every block tile, operand layout, FULL / guarded path and split-K rule gemm_plan can pick, at
kernel level: the rows of gemm_cases.py (test_cpu_gemm_plan.py proves each is in the regime it claims), each in all four
layouts and through all three entries, against the float64 product.

  a. integers in [-3, 3]: every partial sum is below 2^24, so every order of summation, the split slabs and their sum are
     exact and the result must EQUAL float64 - with out pre-filled with NaN (a tile the XCD remap never visits) and with
     beta = 1 (a tile visited twice);
  b. N(0,1) values at the tolerance test_gemm_f32_layouts uses for this kernel, the observed error printed per row;
  c. one order of summation whatever the tile: the layouts agree bit for bit, a 64 x 64 block run as its own call (64x64 tile)
     equals the same block of the large-tile call, and a row chunk of a forward two-slice call equals its rows of the whole;
  d. the split-K plumbing: bias through the vector and the scalar branch of the reduction, out as a column block, a workspace
     of exactly the queried size in front of a guard, two calls with different workspace contents;
  e. operands one float off alignment and an output block at an odd column;
  f. the argument checks reachable from a caller."""
import math

import pytest
import torch

import gemm_cases as gc  # noqa: E402

pytestmark = pytest.mark.gpu

NAN_BITS = 0x7FC0BEEF            # a quiet NaN with a payload: "never written" as a bit pattern


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from sed_crnn_amd import ops as o
    return o


_DATA = {}


def data(name, kind):
    """operands, bias, a prior out and the float64 product (rocBLAS, on the device) of a row, made once and never modified.
    kind "int": integers in [-3, 3]; "real": N(0,1)"""
    key = (name, kind)
    if key not in _DATA:
        M, N, K = gc.case(name)["shape"]
        gen = torch.Generator().manual_seed(2 * gc.NAMES.index(name) + (kind == "real"))
        if kind == "int":
            A, B, bias, prior = (torch.randint(-3, 4, s, generator=gen).float() for s in ((M, K), (K, N), (N,), (M, N)))
        else:
            A, B, bias, prior = (torch.randn(s, generator=gen) for s in ((M, K), (K, N), (N,), (M, N)))
        A, B, bias, prior = (t.cuda() for t in (A, B, bias, prior))
        _DATA[key] = dict(A=A, B=B, bias=bias, prior=prior, prod=A.double() @ B.double(), shape=(M, N, K), kind=kind)
    return _DATA[key]


def layouts(d):
    """the four layouts of a row's operands, built as test_gemm_f32_layouts builds them"""
    A_t, B_t = d["A"].t().contiguous().t(), d["B"].t().contiguous().t()          # stored [K][M] / stored [N][K]
    for ta, tb in gc.LAYOUTS:
        yield f"A[{'K][M' if ta else 'M][K'}] B[{'N][K' if tb else 'K][N'}]", (A_t if ta else d["A"]), (B_t if tb else d["B"])


def shifted(t):
    """the same values and strides one float into a buffer of its own: no 16-byte alignment, so no float4 reads"""
    buf = torch.empty(t.numel() + 1, device=t.device)
    v = buf[1:].as_strided(t.size(), t.stride())
    v.copy_(t)
    assert v.data_ptr() % 16 == 4
    return v


def nan_out(M, N, width=None, col=0):
    """an [M, N] output whose every float is NAN_BITS; with width: a column block starting at col of an [M, width] tensor
    -> (out, whole)"""
    whole = torch.full((M, width or N), NAN_BITS, dtype=torch.int32, device="cuda").view(torch.float32)
    return whole[:, col:col + N], whole


def untouched_outside(whole, col, N):
    bits = whole.view(torch.int32)
    return bool((bits[:, :col] == NAN_BITS).all()) and bool((bits[:, col + N:] == NAN_BITS).all())


def run(ops, policy, A, B, bias=None, out=None, beta=0.0):
    if policy == 0:
        return ops.gemm(A, B, bias=bias, out=out, beta=beta)
    assert beta == 0.0
    return ops.gemm_ws(A, B, out=out, bias=bias if policy == 1 else None, wgrad=policy == 2)


def plan_text(ops, name, policy):
    M, N, K = gc.case(name)["shape"]
    bm, bn, splits, k_len = ops.gemm_plan(M, N, K, policy)
    return f"{name} {M}x{N}x{K} {gc.POLICY_NAME[policy]}: tile {bm}x{bn}, {splits} slice(s) of {k_len}"


def check_tile(ops, name):
    """the row still runs on the tile it claims (test_cpu_gemm_plan.py holds the rest of the claims)"""
    M, N, K = gc.case(name)["shape"]
    assert ops.gemm_plan(M, N, K, 0)[:2] == gc.case(name)["claims"]["tile"], name


def expect_equal(got, ref, what):
    if not torch.equal(got.double(), ref.double()):
        blocks = gc.differing_blocks(got, ref)
        bad = ~(got.double() == ref.double())
        pytest.fail(f"{what}: {int(bad.sum())} of {bad.numel()} elements differ ({int(torch.isnan(got).sum())} NaN); "
                    + gc.describe_blocks(blocks, *got.shape))


def expect_close(got, ref, K, beta, what):
    """-> the largest error as a multiple of sqrt(K) 2^-24"""
    atol, rtol = gc.tolerance(K, beta)
    err = (got.double() - ref).abs()
    bad = ~(err <= atol + rtol * ref.abs())                 # NaN counts as bad
    if bool(bad.any()):
        pytest.fail(f"{what}: {int(bad.sum())} elements beyond atol {atol:.3g} rtol {rtol:g} ({int(torch.isnan(got).sum())} NaN), largest error "
                    f"{torch.nan_to_num(err, nan=0.0).max().item():.3g}; " + gc.describe_blocks(gc.differing_blocks(bad.double(), torch.zeros_like(err)), *got.shape))
    return err.max().item() / (math.sqrt(K) * 2.0 ** -24)


def expect(d, got, ref, beta, what):
    if d["kind"] == "int":
        expect_equal(got, ref, what)
        return 0.0
    return expect_close(got, ref, d["shape"][2], beta, what)


def all_entries(ops, d, name, operands):
    """every layout through gemm, gemm_ws and gemm_ws(wgrad=True) into a NaN-filled out, and gemm with beta = 1 onto a prior out;
    -> {entry: largest error / (sqrt(K) 2^-24)} (zeros for the integer kind, which must be exact)"""
    M, N, K = d["shape"]
    with_bias = d["prod"] + d["bias"].double()
    worst = {}
    for lname, A, B in operands:
        for policy in (0, 1, 2):
            out, _ = nan_out(M, N)
            run(ops, policy, A, B, bias=d["bias"], out=out)
            r = expect(d, out, d["prod"] if policy == 2 else with_bias, 0.0, f"{plan_text(ops, name, policy)}, {lname}, beta = 0")
            worst[gc.POLICY_NAME[policy]] = max(worst.get(gc.POLICY_NAME[policy], 0.0), r)
        out = d["prior"].clone()
        run(ops, 0, A, B, bias=d["bias"], out=out, beta=1.0)
        r = expect(d, out, with_bias + d["prior"].double(), 1.0, f"{plan_text(ops, name, 0)}, {lname}, beta = 1")
        worst["gemm beta=1"] = max(worst.get("gemm beta=1", 0.0), r)
    return worst


@pytest.mark.parametrize("name", gc.NAMES)
def test_exact_on_small_integers(ops, name):
    check_tile(ops, name)
    d = data(name, "int")
    assert gc.exactness_bound(d["shape"][2]) < 2 ** 24
    all_entries(ops, d, name, layouts(d))


@pytest.mark.parametrize("name", gc.NAMES)
def test_real_values_against_float64(ops, name):
    """the bound is test_gemm_f32_layouts's (8e-5 sqrt(K) absolute, 1e-4 relative, the absolute part doubled with beta = 1); the
    printed figures are the observed maxima over the four layouts in units of sqrt(K) 2^-24, for whoever touches the kernel next"""
    check_tile(ops, name)
    d = data(name, "real")
    worst = all_entries(ops, d, name, layouts(d))
    print(f"gemm {plan_text(ops, name, gc.case(name)['policy'])}: max err / (sqrt(K) 2^-24): "
          + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))


def _blocks_of(M, N):
    """an interior 64 x 64 block (odd block indices: the second half of a 128-wide tile) and the ragged corner block"""
    rb, cb = (M // 64) // 2 | 1, (N // 64) // 2 | 1
    assert (rb + 1) * 64 < M and (cb + 1) * 64 < N
    r0, c0 = 64 * ((M - 1) // 64), 64 * ((N - 1) // 64)
    return (("interior", rb * 64, rb * 64 + 64, cb * 64, cb * 64 + 64), ("corner", r0, M, c0, N))


@pytest.mark.parametrize("name", gc.NAMES)
def test_one_summation_order_whatever_the_tile(ops, name):
    """gemm (never split): the four layouts of a row give identical bits, and on the large-tile rows a 64 x 64 block cut out of the
    operands and run as its own call - on the 64x64 tile, and FULL or guarded as ITS extents decide - equals that block of the
    whole call bit for bit"""
    check_tile(ops, name)
    d = data(name, "real")
    M, N, K = d["shape"]
    ops_l = list(layouts(d))
    outs = [ops.gemm(A, B, bias=d["bias"]) for _, A, B in ops_l]
    for (lname, _, _), o in zip(ops_l[1:], outs[1:]):
        expect_equal(o, outs[0], f"{plan_text(ops, name, 0)}: layout {lname} against {ops_l[0][0]}")
    if name not in gc.LARGE_TILE_ROWS:
        return
    for bname, r0, r1, c0, c1 in _blocks_of(M, N):
        assert ops.gemm_plan(r1 - r0, c1 - c0, K, 0) == (64, 64, 1, K)
        for lname, A, B in ops_l:
            sub = ops.gemm(A[r0:r1], B[:, c0:c1], bias=d["bias"][c0:c1])
            expect_equal(sub, outs[0][r0:r1, c0:c1], f"{plan_text(ops, name, 0)}: {bname} block rows {r0}:{r1} cols {c0}:{c1} as its own call, {lname}")


@pytest.mark.parametrize("name", [n for n in gc.FWD2_ROWS if gc.case(n)["shape"][0] > 384])
def test_forward_two_slice_rows_equal_their_row_chunks(ops, name):
    """gemm_ws (policy 1): a chunk of at least 384 rows gets the same two K-slices as the whole call, on whatever tile its own M
    selects, and must equal its rows of the whole bit for bit - batch separability of the eval forward, at the kernel"""
    d = data(name, "real")
    M, N, K = d["shape"]
    whole_plan = ops.gemm_plan(M, N, K, 1)
    assert whole_plan[2:] == (gc.case(name)["claims"]["splits"], gc.case(name)["claims"]["k_len"]) and whole_plan[2] == 2
    chunks = [(0, 384), (M - 384, M)] + ([(640, 1664)] if M >= 1664 else [])
    plans = [ops.gemm_plan(r1 - r0, N, K, 1) for r0, r1 in chunks]
    assert all(p[2:] == whole_plan[2:] for p in plans), plans
    if whole_plan[:2] != (64, 64):
        assert any(p[:2] != whole_plan[:2] for p in plans), "no chunk runs on another tile than the whole"
    ref = None
    for lname, A, B in layouts(d):
        whole = run(ops, 1, A, B, bias=d["bias"])
        ref = whole if ref is None else ref
        expect_equal(whole, ref, f"{plan_text(ops, name, 1)}: layout {lname} against the first")
        for (r0, r1), p in zip(chunks, plans):
            part = run(ops, 1, A[r0:r1], B, bias=d["bias"])
            expect_equal(part, ref[r0:r1], f"{plan_text(ops, name, 1)}: rows {r0}:{r1} as their own call (tile {p[0]}x{p[1]}), {lname}")


def _split_policies(name):
    c = gc.case(name)
    other = 2 if c["policy"] == 1 else 1
    return [c["policy"]] + ([other] if gc.OTHER_POLICY[name][0] > 1 else [])


def _direct(ops, policy, A, B, out, bias, ws):
    """the library entry itself, with the caller's workspace"""
    from sed_crnn_amd._lib import check, ptr, stream_ptr
    M, K = A.shape
    N = B.shape[1]
    L = ops.lib()
    if policy == 1:
        check(L.sed_gemm_f32_ws(ptr(A), A.stride(0), A.stride(1), ptr(B), B.stride(0), B.stride(1), ptr(out), out.stride(0), ptr(bias),
                                M, N, K, ptr(ws), stream_ptr()), "gemm_f32_ws")
    else:
        assert bias is None
        check(L.sed_gemm_f32_wgrad(ptr(A), A.stride(0), A.stride(1), ptr(B), B.stride(0), B.stride(1), ptr(out), out.stride(0),
                                   M, N, K, ptr(ws), stream_ptr()), "gemm_f32_wgrad")


@pytest.mark.parametrize("name,policy", [(n, p) for n in gc.SPLIT_ROWS for p in _split_policies(n)])
def test_split_k_plumbing(ops, name, policy):
    """integers (exact): the slabs land in a workspace of exactly sed_gemm_f32_workspace_bytes and nowhere behind it, the result
    does not depend on what the workspace held, the reduction adds the bias through its float4 branch and (bias one float off
    alignment, ldc % 4 != 0) through its scalar branch, and writes only its column block of a wider out"""
    d = data(name, "int")
    M, N, K = d["shape"]
    splits = ops.gemm_plan(M, N, K, policy)[2]
    assert splits > 1
    nb = ops.lib().sed_gemm_f32_workspace_bytes(M, N, K)
    assert nb >= 4 * M * N * splits and nb % 4 == 0
    guard = 4096
    buf = torch.full((nb // 4 + guard,), NAN_BITS, dtype=torch.int32, device="cuda")
    ws = buf.view(torch.float32)
    bias_off = shifted(d["bias"])
    with_bias = d["prod"] + d["bias"].double()
    what = plan_text(ops, name, policy)
    W = (N + 8 + 3) // 4 * 4
    for lname, A, B in layouts(d):
        out, _ = nan_out(M, N)
        _direct(ops, policy, A, B, out, None, ws)
        expect_equal(out, d["prod"], f"{what}, {lname}, no bias, workspace of NaN")
        buf[:nb // 4] = torch.tensor(1e30).view(torch.int32).item()           # another content: the slabs are written, not added to
        again, _ = nan_out(M, N)
        _direct(ops, policy, A, B, again, None, ws)
        assert torch.equal(out, again), f"{what}, {lname}: two calls differ"
        buf[:nb // 4] = NAN_BITS
        assert bool((buf[nb // 4:] == NAN_BITS).all()), f"{what}, {lname}: the guard behind the workspace was written"
        for width, col, label in ((W, 4, "ldc % 4 == 0"), (W + 1, 4, "ldc % 4 == 1")):
            out, whole = nan_out(M, N, width, col)
            _direct(ops, policy, A, B, out, None, ws)
            expect_equal(out, d["prod"], f"{what}, {lname}, column block at {col} of {width} ({label})")
            assert untouched_outside(whole, col, N), f"{what}, {lname}, {label}: columns outside the block were written"
        if policy == 1:
            for b, label in ((d["bias"], "aligned bias"), (bias_off, "bias one float off alignment")):
                out, whole = nan_out(M, N, W, 4)
                _direct(ops, policy, A, B, out, b, ws)
                expect_equal(out, with_bias, f"{what}, {lname}, {label}, column block")
                assert untouched_outside(whole, 4, N), f"{what}, {lname}, {label}: columns outside the block were written"
                out, _ = nan_out(M, N)
                _direct(ops, policy, A, B, out, b, ws)
                expect_equal(out, with_bias, f"{what}, {lname}, {label}, dense out")
    assert bool((buf[nb // 4:] == NAN_BITS).all()), f"{what}: the guard behind the workspace was written"


@pytest.mark.parametrize("kind", ["int", "real"])
@pytest.mark.parametrize("name", ["ragged_128x128", "full_128x96_k64", "wgrad2_ragged_128x64"])
def test_operands_one_float_off_alignment(ops, name, kind):
    """A and B as views one float into their buffers: a_vec = b_vec = 0 in every layout, so every workgroup takes the guarded
    path with scalar loads - also where the extents alone would make it FULL"""
    d = data(name, kind)
    M, N, K = d["shape"]
    bm, bn, splits, k_len = ops.gemm_plan(M, N, K, gc.case(name)["policy"])
    assert (bm, bn) != (64, 64) and gc.full_class(M, N, K, bm, bn, splits, k_len, *gc.layout_vecs(M, N, K, True, False, aligned=False)) == "none"
    worst = all_entries(ops, d, name, ((f"{lname} + 1 float", shifted(A), shifted(B)) for lname, A, B in layouts(d)))
    if kind == "real":
        print(f"gemm unaligned {plan_text(ops, name, gc.case(name)['policy'])}: max err / (sqrt(K) 2^-24): "
              + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))


@pytest.mark.parametrize("kind", ["int", "real"])
@pytest.mark.parametrize("name", ["ragged_128x64", "fwd2_ragged"])
def test_output_block_at_an_odd_column(ops, name, kind):
    """out as the columns 3 : 3 + N of a wider tensor (an odd ldc too): gemm with beta = 0 and 1, and gemm_ws, whose reduction must
    take its scalar branch on the split row; nothing outside the block is written"""
    d = data(name, kind)
    M, N, K = d["shape"]
    with_bias = d["prod"] + d["bias"].double()
    for lname, A, B in layouts(d):
        for policy in (0, 1):
            out, whole = nan_out(M, N, N + 7, 3)
            assert out.data_ptr() % 8 == 4
            run(ops, policy, A, B, bias=d["bias"], out=out)
            expect(d, out, with_bias, 0.0, f"{plan_text(ops, name, policy)}, {lname}, out at column 3 of {N + 7}")
            assert untouched_outside(whole, 3, N), f"{plan_text(ops, name, policy)}, {lname}: columns outside the block were written"
        out, whole = nan_out(M, N, N + 7, 3)
        out.copy_(d["prior"])
        run(ops, 0, A, B, bias=d["bias"], out=out, beta=1.0)
        expect(d, out, with_bias + d["prior"].double(), 1.0, f"{plan_text(ops, name, 0)}, {lname}, beta = 1, out at column 3 of {N + 7}")
        assert untouched_outside(whole, 3, N)


def test_argument_checks_launch_nothing(ops):
    """what a caller can get wrong on a row that splits: each returns an error with a message, and neither out nor the workspace
    is touched (the checks come before any launch)"""
    from sed_crnn_amd._lib import ptr, stream_ptr
    L = ops.lib()
    M, N, K = gc.case("small_k1024")["shape"]
    assert ops.gemm_plan(M, N, K, 1)[2] > 1
    d = data("small_k1024", "int")
    A, B = d["A"], d["B"]
    nb = L.sed_gemm_f32_workspace_bytes(M, N, K)
    ws_bits = torch.full((nb // 4,), NAN_BITS, dtype=torch.int32, device="cuda")
    ws = ws_bits.view(torch.float32)
    out, whole = nan_out(M, N)
    strided = torch.zeros(K, 2 * K, device="cuda")[:, ::2]                  # strides (2K, 2): no unit stride (large enough for either operand)
    assert strided.stride() == (2 * K, 2)

    def entries(a, a_si, a_sk, b, b_sk, b_sj, ldc, m, n, k):
        return (("gemm_f32", lambda: L.sed_gemm_f32(ptr(a), a_si, a_sk, ptr(b), b_sk, b_sj, ptr(out), ldc, None, 0.0, m, n, k, stream_ptr())),
                ("gemm_f32_ws", lambda: L.sed_gemm_f32_ws(ptr(a), a_si, a_sk, ptr(b), b_sk, b_sj, ptr(out), ldc, None, m, n, k, ptr(ws), stream_ptr())),
                ("gemm_f32_wgrad", lambda: L.sed_gemm_f32_wgrad(ptr(a), a_si, a_sk, ptr(b), b_sk, b_sj, ptr(out), ldc, m, n, k, ptr(ws), stream_ptr())))

    good = (A, K, 1, B, N, 1, N, M, N, K)
    bad = {"ldc < N": (good[:6] + (N - 1, M, N, K), "bad sizes"),
           "A without a unit stride": ((strided, 2 * K, 2) + good[3:], "A must be contiguous"),
           "B without a unit stride": (good[:3] + (strided, 2 * K, 2) + good[6:], "B must be contiguous"),
           "M = 0": (good[:7] + (0, N, K), "bad sizes"), "N = 0": (good[:7] + (M, 0, K), "bad sizes"), "K = 0": (good[:7] + (M, N, 0), "bad sizes")}
    for label, (args, text) in bad.items():
        for entry, call in entries(*args):
            assert L.sed_gemm_f32_plan(0, 0, 0, 0, None, None, None, None) < 0   # another failure in between: the message must be the call's own
            rc = call()
            msg = L.sed_last_error_string().decode()
            assert rc < 0 and text in msg and "gemm_f32:" in msg, (label, entry, rc, msg)
    torch.cuda.synchronize()
    assert bool((whole.view(torch.int32) == NAN_BITS).all()) and bool((ws_bits == NAN_BITS).all())
    # ... and the same arguments, put right, run
    for entry, call in entries(*good):
        assert call() == 0, (entry, L.sed_last_error_string())
    expect_equal(out, d["prod"], "small_k1024 after the rejected calls")
