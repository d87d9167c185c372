"""Every instantiation of the GRU recurrence kernels (csrc/gru.hip) against float64, at the batch sizes where the dispatch
leaves the one-row tile: `gru_bt` picks 2 rows per workgroup from B = 256 and 4 from B = 512 (H < 128), and GRU_DISPATCH turns
(H, tile) into register-resident, streamed or hybrid weight placement.  test_gpu_kernels.py runs B <= 6 only.

Reference: torch.nn.GRU(...).double() on the CPU.  The kernels start from the input projections gi, so the float64 values of
what nn.GRU does not expose (the saved gates, d gi, d gh) come from a float64 restatement of the cell, which every case
first pins to nn.GRU.double() itself (output to 1e-12, input gradient to 1e-10).  Yardstick: the same computation in torch
float32 (nn.GRU for the output and the parameter / input gradients, the restatement for d gi / d gh).

Bounds.  Forward: max |delta| <= 2e-5 on out and on the saved r, z, n, gh_n, h_prev (values bounded by about 1; the bound of
test_gru_recurrence_fwd_bwd).  Backward: e_hip <= 3 * e_torch32 + 2e-6 with both errors relative L2 against float64 (the form of
test_single_step_gradients_are_as_close_to_float64_as_torch_float32) — per batch row for d gi and d gh, so that one wrong row
at a ragged tile end cannot hide in a 1024-row norm, per tensor for dx, dW_ih, dW_hh, db_ih, db_hh formed from the kernel's
d gi / d gh with float64 host products, and for the kernel's own bias-gradient outputs.

Tile invariance.  The rows of a B >= 256 call must be bitwise those of the same rows run in sub-batches of 128 (tile 1; for
H = 256 that is the hybrid against <0,2>): DESIGN 5f's "chunking changes nothing" rests on it.  The same equality of the
backward is printed, not asserted (no documented claim rests on it); the tile-1 errors of the same rows are printed next to
the variant's so that a miss can be attributed to the tile or to the gate arithmetic.

Every case prints its variant class, the HIP and torch-float32 errors and their ratio (run with -s).  Measured on the MI355X
(table in DESIGN 2): forward max |delta| <= 1.9e-7; worst-row d gi / d gh errors 0.7e-7 .. 2.1e-7 next to torch-float32's 0.7e-7 ..
1.7e-7 and within 15 % of the tile-1 errors of the same rows; the largest use of the backward bound, 0.21, is the kernel's own
bias gradient.
Before the forward's four-term groups were written as an explicit FMA chain (gru_dot4), case 300x8x256 failed the tile
invariance: all 300 rows differed from the hybrid's by up to 8.9e-8."""
import copy
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

IN = 24
FWD_ATOL = 2e-5
BWD_FACTOR, BWD_FLOOR = 3.0, 2e-6

# (B, T, H) -> the class sed_gru_seq_variant must report: (rows per workgroup, weights of a gate row in registers, in LDS).
# registers == H: register-resident; 0: streamed from L2; LDS > 0: the H = 256 hybrid (registers + LDS + streamed).
# tests/test_cpu_gru_variants.py asserts that this table covers every class the dispatch can reach.
HYBRID = (1, 116, 48)
CASES = {
    "tile 1": [((5, 4, 8), (1, 8, 0)), ((7, 5, 16), (1, 16, 0)), ((255, 6, 32), (1, 32, 0)), ((6, 5, 64), (1, 64, 0)),
               ((6, 16, 128), (1, 128, 0)), ((4, 6, 20), (1, 0, 0))],
    "tile 2, registers": [((257, 6, 8), (2, 8, 0)), ((300, 5, 16), (2, 16, 0)), ((256, 9, 32), (2, 32, 0)),
                          ((511, 7, 64), (2, 64, 0)), ((256, 16, 128), (2, 128, 0)), ((513, 9, 128), (2, 128, 0)),
                          ((1024, 8, 128), (2, 128, 0))],
    "tile 4, registers": [((512, 5, 8), (4, 8, 0)), ((515, 6, 16), (4, 16, 0)), ((1024, 8, 32), (4, 32, 0)),
                          ((513, 12, 64), (4, 64, 0))],
    "streamed": [((258, 6, 20), (2, 0, 0)), ((257, 5, 136), (2, 0, 0)), ((300, 8, 256), (2, 0, 0)), ((512, 6, 20), (4, 0, 0)),
                 ((514, 5, 100), (4, 0, 0))],
    "hybrid": [((3, 6, 256), HYBRID), ((255, 8, 256), HYBRID)],
    "prefetch edges": [((256, 1, 128), (2, 128, 0)), ((512, 2, 32), (4, 32, 0)), ((512, 1, 20), (4, 0, 0)),
                       ((3, 1, 256), HYBRID), ((3, 2, 256), HYBRID)],
}
CASE_LIST = [(group, shape, cls) for group, rows in CASES.items() for shape, cls in rows]


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from sed_crnn_amd import ops as o
    return o


def g(t):
    return t.cuda().contiguous()


def _cell(gi, whh, bhh):
    """nn.GRU's recurrence restated from the input projections: gi [B,T,2,3H] (a leaf) -> out [B,T,2H], saved [B,T,2,5,H]
    (r, z, n, gh_n, h_prev as the kernel stores them) and the gh = h W_hh^T + b_hh of every (direction, step), kept so that
    autograd reports their gradients.  dtype follows gi."""
    B, T, _, H3 = gi.shape
    H = H3 // 3
    out = [[None] * T for _ in range(2)]
    saved = [[None] * T for _ in range(2)]
    ghs = [[None] * T for _ in range(2)]
    for d in range(2):
        h = torch.zeros(B, H, dtype=gi.dtype)
        for s in range(T):
            tt = T - 1 - s if d else s
            gh = h @ whh[d].t() + bhh[d]
            if gh.requires_grad:
                gh.retain_grad()
            elif gi.requires_grad:
                gh.requires_grad_(True)                     # step 0: h = 0, gh = b_hh is a leaf of its own
            a = gi[:, tt, d]
            r = torch.sigmoid(a[:, :H] + gh[:, :H])
            z = torch.sigmoid(a[:, H:2 * H] + gh[:, H:2 * H])
            n = torch.tanh(a[:, 2 * H:] + r * gh[:, 2 * H:])
            hn = (1 - z) * n + z * h
            saved[d][tt] = torch.stack([r, z, n, gh[:, 2 * H:], h], dim=1)        # [B,5,H]
            ghs[d][tt], out[d][tt] = gh, hn
            h = hn
    out_t = torch.stack([torch.cat([out[0][t], out[1][t]], dim=1) for t in range(T)], dim=1)
    saved_t = torch.stack([torch.stack([saved[0][t], saved[1][t]], dim=1) for t in range(T)], dim=1)
    return out_t, saved_t.detach(), ghs


def _cell_grads(gi_values, whh, bhh, dout):
    gi = gi_values.clone().requires_grad_(True)
    out, saved, ghs = _cell(gi, whh, bhh)
    out.backward(dout)
    T = gi.shape[1]
    dgh = torch.stack([torch.stack([ghs[0][t].grad, ghs[1][t].grad], dim=1) for t in range(T)], dim=1)
    return out.detach(), saved, gi.grad, dgh


def _params(gru):
    return ([gru.weight_ih_l0, gru.weight_ih_l0_reverse], [gru.weight_hh_l0, gru.weight_hh_l0_reverse],
            [gru.bias_ih_l0, gru.bias_ih_l0_reverse], [gru.bias_hh_l0, gru.bias_hh_l0_reverse])


def _rel(a, ref):
    return ((a.double() - ref).norm() / (ref.norm() + 1e-300)).item()


def _rel_rows(a, ref):
    B = ref.shape[0]
    return (a.double() - ref).reshape(B, -1).norm(dim=1) / (ref.reshape(B, -1).norm(dim=1) + 1e-300)


def _derived(dgi, dgh, hprev, x64, wih64):
    """dx, dW_ih, dW_hh, db_ih, db_hh from d gi / d gh by float64 host products"""
    B, T, _, H3 = dgi.shape
    dgi, dgh, hprev = dgi.double(), dgh.double(), hprev.double()
    res = {"dx": sum(dgi[:, :, d] @ wih64[d] for d in range(2))}
    for d in range(2):
        a, c = dgi[:, :, d].reshape(-1, H3), dgh[:, :, d].reshape(-1, H3)
        res[f"dW_ih[{d}]"] = a.t() @ x64.reshape(B * T, -1)
        res[f"dW_hh[{d}]"] = c.t() @ hprev[:, :, d].reshape(B * T, -1)
        res[f"db_ih[{d}]"], res[f"db_hh[{d}]"] = a.sum(0), c.sum(0)
    return res


def _hip_in_chunks(ops, gi, dout, whh, bhh, chunk):
    outs, saveds, dgis, dghs = [], [], [], []
    for i in range(0, gi.shape[0], chunk):
        o, s = ops.gru_seq_fwd(gi[i:i + chunk].contiguous(), whh, bhh)
        a, c = ops.gru_seq_bwd(dout[i:i + chunk].contiguous(), s, whh)
        outs.append(o); saveds.append(s); dgis.append(a); dghs.append(c)
    return torch.cat(outs), torch.cat(saveds), torch.cat(dgis), torch.cat(dghs)


@pytest.mark.parametrize("group,shape,cls", CASE_LIST, ids=[f"{s[0]}x{s[1]}x{s[2]}" for _, s, _ in CASE_LIST])
def test_gru_variant_against_float64(ops, group, shape, cls):
    B, T, H = shape
    assert ops.gru_seq_variant(B, H) == cls, f"{shape} ({group}) no longer runs the variant its row names"
    torch.manual_seed(1000 * H + 10 * B + T)
    ref32 = torch.nn.GRU(IN, H, batch_first=True, bidirectional=True)
    ref64 = copy.deepcopy(ref32).double()
    x32, dout32 = torch.randn(B, T, IN), torch.randn(B, T, 2 * H)
    x64, dout64 = x32.double().requires_grad_(True), dout32.double()
    x32.requires_grad_(True)
    ref64(x64)[0].backward(dout64)
    out_t32 = ref32(x32)[0]
    out_t32.backward(dout32)
    wih64, whh64, bih64, bhh64 = _params(ref64)
    wih32, whh32, bih32, bhh32 = _params(ref32)
    with torch.no_grad():
        gi64 = torch.stack([x64 @ wih64[d].t() + bih64[d] for d in range(2)], dim=2)              # [B,T,2,3H]
        out_gru64 = ref64(x64)[0]
    gi32 = gi64.float()                                     # the kernels' input: the float64 projections, rounded once

    # float64 restatement, pinned to nn.GRU.double() before it serves as reference
    out64, saved64, dgi64, dgh64 = _cell_grads(gi64, [w.detach() for w in whh64], [b.detach() for b in bhh64], dout64)
    assert (out64 - out_gru64).abs().max().item() <= 1e-12
    ref_derived = _derived(dgi64, dgh64, saved64[:, :, :, 4], x64.detach(), [w.detach() for w in wih64])
    truth = {"dx": x64.grad}
    for d in range(2):
        truth.update({f"dW_ih[{d}]": wih64[d].grad, f"dW_hh[{d}]": whh64[d].grad, f"db_ih[{d}]": bih64[d].grad,
                      f"db_hh[{d}]": bhh64[d].grad})
    for k, v in truth.items():
        assert _rel(ref_derived[k], v) <= 1e-10, f"float64 restatement disagrees with nn.GRU.double() on {k}"
    # torch float32 yardsticks
    _, _, dgi_t32, dgh_t32 = _cell_grads(gi32, [w.detach() for w in whh32], [b.detach() for b in bhh32], dout32)
    yard = {"dx": x32.grad}
    for d in range(2):
        yard.update({f"dW_ih[{d}]": wih32[d].grad, f"dW_hh[{d}]": whh32[d].grad, f"db_ih[{d}]": bih32[d].grad,
                     f"db_hh[{d}]": bhh32[d].grad})

    # the kernels
    whh_g, bhh_g = [g(w.detach()) for w in whh32], [g(b.detach()) for b in bhh32]
    gi_g, dout_g = g(gi32), g(dout32)
    out, saved = ops.gru_seq_fwd(gi_g, whh_g, bhh_g)
    dgi, dgh, dbih, dbhh = ops.gru_seq_bwd(dout_g, saved, whh_g, want_bias=True)
    dgi2, dgh2 = ops.gru_seq_bwd(dout_g, saved, whh_g)
    torch.cuda.synchronize()
    assert torch.equal(dgi, dgi2) and torch.equal(dgh, dgh2), "bias-gradient request changes d gi / d gh"
    out_c, saved_c, dgi_c, dgh_c = out.cpu(), saved.cpu(), dgi.cpu(), dgh.cpu()

    tag = f"gru-variant B={B} T={T} H={H} class={cls} [{group}]"
    fails = []
    # forward
    e_out, e_out_t = (out_c.double() - out64).abs().max().item(), (out_t32.detach().double() - out64).abs().max().item()
    print(f"{tag} fwd: max|d out| hip {e_out:.2e} torch-f32 {e_out_t:.2e}")
    if not e_out <= FWD_ATOL:
        fails.append(f"out: max |delta| {e_out:.3e} > {FWD_ATOL}")
    for j, name in enumerate(("r", "z", "n", "gh_n", "h_prev")):
        diff = (saved_c[:, :, :, j].double() - saved64[:, :, :, j]).abs()
        e = diff.max().item()
        if not e <= FWD_ATOL:
            fails.append(f"saved {name}: max |delta| {e:.3e} > {FWD_ATOL} (row {diff.reshape(B, -1).max(1).values.argmax().item()})")
    # tile 1 on the same rows
    sub = None
    if B >= 256:
        sub = _hip_in_chunks(ops, gi_g, dout_g, whh_g, bhh_g, 128)
        assert ops.gru_seq_variant(128, H)[0] == 1
        fwd_same = torch.equal(out, sub[0]) and torch.equal(saved, sub[1])
        bwd_same = torch.equal(dgi, sub[2]) and torch.equal(dgh, sub[3])
        print(f"{tag} vs sub-batches of 128 (tile 1): forward bitwise equal {fwd_same}, backward bitwise equal {bwd_same}")
        if not fwd_same:
            rows = ((out != sub[0]).reshape(B, -1).any(1) | (saved != sub[1]).reshape(B, -1).any(1)).nonzero().flatten().tolist()
            fails.append(f"forward differs from its tile-1 sub-batches in {len(rows)} rows (first {rows[:6]}), "
                         f"max |delta out| {(out - sub[0]).abs().max().item():.3e}")
    # backward, per row
    worst = 0.0
    for name, a, ref, t32, s1 in (("dgi", dgi_c, dgi64, dgi_t32, sub[2].cpu() if sub else None),
                                  ("dgh", dgh_c, dgh64, dgh_t32, sub[3].cpu() if sub else None)):
        e_h, e_t = _rel_rows(a, ref), _rel_rows(t32, ref)
        use = e_h / (BWD_FACTOR * e_t + BWD_FLOOR)
        i = use.argmax().item()
        worst = max(worst, use[i].item())
        line = f"{tag} {name} per row: worst row {i}: hip {e_h[i].item():.2e} torch-f32 {e_t[i].item():.2e} ratio " \
               f"{e_h[i].item() / (e_t[i].item() + 1e-300):.2f} bound use {use[i].item():.2f}; max over rows hip {e_h.max().item():.2e} " \
               f"torch-f32 {e_t.max().item():.2e}"
        if s1 is not None:
            line += f"; tile 1 on the same rows {_rel_rows(s1, ref).max().item():.2e}"
        print(line)
        bad = (use > 1).nonzero().flatten().tolist()
        if bad:
            fails.append(f"{name}: {len(bad)} rows over {BWD_FACTOR} * e_torch32 + {BWD_FLOOR} (first {bad[:6]}); worst row {i}: "
                         f"hip {e_h[i].item():.3e}, torch-f32 {e_t[i].item():.3e}")
    # backward, derived gradients per tensor
    mine = _derived(dgi_c, dgh_c, saved_c[:, :, :, 4], x64.detach(), [w.detach() for w in wih64])
    for d in range(2):
        mine[f"kernel db_ih[{d}]"], mine[f"kernel db_hh[{d}]"] = dbih[d].cpu(), dbhh[d].cpu()
    for k, v in mine.items():
        key = k.replace("kernel ", "")
        e_h, e_t = _rel(v, truth[key]), _rel(yard[key], truth[key])
        use = e_h / (BWD_FACTOR * e_t + BWD_FLOOR)
        worst = max(worst, use)
        print(f"{tag} {k}: hip {e_h:.2e} torch-f32 {e_t:.2e} ratio {e_h / (e_t + 1e-300):.2f} bound use {use:.2f}")
        if not use <= 1:
            fails.append(f"{k}: hip {e_h:.3e} > {BWD_FACTOR} * torch-f32 {e_t:.3e} + {BWD_FLOOR}")
    print(f"{tag} worst use of the backward bound: {worst:.2f}")
    assert not fails, tag + ":\n  " + "\n  ".join(fails)
