"""float64 references of the conv data gradient and of the BatchNorm-backward sums its epilogues form, shared by
test_gpu_wino_dgrad_epilogue.py (the Winograd kernels) and test_gpu_conv_tiles.py (the direct MFMA kernel).  Plain torch on the
CPU: nothing here touches the library."""
import numpy as np
import torch
import torch.nn.functional as F


def _dx_ref(dy, w):
    """float64 data gradient of conv2d(., w, padding=1); dy channels-last [B,T,F,C] -> [B,T,F,Cin]"""
    B, T, Fm, _ = dy.shape
    return torch.nn.grad.conv2d_input((B, w.shape[1], Fm, T), w.double(), dy.permute(0, 3, 2, 1).contiguous().double(), padding=1).permute(0, 3, 2, 1).contiguous()


def _bn_sums_ref(dref, pooled, gamma, beta, keep, small_gamma_rule):
    """(g, sum g, sum g*xhat, zeroed channels) in float64 from the float64 dx and the forward's pooled output.  Channels whose
    xhat the pooled output cannot give get sum g*xhat = 0 from the epilogue by specification: gamma == 0, and — when the block
    below keeps its conv output, from which sed_bn_bwd_finalize_small_gamma finishes them — |gamma| * 64 < |beta|."""
    pq, gm, bt = pooled.cpu().double(), gamma.cpu().double(), beta.cpu().double()
    gg = torch.where(pq > 0, dref / keep, torch.zeros_like(dref))
    zero = gm == 0
    if small_gamma_rule:
        zero = zero | (gm.abs() * 64 < bt.abs())
    xhat = (keep * pq - bt) / torch.where(zero, torch.ones_like(gm), gm)
    sgx = (gg * xhat).sum((0, 1, 2))
    sgx[zero] = 0.0
    return gg, gg.sum((0, 1, 2)), sgx, zero


def _fp32_formula_error(dref, pooled, gamma, beta, keep, zero, sg_ref, sgx_ref):
    """what the epilogue's arithmetic costs when every element is formed in float32 from the correctly rounded dx (the sums kept
    in float64): the part of the bound that no summation order can win back"""
    pq = pooled.cpu()
    g0 = torch.where(pq > 0, dref.float(), torch.zeros_like(pq))
    rg = torch.where(zero, torch.zeros_like(gamma.cpu()), 1.0 / torch.where(zero, torch.ones_like(gamma.cpu()), gamma.cpu()))
    q_kr, q_nb = rg * float(np.float32(keep)), -beta.cpu() * rg
    inv_keep = np.float32(1.0) / np.float32(keep)
    e1 = ((g0.double().sum((0, 1, 2)) * float(inv_keep)) - sg_ref).abs().max()
    e2 = (((g0 * (pq * q_kr + q_nb)).double().sum((0, 1, 2)) * float(inv_keep)) - sgx_ref).abs().max()
    return float(e1), float(e2)


def _first_block_grads_ref(x, w1, b1, mean, rstd, scale, gref, bits):
    """(dW, dgamma) of the first block in float64: conv -> BatchNorm backward (the forward's mean / rstd / scale) ->
    conv2d_weight.  x [B,cin,F,T] is the network input, gref [B,T/2,F,C] the gradient g of the pooled output where it passes; the
    gradient of the selected conv output is g at time 2 t' + (arg-max bit), zero elsewhere."""
    B, cin, Fm, T = x.shape
    C, Tp = w1.shape[0], T // 2
    sel = ((bits.cpu().to(torch.int32).reshape(B, Tp, Fm, C // 4, 1) >> torch.arange(4, dtype=torch.int32)) & 1).reshape(B, Tp, Fm, C).bool()
    G = torch.zeros(B, Tp, 2, Fm, C, dtype=torch.float64)
    G[:, :, 0] = torch.where(sel, torch.zeros_like(gref), gref)
    G[:, :, 1] = torch.where(sel, gref, torch.zeros_like(gref))
    G = G.reshape(B, T, Fm, C).permute(0, 3, 2, 1)                                   # [B,C,F,T]
    mu, rs, sc = (t.cpu().double().reshape(1, C, 1, 1) for t in (mean, rstd, scale))
    y = F.conv2d(x.double(), w1.double(), b1.double(), padding=1)
    xhat = (y - mu) * rs
    n = B * T * Fm
    sgm, sgxm = G.sum((0, 2, 3), keepdim=True) / n, (G * xhat).sum((0, 2, 3), keepdim=True) / n
    dyc = sc * (G - sgm - xhat * sgxm)
    return torch.nn.grad.conv2d_weight(x.double(), (C, cin, 3, 3), dyc, padding=1), (G * xhat).sum((0, 2, 3))
