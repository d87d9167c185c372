#!/usr/bin/env python3
"""Where a Winograd conv launch spends its time (tuning aid): per-workgroup prologue / main loop / epilogue from s_memrealtime
stamps (sed_conv3x3_wino_phase_ticks), next to the launch time — for the three training instantiations at the two workload
shapes: the forward, the data gradient with the BatchNorm-backward sums of the block below (BNR) and with the first block's tap
sums on top (BNR+RG, with and without the dx store).  For the data gradients the epilogue is split at its exchange barrier:
"park + wait for loads" in front of it, "transform + sums" behind.  python tools/wino_probe.py"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from sed_crnn_amd import ops
from sed_crnn_amd._lib import lib, ptr, check, stream_ptr
from tools.kbench import timeit

B, F, C = 128, 40, 128
L = lib()


def probe(name, T, run):
    ms = timeit(run, 20)
    buf = torch.zeros(8, dtype=torch.int64, device="cuda")
    L.sed_conv3x3_wino_phase_ticks(ptr(buf))
    run()
    torch.cuda.synchronize()
    L.sed_conv3x3_wino_phase_ticks(None)
    t = buf.cpu().tolist()
    n = max(t[3], 1)
    us = [v / n / 100.0 for v in t[:3]]
    per_cu = n / 256.0
    split = f" = park + wait {t[4]/n/100.0:.2f} + transform + sums {us[2] - t[4]/n/100.0:.2f}" if t[4] else ""
    print(f"T={T:3d} {name:22s}: launch {ms*1e3:5.0f} us | per workgroup: prologue {us[0]:.2f} us, main loop {us[1]:.2f} us, "
          f"epilogue {us[2]:.2f} us{split} | {n} workgroups = {per_cu:.1f} per CU -> sum {per_cu*sum(us):.0f} us", flush=True)


for T in (128, 64):
    gen = torch.Generator().manual_seed(T)
    x = torch.randn(B, T, F, C, generator=gen).cuda()
    w = (torch.randn(C, C, 3, 3, generator=gen) * 0.03).cuda()
    bias = torch.randn(C, generator=gen).cuda()
    uf, ud = ops.conv3x3_wino_pack(w)
    rows = L.sed_conv3x3_wino_rows(B, C, F, T, C)
    y, stat = torch.empty(B, T, F, C).cuda(), torch.empty(rows, 2, C).cuda()
    probe("forward", T, lambda: check(L.sed_conv3x3_wino_fwd(ptr(x), ptr(uf), ptr(bias), ptr(y), ptr(stat), B, C, F, T, C, stream_ptr()), "fwd"))
    # the block below: its pooled output (what the data gradient's epilogue reads), BatchNorm parameters and statistics
    pooled = torch.randn(B, T, F, C, generator=gen).clamp_(min=0).cuda()
    gamma, beta = (torch.rand(C, generator=gen) + 0.5).cuda(), (torch.randn(C, generator=gen) * 0.3).cuda()
    mean, rstd = torch.randn(C, generator=gen).cuda(), (torch.rand(C, generator=gen) + 0.5).cuda()
    below = torch.empty(B, 2 * T, F, C).cuda()
    probe("dgrad BNR", T, lambda: check(L.sed_conv3x3_wino_dgrad_bnred(ptr(x), ptr(ud), ptr(y), ptr(stat), ptr(pooled), ptr(gamma), ptr(beta), ptr(below), ptr(mean),
                                                                       ptr(rstd), 0.25, 1, 2, F, 2 * T, B, C, F, T, C, stream_ptr()), "bnr"))
    del below
    for cin in (1, 2):
        if not L.sed_conv3x3_wino_rg_rows(B, C, F, T, C, cin):
            continue
        x1 = torch.randn(B, cin, F, 2 * T, generator=gen).cuda()
        bits = torch.randint(0, 16, (B * T * F * C // 4,), generator=gen, dtype=torch.uint8).cuda()
        rgp = torch.empty(rows, C, 1 + 9 * cin).cuda()
        for nm, dx in ((f"dgrad BNR+RG{cin}", y), (f"dgrad BNR+RG{cin}, no dx", None)):
            try:
                probe(nm, T, lambda: check(L.sed_conv3x3_wino_dgrad_bnred_rg(ptr(x), ptr(ud), ptr(dx) if dx is not None else None, ptr(stat), ptr(pooled), ptr(gamma), ptr(beta),
                                                                             ptr(mean), ptr(rstd), 0.25, ptr(x1), cin, ptr(bits), ptr(rgp), B, C, F, T, C, stream_ptr()), "rg"))
            except RuntimeError as e:                 # (a library from before dx became optional)
                print(f"T={T:3d} {nm:22s}: {e}", flush=True)
