"""The Winograd kernel's main loop must not drain its memory counter (no GPU needed: hipcc cross-compiles wino.hip to assembly).

conv3x3_wino_k leaves every s_waitcnt to hipcc.  Its patch comes in by LDS-DMA while the rolling weight fragments are ordinary
register loads; with a FLAT-encoded DMA (global_load_lds) in flight hipcc turned five of the counted waits for those fragments into
vmcnt(0) — the matrix cores then sat out a global -> LDS round trip five times per workgroup.  Through a buffer descriptor
(buffer_load ... lds) the waits are counted.  A compiler update that brings the drains back fails here instead of costing
5 % of the kernel (profiles/r6) unnoticed."""
import os
import re
import shutil
import subprocess

import pytest

from sed_crnn_amd import build as B

N_MFMA = 1024            # 16 steps x 64 MFMAs, fully unrolled
LAST_CHECKED = 960       # the last step carries the epilogue's loads (data gradients) and ends the loop: not part of the claim


def _hipcc():
    try:
        c = B._hipcc()
    except RuntimeError:
        return None
    return c if os.path.isabs(c) else shutil.which(c)


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    hipcc = _hipcc()
    if not hipcc:
        pytest.skip("hipcc not found")
    out = tmp_path_factory.mktemp("wino_asm") / "wino.s"
    cmd = [hipcc] + B.FLAGS + ["-S", "--cuda-device-only", os.path.join(B.CSRC, "wino.hip"), "-o", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    fns, cur = {}, None
    for line in out.read_text().splitlines():
        m = re.match(r"^(_Z\w*conv3x3_wino_k\w*):", line)
        if m:
            cur = fns.setdefault(m.group(1), [])
        elif line.startswith(".Lfunc_end"):
            cur = None
        elif cur is not None:
            s = line.split(";")[0].strip()
            if s and not s.startswith("."):
                cur.append(s)
    return fns


def test_every_instantiation_is_there(kernels):
    # forward, data gradient + BatchNorm-backward sums, + tap sums of one and two input channels, inference
    assert len(kernels) == 5, sorted(kernels)
    for name, ins in kernels.items():
        assert sum(i.startswith("v_mfma_f32_32x32x2") for i in ins) == N_MFMA, name


def test_no_full_drain_inside_the_main_loop(kernels):
    for name, ins in kernels.items():
        n, bad = 0, []
        for i in ins:
            if i.startswith("v_mfma_"):
                n += 1
            elif 1 <= n < LAST_CHECKED and i.startswith("s_waitcnt") and "vmcnt(0)" in i:
                bad.append(n)
        assert not bad, f"{name}: s_waitcnt vmcnt(0) after MFMA {bad}"


def test_patch_dma_is_counted_at_the_prologue_barrier(kernels):
    """the first slice's DMAs have to be complete before any wave passes the prologue barrier: a vmcnt wait between the last of
    them and the barrier, and one that leaves the weight fragments (requested behind the DMAs) in flight"""
    for name, ins in kernels.items():
        first_mfma = next(k for k, i in enumerate(ins) if i.startswith("v_mfma_"))
        bar = max(k for k, i in enumerate(ins[:first_mfma]) if i.startswith("s_barrier"))
        dma = [k for k, i in enumerate(ins[:bar]) if re.match(r"buffer_load_dwordx4 .* lds$", i)]
        assert len(dma) == 14, (name, len(dma))
        assert not any(i.startswith("global_load_lds") for i in ins), name
        behind, covered = 0, False               # loads issued behind the last DMA: vmcnt retires in order
        for i in ins[dma[-1] + 1:bar]:
            m = re.search(r"vmcnt\((\d+)\)", i) if i.startswith("s_waitcnt") else None
            if m and int(m.group(1)) <= behind:
                covered = True
            elif re.match(r"(global|buffer|flat|scratch)_(load|store|atomic)", i):
                behind += 1
        assert covered, f"{name}: no vmcnt wait between the last patch DMA and the prologue barrier that covers the DMA"
