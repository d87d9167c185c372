"""What stands in front of the Winograd kernel's first patch request (no GPU needed: hipcc cross-compiles wino.hip to assembly).

A workgroup of conv3x3_wino_k can do nothing before its first 32-channel slice of the patch has arrived, so every instruction
ahead of the first `buffer_load_dwordx4 ... lds` is paid in full, 60 times per CU and training step.  The index math there is
reciprocal multiplies for the workgroup mapping and a carry per KiB block for the offsets (wino.hip: wino_workgroup, WinoWalk); the
closed form it replaced compiled to 671 - 678 instructions with 6 v_rcp and 14 exec-masked blocks (profiles/r10/README.md).  A
compiler update or an edit that brings a division, a branch around an offset or the epilogue's set-up back in front of the
request fails here."""
import os
import re
import shutil
import subprocess

import pytest

from sed_crnn_amd import build as B

PARENT_SMALLEST = 671    # instructions ahead of the first DMA before the change, the smallest of the five instantiations
# the five instantiations compile to 110 - 118 (profiles/r10/README.md); + 10 % of the largest for compiler drift — and in any
# case below half of what it was
BOUND = 129
assert BOUND < PARENT_SMALLEST / 2


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
    out = tmp_path_factory.mktemp("wino_prologue_asm") / "wino.s"
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
    assert len(fns) == 5, sorted(fns)
    return fns


def _dma(ins):
    return [k for k, i in enumerate(ins) if re.match(r"buffer_load_dwordx4 .* lds$", i)]


def test_nothing_but_scalar_and_carry_arithmetic_ahead_of_the_first_request(kernels):
    for name, ins in kernels.items():
        first = _dma(ins)[0]
        head = ins[:first]
        print(f"{name}: {first} instructions ahead of the first patch DMA")
        assert not [i for i in head if i.startswith("v_rcp_")], name
        assert not [i for i in head if i.startswith(("s_and_saveexec_b64", "s_cbranch_execz"))], name
        assert first <= BOUND, f"{name}: {first} instructions ahead of the first patch DMA (bound {BOUND})"


def test_the_walk_between_the_requests_has_no_division_or_masked_block(kernels):
    """the 13 carries sit between the requests: the same holds up to the last request of the first slice"""
    for name, ins in kernels.items():
        dma = _dma(ins)
        body = ins[:dma[13]]
        assert not [i for i in body if i.startswith("v_rcp_")], name
        assert not [i for i in body if i.startswith(("s_and_saveexec_b64", "s_cbranch_execz"))], name


def test_step_0_weight_fragments_directly_behind_the_requests(kernels):
    for name, ins in kernels.items():
        last = _dma(ins)[13]
        frag = next(k for k, i in enumerate(ins) if k > last and i.startswith("global_load_dwordx4"))
        print(f"{name}: first weight-fragment load {frag - last} instructions behind the 14th patch DMA")
        assert frag - last <= 16, f"{name}: first global_load_dwordx4 {frag - last} instructions behind the last patch DMA"
        assert not [i for i in ins[:last] if i.startswith("global_load_dwordx4")], f"{name}: a fragment load in front of a patch DMA"
