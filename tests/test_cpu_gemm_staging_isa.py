"""What the fp32 GEMM's K loop compiles to (no GPU needed: hipcc cross-compiles gemm.hip to assembly).

gemm_f32_k stages either kind of operand into one k-contiguous LDS image, so every fragment is one ds_read_b128, and its FULL
path addresses global memory with a scalar base and a 32-bit lane offset.  Both are properties of the compiled loop, not of
the result: hipcc's loop strength reduction folds base + offset back into per-lane 64-bit pointers (two vector adds per load
and step) unless it is kept from it, and a fragment gathered with four 4-byte reads computes the same bits.  A compiler
update that undoes either fails here instead of costing a few per cent of three GEMMs unnoticed (profiles/r7).  The three
instantiations are the ones a fit step of the bench workload launches: the layer-0 weight gradient, data gradient and forward
projection of the GRU."""
import os
import re
import shutil
import subprocess

import pytest

from sed_crnn_amd import build as B

# (WVM, WVN, WM, WN, A_KC, B_KC)
WORKLOAD = [(2, 2, 2, 2, False, False), (2, 2, 2, 2, True, False), (4, 1, 1, 3, True, True)]
ADD64 = re.compile(r"v_(lshl_add_u64|add_u64|add_co_u32|addc_co_u32|mad_u64_u32|mad_i64_i32)\b")


def _hipcc():
    try:
        c = B._hipcc()
    except RuntimeError:
        return None
    return c if os.path.isabs(c) else shutil.which(c)


def _mangled(cfg):
    wvm, wvn, wm, wn, akc, bkc = cfg
    return f"gemm_f32_kILi{wvm}ELi{wvn}ELi{wm}ELi{wn}ELb{int(akc)}ELb{int(bkc)}EE"


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    """mangled name -> list of (label, instructions) basic blocks"""
    hipcc = _hipcc()
    if not hipcc:
        pytest.skip("hipcc not found")
    out = tmp_path_factory.mktemp("gemm_asm") / "gemm.s"
    cmd = [hipcc] + B.FLAGS + ["-S", "--cuda-device-only", os.path.join(B.CSRC, "gemm.hip"), "-o", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    fns, cur = {}, None
    for line in out.read_text().splitlines():
        m = re.match(r"^(_Z\w*gemm_f32_k\w*):", line)
        if m:
            cur = fns.setdefault(m.group(1), [(None, [])])
        elif line.startswith(".Lfunc_end"):
            cur = None
        elif cur is not None:
            m = re.match(r"^(\.LBB\d+_\d+):", line)
            if m:
                cur.append((m.group(1), []))
                continue
            s = line.split(";")[0].strip()
            if s and not s.startswith("."):
                cur[-1][1].append(s)
                if s.startswith(("s_cbranch", "s_branch")):          # what follows a branch is a block of its own
                    cur.append((None, []))
    return fns


def _kernel(kernels, cfg):
    hits = [v for k, v in kernels.items() if _mangled(cfg) in k]
    assert len(hits) == 1, (cfg, sorted(kernels))
    return hits[0]


def _count(ins, prefix):
    return sum(i.startswith(prefix) for i in ins)


def _full_steady_loop(blocks, cfg):
    """the FULL path's steady state is branch-free: the one basic block that branches back to its own label and holds the
    MFMAs of a whole K-step (the guarded loop is cut into many blocks by its range tests)"""
    n_mfma = 16 * cfg[2] * cfg[3]
    loops = [ins for label, ins in blocks
             if label and ins and ins[-1].startswith("s_cbranch") and ins[-1].split()[-1] == label and _count(ins, "v_mfma_f32_32x32x2") == n_mfma]
    assert len(loops) == 1, (cfg, len(loops))
    return loops[0]


@pytest.mark.parametrize("cfg", WORKLOAD, ids=_mangled)
def test_every_fragment_is_one_b128_read(kernels, cfg):
    ins = [i for _, b in _kernel(kernels, cfg) for i in b]
    reads = [i.split()[0] for i in ins if i.startswith("ds_read")]
    assert reads and set(reads) == {"ds_read_b128"}, sorted(set(reads))


@pytest.mark.parametrize("cfg", WORKLOAD, ids=_mangled)
def test_reads_per_steady_state_step(kernels, cfg):
    blocks = _kernel(kernels, cfg)
    want = 4 * (cfg[2] + cfg[3])
    assert _count(_full_steady_loop(blocks, cfg), "ds_read_b128") == want
    # every block that holds a whole step's MFMAs (guarded loop, two-step tail) reads the same fragments
    n_mfma = 16 * cfg[2] * cfg[3]
    steps = [ins for _, ins in blocks if _count(ins, "v_mfma_f32_32x32x2") == n_mfma]
    assert len(steps) >= 2
    for ins in steps:
        assert _count(ins, "ds_read_b128") == want


@pytest.mark.parametrize("cfg", WORKLOAD, ids=_mangled)
def test_full_loop_has_no_vector_address_arithmetic(kernels, cfg):
    loop = _full_steady_loop(_kernel(kernels, cfg), cfg)
    bad = [i for i in loop if ADD64.match(i)]
    assert not bad, bad
    loads = [i for i in loop if i.startswith(("global_load", "flat_load", "buffer_load"))]
    n_a = cfg[2] * cfg[0] if cfg[4] else 4              # float4 per thread: BM / 32 of a k-contiguous operand, one 4 x 4 block otherwise
    n_b = cfg[3] * cfg[1] if cfg[5] else 4
    assert len(loads) == n_a + n_b, loads
    for i in loads:                                     # scalar base + 32-bit lane offset
        assert re.match(r"global_load_dwordx4 v\[\d+:\d+\], v\d+, s\[\d+:\d+\]", i), i
