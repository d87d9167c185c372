"""What the FFT's exchange read-back compiles to (no GPU needed: hipcc cross-compiles the kernels to assembly).

exchange_load (fft2048.h) reads the 32 values of one component back from LDS with 32 single asm statements and waits for them
with a hand-placed s_waitcnt lgkmcnt(0).  To the compiler every read's output is valid the moment its statement ends, so
anything it places between a read and the wait that touches a destination — a v_mov, a spill, a copy to an AGPR — would capture
stale data, and no numerical test is certain to notice.  The property the wait relies on is therefore asserted on the compiled
code of every kernel that transforms: the reads of a component stand together, and nothing but reads stands between the first
of them and the wait.  It holds today; the test is there for the compiler update or the extra live value that changes it."""
import os
import re
import shutil
import subprocess

import pytest

from sed_crnn_amd import build as B

# file -> (kernel, instantiations the file compiles)
KERNELS = {"logmel.hip": ("logmel_fft_k", 12), "gcc.hip": ("gcc_phat_k", 1), "tdoa.hip": ("tdoa_accum_k", 2)}
LGKM0 = re.compile(r"^s_waitcnt\b.*\blgkmcnt\(0\)")


def _hipcc():
    try:
        c = B._hipcc()
    except RuntimeError:
        return None
    return c if os.path.isabs(c) else shutil.which(c)


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    """file -> {mangled name: instructions in program order}"""
    hipcc = _hipcc()
    if not hipcc:
        pytest.skip("hipcc not found")
    tmp = tmp_path_factory.mktemp("fft_asm")
    procs = []
    for src in KERNELS:
        out = tmp / (src + ".s")
        cmd = [hipcc] + B.FLAGS + B.EXTRA_FLAGS.get(src, []) + ["-S", "--cuda-device-only", os.path.join(B.CSRC, src), "-o", str(out)]
        procs.append((src, out, subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)))
    found = {}
    for src, out, p in procs:
        _, err = p.communicate()
        assert p.returncode == 0, err
        fns, cur = {}, None
        for line in out.read_text().splitlines():
            m = re.match(r"^(_Z\w*%s\w*):" % KERNELS[src][0], line)
            if m:
                cur = fns.setdefault(m.group(1), [])
            elif line.startswith(".Lfunc_end"):
                cur = None
            elif cur is not None:
                s = line.split(";")[0].strip()
                if s and not s.startswith(".") and not s.endswith(":"):
                    cur.append(s)
        found[src] = fns
    return found


def _read_runs(ins):
    """[(index of the first read, number of reads)] of every maximal run of consecutive ds_read_b32"""
    runs, i = [], 0
    while i < len(ins):
        if ins[i].startswith("ds_read_b32 "):
            j = i
            while j < len(ins) and ins[j].startswith("ds_read_b32 "):
                j += 1
            runs.append((i, j - i))
            i = j
        else:
            i += 1
    return runs


@pytest.mark.parametrize("src", sorted(KERNELS))
def test_every_kernel_was_found(kernels, src):
    name, count = KERNELS[src]
    assert len(kernels[src]) == count, (name, sorted(kernels[src]))


@pytest.mark.parametrize("src", sorted(KERNELS))
def test_nothing_between_the_reads_and_their_wait(kernels, src):
    assert kernels[src]
    for name, ins in kernels[src].items():
        runs = [(at, n) for at, n in _read_runs(ins) if n == 32]
        assert len(runs) == 2, (name, _read_runs(ins))
        for at, n in runs:
            wait = next(k for k in range(at, len(ins)) if LGKM0.match(ins[k]))
            between = [i for i in ins[at:wait] if not i.startswith("ds_read_b32 ")]
            assert not between, (name, between)
