"""What the FFT's exchange read-back compiles to in the covariance kernels of the frames before the onset (no GPU
needed): the property of tests/test_cpu_mvdr_isa.py — the 32 reads of a component stand together and nothing but reads stands
between the first of them and their hand-placed wait.  mvdr_noise_k and mvdr_ring_noise_k transform forward: two read-backs each
(the real and the imaginary parts)."""
import os
import re
import subprocess
import sys

import pytest

from sed_crnn_amd import build as B

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_cpu_fft_exchange_isa import LGKM0, _hipcc, _read_runs  # noqa: E402
from test_cpu_mvdr_isa import SRC  # noqa: E402

READ_BACKS = {"mvdr_noise_k": 2, "mvdr_ring_noise_k": 2}


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    """kernel -> instructions in program order (test_cpu_mvdr_isa's parse, for this file's kernels)"""
    hipcc = _hipcc()
    if not hipcc:
        pytest.skip("hipcc not found")
    out = tmp_path_factory.mktemp("mvdr_noise_asm") / (SRC + ".s")
    cmd = [hipcc] + B.FLAGS + B.EXTRA_FLAGS.get(SRC, []) + ["-S", "--cuda-device-only", os.path.join(B.CSRC, SRC), "-o", str(out)]
    p = subprocess.run(cmd, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    fns, cur = {}, None
    for line in out.read_text().splitlines():
        m = re.match(r"^(_Z\w*(%s)\w*):" % "|".join(READ_BACKS), line)
        if m:
            assert m.group(2) not in fns, m.group(1)
            cur = fns.setdefault(m.group(2), [])
        elif line.startswith(".Lfunc_end"):
            cur = None
        elif cur is not None:
            s = line.split(";")[0].strip()
            if s and not s.startswith(".") and not s.endswith(":"):
                cur.append(s)
    return fns


@pytest.mark.parametrize("name", sorted(READ_BACKS))
def test_nothing_between_the_reads_and_their_wait(kernels, name):
    assert set(kernels) == set(READ_BACKS)
    ins = kernels[name]
    runs = [(at, n) for at, n in _read_runs(ins) if n == 32]
    assert len(runs) == READ_BACKS[name], (name, _read_runs(ins))
    for at, n in runs:
        wait = next(k for k in range(at, len(ins)) if LGKM0.match(ins[k]))
        between = [i for i in ins[at:wait] if not i.startswith("ds_read_b32 ")]
        assert not between, (name, between)
