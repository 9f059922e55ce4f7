"""CPU: div_small (lzm_numerics.h), the three-operation quotient x / d for d in {1, 2, 3} of the
two-action mean-q chain, restated on the host in tools/div_small_check.c and compared bit for bit
with the division: every 251st of the 2^32 patterns of x, every pattern with exponent field 0, 1,
254 or 255 (zeros and subnormals, the smallest normals, the largest finite values, infinities and
NaNs), and +-0, +-inf and a NaN by name. The program's exhaustive mode (all 2^32 patterns, each
divisor) is recorded in profiles/settle_lanes/div_small_exhaustive.txt. Built -ffp-contract=off,
as the library is."""
import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_strided_sweep_has_no_mismatch(tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    if cc is None:
        pytest.fail("no C compiler (cc, gcc, clang) on PATH")
    exe = str(tmp_path / "div_small_check")
    src = os.path.join(REPO, "tools", "div_small_check.c")
    # with OpenMP where the compiler has it (subnormal operands are slow on the host: the sweep takes half a
    # minute on one CPU), else serial
    if subprocess.call([cc, "-O2", "-ffp-contract=off", "-fopenmp", "-o", exe, src, "-lm"], stderr=subprocess.DEVNULL) != 0:
        subprocess.check_call([cc, "-O2", "-ffp-contract=off", "-o", exe, src, "-lm"])
    r = subprocess.run([exe, "--strided"], stdout=subprocess.PIPE, universal_newlines=True)
    print(r.stdout)
    lines = r.stdout.strip().splitlines()
    assert r.returncode == 0, r.stdout
    assert lines[-1] == "mismatches 0"
    per_d = [l for l in lines if l.startswith("d ")]
    assert len(per_d) == 3
    n = (1 << 32) // 251 + 1 + 8 * (1 << 23) + 5
    for d, l in zip((1, 2, 3), per_d):
        assert l.startswith(f"d {d}: {n} patterns, 0 mismatches"), l
