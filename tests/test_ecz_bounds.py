"""CPU: the limb / column / value bounds of the signed 13 x 30-bit EC formulas (csrc/ecz.cuh) hold for the operand classes the kernels
pass (tools/ecz_bounds.py): every column total below 2^63, every value below 2^389, |product| < p wherever fz_is_zero looks, and the
accumulator invariant closed under madd, add, add_quad, dbl, dbl_affine -- and the checker refuses what must not pass."""
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_ecz_bounds_hold():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "ecz_bounds.py")], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "every contract of fz.cuh holds" in out.stdout and out.stdout.count("refused, as it must be") == 2
    worst = float(re.search(r"largest column total: ([\d.]+) \* 2\^58", out.stdout).group(1))
    assert worst < 32.0


def test_the_checked_modulus_is_the_generated_one():
    """constants.cuh (generated) carries the limb count, radix and balanced limbs of p that tools/ecz_bounds.py checks"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import ecz_bounds as E
    text = open(os.path.join(ROOT, "mpc-jellyfish_amd", "csrc", "constants.cuh")).read()
    body = text[text.index("struct BlsFqZ "):]
    body = body[:body.index("\n};")]
    assert int(re.search(r"ZN = (\d+);", body).group(1)) == E.N and int(re.search(r"ZL = (\d+);", body).group(1)) == E.L
    limbs = [int(v) for v in re.search(r"ZP\[\d+\] = \{([^}]*)\}", body).group(1).split(",")]
    assert sum(v << (E.L * i) for i, v in enumerate(limbs)) == E.P and [abs(v) for v in limbs] == E.P_ABS
    assert all(-(1 << 29) <= v < (1 << 29) for v in limbs)
    assert (int(re.search(r"ZINV = 0x([0-9a-f]+)u", body).group(1), 16) * E.P + 1) % (1 << E.L) == 0
