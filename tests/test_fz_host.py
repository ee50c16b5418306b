"""CPU: csrc/fz.cuh and csrc/ecz.cuh -- BLS12-381 Fq on 13 signed 30-bit limbs and the XYZZ formulas over it, what every bucket
addition of the MSM runs -- compiled for the HOST (the headers are host/device code) and verified against Python big integers
(tools/fz_check.cpp prints the cases, tools/fz_check.py checks them): the products on random operands, every limb at +-2^29,
multiples of p up to the class bounds, 0, +-1, +-(p - 1); the carry rounds, the all-limbs-zero test, both boundary conversions; madd,
add and dbl with P = Q, P = -Q and infinity on either side against affine arithmetic.  Equality is exact.  The same program built
with the undefined-behaviour sanitizer aborts on a column sum that leaves 63 bits instead of wrapping."""
import os
import subprocess
import sys


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build_and_check(tmp_path, name, flags, cases):
    exe = str(tmp_path / name)
    subprocess.check_call(["g++", "-std=c++17", "-I", os.path.join(ROOT, "mpc-jellyfish_amd", "csrc"), os.path.join(ROOT, "tools", "fz_check.cpp"), "-o", exe] + flags)
    run = subprocess.run([exe, str(cases)], capture_output=True)
    assert run.returncode == 0, run.stderr.decode()[-3000:]
    assert not run.stderr, run.stderr.decode()[-3000:]
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "fz_check.py")], input=run.stdout, capture_output=True)
    assert out.returncode == 0, out.stderr.decode()[-2000:]
    assert b"lines ok" in out.stdout and (b"mul %d," % cases) in out.stdout, out.stdout
    return out.stdout.decode()


def test_fz_and_ecz_against_big_integers(tmp_path):
    _build_and_check(tmp_path, "fz_check", ["-O2"], 1500)


def test_fz_and_ecz_under_the_undefined_behaviour_sanitizer(tmp_path):
    """a stand-alone executable: a signed column sum beyond 63 bits, a limb sum beyond int32 or a bad shift ends the run"""
    _build_and_check(tmp_path, "fz_check_ubsan", ["-O1", "-g", "-fsanitize=undefined,signed-integer-overflow", "-fno-sanitize-recover=all"], 600)
