"""GPU: BLS12-381's MSM on the signed 13 x 30-bit limb field (csrc/fz.cuh, ecz.cuh, EcFz in msm.cuh) against the C oracle the other MSM
tests use.  The variable-base path at sizes that are one thread's work, at 1023 and at 2^16 pairs (the two-level sort; once more in a
child process with the split tail and its combine forced), the table path at 2^12 and a fused batch of five at 2^10; scalars uniform, all
0, all 1, all r - 1 and all equal (heavy buckets: the rare-path kernels' add and the quad levels see real operands); a point list that
repeats a point and holds its negative under equal scalars (the doubling and the P = -Q branch of the accumulation); and the fixed-base
table of a 2^12-point SRS against the variable-base path."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CURVE = 0
EQUAL = 0x5a3c9e1f7b2d4c6a8e0f1a2b3c4d5e6f708192a3b4c5d6e7f8091a2b3c4d5e


def _bigints(scalars):
    return np.array([[(s >> (64 * j)) & 0xFFFFFFFFFFFFFFFF for j in range(4)] for s in scalars], dtype=np.uint64).reshape(-1, 4)


def _scalar_sets(mj, n, seed):
    c = mj.params.CURVES[CURVE]
    rng = np.random.default_rng(seed)
    uniform = _bigints([int.from_bytes(rng.bytes(32), "little") % c.r for _ in range(n)])
    rep = lambda v: np.repeat(_bigints([v]), n, axis=0)
    return (("uniform", uniform), ("zero", rep(0)), ("one", rep(1)), ("r-1", rep(c.r - 1)), ("equal", rep(EQUAL % c.r)))


def _affine(cref, jac):
    return cref.jac_to_affine(CURVE, jac)[0]


@pytest.fixture(scope="module")
def bases(cref):
    return cref.g1_arith_bases(CURVE, 0x13572468ace, 0x31, 1 << 16)


@pytest.fixture()
def precompute(gpu):
    from mpc_jellyfish_amd import lib as mlib
    L = mlib.ensure_init()
    yield L.mzk_msm_set_precompute
    L.mzk_msm_set_precompute(1)


@pytest.mark.parametrize("n", [1, 2, 3, 1023])
def test_variable_base_small_sizes_and_scalar_kinds(gpu, mj, cref, bases, precompute, n):
    precompute(0)
    pp = mj.UnivariateProverParam.from_affine(CURVE, bases[:n])
    for kind, s in _scalar_sets(mj, n, 100 + n):
        want = _affine(cref, cref.msm(CURVE, bases[:n], s, threads=8))
        assert np.array_equal(_affine(cref, mj.msm_bigint(pp, s)), want), (n, kind)
    pp.release()


_CHILD = r"""
import sys
import numpy as np
root = sys.argv[1]
for p in (root, root + "/oracle"):
    sys.path.insert(0, p)
import mpc_jellyfish_amd as mj
import cref
from importlib import import_module
import_module("mpc-jellyfish_amd.lib").init(0)
L = mj.load()
L.mzk_msm_set_precompute(0)
n = 1 << 16
bases = cref.g1_arith_bases(0, 0x13572468ace, 0x31, n)
scalars = np.load(sys.argv[2])
pp = mj.UnivariateProverParam.from_affine(0, bases)
L.mzk_profile_reset()
L.mzk_profile_enable(1)
jac = mj.msm_bigint(pp, scalars)
L.mzk_profile_enable(0)
comb = import_module("mpc-jellyfish_amd.lib").profile_get("msm_split_combine")[1]
print("POINT", int(comb > 0), cref.jac_to_affine(0, jac)[0].tobytes().hex())
pp.release()
"""


def test_variable_base_two_level_sort_and_forced_tail(gpu, mj, cref, bases, precompute, tmp_path):
    n = 1 << 16
    precompute(0)
    s = _scalar_sets(mj, n, 7)[0][1]
    want = _affine(cref, cref.msm(CURVE, bases, s, threads=8))
    pp = mj.UnivariateProverParam.from_affine(CURVE, bases)
    assert np.array_equal(_affine(cref, mj.msm_bigint(pp, s)), want)
    pp.release()
    # the split tail and its combine launch, in a fresh process (the switch is read once)
    path = str(tmp_path / "scalars.npy")
    np.save(path, s)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", _CHILD, root, path], env=dict(os.environ, MZK_MSM_FORCE_TAIL="1"), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    line = [l.split() for l in r.stdout.split("\n") if l.startswith("POINT")]
    assert len(line) == 1, r.stdout[-2000:]
    assert line[0][1] == "1", "the split tail's combine launch did not run"
    assert line[0][2] == want.tobytes().hex()


def test_table_path_and_scalar_kinds(gpu, mj, cref, bases, precompute):
    n = 1 << 12
    precompute(1)
    pp = mj.UnivariateProverParam.from_affine(CURVE, bases[:n])
    for kind, s in _scalar_sets(mj, n, 12):
        want = _affine(cref, cref.msm(CURVE, bases[:n], s, threads=8))
        assert np.array_equal(_affine(cref, mj.msm_bigint(pp, s)), want), kind
    pp.release()


def test_fused_batch_of_five(gpu, mj, cref, bases, precompute):
    n = 1 << 10
    precompute(1)
    c = mj.params.CURVES[CURVE]
    pp = mj.UnivariateProverParam.from_affine(CURVE, bases[:n])
    sets = _scalar_sets(mj, n, 5)
    polys = [cref.fr_convert(CURVE, s, True) for _, s in sets]                     # coefficients are Montgomery images
    coms = mj.UnivariateKzgPCS.batch_commit(pp, polys)
    assert len(coms) == 5
    for (kind, s), com in zip(sets, coms):
        want = _affine(cref, cref.msm(CURVE, bases[:n], s, threads=8))
        if com.is_infinity():
            assert not want.any(), kind
        else:
            assert np.array_equal(np.asarray(com.xy).reshape(want.shape), want), kind
    pp.release()


@pytest.mark.parametrize("table", [0, 1])
def test_repeated_and_negated_points_under_equal_scalars(gpu, mj, cref, bases, precompute, table):
    """a bucket's run holds P, P, -P, Q, -Q, ...: the accumulation doubles, steps back, and passes through infinity on the device"""
    n = 1024
    c = mj.params.CURVES[CURVE]
    pts = bases[:n].copy()
    for i in range(0, n - 8, 8):
        pts[i + 1] = pts[i]
        pts[i + 2] = cref.g1_mul(CURVE, pts[i], c.r - 1)
        pts[i + 5] = cref.g1_mul(CURVE, pts[i + 4], c.r - 1)
        pts[i + 6] = pts[i + 4]
        pts[i + 7] = pts[i + 4]
    precompute(table)
    pp = mj.UnivariateProverParam.from_affine(CURVE, pts)
    for v in (EQUAL % c.r, 1, c.r - 1, 0x8001):
        s = np.repeat(_bigints([v]), n, axis=0)
        want = _affine(cref, cref.msm(CURVE, pts, s, threads=8))
        assert np.array_equal(_affine(cref, mj.msm_bigint(pp, s)), want), (table, hex(v))
    pp.release()


def test_fixed_base_table_agrees_with_the_variable_base_path(gpu, mj, cref, precompute):
    n = 1 << 12
    pp = mj.UnivariateProverParam.gen_srs_for_testing(CURVE, 0x1f2e3d4c5b6a7988, n - 1)
    srs = pp.powers_of_g()
    s = _scalar_sets(mj, n, 99)[0][1]
    precompute(1)
    with_table = _affine(cref, mj.msm_bigint(pp, s))
    precompute(0)
    plain = _affine(cref, mj.msm_bigint(pp, s))
    assert np.array_equal(with_table, plain)
    assert np.array_equal(plain, _affine(cref, cref.msm(CURVE, srs, s, threads=8)))
    pp.release()
