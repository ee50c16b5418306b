"""Bucket ranks over ALL bucket sets of an MSM (csrc/msm.cuh `order`, csrc/msm.hip rank_global -- round 6) against the oracle and
against the per-set ranks they replace (MZK_MSM_RANK_PER_SET=1), with and without a split tail.

`order` holds global bucket indices (w * M + b) and the consumers derive the window from the bucket, so per-set or global ranks are the
producers' business: msm_order_place_kernel on the two-level sort's paths, msm_order_hist / scan / scatter on the small plain path and
behind MZK_MSM_LEGACY_LAUNCHES=1.  The shapes are the smallest where the plain path has several bucket sets and a non-trivial rank0
(MZK_MSM_FORCE_TAIL=1 takes the tail branch below 2^20 pairs): BLS12-381 at 2^12 + 77 pairs from base 3 (window 10: 26 sets of 512
buckets) and BN254 at 2^13 pairs (window 11: 24 sets of 1024).  Every case is pinned by the trapdoor identity
commit(p) = [beta^off p(beta)]G computed with the C oracle; the schedules run in child processes (the switches are read once per
process) and must print the same affine points as the default.  The full-size schedules are tests/test_msm_tail_split_gpu.py's.

Which ranking kernels a case reaches: the two small plain-path shapes (no table, below the two-level sort's size) rank through
msm_order_hist / scan / scatter under every schedule, MZK_MSM_LEGACY_LAUNCHES=1 included; the fused table-path batches rank through
msm_order_place_kernel, which also registers the over-long and heavy buckets of the skewed batch (SKEW5 below).  The plain path at
2^20 / 2^21 pairs -- msm_order_place_kernel with 16 sets, skewed scalars included -- is tests/test_msm_tail_split_gpu.py's."""
import functools
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

_PRELUDE = r"""
import sys
import numpy as np
root = sys.argv[1]
for p in (root, root + "/oracle"):
    sys.path.insert(0, p)
import torch
import mpc_jellyfish_amd as mj
import cref
from importlib import import_module
lib = import_module("mpc-jellyfish_amd.lib")
lib.init(0)
L = mj.load()


def big(v):
    return np.array([[(v >> (64 * i)) & 0xffffffffffffffff for i in range(4)]], dtype=np.uint64)
"""

_PLAIN = _PRELUDE + r"""
L.mzk_msm_set_precompute(0)                       # the plain path: W windows x own bucket sets over the registered bases
for curve_id, n, off in ((0, (1 << 12) + 77, 3), (1, 1 << 13, 0)):
    c = mj.params.CURVES[curve_id]
    beta = 0x2b3c4d5e6f708192a3b4c5d6e7f8091a2b3c4d5e6f708192a3b4c5d6e7f8091a % c.r
    pp = mj.UnivariateProverParam.gen_srs_for_testing(curve_id, beta, n - 1 + off)
    beta_m = mj.params.fr_to_mont(c, [beta])[0]
    uniform = mj.params.random_fr_mont(c, n, seed=6100 + curve_id)
    skew = uniform.copy()
    skew[::2] = cref.fr_convert(curve_id, big(c.r - 2), True)[0]                # every second scalar r - 2: over-long buckets in every window
    small = uniform.copy()                                                      # the last 3/4 small counters: the high windows are empty
    vals = np.zeros((n - n // 4, 4), dtype=np.uint64)
    vals[:, 0] = np.arange(n - n // 4, dtype=np.uint64)
    small[n // 4:] = cref.fr_convert(curve_id, vals, True)
    zero = np.zeros_like(uniform)
    one = zero.copy()
    one[n // 3] = uniform[n // 3]
    assert np.any(one[n // 3])
    for name, sc in (("uniform", uniform), ("skew", skew), ("small_tail", small), ("zero", zero), ("one", one)):
        s = np.ascontiguousarray(sc)
        t = torch.from_numpy(s.view(np.int64)).cuda()
        L.mzk_profile_reset()
        L.mzk_profile_enable(1)
        jac = mj.msm_bigint(pp, t, scalars_are_mont=True, base_offset=off)
        L.mzk_profile_enable(0)
        comb = lib.profile_get("msm_split_combine")[1]
        c_bits, n_win, n_buckets = lib.msm_last_shape()
        aff = cref.jac_to_affine(curve_id, jac)[0]
        # trapdoor: sum_i s_i [beta^(off+i)]G = [beta^off p(beta)]G
        p_beta = cref.poly_eval(curve_id, s, beta_m)
        k = mj.params.limbs_to_int(cref.fr_convert(curve_id, p_beta.reshape(1, 4), False)[0]) * pow(beta, off, c.r) % c.r
        ok = bool(np.array_equal(aff, cref.g1_mul_gen(curve_id, k)))
        inf = int(not np.any(np.asarray(jac)[2]))                               # Jacobian Z == 0
        print("CASE", curve_id, name, c_bits, n_win, n_buckets, int(comb > 0), int(ok), inf, int(k == 0), aff.tobytes().hex())
    pp.release()
"""

# one fused table-path batch (msm_pre.cuh PreMulti: the bucket sets of the batch's MSMs side by side in one pass), each member against
# a single msm_bigint of the same scalars.  LENS is the batch the round-6 issue names; its 2^10 - 5 lies below the table path's least size,
# so that member runs on the plain path and cuts the batch in two -- LENS5 keeps all five on the table: one pass with five bucket sets;
# SKEW5 is LENS5 with skewed members (every second scalar r - 2, all scalars equal, small counters): the fused pass ranks through
# msm_order_place_kernel, so this is where its (w, b) registration of over-long and heavy buckets runs under global ranks in this file.
_BATCH = _PRELUDE + r"""
curve_id = 0
c = mj.params.CURVES[curve_id]
beta = 0x4d5e6f708192a3b4c5d6e7f8091a2b3c4d5e6f708192a3b4c5d6e7f8091a2b3c % c.r
pp = mj.UnivariateProverParam.gen_srs_for_testing(curve_id, beta, (1 << 12) - 1)
for tag, lens in (("LENS", (1 << 10, (1 << 10) - 5, 1 << 11, 1024, 1 << 12)), ("LENS5", (1 << 10, (1 << 10) + 5, 1 << 11, 1024, 1 << 12)),
                  ("SKEW5", (1 << 10, (1 << 10) + 5, 1 << 11, 1024, 1 << 12))):
    host = [mj.params.random_fr_mont(c, m, seed=6200 + i) for i, m in enumerate(lens)]
    if tag == "SKEW5":                                # over-long / heavy buckets and thin sets inside the fused pass
        host[2][::2] = cref.fr_convert(curve_id, big(c.r - 2), True)[0]         # every second scalar r - 2
        host[4][:] = host[4][7]                                                 # all scalars equal
        vals = np.zeros((lens[3] - lens[3] // 4, 4), dtype=np.uint64)
        vals[:, 0] = np.arange(len(vals), dtype=np.uint64)
        host[3][lens[3] // 4:] = cref.fr_convert(curve_id, vals, True)          # the last 3/4 small counters
    sets = [torch.from_numpy(np.ascontiguousarray(h).view(np.int64)).cuda() for h in host]
    jac = mj.msm_bigint_batch(pp, sets, scalars_are_mont=True)
    for i, t in enumerate(sets):
        aff = cref.jac_to_affine(curve_id, jac[i])[0]
        single = cref.jac_to_affine(curve_id, mj.msm_bigint(pp, t, scalars_are_mont=True))[0]
        print("CASE", tag, i, int(np.array_equal(aff, single)), aff.tobytes().hex())
pp.release()
"""

SHAPES = {0: (10, 26, 512), 1: (11, 24, 1024)}                # (window bits, bucket sets, buckets per set) of the two plain-path shapes
INPUTS = ("uniform", "skew", "small_tail", "zero", "one")

FORCE_TAIL = ({"MZK_MSM_FORCE_TAIL": "1", "MZK_MSM_TAIL_FRAC_LOG": "3", "MZK_MSM_TAIL_SPLIT": "2"},          # the last eighth, four ways
              {"MZK_MSM_FORCE_TAIL": "1", "MZK_MSM_TAIL_FRAC_LOG": "1", "MZK_MSM_TAIL_SPLIT": "3"},          # half of the ranks, eight ways
              {"MZK_MSM_FORCE_TAIL": "1", "MZK_MSM_TAIL_FRAC_LOG": "6", "MZK_MSM_TAIL_SPLIT": "1"})          # the last 1/64, halved
SCHEDULES = ({"MZK_MSM_RANK_PER_SET": "1"},) + FORCE_TAIL + (
    {"MZK_MSM_FORCE_TAIL": "1", "MZK_MSM_RANK_PER_SET": "1"},
    {"MZK_MSM_LEGACY_LAUNCHES": "1"},
    {"MZK_MSM_FORCE_SPLIT": "0"})
_SWITCHES = ("MZK_MSM_RANK_PER_SET", "MZK_MSM_FORCE_TAIL", "MZK_MSM_TAIL_FRAC_LOG", "MZK_MSM_TAIL_SPLIT", "MZK_MSM_LEGACY_LAUNCHES",
             "MZK_MSM_FORCE_SPLIT", "MZK_MSM_NO_TAIL_SPLIT", "MZK_MSM_MAX_SPLIT")


def _child(script, switches):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in _SWITCHES}
    env.update(switches)
    r = subprocess.run([sys.executable, "-c", script, root], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return [line.split() for line in r.stdout.split("\n") if line.startswith("CASE ")]


@functools.lru_cache(maxsize=None)
def _plain(switches):
    out = {}
    for f in _child(_PLAIN, dict(switches)):
        out[(int(f[1]), f[2])] = dict(shape=(int(f[3]), int(f[4]), int(f[5])), combined=int(f[6]), ok=int(f[7]), inf=int(f[8]), k_zero=int(f[9]), point=f[10])
    assert sorted(out) == sorted((cid, name) for cid in SHAPES for name in INPUTS), sorted(out)
    return out


@functools.lru_cache(maxsize=None)
def _batch(switches):
    out = {}
    for f in _child(_BATCH, dict(switches)):
        out[(f[1], int(f[2]))] = dict(same_as_single=int(f[3]), point=f[4])
    assert len(out) == 15, sorted(out)
    return out


def _key(switches):
    return tuple(sorted(switches.items()))


def test_default_schedule_agrees_with_the_oracle(gpu):
    for key, v in _plain(()).items():
        assert v["ok"] == 1, ("default schedule differs from [beta^off p(beta)]G", key)
        assert v["shape"] == SHAPES[key[0]], ("not the several-set plain path the case is meant for", key, v["shape"])
        assert v["inf"] == v["k_zero"], key
        if key[1] == "zero":
            assert v["inf"] == 1, key
        if key[1] in ("uniform", "skew", "one"):
            assert v["inf"] == 0, key


@pytest.mark.parametrize("switches", SCHEDULES, ids=lambda s: ",".join("%s=%s" % (k[8:], v) for k, v in s.items()))
def test_schedule_gives_the_default_point_and_the_oracle_point(gpu, switches):
    default, other = _plain(()), _plain(_key(switches))
    for key, v in other.items():
        assert v["ok"] == 1, (switches, key)
        assert v["shape"] == SHAPES[key[0]], (switches, key, v["shape"])
        assert v["point"] == default[key]["point"], (switches, key)
    if "MZK_MSM_FORCE_TAIL" in switches:                      # the tail branch ran: its combine launch is on the profile
        assert all(v["combined"] == 1 for v in other.values()), switches
    if "MZK_MSM_FORCE_SPLIT" in switches:                     # whole-bucket threads everywhere
        assert all(v["combined"] == 0 for v in other.values()), switches


def test_fused_table_path_batch_ranked_globally_and_per_set(gpu):
    default, per_set = _batch(()), _batch(_key({"MZK_MSM_RANK_PER_SET": "1"}))
    for key, v in default.items():
        assert v["same_as_single"] == 1, ("default", key)
        assert per_set[key]["same_as_single"] == 1, ("per set", key)
        assert per_set[key]["point"] == v["point"], key
