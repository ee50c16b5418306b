"""GPU: UnivariateKzgPCS.batch_open in one pass (mzk_kzg_open_batch_dev: csrc/poly.cuh "batched KZG opening") against the definition:
evaluation = p(z), proof = [(p(beta) - p(z)) / (beta - z)]G through the trapdoor, and against UnivariateKzgPCS.open for the same polynomial
and point.  The lengths sit on the edges of the scan: E = DIV_E coefficients a thread, B = DIV_BLOCK a workgroup, as csrc/poly.cuh defines
them.  Per curve the polynomials, their expected openings and the K = 9 result are computed once (the `world` fixture) and shared."""
import ctypes as C
import os
import random
import re

import numpy as np
import pytest

from conftest import ROOT, affine_from_limbs, fr_mont_limbs

pytestmark = pytest.mark.gpu

ERR_INVALID_ARG = -1
SEED = bytes(range(1, 33))


def _scan_constants():
    text = open(os.path.join(ROOT, "mpc-jellyfish_amd", "csrc", "poly.cuh")).read()
    threads = int(re.search(r"constexpr int POLY_THREADS = (\d+);", text).group(1))
    e = int(re.search(r"constexpr int DIV_E = (\d+);", text).group(1))
    assert re.search(r"constexpr int DIV_BLOCK = POLY_THREADS \* DIV_E;", text)
    return e, threads * e


E, B = _scan_constants()
LENGTHS = (1, 2, E, E + 1, B - 1, B, B + 1, 2 * B + 1, 3 * B + 5)


@pytest.fixture(scope="module")
def world(gpu, mj, pyref):
    out = {}
    for cid in (0, 1):
        c, pc = mj.params.CURVES[cid], pyref.CURVES[cid]
        r = pc.r
        rng = random.Random(7300 + cid)
        beta = rng.randrange(1, r)
        pp = mj.UnivariateProverParam.gen_srs_for_testing(c, beta, LENGTHS[-1] - 1)
        polys = [[rng.randrange(r) for _ in range(n)] for n in LENGTHS]
        polys[2] = [0] * E                                                 # the all-zero polynomial
        polys[3][0] = polys[3][1] = 0                                      # low-order zero coefficients
        polys[6][:B] = [0] * B                                             # ... a whole workgroup of them
        polys[7][B + 3] = polys[7][-1] = 0                                 # a zero inside, and a zero leading coefficient
        points = [rng.randrange(r), 0, rng.randrange(r), 1, r - 1, rng.randrange(r), 0, r - 1, 1]
        G = pyref.g1_gen(pc)
        want = []
        for p, z in zip(polys, points):
            ev = pyref.poly_eval(pc, p, z)
            q = (pyref.poly_eval(pc, p, beta) - ev) * pow(beta - z, -1, r) % r
            want.append((pyref.g1_mul(pc, q, G) if q else None, ev))
        mont = [fr_mont_limbs(pc, p) for p in polys]
        got = mj.UnivariateKzgPCS.batch_open(pp, mont, points)
        out[cid] = dict(c=c, pc=pc, beta=beta, pp=pp, polys=polys, mont=mont, points=points, want=want, got=got)
    yield out
    for w in out.values():
        w["pp"].release()


def _pt(pc, cm):
    return None if cm.is_infinity() else affine_from_limbs(pc, cm.xy)


@pytest.mark.parametrize("cid", [0, 1])
def test_the_ragged_batch_matches_the_definition_and_open(world, mj, cid):
    w = world[cid]
    pc, pp = w["pc"], w["pp"]
    proofs, evals = w["got"]
    assert len(proofs) == len(evals) == len(LENGTHS)
    for n, proof, ev, (want_pt, want_ev), m, z in zip(LENGTHS, proofs, evals, w["want"], w["mont"], w["points"]):
        assert ev == want_ev, n
        assert _pt(pc, proof) == want_pt, n
        one_proof, one_ev = mj.UnivariateKzgPCS.open(pp, m, z)
        assert one_proof == proof and one_ev == ev, n
    assert proofs[0].is_infinity() and proofs[2].is_infinity() and evals[2] == 0     # a constant; the zero polynomial


@pytest.mark.parametrize("cid", [0, 1])
def test_single_openings_and_device_resident_polynomials(world, mj, cid):
    """K = 1 at every length, from CUDA tensors (no staging), and an empty polynomial beside them"""
    import torch
    w = world[cid]
    pp = w["pp"]
    proofs, evals = w["got"]
    for i in range(len(LENGTHS)):
        t = torch.from_numpy(w["mont"][i].view(np.int64)).cuda()
        p1, e1 = mj.UnivariateKzgPCS.batch_open(pp, [t], [w["points"][i]])
        assert p1 == [proofs[i]] and e1 == [evals[i]], LENGTHS[i]
    empty = np.zeros((0, 4), dtype=np.uint64)
    p2, e2 = mj.UnivariateKzgPCS.batch_open(pp, [empty, w["mont"][4], empty], [5, w["points"][4], 0])
    assert p2[0].is_infinity() and p2[2].is_infinity() and e2[0] == e2[2] == 0 and (p2[1], e2[1]) == (proofs[4], evals[4])
    assert mj.UnivariateKzgPCS.batch_open(pp, [], []) == ([], [])


@pytest.mark.parametrize("cid", [0, 1])
def test_the_chunk_rule_changes_nothing(world, mj, cid, monkeypatch):
    """MZK_OPEN_BATCH_BUDGET below the batch's scratch: the polynomials go through in chunks (one larger than the budget alone)"""
    w = world[cid]
    L = mj.load()

    def launches():
        n = C.c_uint64()
        assert L.mzk_launch_count(C.byref(n)) == 0
        return n.value
    before = launches()
    whole = mj.UnivariateKzgPCS.batch_open(w["pp"], w["mont"], w["points"])
    in_one = launches() - before
    assert whole == w["got"]
    for budget in (32 * (B + 8) * 3, 1):                                   # about three workgroups' worth; every polynomial a chunk of its own
        monkeypatch.setenv("MZK_OPEN_BATCH_BUDGET", str(budget))
        before = launches()
        assert mj.UnivariateKzgPCS.batch_open(w["pp"], w["mont"], w["points"]) == w["got"], budget
        assert launches() - before > in_one, "more chunks, more launches"
    monkeypatch.delenv("MZK_OPEN_BATCH_BUDGET")


@pytest.mark.parametrize("cid", [0, 1])
def test_every_opening_is_accepted_by_batch_verify(world, mj, cid):
    w = world[cid]
    c, r = w["c"], w["pc"].r
    key = mj.keys.OpenKey(c, *mj.kzg.open_key_for_testing(c, w["beta"]))
    comms = mj.UnivariateKzgPCS.batch_commit(w["pp"], w["mont"])
    proofs, evals = w["got"]
    assert mj.UnivariateKzgPCS.batch_verify(key, comms, w["points"], evals, proofs, mj.rng.ChaChaRng(SEED, 20)) is True
    for cm, z, ev, pf in zip(comms, w["points"], evals, proofs):
        assert mj.UnivariateKzgPCS.verify(key, cm, z, ev, pf) is True
    wrong = list(evals)
    wrong[7] = (wrong[7] + 1) % r
    assert mj.UnivariateKzgPCS.batch_verify(key, comms, w["points"], wrong, proofs, mj.rng.ChaChaRng(SEED, 20)) is False
    key.release()


@pytest.mark.parametrize("cid", [0, 1])
def test_the_length_guard(world, mj, cid):
    import torch
    w = world[cid]
    pp, pc = w["pp"], w["pc"]
    n = pp.length + 3                                                      # a witness of degree pp.length + 1
    long = fr_mont_limbs(pc, [1] * n)
    with pytest.raises(mj.PCSError):
        mj.UnivariateKzgPCS.batch_open(pp, [w["mont"][1], long], [3, 4])
    padded = np.concatenate([w["mont"][8], np.zeros((5, 4), dtype=np.uint64)])         # trailing zeros beyond the key: the true degree decides
    p, e = mj.UnivariateKzgPCS.batch_open(pp, [padded], [w["points"][8]])
    assert (p[0], e[0]) == (w["got"][0][8], w["got"][1][8])
    # the entry point's own guard
    t = torch.from_numpy(long.view(np.int64)).cuda()
    L = mj.load()
    ptrs, lens = (C.c_void_p * 1)(t.data_ptr()), (C.c_uint64 * 1)(n)
    z, out_p, out_e = np.zeros(4, np.uint64), np.zeros(2 * pc.fq_limbs, np.uint64), np.zeros(4, np.uint64)
    ptr = lambda a: C.c_void_p(a.ctypes.data)
    assert L.mzk_kzg_open_batch_dev(pp.handle, 1, ptrs, lens, ptr(z), ptr(out_p), ptr(out_e), None) == ERR_INVALID_ARG
    assert b"larger than allowed" in L.mzk_last_error()
    with pytest.raises(mj.PCSError):
        mj.UnivariateKzgPCS.batch_open(pp, [w["mont"][0]], [1, 2])


def test_launches_do_not_grow_with_k(world, mj):
    """nine openings of one length share the three kernels and the fused MSM groups: far fewer launches than nine single calls"""
    w = world[1]
    L = mj.load()
    rng = random.Random(5)
    polys = [fr_mont_limbs(w["pc"], [rng.randrange(w["pc"].r) for _ in range(B + 1)]) for _ in range(9)]
    points = [rng.randrange(w["pc"].r) for _ in range(9)]

    def launches_of(k):
        mj.UnivariateKzgPCS.batch_open(w["pp"], polys[:k], points[:k])    # (the first call may build tables)
        n0, n1 = C.c_uint64(), C.c_uint64()
        assert L.mzk_launch_count(C.byref(n0)) == 0
        out = mj.UnivariateKzgPCS.batch_open(w["pp"], polys[:k], points[:k])
        assert L.mzk_launch_count(C.byref(n1)) == 0
        return n1.value - n0.value, out
    one, first = launches_of(1)
    nine, all_nine = launches_of(9)
    assert 0 < one and nine < 9 * one, (one, nine)
    assert (all_nine[0][0], all_nine[1][0]) == (first[0][0], first[1][0])
