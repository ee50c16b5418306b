"""GPU: UnivariateKzgPCS.multi_open_rou (FK23 on the device, mzk_kzg_multi_open_rou_dev: csrc/kzg_multi.hip) against the definition: at every
returned point i the evaluation is p(w^i) and the proof is [(p(beta) - p(w^i)) / (beta - w^i)]G through the trapdoor of the testing SRS -- no
FK23 on the test's side -- and against UnivariateKzgPCS.batch_open at the same points.  The lengths sit on the edges of the padding
(d = next_power_of_two(len - 1)) and at 2T + 1, T the workgroup of the group-NTT kernels as csrc/ec_ntt.cuh defines it: there both
transforms of size 2d have butterflies in more than one workgroup.  Per curve the SRS, the cases and their expected openings are computed
once (the `world` fixture) and shared."""
import ctypes as C
import os
import random
import re

import numpy as np
import pytest

from conftest import ROOT, affine_from_limbs, fr_mont_limbs

pytestmark = pytest.mark.gpu

ERR_INVALID_ARG, ERR_UNSUPPORTED = -1, -5
SEED = bytes(range(1, 33))


def _ntt_threads():
    text = open(os.path.join(ROOT, "mpc-jellyfish_amd", "csrc", "ec_ntt.cuh")).read()
    return int(re.search(r"constexpr int EC_NTT_THREADS = (\d+);", text).group(1))


T = _ntt_threads()
SMALL = (0, 1, 2, 3, 4, 5, 8, 9, 17)
BIG = 2 * T + 1
PADDED = {0: 1, 1: 1, 2: 1, 3: 2, 4: 4, 5: 4, 8: 8, 9: 8, 17: 16, BIG: 2 * T}        # d per length


def _pt(pc, cm):
    return None if cm.is_infinity() else affine_from_limbs(pc, cm.xy)


def _want(pyref, pc, beta, poly, log_n, indices, shift=0):
    """[(proof point, evaluation)] at w^i by the trapdoor; shift: the basis starts at beta^shift G"""
    r, G, w = pc.r, pyref.g1_gen(pc), pc.root_of_unity(log_n)
    at_beta, scale = pyref.poly_eval(pc, poly, beta), pow(beta, shift, pc.r)
    out = []
    for i in indices:
        x = pow(w, i, r)
        ev = pyref.poly_eval(pc, poly, x)
        q = (at_beta - ev) * pow(beta - x, -1, r) * scale % r
        out.append((pyref.g1_mul(pc, q, G) if q else None, ev))
    return out


@pytest.fixture(scope="module")
def world(gpu, mj, pyref):
    out = {}
    for cid in (0, 1):
        c, pc = mj.params.CURVES[cid], pyref.CURVES[cid]
        r = pc.r
        rng = random.Random(7400 + cid)
        beta = rng.randrange(1, r)
        pp = mj.UnivariateProverParam.gen_srs_for_testing(c, beta, 2 * T)
        cases = {}

        def add(name, poly, log_n, num_points, indices=None):
            dom = mj.Radix2EvaluationDomain(c, log_n)
            mont = fr_mont_limbs(pc, poly) if poly else np.zeros((0, 4), dtype=np.uint64)
            got = mj.UnivariateKzgPCS.multi_open_rou(pp, mont, num_points, dom)
            k = min(num_points, dom.size)
            idx = list(range(k)) if indices is None else indices
            cases[name] = dict(poly=poly, mont=mont, dom=dom, got=got, k=k, idx=idx, want=_want(pyref, pc, beta, poly, log_n, idx))

        for n in SMALL:                                                    # N = 2d, every point
            log_n = PADDED[n].bit_length()
            add(("len", n), [rng.randrange(r) for _ in range(n)], log_n, 1 << log_n)
        n_big = 4 * T
        sample = sorted({0, 1, n_big // 2, n_big - 1} | set(random.Random(11).sample(range(n_big), 32)))
        add(("len", BIG), [rng.randrange(r) for _ in range(BIG)], n_big.bit_length() - 1, n_big, sample)
        add("zero", [0] * 8, 4, 16)
        add("low zeros", [0, 0, 0] + [rng.randrange(r) for _ in range(6)], 4, 16)
        five = [rng.randrange(r) for _ in range(5)]
        add("five in 16", five, 4, 16)
        add("five, trailing zeros", five + [0] * 4, 4, 16)                 # len 9: d = 8 instead of 4
        add("five in 32", five, 5, 30)                                     # N = 32 > 2d = 8
        nine = [rng.randrange(r) for _ in range(9)]
        for k in (0, 1, 16, 19):
            add(("nine", k), nine, 4, k)
        out[cid] = dict(c=c, pc=pc, beta=beta, pp=pp, cases=cases)
    yield out
    for w in out.values():
        w["pp"].release()


def _check(w, name):
    pc, case = w["pc"], w["cases"][name]
    proofs, evals = case["got"]
    assert len(proofs) == len(evals) == case["k"], name
    for i, (want_pt, want_ev) in zip(case["idx"], case["want"]):
        assert evals[i] == want_ev, (name, i)
        assert _pt(pc, proofs[i]) == want_pt, (name, i)


@pytest.mark.parametrize("cid", [0, 1])
@pytest.mark.parametrize("n", SMALL)
def test_every_point_matches_the_definition(world, cid, n):
    w = world[cid]
    case = w["cases"][("len", n)]
    assert case["dom"].size == 2 * PADDED[n] and case["k"] == case["dom"].size
    _check(w, ("len", n))
    if n <= 1:                                                             # no polynomial, a constant: the zero witness; 0 and c_0
        assert all(p.is_infinity() for p in case["got"][0]) and set(case["got"][1]) == {case["poly"][0] if n else 0}


@pytest.mark.parametrize("cid", [0, 1])
def test_transforms_wider_than_one_workgroup(world, cid):
    """len = 2T + 1: 2d = 4T points, 2T butterflies a stage"""
    w = world[cid]
    case = w["cases"][("len", BIG)]
    assert PADDED[BIG] == 2 * T and case["dom"].size == 4 * T and len(case["idx"]) >= 32 and {0, 1, 2 * T, 4 * T - 1} <= set(case["idx"])
    _check(w, ("len", BIG))


@pytest.mark.parametrize("cid", [0, 1])
def test_contents_domains_and_point_counts(world, mj, cid):
    w = world[cid]
    cases = w["cases"]
    for name in ("zero", "low zeros", "five in 16", "five, trailing zeros", "five in 32", ("nine", 0), ("nine", 1), ("nine", 16), ("nine", 19)):
        _check(w, name)
    assert all(p.is_infinity() for p in cases["zero"]["got"][0]) and set(cases["zero"]["got"][1]) == {0}
    assert cases["five, trailing zeros"]["got"] == cases["five in 16"]["got"]          # the untrimmed polynomial at a larger d: the same openings
    dom = mj.UnivariateKzgPCS.multi_open_rou_eval_domain(w["c"], 4, 30)
    assert dom.size == 32 == cases["five in 32"]["dom"].size and cases["five in 32"]["k"] == 30
    assert [cases[("nine", k)]["k"] for k in (0, 1, 16, 19)] == [0, 1, 16, 16]         # N + 3 is clamped to N
    full = cases[("nine", 16)]["got"]
    assert cases[("nine", 19)]["got"] == full and cases[("nine", 1)]["got"] == ([full[0][0]], [full[1][0]])
    assert cases[("nine", 0)]["got"] == ([], [])


@pytest.mark.parametrize("cid", [0, 1])
def test_every_opening_equals_batch_open(world, mj, cid):
    w = world[cid]
    pc, pp = w["pc"], w["pp"]
    for name, case in w["cases"].items():
        k = case["k"]
        if k == 0:
            continue
        root = pc.root_of_unity(case["dom"].log_size_of_group)
        points = [pow(root, i, pc.r) for i in range(k)]
        assert mj.UnivariateKzgPCS.batch_open(pp, [case["mont"]] * k, points) == case["got"], name


@pytest.mark.parametrize("cid", [0, 1])
def test_proofs_alone_evaluations_alone_and_device_input(world, mj, cid):
    import torch
    w = world[cid]
    K = mj.UnivariateKzgPCS
    for name in (("len", 17), "five in 32", ("len", 1), ("len", 0)):
        case = w["cases"][name]
        proofs, evals = case["got"]
        assert K.multi_open_rou_proofs(w["pp"], case["mont"], case["k"], case["dom"]) == proofs, name
        assert K.multi_open_rou_evals(case["mont"], case["k"], case["dom"]) == evals, name
        t = torch.from_numpy(case["mont"].view(np.int64)).cuda()
        assert K.multi_open_rou(w["pp"], t, case["k"], case["dom"]) == case["got"], name
        assert K.multi_open_rou_evals(t, case["k"], case["dom"]) == evals, name


@pytest.mark.parametrize("cid", [0, 1])
def test_batch_verify_accepts_the_openings_and_rejects_a_changed_value(world, mj, cid):
    w = world[cid]
    c, pc = w["c"], w["pc"]
    case = w["cases"][("len", 17)]
    proofs, evals = case["got"]
    k = case["k"]
    root = pc.root_of_unity(case["dom"].log_size_of_group)
    points = [pow(root, i, pc.r) for i in range(k)]
    key = mj.keys.OpenKey(c, *mj.kzg.open_key_for_testing(c, w["beta"]))
    comms = [mj.UnivariateKzgPCS.commit(w["pp"], case["mont"])] * k
    assert mj.UnivariateKzgPCS.batch_verify(key, comms, points, evals, proofs, mj.rng.ChaChaRng(SEED, 20)) is True
    wrong = list(evals)
    wrong[k // 2] = (wrong[k // 2] + 1) % pc.r
    assert mj.UnivariateKzgPCS.batch_verify(key, comms, points, wrong, proofs, mj.rng.ChaChaRng(SEED, 20)) is False
    key.release()


def _launches(L):
    n = C.c_uint64()
    assert L.mzk_launch_count(C.byref(n)) == 0
    return n.value


def _table_bytes(L, pp):
    pts, tab = C.c_uint64(), C.c_uint64()
    assert L.mzk_srs_hbm_bytes(pp.handle, C.byref(pts), C.byref(tab)) == 0
    return tab.value


@pytest.mark.parametrize("cid", [0, 1])
def test_the_transformed_srs_is_kept_on_the_handle(world, mj, cid):
    """a second call at the same (SRS, d) skips step A: the same output from fewer launches; the table is counted and goes with the handle"""
    w = world[cid]
    c = w["c"]
    L = mj.load()
    case = w["cases"][("len", 17)]
    K = mj.UnivariateKzgPCS
    pp = mj.UnivariateProverParam.gen_srs_for_testing(c, w["beta"], 16)
    assert _table_bytes(L, pp) == 0
    n0 = _launches(L)
    first = K.multi_open_rou(pp, case["mont"], case["k"], case["dom"])
    n1 = _launches(L)
    second = K.multi_open_rou(pp, case["mont"], case["k"], case["dom"])
    n2 = _launches(L)
    assert first == second == case["got"]
    assert 0 < n2 - n1 < n1 - n0, (n1 - n0, n2 - n1)
    assert _table_bytes(L, pp) == 2 * 16 * (224 if cid == 0 else 144)          # 2d XYZZ points in the group NTT's form
    other = w["cases"][("len", 9)]                                         # another d on the same handle replaces the table
    assert K.multi_open_rou(pp, other["mont"], other["k"], other["dom"]) == other["got"]
    assert _table_bytes(L, pp) == 2 * 8 * (224 if cid == 0 else 144)
    pp.release()
    fresh = mj.UnivariateProverParam.gen_srs_for_testing(c, w["beta"], 16)
    assert K.multi_open_rou(fresh, case["mont"], case["k"], case["dom"]) == case["got"]
    fresh.release()


@pytest.mark.parametrize("cid", [0, 1])
def test_a_view_with_an_offset_opens_over_the_shifted_basis(world, mj, pyref, cid):
    """points 3 .. of the registration: S_k = beta^(3 + k) G, so every proof is beta^3 times the plain one"""
    w = world[cid]
    pc, pp = w["pc"], w["pp"]
    case = w["cases"][("len", 9)]
    view = mj.UnivariateProverParam(w["c"], pp.handle, 8, offset=3, owner=False)
    proofs, evals = mj.UnivariateKzgPCS.multi_open_rou(view, case["mont"], case["k"], case["dom"])
    want = _want(pyref, pc, w["beta"], case["poly"], case["dom"].log_size_of_group, range(case["k"]), shift=3)
    assert evals == case["got"][1]
    assert [_pt(pc, p) for p in proofs] == [pt for pt, _ in want]
    assert mj.UnivariateKzgPCS.multi_open_rou(pp, case["mont"], case["k"], case["dom"]) == case["got"]      # ... and back at offset 0


@pytest.mark.parametrize("cid", [0, 1])
def test_the_entry_point_refuses_on_the_host(world, mj, cid):
    import torch
    w = world[cid]
    pc, pp = w["pc"], w["pp"]
    L = mj.load()
    case = w["cases"][("len", 17)]
    t = torch.from_numpy(case["mont"].view(np.int64)).cuda()
    out_p, out_e = np.zeros((32, 2 * pc.fq_limbs), np.uint64), np.zeros((32, 4), np.uint64)
    ptr = lambda a: C.c_void_p(a.ctypes.data)
    call = lambda off, n, log_n, k, p, e: L.mzk_kzg_multi_open_rou_dev(pp.handle, off, t.data_ptr(), n, log_n, k, p, e, None)
    before = _launches(L)
    assert call(pp.length - 15, 17, 5, 32, ptr(out_p), ptr(out_e)) == ERR_INVALID_ARG and b"fewer than d = 16" in L.mzk_last_error()
    assert call(0, 17, 3, 8, ptr(out_p), None) == ERR_INVALID_ARG and b"smaller domain" in L.mzk_last_error()          # d = 16 > N = 8
    assert call(0, 17, 4, 16, None, ptr(out_e)) == ERR_INVALID_ARG and b"smaller domain" in L.mzk_last_error()         # len = 17 > N = 16
    assert call(0, 17, 22, 32, ptr(out_p), ptr(out_e)) == ERR_UNSUPPORTED and b"log_domain" in L.mzk_last_error()
    assert call(0, 17, pc.two_adicity + 1, 32, None, ptr(out_e)) == ERR_UNSUPPORTED
    assert _launches(L) == before
    assert call(0, 17, 4, 16, ptr(out_p), None) == 0                       # d = 16 = N: proofs alone fit where the evaluations do not
    assert [_pt(pc, mj.Commitment(w["c"], out_p[i])) for i in range(0, 16)] == [_pt(pc, p) for p in case["got"][0][0:32:2]]
    assert call(0, (1 << 21) + 1, 21, 4, ptr(out_p), None) == ERR_UNSUPPORTED and b"2d above" in L.mzk_last_error()   # 2d = 2^22 (d_poly is not read)


@pytest.mark.parametrize("cid", [0, 1])
def test_the_entry_point_with_one_output_and_the_one_point_domain(world, mj, cid):
    """straight at the C ABI: evaluations alone (proofs NULL), and log_domain = 0 -- N = 1, the size-1 scalar NTT and a group NTT of no stage"""
    import torch
    w = world[cid]
    c, pc, pp = w["c"], w["pc"], w["pp"]
    L = mj.load()
    ptr = lambda a: C.c_void_p(a.ctypes.data)

    def call(name, n, log_n, k, want_proofs, want_evals):
        t = torch.from_numpy(w["cases"][name]["mont"].view(np.int64)).cuda()
        out_p, out_e = np.full((max(k, 1), 2 * pc.fq_limbs), 7, np.uint64), np.full((max(k, 1), 4), 7, np.uint64)
        assert L.mzk_kzg_multi_open_rou_dev(pp.handle, 0, t.data_ptr(), n, log_n, k, ptr(out_p) if want_proofs else None,
                                            ptr(out_e) if want_evals else None, None) == 0, L.mzk_last_error()
        k = min(k, 1 << log_n)                                             # what the call returns; the rows behind keep their filler
        assert (out_p[k:] == 7).all() and (out_e[k:] == 7).all()
        return [_pt(pc, mj.Commitment(c, out_p[i])) for i in range(k)], mj.params.fr_from_mont(c, out_e[:k])
    case = w["cases"][("len", 17)]
    _, evals = call(("len", 17), 17, 5, 32, False, True)
    assert evals == case["got"][1]
    line = w["cases"][("len", 2)]                                          # f_0 + f_1 X: every proof is [f_1]G, at N = 1 too
    proofs, _ = call(("len", 2), 2, 0, 1, True, False)
    assert proofs == [_pt(pc, line["got"][0][0])] and proofs[0] is not None
    const = w["cases"][("len", 1)]
    proofs, evals = call(("len", 1), 1, 0, 5, True, True)                  # (5 points asked of a domain of one)
    assert proofs == [None] and evals == [const["poly"][0]]
    _, evals = call(("len", 2), 1, 0, 1, False, True)                      # the first coefficient alone, as a polynomial of len 1
    assert evals == [line["poly"][0]]
