"""GPU: the Plookup builders (csrc/plookup.cuh through mzk_plookup_sorted_vec_dev / mzk_plookup_product_dev) and the lookup family of
mzk_prover_check_witness (csrc/check.cuh) on the scenario catalogue of tests/plookup_cases.py, value for value against the big-int
restatement (oracle/pyref_plonk.py: a dict and a loop) and the integer definition of tests/check_witness_ref.py.

What the catalogue reaches that the circuits of the other tests do not: many non-zero counters (the per-lane atomicAdd path), n - 1
lookups on one entry at either side of a scan-block boundary, values that recur without being adjacent (the atomicMin of the insert
kernel under contention), runs across workgroup and scan-block boundaries, values one word apart, 64 values on one probe chain and
a chain that wraps at the end of the slot array, waves in which one lane disagrees, refused witnesses followed by a valid one on
the same key, and a small problem after a large one in the shared workspace.  Sizes: 2^9 (two workgroups, one scan block) and 2^13
(two scan blocks, four blocks of the product's scan) for the whole catalogue; 2, 4, 2^12 (exactly one scan block) and 2^14 for the
reduced one.  Every comparison is equality of field elements, counts and row numbers."""
import numpy as np
import pytest

import check_witness_ref as REF
import plookup_cases as PC
from conftest import fr_mont_limbs

pytestmark = pytest.mark.gpu

K = [1, 7, 13, 17, 23, 29]
SWEEP = [(curve_id, log_n, s, v, mode) for log_n in (9, 13) for s, v in PC.CATALOGUE for mode in PC.MODES for curve_id in (0, 1)]
EDGES = [(curve_id, log_n, s, v, mode) for log_n in (1, 2, 12, 14) for s, v in PC.REDUCED for mode in PC.MODES for curve_id in (0, 1)]
CHECKS = [(curve_id, log_n, s, v) for log_n in (8, 13) for s, v in PC.CATALOGUE for curve_id in (0, 1)]
ident = lambda e: "%s-2^%d-%s%s" % (("bls12_381", "bn254")[e[0]], e[1], PC.label(e[2], e[3]), "-" + e[4] if len(e) > 4 else "")


def _limbs(cref, curve_id, vals):
    """canonical integers -> (len, 4) uint64 Montgomery limbs, converted by the C oracle (6 n values per witness)"""
    raw = np.frombuffer(b"".join(v.to_bytes(32, "little") for v in vals), dtype=np.uint64).reshape(-1, 4)
    return cref.fr_convert(curve_id, raw, True)


def _ints(cref, curve_id, a):
    a = a.cpu().numpy() if hasattr(a, "cpu") else a
    raw = cref.fr_convert(curve_id, np.ascontiguousarray(a).view(np.uint64).reshape(-1, 4), False).tobytes()
    return [int.from_bytes(raw[i:i + 32], "little") for i in range(0, len(raw), 32)]


def _wires(cref, curve_id, w):
    n = len(w[0])
    return _limbs(cref, curve_id, [x for col in w for x in col]).reshape(6, n, 4)


def _key_polys(mj, cref, curve_id, k):
    """the coefficient forms a key of this instance is registered from: the four tables and q_lookup, inverse NTT on the CPU; every
    other selector and the sigmas are the zero polynomial (the builders and the lookup check read none of them)"""
    poly = lambda vals: cref.ntt(curve_id, _limbs(cref, curve_id, vals), k.log_n, True)
    zero = np.zeros((1, 4), dtype=np.uint64)
    tabs = {name: poly(k.tables[key]) for name, key in zip(mj.plonk.PLOOKUP_TABLE_POLYS, PC.TABLES)}
    return [zero] * 13 + [poly(k.q_lookup)], [zero] * 6, tabs


def _register(mj, cref, curve_id, k):
    sel, sig, tabs = _key_polys(mj, cref, curve_id, k)
    return mj.plonk.ProvingKeyDevice.register(mj.params.CURVES[curve_id], k.n, sel, sig, K, plookup=tabs)


def _builders_match(mj, cref, pyref, curve_id, k, pk, w):
    """both ABI calls on one witness of the instance against the restatement: merged table, merged lookup witness, all 2n - 1 sorted
    entries, and the n values of the Plookup product polynomial on the domain"""
    import pyref_plonk as PP
    pc, n = pyref.CURVES[curve_id], k.n
    want_table = PP.merged_table_values(pc, k.tau, k.tables, k.q_lookup, w)
    want_lookup = PP.merged_lookup_values(pc, k.tau, k.tables, k.q_lookup, w)
    want_sorted = PP.sorted_lookup_vec(want_table, want_lookup[:n - 1])
    assert len(want_sorted) == 2 * n - 1
    table, lookup, sorted_vec = mj.plonk.compute_lookup_sorted_vec(pk, k.tau, _wires(cref, curve_id, w))
    assert _ints(cref, curve_id, table) == want_table, "merged table"
    assert _ints(cref, curve_id, lookup) == want_lookup, "merged lookup witness"
    got = _ints(cref, curve_id, sorted_vec)
    assert got == want_sorted, ("sorted vector: first difference at", next(i for i in range(2 * n - 1) if got[i] != want_sorted[i]))
    prod = mj.plonk.compute_lookup_prod_polynomial(pk, k.beta, k.gamma, table, lookup, sorted_vec)
    values = cref.ntt(curve_id, np.ascontiguousarray(prod.cpu().numpy().view(np.uint64)), k.log_n, False)
    assert _ints(cref, curve_id, values) == PP.lookup_product_values(pc, n, k.tau, k.beta, k.gamma, want_table, want_lookup, want_sorted), "Plookup product"


def _sweep_one(gpu, mj, cref, pyref, curve_id, log_n, scenario, variant, mode):
    k = PC.case(pyref.CURVES[curve_id], log_n, scenario, variant, mode)
    pk = _register(mj, cref, curve_id, k)
    try:
        if k.refused:
            with pytest.raises(mj.plonk.PlonkError, match="outside the table"):
                mj.plonk.compute_lookup_sorted_vec(pk, k.tau, _wires(cref, curve_id, k.w))
            # the valid witness next, on the same key: a stale `missing` word or stale slots would show here
            _builders_match(mj, cref, pyref, curve_id, k, pk, k.w_valid)
        else:
            _builders_match(mj, cref, pyref, curve_id, k, pk, k.w)
    finally:
        pk.release()


def test_limb_conversion_is_the_suites(gpu, mj, cref, pyref):
    """the C oracle's Montgomery conversion, used here for speed, against the big-int one of conftest"""
    for curve_id in (0, 1):
        c = mj.params.CURVES[curve_id]
        vals = [0, 1, c.r - 1, c.r // 3, 1 << 200]
        assert np.array_equal(_limbs(cref, curve_id, vals), fr_mont_limbs(c, vals))
        assert _ints(cref, curve_id, fr_mont_limbs(c, vals)) == vals


@pytest.mark.parametrize("curve_id,log_n,scenario,variant,mode", SWEEP, ids=[ident(e) for e in SWEEP])
def test_builders_on_the_catalogue(gpu, mj, cref, pyref, curve_id, log_n, scenario, variant, mode):
    _sweep_one(gpu, mj, cref, pyref, curve_id, log_n, scenario, variant, mode)


@pytest.mark.parametrize("curve_id,log_n,scenario,variant,mode", EDGES, ids=[ident(e) for e in EDGES])
def test_builders_at_the_edge_sizes(gpu, mj, cref, pyref, curve_id, log_n, scenario, variant, mode):
    """n = 2: one lookup, the product is all ones; n = 4; n = 2^12: exactly one scan block; n = 2^14: four"""
    _sweep_one(gpu, mj, cref, pyref, curve_id, log_n, scenario, variant, mode)


@pytest.mark.parametrize("curve_id,mode", [(0, "direct"), (1, "tuple")])
def test_small_problem_after_a_large_one(gpu, mj, cref, pyref, curve_id, mode):
    """distinct_uniform at 2^14, then interleaved_duplicates at 2^6 on a fresh key: the shared workspace still holds the large
    problem's slots, counters and positions"""
    _sweep_one(gpu, mj, cref, pyref, curve_id, 14, "distinct_uniform", None, mode)
    k = PC.case(pyref.CURVES[curve_id], 6, "interleaved_duplicates", "m7", mode)
    pk = _register(mj, cref, curve_id, k)
    try:
        _builders_match(mj, cref, pyref, curve_id, k, pk, k.w)
    finally:
        pk.release()


# ---- the witness check's lookup family on the same instances (tuple mode) ---------------------------------------------------------
@pytest.fixture(scope="module")
def commit_keys(gpu, mj):
    """one commit key per (curve, domain): the prover handles below share it"""
    made = {}

    def get(curve_id, n):
        if (curve_id, n) not in made:
            made[curve_id, n] = mj.UnivariateProverParam.gen_srs_for_testing(mj.params.CURVES[curve_id], 0x5EED + n, n + 2)
        return made[curve_id, n]
    yield get
    for ck in made.values():
        ck.release()


@pytest.mark.parametrize("curve_id,log_n,scenario,variant", CHECKS, ids=[ident(e) for e in CHECKS])
def test_check_witness_lookup_family(gpu, mj, cref, pyref, commit_keys, curve_id, log_n, scenario, variant):
    """A prover handle whose gates are all padding rows, so that the lookup family alone decides.  Accepted scenarios: "satisfied".
    `missing`: kind "lookup", the exact number of failing rows and the lowest of them -- in the first workgroup (row_0), in the last
    (row_n_minus_2), on both sides of a wave boundary (wave_boundary), scattered (one_third), and one word of one component away
    from a table tuple, each component in turn (one_word); then the valid witness of the same key is satisfied."""
    pc = pyref.CURVES[curve_id]
    k = PC.case(pc, log_n, scenario, variant, "tuple")
    sel, sig, tabs = _key_polys(mj, cref, curve_id, k)
    prover = mj.prover.TurboPlonkProver(mj.params.CURVES[curve_id], k.n, sel, sig, K, commit_keys(curve_id, k.n), plookup=tabs)
    try:
        want = REF.lookup_failures(pc, k.sel, k.w, k.tables)
        rep = prover.check_witness(_wires(cref, curve_id, k.w), [])
        assert rep.gate_failures == 0 and rep.gate_row is None and not rep.copy_checked
        assert (rep.lookup_failures, rep.lookup_row) == (len(want), want[0] if want else None)
        if k.refused:
            assert want and rep.kind == "lookup" and not rep.satisfied
            assert rep.row_wires == [k.w[j][want[0]] for j in range(6)]
            rep = prover.check_witness(_wires(cref, curve_id, k.w_valid), [])
            assert REF.lookup_failures(pc, k.sel, k.w_valid, k.tables) == []
        assert rep.kind == "satisfied" and rep.satisfied and rep.lookup_failures == 0 and rep.lookup_row is None and rep.row_wires == []
    finally:
        prover.release()
