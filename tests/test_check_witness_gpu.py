"""GPU: mzk_prover_check_witness (include/mzk.h; csrc/check.cuh) -- the report for satisfied and corrupted witnesses of general circuits
must hold exactly what the integer restatement of its definitions (tests/check_witness_ref.py) finds: the first failing family, the
number of failing gate rows / lookup rows / copy cells, the lowest of each, the wire values of the reported row and the gate residual.
Sizes: 2^3 (one partial wave), 2^4 (the smallest UltraPlonk domain with a lookup block), 2^6 (one wave), 2^8 / 2^9 (one and two
workgroups of 256), 2^12 (16 workgroups: counts and minima across waves and workgroups)."""
import ctypes as C
import random
import types
from functools import lru_cache

import numpy as np
import pytest

import check_witness_ref as REF
from conftest import build_circuit, build_ultra_circuit, fr_mont_limbs, fr_from_mont_limbs

pytestmark = pytest.mark.gpu
TABLES = ("range", "key", "table_dom_sep", "q_dom_sep")
STATE, INVALID, BAD_HANDLE = -10, -1, -4


@lru_cache(maxsize=None)
def _circuit(curve_id, ultra, log_n, gates, range_bits):
    """the circuit's integers, built once per case and never modified (tests copy the wires they corrupt)"""
    import pyref
    pc = pyref.CURVES[curve_id]
    rng = random.Random(5200 + curve_id + 2 * ultra + 7 * log_n + (gates == "all"))
    if ultra:
        sel, sig, k, w, pi, tabs = build_ultra_circuit(pc, log_n, rng, range_bits=range_bits, gates=gates)
    else:
        sel, sig, k, w, pi = build_circuit(pc, log_n, rng, gates=gates)
        tabs = None
    return sel, sig, k, w, pi, tabs


def _instance(mj, curve_id, ultra, log_n, gates="hot", range_bits=3):
    import pyref
    c, pc = mj.params.CURVES[curve_id], pyref.CURVES[curve_id]
    sel, sig, k, w, pi, tabs = _circuit(curve_id, ultra, log_n, gates, range_bits)
    n = 1 << log_n
    dom = mj.Radix2EvaluationDomain(c, log_n)
    kw = {"plookup": {name: dom.ifft(fr_mont_limbs(c, tabs[key])) for name, key in zip(mj.plonk.PLOOKUP_TABLE_POLYS, TABLES)}} if ultra else {}
    ck = mj.UnivariateProverParam.gen_srs_for_testing(c, 0x5EED + log_n, n + 2)
    mk = lambda: mj.prover.TurboPlonkProver(c, n, [dom.ifft(fr_mont_limbs(c, s)) for s in sel], [dom.ifft(fr_mont_limbs(c, s)) for s in sig], k, ck, **kw)
    inst = types.SimpleNamespace(c=c, pc=pc, n=n, W=6 if ultra else 5, ultra=ultra, sel=sel, sig=sig, k=k, w=w, pi=pi, tabs=tabs, ck=ck, native=mk(), make=mk,
                                 pub=pi[:4], blind=mj.snark.draw_blinders(c, mj.rng.test_rng(), 6 if ultra else 5, ultra))

    def release():
        inst.native.release()
        ck.release()
    inst.release = release
    return inst


def _limbs(inst, w):
    return np.stack([fr_mont_limbs(inst.c, col) for col in w])


def _prove(mj, inst, wires, pub=None, **kw):
    pub = inst.pub if pub is None else pub
    return mj.snark.serialize_proof(inst.c, inst.native.prove(wires, pub, mj.prover.TranscriptChallenges(inst.native, inst.pub), inst.blind, **kw))


def _check(inst, rep, w, pi=None, wire_vars=None, native=None):
    """the whole report against the integer restatement; returns what was expected"""
    n, W = inst.n, inst.W
    exp = REF.expected_report(inst.pc, inst.sel, w, inst.pi if pi is None else pi, inst.tabs, wire_vars)
    print("expected", {k: (v if k == "kind" or v is None else (len(v), v[:1])) for k, v in exp.items()}, "got", rep)
    assert rep.kind == exp["kind"] and rep.satisfied == (exp["kind"] == "satisfied")
    assert rep.gate_failures == len(exp["gate"]) and rep.gate_row == (exp["gate"][0][0] if exp["gate"] else None)
    assert rep.lookup_failures == len(exp["lookup"]) and rep.lookup_row == (exp["lookup"][0] if exp["lookup"] else None)
    if wire_vars is None:
        assert not rep.copy_checked and rep.copy_failures == 0 and rep.copy_cell is None and rep.copy_rep_cell is None
    else:
        cell = lambda v: (v // n, v % n)
        assert rep.copy_checked and rep.copy_failures == len(exp["copy"])
        assert (rep.copy_cell, rep.copy_rep_cell) == ((cell(exp["copy"][0][0]), cell(exp["copy"][0][1])) if exp["copy"] else (None, None))
    assert rep.gate_residual == (exp["gate"][0][1] if exp["gate"] else None)
    row = {"gate": rep.gate_row, "lookup": rep.lookup_row, "copy": rep.copy_cell[1] if rep.copy_cell else None, "satisfied": None}[rep.kind]
    assert rep.row_wires == ([w[j][row] for j in range(W)] if row is not None else [])
    return exp


SATISFIED = [(0, False, 3, "hot", 3), (1, False, 6, "hot", 3), (0, False, 9, "hot", 3), (1, False, 12, "all", 3),
             (1, True, 4, "hot", 2), (0, True, 6, "hot", 3), (1, True, 8, "hot", 3), (0, True, 12, "all", 3)]


@pytest.mark.parametrize("curve_id,ultra,log_n,gates,range_bits", SATISFIED)
def test_satisfied_witness_and_the_proof_after_the_check(gpu, mj, curve_id, ultra, log_n, gates, range_bits):
    inst = _instance(mj, curve_id, ultra, log_n, gates, range_bits)
    wires = _limbs(inst, inst.w)
    before = _prove(mj, inst, wires)
    rep = inst.native.check_witness(wires, inst.pub)
    exp = _check(inst, rep, inst.w)
    assert exp["kind"] == "satisfied" and rep.gate_failures == rep.lookup_failures == rep.copy_failures == 0
    assert rep.gate_row is None and rep.lookup_row is None and rep.copy_cell is None and rep.copy_rep_cell is None
    assert _prove(mj, inst, wires) == before
    inst.release()


@pytest.mark.parametrize("curve_id,ultra,log_n", [(0, False, 6), (1, True, 6)])
def test_one_cell_per_gate_family(gpu, mj, curve_id, ultra, log_n):
    """rows picked as test_native_prover_gpu picks them: wire 2 of a linear combination, wire 1 of a power-5 row, a wire of an ecc row,
    the output of a row with every term"""
    inst = _instance(mj, curve_id, ultra, log_n, "all")
    sel, n, r = inst.sel, inst.n, inst.c.r
    rng = random.Random(17 + curve_id)
    row = lambda cond: next(i for i in range(n) if cond(lambda j: sel[j][i] != 0))
    lc = row(lambda nz: nz(2) and not nz(12))
    pow5 = row(lambda nz: nz(7) and not nz(12))
    ecc = row(lambda nz: nz(12) and not nz(10))
    mixed = row(lambda nz: nz(12) and nz(10) and nz(2) and nz(7))
    assert len({lc, pow5, ecc, mixed}) == 4
    for wire, at in ((2, lc), (1, pow5), (3, ecc), (4, mixed)):
        bad = [col[:] for col in inst.w]
        bad[wire][at] = rng.randrange(r)
        wires = _limbs(inst, bad)
        rep = inst.native.check_witness(wires, inst.pub)
        exp = _check(inst, rep, bad)
        assert rep.kind == "gate" and rep.gate_row == at and rep.gate_failures == len(exp["gate"]) and rep.gate_residual == REF.gate_residual(inst.pc, sel, bad, inst.pi, at)
        with pytest.raises(mj.plonk.PlonkError) as e:
            _prove(mj, inst, wires)
        assert e.value.kind == "WrongQuotientPolyDegree", (wire, at)
    inst.release()


def test_counts_and_lowest_row_across_waves_and_workgroups(gpu, mj):
    """2^12 rows = 64 waves in 16 workgroups.  A gated row fails through its output wire; a row without a gate (row % 4 == 3) can only
    fail through a public input it does not hold, so those rows are given one."""
    inst = _instance(mj, 0, False, 12, "hot")
    n, r = inst.n, inst.c.r
    for rows in ([0, 63, 64, 255, 256, n - 1], [n - 1], [64]):
        bad = [col[:] for col in inst.w]
        pi = inst.pi[:]
        for i in rows:
            if inst.sel[10][i]:
                bad[4][i] = (bad[4][i] + 1 + i) % r
            else:
                assert not any(col[i] for col in inst.sel)
                pi[i] = 1 + i
        pub_rows = [i for i in range(n) if pi[i]]
        rep = inst.native.check_witness(_limbs(inst, bad), (pub_rows, [pi[i] for i in pub_rows]))
        _check(inst, rep, bad, pi=pi)
        assert rep.kind == "gate" and rep.gate_failures == len(rows) and rep.gate_row == min(rows)
    inst.release()


@pytest.mark.parametrize("curve_id,ultra,log_n", [(1, False, 6), (0, True, 6)])
def test_public_input_failures_sit_on_the_public_input_row(gpu, mj, curve_id, ultra, log_n):
    inst = _instance(mj, curve_id, ultra, log_n)
    wires, r = _limbs(inst, inst.w), inst.c.r
    for pub in (inst.pub[:3] + [(inst.pub[3] + 1) % r], []):
        pi = (pub + [0] * inst.n)[:inst.n]
        rep = inst.native.check_witness(wires, pub)
        _check(inst, rep, inst.w, pi=pi)
        assert rep.kind == "gate" and rep.gate_row == 3 and rep.gate_failures == 1 and rep.gate_residual == (5 + pi[3]) % r
    # the same values as (rows, values) and as the n-vector: satisfied
    for pub in (([3], [inst.pub[3]]), fr_mont_limbs(inst.c, inst.pi)):
        assert inst.native.check_witness(wires, pub).satisfied
    inst.release()


@pytest.mark.parametrize("curve_id,log_n", [(1, 6), (0, 8)])
def test_lookup_failures(gpu, mj, curve_id, log_n):
    inst = _instance(mj, curve_id, True, log_n)
    n, r, R, w = inst.n, inst.c.r, 8, inst.w
    copy = lambda: [col[:] for col in w]
    run = lambda bad: _check(inst, inst.native.check_witness(_limbs(inst, bad), inst.pub), bad)
    # a looked-up value of lookup row R + 1
    bad = copy()
    bad[1][R + 1] = (bad[1][R + 1] + 1) % r
    exp = run(bad)
    assert (exp["kind"], exp["lookup"]) == ("lookup", [R + 1])
    with pytest.raises(mj.plonk.PlonkError) as e:                      # round 1.5 refuses it without a row; check=True adds the report
        _prove(mj, inst, _limbs(inst, bad), check=True)
    assert e.value.report.kind == "lookup" and e.value.report.lookup_row == R + 1 and e.value.report.lookup_failures == 1
    # one past the range table on row 0
    bad = copy()
    bad[5][0] = R
    assert run(bad)["lookup"] == [0]
    # the last row is not looked up
    bad = copy()
    bad[5][n - 1] = r - 1
    assert run(bad)["kind"] == "satisfied"
    # a changed table value: every row that looks that entry up fails
    tgt = R + w[0][R]                                                  # the entry lookup row R refers to (key = row - R)
    bad = copy()
    bad[3][tgt] = (bad[3][tgt] + 1) % r
    exp = run(bad)
    assert exp["kind"] == "lookup" and R in exp["lookup"] and exp["lookup"] == [i for i in range(R, R + n // 4) if w[0][i] == tgt - R]
    # gate and lookup failures together: the gate family is named, both are reported
    bad[4][0] = (bad[4][0] + 1) % r
    exp = run(bad)
    assert exp["kind"] == "gate" and exp["gate"][0][0] == 0 and exp["lookup"]
    inst.release()


@pytest.mark.parametrize("curve_id,ultra,log_n", [(0, False, 6), (1, True, 6)])
def test_copy_failures_from_device_wires(gpu, mj, curve_id, ultra, log_n):
    import torch
    inst = _instance(mj, curve_id, ultra, log_n)
    n, r = inst.n, inst.c.r
    wv, n_vars = REF.wire_variables_from_sigma(inst.pc, inst.sig, inst.k, log_n)
    inst.native.set_wire_variables(np.array(wv, dtype=np.uint32), n_vars)
    dev = lambda w: torch.from_numpy(_limbs(inst, w).view(np.int64)).cuda()
    rep = inst.native.check_witness(dev(inst.w), inst.pub)
    _check(inst, rep, inst.w, wire_vars=wv)
    assert rep.satisfied and rep.copy_checked
    by = {}
    for i, col in enumerate(wv):
        for j, v in enumerate(col):
            by.setdefault(v, []).append(i * n + j)
    # a 3-cycle none of whose cells feeds a gate (wire 5 cycles of the Ultra circuit are value classes, not 3-cycles)
    gate_free = lambda cell: REF.gate_failures(inst.pc, inst.sel, [[(x + 1) % r if (i * n + j) == cell else x for j, x in enumerate(col)]
                                                                    for i, col in enumerate(inst.w)], inst.pi) == []
    cyc = next(cells for cells in by.values() if len(cells) == 3 and cells[-1] < 5 * n and all(gate_free(x) for x in cells))
    other = inst.make()                                                # the same key without a wire-variable table
    for pos, fails in ((2, 1), (0, 2)):
        bad = [col[:] for col in inst.w]
        bad[cyc[pos] // n][cyc[pos] % n] = (bad[cyc[pos] // n][cyc[pos] % n] + 1) % r
        rep = inst.native.check_witness(dev(bad), inst.pub)
        _check(inst, rep, bad, wire_vars=wv)
        assert rep.kind == "copy" and rep.copy_failures == fails
        assert rep.copy_cell == ((cyc[2] // n, cyc[2] % n) if pos == 2 else (cyc[1] // n, cyc[1] % n)) and rep.copy_rep_cell == (cyc[0] // n, cyc[0] % n)
        rep = other.check_witness(dev(bad), inst.pub)
        _check(inst, rep, bad, wire_vars=None)
        assert not rep.copy_checked and rep.kind == "satisfied"
    other.release()
    inst.release()


@pytest.mark.parametrize("curve_id,plonk_type", [(0, "TurboPlonk"), (1, "UltraPlonk")])
def test_every_witness_kind_on_the_bench_circuit(gpu, mj, pyref, curve_id, plonk_type):
    """host vector, device vector (gathered through the resident wire variables) and host wires; one changed variable makes exactly the
    rows that read it fail, and the copy constraints hold by construction"""
    import torch
    c, pc = mj.params.CURVES[curve_id], pyref.CURVES[curve_id]
    cs = mj.snark.gen_circuit_for_bench(c, 40, plonk_type)
    ints = lambda t: fr_from_mont_limbs(pc, t.cpu().numpy().view(np.uint64).reshape(-1, 4))
    n, W = cs.n, cs.num_wire_types
    grid = lambda flat, rows: [flat[i * n:(i + 1) * n] for i in range(rows)]
    sel = grid(ints(cs.selector_values), cs.selector_values.shape[0])
    tabs = dict(zip(TABLES, grid(ints(cs.table_values), 4))) if cs.table_values is not None else None
    var = cs.wire_variables.cpu().numpy().astype(np.uint32)
    wit = ints(cs.witness)
    ck = mj.UnivariateProverParam.gen_srs_for_testing(c, 99, n + 2)
    pk = mj.snark.preprocess(ck, cs)
    pk.set_wire_variables(var, len(wit))                               # the host-wires leg is checked against it too, whatever ran before
    inst = types.SimpleNamespace(c=c, pc=pc, n=n, W=W, sel=sel, tabs=tabs, pi=[0] * n)
    bad_wit = cs.witness.clone()
    bad_wit[7] = bad_wit[9]
    bad_ints = wit[:]
    bad_ints[7] = wit[9]
    for name, witness, vals in (("good", cs.witness, wit), ("bad", bad_wit, bad_ints)):
        w = [[vals[v] for v in row] for row in var]
        wires_host = witness.cpu()[torch.from_numpy(var.reshape(-1).astype(np.int64))].reshape(W, n, 4).contiguous()
        kinds = {"host vector": mj.snark.HostWitness(witness.cpu(), cs.wire_variables), "device vector": mj.snark.HostWitness(witness, cs.wire_variables),
                 "host wires": wires_host}
        for kind, arg in kinds.items():
            rep = pk.check_witness(arg, [])
            exp = _check(inst, rep, w, wire_vars=[list(row) for row in var])
            assert rep.copy_checked and rep.copy_failures == 0, kind
            assert (exp["kind"], len(exp["gate"])) == (("satisfied", 0) if name == "good" else ("gate", 2)), kind
    pk.release()
    ck.release()


def test_state_memory_and_arguments(gpu, mj):
    import torch
    L = gpu.load()
    lib = gpu
    inst = _instance(mj, 0, False, 6)
    native, n = inst.native, inst.n
    wires = _limbs(inst, inst.w)
    p = lambda a: C.c_void_p(a.ctypes.data)
    # the check allocates nothing on the handle, before or after a proof
    hb = native.hbm_bytes()
    assert native.check_witness(wires, inst.pub).satisfied and native.hbm_bytes() == hb
    want = _prove(mj, inst, wires)
    hb = native.hbm_bytes()
    assert native.check_witness(torch.from_numpy(wires.view(np.int64)).cuda(), inst.pub).satisfied and native.hbm_bytes() == hb
    # a check abandons the proof in flight: the next round must be round 1
    native.round1(wires, inst.pub, inst.blind.wires)
    assert native.check_witness(wires, inst.pub).satisfied
    one = mj.params.fr_to_mont(inst.c, [1, 2, 3])
    out = np.zeros((8, 2, 6), dtype=np.uint64)
    assert L.mzk_prover_round2(native.handle, p(one), p(one), p(one), p(out)) == STATE
    assert _prove(mj, inst, wires) == want
    # arguments
    rep = lib.WitnessReport()
    pub = mj.params.fr_to_mont(inst.c, inst.pub)
    call = lambda h, kind, ln, rows, n_pub, out_rep: L.mzk_prover_check_witness(h, kind, p(wires), ln, rows, p(pub), n_pub, out_rep)
    assert call(native.handle, 1, 5 * n, None, 4, C.byref(rep)) == 0 and rep.kind == 0 and rep.gate_row == 2 ** 64 - 1
    assert call(native.handle, 1, 5 * n, None, 4, None) == INVALID                                  # null report
    assert call(native.handle, 1, 5 * n - 1, None, 4, C.byref(rep)) == INVALID                      # wrong length
    assert call(native.handle, 7, 5 * n, None, 4, C.byref(rep)) == INVALID                          # unknown kind
    assert call(native.handle, 2, 5 * n, None, 4, C.byref(rep)) == INVALID                          # a vector kind without wire variables
    rows = np.array([0, 1, 2, n], dtype=np.uint64)
    assert call(native.handle, 1, 5 * n, p(rows), 4, C.byref(rep)) == INVALID                       # public-input row outside the domain
    assert call(native.handle + 99, 1, 5 * n, None, 4, C.byref(rep)) == BAD_HANDLE
    # prove(check=True): the refused proof carries the report
    bad = [col[:] for col in inst.w]
    bad[4][0] = (bad[4][0] + 1) % inst.c.r
    with pytest.raises(mj.plonk.PlonkError) as e:
        _prove(mj, inst, _limbs(inst, bad), check=True)
    assert e.value.kind == "WrongQuotientPolyDegree" and e.value.report.kind == "gate" and e.value.report.gate_row == 0
    with pytest.raises(mj.plonk.PlonkError) as e:                      # the default is unchanged: no report
        _prove(mj, inst, _limbs(inst, bad))
    assert not hasattr(e.value, "report")
    assert _prove(mj, inst, wires) == want
    inst.release()
