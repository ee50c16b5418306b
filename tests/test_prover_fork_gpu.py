"""GPU: mzk_prover_fork -- several prover handles (slots) on ONE resident proving key.  A fork must prove exactly what its parent proves
(same bytes from the same rng), keep no state in common with it (interleaved rounds, concurrent threads), serve as another instance
of an aggregated proof, share the variable table until it replaces its own, cost a workspace and not a key in HBM, and account for what
it shares.  Shapes: n = 32 wherever the property does not depend on the size (general circuits with public inputs, copy constraints
and lookups; bench circuits for snark.batch_prove), n = 2^10 for the threads, n = 2^16 where HBM must dominate allocation granularity."""
import ctypes as C
import json
import os
import random
import subprocess
import threading
from functools import lru_cache

import numpy as np
import pytest

import check_witness_ref as REF
import pyref_fs as FS
from conftest import build_circuit, build_ultra_circuit, fr_mont_limbs, verifying_key

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "mpc-jellyfish_amd", "mzk_prove")
TABLES = ("range", "key", "table_dom_sep", "q_dom_sep")
LOG_N = 5
CASES = [(0, False), (1, True)]                 # TurboPlonk / BLS12-381 and UltraPlonk / BN254
SRS_BETA = 0xF02C
ERR_INVALID_ARG, ERR_BAD_HANDLE, ERR_UNSUPPORTED, ERR_STATE = -1, -4, -5, -10


@lru_cache(maxsize=None)
def _circuit(curve_id, ultra):
    """a general circuit at n = 32 (computed once, never modified): selector / sigma / wire / public-input values as integers, the
    Plookup tables, and the variable table its sigma encodes"""
    import pyref
    pc = pyref.CURVES[curve_id]
    rng = random.Random(5100 + curve_id + 2 * ultra)
    if ultra:
        sel, sig, k, w, pi, tabs = build_ultra_circuit(pc, LOG_N, rng)
    else:
        sel, sig, k, w, pi = build_circuit(pc, LOG_N, rng)
        tabs = None
    assert pi[3] != 0 and not any(pi[4:])
    var, n_vars = REF.wire_variables_from_sigma(pc, sig, k, LOG_N)
    return sel, sig, k, w, pi, tabs, var, n_vars


def _limbs(c, rows):
    return np.stack([fr_mont_limbs(c, row) for row in rows])


def _prover(mj, curve_id, ultra, ck, lagrange_ck=None, comm=None):
    """the prover of _circuit from coefficient forms (no variable table)"""
    c = mj.params.CURVES[curve_id]
    sel, sig, k, w, pi, tabs, _, _ = _circuit(curve_id, ultra)
    dom = mj.Radix2EvaluationDomain(c, LOG_N)
    kw = {"plookup": {name: dom.ifft(fr_mont_limbs(c, tabs[key])) for name, key in zip(mj.plonk.PLOOKUP_TABLE_POLYS, TABLES)}} if ultra else {}
    return mj.prover.TurboPlonkProver(c, 1 << LOG_N, [dom.ifft(fr_mont_limbs(c, s)) for s in sel], [dom.ifft(fr_mont_limbs(c, s)) for s in sig], k, ck,
                                      lagrange_ck=lagrange_ck, comm=comm, **kw)


def _prover_from_structure(mj, curve_id, ultra, ck):
    """... and from the circuit's structure: it holds the variable table"""
    c = mj.params.CURVES[curve_id]
    sel, sig, k, w, pi, tabs, var, n_vars = _circuit(curve_id, ultra)
    return mj.prover.TurboPlonkProver.from_circuit(c, 1 << LOG_N, _limbs(c, sel), np.array(var, dtype=np.uint32), n_vars, k, ck,
                                                   table_values=_limbs(c, [tabs[key] for key in TABLES]) if ultra else None)


def _srs(mj, curve_id, n=1 << LOG_N):
    return mj.UnivariateProverParam.gen_srs_for_testing(mj.params.CURVES[curve_id], SRS_BETA, n + 2)


def _blinders(mj, c, p, skip=0):
    """the draws of one proof from the reference's test rng, after `skip` other draws (another proof's blinders)"""
    rng = mj.rng.test_rng()
    for _ in range(skip):
        mj.rng.fr_rand(c, rng)
    return mj.snark.draw_blinders(c, rng, p.W, p.ultra)


def _steps(mj, p, wires, pub, blind, extra=None):
    """TurboPlonkProver.prove round by round: yields after rounds 1 (1.5), 2 (2.5), 3 and 4, returns the serialized proof after round 5"""
    P = mj.prover
    src = P.TranscriptChallenges(p, pub, extra)
    yield
    wires_comms = p.round1(wires, pub, blind.wires)
    tau = src.after_round1(wires_comms)
    h_comms = p.round1_5(tau, blind.h) if p.ultra else None
    yield
    beta, gamma = src.after_round1_5(h_comms)
    z_comm = p.round2(beta, gamma, blind.z)
    pl_comm = p.round2_5(blind.prod_lookup) if p.ultra else None
    yield
    split_comms = P.round3([p], src.after_round2(z_comm, pl_comm), blind.quot)
    yield
    we, wse, pne, pe = p.round4(src.after_round3(split_comms))
    yield
    oc = P.round5([p], src.after_round4(we, wse, pne, pe))
    return mj.snark.serialize_proof(p.curve, P.ProofCore(wires_comms, z_comm, split_comms, oc[0], oc[1], we, wse, pne, {}, h_comms, pl_comm, pe))


def _rng_after_srs(mj, c):
    rng = mj.rng.test_rng()
    mj.rng.fr_rand(c, rng)                                                 # (the SRS trapdoor is the first draw of the bench's stream)
    return rng


def _run(gen):
    try:
        while True:
            next(gen)
    except StopIteration as e:
        return e.value


def _prove(mj, p, wires, pub, skip=0, extra=None):
    return _run(_steps(mj, p, wires, pub, _blinders(mj, p.curve, p, skip), extra))


# ---- 1. same bytes -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("curve_id,ultra", CASES)
def test_a_fork_proves_the_parents_bytes(gpu, mj, pyref, curve_id, ultra):
    import pyref_verifier as V
    c, pc = mj.params.CURVES[curve_id], pyref.CURVES[curve_id]
    sel, sig, k, w, pi, tabs, _, _ = _circuit(curve_id, ultra)
    wires, pub = _limbs(c, w), pi[:4]
    ck = _srs(mj, curve_id)
    parent = _prover(mj, curve_id, ultra, ck)
    want = _prove(mj, parent, wires, pub)
    assert mj.snark.serialize_proof(c, parent.prove(wires, pub, mj.prover.TranscriptChallenges(parent, pub), _blinders(mj, c, parent))) == want
    vk = verifying_key(mj, pc, parent, len(pub))
    fork = parent.fork()
    assert fork.handle not in (0, parent.handle) and fork.ck is parent.ck and fork.k == parent.k
    assert _prove(mj, fork, wires, pub) == want
    assert _prove(mj, parent, wires, pub) == want
    parent.release()                                                       # the key outlives the handle that made it
    assert _prove(mj, fork, wires, pub) == want
    grandchild = fork.fork()
    fork.release()
    got = _prove(mj, grandchild, wires, pub)
    assert got == want
    assert V.verify(pc, FS.StandardTranscript(pc, b"PlonkProof"), vk, pub, got, pyref.g1_gen(pc), SRS_BETA)
    assert verifying_key(mj, pc, grandchild, len(pub)) == vk
    grandchild.release()
    ck.release()


# ---- 2. no state leaks between slots ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("curve_id,ultra", CASES)
def test_interleaved_rounds_of_two_slots_do_not_mix(gpu, mj, curve_id, ultra):
    """Parent and fork each carry a proof, with different blinders and transcript init messages, one round at a time in turn; each proof
    equals the one made alone.  (Both prove the circuit's one witness: the builders draw structure and witness together, so there is no
    second satisfying witness for the same structure to give the fork.)"""
    c = mj.params.CURVES[curve_id]
    sel, sig, k, w, pi, tabs, _, _ = _circuit(curve_id, ultra)
    wires, pub = _limbs(c, w), pi[:4]
    ck = _srs(mj, curve_id)
    parent = _prover(mj, curve_id, ultra, ck)
    fork = parent.fork()
    alone = [_prove(mj, parent, wires, pub, 0, b"first"), _prove(mj, parent, wires, pub, 40, b"second")]
    assert alone[0] != alone[1]
    gens = [_steps(mj, parent, wires, pub, _blinders(mj, c, parent, 0), b"first"), _steps(mj, fork, wires, pub, _blinders(mj, c, fork, 40), b"second")]
    got = [None, None]
    while None in got:
        for i, g in enumerate(gens):                                       # parent round r, fork round r, parent round r + 1, ..
            try:
                next(g)
            except StopIteration as e:
                got[i] = e.value
    assert got == alone
    # ... and the other way round, the fork one round ahead
    gens = [_steps(mj, fork, wires, pub, _blinders(mj, c, fork, 0), b"first"), _steps(mj, parent, wires, pub, _blinders(mj, c, parent, 40), b"second")]
    next(gens[0]), next(gens[0])
    got = [None, None]
    while None in got:
        for i, g in enumerate(gens):
            if got[i] is None:
                try:
                    next(g)
                except StopIteration as e:
                    got[i] = e.value
    assert got == alone
    fork.release()
    parent.release()
    ck.release()


# ---- 3. threads ----------------------------------------------------------------------------------------------------------------------------------
def test_parent_and_forks_prove_from_three_threads(gpu, mj):
    c = mj.params.CURVES[0]
    cs = mj.snark.gen_circuit_for_bench(c, 1000, "TurboPlonk")
    assert cs.n == 1 << 10
    ck = _srs(mj, 0, cs.n)
    parent = mj.snark.preprocess(ck, cs)
    slots = [parent, parent.fork(), parent.fork()]

    def stream(t):                                                          # thread t's rng: the test rng after t draws
        rng = mj.rng.test_rng()
        for _ in range(t):
            mj.rng.fr_rand(c, rng)
        return rng
    want = []
    for t in range(3):
        rng = stream(t)
        want.append([mj.snark.prove(rng, cs, parent)[1] for _ in range(4)])
    assert len({b for row in want for b in row}) == 12
    got, errors, start = [[] for _ in slots], [], threading.Barrier(3)

    def work(t):
        try:
            gpu.check(gpu.load().mzk_init(0), "mzk_init")
            rng = stream(t)
            start.wait()
            for _ in range(4):
                got[t].append(mj.snark.prove(rng, cs, slots[t])[1])
        except Exception as e:                                             # noqa: BLE001
            errors.append(repr(e))
            start.abort()
    threads = [threading.Thread(target=work, args=(t,)) for t in range(3)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not errors, errors
    assert got == want
    for p in slots[::-1]:
        p.release()
    ck.release()


# ---- 4. an aggregate over one circuit ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("curve_id,plonk_type,gates,range_bits", [(0, "TurboPlonk", 30, 8), (1, "UltraPlonk", 20, 4)])
def test_batch_prove_over_a_prover_and_its_forks(gpu, mj, pyref, curve_id, plonk_type, gates, range_bits):
    import pyref_verifier as V
    c, pc = mj.params.CURVES[curve_id], pyref.CURVES[curve_id]
    cs = mj.snark.gen_circuit_for_bench(c, gates, plonk_type, range_bit_len=range_bits)
    assert cs.n == 32
    rng = mj.rng.test_rng()
    srs_beta = mj.rng.fr_rand(c, rng)
    ck = mj.UnivariateProverParam.gen_srs_for_testing(c, srs_beta, cs.n + 2)
    after_srs = lambda: _rng_after_srs(mj, c)
    separate = [mj.snark.preprocess(ck, cs) for _ in range(3)]            # the existing path: three keys of the same circuit
    _, want = mj.snark.batch_prove(after_srs(), [cs, cs, cs], separate)
    pk = mj.snark.preprocess(ck, cs)
    f1 = pk.fork()
    f2 = f1.fork()
    _, got = mj.snark.batch_prove(after_srs(), [cs, cs, cs], [pk, f1, f2])
    assert got == want
    _, again = mj.snark.batch_prove(after_srs(), [cs, cs, cs], [f2, pk, f1])                # any slot may be the first instance
    assert again == want
    vk = verifying_key(mj, pc, pk, 0)
    fresh = lambda: FS.StandardTranscript(pc, b"PlonkProof")
    assert V.verify_batch_proof(pc, fresh(), [vk, vk, vk], [[], [], []], got, pyref.g1_gen(pc), srs_beta)
    with pytest.raises(ValueError):
        mj.snark.batch_prove(after_srs(), [cs, cs], [pk, pk])
    hs = (C.c_uint64 * 2)(pk.handle, pk.handle)                            # ... and below Python: the same HANDLE twice is refused by the library
    a = np.zeros(4, dtype=np.uint64)
    out = np.zeros((8, 2, c.fq_limbs), dtype=np.uint64)
    assert gpu.load().mzk_prover_round3(hs, 2, C.c_void_p(a.ctypes.data), C.c_void_p(a.ctypes.data), C.c_void_p(out.ctypes.data)) == ERR_INVALID_ARG
    for p in separate + [f1, pk, f2]:
        p.release()
    ck.release()


# ---- 5. the variable table -------------------------------------------------------------------------------------------------------------------------
def test_a_fork_shares_the_variable_table_until_it_sets_its_own(gpu, mj, pyref):
    import torch
    curve_id, ultra = 0, False
    c, pc = mj.params.CURVES[curve_id], pyref.CURVES[curve_id]
    sel, sig, k, w, pi, tabs, var, n_vars = _circuit(curve_id, ultra)
    n, r, W, pub = 1 << LOG_N, pc.r, len(var), pi[:4]
    witness = [0] * n_vars
    for i, col in enumerate(var):
        for j, v in enumerate(col):
            witness[v] = w[i][j]
    to_t = lambda ints: torch.from_numpy(fr_mont_limbs(c, ints).view(np.int64))
    table = torch.from_numpy(np.array(var, dtype=np.int32))
    vector = mj.snark.HostWitness(to_t(witness), table)                    # MZK_WITNESS_HOST_VECTOR
    ck = _srs(mj, curve_id)
    parent = _prover_from_structure(mj, curve_id, ultra, ck)
    want = _prove(mj, parent, _limbs(c, w), pub)
    assert _prove(mj, parent, vector, pub) == want
    fork = parent.fork()

    def refuse(*a):
        raise AssertionError("set_wire_variables called on a fork of a prover that holds the table")
    fork.set_wire_variables = refuse
    assert _prove(mj, fork, vector, pub) == want
    del fork.set_wire_variables
    # one corrupted cell of a copy cycle, chosen so that no gate fails: the fork names it from the shared table
    by = {}
    for i, col in enumerate(var):
        for j, v in enumerate(col):
            by.setdefault(v, []).append(i * n + j)
    changed = lambda cell: [[(x + 1) % r if i * n + j == cell else x for j, x in enumerate(col)] for i, col in enumerate(w)]
    cyc = next(cells for cells in by.values() if len(cells) == 3 and all(REF.gate_failures(pc, sel, changed(x), pi) == [] for x in cells))
    bad = _limbs(c, changed(cyc[2]))
    assert REF.copy_failures(changed(cyc[2]), var) == [(cyc[2], cyc[0])]
    reports = lambda p: [p.check_witness(arg, pub) for arg in (bad, torch.from_numpy(bad.view(np.int64)).cuda())]    # HOST_WIRES, DEV_WIRES
    for rep in reports(fork) + reports(parent):
        assert rep.kind == "copy" and rep.copy_checked and rep.copy_failures == 1
        assert rep.copy_cell == (cyc[2] // n, cyc[2] % n) and rep.copy_rep_cell == (cyc[0] // n, cyc[0] % n)
    # another valid table on the fork -- every cell a variable of its own, so no copy constraint at all -- is the fork's alone
    before = parent.hbm_bytes(), parent.shared_hbm_bytes()
    own = np.arange(W * n, dtype=np.uint32).reshape(W, n)
    fork.set_wire_variables(own, W * n)
    for rep in reports(fork):
        assert rep.satisfied and rep.copy_checked and rep.copy_failures == 0
    for rep in reports(parent):
        assert rep.kind == "copy" and rep.copy_cell == (cyc[2] // n, cyc[2] % n) and rep.copy_rep_cell == (cyc[0] // n, cyc[0] % n)
    assert _prove(mj, parent, vector, pub) == want
    cells = mj.snark.HostWitness(to_t([x for col in w for x in col]), torch.from_numpy(own.astype(np.int32)))
    assert _prove(mj, fork, cells, pub) == want                            # the fork gathers W n values through ITS table
    with pytest.raises(gpu.MzkError):
        _prove(mj, fork, vector, pub)                                      # ... and no longer takes the n_vars of the shared one
    assert parent.hbm_bytes() == before[0]
    table_bytes = -(-W * n * 4 // 32) * 32
    assert parent.shared_hbm_bytes() == before[1] and fork.shared_hbm_bytes() == (before[1][0] - table_bytes, 2)
    fork.release()
    assert _prove(mj, parent, vector, pub) == want
    parent.release()
    ck.release()


# ---- 6. the Lagrange key ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("curve_id,ultra", CASES)
def test_a_fork_of_a_prover_with_a_lagrange_key(gpu, mj, curve_id, ultra):
    c = mj.params.CURVES[curve_id]
    sel, sig, k, w, pi, tabs, _, _ = _circuit(curve_id, ultra)
    wires, pub = _limbs(c, w), pi[:4]
    ck = _srs(mj, curve_id)
    lck = ck.lagrange_key(1 << LOG_N)
    parent = _prover(mj, curve_id, ultra, ck, lagrange_ck=lck)
    fork = parent.fork()
    assert fork.lagrange_ck is lck
    want = _prove(mj, parent, wires, pub)
    assert _prove(mj, fork, wires, pub) == want
    plain = _prover(mj, curve_id, ultra, ck)                               # (same commitments from the coefficient forms)
    assert _prove(mj, plain, wires, pub) == want
    for p in (plain, parent, fork):
        p.release()
    lck.release()
    ck.release()


# ---- 7. the key is not copied ----------------------------------------------------------------------------------------------------------------------
def test_a_fork_costs_a_workspace_not_a_key(gpu, mj):
    """The decrease of free device memory across fork() alone, no kernel in between, must stay below workspace + (fixed + proving key) / 2:
    a fork that copied the key would take workspace + key.  From the design, not from a measurement."""
    import torch
    c = mj.params.CURVES[0]
    cs = mj.snark.gen_circuit_for_bench(c, 1 << 16, "TurboPlonk")
    assert cs.n == 1 << 16
    ck = _srs(mj, 0, cs.n)
    parent = mj.snark.preprocess(ck, cs, lagrange=False)
    torch.cuda.synchronize()
    free_before = torch.cuda.mem_get_info()[0]
    fork = parent.fork()
    free_after = torch.cuda.mem_get_info()[0]
    hb = fork.hbm_bytes()
    fixed, key, ws = hb["fixed_coefficient_forms"], hb["proving_key_evaluations"], hb["prover_workspace"]
    drop = free_before - free_after
    print("fork at 2^16 gates: free memory dropped by %d B; workspace %d B, fixed %d B, proving key %d B" % (drop, ws, fixed, key))
    assert fixed + key > 64 << 20                                          # the key dominates allocation granularity (2 MiB)
    assert drop < ws + (fixed + key) // 2
    assert parent.hbm_bytes()["fixed_coefficient_forms"] == fixed and parent.hbm_bytes()["proving_key_evaluations"] == key
    assert mj.snark.prove(_rng_after_srs(mj, c), cs, fork)[1] == mj.snark.prove(_rng_after_srs(mj, c), cs, parent)[1]
    fork.release()
    parent.release()
    ck.release()


# ---- 8. accounting ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_table", [False, True])
def test_shared_hbm_accounting(gpu, mj, with_table):
    ck = _srs(mj, 0)
    parent = (_prover_from_structure if with_table else _prover)(mj, 0, False, ck)
    assert parent.shared_hbm_bytes() == (0, 1)
    before = parent.hbm_bytes()
    table_bytes = -(-5 * (1 << LOG_N) * 4 // 32) * 32 if with_table else 0
    shared = before["fixed_coefficient_forms"] + before["proving_key_evaluations"] + table_bytes
    assert before["fixed_coefficient_forms"] == (13 + 5) * (1 << LOG_N) * 32 and before["proving_key_evaluations"] > 0
    fork = parent.fork()
    assert parent.hbm_bytes() == before and fork.hbm_bytes() == before      # what each handle reaches, shared parts included
    assert parent.shared_hbm_bytes() == (shared, 2) and fork.shared_hbm_bytes() == (shared, 2)
    third = fork.fork()
    assert [p.shared_hbm_bytes() for p in (parent, fork, third)] == [(shared, 3)] * 3
    fork.release()
    assert parent.shared_hbm_bytes() == (shared, 2) and third.shared_hbm_bytes() == (shared, 2)
    parent.release()                                                       # either handle: here the one that made the key
    assert third.shared_hbm_bytes() == (0, 1) and third.hbm_bytes() == before
    other = third.fork()
    third.release()
    assert other.shared_hbm_bytes() == (0, 1) and other.hbm_bytes() == before
    other.release()
    ck.release()


# ---- 9. errors -------------------------------------------------------------------------------------------------------------------------------------
class _TwoRanks:
    """an mzk_comm of two ranks whose callbacks must never run: creating a prover makes no collective call"""

    def __init__(self):
        AG = C.CFUNCTYPE(C.c_int32, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p)
        BA = C.CFUNCTYPE(C.c_int32, C.c_void_p)
        EX = C.CFUNCTYPE(C.c_int32, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32)

        class Comm(C.Structure):
            _fields_ = [("ctx", C.c_void_p), ("rank", C.c_int32), ("world", C.c_int32), ("all_gather", AG), ("barrier", BA), ("exchange_classes", EX)]
        self.calls = 0
        self._cb = (AG(self._called), BA(self._called), EX(self._called))
        self._struct = Comm(None, 0, 2, *self._cb)

    def _called(self, *a):
        self.calls += 1
        return 1

    def struct_ptr(self):
        return C.cast(C.pointer(self._struct), C.c_void_p)


def test_fork_errors(gpu, mj):
    L = gpu.load()
    c = mj.params.CURVES[0]
    sel, sig, k, w, pi, tabs, _, _ = _circuit(0, False)
    ck = _srs(mj, 0)
    parent = _prover(mj, 0, False, ck)
    out = C.c_uint64(7)
    assert L.mzk_prover_fork(parent.handle + 1000, C.byref(out)) == ERR_BAD_HANDLE and out.value == 7
    assert L.mzk_prover_fork(parent.handle, None) == ERR_INVALID_ARG
    assert L.mzk_prover_shared_hbm_bytes(parent.handle + 1000, None, None) == ERR_BAD_HANDLE
    assert parent.shared_hbm_bytes() == (0, 1)                             # the refused calls left no slot behind
    comm = _TwoRanks()
    ranked = _prover(mj, 0, False, ck, comm=comm)
    assert L.mzk_prover_fork(ranked.handle, C.byref(out)) == ERR_UNSUPPORTED and out.value == 7
    assert b"collectives" in L.mzk_last_error() and comm.calls == 0
    with pytest.raises(gpu.MzkError) as e:
        ranked.fork()
    assert e.value.code == ERR_UNSUPPORTED
    ranked.release()
    # rounds out of order on a fork, whatever its parent is doing
    wires, pub = _limbs(c, w), pi[:4]
    blind = _blinders(mj, c, parent)
    parent.round1(wires, pub, blind.wires)                                 # the parent has a proof in flight when it is forked
    fork = parent.fork()
    for call in (lambda: fork.round2(1, 2, blind.z), lambda: mj.prover.round3([fork], 3, blind.quot), lambda: fork.round4(5),
                 lambda: mj.prover.round5([fork], 7), lambda: mj.prover.round3([parent, fork], 3, blind.quot)):
        with pytest.raises(gpu.MzkError) as e:
            call()
        assert e.value.code == ERR_STATE
    fork.round1(wires, pub, blind.wires)
    with pytest.raises(gpu.MzkError) as e:
        fork.round4(5)
    assert e.value.code == ERR_STATE
    want = _prove(mj, parent, wires, pub)
    assert _prove(mj, fork, wires, pub) == want
    fork.release()
    parent.release()
    ck.release()


# ---- 10. the C++ host ----------------------------------------------------------------------------------------------------------------------------
def test_cpp_host_proves_through_three_slots(gpu, mj):
    if not os.path.exists(BIN):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "mpc-jellyfish_amd", "host"), "-s"])
    out = subprocess.run([BIN, "0", "turbo", "1024", "2", "--slots", "3", "--check-agree"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    got = json.loads(out.stdout.strip().splitlines()[-1])
    assert got["slots"] == 3 and got["sharers"] == 3 and got["slots_agree_with_one_slot"] is True and got["proofs_per_s"] > 0
    per_slot = got["hbm_fixed_bytes"] + got["hbm_proving_key_bytes"] + got["hbm_workspace_bytes"]
    assert got["hbm_shared_bytes"] == got["hbm_fixed_bytes"] + got["hbm_proving_key_bytes"]
    assert got["family_hbm_bytes"] == 3 * per_slot - 2 * got["hbm_shared_bytes"]
    one = subprocess.run([BIN, "0", "turbo", "1024", "0"], capture_output=True, text=True, timeout=600)    # without --slots: the program as it was
    assert one.returncode == 0, one.stderr[-2000:]
    assert json.loads(one.stdout.strip().splitlines()[-1])["proof_hex"] == got["proof_hex"]
