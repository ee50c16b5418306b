"""GPU: proving keys from circuit structure (mzk_plonk_sigma_values_dev, mzk_prover_create_from_circuit[_dev]; include/mzk.h) -- the
selector VALUES and the variable table of a finalised circuit must give the key, the verifying-key commitments and the proof bytes that
the coefficient forms of PlonkKzgSnark::preprocess (plonk/src/proof_system/snark.rs:529-617) give."""
import ctypes as C
import random
from functools import lru_cache

import numpy as np
import pytest

import check_witness_ref as REF
from conftest import build_circuit, build_ultra_circuit, fr_mont_limbs, load_golden, verifying_key

pytestmark = pytest.mark.gpu
TABLES = ("range", "key", "table_dom_sep", "q_dom_sep")


# ---- sigma values --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("curve_id,ultra,num_gates,range_bits,n", [(0, False, 24, 8, 16), (1, False, 24, 8, 16), (0, True, 24, 3, 16), (1, True, 24, 3, 16),
                                                                   (0, True, 40, 4, 32), (1, True, 40, 4, 32)])
def test_sigma_values_of_the_bench_circuit(gpu, mj, pyref, curve_id, ultra, num_gates, range_bits, n):
    import torch
    import pyref_circuit as PC
    L = gpu.load()
    c, pc = mj.params.CURVES[curve_id], pyref.CURVES[curve_id]
    W = 6 if ultra else 5
    k = mj.rng.compute_coset_representatives(c, W, n)
    got_n, wires, witness, _, sigma, _ = PC.bench_circuit(pc, num_gates, ultra, range_bits, k)
    assert got_n == n
    d_var = torch.tensor(wires, dtype=torch.int32, device="cuda").contiguous()
    d_next = torch.empty(W * n, dtype=torch.int32, device="cuda")
    d_sigma = torch.zeros((W, n, 4), dtype=torch.int64, device="cuda")
    kk = mj.params.fr_to_mont(c, k)
    torch.cuda.synchronize()
    assert L.mzk_plonk_wire_permutation_dev(C.c_void_p(d_var.data_ptr()), W * n, len(witness), C.c_void_p(d_next.data_ptr()), None) == 0
    assert L.mzk_plonk_sigma_values_dev(curve_id, n.bit_length() - 1, W, C.c_void_p(d_next.data_ptr()), C.c_void_p(kk.ctypes.data), C.c_void_p(d_sigma.data_ptr()),
                                        None) == 0
    torch.cuda.synchronize()
    want = np.stack([fr_mont_limbs(c, row) for row in sigma])
    assert np.array_equal(d_sigma.cpu().numpy().view(np.uint64), want)


# ---- the golden bench proofs -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("index", [0, 1, 2, 3])
def test_from_structure_prover_reproduces_the_golden_proof(gpu, mj, index):
    vec = load_golden("proof_vectors")[index]
    c = mj.params.CURVES[vec["curve"]]
    cs = mj.snark.gen_circuit_for_bench(c, vec["num_gates"], vec["plonk_type"], range_bit_len=vec["range_bit_len"])
    cs.sigma_values = None                                             # not read on this path
    rng = mj.rng.test_rng()
    ck = mj.UnivariateProverParam.gen_srs_for_testing(c, mj.rng.fr_rand(c, rng), cs.n + 2)
    pk = mj.snark.preprocess(ck, cs, from_structure=True)
    g1 = lambda x: mj.snark._g1(c, x).hex()
    sel, sig = pk.vk_commitments()
    assert [g1(x) for x in sel] == vec["selector_comms"] and [g1(x) for x in sig] == vec["sigma_comms"]
    if pk.ultra:
        names = ("range_table_comm", "key_table_comm", "table_dom_sep_comm", "q_dom_sep_comm")
        assert dict(zip(names, [g1(x) for x in pk.plookup_vk_commitments()])) == vec["plookup_comms"]
    _, proof_bytes = mj.snark.prove(rng, cs, pk)
    assert proof_bytes.hex() == vec["proof"]
    pk.release()
    ck.release()


# ---- general circuits ------------------------------------------------------------------------------------------------------------------
LOG_N = 5


@lru_cache(maxsize=None)
def _general(curve_id, ultra, gates):
    """the circuit's integers, its variable table (cells of one sigma-cycle share a variable) and the CANONICAL sigma of that table:
    the builders link their cycles in shuffled order, the reference in cell order (oracle/pyref_circuit.py:55-63)"""
    import pyref
    pc = pyref.CURVES[curve_id]
    rng = random.Random(8800 + curve_id + 2 * ultra + (gates == "all"))
    if ultra:
        sel, sig, k, w, pi, tabs = build_ultra_circuit(pc, LOG_N, rng, gates=gates)
    else:
        sel, sig, k, w, pi = build_circuit(pc, LOG_N, rng, gates=gates)
        tabs = None
    var, n_vars = REF.wire_variables_from_sigma(pc, sig, k, LOG_N)
    n, W, r = 1 << LOG_N, len(var), pc.r
    occ = [[] for _ in range(n_vars)]
    for i in range(W):
        for j, v in enumerate(var[i]):
            occ[v].append((i, j))
    perm = {}
    for lst in occ:
        for q, cell in enumerate(lst):
            perm[cell] = lst[(q + 1) % len(lst)]
    w_n = pc.root_of_unity(LOG_N)
    canon = [[k[perm[(i, j)][0]] * pow(w_n, perm[(i, j)][1], r) % r for j in range(n)] for i in range(W)]
    assert REF.wire_variables_from_sigma(pc, canon, k, LOG_N) == (var, n_vars)
    return sel, canon, k, w, pi, tabs, var, n_vars


def _provers(mj, curve_id, ultra, gates, beta=0x5EED):
    """(coefficient-form prover of the canonical sigma, from-structure prover of the variable table, commit key, the circuit)"""
    c = mj.params.CURVES[curve_id]
    sel, canon, k, w, pi, tabs, var, n_vars = _general(curve_id, ultra, gates)
    n = 1 << LOG_N
    dom = mj.Radix2EvaluationDomain(c, LOG_N)
    limbs = lambda rows: np.stack([fr_mont_limbs(c, row) for row in rows])
    kw = {"plookup": {name: dom.ifft(fr_mont_limbs(c, tabs[key])) for name, key in zip(mj.plonk.PLOOKUP_TABLE_POLYS, TABLES)}} if ultra else {}
    ck = mj.UnivariateProverParam.gen_srs_for_testing(c, beta, n + 2)
    by_coeffs = mj.prover.TurboPlonkProver(c, n, [dom.ifft(fr_mont_limbs(c, s)) for s in sel], [dom.ifft(fr_mont_limbs(c, s)) for s in canon], k, ck, **kw)
    by_structure = mj.prover.TurboPlonkProver.from_circuit(c, n, limbs(sel), np.array(var, dtype=np.uint32), n_vars, k, ck,
                                                           table_values=limbs([tabs[key] for key in TABLES]) if ultra else None)
    return by_coeffs, by_structure, ck, limbs


@pytest.mark.parametrize("curve_id,ultra,gates", [(0, False, "hot"), (1, False, "all"), (1, True, "hot"), (0, True, "all")])
def test_general_circuits_from_host_arrays(gpu, mj, pyref, curve_id, ultra, gates):
    import pyref_fs as FS
    import pyref_verifier as V
    c, pc = mj.params.CURVES[curve_id], pyref.CURVES[curve_id]
    sel, canon, k, w, pi, tabs, var, n_vars = _general(curve_id, ultra, gates)
    by_coeffs, by_structure, ck, limbs = _provers(mj, curve_id, ultra, gates)
    W, pub, wires = len(var), pi[:4], limbs(w)
    pts = lambda comms: [x.xy.tobytes() for x in comms]
    for a, b in zip(by_coeffs.vk_commitments(), by_structure.vk_commitments()):
        assert pts(a) == pts(b)
    if ultra:
        assert pts(by_coeffs.plookup_vk_commitments()) == pts(by_structure.plookup_vk_commitments())
    proofs = []
    for p in (by_coeffs, by_structure):
        blind = mj.snark.draw_blinders(c, mj.rng.test_rng(), W, ultra)
        proofs.append(mj.snark.serialize_proof(c, p.prove(wires, pub, mj.prover.TranscriptChallenges(p, pub), blind)))
    assert proofs[0] == proofs[1]
    vk = verifying_key(mj, pc, by_structure, len(pub))
    assert V.verify(pc, FS.StandardTranscript(pc, b"PlonkProof"), vk, pub, proofs[1], pyref.g1_gen(pc), 0x5EED)
    by_coeffs.release()
    by_structure.release()
    ck.release()


def test_a_table_index_outside_the_variables_is_refused(gpu, mj):
    c = mj.params.CURVES[0]
    sel, canon, k, w, pi, tabs, var, n_vars = _general(0, False, "hot")
    n = 1 << LOG_N
    ck = mj.UnivariateProverParam.gen_srs_for_testing(c, 3, n + 2)
    bad = np.array(var, dtype=np.uint32)
    bad[2, 5] = n_vars
    with pytest.raises(gpu.MzkError) as e:
        mj.prover.TurboPlonkProver.from_circuit(c, n, np.stack([fr_mont_limbs(c, row) for row in sel]), bad, n_vars, k, ck)
    assert e.value.code == -1 and "cell %d " % (2 * n + 5) in str(e.value)
    ck.release()


# ---- the witness check and the witness kinds ---------------------------------------------------------------------------------------------
def test_check_witness_finds_a_broken_copy_in_wire_witnesses(gpu, mj, pyref):
    import torch
    curve_id = 0
    c, pc = mj.params.CURVES[curve_id], pyref.CURVES[curve_id]
    sel, canon, k, w, pi, tabs, var, n_vars = _general(curve_id, False, "hot")
    by_coeffs, by_structure, ck, limbs = _provers(mj, curve_id, False, "hot")
    n, r, pub = 1 << LOG_N, pc.r, pi[:4]
    by = {}
    for i, col in enumerate(var):
        for j, v in enumerate(col):
            by.setdefault(v, []).append(i * n + j)
    changed = lambda cell: [[(x + 1) % r if i * n + j == cell else x for j, x in enumerate(col)] for i, col in enumerate(w)]
    cyc = next(cells for cells in by.values() if len(cells) == 3 and all(REF.gate_failures(pc, sel, changed(x), pi) == [] for x in cells))
    bad = changed(cyc[2])
    for name, arg in (("host wires", limbs(bad)), ("device wires", torch.from_numpy(limbs(bad).view(np.int64)).cuda())):
        rep = by_structure.check_witness(arg, pub)
        assert rep.kind == "copy" and rep.copy_checked and rep.copy_failures == 1, name
        assert rep.copy_cell == (cyc[2] // n, cyc[2] % n) and rep.copy_rep_cell == (cyc[0] // n, cyc[0] % n), name
        assert REF.copy_failures(bad, var) == [(cyc[2], cyc[0])]
        rep = by_coeffs.check_witness(arg, pub)                          # the same key from coefficient forms has no table
        assert not rep.copy_checked and rep.kind == "satisfied", name
    rep = by_structure.check_witness(limbs(w), pub)
    assert rep.satisfied and rep.copy_checked
    by_coeffs.release()
    by_structure.release()
    ck.release()


def test_witness_vectors_prove_without_set_wire_variables(gpu, mj):
    vec = load_golden("proof_vectors")[0]
    c = mj.params.CURVES[vec["curve"]]
    cs = mj.snark.gen_circuit_for_bench(c, vec["num_gates"], vec["plonk_type"], range_bit_len=vec["range_bit_len"])
    for witness in (cs.witness.cpu(), cs.witness):                        # MZK_WITNESS_HOST_VECTOR, MZK_WITNESS_DEV_VECTOR
        rng = mj.rng.test_rng()
        ck = mj.UnivariateProverParam.gen_srs_for_testing(c, mj.rng.fr_rand(c, rng), cs.n + 2)
        pk = mj.snark.preprocess(ck, cs, from_structure=True)

        def refuse(*a):
            raise AssertionError("set_wire_variables called on a prover that holds the table")
        pk.set_wire_variables = refuse
        hw = mj.snark.HostWitness(witness, cs.wire_variables.clone())      # another table object: identity of the tensor must not matter
        rep = pk.check_witness(hw, [])
        assert rep.satisfied and rep.copy_checked
        _, proof_bytes = mj.snark.prove(rng, cs, pk, witness=hw)
        assert proof_bytes.hex() == vec["proof"]
        pk.release()
        ck.release()


# ---- the reference's bench size ----------------------------------------------------------------------------------------------------------
def test_verifying_key_at_the_bench_size(gpu, mj):
    """2^15 gates, TurboPlonk / BLS12-381 (plonk/benches/bench.rs): 128 tiles of the sort per wire, a heavy run (`zero` on 3n of 5n cells)"""
    c = mj.params.CURVES[0]
    cs = mj.snark.gen_circuit_for_bench(c, (1 << 15) + 8, "TurboPlonk")
    assert cs.n == 1 << 15
    ck = mj.UnivariateProverParam.gen_srs_for_testing(c, 0xBE7A, cs.n + 2)
    pts = lambda comms: [x.xy.tobytes() for x in comms]
    got = []
    for from_structure in (False, True):
        pk = mj.snark.preprocess(ck, cs, from_structure=from_structure)
        got.append([pts(x) for x in pk.vk_commitments()])
        pk.release()
    assert got[0] == got[1]
    ck.release()
