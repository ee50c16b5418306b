"""GPU: proofs under the Keccak-256 (Solidity) transcript from every host -- snark.prove, batch_prove, linking.link_proofs and the
compiled host (mzk_prove --transcript solidity) -- against the schoolbook oracle (oracle/pyref_snark.py, pyref_linking.py) taking the
oracle's SolidityTranscript through tests/solidity_adapter.py.  Circuits, `test_rng` draws and SRS are those of the Merlin golden vectors
(tests/golden/make_proof_golden.py: CASES, BATCH_CASES, LINK_CASES), so the bytes differ from the golden ones by the transcript alone."""
import json
import os
import subprocess

import pytest

from conftest import load_golden, verifying_key
import pyref_circuit as PC
import pyref_fs as FS
import pyref_rng as RNG
import pyref_snark as PS
from solidity_adapter import SolidityPlonkTranscript

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "mpc-jellyfish_amd", "mzk_prove")


def _bench(pc, plonk_type, gates, range_bits):
    ultra = plonk_type == "UltraPlonk"
    W = 6 if ultra else 5
    n = PC.bench_circuit(pc, gates, ultra, range_bits, list(range(1, W + 1)))[0]
    k = RNG.compute_coset_representatives(pc, W, n)
    n, wires, witness, sel, sigma, tables = PC.bench_circuit(pc, gates, ultra, range_bits, k)
    return n, k, sel, sigma, [[witness[v] for v in wires[i]] for i in range(W)], tables


def _oracle_prove(pc, plonk_type, gates, range_bits, rng, srs_beta, extra=None):
    n, k, sel, sigma, w_vals, tables = _bench(pc, plonk_type, gates, range_bits)
    blind = RNG.draw_blinders(pc, rng, len(w_vals), plonk_type == "UltraPlonk")
    return PS.prove(pc, n.bit_length() - 1, sel, sigma, k, w_vals, [0] * n, [], blind, srs_beta, SolidityPlonkTranscript(pc), lambda p: FS.g1_bytes(pc, p),
                    lambda x: FS.fr_bytes(pc, x), plookup=tables, extra_msg=extra)


@pytest.mark.parametrize("index", [0, 1, 2, 3])
def test_prove_emits_the_oracles_bytes_and_they_verify(gpu, mj, pyref, index):
    import pyref_verifier as V
    vec = load_golden("proof_vectors")[index]
    cid, plonk_type, gates, range_bits = vec["curve"], vec["plonk_type"], vec["num_gates"], vec["range_bit_len"]
    c, pc = mj.params.CURVES[cid], pyref.CURVES[cid]
    extra = None if index % 2 else b"extra"
    orng = RNG.test_rng()
    srs_beta = RNG.fr_rand(pc, orng)
    want = _oracle_prove(pc, plonk_type, gates, range_bits, orng, srs_beta, extra)["proof"]
    cs = mj.snark.gen_circuit_for_bench(c, gates, plonk_type, range_bit_len=range_bits)
    rng = mj.rng.test_rng()
    assert mj.rng.fr_rand(c, rng) == srs_beta
    ck = mj.UnivariateProverParam.gen_srs_for_testing(c, srs_beta, cs.n + 2)
    pk = mj.snark.preprocess(ck, cs)
    _, proof = mj.snark.prove(rng, cs, pk, extra, transcript="solidity")
    assert proof == want and proof.hex() != vec["proof"] and len(proof) == len(vec["proof"]) // 2
    _, again = mj.snark.prove(mj.rng.test_rng(), cs, pk, extra, transcript="solidity")       # (the head cache keys on the kind: a Merlin proof in between)
    _, merlin = mj.snark.prove(mj.rng.test_rng(), cs, pk, extra)
    _, third = mj.snark.prove(mj.rng.test_rng(), cs, pk, extra, transcript="solidity")
    assert again == third != merlin
    _, h, beta_h = mj.kzg.open_key_for_testing(c, srs_beta)
    vk = mj.keys.VerifyingKey.deserialize(cid, pk.serialize_vk(0, h, beta_h))
    assert mj.snark.verify(vk, [], proof, extra, transcript="solidity") is True
    assert mj.snark.verify(vk, [], proof, extra) is False and mj.snark.verify(vk, [], merlin, extra, transcript="solidity") is False
    if index in (1, 3):                                               # the oracle's verifier, pairing included: one case per curve
        assert V.verify(pc, SolidityPlonkTranscript(pc), verifying_key(mj, pc, pk, 0), [], proof, None, None, extra_msg=extra,
                        open_key=V.open_key_for_testing(pc, srs_beta))
    vk.release_verifier()
    pk.release()
    ck.release()


@pytest.mark.parametrize("index", [0, 1])
def test_batch_prove_emits_the_oracles_bytes(gpu, mj, pyref, index):
    vec = load_golden("batch_vectors")[index]
    cid, plonk_type, gates, range_bits = vec["curve"], vec["plonk_type"], vec["gates"], vec["range_bit_len"]
    c, pc = mj.params.CURVES[cid], pyref.CURVES[cid]
    ultra = plonk_type == "UltraPlonk"
    W = 6 if ultra else 5
    orng = RNG.test_rng()
    srs_beta = RNG.fr_rand(pc, orng)
    blinds, quot = RNG.draw_batch_blinders(pc, orng, W, [ultra] * len(gates))
    instances = []
    for g, bl in zip(gates, blinds):
        n, k, sel, sigma, w_vals, tables = _bench(pc, plonk_type, g, range_bits)
        instances.append({"selector_vals": sel, "sigma_vals": sigma, "k": k, "wire_vals": w_vals, "pi_vals": [0] * n, "blind": bl, "plookup": tables})
    want = PS.batch_prove(pc, n.bit_length() - 1, instances, [[] for _ in gates], quot, srs_beta, SolidityPlonkTranscript(pc), lambda p: FS.g1_bytes(pc, p),
                          lambda x: FS.fr_bytes(pc, x), extra_msg=b"batch")["proof"]
    circuits = [mj.snark.gen_circuit_for_bench(c, g, plonk_type, range_bit_len=range_bits) for g in gates]
    rng = mj.rng.test_rng()
    ck = mj.UnivariateProverParam.gen_srs_for_testing(c, mj.rng.fr_rand(c, rng), circuits[0].n + 2)
    pks = [mj.snark.preprocess(ck, cs) for cs in circuits]
    _, blob = mj.snark.batch_prove(rng, circuits, pks, b"batch", transcript="solidity")
    assert blob == want
    _, h, beta_h = mj.kzg.open_key_for_testing(c, srs_beta)
    vks = [mj.keys.VerifyingKey.deserialize(cid, pk.serialize_vk(0, h, beta_h)) for pk in pks]
    assert mj.snark.verify_batch_proof(vks, [[]] * len(gates), blob, b"batch", transcript="solidity") is True
    assert mj.snark.verify_batch_proof(vks, [[]] * len(gates), blob, b"batch") is False
    out = subprocess.run([BIN, str(cid), "batch", "ultra" if ultra else "turbo", str(range_bits)] + [str(g) for g in gates] + ["--transcript", "solidity"],
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    _, plain = mj.snark.batch_prove(_after_srs(mj, c), circuits, pks, transcript="solidity")
    assert json.loads(out.stdout.strip().splitlines()[-1])["batch_proof_hex"] == plain.hex()
    for vk in vks:
        vk.release_verifier()
    for pk in pks:
        pk.release()
    ck.release()


def _after_srs(mj, c):
    rng = mj.rng.test_rng()
    mj.rng.fr_rand(c, rng)
    return rng


@pytest.mark.parametrize("index", [0, 1])
def test_link_proofs_emits_the_oracles_bytes(gpu, mj, pyref, index):
    import pyref_linking as L
    vec = load_golden("link_vectors")[index]
    cid, gates, layout_args = vec["curve"], vec["gates"], tuple(vec["layout"])
    c, pc = mj.params.CURVES[cid], pyref.CURVES[cid]
    orng = RNG.test_rng()
    srs_beta = RNG.fr_rand(pc, orng)
    outs = [_oracle_prove(pc, "TurboPlonk", g, 8, orng, srs_beta) for g in gates]
    G = pyref.g1_gen(pc)
    a = [o["core"]["wire_polys"][0] for o in outs]
    comms = [pyref.g1_mul(pc, o["core"]["commit_dlogs"]["wires"][0], G) for o in outs]
    lp = L.link_proofs(pc, a[0], a[1], comms[0], comms[1], L.GroupLayout(*layout_args), srs_beta, SolidityPlonkTranscript(pc, b"PlonkLinkingProof"))
    want = L.serialize_link_proof(lambda p: FS.g1_bytes(pc, p), lp["quotient_commitment"], lp["opening_proof"])
    circuits = [mj.snark.gen_circuit_for_bench(c, g, "TurboPlonk", range_bit_len=8) for g in gates]
    rng = mj.rng.test_rng()
    ck = mj.UnivariateProverParam.gen_srs_for_testing(c, mj.rng.fr_rand(c, rng), circuits[0].n + 2)
    pks = [mj.snark.preprocess(ck, cs) for cs in circuits]
    proofs, hints = [], []
    for cs, pk in zip(circuits, pks):
        _, proof, hint = mj.snark.prove_with_link_hint(rng, cs, pk, transcript="solidity")
        proofs.append(proof), hints.append(hint)
    assert proofs == [o["proof"] for o in outs]
    layout = mj.linking.GroupLayout(*layout_args)
    link = mj.linking.link_proofs(hints[0], hints[1], layout, ck, transcript="solidity").serialize_compressed()
    assert link == want and link.hex() != vec["link_proof"]
    _, h, beta_h = mj.kzg.open_key_for_testing(c, srs_beta)
    vk = mj.keys.VerifyingKey.deserialize(cid, pks[0].serialize_vk(0, h, beta_h))
    assert mj.linking.verify_link_proof(proofs[0], proofs[1], link, layout, vk, transcript="solidity") is True
    out = subprocess.run([BIN, str(cid), "link", str(gates[0]), str(gates[1])] + [str(x) for x in layout_args] + ["--transcript", "solidity"],
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    got = json.loads(out.stdout.strip().splitlines()[-1])
    assert (got["proof1_hex"], got["proof2_hex"], got["link_proof_hex"]) == (proofs[0].hex(), proofs[1].hex(), link.hex())
    vk.release_verifier()
    for pk in pks:
        pk.release()
    ck.release()


@pytest.mark.parametrize("cid,kind", [(1, "turbo"), (0, "ultra")])
def test_cpp_host_prints_the_python_routes_bytes(gpu, mj, cid, kind):
    """mzk_prove <curve> turbo|ultra 64 1 --transcript solidity: the proof of snark.prove(transcript="solidity"), which verifies"""
    c = mj.params.CURVES[cid]
    cs = mj.snark.gen_circuit_for_bench(c, 64, "UltraPlonk" if kind == "ultra" else "TurboPlonk")
    rng = mj.rng.test_rng()
    srs_beta = mj.rng.fr_rand(c, rng)
    ck = mj.UnivariateProverParam.gen_srs_for_testing(c, srs_beta, cs.n + 2)
    pk = mj.snark.preprocess(ck, cs)
    _, proof = mj.snark.prove(rng, cs, pk, transcript="solidity")
    _, merlin = mj.snark.prove(_after_srs(mj, c), cs, pk)
    for args, want in ((["--transcript", "solidity"], proof), ([], merlin)):
        out = subprocess.run([BIN, str(cid), kind, "64", "1"] + args, capture_output=True, text=True, timeout=600)
        assert out.returncode == 0, out.stderr[-2000:]
        assert json.loads(out.stdout.strip().splitlines()[-1])["proof_hex"] == want.hex(), args
    _, h, beta_h = mj.kzg.open_key_for_testing(c, srs_beta)
    vk = mj.keys.VerifyingKey.deserialize(cid, pk.serialize_vk(0, h, beta_h))
    assert mj.snark.verify(vk, [], proof, None, transcript="solidity") is True
    out = subprocess.run([BIN, str(cid), kind, "64", "1", "--transcript", "rescue"], capture_output=True, text=True, timeout=60)
    assert out.returncode == 2 and "merlin or solidity" in out.stderr
    vk.release_verifier()
    pk.release()
    ck.release()
