"""GPU: the verifier's Fiat-Shamir stage under the Keccak-256 (Solidity) transcript (MZK_TRANSCRIPT_SOLIDITY: csrc/keccak_transcript.cuh,
the SolidityTranscript instantiations of the three transcript kernels of csrc/verifier.cuh) against the oracle's SolidityTranscript driven
through pyref_verifier / pyref_linking (tests/solidity_adapter.py), for single proofs, aggregated BatchProofs and proof links; then
accept / reject decisions on proofs the device prover made under that transcript.  The keys, circuits and proof images are those of
tests/test_verify_gpu.py and tests/test_verify_aggregate_gpu.py: a challenge does not care whether the proof it is drawn from is valid."""
import ctypes as C
import random

import numpy as np
import pytest

from conftest import build_circuit, fr_mont_limbs, fr_from_mont_limbs, verifying_key
import pyref_fs as FS
from solidity_adapter import CH, SOLIDITY, SolidityPlonkTranscript, oracle_batch_challenge
from test_verify_gpu import ALL, EXTRAS, SETUPS, _uncompressed_proof, world  # noqa: F401  (world: the module fixture, built once for this file)
from test_verify_aggregate_gpu import _build_world, _serialize_bp
from test_link_verify_gpu import _g1_uncompressed

pytestmark = pytest.mark.gpu

K_EDGES = 130                                                      # three blocks of 64 threads, the last ragged
RESIDUES = (135, 0, 1)                                             # of the hashed length mod 136: the pad in a block of its own, a block just filled, one byte in
_memo = {}


def _oracle(pc, case, extra):
    """(the seven challenges, the transcript length at each) of proof 0 of the case under `extra`, once per distinct message"""
    import pyref_verifier as V
    key = (pc.curve_id, id(case), extra)
    if key not in _memo:
        t = SolidityPlonkTranscript(pc)
        ch = V.compute_challenges(t, case.ovk, case.pub, case.pr[0], extra)
        _memo[key] = ([ch[x] for x in CH], list(t.lens))
    return _memo[key]


def _edge_messages(pc, case):
    """None, b"", 300 bytes, and for each of the 7 challenges and each residue a message length e with 65 + e + L_k = residue mod 136
    (65: the 64 bytes of the state and the suffix byte; L_k: the transcript length at challenge k without an extra message)"""
    rng = random.Random(135)
    _, L = _oracle(pc, case, None)
    assert len(L) == 7 and L == sorted(L)
    msgs = [None, b"", rng.randbytes(300)]
    for k in range(7):
        for rho in RESIDUES:
            e = (rho - 65 - L[k]) % 136 or 136
            msgs.append(rng.randbytes(e))
    assert len(msgs) == 24 and len(set(msgs)) == 24
    # the condition itself, from the lengths the oracle hashed: every (challenge, residue) pair is hit
    hit = {(k, (65 + n) % 136) for m in msgs[3:] for k, n in enumerate(_oracle(pc, case, m)[1])}
    assert {(k, rho) for k in range(7) for rho in RESIDUES} <= hit
    return msgs


@pytest.mark.parametrize("compress", [True, False])
@pytest.mark.parametrize("cid,j", ALL)
def test_challenges_at_the_padding_edges(world, mj, pyref, cid, j, compress):
    import pyref_verifier as V
    w = world[cid]
    case, c, pc = w["cases"][j], mj.params.CURVES[cid], pyref.CURVES[cid]
    msgs = _edge_messages(pc, case)
    vk, image = case.vk, case.proofs[0]
    if not compress:
        _, h, beta_h = mj.kzg.open_key_for_testing(c, w["beta"], compress=False)
        vk = mj.keys.VerifyingKey.deserialize(cid, case.prover.serialize_vk(len(case.pub), h, beta_h, compress=False), compress=False)
        image = _uncompressed_proof(pc, case.pr[0])
    extras = [msgs[n % len(msgs)] for n in range(K_EDGES)]
    b = vk.verifier().begin([image] * K_EDGES, [case.pub] * K_EDGES, extras, transcript="solidity")
    got = fr_from_mont_limbs(c, b.challenges().reshape(-1, 4))
    u = fr_from_mont_limbs(c, b.u)
    b.discard()
    for n, m in enumerate(extras):
        want = _oracle(pc, case, m)[0]
        assert got[7 * n:7 * n + 7] == want, (n, None if m is None else len(m))
        assert u[n] == want[6]
    assert _oracle(pc, case, None)[0] == _oracle(pc, case, b"")[0] and len(set(_oracle(pc, case, None)[0])) == 7
    # the flag absent: the same call gives Merlin's values, the existing ones
    b = vk.verifier().begin([image] * K_EDGES, [case.pub] * K_EDGES, extras)
    got = fr_from_mont_limbs(c, b.challenges().reshape(-1, 4))
    b.discard()
    merlin = {m: V.compute_challenges(FS.StandardTranscript(pc, b"PlonkProof"), case.ovk, case.pub, case.pr[0], m) for m in (b"", msgs[2])}
    merlin[None] = case.ch[0]
    for n, m in enumerate(extras):
        if m in merlin:
            assert got[7 * n:7 * n + 7] == [merlin[m][x] for x in CH], n
            assert got[7 * n:7 * n + 7] != _oracle(pc, case, m)[0]
    if not compress:
        vk.release_verifier()


# ---- aggregated proofs --------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=[(1, False), (0, True)], ids=["bn254-turbo", "bls12_381-ultra"])
def agg_world(request, gpu, mj, pyref):
    w = _build_world(mj, pyref, *request.param)
    yield w
    for vk in w.vks:
        vk.release_verifier()
    for p in w.provers:
        p.release()
    w.ck.release()


def test_aggregate_challenges(agg_world, mj):
    import pyref_verifier as V
    w = agg_world
    for m in (1, 2, 3):
        es = [0, 1, 1, 0, 1]
        extras = [None, b"an extra transcript message"]
        agg = mj.keys.AggregateVerifier(w.vks[:m])
        b = agg.begin([w.bp[m, e] for e in es], [w.pubs[:m]] * len(es), [extras[e] for e in es], transcript="solidity")
        got = fr_from_mont_limbs(w.c, b.challenges().reshape(-1, 4))
        u = fr_from_mont_limbs(w.c, b.u)
        b.discard()
        want = [V.compute_challenges_batch(SolidityPlonkTranscript(w.pc), w.ovks[:m], w.pubs[:m], w.parsed[m, e], extras[e]) for e in (0, 1)]
        for n, e in enumerate(es):
            assert got[7 * n:7 * n + 7] == [want[e][x] for x in CH], (m, n)
            assert u[n] == want[e]["u"] and want[e]["u"] != w.ch[m, e]["u"]


def test_one_instance_is_the_single_proof_kernel(agg_world, mj):
    import pyref_verifier as V
    w = agg_world
    c, pc, p, pub = w.c, w.pc, w.provers[0], w.pubs[0]
    blind = mj.snark.draw_blinders(c, mj.rng.test_rng(), w.W, w.ultra)
    extras = [None, b"one instance"]
    proof = mj.snark.serialize_proof(c, p.prove(w.wires[0], pub, mj.prover.TranscriptChallenges(p, pub, None, "solidity"), blind))
    image = _serialize_bp(pc, V.batch_proof_from(V.deserialize_proof(pc, proof)))
    single = w.vks[0].verifier().begin([proof] * 2, [pub] * 2, extras, transcript="solidity")
    both = mj.keys.AggregateVerifier([w.vks[0]]).begin([image] * 2, [[pub]] * 2, extras, transcript="solidity")
    assert np.array_equal(single.challenges(), both.challenges()) and np.array_equal(single.u, both.u)
    want = V.compute_challenges(SolidityPlonkTranscript(pc), w.ovks[0], pub, V.deserialize_proof(pc, proof), None)
    assert fr_from_mont_limbs(c, single.challenges()[0]) == [want[x] for x in CH]
    single.discard()
    both.discard()
    assert mj.snark.verify_batch_proof([w.vks[0]], [pub], image, None, transcript="solidity") is True
    assert mj.snark.verify_batch_proof([w.vks[0]], [pub], image, None) is False


# ---- links -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("compress", [True, False])
@pytest.mark.parametrize("cid", [0, 1])
def test_link_challenges(gpu, mj, pyref, cid, compress):
    import pyref_linking as L
    c, pc = mj.params.CURVES[cid], pyref.CURVES[cid]
    rng = random.Random(70 + cid)
    K = 70
    G = pyref.g1_gen(pc)
    pool = [None] + [pyref.g1_mul(pc, rng.randrange(1, pc.r), G) for _ in range(12)]     # (infinity among them: two proofs of one circuit link with Q = O)
    key = mj.keys.OpenKey(c, *mj.kzg.open_key_for_testing(c, rng.randrange(1, c.r), compress=compress), compressed=compress)
    enc = (lambda p: FS.g1_bytes(pc, p)) if compress else (lambda p: _g1_uncompressed(pc, p))
    links, want, merlin = [], [], []
    for i in range(K):
        a1, a2, q, o = (pool[rng.randrange(1, 13)], pool[rng.randrange(1, 13)], pool[rng.randrange(13)], pool[rng.randrange(13)])
        links.append((enc(a1), enc(a2), enc(q) + enc(o), mj.linking.GroupLayout(3, i % 4, 2)))
        want.append(L.quotient_challenge(SolidityPlonkTranscript(pc, b"PlonkLinkingProof"), a1, a2, q))
        merlin.append(L.quotient_challenge(FS.StandardTranscript(pc, b"PlonkLinkingProof"), a1, a2, q))
    b = key.begin_links(links, transcript="solidity")
    eta, _ = b.link_values()
    assert fr_from_mont_limbs(c, eta) == want and fr_from_mont_limbs(c, b.u) == want
    assert fr_from_mont_limbs(c, b.scalars()[1][K - 1])[3] == want[K - 1]
    b.discard()
    b = key.begin_links(links)
    assert fr_from_mont_limbs(c, b.u) == merlin and merlin != want
    b.discard()
    key.release()


# ---- accept and reject -------------------------------------------------------------------------------------------------------------------
def _flip_eval(proof, W, g1):
    bad = bytearray(proof)
    bad[(8 + W * g1) + g1 + (8 + W * g1) + 2 * g1 + 8] ^= 1            # wires_evals[0]
    return bytes(bad)


@pytest.mark.parametrize("cid", [0, 1])
def test_solidity_proofs_are_accepted_and_merlin_proofs_are_not(world, mj, pyref, cid):
    """the bench case of each curve (BLS12-381: UltraPlonk, BN254: TurboPlonk): one proof under each transcript from the same prover"""
    import pyref_verifier as V
    w = world[cid]
    case, c, pc = w["cases"][1], mj.params.CURVES[cid], pyref.CURVES[cid]
    plonk_type, gates, range_bits = SETUPS[cid][1]
    cs = mj.snark.gen_circuit_for_bench(c, gates, plonk_type, range_bit_len=range_bits)
    extra = b"bound to this message"
    _, proof = mj.snark.prove(mj.rng.test_rng(), cs, case.prover, extra, transcript="solidity")
    assert V.verify(pc, SolidityPlonkTranscript(pc), case.ovk, [], proof, None, None, extra_msg=extra, open_key=w["oracle_open_key"])
    assert mj.snark.verify(case.vk, [], proof, extra, transcript="solidity") is True
    assert mj.snark.verify(case.vk, [], proof, extra) is False
    assert mj.snark.verify(case.vk, [], proof, None, transcript="solidity") is False
    merlin = case.proofs[3]
    assert mj.snark.verify(case.vk, [], merlin, EXTRAS[3]) is True
    assert mj.snark.verify(case.vk, [], merlin, EXTRAS[3], transcript="solidity") is False
    W, g1 = len(case.pr[0]["wires_poly_comms"]), 48 if cid == 0 else 32
    assert mj.snark.verify(case.vk, [], _flip_eval(proof, W, g1), extra, transcript="solidity") is False
    # a malformed proof in a Solidity batch: the lowest bad proof and its field
    evals_off = (8 + W * g1) + g1 + (8 + W * g1) + 2 * g1 + 8
    eval_r = bytearray(proof)
    eval_r[evals_off + 32:evals_off + 64] = c.r.to_bytes(32, "little")
    with pytest.raises(mj.keys.ProofEncodingError) as e:
        mj.snark.batch_verify([case.vk] * 4, [[]] * 4, [proof, proof, bytes(eval_r), bytes(eval_r)], [extra] * 4, transcript="solidity")
    assert (e.value.index, e.value.field) == (2, "wires_evals[1]") and "not below the modulus" in e.value.reason
    with pytest.raises(ValueError):
        mj.snark.verify(case.vk, [], proof, extra, transcript="rescue")


def _prove_linked(mj, pc, c, log_n, layout, shared, rng, ck, n_proofs=1):
    """TurboPlonk proofs under the Solidity transcript of a circuit whose proof-linking gates hold `shared` on the layout's rows:
    (prover, public input, [proof bytes], [LinkingHint])"""
    n = 1 << log_n
    start, _ = layout.range_in_nth_roots(log_n)
    spacing = 1 << (log_n - layout.alignment)
    sel, sig, k, w, pi = build_circuit(pc, log_n, rng, reserved={start + i * spacing: v for i, v in enumerate(shared)})
    dom = mj.Radix2EvaluationDomain(c, log_n)
    prover = mj.prover.TurboPlonkProver(c, n, [dom.ifft(fr_mont_limbs(c, s)) for s in sel], [dom.ifft(fr_mont_limbs(c, s)) for s in sig], k, ck)
    brng = mj.rng.ChaChaRng(bytes([log_n]) * 32, 12)
    proofs, hints = [], []
    for _ in range(n_proofs):
        blind = mj.snark.draw_blinders(c, brng, 5, False)
        core = prover.prove(np.stack([fr_mont_limbs(c, col) for col in w]), pi[:4], mj.prover.TranscriptChallenges(prover, pi[:4], None, "solidity"), blind)
        proofs.append(mj.snark.serialize_proof(c, core))
        hints.append(mj.linking.LinkingHint(prover.poly_dev(mj.linking.PROOF_LINK_WIRE_IDX), core.wires_poly_comms[mj.linking.PROOF_LINK_WIRE_IDX]))
    return prover, pi[:4], proofs, hints


def test_a_bundle_under_two_keys_with_a_link(gpu, mj, pyref):
    """ONE batch_verify: three proofs under two keys, the link between two of them, transcript="solidity"; its r is the oracle's and not the
    Merlin function's"""
    import pyref_verifier as V
    cid = 1
    c, pc = mj.params.CURVES[cid], pyref.CURVES[cid]
    L = mj.load()
    layout = mj.linking.GroupLayout(5, 4, 6)
    rng = random.Random(99)
    shared = [rng.randrange(c.r) for _ in range(layout.size)]
    srs_beta = rng.randrange(1, c.r)
    ck = mj.UnivariateProverParam.gen_srs_for_testing(c, srs_beta, (1 << 6) + 2)
    g, h, beta_h = mj.kzg.open_key_for_testing(c, srs_beta)
    pa, pub_a, proofs_a, hints_a = _prove_linked(mj, pc, c, 5, layout, shared, random.Random(505), ck, n_proofs=2)
    pb, pub_b, proofs_b, hints_b = _prove_linked(mj, pc, c, 6, layout, shared, random.Random(506), ck)
    vka, vkb = (mj.keys.VerifyingKey.deserialize(cid, p.serialize_vk(4, h, beta_h)) for p in (pa, pb))
    link = mj.linking.link_proofs(hints_a[1], hints_b[0], layout, ck, transcript="solidity").serialize_compressed()
    assert link != mj.linking.link_proofs(hints_a[1], hints_b[0], layout, ck).serialize_compressed()
    vks, pubs, proofs, none = [vka, vkb, vka], [pub_a, pub_b, pub_a], [proofs_a[0], proofs_b[0], proofs_a[1]], [None] * 3
    links = [(2, 1, link, layout)]
    assert mj.snark.batch_verify(vks, pubs, proofs, none, links=links, transcript="solidity") is True
    assert mj.snark.batch_verify(vks, pubs, proofs, none, links=links) is False
    assert mj.snark.batch_verify(vks, pubs, proofs, none, links=[(0, 1, link, layout)], transcript="solidity") is False
    assert mj.linking.verify_link_proof(proofs[2], proofs[1], link, layout, vka, transcript="solidity") is True
    assert mj.linking.verify_link_proof(proofs[2], proofs[1], link, layout, vka) is False
    # r: the groups by hand, as batch_verify runs them
    ovks = {id(vka): verifying_key(mj, pc, pa, 4), id(vkb): verifying_key(mj, pc, pb, 4)}
    want_u = [V.compute_challenges(SolidityPlonkTranscript(pc), ovks[id(vk)], pub, V.deserialize_proof(pc, pr), None)["u"] for vk, pub, pr in zip(vks, pubs, proofs)]
    want_r = oracle_batch_challenge(pc, want_u)

    def decide(r_flags):
        ba = vka.verifier().begin([proofs[0], proofs[2]], [pub_a] * 2, transcript="solidity")
        bb = vkb.verifier().begin([proofs[1]], [pub_b], transcript="solidity")
        wire = lambda i: mj.linking.linking_wire_record(c, proofs[i], True)
        bl = vka.verifier().begin_links([(wire(2), wire(1), link, layout)], transcript="solidity")
        u = np.stack([ba.u[0], bb.u[0], ba.u[1]])
        assert fr_from_mont_limbs(c, u) == want_u
        r = np.zeros(4, dtype=np.uint64)
        assert L.mzk_batch_verify_challenge_t(cid, r_flags, C.c_void_p(u.ctypes.data), 3, C.c_void_p(r.ctypes.data)) == 0
        r_int = fr_from_mont_limbs(c, r.reshape(1, 4))[0]
        wts = fr_mont_limbs(c, [pow(r_int, i, c.r) for i in range(3)])
        res = [ba.finish(wts[[0, 2]]), bb.finish(wts[[1]]), bl.finish(bl.link_weights(r))]
        return r_int, vka.verifier().check(np.stack([a for a, _ in res]), np.stack([b for _, b in res]))

    assert decide(SOLIDITY) == (want_r, True)
    # r from the Merlin function is another value.  The groups are still accepted under it: each of them satisfies its own pairing equation, and
    # a sum of true equations holds under ANY weights -- a wrong r cannot reject valid proofs, it only stops binding the weights to them
    r_merlin, ok = decide(0)
    assert r_merlin != want_r and ok is True
    for vk in (vka, vkb):
        vk.release_verifier()
    for p in (pa, pb):
        p.release()
    ck.release()
