"""GPU: verification of aggregated BatchProofs (mzk_verifier_aggregate_*: csrc/verifier.cuh; keys.AggregateVerifier, snark.verify_batch_proof /
batch_verify_batch_proofs) against the restated reference verifier (oracle/pyref_verifier.py: compute_challenges_batch,
prepare_pcs_info_batch, verify_batch_proof) on proofs the device prover made.  Per curve one TurboPlonk (n = 16) and one UltraPlonk (n = 32)
world of five general circuits with every selector live and four public inputs each, distinct per instance; BatchProofs of m = 1, 2, 3, 5
instances with and without an extra transcript message are made once per world and the oracle's values are computed once per proof; larger
batches repeat them.  Stage B and stage C + fold are compared value for value, m = 1 word for word with the single-proof path, A and B with
the oracle's MSMs, the decisions with the oracle's (its trapdoor form: the test SRS has a known beta)."""
import ctypes as C
import random
import struct

import numpy as np
import pytest

from conftest import build_circuit, build_ultra_circuit, fr_mont_limbs, fr_from_mont_limbs, jacobian_to_affine_ints, verifying_key
import general_cases as GC
import pyref_fs as FS

pytestmark = pytest.mark.gpu

M_MAX = 5
MS = (1, 2, 3, 5)
EXTRAS = [None, b"an extra transcript message"]
CH = ("tau", "beta", "gamma", "alpha", "zeta", "v", "u")
WORLDS = [(0, False), (0, True), (1, False), (1, True)]              # (curve, ultra)
LOG_N = {False: 4, True: 5}
ERR_INVALID_ARG, ERR_BAD_HANDLE, ERR_UNSUPPORTED = -1, -4, -5


class World:
    """five provers of one domain size and type with their keys; BatchProofs bp[(m, e)] over the first m of them with extra message EXTRAS[e]"""


def _serialize_bp(pc, bp, compressed=True):
    """BatchProof::serialize_{compressed, uncompressed} from the oracle's parsed proof (records as include/mzk.h states them)"""
    import pyref_verifier as V
    n = 48 if pc.curve_id == 0 else 32

    def g1(pt):
        if compressed:
            return FS.g1_bytes(pc, pt)
        if pt is None:
            rec = bytearray(2 * n)
            rec[0 if pc.curve_id == 0 else -1] |= 0x40
            return bytes(rec)
        x, y = pt
        if pc.curve_id == 0:
            return x.to_bytes(n, "big") + y.to_bytes(n, "big")
        rec = bytearray(x.to_bytes(n, "little") + y.to_bytes(n, "little"))
        rec[-1] |= 0x80 if y > pc.q - y else 0
        return bytes(rec)
    fr = lambda v: v.to_bytes(32, "little")
    vec = lambda items, enc: struct.pack("<Q", len(items)) + b"".join(enc(x) for x in items)
    plookup = lambda pl: b"\x00" if pl is None else (b"\x01" + vec(pl["h_poly_comms"], g1) + g1(pl["prod_lookup_poly_comm"])
                                                     + b"".join(fr(pl["evals"][k]) for k in V.PLOOKUP_EVAL_FIELDS))
    evals = lambda ev: vec(ev["wires_evals"], fr) + vec(ev["wire_sigma_evals"], fr) + fr(ev["perm_next_eval"])
    return (vec(bp["wires_poly_comms_vec"], lambda comms: vec(comms, g1)) + vec(bp["prod_perm_poly_comms_vec"], g1) + vec(bp["poly_evals_vec"], evals)
            + vec(bp["plookup_proofs_vec"], plookup) + vec(bp["split_quot_poly_comms"], g1) + g1(bp["opening_proof"]) + g1(bp["shifted_opening_proof"]))


def _build_world(mj, pyref, cid, ultra):
    import pyref_verifier as V
    c, pc = mj.params.CURVES[cid], pyref.CURVES[cid]
    log_n = LOG_N[ultra]
    n, W = 1 << log_n, 6 if ultra else 5
    w = World()
    w.cid, w.ultra, w.c, w.pc, w.W = cid, ultra, c, pc, W
    w.beta = random.Random(4100 + cid).randrange(1, c.r)              # per curve: the two worlds of a curve share an open key
    w.open_key = mj.kzg.open_key_for_testing(c, w.beta)
    w.ck = mj.UnivariateProverParam.gen_srs_for_testing(c, w.beta, n + 2)
    dom = mj.Radix2EvaluationDomain(c, log_n)
    w.provers, w.wires, w.pubs, w.ovks, w.vks = [], [], [], [], []
    for j in range(M_MAX):
        rng = random.Random(GC.verifier_seed(cid, ultra, log_n) + 7919 * (j + 1))
        if ultra:
            sel, sig, k, wv, pi, tabs = build_ultra_circuit(pc, log_n, rng, gates="all")
            kw = {"plookup": {name: dom.ifft(fr_mont_limbs(c, tabs[key])) for name, key in
                              zip(mj.plonk.PLOOKUP_TABLE_POLYS, ("range", "key", "table_dom_sep", "q_dom_sep"))}}
        else:
            sel, sig, k, wv, pi = build_circuit(pc, log_n, rng, gates="all")
            kw = {}
        # the builders give every circuit the public input (0, 0, 0, -5): make the four values this instance's own.  A row's gate reads
        # .. + q_c + pi = 0, so pi += d, q_c -= d on rows 0..3 keeps the witness satisfying and touches neither wires nor permutation
        for i in range(4):
            d = rng.randrange(1, pc.r)
            pi[i], sel[11][i] = (pi[i] + d) % pc.r, (sel[11][i] - d) % pc.r
        p = mj.prover.TurboPlonkProver(c, n, [dom.ifft(fr_mont_limbs(c, s)) for s in sel], [dom.ifft(fr_mont_limbs(c, s)) for s in sig], k, w.ck, **kw)
        w.provers.append(p)
        w.wires.append(np.stack([fr_mont_limbs(c, col) for col in wv]))
        w.pubs.append(list(pi[:4]))
        w.ovks.append(verifying_key(mj, pc, p, 4))
        w.vks.append(mj.keys.VerifyingKey.deserialize(cid, p.serialize_vk(4, w.open_key[1], w.open_key[2])))
    assert len({tuple(p) for p in w.pubs}) == M_MAX
    brng = mj.rng.test_rng()
    w.bp, w.parsed, w.ch, w.info = {}, {}, {}, {}
    for m in MS:
        for e, extra in enumerate(EXTRAS):
            blinds, quot = mj.snark.draw_batch_blinders(c, brng, W, [ultra] * m)
            core = mj.batch.batch_prove(w.provers[:m], w.wires[:m], w.pubs[:m], blinds, quot, extra)
            blob = mj.batch.serialize_batch_proof(c, core)
            w.bp[m, e] = blob
            # the oracle, once per proof
            bp = w.parsed[m, e] = V.deserialize_batch_proof(pc, blob)
            w.ch[m, e] = V.compute_challenges_batch(FS.StandardTranscript(pc, b"PlonkProof"), w.ovks[:m], w.pubs[:m], bp, extra)
            w.info[m, e] = V.prepare_pcs_info_batch(pc, w.ovks[:m], w.pubs[:m], bp, w.ch[m, e])
    return w


@pytest.fixture(scope="module")
def worlds(gpu, mj, pyref):
    out = {key: _build_world(mj, pyref, *key) for key in WORLDS}
    yield out
    for w in out.values():
        for vk in w.vks:
            vk.release_verifier()
        for p in w.provers:
            p.release()
        w.ck.release()


def _oracle_accepts(w, pyref, vks, pubs, blob, extra):
    """PlonkKzgSnark::verify_batch_proof restated, the final check in its trapdoor form; a proof the oracle cannot parse is rejected"""
    import pyref_verifier as V
    try:
        return V.verify_batch_proof(w.pc, FS.StandardTranscript(w.pc, b"PlonkProof"), vks, pubs, blob, pyref.g1_gen(w.pc), w.beta, extra_msg=extra)
    except V.VerifyError:
        return False


def _cycle(K):
    """which extra message proof n of a batch of K has: mixed, as _batch_indices of tests/test_verify_gpu.py mixes them"""
    return [(0, 1, 1, 0, 1)[n % 5] for n in range(K)]


def _begin(mj, w, m, es, challenges=None, vks=None):
    agg = mj.keys.AggregateVerifier(w.vks[:m] if vks is None else vks)
    extras = [EXTRAS[e] for e in es]
    return agg.begin([w.bp[m, e] for e in es], [w.pubs[:m]] * len(es), extras if any(x is not None for x in extras) else None, challenges)


def _grouped(w, m, e):
    """the oracle's (scalar, base) list of one BatchProof summed by POSITION into the library's column order -> (key row, proof row).  The
    list is walked with the script prepare_pcs_info_batch wrote it by, so equal points at different positions (infinity selectors, a key
    at two positions) are never merged."""
    pc, W, ultra = w.pc, w.W, w.ultra
    r = pc.r
    bp, info, ovks = w.parsed[m, e], w.info[m, e], w.ovks[:m]
    nsel = 14 if ultra else 13
    nkey1 = nsel + W + (4 if ultra else 0)
    key_bases, own_bases = [], []
    for vk in ovks:
        key_bases += list(vk["selector_comms"]) + list(vk["sigma_comms"])
        if ultra:
            key_bases += [vk["plookup"][x] for x in ("range_table_comm", "key_table_comm", "table_dom_sep_comm", "q_dom_sep_comm")]
    for j in range(m):
        own_bases += list(bp["wires_poly_comms_vec"][j]) + [bp["prod_perm_poly_comms_vec"][j]]
    own_bases += list(bp["split_quot_poly_comms"]) + [bp["opening_proof"], bp["shifted_opening_proof"]]
    if ultra:
        for pl in bp["plookup_proofs_vec"]:
            own_bases += list(pl["h_poly_comms"]) + [pl["prod_lookup_poly_comm"]]
    key_row, own_row = [0] * (m * nkey1 + 1), [0] * len(own_bases)
    assert len(own_row) == m * (W + 1) + W + 2 + (3 * m if ultra else 0)
    sb = list(info["comm_scalars_and_bases"])
    pos = 0

    def take(row, col):
        nonlocal pos
        s, base = sb[pos]
        assert base == (key_bases if row is key_row else own_bases)[col], (pos, col)
        row[col] = (row[col] + s) % r
        pos += 1
    KEY = lambda j, k: j * nkey1 + k
    WIRE, PROD = (lambda j, k: j * (W + 1) + k), (lambda j: j * (W + 1) + W)
    QUOT = m * (W + 1)
    H = lambda j: m * (W + 1) + W + 2 + 3 * j
    for j in range(m):                                               # [D]_1 of every instance
        take(own_row, PROD(j))
        take(key_row, KEY(j, nsel + W - 1))
        for k in range(13):
            take(key_row, KEY(j, k))
        if ultra:
            take(own_row, H(j) + 2)
            take(own_row, H(j) + 1)
    for k in range(W):
        take(own_row, QUOT + k)
    for j in range(m):                                               # the openings at zeta and zeta w, instance by instance
        for k in range(W):
            take(own_row, WIRE(j, k))
        for k in range(W - 1):
            take(key_row, KEY(j, nsel + k))
        take(own_row, PROD(j))
        if ultra:
            P = nsel + W
            for row, col in ((key_row, KEY(j, P)), (key_row, KEY(j, P + 1)), (own_row, H(j)), (key_row, KEY(j, 13)), (key_row, KEY(j, P + 2)),
                             (key_row, KEY(j, P + 3)), (own_row, H(j) + 2), (key_row, KEY(j, P)), (key_row, KEY(j, P + 1)), (own_row, H(j)),
                             (own_row, H(j) + 1), (key_row, KEY(j, 13)), (own_row, WIRE(j, 3)), (own_row, WIRE(j, 4)), (key_row, KEY(j, P + 2))):
                take(row, col)
    assert pos == len(sb)
    own_row[QUOT + W] = info["eval_point"]
    own_row[QUOT + W + 1] = info["u"] * info["next_eval_point"] % r
    return key_row, own_row


def test_the_offsets_per_instance_are_the_oracles_walk(worlds):
    """c_v and c_u, the commitments one instance opens at zeta and at zeta w (the strides of the powers of v in stage C), counted from the
    oracle's list: 9 | 17 and 1 | 10"""
    for (cid, ultra), w in worlds.items():
        per = {m: len(w.info[m, 0]["comm_scalars_and_bases"]) for m in (1, 2)}
        d1 = 2 + 13 + (2 if ultra else 0)                            # the [D]_1 entries of one instance
        assert per[2] - per[1] - d1 == (17 + 10 if ultra else 9 + 1)
        assert 2 * w.W - 1 + (6 if ultra else 0) == (17 if ultra else 9)


# ---- 1 ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", WORLDS)
@pytest.mark.parametrize("K", [1, 3, 65])
def test_stage_b_is_compute_challenges_batch(worlds, mj, key, K):
    w = worlds[key]
    for m in MS:
        es = _cycle(K)
        b = _begin(mj, w, m, es)
        got = fr_from_mont_limbs(w.c, b.challenges().reshape(-1, 4))
        u = fr_from_mont_limbs(w.c, b.u)
        b.discard()
        for n, e in enumerate(es):
            assert got[7 * n:7 * n + 7] == [w.ch[m, e][x] for x in CH], (m, n)
            assert u[n] == w.ch[m, e]["u"]


# ---- 2 ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", WORLDS)
@pytest.mark.parametrize("K,ms", [(1, MS), (3, MS), (65, MS), (22, (3,))])
def test_stage_c_and_fold_are_prepare_pcs_info_batch(worlds, mj, key, K, ms):
    w = worlds[key]
    c = w.c
    for m in ms:
        es = _cycle(K)
        want = {e: _grouped(w, m, e) for e in set(es)}
        oracle_ch = np.stack([fr_mont_limbs(c, [w.ch[m, e][x] for x in CH]) for e in es])
        for challenges in (oracle_ch, None):                         # through the seam, then with stage B's own
            b = _begin(mj, w, m, es, challenges)
            kr, pr, ev = b.scalars()
            b.discard()
            assert kr.shape[1] == len(want[0][0]) and pr.shape[1] == len(want[0][1])
            for n, e in enumerate(es):
                key_row, own_row = want[e]
                assert fr_from_mont_limbs(c, kr[n]) == key_row, (m, n)
                assert fr_from_mont_limbs(c, pr[n]) == own_row, (m, n)
                assert fr_from_mont_limbs(c, ev[n:n + 1]) == [w.info[m, e]["eval"]], (m, n)


# ---- 3 ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", WORLDS)
def test_one_instance_is_the_single_proof_path(worlds, mj, key):
    import pyref_verifier as V
    w = worlds[key]
    c, pc, p, pub = w.c, w.pc, w.provers[0], w.pubs[0]
    brng = mj.rng.test_rng()
    proofs = []
    for extra in EXTRAS:
        blind = mj.snark.draw_blinders(c, brng, w.W, w.ultra)
        proofs.append(mj.snark.serialize_proof(c, p.prove(w.wires[0], pub, mj.prover.TranscriptChallenges(p, pub, extra), blind)))
    images = [_serialize_bp(pc, V.batch_proof_from(V.deserialize_proof(pc, pr))) for pr in proofs]
    assert len(images[0]) == len(proofs[0]) + 4 * 8 and images[0] != proofs[0]      # four outer Vec counts more
    single = w.vks[0].verifier().begin(proofs, [pub] * 2, EXTRAS)
    agg = mj.keys.AggregateVerifier([w.vks[0]])
    assert agg.shape == (single.verifier.n_proof_points, single.verifier.n_key_bases, len(images[0]), 4)
    both = agg.begin(images, [[pub]] * 2, EXTRAS)
    assert np.array_equal(single.challenges(), both.challenges()) and np.array_equal(single.u, both.u)
    for a, b in zip(single.scalars(), both.scalars()):
        assert np.array_equal(a, b)
    weights = fr_mont_limbs(c, [1, 0x1234567])
    A1, B1 = single.finish(weights)
    A2, B2 = both.finish(weights)
    assert np.array_equal(A1, A2) and np.array_equal(B1, B2)


# ---- 4 ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", WORLDS)
def test_a_and_b_are_the_oracles_msms(worlds, mj, pyref, key):
    import pyref_verifier as V
    w = worlds[key]
    c, pc, m = w.c, w.pc, 3
    r, g = pc.r, pyref.g1_gen(pc)
    part = {}
    for e in (0, 1):
        info = w.info[m, e]
        a = V._msm(pc, [(1, info["opening_proof"]), (info["u"], info["shifted_opening_proof"])])
        b = V._msm(pc, info["comm_scalars_and_bases"] + [(info["eval_point"], info["opening_proof"]),
                                                         (info["u"] * info["next_eval_point"] % r, info["shifted_opening_proof"])])
        part[e] = (a, b)
    for es, weights in (([0], [1]), ([1], [1]), ([0, 1, 1], None)):
        b = _begin(mj, w, m, es)
        if weights is None:
            rm = np.zeros(4, dtype=np.uint64)
            assert mj.load().mzk_batch_verify_challenge(w.cid, C.c_void_p(b.u.ctypes.data), len(es), C.c_void_p(rm.ctypes.data)) == 0
            rr = fr_from_mont_limbs(c, rm.reshape(1, 4))[0]
            assert rr != 1
            weights = [pow(rr, n, r) for n in range(len(es))]
        A, B = b.finish(fr_mont_limbs(c, weights))
        want_a = V._msm(pc, [(weights[n], part[e][0]) for n, e in enumerate(es)])
        sum_eval = sum(weights[n] * w.info[m, e]["eval"] for n, e in enumerate(es)) % r
        want_b = V._msm(pc, [(weights[n], part[e][1]) for n, e in enumerate(es)] + [(-sum_eval % r, g)])
        assert jacobian_to_affine_ints(pc, A) == want_a and jacobian_to_affine_ints(pc, B) == want_b, es


# ---- 5 ----------------------------------------------------------------------------------------------------------------------------------
def _flip(blob, off, bit=0):
    bad = bytearray(blob)
    bad[off] ^= 1 << bit
    return bytes(bad)


@pytest.mark.parametrize("key", WORLDS)
def test_decisions_are_the_oracles(worlds, mj, pyref, key):
    import pyref_verifier as V
    w = worlds[key]
    verify = mj.snark.verify_batch_proof
    for m in MS:
        for e, extra in enumerate(EXTRAS):
            assert verify(w.vks[:m], w.pubs[:m], w.bp[m, e], extra), (m, e)
    for m, e in ((1, 0), (3, 1)):
        assert _oracle_accepts(w, pyref, w.ovks[:m], w.pubs[:m], w.bp[m, e], EXTRAS[e])
    m, blob, extra = 3, w.bp[3, 1], EXTRAS[1]
    vks, ovks, pubs = w.vks[:m], w.ovks[:m], w.pubs[:m]
    L = mj.keys.batch_proof_layout(w.cid, w.ultra, m)
    swap = lambda x: [x[1], x[0], x[2]]
    cases = [(swap(vks), swap(ovks), pubs, blob, extra),                                     # the keys in another order
             (vks, ovks, swap(pubs), blob, extra),                                           # another instance's public inputs
             (vks, ovks, pubs, blob, None), (vks, ovks, pubs, blob, b"another message"),     # a missing / a different extra message
             (vks, ovks, pubs, _flip(blob, L.wires_evals_off[2] + 32 * 1), extra)]           # one bit of an evaluation
    for n, (vk_, ovk_, pub_, blob_, extra_) in enumerate(cases):
        assert not _oracle_accepts(w, pyref, ovk_, pub_, blob_, extra_), n
        assert not verify(vk_, pub_, blob_, extra_), n
    # one bit of a commitment's x (instance 1's third wire) such that the record still decodes: tried on the CPU until the oracle decodes it
    G = L.g1_record_bytes
    off = L.wires_off[1] + 2 * G
    for bit in range(8 * (G - 1)):
        pos = off + (G - 1 - bit // 8 if w.cid == 0 else bit // 8)    # low bits of x first (BLS12-381 is big-endian)
        bad = _flip(blob, pos, bit % 8)
        try:
            V.g1_decompress(w.pc, bad[off:off + G])
            break
        except V.VerifyError:
            continue
    assert not _oracle_accepts(w, pyref, ovks, pubs, bad, extra)
    if w.cid == 1:
        assert not verify(vks, pubs, bad, extra)                     # BN254's G1 is the whole curve: the point decodes under every check
    else:
        # BLS12-381: a point of the curve found this way is outside the subgroup (cofactor ~ 2^126), which the library's deserialisation checks
        # and the oracle's does not: with the check the image is refused naming the record, without it the proof is rejected as the oracle rejects it
        with pytest.raises(mj.keys.ProofEncodingError) as err:
            verify(vks, pubs, bad, extra)
        assert (err.value.index, err.value.instance, err.value.field) == (0, 1, "wires_poly_comms[2]") and "subgroup" in err.value.reason
        agg = mj.keys.AggregateVerifier(vks)
        A, B = agg.begin([bad], [pubs], [extra], validate=False).finish(fr_mont_limbs(w.c, [1]))
        assert not agg.check(A, B)


# ---- 6 ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid,plonk_type,gates,range_bits", [(0, "TurboPlonk", 30, 8), (1, "UltraPlonk", 25, 4)])
def test_a_key_at_several_positions(gpu, worlds, mj, pyref, cid, plonk_type, gates, range_bits):
    c = mj.params.CURVES[cid]
    cs = mj.snark.gen_circuit_for_bench(c, gates, plonk_type, range_bit_len=range_bits)
    beta = 0xF02C
    ck = mj.UnivariateProverParam.gen_srs_for_testing(c, beta, cs.n + 2)
    pk = mj.snark.preprocess(ck, cs)
    forks = [pk.fork(), pk.fork()]
    _, blob = mj.snark.batch_prove(mj.rng.test_rng(), [cs] * 3, [pk] + forks, b"forks")
    g, h, beta_h = mj.kzg.open_key_for_testing(c, beta)
    vk = mj.keys.VerifyingKey.deserialize(cid, pk.serialize_vk(0, h, beta_h))
    agg = mj.keys.AggregateVerifier([vk, vk, vk])
    assert len(set(agg.handles)) == 1                               # ONE verifier handle, three times
    assert mj.snark.verify_batch_proof([vk, vk, vk], [[], [], []], blob, b"forks")
    assert not mj.snark.verify_batch_proof([vk, vk, vk], [[], [], []], blob, None)
    vk.release_verifier()
    for p in forks + [pk]:
        p.release()
    ck.release()
    # the same handle twice in a tuple of DIFFERENT circuits: a wrong proof, not an error
    w = worlds[cid, plonk_type == "UltraPlonk"]
    assert not mj.snark.verify_batch_proof([w.vks[0], w.vks[0], w.vks[2]], w.pubs[:3], w.bp[3, 0], None)
    assert mj.snark.verify_batch_proof(w.vks[:3], w.pubs[:3], w.bp[3, 0], None)


# ---- 7 ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", WORLDS)
def test_groups_of_aggregates_and_single_proofs_in_one_check(worlds, mj, key):
    w = worlds[key]
    c, L = w.c, mj.load()
    p, pub = w.provers[0], w.pubs[0]
    brng = mj.rng.test_rng()
    singles = []
    for extra in EXTRAS:
        blind = mj.snark.draw_blinders(c, brng, w.W, w.ultra)
        singles.append(mj.snark.serialize_proof(c, p.prove(w.wires[0], pub, mj.prover.TranscriptChallenges(p, pub, extra), blind)))
    # a second tuple: the last two keys, a proof of their own
    blinds, quot = mj.snark.draw_batch_blinders(c, brng, w.W, [w.ultra] * 2)
    other = mj.batch.serialize_batch_proof(c, mj.batch.batch_prove(w.provers[3:], w.wires[3:], w.pubs[3:], blinds, quot, None))
    agg3, agg2 = mj.keys.AggregateVerifier(w.vks[:3]), mj.keys.AggregateVerifier(w.vks[3:])
    lay3, lay2 = mj.keys.batch_proof_layout(w.cid, w.ultra, 3), mj.keys.batch_proof_layout(w.cid, w.ultra, 2)
    g1 = lay3.g1_record_bytes
    single_eval = (8 + w.W * g1) + g1 + (8 + w.W * g1) + 2 * g1 + 8   # wires_evals[0] of a `Proof`

    def decide(flip=None):
        images = [[w.bp[3, 0], w.bp[3, 1]], [other], list(singles)]
        if flip is not None:
            grp, n, off = flip
            images[grp][n] = _flip(images[grp][n], off)
        batches = [agg3.begin(images[0], [w.pubs[:3]] * 2, EXTRAS), agg2.begin(images[1], [w.pubs[3:]]), w.vks[0].verifier().begin(images[2], [pub] * 2, EXTRAS)]
        u = np.concatenate([b.u for b in batches])
        r = np.zeros(4, dtype=np.uint64)
        assert L.mzk_batch_verify_challenge(w.cid, C.c_void_p(u.ctypes.data), u.shape[0], C.c_void_p(r.ctypes.data)) == 0
        r_int = fr_from_mont_limbs(c, r.reshape(1, 4))[0]
        weights = fr_mont_limbs(c, [pow(r_int, i, c.r) for i in range(u.shape[0])])
        results, at = [], 0
        for b in batches:
            results.append(b.finish(weights[at:at + b.K]))
            at += b.K
        return agg2.check(np.stack([a for a, _ in results]), np.stack([b for _, b in results]))
    assert decide()
    assert not decide((0, 1, lay3.wires_evals_off[2]))
    assert not decide((1, 0, lay2.perm_next_off[1]))
    assert not decide((2, 1, single_eval))


# ---- 8 ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", WORLDS)
def test_malformed_images_name_proof_instance_and_field(worlds, mj, pyref, key):
    import pyref_verifier as V
    w = worlds[key]
    c, pc, m = w.c, w.pc, 3
    good = w.bp[m, 0]
    L = mj.keys.batch_proof_layout(w.cid, w.ultra, m)
    G = L.g1_record_bytes
    agg = mj.keys.AggregateVerifier(w.vks[:m])
    E = mj.keys.ProofEncodingError

    def refused(images, index, instance, field, reason, pubs=None):
        seen = []
        for _ in range(2):                                           # the same answer on every run
            with pytest.raises(E) as e:
                agg.begin(images, [pubs or w.pubs[:m]] * len(images))
            assert (e.value.index, e.value.instance, e.value.field) == (index, instance, field) and reason in e.value.reason, e.value.reason
            assert e.value.reason.startswith(f"proof {index}: instance {instance}: {field}: ")
            seen.append(e.value.reason)
        assert seen[0] == seen[1]
    eval_r = bytearray(good)                                         # instance 2: wires_evals[1] = r
    eval_r[L.wires_evals_off[2] + 32:L.wires_evals_off[2] + 64] = c.r.to_bytes(32, "little")
    eval_r = bytes(eval_r)
    off = L.prod_perm_off[1]                                         # instance 1: prod_perm with an x off the curve (x^3 + b no square), found on the CPU
    for bit in range(8 * (G - 1)):
        off_curve = _flip(good, off + (G - 1 - bit // 8 if w.cid == 0 else bit // 8), bit % 8)
        try:
            V.g1_decompress(pc, off_curve[off:off + G])
        except V.VerifyError as err:
            assert "not on the curve" in str(err)
            break
    both = bytearray(off_curve)
    both[L.wires_evals_off[2] + 32:L.wires_evals_off[2] + 64] = c.r.to_bytes(32, "little")
    both = bytes(both)
    quot = bytearray(good)                                           # the whole proof's: split_quot_poly_comms[1].x = q
    rec = L.split_quot_off + G
    if w.cid == 0:
        quot[rec:rec + 48] = bytes([quot[rec] & 0xE0 | (c.q >> 376)]) + (c.q & ((1 << 376) - 1)).to_bytes(47, "big")
    else:
        quot[rec:rec + 32] = (c.q | (quot[rec + 31] & 0x80) << 248).to_bytes(32, "little")
    quot = bytes(quot)
    refused([good, eval_r], 1, 2, "wires_evals[1]", "not below the modulus")
    refused([off_curve], 0, 1, "prod_perm_poly_comm", "x^3 + b is not a square")
    refused([both], 0, 1, "prod_perm_poly_comm", "x^3 + b is not a square")             # the lower instance wins, whatever the field
    refused([good, quot, eval_r], 1, m, "split_quot_poly_comms[1]", "coordinate not below the field modulus")
    batch = [good] * 65
    batch[40], batch[7] = both, eval_r
    refused(batch, 7, 2, "wires_evals[1]", "not below the modulus")
    batch[7] = both
    refused(batch, 7, 1, "prod_perm_poly_comm", "x^3 + b is not a square")
    refused([good, good[:-1]], 1, m, "length", "expected")
    tag = _flip(good, L.plookup_tag_off[1])
    refused([good, good, tag], 2, 1, "plookup_proof", "key")
    # a public input >= r: its instance and index
    pubs = [list(p) for p in w.pubs[:m]]
    pubs[1][2] = c.r
    refused([good], 0, 1, "public_input[2]", "not below the modulus", pubs)
    # a commitment at infinity is flagged, not refused, and decides as the oracle does
    inf = bytearray(good)
    inf[L.wires_off[1] + G:L.wires_off[1] + 2 * G] = FS.g1_bytes(pc, None)
    inf = bytes(inf)
    agg.begin([inf], [w.pubs[:m]]).discard()
    want = _oracle_accepts(w, pyref, w.ovks[:m], w.pubs[:m], inf, None)
    assert mj.snark.verify_batch_proof(w.vks[:m], w.pubs[:m], inf, None) == want and not want


# ---- 9 ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", WORLDS)
def test_uncompressed_keys_and_images(worlds, mj, pyref, key):
    w = worlds[key]
    c, pc, m = w.c, w.pc, 3
    g, h, beta_h = mj.kzg.open_key_for_testing(c, w.beta, compress=False)
    vks = [mj.keys.VerifyingKey.deserialize(w.cid, p.serialize_vk(4, h, beta_h, compress=False), compress=False) for p in w.provers[:m]]
    images = [_serialize_bp(pc, w.parsed[m, e], compressed=False) for e in (0, 1)]
    assert _serialize_bp(pc, w.parsed[m, 0]) == w.bp[m, 0] and len(images[0]) > len(w.bp[m, 0])
    agg = mj.keys.AggregateVerifier(vks)
    assert agg.proof_len == len(images[0]) == mj.keys.batch_proof_layout(w.cid, w.ultra, m, compress=False).total_len
    b = agg.begin(images, [w.pubs[:m]] * 2, EXTRAS)
    got = fr_from_mont_limbs(c, b.challenges().reshape(-1, 4))
    kr, pr, ev = b.scalars()
    b.discard()
    for e in (0, 1):
        key_row, own_row = _grouped(w, m, e)
        assert got[7 * e:7 * e + 7] == [w.ch[m, e][x] for x in CH]
        assert fr_from_mont_limbs(c, kr[e]) == key_row and fr_from_mont_limbs(c, pr[e]) == own_row
        assert fr_from_mont_limbs(c, ev[e:e + 1]) == [w.info[m, e]["eval"]]
    assert mj.snark.batch_verify_batch_proofs(vks, [w.pubs[:m]] * 2, images, EXTRAS)
    assert mj.snark.verify_batch_proof(vks, w.pubs[:m], images[1], EXTRAS[1])
    L = mj.keys.batch_proof_layout(w.cid, w.ultra, m, compress=False)
    flipped = _flip(images[1], L.sigma_evals_off[1])
    assert not _oracle_accepts(w, pyref, w.ovks[:m], w.pubs[:m], _flip(w.bp[m, 1], mj.keys.batch_proof_layout(w.cid, w.ultra, m).sigma_evals_off[1]), EXTRAS[1])
    assert not mj.snark.batch_verify_batch_proofs(vks, [w.pubs[:m]] * 2, [images[0], flipped], EXTRAS)
    with pytest.raises(ValueError):                                  # a compressed key in an uncompressed tuple: another open key image
        mj.keys.AggregateVerifier([vks[0], w.vks[1]])
    for vk in vks:
        vk.release_verifier()


# ---- 10 ---------------------------------------------------------------------------------------------------------------------------------
def _raw_begin(mj, handles, image, pubs, out):
    img = np.frombuffer(image, dtype=np.uint8)
    pub = np.frombuffer(b"".join(int(x).to_bytes(32, "little") for p in pubs for x in p), dtype=np.uint64)
    hs = (C.c_uint64 * len(handles))(*handles)
    return mj.load().mzk_verifier_aggregate_begin(hs, len(handles), C.c_void_p(img.ctypes.data), len(image), 1, C.c_void_p(pub.ctypes.data), None, None, None, 2,
                                                  C.byref(out), None, None)


def test_handles_of_an_aggregate_batch(worlds, mj):
    w = worlds[0, False]
    L = mj.load()
    m = 3
    vs = [mj.keys.Verifier(vk) for vk in w.vks[:m]]                 # verifiers of this test's own
    out = C.c_uint64()
    assert _raw_begin(mj, [v.handle for v in vs], w.bp[m, 0], w.pubs[:m], out) == 0
    batch = out.value
    assert batch >> 48 == vs[0].handle >> 48
    for v in vs:                                                     # the open batch holds every verifier of its tuple
        assert L.mzk_verifier_destroy(v.handle) == ERR_INVALID_ARG and b"open batch" in L.mzk_last_error()
    assert L.mzk_verifier_batch_finish(batch, None, None, None) == 0  # discard
    assert L.mzk_verifier_batch_finish(batch, None, None, None) == ERR_BAD_HANDLE
    # a failed begin leaves no batch open
    lay = mj.keys.batch_proof_layout(0, False, m)
    eval_r = bytearray(w.bp[m, 0])
    eval_r[lay.perm_next_off[1]:lay.perm_next_off[1] + 32] = w.c.r.to_bytes(32, "little")
    out.value = 0
    assert _raw_begin(mj, [v.handle for v in vs], bytes(eval_r), w.pubs[:m], out) == -11 and out.value == 0
    assert L.mzk_last_error().startswith(b"proof 0: instance 1: perm_next_eval: ")
    for v in vs:
        assert L.mzk_verifier_destroy(v.handle) == 0                 # at once: nothing was left registered
    assert _raw_begin(mj, [v.handle for v in vs], w.bp[m, 0], w.pubs[:m], out) == ERR_BAD_HANDLE


def test_tuples_that_are_refused(gpu, worlds, mj):
    L = mj.load()
    turbo, ultra, other_curve = worlds[0, False], worlds[0, True], worlds[1, False]
    hs = lambda *vks: (C.c_uint64 * len(vks))(*[vk.verifier().handle for vk in vks])
    shape = lambda h, m: L.mzk_verifier_aggregate_shape(h, m, None, None, None, None)
    out = C.c_uint64()
    assert shape(hs(turbo.vks[0], turbo.vks[1]), 2) == 0
    # the two worlds of a curve differ in type AND domain size; the domain is looked at first
    assert turbo.vks[0].domain_size != ultra.vks[0].domain_size
    assert shape(hs(turbo.vks[0], ultra.vks[0]), 2) == ERR_INVALID_ARG and b"the domain size of the 1-th verification key is different" in L.mzk_last_error()
    assert _raw_begin(mj, list(hs(turbo.vks[0], ultra.vks[0])), turbo.bp[2, 0], turbo.pubs[:2], out) == ERR_INVALID_ARG
    with pytest.raises(ValueError, match="the domain size of the 1-th verification key is different"):
        mj.keys.AggregateVerifier([turbo.vks[0], ultra.vks[0]])
    # a mixed-type tuple of one domain size: unsupported
    c = turbo.c
    cs = mj.snark.gen_circuit_for_bench(c, 30, "TurboPlonk")          # a TurboPlonk key of the UltraPlonk world's domain size
    assert cs.n == ultra.vks[0].domain_size
    ck = mj.UnivariateProverParam.gen_srs_for_testing(c, turbo.beta, cs.n + 2)
    pk = mj.snark.preprocess(ck, cs)
    vk = mj.keys.VerifyingKey.deserialize(0, pk.serialize_vk(4, turbo.open_key[1], turbo.open_key[2]))
    assert shape(hs(vk, ultra.vks[0]), 2) == ERR_UNSUPPORTED and b"TurboPlonk and UltraPlonk" in L.mzk_last_error()
    with pytest.raises(gpu.MzkError) as e:
        mj.keys.AggregateVerifier([ultra.vks[0], vk])
    assert e.value.code == ERR_UNSUPPORTED
    vk.release_verifier()
    pk.release()
    ck.release()
    # another curve, another open key, no key, too many
    assert shape(hs(turbo.vks[0], other_curve.vks[0]), 2) == ERR_INVALID_ARG
    g, h, beta_h = mj.kzg.open_key_for_testing(c, turbo.beta + 1)
    vk2 = mj.keys.VerifyingKey.deserialize(0, turbo.provers[1].serialize_vk(4, h, beta_h))
    assert shape(hs(turbo.vks[0], vk2), 2) == ERR_INVALID_ARG and b"different open keys" in L.mzk_last_error()
    with pytest.raises(ValueError, match="different open keys"):
        mj.keys.AggregateVerifier([turbo.vks[0], vk2])
    vk2.release_verifier()
    one = hs(turbo.vks[0])
    assert shape(one, 0) == ERR_INVALID_ARG and shape(None, 1) == ERR_INVALID_ARG
    many = (C.c_uint64 * 65)(*[one[0]] * 65)
    assert shape(many, 65) == ERR_UNSUPPORTED and shape(many, 64) == 0
    assert shape((C.c_uint64 * 2)(one[0], one[0] + 1000), 2) == ERR_BAD_HANDLE
    with pytest.raises(ValueError):
        mj.keys.AggregateVerifier([])
    with pytest.raises(ValueError):
        mj.snark.verify_batch_proof(turbo.vks[:2], turbo.pubs[:3], turbo.bp[2, 0])
    with pytest.raises(ValueError, match="the circuit public input length != the 1-th verification key public input length"):
        mj.snark.verify_batch_proof(turbo.vks[:2], [turbo.pubs[0], turbo.pubs[1][:3]], turbo.bp[2, 0])


def test_shutdown_with_an_aggregate_batch_open(worlds, mj, tmp_path):
    """in a child process: mzk_shutdown with an aggregate batch open leaves the batch's and the verifiers' handles unknown"""
    import json
    import os
    import subprocess
    w = worlds[0, False]
    m = 2
    for j in range(m):
        (tmp_path / f"key{j}.bin").write_bytes(w.vks[j].serialize())
    (tmp_path / "proof.bin").write_bytes(w.bp[m, 0])
    (tmp_path / "pub.json").write_text(json.dumps([[int(x) for x in p] for p in w.pubs[:m]]))
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = r'''
import json, os, sys
sys.path.insert(0, %r)
d = %r
import mpc_jellyfish_amd as mj
from importlib import import_module
lib = import_module("mpc-jellyfish_amd.lib")
L = lib.init(0)
vks = [mj.keys.VerifyingKey.deserialize(0, open(os.path.join(d, "key%%d.bin" %% j), "rb").read()) for j in range(2)]
pubs = json.load(open(os.path.join(d, "pub.json")))
proof = open(os.path.join(d, "proof.bin"), "rb").read()
assert mj.snark.verify_batch_proof(vks, pubs, proof)
agg = mj.keys.AggregateVerifier(vks)
b = agg.begin([proof], [pubs])
assert b.challenges().any()
lib.check(L.mzk_shutdown(), "shutdown")
lib.check(L.mzk_init(0), "init again")
assert L.mzk_verifier_batch_challenges(b.handle, None) == -4
assert L.mzk_verifier_batch_finish(b.handle, None, None, None) == -4
assert L.mzk_verifier_aggregate_shape(agg.handles, 2, None, None, None, None) == -4
print("ok")
''' % (root, str(tmp_path))
    out = subprocess.run([os.sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stderr[-3000:]
