"""GPU: the library's verifier (mzk_verifier_*: csrc/verifier.cuh; snark.verify / batch_verify) against the restated reference verifier
(oracle/pyref_verifier.py) on proofs made by the device prover -- the circuits of tests/test_verifier_gpu.py: build_circuit /
build_ultra_circuit at log_n 4 / 5 with four public inputs and every selector live, and the bench circuits of 100 (TurboPlonk) and 40
(UltraPlonk) gates whose keys hold commitments at infinity.  Per curve one TurboPlonk and one UltraPlonk key share an open key, so a batch
spans two keys.  Stage B (Fiat-Shamir) and stage C (scalars) are compared bit for bit, A and B with the oracle's MSM, the decisions with
V.verify; malformed proofs must be refused with their field named and the lowest index.  Five proofs per circuit are made once (three
without an extra transcript message, two with messages of different lengths) and the oracle's results are computed once per proof; larger
batches repeat them."""
import random

import numpy as np
import pytest

from conftest import build_circuit, build_ultra_circuit, fr_mont_limbs, fr_from_mont_limbs, jacobian_to_affine_ints, verifying_key
import general_cases as GC
import pyref_fs as FS

pytestmark = pytest.mark.gpu

EXTRAS = [None, None, None, b"extra message", b"a longer extra transcript message, of forty-nine b"]
CH = ("tau", "beta", "gamma", "alpha", "zeta", "v", "u")
# (curve, general circuit: ultra, log_n; bench circuit: type, gates)
SETUPS = {0: ((False, 4), ("UltraPlonk", 40, 4)), 1: ((True, 5), ("TurboPlonk", 100, 8))}


class Case:
    """one key: the prover, the library's and the oracle's verifying key, five proofs with their public inputs and extra messages"""


def _general(mj, pc, c, ultra, log_n, srs_beta, open_key):
    n = 1 << log_n
    rng = random.Random(GC.verifier_seed(c.curve_id, ultra, log_n))
    W = 6 if ultra else 5
    if ultra:
        sel, sig, k, w, pi, tabs = build_ultra_circuit(pc, log_n, rng, gates="all")
    else:
        sel, sig, k, w, pi = build_circuit(pc, log_n, rng, gates="all")
    dom = mj.Radix2EvaluationDomain(c, log_n)
    ck = mj.UnivariateProverParam.gen_srs_for_testing(c, srs_beta, n + 2)
    kw = {"plookup": {name: dom.ifft(fr_mont_limbs(c, tabs[key])) for name, key in
                      zip(mj.plonk.PLOOKUP_TABLE_POLYS, ("range", "key", "table_dom_sep", "q_dom_sep"))}} if ultra else {}
    prover = mj.prover.TurboPlonkProver(c, n, [dom.ifft(fr_mont_limbs(c, s)) for s in sel], [dom.ifft(fr_mont_limbs(c, s)) for s in sig], k, ck, **kw)
    pub = pi[:4]
    brng = mj.rng.test_rng()
    proofs = []
    for extra in EXTRAS:
        blind = mj.snark.draw_blinders(c, brng, W, ultra)
        src = mj.prover.TranscriptChallenges(prover, pub, extra)
        proofs.append(mj.snark.serialize_proof(c, prover.prove(np.stack([fr_mont_limbs(c, col) for col in w]), fr_mont_limbs(c, pi), src, blind)))
    return _case(mj, pc, prover, pub, proofs, open_key, [ck])


def _bench(mj, pc, c, plonk_type, gates, range_bits, srs_beta, open_key):
    cs = mj.snark.gen_circuit_for_bench(c, gates, plonk_type, range_bit_len=range_bits)
    ck = mj.UnivariateProverParam.gen_srs_for_testing(c, srs_beta, cs.n + 2)
    pk = mj.snark.preprocess(ck, cs)
    rng = mj.rng.test_rng()
    proofs = [mj.snark.prove(rng, cs, pk, extra_transcript_init_msg=extra)[1] for extra in EXTRAS]
    return _case(mj, pc, pk, [], proofs, open_key, [ck])


def _case(mj, pc, prover, pub, proofs, open_key, owned):
    import pyref_verifier as V
    case = Case()
    case.prover, case.pub, case.proofs, case.owned = prover, list(pub), proofs, owned
    case.ovk = verifying_key(mj, pc, prover, len(pub))
    case.vk = mj.keys.VerifyingKey.deserialize(pc.curve_id, prover.serialize_vk(len(pub), open_key[1], open_key[2]))
    assert case.vk.g == open_key[0]
    # the oracle, once per proof
    case.pr = [V.deserialize_proof(pc, p) for p in proofs]
    case.ch = [V.compute_challenges(FS.StandardTranscript(pc, b"PlonkProof"), case.ovk, case.pub, pr, e) for pr, e in zip(case.pr, EXTRAS)]
    case.info = [V.prepare_pcs_info(pc, case.ovk, case.pub, pr, ch) for pr, ch in zip(case.pr, case.ch)]
    return case


@pytest.fixture(scope="module")
def world(gpu, mj, pyref):
    """per curve: srs_beta, the open key as records and for the oracle, and the two cases"""
    import pyref_verifier as V
    out = {}
    for cid, (gen, bench) in SETUPS.items():
        c, pc = mj.params.CURVES[cid], pyref.CURVES[cid]
        srs_beta = random.Random(77 + cid).randrange(1, c.r)
        open_key = mj.kzg.open_key_for_testing(c, srs_beta)
        out[cid] = dict(beta=srs_beta, open_key=open_key, oracle_open_key=V.open_key_for_testing(pc, srs_beta),
                        cases=[_general(mj, pc, c, *gen, srs_beta, open_key), _bench(mj, pc, c, *bench, srs_beta, open_key)])
    yield out
    for w in out.values():
        for case in w["cases"]:
            case.vk.release_verifier()
            case.prover.release()
            for k in case.owned:
                k.release()


ALL = [(cid, j) for cid in (0, 1) for j in (0, 1)]


def _batch_indices(K, kind):
    pool = {"plain": [0, 1, 2], "extra": [3, 4], "mixed": [0, 3, 1, 4, 2]}[kind]
    return [pool[i % len(pool)] for i in range(K)]


def _begin(case, idx, challenges=None):
    extras = [EXTRAS[i] for i in idx]
    return case.vk.verifier().begin([case.proofs[i] for i in idx], [case.pub] * len(idx), extras if any(e is not None for e in extras) else None, challenges)


def _grouped(pc, case, i):
    """the oracle's (scalar, base) list of proof i summed by base, in the library's column order: (key row, proof row)"""
    pr, info, ovk = case.pr[i], case.info[i], case.ovk
    r = pc.r
    pl = pr["plookup"]
    key_bases = list(ovk["selector_comms"]) + list(ovk["sigma_comms"])
    if ovk["plookup"] is not None:
        key_bases += [ovk["plookup"][n] for n in ("range_table_comm", "key_table_comm", "table_dom_sep_comm", "q_dom_sep_comm")]
    own_bases = list(pr["wires_poly_comms"]) + [pr["prod_perm_poly_comm"]] + list(pr["split_quot_poly_comms"])
    own_tail = [] if pl is None else list(pl["h_poly_comms"]) + [pl["prod_lookup_poly_comm"]]
    W = len(pr["wires_poly_comms"])
    key_row, own_row = [0] * (len(key_bases) + 1), [0] * (2 * W + 3 + len(own_tail))
    # a base is found by POSITION in the oracle's list, whose order is fixed (pyref_verifier.prepare_pcs_info_batch): equal points at
    # different positions (infinity selectors) must not be merged, so the list is walked with the same script the oracle wrote it by
    sb = list(info["comm_scalars_and_bases"])
    ultra = pl is not None
    pos = 0

    def take(row, col):
        nonlocal pos
        s, base = sb[pos]
        expect = (key_bases if row is key_row else (own_bases + [None, None] + own_tail))[col]
        assert base == expect, (pos, col)
        row[col] = (row[col] + s) % r
        pos += 1
    nsel = len(ovk["selector_comms"])
    take(own_row, W)                                                   # prod_perm
    take(key_row, nsel + W - 1)                                        # last sigma
    for j in range(13):
        take(key_row, j)
    if ultra:
        take(own_row, 2 * W + 5)
        take(own_row, 2 * W + 4)
    for j in range(W):
        take(own_row, W + 1 + j)
    for j in range(W):
        take(own_row, j)
    for j in range(W - 1):
        take(key_row, nsel + j)
    take(own_row, W)
    if ultra:
        P = nsel + W
        for row, col in ((key_row, P), (key_row, P + 1), (own_row, 2 * W + 3), (key_row, 13), (key_row, P + 2), (key_row, P + 3),
                         (own_row, 2 * W + 5), (key_row, P), (key_row, P + 1), (own_row, 2 * W + 3), (own_row, 2 * W + 4), (key_row, 13),
                         (own_row, 3), (own_row, 4), (key_row, P + 2)):
            take(row, col)
    assert pos == len(sb)
    own_row[2 * W + 1] = info["eval_point"]
    own_row[2 * W + 2] = info["u"] * info["next_eval_point"] % r
    return key_row, own_row


@pytest.mark.parametrize("cid,j", ALL)
@pytest.mark.parametrize("K", [1, 3, 65])
def test_stage_b_is_compute_challenges(world, mj, pyref, cid, j, K):
    case, c = world[cid]["cases"][j], mj.params.CURVES[cid]
    for kind in ("plain", "extra", "mixed"):
        idx = _batch_indices(K, kind)
        b = _begin(case, idx)
        got = fr_from_mont_limbs(c, b.challenges().reshape(-1, 4))
        u = fr_from_mont_limbs(c, b.u)
        b.discard()
        for n, i in enumerate(idx):
            assert got[7 * n:7 * n + 7] == [case.ch[i][x] for x in CH], (kind, n)
            assert u[n] == case.ch[i]["u"]


@pytest.mark.parametrize("cid,j", ALL)
@pytest.mark.parametrize("K", [1, 3, 65])
def test_stage_c_is_prepare_pcs_info(world, mj, pyref, cid, j, K):
    case, c, pc = world[cid]["cases"][j], mj.params.CURVES[cid], pyref.CURVES[cid]
    idx = _batch_indices(K, "mixed")
    want = {i: _grouped(pc, case, i) for i in set(idx)}
    oracle_ch = np.stack([fr_mont_limbs(c, [case.ch[i][x] for x in CH]) for i in idx])
    for challenges in (oracle_ch, None):                              # through the seam, then with the stage's own
        b = _begin(case, idx, challenges)
        kr, pr, ev = b.scalars()
        b.discard()
        for n, i in enumerate(idx):
            key_row, own_row = want[i]
            assert fr_from_mont_limbs(c, kr[n]) == key_row, n
            assert fr_from_mont_limbs(c, pr[n]) == own_row, n
            assert fr_from_mont_limbs(c, ev[n:n + 1]) == [case.info[i]["eval"]], n


@pytest.mark.parametrize("cid,j", ALL)
def test_a_and_b_are_the_oracles_msms(world, mj, pyref, cid, j):
    import ctypes as C
    import pyref_verifier as V
    case, c, pc = world[cid]["cases"][j], mj.params.CURVES[cid], pyref.CURVES[cid]
    r, g = pc.r, pyref.g1_gen(pc)
    lib = mj.load()
    # per proof, once: A_i = W_i + u_i W'_i and B_i without the evaluation term
    part = {}
    for i in (0, 3, 1):
        info = case.info[i]
        a = V._msm(pc, [(1, info["opening_proof"]), (info["u"], info["shifted_opening_proof"])])
        b = V._msm(pc, info["comm_scalars_and_bases"] + [(info["eval_point"], info["opening_proof"]),
                                                         (info["u"] * info["next_eval_point"] % r, info["shifted_opening_proof"])])
        part[i] = (a, b)
    for K in (1, 2, 3):
        idx = [0, 3, 1][:K]
        b = _begin(case, idx)
        rm = np.zeros(4, dtype=np.uint64)
        assert lib.mzk_batch_verify_challenge(cid, C.c_void_p(b.u.ctypes.data), K, C.c_void_p(rm.ctypes.data)) == 0
        rr = fr_from_mont_limbs(c, rm.reshape(1, 4))[0]
        assert (rr == 1) == (K == 1)
        w = [pow(rr, n, r) for n in range(K)]
        A, B = b.finish(fr_mont_limbs(c, w))
        want_a = V._msm(pc, [(w[n], part[i][0]) for n, i in enumerate(idx)])
        sum_eval = sum(w[n] * case.info[i]["eval"] for n, i in enumerate(idx)) % r
        want_b = V._msm(pc, [(w[n], part[i][1]) for n, i in enumerate(idx)] + [(-sum_eval % r, g)])
        assert jacobian_to_affine_ints(pc, A) == want_a and jacobian_to_affine_ints(pc, B) == want_b, K


def _flip_eval(proof, case, which=0):
    W = len(case.pr[0]["wires_poly_comms"])
    g1 = 48 if case.vk.curve.curve_id == 0 else 32
    off = (8 + W * g1) + g1 + (8 + W * g1) + 2 * g1 + 8 + 32 * which
    bad = bytearray(proof)
    bad[off] ^= 1
    return bytes(bad)


@pytest.mark.parametrize("cid,j", ALL)
def test_verify_decides_as_the_oracle(world, mj, pyref, cid, j):
    import pyref_verifier as V
    w = world[cid]
    case, c, pc = w["cases"][j], mj.params.CURVES[cid], pyref.CURVES[cid]
    fresh = lambda: FS.StandardTranscript(pc, b"PlonkProof")
    for i in (0, 3):
        assert V.verify(pc, fresh(), case.ovk, case.pub, case.proofs[i], None, None, extra_msg=EXTRAS[i], open_key=w["oracle_open_key"])
        assert mj.snark.verify(case.vk, case.pub, case.proofs[i], EXTRAS[i])
    proof = case.proofs[3]
    assert not mj.snark.verify(case.vk, case.pub, proof, b"another message")
    assert not mj.snark.verify(case.vk, case.pub, proof, None)
    assert not mj.snark.verify(case.vk, case.pub, _flip_eval(proof, case), EXTRAS[3])
    K = mj.keys.VerifyingKey
    other = lambda **kw: K(c, case.vk.domain_size, case.vk.num_inputs, kw.get("sigma", case.vk.sigma_comms), case.vk.selector_comms, case.vk.k, case.vk.g,
                           case.vk.h, kw.get("beta_h", case.vk.beta_h), False, case.vk.plookup_comms)
    for vk2 in (other(beta_h=mj.kzg.open_key_for_testing(c, w["beta"] + 1)[2]), other(sigma=case.vk.sigma_comms[1:] + case.vk.sigma_comms[:1])):
        assert not mj.snark.verify(vk2, case.pub, proof, EXTRAS[3])
        vk2.release_verifier()
    if case.pub:
        wrong = case.pub[:3] + [(case.pub[3] + 1) % c.r]
        assert not V.verify(pc, fresh(), case.ovk, wrong, proof, None, None, extra_msg=EXTRAS[3], open_key=w["oracle_open_key"])
        assert not mj.snark.verify(case.vk, wrong, proof, EXTRAS[3])


@pytest.mark.parametrize("cid", [0, 1])
def test_batch_verify_of_65_proofs_under_two_keys(world, mj, cid):
    cases = world[cid]["cases"]
    pick = [(cases[n % 2], [0, 3, 1, 4, 2][n % 5]) for n in range(65)]
    vks, pubs = [cs.vk for cs, _ in pick], [cs.pub for cs, _ in pick]
    proofs, extras = [cs.proofs[i] for cs, i in pick], [EXTRAS[i] for _, i in pick]
    assert mj.snark.batch_verify(vks, pubs, proofs, extras)
    proofs[64] = _flip_eval(proofs[64], pick[64][0], which=2)
    assert not mj.snark.batch_verify(vks, pubs, proofs, extras)
    with pytest.raises(ValueError):
        mj.snark.batch_verify(vks, pubs[:-1], proofs, extras)
    with pytest.raises(ValueError):
        mj.snark.batch_verify([], [], [], [])
    with pytest.raises(ValueError):
        mj.snark.batch_verify([cases[0].vk, world[1 - cid]["cases"][0].vk], [cases[0].pub] * 2, proofs[:2], [None, None])


@pytest.mark.parametrize("cid,j", ALL)
def test_malformed_proofs_are_refused_with_field_and_lowest_index(world, mj, cid, j):
    w = world[cid]
    case, c = w["cases"][j], mj.params.CURVES[cid]
    E = mj.keys.ProofEncodingError
    good = case.proofs[0]
    W = len(case.pr[0]["wires_poly_comms"])
    g1 = 48 if cid == 0 else 32
    evals_off = (8 + W * g1) + g1 + (8 + W * g1) + 2 * g1 + 8

    def refused(proofs, index, field, reason):
        with pytest.raises(E) as e:
            case.vk.verifier().begin(proofs, [case.pub] * len(proofs))
        assert (e.value.index, e.value.field) == (index, field) and reason in e.value.reason, e.value.reason
        assert e.value.reason.startswith(f"proof {index}: {field}: ")

    count = bytearray(good)
    count[8 + W * g1 + g1] = W + 1                                     # split_quot_poly_comms' count
    x_big = bytearray(good)                                           # wires_poly_comms[1].x = q (sign and compression flags kept)
    rec = 8 + g1
    if cid == 0:
        x_big[rec:rec + 48] = bytes([x_big[rec] & 0xE0 | (c.q >> 376)]) + (c.q & ((1 << 376) - 1)).to_bytes(47, "big")
    else:
        x_big[rec:rec + 32] = (c.q | (x_big[rec + 31] & 0x80) << 248).to_bytes(32, "little")
    eval_r = bytearray(good)
    eval_r[evals_off + 32:evals_off + 64] = c.r.to_bytes(32, "little")  # wires_evals[1] = r
    other = w["cases"][1 - j].proofs[0]                               # the other key's type: an Ultra proof under a Turbo key or the reverse
    refused([good, good[:-1], good, good[:-3]], 1, "length", "expected")
    refused([good, other], 1, "length", "expected")
    refused([good, good, bytes(count), bytes(eval_r)], 2, "split_quot_poly_comms.len", f"{W + 1}, expected {W}")
    refused([good, bytes(eval_r), bytes(x_big)], 1, "wires_evals[1]", "not below the modulus")
    refused([bytes(x_big), good, bytes(eval_r)], 0, "wires_poly_comms[1]", "coordinate not below the field modulus")
    tag = bytearray(good)
    tag[evals_off + 32 * W + 8 + 32 * (W - 1) + 32] ^= 1
    refused([good, bytes(tag)], 1, "plookup_proof", "key")


@pytest.mark.parametrize("cid,j", ALL)
def test_a_proof_commitment_at_infinity_is_flagged_not_refused(world, mj, pyref, cid, j):
    import pyref_verifier as V
    w = world[cid]
    case, pc = w["cases"][j], pyref.CURVES[cid]
    g1 = 48 if cid == 0 else 32
    bad = bytearray(case.proofs[0])
    bad[8 + g1:8 + 2 * g1] = FS.g1_bytes(pc, None)                     # wires_poly_comms[1] = O
    b = case.vk.verifier().begin([bytes(bad)], [case.pub])            # decodes
    b.discard()
    want = V.verify(pc, FS.StandardTranscript(pc, b"PlonkProof"), case.ovk, case.pub, bytes(bad), None, None, open_key=w["oracle_open_key"])
    assert mj.snark.verify(case.vk, case.pub, bytes(bad), None) == want and not want


def _uncompressed_proof(pc, pr):
    """Proof::serialize_uncompressed from the oracle's deserialized proof (records as include/mzk.h states them)"""
    import struct
    import pyref_verifier as V
    n = 48 if pc.curve_id == 0 else 32

    def g1(pt):
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
    out = vec(pr["wires_poly_comms"], g1) + g1(pr["prod_perm_poly_comm"]) + vec(pr["split_quot_poly_comms"], g1) + g1(pr["opening_proof"])
    out += g1(pr["shifted_opening_proof"]) + vec(pr["wires_evals"], fr) + vec(pr["wire_sigma_evals"], fr) + fr(pr["perm_next_eval"])
    pl = pr["plookup"]
    if pl is None:
        return out + b"\x00"
    return out + b"\x01" + vec(pl["h_poly_comms"], g1) + g1(pl["prod_lookup_poly_comm"]) + b"".join(fr(pl["evals"][k]) for k in V.PLOOKUP_EVAL_FIELDS)


@pytest.mark.parametrize("cid,j", ALL)
def test_uncompressed_key_and_proofs(world, mj, pyref, cid, j):
    """the same proofs as uncompressed images under the key's uncompressed image: the transcript still takes every commitment in its
    compressed form, so the challenges, the scalars and the decision are those of the compressed run"""
    w = world[cid]
    case, c, pc = w["cases"][j], mj.params.CURVES[cid], pyref.CURVES[cid]
    g, h, beta_h = mj.kzg.open_key_for_testing(c, w["beta"], compress=False)
    vk = mj.keys.VerifyingKey.deserialize(cid, case.prover.serialize_vk(len(case.pub), h, beta_h, compress=False), compress=False)
    assert vk.g == g and len(vk.g) == 2 * len(case.vk.g)
    idx = [0, 3, 4]
    proofs = [_uncompressed_proof(pc, case.pr[i]) for i in idx]
    assert len(proofs[0]) > len(case.proofs[0])
    b = vk.verifier().begin(proofs, [case.pub] * 3, [EXTRAS[i] for i in idx])
    got = fr_from_mont_limbs(c, b.challenges().reshape(-1, 4))
    kr, pr, ev = b.scalars()
    b.discard()
    for n, i in enumerate(idx):
        key_row, own_row = _grouped(pc, case, i)
        assert got[7 * n:7 * n + 7] == [case.ch[i][x] for x in CH], n
        assert fr_from_mont_limbs(c, kr[n]) == key_row and fr_from_mont_limbs(c, pr[n]) == own_row
        assert fr_from_mont_limbs(c, ev[n:n + 1]) == [case.info[i]["eval"]]
    assert mj.snark.batch_verify([vk] * 3, [case.pub] * 3, proofs, [EXTRAS[i] for i in idx])
    flipped = bytearray(proofs[2])
    W = len(case.pr[0]["wires_poly_comms"])
    g1 = 2 * (48 if cid == 0 else 32)
    flipped[(8 + W * g1) + g1 + (8 + W * g1) + 2 * g1 + 8] ^= 1          # wires_evals[0]
    assert not mj.snark.batch_verify([vk] * 3, [case.pub] * 3, proofs[:2] + [bytes(flipped)], [EXTRAS[i] for i in idx])
    vk.release_verifier()


# ---- handles: ownership, device and release (csrc/verifier.hip; DESIGN.md section 4.14 "Handles") ----
ERR_INVALID_ARG, ERR_BAD_HANDLE = -1, -4


@pytest.mark.parametrize("cid", [0, 1])
def test_handle_lifecycle(world, mj, cid):
    """an open batch holds its verifier: destroy is refused and changes nothing; destroyed / consumed handles are unknown to every entry point"""
    import ctypes as C
    case, c = world[cid]["cases"][0], mj.params.CURVES[cid]
    L = mj.load()
    one = fr_mont_limbs(c, [1])
    v = mj.keys.Verifier(case.vk)
    vh = v.handle
    b = v.begin([case.proofs[0]], [case.pub])
    bh = b.handle
    assert L.mzk_verifier_destroy(vh) == ERR_INVALID_ARG and b"open batch" in L.mzk_last_error()
    A, B = b.finish(one)
    A2, B2 = v.begin([case.proofs[0]], [case.pub]).finish(one)        # the same proof with no destroy attempt in between
    assert np.array_equal(A, A2) and np.array_equal(B, B2)
    assert v.check(A, B)
    assert L.mzk_verifier_destroy(vh) == 0
    v.handle = 0
    image = np.frombuffer(case.proofs[0], dtype=np.uint8)
    pub = np.frombuffer(b"".join(int(x).to_bytes(32, "little") for x in case.pub) or bytes(32), dtype=np.uint64)
    ptr = lambda a: C.c_void_p(a.ctypes.data)
    out, ok, big = C.c_uint64(), C.c_int32(), np.zeros((64, 4), dtype=np.uint64)
    assert L.mzk_verifier_shape(vh, None, None, C.byref(out), None) == ERR_BAD_HANDLE
    assert L.mzk_verifier_batch_begin(vh, ptr(image), len(case.proofs[0]), 1, ptr(pub), None, None, None, 0, C.byref(out), None, None) == ERR_BAD_HANDLE
    assert L.mzk_verifier_check(vh, ptr(A), ptr(B), 1, C.byref(ok)) == ERR_BAD_HANDLE
    assert L.mzk_verifier_destroy(vh) == ERR_BAD_HANDLE
    assert L.mzk_verifier_batch_challenges(bh, ptr(big)) == ERR_BAD_HANDLE
    assert L.mzk_verifier_batch_scalars(bh, None, None, None) == ERR_BAD_HANDLE
    assert L.mzk_verifier_batch_finish(bh, ptr(one), ptr(big), ptr(big[32:])) == ERR_BAD_HANDLE


def test_a_failed_begin_leaves_no_batch_open(world, mj):
    case, c = world[0]["cases"][0], mj.params.CURVES[0]
    W = len(case.pr[0]["wires_poly_comms"])
    evals_off = (8 + W * 48) + 48 + (8 + W * 48) + 2 * 48 + 8
    eval_r = bytearray(case.proofs[0])                                # wires_evals[1] = r: the malformed proof of the test above
    eval_r[evals_off + 32:evals_off + 64] = c.r.to_bytes(32, "little")
    v = mj.keys.Verifier(case.vk)
    with pytest.raises(mj.keys.ProofEncodingError) as e:
        v.begin([case.proofs[0], bytes(eval_r)], [case.pub] * 2)
    assert (e.value.index, e.value.field) == (1, "wires_evals[1]")
    assert mj.load().mzk_verifier_destroy(v.handle) == 0              # at once: nothing was left registered
    v.handle = 0


def test_a_handle_finds_its_device(world, mj, tmp_path):
    """Two contexts in a child process (MZK_VIRTUAL_DEVICES=2, read at mzk_init): a verifier created on device 1 is driven from a thread bound to
    device 0.  Handles name device 1, the results are the parent's, the thread's binding is untouched, and mzk_shutdown releases the handle."""
    import json
    import os
    import subprocess
    case, c = world[0]["cases"][0], mj.params.CURVES[0]
    one = fr_mont_limbs(c, [1])
    A, B = case.vk.verifier().begin([case.proofs[0]], [case.pub]).finish(one)
    assert case.vk.verifier().check(A, B)
    np.savez(tmp_path / "want.npz", A=A, B=B, one=one)
    (tmp_path / "key.bin").write_bytes(case.vk.serialize())
    (tmp_path / "proof.bin").write_bytes(case.proofs[0])
    (tmp_path / "pub.json").write_text(json.dumps([int(x) for x in case.pub]))
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = r'''
import ctypes as C, json, os, sys
import numpy as np
sys.path.insert(0, %r)
d = %r
import mpc_jellyfish_amd as mj
from importlib import import_module
lib = import_module("mpc-jellyfish_amd.lib")
L = lib.init(0)
lib.check(L.mzk_init(1), "init1"); lib.check(L.mzk_set_device(1), "set1")
def bound():
    dev = C.c_int32(-1)
    lib.check(L.mzk_get_device(C.byref(dev)), "get")
    return dev.value
want = np.load(os.path.join(d, "want.npz"))
pub = json.load(open(os.path.join(d, "pub.json")))
proof = open(os.path.join(d, "proof.bin"), "rb").read()
v = mj.keys.VerifyingKey.deserialize(0, open(os.path.join(d, "key.bin"), "rb").read()).verifier()
assert v.handle >> 48 == 2 and bound() == 1                         # created on the calling thread's device, which the handle names
lib.check(L.mzk_set_device(0), "set0")
b = v.begin([proof], [pub])
assert b.handle >> 48 == 2 and bound() == 0
ch = b.challenges()
assert ch.any() and bound() == 0
A, B = b.finish(want["one"])
assert bound() == 0
assert np.array_equal(A, want["A"]) and np.array_equal(B, want["B"])
assert v.check(A, B) and bound() == 0
lib.check(L.mzk_shutdown(), "shutdown")
lib.check(L.mzk_init(0), "init0 again")
assert L.mzk_verifier_shape(v.handle, None, None, None, None) == -4  # MZK_ERR_BAD_HANDLE: the shutdown released it
print("ok")
''' % (root, str(tmp_path))
    out = subprocess.run([os.sys.executable, "-c", code], capture_output=True, text=True, timeout=300, env=dict(os.environ, MZK_VIRTUAL_DEVICES="2"))
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stderr[-3000:]
