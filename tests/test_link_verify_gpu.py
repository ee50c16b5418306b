"""GPU: the library's proof-link verifier (mzk_verifier_create_open_key / _link_begin / _link_values / _link_weights: csrc/verifier.cuh
"proof links"; linking.verify_link_proof, linking.batch_verify_link_proofs, snark.batch_verify(links=..)) against the big-int restatement
oracle/pyref_linking.py (quotient_challenge, vanishing_eval, verify_link_proof in its trapdoor form).

Synthetic links come from the oracle and need no prover: a_1 random of size + 12 coefficients, a_2 = a_1 + s Z_D with 12 random coefficients
in s, both committed through the trapdoor, linked by L.link_proofs.  Per curve every link and every oracle verdict is computed once (the `world`
fixture) and shared by the tests."""
import ctypes as C
import random

import numpy as np
import pytest

from conftest import build_circuit, fr_from_mont_limbs, fr_mont_limbs, load_golden
import pyref_fs as FS
from test_linking_gpu import _prove_linked

pytestmark = pytest.mark.gpu

ERR_INVALID_ARG, ERR_UNSUPPORTED = -1, -5
# (alignment, offset, size): 63 .. 129 the lane-stride edges of the vanishing kernel (64 lanes), (7,120,20) wraps past 2^alignment, (3,2,11) repeats roots
LAYOUTS = [(4, 2, 9), (5, 4, 1), (5, 0, 0), (8, 3, 63), (8, 3, 64), (8, 3, 65), (8, 3, 128), (8, 3, 129), (7, 120, 20), (3, 2, 11)]
VARIANTS = ("valid", "offset+1", "alignment+1", "size+1", "swapped", "one point")
FIELDS = ("lhs.wires_poly_comms[0]", "rhs.wires_poly_comms[0]", "quotient_commitment", "opening_proof")


def _g1_uncompressed(pc, pt):
    """Affine<G1>::serialize_uncompressed (include/mzk.h, "G1 records")"""
    n = 48 if pc.curve_id == 0 else 32
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


class Link:
    """one link as the oracle made it: the four points, the layout it is verified under, eta, Z_D(eta) and the oracle's verdict"""

    def __init__(self, pc, P, L, points, layout_args, srs_beta):
        self.points, self.layout_args = points, layout_args
        lay = L.GroupLayout(*layout_args)
        self.eta = L.quotient_challenge(FS.StandardTranscript(pc, b"PlonkLinkingProof"), *points[:3])
        self.vanish = L.vanishing_eval(pc, lay, self.eta)
        self.verdict = L.verify_link_proof(pc, FS.StandardTranscript(pc, b"PlonkLinkingProof"), *points, lay, srs_beta)
        self._pc = pc

    def tuple(self, mj, compress=True):
        enc = (lambda p: FS.g1_bytes(self._pc, p)) if compress else (lambda p: _g1_uncompressed(self._pc, p))
        a1, a2, q, o = self.points
        return enc(a1), enc(a2), enc(q) + enc(o), mj.linking.GroupLayout(*self.layout_args)


def _pmul(r, a, b):
    out = [0] * (len(a) + len(b) - 1)
    for i, x in enumerate(a):
        for j, y in enumerate(b):
            out[i + j] = (out[i + j] + x * y) % r
    return out


def _synthetic(pc, P, L, rng, layout_args, srs_beta):
    """{variant: Link} for one layout"""
    r = pc.r
    al, off, size = layout_args
    lay = L.GroupLayout(*layout_args)
    z = L.vanishing_polynomial(pc, lay)
    a1 = [rng.randrange(r) for _ in range(size + 12)]
    sz = _pmul(r, [rng.randrange(r) for _ in range(12)], z)
    a2 = [(x + y) % r for x, y in zip(a1, sz)]
    G = P.g1_gen(pc)
    commit = lambda poly: P.g1_mul(pc, P.poly_eval(pc, poly, srs_beta), G)
    fresh = lambda: FS.StandardTranscript(pc, b"PlonkLinkingProof")
    a1c, a2c = commit(a1), commit(a2)
    lp = L.link_proofs(pc, a1, a2, a1c, a2c, lay, srs_beta, fresh())
    pts = (a1c, a2c, lp["quotient_commitment"], lp["opening_proof"])
    out = {"valid": Link(pc, P, L, pts, layout_args, srs_beta),
           "offset+1": Link(pc, P, L, pts, (al, off + 1, size), srs_beta),
           "alignment+1": Link(pc, P, L, pts, (al + 1, off, size), srs_beta),
           "size+1": Link(pc, P, L, pts, (al, off, size + 1), srs_beta),
           "swapped": Link(pc, P, L, (a2c, a1c, pts[2], pts[3]), layout_args, srs_beta)}
    assert out["valid"].verdict and out["valid"].eta == lp["eta"]
    if size:                                                          # a_2 differs from a_1 at one point of the domain: + Z_D / (X - g^offset)
        root = pow(lay.domain_generator(pc), off, r)
        delta = L.pdiv(pc, z, [-root % r, 1])
        b2 = [(x + (delta[i] if i < len(delta) else 0)) % r for i, x in enumerate(a2)]
        b2c = commit(b2)
        lp2 = L.link_proofs(pc, a1, b2, a1c, b2c, lay, srs_beta, fresh())
        out["one point"] = Link(pc, P, L, (a1c, b2c, lp2["quotient_commitment"], lp2["opening_proof"]), layout_args, srs_beta)
    return out


@pytest.fixture(scope="module")
def world(gpu, mj, pyref):
    import pyref_linking as L
    out = {}
    for cid in (0, 1):
        c, pc = mj.params.CURVES[cid], pyref.CURVES[cid]
        rng = random.Random(4100 + cid)
        srs_beta = rng.randrange(1, c.r)
        keys = {cmp: mj.keys.OpenKey(c, *mj.kzg.open_key_for_testing(c, srs_beta, compress=cmp), compressed=cmp) for cmp in (True, False)}
        out[cid] = dict(beta=srs_beta, keys=keys, links={la: _synthetic(pc, pyref, L, rng, la, srs_beta) for la in LAYOUTS})
    yield out
    for w in out.values():
        for k in w["keys"].values():
            k.release()


def _verdict(mj, key, link, compress=True):
    return mj.linking.batch_verify_link_proofs(key, [link.tuple(mj, compress)])


# ---- 1. golden ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("index", [0, 1])
def test_golden_link_vectors(gpu, mj, index):
    vec = load_golden("link_vectors")[index]
    c = mj.params.CURVES[vec["curve"]]
    key = mj.keys.OpenKey(c, *mj.kzg.open_key_for_testing(c, int(vec["srs_beta"], 16)))
    p1, p2 = (bytes.fromhex(p) for p in vec["proofs"])
    link = bytes.fromhex(vec["link_proof"])
    layout = mj.linking.GroupLayout(*vec["layout"])
    wire = lambda p: mj.linking.linking_wire_record(c, p)
    b = key.begin_links([(wire(p1), wire(p2), link, layout)])
    eta, _ = b.link_values()
    b.discard()
    assert fr_from_mont_limbs(c, eta) == [int(vec["eta"], 16)] and np.array_equal(eta, b.u)
    assert mj.linking.verify_link_proof(p1, p2, link, layout, key) is True
    half = len(link) // 2
    assert mj.linking.verify_link_proof(p1, p2, link[half:] + link[:half], layout, key) is False
    key.release()


# ---- 2. single links ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("compress", [True, False])
@pytest.mark.parametrize("cid", [0, 1])
def test_single_links_decide_as_the_oracle(world, mj, cid, compress):
    c, w = mj.params.CURVES[cid], world[cid]
    key = w["keys"][compress]
    one = fr_mont_limbs(c, [1])
    for la in LAYOUTS:
        for name in VARIANTS:
            link = w["links"][la].get(name)
            if link is None:                                          # size 0: the domain has no point to differ at
                assert la[2] == 0 and name == "one point"
                continue
            b = key.begin_links([link.tuple(mj, compress)])
            eta, van = b.link_values()
            kr, pr, ev = b.scalars()
            assert np.array_equal(b.link_weights(), one), "one link, no r: weight exactly 1"
            A, B = b.finish(one)
            assert fr_from_mont_limbs(c, eta) == [link.eta] and fr_from_mont_limbs(c, van) == [link.vanish], (la, name)
            assert fr_from_mont_limbs(c, pr[0]) == [1, c.r - 1, -link.vanish % c.r, link.eta], (la, name)
            assert not kr.any() and not ev.any() and kr.shape == (1, 1, 4)
            assert key.check(A, B) == link.verdict, (la, name)
            if la[2] and la not in ((7, 120, 20), (3, 2, 11)):       # (an empty domain, wrapped or repeated roots: whatever the oracle decides)
                assert link.verdict == (name == "valid"), (la, name)
        # the eta seam: the oracle's eta in place of the transcript stage gives the same scalars
        link = w["links"][la]["valid"]
        b = key.begin_links([link.tuple(mj, compress)], eta=fr_mont_limbs(c, [link.eta]))
        assert fr_from_mont_limbs(c, b.scalars()[1][0]) == [1, c.r - 1, -link.vanish % c.r, link.eta]
        assert fr_from_mont_limbs(c, b.link_values()[1]) == [link.vanish]
        b.discard()


# ---- 3. infinity ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("compress", [True, False])
@pytest.mark.parametrize("cid", [0, 1])
def test_a_proof_linked_with_itself(world, mj, pyref, cid, compress):
    """proof_linking.rs:124-127: Q = pi = O, both records the infinity encoding: flagged, accepted, and the finish runs over flagged bases"""
    import pyref_linking as L
    c, pc, w = mj.params.CURVES[cid], pyref.CURVES[cid], world[cid]
    a1c = w["links"][(4, 2, 9)]["valid"].points[0]
    link = Link(pc, pyref, L, (a1c, a1c, None, None), (4, 2, 9), w["beta"])
    assert link.verdict
    key = w["keys"][compress]
    b = key.begin_links([link.tuple(mj, compress)])
    _, pr, _ = b.scalars()
    assert fr_from_mont_limbs(c, pr[0]) == [1, c.r - 1, -link.vanish % c.r, link.eta]
    A, B = b.finish(b.link_weights())
    assert key.check(A, B)
    other = Link(pc, pyref, L, (a1c, w["links"][(4, 2, 9)]["valid"].points[1], None, None), (4, 2, 9), w["beta"])   # a_1 != a_2 with Q = pi = O
    assert _verdict(mj, key, other, compress) is other.verdict is False


# ---- 4. batches -----------------------------------------------------------------------------------------------------------------------------
MIXED = [(4, 2, 9), (8, 3, 65), (5, 4, 1), (8, 3, 129), (5, 0, 0)]


@pytest.mark.parametrize("cid", [0, 1])
def test_batches_decide_as_the_and_of_the_oracles_verdicts(world, mj, cid):
    w = world[cid]
    key = w["keys"][True]
    good = [w["links"][la]["valid"] for la in MIXED]
    bad = [w["links"][la]["one point" if la[2] else "offset+1"] for la in MIXED]
    bad[4] = w["links"][(5, 0, 0)]["swapped"]                         # (size 0: another offset is the same empty domain)
    assert mj.linking.batch_verify_link_proofs(key, [l.tuple(mj) for l in good]) is all(l.verdict for l in good) is True
    for k in range(5):
        links = good[:k] + [bad[k]] + good[k + 1:]
        want = all(l.verdict for l in links)
        assert mj.linking.batch_verify_link_proofs(key, [l.tuple(mj) for l in links]) is want is False, k


def _weights_restated(pc, etas, records, r=None):
    t = FS.Merlin(b"batch verify links")
    if r is not None:
        t.append_message(b"r", FS.fr_bytes(pc, r))
    for e in etas:
        t.append_message(b"eta", FS.fr_bytes(pc, e))
    for rec in records:
        t.append_message(b"opening_proof", rec)
    s = int.from_bytes(t.challenge_bytes(b"s", 64), "little") % pc.r
    return [pow(s, i + 1, pc.r) for i in range(len(etas))]


@pytest.mark.parametrize("compress", [True, False])
@pytest.mark.parametrize("cid", [0, 1])
def test_link_weights(world, mj, pyref, cid, compress):
    c, pc, w = mj.params.CURVES[cid], pyref.CURVES[cid], world[cid]
    key = w["keys"][compress]
    links = [w["links"][la]["valid"] for la in MIXED[:3]]
    tuples = [l.tuple(mj, compress) for l in links]
    G = len(tuples[0][0])
    b = key.begin_links(tuples)
    r = 0x1234567 * 0x10001 % c.r
    for rr in (None, r):
        got = fr_from_mont_limbs(c, b.link_weights(None if rr is None else fr_mont_limbs(c, [rr])[0]))
        assert got == _weights_restated(pc, [l.eta for l in links], [t[2][G:] for t in tuples], rr), rr
        assert 1 not in got
    base = fr_from_mont_limbs(c, b.link_weights())
    b.discard()
    # only one opening record changes (link 1's, for another link's: still a valid record): every weight changes
    other = w["links"][(8, 3, 64)]["valid"].tuple(mj, compress)[2][G:]
    changed = list(tuples)
    changed[1] = (tuples[1][0], tuples[1][1], tuples[1][2][:G] + other, tuples[1][3])
    b = key.begin_links(changed)
    assert fr_from_mont_limbs(c, b.link_values()[0]) == [l.eta for l in links], "eta does not see the opening proof"
    got = fr_from_mont_limbs(c, b.link_weights())
    b.discard()
    assert all(x != y for x, y in zip(got, base))
    # one link with r: not 1
    b = key.begin_links(tuples[:1])
    assert fr_from_mont_limbs(c, b.link_weights(fr_mont_limbs(c, [r])[0])) == _weights_restated(pc, [links[0].eta], [tuples[0][2][G:]], r)
    b.discard()


# ---- 5. a bundle ----------------------------------------------------------------------------------------------------------------------------
def test_a_bundle_of_two_proofs_and_their_link(gpu, mj, pyref):
    """two real TurboPlonk proofs (log_n 5 and 6, BN254) that share a group, their LinkingProof, one pairing check for all three"""
    cid = 1
    c, pc = mj.params.CURVES[cid], pyref.CURVES[cid]
    layout = mj.linking.GroupLayout(5, 4, 6)
    rng = random.Random(99)
    shared = [rng.randrange(c.r) for _ in range(layout.size)]
    srs_beta = rng.randrange(1, c.r)
    ck = mj.UnivariateProverParam.gen_srs_for_testing(c, srs_beta, (1 << 6) + 2)
    g, h, beta_h = mj.kzg.open_key_for_testing(c, srs_beta)
    rec = lambda cm: mj.snark._g1(c, cm)
    vks, pubs, proofs, hints, provers = [], [], [], [], []
    for log_n in (5, 6):
        proof, pub, hint, prover = _prove_linked(mj, pyref, cid, log_n, layout, shared, random.Random(500 + log_n), srs_beta, ck)
        sel, sig = prover.vk_commitments()
        vks.append(mj.keys.VerifyingKey(c, prover.n, len(pub), [rec(x) for x in sig], [rec(x) for x in sel], prover.k, g, h, beta_h))
        pubs.append(pub), proofs.append(proof), hints.append(hint), provers.append(prover)
    link = mj.linking.link_proofs(hints[0], hints[1], layout, ck).serialize_compressed()
    none = [None, None]
    assert mj.snark.batch_verify(vks, pubs, proofs, none) is True
    assert mj.snark.batch_verify(vks, pubs, proofs, none, links=[(0, 1, link, layout)]) is True
    assert mj.linking.verify_link_proof(proofs[0], proofs[1], link, layout, vks[0]) is True
    # the link made over a layout the circuits do not share
    wrong = mj.linking.GroupLayout(5, 3, 6)
    bad_link = mj.linking.link_proofs(hints[0], hints[1], wrong, ck).serialize_compressed()
    assert mj.snark.batch_verify(vks, pubs, proofs, none, links=[(0, 1, bad_link, wrong)]) is False
    assert mj.snark.batch_verify(vks, pubs, proofs, none) is True
    # proof 1 replaced by another valid proof of the same circuit and witness (other blinders: another wire commitment)
    _, _, _, w, pi = build_circuit(pc, 6, random.Random(506), reserved={(4 + i) * 2: v for i, v in enumerate(shared)})
    blind = mj.snark.draw_blinders(c, mj.rng.ChaChaRng(bytes([77]) * 32, 12), 5, False)
    src = mj.prover.TranscriptChallenges(provers[1], pi[:4])
    other = mj.snark.serialize_proof(c, provers[1].prove(np.stack([fr_mont_limbs(c, col) for col in w]), fr_mont_limbs(c, pi), src, blind))
    assert other != proofs[1] and pi[:4] == pubs[1]
    assert mj.snark.batch_verify(vks, pubs, [proofs[0], other], none) is True
    assert mj.snark.batch_verify(vks, pubs, [proofs[0], other], none, links=[(0, 1, link, layout)]) is False
    for vk in vks:
        vk.release_verifier()
    for p in provers:
        p.release()
    ck.release()


# ---- 6. encoding and refusals ------------------------------------------------------------------------------------------------------------
def _x_not_below_q(c, rec):
    out = bytearray(rec)
    if c.curve_id == 0:
        out[:48] = bytes([out[0] & 0xE0 | (c.q >> 376)]) + (c.q & ((1 << 376) - 1)).to_bytes(47, "big")
    else:
        out[:32] = (c.q | (out[31] & 0x80) << 248).to_bytes(32, "little")
    return bytes(out)


def _x_off_the_curve(c, pc):
    b = 4 if c.curve_id == 0 else 3
    x = next(x for x in range(1, 100) if pow((x ** 3 + b) % c.q, (c.q - 1) // 2, c.q) != 1)
    return FS.g1_bytes(pc, (x, 1))


@pytest.mark.parametrize("cid", [0, 1])
def test_malformed_links_are_refused_with_field_and_lowest_index(world, mj, pyref, cid):
    c, pc, w = mj.params.CURVES[cid], pyref.CURVES[cid], world[cid]
    key = w["keys"][True]
    lhs, rhs, lp, lay = w["links"][(4, 2, 9)]["valid"].tuple(mj)
    G = len(lhs)
    links = [(lhs, rhs, lp, lay), (lhs, rhs, _x_not_below_q(c, lp[:G]) + lp[G:], lay), (_x_off_the_curve(c, pc), rhs, lp, lay)]
    for _ in range(2):
        with pytest.raises(mj.keys.ProofEncodingError) as e:
            key.begin_links(links)
        assert (e.value.index, e.value.field) == (1, "quotient_commitment"), e.value.reason
        assert e.value.reason == "link 1: quotient_commitment: coordinate not below the field modulus"
    with pytest.raises(mj.keys.ProofEncodingError) as e:
        key.begin_links([links[0], links[2]])
    assert (e.value.index, e.value.field) == (1, "lhs.wires_poly_comms[0]") and e.value.field in FIELDS
    key.release()                                                     # mzk_verifier_destroy succeeds: no batch was left open


@pytest.mark.parametrize("cid", [0, 1])
def test_open_key_verifier_and_host_side_refusals(world, mj, cid):
    c, w = mj.params.CURVES[cid], world[cid]
    key = w["keys"][True]
    v = key.verifier()
    L = mj.load()
    assert (v.n_proof_points, v.n_key_bases, v.proof_len, v.num_inputs) == (0, 0, 0, 0)
    with pytest.raises(ValueError, match="the verifier holds no verifying key"):
        v.begin([b"x"], [[]])
    out, dummy = C.c_uint64(), np.zeros(64, dtype=np.uint8)
    ptr = lambda a: C.c_void_p(a.ctypes.data)
    assert L.mzk_verifier_batch_begin(v.handle, ptr(dummy), 64, 1, None, None, None, None, 0, C.byref(out), None, None) == ERR_INVALID_ARG
    assert L.mzk_last_error() == b"the verifier holds no verifying key"
    handles = (C.c_uint64 * 1)(v.handle)
    assert L.mzk_verifier_aggregate_begin(handles, 1, ptr(dummy), 64, 1, None, None, None, None, 0, C.byref(out), None, None) == ERR_INVALID_ARG
    assert L.mzk_last_error() == b"the verifier holds no verifying key"
    # layouts refused on the host, before any launch
    lhs, rhs, lp, _ = w["links"][(4, 2, 9)]["valid"].tuple(mj)
    two_adicity = 32 if cid == 0 else 28

    def launches():
        n = C.c_uint64()
        assert L.mzk_launch_count(C.byref(n)) == 0
        return n.value
    before = launches()
    for layout, code in (((two_adicity + 1, 0, 4), ERR_INVALID_ARG), ((4, 0, (1 << 27) + 1), ERR_UNSUPPORTED)):
        with pytest.raises(mj.MzkError) as e:
            v.begin_links([(lhs, rhs, lp, mj.linking.GroupLayout(*layout))])
        assert e.value.code == code
    with pytest.raises(ValueError):
        v.begin_links([])
    recs = np.frombuffer(lhs + rhs + lp, dtype=np.uint8)
    lay = np.array([4, 2, 9], dtype=np.uint64)
    assert L.mzk_verifier_link_begin(v.handle, ptr(recs), 0, ptr(lay), None, 0, C.byref(out), None, None) == ERR_INVALID_ARG
    assert launches() == before
    # an open link batch holds its verifier; it has no seven challenges
    b = v.begin_links([(lhs, rhs, lp, mj.linking.GroupLayout(4, 2, 9))])
    assert L.mzk_verifier_destroy(v.handle) == ERR_INVALID_ARG and b"open batch" in L.mzk_last_error()
    assert L.mzk_verifier_batch_challenges(b.handle, ptr(np.zeros(64, dtype=np.uint64))) == ERR_INVALID_ARG
    A, B = b.finish(b.link_weights())
    assert v.check(A, B)
    assert L.mzk_verifier_link_values(b.handle, None, None) == -4      # consumed: MZK_ERR_BAD_HANDLE
