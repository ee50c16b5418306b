"""GPU: which defect a refused batch names (mzk_verifier_batch_begin, mzk_verifier_create), on the keys and proofs of tests/test_verify_gpu.py
and with the defects of its test_malformed_proofs_are_refused_with_field_and_lowest_index.  Every stage reports through one error word,
lowest proof first and within a proof its first field: the G1 records in image order, then the evaluations, then the public inputs.
These cases pin that order where several defects meet, a proof index beyond one block of 64 threads, the public inputs' range check under
caller-supplied challenges, and the key's own field names.  (A link's: tests/test_link_verify_gpu.py,
test_malformed_links_are_refused_with_field_and_lowest_index.)"""
import types

import pytest

from test_verify_gpu import ALL, world  # noqa: F401  (the module's fixture: the same keys and proofs)

pytestmark = pytest.mark.gpu

NOT_BELOW_Q, NOT_BELOW_R = "coordinate not below the field modulus", "not below the modulus"


def _x_is_q(c, image, rec):
    """the G1 record at `rec` with x = q, sign and compression flags kept"""
    out = bytearray(image)
    if c.curve_id == 0:
        out[rec:rec + 48] = bytes([out[rec] & 0xE0 | (c.q >> 376)]) + (c.q & ((1 << 376) - 1)).to_bytes(47, "big")
    else:
        out[rec:rec + 32] = (c.q | (out[rec + 31] & 0x80) << 248).to_bytes(32, "little")
    return bytes(out)


def _fr_is_r(c, image, rec):
    out = bytearray(image)
    out[rec:rec + 32] = c.r.to_bytes(32, "little")
    return bytes(out)


class Layout:
    """byte offsets of a `Proof` image (structs.rs:59-84) of W wire types with G-byte commitments"""

    def __init__(self, case, cid):
        W, G = len(case.pr[0]["wires_poly_comms"]), 48 if cid == 0 else 32
        self.ultra = case.pr[0]["plookup"] is not None
        self.wires = [8 + k * G for k in range(W)]
        self.split_quot = [8 + W * G + G + 8 + k * G for k in range(W)]
        self.opening = self.split_quot[0] + W * G
        self.shifted_opening = self.opening + G
        self.wires_evals = [self.shifted_opening + G + 8 + 32 * k for k in range(W)]
        tag = self.wires_evals[0] + 32 * W + 8 + 32 * (W - 1) + 32
        self.prod_lookup = tag + 1 + 8 + 2 * G
        self.range_table_eval = self.prod_lookup + G


def _refused(mj, case, proofs, index, field, reason, pubs=None, challenges=None):
    with pytest.raises(mj.keys.ProofEncodingError) as e:
        case.vk.verifier().begin(proofs, pubs or [case.pub] * len(proofs), None, challenges)
    assert (e.value.index, e.value.field) == (index, field), e.value.reason
    assert e.value.reason == f"proof {index}: {field}: {reason}"


@pytest.mark.parametrize("cid,j", ALL)
def test_a_point_is_named_before_an_evaluation_of_the_same_proof(world, mj, cid, j):
    case, c = world[cid]["cases"][j], mj.params.CURVES[cid]
    good = case.proofs[0]
    at = Layout(case, cid)
    later = _x_is_q(c, good, at.wires[1])                             # proof 2: a defect in an earlier field of a later proof
    pairs = [("shifted_opening_proof", at.shifted_opening, at.wires_evals[1]), ("split_quot_poly_comms[0]", at.split_quot[0], at.wires_evals[1])]
    if at.ultra:
        pairs.append(("plookup_proof.prod_lookup_poly_comm", at.prod_lookup, at.range_table_eval))
    for field, point, evaluation in pairs:
        both = _fr_is_r(c, _x_is_q(c, good, point), evaluation)
        _refused(mj, case, [good, both, later], 1, field, NOT_BELOW_Q)


@pytest.mark.parametrize("cid,j", ALL)
def test_the_last_of_65_proofs_is_named(world, mj, cid, j):
    case, c = world[cid]["cases"][j], mj.params.CURVES[cid]
    good = case.proofs[0]
    at = Layout(case, cid)
    _refused(mj, case, [good] * 64 + [_fr_is_r(c, good, at.wires_evals[0])], 64, "wires_evals[0]", NOT_BELOW_R)
    _refused(mj, case, [good] * 64 + [_x_is_q(c, good, at.wires[1])], 64, "wires_poly_comms[1]", NOT_BELOW_Q)


@pytest.mark.parametrize("cid", [0, 1])
def test_a_public_input_is_range_checked_under_supplied_challenges(world, mj, cid):
    case, c = world[cid]["cases"][0], mj.params.CURVES[cid]           # the general circuit: four public inputs
    proofs = [case.proofs[i] for i in (0, 1, 2)]
    b = case.vk.verifier().begin(proofs, [case.pub] * 3)
    ch = b.challenges()                                               # the batch's own: zeta is a hash value, off the domain
    b.discard()
    pubs = [case.pub, case.pub[:2] + [c.r] + case.pub[3:], case.pub]
    _refused(mj, case, proofs, 1, "public_input[2]", NOT_BELOW_R, pubs=pubs, challenges=ch)
    _refused(mj, case, proofs, 1, "public_input[2]", NOT_BELOW_R, pubs=pubs)


@pytest.mark.parametrize("cid,j", ALL)
def test_a_key_commitment_is_named(world, mj, cid, j):
    case, c = world[cid]["cases"][j], mj.params.CURVES[cid]
    image = case.vk.serialize()
    lay = mj.keys.key_layout(c, image, vk_only=True)
    bad = _x_is_q(c, image, lay.sigma_comms_off + 2 * (48 if cid == 0 else 32))
    with pytest.raises(mj.keys.KeySerializationError) as e:
        mj.keys.Verifier(types.SimpleNamespace(curve=c, compressed=True, serialize=lambda: bad))
    assert e.value.reason == "vk.sigma_comms[2]: " + NOT_BELOW_Q
