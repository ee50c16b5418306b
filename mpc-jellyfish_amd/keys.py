"""ProvingKey / VerifyingKey as their CanonicalSerialize images (ark-serialize 0.4, derive order; include/mzk.h, mzk_key_layout):

    ProvingKey<E>    plonk/src/proof_system/structs.rs:575-590  -> ProvingKey.deserialize: a TurboPlonkProver on the GPU
    VerifyingKey<E>  structs.rs:682-707                          -> VerifyingKey: fields, records as bytes, serialize / deserialize

The container is parsed on the host (mzk_key_layout: no GPU); the polynomials, k and the commit key are decoded and checked on the
device (mzk_prover_create_serialized).  G1 / G2 records of the verifying key are kept as the bytes they were read as.  The image names
neither its curve nor its mode: the caller states both, as for the SRS (kzg.UnivariateProverParam.deserialize).
"""
from __future__ import annotations

import ctypes as C
import re

import numpy as np

from . import kzg
from . import lib as _lib
from . import transcript as _transcript
from .kzg import SerializationError
from .params import curve as _curve

_SER_COMPRESSED, _SER_VALIDATE, _KEY_CHECK_COMMITMENTS, _KEY_VK_ONLY = 1, 2, 4, 8
_ERR_ENCODING = -11
_FIELD = re.compile(r"^([A-Za-z_.]+(?:\[\d+\])?(?:\.len)?)")


class KeySerializationError(SerializationError):
    """A serialized key that ark-serialize would refuse (MZK_ERR_ENCODING).  .field: the field of the image the error is in
    ("sigmas[2]", "commit_key", "vk.selector_comms[3]", ..); .index: the index within it (coefficient, point; None for container
    errors); .reason: the library's text."""

    def __init__(self, reason: str, field: str | None, index: int | None = None):
        ValueError.__init__(self, reason)
        self.field, self.index, self.reason = field, index, reason


def _raise_encoding(L, bad: int | None):
    msg = L.mzk_last_error().decode()
    m = _FIELD.match(msg[len("truncated in "):] if msg.startswith("truncated in ") else msg)
    raise KeySerializationError(msg, m.group(1) if m else None, None if bad is None or bad == 2**64 - 1 else bad)


def key_layout(curve, data, compress: bool = True, vk_only: bool = False) -> _lib.KeyLayout:
    """mzk_key_layout: offsets and counts of every field of a ProvingKey (or, vk_only, a bare VerifyingKey) image.  Host-only."""
    c = _curve(curve)
    buf = kzg._as_bytes(data)
    L = _lib.load()
    out = _lib.KeyLayout()
    rc = L.mzk_key_layout(c.curve_id, C.c_void_p(buf.ctypes.data) if buf.shape[0] else None, buf.shape[0],
                          (_SER_COMPRESSED if compress else 0) | (_KEY_VK_ONLY if vk_only else 0), C.byref(out))
    if rc == _ERR_ENCODING:
        _raise_encoding(L, None)
    _lib.check(rc, "mzk_key_layout")
    return out


class VerifyingKey:
    """structs.rs:682-707.  domain_size, num_inputs, is_merged; k as canonical integers; sigma_comms / selector_comms / plookup_comms
    (None for TurboPlonk) as lists of G1 records and g, h, beta_h as records, all bytes of the mode `compressed`."""

    def __init__(self, curve, domain_size, num_inputs, sigma_comms, selector_comms, k, g, h, beta_h, is_merged=False, plookup_comms=None, compressed=True):
        self.curve = _curve(curve)
        self.domain_size, self.num_inputs, self.is_merged, self.compressed = domain_size, num_inputs, bool(is_merged), compressed
        self.sigma_comms, self.selector_comms, self.k = [bytes(b) for b in sigma_comms], [bytes(b) for b in selector_comms], [int(x) for x in k]
        self.g, self.h, self.beta_h = bytes(g), bytes(h), bytes(beta_h)
        self.plookup_comms = None if plookup_comms is None else [bytes(b) for b in plookup_comms]

    @classmethod
    def _from_layout(cls, c, buf, lay, compress) -> "VerifyingKey":
        g1, g2, W, nsel = lay.g1_record_bytes, lay.g2_record_bytes, lay.num_wire_types, lay.num_selectors
        cut = lambda off, size: bytes(buf[off:off + size])
        recs = lambda off, cnt: [cut(off + i * g1, g1) for i in range(cnt)]
        return cls(c, lay.domain_size, lay.num_inputs, recs(lay.sigma_comms_off, W), recs(lay.selector_comms_off, nsel),
                   [int.from_bytes(cut(lay.k_off + 32 * i, 32), "little") for i in range(W)], cut(lay.g_off, g1), cut(lay.h_off, g2), cut(lay.beta_h_off, g2),
                   lay.is_merged, recs(lay.plookup_comms_off, 4) if lay.has_plookup_vk else None, compress)

    @classmethod
    def deserialize(cls, curve, data, compress: bool = True) -> "VerifyingKey":
        """A bare VerifyingKey image (mzk_key_layout with MZK_KEY_VK_ONLY); raises KeySerializationError naming the field."""
        c = _curve(curve)
        buf = kzg._as_bytes(data)
        return cls._from_layout(c, buf, key_layout(c, buf, compress, vk_only=True), compress)

    def serialize(self) -> bytes:
        u64 = lambda v: int(v).to_bytes(8, "little")
        vec = lambda items: u64(len(items)) + b"".join(items)
        out = u64(self.domain_size) + u64(self.num_inputs) + vec(self.sigma_comms) + vec(self.selector_comms)
        out += vec([x.to_bytes(32, "little") for x in self.k]) + self.g + self.h + self.beta_h + bytes([int(self.is_merged)])
        return out + (b"\x00" if self.plookup_comms is None else b"\x01" + b"".join(self.plookup_comms))

    def verifier(self, validate: bool = True) -> "Verifier":
        """The device verifier of this key (mzk_verifier_create), created once and cached; release_verifier() frees it."""
        v = getattr(self, "_verifier", None)
        if v is None:
            v = self._verifier = Verifier(self, validate)
        return v

    def release_verifier(self):
        v = getattr(self, "_verifier", None)
        if v is not None:
            v.release()
            self._verifier = None


class OpenKey:
    """UnivariateVerifierParam / OpenKey (univariate_kzg/srs.rs:48-55): g (G1), h, beta_h (G2) as records of the mode `compressed` -- all that
    PlonkKzgSnark::verify_link_proof takes.  verifier(): a device verifier that carries the open key alone (mzk_verifier_create_open_key):
    it begins link batches and runs the pairing check, but holds no verifying key (begin() raises)."""

    def __init__(self, curve, g, h, beta_h, compressed: bool = True):
        self.curve, self.compressed = _curve(curve), compressed
        self.g, self.h, self.beta_h = bytes(g), bytes(h), bytes(beta_h)

    def verifier(self, validate: bool = True) -> "Verifier":
        v = getattr(self, "_verifier", None)
        if v is None:
            v = self._verifier = Verifier(self, validate)
        return v

    def begin_links(self, links, eta=None, validate: bool = True, transcript: str = "merlin") -> "VerifierBatch":
        return self.verifier().begin_links(links, eta, validate, transcript)

    def begin_openings(self, commitments, points, values, proofs, validate: bool = True) -> "VerifierBatch":
        return self.verifier().begin_openings(commitments, points, values, proofs, validate)

    def check(self, A_xyz, B_xyz) -> bool:
        return self.verifier().check(A_xyz, B_xyz)

    def release(self):
        v = getattr(self, "_verifier", None)
        if v is not None:
            v.release()
            self._verifier = None

    release_verifier = release


class ProofEncodingError(SerializationError):
    """A proof that ark-serialize or the verifier's range checks would refuse (MZK_ERR_ENCODING).  .index: the lowest bad proof of the batch;
    .field: the field of the `Proof` ("wires_poly_comms[2]", "wires_evals[0]", "length", ..); .reason: the library's text."""

    def __init__(self, reason: str, index: int, field: str | None, instance: int | None = None):
        ValueError.__init__(self, reason)
        self.index, self.field, self.reason = index, field, reason
        self.instance = instance                                       # of a BatchProof: the instance the field is in (m: the whole proof's)


_PROOF_MSG = re.compile(r"^proof (\d+): ([^:]+): ")
_BATCH_PROOF_MSG = re.compile(r"^(?:proof (\d+): )?instance (\d+): ([^:]+): ")
_LINK_MSG = re.compile(r"^link (\d+): ([^:]+): ")
_OPENING_MSG = re.compile(r"^opening (\d+): ([^:]+): ")


def _begin_arrays(proofs, flat_inputs, extra_msgs, challenges):
    """what a begin call takes: the K images back to back, the public inputs as canonical limbs (None without any), the extra messages as one
    blob with K (begin, end) ranges (None when no proof has one) and the challenges as (K, 7, 4)"""
    K = len(proofs)
    images = np.frombuffer(b"".join(bytes(p) for p in proofs), dtype=np.uint8)
    pub = np.frombuffer(b"".join(int(x).to_bytes(32, "little") for x in flat_inputs), dtype=np.uint64) if flat_inputs else None
    extra = ranges = None
    if extra_msgs is not None and any(m is not None for m in extra_msgs):
        blob, r = b"", []
        for m in extra_msgs:
            r += [2**64 - 1, 0] if m is None else [len(blob), len(blob) + len(m)]
            blob += b"" if m is None else bytes(m)
        extra, ranges = np.frombuffer(blob + b"\0", dtype=np.uint8), np.array(r, dtype=np.uint64)
    ch = None if challenges is None else np.ascontiguousarray(challenges, dtype=np.uint64).reshape(K, 7, 4)
    return images, pub, extra, ranges, ch


class Verifier:
    """mzk_verifier_*: the decoded commitments, k and the transcript script of one VerifyingKey on the device, h and beta_h on the host.
    begin() runs the per-proof stages of a group of proofs under this key and returns a VerifierBatch."""

    def __init__(self, vk, validate: bool = True):
        """vk: a VerifyingKey, or an OpenKey for a verifier of proof links alone"""
        L = _lib.ensure_init()
        self.vk, self.curve = vk, vk.curve
        flags = (_SER_COMPRESSED if vk.compressed else 0) | (_SER_VALIDATE if validate else 0)
        h = C.c_uint64()
        if isinstance(vk, OpenKey):
            recs = [np.frombuffer(b, dtype=np.uint8) for b in (vk.g, vk.h, vk.beta_h)]
            if [len(b) for b in recs] != [kzg.g1_record_bytes(vk.curve, vk.compressed)] + [kzg.g2_record_bytes(vk.curve, vk.compressed)] * 2:
                raise KeySerializationError("open_key: a record of the wrong length for this curve and mode", "open_key")
            rc = L.mzk_verifier_create_open_key(vk.curve.curve_id, *[C.c_void_p(b.ctypes.data) for b in recs], flags, C.byref(h))
        else:
            img = np.frombuffer(vk.serialize(), dtype=np.uint8)
            rc = L.mzk_verifier_create(vk.curve.curve_id, C.c_void_p(img.ctypes.data), img.shape[0], flags, C.byref(h))
        if rc == _ERR_ENCODING:
            _raise_encoding(L, None)
        _lib.check(rc, "mzk_verifier_create")
        self.handle = h.value
        np_, nkey, plen, nin = C.c_uint32(), C.c_uint32(), C.c_uint64(), C.c_uint64()
        _lib.check(L.mzk_verifier_shape(self.handle, C.byref(np_), C.byref(nkey), C.byref(plen), C.byref(nin)), "mzk_verifier_shape")
        self.n_proof_points, self.n_key_bases, self.proof_len, self.num_inputs = np_.value, nkey.value, plen.value, nin.value

    def begin(self, proofs, public_inputs, extra_msgs=None, challenges=None, validate: bool = True, transcript: str = "merlin") -> "VerifierBatch":
        """mzk_verifier_batch_begin.  proofs: K images (bytes); public_inputs: K lists of num_inputs canonical integers; extra_msgs: None or
        K entries, each bytes or None; challenges: None or (K, 7, 4) uint64 Montgomery (tau, beta, gamma, alpha, zeta, v, u) replacing the
        transcript; transcript: "merlin" | "solidity", the kind the device's Fiat-Shamir stage runs.  Raises ProofEncodingError naming the
        lowest bad proof."""
        L = _lib.load()
        kind = _transcript.flag(transcript)
        if isinstance(self.vk, OpenKey):
            raise ValueError("the verifier holds no verifying key")     # (mzk_verifier_batch_begin: MZK_ERR_INVALID_ARG with this text)
        K = len(proofs)
        if K == 0 or len(public_inputs) != K or (extra_msgs is not None and len(extra_msgs) != K):
            raise ValueError("the number of proofs / public inputs / extra messages differ, or no proof")
        for i, p in enumerate(proofs):                                 # (the ABI takes one length for the batch)
            if len(p) != self.proof_len:
                raise ProofEncodingError(f"proof {i}: length: {len(p)} bytes, expected {self.proof_len} under this key", i, "length")
        for pi in public_inputs:
            if len(pi) != self.num_inputs:
                raise ValueError("the circuit public input length != the verification key public input length")   # verifier.rs:99-108
        images, pub, extra, ranges, ch = _begin_arrays(proofs, [x for pi in public_inputs for x in pi], extra_msgs, challenges)
        ptr = lambda a: None if a is None else C.c_void_p(a.ctypes.data)
        batch, bad = C.c_uint64(), C.c_uint64()
        u = np.zeros((K, 4), dtype=np.uint64)
        rc = L.mzk_verifier_batch_begin(self.handle, ptr(images), self.proof_len, K, ptr(pub), ptr(extra), ptr(ranges), ptr(ch),
                                        (_SER_VALIDATE if validate else 0) | kind, C.byref(batch), ptr(u), C.byref(bad))
        if rc == _ERR_ENCODING:
            msg = L.mzk_last_error().decode()
            m = _PROOF_MSG.match(msg)
            raise ProofEncodingError(msg, bad.value, m.group(2) if m else None)
        _lib.check(rc, "mzk_verifier_batch_begin")
        return VerifierBatch(self, batch.value, K, u)

    def begin_links(self, links, eta=None, validate: bool = True, transcript: str = "merlin") -> "VerifierBatch":
        """mzk_verifier_link_begin.  links: K tuples (lhs_record, rhs_record, link_proof_bytes, layout) -- wires_poly_comms[0] of the two
        Plonk proofs (linking.linking_wire_record), the LinkingProof image (quotient_commitment || opening_proof) and a GroupLayout, records
        in this verifier's mode; eta: None or (K, 4) uint64 Montgomery replacing the transcript; transcript: "merlin" | "solidity".  Returns a VerifierBatch whose rows are (1, -1,
        -Z_D(eta), eta) over the four records and whose .u holds the K challenges eta.  Raises ProofEncodingError naming the lowest bad link
        (.index) and its field."""
        L = _lib.load()
        kind = _transcript.flag(transcript)
        K = len(links)
        if K == 0:
            raise ValueError("no link to verify")
        G = kzg.g1_record_bytes(self.curve, self.vk.compressed)
        for i, (lhs, rhs, link, _) in enumerate(links):
            for name, rec, want in (("lhs.wires_poly_comms[0]", lhs, G), ("rhs.wires_poly_comms[0]", rhs, G), ("length", link, 2 * G)):
                if len(rec) != want:
                    raise ProofEncodingError(f"link {i}: {name}: {len(rec)} bytes, expected {want} on this curve and in this mode", i, name)
        records = np.frombuffer(b"".join(bytes(lhs) + bytes(rhs) + bytes(link) for lhs, rhs, link, _ in links), dtype=np.uint8)
        layouts = np.array([[lay.alignment, lay.offset, lay.size] for _, _, _, lay in links], dtype=np.uint64)
        e = None if eta is None else np.ascontiguousarray(eta, dtype=np.uint64).reshape(K, 4)
        batch, bad = C.c_uint64(), C.c_uint64()
        out = np.zeros((K, 4), dtype=np.uint64)
        rc = L.mzk_verifier_link_begin(self.handle, C.c_void_p(records.ctypes.data), K, C.c_void_p(layouts.ctypes.data), None if e is None else C.c_void_p(e.ctypes.data),
                                       (_SER_VALIDATE if validate else 0) | kind, C.byref(batch), C.c_void_p(out.ctypes.data), C.byref(bad))
        if rc == _ERR_ENCODING:
            msg = L.mzk_last_error().decode()
            m = _LINK_MSG.match(msg)
            raise ProofEncodingError(msg, bad.value, m.group(2) if m else None)
        _lib.check(rc, "mzk_verifier_link_begin")
        return VerifierBatch(self, batch.value, K, out, shape=(1, 4))

    def begin_openings(self, commitments, points, values, proofs, validate: bool = True) -> "VerifierBatch":
        """mzk_verifier_open_begin: K KZG openings (univariate_kzg/mod.rs:195-271) as one batch.  commitments, proofs: kzg.Commitment objects
        (written as records of this verifier's mode) or G1 records, staged as they are; points, values: canonical integers, staged as they are
        -- the device range-checks them against r.  Returns a VerifierBatch whose rows are (1, z_i) over the two records, whose evaluations
        are the v_i and whose .u holds nothing; finish(weights) -> (A, B).  Raises ProofEncodingError naming the lowest bad opening (.index)
        and its field (commitment | proof | point | value)."""
        L = _lib.load()
        K = len(commitments)
        if K == 0 or len(points) != K or len(values) != K or len(proofs) != K:
            raise ValueError("the number of commitments / points / values / proofs differ, or no opening")
        G = kzg.g1_record_bytes(self.curve, self.vk.compressed)
        rec = lambda x: kzg.g1_record(self.curve, x, self.vk.compressed) if isinstance(x, kzg.Commitment) else bytes(x)
        pairs = [(rec(cm), rec(pf)) for cm, pf in zip(commitments, proofs)]
        for i, pair in enumerate(pairs):
            for name, r in zip(("commitment", "proof"), pair):
                if len(r) != G:
                    raise ProofEncodingError(f"opening {i}: {name}: {len(r)} bytes, expected {G} on this curve and in this mode", i, name)
        for name, xs in (("point", points), ("value", values)):
            for i, x in enumerate(xs):
                if not 0 <= int(x) < 1 << 256:
                    raise ProofEncodingError(f"opening {i}: {name}: not below the modulus", i, name)
        records = np.frombuffer(b"".join(cm + pf for cm, pf in pairs), dtype=np.uint8)
        limbs = lambda xs: np.frombuffer(b"".join(int(x).to_bytes(32, "little") for x in xs), dtype=np.uint64)
        z, v = limbs(points), limbs(values)
        batch, bad = C.c_uint64(), C.c_uint64()
        rc = L.mzk_verifier_open_begin(self.handle, C.c_void_p(records.ctypes.data), K, C.c_void_p(z.ctypes.data), C.c_void_p(v.ctypes.data),
                                       _SER_VALIDATE if validate else 0, C.byref(batch), C.byref(bad))
        if rc == _ERR_ENCODING:
            msg = L.mzk_last_error().decode()
            m = _OPENING_MSG.match(msg)
            raise ProofEncodingError(msg, bad.value, m.group(2) if m else None)
        _lib.check(rc, "mzk_verifier_open_begin")
        return VerifierBatch(self, batch.value, K, np.zeros((K, 4), dtype=np.uint64), shape=(1, 2))

    def check(self, A_xyz, B_xyz) -> bool:
        """mzk_verifier_check over the (A, B) of one or more groups with this key's open key: e(sum A, beta_h) e(-sum B, h) == 1."""
        A = np.ascontiguousarray(A_xyz, dtype=np.uint64).reshape(-1, 3, self.curve.fq_limbs)
        B = np.ascontiguousarray(B_xyz, dtype=np.uint64).reshape(-1, 3, self.curve.fq_limbs)
        assert A.shape == B.shape and A.shape[0] >= 1
        ok = C.c_int32()
        _lib.check(_lib.load().mzk_verifier_check(self.handle, C.c_void_p(A.ctypes.data), C.c_void_p(B.ctypes.data), A.shape[0], C.byref(ok)), "mzk_verifier_check")
        return bool(ok.value)

    def release(self):
        if self.handle:
            _lib.check(_lib.load().mzk_verifier_destroy(self.handle), "mzk_verifier_destroy")
            self.handle = 0


class VerifierBatch:
    """An open batch: .u (K, 4) Montgomery, challenges() / scalars() the stage outputs, finish(r_weights) -> (A, B) Jacobian; finish or
    discard consumes it."""

    def __init__(self, verifier: Verifier, handle: int, K: int, u: np.ndarray, shape=None):
        self.verifier, self.handle, self.K, self.u = verifier, handle, K, u
        self.n_key_bases, self.n_proof_points = shape or (verifier.n_key_bases, verifier.n_proof_points)   # (a link batch: 1, 4)

    def challenges(self) -> np.ndarray:
        out = np.zeros((self.K, 7, 4), dtype=np.uint64)
        _lib.check(_lib.load().mzk_verifier_batch_challenges(self.handle, C.c_void_p(out.ctypes.data)), "mzk_verifier_batch_challenges")
        return out

    def scalars(self):
        """(key_rows (K, NKEY, 4), proof_rows (K, NP, 4), evals (K, 4)), Montgomery, unweighted"""
        kr, pr, ev = np.zeros((self.K, self.n_key_bases, 4), np.uint64), np.zeros((self.K, self.n_proof_points, 4), np.uint64), np.zeros((self.K, 4), np.uint64)
        _lib.check(_lib.load().mzk_verifier_batch_scalars(self.handle, C.c_void_p(kr.ctypes.data), C.c_void_p(pr.ctypes.data), C.c_void_p(ev.ctypes.data)),
                   "mzk_verifier_batch_scalars")
        return kr, pr, ev

    def link_values(self):
        """mzk_verifier_link_values of a link batch: (eta (K, 4), Z_D(eta) (K, 4)), Montgomery"""
        eta, van = np.zeros((self.K, 4), np.uint64), np.zeros((self.K, 4), np.uint64)
        _lib.check(_lib.load().mzk_verifier_link_values(self.handle, C.c_void_p(eta.ctypes.data), C.c_void_p(van.ctypes.data)), "mzk_verifier_link_values")
        return eta, van

    def link_weights(self, r=None) -> np.ndarray:
        """mzk_verifier_link_weights: the (K, 4) Montgomery weights for finish().  r: None, or the (4,) Montgomery batch challenge of the Plonk
        groups this link batch is checked with.  One link and no r: exactly 1."""
        rm = None if r is None else np.ascontiguousarray(r, dtype=np.uint64).reshape(4)
        out = np.zeros((self.K, 4), np.uint64)
        _lib.check(_lib.load().mzk_verifier_link_weights(self.handle, None if rm is None else C.c_void_p(rm.ctypes.data), C.c_void_p(out.ctypes.data)),
                   "mzk_verifier_link_weights")
        return out

    def finish(self, r_weights_mont):
        L = self.verifier.curve.fq_limbs
        w = np.ascontiguousarray(r_weights_mont, dtype=np.uint64).reshape(self.K, 4)
        A, B = np.zeros((3, L), np.uint64), np.zeros((3, L), np.uint64)
        h, self.handle = self.handle, 0
        _lib.check(_lib.load().mzk_verifier_batch_finish(h, C.c_void_p(w.ctypes.data), C.c_void_p(A.ctypes.data), C.c_void_p(B.ctypes.data)), "mzk_verifier_batch_finish")
        return A, B

    def discard(self):
        if self.handle:
            h, self.handle = self.handle, 0
            _lib.check(_lib.load().mzk_verifier_batch_finish(h, None, None, None), "mzk_verifier_batch_finish")


def batch_proof_layout(curve, ultra: bool, m: int, compress: bool = True, image=None) -> _lib.BatchProofLayout:
    """mzk_batch_proof_layout: the length and the offset of every record of a BatchProof image of m instances.  Host-only.  With `image` its
    container (length, Vec counts, Option tags) is checked too: ProofEncodingError with .instance and .field."""
    c = _curve(curve)
    L = _lib.load()
    out = _lib.BatchProofLayout()
    buf = None if image is None else np.frombuffer(bytes(image) + b"\0", dtype=np.uint8)
    rc = L.mzk_batch_proof_layout(c.curve_id, int(bool(ultra)), m, _SER_COMPRESSED if compress else 0, None if buf is None else C.c_void_p(buf.ctypes.data),
                                  0 if buf is None else buf.shape[0] - 1, C.byref(out))
    if rc == _ERR_ENCODING:
        msg = L.mzk_last_error().decode()
        mt = _BATCH_PROOF_MSG.match(msg)
        raise ProofEncodingError(msg, 0, mt.group(3) if mt else None, int(mt.group(2)) if mt else None)
    _lib.check(rc, "mzk_batch_proof_layout")
    return out


class AggregateVerifier:
    """mzk_verifier_aggregate_*: `BatchProof`s of m instances under the tuple `vks` of m VerifyingKeys (one key may stand at several
    positions: a circuit and its forks).  begin() runs the per-proof stages of K BatchProofs and returns an ordinary VerifierBatch; the
    verifiers are the keys' own (VerifyingKey.verifier()), so release() has nothing of its own to free but the keys' verifiers on request."""

    def __init__(self, vks, validate: bool = True):
        vks = list(vks)
        if not vks:
            raise ValueError("the number of verification keys / instances / public inputs differ, or no key")           # verifier.rs:77-86
        open_key = (vks[0].g, vks[0].h, vks[0].beta_h, vks[0].compressed)
        for i, vk in enumerate(vks):
            if (vk.g, vk.h, vk.beta_h, vk.compressed) != open_key:
                raise ValueError("the verification keys have different open keys")                                      # snark.rs:160-166
            if vk.domain_size != vks[0].domain_size:
                raise ValueError("the domain size of the %d-th verification key is different" % i)                      # verifier.rs:88-97
        self.vks, self.curve, self.m = vks, vks[0].curve, len(vks)
        self.verifiers = [vk.verifier(validate) for vk in vks]
        self.handles = (C.c_uint64 * self.m)(*[v.handle for v in self.verifiers])
        np_, nkey, plen, nin = C.c_uint32(), C.c_uint32(), C.c_uint64(), C.c_uint64()
        _lib.check(_lib.load().mzk_verifier_aggregate_shape(self.handles, self.m, C.byref(np_), C.byref(nkey), C.byref(plen), C.byref(nin)),
                   "mzk_verifier_aggregate_shape")
        self.n_proof_points, self.n_key_bases, self.proof_len, self.num_inputs = np_.value, nkey.value, plen.value, nin.value

    @property
    def shape(self):
        """(points per BatchProof, key bases of the tuple, image length, public inputs per proof)"""
        return self.n_proof_points, self.n_key_bases, self.proof_len, self.num_inputs

    def begin(self, batch_proofs, public_inputs, extra_msgs=None, challenges=None, validate: bool = True, transcript: str = "merlin") -> "VerifierBatch":
        """mzk_verifier_aggregate_begin.  batch_proofs: K images; public_inputs: per proof a list of m lists of canonical integers, in tuple
        order; extra_msgs / challenges / transcript as for Verifier.begin.  Raises ProofEncodingError naming the lowest bad proof, its lowest instance
        (.instance; m: the whole proof's) and the field."""
        L = _lib.load()
        kind = _transcript.flag(transcript)
        K = len(batch_proofs)
        if K == 0 or len(public_inputs) != K or (extra_msgs is not None and len(extra_msgs) != K):
            raise ValueError("the number of proofs / public inputs / extra messages differ, or no proof")
        for i, p in enumerate(batch_proofs):
            if len(p) != self.proof_len:
                raise ProofEncodingError(f"proof {i}: instance {self.m}: length: {len(p)} bytes, expected {self.proof_len} under these keys", i, "length", self.m)
        for pubs in public_inputs:
            if len(pubs) != self.m:
                raise ValueError("the number of verification keys / instances / public inputs differ")                  # verifier.rs:77-86
            for j, (pi, vk) in enumerate(zip(pubs, self.vks)):
                if len(pi) != vk.num_inputs:
                    raise ValueError("the circuit public input length != the %d-th verification key public input length" % j)   # verifier.rs:99-108
        images, pub, extra, ranges, ch = _begin_arrays(batch_proofs, [x for pubs in public_inputs for pi in pubs for x in pi], extra_msgs, challenges)
        ptr = lambda a: None if a is None else C.c_void_p(a.ctypes.data)
        batch, bad = C.c_uint64(), C.c_uint64()
        u = np.zeros((K, 4), dtype=np.uint64)
        rc = L.mzk_verifier_aggregate_begin(self.handles, self.m, ptr(images), self.proof_len, K, ptr(pub), ptr(extra), ptr(ranges), ptr(ch),
                                            (_SER_VALIDATE if validate else 0) | kind, C.byref(batch), ptr(u), C.byref(bad))
        if rc == _ERR_ENCODING:
            msg = L.mzk_last_error().decode()
            mt = _BATCH_PROOF_MSG.match(msg)
            raise ProofEncodingError(msg, bad.value, mt.group(3) if mt else None, int(mt.group(2)) if mt else None)
        _lib.check(rc, "mzk_verifier_aggregate_begin")
        return VerifierBatch(self, batch.value, K, u)

    def check(self, A_xyz, B_xyz) -> bool:
        """mzk_verifier_check with the tuple's open key (any group under the same open key may be among the summands)"""
        return self.verifiers[0].check(A_xyz, B_xyz)

    def release(self):
        """frees the verifiers of the tuple's keys (VerifyingKey.release_verifier of each)"""
        for vk in self.vks:
            vk.release_verifier()
        self.verifiers = []


class ProvingKey:
    """A loaded `ProvingKey<E>`: .prover (a TurboPlonkProver whose coefficient forms were decoded on the device), .vk (VerifyingKey) and
    the SRS handles this object owns (.commit_key unless one was passed in, .lagrange_key when asked for).  release() frees the prover,
    then the keys it owns."""

    def __init__(self, prover, vk: VerifyingKey, owned):
        self.prover, self.vk, self._owned = prover, vk, list(owned)

    @classmethod
    def deserialize(cls, curve, data, compress: bool = True, validate: bool = True, check_commitments: bool = False,
                    commit_key: kzg.UnivariateProverParam | None = None, lagrange: bool = False) -> "ProvingKey":
        """mzk_prover_create_serialized.  compress / validate as for the SRS (they select ark's deserialize_* variant; validate applies
        to the commit key's points); check_commitments: the commitments in vk must commit the key's polynomials and vk.open_key.g must
        be commit-key point 0.  commit_key: an SRS already on the device -- the embedded points are then skipped, not compared, and one
        SRS with its fixed-base table serves many keys.  lagrange: also derive the Lagrange-basis key (round 1 commits wire values).
        Raises KeySerializationError with .field and .index."""
        from .prover import TurboPlonkProver
        c = _curve(curve)
        buf = kzg._as_bytes(data)
        if kzg._is_torch(buf):
            raise ValueError("a key image is read from host memory")
        lay = key_layout(c, buf, compress)
        L = _lib.ensure_init()
        flags = (_SER_COMPRESSED if compress else 0) | (_SER_VALIDATE if validate else 0) | (_KEY_CHECK_COMMITMENTS if check_commitments else 0)
        assert commit_key is None or commit_key.offset == 0
        h, ck, lk, bad = C.c_uint64(), C.c_uint64(), C.c_uint64(), C.c_uint64()
        rc = L.mzk_prover_create_serialized(c.curve_id, C.c_void_p(buf.ctypes.data), buf.shape[0], flags, commit_key.handle if commit_key is not None else 0, None,
                                            C.byref(h), C.byref(ck), C.byref(lk) if lagrange else None, C.byref(bad))
        if rc == _ERR_ENCODING:
            _raise_encoding(L, bad.value)
        _lib.check(rc, "mzk_prover_create_serialized")
        n, W = lay.domain_size, lay.num_wire_types
        vk = VerifyingKey._from_layout(c, buf, lay, compress)
        own_ck = kzg.UnivariateProverParam(c, ck.value, lay.commit_key_count) if commit_key is None else None
        own_lk = kzg.UnivariateProverParam(c, lk.value, n + 3) if lagrange else None
        p = TurboPlonkProver.__new__(TurboPlonkProver)
        p._describe(c, n, vk.k, own_ck if commit_key is None else commit_key, own_lk, W, lay.num_selectors)
        p._adopt(h.value, None)
        return cls(p, vk, [k for k in (own_lk, own_ck) if k is not None])

    @property
    def commit_key(self):
        return self.prover.ck

    @property
    def lagrange_key(self):
        return self.prover.lagrange_ck

    def serialize(self, compress: bool | None = None) -> bytes:
        """The image again, from the resident key (TurboPlonkProver.serialize_key with this key's vk fields)."""
        compress = self.vk.compressed if compress is None else compress
        assert compress == self.vk.compressed, "the G2 elements are held as bytes of the mode they were read in"
        return self.prover.serialize_key(self.vk.num_inputs, self.vk.h, self.vk.beta_h, self.vk.is_merged, compress)

    def release(self):
        self.prover.release()
        for k in self._owned:
            k.release()
        self._owned = []
