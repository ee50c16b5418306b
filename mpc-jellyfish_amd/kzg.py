"""UnivariateKzgPCS -- mirror of primitives/src/pcs/univariate_kzg/{mod,srs}.rs: commit, open and verify, single and batched:

    UnivariateProverParam{powers_of_g}      srs.rs:36-40   -> an SRS resident in HBM (handle)
    gen_srs_for_testing                     srs.rs:118-153 -> UnivariateProverParam.gen_srs_for_testing
    trim                                    srs.rs:77-93   -> UnivariateProverParam.trim
    commit / batch_commit                   mod.rs:90-131  -> UnivariateKzgPCS.commit / batch_commit
    <G1 as VariableBaseMSM>::msm_bigint     mod.rs:109-111 -> msm_bigint
    open / batch_open                       mod.rs:135-190 -> UnivariateKzgPCS.open / batch_open (one pass: mzk_kzg_open_batch_dev)
    verify / batch_verify                   mod.rs:195-271 -> UnivariateKzgPCS.verify / batch_verify (keys.OpenKey.begin_openings)
    multi_open_rou[_proofs|_evals], multi_open_rou_eval_domain, trim_fft_size, checked_fft_size
                                            mod.rs:298-377, pcs/mod.rs:236-322 -> UnivariateKzgPCS.multi_open_rou .. (FK23: mzk_kzg_multi_open_rou_dev)
    UnivariateVerifierParam, trim's 2nd half srs.rs:48-55, 77-93 -> keys.OpenKey, UnivariateUniversalParams.verifier_param
    CanonicalSerialize / Deserialize        srs.rs:18-40   -> UnivariateProverParam.serialize / deserialize,
                                                              UnivariateUniversalParams (points decoded on the GPU)

Polynomials are (len,4) uint64 Montgomery coefficient arrays, low order first (DensePolynomial);
commitments are affine points x||y (Montgomery limbs), (0,0) = infinity.  Error behaviour follows
the reference: commit raises PCSError (InvalidParameters) when the degree exceeds the key.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import lib as _lib
from .params import CurveParams, curve as _curve, fq_from_mont, fq_to_mont, fr_from_mont, fr_to_mont, int_to_limbs


class PCSError(Exception):
    """primitives/src/pcs/errors.rs:16-33 (InvalidParameters is the only variant raised here)."""


class SerializationError(ValueError):
    """A serialized setup that ark-serialize would refuse, or that holds a point at infinity (include/mzk.h, MZK_ERR_ENCODING).
    .index: the lowest failing point (None for container errors); .reason: what failed."""

    def __init__(self, reason: str, index: int | None = None):
        super().__init__(reason if index is None else f"point {index}: {reason}")
        self.index, self.reason = index, reason


_SER_COMPRESSED, _SER_VALIDATE = 1, 2
_ERR_ENCODING = -11


def g1_record_bytes(curve, compress: bool = True) -> int:
    """Bytes of one G1 point in ark-serialize 0.4: 48 / 96 on BLS12-381, 32 / 64 on BN254 (compressed / uncompressed)."""
    return (48 if _curve(curve).curve_id == 0 else 32) * (1 if compress else 2)


def g1_record(curve, commitment, compress: bool = True) -> bytes:
    """A Commitment as the G1 record ark-serialize writes (transcript.g1_bytes for the compressed form; uncompressed: x || y, BLS12-381
    big-endian, BN254 little-endian with y's sign flag in the last byte; infinity: the flag byte alone)."""
    from . import transcript as _transcript
    c = _curve(curve)
    pt = None if commitment.is_infinity() else tuple(fq_from_mont(c, commitment.xy))
    if compress:
        return _transcript.g1_bytes(c, pt)
    n = g1_record_bytes(c)
    if pt is None:
        rec = bytearray(2 * n)
        rec[0 if c.curve_id == 0 else -1] |= 0x40
        return bytes(rec)
    x, y = pt
    if c.curve_id == 0:
        return x.to_bytes(n, "big") + y.to_bytes(n, "big")
    rec = bytearray(x.to_bytes(n, "little") + y.to_bytes(n, "little"))
    rec[-1] |= 0x80 if y > c.q - y else 0
    return bytes(rec)


def g2_record_bytes(curve, compress: bool = True) -> int:
    """Bytes of one G2 point: 96 / 192 on BLS12-381, 64 / 128 on BN254."""
    return 2 * g1_record_bytes(curve, compress)


def _as_bytes(data):
    """Any host buffer (bytes, bytearray, memoryview, numpy uint8 incl. np.memmap) as a flat uint8 array, without a copy where possible;
    a CUDA uint8 tensor is returned as is."""
    if _is_torch(data):
        import torch
        if data.dtype != torch.uint8 or not data.is_cuda or data.dim() != 1 or not data.is_contiguous():
            raise ValueError("expected a contiguous 1-D uint8 CUDA tensor")
        return data
    a = data if isinstance(data, np.ndarray) else np.frombuffer(memoryview(data).cast("B"), dtype=np.uint8)
    if a.dtype != np.uint8:
        raise ValueError("expected uint8 data")
    return np.ascontiguousarray(a.reshape(-1))


def _vec_header(buf, rec: int, what: str) -> tuple[int, int]:
    """(count, bytes of the Vec<G1Affine> image) from its u64 LE length prefix; raises SerializationError on a short buffer."""
    total = buf.shape[0]
    if total < 8:
        raise SerializationError(f"{what}: {total} bytes, shorter than the 8-byte length prefix")
    head = buf[:8].cpu().numpy() if _is_torch(buf) else buf[:8]
    count = int.from_bytes(bytes(head), "little")
    if count > (total - 8) // rec:
        raise SerializationError(f"{what}: the prefix counts {count} points, the data holds {(total - 8) // rec} ({total} bytes)")
    return count, 8 + count * rec


class Commitment:
    """pcs/structs.rs:16-19: a G1 affine point; .xy is (2, fq_limbs) uint64 Montgomery."""

    def __init__(self, curve: CurveParams, xy: np.ndarray):
        self.curve = curve
        self.xy = np.ascontiguousarray(xy, dtype=np.uint64).reshape(2, curve.fq_limbs)

    def is_infinity(self) -> bool:
        return not self.xy.any()

    def __eq__(self, other):
        return isinstance(other, Commitment) and self.curve is other.curve and np.array_equal(self.xy, other.xy)

    def __repr__(self):
        return f"Commitment({self.curve.name}, x[0]=0x{int(self.xy[0, 0]):016x})"


class UnivariateProverParam:
    """powers_of_g held on the GPU.  `offset`/`length` give a trimmed view of one registration."""

    def __init__(self, curve: CurveParams, handle: int, length: int, offset: int = 0, owner: bool = True):
        self.curve, self.handle, self.length, self.offset, self._owner = curve, handle, length, offset, owner

    @classmethod
    def from_affine(cls, curve, powers_of_g: np.ndarray) -> "UnivariateProverParam":
        c = _curve(curve)
        a = np.ascontiguousarray(powers_of_g, dtype=np.uint64).reshape(-1, 2, c.fq_limbs)
        L = _lib.ensure_init()
        h = C.c_uint64()
        _lib.check(L.mzk_srs_register(c.curve_id, C.c_void_p(a.ctypes.data), a.shape[0], C.byref(h)), "mzk_srs_register")
        return cls(c, h.value, a.shape[0])

    @classmethod
    def gen_srs_for_testing(cls, curve, beta: int, max_degree: int, g=None) -> "UnivariateProverParam":
        """powers_of_g = [beta^i * g] for i <= max_degree (srs.rs:118-153), built on the GPU.  g: affine base point as canonical
        integers (x, y) -- `universal_setup_for_testing` draws it with G1::rand after beta (snark.rs:495-497); None: the curve's
        standard generator."""
        c = _curve(curve)
        L = _lib.ensure_init()
        h = C.c_uint64()
        b = int_to_limbs(beta % c.r, 4)
        gm = None if g is None else np.ascontiguousarray(np.concatenate([fq_to_mont(c, [g[0]])[0], fq_to_mont(c, [g[1]])[0]]))
        _lib.check(L.mzk_srs_generate_for_testing_g(c.curve_id, C.c_void_p(b.ctypes.data), None if gm is None else C.c_void_p(gm.ctypes.data),
                                                    max_degree + 1, C.byref(h)), "mzk_srs_generate_for_testing_g")
        return cls(c, h.value, max_degree + 1)

    @classmethod
    def gen_lagrange_srs_for_testing(cls, curve, beta: int, domain_size: int, n_extra: int = 3, g=None) -> "UnivariateProverParam":
        """The testing SRS over the Lagrange basis of the gate domain H (|H| = domain_size): point i = L_i(beta) g, then n_extra points
        beta^j (beta^n - 1) g (include/mzk.h, mzk_srs_generate_lagrange_for_testing).  An MSM of (values on H, blinders) over it equals
        the commitment of the masked coefficient form over gen_srs_for_testing(beta, ..., g) -- round 1 commits the wires this way
        (TurboPlonkProver.lagrange_ck): witness values are mostly small numbers, whose high digits cost the MSM nothing."""
        c = _curve(curve)
        assert domain_size & (domain_size - 1) == 0
        L = _lib.ensure_init()
        h = C.c_uint64()
        b = int_to_limbs(beta % c.r, 4)
        gm = None if g is None else np.ascontiguousarray(np.concatenate([fq_to_mont(c, [g[0]])[0], fq_to_mont(c, [g[1]])[0]]))
        _lib.check(L.mzk_srs_generate_lagrange_for_testing(c.curve_id, C.c_void_p(b.ctypes.data), None if gm is None else C.c_void_p(gm.ctypes.data),
                                                           domain_size.bit_length() - 1, n_extra, C.byref(h)), "mzk_srs_generate_lagrange_for_testing")
        return cls(c, h.value, domain_size + n_extra)

    def lagrange_key(self, domain_size: int, n_extra: int = 3) -> "UnivariateProverParam":
        """The Lagrange-basis key of THIS SRS for the gate domain of `domain_size` points, without the trapdoor: the inverse group-NTT of
        its first domain_size points (mzk_srs_lagrange_from_srs; 0.14 s at 2^16, 1.2 s at 2^20 on BLS12-381: a one-off per SRS and domain)."""
        assert domain_size & (domain_size - 1) == 0 and self.offset == 0 and self.length >= domain_size + n_extra
        h = C.c_uint64()
        _lib.check(_lib.ensure_init().mzk_srs_lagrange_from_srs(self.handle, domain_size.bit_length() - 1, n_extra, C.byref(h)), "mzk_srs_lagrange_from_srs")
        return UnivariateProverParam(self.curve, h.value, domain_size + n_extra)

    def slice(self, first: int, count: int) -> "UnivariateProverParam":
        """A NEW registration holding the points [first, first + count) of this one (mzk_srs_slice): what a rank of a multi-GPU prover keeps
        of the commit key -- its own fixed-base table, 1 / G of the size, built with the window that suits the slice."""
        assert 0 <= first and first + count <= self.length
        h = C.c_uint64()
        _lib.check(_lib.ensure_init().mzk_srs_slice(self.handle, self.offset + first, count, C.byref(h)), "mzk_srs_slice")
        return UnivariateProverParam(self.curve, h.value, count)

    def trim(self, supported_degree: int) -> "UnivariateProverParam":
        """srs.rs:77-93: keep powers_of_g[..=supported_degree]."""
        if supported_degree + 1 > self.length:
            raise PCSError("InvalidParameters: supported degree larger than the SRS")
        return UnivariateProverParam(self.curve, self.handle, supported_degree + 1, self.offset, owner=False)

    @classmethod
    def deserialize(cls, curve, data, compress: bool = True, validate: bool = True) -> "UnivariateProverParam":
        """The CanonicalDeserialize image of `UnivariateProverParam` (a Vec<G1Affine>: u64 LE count, then the points; srs.rs:36-40) ->
        a key on the GPU, decoded and checked there (mzk_srs_register_serialized).  compress / validate select ark's
        deserialize_{compressed,uncompressed}[_unchecked]; unlike ark a point at infinity is always refused.  data: bytes, memoryview,
        a numpy uint8 array (np.memmap of a file included), or a 1-D uint8 CUDA tensor (decoded in place on the current stream).
        Raises SerializationError (container length before any device call; a bad point with its lowest index and reason)."""
        c = _curve(curve)
        buf = _as_bytes(data)
        count, used = _vec_header(buf, g1_record_bytes(c, compress), "UnivariateProverParam")
        if used != buf.shape[0]:
            raise SerializationError(f"UnivariateProverParam: {buf.shape[0] - used} trailing bytes after {count} points")
        return cls._register_records(c, buf, 8, count, compress, validate)

    @classmethod
    def _register_records(cls, c, buf, offset: int, count: int, compress: bool, validate: bool) -> "UnivariateProverParam":
        L = _lib.ensure_init()
        h, bad = C.c_uint64(), C.c_uint64()
        flags = (_SER_COMPRESSED if compress else 0) | (_SER_VALIDATE if validate else 0)
        if _is_torch(buf):
            import torch
            st = torch.cuda.current_stream(buf.device).cuda_stream
            rc = L.mzk_srs_register_serialized_dev(c.curve_id, C.c_void_p(buf.data_ptr() + offset), count, flags, C.byref(h), C.byref(bad),
                                                   C.c_void_p(st))
        else:
            rc = L.mzk_srs_register_serialized(c.curve_id, C.c_void_p(buf.ctypes.data + offset) if count else None, count, flags, C.byref(h),
                                               C.byref(bad))
        if rc == _ERR_ENCODING:
            msg = L.mzk_last_error().decode()
            raise SerializationError(msg.split(": ", 1)[1] if ": " in msg else msg, bad.value)
        _lib.check(rc, "mzk_srs_register_serialized")
        return cls(c, h.value, count)

    def serialize(self, compress: bool = True) -> bytes:
        """CanonicalSerialize of this key (a trimmed view: its own `length` points from `offset`), encoded on the GPU."""
        rec = g1_record_bytes(self.curve, compress)
        out = np.empty(8 + self.length * rec, dtype=np.uint8)
        out[:8] = np.frombuffer(self.length.to_bytes(8, "little"), dtype=np.uint8)
        if self.length:
            _lib.check(_lib.ensure_init().mzk_srs_serialize(self.handle, self.offset, self.length, _SER_COMPRESSED if compress else 0,
                                                            C.c_void_p(out.ctypes.data + 8)), "mzk_srs_serialize")
        return out.tobytes()

    def powers_of_g(self, first: int = 0, count: int | None = None) -> np.ndarray:
        count = self.length - first if count is None else count
        out = np.empty((count, 2, self.curve.fq_limbs), dtype=np.uint64)
        _lib.check(_lib.ensure_init().mzk_srs_download(self.handle, self.offset + first, count, C.c_void_p(out.ctypes.data)),
                   "mzk_srs_download")
        return out

    def release(self):
        if self._owner and self.handle:
            _lib.check(_lib.load().mzk_srs_release(self.handle), "mzk_srs_release")
            self.handle = 0


class UnivariateUniversalParams:
    """srs.rs:18-27: powers_of_g (a UnivariateProverParam on the GPU), then h and beta_h (G2).  The G2 elements are kept as the bytes they
    were read as -- only their length is checked; the prover never reads them, and decoding or validating G2 is not done here.
    `compressed`: the mode the container was read in, and the one serialize() writes back."""

    def __init__(self, powers_of_g: UnivariateProverParam, h: bytes, beta_h: bytes, compressed: bool = True):
        self.powers_of_g, self.h, self.beta_h, self.compressed = powers_of_g, bytes(h), bytes(beta_h), compressed
        g2 = g2_record_bytes(powers_of_g.curve, compressed)
        if len(self.h) != g2 or len(self.beta_h) != g2:
            raise SerializationError(f"UnivariateUniversalParams: G2 elements are {g2} bytes in this mode")

    @classmethod
    def deserialize(cls, curve, data, compress: bool = True, validate: bool = True) -> "UnivariateUniversalParams":
        """CanonicalDeserialize of the whole setup (derive order: powers_of_g, h, beta_h).  The points are decoded as by
        UnivariateProverParam.deserialize; h and beta_h are length-checked and kept as bytes.  Container length errors (truncation,
        trailing bytes, a count that does not fit) raise SerializationError before any device call."""
        c = _curve(curve)
        buf = _as_bytes(data)
        count, used = _vec_header(buf, g1_record_bytes(c, compress), "UnivariateUniversalParams")
        g2 = g2_record_bytes(c, compress)
        if buf.shape[0] != used + 2 * g2:
            raise SerializationError(f"UnivariateUniversalParams: {buf.shape[0]} bytes, expected {used + 2 * g2} for {count} points")
        tail = buf[used:]
        tail = bytes(tail.cpu().numpy()) if _is_torch(tail) else bytes(tail)
        pp = UnivariateProverParam._register_records(c, buf, 8, count, compress, validate)
        return cls(pp, tail[:g2], tail[g2:], compress)

    def serialize(self) -> bytes:
        return self.powers_of_g.serialize(self.compressed) + self.h + self.beta_h

    def verifier_param(self):
        """The second half of `trim` (srs.rs:77-93): UnivariateVerifierParam { g: powers_of_g[0], h, beta_h } as a keys.OpenKey of this
        container's mode -- what UnivariateKzgPCS.verify / batch_verify take."""
        from . import keys as _keys
        g = g1_record(self.powers_of_g.curve, Commitment(self.powers_of_g.curve, self.powers_of_g.powers_of_g(0, 1)[0]), self.compressed)
        return _keys.OpenKey(self.powers_of_g.curve, g, self.h, self.beta_h, self.compressed)

    def release(self):
        self.powers_of_g.release()


def _is_torch(x) -> bool:
    return type(x).__module__.startswith("torch")


def _degree_and_leading_zeros(coeffs: np.ndarray):
    """(degree, num_leading_zeros) of a coefficient array; degree of the zero polynomial is 0."""
    nz = np.flatnonzero(coeffs.any(axis=1))
    if nz.size == 0:
        return 0, coeffs.shape[0]
    return int(nz[-1]), int(nz[0])


def _next_power_of_two(n: int) -> int:
    """usize::next_power_of_two: 1 for 0"""
    return 1 if n <= 1 else 1 << (n - 1).bit_length()


def checked_fft_size(degree: int) -> int:
    """pcs/mod.rs:308-322: the FFT size (`num_coeffs`) for a degree -- twice a power of two, else the next power of two; PCSError where
    usize overflows."""
    size = 2 * degree if degree > 0 and degree & (degree - 1) == 0 else _next_power_of_two(degree)
    if degree < 0 or size >= 1 << 64:
        raise PCSError(f"InvalidParameters: Next power of two overflows! Got: {degree}")
    return size


def msm_bigint(pp: UnivariateProverParam, bigints, base_offset: int = 0, scalars_are_mont: bool = False) -> np.ndarray:
    """sum_i bigints[i] * powers_of_g[base_offset + i] as a Jacobian point (3, fq_limbs), Montgomery.
    Uses min(len) of the two sides like ark-ec.  bigints: (n,4) uint64 host array or int64 CUDA tensor."""
    L = _lib.ensure_init()
    out = np.empty((3, pp.curve.fq_limbs), dtype=np.uint64)
    avail = max(0, pp.length - base_offset)
    if _is_torch(bigints):
        import torch
        if bigints.dtype != torch.int64 or not bigints.is_cuda or not bigints.is_contiguous() or bigints.shape[-1] != 4:
            raise ValueError("expected a contiguous int64 CUDA tensor of shape (n, 4)")
        n = min(bigints.shape[0], avail)
        st = torch.cuda.current_stream(bigints.device).cuda_stream
        _lib.check(L.mzk_msm_dev(pp.handle, pp.offset + base_offset, bigints.data_ptr(), n, int(scalars_are_mont),
                                 C.c_void_p(out.ctypes.data), st), "mzk_msm_dev")
        return out
    s = np.ascontiguousarray(bigints, dtype=np.uint64).reshape(-1, 4)
    n = min(s.shape[0], avail)
    _lib.check(L.mzk_msm(pp.handle, pp.offset + base_offset, C.c_void_p(s.ctypes.data), n, int(scalars_are_mont),
                         C.c_void_p(out.ctypes.data)), "mzk_msm")
    return out


class UnivariateKzgPCS:
    @staticmethod
    def commit(prover_param: UnivariateProverParam, poly) -> Commitment:
        """mod.rs:90-116: degree guard, skip low-order zero coefficients, MSM, into_affine.
        poly: (len, 4) Montgomery coefficients, host array or CUDA tensor."""
        pp = prover_param
        if _is_torch(poly) and poly.is_cuda and 0 < poly.shape[0] <= pp.length:
            # device-resident coefficients that fit the key: zero coefficients contribute nothing to the MSM, so skipping the
            # leading ones (mod.rs:106) needs no host copy
            jac = msm_bigint(pp, poly.contiguous(), 0, scalars_are_mont=True)
            return Commitment(pp.curve, jacobian_to_affine(pp.curve, jac[None])[0])
        if _is_torch(poly):
            poly = poly.cpu().numpy().view(np.uint64)
        coeffs = np.ascontiguousarray(poly, dtype=np.uint64).reshape(-1, 4)
        degree, lead = _degree_and_leading_zeros(coeffs)
        if degree > pp.length:                                             # mod.rs:98
            raise PCSError(f"InvalidParameters: poly degree {degree} is larger than allowed {pp.length}")
        body = coeffs[lead:degree + 1] if lead <= degree else coeffs[:0]
        if lead + body.shape[0] > pp.length:
            # degree == powers_of_g.len(): passes the reference's guard, then ark-ec truncates to min(len)
            body = body[:pp.length - lead]
        if not body.size:
            lead = 0                                                       # the zero polynomial (ark-poly keeps no coefficients for it)
        L = _lib.ensure_init()
        out = np.empty((2, pp.curve.fq_limbs), dtype=np.uint64)
        _lib.check(L.mzk_msm_affine(pp.handle, pp.offset + lead, C.c_void_p(body.ctypes.data) if body.size else None,
                                    body.shape[0], 1, C.c_void_p(out.ctypes.data)), "mzk_msm_affine")
        return Commitment(pp.curve, out)

    @staticmethod
    def batch_commit(prover_param: UnivariateProverParam, polys) -> list[Commitment]:
        """mod.rs:119-131.  The reference maps `commit` over the polynomials on Rayon workers; here
        the MSMs run back to back on the GPU and share one bucket-reduction phase (mzk_msm_batch)."""
        pp = prover_param
        bodies, offs = [], []
        for poly in polys:
            coeffs = np.ascontiguousarray(poly, dtype=np.uint64).reshape(-1, 4)
            degree, lead = _degree_and_leading_zeros(coeffs)
            if degree > pp.length:
                raise PCSError(f"InvalidParameters: poly degree {degree} is larger than allowed {pp.length}")
            body = coeffs[lead:degree + 1] if lead <= degree else coeffs[:0]
            if lead + body.shape[0] > pp.length:
                body = body[:pp.length - lead]
            bodies.append(np.ascontiguousarray(body))
            offs.append(pp.offset + lead)
        jac = msm_bigint_batch(pp, bodies, offs, scalars_are_mont=True, absolute_offsets=True)
        xy = jacobian_to_affine(pp.curve, jac)
        return [Commitment(pp.curve, xy[i]) for i in range(len(bodies))]


    @staticmethod
    def open(prover_param: UnivariateProverParam, polynomial, point: int):
        """mod.rs:135-161: witness polynomial p(X) / (X - point) (remainder dropped), its commitment, and p(point).
        polynomial: (len, 4) Montgomery coefficients, numpy or CUDA tensor.  Returns (Commitment proof, evaluation int)."""
        import torch
        from . import poly as _poly
        pp = prover_param
        t = polynomial if _is_torch(polynomial) else torch.from_numpy(np.ascontiguousarray(polynomial, dtype=np.uint64).reshape(-1, 4).view(np.int64)).cuda()
        t = t.contiguous()
        if t.shape[0] == 0:
            return Commitment(pp.curve, np.zeros((2, pp.curve.fq_limbs), dtype=np.uint64)), 0
        ev = _poly.evaluate(pp.curve, t, point)[0]
        if t.shape[0] == 1:                                                # constant polynomial: zero witness
            return Commitment(pp.curve, np.zeros((2, pp.curve.fq_limbs), dtype=np.uint64)), ev
        witness = _poly.div_by_linear(pp.curve, t, point)
        proof = UnivariateKzgPCS.commit(pp, witness)
        return proof, ev

    @staticmethod
    def batch_open(prover_param: UnivariateProverParam, polynomials, points):
        """mod.rs:163-190 ("a naive approach" there: a loop over open): every polynomial opened at its own point in ONE pass of the device
        (mzk_kzg_open_batch_dev) -- the K witness polynomials and evaluations from one kernel family, the K commitments from one fused batch
        MSM, which waits once per group of six and not twice per polynomial.  polynomials: (len, 4) Montgomery coefficient arrays (numpy or CUDA tensors, ragged); host arrays are staged in one
        upload.  Returns ([Commitment proofs], [evaluation ints]) as the loop over open did."""
        if len(polynomials) != len(points):
            raise PCSError("InvalidParameters: poly length %d is different from points length %d" % (len(polynomials), len(points)))
        pp = prover_param
        K = len(polynomials)
        if K == 0:
            return [], []
        import torch
        polys, one_by_one = [], bool(pp.offset)                            # (a view that does not start at its registration's first point: the loop)
        for p in polynomials:
            if _is_torch(p) and p.shape[0] - 1 <= pp.length:
                polys.append(p)
                continue
            a = p.cpu().numpy().view(np.uint64) if _is_torch(p) else np.ascontiguousarray(p, dtype=np.uint64)
            a = a.reshape(-1, 4)
            if a.shape[0] - 1 > pp.length:                                 # the witness array is longer than the key: its true degree decides (mod.rs:98)
                degree, _ = _degree_and_leading_zeros(a)
                if degree - 1 > pp.length:
                    raise PCSError(f"InvalidParameters: poly degree {degree - 1} is larger than allowed {pp.length}")
                one_by_one |= degree - 1 == pp.length                      # passes the reference's guard, then ark-ec truncates: commit's own edge
                a = a[:degree + 1]
            polys.append(a)
        if one_by_one:
            out = [UnivariateKzgPCS.open(pp, p, z) for p, z in zip(polynomials, points)]
            return [o[0] for o in out], [o[1] for o in out]
        host = [i for i, p in enumerate(polys) if not _is_torch(p)]
        if host:                                                           # one slab, one upload
            slab = torch.from_numpy(np.concatenate([polys[i] for i in host]).view(np.int64)).cuda()
            at = 0
            for i in host:
                n = polys[i].shape[0]
                polys[i] = slab[at:at + n]
                at += n
        polys = [p.contiguous() for p in polys]
        for p in polys:
            if p.dtype != torch.int64 or not p.is_cuda or p.dim() != 2 or p.shape[1] != 4:
                raise ValueError("expected (len, 4) int64 CUDA tensors or uint64 host arrays")
        c = pp.curve
        ptrs = (C.c_void_p * K)(*[p.data_ptr() if p.shape[0] else None for p in polys])
        lens = (C.c_uint64 * K)(*[p.shape[0] for p in polys])
        z = fr_to_mont(c, [int(x) % c.r for x in points])
        proofs, evals = np.zeros((K, 2, c.fq_limbs), dtype=np.uint64), np.zeros((K, 4), dtype=np.uint64)
        st = torch.cuda.current_stream(polys[0].device).cuda_stream
        _lib.check(_lib.ensure_init().mzk_kzg_open_batch_dev(pp.handle, K, ptrs, lens, C.c_void_p(z.ctypes.data), C.c_void_p(proofs.ctypes.data),
                                                             C.c_void_p(evals.ctypes.data), C.c_void_p(st)), "mzk_kzg_open_batch_dev")
        return [Commitment(c, proofs[i]) for i in range(K)], fr_from_mont(c, evals)

    @staticmethod
    def verify(verifier_param, commitment, point: int, value: int, proof) -> bool:
        """mod.rs:195-216: e(C - [v]g + [z]pi, h) == e(pi, beta_h).  verifier_param: a keys.OpenKey (UnivariateVerifierParam; jf-plonk's
        OpenKey); commitment, proof: Commitment objects or G1 records of the key's mode.  A batch of one with weight 1, on the device
        (keys.OpenKey.begin_openings); a malformed record or scalar raises the SerializationError family."""
        c = verifier_param.curve
        b = verifier_param.begin_openings([commitment], [point], [value], [proof])
        return verifier_param.check(*b.finish(fr_to_mont(c, [1])))

    @staticmethod
    def batch_verify(verifier_param, commitments, points, values, proofs, rng) -> bool:
        """mod.rs:223-271: the K openings under random weights in one check of two pairings.  Weights as the reference draws them: 1, then
        per further opening u128::rand(rng) -- rng.next_u64() for the low half, then for the high half (rng: an rng.ChaChaRng) -- so a
        seeded caller gets the reference's randomizers.  Length mismatches raise PCSError; an empty batch is accepted (two pairings of O)."""
        K = len(commitments)
        for name, n in (("points", len(points)), ("values", len(values)), ("proofs", len(proofs))):
            if n != K:
                raise PCSError("InvalidParameters: commitments length %d is different from %s length %d" % (K, name, n))
        if K == 0:
            return True
        c = verifier_param.curve
        weights = [1]
        for _ in range(K - 1):
            lo = rng.next_u64()
            weights.append(lo | rng.next_u64() << 64)
        b = verifier_param.begin_openings(commitments, points, values, proofs)
        return verifier_param.check(*b.finish(fr_to_mont(c, weights)))

    # ---- UnivariatePCS (pcs/mod.rs:228-306): one polynomial opened over a radix-2 domain ------------------------------------------
    @staticmethod
    def trim_fft_size(params, supported_degree: int):
        """pcs/mod.rs:236-254: `trim` to checked_fft_size(supported_degree).  params: a UnivariateUniversalParams -> (prover param, OpenKey), or
        a UnivariateProverParam alone -> its trimmed view."""
        fft_degree = checked_fft_size(supported_degree)
        pp = params.powers_of_g if isinstance(params, UnivariateUniversalParams) else params
        try:
            trimmed = pp.trim(fft_degree)
        except PCSError as e:
            raise PCSError(f"InvalidParameters: Requesting degree of {fft_degree} for FFT:\n\t\t{e}") from None
        return (trimmed, params.verifier_param()) if isinstance(params, UnivariateUniversalParams) else trimmed

    @staticmethod
    def multi_open_rou_eval_domain(curve, degree: int, num_points: int):
        """pcs/mod.rs:259-275: the domain of max(checked_fft_size(degree) + 1, num_points) points, rounded up to a power of two."""
        from .domain import Radix2EvaluationDomain
        size = max(checked_fft_size(degree) + 1, num_points)
        try:
            return Radix2EvaluationDomain.new(curve, size)
        except ValueError:
            raise PCSError(f"UpstreamError: Fail to init eval domain of size {size}") from None

    @staticmethod
    def _rou_check(curve, n: int, domain, degree_limit: int | None):
        """The reference's refusals for a polynomial of n coefficients, made before the device is touched: those of the evaluations
        (degree_limit None), or of the proofs under a prover param of degree_limit points."""
        if domain.curve is not curve or not domain.coset_offset_is_one():
            raise PCSError("InvalidParameters: multi_open_rou takes the radix-2 domain of the polynomial's field with offset one, not a coset")
        if degree_limit is None:
            if n > domain.size:                                            # pcs/poly.rs:141-147
                raise PCSError(f"InvalidParameters: Polynomial with {n} num_of_coeffs can't be evaluated on a smaller domain with size {domain.size}")
            return
        d = _next_power_of_two(max(n, 1) - 1)                              # mod.rs:342-349: the padded degree, from the length as given
        if d > degree_limit:                                               # (srs_vec comes out shorter than the matrix: toeplitz.rs:127-131)
            raise PCSError(f"InvalidParameters: the prover parameter holds {degree_limit} points, FK23 at padded degree {d} takes {d}")
        if d > domain.size:
            raise PCSError(f"InvalidParameters: Polynomial with {d} num_of_coeffs can't be evaluated on a smaller domain with size {domain.size}")

    @staticmethod
    def _rou_coeffs(polynomial):
        """(len, 4) Montgomery coefficients as given: a CUDA tensor stays where it is, a host array stays on the host until the checks passed"""
        if _is_torch(polynomial):
            import torch
            if polynomial.dtype != torch.int64 or not polynomial.is_cuda or polynomial.dim() != 2 or polynomial.shape[1] != 4:
                raise ValueError("expected a (len, 4) int64 CUDA tensor or a uint64 host array")
            return polynomial.contiguous()
        return np.ascontiguousarray(polynomial, dtype=np.uint64).reshape(-1, 4)

    @staticmethod
    def _rou_device(a):
        if _is_torch(a):
            return a
        import torch
        return torch.from_numpy(a.view(np.int64)).cuda()

    @staticmethod
    def _rou_open(pp, a, num_points: int, domain, want_evals: bool):
        import torch
        c, t, n, k = pp.curve, UnivariateKzgPCS._rou_device(a), a.shape[0], min(max(num_points, 0), domain.size)
        proofs = np.zeros((k, 2, c.fq_limbs), dtype=np.uint64)
        evals = np.zeros((k, 4), dtype=np.uint64) if want_evals else None
        st = torch.cuda.current_stream(t.device).cuda_stream
        _lib.check(_lib.ensure_init().mzk_kzg_multi_open_rou_dev(pp.handle, pp.offset, t.data_ptr() if n else None, n, domain.log_size_of_group, k,
                                                                 C.c_void_p(proofs.ctypes.data), None if evals is None else C.c_void_p(evals.ctypes.data),
                                                                 C.c_void_p(st)), "mzk_kzg_multi_open_rou_dev")
        return [Commitment(c, proofs[i]) for i in range(k)], None if evals is None else fr_from_mont(c, evals)

    @staticmethod
    def multi_open_rou(prover_param: UnivariateProverParam, polynomial, num_points: int, domain):
        """pcs/mod.rs:281-290: the polynomial opened at the first num_points points w^0, w^1, .. of `domain` (a domain.Radix2EvaluationDomain with
        offset one; at most its size: the reference's `take`) -> ([Commitment proofs], [evaluation ints]).  One call of the device
        (mzk_kzg_multi_open_rou_dev): the evaluations by a scalar NTT, the proofs by FK23 in O(d log d) group operations, d the padded degree --
        next_power_of_two(len - 1) of the coefficient array AS GIVEN (trailing zeros are not trimmed; the proofs do not depend on it, the
        number of points taken from prover_param does).  The transformed SRS vector stays on the prover param's registration for the next call
        at the same d.  polynomial: (len, 4) Montgomery coefficients, host array or CUDA tensor.  The evaluation step's checks come first, as
        in the reference; every refusal raises PCSError before the device is touched."""
        pp, K = prover_param, UnivariateKzgPCS
        a = K._rou_coeffs(polynomial)
        K._rou_check(pp.curve, a.shape[0], domain, None)                   # multi_open_rou_evals's refusals, then multi_open_rou_proofs's
        K._rou_check(pp.curve, a.shape[0], domain, pp.length)
        return K._rou_open(pp, a, num_points, domain, True)

    @staticmethod
    def multi_open_rou_proofs(prover_param: UnivariateProverParam, polynomial, num_points: int, domain) -> list[Commitment]:
        """mod.rs:299-313: the proofs of multi_open_rou alone."""
        a = UnivariateKzgPCS._rou_coeffs(polynomial)
        UnivariateKzgPCS._rou_check(prover_param.curve, a.shape[0], domain, prover_param.length)
        return UnivariateKzgPCS._rou_open(prover_param, a, num_points, domain, False)[0]

    @staticmethod
    def multi_open_rou_evals(polynomial, num_points: int, domain) -> list[int]:
        """mod.rs:316-327: the evaluations of multi_open_rou alone -- the coefficients zero-padded to the domain, one forward NTT
        (domain.fft_in_place), the first num_points values.  No SRS."""
        import torch
        a = UnivariateKzgPCS._rou_coeffs(polynomial)
        UnivariateKzgPCS._rou_check(domain.curve, a.shape[0], domain, None)
        t, n, k = UnivariateKzgPCS._rou_device(a), a.shape[0], min(max(num_points, 0), domain.size)
        buf = torch.zeros((domain.size, 4), dtype=torch.int64, device=t.device)
        buf[:n] = t
        domain.fft_in_place(buf)
        return fr_from_mont(domain.curve, buf[:k].cpu().numpy().view(np.uint64))


def jacobian_to_affine(curve, xyz: np.ndarray) -> np.ndarray:
    """(n,3,fq_limbs) Jacobian -> (n,2,fq_limbs) affine on the host (`into_affine`, mod.rs:111)."""
    c = _curve(curve)
    a = np.ascontiguousarray(xyz, dtype=np.uint64).reshape(-1, 3, c.fq_limbs)
    out = np.empty((a.shape[0], 2, c.fq_limbs), dtype=np.uint64)
    _lib.check(_lib.load().mzk_g1_jacobian_to_affine(c.curve_id, C.c_void_p(a.ctypes.data), a.shape[0], C.c_void_p(out.ctypes.data)),
               "mzk_g1_jacobian_to_affine")
    return out


def msm_bigint_batch(pp: UnivariateProverParam, scalar_sets, base_offsets=None, scalars_are_mont: bool = False,
                     absolute_offsets: bool = False) -> np.ndarray:
    """Several MSMs over one SRS in one call -> (k,3,fq_limbs) Jacobian.  scalar_sets: host (n_i,4) uint64
    arrays, or int64 CUDA tensors (all of one kind)."""
    L = _lib.ensure_init()
    k = len(scalar_sets)
    out = np.empty((k, 3, pp.curve.fq_limbs), dtype=np.uint64)
    if k == 0:
        return out
    offs = [0] * k if base_offsets is None else list(base_offsets)
    if not absolute_offsets:
        offs = [pp.offset + o for o in offs]
    limit = pp.offset + pp.length
    lens = (C.c_uint64 * k)()
    offa = (C.c_uint64 * k)(*offs)
    ptrs = (C.c_void_p * k)()
    if _is_torch(scalar_sets[0]):
        import torch
        for i, t in enumerate(scalar_sets):
            if t.dtype != torch.int64 or not t.is_cuda or not t.is_contiguous() or t.shape[-1] != 4:
                raise ValueError("expected contiguous int64 CUDA tensors of shape (n, 4)")
            lens[i] = min(t.shape[0], max(0, limit - offs[i]))
            ptrs[i] = t.data_ptr()
        st = torch.cuda.current_stream(scalar_sets[0].device).cuda_stream
        _lib.check(L.mzk_msm_batch_dev(pp.handle, k, ptrs, lens, offa, int(scalars_are_mont), C.c_void_p(out.ctypes.data), st),
                   "mzk_msm_batch_dev")
        return out
    keep = []
    for i, s in enumerate(scalar_sets):
        a = np.ascontiguousarray(s, dtype=np.uint64).reshape(-1, 4)
        keep.append(a)
        lens[i] = min(a.shape[0], max(0, limit - offs[i]))
        ptrs[i] = a.ctypes.data if a.size else None
    _lib.check(L.mzk_msm_batch(pp.handle, k, ptrs, lens, offa, int(scalars_are_mont), C.c_void_p(out.ctypes.data)), "mzk_msm_batch")
    return out


def open_key_for_testing(curve, beta: int, h: bytes | None = None, compress: bool = True):
    """(g, h, beta_h) of `gen_srs_for_testing` (srs.rs:118-153) as records of the mode `compress`: g the curve's G1 generator, h the G2
    generator (or the record given), beta_h = [beta]h through the host G2 arithmetic (mzk_g2_mul; no GPU)."""
    from . import transcript as _transcript
    c = _curve(curve)
    L = _lib.load()
    flags, n = (1 if compress else 0), g2_record_bytes(c, compress)
    one, k = (C.c_uint64 * 4)(1, 0, 0, 0), (C.c_uint64 * 4)(*[(beta % c.r >> (64 * i)) & (2**64 - 1) for i in range(4)])
    h_buf = None if h is None else (C.c_uint8 * n).from_buffer_copy(bytes(h))
    h_out, bh_out = (C.c_uint8 * n)(), (C.c_uint8 * n)()
    _lib.check(L.mzk_g2_mul(c.curve_id, h_buf, one, flags | 2, h_out), "mzk_g2_mul")
    _lib.check(L.mzk_g2_mul(c.curve_id, h_buf, k, flags | 2, bh_out), "mzk_g2_mul")
    g = _transcript.g1_bytes(c, (c.gx, c.gy))
    if not compress:                                      # x || y, no flag set: y's sign flag belongs to BN254's last byte and is ignored on read
        size = len(g)
        g = c.gx.to_bytes(size, "big") + c.gy.to_bytes(size, "big") if c.curve_id == 0 else c.gx.to_bytes(size, "little") + c.gy.to_bytes(size, "little")
    return g, bytes(h_out), bytes(bh_out)
