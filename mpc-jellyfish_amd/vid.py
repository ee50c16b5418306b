"""Advz -- mirror of primitives/src/vid/advz.rs, `Advz<E, Sha256>`: verifiable information dispersal over KZG and a ternary SHA-256 tree.

    GenericAdvz::new                       advz.rs:88-109   -> Advz(curve, payload_chunk_size, num_storage_nodes, srs)
    commit_only                            advz.rs:171-184  -> Advz.commit_only            (mzk_vid_advz_commit_only_dev)
    disperse / disperse_from_elems         advz.rs:186-192, 279-391 -> Advz.disperse / disperse_from_elems (mzk_vid_advz_disperse_dev)
    verify_share                           advz.rs:194-257  -> Advz.verify_share, and the batched Advz.verify_shares (mzk_vid_advz_verify_shares_dev,
                                                               then UnivariateKzgPCS.verify / batch_verify)
    recover_payload / recover_elems        advz.rs:259-262, 395-439 -> Advz.recover_payload / recover_elems (mzk_vid_advz_recover_dev)
    bytes_to_field / field_to_bytes        utilities/src/conversion.rs:379-523 -> bytes_to_field / field_to_bytes (on the device)

Everything is restated as the reference has it, quirks included: the aggregate is s * SUM (polynomial_eval is not
Horner), a payload of a multiple of 31 bytes gets no length element, the domain follows multi_open_rou_eval_domain(k, n).  A Share's evals_proof
is the path of sibling digests alone -- (height, 2, 32) bytes, zeros for an empty sibling -- and the leaf is hashed from Share.evals.
Payloads: bytes, a numpy uint8 array or a 1-D uint8 CUDA tensor.  Field elements: Python ints."""
from __future__ import annotations

import ctypes as C
import os
from dataclasses import dataclass, field

import numpy as np

from . import lib as _lib
from .kzg import (Commitment, PCSError, UnivariateKzgPCS, UnivariateProverParam, UnivariateUniversalParams, _as_bytes, _is_torch, g1_record)
from .params import curve as _curve, fr_from_mont, fr_to_mont

ELEM_BYTES = 31                                                    # conversion.rs: (MODULUS_BIT_SIZE - 1) / 8 on both curves
DST = b"rick"                                                      # advz.rs:454
RECOVER_MAX_K = 1024                                               # include/mzk.h, mzk_vid_advz_recover_dev


class VidError(Exception):
    """vid/mod.rs VidError: .kind is "Argument" (the caller's) or "Internal" (everything the reference maps through `vid`)."""

    def __init__(self, kind: str, message: str):
        super().__init__(f"{kind}: {message}")
        self.kind = kind

    @classmethod
    def Argument(cls, message: str) -> "VidError":
        return cls("Argument", message)

    @classmethod
    def Internal(cls, message: str) -> "VidError":
        return cls("Internal", message)


@dataclass
class Share:
    """advz.rs:117-129.  evals: K ints; aggregate_proof: a Commitment; evals_proof: (height, 2, 32) uint8 sibling digests, leaf level first."""
    index: int
    evals: list
    aggregate_proof: Commitment
    evals_proof: np.ndarray


@dataclass
class Common:
    """advz.rs:136-145.  all_evals_digest: the 32-byte root."""
    poly_commits: list
    all_evals_digest: bytes
    elems_len: int
    _aggregate: object = field(default=None, repr=False, compare=False)     # (s, s * sum_j C_j) once computed: Advz._aggregate_commit


@dataclass
class VidDisperse:
    """vid/mod.rs VidDisperse: shares, common, commit (32 bytes)."""
    shares: list
    common: Common
    commit: bytes


def field_count(n_bytes: int) -> int:
    """elements bytes_to_field makes of n_bytes bytes: no length element at a multiple of 31"""
    return n_bytes // ELEM_BYTES + (2 if n_bytes % ELEM_BYTES else 0)


def tree_height(n: int) -> int:
    """advz.rs:325-337: ilog3(n) + 1"""
    h = 1
    while n >= 3:
        n //= 3
        h += 1
    return h


def _stream(t) -> int:
    import torch
    return torch.cuda.current_stream(t.device).cuda_stream


def _payload_tensor(payload):
    """the payload's bytes on the device (a CUDA tensor stays where it is)"""
    import torch
    buf = _as_bytes(payload)
    if _is_torch(buf):
        return buf
    _lib.ensure_init()
    return torch.from_numpy(np.array(buf, copy=True)).cuda() if buf.shape[0] else torch.zeros(0, dtype=torch.uint8, device="cuda")


def bytes_to_field(curve, payload):
    """conversion.rs:379-408 on the device -> (count, 4) int64 CUDA tensor of Montgomery elements"""
    import torch
    c = _curve(curve)
    t = _payload_tensor(payload)
    out = torch.empty((field_count(t.shape[0]), 4), dtype=torch.int64, device=t.device)
    _lib.check(_lib.ensure_init().mzk_bytes_to_field_dev(c.curve_id, C.c_void_p(t.data_ptr() if t.shape[0] else None), t.shape[0],
                                                         C.c_void_p(out.data_ptr() if out.shape[0] else None), C.c_void_p(_stream(t))), "mzk_bytes_to_field_dev")
    return out


def field_to_bytes(curve, elems) -> bytes:
    """conversion.rs:443-523 on the device, as written.  elems: a (count, 4) int64 CUDA tensor (Montgomery) or a list of ints."""
    import torch
    c = _curve(curve)
    t = _elems_tensor(c, elems)
    count = t.shape[0]
    if count == 0:
        return b""
    out = torch.empty(ELEM_BYTES * max(count - 2, 0) + 32, dtype=torch.uint8, device=t.device)
    n = C.c_uint64()
    _lib.check(_lib.ensure_init().mzk_field_to_bytes_dev(c.curve_id, C.c_void_p(t.data_ptr()), count, C.c_void_p(out.data_ptr()), C.byref(n),
                                                         C.c_void_p(_stream(t))), "mzk_field_to_bytes_dev")
    return bytes(out[:n.value].cpu().numpy())


def _elems_tensor(c, elems):
    import torch
    if _is_torch(elems):
        if elems.dtype != torch.int64 or not elems.is_cuda or elems.dim() != 2 or elems.shape[1] != 4:
            raise ValueError("expected a (count, 4) int64 CUDA tensor of Montgomery elements or a list of ints")
        return elems.contiguous()
    _lib.ensure_init()
    vals = [int(v) for v in elems]
    if not vals:
        return torch.zeros((0, 4), dtype=torch.int64, device="cuda")
    return torch.from_numpy(fr_to_mont(c, vals).view(np.int64)).cuda()


class _OsRng:
    """weights of verify_shares' batch check: u128 from the operating system, drawn as batch_verify draws them"""

    def next_u64(self) -> int:
        return int.from_bytes(os.urandom(8), "little")


class Advz:
    def __init__(self, curve, payload_chunk_size: int, num_storage_nodes: int, srs, open_key=None):
        """advz.rs:88-109.  srs: a UnivariateUniversalParams, or a UnivariateProverParam with its keys.OpenKey (open_key; None: an instance that
        disperses and recovers but cannot verify).  Trims to checked_fft_size(payload_chunk_size), as trim_fft_size does."""
        self.curve = _curve(curve)
        k, n = int(payload_chunk_size), int(num_storage_nodes)
        if n < k:
            raise VidError.Argument(f"payload_chunk_size {k} exceeds num_storage_nodes {n}")
        if k < 1:
            raise VidError.Argument("payload_chunk_size must be positive")
        try:
            if isinstance(srs, UnivariateUniversalParams):
                self.ck, self.vk = UnivariateKzgPCS.trim_fft_size(srs, k)
            else:
                self.ck, self.vk = UnivariateKzgPCS.trim_fft_size(srs, k), open_key
            self.domain = UnivariateKzgPCS.multi_open_rou_eval_domain(self.curve, k, n)    # the chunk size where a degree is expected: as the reference
        except PCSError as e:
            raise VidError.Internal(str(e)) from None
        if self.ck.curve is not self.curve:
            raise VidError.Argument("the SRS belongs to another curve")
        self.payload_chunk_size, self.num_storage_nodes = k, n
        self.height = tree_height(n)

    def _group_gen(self) -> int:
        """the generator of the domain, as ark-ff derives it: GENERATOR^((r - 1) / 2^two_adicity), squared down to the domain's order"""
        c = self.curve
        root = pow(c.fr_generator, (c.r - 1) >> c.two_adicity, c.r)
        return pow(root, 1 << (c.two_adicity - self.domain.log_size_of_group), c.r)

    # ---- commit_only, disperse ----------------------------------------------------------------------------------------------------------
    def _shape_args(self, t):
        return (self.ck.handle, self.ck.offset, self.ck.length, C.c_void_p(t.data_ptr() if t.shape[0] else None), t.shape[0], self.payload_chunk_size,
                self.num_storage_nodes, self.domain.log_size_of_group)

    def commit_only(self, payload) -> bytes:
        """advz.rs:171-184: SHA256 over the uncompressed records of the polynomial commitments"""
        t = bytes_to_field(self.curve, payload)
        out = (C.c_uint8 * 32)()
        _lib.check(_lib.ensure_init().mzk_vid_advz_commit_only_dev(*self._shape_args(t), out, C.c_void_p(_stream(t))), "mzk_vid_advz_commit_only_dev")
        return bytes(out)

    def disperse(self, payload) -> VidDisperse:
        """advz.rs:186-192"""
        return self.disperse_from_elems(bytes_to_field(self.curve, payload))

    def disperse_from_elems(self, elems) -> VidDisperse:
        """advz.rs:279-391 in one call of the device.  elems: a (count, 4) int64 CUDA tensor of Montgomery elements, or a list of ints."""
        c, k, n = self.curve, self.payload_chunk_size, self.num_storage_nodes
        t = _elems_tensor(c, elems)
        M = t.shape[0]
        K = (M + k - 1) // k
        sizes, m = [], n
        for _ in range(self.height + 1):
            sizes.append(m)
            m = (m + 2) // 3
        commits = np.zeros((K, 2, c.fq_limbs), dtype=np.uint64)
        evals = np.zeros((n, K, 32), dtype=np.uint8)
        proofs = np.zeros((n, 2, c.fq_limbs), dtype=np.uint64)
        nodes = np.zeros((sum(sizes), 32), dtype=np.uint8)
        commit, root, s = (C.c_uint8 * 32)(), (C.c_uint8 * 32)(), np.zeros(4, dtype=np.uint64)
        _lib.check(_lib.ensure_init().mzk_vid_advz_disperse_dev(*self._shape_args(t), C.c_void_p(commits.ctypes.data), C.c_void_p(evals.ctypes.data),
                                                                C.c_void_p(proofs.ctypes.data), C.c_void_p(nodes.ctypes.data), commit, root,
                                                                C.c_void_p(s.ctypes.data), C.c_void_p(_stream(t))), "mzk_vid_advz_disperse_dev")
        paths = self._paths(nodes, sizes)
        raw = evals.tobytes()
        shares = []
        for i in range(n):
            row = [int.from_bytes(raw[(i * K + j) * 32:(i * K + j + 1) * 32], "little") for j in range(K)]
            shares.append(Share(i, row, Commitment(c, proofs[i]), paths[i]))
        common = Common([Commitment(c, commits[j]) for j in range(K)], bytes(root), M)
        return VidDisperse(shares, common, bytes(commit))

    def _paths(self, nodes: np.ndarray, sizes) -> np.ndarray:
        """(n, height, 2, 32): for every leaf and level the two other children of its parent, zeros where the tree has none"""
        n = self.num_storage_nodes
        paths = np.zeros((n, self.height, 2, 32), dtype=np.uint8)
        pos, first = np.arange(n), 0
        for level in range(self.height):
            padded = np.zeros((3 * sizes[level + 1], 32), dtype=np.uint8)
            padded[:sizes[level]] = nodes[first:first + sizes[level]]
            group = padded.reshape(-1, 3, 32)[pos // 3]                  # (n, 3, 32)
            digit = pos % 3
            paths[:, level, 0] = np.where((digit == 0)[:, None], group[:, 1], group[:, 0])
            paths[:, level, 1] = np.where((digit == 2)[:, None], group[:, 1], group[:, 2])
            first += sizes[level]
            pos = pos // 3
        return paths

    # ---- verify -------------------------------------------------------------------------------------------------------------------------
    def pseudorandom_scalar(self, common: Common) -> np.ndarray:
        """advz.rs:441-462 -> 4 Montgomery limbs: SHA256(records || root) through DefaultFieldHasher<Sha256, 128> with DST "rick" """
        L = _lib.load()
        msg = b"".join(g1_record(self.curve, cm, compress=False) for cm in common.poly_commits) + bytes(common.all_evals_digest)
        digest, out = (C.c_uint8 * 32)(), np.zeros(4, dtype=np.uint64)
        _lib.check(L.mzk_sha256(msg, len(msg), digest), "mzk_sha256")
        _lib.check(L.mzk_hash_to_field_sha256(self.curve.curve_id, digest, 32, DST, len(DST), C.c_void_p(out.ctypes.data)), "mzk_hash_to_field_sha256")
        return out

    def _aggregate_commit(self, common: Common):
        """(s, s * sum_j C_j), computed once per Common and kept on it.  The K commitments go through the device MSM as a K-point key with
        every scalar s (points at infinity left out: they add nothing) -- the adder of the host tail would need a host scalar multiplication
        on top, which the library does not have for G1."""
        if common._aggregate is None:
            c = self.curve
            s = self.pseudorandom_scalar(common)
            pts = [cm.xy for cm in common.poly_commits if not cm.is_infinity()]
            agg = Commitment(c, np.zeros((2, c.fq_limbs), dtype=np.uint64))
            if pts:
                key = UnivariateProverParam.from_affine(c, np.stack(pts))
                try:
                    out = np.empty((2, c.fq_limbs), dtype=np.uint64)
                    sc = np.ascontiguousarray(np.tile(s, (len(pts), 1)))
                    _lib.check(_lib.ensure_init().mzk_msm_affine(key.handle, 0, C.c_void_p(sc.ctypes.data), len(pts), 1, C.c_void_p(out.ctypes.data)),
                               "mzk_msm_affine")
                    agg = Commitment(c, out)
                finally:
                    key.release()
            common._aggregate = (s, agg)
        return common._aggregate

    def _merkle_and_evals(self, shares, common: Common):
        """one launch: ([Merkle verdict], [aggregate evaluation]) of the shares"""
        c, S, K = self.curve, len(shares), len(common.poly_commits)
        s, _ = self._aggregate_commit(common)
        index = np.array([sh.index for sh in shares], dtype=np.uint64)
        evals = np.frombuffer(b"".join((int(v) % c.r).to_bytes(32, "little") for sh in shares for v in sh.evals), dtype=np.uint8) if S * K else np.zeros(0, np.uint8)
        paths = np.ascontiguousarray(np.stack([np.asarray(sh.evals_proof, dtype=np.uint8).reshape(self.height, 2, 32) for sh in shares]))
        root = (C.c_uint8 * 32).from_buffer_copy(bytes(common.all_evals_digest))
        ok, agg = np.zeros(S, dtype=np.int32), np.zeros((S, 4), dtype=np.uint64)
        import torch
        st = torch.cuda.current_stream().cuda_stream
        _lib.check(_lib.ensure_init().mzk_vid_advz_verify_shares_dev(c.curve_id, S, K, self.num_storage_nodes, C.c_void_p(index.ctypes.data),
                                                                     C.c_void_p(evals.ctypes.data) if evals.size else None, C.c_void_p(paths.ctypes.data), root,
                                                                     C.c_void_p(s.ctypes.data), C.c_void_p(ok.ctypes.data), C.c_void_p(agg.ctypes.data), C.c_void_p(st)),
                   "mzk_vid_advz_verify_shares_dev")
        return [bool(v) for v in ok], fr_from_mont(c, agg)

    def _check_lengths(self, share: Share, common: Common):
        if len(share.evals) != len(common.poly_commits):
            raise VidError.Argument(f"(share eval, common poly commit) lengths differ ({len(share.evals)},{len(common.poly_commits)})")
        if np.asarray(share.evals_proof).size != self.height * 64:
            raise VidError.Argument(f"evals_proof holds {np.asarray(share.evals_proof).size} bytes, a path of this tree {self.height * 64}")
        if len(bytes(common.all_evals_digest)) != 32:
            raise VidError.Argument("all_evals_digest is not 32 bytes")

    def _require_vk(self):
        if self.vk is None:
            raise VidError.Argument("this Advz was made without an open key: it cannot verify")

    def verify_share(self, share: Share, common: Common) -> bool:
        """advz.rs:194-257: raises VidError for the length mismatch; False for index >= n, a Merkle failure or a KZG failure"""
        return self.verify_shares([share], common)[0]

    def verify_shares(self, shares, common: Common, rng=None) -> list:
        """verify_share for many shares of one Common: the Merkle verdicts and aggregate evaluations in one launch, the openings that passed in
        one batch_verify (weights from rng, an object with next_u64(); None: the operating system's), and one by one only when that fails"""
        self._require_vk()
        for sh in shares:
            self._check_lengths(sh, common)
        n = self.num_storage_nodes
        live = [i for i, sh in enumerate(shares) if 0 <= sh.index < n]
        out = [False] * len(shares)
        if not live:
            return out
        ok, agg = self._merkle_and_evals([shares[i] for i in live], common)
        _, cm = self._aggregate_commit(common)
        passed = [(i, v) for i, good, v in zip(live, ok, agg) if good]
        if not passed:
            return out
        w = self._group_gen()
        args = lambda items: ([cm] * len(items), [pow(w, shares[i].index, self.curve.r) for i, _ in items], [v for _, v in items],
                              [shares[i].aggregate_proof for i, _ in items])
        if len(passed) == 1:
            out[passed[0][0]] = UnivariateKzgPCS.verify(self.vk, cm, *[a[0] for a in args(passed)[1:]])
            return out
        if UnivariateKzgPCS.batch_verify(self.vk, *args(passed), rng or _OsRng()):
            for i, _ in passed:
                out[i] = True
            return out
        for item in passed:
            a = args([item])
            out[item[0]] = UnivariateKzgPCS.verify(self.vk, cm, a[1][0], a[2][0], a[3][0])
        return out

    # ---- recover ------------------------------------------------------------------------------------------------------------------------
    def _recover_tensor(self, shares, common: Common):
        """advz.rs:395-439 -> (elems_len, 4) int64 CUDA tensor, Montgomery.  The reference's refusals come before any launch."""
        import torch
        c, k = self.curve, self.payload_chunk_size
        if len(shares) < k:
            raise VidError.Argument(f"not enough shares {len(shares)}, expected at least {k}")
        K = len(shares[0].evals)
        for i, sh in enumerate(shares):
            if len(sh.evals) != K:
                raise VidError.Argument(f"shares do not have equal evals lengths: share 0 len {K}, share {i} len {len(sh.evals)}")
        _lib.ensure_init()
        out = torch.zeros((K * k, 4), dtype=torch.int64, device="cuda")
        if K:
            top = max(sh.index for sh in shares)
            if top >= self.domain.size or min(sh.index for sh in shares) < 0:                         # reed_solomon_code/mod.rs:162-174: over ALL shares
                raise VidError.Internal(f"share index {top} out of bounds for domain size {self.domain.size}")
            first = shares[:k]
            seen = {}
            for i, sh in enumerate(first):
                if sh.index in seen:
                    raise VidError.Internal(f"duplicate input point at indices {seen[sh.index]}, {i}")
                seen[sh.index] = i
            if k > RECOVER_MAX_K:
                raise VidError.Internal(f"recover takes payload_chunk_size up to {RECOVER_MAX_K}")
            index = np.array([sh.index for sh in first], dtype=np.uint64)
            y = fr_to_mont(c, [first[i].evals[p] for p in range(K) for i in range(k)])
            _lib.check(_lib.load().mzk_vid_advz_recover_dev(c.curve_id, k, K, self.domain.log_size_of_group, C.c_void_p(index.ctypes.data), C.c_void_p(y.ctypes.data),
                                                            C.c_void_p(out.data_ptr()), C.c_void_p(_stream(out))), "mzk_vid_advz_recover_dev")
        return out[:common.elems_len]

    def recover_elems(self, shares, common: Common) -> list:
        t = self._recover_tensor(shares, common)
        return fr_from_mont(self.curve, t.cpu().numpy().view(np.uint64)) if t.shape[0] else []

    def recover_payload(self, shares, common: Common) -> bytes:
        """advz.rs:259-262: field_to_bytes of recover_elems, both on the device"""
        return field_to_bytes(self.curve, self._recover_tensor(shares, common).contiguous())
