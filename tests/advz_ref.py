"""Test-side restatement of the ADVZ VID scheme (primitives/src/vid/advz.rs, `Advz<E, Sha256>`) on oracle/pyref.py's big-int helpers: not a
test, and no code shared with the product.  Restated as the reference has it:

    bytes_to_field / field_to_bytes   utilities/src/conversion.rs:379-523 (31 bytes an element; no length element at a multiple of 31)
    leaf / branch digests, the tree   merkle_tree/hasher.rs:141-161, internal.rs:166-227 (ternary, height = ilog3(n) + 1, zeros for Empty)
    expand_message_xmd, hash_to_field ark-ff 0.4 DefaultFieldHasher<Sha256, 128>: Z_pad of 48 bytes by default (RFC 9380 has 64)
    polynomial_eval                   advz.rs:499-506: `coeff * point + res`, i.e. point * SUM
    disperse                          advz.rs:279-391; commitments and proofs through the trapdoor beta of the testing SRS:
                                      C = p(beta) G, proof_i = [(a(beta) - a(w^i)) / (beta - w^i)] G
    reed_solomon_erasure_decode_rou   reed_solomon_code/mod.rs:68-187, the O(k^2) Lagrange routine"""
import hashlib

import pyref

ELEM = 31
Z_PAD_ARK = 48


def sha256(b: bytes) -> bytes:
    return hashlib.sha256(b).digest()


# ---- conversion.rs --------------------------------------------------------------------------------------------------------------------------
def bytes_to_field(payload: bytes) -> list:
    """the iterator of conversion.rs:379-408 step by step: `new` is never cleared, so an exhausted iterator at a group boundary ends the output"""
    it, out, final_len, at = bytes(payload), [], None, 0
    while True:
        if final_len is not None:
            out.append(final_len)
            return out
        if at >= len(it):                                                  # self.new && peek().is_none()
            return out
        group = it[at:at + ELEM]
        at += len(group)
        if len(group) < ELEM:
            final_len = len(group)
        out.append(int.from_bytes(group, "little"))


def field_to_bytes(elems) -> bytes:
    """conversion.rs:443-523: the last element is a length for the one before it, whatever it holds"""
    elems = list(elems)
    if not elems:
        return b""
    if len(elems) == 1:
        return elems[0].to_bytes(32, "little")[:ELEM]
    out = b"".join(e.to_bytes(32, "little")[:ELEM] for e in elems[:-2])
    take = elems[-1] & ((1 << 64) - 1)
    return out + elems[-2].to_bytes(32, "little")[:take]


# ---- the Merkle tree ------------------------------------------------------------------------------------------------------------------------
def tree_height(n: int) -> int:
    h = 0
    while 3 ** (h + 1) <= n:
        h += 1
    return h + 1


def leaf_digest(pos: int, evals) -> bytes:
    return sha256(pos.to_bytes(8, "little") + len(evals).to_bytes(8, "little") + b"".join(e.to_bytes(32, "little") for e in evals))


def tree_levels(leaves, height: int):
    """[leaves, level 1, .., root level]: `height` branch levels whatever the number of leaves"""
    levels = [list(leaves)]
    for _ in range(height):
        cur = levels[-1]
        nxt = []
        for g in range(0, len(cur), 3):
            kids = cur[g:g + 3]
            kids += [bytes(32)] * (3 - len(kids))
            nxt.append(sha256(b"".join(kids)))
        levels.append(nxt)
    assert len(levels[-1]) == 1
    return levels


def tree_path(levels, pos: int):
    """per level the two siblings in child order, zeros for an empty one"""
    path = []
    for level in levels[:-1]:
        group = level[pos // 3 * 3:pos // 3 * 3 + 3]
        group += [bytes(32)] * (3 - len(group))
        path.append([d for t, d in enumerate(group) if t != pos % 3])
        pos //= 3
    return path


def tree_verify(root: bytes, pos: int, evals, path) -> bool:
    cur = leaf_digest(pos, evals)
    for sib in path:
        kids = list(sib)
        kids.insert(pos % 3, cur)
        cur = sha256(b"".join(kids))
        pos //= 3
    return cur == root


# ---- hash to field --------------------------------------------------------------------------------------------------------------------------
def expand_message_xmd(msg: bytes, dst: bytes, out_len: int, z_pad_len: int = Z_PAD_ARK) -> bytes:
    ell = -(-out_len // 32)
    assert ell <= 255 and len(dst) <= 255
    dst_prime = dst + bytes([len(dst)])
    b0 = sha256(bytes(z_pad_len) + msg + out_len.to_bytes(2, "big") + b"\x00" + dst_prime)
    b = [sha256(b0 + b"\x01" + dst_prime)]
    for i in range(2, ell + 1):
        b.append(sha256(bytes(x ^ y for x, y in zip(b0, b[-1])) + bytes([i]) + dst_prime))
    return b"".join(b)[:out_len]


def hash_to_field(c, msg: bytes, dst: bytes, z_pad_len: int = Z_PAD_ARK) -> int:
    return int.from_bytes(expand_message_xmd(msg, dst, 48, z_pad_len), "big") % c.r


# ---- G1 records -----------------------------------------------------------------------------------------------------------------------------
def g1_uncompressed(c, pt) -> bytes:
    """ark-serialize 0.4 serialize_uncompressed of an affine point (None: infinity)"""
    size = 8 * c.fq_limbs
    if c is pyref.BLS12_381:
        if pt is None:
            return bytes([0x40]) + bytes(2 * size - 1)
        return pt[0].to_bytes(size, "big") + pt[1].to_bytes(size, "big")
    if pt is None:
        return bytes(2 * size - 1) + bytes([0x40])
    rec = bytearray(pt[0].to_bytes(size, "little") + pt[1].to_bytes(size, "little"))
    if pt[1] > c.q - pt[1]:
        rec[-1] |= 0x80
    return bytes(rec)


# ---- the scheme -----------------------------------------------------------------------------------------------------------------------------
def domain_log(k: int, n: int) -> int:
    """multi_open_rou_eval_domain(k, n): checked_fft_size(k) + 1 against n, up to a power of two"""
    fft = 2 * k if k > 0 and k & (k - 1) == 0 else (1 if k <= 1 else 1 << (k - 1).bit_length())
    size = max(fft + 1, n)
    return (size - 1).bit_length() if size > 1 else 0


def pseudorandom_scalar(c, commits, root: bytes) -> int:
    msg = b"".join(g1_uncompressed(c, p) for p in commits) + root
    return hash_to_field(c, sha256(msg), b"rick")


def disperse(c, k: int, n: int, beta: int, elems):
    """-> dict(commits, evals[n][K], root, paths[n], commit, proofs[n], s, elems_len, log_n)"""
    r, G = c.r, pyref.g1_gen(c)
    elems = list(elems)
    polys = [elems[i:i + k] for i in range(0, len(elems), k)]
    log_n = domain_log(k, n)
    w = c.root_of_unity(log_n)
    xs = [pow(w, i, r) for i in range(n)]
    evals = [[pyref.poly_eval(c, p, x) for p in polys] for x in xs]
    levels = tree_levels([leaf_digest(i, evals[i]) for i in range(n)], tree_height(n))
    root = levels[-1][0]
    mul = lambda s: pyref.g1_mul(c, s % r, G) if s % r else None
    commits = [mul(pyref.poly_eval(c, p, beta)) for p in polys]
    commit = sha256(b"".join(g1_uncompressed(c, p) for p in commits))
    s = pseudorandom_scalar(c, commits, root)
    agg = [0] * k
    for p in polys:                                                        # fold(zero, |res, coeff| coeff * point + res)
        for j, v in enumerate(p):
            agg[j] = (v * s + agg[j]) % r
    at_beta = pyref.poly_eval(c, agg, beta)
    proofs = [mul((at_beta - pyref.poly_eval(c, agg, x)) * pow(beta - x, -1, r)) for x in xs]
    return dict(commits=commits, evals=evals, root=root, paths=[tree_path(levels, i) for i in range(n)], commit=commit, proofs=proofs, s=s,
                elems_len=len(elems), log_n=log_n, levels=levels)


def rs_decode(c, shares, k: int, log_n: int) -> list:
    """reed_solomon_erasure_decode_rou on (index, eval) pairs: the first k of them"""
    r = c.r
    if max(i for i, _ in shares) >= 1 << log_n:
        raise ValueError("share index out of bounds")
    w = c.root_of_unity(log_n)
    pts = [(pow(w, i, r), y) for i, y in shares][:k]
    if len(pts) < k:
        raise ValueError("Insufficient evaluation points")
    x = [p[0] for p in pts]
    l = [0] * (k + 1)
    l[0] = 1
    for i in range(1, k + 1):
        l[i] = 1
        for j in range(i - 1, 0, -1):
            l[j] = (l[j - 1] - x[i - 1] * l[j]) % r
        l[0] = -x[i - 1] * l[0] % r
    wts = []
    for i in range(k):
        d = 1
        for j in range(k):
            if i != j:
                if (x[i] - x[j]) % r == 0:
                    raise ValueError("duplicate input point")
                d = d * (x[i] - x[j]) % r
        wts.append(pow(d, -1, r))
    f = [0] * k
    for i, (xi, yi) in enumerate(pts):
        li = [0] * k
        li[k - 1] = 1
        for j in range(k - 2, -1, -1):
            li[j] = (l[j + 1] + xi * li[j + 1]) % r
        wt = wts[i] * yi % r
        for j in range(k):
            f[j] = (f[j] + wt * li[j]) % r
    return f


def recover_elems(c, shares, k: int, n: int, elems_len: int) -> list:
    """shares: [(index, evals)] -> the payload's elements (advz.rs:395-439)"""
    K = len(shares[0][1])
    out = []
    for p in range(K):
        out += rs_decode(c, [(i, ev[p]) for i, ev in shares], k, domain_log(k, n))
    return out[:elems_len]
