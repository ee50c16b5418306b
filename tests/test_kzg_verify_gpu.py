"""GPU: KZG openings as a verifier group (mzk_verifier_open_begin: csrc/verifier.cuh "KZG openings"; keys.OpenKey.begin_openings,
UnivariateKzgPCS.verify / batch_verify) against integer arithmetic through the trapdoor.

Every G1 point is a known multiple of the generator, so no prover and no pairing oracle is needed: with the commitment [c]G, the proof
[w]G, the point z and the value v, one opening is valid iff c - v == (beta - z) w (mod r), and a batch under weights t_i is accepted iff
sum_i t_i (c_i - v_i - (beta - z_i) w_i) == 0.  Per curve the pool of 129 valid openings is built once (the `world` fixture) and shared."""
import ctypes as C
import random

import numpy as np
import pytest

from conftest import fr_from_mont_limbs, fr_mont_limbs
import pyref_fs as FS
from test_link_verify_gpu import _g1_uncompressed, _synthetic, _x_off_the_curve

pytestmark = pytest.mark.gpu

ERR_INVALID_ARG, ERR_BAD_HANDLE = -1, -4
SIZES = (1, 2, 63, 64, 65, 129)                                       # the lane and workgroup edges of VFY_THREADS = 64
SEED = bytes(range(32))


class Opening:
    """commitment [c]G, proof [w]G, point z, value v; the points as the oracle's affine pairs (None: infinity)"""

    def __init__(self, c, C_pt, z, v, w, W_pt):
        self.c, self.C, self.z, self.v, self.w, self.W = c, C_pt, z, v, w, W_pt

    def error(self, r, beta):
        return (self.c - self.v - (beta - self.z) * self.w) % r

    def replace(self, **kw):
        o = Opening(self.c, self.C, self.z, self.v, self.w, self.W)
        o.__dict__.update(kw)
        return o

    def swapped(self):
        return Opening(self.w, self.W, self.z, self.v, self.c, self.C)


def _accepts(r, beta, openings, weights):
    return sum(t * o.error(r, beta) for o, t in zip(openings, weights)) % r == 0


def _pool(pc, P, rng, beta):
    """129 valid openings: real ones of polynomials of lengths 0, 1, 2 and 41 (the longest opened at 0, 1, r - 1 and random points: one
    commitment, repeated), one with value 0, then synthetic ones over the same few commitments whose proofs [w_0 + i d]G come from a chain
    of additions"""
    r, G = pc.r, P.g1_gen(pc)
    mul = lambda k: P.g1_mul(pc, k % r, G) if k % r else None
    out = []
    polys = {n: [rng.randrange(r) for _ in range(n)] for n in (1, 2, 41)}
    polys[0] = []
    comm = {n: P.poly_eval(pc, p, beta) if p else 0 for n, p in polys.items()}
    comm_pt = {n: mul(k) for n, k in comm.items()}
    for n, z in ((41, 0), (41, 1), (41, r - 1), (41, rng.randrange(r)), (2, rng.randrange(r)), (2, 0), (1, rng.randrange(r)), (1, r - 1), (0, rng.randrange(r)), (0, 0)):
        v = P.poly_eval(pc, polys[n], z) if polys[n] else 0
        w = (comm[n] - v) * pow(beta - z, -1, r) % r
        out.append(Opening(comm[n], comm_pt[n], z, v, w, mul(w)))
    assert out[6].W is None and out[8].C is None and out[8].W is None      # a constant opens with pi = O; the zero polynomial: C = pi = O
    z, w = rng.randrange(r), rng.randrange(1, r)                           # value 0: the commitment of (X - z) s(X)
    out.append(Opening((beta - z) * w % r, mul((beta - z) * w), z, 0, w, mul(w)))
    w, d = rng.randrange(r), rng.randrange(1, r)
    W, D = mul(w), mul(d)
    while len(out) < SIZES[-1]:
        n = (41, 2, 1)[len(out) % 3]
        z = rng.randrange(r)
        out.append(Opening(comm[n], comm_pt[n], z, (comm[n] - (beta - z) * w) % r, w, W))
        w, W = (w + d) % r, P.g1_add(pc, W, D)
    assert all(o.error(r, beta) == 0 for o in out) and any(o.v == 0 for o in out)
    return out


@pytest.fixture(scope="module")
def world(gpu, mj, pyref):
    out = {}
    for cid in (0, 1):
        c, pc = mj.params.CURVES[cid], pyref.CURVES[cid]
        rng = random.Random(5200 + cid)
        beta = rng.randrange(1, c.r)
        keys = {cmp: mj.keys.OpenKey(c, *mj.kzg.open_key_for_testing(c, beta, compress=cmp), compressed=cmp) for cmp in (True, False)}
        pool = _pool(pc, pyref, rng, beta)
        assert pyref.g1_mul(pc, pool[-1].w, pyref.g1_gen(pc)) == pool[-1].W
        out[cid] = dict(beta=beta, keys=keys, pool=pool, pc=pc, rng=rng)
    yield out
    for w in out.values():
        for k in w["keys"].values():
            k.release()


def _enc(pc, compress):
    return (lambda p: FS.g1_bytes(pc, p)) if compress else (lambda p: _g1_uncompressed(pc, p))


def _args(pc, openings, compress=True):
    enc = _enc(pc, compress)
    return [enc(o.C) for o in openings], [o.z for o in openings], [o.v for o in openings], [enc(o.W) for o in openings]


def _drawn_weights(mj, K):
    rng = mj.rng.ChaChaRng(SEED, 20)
    out = [1]
    for _ in range(K - 1):
        lo = rng.next_u64()
        out.append(lo | rng.next_u64() << 64)
    return out


def _batch_verify(mj, key, pc, openings, compress=True):
    return mj.UnivariateKzgPCS.batch_verify(key, *_args(pc, openings, compress), mj.rng.ChaChaRng(SEED, 20))


def _c_level(mj, key, pc, openings, weights, compress=True):
    b = key.begin_openings(*_args(pc, openings, compress))
    return key.check(*b.finish(fr_mont_limbs(pc, weights)))


# ---- 1. verdicts ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("compress", [True, False])
@pytest.mark.parametrize("cid", [0, 1])
def test_verdicts_equal_the_trapdoor_formula(world, mj, cid, compress):
    w = world[cid]
    c, pc, r, beta, pool, key = mj.params.CURVES[cid], w["pc"], w["pc"].r, w["beta"], w["pool"], w["keys"][compress]
    rng = random.Random(61 + cid)
    for o in pool[:11]:                                                    # the real openings, one by one: weight 1
        assert mj.UnivariateKzgPCS.verify(key, *[a[0] for a in _args(pc, [o], compress)]) is _accepts(r, beta, [o], [1]) is True
    for K in SIZES:
        good = pool[:K]
        k = rng.randrange(K)
        bad = good[:k] + [good[k].replace(v=(good[k].v + 1) % r)] + good[k + 1:]
        drawn, own = _drawn_weights(mj, K), [rng.randrange(1, r) for _ in range(K)]
        assert drawn[0] == 1 and all(1 < t < 1 << 128 for t in drawn[1:])
        for openings in (good, bad):
            want = openings is good
            assert _accepts(r, beta, openings, drawn) is _accepts(r, beta, openings, own) is want
            assert _batch_verify(mj, key, pc, openings, compress) is want, K
            assert _c_level(mj, key, pc, openings, own, compress) is want, K
    # the stage's outputs: the unweighted row (1, z), the evaluation v, a zero key row
    b = key.begin_openings(*_args(pc, pool[:65], compress))
    kr, pr, ev = b.scalars()
    b.discard()
    assert kr.shape == (65, 1, 4) and not kr.any() and pr.shape == (65, 2, 4)
    assert fr_from_mont_limbs(c, pr.reshape(-1, 4)) == [x for o in pool[:65] for x in (1, o.z)]
    assert fr_from_mont_limbs(c, ev) == [o.v for o in pool[:65]]
    assert mj.UnivariateKzgPCS.batch_verify(key, [], [], [], [], mj.rng.ChaChaRng(SEED, 20)) is True
    with pytest.raises(mj.PCSError):
        mj.UnivariateKzgPCS.batch_verify(key, *_args(pc, pool[:2], compress)[:3], [b""], mj.rng.ChaChaRng(SEED, 20))


def test_commitment_objects_are_written_in_the_keys_mode(world, mj):
    """Commitment objects in place of records, under both modes; verifier_param of a deserialized setup is the same open key"""
    cid = 1
    w = world[cid]
    c, pc, pool = mj.params.CURVES[cid], w["pc"], w["pool"]
    from conftest import affine_limbs
    cm = lambda p: mj.Commitment(c, affine_limbs(pc, [p])[0])
    for compress in (True, False):
        key = w["keys"][compress]
        enc = _enc(pc, compress)
        for o in (pool[0], pool[6], pool[8]):
            assert mj.kzg.g1_record(c, cm(o.C), compress) == enc(o.C) and mj.kzg.g1_record(c, cm(o.W), compress) == enc(o.W)
            assert mj.UnivariateKzgPCS.verify(key, cm(o.C), o.z, o.v, cm(o.W)) is True
            assert mj.UnivariateKzgPCS.verify(key.verifier(), cm(o.C), o.z, (o.v + 1) % pc.r, enc(o.W)) is False
        pp = mj.UnivariateProverParam.gen_srs_for_testing(c, w["beta"], 3)
        g, h, beta_h = mj.kzg.open_key_for_testing(c, w["beta"], compress=compress)
        vp = mj.UnivariateUniversalParams(pp, h, beta_h, compress).verifier_param()
        assert isinstance(vp, mj.keys.OpenKey) and (vp.g, vp.h, vp.beta_h, vp.compressed) == (g, h, beta_h, compress)
        pp.release()


# ---- 2. tampers -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", [0, 1])
def test_each_single_tamper_is_rejected(world, mj, cid):
    w = world[cid]
    pc, r, beta, pool, key = w["pc"], w["pc"].r, w["beta"], w["pool"], w["keys"][True]
    verify = lambda o: mj.UnivariateKzgPCS.verify(key, *[a[0] for a in _args(pc, [o])])
    for o in (pool[3], pool[4], pool[20]):
        other = pool[21]
        for bad in (o.replace(v=(o.v + 1) % r), o.replace(z=(o.z + 1) % r), o.swapped(), o.replace(w=other.w, W=other.W)):
            assert verify(bad) is _accepts(r, beta, [bad], [1]) is False
        assert verify(o) is True
    good = pool[:65]
    drawn = _drawn_weights(mj, 65)
    for k in (0, 31, 64):
        openings = good[:k] + [good[k].replace(z=(good[k].z + 1) % r)] + good[k + 1:]
        assert _batch_verify(mj, key, pc, openings) is _accepts(r, beta, openings, drawn) is False, k


# ---- 3. the weights -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", [0, 1])
def test_the_weights_are_applied(world, mj, cid):
    """two false openings whose errors cancel under (1, 1): accepted there -- that is the formula -- and rejected under the drawn weights"""
    w = world[cid]
    pc, r, beta, pool, key = w["pc"], w["pc"].r, w["beta"], w["pool"], w["keys"][True]
    pair = [pool[3].replace(v=(pool[3].v + 1) % r), pool[12].replace(v=(pool[12].v - 1) % r)]
    assert all(o.error(r, beta) for o in pair)
    assert _c_level(mj, key, pc, pair, [1, 1]) is _accepts(r, beta, pair, [1, 1]) is True
    assert _batch_verify(mj, key, pc, pair) is _accepts(r, beta, pair, _drawn_weights(mj, 2)) is False
    assert _c_level(mj, key, pc, pair, [1, 2]) is False


# ---- 4. refusals ----------------------------------------------------------------------------------------------------------------------------
def _off_subgroup(pc):
    """a point of E(Fq) outside G1 on BLS12-381 (q = 3 mod 4; the cofactor is ~2^126, so the first point found is outside)"""
    for x in range(1, 100):
        a = (x ** 3 + 4) % pc.q
        y = pow(a, (pc.q + 1) // 4, pc.q)
        if y * y % pc.q == a:
            return x, y


@pytest.mark.parametrize("cid", [0, 1])
def test_malformed_openings_are_refused_with_field_and_lowest_index(world, mj, pyref, cid):
    w = world[cid]
    c, pc, r, beta, pool = mj.params.CURVES[cid], w["pc"], w["pc"].r, w["beta"], w["pool"]
    key = mj.keys.OpenKey(c, *mj.kzg.open_key_for_testing(c, beta))
    good = pool[:5]

    def refused(openings, index, field, reason, records=None, validate=True):
        cms, zs, vs, pfs = _args(pc, openings)
        for i, (cm, pf) in (records or {}).items():
            cms[i], pfs[i] = cm or cms[i], pf or pfs[i]
        for _ in range(2):                                                 # the same answer on every run
            with pytest.raises(mj.keys.ProofEncodingError) as e:
                key.begin_openings(cms, zs, vs, pfs, validate)
            assert isinstance(e.value, mj.SerializationError)
            assert (e.value.index, e.value.field, e.value.reason) == (index, field, f"opening {index}: {field}: {reason}")

    for big in (r, 2 ** 256 - 1):
        refused(good[:3] + [good[3].replace(v=big)] + good[4:], 3, "value", "not below the modulus")
        refused(good[:2] + [good[2].replace(z=big)] + good[3:], 2, "point", "not below the modulus")
    off = _x_off_the_curve(c, pc)
    refused(good, 1, "commitment", "x^3 + b is not a square", {1: (off, None)})
    refused(good, 4, "proof", "x^3 + b is not a square", {4: (None, off)})
    flags = bytearray(FS.g1_bytes(pc, good[0].W))
    if cid == 0:
        flags[0] &= 0x7F                                                   # the compressed bit cleared
    else:
        flags[-1] |= 0xC0
    refused(good, 0, "proof", "invalid flag bits", {0: (None, bytes(flags))})
    if cid == 0:
        rec = FS.g1_bytes(pc, _off_subgroup(pc))
        refused(good, 2, "commitment", "not in the subgroup", {2: (rec, None)})
        cms, zs, vs, pfs = _args(pc, good)
        b = key.begin_openings(cms[:2] + [rec] + cms[3:], zs, vs, pfs, validate=False)     # unchecked: decodes, and the opening is false
        assert key.check(*b.finish(fr_mont_limbs(pc, [1, 2, 3, 4, 5]))) is False
    # two bad openings: the lowest index, and within one opening its first field
    refused(good[:1] + [good[1].replace(v=r)] + good[2:4] + [good[4].replace(z=r)], 1, "value", "not below the modulus", {4: (off, None)})
    refused(good[:3] + [good[3].replace(z=r, v=r)] + good[4:], 3, "point", "not below the modulus")
    refused(good[:3] + [good[3].replace(z=r)] + good[4:], 3, "proof", "x^3 + b is not a square", {3: (None, off)})
    with pytest.raises(mj.keys.ProofEncodingError) as e:
        key.begin_openings([b"short"], [0], [0], [FS.g1_bytes(pc, None)])
    assert (e.value.index, e.value.field) == (0, "commitment")
    key.release()                                                         # mzk_verifier_destroy succeeds: no batch was left open


@pytest.mark.parametrize("cid", [0, 1])
def test_host_side_refusals_and_handle_rules(world, mj, cid):
    w = world[cid]
    c, pc, beta, pool = mj.params.CURVES[cid], w["pc"], w["beta"], w["pool"]
    key = mj.keys.OpenKey(c, *mj.kzg.open_key_for_testing(c, beta))
    v = key.verifier()
    L = mj.load()
    ptr = lambda a: C.c_void_p(a.ctypes.data)
    cms, zs, vs, pfs = _args(pc, pool[:1])
    recs = np.frombuffer(cms[0] + pfs[0], dtype=np.uint8)
    z, val = (np.frombuffer(x[0].to_bytes(32, "little"), dtype=np.uint64) for x in (zs, vs))
    out = C.c_uint64()

    def launches():
        n = C.c_uint64()
        assert L.mzk_launch_count(C.byref(n)) == 0
        return n.value
    before = launches()
    assert L.mzk_verifier_open_begin(v.handle, ptr(recs), 0, ptr(z), ptr(val), 0, C.byref(out), None) == ERR_INVALID_ARG       # K = 0
    for flags in (1, 4, 1 << 31):                                          # MZK_SER_COMPRESSED, MZK_TRANSCRIPT_SOLIDITY, a stray bit
        assert L.mzk_verifier_open_begin(v.handle, ptr(recs), 1, ptr(z), ptr(val), flags, C.byref(out), None) == ERR_INVALID_ARG
    assert launches() == before
    with pytest.raises(ValueError):
        v.begin_openings([], [], [], [])
    # an open openings batch holds its verifier; the three calls of the other kinds refuse it and name the kind
    b = key.begin_openings(cms, zs, vs, pfs)
    assert L.mzk_verifier_destroy(v.handle) == ERR_INVALID_ARG and b"open batch" in L.mzk_last_error()
    buf = np.zeros(64, dtype=np.uint64)
    assert L.mzk_verifier_batch_challenges(b.handle, ptr(buf)) == ERR_INVALID_ARG and b"openings batch" in L.mzk_last_error()
    assert L.mzk_verifier_link_values(b.handle, ptr(buf), None) == ERR_INVALID_ARG and b"openings batch" in L.mzk_last_error()
    assert L.mzk_verifier_link_weights(b.handle, None, ptr(buf)) == ERR_INVALID_ARG and b"openings batch" in L.mzk_last_error()
    handle = b.handle
    b.discard()                                                            # closes it
    assert L.mzk_verifier_batch_scalars(handle, None, None, None) == ERR_BAD_HANDLE
    key.release()
    assert v.handle == 0


# ---- 5. summation across kinds --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", [0, 1])
def test_an_openings_group_and_a_link_group_in_one_check(world, mj, pyref, cid):
    """one openings group and one synthetic link group (the fixture pattern of test_link_verify_gpu) under one open key, no weight 1"""
    import pyref_linking as LK
    w = world[cid]
    pc, r, beta, pool, key = w["pc"], w["pc"].r, w["beta"], w["pool"], w["keys"][True]
    rng = random.Random(88 + cid)
    links = _synthetic(pc, pyref, LK, rng, (4, 2, 9), beta)
    assert links["valid"].verdict and not links["one point"].verdict
    opens = pool[2:5]
    false_open = opens[:1] + [opens[1].replace(v=(opens[1].v + 1) % r)] + opens[2:]
    weights = [rng.randrange(2, r) for _ in range(3)]
    s = fr_mont_limbs(pc, [rng.randrange(2, r)])[0]

    def check(openings, link):
        bo = key.begin_openings(*_args(pc, openings))
        bl = key.begin_links([link.tuple(mj)] * 2)
        lw = bl.link_weights(s)
        assert 1 not in fr_from_mont_limbs(pc, lw)
        Ao, Bo = bo.finish(fr_mont_limbs(pc, weights))
        Al, Bl = bl.finish(lw)
        return key.check(np.stack([Ao, Al]), np.stack([Bo, Bl]))
    assert check(opens, links["valid"]) is True
    assert check(false_open, links["valid"]) is False
    assert check(opens, links["one point"]) is False
