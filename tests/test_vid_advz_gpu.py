"""GPU: the ADVZ VID scheme (mpc-jellyfish_amd/vid.py over mzk_vid_advz_*_dev, csrc/vid.hip) against the test-side restatement
(tests/advz_ref.py): every field of a dispersal exactly, verify_share / verify_shares on the reference's happy and sad paths
(advz.rs:563-683), recovery from four selections of shares, the refusals.  The shapes are the smallest at which each kernel can still go
wrong: tree heights 1 to 4, a top level with one real child, n = N / 2 and n < N / 2, k a power of two and not, both parities of K (leaf
messages ending at 48 and 16 mod 64), a short last polynomial, a last polynomial that is zero after its length element, a zero polynomial
(a commitment at infinity) and the empty payload.  Per curve one SRS; every dispersal and its restatement are computed once and shared."""
import random

import numpy as np
import pytest

import advz_ref
from conftest import affine_from_limbs

pytestmark = pytest.mark.gpu

SHAPES = ((1, 1), (2, 3), (2, 4), (3, 5), (4, 4), (4, 10), (8, 28))
HEIGHTS = {1: 1, 3: 2, 4: 2, 5: 2, 10: 3, 28: 4}
DOMAINS = {(1, 1): 4, (2, 3): 8, (2, 4): 8, (3, 5): 8, (4, 4): 16, (4, 10): 16, (8, 28): 32}
# (k, n, payload bytes, K)
CASES = ((1, 1, 0, 0), (1, 1, 1, 2), (1, 1, 63, 4),
         (2, 3, 30, 1), (2, 3, 31, 1), (2, 3, 62, 1),
         (2, 4, 32, 2), (2, 4, 61, 2),
         (3, 5, 63, 2), (3, 5, 0, 0),
         (4, 4, 31 * 4 + 5, 2), (4, 4, 1, 1),
         (4, 10, 31 * 9 + 3, 3), (4, 10, 31 * 17 + 1, 5),
         (8, 28, 31 * 5 + 2, 1), (8, 28, 31 * 10 + 4, 2), (8, 28, 31 * 15 + 7, 3))
ZERO_CASE = (2, 3, "zeros")                                           # 31 zero bytes: one zero polynomial, its commitment at infinity
ROUND_TRIP = lambda n: n % 31 != 0 or n in (0, 31)


def _payload(rng, n):
    return bytes(rng.randrange(256) for _ in range(n))


def _pt(pc, cm):
    return None if cm.is_infinity() else affine_from_limbs(pc, cm.xy)


@pytest.fixture(scope="module")
def world(gpu, mj, pyref):
    out = {}
    for cid in (0, 1):
        c, pc = mj.params.CURVES[cid], pyref.CURVES[cid]
        rng = random.Random(9100 + cid)
        beta = rng.randrange(1, pc.r)
        pp = mj.UnivariateProverParam.gen_srs_for_testing(c, beta, 16)                # checked_fft_size(8)
        key = mj.keys.OpenKey(c, *mj.kzg.open_key_for_testing(c, beta))
        schemes = {(k, n): mj.Advz(c, k, n, pp, key) for k, n in SHAPES}
        cases = {}
        for k, n, size, K in CASES + (ZERO_CASE + (1,),):
            payload = bytes(31) if size == "zeros" else _payload(rng, size)
            elems = advz_ref.bytes_to_field(payload)
            cases[(k, n, size)] = dict(payload=payload, elems=elems, got=schemes[(k, n)].disperse(payload), want=advz_ref.disperse(pc, k, n, beta, elems),
                                       vid=schemes[(k, n)], k=k, n=n, K=K)
        out[cid] = dict(c=c, pc=pc, beta=beta, pp=pp, key=key, schemes=schemes, cases=cases)
    yield out
    for w in out.values():
        w["key"].release()
        w["pp"].release()


ALL = [(k, n, size) for k, n, size, _ in CASES] + [ZERO_CASE]


@pytest.mark.parametrize("cid", [0, 1])
def test_shapes_domains_and_heights(world, mj, cid):
    w = world[cid]
    for (k, n), vid in w["schemes"].items():
        assert vid.domain.size == DOMAINS[(k, n)] and vid.height == HEIGHTS[n] == advz_ref.tree_height(n)
        assert vid.ck.length == mj.checked_fft_size(k) + 1
    with pytest.raises(mj.VidError) as e:
        mj.Advz(w["c"], 4, 3, w["pp"], w["key"])
    assert e.value.kind == "Argument"


@pytest.mark.parametrize("cid", [0, 1])
@pytest.mark.parametrize("case", ALL, ids=str)
def test_disperse_matches_the_restatement_field_by_field(world, cid, case):
    w = world[cid]
    pc, d = w["pc"], w["cases"][case]
    got, want, n, K = d["got"], d["want"], d["n"], d["K"]
    assert len(want["commits"]) == K == len(got.common.poly_commits) and len(got.shares) == n
    assert got.common.elems_len == len(d["elems"]) == want["elems_len"]
    assert [_pt(pc, cm) for cm in got.common.poly_commits] == want["commits"]
    assert got.common.all_evals_digest == want["root"]
    assert got.commit == want["commit"]
    for i, sh in enumerate(got.shares):
        assert sh.index == i and sh.evals == want["evals"][i], i
        assert [[bytes(s) for s in level] for level in np.asarray(sh.evals_proof)] == want["paths"][i], i
        assert _pt(pc, sh.aggregate_proof) == want["proofs"][i], i
    assert w["schemes"][(d["k"], n)].commit_only(d["payload"]) == got.commit
    if case == ZERO_CASE:
        assert got.common.poly_commits[0].is_infinity() and all(sh.aggregate_proof.is_infinity() for sh in got.shares)
    if K == 0:
        assert all(sh.aggregate_proof.is_infinity() and sh.evals == [] for sh in got.shares)


@pytest.mark.parametrize("cid", [0, 1])
def test_pseudorandom_scalar_is_the_restated_one(world, mj, cid):
    w = world[cid]
    d = w["cases"][(4, 10, 31 * 9 + 3)]
    assert mj.params.fr_from_mont(w["c"], d["vid"].pseudorandom_scalar(d["got"].common)[None])[0] == d["want"]["s"]


@pytest.mark.parametrize("cid", [0, 1])
@pytest.mark.parametrize("case", ALL, ids=str)
def test_every_share_verifies(world, cid, case):
    d = world[cid]["cases"][case]
    vid, got = d["vid"], d["got"]
    assert vid.verify_shares(got.shares, got.common) == [True] * d["n"]
    assert vid.verify_share(got.shares[-1], got.common) is True
    for sh, path in zip(got.shares, d["want"]["paths"]):                      # ... and the restated tree accepts the device's paths
        assert advz_ref.tree_verify(got.common.all_evals_digest, sh.index, sh.evals, [[bytes(s) for s in level] for level in np.asarray(sh.evals_proof)])


def _copy(mj, share, **kw):
    f = dict(index=share.index, evals=list(share.evals), aggregate_proof=share.aggregate_proof, evals_proof=np.array(share.evals_proof, copy=True))
    f.update(kw)
    return mj.vid.Share(**f)


@pytest.mark.parametrize("cid", [0, 1])
@pytest.mark.parametrize("case", [(3, 5, 63), (4, 10, 31 * 9 + 3), (8, 28, 31 * 10 + 4)], ids=str)
def test_sad_paths_are_refused(world, mj, cid, case):
    """advz.rs:563-683.  k >= 3: the witness of a polynomial of two coefficients is the same constant at every point, so at k = 2 another
    share's proof IS this share's proof."""
    w = world[cid]
    d = w["cases"][case]
    vid, got, n, r = d["vid"], d["got"], d["n"], w["pc"].r
    sh, other = got.shares[1], got.shares[2]
    bad = {"doubled eval": _copy(mj, sh, evals=[2 * sh.evals[0] % r] + sh.evals[1:]),
           "index shift": _copy(mj, sh, index=(sh.index + 1) % n),
           "index + n": _copy(mj, sh, index=sh.index + n),
           "another path": _copy(mj, sh, evals_proof=other.evals_proof),
           "another proof": _copy(mj, sh, aggregate_proof=other.aggregate_proof)}
    for name, share in bad.items():
        assert vid.verify_share(share, got.common) is False, name
    assert vid.verify_shares(list(bad.values()), got.common) == [False] * len(bad)
    commits = list(got.common.poly_commits)
    commits[0] = got.shares[0].aggregate_proof                                # another point of the curve
    for name, common in (("commitment", mj.vid.Common(commits, got.common.all_evals_digest, got.common.elems_len)),
                         ("root", mj.vid.Common(got.common.poly_commits, bytes(32 - 1) + b"\x01", got.common.elems_len))):
        assert vid.verify_share(sh, common) is False, name
        assert vid.verify_shares(got.shares, common) == [False] * n, name
    with pytest.raises(mj.VidError) as e:                                     # a missing eval: the one argument error
        vid.verify_share(_copy(mj, sh, evals=sh.evals[:-1]), got.common)
    assert e.value.kind == "Argument"
    with pytest.raises(mj.VidError):
        vid.verify_shares([sh, _copy(mj, sh, evals=sh.evals + [0])], got.common)
    # one bad share among good ones: the batch check fails, the one-by-one pass names it
    mixed = list(got.shares)
    mixed[1] = bad["another proof"]
    assert vid.verify_shares(mixed, got.common) == [True, False] + [True] * (n - 2)
    assert vid.verify_shares(got.shares, got.common) == [True] * n            # (the cached aggregate commitment of the good Common is untouched)


def _selections(k, n):
    rng = random.Random(31 * k + n)
    scattered = sorted(rng.sample(range(n), k), key=lambda i: (i * 7) % n)
    return {"first k": list(range(k)), "last k": list(range(n - k, n)), "scattered": scattered, "all n": list(range(n))}


@pytest.mark.parametrize("cid", [0, 1])
@pytest.mark.parametrize("case", ALL, ids=str)
def test_recover_from_four_selections(world, cid, case):
    w = world[cid]
    pc, d = w["pc"], w["cases"][case]
    vid, got, k, n = d["vid"], d["got"], d["k"], d["n"]
    for name, sel in _selections(k, n).items():
        shares = [got.shares[i] for i in sel]
        want = advz_ref.recover_elems(pc, [(s.index, s.evals) for s in shares], k, n, got.common.elems_len)
        assert want == d["elems"], name                                       # the restated decoder recovers the elements
        assert vid.recover_elems(shares, got.common) == want, name
        payload = vid.recover_payload(shares, got.common)
        assert payload == advz_ref.field_to_bytes(want), name
        if ROUND_TRIP(len(d["payload"])):
            assert payload == d["payload"], name
    if not ROUND_TRIP(len(d["payload"])):
        assert vid.recover_payload(got.shares, got.common) != d["payload"]    # 62 bytes: the reference's field_to_bytes does not invert


@pytest.mark.parametrize("cid", [0, 1])
def test_recover_refusals_come_before_any_launch(world, mj, cid):
    w = world[cid]
    d = w["cases"][(4, 10, 31 * 9 + 3)]
    vid, got = d["vid"], d["got"]
    L = mj.load()
    import ctypes as C
    launches = lambda: (lambda v: (L.mzk_launch_count(C.byref(v)), v.value)[1])(C.c_uint64())
    before = launches()
    for shares in (got.shares[:3],                                                               # fewer than k
                   got.shares[:3] + [_copy(mj, got.shares[3], evals=got.shares[3].evals[:-1])],       # unequal eval lengths
                   got.shares[:4] + [_copy(mj, got.shares[4], index=vid.domain.size)],                # an index >= N, beyond the first k
                   [got.shares[0], got.shares[1], _copy(mj, got.shares[1]), got.shares[2]]):          # a duplicate among the first k
        with pytest.raises(mj.VidError):
            vid.recover_elems(shares, got.common)
    assert launches() == before
    # a duplicate beyond the first k is not looked at, as in the reference
    assert vid.recover_elems(got.shares[:4] + [got.shares[0]], got.common) == d["elems"]


@pytest.mark.parametrize("cid", [0, 1])
def test_payload_kinds_and_elements_give_identical_results(world, mj, cid):
    import torch
    w = world[cid]
    d = w["cases"][(3, 5, 63)]
    vid, got = d["vid"], d["got"]
    as_np = np.frombuffer(d["payload"], dtype=np.uint8)
    for other in (vid.disperse(as_np), vid.disperse(torch.from_numpy(as_np.copy()).cuda()), vid.disperse_from_elems(d["elems"])):
        assert other.commit == got.commit and other.common.poly_commits == got.common.poly_commits
        assert other.common.all_evals_digest == got.common.all_evals_digest and other.common.elems_len == got.common.elems_len
        for a, b in zip(other.shares, got.shares):
            assert a.index == b.index and a.evals == b.evals and a.aggregate_proof == b.aggregate_proof and np.array_equal(a.evals_proof, b.evals_proof)
    assert vid.commit_only(as_np) == vid.commit_only(torch.from_numpy(as_np.copy()).cuda()) == got.commit


@pytest.mark.parametrize("cid", [0, 1])
def test_bytes_to_field_and_back_on_the_device(world, mj, cid):
    c = world[cid]["c"]
    rng = random.Random(5)
    for n in (0, 1, 30, 31, 32, 61, 62, 63, 93, 31 * 300 + 17):                   # the last: more than one workgroup
        p = _payload(rng, n)
        t = mj.vid.bytes_to_field(c, p)
        elems = mj.params.fr_from_mont(c, t.cpu().numpy().view(np.uint64)) if t.shape[0] else []
        assert elems == advz_ref.bytes_to_field(p), n
        assert mj.vid.field_to_bytes(c, t) == advz_ref.field_to_bytes(elems), n
    import torch
    buf = torch.from_numpy(np.frombuffer(b"\xff" + _payload(rng, 100), dtype=np.uint8).copy()).cuda()
    t = mj.vid.bytes_to_field(c, buf[1:])                                         # a payload at an odd address
    assert mj.params.fr_from_mont(c, t.cpu().numpy().view(np.uint64)) == advz_ref.bytes_to_field(bytes(buf[1:].cpu().numpy()))


def test_entry_points_refuse_bad_arguments(world, mj):
    import ctypes as C
    L = mj.load()
    w = world[0]
    pp = w["pp"]
    out32, limbs, n = (C.c_uint8 * 32)(), (C.c_uint64 * 4)(), C.c_uint64()
    assert L.mzk_vid_advz_commit_only_dev(pp.handle, 0, pp.length, None, 0, 4, 3, 4, out32, None) == -1          # n < k
    assert L.mzk_vid_advz_commit_only_dev(pp.handle, 0, pp.length, None, 0, 0, 3, 4, out32, None) == -1          # k = 0
    assert L.mzk_vid_advz_commit_only_dev(pp.handle, 0, pp.length + 1, None, 0, 2, 3, 3, out32, None) == -1      # a view outside the SRS
    assert L.mzk_vid_advz_commit_only_dev(pp.handle, 0, pp.length, None, 0, 2, 9, 3, out32, None) == -1          # n above the domain
    assert L.mzk_vid_advz_commit_only_dev(pp.handle, 0, pp.length, None, 0, 2, 3, 40, out32, None) == -5         # log_domain above the cap
    assert L.mzk_vid_advz_commit_only_dev(pp.handle, 0, pp.length, None, 5, 2, 3, 3, out32, None) == -1          # elements without a pointer
    assert L.mzk_vid_advz_commit_only_dev(pp.handle, 0, pp.length, None, 0, 2, 3, 3, None, None) == -1
    assert L.mzk_vid_advz_commit_only_dev(12345, 0, 1, None, 0, 2, 3, 3, out32, None) == -4
    assert L.mzk_bytes_to_field_dev(0, None, 5, None, None) == -1
    assert L.mzk_field_to_bytes_dev(0, None, 5, None, C.byref(n), None) == -1
    idx = (C.c_uint64 * 2)(0, 0)
    assert L.mzk_vid_advz_recover_dev(0, 2, 0, 3, idx, None, None, None) == -1                                   # a duplicate index
    idx = (C.c_uint64 * 2)(0, 8)
    assert L.mzk_vid_advz_recover_dev(0, 2, 0, 3, idx, None, None, None) == -1                                   # an index >= N
    big = (C.c_uint64 * 1025)(*range(1025))
    assert L.mzk_vid_advz_recover_dev(0, 1025, 0, 11, big, None, None, None) == -5                               # k above the cap
    assert L.mzk_vid_advz_verify_shares_dev(0, 1, 0, 3, None, None, None, out32, limbs, None, None, None) == -1
