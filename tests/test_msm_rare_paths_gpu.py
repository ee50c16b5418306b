"""GPU: the RARE paths of the MSM at exact, chosen bucket loads -- over-long buckets (chunk descriptors, msm_long_*), heavy buckets
(level-1 runs and the LDS trees, msm_heavy_*) and the retry after an overflow of their optimistically sized scratch (csrc/msm.hip,
MSM_RETRY).  The regular path is pinned elsewhere; here every scalar vector is BUILT so that named buckets hold a load on a threshold
of that machinery: cap, cap + 1, cap + MSM_HEAVY_RUN (+ 1), whole and short level-1 runs, threads with 16, 1 or 0 entries.

How the loads are exact: scalars are canonical, and a scalar of value d with 1 <= d < 2^(c-1) has ONE non-zero signed digit, d, in
the lowest window -- so bucket d of that window (the table path: of the one bucket set) holds as many entries as there are scalars
equal to d.  The thresholds themselves (cap, descriptor and level-1 capacities) are READ from the library after a dense probe call of
the same size and path (mzk_msm_last_shape, mzk_msm_last_rare), never restated; every test asserts what it needs of them, so a change
of the sizing policy fails a test instead of hollowing it out.  Every result is compared bit for bit with the C oracle."""
import ctypes as C
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N = (1 << 17) + 5
HEAVY_RUN = 2048                     # csrc/msm.cuh MSM_HEAVY_RUN = 128 threads x 16 entries (fixed by the kernels' shape, not by sizing policy)


def scalars_with_loads(n, loads, values, rng, by_parity=False):
    """(n, 4) uint64 canonical scalars: loads[k] copies of the integer values[k] at shuffled positions, zeros elsewhere.  Shuffled, so
    that the chunks of a bucket are not runs of neighbouring base indices.  by_parity: ceil(L/2) of a load's copies at even positions,
    floor(L/2) at odd ones (bases that alternate P, -P by index parity)."""
    assert len(loads) == len(values) and len(set(values)) == len(values) and sum(loads) <= n
    out = np.zeros((n, 4), dtype=np.uint64)
    limbs = np.array([[(v >> (64 * j)) & 0xFFFFFFFFFFFFFFFF for j in range(4)] for v in values], dtype=np.uint64)
    if by_parity:
        pos = [rng.permutation(np.arange(0, n, 2)), rng.permutation(np.arange(1, n, 2))]
        used = [0, 0]
        for k, L in enumerate(loads):
            for par, cnt in ((0, (L + 1) // 2), (1, L // 2)):
                out[pos[par][used[par]:used[par] + cnt]] = limbs[k]
                used[par] += cnt
        assert used[0] <= len(pos[0]) and used[1] <= len(pos[1])
    else:
        pos = rng.permutation(n)
        at = 0
        for k, L in enumerate(loads):
            out[pos[at:at + L]] = limbs[k]
            at += L
    return out


def ladder_loads(cap):
    """One bucket at each threshold of the over-long / heavy machinery (csrc/msm.cuh), lightest first."""
    assert 3 <= cap and 2 * cap + 1 < cap + HEAVY_RUN - 1 and cap + HEAVY_RUN + 1 < 4096, cap
    return [1,                                                         # (strictly increasing under the assertion above: all distinct)
            cap - 1, cap, cap + 1,                                     # the cap itself; one chunk of length 1
            2 * cap - 1, 2 * cap, 2 * cap + 1,                         # a full first chunk; a second chunk of length 1
            cap + HEAVY_RUN - 1, cap + HEAVY_RUN,                      # the longest over-long bucket
            cap + HEAVY_RUN + 1,                                       # the smallest heavy bucket: two level-1 runs, the second of cap + 1 entries
            4096, 4097,                                                # two whole runs; a last run of ONE entry (one thread with one entry)
            4096 + 16, 4096 + 17,                                      # a last run of one whole thread; of a whole thread and one entry
            cap + HEAVY_RUN + 3 * HEAVY_RUN]


def ladder_values(c_bits, count):
    """`count` distinct bucket values below 2^(c-1), spread over the bucket range (both ends included)."""
    M = 1 << (c_bits - 1)
    vals = [1, 2, M - 1, M - 2] + [3 + (k * 2654435761) % (M - 6) for k in range(count)]
    out = []
    for v in vals:
        if v not in out:
            out.append(v)
    assert len(out) >= count and max(out) < M and min(out) >= 1
    return out[:count]


@functools.lru_cache(maxsize=None)
def _bases(curve_id, n=N):
    import cref
    b = cref.g1_arith_bases(curve_id, 0xbeef, 0x2b, n)
    b.setflags(write=False)
    return b


@functools.lru_cache(maxsize=None)
def _dense(curve_id, n=N):
    import mpc_jellyfish_amd as mj
    d = mj.params.random_fr_mont(mj.params.CURVES[curve_id], n, seed=41)      # (arbitrary values < r, used as canonical scalars)
    d.setflags(write=False)
    return d


_ORACLE = {}


def _want(cref, curve_id, key, bases, scalars):
    """The C oracle's affine point for (bases, scalars), computed once per key and shared among the tests."""
    if (curve_id, key) not in _ORACLE:
        _ORACLE[(curve_id, key)] = cref.jac_to_affine(curve_id, cref.msm(curve_id, bases, scalars, scalars_are_mont=False, threads=8))[0]
    return _ORACLE[(curve_id, key)]


def _aff(cref, curve_id, jac):
    return cref.jac_to_affine(curve_id, jac)[0]


def _ws_bytes(mj):
    ws = C.c_uint64()
    mj.lib.check(mj.load().mzk_workspace_hbm_bytes(C.byref(ws)), "mzk_workspace_hbm_bytes")
    return ws.value


def _probe(mj, pp, dense, batch=0):
    """Sizing of a dense call (batch = 0) or a dense batch of `batch` MSMs: (c, M, cap, desc_cap, h1_cap)."""
    if batch:
        mj.msm_bigint_batch(pp, [dense] * batch, scalars_are_mont=False)
    else:
        mj.msm_bigint(pp, dense, scalars_are_mont=False)
    c_bits, _, M = mj.lib.msm_last_shape()
    cap, desc_cap, h1_cap, attempts = mj.lib.msm_last_rare()
    assert attempts == 1 and M == 1 << (c_bits - 1) and cap >= 1
    return c_bits, M, cap, desc_cap, h1_cap


def _ladder(mj, pp, curve_id, table):
    """The ladder's loads and bucket values for this curve and path, and the cap they were built from."""
    c_bits, M, cap, desc_cap, h1_cap = _probe(mj, pp, _dense(curve_id))
    loads = ladder_loads(cap)
    # the table path's cap may be too large for the whole ladder: rungs go from the top, never one up to the smallest heavy bucket
    while sum(loads) > N:
        loads.pop()
    assert cap + HEAVY_RUN + 1 in loads, ("every rung up to cap + MSM_HEAVY_RUN + 1 must fit", cap, sum(loads))
    values = ladder_values(c_bits, len(loads))
    assert max(values) < 1 << (c_bits - 1)
    print("sizing: curve", curve_id, "table" if table else "plain", "single c", c_bits, "M", M, "cap", cap, "desc_cap", desc_cap, "h1_cap", h1_cap,
          "rungs", len(loads), "entries", sum(loads))
    return loads, values, cap


# ---- one bucket at every threshold load ----------------------------------------------------------------
@pytest.mark.parametrize("table", [1, 0])
@pytest.mark.parametrize("curve_id", [0, 1])
def test_bucket_load_ladder(gpu, mj, cref, curve_id, table):
    """One bucket at every threshold load in ONE scalar vector, as a single call (one worst-case scratch slot) and as the batch
    [ladder, dense, ladder] (the deferred rare-path launches, a slot per MSM).  An off-by-one at any threshold drops or double-counts one
    point of one bucket; the oracle's sum then differs."""
    bases = _bases(curve_id)
    pp = mj.UnivariateProverParam.from_affine(curve_id, bases)
    L = mj.load()
    L.mzk_msm_set_precompute(table)
    try:
        loads, values, cap = _ladder(mj, pp, curve_id, table)
        sc = scalars_with_loads(N, loads, values, np.random.default_rng(7))
        want = _want(cref, curve_id, ("ladder", table, cap), bases, sc)
        want_dense = _want(cref, curve_id, "dense", bases, _dense(curve_id))
        got = _aff(cref, curve_id, mj.msm_bigint(pp, sc, scalars_are_mont=False))
        assert mj.lib.msm_last_rare()[0] == cap and mj.lib.msm_last_rare()[3] == 1            # (a single call never overflows: worst-case slot)
        pts, tab = C.c_uint64(), C.c_uint64()
        mj.lib.check(L.mzk_srs_hbm_bytes(pp.handle, C.byref(pts), C.byref(tab)), "mzk_srs_hbm_bytes")
        assert (tab.value > 0) == bool(table), "the fixed-base table decides the path: built for the table path only"
        assert np.array_equal(got, want), (curve_id, table, "single")
        jac = mj.msm_bigint_batch(pp, [sc, _dense(curve_id), sc], scalars_are_mont=False)
        b_cap, b_desc_cap, b_h1_cap, attempts = mj.lib.msm_last_rare()
        print("sizing: curve", curve_id, "table" if table else "plain", "batch3 cap", b_cap, "desc_cap", b_desc_cap, "h1_cap", b_h1_cap, "attempts", attempts)
        assert b_cap == cap, "the batch must size its chains like the single call the ladder was built for"
        for i, w in enumerate((want, want_dense, want)):
            assert np.array_equal(_aff(cref, curve_id, jac[i]), w), (curve_id, table, "batch", i)
    finally:
        L.mzk_msm_set_precompute(1)
        pp.release()


# ---- the same loads in every window ------------------------------------------------------------------
@pytest.mark.parametrize("table", [1, 0])
def test_ladder_in_every_window(gpu, mj, cref, table):
    """The ladder's loads on fixed-seed FULL-WIDTH values < r: every window sees them -- the short top one too -- and the table path gets
    all its levels in one bucket set.  Digit collisions merge buckets, so the loads are lower bounds here; the oracle is the assertion."""
    curve_id = 0
    c = mj.params.CURVES[curve_id]
    bases = _bases(curve_id)
    pp = mj.UnivariateProverParam.from_affine(curve_id, bases)
    L = mj.load()
    L.mzk_msm_set_precompute(table)
    try:
        loads, _, cap = _ladder(mj, pp, curve_id, table)
        rs = np.random.default_rng(1234)
        values = [int.from_bytes(rs.bytes(40), "little") % c.r for _ in loads]
        assert len(set(values)) == len(values) and min(values) >> 200
        sc = scalars_with_loads(N, loads, values, np.random.default_rng(8))
        want = _want(cref, curve_id, ("wide", table, cap), bases, sc)
        assert np.array_equal(_aff(cref, curve_id, mj.msm_bigint(pp, sc, scalars_are_mont=False)), want), (table, "single")
        jac = mj.msm_bigint_batch(pp, [sc, _dense(curve_id), sc], scalars_are_mont=False)
        for i, w in enumerate((want, _want(cref, curve_id, "dense", bases, _dense(curve_id)), want)):
            assert np.array_equal(_aff(cref, curve_id, jac[i]), w), (table, "batch", i)
    finally:
        L.mzk_msm_set_precompute(1)
        pp.release()


# ---- exceptional operands in the rare-path adders ----------------------------------------------------
@pytest.mark.parametrize("table", [1, 0])
@pytest.mark.parametrize("curve_id", [0, 1])
def test_rare_paths_with_equal_and_inverse_bases(gpu, mj, cref, curve_id, table):
    """Exceptional operands in the rare-path adders.  Every base is one point P (a): every chunk sum of an over-long bucket is the same
    point [cap]P, so msm_long_combine adds EQUAL points (a doubling inside EC::add), and so do all three levels of the heavy trees.  Bases
    P, -P by index parity (b): partial sums are small multiples of P of either sign and often infinity -- additions of a point and its
    inverse, of infinity on either side; a bucket sums to P or to infinity (occ must follow).  (c) as (b) with even loads: EVERY bucket,
    and the MSM, is infinity."""
    c = mj.params.CURVES[curve_id]
    P = np.array(_bases(curve_id)[5])
    negP = P.copy()
    y = sum(int(P[1][j]) << (64 * j) for j in range(c.fq_limbs))
    ny = c.q - y                                                       # (the negative of a Montgomery residue is the residue of the negative)
    negP[1] = [(ny >> (64 * j)) & 0xFFFFFFFFFFFFFFFF for j in range(c.fq_limbs)]
    all_p = np.repeat(P[None], N, axis=0)
    alt = all_p.copy()
    alt[1::2] = negP
    L = mj.load()
    L.mzk_msm_set_precompute(table)
    pps = []
    try:
        pp_p = mj.UnivariateProverParam.from_affine(curve_id, all_p)
        pps.append(pp_p)
        pp_alt = mj.UnivariateProverParam.from_affine(curve_id, alt)
        pps.append(pp_alt)
        c_bits, M, cap, desc_cap, h1_cap = _probe(mj, pp_p, _dense(curve_id))
        print("sizing: equal bases curve", curve_id, "table" if table else "plain", "single c", c_bits, "M", M, "cap", cap, "desc_cap", desc_cap, "h1_cap", h1_cap)
        loads = ladder_loads(cap)
        assert sum(loads) + len(loads) <= N
        values = ladder_values(c_bits, len(loads))
        assert max(values) < 1 << (c_bits - 1)
        # (a) all +P
        sc = scalars_with_loads(N, loads, values, np.random.default_rng(9))
        k_a = sum(d * l for d, l in zip(values, loads)) % c.r
        want_a = cref.g1_mul(curve_id, P, k_a)
        assert np.array_equal(_aff(cref, curve_id, cref.msm(curve_id, all_p, sc, scalars_are_mont=False, threads=8)), want_a)      # the two oracles agree
        assert np.array_equal(_aff(cref, curve_id, mj.msm_bigint(pp_p, sc, scalars_are_mont=False)), want_a), "all +P"
        assert mj.lib.msm_last_rare()[0] == cap
        jac = mj.msm_bigint_batch(pp_p, [sc, sc], scalars_are_mont=False)
        assert np.array_equal(_aff(cref, curve_id, jac[0]), want_a) and np.array_equal(_aff(cref, curve_id, jac[1]), want_a), "all +P, batch"
        # (b) P, -P by parity: bucket k nets (loads[k] mod 2) P
        sc = scalars_with_loads(N, loads, values, np.random.default_rng(10), by_parity=True)
        k_b = sum(d * (l & 1) for d, l in zip(values, loads)) % c.r
        assert k_b != 0
        want_b = cref.g1_mul(curve_id, P, k_b)
        assert np.array_equal(_aff(cref, curve_id, mj.msm_bigint(pp_alt, sc, scalars_are_mont=False)), want_b), "P, -P"
        jac = mj.msm_bigint_batch(pp_alt, [sc, sc], scalars_are_mont=False)
        assert np.array_equal(_aff(cref, curve_id, jac[0]), want_b) and np.array_equal(_aff(cref, curve_id, jac[1]), want_b), "P, -P, batch"
        # (c) every load even: infinity, Z = 0
        even = [l + (l & 1) for l in loads]
        sc = scalars_with_loads(N, even, values, np.random.default_rng(11), by_parity=True)
        out = mj.msm_bigint(pp_alt, sc, scalars_are_mont=False)
        assert not out[2].any(), "every bucket cancels: the MSM is infinity (Z = 0)"
        jac = mj.msm_bigint_batch(pp_alt, [sc, sc], scalars_are_mont=False)
        assert not jac[0][2].any() and not jac[1][2].any(), "infinity, batch"
    finally:
        L.mzk_msm_set_precompute(1)
        for p in pps:
            p.release()


# ---- overflow of the optimistically sized scratch ------------------------------------------
def _overflow_member(cap, desc_cap, c_bits, chunks):
    """Scalars whose lowest window holds K over-long buckets of `chunks` chunk descriptors each (load chunks * cap + 1: the last chunk
    has ONE entry; no bucket is heavy), with chunks * K past desc_cap by an eighth: the reservations of the last buckets lie beyond the
    array, and with desc_cap no multiple of `chunks` one bucket STRADDLES its end -- some of its slots inside, unwritten before the fix of
    msm_long_register (csrc/msm.cuh) and still walked by the consumers of that attempt."""
    load = chunks * cap + 1
    assert load <= cap + HEAVY_RUN, "over-long, not heavy"
    K = (desc_cap + desc_cap // 8 + 7 + chunks - 1) // chunks
    assert K * chunks > desc_cap and K < 1 << (c_bits - 1) and K * load <= N, (K, load, desc_cap)
    return scalars_with_loads(N, [load] * K, list(range(1, K + 1)), np.random.default_rng(100 + chunks)), K


def _chunks_that_straddle(desc_cap):
    """The smallest number of chunks per bucket (>= 2) that does not divide desc_cap: reservations are multiples of it, so the bucket
    that crosses the end of the array starts inside it.  Two chunks and an odd desc_cap: exactly one unwritten slot before the end."""
    for m in (2, 3, 5, 7):
        if desc_cap % m:
            return m
    raise AssertionError(("no straddling chunk count for", desc_cap))


@pytest.mark.parametrize("straddle", [False, True])
def test_chunk_descriptor_overflow_reruns_the_group(gpu, mj, cref, straddle):
    """More chunk descriptors than the optimistic array holds (batch of two: only a batch sizes optimistically): the host reads the
    counter with the results, enlarges the share and runs the group again (csrc/msm.hip MSM_RETRY).  The overflowed attempt may touch
    only what it wrote; its result is thrown away and the second one must be the oracle's.  The share goes 1/8 -> 1/4 -> 1/2
    -> 1, so a fourth attempt always fits."""
    curve_id = 0
    bases = _bases(curve_id)
    dense = _dense(curve_id)
    L = mj.load()
    mj.lib.check(L.mzk_workspace_release(), "mzk_workspace_release")            # the share starts at 1/8 again
    pp = mj.UnivariateProverParam.from_affine(curve_id, bases)
    L.mzk_msm_set_precompute(0)
    try:
        c_bits, M, cap, desc_cap, h1_cap = _probe(mj, pp, dense, batch=2)
        chunks = _chunks_that_straddle(desc_cap) if straddle else 1
        sc, K = _overflow_member(cap, desc_cap, c_bits, chunks)
        print("sizing: overflow batch2 plain c", c_bits, "M", M, "cap", cap, "desc_cap", desc_cap, "h1_cap", h1_cap, "chunks", chunks, "K", K,
              "entries", K * (chunks * cap + 1), "unwritten slots before the end", (desc_cap % chunks) if straddle else 0)
        want = [_want(cref, curve_id, ("overflow", chunks, cap, desc_cap), bases, sc), _want(cref, curve_id, "dense", bases, dense)]
        before = _ws_bytes(mj)
        jac = mj.msm_bigint_batch(pp, [sc, dense], scalars_are_mont=False)
        _, desc_cap_after, _, attempts = mj.lib.msm_last_rare()
        print("sizing: overflow attempts", attempts, "desc_cap after", desc_cap_after)
        for i in range(2):
            assert np.array_equal(_aff(cref, curve_id, jac[i]), want[i]), ("first call", i)
        assert attempts >= 2, "the construction must overflow the descriptors"
        assert attempts <= 4
        assert desc_cap_after >= K * chunks
        assert _ws_bytes(mj) > before, "the overflow must have enlarged the rare-path scratch"
        jac = mj.msm_bigint_batch(pp, [sc, dense], scalars_are_mont=False)
        assert mj.lib.msm_last_rare()[3] == 1, "the second call finds the scratch large enough"
        for i in range(2):
            assert np.array_equal(_aff(cref, curve_id, jac[i]), want[i]), ("second call", i)
    finally:
        L.mzk_msm_set_precompute(1)
        pp.release()
        mj.lib.check(L.mzk_workspace_release(), "mzk_workspace_release")        # later tests start from the default share


def test_descriptor_and_heavy_overflow_in_one_group(gpu, mj, cref):
    """Both optimistic arrays overflow in ONE attempt, in different members of a batch of three: chunk descriptors (member 0), level-1
    sums of heavy buckets (member 1: all-equal scalars, every entry of every window in one heavy bucket); member 2 is dense with another
    length of the same window class (per-MSM capacities under the group's maxima)."""
    curve_id = 0
    c = mj.params.CURVES[curve_id]
    n2 = (1 << 17) + 1
    bases = _bases(curve_id)
    dense = _dense(curve_id)
    L = mj.load()
    mj.lib.check(L.mzk_workspace_release(), "mzk_workspace_release")
    pp = mj.UnivariateProverParam.from_affine(curve_id, bases)
    L.mzk_msm_set_precompute(0)
    try:
        c_bits, M, cap, desc_cap, h1_cap = _probe(mj, pp, dense, batch=3)
        mj.msm_bigint_batch(pp, [dense, dense, dense[:n2]], scalars_are_mont=False)
        assert mj.lib.msm_last_shape()[0] == c_bits and mj.lib.msm_last_rare()[3] == 1, "both lengths must share a window size (one group)"
        sc, K = _overflow_member(cap, desc_cap, c_bits, 1)
        equal = np.repeat(np.array(dense[3:4]), N, axis=0)
        assert N // 16 > h1_cap, "all-equal scalars must overflow the level-1 sums"
        members = [sc, equal, np.array(dense[:n2])]
        want = [_want(cref, curve_id, ("overflow", 1, cap, desc_cap), bases, sc), _want(cref, curve_id, "equal", bases, equal),
                _want(cref, curve_id, "dense_n2", bases[:n2], members[2])]
        jac = mj.msm_bigint_batch(pp, members, scalars_are_mont=False)
        attempts = mj.lib.msm_last_rare()[3]
        print("sizing: both overflows batch3 plain c", c_bits, "M", M, "cap", cap, "desc_cap", desc_cap, "h1_cap", h1_cap, "K", K, "attempts", attempts)
        for i in range(3):
            assert np.array_equal(_aff(cref, curve_id, jac[i]), want[i]), i
        assert 2 <= attempts <= 4
    finally:
        L.mzk_msm_set_precompute(1)
        pp.release()
        mj.lib.check(L.mzk_workspace_release(), "mzk_workspace_release")


def test_stale_scratch_of_a_larger_problem_does_not_leak(gpu, mj, cref):
    """The descriptor and chunk-sum arrays are grow-only and never cleared.  The ladder batch right AFTER the descriptor overflow --
    the workspace not released: the arrays hold the descriptors of a larger, earlier problem -- gives the points it gives from a fresh
    workspace, the oracle's."""
    curve_id = 0
    bases = _bases(curve_id)
    dense = _dense(curve_id)
    L = mj.load()
    mj.lib.check(L.mzk_workspace_release(), "mzk_workspace_release")
    pp = mj.UnivariateProverParam.from_affine(curve_id, bases)
    L.mzk_msm_set_precompute(0)
    try:
        loads, values, cap = _ladder(mj, pp, curve_id, 0)
        ladder = scalars_with_loads(N, loads, values, np.random.default_rng(7))
        want = [_want(cref, curve_id, ("ladder", 0, cap), bases, ladder), _want(cref, curve_id, "dense", bases, dense)]
        mj.lib.check(L.mzk_workspace_release(), "mzk_workspace_release")
        c_bits, M, cap2, desc_cap, h1_cap = _probe(mj, pp, dense, batch=2)
        assert cap2 == cap
        sc, K = _overflow_member(cap, desc_cap, c_bits, 1)
        mj.msm_bigint_batch(pp, [sc, dense], scalars_are_mont=False)
        assert mj.lib.msm_last_rare()[3] >= 2, "the earlier problem must have been the larger one"
        stale = mj.msm_bigint_batch(pp, [ladder, dense, ladder], scalars_are_mont=False)      # (no release in between)
        assert mj.lib.msm_last_rare()[3] == 1
        mj.lib.check(L.mzk_workspace_release(), "mzk_workspace_release")
        fresh = mj.msm_bigint_batch(pp, [ladder, dense, ladder], scalars_are_mont=False)
        for i, w in enumerate((want[0], want[1], want[0])):
            assert np.array_equal(_aff(cref, curve_id, stale[i]), w), ("stale", i)
            assert np.array_equal(_aff(cref, curve_id, fresh[i]), w), ("fresh", i)
    finally:
        L.mzk_msm_set_precompute(1)
        pp.release()
        mj.lib.check(L.mzk_workspace_release(), "mzk_workspace_release")
