"""tests/plookup_cases.py -- TEST INFRASTRUCTURE ONLY: a catalogue of seeded Plookup instances for the hash joins, the counting
kernel, the three-kernel scan and the gather of csrc/plookup.cuh, and for the 5-tuple hash join of csrc/check.cuh.

WHITE BOX.  This module restates, in Python, the two hash functions of the device code -- `fr_words_hash` (csrc/plookup.cuh) and
`lookup_key_hash` (csrc/check.cuh) -- and the slot count of their open-addressing tables (`sorted_vec_run`, `witness_check_run` in
csrc/plonk.hip), in order to AIM values at one probe chain (`same_hash_cluster`).  A change to either hash must be restated here, or
tests/test_plookup_cases.py fails at "restated hash"; nothing else depends on the restatement.  The block sizes the scenarios are laid
out against (PLK_THREADS, PLK_SCAN_T, PLK_SCAN_E) are read from the sources.

    case(c, log_n, scenario, variant, mode) -> a Case in the arrays of oracle/pyref_circuit.py (canonical integers):
        tables     {"range", "key", "table_dom_sep", "q_dom_sep"} -> n values
        q_lookup   n values (0 / 1)
        w          six wire columns of n values
        refused    the instance holds a looked-up value outside the table (rows < n - 1): the builders must refuse it
        w_valid    refused instances: the same wires with the absent lookups replaced by present ones (same key)
        tau, beta, gamma    the challenges the tests use with this instance

    mode "direct": q_lookup = 0 everywhere -- the merged table is the range column, the merged lookup witness is wire 5, and the
        scenario dictates the 256-bit values the hash join sees; the other table columns and wires 0-4 hold noise that q_lookup = 0
        must mask.
    mode "tuple": every value of the scenario is a 5-tuple (first, dom_sep, a0, a1, a2): (range, table_dom_sep, key, w3, w4) on the
        table side and (w5, q_dom_sep, w0, w1, w2) on the lookup side, q_lookup = 1 -- merged with tau by plookup_merge_kernel, keyed as
        they stand by check.cuh.  Some values are "plain" (first, 0, 0, 0, 0); a row whose table and lookup values are both plain has
        q_lookup = 0 and noise in the masked columns, so that both settings of the selector occur in one instance.
"""
import os
import random
import re
import types
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mpc-jellyfish_amd", "csrc")
M32 = 0xFFFFFFFF
R = 1 << 256
WAVE = 64
TABLES = ("range", "key", "table_dom_sep", "q_dom_sep")


def _source_constant(file, name):
    with open(os.path.join(CSRC, file)) as f:
        m = re.search(r"constexpr\s+int\s+%s\s*=\s*(\d+)\s*;" % name, f.read())
    assert m, "%s: no integer constant %s" % (file, name)
    return int(m.group(1))


PLK_THREADS = _source_constant("plonk.cuh", "PLK_THREADS")
PLK_SCAN_BLOCK = _source_constant("plookup.cuh", "PLK_SCAN_T") * _source_constant("plookup.cuh", "PLK_SCAN_E")


# ---- the restatement of the device hashes ----------------------------------------------------------------------------------------
def words_of(x):
    """the eight 32-bit words of a 256-bit integer, least significant first (the uint4 pair the kernels load)"""
    return [(x >> (32 * i)) & M32 for i in range(8)]


def int_of(words):
    return sum(w << (32 * i) for i, w in enumerate(words))


WORD_MULTIPLIERS = (0x9E3779B1, 0x85EBCA77, 0xC2B2AE3D, 0x27D4EB2F, 0x165667B1, 0x9E3779B1)      # words 0..4, then y ^ z ^ w of the top three
WORD_SHIFTS = (15, 13, 16, 15, 13, 16)                                                            # after each of them
KEY_MULTIPLIER, KEY_SHIFTS = 0x9E3779B1, (15, 16)


def fr_words_hash(w):
    """csrc/plookup.cuh fr_words_hash on the eight words of the Montgomery image"""
    h = 0
    for k, x in enumerate(list(w[:5]) + [w[5] ^ w[6] ^ w[7]]):
        h = (h + x * WORD_MULTIPLIERS[k]) & M32
        h ^= h >> WORD_SHIFTS[k]
    return h


def fold_key_hash(component_hashes):
    """csrc/check.cuh lookup_key_hash, given fr_words_hash of each of the five components"""
    h = 0
    for e in component_hashes:
        h = ((h ^ (h >> KEY_SHIFTS[0])) * KEY_MULTIPLIER + e) & M32
    return h ^ (h >> KEY_SHIFTS[1])


def lookup_key_hash(key_words):
    return fold_key_hash([fr_words_hash(w) for w in key_words])


def slot_count(n):
    """slots of both open-addressing tables (csrc/plonk.hip): the power of two >= 4n, at least 4"""
    s = 4
    while s < 4 * n:
        s <<= 1
    return s


def mont_words(c, v):
    return words_of(v % c.r * R % c.r)


def from_mont_words(c, words):
    """the canonical integer whose Montgomery image has these words: limbs * R^-1 mod r"""
    x = int_of(words)
    assert x < c.r, "the chosen limbs must stay below r"
    return x * pow(R, -1, c.r) % c.r


def value_hash(c, v):
    return fr_words_hash(mont_words(c, v))


def tuple_hash(c, t):
    return lookup_key_hash([mont_words(c, x) for x in t])


# ---- the catalogue ---------------------------------------------------------------------------------------------------------------
CATALOGUE = (
    ("distinct_uniform", None),
    ("hot_first", None), ("hot_last", None), ("hot_boundary", "last_of_block"), ("hot_boundary", "first_of_next"),
    ("interleaved_duplicates", "m2"), ("interleaved_duplicates", "m7"), ("interleaved_duplicates", "m64"), ("interleaved_duplicates", "late_m7"),
    ("runs", None),
    ("one_word_apart", None),
    ("same_hash_cluster", None),
    ("almost_uniform_waves", None),
    ("missing", "row_0"), ("missing", "row_n_minus_2"), ("missing", "one_third"), ("missing", "one_word"), ("missing", "last_row_only"),
    ("missing", "wave_boundary"),
)
REDUCED = tuple(e for e in CATALOGUE if e[0] in ("distinct_uniform", "hot_boundary", "interleaved_duplicates", "runs"))
MODES = ("direct", "tuple")
TOP_WORD_LIMIT = 0x10000000           # chosen top words stay below this; one flipped bit below 2^28 keeps them below 2^29 < r >> 224


def boundary(n):
    """the block boundary a scenario of n rows is laid out against: the scan block, else the workgroup, else the middle"""
    if n > PLK_SCAN_BLOCK:
        return PLK_SCAN_BLOCK
    if n > PLK_THREADS:
        return PLK_THREADS
    return max(n // 2, 1)


class _Build:
    """values are handled as ids until the end: `direct` / `tuples` hold the ids a scenario pins to chosen values"""

    def __init__(self, c, n, rng, mode):
        self.c, self.n, self.rng, self.mode = c, n, rng, mode
        self.next_id = 0
        self.direct = {}
        self.tuples = {}
        self.meta = {}

    def fresh(self, k):
        out = list(range(self.next_id, self.next_id + k))
        self.next_id += k
        return out

    def fresh1(self):
        return self.fresh(1)[0]

    def small_top_words(self):
        """eight random Montgomery words with distinct top three words below TOP_WORD_LIMIT (so: below r, whatever is flipped below)"""
        rng = self.rng
        top = rng.sample(range(1, TOP_WORD_LIMIT), 3)
        return [rng.getrandbits(32) for _ in range(5)] + top

    def flip(self, words, k):
        """one bit of word k changed (below bit 28 in the top word)"""
        out = list(words)
        out[k] ^= 1 << self.rng.randrange(28)
        return out

    def hash_class(self, count, accept):
        """`count` distinct canonical values with one fr_words_hash h, accept(h) true: equal low words, equal y ^ z ^ w on top"""
        rng = self.rng
        while True:
            low = [rng.getrandbits(32) for _ in range(5)]
            x = rng.getrandbits(32)
            if accept(fr_words_hash(low + [x, 0, 0])):
                break
        seen, out = set(), []
        while len(out) < count:
            y, w = rng.getrandbits(32), rng.randrange(2 * TOP_WORD_LIMIT)
            if (y, w) in seen:
                continue
            seen.add((y, w))
            out.append(from_mont_words(self.c, low + [y, x ^ y ^ w, w]))
        return out


def _uniform_lookups(b, T):
    pool = sorted(set(T))
    return [b.rng.choice(pool) for _ in range(b.n)]


def _distinct_uniform(b, variant):
    T = b.fresh(b.n)
    return T, _uniform_lookups(b, T)


def _hot(b, variant):
    n = b.n
    T = b.fresh(n)
    at = {"first": 0, "last": n - 1, "last_of_block": boundary(n) - 1, "first_of_next": min(boundary(n), n - 1)}[variant]
    b.meta["hot_index"] = at
    return T, [T[at]] * n


def _interleaved(b, variant):
    n, rng = b.n, b.rng
    late = variant.startswith("late_")
    m = int(variant.split("m")[-1])
    p = rng.randrange(n // 8, n // 2) if late and n >= 16 else 0
    v = b.fresh(m)
    T = b.fresh(p) + [v[i % m] for i in range(n - p)]
    b.meta.update(m=m, prefix=p)
    return T, [rng.choice(v[:n]) if rng.random() < 0.5 else rng.choice(T[:p] or v[:n]) for _ in range(n)]       # half of them hit the repeating values


RUN_LENGTHS = (65, 63, 64, 255, 256, 257)


def _runs(b, variant):
    n, rng = b.n, b.rng
    T, runs = [], []
    reserve = 4 if n >= 16 else 0

    def place(length, straddle=None, vid=None):
        start = len(T)
        if straddle:
            k = max(1, -(-(start + length // 2) // straddle))
            start = k * straddle - length // 2
        if start + length > n - reserve:
            return None
        T.extend(b.fresh(start - len(T)))
        vid = b.fresh1() if vid is None else vid
        T.extend([vid] * length)
        runs.append((start, length, vid))
        return vid

    first = place(2)                                        # a run that starts at index 0
    if n >= 4:
        T.append(b.fresh1())
        place(1, vid=first)                                 # run, other value, the same value again
    placed = {}
    for length in RUN_LENGTHS:
        placed[length] = place(length, straddle=PLK_THREADS if length in (63, 255) else None)
    if n >= 4 * PLK_SCAN_BLOCK:
        placed["short_across_scan_block"] = place(3, straddle=PLK_SCAN_BLOCK)
    placed["long"] = place(PLK_SCAN_BLOCK + 1)              # longer than a scan block: covers a boundary wherever it starts
    tail = [v for v in (placed[64], placed["long"], placed[65], first) if v is not None][:reserve]
    T.extend(b.fresh(n - len(tail) - len(T)))
    T.extend(tail)                                          # values of earlier runs, recurring far from them
    assert len(T) == n
    b.meta["runs"] = runs
    hot = sorted({v for _, length, v in runs if length > 1} | set(tail))
    return T, [rng.choice(hot) if rng.random() < 0.7 else rng.choice(T) for _ in range(n)]


def _scatter(b, members, lookups_of_members):
    """members at random table rows among fresh values; every member looked up at least once, `lookups_of_members` of the n rows in all"""
    n, rng = b.n, b.rng
    assert len(members) <= n // 2
    T = members + b.fresh(n - len(members))
    rng.shuffle(T)
    L = list(members)
    L += [rng.choice(members) for _ in range(max(0, lookups_of_members - len(L)))]
    L += [rng.choice(T) for _ in range(n - len(L))]
    head = L[:n - 1]
    rng.shuffle(head)
    return T, head + L[n - 1:]


def _one_word_apart(b, variant):
    """direct: clusters {base, base with one word changed -- each of the eight words in turn} and clusters of six values whose top
    three words are the permutations of one triple.  tuple: {base tuple, the tuple with one word of one component changed -- each
    component and each word in turn}: 41 table tuples any two of which agree in at least three components."""
    c = b.c
    clusters, members = [], []
    if b.mode == "direct":
        for _ in range(3):
            base = b.small_top_words()
            ids = b.fresh(9)
            for i, k in zip(ids, [None] + list(range(8))):
                b.direct[i] = from_mont_words(c, base if k is None else b.flip(base, k))
            clusters.append(("one_word", ids))
        for _ in range(2):
            base = b.small_top_words()
            ids = b.fresh(6)
            y, z, w = base[5:]
            for i, top in zip(ids, [(y, z, w), (y, w, z), (z, y, w), (z, w, y), (w, y, z), (w, z, y)]):
                b.direct[i] = from_mont_words(c, base[:5] + list(top))
            clusters.append(("permuted_top", ids))
    else:
        base = [b.small_top_words() for _ in range(5)]
        ids = b.fresh(41)
        b.tuples[ids[0]] = tuple(from_mont_words(c, x) for x in base)
        for q, i in enumerate(ids[1:]):
            e, k = divmod(q, 8)
            b.tuples[i] = tuple(from_mont_words(c, b.flip(x, k) if j == e else x) for j, x in enumerate(base))
        clusters.append(("one_word_tuple", ids))
    for _, ids in clusters:
        members += ids
    b.meta["clusters"] = clusters
    return _scatter(b, members, len(members) * 2)


def _same_hash_cluster(b, variant):
    """64 values (tuple mode: 64 tuples) with one hash, and 16 more whose common hash lands within 8 slots of the end of the slot
    array: nine of them already carry the probe chain over the wrap"""
    n, rng = b.n, b.rng
    mask = slot_count(n) - 1
    near_end = lambda h: h & mask >= mask - 7
    clusters = []
    if b.mode == "direct":
        for count, accept in ((64, lambda h: True), (16, near_end)):
            ids = b.fresh(count)
            for i, v in zip(ids, b.hash_class(count, accept)):
                b.direct[i] = v
            clusters.append(ids)
    else:
        for count, accept in ((64, lambda h: True), (16, lambda h: near_end(fold_key_hash([h] * 5)))):
            pool = b.hash_class(16, accept)
            ids = b.fresh(count)
            seen = set()
            for i in ids:
                while True:
                    t = tuple(rng.choice(pool) for _ in range(5))
                    if t not in seen:
                        break
                seen.add(t)
                b.tuples[i] = t
            clusters.append(ids)
    b.meta["clusters"] = clusters
    return _scatter(b, clusters[0] + clusters[1], n // 2)


def _almost_uniform_waves(b, variant):
    n, rng = b.n, b.rng
    T = b.fresh(n)
    L, odd = [], []
    for g in range(-(-n // WAVE)):
        a, o = rng.sample(T, 2)
        at = (0, 31, 63)[g % 3]
        L += [o if lane == at else a for lane in range(min(WAVE, n - g * WAVE))]
        odd.append(g * WAVE + at)
    b.meta["odd_rows"] = odd
    return T, L


def _missing(b, variant):
    n, rng, c = b.n, b.rng, b.c
    T = b.fresh(n)
    L = _uniform_lookups(b, T)
    if variant == "row_0":
        rows = [0]
    elif variant == "row_n_minus_2":
        rows = [n - 2]
    elif variant == "last_row_only":
        rows = [n - 1]
    elif variant == "wave_boundary":
        rows = [WAVE - 1, WAVE] if n >= 2 * WAVE else [n // 2 - 1, n // 2]
    elif variant == "one_third":
        rows = sorted(rng.sample(range(n - 1), n // 3))
    else:
        assert variant == "one_word"
        rows = sorted(rng.sample(range(n - 1), 1 if b.mode == "direct" else 5))
    absent = b.fresh(max(1, len(rows) // 2))                # one_third: every absent value on about two rows
    for q, row in enumerate(rows):
        L[row] = absent[q % len(absent)]
    if variant == "one_word":
        near = T[rng.randrange(n)]                          # the present value the absent ones are one word away from
        if b.mode == "direct":
            words = b.small_top_words()
            b.direct[near] = from_mont_words(c, words)
            b.direct[absent[0]] = from_mont_words(c, b.flip(words, rng.randrange(8)))
        else:
            absent = b.fresh(5)
            words = [b.small_top_words() for _ in range(5)]
            b.tuples[near] = tuple(from_mont_words(c, x) for x in words)
            for e, (row, i) in enumerate(zip(rows, absent)):    # component e of the lookup on rows[e] differs in one word
                k = rng.randrange(8)
                b.tuples[i] = tuple(from_mont_words(c, b.flip(x, k) if j == e else x) for j, x in enumerate(words))
                L[row] = i
            # q_dom_sep is a column of the key: the valid witness of the same key needs a table entry under the changed separator too
            other = next(v for v in T if v != near)
            b.tuples[other] = (rng.randrange(c.r), b.tuples[absent[1]][1]) + tuple(rng.randrange(c.r) for _ in range(3))
        b.meta["near"] = near
    b.meta["absent_rows"] = [row for row in rows if row < n - 1]
    return T, L


SCENARIOS = {
    "distinct_uniform": _distinct_uniform,
    "hot_first": lambda b, v: _hot(b, "first"), "hot_last": lambda b, v: _hot(b, "last"), "hot_boundary": _hot,
    "interleaved_duplicates": _interleaved,
    "runs": _runs,
    "one_word_apart": _one_word_apart,
    "same_hash_cluster": _same_hash_cluster,
    "almost_uniform_waves": _almost_uniform_waves,
    "missing": _missing,
}


def case(c, log_n, scenario, variant=None, mode="direct"):
    """The instance of (scenario, variant) on 2^log_n rows over the scalar field of c (anything with `.r`), in `mode`.  Deterministic."""
    assert mode in MODES and (scenario, variant) in CATALOGUE
    n, r = 1 << log_n, c.r
    rng = random.Random(zlib.crc32(repr((scenario, variant, mode, log_n, r)).encode()))
    b = _Build(c, n, rng, mode)
    T, L = SCENARIOS[scenario](b, variant)
    assert len(T) == n and len(L) == n
    present = set(T)
    absent_rows = [i for i in range(n - 1) if L[i] not in present]
    noise = lambda: [rng.randrange(r) for _ in range(n)]
    ids = sorted(present | set(L))
    if mode == "direct":
        used = set(b.direct.values())
        assert len(used) == len(b.direct)
        val = dict(b.direct)
        for i in ids:
            while i not in val:
                v = rng.randrange(r)
                if v not in used:
                    used.add(v)
                    val[i] = v
        L_valid = [v if v in present else T[i] for i, v in enumerate(L)]
        tables = {"range": [val[i] for i in T], "key": noise(), "table_dom_sep": noise(), "q_dom_sep": noise()}
        q = [0] * n
        low = [noise() for _ in range(5)]
        w, w_valid = low + [[val[i] for i in L]], low + [[val[i] for i in L_valid]]
    else:
        used = set(b.tuples.values())
        assert len(used) == len(b.tuples)
        tup = dict(b.tuples)
        for i in ids:                                       # domain separators as circuits have them: a few small constants
            while i not in tup:
                t = (rng.randrange(r), 0, 0, 0, 0) if rng.random() < 0.3 else (rng.randrange(r), rng.randrange(1, 4)) + tuple(rng.randrange(r) for _ in range(3))
                if t not in used:
                    used.add(t)
                    tup[i] = t
        # q_dom_sep is a column of the key, not of the witness: the valid witness looks up, on the rows of the absent values, present
        # values under the same domain separator
        by_sep = {}
        for i in sorted(present):
            by_sep.setdefault(tup[i][1], []).append(i)
        L_valid = [v if v in present or j == n - 1 else rng.choice(by_sep[tup[v][1]]) for j, v in enumerate(L)]
        plain = lambda i: not any(tup[i][1:])
        q = [0 if plain(T[j]) and plain(L[j]) and plain(L_valid[j]) else 1 for j in range(n)]
        pick = lambda src, e: [tup[src[j]][e] if q[j] or e == 0 else rng.randrange(r) for j in range(n)]
        tables = {"range": pick(T, 0), "table_dom_sep": pick(T, 1), "key": pick(T, 2), "q_dom_sep": pick(L, 1)}
        w3, w4 = pick(T, 3), pick(T, 4)
        w = [pick(L, 2), pick(L, 3), pick(L, 4), w3, w4, pick(L, 0)]
        w_valid = [pick(L_valid, 2), pick(L_valid, 3), pick(L_valid, 4), w3, w4, pick(L_valid, 0)]
    refused = bool(absent_rows)
    out = types.SimpleNamespace(curve=c, log_n=log_n, n=n, scenario=scenario, variant=variant, mode=mode, tables=tables, q_lookup=q, w=w,
                                w_valid=w_valid if refused else None, refused=refused, absent_rows=absent_rows, table_ids=T, lookup_ids=L,
                                meta=b.meta, values=val if mode == "direct" else None, tuples=tup if mode == "tuple" else None,
                                tau=rng.randrange(1, r), beta=rng.randrange(1, r), gamma=rng.randrange(1, r))
    out.sel = [None] * 13 + [q]                             # as check_witness_ref.lookup_failures reads the selectors
    return out


def label(scenario, variant):
    return scenario if variant is None else "%s-%s" % (scenario, variant)
