"""The scenario catalogue of tests/plookup_cases.py, held to what its scenarios are named for -- on the CPU, against the big-int
restatement (oracle/pyref_plonk.py) and the integer definition of the witness check's lookup family (tests/check_witness_ref.py) --
at every size the GPU sweep (tests/test_plookup_sweep_gpu.py) uses.  A generator that degrades into "random values" fails here."""
import os
import re
from collections import Counter

import pytest

import check_witness_ref as REF
import plookup_cases as PC

SWEEP_LOG_N = (9, 13)                # the whole catalogue, both modes: two workgroups in one scan block; two scan blocks
EDGE_LOG_N = (1, 2, 12, 14)          # the reduced catalogue: one lookup; n = 4; exactly one scan block; four scan blocks
CHECK_LOG_N = (8, 13)                # the witness check's lookup family: tuple mode

CASES = [(log_n, s, v, mode) for log_n in SWEEP_LOG_N for s, v in PC.CATALOGUE for mode in PC.MODES]
CASES += [(log_n, s, v, mode) for log_n in EDGE_LOG_N for s, v in PC.REDUCED for mode in PC.MODES]
CASES += [(log_n, s, v, "tuple") for log_n in CHECK_LOG_N if log_n not in SWEEP_LOG_N for s, v in PC.CATALOGUE]
CASES += [(6, "interleaved_duplicates", "m7", mode) for mode in PC.MODES]         # the small problem of the stale-workspace test
IDS = ["2^%d-%s-%s" % (log_n, PC.label(s, v), mode) for log_n, s, v, mode in CASES]


def _rle(values):
    out = []
    for i, v in enumerate(values):
        if out and out[-1][2] == v:
            out[-1][1] += 1
        else:
            out.append([i, 1, v])
    return out


def _one_word_difference(a, b):
    """the index of the only 32-bit word in which the Montgomery images a and b differ, or None"""
    d = [k for k in range(8) if a[k] != b[k]]
    return d[0] if len(d) == 1 else None


def test_restated_hash_follows_the_sources():
    """the multipliers and shifts of the two device hashes, read from the sources, are the ones the restatement uses"""
    def body(file, name):
        with open(os.path.join(PC.CSRC, file)) as f:
            text = f.read()
        at = text.index("uint32_t %s(" % name)
        return text[at:text.index("\n}", at)]
    nums = lambda text, pat: tuple(int(x, 0) for x in re.findall(pat, text))
    words = body("plookup.cuh", "fr_words_hash")
    assert nums(words, r"(0x[0-9A-Fa-f]+)u") == PC.WORD_MULTIPLIERS and nums(words, r">> (\d+)") == PC.WORD_SHIFTS
    assert re.findall(r"a[01]\.[xyzw]", words) == ["a0.x", "a0.y", "a0.z", "a0.w", "a1.x", "a1.y", "a1.z", "a1.w"]
    key = body("check.cuh", "lookup_key_hash")
    assert nums(key, r"(0x[0-9A-Fa-f]+)u") == (PC.KEY_MULTIPLIER,) and nums(key, r">> (\d+)") == PC.KEY_SHIFTS
    for file, name in (("plookup.cuh", "fr_words_hash"), ("check.cuh", "lookup_key_hash")):
        with open(os.path.join(PC.CSRC, file)) as f:
            text = f.read()
        assert "tests/plookup_cases.py" in text[:text.index("uint32_t %s(" % name)].rsplit("\n", 2)[-2], "the pointer to the restatement at " + name
    # a value, its Montgomery words and back
    import pyref
    for pc in (pyref.CURVES[0], pyref.CURVES[1]):
        v = 0x1234567 % pc.r
        assert PC.from_mont_words(pc, PC.mont_words(pc, v)) == v
    assert [PC.slot_count(n) for n in (1, 2, 4, 512, 8192)] == [4, 8, 16, 2048, 32768]


@pytest.mark.parametrize("curve_id", [0, 1])
@pytest.mark.parametrize("log_n,scenario,variant,mode", CASES, ids=IDS)
def test_scenario_is_what_it_is_named_for(pyref, curve_id, log_n, scenario, variant, mode):
    import pyref_plonk as PP
    pc = pyref.CURVES[curve_id]
    k = PC.case(pc, log_n, scenario, variant, mode)
    n, r, SB, WG = k.n, pc.r, PC.PLK_SCAN_BLOCK, PC.PLK_THREADS
    # ---- the forms of oracle/pyref_circuit.py, canonical, and the mode
    cols = [k.tables[name] for name in PC.TABLES] + [k.q_lookup] + k.w
    assert len(k.w) == 6 and all(len(col) == n and all(0 <= x < r for x in col) for col in cols)
    assert set(k.q_lookup) <= {0, 1} and (mode == "tuple" or not any(k.q_lookup))
    table = PP.merged_table_values(pc, k.tau, k.tables, k.q_lookup, k.w)
    lookup = PP.merged_lookup_values(pc, k.tau, k.tables, k.q_lookup, k.w)
    if mode == "direct":
        assert table == k.tables["range"] and lookup == k.w[5]
    # ---- accepted / refused, by both references
    looked = lookup[:n - 1]
    sorted_vec = PP.sorted_lookup_vec(table, looked)
    failing = REF.lookup_failures(pc, k.sel, k.w, k.tables)
    assert k.refused == (scenario == "missing" and variant != "last_row_only")
    assert (len(sorted_vec) == 2 * n - 1) == (not k.refused)
    in_table = set(table)
    assert failing == k.absent_rows == [i for i in range(n - 1) if looked[i] not in in_table] and bool(failing) == k.refused
    if k.refused:
        valid = PP.merged_lookup_values(pc, k.tau, k.tables, k.q_lookup, k.w_valid)
        sorted_vec = PP.sorted_lookup_vec(table, valid[:n - 1])
        assert len(sorted_vec) == 2 * n - 1 and REF.lookup_failures(pc, k.sel, k.w_valid, k.tables) == []
    # ---- no zero denominator in the Plookup product (of the valid witness, for a refused instance)
    g1 = k.gamma * (1 + k.beta) % r
    for j in range(n - 2):
        assert (g1 + sorted_vec[j] + k.beta * sorted_vec[j + 1]) % r and (g1 + sorted_vec[n - 1 + j] + k.beta * sorted_vec[n + j]) % r
    # ---- the property of the name
    hits = Counter(looked)
    first_at = {}
    for i, v in enumerate(table):
        first_at.setdefault(v, i)
    runs = _rle(table)
    if mode == "tuple" and n >= 64 and scenario in ("distinct_uniform", "missing"):
        assert 0 < k.q_lookup.count(0) < n                                        # both settings of the selector in one instance
    if scenario == "distinct_uniform":
        assert len(first_at) == n and (n < 64 or len(hits) > n // 2)              # many counters, most of them small and non-zero
    elif scenario.startswith("hot"):
        want = {"hot_first": 0, "hot_last": n - 1}.get(scenario)
        if want is None:
            b = SB if n > SB else WG if n > WG else max(n // 2, 1)
            want = b - 1 if variant == "last_of_block" else min(b, n - 1)
        assert len(first_at) == n and set(looked) == {table[want]} and k.meta["hot_index"] == want
    elif scenario == "interleaved_duplicates":
        m, p = int(variant.split("m")[-1]), k.meta["prefix"]
        assert (p >= n // 8 and n >= 16) == variant.startswith("late_") or n < 16
        pattern = table[p:p + m]
        assert len(set(table[:p + m])) == min(p + m, n) and all(table[i] == pattern[(i - p) % m] for i in range(p, n))
        assert all(length == 1 for _, length, _ in runs)                          # never adjacent
        copies = Counter(table)
        if m < n - p:
            assert all(p <= first_at[v] < p + m and copies[v] >= (n - p) // m for v in pattern)
            assert n < 64 or sum(hits[v] for v in pattern) > n // 4         # the copies that must all land at their first entry
    elif scenario == "runs":
        lengths = {length for _, length, _ in runs}
        want = {2} | ({1} if n >= 4 else set())
        want |= {x for x, need in ((65, 128), (63, 512), (64, 512), (255, 1024), (256, 1024), (257, 2048)) if n >= need}
        assert want <= lengths and runs[0][0] == 0 and runs[0][1] == 2
        straddles = lambda B: [(s, length) for s, length, _ in runs if length > 1 and s // B != (s + length - 1) // B]
        assert n < 512 or straddles(WG)
        if n > SB:
            assert max(lengths) > SB and straddles(SB)
        if n >= 4 * SB:
            assert any(length <= 257 for _, length in straddles(SB))
        recurring = [v for v, c in Counter(v for _, _, v in runs).items() if c > 1]
        assert n < 4 or recurring
        if n >= 64:
            assert any(hits[v] for v in recurring) and any(hits[v] for _, length, v in runs if length > 1)
    elif scenario == "one_word_apart":
        img = (lambda i: PC.mont_words(pc, k.values[i])) if mode == "direct" else (lambda i: [PC.mont_words(pc, x) for x in k.tuples[i]])
        members = [i for _, ids in k.meta["clusters"] for i in ids]
        where = {v: j for j, v in enumerate(k.table_ids)}
        assert all(i in where and hits[table[where[i]]] for i in members)       # every member is in the table and looked up
        for kind, ids in k.meta["clusters"]:
            base = img(ids[0])
            if kind == "one_word":
                assert [_one_word_difference(base, img(i)) for i in ids[1:]] == list(range(8))
            elif kind == "permuted_top":
                tops = [tuple(img(i)[5:]) for i in ids]
                assert len(set(tops)) == 6 and all(sorted(t) == sorted(base[5:]) for t in tops) and all(img(i)[:5] == base[:5] for i in ids)
                assert len({PC.fr_words_hash(img(i)) for i in ids}) == 1
            else:
                diffs = [[(e, _one_word_difference(base[e], x)) for e, x in enumerate(img(i)) if x != base[e]] for i in ids[1:]]
                assert diffs == [[(e, w)] for e in range(5) for w in range(8)]
    elif scenario == "same_hash_cluster":
        h = (lambda i: PC.value_hash(pc, k.values[i])) if mode == "direct" else (lambda i: PC.tuple_hash(pc, k.tuples[i]))
        one, two = k.meta["clusters"]
        where = {v: j for j, v in enumerate(k.table_ids)}
        assert len(one) >= 64 and len({h(i) for i in one}) == 1 and len({table[where[i]] for i in one}) == len(one)
        slots = PC.slot_count(n)
        assert len(two) >= 9 and len({h(i) for i in two}) == 1 and slots - 8 <= (h(two[0]) & (slots - 1)) < slots      # the chain wraps
        assert h(one[0]) != h(two[0]) and len({table[where[i]] for i in two}) == len(two)
        members = {table[where[i]] for i in one + two}
        assert all(hits[v] for v in members) and sum(hits[v] for v in members) >= n // 2 - 1
        if mode == "tuple":         # what check.cuh hashes on a q_lookup = 1 row is the tuple as it stands in the columns
            j = where[one[0]]
            assert k.q_lookup[j] == 1 and (k.tables["range"][j], k.tables["table_dom_sep"][j], k.tables["key"][j], k.w[3][j], k.w[4][j]) == k.tuples[one[0]]
    elif scenario == "almost_uniform_waves":
        assert len(first_at) == n
        for g in range(n // PC.WAVE):
            rows = range(g * PC.WAVE, min((g + 1) * PC.WAVE, n))
            split = Counter(lookup[i] for i in rows).most_common()
            assert [c for _, c in split] == [63, 1] and lookup[g * PC.WAVE + (0, 31, 63)[g % 3]] == split[1][0]
    else:
        assert scenario == "missing"
        want = {"row_0": [0], "row_n_minus_2": [n - 2], "last_row_only": [], "wave_boundary": [PC.WAVE - 1, PC.WAVE]}.get(variant)
        if want is not None:
            assert failing == want
        if variant == "last_row_only":
            assert lookup[n - 1] not in first_at
        if variant == "one_third":
            assert abs(len(failing) - n // 3) <= 1 and len({looked[i] for i in failing}) < len(failing)
        if variant == "one_word":
            near = k.table_ids.index(k.meta["near"])
            if mode == "direct":
                assert len(failing) == 1
                assert _one_word_difference(PC.mont_words(pc, table[near]), PC.mont_words(pc, looked[failing[0]])) is not None
            else:
                have = (k.tables["range"][near], k.tables["table_dom_sep"][near], k.tables["key"][near], k.w[3][near], k.w[4][near])
                assert k.q_lookup[near] == 1 and len(failing) == 5
                for e, i in enumerate(failing):                                   # component e in turn: four equal, one word of the fifth changed
                    got = (k.w[5][i], k.tables["q_dom_sep"][i], k.w[0][i], k.w[1][i], k.w[2][i])
                    assert k.q_lookup[i] == 1 and [j for j in range(5) if got[j] != have[j]] == [e]
                    assert _one_word_difference(PC.mont_words(pc, got[e]), PC.mont_words(pc, have[e])) is not None
