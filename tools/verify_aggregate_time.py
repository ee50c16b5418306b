"""First timings of aggregated-proof verification (profiles/verify_aggregate_time.txt): wall clock around the
synchronous entry points from the Python client, as profiles/verify_time.txt measures the single-proof path.  BatchProofs of m = 1, 4, 16
instances, K = 1 and 1024 of them under one tuple; beside m = 1 the single-proof path (keys.Verifier.begin on `Proof` images) at the same K.
General circuits (oracle/pyref_circuit.py: every selector live, four public inputs), two distinct proofs repeated, compressed mode, subgroup
checks on.  Needs a GPU:  python tools/verify_aggregate_time.py"""
import os
import random
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle")]
import mpc_jellyfish_amd as mj  # noqa: E402
import pyref  # noqa: E402
from pyref_circuit import general_circuit, general_ultra_circuit  # noqa: E402

MS, KS, M_MAX = (1, 4, 16), (1, 1024), 16


def mont(c, ints):
    return mj.params.fr_to_mont(c, [int(x) % c.r for x in ints])


def best(fn, reps):
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        r = fn()
        out.append((time.perf_counter() - t0) * 1e3)
    return min(out), r


def world(cid, ultra, log_n):
    c, pc = mj.params.CURVES[cid], pyref.CURVES[cid]
    n, W = 1 << log_n, 6 if ultra else 5
    beta = 0xBE7A + cid
    g, h, beta_h = mj.kzg.open_key_for_testing(c, beta)
    ck = mj.UnivariateProverParam.gen_srs_for_testing(c, beta, n + 2)
    dom = mj.Radix2EvaluationDomain(c, log_n)
    provers, wires, pubs, vks = [], [], [], []
    for j in range(M_MAX):
        rng = random.Random(9000 + 31 * j + cid)
        if ultra:
            sel, sig, k, wv, pi, tabs = general_ultra_circuit(pc, log_n, rng, gates="all")
            kw = {"plookup": {name: dom.ifft(mont(c, tabs[key])) for name, key in zip(mj.plonk.PLOOKUP_TABLE_POLYS, ("range", "key", "table_dom_sep", "q_dom_sep"))}}
        else:
            sel, sig, k, wv, pi = general_circuit(pc, log_n, rng, gates="all")
            kw = {}
        p = mj.prover.TurboPlonkProver(c, n, [dom.ifft(mont(c, s)) for s in sel], [dom.ifft(mont(c, s)) for s in sig], k, ck, **kw)
        provers.append(p)
        wires.append(np.stack([mont(c, col) for col in wv]))
        pubs.append(list(pi[:4]))
        vks.append(mj.keys.VerifyingKey.deserialize(cid, p.serialize_vk(4, h, beta_h)))
    brng = mj.rng.test_rng()
    rows = {}
    for m in MS:
        proofs = []
        for extra in (None, b"extra message"):
            blinds, quot = mj.snark.draw_batch_blinders(c, brng, W, [ultra] * m)
            proofs.append((mj.batch.serialize_batch_proof(c, mj.batch.batch_prove(provers[:m], wires[:m], pubs[:m], blinds, quot, extra)), extra))
        agg = mj.keys.AggregateVerifier(vks[:m])
        for K in KS:
            images, extras = [proofs[i % 2][0] for i in range(K)], [proofs[i % 2][1] for i in range(K)]
            rows[m, K] = measure(c, lambda: agg.begin(images, [pubs[:m]] * K, extras), agg,
                                 lambda: mj.snark.batch_verify_batch_proofs(vks[:m], [pubs[:m]] * K, images, extras))
    singles = []
    for extra in (None, b"extra message"):
        blind = mj.snark.draw_blinders(c, brng, W, ultra)
        singles.append((mj.snark.serialize_proof(c, provers[0].prove(wires[0], pubs[0], mj.prover.TranscriptChallenges(provers[0], pubs[0], extra), blind)), extra))
    v = vks[0].verifier()
    for K in KS:
        images, extras = [singles[i % 2][0] for i in range(K)], [singles[i % 2][1] for i in range(K)]
        rows["single", K] = measure(c, lambda: v.begin(images, [pubs[0]] * K, extras), v, lambda: mj.snark.batch_verify([vks[0]] * K, [pubs[0]] * K, images, extras))
    return rows


def measure(c, begin, checker, end_to_end):
    begin().discard()                                                # warm-up: kernels loaded, allocator primed
    t_begin, b = best(lambda: begin(), 5)
    K = b.K
    b.discard()
    weights = mont(c, [random.Random(1).randrange(c.r) for _ in range(K)])
    fin = []
    for _ in range(3):
        b = begin()
        t0 = time.perf_counter()
        A, B = b.finish(weights)
        fin.append((time.perf_counter() - t0) * 1e3)
    t_check, _ = best(lambda: checker.check(A, B), 3)
    t_all, ok = best(end_to_end, 3)
    assert ok
    return t_begin, min(fin), t_check, t_all


if __name__ == "__main__":
    from importlib import import_module
    import_module("mpc-jellyfish_amd.lib").init(0)
    for title, args in (("TurboPlonk / BLS12-381, n = 2^4", (0, False, 4)), ("UltraPlonk / BN254, n = 2^5", (1, True, 5))):
        rows = world(*args)
        print(title)
        print("  %-22s %10s %10s %10s %12s" % ("", "begin", "finish", "check", "end to end"))
        for key in [("single", K) for K in KS] + [(m, K) for m in MS for K in KS]:
            name = ("single-proof path" if key[0] == "single" else "aggregate m = %d" % key[0]) + ", K = %d" % key[1]
            print("  %-28s %7.2f ms %7.2f ms %7.2f ms %9.2f ms" % ((name,) + rows[key]))
