"""Wall time of mzk_prover_derive_wire_variables -- the wire-variable table recovered from a proving key's sigma polynomials -- and of
its three steps on their own (every one ends in a device synchronise).
    python tools/derive_variables_time.py [--log-n 20] [--reps 10]
Two legs, the ones DESIGN.md 4.12 quotes: the 2^log_n-gate TurboPlonk bench circuit on BLS12-381 in its DENSE variant (dense_seed: five
variables per addition, every variable on one to three cells), and the UltraPlonk bench circuit on BN254, where `zero` and `one` own most
of the 6 x 2^log_n cells (cycles of millions of cells).  The provers come from coefficient forms (no table).  Per leg one JSON line: median
and minimum of `reps` calls of derive, and of its steps as the stateless primitives run them -- the W forward NTTs (mzk_ntt_dev over W
rows), mzk_plonk_sigma_decode_dev, mzk_plonk_variables_from_permutation_dev -- with the number of variables, the longest cycle and the
number of doubling rounds that length takes.  The derived table is compared with the circuit's own, renumbered by first occurrence.
--only turbo | ultra: one leg (for a profiler run).  Every step is warmed up once before its window (the first call sizes the shared scratch)."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-n", type=int, default=20)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--only", choices=("turbo", "ultra"))
    args = ap.parse_args()
    import numpy as np
    import torch
    import mpc_jellyfish_amd as mj
    n = 1 << args.log_n

    def window(fn):
        fn()
        times = []
        for _ in range(args.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            times.append((time.perf_counter() - t0) * 1e3)
        times.sort()
        return {"median_ms": round(times[len(times) // 2], 3), "min_ms": round(times[0], 3)}

    for curve_id, plonk_type, dense in ((0, "TurboPlonk", True), (1, "UltraPlonk", False)):
        if args.only and not plonk_type.lower().startswith(args.only):
            continue
        c = mj.params.CURVES[curve_id]
        cs = mj.snark.gen_circuit_for_bench(c, n, plonk_type, **({"dense_seed": 77} if dense else {}))
        W, log_n = cs.num_wire_types, cs.n.bit_length() - 1
        rng = mj.rng.test_rng()
        ck = mj.UnivariateProverParam.gen_srs_for_testing(c, mj.rng.fr_rand(c, rng), cs.n + 2)
        pk = mj.snark.preprocess(ck, cs, lagrange=False)
        out = {"curve": c.name, "plonk_type": plonk_type, "log_n": log_n, "cells": W * cs.n, "derive": window(pk.derive_wire_variables)}
        # the table against the circuit's own, renumbered by first occurrence
        flat = cs.wire_variables.cpu().numpy().reshape(-1)
        uniq, first, counts = np.unique(flat, return_index=True, return_counts=True)
        rank = np.empty(uniq.shape[0], dtype=np.uint32)
        rank[np.argsort(first)] = np.arange(uniq.shape[0], dtype=np.uint32)
        table, n_vars = pk.wire_variables()
        assert n_vars == uniq.shape[0] and np.array_equal(table.reshape(-1), rank[np.searchsorted(uniq, flat)]), "derived table differs from the circuit's"
        longest = int(counts.max())
        out.update(n_vars=n_vars, longest_cycle=longest, doubling_rounds=min(max(1, (longest - 1).bit_length() + (longest > 1)), (W * cs.n - 1).bit_length()))
        # the steps on their own: W forward NTTs (timed on values: the transform does the same work on any input), decode, label
        dom = mj.Radix2EvaluationDomain(c, log_n)
        scratch = cs.sigma_values.clone()
        out["ntt"] = window(lambda: dom.fft_in_place(scratch))
        del scratch
        out["decode"] = window(lambda: mj.plonk.sigma_decode(c, cs.sigma_values, cs.k))
        nxt = mj.plonk.sigma_decode(c, cs.sigma_values, cs.k)
        out["label"] = window(lambda: mj.plonk.variables_from_permutation(nxt))
        print(json.dumps(out), flush=True)
        pk.release()
        ck.release()


if __name__ == "__main__":
    main()
