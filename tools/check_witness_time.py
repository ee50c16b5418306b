"""Wall time of mzk_prover_check_witness beside the same run's `prove` on the same circuit and witness (both end in a device
synchronise: the check reads its report back, the proof its last commitments).
    python tools/check_witness_time.py [--log-n 20] [--reps 10]
Two legs, the ones DESIGN.md 4.9 quotes: the 2^log_n-gate TurboPlonk bench circuit on BLS12-381 with a DENSE witness (dense_seed: every
wire polynomial has n random coefficients), and the UltraPlonk bench circuit on BN254 (its own witness: the dense variant exists for
TurboPlonk only).  Per leg one JSON line: median and minimum of `reps` checks on device-resident wire values and on the host witness
vector (gathered on the device), median and minimum of `reps` proofs, and their ratio.  Device wires are timed twice: before the
wire-variable table is set (gate and lookup families only) and after (`check_device_wires_copy`: the copy constraints as well).
--only turbo | ultra: one leg (for a profiler run).  The check is warmed up once before its window
(the first call sizes the shared scratch) and the prover twice."""
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
    import torch
    import mpc_jellyfish_amd as mj
    n = 1 << args.log_n

    def window(fn):
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
        rng = mj.rng.test_rng()
        ck = mj.UnivariateProverParam.gen_srs_for_testing(c, mj.rng.fr_rand(c, rng), cs.n + 2)
        pk = mj.snark.preprocess(ck, cs)
        host_vec = mj.snark.HostWitness(cs.witness.cpu().pin_memory(), cs.wire_variables)
        for _ in range(2):
            mj.snark.prove(rng, cs, pk)
        rep = pk.check_witness(cs.wire_values, [])
        assert rep.satisfied and not rep.copy_checked, rep
        no_table = window(lambda: pk.check_witness(cs.wire_values, []))
        assert pk.check_witness(host_vec, []).satisfied                      # (sets the wire-variable table)
        rep = pk.check_witness(cs.wire_values, [])
        assert rep.satisfied and rep.copy_checked, rep
        out = {"curve": c.name, "plonk_type": plonk_type, "log_n": cs.n.bit_length() - 1, "dense_witness": dense,
               "check_device_wires": no_table,
               "check_device_wires_copy": window(lambda: pk.check_witness(cs.wire_values, [])),
               "check_host_vector": window(lambda: pk.check_witness(host_vec, [])),
               "prove": window(lambda: mj.snark.prove(rng, cs, pk))}
        out["check_over_prove"] = round(out["check_device_wires_copy"]["median_ms"] / out["prove"]["median_ms"], 4)
        print(json.dumps(out), flush=True)
        pk.release()
        ck.release()


if __name__ == "__main__":
    main()
