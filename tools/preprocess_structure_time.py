"""Preprocess from circuit structure: what profiles/preprocess_structure.txt records.
    python tools/preprocess_structure_time.py [--out FILE]
Three parts, all in one process so that the paths alternate on the same card: (i) mzk_plonk_wire_permutation_dev and
mzk_plonk_sigma_values_dev alone at 5 x 2^20 and 6 x 2^22 cells (device events, 3 warm-up calls, 20 timed); (ii) snark.preprocess of the
2^20-gate TurboPlonk bench circuit up to a ready prover, default against from_structure=True (wall, device synchronised); (iii) the
compiled host, `mzk_prove 0 turbo 1048584 0` with and without --device-preprocess (circuit build + preprocess seconds from its JSON)."""
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import time

import argparse

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "out", "preprocess_structure.txt"))
args = ap.parse_args()
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
import numpy as np
import torch
import mpc_jellyfish_amd as mj
from importlib import import_module

lib = import_module("mpc-jellyfish_amd.lib")
L = lib.init(0)
out = open(args.out, "w")


def say(*a):
    line = " ".join(str(x) for x in a)
    print(line, flush=True)
    out.write(line + "\n")
    out.flush()


def bench_table(W, n):
    """variable table of the bench circuit (snark.gen_circuit_for_bench) filling the domain: n - 2 additions"""
    n_add = n - 2
    var = torch.zeros((W, n), dtype=torch.int64, device="cuda")
    rows = torch.arange(2, 2 + n_add, device="cuda")
    var[4, 1] = 1
    var[0, 2:2 + n_add] = torch.where(rows == 2, torch.zeros_like(rows), rows - 1)
    var[1, 2:2 + n_add] = 1
    var[4, 2:2 + n_add] = rows
    return var.to(torch.int32).contiguous(), 2 + n_add


def device_ms(fn, warm=3, reps=20):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return statistics.median(ts), min(ts), max(ts)


say("# kernels alone (device events on the null stream around the library call; 3 warm-up calls, 20 timed; median / min / max ms)")
for curve_id, W, log_n, what in ((0, 5, 20, "bench table"), (1, 6, 22, "bench table"), (0, 5, 20, "all distinct"), (0, 5, 20, "random over n variables")):
    c = mj.params.CURVES[curve_id]
    n = 1 << log_n
    if what == "bench table":
        var, n_vars = bench_table(W, n)
    elif what == "all distinct":
        var, n_vars = torch.randperm(W * n, device="cuda").to(torch.int32).reshape(W, n).contiguous(), W * n
    else:
        var, n_vars = torch.randint(0, n, (W, n), device="cuda", dtype=torch.int32), n
    nxt = torch.empty(W * n, dtype=torch.int32, device="cuda")
    sig = torch.empty((W, n, 4), dtype=torch.int64, device="cuda")
    k = mj.params.fr_to_mont(c, mj.rng.compute_coset_representatives(c, W, n))
    perm = lambda: lib.check(L.mzk_plonk_wire_permutation_dev(C.c_void_p(var.data_ptr()), W * n, n_vars, C.c_void_p(nxt.data_ptr()), None), "perm")
    sigma = lambda: lib.check(L.mzk_plonk_sigma_values_dev(curve_id, log_n, W, C.c_void_p(nxt.data_ptr()), C.c_void_p(k.ctypes.data), C.c_void_p(sig.data_ptr()), None), "sigma")
    say("cells = %d x 2^%d, n_vars = %d (%s), curve %d:" % (W, log_n, n_vars, what, curve_id),
        "wire permutation %.3f / %.3f / %.3f ms;" % device_ms(perm), "sigma values %.3f / %.3f / %.3f ms" % device_ms(sigma))
    del var, nxt, sig
torch.cuda.empty_cache()

say("# Python host, 2^20-gate TurboPlonk bench circuit, BLS12-381: snark.preprocess up to a ready prover (wall ms, device synchronised; alternating, 1 warm-up each)")
c = mj.params.CURVES[0]
cs = mj.snark.gen_circuit_for_bench(c, (1 << 20) + 8, "TurboPlonk")
assert cs.n == 1 << 20
ck = mj.UnivariateProverParam.gen_srs_for_testing(c, 0x1234567, cs.n + 2)
times = {False: [], True: []}
vk = {}
for rep in range(4):
    for fs in (False, True):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        pk = mj.snark.preprocess(ck, cs, lagrange=False, from_structure=fs)
        L.mzk_dev_sync()
        dt = (time.perf_counter() - t0) * 1e3
        if rep:
            times[fs].append(dt)
        else:
            vk[fs] = [x.xy.tobytes() for part in pk.vk_commitments() for x in part]
        pk.release()
assert vk[False] == vk[True], "verifying keys differ"
for fs in (False, True):
    say("from_structure=%s:" % fs, " ".join("%.1f" % t for t in times[fs]), "median %.1f ms" % statistics.median(times[fs]))
say("verifying-key commitments of the two paths are equal")
ck.release()
del cs
torch.cuda.empty_cache()

say("# C++ host: mzk_prove 0 turbo 1048584 0 --no-lagrange, circuit_build_s (holds the CPU permutation) + preprocess_s (SRS, upload, key); alternating, 3 runs each")
binp = os.path.join(ROOT, "mpc-jellyfish_amd", "mzk_prove")
res = {"cpu": [], "device": []}
proofs = set()
for rep in range(3):
    for name, extra in (("cpu", []), ("device", ["--device-preprocess"])):
        r = subprocess.run([binp, "0", "turbo", str((1 << 20) + 8), "0", "--no-lagrange"] + extra, capture_output=True, text=True, timeout=300)
        if r.returncode != 0:
            say("mzk_prove failed:", r.stderr[-500:])
            sys.exit(1)
        j = json.loads(r.stdout.strip().splitlines()[-1])
        res[name].append((j["circuit_build_s"], j["preprocess_s"]))
        proofs.add(j["proof_hex"])
for name in res:
    say(name, "preprocess:", "; ".join("build %.3f s + preprocess %.3f s = %.3f s" % (a, b, a + b) for a, b in res[name]),
        "| median of sums %.3f s" % statistics.median(a + b for a, b in res[name]))
say("proof bytes equal across all six runs:", len(proofs) == 1)
out.close()
