"""First timings of the KZG openings (DESIGN.md sections 4.14 "KZG openings" and 4.15; profiles/kzg_openings.txt).  Wall clock around the
synchronous calls from the Python client, polynomials resident on the device, on both curves:
  open     UnivariateKzgPCS.batch_open at K = 1 and K = 16, 2^16 coefficients each.  With --parent-root DIR (a built checkout of the parent
           commit) the same calls run on that tree too, in processes of their own that ALTERNATE with this tree's, --reps times: the
           parent's run-to-run spread is the range of its medians over those processes.
  verify   UnivariateKzgPCS.batch_verify at K = 2^12 (one pairing check) against 2^12 calls of verify (one each).  Openings are made
           through the trapdoor without a prover; every point is a known multiple of g.
Needs a GPU:  python tools/kzg_openings_time.py [--parent-root DIR] [--reps 3] > profiles/kzg_openings.txt"""
import argparse
import json
import os
import random
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LOG_LEN, KS, CALLS = 16, (1, 16), 20
VERIFY_K = 1 << 12


def wall_ms(fn):
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e3, out


def worker_open(root):
    sys.path[:0] = [root]
    import numpy as np
    import torch
    import mpc_jellyfish_amd as mj
    out = {}
    for cid in (0, 1):
        c = mj.params.CURVES[cid]
        rng = random.Random(31 + cid)
        pp = mj.UnivariateProverParam.gen_srs_for_testing(c, rng.randrange(1, c.r), (1 << LOG_LEN) - 1)
        polys = [torch.from_numpy(mj.params.random_fr_mont(c, 1 << LOG_LEN, 100 + i).view(np.int64)).cuda() for i in range(max(KS))]
        points = [rng.randrange(c.r) for _ in polys]
        for K in KS:
            run = lambda: mj.UnivariateKzgPCS.batch_open(pp, polys[:K], points[:K])
            for _ in range(3):
                first = run()
            times = [wall_ms(run)[0] for _ in range(CALLS)]
            digest = [int(p.xy[0, 0]) for p in first[0]] + [e % (1 << 64) for e in first[1]]
            out["%d/%d" % (cid, K)] = dict(median=statistics.median(times), best=min(times), worst=max(times), digest=digest)
        pp.release()
    print("RESULT " + json.dumps(out))


def make_openings(mj, pyref, FS, cid, count):
    c, pc = mj.params.CURVES[cid], pyref.CURVES[cid]
    rng = random.Random(47 + cid)
    r, g = pc.r, pyref.g1_gen(pc)
    beta = rng.randrange(1, r)
    cm = rng.randrange(1, r)
    cm_rec = FS.g1_bytes(pc, pyref.g1_mul(pc, cm, g))
    w, d = rng.randrange(1, r), rng.randrange(1, r)
    W, D = pyref.g1_mul(pc, w, g), pyref.g1_mul(pc, d, g)
    cms, zs, vs, pfs = [], [], [], []
    for _ in range(count):                                             # one commitment "opened" at count points: v = c - (beta - z) w
        z = rng.randrange(r)
        cms.append(cm_rec), zs.append(z), vs.append((cm - (beta - z) * w) % r), pfs.append(FS.g1_bytes(pc, W))
        w, W = (w + d) % r, pyref.g1_add(pc, W, D)
    return c, beta, (cms, zs, vs, pfs)


def worker_verify(root):
    sys.path[:0] = [root, os.path.join(root, "oracle")]
    import mpc_jellyfish_amd as mj
    import pyref
    import pyref_fs as FS
    out = {}
    for cid in (0, 1):
        c, beta, args = make_openings(mj, pyref, FS, cid, VERIFY_K)
        key = mj.keys.OpenKey(c, *mj.kzg.open_key_for_testing(c, beta))
        batched = lambda: mj.UnivariateKzgPCS.batch_verify(key, *args, mj.rng.ChaChaRng(bytes(32), 20))
        singles = lambda: all(mj.UnivariateKzgPCS.verify(key, *one) for one in zip(*args))
        assert batched() and mj.UnivariateKzgPCS.verify(key, args[0][0], args[1][0], args[2][0], args[3][0])       # warm-up; they verify
        wrong = (args[0], args[1], [(args[2][0] + 1) % c.r] + args[2][1:], args[3])
        assert not mj.UnivariateKzgPCS.batch_verify(key, *wrong, mj.rng.ChaChaRng(bytes(32), 20))
        tb = [wall_ms(batched)[0] for _ in range(3)]
        ts, ok = wall_ms(singles)
        assert ok
        out[str(cid)] = dict(batched=min(tb), batched_all=tb, singles=ts)
        key.release()
    print("RESULT " + json.dumps(out))


def spawn(kind, root):
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", kind, "--root", root], capture_output=True, text=True, timeout=600)
    if p.returncode != 0:
        sys.exit("worker %s on %s failed (%d):\n%s" % (kind, root, p.returncode, p.stderr[-2000:]))
    return json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--worker", choices=("open", "verify"))
    ap.add_argument("--root", default=HERE)
    ap.add_argument("--parent-root")
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    if a.worker:
        return worker_open(a.root) if a.worker == "open" else worker_verify(a.root)
    names = ("BLS12-381", "BN254")
    runs = {"parent": [], "this": []}
    for _ in range(a.reps):                                            # alternating, a process each
        if a.parent_root:
            runs["parent"].append(spawn("open", a.parent_root))
        runs["this"].append(spawn("open", HERE))
    print("batch_open, 2^%d coefficients a polynomial, device-resident; ms, median of %d calls per process, %d processes a tree, alternating" % (LOG_LEN, CALLS, a.reps))
    for cid in (0, 1):
        for K in KS:
            k = "%d/%d" % (cid, K)
            line = "  %-9s K = %2d" % (names[cid], K)
            for tree in ("parent", "this"):
                if not runs[tree]:
                    line += "   %s: not measured" % tree
                    continue
                med = [r[k]["median"] for r in runs[tree]]
                line += "   %s: %s  (median %.3f, spread %.3f, best call %.3f)" % (tree, " ".join("%.3f" % m for m in med), statistics.median(med), max(med) - min(med),
                                                                                    min(r[k]["best"] for r in runs[tree]))
            if runs["parent"]:
                assert all(r[k]["digest"] == runs["this"][0][k]["digest"] for tree in runs for r in runs[tree]), "the two trees disagree on " + k
                line += "   same proofs and evaluations"
            print(line)
    v = spawn("verify", HERE)
    print("batch_verify at K = 2^12 against 2^12 calls of verify; ms (batched: best of 3; the singles once)")
    for cid in (0, 1):
        print("  %-9s batched %.1f   (all: %s)   singles %.0f" % (names[cid], v[str(cid)]["batched"], " ".join("%.1f" % t for t in v[str(cid)]["batched_all"]), v[str(cid)]["singles"]))


if __name__ == "__main__":
    main()
