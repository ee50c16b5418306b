"""First timings of proof-link verification ("Proof links"; profiles/link_verify_time.txt).  For K = 1, 16, 256 links of
size 256 and 1024 on both curves, wall clock around the synchronous entry points from the Python client:
  (a) one batched verification: begin_links, link_weights, finish, check -- one pairing check for the K links;
  (b) the baseline: K single verifications through the same entry points, weight 1, one pairing check each.
Separately the two link kernels' own times from the library's profile regions (vfy_link_transcript, vfy_link_vanishing).
The links are valid and distinct, made through the trapdoor without a prover: a_2 = a_1 + s Z_D, so q = -s and the opened polynomial is
s(X) (Z_D(eta) - Z_D(X)); every commitment is a scalar multiple of g.  Needs a GPU:  python tools/link_verify_time.py"""
import ctypes as C
import os
import random
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle")]
import mpc_jellyfish_amd as mj  # noqa: E402
import pyref  # noqa: E402
import pyref_fs as FS  # noqa: E402

KS, SIZES, ALIGNMENT = (1, 16, 256), (256, 1024), 12


def make_links(c, pc, rng, beta, size, count):
    r, g = pc.r, pyref.g1_gen(pc)
    out = []
    for i in range(count):
        layout = mj.linking.GroupLayout(ALIGNMENT, rng.randrange(1 << ALIGNMENT), size)
        z = lambda x: mj.linking.compute_vanishing_poly_eval(c, x, layout)
        a1, s = rng.randrange(r), rng.randrange(1, r)               # a_1(beta), s(beta)
        pts = [pyref.g1_mul(pc, a1, g), pyref.g1_mul(pc, (a1 + s * z(beta)) % r, g), pyref.g1_mul(pc, -s % r, g)]
        t = FS.StandardTranscript(pc, b"PlonkLinkingProof")
        t.append_commitments(b"linking_wire_comms", pts[:2])
        t.append_commitment(b"quotient_comm", pts[2])
        eta = t.get_and_append_challenge(b"eta")
        pi = s * (z(eta) - z(beta)) % r * pow(beta - eta, -1, r) % r
        recs = [FS.g1_bytes(pc, p) for p in pts + [pyref.g1_mul(pc, pi, g)]]
        out.append((recs[0], recs[1], recs[2] + recs[3], layout))
    return out


def best(fn, reps=5):
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        r = fn()
        times.append((time.perf_counter() - t0) * 1e3)
    return min(times), r


def batched(key, links):
    b = key.begin_links(links)
    A, B = b.finish(b.link_weights())
    return key.check(A, B)


def singles(key, links, one):
    ok = True
    for link in links:
        b = key.begin_links([link])
        A, B = b.finish(one)
        ok = key.check(A, B) and ok
    return ok


def kernel_times(key, links):
    L = mj.load()
    L.mzk_profile_reset()
    L.mzk_profile_enable(1)
    for _ in range(5):
        key.begin_links(links).discard()
    L.mzk_profile_enable(0)
    lib = sys.modules["mpc-jellyfish_amd.lib"]
    out = []
    for name in ("vfy_link_transcript", "vfy_link_vanishing"):
        ms, count = lib.profile_get(name)
        out.append(ms / max(count, 1))
    L.mzk_profile_reset()
    return out


def main():
    lines = []
    for cid in (0, 1):
        c, pc = mj.params.CURVES[cid], pyref.CURVES[cid]
        rng = random.Random(8800 + cid)
        beta = rng.randrange(1, c.r)
        key = mj.keys.OpenKey(c, *mj.kzg.open_key_for_testing(c, beta))
        one = mj.params.fr_to_mont(c, [1])
        lines.append("%s" % ("BLS12-381" if cid == 0 else "BN254"))
        lines.append("  size     K    (a) batched   (b) K singles    transcript kernel   vanishing kernel")
        for size in SIZES:
            links = make_links(c, pc, rng, beta, size, max(KS))
            assert batched(key, links[:2]) and singles(key, links[:2], one)        # warm-up: kernels loaded, allocator primed; the links verify
            bad = list(links[:2])
            bad[1] = (bad[1][0], bad[1][1], bad[1][2], mj.linking.GroupLayout(ALIGNMENT, bad[1][3].offset + 1, size))
            assert not batched(key, bad)
            for K in KS:
                ta, ok_a = best(lambda: batched(key, links[:K]))
                tb, ok_b = best(lambda: singles(key, links[:K], one), reps=3)
                assert ok_a and ok_b
                kt, kv = kernel_times(key, links[:K])
                lines.append("  %4d  %4d   %9.2f ms   %10.2f ms   %14.3f ms   %14.3f ms" % (size, K, ta, tb, kt, kv))
        key.release()
    print("\n".join(lines))


if __name__ == "__main__":
    main()
