"""Timings of Advz.disperse and Advz.verify_shares (mpc-jellyfish_amd/vid.py; DESIGN.md section 4.17, profiles/vid_advz_time.txt) beside the
composition a caller had before, written out below from the public calls of the commit before this scheme existed: bytes -> elements on the
host, multi_open_rou_evals per polynomial, batch_commit, a hashlib tree over the downloaded evaluations, the field hasher on the host, the
aggregate polynomial on the host, multi_open_rou_proofs.  One card, both curves, (k, n) = (2^8, 2^10) and (2^10, 2^12), payloads of 1 MiB and
8 MiB (+ 1 byte, so that the payload has a length element).  Wall clock around the synchronous calls from the Python client, results on the host
as Python objects included on both sides; min .. max of REPS repeats after one untimed call, one process.  No gate: the host tree's share
depends on the box's CPU.  Where the fused path is not below the composition the line says so.
Needs a GPU:  python tools/vid_advz_time.py > profiles/vid_advz_time.txt"""
import hashlib
import os
import random
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [HERE]
SHAPES, SIZES, REPS = ((8, 10), (10, 12)), (1 << 20, 8 << 20), 3


def wall_ms(fn):
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e3, out


def span(ts):
    return "%9.1f .. %9.1f" % (min(ts), max(ts))


def composed_disperse(mj, vid, payload):
    """disperse from the parent's public calls; returns (commit, root, proofs) for the cross-check"""
    import numpy as np
    c, k, n, dom = vid.curve, vid.payload_chunk_size, vid.num_storage_nodes, vid.domain
    K = mj.UnivariateKzgPCS
    elems = []
    for at in range(0, len(payload), 31):                                  # bytes_to_field on the host
        elems.append(int.from_bytes(payload[at:at + 31], "little"))
    if len(payload) % 31:
        elems.append(len(payload) % 31)
    mont = mj.params.fr_to_mont(c, elems)
    polys = [mont[i:i + k] for i in range(0, len(elems), k)]
    evals = [K.multi_open_rou_evals(p, n, dom) for p in polys]             # one NTT and one download per polynomial
    commits = K.batch_commit(vid.ck, polys)
    level = [hashlib.sha256(i.to_bytes(8, "little") + len(polys).to_bytes(8, "little") + b"".join(e[i].to_bytes(32, "little") for e in evals)).digest()
             for i in range(n)]
    for _ in range(vid.height):
        level = [hashlib.sha256(b"".join((level[g:g + 3] + [bytes(32)] * 2)[:3])).digest() for g in range(0, len(level), 3)]
    records = b"".join(mj.kzg.g1_record(c, cm, compress=False) for cm in commits)
    commit = hashlib.sha256(records).digest()
    s = mj.params.fr_from_mont(c, vid.pseudorandom_scalar(mj.vid.Common(commits, level[0], len(elems)))[None])[0]
    agg = [0] * k
    for at in range(0, len(elems), k):
        for j, v in enumerate(elems[at:at + k]):
            agg[j] += v
    agg = mj.params.fr_to_mont(c, [a * s % c.r for a in agg])
    proofs = K.multi_open_rou_proofs(vid.ck, agg, n, dom)
    return commit, level[0], proofs


def main():
    import mpc_jellyfish_amd as mj
    print("Advz.disperse / verify_shares against the composition of the former public calls; ms, wall clock around the synchronous calls, "
          "min .. max of %d repeats" % REPS)
    for cid, name in ((0, "BLS12-381"), (1, "BN254")):
        c = mj.params.CURVES[cid]
        rng = random.Random(77 + cid)
        beta = rng.randrange(1, c.r)
        pp = mj.UnivariateProverParam.gen_srs_for_testing(c, beta, 2 << SHAPES[-1][0])
        key = mj.keys.OpenKey(c, *mj.kzg.open_key_for_testing(c, beta))
        for log_k, log_n in SHAPES:
            vid = mj.Advz(c, 1 << log_k, 1 << log_n, pp, key)
            for size in SIZES:
                payload = random.Random(size + log_k).randbytes(size + 1)
                got = vid.disperse(payload)                                    # untimed: the FK23 table of this (offset, d), the workspace
                want = composed_disperse(mj, vid, payload)
                same = (got.commit, got.common.all_evals_digest, [s.aggregate_proof for s in got.shares]) == want
                fused = [wall_ms(lambda: vid.disperse(payload))[0] for _ in range(REPS)]
                comp = [wall_ms(lambda: composed_disperse(mj, vid, payload))[0] for _ in range(REPS)]
                got.common._aggregate = None
                ver = []
                for _ in range(REPS):
                    got.common._aggregate = None                               # (the aggregate commitment is part of a first verification)
                    ms, ok = wall_ms(lambda: vid.verify_shares(got.shares, got.common))
                    ver.append(ms)
                note = "fused below composed" if max(fused) < min(comp) else "fused NOT below composed"
                print("  %-9s k = 2^%d, n = 2^%d, %d MiB (K = %4d)   disperse %s   composed %s   composed / fused = %5.1f   %s   verify_shares (all n) %s   %s%s" %
                      (name, log_k, log_n, size >> 20, len(got.common.poly_commits), span(fused), span(comp), min(comp) / min(fused), note, span(ver),
                       "every share accepted" if all(ok) else "SHARES REFUSED", "" if same else "   RESULTS DIFFER FROM THE COMPOSITION"))
                sys.stdout.flush()
        key.release()
        pp.release()


if __name__ == "__main__":
    main()
