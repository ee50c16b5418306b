"""Timings of UnivariateKzgPCS.multi_open_rou (FK23 on the device; DESIGN.md section 4.16, profiles/kzg_multi_open_time.txt) beside
UnivariateKzgPCS.batch_open at the same points -- the loop a caller had before, one MSM per point, which this work leaves unchanged.  Both
curves, len = 2^10 + 1, 2^14 + 1 and 2^16 + 1 coefficients resident on the device, every point of the domain of N = 2d points.  Wall clock from
the Python client around the synchronous calls, results to the host included; REPS repeats each, with their minimum and maximum:
  cold   the call that builds the transformed SRS vector (step A): the handle's table is evicted first by a call at another d
  warm   the calls after it
  loop   batch_open at the N points.  Above LOOP_DIRECT points only the first LOOP_SAMPLE are timed and the figure is scaled by
         N / LOOP_SAMPLE: it is then printed as EXTRAPOLATED (the loop's cost is linear in the points: one witness and one MSM each).
The last line states the criterion of the work: at len = 2^14 + 1 the warm range lies below the loop's range.
Needs a GPU:  python tools/kzg_multi_open_time.py > profiles/kzg_multi_open_time.txt"""
import os
import random
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [HERE]
LOGS, REPS = (10, 14, 16), 3
LOOP_DIRECT, LOOP_SAMPLE = 4096, 1024


def wall_ms(fn):
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e3, out


def span(ts):
    return "%10.2f .. %10.2f" % (min(ts), max(ts))


def main():
    import numpy as np
    import torch
    import mpc_jellyfish_amd as mj
    K = mj.UnivariateKzgPCS
    verdict = []
    print("multi_open_rou (FK23) against batch_open at the same points; ms, wall clock around the synchronous call, min .. max of %d repeats" % REPS)
    for cid, name in ((0, "BLS12-381"), (1, "BN254")):
        c = mj.params.CURVES[cid]
        rng = random.Random(53 + cid)
        pp = mj.UnivariateProverParam.gen_srs_for_testing(c, rng.randrange(1, c.r), 1 << LOGS[-1])
        tiny = mj.params.random_fr_mont(c, 3, 7)
        tiny_dom = mj.Radix2EvaluationDomain(c, 2)
        for log_d in LOGS:
            d, n = 1 << log_d, 2 << log_d
            poly = torch.from_numpy(mj.params.random_fr_mont(c, d + 1, 200 + log_d).view(np.int64)).cuda()
            dom = mj.Radix2EvaluationDomain(c, log_d + 1)                  # (multi_open_rou_eval_domain picks 4d for a power-of-two degree)
            run = lambda: K.multi_open_rou(pp, poly, n, dom)
            cold, warm = [], []
            for _ in range(REPS):
                K.multi_open_rou(pp, tiny, 4, tiny_dom)                    # another d: the table of this one goes
                cold.append(wall_ms(run)[0])
            for _ in range(REPS):
                ms, got = wall_ms(run)
                warm.append(ms)
            k = n if n <= LOOP_DIRECT else LOOP_SAMPLE
            points = roots(c, dom.log_size_of_group, k)
            loop_run = lambda: K.batch_open(pp, [poly] * k, points)
            loop_run()                                                     # (the first call may build the fixed-base table)
            loop = []
            for _ in range(REPS):
                ms, ref = wall_ms(loop_run)
                loop.append(ms * n / k)
            assert (got[0][:k], got[1][:k]) == ref, "multi_open_rou and batch_open disagree"
            label = "measured at all %d points" % n if k == n else "EXTRAPOLATED: %d of %d points timed, x %d" % (k, n, n // k)
            print("  %-9s len = 2^%d + 1, N = 2^%d   cold %s   warm %s   batch_open %s (%s)   loop / warm = %.1f" %
                  (name, log_d, log_d + 1, span(cold), span(warm), span(loop), label, min(loop) / max(warm)))
            if log_d == 14:
                verdict.append("%s %s" % (name, "met" if max(warm) < min(loop) else "NOT met"))
        pp.release()
    print("criterion (len = 2^14 + 1: warm below batch_open, ranges apart): " + ", ".join(verdict))


def roots(c, log_n, k):
    """w^0 .. w^(k-1) of the domain of 2^log_n points, as ark-poly picks w"""
    w = pow(c.fr_generator, (c.r - 1) >> log_n, c.r)
    return [pow(w, i, c.r) for i in range(k)]


if __name__ == "__main__":
    main()
