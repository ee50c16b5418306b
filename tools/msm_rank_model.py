#!/usr/bin/env python3
"""tools/msm_rank_model.py [--log-n 20] [--seed 1] -- a schedule MODEL of the plain path's accumulation launch (csrc/msm.cuh,
msm_accumulate_split_kernel) under the two bucket rankings: per window (rounds 1-5) and over all windows (round 6).  numpy only, a few
seconds on the CPU.  It is a model, not a measurement: read it for the direction and against profiles/r06_global_rank_ab.txt.

Assumptions:
  * 2^log_n uniform scalars on BLS12-381, window 16: 16 windows of 2^15 buckets with Poisson loads (mean 32 at 2^20 pairs); the top
    window's digit has 15 bits and takes 29 678 values (r >> 240), so its occupied buckets carry 35.3 and the others nothing;
  * 1024 workgroup slots of 2 waves (MSM_ACC_THREADS = 128), a workgroup goes to the slot that frees first, in rank order;
  * a wave lasts as long as its longest lane, a workgroup as long as its longer wave;
  * a wave's speed does not depend on its neighbour (profiles/r04_fy_madd_bench.txt: 4.19 ns per multiply-add alone, 2 x 2.21 at two);
  * the tail (ranks >= rank0) is split S ways: thread s of a bucket takes entries s, s + S, ...; the combine costs (S - 1) full additions
    per tail bucket at the ideal rate, a full XYZZ addition counted as 1.4 mixed ones (14 field products against 10).
Output: makespan / ideal, where ideal = all mixed additions spread evenly over 1024 x 128 lanes."""
import argparse
import heapq

import numpy as np

SLOTS, WG, WAVE = 1024, 128, 64
ADD_VS_MADD = 1.4
TOP_VALUES = 29678                                    # values of the top 15-bit digit of a scalar < r (BLS12-381: r >> 240, + 1)


def loads(log_n, rng):
    n, m, n_win = 1 << log_n, 1 << 15, 16
    out = rng.poisson(n / m, size=(n_win, m)).astype(np.int64)
    top = np.zeros(m, dtype=np.int64)
    top[:TOP_VALUES] = rng.poisson(n / TOP_VALUES, size=TOP_VALUES)
    out[n_win - 1] = top
    return out


def makespan(lane_work):
    """lane_work: per-thread additions in dispatch order -> time at which the last workgroup ends"""
    pad = (-len(lane_work)) % WG
    w = np.concatenate([lane_work, np.zeros(pad, dtype=np.int64)]).reshape(-1, WG)
    wg_time = w.reshape(len(w), WG // WAVE, WAVE).max(axis=2).max(axis=1)
    free = [0] * SLOTS
    heapq.heapify(free)
    end = 0
    for t in wg_time:
        s = heapq.heappop(free) + int(t)
        end = max(end, s)
        heapq.heappush(free, s)
    return end


def schedule(cnt, global_rank, frac_log, log_split):
    """cnt[w][b] -> (makespan / ideal of the accumulation, combine / ideal)"""
    if global_rank:
        ranked = -np.sort(-cnt.reshape(-1), kind="stable")
    else:
        ranked = -np.sort(-cnt, axis=1, kind="stable")
        ranked = ranked.reshape(-1)
    total = int(ranked.sum())
    ideal = total / (SLOTS * WG)
    wm = len(ranked)
    if frac_log is None:
        return makespan(ranked) / ideal, 0.0
    rank0 = (wm - (wm >> frac_log)) & ~(WG - 1)
    S = 1 << log_split
    tail = ranked[rank0:]
    parts = np.stack([(tail - s + S - 1) // S for s in range(S)], axis=1).clip(min=0).reshape(-1)       # entries s, s + S, ...
    work = np.concatenate([ranked[:rank0], parts])
    combine = ADD_VS_MADD * (S - 1) * len(tail) / (SLOTS * WG)
    return makespan(work) / ideal, combine / ideal


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-n", type=int, default=20)
    ap.add_argument("--seed", type=int, default=1)
    a = ap.parse_args()
    cnt = loads(a.log_n, np.random.default_rng(a.seed))
    print("order        tail        makespan/ideal  + combine/ideal")
    for name, g in (("per window", False), ("all windows", True)):
        for label, frac_log, log_split in (("none", None, 0), ("1/8 x 4", 3, 2), ("1/16 x 4", 4, 2), ("1/32 x 2", 5, 1), ("1/64 x 2", 6, 1)):
            m, c = schedule(cnt, g, frac_log, log_split)
            print("%-12s %-11s %.3f           %.3f" % (name, label, m, c))


if __name__ == "__main__":
    main()
