"""tools/msm_plain_sizes.py -- single MSMs on the plain path (fixed-base table off) at 2^12 .. 2^21 pairs, both curves: best of 4 means
of 8 calls, ms.  Run it once as it is and once with MZK_MSM_RANK_PER_SET=1 (or any other switch of csrc/msm.hip: read once per
process) from the repository root -> the "where else" section of profiles/r06_global_rank_ab.txt."""
import os, sys, time
sys.path.insert(0, os.getcwd())
import numpy as np, torch
import mpc_jellyfish_amd as mj
from mpc_jellyfish_amd import lib as mlib
L = mlib.ensure_init()
L.mzk_msm_set_precompute(0)
for cid in (0, 1):
    c = mj.params.CURVES[cid]
    for ln in (12, 14, 16, 17, 18, 19, 21):
        n = 1 << ln
        ck = mj.UnivariateProverParam.gen_srs_for_testing(c, 12345, n + 2)
        s = torch.from_numpy(mj.params.random_fr_mont(c, n, seed=3).view(np.int64)).cuda()
        f = lambda: mj.kzg.msm_bigint(ck, s, scalars_are_mont=True)
        for _ in range(3): f()
        torch.cuda.synchronize()
        best = 1e9
        for _ in range(4):
            t0 = time.perf_counter()
            for _ in range(8): f()
            best = min(best, (time.perf_counter() - t0) / 8 * 1e3)
        print("plain rank", "per_set" if os.environ.get("MZK_MSM_RANK_PER_SET") else "global", "curve", cid, "log", ln, "shape", mlib.msm_last_shape(), "ms %.3f" % best, flush=True)
        ck.release()
