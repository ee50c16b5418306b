"""Load time of a serialized ProvingKey (keys.ProvingKey.deserialize: mzk_prover_create_serialized) at 2^20 gates, TurboPlonk / BLS12-381
and UltraPlonk / BN254, compressed and validated, on one GPU -- end to end and by region -- against the route the library offered before
for the same key: mzk_srs_register_serialized for the commit key plus mzk_prover_create from Montgomery host arrays, with and without
the byte-to-Montgomery conversion that route leaves to the caller.
  copy        the image's one host-to-device copy, timed on its own (mzk_dev_upload of the same bytes)
  fr_decode   the one mzk_fr_decode_dev launch over all polynomials and k, timed on its own on the staged image (it synchronises)
  g1_decode   the library's profile regions srs_load.decode / srs_load.table inside the load (commit key: decode, internal table)
  rest        end to end minus those: the prover's own set-up (class evaluations, workspace) and the container parse
The caller's conversion is timed on a sample of 2^14 records with params.fr_to_mont (Python big integers) and scaled to the key's count:
an EXTRAPOLATION, printed as such.  Prints one JSON line per case.
    python tools/key_io_time.py [--log-n 20] [--only turbo|ultra] [--reps 3]"""
import argparse, ctypes as C, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import mpc_jellyfish_amd as mj
from importlib import import_module

ap = argparse.ArgumentParser()
ap.add_argument("--log-n", type=int, default=20)
ap.add_argument("--only", choices=("turbo", "ultra"))
ap.add_argument("--reps", type=int, default=3)
args = ap.parse_args()
lib = import_module("mpc-jellyfish_amd.lib")
L = lib.ensure_init()
med = lambda xs: sorted(xs)[len(xs) // 2]


def timed(f, reps=args.reps):
    out = []
    for _ in range(reps):
        L.mzk_dev_sync()
        t0 = time.perf_counter()
        r = f()
        L.mzk_dev_sync()
        out.append((time.perf_counter() - t0) * 1e3)
        if hasattr(r, "release"):
            r.release()
    return round(med(out), 3), round(min(out), 3)


for cid, kind in ((0, "TurboPlonk"), (1, "UltraPlonk")):
    if args.only and args.only != kind[:5].lower():
        continue
    c = mj.params.CURVES[cid]
    cs = mj.snark.gen_circuit_for_bench(c, 1 << args.log_n, kind)
    n, W, nsel = cs.n, 6 if kind == "UltraPlonk" else 5, 14 if kind == "UltraPlonk" else 13
    ck = mj.UnivariateProverParam.gen_srs_for_testing(c, 0x1234567, n + 2)
    pk = mj.snark.preprocess(ck, cs, lagrange=False, from_structure=True)
    g2 = mj.kzg.g2_record_bytes(c)
    image = np.frombuffer(pk.serialize_key(0, bytes(g2), bytes(g2)), dtype=np.uint8)
    pk.release()
    ck.release()
    lay = mj.key_layout(c, image)
    load = lambda: mj.ProvingKey.deserialize(c, image, compress=True, validate=True)
    load().release()                                                # warm-up (code objects, allocator, MSM-free path)
    L.mzk_profile_enable(1)
    L.mzk_profile_reset()
    total = timed(load)
    regions = {k: round(lib.profile_get("srs_load." + k)[0] / args.reps, 3) for k in ("decode", "table")}
    L.mzk_profile_enable(0)
    # the regions on their own
    d_img = C.c_void_p()
    lib.check(L.mzk_dev_alloc(image.shape[0] + 32, C.byref(d_img)), "alloc")
    copy = timed(lambda: lib.check(L.mzk_dev_upload(d_img, C.c_void_p(image.ctypes.data), image.shape[0]), "upload"))
    segs = [(lay.sigma_off[i], lay.sigma_len[i]) for i in range(W)] + [(lay.selector_off[i], lay.selector_len[i]) for i in range(nsel)] + \
           [(lay.table_off[i], lay.table_len[i]) for i in range(4 if W == 6 else 0)]
    src, cnt = (np.array([s[i] for s in segs], dtype=np.uint64) for i in (0, 1))
    row = np.arange(len(segs), dtype=np.uint32)
    rows = torch.empty((len(segs), n, 4), dtype=torch.int64, device="cuda")
    p = lambda a: C.c_void_p(a.ctypes.data)
    fr = timed(lambda: lib.check(L.mzk_fr_decode_dev(cid, d_img, image.shape[0], len(segs), p(src), p(cnt), p(row), C.c_void_p(rows.data_ptr()), len(segs), n,
                                                     None, None, None), "mzk_fr_decode_dev"))
    L.mzk_dev_free(d_img)
    # the former route: the commit key from its records, the prover from Montgomery host arrays (here: the decoded rows, downloaded)
    host = rows.cpu().numpy().view(np.uint64)
    del rows
    sig_p, sel_p = list(host[:W]), list(host[W:W + nsel])
    plookup = dict(zip(mj.plonk.PLOOKUP_TABLE_POLYS, host[W + nsel:])) if W == 6 else None
    k = [int.from_bytes(bytes(image[lay.k_off + 32 * i:lay.k_off + 32 * i + 32]), "little") for i in range(W)]
    records = image[lay.commit_key_off - 8:lay.commit_key_off + lay.commit_key_count * lay.g1_record_bytes]

    def former():
        srs = mj.UnivariateProverParam.deserialize(c, records, compress=True, validate=True)
        pr = mj.prover.TurboPlonkProver(c, n, sel_p, sig_p, k, srs, plookup=plookup)
        pr.owned_keys = [srs]
        return pr

    former().release()
    old = timed(former)
    sample = 1 << 14
    ints = [int.from_bytes(bytes(image[lay.sigma_off[0] + 32 * i:lay.sigma_off[0] + 32 * i + 32]), "little") for i in range(sample)]
    t0 = time.perf_counter()
    mj.params.fr_to_mont(c, ints)
    conv_ms = (time.perf_counter() - t0) * 1e3 * (sum(int(x) for x in cnt) / sample)
    print(json.dumps({"curve": c.name, "plonk_type": kind, "log_n": n.bit_length() - 1, "image_bytes": int(image.shape[0]), "fr_records": int(sum(int(x) for x in cnt)),
                      "g1_records": int(lay.commit_key_count), "deserialize": {"median_ms": total[0], "min_ms": total[1]},
                      "copy": {"median_ms": copy[0], "min_ms": copy[1]}, "fr_decode": {"median_ms": fr[0], "min_ms": fr[1]},
                      "g1_decode_ms": regions["decode"], "g1_table_ms": regions["table"],
                      "rest_ms": round(total[0] - copy[0] - fr[0] - regions["decode"] - regions["table"], 3),
                      "former_route_montgomery_arrays": {"median_ms": old[0], "min_ms": old[1]},
                      "former_route_with_python_conversion_extrapolated_ms": round(old[0] + conv_ms, 1)}), flush=True)
