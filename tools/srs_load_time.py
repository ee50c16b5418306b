"""Load and save times of a serialized KZG setup (UnivariateProverParam.deserialize / serialize: mzk_srs_register_serialized,
mzk_srs_serialize) on both curves, both modes (compressed / uncompressed) and both validate settings, by point count.  Splits each
into the library's profile regions -- load: host-to-device copy, decode kernel, internal MSM table; save: encode kernel, device-to-host
copy -- plus the wall time of the whole call.  Writes $OUT/srs_load_time.json (OUT defaults to the current directory) and prints one line per case.
    python tools/srs_load_time.py [log_n ...]          (default: 20 24)"""
import json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import mpc_jellyfish_amd as mj
from importlib import import_module

lib = import_module("mpc-jellyfish_amd.lib")
L = lib.ensure_init()
sizes = [int(a) for a in sys.argv[1:]] or [20, 24]
region = lambda name: lib.profile_get(name)[0]
rows = []
for lg in sizes:
    for cid in (0, 1):
        c = mj.params.CURVES[cid]
        n = 1 << lg
        pp = mj.UnivariateProverParam.gen_srs_for_testing(c, 0x5EED, n - 1)
        want = pp.powers_of_g(n - 5, 5)
        for compress in (True, False):
            L.mzk_profile_enable(1)
            L.mzk_profile_reset()
            t0 = time.perf_counter()
            data = np.frombuffer(pp.serialize(compress), dtype=np.uint8)
            save_ms = (time.perf_counter() - t0) * 1e3
            save = {"encode_ms": region("srs_save.encode"), "copy_ms": region("srs_save.copy"), "total_ms": save_ms}
            for validate in (True, False):
                deserialize = lambda: mj.UnivariateProverParam.deserialize(c, data, compress=compress, validate=validate)
                deserialize().release()                                  # warm-up (code objects, allocator)
                L.mzk_profile_reset()
                t0 = time.perf_counter()
                back = deserialize()
                load_ms = (time.perf_counter() - t0) * 1e3
                assert np.array_equal(back.powers_of_g(n - 5, 5), want)
                back.release()
                row = {"curve": c.name, "points": n, "compressed": compress, "validate": validate, "bytes": int(data.shape[0]),
                       "load": {"copy_ms": region("srs_load.copy"), "decode_ms": region("srs_load.decode"), "table_ms": region("srs_load.table"),
                                "total_ms": load_ms},
                       "save": save}
                rows.append(row)
                print(json.dumps(row), flush=True)
            L.mzk_profile_enable(0)
        pp.release()
out = os.environ.get("OUT", ".")
os.makedirs(out, exist_ok=True)
with open(os.path.join(out, "srs_load_time.json"), "w") as f:
    json.dump(rows, f, indent=1)
