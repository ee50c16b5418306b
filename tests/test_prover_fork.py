"""CPU: mzk_prover_fork and mzk_prover_shared_hbm_bytes are declared in include/mzk.h, exported by libmi355zk.so and bound by
mpc-jellyfish_amd/lib.py; without a device (or with one, on a handle nobody made) both return an error code instead of crashing."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("mzk_prover_fork", "mzk_prover_shared_hbm_bytes")
ERR_BAD_HANDLE = -4


def test_header_declares_and_library_exports_the_fork_calls(mj):
    text = open(os.path.join(ROOT, "include", "mzk.h")).read()
    declared = set(re.findall(r"MZK_API\s+[\w\s\*]+?\b(mzk_\w+)\s*\(", text))
    from importlib import import_module
    lib = import_module("mpc-jellyfish_amd.lib")
    L = mj.load()
    for name in NEW:
        assert name in declared, name + " is not declared in include/mzk.h"
        assert hasattr(L, name), name + " is not exported by libmi355zk.so"
        assert name in lib.EXPORTS
    assert "world > 1" in text[text.index("MZK_API int32_t mzk_prover_fork") - 2500:text.index("MZK_API int32_t mzk_prover_fork")]


def test_fork_calls_fail_cleanly_on_a_handle_nobody_made(mj):
    L = mj.load()
    out, shared, sharers = C.c_uint64(7), C.c_uint64(7), C.c_uint32(7)
    for handle in (0, 12345, (1 << 48) | 99):
        assert L.mzk_prover_fork(handle, C.byref(out)) == ERR_BAD_HANDLE
        assert L.mzk_prover_fork(handle, None) == ERR_BAD_HANDLE
        assert L.mzk_prover_shared_hbm_bytes(handle, C.byref(shared), C.byref(sharers)) == ERR_BAD_HANDLE
        assert L.mzk_prover_shared_hbm_bytes(handle, None, None) == ERR_BAD_HANDLE
    assert b"unknown prover handle" in L.mzk_last_error()
    assert (out.value, shared.value, sharers.value) == (7, 7, 7)      # nothing written on failure
