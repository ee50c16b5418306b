"""CPU: the hold on a context's shared workspace (csrc/internal.hpp WsHold) waits once when it is acquired and records once on EVERY
return path -- the normal one, an MZK_TRY early return, nested holds in stack order -- and records nothing when the acquire failed or
never happened.  Host logic only: tools/ws_hold_check.cpp includes internal.hpp and stubs the hold's two HIP calls, so it needs the HIP
headers but no HIP library and no GPU; built plain and with the address and undefined-behaviour sanitizers (a stand-alone program)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tools", "ws_hold_check.cpp")
INC = os.path.join(ROOT, "mpc-jellyfish_amd", "csrc")
ROCM_INC = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "include")
CASES = ["(a)", "(b)", "(c)", "(d)", "(d')", "(d'')", "(e)", "(e')"]


@pytest.mark.parametrize("name,flags", [("plain", ["-O2"]), ("asan_ubsan", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])])
def test_hold_call_sequences(tmp_path, name, flags):
    exe = str(tmp_path / ("ws_hold_check_" + name))
    subprocess.check_call(["g++", "-std=c++17", "-pthread", "-Wall", "-Werror", "-I", ROCM_INC, "-D__HIP_PLATFORM_AMD__", "-I", INC, "-o", exe, SRC] + flags)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and out.stdout.splitlines()[-1] == "ws hold: ok", out.stdout + out.stderr
    lines = out.stdout.splitlines()[:-1]
    assert [ln.split()[0] for ln in lines] == CASES and all(ln.endswith(" ok") for ln in lines), out.stdout
    assert "Sanitizer" not in out.stderr and "runtime error" not in out.stderr, out.stderr
