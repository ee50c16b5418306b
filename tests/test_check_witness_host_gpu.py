"""GPU: `mzk_prove ... --check-witness` (mpc-jellyfish_amd/host/): the compiled host says where a witness fails before it proves, and
does not prove a witness that fails.  Every run is a fresh child process with a time limit of its own."""
import json
import os
import random
import subprocess
from importlib import import_module

import pytest

import check_witness_ref as REF
from conftest import build_circuit, build_ultra_circuit

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "mpc-jellyfish_amd", "mzk_prove")


def _run(*args, env=None):
    if not os.path.exists(BIN):                                        # normally built by __graft_entry__.build()
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "mpc-jellyfish_amd", "host"), "-s"])
    return subprocess.run([BIN] + [str(a) for a in args], capture_output=True, text=True, timeout=120, env=env)


@pytest.mark.parametrize("curve_id,ultra,log_n", [(0, False, 6), (1, True, 6)])
def test_file_circuit_good_and_with_one_changed_wire(gpu, mj, pyref, tmp_path, curve_id, ultra, log_n):
    io = import_module("mpc-jellyfish_amd.circuit_io")
    c, pc = mj.params.CURVES[curve_id], pyref.CURVES[curve_id]
    rng = random.Random(640 + curve_id)
    tabs = None
    if ultra:
        sel, sig, k, w, pi, tabs = build_ultra_circuit(pc, log_n, rng)
    else:
        sel, sig, k, w, pi = build_circuit(pc, log_n, rng)
    good, bad_path = str(tmp_path / "good.mzkc"), str(tmp_path / "bad.mzkc")
    io.write_circuit(good, c, log_n, sel, sig, k, w, pub_input=pi[:4], tables=tabs)
    out = _run(curve_id, "file", good, 0, "--check-witness")
    assert out.returncode == 0, out.stderr[-2000:]
    lines = out.stdout.strip().splitlines()
    assert lines[0].startswith("witness: satisfied; failing gate rows 0, lookup rows 0, copy cells 0")
    with_check = json.loads(lines[-1])["proof_hex"]
    plain = _run(curve_id, "file", good, 0)
    assert plain.returncode == 0 and "witness:" not in plain.stdout and json.loads(plain.stdout.strip().splitlines()[-1])["proof_hex"] == with_check
    # the output wire of a gated row (here the first multiplication row)
    R = next(i for i in range(1 << log_n) if sel[4][i])
    bad = [col[:] for col in w]
    bad[4][R] = (bad[4][R] + 1) % pc.r
    io.write_circuit(bad_path, c, log_n, sel, sig, k, bad, pub_input=pi[:4], tables=tabs)
    out = _run(curve_id, "file", bad_path, 0, "--check-witness")
    assert out.returncode == 3 and "proof_hex" not in out.stdout, (out.returncode, out.stderr[-2000:])
    residual = REF.gate_residual(pc, sel, bad, pi, R)
    assert out.stdout.strip() == "witness: gate row %d residual 0x%064x; failing gate rows 1, lookup rows 0, copy cells 0 " \
                                 "(copy constraints not checked: no wire-variable table)" % (R, residual)
    # without the flag the same file is refused only at the end of the proof, without a row
    out = _run(curve_id, "file", bad_path, 0)
    assert out.returncode == 1 and "WrongQuotientPolyDegree" in out.stderr


def test_bench_circuit_and_several_devices(gpu):
    """turbo / ultra bench circuits; the witness vector gathered through the wire variables (copy constraints hold by construction);
    with --gpus 2 rank 0 checks alone"""
    out = _run(0, "turbo", 64, 0, "--check-witness")
    assert out.returncode == 0 and out.stdout.startswith("witness: satisfied; failing gate rows 0, lookup rows 0, copy cells 0 (copy"), out.stderr[-2000:]
    out = _run(1, "ultra", 64, 0, 4, "--check-witness", "--host-witness-vars")
    assert out.returncode == 0 and out.stdout.splitlines()[0] == "witness: satisfied; failing gate rows 0, lookup rows 0, copy cells 0", out.stderr[-2000:]
    env = dict(os.environ, MZK_PROVE_CORRUPT_WITNESS="1")              # wire 0 of row 5 takes the value of row 6
    out = _run(0, "turbo", 64, 0, "--check-witness", env=env)
    assert out.returncode == 3 and out.stdout.startswith("witness: gate row 5 residual 0x" + "0" * 63 + "1;") and "proof_hex" not in out.stdout
    env["MZK_VIRTUAL_DEVICES"] = "2"
    out = _run(0, "turbo", 64, 0, "--gpus", 2, "--check-witness", env=env)
    assert out.returncode == 3 and out.stdout.startswith("witness: gate row 5 residual 0x"), out.stderr[-2000:]
    out = _run(0, "turbo", 64, 0, "--gpus", 2, "--check-witness", env=dict(os.environ, MZK_VIRTUAL_DEVICES="2"))
    assert out.returncode == 0 and out.stdout.startswith("witness: satisfied") and "proof_hex" in out.stdout, out.stderr[-2000:]
