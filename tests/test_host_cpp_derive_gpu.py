"""GPU: `mzk_prove ... --check-witness --derive-variables` (mpc-jellyfish_amd/host/): a prover that came from coefficient forms recovers
its wire-variable table from sigma (mzk_prover_derive_wire_variables) and the check covers the copy constraints.  Every run is a fresh
child process with a time limit of its own."""
import json
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "mpc-jellyfish_amd", "mzk_prove")


def _run(*args, env=None):
    if not os.path.exists(BIN):                                        # normally built by __graft_entry__.build()
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "mpc-jellyfish_amd", "host"), "-s"])
    return subprocess.run([BIN] + [str(a) for a in args], capture_output=True, text=True, timeout=120, env=env)


def test_the_copy_family_is_checked_and_the_proof_is_the_same(gpu):
    out = _run(0, "turbo", 1024, 0, "--check-witness", "--derive-variables")
    assert out.returncode == 0, out.stderr[-2000:]
    lines = out.stdout.strip().splitlines()
    assert lines[0] == "witness: satisfied; failing gate rows 0, lookup rows 0, copy cells 0" and "not checked" not in out.stdout
    plain = _run(0, "turbo", 1024, 0, "--check-witness")
    assert plain.returncode == 0 and "copy constraints not checked: no wire-variable table" in plain.stdout.splitlines()[0]
    assert json.loads(lines[-1])["proof_hex"] == json.loads(plain.stdout.strip().splitlines()[-1])["proof_hex"]


def test_a_changed_wire_names_the_copy_cell(gpu):
    """MZK_PROVE_CORRUPT_WITNESS: wire 0 of row 5 takes the value of row 6.  Gate 5 no longer holds, and the cell is the smallest of its
    variable (the sum that wire 4 of row 4 puts out), so that one differs from its representative: cell (4,4) != (0,5)."""
    env = dict(os.environ, MZK_PROVE_CORRUPT_WITNESS="1")
    out = _run(0, "turbo", 1024, 0, "--check-witness", "--derive-variables", env=env)
    assert out.returncode == 3 and "proof_hex" not in out.stdout, (out.returncode, out.stderr[-2000:])
    line = out.stdout.strip()
    assert line.startswith("witness: gate row 5 residual 0x" + "0" * 63 + "1; failing gate rows 1, lookup rows 0, copy cells 1;") and "not checked" not in line
    assert line.endswith("; first copy cell (4,4) != (0,5)")
    out = _run(1, "ultra", 1024, 0, 4, "--check-witness", "--derive-variables", env=env)
    assert out.returncode == 3 and out.stdout.strip().endswith("copy cells 1; first copy cell (4,4) != (0,5)"), (out.stdout, out.stderr[-2000:])


def test_refused_with_a_witness_vector_in_the_circuits_numbering(gpu):
    out = _run(0, "turbo", 64, 0, "--check-witness", "--derive-variables", "--host-witness-vars")
    assert out.returncode == 2 and "--derive-variables" in out.stderr
