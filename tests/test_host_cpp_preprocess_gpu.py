"""GPU: `mzk_prove ... --device-preprocess` (mpc-jellyfish_amd/host/) -- the compiled host hands the bench circuit's selector values and
variable table to mzk_prover_create_from_circuit_dev instead of computing the wire permutation and the sigma values on one CPU core:
the proof and the verifying key must keep their bytes.  A circuit file holds sigma values, not variables: there the flag is refused."""
import json
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "mpc-jellyfish_amd", "mzk_prove")


def _run(args, **kw):
    return subprocess.run([BIN] + [str(a) for a in args], capture_output=True, text=True, timeout=600, **kw)


@pytest.mark.parametrize("args", [(0, "turbo", 4096, 0), (1, "ultra", 40, 0, 3), (0, "turbo", 4096, 0, 8, "--host-witness-vars")])
def test_device_preprocess_keeps_the_bytes(gpu, args):
    outs = []
    for extra in ([], ["--device-preprocess"]):
        out = _run(list(args) + extra)
        assert out.returncode == 0, out.stderr[-2000:]
        outs.append(json.loads(out.stdout.strip().splitlines()[-1]))
    assert outs[0]["proof_hex"] == outs[1]["proof_hex"] and outs[0]["vk_hex"] == outs[1]["vk_hex"]
    assert len(outs[0]["proof_hex"]) > 1000


def test_device_preprocess_is_refused_for_circuit_files(gpu, tmp_path):
    path = tmp_path / "circuit.bin"
    path.write_bytes(b"")
    out = _run([0, "file", path, 0, "--device-preprocess"])
    assert out.returncode == 2 and "--device-preprocess" in out.stderr and "variable" in out.stderr
    assert out.stdout == ""
