"""CPU: the container checks of a serialized KZG setup (kzg.UnivariateProverParam / UnivariateUniversalParams.deserialize) raise
SerializationError before any device call, and the endomorphism constant of the G1 membership test (csrc/gen_constants.py) is the
cube root of unity for which phi(G) = -[u^2]G holds at the generator."""
import numpy as np
import pytest


def _container(n, rec, tail=0):
    return n.to_bytes(8, "little") + bytes(n * rec + tail)


@pytest.mark.parametrize("curve", [0, 1])
@pytest.mark.parametrize("compress", [True, False])
def test_container_errors_raise_without_a_gpu(mj, curve, compress):
    c = mj.params.CURVES[curve]
    rec, g2 = mj.kzg.g1_record_bytes(c, compress), mj.kzg.g2_record_bytes(c, compress)
    assert (rec, g2) == ((48 if curve == 0 else 32) * (1 if compress else 2), (96 if curve == 0 else 64) * (1 if compress else 2))
    pp_bad = [b"", bytes(7), _container(5, rec)[:-1], _container(5, rec) + b"\0", (6).to_bytes(8, "little") + _container(5, rec)[8:],
              (4).to_bytes(8, "little") + _container(5, rec)[8:], (1 << 63).to_bytes(8, "little")]
    for data in pp_bad:
        for form in (data, memoryview(data), np.frombuffer(data, dtype=np.uint8)):
            with pytest.raises(mj.SerializationError) as e:
                mj.UnivariateProverParam.deserialize(c, form, compress=compress)
            assert e.value.index is None and isinstance(e.value, ValueError)
    full = _container(5, rec, 2 * g2)
    for data in (full[:-1], full + b"\0", (6).to_bytes(8, "little") + full[8:], _container(5, rec, g2), b"\0" * 8):
        with pytest.raises(mj.SerializationError):
            mj.UnivariateUniversalParams.deserialize(c, data, compress=compress)


def test_serialization_error_carries_index_and_reason(mj):
    e = mj.SerializationError("not in the subgroup", 17)
    assert (e.index, e.reason, str(e)) == (17, "not in the subgroup", "point 17: not in the subgroup")


def test_endomorphism_beta(pyref):
    import os
    import re
    pc = pyref.BLS12_381
    q = pc.q
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "mpc-jellyfish_amd", "csrc", "constants.cuh")).read()
    limbs = [int(v, 16) for v in re.search(r"XENDO_BETA\[14\] = \{([^}]*)\}", src).group(1).replace("u", "").split(",")]
    beta = sum(l << (29 * i) for i, l in enumerate(limbs)) * pow(1 << (29 * 14), -1, q) % q
    assert beta != 1 and pow(beta, 3, q) == 1
    u2 = 0xd201000000010000 ** 2
    assert u2 == (0xac45a4010001a402 << 64) | 0x0000000100000000
    g = pyref.g1_gen(pc)
    assert (beta * g[0] % q, g[1]) == pyref.g1_neg(pc, pyref.g1_mul(pc, u2, g))
