"""The general-circuit cases (oracle/pyref_circuit.py general_circuit / general_ultra_circuit) that the GPU tests prove, as data: the
CPU suite (test_golden_proofs.py) builds every one of them and asserts what the GPU comparisons rely on -- with gates="all" no selector
column is zero, and every row satisfies the gate identity.  Each entry: (curve id, UltraPlonk?, log2 domain size); the seed of the
builder's rng is a function of the entry, stated beside the list."""
import pytest

# tests/test_native_prover_gpu.py::test_round_level_abi_on_general_circuits
ROUND_LEVEL = [(0, False, 6), (1, False, 9), (1, True, 6), (0, True, 8), (0, False, 3), (1, True, 4), (0, False, 12)]
ROUND_LEVEL_ALL_ONLY = [(1, False, 14)]             # every residue class in one launch per step, W classes + top coefficients, live q_hash / q_ecc
round_level_seed = lambda curve_id, ultra, log_n: 9100 + curve_id + 2 * ultra + log_n

# tests/test_native_prover_gpu.py::test_unsatisfied_witness_is_rejected_under_the_reference_error_name
UNSATISFIED = [(0, False, 6), (1, True, 6), (1, False, 3)]
unsatisfied_seed = lambda curve_id, ultra, log_n: 77 + curve_id

# tests/test_native_prover_gpu.py::test_batch_prove_over_native_handles_matches_the_mirror: three instances drawn from one rng
BATCH = [(0, False, 5), (1, True, 5)]
batch_seed = lambda curve_id, ultra, log_n: 600 + curve_id

# tests/test_verifier_gpu.py::test_proof_with_public_input_and_copy_constraints_verifies
VERIFIER = [(0, False, 6), (1, False, 9), (1, True, 6), (0, True, 8)]
verifier_seed = lambda curve_id, ultra, log_n: 4100 + curve_id + 2 * ultra

# tests/test_host_cpp_gpu.py::test_cpp_host_proves_a_general_circuit_from_a_file: (..., devices)
CPP_FILE = [(0, False, 6, 1), (1, True, 6, 1), (1, False, 9, 1), (0, True, 8, 1), (0, False, 7, 3), (1, True, 6, 2)]
CPP_FILE_ALL_ONLY = [(1, False, 7, 2), (0, True, 6, 3)]     # with CPP_FILE: Turbo and Ultra at 1, 2 and 3 devices
cpp_file_seed = lambda curve_id, ultra, log_n: 31 + curve_id + log_n


def with_gates(cases, all_only=()):
    """`cases` with gates="hot" under the ids they have always had, then `cases + all_only` with gates="all" (id suffix -all)."""
    name = lambda case: "-".join(str(x) for x in case)
    return [pytest.param(*case, "hot", id=name(case)) for case in cases] + [pytest.param(*case, "all", id=name(case) + "-all") for case in list(cases) + list(all_only)]


def nonzero_selectors(sel):
    """how many entries of each selector column are non-zero"""
    return [sum(1 for v in col if v) for col in sel]
