"""GPU: UnivariateKzgPCS.multi_open_rou against the reference's own `UnivariatePCS::multi_open_rou` on the cases of
tests/golden/multi_open_cases.json: tests/golden/ref_multi_open.json, written by integration/rust/src/bin/gen_fixtures.rs (the `multi_open`
family) where the reference can be built.  Skips while that file is absent, as the other reference-fixture tests do."""
import json
import os

import pytest

from conftest import ROOT, affine_from_limbs, fr_mont_limbs, golden_pt, load_golden

pytestmark = pytest.mark.gpu


def test_reference_multi_open_fixtures_when_present(gpu, mj, pyref):
    path = os.path.join(ROOT, "tests", "golden", "ref_multi_open.json")
    if not os.path.exists(path):
        pytest.skip("reference fixtures absent (integration/rust has not been run): parity unpinned")
    ref = json.load(open(path))
    cases = load_golden("multi_open_cases")
    assert len(ref) == len(cases)
    for case, want in zip(cases, ref):
        assert all(case[f] == want[f] for f in ("curve", "beta", "coeffs", "num_points"))
        c, pc = mj.params.CURVES[case["curve"]], pyref.CURVES[case["curve"]]
        coeffs = [int(x, 16) for x in case["coeffs"]]
        pp = mj.UnivariateProverParam.gen_srs_for_testing(c, int(case["beta"], 16), len(coeffs))
        dom = mj.UnivariateKzgPCS.multi_open_rou_eval_domain(c, len(coeffs) - 1, case["num_points"])
        assert dom.size == want["domain_size"]
        proofs, evals = mj.UnivariateKzgPCS.multi_open_rou(pp, fr_mont_limbs(pc, coeffs), case["num_points"], dom)
        assert evals == [int(x, 16) for x in want["evals"]]
        assert [None if p.is_infinity() else affine_from_limbs(pc, p.xy) for p in proofs] == [golden_pt(p) for p in want["proofs"]]
        pp.release()
