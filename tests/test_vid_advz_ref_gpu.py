"""GPU: Advz.disperse against the reference's own `Advz<E, Sha256>::disperse` on the cases of tests/golden/vid_cases.json (curve, k, n, beta,
payload): tests/golden/ref_vid.json, written by integration/rust/src/bin/gen_fixtures.rs (the `vid` family) where the reference can be
built.  That file is what pins the pieces restated from recollection -- above all the 48-byte Z_pad of ark-ff 0.4's field hasher, which decides
the pseudorandom scalar and with it every proof.  Skips while the file is absent, as the other reference-fixture tests do."""
import json
import os

import numpy as np
import pytest

from conftest import ROOT, affine_from_limbs, golden_pt, load_golden

pytestmark = pytest.mark.gpu


def test_reference_vid_fixtures_when_present(gpu, mj, pyref):
    path = os.path.join(ROOT, "tests", "golden", "ref_vid.json")
    if not os.path.exists(path):
        pytest.skip("reference fixtures absent (integration/rust has not been run): parity unpinned")
    ref = json.load(open(path))
    cases = load_golden("vid_cases")
    assert len(ref) == len(cases)
    for case, want in zip(cases, ref):
        assert all(case[f] == want[f] for f in ("curve", "k", "n", "beta", "payload"))
        c, pc = mj.params.CURVES[case["curve"]], pyref.CURVES[case["curve"]]
        beta = int(case["beta"], 16)
        pp = mj.UnivariateProverParam.gen_srs_for_testing(c, beta, mj.checked_fft_size(case["k"]))
        key = mj.keys.OpenKey(c, *mj.kzg.open_key_for_testing(c, beta))
        vid = mj.Advz(c, case["k"], case["n"], pp, key)
        got = vid.disperse(bytes.fromhex(case["payload"]))
        pt = lambda cm: None if cm.is_infinity() else affine_from_limbs(pc, cm.xy)
        assert got.commit.hex() == want["commit"]
        assert got.common.elems_len == want["elems_len"] and got.common.all_evals_digest.hex() == want["all_evals_digest"]
        assert [pt(cm) for cm in got.common.poly_commits] == [golden_pt(p) for p in want["poly_commits"]]
        for sh, ws in zip(got.shares, want["shares"]):
            assert sh.index == ws["index"] and sh.evals == [int(x, 16) for x in ws["evals"]]
            assert pt(sh.aggregate_proof) == golden_pt(ws["aggregate_proof"])
            assert [[bytes(s).hex() for s in level] for level in np.asarray(sh.evals_proof)] == ws["siblings"]
        assert vid.verify_shares(got.shares, got.common) == [True] * case["n"]
        key.release()
        pp.release()
