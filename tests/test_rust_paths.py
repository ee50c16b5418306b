"""CPU suite: integration/rust/ (the Rust shim and the fixture generator -- source only, never compiled here) names only items
that exist in the reference tree (tools/check_rust_paths.py).  Where the reference is absent, against the recorded results of that
check (tests/golden/rust_paths.json, written by tests/golden/make_rust_paths.py); where it is present, live as well."""
import os
import re
import subprocess
import sys

from conftest import load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import check_rust_paths as crp  # noqa: E402


def test_rust_sources_name_existing_reference_items():
    recorded = {(c["file"], c["pattern"]): c["found"] for c in load_golden("rust_paths")["checks"]}
    flat = re.sub(r"\s+", " ", "\n".join(open(p).read() for p in crp.RUST))
    for rel, pattern, token in crp.CHECKS:
        assert recorded.get((rel, pattern)) is True, "no recorded match of /%s/ in %s (re-run tests/golden/make_rust_paths.py)" % (pattern, rel)
        assert re.sub(r"\s+", " ", token) in flat, "integration/rust no longer contains `%s`" % token
    # the live check (a no-op that says so where the reference tree is absent)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "check_rust_paths.py")], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout
