"""tests/golden/make_rust_paths.py [reference_root] -- records, for every check of tools/check_rust_paths.py, whether its pattern is
found in the reference tree, so that tests/test_rust_paths.py can check integration/rust/ against the table where the reference is
absent.  The fixture holds file names, the patterns and the results: nothing of the reference's text.

    python tests/golden/make_rust_paths.py [reference_root]      # rewrites rust_paths.json
"""
import json
import os
import re
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "..", "tools"))
import check_rust_paths as crp  # noqa: E402


def main() -> int:
    ref = sys.argv[1] if len(sys.argv) > 1 else crp.REF
    if not os.path.isdir(ref):
        print("reference tree %s absent" % ref)
        return 1
    checks = []
    for rel, pattern, _ in crp.CHECKS:
        path = os.path.join(ref, rel)
        found = os.path.exists(path) and re.search(pattern, open(path).read(), re.M | re.S) is not None
        checks.append({"file": rel, "pattern": pattern, "found": bool(found)})
    with open(os.path.join(HERE, "rust_paths.json"), "w") as f:
        json.dump({"what": "tools/check_rust_paths.py run against the reference tree: is each pattern found in its file", "checks": checks}, f, indent=1)
        f.write("\n")
    print("%d checks, %d not found" % (len(checks), sum(not c["found"] for c in checks)))
    return 0


if __name__ == "__main__":
    sys.exit(main())
