"""Dev container only: runs the REAL reference (oracle/_ref/regtools_ref) on every file of tests/layout_cases.py under every argument list and stores
its exit status, the SHA-256 and the row count of its BED12, and a digest of the inputs -> tests/golden/layout/layout_ref.json.
Digests, not text: when one differs, the oracle's text names the row.   python tests/golden/make_golden_layout.py"""
import hashlib, json, os, subprocess, sys, tempfile
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import layout_cases
REF = os.path.join(ROOT, "oracle", "_ref", "regtools_ref")
gold = {}
with tempfile.TemporaryDirectory() as td:
    for name in layout_cases.NAMES:
        case = layout_cases.build(name, td)
        gold[name] = {"inputs_sha256": case.digest, "runs": {}}
        for args in case.arglists:
            r = subprocess.run([REF, "junctions", "extract"] + case.argv(args), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
            gold[name]["runs"][" ".join(args)] = {"rc": r.returncode, "sha256": hashlib.sha256(r.stdout).hexdigest(), "rows": r.stdout.count(b"\n")}
            print(name, " ".join(args), r.returncode, r.stdout.count(b"\n"), case.planted[" ".join(args)])
        os.remove(case.path)
os.makedirs(os.path.join(ROOT, "tests", "golden", "layout"), exist_ok=True)
with open(os.path.join(ROOT, "tests", "golden", "layout", "layout_ref.json"), "w") as f:
    json.dump(gold, f, indent=0, sort_keys=True)
    f.write("\n")
