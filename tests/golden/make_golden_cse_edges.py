#!/usr/bin/env python
"""What the REAL reference (oracle/_ref/regtools_ref) makes of the files of tests/cse_edge_cases.py: `junctions annotate` (with and without -S) on the
junction cases whose contigs are small enough for a FASTA, `variants annotate` under all eighteen option sets on the variant case, both in the
3-contig and in the 230-contig layout.  Written to tests/golden/cse_edges/ref.json: per run the exit status, the row count, the SHA-256 of the
columns the kernels decide (tests/cse_edge_common.py) and the first rows of them; per case the digest of its inputs, so that a builder that
drifts fails tests/test_cse_edges_host.py.  Data only.  Dev container only."""
import json
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import cse_edge_cases as ec  # noqa: E402
import cse_edge_common as cm  # noqa: E402

REF = os.path.join(ROOT, "oracle", "_ref", "regtools_ref")


def main():
    out = {}
    with tempfile.TemporaryDirectory() as td:
        for layout in ec.LAYOUTS:
            for name in cm.FILE_JUNCTION_CASES:
                c = ec.build(name, td, layout)
                runs = {}
                for args in cm.JUNCTION_RUNS:
                    o = os.path.join(td, "ja.tsv")
                    r = subprocess.run([REF, "junctions", "annotate"] + args + ["-o", o, c.bed, c.fasta, c.gtf], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
                    rows = cm.junction_columns(open(o, "rb").read())
                    runs[" ".join(args)] = dict(rc=r.returncode, rows=len(rows), sha256=cm.digest(rows), head=[list(x[:5]) for x in rows[:3]])
                    print(name, layout, args, r.returncode, len(rows))
                out["%s/%s" % (name, layout)] = dict(inputs_sha256=c.digest, runs=runs)
            c = ec.build("V_edges", td, layout)
            runs = {}
            for args in cm.VARIANT_RUNS:
                o = os.path.join(td, "va.vcf")
                r = subprocess.run([REF, "variants", "annotate"] + args + ["-o", o, c.vcf, c.gtf], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
                rows = cm.variant_columns(open(o, "rb").read())
                runs[" ".join(args)] = dict(rc=r.returncode, rows=len(rows), sha256=cm.digest(rows), hits=sum(x[2] != "NA" for x in rows))
                print("V_edges", layout, args, r.returncode, len(rows))
            out["V_edges/%s" % layout] = dict(inputs_sha256=c.digest, runs=runs)
    os.makedirs(os.path.join(HERE, "cse_edges"), exist_ok=True)
    json.dump(out, open(os.path.join(HERE, "cse_edges", "ref.json"), "w"), indent=1, sort_keys=True)


if __name__ == "__main__":
    main()
