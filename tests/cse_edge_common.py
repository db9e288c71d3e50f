"""Shared by tests/test_cse_edges_host.py, tests/test_gpu_cse_edges.py and tests/golden/make_golden_cse_edges.py (TEST INFRASTRUCTURE): which runs
the file-level checks make of the cases of tests/cse_edge_cases.py, and the columns of an annotate command's output that the kernels decide."""
import hashlib

import cse_edge_cases as ec

FILE_JUNCTION_CASES = ["J_totals", "J_setter_known", "J_setter_donor", "J_setter_acceptor", "J_items"]      # contigs of at most 200 kb: a FASTA is written
JUNCTION_RUNS = [[], ["-S"]]


def variant_args(o):
    return ["-i", str(o["intronic_min"]), "-e", str(o["exonic_min"])] + (["-I"] if o["all_intronic"] else []) + (["-E"] if o["all_exonic"] else []) + \
           ([] if o["skip_single"] else ["-S"])


VARIANT_RUNS = [variant_args(o) for o in ec.VARIANT_OPTS]


def junction_columns(tsv_bytes):
    """[(name, acceptors, exons, donors skipped, anchor, transcripts)] of a `junctions annotate` table, in file order"""
    rows = []
    for line in tsv_bytes.decode().splitlines()[1:]:
        f = line.split("\t")
        rows.append((f[3], int(f[7]), int(f[8]), int(f[9]), f[10], f[16]))
    return rows


def variant_columns(vcf_bytes):
    """[(contig, position, transcripts, distances, annotations)] of a `variants annotate` file, in file order"""
    rows = []
    for line in vcf_bytes.decode().splitlines():
        if line.startswith("#"):
            continue
        f = line.split("\t")
        info = dict(x.split("=", 1) for x in f[7].split(";") if "=" in x)
        rows.append((f[0], int(f[1]), info["transcripts"], info["distances"], info["annotations"]))
    return rows


def digest(rows):
    return hashlib.sha256("\n".join("\t".join(str(x) for x in r) for r in rows).encode()).hexdigest()


ANCHOR = {0: "N", 1: "D", 2: "A", 3: "NDA"}


def anchor_of(flags):
    return "DA" if flags & 4 else ANCHOR[flags & 3]
