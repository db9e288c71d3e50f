"""bench.py's plain run (the headline alone) and --dump-outputs (the last timed step's junction table as .npy files)."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture
def bench(monkeypatch):
    # bench.py sets GPU_MAX_HW_QUEUES for its own process when it is imported: keep that out of the test process's environment
    monkeypatch.setenv("GPU_MAX_HW_QUEUES", os.environ.get("GPU_MAX_HW_QUEUES", "4"))
    import bench
    return bench


def _table(n):
    from regtools_amd import _ffi
    t, keep, r = _ffi.JunctionTable(), [], np.arange(n)

    def arr(ct, vals):
        a = (ct * max(n, 1))(*vals)
        keep.append(a)
        return C.cast(a, C.POINTER(ct))
    t.n, t.n_records, t.n_events = n, 1000, 77
    t.tid, t.start, t.end = arr(C.c_int32, r % 24), arr(C.c_uint32, 100 + r), arr(C.c_uint32, 4000000000 - r)
    t.thick_start, t.thick_end, t.read_count = arr(C.c_uint32, r), arr(C.c_uint32, r + 5), arr(C.c_uint32, r % 7 + 1)
    t.name_index = arr(C.c_uint64, r + (1 << 40))
    t.strand = C.cast(arr(C.c_uint8, [ord("+-?"[i % 3]) for i in r]), C.POINTER(C.c_char))
    t.left_ok, t.right_ok = arr(C.c_uint8, r % 2), arr(C.c_uint8, (r + 1) % 2)
    return C.pointer(t), keep


@pytest.mark.parametrize("n", [0, 5, 2_000_000])
def test_dump_outputs_writes_every_column_within_64_mb(bench, tmp_path, n):
    tab, keep = _table(n)
    bench.dump_outputs(tab, str(tmp_path))
    names = sorted(bench.DUMP_COLUMNS + ("row_index", "totals"))
    assert sorted(f[:-4] for f in os.listdir(tmp_path)) == names
    assert sum(os.path.getsize(tmp_path / (f + ".npy")) for f in names) <= 64_000_000
    got = {f: np.load(tmp_path / (f + ".npy")) for f in names}
    assert all(a.dtype == np.float64 for a in got.values())
    assert got["totals"].tolist() == [n, 1000, 77]
    idx = got["row_index"].astype(np.int64)
    if n <= 5:
        assert idx.tolist() == list(range(n))
    else:                                             # an evenly spaced sample: first row first, strictly increasing, the same on every call
        assert 0 < len(idx) < n and idx[0] == 0 and (np.diff(idx) > 0).all() and idx[-1] < n
    assert (got["end"] == 4000000000 - idx).all() and (got["name_index"] == idx + (1 << 40)).all()
    assert (got["strand"] == [ord("+-?"[i % 3]) for i in idx]).all() and (got["tid"] == idx % 24).all()
    assert (got["left_ok"] == idx % 2).all() and (got["right_ok"] == (idx + 1) % 2).all()


@pytest.mark.gpu
def test_plain_run_prints_the_headline_and_dumps_the_last_steps_table(gpu_ctx, bench, tmp_path):
    """A plain run times exactly --steps steps and reports only what they measured; --dump-outputs holds the table an independent extraction
    of the same seeded input makes (and --dump-bed its BED12)."""
    import regtools_amd
    from regtools_amd import synth
    out, bed = tmp_path / "outputs", tmp_path / "last.bed"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--reads", "200000",
                        "--dump-outputs", str(out), "--dump-bed", str(bed)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    line = json.loads([l for l in r.stdout.decode().splitlines() if l.startswith("{")][-1])
    assert line["steps"] == 3 and line["warmup"] == 1 and line["ms_per_step"] > 0 and line["value"] > 0
    assert line["unit"] == "alignments/s" and line["higher_is_better"] is True and line["dtype"] == "u8/u32 integer"
    assert not {"roofline", "cpu_baseline", "sustained", "stage_ms", "value_device_resident", "cli", "realistic"} & set(line)
    bam, bai, _ = synth.generate(200000, shape="short", seed=1)
    je = regtools_amd.JunctionsExtractor(strandness=0, ctx=gpu_ctx)
    je.identify_junctions_from_BAM(bam_bytes=bam, bai_bytes=bai)
    here = tmp_path / "here"
    bench.dump_outputs(je.table, str(here))
    assert line["junction_rows"] == je.stats["n_junctions"] > 0
    for f in sorted(os.listdir(here)):
        assert np.array_equal(np.load(out / f), np.load(here / f)), f
    assert bed.read_bytes() == je.bed12()
