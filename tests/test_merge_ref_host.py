"""tests/merge_ref.py on the CPU: the restatement of the merge contract equals the host merge (rgx_table_merge) in every column on every case the
GPU test hands the device merge, and the cases hold what they were built for."""
import ctypes as C

import pytest

import merge_ref as mref

CASES = mref.all_cases()


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_restatement_equals_the_host_merge(built, case):
    from regtools_amd import distributed
    proto, keep = mref.names_table(case.names)
    host = distributed.merge_packed(case.packed_parts(), C.byref(proto), case.min_anchor)
    want = mref.merge(case.parts, case.names, case.min_anchor)
    got = mref.table_columns(host.table)
    for col in mref.COLS:
        assert got[col] == want[col], (case.name, col)
    assert host.n == len(case.keys())


def test_the_cases_hold_what_they_were_built_for():
    by = {c.name: c for c in CASES}
    assert sorted({c.N for c in CASES} & {1, 255, 256, 257, 513}) == [1, 255, 256, 257, 513]
    assert {len(c.parts) for c in CASES} >= {1, 2, 3, 255}
    assert {len(c.names) for c in CASES} >= {1, 2, 3, 256, 257}
    for c in CASES:                                                          # the highest tid is used
        assert max(k[0] for k in c.keys()) == len(c.names) - 1, c.name
        slack_counts = {int(v) for s in c.slack for v in s[:, 5]}
        assert slack_counts <= {999999} and 999999 not in mref.merge(c.parts, c.names, c.min_anchor)["read_count"]
    assert len(by["N255_one_key_in_255_parts"].keys()) == 1
    assert len(by["N256_all_distinct"].keys()) == 256
    assert all(len(p) == 64 for p in by["every_key_in_every_part"].parts) and len(by["every_key_in_every_part"].keys()) == 64
    big = by["255_parts_mixed_from_0_1_and_the_stride"]
    assert set(big.part_rows) == {0, 1, 513} and big.part_rows[0] == 0 and big.part_rows[-1] == 0 and big.N <= 131325
    assert by["N257_empty_first_and_last"].part_rows == [0, 257, 0] and by["N513_empty_middle"].part_rows == [256, 0, 257]
    one = by["one_field/min_anchor_8"]
    keys = one.keys()
    base = (1, 500, 900, 0)
    assert {(0, 500, 900, 0), (1, 501, 900, 0), (1, 500, 901, 0), (1, 500, 900, 1), base} <= keys
    r = mref.merge(one.parts, one.names, 8)
    i = [k for k in range(len(r["tid"])) if (r["tid"][k], r["start"][k], r["end"][k], r["strand"][k]) == (1, 500, 900, ord("+"))][0]
    assert (r["read_count"][i], r["thick_start"][i], r["thick_end"][i]) == (0x10, 492, 908)       # the sum wrapped; min and max from different parts
    assert (r["left_ok"][i], r["right_ok"][i]) == (1, 1)
    j = [k for k in range(len(r["tid"])) if r["end"][k] == 700][0]
    assert r["strand"][j] == ord("*") and (r["thick_start"][j], r["thick_end"][j], r["left_ok"][j], r["right_ok"][j]) == (492, 708, 1, 1)
    names = one.names
    assert sorted(names) != names and [r["tid"][k] for k in range(len(r["tid"]))] != sorted(r["tid"])      # string order is not tid order
    assert len(set(mref.names_for(3))) == 2
