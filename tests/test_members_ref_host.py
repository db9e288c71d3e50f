"""tests/members_ref.py on the CPU: on well-formed files the restatement of BGZF member discovery is the plain BSIZE walk (bamio.bgzf_members) and
the product's host scan (scan_members_parallel through tests/hostemu), and every file the GPU tests use meets the condition it was built for."""
import ctypes
import os

import numpy as np
import pytest

import bamio
import members_ref as mr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def emu(built):
    lib = ctypes.CDLL(os.path.join(ROOT, "tests", "hostemu", "libhostemu.so"))
    lib.emu_scan_members.restype = ctypes.c_long
    lib.emu_scan_members.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_int, ctypes.POINTER(ctypes.c_uint64), ctypes.c_size_t,
                                     ctypes.POINTER(ctypes.c_uint64)]
    return lib


def _host_scan(emu, data, threads):
    cap = 80000
    arr = (ctypes.c_uint64 * (4 * cap))()
    total = ctypes.c_uint64(0)
    n = emu.emu_scan_members(data, len(data), threads, arr, cap, ctypes.byref(total))
    return n, np.ctypeslib.as_array(arr)[:4 * max(n, 0)].reshape(-1, 4).copy(), total.value


def _well_formed():
    yield "plain_1", mr.plain_run(1)
    yield "plain_2049", mr.plain_run(2049, np.full(2049, 65536)) + mr.EOF_MEMBER
    yield "decoys_257", mr.decoy_run(257) + mr.EOF_MEMBER
    yield "decoys_landing", mr.decoy_run(40, land_on_next={10}) + mr.EOF_MEMBER
    yield "two_in_one_thread", mr.two_in_one_thread()[0]
    yield "small_file", mr.small_file()
    yield "big", mr.plain_run(mr.BIG_N, np.full(mr.BIG_N, 65536))


@pytest.mark.parametrize("name,data", list(_well_formed()), ids=[n for n, _ in _well_formed()])
def test_restatement_equals_the_bsize_walk_and_the_host_scan(emu, name, data):
    got = mr.discover(data)
    want, up = [], 0
    for off, payload, isize in bamio.bgzf_members(data):
        clen = len(payload) + 8
        if off + 18 + clen + 8 > len(data):
            clen = len(data) - 8 - (off + 18)                # (the last member: the decoder's look-ahead stays inside the file's bytes + 8)
        want.append((off + 18, up, clen, isize))
        up += isize
    assert got["members"] == want and got["total"] == up
    for threads in (1, 4):
        n, arr, total = _host_scan(emu, data, threads)
        assert n == len(want), (name, threads, n)
        assert np.array_equal(arr, mr.members_array(got["members"])) and total == got["total"]


def test_tile_files_take_every_residue():
    a = mr.discover(mr.plain_run(4200))
    assert len(a["members"]) == 4200 == len(a["candidates"])
    assert {o % 4096 for o in a["candidates"]} == set(range(4096))
    assert {o % 16 for o in a["candidates"]} == set(range(16))
    b = mr.discover(mr.decoy_run(4200))
    starts = {m[0] - 18 for m in b["members"]}
    decoys = [o for o in b["candidates"] if o not in starts]
    assert len(starts) == 4200 == len(decoys)
    assert {o % 4096 for o in starts} == set(range(4096)) and {o % 4096 for o in decoys} == set(range(4096))
    # every split of the 16 header bytes across a tile edge: a header starts 1 .. 15 bytes in front of one
    assert {4096 - o % 4096 for o in b["candidates"] if o % 4096 > 4080} == set(range(1, 16))


def test_two_in_one_thread_condition():
    data, ks = mr.two_in_one_thread()
    r = mr.discover(data)
    starts = {m[0] - 18 for m in r["members"]}
    assert sorted(k % 16 for k in ks) == list(range(16))
    for k in ks:
        assert k in r["candidates"] and k + 6 in r["candidates"] and k not in starts and k + 6 not in starts
    assert len(r["members"]) == 17


def test_small_file_cuts_cover_a_last_header_of_17_and_18_bytes():
    data = mr.small_file()
    n = len(data)
    assert n > 64 + 34
    last = mr.candidates(data)[-1]
    assert n - 64 <= last + 17 and last + 18 <= n
    assert last not in mr.candidates(data[:last + 17]) and last in mr.candidates(data[:last + 18])
    # the list ends with a candidate that runs past the file at most cuts, and is one member shorter each time a header falls off
    sizes = {len(mr.discover(data[:cut])["members"]) for cut in range(n - 64, n + 1)}
    assert len(sizes) >= 3


@pytest.mark.parametrize("n", mr.CHAIN_LENGTHS)
def test_chain_files_list_their_last_member(n):
    data = mr.decoy_run(n)
    r = mr.discover(data)
    assert len(r["candidates"]) == 2 * n and len(r["members"]) == n
    assert r["members"][-1][0] == 51 * (n - 1) + 18


def test_broken_and_foreign_links():
    n, mid = 40, 20
    for delta in (-1, 1):
        r = mr.discover(mr.decoy_run(n, blen_delta={mid: delta}))
        assert len(r["members"]) == mid + 1                                    # the member with the wrong BSIZE is the last one reached
        r2 = mr.discover(mr.decoy_run(n, blen_delta={mid: delta}), root2=51 * (mid + 1))
        assert len(r2["members"]) == n and [m[0] - 18 for m in r2["members"]] == [51 * k for k in range(n)]
    data = mr.decoy_run(n, land_on_next={10})
    d10 = 51 * 10 + mr.DATA_AT
    assert d10 + mr.u16(data, d10 + 16) + 1 == 51 * 11                          # the decoy's link lands on a real member
    r = mr.discover(data)
    assert len(r["members"]) == n and d10 + 18 not in [m[0] for m in r["members"]]
    r = mr.discover(data, root2=d10)
    assert len(r["members"]) == n + 1 and r["members"][11][0] == d10 + 18        # listed, between members 10 and 11
    for root2 in (0, 7, 51 * 5):                                                # offset 0, no candidate, a member already reached
        assert mr.discover(data, root2=root2)["members"] == mr.discover(data)["members"]


def test_upos_files():
    for n in mr.UPOS_LENGTHS:
        f = mr.drawn_footers(n, n)
        assert set(mr.FOOTER_KINDS) <= set(int(v) for v in f)
        r = mr.discover(mr.plain_run(n, f))
        assert len(r["members"]) == n
        assert [m[3] for m in r["members"]] == [0xfffffffe if v == 0xffffffff else int(v) for v in f]
        assert r["total"] == sum(int(v) for v in f if v <= 65536)
    data = mr.plain_run(mr.BIG_N, np.full(mr.BIG_N, 65536))
    r = mr.discover(data)
    assert len(data) == 33 * mr.BIG_N and r["total"] == mr.BIG_TOTAL > 1 << 32 and r["members"][-1][1] > 1 << 32
    t = mr.drawn_true_sizes(mr.BIG_N, 5)
    r = mr.discover(data, true_sizes=t)
    assert r["total"] == sum(int(v) for v in t if v <= 65536) and [m[3] for m in r["members"]] == [int(v) for v in t]


def test_query_and_stop():
    n = 64
    f = np.full(n, 100)
    f[[10, 40]] = [0, 70000]
    data = mr.decoy_run(n, f)
    hit = lambda k: 51 * k
    r = mr.discover(data, q=(hit(0), hit(n - 1), hit(31)))
    assert r["q_index"] == [0, n - 1, 31] and r["q_upos"] == [0, 100 * (n - 3), 100 * 30] and r["stop"] == 10
    r = mr.discover(data, q=(hit(31) + 1, hit(31) + mr.DATA_AT, len(data)))
    assert r["q_index"] == [n, n, n] and r["q_upos"] == [mr.NONE] * 3 and r["stop"] == 0xffffffff
    assert mr.discover(data, q=(mr.NONE - 64, 0, 0))["q_index"][0] == n
    assert [mr.discover(data, q=(hit(k), 0, 0))["stop"] for k in (10, 11, 40, 41)] == [10, 40, 40, 0xffffffff]
