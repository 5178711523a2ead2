"""The de Bruijn adjacency of a table: kt_ctr_graph against the numpy restatement of tests/graph_ref.py over the oracle's
tables (which test_ctr_graph_cli_args.py pins, on the CPU, to worked answers and to a string-level brute force) - host and
device mode, sorted and not, every k that takes another path, count ranges, every table form, a nearly full small table
whose probes wrap, the shapes and argument errors of the call, shifted output views between guards, one larger case; and
`kmertools graph` end to end, byte for byte against the restated files.  Every comparison is exact."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "kmertools_amd", "bin", "kmertools")
GOLDEN = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, os.path.join(ROOT, "tests"))
import graph_ref as gr  # noqa: E402

U32 = 0xFFFFFFFF
RANGES = ((1, None), (2, None), (1, 1), (2, 3))
PRIME_K, PRIME_I, PRIME_C = 0xA5A5A5A5A5A5A5A5, 0x5A5A5A5A, 0x3C3C3C3C


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    return torch


@pytest.fixture(scope="module")
def ctx(torch_mod):
    from kmertools_amd import device
    c = device.Context(0, stream=torch_mod.cuda.current_stream().cuda_stream)
    yield c
    c.close()


def noisy_reads(seed, n, k, genome_len=12000):
    """reads sampled from a small genome with substitutions, runs of N, lower-case stretches, some shorter than k, some
    repeated"""
    rng = np.random.default_rng(seed)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    genome = acgt[rng.integers(0, 4, size=genome_len)]
    out = []
    for i in range(n):
        L = int(rng.integers(0, k)) if i % 25 == 0 else int(rng.integers(40, 200))
        a = int(rng.integers(0, len(genome) - L))
        s = genome[a:a + L].copy()
        err = rng.random(L) < 0.01
        s[err] = acgt[rng.integers(0, 4, size=int(err.sum()))]
        if L > 50 and rng.random() < 0.15:
            p = int(rng.integers(0, L - 6))
            s[p:p + int(rng.integers(1, 6))] = ord("N")
        if L > 50 and rng.random() < 0.15:
            p = int(rng.integers(0, L - 20))
            s[p:p + 20] = np.frombuffer(bytes(s[p:p + 20]).lower(), np.uint8)
        out.append(s.tobytes())
    return out + out[:40] * 2 + out[700:720] * 5


def sample(seed, k, n=1600):
    from kmertools_amd.device import to_csr
    return to_csr(noisy_reads(seed, n, k))


def sorted_table(keys, counts):
    order = np.argsort(keys)
    return np.asarray(keys, np.uint64)[order], np.asarray(counts, np.uint32)[order]


def counter_of(ctx, k, bases, offsets, n_keys):
    from kmertools_amd import device
    c = device.Counter(ctx, k, max(1 << 16, 2 * n_keys))
    c.add_reads_host(bases, offsets)
    return c


def pairs_counter(ctx, k, keys, counts, slots=1 << 16):
    from kmertools_amd import device
    c = device.Counter(ctx, k, slots)
    if len(keys):
        c.add_pairs_host(np.asarray(keys, np.uint64), np.asarray(counts, np.uint32))
    return c


def by_key(keys, *rest):
    order = np.argsort(keys, kind="stable")
    return (keys[order],) + tuple(r[order] for r in rest)


def graph_dev(torch, c, lo, hi, sort, room, with_counts=True, with_census=True):
    """device mode into arrays of room + 3 entries: nothing at or past n is written -> (keys, info, counts, census)"""
    keys = torch.full((room + 3,), -1, dtype=torch.int64, device="cuda")
    info = torch.full((room + 3,), -1, dtype=torch.int32, device="cuda")
    counts = torch.full((room + 3,), -1, dtype=torch.int32, device="cuda") if with_counts else None
    cen = torch.zeros(32, dtype=torch.int64, device="cuda") if with_census else None
    n = c.graph_device(keys, info, counts, room, lo, hi, sort=sort, census=cen)
    torch.cuda.synchronize()
    assert n <= room and (keys[n:] == -1).all() and (info[n:] == -1).all()
    if with_counts:
        assert (counts[n:] == -1).all()
    return (keys[:n].cpu().numpy().view(np.uint64), info[:n].cpu().numpy().view(np.uint32),
            counts[:n].cpu().numpy().view(np.uint32) if with_counts else None,
            cen.cpu().numpy().view(np.uint64) if with_census else None)


def check_all_modes(torch, c, tk, tc, k, ranges=RANGES, tag=None):
    """host and device mode, sorted and not, of counter c against the restatement of table (tk, tc) -> the wanted results"""
    wants = []
    for lo, hi in ranges:
        wk, wi, wc, wcen = gr.restate(tk, tc, k, lo, hi)
        wants.append((wk, wi, wc, wcen))
        t = (tag, k, lo, hi)
        assert (wi != 0).all() and (wi < 1 << 10).all()
        gk, gi, gc, gcen = c.graph(lo, hi, census=True)
        assert gk.dtype == np.uint64 and gi.dtype == np.uint32 and gc.dtype == np.uint32 and gcen.dtype == np.uint64
        assert np.array_equal(gk, wk) and np.array_equal(gi, wi) and np.array_equal(gc, wc), (t, "host sorted")
        assert np.array_equal(gcen, wcen), (t, "host census", gcen, wcen)
        gk, gi, gc = c.graph(lo, hi, sort=False)
        assert len(np.unique(gk)) == len(gk), (t, "host unsorted: a key twice")
        gk, gi, gc = by_key(gk, gi, gc)
        assert np.array_equal(gk, wk) and np.array_equal(gi, wi) and np.array_equal(gc, wc), (t, "host unsorted")
        gk, gi, gc, gcen = graph_dev(torch, c, lo, hi, True, len(wk) + 5)
        assert np.array_equal(gk, wk) and np.array_equal(gi, wi) and np.array_equal(gc, wc), (t, "device sorted")
        assert np.array_equal(gcen, wcen), (t, "device census")
        gk, gi, gc, gcen = graph_dev(torch, c, lo, hi, False, len(wk))  # (exactly the room it needs)
        assert len(np.unique(gk)) == len(gk), (t, "device unsorted: a key twice")
        gk, gi, gc = by_key(gk, gi, gc)
        assert np.array_equal(gk, wk) and np.array_equal(gi, wi) and np.array_equal(gc, wc), (t, "device unsorted")
        assert np.array_equal(gcen, wcen), (t, "device census, unsorted")
    return wants


def snapshot(ctr):
    return ctr.size(), ctr.export_host()


def same_snapshot(ctr, snap):
    n, (k, c) = snap
    n2, (k2, c2) = snapshot(ctr)
    return n == n2 and np.array_equal(k, k2) and np.array_equal(c, c2)


# ---- 1. worked answers ----------------------------------------------------------------------------------------------------

KNOWN = json.load(open(os.path.join(GOLDEN, "graph_known.json")))["cases"]


@pytest.mark.parametrize("case", KNOWN, ids=lambda c: "k%d_%s_min%d" % (c["k"], "+".join(c["reads"])[:24], c["min_count"]))
def test_graph_known_answers(torch_mod, ctx, case):
    k, lo = case["k"], case["min_count"]
    table = gr.count_strings(case["reads"], k)
    tk, tc = sorted_table([gr.key_of(s) for s in table], list(table.values()))
    want = case["nodes"]
    cen = list(case["census"]) + [0] * 25
    for cell, v in case["cells"].items():
        dl, dr = map(int, cell.split(","))
        cen[7 + 5 * dl + dr] = v
    c = pairs_counter(ctx, k, tk, tc)
    try:
        gk, gi, gc, gcen = c.graph(lo, None, census=True)
        assert [list(map(int, n)) for n in zip(gk, gc, gi)] == want
        assert gcen.tolist() == cen
        gk, gi, gc, gcen = graph_dev(torch_mod, c, lo, None, True, len(want) + 2)
        assert [list(map(int, n)) for n in zip(gk, gc, gi)] == want
        assert gcen.tolist() == cen
        check_all_modes(torch_mod, c, tk, tc, k, ((lo, None),))
    finally:
        c.close()


# ---- 2. every k that takes another path ------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", [1, 2, 4, 10, 15, 16, 17, 30, 31])
def test_graph_k_sweep(torch_mod, ctx, oracle, k):
    bases, offsets = sample(300 + k, k)
    tk, tc = sorted_table(*oracle.count_reads(bases, offsets, k))
    c = counter_of(ctx, k, bases, offsets, len(tk))
    try:
        snap = snapshot(c)
        wants = check_all_modes(torch_mod, c, tk, tc, k)
        assert same_snapshot(c, snap) and np.array_equal(snap[1][0], tk) and np.array_equal(snap[1][1], tc)
        cen = wants[0][3]
        assert cen[0] == len(tk) and cen[1] == int(tc.astype(np.uint64).sum())
        if k >= 10:  # the sample is a graph worth the name: unitig interiors, tips, branches, and ranges that differ
            assert cen[7 + 5 + 1] > 0 and cen[5] > 0 and cen[6] > 0
            assert len({len(w[0]) for w in wants}) == len(RANGES)
        if k % 2 == 0 and k <= 10:
            assert (gr.rc_np(tk, k) == tk).any()  # palindromic k-mers among the nodes
    finally:
        c.close()


# ---- 3. the complete graph -----------------------------------------------------------------------------------------------------

def test_graph_complete_k5(torch_mod, ctx):
    k = 5
    every = np.arange(4 ** k, dtype=np.uint64)
    tk = every[every <= gr.rc_np(every, k)]
    assert len(tk) == 512  # odd k: no palindromes
    tc = (np.arange(len(tk)) % 7 + 1).astype(np.uint32)
    c = pairs_counter(ctx, k, tk, tc)
    try:
        gk, gi, gc, cen = c.graph(census=True)
        assert np.array_equal(gk, tk) and np.array_equal(gc, tc) and (gi == 0x3FF).all()
        want = np.zeros(32, np.uint64)
        want[0], want[1], want[2], want[3], want[6], want[7 + 5 * 4 + 4] = 512, int(tc.sum()), 8 * 512, 2 * 512, 512, 512
        assert np.array_equal(cen, want)
        check_all_modes(torch_mod, c, tk, tc, k)
    finally:
        c.close()


# ---- 4. count ranges -----------------------------------------------------------------------------------------------------------

def test_graph_count_ranges(torch_mod, ctx, oracle):
    k = 19
    bases, offsets = sample(419, k)
    tk, tc = sorted_table(*oracle.count_reads(bases, offsets, k))
    c = counter_of(ctx, k, bases, offsets, len(tk))
    try:
        wants = check_all_modes(torch_mod, c, tk, tc, k)
        plain = dict(zip(wants[0][0].tolist(), wants[0][1].tolist()))
        for (lo, hi), (wk, wi, wc, _) in zip(RANGES[1:], wants[1:]):
            top = U32 if hi is None else hi
            # walked entries outside the range are not emitted ...
            assert 0 < len(wk) < len(tk) and (wc >= lo).all() and (wc <= top).all()
            assert len(wk) == int(((tc >= lo) & (tc <= top)).sum())
            # ... and neighbours outside it are not counted: some node lost a neighbour that the plain graph gives it
            lost = [key for key, i in zip(wk.tolist(), wi.tolist()) if (plain[key] & 0xFF) & ~(i & 0xFF)]
            assert lost, (lo, hi)
            assert all((i & 0xFF) & ~(plain[key] & 0xFF) == 0 for key, i in zip(wk.tolist(), wi.tolist()))
        # a range that holds nothing
        gk, gi, gc, cen = c.graph(int(tc.max()) + 1, None, census=True)
        assert len(gk) == 0 and len(gi) == 0 and len(gc) == 0 and not cen.any()
    finally:
        c.close()


# ---- 5. every table form before the call ------------------------------------------------------------------------------------

FORMS = ("probing", "add_pairs", "bulk", "export target")


def table_in_form(torch, ctx, form, k, bases, offsets, tk, tc, cap, monkeypatch):
    from kmertools_amd import device
    monkeypatch.delenv("KT_BULK", raising=False)
    monkeypatch.delenv("KT_BULK_MIN_BASES", raising=False)
    if form in ("bulk", "export target"):
        monkeypatch.setenv("KT_BULK", "1")
        monkeypatch.setenv("KT_BULK_MIN_BASES", "0")
    c = device.Counter(ctx, k, cap)
    target = None
    if form == "add_pairs":
        c.add_pairs_host(tk, tc)
    elif form == "export target":
        m = len(tk) + 9
        xk = torch.full((m,), 0x1D1D1D1D1D1D1D1D, dtype=torch.int64, device="cuda")
        xc = torch.full((m,), 0x2E2E2E2E, dtype=torch.int32, device="cuda")
        c.export_target(xk, xc, m)
        c.add_reads(torch.from_numpy(bases).cuda(), torch.from_numpy(offsets.astype(np.int64)).cuda(), len(offsets) - 1)
        torch.cuda.synchronize()
        target = (xk, xc)
    else:
        c.add_reads_host(bases, offsets)
    monkeypatch.delenv("KT_BULK", raising=False)
    monkeypatch.delenv("KT_BULK_MIN_BASES", raising=False)
    return c, target


@pytest.mark.parametrize("size", ["one range", "many ranges"])
def test_graph_every_table_form(torch_mod, ctx, oracle, monkeypatch, size):
    torch = torch_mod
    k = 13
    if size == "one range":  # a table below 8192 slots is a single range
        bases, offsets = sample(513, k, n=24)
        cap = 4096
    else:
        bases, offsets = sample(2013, k)
        cap = 1 << 17
    tk, tc = sorted_table(*oracle.count_reads(bases, offsets, k))
    assert (len(tk) < 3000) if size == "one range" else (len(tk) > 10000)
    lo, hi = 1, 6
    wk, wi, wc, wcen = gr.restate(tk, tc, k, lo, hi)
    assert 0 < len(wk) < len(tk)
    for form in FORMS:
        for mode in ("host", "device"):
            c, target = table_in_form(torch, ctx, form, k, bases, offsets, tk, tc, cap, monkeypatch)
            try:
                assert c.capacity() < 8192 if size == "one range" else c.capacity() >= 4 * 8192
                before = tuple(t.clone() for t in target) if target else None
                if mode == "host":
                    gk, gi, gc, gcen = c.graph(lo, hi, census=True)
                else:
                    gk, gi, gc, gcen = graph_dev(torch, c, lo, hi, False, len(wk))
                    gk, gi, gc = by_key(gk, gi, gc)
                assert np.array_equal(gk, wk) and np.array_equal(gi, wi) and np.array_equal(gc, wc), (form, mode)
                assert np.array_equal(gcen, wcen), (form, mode)
                n, (ek, ec) = snapshot(c)  # the table's content did not change
                assert n == len(tk) and np.array_equal(ek, tk) and np.array_equal(ec, tc), (form, mode)
                if target:
                    torch.cuda.synchronize()
                    assert torch.equal(before[0], target[0]) and torch.equal(before[1], target[1]), (form, mode)
                    # (a table of one range is below the bulk build's sizes: it was counted by probing and its target left
                    # alone; the larger one's entries were in the target before the call)
                    written = bool((target[0][0] != 0x1D1D1D1D1D1D1D1D).item())
                    assert written == (size == "many ranges"), (form, mode)
                    if written:
                        xk = target[0][:n].cpu().numpy().view(np.uint64)
                        assert np.array_equal(np.sort(xk), tk) and bool((target[0][n:] == 0x1D1D1D1D1D1D1D1D).all())
            finally:
                c.close()


# ---- 6. a small table near load 0.7: probes walk past the home slot and wrap at the range end ---------------------------------

def home_slot(key, cap):
    """kttab::probe_of for a table of one range (cap a power of two below 8192) and k > 16: the top bits of ktd::khash"""
    h = (int(key) * 0x9E3779B97F4A7C15) & 0xFFFFFFFFFFFFFFFF
    h ^= h >> 32
    return h >> (64 - cap.bit_length() + 1)


def test_graph_small_table_near_full_probes_wrap(torch_mod, ctx, oracle):
    from kmertools_amd.device import to_csr
    k, cap = 21, 1024
    rng = np.random.default_rng(6024)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    genome = acgt[rng.integers(0, 4, size=640)]
    reads = []
    for _ in range(60):
        a = int(rng.integers(0, len(genome) - 60))
        s = genome[a:a + int(rng.integers(30, 60))].copy()
        if rng.random() < 0.3:
            s[int(rng.integers(0, len(s)))] = acgt[int(rng.integers(0, 4))]
        reads.append(s.tobytes())
    reads.append(genome.tobytes())
    bases, offsets = to_csr(reads)
    tk, tc = sorted_table(*oracle.count_reads(bases, offsets, k))
    assert 0.66 * cap < len(tk) < 0.8 * cap, len(tk)
    # the shape, from the hash: linear probing fills the same slots in whatever order the keys arrive, so placing them in
    # key order tells how many keys do not sit in their home slot and how many probe sequences pass the end of the range
    taken, displaced, wrapped = set(), 0, 0
    for key in tk:
        h = home_slot(key, cap)
        s = h
        while s in taken:
            s = (s + 1) % cap
            wrapped += s == 0
        taken.add(s)
        displaced += s != h
    assert displaced > 50 and wrapped > 0, (displaced, wrapped)
    c = pairs_counter(ctx, k, tk, tc, slots=cap)
    try:
        assert c.capacity() == cap and c.size() == len(tk)
        wants = check_all_modes(torch_mod, c, tk, tc, k, ((1, None), (2, None)))
        assert wants[0][3][6] > 0 and wants[0][3][12] > 0
    finally:
        c.close()


# ---- 7. shapes -----------------------------------------------------------------------------------------------------------------

def raw_graph(L, t, lo=1, hi=U32, keys=None, info=None, counts=None, max_out=0, n=None, census=None, mem=0, sort=1):
    ptr = lambda x: None if x is None else x.ctypes.data
    return L.kt_ctr_graph(t, lo, hi, ptr(keys), ptr(info), ptr(counts), max_out, None if n is None else C.byref(n),
                          ptr(census), mem, sort)


def test_graph_shapes(torch_mod, ctx, oracle):
    torch = torch_mod
    from kmertools_amd import device
    from kmertools_amd._lib import KT_ERR_ARG, lib
    L = lib()
    k = 23
    made = []
    try:
        # no entry, one entry
        empty = device.Counter(ctx, k, 1 << 16)
        made.append(empty)
        for sort in (True, False):
            gk, gi, gc, cen = empty.graph(census=True, sort=sort)
            assert len(gk) == 0 and len(gi) == 0 and len(gc) == 0 and not cen.any()
            gk, gi, gc, cen = graph_dev(torch, empty, 1, None, sort, 4)
            assert len(gk) == 0 and not cen.any()
        n = C.c_uint64(99)
        cen = np.full(32, 7, np.uint64)
        assert raw_graph(L, empty._h, n=n, census=cen) == 0 and n.value == 0 and (cen == 7).all()
        assert empty.size() == 0
        one = pairs_counter(ctx, k, [gr.key_of("ACGTTGCATGCAGGATCCATTAG")], [3])
        made.append(one)
        tk1, tc1 = np.array([gr.key_of("ACGTTGCATGCAGGATCCATTAG")], np.uint64), np.array([3], np.uint32)
        check_all_modes(torch, one, tk1, tc1, k, ((1, None), (3, 3), (4, None)))
        assert one.graph()[1].tolist() == [0x300]
        # an entry count that is no multiple of the workgroup tile (nor of anything else)
        bases, offsets = sample(723, k)
        tk, tc = sorted_table(*oracle.count_reads(bases, offsets, k))
        assert len(tk) % 256 and len(tk) > 20000
        c = counter_of(ctx, k, bases, offsets, len(tk))
        made.append(c)
        wk, wi, wc, wcen = gr.restate(tk, tc, k)
        w2 = gr.restate(tk, tc, k, 2, 9)
        want = len(wk)
        # max_out == 0: only the number and the census, no arrays
        for mem in (0, 1):
            for sort in (0, 1):
                n = C.c_uint64(99)
                if mem == 0:
                    cen = np.zeros(32, np.uint64)
                    assert raw_graph(L, c._h, n=n, census=cen, sort=sort) == 0
                else:
                    dcen = torch.zeros(32, dtype=torch.int64, device="cuda")
                    assert L.kt_ctr_graph(c._h, 1, U32, None, None, None, 0, C.byref(n), dcen.data_ptr(), 1, sort) == 0
                    torch.cuda.synchronize()
                    cen = dcen.cpu().numpy().view(np.uint64)
                assert n.value == want and np.array_equal(cen, wcen), (mem, sort)
        n = C.c_uint64(99)
        assert raw_graph(L, c._h, lo=2, hi=9, n=n) == 0 and n.value == len(w2[0])  # census = NULL too
        # the census is ADDED: twice doubles, and what was there stays
        cen = np.arange(32, dtype=np.uint64)
        for _ in range(2):
            assert raw_graph(L, c._h, n=n, census=cen) == 0
        assert np.array_equal(cen, np.arange(32, dtype=np.uint64) + 2 * wcen)
        dcen = torch.arange(32, dtype=torch.int64, device="cuda")
        for _ in range(2):
            assert c.graph_device(None, None, None, 0, census=dcen) == want
        torch.cuda.synchronize()
        assert np.array_equal(dcen.cpu().numpy().view(np.uint64), np.arange(32, dtype=np.uint64) + 2 * wcen)
        # counts = NULL, census = NULL: keys and info alone
        keys, info = np.full(want + 2, PRIME_K, np.uint64), np.full(want + 2, PRIME_I, np.uint32)
        assert raw_graph(L, c._h, keys=keys, info=info, max_out=want, n=n) == 0 and n.value == want
        assert np.array_equal(keys[:want], wk) and np.array_equal(info[:want], wi)
        assert (keys[want:] == PRIME_K).all() and (info[want:] == PRIME_I).all()
        gk, gi, gc, gcen = graph_dev(torch, c, 1, None, True, want, with_counts=False, with_census=False)
        assert np.array_equal(gk, wk) and np.array_equal(gi, wi) and gc is None and gcen is None
        # one short: KT_ERR_ARG, the number exact, nothing at or past max_out, the census added
        for mem in (0, 1):
            for sort in (0, 1):
                n = C.c_uint64(0)
                if mem == 0:
                    keys, info = np.full(want + 2, PRIME_K, np.uint64), np.full(want + 2, PRIME_I, np.uint32)
                    counts, cen = np.full(want + 2, PRIME_C, np.uint32), np.zeros(32, np.uint64)
                    rc = raw_graph(L, c._h, keys=keys, info=info, counts=counts, max_out=want - 1, n=n, census=cen, sort=sort)
                    tails = keys[want - 1:], info[want - 1:], counts[want - 1:]
                else:
                    dk = torch.from_numpy(np.full(want + 2, PRIME_K, np.uint64).view(np.int64)).cuda()
                    di = torch.from_numpy(np.full(want + 2, PRIME_I, np.uint32).view(np.int32)).cuda()
                    dc = torch.from_numpy(np.full(want + 2, PRIME_C, np.uint32).view(np.int32)).cuda()
                    dcen = torch.zeros(32, dtype=torch.int64, device="cuda")
                    rc = L.kt_ctr_graph(c._h, 1, U32, dk.data_ptr(), di.data_ptr(), dc.data_ptr(), want - 1, C.byref(n),
                                        dcen.data_ptr(), 1, sort)
                    torch.cuda.synchronize()
                    tails = (dk.cpu().numpy().view(np.uint64)[want - 1:], di.cpu().numpy().view(np.uint32)[want - 1:],
                             dc.cpu().numpy().view(np.uint32)[want - 1:])
                    cen = dcen.cpu().numpy().view(np.uint64)
                assert rc == KT_ERR_ARG and L.kt_last_error() and n.value == want, (mem, sort)
                assert (tails[0] == PRIME_K).all() and (tails[1] == PRIME_I).all() and (tails[2] == PRIME_C).all(), (mem, sort)
                assert np.array_equal(cen, wcen), (mem, sort)
        with pytest.raises(device._lib.KmertoolsError):
            c.graph_device(*(torch.zeros(4, dtype=d, device="cuda") for d in (torch.int64, torch.int32, torch.int32)), 4)
    finally:
        for t in reversed(made):
            t.close()


# ---- 8. views and fences ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shift", [1, 3, 5])
def test_graph_into_shifted_views_between_guards(torch_mod, ctx, oracle, shift):
    torch = torch_mod
    k = 27
    bases, offsets = sample(7000 + shift, k, n=2400)
    tk, tc = sorted_table(*oracle.count_reads(bases, offsets, k))
    c = counter_of(ctx, k, bases, offsets, len(tk))
    guard = 4096
    KG, IG, CG, EG = 0x7E7E7E7E7E7E7E7E, 0x6D6D6D6D, 0x5C5C5C5C, 0x4B4B4B4B4B4B4B4B
    try:
        for lo, hi in ((1, None), (2, None)):
            wk, wi, wc, wcen = gr.restate(tk, tc, k, lo, hi)
            n = len(wk)
            assert n > 4096  # more than one wave tile of the sort
            for sort in (True, False):
                bk = torch.full((guard + shift + n + guard,), KG, dtype=torch.int64, device="cuda")
                bi = torch.full((guard + shift + n + guard,), IG, dtype=torch.int32, device="cuda")
                bc = torch.full((guard + shift + n + guard,), CG, dtype=torch.int32, device="cuda")
                be = torch.full((guard + shift + 32 + guard,), EG, dtype=torch.int64, device="cuda")
                sl = slice(guard + shift, guard + shift + n)
                vk, vi, vc, ve = bk[sl], bi[sl], bc[sl], be[guard + shift:guard + shift + 32]
                assert vk.data_ptr() == bk.data_ptr() + 8 * (guard + shift) and vi.data_ptr() == bi.data_ptr() + 4 * (guard + shift)
                ve.zero_()
                got = c.graph_device(vk, vi, vc, n, lo, hi, sort=sort, census=ve)
                torch.cuda.synchronize()
                assert got == n
                hk, hi_, hc, he = bk.cpu().numpy(), bi.cpu().numpy(), bc.cpu().numpy(), be.cpu().numpy()
                for h, g in ((hk, KG), (hi_, IG), (hc, CG)):
                    assert (h[:guard + shift] == g).all() and (h[guard + shift + n:] == g).all(), (lo, sort)
                assert (he[:guard + shift] == EG).all() and (he[guard + shift + 32:] == EG).all(), (lo, sort)
                assert np.array_equal(he[guard + shift:guard + shift + 32].view(np.uint64), wcen), (lo, sort)
                gk, gi, gc = hk[sl].view(np.uint64), hi_[sl].view(np.uint32), hc[sl].view(np.uint32)
                if not sort:
                    gk, gi, gc = by_key(gk, gi, gc)
                assert np.array_equal(gk, wk) and np.array_equal(gi, wi) and np.array_equal(gc, wc), (lo, sort)
    finally:
        c.close()


# ---- 9. argument errors -----------------------------------------------------------------------------------------------------------

def test_graph_errors(torch_mod, ctx, oracle):
    torch = torch_mod
    from kmertools_amd import device
    from kmertools_amd._lib import KT_ERR_ARG, KT_ERR_FULL, lib
    L = lib()
    k = 21
    bases, offsets = sample(6000, k)
    made = []  # closed whatever happens: a table must not outlive its context

    def keep(c):
        made.append(c)
        return c

    try:
        a = keep(counter_of(ctx, k, bases, offsets, 1 << 17))
        room = a.size()
        keys, info = np.full(room, PRIME_K, np.uint64), np.full(room, PRIME_I, np.uint32)
        counts, cen = np.full(room, PRIME_C, np.uint32), np.full(32, 11, np.uint64)
        n = C.c_uint64(0)

        def call(t=a._h, **kw):
            kw.setdefault("keys", keys)
            kw.setdefault("info", info)
            kw.setdefault("counts", counts)
            kw.setdefault("census", cen)
            kw.setdefault("max_out", room)
            kw.setdefault("n", n)
            return raw_graph(L, t, **kw)

        for kw in (dict(t=None), dict(n=None), dict(lo=0), dict(lo=0, hi=0), dict(lo=3, hi=2), dict(lo=U32, hi=U32 - 1),
                   dict(mem=2), dict(mem=-1), dict(keys=None), dict(info=None), dict(keys=None, info=None)):
            assert call(**kw) == KT_ERR_ARG, kw
            assert L.kt_last_error(), kw
        # one shard of a sharded table (allocated as rank 0 of 2, never connected)
        sh = keep(device.Sharded(ctx, k, 1 << 16, 1 << 16, 2, 0, ("host", lambda s, r, n: 1), connect=False))
        assert call(t=sh.table._h) == KT_ERR_ARG and b"shard" in L.kt_last_error()
        # an overflowed table (far more distinct keys than slots)
        full = keep(device.Counter(ctx, k, 1024))
        full.add_pairs_host(np.arange(1, 5000, dtype=np.uint64) * 7919, np.ones(4999, np.uint32))
        assert call(t=full._h) == KT_ERR_FULL and L.kt_last_error()
        assert call(t=full._h, keys=None, info=None, counts=None, max_out=0) == KT_ERR_FULL
        # no refused call wrote anything
        assert (keys == PRIME_K).all() and (info == PRIME_I).all() and (counts == PRIME_C).all() and (cen == 11).all()
        # device outputs are left alone as well
        dk = torch.from_numpy(keys.view(np.int64)).cuda()
        di = torch.from_numpy(info.view(np.int32)).cuda()
        dc = torch.from_numpy(counts.view(np.int32)).cuda()
        de = torch.full((32,), 11, dtype=torch.int64, device="cuda")
        for t, lo, hi, want in ((a._h, 0, U32, KT_ERR_ARG), (a._h, 9, 8, KT_ERR_ARG), (sh.table._h, 1, U32, KT_ERR_ARG),
                                (full._h, 1, U32, KT_ERR_FULL)):
            rc = L.kt_ctr_graph(t, lo, hi, dk.data_ptr(), di.data_ptr(), dc.data_ptr(), room, C.byref(n), de.data_ptr(), 1, 1)
            assert rc == want and L.kt_last_error(), (lo, hi)
        torch.cuda.synchronize()
        assert (dk.cpu().numpy().view(np.uint64) == PRIME_K).all() and (di.cpu().numpy().view(np.uint32) == PRIME_I).all()
        assert (dc.cpu().numpy().view(np.uint32) == PRIME_C).all() and bool((de == 11).all())
        assert call() == 0 and n.value == room  # the context is still good
    finally:
        for c in reversed(made):
            c.close()


# ---- 10. one larger case ------------------------------------------------------------------------------------------------------------

def test_graph_full_size_k31(torch_mod, ctx, oracle):
    """24 000 reads of 150 bases sampled from a random genome of 800 k bases with 0.5 % substitutions, k = 31: about a
    million nodes - some thousand workgroup tiles over some hundred ranges - against the restatement of the oracle's table
    of the same reads, in device mode, sorted and not; and the solid half of it (min_count = 2) in host mode."""
    torch = torch_mod
    k, L, G, n = 31, 150, 800_000, 24_000
    rng = np.random.default_rng(31)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    genome = acgt[rng.integers(0, 4, size=G)]
    reads = genome[rng.integers(0, G - L, size=n)[:, None] + np.arange(L)[None, :]]
    err = rng.random(reads.shape) < 0.005
    reads[err] = acgt[rng.integers(0, 4, size=int(err.sum()))]
    bases, offsets = np.ascontiguousarray(reads.reshape(-1)), np.arange(n + 1, dtype=np.uint64) * np.uint64(L)
    tk, tc = sorted_table(*oracle.count_reads(bases, offsets, k, threads=16))
    assert 900_000 < len(tk) < 2_000_000
    c = counter_of(ctx, k, bases, offsets, len(tk))
    try:
        assert c.capacity() >= 128 * 8192
        wk, wi, wc, wcen = gr.restate(tk, tc, k)
        print("full size: %d nodes, census %s" % (len(wk), wcen[:7].tolist()), flush=True)
        assert wcen[5] > 1000 and wcen[6] > 1000 and wcen[7 + 6] > 800_000
        gk, gi, gc, gcen = graph_dev(torch, c, 1, None, True, len(wk))
        assert np.array_equal(gcen, wcen)
        assert np.array_equal(gk, wk) and np.array_equal(gi, wi) and np.array_equal(gc, wc)
        gk, gi, gc, gcen = graph_dev(torch, c, 1, None, False, len(wk) + 1000)
        gk, gi, gc = by_key(gk, gi, gc)
        assert np.array_equal(gk, wk) and np.array_equal(gi, wi) and np.array_equal(gc, wc) and np.array_equal(gcen, wcen)
        wk, wi, wc, wcen = gr.restate(tk, tc, k, 2, None)
        assert 400_000 < len(wk) < len(tk)
        gk, gi, gc, gcen = c.graph(2, None, census=True)
        assert np.array_equal(gk, wk) and np.array_equal(gi, wi) and np.array_equal(gc, wc) and np.array_equal(gcen, wcen)
        assert c.size() == len(tk)
    finally:
        c.close()


# ---- 11. the CLI end to end -----------------------------------------------------------------------------------------------------------

def run(*args, env=None):
    return subprocess.run([CLI, *map(str, args)], capture_output=True, timeout=600, env=env)


@pytest.fixture(scope="module")
def cli_bin():
    if not os.path.exists(CLI):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "kmertools_amd", "csrc"), "-j4"], stdout=subprocess.DEVNULL)
    return CLI


def table_of_file(oracle, path, k):
    return sorted_table(*oracle.count_reads(*oracle.to_csr([s for _, s in oracle.read_records(path)]), k))


@pytest.mark.parametrize("k", [15, 31])
def test_graph_cli_end_to_end(cli_bin, oracle, tmp_path, k):
    fa = tmp_path / "reads.fasta"
    fa.write_bytes(b"".join(b">rec%d lane=%d  sample x\n%s\n" % (i, i % 5, s) for i, s in enumerate(noisy_reads(80 + k, 3000, k))))
    tk, tc = table_of_file(oracle, str(fa), k)
    env = dict(os.environ, KT_CLI_TIMING="1")
    cases = (("plain", [], 1, None, False), ("acgt", ["--acgt"], 1, None, True), ("min2", ["--min-count", 2], 2, None, False),
             ("min2max5acgt", ["--min-count", 2, "--max-count", 5, "--acgt"], 2, 5, True))
    for name, flags, lo, hi, acgt in cases:
        nodes, stats, n = gr.want_files(tk, tc, k, lo, hi, acgt)
        assert n > 1000
        d = tmp_path / name
        r = run("graph", "-i", fa, "-o", d, "-k", k, *flags, env=env)
        assert r.returncode == 0, r.stderr
        assert (d / "graph.nodes").read_bytes() == nodes, (k, name)
        assert (d / "graph.stats").read_bytes() == stats, (k, name)
        assert sorted(os.listdir(d)) == ["graph.nodes", "graph.stats"]
        d2 = tmp_path / (name + "_stats_only")
        r = run("graph", "-i", fa, "-o", d2, "-k", k, *flags, "--stats-only", env=env)
        assert r.returncode == 0, r.stderr
        assert os.listdir(d2) == ["graph.stats"] and (d2 / "graph.stats").read_bytes() == stats, (k, name)
    # the same in batches of 7 reads, and from the dense bulk build
    nodes, stats, _ = gr.want_files(tk, tc, k)
    for name, extra in (("batched", dict(KT_CLI_BATCH_READS="7")), ("dense", dict(KT_BULK_MIN_BASES="0"))):
        d = tmp_path / name
        r = run("graph", "-i", fa, "-o", d, "-k", k, env=dict(env, **extra))
        assert r.returncode == 0, r.stderr
        assert (d / "graph.nodes").read_bytes() == nodes and (d / "graph.stats").read_bytes() == stats, (k, name)
    # a table that would take passes: refused before any file exists
    d = tmp_path / "passes"
    r = run("graph", "-i", fa, "-o", d, "-k", k, "--min-count", 2, env=dict(env, KT_CTR_MAX_SLOTS="65536"))
    assert r.returncode != 0 and r.returncode != 2
    msg = r.stderr.decode()
    assert msg.startswith("Error: ") and "graph needs the whole table on the device" in msg and "--min-count is no remedy" in msg
    assert not d.exists() or os.listdir(d) == []


def test_graph_cli_golden_inputs(cli_bin, oracle, tmp_path):
    for i, (name, k, acgt) in enumerate((("reads.fq", 15, False), ("reads.fa", 31, True), ("reads.fq.gz", 21, False))):
        path = os.path.join(GOLDEN, name)
        tk, tc = table_of_file(oracle, path, k)
        nodes, stats, n = gr.want_files(tk, tc, k, acgt=acgt)
        assert n > 0
        d = tmp_path / ("out_%d" % i)
        r = run("graph", "-i", path, "-o", d, "-k", k, *(["--acgt"] if acgt else []))
        assert r.returncode == 0, r.stderr
        assert (d / "graph.nodes").read_bytes() == nodes and (d / "graph.stats").read_bytes() == stats, name
