"""The heterozygous k-mer pairs of a table: kt_ctr_hetmers against the numpy restatement of tests/hetmer_ref.py (which
test_ctr_hetmers_cli_args.py pins, on the CPU, to worked answers and to a string-level brute force) - random subsets of all
canonical k-mers for k = 3..6, the worked answers, two-haplotype reads at every k that takes another path, hand-placed
pairs at the ends and the middle of k = 31, the largest count and the matrix clamps, every table form, a nearly full small
table whose probes wrap, host and device mode, sorted and not, both position modes, the shapes and argument errors of the
call, shifted output views between guards, one larger case; and `kmertools hetmers` end to end, byte for byte against the
restated files.  Every comparison is exact."""
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
import hetmer_ref as hr  # noqa: E402

U32 = 0xFFFFFFFF
RANGES = ((1, None), (2, None), (1, 1), (2, 3))
PRIME_K, PRIME_C, PRIME_M = 0xA5A5A5A5A5A5A5A5, 0x3C3C3C3C, 0x4B4B4B4B4B4B4B4B
ROWS, COLS = 4, 6  # a matrix small enough that the counts 1..5 of the small tables reach both clamps


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


def diploid_reads(seed, n, genome_len=12000, err=0.004):
    """reads sampled from the two haplotypes of a random genome: an isolated SNP every 97 bases, and at every fifth of them
    two more SNPs 3 and 9 bases on - closer than any k here, so that their k-mers have several partners - with substitution
    errors and a few runs of N"""
    rng = np.random.default_rng(seed)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    h1 = rng.integers(0, 4, size=genome_len)
    h2 = h1.copy()
    snp = np.arange(50, genome_len - 50, 97)
    snp = np.unique(np.concatenate([snp, snp[::5] + 3, snp[::5] + 9]))
    h2[snp] = (h1[snp] + rng.integers(1, 4, size=len(snp))) % 4
    haps = (acgt[h1], acgt[h2])
    out = []
    for i in range(n):
        L = int(rng.integers(80, 150))
        a = int(rng.integers(0, genome_len - L))
        s = haps[int(rng.integers(0, 2))][a:a + L].copy()
        e = rng.random(L) < err
        s[e] = acgt[rng.integers(0, 4, size=int(e.sum()))]
        if i % 40 == 0:
            p = int(rng.integers(0, L - 6))
            s[p:p + 3] = ord("N")
        out.append(s.tobytes())
    return out


def sample(seed, n=1600, genome_len=12000):
    from kmertools_amd.device import to_csr
    return to_csr(diploid_reads(seed, n, genome_len))


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


def by_a(a, *rest):
    order = np.argsort(a, kind="stable")
    return (a[order],) + tuple(r[order] for r in rest)


def het_dev(torch, c, lo, hi, middle, sort, room, with_counts=True, with_sums=True):
    """device mode into arrays of room + 3 entries: nothing at or past n is written -> (a, b, ca, cb, census, matrix)"""
    ka = torch.full((room + 3,), -1, dtype=torch.int64, device="cuda")
    kb = torch.full((room + 3,), -1, dtype=torch.int64, device="cuda")
    ca = torch.full((room + 3,), -1, dtype=torch.int32, device="cuda") if with_counts else None
    cb = torch.full((room + 3,), -1, dtype=torch.int32, device="cuda") if with_counts else None
    cen = torch.zeros(8, dtype=torch.int64, device="cuda") if with_sums else None
    m = torch.zeros(ROWS * COLS, dtype=torch.int64, device="cuda") if with_sums else None
    n = c.hetmers_device(ka, kb, ca, cb, room, lo, hi, middle=middle, sort=sort, matrix=m, n_rows=ROWS if with_sums else 0,
                         n_cols=COLS if with_sums else 0, census=cen)
    torch.cuda.synchronize()
    assert n <= room and (ka[n:] == -1).all() and (kb[n:] == -1).all()
    if with_counts:
        assert (ca[n:] == -1).all() and (cb[n:] == -1).all()
    u64 = lambda t: t[:n].cpu().numpy().view(np.uint64)
    u32 = lambda t: t[:n].cpu().numpy().view(np.uint32)
    return (u64(ka), u64(kb), u32(ca) if with_counts else None, u32(cb) if with_counts else None,
            cen.cpu().numpy().view(np.uint64) if with_sums else None,
            m.cpu().numpy().view(np.uint64).reshape(ROWS, COLS) if with_sums else None)


def same(got, r, wm=None):
    a, b, ca, cb = got[:4]
    ok = np.array_equal(a, r.a) and np.array_equal(b, r.b)
    if ca is not None:
        ok = ok and np.array_equal(ca, r.ca) and np.array_equal(cb, r.cb)
    if len(got) > 4 and got[4] is not None:
        ok = ok and np.array_equal(got[4], r.census)
    if len(got) > 5 and got[5] is not None:
        ok = ok and np.array_equal(got[5], wm)
    return ok


def check_all_modes(torch, c, tk, tc, k, ranges=RANGES, middles=None, tag=None):
    """host and device mode, sorted and not, of counter c against the restatement of table (tk, tc) -> the wanted results"""
    wants = []
    for middle in ((False, True) if k % 2 else (False,)) if middles is None else middles:
        for lo, hi in ranges:
            r = hr.restate(tk, tc, k, lo, hi, middle)
            wm = hr.matrix_of(r.ca, r.cb, ROWS, COLS)
            wants.append(r)
            t = (tag, k, lo, hi, middle)
            assert (r.a < r.b).all() and len(np.unique(np.concatenate([r.a, r.b]))) == 2 * len(r.a)
            a, b, ca, cb, m, cen = c.hetmers(lo, hi, middle=middle, matrix=(ROWS, COLS), census=True)
            assert a.dtype == np.uint64 and b.dtype == np.uint64 and ca.dtype == np.uint32 and cb.dtype == np.uint32
            assert m.dtype == np.uint64 and m.shape == (ROWS, COLS) and cen.dtype == np.uint64
            assert same((a, b, ca, cb, cen, m), r, wm), (t, "host sorted", cen, r.census)
            a, b, ca, cb = c.hetmers(lo, hi, middle=middle, sort=False)
            assert len(np.unique(a)) == len(a), (t, "host unsorted: a pair twice")
            assert same(by_a(a, b, ca, cb), r), (t, "host unsorted")
            assert same(het_dev(torch, c, lo, hi, middle, True, len(r.a) + 5), r, wm), (t, "device sorted")
            got = het_dev(torch, c, lo, hi, middle, False, len(r.a))  # (exactly the room it needs)
            assert len(np.unique(got[0])) == len(got[0]), (t, "device unsorted: a pair twice")
            assert same(by_a(*got[:4]) + got[4:], r, wm), (t, "device unsorted")
    return wants


def snapshot(ctr):
    return ctr.size(), ctr.export_host()


def same_snapshot(ctr, snap):
    n, (k, c) = snap
    n2, (k2, c2) = snapshot(ctr)
    return n == n2 and np.array_equal(k, k2) and np.array_equal(c, c2)


def shape_of(r):
    """(a pair, a node of degree 1 whose neighbour has more, a node of degree >= 2, a node reached twice or reaching itself)"""
    if not len(r.F):
        return (False,) * 4
    one = r.deg == 1
    partner = np.minimum(np.searchsorted(r.F, r.first), len(r.F) - 1)
    return (len(r.a) > 0, bool((one & ~one[partner]).any()), bool((r.deg >= 2).any()), bool((r.subs != r.deg).any()))


# ---- 1. worked answers ----------------------------------------------------------------------------------------------------

KNOWN = json.load(open(os.path.join(GOLDEN, "hetmers_known.json")))["cases"]


@pytest.mark.parametrize("case", KNOWN, ids=lambda c: c["name"].replace(" ", "_"))
def test_hetmers_known_answers(torch_mod, ctx, case):
    k, lo, hi, middle = case["k"], case["min_count"], case["max_count"], case["middle"]
    tk, tc = sorted_table([hr.key_of(s) for s in case["table"]], list(case["table"].values()))
    want = [[hr.key_of(a), hr.key_of(b), ca, cb] for a, b, ca, cb in case["pairs"]]
    c = pairs_counter(ctx, k, tk, tc)
    try:
        a, b, ca, cb, cen = c.hetmers(lo, hi, middle=middle, census=True)
        assert [list(map(int, p)) for p in zip(a, b, ca, cb)] == want
        assert cen.tolist() == case["census"]
        a, b, ca, cb, cen, _ = het_dev(torch_mod, c, lo, hi, middle, True, len(want) + 2)
        assert [list(map(int, p)) for p in zip(a, b, ca, cb)] == want
        assert cen.tolist() == case["census"]
        check_all_modes(torch_mod, c, tk, tc, k, ((lo, hi),), (middle,))
    finally:
        c.close()


# ---- 2. random subsets of all canonical k-mers, k = 3..6 --------------------------------------------------------------------
# The seeds were chosen so that the subset, taken whole (range (1, None), every position), holds a pair, a node of degree 1
# that is in no pair, a node of degree >= 2 and a node whose solid substitutions outnumber its neighbours (reached twice, or
# reaching itself).  5 % of the 32 canonical 3-mers are too few k-mers for all four at once: that batch holds them over its
# ranges and modes together.
SEEDS = {(3, 0.05): 49, (3, 0.2): 49, (4, 0.05): 0, (4, 0.2): 0, (5, 0.05): 14, (5, 0.2): 6, (6, 0.05): 0, (6, 0.2): 1}


@pytest.mark.parametrize("k, density", sorted(SEEDS))
def test_hetmers_exhaustive_small_k(torch_mod, ctx, k, density):
    tk, tc = hr.random_subset(k, density, SEEDS[k, density])
    assert len(tk) and tc.min() >= 1 and tc.max() <= 5
    if (k, density) != (3, 0.05):
        assert all(shape_of(hr.restate(tk, tc, k))), (k, density)
    c = pairs_counter(ctx, k, tk, tc)
    try:
        snap = snapshot(c)
        wants = check_all_modes(torch_mod, c, tk, tc, k)
        assert len(wants) == (8 if k % 2 else 4)
        assert all(any(col) for col in zip(*(shape_of(r) for r in wants))), (k, density)
        assert same_snapshot(c, snap) and np.array_equal(snap[1][0], tk) and np.array_equal(snap[1][1], tc)
    finally:
        c.close()


# ---- 3. every k that takes another path -----------------------------------------------------------------------------------

@pytest.mark.parametrize("k", [10, 15, 16, 17, 21, 30, 31])
def test_hetmers_k_sweep(torch_mod, ctx, oracle, k):
    bases, offsets = sample(500 + k)
    tk, tc = sorted_table(*oracle.count_reads(bases, offsets, k))
    plain = hr.restate(tk, tc, k)
    # the sample is worth the name: pairs, nodes of degree 1 in no pair, nodes with several partners (the close SNPs)
    assert plain.census[0] == len(tk) > 15000 and plain.census[5] > 100 and plain.census[4] > 100
    assert plain.census[3] > 2 * plain.census[5]
    c = counter_of(ctx, k, bases, offsets, len(tk))
    try:
        snap = snapshot(c)
        wants = check_all_modes(torch_mod, c, tk, tc, k)
        assert same_snapshot(c, snap) and np.array_equal(snap[1][0], tk) and np.array_equal(snap[1][1], tc)
        assert len({len(w.a) for w in wants[:4]}) > 2  # the ranges differ
        if k % 2:
            assert 0 < wants[4].census[5] < wants[0].census[5]  # the middle base alone finds fewer pairs
    finally:
        c.close()


# ---- 4. k = 31: pairs that differ at the first, the last and the middle base ------------------------------------------------

def test_hetmers_k31_pairs_at_the_ends_and_the_middle(torch_mod, ctx):
    k = 31
    rng = np.random.default_rng(3131)
    keys, counts, placed = [], [], []
    for i, pos in enumerate((0, 30, 15, 0, 30)):
        f = int(rng.integers(0, 1 << 62, dtype=np.uint64))
        g = f ^ (int(rng.integers(1, 4)) << 2 * (k - 1 - pos))  # (position 0: bits 60..61)
        cf, cg = (int(min(x, hr.rc_np(np.array([x], np.uint64), k)[0])) for x in (f, g))
        keys += [cf, cg]
        counts += [10 + i, 20 + i]
        placed.append((min(cf, cg), max(cf, cg)))
    tk, tc = sorted_table(keys, counts)
    assert len(np.unique(tk)) == 10 and (tk >> np.uint64(60)).max() > 0
    c = pairs_counter(ctx, k, tk, tc)
    try:
        wants = check_all_modes(torch_mod, c, tk, tc, k, ((1, None),))
        assert sorted(zip(wants[0].a.tolist(), wants[0].b.tolist())) == sorted(placed)
        assert list(zip(wants[1].a.tolist(), wants[1].b.tolist())) == [placed[2]]  # the middle base alone
        assert wants[0].census.tolist()[:6] == [10, sum(counts), 0, 10, 0, 5]
    finally:
        c.close()


# ---- 5. the largest count, and counts either side of the matrix clamps ------------------------------------------------------

def test_hetmers_largest_count_and_matrix_clamps(torch_mod, ctx):
    k = 21
    rng = np.random.default_rng(2121)
    keys, counts = [], []
    # (minor, major): both clamps from below, at and above (ROWS - 1 = 3, COLS - 1 = 5), and 0xFFFFFFFF as an ordinary count
    want_counts = [(2, 4), (3, 5), (4, 6), (2, 5), (3, 4), (4, 4), (7, U32), (U32, U32), (U32 - 1, U32), (1, U32)]
    for mn, mx in want_counts:
        f = int(rng.integers(0, 1 << (2 * k), dtype=np.uint64))
        g = f ^ (int(rng.integers(1, 4)) << 2 * int(rng.integers(0, k)))
        keys += [int(min(x, hr.rc_np(np.array([x], np.uint64), k)[0])) for x in (f, g)]
        counts += [mn, mx] if rng.random() < 0.5 else [mx, mn]
    # a node of count 0xFFFFFFFF that is a neighbour and breaks a pair
    f = int(rng.integers(0, 1 << (2 * k), dtype=np.uint64))
    keys += [int(min(x, hr.rc_np(np.array([x], np.uint64), k)[0])) for x in (f, f ^ 1, f ^ (2 << 20))]
    counts += [5, 6, U32]
    tk, tc = sorted_table(keys, counts)
    assert len(np.unique(tk)) == len(tk) == 23
    c = pairs_counter(ctx, k, tk, tc)
    try:
        wants = check_all_modes(torch_mod, c, tk, tc, k, ((1, None), (1, U32 - 1), (U32, U32), (4, U32)))
        r = wants[0]
        assert sorted(zip(np.minimum(r.ca, r.cb).tolist(), np.maximum(r.ca, r.cb).tolist())) == sorted(want_counts)
        assert r.census[4] == 1 and r.census[7] > 4 * U32 and r.census[6] > 2 * U32  # exact u64 sums
        m = hr.matrix_of(r.ca, r.cb, ROWS, COLS)
        assert m[2, 4] == 1 and m[3, 5] == 5 and m[2, 5] == 1 and m[3, 4] == 2 and m[1, 5] == 1 and m.sum() == 10
        assert len(wants[1].a) == 7  # without 0xFFFFFFFF the broken pair (5, 6) is whole again
        assert len(wants[2].a) == 1 and wants[2].census[0] == 6
    finally:
        c.close()


# ---- 6. every table form before the call ------------------------------------------------------------------------------------

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
def test_hetmers_every_table_form(torch_mod, ctx, oracle, monkeypatch, size):
    torch = torch_mod
    k = 13
    if size == "one range":  # a table below 8192 slots is a single range
        bases, offsets = sample(513, n=40, genome_len=900)
        cap = 4096
    else:
        bases, offsets = sample(2013)
        cap = 1 << 17
    tk, tc = sorted_table(*oracle.count_reads(bases, offsets, k))
    assert (len(tk) < 3000) if size == "one range" else (len(tk) > 10000)
    lo, hi = 2, 12
    r = hr.restate(tk, tc, k, lo, hi)
    wm = hr.matrix_of(r.ca, r.cb, ROWS, COLS)
    assert 0 < len(r.F) < len(tk) and len(r.a) > 20 and (r.census[4] > 0 or size == "one range")
    for form in FORMS:
        for mode in ("host", "device"):
            c, target = table_in_form(torch, ctx, form, k, bases, offsets, tk, tc, cap, monkeypatch)
            try:
                assert c.capacity() < 8192 if size == "one range" else c.capacity() >= 4 * 8192
                before = tuple(t.clone() for t in target) if target else None
                if mode == "host":
                    a, b, ca, cb, m, cen = c.hetmers(lo, hi, matrix=(ROWS, COLS), census=True)
                    got = (a, b, ca, cb, cen, m)
                else:
                    got = het_dev(torch, c, lo, hi, False, False, len(r.a))
                    got = by_a(*got[:4]) + got[4:]
                assert same(got, r, wm), (form, mode)
                n, (ek, ec) = snapshot(c)  # the table's content did not change
                assert n == len(tk) and np.array_equal(ek, tk) and np.array_equal(ec, tc), (form, mode)
                if target:
                    torch.cuda.synchronize()
                    assert torch.equal(before[0], target[0]) and torch.equal(before[1], target[1]), (form, mode)
            finally:
                c.close()


# ---- 7. a small table near load 0.7: probes walk past the home slot and wrap at the range end ---------------------------------

def home_slot(key, cap):
    """kttab::probe_of for a table of one range (cap a power of two below 8192) and k > 16: the top bits of ktd::khash"""
    h = (int(key) * 0x9E3779B97F4A7C15) & 0xFFFFFFFFFFFFFFFF
    h ^= h >> 32
    return h >> (64 - cap.bit_length() + 1)


def test_hetmers_small_table_near_full_probes_wrap(torch_mod, ctx, oracle):
    k, cap = 21, 1024
    bases, offsets = sample(6021, n=36, genome_len=330)
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
        assert wants[0].census[5] > 0 and wants[0].census[3] > 2 * wants[0].census[5]
    finally:
        c.close()


# ---- 8. shapes -----------------------------------------------------------------------------------------------------------------

def raw(L, t, lo=1, hi=U32, pos=0, ka=None, kb=None, ca=None, cb=None, max_out=0, n=None, matrix=None, n_rows=0, n_cols=0,
        census=None, mem=0, sort=1):
    ptr = lambda x: None if x is None else x.ctypes.data
    return L.kt_ctr_hetmers(t, lo, hi, pos, ptr(ka), ptr(kb), ptr(ca), ptr(cb), max_out, None if n is None else C.byref(n),
                            ptr(matrix), n_rows, n_cols, ptr(census), mem, sort)


def test_hetmers_shapes(torch_mod, ctx, oracle):
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
            a, b, ca, cb, m, cen = empty.hetmers(census=True, matrix=(ROWS, COLS), sort=sort)
            assert len(a) == 0 and len(b) == 0 and len(ca) == 0 and len(cb) == 0 and not cen.any() and not m.any()
            got = het_dev(torch, empty, 1, None, False, sort, 4)
            assert len(got[0]) == 0 and not got[4].any() and not got[5].any()
        n = C.c_uint64(99)
        cen, mat = np.full(8, 7, np.uint64), np.full(ROWS * COLS, 9, np.uint64)
        assert raw(L, empty._h, n=n, census=cen, matrix=mat, n_rows=ROWS, n_cols=COLS) == 0
        assert n.value == 0 and (cen == 7).all() and (mat == 9).all() and empty.size() == 0
        one_key = hr.key_of("ACGTTGCATGCAGGATCCATTAG")
        one = pairs_counter(ctx, k, [one_key], [3])
        made.append(one)
        wants = check_all_modes(torch, one, np.array([one_key], np.uint64), np.array([3], np.uint32), k, ((1, None), (4, None)))
        assert wants[0].census.tolist() == [1, 3, 1, 0, 0, 0, 0, 0] and not wants[1].census.any()
        # a table whose entries, candidates and pairs are no multiple of the workgroup tile (nor of anything else)
        bases, offsets = sample(723)
        tk, tc = sorted_table(*oracle.count_reads(bases, offsets, k))
        assert len(tk) % 256 and len(tk) > 20000
        c = counter_of(ctx, k, bases, offsets, len(tk))
        made.append(c)
        r = hr.restate(tk, tc, k)
        r2 = hr.restate(tk, tc, k, 2, 9, True)
        wm = hr.matrix_of(r.ca, r.cb, ROWS, COLS).reshape(-1)
        want = len(r.a)
        assert want > 300 and want % 64
        # max_out == 0: only the number, the census and the matrix, no arrays
        for mem in (0, 1):
            for sort in (0, 1):
                n = C.c_uint64(99)
                if mem == 0:
                    cen, mat = np.zeros(8, np.uint64), np.zeros(ROWS * COLS, np.uint64)
                    assert raw(L, c._h, n=n, census=cen, matrix=mat, n_rows=ROWS, n_cols=COLS, sort=sort) == 0
                else:
                    dcen = torch.zeros(8, dtype=torch.int64, device="cuda")
                    dmat = torch.zeros(ROWS * COLS, dtype=torch.int64, device="cuda")
                    assert L.kt_ctr_hetmers(c._h, 1, U32, 0, None, None, None, None, 0, C.byref(n), dmat.data_ptr(), ROWS, COLS,
                                            dcen.data_ptr(), 1, sort) == 0
                    torch.cuda.synchronize()
                    cen, mat = dcen.cpu().numpy().view(np.uint64), dmat.cpu().numpy().view(np.uint64)
                assert n.value == want and np.array_equal(cen, r.census) and np.array_equal(mat, wm), (mem, sort)
        n = C.c_uint64(99)
        assert raw(L, c._h, lo=2, hi=9, pos=1, n=n) == 0 and n.value == len(r2.a) > 0  # census = matrix = NULL too
        # the census and the matrix are ADDED: twice doubles, and what was there stays
        cen, mat = np.arange(8, dtype=np.uint64), np.arange(ROWS * COLS, dtype=np.uint64)
        for _ in range(2):
            assert raw(L, c._h, n=n, census=cen, matrix=mat, n_rows=ROWS, n_cols=COLS) == 0
        assert np.array_equal(cen, np.arange(8, dtype=np.uint64) + 2 * r.census)
        assert np.array_equal(mat, np.arange(ROWS * COLS, dtype=np.uint64) + 2 * wm)
        dcen = torch.arange(8, dtype=torch.int64, device="cuda")
        dmat = torch.arange(ROWS * COLS, dtype=torch.int64, device="cuda")
        for _ in range(2):
            assert c.hetmers_device(None, None, None, None, 0, matrix=dmat, n_rows=ROWS, n_cols=COLS, census=dcen) == want
        torch.cuda.synchronize()
        assert np.array_equal(dcen.cpu().numpy().view(np.uint64), np.arange(8, dtype=np.uint64) + 2 * r.census)
        assert np.array_equal(dmat.cpu().numpy().view(np.uint64), np.arange(ROWS * COLS, dtype=np.uint64) + 2 * wm)
        # counts = NULL (both, or one of them), census = matrix = NULL: the keys alone
        ka, kb = np.full(want + 2, PRIME_K, np.uint64), np.full(want + 2, PRIME_K, np.uint64)
        assert raw(L, c._h, ka=ka, kb=kb, max_out=want, n=n) == 0 and n.value == want
        assert np.array_equal(ka[:want], r.a) and np.array_equal(kb[:want], r.b)
        assert (ka[want:] == PRIME_K).all() and (kb[want:] == PRIME_K).all()
        for which in ("ca", "cb"):
            cx = np.full(want + 2, PRIME_C, np.uint32)
            assert raw(L, c._h, ka=ka, kb=kb, max_out=want, n=n, **{which: cx}) == 0
            assert np.array_equal(cx[:want], r.ca if which == "ca" else r.cb) and (cx[want:] == PRIME_C).all()
        assert same(het_dev(torch, c, 1, None, False, True, want, with_counts=False, with_sums=False), r)
        # one short: KT_ERR_ARG, the number exact, nothing at or past max_out, the census and the matrix added
        for mem in (0, 1):
            for sort in (0, 1):
                n = C.c_uint64(0)
                if mem == 0:
                    ka, kb = np.full(want + 2, PRIME_K, np.uint64), np.full(want + 2, PRIME_K, np.uint64)
                    ca, cb = np.full(want + 2, PRIME_C, np.uint32), np.full(want + 2, PRIME_C, np.uint32)
                    cen, mat = np.zeros(8, np.uint64), np.zeros(ROWS * COLS, np.uint64)
                    rc = raw(L, c._h, ka=ka, kb=kb, ca=ca, cb=cb, max_out=want - 1, n=n, census=cen, matrix=mat, n_rows=ROWS,
                             n_cols=COLS, sort=sort)
                    tails = ka[want - 1:], kb[want - 1:], ca[want - 1:], cb[want - 1:]
                else:
                    dk = [torch.from_numpy(np.full(want + 2, PRIME_K, np.uint64).view(np.int64)).cuda() for _ in range(2)]
                    dc = [torch.from_numpy(np.full(want + 2, PRIME_C, np.uint32).view(np.int32)).cuda() for _ in range(2)]
                    dcen = torch.zeros(8, dtype=torch.int64, device="cuda")
                    dmat = torch.zeros(ROWS * COLS, dtype=torch.int64, device="cuda")
                    rc = L.kt_ctr_hetmers(c._h, 1, U32, 0, dk[0].data_ptr(), dk[1].data_ptr(), dc[0].data_ptr(), dc[1].data_ptr(),
                                          want - 1, C.byref(n), dmat.data_ptr(), ROWS, COLS, dcen.data_ptr(), 1, sort)
                    torch.cuda.synchronize()
                    tails = tuple(t.cpu().numpy().view(np.uint64)[want - 1:] for t in dk) + tuple(
                        t.cpu().numpy().view(np.uint32)[want - 1:] for t in dc)
                    cen, mat = dcen.cpu().numpy().view(np.uint64), dmat.cpu().numpy().view(np.uint64)
                assert rc == KT_ERR_ARG and L.kt_last_error() and n.value == want, (mem, sort)
                assert (tails[0] == PRIME_K).all() and (tails[1] == PRIME_K).all(), (mem, sort)
                assert (tails[2] == PRIME_C).all() and (tails[3] == PRIME_C).all(), (mem, sort)
                assert np.array_equal(cen, r.census) and np.array_equal(mat, wm), (mem, sort)
        with pytest.raises(device._lib.KmertoolsError):
            c.hetmers_device(*(torch.zeros(4, dtype=d, device="cuda") for d in (torch.int64, torch.int64, torch.int32, torch.int32)), 4)
    finally:
        for t in reversed(made):
            t.close()


# ---- 9. views and fences ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shift", [1, 3, 5])
def test_hetmers_into_shifted_views_between_guards(torch_mod, ctx, oracle, shift):
    torch = torch_mod
    k = 27
    bases, offsets = sample(7000 + shift)
    tk, tc = sorted_table(*oracle.count_reads(bases, offsets, k))
    c = counter_of(ctx, k, bases, offsets, len(tk))
    guard = 4096
    KG, CG, EG = 0x7E7E7E7E7E7E7E7E, 0x5C5C5C5C, 0x4B4B4B4B4B4B4B4B
    try:
        for lo, hi, middle in ((1, None, False), (2, None, True)):
            r = hr.restate(tk, tc, k, lo, hi, middle)
            wm = hr.matrix_of(r.ca, r.cb, ROWS, COLS).reshape(-1)
            n = len(r.a)
            assert n > 64
            for sort in (True, False):
                bka, bkb = (torch.full((guard + shift + n + guard,), KG, dtype=torch.int64, device="cuda") for _ in range(2))
                bca, bcb = (torch.full((guard + shift + n + guard,), CG, dtype=torch.int32, device="cuda") for _ in range(2))
                be, bm = (torch.full((guard + shift + w + guard,), EG, dtype=torch.int64, device="cuda") for w in (8, ROWS * COLS))
                sl = slice(guard + shift, guard + shift + n)
                ve, vm = be[guard + shift:guard + shift + 8], bm[guard + shift:guard + shift + ROWS * COLS]
                assert bka[sl].data_ptr() == bka.data_ptr() + 8 * (guard + shift)
                assert bca[sl].data_ptr() == bca.data_ptr() + 4 * (guard + shift)
                ve.zero_()
                vm.zero_()
                got = c.hetmers_device(bka[sl], bkb[sl], bca[sl], bcb[sl], n, lo, hi, middle=middle, sort=sort, matrix=vm,
                                       n_rows=ROWS, n_cols=COLS, census=ve)
                torch.cuda.synchronize()
                assert got == n
                hka, hkb, hca, hcb, he, hm = (t.cpu().numpy() for t in (bka, bkb, bca, bcb, be, bm))
                for h, g in ((hka, KG), (hkb, KG), (hca, CG), (hcb, CG)):
                    assert (h[:guard + shift] == g).all() and (h[guard + shift + n:] == g).all(), (lo, sort)
                for h, w in ((he, 8), (hm, ROWS * COLS)):
                    assert (h[:guard + shift] == EG).all() and (h[guard + shift + w:] == EG).all(), (lo, sort)
                assert np.array_equal(he[guard + shift:guard + shift + 8].view(np.uint64), r.census), (lo, sort)
                assert np.array_equal(hm[guard + shift:guard + shift + ROWS * COLS].view(np.uint64), wm), (lo, sort)
                res = hka[sl].view(np.uint64), hkb[sl].view(np.uint64), hca[sl].view(np.uint32), hcb[sl].view(np.uint32)
                assert same(res if sort else by_a(*res), r), (lo, sort)
    finally:
        c.close()


# ---- 10. argument errors -----------------------------------------------------------------------------------------------------------

def test_hetmers_errors(torch_mod, ctx, oracle):
    torch = torch_mod
    from kmertools_amd import device
    from kmertools_amd._lib import KT_ERR_ARG, KT_ERR_FULL, lib
    L = lib()
    k = 21
    bases, offsets = sample(6000)
    made = []  # closed whatever happens: a table must not outlive its context

    def keep(c):
        made.append(c)
        return c

    try:
        a = keep(counter_of(ctx, k, bases, offsets, 1 << 17))
        even = keep(counter_of(ctx, 20, bases, offsets, 1 << 17))
        room = a.size() // 2
        ka, kb = np.full(room, PRIME_K, np.uint64), np.full(room, PRIME_K, np.uint64)
        ca, cb = np.full(room, PRIME_C, np.uint32), np.full(room, PRIME_C, np.uint32)
        cen, mat = np.full(8, 11, np.uint64), np.full(ROWS * COLS, PRIME_M, np.uint64)
        n = C.c_uint64(0)

        def call(t=a._h, **kw):
            for name, v in (("ka", ka), ("kb", kb), ("ca", ca), ("cb", cb), ("census", cen), ("matrix", mat), ("n_rows", ROWS),
                            ("n_cols", COLS), ("max_out", room), ("n", n)):
                kw.setdefault(name, v)
            return raw(L, t, **kw)

        for kw in (dict(t=None), dict(n=None), dict(lo=0), dict(lo=0, hi=0), dict(lo=3, hi=2), dict(lo=U32, hi=U32 - 1),
                   dict(pos=2), dict(pos=-1), dict(pos=8), dict(t=even._h, pos=1), dict(mem=2), dict(mem=-1), dict(ka=None),
                   dict(kb=None), dict(ka=None, kb=None), dict(n_rows=1), dict(n_cols=1), dict(n_rows=0, n_cols=0),
                   dict(n_rows=4097, n_cols=4096), dict(n_rows=U32, n_cols=U32)):
            assert call(**kw) == KT_ERR_ARG, kw
            assert L.kt_last_error(), kw
        # one shard of a sharded table (allocated as rank 0 of 2, never connected)
        sh = keep(device.Sharded(ctx, k, 1 << 16, 1 << 16, 2, 0, ("host", lambda s, r, n: 1), connect=False))
        assert call(t=sh.table._h) == KT_ERR_ARG and b"shard" in L.kt_last_error()
        # an overflowed table (far more distinct keys than slots)
        full = keep(device.Counter(ctx, k, 1024))
        full.add_pairs_host(np.arange(1, 5000, dtype=np.uint64) * 7919, np.ones(4999, np.uint32))
        assert call(t=full._h) == KT_ERR_FULL and L.kt_last_error()
        assert call(t=full._h, ka=None, kb=None, ca=None, cb=None, max_out=0) == KT_ERR_FULL
        # no refused call wrote anything
        assert (ka == PRIME_K).all() and (kb == PRIME_K).all() and (ca == PRIME_C).all() and (cb == PRIME_C).all()
        assert (cen == 11).all() and (mat == PRIME_M).all()
        # device outputs are left alone as well
        dka, dkb = (torch.from_numpy(ka.view(np.int64)).cuda() for _ in range(2))
        dca, dcb = (torch.from_numpy(ca.view(np.int32)).cuda() for _ in range(2))
        de = torch.full((8,), 11, dtype=torch.int64, device="cuda")
        dm = torch.full((ROWS * COLS,), 13, dtype=torch.int64, device="cuda")
        for t, lo, hi, pos, rows, want in ((a._h, 0, U32, 0, ROWS, KT_ERR_ARG), (a._h, 9, 8, 0, ROWS, KT_ERR_ARG),
                                           (a._h, 1, U32, 3, ROWS, KT_ERR_ARG), (even._h, 1, U32, 1, ROWS, KT_ERR_ARG),
                                           (a._h, 1, U32, 0, 1, KT_ERR_ARG), (sh.table._h, 1, U32, 0, ROWS, KT_ERR_ARG),
                                           (full._h, 1, U32, 0, ROWS, KT_ERR_FULL)):
            rc = L.kt_ctr_hetmers(t, lo, hi, pos, dka.data_ptr(), dkb.data_ptr(), dca.data_ptr(), dcb.data_ptr(), room, C.byref(n),
                                  dm.data_ptr(), rows, COLS, de.data_ptr(), 1, 1)
            assert rc == want and L.kt_last_error(), (lo, hi, pos, rows)
        torch.cuda.synchronize()
        for d in (dka, dkb):
            assert (d.cpu().numpy().view(np.uint64) == PRIME_K).all()
        for d in (dca, dcb):
            assert (d.cpu().numpy().view(np.uint32) == PRIME_C).all()
        assert bool((de == 11).all()) and bool((dm == 13).all())
        # the context is still good; the even k has its pairs at every position
        assert call() == 0 and n.value == len(hr.restate(*sorted_table(*a.export_host()), k).a)
        assert call(t=even._h) == 0 and n.value > 0
    finally:
        for c in reversed(made):
            c.close()


# ---- 11. one larger case ------------------------------------------------------------------------------------------------------------

def test_hetmers_full_size_k21(torch_mod, ctx, oracle):
    """11 000 reads of 150 bases from the two haplotypes of a random genome of 60 k bases (a SNP every 61 bases) with 0.5 %
    substitutions, k = 21: about 200 k nodes - some hundred workgroup tiles share the two cursors - against the restatement
    of the oracle's table of the same reads, in device mode, sorted and not, and in host mode."""
    torch = torch_mod
    k, L, G, n = 21, 150, 60_000, 11_000
    rng = np.random.default_rng(21)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    h1 = rng.integers(0, 4, size=G)
    h2 = h1.copy()
    h2[30::61] = (h1[30::61] + rng.integers(1, 4, size=len(h1[30::61]))) % 4
    haps = np.stack([acgt[h1], acgt[h2]])
    reads = haps[rng.integers(0, 2, size=n)[:, None], rng.integers(0, G - L, size=n)[:, None] + np.arange(L)[None, :]]
    err = rng.random(reads.shape) < 0.005
    reads[err] = acgt[rng.integers(0, 4, size=int(err.sum()))]
    bases, offsets = np.ascontiguousarray(reads.reshape(-1)), np.arange(n + 1, dtype=np.uint64) * np.uint64(L)
    tk, tc = sorted_table(*oracle.count_reads(bases, offsets, k, threads=16))
    assert 150_000 < len(tk) < 300_000
    c = counter_of(ctx, k, bases, offsets, len(tk))
    try:
        r = hr.restate(tk, tc, k)
        wm = hr.matrix_of(r.ca, r.cb, ROWS, COLS)
        print("full size: %d nodes, census %s" % (len(tk), r.census.tolist()), flush=True)
        assert r.census[5] > 10_000 and r.census[4] > 1_000 and r.census[3] > 2 * r.census[5] + 1_000
        assert same(het_dev(torch, c, 1, None, False, True, len(r.a)), r, wm)
        got = het_dev(torch, c, 1, None, False, False, len(r.a) + 1000)
        assert same(by_a(*got[:4]) + got[4:], r, wm)
        r2 = hr.restate(tk, tc, k, 2, None, True)
        assert 500 < len(r2.a) < len(r.a)
        a, b, ca, cb, cen = c.hetmers(2, None, middle=True, census=True)
        assert same((a, b, ca, cb, cen), r2)
        assert c.size() == len(tk)
    finally:
        c.close()


# ---- 12. the CLI end to end -----------------------------------------------------------------------------------------------------------

def run(*args, env=None):
    return subprocess.run([CLI, *map(str, args)], capture_output=True, timeout=600, env=env)


@pytest.fixture(scope="module")
def cli_bin():
    if not os.path.exists(CLI):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "kmertools_amd", "csrc"), "-j4"], stdout=subprocess.DEVNULL)
    return CLI


def table_of_file(oracle, path, k):
    return sorted_table(*oracle.count_reads(*oracle.to_csr([s for _, s in oracle.read_records(path)]), k))


@pytest.mark.parametrize("k", [21, 16])
def test_hetmers_cli_end_to_end(cli_bin, oracle, tmp_path, k):
    fa = tmp_path / "reads.fasta"
    fa.write_bytes(b"".join(b">rec%d lane=%d  sample x\n%s\n" % (i, i % 5, s) for i, s in enumerate(diploid_reads(90 + k, 3000))))
    tk, tc = table_of_file(oracle, str(fa), k)
    env = dict(os.environ, KT_CLI_TIMING="1")
    cases = [("plain", [], 1, None, False, 500, 1000), ("min2", ["--min-count", 2], 2, None, False, 500, 1000),
             ("small", ["--min-count", 2, "--max-count", 40, "--max-minor", 7, "--max-major", 12], 2, 40, False, 7, 12),
             ("estimate", ["--estimate-size", "--estimate-precision", 12], 1, None, False, 500, 1000)]
    if k % 2:
        cases += [("middle", ["--middle"], 1, None, True, 500, 1000),
                  ("middle_small", ["--middle", "--min-count", 3, "--max-minor", 3, "--max-major", 5], 3, None, True, 3, 5)]
    for name, flags, lo, hi, middle, mm, mj in cases:
        pairs, cov, matrix, stats, n = hr.want_files(tk, tc, k, lo, hi, middle, mm, mj)
        assert n > 50
        d = tmp_path / name
        r = run("hetmers", "-i", fa, "-o", d, "-k", k, *flags, env=env)
        assert r.returncode == 0, r.stderr
        assert (d / "hetmers.pairs").read_bytes() == pairs, (k, name)
        assert (d / "hetmers.cov").read_bytes() == cov, (k, name)
        assert (d / "hetmers.matrix").read_bytes() == matrix, (k, name)
        assert (d / "hetmers.stats").read_bytes() == stats, (k, name)
        assert sorted(os.listdir(d)) == ["hetmers.cov", "hetmers.matrix", "hetmers.pairs", "hetmers.stats"]
        d2 = tmp_path / (name + "_stats_only")
        r = run("hetmers", "-i", fa, "-o", d2, "-k", k, *flags, "--stats-only", env=env)
        assert r.returncode == 0, r.stderr
        assert sorted(os.listdir(d2)) == ["hetmers.matrix", "hetmers.stats"]
        assert (d2 / "hetmers.matrix").read_bytes() == matrix and (d2 / "hetmers.stats").read_bytes() == stats, (k, name)
    # some pair is written on its other strand
    lines = [ln.split(b"\t") for ln in hr.want_files(tk, tc, k)[0].splitlines()]
    assert any(hr.key_of(ln[1].decode()) != hr.key_of(hr.canon_s(ln[1].decode())) for ln in lines)
    # the same in batches of 7 reads, and from the dense bulk build
    pairs, cov, matrix, stats, _ = hr.want_files(tk, tc, k)
    for name, extra in (("batched", dict(KT_CLI_BATCH_READS="7")), ("dense", dict(KT_BULK_MIN_BASES="0"))):
        d = tmp_path / name
        r = run("hetmers", "-i", fa, "-o", d, "-k", k, env=dict(env, **extra))
        assert r.returncode == 0, r.stderr
        assert (d / "hetmers.pairs").read_bytes() == pairs and (d / "hetmers.cov").read_bytes() == cov, (k, name)
        assert (d / "hetmers.matrix").read_bytes() == matrix and (d / "hetmers.stats").read_bytes() == stats, (k, name)
    # a table that would take passes: refused before any file exists
    d = tmp_path / "passes"
    r = run("hetmers", "-i", fa, "-o", d, "-k", k, env=dict(env, KT_CTR_MAX_SLOTS="65536"))
    assert r.returncode != 0 and r.returncode != 2
    msg = r.stderr.decode()
    assert msg.startswith("Error: ") and "hetmers needs the whole table on the device" in msg
    assert not d.exists() or os.listdir(d) == []
