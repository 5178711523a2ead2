"""Two-table comparison: kt_ctr_compare (the k-mer spectrum matrix of table A against table B, and the totals behind the
Jaccard, containment and weighted Jaccard) against a numpy restatement over the oracle's tables, in host and device mode,
with every table form on either side, a table compared with itself, over hash partitions, at full size; its argument
errors; and `kmertools compare` end to end, byte for byte against the restated files, resident and in passes."""
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "kmertools_amd", "bin", "kmertools")
GOLDEN = os.path.join(ROOT, "tests", "golden")
TOTALS = ("distinct_a", "distinct_b", "shared", "occurrences_a", "occurrences_b", "shared_min")
SHAPES = ((2, 2), (2, 7), (5, 2), (12, 9), (1001, 101), (4096, 4096))


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


# ---- the restatement ----------------------------------------------------------------------------------------------------

class Table:
    """the oracle's table of some reads: count of a canonical k-mer (0 when absent)"""

    def __init__(self, oracle, bases, offsets, k):
        wk, wc = oracle.count_reads(bases, offsets, k)
        order = np.argsort(wk)
        self.keys, self.counts = wk[order], wc[order]

    def count(self, keys):
        if not len(self.keys):
            return np.zeros(len(keys), np.uint32)
        i = np.minimum(np.searchsorted(self.keys, keys), len(self.keys) - 1)
        return np.where(self.keys[i] == keys, self.counts[i], 0).astype(np.uint32)


def want_compare(ta, tb, n_rows, n_cols):
    """(matrix, totals) of A's rows against B's columns, by definition"""
    m = np.zeros((n_rows, n_cols), np.uint64)
    b_of_a = tb.count(ta.keys).astype(np.int64)
    rows = np.minimum(ta.counts.astype(np.int64), n_rows - 1)
    np.add.at(m, (rows, np.minimum(b_of_a, n_cols - 1)), np.uint64(1))
    absent = ta.count(tb.keys) == 0  # B's k-mers that A does not hold: row 0
    np.add.at(m, (np.zeros(int(absent.sum()), np.int64), np.minimum(tb.counts[absent].astype(np.int64), n_cols - 1)),
              np.uint64(1))
    sh = b_of_a > 0
    tot = dict(distinct_a=len(ta.keys), distinct_b=len(tb.keys), shared=int(sh.sum()),
               occurrences_a=int(ta.counts.astype(np.int64).sum()), occurrences_b=int(tb.counts.astype(np.int64).sum()),
               shared_min=int(np.minimum(ta.counts.astype(np.int64), b_of_a)[sh].sum()))
    return m, tot


def random_reads(seed, n, lo=20, hi=300):
    rng = np.random.default_rng(seed)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    out = []
    for L in rng.integers(lo, hi, size=n):
        s = acgt[rng.integers(0, 4, size=int(L))].copy()
        if L > 60 and rng.random() < 0.2:
            s[int(rng.integers(0, L))] = ord("N")
        out.append(s.tobytes())
    return out


def sample_pair(oracle, seed, k):
    """two read sets with deliberate overlap: reads sampled (with errors) from one genome - disjoint read ids of the same
    genome seed - plus reads unique to each side, some of them repeated (counts 1..~40 on both sides)"""
    from kmertools_amd.device import to_csr
    genome = 30_000
    ab, ao = oracle.synth_reads(seed, 3000, 150, noise=True, genome_len=genome)
    bb, bo = oracle.synth_reads(seed, 1500, 150, noise=True, genome_len=genome, first_read=50_000)
    seqs_a = [ab[ao[i]:ao[i + 1]].tobytes() for i in range(len(ao) - 1)]
    seqs_b = [bb[bo[i]:bo[i + 1]].tobytes() for i in range(len(bo) - 1)]
    ua, ub = random_reads(seed + 1, 600), random_reads(seed + 2, 400)
    seqs_a += ua + ua[:100] * 3
    seqs_b += ub + ub[:50] * 2 + [b"A" * 3000]
    return to_csr(seqs_a), to_csr(seqs_b)


def counter_of(ctx, k, bases, offsets, n_keys, **kw):
    from kmertools_amd import device
    c = device.Counter(ctx, k, max(1 << 16, 2 * n_keys))
    c.add_reads_host(bases, offsets, **kw)
    return c


def compare_device(torch, a, b, n_rows, n_cols, totals=True):
    m = torch.zeros((n_rows, n_cols), dtype=torch.int64, device="cuda")
    t = torch.zeros(6, dtype=torch.int64, device="cuda") if totals else None
    a.compare_into(b, m, n_rows, n_cols, t)
    torch.cuda.synchronize()
    tot = dict(zip(TOTALS, (int(v) for v in t.cpu().numpy().view(np.uint64)))) if totals else None
    return m.cpu().numpy().view(np.uint64), tot


def snapshot(ctr):
    return ctr.size(), ctr.export_host()


def same_snapshot(ctr, snap):
    n, (k, c) = snap
    n2, (k2, c2) = snapshot(ctr)
    return n == n2 and np.array_equal(k, k2) and np.array_equal(c, c2)


# ---- 1. the ABI against the restatement -----------------------------------------------------------------------------------

@pytest.mark.parametrize("k", [11, 15, 21, 31])
def test_compare_against_restatement(torch_mod, ctx, oracle, k):
    torch = torch_mod
    (ab, ao), (bb, bo) = sample_pair(oracle, 1000 + k, k)
    ta, tb = Table(oracle, ab, ao, k), Table(oracle, bb, bo, k)
    a = counter_of(ctx, k, ab, ao, len(ta.keys))
    b = counter_of(ctx, k, bb, bo, len(tb.keys))
    for n_rows, n_cols in SHAPES:
        want, wtot = want_compare(ta, tb, n_rows, n_cols)
        assert wtot["shared"] and wtot["shared"] < min(wtot["distinct_a"], wtot["distinct_b"])
        m, tot = a.compare(b, n_rows, n_cols, totals=True)
        assert m.shape == (n_rows, n_cols) and m.dtype == np.uint64
        assert np.array_equal(m, want), (k, n_rows, n_cols, "host", np.argwhere(m != want)[:5])
        assert tot == wtot, (k, n_rows, n_cols)
        assert np.array_equal(a.compare(b, n_rows, n_cols), want)
        m, tot = compare_device(torch, a, b, n_rows, n_cols)
        assert np.array_equal(m, want) and tot == wtot, (k, n_rows, n_cols, "device")
        m, _ = compare_device(torch, a, b, n_rows, n_cols, totals=False)
        assert np.array_equal(m, want), (k, n_rows, n_cols, "device, no totals")
    # the other way round: B's rows against A's columns
    want, wtot = want_compare(tb, ta, 64, 64)
    m, tot = b.compare(a, 64, 64, totals=True)
    assert np.array_equal(m, want) and tot == wtot
    # results are added into: twice doubles everything, and cell [0][0] stays as the caller left it
    from kmertools_amd._lib import KT_MEM_HOST
    want, wtot = want_compare(ta, tb, 40, 30)
    m = np.zeros((40, 30), np.uint64)
    t = np.zeros(6, np.uint64)
    a.compare_into(b, m, 40, 30, t, KT_MEM_HOST)
    a.compare_into(b, m, 40, 30, t, KT_MEM_HOST)
    assert m[0, 0] == 0 and np.array_equal(m, 2 * want) and t.tolist() == [2 * wtot[n] for n in TOTALS]
    dm = torch.zeros((40, 30), dtype=torch.int64, device="cuda")
    dm[0, 0] = 77
    a.compare_into(b, dm, 40, 30)
    a.compare_into(b, dm, 40, 30)
    torch.cuda.synchronize()
    got = dm.cpu().numpy().view(np.uint64)
    assert got[0, 0] == 77 and np.array_equal(got[1:], 2 * want[1:]) and np.array_equal(got[0, 1:], 2 * want[0, 1:])
    a.close()
    b.close()


# ---- 2. every table form -------------------------------------------------------------------------------------------------

def forms_of(torch, ctx, k, bases, offsets, n_keys, monkeypatch):
    """(tag, Counter) of the table of the reads in every form it can be in (the caller closes them)"""
    from kmertools_amd import device
    cap = max(1 << 16, 2 * n_keys)
    out = []
    monkeypatch.delenv("KT_BULK", raising=False)
    monkeypatch.delenv("KT_BULK_MIN_BASES", raising=False)
    c = device.Counter(ctx, k, cap)
    c.add_reads_host(bases, offsets)
    out.append(("probing", c))
    c = device.Counter(ctx, k, cap)
    ta_keys, ta_counts = out[0][1].export_host()
    c.add_pairs_host(ta_keys, ta_counts)
    out.append(("add_pairs", c))
    monkeypatch.setenv("KT_BULK", "1")
    monkeypatch.setenv("KT_BULK_MIN_BASES", "0")
    c = device.Counter(ctx, k, cap)
    c.add_reads_host(bases, offsets)
    out.append(("bulk", c))
    m = n_keys + 9
    xk = torch.zeros(m, dtype=torch.int64, device="cuda")
    xc = torch.zeros(m, dtype=torch.int32, device="cuda")
    c = device.Counter(ctx, k, cap)
    c.export_target(xk, xc, m)
    c.add_reads(torch.from_numpy(bases).cuda(), torch.from_numpy(offsets.astype(np.int64)).cuda(), len(offsets) - 1)
    out.append(("export target", c))
    if k <= 15:
        c = device.Counter(ctx, k, 4 ** k)
        assert c.capacity() == 4 ** k
        c.add_reads_host(bases, offsets)
        out.append(("direct", c))
    monkeypatch.delenv("KT_BULK")
    monkeypatch.delenv("KT_BULK_MIN_BASES")
    return out


@pytest.mark.parametrize("k", [13, 21])
def test_compare_every_table_form(torch_mod, ctx, oracle, monkeypatch, k):
    torch = torch_mod
    (ab, ao), (bb, bo) = sample_pair(oracle, 2000 + k, k)
    ta, tb = Table(oracle, ab, ao, k), Table(oracle, bb, bo, k)
    want, wtot = want_compare(ta, tb, 80, 50)
    n_forms = 5 if k <= 15 else 4

    def check(a, b, tag):
        sa, sb = snapshot(a), snapshot(b)
        m, tot = a.compare(b, 80, 50, totals=True)
        assert np.array_equal(m, want) and tot == wtot, (tag, k, "host")
        m, tot = compare_device(torch, a, b, 80, 50)
        assert np.array_equal(m, want) and tot == wtot, (tag, k, "device")
        assert same_snapshot(a, sa) and same_snapshot(b, sb), (tag, k, "a table changed")
        assert sa[0] == len(ta.keys) and sb[0] == len(tb.keys)

    # every form of A against a probing B
    forms = forms_of(torch, ctx, k, ab, ao, len(ta.keys), monkeypatch)
    assert len(forms) == n_forms
    for tag, a in forms:
        b = counter_of(ctx, k, bb, bo, len(tb.keys))
        check(a, b, ("A", tag))
        a.close()
        b.close()
    # every form of B against a dense A (the dense table's ranges are walked as they are)
    monkeypatch.setenv("KT_BULK", "1")
    monkeypatch.setenv("KT_BULK_MIN_BASES", "0")
    a = counter_of(ctx, k, ab, ao, len(ta.keys))
    monkeypatch.delenv("KT_BULK")
    monkeypatch.delenv("KT_BULK_MIN_BASES")
    forms = forms_of(torch, ctx, k, bb, bo, len(tb.keys), monkeypatch)
    for tag, b in forms:
        check(a, b, ("B", tag))
        b.close()
    a.close()
    # a table compared with itself, in every form: the diagonal, which is its spectrum
    for n in (2, 40):
        forms = forms_of(torch, ctx, k, ab, ao, len(ta.keys), monkeypatch)
        for tag, a in forms:
            s = snapshot(a)
            m, tot = a.compare(a, n, n, totals=True)
            spec, (d, occ) = a.spectrum(n, totals=True)
            assert np.array_equal(np.diag(m)[1:], spec[1:]) and m[0].sum() == 0, (tag, n)
            assert np.count_nonzero(m - np.diag(np.diag(m))) == 0, (tag, n)
            assert tot == dict(distinct_a=d, distinct_b=d, shared=d, occurrences_a=occ, occurrences_b=occ, shared_min=occ)
            m, _ = compare_device(torch, a, a, n, n)
            assert np.array_equal(np.diag(m)[1:], spec[1:]) and np.count_nonzero(m - np.diag(np.diag(m))) == 0, (tag, n)
            assert same_snapshot(a, s), tag
            a.close()


# ---- 3. hash partitions -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", [15, 31])
def test_compare_partitions_add_up(torch_mod, ctx, oracle, k):
    torch = torch_mod
    (ab, ao), (bb, bo) = sample_pair(oracle, 3000 + k, k)
    ta, tb = Table(oracle, ab, ao, k), Table(oracle, bb, bo, k)
    want, wtot = want_compare(ta, tb, 60, 45)
    a = counter_of(ctx, k, ab, ao, len(ta.keys))
    b = counter_of(ctx, k, bb, bo, len(tb.keys))
    whole, whole_tot = a.compare(b, 60, 45, totals=True)
    assert np.array_equal(whole, want) and whole_tot == wtot
    a.close()
    b.close()
    from kmertools_amd._lib import KT_MEM_HOST
    for n_parts in (3, 7):
        m = np.zeros((60, 45), np.uint64)
        t = np.zeros(6, np.uint64)
        dm = torch.zeros((60, 45), dtype=torch.int64, device="cuda")
        dt = torch.zeros(6, dtype=torch.int64, device="cuda")
        for part in range(n_parts):
            a = counter_of(ctx, k, ab, ao, len(ta.keys), n_parts=n_parts, part=part)
            b = counter_of(ctx, k, bb, bo, len(tb.keys), n_parts=n_parts, part=part)
            a.compare_into(b, m, 60, 45, t, KT_MEM_HOST)
            a.compare_into(b, dm, 60, 45, dt)
            torch.cuda.synchronize()
            a.close()
            b.close()
        assert np.array_equal(m, want) and t.tolist() == [wtot[n] for n in TOTALS], n_parts
        assert np.array_equal(dm.cpu().numpy().view(np.uint64), want), (n_parts, "device")
        assert dt.cpu().numpy().view(np.uint64).tolist() == [wtot[n] for n in TOTALS], (n_parts, "device")


# ---- 4. errors -------------------------------------------------------------------------------------------------------------

def test_compare_errors(torch_mod, ctx, oracle):
    torch = torch_mod
    from kmertools_amd import device
    from kmertools_amd._lib import KT_ERR_ARG, KT_ERR_FULL, KT_MEM_HOST, lib
    L = lib()
    k = 21
    (ab, ao), (bb, bo) = sample_pair(oracle, 4000, k)
    made = []  # closed whatever happens: a table must not outlive its context
    try:
        errors_body(torch, ctx, device, L, k, ab, ao, bb, bo, made, KT_ERR_ARG, KT_ERR_FULL, KT_MEM_HOST)
    finally:
        for c in reversed(made):
            c.close()


def errors_body(torch, ctx, device, L, k, ab, ao, bb, bo, made, KT_ERR_ARG, KT_ERR_FULL, KT_MEM_HOST):
    def keep(c):
        made.append(c)
        return c

    a = keep(counter_of(ctx, k, ab, ao, 1 << 20))
    b = keep(counter_of(ctx, k, bb, bo, 1 << 20))
    m = np.zeros(16 * 16, np.uint64)
    t = np.zeros(6, np.uint64)

    def call(x=a._h, y=b._h, mat=m.ctypes.data, R=16, C=16, tot=t.ctypes.data, mem=KT_MEM_HOST):
        return L.kt_ctr_compare(x, y, mat, R, C, tot, mem)

    assert call() == 0 and call(tot=None) == 0 and m.any() and t.any()
    m[:] = 0
    t[:] = 0
    other_k = keep(device.Counter(ctx, 23, 1 << 16))
    ctx2 = keep(device.Context(0, stream=torch.cuda.current_stream().cuda_stream))
    other_ctx = keep(device.Counter(ctx2, k, 1 << 20))
    other_ctx.add_reads_host(bb, bo)
    big = np.zeros(2, np.uint64)
    for kw in (dict(x=None), dict(y=None), dict(mat=None), dict(y=other_k._h), dict(x=other_k._h), dict(y=other_ctx._h),
               dict(x=other_ctx._h), dict(R=1), dict(C=1), dict(R=0, C=0), dict(R=4097, C=4097, mat=big.ctypes.data),
               dict(R=1 << 24, C=2, mat=big.ctypes.data), dict(mem=7)):
        assert call(**kw) == KT_ERR_ARG, kw
        assert L.kt_last_error(), kw
    assert not m.any() and not t.any()  # nothing was added by a refused call
    assert call(R=1 << 23, C=2, mat=np.zeros(1 << 24, np.uint64).ctypes.data) == 0  # 2^24 cells: the largest matrix
    # one shard of a sharded table (allocated as rank 0 of 2, never connected): refused on either side
    sh = keep(device.Sharded(ctx, k, 1 << 16, 1 << 16, 2, 0, ("host", lambda s, r, n: 1), connect=False))
    assert call(x=sh.table._h) == KT_ERR_ARG and b"shard" in L.kt_last_error()
    assert call(y=sh.table._h) == KT_ERR_ARG and b"shard" in L.kt_last_error()
    # an overflowed table (far more distinct keys than slots): KT_ERR_FULL, on either side
    full = keep(device.Counter(ctx, k, 1024))
    full.add_pairs_host(np.arange(1, 5000, dtype=np.uint64) * 7919, np.ones(4999, np.uint32))
    assert call(x=full._h) == KT_ERR_FULL and call(y=full._h) == KT_ERR_FULL
    # empty tables add nothing; an empty A puts B's spectrum into row 0, an empty B A's into column 0
    e1, e2 = keep(device.Counter(ctx, k, 1 << 16)), keep(device.Counter(ctx, k, 1 << 16))
    m[:] = 0
    t[:] = 0
    assert call(x=e1._h, y=e2._h) == 0 and call(x=e1._h, y=e1._h) == 0 and not m.any() and not t.any()
    ma, tot = e1.compare(b, 16, 16, totals=True)
    spec, (d, occ) = b.spectrum(16, totals=True)
    assert np.array_equal(ma[0, 1:], spec[1:]) and not ma[1:].any() and tot["distinct_b"] == d and tot["distinct_a"] == 0
    mb, tot = a.compare(e1, 16, 16, totals=True)
    spec, (d, occ) = a.spectrum(16, totals=True)
    assert np.array_equal(mb[1:, 0], spec[1:]) and not mb[:, 1:].any() and tot["occurrences_a"] == occ and tot["shared"] == 0
    assert call() == 0  # the context is still good


# ---- 5. full size -----------------------------------------------------------------------------------------------------------

def test_compare_full_size_k31(torch_mod, ctx):
    """two samples of 10 M x 150 bp reads of one 20 Mbp genome (disjoint read ids, sequencing errors on) at k = 31 through
    the bulk build: the matrix's rows and columns sum to the two spectra, the totals are theirs, a table against itself
    is diagonal, and `shared` is the number of A's k-mers that kt_ctr_lookup finds in B"""
    torch = torch_mod
    from kmertools_amd import device
    k, n, L, genome = 31, 10_000_000, 150, 20_000_000
    kpr = L - k + 1
    seed = 0xC0A1BE
    tabs = []
    for first in (0, n):
        bases = torch.empty(n * L, dtype=torch.uint8, device="cuda")
        offsets = torch.empty(n + 1, dtype=torch.int64, device="cuda")
        ctx.synth_reads(seed, n, L, bases, offsets, noise=True, genome_len=genome, first_read=first)
        c = device.Counter(ctx, k, int(1.9 * n * kpr))
        c.add_reads(bases, offsets, n)
        tabs.append(c)
        del bases, offsets
        torch.cuda.empty_cache()
    a, b = tabs
    R, C = 1001, 101
    m, tot = a.compare(b, R, C, totals=True)
    spec_a, (da, oa) = a.spectrum(R, totals=True)
    spec_b, (db, ob) = b.spectrum(C, totals=True)
    assert np.array_equal(m[1:].sum(axis=1), spec_a[1:])
    assert np.array_equal(m[:, 1:].sum(axis=0), spec_b[1:])
    assert (tot["distinct_a"], tot["occurrences_a"], tot["distinct_b"], tot["occurrences_b"]) == (da, oa, db, ob)
    assert m[0, 0] == 0 and int(m[1:, 0].sum()) == da - tot["shared"] and int(m[0, 1:].sum()) == db - tot["shared"]
    assert int(m[1:, 1:].sum()) == tot["shared"] > 15_000_000  # nearly all of the genome's k-mers are in both
    assert tot["shared_min"] <= min(oa, ob)
    # the coverage peak lies away from the register cells: the LDS tile and the global tier both take part
    peak = np.unravel_index(np.argmax(m[5:, 5:]), m[5:, 5:].shape)
    assert peak[0] > 20 and peak[1] > 20
    d, _ = compare_device(torch, a, b, R, C, totals=False)
    assert np.array_equal(d, m)
    mm, tt = a.compare(a, 301, 301, totals=True)
    spec, _ = a.spectrum(301, totals=True)
    assert np.array_equal(np.diag(mm)[1:], spec[1:]) and np.count_nonzero(mm - np.diag(np.diag(mm))) == 0
    assert tt["shared"] == da and tt["shared_min"] == oa
    # shared = A's keys found in B by kt_ctr_lookup (A exported to the device, looked up there)
    xk = torch.empty(da, dtype=torch.int64, device="cuda")
    xc = torch.empty(da, dtype=torch.int32, device="cuda")
    assert a.export(xk, xc, da) == da
    del xc
    hits = torch.empty(da, dtype=torch.int32, device="cuda")
    b.lookup(xk, da, hits)
    torch.cuda.synchronize()
    assert int((hits != 0).sum()) == tot["shared"]
    del xk, hits
    a.close()
    b.close()
    torch.cuda.empty_cache()


# ---- 6. the CLI end to end ----------------------------------------------------------------------------------------------------

def run(*args, env=None):
    return subprocess.run([CLI, *map(str, args)], capture_output=True, timeout=600, env=env)


def want_files(oracle, path_a, path_b, k, max_a, max_b):
    """the restated compare.matrix and compare.stats"""
    ta = Table(oracle, *oracle.to_csr([s for _, s in oracle.read_records(path_a)]), k)
    tb = Table(oracle, *oracle.to_csr([s for _, s in oracle.read_records(path_b)]), k)
    m, t = want_compare(ta, tb, max_a + 1, max_b + 1)
    matrix = "".join("\t".join(str(int(v)) for v in row) + "\n" for row in m)
    ratio = lambda num, den: "%.6f" % (num / den if den else 0.0)
    stats = "".join("%s\t%d\n" % (n, t[n]) for n in TOTALS)
    stats += "jaccard\t%s\n" % ratio(t["shared"], t["distinct_a"] + t["distinct_b"] - t["shared"])
    stats += "containment_a\t%s\n" % ratio(t["shared"], t["distinct_a"])
    stats += "containment_b\t%s\n" % ratio(t["shared"], t["distinct_b"])
    stats += "weighted_jaccard\t%s\n" % ratio(t["shared_min"], t["occurrences_a"] + t["occurrences_b"] - t["shared_min"])
    return matrix.encode(), stats.encode(), t


def noisy_fastq(seed, n, genome):
    rng = np.random.default_rng(seed)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    out = []
    for i in range(n):
        L = int(rng.integers(40, 220))
        a = int(rng.integers(0, len(genome) - L))
        s = genome[a:a + L].copy()
        err = rng.random(L) < 0.01
        s[err] = acgt[rng.integers(0, 4, size=int(err.sum()))]
        if rng.random() < 0.1:
            s[int(rng.integers(0, L))] = ord("N")
        out.append(b"@r%d x\n%s\n+\n%s\n" % (i, s.tobytes(), b"I" * L))
    return b"".join(out)


@pytest.fixture(scope="module")
def cli_bin():
    if not os.path.exists(CLI):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "kmertools_amd", "csrc"), "-j4"], stdout=subprocess.DEVNULL)
    return CLI


def test_compare_cli_golden_inputs(cli_bin, oracle, tmp_path):
    fq, fa, gz = (os.path.join(GOLDEN, n) for n in ("reads.fq", "reads.fa", "reads.fq.gz"))
    for a, b, k, max_a, max_b in ((fq, fa, 15, 1000, 100), (gz, fa, 21, 8, 3), (fa, gz, 11, 1, 1), (fq, fq, 31, 50, 50)):
        d = tmp_path / ("out_%d" % k)
        r = run("compare", "-i", a, "-a", b, "-o", d, "-k", k, "--max-a", max_a, "--max-b", max_b)
        assert r.returncode == 0, r.stderr
        wm, ws, t = want_files(oracle, a, b, k, max_a, max_b)
        assert (d / "compare.matrix").read_bytes() == wm, (a, b, k)
        assert (d / "compare.stats").read_bytes() == ws, (a, b, k)
        assert t["shared"] > 0
    # the defaults: 1001 x 101
    d = tmp_path / "defaults"
    r = run("compare", "--input=%s" % fq, "--alt-input", fa, "-o", d, "-k15")
    assert r.returncode == 0, r.stderr
    assert (d / "compare.matrix").read_bytes() == want_files(oracle, fq, fa, 15, 1000, 100)[0]


def test_compare_cli_noisy_fastq_against_fasta_in_passes(cli_bin, oracle, tmp_path):
    rng = np.random.default_rng(5)
    genome = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, size=30000)]
    fq = tmp_path / "reads.fastq"
    fq.write_bytes(noisy_fastq(6, 4000, genome))
    fa = tmp_path / "asm.fasta"  # the genome's first two thirds in lines of 70, and a contig of its own
    g = genome[:20000].tobytes()
    other = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, size=5000)].tobytes()
    fa.write_bytes(b">contig1 first\n" + b"\n".join(g[i:i + 70] for i in range(0, len(g), 70)) + b"\n>contig2\n" + other + b"\n")
    k = 25
    wm, ws, t = want_files(oracle, str(fq), str(fa), k, 200, 5)
    assert 0 < t["shared"] < t["distinct_b"]
    env = dict(os.environ, KT_CLI_TIMING="1")
    d1 = tmp_path / "resident"
    r = run("compare", "-i", fq, "-a", fa, "-o", d1, "-k", k, "--max-a", 200, "--max-b", 5, env=env)
    assert r.returncode == 0, r.stderr
    assert int(r.stderr.decode().split(" pass(es)")[0].split()[-1]) == 1
    assert (d1 / "compare.matrix").read_bytes() == wm and (d1 / "compare.stats").read_bytes() == ws
    small = str(max(1024, fq.stat().st_size // 2 * 19 // 10 // 5))
    d2 = tmp_path / "passes"
    r = run("compare", "-i", fq, "-a", fa, "-o", d2, "-k", k, "--max-a", 200, "--max-b", 5,
            env=dict(env, KT_CTR_MAX_SLOTS=small))
    assert r.returncode == 0, r.stderr
    assert int(r.stderr.decode().split(" pass(es)")[0].split()[-1]) >= 4
    assert (d2 / "compare.matrix").read_bytes() == (d1 / "compare.matrix").read_bytes()
    assert (d2 / "compare.stats").read_bytes() == (d1 / "compare.stats").read_bytes()
    # the dense bulk build on both sides gives the same files too
    d3 = tmp_path / "dense"
    r = run("compare", "-i", fq, "-a", fa, "-o", d3, "-k", k, "--max-a", 200, "--max-b", 5,
            env=dict(env, KT_BULK_MIN_BASES="0"))
    assert r.returncode == 0, r.stderr
    assert (d3 / "compare.matrix").read_bytes() == wm and (d3 / "compare.stats").read_bytes() == ws
