"""Set operations of two tables: kt_ctr_setop (intersect / subtract / union / xor under count ranges, four count rules,
sorted or not) against a numpy restatement over the oracle's tables - host and device mode, every table form on either
side, saturating counts, hash partitions, empty tables and a table with itself, its argument errors, shifted output views
between guards, at full size; and `kmertools setop` end to end, byte for byte against the restated files, resident and in
passes.  Every comparison is exact."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "kmertools_amd", "bin", "kmertools")
GOLDEN = os.path.join(ROOT, "tests", "golden")
OPS = ("intersect", "subtract", "union", "xor")
RULES = ("first", "min", "max", "sum")
PLAIN = ((1, None), (1, None))
# (a_range, b_range): plain presence; min_a = 2; max_b = 1; min_a = 2, max_a = 3, min_b = 2
RANGES = (PLAIN, ((2, None), (1, None)), ((1, None), (1, 1)), ((2, 3), (2, None)))
U32 = 0xFFFFFFFF


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
    """a table as sorted (keys, counts): count of a canonical k-mer (0 when absent)"""

    def __init__(self, keys, counts):
        order = np.argsort(keys)
        self.keys, self.counts = np.asarray(keys, np.uint64)[order], np.asarray(counts, np.uint32)[order]

    @classmethod
    def of_reads(cls, oracle, bases, offsets, k):
        return cls(*oracle.count_reads(bases, offsets, k))

    def count(self, keys):
        if not len(self.keys):
            return np.zeros(len(keys), np.uint32)
        i = np.minimum(np.searchsorted(self.keys, keys), len(self.keys) - 1)
        return np.where(self.keys[i] == keys, self.counts[i], 0).astype(np.uint32)


def want_setop(ta, tb, op, rule, ra=(1, None), rb=(1, None), keys=None):
    """(keys ascending, counts) of op(A, B) by definition; `keys`: only among these (sorted, distinct) k-mers"""
    if keys is None:
        keys = np.union1d(ta.keys, tb.keys)
    ca, cb = ta.count(keys).astype(np.uint64), tb.count(keys).astype(np.uint64)
    a = np.where((ca >= ra[0]) & (ca <= (U32 if ra[1] is None else ra[1])), ca, 0).astype(np.uint64)
    b = np.where((cb >= rb[0]) & (cb <= (U32 if rb[1] is None else rb[1])), cb, 0).astype(np.uint64)
    ina, inb = a > 0, b > 0
    keep = {"intersect": ina & inb, "subtract": ina & ~inb, "union": ina | inb, "xor": ina ^ inb}[op]
    c = {"first": np.where(ina, a, b), "min": np.where(ina & inb, np.minimum(a, b), a + b), "max": np.maximum(a, b),
         "sum": np.minimum(a + b, np.uint64(U32))}[rule]
    return keys[keep], c[keep].astype(np.uint32)


def noisy_reads(seed, n, k):
    """reads sampled from a small genome with substitutions, runs of N, lower-case stretches, some shorter than k"""
    rng = np.random.default_rng(seed)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    genome = acgt[rng.integers(0, 4, size=12000)]
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
    return out


def sample_pair(seed, k, n=1600):
    """A and B from overlapping parts of one noisy read set, some reads of each repeated up to five more times"""
    from kmertools_amd.device import to_csr
    reads = noisy_reads(seed, n, k)
    sa = reads[:n * 5 // 8] + reads[:40] * 2 + reads[700:720] * 5
    sb = reads[n * 3 // 8:] + reads[n - 30:] * 3 + reads[700:710]
    return to_csr(sa), to_csr(sb)


def counter_of(ctx, k, bases, offsets, n_keys, **kw):
    from kmertools_amd import device
    c = device.Counter(ctx, k, max(1 << 16, 2 * n_keys))
    c.add_reads_host(bases, offsets, **kw)
    return c


def pairs_counter(ctx, k, keys, counts, slots=1 << 16):
    from kmertools_amd import device
    c = device.Counter(ctx, k, slots)
    c.add_pairs_host(np.asarray(keys, np.uint64), np.asarray(counts, np.uint32))
    return c


def setop_dev(torch, a, b, op, rule, ra, rb, sort, room):
    keys = torch.full((room + 3,), -1, dtype=torch.int64, device="cuda")
    counts = torch.full((room + 3,), -1, dtype=torch.int32, device="cuda")
    n = a.setop_device(b, op, keys, counts, room, count=rule, a_range=ra, b_range=rb, sort=sort)
    torch.cuda.synchronize()
    assert n <= room and (keys[n:] == -1).all() and (counts[n:] == -1).all()
    return keys[:n].cpu().numpy().view(np.uint64), counts[:n].cpu().numpy().view(np.uint32)


def by_key(keys, counts):
    order = np.argsort(keys, kind="stable")
    return keys[order], counts[order]


def snapshot(ctr):
    return ctr.size(), ctr.export_host()


def same_snapshot(ctr, snap):
    n, (k, c) = snap
    n2, (k2, c2) = snapshot(ctr)
    return n == n2 and np.array_equal(k, k2) and np.array_equal(c, c2)


# ---- 1. the ABI against the restatement -----------------------------------------------------------------------------------

@pytest.mark.parametrize("k", [11, 15, 21, 31])
def test_setop_against_restatement(torch_mod, ctx, oracle, k):
    torch = torch_mod
    (ab, ao), (bb, bo) = sample_pair(100 + k, k)
    ta, tb = Table.of_reads(oracle, ab, ao, k), Table.of_reads(oracle, bb, bo, k)
    # the restated side first: the sample exercises every branch
    for op in ("subtract", "intersect"):
        assert len(want_setop(ta, tb, op, "first")[0]) and len(want_setop(tb, ta, op, "first")[0]), op
    shared = want_setop(ta, tb, "intersect", "first")[0]
    assert (ta.count(shared) != tb.count(shared)).any(), "the count rules cannot be told apart"
    for c in range(1, 6):
        assert (ta.counts == c).any() and (tb.counts == c).any(), c
    assert (ta.counts > 5).any() and (tb.counts > 5).any()
    for ra, rb in RANGES[1:]:
        assert any(not np.array_equal(want_setop(ta, tb, op, "first", ra, rb)[0], want_setop(ta, tb, op, "first")[0])
                   for op in OPS), (ra, rb)
    a = counter_of(ctx, k, ab, ao, len(ta.keys))
    b = counter_of(ctx, k, bb, bo, len(tb.keys))
    sa, sb = snapshot(a), snapshot(b)
    room = len(ta.keys) + len(tb.keys)
    for op in OPS:
        for rule in RULES:
            for ra, rb in RANGES:
                tag = (k, op, rule, ra, rb)
                wk, wc = want_setop(ta, tb, op, rule, ra, rb)
                assert (wc >= 1).all()
                gk, gc = a.setop(b, op, rule, ra, rb)
                assert gk.dtype == np.uint64 and gc.dtype == np.uint32
                assert np.array_equal(gk, wk) and np.array_equal(gc, wc), (tag, "host sorted")
                gk, gc = a.setop(b, op, rule, ra, rb, sort=False)
                assert len(np.unique(gk)) == len(gk), (tag, "host unsorted: a key twice")
                gk, gc = by_key(gk, gc)
                assert np.array_equal(gk, wk) and np.array_equal(gc, wc), (tag, "host unsorted")
                gk, gc = setop_dev(torch, a, b, op, rule, ra, rb, True, room)
                assert np.array_equal(gk, wk) and np.array_equal(gc, wc), (tag, "device sorted")
                gk, gc = setop_dev(torch, a, b, op, rule, ra, rb, False, len(wk))  # (exactly the room it needs)
                assert len(np.unique(gk)) == len(gk), (tag, "device unsorted: a key twice")
                gk, gc = by_key(gk, gc)
                assert np.array_equal(gk, wk) and np.array_equal(gc, wc), (tag, "device unsorted")
    # the other way round
    wk, wc = want_setop(tb, ta, "subtract", "max", (1, 4), (2, None))
    gk, gc = b.setop(a, "subtract", "max", (1, 4), (2, None))
    assert np.array_equal(gk, wk) and np.array_equal(gc, wc)
    assert same_snapshot(a, sa) and same_snapshot(b, sb)
    for bad in (dict(op="and"), dict(op="union", count="avg"), dict(op=2), dict(op="union", count=None)):
        with pytest.raises(ValueError):
            a.setop(b, **bad)
        with pytest.raises(ValueError):
            a.setop_device(b, bad["op"], None, None, 0, **{n: v for n, v in bad.items() if n != "op"})
    a.close()
    b.close()


# ---- 2. every table form on both sides ----------------------------------------------------------------------------------------

FORMS = ("probing", "add_pairs", "bulk", "export target", "direct")


def table_in_form(torch, ctx, form, k, bases, offsets, t, monkeypatch):
    """the table of the reads (restated: t) in one of the forms a table can be in"""
    from kmertools_amd import device
    cap = max(1 << 16, 2 * len(t.keys))
    monkeypatch.delenv("KT_BULK", raising=False)
    monkeypatch.delenv("KT_BULK_MIN_BASES", raising=False)
    if form in ("bulk", "export target"):
        monkeypatch.setenv("KT_BULK", "1")
        monkeypatch.setenv("KT_BULK_MIN_BASES", "0")
    if form == "direct":
        c = device.Counter(ctx, k, 4 ** k)
        assert c.capacity() == 4 ** k
    else:
        c = device.Counter(ctx, k, cap)
    if form == "add_pairs":
        c.add_pairs_host(t.keys, t.counts)
    elif form == "export target":
        m = len(t.keys) + 9
        xk = torch.zeros(m, dtype=torch.int64, device="cuda")
        xc = torch.zeros(m, dtype=torch.int32, device="cuda")
        c.export_target(xk, xc, m)
        c.add_reads(torch.from_numpy(bases).cuda(), torch.from_numpy(offsets.astype(np.int64)).cuda(), len(offsets) - 1)
    else:
        c.add_reads_host(bases, offsets)
    monkeypatch.delenv("KT_BULK", raising=False)
    monkeypatch.delenv("KT_BULK_MIN_BASES", raising=False)
    return c


def test_setop_every_table_form(torch_mod, ctx, oracle, monkeypatch):
    torch = torch_mod
    k = 13
    (ab, ao), (bb, bo) = sample_pair(2013, k)
    ta, tb = Table.of_reads(oracle, ab, ao, k), Table.of_reads(oracle, bb, bo, k)
    ra, rb = (1, 6), (2, None)
    n_run = 0
    for op, rule in (("union", "sum"), ("subtract", "first")):
        wk, wc = want_setop(ta, tb, op, rule, ra, rb)
        assert len(wk)
        for fa in FORMS:
            for fb in FORMS:
                a = table_in_form(torch, ctx, fa, k, ab, ao, ta, monkeypatch)
                b = table_in_form(torch, ctx, fb, k, bb, bo, tb, monkeypatch)
                gk, gc = a.setop(b, op, rule, ra, rb)
                assert np.array_equal(gk, wk) and np.array_equal(gc, wc), (op, fa, fb, "host")
                gk, gc = setop_dev(torch, a, b, op, rule, ra, rb, False, len(wk))
                gk, gc = by_key(gk, gc)
                assert np.array_equal(gk, wk) and np.array_equal(gc, wc), (op, fa, fb, "device")
                for c, t in ((a, ta), (b, tb)):  # neither table's content changed
                    n, (ek, ec) = snapshot(c)
                    assert n == len(t.keys) and np.array_equal(ek, t.keys) and np.array_equal(ec, t.counts), (op, fa, fb)
                a.close()
                b.close()
                n_run += 1
    assert n_run == 2 * 5 * 5
    # the walked table in its fresh form on the device path too (the host call above had made the probed side's image)
    for fa in FORMS:
        a = table_in_form(torch, ctx, fa, k, ab, ao, ta, monkeypatch)
        b = table_in_form(torch, ctx, fa, k, bb, bo, tb, monkeypatch)
        wk, wc = want_setop(ta, tb, "xor", "min")
        gk, gc = setop_dev(torch, a, b, "xor", "min", (1, None), (1, None), True, len(wk) + 5)
        assert np.array_equal(gk, wk) and np.array_equal(gc, wc), fa
        a.close()
        b.close()


# ---- 3. saturation and extremes -------------------------------------------------------------------------------------------------

def test_setop_saturation_and_extremes(torch_mod, ctx):
    k = 21
    big = U32 - 1
    a_keys, a_counts = [5, 77, 1000, 123456789, 4 ** 21 - 2], [big, 1, U32, 7, big]
    b_keys, b_counts = [77, 1000, 4 ** 21 - 2, 42], [U32, 1, 5, big]
    ta, tb = Table(a_keys, a_counts), Table(b_keys, b_counts)
    a, b = pairs_counter(ctx, k, a_keys, a_counts), pairs_counter(ctx, k, b_keys, b_counts)
    assert np.array_equal(a.export_host()[1], ta.counts) and np.array_equal(b.export_host()[1], tb.counts)
    top = 4 ** 21 - 2  # shared: 0xFFFFFFFE in A, 5 in B
    for rule, want_ab, want_ba in (("sum", U32, U32), ("min", 5, 5), ("max", big, big), ("first", big, 5)):
        for x, y, want in ((a, b, want_ab), (b, a, want_ba)):
            gk, gc = x.setop(y, "intersect", rule, (1, U32), (1, U32))
            assert int(gc[list(gk).index(top)]) == want, rule
    for op in OPS:
        for rule in RULES:
            for ra, rb in (PLAIN, ((1, U32), (1, U32)), ((U32, U32), (1, None)), ((big, None), (5, big)), ((1, big), (U32, None))):
                wk, wc = want_setop(ta, tb, op, rule, ra, rb)
                gk, gc = a.setop(b, op, rule, ra, rb)
                assert np.array_equal(gk, wk) and np.array_equal(gc, wc), (op, rule, ra, rb)
    a.close()
    b.close()


# ---- 4. hash partitions -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n_parts", [2, 3, 7])
def test_setop_partitions_combine(torch_mod, ctx, oracle, n_parts):
    torch = torch_mod
    k = 23
    (ab, ao), (bb, bo) = sample_pair(4000 + n_parts, k)
    ta, tb = Table.of_reads(oracle, ab, ao, k), Table.of_reads(oracle, bb, bo, k)
    cases = (("intersect", "min", (1, None), (1, None)), ("subtract", "first", (2, None), (1, None)),
             ("union", "sum", (1, None), (1, 3)), ("xor", "max", (1, 4), (2, None)))
    got = {c: [] for c in cases}
    n_sum = {c: 0 for c in cases}
    for part in range(n_parts):
        a = counter_of(ctx, k, ab, ao, len(ta.keys), n_parts=n_parts, part=part)
        b = counter_of(ctx, k, bb, bo, len(tb.keys), n_parts=n_parts, part=part)
        assert 0 < a.size() < len(ta.keys)
        for c in cases:
            op, rule, ra, rb = c
            gk, gc = a.setop(b, op, rule, ra, rb)
            assert (np.diff(gk.astype(np.int64)) > 0).all()  # each partition's output is sorted
            n_sum[c] += a.setop_device(b, op, None, None, 0, count=rule, a_range=ra, b_range=rb)
            dk, dc = setop_dev(torch, a, b, op, rule, ra, rb, True, len(gk))
            assert np.array_equal(dk, gk) and np.array_equal(dc, gc)
            got[c].append((gk, gc))
        a.close()
        b.close()
    for c in cases:
        wk, wc = want_setop(ta, tb, *c)
        gk, gc = by_key(np.concatenate([g[0] for g in got[c]]), np.concatenate([g[1] for g in got[c]]))
        assert len(wk) and np.array_equal(gk, wk) and np.array_equal(gc, wc), c
        assert n_sum[c] == len(wk), c


# ---- 5. edges and errors ----------------------------------------------------------------------------------------------------------

PRIME_K, PRIME_C = 0xA5A5A5A5A5A5A5A5, 0x5A5A5A5A


def raw_setop(L, a, b, op=0, rule=0, ra=(1, U32), rb=(1, U32), keys=None, counts=None, max_out=0, n=None, mem=0, sort=1):
    ptr = lambda x: None if x is None else x.ctypes.data
    return L.kt_ctr_setop(a, b, op, rule, ra[0], ra[1], rb[0], rb[1], ptr(keys), ptr(counts), max_out,
                          None if n is None else C.byref(n), mem, sort)


def test_setop_edges(torch_mod, ctx, oracle):
    torch = torch_mod
    from kmertools_amd import device
    from kmertools_amd._lib import KT_ERR_ARG, lib
    L = lib()
    k = 21
    (ab, ao), (bb, bo) = sample_pair(5000, k)
    ta, tb = Table.of_reads(oracle, ab, ao, k), Table.of_reads(oracle, bb, bo, k)
    a = counter_of(ctx, k, ab, ao, len(ta.keys))
    b = counter_of(ctx, k, bb, bo, len(tb.keys))
    e1, e2 = device.Counter(ctx, k, 1 << 16), device.Counter(ctx, k, 1 << 16)
    none = Table(np.zeros(0, np.uint64), np.zeros(0, np.uint32))
    try:
        # empty tables: A, B, both
        for x, y, tx, ty in ((e1, b, none, tb), (a, e1, ta, none), (e1, e2, none, none), (e1, e1, none, none)):
            for op in OPS:
                wk, wc = want_setop(tx, ty, op, "sum", (1, None), (1, 2))
                gk, gc = x.setop(y, op, "sum", (1, None), (1, 2))
                assert np.array_equal(gk, wk) and np.array_equal(gc, wc), op
                room = len(wk) + 4
                dk, dc = setop_dev(torch, x, y, op, "sum", (1, None), (1, 2), True, room)
                assert np.array_equal(dk, wk) and np.array_equal(dc, wc), op
                if tx is none and ty is none:
                    assert len(gk) == 0
        assert e1.size() == 0 and e2.size() == 0
        # a table with itself
        sa = snapshot(a)
        for ra in ((1, None), (2, 5)):
            inr = (ta.counts >= ra[0]) & (ta.counts <= (U32 if ra[1] is None else ra[1]))
            assert inr.any()
            for rule in RULES:
                wc = ta.counts[inr].astype(np.uint64) * (2 if rule == "sum" else 1)
                for op in ("intersect", "union"):
                    gk, gc = a.setop(a, op, rule, ra, ra)
                    assert np.array_equal(gk, ta.keys[inr]) and np.array_equal(gc, wc.astype(np.uint32)), (op, rule, ra)
                    dk, dc = setop_dev(torch, a, a, op, rule, ra, ra, False, int(inr.sum()))
                    dk, dc = by_key(dk, dc)
                    assert np.array_equal(dk, gk) and np.array_equal(dc, gc), (op, rule, ra)
                for op in ("subtract", "xor"):
                    assert len(a.setop(a, op, rule, ra, ra)[0]) == 0, (op, rule, ra)
        # ... under different ranges on its two sides it is still one table
        wk, wc = want_setop(ta, ta, "xor", "first", (1, 2), (2, None))
        gk, gc = a.setop(a, "xor", "first", (1, 2), (2, None))
        assert len(wk) and np.array_equal(gk, wk) and np.array_equal(gc, wc)
        assert same_snapshot(a, sa)
        # count only: max_out = 0, no arrays
        for op in OPS:
            n = C.c_uint64(99)
            assert raw_setop(L, a._h, b._h, OPS.index(op), n=n) == 0
            assert n.value == len(want_setop(ta, tb, op, "first")[0])
            n = C.c_uint64(99)
            assert raw_setop(L, a._h, b._h, OPS.index(op), n=n, mem=1, sort=0) == 0
            assert n.value == len(want_setop(ta, tb, op, "first")[0])
        # one short: KT_ERR_ARG, the number exact, nothing at or past max_out
        for op in OPS:
            want = len(want_setop(ta, tb, op, "first")[0])
            for mem in (0, 1):
                for sort in (0, 1):
                    n = C.c_uint64(0)
                    if mem == 0:
                        keys, counts = np.full(want + 2, PRIME_K, np.uint64), np.full(want + 2, PRIME_C, np.uint32)
                        rc = raw_setop(L, a._h, b._h, OPS.index(op), keys=keys, counts=counts, max_out=want - 1, n=n, sort=sort)
                        tail_k, tail_c = keys[want - 1:], counts[want - 1:]
                    else:
                        dk = torch.from_numpy(np.full(want + 2, PRIME_K, np.uint64).view(np.int64)).cuda()
                        dc = torch.from_numpy(np.full(want + 2, PRIME_C, np.uint32).view(np.int32)).cuda()
                        rc = L.kt_ctr_setop(a._h, b._h, OPS.index(op), 0, 1, U32, 1, U32, dk.data_ptr(), dc.data_ptr(), want - 1,
                                            C.byref(n), 1, sort)
                        torch.cuda.synchronize()
                        tail_k = dk.cpu().numpy().view(np.uint64)[want - 1:]
                        tail_c = dc.cpu().numpy().view(np.uint32)[want - 1:]
                    assert rc == KT_ERR_ARG and L.kt_last_error() and n.value == want, (op, mem, sort)
                    assert (tail_k == PRIME_K).all() and (tail_c == PRIME_C).all(), (op, mem, sort)
    finally:
        for c in (a, b, e1, e2):
            c.close()


def test_setop_errors(torch_mod, ctx, oracle):
    torch = torch_mod
    from kmertools_amd import device
    from kmertools_amd._lib import KT_ERR_ARG, KT_ERR_FULL, lib
    L = lib()
    k = 21
    (ab, ao), (bb, bo) = sample_pair(6000, k)
    made = []  # closed whatever happens: a table must not outlive its context

    def keep(c):
        made.append(c)
        return c

    try:
        a = keep(counter_of(ctx, k, ab, ao, 1 << 18))
        b = keep(counter_of(ctx, k, bb, bo, 1 << 18))
        room = a.size() + b.size()
        keys, counts = np.full(room, PRIME_K, np.uint64), np.full(room, PRIME_C, np.uint32)
        n = C.c_uint64(0)

        def call(x=a._h, y=b._h, **kw):
            kw.setdefault("keys", keys)
            kw.setdefault("counts", counts)
            kw.setdefault("max_out", room)
            kw.setdefault("n", n)
            kw.setdefault("op", 2)
            return raw_setop(L, x, y, **kw)

        other_k = keep(device.Counter(ctx, 23, 1 << 16))
        ctx2 = keep(device.Context(0, stream=torch.cuda.current_stream().cuda_stream))
        other_ctx = keep(device.Counter(ctx2, k, 1 << 18))
        other_ctx.add_reads_host(bb, bo)
        for kw in (dict(x=None), dict(y=None), dict(n=None), dict(y=other_k._h), dict(x=other_k._h), dict(y=other_ctx._h),
                   dict(x=other_ctx._h), dict(op=4), dict(op=-1), dict(rule=4), dict(rule=-1), dict(ra=(0, U32)), dict(rb=(0, 5)),
                   dict(ra=(0, 0)), dict(ra=(3, 2)), dict(rb=(5, 4)), dict(mem=2), dict(mem=-1), dict(keys=None),
                   dict(counts=None), dict(keys=None, counts=None)):
            assert call(**kw) == KT_ERR_ARG, kw
            assert L.kt_last_error(), kw
        # one shard of a sharded table (allocated as rank 0 of 2, never connected): refused on either side
        sh = keep(device.Sharded(ctx, k, 1 << 16, 1 << 16, 2, 0, ("host", lambda s, r, n: 1), connect=False))
        assert call(x=sh.table._h) == KT_ERR_ARG and b"shard" in L.kt_last_error()
        assert call(y=sh.table._h) == KT_ERR_ARG and b"shard" in L.kt_last_error()
        # an overflowed table (far more distinct keys than slots): KT_ERR_FULL, on either side
        full = keep(device.Counter(ctx, k, 1024))
        full.add_pairs_host(np.arange(1, 5000, dtype=np.uint64) * 7919, np.ones(4999, np.uint32))
        assert call(x=full._h) == KT_ERR_FULL and call(y=full._h) == KT_ERR_FULL and L.kt_last_error()
        assert (keys == PRIME_K).all() and (counts == PRIME_C).all()  # no refused call wrote anything
        # device outputs are left alone as well
        dk = torch.from_numpy(keys.view(np.int64)).cuda()
        dc = torch.from_numpy(counts.view(np.int32)).cuda()
        for kw in (dict(op=7), dict(ra=(0, 1)), dict(rb=(9, 8)), dict(rule=9)):
            args = dict(op=2, rule=0, ra=(1, U32), rb=(1, U32))
            args.update(kw)
            rc = L.kt_ctr_setop(a._h, b._h, args["op"], args["rule"], *args["ra"], *args["rb"], dk.data_ptr(), dc.data_ptr(), room,
                                C.byref(n), 1, 1)
            assert rc == KT_ERR_ARG and L.kt_last_error(), kw
        rc = L.kt_ctr_setop(full._h, b._h, 2, 0, 1, U32, 1, U32, dk.data_ptr(), dc.data_ptr(), room, C.byref(n), 1, 1)
        assert rc == KT_ERR_FULL
        torch.cuda.synchronize()
        assert (dk.cpu().numpy().view(np.uint64) == PRIME_K).all() and (dc.cpu().numpy().view(np.uint32) == PRIME_C).all()
        assert call() == 0 and n.value == room - len(a.setop(b, "intersect")[0])  # the context is still good
    finally:
        for c in reversed(made):
            c.close()


# ---- 6. views and fences ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shift", [1, 3, 5])
def test_setop_into_shifted_views_between_guards(torch_mod, ctx, oracle, shift):
    torch = torch_mod
    k = 27
    (ab, ao), (bb, bo) = sample_pair(7000 + shift, k, n=2400)
    ta, tb = Table.of_reads(oracle, ab, ao, k), Table.of_reads(oracle, bb, bo, k)
    a = counter_of(ctx, k, ab, ao, len(ta.keys))
    b = counter_of(ctx, k, bb, bo, len(tb.keys))
    guard = 4096
    for op, rule in (("union", "max"), ("subtract", "first"), ("xor", "sum"), ("intersect", "min")):
        wk, wc = want_setop(ta, tb, op, rule)
        n = len(wk)
        assert n > 4096  # more than one wave tile of the sort
        for sort in (True, False):
            bk = torch.full((guard + shift + n + guard,), 0x7E7E7E7E7E7E7E7E, dtype=torch.int64, device="cuda")
            bc = torch.full((guard + shift + n + guard,), 0x6D6D6D6D, dtype=torch.int32, device="cuda")
            vk, vc = bk[guard + shift:guard + shift + n], bc[guard + shift:guard + shift + n]
            assert vk.data_ptr() == bk.data_ptr() + 8 * (guard + shift) and vc.data_ptr() == bc.data_ptr() + 4 * (guard + shift)
            got = a.setop_device(b, op, vk, vc, n, count=rule, sort=sort)
            torch.cuda.synchronize()
            assert got == n
            hk, hc = bk.cpu().numpy(), bc.cpu().numpy()
            assert (hk[:guard + shift] == 0x7E7E7E7E7E7E7E7E).all() and (hk[guard + shift + n:] == 0x7E7E7E7E7E7E7E7E).all(), (op, sort)
            assert (hc[:guard + shift] == 0x6D6D6D6D).all() and (hc[guard + shift + n:] == 0x6D6D6D6D).all(), (op, sort)
            gk = hk[guard + shift:guard + shift + n].view(np.uint64)
            gc = hc[guard + shift:guard + shift + n].view(np.uint32)
            if not sort:
                gk, gc = by_key(gk, gc)
            assert np.array_equal(gk, wk) and np.array_equal(gc, wc), (op, sort)
    a.close()
    b.close()


# ---- 7. full size -----------------------------------------------------------------------------------------------------------------

def test_setop_full_size_k31(torch_mod, ctx, oracle):
    """A = 10 M x 150 bp reads of a 20 Mbase genome with sequencing errors, B = 4 M reads of the same genome under another
    seed, k = 31.  On the whole outputs: the four sizes fit together and agree with kt_ctr_compare's totals, sorted output
    ascends strictly, every key of subtract looks up to 0 in B and to its count in A, every key of intersect (rule min) to
    the smaller of its two lookups.  And for the k-mers of 20 000 sampled reads of A: which of them each op emits, with
    which count, against the restatement over tables the oracle counts.  (The oracle counts, of A and of B, every read that
    holds at least one of the sample's k-mers - found with kt_ctr_read_solidity against a table of the sample, which the
    filter tests pin - so its tables hold the sample's k-mers with the counts they have in all of A and all of B; counting
    the 1.8 G k-mers of both on the CPU would take the oracle's map tens of GB and many minutes.)"""
    torch = torch_mod
    from kmertools_amd import device
    k, L, genome = 31, 150, 20_000_000
    n_a, n_b = 10_000_000, 4_000_000
    kpr = L - k + 1
    tabs, reads = [], []
    for n, seed in ((n_a, 0x5E70A), (n_b, 0x5E70B)):
        bases = torch.empty(n * L, dtype=torch.uint8, device="cuda")
        offsets = torch.empty(n + 1, dtype=torch.int64, device="cuda")
        ctx.synth_reads(seed, n, L, bases, offsets, noise=True, genome_len=genome)
        c = device.Counter(ctx, k, int(1.9 * n * kpr))
        c.add_reads(bases, offsets, n)
        tabs.append(c)
        reads.append((bases, offsets))
    a, b = tabs
    size_a, size_b = a.size(), b.size()
    _, tot = a.compare(b, 4, 4, totals=True)
    assert (tot["distinct_a"], tot["distinct_b"]) == (size_a, size_b)
    n_of = {op: a.setop_device(b, op, None, None, 0, sort=False) for op in OPS}
    print("full size: size(A) %d size(B) %d n_out %s" % (size_a, size_b, n_of), flush=True)
    assert n_of["intersect"] + n_of["subtract"] == size_a
    assert n_of["union"] == size_a + size_b - n_of["intersect"]
    assert n_of["xor"] == n_of["union"] - n_of["intersect"]
    assert n_of["intersect"] == tot["shared"] > 15_000_000
    assert n_of["subtract"] > 0 and n_of["xor"] > n_of["subtract"]

    # the sample: the distinct canonical k-mers of 20 000 reads of A, and the oracle's tables of the reads that hold any
    rng = np.random.default_rng(31)
    sample = np.sort(rng.choice(n_a, size=20000, replace=False))
    hs = reads[0][0].view(n_a, L)[torch.from_numpy(sample).cuda()].cpu().numpy()
    s_keys = np.unique(np.concatenate([np.minimum(f, r) for f, r, _ in (oracle.kmers(hs[i].tobytes(), k) for i in range(len(sample)))]))
    assert len(s_keys) > 1_000_000
    of_sample = device.Counter(ctx, k, 2 * len(s_keys))
    of_sample.add_pairs_host(s_keys, np.ones(len(s_keys), np.uint32))
    sampled = []
    for n, (bases, offsets) in zip((n_a, n_b), reads):
        nk = torch.zeros(n, dtype=torch.int32, device="cuda")
        ns = torch.zeros(n, dtype=torch.int32, device="cuda")
        of_sample.read_solidity(bases, offsets, n, 1, U32, nk, ns)
        torch.cuda.synchronize()
        idx = torch.nonzero(ns > 0).flatten()
        hb = bases.view(n, L)[idx].cpu().numpy().reshape(-1)
        print("full size: the oracle counts %d of %d reads" % (len(idx), n), flush=True)
        assert 20000 <= len(idx) < n // 2
        wk, wc = oracle.count_reads(hb, np.arange(len(idx) + 1, dtype=np.uint64) * np.uint64(L), k, threads=16)
        i = np.minimum(np.searchsorted(wk, s_keys), len(wk) - 1)
        hit = wk[i] == s_keys
        sampled.append(Table(s_keys[hit], wc[i][hit]))
        del nk, ns, idx, hb, wk, wc
    of_sample.close()
    del reads, bases, offsets
    torch.cuda.empty_cache()
    sa, sb = sampled
    assert len(sa.keys) == len(s_keys) and 0 < len(sb.keys) < len(s_keys)
    assert (sa.counts > 20).any() and (sa.counts == 1).any()
    d_sample = torch.from_numpy(s_keys.view(np.int64)).cuda()

    for op, rule in (("subtract", "first"), ("intersect", "min"), ("union", "sum"), ("xor", "max")):
        n = n_of[op]
        keys = torch.empty(n, dtype=torch.int64, device="cuda")
        counts = torch.empty(n, dtype=torch.int32, device="cuda")
        assert a.setop_device(b, op, keys, counts, n, count=rule, sort=True) == n
        torch.cuda.synchronize()
        assert bool((keys[1:] > keys[:-1]).all())  # strictly ascending (k = 31: the keys are below 2^62, signed order is theirs)
        in_a = torch.empty(n, dtype=torch.int32, device="cuda")
        in_b = torch.empty(n, dtype=torch.int32, device="cuda")
        a.lookup(keys, n, in_a)
        b.lookup(keys, n, in_b)
        torch.cuda.synchronize()
        if op == "subtract":
            assert bool((in_b == 0).all()) and bool((in_a == counts).all())
        elif op == "intersect":
            assert bool((in_a > 0).all()) and bool((in_b > 0).all()) and bool((torch.minimum(in_a, in_b) == counts).all())
        elif op == "union":
            assert bool((in_a + in_b == counts).all())  # (no count here is near 2^31)
        else:
            assert bool(((in_a == 0) != (in_b == 0)).all()) and bool((torch.maximum(in_a, in_b) == counts).all())
        del in_a, in_b
        # the sample's k-mers in this output: a sorted search on the device
        pos = torch.searchsorted(keys, d_sample).clamp_(max=n - 1)
        found = keys[pos] == d_sample
        gk = d_sample[found].cpu().numpy().view(np.uint64)
        gc = counts[pos[found]].cpu().numpy().view(np.uint32)
        wk, wc = want_setop(sa, sb, op, rule, keys=s_keys)
        print("full size: %s, %d entries, %d of the sample's k-mers" % (op, n, len(wk)), flush=True)
        assert len(wk) and np.array_equal(gk, wk) and np.array_equal(gc, wc), (op, rule)
        # the unsorted call emits the same pairs
        ukeys = torch.empty(n, dtype=torch.int64, device="cuda")
        ucounts = torch.empty(n, dtype=torch.int32, device="cuda")
        assert a.setop_device(b, op, ukeys, ucounts, n, count=rule, sort=False) == n
        torch.cuda.synchronize()
        order = torch.argsort(ukeys)
        assert bool((ukeys[order] == keys).all()) and bool((ucounts[order] == counts).all())
        del keys, counts, ukeys, ucounts, order, pos, found
        torch.cuda.empty_cache()
    a.close()
    b.close()
    torch.cuda.empty_cache()


# ---- 8. the CLI end to end ------------------------------------------------------------------------------------------------------------

def run(*args, env=None):
    return subprocess.run([CLI, *map(str, args)], capture_output=True, timeout=600, env=env)


def want_files(oracle, path_a, path_b, k, op, rule="first", ra=(1, None), rb=(1, None), acgt=False):
    """the restated kmers.counts (ascending numeric key) and setop.stats"""
    ta = Table.of_reads(oracle, *oracle.to_csr([s for _, s in oracle.read_records(path_a)]), k)
    tb = Table.of_reads(oracle, *oracle.to_csr([s for _, s in oracle.read_records(path_b)]), k)
    wk, wc = want_setop(ta, tb, op, rule, ra, rb)
    if acgt:
        lines = "".join("%s\t%d\n" % (oracle.numeric_to_kmer(int(key), k), int(c)) for key, c in zip(wk, wc))
    else:
        lines = "".join("%d\t%d\n" % (int(key), int(c)) for key, c in zip(wk, wc))
    inr = lambda t, r: int(((t.counts >= r[0]) & (t.counts <= (U32 if r[1] is None else r[1]))).sum())
    stats = "distinct_a\t%d\ndistinct_b\t%d\nin_a\t%d\nin_b\t%d\nemitted\t%d\nemitted_occurrences\t%d\n" % (
        len(ta.keys), len(tb.keys), inr(ta, ra), inr(tb, rb), len(wk), int(wc.astype(np.uint64).sum()))
    return lines.encode(), stats.encode(), len(wk)


def range_flags(ra, rb):
    out = []
    for name, v in (("--min-a", ra[0]), ("--max-a", ra[1]), ("--min-b", rb[0]), ("--max-b", rb[1])):
        if v is not None and not (name.startswith("--min") and v == 1):
            out += [name, v]
    return out


@pytest.fixture(scope="module")
def cli_bin():
    if not os.path.exists(CLI):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "kmertools_amd", "csrc"), "-j4"], stdout=subprocess.DEVNULL)
    return CLI


def test_setop_cli_golden_inputs(cli_bin, oracle, tmp_path):
    fq, fa, gz = (os.path.join(GOLDEN, n) for n in ("reads.fq", "reads.fa", "reads.fq.gz"))
    n_run = 0
    for a, b, k in ((fq, fa, 15), (gz, fa, 31), (fa, gz, 15), (fq, gz, 31)):
        for op in OPS:
            acgt = op == "union" and k == 31 and a == gz
            special = op == "xor" and k == 15 and a == fq
            rule, ra, rb = ("sum", (2, 9), (1, 3)) if special else ("first", (1, None), (1, None))
            d = tmp_path / ("out_%d" % n_run)
            args = ["setop", "-i", a, "-a", b, "-o", d, "-k", k, "--op", op]
            args += ["--count", rule] + range_flags(ra, rb) if special else []
            args += ["--acgt"] if acgt else []
            r = run(*args)
            assert r.returncode == 0, r.stderr
            lines, stats, n = want_files(oracle, a, b, k, op, rule, ra, rb, acgt)
            assert (d / "kmers.counts").read_bytes() == lines, (a, b, k, op)
            assert (d / "setop.stats").read_bytes() == stats, (a, b, k, op)
            assert sorted(os.listdir(d)) == ["kmers.counts", "setop.stats"]
            if op in ("union", "intersect"):
                assert n > 0
            # the same in batches of 7 reads
            d2 = tmp_path / ("batched_%d" % n_run)
            r = run(*(args[:6] + [d2] + args[7:]), env=dict(os.environ, KT_CLI_BATCH_READS="7"))
            assert r.returncode == 0, r.stderr
            assert (d2 / "kmers.counts").read_bytes() == lines and (d2 / "setop.stats").read_bytes() == stats, (a, b, k, op, "batched")
            n_run += 1
    assert n_run == 16


def noisy_fasta(seed, n, k):
    """records sampled from a small genome with substitutions, N and lower case, multi-word headers, some shorter than k"""
    return b"".join(b">rec%d lane=%d  sample x\n%s\n" % (i, i % 5, s) for i, s in enumerate(noisy_reads(seed, n, k)))


@pytest.mark.parametrize("k", [15, 31])
def test_setop_cli_noisy_pair_resident_and_in_passes(cli_bin, oracle, tmp_path, k):
    reads = noisy_fasta(80 + k, 3000, k)
    recs = reads.split(b">")[1:]
    fa = tmp_path / "a.fasta"
    fa.write_bytes(b">" + b">".join(recs[:2000] + recs[100:160] * 3))
    fb = tmp_path / "b.fa"
    fb.write_bytes(b">" + b">".join(recs[1200:] + recs[2900:] * 2))
    env = dict(os.environ, KT_CLI_TIMING="1")
    for op in OPS:
        special = op in ("subtract", "union")
        rule, ra, rb = ("max", (1, 6), (2, None)) if special else ("first", (1, None), (1, None))
        acgt = op == "xor"
        lines, stats, n = want_files(oracle, str(fa), str(fb), k, op, rule, ra, rb, acgt)
        assert n > 0
        args = ["--op", op, "-k", k] + (["--count", rule] + range_flags(ra, rb) if special else []) + (["--acgt"] if acgt else [])
        d1 = tmp_path / ("resident_" + op)
        r = run("setop", "-i", fa, "-a", fb, "-o", d1, *args, env=env)
        assert r.returncode == 0, r.stderr
        assert int(r.stderr.decode().split(" pass(es)")[0].split()[-1]) == 1
        assert (d1 / "kmers.counts").read_bytes() == lines and (d1 / "setop.stats").read_bytes() == stats, (k, op)
        d2 = tmp_path / ("batched_" + op)
        r = run("setop", "-i", fa, "-a", fb, "-o", d2, *args, env=dict(env, KT_CLI_BATCH_READS="7"))
        assert r.returncode == 0, r.stderr
        assert (d2 / "kmers.counts").read_bytes() == lines and (d2 / "setop.stats").read_bytes() == stats, (k, op, "batched")
        d3 = tmp_path / ("passes_" + op)
        r = run("setop", "-i", fa, "-a", fb, "-o", d3, *args, env=dict(env, KT_CTR_MAX_SLOTS="65536"))
        assert r.returncode == 0, r.stderr
        assert int(r.stderr.decode().split(" pass(es)")[0].split()[-1]) >= 3
        got = (d3 / "kmers.counts").read_bytes()
        assert got != lines or n < 2  # (passes follow one another: the file as a whole is not in key order)
        assert sorted(got.splitlines()) == sorted(lines.splitlines()), (k, op, "passes")
        assert (d3 / "setop.stats").read_bytes() == stats, (k, op, "passes")
        # the dense bulk build on both sides gives the same files
        d4 = tmp_path / ("dense_" + op)
        r = run("setop", "-i", fa, "-a", fb, "-o", d4, *args, env=dict(env, KT_BULK_MIN_BASES="0"))
        assert r.returncode == 0, r.stderr
        assert (d4 / "kmers.counts").read_bytes() == lines and (d4 / "setop.stats").read_bytes() == stats, (k, op, "dense")
