"""The two-pass pre-filter on the GPU against tests/prefilter_ref.py: after pass 1 `once` is exactly the model's array and
`twice` lies between the model's L and U; after pass 2 into an empty table every k-mer with two or more occurrences is there
with its exact count and every other key has count 1 and lies in E.  The batches, the k and the filter sizes are
prefilter_ref.CASES (the smallest filters, 2^10 words, and 2^12 / 2^10; 2^14 / 2^12 where the genome's reads would make
every k-mer a false positive); tests/test_prefilter_ref.py holds them to what these tests rely on.  The seed is fixed."""
import numpy as np
import pytest

import prefilter_ref as ref
from read_batches import Fenced, HostFenced, bases_view, offsets_view

pytestmark = pytest.mark.gpu
PROBE = {"KT_BULK_MIN_BASES": str(1 << 40)}


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


def absent_keys(keys, k, n=10000, seed=77):
    """n canonical-range values the batch does not hold (for k = 5 fewer exist: all that are left of the 4^k words)"""
    rng = np.random.default_rng(seed)
    if k <= 8:
        return np.setdiff1d(np.arange(4 ** k, dtype=np.uint64), keys)[:n]
    x = np.unique(rng.integers(0, 1 << (2 * k), size=n + n // 4, dtype=np.uint64))
    return np.setdiff1d(x, keys)[:n]


def check_filter(f, m, k, windows, tag):
    st = f.stats()
    assert st["windows"] == windows, (tag, st)
    assert st["once_bits_set"] == ref.popcount(m.once), (tag, st)
    lo, hi = ref.popcount(m.L), ref.popcount(m.U)
    print("%s: twice bits %d in [%d, %d], promotions %d >= %d" % (tag, st["twice_bits_set"], lo, hi, st["promotions"], m.min_promotions))
    assert lo <= st["twice_bits_set"] <= hi, (tag, st, lo, hi)
    assert m.min_promotions <= st["promotions"] <= windows, (tag, st, m.min_promotions)
    probe = np.concatenate([m.keys, absent_keys(m.keys, k)])
    got = f.query_host(probe)
    assert got.max(initial=0) <= 3
    b0, b1_must, b1_may = m.query(probe)
    assert np.array_equal((got & 1).astype(bool), b0), tag
    b1 = (got & 2).astype(bool)
    assert b1[b1_must].all(), (tag, "a k-mer of L is not marked in twice")
    assert not b1[~b1_may].any(), (tag, "a key outside U is marked in twice")
    return st


def check_table(ctr, twin_pairs, m, tag, base=0):
    """the table after pass 2: [2, max] is the twin's (`base` occurrences more of every key it held before), the rest count 1 in E"""
    wk, wc = twin_pairs
    rep = wc >= 2
    gk, gc = ctr.export_host()
    if base:
        held = np.isin(gk, m.keys[:100])
        assert held.sum() == 100 and (gc[held] >= base).all(), tag
        gc = gc - np.where(held, base, 0).astype(gc.dtype)
        keep = gc > 0
        gk, gc = gk[keep], gc[keep]
    many = gc >= 2
    assert np.array_equal(gk[many], wk[rep]) and np.array_equal(gc[many], wc[rep]), tag
    assert np.isin(gk[~many], m.E).all(), (tag, "a key with count 1 that is not in E")
    print("%s: %d of %d k-mers seen once got in (E: %d)" % (tag, int((~many).sum()), int((~rep).sum()), len(m.E)))
    return int((~many).sum())


@pytest.mark.parametrize("name, k, a, b", ref.CASES, ids=lambda v: str(v))
def test_two_passes(torch_mod, ctx, oracle, monkeypatch, name, k, a, b):
    from kmertools_amd import device
    torch = torch_mod
    batch, m = ref.batch(name), ref.model(oracle, name, k, a, b)
    tag = "%s k=%d a=%d b=%d" % (name, k, a, b)
    f = device.Prefilter(ctx, k, a, b, ref.SEED)
    bv, ov = bases_view(torch, batch.bases, (k + a) % 16), offsets_view(torch, batch.offsets)
    f.add_reads(bv, ov, batch.n)
    check_filter(f, m, k, int(m.counts.sum()), tag)
    twin = ref.table_of(oracle, name, k)
    ctr = device.Counter(ctx, k, 1 << 19)
    ctr.add_reads_filtered(f, bv, ov, batch.n)
    got_in = check_table(ctr, twin, m, tag)
    assert ctr.size() == int((twin[1] >= 2).sum()) + got_in
    # ... and against add_reads itself on a twin table, over the exported range [2, max]
    if (a, b) == (10, 10):
        t2 = device.Counter(ctx, k, 1 << 19)
        t2.add_reads(bv, ov, batch.n)
        x, y = ctr.export_host(min_count=2), t2.export_host(min_count=2)
        assert np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1]), tag
        t2.close()
    # cleared, the filter is empty again and lets nothing through
    f.clear()
    assert f.stats() == dict(windows=0, promotions=0, once_bits_set=0, twice_bits_set=0)
    ctr.clear()
    ctr.add_reads_filtered(f, bv, ov, batch.n)
    assert ctr.size() == 0
    ctr.close()
    f.close()


def test_false_positives_get_in(ctx, oracle):
    """the false-positive path runs: in the 2^14 / 2^12 filter some k-mers seen once reach the table, all of them from E"""
    from kmertools_amd import device
    name, k, a, b = "noisy", 31, 14, 12
    batch, m = ref.batch(name), ref.model(oracle, name, k, a, b)
    assert len(m.E) > 0
    f = device.Prefilter(ctx, k, a, b, ref.SEED)
    f.add_reads_host(batch.bases, batch.offsets)
    ctr = device.Counter(ctx, k, 1 << 19)
    ctr.add_reads_filtered_host(f, batch.bases, batch.offsets)
    got_in = check_table(ctr, ref.table_of(oracle, name, k), m, "host mem")
    assert 0 < got_in <= len(m.E)
    ctr.close()
    f.close()


def test_host_mem_and_order_of_batches(ctx, oracle):
    """host `mem`; two batches in two calls, and in the other order, leave the same `once` array (read through query)"""
    from kmertools_amd import device
    k, a, b = 21, 12, 10
    x, y = ref.batch("noisy"), ref.batch("short")
    keys = np.union1d(ref.table_of(oracle, "noisy", k)[0], ref.table_of(oracle, "short", k)[0])
    probe = np.concatenate([keys, absent_keys(keys, k)])
    seen = []
    for order in ((x, y), (y, x)):
        f = device.Prefilter(ctx, k, a, b, ref.SEED)
        for bt in order:
            f.add_reads_host(bt.bases, bt.offsets)
        st = f.stats()
        seen.append((st["windows"], st["once_bits_set"], f.query_host(probe) & 1))
        f.close()
    assert seen[0][0] == seen[1][0] and seen[0][1] == seen[1][1] and np.array_equal(seen[0][2], seen[1][2])
    both = ref.Model(keys, np.ones(len(keys)), a, b)     # (`once` does not look at the counts)
    assert seen[0][1] == ref.popcount(both.once) and np.array_equal(seen[0][2].astype(bool), both.query(probe)[0])


def test_parts_sum_to_the_whole(ctx, oracle):
    from kmertools_amd import device
    name, k, a, b = "noisy", 31, 14, 12
    batch, m = ref.batch(name), ref.model(oracle, name, k, a, b)
    f = device.Prefilter(ctx, k, a, b, ref.SEED)
    f.add_reads_host(batch.bases, batch.offsets)
    ctr = device.Counter(ctx, k, 1 << 18)
    ctr.add_reads_filtered_host(f, batch.bases, batch.offsets)
    whole = ctr.export_host()
    ks, cs = [], []
    for part in range(3):
        ctr.clear()
        ctr.add_reads_filtered_host(f, batch.bases, batch.offsets, 3, part)
        pk, pc = ctr.export_host()
        assert all(device.owner_of(int(v), 3) == part for v in pk[:200])
        ks.append(pk)
        cs.append(pc)
    gk, gc = np.concatenate(ks), np.concatenate(cs)
    o = np.argsort(gk, kind="stable")
    # (pass 2 only reads the filter: what it lets through is the same in every call)
    assert np.array_equal(gk[o], whole[0]) and np.array_equal(gc[o], whole[1])
    ctr.close()
    f.close()


def test_refusals(ctx):
    from kmertools_amd import _lib, device
    f = device.Prefilter(ctx, 21, 10, 10, ref.SEED)
    ctr = device.Counter(ctx, 31, 1024)
    b = ref.batch("short")
    with pytest.raises(_lib.KmertoolsError) as e:
        ctr.add_reads_filtered_host(f, b.bases, b.offsets)
    assert e.value.code == _lib.KT_ERR_ARG and "k" in str(e.value)
    assert ctr.size() == 0
    with pytest.raises(_lib.KmertoolsError):
        ctr.add_reads_filtered_host(f, b.bases, b.offsets, 3, 3)
    for bad in ((9, 10), (10, 9), (35, 10), (10, 35)):
        with pytest.raises(_lib.KmertoolsError) as e:
            device.Prefilter(ctx, 21, bad[0], bad[1])
        assert e.value.code == _lib.KT_ERR_ARG
    for k in (0, 32):
        with pytest.raises(_lib.KmertoolsError):
            device.Prefilter(ctx, k, 10, 10)
    ctr.close()
    f.close()


def test_table_that_holds_pairs_keeps_them(ctx, oracle):
    from kmertools_amd import device
    name, k, a, b = "noisy", 21, 14, 12
    batch, m = ref.batch(name), ref.model(oracle, name, k, a, b)
    f = device.Prefilter(ctx, k, a, b, ref.SEED)
    f.add_reads_host(batch.bases, batch.offsets)
    ctr = device.Counter(ctx, k, 1 << 18)
    held = m.keys[:100]
    ctr.add_pairs_host(held, np.full(100, 1000, np.uint32))
    ctr.add_reads_filtered_host(f, batch.bases, batch.offsets)
    check_table(ctr, ref.table_of(oracle, name, k), m, "on top of pairs", base=1000)
    ctr.close()
    f.close()


@pytest.mark.parametrize("shift", [0, 1, 5])
def test_query_views_and_fenced_output(torch_mod, ctx, oracle, shift):
    from kmertools_amd import _lib, device
    torch = torch_mod
    name, k, a, b = "short", 15, 12, 10
    batch, m = ref.batch(name), ref.model(oracle, name, k, a, b)
    f = device.Prefilter(ctx, k, a, b, ref.SEED)
    f.add_reads(bases_view(torch, batch.bases, shift), offsets_view(torch, batch.offsets), batch.n)
    probe = np.concatenate([m.keys, absent_keys(m.keys, k, 1003)])
    n = len(probe)
    raw = torch.zeros(n + 2, dtype=torch.int64, device="cuda")
    raw[1:n + 1] = torch.from_numpy(probe.view(np.int64))
    kv = raw[1:n + 1]                                         # 8 mod 16
    out = Fenced(torch, n, torch.uint8, align=shift)
    f.query(kv, n, out.t)
    torch.cuda.synchronize()
    out.check("query")
    got = out.np(np.uint8)
    host = HostFenced(n, np.uint8)
    f.query(probe, n, host.a, _lib.KT_MEM_HOST)
    host.check("query, host")
    assert np.array_equal(got, host.a) and np.array_equal((got & 1).astype(bool), m.query(probe)[0])
    f.close()


def test_grid_held_to_a_few_workgroups(torch_mod, ctx, oracle):
    from kmertools_amd import device
    torch = torch_mod
    name, k, a, b = "noisy", 31, 14, 12
    batch, m = ref.batch(name), ref.model(oracle, name, k, a, b)
    bv, ov = bases_view(torch, batch.bases, 3), offsets_view(torch, batch.offsets)
    with ctx.cu_limit(1):
        f = device.Prefilter(ctx, k, a, b, ref.SEED)
        f.add_reads(bv, ov, batch.n)
        check_filter(f, m, k, int(m.counts.sum()), "8 workgroups")
        ctr = device.Counter(ctx, k, 1 << 19)
        ctr.add_reads_filtered(f, bv, ov, batch.n)
        check_table(ctr, ref.table_of(oracle, name, k), m, "8 workgroups")
    ctr.close()
    f.close()


def test_small_table_overflows_as_add_reads_does(ctx, oracle, monkeypatch):
    from kmertools_amd import _lib, device
    for name, val in PROBE.items():
        monkeypatch.setenv(name, val)
    name, k, a, b = "noisy", 31, 14, 12
    batch = ref.batch(name)
    f = device.Prefilter(ctx, k, a, b, ref.SEED)
    f.add_reads_host(batch.bases, batch.offsets)
    errs = []
    for filtered in (True, False):
        ctr = device.Counter(ctx, k, 1024)
        assert ctr.capacity() == 1024
        if filtered:
            ctr.add_reads_filtered_host(f, batch.bases, batch.offsets)
        else:
            ctr.add_reads_host(batch.bases, batch.offsets)
        with pytest.raises(_lib.KmertoolsError) as e:
            ctr.size()
        errs.append((e.value.code, str(e.value)))
        ctr.close()
    assert errs[0] == errs[1] and errs[0][0] == _lib.KT_ERR_FULL
    f.close()
