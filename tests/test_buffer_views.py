"""Every kernel on the memory a caller really hands over: read batches that start at any byte address inside a larger
buffer (`bases[5:]` is a legal call - the C ABI takes any pointer), surrounded by random ACGT bytes, so that a read of a
byte before or after the batch changes a k-mer, a walk or a minimiser instead of hitting an invalid `N`; offsets and
key arrays at 8 mod 16; every output inside guard bands of a fixed byte that must be untouched afterwards, including the
partial-write contracts (export into fewer slots than the table holds, a too small export target, minimisers beyond
`capacity`) and the outputs the API adds into (pre-filled, checked as prefill + expected); and the slab loops of the
oligo paths, host and generic, run to a second and third slab.  Results against the oracle: integers and f64 bit-exact,
f32 within 1e-6.  The fence is checked before the values, so that a failure says which of the two broke.

Every view keeps >= 4 KiB of slack on both sides and only bytes are poisoned, never offsets: a kernel that reads or writes
a little outside its range stays inside the allocation and shows up as a wrong value or a broken fence."""
import ctypes as C

import numpy as np
import pytest

from read_batches import (ACGT, GUARD, SLACK, Batch, Fenced, HostFenced, bases_view, host_bases_view,  # noqa: F401
                          noisy_reads, offsets_view)

pytestmark = pytest.mark.gpu

SHIFTS = (0, 1, 2, 3, 4, 5, 8, 12, 15, 16, 17, 31)   # odd, 4-aligned but not 16-aligned, aligned
CTR_SHIFTS = (0, 1, 3, 4, 15)                       # 1 and 3: the halo of kt_segment.hpp through the byte path
U32_MAX = 0xFFFFFFFF


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


@pytest.fixture(scope="module")
def hctx():
    from kmertools_amd import device
    c = device.Context(0)
    yield c
    c.close()


# ---- inputs ---------------------------------------------------------------------------------------------------------

def equal_reads(seed, n=1001, L=150):
    """reads of one length >= 16 (kt_oligo.hip's non-general tiles), N and lower case sprinkled in; n odd: the batch
    ends off a 16-byte boundary"""
    rng = np.random.default_rng(seed)
    alpha = np.frombuffer(b"ACGTNacgt", np.uint8)
    return [alpha[rng.choice(9, size=L, p=[.24, .24, .24, .24, .01, .0075, .0075, .0075, .0075])].tobytes()
            for _ in range(n)]


@pytest.fixture(scope="module")
def ragged():
    b = Batch("ragged", noisy_reads(0x5eed, 700))
    assert b.total % 16 and b.total % 32 and b.total > 4 * 8192
    return b


@pytest.fixture(scope="module")
def equal():
    b = Batch("equal", equal_reads(0x5eee))
    assert b.total % 16
    return b


# ---- oracle answers, computed once per module ------------------------------------------------------------------------

_memo = {}


def memo(key, fn):
    if key not in _memo:
        _memo[key] = fn()
    return _memo[key]


def oracle_kmers(oracle, batch, k):
    def run():
        ends, fs, rs = [], [], []
        for s, o in zip(batch.seqs, batch.offsets[:-1]):
            f, r, e = oracle.kmers(s, k)
            fs.append(f)
            rs.append(r)
            ends.append(e + np.uint64(o))
        return np.concatenate(fs), np.concatenate(rs), np.concatenate(ends)
    return memo(("kmers", batch.name, k), run)


def oracle_table(oracle, batch, k):
    return memo(("table", batch.name, k), lambda: oracle.count_reads(batch.bases, batch.offsets, k))


def oracle_oligo(oracle, batch, k, count_min, norm):
    return memo(("oligo", batch.name, k, count_min, norm),
                lambda: oracle.oligo_batch(batch.bases, batch.offsets, k, count_min, norm, 1.0, threads=8))


def sort_pairs(keys, counts):
    o = np.argsort(keys, kind="stable")
    return keys[o], counts[o]


def _sync(torch):
    torch.cuda.synchronize()


# ---- 1. read-consuming entry points on shifted views -------------------------------------------------------------------

@pytest.mark.parametrize("shift", SHIFTS)
@pytest.mark.parametrize("k", [1, 16, 17, 31])
def test_kmers_from_views(torch_mod, ctx, oracle, ragged, equal, k, shift):
    torch = torch_mod
    for batch in (ragged, equal):
        bv, ov = bases_view(torch, batch.bases, shift), offsets_view(torch, batch.offsets)
        fwd = Fenced(torch, batch.total, torch.int64)
        rev = Fenced(torch, batch.total, torch.int64, align=8)
        valid = Fenced(torch, batch.total, torch.uint8, align=shift)
        ctx.kmers(bv, ov, batch.n, k, fwd.t, rev.t, valid.t)
        _sync(torch)
        for f, what in ((fwd, "fwd"), (rev, "rev"), (valid, "valid")):
            f.check(what)
        wf, wr, we = oracle_kmers(oracle, batch, k)
        idx = np.flatnonzero(valid.np(np.uint8))
        assert np.array_equal(idx, we), (k, shift, batch.n)
        assert np.array_equal(fwd.np(np.uint64)[idx], wf) and np.array_equal(rev.np(np.uint64)[idx], wr), (k, shift)


def _oligo_check(torch, ctx, oracle, batch, bv, ov, k, count_min, tag):
    from kmertools_amd import device
    bins = device.bins(k, count_min)
    for dt, tdt, npdt, norm in (("f64", torch.float64, np.uint64, True), ("f32", torch.float32, np.float32, True),
                                ("u32", torch.int32, np.uint32, False)):
        out = Fenced(torch, (batch.n, bins), tdt, align=16 if dt == "f32" else 0)
        ctx.oligo(bv, ov, batch.n, k, out.t, count_min, norm, 1, dt)
        _sync(torch)
        out.check((tag, dt))
        want = oracle_oligo(oracle, batch, k, count_min, norm)
        got = out.np(npdt)
        if dt == "f64":
            assert np.array_equal(got, want.view(np.uint64)), (tag, dt)
        elif dt == "f32":
            assert np.max(np.abs(got.astype(np.float64) - want), initial=0.0) <= 1e-6, (tag, dt)
        else:
            assert np.array_equal(got.astype(np.float64), want), (tag, dt)


def _head(batch, n):
    """the first n reads (rows of 4^9 / 2 bins: a few dozen reads are enough)"""
    return memo(("head", batch.name, n), lambda: Batch("%s[:%d]" % (batch.name, n), batch.seqs[:n]))


@pytest.mark.parametrize("shift", SHIFTS)
@pytest.mark.parametrize("k", [3, 4, 7, 1, 2, 9])
def test_oligo_from_views(torch_mod, ctx, oracle, ragged, equal, k, shift):
    """the LDS kernel (k 3..7: 16-byte loads rounded down from the address, guarded at the batch's ends) and the generic
    path (k 1, 2, 9), canonical and raw, every dtype, ragged tiles and equal-length (non-general) tiles"""
    torch = torch_mod
    for batch in ((ragged, equal) if k < 8 else (_head(ragged, 80), _head(equal, 81))):
        bv, ov = bases_view(torch, batch.bases, shift), offsets_view(torch, batch.offsets)
        for count_min in ((True, False) if k <= 4 else (True,)):
            _oligo_check(torch, ctx, oracle, batch, bv, ov, k, count_min, (k, shift, batch.n, count_min))


@pytest.mark.parametrize("shift", SHIFTS)
def test_oligo_k7_without_producer_wave_from_views(torch_mod, oracle, monkeypatch, ragged, equal, shift):
    torch = torch_mod
    from kmertools_amd import device
    monkeypatch.setenv("KT_OLIGO_PW", "8")          # read once per context
    c = device.Context(0, stream=torch.cuda.current_stream().cuda_stream)
    try:
        for batch in (ragged, equal):
            bv, ov = bases_view(torch, batch.bases, shift), offsets_view(torch, batch.offsets)
            _oligo_check(torch, c, oracle, batch, bv, ov, 7, True, (shift, batch.n, "pw8"))
    finally:
        c.close()


@pytest.mark.parametrize("k", [4, 9])
def test_oligo_output_alignment(torch_mod, ctx, oracle, equal, k):
    """a device output at 8 mod 16 is refused and left untouched; one at 16 mod 256 works"""
    torch = torch_mod
    from kmertools_amd import _lib, device
    bins = device.bins(k, True)
    bv, ov = bases_view(torch, equal.bases, 5), offsets_view(torch, equal.offsets)
    bad = Fenced(torch, (equal.n, bins), torch.float64, align=8)
    with pytest.raises(_lib.KmertoolsError) as ei:
        ctx.oligo(bv, ov, equal.n, k, bad.t)
    assert ei.value.code == _lib.KT_ERR_ARG
    _sync(torch)
    bad.check()
    assert (bad.raw[bad.lo:bad.hi].cpu().numpy() == GUARD).all()
    good = Fenced(torch, (equal.n, bins), torch.float64, align=16)
    ctx.oligo(bv, ov, equal.n, k, good.t)
    _sync(torch)
    good.check()
    assert np.array_equal(good.np(np.uint64), oracle_oligo(oracle, equal, k, True, True).view(np.uint64))


_CTR_ENV = {"probe": {"KT_BULK_MIN_BASES": str(1 << 40)},
            "packed": {"KT_BULK_MIN_BASES": "0", "KT_BULK_PACK": "1"},
            "staged": {"KT_BULK_MIN_BASES": "0", "KT_BULK_PACK": "0"},
            "direct": {"KT_BULK_MIN_BASES": "0"},
            "target": {"KT_BULK_MIN_BASES": "0"}}


@pytest.mark.parametrize("shift", CTR_SHIFTS)
@pytest.mark.parametrize("form,k", [("probe", 15), ("probe", 31), ("packed", 15), ("packed", 31), ("staged", 15),
                                    ("staged", 31), ("direct", 12), ("target", 15), ("target", 31)])
def test_ctr_add_reads_from_views(torch_mod, ctx, oracle, monkeypatch, ragged, form, k, shift):
    """the probing path, the bulk build over packed reads (the pack pass: request_ahead) and over staged reads (level 1:
    prefetch_issue), the direct 4^k table, an export target: the oracle's table; a second add from a differently shifted
    view doubles it"""
    torch = torch_mod
    from kmertools_amd import device
    for name, val in _CTR_ENV[form].items():
        monkeypatch.setenv(name, val)
    wk, wc = oracle_table(oracle, ragged, k)
    ov = offsets_view(torch, ragged.offsets)
    ctr = device.Counter(ctx, k, 4 ** k if form == "direct" else 1 << 20)
    xk = xc = None
    if form == "target":
        room = len(wk) + 5
        xk, xc = Fenced(torch, room, torch.int64), Fenced(torch, room, torch.int32, align=8)
        ctr.export_target(xk.t, xc.t, room)
    ctr.add_reads(bases_view(torch, ragged.bases, shift), ov, ragged.n)
    if form == "target":
        d = ctr.size()
        assert ctr.export(xk.t, xc.t, len(wk) + 5) == d
        xk.check("target keys")
        xc.check("target counts")
        gk, gc = sort_pairs(xk.np(np.uint64)[:d], xc.np(np.uint32)[:d])
    else:
        gk, gc = ctr.export_host()
    assert np.array_equal(gk, wk) and np.array_equal(gc, wc), (form, k, shift)
    shift2 = (7 * shift + 3) % 32
    ctr.add_reads(bases_view(torch, ragged.bases, shift2, seed=1), ov, ragged.n)
    gk, gc = ctr.export_host()
    if form == "target":
        xk.check("target keys, second add")
        xc.check("target counts, second add")
    assert np.array_equal(gk, wk) and np.array_equal(gc, 2 * wc), (form, k, shift, shift2)
    ctr.close()


@pytest.mark.parametrize("shift", CTR_SHIFTS)
@pytest.mark.parametrize("bulk", ["0", str(1 << 40)])
def test_ctr_add_reads_part_from_views(torch_mod, ctx, oracle, monkeypatch, ragged, bulk, shift):
    torch = torch_mod
    from kmertools_amd import device
    monkeypatch.setenv("KT_BULK_MIN_BASES", bulk)
    k = 31
    wk, wc = oracle_table(oracle, ragged, k)
    bv, ov = bases_view(torch, ragged.bases, shift), offsets_view(torch, ragged.offsets)
    ks, cs = [], []
    ctr = device.Counter(ctx, k, 1 << 19)
    for part in range(3):
        ctr.clear()
        ctr.add_reads_part(bv, ov, ragged.n, 3, part)
        pk, pc = ctr.export_host()
        assert all(device.owner_of(int(x), 3) == part for x in pk[:200])
        ks.append(pk)
        cs.append(pc)
    ctr.close()
    gk, gc = sort_pairs(np.concatenate(ks), np.concatenate(cs))
    assert np.array_equal(gk, wk) and np.array_equal(gc, wc), shift


@pytest.mark.parametrize("shift", SHIFTS)
def test_route_from_views(torch_mod, ctx, oracle, ragged, shift):
    torch = torch_mod
    from kmertools_amd import device
    k, n_owners = 31, 3
    bv, ov = bases_view(torch, ragged.bases, shift), offsets_view(torch, ragged.offsets)
    keys = Fenced(torch, ragged.total, torch.int64, align=8)
    counts = Fenced(torch, n_owners, torch.int64, align=8)
    ctx.route(bv, ov, ragged.n, k, n_owners, keys.t, counts.t)
    _sync(torch)
    keys.check("keys_out")
    counts.check("owner_counts")
    wf, wr, _ = oracle_kmers(oracle, ragged, k)
    canon = np.minimum(wf, wr)
    cnt = counts.np(np.uint64)
    assert int(cnt.sum()) == len(canon)
    got = keys.np(np.uint64)[:len(canon)]
    assert np.array_equal(np.sort(got), np.sort(canon))
    start = 0
    for o in range(n_owners):
        grp = got[start:start + int(cnt[o])]
        assert {device.owner_of(int(x), n_owners) for x in grp[:: max(1, len(grp) // 1500)]} <= {o}
        start += int(cnt[o])


@pytest.mark.parametrize("shift", CTR_SHIFTS)
@pytest.mark.parametrize("owners", [3, 8])
def test_sharded_route_pass_from_views(torch_mod, ctx, oracle, monkeypatch, ragged, owners, shift):
    """one rank routing into several owners' regions (the route pass reads the halo through request_ahead), the regions
    counted: the oracle's table, then doubled by a batch from another shift"""
    torch = torch_mod
    from kmertools_amd import device
    monkeypatch.setenv("KT_SHARD_FORCE", str(owners))
    monkeypatch.setenv("KT_BULK_MIN_BASES", "0")
    k = 31
    wk, wc = oracle_table(oracle, ragged, k)
    ov = offsets_view(torch, ragged.offsets)
    sh = device.Sharded(ctx, k, 1 << 20, ragged.total, 1, 0, None)
    try:
        sh.add_reads(bases_view(torch, ragged.bases, shift), ov, ragged.n)
        sh.finalize()
        gk, gc = sh.table.export_host()
        assert np.array_equal(gk, wk) and np.array_equal(gc, wc), (owners, shift)
        sh.add_reads(bases_view(torch, ragged.bases, (shift + 17) % 32, seed=2), ov, ragged.n)
        sh.finalize()
        gk, gc = sh.table.export_host()
        assert np.array_equal(gk, wk) and np.array_equal(gc, 2 * wc), (owners, shift)
    finally:
        sh.close()


@pytest.fixture(scope="module")
def cov_table(ctx, oracle, ragged):
    """k = 21 table of the aligned reads (host mode) and the oracle's coverage rows of the same reads"""
    from kmertools_amd import device
    k = 21
    ctr = device.Counter(ctx, k, 1 << 20)
    ctr.add_reads_host(ragged.bases, ragged.offsets)
    oc = oracle.Counter(1)
    oc.add_reads(ragged.bases, ragged.offsets, k)
    want = {norm: oc.cov_batch(ragged.bases, ragged.offsets, k, 2, 9, norm) for norm in (True, False)}
    yield ctr, want
    ctr.close()


@pytest.mark.parametrize("shift", SHIFTS)
def test_cov_from_views(torch_mod, ctx, cov_table, ragged, shift):
    torch = torch_mod
    ctr, want = cov_table
    bv, ov = bases_view(torch, ragged.bases, shift), offsets_view(torch, ragged.offsets)
    for dt, tdt, npdt, norm in (("f64", torch.float64, np.uint64, True), ("f32", torch.float32, np.float32, True),
                                ("u32", torch.int32, np.uint32, False)):
        out = Fenced(torch, (ragged.n, 9), tdt)
        ctr.cov(bv, ov, ragged.n, 2, 9, out.t, norm, dt)
        _sync(torch)
        out.check(dt)
        got = out.np(npdt)
        if dt == "f64":
            assert np.array_equal(got, want[True].view(np.uint64)), shift
        elif dt == "f32":
            assert np.max(np.abs(got.astype(np.float64) - want[True])) <= 1e-6, shift
        else:
            assert np.array_equal(got.astype(np.float64), want[False]), shift


@pytest.mark.parametrize("shift", CTR_SHIFTS)
def test_cov_part_from_views_adds_into_prefilled_rows(torch_mod, ctx, oracle, ragged, shift):
    """kt_cov_batch_part over 3 hash partitions, device and host rows, each pre-filled: rows = prefill + the whole table's
    raw rows"""
    torch = torch_mod
    from kmertools_amd import device
    from kmertools_amd._lib import KT_MEM_HOST
    k, parts = 15, 3
    oc = oracle.Counter(1)
    oc.add_reads(ragged.bases, ragged.offsets, k)
    want = oc.cov_batch(ragged.bases, ragged.offsets, k, 3, 7, False).astype(np.uint32)
    pre = np.random.default_rng(shift).integers(0, 1000, size=(ragged.n, 7)).astype(np.uint32)
    bv, ov = bases_view(torch, ragged.bases, shift), offsets_view(torch, ragged.offsets)
    hb = host_bases_view(ragged.bases, shift)
    dev = Fenced(torch, (ragged.n, 7), torch.int32, align=8, prefill=torch.from_numpy(pre.view(np.int32)))
    host = HostFenced((ragged.n, 7), np.uint32, prefill=pre)
    for part in range(parts):
        ctr = device.Counter(ctx, k, 1 << 18)
        ctr.add_reads_host(ragged.bases, ragged.offsets, parts, part)
        ctr.cov_part(bv, ov, ragged.n, 3, 7, dev.t, parts, part)
        ctr.cov_part(hb, ragged.offsets, ragged.n, 3, 7, host.a, parts, part, mem=KT_MEM_HOST)
        _sync(torch)
        ctr.close()
    dev.check("device rows")
    host.check("host rows")
    assert np.array_equal(dev.np(np.uint32), pre + want), shift
    assert np.array_equal(host.a, pre + want), shift


def _want_solidity(oracle, batch, k, keys, counts, lo, hi):
    """the definition of kt_ctr_read_solidity restated over the oracle's k-mers and table (as test_read_filter.py)"""
    out = []
    for s in batch.seqs:
        f, r, end = oracle.kmers(s, k)
        if not len(f):
            out.append((0, 0, U32_MAX))
            continue
        c = np.minimum(f, r)
        i = np.minimum(np.searchsorted(keys, c), len(keys) - 1)
        cnt = np.where(keys[i] == c, counts[i], 0)
        solid = (cnt >= lo) & (cnt <= hi)
        weak = np.flatnonzero(~solid)
        out.append((len(f), int(solid.sum()), int(end[weak[0]]) - k + 1 if len(weak) else U32_MAX))
    a = np.array(out, np.uint64)
    return a[:, 0].astype(np.uint32), a[:, 1].astype(np.uint32), a[:, 2].astype(np.uint32)


@pytest.mark.parametrize("shift", SHIFTS)
def test_read_solidity_from_views(torch_mod, ctx, oracle, ragged, shift):
    """n_kmers / n_solid are added into pre-filled arrays, first_weak is a min with its prefill; with and without
    first_weak; device arrays and host arrays, all fenced"""
    torch = torch_mod
    from kmertools_amd import device
    from kmertools_amd._lib import KT_MEM_HOST
    k, lo, hi = 21, 2, U32_MAX
    half = Batch("half", ragged.seqs[: ragged.n // 2] + ragged.seqs[ragged.n // 3:])  # repeats: counts > 1
    wk, wc = oracle_table(oracle, half, k)
    ctr = device.Counter(ctx, k, 1 << 20)
    ctr.add_reads_host(half.bases, half.offsets)
    wn, ws, ww = memo(("solid", k), lambda: _want_solidity(oracle, ragged, k, wk, wc, lo, hi))
    rng = np.random.default_rng(shift)
    pn = rng.integers(0, 1 << 20, size=ragged.n).astype(np.uint32)
    ps = rng.integers(0, 1 << 20, size=ragged.n).astype(np.uint32)
    pw = np.where(rng.random(ragged.n) < 0.2, rng.integers(0, 50, size=ragged.n), U32_MAX).astype(np.uint32)
    bv, ov = bases_view(torch, ragged.bases, shift), offsets_view(torch, ragged.offsets)
    for first in (True, False):
        nk = Fenced(torch, ragged.n, torch.int32, prefill=torch.from_numpy(pn.view(np.int32)))
        ns = Fenced(torch, ragged.n, torch.int32, align=8, prefill=torch.from_numpy(ps.view(np.int32)))
        fw = Fenced(torch, ragged.n, torch.int32, align=4, prefill=torch.from_numpy(pw.view(np.int32)))
        ctr.read_solidity(bv, ov, ragged.n, lo, hi, nk.t, ns.t, fw.t if first else None)
        _sync(torch)
        for f, what in ((nk, "n_kmers"), (ns, "n_solid"), (fw, "first_weak")):
            f.check((what, first))
        assert np.array_equal(nk.np(np.uint32), pn + wn) and np.array_equal(ns.np(np.uint32), ps + ws), (shift, first)
        assert np.array_equal(fw.np(np.uint32), np.minimum(pw, ww) if first else pw), (shift, first)
    hb = host_bases_view(ragged.bases, shift)
    hn, hs, hw = HostFenced(ragged.n, np.uint32, prefill=pn), HostFenced(ragged.n, np.uint32, prefill=ps), \
        HostFenced(ragged.n, np.uint32, prefill=pw)
    ctr.read_solidity(hb, ragged.offsets, ragged.n, lo, hi, hn.a, hs.a, hw.a, KT_MEM_HOST)
    for f, what in ((hn, "n_kmers"), (hs, "n_solid"), (hw, "first_weak")):
        f.check(("host", what))
    assert np.array_equal(hn.a, pn + wn) and np.array_equal(hs.a, ps + ws) and np.array_equal(hw.a, np.minimum(pw, ww))
    ctr.close()


@pytest.fixture(scope="module")
def cgr_batch():
    rng = np.random.default_rng(0xc64)
    alpha = np.frombuffer(b"ACGTUacgtu", np.uint8)
    lens = list(rng.integers(0, 400, size=300)) + [0, 1, 9000, 8193, 17]
    return Batch("cgr", [alpha[rng.integers(0, 10, size=L)].tobytes() for L in lens])


@pytest.mark.parametrize("shift", SHIFTS)
def test_cgr_from_views(torch_mod, ctx, oracle, cgr_batch, shift):
    torch = torch_mod
    b = cgr_batch
    want = memo(("cgr",), lambda: oracle.cgr_batch(b.bases, b.offsets, 1).copy())
    bv, ov = bases_view(torch, b.bases, shift), offsets_view(torch, b.offsets)
    xy = Fenced(torch, (b.total, 2), torch.float64)
    bad = Fenced(torch, 1, torch.int64, align=8)
    ctx.cgr(bv, ov, b.n, 1, xy.t, bad.t)
    _sync(torch)
    xy.check("xy")
    bad.check("bad_pos")
    assert int(bad.np(np.uint64)[0]) == 2 ** 64 - 1
    assert np.array_equal(xy.np(np.uint64), want.view(np.uint64)), shift
    pos = int(b.offsets[-4]) + 4321                   # inside the 9000-base read
    bv[pos] = ord("N")
    bv[pos + 100] = ord("x")
    ctx.cgr(bv, ov, b.n, 1, xy.t, bad.t)
    _sync(torch)
    xy.check("xy, bad byte")
    bad.check("bad_pos, bad byte")
    assert int(bad.np(np.uint64)[0]) == pos


def _oracle_min(oracle, batch, w, m):
    return memo(("min", batch.name, w, m), lambda: [oracle.minimisers(s, w, m) for s in batch.seqs])


@pytest.mark.parametrize("shift", SHIFTS)
@pytest.mark.parametrize("w,m", [(31, 7), (0, 10), (5000, 7)])
def test_minimisers_from_views(torch_mod, ctx, oracle, ragged, equal, w, m, shift):
    torch = torch_mod
    batches = (ragged, equal) if w else (memo(("min0", m), lambda: Batch("ragged>=%d" % m, [s for s in ragged.seqs if len(s) >= m])), equal)
    for batch in batches:
        want = _oracle_min(oracle, batch, w, m)
        flat = [t for r in want for t in r]
        bv, ov = bases_view(torch, batch.bases, shift), offsets_view(torch, batch.offsets)
        evo = Fenced(torch, batch.n + 1, torch.int64, align=8)
        cnt = ctx.minimisers(bv, ov, batch.n, w, m, evo.t, evo.t, evo.t, evo.t, 0)
        assert cnt == len(flat), (w, m, shift)
        ks = Fenced(torch, cnt, torch.int64, align=8)
        ss = Fenced(torch, cnt, torch.int64)
        es = Fenced(torch, cnt, torch.int64, align=24)
        assert ctx.minimisers(bv, ov, batch.n, w, m, evo.t, ks.t, ss.t, es.t, cnt) == cnt
        for f, what in ((evo, "ev_offsets"), (ks, "kmers"), (ss, "starts"), (es, "ends")):
            f.check(what)
        if cnt:     # (capacity 0 only counts: ev_offsets unspecified)
            assert np.array_equal(evo.np(np.uint64), np.cumsum([0] + [len(r) for r in want]).astype(np.uint64))
        got = list(zip(ks.np(np.uint64).tolist(), ss.np(np.uint64).tolist(), es.np(np.uint64).tolist()))
        assert got == flat, (w, m, shift, batch.n)


@pytest.mark.parametrize("shift", [0, 3, 8])
def test_pairs_and_lookup_at_8_mod_16(torch_mod, ctx, oracle, ragged, shift):
    torch = torch_mod
    from kmertools_amd import device
    k = 31
    wk, wc = oracle_table(oracle, ragged, k)
    raw_k = torch.zeros(len(wk) + 2, dtype=torch.int64, device="cuda")
    raw_k[1:len(wk) + 1] = torch.from_numpy(wk.view(np.int64))
    keys = raw_k[1:len(wk) + 1]
    raw_c = torch.zeros(len(wk) + 4, dtype=torch.int32, device="cuda")
    raw_c[2:len(wk) + 2] = torch.from_numpy(wc.view(np.int32))
    counts = raw_c[2:len(wk) + 2]
    assert keys.data_ptr() % 16 == 8 and counts.data_ptr() % 16 == 8
    ctr = device.Counter(ctx, k, 1 << 20)
    ctr.add_pairs(keys, counts, len(wk))
    ctr.add_pairs(keys, None, len(wk))
    gk, gc = ctr.export_host()
    assert np.array_equal(gk, wk) and np.array_equal(gc, wc + 1)
    rng = np.random.default_rng(shift)
    probe = np.concatenate([wk[::7], rng.integers(0, 1 << 62, size=500, dtype=np.uint64)])
    table = dict(zip(wk.tolist(), (wc + 1).tolist()))
    want = np.array([table.get(int(x), 0) for x in probe], np.uint32)
    raw_p = torch.zeros(len(probe) + 2, dtype=torch.int64, device="cuda")
    raw_p[1:len(probe) + 1] = torch.from_numpy(probe.view(np.int64))
    out = Fenced(torch, len(probe), torch.int32, align=8 + shift * 4)
    ctr.lookup(raw_p[1:len(probe) + 1], len(probe), out.t)
    _sync(torch)
    out.check("lookup counts")
    assert np.array_equal(out.np(np.uint32), want)
    ctr.close()


@pytest.mark.parametrize("shift", SHIFTS)
@pytest.mark.parametrize("noise,genome", [(True, 0), (False, 5000)])
def test_synth_into_views(torch_mod, ctx, oracle, noise, genome, shift):
    torch = torch_mod
    n, L, seed = 333, 150, 0x6b6d + shift
    bases = Fenced(torch, n * L, torch.uint8, align=shift)
    offs = Fenced(torch, n + 1, torch.int64, align=8)
    ctx.synth_reads(seed, n, L, bases.t, offs.t, noise=noise, genome_len=genome, first_read=77)
    _sync(torch)
    bases.check("bases")
    offs.check("offsets")
    want, woff = oracle.synth_reads(seed, n, L, noise=noise, genome_len=genome, first_read=77)
    assert np.array_equal(bases.np(np.uint8), want)
    assert np.array_equal(offs.np(np.uint64), woff)


# ---- 2. fenced partial writes and outputs added into ----------------------------------------------------------------

def _export_raw(ctr, keys, counts, max_out, mem):
    from kmertools_amd import _lib, device
    n = C.c_uint64()
    rc = _lib.lib().kt_ctr_export(ctr._h, device._ptr(keys), device._ptr(counts), int(max_out), C.byref(n), mem)
    return rc, n.value


@pytest.mark.parametrize("bulk", ["0", str(1 << 40)])      # a dense (range-built) table / a probing table
def test_ctr_export_into_fewer_slots(torch_mod, ctx, oracle, monkeypatch, ragged, bulk):
    """kt_ctr_export with max_out = size - 7: max_out distinct pairs with the oracle's counts, KT_ERR_ARG, nothing past
    max_out - into device and into host arrays"""
    torch = torch_mod
    from kmertools_amd import _lib, device
    monkeypatch.setenv("KT_BULK_MIN_BASES", bulk)
    k = 31
    wk, wc = oracle_table(oracle, ragged, k)
    table = dict(zip(wk.tolist(), wc.tolist()))
    ctr = device.Counter(ctx, k, 1 << 20)
    ctr.add_reads(bases_view(torch, ragged.bases, 3), offsets_view(torch, ragged.offsets), ragged.n)
    size = ctr.size()
    assert size == len(wk)
    m = size - 7
    dk, dc = Fenced(torch, m, torch.int64), Fenced(torch, m, torch.int32, align=8)
    rc, n = _export_raw(ctr, dk.t, dc.t, m, _lib.KT_MEM_DEVICE)
    dk.check("device keys")
    dc.check("device counts")
    hk, hc = HostFenced(m, np.uint64), HostFenced(m, np.uint32)
    rc2, n2 = _export_raw(ctr, hk.a, hc.a, m, _lib.KT_MEM_HOST)
    hk.check("host keys")
    hc.check("host counts")
    for rc_, n_, keys, counts in ((rc, n, dk.np(np.uint64), dc.np(np.uint32)), (rc2, n2, hk.a, hc.a)):
        assert rc_ == _lib.KT_ERR_ARG and n_ == m
        assert len(np.unique(keys)) == m
        assert all(table.get(int(a), -1) == int(b) for a, b in zip(keys, counts))
    gk, gc = ctr.export_host()
    assert np.array_equal(gk, wk) and np.array_equal(gc, wc)
    ctr.close()


@pytest.mark.parametrize("k", [15, 31])
def test_ctr_export_target_too_small(torch_mod, ctx, oracle, monkeypatch, ragged, k):
    torch = torch_mod
    from kmertools_amd import _lib, device
    monkeypatch.setenv("KT_BULK_MIN_BASES", "0")
    wk, wc = oracle_table(oracle, ragged, k)
    ov = offsets_view(torch, ragged.offsets)
    for small in (len(wk) // 2, len(wk) - 1):
        sk, sc = Fenced(torch, small, torch.int64), Fenced(torch, small, torch.int32, align=8)
        ctr = device.Counter(ctx, k, 1 << 20)
        ctr.export_target(sk.t, sc.t, small)
        with pytest.raises(_lib.KmertoolsError) as ei:
            ctr.add_reads(bases_view(torch, ragged.bases, 1), ov, ragged.n)
        assert ei.value.code == _lib.KT_ERR_ARG
        _sync(torch)
        sk.check(("target keys", small))
        sc.check(("target counts", small))
        assert ctr.size() == len(wk)
        ctr.export_target(None, None, 0)
        gk, gc = ctr.export_host()
        assert np.array_equal(gk, wk) and np.array_equal(gc, wc)
        ctr.close()


def test_minimisers_beyond_capacity(torch_mod, ctx, oracle, ragged):
    """0 < capacity < n_events: KT_ERR_ARG, the first `capacity` triples in iterator order, nothing past them"""
    torch = torch_mod
    from kmertools_amd import _lib, device
    w, m = 31, 7
    flat = [t for r in _oracle_min(oracle, ragged, w, m) for t in r]
    bv, ov = bases_view(torch, ragged.bases, 1), offsets_view(torch, ragged.offsets)
    for cap in (1, 1000, len(flat) // 2, len(flat) - 1):
        evo = Fenced(torch, ragged.n + 1, torch.int64)
        ks, ss, es = Fenced(torch, cap, torch.int64), Fenced(torch, cap, torch.int64, align=8), Fenced(torch, cap, torch.int64)
        n = C.c_uint64()
        rc = _lib.lib().kt_minimisers(ctx._h, device._ptr(bv), device._ptr(ov), ragged.n, w, m, device._ptr(evo.t),
                                      device._ptr(ks.t), device._ptr(ss.t), device._ptr(es.t), cap, C.byref(n),
                                      _lib.KT_MEM_DEVICE)
        _sync(torch)
        for f, what in ((evo, "ev_offsets"), (ks, "kmers"), (ss, "starts"), (es, "ends")):
            f.check((what, cap))
        assert rc == _lib.KT_ERR_ARG and n.value == len(flat), cap
        got = list(zip(ks.np(np.uint64).tolist(), ss.np(np.uint64).tolist(), es.np(np.uint64).tolist()))
        assert got == flat[:cap], cap


@pytest.fixture(scope="module")
def heavy_tables(ctx, oracle, ragged):
    """two k = 15 tables: the ragged reads plus a poly-A read (one k-mer seen 5986 times: past any LDS bin) / every other
    read of them plus repeats; their oracle tables"""
    from kmertools_amd import device
    k = 15
    a = Batch("heavy_a", ragged.seqs + [b"A" * 6000, b"ACGT" * 300])
    b = Batch("heavy_b", ragged.seqs[::2] + ragged.seqs[5:40] + [b"A" * 100])
    out = []
    for batch in (a, b):
        ctr = device.Counter(ctx, k, 1 << 20)
        ctr.add_reads_host(batch.bases, batch.offsets)
        out.append((ctr, oracle_table(oracle, batch, k)))
    yield out
    for ctr, _ in out:
        ctr.close()


def _want_spectrum(counts, n_bins):
    h = np.bincount(np.minimum(counts, n_bins - 1), minlength=n_bins).astype(np.uint64)
    h[0] = 0
    return h, np.array([len(counts), int(counts.astype(np.uint64).sum())], np.uint64)


@pytest.mark.parametrize("n_bins", [5000, 4097, 64, 2])
def test_spectrum_into_fenced_prefilled(torch_mod, ctx, heavy_tables, n_bins):
    """kt_ctr_spectrum adds into hist / totals: body = prefill + expected, hist[0] keeps its prefill, device and host;
    with n_bins above the LDS bins the saturating bin comes from the global tier"""
    torch = torch_mod
    from kmertools_amd._lib import KT_MEM_HOST
    ctr, (wk, wc) = heavy_tables[0]
    assert wc.max() >= 5000
    want, wtot = _want_spectrum(wc, n_bins)
    rng = np.random.default_rng(n_bins)
    pre = rng.integers(0, 1 << 40, size=n_bins).astype(np.uint64)
    ptot = rng.integers(0, 1 << 40, size=2).astype(np.uint64)
    hist = Fenced(torch, n_bins, torch.int64, prefill=torch.from_numpy(pre.view(np.int64)))
    tot = Fenced(torch, 2, torch.int64, align=8, prefill=torch.from_numpy(ptot.view(np.int64)))
    ctr.spectrum_into(hist.t, n_bins, tot.t)
    _sync(torch)
    hist.check("device hist")
    tot.check("device totals")
    assert np.array_equal(hist.np(np.uint64), pre + want) and np.array_equal(tot.np(np.uint64), ptot + wtot)
    hh, ht = HostFenced(n_bins, np.uint64, prefill=pre), HostFenced(2, np.uint64, prefill=ptot)
    ctr.spectrum_into(hh.a, n_bins, ht.a, KT_MEM_HOST)
    hh.check("host hist")
    ht.check("host totals")
    assert np.array_equal(hh.a, pre + want) and np.array_equal(ht.a, ptot + wtot)


@pytest.mark.parametrize("n_rows,n_cols", [(5000, 3), (17, 9), (2, 4097)])
def test_compare_into_fenced_prefilled(torch_mod, ctx, heavy_tables, n_rows, n_cols):
    torch = torch_mod
    from kmertools_amd._lib import KT_MEM_HOST
    (ca, (ak, ac)), (cb, (bk, bc)) = heavy_tables
    keys = np.union1d(ak, bk)
    va = np.zeros(len(keys), np.uint64)
    vb = np.zeros(len(keys), np.uint64)
    va[np.searchsorted(keys, ak)] = ac
    vb[np.searchsorted(keys, bk)] = bc
    want = np.zeros((n_rows, n_cols), np.uint64)
    np.add.at(want, (np.minimum(va, n_rows - 1).astype(np.int64), np.minimum(vb, n_cols - 1).astype(np.int64)), 1)
    want[0, 0] = 0
    shared = (va > 0) & (vb > 0)
    wtot = np.array([len(ak), len(bk), int(shared.sum()), int(va.sum()), int(vb.sum()),
                     int(np.minimum(va, vb)[shared].sum())], np.uint64)
    rng = np.random.default_rng(n_rows * n_cols)
    pre = rng.integers(0, 1 << 40, size=(n_rows, n_cols)).astype(np.uint64)
    ptot = rng.integers(0, 1 << 40, size=6).astype(np.uint64)
    m = Fenced(torch, (n_rows, n_cols), torch.int64, align=8, prefill=torch.from_numpy(pre.view(np.int64)))
    tot = Fenced(torch, 6, torch.int64, prefill=torch.from_numpy(ptot.view(np.int64)))
    ca.compare_into(cb, m.t, n_rows, n_cols, tot.t)
    _sync(torch)
    m.check("device matrix")
    tot.check("device totals")
    assert np.array_equal(m.np(np.uint64), pre + want) and np.array_equal(tot.np(np.uint64), ptot + wtot)
    hm, ht = HostFenced((n_rows, n_cols), np.uint64, prefill=pre), HostFenced(6, np.uint64, prefill=ptot)
    ca.compare_into(cb, hm.a, n_rows, n_cols, ht.a, KT_MEM_HOST)
    hm.check("host matrix")
    ht.check("host totals")
    assert np.array_equal(hm.a, pre + want) and np.array_equal(ht.a, ptot + wtot)


# ---- 3. slab boundaries of the oligo paths ----------------------------------------------------------------------------

def test_oligo_host_slabs(hctx, oracle):
    """host mode, k = 7 canonical: f64 rows come in slabs of 16 384 reads, u32 rows in slabs of 32 768; reads of unusual
    length (empty, shorter than k, longer than a 1008-base chunk) on both sides of every boundary; compared in chunks"""
    from kmertools_amd import device
    k, n = 7, 40_000
    rng = np.random.default_rng(0x51ab)
    lens = rng.integers(0, 400, size=n)
    for b in (16_384, 32_768):
        lens[b - 3:b + 3] = (1500, 0, 5, 0, 2100, 3)
    bases = ACGT[rng.integers(0, 4, size=int(lens.sum()))].copy()
    m = rng.random(len(bases))
    bases[m < 0.01] = ord("N")
    bases[(m > 0.01) & (m < 0.03)] |= 0x20
    offsets = np.zeros(n + 1, np.uint64)
    offsets[1:] = np.cumsum(lens)
    hb = host_bases_view(bases, 3)
    for dt, norm in (("u32", False), ("f64", True)):
        got = hctx.oligo_host(hb, offsets, k, True, norm, 1, dt)
        for r0 in range(0, n, 4096):
            r1 = min(n, r0 + 4096)
            o = offsets[r0:r1 + 1] - offsets[r0]
            want = oracle.oligo_batch(bases[int(offsets[r0]):int(offsets[r1])], o, k, True, norm, 1.0, threads=8)
            if dt == "f64":
                assert np.array_equal(got[r0:r1].view(np.uint64), want.view(np.uint64)), (dt, r0)
            else:
                assert np.array_equal(got[r0:r1].astype(np.float64), want), (dt, r0)
        del got


def _generic_slab_batch(seed, n, slab, short, long_):
    """reads of up to `short` bases in the first slab, of `long_` in the second (more bases than the first: the scratch of
    the segment arguments grows mid-call), mixed after that"""
    rng = np.random.default_rng(seed)
    alpha = np.frombuffer(b"ACGTNacgt", np.uint8)
    lens = np.concatenate([rng.integers(0, short, size=slab), rng.integers(long_ // 2, long_, size=slab),
                           rng.integers(0, long_, size=n - 2 * slab)])
    lens[[0, slab - 1, slab, 2 * slab - 1, 2 * slab]] = (0, 3, 0, long_ + 1, 1)
    return Batch("slabs%d" % seed, [alpha[rng.choice(9, size=L, p=[.24, .24, .24, .24, .01, .0075, .0075, .0075, .0075])]
                                    .tobytes() for L in lens])


@pytest.mark.parametrize("k,count_min,n,slab,short,long_", [(12, True, 70, 31, 60, 4000), (9, False, 2300, 1024, 40, 700)])
def test_oligo_generic_device_slabs(torch_mod, ctx, oracle, k, count_min, n, slab, short, long_):
    """the generic path (k = 12: 8 390 656 bins, 31 reads per slab; k = 9 raw: 262 144 bins, 1024 per slab) cuts a device
    batch into slabs, each slab's reads at bases + b0 (an odd address here); sparse comparison: the non-zero cells =
    (read, bin, count) of the oracle's k-mers, row sums = k-mer counts, f64 = count / max(1, total)"""
    torch = torch_mod
    from kmertools_amd import device
    bins = device.bins(k, count_min)
    assert (1 << 28) // bins == slab
    batch = _generic_slab_batch(k, n, slab, short, long_)
    first = int(batch.offsets[slab])
    assert int(batch.offsets[2 * slab]) - first > first
    rows, cols, vals, totals = [], [], [], np.zeros(n, np.int64)
    pmap = device.pos_map(k)[0] if count_min else None
    for i, s in enumerate(batch.seqs):
        f, r, _ = oracle.kmers(s, k)
        totals[i] = len(f)
        if not len(f):
            continue
        key = np.minimum(f, r) if count_min else f
        b, c = np.unique(pmap[key] if count_min else key, return_counts=True)
        rows.append(np.full(len(b), i))
        cols.append(b.astype(np.int64))
        vals.append(c)
    rows, cols, vals = np.concatenate(rows), np.concatenate(cols), np.concatenate(vals)
    bv, ov = bases_view(torch, batch.bases, 5), offsets_view(torch, batch.offsets)
    try:
        out = torch.empty((n, bins), dtype=torch.int32, device="cuda")
        ctx.oligo(bv, ov, n, k, out, count_min, False, 1, "u32")
        nzt = torch.nonzero(out)
        got = out[nzt[:, 0], nzt[:, 1]].cpu().numpy()
        nz = nzt.cpu().numpy()
        del nzt
        assert np.array_equal(out.sum(dim=1, dtype=torch.int64).cpu().numpy(), totals)
        del out
        assert np.array_equal(nz[:, 0], rows) and np.array_equal(nz[:, 1], cols) and np.array_equal(got, vals)
        out = torch.empty((n, bins), dtype=torch.float64, device="cuda")
        ctx.oligo(bv, ov, n, k, out, count_min, True, 1, "f64")
        nzt = torch.nonzero(out)
        got = out[nzt[:, 0], nzt[:, 1]].cpu().numpy()
        nz = nzt.cpu().numpy()
        del nzt
        del out
        assert np.array_equal(nz[:, 0], rows) and np.array_equal(nz[:, 1], cols)
        want = vals.astype(np.float64) / np.maximum(1, totals[rows]).astype(np.float64)
        assert np.array_equal(got.view(np.uint64), want.view(np.uint64))
    finally:
        torch.cuda.empty_cache()
