"""Batches of more than 2^32 bases through every kernel that walks reads.

Every entry point that takes a CSR batch promises 64-bit global base indices, and the calls that keep u32 positions refuse
only a READ of 2^32 bases, never a batch of that size - but the largest batch any other test hands a kernel has 3.75 G
bases, 87 % of 2^32.  A `(uint32_t)` on an offset, a 32-bit `blockIdx.x * N` or a `seg * SEG` kept in 32 bits passes all of
them.  Here the batches have 4.3 G bases (tests/big_batches.py: head | ballast | tail, built on the GPU from three small
pieces), and what is expected of a call is what the CPU oracle says of the three pieces alone.  Three guards:

  poison    an output that a call does not write is filled with a pattern first and must still hold it: a truncated OUTPUT
            index writes below 2^32, into what belongs to the head or the ballast;
  content   the reads at and behind base 2^32 (probe B) differ from the bytes 2^32 bases before them (probe A and the
            ballast's first copy; bb.check_plan asserts it): a truncated INPUT index gives B's reads A's answers;
  period    the ballast is one block `copies` times, each copy one read: all its rows, and all its slices of a per-base
            output, equal the first one's (compared on the GPU in chunks), and the first equals the oracle's answer for
            the block - a truncation anywhere in the ballast breaks the period.

Integers and f64 bit-exact, f32 within the 1e-6 of the parity suite.  The plan tests at the top need no GPU.  Every GPU test
works out the bytes it needs and skips, with both numbers in the reason, only when the card has less free; after each test
`big: ...` is printed: its seconds and the device bytes it was seen to use (free memory sampled after the calls).

Left out, and why: a bulk build with `cap1 * ksz() >= 2^31` (paging switched off) under such a batch needs a k = 31 table
of at most 2^21 = 2.10 M slots (kt_bulk_job::plan: B1 <= 16 level-1 buckets, so at most 8 hash bits above the 8192-position
ranges), and the batch has 2.06 M distinct 31-mers: at a load of 98 % the ranges overflow before the case says anything.

Measured on an idle MI355X (35 passed, none skipped, 60 s in all; seconds include the oracle's work on the CPU; GB of
device memory seen in use beside the cached batches of 4.3 GB each):
  oligo k = 4 / 7 / 9, each layout        0.2-0.8 / 0.2-0.5 / 3.3 s    0.02 / 0.5 / 8.9 GB   content, period, poison
  oligo tiles of 2^31 - 16 and 2^31 bases 2.5 / 2.6 s                  2.1 GB                four equal rows, the oracle's sums
  ctr k = 31 / 16 / 9, bulk               1.8 / 2.8 / 0.5 s            91.6 / 48.1 / 46.0 GB content, period (the counts)
       trace: level1=paged level2=fixed build l1=scatter1y l2=fast build=dense, for all three
  ctr k = 31 / 16 / 9, probing            0.5 / 0.5 / 0.4 s            2.2 / 2.2 / 0.04 GB   (no [bulk] line)
  ctr in 3 parts, k = 21                  5.5 s (three bulk builds)    89.2 GB               content, period
  cov, read_solidity                      1.4-1.7, 1.0-1.1 s           0.2 GB                content, period, poison
  profile and stats                       1.9 s                        21.7 GB               poison, content, period
  correct support and apply               3.3 s                        35.2 GB               poison, content, period
  sketch and card                         0.7-1.1 s                    1.3 GB                content, period (sketch), poison
  minimisers (0,15) (31,15) (5000,21)     2.1 / 0.3 / 0.6 s            0.1 / 28.6 / 116.1 GB content, period, poison
  minimisers (5000,21), KT_MIN_SERIAL=1   4.2 s (a thread per read)    38.8 GB               content, period, poison
  kmers k = 31, cgr, route                0.4, 0.5, 0.7 s              73.0, 68.9, 63.1 GB   poison, content, period
  the sharded refusal                     0.1-5.4 s (the pending table of 512 M slots is allocated and freed)
That the guards bite was seen once with a scratch build in which stage_segment (kt_segment.hpp) loads its 32 bases from
`a.bases + (uint32_t)b`: the 14 tests of the calls that stage segments that way failed - the probing counter (1.40 M keys
for 2.06 M), cov, read_solidity, profile ("base 2^32 - 18": the first window that reaches over it), correct_support, sketch
and card (`inside_ballast`: copy 4294 differs from the first), kmers, route - all through the content guard or the period;
the kernels with a front end of their own (the oligo kernels, the bulk build over packed reads, minimisers, cgr) passed."""
import ctypes as C
import gc
import time

import numpy as np
import pytest

import big_batches as bb
import read_batches as rb
import test_read_boundaries as trb
from big_batches import BLOCK, G32

gpu = pytest.mark.gpu

U32_MAX = 0xFFFFFFFF
U64 = np.uint64
P8, P32, P64 = 0xA5, 0xA5A5A5A5, 0xA5A5A5A5A5A5A5A5          # poison
NONE_KMER = 0xFFFFFFFFFFFFFFFF
LOOKUP_K = 21
TABLE_KS = (31, 21, 16, 9)
SLOTS = {31: 1 << 27, 21: 1 << 27, 16: 1 << 27, 9: 1 << 21}
TILE_EDGE = {536_854_524: 0x7FFEFFF0, 536_870_912: 1 << 31}   # read length -> bases of a tile of four such reads


def signed(v, bits):
    return v - (1 << bits) if v >> (bits - 1) else v


def expected_table(oracle, p, k):
    return bb.memo(("table", p.name, k), lambda: bb.merged_table(p, lambda x: oracle.count_reads(x.bases, x.offsets, k)))


# ---- the plans: no GPU -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("layout,letters", [(name, False) for name in bb.LAYOUTS] + [("straddle", True)])
def test_plan_crosses_2_32_where_it_says(layout, letters):
    """bb.check_plan: total > 2^32; the read that holds base 2^32 has 64 bases or more and is a read of B (`straddle`:
    strictly inside it; `aligned`: it starts there) or a ballast read with 64 bases on either side (`inside_ballast`); 1000
    reads of B wholly before and 1000 wholly behind; and no read that reaches a base index >= 2^32 holds the bytes that lie
    2^32 before it - every such read of 16 bases or more differs in more than a quarter of them, all of them together in more
    than 70 % (random bases: 75 %; a read of one or two bases may agree by chance, it holds no k-mer of the k used here
    but those of k = 4, 7, 9, where its row is compared all the same)"""
    p = bb.plan(layout, letters)
    nums = bb.check_plan(p)
    assert len(p.offsets) < 16000 and nums["total"] == int(p.offsets[-1])
    if letters:
        for x in bb.pieces(p):
            assert np.isin(x.bases, rb.LETTERS).all(), x.name
    if layout == "straddle":
        assert p.copies * BLOCK == 4_294_012_882 and G32 - p.copies * BLOCK == 954_414


def test_pieces_are_what_they_are_meant_to_be():
    a, b, s, blk = bb.probe("A"), bb.probe("B"), bb.probe("short_B"), bb.block()
    for x in (a, b, s):
        lens = x.lens
        assert (lens == 0).sum() >= 2 and ((lens > 0) & (lens < 9)).any() and (lens == 9000).any() and (lens == 8192).any(), x.name
        assert (x.bases == ord("N")).sum() > 25 and np.isin(x.bases, np.frombuffer(b"acgt", np.uint8)).any(), x.name
    assert 200 <= a.n <= 400 and 1_900_000 <= b.total <= 2_200_000 and s.n == a.n
    m = min(a.total, b.total, s.total)
    assert (a.bases[:m] != b.bases[:m]).mean() > 0.6 and (a.bases[:m] != s.bases[:m]).mean() > 0.6
    assert blk.n == 1 and blk.total == BLOCK and all(BLOCK % q for q in (2, 3, 5, 7, 16, 1008, 8192))
    assert all((blk.bases == v).sum() > 100 for v in b"NUacgt") and np.isin(blk.bases[bb.CLEAN[0]:bb.CLEAN[1]], rb.VALID).all()


@pytest.mark.parametrize("k", TABLE_KS)
def test_expected_counts_stay_below_the_top_of_u32(oracle, k):
    """the tables are compared with oracle(A) + oracle(B) + copies x oracle(block): no count may saturate"""
    p = bb.plan("straddle")
    keys, counts = expected_table(oracle, p, k)
    assert len(keys) == len(np.unique(keys)) and int(counts.max()) < U32_MAX and int(counts.max()) >= p.copies
    wk, wc = oracle.count_reads(p.block.bases, p.block.offsets, k)
    assert int(counts.sum()) > p.copies * int(wc.sum()) > G32 * 0.7


@pytest.mark.parametrize("L", sorted(TILE_EDGE))
def test_tile_edge_lengths(L):
    """kt_oligo.hip: a tile of equal-length reads takes the 32-bit fast path while its bases TL < 0x7FFF0000"""
    assert 4 * L == TILE_EDGE[L] and trb.oligo_max_R(7, True) == 4
    assert (4 * L < 0x7FFF0000) == (L == min(TILE_EDGE)) and 0x7FFF0000 - 4 * min(TILE_EDGE) == 16
    assert L % BLOCK >= 6 and L // BLOCK >= 536


# ---- the GPU side --------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    return torch


_use = {}


def free_bytes(ctx):
    from kmertools_amd import _lib
    f, t = C.c_uint64(), C.c_uint64()
    _lib.check(_lib.lib().kt_device_memory(ctx._h, C.byref(f), C.byref(t)))
    return f.value


def room(torch, ctx, need, what):
    """skips when `need` bytes are not free on the device; starts the record of what the test uses"""
    gc.collect()
    torch.cuda.empty_cache()
    free = free_bytes(ctx)
    if need > free:
        pytest.skip("%s needs %d bytes of device memory, %d are free" % (what, need, free))
    _use.update(need=int(need), start=free, low=free)


def mark(torch, ctx):
    """after a call: everything has run, and the free memory is sampled (torch's cache and the library's scratch count as used)"""
    torch.cuda.synchronize()
    _use["low"] = min(_use.get("low", 1 << 62), free_bytes(ctx))


@pytest.fixture
def ctx(torch_mod, request):
    """a context per test (its scratch goes with it), on torch's stream"""
    from kmertools_amd import device
    torch = torch_mod
    _use.clear()
    t0 = time.time()
    c = device.Context(0, stream=torch.cuda.current_stream().cuda_stream)
    yield c
    torch.cuda.synchronize()
    c.close()
    gc.collect()
    torch.cuda.empty_cache()
    print("big: %s: %.1f s, %d bytes needed by its own count, %d bytes seen in use" % (
        request.node.name, time.time() - t0, _use.get("need", 0), _use.get("start", 0) - _use.get("low", 0)))


@pytest.fixture(scope="module")
def batches(torch_mod):
    """(layout, letters) -> (plan, bases, offsets): each batch is checked (bb.check_plan) and assembled once"""
    made = {}

    def get(layout, letters=False):
        if (layout, letters) not in made:
            p = bb.plan(layout, letters)
            bb.check_plan(p)
            made[(layout, letters)] = (p,) + bb.assemble(torch_mod, p)
        return made[(layout, letters)]

    yield get
    made.clear()
    gc.collect()
    torch_mod.cuda.empty_cache()


def dev(torch, a):
    a = np.ascontiguousarray(a)
    a = a.view({np.dtype(np.uint64): np.int64, np.dtype(np.uint32): np.int32}.get(a.dtype, a.dtype))
    return torch.from_numpy(a if a.size else np.zeros(1, a.dtype)).cuda()


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({1: np.uint8, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def same_part(got, want, tol):
    """-> indices (first axis) where the device part `got` differs from the numpy array `want`"""
    g = got.cpu().numpy()
    if not len(g):
        return np.zeros(0, np.int64), g
    if tol is None:
        g, w = bits(g), bits(np.asarray(want))
        assert g.dtype == w.dtype and g.size == w.size, (g.dtype, w.dtype, g.shape, w.shape)
        bad = g != w.reshape(g.shape)
    else:
        w = np.asarray(want, np.float64).reshape(g.shape)
        bad = ~(np.abs(g.astype(np.float64) - w) <= tol)          # (a NaN is bad)
    return np.flatnonzero(bad.reshape(len(g), -1).any(axis=1)), g


def check_parts(torch, p, got, sizes, want, tag, tol=None, by_base=False):
    """got: a device tensor whose first axis is head | copies x unit | tail (sizes = (head, unit, tail) entries); want: the
    numpy answers for (head, one unit, tail).  The period on the GPU, the three parts against the oracle's.  by_base: an
    entry is a base (a failure says where it lies relative to base 2^32)"""
    nh, unit, nt = sizes

    def rel(g):
        return ", base 2^32 %+d" % (g - G32) if by_base else ""
    a, b = nh, nh + p.copies * unit
    assert got.shape[0] == b + nt, (tag, got.shape, sizes)
    if unit:
        inner = int(np.prod(got.shape[1:], dtype=np.int64))
        ball = got[a:b].view(p.copies, unit * inner)
        step = max(1, (1 << 27) // (unit * inner))
        for r in range(1, p.copies, step):
            eq = ball[r:r + step] == ball[:1]
            if not bool(eq.all()):
                at = int(torch.nonzero(~eq.reshape(-1))[0])
                c, e = r + at // (unit * inner), at % (unit * inner) // inner
                g = a + c * unit + e
                pytest.fail("%s, %s: copy %d of the ballast differs from the first at its entry %d (entry %d of the whole%s): %s, "
                            "the first copy has %s" % (tag, p.name, c, e, g, rel(g), ball[c, at % (unit * inner)].item(),
                                                       ball[0, at % (unit * inner)].item()))
            del eq
    for name, lo, hi, w in (("head", 0, a, want[0]), ("first copy", a, a + unit, want[1]), ("tail", b, b + nt, want[2])):
        bad, g = same_part(got[lo:hi], w, tol)
        if len(bad):
            i = int(bad[0])
            w = np.asarray(w).reshape((hi - lo,) + g.shape[1:])
            pytest.fail("%s, %s: entry %d (%s entry %d%s) differs, %d of the %s do: got %s, expected %s" % (
                tag, p.name, lo + i, name, i, rel(lo + i), len(bad), name, g[i], w[i]))


def check_rows(torch, p, got, want, tag, tol=None):
    """one row per read"""
    check_parts(torch, p, got, (p.n_head, 1, p.n_tail), want, tag + " (rows by read: 2^32 is in read %d)" % p.read_of(G32), tol)


def check_bases(torch, p, got, want, tag):
    """one entry per base"""
    check_parts(torch, p, got, (p.o_ball, BLOCK, p.tail.total), want, tag + " (by base)", by_base=True)


def assemble_flat(torch, p, parts, dtype):
    """a per-base device array from the three pieces' arrays"""
    out = torch.empty(p.total, dtype=dtype, device="cuda")
    out[:p.o_ball].copy_(dev(torch, parts[0])[:p.o_ball])
    out[p.o_ball:p.o_tail].view(p.copies, BLOCK).copy_(dev(torch, parts[1]))
    out[p.o_tail:].copy_(dev(torch, parts[2]))
    return out


# ---- 1. kt_oligo_batch ---------------------------------------------------------------------------------------------------------------

OLIGO = {4: ("f64", True), 7: ("f32", True), 9: ("u32", False)}     # the LDS kernel, oligo_pw_kernel, kt_oligo_generic


@gpu
@pytest.mark.parametrize("k", sorted(OLIGO))
@pytest.mark.parametrize("layout", bb.LAYOUTS)
def test_oligo(torch_mod, ctx, batches, oracle, layout, k):
    """canonical rows, n_reads x bins: the output is small, the input is not.  Guards: content (B's rows), period (the
    ballast's rows; `inside_ballast`: the equal-length fast path with a tile's first base on both sides of 2^32), poison
    (every row is primed with a value no row holds)"""
    torch = torch_mod
    from kmertools_amd import device
    p, bases, offsets = batches(layout)
    dt, norm = OLIGO[k]
    bins = device.bins(k, True)
    tdt = {"f64": torch.float64, "f32": torch.float32, "u32": torch.int32}[dt]
    room(torch, ctx, p.n * bins * (8 if dt == "f64" else 4) * 3 + (1 << 30), "oligo k = %d" % k)
    out = torch.full((p.n, bins), 0x5A5A5A5A if dt == "u32" else 7.25, dtype=tdt, device="cuda")
    ctx.oligo(bases, offsets, p.n, k, out, True, norm, 1, dt)
    mark(torch, ctx)
    tag = "oligo, k = %d, %s" % (k, dt)
    if k < 9:
        want = tuple(oracle.oligo_batch(x.bases, x.offsets, k, True, True, 1.0, threads=8) for x in bb.pieces(p))
        check_rows(torch, p, out, want, tag, 1e-6 if dt == "f32" else None)
        return
    # rows of 512 KB: the period and the block's row dense, the probes' rows through their non-zero cells
    nh, nc = p.n_head, p.copies
    row = oracle.oligo_batch(p.block.bases, p.block.offsets, k, True, False, 1.0)
    assert row.max() < 2 ** 32
    check_parts(torch, p, out[nh:nh + nc], (0, 1, 0), (np.zeros((0, bins), np.uint32), row.astype(np.uint32), np.zeros((0, bins), np.uint32)), tag)
    for x, first in ((p.head, 0), (p.tail, nh + nc)):
        flat = out[first:first + x.n].reshape(-1)
        nz = torch.nonzero(flat).flatten()
        cells, vals = nz.cpu().numpy(), flat[nz].cpu().numpy().view(np.uint32)
        wcells, wcounts, _ = trb.sparse_rows(oracle, x, k, True)
        j = trb.first_flat_diff((cells, vals), (wcells, wcounts))
        if j is not None:
            cell = min(int(cells[j]) if j < len(cells) else x.n * bins, int(wcells[j]) if j < len(wcells) else x.n * bins)
            i = first + cell // bins
            pytest.fail("%s, %s: read %d (%s; it starts at 2^32 %+d): non-zero cell %d differs (%d found, %d expected), bin %d" % (
                tag, p.name, i, rb.where(x, cell // bins), int(p.offsets[i]) - G32, j, len(cells), len(wcells), cell % bins))


@gpu
@pytest.mark.parametrize("L", sorted(TILE_EDGE))
def test_oligo_tile_at_2_31(torch_mod, ctx, oracle, L):
    """four equal reads, k = 7 canonical (tiles of four reads): 4 L = 0x7FFEFFF0 is the last tile of the 32-bit fast path
    (lr_magic, (uint32_t)t.flat_end, safe_hi at their edge), 4 L = 2^31 the first of the general path (pos0 clamped at
    0x7FFFFFF0).  Every read is the block repeated and cut to length: its counts are the block's times the whole copies,
    the cut tail's, and the k - 1 windows over each seam (the oracle on pieces of 1 Mbase at most).  f32 rows as the CLI
    writes them, and the raw u32 counts, which must be exact."""
    torch = torch_mod
    k, blk = 7, bb.block().bases
    whole, cut = divmod(L, BLOCK)
    assert 4 * L == TILE_EDGE[L] and cut >= k - 1

    def counts(b):
        return oracle.oligo_batch(np.ascontiguousarray(b), np.array([0, len(b)], U64), k, True, False, 1.0)[0]
    seam = np.concatenate([blk[-(k - 1):], blk[:k - 1]])          # 2 k - 2 bases: exactly the k - 1 windows over a seam
    want = whole * counts(blk) + counts(blk[:cut]) + whole * counts(seam)
    assert want.max() < 2 ** 32 and 0.9 * L < want.sum() <= L - k + 1
    room(torch, ctx, 4 * L + 3 * BLOCK + (1 << 30), "oligo at the tile edge")
    dblk = torch.from_numpy(blk).cuda()
    bases = torch.empty(4 * L, dtype=torch.uint8, device="cuda")
    reads = bases.view(4, L)
    reads[0, :whole * BLOCK].view(whole, BLOCK).copy_(dblk)
    reads[0, whole * BLOCK:].copy_(dblk[:cut])
    reads[1:].copy_(reads[:1])
    offsets = dev(torch, (np.arange(5, dtype=np.int64) * L).astype(U64))
    for dt, tdt, fill in (("f32", torch.float32, 7.25), ("u32", torch.int32, 0x5A5A5A5A)):
        out = torch.full((4, len(want)), fill, dtype=tdt, device="cuda")
        ctx.oligo(bases, offsets, 4, k, out, True, dt == "f32", 1, dt)
        mark(torch, ctx)
        g = out.cpu().numpy()
        assert (g == g[0]).all(), ("the four rows differ", L, dt, np.flatnonzero((g != g[0]).any(axis=1)))
        if dt == "u32":
            bad = np.flatnonzero(g[0].view(np.uint32) != want.astype(np.uint32))
            assert not len(bad), (L, dt, bad[:4], g[0].view(np.uint32)[bad[:4]], want[bad[:4]])
        else:
            err = np.abs(g[0].astype(np.float64) - want / want.sum())
            assert np.isfinite(g).all() and err.max() <= 1e-6, (L, dt, int(err.argmax()), err.max())


# ---- 2. counting ----------------------------------------------------------------------------------------------------------------------

def table_mismatch(p, gk, gc, wk, wc):
    if np.array_equal(gk, wk) and np.array_equal(gc.astype(U64), wc):
        return None
    extra, missing = np.setdiff1d(gk, wk), np.setdiff1d(wk, gk)
    if len(extra) or len(missing):
        return "%d keys that no read holds (first %#x), %d keys missing (first %#x)" % (
            len(extra), int(extra[0]) if len(extra) else 0, len(missing), int(missing[0]) if len(missing) else 0)
    bad = np.flatnonzero(gc.astype(U64) != wc)
    return "%d of %d counts differ, first: key %#x has %d, expected %d (%d copies of the block)" % (
        len(bad), len(wk), int(wk[bad[0]]), int(gc[bad[0]]), int(wc[bad[0]]), p.copies)


def bulk_bytes(p, k):
    """what a bulk build of the batch holds beside the table: two key arrays with the paged layout's eighth of slack, the
    packed reads (half a byte per base) and the metadata - measured at 90 GB for 8-byte keys, 46 GB for 4-byte ones"""
    return p.total * (8 if k > 16 else 4) * 5 // 2 + p.total + (4 << 30)


def bulk_lines(capfd):
    return [line for line in capfd.readouterr().err.splitlines() if line.startswith("[bulk]")]


@gpu
@pytest.mark.parametrize("path", ["bulk", "probing"])
@pytest.mark.parametrize("k", [31, 16, 9])
def test_ctr_add_reads(torch_mod, ctx, batches, oracle, monkeypatch, capfd, k, path):
    """the exported table is oracle(A) + oracle(B) + copies x oracle(block), key by key.  Which path ran is read off the
    verbose trace: one [bulk] build line, or none.  Guards: content (a k-mer of B counted as one of A changes two counts),
    period (every count of the block's k-mers is a multiple met exactly)"""
    torch = torch_mod
    from kmertools_amd import device
    p, bases, offsets = batches("straddle")
    monkeypatch.setenv("KT_BULK_VERBOSE", "1")
    monkeypatch.delenv("KT_BULK", raising=False)
    if path == "probing":
        monkeypatch.setenv("KT_BULK_MIN_BASES", str(1 << 40))
    else:
        monkeypatch.delenv("KT_BULK_MIN_BASES", raising=False)
    wk, wc = expected_table(oracle, p, k)
    room(torch, ctx, SLOTS[k] * 16 + (bulk_bytes(p, k) if path == "bulk" else 0) + (2 << 30), "ctr k = %d, %s" % (k, path))
    ctr = device.Counter(ctx, k, SLOTS[k])
    try:
        capfd.readouterr()
        ctr.add_reads(bases, offsets, p.n)
        mark(torch, ctx)
        lines = bulk_lines(capfd)
        if path == "bulk":
            assert len(lines) == 1 and lines[0].split()[5] == "build", lines
            print("big: ctr k = %d: %s" % (k, lines[0]))
        else:
            assert not lines, lines
        assert ctr.size() == len(wk), (k, path, ctr.size(), len(wk))
        gk, gc = ctr.export_host()
        bad = table_mismatch(p, gk, gc, wk, wc)
        assert bad is None, "ctr (%s), k = %d, %s: %s" % (path, k, p.name, bad)
    finally:
        ctr.close()


@gpu
def test_ctr_add_reads_part(torch_mod, ctx, batches, oracle, monkeypatch, capfd):
    """three hash partitions into three tables, k = 21: they share no key and their union is the whole table"""
    torch = torch_mod
    from kmertools_amd import device
    k, parts = LOOKUP_K, 3
    p, bases, offsets = batches("straddle")
    monkeypatch.setenv("KT_BULK_VERBOSE", "1")
    wk, wc = expected_table(oracle, p, k)
    room(torch, ctx, SLOTS[k] * 16 + bulk_bytes(p, k) + (2 << 30), "ctr parts")
    keys, counts, paths = [], [], []
    for part in range(parts):
        ctr = device.Counter(ctx, k, SLOTS[k])
        try:
            capfd.readouterr()
            ctr.add_reads_part(bases, offsets, p.n, parts, part)
            mark(torch, ctx)
            paths.append(bulk_lines(capfd) or "no [bulk] line: the probing path")
            gk, gc = ctr.export_host()
        finally:
            ctr.close()
        assert len(gk) > len(wk) // 6, (part, len(gk))
        keys.append(gk)
        counts.append(gc)
    print("big: ctr in %d parts: %s" % (parts, paths))
    gk, gc = np.concatenate(keys), np.concatenate(counts)
    assert len(np.unique(gk)) == len(gk), "a key in two partitions"
    order = np.argsort(gk, kind="stable")
    bad = table_mismatch(p, gk[order], gc[order], wk, wc)
    assert bad is None, "ctr in %d parts, k = %d, %s: %s" % (parts, k, p.name, bad)


# ---- 3. the calls that look reads up in a table ------------------------------------------------------------------------------------------

def alt_tail(p):
    """the tail with 2 % of its valid bases substituted: what the table is made of, so that the batch's own tail reads
    carry errors against it - weak windows, uncovered bases and a supported candidate at each"""
    import test_correct as tc

    def make():
        rng = np.random.default_rng(bb.SEED + 9)
        bases = p.tail.bases.copy()
        hit = np.flatnonzero((rng.random(len(bases)) < 0.02) & (tc.NT4[bases] < 4))
        bases[hit] = rb.ACGT[(tc.NT4[bases[hit]] + rng.integers(1, 4, size=len(hit))) & 3]
        return bases
    return bb.memo(("alt_tail", p.name), make)


def lookup_want(oracle, p):
    """the table the lookups go to, as the oracle's Counter and as sorted arrays: the block twice, the substituted tail twice;
    none of A"""
    import test_profile as tp

    def make():
        oc = oracle.Counter(1)
        for _ in range(2):
            oc.add_reads(p.block.bases, p.block.offsets, LOOKUP_K)
            oc.add_reads(alt_tail(p), p.tail.offsets, LOOKUP_K)
        keys, counts = oc.export(True)
        assert (counts >= 2).all()
        return oc, tp.Table(keys, counts)
    return bb.memo(("lookup", p.name), make)


def lookup_counter(torch, ctx, oracle, p, n_parts=1, part=0):
    """the same table on the device (or one hash partition of it), from the two small batches"""
    from kmertools_amd import device
    ctr = device.Counter(ctx, LOOKUP_K, 1 << 23)
    blk, blk_o = dev(torch, p.block.bases), dev(torch, p.block.offsets)
    alt, alt_o = dev(torch, alt_tail(p)), dev(torch, p.tail.offsets)
    for _ in range(2):
        ctr.add_reads_part(blk, blk_o, 1, n_parts, part)
        ctr.add_reads_part(alt, alt_o, p.tail.n, n_parts, part)
    torch.cuda.synchronize()
    if n_parts == 1:
        table = lookup_want(oracle, p)[1]
        gk, gc = ctr.export_host()
        assert np.array_equal(gk, table.keys) and np.array_equal(gc, table.counts), "the small table itself is wrong"
    return ctr


@gpu
@pytest.mark.parametrize("layout", ["straddle", "aligned"])
def test_cov(torch_mod, ctx, batches, oracle, layout):
    """kt_cov_batch, f64 normalised and u32 raw, and kt_cov_batch_part over three partitions of the table.  A's k-mers are
    absent from the table: a read of B answered with A's bases falls into bin 0.  Guards: content, period, poison (rows
    primed; the partition counts are combined into zeros)"""
    torch = torch_mod
    p, bases, offsets = batches(layout)
    oc, _ = lookup_want(oracle, p)
    size, count = 1, 6
    room(torch, ctx, 1 << 31, "cov")
    raw = tuple(oc.cov_batch(x.bases, x.offsets, LOOKUP_K, size, count, False) for x in bb.pieces(p))
    assert all(r.max() < 2 ** 32 for r in raw) and raw[2][:, 0].any() and raw[2][:, 2].any() and not raw[0][:, 1:].any()
    ctr = lookup_counter(torch, ctx, oracle, p)
    try:
        out = torch.full((p.n, count), 7.25, dtype=torch.float64, device="cuda")
        ctr.cov(bases, offsets, p.n, size, count, out, True, "f64")
        mark(torch, ctx)
        check_rows(torch, p, out, tuple(oc.cov_batch(x.bases, x.offsets, LOOKUP_K, size, count, True) for x in bb.pieces(p)), "cov f64")
        out = torch.full((p.n, count), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
        ctr.cov(bases, offsets, p.n, size, count, out, False, "u32")
        mark(torch, ctx)
        check_rows(torch, p, out, tuple(r.astype(np.uint32) for r in raw), "cov u32")
    finally:
        ctr.close()
    out = torch.zeros((p.n, count), dtype=torch.int32, device="cuda")
    for part in range(3):
        ctr = lookup_counter(torch, ctx, oracle, p, 3, part)
        try:
            ctr.cov_part(bases, offsets, p.n, size, count, out, 3, part)
            mark(torch, ctx)
        finally:
            ctr.close()
    check_rows(torch, p, out, tuple(r.astype(np.uint32) for r in raw), "cov in 3 parts")


@gpu
@pytest.mark.parametrize("layout", ["straddle", "aligned"])
def test_read_solidity(torch_mod, ctx, batches, oracle, layout):
    """with first_weak.  The device half of refuse_long_reads (long_read_kernel, its claim and read-back) has to let this
    batch through: total >= 2^32 and no read that long.  Guards: content (A's reads have no solid k-mer, B's nearly all),
    period"""
    import test_read_filter as trf
    torch = torch_mod
    p, bases, offsets = batches(layout)
    _, table = lookup_want(oracle, p)
    lo, hi = 2, U32_MAX
    room(torch, ctx, 1 << 31, "read_solidity")
    want = [trf.want_solidity(oracle, x.seqs, LOOKUP_K, table, lo, hi) for x in bb.pieces(p)]
    assert not want[0][1].any() and want[2][1].any() and (want[2][2] != U32_MAX).sum() > 1000
    ctr = lookup_counter(torch, ctx, oracle, p)
    try:
        nk = torch.zeros(p.n, dtype=torch.int32, device="cuda")
        ns = torch.zeros(p.n, dtype=torch.int32, device="cuda")
        fw = torch.full((p.n,), -1, dtype=torch.int32, device="cuda")
        ctr.read_solidity(bases, offsets, p.n, lo, hi, nk, ns, fw)
        mark(torch, ctx)
    finally:
        ctr.close()
    for j, (what, got) in enumerate((("n_kmers", nk), ("n_solid", ns), ("first_weak", fw))):
        check_rows(torch, p, got, tuple(w[j] for w in want), "read_solidity, " + what)


def want_profiles(oracle, p, fill):
    import test_profile as tp
    _, table = lookup_want(oracle, p)
    return bb.memo(("profile", p.name, fill), lambda: tuple(tp.want_profile(oracle, x.seqs, LOOKUP_K, table, fill) for x in bb.pieces(p)))


@gpu
@pytest.mark.parametrize("layout", ["straddle", "aligned"])
def test_profile_and_stats(torch_mod, ctx, batches, oracle, layout):
    """kt_ctr_profile into 17 GB of poison - positions are global, and what no window starts at keeps the poison - then
    kt_profile_stats over it, which reads profile + o0 with o0 > 2^32.  Guards: poison, content, period"""
    import test_profile as tp
    torch = torch_mod
    p, bases, offsets = batches(layout)
    room(torch, ctx, p.total * 4 + p.total + (4 << 30), "profile")
    ctr = lookup_counter(torch, ctx, oracle, p)
    try:
        prof = torch.full((p.total,), signed(P32, 32), dtype=torch.int32, device="cuda")
        ctr.profile(bases, offsets, p.n, prof)
        mark(torch, ctx)
    finally:
        ctr.close()
    check_bases(torch, p, prof, want_profiles(oracle, p, P32), "profile")
    prof.masked_fill_(prof == signed(P32, 32), -1)                # the caller's fill as kt_profile_stats knows it
    outs = {name: torch.full((p.n,), signed(P64, 64) if name == "sum" else signed(P32, 32),
                             dtype=torch.int64 if name == "sum" else torch.int32, device="cuda") for name in tp.NAMES}
    ctx.profile_stats(prof, offsets, p.n, outs["n_kmers"], outs["n_present"], outs["min"], outs["median"], outs["max"], outs["sum"])
    mark(torch, ctx)
    want = [tp.want_stats(w, x.offsets) for w, x in zip(want_profiles(oracle, p, tp.NO), bb.pieces(p))]
    for name in tp.NAMES:
        check_rows(torch, p, outs[name], tuple(w[name] for w in want), "profile_stats, " + name)


@gpu
def test_correct_support_and_apply(torch_mod, ctx, batches, oracle):
    """kt_ctr_correct_support over the expected profile (put together on the GPU from the pieces' profiles, not taken from the
    call above) into 17 GB of zeros, then kt_correct_apply to a second array and in place.  B's reads differ from what the
    table was made of in 2 % of their bases: those are uncovered and the base that was there is supported.  Guards: poison
    (support stays zero where nothing is added; out_bases primed), content, period"""
    import test_correct as tc
    torch = torch_mod
    p, bases, offsets = batches("straddle")
    _, table = lookup_want(oracle, p)
    lo, hi = 2, U32_MAX
    room(torch, ctx, p.total * 4 * 2 + p.total * 3 + (4 << 30), "correct")
    profs = want_profiles(oracle, p, tc.NO)
    want = bb.memo(("support", p.name), lambda: tuple(tc.want_support(oracle, x.bases, x.offsets, LOOKUP_K, table, w, lo, hi)
                                                      for w, x in zip(profs, bb.pieces(p))))
    assert (want[2] != 0).sum() > 10000 and (want[0] != 0).sum() < 100
    prof = assemble_flat(torch, p, profs, torch.int32)
    sup = torch.zeros(p.total, dtype=torch.int32, device="cuda")
    ctr = lookup_counter(torch, ctx, oracle, p)
    try:
        ctr.correct_support(bases, offsets, p.n, prof, lo, hi, sup)
        mark(torch, ctx)
    finally:
        ctr.close()
    del prof
    check_bases(torch, p, sup, want, "correct_support")
    applied = [tc.want_apply(x.bases, x.offsets, w, 1, 0) for w, x in zip(want, bb.pieces(p))]
    assert (applied[2][0] != p.tail.bases).sum() > 10000
    out = torch.full((p.total,), P8, dtype=torch.uint8, device="cuda")
    ns = torch.full((p.n,), signed(P32, 32), dtype=torch.int32, device="cuda")
    na = torch.full((p.n,), signed(P32, 32), dtype=torch.int32, device="cuda")
    ctx.correct_apply(bases, offsets, p.n, sup, 1, 0, out, ns, na)
    mark(torch, ctx)
    check_bases(torch, p, out, tuple(a[0] for a in applied), "correct_apply, out_bases")
    check_rows(torch, p, ns, tuple(a[1] for a in applied), "correct_apply, n_single")
    check_rows(torch, p, na, tuple(a[2] for a in applied), "correct_apply, n_ambiguous")
    inplace = bases.clone()
    ctx.correct_apply(inplace, offsets, p.n, sup, 1, 0, inplace, None, None)
    mark(torch, ctx)
    assert torch.equal(inplace, out), "correct_apply in place differs from the copy"


# ---- 4. sketches and cardinality ------------------------------------------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize("layout", ["straddle", "inside_ballast"])
def test_sketch_and_card(torch_mod, ctx, batches, oracle, layout):
    """kt_sketch_batch (k = 21, s = 64): rows per read.  kt_card_add_reads (p = 14): the registers are the max-merge
    (kt_card_merge) of the oracle's registers for A, B and the block, the windows their sum.  Guards: content, period
    (sketch rows; the registers have no period: a k-mer of the ballast that is lost or made up shows only where it decides
    a register), poison (every output primed)"""
    import card_ref
    import test_sketch as ts
    torch = torch_mod
    from kmertools_amd import device
    p, bases, offsets = batches(layout)
    k, s, seed, pp = LOOKUP_K, 64, 0x5eed, 14
    room(torch, ctx, 40 << 30, "sketch and card")
    hashes = torch.full((p.n, s), signed(P64, 64), dtype=torch.int64, device="cuda")
    sizes = torch.full((p.n,), signed(P32, 32), dtype=torch.int32, device="cuda")
    nk = torch.full((p.n,), signed(P32, 32), dtype=torch.int32, device="cuda")
    ctx.sketch(bases, offsets, p.n, k, s, hashes, sizes, nk, seed)
    mark(torch, ctx)
    want = [ts.rows_of(ts.hash_sets(oracle, x.bases, x.offsets, k, seed), s) for x in bb.pieces(p)]
    for j, (what, got) in enumerate((("hashes", hashes), ("sizes", sizes), ("n_kmers", nk))):
        check_rows(torch, p, got, tuple(w[j] for w in want), "sketch, " + what)
    regs = torch.zeros(1 << pp, dtype=torch.uint8, device="cuda")
    windows = torch.zeros(1, dtype=torch.int64, device="cuda")
    ctx.card_add(bases, offsets, p.n, k, regs, pp, seed, windows)
    mark(torch, ctx)
    wregs, wwin = np.zeros(1 << pp, np.uint8), 0
    for x, times in zip(bb.pieces(p), (1, p.copies, 1)):
        r, w = card_ref.registers(oracle, x.bases, x.offsets, k, pp, seed)
        device.card_merge(wregs, r)
        wwin += times * w
    got = regs.cpu().numpy()
    bad = np.flatnonzero(got != wregs)
    assert not len(bad), ("card registers", p.name, len(bad), bad[:4], got[bad[:4]], wregs[bad[:4]])
    assert int(windows.cpu().numpy().view(U64)[0]) == wwin > G32 * 0.7, ("card windows", p.name, int(windows[0]), wwin)


# ---- 5. minimisers --------------------------------------------------------------------------------------------------------------------------

def minimisers_flat(oracle, x, w, m):
    """rb.oracle_minimisers_flat; w = 0: a read shorter than m yields nothing (kt_minimisers says so; the reference's own
    arithmetic underflows there), which is what an empty read yields"""
    if w == 0 and (x.lens < m).any():
        lens = x.lens
        keep = np.repeat(lens >= m, lens)
        evo, k, s, e = rb.oracle_minimisers_flat(oracle, rb.Batch.of_lens(x.name + ", reads of m bases or more", x.bases[keep],
                                                                         np.where(lens >= m, lens, 0)), w, m)
        return evo, k, s, e
    return rb.oracle_minimisers_flat(oracle, x, w, m)


MIN_CASES = [(0, 15, False), (31, 15, False), (5000, 21, False), (5000, 21, True)]


@gpu
@pytest.mark.parametrize("w,m,serial", MIN_CASES, ids=["w0_m15", "w31_m15", "w5000_m21_two_level", "w5000_m21_serial"])
def test_minimisers(torch_mod, ctx, batches, oracle, monkeypatch, w, m, serial):
    """events per read are the small batches' events: starts and ends are read-local, so the ballast's events have the
    period; ev_offsets is the running sum of the expected events per read (monotone, ending at n_events).  (5000, 21): the
    two-level sliding minimum (three scratch arrays of one m-mer per base), and with KT_MIN_SERIAL=1 one thread per read -
    4294 threads walk a million bases each, which is why that case takes seconds.  Guards: content, period, poison (the
    event arrays are primed, and exactly n_events of room)"""
    torch = torch_mod
    p, bases, offsets = batches("straddle")
    if serial:
        monkeypatch.setenv("KT_MIN_SERIAL", "1")
    else:
        monkeypatch.delenv("KT_MIN_SERIAL", raising=False)
    want = [bb.memo(("minimisers", x.name, w, m), lambda x=x: minimisers_flat(oracle, x, w, m)) for x in bb.pieces(p)]
    per_read = np.concatenate([np.diff(want[0][0].astype(np.int64)), np.full(p.copies, int(want[1][0][-1])),
                               np.diff(want[2][0].astype(np.int64))])
    evo = np.concatenate(([0], np.cumsum(per_read))).astype(U64)
    n_ev, unit = int(evo[-1]), int(want[1][0][-1])
    real = [int((x[1] != U64(NONE_KMER)).sum()) for x in want]     # minimisers that are k-mers, not the "none" of a window that never fills
    assert unit >= 1 and (real[2] > 1000 if w == 0 else real[1] > 1000 and real[2] > 1000 if w < 5000 else real[1] >= 3), (w, m, unit, real)
    room(torch, ctx, n_ev * 24 + (27 * p.total if w >= 5000 else 8 * p.total) + (4 << 30), "minimisers")   # (measured: 116 GB two-level)
    d_evo = torch.full((p.n + 1,), signed(P64, 64), dtype=torch.int64, device="cuda")
    counted = ctx.minimisers(bases, offsets, p.n, w, m, d_evo, None, None, None, 0)
    mark(torch, ctx)
    assert counted == n_ev, ("minimisers, count only", p.name, w, m, counted, n_ev)
    outs = [torch.full((n_ev,), signed(P64, 64), dtype=torch.int64, device="cuda") for _ in range(3)]
    written = ctx.minimisers(bases, offsets, p.n, w, m, d_evo, outs[0], outs[1], outs[2], n_ev)
    mark(torch, ctx)
    assert written == n_ev, ("minimisers", p.name, w, m, written, n_ev)
    got = d_evo.cpu().numpy().view(U64)
    bad = np.flatnonzero(got != evo)
    assert not len(bad), ("ev_offsets", p.name, w, m, bad[:4], got[bad[:4]], evo[bad[:4]], "2^32 is in read %d" % p.read_of(G32))
    sizes = (int(want[0][0][-1]), unit, int(want[2][0][-1]))
    for j, what in ((1, "kmers"), (2, "starts"), (3, "ends")):
        check_parts(torch, p, outs[j - 1], sizes, tuple(x[j] for x in want), "minimisers w = %d, m = %d%s, %s" % (
            w, m, ", KT_MIN_SERIAL=1" if serial else "", what))


# ---- 6. the outputs with an entry per base ------------------------------------------------------------------------------------------------------

@gpu
def test_kmers(torch_mod, ctx, batches, oracle):
    """kt_kmers, k = 31: 73 GB of outputs indexed by the global base index.  fwd and rev are written only where a k-mer ends:
    everything else keeps the poison.  Guards: poison, content, period"""
    torch = torch_mod
    p, bases, offsets = batches("straddle")
    k = 31
    room(torch, ctx, p.total * 17 + (4 << 30), "kmers")
    fwd = torch.full((p.total,), signed(P64, 64), dtype=torch.int64, device="cuda")
    rev = torch.full((p.total,), signed(P64, 64), dtype=torch.int64, device="cuda")
    valid = torch.full((p.total,), P8, dtype=torch.uint8, device="cuda")
    ctx.kmers(bases, offsets, p.n, k, fwd, rev, valid)
    mark(torch, ctx)
    want = {"fwd": [], "rev": [], "valid": []}
    for x in bb.pieces(p):
        f, r, e = rb.oracle_kmers_flat(oracle, x, k)
        e = e.astype(np.int64)
        wf, wr, wv = np.full(x.total, P64, U64), np.full(x.total, P64, U64), np.zeros(x.total, np.uint8)
        wf[e], wr[e], wv[e] = f, r, 1
        want["fwd"].append(wf)
        want["rev"].append(wr)
        want["valid"].append(wv)
    assert want["valid"][2].sum() > 1_000_000
    for what, got in (("valid", valid), ("fwd", fwd), ("rev", rev)):
        check_bases(torch, p, got, tuple(want[what]), "kmers k = %d, %s" % (k, what))


@gpu
def test_cgr_points(torch_mod, ctx, batches, oracle):
    """kt_cgr_points: 69 GB of points, on the letters-only variants of the pieces (any other byte fails the whole call).
    bad_pos stays UINT64_MAX; with one N planted at base 2^32 + 5 it is exactly that index.  Guards: poison (the points are
    primed with NaN, which equals nothing), content, period"""
    torch = torch_mod
    p, bases, offsets = batches("straddle", True)
    room(torch, ctx, p.total * 16 + (4 << 30), "cgr")
    xy = torch.full((p.total, 2), float("nan"), dtype=torch.float64, device="cuda")
    bad = torch.full((1,), 12345, dtype=torch.int64, device="cuda")
    ctx.cgr(bases, offsets, p.n, 1, xy, bad)
    mark(torch, ctx)
    assert int(bad.cpu().numpy().view(U64)[0]) == 2 ** 64 - 1, ("bad_pos of a batch of letters", int(bad[0]))
    check_bases(torch, p, xy, tuple(oracle.cgr_batch(x.bases, x.offsets, 1) for x in bb.pieces(p)), "cgr")
    at = G32 + 5
    assert p.offsets[p.read_of(at)] < at < p.offsets[p.read_of(at) + 1] - 1
    keep = int(bases[at])
    try:
        bases[at] = ord("N")
        bad.fill_(12345)
        ctx.cgr(bases, offsets, p.n, 1, xy, bad)
        mark(torch, ctx)
        assert int(bad.cpu().numpy().view(U64)[0]) == at, ("bad_pos", int(bad[0]), at, int(bad[0]) - at)
    finally:
        bases[at] = keep


@gpu
def test_route(torch_mod, ctx, batches, oracle):
    """kt_ctr_route, k = 31, 8 owners: 34 GB of keys_out.  Owner by owner the group, sorted on the GPU, holds exactly the
    expected k-mers of kt_owner_of's owner, each as often as expected; owner_counts sum to the valid k-mers and nothing is
    written behind them.  Guards: content and period (through the multiplicities), poison"""
    import test_correct as tc
    torch = torch_mod
    from kmertools_amd import device
    p, bases, offsets = batches("straddle")
    k, owners = 31, 8
    wk, wc = expected_table(oracle, p, k)
    own = tc.owner_of(wk, owners)
    step = max(1, len(wk) // 300)
    assert [device.owner_of(int(x), owners) for x in wk[::step]] == own[::step].tolist()
    room(torch, ctx, p.total * 8 + 3 * 8 * (int(wc.sum()) // owners * 2) + (8 << 30), "route")
    keys = torch.full((p.total,), signed(P64, 64), dtype=torch.int64, device="cuda")
    counts = torch.full((owners,), signed(P64, 64), dtype=torch.int64, device="cuda")
    ctx.route(bases, offsets, p.n, k, owners, keys, counts)
    mark(torch, ctx)
    got = counts.cpu().numpy().view(U64)
    want = np.array([int(wc[own == o].sum()) for o in range(owners)], U64)
    assert np.array_equal(got, want), ("owner_counts", got, want, "sum %d, expected %d" % (int(got.sum()), int(wc.sum())))
    start = 0
    for o in range(owners):
        n = int(want[o])
        uk, uc = torch.unique_consecutive(torch.sort(keys[start:start + n]).values, return_counts=True)
        mark(torch, ctx)
        gk, gc = uk.cpu().numpy().view(U64), uc.cpu().numpy().astype(U64)
        del uk, uc
        bad = table_mismatch(p, gk, gc, wk[own == o], wc[own == o])
        assert bad is None, "route, owner %d of %d, %s: %s" % (o, owners, p.name, bad)
        start += n
    assert bool((keys[start:] == signed(P64, 64)).all()), "keys_out is written behind the last group"


# ---- 7. a refusal -----------------------------------------------------------------------------------------------------------------------------

@gpu
def test_sharded_refuses_regions_past_32_bits(torch_mod, ctx):
    """kt_sharded_create_local with a max_batch_bases whose exchange regions would hold 0xFFF00000 records or more (the route
    pass keeps a record's place in 32 bits): KT_ERR_ARG, and what sharded_alloc had allocated before the check - the shard's
    table and the pending table - is given back"""
    torch = torch_mod
    from kmertools_amd import _lib, device
    room(torch, ctx, 16 << 30, "the refusal")
    before = free_bytes(ctx)
    with pytest.raises(_lib.KmertoolsError) as err:
        device.Sharded(ctx, 31, 1 << 16, 1 << 35, 2, 0, ("host", lambda *a: 0), connect=False)
    assert err.value.code == _lib.KT_ERR_ARG and "too large for the exchange regions" in str(err.value), str(err.value)
    mark(torch, ctx)
    assert free_bytes(ctx) >= before - (256 << 20), (before, free_bytes(ctx))
