"""Every kernel that turns a CSR batch into per-read or per-k-mer results, on the read-length distributions where "which read
does this base belong to" is hard: reads far shorter than a 16-base lane by the ten thousand (family A), runs of up to 5000
empty reads (B), read ends one before, on and one after every structural constant of the kernels, followed by reads of 0, 1,
k-1, k, k+1 bases (C), reads of one length at the lengths where the equal-length oligo path changes its arithmetic (D), and
the letters-only / minimiser variants of A-C (E).  tests/read_batches.py builds them from a seed.

Each test first asserts, from the offsets alone, that its batch has the shape it is meant to have (`check_*`): a generator
that is reseeded or resized cannot quietly stop reaching the branch.  Results against the CPU oracle (which
tests/test_oracle_brute_force.py holds against a brute force): integers and f64 bit-exact, f32 within 1e-6.  A failure names
the family, k, the configuration and the first differing read with its length, its neighbours' lengths and its start
modulo 16, 32 and 8192.

What a configuration leaves out is decided here, statically, and said where it is decided: a tile size that does not fit
the LDS is not listed; the rows of the generic oligo path at k = 8 / 12 (256 KB / 64 MB each) bound the number of reads
of those batches; `w = 0` minimisers are undefined by the reference for a read shorter than m."""
import numpy as np
import pytest

import read_batches as rb
import shard_ref
from read_batches import bases_view, offsets_view, where

pytestmark = pytest.mark.gpu

SEED = 0xb0a7
U32_MAX = 0xFFFFFFFF
U = np.uint64


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


_memo = {}


def memo(key, fn):
    if key not in _memo:
        _memo[key] = fn()
    return _memo[key]


# ---- the batches and their self-checks -------------------------------------------------------------------------------------

def check_dense(b, segments=True, lanes_3=100):
    """family A: a segment with more than 512 read starts and one with 257..512 (`segments`: for the kernels that work by
    8192-base segments), 100 lanes with three or more read starts, 10 lanes whose following read ends on the lane's last
    base - the latter two hold for every batch, however few reads its rows allow (tiny_batch's core)"""
    s = rb.shape_numbers(b.offsets)
    if segments:
        assert s["segments_over_512"] >= 1 and s["segments_257_512"] >= 1, (b.name, s)
    assert s["lanes_3_starts"] >= lanes_3 and s["lane_end_reads"] >= 10 and len(s["lane_end_rems"]) >= 10, (b.name, s)
    return s


def check_empty_runs(b):
    """family B: every run is where it is meant to be - all of its reads empty, a read with bases on both sides (none
    before the first run, none behind the last), the aligned ones right behind a read that ends on a multiple of 8192"""
    lens, o = b.lens, b.offsets.astype(np.int64)
    kinds = set()
    for at, r, kind in b.meta["runs"]:
        assert (lens[at:at + r] == 0).all(), (b.name, at, r, kind)
        assert at == 0 if kind == "start" else lens[at - 1] > 0, (b.name, at, r, kind)
        assert at + r == b.n if kind == "end" else lens[at + r] > 0, (b.name, at, r, kind)
        if kind == "aligned":
            assert o[at] % rb.SEG == 0 and o[at] > 0, (b.name, at, r, kind)
        kinds.add((kind, r))
    return kinds


def check_lattice(b, consts, follows):
    """family C: every (c, d, follow length) has a read that ends at m c + d with a read of that length behind it and a
    read with bases in front; the reads that end on a lane's last base come with every rem in 1..15 (rem + K - 1 on both
    sides of 16 for every K); a poly-A read starts where it is meant to"""
    lens, o = b.lens, b.offsets.astype(np.int64)
    seen = set()
    for c, d, f, pos, i in b.meta["junctions"]:
        assert o[i] == pos and pos % c == d % c and lens[i] == f and lens[i - 1] >= 17, (b.name, c, d, f, pos, i)
        seen.add((c, d, f))
    assert seen == {(c, d, f) for c in consts for d in (-1, 0, 1) for f in follows}, b.name
    for rem, i in b.meta["lane_ends"]:
        assert o[i] % 16 == rem and o[i + 1] % 16 == 0 and lens[i] == 16 - rem and lens[i - 1] >= 17, (b.name, rem, i)
    for before, i in b.meta["poly_a"]:
        assert (o[i] + before) % 128 == 0 and lens[i] == 300 and (b.bases[o[i]:o[i + 1]] == ord("A")).all(), (b.name, before)
    s = rb.shape_numbers(b.offsets)
    if b.meta["lane_ends"]:
        assert s["lane_end_rems"] == list(range(1, 16)) and s["lane_end_reads"] >= 10, (b.name, s)
    return s


def follows_of(k, min_len=0):
    return sorted({min_len + x for x in (0, 1, k - 1, k, k + 1)})


def family_batch(family, k):
    """the batch of a family at full size (for the kernels whose output is per k-mer or one table), self-checked"""
    def make():
        if family == "tiny":
            b = rb.tiny_batch(SEED + k, k, 16000)
            b.meta["shape"] = check_dense(b)
        elif family == "empty_runs":
            b = rb.empty_runs_batch(SEED)
            assert check_empty_runs(b) >= {(w, r) for w in ("between", "aligned") for r in rb.EMPTY_RUNS} | {("start", 5000), ("end", 257)}
        elif family == "empty_runs2":                     # the other lengths at the batch's two ends
            b = rb.empty_runs_batch(SEED + 1, first=65, last=5000)
            assert check_empty_runs(b) >= {("start", 65), ("end", 5000)}
        elif family == "lattice":
            b = rb.lattice_batch(SEED + k, k)
            b.meta["shape"] = check_lattice(b, rb.LATTICE, follows_of(k))
        else:
            b = rb.equal_concat_batch(SEED + k, k)
        assert b.total <= 600_000, (b.name, b.total)
        return b
    return memo(("family", family, 0 if family.startswith("empty") else k), make)


FAMILIES = ("tiny", "empty_runs", "empty_runs2", "lattice", "equal")


def oracle_kmers(oracle, b, k):
    return memo(("kmers", b.name, k), lambda: rb.oracle_kmers_flat(oracle, b, k))


def oracle_table(oracle, b, k):
    return memo(("table", b.name, k), lambda: oracle.count_reads(b.bases, b.offsets, k))


def first_flat_diff(got, want):
    """index of the first element in which two tuples of flat arrays differ (their lengths included), None when equal"""
    n = min(len(got[0]), len(want[0]))
    bad = np.zeros(n, bool)
    for g, w in zip(got, want):
        bad |= g[:n] != w[:n]
    hit = np.flatnonzero(bad)
    if len(hit):
        return int(hit[0])
    return None if len(got[0]) == len(want[0]) else n


def first_row_diff(got, want):
    bad = got != want
    if bad.ndim > 1:
        bad = bad.any(axis=1)
    hit = np.flatnonzero(bad)
    return int(hit[0]) if len(hit) else None


def table_diff(oracle, b, k, gk, gc, wk, wc, times=1):
    """None when the exported table is the oracle's (counts `times` over); else where: the read of the first k-mer, in
    batch order, whose count is wrong or missing, or the first key that no read has"""
    if np.array_equal(gk, wk) and np.array_equal(gc, times * wc):
        return None
    extra = np.setdiff1d(gk, wk)
    if len(extra):
        return "a key that no read holds: %#x (%d such keys)" % (int(extra[0]), len(extra))
    got = dict(zip(gk.tolist(), gc.tolist()))
    f, r, e = oracle_kmers(oracle, b, k)
    canon = np.minimum(f, r)
    want = dict(zip(wk.tolist(), wc.tolist()))
    for key, end in zip(canon.tolist(), e.tolist()):
        if got.get(key, 0) != times * want[key]:
            return "k-mer %#x that ends at base %d: count %d, expected %d; %s" % (
                key, end, got.get(key, 0), times * want[key], where(b, rb.read_of(b, end)))
    return "tables differ in length only: %d / %d" % (len(gk), len(wk))


# ---- 1. kt_kmers -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", [1, 2, 4, 15, 16, 17, 31])
@pytest.mark.parametrize("family", FAMILIES)
def test_kmers(hctx, oracle, family, k):
    b = family_batch(family, k)
    want = oracle_kmers(oracle, b, k)
    gf, gr, ge = hctx.kmers_host(b.bases, b.offsets, k)
    j = first_flat_diff((ge, gf, gr), (want[2], want[0], want[1]))
    if j is not None:
        pos = min(int(ge[j]) if j < len(ge) else b.total, int(want[2][j]) if j < len(want[2]) else b.total)
        pytest.fail("kmers, family %s, k = %d: k-mer %d differs (%d found, %d expected); %s" % (
            family, k, j, len(ge), len(want[2]), where(b, rb.read_of(b, pos))))


# ---- 2. the LDS oligo kernel (k = 3..7) ---------------------------------------------------------------------------------------

def oligo_bins(k, count_min):
    return (4 ** k + (4 ** (k // 2) if k % 2 == 0 else 0)) // 2 if count_min else 4 ** k


def oligo_max_R(k, count_min):
    """the largest tile kt_oligo_batch accepts (kt_oligo.hip, oligo_launch): LUT (canonical, k <= 5) + R rows of u32 bins +
    the per-read arrays of 64 reads within 160 KB of LDS, at most 64 reads"""
    lut = (4 ** k * 2 + 15) // 16 * 16 if count_min and k <= 5 else 0
    fixed = 2 * 64 * 4 + 2 * 64 * 8 + 65 * 8 + 8 + 128
    return min(64, (160 * 1024 - lut - fixed) // (oligo_bins(k, count_min) * 4))


def oligo_tile_sizes(k, count_min):
    """None (the library's own choice), 1, 3 and the largest that fits - those of them that fit"""
    top = oligo_max_R(k, count_min)
    return [None] + sorted({r for r in (1, 3, top) if r <= top})


OLIGO_CASES = [(k, cm) for k in (3, 4, 5, 6, 7) for cm in (True, False)]


def oligo_family_batch(family, k, count_min):
    """the batches of the LDS oligo tests: as many reads as 2^23 output cells allow (rows of up to 64 KB)"""
    bins = oligo_bins(k, count_min)

    def make():
        if family == "tiny":
            b = rb.tiny_batch(SEED + k, k, int(min(24000, max(400, (1 << 23) // bins * 4 // 7))))
            # (this kernel works by tiles of R reads, not by segments: with rows of 64 KB the whole batch is less than one)
            b.meta["shape"] = check_dense(b, segments=False)
        elif family == "empty_runs":
            # an empty read is a row of zeros: the runs are as long as the rows allow, and always cross the tile sizes
            runs = rb.EMPTY_RUNS if bins <= 1024 else (1, 63, 64, 65, 256, 257) if bins <= 4096 else (1, 3, 4, 5, 63, 64, 65)
            b = rb.empty_runs_batch(SEED + k, runs=runs)
            assert check_empty_runs(b) >= {(w, r) for w in ("between", "aligned") for r in runs}
        else:
            b = rb.lattice_batch(SEED + k, k)
            b.meta["shape"] = check_lattice(b, rb.LATTICE, follows_of(k))
        return b
    return memo(("oligo", family, k, bins), make)


class OligoWant:
    """the oracle's rows of a batch on the device: raw counts as u32, normalised rows as f64"""

    def __init__(self, torch, oracle, b, k, count_min):
        raw = oracle.oligo_batch(b.bases, b.offsets, k, count_min, False, 1.0, threads=8)
        assert raw.max(initial=0) < 2 ** 32
        short = b.lens < k
        assert not raw[short].any()                       # (rows of empty and too short reads: exactly zero)
        self.host_u32 = raw.astype(np.uint32)
        del raw
        self.host_f64 = oracle.oligo_batch(b.bases, b.offsets, k, count_min, True, 1.0, threads=8)
        assert not self.host_f64[short].any()
        self.u32 = torch.from_numpy(self.host_u32.view(np.int32)).cuda()
        self.f64 = torch.from_numpy(self.host_f64).cuda()


def oligo_compare(torch, c, b, bv, ov, k, count_min, want, dtypes, tag):
    from kmertools_amd import device
    bins = device.bins(k, count_min)
    assert bins == oligo_bins(k, count_min)
    for dt in dtypes:
        tdt = {"u32": torch.int32, "f64": torch.float64, "f32": torch.float32}[dt]
        out = torch.full((b.n, bins), 0x5A5A5A5A if dt == "u32" else 7.25, dtype=tdt, device="cuda")   # (never a valid row)
        c.oligo(bv, ov, b.n, k, out, count_min, dt != "u32", 1, dt)
        torch.cuda.synchronize()
        if dt == "u32":
            bad = (out != want.u32).any(dim=1)
        elif dt == "f64":
            bad = (out.view(torch.int64) != want.f64.view(torch.int64)).any(dim=1)
        else:
            bad = ((out.double() - want.f64).abs() > 1e-6).any(dim=1) | ~torch.isfinite(out).all(dim=1)
        rows = torch.nonzero(bad).flatten()
        if rows.numel():
            i = int(rows[0])
            exp = (want.u32 if dt == "u32" else want.f64)[i]
            cols = torch.nonzero(out[i].double() != exp.double()).flatten()[:4].tolist()
            pytest.fail("oligo %s, %s: %d rows differ, first: %s; bins %s: got %s, expected %s" % (
                tag, dt, rows.numel(), where(b, i), cols, out[i][cols].tolist(), exp[cols].tolist()))
        del out


def oligo_compare_host(c, b, k, count_min, want, tag):
    """the same through host arrays (kt_oligo_batch stages them and the rows, slab by slab)"""
    for dt in ("u32", "f64"):
        got = c.oligo_host(b.bases, b.offsets, k, count_min, dt == "f64", 1, dt)
        exp = want.host_u32 if dt == "u32" else want.host_f64
        i = first_row_diff(got.view(np.uint64) if dt == "f64" else got, exp.view(np.uint64) if dt == "f64" else exp)
        if i is not None:
            cols = np.flatnonzero(got[i] != exp[i])[:4]
            pytest.fail("oligo %s, host arrays, %s: first differing row: %s; bins %s: got %s, expected %s" % (
                tag, dt, where(b, i), cols, got[i][cols], exp[i][cols]))
        del got


def oligo_context(monkeypatch, torch, R=None, pw=None):
    """a context of its own: the tile size and the producer-wave threshold are read once per context"""
    from kmertools_amd import device
    for name, val in (("KT_OLIGO_R", R), ("KT_OLIGO_PW", pw)):
        if val is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, str(val))
    return device.Context(0, stream=torch.cuda.current_stream().cuda_stream)


@pytest.mark.parametrize("k,count_min", OLIGO_CASES)
@pytest.mark.parametrize("family", ["tiny", "empty_runs", "lattice"])
def test_oligo_lds(torch_mod, oracle, monkeypatch, family, k, count_min):
    """every tile size, with and without the producer wave at k = 7; u32 and f64 everywhere, f32 and the call through host
    arrays at the library's own tile size.  With R known, the tiny batch must hold 10 tiles on process_chunk's `t0 < 0` per-base path."""
    torch = torch_mod
    b = oligo_family_batch(family, k, count_min)
    want = OligoWant(torch, oracle, b, k, count_min)
    bv, ov = bases_view(torch, b.bases, 0), offsets_view(torch, b.offsets)
    for R in oligo_tile_sizes(k, count_min):
        if family == "tiny" and R is not None and R > 1:
            tiles = rb.split_first_lane_tiles(b.offsets, R)
            assert tiles >= 10, (b.name, R, tiles)
        for pw in (7, 8) if k == 7 else (None,):
            c = oligo_context(monkeypatch, torch, R, pw)
            try:
                tag = "family %s, k = %d, count_min = %s, KT_OLIGO_R = %s, KT_OLIGO_PW = %s" % (family, k, count_min, R, pw)
                oligo_compare(torch, c, b, bv, ov, k, count_min, want, ("u32", "f64") + (("f32",) if R is None else ()), tag)
                if R is None:
                    oligo_compare_host(c, b, k, count_min, want, tag)
            finally:
                c.close()


@pytest.mark.parametrize("k,count_min", OLIGO_CASES)
def test_oligo_equal_length(torch_mod, ctx, oracle, k, count_min):
    """family D: 193 reads (a prime: the last tile is partial whatever the tile size) of every length at which the
    equal-length path changes - the smallest it takes, one more, a k-mer more than a lane, around 32, 64, the clamp at 255
    and the 1008-base chunk - from a base pointer 0, 1 and 15 past a 256-byte boundary"""
    torch = torch_mod
    for L in rb.equal_lengths(k):
        b = rb.equal_batch(SEED + k, L, 193)
        assert (b.lens == L).all() and L >= 16 and b.n % 2 and b.n % 3 and b.n > 64
        want = OligoWant(torch, oracle, b, k, count_min)
        ov = offsets_view(torch, b.offsets)
        for shift in (0, 1, 15):
            oligo_compare(torch, ctx, b, bases_view(torch, b.bases, shift), ov, k, count_min, want,
                          ("u32", "f64") + (("f32",) if L == 257 and shift == 1 else ()),
                          "family equal, L = %d, k = %d, count_min = %s, shift %d" % (L, k, count_min, shift))


@pytest.mark.parametrize("k,count_min", OLIGO_CASES)
def test_oligo_mixed_tiles(torch_mod, oracle, monkeypatch, k, count_min):
    """family D, mixed: with the tile size known, equal tiles next to ragged ones (`general` flips from tile to tile), a tile
    of equal reads shorter than a lane, a tile equal but for its last read"""
    torch = torch_mod
    for R in sorted({min(3, oligo_max_R(k, count_min)), min(8, oligo_max_R(k, count_min))}):
        b = rb.mixed_tiles_batch(SEED + k, R)
        lens = b.lens
        equal = [len(set(lens[t * R:(t + 1) * R])) == 1 and lens[t * R] >= 16 for t in range(len(b.meta["tiles"]))]
        assert equal == [kind in ("equal40", "equal33", "equal17") for kind in b.meta["tiles"]] and b.n % R == 1
        assert (lens[4 * R:5 * R] == 9).all() and len(set(lens[6 * R:7 * R - 1])) == 1 and (R == 1 or lens[7 * R - 1] != lens[6 * R])
        want = OligoWant(torch, oracle, b, k, count_min)
        ov = offsets_view(torch, b.offsets)
        c = oligo_context(monkeypatch, torch, R)
        try:
            for shift in (0, 1, 15):
                oligo_compare(torch, c, b, bases_view(torch, b.bases, shift), ov, k, count_min, want, ("u32", "f64"),
                              "family mixed tiles, KT_OLIGO_R = %d, k = %d, count_min = %s, shift %d" % (R, k, count_min, shift))
        finally:
            c.close()


# ---- 3. the generic oligo path (rows in global memory) ----------------------------------------------------------------------

def generic_batch(family, k):
    """k = 1, 2: the full families.  k = 8 (rows of 256 KB): 7000 reads at most - the longest run of empty reads is 1500.
    k = 12 (rows of 64 MB, 16 or 31 reads per slab): about 100 reads - runs of 1, 16 and 31 empty reads, the lattice of 16 and
    8192 alone with fillers of 2000..4000 bases."""
    def make():
        if family == "tiny":
            if k < 12:
                b = rb.tiny_batch(SEED + k, k, {1: 16000, 2: 16000, 8: 2400}[k])
                b.meta["shape"] = check_dense(b)
            else:
                # rows of 64 MB: about 120 reads, all in one segment - no segment can have 257 read starts and there is no
                # room for 100 lanes of three; what holds is asserted: a core of 10 lane-end pairs and 20 lanes of three
                # reads (80 reads), 24 random ones, every read start of the batch inside one segment
                b = rb.tiny_batch(SEED + k, k, 14, core=(10, 20))
                b.meta["shape"] = check_dense(b, segments=False, lanes_3=20)
                assert b.meta["shape"]["max_starts_per_segment"] == b.n >= 100, (b.name, b.meta["shape"])
        elif family == "empty_runs":
            runs = rb.EMPTY_RUNS if k <= 2 else (1, 63, 64, 65, 256, 257, 1500) if k == 8 else (1, 16, 31)
            b = rb.empty_runs_batch(SEED + k, runs=runs, first=runs[-1] if k < 12 else 2, last=runs[-2] if k < 12 else 3,
                                    filler=(17, 300) if k < 12 else (2000, 4000))
            assert check_empty_runs(b) >= {(w, r) for w in ("between", "aligned") for r in runs}
        else:
            consts = rb.LATTICE if k < 12 else (16, 8192)
            b = rb.lattice_batch(SEED + k, k, consts=consts, filler=(17, 300) if k < 12 else (2000, 4000))
            b.meta["shape"] = check_lattice(b, consts, follows_of(k))
        assert b.n <= {1: 1 << 20, 2: 1 << 20, 8: 7000, 12: 140}[k], (b.name, b.n)
        return b
    return memo(("generic", family, k), make)


def sparse_rows(oracle, b, k, count_min):
    """the non-zero cells of the oracle's rows -> (flat cell index row * bins + bin, ascending; count; k-mers per read)"""
    f, r, e = oracle_kmers(oracle, b, k)
    bins = oligo_bins(k, count_min)
    if count_min:
        pmap = memo(("pos_map", k), lambda: oracle.pos_maps(k)[0])
        col = pmap[np.minimum(f, r)].astype(np.int64)
    else:
        col = f.astype(np.int64)
    row = np.searchsorted(b.offsets.astype(np.int64), e.astype(np.int64), side="right") - 1
    cells, counts = np.unique(row * bins + col, return_counts=True)
    return cells, counts, np.bincount(row, minlength=b.n)


# u32 and f64 rows at every k but 12, where the u32 rows of a batch alone take 4 to 8 GB
GENERIC_DTYPES = {1: ("u32", "f64"), 2: ("u32", "f64"), 8: ("u32", "f64"), 12: ("u32",)}


@pytest.mark.parametrize("count_min", [True, False])
@pytest.mark.parametrize("k", [1, 2, 8, 12])
@pytest.mark.parametrize("family", ["tiny", "empty_runs", "lattice"])
def test_oligo_generic(torch_mod, ctx, oracle, family, k, count_min):
    """u32 and f64 rows (GENERIC_DTYPES), compared cell by cell through the non-zero cells"""
    torch = torch_mod
    from kmertools_amd import device
    b = generic_batch(family, k)
    bins = device.bins(k, count_min)
    assert bins == oligo_bins(k, count_min)
    cells, counts, totals = sparse_rows(oracle, b, k, count_min)
    bv, ov = bases_view(torch, b.bases, 0), offsets_view(torch, b.offsets)
    try:
        for dt in GENERIC_DTYPES[k]:
            out = torch.full((b.n, bins), 0x5A5A5A5A if dt == "u32" else 7.25,
                             dtype=torch.int32 if dt == "u32" else torch.float64, device="cuda")
            ctx.oligo(bv, ov, b.n, k, out, count_min, dt == "f64", 1, dt)
            nz = torch.nonzero(out.view(-1)).flatten()
            vals = out.view(-1)[nz].cpu().numpy()
            got_cells = nz.cpu().numpy()
            del nz, out
            want_vals = counts if dt == "u32" else counts.astype(np.float64) / np.maximum(1, totals[cells // bins])
            j = first_flat_diff((got_cells, vals.view(np.uint64) if dt == "f64" else vals),
                                (cells, want_vals.view(np.uint64) if dt == "f64" else want_vals))
            if j is not None:
                cell = min(int(got_cells[j]) if j < len(got_cells) else b.n * bins, int(cells[j]) if j < len(cells) else b.n * bins)
                pytest.fail("generic oligo, family %s, k = %d, count_min = %s, %s: non-zero cell %d differs (%d found, %d "
                            "expected), bin %d; %s" % (family, k, count_min, dt, j, len(got_cells), len(cells), cell % bins,
                                                      where(b, cell // bins)))
    finally:
        torch.cuda.empty_cache()


# ---- 4. counting ---------------------------------------------------------------------------------------------------------------

CTR_ENV = {"incremental": {"KT_BULK_MIN_BASES": str(1 << 40)},
           "packed": {"KT_BULK_MIN_BASES": "0", "KT_BULK_PACK": "1"},
           "staged": {"KT_BULK_MIN_BASES": "0", "KT_BULK_PACK": "0"},
           "direct": {"KT_BULK_MIN_BASES": "0"}}
CTR_CASES = [(form, k) for form in ("incremental", "packed", "staged") for k in (1, 4, 15, 16, 17, 31)] + [("direct", 8)]


@pytest.mark.parametrize("form,k", CTR_CASES)
@pytest.mark.parametrize("family", FAMILIES)
def test_counter(torch_mod, ctx, oracle, monkeypatch, family, form, k):
    """the incremental path, the bulk build over packed reads and over staged reads, a direct-addressed table: the oracle's
    table; the same batch again doubles it (the merge / the probes over the same boundaries)"""
    torch = torch_mod
    from kmertools_amd import device
    for name, val in CTR_ENV[form].items():
        monkeypatch.setenv(name, val)
    b = family_batch(family, k)
    wk, wc = oracle_table(oracle, b, k)
    bv, ov = bases_view(torch, b.bases, 0), offsets_view(torch, b.offsets)
    ctr = device.Counter(ctx, k, 4 ** k if form == "direct" else 1 << 21)
    try:
        for times in (1, 2):
            ctr.add_reads(bv, ov, b.n)
            gk, gc = ctr.export_host()
            bad = table_diff(oracle, b, k, gk, gc, wk, wc, times)
            assert bad is None, "counter (%s), family %s, k = %d, add %d: %s" % (form, family, k, times, bad)
    finally:
        ctr.close()


# ---- 5. the route kernel and the routed (sharded) counter ------------------------------------------------------------------------

def route_batch(family, k):
    """the families at a size the numpy restatement of the records (tests/shard_ref.py, read by read) gets through"""
    def make():
        if family == "tiny":
            b = rb.tiny_batch(SEED + k, k, 6000)
            b.meta["shape"] = check_dense(b)
            return b
        return family_batch(family, k)
    return memo(("route", family, k), make)


@pytest.mark.parametrize("owners", [3, 8])
@pytest.mark.parametrize("k", [5, 31])
@pytest.mark.parametrize("family", ["tiny", "empty_runs", "lattice"])
def test_route(hctx, oracle, family, k, owners):
    """kt_ctr_route: the canonical k-mers of the oracle, each once, grouped by owner"""
    from kmertools_amd import device
    b = route_batch(family, k)
    f, r, e = oracle_kmers(oracle, b, k)
    canon = np.minimum(f, r)
    keys, counts = hctx.route_host(b.bases, b.offsets, k, owners)
    tag = "route, family %s, k = %d, %d owners" % (family, k, owners)
    gk, gc = np.unique(keys, return_counts=True)
    wk, wc = np.unique(canon, return_counts=True)
    bad = table_diff(oracle, b, k, gk, gc.astype(np.uint32), wk, wc.astype(np.uint32))
    assert bad is None and int(counts.sum()) == len(canon), "%s: %s" % (tag, bad)
    # every key sits in its owner's group: ktd::owner_of restated over arrays (tests/test_correct.py), itself held against
    # the library's kt_owner_of on a sample.  (kt_ctr_route partitions by the k-mer's hash; the minimiser owners of
    # tests/shard_ref.py are the routed counter's, checked in test_sharded_route_pass.)
    import test_correct as tc
    own = tc.owner_of(keys, owners)
    step = max(1, len(keys) // 500)
    assert [device.owner_of(int(x), owners) for x in keys[::step]] == own[::step].tolist(), tag
    want_own = np.repeat(np.arange(owners), counts.astype(np.int64))
    bad_at = np.flatnonzero(own != want_own)
    assert not len(bad_at), "%s: key %#x of owner %d in the group of owner %d (%d such keys)" % (
        tag, keys[bad_at[0]], own[bad_at[0]], want_own[bad_at[0]], len(bad_at))


def want_records(oracle, b, k, owners):
    """-> (records per owner, k-mers per owner) of the cut tests/shard_ref.py states - maximal runs of consecutive k-mers of
    one read with one owner (shard_ref.owner_of_kmers), cut every eight k-mers from the run's start - over the oracle's
    k-mers of the whole batch at once (shard_ref.records_of_read, read by read, gives the same: checked on the first reads)"""
    f, _, e = oracle_kmers(oracle, b, k)
    own = shard_ref.owner_of_kmers(f, k, owners)
    rid = np.searchsorted(b.offsets.astype(np.int64), e.astype(np.int64), side="right") - 1
    new = np.ones(len(f), bool)
    new[1:] = (e[1:] != e[:-1] + U(1)) | (rid[1:] != rid[:-1]) | (own[1:] != own[:-1])
    first = np.flatnonzero(new)
    runs = np.diff(np.append(first, len(f)))
    rec = np.bincount(own[first], weights=(runs + shard_ref.REC_KMERS - 1) // shard_ref.REC_KMERS, minlength=owners).astype(np.int64)
    km = np.bincount(own, minlength=owners).astype(np.int64)
    head = np.zeros(owners, np.int64)
    last = min(b.n, 300)
    for s in b.seqs[:last]:
        if len(s) >= k:
            for o, _, n in shard_ref.records_of_read(*shard_ref.codes_of(s), k, owners):
                assert 1 <= n <= shard_ref.REC_KMERS
                head[o] += 1
    m = rid[first] < last
    assert np.array_equal(head, np.bincount(own[first][m], weights=((runs + 7) // 8)[m], minlength=owners).astype(np.int64))
    return rec, km


@pytest.mark.parametrize("owners", [3, 8])
@pytest.mark.parametrize("k", [5, 31])
@pytest.mark.parametrize("family", ["tiny", "empty_runs", "lattice"])
def test_sharded_route_pass(torch_mod, ctx, oracle, monkeypatch, family, k, owners):
    """one rank routing into several owners' regions, the regions counted: the oracle's table, doubled by the same batch
    again.  The k-mers every owner got are those of the restatement; no cut into records of one read's k-mers of one owner,
    eight at most, has fewer records than the restatement's, and none more than one per k-mer."""
    torch = torch_mod
    from kmertools_amd import device
    monkeypatch.setenv("KT_SHARD_FORCE", str(owners))
    monkeypatch.setenv("KT_BULK_MIN_BASES", "0")
    b = route_batch(family, k)
    wk, wc = oracle_table(oracle, b, k)
    want_rec, want_km = memo(("records", b.name, k, owners), lambda: want_records(oracle, b, k, owners))
    assert int(want_km.sum()) == int(wc.sum())
    tag = "sharded, family %s, k = %d, %d owners" % (family, k, owners)
    bv, ov = bases_view(torch, b.bases, 0), offsets_view(torch, b.offsets)
    sh = device.Sharded(ctx, k, 1 << 21, max(b.total, 1), 1, 0, None)
    try:
        for times in (1, 2):
            sh.add_reads(bv, ov, b.n)
            sh.finalize()
            rec, km = sh.route_stats()
            assert np.array_equal(km.astype(np.int64), want_km), (tag, times, km, want_km)
            assert (rec.astype(np.int64) >= want_rec).all() and (rec <= km).all(), (tag, times, rec, want_rec)
            gk, gc = sh.table.export_host()
            bad = table_diff(oracle, b, k, gk, gc, wk, wc, times)
            assert bad is None, "%s, add %d: %s" % (tag, times, bad)
    finally:
        sh.close()


# ---- 6. the kernels that look reads up in a table ------------------------------------------------------------------------------

LOOKUP_K = 21


@pytest.fixture(scope="module")
def lookup(hctx, oracle):
    """per family: the batch, a table of it (every k-mer counted twice, those of a third of the reads four times) as a
    device.Counter, as the oracle's Counter and as sorted arrays"""
    from kmertools_amd import device
    made = {}

    def get(family):
        if family not in made:
            b = family_batch(family, LOOKUP_K)
            third = rb.Batch("third", b.seqs[::3])
            ctr = device.Counter(hctx, LOOKUP_K, 1 << 21)
            oc = oracle.Counter(1)
            for part in (b, b, third, third):
                ctr.add_reads_host(part.bases, part.offsets)
                oc.add_reads(part.bases, part.offsets, LOOKUP_K)
            keys, counts = oc.export(True)
            gk, gc = ctr.export_host()
            assert np.array_equal(gk, keys) and np.array_equal(gc, counts), family
            made[family] = (b, ctr, oc, keys, counts)
        return made[family]

    yield get
    for _, ctr, _, _, _ in made.values():
        ctr.close()


LOOKUP_FAMILIES = ["empty_runs", "empty_runs2", "lattice"]


@pytest.mark.parametrize("family", LOOKUP_FAMILIES)
def test_cov(lookup, family):
    b, ctr, oc, _, _ = lookup(family)
    for dt, norm in (("u32", False), ("f64", True), ("f32", True)):
        want = oc.cov_batch(b.bases, b.offsets, LOOKUP_K, 1, 6, norm)
        got = ctr.cov_host(b.bases, b.offsets, 1, 6, norm, dt)
        if dt == "f32":
            i = first_row_diff(np.abs(got.astype(np.float64) - want) <= 1e-6, np.ones(want.shape, bool))
        else:
            i = first_row_diff(got.view(np.uint64) if dt == "f64" else got.astype(np.float64), want.view(np.uint64) if dt == "f64" else want)
        assert i is None, "cov, family %s, %s: %s; got %s, expected %s" % (family, dt, where(b, i), got[i], want[i])


@pytest.mark.parametrize("family", LOOKUP_FAMILIES)
def test_read_solidity(lookup, oracle, family):
    import test_read_filter as trf
    b, ctr, _, keys, counts = lookup(family)
    table = trf.Table.__new__(trf.Table)
    table.keys, table.counts = keys, counts
    for lo, hi in ((3, U32_MAX), (2, 2)):
        want = trf.want_solidity(oracle, b.seqs, LOOKUP_K, table, lo, hi)
        got = ctr.read_solidity_host(b.bases, b.offsets, lo, hi)
        for name, g, w in zip(("n_kmers", "n_solid", "first_weak"), got, want):
            i = first_row_diff(g, w)
            assert i is None, "read_solidity, family %s, %d..%d, %s: %s; got %d, expected %d" % (
                family, lo, hi, name, where(b, i), g[i], w[i])


@pytest.mark.parametrize("family", LOOKUP_FAMILIES)
def test_profile_and_stats(lookup, hctx, oracle, family):
    import test_profile as tp
    b, ctr, _, keys, counts = lookup(family)
    want = tp.want_profile(oracle, b.seqs, LOOKUP_K, tp.Table(keys, counts))
    got = ctr.profile_host(b.bases, b.offsets)
    i = first_row_diff(got, want)
    assert i is None, "profile, family %s: base %d; %s" % (family, i, where(b, rb.read_of(b, i)))
    wstats = tp.want_stats(want, b.offsets)
    gstats = hctx.profile_stats_host(want, b.offsets)
    for name in tp.NAMES:
        i = first_row_diff(gstats[name], wstats[name])
        assert i is None, "profile_stats, family %s, %s: %s; got %d, expected %d" % (
            family, name, where(b, i), gstats[name][i], wstats[name][i])


@pytest.mark.parametrize("family", LOOKUP_FAMILIES)
def test_correct_support(lookup, oracle, family):
    """the reads with 2 % of their bases substituted, against the table of the reads as they were: the substituted bases are
    covered by no solid window and the base that was there is supported"""
    import test_correct as tc
    from kmertools_amd._lib import KT_MEM_HOST
    b, ctr, _, keys, counts = lookup(family)
    rng = np.random.default_rng(SEED)
    bases = b.bases.copy()
    hit = np.flatnonzero(rng.random(b.total) < 0.02)
    bases[hit] = rb.ACGT[(tc.NT4[bases[hit]] + rng.integers(1, 4, size=len(hit))) & 3]
    table = tc.Table(keys, counts)
    lo, hi = 2, U32_MAX
    prof = tc.want_profile(oracle, bases, b.offsets, LOOKUP_K, table)
    want = tc.want_support(oracle, bases, b.offsets, LOOKUP_K, table, prof, lo, hi)
    assert (want != 0).sum() > 100
    got = np.zeros(b.total, np.uint32)
    ctr.correct_support(bases, b.offsets, b.n, prof, lo, hi, got, KT_MEM_HOST)
    i = first_row_diff(got, want)
    assert i is None, "correct_support, family %s: base %d, got %#x, expected %#x; %s" % (
        family, i, got[i], want[i], where(b, rb.read_of(b, i)))


@pytest.mark.parametrize("family", LOOKUP_FAMILIES)
def test_sketch(hctx, oracle, family):
    import test_sketch as ts
    b = family_batch(family, LOOKUP_K)
    s, seed = 8, 0x5eed
    wh, wz, wn = ts.rows_of(ts.hash_sets(oracle, b.bases, b.offsets, LOOKUP_K, seed), s)
    gh, gz, gn = hctx.sketch_host(b.bases, b.offsets, LOOKUP_K, s, seed)
    for name, g, w in (("n_kmers", gn, wn), ("sizes", gz, wz), ("hashes", gh, wh)):
        i = first_row_diff(g, w)
        assert i is None, "sketch, family %s, %s: %s; got %s, expected %s" % (family, name, where(b, i), g[i], w[i])


# ---- 7. whole-sequence CGR ---------------------------------------------------------------------------------------------------------

def letters_batch(family):
    """family E for kt_cgr_points: letters only (any other byte is an error for the whole call)"""
    def make():
        if family == "tiny":
            b = rb.tiny_batch(SEED, 7, 16000, letters=True)
            b.meta["shape"] = check_dense(b)
        elif family == "empty_runs":
            b = rb.empty_runs_batch(SEED, letters=True)
            assert check_empty_runs(b) >= {(w, r) for w in ("between", "aligned") for r in rb.EMPTY_RUNS}
        else:
            b = rb.lattice_batch(SEED, 7, letters=True, poly_a=True)
            b.meta["shape"] = check_lattice(b, rb.LATTICE, follows_of(7))
            assert [x for x, _ in b.meta["poly_a"]] == [1, 63, 64, 65]
        assert np.isin(b.bases, rb.LETTERS).all()
        return b
    return memo(("letters", family), make)


@pytest.mark.parametrize("vecsize", [1, 16])
@pytest.mark.parametrize("family", ["tiny", "empty_runs", "lattice"])
def test_cgr(hctx, oracle, family, vecsize):
    b = letters_batch(family)
    want = oracle.cgr_batch(b.bases, b.offsets, vecsize)
    got = hctx.cgr_host(b.bases, b.offsets, vecsize)
    i = first_row_diff(got.view(np.uint64), want.view(np.uint64))
    assert i is None, "cgr, family %s, vecsize %d: base %d, got %s, expected %s; %s" % (
        family, vecsize, i, [x.hex() for x in got[i].tolist()], [x.hex() for x in want[i].tolist()], where(b, rb.read_of(b, i)))


# ---- 8. window minimisers --------------------------------------------------------------------------------------------------------

def min_batch(family, w, m):
    """family E for kt_minimisers.  w = 0 (one minimiser per read): the reference defines nothing for a read shorter than m,
    so there every read has m bases more and the runs of empty reads are not part of the case list."""
    def make():
        short = m if w == 0 else 0
        if family == "tiny":
            b = rb.tiny_batch(SEED + m, m, 12000, min_len=short)
            s = rb.shape_numbers(b.offsets)
            assert s["segments_257_512" if short else "segments_over_512"] >= 1, (b.name, s)
            if not short:
                check_dense(b)
        elif family == "empty_runs":
            b = rb.empty_runs_batch(SEED + m)
            assert check_empty_runs(b) >= {(x, r) for x in ("between", "aligned") for r in rb.EMPTY_RUNS}
        else:
            b = rb.lattice_batch(SEED + m, m, poly_a=True, min_len=short)
            check_lattice(b, rb.LATTICE, follows_of(m, short))
        assert not short or b.lens.min() >= m
        return b
    return memo(("min", family, m, w == 0), make)


MIN_CASES = [(family, w, m) for w, m in ((31, 7), (5, 5), (200, 15), (0, 7), (5000, 7))
             for family in (("tiny", "empty_runs", "lattice") if w else ("tiny", "lattice"))]


@pytest.mark.parametrize("family,w,m", MIN_CASES)
def test_minimisers(hctx, oracle, family, w, m):
    b = min_batch(family, w, m)
    wevo, wk, ws, we = memo(("minimisers", b.name, w, m), lambda: rb.oracle_minimisers_flat(oracle, b, w, m))
    evo, gk, gs, ge = hctx.minimisers_host(b.bases, b.offsets, w, m)
    tag = "minimisers, family %s, w = %d, m = %d" % (family, w, m)
    i = first_row_diff(np.diff(evo.astype(np.int64)), np.diff(wevo.astype(np.int64))) if len(wk) or len(gk) else None
    assert i is None, "%s: %d minimisers, expected %d; %s" % (tag, int(evo[i + 1] - evo[i]), int(wevo[i + 1] - wevo[i]), where(b, i))
    j = first_flat_diff((gk, gs, ge), (wk, ws, we))
    if j is not None:
        triple = lambda k_, s_, e_: "(%#x, %d, %d)" % (k_[j], s_[j], e_[j]) if j < len(k_) else "none"   # noqa: E731
        pytest.fail("%s: triple %d (%d found, %d expected): got %s, expected %s; %s" % (
            tag, j, len(gk), len(wk), triple(gk, gs, ge), triple(wk, ws, we),
            where(b, int(np.searchsorted(wevo, j, side="right") - 1))))
