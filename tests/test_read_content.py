"""Every kernel that reads bases, on what the bytes are: all 256 byte values at every position of a 32-base item, alone and
with a raw 0..3 code within 15 bases behind them, in reads of one length and in ragged ones (rb.alphabet_batch), and reads of
nothing but the 14 valid bytes - ACGTUacgtu and the raw codes (rb.valid_mix_batch).

Why: a base is classified in two ways.  ktd::swar4 takes four bytes per instruction (case fold, a v_perm_b32 table compare,
a carry trick) and knows letters only; ktd::nt4 is the per-byte arithmetic form.  Which of them a byte goes through depends
on its neighbours: a 32-base item that holds a raw code is re-encoded whole with nt4 (kt_segment.hpp, two copies), a whole
wave of the oligo kernel switches when one of its lanes holds one (kt_oligo.hip, encode16), kt_min.hip has two SWAR encoders
and a serial nt4 path, kt_cgr.hip a rule of its own (letters only, raw codes are errors) and kt_correct_apply promises to
hand every byte it does not repair through untouched.  The other suites draw their reads from about a dozen byte values and
a raw code in 0.2 % of the bytes: "byte X next to a raw code" is met there for a handful of X by chance.

Every test first asserts, from the bytes and offsets alone, that its batch holds every (value, position mod 32) pair with
valid windows of 31 on both sides (rb.check_alphabet) or all 14 valid bytes and no other (rb.check_valid_mix).  Results
against the CPU oracle, which tests/test_oracle_brute_force.py holds against a brute force on these very batches, and
against the restatements of tests/test_profile.py, test_read_filter.py, test_correct.py, test_sketch.py and shard_ref.py:
integers and f64 bit-exact, f32 within 1e-6.  A failure names the batch, the configuration and the read - in an alphabet
batch a read is a byte value, given as 0x.. - and where there is one the position of the first difference modulo 16 and 32.

Left out, statically: the generic oligo path at k = 12 (256 rows of 64 MB each); the routed counter at k = 31 (its cases took
longer than any of tests/test_read_boundaries.py's - see there; kt_ctr_route and the four counter forms keep k = 31).  The
windows of more than 4096 m-mers (KT_MIN_SERIAL=1) have a batch of their own: none fills in reads of 1104 bases."""
import contextlib
import re

import numpy as np
import pytest

import read_batches as rb
import test_read_boundaries as trb
from read_batches import bases_view, offsets_view
from test_read_boundaries import first_flat_diff, first_row_diff, memo, oracle_kmers, oracle_table, table_diff

pytestmark = pytest.mark.gpu

SEED = 0xb17e
U32_MAX = 0xFFFFFFFF
MIX_READS = 1400                                          # about 280 000 bases, as an alphabet batch
BATCHES = ("alphabet", "alphabet_ragged", "alphabet_raw", "alphabet_raw_ragged", "valid_mix")
ALPHABETS = BATCHES[:4]


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


# ---- the batches, self-checked ------------------------------------------------------------------------------------------------

def batch(name):
    """alphabet[_raw][_ragged] (values: all 256 bytes, or with _letters the ten kt_cgr_points takes), valid_mix, letters_mix,
    valid_mix_min10 (no read shorter than 10 bases: the reference defines no w = 0 minimiser of a shorter one)"""
    def make():
        if name.startswith("alphabet"):
            raw, values = "_raw" in name, rb.LETTERS if "_letters" in name else range(256)
            b = rb.alphabet_batch(SEED + BATCHES.index(name) if name in BATCHES else SEED, raw_neighbour=raw,
                                  ragged="_ragged" in name, values=values)
            assert rb.check_alphabet(b, raw, values) >= 32 * len(values), b.name
            assert (len(set(b.lens)) > 1) == ("_ragged" in name) and b.lens.min() == rb.ALPHA_LEN > 1008
        elif name == "letters_mix":
            b = rb.valid_mix_batch(SEED, MIX_READS, alphabet=rb.LETTERS)
            rb.check_valid_mix(b, rb.LETTERS)
        else:
            short = 10 if name == "valid_mix_min10" else 0
            b = rb.valid_mix_batch(SEED, MIX_READS, min_len=short)
            rb.check_valid_mix(b, min_len=short)
        if "_letters" in name or name == "letters_mix":
            assert np.isin(b.bases, rb.LETTERS).all()
        assert b.total <= 300_000, (b.name, b.total)      # half of tests/test_read_boundaries.py's
        return b
    return memo(("content", name), make)


def occurrences(b):
    """-> (positions [reads, 32] of the byte value of each read of an alphabet batch, the values [reads])"""
    values = np.array(b.meta["values"], np.int64)
    first = b.offsets[1:].astype(np.int64) - rb.ALPHA_LEN + rb.ALPHA_FIRST
    at = first[:, None] + rb.ALPHA_STEP * np.arange(rb.ALPHA_TIMES)[None, :]
    assert (b.bases[at] == values[:, None]).all()
    return at, values


def place(b, i=None, pos=None):
    """for a failure message: the read (rb.where), its byte value in an alphabet batch, the position modulo 16 and 32"""
    if i is None:
        i = rb.read_of(b, min(int(pos), max(b.total - 1, 0)))
    out = rb.where(b, i)
    if "values" in b.meta and 0 <= i < b.n:
        out = "byte %#04x; %s" % (b.meta["values"][i], out)
    if pos is not None:
        out += "; position %d = %d mod 16, %d mod 32, base %d of its read" % (pos, pos % 16, pos % 32, pos - int(b.offsets[i]))
    return out


@contextlib.contextmanager
def naming(b, tag=""):
    """the comparers of the other suites name a read by its index: in an alphabet batch, add the byte value it stands for"""
    try:
        yield
    except (pytest.fail.Exception, AssertionError) as e:
        m = re.search(r"read (\d+) of %d" % b.n, str(e))
        raise AssertionError("%s %s: %s\n%s" % (b.name, tag, place(b, int(m.group(1))) if m else "", e)) from None


# ---- 1. kt_kmers --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", [1, 4, 15, 16, 17, 31])
@pytest.mark.parametrize("name", BATCHES)
def test_kmers(hctx, oracle, name, k):
    b = batch(name)
    want = oracle_kmers(oracle, b, k)
    gf, gr, ge = hctx.kmers_host(b.bases, b.offsets, k)
    j = first_flat_diff((ge, gf, gr), (want[2], want[0], want[1]))
    if j is not None:
        pos = min(int(ge[j]) if j < len(ge) else b.total, int(want[2][j]) if j < len(want[2]) else b.total)
        pytest.fail("kmers, %s, k = %d: k-mer %d differs (%d found, %d expected), the first ends at %s" % (
            b.name, k, j, len(ge), len(want[2]), place(b, pos=pos)))


# ---- 2. the LDS oligo kernel (k = 3..7) ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("k,count_min", trb.OLIGO_CASES)
@pytest.mark.parametrize("name", BATCHES)
def test_oligo_lds(torch_mod, oracle, monkeypatch, name, k, count_min):
    """u32 and f64 rows at the library's own tile size from a base pointer 0 and 1 past a 256-byte boundary, at k = 7 with and
    without the producer wave; f32 and the call through host arrays once.  The reads of one length take the equal-length
    path, the ragged ones the general one; both exceed the 1008-byte chunk."""
    torch = torch_mod
    b = batch(name)
    want = trb.OligoWant(torch, oracle, b, k, count_min)
    ov = offsets_view(torch, b.offsets)
    for shift in (0, 1):
        bv = bases_view(torch, b.bases, shift)
        for pw in (7, 8) if k == 7 else (None,):
            c = trb.oligo_context(monkeypatch, torch, None, pw)
            try:
                tag = "%s, k = %d, count_min = %s, shift %d, KT_OLIGO_PW = %s" % (b.name, k, count_min, shift, pw)
                once = shift == 0 and pw != 8
                with naming(b, tag):
                    trb.oligo_compare(torch, c, b, bv, ov, k, count_min, want, ("u32", "f64") + (("f32",) if once else ()), tag)
                    if once:
                        trb.oligo_compare_host(c, b, k, count_min, want, tag)
            finally:
                c.close()


# ---- 3. the generic oligo path (rows in global memory): k = 1, 2, 8 -------------------------------------------------------------

@pytest.mark.parametrize("count_min", [True, False])
@pytest.mark.parametrize("k", [1, 2, 8])
@pytest.mark.parametrize("name", BATCHES)
def test_oligo_generic(torch_mod, ctx, oracle, name, k, count_min):
    """u32 and f64 rows, compared cell by cell through the non-zero cells (k = 12: 256 rows of 64 MB, left out)"""
    torch = torch_mod
    from kmertools_amd import device
    b = batch(name)
    bins = device.bins(k, count_min)
    assert bins == trb.oligo_bins(k, count_min)
    cells, counts, totals = trb.sparse_rows(oracle, b, k, count_min)
    bv, ov = bases_view(torch, b.bases, 0), offsets_view(torch, b.offsets)
    try:
        for dt in ("u32", "f64"):
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
                pytest.fail("generic oligo, %s, k = %d, count_min = %s, %s: non-zero cell %d differs (%d found, %d expected), "
                            "bin %d; %s" % (b.name, k, count_min, dt, j, len(got_cells), len(cells), cell % bins,
                                            place(b, min(cell // bins, b.n - 1))))
    finally:
        torch.cuda.empty_cache()


# ---- 4. counting --------------------------------------------------------------------------------------------------------------

CTR_CASES = [(form, k) for form in ("incremental", "packed", "staged") for k in (4, 15, 16, 17, 31)] + [("direct", 8)]


@pytest.mark.parametrize("form,k", CTR_CASES)
@pytest.mark.parametrize("name", BATCHES)
def test_counter(torch_mod, ctx, oracle, monkeypatch, name, form, k):
    """the incremental path, the bulk build over packed and over staged reads, a direct-addressed table: the oracle's table;
    the same batch again doubles it"""
    torch = torch_mod
    from kmertools_amd import device
    for var, val in trb.CTR_ENV[form].items():
        monkeypatch.setenv(var, val)
    b = batch(name)
    wk, wc = oracle_table(oracle, b, k)
    bv, ov = bases_view(torch, b.bases, 0), offsets_view(torch, b.offsets)
    ctr = device.Counter(ctx, k, 4 ** k if form == "direct" else 1 << 21)
    try:
        for times in (1, 2):
            ctr.add_reads(bv, ov, b.n)
            gk, gc = ctr.export_host()
            tag = "counter (%s), k = %d, add %d" % (form, k, times)
            with naming(b, tag):
                bad = table_diff(oracle, b, k, gk, gc, wk, wc, times)
                assert bad is None, "%s: %s%s" % (tag, bad, end_position(bad))
    finally:
        ctr.close()


def end_position(msg):
    """table_diff names the base a k-mer ends at: that position modulo 16 and 32"""
    m = re.search(r"ends at base (\d+)", msg or "")
    return "; it ends at %d mod 16, %d mod 32" % (int(m.group(1)) % 16, int(m.group(1)) % 32) if m else ""


# ---- 5. the route kernel and the routed (sharded) counter ------------------------------------------------------------------------

OWNERS = 3


@pytest.mark.parametrize("k", [5, 31])
@pytest.mark.parametrize("name", BATCHES)
def test_route(hctx, oracle, name, k):
    """kt_ctr_route: the canonical k-mers of the oracle, each once, grouped by owner (as test_read_boundaries.py's test_route)"""
    import test_correct as tc
    from kmertools_amd import device
    b = batch(name)
    f, r, e = oracle_kmers(oracle, b, k)
    canon = np.minimum(f, r)
    keys, counts = hctx.route_host(b.bases, b.offsets, k, OWNERS)
    tag = "route, k = %d, %d owners" % (k, OWNERS)
    gk, gc = np.unique(keys, return_counts=True)
    wk, wc = np.unique(canon, return_counts=True)
    with naming(b, tag):
        bad = table_diff(oracle, b, k, gk, gc.astype(np.uint32), wk, wc.astype(np.uint32))
        assert bad is None and int(counts.sum()) == len(canon), "%s: %s%s" % (tag, bad, end_position(bad))
    own = tc.owner_of(keys, OWNERS)
    step = max(1, len(keys) // 500)
    assert [device.owner_of(int(x), OWNERS) for x in keys[::step]] == own[::step].tolist(), (b.name, tag)
    want_own = np.repeat(np.arange(OWNERS), counts.astype(np.int64))
    bad_at = np.flatnonzero(own != want_own)
    assert not len(bad_at), "%s, %s: key %#x of owner %d in the group of owner %d (%d such keys)" % (
        b.name, tag, keys[bad_at[0]], own[bad_at[0]], want_own[bad_at[0]], len(bad_at))


# k = 5 alone: at k = 31 the restatement of the records (shard_ref.records_of_read over 256 reads of 1104 bases) made every case
# take 0.85 s where the slowest routed-counter case of tests/test_read_boundaries.py takes 0.79 s; kt_ctr_route above and the
# counter forms keep k = 31
@pytest.mark.parametrize("k", [5])
@pytest.mark.parametrize("name", BATCHES)
def test_sharded_route_pass(torch_mod, ctx, oracle, monkeypatch, name, k):
    """one rank routing into three owners' regions, the regions counted: the oracle's table, doubled by the same batch again;
    the k-mers every owner got and the bounds on its records as test_read_boundaries.py's test_sharded_route_pass has them"""
    torch = torch_mod
    from kmertools_amd import device
    monkeypatch.setenv("KT_SHARD_FORCE", str(OWNERS))
    monkeypatch.setenv("KT_BULK_MIN_BASES", "0")
    b = batch(name)
    wk, wc = oracle_table(oracle, b, k)
    want_rec, want_km = memo(("records", b.name, k, OWNERS), lambda: trb.want_records(oracle, b, k, OWNERS))
    assert int(want_km.sum()) == int(wc.sum())
    tag = "sharded, k = %d, %d owners" % (k, OWNERS)
    bv, ov = bases_view(torch, b.bases, 0), offsets_view(torch, b.offsets)
    sh = device.Sharded(ctx, k, 1 << 21, max(b.total, 1), 1, 0, None)
    try:
        for times in (1, 2):
            sh.add_reads(bv, ov, b.n)
            sh.finalize()
            rec, km = sh.route_stats()
            assert np.array_equal(km.astype(np.int64), want_km), (b.name, tag, times, km, want_km)
            assert (rec.astype(np.int64) >= want_rec).all() and (rec <= km).all(), (b.name, tag, times, rec, want_rec)
            gk, gc = sh.table.export_host()
            with naming(b, tag):
                bad = table_diff(oracle, b, k, gk, gc, wk, wc, times)
                assert bad is None, "%s, add %d: %s%s" % (tag, times, bad, end_position(bad))
    finally:
        sh.close()


# ---- 6. the kernels that look reads up in a table ------------------------------------------------------------------------------

LOOKUP_K = 21


@pytest.fixture(scope="module")
def lookup(hctx, oracle):
    """per batch: the batch, a table of it (every k-mer counted twice) as a device.Counter, as the oracle's Counter and as
    sorted arrays"""
    from kmertools_amd import device
    made, counters = {}, []

    def get(name):
        if name not in made:
            b = batch(name)
            ctr = device.Counter(hctx, LOOKUP_K, 1 << 21)
            counters.append(ctr)                          # (closed below even when the table is not the oracle's: never left to the
            oc = oracle.Counter(1)                        # garbage collector, which may run after the context is gone)
            for _ in range(2):
                ctr.add_reads_host(b.bases, b.offsets)
                oc.add_reads(b.bases, b.offsets, LOOKUP_K)
            keys, counts = oc.export(True)
            gk, gc = ctr.export_host()
            assert np.array_equal(gk, keys) and np.array_equal(gc, counts) and (counts >= 2).all(), b.name
            made[name] = (b, ctr, oc, keys, counts)
        return made[name]

    yield get
    for ctr in counters:
        ctr.close()


@pytest.mark.parametrize("name", BATCHES)
def test_cov(lookup, name):
    b, ctr, oc, _, _ = lookup(name)
    for dt, norm in (("u32", False), ("f64", True), ("f32", True)):
        want = oc.cov_batch(b.bases, b.offsets, LOOKUP_K, 1, 6, norm)
        got = ctr.cov_host(b.bases, b.offsets, 1, 6, norm, dt)
        if dt == "f32":
            i = first_row_diff(np.abs(got.astype(np.float64) - want) <= 1e-6, np.ones(want.shape, bool))
        else:
            i = first_row_diff(got.view(np.uint64) if dt == "f64" else got.astype(np.float64), want.view(np.uint64) if dt == "f64" else want)
        assert i is None, "cov, %s, %s: %s; got %s, expected %s" % (b.name, dt, place(b, i), got[i], want[i])


@pytest.mark.parametrize("name", BATCHES)
def test_read_solidity(lookup, oracle, name):
    import test_read_filter as trf
    b, ctr, _, keys, counts = lookup(name)
    table = trf.Table.__new__(trf.Table)
    table.keys, table.counts = keys, counts
    for lo, hi in ((3, U32_MAX), (2, 2)):
        want = trf.want_solidity(oracle, b.seqs, LOOKUP_K, table, lo, hi)
        got = ctr.read_solidity_host(b.bases, b.offsets, lo, hi)
        for what, g, w in zip(("n_kmers", "n_solid", "first_weak"), got, want):
            i = first_row_diff(g, w)
            assert i is None, "read_solidity, %s, %d..%d, %s: %s; got %d, expected %d" % (
                b.name, lo, hi, what, place(b, i), g[i], w[i])


@pytest.mark.parametrize("name", BATCHES)
def test_profile_and_stats(lookup, hctx, oracle, name):
    import test_profile as tp
    b, ctr, _, keys, counts = lookup(name)
    want = tp.want_profile(oracle, b.seqs, LOOKUP_K, tp.Table(keys, counts))
    got = ctr.profile_host(b.bases, b.offsets)
    i = first_row_diff(got, want)
    assert i is None, "profile, %s: got %#x, expected %#x; %s" % (b.name, got[i], want[i], place(b, pos=i))
    wstats = tp.want_stats(want, b.offsets)
    gstats = hctx.profile_stats_host(want, b.offsets)
    for what in tp.NAMES:
        i = first_row_diff(gstats[what], wstats[what])
        assert i is None, "profile_stats, %s, %s: %s; got %d, expected %d" % (
            b.name, what, place(b, i), gstats[what][i], wstats[what][i])


def substituted(b, protect=None):
    """the bases with 2 % of the valid ones substituted as test_read_boundaries.py's test_correct_support does; the positions
    in `protect` (the occurrences of an alphabet batch's byte values and their raw codes) stay as they are"""
    import test_correct as tc
    rng = np.random.default_rng(SEED)
    bases = b.bases.copy()
    ok = tc.NT4[bases] < 4
    if protect is not None:
        ok[protect] = False
    hit = np.flatnonzero((rng.random(b.total) < 0.02) & ok)
    bases[hit] = rb.ACGT[(tc.NT4[bases[hit]] + rng.integers(1, 4, size=len(hit))) & 3]
    return bases, hit


def protected(b):
    """an alphabet batch's occurrences and the 15 bases behind each (where its raw code is, if it has one)"""
    at, _ = occurrences(b)
    return (at[:, :, None] + np.arange(16)[None, None, :]).ravel()


@pytest.mark.parametrize("name", BATCHES)
def test_correct_support(lookup, oracle, name):
    """the reads with 2 % of their valid bases substituted, against the table of the reads as they were: the substituted
    bases are covered by no solid window and the base that was there is supported"""
    import test_correct as tc
    from kmertools_amd._lib import KT_MEM_HOST
    b, ctr, _, keys, counts = lookup(name)
    bases, hit = substituted(b, protected(b) if name in ALPHABETS else None)
    if name in ALPHABETS:
        at, values = occurrences(b)
        assert np.array_equal(bases[at], b.bases[at]) and (bases[at] == values[:, None]).all()
    table = tc.Table(keys, counts)
    lo, hi = 2, U32_MAX
    prof = tc.want_profile(oracle, bases, b.offsets, LOOKUP_K, table)
    want = tc.want_support(oracle, bases, b.offsets, LOOKUP_K, table, prof, lo, hi)
    assert len(hit) > 1000 and (want[hit] != 0).sum() > 100
    got = np.zeros(b.total, np.uint32)
    ctr.correct_support(bases, b.offsets, b.n, prof, lo, hi, got, KT_MEM_HOST)
    i = first_row_diff(got, want)
    assert i is None, "correct_support, %s: got %#x, expected %#x; %s" % (b.name, got[i], want[i], place(b, pos=i))


@pytest.mark.parametrize("name", ALPHABETS)
def test_correct_support_at_the_byte_itself(hctx, oracle, name):
    """the candidates at the byte value itself.  The table also holds the reads with every occurrence i of byte v replaced by
    "ACGT"[(v + i) & 3], and the profile is made up to leave half of the occurrences uncovered (windows of a valid v are solid:
    from the real profile it would never be looked at).  An invalid byte then gets support for each of the four nucleotides,
    a u, a T or a raw 3 for the other three alone - although the windows with T there are solid."""
    import test_correct as tc
    from kmertools_amd import device
    from kmertools_amd._lib import KT_MEM_HOST
    b = batch(name)
    at, values = occurrences(b)
    repaired = b.bases.copy()
    repaired[at] = rb.ACGT[(values[:, None] + np.arange(rb.ALPHA_TIMES)[None, :]) & 3]
    ctr = device.Counter(hctx, LOOKUP_K, 1 << 21)
    try:
        oc = oracle.Counter(1)
        for part in (b.bases, b.bases, repaired, repaired):
            ctr.add_reads_host(part, b.offsets)
            oc.add_reads(part, b.offsets, LOOKUP_K)
        table = tc.Table(*oc.export(True))
        bases, lo, hi = b.bases, 2, U32_MAX
        prof = tc.want_profile(oracle, bases, b.offsets, LOOKUP_K, table)
        open_at = at[:, np.arange(rb.ALPHA_TIMES) % 8 < 4]    # half of the occurrences (every i mod 4): no window over them is solid
        prof[(open_at[:, :, None] - np.arange(LOOKUP_K)[None, None, :]).ravel()] = tc.NO
        want = tc.want_support(oracle, bases, b.offsets, LOOKUP_K, table, prof, lo, hi)
        by = (want[open_at][:, :, None] >> np.array([0, 8, 16, 24], np.uint32)[None, None, :]) & np.uint32(255)   # [read, occurrence, x]
        code = tc.NT4[values]
        assert (by[code == 4].max(axis=1) > 0).all(), "an invalid byte: every nucleotide is a candidate somewhere"
        for v in (ord("u"), ord("U"), ord("T"), ord("t"), 3):
            assert not by[v, :, 3].any() and (by[v].max(axis=0)[:3] > 0).all(), "%#04x: the other three alone" % v
        got = np.zeros(b.total, np.uint32)
        ctr.correct_support(bases, b.offsets, b.n, prof, lo, hi, got, KT_MEM_HOST)
        i = first_row_diff(got, want)
        assert i is None, "correct_support, %s, made-up profile: got %#x, expected %#x; %s" % (b.name, got[i], want[i], place(b, pos=i))
    finally:
        ctr.close()


# ---- 7. kt_correct_apply: what it does not repair comes out byte for byte ----------------------------------------------------------

@pytest.mark.parametrize("name", ALPHABETS)
def test_correct_apply(torch_mod, ctx, name):
    """a made-up support array (no, one, several candidates, by seed); at every fourth occurrence of a byte value it is zero
    (the byte comes out as it went in - checked for all 256), at the next it names one candidate, at the next two"""
    import test_correct as tc
    from kmertools_amd._lib import KT_MEM_HOST
    torch = torch_mod
    b = batch(name)
    at, values = occurrences(b)
    rng = np.random.default_rng(SEED + 1)
    sup = tc.pattern_support(rng, b.total, np.array([0, 1, 2, 3, 21, 255]))
    sup[at[:, 0::4]] = 0
    sup[at[:, 1::4]] = (np.uint32(1) << (8 * rng.integers(0, 4, size=at[:, 1::4].shape)).astype(np.uint32))
    sup[at[:, 2::4]] = 0x00020100 | (np.uint32(5) << (8 * rng.integers(0, 4, size=at[:, 2::4].shape)).astype(np.uint32))
    busy = int(np.median(tc.want_apply(b.bases, b.offsets, sup)[1]))     # (half of the reads have more single bases: left alone)
    settings = ((1, 0), (2, 0), (1, busy))
    for ms, mc in settings:
        out, ns, na = tc.want_apply(b.bases, b.offsets, sup, ms, mc)
        assert (out[at[:, 0::4]] == values[:, None]).all() and len(set(out[at[:, 0]].tolist())) == 256
        assert ns.any() and na.any() and (out != b.bases).any()
        if mc == 0 and ms == 1:
            assert np.isin(out[at[:, 1::4]], rb.ACGT).all()
    with naming(b, "correct_apply"):
        tc.check_apply(torch, ctx, b.bases, b.offsets, sup, b.name, settings)
    want = tc.want_apply(b.bases, b.offsets, sup, 1, 0)[0]    # in place, host and device
    inplace = b.bases.copy()
    ctx.correct_apply(inplace, b.offsets, b.n, sup, 1, 0, inplace, None, None, KT_MEM_HOST)
    dinplace = tc.dev(torch, b.bases)
    ctx.correct_apply(dinplace, tc.dev(torch, b.offsets), b.n, tc.dev(torch, sup), 1, 0, dinplace, None, None)
    torch.cuda.synchronize()
    for how, got in (("host", inplace), ("device", dinplace.cpu().numpy())):
        i = first_row_diff(got, want)
        assert i is None, "correct_apply in place (%s), %s: got %#04x, expected %#04x; %s" % (how, b.name, got[i], want[i], place(b, pos=i))


# ---- 8. sketches ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("s", [16, 1000])
@pytest.mark.parametrize("name", BATCHES)
def test_sketch(hctx, oracle, name, s):
    import test_sketch as ts
    b = batch(name)
    seed = 0x5eed
    sets = memo(("hash_sets", b.name), lambda: ts.hash_sets(oracle, b.bases, b.offsets, LOOKUP_K, seed))
    wh, wz, wn = ts.rows_of(sets, s)
    gh, gz, gn = hctx.sketch_host(b.bases, b.offsets, LOOKUP_K, s, seed)
    for what, g, w in (("n_kmers", gn, wn), ("sizes", gz, wz), ("hashes", gh, wh)):
        i = first_row_diff(g, w)
        assert i is None, "sketch, %s, s = %d, %s: %s; got %s, expected %s" % (b.name, s, what, place(b, i), g[i], w[i])


# ---- 9. window minimisers --------------------------------------------------------------------------------------------------------

# w = 0: the window is the whole read, which in an alphabet batch only the 14 reads of a valid byte ever fill - the other 242
# answer with the reference's "none" triple (what they check is where the last invalid byte is); the valid mix fills every one
MIN_CASES = [(31, 7), (12, 3), (0, 10)]
NONE_KMER = 0xFFFFFFFFFFFFFFFF


def minimisers_compare(hctx, oracle, b, w, m, tag):
    """-> the oracle's minimisers (for what the caller asserts about them)"""
    wevo, wk, ws, we = memo(("minimisers", b.name, w, m), lambda: rb.oracle_minimisers_flat(oracle, b, w, m))
    evo, gk, gs, ge = hctx.minimisers_host(b.bases, b.offsets, w, m)
    i = first_row_diff(np.diff(evo.astype(np.int64)), np.diff(wevo.astype(np.int64)))
    assert i is None, "%s: %d minimisers, expected %d; %s" % (tag, int(evo[i + 1] - evo[i]), int(wevo[i + 1] - wevo[i]), place(b, i))
    j = first_flat_diff((gk, gs, ge), (wk, ws, we))
    if j is not None:
        triple = lambda k_, s_, e_: "(%#x, %d, %d)" % (k_[j], s_[j], e_[j]) if j < len(k_) else "none"   # noqa: E731
        i = min(int(np.searchsorted(wevo, j, side="right") - 1), b.n - 1)
        pos = int(b.offsets[i]) + int(min(gs[j] if j < len(gs) else ws[j], ws[j] if j < len(ws) else gs[j]))
        pytest.fail("%s: triple %d (%d found, %d expected): got %s, expected %s; its window starts at %s" % (
            tag, j, len(gk), len(wk), triple(gk, gs, ge), triple(wk, ws, we), place(b, i, pos)))
    return wevo, wk


@pytest.mark.parametrize("w,m", MIN_CASES)
@pytest.mark.parametrize("name", BATCHES)
def test_minimisers(hctx, oracle, monkeypatch, name, w, m):
    monkeypatch.delenv("KT_MIN_SERIAL", raising=False)
    b = batch("valid_mix_min10" if name == "valid_mix" and w == 0 else name)
    wevo, wk = minimisers_compare(hctx, oracle, b, w, m, "minimisers, %s, w = %d, m = %d" % (b.name, w, m))
    real = int((wk != np.uint64(NONE_KMER)).sum())
    assert real >= (b.n if w else 14), (b.name, w, m, real)


SERIAL_W, SERIAL_STRETCH = 5000, 12000


@pytest.mark.parametrize("m", [7, 31])
def test_minimisers_serial(hctx, oracle, monkeypatch, m):
    """KT_MIN_SERIAL=1 chooses the one-read-per-thread iterator (min_serial_kernel: nt4 byte by byte) for windows of more
    than 4096 m-mers only, and a window that never fills emits no minimiser value at all.  So this case has a batch of its
    own (rb.long_stretch_batch): stretches of 12000 valid bytes, each of which fills a window of 5000 seven thousand times,
    with all 256 byte values between them.  Asserted before the launch: every long read has real minimisers - at m = 31 five
    at least and 40 different ones in the batch, each a function of the codes nt4 gives 31 of the 14 valid bytes; at m = 7
    (32-bit m-mers) the least of 5000 random 7-mers is one of a few - and every byte value lies between two stretches.
    (One thread walks a whole read: 0.1 to 0.3 s here.  tests/test_read_boundaries.py has no case of this kernel; those of
    tests/test_gpu_parity.py's test_minimisers_windows_wider_than_4096 take 3 to 50 s.)"""
    monkeypatch.setenv("KT_MIN_SERIAL", "1")
    b = memo(("content", "long_stretch"), lambda: rb.long_stretch_batch(SEED, SERIAL_STRETCH))
    rb.check_long_stretch(b, SERIAL_W)
    assert b.total <= 300_000 and SERIAL_W - m + 1 > 4096
    wevo, wk, _, _ = memo(("minimisers", b.name, SERIAL_W, m), lambda: rb.oracle_minimisers_flat(oracle, b, SERIAL_W, m))
    per_read = np.diff(wevo.astype(np.int64))
    long_reads = b.lens > 2 * SERIAL_W
    assert not (wk[np.repeat(long_reads, per_read)] == np.uint64(NONE_KMER)).any() and long_reads.sum() >= 6, b.name
    assert (per_read[long_reads] >= (5 if m == 31 else 2)).all() and len(np.unique(wk)) >= (40 if m == 31 else 3), (b.name, per_read)
    minimisers_compare(hctx, oracle, b, SERIAL_W, m, "minimisers, %s, w = %d, m = %d, KT_MIN_SERIAL = 1" % (b.name, SERIAL_W, m))


# ---- 10. whole-sequence CGR: a rule of its own ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("vecsize", [1, 16])
@pytest.mark.parametrize("name", ["alphabet_letters", "alphabet_letters_ragged", "letters_mix"])
def test_cgr_letters(hctx, oracle, name, vecsize):
    b = batch(name)
    want = oracle.cgr_batch(b.bases, b.offsets, vecsize)
    got = hctx.cgr_host(b.bases, b.offsets, vecsize)
    i = first_row_diff(got.view(np.uint64), want.view(np.uint64))
    assert i is None, "cgr, %s, vecsize %d: got %s, expected %s; %s" % (
        b.name, vecsize, [x.hex() for x in got[i].tolist()], [x.hex() for x in want[i].tolist()], place(b, pos=i))


def test_cgr_every_other_byte_is_an_error(torch_mod, ctx, hctx):
    """each of the 246 bytes outside ACGTUacgtu - the raw codes 0..3 among them - twice, 9 bases apart, in the second of three
    reads of letters: host arrays, KT_ERR_BADNT and the position of the first; device buffers (eight of the values), KT_OK
    and the same position in bad_pos once the stream has run"""
    torch = torch_mod
    from kmertools_amd import _lib
    rng = np.random.default_rng(SEED)
    lens = np.array([70, 300, 45])
    offsets = np.concatenate(([0], np.cumsum(lens))).astype(np.uint64)
    clean = rb.LETTERS[rng.integers(0, len(rb.LETTERS), size=int(lens.sum()))]
    others = [v for v in range(256) if v not in set(rb.LETTERS.tolist())]
    spots = {v: 70 + 3 + v for v in others}               # 246 positions in a row, 9 more stay inside the second read
    assert len(others) == 246 and {p % 8 for p in spots.values()} == set(range(8)) and {p % 128 for p in spots.values()} == set(range(128))
    assert max(spots.values()) + 9 < 370 and all(v in others for v in (0, 1, 2, 3, 0xFF))
    dov = torch.from_numpy(offsets.astype(np.int64)).cuda()
    xy = torch.zeros((len(clean), 2), dtype=torch.float64, device="cuda")
    on_device = (0, 3, ord("N"), 0x40, 0x7B, 0xC1, 0xF5, 0xFF)
    assert all(v in spots for v in on_device)
    for v in others:
        bases = clean.copy()
        bases[spots[v]] = bases[spots[v] + 9] = v
        tag = "cgr, byte %#04x at %d = %d mod 8, %d mod 128 and 9 bases on" % (v, spots[v], spots[v] % 8, spots[v] % 128)
        bad = np.full(1, 12345, np.uint64)
        with pytest.raises(_lib.KmertoolsError) as err:
            hctx.cgr(bases, offsets, 3, 1, np.zeros((len(bases), 2), np.float64), bad, _lib.KT_MEM_HOST)
        assert err.value.code == _lib.KT_ERR_BADNT and int(bad[0]) == spots[v], (tag, "host arrays", err.value.code, int(bad[0]))
        if v in on_device:
            dbad = torch.full((1,), 12345, dtype=torch.int64, device="cuda")
            ctx.cgr(torch.from_numpy(bases).cuda(), dov, 3, 1, xy, dbad)      # (raises on anything but KT_OK)
            torch.cuda.synchronize()
            assert int(dbad.cpu().numpy().view(np.uint64)[0]) == spots[v], (tag, "device buffers")
    bad = np.full(1, 12345, np.uint64)                    # and the letters alone are none
    hctx.cgr(clean, offsets, 3, 1, np.zeros((len(clean), 2), np.float64), bad, _lib.KT_MEM_HOST)
    assert int(bad[0]) == 2 ** 64 - 1
