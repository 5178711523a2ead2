"""Table files on the GPU: Counter.save's bytes against the numpy restatement (tests/ktab_ref.py) over key sizes, entry
counts around every tile size of the pack kernels, bucket patterns, count edges and every table form; Counter.add_file /
from_file against table_model.Model through the table's readers, appended sections, forced S; every content corruption is
refused by name with the table left as it was; the argument and file errors.  Every comparison is exact."""
import os
import struct
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import graph_ref as gr  # noqa: E402
import ktab_ref as R  # noqa: E402
from table_model import Model, canonical_keys  # noqa: E402
from test_ctr_setop import FORMS, Table, sample_pair, snapshot, table_in_form  # noqa: E402

U32 = 0xFFFFFFFF
# the pack kernels' tiles: a wave (64), a workgroup (256), a scan tile (1024), a wave tile of the sort (4096)
SIZES = (0, 1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097)
EDGE_COUNTS = np.array([1, 254, 255, 256, 65535, 65536, U32], np.uint32)


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


def all_canonical(k):
    x = np.arange(1 << (2 * k), dtype=np.uint64)
    return x[x <= gr.rc_np(x, k)]


def some_keys(rng, k, n):
    if 2 * k <= 24:
        pool = all_canonical(k)
        return np.sort(rng.choice(pool, min(n, len(pool)), replace=False))
    return canonical_keys(rng, k, n)


def pairs_table(ctx, k, keys, counts, slots=None):
    from kmertools_amd import device
    c = device.Counter(ctx, k, slots or max(1 << 12, 2 * len(keys)))
    c.add_pairs_host(np.asarray(keys, np.uint64), np.asarray(counts, np.uint32))
    return c


def saved_bytes(c, path, **kw):
    n = c.save(path, **kw)
    data = open(path, "rb").read()
    os.unlink(path)
    return n, data


def check_save(ctx, tmp_path, k, keys, counts, tag):
    c = pairs_table(ctx, k, keys, counts)
    n, data = saved_bytes(c, tmp_path / "t.ktab")
    c.close()
    want = R.encode(k, keys, counts)
    assert n == len(keys), tag
    assert len(data) == R.FILE_HDR + R.section_size(k, len(keys), int((np.asarray(counts) >= 255).sum())), tag
    assert data == want, tag


# ---- bytes ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", [1, 3, 4, 12, 15, 16, 17, 21, 31])
def test_save_bytes_every_k_and_size(ctx, tmp_path, k):
    rng = np.random.default_rng(100 + k)
    seen_p = set()
    for n in SIZES:
        keys = some_keys(rng, k, n)
        counts = rng.choice(EDGE_COUNTS, len(keys))
        check_save(ctx, tmp_path, k, keys, counts, (k, n))
        seen_p.add(R.prefix_bits(k, R.pick_s(k, len(keys))) > 0)
    if k >= 12:
        assert seen_p == {False, True}  # sizes with P = 0 and sizes with P > 0


def test_save_direct_addressed_table(ctx, tmp_path):
    from kmertools_amd import device
    for k in (6, 8):
        rng = np.random.default_rng(k)
        keys = some_keys(rng, k, 100)
        counts = rng.choice(EDGE_COUNTS, len(keys))
        c = device.Counter(ctx, k, 4 ** k)
        assert c.capacity() == 4 ** k
        c.add_pairs_host(keys, counts)
        assert saved_bytes(c, tmp_path / "t.ktab")[1] == R.encode(k, keys, counts)
        c.close()


def test_bucket_patterns(ctx, tmp_path):
    rng = np.random.default_rng(12)
    # k = 13 (B = 26): n = 2000 gives t = 8, S = 3, P = 2 - four buckets, by the first base
    k, n = 13, 2000
    assert (R.pick_s(k, n), R.prefix_bits(k, 3)) == (3, 2)
    pool = canonical_keys(rng, k, 40000)
    bucket = (pool >> np.uint64(24)).astype(np.int64)
    first, last = pool[bucket == 0], pool[bucket == 3]
    assert len(first) >= n and len(last) >= n
    cases = {
        "all in bucket 0": rng.choice(first, n, replace=False),
        "all in the last bucket": rng.choice(last, n, replace=False),
        "first and last only": np.concatenate([rng.choice(first, n // 2, replace=False), rng.choice(last, n // 2, replace=False)]),
    }
    for name, keys in cases.items():
        keys = np.sort(keys)
        check_save(ctx, tmp_path, k, keys, rng.integers(1, 300, len(keys)).astype(np.uint32), name)
    # empty runs longer than a workgroup's 256 buckets, in the middle and at the end: k = 21 (B = 42), n = 70000 gives
    # t = 14, S = 4, P = 10 - 1024 buckets of 2^32 keys, of which 100..499 and 600..1023 stay empty
    k, n = 21, 70000
    assert (R.pick_s(k, n), R.prefix_bits(k, 4)) == (4, 10)
    pool = canonical_keys(rng, k, 600000)
    b = (pool >> np.uint64(32)).astype(np.int64)
    pool = pool[(b < 100) | ((b >= 500) & (b < 600))]
    assert len(pool) >= n
    keys = np.sort(rng.choice(pool, n, replace=False))
    assert (keys >> np.uint64(32)).max() >= 500
    check_save(ctx, tmp_path, k, keys, rng.integers(1, 300, n).astype(np.uint32), "long empty runs")
    # every bucket occupied: k = 8 (B = 16), n = 2048 gives t = 8, S = 1, P = 8; bucket TTTT holds one canonical k-mer only
    # (TTTTAAAA), so "exactly one key in every bucket" is the restatement's file with a forced S (test_load_forced_S)
    k = 8
    pool = all_canonical(k)
    keys = np.sort(np.concatenate([pool[(pool >> np.uint64(8)) == np.uint64(p)][:9] for p in range(256)]))
    assert (R.pick_s(k, len(keys)), len(np.unique(keys >> np.uint64(8)))) == (1, 256)
    check_save(ctx, tmp_path, k, keys, rng.integers(1, 300, len(keys)).astype(np.uint32), "every bucket occupied")


def test_counts(ctx, tmp_path):
    k = 17
    rng = np.random.default_rng(17)
    keys = canonical_keys(rng, k, 4200)
    n = len(keys)
    no_escapes = rng.integers(1, 255, n).astype(np.uint32)
    only_escapes = rng.choice(np.array([255, 256, 65535, 65536, U32], np.uint32), n)
    borders = np.ones(n, np.uint32)
    for t in (64, 256, 1024, 4096):  # escapes on both sides of every tile border
        for m in range(t, n, t):
            borders[m - 1], borders[m] = 255 + (m % 7), U32 - (m % 5)
    for name, counts in (("no escapes", no_escapes), ("only escapes", only_escapes), ("borders", borders),
                         ("edges", np.resize(EDGE_COUNTS, n))):
        check_save(ctx, tmp_path, k, keys, counts, name)


def test_every_table_form_gives_the_same_bytes(torch_mod, ctx, oracle, monkeypatch, tmp_path):
    k = 13
    (ab, ao), _ = sample_pair(2013, k)
    t = Table.of_reads(oracle, ab, ao, k)
    want = R.encode(k, t.keys, t.counts)
    for form in FORMS:
        c = table_in_form(torch_mod, ctx, form, k, ab, ao, t, monkeypatch)
        n, data = saved_bytes(c, tmp_path / "t.ktab")
        assert n == len(t.keys) and data == want, form
        sn, (ek, ec) = snapshot(c)  # the save left the table as it was
        assert sn == len(t.keys) and np.array_equal(ek, t.keys) and np.array_equal(ec, t.counts), form
        c.close()


def test_count_filter_and_snapshot(ctx, tmp_path):
    k = 21
    rng = np.random.default_rng(21)
    keys = canonical_keys(rng, k, 3000)
    counts = rng.choice(np.array([1, 2, 3, 5, 254, 255, 300, U32], np.uint32), len(keys))
    m = Model(k, keys, counts)
    c = pairs_table(ctx, k, keys, counts)
    for lo, hi in ((1, None), (2, None), (1, 1), (3, 255), (255, None), (256, 299), (U32, U32)):
        wk, wc = m.stage(lo, hi)
        n, data = saved_bytes(c, tmp_path / "t.ktab", min_count=lo, max_count=hi)
        assert n == len(wk) and data == R.encode(k, wk, wc), (lo, hi)
        sn, (ek, ec) = snapshot(c)
        assert sn == m.size and np.array_equal(ek, m.keys) and np.array_equal(ec, m.counts), (lo, hi)
    c.close()


# ---- load -----------------------------------------------------------------------------------------------------------------

def check_against_model(c, m, rng):
    from kmertools_amd import device  # noqa: F401
    assert c.size() == m.size
    absent = canonical_keys(rng, m.k, 300) if 2 * m.k > 24 else all_canonical(m.k)[:300]
    q = np.concatenate([m.keys[:500], absent])
    assert np.array_equal(c.lookup_host(q), m.count(q))
    ek, ec = c.export_host()
    assert np.array_equal(ek, m.keys) and np.array_equal(ec, m.counts)
    hist, tot = c.spectrum(300, totals=True)
    wh, wt = m.spectrum(300)
    assert np.array_equal(hist[1:], wh[1:]) and tuple(int(x) for x in tot) == wt
    gk, gi, gc, _ = c.graph(census=True)
    wk, wi, wc, _ = m.graph()
    assert np.array_equal(gk, wk) and np.array_equal(gi, wi) and np.array_equal(gc, wc)


@pytest.mark.parametrize("k", [4, 15, 16, 31])
def test_load_equals_the_model(ctx, tmp_path, k):
    from kmertools_amd import device
    rng = np.random.default_rng(300 + k)
    keys = some_keys(rng, k, 5000)
    counts = rng.choice(EDGE_COUNTS, len(keys))
    m = Model(k, keys, counts)
    path = tmp_path / "t.ktab"
    src = pairs_table(ctx, k, keys, counts)
    assert src.save(path) == m.size
    src.close()
    assert device.table_file_info(path) == {"k": k, "sections": 1, "entries": m.size, "occurrences": m.occurrences}
    c = device.Counter.from_file(ctx, path)
    assert c.k == k
    check_against_model(c, m, rng)
    c.close()
    # into a table that holds entries: the counts add
    small = counts.copy()
    small[small > 65536] = 9
    m2 = Model(k, keys[::3], np.ones(len(keys[::3]), np.uint32))
    c = pairs_table(ctx, k, m2.keys, m2.counts, slots=4 * len(keys) + 1024)
    src = pairs_table(ctx, k, keys, small)
    src.save(path)
    src.close()
    assert c.add_file(path) == len(keys)
    m2.add_pairs(keys, small)
    check_against_model(c, m2, rng)
    c.close()


def test_appended_sections_add(ctx, tmp_path):
    from kmertools_amd import device
    k = 19
    rng = np.random.default_rng(19)
    keys = canonical_keys(rng, k, 3000)
    a = pairs_table(ctx, k, keys[:2000], np.full(2000, 3, np.uint32))
    cb = np.full(2000, 5, np.uint32)
    cb[0] = U32 - 3  # keys[1000] reaches exactly 0xFFFFFFFF
    b = pairs_table(ctx, k, keys[1000:], cb)
    path = tmp_path / "two.ktab"
    assert a.save(path, append=True) == 2000  # (append to a file that does not exist creates it)
    assert b.save(path, append=True) == 2000
    assert device.table_file_info(path) == {"k": k, "sections": 2, "entries": 4000, "occurrences": 6000 + 1999 * 5 + U32 - 3}
    data = open(path, "rb").read()
    assert data == R.file_header(k) + R.encode_section(k, keys[:2000], np.full(2000, 3)) + R.encode_section(k, keys[1000:], cb)
    m = Model(k, keys[:2000], np.full(2000, 3, np.uint32))
    m.add_pairs(keys[1000:], cb)
    assert m.count(keys[1000:1001])[0] == U32
    c = device.Counter.from_file(ctx, path, slots=1 << 14)
    check_against_model(c, m, rng)
    a.close(), b.close(), c.close()


def test_load_forced_S(ctx, tmp_path):
    from kmertools_amd import device
    rng = np.random.default_rng(8)
    for k, n in ((8, 256), (12, 40), (16, 33), (31, 700)):  # (12, S = 1: P = 16 and 40 entries; 16, S = 1: P = 24 and 33)
        if k == 8:  # exactly one key in every bucket of S = 1 (P = 8)
            pool = all_canonical(k)
            keys = np.array([pool[(pool >> np.uint64(8)) == np.uint64(p)][0] for p in range(256)], np.uint64)
        else:
            keys = some_keys(rng, k, n)
        counts = rng.choice(EDGE_COUNTS, len(keys))
        m = Model(k, keys, counts)
        seen_p = set()
        for s in R.legal_s(k):
            path = tmp_path / "f.ktab"
            R.write_file(path, k, [(keys, counts)], s)
            c = device.Counter.from_file(ctx, path)
            ek, ec = c.export_host()
            assert np.array_equal(ek, m.keys) and np.array_equal(ec, m.counts), (k, s)
            c.close()
            seen_p.add(R.prefix_bits(k, s))
        assert {8: 8, 12: 16, 16: 24, 31: 22}[k] in seen_p


# ---- content corruption -------------------------------------------------------------------------------------------------------

def corrupt_cases():
    """name -> (file bytes, the words of the error): k = 31 with S = 8 (one bucket: any key order can be written down)"""
    k = 31
    rng = np.random.default_rng(31)
    keys = canonical_keys(rng, k, 600)
    counts = np.full(600, 7, np.uint32)
    counts[::50] = 300
    counts[255], counts[256] = 255, 1000  # escapes on both sides of the workgroup border

    def build(keys=keys, counts=counts, edit=None):
        parts = R.section_parts(k, keys, counts, 8, sort=False)
        parts = [bytearray(p) for p in parts]
        if edit:
            edit(parts)
        return R.file_header(k) + b"".join(bytes(p) for p in parts)

    def swapped():
        x = keys.copy()
        x[255], x[256] = keys[256], keys[255]
        return x

    def dup():
        x = keys.copy()
        x[256] = x[255]
        return x

    def noncanon():
        x = keys.copy()
        x[-1] = gr.rc_np(keys[-1:], k)[0]
        assert x[-1] > x[-2] and x[-1] > keys[-1]
        return x

    def too_big():
        x = keys.copy()
        x[-1] = (1 << 62) + 5
        return x

    n_ovf = int((counts >= 255).sum())

    def set_cbyte(i, v):
        def edit(parts):
            parts[3][i] = v
        return edit

    def ovf_value(parts):
        parts[4][0:4] = struct.pack("<I", 254)

    def occurrences(parts):
        occ, = struct.unpack_from("<Q", parts[0], 24)
        struct.pack_into("<Q", parts[0], 24, occ + 1)

    assert counts[3] == 7 and counts[50] == 300 and n_ovf == 14
    return k, keys, counts, {
        "non-ascending keys at a tile border": (build(keys=swapped()), "not strictly ascending"),
        "a duplicate key": (build(keys=dup()), "not strictly ascending"),
        "a non-canonical key": (build(keys=noncanon()), "non-canonical"),
        "a key >= 4^k": (build(keys=too_big()), "key >= 4^k"),
        "a zero count byte": (build(edit=set_cbyte(3, 0)), "zero count byte"),
        "one escape more than n_overflow": (build(edit=set_cbyte(3, 255)), "more escapes than n_overflow"),
        "one escape fewer": (build(edit=set_cbyte(50, 9)), "fewer escapes than n_overflow"),
        "an overflow value < 255": (build(edit=ovf_value), "overflow value < 255"),
        "wrong occurrences": (build(edit=occurrences), "occurrences"),
        "good": (build(), None),
    }


def test_content_corruption_is_refused_and_adds_nothing(ctx, tmp_path):
    from kmertools_amd import _lib, device
    k, keys, counts, cases = corrupt_cases()
    rng = np.random.default_rng(1)
    held = canonical_keys(rng, k, 900)
    m = Model(k, held, np.full(len(held), 2, np.uint32))
    c = pairs_table(ctx, k, m.keys, m.counts, slots=1 << 13)
    other = pairs_table(ctx, k, keys[:10], counts[:10])
    path = tmp_path / "c.ktab"
    for name, (data, words) in cases.items():
        if words is None:
            continue
        path.write_bytes(data)
        device.table_file_check(path)  # structurally whole: only the kernels can tell
        with pytest.raises(_lib.KmertoolsError) as e:
            c.add_file(path)
        assert e.value.code == _lib.KT_ERR_IO and words in str(e.value) and "section 0" in str(e.value), (name, str(e.value))
        sn, (ek, ec) = snapshot(c)
        assert sn == m.size and np.array_equal(ek, m.keys) and np.array_equal(ec, m.counts), name
        assert np.array_equal(other.lookup_host(keys[:20]), np.concatenate([counts[:10], np.zeros(10, np.uint32)])), name
    # a bad second section: the first one stays added, nothing of the second
    bad_second = cases["good"][0] + cases["a zero count byte"][0][R.FILE_HDR:]
    path.write_bytes(bad_second)
    with pytest.raises(_lib.KmertoolsError) as e:
        c.add_file(path)
    assert "section 1" in str(e.value) and "zero count byte" in str(e.value)
    m.add_pairs(keys, counts)
    sn, (ek, ec) = snapshot(c)
    assert sn == m.size and np.array_equal(ek, m.keys) and np.array_equal(ec, m.counts)
    c.close(), other.close()


# ---- errors ---------------------------------------------------------------------------------------------------------------

def test_errors(ctx, tmp_path):
    from kmertools_amd import _lib, device
    L = _lib.lib()
    k = 11
    rng = np.random.default_rng(11)
    keys = some_keys(rng, k, 500)
    c = pairs_table(ctx, k, keys, np.ones(len(keys), np.uint32))
    path = tmp_path / "e.ktab"
    assert L.kt_ctr_save(None, os.fsencode(path), 1, U32, 0, None) == _lib.KT_ERR_ARG
    assert L.kt_ctr_save(c._h, None, 1, U32, 0, None) == _lib.KT_ERR_ARG
    assert L.kt_ctr_add_file(None, os.fsencode(path), None) == _lib.KT_ERR_ARG
    assert L.kt_ctr_add_file(c._h, None, None) == _lib.KT_ERR_ARG
    assert L.kt_ctr_save(c._h, os.fsencode(path), 5, 4, 0, None) == _lib.KT_ERR_ARG
    assert not path.exists()
    c.save(path)
    good = path.read_bytes()

    def refused(fn, code, *words):
        with pytest.raises(_lib.KmertoolsError) as e:
            fn()
        assert e.value.code == code and all(w in str(e.value) for w in words), str(e.value)

    other = pairs_table(ctx, 12, some_keys(rng, 12, 50), np.ones(50, np.uint32))
    refused(lambda: other.add_file(path), _lib.KT_ERR_ARG, "k = 11", "k = 12")       # k mismatch
    refused(lambda: other.save(path, append=True), _lib.KT_ERR_ARG, "k = 11", "k = 12")  # append to a file of another k
    assert path.read_bytes() == good
    assert other.size() == 50
    refused(lambda: c.save(tmp_path / "no" / "such" / "dir.ktab"), _lib.KT_ERR_IO, "cannot open for writing")
    refused(lambda: c.add_file(tmp_path / "absent.ktab"), _lib.KT_ERR_IO, "cannot open")
    path.write_bytes(good[:-1])
    refused(lambda: c.add_file(path), _lib.KT_ERR_IO, "truncated")
    refused(lambda: c.save(path, append=True), _lib.KT_ERR_IO, "truncated")  # not a whole table file: left alone
    assert path.read_bytes() == good[:-1]
    assert sorted(os.listdir(tmp_path)) == ["e.ktab"]  # no temporary file stays behind
    # an overflowed table
    full = device.Counter(ctx, 31, 1024)
    many = canonical_keys(rng, 31, 3000)
    full.add_pairs_host(many, np.ones(len(many), np.uint32))
    path2 = tmp_path / "full.ktab"
    refused(lambda: full.save(path2), _lib.KT_ERR_FULL, "full")
    assert not path2.exists()
    full.close()
    # a table too small for the file: the load reports KT_ERR_FULL like any other add
    path.write_bytes(R.encode(31, many, np.ones(len(many), np.uint32)))
    small = device.Counter(ctx, 31, 1024)
    small.add_file(path)
    refused(small.size, _lib.KT_ERR_FULL, "full")
    small.close()
    c.close(), other.close()


# ---- the command line -----------------------------------------------------------------------------------------------------

CLI = os.path.join(ROOT, "kmertools_amd", "bin", "kmertools")
GOLDEN_READS = os.path.join(ROOT, "tests", "golden", "reads.fq")


def cli(*args, env=None):
    import subprocess
    return subprocess.run([CLI, *map(str, args)], capture_output=True, text=True, timeout=300, env=dict(os.environ, **(env or {})))


def files_of(d):
    return {f: open(os.path.join(d, f), "rb").read() for f in sorted(os.listdir(d))}


def synthetic_reads(path):
    rng = np.random.default_rng(77)
    genome = "".join("ACGT"[i] for i in rng.integers(0, 4, 3000))
    hap = list(genome)
    for p in range(100, 2900, 211):
        hap[p] = "ACGT"[("ACGT".index(hap[p]) + 1) % 4]
    hap = "".join(hap)
    with open(path, "w") as f:
        for i in range(600):
            a = int(rng.integers(0, 2900))
            f.write(">r%d\n%s\n" % (i, (genome if i % 2 else hap)[a:a + 100]))


@pytest.mark.parametrize("which", ["golden", "synthetic"])
def test_cli_table_commands_equal_counting_from_the_reads(oracle, tmp_path, which):
    from kmertools_amd import device
    k = 21
    reads = GOLDEN_READS
    if which == "synthetic":
        reads = tmp_path / "reads.fa"
        synthetic_reads(reads)
    tab = tmp_path / "reads.ktab"
    r = cli("ctr", "-i", reads, "-o", tmp_path / "ctr", "-k", k, "--save-table", tab)
    assert r.returncode == 0, r.stderr
    # the file is the restatement's of the table kmers.counts lists
    kc = sorted((int(ln.split()[0]), int(ln.split()[1])) for ln in open(tmp_path / "ctr" / "kmers.counts"))
    keys = np.array([a for a, _ in kc], np.uint64)
    counts = np.array([c for _, c in kc], np.uint32)
    assert len(keys) and open(tab, "rb").read() == R.encode(k, keys, counts)
    assert device.table_file_info(tab)["entries"] == len(keys)
    for name, args in (("graph", ()), ("unitigs", ("--gfa", "--links")), ("hetmers", ()), ("unitigs", ("--clip-tips", "--pop-bubbles")),
                       ("graph", ("--min-count", 2, "--acgt"))):
        a, b = tmp_path / ("a_" + name), tmp_path / ("b_" + name)
        ra = cli(name, "-i", reads, "-o", a, "-k", k, *args)
        rb = cli(name, "--table", tab, "-o", b, "-k", k, *args, env={"KT_CLI_TIMING": "1"})
        assert ra.returncode == 0 and rb.returncode == 0, (name, ra.stderr, rb.stderr)
        fa, fb = files_of(a), files_of(b)
        assert fa.keys() == fb.keys() and len(fa) >= 1 and any(len(v) for v in fa.values()), (name, list(fa))
        assert fa == fb, (name, args)
        assert "table file: table of" in rb.stderr and "entries loaded" in rb.stderr
        for d in (a, b):
            for f in os.listdir(d):
                os.unlink(os.path.join(d, f))
    # the count filter and --histo-only: the saved section is the filtered table, kmers.counts is not written
    r = cli("ctr", "-i", reads, "-o", tmp_path / "h", "-k", k, "--save-table", tab, "--min-count", 2, "--max-count", 40, "--histo-only")
    assert r.returncode == 0, r.stderr
    assert sorted(os.listdir(tmp_path / "h")) == ["kmers.histo"]
    sel = (counts >= 2) & (counts <= 40)
    assert open(tab, "rb").read() == R.encode(k, keys[sel], counts[sel])


def test_cli_out_of_core_saves_one_section_per_pass(ctx, tmp_path):
    from kmertools_amd import device
    k = 21
    reads = tmp_path / "reads.fa"
    synthetic_reads(reads)
    one, many = tmp_path / "one.ktab", tmp_path / "many.ktab"
    assert cli("ctr", "-i", reads, "-o", tmp_path / "o1", "-k", k, "--save-table", one).returncode == 0
    r = cli("ctr", "-i", reads, "-o", tmp_path / "o2", "-k", k, "--save-table", many, env={"KT_CTR_MAX_SLOTS": "4096"})
    assert r.returncode == 0, r.stderr
    info1, info2 = device.table_file_info(one), device.table_file_info(many)
    assert info1["sections"] == 1 and info2["sections"] > 1
    assert (info2["entries"], info2["occurrences"]) == (info1["entries"], info1["occurrences"])
    device.table_file_check(many)
    a, b = device.Counter.from_file(ctx, one), device.Counter.from_file(ctx, many)
    (ak, ac), (bk, bc) = a.export_host(), b.export_host()
    assert len(ak) == info1["entries"] and np.array_equal(ak, bk) and np.array_equal(ac, bc)
    a.close(), b.close()
    # the sections partition the keys: loading them is the same as decoding and merging them
    _, sections = R.decode(open(many, "rb").read())
    assert np.array_equal(np.sort(np.concatenate([s[0] for s in sections])), ak)


def test_cli_table_that_does_not_fit(tmp_path):
    k = 21
    reads = tmp_path / "reads.fa"
    synthetic_reads(reads)
    tab = tmp_path / "t.ktab"
    assert cli("ctr", "-i", reads, "-o", tmp_path / "o", "-k", k, "--save-table", tab, "--histo-only").returncode == 0
    for name in ("graph", "unitigs", "hetmers"):
        out = tmp_path / ("fit_" + name)
        r = cli(name, "--table", tab, "-o", out, "-k", k, env={"KT_CTR_MAX_SLOTS": "2048"})
        assert r.returncode == 101 and "does not fit" in r.stderr and "entries" in r.stderr and "room for 2048" in r.stderr, r.stderr
        assert not out.exists() or os.listdir(out) == []


def first_half(src, dst):
    """the first half of the records of a FASTA (2 lines each) or FASTQ (4 lines each) file"""
    lines = open(src).read().splitlines(keepends=True)
    per = 4 if lines[0].startswith("@") else 2
    n = max(1, len(lines) // per // 2)
    open(dst, "w").writelines(lines[:n * per])


def same_files(a, b, unordered=()):
    """byte-identical files in both places; those named in `unordered` as sorted line sets (a table's dump order follows the
    order in which the table was filled)"""
    fa, fb = files_of(a), files_of(b)
    assert fa.keys() == fb.keys() and len(fa) >= 1 and any(len(v) for v in fa.values()), (list(fa), list(fb))
    for name in fa:
        if name in unordered:
            assert sorted(fa[name].splitlines()) == sorted(fb[name].splitlines()), name
        else:
            assert fa[name] == fb[name], name


@pytest.mark.parametrize("which", ["golden", "synthetic"])
def test_cli_lookup_and_two_table_commands_equal_counting_from_the_reads(tmp_path, which):
    k = 21
    reads = GOLDEN_READS
    ext = ".fq"
    if which == "synthetic":
        reads, ext = tmp_path / "reads.fa", ".fa"
        synthetic_reads(reads)
    reads_b = tmp_path / ("half" + ext)
    first_half(reads, reads_b)
    tab, tab_b = tmp_path / "a.ktab", tmp_path / "b.ktab"
    assert cli("ctr", "-i", reads, "-o", tmp_path / "c_a", "-k", k, "--save-table", tab, "--histo").returncode == 0
    assert cli("ctr", "-i", reads_b, "-o", tmp_path / "c_b", "-k", k, "--save-table", tab_b, "--histo-only").returncode == 0
    # ctr --table: the file dumped and its spectrum, as sorted line sets; re-saved filtered
    r = cli("ctr", "--table", tab, "-o", tmp_path / "c_t", "-k", k, "--histo", env={"KT_CLI_TIMING": "1"})
    assert r.returncode == 0 and "entries loaded" in r.stderr, r.stderr
    same_files(tmp_path / "c_a", tmp_path / "c_t", unordered=("kmers.counts", "kmers.histo"))
    lo2 = tmp_path / "lo2.ktab"
    assert cli("ctr", "--table", tab, "-o", tmp_path / "c_f", "-k", k, "--min-count", 2, "--histo-only", "--save-table", lo2).returncode == 0
    assert cli("ctr", "-i", reads, "-o", tmp_path / "c_g", "-k", k, "--min-count", 2, "--histo-only", "--save-table", tmp_path / "lo2r.ktab").returncode == 0
    assert open(lo2, "rb").read() == open(tmp_path / "lo2r.ktab", "rb").read()
    # the read-level commands: the table counted from -a (here: the first half) against --table
    for name, args, out in (("filter", ("--min-count", 1), "kept" + ext), ("correct", ("--min-count", 1), "fixed" + ext),
                            ("profile", ("--positions",), None), ("cov", (), None)):
        a, b = tmp_path / ("a_" + name), tmp_path / ("b_" + name)
        if out:
            os.mkdir(a), os.mkdir(b)
        ra = cli(name, "-i", reads, "-a", reads_b, "-o", os.path.join(a, out) if out else a, "-k", k, *args)
        rb = cli(name, "-i", reads, "--table", tab_b, "-o", os.path.join(b, out) if out else b, "-k", k, *args)
        assert ra.returncode == 0 and rb.returncode == 0, (name, ra.stderr, rb.stderr)
        same_files(a, b, unordered=("kmers.counts",))
    # compare and setop: A, B or both from table files
    for name, args in (("compare", ()), ("setop", ("--op", "subtract")), ("setop", ("--op", "union", "--count", "sum", "--min-b", 2))):
        a = tmp_path / "a_two"
        assert cli(name, "-i", reads, "-a", reads_b, "-o", a, "-k", k, *args).returncode == 0
        for j, sides in enumerate((("--table", tab, "-a", reads_b), ("-i", reads, "--alt-table", tab_b), ("--table", tab, "--alt-table", tab_b))):
            b = tmp_path / ("b_two%d" % j)
            r = cli(name, *sides, "-o", b, "-k", k, *args)
            assert r.returncode == 0, (name, sides, r.stderr)
            same_files(a, b)
            for f in os.listdir(b):
                os.unlink(os.path.join(b, f))
        for f in os.listdir(a):
            os.unlink(os.path.join(a, f))


def test_cli_failed_out_of_core_save_leaves_no_file(tmp_path):
    k = 21
    reads = tmp_path / "reads.fa"
    synthetic_reads(reads)
    tab = tmp_path / "sub" / "t.ktab"  # the directory does not exist: every section's save fails
    r = cli("ctr", "-i", reads, "-o", tmp_path / "o", "-k", k, "--save-table", tab, env={"KT_CTR_MAX_SLOTS": "4096"})
    assert r.returncode == 101 and "cannot open for writing" in r.stderr, r.stderr
    ok = tmp_path / "t.ktab"
    assert cli("ctr", "-i", reads, "-o", tmp_path / "o2", "-k", k, "--save-table", ok, env={"KT_CTR_MAX_SLOTS": "4096"}).returncode == 0
    assert sorted(f for f in os.listdir(tmp_path) if "ktab" in f) == ["t.ktab"]  # no .partial stays behind
