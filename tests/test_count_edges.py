"""Counts at the edges of u32 through every call that writes or reads a k-mer table.

A count is a u32 stored as occurrences - 1 and turned back with + 1 by every reader.  tests/count_edges.py builds, per k in
(31, 15, 9), a small de Bruijn graph whose counts are the values on either side of 2^8, 2^16, 2^24, 2^31 and 2^32; here

  without a GPU  the builder's conditions, and every restatement the GPU tests compare with (graph_ref, unitig_ref,
                 unitig_link_ref, tip_ref, want_spectrum / compare / setop / profile, the oracle's counter and the model's
                 add_pairs, cov and lookup) against a brute force over a dict of Python integers on 200 keys;
  readers        one table per k and per way of getting there (FORMS), every reader exact against the restatements;
  writers        every path that adds brings a key from e - m to exactly e, 0xFFFFFFFF included, and pairs with count 0 add
                 nothing.

What the forms can and cannot hold.  Large counts are placed with kt_ctr_add_pairs, and add_pairs (like every probing add)
first turns a densely packed table, or one that lives in its export target, into the probing image: a dense, target or
direct-built table only ever holds what ONE bulk batch counted.  So the forms "bulk", "target" and "direct" below are bulk
builds (checked by their [bulk] line) raised by add_pairs - the image made from the packed ranges, from the target's pairs,
from the direct counters, then the adds - and the form every reader then meets is the probing image, direct-addressed for
"direct".  The packed forms themselves are read at the counts reads can reach in a test (a k-mer 255 .. 65 537 times in one
batch, which is also what a 16-bit field in a hand-over format would break): test_bulk_built_forms_at_the_counts_reads_reach.
Every comparison is exact integer equality; the one tolerance is the README's 1e-6 for f32 coverage rows."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import count_edges as ce  # noqa: E402
import graph_ref as gr  # noqa: E402
import table_model as tm  # noqa: E402
import tip_ref as tr  # noqa: E402
import unitig_link_ref as lr  # noqa: E402
import unitig_ref as ur  # noqa: E402
from test_correct import owner_of as owner_np, want_apply, want_covered, want_support  # noqa: E402
from test_ctr_compare import want_compare  # noqa: E402
from test_ctr_setop import want_setop  # noqa: E402
from test_ctr_spectrum import want_spectrum  # noqa: E402
from test_profile import want_profile, want_stats  # noqa: E402

U32 = ce.U32
NO = 0xFFFFFFFF  # KT_NO_KMER
EDGES = ce.EDGES
KS = ce.KS
SLOTS = 1 << 17
OPS = ("intersect", "subtract", "union", "xor")
RULES = ("first", "min", "max", "sum")


def windows():
    """every (lo, hi) of {(e, e), (e, 0xFFFFFFFF), (1, e), (e - 1, e + 1)} over EDGES, clipped to 1 <= lo <= hi <= 0xFFFFFFFF"""
    out = []
    for e in EDGES:
        for lo, hi in ((e, e), (e, U32), (1, e), (e - 1, e + 1)):
            w = (max(lo, 1), min(hi, U32))
            if w not in out:
                out.append(w)
    return out


WINDOWS = windows()
assert len(WINDOWS) >= 50 and (U32, U32) in WINDOWS and (1, U32) in WINDOWS and (U32 - 1, U32) in WINDOWS


def model(k, b=False):
    fx = ce.fixture(k)
    return tm.Model(k, fx.keys, fx.counts_b if b else fx.counts)


# ---- without a GPU ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", KS)
def test_fixture_conditions(oracle, k):
    """fixture() asserts them while it builds; here: that it builds without a GPU, and the numbers a reader can check by eye"""
    fx = ce.fixture(k)
    assert 3000 <= len(fx.keys) <= 6000
    assert min(np.bincount(np.searchsorted(np.array(EDGES, np.uint64), fx.counts.astype(np.uint64)))) >= 8
    assert fx.big_sum > 2 ** 33 and fx.big_sum % U32 == 0 and fx.big_sum // U32 >= 3
    assert sorted(fx.straddle) == [2 ** 16, 2 ** 24, 2 ** 31]
    assert int(fx.counts.astype(np.uint64).sum()) > 2 ** 40  # (the occurrences no 32-bit sum holds)
    # the contigs counted as reads give the keys, with small counts: what a bulk build of them leaves before the pairs
    assert fx.built.max() < 255 and len(fx.built) == len(fx.keys)


def test_tip_cases_conditions():
    """the Y graphs: the sums are what the docstrings say, and float / double do get the third one wrong"""
    cases = ce.tip_cases()
    n_u, c_u, n_w, c_w = cases["equal means"]["sums"]
    assert c_u * n_w == c_w * n_u and c_u > 2 ** 33
    n_u, c_u, n_w, c_w = cases["sums one apart"]["sums"]
    assert n_u == n_w and c_w - c_u == 1 and c_u > 2 ** 33
    n_u, c_u, n_w, c_w = cases["float trap"]["sums"]
    assert n_w == n_u + 1 and c_w * n_u > c_u * n_w  # w's mean is the greater one, exactly
    assert float(c_w) / n_w <= float(c_u) / n_u, "a comparison of the means in double gets this one right"
    assert np.float32(c_w) / np.float32(n_w) <= np.float32(c_u) / np.float32(n_u)
    for name, case in cases.items():
        t = case["table"]
        assert all(isinstance(c, int) and 1 <= c <= U32 for c in t.values())
        us, ls, marks, tally = tr.marks(t, 15, case["max_tip_nodes"])
        assert len(us) == 3 and sorted(marks) == [tr.KEEP, tr.KEEP, tr.TIP], (name, marks)
        number = {b: next(i for i, u in enumerate(us) if {gr.canon_s(u[0][j:j + 15]) for j in range(u[3])} == set(case[b]))
                  for b in "uw"}
        # (equal means: the higher number goes)
        lost = number[case["loser"]] if case["loser"] else max(number.values())
        assert marks[lost] == tr.TIP, (name, marks, number)


def subset_of(fx, n=200):
    """200 keys of the fixture that hang together: the unitig at 2^32 - 1, the straddling pairs, then the k-mers of the
    backbone in walking order - as indices into fx.keys, ascending"""
    k = fx.k
    idx = list(fx.big_nodes)
    pos = {int(key): i for i, key in enumerate(fx.keys.tolist())}
    for b in ce.STRADDLES:
        idx += [pos[key] for key in fx.straddle[b]]
    back = fx.contigs[0].decode()
    for j in range(len(back) - k + 1):
        i = pos[gr.key_of(gr.canon_s(back[j:j + k]))]
        if i not in idx:
            idx.append(i)
        if len(idx) == n:
            break
    assert len(idx) == n == len(set(idx))
    return np.sort(np.array(idx))


def brute_spectrum(d, n_bins):
    h = [0] * n_bins
    for c in d.values():
        h[min(c, n_bins - 1)] += 1
    h[0] = 0
    return h


def brute_compare(da, db, n_rows, n_cols):
    m = [[0] * n_cols for _ in range(n_rows)]
    tot = dict(distinct_a=len(da), distinct_b=len(db), shared=0, occurrences_a=sum(da.values()), occurrences_b=sum(db.values()),
               shared_min=0)
    for key in set(da) | set(db):
        a, b = da.get(key, 0), db.get(key, 0)
        m[min(a, n_rows - 1)][min(b, n_cols - 1)] += 1
        if a and b:
            tot["shared"] += 1
            tot["shared_min"] += min(a, b)
    return m, tot


def brute_setop(da, db, op, rule, ra, rb):
    out = {}
    for key in set(da) | set(db):
        a, b = da.get(key, 0), db.get(key, 0)
        a = a if ra[0] <= a <= ra[1] else 0
        b = b if rb[0] <= b <= rb[1] else 0
        keep = {"intersect": a and b, "subtract": a and not b, "union": a or b, "xor": bool(a) != bool(b)}[op]
        if keep:
            out[key] = {"first": a or b, "min": min(a, b) if a and b else a + b, "max": max(a, b), "sum": min(a + b, U32)}[rule]
    return out


@pytest.mark.parametrize("k", KS)
def test_table_references_against_big_integers(oracle, k):
    """the model, the oracle's counter, want_spectrum / compare / setop / profile and the coverage rows on 200 keys at edge
    counts, against dicts of Python integers"""
    fx = ce.fixture(k)
    sub = subset_of(fx)
    keys, ca, cb = fx.keys[sub], fx.counts[sub], fx.counts_b[sub]
    cb[:20] = ca[:20]  # (some keys with the same count on both sides)
    da = dict(zip(keys.tolist(), (int(c) for c in ca)))
    db = dict(zip(keys[30:].tolist(), (int(c) for c in cb[30:])))  # (B lacks thirty of A's keys ...)
    extra = np.setdiff1d(tm.canonical_keys(np.random.default_rng(k), k, 40), fx.keys)[:25]
    db.update(zip(extra.tolist(), [int(EDGES[i % len(EDGES)]) for i in range(len(extra))]))  # (... and has 25 of its own)
    assert sum(da.values()) > 2 ** 36 and all(isinstance(c, int) for c in da.values())
    bk = np.array(sorted(db), np.uint64)
    A, B = tm.Model(k, keys, ca), tm.Model(k, bk, np.array([db[x] for x in bk.tolist()], np.uint32))
    # add_pairs reaches the edge counts in pieces: e - 5, then 2 and 3 in one call, with zeros strewn in
    m = tm.Model(k)
    m.add_pairs(keys, (ca.astype(np.int64) - 5).clip(0).astype(np.uint32))
    rest = np.minimum(ca, 5)
    m.add_pairs(np.concatenate([keys, keys, keys]), np.concatenate([rest - rest // 2, np.zeros(len(keys), np.uint32), rest // 2]))
    assert np.array_equal(m.keys, A.keys) and np.array_equal(m.counts, A.counts) and m.counts.dtype == np.uint32
    m.add_pairs(extra[:3], np.zeros(3, np.uint32))
    assert m.size == len(da) and not m.count(extra[:3]).any()
    c = oracle.Counter()
    c.add_pairs(keys, ca - np.minimum(ca, 5))
    c.add_pairs(keys, np.minimum(ca, 5))
    ok, oc = c.export(True)
    assert ok.tolist() == sorted(da) and oc.tolist() == [da[x] for x in sorted(da)]
    # lookup
    q = np.concatenate([keys[::3], extra])
    assert A.count(q).tolist() == [da.get(x, 0) for x in q.tolist()]
    assert A.occurrences == sum(da.values())
    for lo, hi in WINDOWS:
        sk, sc = A.stage(lo, hi)
        assert sk.tolist() == [x for x in sorted(da) if lo <= da[x] <= hi], (lo, hi)
        assert sc.tolist() == [da[x] for x in sk.tolist()]
    # spectrum
    for n_bins in (2, 3, 257, 65537):
        assert want_spectrum(ca, n_bins).tolist() == brute_spectrum(da, n_bins), n_bins
    h = want_spectrum(ca, 2 ** 24)
    assert int(h[2 ** 24 - 1]) == sum(1 for c in da.values() if c >= 2 ** 24 - 1) and int(h.sum()) == len(da)
    assert int(h[2 ** 24 - 2]) == 0 and int(h[65536]) == sum(1 for c in da.values() if c == 65536)
    # compare
    for n_rows, n_cols in ((2, 2), (257, 3), (3, 257)):
        for X, Y, dx, dy in ((A, B, da, db), (A, A, da, da), (B, A, db, da)):
            wm, wt = want_compare(X, Y, n_rows, n_cols)
            bm, bt = brute_compare(dx, dy, n_rows, n_cols)
            bm[0][0] = 0
            assert wm.tolist() == bm and wt == bt, (n_rows, n_cols)
    wm, wt = want_compare(A, B, 4096, 4096)
    bm, bt = brute_compare(da, db, 4096, 4096)
    assert wt == bt and int(wm[4095, 4095]) == bm[4095][4095] and int(wm.sum()) == len(set(da) | set(db))
    # setop
    for op in OPS:
        for rule in RULES:
            for ra, rb in (((1, U32), (1, U32)), ((2 ** 31, U32), (1, 2 ** 31)), ((U32, U32), (1, U32 - 1)), ((1, 65536), (65536, U32))):
                wk, wc = want_setop(A, B, op, rule, ra, rb)
                want = brute_setop(da, db, op, rule, ra, rb)
                assert wk.tolist() == sorted(want) and wc.tolist() == [want[x] for x in sorted(want)], (op, rule, ra, rb)
    # profile and coverage over the walking reads
    prof = want_profile(oracle, fx.reads, k, A)
    at = 0
    for s in fx.reads:
        rk, pos = ce.read_kmers(fx, s)
        row = [NO] * len(s)
        for key, p in zip(rk.tolist(), pos.tolist()):
            row[p] = min(da.get(key, 0), U32 - 1)
        assert prof[at:at + len(s)].tolist() == row
        at += len(s)
    assert at == len(prof) and (prof == U32 - 1).any() and (prof == 0).any()
    for bin_size in (1, 3, 65536, 2 ** 31, 2 ** 32 - 1, 2 ** 32, 2 ** 40):
        for bin_count in (1, 2, 16, 300):
            rows = c.cov_batch(fx.reads_csr[0], fx.reads_csr[1], k, bin_size, bin_count, norm=False)
            for i, s in enumerate(fx.reads):
                want = [0] * bin_count
                for key in ce.read_kmers(fx, s)[0].tolist():
                    want[min(da.get(key, 0) // bin_size, bin_count - 1)] += 1
                assert rows[i].tolist() == want, (bin_size, bin_count, i)


@pytest.mark.parametrize("k", KS)
def test_graph_references_against_big_integers(oracle, k):
    """graph_ref's numpy restatement against its string one, and the unitig, link and tip restatements against their
    definitions over Python integers, on 200 keys and the count windows that cut the graph at the edges"""
    fx = ce.fixture(k)
    sub = subset_of(fx)
    keys, counts = fx.keys[sub], fx.counts[sub]
    d = ce.strings_of(keys, counts, k)
    assert all(isinstance(c, int) for c in d.values())
    for lo, hi in ((1, U32), (2 ** 31, U32), (1, 2 ** 31 - 1), (U32, U32), (65536, 2 ** 24), (2 ** 24 + 1, U32 - 1)):
        nodes = gr.brute(d, k, lo, hi)
        F, info, c, cen = gr.restate(keys, counts, k, lo, hi)
        assert F.tolist() == [x[0] for x in nodes] and c.tolist() == [x[1] for x in nodes], (lo, hi)
        assert info.tolist() == [x[2] for x in nodes], (lo, hi)
        assert [int(x) for x in cen] == gr.census_of(nodes), (lo, hi)
        assert c.dtype == np.uint32 and cen.dtype == np.uint64
        # a k-mer out of range is no node: the unitigs, links and marks are those of the table without it
        cut = {s: 1 for s, x in d.items() if lo <= x <= hi}
        us, ls = lr.links(d, k, lo, hi)
        us1, ls1 = lr.links(cut, k)
        assert [(u[0], u[2], u[3]) for u in us] == [(u[0], u[2], u[3]) for u in us1] and ls == ls1, (lo, hi)
        for u in us:
            s = sum(d[gr.canon_s(u[0][j:j + k])] for j in range(u[3]))
            assert u[1] == s and isinstance(u[1], int), (lo, hi)
        for tip in (3, k, 2 ** 31 - 2):
            marks = tr.marks(d, k, tip, lo, hi)[2]
            off = np.zeros(len(us) + 1, np.uint64)
            off[1:] = np.cumsum([len(u[0]) for u in us])
            lo_, to = lr.as_arrays(ls)
            m2, tally = tr.marks_of_arrays(off, np.array([u[1] for u in us], np.uint64), np.array([u[2] for u in us], np.uint32),
                                           lo_, to, k, tip)
            assert m2.tolist() == marks and tally.tolist() == tr.tally_of(marks, [u[3] for u in us]), (lo, hi, tip)
    us = ur.unitigs(d, k)
    assert max(u[1] for u in us) >= fx.big_sum > 2 ** 33
    if k >= 15:  # the straddling pair is a pair of neighbours: one side of the window sees the edge, the other does not
        for b in ce.STRADDLES:
            lo_key, hi_key = fx.straddle[b]
            for (lo, hi), inside, outside in (((b, U32), hi_key, lo_key), ((1, b - 1), lo_key, hi_key)):
                F, info, c, cen = gr.restate(keys, counts, k, lo, hi)
                assert inside in F.tolist() and outside not in F.tolist()
                F1, info1, _, _ = gr.restate(keys, counts, k)
                i, i1 = F.tolist().index(inside), F1.tolist().index(inside)
                assert bin(int(info[i]) & 0xFF).count("1") < bin(int(info1[i1]) & 0xFF).count("1"), (b, lo, hi)


# ---- the rig ------------------------------------------------------------------------------------------------------------------

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


@pytest.fixture
def make_counter(ctx):
    """Counter(ctx, k, capacity), released when the test ends however it ends"""
    from kmertools_amd import device
    made = []

    def make(k, capacity=SLOTS):
        made.append(device.Counter(ctx, k, capacity))
        return made[-1]

    yield make
    for c in reversed(made):
        c.close()


BULK_ENV = {"KT_BULK": "1", "KT_BULK_MIN_BASES": "0", "KT_BULK_MERGE_DIV": "1000000000", "KT_BULK_VERBOSE": "1"}


class Env:
    """the environment of a bulk build (read by every job when it begins) for the length of a with block"""

    def __init__(self, **kw):
        self.kw = kw

    def __enter__(self):
        self.old = {n: os.environ.get(n) for n in self.kw}
        os.environ.update(self.kw)

    def __exit__(self, *exc):
        for n, v in self.old.items():
            if v is None:
                os.environ.pop(n, None)
            else:
                os.environ[n] = v


def bulk_lines(capfd):
    return [line for line in capfd.readouterr().err.splitlines() if line.startswith("[bulk]")]


def the_bulk_line(capfd, tag, merge, build):
    """the one [bulk] line of the job just run: (k, keys, level1, level2, build | merge, spilled, l1, l2, build=...)"""
    lines = bulk_lines(capfd)
    assert len(lines) == 1, (tag, lines)
    words = lines[0].split()
    assert words[5] == ("merge" if merge else "build") and words[-1] == "build=" + build, (tag, lines)
    return words


def dev(torch, a):
    a = np.ascontiguousarray(a)
    a = a.view({np.dtype(np.uint64): np.int64, np.dtype(np.uint32): np.int32}.get(a.dtype, a.dtype))
    return torch.from_numpy(a if a.size else np.zeros(1, a.dtype)).cuda()


def by_key(keys, *rest):
    order = np.argsort(keys, kind="stable")
    return (keys[order],) + tuple(r[order] for r in rest)


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b)


FORMS = ("probing", "bulk", "target", "direct")
BUILT_AS = {"bulk": "dense", "target": "dense-ext", "direct": "direct"}


def forms_of(k):
    return FORMS if k == 9 else FORMS[:3]


def raised_table(torch, ctx, capfd, form, k, keys, counts, made):
    """a table that holds (keys, counts) of the fixture, reached as `form` says; -> (Counter, what the form is by now)"""
    from kmertools_amd import device
    fx = ce.fixture(k)
    c = device.Counter(ctx, k, 4 ** k if form == "direct" else SLOTS)
    made.append(c)
    if form == "probing":
        c.add_pairs_host(keys, counts)
        return c, "the probing image, filled by add_pairs"
    assert c.capacity() == (4 ** k if form == "direct" else SLOTS)
    if form == "target":
        room = len(fx.keys) + 9
        xk, xc = torch.zeros(room, dtype=torch.int64, device="cuda"), torch.zeros(room, dtype=torch.int32, device="cuda")
        c.export_target(xk, xc, room)
    capfd.readouterr()
    with Env(**BULK_ENV):
        c.add_reads(dev(torch, fx.csr[0]), dev(torch, fx.csr[1]), len(fx.contigs))
    torch.cuda.synchronize()
    the_bulk_line(capfd, (k, form), False, BUILT_AS[form])
    assert c.size() == len(fx.keys), (k, form)
    assert same(keys, fx.keys) and (counts >= fx.built).all()
    c.add_pairs_host(keys, counts - fx.built)  # (a probing add: the packed entries become the probing image first)
    return c, "the probing image made from the %s build, raised by add_pairs" % BUILT_AS[form]


class Tables:
    """the reader tests' tables, built on first use and shared: no reader changes a table's content"""

    def __init__(self):
        self.made, self.cache = [], {}

    def get(self, torch, ctx, capfd, k, form, b=False):
        name = (k, form, b)
        if name not in self.cache:
            fx = ce.fixture(k)
            self.cache[name] = raised_table(torch, ctx, capfd, form, k, fx.keys, fx.counts_b if b else fx.counts, self.made)
        return self.cache[name]

    def close(self):
        for c in reversed(self.made):
            c.close()


@pytest.fixture(scope="module")
def tables(ctx):
    t = Tables()
    yield t
    t.close()


def each_form(torch, ctx, capfd, tables, k):
    for form in forms_of(k):
        c, reached = tables.get(torch, ctx, capfd, k, form)
        yield c, "k=%d form %s (%s)" % (k, form, reached)


@functools.lru_cache(maxsize=None)
def lookup_keys(k):
    fx = ce.fixture(k)
    absent = np.setdiff1d(tm.canonical_keys(np.random.default_rng(50 + k), k, 1500), fx.keys)
    q = np.concatenate([fx.keys, absent])
    return q[np.random.default_rng(51 + k).permutation(len(q))]


# ---- readers ------------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("k", KS)
def test_lookup_and_exports_return_the_pairs(torch_mod, ctx, capfd, tables, oracle, k):
    m = model(k)
    q = lookup_keys(k)
    for c, tag in each_form(torch_mod, ctx, capfd, tables, k):
        assert c.size() == m.size, tag
        assert same(c.lookup_host(q), m.count(q)), tag
        gk, gc = c.export_host()
        assert same(gk, m.keys) and same(gc, m.counts), tag
        n = c.export_stage_range(1, None)
        assert n == m.size, tag
        a = n // 3
        (k2, c2), (k1, c1) = c.export_fetch(a, n - a), c.export_fetch(0, a)
        gk, gc = by_key(np.concatenate([k1, k2]), np.concatenate([c1, c2]))
        assert same(gk, m.keys) and same(gc, m.counts), tag
        tk = torch_mod.zeros(n + 3, dtype=torch_mod.int64, device="cuda")
        tc = torch_mod.zeros(n + 3, dtype=torch_mod.int32, device="cuda")
        assert c.export(tk, tc, n) == n
        gk, gc = by_key(tk[:n].cpu().numpy().view(np.uint64), tc[:n].cpu().numpy().view(np.uint32))
        assert same(gk, m.keys) and same(gc, m.counts), tag


@pytest.mark.gpu
@pytest.mark.parametrize("k", KS)
def test_stage_range_at_every_edge(torch_mod, ctx, capfd, tables, oracle, k):
    """FILTER in the probing export, for every window; the packed forms' filters are in
    test_bulk_built_forms_at_the_counts_reads_reach"""
    m = model(k)
    for c, tag in each_form(torch_mod, ctx, capfd, tables, k):
        for lo, hi in WINDOWS:
            wk, wc = m.stage(lo, hi)
            n = c.export_stage_range(lo, hi)
            assert n == len(wk), (tag, lo, hi, n, len(wk))
            gk, gc = by_key(*c.export_fetch(0, n))
            assert same(gk, wk) and same(gc, wc), (tag, lo, hi)
        gk, gc = c.export_host()
        assert same(gk, m.keys) and same(gc, m.counts), tag


@pytest.mark.gpu
@pytest.mark.parametrize("k", KS)
def test_spectrum_top_bin_and_totals(torch_mod, ctx, capfd, tables, oracle, k):
    m = model(k)
    occ = sum(int(x) for x in m.counts)
    assert occ > 2 ** 40
    for c, tag in each_form(torch_mod, ctx, capfd, tables, k):
        for n_bins in (2, 3, 257, 65537) + ((2 ** 24,) if "form probing" in tag else ()):
            hist, (d, o) = c.spectrum(n_bins, totals=True)
            want = want_spectrum(m.counts, n_bins)
            assert same(hist, want), (tag, n_bins, int(hist[n_bins - 1]), int(want[n_bins - 1]))
            assert d == m.size and o == occ, (tag, n_bins, d, o, occ)


@pytest.mark.gpu
@pytest.mark.parametrize("k", KS)
def test_compare_totals_and_matrix(torch_mod, ctx, capfd, tables, oracle, k):
    A, B = model(k), model(k, b=True)
    b, _ = tables.get(torch_mod, ctx, capfd, k, "probing", b=True)
    names = ("distinct_a", "distinct_b", "shared", "occurrences_a", "occurrences_b", "shared_min")
    big = {}
    for c, tag in each_form(torch_mod, ctx, capfd, tables, k):
        for other, Other, who in ((b, B, "the permuted table"), (c, A, "itself")):
            for n_rows, n_cols in ((2, 2), (257, 3)) + (((4096, 4096),) if "form probing" in tag else ()):
                key = (who, n_rows, n_cols)
                if key not in big:
                    big[key] = want_compare(A, Other, n_rows, n_cols)
                wm, wt = big[key]
                gm, gt = c.compare(other, n_rows, n_cols, totals=True)
                assert gt == wt, (tag, who, n_rows, n_cols, gt, wt)
                assert same(gm, wm), (tag, who, n_rows, n_cols)
            gm, gt = other.compare(c, 3, 257, totals=True)  # (the raised table probed)
            wm, wt = want_compare(Other, A, 3, 257)
            assert gt == wt and same(gm, wm), (tag, who, "probed")
    assert big[("the permuted table", 2, 2)][1]["shared_min"] > 2 ** 39  # (no 32-bit sum holds it)
    assert set(big[("itself", 2, 2)][1]) == set(names)


@pytest.mark.gpu
@pytest.mark.parametrize("k", KS)
def test_setop_four_count_rules(torch_mod, ctx, capfd, tables, oracle, k):
    A, B = model(k), model(k, b=True)
    b, _ = tables.get(torch_mod, ctx, capfd, k, "probing", b=True)
    cases = [("union", ((1, None), (1, None))), ("intersect", ((2 ** 31, None), (1, 2 ** 31))), ("xor", ((U32, U32), (1, U32 - 1)))]
    for c, tag in each_form(torch_mod, ctx, capfd, tables, k):
        for op, (ra, rb) in cases:
            for rule in RULES:
                wk, wc = want_setop(A, B, op, rule, ra, rb)
                assert len(wk)
                gk, gc = c.setop(b, op, rule, ra, rb)
                assert same(gk, wk) and same(gc, wc), (tag, op, rule, ra, rb)
                wk, wc = want_setop(B, A, op, rule, ra, rb)
                gk, gc = b.setop(c, op, rule, ra, rb)
                assert same(gk, wk) and same(gc, wc), (tag, op, rule, ra, rb, "probed")
    assert (want_setop(A, B, "union", "sum")[1] == U32).sum() >= 8  # (sums that saturate)


def part_tables(make_counter, k, n_parts):
    """the fixture's table as n_parts tables, each with the keys of one hash partition"""
    from kmertools_amd import device
    fx = ce.fixture(k)
    own = owner_np(fx.keys, n_parts)
    assert [device.owner_of(key, n_parts) for key in fx.keys[:64].tolist()] == own[:64].tolist()
    out = []
    for p in range(n_parts):
        assert (own == p).any()
        c = make_counter(k, 1 << 15)
        c.add_pairs_host(fx.keys[own == p], fx.counts[own == p])
        out.append(c)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("k", KS)
def test_cov_rows_at_every_bin_size(torch_mod, ctx, capfd, tables, make_counter, oracle, k):
    fx = ce.fixture(k)
    bases, offsets = fx.reads_csr
    n = len(fx.reads)
    ref = oracle.Counter()
    ref.add_pairs(fx.keys, fx.counts)
    parts = part_tables(make_counter, k, 2)
    for c, tag in each_form(torch_mod, ctx, capfd, tables, k):
        full = "form probing" in tag
        for bin_size in (1, 3, 65536, 2 ** 31, 2 ** 32 - 1, 2 ** 32, 2 ** 40):
            for bin_count in (1, 2, 16, 70000) if full else (16,):
                t = (tag, bin_size, bin_count)
                raw = ref.cov_batch(bases, offsets, k, bin_size, bin_count, norm=False)
                want = raw.astype(np.uint32)
                assert (want == raw).all()
                got = c.cov_host(bases, offsets, bin_size, bin_count, norm=False, dtype="u32")
                assert same(got, want), t
                if full:
                    acc = np.zeros((n, bin_count), np.uint32)
                    for p, part in enumerate(parts):
                        part.cov_part(bases, offsets, n, bin_size, bin_count, acc, 2, p, mem=0)
                    assert same(acc, want), (t, "two partitions")
                wn = ref.cov_batch(bases, offsets, k, bin_size, bin_count, norm=True)
                g64 = c.cov_host(bases, offsets, bin_size, bin_count, norm=True, dtype="f64")
                assert same(g64.view(np.uint64), wn.view(np.uint64)), (t, "f64")
                g32 = c.cov_host(bases, offsets, bin_size, bin_count, norm=True, dtype="f32")
                assert g32.dtype == np.float32 and float(np.abs(g32.astype(np.float64) - wn).max()) <= 1e-6, (t, "f32")


@functools.lru_cache(maxsize=None)
def read_counts(k):
    """per read of the walking batch: (the counts of its k-mers in the fixture's table, their start positions, their keys)"""
    fx = ce.fixture(k)
    out = []
    for s in fx.reads:
        rk, pos = ce.read_kmers(fx, s)
        out.append((ce.count_of(fx.keys, fx.counts, rk), pos, rk))
    return out


def want_solidity(k, lo, hi):
    rc = read_counts(k)
    nk = np.array([len(c) for c, _, _ in rc], np.uint32)
    ns = np.array([int(((c >= lo) & (c <= hi)).sum()) for c, _, _ in rc], np.uint32)
    fw = np.array([int(p[(c < lo) | (c > hi)].min(initial=NO)) for c, p, _ in rc], np.uint32)
    return nk, ns, fw


@pytest.mark.gpu
@pytest.mark.parametrize("k", KS)
def test_read_solidity_at_every_edge(torch_mod, ctx, capfd, tables, make_counter, oracle, k):
    fx = ce.fixture(k)
    bases, offsets = fx.reads_csr
    n = len(fx.reads)
    parts = part_tables(make_counter, k, 3)
    for c, tag in each_form(torch_mod, ctx, capfd, tables, k):
        for lo, hi in WINDOWS:
            want = want_solidity(k, lo, hi)
            got = c.read_solidity_host(bases, offsets, lo, hi)
            for g, w, name in zip(got, want, ("n_kmers", "n_solid", "first_weak")):
                assert same(g, w), (tag, lo, hi, name)
            if "form probing" in tag:
                nk, ns, fw = np.zeros(n, np.uint32), np.zeros(n, np.uint32), np.full(n, NO, np.uint32)
                for p, part in enumerate(parts):
                    part.read_solidity(bases, offsets, n, lo, hi, nk, ns, fw, 0, 3, p)
                for g, w, name in zip((nk, ns, fw), want, ("n_kmers", "n_solid", "first_weak")):
                    assert same(g, w), (tag, lo, hi, name, "three partitions")
    assert want_solidity(k, U32, U32)[1].sum() > 0


@pytest.mark.gpu
@pytest.mark.parametrize("k", KS)
def test_profile_is_the_count_capped_and_its_stats(torch_mod, ctx, capfd, tables, oracle, k):
    fx = ce.fixture(k)
    bases, offsets = fx.reads_csr
    want = want_profile(oracle, fx.reads, k, model(k))
    real = np.full(len(want), NO, np.uint32)  # the uncapped counts, for the one value the cap moves
    starts = np.zeros(len(want), bool)
    at = 0
    for (c, pos, _), s in zip(read_counts(k), fx.reads):
        real[at + pos] = c
        starts[at + pos] = True
        at += len(s)
    moved = starts & (real == U32)
    assert moved.any() and (want[moved] == U32 - 1).all() and same(want[~moved], real[~moved])
    assert (want[~starts] == NO).all() and (want[starts] != NO).all()
    stats = want_stats(want, offsets)
    assert int(stats["sum"].max()) > 2 ** 33
    for c, tag in each_form(torch_mod, ctx, capfd, tables, k):
        got = c.profile_host(bases, offsets)
        assert same(got, want), tag
        st = ctx.profile_stats_host(got, offsets)
        for name in stats:
            assert same(st[name], stats[name]), (tag, name)


def substituted_reads(k):
    """the walking reads with one substituted base each (where a read has a base to substitute), and a read across the unitig
    whose nodes all stand at 2^32 - 1 with its middle base substituted"""
    fx = ce.fixture(k)
    rng = np.random.default_rng(7400 + k)
    out = []
    big = next(u[0] for u in fx.unitigs if u[3] >= 3 and u[1] == u[3] * U32)
    for s in [big.encode()] + list(fx.reads):
        s = np.frombuffer(s, np.uint8).copy()
        if len(s):
            at = len(s) // 2 if not out else int(rng.integers(0, len(s)))
            if chr(s[at]).upper() in "ACGT":
                s[at] = ord("ACGT"[("ACGT".index(chr(s[at]).upper()) + 1 + int(rng.integers(0, 3))) % 4])
        out.append(s.tobytes())
    return out


CORRECT_WINDOWS = ((2 ** 31, 2 ** 31), (U32 - 1, U32 - 1), (U32 - 1, U32), (U32, U32), (2 ** 31, U32))


@functools.lru_cache(maxsize=None)
def correct_case(k):
    """the substituted reads, their profile and, per count window, the restated (covered, support, apply)"""
    from oracle import kt_oracle
    m = model(k)
    seqs = substituted_reads(k)
    bases, offsets = ce.to_csr(seqs)
    prof = want_profile(kt_oracle, seqs, k, m)
    want = {}
    for lo, hi in CORRECT_WINDOWS:
        sup = want_support(kt_oracle, bases, offsets, k, m, prof, lo, hi)
        want[(lo, hi)] = (want_covered(prof, offsets, k, lo, hi), sup, want_apply(bases, offsets, sup))
    return seqs, bases, offsets, prof, want


@pytest.mark.parametrize("k", KS)
def test_the_two_meanings_of_0xffffffff_in_the_restatement(oracle, k):
    """include/kmertools_hip.h, at kt_ctr_correct_support and kt_ctr_read_solidity: a k-mer with 0xFFFFFFFF occurrences is
    solid for the filter and for a substituted k-mer (both probe the table), reads as 0xFFFFFFFE in a profile, and so does
    not cover with min_count == 0xFFFFFFFF.  Here on the restatement, which the GPU test holds the library to: the first
    read is the unitig whose nodes all stand at 2^32 - 1, with its middle base substituted."""
    fx = ce.fixture(k)
    seqs, bases, offsets, prof, want = correct_case(k)
    orig = next(u[0] for u in fx.unitigs if u[3] >= 3 and u[1] == u[3] * U32).encode()
    L, at = len(orig), len(orig) // 2
    assert L >= k + 2 and len(seqs[0]) == L and [i for i in range(L) if seqs[0][i] != orig[i]] == [at]
    rk, _ = ce.read_kmers(fx, orig)
    assert (ce.count_of(fx.keys, fx.counts, rk) == U32).all()  # the filter's view of the unsubstituted read: all solid
    whole = want_profile(oracle, [orig], k, model(k))
    assert (whole[:L - k + 1] == U32 - 1).all()                # the profile's view of the same k-mers
    cov, sup, (out, ns, na) = want[(U32, U32)]
    assert not cov[:L].any(), "0xFFFFFFFE in the profile must not cover with min_count == 0xFFFFFFFF"
    x = "ACGT".index(chr(orig[at]))
    windows_over = min(at, L - k) - max(0, at - k + 1) + 1
    assert (int(sup[at]) >> (8 * x)) & 255 == windows_over, "the substituted k-mers count with their real 0xFFFFFFFF"
    if sum(1 for y in range(4) if (int(sup[at]) >> (8 * y)) & 255) == 1:  # (no chance k-mer supports another base)
        assert out[at] == orig[at], "the base is repaired"
    assert not want_covered(whole, np.array([0, L], np.uint64), k, U32, U32).any()
    assert want_covered(whole, np.array([0, L], np.uint64), k, U32 - 1, U32).all()
    for w in CORRECT_WINDOWS:
        assert want[w][1].any(), w


@pytest.mark.gpu
@pytest.mark.parametrize("k", KS)
def test_correct_support_at_the_top_counts(torch_mod, ctx, capfd, tables, oracle, k):
    """solid only because of a count at 2^31, 2^32 - 2 or 2^32 - 1 - and the documented corner, min_count == max_count ==
    0xFFFFFFFF (test_the_two_meanings_of_0xffffffff_in_the_restatement says what the restatement holds there)"""
    fx = ce.fixture(k)
    seqs, bases, offsets, prof, want = correct_case(k)
    n = len(seqs)
    c, tag = tables.get(torch_mod, ctx, capfd, k, "probing")
    assert same(c.profile_host(bases, offsets), prof), tag
    for lo, hi in CORRECT_WINDOWS:
        cov, wsup, (wo, ws, wa) = want[(lo, hi)]
        sup = np.zeros(len(bases), np.uint32)
        c.correct_support(bases, offsets, n, prof, lo, hi, sup, mem=0)
        assert same(sup, wsup), (tag, lo, hi)
        out, ns, na = np.zeros_like(bases), np.zeros(n, np.uint32), np.zeros(n, np.uint32)
        ctx.correct_apply(bases, offsets, n, sup, 1, 0, out, ns, na, mem=0)
        assert same(out, wo) and same(ns, ws) and same(na, wa), (tag, lo, hi)
        go, gs, ga = c.correct_host(bases, offsets, lo, hi)
        assert same(go, wo) and same(gs, ws) and same(ga, wa), (tag, lo, hi, "correct_host")
    # the filter's side of the corner: every k-mer of the unsubstituted first read is solid for (0xFFFFFFFF, 0xFFFFFFFF)
    orig = next(u[0] for u in fx.unitigs if u[3] >= 3 and u[1] == u[3] * U32).encode()
    nk, ns, fw = c.read_solidity_host(*ce.to_csr([orig]), U32, U32)
    assert nk[0] == ns[0] == len(orig) - k + 1 and fw[0] == NO, tag


@pytest.mark.gpu
@pytest.mark.parametrize("k", KS)
def test_graph_windows_that_separate_neighbours(torch_mod, ctx, capfd, tables, oracle, k):
    fx = ce.fixture(k)
    wins = [(1, U32), (U32, U32), (1, U32 - 1)]
    for b in ce.STRADDLES:
        wins += [(b, U32), (1, b - 1), (b - 1, b - 1), (b, b), (b - 1, b)]
    want = {w: gr.restate(fx.keys, fx.counts, k, *w) for w in wins}
    for c, tag in each_form(torch_mod, ctx, capfd, tables, k):
        for w in wins:
            wk, wi, wc, wcen = want[w]
            gk, gi, gc, gcen = c.graph(w[0], w[1], census=True)
            assert same(gk, wk) and same(gi, wi) and same(gc, wc), (tag, w)
            assert same(gcen, wcen), (tag, w, gcen[:7].tolist(), wcen[:7].tolist())
    assert int(want[(1, U32)][3][1]) > 2 ** 40


@functools.lru_cache(maxsize=None)
def links_ref(k, lo, hi):
    return lr.links(ce.fixture(k).table, k, lo, hi)


def check_unitigs(c, ref, lo, hi, tag):
    us, ls = ref
    bases, offsets, sums, flags, link_offsets, link_to = c.unitig_links(lo, hi)
    got = [bases[int(offsets[i]):int(offsets[i + 1])].tobytes().decode() for i in range(len(offsets) - 1)]
    assert got == [u[0] for u in us], tag
    assert sums.dtype == np.uint64 and [int(x) for x in sums] == [u[1] for u in us], tag
    assert flags.tolist() == [u[2] for u in us], tag
    wo, wt = lr.as_arrays(ls)
    assert same(link_offsets, wo) and same(link_to, wt), tag
    b2, o2, s2, f2 = c.unitigs(lo, hi)
    assert same(b2, bases) and same(o2, offsets) and same(s2, sums) and same(f2, flags), tag
    return us, ls


@pytest.mark.gpu
@pytest.mark.parametrize("k", KS)
def test_unitigs_and_links_count_sums(torch_mod, ctx, capfd, tables, oracle, k):
    fx = ce.fixture(k)
    for c, tag in each_form(torch_mod, ctx, capfd, tables, k):
        for lo, hi in ((1, U32), (2 ** 31, U32), (1, 2 ** 31 - 1), (U32, U32)) if "form probing" in tag else ((1, U32),):
            us, _ = check_unitigs(c, links_ref(k, lo, hi), lo, hi, (tag, lo, hi))
            if (lo, hi) == (1, U32):
                assert fx.big_sum in [u[1] for u in us] and fx.big_sum > 2 ** 33
            else:  # (a window can only join that unitig to more nodes of 2^32 - 1, never split it)
                assert hi < U32 or max(u[1] for u in us) >= fx.big_sum


def check_tips(c, table, k, tip, lo, hi, tag):
    us, ls, marks, tally = tr.marks(table, k, tip, lo, hi)
    gm, gt = c.unitig_tips(tip, lo, hi)
    assert gm.tolist() == marks and [int(x) for x in gt] == tally, (tag, gm.tolist(), marks)
    return us, marks


@pytest.mark.gpu
@pytest.mark.parametrize("k", KS)
def test_tips_and_clip_on_the_fixture(torch_mod, ctx, capfd, tables, make_counter, oracle, k):
    fx = ce.fixture(k)
    c, tag = tables.get(torch_mod, ctx, capfd, k, "probing")
    n_tips = 0
    for tip, lo, hi in ((4, 1, U32), (k, 1, U32), (2 ** 31 - 2, 1, U32), (k, 2 ** 24, U32), (k, 1, 2 ** 31 - 1)):
        us, marks = check_tips(c, fx.table, k, tip, lo, hi, (tag, tip, lo, hi))
        n_tips += marks.count(tr.TIP)
        assert sum(u[1] for u in us) > 2 ** 32
    assert n_tips
    # clipping erases: the occurrence word exceeds 2^32, the survivors keep their counts
    t = make_counter(k)
    t.add_pairs_host(fx.keys, fx.counts)
    left, stats, _ = tr.clip(fx.table, k, k, 8, True)
    got = t.clip_tips(k, 8, True)
    want = dict(zip(tr.STATS, stats[:6] + [1 - stats[6]]))
    assert {n: got[n] for n in want} == want, (got, want)
    assert want["occurrences"] > 2 ** 32
    gk, gc = t.export_host()
    assert ce.strings_of(gk, gc, k) == left


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["equal means", "sums one apart", "float trap"])
def test_tip_rivals_at_the_u32_scale(torch_mod, ctx, make_counter, name):
    """two dead ends at one fork: the loser is decided by an exact comparison of c_w n_u with c_u n_w"""
    k = 15
    case = ce.tip_cases()[name]
    table = case["table"]
    c = make_counter(k, 1 << 14)
    keys = np.array([gr.key_of(s) for s in table], np.uint64)
    c.add_pairs_host(keys, np.array(list(table.values()), np.uint32))
    us, marks = check_tips(c, table, k, case["max_tip_nodes"], 1, U32, name)
    assert sorted(marks) == [tr.KEEP, tr.KEEP, tr.TIP]
    check_unitigs(c, lr.links(table, k), 1, U32, name)
    left, stats, _ = tr.clip(table, k, case["max_tip_nodes"], 8, False)
    got = c.clip_tips(case["max_tip_nodes"], 8, False)
    assert [got[n] for n in tr.STATS[:6]] == stats[:6], (name, got, stats)
    gk, gc = c.export_host()
    assert ce.strings_of(gk, gc, k) == left


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["one node at 2^32 - 2", "products either side of 2^64"])
def test_tip_rivals_whose_cross_products_pass_64_bits(torch_mod, ctx, make_counter, oracle, case):
    """two dead ends of 65 537 k-mers each at one fork, max_tip_nodes = 2^31 - 2: c n is about 2^64.
      one node at 2^32 - 2             every count 2^32 - 1 but one node of the first branch: the products differ by 65 537
                                       (both are past 2^64 by the same 2^49, so 64-bit products still order them);
      products either side of 2^64     the first branch's sum is the least c with c n >= 2^64, the second's is 65 537 less:
                                       a product kept in 64 bits wraps for the first one only and makes it the loser.
    The expected marks come from the construction (the branch with the lesser sum is the tip; the other and the trunk stay)
    and from tip_ref's rule applied to the call's own unitig and link arrays (marks_of_arrays: Python integers) - the string
    restatement would walk 131 000 nodes."""
    k, n = 31, 65537
    rng = np.random.default_rng(65537)
    trunk = ce.rand_seq(rng, 50 + k - 1)
    bu, bw = "A" + ce.rand_seq(rng, n - 1), "C" + ce.rand_seq(rng, n - 1)
    seqs = [trunk, trunk[-(k - 1):] + bu, trunk[-(k - 1):] + bw]
    ks = [oracle.count_reads(*ce.to_csr([s.encode()]), k) for s in seqs]
    keys = np.concatenate([x[0] for x in ks])
    assert len(np.unique(keys)) == 50 + 2 * n and all((x[1] == 1).all() for x in ks), "a k-mer twice: not a Y"
    assert [len(x[0]) for x in ks] == [50, n, n]
    counts = np.full(len(keys), U32, np.uint32)
    counts[:50] = 1000
    if case == "one node at 2^32 - 2":
        counts[50 + n // 2] = U32 - 1
        c_u, c_w = n * U32 - 1, n * U32  # the first branch is the tip
        assert c_u * n >= 2 ** 64
    else:
        c_w = -(-2 ** 64 // n)  # the first branch stays: its sum is the greater one
        c_u, c_w = c_w - n, c_w
        assert c_w * n >= 2 ** 64 > c_u * n and (c_w * n) % 2 ** 64 < c_u * n
        counts[50:50 + n] = rng.permutation(np.array(ce.spread(c_w, n), np.uint32))
        counts[50 + n:] = rng.permutation(np.array(ce.spread(c_u, n), np.uint32))
    c = make_counter(k, 200_000)
    c.add_pairs_host(keys, counts)
    bases, offsets, sums, flags, link_offsets, link_to = c.unitig_links()
    assert sorted(int(x) for x in sums) == [50 * 1000, c_u, c_w]
    marks, tally = c.unitig_tips(2 ** 31 - 2)
    wm, wt = tr.marks_of_arrays(offsets, sums, flags, link_offsets, link_to, k, 2 ** 31 - 2)
    assert same(marks, wm) and same(tally, wt)
    by_sum = {int(s): int(m) for s, m in zip(sums, marks)}
    assert by_sum == {50 * 1000: tr.KEEP, c_u: tr.TIP, c_w: tr.KEEP}
    assert tally.tolist() == [1, n, 0, 0]
    got = c.clip_tips(2 ** 31 - 2, 2, False)
    assert (got["tips"], got["tip_nodes"], got["occurrences"]) == (1, n, c_u) and c_u > 2 ** 47
    assert c.size() == 50 + n


@pytest.mark.gpu
@pytest.mark.parametrize("k", KS)
def test_erase_keeps_the_survivors_counts(torch_mod, ctx, capfd, make_counter, oracle, k):
    fx = ce.fixture(k)
    rng = np.random.default_rng(7500 + k)
    gone = np.zeros(len(fx.keys), bool)
    for e in EDGES:
        at = np.flatnonzero(fx.counts == e)
        gone[rng.choice(at, len(at) // 2, replace=False)] = True
    m = tm.Model(k, fx.keys[~gone], fx.counts[~gone])
    assert all((m.counts == e).sum() >= 4 for e in EDGES)
    dead = fx.keys[gone][rng.permutation(int(gone.sum()))]
    absent = np.setdiff1d(lookup_keys(k)[:200], fx.keys)
    # what the call ignores: keys the table does not hold, duplicates, KT_EMPTY_KEY, values >= 4^k
    arg = np.concatenate([dead, dead[:7], absent, np.array([2 ** 64 - 1, 4 ** k, 4 ** k + 5], np.uint64)])
    q = lookup_keys(k)
    made = []
    try:
        for form in forms_of(k):
            c, reached = raised_table(torch_mod, ctx, capfd, form, k, fx.keys, fx.counts, made)
            tag = (k, form, reached)
            assert c.erase(arg) == len(dead), tag
            assert c.size() == m.size, tag
            assert same(c.lookup_host(q), m.count(q)), tag
            gk, gc = c.export_host()
            assert same(gk, m.keys) and same(gc, m.counts), tag
            for n_bins in (3, 65537):
                hist, tot = c.spectrum(n_bins, totals=True)
                assert same(hist, want_spectrum(m.counts, n_bins)) and tot == (m.size, m.occurrences), (tag, n_bins)
            c.add_pairs_host(fx.keys[gone], fx.counts[gone])  # (a later add of an erased k-mer starts from 0)
            gk, gc = c.export_host()
            assert same(gk, fx.keys) and same(gc, fx.counts), tag
            c.close()
    finally:
        for c in made:
            c.close()


# ---- writers ------------------------------------------------------------------------------------------------------------------

MS = (1, 2, 600)
BIG_EDGES = tuple(e for e in EDGES if e >= 256)


class Reach:
    pass


@functools.lru_cache(maxsize=None)
def reach(k):
    """for every edge e >= 256 and every m of MS one key that sits at e - m and a batch of reads that brings exactly m more
    occurrences of it (the key's own k bases, m times), among the fixture's contigs five times over as the crowd: at least
    16 384 k-mers, so that the bulk paths take the batch"""
    fx = ce.fixture(k)
    R = Reach()
    n = len(BIG_EDGES) * len(MS)
    R.keys = np.setdiff1d(tm.canonical_keys(np.random.default_rng(7600 + k), k, n + 40), fx.keys)[:n]
    assert len(R.keys) == n
    R.e = np.array([e for e in BIG_EDGES for _ in MS], np.uint64)
    # (m = 600 below e = 256 would start below 0: there the key sits at 1 and the batch brings the other 255)
    R.m = np.array([min(m, e - 1) for e in BIG_EDGES for m in MS], np.uint64)
    R.start = (R.e - R.m).astype(np.uint32)
    reads = list(fx.contigs) * 5
    for key, m in zip(R.keys.tolist(), R.m.tolist()):
        s = gr.str_of(key, k)
        reads += [(s if i % 2 else gr.rc_s(s)).encode() for i in range(m)]  # (either strand)
    order = np.random.default_rng(7700 + k).permutation(len(reads))
    R.reads = [reads[i] for i in order]
    R.csr = ce.to_csr(R.reads)
    R.before = tm.Model(k)
    R.before.add_pairs(R.keys, R.start)
    R.after = R.before.copy()
    R.after.add_reads(*R.csr)
    assert R.after.occurrences - R.before.occurrences >= 16384
    assert same(R.after.count(R.keys), R.e.astype(np.uint32)) and (R.after.counts == U32).sum() == len(MS)
    return R


def check_reached(c, R, tag):
    got = c.lookup_host(R.keys)
    assert same(got, R.e.astype(np.uint32)), (tag, [(int(e), int(m), int(g)) for e, m, g in zip(R.e, R.m, got) if g != e])
    gk, gc = c.export_host()
    assert same(gk, R.after.keys) and same(gc, R.after.counts), tag
    hist, tot = c.spectrum(3, totals=True)
    assert tot == (R.after.size, R.after.occurrences), tag


@pytest.mark.gpu
@pytest.mark.parametrize("k", KS)
def test_probing_adds_reach_the_edge(torch_mod, ctx, make_counter, oracle, monkeypatch, k):
    R = reach(k)
    monkeypatch.setenv("KT_BULK", "0")
    c = make_counter(k)
    c.add_pairs_host(R.keys, R.start)
    c.add_reads_host(*R.csr)
    check_reached(c, R, (k, "add_reads"))
    c = make_counter(k)
    c.add_pairs_host(R.keys, R.start)
    for part in range(3):
        c.add_reads_host(*R.csr, n_parts=3, part=part)
    check_reached(c, R, (k, "add_reads_part x 3"))
    # add_pairs: the batch's table as pairs on top of the keys at e - m
    c = make_counter(k)
    c.add_pairs_host(R.keys, R.start)
    batch = tm.Model(k)
    batch.add_reads(*R.csr)
    c.add_pairs_host(batch.keys, batch.counts)
    check_reached(c, R, (k, "add_pairs"))
    # ... and many pairs of one key in one call whose counts sum to e, zeros among them
    c = make_counter(k)
    rng = np.random.default_rng(7800 + k)
    pk, pc = [], []
    for key, e in zip(R.keys[::len(MS)].tolist(), BIG_EDGES):
        pieces = ce.spread(e, 600 if e >= 600 else e) + [0] * 5
        pk += [key] * len(pieces)
        pc += pieces
    order = rng.permutation(len(pk))
    c.add_pairs_host(np.array(pk, np.uint64)[order], np.array(pc, np.uint32)[order])
    assert c.size() == len(BIG_EDGES)
    assert same(c.lookup_host(R.keys[::len(MS)]), np.array(BIG_EDGES, np.uint32)), k


@pytest.mark.gpu
@pytest.mark.parametrize("paged", ["0", "1"])
@pytest.mark.parametrize("pack", ["1", "0"], ids=["packed", "staged"])
@pytest.mark.parametrize("k", KS)
def test_bulk_merge_reaches_the_edge(torch_mod, ctx, make_counter, oracle, capfd, k, pack, paged):
    R = reach(k)
    c = make_counter(k)
    c.add_pairs_host(R.keys, R.start)
    capfd.readouterr()
    with Env(KT_BULK_PACK=pack, KT_BULK_PAGED=paged, **BULK_ENV):
        c.add_reads(dev(torch_mod, R.csr[0]), dev(torch_mod, R.csr[1]), len(R.reads))
    torch_mod.cuda.synchronize()
    words = the_bulk_line(capfd, (k, pack, paged), True, "merge")
    assert words[3] == ("level1=paged" if paged == "1" else "level1=exact"), words
    check_reached(c, R, (k, "bulk merge", pack, paged, " ".join(words)))


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["direct", "target"])
def test_bulk_merge_into_a_direct_table_and_a_target(torch_mod, ctx, oracle, capfd, form):
    """the direct-addressed build (k = 9, 4^9 slots) and its rebuild; a bulk batch into a table counted into an export target"""
    k = 9 if form == "direct" else 31
    fx, R = ce.fixture(k), reach(k)
    made = []
    try:
        # the contigs, bulk-built as `form` says (raised_table checks the [bulk] line; its add_pairs adds zeros here and
        # makes the probing image), then the keys at e - m
        c, reached = raised_table(torch_mod, ctx, capfd, form, k, fx.keys, fx.built, made)
        c.add_pairs_host(R.keys, R.start)
        start = tm.Model(k, fx.keys, fx.built)
        start.add_pairs(R.keys, R.start)
        gk, gc = c.export_host()
        assert same(gk, start.keys) and same(gc, start.counts), (form, reached)
        capfd.readouterr()
        with Env(**BULK_ENV):
            c.add_reads(dev(torch_mod, R.csr[0]), dev(torch_mod, R.csr[1]), len(R.reads))
        torch_mod.cuda.synchronize()
        words = the_bulk_line(capfd, form, True, "merge")
        want = start.copy()
        want.add_reads(*R.csr)
        tag = (form, reached, " ".join(words))
        assert same(c.lookup_host(R.keys), R.e.astype(np.uint32)), tag
        gk, gc = c.export_host()
        assert same(gk, want.keys) and same(gc, want.counts), tag
    finally:
        for c in made:
            c.close()


@functools.lru_cache(maxsize=None)
def heavy_batch(k):
    """one batch in which five k-mers occur 255, 256, 65 535, 65 536 and 65 537 times among the fixture's contigs: the counts
    a bulk build hands from level to level, at the widths a narrower field would cut"""
    fx = ce.fixture(k)
    times = (255, 256, 65535, 65536, 65537)
    keys = np.setdiff1d(tm.canonical_keys(np.random.default_rng(7900 + k), k, 40), fx.keys)[:len(times)]
    reads = list(fx.contigs)
    for key, t in zip(keys.tolist(), times):
        s = gr.str_of(key, k).encode()
        reads += [s] * t
    order = np.random.default_rng(7950 + k).permutation(len(reads))
    reads = [reads[i] for i in order]
    csr = ce.to_csr(reads)
    m = tm.Model(k)
    m.add_reads(*csr)
    assert same(m.count(keys), np.array(times, np.uint32))
    return csr, len(reads), m, keys, times


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["bulk", "target", "direct"])
def test_bulk_built_forms_at_the_counts_reads_reach(torch_mod, ctx, oracle, capfd, form):
    """the packed forms read as they are, walkers only: kt_table_dense_export_range, the target's filter, spectrum, export"""
    from kmertools_amd import device
    torch = torch_mod
    for k in (9,) if form == "direct" else (31, 15):
        (bases, offsets), n_reads, m, keys, times = heavy_batch(k)
        c = device.Counter(ctx, k, 4 ** k if form == "direct" else SLOTS)
        try:
            room = m.size + 9
            xk, xc = torch.zeros(room, dtype=torch.int64, device="cuda"), torch.zeros(room, dtype=torch.int32, device="cuda")
            if form == "target":
                c.export_target(xk, xc, room)
            capfd.readouterr()
            with Env(**BULK_ENV):
                c.add_reads(dev(torch, bases), dev(torch, offsets), n_reads)
            torch.cuda.synchronize()
            words = the_bulk_line(capfd, (k, form), False, BUILT_AS[form])
            tag = (k, form, " ".join(words))
            assert c.size() == m.size, tag
            wins = [(1, U32), (2, U32), (U32, U32)]
            for t in times:
                wins += [(t, t), (t, U32), (1, t), (t - 1, t + 1)]
            for lo, hi in wins:
                wk, wc = m.stage(lo, hi)
                n = c.export_stage_range(lo, hi)
                assert n == len(wk), (tag, lo, hi, n, len(wk))
                gk, gc = by_key(*c.export_fetch(0, n))
                assert same(gk, wk) and same(gc, wc), (tag, lo, hi)
            for n_bins in (2, 257, 65537):
                hist, tot = c.spectrum(n_bins, totals=True)
                assert same(hist, want_spectrum(m.counts, n_bins)) and tot == (m.size, m.occurrences), (tag, n_bins)
            gk, gc = c.export_host()
            assert same(gk, m.keys) and same(gc, m.counts), tag
            if form == "target":
                gk, gc = by_key(xk[:m.size].cpu().numpy().view(np.uint64), xc[:m.size].cpu().numpy().view(np.uint32))
                assert same(gk, m.keys) and same(gc, m.counts), tag
            assert same(c.lookup_host(keys), np.array(times, np.uint32)), tag  # (a prober last: it images the table)
        finally:
            c.close()


# ---- pairs with count 0 ---------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("k", KS)
def test_zero_count_pairs_add_nothing(torch_mod, ctx, make_counter, oracle, k):
    """kt_ctr_add_pairs: table[keys[i]] += counts[i], and adding 0 adds nothing - a key the table does not hold stays absent"""
    fx = ce.fixture(k)
    new = np.setdiff1d(tm.canonical_keys(np.random.default_rng(8000 + k), k, 60), fx.keys)[:30]
    m = tm.Model(k)
    c = make_counter(k)

    def check(tag):
        assert c.size() == m.size, "%s: size %d, the model's %d" % (tag, c.size(), m.size)
        q = np.concatenate([new, fx.keys[:50]])
        assert same(c.lookup_host(q), m.count(q)), tag
        gk, gc = c.export_host()
        assert same(gk, m.keys) and same(gc, m.counts), tag
        hist, tot = c.spectrum(4, totals=True)
        assert tot == (m.size, m.occurrences) and same(hist, want_spectrum(m.counts, 4)), tag

    # an all-zero call on an empty table
    for t in (c, m):
        (t.add_pairs_host if t is c else t.add_pairs)(new[:10], np.zeros(10, np.uint32))
    check("zeros into an empty table")
    assert c.size() == 0 and c.erase(new[:10]) == 0
    # [0, 5, 0] for new keys
    for t in (c, m):
        (t.add_pairs_host if t is c else t.add_pairs)(new[10:13], np.array([0, 5, 0], np.uint32))
    check("[0, 5, 0] for new keys")
    assert m.size == 1 and c.lookup_host(new[10:13]).tolist() == [0, 5, 0]
    # zeros for keys the table holds, among edge counts for others; a key with a zero and a count in the one call
    c.add_pairs_host(fx.keys, fx.counts)
    m.add_pairs(fx.keys, fx.counts)
    pk = np.concatenate([fx.keys[:400], new[13:20], new[13:16]])
    pc = np.concatenate([np.zeros(400, np.uint32), np.zeros(7, np.uint32), np.array([U32, 1, 2 ** 31], np.uint32)])
    for t in (c, m):
        (t.add_pairs_host if t is c else t.add_pairs)(pk, pc)
    check("zeros for keys the table holds")
    assert c.lookup_host(new[13:20]).tolist() == [U32, 1, 2 ** 31, 0, 0, 0, 0]
    # the erase bookkeeping: only what is there goes
    assert c.erase(np.concatenate([new, fx.keys[:5]])) == 1 + 3 + 5
    m = tm.Model(k, *[a[~np.isin(m.keys, np.concatenate([new, fx.keys[:5]]))] for a in (m.keys, m.counts)])
    check("after the erase")
