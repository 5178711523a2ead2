"""The links between a table's unitigs: kt_ctr_unitigs_linked against the reference of tests/unitig_link_ref.py (which
test_ctr_unitig_links_cli_args.py pins, on the CPU, to worked answers and to its own invariants), through both memory
kinds - the worked answers, every k that takes another path with several count ranges, small k where palindromes, ends of 5
links and links that are their own mirror occur, unitig counts on either side of one scan tile and of the one-workgroup tile
scan's first round, one path and one cycle longer than any tile, every table form, the shapes and argument errors of the
call between guards, the unitigs byte for byte kt_ctr_unitigs's, the scratch claims between other entry points, the three
entry points that share the stages back to back in two orders; and `kmertools unitigs --gfa --links` end to end.  Every comparison is exact."""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import graph_ref as gr  # noqa: E402
import test_ctr_unitigs as tu  # noqa: E402  (its table builders, buffers and guards: the same tables, the same forms)
import tip_ref as tr  # noqa: E402
import unitig_link_ref as lr  # noqa: E402
import unitig_ref as ur  # noqa: E402

U32 = 0xFFFFFFFF
GUARD = tu.GUARD
LOG, LTG = 0x3A3A3A3A3A3A3A3A, 0x29292929  # what unwritten link_offsets / link_to hold
NAMES = ("bases", "offsets", "count_sums", "flags", "link_offsets", "link_to")


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


def reference(table, k, lo=1, hi=None):
    """the six arrays of the call for a {string: count} table"""
    us, ls = lr.links(table, k, lo, U32 if hi is None else hi)
    return tu.as_arrays(us) + lr.as_arrays(ls)


def first_difference(got, want):
    for name, g, w in zip(NAMES, got, want):
        if g.dtype != w.dtype:
            return "%s: dtype %s, want %s" % (name, g.dtype, w.dtype)
        if len(g) != len(w):
            return "%s: %d entries, want %d" % (name, len(g), len(w))
        bad = np.flatnonzero(g != w)
        if len(bad):
            return "%s[%d] = %r, want %r (%d differ)" % (name, bad[0], g[bad[0]], w[bad[0]], len(bad))
    return None if len(got) == len(want) == 6 else "not six arrays"


def links_dev(torch, c, lo, hi, nu, nb, nl):
    """device mode into views of exactly the room needed, GUARD elements of a pattern on either side of each"""
    def fenced(n, fill, dt, view):
        return torch.from_numpy(np.full(GUARD + n + GUARD, fill, dt).view(view)).cuda()
    sizes = (nb, nu + 1, nu, nu, 2 * nu + 1, nl)
    fills = (tu.BG, tu.OG, tu.SG, tu.FG, LOG, LTG)
    dts = (np.uint8, np.uint64, np.uint64, np.uint32, np.uint64, np.uint32)
    views = (np.uint8, np.int64, np.int64, np.int32, np.int64, np.int32)
    d = [fenced(n, f, dt, v) for n, f, dt, v in zip(sizes, fills, dts, views)]
    v = [t[GUARD:GUARD + n] for t, n in zip(d, sizes)]
    got = c.unitigs_linked_device(v[0], nb, v[1], v[2], v[3], nu, v[4], v[5], nl, lo, hi)
    torch.cuda.synchronize()
    assert got == (nu, nb, nl), (got, nu, nb, nl)
    h = [t.cpu().numpy().view(dt) for t, dt in zip(d, dts)]
    for a, f, n in zip(h, fills, sizes):
        assert (a[:GUARD] == f).all() and (a[GUARD + n:] == f).all(), "a guard was written"
    if nu == 0:  # no room at all is the count-only call: not even offsets[0] and link_offsets[0] are written
        assert h[1][GUARD] == tu.OG and h[4][GUARD] == LOG
        h[1], h[4] = h[1].copy(), h[4].copy()
        h[1][GUARD] = h[4][GUARD] = 0
    return tuple(a[GUARD:GUARD + n] for a, n in zip(h, sizes))


def check_both_modes(torch, c, want, lo=1, hi=None, tag=None):
    got = c.unitig_links(lo, hi)
    assert first_difference(got, want) is None, (tag, "host", first_difference(got, want))
    got = links_dev(torch, c, lo, hi, len(want[2]), len(want[0]), len(want[5]))
    assert first_difference(got, want) is None, (tag, "device", first_difference(got, want))
    return got


def table_of(reads, k):
    table = gr.count_strings(reads, k)
    tk, tc = tu.sorted_table([gr.key_of(s) for s in table], list(table.values()))
    return table, tk, tc


# ---- 1. worked answers ----------------------------------------------------------------------------------------------------

KNOWN = json.load(open(os.path.join(tu.GOLDEN, "unitig_links_known.json")))["cases"]


@pytest.mark.parametrize("case", KNOWN, ids=lambda c: c["name"])
def test_links_known_answers(torch_mod, ctx, case):
    k = case["k"]
    table, tk, tc = table_of(case["reads"], k)
    c = tu.pairs_counter(ctx, k, tk, tc)
    try:
        bases, offsets, _, _, loff, lto = c.unitig_links()
        text = bases.tobytes().decode()
        assert [text[int(offsets[i]):int(offsets[i + 1])] for i in range(len(offsets) - 1)] == case["unitigs"]
        assert [lto[int(loff[e]):int(loff[e + 1])].tolist() for e in range(len(loff) - 1)] == case["links"]
        check_both_modes(torch_mod, c, reference(table, k))
    finally:
        c.close()


# ---- 2. every k that takes another path, several count ranges -------------------------------------------------------------

@pytest.mark.parametrize("k", [1, 2, 4, 10, 15, 16, 17, 30, 31])
def test_links_k_sweep(torch_mod, ctx, oracle, k):
    bases, offsets = tu.sample(300 + k, k)
    tk, tc = tu.sorted_table(*oracle.count_reads(bases, offsets, k))
    table = tu.strings_table(tk, tc, k)
    c = tu.counter_of(ctx, k, bases, offsets, len(tk))
    try:
        snap = tu.snapshot(c)
        totals = set()
        for lo, hi in tu.RANGES:
            want = reference(table, k, lo, hi)
            check_both_modes(torch_mod, c, want, lo, hi, ("sweep", k, lo, hi))
            totals.add((len(want[2]), len(want[5])))
        if k >= 10:  # the sample is a graph worth the name: every range its own unitigs, links among those of the widest
            assert len(totals) == len(tu.RANGES) and max(nl for _, nl in totals) > 100 and len(tk) > 3000
        n2, (k2, c2) = tu.snapshot(c)  # the table's content did not change
        assert n2 == snap[0] and np.array_equal(k2, tk) and np.array_equal(c2, tc)
    finally:
        c.close()


# ---- 3. small k through add_pairs: palindromes, ends of 5 links, links that are their own mirror ---------------------------

@pytest.mark.parametrize("k", [4, 5, 6])
def test_links_small_k_through_add_pairs(torch_mod, ctx, k):
    """Even k: a k-mer that is its own reverse complement is linked under both signs, so an end whose four neighbours are all
    solid, one of them such a palindrome, has 5 links.  A link (u, +) -> (u, -) that is its own mirror needs k - 1 bases that
    are their own reverse complement, so it exists for odd k only: k = 5 stands between the two even k for it."""
    rng = np.random.default_rng(900 + k)
    pal = ("ACGCGT" if k == 6 else "ACGT") if k % 2 == 0 else None
    kinds = dict(five=0, self_mirror=0, palindrome=0, circular=0, n=0)
    for trial in range(5):
        g = "".join(rng.choice(list("ACGT"), size=int(rng.integers(20, 90))))
        cyc = "".join(rng.choice(list("ACGT"), size=int(rng.integers(3, 30))))
        reads = [g, gr.rc_s(g[5:40]), g[3:30], cyc * 3 + cyc[:k - 1], "A" * (k + 3), ("AT" * k)[:k + 3], ("ACGT" * k)[:k + 5],
                 g[:k] + gr.rc_s(g[:k])]
        if pal:
            reads += ["A" + pal[:-1] + x for x in "ACGT"]
        table, tk, tc = table_of(reads, k)
        us, ls = lr.links(table, k)
        kinds["five"] += sum(1 for fs in ls if len(fs) == 5)
        kinds["self_mirror"] += sum(1 for e, fs in enumerate(ls) if e ^ 1 in fs)
        kinds["palindrome"] += sum(1 for s, _, _, _ in us if gr.rc_s(s) == s)
        kinds["circular"] += sum(1 for u in us if u[2] & ur.CIRCULAR)
        kinds["n"] += len(table)
        c = tu.pairs_counter(ctx, k, tk, tc)
        try:
            for lo, hi in ((1, None), (2, None)):
                check_both_modes(torch_mod, c, reference(table, k, lo, hi), lo, hi, ("pairs", k, trial, lo))
        finally:
            c.close()
    # the input's shape, before anything is concluded from the comparisons
    assert kinds["n"] > 150, kinds
    assert (kinds["five"] > 0 and kinds["palindrome"] > 0) if k % 2 == 0 else kinds["self_mirror"] > 0, kinds


# ---- 4. the scan over the ends --------------------------------------------------------------------------------------------

def random_canonical(rng, k, n):
    keys = np.unique(gr.canon_np(rng.integers(0, 4 ** k, size=3 * n, dtype=np.uint64), k))
    return np.sort(rng.permutation(keys)[:n])


@pytest.mark.parametrize("k, n, least, most", [(6, 832, 513, 1024), (10, 560, 513, 1024), (10, 209920, 131073, 1 << 30)],
                         ids=["one tile crossed, dense", "one tile crossed, sparse", "256 tiles crossed"])
def test_links_scan_boundaries(torch_mod, ctx, k, n, least, most):
    """Random distinct canonical k-mers, 0.4 of all there are (6-mers: 2080, 10-mers: 524 800; a handful of 10-mers are all
    but isolated): nearly every unitig is a single node with links.  The ends, two a unitig, are scanned in tiles of 1024, the
    tiles' sums by one workgroup 256 at a time: more than 512 unitigs need a second tile, more than 131 072 a second round.
    The reference here is the string rule on arrays (links_of_arrays), over the unitigs of kt_ctr_unitigs, whose own tests
    hold them to the string-level reference; the nodes are counted against the restated graph."""
    rng = np.random.default_rng(1000 * k + n)
    tk = random_canonical(rng, k, n)
    tc = np.ones(len(tk), np.uint32)
    assert len(tk) == n
    c = tu.pairs_counter(ctx, k, tk, tc, slots=max(1 << 16, 1 << int(2 * n).bit_length()))
    try:
        bases, offsets, sums, flags = c.unitigs()
        nu = len(sums)
        assert least <= nu <= most and nu > 0.8 * n, nu
        assert len(bases) - nu * (k - 1) == n == int(gr.restate(tk, tc, k)[3][0]) and int(sums.sum()) == n
        want = (bases, offsets, sums, flags) + lr.links_of_arrays(bases, offsets, k)
        deg = np.diff(want[4].astype(np.int64))
        if n > 600:  # the dense ones: links nearly everywhere
            assert (deg > 0).mean() > 0.7 and len(want[5]) > nu
        got = check_both_modes(torch_mod, c, want, tag=("scan", k, n))
        # ... and the links as such: in range, ascending within an end, each with its mirror
        loff, lto = got[4].astype(np.int64), got[5].astype(np.int64)
        e_of = np.repeat(np.arange(2 * nu), np.diff(loff))
        assert (lto < 2 * nu).all() and ((np.diff(lto) > 0) | (np.diff(e_of) > 0)).all()
        fwd = e_of * (2 * nu) + lto
        assert np.array_equal(np.sort(fwd), np.sort((lto ^ 1) * (2 * nu) + (e_of ^ 1)))
    finally:
        c.close()


# ---- 5. one path and one cycle longer than any tile -----------------------------------------------------------------------

@pytest.mark.parametrize("shape", ["path", "cycle"])
def test_links_one_long_unitig(torch_mod, ctx, oracle, shape):
    """2500 nodes in one unitig: the ends of the path are 2499 places from each other, one of them as far from the start node;
    both branch into two single nodes.  The cycle has its two closing links and nothing else."""
    from kmertools_amd.device import to_csr
    k, N = 31, 2500
    rng = np.random.default_rng(2500 + len(shape))
    acgt = np.frombuffer(b"ACGT", np.uint8)
    if shape == "path":
        G = acgt[rng.integers(0, 4, size=N + k - 1)].tobytes()
        reads = [G] + [y + G[:k - 1] for y in (b"A", b"C")] + [G[-(k - 1):] + x for x in (b"G", b"T")]
    else:
        G = acgt[rng.integers(0, 4, size=N)].tobytes()
        reads = [G + G[:k - 1]]
    bases, offsets = to_csr(reads)
    tk, tc = tu.sorted_table(*oracle.count_reads(bases, offsets, k))
    table = tu.strings_table(tk, tc, k)
    us, ls = lr.links(table, k)
    long_ = [i for i, u in enumerate(us) if u[3] == N]
    assert len(long_) == 1 and N > 2048
    u = long_[0]
    if shape == "path":
        assert len(us) == 5 and sorted(len(ls[2 * u + s]) for s in (0, 1)) == [2, 2] and sum(map(len, ls)) == 8
    else:
        assert len(us) == 1 and us[0][2] & ur.CIRCULAR and ls == [[0], [1]]
    c = tu.counter_of(ctx, k, bases, offsets, len(tk))
    try:
        check_both_modes(torch_mod, c, tu.as_arrays(us) + lr.as_arrays(ls), tag=shape)
    finally:
        c.close()


# ---- 6. every table form before the call ----------------------------------------------------------------------------------

@pytest.mark.parametrize("size", ["one range", "many ranges"])
def test_links_every_table_form(torch_mod, ctx, oracle, monkeypatch, size):
    torch = torch_mod
    k = 13
    if size == "one range":  # a table below 8192 slots is a single range
        bases, offsets = tu.sample(513, k, n=24, genome_len=12000)
        cap = 4096
    else:
        bases, offsets = tu.sample(2013, k, n=1600, genome_len=12000)
        cap = 1 << 17
    tk, tc = tu.sorted_table(*oracle.count_reads(bases, offsets, k))
    assert (len(tk) < 3000) if size == "one range" else (len(tk) > 10000)
    lo, hi = 1, 6
    want = reference(tu.strings_table(tk, tc, k), k, lo, hi)
    assert len(want[2]) > 1 and (size == "one range" or len(want[5]) > 100)  # (the two dozen reads of the small one hardly meet)
    for form in tu.FORMS:
        for mode in ("host", "device"):
            c, target = tu.table_in_form(torch, ctx, form, k, bases, offsets, tk, tc, cap, monkeypatch)
            try:
                before = tuple(t.clone() for t in target) if target else None
                got = c.unitig_links(lo, hi) if mode == "host" else links_dev(torch, c, lo, hi, len(want[2]), len(want[0]), len(want[5]))
                assert first_difference(got, want) is None, (form, mode, first_difference(got, want))
                n, (ek, ec) = tu.snapshot(c)  # the table's content did not change
                assert n == len(tk) and np.array_equal(ek, tk) and np.array_equal(ec, tc), (form, mode)
                if target:
                    torch.cuda.synchronize()
                    assert torch.equal(before[0], target[0]) and torch.equal(before[1], target[1]), (form, mode)
            finally:
                c.close()


# ---- 7. shapes and errors -------------------------------------------------------------------------------------------------

def raw(L, t, lo=1, hi=U32, bases=None, max_bases=0, offsets=None, sums=None, flags=None, max_unitigs=0, nu=None, nb=None,
        loff=None, lto=None, max_links=0, nl=None, mem=0):
    ptr = lambda x: None if x is None else (x.ctypes.data if isinstance(x, np.ndarray) else x.data_ptr())
    ref = lambda x: None if x is None else C.byref(x)
    return L.kt_ctr_unitigs_linked(t, lo, hi, ptr(bases), max_bases, ptr(offsets), ptr(sums), ptr(flags), max_unitigs, ref(nu), ref(nb),
                                   ptr(loff), ptr(lto), max_links, ref(nl), mem)


def host_buffers(nu, nb, nl, extra=2):
    return tu.host_buffers(nu, nb, extra) + (np.full(2 * nu + 1 + extra, LOG, np.uint64), np.full(nl + extra, LTG, np.uint32))


def untouched(bufs):
    return tu.untouched(bufs[:4]) and bool((bufs[4] == LOG).all() and (bufs[5] == LTG).all())


def dev_buffers(torch, nu, nb, nl, extra=2):
    views = (np.uint8, np.int64, np.int64, np.int32, np.int64, np.int32)
    return tuple(torch.from_numpy(a.view(v)).cuda() for a, v in zip(host_buffers(nu, nb, nl, extra), views))


def dev_untouched(torch, bufs):
    torch.cuda.synchronize()
    views = (np.uint8, np.uint64, np.uint64, np.uint32, np.uint64, np.uint32)
    return untouched(tuple(t.cpu().numpy().view(v) for t, v in zip(bufs, views)))


def all_args(bufs, nu, nb, nl):
    return dict(bases=bufs[0], max_bases=nb, offsets=bufs[1], sums=bufs[2], flags=bufs[3], max_unitigs=nu, loff=bufs[4], lto=bufs[5],
                max_links=nl)


def test_links_shapes(torch_mod, ctx, oracle):
    torch = torch_mod
    from kmertools_amd import device
    from kmertools_amd._lib import KT_ERR_ARG, lib
    L = lib()
    k = 23
    made = []
    try:
        # an empty table: 0 / 0 / 0 and offsets[0] = link_offsets[0] = 0; count-only touches nothing
        empty = device.Counter(ctx, k, 1 << 16)
        made.append(empty)
        got = empty.unitig_links()
        assert [len(a) for a in got] == [0, 1, 0, 0, 1, 0] and got[1][0] == 0 and got[4][0] == 0
        n3 = [C.c_uint64(9) for _ in range(3)]
        assert raw(L, empty._h, nu=n3[0], nb=n3[1], nl=n3[2]) == 0 and [x.value for x in n3] == [0, 0, 0]
        for mem in (0, 1):
            bufs = host_buffers(3, 40, 7) if mem == 0 else dev_buffers(torch, 3, 40, 7)
            n3 = [C.c_uint64(9) for _ in range(3)]
            assert raw(L, empty._h, nu=n3[0], nb=n3[1], nl=n3[2], mem=mem, **all_args(bufs, 3, 40, 7)) == 0
            assert [x.value for x in n3] == [0, 0, 0]
            torch.cuda.synchronize()
            h = bufs if mem == 0 else [t.cpu().numpy() for t in bufs]
            o, lo_ = np.asarray(h[1]).view(np.uint64), np.asarray(h[4]).view(np.uint64)
            assert o[0] == 0 and (o[1:] == tu.OG).all() and lo_[0] == 0 and (lo_[1:] == LOG).all()
            assert (np.asarray(h[5]).view(np.uint32) == LTG).all() and (np.asarray(h[0]) == tu.BG).all()
        # a node count that is no multiple of any tile
        bases, offsets = tu.sample(723, k)
        tk, tc = tu.sorted_table(*oracle.count_reads(bases, offsets, k))
        c = tu.counter_of(ctx, k, bases, offsets, len(tk))
        made.append(c)
        want = reference(tu.strings_table(tk, tc, k), k)
        wnu, wnb, wnl = len(want[2]), len(want[0]), len(want[5])
        assert wnu > 20 and wnl > 20
        # count only: no arrays, host and device
        for mem in (0, 1):
            n3 = [C.c_uint64(9) for _ in range(3)]
            assert raw(L, c._h, nu=n3[0], nb=n3[1], nl=n3[2], mem=mem) == 0 and [x.value for x in n3] == [wnu, wnb, wnl], mem
        assert c.unitigs_linked_device(None, 0, None, None, None, 0, None, None, 0) == (wnu, wnb, wnl)
        # a range with no nodes
        top = int(tc.max()) + 1
        got = c.unitig_links(top, None)
        assert [len(a) for a in got] == [0, 1, 0, 0, 1, 0] and got[1][0] == 0 and got[4][0] == 0
        bufs = dev_buffers(torch, 3, 40, 7)
        assert c.unitigs_linked_device(bufs[0], 40, bufs[1], bufs[2], bufs[3], 3, bufs[4], bufs[5], 7, top, None) == (0, 0, 0)
        torch.cuda.synchronize()
        o, lo_ = bufs[1].cpu().numpy().view(np.uint64), bufs[4].cpu().numpy().view(np.uint64)
        assert o[0] == 0 and (o[1:] == tu.OG).all() and lo_[0] == 0 and (lo_[1:] == LOG).all()
        assert bool((bufs[5].cpu().numpy().view(np.uint32) == LTG).all())
        # count_sums / flags NULL
        b = host_buffers(wnu, wnb, wnl)
        n3 = [C.c_uint64(0) for _ in range(3)]
        assert raw(L, c._h, nu=n3[0], nb=n3[1], nl=n3[2], **dict(all_args(b, wnu, wnb, wnl), sums=None, flags=None)) == 0
        assert (b[2] == tu.SG).all() and (b[3] == tu.FG).all()
        for i, n in ((0, wnb), (1, wnu + 1), (4, 2 * wnu + 1), (5, wnl)):
            assert np.array_equal(b[i][:n], want[i]) and (b[i][n:] == (tu.BG, tu.OG, 0, 0, LOG, LTG)[i]).all(), NAMES[i]
        # each room one too small: KT_ERR_ARG, all three numbers exact, nothing written
        for mem in (0, 1):
            for short in ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 1)):
                bufs = host_buffers(wnu, wnb, wnl) if mem == 0 else dev_buffers(torch, wnu, wnb, wnl)
                n3 = [C.c_uint64(0) for _ in range(3)]
                rc = raw(L, c._h, nu=n3[0], nb=n3[1], nl=n3[2], mem=mem,
                         **all_args(bufs, wnu - short[0], wnb - short[1], wnl - short[2]))
                assert rc == KT_ERR_ARG and L.kt_last_error() and [x.value for x in n3] == [wnu, wnb, wnl], (mem, short)
                assert untouched(bufs) if mem == 0 else dev_untouched(torch, bufs), (mem, short)
        with pytest.raises(device._lib.KmertoolsError):
            bufs = dev_buffers(torch, wnu, wnb, 4)
            c.unitigs_linked_device(bufs[0], wnb, bufs[1], bufs[2], bufs[3], wnu, bufs[4], bufs[5], 4)
        # more room than needed: nothing past the result
        b = host_buffers(wnu + 5, wnb + 50, wnl + 9)
        n3 = [C.c_uint64(0) for _ in range(3)]
        assert raw(L, c._h, nu=n3[0], nb=n3[1], nl=n3[2], **all_args(b, wnu + 5, wnb + 50, wnl + 9)) == 0
        assert [x.value for x in n3] == [wnu, wnb, wnl]
        sizes = (wnb, wnu + 1, wnu, wnu, 2 * wnu + 1, wnl)
        assert first_difference(tuple(a[:n] for a, n in zip(b, sizes)), want) is None
        assert all((a[n:] == f).all() for a, n, f in zip(b, sizes, (tu.BG, tu.OG, tu.SG, tu.FG, LOG, LTG)))
    finally:
        for t in reversed(made):
            t.close()


def test_links_errors(torch_mod, ctx, oracle):
    torch = torch_mod
    from kmertools_amd import device
    from kmertools_amd._lib import KT_ERR_ARG, KT_ERR_FULL, lib
    L = lib()
    k = 21
    bases, offsets = tu.sample(6000, k)
    made = []

    def keep(c):
        made.append(c)
        return c

    try:
        a = keep(tu.counter_of(ctx, k, bases, offsets, 1 << 16))
        wnu, wnb, wnl = a.unitigs_linked_device(None, 0, None, None, None, 0, None, None, 0)
        assert wnu > 20 and wnl > 20
        bufs = host_buffers(wnu, wnb, wnl, 0)
        n3 = [C.c_uint64(77), C.c_uint64(88), C.c_uint64(99)]

        def call(t=a._h, **kw):
            args = dict(all_args(bufs, wnu, wnb, wnl), nu=n3[0], nb=n3[1], nl=n3[2])
            args.update(kw)
            return raw(L, t, **args)

        for kw in (dict(t=None), dict(nu=None), dict(nb=None), dict(nl=None), dict(lo=0), dict(lo=0, hi=0), dict(lo=3, hi=2),
                   dict(lo=U32, hi=U32 - 1), dict(mem=2), dict(mem=-1), dict(bases=None), dict(offsets=None),
                   dict(bases=None, offsets=None), dict(offsets=None, max_bases=0), dict(bases=None, max_unitigs=0),
                   dict(loff=None), dict(lto=None), dict(loff=None, lto=None), dict(loff=None, max_links=0),
                   dict(loff=None, max_links=0, max_bases=0), dict(loff=None, max_bases=0, max_unitigs=0),
                   dict(max_unitigs=0), dict(max_unitigs=0, max_bases=0)):
            assert call(**kw) == KT_ERR_ARG, kw
            assert L.kt_last_error(), kw
        sh = keep(device.Sharded(ctx, k, 1 << 16, 1 << 16, 2, 0, ("host", lambda s, r, n: 1), connect=False))
        assert call(t=sh.table._h) == KT_ERR_ARG and b"shard" in L.kt_last_error()
        full = keep(device.Counter(ctx, k, 1024))
        full.add_pairs_host(np.arange(1, 5000, dtype=np.uint64) * 7919, np.ones(4999, np.uint32))
        assert call(t=full._h) == KT_ERR_FULL and L.kt_last_error()
        # no refused call wrote anything, the sizes included
        assert untouched(bufs) and [x.value for x in n3] == [77, 88, 99]
        dbufs = dev_buffers(torch, wnu, wnb, wnl, 0)
        for t, lo, hi, want in ((a._h, 0, U32, KT_ERR_ARG), (a._h, 9, 8, KT_ERR_ARG), (sh.table._h, 1, U32, KT_ERR_ARG),
                                (full._h, 1, U32, KT_ERR_FULL)):
            rc = raw(L, t, lo, hi, nu=n3[0], nb=n3[1], nl=n3[2], mem=1, **all_args(dbufs, wnu, wnb, wnl))
            assert rc == want and L.kt_last_error(), (lo, hi)
        assert dev_untouched(torch, dbufs) and [x.value for x in n3] == [77, 88, 99]
        assert call() == 0 and [x.value for x in n3] == [wnu, wnb, wnl]  # the context is still good
    finally:
        for c in reversed(made):
            c.close()


# ---- 8. the same unitigs; the scratch claims --------------------------------------------------------------------------------

def test_links_same_unitigs_and_scratch_claims(torch_mod, ctx, oracle):
    """bases, offsets, count_sums and flags are kt_ctr_unitigs's byte for byte; kt_ctr_unitigs after a linked call, and other
    entry points between two linked calls, answer what they answer on their own"""
    k = 19
    bases, offsets = tu.sample(1919, k)
    tk, tc = tu.sorted_table(*oracle.count_reads(bases, offsets, k))
    c = tu.counter_of(ctx, k, bases, offsets, len(tk))
    try:
        for lo, hi in ((1, None), (2, 5)):
            plain = c.unitigs(lo, hi)
            linked = c.unitig_links(lo, hi)
            assert tu.same(linked[:4], plain) and all(a.tobytes() == b.tobytes() for a, b in zip(linked[:4], plain)), (lo, hi)
            assert tu.same(c.unitigs(lo, hi), plain)  # ... and after a linked call
            nu, nb, nl = len(plain[2]), len(plain[0]), len(linked[5])
            assert tu.same(tu.unitigs_dev(torch_mod, c, lo, hi, nu, nb), plain)
            assert first_difference(links_dev(torch_mod, c, lo, hi, nu, nb, nl), linked) is None
            assert tu.same(tu.unitigs_dev(torch_mod, c, lo, hi, nu, nb), plain)
        first = c.unitig_links()
        graph = c.graph(1, None, census=True)
        ek, ec = c.export_host()
        spec = c.spectrum_host(64) if hasattr(c, "spectrum_host") else None
        again = c.unitig_links()
        assert first_difference(again, first) is None
        g2 = c.graph(1, None, census=True)
        assert all(np.array_equal(x, y) for x, y in zip(graph, g2)) and np.array_equal(ek, tk) and np.array_equal(ec, tc)
        if spec is not None:
            s2 = c.spectrum_host(64)
            assert all(np.array_equal(x, y) for x, y in zip(spec, s2))
        assert first_difference(reference(tu.strings_table(tk, tc, k), k), first) is None
    finally:
        c.close()


def test_links_three_entry_points_share_stages(torch_mod, ctx):
    """kt_ctr_unitig_tips, kt_ctr_unitigs and kt_ctr_unitigs_linked run the same stages into the same scratch: on one table,
    back to back in two orders and through both memory kinds, every call answers the same each time it is made.  The table at
    k = 11 is a cycle of 40 nodes, a path seen twice with a branch of 3 nodes seen once (a tip), and single 11-mers that touch
    nothing, up to 1025 unitigs: the scan over nodes, the scan over ends and the tip kernels all cross a tile."""
    torch = torch_mod
    k, mt, NU = 11, 11, 1025
    rng = np.random.default_rng(NU)
    word = lambda n: "".join(rng.choice(list("ACGT"), size=n))
    cyc, G = word(40), word(80)
    branch = G[30:30 + k - 1] + ("A" if G[30 + k - 1] != "A" else "C") + word(2)
    table = gr.count_strings([cyc + cyc[:k - 1], G, G, branch], k)
    short = NU - len(ur.unitigs(table, k))
    while short:
        s = word(k)
        if not any(gr.canon_s(x) in table for b in "ACGT" for x in (s, s[1:] + b, b + s[:-1])):
            table[gr.canon_s(s)] = int(rng.integers(1, 5))
            short -= 1
    # the input's shape, on the CPU
    us, ls, wm, wt = tr.marks(table, k, mt)
    assert len(us) == NU and sum(1 for u in us if u[2] & ur.CIRCULAR) == 1 and wt[0] >= 1 and wt[2] >= NU - 10, wt
    want = tu.as_arrays(us) + lr.as_arrays(ls)
    nu, nb, nl = NU, len(want[0]), len(want[5])
    tk, tc = tu.sorted_table([gr.key_of(s) for s in table], list(table.values()))
    c = tu.pairs_counter(ctx, k, tk, tc)

    def tips_dev():
        dm = torch.zeros(nu, dtype=torch.uint8, device="cuda")
        dt = torch.zeros(4, dtype=torch.int64, device="cuda")
        assert c.unitig_tips_device(dm, nu, dt, mt, 1, None) == nu
        torch.cuda.synchronize()
        return dm.cpu().numpy(), dt.cpu().numpy().view(np.uint64)

    calls = {"tips": (lambda: c.unitig_tips(mt, 1, None), tips_dev),
             "unitigs": (lambda: c.unitigs(1, None), lambda: tu.unitigs_dev(torch, c, 1, None, nu, nb)),
             "linked": (lambda: c.unitig_links(1, None), lambda: links_dev(torch, c, 1, None, nu, nb, nl))}
    try:
        first = {}
        for order in (("tips", "unitigs", "linked", "tips"), ("tips", "linked", "unitigs", "tips")):
            for name in order:
                for mode, fn in zip(("host", "device"), calls[name]):
                    got = tuple(np.asarray(a).copy() for a in fn())
                    was = first.setdefault(name, got)
                    assert len(got) == len(was) and all(g.dtype == w.dtype and np.array_equal(g, w) for g, w in zip(got, was)), \
                        (order, name, mode)
        assert tu.same(first["unitigs"], first["linked"][:4])
        assert first_difference(first["linked"], want) is None, first_difference(first["linked"], want)
        am, at = tr.marks_of_arrays(*first["linked"][1:], k, mt)
        assert np.array_equal(first["tips"][0], am) and np.array_equal(first["tips"][1], at)
        assert np.array_equal(am, np.asarray(wm, np.uint8)) and at.tolist() == list(wt)
    finally:
        c.close()


# ---- 9. the CLI end to end ------------------------------------------------------------------------------------------------

def parse_gfa(text, k):
    """independent of the reference: -> (segments by id, [(u, su, v, sv)])"""
    lines = text.decode().splitlines()
    assert lines[0] == "H\tVN:Z:1.0"
    seg, ls = {}, []
    for ln in lines[1:]:
        f = ln.split("\t")
        if f[0] == "S":
            assert int(f[1]) == len(seg) and f[3] == "LN:i:%d" % len(f[2]) and f[4].startswith("KC:i:") and f[5].startswith("km:f:")
            assert f[6:] in ([], ["CL:i:1"]) and not ls, "S lines ascend and come first"
            seg[int(f[1])] = f[2]
        else:
            assert f[0] == "L" and len(f) == 6 and f[2] in "+-" and f[4] in "+-" and f[5] == "%dM" % (k - 1)
            ls.append((int(f[1]), f[2], int(f[3]), f[4]))
    return seg, ls


@pytest.mark.parametrize("k", [15, 31])
def test_links_cli_end_to_end(oracle, tmp_path, k):
    cli_bin = tu.CLI
    assert os.path.exists(cli_bin)
    fa = tmp_path / "reads.fasta"
    cyc = np.frombuffer(b"ACGT", np.uint8)[np.random.default_rng(k).integers(0, 4, size=300)].tobytes()
    reads = tu.noisy_reads(80 + k, 500, k, 4000) + [cyc + cyc[:k - 1]] * 2
    fa.write_bytes(b"".join(b">rec%d lane=%d  sample x\n%s\n" % (i, i % 5, s) for i, s in enumerate(reads)))
    tk, tc = tu.sorted_table(*oracle.count_reads(*oracle.to_csr([s for _, s in oracle.read_records(str(fa))]), k))
    table = tu.strings_table(tk, tc, k)
    cases = (("both", ["--gfa", "--links"], 1, U32, True, True),
             ("gfa", ["--gfa", "--min-count", 2, "--max-count", 5], 2, 5, True, False),
             ("fa", ["--links", "--min-count", 2], 2, U32, False, True))
    for name, flags, lo, hi, gfa, links in cases:
        plain_fa, plain_stats = ur.want_files(table, k, lo, hi)
        d = tmp_path / name
        r = tu.run("unitigs", "-i", fa, "-o", d, "-k", k, *flags)
        assert r.returncode == 0, r.stderr
        assert sorted(os.listdir(d)) == sorted(["unitigs.fa", "unitigs.stats", "unitigs.links.stats"] + (["unitigs.gfa"] if gfa else []))
        assert (d / "unitigs.stats").read_bytes() == plain_stats, (k, name)
        assert (d / "unitigs.links.stats").read_bytes() == lr.want_link_stats(table, k, lo, hi), (k, name)
        assert (d / "unitigs.fa").read_bytes() == (lr.want_fa_links(table, k, lo, hi) if links else plain_fa), (k, name)
        if not gfa:
            continue
        text = (d / "unitigs.gfa").read_bytes()
        assert text == lr.want_gfa(table, k, lo, hi), (k, name)
        seg, ls = parse_gfa(text, k)
        assert len(seg) == plain_fa.count(b">") > 20 and len(ls) > 0
        if name == "both":  # (the narrow range leaves a few stretches that hardly touch)
            assert b"\tCL:i:1\n" in text and len(ls) > 20
        orient = lambda u, s: seg[u] if s == "+" else gr.rc_s(seg[u])
        seen = set()
        for u, su, v, sv in ls:
            assert u < len(seg) and v < len(seg)
            a, b = orient(u, su), orient(v, sv)
            assert a[len(a) - (k - 1):] == b[:k - 1]
            flip = {"+": "-", "-": "+"}
            assert (u, su, v, sv) not in seen
            seen |= {(u, su, v, sv), (v, flip[sv], u, flip[su])}  # (its mirror is the same edge: not written either)
        stats = dict(ln.split(b"\t") for ln in (d / "unitigs.links.stats").read_bytes().splitlines())
        assert int(stats[b"edges"]) == len(ls) and int(stats[b"links"]) == len(seen)
    # without the new flags: the files of before, byte for byte, and no others
    want_fa, want_stats = ur.want_files(table, k)
    d = tmp_path / "plain"
    r = tu.run("unitigs", "-i", fa, "-o", d, "-k", k)
    assert r.returncode == 0, r.stderr
    assert sorted(os.listdir(d)) == ["unitigs.fa", "unitigs.stats"]
    assert (d / "unitigs.fa").read_bytes() == want_fa and (d / "unitigs.stats").read_bytes() == want_stats
