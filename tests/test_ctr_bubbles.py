"""Bubble popping on the GPU: kt_ctr_unitig_bubbles and kt_ctr_simplify against the reference of tests/bubble_ref.py (which
test_ctr_bubbles_cli_args.py pins, on the CPU, to worked answers and to its assertions) - the worked answers through add_pairs
and through reads, one round at a time, kt_ctr_simplify without the bubble rule against kt_ctr_clip_tips, two-haplotype tables
at every k that takes another path and in every form a table can be in, unitig counts around a wave, a workgroup and a scan
tile, a long genome round by round against the rule on the call's own arrays, a class of four, a count range, the argument errors of the calls between guards, the scratch claims between other entry
points; and `kmertools unitigs --pop-bubbles` end to end.  Every comparison is exact."""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import bubble_ref as br  # noqa: E402
import graph_ref as gr  # noqa: E402
import test_ctr_clip_tips as tct  # noqa: E402  (its guards, check_table_is and stats_list)
import test_ctr_unitigs as tu  # noqa: E402  (its table builders and forms)
import tip_ref as tr  # noqa: E402
import unitig_link_ref as lr  # noqa: E402
import unitig_ref as ur  # noqa: E402

U32 = 0xFFFFFFFF
GUARD = 64
MG, TG, STG = tct.MG, tct.TG, tct.STG  # what unwritten marks / tally / stats hold

torch_mod = tu.torch_mod
ctx = tu.ctx


def bubbles_dev(torch, c, mb, lo, hi, nu):
    """device mode: marks are nu bytes at byte offset 1 of a buffer (then GUARD more), the tally lies between guards"""
    dm = torch.full((1 + nu + GUARD,), MG, dtype=torch.uint8, device="cuda")
    dt = torch.from_numpy(np.full(GUARD + 4 + GUARD, TG, np.uint64).view(np.int64)).cuda()
    got = c.unitig_bubbles_device(dm[1:1 + nu] if nu else None, nu, dt[GUARD:GUARD + 4], mb, lo, hi)
    torch.cuda.synchronize()
    assert got == nu, (got, nu)
    hm, ht = dm.cpu().numpy(), dt.cpu().numpy().view(np.uint64)
    assert hm[0] == MG and (hm[1 + nu:] == MG).all() and (ht[:GUARD] == TG).all() and (ht[GUARD + 4:] == TG).all(), "a guard was written"
    return hm[1:1 + nu], ht[GUARD:GUARD + 4]


def check_bubbles(torch, c, want_marks, want_tally, mb, lo=1, hi=None, tag=None):
    want_marks, want_tally = np.asarray(want_marks, np.uint8).reshape(-1), np.asarray(want_tally, np.uint64)
    for mode, (m, t) in (("host", c.unitig_bubbles(mb, lo, hi)), ("device", bubbles_dev(torch, c, mb, lo, hi, len(want_marks)))):
        assert m.dtype == np.uint8 and t.dtype == np.uint64 and len(m) == len(want_marks), (tag, mode, len(m), len(want_marks))
        bad = np.flatnonzero(m != want_marks)
        assert not len(bad), (tag, mode, "marks[%d] = %d, want %d (%d differ)" % (bad[0], m[bad[0]], want_marks[bad[0]], len(bad)))
        assert np.array_equal(t, want_tally), (tag, mode, t, want_tally)


def stats_list(d):
    """Counter.simplify's dict as the call's first ten stats"""
    return [d[n] for n in br.STATS[:9]] + [1 - d["converged"]]


def table_arrays(table):
    return tu.sorted_table([gr.key_of(s) for s in table], list(table.values()))


def pops_only(m):
    return [x & br.POP for x in m]


# ---- 1. worked answers ----------------------------------------------------------------------------------------------------

KNOWN = json.load(open(os.path.join(tu.GOLDEN, "bubble_known.json")))["cases"]
CLIP_KNOWN = json.load(open(os.path.join(tu.GOLDEN, "clip_tips_known.json")))["cases"]


@pytest.mark.parametrize("path", ["pairs", "reads"])
@pytest.mark.parametrize("case", KNOWN, ids=lambda c: c["name"])
def test_bubble_known_answers(torch_mod, ctx, case, path):
    from kmertools_amd import device
    k, mb, mt = case["k"], case["max_bubble_nodes"], case["max_tip_nodes"]
    table = gr.count_strings(case["reads"], k)

    def fresh():
        if path == "pairs":
            return tu.pairs_counter(ctx, k, *table_arrays(table))
        c = device.Counter(ctx, k, 1 << 16)
        c.add_reads_host(*device.to_csr(case["reads"]))
        return c

    for tips, pre in ((0, ""), (mt, "tip_")):
        c = fresh()
        try:
            us = ur.unitigs(table, k)
            assert [u[0] for u in us] == case["unitigs"]
            first = pops_only(case["rounds"][0])  # (the read-only call knows the bubble rule alone)
            assert first == case["rounds"][0]
            check_bubbles(torch_mod, c, first, br.marks(table, k, mb)[3], mb, tag=case["name"])
            got = c.simplify(tips, mb)
            assert stats_list(got) == case[pre + "stats"][:10], (case["name"], tips, got)
            red = br.simplify(table, k, tips, mb)[0]
            assert [u[0] for u in ur.unitigs(red, k)] == case[pre + "survivors"]
            tct.check_table_is(torch_mod, c, red, k, tag=(case["name"], tips))
            assert stats_list(c.simplify(tips, mb)) == [0] * 10  # nothing is left to do
        finally:
            c.close()


def test_simplify_two_rounds_one_at_a_time(torch_mod, ctx):
    """max_rounds 1 on the bubble behind a tip: the call says that it was stopped, a second call pops the bubble"""
    from kmertools_amd._lib import lib
    case = next(c for c in KNOWN if c["name"] == "a bubble behind a tip")
    k, mb, mt = case["k"], case["max_bubble_nodes"], case["max_tip_nodes"]
    table = gr.count_strings(case["reads"], k)
    c = tu.pairs_counter(ctx, k, *table_arrays(table))
    try:
        st = np.full(12 + 2, STG, np.uint64)
        assert lib().kt_ctr_simplify(c._h, 1, U32, mt, mb, 1, 0, st[1:].ctypes.data) == 0
        red1, s1, _ = br.simplify(table, k, mt, mb, 1)
        assert st[1:13].tolist() == s1 and s1[9] == 1 and s1[0] == 1 and s1[1] == 1 and s1[5] == 0 and st[0] == STG and st[13] == STG
        tct.check_table_is(torch_mod, c, red1, k)
        got = c.simplify(mt, mb)
        red2, s2, _ = br.simplify(red1, k, mt, mb)
        assert stats_list(got) == s2[:10] and s2[0] == 1 and s2[9] == 0 and s2[5] == 1
        tct.check_table_is(torch_mod, c, red2, k)
        assert [u[0] for u in ur.unitigs(red2, k)] == case["tip_survivors"]
    finally:
        c.close()


@pytest.mark.parametrize("case", CLIP_KNOWN, ids=lambda c: c["name"])
def test_simplify_without_bubbles_is_clip_tips(torch_mod, ctx, case):
    k, mt = case["k"], case["max_tip_nodes"]
    table = gr.count_strings(case["reads"], k)
    for drop in (False, True):
        a, b = tu.pairs_counter(ctx, k, *table_arrays(table)), tu.pairs_counter(ctx, k, *table_arrays(table))
        try:
            clip = a.clip_tips(mt, 8, drop)
            simp = b.simplify(mt, 0, 8, drop)
            assert [simp[n] for n in tr.STATS] == [clip[n] for n in tr.STATS], (case["name"], drop, simp, clip)
            assert (simp["popped"], simp["popped_nodes"], simp["bubbles"]) == (0, 0, 0)
            ka, ca = a.export_host()
            kb, cb = b.export_host()
            assert np.array_equal(ka, kb) and np.array_equal(ca, cb) and a.size() == b.size()
            assert tct.stats_list(clip) == case["drop_stats" if drop else "stats"][:7]
        finally:
            a.close()
            b.close()


# ---- 2. two-haplotype tables: every k that takes another path, every form a table can be in --------------------------------

FORMS = tu.FORMS + ("dense bulk", "dense probing")  # dense: a table of exactly 4^k slots, for the k at which that fits
RECIPE_CASES = [(k, form) for k in (9, 12, 16, 17, 31) for form in (FORMS if k <= 12 else tu.FORMS)] + [(32, "none")]


@pytest.mark.parametrize("k, form", RECIPE_CASES)
def test_simplify_recipe_tables(torch_mod, ctx, monkeypatch, k, form):
    """k = 32: a table takes k in 1..31, so there is no form it can be in - what the case holds is that the table is refused."""
    from kmertools_amd import device
    if k == 32:
        with pytest.raises(device._lib.KmertoolsError) as ei:
            device.Counter(ctx, k, 1 << 16)
        assert ei.value.code == device._lib.KT_ERR_ARG and "1..31" in str(ei.value)
        return
    dense = form.startswith("dense")
    reads = br.two_haplotypes(7000 + 10 * k + FORMS.index(form), k)
    table = gr.count_strings(reads, k)
    tk, tc = table_arrays(table)
    bases, offsets = device.to_csr(reads)
    c, target = tu.table_in_form(torch_mod, ctx, form.replace("dense ", ""), k, bases, offsets, tk, tc, 4 ** k if dense else 1 << 16, monkeypatch)
    try:
        assert not dense or c.capacity() == 4 ** k
        us, ls, m, bt, _ = br.marks(table, k, 2 * k)
        assert bt[0] >= 4, bt
        check_bubbles(torch_mod, c, m, bt, 2 * k, tag=(k, form))
        n2, (k2, c2) = tu.snapshot(c)  # the marks left the table alone
        assert n2 == len(tk) and np.array_equal(k2, tk) and np.array_equal(c2, tc)
        red, s, rounds = br.simplify(table, k, k, 2 * k)
        got = c.simplify()
        assert stats_list(got) == s[:10] and s[1] >= 1 and s[5] >= 4, (k, form, got, s)
        tct.check_table_is(torch_mod, c, red, k, tag=(k, form))
    finally:
        c.close()


# ---- 3. the wave's tally, the workgroup, the scan tile ----------------------------------------------------------------------

def disjoint_bubbles(seed, k, n_unitigs):
    """n_unitigs // 4 genomes of 3k bases with a second haplotype (4 unitigs each) and n_unitigs % 4 plain ones (1 each)"""
    rng = np.random.default_rng(seed)
    L = list("ACGT")
    reads, seen, i = [], set(), 0
    while i < n_unitigs // 4 + n_unitigs % 4:
        g = "".join(rng.choice(L, size=3 * k))
        mine = [g, g]
        if i < n_unitigs // 4:
            p = 3 * k // 2
            mine.append(g[:p] + L[(L.index(g[p]) + 1 + i % 3) % 4] + g[p + 1:])
        # a genome with a repeat or a hairpin of its own, or one that shares k - 1 bases with an earlier one, is drawn again
        overlaps = {gr.canon_s(r[j:j + k - 1]) for r in mine for j in range(len(r) - k + 2)}
        if len(ur.unitigs(gr.count_strings(mine, k), k)) != (4 if len(mine) == 3 else 1) or overlaps & seen:
            continue
        seen |= overlaps
        reads += mine
        i += 1
    return reads


@pytest.mark.parametrize("n", [63, 64, 65, 255, 256, 257, 1023, 1024, 1025])
def test_bubbles_around_wave_block_and_tile(torch_mod, ctx, n):
    k = 15
    table = gr.count_strings(disjoint_bubbles(n, k, n), k)
    tk, tc = table_arrays(table)
    c = tu.pairs_counter(ctx, k, tk, tc, slots=1 << 17)
    try:
        _, offsets, sums, flags, loff, lto = c.unitig_links()
        assert len(sums) == n  # (the input's shape)
        want, tally = br.marks_of_arrays(offsets, sums, flags, loff, lto, k, 2 * k)
        B = n // 4
        assert tally.tolist() == [B, B * k, B, B * k] and int((want == br.POP).sum()) == B
        check_bubbles(torch_mod, c, want, tally, 2 * k, tag=n)
        both, _ = br.marks_of_arrays(offsets, sums, flags, loff, lto, k, 2 * k, k)  # the genomes' ends are tip candidates and anchors: never tips
        assert np.array_equal(both, want)
        got = c.simplify(0, 2 * k)
        assert stats_list(got) == [1, 0, 0, 0, 0, B, B * k, B, B * k, 0] and c.size() == len(tk) - B * k
        assert len(c.unitig_links()[2]) == B + n % 4
        assert stats_list(c.simplify(k, 2 * k, 8, True)) == [0] * 10
    finally:
        c.close()


def test_simplify_long_genome_against_the_array_form(torch_mod, ctx):
    """Two haplotypes of 20 000 bases and 150 reads with an error near their end: some 1600 unitigs in the first round, tips,
    bubbles and bubbles behind tips over several workgroups.  The answer is both rules in numpy on the call's own arrays,
    round by round."""
    k = 21
    reads = br.two_haplotypes(2100, k, 20000)
    rng = np.random.default_rng(2101)
    g, L = reads[0], list("ACGT")
    for _ in range(150):
        a = int(rng.integers(0, len(g) - 40))
        r = list(g[a:a + 40])
        p = 39 - int(rng.integers(0, 8))
        r[p] = L[(L.index(r[p]) + int(rng.integers(1, 4))) % 4]
        reads.append("".join(r))
    table = gr.count_strings(reads, k)
    tk, tc = table_arrays(table)
    c = tu.pairs_counter(ctx, k, tk, tc, slots=1 << 18)
    try:
        seen = dict(popped=0, tips=0)
        for rnd in range(3):
            _, offsets, sums, flags, loff, lto = c.unitig_links()
            nu = len(sums)
            assert rnd or nu > 4 * 256
            pops, bt = br.marks_of_arrays(offsets, sums, flags, loff, lto, k, 2 * k)
            check_bubbles(torch_mod, c, pops, bt, 2 * k, tag=rnd)
            tips, tt = tr.marks_of_arrays(offsets, sums, flags, loff, lto, k, k)
            tct.check_tips(torch_mod, c, tips, tt, k, tag=rnd)
            both, _ = br.marks_of_arrays(offsets, sums, flags, loff, lto, k, 2 * k, k)
            assert np.array_equal(both, pops | tips) and not ((pops != 0) & (tips != 0)).any()
            nodes = np.asarray(offsets[1:], np.int64) - np.asarray(offsets[:-1], np.int64) - (k - 1)
            gone = (both == br.TIP) | (both == br.POP)
            before = c.size()
            got = stats_list(c.simplify(k, 2 * k, 1))
            want = [1, int(tt[0]), int(tt[1]), 0, 0, int(bt[0]), int(bt[1]), int(bt[2]), int(np.asarray(sums)[gone].sum()), 1]
            assert got == (want if gone.any() else [0] * 10), (rnd, got, want)
            assert c.size() == before - int(nodes[gone].sum())
            seen["popped"] += int(bt[0])
            seen["tips"] += int(tt[0])
            print("long genome round %d: %d unitigs, bubble tally %s, tip tally %s" % (rnd, nu, bt.tolist(), tt.tolist()))
        assert seen["popped"] > 300 and seen["tips"] > 100, seen  # (some 440 substitutions, 153 reads with an error)
        ek, ec = c.export_host()  # what is left is of the table, with its counts
        assert np.isin(ek, tk).all() and np.array_equal(ec, tc[np.searchsorted(tk, ek)])
    finally:
        c.close()


# ---- 4. a class of four, a count range ---------------------------------------------------------------------------------------

def test_a_class_of_four_parallel_branches(torch_mod, ctx):
    k = 11
    rng = np.random.default_rng(411)
    g = "".join(rng.choice(list("ACGT"), size=40))
    alts = [g[:20] + x + g[21:] for x in "ACGT"]
    reads = [r for i, r in enumerate(alts) for _ in range(i + 1)]  # coverage 1, 2, 3, 4
    table = gr.count_strings(reads, k)
    us, ls, m, bt, _ = br.marks(table, k, 2 * k)
    assert len(us) == 6 and bt == [3, 3 * k, 1, (1 + 2 + 3) * k]
    c = tu.pairs_counter(ctx, k, *table_arrays(table))
    try:
        check_bubbles(torch_mod, c, m, bt, 2 * k)
        check_bubbles(torch_mod, c, [0] * 6, [0] * 4, k - 1)  # branches one node too long
        assert stats_list(c.simplify(0, 2 * k)) == [1, 0, 0, 0, 0, 3, 3 * k, 1, 6 * k, 0]
        red = br.simplify(table, k, 0, 2 * k)[0]
        assert len(ur.unitigs(red, k)) == 1 and ur.unitigs(red, k)[0][0] in (alts[3], gr.rc_s(alts[3]))
        tct.check_table_is(torch_mod, c, red, k)
    finally:
        c.close()


def test_a_count_range_turns_a_bubble_into_a_path(torch_mod, ctx):
    case = next(c for c in KNOWN if c["name"] == "SNP, unequal coverage")
    k, mb = case["k"], case["max_bubble_nodes"]
    table = gr.count_strings(case["reads"], k)
    c = tu.pairs_counter(ctx, k, *table_arrays(table))
    try:
        for lo, hi in ((1, None), (1, 3), (2, None), (1, 1), (1, 2), (2, 2)):  # (the anchors' counts are 3, the branches' 2 and 1)
            us, ls, m, bt, _ = br.marks(table, k, mb, 0, lo, hi or U32)
            check_bubbles(torch_mod, c, m, bt, mb, lo, hi, tag=(lo, hi))
            assert bt == ([1, 5, 1, 5] if (lo, hi) in ((1, None), (1, 3)) else [0] * 4)
        assert len(br.marks(table, k, mb, 0, 2)[0]) == 1  # without the weaker haplotype: one path
        assert stats_list(c.simplify(0, mb, min_count=2)) == [0] * 10 and c.size() == len(table)
    finally:
        c.close()


# ---- 5. errors -------------------------------------------------------------------------------------------------------------

def raw_bubbles(L, t, lo=1, hi=U32, mb=5, marks=None, max_unitigs=0, nu=None, tally=None, mem=0):
    ptr = lambda x: None if x is None else (x.ctypes.data if isinstance(x, np.ndarray) else x.data_ptr())
    return L.kt_ctr_unitig_bubbles(t, lo, hi, mb, ptr(marks), max_unitigs, None if nu is None else C.byref(nu), ptr(tally), mem)


def test_bubbles_errors_and_shapes(torch_mod, ctx):
    torch = torch_mod
    from kmertools_amd import device
    from kmertools_amd._lib import KT_ERR_ARG, KT_ERR_FULL, lib
    L = lib()
    k = 21
    reads = br.two_haplotypes(2121, k)
    table = gr.count_strings(reads, k)
    made = []

    def keep(c):
        made.append(c)
        return c

    try:
        empty = keep(device.Counter(ctx, k, 1 << 16))
        m, t = empty.unitig_bubbles()
        assert len(m) == 0 and t.tolist() == [0, 0, 0, 0] and stats_list(empty.simplify()) == [0] * 10
        a = keep(tu.pairs_counter(ctx, k, *table_arrays(table)))
        us, ls, want, wt, _ = br.marks(table, k, 2 * k)
        wnu = len(us)
        assert a.unitig_bubbles_device(None, 0) == wnu and wt[0] >= 3
        n0, (k0, c0) = tu.snapshot(a)
        marks, tally, nu = np.full(wnu + 4, MG, np.uint8), np.full(6, TG, np.uint64), C.c_uint64(77)

        def call(t=a._h, **kw):
            args = dict(marks=marks, max_unitigs=wnu, nu=nu, tally=tally, mb=2 * k)
            args.update(kw)
            return raw_bubbles(L, t, **args)

        sh = keep(device.Sharded(ctx, k, 1 << 16, 1 << 16, 2, 0, ("host", lambda s, r, n: 1), connect=False))
        full = keep(device.Counter(ctx, k, 1024))
        full.add_pairs_host(np.arange(1, 5000, dtype=np.uint64) * 7919, np.ones(4999, np.uint32))
        for kw in (dict(t=None), dict(nu=None), dict(lo=0), dict(lo=3, hi=2), dict(mem=2), dict(mem=-1), dict(mb=0), dict(marks=None),
                   dict(t=sh.table._h)):
            assert call(**kw) == KT_ERR_ARG and L.kt_last_error(), kw
        assert call(t=full._h) == KT_ERR_FULL and L.kt_last_error()
        assert (marks == MG).all() and (tally == TG).all() and nu.value == 77
        # room one too small: the number exact, nothing written; more room than needed: nothing past the result
        assert call(max_unitigs=wnu - 1) == KT_ERR_ARG and nu.value == wnu and (marks == MG).all() and (tally == TG).all()
        assert call(max_unitigs=wnu + 4) == 0 and marks[:wnu].tolist() == want and (marks[wnu:] == MG).all()
        assert tally[:4].tolist() == wt and (tally[4:] == TG).all()
        nu = C.c_uint64(9)
        assert raw_bubbles(L, a._h, mb=2 * k, nu=nu) == 0 and nu.value == wnu  # count only, a null tally
        dm = torch.full((wnu,), MG, dtype=torch.uint8, device="cuda")
        dt = torch.from_numpy(np.full(4, TG, np.uint64).view(np.int64)).cuda()
        nu = C.c_uint64(77)
        for kw in (dict(lo=0), dict(mb=0), dict(t=sh.table._h), dict(marks=None), dict(max_unitigs=wnu - 1)):
            assert call(mem=1, **dict(dict(marks=dm, tally=dt, nu=nu), **kw)) == KT_ERR_ARG, kw
        assert call(t=full._h, marks=dm, tally=dt, mem=1) == KT_ERR_FULL
        torch.cuda.synchronize()
        assert (dm.cpu().numpy() == MG).all() and (dt.cpu().numpy().view(np.uint64) == TG).all()
        with pytest.raises(device._lib.KmertoolsError):
            a.unitig_bubbles_device(torch.zeros(3, dtype=torch.uint8, device="cuda"), 3)
        # kt_ctr_simplify
        st = np.full(16, STG, np.uint64)
        simp = lambda t=a._h, lo=1, hi=U32, mt=k, mb=2 * k, rounds=8, flags=0: L.kt_ctr_simplify(t, lo, hi, mt, mb, rounds, flags,
                                                                                                 st[2:].ctypes.data)
        for kw in (dict(t=None), dict(lo=0), dict(lo=3, hi=2), dict(mt=0, mb=0), dict(rounds=0), dict(rounds=1025), dict(flags=2), dict(flags=9),
                   dict(mt=0, flags=1), dict(t=sh.table._h)):
            assert simp(**kw) == KT_ERR_ARG and L.kt_last_error(), kw
        assert simp(t=full._h) == KT_ERR_FULL
        assert (st == STG).all()
        # no refused call changed the table
        n1, (k1, c1) = tu.snapshot(a)
        assert n1 == n0 and np.array_equal(k1, k0) and np.array_equal(c1, c0)
        # stats between guards; a null stats
        red, s, _ = br.simplify(table, k, k, 2 * k)
        assert simp() == 0 and st[2:14].tolist() == s and (st[:2] == STG).all() and (st[14:] == STG).all() and s[0] >= 1
        assert L.kt_ctr_simplify(a._h, 1, U32, k, 2 * k, 8, 0, None) == 0
        tct.check_table_is(torch, a, red, k)
    finally:
        for c in reversed(made):
            c.close()


# ---- 6. the scratch claims ------------------------------------------------------------------------------------------------

def test_simplify_scratch_reuse(torch_mod, ctx):
    """bubbles and simplify, then the linked unitigs, a cov batch, a setop and the tips, then simplify on a second table of the
    same context"""
    from kmertools_amd import device
    k = 19
    tabs = []
    try:
        for seed in (1919, 1920):
            reads = br.two_haplotypes(seed, k)
            table = gr.count_strings(reads, k)
            tabs.append((tu.pairs_counter(ctx, k, *table_arrays(table)), table, reads))
        a, ta, ra = tabs[0]
        b, tb, _ = tabs[1]
        ba, oa = device.to_csr(ra)
        us, ls, m, bt, _ = br.marks(ta, k, 2 * k)
        check_bubbles(torch_mod, a, m, bt, 2 * k)
        tct.check_tips(torch_mod, a, *tr.marks(ta, k, k)[2:], k)
        check_bubbles(torch_mod, a, m, bt, 2 * k)
        reda, sa, _ = br.simplify(ta, k, k, 2 * k)
        assert stats_list(a.simplify()) == sa[:10] and sa[5] >= 4
        tct.check_table_is(torch_mod, a, reda, k)
        cov = a.cov_host(ba, oa, 4, 8, norm=False, dtype="u32")
        ok_, _ = a.setop(b, "intersect")
        assert ok_.tolist() == sorted(gr.key_of(s) for s in reda if s in tb)
        redb, sb, _ = br.simplify(tb, k, k, 2 * k, 8, True, 2)
        assert stats_list(b.simplify(None, None, 8, True, 2)) == sb[:10]
        tct.check_table_is(torch_mod, b, redb, k, 2)
        redc, sc, _ = tr.clip(redb, k, k, 8, False, 2)
        assert tct.stats_list(b.clip_tips(None, 8, False, 2)) == sc[:7]
        assert np.array_equal(a.cov_host(ba, oa, 4, 8, norm=False, dtype="u32"), cov)
        tct.check_table_is(torch_mod, a, reda, k)
    finally:
        for t in tabs:
            t[0].close()


# ---- 7. the CLI end to end ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", [15, 31])
def test_bubbles_cli_end_to_end(tmp_path, k):
    assert os.path.exists(tu.CLI)
    fa = tmp_path / "reads.fasta"
    reads = [r for seed in range(4) for r in br.two_haplotypes(100 * k + seed, k)]
    fa.write_text("".join(">rec%d lane=%d\n%s\n" % (i, i % 5, s) for i, s in enumerate(reads)))
    table = gr.count_strings(reads, k)
    cases = (("pop", ["--pop-bubbles"], dict(mt=0), 1, U32),
             ("pop_clip", ["--pop-bubbles", "--clip-tips", "--gfa", "--links"], dict(), 1, U32),
             ("pop_one", ["--pop-bubbles", "--clip-tips", "--clip-rounds", 1, "--bubble-nodes", k, "--links"], dict(mb=k, rounds=1), 1, U32),
             ("pop_drop", ["--pop-bubbles", "--clip-tips", "--drop-isolated", "--tip-nodes", 2 * k, "--min-count", 2, "--gfa"],
              dict(mt=2 * k, drop=True), 2, U32),
             ("pop_stats", ["--pop-bubbles", "--clip-rounds", 3, "--stats-only", "--max-count", 6], dict(mt=0, rounds=3), 1, 6))
    popped = 0
    for name, flags, kw, lo, hi in cases:
        red, s, _ = br.simplify(table, k, kw.get("mt", k), kw.get("mb", 2 * k), kw.get("rounds", 8), kw.get("drop", False), lo, hi)
        popped += s[5]
        gfa, links, stats_only = "--gfa" in flags, "--links" in flags, "--stats-only" in flags
        d = tmp_path / name
        r = tu.run("unitigs", "-i", fa, "-o", d, "-k", k, *flags)
        assert r.returncode == 0, r.stderr
        files = ["unitigs.stats", "unitigs.simplify.stats"] + ([] if stats_only else ["unitigs.fa"]) + (["unitigs.gfa"] if gfa else []) + \
            (["unitigs.links.stats"] if gfa or links else [])
        assert sorted(os.listdir(d)) == sorted(files)
        assert (d / "unitigs.simplify.stats").read_bytes() == br.want_simplify_stats(s), (k, name)
        plain_fa, plain_stats = ur.want_files(red, k, lo, hi)
        assert (d / "unitigs.stats").read_bytes() == plain_stats, (k, name)
        if not stats_only:
            assert (d / "unitigs.fa").read_bytes() == (lr.want_fa_links(red, k, lo, hi) if links else plain_fa), (k, name)
        if gfa:
            assert (d / "unitigs.gfa").read_bytes() == lr.want_gfa(red, k, lo, hi), (k, name)
        if gfa or links:
            assert (d / "unitigs.links.stats").read_bytes() == lr.want_link_stats(red, k, lo, hi), (k, name)
    assert popped > 20  # (the input's shape: there was something to pop)
    # --clip-tips alone: its own stats file, as before, and no other
    d = tmp_path / "clip"
    r = tu.run("unitigs", "-i", fa, "-o", d, "-k", k, "--clip-tips")
    assert r.returncode == 0, r.stderr
    assert sorted(os.listdir(d)) == ["unitigs.clip.stats", "unitigs.fa", "unitigs.stats"]
    red, s, _ = tr.clip(table, k, k)
    assert (d / "unitigs.clip.stats").read_bytes() == tr.want_clip_stats(s)
    assert (d / "unitigs.fa").read_bytes() == ur.want_files(red, k)[0]
