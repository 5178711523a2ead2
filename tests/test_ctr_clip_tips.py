"""Tip clipping on the GPU: kt_ctr_erase against a model of the table, kt_ctr_unitig_tips and kt_ctr_clip_tips against the
reference of tests/tip_ref.py (which test_ctr_clip_tips_cli_args.py pins, on the CPU, to worked answers and to its invariant)
- the worked answers through add_pairs and through reads, every k that takes another path, every form a table can be in,
erases inside probe chains that wrap at a range's end, unitig counts around the scan tiles, the shapes and argument errors
of the calls between guards, the scratch claims between other entry points; and `kmertools unitigs --clip-tips` end to end.
Every comparison is exact."""
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
import table_model as tm  # noqa: E402
import test_ctr_unitig_links as tl  # noqa: E402  (the six arrays of the linked call, compared)
import test_ctr_unitigs as tu  # noqa: E402  (its table builders and forms)
import tip_ref as tr  # noqa: E402
import unitig_link_ref as lr  # noqa: E402
import unitig_ref as ur  # noqa: E402

U32 = 0xFFFFFFFF
EMPTY = 0xFFFFFFFFFFFFFFFF
GUARD = 64
MG, TG, STG = 0x5A, 0x4C4C4C4C4C4C4C4C, 0x3B3B3B3B3B3B3B3B  # what unwritten marks / tally / stats hold
ANY = 2**31 - 2


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


def tips_dev(torch, c, mt, lo, hi, nu):
    """device mode: marks are nu bytes at byte offset 1 of a buffer (then GUARD more), the tally lies between guards"""
    dm = torch.full((1 + nu + GUARD,), MG, dtype=torch.uint8, device="cuda")
    dt = torch.from_numpy(np.full(GUARD + 4 + GUARD, TG, np.uint64).view(np.int64)).cuda()
    got = c.unitig_tips_device(dm[1:1 + nu] if nu else None, nu, dt[GUARD:GUARD + 4], mt, lo, hi)
    torch.cuda.synchronize()
    assert got == nu, (got, nu)
    hm, ht = dm.cpu().numpy(), dt.cpu().numpy().view(np.uint64)
    assert hm[0] == MG and (hm[1 + nu:] == MG).all() and (ht[:GUARD] == TG).all() and (ht[GUARD + 4:] == TG).all(), "a guard was written"
    return hm[1:1 + nu], ht[GUARD:GUARD + 4]


def check_tips(torch, c, want_marks, want_tally, mt, lo=1, hi=None, tag=None):
    want_marks, want_tally = np.asarray(want_marks, np.uint8).reshape(-1), np.asarray(want_tally, np.uint64)
    for mode, (m, t) in (("host", c.unitig_tips(mt, lo, hi)), ("device", tips_dev(torch, c, mt, lo, hi, len(want_marks)))):
        assert m.dtype == np.uint8 and t.dtype == np.uint64 and len(m) == len(want_marks), (tag, mode, len(m), len(want_marks))
        bad = np.flatnonzero(m != want_marks)
        assert not len(bad), (tag, mode, "marks[%d] = %d, want %d (%d differ)" % (bad[0], m[bad[0]], want_marks[bad[0]], len(bad)))
        assert np.array_equal(t, want_tally), (tag, mode, t, want_tally)


def stats_list(d):
    """Counter.clip_tips' dict as the call's first seven stats"""
    return [d[n] for n in tr.STATS[:6]] + [1 - d["converged"]]


def check_table_is(torch, c, red, k, lo=1, hi=None, tag=None):
    """the table's content is the dict `red`, and its unitigs and links are the reference's of it"""
    ek, ec = c.export_host()
    wk, wc = tu.sorted_table([gr.key_of(s) for s in red], list(red.values())) if red else (np.zeros(0, np.uint64), np.zeros(0, np.uint32))
    assert c.size() == len(red) and np.array_equal(ek, wk) and np.array_equal(ec, wc), tag
    got = c.unitig_links(lo, hi)
    want = tl.reference(red, k, lo, hi)
    assert tl.first_difference(got, want) is None, (tag, tl.first_difference(got, want))


# ---- 1. worked answers ----------------------------------------------------------------------------------------------------

KNOWN = json.load(open(os.path.join(tu.GOLDEN, "clip_tips_known.json")))["cases"]


@pytest.mark.parametrize("path", ["pairs", "reads"])
@pytest.mark.parametrize("case", KNOWN, ids=lambda c: c["name"])
def test_clip_known_answers(torch_mod, ctx, case, path):
    from kmertools_amd import device
    k, mt = case["k"], case["max_tip_nodes"]
    table = gr.count_strings(case["reads"], k)

    def fresh():
        if path == "pairs":
            return tu.pairs_counter(ctx, k, *tu.sorted_table([gr.key_of(s) for s in table], list(table.values())))
        c = device.Counter(ctx, k, 1 << 16)
        c.add_reads_host(*device.to_csr(case["reads"]))
        return c

    for drop, pre in ((False, ""), (True, "drop_")):
        c = fresh()
        try:
            n = [len(u) - k + 1 for u in case["unitigs"]]
            check_tips(torch_mod, c, case[pre + "rounds"][0], tr.tally_of(case[pre + "rounds"][0], n), mt, tag=case["name"])
            got = c.clip_tips(mt, 8, drop)
            assert stats_list(got) == case[pre + "stats"][:7], (case["name"], drop, got)
            red = tr.clip(table, k, mt, 8, drop)[0]
            assert [u[0] for u in ur.unitigs(red, k)] == case[pre + "survivors"]
            check_table_is(torch_mod, c, red, k, tag=(case["name"], drop))
            assert stats_list(c.clip_tips(mt, 8, drop)) == [0] * 7  # nothing is left to clip
        finally:
            c.close()


def test_clip_two_rounds_one_at_a_time(torch_mod, ctx):
    """max_rounds 1 on the tip on a tip: the call says that it was stopped, a second call finishes the job"""
    from kmertools_amd._lib import lib
    case = next(c for c in KNOWN if c["name"] == "tip on a tip")
    k, mt = case["k"], case["max_tip_nodes"]
    table = gr.count_strings(case["reads"], k)
    c = tu.pairs_counter(ctx, k, *tu.sorted_table([gr.key_of(s) for s in table], list(table.values())))
    try:
        st = np.full(8 + 2, STG, np.uint64)
        assert lib().kt_ctr_clip_tips(c._h, 1, U32, mt, 1, 0, st[1:].ctypes.data) == 0
        red1, s1, _ = tr.clip(table, k, mt, 1)
        assert st[1:9].tolist() == s1 and s1[6] == 1 and s1[0] == 1 and st[0] == STG and st[9] == STG
        check_table_is(torch_mod, c, red1, k)
        got = c.clip_tips(mt)
        red2, s2, _ = tr.clip(red1, k, mt)
        assert stats_list(got) == s2[:7] and s2[0] == 1 and s2[6] == 0
        check_table_is(torch_mod, c, red2, k)
        assert [u[0] for u in ur.unitigs(red2, k)] == case["survivors"]
    finally:
        c.close()


# ---- 2. every k that takes another path ---------------------------------------------------------------------------------

@pytest.mark.parametrize("k", [2, 4, 10, 15, 16, 17, 30, 31])
def test_clip_k_sweep(torch_mod, ctx, oracle, k):
    bases, offsets = tu.sample(300 + k, k, n=200, genome_len=2000)
    tk, tc = tu.sorted_table(*oracle.count_reads(bases, offsets, k))
    table = tu.strings_table(tk, tc, k)
    seen = dict(tips=0, isolated=0, erased=0)
    c = tu.counter_of(ctx, k, bases, offsets, len(tk))
    try:
        for lo in (1, 2):
            for mt in (1, k, ANY):
                us, ls, m, tally = tr.marks(table, k, mt, lo)
                check_tips(torch_mod, c, m, tally, mt, lo, None, ("sweep", k, lo, mt))
                seen["tips"] += tally[0]
                seen["isolated"] += tally[2]
        n2, (k2, c2) = tu.snapshot(c)  # the marks left the table alone
        assert n2 == len(tk) and np.array_equal(k2, tk) and np.array_equal(c2, tc)
    finally:
        c.close()
    for i, (lo, mt, drop) in enumerate([(1, k, False), (1, k, True), (2, k, False), (2, k, True), (1, 1, True), (2, 1, False),
                                        (1, ANY, False), (2, ANY, True)]):
        c = tu.counter_of(ctx, k, bases, offsets, len(tk))
        try:
            got = c.clip_tips(mt, 8, drop, lo)
            red, s, _ = tr.clip(table, k, mt, 8, drop, lo)
            assert stats_list(got) == s[:7], (k, lo, mt, drop, got, s)
            ek, ec = c.export_host()
            wk, wc = tu.sorted_table([gr.key_of(x) for x in red], list(red.values()))
            assert np.array_equal(ek, wk) and np.array_equal(ec, wc), (k, lo, mt, drop)
            seen["erased"] += s[2] + s[4]
        finally:
            c.close()
    if k >= 10:  # the sample is a graph worth the name
        assert seen["tips"] > 10 and seen["erased"] > 50 and len(tk) > 3000, seen


# ---- 3. erase against a model, every form a table can be in ----------------------------------------------------------------

def erase_sets(rng, tk, k):
    """(name, the keys to erase, the keys that go)"""
    absent = tm.canonical_keys(rng, k, 40) if 4 ** k > 4 * len(tk) + 200 else np.zeros(0, np.uint64)
    absent = absent[~np.isin(absent, tk)]
    some = rng.choice(tk, min(len(tk), 50), replace=False)
    mixed = np.concatenate([some, some[:20], absent, np.full(5, EMPTY, np.uint64),
                            np.array([4 ** k, 4 ** k + 12345, (1 << 63) + 5], np.uint64), some[-3:]])
    return [("nothing", np.zeros(0, np.uint64), np.zeros(0, np.uint64)), ("one", tk[len(tk) // 3:len(tk) // 3 + 1], tk[len(tk) // 3:len(tk) // 3 + 1]),
            ("every second", tk[::2], tk[::2]), ("all", rng.permutation(tk), tk), ("mixed", rng.permutation(mixed), np.unique(some))]


def check_against_model(c, model, tk):
    assert c.size() == model.size
    assert np.array_equal(c.lookup_host(tk), model.count(tk))
    ek, ec = c.export_host()
    assert np.array_equal(ek, model.keys) and np.array_equal(ec, model.counts)
    hist, totals = c.spectrum(64, totals=True)
    wh, wt = model.spectrum(64)
    assert np.array_equal(hist, wh) and tuple(int(x) for x in totals) == tuple(wt)


def erase_round(torch, ctx, make, tk, tc, k, seed):
    rng = np.random.default_rng(seed)
    for i, (name, keys, goes) in enumerate(erase_sets(rng, tk, k)):
        c, target = make()
        try:
            before = tuple(t.clone() for t in target) if target else None
            keep = ~np.isin(tk, goes)
            model = tm.Model(k, tk[keep], tc[keep])
            if (i + seed) % 2:
                gone = c.erase(keys)
            else:  # device keys: a view into a larger tensor
                d = torch.from_numpy(np.concatenate([np.full(3, 7, np.uint64), keys]).view(np.int64)).cuda()
                gone = c.erase_device(d[3:], len(keys))
                torch.cuda.synchronize()
            assert gone == len(goes), (name, gone, len(goes))
            if target:  # the target's arrays are the caller's again: unchanged by the erase, and free to be overwritten
                torch.cuda.synchronize()
                assert torch.equal(before[0], target[0]) and torch.equal(before[1], target[1]), name
                target[0].fill_(0x1111111111111111), target[1].fill_(0x22222222)
                torch.cuda.synchronize()
            check_against_model(c, model, tk)
            assert c.erase(goes) == 0  # what is gone is not there to erase
            if name in ("all", "every second"):  # a later add starts from 0
                again = goes[:64]
                c.add_pairs_host(again, np.full(len(again), 3, np.uint32))
                model.add_pairs(again, np.full(len(again), 3, np.uint32))
                assert name != "all" or model.size == len(again)
                check_against_model(c, model, tk)
        finally:
            c.close()


@pytest.mark.parametrize("size", ["one range", "many ranges"])
@pytest.mark.parametrize("form", tu.FORMS)
def test_erase_every_table_form(torch_mod, ctx, oracle, monkeypatch, form, size):
    k = 13
    if size == "one range":  # a table below 8192 slots is a single range
        bases, offsets = tu.sample(513, k, n=24, genome_len=12000)
        cap = 4096
    else:
        bases, offsets = tu.sample(2013, k, n=1600, genome_len=12000)
        cap = 1 << 17
    tk, tc = tu.sorted_table(*oracle.count_reads(bases, offsets, k))
    assert (len(tk) < 3000) if size == "one range" else (len(tk) > 10000)
    erase_round(torch_mod, ctx, lambda: tu.table_in_form(torch_mod, ctx, form, k, bases, offsets, tk, tc, cap, monkeypatch), tk, tc, k,
                tu.FORMS.index(form))


@pytest.mark.parametrize("k", [8, 12])
def test_erase_direct_addressed(torch_mod, ctx, oracle, monkeypatch, k):
    """a table of exactly 4^k slots, straight after its bulk build and as the probing image"""
    bases, offsets = tu.sample(800 + k, k, n=300, genome_len=3000)
    tk, tc = tu.sorted_table(*oracle.count_reads(bases, offsets, k))
    for form in ("bulk", "probing"):
        def make():
            c, target = tu.table_in_form(torch_mod, ctx, form, k, bases, offsets, tk, tc, 4 ** k, monkeypatch)
            assert c.capacity() == 4 ** k
            return c, target
        erase_round(torch_mod, ctx, make, tk, tc, k, k + (form == "bulk"))


def test_erase_inside_probe_chains(torch_mod, ctx):
    """Twelve keys that all have slot 8190 of range 1 for their home, added one at a time: key i sits i slots on, keys 2..11
    past the range's end in its first slots.  The first of the chain, one in its middle and the ones on either side of the
    wrap are erased in turn: every survivor is still found, behind the holes; then the erased ones come back."""
    from kmertools_amd import device
    k, log2 = 21, 15
    chain = tm.keys_homed_at(k, log2, 1, 8190, 12)
    rng = np.random.default_rng(21)
    other = tm.canonical_keys(rng, k, 600)
    other = other[~np.isin(other, chain)]
    c = device.Counter(ctx, k, 1 << log2)
    try:
        assert c.capacity() == 1 << log2
        r, p = tm.home_of(other, k, log2)
        other = other[~((r == 1) & ((p >= 8100) | (p < 16)))]  # (the chain's slots are its own)
        assert len(other) > 500
        c.add_pairs_host(other, np.arange(1, len(other) + 1, dtype=np.uint32))
        for i, key in enumerate(chain):
            c.add_pairs_host(chain[i:i + 1], np.array([100 + i], np.uint32))
        model = tm.Model(k)
        model.add_pairs(other, np.arange(1, len(other) + 1, dtype=np.uint32))
        model.add_pairs(chain, 100 + np.arange(12, dtype=np.uint32))
        every = np.concatenate([other, chain])
        for victim in (0, 6, 1, 2, 11):
            assert c.erase(chain[victim:victim + 1]) == 1
            keep = model.keys != chain[victim]
            model = tm.Model(k, model.keys[keep], model.counts[keep])
            assert np.array_equal(c.lookup_host(every), model.count(every)), victim
            assert c.size() == model.size
        back = chain[[0, 6, 1, 2, 11]]
        c.add_pairs_host(back, np.full(5, 9, np.uint32))
        model.add_pairs(back, np.full(5, 9, np.uint32))
        check_against_model(c, model, every)
        # ... and several of one chain in one call
        assert c.erase(chain[[0, 3, 4, 11]]) == 4
        keep = ~np.isin(model.keys, chain[[0, 3, 4, 11]])
        model = tm.Model(k, model.keys[keep], model.counts[keep])
        check_against_model(c, model, every)
    finally:
        c.close()


# ---- 4. the scans and the list ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1023, 1024, 1025])
def test_clip_isolated_unitigs_around_a_tile(torch_mod, ctx, n):
    """n random 15-mers: every one an isolated unitig of one node.  Without the flag the list holds no key and the table stays;
    with it every node is listed and the table is empty."""
    k = 15
    rng = np.random.default_rng(n)
    tk = tm.canonical_keys(rng, k, n)
    tc = rng.integers(1, 9, size=n).astype(np.uint32)
    c = tu.pairs_counter(ctx, k, tk, tc)
    try:
        arrays = c.unitig_links()
        assert len(arrays[2]) == n and len(arrays[5]) == 0  # (the input's shape: no two of them are neighbours)
        check_tips(torch_mod, c, np.full(n, tr.ISOLATED, np.uint8), [0, 0, n, n], k)
        assert stats_list(c.clip_tips(k)) == [0] * 7 and c.size() == n
        ek, ec = c.export_host()
        assert np.array_equal(ek, tk) and np.array_equal(ec, tc)
        assert stats_list(c.clip_tips(k, 8, True)) == [1, 0, 0, n, n, int(tc.sum()), 0] and c.size() == 0
        assert [len(a) for a in c.unitig_links()] == [0, 1, 0, 0, 1, 0]
        c.add_pairs_host(tk[:10], tc[:10])  # the emptied table takes keys again
        assert np.array_equal(c.lookup_host(tk[:12]), np.concatenate([tc[:10], [0, 0]]))
    finally:
        c.close()


@pytest.mark.parametrize("k, n, least", [(6, 832, 513), (10, 209920, 131073)], ids=["one tile crossed", "256 tiles crossed"])
def test_clip_dense_random_tables(torch_mod, ctx, k, n, least):
    """Random distinct canonical k-mers, 0.4 of all there are: nearly every unitig is a single node with links, thousands of
    them candidates.  The answer is the rule in numpy on the call's own arrays, round by round."""
    rng = np.random.default_rng(1000 * k + n)
    tk = tl.random_canonical(rng, k, n)
    tc = rng.integers(1, 4, size=n).astype(np.uint32)
    c = tu.pairs_counter(ctx, k, tk, tc, slots=max(1 << 16, 1 << int(2 * n).bit_length()))
    try:
        erased = 0
        for rnd in range(3):
            _, offsets, sums, flags, loff, lto = c.unitig_links()
            nu = len(sums)
            assert rnd or nu >= least
            want, tally = tr.marks_of_arrays(offsets, sums, flags, loff, lto, k, k)
            check_tips(torch_mod, c, want, tally, k, tag=(k, n, rnd))
            print("dense table k=%d n=%d round %d: %d unitigs, %d links, tally %s" % (k, n, rnd, nu, len(lto), tally.tolist()))
            before = c.size()
            got = stats_list(c.clip_tips(k, 1, rnd == 1))
            occ = int(sums[want == tr.TIP].sum()) + (int(sums[want == tr.ISOLATED].sum()) if rnd == 1 else 0)
            iso = [int(tally[2]), int(tally[3])] if rnd == 1 else [0, 0]
            gone = int(tally[1]) + iso[1]
            assert got == [1 if gone else 0, int(tally[0]) if gone else 0, int(tally[1]) if gone else 0] + (iso if gone else [0, 0]) + \
                [occ if gone else 0, 1 if gone else 0], (rnd, got, tally)
            assert c.size() == before - gone
            erased += gone
        assert erased > n // 100
        ek, ec = c.export_host()  # what is left is of the table, with its counts
        assert np.isin(ek, tk).all() and np.array_equal(ec, tc[np.searchsorted(tk, ek)]) and len(ek) == n - erased
    finally:
        c.close()


# ---- 5. shapes and errors -------------------------------------------------------------------------------------------------

def raw_tips(L, t, lo=1, hi=U32, mt=5, marks=None, max_unitigs=0, nu=None, tally=None, mem=0):
    ptr = lambda x: None if x is None else (x.ctypes.data if isinstance(x, np.ndarray) else x.data_ptr())
    return L.kt_ctr_unitig_tips(t, lo, hi, mt, ptr(marks), max_unitigs, None if nu is None else C.byref(nu), ptr(tally), mem)


def test_tips_shapes(torch_mod, ctx, oracle):
    torch = torch_mod
    from kmertools_amd import device
    from kmertools_amd._lib import KT_ERR_ARG, lib
    L = lib()
    k = 23
    made = []
    try:
        empty = device.Counter(ctx, k, 1 << 16)
        made.append(empty)
        m, t = empty.unitig_tips()
        assert len(m) == 0 and t.tolist() == [0, 0, 0, 0]
        assert stats_list(empty.clip_tips()) == [0] * 7
        assert empty.erase(np.array([5, 6], np.uint64)) == 0 and empty.erase(np.zeros(0, np.uint64)) == 0
        for mem in (0, 1):
            nu = C.c_uint64(9)
            marks = np.full(8, MG, np.uint8) if mem == 0 else torch.full((8,), MG, dtype=torch.uint8, device="cuda")
            tally = np.full(6, TG, np.uint64) if mem == 0 else torch.from_numpy(np.full(6, TG, np.uint64).view(np.int64)).cuda()
            assert raw_tips(L, empty._h, marks=marks, max_unitigs=8, nu=nu, tally=tally, mem=mem) == 0 and nu.value == 0
            torch.cuda.synchronize()
            hm = marks if mem == 0 else marks.cpu().numpy()
            ht = tally if mem == 0 else tally.cpu().numpy().view(np.uint64)
            assert (hm == MG).all() and ht[:4].tolist() == [0, 0, 0, 0] and (ht[4:] == TG).all()
        bases, offsets = tu.sample(723, k)
        tk, tc = tu.sorted_table(*oracle.count_reads(bases, offsets, k))
        c = tu.counter_of(ctx, k, bases, offsets, len(tk))
        made.append(c)
        us, ls, want, tally = tr.marks(tu.strings_table(tk, tc, k), k, k)
        wnu = len(us)
        assert wnu > 20 and tally[0] > 3
        check_tips(torch, c, want, tally, k)
        for mem in (0, 1):
            # count only: no marks, the tally still filled; a null tally
            nu = C.c_uint64(9)
            t4 = np.full(4, TG, np.uint64) if mem == 0 else torch.from_numpy(np.full(4, TG, np.uint64).view(np.int64)).cuda()
            assert raw_tips(L, c._h, mt=k, nu=nu, tally=t4, mem=mem) == 0 and nu.value == wnu
            torch.cuda.synchronize()
            assert (t4 if mem == 0 else t4.cpu().numpy().view(np.uint64)).tolist() == tally
            nu = C.c_uint64(9)
            assert raw_tips(L, c._h, mt=k, nu=nu, mem=mem) == 0 and nu.value == wnu
            # room one too small: KT_ERR_ARG, the number exact, nothing written
            nu = C.c_uint64(9)
            marks = np.full(wnu + 4, MG, np.uint8) if mem == 0 else torch.full((wnu + 4,), MG, dtype=torch.uint8, device="cuda")
            t4 = np.full(4, TG, np.uint64) if mem == 0 else torch.from_numpy(np.full(4, TG, np.uint64).view(np.int64)).cuda()
            assert raw_tips(L, c._h, mt=k, marks=marks, max_unitigs=wnu - 1, nu=nu, tally=t4, mem=mem) == KT_ERR_ARG
            assert nu.value == wnu and L.kt_last_error()
            torch.cuda.synchronize()
            assert ((marks if mem == 0 else marks.cpu().numpy()) == MG).all()
            assert ((t4 if mem == 0 else t4.cpu().numpy().view(np.uint64)) == TG).all()
            # more room than needed: nothing past the result
            nu = C.c_uint64(9)
            assert raw_tips(L, c._h, mt=k, marks=marks, max_unitigs=wnu + 4, nu=nu, mem=mem) == 0 and nu.value == wnu
            torch.cuda.synchronize()
            hm = marks if mem == 0 else marks.cpu().numpy()
            assert hm[:wnu].tolist() == want and (hm[wnu:] == MG).all()
        with pytest.raises(device._lib.KmertoolsError):
            c.unitig_tips_device(torch.zeros(3, dtype=torch.uint8, device="cuda"), 3)
        # a range with no nodes
        m, t = c.unitig_tips(k, int(tc.max()) + 1)
        assert len(m) == 0 and t.tolist() == [0, 0, 0, 0]
        # stats between guards
        st = np.full(12, STG, np.uint64)
        assert L.kt_ctr_clip_tips(c._h, 1, U32, k, 8, 0, st[2:].ctypes.data) == 0
        red, s, _ = tr.clip(tu.strings_table(tk, tc, k), k, k)
        assert st[2:10].tolist() == s and (st[:2] == STG).all() and (st[10:] == STG).all() and s[0] >= 1
        assert L.kt_ctr_clip_tips(c._h, 1, U32, k, 8, 0, None) == 0  # (stats may be NULL)
        check_table_is(torch, c, red, k)
    finally:
        for t in reversed(made):
            t.close()


def test_tips_errors(torch_mod, ctx, oracle):
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
        wnu = a.unitig_tips_device(None, 0)
        n0, (k0, c0) = tu.snapshot(a)
        marks, tally, nu = np.full(wnu, MG, np.uint8), np.full(4, TG, np.uint64), C.c_uint64(77)

        def call(t=a._h, **kw):
            args = dict(marks=marks, max_unitigs=wnu, nu=nu, tally=tally, mt=k)
            args.update(kw)
            return raw_tips(L, t, **args)

        sh = keep(device.Sharded(ctx, k, 1 << 16, 1 << 16, 2, 0, ("host", lambda s, r, n: 1), connect=False))
        full = keep(device.Counter(ctx, k, 1024))
        full.add_pairs_host(np.arange(1, 5000, dtype=np.uint64) * 7919, np.ones(4999, np.uint32))
        for kw in (dict(t=None), dict(nu=None), dict(lo=0), dict(lo=3, hi=2), dict(mem=2), dict(mem=-1), dict(mt=0), dict(marks=None),
                   dict(t=sh.table._h)):
            assert call(**kw) == KT_ERR_ARG and L.kt_last_error(), kw
        assert call(t=full._h) == KT_ERR_FULL and L.kt_last_error()
        assert (marks == MG).all() and (tally == TG).all() and nu.value == 77
        dm = torch.full((wnu,), MG, dtype=torch.uint8, device="cuda")
        for kw in (dict(lo=0), dict(mt=0), dict(t=sh.table._h), dict(marks=None)):
            assert call(mem=1, **dict(dict(marks=dm, tally=None), **kw)) == KT_ERR_ARG, kw
        assert call(t=full._h, marks=dm, tally=None, mem=1) == KT_ERR_FULL
        torch.cuda.synchronize()
        assert (dm.cpu().numpy() == MG).all() and nu.value == 77
        # kt_ctr_clip_tips
        st = np.full(8, STG, np.uint64)
        clip = lambda t=a._h, lo=1, hi=U32, mt=k, rounds=8, flags=0: L.kt_ctr_clip_tips(t, lo, hi, mt, rounds, flags, st.ctypes.data)
        for kw in (dict(t=None), dict(lo=0), dict(lo=3, hi=2), dict(mt=0), dict(rounds=0), dict(rounds=1025), dict(flags=2), dict(flags=9),
                   dict(t=sh.table._h)):
            assert clip(**kw) == KT_ERR_ARG and L.kt_last_error(), kw
        assert clip(t=full._h) == KT_ERR_FULL
        assert (st == STG).all()
        # kt_ctr_erase
        keys = k0[:5].copy()
        gone = C.c_uint64(55)
        erase = lambda t=a._h, p=keys.ctypes.data, n=5, mem=0: L.kt_ctr_erase(t, p, n, C.byref(gone), mem)
        for kw in (dict(t=None), dict(p=None), dict(mem=2), dict(mem=-1), dict(t=sh.table._h)):
            assert erase(**kw) == KT_ERR_ARG and L.kt_last_error(), kw
        assert erase(t=full._h) == KT_ERR_FULL and gone.value == 55
        assert L.kt_ctr_erase(a._h, None, 0, C.byref(gone), 0) == 0 and gone.value == 0  # n == 0: nothing, and fine
        assert L.kt_ctr_erase(a._h, keys.ctypes.data, 5, None, 0) == 0  # (n_erased may be NULL)
        # no refused call changed the table; the last one took five keys
        n1, (k1, c1) = tu.snapshot(a)
        assert n1 == n0 - 5 and np.array_equal(k1, k0[5:]) and np.array_equal(c1, c0[5:])
        assert call(marks=None, max_unitigs=0) == 0 and 0 < nu.value != 77  # the context is still good
    finally:
        for c in reversed(made):
            c.close()


def test_erase_invalidates_the_staged_export(ctx):
    from kmertools_amd import device
    k = 17
    tk = tm.canonical_keys(np.random.default_rng(17), k, 300)
    c = tu.pairs_counter(ctx, k, tk, np.ones(300, np.uint32))
    try:
        assert c.export_stage_range() == 300
        assert c.erase(tk[:7]) == 7
        with pytest.raises(device._lib.KmertoolsError):  # as after an add: stage first
            c.export_fetch(0, 1)
        assert c.export_stage_range() == 293
        assert np.array_equal(np.sort(c.export_fetch(0, 293)[0]), tk[7:])
    finally:
        c.close()


# ---- 6. the scratch claims ------------------------------------------------------------------------------------------------

def test_clip_scratch_reuse(torch_mod, ctx, oracle):
    """clip, then the linked unitigs, a cov batch and a setop, then clip on a second table of the same context"""
    k = 19
    tabs = []
    try:
        for seed in (1919, 1920):
            bases, offsets = tu.sample(seed, k, n=200, genome_len=2000)
            tk, tc = tu.sorted_table(*oracle.count_reads(bases, offsets, k))
            tabs.append((tu.counter_of(ctx, k, bases, offsets, len(tk)), tu.strings_table(tk, tc, k), bases, offsets))
        a, ta, ba, oa = tabs[0]
        b, tb, _, _ = tabs[1]
        reda, sa, _ = tr.clip(ta, k, k)
        assert stats_list(a.clip_tips()) == sa[:7] and sa[1] > 3
        check_table_is(torch_mod, a, reda, k)
        cov = a.cov_host(ba, oa, 4, 8, norm=False, dtype="u32")
        ok_, oc_ = a.setop(b, "intersect")
        wk = sorted(gr.key_of(s) for s in reda if s in tb)
        assert ok_.tolist() == wk
        redb, sb, _ = tr.clip(tb, k, k, 8, True, 2)
        assert stats_list(b.clip_tips(None, 8, True, 2)) == sb[:7]
        check_table_is(torch_mod, b, redb, k, 2)
        assert np.array_equal(a.cov_host(ba, oa, 4, 8, norm=False, dtype="u32"), cov)
        check_table_is(torch_mod, a, reda, k)
    finally:
        for t in tabs:
            t[0].close()


# ---- 7. the CLI end to end ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", [15, 31])
def test_clip_cli_end_to_end(oracle, tmp_path, k):
    assert os.path.exists(tu.CLI)
    fa = tmp_path / "reads.fasta"
    cyc = np.frombuffer(b"ACGT", np.uint8)[np.random.default_rng(k).integers(0, 4, size=300)].tobytes()
    reads = tu.noisy_reads(80 + k, 250, k, 2500) + [cyc + cyc[:k - 1]] * 2
    fa.write_bytes(b"".join(b">rec%d lane=%d  sample x\n%s\n" % (i, i % 5, s) for i, s in enumerate(reads)))
    tk, tc = tu.sorted_table(*oracle.count_reads(*oracle.to_csr([s for _, s in oracle.read_records(str(fa))]), k))
    table = tu.strings_table(tk, tc, k)
    cases = (("clip", ["--clip-tips", "--gfa", "--links"], dict(), 1, U32),
             ("clip_drop", ["--clip-tips", "--drop-isolated", "--tip-nodes", 2 * k, "--min-count", 2, "--gfa"], dict(mt=2 * k, drop=True), 2, U32),
             ("clip_one", ["--clip-tips", "--clip-rounds", 1, "--tip-nodes", 3, "--links"], dict(mt=3, rounds=1), 1, U32),
             ("clip_stats", ["--clip-tips", "--stats-only", "--max-count", 6], dict(), 1, 6))
    total = 0
    for name, flags, kw, lo, hi in cases:
        red, s, _ = tr.clip(table, k, kw.get("mt", k), kw.get("rounds", 8), kw.get("drop", False), lo, hi)
        total += s[1]
        gfa, links, stats_only = "--gfa" in flags, "--links" in flags, "--stats-only" in flags
        d = tmp_path / name
        r = tu.run("unitigs", "-i", fa, "-o", d, "-k", k, *flags)
        assert r.returncode == 0, r.stderr
        files = ["unitigs.stats", "unitigs.clip.stats"] + ([] if stats_only else ["unitigs.fa"]) + (["unitigs.gfa"] if gfa else []) + \
            (["unitigs.links.stats"] if gfa or links else [])
        assert sorted(os.listdir(d)) == sorted(files)
        assert (d / "unitigs.clip.stats").read_bytes() == tr.want_clip_stats(s), (k, name)
        plain_fa, plain_stats = ur.want_files(red, k, lo, hi)
        assert (d / "unitigs.stats").read_bytes() == plain_stats, (k, name)
        if not stats_only:
            assert (d / "unitigs.fa").read_bytes() == (lr.want_fa_links(red, k, lo, hi) if links else plain_fa), (k, name)
        if gfa:
            assert (d / "unitigs.gfa").read_bytes() == lr.want_gfa(red, k, lo, hi), (k, name)
        if gfa or links:
            assert (d / "unitigs.links.stats").read_bytes() == lr.want_link_stats(red, k, lo, hi), (k, name)
    assert total > 20  # (the input's shape: there was something to clip)
    # without the new flags: the files of before, byte for byte, and no others
    want_fa, want_stats = ur.want_files(table, k)
    d = tmp_path / "plain"
    r = tu.run("unitigs", "-i", fa, "-o", d, "-k", k)
    assert r.returncode == 0, r.stderr
    assert sorted(os.listdir(d)) == ["unitigs.fa", "unitigs.stats"]
    assert (d / "unitigs.fa").read_bytes() == want_fa and (d / "unitigs.stats").read_bytes() == want_stats
