"""One kt_ctr through its whole life, every reader after every step.

A table is a small state machine (kt_internal.hpp: empty, needs_clear, dense, dense_ext, the stage, the flags, buffers kept
from call to call) and every call that reads it first brings it into a readable form - some change the form while doing so.
The reader tests each build a fresh table in one form and read it once; here ONE table and a plain model of its content
(tests/table_model.py) go through the same adds, clears, export targets and stages, and after every step every reader is
compared with the model - walkers (which take the table in the form it is in) before probers (which turn it into the probing
image) and the other way round, on torch's stream and on a stream of the context's own.  A seeded random walk over the same
transitions follows.  Everything is integers: every comparison is exact.

The conditions the script rests on (batch sizes that make the bulk build eligible, no range ever near full, keys that
collide at a range's last slot) are settled by the oracle in plan() and checked without a GPU by the tests at the top."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import table_model as tm  # noqa: E402

U32 = 0xFFFFFFFF
NO = 0xFFFFFFFF  # KT_NO_KMER
LOG2_SLOTS = 17
SLOTS = 1 << LOG2_SLOTS  # 16 ranges of 8192 slots
GUARD = 5
KPAT, CPAT, IPAT = 0x1D1D1D1D1D1D1D1D, 0x2E2E2E2E, 0x3F3F3F3F      # what output arrays hold before a call
KPAT2, CPAT2 = 0x4A4A4A4A4A4A4A4A, 0x5B5B5B5B                      # what a caller writes over arrays it got back
N_BINS, N_ROWS, N_COLS = 8, 12, 9
CLUSTER_AT = (3, 8191)  # (range, position): the last slot of range 3


# ---- reads, batches, the models of every step: made once per k, on the CPU ------------------------------------------------

def genome_of(rng, n=12000):
    return np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, size=n)]


def sample_reads(rng, genome, n, k, err):
    """test_ctr_graph.py's noisy_reads with the substitution rate as a parameter: reads of 40..200 bases from a small
    genome, runs of N, lower-case stretches, every 25th read shorter than k, some reads repeated"""
    acgt = np.frombuffer(b"ACGT", np.uint8)
    out = []
    for i in range(n):
        L = int(rng.integers(0, k)) if i % 25 == 0 else int(rng.integers(40, 200))
        a = int(rng.integers(0, len(genome) - L))
        s = genome[a:a + L].copy()
        e = rng.random(L) < err
        s[e] = acgt[rng.integers(0, 4, size=int(e.sum()))]
        if L > 50 and rng.random() < 0.15:
            p = int(rng.integers(0, L - 6))
            s[p:p + int(rng.integers(1, 6))] = ord("N")
        if L > 50 and rng.random() < 0.15:
            p = int(rng.integers(0, L - 20))
            s[p:p + 20] = np.frombuffer(bytes(s[p:p + 20]).lower(), np.uint8)
        out.append(s.tobytes())
    return out + out[:6] * 2


class Ref:
    """a model frozen at one state, with its answers computed once and kept (the parametrized cases share them)"""

    def __init__(self, model):
        self.m = model.copy()
        self._memo = {}

    def memo(self, name, fn):
        if name not in self._memo:
            self._memo[name] = fn()
        return self._memo[name]


class Plan:
    pass


@functools.lru_cache(maxsize=None)
def plan(k):
    """the script's batches and the model after every step; asserts the conditions the steps rest on"""
    from kmertools_amd.device import to_csr
    from oracle import kt_oracle
    P = Plan()
    P.k = k
    rng = np.random.default_rng(4100 + k)
    g1, g2 = genome_of(rng), genome_of(rng)
    err = 0.003
    seqs = {
        "small2": sample_reads(rng, g1, 40, k, err),
        "small5": sample_reads(rng, g2, 40, k, err),
        "bulk1": sample_reads(rng, g1, 300, k, err),
        "bulk2": sample_reads(rng, g1, 260, k, err) + sample_reads(rng, g2, 120, k, err),
        "small8": sample_reads(rng, g1, 25, k, err) + sample_reads(rng, g2, 10, k, err),
        "small11": sample_reads(rng, g2, 30, k, err),
        "tiny": sample_reads(rng, g1, 3, k, err)[1:4],
        "profile": sample_reads(rng, g1, 22, k, 0.01) + sample_reads(rng, g2, 8, k, 0.01) + [b"", b"ACGTN" * 9],
    }
    P.seqs = seqs
    P.csr = {name: to_csr(s) for name, s in seqs.items()}
    table = {name: tm.Model(k) for name in seqs}
    for name in seqs:
        table[name].add_reads(*P.csr[name])
    P.table = table

    def kmers_in(name):
        return table[name].occurrences
    # a bulk batch holds at least 16 384 k-mers - and an eighth of the slots, what a merge wants by default
    for name in ("bulk1", "bulk2"):
        assert kmers_in(name) >= 16384 and kmers_in(name) >= SLOTS // 8, (name, kmers_in(name))
        assert len(P.csr[name][0]) <= 300_000
    assert table["tiny"].size < 500  # (fits a table of 1024 slots)

    # keys that all have the last slot of a range for their home: at most one of them sits there, every other one's probe
    # sequence wraps to the range's first slots - 24 that step 3 adds, 8 that are never in any table
    cl = tm.keys_homed_at(k, LOG2_SLOTS, CLUSTER_AT[0], CLUSTER_AT[1], 32)
    r, p = tm.home_of(cl, k, LOG2_SLOTS)
    assert (r == CLUSTER_AT[0]).all() and (p == CLUSTER_AT[1]).all() and len(np.unique(cl)) == 32
    P.cluster, P.cluster_in = cl, cl[:24]
    every_read = tm.Model(k)
    for name in seqs:
        every_read._merge(table[name].keys, table[name].counts)
    assert not every_read.count(cl).any()
    P.absent = np.setdiff1d(tm.canonical_keys(rng, k, 4000), np.concatenate([every_read.keys, cl]))
    P.absent = P.absent[rng.permutation(len(P.absent))]
    assert len(P.absent) >= 3456

    # step 3: 3 000 pairs with counts 1..9 - 1 500 keys the table holds, the cluster, new keys, 20 keys twice
    m2 = table["small2"]
    assert m2.size >= 1500
    old = rng.choice(m2.keys, 1500, replace=False)
    new = P.absent[2000:2000 + 1456]
    assert len(new) == 1456
    pk = np.concatenate([old, P.cluster_in, new])
    pk = np.concatenate([pk, rng.choice(pk, 20, replace=False)])
    pk = pk[rng.permutation(len(pk))]
    P.pairs3 = (pk, rng.integers(1, 10, size=len(pk)).astype(np.uint32))
    assert len(pk) == 3000
    P.absent = P.absent[:2000]

    # the partner: about half its keys are the model's through most of the script (the first genome's k-mers)
    half = rng.choice(table["bulk1"].keys, 3000, replace=False)
    pkeys = np.unique(np.concatenate([half, tm.canonical_keys(rng, k, 3000), P.cluster_in[:5]]))
    P.partner = tm.Model(k)
    P.partner.add_pairs(pkeys, rng.integers(1, 8, size=len(pkeys)).astype(np.uint32))
    # ... and the second, small table's partner share after step 14 is whatever the tiny batch has of it

    # the model after every step
    m = tm.Model(k)
    step = {1: Ref(m)}
    m.add_reads(*P.csr["small2"]); step[2] = Ref(m)
    m.add_pairs(*P.pairs3); step[3] = Ref(m)
    P.gone_at_5 = m.keys.copy()
    m.clear(); step[4] = Ref(m)
    m.add_reads(*P.csr["small5"]); step[5] = Ref(m)
    assert not m.count(P.gone_at_5).any(), "step 5: a key of steps 2 and 3 is in the second genome's batch"
    m.clear(); m.add_reads(*P.csr["bulk1"]); step[6] = Ref(m)
    m.add_reads(*P.csr["bulk2"]); step[7] = Ref(m)
    m.add_reads(*P.csr["small8"]); step[8] = Ref(m)
    # (steps 9 to 13 count into an export target with room for the first of their batches + 9: the larger batch first)
    m.clear(); m.add_reads(*P.csr["bulk2"]); step[9] = Ref(m); step[10] = step[9]
    m.add_reads(*P.csr["small11"]); step[11] = Ref(m)
    m.clear(); m.add_reads(*P.csr["bulk1"]); step[12] = Ref(m); step[13] = step[12]
    t = tm.Model(k); t.add_reads(*P.csr["tiny"]); step[14] = Ref(t)
    P.step = step
    P.only_bulk2 = np.setdiff1d(table["bulk2"].keys, table["bulk1"].keys)
    assert len(P.only_bulk2) > 100
    P.target_room = table["bulk2"].size + 9
    assert table["bulk1"].size <= P.target_room

    # no range ever fills: the distinct keys stay below 0.6 of the slots over the whole script - settled by the oracle's
    # table of everything the script ever adds
    every = every_read.copy()
    every.add_pairs(*P.pairs3)
    direct = tm.Model(k)
    direct._merge(*kt_oracle.count_reads(*to_csr([s for name in seqs for s in seqs[name]]), k))
    assert np.array_equal(direct.keys, every_read.keys) and np.array_equal(direct.counts, every_read.counts)
    assert every.size < 0.6 * SLOTS, every.size
    assert max(r.m.size for r in step.values()) <= every.size
    P.every = every
    # the random walk's pool: its batches in any multiplicity stay inside the same key set
    P.walk_room = every.size + 9
    return P


# ---- without a GPU: the model against the oracle, the script's conditions ------------------------------------------------------

@pytest.mark.parametrize("k", [15, 31])
def test_model_equals_the_oracle_of_the_concatenated_batches(oracle, k):
    """three add_reads and one add_pairs: exactly the oracle's count_reads of the three batches as one, plus the pairs"""
    from kmertools_amd.device import to_csr
    rng = np.random.default_rng(90 + k)
    g = genome_of(rng)
    batches = [sample_reads(rng, g, n, k, 0.01) for n in (60, 35, 80)]
    m = tm.Model(k)
    for b in batches:
        m.add_reads(*to_csr(b))
    wk, wc = oracle.count_reads(*to_csr(batches[0] + batches[1] + batches[2]), k)
    order = np.argsort(wk)
    wk, wc = wk[order], wc[order]
    assert np.array_equal(m.keys, wk) and np.array_equal(m.counts, wc)
    pk = np.concatenate([rng.choice(wk, 500, replace=False), tm.canonical_keys(rng, k, 500)])
    pk = np.concatenate([pk, pk[:50]])  # (fifty keys twice in the one call)
    pc = rng.integers(1, 10, size=len(pk)).astype(np.uint32)
    m.add_pairs(pk, pc)
    want = dict(zip(wk.tolist(), wc.tolist()))
    for key, c in zip(pk.tolist(), pc.tolist()):
        want[key] = want.get(key, 0) + c
    assert m.keys.tolist() == sorted(want) and m.counts.tolist() == [want[key] for key in sorted(want)]
    assert m.keys.dtype == np.uint64 and m.counts.dtype == np.uint32
    assert m.size == len(want) and m.occurrences == sum(want.values())
    assert np.array_equal(m.count(pk[:7]), [want[key] for key in pk[:7].tolist()])
    gone = np.setdiff1d(tm.canonical_keys(rng, k, 100), m.keys)
    assert len(gone) and not m.count(gone).any()
    m.clear()
    assert m.size == 0 and not m.count(pk).any()


@pytest.mark.parametrize("k", [15, 31])
def test_script_conditions_hold(oracle, k):
    """plan() asserts them; here: that it does so without a GPU, and the restated hash against a worked placement"""
    P = plan(k)
    assert P.step[3].m.count(P.cluster_in).all() and not P.step[3].m.count(P.cluster[24:]).any()
    assert P.step[7].m.size > P.step[6].m.size > 10000
    # the restated hash: khash / nhash of small keys by hand
    if k == 31:
        h = (5 * 0x9E3779B97F4A7C15) & (2 ** 64 - 1)
        h ^= h >> 32
        x = h >> (64 - LOG2_SLOTS)
    else:
        t = ((5 * 0x9E3779B1) & 0xFFFFFFFF) << 2 & 0xFFFFFFFF
        t ^= t >> 15
        x = t >> (32 - LOG2_SLOTS)
    r, p = tm.home_of(np.array([5], np.uint64), k, LOG2_SLOTS)
    assert (int(r[0]), int(p[0])) == (x >> 13, x & 8191)


# ---- the rig: a context, the partner table, device arrays, the stream discipline ------------------------------------------------

@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    return torch


class Rig:
    """own_stream: the context enqueues on a non-blocking stream of its own - torch's work is waited for before a call
    that takes arrays torch made, the context's before torch reads what the call wrote"""

    def __init__(self, torch, P, own_stream):
        from kmertools_amd import device
        self.torch, self.P, self.k, self.own = torch, P, P.k, own_stream
        self.ctx = device.Context(0, stream=None if own_stream else torch.cuda.current_stream().cuda_stream)
        self.made = []
        self.pm = P.partner
        self.partner = self.counter(1 << 16)
        self.partner.add_pairs_host(self.pm.keys, self.pm.counts)
        self.prof_csr = P.csr["profile"]

    def counter(self, slots):
        from kmertools_amd import device
        c = device.Counter(self.ctx, self.k, slots)
        self.made.append(c)
        return c

    def close(self):
        for c in reversed(self.made):  # every counter before its context
            c.close()
        self.ctx.close()

    def before(self):
        if self.own:
            self.torch.cuda.synchronize()

    def after(self):
        if self.own:
            self.ctx.sync()
        else:
            self.torch.cuda.synchronize()

    def full(self, n, value, bits):
        return self.torch.full((n,), value, dtype=self.torch.int64 if bits == 64 else self.torch.int32, device="cuda")

    def dev(self, a):
        a = np.ascontiguousarray(a)
        a = a.view({np.dtype(np.uint64): np.int64, np.dtype(np.uint32): np.int32}.get(a.dtype, a.dtype))
        return self.torch.from_numpy(a if a.size else np.zeros(1, a.dtype)).cuda()


def u64(t):
    return t.cpu().numpy().view(np.uint64)


def u32(t):
    return t.cpu().numpy().view(np.uint32)


def by_key(keys, *rest):
    order = np.argsort(keys, kind="stable")
    return (keys[order],) + tuple(r[order] for r in rest)


def same(a, b):
    return a.dtype == b.dtype and np.array_equal(a, b)


# ---- the readers: each compares one call with the model ---------------------------------------------------------------------------

def r_size(R, c, ref):
    assert c.size() == ref.m.size


def r_export_host(R, c, ref):
    gk, gc = c.export_host()
    assert same(gk, ref.m.keys) and same(gc, ref.m.counts)


def r_export_device(R, c, ref):
    n = ref.m.size
    tk, tc = R.full(n + GUARD, KPAT, 64), R.full(n + GUARD, CPAT, 32)
    R.before()
    got = c.export(tk, tc, n)
    R.after()
    hk, hc = u64(tk), u32(tc)
    assert got == n and (hk[n:] == KPAT).all() and (hc[n:] == CPAT).all()
    gk, gc = by_key(hk[:n], hc[:n])
    assert same(gk, ref.m.keys) and same(gc, ref.m.counts)


def refused(fn, code, tag=""):
    from kmertools_amd._lib import KmertoolsError
    try:
        fn()
    except KmertoolsError as e:
        assert e.code == code, "%s: error %d where %d is due: %s" % (tag, e.code, code, e)
        return
    raise AssertionError("%s: the call returned KT_OK where error %d is due" % (tag, code))


def r_stage_pieces(R, c, ref):
    from kmertools_amd._lib import KT_ERR_ARG
    n = c.export_stage_range(1, None)
    assert n == ref.m.size
    a, b = n // 5, n // 2 + 1 if n else 0
    pieces = [c.export_fetch(b, n - b), c.export_fetch(0, a), c.export_fetch(a, b - a)]  # (in any order)
    gk = np.concatenate([pieces[1][0], pieces[2][0], pieces[0][0]])
    gc = np.concatenate([pieces[1][1], pieces[2][1], pieces[0][1]])
    gk, gc = by_key(gk, gc)
    assert same(gk, ref.m.keys) and same(gc, ref.m.counts)
    refused(lambda: c.export_fetch(n, 1), KT_ERR_ARG)
    refused(lambda: c.export_fetch(0, n + 1), KT_ERR_ARG)


def r_stage_2_5(R, c, ref):
    from kmertools_amd._lib import KT_ERR_ARG
    wk, wc = ref.m.stage(2, 5)
    n = c.export_stage_range(2, 5)
    assert n == len(wk)
    gk, gc = by_key(*c.export_fetch(0, n))
    assert same(gk, wk) and same(gc, wc)
    refused(lambda: c.export_fetch(0, n + 1), KT_ERR_ARG)


def spectrum_want(ref):
    hist, (d, occ) = ref.memo("spectrum", lambda: ref.m.spectrum(N_BINS))
    return np.arange(N_BINS, dtype=np.uint64) + 100 + hist, np.array([7 + d, 9 + occ], np.uint64)


def r_spectrum_host(R, c, ref):
    from kmertools_amd._lib import KT_MEM_HOST
    hist, tot = np.arange(N_BINS, dtype=np.uint64) + 100, np.array([7, 9], np.uint64)
    c.spectrum_into(hist, N_BINS, tot, KT_MEM_HOST)
    wh, wt = spectrum_want(ref)
    assert same(hist, wh) and same(tot, wt)  # (added to what was there; bin 0 left alone)


def r_spectrum_device(R, c, ref):
    hist, tot = R.dev(np.arange(N_BINS, dtype=np.uint64) + 100), R.dev(np.array([7, 9], np.uint64))
    R.before()
    c.spectrum_into(hist, N_BINS, tot)
    R.after()
    wh, wt = spectrum_want(ref)
    assert same(u64(hist), wh) and same(u64(tot), wt)


def lookup_keys(R, ref):
    def make():
        rng = np.random.default_rng(ref.m.size + R.k)
        present = rng.choice(ref.m.keys, min(1000, ref.m.size), replace=False)
        keys = np.concatenate([present, R.P.absent[:2000 - len(present)], R.P.cluster])
        return keys[rng.permutation(len(keys))]
    return ref.memo("lookup_keys", make)


def r_lookup(R, c, ref):
    keys = lookup_keys(R, ref)
    want = ref.m.count(keys)
    dk, out = R.dev(keys), R.full(len(keys) + 1, CPAT, 32)
    R.before()
    c.lookup(dk, len(keys), out)
    R.after()
    got = u32(out)
    assert same(got[:-1], want) and got[-1] == CPAT
    assert same(c.lookup_host(keys), want)


def r_profile(R, c, ref):
    bases, offsets = R.prof_csr
    want = ref.memo("profile", lambda: ref.m.profile(R.P.seqs["profile"]))
    total = int(offsets[-1])
    prof = R.full(total + 1, -1, 32)
    db, do = R.dev(bases), R.dev(offsets)
    R.before()
    c.profile(db, do, len(offsets) - 1, prof)
    R.after()
    got = u32(prof)
    assert same(got[:total], want) and got[total] == NO


def compare_base():
    return np.full((N_ROWS, N_COLS), 3, np.uint64), np.arange(6, dtype=np.uint64) + 11


def r_compare_walked(R, c, ref):
    """compare(t, partner), host mode: t is walked in the form it is in, the partner probed"""
    from kmertools_amd._lib import KT_MEM_HOST
    wm, wt = ref.memo("compare_a", lambda: ref.m.compare(R.pm, N_ROWS, N_COLS))
    m, tot = compare_base()
    c.compare_into(R.partner, m, N_ROWS, N_COLS, tot, KT_MEM_HOST)
    bm, bt = compare_base()
    assert wm[0, 0] == 0 and same(m, bm + wm) and same(tot, bt + wt)


def r_compare_probed(R, c, ref):
    """compare(partner, t), device mode: t is probed"""
    wm, wt = ref.memo("compare_b", lambda: R.pm.compare(ref.m, N_ROWS, N_COLS))
    bm, bt = compare_base()
    m, tot = R.dev(bm.reshape(-1)), R.dev(bt)
    R.before()
    R.partner.compare_into(c, m, N_ROWS, N_COLS, tot)
    R.after()
    assert same(u64(m).reshape(N_ROWS, N_COLS), bm + wm) and same(u64(tot), bt + wt)


def setop_host(R, a, b, ref, name, want):
    wk, wc = ref.memo(name, want)
    gk, gc = a.setop(b, name.split("_")[0], count="sum", sort=True)
    assert same(gk, wk) and same(gc, wc)


def setop_device(R, a, b, ref, name, want):
    wk, wc = ref.memo(name, want)
    room = len(wk) + 2
    keys, counts = R.full(room + 3, KPAT, 64), R.full(room + 3, CPAT, 32)
    R.before()
    n = a.setop_device(b, name.split("_")[0], keys, counts, room, count="sum", sort=True)
    R.after()
    hk, hc = u64(keys), u32(counts)
    assert n == len(wk) and (hk[n:] == KPAT).all() and (hc[n:] == CPAT).all()
    assert same(hk[:n], wk) and same(hc[:n], wc)


def r_intersect_as_a(R, c, ref):
    setop_host(R, c, R.partner, ref, "intersect_a", lambda: ref.m.setop(R.pm, "intersect", "sum"))


def r_intersect_as_b(R, c, ref):
    setop_device(R, R.partner, c, ref, "intersect_b", lambda: R.pm.setop(ref.m, "intersect", "sum"))


def r_xor_as_a(R, c, ref):
    setop_host(R, c, R.partner, ref, "xor_a", lambda: ref.m.setop(R.pm, "xor", "sum"))


def r_xor_as_b(R, c, ref):
    setop_device(R, R.partner, c, ref, "xor_b", lambda: R.pm.setop(ref.m, "xor", "sum"))


def graph_reader(lo):
    def r_graph(R, c, ref):
        wk, wi, wc, wcen = ref.memo("graph%d" % lo, lambda: ref.m.graph(lo, None))
        room = len(wk) + 2
        keys, info, counts = R.full(room + 3, KPAT, 64), R.full(room + 3, IPAT, 32), R.full(room + 3, CPAT, 32)
        cen = R.dev(np.arange(32, dtype=np.uint64) + 50)
        R.before()
        n = c.graph_device(keys, info, counts, room, lo, None, sort=True, census=cen)
        R.after()
        hk, hi, hc = u64(keys), u32(info), u32(counts)
        assert n == len(wk) and (hk[n:] == KPAT).all() and (hi[n:] == IPAT).all() and (hc[n:] == CPAT).all()
        assert same(hk[:n], wk) and same(hi[:n], wi) and same(hc[:n], wc)
        assert same(u64(cen), np.arange(32, dtype=np.uint64) + 50 + wcen)
    return r_graph


READERS = {
    "size": r_size, "export_host": r_export_host, "export_device": r_export_device, "stage_pieces": r_stage_pieces,
    "stage_2_5": r_stage_2_5, "spectrum_host": r_spectrum_host, "spectrum_device": r_spectrum_device,
    "compare(t, partner)": r_compare_walked, "intersect(t, partner)": r_intersect_as_a,
    "lookup": r_lookup, "profile": r_profile, "compare(partner, t)": r_compare_probed,
    "intersect(partner, t)": r_intersect_as_b, "xor(t, partner)": r_xor_as_a, "xor(partner, t)": r_xor_as_b,
    "graph(1)": graph_reader(1), "graph(2)": graph_reader(2),
}
# never need the probing image: the table is read in the form it is in
WALKERS = ("size", "export_host", "export_device", "stage_pieces", "stage_2_5", "spectrum_host", "spectrum_device",
           "compare(t, partner)", "intersect(t, partner)")
# need it: a dense table, or one held in an export target, is turned into it (xor walks both tables and probes both)
PROBERS = ("lookup", "profile", "compare(partner, t)", "intersect(partner, t)", "xor(t, partner)", "xor(partner, t)",
           "graph(1)", "graph(2)")
assert set(WALKERS) | set(PROBERS) == set(READERS)


def read(R, c, ref, name, tag):
    """one reader against the model; the call left the content as it was: the size and the sorted export"""
    try:
        READERS[name](R, c, ref)
        assert c.size() == ref.m.size, "the size afterwards"
        gk, gc = c.export_host()
        assert same(gk, ref.m.keys) and same(gc, ref.m.counts), "the content afterwards"
    except Exception as e:  # noqa: BLE001 (an error code of the library is a finding like a mismatch)
        raise AssertionError("%s: reader %s: %s: %s" % (tag, name, type(e).__name__, e)) from e


def check_all(R, c, ref, order, tag, only=None):
    names = WALKERS + PROBERS if order == "walkers_first" else PROBERS + WALKERS
    for name in names:
        if only is None or name in only:
            read(R, c, ref, name, tag)


def check_all_full(R, t, tag):
    """an overflowed table: every reader is KT_ERR_FULL and leaves its outputs - the accumulating ones too - as they were"""
    from kmertools_amd._lib import KT_ERR_FULL, KT_MEM_HOST
    torch = R.torch
    bases, offsets = R.prof_csr
    total = int(offsets[-1])
    hk, hc, hh, ht = np.full(16, KPAT, np.uint64), np.full(16, CPAT, np.uint32), np.full(N_BINS, 77, np.uint64), np.full(2, 78, np.uint64)
    hm, h6 = np.full((N_ROWS, N_COLS), 79, np.uint64), np.full(6, 80, np.uint64)
    dk, di, dc = R.full(64, KPAT, 64), R.full(64, IPAT, 32), R.full(max(64, total + 1), CPAT, 32)
    dh, dt, dm, d6, dcen = R.full(N_BINS, 77, 64), R.full(2, 78, 64), R.full(N_ROWS * N_COLS, 79, 64), R.full(6, 80, 64), R.full(32, 81, 64)
    lk = R.dev(R.P.absent[:32])
    db, do = R.dev(bases), R.dev(offsets)
    R.before()
    calls = {
        "size": lambda: t.size(),
        "export host": lambda: t.export(hk, hc, 16, KT_MEM_HOST),
        "export device": lambda: t.export(dk, dc, 16),
        "stage": lambda: t.export_stage_range(1, None),
        "stage 2..5": lambda: t.export_stage_range(2, 5),
        "spectrum host": lambda: t.spectrum_into(hh, N_BINS, ht, KT_MEM_HOST),
        "spectrum device": lambda: t.spectrum_into(dh, N_BINS, dt),
        "lookup": lambda: t.lookup(lk, 32, dc),
        "profile": lambda: t.profile(db, do, len(offsets) - 1, dc),
        "compare(t, partner)": lambda: t.compare_into(R.partner, hm, N_ROWS, N_COLS, h6, KT_MEM_HOST),
        "compare(partner, t)": lambda: R.partner.compare_into(t, dm, N_ROWS, N_COLS, d6),
        "intersect(t, partner)": lambda: t.setop_device(R.partner, "intersect", dk, dc, 64, count="sum"),
        "intersect(partner, t)": lambda: R.partner.setop_device(t, "intersect", dk, dc, 64, count="sum"),
        "xor(t, partner)": lambda: t.setop_device(R.partner, "xor", dk, dc, 64, count="sum"),
        "xor(partner, t)": lambda: R.partner.setop_device(t, "xor", dk, dc, 64, count="sum"),
        "graph(1)": lambda: t.graph_device(dk, di, dc, 64, 1, None, census=dcen),
        "graph(2)": lambda: t.graph_device(dk, di, dc, 64, 2, None, census=dcen),
    }
    for name, fn in calls.items():
        refused(fn, KT_ERR_FULL, "%s: reader %s of an overflowed table" % (tag, name))
    refused(lambda: t.export_fetch(0, 1), 1, tag)  # (KT_ERR_ARG: nothing was staged)
    R.after()
    torch.cuda.synchronize()
    assert (hk == KPAT).all() and (hc == CPAT).all() and (hh == 77).all() and (ht == 78).all() and (hm == 79).all() and (h6 == 80).all(), tag
    for tns, v in ((dk, KPAT), (di, IPAT), (dc, CPAT), (dh, 77), (dt, 78), (dm, 79), (d6, 80), (dcen, 81)):
        assert bool((tns == v).all()), (tag, v)


# ---- the transitions ----------------------------------------------------------------------------------------------------------------

def env_probing(mp):
    mp.setenv("KT_BULK", "0")


def env_bulk(mp):
    mp.setenv("KT_BULK", "1")
    mp.setenv("KT_BULK_MIN_BASES", "0")
    mp.setenv("KT_BULK_MERGE_DIV", "1000000000")  # a batch of any size is worth a rebuild of the ranges
    mp.setenv("KT_BULK_VERBOSE", "1")


def add_device(R, c, name):
    bases, offsets = R.P.csr[name]
    db, do = R.dev(bases), R.dev(offsets)
    R.before()
    c.add_reads(db, do, len(offsets) - 1)
    R.after()


def bulk_lines(capfd):
    return [line for line in capfd.readouterr().err.splitlines() if line.startswith("[bulk]")]


def fetch_or_refuse(c, ref, n, tag):
    """after something that may have ended the stage: export_fetch hands out the table's entries or refuses"""
    from kmertools_amd._lib import KT_ERR_ARG, KmertoolsError
    try:
        gk, gc = c.export_fetch(0, n)
    except KmertoolsError as e:
        assert e.code == KT_ERR_ARG, (tag, e)
        return "refused"
    gk, gc = by_key(gk, gc)
    assert same(gk, ref.m.keys) and same(gc, ref.m.counts), \
        "%s: export_fetch returned KT_OK and %d entries that are not the table's (first key %#x)" % (tag, n, int(gk[0]))
    return "entries"


# ---- the scripted life -----------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("own_stream", [False, True], ids=["torch_stream", "own_stream"])
@pytest.mark.parametrize("order", ["walkers_first", "probers_first"])
@pytest.mark.parametrize("k", [15, 31])
def test_one_table_through_its_whole_life(torch_mod, oracle, monkeypatch, capfd, k, order, own_stream):
    from kmertools_amd._lib import KT_ERR_ARG
    torch = torch_mod
    P = plan(k)
    R = Rig(torch, P, own_stream)
    S = P.step
    try:
        c = R.counter(SLOTS)
        assert c.capacity() == SLOTS
        tag = lambda n: "k=%d %s step %d" % (k, order, n)  # noqa: E731

        # 1. freshly created, never written
        check_all(R, c, S[1], order, tag(1))
        # 2. a small probing add
        env_probing(monkeypatch)
        c.add_reads_host(*P.csr["small2"])
        check_all(R, c, S[2], order, tag(2))
        # 3. 3 000 pairs with counts 1..9, half of their keys present; 24 of the new ones collide at a range's last slot
        c.add_pairs_host(*P.pairs3)
        check_all(R, c, S[3], order, tag(3))
        # 4. clear: empty while the clear is still pending - for every reader: whichever reader carried the clear out, the
        # next one finds stale entries under a pending clear again
        c.clear()
        refused(lambda: c.export_fetch(0, 1), KT_ERR_ARG, tag(4) + ": export_fetch after clear")
        for name in (WALKERS + PROBERS if order == "walkers_first" else PROBERS + WALKERS):
            read(R, c, S[4], name, tag(4))
            c.add_pairs_host(P.pairs3[0][:300], P.pairs3[1][:300])
            assert c.size() > 0
            c.clear()
        check_all(R, c, S[4], order, tag(4))
        # 5. a small probing add of another genome's reads: nothing of steps 2 and 3 is left
        c.clear()  # (a second clear on top of a pending or done one changes nothing)
        c.add_reads_host(*P.csr["small5"])
        assert not c.lookup_host(P.gone_at_5[::7]).any(), tag(5)
        check_all(R, c, S[5], order, tag(5))
        # 6. clear, then a fresh bulk build: dense ranges (the walkers see them when they come first)
        env_bulk(monkeypatch)
        c.clear()
        capfd.readouterr()
        add_device(R, c, "bulk1")
        lines = bulk_lines(capfd)
        assert len(lines) == 1 and lines[0].split()[5] == "build", (tag(6), lines)  # (k, keys, level1, level2, build | merge, ...)
        check_all(R, c, S[6], order, tag(6))
        # 7. a second batch merged in place by the bulk path
        add_device(R, c, "bulk2")
        lines = bulk_lines(capfd)
        assert len(lines) == 1 and lines[0].split()[5] == "merge", (tag(7), lines)
        check_all(R, c, S[7], order, tag(7))
        # 8. a small batch by the probing path on top of the rebuilt ranges
        env_probing(monkeypatch)
        c.add_reads_host(*P.csr["small8"])
        assert bulk_lines(capfd) == [], tag(8)
        check_all(R, c, S[8], order, tag(8))
        # 9. counted into an export target, read without imaging: the walkers only
        m = P.target_room
        xk, xc = R.full(m, KPAT, 64), R.full(m, CPAT, 32)
        env_bulk(monkeypatch)
        R.before()
        c.export_target(xk, xc, m)
        c.clear()
        add_device(R, c, "bulk2")
        lines = bulk_lines(capfd)
        assert len(lines) == 1 and lines[0].split()[5] == "build", (tag(9), lines)  # (no "redone into the table" line)
        check_all(R, c, S[9], order, tag(9), only=WALKERS)
        R.after()
        n = S[9].m.size
        hk, hc = u64(xk), u32(xc)
        assert same(np.sort(hk[:n]), S[9].m.keys) and (hk[n:] == KPAT).all() and (hc[n:] == CPAT).all(), tag(9)
        gk, gc = by_key(hk[:n], hc[:n])
        assert same(gc, S[9].m.counts), tag(9)
        # 10. staged from the target, imaged by a prober, the target overwritten by its owner
        assert c.export_stage_range(1, None) == n
        read(R, c, S[10], "lookup", tag(10))
        xk.fill_(KPAT2)
        xc.fill_(CPAT2)
        torch.cuda.synchronize()
        fetch_or_refuse(c, S[10], n, tag(10))
        check_all(R, c, S[10], order, tag(10))
        R.after()
        torch.cuda.synchronize()
        assert bool((xk == KPAT2).all()) and bool((xc == CPAT2).all()), "%s: the library wrote to arrays it had given back" % tag(10)
        # 11. a probing add on top: the stage is gone until staged again
        env_probing(monkeypatch)
        assert c.export_stage_range(1, None) == n
        c.add_reads_host(*P.csr["small11"])
        refused(lambda: c.export_fetch(0, 1), KT_ERR_ARG, tag(11) + ": export_fetch after an add")
        check_all(R, c, S[11], order, tag(11))
        # 12. clear with the target still set, another batch built into the same arrays
        env_bulk(monkeypatch)
        c.clear()
        capfd.readouterr()
        add_device(R, c, "bulk1")
        lines = bulk_lines(capfd)
        assert len(lines) == 1 and lines[0].split()[5] == "build", (tag(12), lines)
        n = S[12].m.size
        hk, hc = by_key(u64(xk)[:n], u32(xc)[:n])  # (what the arrays hold beyond the entries is unspecified)
        assert same(hk, S[12].m.keys) and same(hc, S[12].m.counts), tag(12)
        assert not np.isin(P.only_bulk2, hk).any(), tag(12)
        check_all(R, c, S[12], order, tag(12), only=WALKERS)
        assert not c.lookup_host(P.only_bulk2).any(), tag(12)
        check_all(R, c, S[12], order, tag(12))
        # 13. the target switched off while the entries are in it: the table takes its own copy first
        c.clear()
        add_device(R, c, "bulk1")
        assert same(np.sort(u64(xk)[:n]), S[13].m.keys), tag(13)
        c.export_target(None, None, 0)
        xk.fill_(KPAT2)
        xc.fill_(CPAT2)
        torch.cuda.synchronize()
        check_all(R, c, S[13], order, tag(13))
        R.after()
        torch.cuda.synchronize()
        assert bool((xk == KPAT2).all()) and bool((xc == CPAT2).all()), tag(13)
        # 14. a second table overflows, is cleared and used again: the flag does not survive the clear
        env_probing(monkeypatch)
        t = R.counter(1024)
        t.add_pairs_host(np.arange(1, 5000, dtype=np.uint64) * 7919, np.ones(4999, np.uint32))
        check_all_full(R, t, tag(14))
        t.clear()
        t.add_reads_host(*P.csr["tiny"])
        check_all(R, t, S[14], order, tag(14))
        # ... and the first table is what it was
        read(R, c, S[13], "export_host", tag(14))
    finally:
        R.close()


# ---- a seeded random walk over the same transitions ----------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("seed", [11, 23, 47])
@pytest.mark.parametrize("k", [15, 31])
def test_random_walk_over_the_transitions(torch_mod, oracle, monkeypatch, k, seed):
    """40 steps, each one transition (probing add, bulk add, add_pairs, clear, set target, drop target) or two to four
    readers in random order.  No overflow and no target that is too small are drawn: every batch of the pool lies inside
    the key set plan() measured, and a target has room for all of it."""
    torch = torch_mod
    P = plan(k)
    rng = np.random.default_rng(seed * 100 + k)
    R = Rig(torch, P, own_stream=seed == 23)
    taken = []
    try:
        c = R.counter(SLOTS)
        room = P.walk_room
        targets = [(R.full(room, KPAT, 64), R.full(room, CPAT, 32)) for _ in range(2)]
        model = tm.Model(k)
        ref = Ref(model)
        pk, pc = P.pairs3
        for step in range(40):
            if rng.random() < 0.5:
                kind = str(rng.choice(["probing add", "bulk add", "add_pairs", "clear", "set target", "drop target"],
                                      p=[0.22, 0.26, 0.12, 0.18, 0.14, 0.08]))
                if kind == "probing add":
                    name = str(rng.choice(["small2", "small5", "small8", "small11"]))
                    taken.append("%s %s" % (kind, name))
                    env_probing(monkeypatch)
                    c.add_reads_host(*P.csr[name])
                    model.add_reads(*P.csr[name])
                elif kind == "bulk add":
                    name = str(rng.choice(["bulk1", "bulk2"]))
                    taken.append("%s %s" % (kind, name))
                    env_bulk(monkeypatch)
                    monkeypatch.setenv("KT_BULK_VERBOSE", "0")
                    add_device(R, c, name)
                    model.add_reads(*P.csr[name])
                elif kind == "add_pairs":
                    lo = int(rng.integers(0, 2000))
                    taken.append("%s pairs3[%d:%d]" % (kind, lo, lo + 1000))
                    c.add_pairs_host(pk[lo:lo + 1000], pc[lo:lo + 1000])
                    model.add_pairs(pk[lo:lo + 1000], pc[lo:lo + 1000])
                elif kind == "clear":
                    taken.append(kind)
                    c.clear()
                    model.clear()
                elif kind == "set target":
                    i = int(rng.integers(0, 2))
                    taken.append("%s %d" % (kind, i))
                    R.before()
                    c.export_target(targets[i][0], targets[i][1], room)
                else:
                    taken.append(kind)
                    c.export_target(None, None, 0)
                ref = Ref(model)
            else:
                names = [str(n) for n in rng.choice(sorted(READERS), size=int(rng.integers(2, 5)), replace=False)]
                for name in names:
                    taken.append(name)
                    read(R, c, ref, name, "k=%d seed=%d" % (k, seed))
        taken.append("every reader")
        check_all(R, c, ref, "walkers_first", "k=%d seed=%d" % (k, seed))
    except Exception as e:  # noqa: BLE001
        raise AssertionError("%s\nafter the steps: %s" % (e, "; ".join(taken))) from e
    finally:
        R.close()
