"""The maximal unitigs of a table: kt_ctr_unitigs against the string-level reference of tests/unitig_ref.py (which
test_ctr_unitigs_cli_args.py pins, on the CPU, to worked answers and to its own invariants) - the worked answers, every k
that takes another path, count ranges, a lattice of unitig lengths around every wave, workgroup and scan-tile edge, one
path and one cycle longer than any tile, every table form, the shapes and argument errors of the call, device outputs
between guards with exactly the room needed; and `kmertools unitigs` end to end, byte for byte against the reference's
files.  Every comparison is exact."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "kmertools_amd", "bin", "kmertools")
GOLDEN = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, os.path.join(ROOT, "tests"))
import graph_ref as gr  # noqa: E402
import unitig_ref as ur  # noqa: E402

U32 = 0xFFFFFFFF
RANGES = ((1, None), (2, None), (1, 1), (2, 3))
GUARD = 64
BG, OG, SG, FG = 0x7E, 0x6D6D6D6D6D6D6D6D, 0x5C5C5C5C5C5C5C5C, 0x4B4B4B4B


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


def noisy_reads(seed, n, k, genome_len=12000):
    """reads sampled from a small genome with substitutions, runs of N, lower-case stretches, some shorter than k, some
    repeated (test_ctr_graph.py's, with the repeats scaled to n)"""
    rng = np.random.default_rng(seed)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    genome = acgt[rng.integers(0, 4, size=genome_len)]
    out = []
    for i in range(n):
        L = int(rng.integers(0, k)) if i % 25 == 0 else int(rng.integers(40, 200))
        a = int(rng.integers(0, len(genome) - L))
        s = genome[a:a + L].copy()
        err = rng.random(L) < 0.01
        s[err] = acgt[rng.integers(0, 4, size=int(err.sum()))]
        if L > 50 and rng.random() < 0.15:
            p = int(rng.integers(0, L - 6))
            s[p:p + int(rng.integers(1, 6))] = ord("N")
        if L > 50 and rng.random() < 0.15:
            p = int(rng.integers(0, L - 20))
            s[p:p + 20] = np.frombuffer(bytes(s[p:p + 20]).lower(), np.uint8)
        out.append(s.tobytes())
    return out + out[:40] * 2 + out[n // 2:n // 2 + 20] * 5


def sample(seed, k, n=400, genome_len=4000):
    from kmertools_amd.device import to_csr
    return to_csr(noisy_reads(seed, n, k, genome_len))


def sorted_table(keys, counts):
    order = np.argsort(keys)
    return np.asarray(keys, np.uint64)[order], np.asarray(counts, np.uint32)[order]


def strings_table(tk, tc, k):
    return {gr.str_of(key, k): int(c) for key, c in zip(tk.tolist(), tc.tolist())}


def counter_of(ctx, k, bases, offsets, n_keys):
    from kmertools_amd import device
    c = device.Counter(ctx, k, max(1 << 16, 2 * n_keys))
    c.add_reads_host(bases, offsets)
    return c


def pairs_counter(ctx, k, keys, counts, slots=1 << 16):
    from kmertools_amd import device
    c = device.Counter(ctx, k, slots)
    if len(keys):
        c.add_pairs_host(np.asarray(keys, np.uint64), np.asarray(counts, np.uint32))
    return c


def as_arrays(us):
    """the reference's [(string, count_sum, flags, nodes)] as the call's four arrays"""
    bases = np.frombuffer("".join(s for s, _, _, _ in us).encode(), np.uint8)
    offsets = np.zeros(len(us) + 1, np.uint64)
    offsets[1:] = np.cumsum([len(s) for s, _, _, _ in us], dtype=np.uint64)
    return (bases, offsets, np.array([c for _, c, _, _ in us], np.uint64).reshape(-1),
            np.array([f for _, _, f, _ in us], np.uint32).reshape(-1))


def same(got, want):
    return all(g.dtype == w.dtype and np.array_equal(g, w) for g, w in zip(got, want)) and len(got) == len(want) == 4


def first_difference(got, want):
    for name, g, w in zip(("bases", "offsets", "count_sums", "flags"), got, want):
        if len(g) != len(w):
            return "%s: %d entries, want %d" % (name, len(g), len(w))
        bad = np.flatnonzero(g != w)
        if len(bad):
            return "%s[%d] = %r, want %r (%d differ)" % (name, bad[0], g[bad[0]], w[bad[0]], len(bad))
    return None


def unitigs_dev(torch, c, lo, hi, nu, nb, sums=True, flags=True):
    """device mode into views of exactly the room needed, GUARD elements of a pattern on either side of each"""
    db = torch.full((GUARD + nb + GUARD,), BG, dtype=torch.uint8, device="cuda")
    do = torch.from_numpy(np.full(GUARD + nu + 1 + GUARD, OG, np.uint64).view(np.int64)).cuda()
    ds = torch.from_numpy(np.full(GUARD + nu + GUARD, SG, np.uint64).view(np.int64)).cuda()
    df = torch.from_numpy(np.full(GUARD + nu + GUARD, FG, np.uint32).view(np.int32)).cuda()
    got = c.unitigs_device(db[GUARD:GUARD + nb], nb, do[GUARD:GUARD + nu + 1], ds[GUARD:GUARD + nu] if sums else None,
                           df[GUARD:GUARD + nu] if flags else None, nu, lo, hi)
    torch.cuda.synchronize()
    assert got == (nu, nb), (got, nu, nb)
    hb, ho = db.cpu().numpy(), do.cpu().numpy().view(np.uint64)
    hs, hf = ds.cpu().numpy().view(np.uint64), df.cpu().numpy().view(np.uint32)
    for h, g, n in ((hb, BG, nb), (ho, OG, nu + 1), (hs, SG, nu if sums else 0), (hf, FG, nu if flags else 0)):
        assert (h[:GUARD] == g).all() and (h[GUARD + n:] == g).all(), "a guard was written"
    if nu == 0 and nb == 0:  # no room at all is the count-only call: not even offsets[0] is written
        assert ho[GUARD] == OG
        ho = ho.copy()
        ho[GUARD] = 0
    return hb[GUARD:GUARD + nb], ho[GUARD:GUARD + nu + 1], hs[GUARD:GUARD + nu], hf[GUARD:GUARD + nu]


def check_both_modes(torch, c, want, lo=1, hi=None, tag=None):
    got = c.unitigs(lo, hi)
    assert same(got, want), (tag, "host", first_difference(got, want))
    got = unitigs_dev(torch, c, lo, hi, len(want[2]), len(want[0]))
    assert same(got, want), (tag, "device", first_difference(got, want))


def snapshot(ctr):
    return ctr.size(), ctr.export_host()


# ---- 1. worked answers ----------------------------------------------------------------------------------------------------

KNOWN = json.load(open(os.path.join(GOLDEN, "unitig_known.json")))["cases"]


@pytest.mark.parametrize("case", KNOWN, ids=lambda c: "k%d_%s" % (c["k"], "+".join(c["reads"])[:24]))
def test_unitigs_known_answers(torch_mod, ctx, case):
    k = case["k"]
    table = gr.count_strings(case["reads"], k)
    us = ur.unitigs(table, k)
    assert [[s, c, f] for s, c, f, _ in us] == case["unitigs"]  # the input's shape: the reference gives the worked answer
    tk, tc = sorted_table([gr.key_of(s) for s in table], list(table.values()))
    c = pairs_counter(ctx, k, tk, tc)
    try:
        bases, offsets, sums, flags = c.unitigs()
        text = bases.tobytes().decode()
        got = [[text[int(offsets[i]):int(offsets[i + 1])], int(sums[i]), int(flags[i])] for i in range(len(sums))]
        assert got == case["unitigs"]
        check_both_modes(torch_mod, c, as_arrays(us))
    finally:
        c.close()


# ---- 2. every k that takes another path, count ranges; 7. the cross-checks against kt_ctr_graph --------------------------

def check_ranges(torch, c, tk, tc, k, tag):
    table = strings_table(tk, tc, k)
    sizes = set()
    for lo, hi in RANGES:
        us = ur.unitigs(table, k, lo, U32 if hi is None else hi)
        want = as_arrays(us)
        check_both_modes(torch, c, want, lo, hi, (tag, k, lo, hi))
        # against kt_ctr_graph's census of the same range
        cen = c.graph(lo, hi, census=True)[3]
        assert len(want[0]) == int(cen[0]) + len(us) * (k - 1) and int(want[2].sum()) == int(cen[1]), (tag, k, lo, hi)
        sizes.add((len(us), len(want[0])))
    return sizes


@pytest.mark.parametrize("k", [1, 2, 4, 10, 15, 16, 17, 30, 31])
def test_unitigs_k_sweep(torch_mod, ctx, oracle, k):
    bases, offsets = sample(300 + k, k)
    tk, tc = sorted_table(*oracle.count_reads(bases, offsets, k))
    cen = gr.restate(tk, tc, k)[3]
    if k >= 10:  # the sample is a graph worth the name: unitig interiors, tips, branches
        assert cen[7 + 5 + 1] > 0 and cen[5] > 0 and cen[6] > 0 and len(tk) > 3000
    c = counter_of(ctx, k, bases, offsets, len(tk))
    try:
        snap = snapshot(c)
        sizes = check_ranges(torch_mod, c, tk, tc, k, "sweep")
        if k >= 10:
            assert len(sizes) == len(RANGES)
        n2, (k2, c2) = snapshot(c)
        assert n2 == snap[0] and np.array_equal(k2, tk) and np.array_equal(c2, tc)
    finally:
        c.close()


@pytest.mark.parametrize("k", [5, 6])
def test_unitigs_small_k_through_add_pairs(torch_mod, ctx, k):
    """tables of a few dozen nodes with cycles, palindromes (k = 6), hairpins (k = 5) and self-links among them"""
    rng = np.random.default_rng(500 + k)
    kinds = dict(circular=0, palindrome=0, n=0)
    for trial in range(6):
        g = "".join(rng.choice(list("ACGT"), size=int(rng.integers(20, 90))))
        cyc = "".join(rng.choice(list("ACGT"), size=int(rng.integers(3, 30))))
        reads = [g, gr.rc_s(g[5:40]), g[3:30], cyc * 3 + cyc[:k - 1], "A" * (k + 3), ("AT" * k)[:k + 3], ("ACGT" * k)[:k + 5],
                 g[:k] + gr.rc_s(g[:k])]
        table = gr.count_strings(reads, k)
        tk, tc = sorted_table([gr.key_of(s) for s in table], list(table.values()))
        us = ur.unitigs(table, k)
        kinds["circular"] += sum(1 for _, _, f, _ in us if f)
        kinds["palindrome"] += sum(1 for s in table if gr.rc_s(s) == s)
        kinds["n"] += len(table)
        c = pairs_counter(ctx, k, tk, tc)
        try:
            check_ranges(torch_mod, c, tk, tc, k, ("pairs", trial))
        finally:
            c.close()
    assert kinds["circular"] and kinds["n"] > 200 and (kinds["palindrome"] > 0) == (k % 2 == 0), kinds


# ---- 3. the length lattice ------------------------------------------------------------------------------------------------

def codes_of(seq):
    return (np.frombuffer(seq, np.uint8) >> 1 & 3) ^ (np.frombuffer(seq, np.uint8) >> 2 & 1)  # A C G T -> 0 1 2 3


def kmer_words(seq, k):
    """the 2-bit words of every window of k bases of an ACGT byte string"""
    code = codes_of(seq).astype(np.uint64)
    n = len(seq) - k + 1
    w = np.zeros(n, np.uint64)
    for j in range(k):
        w = (w << np.uint64(2)) | code[j:j + n]
    return w


def rc_bytes(seq):
    return seq.translate(bytes.maketrans(b"ACGT", b"TGCA"))[::-1]


def test_codes_of_is_acgt():
    assert codes_of(b"ACGT").tolist() == [0, 1, 2, 3]
    assert kmer_words(b"ACGTA", 4).tolist() == [gr.key_of("ACGT"), gr.key_of("CGTA")]


LATTICE = list(range(1, 131)) + [255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 4095, 4096, 4097]


def test_unitigs_length_lattice(torch_mod, ctx, oracle):
    """one independent random sequence per n: n nodes, one unitig each - the sequence or its reverse complement by the start
    rule, in start-key order.  The sequences' nodes interleave in key order, so every wave, workgroup and scan-tile edge of
    the node array lies inside some unitig and between two others."""
    from kmertools_amd.device import to_csr
    k = 31
    rng = np.random.default_rng(3131)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    seqs = [acgt[rng.integers(0, 4, size=n + k - 1)].tobytes() for n in LATTICE]
    bases, offsets = to_csr(seqs)
    tk, tc = sorted_table(*oracle.count_reads(bases, offsets, k))
    cen = gr.restate(tk, tc, k)[3]
    nodes = sum(LATTICE)
    # the shape: every window its own node, nothing branches, two end sides a sequence, every other side joined
    assert 26000 < nodes == len(tk) == cen[0] and cen[6] == 0 and cen[3] == 2 * len(seqs) and cen[2] == 2 * (nodes - len(seqs))
    want = []
    for s, n in zip(seqs, LATTICE):
        w = kmer_words(s, k)
        can = np.minimum(w, gr.rc_np(w, k))
        assert not (n > 1 and can[0] == can[-1])
        fwd = can[0] < can[-1] if n > 1 else w[0] == can[0]
        want.append((int(min(can[0], can[-1])), (s if fwd else rc_bytes(s)).decode(), n, 0, n))
    want = as_arrays([u[1:] for u in sorted(want)])
    c = counter_of(ctx, k, bases, offsets, len(tk))
    try:
        check_both_modes(torch_mod, c, want, tag="lattice")
    finally:
        c.close()


# ---- 4. one path and one cycle longer than any tile -----------------------------------------------------------------------

@pytest.mark.parametrize("shape", ["path", "cycle"])
def test_unitigs_one_long_unitig(torch_mod, ctx, oracle, shape):
    """70 000 nodes in one path, 40 000 in one cycle: more doubling rounds than any tile holds nodes.  The expected answer is
    written down from the construction: the genome or its reverse complement from the smaller end; the circular genome,
    on the strand and from the place of its smallest canonical k-mer, once around and k - 1 bases on."""
    from kmertools_amd.device import to_csr
    k = 31
    rng = np.random.default_rng(70031 if shape == "path" else 40031)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    if shape == "path":
        N = 70000
        G = acgt[rng.integers(0, 4, size=N + k - 1)].tobytes()
        read = G
    else:
        N = 40000
        G = acgt[rng.integers(0, 4, size=N)].tobytes()
        read = G + G[:k - 1]
    bases, offsets = to_csr([read])
    tk, tc = sorted_table(*oracle.count_reads(bases, offsets, k))
    cen = gr.restate(tk, tc, k)[3]
    assert len(tk) == N == cen[0] and cen[6] == 0 and cen[3] == (2 if shape == "path" else 0) and (tc == 1).all()
    w = kmer_words(read, k)
    can = np.minimum(w, gr.rc_np(w, k))
    if shape == "path":
        text = G if can[0] < can[-1] else rc_bytes(G)
        flags = 0
    else:
        j = int(np.argmin(can))
        if w[j] == can[j]:
            text = (G + G)[j:j + N] + (G + G)[j + N:j + N + k - 1]
        else:  # the smallest node reads on the other strand: window j there starts k bases before the mirror of j
            R = rc_bytes(G)
            j2 = (N - j - k) % N
            text = (R + R + R)[j2:j2 + N + k - 1]
        assert kmer_words(text[:k], k)[0] == can[j] and text[-(k - 1):] == text[:k - 1]
        flags = ur.CIRCULAR
    assert len(text) == N + k - 1
    want = as_arrays([(text.decode(), N, flags, N)])
    c = counter_of(ctx, k, bases, offsets, len(tk))
    try:
        check_both_modes(torch_mod, c, want, tag=shape)
    finally:
        c.close()


# ---- 5. every table form before the call ----------------------------------------------------------------------------------

FORMS = ("probing", "add_pairs", "bulk", "export target")


def table_in_form(torch, ctx, form, k, bases, offsets, tk, tc, cap, monkeypatch):
    from kmertools_amd import device
    monkeypatch.delenv("KT_BULK", raising=False)
    monkeypatch.delenv("KT_BULK_MIN_BASES", raising=False)
    if form in ("bulk", "export target"):
        monkeypatch.setenv("KT_BULK", "1")
        monkeypatch.setenv("KT_BULK_MIN_BASES", "0")
    c = device.Counter(ctx, k, cap)
    target = None
    if form == "add_pairs":
        c.add_pairs_host(tk, tc)
    elif form == "export target":
        m = len(tk) + 9
        xk = torch.full((m,), 0x1D1D1D1D1D1D1D1D, dtype=torch.int64, device="cuda")
        xc = torch.full((m,), 0x2E2E2E2E, dtype=torch.int32, device="cuda")
        c.export_target(xk, xc, m)
        c.add_reads(torch.from_numpy(bases).cuda(), torch.from_numpy(offsets.astype(np.int64)).cuda(), len(offsets) - 1)
        torch.cuda.synchronize()
        target = (xk, xc)
    else:
        c.add_reads_host(bases, offsets)
    monkeypatch.delenv("KT_BULK", raising=False)
    monkeypatch.delenv("KT_BULK_MIN_BASES", raising=False)
    return c, target


@pytest.mark.parametrize("size", ["one range", "many ranges"])
def test_unitigs_every_table_form(torch_mod, ctx, oracle, monkeypatch, size):
    torch = torch_mod
    k = 13
    if size == "one range":  # a table below 8192 slots is a single range
        bases, offsets = sample(513, k, n=24, genome_len=12000)
        cap = 4096
    else:
        bases, offsets = sample(2013, k, n=1600, genome_len=12000)
        cap = 1 << 17
    tk, tc = sorted_table(*oracle.count_reads(bases, offsets, k))
    assert (len(tk) < 3000) if size == "one range" else (len(tk) > 10000)
    lo, hi = 1, 6
    us = ur.unitigs(strings_table(tk, tc, k), k, lo, hi)
    want = as_arrays(us)
    assert 1 < len(us) < sum(n for _, _, _, n in us) < len(tk)
    for form in FORMS:
        for mode in ("host", "device"):
            c, target = table_in_form(torch, ctx, form, k, bases, offsets, tk, tc, cap, monkeypatch)
            try:
                assert c.capacity() < 8192 if size == "one range" else c.capacity() >= 4 * 8192
                before = tuple(t.clone() for t in target) if target else None
                got = c.unitigs(lo, hi) if mode == "host" else unitigs_dev(torch, c, lo, hi, len(us), len(want[0]))
                assert same(got, want), (form, mode, first_difference(got, want))
                n, (ek, ec) = snapshot(c)  # the table's content did not change
                assert n == len(tk) and np.array_equal(ek, tk) and np.array_equal(ec, tc), (form, mode)
                if target:
                    torch.cuda.synchronize()
                    assert torch.equal(before[0], target[0]) and torch.equal(before[1], target[1]), (form, mode)
            finally:
                c.close()


# ---- 6. shapes and errors ------------------------------------------------------------------------------------------------

def raw(L, t, lo=1, hi=U32, bases=None, max_bases=0, offsets=None, sums=None, flags=None, max_unitigs=0, nu=None, nb=None, mem=0):
    ptr = lambda x: None if x is None else (x.ctypes.data if isinstance(x, np.ndarray) else x.data_ptr())
    return L.kt_ctr_unitigs(t, lo, hi, ptr(bases), max_bases, ptr(offsets), ptr(sums), ptr(flags), max_unitigs,
                            None if nu is None else C.byref(nu), None if nb is None else C.byref(nb), mem)


def host_buffers(nu, nb, extra=2):
    return (np.full(nb + extra, BG, np.uint8), np.full(nu + 1 + extra, OG, np.uint64), np.full(nu + extra, SG, np.uint64),
            np.full(nu + extra, FG, np.uint32))


def untouched(bufs):
    b, o, s, f = bufs
    return bool((b == BG).all() and (o == OG).all() and (s == SG).all() and (f == FG).all())


def dev_buffers(torch, nu, nb, extra=2):
    return tuple(torch.from_numpy(a.view(v)).cuda() for a, v in zip(host_buffers(nu, nb, extra), (np.uint8, np.int64, np.int64, np.int32)))


def dev_untouched(torch, bufs):
    torch.cuda.synchronize()
    views = (np.uint8, np.uint64, np.uint64, np.uint32)
    return untouched(tuple(t.cpu().numpy().view(v) for t, v in zip(bufs, views)))


def test_unitigs_shapes(torch_mod, ctx, oracle):
    torch = torch_mod
    from kmertools_amd import device
    from kmertools_amd._lib import KT_ERR_ARG, lib
    L = lib()
    k = 23
    made = []
    try:
        # an empty table: 0 / 0 and offsets[0] = 0; count-only touches nothing
        empty = device.Counter(ctx, k, 1 << 16)
        made.append(empty)
        got = empty.unitigs()
        assert [len(a) for a in got] == [0, 1, 0, 0] and got[1][0] == 0
        nu, nb = C.c_uint64(9), C.c_uint64(9)
        assert raw(L, empty._h, nu=nu, nb=nb) == 0 and (nu.value, nb.value) == (0, 0)
        for mem in (0, 1):
            bufs = host_buffers(3, 40) if mem == 0 else dev_buffers(torch, 3, 40)
            nu, nb = C.c_uint64(9), C.c_uint64(9)
            assert raw(L, empty._h, bases=bufs[0], max_bases=40, offsets=bufs[1], sums=bufs[2], flags=bufs[3], max_unitigs=3,
                       nu=nu, nb=nb, mem=mem) == 0
            assert (nu.value, nb.value) == (0, 0)
            torch.cuda.synchronize()
            o = bufs[1] if mem == 0 else bufs[1].cpu().numpy().view(np.uint64)
            assert o[0] == 0 and (o[1:] == OG).all()
        assert empty.size() == 0
        # one entry: one unitig, the k-mer itself
        one = pairs_counter(ctx, k, [gr.key_of("ACGTTGCATGCAGGATCCATTAG")], [3])
        made.append(one)
        check_both_modes(torch, one, as_arrays([("ACGTTGCATGCAGGATCCATTAG", 3, 0, 1)]))
        # a node count that is no multiple of any tile
        bases, offsets = sample(723, k)
        tk, tc = sorted_table(*oracle.count_reads(bases, offsets, k))
        assert len(tk) % 256 and len(tk) > 3000
        c = counter_of(ctx, k, bases, offsets, len(tk))
        made.append(c)
        want = as_arrays(ur.unitigs(strings_table(tk, tc, k), k))
        wnu, wnb = len(want[2]), len(want[0])
        assert wnu > 20
        # count only: no arrays, host and device
        for mem in (0, 1):
            nu, nb = C.c_uint64(9), C.c_uint64(9)
            assert raw(L, c._h, nu=nu, nb=nb, mem=mem) == 0 and (nu.value, nb.value) == (wnu, wnb), mem
        assert c.unitigs_device(None, 0, None, None, None, 0) == (wnu, wnb)
        # a range with no nodes: 0 / 0, offsets[0] = 0
        top = int(tc.max()) + 1
        got = c.unitigs(top, None)
        assert [len(a) for a in got] == [0, 1, 0, 0] and got[1][0] == 0
        bufs = dev_buffers(torch, 3, 40)
        assert c.unitigs_device(bufs[0], 40, bufs[1], bufs[2], bufs[3], 3, top, None) == (0, 0)
        torch.cuda.synchronize()
        o = bufs[1].cpu().numpy().view(np.uint64)
        assert o[0] == 0 and (o[1:] == OG).all() and bool((bufs[0] == BG).all())
        # count_sums / flags NULL, together and one at a time
        for sums, flags in ((False, False), (True, False), (False, True)):
            b, o, s, f = host_buffers(wnu, wnb)
            nu, nb = C.c_uint64(0), C.c_uint64(0)
            assert raw(L, c._h, bases=b, max_bases=wnb, offsets=o, sums=s if sums else None, flags=f if flags else None,
                       max_unitigs=wnu, nu=nu, nb=nb) == 0
            assert np.array_equal(b[:wnb], want[0]) and np.array_equal(o[:wnu + 1], want[1])
            assert np.array_equal(s[:wnu], want[2]) if sums else (s == SG).all()
            assert np.array_equal(f[:wnu], want[3]) if flags else (f == FG).all()
            assert (b[wnb:] == BG).all() and (o[wnu + 1:] == OG).all() and (s[wnu:] == SG).all() and (f[wnu:] == FG).all()
            got = unitigs_dev(torch, c, 1, None, wnu, wnb, sums=sums, flags=flags)
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
            assert not sums or np.array_equal(got[2], want[2])
            assert not flags or np.array_equal(got[3], want[3])
        # each room one too small: KT_ERR_ARG, both numbers exact, nothing written
        for mem in (0, 1):
            for short_u, short_b in ((1, 0), (0, 1), (1, 1)):
                bufs = host_buffers(wnu, wnb) if mem == 0 else dev_buffers(torch, wnu, wnb)
                nu, nb = C.c_uint64(0), C.c_uint64(0)
                rc = raw(L, c._h, bases=bufs[0], max_bases=wnb - short_b, offsets=bufs[1], sums=bufs[2], flags=bufs[3],
                         max_unitigs=wnu - short_u, nu=nu, nb=nb, mem=mem)
                assert rc == KT_ERR_ARG and L.kt_last_error() and (nu.value, nb.value) == (wnu, wnb), (mem, short_u, short_b)
                assert untouched(bufs) if mem == 0 else dev_untouched(torch, bufs), (mem, short_u, short_b)
        with pytest.raises(device._lib.KmertoolsError):
            bufs = dev_buffers(torch, 4, 100)
            c.unitigs_device(bufs[0], 100, bufs[1], bufs[2], bufs[3], 4)
        # more room than needed: nothing past the result
        b, o, s, f = host_buffers(wnu + 5, wnb + 50)
        nu, nb = C.c_uint64(0), C.c_uint64(0)
        assert raw(L, c._h, bases=b, max_bases=wnb + 50, offsets=o, sums=s, flags=f, max_unitigs=wnu + 5, nu=nu, nb=nb) == 0
        assert same((b[:wnb], o[:wnu + 1], s[:wnu], f[:wnu]), want)
        assert (b[wnb:] == BG).all() and (o[wnu + 1:] == OG).all() and (s[wnu:] == SG).all() and (f[wnu:] == FG).all()
    finally:
        for t in reversed(made):
            t.close()


def test_unitigs_errors(torch_mod, ctx, oracle):
    torch = torch_mod
    from kmertools_amd import device
    from kmertools_amd._lib import KT_ERR_ARG, KT_ERR_FULL, lib
    L = lib()
    k = 21
    bases, offsets = sample(6000, k)
    made = []  # closed whatever happens: a table must not outlive its context

    def keep(c):
        made.append(c)
        return c

    try:
        a = keep(counter_of(ctx, k, bases, offsets, 1 << 16))
        wnu, wnb = a.unitigs_device(None, 0, None, None, None, 0)
        assert wnu > 20
        bufs = host_buffers(wnu, wnb, 0)
        nu, nb = C.c_uint64(77), C.c_uint64(88)

        def call(t=a._h, **kw):
            kw.setdefault("bases", bufs[0])
            kw.setdefault("offsets", bufs[1])
            kw.setdefault("sums", bufs[2])
            kw.setdefault("flags", bufs[3])
            kw.setdefault("max_bases", wnb)
            kw.setdefault("max_unitigs", wnu)
            kw.setdefault("nu", nu)
            kw.setdefault("nb", nb)
            return raw(L, t, **kw)

        for kw in (dict(t=None), dict(nu=None), dict(nb=None), dict(lo=0), dict(lo=0, hi=0), dict(lo=3, hi=2),
                   dict(lo=U32, hi=U32 - 1), dict(mem=2), dict(mem=-1), dict(bases=None), dict(offsets=None),
                   dict(bases=None, offsets=None), dict(offsets=None, max_bases=0), dict(bases=None, max_unitigs=0)):
            assert call(**kw) == KT_ERR_ARG, kw
            assert L.kt_last_error(), kw
        # one shard of a sharded table (allocated as rank 0 of 2, never connected)
        sh = keep(device.Sharded(ctx, k, 1 << 16, 1 << 16, 2, 0, ("host", lambda s, r, n: 1), connect=False))
        assert call(t=sh.table._h) == KT_ERR_ARG and b"shard" in L.kt_last_error()
        # an overflowed table (far more distinct keys than slots)
        full = keep(device.Counter(ctx, k, 1024))
        full.add_pairs_host(np.arange(1, 5000, dtype=np.uint64) * 7919, np.ones(4999, np.uint32))
        assert call(t=full._h) == KT_ERR_FULL and L.kt_last_error()
        assert call(t=full._h, bases=None, offsets=None, sums=None, flags=None, max_bases=0, max_unitigs=0) == KT_ERR_FULL
        # no refused call wrote anything, the sizes included
        assert untouched(bufs) and (nu.value, nb.value) == (77, 88)
        # device outputs are left alone as well
        dbufs = dev_buffers(torch, wnu, wnb, 0)
        for t, lo, hi, want in ((a._h, 0, U32, KT_ERR_ARG), (a._h, 9, 8, KT_ERR_ARG), (sh.table._h, 1, U32, KT_ERR_ARG),
                                (full._h, 1, U32, KT_ERR_FULL)):
            rc = raw(L, t, lo, hi, dbufs[0], wnb, dbufs[1], dbufs[2], dbufs[3], wnu, nu, nb, 1)
            assert rc == want and L.kt_last_error(), (lo, hi)
        assert dev_untouched(torch, dbufs) and (nu.value, nb.value) == (77, 88)
        assert call() == 0 and (nu.value, nb.value) == (wnu, wnb)  # the context is still good
    finally:
        for c in reversed(made):
            c.close()


# ---- 8. the CLI end to end ------------------------------------------------------------------------------------------------

def run(*args, env=None):
    return subprocess.run([CLI, *map(str, args)], capture_output=True, timeout=600, env=env)


@pytest.fixture(scope="module")
def cli_bin():
    if not os.path.exists(CLI):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "kmertools_amd", "csrc"), "-j4"], stdout=subprocess.DEVNULL)
    return CLI


@pytest.mark.parametrize("k", [15, 31])
def test_unitigs_cli_end_to_end(cli_bin, oracle, tmp_path, k):
    fa = tmp_path / "reads.fasta"
    cyc = np.frombuffer(b"ACGT", np.uint8)[np.random.default_rng(k).integers(0, 4, size=300)].tobytes()
    reads = noisy_reads(80 + k, 500, k, 4000) + [cyc + cyc[:k - 1]] * 2
    fa.write_bytes(b"".join(b">rec%d lane=%d  sample x\n%s\n" % (i, i % 5, s) for i, s in enumerate(reads)))
    tk, tc = sorted_table(*oracle.count_reads(*oracle.to_csr([s for _, s in oracle.read_records(str(fa))]), k))
    table = strings_table(tk, tc, k)
    env = dict(os.environ, KT_CLI_TIMING="1")
    cases = (("plain", [], 1, U32), ("min2", ["--min-count", 2], 2, U32), ("min2max5", ["--min-count", 2, "--max-count", 5], 2, 5))
    for name, flags, lo, hi in cases:
        want_fa, want_stats = ur.want_files(table, k, lo, hi)
        assert want_fa.count(b">") > 20 and (name != "plain" or b" CL:i:1\n" in want_fa)
        d = tmp_path / name
        r = run("unitigs", "-i", fa, "-o", d, "-k", k, *flags, env=env)
        assert r.returncode == 0, r.stderr
        assert (d / "unitigs.fa").read_bytes() == want_fa, (k, name)
        assert (d / "unitigs.stats").read_bytes() == want_stats, (k, name)
        assert sorted(os.listdir(d)) == ["unitigs.fa", "unitigs.stats"]
        d2 = tmp_path / (name + "_stats_only")
        r = run("unitigs", "-i", fa, "-o", d2, "-k", k, *flags, "--stats-only", env=env)
        assert r.returncode == 0, r.stderr
        assert os.listdir(d2) == ["unitigs.stats"] and (d2 / "unitigs.stats").read_bytes() == want_stats, (k, name)
    # the same in batches of 7 reads, and from the dense bulk build
    want_fa, want_stats = ur.want_files(table, k)
    for name, extra in (("batched", dict(KT_CLI_BATCH_READS="7")), ("dense", dict(KT_BULK_MIN_BASES="0"))):
        d = tmp_path / name
        r = run("unitigs", "-i", fa, "-o", d, "-k", k, env=dict(env, **extra))
        assert r.returncode == 0, r.stderr
        assert (d / "unitigs.fa").read_bytes() == want_fa and (d / "unitigs.stats").read_bytes() == want_stats, (k, name)
    # a table that would take passes: refused before any file exists
    d = tmp_path / "passes"
    r = run("unitigs", "-i", fa, "-o", d, "-k", k, "--min-count", 2, env=dict(env, KT_CTR_MAX_SLOTS="4096"))
    assert r.returncode != 0 and r.returncode != 2
    msg = r.stderr.decode()
    assert msg.startswith("Error: ") and "unitigs needs the whole table on the device" in msg and "--min-count is no remedy" in msg
    assert not d.exists() or os.listdir(d) == []
