"""Read error correction: kt_ctr_correct_support (per uncovered base, in how many windows each other nucleotide makes a
solid k-mer) and kt_correct_apply (the decision) against a restatement over the oracle's k-mers and table and a few lines of
numpy - host and device mode, the corners of the rule, every table form, hash partitions, synthetic support and profile
arrays, argument errors, shifted views with fenced guards, planted errors that really get repaired, full size; and
`kmertools correct` end to end, byte for byte against files restated from the parsed records.  The rule is integers: every
comparison is exact."""
import gzip
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "kmertools_amd", "bin", "kmertools")
GOLDEN = os.path.join(ROOT, "tests", "golden")
NO = 0xFFFFFFFF  # KT_NO_KMER
U32_MAX = 0xFFFFFFFF
SEG = 8192  # bases per workgroup of the support kernel (kt_segment.hpp)
ACGT = np.frombuffer(b"ACGT", np.uint8)
NT4 = np.full(256, 4, np.uint8)  # ktd::nt4: A/a 0, C/c 1, G/g 2, T/t/U/u 3, raw bytes 0..3 themselves, 4: invalid
for _ch, _c in zip(b"ACGTU", (0, 1, 2, 3, 3)):
    NT4[_ch] = NT4[_ch | 0x20] = _c
NT4[:4] = np.arange(4)


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
    """Counter(ctx, k, capacity) whose table is released when the test ends, however it ends (one that is only collected when
    the interpreter exits would be destroyed after the HIP runtime)"""
    from kmertools_amd import device
    made = []

    def make(k, capacity):
        made.append(device.Counter(ctx, k, capacity))
        return made[-1]

    yield make
    for c in made:
        c.close()


# ---- the restatement ----------------------------------------------------------------------------------------------------

class Table:
    """a table as sorted (canonical key, count) arrays: count of a k-mer, 0 when absent"""

    def __init__(self, keys, counts):
        order = np.argsort(keys)
        self.keys, self.counts = np.asarray(keys, np.uint64)[order], np.asarray(counts, np.uint32)[order]

    @classmethod
    def of_reads(cls, oracle, bases, offsets, k):
        return cls(*oracle.count_reads(bases, offsets, k, 1, 1))

    def count(self, keys):
        if not len(self.keys):
            return np.zeros(len(keys), np.uint32)
        i = np.minimum(np.searchsorted(self.keys, keys), len(self.keys) - 1)
        return np.where(self.keys[i] == keys, self.counts[i], 0).astype(np.uint32)


def want_profile(oracle, bases, offsets, k, table):
    """kt_ctr_profile's complete answer: the count at each valid window start, KT_NO_KMER elsewhere"""
    prof = np.full(int(offsets[-1]), NO, np.uint32)
    for i in range(len(offsets) - 1):
        o, e = int(offsets[i]), int(offsets[i + 1])
        if e - o < k:
            continue
        f, r, end = oracle.kmers(bases[o:e].tobytes(), k)
        if len(f):
            prof[o + end.astype(np.int64) - (k - 1)] = np.minimum(table.count(np.minimum(f, r)), 0xFFFFFFFE)
    return prof


def read_of_base(offsets):
    total = int(offsets[-1])
    return np.searchsorted(offsets.astype(np.int64), np.arange(total, dtype=np.int64), side="right") - 1


def owner_of(keys, n):
    """ktd::owner_of over an array (checked against the library's kt_owner_of where it is used)"""
    h = keys.astype(np.uint64) * np.uint64(0x9E3779B97F4A7C15)
    h ^= h >> np.uint64(32)
    return (((h & np.uint64(0xFFFFFFFF)) * np.uint64(n)) >> np.uint64(32)).astype(np.int64)


def want_covered(prof, offsets, k, lo, hi):
    """step 1, from the profile alone: base g of read [o, e) is covered when a window j in [max(o, g-k+1), min(g, e-k)] has
    profile[j] != KT_NO_KMER and lo <= profile[j] <= hi"""
    total = len(prof)
    g = np.arange(total, dtype=np.int64)
    rid = read_of_base(offsets)
    o, e = offsets[rid].astype(np.int64), offsets[rid + 1].astype(np.int64)
    ok = (prof != NO) & (prof >= lo) & (prof <= hi) & (g <= e - k)
    c = np.concatenate(([0], np.cumsum(ok)))
    return (c[g + 1] - c[np.maximum(o, g - k + 1)]) > 0


def want_support(oracle, bases, offsets, k, table, prof, lo, hi, keep=None):
    """step 2: for every uncovered base g of a read of at least k bases and every x != code(g): the k-mers of the read's
    stretch [max(o, g-k+1), min(e, g+k)) with x written at g (every window of it contains g; one over an invalid byte is
    none) that are solid, counted into byte x.  keep(keys) -> bool: only those k-mers count (a hash partition)."""
    total = int(offsets[-1])
    sup = np.zeros(total, np.uint32)
    if not total:
        return sup
    rid = read_of_base(offsets)
    o, e = offsets[rid].astype(np.int64), offsets[rid + 1].astype(np.int64)
    todo = np.flatnonzero(~want_covered(prof, offsets, k, lo, hi) & (e - o >= k))
    code = NT4[bases]
    W = 2 * k  # a stretch has at most 2k - 1 bases: the last column is always the N that separates the rows
    for x in range(4):
        gx = todo[code[todo] != x]
        for at in range(0, len(gx), 100_000):
            g = gx[at:at + 100_000]
            a, b = np.maximum(o[g], g - k + 1), np.minimum(e[g], g + k)
            idx = a[:, None] + np.arange(W)[None, :]
            rows = np.where(idx < b[:, None], bases[np.minimum(idx, total - 1)], ord("N")).astype(np.uint8)
            rows[np.arange(len(g)), g - a] = ACGT[x]
            f, r, end = oracle.kmers(rows.tobytes(), k)
            keys = np.minimum(f, r)
            cnt = table.count(keys)
            good = (cnt >= lo) & (cnt <= hi)
            if keep is not None:
                good &= keep(keys)
            s = np.bincount((end.astype(np.int64) // W)[good], minlength=len(g))
            assert s.max(initial=0) <= k
            sup[g] |= s.astype(np.uint32) << np.uint32(8 * x)
    return sup


def want_apply(bases, offsets, sup, min_support=1, max_corrections=0):
    """step 3 -> (out_bases, n_single, n_ambiguous)"""
    n = len(offsets) - 1
    by = (sup[:, None] >> np.array([0, 8, 16, 24], np.uint32)[None, :]) & np.uint32(255)
    m = by >= min_support
    cands = m.sum(axis=1)
    single, amb = cands == 1, cands >= 2
    rid = read_of_base(offsets)
    ns = np.bincount(rid[single], minlength=n).astype(np.uint32)
    na = np.bincount(rid[amb], minlength=n).astype(np.uint32)
    out = bases[:len(sup)].copy()
    sel = single & ((ns <= max_corrections) | (max_corrections == 0))[rid] if len(sup) else single
    out[sel] = ACGT[m.argmax(axis=1)[sel]]
    return out, ns, na


# ---- inputs ---------------------------------------------------------------------------------------------------------------

def rc(s):
    return (3 - NT4[s][::-1]).astype(np.uint8)


def sub(s, at, rng=None):
    """a substitution at `at` (the next nucleotide, or a random other one)"""
    c = int(NT4[s[at]])
    s[at] = ACGT[(c + (1 if rng is None else int(rng.integers(1, 4)))) & 3]


def corner_batch(seed, k):
    """reads sampled from a small genome (one stretch of it three times over: its k-mers are the abundant ones) with
    substitutions planted where the rule has corners - see the comments - in an order that puts the long reads' planted
    errors on the last and the first base of a segment"""
    rng = np.random.default_rng(seed)
    genome = ACGT[rng.integers(0, 4, size=6000)]
    genome[3000:3300] = genome[1000:1300]
    genome[5000:5300] = genome[1000:1300]
    G = len(genome)
    ring = np.concatenate([genome] * 5)

    def sample(L, a=None):
        a = int(rng.integers(0, G - L)) if a is None else a
        s = genome[a:a + L].copy()
        return ACGT[rc(s)] if rng.random() < 0.5 else s

    seqs = []
    # two long reads first (so that their place in the batch is known): errors on both sides of the segment edges
    for L in (20_000, 10_500):
        o = sum(len(s) for s in seqs)
        s = ring[37:37 + L].copy()
        for edge in range(SEG, o + L, SEG):
            if edge - 1 >= o and edge < o + L:
                sub(s, edge - 1 - o)
                sub(s, edge - o)
        sub(s, 0)
        sub(s, L - 1)
        s[L // 2] = ord("N")
        seqs.append(s)
    plain = [sample(150) for _ in range(700)]  # the coverage: about 17 x
    seqs += plain
    L = 150
    for at in (0, L - 1, k - 1, k, L - k, L - k - 1, k - 2, 75):  # position 0, the last base, k-1 and k from either end
        s = sample(L)
        sub(s, at)
        seqs.append(s)
    for gap in (k - 1, k, k + 1, 1, 2):  # two errors: no clean window between them, exactly one, two
        s = sample(L)
        sub(s, 50)
        sub(s, 50 + gap)
        seqs.append(s)
    for at, run in ((0, 1), (70, 1), (L - 1, 1), (40, 3), (60, k), (3, 2)):  # N alone and in runs
        s = sample(L)
        s[at:at + run] = ord("N")
        seqs.append(s)
    s = sample(L)
    s[20], s[100] = ord("N"), ord("n")
    sub(s, 60)
    seqs.append(s)
    for _ in range(3):  # lower case, U, and an error in them
        s = np.frombuffer(sample(L).tobytes().lower(), np.uint8).copy()
        sub(s, int(rng.integers(0, L)))
        seqs.append(s)
    s = sample(L)
    s[s == ord("T")] = ord("U")
    sub(s, 33)
    seqs.append(s)
    for Ls in (k - 1, k, k, k + 1, k + 1, 0, 1, 0):  # shorter than k, k, k + 1 (with and without an error), empty
        seqs.append(sample(Ls))
    for Ls in (k, k + 1, k + 1):
        s = sample(Ls)
        sub(s, Ls // 2)
        seqs.append(s)
    s = sample(k + 1)
    sub(s, 0)
    seqs.append(s)
    for i in range(900):  # many 20-base reads per segment, every third with an error
        s = sample(20)
        if i % 3 == 0:
            sub(s, int(rng.integers(0, 20)), rng)
        seqs.append(s)
    seqs.append(ACGT[rng.integers(0, 4, size=400)])  # a foreign read: uncovered from end to end
    for _ in range(120):  # random errors, 2 %
        s = sample(L)
        for at in np.flatnonzero(rng.random(L) < 0.02):
            sub(s, int(at), rng)
        seqs.append(s)
    tail = seqs[2:]
    order = rng.permutation(len(tail))
    return [bytes(x) for x in seqs[:2]] + [bytes(tail[i]) for i in order]


def u32(t):
    return t.cpu().numpy().view(np.uint32)


def dev(torch, a):
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint64:
        a = a.view(np.int64)
    elif a.dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(a if a.size else np.zeros(1, a.dtype)).cuda()


def support_device(torch, ctr, bases, offsets, prof, lo, hi, n_parts=1, part=0, into=None):
    """the device-mode call into zeros with a guard element behind them -> (array, guard)"""
    total = int(offsets[-1])
    sup = into if into is not None else torch.zeros(total + 1, dtype=torch.int32, device="cuda")
    ctr.correct_support(dev(torch, bases), dev(torch, offsets), len(offsets) - 1, dev(torch, prof), lo, hi, sup,
                        n_parts=n_parts, part=part)
    torch.cuda.synchronize()
    got = u32(sup)
    return got[:total], got[total]


def support_host(ctr, bases, offsets, prof, lo, hi, n_parts=1, part=0, into=None):
    from kmertools_amd._lib import KT_MEM_HOST
    total = int(offsets[-1])
    sup = into if into is not None else np.zeros(total + 1, np.uint32)
    ctr.correct_support(bases if bases.size else np.zeros(1, np.uint8), offsets, len(offsets) - 1,
                        prof if prof.size else np.zeros(1, np.uint32), lo, hi, sup, KT_MEM_HOST, n_parts, part)
    return sup[:total], sup[total]


def apply_device(torch, ctx, bases, offsets, sup, min_support=1, max_corrections=0):
    """the device-mode call into arrays primed with a pattern (the outputs are overwritten)"""
    n, total = len(offsets) - 1, int(offsets[-1])
    out = torch.full((total + 1,), 0x5A, dtype=torch.uint8, device="cuda")
    ns = torch.full((n + 1,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    na = torch.full((n + 1,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    ctx.correct_apply(dev(torch, bases), dev(torch, offsets), n, dev(torch, sup), min_support, max_corrections, out, ns, na)
    torch.cuda.synchronize()
    assert int(out[total]) == 0x5A and u32(ns)[n] == 0x5A5A5A5A and u32(na)[n] == 0x5A5A5A5A
    return out.cpu().numpy()[:total], u32(ns)[:n], u32(na)[:n]


def apply_host(ctx, bases, offsets, sup, min_support=1, max_corrections=0):
    from kmertools_amd._lib import KT_MEM_HOST
    n, total = len(offsets) - 1, int(offsets[-1])
    out = np.full(total + 1, 0x5A, np.uint8)
    ns = np.full(n + 1, 0x5A5A5A5A, np.uint32)
    na = np.full(n + 1, 0x5A5A5A5A, np.uint32)
    ctx.correct_apply(bases if bases.size else np.zeros(1, np.uint8), offsets, n, sup if sup.size else np.zeros(1, np.uint32),
                      min_support, max_corrections, out, ns, na, KT_MEM_HOST)
    assert out[total] == 0x5A and ns[n] == 0x5A5A5A5A and na[n] == 0x5A5A5A5A
    return out[:total], ns[:n], na[:n]


def same(got, want, tag):
    for name, g, w in zip(("out_bases", "n_single", "n_ambiguous"), got, want):
        bad = np.flatnonzero(g != w)
        assert not len(bad), (tag, name, bad[:5], g[bad[:5]], w[bad[:5]])


def check_apply(torch, ctx, bases, offsets, sup, tag, settings=((1, 0),)):
    for ms, mc in settings:
        want = want_apply(bases, offsets, sup, ms, mc)
        same(apply_host(ctx, bases, offsets, sup, ms, mc), want, (tag, ms, mc, "host"))
        same(apply_device(torch, ctx, bases, offsets, sup, ms, mc), want, (tag, ms, mc, "device"))


# ---- 1. support and apply against the restatement ---------------------------------------------------------------------------

@pytest.mark.parametrize("k", [11, 15, 21, 31])
def test_correct_against_restatement(torch_mod, ctx, oracle, make_counter, k):
    from kmertools_amd import device
    from kmertools_amd.device import to_csr
    seqs = corner_batch(100 + k, k)
    assert len(seqs[0]) > 2 * SEG and any(len(s) == k for s in seqs) and any(len(s) == 0 for s in seqs)
    bases, offsets = to_csr(seqs)
    table = Table.of_reads(oracle, bases, offsets, k)
    ctr = make_counter(k, max(1 << 16, 2 * len(table.keys)))
    ctr.add_pairs_host(table.keys, table.counts)
    prof = want_profile(oracle, bases, offsets, k, table)
    assert np.array_equal(ctr.profile_host(bases, offsets), prof)
    # (2, ..): the errors are weak; (3, 30): the genome's threefold stretch is weak as well; (1, 1): only what was seen once is solid
    ambiguous_seen = False
    for lo, hi in ((2, U32_MAX), (3, 30), (4, U32_MAX), (1, 1)):
        want = want_support(oracle, bases, offsets, k, table, prof, lo, hi)
        cov = want_covered(prof, offsets, k, lo, hi)
        assert not want[cov].any() and want.any() and cov.any() and not cov.all()
        got, guard = support_device(torch_mod, ctr, bases, offsets, prof, lo, hi)
        assert guard == 0 and np.array_equal(got, want), (k, lo, hi, "device", np.flatnonzero(got != want)[:5])
        got, guard = support_host(ctr, bases, offsets, prof, lo, hi)
        assert guard == 0 and np.array_equal(got, want), (k, lo, hi, "host", np.flatnonzero(got != want)[:5])
        _, ns, na = want_apply(bases, offsets, want)
        assert ns.any() and (ns == 0).any()
        ambiguous_seen = ambiguous_seen or bool(na.any())
        check_apply(torch_mod, ctx, bases, offsets, want, (k, lo, hi), ((1, 0), (2, 0), (1, 1), (1, 2), (k, 0)))
        out, ns, na = ctr.correct_host(bases, offsets, lo, None if hi == U32_MAX else hi)
        same((out, ns, na), want_apply(bases, offsets, want), (k, lo, hi, "correct_host"))
    # the corners really occur at the usual setting
    want = want_support(oracle, bases, offsets, k, table, prof, 2, U32_MAX)
    out, ns, na = want_apply(bases, offsets, want)
    assert ambiguous_seen and (out != bases).sum() > 50
    assert ((want >> 24) != 0).any()          # a T candidate
    assert (want[NT4[bases] == 4] != 0).any()  # an N with a supported candidate
    # no reads, and reads with no bases at all
    for offs in (np.zeros(1, np.uint64), np.zeros(4, np.uint64)):
        out, ns, na = ctr.correct_host(np.zeros(0, np.uint8), offs)
        assert len(out) == 0 and len(ns) == len(offs) - 1 and not ns.any() and not na.any()
    same(apply_host(ctx, np.zeros(0, np.uint8), np.zeros(4, np.uint64), np.zeros(0, np.uint32)),
         (np.zeros(0, np.uint8), np.zeros(3, np.uint32), np.zeros(3, np.uint32)), "empty reads")
    ctr.close()


# ---- 2. every table form ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", [13, 21])
def test_correct_every_table_form(torch_mod, ctx, oracle, make_counter, monkeypatch, k):
    torch = torch_mod
    from kmertools_amd import device
    from kmertools_amd.device import to_csr
    seqs = corner_batch(500 + k, k)
    bases, offsets = to_csr(seqs)
    table = Table.of_reads(oracle, bases, offsets, k)
    cap = max(1 << 16, 2 * len(table.keys))
    prof = want_profile(oracle, bases, offsets, k, table)
    lo, hi = 2, U32_MAX
    want = want_support(oracle, bases, offsets, k, table, prof, lo, hi)
    assert want.any()
    forms = []

    def check(ctr, tag):
        assert ctr.size() == len(table.keys), tag
        got, guard = support_host(ctr, bases, offsets, prof, lo, hi)
        assert guard == 0 and np.array_equal(got, want), (tag, k, "host")
        got, guard = support_device(torch, ctr, bases, offsets, prof, lo, hi)
        assert guard == 0 and np.array_equal(got, want), (tag, k, "device")
        forms.append(tag)

    ctr = make_counter(k, cap)
    ctr.add_reads_host(bases, offsets)
    check(ctr, "probing")
    ctr.close()
    ctr = make_counter(k, cap)
    ctr.add_pairs_host(table.keys, table.counts)
    check(ctr, "add_pairs")
    ctr.close()
    monkeypatch.setenv("KT_BULK", "1")
    monkeypatch.setenv("KT_BULK_MIN_BASES", "0")
    ctr = make_counter(k, cap)
    ctr.add_reads_host(bases, offsets)
    check(ctr, "bulk")
    ctr.close()
    m = len(table.keys) + 9
    xk = torch.zeros(m, dtype=torch.int64, device="cuda")
    xc = torch.zeros(m, dtype=torch.int32, device="cuda")
    ctr = make_counter(k, cap)
    ctr.export_target(xk, xc, m)
    ctr.add_reads(torch.from_numpy(bases).cuda(), torch.from_numpy(offsets.astype(np.int64)).cuda(), len(seqs))
    check(ctr, "export target")
    ctr.close()
    if k <= 15:
        ctr = make_counter(k, 4 ** k)
        assert ctr.capacity() == 4 ** k
        ctr.add_reads_host(bases, offsets)
        check(ctr, "direct")
        ctr.close()
    assert len(forms) == (5 if k <= 15 else 4)


# ---- 3. hash partitions -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", [15, 31])
def test_correct_partitions_combine(torch_mod, ctx, oracle, make_counter, k):
    torch = torch_mod
    from kmertools_amd import device
    from kmertools_amd.device import to_csr
    seqs = corner_batch(700 + k, k)
    bases, offsets = to_csr(seqs)
    table = Table.of_reads(oracle, bases, offsets, k)
    some = table.keys[:: max(1, len(table.keys) // 500)]
    for n in (2, 3, 5):
        assert np.array_equal(owner_of(some, n), [device.owner_of(int(x), n) for x in some])
    prof = want_profile(oracle, bases, offsets, k, table)
    lo, hi = 2, U32_MAX
    whole = want_support(oracle, bases, offsets, k, table, prof, lo, hi)
    total = int(offsets[-1])
    for n_parts in (2, 3, 5):
        hs = np.zeros(total + 1, np.uint32)
        ds = torch.zeros(total + 1, dtype=torch.int32, device="cuda")
        sizes = 0
        for part in range(n_parts):
            ctr = make_counter(k, max(1 << 16, 2 * len(table.keys)))
            ctr.add_reads_host(bases, offsets, n_parts, part)
            sizes += ctr.size()
            if n_parts == 3 or part == 0:  # a single part on its own
                alone = want_support(oracle, bases, offsets, k, table, prof, lo, hi, lambda keys: owner_of(keys, n_parts) == part)
                got, guard = support_device(torch, ctr, bases, offsets, prof, lo, hi, n_parts, part)
                assert guard == 0 and np.array_equal(got, alone), (k, n_parts, part)
                assert alone.any() and not np.array_equal(alone, whole)
            support_host(ctr, bases, offsets, prof, lo, hi, n_parts, part, into=hs)
            support_device(torch, ctr, bases, offsets, prof, lo, hi, n_parts, part, into=ds)
            ctr.close()
        assert sizes == len(table.keys)
        assert hs[total] == 0 and np.array_equal(hs[:total], whole), (k, n_parts, "host")
        got = u32(ds)
        assert got[total] == 0 and np.array_equal(got[:total], whole), (k, n_parts, "device")


# ---- 4. kt_correct_apply alone ------------------------------------------------------------------------------------------------

def pattern_support(rng, total, values):
    """support words of every class: no, one, two, three, four supported candidates, the values on both sides of thresholds"""
    sup = np.zeros(total, np.uint32)
    pick = rng.random(total) < 0.3
    for x in range(4):
        on = pick & (rng.random(total) < 0.45)
        sup |= np.where(on, rng.choice(values, size=total), 0).astype(np.uint32) << np.uint32(8 * x)
    return sup


def test_correct_apply_synthetic(torch_mod, ctx):
    torch = torch_mod
    from kmertools_amd._lib import KT_MEM_HOST
    rng = np.random.default_rng(5)
    lens = np.concatenate([rng.integers(0, 300, size=3000), [0, 0, 1, 1, 2, 70_000, 0, 9000]])
    offsets = np.zeros(len(lens) + 1, np.uint64)
    offsets[1:] = np.cumsum(lens)
    total = int(offsets[-1])
    letters = np.frombuffer(b"ACGTNacgtnUu\x00\x01\x02\x03RY", np.uint8)
    bases = letters[rng.integers(0, len(letters), size=total)].copy()
    sup = pattern_support(rng, total, np.array([0, 1, 2, 3, 31, 254, 255]))
    by = (sup[:, None] >> np.array([0, 8, 16, 24], np.uint32)) & 255
    for ms in (1, 2, 255):
        n_c = (by >= ms).sum(axis=1)
        assert all((n_c == c).any() for c in range(4)), ms
    _, ns, _ = want_apply(bases, offsets, sup)
    busy = int(np.median(ns[ns > 0]))
    settings = [(1, 0), (2, 0), (255, 0), (3, 0), (1, busy - 1), (1, busy), (1, busy + 1), (2, 1), (255, 1), (1, U32_MAX)]
    check_apply(torch, ctx, bases, offsets, sup, "patterns", settings)
    for ms, mc in ((1, busy), (2, 0)):
        want = want_apply(bases, offsets, sup, ms, mc)
        assert (want[0] != bases).any() and (want[1] > 0).any() and (want[2] > 0).any()
        if mc:
            assert (want[1] > mc).any() and ((want[1] <= mc) & (want[1] > 0)).any()
        # NULL outputs, each alone and in pairs; in place
        n = len(lens)
        for use in ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1)):
            out = np.full(total, 0x5A, np.uint8) if use[0] else None
            a = np.full(n, 7, np.uint32) if use[1] else None
            b = np.full(n, 7, np.uint32) if use[2] else None
            ctx.correct_apply(bases, offsets, n, sup, ms, mc, out, a, b, KT_MEM_HOST)
            same([x for x in (out, a, b) if x is not None], [w for w, u in zip(want, use) if u], ("null host", use, ms, mc))
            dout = torch.full((total,), 0x5A, dtype=torch.uint8, device="cuda") if use[0] else None
            da = torch.full((n,), 7, dtype=torch.int32, device="cuda") if use[1] else None
            db_ = torch.full((n,), 7, dtype=torch.int32, device="cuda") if use[2] else None
            ctx.correct_apply(dev(torch, bases), dev(torch, offsets), n, dev(torch, sup), ms, mc, dout, da, db_)
            torch.cuda.synchronize()
            got = [x.cpu().numpy() if x.dtype == torch.uint8 else u32(x) for x in (dout, da, db_) if x is not None]
            same(got, [w for w, u in zip(want, use) if u], ("null device", use, ms, mc))
        ctx.correct_apply(bases, offsets, n, sup, ms, mc, None, None, None, KT_MEM_HOST)  # nothing asked for: fine
        inplace = bases.copy()
        ctx.correct_apply(inplace, offsets, n, sup, ms, mc, inplace, None, None, KT_MEM_HOST)
        assert np.array_equal(inplace, want[0])
        dinplace = dev(torch, bases)
        ctx.correct_apply(dinplace, dev(torch, offsets), n, dev(torch, sup), ms, mc, dinplace, None, None)
        torch.cuda.synchronize()
        assert np.array_equal(dinplace.cpu().numpy(), want[0])


def test_correct_apply_long_and_many(torch_mod, ctx):
    """a 20 Mbase read beside short ones (its counts are sums over many workgroups), and 2^17 reads of one base"""
    torch = torch_mod
    rng = np.random.default_rng(6)
    for lens in ([50, 20_000_000, 0, 1000], [1] * (1 << 17)):
        offsets = np.zeros(len(lens) + 1, np.uint64)
        offsets[1:] = np.cumsum(lens)
        total = int(offsets[-1])
        bases = ACGT[rng.integers(0, 4, size=total)]
        sup = pattern_support(rng, total, np.array([0, 1, 2, 9]))
        _, ns, _ = want_apply(bases, offsets, sup)
        big = int(ns.max())
        settings = ((1, 0), (2, 0), (1, big - 1), (1, big)) if len(lens) == 4 else ((1, 0), (1, 1), (2, 0))
        for ms, mc in settings:
            same(apply_device(torch, ctx, bases, offsets, sup, ms, mc), want_apply(bases, offsets, sup, ms, mc), (len(lens), ms, mc))
        same(apply_host(ctx, bases, offsets, sup, 1, 0), want_apply(bases, offsets, sup, 1, 0), (len(lens), "host"))


# ---- 5. a synthetic profile; argument errors ------------------------------------------------------------------------------------

def test_correct_synthetic_profile(torch_mod, ctx, oracle, make_counter):
    """coverage comes from the profile array alone: a made-up one (solid entries at random places, also where no window of the
    read starts) decides which bases are looked at; the probes still go to the real table"""
    from kmertools_amd import device
    from kmertools_amd.device import to_csr
    k = 17
    seqs = corner_batch(900, k)
    bases, offsets = to_csr(seqs)
    table = Table.of_reads(oracle, bases, offsets, k)
    ctr = make_counter(k, max(1 << 16, 2 * len(table.keys)))
    ctr.add_pairs_host(table.keys, table.counts)
    rng = np.random.default_rng(9)
    total = int(offsets[-1])
    real = want_profile(oracle, bases, offsets, k, table)
    for fake in (np.where(rng.random(total) < 0.03, 5, NO).astype(np.uint32),
                 np.where(rng.random(total) < 0.5, rng.integers(0, 9, size=total), NO).astype(np.uint32),
                 np.full(total, NO, np.uint32), np.full(total, 3, np.uint32)):
        for lo, hi in ((2, U32_MAX), (3, 6)):
            want = want_support(oracle, bases, offsets, k, table, fake, lo, hi)
            if (fake == NO).all() and hi == U32_MAX:  # (with (3, 6) the real profile covers next to nothing either)
                assert want.any() and not np.array_equal(want, want_support(oracle, bases, offsets, k, table, real, lo, hi))
            got, guard = support_device(torch_mod, ctr, bases, offsets, fake, lo, hi)
            assert guard == 0 and np.array_equal(got, want), (lo, hi, "device", np.flatnonzero(got != want)[:5])
            got, guard = support_host(ctr, bases, offsets, fake, lo, hi)
            assert guard == 0 and np.array_equal(got, want), (lo, hi, "host")
    ctr.close()


def test_correct_errors(torch_mod, ctx, make_counter):
    torch = torch_mod
    from kmertools_amd import device
    from kmertools_amd._lib import KT_ERR_ARG, KT_MEM_DEVICE, KT_MEM_HOST, lib
    L = lib()
    k = 21
    ctr = make_counter(k, 1 << 16)
    bases = np.frombuffer(b"ACGTACGTACGTACGTACGTACGTACGTACGTACGTTTGACCA", np.uint8).copy()
    offsets = np.array([0, 20, len(bases)], np.uint64)
    ctr.add_reads_host(bases, offsets)
    total = len(bases)
    prof = np.full(total, NO, np.uint32)
    sup = np.full(total, 0x01020300, np.uint32)
    out = np.full(total, 0x5A, np.uint8)
    ns = np.full(2, 77, np.uint32)
    na = np.full(2, 77, np.uint32)
    p = lambda a: a.ctypes.data if a is not None else None

    def support(h=ctr._h, b=bases, o=offsets, n=2, pr=prof, lo=2, hi=U32_MAX, s=sup, mem=KT_MEM_HOST, parts=1, part=0):
        return L.kt_ctr_correct_support(h, p(b), p(o), n, p(pr), lo, hi, p(s), mem, parts, part)

    def apply(c=ctx._h, b=bases, o=offsets, n=2, s=sup, ms=1, mc=0, ob=out, a=ns, m=na, mem=KT_MEM_HOST):
        return L.kt_correct_apply(c, p(b), p(o), n, p(s), ms, mc, p(ob), p(a), p(m), mem)

    for kw in (dict(h=None), dict(lo=0), dict(lo=0, hi=0), dict(lo=6, hi=5), dict(parts=2, part=2), dict(parts=0), dict(mem=7),
               dict(o=None), dict(pr=None), dict(s=None), dict(b=None)):
        assert support(**kw) == KT_ERR_ARG, kw
        assert L.kt_last_error(), kw
        assert (sup == 0x01020300).all(), kw
    assert support(o=None, pr=None, s=None, b=None, n=0) == 0  # no reads: nothing to check
    for kw in (dict(c=None), dict(ms=0), dict(ms=256), dict(mem=7), dict(o=None), dict(s=None), dict(b=None)):
        assert apply(**kw) == KT_ERR_ARG, kw
        assert L.kt_last_error(), kw
        assert (out == 0x5A).all() and (ns == 77).all() and (na == 77).all(), kw
    assert apply(o=None, s=None, b=None, n=0) == 0
    # a read of 2^32 bases: refused from the offsets alone, host and device
    big = np.array([0, 5, 5 + (1 << 32)], np.uint64)
    assert apply(o=big) == KT_ERR_ARG and b"2^32" in L.kt_last_error()
    db = torch.from_numpy(bases).cuda()
    dbig = torch.from_numpy(big.astype(np.int64)).cuda()
    dn = torch.zeros(total, dtype=torch.int32, device="cuda")
    assert L.kt_correct_apply(ctx._h, db.data_ptr(), dbig.data_ptr(), 2, dn.data_ptr(), 1, 0, None, dn.data_ptr(), None,
                              KT_MEM_DEVICE) == KT_ERR_ARG
    assert b"2^32" in L.kt_last_error()
    assert (out == 0x5A).all() and (ns == 77).all()
    # the calls themselves work on this input, and support is added into
    assert support() == 0 and apply() == 0
    assert (sup >= 0x01020300).all() and out[:total].tobytes().isalpha() and ns.sum() + na.sum() > 0
    ctr.close()
    sh = device.Sharded(ctx, k, 1 << 16, 1 << 16, 2, 0, ("host", lambda s, r, n: 1), connect=False)
    assert L.kt_ctr_correct_support(sh.table._h, p(bases), p(offsets), 2, p(prof), 2, U32_MAX, p(sup), KT_MEM_HOST, 1, 0) == KT_ERR_ARG
    assert b"shard" in L.kt_last_error()
    sh.close()


# ---- 6. shifted views and fenced outputs ------------------------------------------------------------------------------------------

def test_correct_shifted_views(torch_mod, ctx, oracle, make_counter):
    """every array at an address that is not the allocation's own (bases at byte shifts 1..3, the others at element shifts),
    guard words before and after every output; support prefilled: the call adds, and writes nowhere else"""
    torch = torch_mod
    from kmertools_amd import device
    from kmertools_amd.device import to_csr
    k = 15
    seqs = corner_batch(1100, k)
    bases, offsets = to_csr(seqs)
    n, total = len(seqs), int(offsets[-1])
    table = Table.of_reads(oracle, bases, offsets, k)
    ctr = make_counter(k, max(1 << 16, 2 * len(table.keys)))
    ctr.add_pairs_host(table.keys, table.counts)
    prof = want_profile(oracle, bases, offsets, k, table)
    want = want_support(oracle, bases, offsets, k, table, prof, 2, U32_MAX)
    wout, wns, wna = want_apply(bases, offsets, want, 1, 2)
    G = 8  # guard elements on either side
    fill = np.uint32(0x40404040)  # (bytes of 64: adding at most k = 15 to one never carries)

    def shifted(arr, shift, fill_value):
        """a device buffer of guards with arr at element `shift` + G -> (buffer, view)"""
        t = torch.from_numpy(np.ascontiguousarray(arr).view({1: np.uint8, 4: np.int32, 8: np.int64}[arr.dtype.itemsize]))
        buf = torch.full((len(arr) + 2 * G + shift,), fill_value, dtype=t.dtype, device="cuda")
        view = buf[G + shift:G + shift + len(arr)]
        view.copy_(t)
        return buf, view

    def fenced(buf, view_len, shift, fill_value):
        h = buf.cpu().numpy()
        return (h[:G + shift] == fill_value).all() and (h[G + shift + view_len:] == fill_value).all()

    for shift in (1, 2, 3):
        _, vb = shifted(bases, shift, 0x4E)
        _, vo = shifted(offsets, shift, -1)
        _, vp = shifted(prof, shift, -1)
        sb, vs = shifted(np.full(total, fill, np.uint32), shift % 2 + 1, 0x77777777)
        ctr.correct_support(vb, vo, n, vp, 2, U32_MAX, vs)
        torch.cuda.synchronize()
        assert fenced(sb, total, shift % 2 + 1, 0x77777777), shift
        assert np.array_equal(u32(vs), want + fill), shift
        _, vsup = shifted(want, shift, 0x01010101)  # (guards that would decide something if they were read as support)
        ob, vout = shifted(np.full(total, 0x5A, np.uint8), (shift + 1) % 4, 0x6B)
        nb, vns = shifted(np.full(n, 9, np.uint32), shift, 0x33333333)
        ab, vna = shifted(np.full(n, 9, np.uint32), 3 - shift, 0x33333333)
        ctx.correct_apply(vb, vo, n, vsup, 1, 2, vout, vns, vna)
        torch.cuda.synchronize()
        assert fenced(ob, total, (shift + 1) % 4, 0x6B) and fenced(nb, n, shift, 0x33333333) and fenced(ab, n, 3 - shift, 0x33333333)
        same((vout.cpu().numpy(), u32(vns), u32(vna)), (wout, wns, wna), ("views", shift))
    ctr.close()


# ---- 7. it repairs --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", [21, 31])
def test_correct_repairs_planted_errors(torch_mod, ctx, oracle, make_counter, k):
    """a random 20 kb genome, both strands, 30 x = 4000 reads of 150 bases, 1 % substitutions, min_count 3.  The GPU equals the
    restatement exactly; and the restatement itself repairs at least 0.85 of the planted errors and changes no more than
    0.001 of the true bases (conditions on the input: the test cannot pass on one where nothing gets corrected)"""
    from kmertools_amd import device
    from kmertools_amd.device import to_csr
    rng = np.random.default_rng(2100 + k)
    genome = ACGT[rng.integers(0, 4, size=20_000)]
    n, L = 4000, 150
    truth, seqs = [], []
    for _ in range(n):
        a = int(rng.integers(0, len(genome) - L + 1))
        s = genome[a:a + L].copy()
        if rng.random() < 0.5:
            s = ACGT[rc(s)]
        truth.append(s.copy())
        for at in np.flatnonzero(rng.random(L) < 0.01):
            sub(s, int(at), rng)
        seqs.append(s.tobytes())
    bases, offsets = to_csr(seqs)
    true = np.concatenate(truth)
    planted = bases != true
    table = Table.of_reads(oracle, bases, offsets, k)
    prof = want_profile(oracle, bases, offsets, k, table)
    want = want_support(oracle, bases, offsets, k, table, prof, 3, U32_MAX)
    wout, wns, wna = want_apply(bases, offsets, want)
    repaired = int((planted & (wout == true)).sum())
    spoiled = int((~planted & (wout != true)).sum())
    print("k=%d planted %d repaired %d (%.3f) spoiled %d ambiguous %d" % (k, planted.sum(), repaired, repaired / planted.sum(),
                                                                         spoiled, wna.sum()))
    assert planted.sum() > 5000 and repaired >= 0.85 * planted.sum() and spoiled <= 0.001 * (~planted).sum()
    ctr = make_counter(k, max(1 << 16, 2 * len(table.keys)))
    ctr.add_reads_host(bases, offsets)
    got, guard = support_device(torch_mod, ctr, bases, offsets, prof, 3, U32_MAX)
    assert guard == 0 and np.array_equal(got, want)
    same(apply_device(torch_mod, ctx, bases, offsets, got), (wout, wns, wna), k)
    same(ctr.correct_host(bases, offsets, 3), (wout, wns, wna), (k, "correct_host"))
    ctr.close()


# ---- 8. full size -----------------------------------------------------------------------------------------------------------------

def test_correct_full_size_k31(torch_mod, ctx, oracle, make_counter):
    """10 M x 150 bp at k = 31, sampled from a genome with sequencing errors: invariants over all of it (covered bases have no
    support, no byte above k, out_bases differs from bases only at single bases and holds the supported nucleotide there), and
    20 000 sampled reads agree with the restatement over kt_ctr_lookup's counts"""
    torch = torch_mod
    from kmertools_amd import device
    k, n, L = 31, 10_000_000, 150
    kpr = L - k + 1
    bases = torch.empty(n * L, dtype=torch.uint8, device="cuda")
    offsets = torch.empty(n + 1, dtype=torch.int64, device="cuda")
    ctx.synth_reads(0xF117E5, n, L, bases, offsets, noise=True, genome_len=20_000_000)
    ctr = make_counter(k, int(1.9 * n * kpr))
    ctr.add_reads(bases, offsets, n)
    lo, hi = 2, U32_MAX
    prof = torch.full((n * L,), -1, dtype=torch.int32, device="cuda")
    ctr.profile(bases, offsets, n, prof)
    sup = torch.zeros(n * L, dtype=torch.int32, device="cuda")
    ctr.correct_support(bases, offsets, n, prof, lo, hi, sup)
    out = torch.empty_like(bases)
    ns = torch.empty(n, dtype=torch.int32, device="cuda")
    na = torch.empty(n, dtype=torch.int32, device="cuda")
    ctx.correct_apply(bases, offsets, n, sup, 1, 0, out, ns, na)
    torch.cuda.synchronize()
    # invariants over all of it
    for x in range(4):
        assert int(((sup >> (8 * x)) & 255).max()) <= k
    solid = (prof != -1) & (prof >= lo)  # (a count is below 2^31 here)
    c = torch.cumsum(solid.view(n, L).to(torch.int32), dim=1)
    c = torch.nn.functional.pad(c, (1, 0))
    g = torch.arange(L, device="cuda")
    covered = (c[:, g + 1] - c[:, torch.clamp(g - k + 1, min=0)]) > 0
    del c, solid
    s2 = sup.view(n, L)
    assert not bool((s2[covered] != 0).any()) and bool(covered.any()) and not bool(covered.all())
    del covered
    cands = sum((((sup >> (8 * x)) & 255) >= 1).to(torch.int8) for x in range(4))
    changed = out != bases
    assert bool(changed.any()) and not bool((changed & (cands != 1)).any())
    assert int((cands == 1).view(n, L).sum(dim=1).to(torch.int32).ne(ns).sum()) == 0
    assert int((cands >= 2).view(n, L).sum(dim=1).to(torch.int32).ne(na).sum()) == 0
    del cands, changed
    # sampled reads against the restatement
    rng = np.random.default_rng(7)
    sample = np.sort(rng.choice(n, size=20000, replace=False))
    idx = torch.from_numpy(sample).cuda()
    hb = bases.view(n, L)[idx].cpu().numpy().reshape(-1)
    hoff = (np.arange(len(sample) + 1, dtype=np.uint64) * np.uint64(L)).astype(np.uint64)
    hprof = prof.view(n, L)[idx].cpu().numpy().view(np.uint32).reshape(-1)
    hsup = s2[idx].cpu().numpy().view(np.uint32).reshape(-1)
    hout = out.view(n, L)[idx].cpu().numpy().reshape(-1)

    class Lookup:
        def count(self, keys):
            return ctr.lookup_host(keys)

    want = want_support(oracle, hb, hoff, k, Lookup(), hprof, lo, hi)
    assert want.any() and np.array_equal(hsup, want), np.flatnonzero(hsup != want)[:5]
    wout, wns, wna = want_apply(hb, hoff, want)
    assert np.array_equal(hout, wout) and np.array_equal(u32(ns[idx]), wns) and np.array_equal(u32(na[idx]), wna)
    ctr.close()
    del bases, offsets, prof, sup, out
    torch.cuda.empty_cache()


# ---- 9. the CLI end to end ----------------------------------------------------------------------------------------------------------

def run(*args, env=None, cwd=None):
    return subprocess.run([CLI, *map(str, args)], capture_output=True, timeout=600, env=env, cwd=cwd)


def parse_records(data):
    """(header without '>' / '@', sequence, quality or None): what the reader keeps with keep_records"""
    ws = b" \t\r\n\v\f"
    lines = data.split(b"\n")
    out = []
    i = 0
    if data[:1] == b">":
        while i < len(lines):
            h = lines[i].rstrip(ws)
            i += 1
            if not h:
                continue
            seq = []
            while i < len(lines) and not lines[i].startswith(b">"):
                seq.append(lines[i].rstrip(ws))
                i += 1
            out.append((h[1:], b"".join(seq), None))
    else:
        while i < len(lines):
            h = lines[i].rstrip(ws)
            if not h:
                i += 1
                continue
            out.append((h[1:], lines[i + 1].rstrip(ws), lines[i + 3].rstrip(ws)))
            i += 4
    return out


def read_file(path):
    data = open(path, "rb").read()
    return gzip.decompress(data) if str(path).endswith(".gz") else data


def want_corrected(oracle, recs, count_recs, k, lo=2, hi=U32_MAX, min_support=1, max_corrections=0):
    """-> (the output file, the --stats file)"""
    table = Table.of_reads(oracle, *oracle.to_csr([s for _, s, _ in count_recs]), k)
    bases, offsets = oracle.to_csr([s for _, s, _ in recs])
    prof = want_profile(oracle, bases, offsets, k, table)
    sup = want_support(oracle, bases, offsets, k, table, prof, lo, hi)
    out, ns, na = want_apply(bases, offsets, sup, min_support, max_corrections)
    text = []
    for i, (hdr, seq, qual) in enumerate(recs):
        s = out[int(offsets[i]):int(offsets[i + 1])].tobytes()
        text.append(b">" + hdr + b"\n" + s + b"\n" if qual is None else b"@" + hdr + b"\n" + s + b"\n+\n" + qual + b"\n")
    over = (ns > max_corrections) if max_corrections else np.zeros(len(ns), bool)
    stats = [("reads", len(recs)), ("bases", int(offsets[-1])), ("reads_corrected", int(((ns > 0) & ~over).sum())),
             ("bases_corrected", int(ns[~over].sum())), ("positions_ambiguous", int(na.sum())), ("reads_over_limit", int(over.sum()))]
    return b"".join(text), "".join("%s\t%d\n" % kv for kv in stats).encode()


def noisy_fastq(seed, n):
    """reads sampled from a small genome at about 25 x with substitutions, N and lower case, multi-word headers, some shorter than k"""
    rng = np.random.default_rng(seed)
    genome = ACGT[rng.integers(0, 4, size=20000)]
    quals = np.frombuffer(b"!#+5?I", np.uint8)
    out = []
    for i in range(n):
        L = int(rng.integers(0, 220)) if i % 10 == 0 else int(rng.integers(60, 220))
        a = int(rng.integers(0, len(genome) - L))
        s = genome[a:a + L].copy()
        err = rng.random(L) < 0.01
        s[err] = ACGT[rng.integers(0, 4, size=int(err.sum()))]
        if L > 50 and rng.random() < 0.1:
            s[int(rng.integers(0, L))] = ord("N")
        if L > 50 and rng.random() < 0.1:
            b = int(rng.integers(0, L - 20))
            s[b:b + 20] = np.frombuffer(bytes(s[b:b + 20]).lower(), np.uint8)
        q = quals[rng.integers(0, len(quals), size=L)].tobytes()
        out.append(b"@read%d lane=%d  sample x\n%s\n+\n%s\n" % (i, i % 5, s.tobytes(), q))
    return b"".join(out)


@pytest.fixture(scope="module")
def cli_bin():
    if not os.path.exists(CLI):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "kmertools_amd", "csrc"), "-j4"], stdout=subprocess.DEVNULL)
    return CLI


def test_correct_cli_golden_inputs(cli_bin, oracle, tmp_path):
    for name in ("reads.fq", "reads.fa", "reads.fq.gz"):
        src = os.path.join(GOLDEN, name)
        recs = parse_records(read_file(src))
        for extra, kw in (((), {}), (("--min-count", "1"), dict(lo=1)), (("--min-count", "3", "--min-support", "2"), dict(lo=3, min_support=2))):
            out = tmp_path / ("fixed_" + name.replace(".gz", ""))
            r = run("correct", "-i", src, "-o", out, "-k", "15", *extra)
            assert r.returncode == 0, r.stderr
            want, _ = want_corrected(oracle, recs, recs, 15, **kw)
            assert out.read_bytes() == want, (name, extra)
            assert len(parse_records(out.read_bytes())) == len(recs)


def test_correct_cli_noisy_fastq(cli_bin, oracle, tmp_path):
    fq = tmp_path / "noisy.fastq"
    fq.write_bytes(noisy_fastq(11, 3000))
    recs = parse_records(fq.read_bytes())
    k = 21
    cases = [((), {}),
             (("--min-count", "3"), dict(lo=3)),
             (("--min-count", "3", "--max-count", "25"), dict(lo=3, hi=25)),  # (the coverage is about 21 x)
             (("--min-support", "3"), dict(min_support=3)),
             (("--max-corrections", "1"), dict(max_corrections=1)),
             (("--min-count", "3", "--max-corrections", "2", "--min-support", "2"), dict(lo=3, max_corrections=2, min_support=2))]
    seen = {}
    for extra, kw in cases:
        out, st = tmp_path / "fixed.fastq", tmp_path / "fixed.stats"
        r = run("correct", "-i", fq, "-o", out, "-k", k, "--stats", st, *extra)
        assert r.returncode == 0, r.stderr
        want, want_stats = want_corrected(oracle, recs, recs, k, **kw)
        got = out.read_bytes()
        assert got == want, extra
        assert st.read_bytes() == want_stats, (extra, st.read_bytes(), want_stats)
        fixed = parse_records(got)
        assert len(fixed) == len(recs) and all(a[0] == b[0] and a[2] == b[2] and len(a[1]) == len(b[1]) for a, b in zip(fixed, recs))
        assert sum(a[1] != b[1] for a, b in zip(fixed, recs)) > 100, extra  # reads really repaired
        seen[extra] = got
    assert len(set(seen.values())) == len(cases)  # every setting made a difference
    stats = dict(line.split(b"\t") for line in want_corrected(oracle, recs, recs, k, max_corrections=1)[1].splitlines())
    assert int(stats[b"reads_over_limit"]) > 0 and int(stats[b"reads_corrected"]) > 0
    # out-of-core passes: the same bytes as the single pass
    size = fq.stat().st_size
    want_slots = size // 2 + size // 2 // 10 * 9
    env = dict(os.environ, KT_CTR_MAX_SLOTS=str(want_slots // 4 + 1), KT_CLI_TIMING="1")
    for extra, kw in (cases[0], cases[2], cases[5]):
        out, st = tmp_path / "fixed_passes.fastq", tmp_path / "fixed_passes.stats"
        r = run("correct", "-i", fq, "-o", out, "-k", k, "--stats", st, *extra, env=env, cwd=tmp_path)
        assert r.returncode == 0, r.stderr
        assert int(r.stderr.decode().split(" pass(es)")[0].split()[-1]) >= 4
        want, want_stats = want_corrected(oracle, recs, recs, k, **kw)
        assert out.read_bytes() == want and st.read_bytes() == want_stats, extra
    assert not (tmp_path / "kmers.counts").exists() and not (tmp_path / "kmers.histo").exists()


def test_correct_cli_alt_input_and_fasta(cli_bin, oracle, tmp_path):
    """-a: the table is counted from another file (a FASTA of every other read); FASTA in (sequences over two lines), FASTA
    out (one line)"""
    recs = parse_records(noisy_fastq(12, 2000))
    fa = tmp_path / "reads.fa"
    fa.write_bytes(b"".join(b">" + h + b"\n" + s[:40] + b"\n" + s[40:] + b"\n" for h, s, _ in recs))
    alt = tmp_path / "alt.fasta"
    alt.write_bytes(b"".join(b">a%d\n%s\n" % (i, s) for i, (_, s, _) in enumerate(recs[::2])))
    fa_recs = [(h, s, None) for h, s, _ in recs]
    alt_recs = [(b"", s, None) for _, s, _ in recs[::2]]
    k = 25
    for extra, kw in ((("--min-count", "1"), dict(lo=1)), ((), {}), (("--max-corrections", "3"), dict(max_corrections=3))):
        out = tmp_path / "fixed.fa"
        r = run("correct", "-i", fa, "-a", alt, "-o", out, "-k", k, *extra)
        assert r.returncode == 0, r.stderr
        want, _ = want_corrected(oracle, fa_recs, alt_recs, k, **kw)
        assert out.read_bytes() == want, extra
        assert out.read_bytes() != b"".join(b">" + h + b"\n" + s + b"\n" for h, s, _ in fa_recs)
