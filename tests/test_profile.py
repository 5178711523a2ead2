"""The k-mer count profile: kt_ctr_profile (the table's count of the k-mer that starts at every base of a batch) and
kt_profile_stats (per read: k-mers, present ones, min, median = element n // 2, max, sum) against a restatement over the
oracle's k-mers and table and a few lines of numpy - host and device mode, every table form, hash partitions, short reads,
long sequences on both sides of every length threshold of the selection, the adversarial inputs of a selection, synthetic
arrays with no table at all, NULL outputs, argument errors, shifted views with fenced guards, full size; and
`kmertools profile` end to end, byte for byte against the restated files.  Every comparison is exact."""
import gzip
import os
import re
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "kmertools_amd", "bin", "kmertools")
GOLDEN = os.path.join(ROOT, "tests", "golden")
NO = 0xFFFFFFFF  # KT_NO_KMER
# the length thresholds of kt_profile_stats (kt_profile.hip): a sequence of at most SHORT_MAX bases is selected from a
# wave's registers, one of at most MID_MAX from its LDS, a longer one by four histogram passes over chunks of CHUNK entries
SHORT_MAX, MID_MAX, CHUNK = 256, 2048, 16384
NAMES = ("n_kmers", "n_present", "min", "median", "max", "sum")


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


# ---- the restatement ----------------------------------------------------------------------------------------------------

class Table:
    """a table as sorted (canonical key, count) arrays: count of a k-mer, 0 when absent"""

    def __init__(self, keys, counts):
        order = np.argsort(keys)
        self.keys, self.counts = np.asarray(keys, np.uint64)[order], np.asarray(counts, np.uint32)[order]

    @classmethod
    def of_reads(cls, oracle, bases, offsets, k, threads=1):
        return cls(*oracle.count_reads(bases, offsets, k, 1, threads))

    def count(self, keys):
        if not len(self.keys):
            return np.zeros(len(keys), np.uint32)
        i = np.minimum(np.searchsorted(self.keys, keys), len(self.keys) - 1)
        return np.where(self.keys[i] == keys, self.counts[i], 0).astype(np.uint32)


def want_profile(oracle, seqs, k, table, fill=NO, keep=None):
    """the count at each valid window start, `fill` elsewhere (keep(keys) -> bool: only those k-mers are written)"""
    offsets = np.zeros(len(seqs) + 1, np.uint64)
    offsets[1:] = np.cumsum([len(s) for s in seqs], dtype=np.uint64)
    prof = np.full(int(offsets[-1]), fill, np.uint32)
    for s, o in zip(seqs, offsets[:-1]):
        f, r, end = oracle.kmers(s, k)
        if not len(f):
            continue
        keys = np.minimum(f, r)
        at = (int(o) + end - np.uint64(k - 1)).astype(np.int64)
        cnt = np.minimum(table.count(keys), 0xFFFFFFFE).astype(np.uint32)
        if keep is not None:
            m = keep(keys)
            at, cnt = at[m], cnt[m]
        prof[at] = cnt
    return prof


def want_stats(prof, offsets):
    n = len(offsets) - 1
    out = {name: np.zeros(n, np.uint64 if name == "sum" else np.uint32) for name in NAMES}
    for i in range(n):
        v = prof[int(offsets[i]):int(offsets[i + 1])]
        v = v[v != NO]
        if not len(v):
            continue
        out["n_kmers"][i] = len(v)
        out["n_present"][i] = int((v >= 1).sum())
        out["min"][i] = v.min()
        out["median"][i] = np.sort(v)[len(v) // 2]
        out["max"][i] = v.max()
        out["sum"][i] = sum(int(x) for x in v) if len(v) < 4096 else int(v.astype(np.uint64).sum(dtype=np.uint64))
    return out


def mixed_reads(seed, n, k):
    """random reads with N runs and lower case, repeated so that counts 1..5 and more occur, reads shorter than k, empty
    reads, reads of exactly k, reads of 10 kbases and more (straddling segment edges; one of more than 3 segments)"""
    rng = np.random.default_rng(seed)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    seqs = []
    for L in rng.integers(0, 400, size=n):
        s = acgt[rng.integers(0, 4, size=int(L))].copy()
        if L > 40 and rng.random() < 0.3:
            a = int(rng.integers(0, L - 20))
            s[a:a + int(rng.integers(1, 20))] = ord("N")
        if L > 40 and rng.random() < 0.2:
            a = int(rng.integers(0, L - 30))
            s[a:a + 30] = np.frombuffer(bytes(s[a:a + 30]).lower(), np.uint8)
        seqs.append(s.tobytes())
    seqs += [b"", b"ACGTACG", b"acgtn" * 2, b"A" * (k - 1), b"", b"C" * k, acgt[rng.integers(0, 4, size=k)].tobytes()]
    for L in (10_000, 17_321, 3 * 8192 + 1000):
        s = acgt[rng.integers(0, 4, size=L)].copy()
        s[L // 3:L // 3 + 5] = ord("N")
        seqs.append(s.tobytes())
    seqs += seqs[: n // 4] * 2 + seqs[: n // 10] * 2 + [b"A" * 2500]
    order = rng.permutation(len(seqs))
    return [seqs[i] for i in order]


def tiny_reads(seed, n, k, donors):
    """n short reads (20 bases, k + 1 when that is more): more than 256 of them per 8192-base segment"""
    rng = np.random.default_rng(seed)
    L = max(20, k + 1)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    long_ = [d for d in donors if len(d) >= L + 1]
    out = []
    for i in range(n):
        Li = L + (i % 3 == 0)  # both parities of the number of k-mers
        if i % 2 and long_:
            d = long_[int(rng.integers(0, len(long_)))]
            a = int(rng.integers(0, len(d) - Li + 1))
            out.append(d[a:a + Li])
        else:
            out.append(acgt[rng.integers(0, 4, size=Li)].tobytes())
    return out


def u32(t):
    return t.cpu().numpy().view(np.uint32)


def dev(torch, a):
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint64:
        a = a.view(np.int64)
    elif a.dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(a if a.size else np.zeros(1, a.dtype)).cuda()


def profile_device(torch, ctr, bases, offsets, fill=NO, n_parts=1, part=0, into=None):
    """the device-mode call into an array of `fill` with a guard element behind it -> (array, guard)"""
    total = int(offsets[-1])
    prof = into if into is not None else dev(torch, np.full(total + 1, fill, np.uint32))
    ctr.profile(dev(torch, bases), dev(torch, offsets), len(offsets) - 1, prof, n_parts=n_parts, part=part)
    torch.cuda.synchronize()
    got = u32(prof)
    return got[:total], got[total]


def profile_host(ctr, bases, offsets, fill=NO, n_parts=1, part=0, into=None):
    from kmertools_amd._lib import KT_MEM_HOST
    total = int(offsets[-1])
    prof = into if into is not None else np.full(total + 1, fill, np.uint32)
    ctr.profile(bases if bases.size else np.zeros(1, np.uint8), offsets, len(offsets) - 1, prof, KT_MEM_HOST, n_parts, part)
    return prof[:total], prof[total]


def stats_device(torch, ctx, prof, offsets, skip=()):
    """the device-mode call into arrays primed with a pattern (the outputs are overwritten, not combined into)"""
    n = len(offsets) - 1
    outs = {}
    for name in NAMES:
        if name in skip:
            outs[name] = None
        elif name == "sum":
            outs[name] = torch.full((max(n, 1),), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device="cuda")
        else:
            outs[name] = torch.full((max(n, 1),), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    ctx.profile_stats(dev(torch, prof), dev(torch, offsets), n, outs["n_kmers"], outs["n_present"], outs["min"], outs["median"],
                      outs["max"], outs["sum"])
    torch.cuda.synchronize()
    return {name: (None if t is None else t.cpu().numpy().view(np.uint64 if name == "sum" else np.uint32)[:n])
            for name, t in outs.items()}


def assert_stats(got, want, tag):
    for name in NAMES:
        if got[name] is None:
            continue
        bad = np.flatnonzero(got[name] != want[name])
        assert not len(bad), (tag, name, bad[:5], got[name][bad[:5]], want[name][bad[:5]])


def check_stats(torch, ctx, prof, offsets, tag):
    want = want_stats(prof, offsets)
    assert_stats(ctx.profile_stats_host(prof, offsets), want, (tag, "host"))
    assert_stats(stats_device(torch, ctx, prof, offsets), want, (tag, "device"))
    return want


# ---- 1. the profile against the restatement ----------------------------------------------------------------------------------

@pytest.mark.parametrize("k", [11, 15, 21, 31])
def test_profile_against_restatement(torch_mod, ctx, oracle, k):
    from kmertools_amd import device
    from kmertools_amd.device import to_csr
    seqs = mixed_reads(300 + k, 1200, k)
    tiny = tiny_reads(400 + k, 4000, k, seqs)
    assert any(len(s) > 3 * 8192 for s in seqs) and any(len(s) == k for s in seqs) and any(len(s) == 0 for s in seqs)
    table = Table.of_reads(oracle, *to_csr(seqs[::2] + tiny[::2]), k)  # (half of the reads: absent k-mers occur)
    assert (table.counts >= 3).any() and (table.counts == 1).any()
    ctr = device.Counter(ctx, k, max(1 << 16, 2 * len(table.keys)))
    ctr.add_pairs_host(table.keys, table.counts)
    for batch, tag in ((seqs, "mixed"), (tiny, "tiny reads")):
        bases, offsets = to_csr(batch)
        for fill in (NO, 0x12345678):  # "written with the sentinel" is not "not written"
            want = want_profile(oracle, batch, k, table, fill)
            assert (want == 0).any() and (want == fill).any() and ((want != fill) & (want > 1)).any()
            got, guard = profile_device(torch_mod, ctr, bases, offsets, fill)
            assert guard == fill and np.array_equal(got, want), (tag, k, hex(fill), "device", np.flatnonzero(got != want)[:5])
            got, guard = profile_host(ctr, bases, offsets, fill)
            assert guard == fill and np.array_equal(got, want), (tag, k, hex(fill), "host", np.flatnonzero(got != want)[:5])
        assert np.array_equal(ctr.profile_host(bases, offsets), want_profile(oracle, batch, k, table))
        check_stats(torch_mod, ctx, want_profile(oracle, batch, k, table), offsets, (tag, k))
    # no reads, and reads with no bases at all
    assert len(ctr.profile_host(np.zeros(0, np.uint8), np.zeros(1, np.uint64))) == 0
    assert len(ctr.profile_host(np.zeros(0, np.uint8), np.zeros(4, np.uint64))) == 0
    st = ctx.profile_stats_host(np.zeros(0, np.uint32), np.zeros(4, np.uint64))
    assert all(len(st[name]) == 3 and not st[name].any() for name in NAMES)
    ctr.close()


# ---- 2. every table form -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", [13, 21])
def test_profile_every_table_form(torch_mod, ctx, oracle, monkeypatch, k):
    torch = torch_mod
    from kmertools_amd import device
    from kmertools_amd.device import to_csr
    seqs = mixed_reads(500 + k, 1500, k)
    bases, offsets = to_csr(seqs)
    table = Table.of_reads(oracle, bases, offsets, k)
    cap = max(1 << 16, 2 * len(table.keys))
    want = want_profile(oracle, seqs, k, table)
    forms = []

    def check(ctr, tag):
        assert ctr.size() == len(table.keys), tag
        got, guard = profile_host(ctr, bases, offsets)
        assert guard == NO and np.array_equal(got, want), (tag, k, "host")
        got, guard = profile_device(torch, ctr, bases, offsets)
        assert guard == NO and np.array_equal(got, want), (tag, k, "device")
        forms.append(tag)

    ctr = device.Counter(ctx, k, cap)
    ctr.add_reads_host(bases, offsets)
    check(ctr, "probing")
    ctr.close()
    ctr = device.Counter(ctx, k, cap)
    ctr.add_pairs_host(table.keys, table.counts)
    check(ctr, "add_pairs")
    ctr.close()
    monkeypatch.setenv("KT_BULK", "1")
    monkeypatch.setenv("KT_BULK_MIN_BASES", "0")
    ctr = device.Counter(ctx, k, cap)
    ctr.add_reads_host(bases, offsets)
    check(ctr, "bulk")
    ctr.close()
    m = len(table.keys) + 9
    xk = torch.zeros(m, dtype=torch.int64, device="cuda")
    xc = torch.zeros(m, dtype=torch.int32, device="cuda")
    ctr = device.Counter(ctx, k, cap)
    ctr.export_target(xk, xc, m)
    ctr.add_reads(torch.from_numpy(bases).cuda(), torch.from_numpy(offsets.astype(np.int64)).cuda(), len(seqs))
    check(ctr, "export target")
    ctr.close()
    if k <= 15:
        ctr = device.Counter(ctx, k, 4 ** k)
        assert ctr.capacity() == 4 ** k
        ctr.add_reads_host(bases, offsets)
        check(ctr, "direct")
        ctr.close()
    assert len(forms) == (5 if k <= 15 else 4)


# ---- 3. hash partitions -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", [15, 31])
def test_profile_partitions_combine(torch_mod, ctx, oracle, k):
    torch = torch_mod
    from kmertools_amd import device
    from kmertools_amd.device import owner_of, to_csr
    seqs = mixed_reads(700 + k, 1000, k)
    bases, offsets = to_csr(seqs)
    table = Table.of_reads(oracle, bases, offsets, k)
    whole = want_profile(oracle, seqs, k, table)
    total = int(offsets[-1])
    for n_parts in (2, 3, 7):
        hp = np.full(total + 1, NO, np.uint32)
        dp = dev(torch, hp)
        sizes = 0
        for part in range(n_parts):
            ctr = device.Counter(ctx, k, max(1 << 16, 2 * len(table.keys)))
            ctr.add_reads_host(bases, offsets, n_parts, part)
            sizes += ctr.size()
            # a single part on its own: only that part's positions differ from the fill
            own = lambda keys: np.array([owner_of(int(x), n_parts) == part for x in keys], bool)
            if n_parts == 3 or part == 0:
                alone = want_profile(oracle, seqs, k, table, 0x0BADF00D, own)
                got, guard = profile_device(torch, ctr, bases, offsets, 0x0BADF00D, n_parts, part)
                assert guard == 0x0BADF00D and np.array_equal(got, alone), (k, n_parts, part)
                assert (alone == 0x0BADF00D).sum() > (whole == NO).sum()
            profile_host(ctr, bases, offsets, n_parts=n_parts, part=part, into=hp)
            profile_device(torch, ctr, bases, offsets, n_parts=n_parts, part=part, into=dp)
            ctr.close()
        assert sizes == len(table.keys)
        assert hp[total] == NO and np.array_equal(hp[:total], whole), (k, n_parts, "host")
        got = u32(dp)
        assert got[total] == NO and np.array_equal(got[:total], whole), (k, n_parts, "device")


# ---- 4. statistics on short reads ----------------------------------------------------------------------------------------------

def test_profile_stats_short_reads(torch_mod, ctx, oracle):
    from kmertools_amd import device
    from kmertools_amd.device import to_csr
    k = 21
    rng = np.random.default_rng(41)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    genome = acgt[rng.integers(0, 4, size=300_000)]
    repeat = acgt[rng.integers(0, 4, size=400)]
    for a in rng.integers(0, len(genome) - 400, size=60):
        genome[a:a + 400] = repeat  # a repeat family
    seqs = []
    for L in rng.integers(30, 301, size=20_000):
        a = int(rng.integers(0, len(genome) - L))
        s = genome[a:a + int(L)].copy()
        err = rng.random(int(L)) < 0.01
        s[err] = acgt[rng.integers(0, 4, size=int(err.sum()))]
        seqs.append(s.tobytes())
    seqs += [bytes(repeat[:300])] * 3000  # ... in the thousands
    lens = np.array([len(s) for s in seqs])
    assert ((lens - k + 1) % 2 == 0).any() and ((lens - k + 1) % 2 == 1).any() and lens.max() > SHORT_MAX > lens.min()
    bases, offsets = to_csr(seqs)
    table = Table.of_reads(oracle, bases, offsets, k)
    assert table.counts.max() > 3000 and np.median(table.counts) < 50
    ctr = device.Counter(ctx, k, 2 * len(table.keys))
    ctr.add_pairs_host(table.keys, table.counts)
    prof = want_profile(oracle, seqs, k, table)
    got, _ = profile_device(torch_mod, ctr, bases, offsets)
    assert np.array_equal(got, prof)
    want = check_stats(torch_mod, ctx, got, offsets, "short reads")
    assert (want["median"] > 1000).any() and (want["median"] < 50).any() and (want["min"] < want["median"]).any()
    # tiny reads, more than 256 of them per segment
    tiny = tiny_reads(43, 30_000, k, seqs)
    tb, to = to_csr(tiny)
    got, _ = profile_device(torch_mod, ctr, tb, to)
    assert np.array_equal(got, want_profile(oracle, tiny, k, table))
    check_stats(torch_mod, ctx, got, to, "tiny reads")
    ctr.close()


# ---- 5. statistics on long sequences -----------------------------------------------------------------------------------------

def test_profile_stats_long_sequences(torch_mod, ctx, oracle):
    from kmertools_amd import device
    from kmertools_amd.device import to_csr
    k = 21
    rng = np.random.default_rng(51)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    rand = lambda L: acgt[rng.integers(0, 4, size=L)].tobytes()
    # (sequence, how its k-mer at index j of n gets its count)
    half = lambda j, n: np.where(j < n // 2, 5, 9)
    cases = [(b"A" * 5000, lambda j, n: np.full(n, 1)),                  # all equal
             (b"C" * 5000, lambda j, n: np.full(n, 0x80000001)),         # ... with the top bit set
             (rand(70_000), half),                                        # two values, the median on the boundary (n even)
             (rand(70_001), half),                                        # ... n odd
             (rand(5000), lambda j, n: (rng.integers(0, 256, size=n) << 24) | 0x00ABCDEF),  # only the top byte differs
             (rand(5000), lambda j, n: 0x12345600 | rng.integers(0, 256, size=n)),          # only the bottom byte
             (b"N" * 6000, None),                                         # no k-mer
             (rand(3000), lambda j, n: np.where(j == 7, 0xFFFFFFFE, 3)),  # the largest count there is, once
             (rand(3000), lambda j, n: np.where(j % 2 == 0, 0xFFFFFFFE, 0xFFFFFFFD)),
             (rand(1_000_003), lambda j, n: rng.integers(1, 60, size=n)),
             (rand(4_200_000), lambda j, n: np.where(rng.random(n) < 0.01, rng.integers(1000, 1 << 31, size=n), rng.integers(0, 40, size=n)))]
    # one sequence on each side of each threshold (lengths in bases), and the same with an N in the middle
    for L in (SHORT_MAX - 1, SHORT_MAX, SHORT_MAX + 1, MID_MAX - 1, MID_MAX, MID_MAX + 1, CHUNK - 1, CHUNK, CHUNK + 1,
              2 * CHUNK, 2 * CHUNK + 1):
        cases.append((rand(L), lambda j, n: rng.integers(0, 1 << 32, size=n, dtype=np.uint64) >> rng.integers(0, 32, size=n, dtype=np.uint64)))
        s = bytearray(rand(L))
        s[L // 2] = ord("N")
        cases.append((bytes(s), lambda j, n: rng.integers(0, 300, size=n)))
    keys, counts = [], []
    for s, how in cases:
        f, r, _ = oracle.kmers(s, k)
        if how is None or not len(f):
            continue
        keys.append(np.minimum(f, r))
        counts.append(np.minimum(np.asarray(how(np.arange(len(f)), len(f)), np.uint64), 0xFFFFFFFE).astype(np.uint32))
    keys, first = np.unique(np.concatenate(keys), return_index=True)
    counts = np.concatenate(counts)[first]
    table = Table(keys[counts > 0], counts[counts > 0])  # (a k-mer given count 0 is an absent one)
    assert table.counts.max() == 0xFFFFFFFE
    ctr = device.Counter(ctx, k, 2 * len(keys))
    ctr.add_pairs_host(table.keys, table.counts)
    seqs = [s for s, _ in cases]
    bases, offsets = to_csr(seqs)
    prof = want_profile(oracle, seqs, k, table)
    got, guard = profile_device(torch_mod, ctr, bases, offsets)
    bad = np.flatnonzero(got != prof)
    assert guard == NO and not len(bad), (len(bad), bad[:5], got[bad[:5]], prof[bad[:5]], np.searchsorted(offsets, bad[:5], "right") - 1)
    want = check_stats(torch_mod, ctx, got, offsets, "long sequences")
    assert want["median"][0] == 1 and want["median"][1] == 0x80000001 and want["median"][2] == 9 and want["n_kmers"][6] == 0
    assert want["max"][7] == 0xFFFFFFFE and want["median"][8] == 0xFFFFFFFE and want["sum"][8] > 1 << 42
    ctr.close()


@pytest.mark.parametrize("order", ["random", "ascending", "descending"])
@pytest.mark.parametrize("holes", [0.0, 0.5, 0.99])
def test_profile_stats_synthetic_arrays(torch_mod, ctx, order, holes):
    """kt_profile_stats takes any u32 array: seeded values straight into it, no table"""
    rng = np.random.default_rng(int(holes * 100) + len(order))
    lens = [0, 1, 2, 3, 63, 64, 65, 127, 128, 129, SHORT_MAX - 1, SHORT_MAX, SHORT_MAX + 1, 1000, MID_MAX - 1, MID_MAX,
            MID_MAX + 1, 5000, CHUNK - 1, CHUNK, CHUNK + 1, 70_000, 3 * CHUNK, 1_000_003]
    lens += [int(x) for x in rng.integers(1, 400, size=3000)] + [int(x) for x in rng.integers(200, 6000, size=300)]
    lens = [lens[i] for i in rng.permutation(len(lens))]
    offsets = np.zeros(len(lens) + 1, np.uint64)
    offsets[1:] = np.cumsum(lens, dtype=np.uint64)
    parts = []
    for i, L in enumerate(lens):
        shift = (0, 8, 24, 31)[i % 4]  # full-range values, and values that agree in their top bits
        v = (rng.integers(0, 0xFFFFFFFF, size=L, dtype=np.uint64) >> np.uint64(shift)).astype(np.uint32)
        if i % 7 == 0 and L:
            v[:] = v[0]
        if order != "random":
            v.sort()
            if order == "descending":
                v = v[::-1].copy()
        v[rng.random(L) < holes] = NO
        parts.append(v)
    prof = np.concatenate(parts)
    check_stats(torch_mod, ctx, prof, offsets, (order, holes))


# ---- 6. NULL outputs and errors ----------------------------------------------------------------------------------------------

def test_profile_stats_null_outputs(torch_mod, ctx):
    rng = np.random.default_rng(61)
    lens = [0, 5, 150, 151, 300, 2048, 2049, 40_000]
    offsets = np.zeros(len(lens) + 1, np.uint64)
    offsets[1:] = np.cumsum(lens, dtype=np.uint64)
    prof = rng.integers(0, 500, size=int(offsets[-1]), dtype=np.uint64).astype(np.uint32)
    prof[rng.random(len(prof)) < 0.2] = NO
    want = want_stats(prof, offsets)
    from kmertools_amd._lib import KT_MEM_HOST
    for skip in NAMES:
        got = stats_device(torch_mod, ctx, prof, offsets, skip=(skip,))
        assert got[skip] is None
        assert_stats(got, want, ("device, no", skip))
        outs = {name: (None if name == skip else np.full(len(lens), 0x5A, np.uint64 if name == "sum" else np.uint32)) for name in NAMES}
        ctx.profile_stats(prof, offsets, len(lens), outs["n_kmers"], outs["n_present"], outs["min"], outs["median"], outs["max"],
                          outs["sum"], KT_MEM_HOST)
        assert_stats(outs, want, ("host, no", skip))
    got = stats_device(torch_mod, ctx, prof, offsets, skip=NAMES)  # nothing asked for: nothing done
    assert all(v is None for v in got.values())


def test_profile_errors(torch_mod, ctx):
    torch = torch_mod
    from kmertools_amd import device
    from kmertools_amd._lib import KT_ERR_ARG, KT_MEM_DEVICE, KT_MEM_HOST, lib
    L = lib()
    k = 21
    ctr = device.Counter(ctx, k, 1 << 16)
    bases = np.frombuffer(b"ACGTACGTACGTACGTACGTACGTACGTACGTACGTTT", np.uint8).copy()
    offsets = np.array([0, 25, len(bases)], np.uint64)
    ctr.add_reads_host(bases, offsets)
    prof = np.full(len(bases), 0x77777777, np.uint32)
    p = lambda a: a.ctypes.data if a is not None else None

    def call(h=ctr._h, b=bases, o=offsets, n=2, a=prof, mem=KT_MEM_HOST, parts=1, part=0):
        return L.kt_ctr_profile(h, p(b), p(o), n, p(a), mem, parts, part)

    for kw in [dict(h=None), dict(parts=2, part=2), dict(parts=0, part=0), dict(mem=7), dict(o=None), dict(a=None), dict(b=None)]:
        assert call(**kw) == KT_ERR_ARG, kw
        assert L.kt_last_error(), kw
        assert (prof == 0x77777777).all(), kw
    assert call(a=None, o=None, b=None, n=0) == 0  # no reads: nothing to check
    assert call() == 0 and (prof[:5] != 0x77777777).all() and (prof[5:25] == 0x77777777).all()
    # one shard of a sharded table (allocated as rank 0 of 2, never connected): refused
    sh = device.Sharded(ctx, k, 1 << 16, 1 << 16, 2, 0, ("host", lambda s, r, n: 1), connect=False)
    prof[:] = 0x77777777
    assert call(h=sh.table._h) == KT_ERR_ARG and b"shard" in L.kt_last_error() and (prof == 0x77777777).all()
    sh.close()
    ctr.close()

    # kt_profile_stats
    outs = [np.full(2, 0x66666666, np.uint32) for _ in range(5)] + [np.full(2, 0x66, np.uint64)]

    def stats(c=ctx._h, a=prof, o=offsets, n=2, mem=KT_MEM_HOST):
        return L.kt_profile_stats(c, p(a), p(o), n, *[p(x) for x in outs], mem)

    big = np.array([0, 5, 5 + (1 << 32)], np.uint64)
    for kw in [dict(c=None), dict(mem=7), dict(o=None), dict(a=None), dict(o=big)]:
        assert stats(**kw) == KT_ERR_ARG, kw
        assert L.kt_last_error(), kw
        assert all((x == x[0]).all() and x[0] in (0x66666666, 0x66) for x in outs), kw
    assert b"2^32" in L.kt_last_error()
    dbig = torch.from_numpy(big.astype(np.int64)).cuda()
    dn = torch.zeros(2, dtype=torch.int64, device="cuda")
    assert L.kt_profile_stats(ctx._h, dn.data_ptr(), dbig.data_ptr(), 2, dn.data_ptr(), None, None, None, None, None,
                              KT_MEM_DEVICE) == KT_ERR_ARG
    assert b"2^32" in L.kt_last_error()
    assert stats(a=None, o=None, n=0) == 0
    prof[:] = NO
    assert stats() == 0 and outs[0][0] == 0 and outs[5][1] == 0  # (a profile of fill only: no k-mer anywhere)


# ---- 7. views and fences -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shift", [1, 3, 5])
def test_profile_views_and_fences(torch_mod, ctx, oracle, shift):
    """inputs and outputs as shifted views (4-byte arrays `shift` elements, the bases `shift` bytes into their buffers: not
    16-byte aligned) with guard regions before and behind every output"""
    torch = torch_mod
    from kmertools_amd import device
    from kmertools_amd.device import to_csr
    k, G = 15, 64
    seqs = mixed_reads(900 + shift, 600, k) + [np.frombuffer(b"ACGT", np.uint8)[np.random.default_rng(shift).integers(0, 4, size=40_000)].tobytes()]
    bases, offsets = to_csr(seqs)
    n, total = len(seqs), int(offsets[-1])
    table = Table.of_reads(oracle, bases, offsets, k)
    ctr = device.Counter(ctx, k, max(1 << 16, 2 * len(table.keys)))
    ctr.add_pairs_host(table.keys, table.counts)
    want = want_profile(oracle, seqs, k, table)

    def fenced(count, dtype, fill):
        """(whole buffer, the view of `count` elements behind a guard of G + shift elements)"""
        buf = torch.full((count + 2 * G + shift,), fill, dtype=dtype, device="cuda")
        return buf, buf[G + shift:G + shift + count]

    bb = torch.zeros(total + shift + 64, dtype=torch.uint8, device="cuda")
    bview = bb[shift:shift + total]
    bview.copy_(torch.from_numpy(bases))
    ob, oview = fenced(n + 1, torch.int64, -1)  # (8-byte elements: the offsets stay 8-byte aligned)
    oview.copy_(torch.from_numpy(offsets.astype(np.int64)))
    pb, pview = fenced(total, torch.int32, -1)
    assert pview.data_ptr() % 16 != 0 and bview.data_ptr() % 4 != 0
    ctr.profile(bview, oview, n, pview)
    torch.cuda.synchronize()
    got = u32(pb)
    assert np.array_equal(got[G + shift:G + shift + total], want)
    assert (got[:G + shift] == NO).all() and (got[G + shift + total:] == NO).all()
    # a 16-byte aligned view gives the same (the other store path of the kernel)
    pa = torch.full((total + 4,), -1, dtype=torch.int32, device="cuda")
    assert pa.data_ptr() % 16 == 0
    ctr.profile(bview, oview, n, pa)
    torch.cuda.synchronize()
    assert np.array_equal(u32(pa)[:total], want) and (u32(pa)[total:] == NO).all()
    # the statistics from the shifted profile into fenced outputs
    ws = want_stats(want, offsets)
    outs = {name: fenced(n, torch.int64 if name == "sum" else torch.int32, 0x3C3C3C3C) for name in NAMES}
    ctx.profile_stats(pview, oview, n, *[outs[name][1] for name in NAMES])
    torch.cuda.synchronize()
    for name in NAMES:
        whole = outs[name][0].cpu().numpy()
        body = whole[G + shift:G + shift + n].view(np.uint64 if name == "sum" else np.uint32)
        assert np.array_equal(body, ws[name]), (name, shift)
        assert (whole[:G + shift] == 0x3C3C3C3C).all() and (whole[G + shift + n:] == 0x3C3C3C3C).all(), (name, shift)
    ctr.close()


# ---- 8. full size ---------------------------------------------------------------------------------------------------------------

def test_profile_full_size_k31(torch_mod, ctx, oracle):
    """10 M x 150 bp against their own k = 31 table: the invariants on every read, the profile and the statistics of 20 000
    sampled reads against the oracle; then four sequences of 20 Mbases"""
    torch = torch_mod
    from kmertools_amd import device
    k, n, L = 31, 10_000_000, 150
    kpr = L - k + 1
    bases = torch.empty(n * L, dtype=torch.uint8, device="cuda")
    offsets = torch.empty(n + 1, dtype=torch.int64, device="cuda")
    ctx.synth_reads(0xF117E5, n, L, bases, offsets, noise=True, genome_len=20_000_000)
    ctr = device.Counter(ctx, k, int(1.9 * n * kpr))
    ctr.add_reads(bases, offsets, n)
    prof = torch.full((n * L + 1,), -1, dtype=torch.int32, device="cuda")
    ctr.profile(bases, offsets, n, prof)
    out = {name: torch.full((n,), 0x5A5A5A5A, dtype=torch.int64 if name == "sum" else torch.int32, device="cuda") for name in NAMES}
    ctx.profile_stats(prof, offsets, n, *[out[name] for name in NAMES])
    torch.cuda.synchronize()
    assert int(prof[n * L]) == -1
    st = {name: out[name].cpu().numpy().view(np.uint64 if name == "sum" else np.uint32) for name in NAMES}
    clean = (bases.view(n, L) != ord("N")).all(dim=1).cpu().numpy()  # (the synthetic reads are upper case)
    assert clean.any() and (st["n_kmers"][clean] == kpr).all() and (st["n_kmers"] <= kpr).all()
    assert (st["min"] <= st["median"]).all() and (st["median"] <= st["max"]).all()
    assert (st["sum"] >= st["n_kmers"]).all() and (st["n_present"] == st["n_kmers"]).all()
    assert (st["median"] > 1).any() and (st["min"] < st["median"]).any()
    rng = np.random.default_rng(8)
    sample = np.sort(rng.choice(n, size=20000, replace=False))
    ds = torch.from_numpy(sample).cuda()
    hb = bases.view(n, L)[ds].cpu().numpy()
    hp = prof[:n * L].view(n, L)[ds].cpu().numpy().view(np.uint32)
    per = [oracle.kmers(hb[i].tobytes(), k) for i in range(len(sample))]
    counts = ctr.lookup_host(np.concatenate([np.minimum(f, r) for f, r, _ in per]))
    # (kt_ctr_lookup is the parent's; the table itself is pinned to the oracle by the counting tests)
    at = 0
    want = np.full((len(sample), L), NO, np.uint32)
    for j, (f, r, end) in enumerate(per):
        want[j, (end - np.uint64(k - 1)).astype(np.int64)] = counts[at:at + len(f)]
        at += len(f)
    assert np.array_equal(hp, want)
    ws = want_stats(want.reshape(-1), np.arange(len(sample) + 1, dtype=np.uint64) * np.uint64(L))
    for name in NAMES:
        assert np.array_equal(st[name][sample], ws[name]), name
    ctr.close()
    del bases, offsets, prof, out
    torch.cuda.empty_cache()

    # four sequences of 20 Mbases (tools/min_wide_timing.py's), parts of the first counted two and three times
    n, L = 4, 20_000_000
    g = torch.Generator(device="cuda").manual_seed(7)
    bases = torch.tensor(list(b"ACGT"), dtype=torch.uint8, device="cuda")[torch.randint(0, 4, (n * L,), device="cuda", generator=g)]
    offsets = torch.arange(0, (n + 1) * L, L, dtype=torch.int64, device="cuda")
    again = torch.tensor([0, 11_000_000, 11_000_000 + L // 3], dtype=torch.int64, device="cuda")  # seq 0's [0, 11 M) and [11 M, 11 M + L / 3)
    ctr = device.Counter(ctx, k, int(1.9 * (n * L + 2 * L)))
    ctr.add_reads(bases, offsets, n)
    ctr.add_reads(bases, again, 2)
    ctr.add_reads(bases, again, 1)
    prof = torch.full((n * L + 1,), -1, dtype=torch.int32, device="cuda")
    ctr.profile(bases, offsets, n, prof)
    out = {name: torch.full((n,), 0x5A5A5A5A, dtype=torch.int64 if name == "sum" else torch.int32, device="cuda") for name in NAMES}
    ctx.profile_stats(prof, offsets, n, *[out[name] for name in NAMES])
    torch.cuda.synchronize()
    st = {name: out[name].cpu().numpy().view(np.uint64 if name == "sum" else np.uint32) for name in NAMES}
    assert int(prof[n * L]) == -1
    assert (st["n_kmers"] == L - k + 1).all() and (st["n_present"] == st["n_kmers"]).all()
    assert (st["min"] <= st["median"]).all() and (st["median"] <= st["max"]).all() and (st["sum"] >= st["n_kmers"]).all()
    # sequence 0 exactly: the oracle's table of everything that was counted, its k-mers, numpy
    hb = bases.cpu().numpy()
    ho = offsets.cpu().numpy().astype(np.uint64)
    ha = again.cpu().numpy().astype(np.uint64)
    seq0 = hb[:L]
    cb = np.concatenate([hb, seq0[int(ha[0]):int(ha[2])], seq0[int(ha[0]):int(ha[1])]])
    co = np.concatenate([ho, ho[-1] + np.array([ha[1], ha[2], ha[2] + ha[1]], np.uint64)])
    table = Table.of_reads(oracle, cb, co, k, threads=16)
    f, r, end = oracle.kmers(seq0.tobytes(), k)
    want = np.full(L, NO, np.uint32)
    want[(end - np.uint64(k - 1)).astype(np.int64)] = table.count(np.minimum(f, r))
    assert np.array_equal(prof[:L].cpu().numpy().view(np.uint32), want)
    ws = want_stats(want, np.array([0, L], np.uint64))
    assert ws["median"][0] == 3 and ws["min"][0] == 1  # (more than half of its k-mers were counted three times)
    for name in NAMES:
        assert st[name][0] == ws[name][0], name
    ctr.close()
    del bases, offsets, prof
    torch.cuda.empty_cache()


# ---- 9. the CLI end to end ----------------------------------------------------------------------------------------------------

def run(*args, env=None, cwd=None):
    return subprocess.run([CLI, *map(str, args)], capture_output=True, timeout=600, env=env, cwd=cwd)


def parse_records(data):
    """(header without '>' / '@', sequence): what the reader keeps with keep_records"""
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
            out.append((h[1:], b"".join(seq)))
    else:
        while i < len(lines):
            h = lines[i].rstrip(ws)
            if not h:
                i += 1
                continue
            out.append((h[1:], lines[i + 1].rstrip(ws)))
            i += 4
    return out


def read_file(path):
    data = open(path, "rb").read()
    return gzip.decompress(data) if str(path).endswith(".gz") else data


def want_files(oracle, recs, count_recs, k):
    """(profile.stats, profile.counts) as bytes"""
    table = Table.of_reads(oracle, *oracle.to_csr([s for _, s in count_recs]), k)
    seqs = [s for _, s in recs]
    prof = want_profile(oracle, seqs, k, table)
    offsets = np.zeros(len(seqs) + 1, np.uint64)
    offsets[1:] = np.cumsum([len(s) for s in seqs], dtype=np.uint64)
    st = want_stats(prof, offsets)
    stats = ["#name\tlength\tkmers\tpresent\tmin\tmedian\tmean\tmax\n"]
    counts = []
    for i, (hdr, seq) in enumerate(recs):
        name = hdr.split()[0].decode("latin-1") if hdr.split() else ""
        nk = int(st["n_kmers"][i])
        stats.append("%s\t%d\t%d\t%d\t%d\t%d\t%s\t%d\n" % (name, len(seq), nk, st["n_present"][i], st["min"][i], st["median"][i],
                                                          oracle.fmt_fixed6(int(st["sum"][i]) / max(1, nk)), st["max"][i]))
        v = prof[int(offsets[i]):int(offsets[i + 1])].astype(np.int64)
        v[v == NO] = -1
        counts.append(">%s\n%s\n" % (name, " ".join(map(str, v))))
    return "".join(stats).encode("latin-1"), "".join(counts).encode("latin-1")


@pytest.fixture(scope="module")
def cli_bin():
    if not os.path.exists(CLI):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "kmertools_amd", "csrc"), "-j4"], stdout=subprocess.DEVNULL)
    return CLI


def test_profile_cli_golden_inputs(cli_bin, oracle, tmp_path):
    for name in ("reads.fa", "reads.fq", "reads.fq.gz"):
        src = os.path.join(GOLDEN, name)
        recs = parse_records(read_file(src))
        for k in (5, 15, 31):
            ws, wc = want_files(oracle, recs, recs, k)
            out = tmp_path / ("out_%s_%d" % (name, k))
            r = run("profile", "-i", src, "-o", out, "-k", k, "--positions")
            assert r.returncode == 0, r.stderr
            assert (out / "profile.stats").read_bytes() == ws, (name, k)
            assert (out / "profile.counts").read_bytes() == wc, (name, k)
            out2 = tmp_path / ("out2_%s_%d" % (name, k))
            r = run("profile", "-i", src, "-o", out2, "-k", k)
            assert r.returncode == 0, r.stderr
            assert (out2 / "profile.stats").read_bytes() == ws and not (out2 / "profile.counts").exists()


def noisy_fasta(seed, n, k):
    """records sampled from a small genome with substitutions, N and lower case, multi-word headers, some shorter than k,
    an empty one, two long ones"""
    rng = np.random.default_rng(seed)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    genome = acgt[rng.integers(0, 4, size=20000)]
    out = []
    for i in range(n):
        L = int(rng.integers(0, 220)) if i % 10 == 0 else int(rng.integers(60, 220))
        if i == 5:
            L = k - 1
        if i in (17, 400):
            L = 9000
        a = int(rng.integers(0, len(genome) - L))
        s = genome[a:a + L].copy()
        err = rng.random(L) < 0.01
        s[err] = acgt[rng.integers(0, 4, size=int(err.sum()))]
        if L > 50 and rng.random() < 0.1:
            s[int(rng.integers(0, L))] = ord("N")
        if L > 50 and rng.random() < 0.1:
            b = int(rng.integers(0, L - 20))
            s[b:b + 20] = np.frombuffer(bytes(s[b:b + 20]).lower(), np.uint8)
        out.append(b">rec%d lane=%d  sample x\n%s\n" % (i, i % 5, s.tobytes()))
    return b"".join(out)


def test_profile_cli_batches_passes_and_counting_input(cli_bin, oracle, tmp_path):
    k = 21
    fa = tmp_path / "seqs.fa"
    fa.write_bytes(noisy_fasta(12, 1500, k))
    other = tmp_path / "sample.fa"
    other.write_bytes(noisy_fasta(12, 900, k) + noisy_fasta(13, 300, k))
    recs = parse_records(fa.read_bytes())
    assert any(len(s) == k - 1 for _, s in recs) and any(len(s) == 0 for _, s in recs)
    ws, wc = want_files(oracle, recs, recs, k)
    short = [i for i, (_, s) in enumerate(recs) if len(s) == k - 1][0]
    line = ws.split(b"\n")[1 + short].split(b"\t")
    assert line[1:] == [b"%d" % (k - 1), b"0", b"0", b"0", b"0", b"0.000000", b"0"]  # a record below k: zeros ...
    assert wc.split(b"\n")[2 * short + 1] == b" ".join([b"-1"] * (k - 1))           # ... and a line of -1
    env0 = dict(os.environ)
    outs = []
    for tag, extra in (("plain", {}), ("batches", {"KT_CLI_BATCH_READS": "7"}), ("passes", {"KT_CTR_MAX_SLOTS": "65536"}),
                       ("both", {"KT_CLI_BATCH_READS": "50", "KT_CLI_BATCH_BASES": "20000", "KT_CTR_MAX_SLOTS": "65536"})):
        out = tmp_path / tag
        r = run("profile", "-i", fa, "-o", out, "-k", k, "--positions", "-t", "3", env={**env0, **extra, "KT_CLI_TIMING": "1"})
        assert r.returncode == 0, r.stderr
        if "KT_CTR_MAX_SLOTS" in extra:
            passes = re.findall(rb"(\d+) pass\(es\)", r.stderr)  # (the count's setup line under KT_CLI_TIMING)
            assert passes and int(passes[0]) >= 3, r.stderr
        assert (out / "profile.stats").read_bytes() == ws, tag
        assert (out / "profile.counts").read_bytes() == wc, tag
    # another counting input
    crecs = parse_records(other.read_bytes())
    ws2, wc2 = want_files(oracle, recs, crecs, k)
    assert ws2 != ws
    for tag, extra in (("a_plain", {}), ("a_passes", {"KT_CTR_MAX_SLOTS": "65536", "KT_CLI_BATCH_READS": "64"})):
        out = tmp_path / tag
        r = run("profile", "-i", fa, "-a", other, "-o", out, "-k", k, "--positions", env={**env0, **extra})
        assert r.returncode == 0, r.stderr
        assert (out / "profile.stats").read_bytes() == ws2 and (out / "profile.counts").read_bytes() == wc2, tag
