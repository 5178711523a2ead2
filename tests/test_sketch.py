"""MinHash sketches: kt_sketch_batch (the s smallest distinct hashes of every read's canonical k-mers), kt_sketch_merge
(bottom-s of unions of sketches) and kt_sketch_pairs (Mash's merge walk of every pair) against a numpy restatement over the
oracle's k-mers - known answers, ragged batches over the segment edges, inputs made of repeats, merges, pair matrices,
shifted views with fenced outputs, argument errors, full size; and `kmertools sketch` end to end against files restated
from the parsed records.  Everything is integers and compared exactly; the two floats of sketch.dist within 1e-12."""
import gzip
import json
import math
import os
import subprocess

import numpy as np
import pytest

from test_buffer_views import Fenced, HostFenced, bases_view, host_bases_view, noisy_reads, offsets_view

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "kmertools_amd", "bin", "kmertools")
GOLDEN = os.path.join(ROOT, "tests", "golden")
EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)  # KT_EMPTY_KEY
MAX_S = 16384
ACGT = np.frombuffer(b"ACGT", np.uint8)
U = np.uint64


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
def skat():
    with open(os.path.join(GOLDEN, "sketch_kat.json")) as f:
        return json.load(f)


# ---- the restatement ----------------------------------------------------------------------------------------------------

def mix64(z):
    """ktd::mix64 (splitmix64's finaliser) over a u64 array"""
    z = np.asarray(z, np.uint64) + U(0x9E3779B97F4A7C15)
    z = (z ^ (z >> U(30))) * U(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> U(27))) * U(0x94D049BB133111EB)
    return z ^ (z >> U(31))


def hash_sets(oracle, bases, offsets, k, seed):
    """per read: (its windows with multiplicity, the distinct hashes of its canonical k-mers, ascending)"""
    out = []
    for i in range(len(offsets) - 1):
        o, e = int(offsets[i]), int(offsets[i + 1])
        if e - o < k:
            out.append((0, np.zeros(0, np.uint64)))
            continue
        f, r, _ = oracle.kmers(np.ascontiguousarray(bases[o:e]).tobytes(), k)
        out.append((len(f), np.unique(mix64(np.minimum(f, r) ^ U(seed)))))
    return out


def rows_of(sets, s):
    """what kt_sketch_batch writes for such sets: (hashes [n, s] with KT_EMPTY_KEY behind the sizes, sizes, n_kmers)"""
    n = len(sets)
    hashes = np.full((n, s), EMPTY, np.uint64)
    sizes, nk = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
    for i, (windows, h) in enumerate(sets):
        m = min(s, len(h))
        hashes[i, :m] = h[:m]
        sizes[i], nk[i] = m, windows
    return hashes, sizes, nk


def merge_walk(a, b, s):
    """Mash's walk over two strictly ascending arrays: (shared, denom)"""
    i = j = shared = denom = 0
    while denom < s and i < len(a) and j < len(b):
        if a[i] < b[j]:
            i += 1
        elif b[j] < a[i]:
            j += 1
        else:
            shared += 1
            i += 1
            j += 1
        denom += 1
    if denom < s:
        denom = min(s, denom + (len(a) - i) + (len(b) - j))
    return shared, denom


def want_pair(a, b, s, walk=True):
    """the definition: denom = min(s, |A u B|), shared = those of the denom smallest of A u B that are in both; asserted to be
    what the merge walk gives"""
    u = np.union1d(a, b)
    denom = min(s, len(u))
    shared = int(np.isin(np.intersect1d(a, b), u[:denom]).sum())
    if walk:
        assert merge_walk(a, b, s) == (shared, denom)
    return shared, denom


def want_pairs(ah, asz, bh, bsz, s, walk=True):
    shared = np.zeros((len(asz), len(bsz)), np.uint32)
    denom = np.zeros_like(shared)
    for i in range(len(asz)):
        for j in range(len(bsz)):
            shared[i, j], denom[i, j] = want_pair(ah[i, :asz[i]], bh[j, :bsz[j]], s, walk)
    return shared, denom


def dev_sketch(torch, ctx, bases, offsets, k, s, seed, n_kmers=True):
    """kt_sketch_batch in device mode over prefilled outputs"""
    n = len(offsets) - 1
    d_b = torch.from_numpy(np.ascontiguousarray(bases) if len(bases) else np.zeros(1, np.uint8)).cuda()
    d_o = torch.from_numpy(np.asarray(offsets).astype(np.int64)).cuda()
    h = torch.full((n, s), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device="cuda")
    z = torch.full((n,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    nk = torch.full((n,), 0x5A5A5A5A, dtype=torch.int32, device="cuda") if n_kmers else None
    ctx.sketch(d_b, d_o, n, k, s, h, z, nk, seed)
    torch.cuda.synchronize()
    return (h.cpu().numpy().view(np.uint64), z.cpu().numpy().view(np.uint32),
            nk.cpu().numpy().view(np.uint32) if n_kmers else None)


def check_batch(torch, ctx, oracle, bases, offsets, k, s, seed, mode, sets=None):
    sets = hash_sets(oracle, bases, offsets, k, seed) if sets is None else sets
    wh, wz, wn = rows_of(sets, s)
    if mode == "host":
        gh, gz, gn = ctx.sketch_host(bases, offsets, k, s, seed)
    else:
        gh, gz, gn = dev_sketch(torch, ctx, bases, offsets, k, s, seed)
    assert np.array_equal(gn, wn), ("n_kmers", k, s, seed, mode, np.flatnonzero(gn != wn)[:8])
    assert np.array_equal(gz, wz), ("sizes", k, s, seed, mode, np.flatnonzero(gz != wz)[:8], gz[:12], wz[:12])
    assert np.array_equal(gh, wh), ("hashes", k, s, seed, mode, np.argwhere(gh != wh)[:8])


def read_fasta(path):
    opener = gzip.open if str(path).endswith(".gz") else open
    recs = []
    with opener(path, "rt") as f:
        for line in f:
            line = line.rstrip("\n")
            if line.startswith(">"):
                recs.append([line[1:].split()[0], ""])
            elif line:
                recs[-1][1] += line
    return [(n, s.encode()) for n, s in recs]


# ---- known answers ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", ["host", "device"])
def test_sketch_known_answers(torch_mod, ctx, skat, mode):
    from kmertools_amd import device
    assert int(mix64(np.zeros(1, np.uint64))[0]) == skat["mix64_of_0"]
    recs = read_fasta(os.path.join(GOLDEN, "reads.fa"))
    bases, offsets = device.to_csr([s for _, s in recs])

    def run(k, s, seed):
        if mode == "host":
            return ctx.sketch_host(bases, offsets, k, s, seed)
        return dev_sketch(torch_mod, ctx, bases, offsets, k, s, seed)

    for ka in skat["sketches"]:
        h, z, nk = run(ka["k"], ka["s"], ka["seed"])
        r = ka["record"]
        assert int(nk[r]) == ka["windows"] and int(z[r]) == ka["size"]
        assert [int(x) for x in h[r]] == ka["hashes"], ka
    h, z, nk = run(4, 1000, 0)
    for ka in skat["k4_s1000_seed0"]:
        r = ka["record"]
        assert (int(nk[r]), int(z[r]), int(h[r, 0])) == (ka["windows"], ka["size"], ka["first_hash"])
        assert (h[r, z[r]:] == EMPTY).all() and (np.diff(h[r, :z[r]].astype(object)) > 0).all()
    h, z, _ = run(4, 16, 0)
    pk = skat["pair_k4_s16_seed0"]
    if mode == "host":
        shared, denom = ctx.sketch_pairs_host(h, z)
    else:
        d_h, d_z = torch_mod.from_numpy(h.view(np.int64)).cuda(), torch_mod.from_numpy(z.view(np.int32)).cuda()
        d_s = torch_mod.full((len(z), len(z)), -1, dtype=torch_mod.int32, device="cuda")
        d_d = torch_mod.full((len(z), len(z)), -1, dtype=torch_mod.int32, device="cuda")
        ctx.sketch_pairs(d_h, d_z, len(z), d_h, d_z, len(z), 16, d_s, d_d)
        torch_mod.cuda.synchronize()
        shared, denom = d_s.cpu().numpy().view(np.uint32), d_d.cpu().numpy().view(np.uint32)
    assert (int(shared[pk["a"], pk["b"]]), int(denom[pk["a"], pk["b"]])) == (pk["shared"], pk["denom"])
    assert (int(shared[pk["b"], pk["a"]]), int(denom[pk["b"], pk["a"]])) == (pk["shared"], pk["denom"])


# ---- ragged batches --------------------------------------------------------------------------------------------------------

def noisy(rng, L):
    s = ACGT[rng.integers(0, 4, size=L)].copy()
    if L:
        m = rng.random(L)
        s[m < 0.002] = ord("N")
        s[(m > 0.01) & (m < 0.05)] |= 0x20
        s[(m > 0.05) & (m < 0.055)] = ord("U")
    return s.tobytes()


def ragged_batch(k):
    """the segment edges (8192 bases), the lengths around k, long reads - and more short ones between, so that reads start and
    end at every kind of place in a segment"""
    rng = np.random.default_rng(1000 + k)
    lens = [0, k - 1, k, 150, 257, 2049, 8191, 8192, 8193, 100_000, 0, 40, 1_000_000, 150, 3, 16384, 0]
    return [noisy(rng, L) for L in lens]


_sets = {}


@pytest.mark.parametrize("k", [4, 15, 21, 31])
@pytest.mark.parametrize("s", [1, 16, 1000, 16384])
def test_sketch_ragged_batches(torch_mod, ctx, oracle, k, s):
    from kmertools_amd import device
    bases, offsets = device.to_csr(ragged_batch(k))
    for seed, mode in ((0, "host"), (0x9E3779B97F4A7C15, "device")):
        key = (k, seed)
        if key not in _sets:
            _sets[key] = hash_sets(oracle, bases, offsets, k, seed)
        check_batch(torch_mod, ctx, oracle, bases, offsets, k, s, seed, mode, _sets[key])


def test_sketch_many_short_reads(torch_mod, ctx, oracle):
    """the reads of the buffer-view suite: empty ones, shorter than k, N runs, raw codes, several per segment and across its edges"""
    from kmertools_amd import device
    bases, offsets = device.to_csr(noisy_reads(0x5eed, 700))
    for k, s in ((5, 16), (21, 64), (31, 1000)):
        check_batch(torch_mod, ctx, oracle, bases, offsets, k, s, 7, "device")
    check_batch(torch_mod, ctx, oracle, bases, offsets, 21, 16, 7, "host")
    # n_kmers may be NULL
    gh, gz, _ = dev_sketch(torch_mod, ctx, bases, offsets, 21, 16, 7, n_kmers=False)
    wh, wz, _ = rows_of(hash_sets(oracle, bases, offsets, 21, 7), 16)
    assert np.array_equal(gz, wz) and np.array_equal(gh, wh)


# ---- duplicates ------------------------------------------------------------------------------------------------------------

def test_sketch_duplicates(torch_mod, ctx, oracle):
    from kmertools_amd import device
    rng = np.random.default_rng(77)
    half = ACGT[rng.integers(0, 4, size=300_000)].tobytes()
    seqs = [b"A" * 1_000_000,                      # one distinct k-mer
            b"ACGGTCA" * 60_000,                   # a period-7 tandem repeat
            half + half,                           # the second half repeats the first
            ACGT[rng.integers(0, 4, size=500_000)].tobytes()]
    bases, offsets = device.to_csr(seqs)
    for k, s in ((21, 1000), (31, 16), (7, 16384)):
        sets = hash_sets(oracle, bases, offsets, k, 0)
        assert len(sets[0][1]) == 1 and len(sets[1][1]) <= 7
        check_batch(torch_mod, ctx, oracle, bases, offsets, k, s, 0, "device", sets)
    # k = 4: at most 136 canonical k-mers, size < s on a long input
    sets = hash_sets(oracle, bases, offsets, 4, 3)
    assert all(len(h) <= 136 for _, h in sets) and len(sets[3][1]) == 136
    check_batch(torch_mod, ctx, oracle, bases, offsets, 4, 1000, 3, "device", sets)
    check_batch(torch_mod, ctx, oracle, bases, offsets, 4, 1000, 3, "host", sets)


def test_sketch_repeated_kmer_below_the_threshold(torch_mod, ctx, oracle):
    """1 Mbase of one repeated k-mer and 2000 random bases behind it, with a seed that puts the repeated k-mer's hash below
    the 1000th smallest hash of the random part: a threshold taken from counts with multiplicity would stop at that hash"""
    from kmertools_amd import device
    k, s = 21, 1000
    rng = np.random.default_rng(5)
    tail = ACGT[rng.integers(0, 4, size=2000)].tobytes()
    f, r, _ = oracle.kmers(tail, k)
    keys = np.minimum(f, r)
    seed = next(sd for sd in range(1, 1000) if mix64(np.array([0 ^ sd], np.uint64))[0] < np.unique(mix64(keys ^ U(sd)))[s - 1])
    bases, offsets = device.to_csr([b"A" * 1_000_000 + tail, tail])
    sets = hash_sets(oracle, bases, offsets, k, seed)
    assert mix64(np.array([seed], np.uint64))[0] in sets[0][1][:s] and len(sets[0][1]) > s
    check_batch(torch_mod, ctx, oracle, bases, offsets, k, s, seed, "device", sets)
    check_batch(torch_mod, ctx, oracle, bases, offsets, k, s, seed, "host", sets)


# ---- merge -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("s", [16, 1000, 16384])
def test_sketch_merge(torch_mod, ctx, oracle, s):
    from kmertools_amd import device
    from kmertools_amd._lib import KT_MEM_DEVICE
    torch = torch_mod
    rng = np.random.default_rng(s)
    k = 15
    lens = [int(x) for x in rng.integers(0, 3000, size=40)]
    lens[3], lens[17] = 0, 20_000
    genome = ACGT[rng.integers(0, 4, size=30_000)]
    seqs = []
    for L in lens:  # pieces of one genome: the rows overlap
        a = int(rng.integers(0, len(genome) - L))
        seqs.append(genome[a:a + L].tobytes())
    bases, offsets = device.to_csr(seqs)
    sets = hash_sets(oracle, bases, offsets, k, 1)
    rows, sizes, _ = rows_of(sets, s)

    def want(groups):
        out = []
        for g in range(len(groups) - 1):
            parts = [sets[i][1] for i in range(groups[g], groups[g + 1])]
            out.append((0, np.unique(np.concatenate(parts)) if parts else np.zeros(0, np.uint64)))
        wh, wz, _ = rows_of(out, s)
        return wh, wz

    # a group of one row, of many, an empty one, the rest; then the whole batch; then rows in front of and behind the groups
    for groups in ([0, 1, 30, 30, 40], [0, 40], [0, 0, 2, 5, 5], [3, 4, 20], [7, 7]):
        go = np.array(groups, np.uint64)
        wh, wz = want(groups)
        gh, gz = ctx.sketch_merge(rows, sizes, go)
        assert np.array_equal(gz, wz), (groups, gz, wz)
        assert np.array_equal(gh, wh), (groups, np.argwhere(gh != wh)[:8])
        d_rows, d_sizes = torch.from_numpy(rows.view(np.int64)).cuda(), torch.from_numpy(sizes.view(np.int32)).cuda()
        d_go = torch.from_numpy(go.view(np.int64)).cuda()
        d_h = torch.full((len(groups) - 1, s), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device="cuda")
        d_z = torch.full((len(groups) - 1,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
        ctx.sketch_merge(d_rows, d_sizes, d_go, d_h, d_z, s, KT_MEM_DEVICE)
        torch.cuda.synchronize()
        assert np.array_equal(d_z.cpu().numpy().view(np.uint32), wz), groups
        assert np.array_equal(d_h.cpu().numpy().view(np.uint64), wh), groups
        assert np.array_equal(d_rows.cpu().numpy().view(np.uint64), rows)
    # the merge of the batch is the sketch of the concatenation's k-mer set: the same through kt_sketch_batch, read by read
    gh, gz, _ = ctx.sketch_host(bases, offsets, k, s, 1)
    mh, mz = ctx.sketch_merge(gh, gz, np.array([0, 40], np.uint64))
    wh, wz = want([0, 40])
    assert np.array_equal(mz, wz) and np.array_equal(mh, wh)


# ---- pairs -----------------------------------------------------------------------------------------------------------------

def random_sketches(rng, n, s, pool):
    """n rows of s: random subsets of a pool (so that rows share hashes), sizes mixed, 0 and s among them"""
    sizes = rng.integers(0, s + 1, size=n).astype(np.uint32)
    sizes[0], sizes[1 % n] = 0, s
    if n > 3:
        sizes[3] = s
    rows = np.full((n, s), EMPTY, np.uint64)
    for i in range(n):
        rows[i, :sizes[i]] = np.sort(rng.choice(pool, size=int(sizes[i]), replace=False))
    return rows, sizes


@pytest.mark.parametrize("s", [1, 16, 1000, 2049, 16384])
def test_sketch_pairs(torch_mod, ctx, s):
    torch = torch_mod
    rng = np.random.default_rng(100 + s)
    pool = np.unique(rng.integers(0, 2**63, size=3 * s + 8, dtype=np.int64).astype(np.uint64))
    n_a, n_b = (13, 9) if s <= 1000 else (6, 5)
    ah, asz = random_sketches(rng, n_a, s, pool)
    bh, bsz = random_sketches(rng, n_b, s, pool)
    bh[2], bsz[2] = ah[1], asz[1]  # an identical pair
    walk = s <= 1000
    # rectangular, host mode
    ws, wd = want_pairs(ah, asz, bh, bsz, s, walk)
    gs, gd = ctx.sketch_pairs_host(ah, asz, bh, bsz)
    assert np.array_equal(gd, wd), np.argwhere(gd != wd)[:8]
    assert np.array_equal(gs, ws), np.argwhere(gs != ws)[:8]
    assert (gs[1, 2], gd[1, 2]) == (s, s)
    # a against itself, device mode: symmetric, the diagonal is (size, size)
    ws, wd = want_pairs(ah, asz, ah, asz, s, walk)
    d_h, d_z = torch.from_numpy(ah.view(np.int64)).cuda(), torch.from_numpy(asz.view(np.int32)).cuda()
    d_s = torch.full((n_a, n_a), -1, dtype=torch.int32, device="cuda")
    d_d = torch.full((n_a, n_a), -1, dtype=torch.int32, device="cuda")
    ctx.sketch_pairs(d_h, d_z, n_a, d_h, d_z, n_a, s, d_s, d_d)
    torch.cuda.synchronize()
    gs, gd = d_s.cpu().numpy().view(np.uint32), d_d.cpu().numpy().view(np.uint32)
    assert np.array_equal(gs, ws) and np.array_equal(gd, wd)
    assert np.array_equal(gs, gs.T) and np.array_equal(gd, gd.T)
    assert np.array_equal(np.diag(gs), asz) and np.array_equal(np.diag(gd), asz)
    # denom == NULL, both modes
    d_s.fill_(-1)
    ctx.sketch_pairs(d_h, d_z, n_a, d_h, d_z, n_a, s, d_s, None)
    torch.cuda.synchronize()
    assert np.array_equal(d_s.cpu().numpy().view(np.uint32), ws)
    from kmertools_amd._lib import KT_MEM_HOST
    hs = np.full((n_a, n_b), 0xFFFFFFFF, np.uint32)
    ctx.sketch_pairs(ah, asz, n_a, bh, bsz, n_b, s, hs, None, KT_MEM_HOST)
    assert np.array_equal(hs, want_pairs(ah, asz, bh, bsz, s, False)[0])


def test_sketch_pairs_of_real_sketches_equal_the_full_sets(ctx, oracle):
    """shared / denom from the sketches are the same quantities taken over the reads' whole k-mer sets"""
    from kmertools_amd import device
    rng = np.random.default_rng(9)
    genome = ACGT[rng.integers(0, 4, size=6000)]
    seqs = [genome[a:a + L].tobytes() for a, L in ((0, 3000), (1000, 3000), (2500, 3500), (0, 6000), (5990, 10), (100, 25))]
    bases, offsets = device.to_csr(seqs)
    k, s = 15, 200
    sets = hash_sets(oracle, bases, offsets, k, 0)
    h, z, _ = ctx.sketch_host(bases, offsets, k, s, 0)
    gs, gd = ctx.sketch_pairs_host(h, z)
    for i in range(len(seqs)):
        for j in range(len(seqs)):
            assert (int(gs[i, j]), int(gd[i, j])) == want_pair(sets[i][1], sets[j][1], s, False), (i, j)
    assert gs[0, 1] > 0 and gs[0, 4] == 0


# ---- buffer views ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shift", [0, 1, 3, 4, 15, 17])
def test_sketch_batch_on_views(torch_mod, ctx, oracle, shift):
    from kmertools_amd import device
    torch = torch_mod
    bases, offsets = device.to_csr(noisy_reads(0x5eed + 1, 300))
    n, k, s = len(offsets) - 1, 21, 48
    wh, wz, wn = rows_of(hash_sets(oracle, bases, offsets, k, 2), s)
    d_b, d_o = bases_view(torch, bases, shift), offsets_view(torch, offsets)
    keep = d_b.clone()
    h = Fenced(torch, (n, s), torch.int64, align=8, prefill=torch.full((n, s), 0x1111111111111111, dtype=torch.int64))
    z = Fenced(torch, n, torch.int32, align=4, prefill=torch.full((n,), 0x22222222, dtype=torch.int32))
    nk = Fenced(torch, n, torch.int32, align=12, prefill=torch.full((n,), 0x33333333, dtype=torch.int32))
    ctx.sketch(d_b, d_o, n, k, s, h.t, z.t, nk.t, 2)
    torch.cuda.synchronize()
    for f, name in ((h, "hashes"), (z, "sizes"), (nk, "n_kmers")):
        f.check(name)
    assert torch.equal(d_b, keep)
    assert np.array_equal(nk.np(np.uint32), wn) and np.array_equal(z.np(np.uint32), wz)
    assert np.array_equal(h.np(np.uint64).reshape(n, s), wh)
    # host mode
    hb = host_bases_view(bases, shift)
    hh, hz, hn = (HostFenced((n, s), np.uint64, prefill=0x1111111111111111), HostFenced(n, np.uint32, prefill=0x22222222),
                  HostFenced(n, np.uint32, prefill=0x33333333))
    from kmertools_amd._lib import KT_MEM_HOST
    ctx.sketch(hb, offsets, n, k, s, hh.a, hz.a, hn.a, 2, KT_MEM_HOST)
    for f, name in ((hh, "hashes"), (hz, "sizes"), (hn, "n_kmers")):
        f.check(name)
    assert np.array_equal(hn.a, wn) and np.array_equal(hz.a, wz) and np.array_equal(hh.a, wh)


def test_sketch_merge_and_pairs_on_views(torch_mod, ctx):
    from kmertools_amd._lib import KT_MEM_DEVICE
    torch = torch_mod
    s = 40
    rng = np.random.default_rng(4)
    pool = np.unique(rng.integers(0, 2**63, size=200, dtype=np.int64).astype(np.uint64))
    rows, sizes = random_sketches(rng, 11, s, pool)
    groups = [0, 3, 3, 4, 11]
    want = []
    for g in range(len(groups) - 1):
        parts = [rows[i, :sizes[i]] for i in range(groups[g], groups[g + 1])]
        want.append((0, np.unique(np.concatenate(parts)) if parts else np.zeros(0, np.uint64)))
    wh, wz, _ = rows_of(want, s)

    def view(a, dtype):  # the array at 8 mod 16 (u64) / 4 mod 8 (u32) inside a larger one
        raw = torch.zeros(a.size + 4, dtype=dtype, device="cuda")
        raw[1:1 + a.size] = torch.from_numpy(a.reshape(-1).view(np.int64 if dtype == torch.int64 else np.int32))
        return raw[1:1 + a.size]

    d_rows, d_sizes, d_go = view(rows, torch.int64), view(sizes, torch.int32), view(np.array(groups, np.uint64), torch.int64)
    oh = Fenced(torch, (4, s), torch.int64, align=8, prefill=torch.full((4, s), 0x1111111111111111, dtype=torch.int64))
    oz = Fenced(torch, 4, torch.int32, align=4, prefill=torch.full((4,), 0x22222222, dtype=torch.int32))
    ctx.sketch_merge(d_rows, d_sizes, d_go, oh.t, oz.t, s, KT_MEM_DEVICE)
    torch.cuda.synchronize()
    oh.check("merged hashes")
    oz.check("merged sizes")
    assert np.array_equal(oz.np(np.uint32), wz) and np.array_equal(oh.np(np.uint64).reshape(4, s), wh)
    assert np.array_equal(d_rows.cpu().numpy().view(np.uint64).reshape(11, s), rows)

    ws, wd = want_pairs(rows, sizes, wh, wz, s)
    sh = Fenced(torch, (11, 4), torch.int32, align=4, prefill=torch.full((11, 4), 0x44444444, dtype=torch.int32))
    dn = Fenced(torch, (11, 4), torch.int32, align=12, prefill=torch.full((11, 4), 0x55555555, dtype=torch.int32))
    ctx.sketch_pairs(d_rows, d_sizes, 11, oh.t, oz.t, 4, s, sh.t, dn.t)
    torch.cuda.synchronize()
    sh.check("shared")
    dn.check("denom")
    assert np.array_equal(sh.np(np.uint32).reshape(11, 4), ws) and np.array_equal(dn.np(np.uint32).reshape(11, 4), wd)


# ---- argument errors -------------------------------------------------------------------------------------------------------

def _raises_arg(fn):
    from kmertools_amd._lib import KT_ERR_ARG, KmertoolsError
    with pytest.raises(KmertoolsError) as e:
        fn()
    assert e.value.code == KT_ERR_ARG, e.value


def _small():
    from kmertools_amd import device
    bases, offsets = device.to_csr([b"ACGTTGCAACGTGGTCAGTCGATCGATTGCA", b"ACGT"])
    return bases, offsets, np.zeros((2, 8), np.uint64), np.zeros(2, np.uint32)


@pytest.mark.parametrize("k", [0, 32, -1])
def test_sketch_batch_rejects_k(ctx, k):
    from kmertools_amd._lib import KT_MEM_HOST
    b, o, h, z = _small()
    _raises_arg(lambda: ctx.sketch(b, o, 2, k, 8, h, z, None, 0, KT_MEM_HOST))


@pytest.mark.parametrize("s", [0, MAX_S + 1])
def test_sketch_calls_reject_s(ctx, s):
    from kmertools_amd._lib import KT_MEM_HOST
    b, o, h, z = _small()
    out = np.zeros(4, np.uint32)
    _raises_arg(lambda: ctx.sketch(b, o, 2, 21, s, h, z, None, 0, KT_MEM_HOST))
    _raises_arg(lambda: ctx.sketch_merge(h, z, np.array([0, 2], np.uint64), s=s))
    _raises_arg(lambda: ctx.sketch_pairs(h, z, 2, h, z, 2, s, out, None, KT_MEM_HOST))


def test_sketch_calls_reject_a_bad_mem(ctx):
    b, o, h, z = _small()
    out = np.zeros(4, np.uint32)
    _raises_arg(lambda: ctx.sketch(b, o, 2, 21, 8, h, z, None, 0, 2))
    _raises_arg(lambda: ctx.sketch_merge(h, z, np.array([0, 2], np.uint64), h[:1].copy(), z[:1].copy(), 8, 2))
    _raises_arg(lambda: ctx.sketch_pairs(h, z, 2, h, z, 2, 8, out, None, 2))


def test_sketch_calls_reject_null_buffers(ctx):
    from kmertools_amd._lib import KT_MEM_HOST
    b, o, h, z = _small()
    out = np.zeros(4, np.uint32)
    go = np.array([0, 2], np.uint64)
    for args in ((None, o, 2, 21, 8, h, z), (b, None, 2, 21, 8, h, z), (b, o, 2, 21, 8, None, z), (b, o, 2, 21, 8, h, None)):
        _raises_arg(lambda: ctx.sketch(*args, None, 0, KT_MEM_HOST))
    from kmertools_amd import _lib
    from kmertools_amd.device import _ptr
    L = _lib.lib()
    for bad in range(5):
        a = [_ptr(h), _ptr(z), 2, 8, _ptr(go), 1, _ptr(h.copy()), _ptr(z.copy()), KT_MEM_HOST]
        a[(0, 1, 4, 6, 7)[bad]] = None
        assert L.kt_sketch_merge(ctx._h, *a) == _lib.KT_ERR_ARG, bad
    for bad in range(5):
        a = [_ptr(h), _ptr(z), 2, _ptr(h), _ptr(z), 2, 8, _ptr(out), None, KT_MEM_HOST]
        a[(0, 1, 3, 4, 7)[bad]] = None
        assert L.kt_sketch_pairs(ctx._h, *a) == _lib.KT_ERR_ARG, bad
    # nothing to do is no error
    ctx.sketch(None, None, 0, 21, 8, None, None, None, 0, KT_MEM_HOST)


def test_sketch_batch_rejects_a_read_of_2_32_bases(torch_mod, ctx):
    """offsets alone say so: the bases are never touched (device mode; one byte of bases is allocated)"""
    torch = torch_mod
    from kmertools_amd._lib import KT_MEM_HOST
    d_b = torch.zeros(16, dtype=torch.uint8, device="cuda")
    d_o = torch.tensor([0, 5, 5 + 2**32], dtype=torch.int64, device="cuda")
    h = torch.zeros((2, 4), dtype=torch.int64, device="cuda")
    z = torch.zeros(2, dtype=torch.int32, device="cuda")
    _raises_arg(lambda: ctx.sketch(d_b, d_o, 2, 21, 4, h, z, None, 0))
    _raises_arg(lambda: ctx.sketch(np.zeros(16, np.uint8), np.array([0, 5, 5 + 2**32], np.uint64), 2, 21, 4,
                                   np.zeros((2, 4), np.uint64), np.zeros(2, np.uint32), None, 0, KT_MEM_HOST))


@pytest.mark.parametrize("groups", [[0, 2, 1], [1, 0], [0, 3]])
def test_sketch_merge_rejects_bad_group_offsets(torch_mod, ctx, groups):
    from kmertools_amd._lib import KT_MEM_DEVICE
    torch = torch_mod
    _, _, h, z = _small()
    go = np.array(groups, np.uint64)
    _raises_arg(lambda: ctx.sketch_merge(h, z, go))
    d_h, d_z = torch.from_numpy(h.view(np.int64)).cuda(), torch.from_numpy(z.view(np.int32)).cuda()
    d_go = torch.from_numpy(go.view(np.int64)).cuda()
    o_h = torch.zeros((len(groups) - 1, 8), dtype=torch.int64, device="cuda")
    o_z = torch.zeros(len(groups) - 1, dtype=torch.int32, device="cuda")
    _raises_arg(lambda: ctx.sketch_merge(d_h, d_z, d_go, o_h, o_z, 8, KT_MEM_DEVICE))


# ---- the command line --------------------------------------------------------------------------------------------------------

def cli_run(*args, env=None):
    e = dict(os.environ)
    e.update(env or {})
    return subprocess.run([CLI, *map(str, args)], capture_output=True, text=True, timeout=600, env=e)


def write_fasta(path, recs, width=70):
    opener = gzip.open if str(path).endswith(".gz") else open
    with opener(path, "wt") as f:
        for name, seq in recs:
            f.write(">%s some description\n" % name)
            for a in range(0, len(seq), width):
                f.write(seq[a:a + width].decode() + "\n")


def cli_records(seed, n):
    rng = np.random.default_rng(seed)
    genome = ACGT[rng.integers(0, 4, size=40_000)]
    recs = []
    for i in range(n):
        L = int(rng.integers(0, 12_000)) if i % 5 else (0, 10, 20_000)[i // 5 % 3]
        a = int(rng.integers(0, len(genome) - L))
        seq = genome[a:a + L].copy()
        if L > 50:
            seq[rng.integers(0, L, size=3)] = ord("N")
            seq[10:20] |= 0x20
        recs.append(("rec%d" % i, seq.tobytes()))
    recs.append(("copy_of_1", recs[1][1]))
    return recs


def want_tsv(oracle, recs, k, s, seed):
    from kmertools_amd import device
    bases, offsets = device.to_csr([q for _, q in recs])
    sets = hash_sets(oracle, bases, offsets, k, seed)
    lines = ["%s\t%d\t%d\t%d\t%s" % (name, len(q), w, min(s, len(h)), ",".join(str(int(x)) for x in h[:s]))
             for (name, q), (w, h) in zip(recs, sets)]
    return lines, sets


def want_distance(shared, denom, k):
    j = shared / denom if denom else 0.0
    return (j, 1.0) if j == 0.0 else (j, min(1.0, -math.log(2.0 * j / (1.0 + j)) / k))


def check_dist(path, pairs, k, max_dist=1.0):
    """pairs: (id_a, id_b, shared, denom) in the order of the file, before --max-dist"""
    want = []
    for a, b, sh, dn in pairs:
        j, d = want_distance(sh, dn, k)
        if d <= max_dist:
            want.append((a, b, "%d/%d" % (sh, dn), j, d))
    got = [line.split("\t") for line in open(path).read().splitlines()]
    assert len(got) == len(want), (len(got), len(want))
    for g, w in zip(got, want):
        assert len(g) == 5 and tuple(g[:3]) == w[:3], (g, w)
        assert abs(float(g[3]) - w[3]) <= 1e-12 and abs(float(g[4]) - w[4]) <= 1e-12, (g, w)
        if w[4] == 0.0:
            assert g[4] == "0"
    return len(want)


@pytest.mark.parametrize("gz", [False, True])
def test_cli_sketch_end_to_end(oracle, tmp_path, gz):
    k, s, seed = 15, 64, 5
    recs_a, recs_b = cli_records(1, 23), cli_records(2, 9)
    fa = tmp_path / ("a.fa.gz" if gz else "a.fa")
    fb = tmp_path / ("b.fasta.gz" if gz else "b.fasta")
    write_fasta(fa, recs_a)
    write_fasta(fb, recs_b)
    lines_a, sets_a = want_tsv(oracle, recs_a, k, s, seed)
    lines_b, sets_b = want_tsv(oracle, recs_b, k, s, seed)
    # the input alone, all pairs i < j
    out = tmp_path / "one"
    r = cli_run("sketch", "-i", fa, "-o", out, "-k", k, "-s", s, "--seed", seed, "--dist")
    assert r.returncode == 0, r.stderr
    assert open(out / "sketch.tsv").read().splitlines() == lines_a
    assert not (out / "sketch.alt.tsv").exists()
    pairs = [(recs_a[i][0], recs_a[j][0]) + want_pair(sets_a[i][1][:s], sets_a[j][1][:s], s)
             for i in range(len(recs_a)) for j in range(i + 1, len(recs_a))]
    n_all = check_dist(out / "sketch.dist", pairs, k)
    assert n_all == len(recs_a) * (len(recs_a) - 1) // 2
    assert any(p[0] == "rec1" and p[1] == "copy_of_1" and p[2] == p[3] for p in pairs)
    # --max-dist keeps exactly the lines at or below D; several batches give the same files
    out2 = tmp_path / "two"
    r = cli_run("sketch", "-i", fa, "-o", out2, "-k", k, "-s", s, "--seed", seed, "--dist", "--max-dist", "0.05",
                env={"KT_CLI_BATCH_READS": "4"})
    assert r.returncode == 0, r.stderr
    assert open(out2 / "sketch.tsv").read().splitlines() == lines_a
    n_kept = check_dist(out2 / "sketch.dist", pairs, k, 0.05)
    assert 0 < n_kept < n_all
    # two inputs: every (i of -i, j of -a)
    out3 = tmp_path / "three"
    r = cli_run("sketch", "-i", fa, "-a", fb, "-o", out3, "-k", k, "-s", s, "--seed", seed, "--dist")
    assert r.returncode == 0, r.stderr
    assert open(out3 / "sketch.tsv").read().splitlines() == lines_a
    assert open(out3 / "sketch.alt.tsv").read().splitlines() == lines_b
    pairs = [(recs_a[i][0], recs_b[j][0]) + want_pair(sets_a[i][1][:s], sets_b[j][1][:s], s)
             for i in range(len(recs_a)) for j in range(len(recs_b))]
    assert check_dist(out3 / "sketch.dist", pairs, k) == len(recs_a) * len(recs_b)
    # without --dist there is no sketch.dist; the defaults are k = 21, s = 1000, seed 0
    out4 = tmp_path / "four"
    r = cli_run("sketch", "-i", fb, "-o", out4)
    assert r.returncode == 0, r.stderr
    assert open(out4 / "sketch.tsv").read().splitlines() == want_tsv(oracle, recs_b, 21, 1000, 0)[0]
    assert not (out4 / "sketch.dist").exists()


def test_cli_sketch_single(oracle, tmp_path):
    k, s, seed = 15, 500, 0
    recs_a, recs_b = cli_records(3, 17), cli_records(4, 6)
    fa, fb = tmp_path / "sample_a.fa", tmp_path / "sample_b.fa.gz"
    write_fasta(fa, recs_a)
    write_fasta(fb, recs_b)

    def want_single(path, recs):
        _, sets = want_tsv(oracle, recs, k, s, seed)
        h = np.unique(np.concatenate([x for _, x in sets]))
        line = "%s\t%d\t%d\t%d\t%s" % (os.path.basename(path), sum(len(q) for _, q in recs), sum(w for w, _ in sets),
                                       min(s, len(h)), ",".join(str(int(x)) for x in h[:s]))
        return line, h[:s]

    la, ha = want_single(fa, recs_a)
    lb, hb = want_single(fb, recs_b)
    outs = []
    for name, env in (("one", {}), ("many", {"KT_CLI_BATCH_READS": "3"})):
        out = tmp_path / name
        r = cli_run("sketch", "-i", fa, "-a", fb, "-o", out, "-k", k, "-s", s, "--single", "--dist", env=env)
        assert r.returncode == 0, r.stderr
        assert open(out / "sketch.tsv").read().splitlines() == [la]
        assert open(out / "sketch.alt.tsv").read().splitlines() == [lb]
        check_dist(out / "sketch.dist", [(os.path.basename(fa), os.path.basename(fb)) + want_pair(ha, hb, s)], k)
        outs.append(open(out / "sketch.dist").read())
    assert outs[0] == outs[1]


# ---- full size -------------------------------------------------------------------------------------------------------------

def test_sketch_full_size(torch_mod, ctx, oracle):
    """4 x 20 Mbases and 100 000 x 5000 bases at k = 21, s = 1000: the sizes and the order of every row, sampled rows against
    the restatement"""
    torch = torch_mod
    k, s = 21, 1000
    rng = np.random.default_rng(2024)
    seqs = [ACGT[rng.integers(0, 4, size=20_000_000)] for _ in range(4)]
    seqs[1][5_000_000:5_000_100] = ord("N")
    seqs[2][10_000_000:] = seqs[2][:10_000_000]  # the second half repeats the first
    bases = np.concatenate(seqs)
    offsets = np.arange(5, dtype=np.uint64) * U(20_000_000)
    gh, gz, gn = dev_sketch(torch, ctx, bases, offsets, k, s, 0)
    sets = hash_sets(oracle, bases, offsets, k, 0)
    wh, wz, wn = rows_of(sets, s)
    assert np.array_equal(gn, wn) and np.array_equal(gz, wz) and (gz == s).all()
    assert np.array_equal(gh, wh)
    del seqs, bases, sets

    n, L = 100_000, 5000
    d_b = torch.empty(n * L, dtype=torch.uint8, device="cuda")
    d_o = torch.empty(n + 1, dtype=torch.int64, device="cuda")
    ctx.synth_reads(0x5CE7C4, n, L, d_b, d_o, noise=True)
    h = torch.full((n, s), -1, dtype=torch.int64, device="cuda")
    z = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    nk = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    ctx.sketch(d_b, d_o, n, k, s, h, z, nk, 11)
    torch.cuda.synchronize()
    # every row: full (5000 random bases hold far more than 1000 distinct 21-mers), strictly ascending as unsigned numbers
    assert bool((z == s).all())
    flipped = h ^ torch.tensor(-2**63, dtype=torch.int64, device="cuda")  # (unsigned order through signed compares)
    assert bool((flipped[:, 1:] > flipped[:, :-1]).all())
    assert bool((nk <= L - k + 1).all()) and bool((nk > 0).all())
    sample = np.sort(rng.choice(n, size=2000, replace=False))
    ds = torch.from_numpy(sample).cuda()
    hb = d_b.view(n, L)[ds].cpu().numpy()
    so = np.arange(len(sample) + 1, dtype=np.uint64) * U(L)
    wh, wz, wn = rows_of(hash_sets(oracle, hb.reshape(-1), so, k, 11), s)
    assert np.array_equal(nk[ds].cpu().numpy().view(np.uint32), wn)
    assert np.array_equal(h[ds].cpu().numpy().view(np.uint64), wh)
