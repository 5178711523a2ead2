"""The restatement of the two-pass pre-filter (no test in here): the hash and the two patterns of include/kmertools_hip.h
with numpy, and from the distinct canonical k-mers of an input with their multiplicities what the filter must hold after
pass 1 and what pass 2 may let through.

`once` does not depend on the order of execution: it is the OR of every k-mer's pattern.  `twice` does, between two sets:
  L  the OR of the twice patterns of the k-mers with two or more occurrences (each of them is promoted, whatever the order)
  U  L plus the twice patterns of every k-mer seen once whose once pattern is covered, in its word, by the patterns of OTHER
     k-mers (only those can have found their pattern covered when they arrived)
  E  the k-mers seen once whose twice pattern is covered by U: the only ones that may reach a table through pass 2.
The inputs of the GPU tests (tests/test_prefilter.py) are built here too, so that tests/test_prefilter_ref.py can hold them
to the conditions those tests rely on without a GPU."""
import numpy as np

import card_ref
from read_batches import ACGT, Batch

U64 = np.uint64
SEED = 0x5eed0f11
mix64 = card_ref.mix64


def pattern_of(h):
    """the OR of 1 << ((h >> 6 j) & 63), j = 0..3, over a u64 array"""
    h = np.asarray(h, np.uint64)
    p = np.zeros(len(h), np.uint64)
    for j in range(4):
        p |= U64(1) << ((h >> U64(6 * j)) & U64(63))
    return p


def once_of(kmers, a, seed=SEED):
    """-> (word index, pattern) in `once` of every canonical k-mer, and the hash the twice pair is made from"""
    h = mix64(np.asarray(kmers, np.uint64) ^ U64(seed))
    return (h >> U64(64 - a)).astype(np.int64), pattern_of(h), h


def twice_of(h, b):
    g = mix64(h)
    return (g >> U64(64 - b)).astype(np.int64), pattern_of(g)


def covered(arr, w, p):
    return (arr[w] & p) == p


def popcount(arr):
    return int(np.unpackbits(np.ascontiguousarray(arr).view(np.uint8)).sum())


class Model:
    def __init__(self, keys, counts, a, b, seed=SEED):
        """keys: the distinct canonical k-mers of the input, counts: their occurrences"""
        self.keys, self.counts = np.asarray(keys, np.uint64), np.asarray(counts, np.int64)
        self.a, self.b, self.seed = a, b, seed
        w1, p1, h = once_of(self.keys, a, seed)
        w2, p2 = twice_of(h, b)
        self.w1, self.p1, self.w2, self.p2 = w1, p1, w2, p2
        self.once = np.zeros(1 << a, np.uint64)
        np.bitwise_or.at(self.once, w1, p1)
        rep = self.counts >= 2
        self.single = ~rep
        self.L = np.zeros(1 << b, np.uint64)
        np.bitwise_or.at(self.L, w2[rep], p2[rep])
        # bit x of word w is set by others than k-mer i when at least two k-mers set it, or one that is not i: count the setters
        bits = ((p1[:, None] >> np.arange(64, dtype=np.uint64)[None, :]) & U64(1)).astype(np.int32)   # [n, 64]
        setters = np.zeros((1 << a, 64), np.int32)
        np.add.at(setters, w1, bits)
        by_others = ((setters[w1] - bits >= 1) | (bits == 0)).all(axis=1)
        self.may_promote = self.single & by_others
        self.U = self.L.copy()
        np.bitwise_or.at(self.U, w2[self.may_promote], p2[self.may_promote])
        self.in_E = self.single & covered(self.U, w2, p2)
        self.E = self.keys[self.in_E]
        # every bit of `twice` is set by an atomic OR that counts as a promotion and sets at most four: a lower bound
        self.min_promotions = int(sum((bin(int(x)).count("1") + 3) // 4 for x in self.L[self.L != 0]))

    def query(self, kmers):
        """-> (bit 0 as kt_prefilter_query must give it, bit 1 where L demands it, bit 1 where U allows it)"""
        w1, p1, h = once_of(kmers, self.a, self.seed)
        w2, p2 = twice_of(h, self.b)
        return covered(self.once, w1, p1), covered(self.L, w2, p2), covered(self.U, w2, p2)


# ---- a string-level brute force that shares nothing with the above but the constants ------------------------------------------

def brute(kmer_counts, a, b, seed=SEED):
    """kmer_counts: {canonical k-mer (int): occurrences}.  -> (once, L, U as lists of ints, E as a set), with Python integers,
    one k-mer at a time, `covered by others` by OR-ing the others' patterns"""
    def pat(h):
        p = 0
        for j in range(4):
            p |= 1 << ((h >> (6 * j)) & 63)
        return p
    info = {}
    for m in kmer_counts:
        h = card_ref.mix64_int(m ^ seed)
        g = card_ref.mix64_int(h)
        info[m] = (h >> (64 - a), pat(h), g >> (64 - b), pat(g))
    once, L = [0] * (1 << a), [0] * (1 << b)
    for m, c in kmer_counts.items():
        w1, p1, w2, p2 = info[m]
        once[w1] |= p1
        if c >= 2:
            L[w2] |= p2
    U = list(L)
    for m, c in kmer_counts.items():
        if c != 1:
            continue
        w1, p1, w2, p2 = info[m]
        others = 0
        for x in kmer_counts:
            if x != m and info[x][0] == w1:
                others |= info[x][1]
        if others & p1 == p1:
            U[w2] |= p2
    E = {m for m, c in kmer_counts.items() if c == 1 and U[info[m][2]] & info[m][3] == info[m][3]}
    return once, L, U, E


# ---- the inputs of the GPU tests ------------------------------------------------------------------------------------------------

def genome_reads(seed=11, genome=20000, cover=30, L=150, err=0.01):
    rng = np.random.default_rng(seed)
    g = ACGT[rng.integers(0, 4, size=genome)]
    reads = []
    for s in rng.integers(0, genome - L + 1, size=genome * cover // L):
        r = g[s:s + L].copy()
        hit = np.flatnonzero(rng.random(L) < err)
        r[hit] = ACGT[(np.searchsorted(ACGT, r[hit]) + rng.integers(1, 4, size=len(hit))) % 4]   # a substitution: another base
        reads.append(r.tobytes())
    return reads


def all_5mers(times):
    """every canonical 5-mer exactly `times` times: each as a read of its own (a window of 5 bases has one k-mer)"""
    out = []
    for v in range(4 ** 5):
        s = bytes(b"ACGT"[(v >> (2 * (4 - i))) & 3] for i in range(5))
        rc = bytes({65: 84, 67: 71, 71: 67, 84: 65}[c] for c in reversed(s))
        if s <= rc:          # (no 5-mer is its own reverse complement: k is odd)
            out += [s] * times
    return out


_batches = {}


def batch(name):
    """the batches of the issue, built once: noisy (the 20 kb genome at 30x, 1 % substitutions), twins (every read twice in a
    row), apart (the copies more than a segment of 8192 bases apart), homo (poly-A reads and one 100 kb homopolymer), short
    (reads shorter than k, empty reads, an N every k-th base), fives1 / fives2 (all canonical 5-mers once / twice)"""
    if name not in _batches:
        if name in ("noisy", "twins", "apart"):
            reads = genome_reads()
            if name == "twins":
                reads = [r for r in reads for _ in (0, 1)]
            elif name == "apart":
                reads = reads + reads          # 600 kb between a read and its copy
            seqs = reads
        elif name == "homo":
            seqs = [b"A" * 150] * 64 + [b"A" * 100000] + [b"T" * 150] * 3 + [b"a" * 31]
        elif name == "short":
            rng = np.random.default_rng(5)
            seqs = []
            for i in range(600):
                L = int(rng.integers(0, 40))
                s = ACGT[rng.integers(0, 4, size=L)].copy()
                if i % 3 == 0 and L:
                    s[::max(1, L // 3)] = ord("N")
                seqs.append(s.tobytes() if i % 7 else b"")
            for k in (5, 15, 21, 31):      # a long read with N at every k-th base: no window of k without one
                s = ACGT[rng.integers(0, 4, size=900)].copy()
                s[k - 1::k] = ord("N")
                seqs.append(s.tobytes())
            seqs += [seqs[10], seqs[11]]   # a few k-mers seen twice
        elif name in ("fives1", "fives2"):
            seqs = all_5mers(1 if name == "fives1" else 2)
        else:
            raise KeyError(name)
        _batches[name] = Batch(name, seqs)
    return _batches[name]


# (batch, k, log2_once, log2_twice): the smallest filters on every batch, and for the genome's reads - whose k-mers seen
# once outnumber the 2^16 bits of the smallest filter several times, so that every one of them is a false positive there -
# one filter in which the false positives are a minority: 2^14 and 2^12 words (`twice` a quarter of `once`, as the command
# line sizes them).  SELECTIVE holds, per batch, the cases whose E is held to a quarter of the k-mers seen once.
SMALLEST = ((10, 10), (12, 10))
CASES = ([("noisy", k, a, b) for k in (15, 21, 31) for a, b in SMALLEST + ((14, 12),)] +
         [("noisy", 5, 10, 10), ("twins", 31, 10, 10), ("twins", 21, 14, 12), ("apart", 31, 12, 10), ("apart", 15, 14, 12),
          ("homo", 31, 10, 10), ("homo", 5, 12, 10), ("homo", 15, 10, 10),
          ("short", 5, 10, 10), ("short", 15, 12, 10), ("short", 21, 10, 10), ("short", 31, 10, 10),
          ("fives1", 5, 10, 10), ("fives1", 5, 12, 10), ("fives2", 5, 10, 10), ("fives2", 5, 12, 10)])
SELECTIVE = [c for c in CASES if c[0] not in ("noisy", "twins", "apart") or (c[2], c[3]) == (14, 12) or c[1] == 5]

_models = {}


def table_of(oracle, name, k):
    key = ("table", name, k)
    if key not in _models:
        b = batch(name)
        _models[key] = oracle.count_reads(b.bases, b.offsets, k)
    return _models[key]


def model(oracle, name, k, a, b):
    key = (name, k, a, b)
    if key not in _models:
        keys, counts = table_of(oracle, name, k)
        _models[key] = Model(keys, counts, a, b)
    return _models[key]
