"""A k-mer table as plain numpy: {canonical key: occurrences} held as sorted u64 / u32 arrays, with the C ABI's update
arithmetic (add_reads = the oracle's count_reads of the batch merged in, add_pairs = counts added per key, clear) and an
answer for every call that reads a table - the restatements the reader tests already have, imported, not rewritten:

  graph                 tests/graph_ref.py            restate
  setop                 tests/test_ctr_setop.py       want_setop
  compare               tests/test_ctr_compare.py     want_compare
  spectrum              tests/test_ctr_spectrum.py    want_spectrum
  profile               tests/test_profile.py         want_profile
  lookup, export,       a binary search in the sorted keys, a mask over the counts
  the filtered stage

A Model is also the `Table` those restatements take (keys, counts, count(keys)).  tests/test_table_lifecycle.py walks one
kt_ctr and one Model through the same calls and compares every reader with it; the table's hash is restated here too
(home_of), for the one thing a reference of the CONTENT cannot say: which keys' probe sequences wrap at a range's end."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import graph_ref as gr  # noqa: E402
from test_ctr_compare import want_compare  # noqa: E402
from test_ctr_setop import want_setop  # noqa: E402
from test_ctr_spectrum import want_spectrum  # noqa: E402
from test_profile import want_profile  # noqa: E402

U32 = 0xFFFFFFFF


class Model:
    def __init__(self, k, keys=None, counts=None):
        self.k = k
        self.keys = np.zeros(0, np.uint64) if keys is None else np.asarray(keys, np.uint64).copy()
        self.counts = np.zeros(0, np.uint32) if counts is None else np.asarray(counts, np.uint32).copy()
        assert len(self.keys) == len(self.counts) and (self.keys[1:] > self.keys[:-1]).all() and (self.counts >= 1).all()

    def copy(self):
        return Model(self.k, self.keys, self.counts)

    # ---- updates ------------------------------------------------------------------------------------------------------
    def _merge(self, keys, counts):
        keys = np.concatenate([self.keys, np.asarray(keys, np.uint64)])
        counts = np.concatenate([self.counts.astype(np.uint64), np.asarray(counts, np.uint64)])
        uk, inv = np.unique(keys, return_inverse=True)
        uc = np.zeros(len(uk), np.uint64)
        np.add.at(uc, inv, counts)
        assert (uc <= U32).all(), ("more than 0xFFFFFFFF occurrences of a k-mer: past the exactness limit the result is "
                                   "unspecified (include/kmertools_hip.h, kt_ctr_add_reads)")
        self.keys, self.counts = uk, uc.astype(np.uint32)

    def add_reads(self, bases, offsets):
        from oracle import kt_oracle
        self._merge(*kt_oracle.count_reads(np.ascontiguousarray(bases, np.uint8), np.ascontiguousarray(offsets, np.uint64), self.k))

    def add_pairs(self, keys, counts):
        keys, counts = np.asarray(keys, np.uint64), np.asarray(counts, np.uint32)
        some = counts >= 1  # (a pair with count 0 adds nothing: its key stays absent if the table does not hold it)
        self._merge(keys[some], counts[some])

    def clear(self):
        self.keys, self.counts = np.zeros(0, np.uint64), np.zeros(0, np.uint32)

    # ---- answers ------------------------------------------------------------------------------------------------------
    @property
    def size(self):
        return len(self.keys)

    @property
    def occurrences(self):
        return int(self.counts.astype(np.uint64).sum())

    def count(self, keys):
        """occurrences of each key, 0 when absent (kt_ctr_lookup; the `Table.count` of the reader tests' restatements)"""
        keys = np.asarray(keys, np.uint64)
        if not len(self.keys):
            return np.zeros(len(keys), np.uint32)
        i = np.minimum(np.searchsorted(self.keys, keys), len(self.keys) - 1)
        return np.where(self.keys[i] == keys, self.counts[i], 0).astype(np.uint32)

    def stage(self, lo=1, hi=None):
        """the entries with lo <= count <= hi, ascending by key (kt_ctr_export_stage_range)"""
        sel = (self.counts >= lo) & (self.counts <= (U32 if hi is None else hi))
        return self.keys[sel], self.counts[sel]

    def spectrum(self, n_bins):
        """-> (hist, (distinct, occurrences))"""
        return want_spectrum(self.counts, n_bins), (self.size, self.occurrences)

    def profile(self, seqs):
        from oracle import kt_oracle
        return want_profile(kt_oracle, seqs, self.k, self)

    def compare(self, other, n_rows, n_cols):
        """this table's rows against other's columns -> (matrix, the six totals in the ABI's order)"""
        m, tot = want_compare(self, other, n_rows, n_cols)
        return m, np.array([tot[n] for n in ("distinct_a", "distinct_b", "shared", "occurrences_a", "occurrences_b",
                                             "shared_min")], np.uint64)

    def setop(self, other, op, rule):
        return want_setop(self, other, op, rule)

    def graph(self, lo=1, hi=None):
        """-> (keys ascending, info, counts, census)"""
        return gr.restate(self.keys, self.counts, self.k, lo, hi)


# ---- the table's hash, restated (kt_device.hpp khash / nhash_top, kt_table.hpp probe_of) -----------------------------------

def home_of(keys, k, log2_slots):
    """(range, position inside it) of the home slot of canonical k-mers in a table of 2^log2_slots slots (a whole power of
    two of at least 2^15: ranges of 8192 slots).  k <= 16: the top bits of nhash, a bijection of the 2k-bit words; else of
    khash."""
    keys = np.asarray(keys, np.uint64)
    n = log2_slots
    assert n >= 15
    if k <= 16:
        kb = 2 * k
        t = ((keys & np.uint64(0xFFFFFFFF)) * np.uint64(0x9E3779B1)) & np.uint64(0xFFFFFFFF)
        t = (t << np.uint64(32 - kb)) & np.uint64(0xFFFFFFFF)
        t ^= t >> np.uint64(kb >> 1)
        x = t >> np.uint64(32 - n)  # (the 64-bit hash word is t << 32, its top n bits address the table)
    else:
        h = keys * np.uint64(0x9E3779B97F4A7C15)  # (wraps modulo 2^64)
        h ^= h >> np.uint64(32)
        x = h >> np.uint64(64 - n)
    return (x >> np.uint64(13)).astype(np.int64), (x & np.uint64(8191)).astype(np.int64)


def canonical_keys(rng, k, n):
    """n random canonical k-mers (distinct, ascending)"""
    x = rng.integers(0, 1 << (2 * k), size=2 * n + 16, dtype=np.uint64)
    return np.sort(rng.choice(np.unique(gr.canon_np(x, k)), n, replace=False))


def keys_homed_at(k, log2_slots, rng_range, position, n, seed=7):
    """n distinct canonical k-mers whose home slot is `position` of range `rng_range`, by search over random k-mers"""
    rng = np.random.default_rng(seed)
    found = np.zeros(0, np.uint64)
    for _ in range(64):
        x = rng.integers(0, 1 << (2 * k), size=1 << 22, dtype=np.uint64)
        x = x[x <= gr.rc_np(x, k)]
        r, p = home_of(x, k, log2_slots)
        found = np.unique(np.concatenate([found, x[(r == rng_range) & (p == position)]]))
        if len(found) >= n:
            return found[:n]
    raise AssertionError("no %d keys homed at (%d, %d)" % (n, rng_range, position))
