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
import collections
import functools
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

class Geometry(collections.namedtuple("Geometry", "cap n m8 range_slots n_ranges")):
    """a table's shape (kt_table.hpp kttab::Geom): cap slots addressed by the top n hash bits, n_ranges ranges of range_slots
    slots each (1024 * m8, or the whole table when it has fewer than 8192 slots)"""
    __slots__ = ()

    @property
    def shift(self):
        return 64 - self.n


def geometry(cap_request, k=0):
    """make_geom restated: the request rounded up to a power of two of at least 1024 slots and, from 2^15 slots on, down to
    the least of 5..8 eighths of it that still holds the request (k does not change the shape: it selects the hash)"""
    p, n = 1024, 10
    while p < cap_request:
        p, n = p << 1, n + 1
    m8 = 8
    if n >= 15:
        while m8 > 5 and p // 8 * (m8 - 1) >= cap_request:
            m8 -= 1
    cap = p // 8 * m8
    rs = cap if n < 13 else 1024 * m8
    return Geometry(cap, n, m8, rs, cap // rs)


def home_of(keys, k, geom):
    """(range, position inside it) of the home slot of canonical k-mers in a table of shape `geom` - a Geometry, or the
    log2 of a whole power of two of at least 2^15 slots (ranges of 8192 slots).  k <= 16: the top bits of nhash, a
    bijection of the 2k-bit words; else of khash.  A table of fewer than 8192 slots is one range, the position the top n
    bits themselves; else the top n - 13 bits are the range and the low 13, scaled to the range's 1024 * m8 slots, the
    position (probe_of)."""
    keys = np.asarray(keys, np.uint64)
    if not isinstance(geom, Geometry):
        assert geom >= 15
        geom = Geometry(1 << geom, geom, 8, 8192, 1 << (geom - 13))
    n = geom.n
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
    x = x.astype(np.int64)
    if n < 13:
        return np.zeros(len(x), np.int64), x
    return x >> 13, ((x & 8191) * geom.m8) >> 3


def hash_inverse(x, k):
    """the k-mer word whose hash is x (khash_inv / nhash_inv): for k > 16 x is the whole 64-bit khash; for k <= 16 the
    2k-bit nhash.  Not every word that comes back is a k-mer (k > 16: below 4^k) or canonical: the caller keeps those."""
    x = np.asarray(x, np.uint64)
    if k <= 16:
        kb = 2 * k
        t = (x << np.uint64(32 - kb)) & np.uint64(0xFFFFFFFF)
        t ^= t >> np.uint64(kb >> 1)  # (the fold is its own inverse)
        return ((t >> np.uint64(32 - kb)) * np.uint64(0x0E8B2F51)) & np.uint64((1 << kb) - 1)
    h = x ^ (x >> np.uint64(32))
    return h * np.uint64(0xF1DE83E19937733D)  # (wraps modulo 2^64: the inverse of 0x9E3779B97F4A7C15)


def keys_built_at(k, geom, rng_range, position, n, rng):
    """n distinct canonical k-mers (ascending) whose home slot lies in range `rng_range` at `position` - one position, a
    window (first, last) or None for anywhere in the range - BUILT from the hash's inverse, not searched for: the top
    geom.n bits of the hash are chosen (the range, and 13 bits below it that scale to a wanted position), the bits below
    are drawn from `rng` until enough of the words that come back are canonical k-mers - k = 31: one in eight; a khash word
    is a k-mer once in 4^(32 - k), so for 16 < k < 28 or so this is no way to get keys.  What keys_homed_at cannot do on a
    table of 2^20 ranges."""
    g = geom
    assert g.n >= 13 and 0 <= rng_range < g.n_ranges
    lo, hi = (0, g.range_slots - 1) if position is None else position if isinstance(position, tuple) else (position, position)
    low13 = np.arange(8192, dtype=np.int64)
    low13 = low13[((low13 * g.m8) >> 3 >= lo) & ((low13 * g.m8) >> 3 <= hi)]
    assert len(low13), "no hash bits give a position in %d..%d of a range of %d slots" % (lo, hi, g.range_slots)
    width = 2 * k if k <= 16 else 64  # bits of the hash word
    assert width >= g.n
    free = width - g.n
    found = np.zeros(0, np.uint64)
    for _ in range(200):
        m = 16 * n + 64
        top = (np.uint64(rng_range) << np.uint64(13)) | rng.choice(low13, m).astype(np.uint64)
        x = top << np.uint64(free)
        if free:
            x |= rng.integers(0, 1 << free, size=m, dtype=np.uint64)
        key = hash_inverse(x, k)
        if k > 16:
            key = key[key < np.uint64(1 << (2 * k))]
        key = key[key <= gr.rc_np(key, k)]
        found = np.unique(np.concatenate([found, key]))
        if len(found) >= n:
            break
    assert len(found) >= n, "only %d of %d keys built at (%d, %s)" % (len(found), n, rng_range, position)
    return np.sort(rng.choice(found, n, replace=False))


class Layout:
    """where linear probing puts keys: per key its range, home position, slot and displacement and whether its probe
    sequence passed the range's end; per range how many keys it holds"""


def layout(keys, k, geom):
    """the keys placed range by range, in the order given: each goes to the first free slot from its home position on,
    circularly inside its range.  Which slots end up taken, and how many keys pass a range's end, does not depend on the
    order.  Raises when a range gets more keys than it has slots."""
    keys = np.asarray(keys, np.uint64)
    if not isinstance(geom, Geometry):
        geom = Geometry(1 << geom, geom, 8, 8192, 1 << (geom - 13))
    rs = geom.range_slots
    L = Layout()
    L.range, L.home = home_of(keys, k, geom)
    L.fill = np.bincount(L.range, minlength=geom.n_ranges)
    assert len(L.fill) == geom.n_ranges and (L.fill <= rs).all(), "a range holds more keys than slots"
    L.slot = np.zeros(len(keys), np.int64)
    by_range = np.argsort(L.range, kind="stable")  # (the keys of a range in the order given; a table may have 2^20 ranges)
    starts = np.concatenate([[0], np.cumsum(L.fill)])
    for r in np.flatnonzero(L.fill):
        members = by_range[starts[r]:starts[r + 1]]
        if len(members) == 1:  # (alone in its range: at home)
            L.slot[members[0]] = L.home[members[0]]
            continue
        nxt = list(range(rs + 1))  # nxt[s]: a slot >= s that may be free (followed to a fixed point); rs: past the end
        for i, h in zip(members.tolist(), L.home[members].tolist()):
            s = h
            while True:
                path = []
                while nxt[s] != s:
                    path.append(s)
                    s = nxt[s]
                for q in path:
                    nxt[q] = s
                if s < rs:
                    break
                s = 0  # (past the range's last slot: on from its first)
            nxt[s] = s + 1
            L.slot[i] = s
    L.wrapped = L.slot < L.home
    L.displacement = np.where(L.wrapped, L.slot + rs - L.home, L.slot - L.home)
    return L


def canonical_keys(rng, k, n):
    """n random canonical k-mers (distinct, ascending)"""
    x = rng.integers(0, 1 << (2 * k), size=2 * n + 16, dtype=np.uint64)
    return np.sort(rng.choice(np.unique(gr.canon_np(x, k)), n, replace=False))


class _Pool:
    """the random canonical k-mers keys_homed_at searches: one stream per (k, seed), its draws kept (16 MB each; a search
    rarely needs a third), so that every geometry and window of a test module searches the same arrays"""

    def __init__(self, k, seed):
        self.k, self.rng, self.drawn = k, np.random.default_rng(seed), []

    def draw(self, i):
        while len(self.drawn) <= i:
            x = self.rng.integers(0, 1 << (2 * self.k), size=1 << 22, dtype=np.uint64)
            x = x[x <= gr.rc_np(x, self.k)]
            x.setflags(write=False)
            self.drawn.append(x)
        return self.drawn[i]


@functools.lru_cache(maxsize=4)
def _pool(k, seed):
    return _Pool(k, seed)


def keys_homed_at(k, geom, rng_range, position, n, seed=7):
    """n distinct canonical k-mers (ascending) whose home slot lies in range `rng_range` at `position` - one position, or
    a window (first, last) of positions, None for anywhere in the range - by search over random k-mers"""
    lo, hi = (0, 1 << 62) if position is None else position if isinstance(position, tuple) else (position, position)
    found = np.zeros(0, np.uint64)
    for i in range(64):
        x = _pool(k, seed).draw(i)
        r, p = home_of(x, k, geom)
        found = np.unique(np.concatenate([found, x[(r == rng_range) & (p >= lo) & (p <= hi)]]))
        if len(found) >= n:
            return found[:n]
    raise AssertionError("no %d keys homed at (%d, %s)" % (n, rng_range, position))
