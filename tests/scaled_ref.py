"""Scaled (FracMinHash) sketches restated in numpy over the oracle's k-mers, for tests/test_scaled_sketch.py and
tests/test_scaled_sketch_cli_args.py: the hash and its inverse, the kept set of a read with its abundances, the CSR layout
kt_scaled_batch writes, unions with saturating sums, and a string-level pure-Python brute force the restatement itself is
checked against."""
import numpy as np

U = np.uint64
MASK = (1 << 64) - 1
C0, C1, C2 = 0x9E3779B97F4A7C15, 0xBF58476D1CE4E5B9, 0x94D049BB133111EB
SAT = 0xFFFFFFFF


def mix64(z):
    """ktd::mix64 (splitmix64's finaliser) over a u64 array"""
    z = np.asarray(z, np.uint64) + U(C0)
    z = (z ^ (z >> U(30))) * U(C1)
    z = (z ^ (z >> U(27))) * U(C2)
    return z ^ (z >> U(31))


def mix64_int(z):
    """the same over one Python integer"""
    z = (z + C0) & MASK
    z = ((z ^ (z >> 30)) * C1) & MASK
    z = ((z ^ (z >> 27)) * C2) & MASK
    return z ^ (z >> 31)


def _unshift(y, s):
    """x with x ^ (x >> s) == y"""
    x, t = y, y >> s
    while t:
        x ^= t
        t >>= s
    return x


def inv_mix64(h):
    """the z with mix64_int(z) == h: every xor-shift undone, the multiplications by the constants' inverses mod 2^64"""
    z = _unshift(h, 31)
    z = (z * pow(C2, -1, 1 << 64)) & MASK
    z = _unshift(z, 27)
    z = (z * pow(C1, -1, 1 << 64)) & MASK
    z = _unshift(z, 30)
    return (z - C0) & MASK


def max_hash(scaled):
    return MASK // scaled if scaled else 0


def read_hashes(oracle, bases, offsets, k, seed):
    """per read: the hashes of its windows, with multiplicity, in read order"""
    out = []
    for i in range(len(offsets) - 1):
        o, e = int(offsets[i]), int(offsets[i + 1])
        if e - o < k:
            out.append(np.zeros(0, np.uint64))
            continue
        f, r, _ = oracle.kmers(np.ascontiguousarray(bases[o:e]).tobytes(), k)
        out.append(mix64(np.minimum(f, r) ^ U(seed)).astype(np.uint64))
    return out


def rows_of(read_hashes_, scaled):
    """per read: (its windows with multiplicity, its kept hashes ascending, their abundances)"""
    out, mh = [], U(max_hash(scaled))
    for h in read_hashes_:
        u, c = np.unique(h[h <= mh], return_counts=True)
        out.append((len(h), u.astype(np.uint64), np.minimum(c, SAT).astype(np.uint32)))
    return out


def read_rows(oracle, bases, offsets, k, scaled, seed):
    return rows_of(read_hashes(oracle, bases, offsets, k, seed), scaled)


def csr(rows):
    """what kt_scaled_batch writes for such rows: (hashes, abunds, row_offsets u64[n + 1], n_kmers u32[n])"""
    offsets = np.zeros(len(rows) + 1, np.uint64)
    offsets[1:] = np.cumsum([len(h) for _, h, _ in rows])
    hashes = np.concatenate([h for _, h, _ in rows] + [np.zeros(0, np.uint64)]).astype(np.uint64)
    abunds = np.concatenate([a for _, _, a in rows] + [np.zeros(0, np.uint32)]).astype(np.uint32)
    return hashes, abunds, offsets, np.array([w for w, _, _ in rows], np.uint32)


def union(parts):
    """the union of (hashes, abunds) rows, abundances summed and saturating (abunds None: 1 each): (hashes, abunds)"""
    hs = [np.asarray(h, np.uint64) for h, _ in parts]
    ab = [np.ones(len(h), np.uint64) if a is None else np.asarray(a).astype(np.uint64) for h, a in parts]
    if not hs:
        return np.zeros(0, np.uint64), np.zeros(0, np.uint32)
    h, a = np.concatenate(hs), np.concatenate(ab)
    u, inv = np.unique(h, return_inverse=True)
    s = np.zeros(len(u), np.uint64)
    np.add.at(s, inv, a)  # (at most 2^32 rows of < 2^32 each: no u64 overflow)
    return u.astype(np.uint64), np.minimum(s, U(SAT)).astype(np.uint32)


def merge(hashes, abunds, row_offsets, group_offsets):
    """kt_scaled_merge restated: (out_hashes, out_abunds, out_offsets)"""
    ro = np.asarray(row_offsets).astype(np.int64)
    rows = []
    for g in range(len(group_offsets) - 1):
        parts = [(hashes[ro[r]:ro[r + 1]], None if abunds is None else abunds[ro[r]:ro[r + 1]])
                 for r in range(int(group_offsets[g]), int(group_offsets[g + 1]))]
        h, a = union(parts)
        rows.append((0, h, a))
    return csr(rows)[:3]


def table_sketch(keys, counts, lo, hi, scaled, seed):
    """kt_ctr_scaled restated over a table's (keys, counts): (hashes, abunds, (entries in range, their occurrences))"""
    keys, counts = np.asarray(keys, np.uint64), np.asarray(counts, np.uint32)
    m = (counts >= lo) & (counts <= hi)
    h = mix64(keys[m] ^ U(seed))
    kept = h <= U(max_hash(scaled))
    order = np.argsort(h[kept], kind="stable")
    return h[kept][order], counts[m][kept][order], (int(m.sum()), int(counts[m].astype(np.uint64).sum()))


# ---- the brute force: windows from strings, the canonical k-mer by reverse-complementing the string ------------------------
_CODE = {"A": 0, "C": 1, "G": 2, "T": 3}
_COMP = {"A": "T", "C": "G", "G": "C", "T": "A"}


def brute_row(seq, k, scaled, seed):
    """(windows, {hash: abundance}) of one upper-case string; a window over a letter outside ACGT is none"""
    mh, windows, kept = max_hash(scaled), 0, {}
    for i in range(len(seq) - k + 1):
        w = seq[i:i + k]
        if any(c not in _CODE for c in w):
            continue
        windows += 1
        rc = "".join(_COMP[c] for c in reversed(w))
        f = r = 0
        for a, b in zip(w, rc):
            f, r = f * 4 + _CODE[a], r * 4 + _CODE[b]
        h = mix64_int(min(f, r) ^ seed)
        if h <= mh:
            kept[h] = kept.get(h, 0) + 1
    return windows, kept
