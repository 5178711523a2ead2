"""The heterozygous k-mer pairs of a k-mer table (kt_ctr_hetmers, `kmertools hetmers`), restated twice: in numpy over a
sorted (keys, counts) table - every one-substitution variant of every solid k-mer made as a string of bits, canonicalised
by its own reverse complement and looked up with searchsorted - and as a string-level brute force over a dict.  The rule
(include/kmertools_hip.h): a node is a canonical k-mer with lo <= count <= hi; N(u) is the SET of solid canonical k-mers
that one substitution of u's forward string at an allowed position leads to, u itself removed; {u, v} is a pair when
N(u) = {v} and N(v) = {u}, written (a, b) with a < b.  And the files of `kmertools hetmers`, restated from the pairs."""
import numpy as np

U32 = 0xFFFFFFFF
CENSUS_NAMES = ["nodes", "occurrences", "degree_0", "degree_1", "degree_2_or_more", "pairs", "minor_sum", "major_sum"]
COMP = {"A": "T", "C": "G", "G": "C", "T": "A"}


def key_of(s):
    v = 0
    for ch in s:
        v = v << 2 | "ACGT".index(ch)
    return v


def str_of(v, k):
    return "".join("ACGT"[int(v) >> 2 * (k - 1 - i) & 3] for i in range(k))


def rc_s(s):
    return "".join(COMP[ch] for ch in reversed(s))


def canon_s(s):
    return min(s, rc_s(s))


def rc_np(x, k):
    """the reverse complement of every k-mer of a u64 array, base by base"""
    x = np.asarray(x, np.uint64).copy()
    out = np.zeros_like(x)
    for _ in range(k):
        out = (out << np.uint64(2)) | (np.uint64(3) - (x & np.uint64(3)))
        x >>= np.uint64(2)
    return out


def rc_fast(x, k):
    """the same by swapping bit groups (the CPU tests pin it to rc_np)"""
    u = np.uint64
    x = ~np.asarray(x, np.uint64)
    for sh, m in ((2, 0x3333333333333333), (4, 0x0F0F0F0F0F0F0F0F), (8, 0x00FF00FF00FF00FF), (16, 0x0000FFFF0000FFFF)):
        x = ((x >> u(sh)) & u(m)) | ((x & u(m)) << u(sh))
    x = (x >> u(32)) | (x << u(32))
    return x >> u(64 - 2 * k)


def positions(k, middle):
    if middle:
        assert k % 2 == 1, "the middle mode needs an odd k"
        return [(k - 1) // 2]
    return list(range(k))


class Result:
    """F, c: the nodes and their counts, ascending; subs: solid substitutions per node (over positions and bases, the node
    itself not counted); deg: distinct solid neighbours; first: the smallest of them (where deg > 0); a, b, ca, cb: the pairs,
    ascending by a; census: the eight cells"""


def restate(keys, counts, k, lo=1, hi=None, middle=False):
    hi = U32 if hi is None else hi
    keys, counts = np.asarray(keys, np.uint64), np.asarray(counts, np.uint32)
    order = np.argsort(keys)
    keys, counts = keys[order], counts[order]
    solid = (counts >= lo) & (counts <= hi)
    F, c = keys[solid], counts[solid]
    n = len(F)
    r = Result()
    r.F, r.c = F, c
    P = positions(k, middle)
    none = np.uint64(0xFFFFFFFFFFFFFFFF)
    cand = np.empty((n, 3 * len(P)), np.uint64)
    for j, i in enumerate(P):
        for d in (1, 2, 3):
            f = F ^ np.uint64(d << 2 * (k - 1 - i))
            cand[:, 3 * j + d - 1] = np.minimum(f, rc_fast(f, k))
    if n:
        at = np.minimum(np.searchsorted(F, cand), n - 1)
        found = (F[at] == cand) & (cand != F[:, None])
    else:
        found = np.zeros(cand.shape, bool)
    r.subs = found.sum(axis=1)
    nb = np.sort(np.where(found, cand, none), axis=1)
    fresh = nb != none
    fresh[:, 1:] &= nb[:, 1:] != nb[:, :-1]
    r.deg = fresh.sum(axis=1)
    r.first = nb[:, 0] if nb.shape[1] else np.full(n, none)
    one = r.deg == 1
    partner = np.minimum(np.searchsorted(F, r.first), max(n - 1, 0))
    mutual = one & one[partner] if n else one
    if n:  # the rule is symmetric: a node's only neighbour has the node among its own
        assert (r.first[partner[mutual]] == F[mutual]).all()
    pick = mutual & (F < r.first)
    r.a, r.b, r.ca, r.cb = F[pick], r.first[pick], c[pick], c[partner[pick]] if n else c[pick]
    mn, mx = np.minimum(r.ca, r.cb).astype(np.uint64), np.maximum(r.ca, r.cb).astype(np.uint64)
    r.census = np.array([n, int(c.astype(np.uint64).sum()), int((r.deg == 0).sum()), int(one.sum()), int((r.deg >= 2).sum()),
                         len(r.a), int(mn.sum()), int(mx.sum())], np.uint64)
    return r


def matrix_of(ca, cb, n_rows, n_cols):
    m = np.zeros((n_rows, n_cols), np.uint64)
    mn, mx = np.minimum(ca, cb).astype(np.int64), np.maximum(ca, cb).astype(np.int64)
    np.add.at(m, (np.minimum(mn, n_rows - 1), np.minimum(mx, n_cols - 1)), 1)
    return m


def brute(table, k, lo=1, hi=U32, middle=False):
    """table: {canonical k-mer string: count} -> ([(a, b, count_a, count_b) as numbers, ascending], census list,
    {node string: sorted neighbour strings})"""
    hi = U32 if hi is None else hi
    solid = {s: c for s, c in table.items() if lo <= c <= hi}
    assert all(canon_s(s) == s and len(s) == k for s in solid)
    nbrs = {}
    for s in solid:
        N = set()
        for i in positions(k, middle):
            for ch in "ACGT":
                if ch != s[i]:
                    t = canon_s(s[:i] + ch + s[i + 1:])
                    if t != s and t in solid:
                        N.add(t)
        nbrs[s] = sorted(N)
    pairs = sorted((key_of(s), key_of(N[0]), solid[s], solid[N[0]]) for s, N in nbrs.items()
                   if len(N) == 1 and nbrs[N[0]] == [s] and s < N[0])
    deg = [len(N) for N in nbrs.values()]
    census = [len(solid), sum(solid.values()), deg.count(0), deg.count(1), sum(d >= 2 for d in deg), len(pairs),
              sum(min(p[2], p[3]) for p in pairs), sum(max(p[2], p[3]) for p in pairs)]
    return pairs, census, nbrs


def asymmetries(nbrs):
    """the (u, v) with v in N(u) but u not in N(v): none, by the rule's symmetry"""
    return [(u, v) for u, N in nbrs.items() for v in N if u not in nbrs[v]]


def written_b(a, b, k, middle):
    """b as `kmertools hetmers` writes it, and the position: b's forward string when it differs from a's at exactly one
    allowed position (the lowest), else its reverse complement"""
    for w in (int(b), int(rc_np(np.array([b], np.uint64), k)[0])):
        for i in positions(k, middle):
            x = int(a) ^ w
            if x and x & ~(3 << 2 * (k - 1 - i)) == 0:
                return w, i
    raise AssertionError("not a pair: %s %s" % (str_of(a, k), str_of(b, k)))


def want_files(keys, counts, k, lo=1, hi=None, middle=False, max_minor=500, max_major=1000):
    """(hetmers.pairs, hetmers.cov, hetmers.matrix, hetmers.stats) as bytes, and the number of pairs"""
    r = restate(keys, counts, k, lo, hi, middle)
    pairs, cov = [], []
    for a, b, ca, cb in zip(r.a.tolist(), r.b.tolist(), r.ca.tolist(), r.cb.tolist()):
        w, pos = written_b(a, b, k, middle)
        pairs.append("%s\t%s\t%d\t%d\t%d\n" % (str_of(a, k), str_of(w, k), pos, ca, cb))
        cov.append("%d\t%d\n" % (min(ca, cb), max(ca, cb)))
    m = matrix_of(r.ca, r.cb, max_minor + 1, max_major + 1)
    matrix = "".join("\t".join(map(str, row)) + "\n" for row in m.tolist())
    stats = "k\t%d\nmin_count\t%d\nmax_count\t%d\npositions\t%s\n" % (k, lo, U32 if hi is None else hi, "middle" if middle else "all")
    stats += "".join("%s\t%d\n" % (name, v) for name, v in zip(CENSUS_NAMES, r.census.tolist()))
    return "".join(pairs).encode(), "".join(cov).encode(), matrix.encode(), stats.encode(), len(r.a)


def canonical_kmers(k):
    every = np.arange(4 ** k, dtype=np.uint64)
    return every[every <= rc_np(every, k)]


def random_subset(k, density, seed):
    """a seeded random subset of all canonical k-mers with counts 1..5 -> (keys ascending, counts)"""
    rng = np.random.default_rng(seed)
    every = canonical_kmers(k)
    keys = every[rng.random(len(every)) < density]
    return keys, rng.integers(1, 6, size=len(keys)).astype(np.uint32)
