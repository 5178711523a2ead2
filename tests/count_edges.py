"""Counts at the edges of u32, as a fixture: plain numpy and strings, no GPU.

A k-mer's count is a u32 stored as occurrences - 1 (kt_table.hpp).  fixture(k) is a small de Bruijn graph - a seeded backbone
with bubbles and side branches, a few dead ends of 1..4 nodes, one cycle and one isolated piece - whose canonical k-mers come
from oracle.kt_oracle.count_reads of its contigs and whose counts are drawn from EDGES: the values on either side of every
width a count could be carried in by mistake (8, 16, 24, 31, 32 bits) and of the signed boundary.  On top of the seeded
permutation one unitig of at least three nodes has every node at 2^32 - 1 (its count sum exceeds 2^33) and three pairs of
adjacent k-mers straddle 2^16, 2^24 and 2^31 (one of the pair below the boundary, the other at it).  The builder asserts
these conditions.  A batch of reads walks the graph - with N, lower case, a read shorter than k, an empty read and k-mers the
table does not hold - for the calls that take reads.

tip_cases() builds the Y-shaped graphs by hand whose two dead ends compete at this scale: equal means, sums one apart at
2^32, and means that a comparison in double or float gets wrong (the pair of 65 537-node dead ends whose cross products pass
2^64 is made in tests/test_count_edges.py, on arrays: it is too large for strings).
"""
import functools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import graph_ref as gr  # noqa: E402
import unitig_ref as ur  # noqa: E402

U32 = 0xFFFFFFFF
EDGES = (1, 2, 255, 256, 65535, 65536, 2 ** 24 - 1, 2 ** 24, 2 ** 24 + 1, 2 ** 31 - 1, 2 ** 31, 2 ** 31 + 1, 2 ** 32 - 2,
         2 ** 32 - 1)
KS = (31, 15, 9)
STRADDLES = (2 ** 16, 2 ** 24, 2 ** 31)
ACGT = "ACGT"


def rand_seq(rng, n):
    return "".join(ACGT[i] for i in rng.integers(0, 4, size=n))


def contigs_of(k, seed):
    """the strings whose k-mers are the graph"""
    rng = np.random.default_rng(seed)
    back = rand_seq(rng, 2400 + k)
    out = [back]
    at = rng.choice(np.arange(50, 2300), 24, replace=False)
    for i, p in enumerate(at[:12]):  # side branches; every other one comes back to the backbone (a bubble)
        p = int(p)
        s = back[p:p + k - 1] + rand_seq(rng, int(rng.integers(40, 90)))
        if i % 2 == 0:
            q = min(p + int(rng.integers(30, 120)), len(back) - k)
            s += back[q:q + k - 1]
        out.append(s)
    for j, p in enumerate(at[12:20]):  # short dead ends: 1..4 nodes off the backbone
        p = int(p)
        out.append(back[p:p + k - 1] + rand_seq(rng, 1 + j % 4))
    c = rand_seq(rng, 70)
    out.append(c + c[:k - 1])  # a cycle of 70 nodes
    out.append(rand_seq(rng, 45 + k - 1))  # an isolated piece
    return out


def to_csr(seqs):
    from oracle import kt_oracle
    return kt_oracle.to_csr(seqs)


def strings_of(keys, counts, k):
    """{canonical string: Python int} of a table's arrays"""
    return {gr.str_of(key, k): int(c) for key, c in zip(keys.tolist(), counts.tolist())}


def adjacent(a, b):
    """two canonical k-mer strings that follow each other in the de Bruijn graph (either strand of either)"""
    return any(x[1:] == y[:-1] or y[1:] == x[:-1] for x in (a, gr.rc_s(a)) for y in (b, gr.rc_s(b)))


class Fixture:
    pass


@functools.lru_cache(maxsize=None)
def fixture(k):
    from oracle import kt_oracle
    fx = Fixture()
    fx.k = k
    fx.contigs = [c.encode() for c in contigs_of(k, 7000 + k)]
    fx.csr = to_csr(fx.contigs)
    keys, built = kt_oracle.count_reads(fx.csr[0], fx.csr[1], k)
    order = np.argsort(keys)
    fx.keys, fx.built = keys[order], built[order]  # (built: what counting the contigs as reads gives)
    n = len(fx.keys)
    assert 3000 <= n <= 6000, n
    rng = np.random.default_rng(7100 + k)
    counts = np.array(EDGES, np.uint64)[np.arange(n) % len(EDGES)][rng.permutation(n)]
    # the unitigs of the key set (every count in range: the topology is the keys' alone)
    names = [gr.str_of(key, k) for key in fx.keys.tolist()]
    index = {s: i for i, s in enumerate(names)}
    us = ur.unitigs({s: 1 for s in names}, k)
    nodes_of = lambda u: [index[gr.canon_s(u[0][j:j + k])] for j in range(u[3])]  # noqa: E731
    # (k = 9: 3 500 of the 131 072 canonical 9-mers - chance neighbours branch the cycle's walk, it is no unitig there)
    assert k < 15 or any(u[2] & ur.CIRCULAR for u in us), "no cycle"
    assert sum(1 for u in us if u[3] <= 4) >= 4, "no short dead ends"
    big = next(i for i, u in enumerate(us) if 3 <= u[3] <= 40 and not u[2])
    fx.big_nodes = nodes_of(us[big])
    counts[fx.big_nodes] = U32
    two = [i for i, u in enumerate(us) if u[3] >= 2 and i != big][:len(STRADDLES)]
    fx.straddle = {}
    for b, i in zip(STRADDLES, two):
        lo_i, hi_i = nodes_of(us[i])[:2]
        counts[lo_i], counts[hi_i] = b - 1, b
        fx.straddle[b] = (int(fx.keys[lo_i]), int(fx.keys[hi_i]))
    # a bulk build of the contigs leaves fx.built, and add_pairs raises that to the edge: no count below what the contigs
    # themselves count (a k-mer that two contigs share gets the next edge value up)
    edges = np.array(EDGES, np.uint64)
    at_least = lambda c: np.where(c < fx.built, edges[np.searchsorted(edges, fx.built)], c).astype(np.uint32)  # noqa: E731
    fx.counts = at_least(counts)
    fx.counts_b = at_least(counts[np.random.default_rng(7200 + k).permutation(n)])  # the second table: the same keys
    assert (fx.counts >= fx.built).all() and (fx.counts_b >= fx.built).all()
    fx.table = strings_of(fx.keys, fx.counts, k)
    fx.table_b = strings_of(fx.keys, fx.counts_b, k)
    check_conditions(fx)
    fx.reads = reads_of(fx)
    fx.reads_csr = to_csr(fx.reads)
    check_reads(fx)
    return fx


def check_conditions(fx):
    """what the issue asks of the counts - from the final arrays, not from how they were made"""
    k = fx.k
    assert fx.counts.dtype == np.uint32 and len(fx.counts) == len(fx.keys) and (fx.keys[1:] > fx.keys[:-1]).all()
    for e in EDGES:
        assert int((fx.counts == e).sum()) >= 8 and int((fx.counts_b == e).sum()) >= 8, e
    assert set(fx.counts.tolist()) == set(EDGES)
    us = ur.unitigs(fx.table, k)
    full = [u for u in us if u[3] >= 3 and u[1] == u[3] * U32]
    assert full and full[0][1] > 2 ** 33 and isinstance(full[0][1], int), "no unitig with every node at 2^32 - 1"
    fx.big_sum = max(u[1] for u in full)
    for b in STRADDLES:
        lo_key, hi_key = fx.straddle[b]
        a, c = gr.str_of(lo_key, k), gr.str_of(hi_key, k)
        assert adjacent(a, c) and fx.table[a] == b - 1 and fx.table[c] == b, b
    fx.unitigs = us


def reads_of(fx):
    """a batch that walks the graph: pieces of the contigs (either strand), some with N or lower case, the short contigs
    whole, a read shorter than k, an empty one, reads of k-mers the table does not hold"""
    k = fx.k
    rng = np.random.default_rng(7300 + k)
    out = []
    for c in fx.contigs:
        if len(c) <= 200:
            out.append(c)
    back = fx.contigs[0]
    for i in range(36):
        src = back if i % 3 else fx.contigs[1 + i % 12]
        L = min(int(rng.integers(k + 1, 140)), len(src))
        a = int(rng.integers(0, len(src) - L + 1))
        s = np.frombuffer(src[a:a + L], np.uint8).copy()
        if i % 4 == 1:
            s = np.frombuffer(gr.rc_s(s.tobytes().decode()).encode(), np.uint8).copy()
        if i % 5 == 2:
            s[int(rng.integers(0, L))] = ord("N")
        if i % 7 == 3:
            s = np.frombuffer(s.tobytes().lower(), np.uint8).copy()
        out.append(s.tobytes())
    out += [back[:k - 1], b"", rand_seq(rng, 90).encode(), rand_seq(rng, k).encode(), b"N" * (k + 2)]
    return out


def read_kmers(fx, seq):
    """(canonical keys, start positions) of a read's valid windows"""
    from oracle import kt_oracle
    f, r, end = kt_oracle.kmers(seq, fx.k)
    return np.minimum(f, r), end.astype(np.int64) - (fx.k - 1)


def count_of(keys, counts, q):
    """counts of the k-mers q in the sorted table (0: absent), u32"""
    q = np.asarray(q, np.uint64)
    i = np.minimum(np.searchsorted(keys, q), len(keys) - 1)
    return np.where(keys[i] == q, counts[i], 0).astype(np.uint32)


def check_reads(fx):
    seen = np.concatenate([count_of(fx.keys, fx.counts, read_kmers(fx, s)[0]) for s in fx.reads])
    assert set(EDGES) <= set(seen.tolist()), "the reads miss an edge value"
    assert int((seen == 0).sum()) >= 20, "the reads hold no k-mers absent from the table"
    assert any(b"N" in s for s in fx.reads) and any(0 < len(s) < fx.k for s in fx.reads) and b"" in fx.reads
    assert int(fx.reads_csr[1][-1]) < 20000


# ---- the Y-shaped graphs: two dead ends at one fork ---------------------------------------------------------------------------

def unique_kmers(seqs, k):
    """every k-mer of the strings, canonical, occurs once over all of them"""
    seen = [gr.canon_s(s[j:j + k]) for s in seqs for j in range(len(s) - k + 1)]
    return len(set(seen)) == len(seen)


def y_graph(k, n_u, n_w, seed, trunk=40):
    """a trunk of `trunk` nodes (longer than any tip) whose right end forks into two dead ends of n_u and n_w nodes: returns
    (trunk, branch_u, branch_w) as lists of canonical k-mer strings in walking order.  The branches differ in the first
    base after the fork."""
    rng = np.random.default_rng(seed)
    for _ in range(64):
        t = rand_seq(rng, trunk + k - 1)
        bu, bw = rand_seq(rng, n_u), rand_seq(rng, n_w)
        if bu[0] == bw[0]:
            continue
        su, sw = t[-(k - 1):] + bu, t[-(k - 1):] + bw
        if unique_kmers([t, su, sw], k):
            walk = lambda s: [gr.canon_s(s[j:j + k]) for j in range(len(s) - k + 1)]  # noqa: E731
            return walk(t), walk(su), walk(sw)
    raise AssertionError("no Y graph found")


def spread(total, n, top=U32):
    """n counts in 1..top whose sum is `total`"""
    assert n <= total <= n * top
    base, extra = divmod(total, n)
    out = [base + 1] * extra + [base] * (n - extra)
    assert sum(out) == total and 1 <= min(out) and max(out) <= top
    return out


def float_trap(n):
    """sums (c_u over n nodes, c_w over n + 1) with c_w / (n + 1) > c_u / n exactly, by the smallest margin the integers
    allow - c_w * n - c_u * (n + 1) == 1 - at the 2^32 scale.  The quotients agree to about 2 / (n^2 2^32) of their value:
    far below half an ulp of a float, and for the n that tip_cases() picks (_float_fails) the two divisions in double
    come out equal or the wrong way round too.  The 128-bit cross product is exact."""
    # c_w * n = c_u * (n + 1) + 1: with c_u = n * t - 1, c_w = (n + 1) * t - 1 (then c_w n - c_u (n + 1) = -n + n + 1 = 1)
    t = U32 - 1
    c_u, c_w = n * t - 1, (n + 1) * t - 1
    assert c_w * n - c_u * (n + 1) == 1
    return c_u, c_w


@functools.lru_cache(maxsize=None)
def tip_cases(k=15):
    """name -> dict(table {canonical string: count}, u / w: the two dead ends' k-mers, loser: which one must be the tip
    (None: the one with the higher unitig number), max_tip_nodes, sums)"""
    out = {}

    def case(name, n_u, n_w, c_u, c_w, seed, loser):
        t, bu, bw = y_graph(k, n_u, n_w, seed, trunk=max(n_u, n_w) + 30)  # (the trunk is never short: max_tip_nodes is
        table = {s: 1000 for s in t}                                       #  the longer branch's nodes)
        table.update(zip(bu, spread(c_u, n_u)))
        table.update(zip(bw, spread(c_w, n_w)))
        out[name] = dict(table=table, u=bu, w=bw, loser=loser, max_tip_nodes=max(n_u, n_w), sums=(n_u, c_u, n_w, c_w))

    # equal means at the top of the range: the lower unitig number stays - which branch that is depends on the unitigs'
    # order (by their smaller terminal's k-mer), so the loser is taken from the restated numbering in the test
    case("equal means", 3, 6, 3 * (U32 - 5), 6 * (U32 - 5), 11, None)
    # sums one apart at the 2^32 scale, the same number of nodes
    case("sums one apart", 4, 4, 4 * (U32 - 7), 4 * (U32 - 7) + 1, 12, "u")
    # n and n + 1 nodes, the exact means 1 / (n (n + 1)) apart: below half an ulp of a double at 2^32 from n ~ 1450 on
    n = next(n for n in range(1000, 6000) if _float_fails(n))
    c_u, c_w = float_trap(n)
    case("float trap", n, n + 1, c_u, c_w, 13, "u")
    return out


def _float_fails(n):
    c_u, c_w = float_trap(n)
    in_double = float(c_w) / (n + 1) <= float(c_u) / n
    in_float = np.float32(c_w) / np.float32(n + 1) <= np.float32(c_u) / np.float32(n)
    return bool(in_double and in_float)
