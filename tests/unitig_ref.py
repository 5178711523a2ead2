"""What kt_ctr_unitigs computes, restated on strings on top of graph_ref.brute (the nodes and their info words).

The rule (the header's): a side of node u (R or L) is JOINED when its end bit is clear - it then has exactly one neighbour
string s = F[1:] + x (R) or x + F[:-1] (L) - and canon(s) != F, s is not its own reverse complement and F is not its own.
The facing side of v = canon(s) is its L side if u's R side leads to s == v, its R side if it leads to rc(s) == v (mirrored
for u's L side).  Joined sides pair up sides of distinct nodes, so the nodes fall into simple paths and simple cycles.
A path is spelled from its terminal with the smaller canonical k-mer, unjoined side first (a single node: F); a cycle from
its smallest node's F, leaving through its right side, once around (flag CIRCULAR).  n nodes spell n + k - 1 bases.
Unitigs ascend by the canonical k-mer of their start node.

Every call asserts: joins are mutual; the k-mers of all unitig strings, canonicalised, are the nodes, each exactly once;
every unitig's first k-mer canonicalises to its start key.
"""
import graph_ref as gr

CIRCULAR = 1
R, L = 0, 1


def joins(nodes, k):
    """nodes: graph_ref.brute's list -> {(i, side): (j, facing side)} over node indices (ascending key order)"""
    F_of = [gr.str_of(key, k) for key, _, _ in nodes]
    index = {F: i for i, F in enumerate(F_of)}
    link = {}
    for i, (_, _, info) in enumerate(nodes):
        F = F_of[i]
        for side, end_bit, shift in ((R, 0x100, 0), (L, 0x200, 4)):
            if info & end_bit:
                continue
            xs = [x for x in range(4) if info >> (shift + x) & 1]
            assert len(xs) == 1, (F, side, xs)
            s = F[1:] + gr.ACGT[xs[0]] if side == R else gr.ACGT[xs[0]] + F[:-1]
            v = gr.canon_s(s)
            if v == F or s == gr.rc_s(s) or F == gr.rc_s(F):
                continue
            # u's string leaves s on the left (side R) or on the right (side L); as v's reverse complement the sides swap
            facing = (L if side == R else R) if s == v else side
            link[(i, side)] = (index[v], facing)
    for (i, side), (j, facing) in link.items():
        assert i != j and link.get((j, facing)) == (i, side), ("a join is not mutual", F_of[i], side, F_of[j], facing)
    return F_of, link


def _walk(F_of, link, i, enter, stop_at=None):
    """from node i entered through side `enter`, through the joins: (string, [node indices], side the last exit was)"""
    k = len(F_of[i])
    s = F_of[i] if enter == L else gr.rc_s(F_of[i])
    seen = [i]
    while True:
        nxt = link.get((seen[-1], 1 - enter))
        if nxt is None or nxt[0] == stop_at:
            if nxt is not None:
                assert nxt[1] == L, "a cycle comes back through the side it did not leave by"
            return s, seen
        j, enter = nxt
        o = F_of[j] if enter == L else gr.rc_s(F_of[j])
        assert o[:-1] == s[-(k - 1):] if k > 1 else True
        s += o[-1]
        seen.append(j)
        assert len(seen) <= len(F_of)


def unitigs(table, k, lo=1, hi=gr.U32):
    """table: {canonical string: count} -> [(string, count_sum, flags, n_nodes)] in the library's order"""
    nodes = gr.brute(table, k, lo, hi)
    F_of, link = joins(nodes, k)
    count = [c for _, c, _ in nodes]
    done = [False] * len(nodes)
    out = []
    for i in range(len(nodes)):  # paths, from every terminal; kept from the smaller one
        open_sides = [side for side in (R, L) if (i, side) not in link]
        if not open_sides:
            continue
        enter = L if len(open_sides) == 2 else open_sides[0]
        s, seen = _walk(F_of, link, i, enter)
        assert (seen[-1] == i) == (len(seen) == 1)
        if i <= seen[-1]:
            assert not any(done[j] for j in seen)
            for j in seen:
                done[j] = True
            out.append((i, s, sum(count[j] for j in seen), 0, len(seen)))
    for i in range(len(nodes)):  # what is left lies on cycles: i is the smallest node of its own
        if done[i]:
            continue
        s, seen = _walk(F_of, link, i, L, stop_at=i)
        assert len(seen) >= 2 and min(seen) == i and not any(done[j] for j in seen)
        for j in seen:
            done[j] = True
        assert s[-(k - 1):] == s[:k - 1]
        out.append((i, s, sum(count[j] for j in seen), CIRCULAR, len(seen)))
    out.sort()
    kmers = []
    for i, s, _, _, n in out:
        assert len(s) == n + k - 1
        assert gr.canon_s(s[:k]) == F_of[i], "a unitig does not start with its start node"
        kmers += [gr.canon_s(s[j:j + k]) for j in range(n)]
    assert sorted(kmers) == F_of, "the unitigs' k-mers are not the nodes, each once"
    return [(s, c, f, n) for _, s, c, f, n in out]


def n50(lengths):
    total, run = sum(lengths), 0
    for x in sorted(lengths, reverse=True):
        run += x
        if 2 * run >= total:
            return x
    return 0


def want_files(table, k, lo=1, hi=gr.U32):
    """the reference's unitigs.fa and unitigs.stats of a table"""
    us = unitigs(table, k, lo, hi)
    fa = []
    for i, (s, c, f, n) in enumerate(us):
        fa.append(">%d LN:i:%d KC:i:%d km:f:%.1f%s\n%s\n" % (i, len(s), c, c / n, " CL:i:1" if f & CIRCULAR else "", s))
    lens = [len(s) for s, _, _, _ in us]
    stats = [("unitigs", len(us)), ("bases", sum(lens)), ("nodes", sum(n for _, _, _, n in us)),
             ("occurrences", sum(c for _, c, _, _ in us)), ("circular", sum(1 for _, _, f, _ in us if f & CIRCULAR)),
             ("singletons", sum(1 for _, _, _, n in us if n == 1)), ("longest", max(lens, default=0)), ("n50", n50(lens))]
    return "".join(fa).encode(), "".join("%s\t%d\n" % nv for nv in stats).encode()
