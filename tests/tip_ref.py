"""What kt_ctr_unitig_tips and kt_ctr_clip_tips compute, restated on top of unitig_link_ref.links (the unitigs and their
links) and dict deletion (the erase).

The rule (the header's).  n_u = nodes of unitig u, c_u = its count sum.  End e = 2u + (sign is '-') owns links[e], values
f = 2v + (sv is '-'); a link e -> f arrives at end f ^ 1 of unitig f >> 1, its mirror is (f ^ 1) -> (e ^ 1).  u is SHORT when it
is not circular and n_u <= max_tip_nodes.
  - a short u with no link at either end is ISOLATED;
  - a short u with no link at exactly one end is a CANDIDATE, e its live end;
  - w BEATS a candidate u when w is no candidate, or when c_w / n_w > c_u / n_u, or the two are equal and w < u (exact:
    Python integers);
  - a candidate u is a TIP when for EVERY link f of its live end, end g = f ^ 1 has a link h != e ^ 1 whose unitig beats u;
  - everything else is kept.

marks() asserts on every call that every marked unitig is short, non-circular and dead at the right ends, and the invariant:
an end of an unmarked unitig that had links keeps at least one of them among the unmarked unitigs.
marks_of_arrays() is the rule again with numpy on a call's own (offsets, count_sums, flags, link_offsets, link_to), for
tables too large for strings.
"""
import numpy as np

import graph_ref as gr
import unitig_link_ref as lr
import unitig_ref as ur

KEEP, TIP, ISOLATED = 0, 1, 2
STATS = ("rounds", "tips", "tip_nodes", "isolated", "isolated_nodes", "occurrences", "converged")


def marks_of(n, c, circ, ls, max_tip_nodes):
    """n, c: nodes and count sum per unitig, circ: is a cycle, ls: the links of every end -> [mark per unitig]"""
    nu = len(n)
    short = [not circ[u] and n[u] <= max_tip_nodes for u in range(nu)]
    live = {}  # candidate -> its live end
    out = [KEEP] * nu
    for u in range(nu):
        if not short[u]:
            continue
        if not ls[2 * u] and not ls[2 * u + 1]:
            out[u] = ISOLATED
        elif not ls[2 * u] or not ls[2 * u + 1]:
            live[u] = 2 * u if ls[2 * u] else 2 * u + 1

    def beats(w, u):
        if w not in live:
            return True
        a, b = c[w] * n[u], c[u] * n[w]
        return a > b or (a == b and w < u)

    for u, e in live.items():
        if all(any(h != e ^ 1 and beats(h >> 1, u) for h in ls[f ^ 1]) for f in ls[e]):
            out[u] = TIP
    # what every answer has to satisfy, whatever the rule's wording
    for u in range(nu):
        if out[u] != KEEP:
            assert short[u] and not circ[u]
            dead = [not ls[2 * u], not ls[2 * u + 1]]
            assert dead == [True, True] if out[u] == ISOLATED else sorted(dead) == [False, True], (u, out[u], dead)
        else:
            for e in (2 * u, 2 * u + 1):
                assert not ls[e] or any(out[f >> 1] == KEEP for f in ls[e]), ("an end lost all its links", e, ls[e])
    return out


def marks(table, k, max_tip_nodes, lo=1, hi=gr.U32):
    """table: {canonical string: count} -> (unitigs, links, [mark per unitig], tally of 4)"""
    us, ls = lr.links(table, k, lo, hi)
    m = marks_of([u[3] for u in us], [u[1] for u in us], [bool(u[2] & ur.CIRCULAR) for u in us], ls, max_tip_nodes)
    return us, ls, m, tally_of(m, [u[3] for u in us])


def tally_of(m, n):
    return [sum(1 for x in m if x == TIP), sum(y for x, y in zip(m, n) if x == TIP),
            sum(1 for x in m if x == ISOLATED), sum(y for x, y in zip(m, n) if x == ISOLATED)]


def nodes_of(us, k, which):
    """the canonical k-mers of the unitigs whose index is in `which`"""
    return [gr.canon_s(us[u][0][j:j + k]) for u in which for j in range(us[u][3])]


def clip(table, k, max_tip_nodes, max_rounds=8, drop_isolated=False, lo=1, hi=gr.U32):
    """-> (the reduced table: a new dict, the stats as kt_ctr_clip_tips fills them (8), the marks of every round made)"""
    table = dict(table)
    s = [0] * 8
    rounds = []
    for _ in range(max_rounds):
        us, ls, m, t = marks(table, k, max_tip_nodes, lo, hi)
        rounds.append(m)
        gone = [u for u, x in enumerate(m) if x == TIP or (drop_isolated and x == ISOLATED)]
        if not gone:
            s[6] = 0
            break
        for key in nodes_of(us, k, gone):
            del table[key]
        s[0] += 1
        s[1], s[2] = s[1] + t[0], s[2] + t[1]
        if drop_isolated:
            s[3], s[4] = s[3] + t[2], s[4] + t[3]
        s[5] += sum(us[u][1] for u in gone)
        s[6] = 1
    return table, s, rounds


def want_clip_stats(s):
    """unitigs.clip.stats of the stats of a call"""
    vals = list(s[:6]) + [1 - s[6]]
    return "".join("%s\t%d\n" % nv for nv in zip(STATS, vals)).encode()


def marks_of_arrays(offsets, count_sums, flags, link_offsets, link_to, k, max_tip_nodes):
    """the rule on the arrays of a kt_ctr_unitigs_linked call -> (marks u8, tally u64[4])"""
    off = np.asarray(offsets, np.int64)
    nu = len(off) - 1
    n = off[1:] - off[:-1] - (k - 1)
    c = np.asarray(count_sums, np.uint64)
    lo = np.asarray(link_offsets, np.int64)
    to = np.asarray(link_to, np.int64)
    deg = lo[1:] - lo[:-1]
    short = ((np.asarray(flags) & ur.CIRCULAR) == 0) & (n <= max_tip_nodes)
    dp, dm = deg[0::2], deg[1::2]
    iso = short & (dp == 0) & (dm == 0)
    cand = short & ((dp == 0) != (dm == 0))
    live = 2 * np.arange(nu) + (dp == 0)  # (of a candidate)
    out = np.zeros(nu, np.uint8)
    out[iso] = ISOLATED
    for u in np.flatnonzero(cand):  # few enough: a candidate is a short dead end
        e = int(live[u])
        tip = True
        for f in to[lo[e]:lo[e + 1]]:
            g = int(f) ^ 1
            beaten = False
            for h in to[lo[g]:lo[g + 1]]:
                w = int(h) >> 1
                if int(h) == e ^ 1:
                    continue
                if not cand[w]:
                    beaten = True
                else:
                    a, b = int(c[w]) * int(n[u]), int(c[u]) * int(n[w])
                    beaten = a > b or (a == b and w < u)
                if beaten:
                    break
            if not beaten:
                tip = False
                break
        if tip:
            out[u] = TIP
    tally = np.array([np.sum(out == TIP), n[out == TIP].sum(), np.sum(out == ISOLATED), n[out == ISOLATED].sum()], np.uint64)
    return out, tally
