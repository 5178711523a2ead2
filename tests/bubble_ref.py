"""What kt_ctr_unitig_bubbles and kt_ctr_simplify compute, restated twice on top of unitig_link_ref.links (the unitigs and their
links), tip_ref.marks_of (the tip rule) and dict deletion (the erase).

The rule (the header's), in the tip rule's vocabulary.  n_u = nodes of unitig u, c_u = its count sum.  End e = 2u + (sign is
'-') owns links[e], values f = 2v + (sv is '-'); a link e -> f arrives at end f ^ 1 of unitig f >> 1, its mirror is
(f ^ 1) -> (e ^ 1).
  - u is a BRANCH when it is not circular, n_u <= max_bubble_nodes, end 2u has exactly one link a, end 2u + 1 exactly one
    link b, and neither leads to u itself (a >> 1 != u, b >> 1 != u);
  - branches u != w are PARALLEL when {a_u, b_u} == {a_w, b_w} as unordered pairs (w may lie the other way round between
    the same two ends): an equivalence, every branch is in exactly one class;
  - w OUTRANKS u when c_w / n_w > c_u / n_u, or the two are equal and w < u (exact: Python integers);
  - a branch is POPPED when some parallel branch outranks it: exactly one branch of every class stays.

  definition  the sentences above: the branches grouped by their anchor pair, the best of every group stays
  per thread  what the kernel does: branch u looks at the links h of end a ^ 1 (at most 5, its own mirror among them); w = h >> 1
              is parallel when it is a branch whose end h ^ 1 links to a (the mirror) and whose end h links to b

marks_of() asserts on every call that the two agree, that every popped unitig is a branch with a parallel branch that stays,
that exactly one member of every class stays, that an anchor end of a class of two or more has at least two links (so an
anchor is no branch and is never popped), that no popped unitig is a tip candidate, and the invariant of the UNION of the
tip marks and the bubble marks: an end of an unmarked unitig that had links keeps at least one of them among the unmarked
unitigs.
marks_of_arrays() is the rule again with numpy on a call's own (offsets, count_sums, flags, link_offsets, link_to), for
tables too large for strings.  two_haplotypes() makes the reads the tests count: a genome and a second haplotype beside it.
"""
import numpy as np

import graph_ref as gr
import tip_ref as tr
import unitig_link_ref as lr
import unitig_ref as ur

KEEP, TIP, ISOLATED, POP = 0, 1, 2, 4
STATS = ("rounds", "tips", "tip_nodes", "isolated", "isolated_nodes", "popped", "popped_nodes", "bubbles", "occurrences", "converged")


def branches_of(n, circ, ls, max_bubble_nodes):
    """-> {branch u: (a, b)}"""
    out = {}
    for u in range(len(n)):
        if circ[u] or n[u] > max_bubble_nodes or len(ls[2 * u]) != 1 or len(ls[2 * u + 1]) != 1:
            continue
        a, b = ls[2 * u][0], ls[2 * u + 1][0]
        if a >> 1 != u and b >> 1 != u:
            out[u] = (a, b)
    return out


def outranks(n, c, w, u):
    x, y = c[w] * n[u], c[u] * n[w]
    return x > y or (x == y and w < u)


def by_definition(n, c, br):
    """-> (the classes of two or more: lists of branches, the popped branches)"""
    groups = {}
    for u, (a, b) in br.items():
        groups.setdefault((min(a, b), max(a, b)), []).append(u)
    classes = [g for g in groups.values() if len(g) >= 2]
    popped = {u for g in classes for u in g if any(w != u and outranks(n, c, w, u) for w in g)}
    return classes, popped


def per_thread(n, c, ls, br):
    """-> (the branches that stay and have a parallel branch, the popped branches)"""
    stay, popped = set(), set()
    for u, (a, b) in br.items():
        found = beaten = False
        for h in ls[a ^ 1]:
            w = h >> 1
            if w == u or w not in br:
                continue
            near, far = (br[w][1], br[w][0]) if h & 1 == 0 else (br[w][0], br[w][1])  # the links of ends h ^ 1 and h
            if near != a or far != b:
                continue
            found = True
            beaten = beaten or outranks(n, c, w, u)
        if beaten:
            popped.add(u)
        elif found:
            stay.add(u)
    return stay, popped


def marks_of(n, c, circ, ls, max_bubble_nodes, max_tip_nodes=0):
    """n, c: nodes and count sum per unitig, circ: is a cycle, ls: the links of every end
    -> ([mark per unitig: TIP, ISOLATED (max_tip_nodes > 0) or POP], bubbles: the classes of two or more)"""
    nu = len(n)
    br = branches_of(n, circ, ls, max_bubble_nodes) if max_bubble_nodes else {}
    classes, popped = by_definition(n, c, br)
    stay, popped2 = per_thread(n, c, ls, br)
    assert popped == popped2, ("the definition and the per-thread search disagree", sorted(popped), sorted(popped2))
    assert len(stay) == len(classes), (sorted(stay), classes)
    for g in classes:
        left = [u for u in g if u not in popped]
        assert len(left) == 1 and left[0] in stay, ("not exactly one member of a class stays", g, left)
        assert all(u in br for u in g)
        a, b = br[g[0]]
        for anchor_end in (a ^ 1, b ^ 1):  # an anchor: at least two links at that end, so no branch, so never popped
            assert len(ls[anchor_end]) >= 2 and anchor_end >> 1 not in br and anchor_end >> 1 not in popped
        s = left[0]  # the one that stays keeps both anchors joined
        assert {br[s][0], br[s][1]} == {a, b}
    assert all(u in br and ls[2 * u] and ls[2 * u + 1] for u in popped)  # (no dead end: no tip candidate)
    tips = tr.marks_of(n, c, circ, ls, max_tip_nodes) if max_tip_nodes else [KEEP] * nu
    out = [tips[u] | (POP if u in popped else 0) for u in range(nu)]
    assert all(x in (KEEP, TIP, ISOLATED, POP) for x in out), "a unitig with both marks"
    for g in classes:  # an anchor that is a tip candidate is never a tip
        for f in br[g[0]]:
            assert tips[f >> 1] != TIP, ("an anchor was clipped", g, f)
    for u in range(nu):
        if out[u] == KEEP:
            for e in (2 * u, 2 * u + 1):
                assert not ls[e] or any(out[f >> 1] == KEEP for f in ls[e]), ("an end lost all its links", e, ls[e], out)
    return out, len(classes)


def marks(table, k, max_bubble_nodes, max_tip_nodes=0, lo=1, hi=gr.U32):
    """table: {canonical string: count} -> (unitigs, links, [mark per unitig], the bubble tally of 4, the tip tally of 4)"""
    us, ls = lr.links(table, k, lo, hi)
    n, c = [u[3] for u in us], [u[1] for u in us]
    m, bubbles = marks_of(n, c, [bool(u[2] & ur.CIRCULAR) for u in us], ls, max_bubble_nodes, max_tip_nodes)
    return us, ls, m, tally_of(m, n, c, bubbles), tr.tally_of(m, n)


def tally_of(m, n, c, bubbles):
    """KT_BUBBLE_TALLY: popped unitigs, their nodes, bubbles, occurrences popped"""
    pop = [u for u, x in enumerate(m) if x == POP]
    return [len(pop), sum(n[u] for u in pop), bubbles, sum(c[u] for u in pop)]


def simplify(table, k, max_tip_nodes, max_bubble_nodes, max_rounds=8, drop_isolated=False, lo=1, hi=gr.U32):
    """-> (the reduced table: a new dict, the stats as kt_ctr_simplify fills them (12), the marks of every round made)"""
    table = dict(table)
    s = [0] * 12
    rounds = []
    for _ in range(max_rounds):
        us, ls, m, bt, tt = marks(table, k, max_bubble_nodes, max_tip_nodes, lo, hi)
        rounds.append(m)
        gone = [u for u, x in enumerate(m) if x in (TIP, POP) or (drop_isolated and x == ISOLATED)]
        if not gone:
            s[9] = 0
            break
        for key in tr.nodes_of(us, k, gone):
            del table[key]
        s[0] += 1
        s[1], s[2] = s[1] + tt[0], s[2] + tt[1]
        if drop_isolated:
            s[3], s[4] = s[3] + tt[2], s[4] + tt[3]
        s[5], s[6], s[7] = s[5] + bt[0], s[6] + bt[1], s[7] + bt[2]
        s[8] += sum(us[u][1] for u in gone)
        s[9] = 1
    return table, s, rounds


def want_simplify_stats(s):
    """unitigs.simplify.stats of the stats of a call"""
    vals = list(s[:9]) + [1 - s[9]]
    return "".join("%s\t%d\n" % nv for nv in zip(STATS, vals)).encode()


def marks_of_arrays(offsets, count_sums, flags, link_offsets, link_to, k, max_bubble_nodes, max_tip_nodes=0):
    """the rule on the arrays of a kt_ctr_unitigs_linked call -> (marks u8, the bubble tally u64[4]); with max_tip_nodes the
    marks carry tip_ref.marks_of_arrays' as well"""
    off = np.asarray(offsets, np.int64)
    nu = len(off) - 1
    n = off[1:] - off[:-1] - (k - 1)
    c = np.asarray(count_sums, np.uint64)
    lo = np.asarray(link_offsets, np.int64)
    to = np.asarray(link_to, np.int64)
    out = np.zeros(nu, np.uint8)
    bubbles = 0
    if nu and max_bubble_nodes:
        deg = lo[1:] - lo[:-1]
        ok = ((np.asarray(flags) & ur.CIRCULAR) == 0) & (n <= max_bubble_nodes) & (deg[0::2] == 1) & (deg[1::2] == 1)
        us = np.flatnonzero(ok)
        a, b = to[lo[2 * us]], to[lo[2 * us + 1]]
        own = (a >> 1 != us) & (b >> 1 != us)
        us, a, b = us[own], a[own], b[own]
        pair = (np.minimum(a, b).astype(np.uint64) << np.uint64(32)) | np.maximum(a, b).astype(np.uint64)
        order = np.argsort(pair, kind="stable")
        sp, su = pair[order], us[order]
        starts = np.flatnonzero(np.concatenate([[True], sp[1:] != sp[:-1]])) if len(sp) else np.zeros(0, np.int64)
        ends = np.concatenate([starts[1:], [len(sp)]]) if len(sp) else starts
        for s, e in zip(starts, ends):
            if e - s < 2:
                continue
            bubbles += 1
            g = [int(u) for u in su[s:e]]
            gn, gc = {u: int(n[u]) for u in g}, {u: int(c[u]) for u in g}  # (Python integers: the products are exact)
            for u in g:
                if any(w != u and outranks(gn, gc, w, u) for w in g):
                    out[u] = POP
    pop = out == POP
    tally = np.array([pop.sum(), n[pop].sum(), bubbles, c[pop].sum()], np.uint64)
    if max_tip_nodes:
        out |= tr.marks_of_arrays(offsets, count_sums, flags, link_offsets, link_to, k, max_tip_nodes)[0]
    return out, tally


def two_haplotypes(seed, k, genome_len=400):
    """The reads of a diploid sample: a random genome three times; a second haplotype - a substitution every 45 bases and one
    deletion of a base, its branch a node shorter - one to three times; three reads of 40 bases with an error each near their end, for tips."""
    rng = np.random.default_rng(seed)
    L = list("ACGT")
    g = "".join(rng.choice(L, size=genome_len))
    h = list(g)
    for p in range(22, genome_len, 45):
        h[p] = L[(L.index(h[p]) + int(rng.integers(1, 4))) % 4]
    del h[22 + 45 * int(rng.integers(2, genome_len // 45 - 1)) + 3]  # (three bases behind a substitution: one bubble with it, at every k)
    reads = [g] * 3 + ["".join(h)] * int(rng.integers(1, 4))
    for _ in range(3):
        a = int(rng.integers(0, genome_len - 40))
        r = list(g[a:a + 40])
        p = 39 - int(rng.integers(0, min(k - 1, 8)))
        r[p] = L[(L.index(r[p]) + int(rng.integers(1, 4))) % 4]
        reads.append("".join(r))
    return reads
