"""What kt_unitig_components and kt_thread_read_components compute, restated over the calls' own arrays.

The definition (the header's): end e = 2u + sign owns link_to[link_offsets[e]:link_offsets[e + 1]]; a value f joins unitig
e >> 1 to unitig f >> 1, whatever the direction and whether or not the mirror is there; a link to oneself joins nothing; a
value f >= 2 * n_unitigs is a bad link, counted and otherwise ignored.  Components are numbered by their smallest unitig.

The labelling is made twice - a union-find over the links, and a breadth-first search from every unvisited unitig in ascending
order, which gives the numbering directly - and components() asserts on every call that the two agree.
sync_rounds() plays the library's round scheme synchronously (every hook of a round reads the labels as the round began) and
returns the rounds it takes, the last one - which changes nothing - included: the yardstick for the library's tally[5].
"""
import numpy as np

NO_COMPONENT = 0xFFFFFFFF
FIELDS = ("unitigs", "nodes", "count_sum", "links", "first_unitig")
M64 = (1 << 64) - 1


def pairs_of(link_offsets, link_to):
    """-> (n_unitigs, [(u, v)] for every owned link that is neither bad nor a link to oneself, good links per unitig, bad links)"""
    off = np.asarray(link_offsets, np.uint64).astype(np.int64)
    to = np.asarray(link_to, np.uint32).astype(np.int64)
    nu = (len(off) - 1) // 2
    if nu == 0:
        return 0, np.zeros((0, 2), np.int64), np.zeros(0, np.int64), 0
    lo, hi = int(off[0]), int(off[2 * nu])
    owner = np.repeat(np.arange(2 * nu), np.diff(off)) >> 1  # the unitig of the end that owns link lo + j
    f = to[lo:hi]
    assert len(owner) == len(f)
    bad = f >= 2 * nu
    good = np.bincount(owner[~bad], minlength=nu)
    keep = ~bad & ((f >> 1) != owner)
    return nu, np.stack([owner[keep], f[keep] >> 1], axis=1), good, int(bad.sum())


def by_union_find(nu, pairs):
    parent = list(range(nu))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x
    for u, v in pairs.tolist():
        a, b = find(u), find(v)
        if a != b:
            parent[max(a, b)] = min(a, b)  # (the smaller root stays: a root is its set's smallest member)
    roots = [find(u) for u in range(nu)]
    number, out = {}, []
    for u, r in enumerate(roots):
        assert r <= u
        if r == u:
            number[u] = len(number)
        out.append(number[r])
    return out


def by_search(nu, pairs):
    heads = [[] for _ in range(nu)]
    for u, v in pairs.tolist():
        heads[u].append(v)
        heads[v].append(u)
    comp, n = [-1] * nu, 0
    for s in range(nu):
        if comp[s] >= 0:
            continue
        comp[s] = n
        queue = [s]
        while queue:
            nxt = []
            for u in queue:
                for v in heads[u]:
                    if comp[v] < 0:
                        comp[v] = n
                        nxt.append(v)
            queue = nxt
        n += 1
    return comp


def components(link_offsets, link_to, unitig_offsets=None, count_sums=None, k=None):
    """-> {"component": u32 per unitig, "stats": u64 (components x 5: FIELDS), "tally": u64[6] - [5], the rounds, is 0}"""
    nu, pairs, good, bad = pairs_of(link_offsets, link_to)
    comp = by_union_find(nu, pairs)
    assert comp == by_search(nu, pairs), "the union-find and the search disagree"
    nc = max(comp) + 1 if nu else 0
    rows = [[0, 0, 0, 0, None] for _ in range(nc)]
    uoff = None if unitig_offsets is None else [int(x) for x in np.asarray(unitig_offsets, np.uint64)]
    sums = None if count_sums is None else [int(x) for x in np.asarray(count_sums, np.uint64)]
    for u, c in enumerate(comp):
        r = rows[c]
        r[0] += 1
        if uoff is not None:
            r[1] += max(0, uoff[u + 1] - uoff[u] - (k - 1))
        if sums is not None:
            r[2] += sums[u]
        r[3] += int(good[u])
        if r[4] is None:
            r[4] = u
    stats = np.array([[x & M64 for x in r] for r in rows], np.uint64).reshape(nc, 5)
    tally = np.array([nc, sum(1 for r in rows if r[0] == 1), max((r[0] for r in rows), default=0),
                      max((r[1] for r in rows), default=0), bad, 0], np.uint64)
    return {"component": np.array(comp, np.uint32).reshape(nu), "stats": stats, "tally": tally}


def sync_rounds(link_offsets, link_to):
    """the round scheme, synchronous: hook - every link (u, v) reads lu = L[u], lv = L[v] as the round began and lowers L[the
    other unitig] and L[the larger label] to the smaller label -, shortcut - L[u] = L[L[u]] over the hooks' result -, until a
    round's hooks lower nothing.  -> (the labels, the rounds, the last included; 0 when no link is owned)"""
    nu, pairs, _, _ = pairs_of(link_offsets, link_to)
    L = np.arange(nu, dtype=np.int64)
    off = np.asarray(link_offsets, np.uint64)
    if nu == 0 or int(off[2 * nu]) == int(off[0]):
        return L, 0
    u, v = pairs[:, 0], pairs[:, 1]
    rounds = 0
    while True:
        rounds += 1
        assert rounds <= nu + 1
        lu, lv = L[u], L[v]
        lo, hi = np.minimum(lu, lv), np.maximum(lu, lv)
        far = np.where(lu < lv, v, u)
        new = L.copy()
        np.minimum.at(new, far, lo)
        np.minimum.at(new, hi, lo)
        changed = bool((new != L).any())
        L = new[new]
        if not changed:
            return L, rounds


def check_labels(link_offsets, link_to, comp):
    """what must hold of a component array: every link's two unitigs share a component; first occurrences ascend"""
    nu, pairs, _, _ = pairs_of(link_offsets, link_to)
    comp = np.asarray(comp).astype(np.int64)
    assert len(comp) == nu
    assert (comp[pairs[:, 0]] == comp[pairs[:, 1]]).all()
    seen = -1
    for u, c in enumerate(comp.tolist()):
        assert c <= seen + 1 and c <= u, (u, c)
        seen = max(seen, c)


def read_components(run_unitig, run_len, run_offsets, component, n_components, comp_reads=None, comp_hits=None):
    """-> {"read_component" u32, "read_mixed" u8, "tally" u64[4]}; comp_reads / comp_hits (lists or arrays of n_components, or
    None) are added to in place"""
    ru = np.asarray(run_unitig, np.uint32).astype(np.int64) >> 1
    rl = np.asarray(run_len, np.uint32).astype(np.int64)
    ro = [int(x) for x in np.asarray(run_offsets, np.uint64)]
    comp = np.asarray(component, np.uint32).astype(np.int64)
    n = len(ro) - 1
    rc = np.full(len(ru), -1, np.int64)  # a run's component, -1 for a bad run
    ok = ru < len(comp)
    rc[ok] = comp[ru[ok]]
    rc[rc >= n_components] = -1
    out_c, out_m = np.full(n, NO_COMPONENT, np.uint32), np.zeros(n, np.uint8)
    for i in range(n):
        mine = rc[ro[i]:ro[i + 1]]
        mine = mine[mine >= 0]
        if len(mine):
            out_c[i] = mine[0]
            out_m[i] = bool((mine != mine[0]).any())
            if comp_reads is not None:
                comp_reads[int(mine[0])] += 1
    nr = ro[n] if n else 0
    if comp_hits is not None:
        for c, ln in zip(rc[:nr].tolist(), rl[:nr].tolist()):
            if c >= 0:
                comp_hits[c] += ln
    with_c = int((out_c != NO_COMPONENT).sum())
    return {"read_component": out_c, "read_mixed": out_m,
            "tally": np.array([with_c, n - with_c, int(out_m.sum()), int((rc[:nr] < 0).sum())], np.uint64)}


# ---- the files of `kmertools unitigs --components` and `kmertools thread --components` -------------------------------------------

def want_components(stats, k):
    """unitigs.components: component, unitigs, nodes, bases, count_sum, km, links, first_unitig"""
    return "".join("%d\t%d\t%d\t%d\t%d\t%.1f\t%d\t%d\n" % (c, r[0], r[1], r[1] + (k - 1) * r[0], r[2], r[2] / r[1], r[3], r[4])
                   for c, r in enumerate([[int(x) for x in row] for row in stats])).encode()


def want_components_stats(stats, tally):
    nodes = sum(int(r[1]) for r in stats)
    t = [int(x) for x in tally]
    return ("components\t%d\nsingletons\t%d\nlargest_unitigs\t%d\nlargest_nodes\t%d\nlargest_share\t%.4f\n"
            % (t[0], t[1], t[2], t[3], t[3] / nodes if nodes else 0.0)).encode()


def tagged_fa(fa, comp):
    """unitigs.fa with " CC:i:{c}" behind every header line"""
    lines = fa.split(b"\n")
    heads = [i for i, ln in enumerate(lines) if ln.startswith(b">")]
    assert len(heads) == len(comp)
    for i, c in zip(heads, comp):
        lines[i] += b" CC:i:%d" % int(c)
    return b"\n".join(lines)


def tagged_gfa(gfa, comp):
    """unitigs.gfa with "\\tCC:i:{c}" behind every S line"""
    lines = gfa.split(b"\n")
    segs = [i for i, ln in enumerate(lines) if ln.startswith(b"S\t")]
    assert len(segs) == len(comp)
    for i, c in zip(segs, comp):
        lines[i] += b"\tCC:i:%d" % int(c)
    return b"\n".join(lines)


def want_thread_reads(names, read_component, read_mixed, run_len, run_offsets):
    """thread.reads: name, component or *, mixed, hits"""
    rl = np.asarray(run_len).astype(np.int64)
    ro = [int(x) for x in run_offsets]
    return "".join("%s\t%s\t%d\t%d\n" % (name, "*" if c == NO_COMPONENT else "%d" % c, m, int(rl[ro[i]:ro[i + 1]].sum()))
                   for i, (name, c, m) in enumerate(zip(names, [int(x) for x in read_component], [int(x) for x in read_mixed]))).encode()


def want_thread_components(stats, comp_reads, comp_hits):
    """thread.components: component, unitigs, nodes, reads, hits"""
    return "".join("%d\t%d\t%d\t%d\t%d\n" % (c, int(r[0]), int(r[1]), int(comp_reads[c]), int(comp_hits[c])) for c, r in enumerate(stats)).encode()


def want_thread_stats_lines(tally, comp_hits):
    return ("reads_with_component\t%d\nreads_mixed\t%d\ncomponents_hit\t%d\n" % (int(tally[0]), int(tally[2]), sum(1 for h in comp_hits if h))).encode()
