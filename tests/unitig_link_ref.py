"""What kt_ctr_unitigs_linked adds to kt_ctr_unitigs, restated twice on top of unitig_ref.unitigs (the unitigs themselves).

The rule (the header's): oriented unitig (u, +) is unitig u's string U, (u, -) its reverse complement.  There is a directed
link (u, su) -> (v, sv) exactly when the last k - 1 bases of oriented (u, su) equal the first k - 1 bases of oriented (v, sv)
(k = 1: every pair).  No pair is excluded.  End e = 2u + (su is '-') owns its links 2v + (sv is '-'), ascending.

  string rule  the sentence above, over all oriented pairs (grouped by their first k - 1 bases)
  node rule    the last k-mer T of the oriented unitig is a node read as F (its right nibble faces outward) or as rc(F) (its
               left nibble does); every set bit names a neighbour string W that goes on from T.  canon(W) is a node of some
               unitig v: W has to be the first k-mer of (v, +) or of (v, -) - the neighbour stands at an end of its unitig,
               the facing side outward - and v is no cycle unless the link is the cycle's own.

links() asserts on every call that the two agree, that every link has its mirror (v, !sv) -> (u, !su), that a cycle has
exactly its two closing links and that no end has more than 5 links (4 for odd k).
links_of_arrays() is the string rule again on the call's own arrays with numpy, for tables too large for strings.
"""
import numpy as np

import graph_ref as gr
import unitig_ref as ur


def oriented(us):
    """[(string, ...)] -> the 2 * len(us) oriented strings, index 2u + (sign is '-')"""
    out = []
    for u in us:
        out += [u[0], gr.rc_s(u[0])]
    return out


def string_rule(us, k):
    o = oriented(us)
    heads = {}
    for f, s in enumerate(o):
        heads.setdefault(s[:k - 1], []).append(f)
    return [sorted(heads.get(s[len(s) - (k - 1):], [])) for s in o]


def node_rule(table, us, k, lo, hi):
    info_of = {gr.str_of(key, k): info for key, _, info in gr.brute(table, k, lo, hi)}
    o = oriented(us)
    where = {}  # canonical k-mer -> its unitig
    for u, rec in enumerate(us):
        for j in range(len(rec[0]) - k + 1):
            where[gr.canon_s(rec[0][j:j + k])] = u
    out = []
    for e, s in enumerate(o):
        T = s[len(s) - k:]
        F = gr.canon_s(T)
        info = info_of[F]
        if T == F:
            ws = [F[1:] + gr.ACGT[x] for x in range(4) if info >> x & 1]
        else:
            ws = [gr.rc_s(gr.ACGT[x] + F[:-1]) for x in range(4) if info >> (4 + x) & 1]
        mine = []
        for W in ws:
            assert W[:k - 1] == T[1:]
            v = where[gr.canon_s(W)]
            ends = [f for f in (2 * v, 2 * v + 1) if o[f][:k] == W]
            assert ends, ("a neighbour is not at an end of its unitig, the facing side outward", T, W, us[v][0])
            assert not (us[v][2] & ur.CIRCULAR) or v == e >> 1, ("a link leads into a cycle", T, W)
            mine += ends
        assert len(set(mine)) == len(mine)
        out.append(sorted(mine))
    return out


def links(table, k, lo=1, hi=gr.U32):
    """table: {canonical string: count} -> (unitig_ref.unitigs' list, [the links of end e, ascending] for e in 0 .. 2 * unitigs)"""
    us = ur.unitigs(table, k, lo, hi)
    ls = string_rule(us, k)
    assert ls == node_rule(table, us, k, lo, hi), "the string rule and the node rule disagree"
    have = {(e, f) for e, fs in enumerate(ls) for f in fs}
    for e, f in have:
        assert (f ^ 1, e ^ 1) in have, ("a link without its mirror", e, f)
    for u, rec in enumerate(us):
        if rec[2] & ur.CIRCULAR:
            assert ls[2 * u] == [2 * u] and ls[2 * u + 1] == [2 * u + 1], ("a cycle's links", u)
    assert all(len(fs) <= (5 if k % 2 == 0 else 4) for fs in ls)
    return us, ls


def as_arrays(ls):
    """[the links of end e] -> (link_offsets u64, link_to u32) as the call fills them"""
    off = np.zeros(len(ls) + 1, np.uint64)
    off[1:] = np.cumsum([len(fs) for fs in ls], dtype=np.uint64)
    return off, np.array([f for fs in ls for f in fs], np.uint32).reshape(-1)


_CODE = np.zeros(256, np.uint64)
for _i, _ch in enumerate(b"ACGT"):
    _CODE[_ch] = _i


def links_of_arrays(bases, offsets, k):
    """the string rule on (bases, offsets) as kt_ctr_unitigs fills them, 2 <= k <= 32 -> (link_offsets, link_to)"""
    assert 2 <= k <= 32
    off = np.asarray(offsets, np.int64)
    nu = len(off) - 1
    code = _CODE[np.asarray(bases, np.uint8)]
    first = np.zeros(nu, np.uint64)  # U[:k - 1] and U[-(k - 1):] as 2-bit words
    last = np.zeros(nu, np.uint64)
    for j in range(k - 1):
        first = (first << np.uint64(2)) | code[off[:-1] + j]
        last = (last << np.uint64(2)) | code[off[1:] - (k - 1) + j]
    # oriented 2u: starts with first, ends with last; 2u + 1: starts with rc(last), ends with rc(first)
    head = np.empty(2 * nu, np.uint64)
    tail = np.empty(2 * nu, np.uint64)
    head[0::2], head[1::2] = first, gr.rc_np(last, k - 1)
    tail[0::2], tail[1::2] = last, gr.rc_np(first, k - 1)
    order = np.argsort(head, kind="stable")  # (equal heads keep the order of their numbers: ascending within an end)
    sh = head[order]
    a, b = np.searchsorted(sh, tail, "left"), np.searchsorted(sh, tail, "right")
    link_offsets = np.zeros(2 * nu + 1, np.uint64)
    link_offsets[1:] = np.cumsum(b - a, dtype=np.uint64)
    total = int(link_offsets[-1])
    # link j of end e is order[a[e] + (j - link_offsets[e])]
    e_of = np.repeat(np.arange(2 * nu), b - a)
    within = np.arange(total) - link_offsets[:-1].astype(np.int64)[e_of]
    return link_offsets, order[a[e_of] + within].astype(np.uint32)


def sign(x):
    return "-" if x & 1 else "+"


def written(e, f):
    """of a link and its mirror the GFA holds the one whose (u, su is '-', v, sv is '-') is not the larger"""
    return (e, f) <= (f ^ 1, e ^ 1)


def want_gfa(table, k, lo=1, hi=gr.U32):
    us, ls = links(table, k, lo, hi)
    out = ["H\tVN:Z:1.0\n"]
    for i, (s, c, f, n) in enumerate(us):
        out.append("S\t%d\t%s\tLN:i:%d\tKC:i:%d\tkm:f:%.1f%s\n" % (i, s, len(s), c, c / n, "\tCL:i:1" if f & ur.CIRCULAR else ""))
    for e, fs in enumerate(ls):
        out += ["L\t%d\t%s\t%d\t%s\t%dM\n" % (e >> 1, sign(e), f >> 1, sign(f), k - 1) for f in fs if written(e, f)]
    return "".join(out).encode()


def want_fa_links(table, k, lo=1, hi=gr.U32):
    us, ls = links(table, k, lo, hi)
    fa = []
    for i, (s, c, f, n) in enumerate(us):
        fields = "".join(" L:%s:%d:%s" % (sign(e), t >> 1, sign(t)) for e in (2 * i, 2 * i + 1) for t in ls[e])
        fa.append(">%d LN:i:%d KC:i:%d km:f:%.1f%s%s\n%s\n" % (i, len(s), c, c / n, " CL:i:1" if f & ur.CIRCULAR else "", fields, s))
    return "".join(fa).encode()


def link_stats(ls):
    pairs = [(e, f) for e, fs in enumerate(ls) for f in fs]
    return [("links", len(pairs)), ("edges", sum(1 for e, f in pairs if written(e, f))),
            ("dead_ends", sum(1 for fs in ls if not fs)),
            ("isolated", sum(1 for u in range(len(ls) // 2) if not ls[2 * u] and not ls[2 * u + 1])),
            ("self_links", sum(1 for e, f in pairs if e >> 1 == f >> 1)), ("max_end_degree", max(map(len, ls), default=0))]


def want_link_stats(table, k, lo=1, hi=gr.U32):
    return "".join("%s\t%d\n" % nv for nv in link_stats(links(table, k, lo, hi)[1])).encode()
