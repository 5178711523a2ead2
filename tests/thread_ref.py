"""What `kmertools thread` computes, restated on strings and numpy on top of unitig_ref / unitig_link_ref (the unitigs and
the GFA): the index values of kt_ctr_index_sequences, the oriented hits of kt_ctr_thread_hits, the runs of kt_thread_runs,
the chains of runs and the three text files.

  index   every window of the unitigs that starts at global base G (the unitigs concatenated) with string w puts
          canon(w) -> 1 + 2 * G + S into the index, S = 1 when w is not canon(w).  A k-mer may occur once only (asserted).
  hits    a read's window with string w: KT_NO_KMER where no window starts, 0 when canon(w) is not in the index, otherwise
          1 + ((v - 1) ^ t) with t = 1 when w is not canon(w).  (h - 1) >> 1 = G, (h - 1) & 1 = a: antiparallel.
  runs    the header's rule, position by position (runs()), and once more from strings alone with str.find (brute_runs()).
  chains  maximal sequences of runs of one read, each starting at the read position where the one before stopped, at the
          first k-mer of its oriented unitig, the one before having ended at the last k-mer of its own.
"""
import numpy as np

import graph_ref as gr
import unitig_link_ref as lr
import unitig_ref as ur

NO_KMER = 0xFFFFFFFF
TALLY_NAMES = ("windows", "hits", "misses", "bad", "runs", "reads_with_hit")


def norm(read):
    """a record as the walks read it: both cases, U for T"""
    return read.upper().replace("U", "T")


def window_starts(read, k):
    """the starts of the read's valid windows (k bases, ACGT only; the caller norm()s)"""
    return [j for j in range(len(read) - k + 1) if all(c in gr.ACGT for c in read[j:j + k])]


def csr(strings):
    """strings -> (bases u8, offsets u64)"""
    off = np.zeros(len(strings) + 1, np.uint64)
    off[1:] = np.cumsum([len(s) for s in strings], dtype=np.uint64)
    return np.frombuffer("".join(strings).encode(), np.uint8).copy(), off


def index_values(unitigs, k):
    """unitig strings -> {canonical k-mer string: 1 + 2 G + S}"""
    out, base = {}, 0
    for s in unitigs:
        for j in window_starts(s, k):
            w = s[j:j + k]
            c = gr.canon_s(w)
            assert c not in out, ("a k-mer occurs twice in the indexed sequences", c)
            out[c] = 1 + 2 * (base + j) + (1 if w != c else 0)
        base += len(s)
    return out


def hits_of(index, reads, k):
    """-> u32 array over the concatenated reads"""
    out = np.full(sum(len(r) for r in reads), NO_KMER, np.uint32)
    base = 0
    for r in map(norm, reads):
        for j in window_starts(r, k):
            w = r[j:j + k]
            c = gr.canon_s(w)
            v = index.get(c, 0)
            out[base + j] = 1 + ((v - 1) ^ (1 if w != c else 0)) if v else 0
        base += len(r)
    return out


def _decode(h, uoff, k):
    """a hits entry -> None (no window), "miss", "bad" or (u, p, a)"""
    if h == NO_KMER:
        return None
    if h == 0:
        return "miss"
    G, a = (h - 1) >> 1, (h - 1) & 1
    if G >= uoff[-1]:
        return "bad"
    u = int(np.searchsorted(uoff, G, "right")) - 1
    p = G - int(uoff[u])
    if p > int(uoff[u + 1]) - int(uoff[u]) - k:
        return "bad"
    return (u, p, a)


def runs(hits, read_offsets, unitig_offsets, k):
    """the rule of kt_thread_runs -> {"runs": [(start, len, 2u + a, upos)], "run_offsets": [...], "unitig_hits": [...],
    "unitig_runs": [...], "tally": [6]}"""
    roff = [int(x) for x in read_offsets]
    uoff = np.asarray(unitig_offsets, np.int64)
    nu = len(uoff) - 1
    out, run_offsets = [], []
    uh, urn = [0] * nu, [0] * nu
    tally = [0] * 6
    for i in range(len(roff) - 1):
        run_offsets.append(len(out))
        prev, first = None, len(out)
        for j in range(roff[i], roff[i + 1]):
            d = _decode(int(hits[j]), uoff, k)
            if d is None:
                prev = None
                continue
            tally[0] += 1
            if not isinstance(d, tuple):
                tally[2 if d == "miss" else 3] += 1
                prev = None
                continue
            tally[1] += 1
            u, p, a = d
            if prev is not None and prev[0] == u and prev[2] == a and p == prev[1] + (1 if a == 0 else -1):
                s, n, e, q = out[-1]
                out[-1] = (s, n + 1, e, q)
            else:
                out.append((j, 1, 2 * u + a, p))
                urn[u] += 1
            uh[u] += 1
            prev = d
        tally[5] += len(out) > first
    run_offsets.append(len(out))
    tally[4] = len(out)
    return {"runs": out, "run_offsets": run_offsets, "unitig_hits": uh, "unitig_runs": urn, "tally": tally}


def brute_runs(unitigs, reads, k):
    """the same runs from strings alone: every read k-mer and its reverse complement looked up with str.find"""
    uoff = np.cumsum([0] + [len(s) for s in unitigs])
    out, run_offsets, base = [], [], 0
    for r in map(norm, reads):
        run_offsets.append(len(out))
        prev = None
        for j in range(len(r)):
            w = r[j:j + k]
            d = None
            if len(w) == k and all(c in gr.ACGT for c in w):
                for u, s in enumerate(unitigs):
                    p = s.find(w)
                    if p >= 0:
                        d = (u, p, 0)
                        break
                    p = s.find(gr.rc_s(w))
                    if p >= 0:
                        d = (u, p, 1)
                        break
            if d is not None and prev is not None and prev[0] == d[0] and prev[2] == d[2] and d[1] == prev[1] + (1 if d[2] == 0 else -1):
                s0, n, e, q = out[-1]
                out[-1] = (s0, n + 1, e, q)
            elif d is not None:
                out.append((base + j, 1, 2 * d[0] + d[2], d[1]))
            prev = d
        base += len(r)
    run_offsets.append(len(out))
    return out, run_offsets, uoff


def chains(read_runs, ulen, k):
    """the runs of one read, in order -> [[run, ...]]"""
    out = []
    for r in read_runs:
        s, n, e, p = r
        if out:
            s0, n0, e0, p0 = out[-1][-1]
            L, L0 = ulen[e >> 1], ulen[e0 >> 1]
            starts = p == (0 if e & 1 == 0 else L - k)
            ended = (p0 + n0 - 1 == L0 - k) if e0 & 1 == 0 else (p0 - (n0 - 1) == 0)
            if s == s0 + n0 and starts and ended:
                out[-1].append(r)
                continue
        out.append([r])
    return out


def gaf_line(read_id, read_len, read_start, chain, ulen, k):
    s, n, e, p = chain[0]
    qs = s - read_start
    qe = chain[-1][0] - read_start + chain[-1][1] - 1 + k
    path = "".join((">" if r[2] & 1 == 0 else "<") + str(r[2] >> 1) for r in chain)
    plen = sum(ulen[r[2] >> 1] for r in chain) - (k - 1) * (len(chain) - 1)
    ps = p if e & 1 == 0 else ulen[e >> 1] - k - p
    return "%s\t%d\t%d\t%d\t+\t%s\t%d\t%d\t%d\t%d\t%d\t255\n" % (read_id, read_len, qs, qe, path, plen, ps, ps + qe - qs, qe - qs, qe - qs)


def path_string(unitigs, chain, k):
    """the chain's oriented unitigs concatenated with k - 1 overlap"""
    out = ""
    for r in chain:
        s = unitigs[r[2] >> 1] if r[2] & 1 == 0 else gr.rc_s(unitigs[r[2] >> 1])
        if out:
            assert k == 1 or out[-(k - 1):] == s[:k - 1], "consecutive unitigs of a chain do not overlap by k - 1"
        out += s[k - 1:] if out else s
    return out


def thread(unitigs, reads, k):
    """unitig strings, read strings -> (runs()' dict with "chains": per read [[run, ...]], hits array)"""
    _, uoff = csr(unitigs)
    _, roff = csr(reads)
    hits = hits_of(index_values(unitigs, k), reads, k)
    res = runs(hits, roff, uoff, k)
    ulen = [len(s) for s in unitigs]
    ro = res["run_offsets"]
    res["chains"] = [chains(res["runs"][ro[i]:ro[i + 1]], ulen, k) for i in range(len(reads))]
    return res, hits


# ---- the same on arrays with numpy, for batches too large for strings (checked against the above on the CPU) -------------------

_CODE = np.full(256, 4, np.uint64)  # every byte the walks take for a nucleotide: the letters, both cases, U, the raw codes
for _letters, _v in ((b"Aa\x00", 0), (b"Cc\x01", 1), (b"Gg\x02", 2), (b"TtUu\x03", 3)):
    for _x in _letters:
        _CODE[_x] = _v


def windows_np(bases, offsets, k):
    """-> (valid bool per base: a window starts here, fwd u64, rc u64 - the latter two only meaningful where valid)"""
    bases = np.asarray(bases, np.uint8)
    off = np.asarray(offsets, np.int64)
    total = len(bases)
    code = _CODE[bases]
    f = np.zeros(total, np.uint64)
    r = np.zeros(total, np.uint64)
    bad = np.zeros(total + 1, np.int64)
    bad[1:] = np.cumsum(code > 3)
    pos = np.arange(total, dtype=np.int64)
    end = off[np.searchsorted(off, pos, "right")] if total else pos  # the end of the read that holds the base
    valid = pos + k <= end
    valid &= bad[np.minimum(pos + k, total)] - bad[pos] == 0
    c3 = code & np.uint64(3)
    for i in range(k):
        sh = np.zeros(total, np.uint64)
        sh[:total - i] = c3[i:]
        f |= sh << np.uint64(2 * (k - 1 - i))
        r |= (np.uint64(3) - sh) << np.uint64(2 * i)
    return valid, f, r


def index_np(unitig_bases, unitig_offsets, k):
    """-> (keys u64 ascending, values u32, number of windows); asserts that no k-mer occurs twice"""
    valid, f, r = windows_np(unitig_bases, unitig_offsets, k)
    G = np.flatnonzero(valid)
    key = np.minimum(f[G], r[G])
    val = (1 + 2 * G + (f[G] > r[G])).astype(np.uint32)
    order = np.argsort(key, kind="stable")
    key, val = key[order], val[order]
    assert not (key[1:] == key[:-1]).any(), "a k-mer occurs twice in the indexed sequences"
    return key, val, len(G)


def hits_np(index, bases, offsets, k):
    key, val, _ = index
    valid, f, r = windows_np(bases, offsets, k)
    out = np.full(len(valid), NO_KMER, np.uint32)
    j = np.flatnonzero(valid)
    c = np.minimum(f[j], r[j])
    at = np.minimum(np.searchsorted(key, c), max(len(key) - 1, 0))
    found = key[at] == c if len(key) else np.zeros(len(j), bool)
    v = np.where(found, val[at] if len(key) else 0, 0).astype(np.uint32)
    t = (f[j] > r[j]).astype(np.uint32)
    out[j] = np.where(found, 1 + ((v - 1) ^ t), 0)
    return out


def runs_np(hits, read_offsets, unitig_offsets, k):
    """runs() on arrays -> {"run_start" u64, "run_len", "run_unitig", "run_upos" u32, "run_offsets" u64, "unitig_hits",
    "unitig_runs" u64, "tally" u64[6]}"""
    hits = np.asarray(hits, np.uint32).astype(np.int64)
    roff = np.asarray(read_offsets, np.int64)
    uoff = np.asarray(unitig_offsets, np.int64)
    nu, total = len(uoff) - 1, len(hits)
    window = hits != NO_KMER
    miss = hits == 0
    cand = window & ~miss
    G, a = (hits - 1) >> 1, (hits - 1) & 1
    u = np.clip(np.searchsorted(uoff, G, "right") - 1, 0, max(nu - 1, 0))
    if nu:
        p = G - uoff[u]
        hit = cand & (G < uoff[-1]) & (p <= uoff[u + 1] - uoff[u] - k)
    else:
        p, hit = G, np.zeros(total, bool)
    first = np.zeros(total + 1, bool)  # a read starts here
    first[roff[:-1][roff[1:] > roff[:-1]]] = True
    cont = np.zeros(total, bool)
    cont[1:] = (hit[1:] & hit[:-1] & ~first[1:total] & (a[1:] == a[:-1]) & (u[1:] == u[:-1])
                & (G[1:] - G[:-1] == np.where(a[1:] == 0, 1, -1)))
    start = hit & ~cont
    s = np.flatnonzero(start)
    rid = np.cumsum(start) - 1
    run_len = np.bincount(rid[hit], minlength=len(s)).astype(np.uint32)
    tally = np.array([window.sum(), hit.sum(), miss.sum(), (cand & ~hit).sum(), len(s), 0], np.uint64)
    run_offsets = np.searchsorted(s, roff, "left").astype(np.uint64)
    tally[5] = (run_offsets[1:] > run_offsets[:-1]).sum()
    return {"run_start": s.astype(np.uint64), "run_len": run_len, "run_unitig": (2 * u[s] + a[s]).astype(np.uint32),
            "run_upos": p[s].astype(np.uint32), "run_offsets": run_offsets,
            "unitig_hits": np.bincount(u[hit], minlength=nu).astype(np.uint64),
            "unitig_runs": np.bincount(u[s], minlength=nu).astype(np.uint64), "tally": tally}


def want_files(table, k, ids, reads, lo=1, hi=gr.U32):
    """table: {canonical string: count}; ids, reads: the threaded records -> {file name: bytes} of `kmertools thread`"""
    us = ur.unitigs(table, k, lo, hi)
    unitigs = [u[0] for u in us]
    res, _ = thread(unitigs, reads, k)
    ulen = [len(s) for s in unitigs]
    gaf, base, n_chains, whole = [], 0, 0, 0
    for rid, r, cs in zip(ids, reads, res["chains"]):
        for c in cs:
            gaf.append(gaf_line(rid, len(r), base, c, ulen, k))
        n_chains += len(cs)
        whole += len(cs) == 1 and len(r) >= k and cs[0][0][0] == base and cs[0][-1][0] - base + cs[0][-1][1] - 1 + k == len(r)
        base += len(r)
    ut = ["%d\t%d\t%d\t%d\t%d\t%d\t%.6f\n" % (i, len(s), n, c, res["unitig_hits"][i], res["unitig_runs"][i], res["unitig_hits"][i] / n)
          for i, (s, c, _, n) in enumerate(us)]
    t = res["tally"]
    stats = [("reads", len(reads)), ("bases", sum(map(len, reads))), ("windows", t[0]), ("hits", t[1]), ("misses", t[2]),
             ("runs", t[4]), ("chains", n_chains), ("reads_with_hit", t[5]), ("reads_one_chain_end_to_end", whole),
             ("unitigs_hit", sum(1 for x in res["unitig_hits"] if x))]
    return {"unitigs.fa": ur.want_files(table, k, lo, hi)[0], "unitigs.gfa": lr.want_gfa(table, k, lo, hi),
            "thread.gaf": "".join(gaf).encode(), "thread.unitigs": "".join(ut).encode(),
            "thread.stats": "".join("%s\t%d\n" % nv for nv in stats).encode()}
