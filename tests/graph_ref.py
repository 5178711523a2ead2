"""What kt_ctr_graph computes, restated twice and independently of each other and of the library:

  brute(...)   on strings: reverse complement by translate + reverse, canon by comparing strings, solidity by a dict
  restate(...) on numpy arrays of 2-bit words: 14 searchsorted lookups per node into a sorted (keys, counts) table

The rule (the header's): a canonical k-mer u is a node when lo <= count(u) <= hi ("solid"; absent = 0).  F = u's own string.
Right bit x: canon(F[1:] + x) solid; left bit 4 + x: canon(x + F[:-1]) solid; dR, dL their popcounts; sibR = #y with
canon(y + F[1:]) solid, sibL = #y with canon(F[:-1] + y) solid; bit 8 (right end): dR != 1 or sibR != 1; bit 9 (left end):
dL != 1 or sibL != 1.  Census: nodes, occurrences, degree sum, end sides, isolated, tips, branching, then cell 7 + 5 dL + dR.
"""
import numpy as np

U32 = 0xFFFFFFFF
ACGT = "ACGT"
CENSUS = 32
_COMP = str.maketrans("ACGT", "TGCA")


# ---- strings ------------------------------------------------------------------------------------------------------------

def rc_s(s):
    return s.translate(_COMP)[::-1]


def canon_s(s):
    r = rc_s(s)
    return s if s <= r else r  # (the order of ACGT strings of one length is the order of their 2-bit words)


def key_of(s):
    v = 0
    for ch in s:
        v = v * 4 + ACGT.index(ch)
    return v


def str_of(key, k):
    return "".join(ACGT[(int(key) >> (2 * (k - 1 - i))) & 3] for i in range(k))


def count_strings(reads, k):
    """{canonical k-mer string: occurrences} of upper-case reads; a window with anything but ACGT is no k-mer"""
    out = {}
    for r in reads:
        for i in range(len(r) - k + 1):
            w = r[i:i + k]
            if all(ch in ACGT for ch in w):
                c = canon_s(w)
                out[c] = out.get(c, 0) + 1
    return out


def info_s(table, F, lo, hi):
    solid = lambda s: lo <= table.get(canon_s(s), 0) <= hi
    info = 0
    for x in range(4):
        if solid(F[1:] + ACGT[x]):
            info |= 1 << x
        if solid(ACGT[x] + F[:-1]):
            info |= 1 << (4 + x)
    dR, dL = bin(info & 0xF).count("1"), bin(info & 0xF0).count("1")
    sibR = sum(solid(y + F[1:]) for y in ACGT)
    sibL = sum(solid(F[:-1] + y) for y in ACGT)
    if dR != 1 or sibR != 1:
        info |= 0x100
    if dL != 1 or sibL != 1:
        info |= 0x200
    return info


def census_of(nodes):
    """nodes: iterable of (key, count, info) -> the 32 census values as a list of ints"""
    cen = [0] * CENSUS
    for _, c, info in nodes:
        dR, dL = bin(info & 0xF).count("1"), bin(info & 0xF0).count("1")
        cen[0] += 1
        cen[1] += int(c)
        cen[2] += dL + dR
        cen[3] += bin(info & 0x300).count("1")
        cen[4] += dL == 0 and dR == 0
        cen[5] += (dL == 0) != (dR == 0)
        cen[6] += dL > 1 or dR > 1
        cen[7 + 5 * dL + dR] += 1
    return cen


def brute(table, k, lo=1, hi=U32):
    """table: {canonical string: count} -> [(key, count, info)] ascending by key"""
    return [(key_of(F), table[F], info_s(table, F, lo, hi)) for F in sorted(table) if lo <= table[F] <= hi]


def mutual_failures(nodes, k):
    """nodes: [(key, count, info)] of one graph.  A side that is not an end has exactly one neighbour, that neighbour is a
    node, and the side of it that faces back is not an end either.  -> the list of violations (empty: the rule is mutual)"""
    info_of = {str_of(key, k): info for key, _, info in nodes}
    bad = []
    for F, info in info_of.items():
        for side, end_bit, shift in (("R", 0x100, 0), ("L", 0x200, 4)):
            if info & end_bit:
                continue
            xs = [x for x in range(4) if info >> (shift + x) & 1]
            if len(xs) != 1:
                bad.append((F, side, "degree", xs))
                continue
            s = F[1:] + ACGT[xs[0]] if side == "R" else ACGT[xs[0]] + F[:-1]
            v = canon_s(s)
            if v not in info_of:
                bad.append((F, side, "neighbour is no node", v))
                continue
            # u's string leaves s on the left (side R: s = F[1:] + x follows F) or on the right (side L): as v's own string
            # that is v's left / right side; as v's reverse complement the sides swap; a palindromic s faces both ways
            facing = []
            if s == v:
                facing.append(0x200 if side == "R" else 0x100)
            if rc_s(s) == v:
                facing.append(0x100 if side == "R" else 0x200)
            for bit in facing:
                if info_of[v] & bit:
                    bad.append((F, side, "the facing side is an end", v))
    return bad


# ---- numpy ----------------------------------------------------------------------------------------------------------------

def rc_np_loop(x, k):
    """base by base: what rc_np must equal"""
    x = np.asarray(x, np.uint64).copy()
    r = np.zeros_like(x)
    for _ in range(k):
        r = (r << np.uint64(2)) | (np.uint64(3) - (x & np.uint64(3)))
        x >>= np.uint64(2)
    return r


# the reverse complement of the four bases of a byte
_RC_BYTE = np.array([sum((3 - (b >> (2 * i) & 3)) << (2 * (3 - i)) for i in range(4)) for b in range(256)], np.uint8)


def rc_np(x, k):
    """a table look-up per byte and the bytes in reverse order (little-endian words), then down to the low 2k bits"""
    x = np.ascontiguousarray(x, "<u8")
    b = _RC_BYTE[x.view(np.uint8).reshape(-1, 8)[:, ::-1]]
    return np.ascontiguousarray(b).view("<u8").reshape(x.shape) >> np.uint64(64 - 2 * k)


def canon_np(x, k):
    return np.minimum(x, rc_np(x, k))


def restate(keys, counts, k, lo=1, hi=None):
    """keys (canonical, distinct), counts of a table -> (keys ascending, info u32, counts u32, census u64[32]) of its graph"""
    hi = U32 if hi is None else hi
    order = np.argsort(keys)
    tk, tc = np.asarray(keys, np.uint64)[order], np.asarray(counts, np.uint32)[order]
    node = (tc >= lo) & (tc <= hi)
    F, c = tk[node], tc[node]
    cen = np.zeros(CENSUS, np.uint64)
    if not len(F):
        return F, np.zeros(0, np.uint32), c, cen

    def solid(s):
        s = canon_np(s, k)
        i = np.minimum(np.searchsorted(tk, s), len(tk) - 1)
        cs = np.where(tk[i] == s, tc[i], 0)
        return (cs >= lo) & (cs <= hi)

    two = np.uint64(2)
    top = np.uint64(2 * k - 2)
    mask = np.uint64((1 << (2 * k)) - 1)
    low = np.uint64((1 << (2 * k - 2)) - 1)  # the last k - 1 bases
    info = np.zeros(len(F), np.uint32)
    sibR = np.zeros(len(F), np.uint32)
    sibL = np.zeros(len(F), np.uint32)
    for x in range(4):
        ux = np.uint64(x)
        info |= solid(((F << two) & mask) | ux).astype(np.uint32) << np.uint32(x)          # F[1:] + x
        info |= solid((F >> two) | (ux << top)).astype(np.uint32) << np.uint32(4 + x)      # x + F[:-1]
        sibR += solid((F & low) | (ux << top))                                             # y + F[1:]
        sibL += solid((F & ~np.uint64(3)) | ux)                                            # F[:-1] + y
    dR = sum(((info >> np.uint32(x)) & 1) for x in range(4))
    dL = sum(((info >> np.uint32(4 + x)) & 1) for x in range(4))
    info |= np.where((dR != 1) | (sibR != 1), 0x100, 0).astype(np.uint32)
    info |= np.where((dL != 1) | (sibL != 1), 0x200, 0).astype(np.uint32)
    cen[0] = len(F)
    cen[1] = int(c.astype(np.uint64).sum())
    cen[2] = int(dL.sum() + dR.sum())
    cen[3] = int(((info >> 8) & 1).sum() + ((info >> 9) & 1).sum())
    cen[4] = int(((dL == 0) & (dR == 0)).sum())
    cen[5] = int(((dL == 0) != (dR == 0)).sum())
    cen[6] = int(((dL > 1) | (dR > 1)).sum())
    cells = np.bincount((5 * dL + dR).astype(np.int64), minlength=25)
    cen[7:] = cells.astype(np.uint64)
    return F, info, c, cen


def info_text(info):
    info = int(info)
    right = "".join(ACGT[x] if info >> x & 1 else "." for x in range(4))
    left = "".join(ACGT[x] if info >> (4 + x) & 1 else "." for x in range(4))
    return left, right, ("L" if info & 0x200 else ".") + ("R" if info & 0x100 else ".")


CENSUS_NAMES = ["nodes", "occurrences", "degree_sum", "end_sides", "isolated", "tips", "branching"] + [
    "degree_%d_%d" % (a, b) for a in range(5) for b in range(5)]


def want_files(keys, counts, k, lo=1, hi=None, acgt=False):
    """the restated graph.nodes and graph.stats of a table"""
    F, info, c, cen = restate(keys, counts, k, lo, hi)
    lines = []
    for key, cc, i in zip(F, c, info):
        name = str_of(key, k) if acgt else "%d" % int(key)
        lines.append("%s\t%d\t%s\t%s\t%s\n" % ((name, int(cc)) + info_text(i)))
    stats = "".join("%s\t%d\n" % (n, int(v)) for n, v in zip(CENSUS_NAMES, cen))
    return "".join(lines).encode(), stats.encode(), len(F)
