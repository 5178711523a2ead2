"""Read batches for the tests, as plain helpers (no test in here): the CSR `Batch`, the noisy ragged reads and the buffer
views / guard bands that tests/test_buffer_views.py introduced, the seeded batch families of
tests/test_read_boundaries.py - reads far shorter than a 16-base lane, long runs of empty reads, read ends placed on the
kernels' structural constants, reads of one length - with the numbers that say, from the offsets alone, that a batch
has the shape it is meant to have, and the content families of tests/test_read_content.py - every byte value at every
position of a 32-base item, with and without a raw code next to it, and reads of nothing but the 14 valid bytes - with
the check that says, from the bytes and offsets alone, that every (value, position) pair is there.  Also the per-read
oracle answers as flat arrays, a pure-Python brute force of "the k-mers of a read" that shares no code with the oracle,
and the text that says where a result differs.

Vocabulary (kmertools_amd/csrc): a *lane* is 16 consecutive bases starting at a multiple of 16 (one thread's load in
kt_oligo.hip, one thread's positions in kt_min.hip); a *segment* is 8192 bases starting at a multiple of 8192 (one
workgroup's share in kt_segment.hpp / kt_bulk.hip); a *tile* of the LDS oligo kernel is R consecutive reads.  A batch
handed over at an address that is 0 mod 16 has its lanes where these helpers count them."""
import numpy as np

SLACK = 4096
GUARD = 0xA5
ACGT = np.frombuffer(b"ACGT", np.uint8)
LETTERS = np.frombuffer(b"ACGTUacgtu", np.uint8)      # everything kt_cgr_points accepts
VALID = np.frombuffer(b"ACGTUacgtu\x00\x01\x02\x03", np.uint8)   # every byte that is a nucleotide: the letters and the raw codes
ALPHA_LEN, ALPHA_FIRST, ALPHA_STEP, ALPHA_TIMES = 1104, 32, 33, 32   # alphabet_batch: a read, its first occurrence, their distance
LANE, SEG = 16, 8192
EMPTY_RUNS = (1, 63, 64, 65, 256, 257, 5000)
LATTICE = (16, 32, 64, 128, 256, 1008, 1024, 2048, 4096, 7168, 8192)   # 256: kt_sketch.hip's chunks, 2048: a wave's span of a segment
EQUAL_LENGTHS = (16, 17, 31, 32, 33, 63, 64, 65, 255, 256, 257, 1007, 1008, 1009)   # + 16 + k - 2 and 16 + k - 1


# ---- a batch ---------------------------------------------------------------------------------------------------------------

class Batch:
    def __init__(self, name, seqs):
        from kmertools_amd import device
        self.name, self.seqs = name, seqs
        self.bases, self.offsets = device.to_csr(seqs)
        self.n = len(seqs)
        self.total = int(self.offsets[-1])
        self.meta = {}

    @classmethod
    def of_lens(cls, name, bases, lens, **meta):
        """a batch from its bases and read lengths (numpy arrays)"""
        b = cls.__new__(cls)
        lens = np.asarray(lens, np.int64)
        b.name, b.n = name, len(lens)
        b.offsets = np.zeros(b.n + 1, np.uint64)
        b.offsets[1:] = np.cumsum(lens)
        b.total = int(b.offsets[-1])
        assert b.total == len(bases)
        b.bases = np.ascontiguousarray(bases, np.uint8)
        raw, o = b.bases.tobytes(), b.offsets.astype(np.int64).tolist()
        b.seqs = [raw[o[i]:o[i + 1]] for i in range(b.n)]
        b.meta = meta
        return b

    @property
    def lens(self):
        return np.diff(self.offsets.astype(np.int64))


def noisy_reads(seed, n, max_len=400):
    """empty reads, reads shorter than k, N runs, lower case, U, raw 0..3 codes, IUPAC bytes, reads over several 8192-base
    segments; the batch ends off a 16- and a 32-byte boundary"""
    rng = np.random.default_rng(seed)
    lens = rng.integers(0, max_len, size=n)
    lens[:8] = (0, 1, 2, 31, 64, 0, 9000, 8192)
    seqs = []
    for L in lens:
        s = ACGT[rng.integers(0, 4, size=L)].copy()
        if L:
            m = rng.random(L)
            s[m < 0.01] = ord("N")
            s[(m > 0.01) & (m < 0.05)] |= 0x20
            s[(m > 0.05) & (m < 0.055)] = ord("U")
            s[(m > 0.055) & (m < 0.057)] = 2
            s[(m > 0.057) & (m < 0.059)] = ord("R")
        if L > 100 and rng.random() < 0.1:
            a = int(rng.integers(0, L - 30))
            s[a:a + 25] = ord("N")
        seqs.append(s.tobytes())
    total = sum(len(s) for s in seqs)
    tail = next(t for t in range(1, 40) if (total + t) % 16)
    seqs.append(ACGT[rng.integers(0, 4, size=tail)].tobytes())
    return seqs


# ---- views and guard bands ---------------------------------------------------------------------------------------------------

def _place(addr, slack, mod):
    """offset from addr of the first address >= addr + slack that is `mod` past a 256-byte boundary"""
    return ((addr + slack + 255) & ~255) + mod - addr


def bases_view(torch, bases, shift, slack=SLACK, seed=0):
    """the bases inside one device buffer of random ACGT bytes, starting `shift` bytes after a 256-byte boundary, with
    >= slack bytes of poison on both sides"""
    n = len(bases)
    raw = torch.from_numpy(ACGT[np.random.default_rng(seed + 1000 * shift).integers(0, 4, size=2 * slack + 512 + n)]).cuda()
    start = _place(raw.data_ptr(), slack, shift)
    v = raw[start:start + n]
    if n:
        v.copy_(torch.from_numpy(np.ascontiguousarray(bases)))
    assert v.data_ptr() % 256 == shift and raw.numel() - (start + n) >= slack
    return v


def offsets_view(torch, offsets):
    """the int64 offsets at an address that is 8 mod 16 (one leading element)"""
    raw = torch.zeros(len(offsets) + 2, dtype=torch.int64, device="cuda")
    raw[1:len(offsets) + 1] = torch.from_numpy(np.asarray(offsets).astype(np.int64))
    v = raw[1:len(offsets) + 1]
    assert v.data_ptr() % 16 == 8
    return v


def host_bases_view(bases, shift, slack=SLACK):
    """host-mode counterpart of bases_view: a numpy slice at `shift` past a 256-byte boundary inside random ACGT"""
    n = len(bases)
    raw = ACGT[np.random.default_rng(7 + shift).integers(0, 4, size=2 * slack + 512 + n)]
    start = _place(raw.ctypes.data, slack, shift)
    v = raw[start:start + n]
    v[:] = bases
    return v


class Fenced:
    """a device output of `shape` / `dtype` at `align` past a 256-byte boundary, inside guard bands of GUARD bytes;
    prefill: the body's initial value (default: the guard byte itself)"""

    def __init__(self, torch, shape, dtype, guard=4096, align=0, prefill=None):
        shape = tuple(shape) if isinstance(shape, (tuple, list)) else (int(shape),)
        nbytes = int(np.prod(shape)) * torch.empty(0, dtype=dtype).element_size()
        self.raw = torch.full((2 * guard + 512 + nbytes,), GUARD, dtype=torch.uint8, device="cuda")
        self.lo = _place(self.raw.data_ptr(), guard, align)
        self.hi = self.lo + nbytes
        self.t = self.raw[self.lo:self.hi].view(dtype).view(shape)
        assert self.t.data_ptr() % 256 == align
        if prefill is not None:
            self.t.copy_(torch.as_tensor(prefill).to(dtype).view(shape))

    def check(self, what=""):
        head = self.raw[:self.lo].cpu().numpy()
        tail = self.raw[self.hi:].cpu().numpy()
        assert (head == GUARD).all(), ("written before the output", what, self.lo - np.flatnonzero(head != GUARD)[-8:])
        assert (tail == GUARD).all(), ("written after the output", what, np.flatnonzero(tail != GUARD)[:8])

    def np(self, dtype):
        return self.t.cpu().numpy().view(dtype)


class HostFenced:
    """the same for host-mode calls: a numpy body between guard bands"""

    def __init__(self, shape, dtype, guard=4096, prefill=None):
        shape = tuple(shape) if isinstance(shape, (tuple, list)) else (int(shape),)
        nbytes = int(np.prod(shape)) * np.dtype(dtype).itemsize
        self.raw = np.full(2 * guard + nbytes, GUARD, np.uint8)
        self.lo, self.hi = guard, guard + nbytes
        self.a = self.raw[self.lo:self.hi].view(dtype).reshape(shape)
        if prefill is not None:
            self.a[...] = prefill

    def check(self, what=""):
        assert (self.raw[:self.lo] == GUARD).all(), ("written before the output", what)
        assert (self.raw[self.hi:] == GUARD).all(), ("written after the output", what,
                                                     np.flatnonzero(self.raw[self.hi:] != GUARD)[:8])


# ---- the batch families ----------------------------------------------------------------------------------------------------

def _random_bases(rng, total, letters):
    alpha = LETTERS if letters else ACGT
    return alpha[rng.integers(0, len(alpha), size=total)].copy()


def _sprinkle(rng, bases, offsets=None, clear=0):
    """noise as in noisy_reads at a rate that leaves most windows of 31 bases valid (0.6 % of the bytes are no
    nucleotide): N, lower case, U, a raw 0..3 code, an IUPAC letter; `clear`: the bases closer than that to a read start
    or end stay as they are (valid ACGT on both sides of every junction)"""
    keep = bases.copy()
    m = rng.random(len(bases))
    bases[m < 0.004] = ord("N")
    bases[(m > 0.004) & (m < 0.04)] |= 0x20
    bases[(m > 0.04) & (m < 0.044)] = ord("U")
    bases[(m > 0.044) & (m < 0.046)] = 2
    bases[(m > 0.046) & (m < 0.048)] = ord("R")
    if clear and offsets is not None and len(bases):
        edges = np.unique(np.asarray(offsets, np.int64))
        pos = np.arange(len(bases), dtype=np.int64)
        at = np.searchsorted(edges, pos, side="right")                    # edges[at - 1] <= pos < edges[at]
        near = np.minimum(pos - edges[at - 1], edges[np.minimum(at, len(edges) - 1)] - 1 - pos) < clear
        bases[near] = keep[near]
    return bases


def tiny_batch(seed, k, n, letters=False, min_len=0, core=(30, 120)):
    """family A: a deterministic core, then n reads of min_len + 0..8 bases, n / 2 of min_len + 0..2k (2k capped at 47: a mean
    below 24) and n / 4 of min_len + 12..34 (a mean of 23: segments with 257..512 read starts whatever k is).  The core
    (none with min_len) starts at base 0 and is made of whole lanes, so that the batch has its shape however few random
    reads follow: core[0] lanes of a read of rem bases and one of 16 - rem (rem = 1..15 in turn: the following read ends
    on the lane's last base), core[1] lanes of three reads of a, b and 16 - a - b bases (a, b in 1..4)"""
    rng = np.random.default_rng(seed)
    head = []
    if not min_len:
        for i in range(core[0]):
            head += [1 + i % 15, 15 - i % 15]
        for i in range(core[1]):
            a, b = 1 + i % 4, 1 + (i // 4) % 4
            head += [a, b, LANE - a - b]
    lens = np.concatenate([np.array(head, np.int64),
                           min_len + np.concatenate([rng.integers(0, 9, size=n), rng.integers(0, min(2 * k, 47) + 1, size=n // 2),
                                                     rng.integers(12, 35, size=n // 4)])])
    bases = _random_bases(rng, int(lens.sum()), letters)
    if not letters:
        _sprinkle(rng, bases)
    return Batch.of_lens("tiny(seed=%d,k=%d,n=%d,letters=%s,min_len=%d,core=%s)" % (seed, k, n, letters, min_len, core if not min_len else None),
                         bases, lens)


def _fill(rng, lens, pos, target, lo=17, hi=300):
    """appends filler reads of lo..hi bases that bring the batch from pos to exactly target (target - pos >= lo)"""
    gap = target - pos
    assert gap >= lo
    while gap > hi:
        L = int(rng.integers(lo, hi + 1))
        if gap - L < lo:
            L = gap - lo
        lens.append(L)
        gap -= L
    lens.append(gap)
    return target


def empty_runs_batch(seed, runs=EMPTY_RUNS, first=None, last=None, letters=False, filler=(17, 300)):
    """family B: runs of empty reads between ordinary reads of 17..300 bases, directly after a read that ends on a multiple of
    8192, at the very start (`first` empty reads, default the longest run) and at the very end (`last`, default the
    second longest); meta["runs"] = [(index of the run's first read, its length, where: "start" / "between" / "aligned" /
    "end")]"""
    rng = np.random.default_rng(seed)
    first = max(runs) if first is None else first
    last = sorted(runs)[-2] if last is None else last
    lo, hi = filler
    lens, where, pos = [0] * first, [(0, first, "start")], 0
    for r in runs:                                      # between ordinary reads, at whatever position they end
        for _ in range(3):
            lens.append(int(rng.integers(lo, hi + 1)))
            pos += lens[-1]
        where.append((len(lens), r, "between"))
        lens += [0] * r
    for r in runs:                                      # after a read whose last base is the last of a segment
        pos = _fill(rng, lens, pos, (pos + lo + SEG - 1) // SEG * SEG, lo, hi)
        where.append((len(lens), r, "aligned"))
        lens += [0] * r
        lens.append(int(rng.integers(lo, hi + 1)))
        pos += lens[-1]
    where.append((len(lens), last, "end"))
    lens += [0] * last
    bases = _random_bases(rng, pos, letters)
    if not letters:
        _sprinkle(rng, bases)
    return Batch.of_lens("empty_runs(seed=%d,runs=%s,first=%d,last=%d,letters=%s,filler=%s)" % (
        seed, list(runs), first, last, letters, filler), bases, lens,
                         runs=where)


def lattice_batch(seed, k, consts=LATTICE, letters=False, filler=(17, 300), poly_a=False, min_len=0):
    """family C: for every structural constant c, every d in -1, 0, +1 and every follow length f in 0, 1, k-1, k, k+1 a read
    that ends at m c + d followed by a read of f bases, filler reads in between; then, for every rem in 1..15, a read that
    ends rem bases into a lane followed by one of 16 - rem bases (it ends on the lane's last base); with poly_a a 300-base
    poly-A read that starts 1, 63, 64, 65 bases before a multiple of 128.  The bases within 32 of a read end are valid
    ACGT.  min_len > 0 (callers that define nothing for a shorter read): the follow lengths are min_len more and the
    reads that end on a lane's last base are left out.  meta["junctions"] = [(c, d, f, position of the read end, index
    of the follow read)], meta["lane_ends"] = [(rem, index of the follow read)], meta["poly_a"] = [(bases before the
    multiple of 128, index of the read)]"""
    rng = np.random.default_rng(seed)
    lo, hi = filler
    lens, pos, junctions, lane_ends, polys = [], 0, [], [], []
    follows = sorted({min_len + x for x in (0, 1, k - 1, k, k + 1)})
    for c in consts:
        for d in (-1, 0, 1):
            for f in follows:
                target = (pos + lo - d + c - 1) // c * c + d
                pos = _fill(rng, lens, pos, target, lo, hi)
                junctions.append((c, d, f, target, len(lens)))
                lens.append(f)
                pos += f
    for rem in range(1, LANE if not min_len else 1):
        pos = _fill(rng, lens, pos, (pos + lo - rem + LANE - 1) // LANE * LANE + rem, lo, hi)
        lane_ends.append((rem, len(lens)))
        lens.append(LANE - rem)
        pos += LANE - rem
    a_at = []
    if poly_a:
        for before in (1, 63, 64, 65):
            pos = _fill(rng, lens, pos, (pos + lo + before + 127) // 128 * 128 - before, lo, hi)
            polys.append((before, len(lens)))
            a_at.append(pos)
            lens.append(300)
            pos += 300
    lens.append(int(rng.integers(lo, hi + 1)))
    pos += lens[-1]
    bases = _random_bases(rng, pos, letters)
    offsets = np.concatenate(([0], np.cumsum(lens)))
    if not letters:
        _sprinkle(rng, bases, offsets, clear=32)
    for a in a_at:
        bases[a:a + 300] = ord("A")
    return Batch.of_lens("lattice(seed=%d,k=%d,consts=%s,letters=%s,filler=%s,poly_a=%s,min_len=%d)" % (
        seed, k, list(consts), letters, filler, poly_a, min_len), bases, lens, junctions=junctions,
                         lane_ends=lane_ends, poly_a=polys)


def equal_lengths(k):
    return tuple(sorted(set(EQUAL_LENGTHS) | {16 + k - 2, 16 + k - 1}))


def equal_batch(seed, L, n):
    """family D: n reads of L bases, N and lower case sprinkled in"""
    rng = np.random.default_rng(seed + 7919 * L)
    bases = _sprinkle(rng, _random_bases(rng, n * L, False))
    return Batch.of_lens("equal(seed=%d,L=%d,n=%d)" % (seed, L, n), bases, np.full(n, L))


def equal_concat_batch(seed, k, per=5):
    """the lengths of family D in one batch, `per` reads of each: what the kernels without an equal-length path see of it"""
    rng = np.random.default_rng(seed)
    lens = np.repeat(np.array(equal_lengths(k)), per)
    bases = _sprinkle(rng, _random_bases(rng, int(lens.sum()), False))
    return Batch.of_lens("equal_concat(seed=%d,k=%d,per=%d)" % (seed, k, per), bases, lens)


def mixed_tiles_batch(seed, R):
    """family D, mixed: tiles of R reads - equal (40), ragged, equal (40), ragged, all 9 bases (equal but shorter than a
    lane), equal (33), equal (40) except for its last read, equal (17) - and one read more; meta["tiles"] names them"""
    rng = np.random.default_rng(seed)
    kinds = ("equal40", "ragged", "equal40", "ragged", "short9", "equal33", "last_differs", "equal17")
    lens = []
    for kind in kinds:
        if kind == "ragged":
            t = rng.integers(0, 60, size=R)
            if R > 1:
                t[0], t[-1] = 21, 3                      # (never equal by accident)
            else:
                t[0] = 21
        elif kind == "short9":
            t = np.full(R, 9)
        elif kind == "last_differs":
            t = np.full(R, 40)
            t[-1] = 41
        else:
            t = np.full(R, int(kind[5:]))
        lens += [int(x) for x in t]
    lens.append(25)
    bases = _sprinkle(rng, _random_bases(rng, int(np.sum(lens)), False))
    return Batch.of_lens("mixed_tiles(seed=%d,R=%d)" % (seed, R), bases, lens, tiles=kinds)


# ---- what the bytes are: every value at every position of an item ------------------------------------------------------------

def alphabet_batch(seed, raw_neighbour=False, ragged=False, values=range(256)):
    """one read per byte value v: 1104 random ACGT bases (69 lanes, more than the oligo kernel's 1008-byte chunk) with v at the
    read positions 32 + 33 i, i = 0..31 - 33 apart, so that their batch positions take 32 consecutive residues modulo 32 (every
    byte of a dword, every dword of a lane's 16-byte load, both lanes of a 32-base item), with 32 valid bases between two of
    them and at both read ends (valid windows of 31 on both sides of each).  raw_neighbour: a raw code (v + i) & 3 sits
    1 + (v + i) % 15 bases behind each occurrence - in the same item or the next lane, always in the same wave.  That puts v
    and the letters around it on the oligo kernel's per-byte path at every position, and on the per-item one of
    kt_segment.hpp where the raw code shares v's 32-base item: always at the positions 0..16 mod 32, never at 31, in between
    as the distance has it (check_alphabet says for which positions).  ragged: v % 7 more valid bases in front of each read -
    the reads differ in length (the oligo kernel's general path) and the items are no longer aligned with them.  meta["values"]: read i is
    byte values[i]"""
    rng = np.random.default_rng(seed)
    values = [int(v) for v in values]
    lens = np.array([ALPHA_LEN + (v % 7 if ragged else 0) for v in values], np.int64)
    bases = _random_bases(rng, int(lens.sum()), False)
    start = np.concatenate(([0], np.cumsum(lens)))[:-1]
    for v, s, L in zip(values, start.tolist(), lens.tolist()):
        first = s + L - ALPHA_LEN + ALPHA_FIRST
        for i in range(ALPHA_TIMES):
            p = first + ALPHA_STEP * i
            bases[p] = v
            if raw_neighbour:
                bases[p + 1 + (v + i) % 15] = (v + i) & 3
    return Batch.of_lens("alphabet(seed=%d,raw_neighbour=%s,ragged=%s,%d values)" % (seed, raw_neighbour, ragged, len(values)),
                         bases, lens, values=values)


def valid_mix_batch(seed, n, alphabet=VALID, min_len=0):
    """n ragged reads of 0..400 bases, every byte drawn uniformly from the 14 valid ones (ACGTUacgtu and the raw codes 0..3):
    every window is a k-mer, and nearly every item and wave is on the per-byte path with letters in it.  alphabet=LETTERS:
    the letters alone (for kt_cgr_points); min_len: no read is shorter (callers that define nothing for a shorter one)"""
    rng = np.random.default_rng(seed)
    lens = rng.integers(min_len, 401, size=n)
    lens[:4] = (min_len, 400, min_len + 1, min_len)
    total = int(lens.sum())
    assert total <= 600_000, total
    alphabet = np.asarray(alphabet, np.uint8)
    bases = alphabet[rng.integers(0, len(alphabet), size=total)].copy()
    return Batch.of_lens("valid_mix(seed=%d,n=%d,%d byte values,min_len=%d)" % (seed, n, len(alphabet), min_len), bases, lens)


def _valid_runs(bases, offsets):
    """-> (left, right): the valid nucleotide bytes directly in front of / behind each base, inside its read"""
    total = len(bases)
    pos = np.arange(total, dtype=np.int64)
    ok = np.isin(bases, VALID)
    o = np.asarray(offsets, np.int64)
    rid = np.searchsorted(o, pos, side="right") - 1
    last_bad = np.maximum.accumulate(np.where(ok, -1, pos))            # the last invalid byte at or before pos
    prev_bad = np.concatenate(([-1], last_bad[:-1]))                   # ... before pos
    left = pos - np.maximum(prev_bad + 1, o[rid])
    next_bad = np.minimum.accumulate(np.where(ok, total, pos)[::-1])[::-1]
    next_bad = np.concatenate((next_bad[1:], [total]))                 # the first invalid byte behind pos
    right = np.minimum(next_bad, o[rid + 1]) - 1 - pos
    return left, right


def check_alphabet(batch, raw_neighbour, values=range(256)):
    """from the bytes and offsets alone: for every value v and every residue q in 0..31 an occurrence of v at a batch position
    = q mod 32 with at least 31 valid nucleotide bytes on either side inside its read and, with raw_neighbour, a raw code
    1..15 bases behind it; without, none (v itself apart) within 32 bases on either side: it is v alone that chooses the
    encoder.  With raw_neighbour, batch.meta["same_item"][v] is the set of positions mod 32 at which that raw code lies in
    v's own 32-base item (asserted: all of 0..16, and 20 of the 32 at least).  -> the number of such occurrences"""
    bases = batch.bases
    total = len(bases)
    left, right = _valid_runs(bases, batch.offsets)
    good = (left >= 31) & (right >= 31)
    c = np.concatenate(([0], np.cumsum(bases < 4)))
    pos = np.arange(total, dtype=np.int64)
    near = c[np.minimum(pos + 16, total)] - c[np.minimum(pos + 1, total)] > 0       # (right >= 31: those 15 are in the read)
    if raw_neighbour:
        good &= near
    else:
        good &= c[np.minimum(pos + 33, total)] - c[np.minimum(pos + 1, total)] + c[pos] - c[np.maximum(pos - 32, 0)] == 0
    values = np.array([int(v) for v in values], np.int64)
    seen = np.unique(bases[good].astype(np.int64) * 32 + pos[good] % 32)
    want = (values[:, None] * 32 + np.arange(32)[None, :]).ravel()
    missing = np.setdiff1d(want, seen)
    assert not len(missing), (batch.name, "byte %#04x never at a position = %d mod 32 with valid windows on both sides%s" % (
        missing[0] // 32, missing[0] % 32, " and a raw code behind it" if raw_neighbour else ""), len(missing))
    if raw_neighbour:
        rest = 31 - pos % 32                                                # bases of the item behind pos
        c_item = c[np.minimum(pos + 1 + np.minimum(rest, 15), total)] - c[np.minimum(pos + 1, total)] > 0
        shared = good & c_item & np.isin(bases, values)
        same = {int(v): set() for v in values}
        for v, q in zip(bases[shared].tolist(), (pos[shared] % 32).tolist()):
            same[v].add(q)
        assert all(set(range(17)) <= qs and 31 not in qs and len(qs) >= 20 for qs in same.values()), batch.name
        batch.meta["same_item"] = same
    return int(np.isin(bases[good], values).sum())


def check_valid_mix(batch, alphabet=VALID, min_len=0):
    """all of the alphabet's bytes occur, and no other; the shortest and the longest reads are there; with raw codes in the
    alphabet next to no 32-base item is without one"""
    assert np.array_equal(np.unique(batch.bases), np.sort(np.asarray(alphabet, np.uint8))), batch.name
    lens = batch.lens
    assert (lens == min_len).any() and (lens == 400).any() and (lens < min_len + 16).any() and lens.min() == min_len, batch.name
    assert batch.total <= 600_000, (batch.name, batch.total)
    if (np.asarray(alphabet) < 4).any():
        items = (batch.bases[:batch.total // 32 * 32].reshape(-1, 32) < 4).any(axis=1)
        assert items.mean() > 0.99, (batch.name, items.mean())


def long_stretch_batch(seed, stretch, n_long=6, gap=24):
    """for the windows wider than the reads of the other content batches: n_long reads, each a stretch of `stretch` bytes
    drawn from the 14 valid ones, then its share of the 256 byte values, each followed by `gap` valid bytes, then another
    such stretch; between them a read shorter than the window, an empty one and one of a single stretch.  meta["planted"]:
    the position of each byte value"""
    rng = np.random.default_rng(seed)
    draw = lambda n: VALID[rng.integers(0, len(VALID), size=n)]   # noqa: E731
    parts, lens, planted, pos = [], [], {}, 0
    share = np.array_split(np.arange(256), n_long)
    for j in range(n_long):
        read = [draw(stretch)]
        at = pos + stretch
        for v in share[j].tolist():
            planted[v] = at
            read += [np.array([v], np.uint8), draw(gap)]
            at += 1 + gap
        read.append(draw(stretch))
        parts += read
        lens.append(sum(len(x) for x in read))
        pos += lens[-1]
        for extra in ((300, 0, stretch) if j == 0 else ()):
            parts.append(draw(extra))
            lens.append(extra)
            pos += extra
    b = Batch.of_lens("long_stretch(seed=%d,stretch=%d,n_long=%d,gap=%d)" % (seed, stretch, n_long, gap),
                      np.concatenate(parts), lens, planted=planted)
    return b


def check_long_stretch(batch, window):
    """every byte value is planted once, with `gap` valid bytes behind it and a valid one in front; every read of more than
    two windows begins and ends with more than `window` valid bytes; all 14 valid bytes occur in them"""
    left, right = _valid_runs(batch.bases, batch.offsets)
    at = np.array([batch.meta["planted"][v] for v in range(256)], np.int64)
    assert (batch.bases[at] == np.arange(256)).all() and (left[at] >= 1).all() and (right[at] >= 1).all(), batch.name
    o = batch.offsets.astype(np.int64)
    long_reads = np.flatnonzero(batch.lens > 2 * window)
    assert len(long_reads) >= 2, batch.name
    for i in long_reads.tolist():
        assert right[o[i]] >= window and left[o[i + 1] - 1] >= window, (batch.name, i)
        assert len(np.unique(batch.bases[o[i]:o[i] + window])) == len(VALID), (batch.name, i)
    assert (batch.lens == 0).any() and ((batch.lens > 0) & (batch.lens < window)).any(), batch.name


# ---- what a batch looks like, from its offsets alone --------------------------------------------------------------------------

def starts_per(offsets, unit):
    """read starts (empty reads included) in each block of `unit` bases"""
    o = np.asarray(offsets, np.int64)
    return np.bincount(o[:-1] // unit, minlength=int(o[-1]) // unit + 1)


def shape_numbers(offsets):
    """-> dict: segments with more than 512 / with 257..512 read starts, the most read starts in a segment, lanes with three
    or more read starts, lanes whose following read ends on the lane's last base (the lane's base 0 lies in a read that
    ends rem < 16 bases on, the next read has exactly 16 - rem bases) and the set of those rem"""
    o = np.asarray(offsets, np.int64)
    seg, lane = starts_per(o, SEG), starts_per(o, LANE)
    s, e, ps = o[1:-1], o[2:], o[:-2]                     # read j = 1 .. n - 1: its start, its end, its predecessor's start
    hit = (s % LANE != 0) & (e % LANE == 0) & (e - s < LANE) & (e > s) & (ps <= s - s % LANE) & (ps < s)
    return {"segments_over_512": int((seg > 512).sum()), "segments_257_512": int(((seg >= 257) & (seg <= 512)).sum()),
            "max_starts_per_segment": int(seg.max(initial=0)), "lanes_3_starts": int((lane >= 3).sum()),
            "lane_end_reads": int(hit.sum()), "lane_end_rems": sorted(set((s[hit] % LANE).tolist()))}


def split_first_lane_tiles(offsets, R):
    """tiles (R reads each) behind the first that start off a 16-byte boundary, whose first read ends inside its first lane
    and whose second read ends in that same lane: kt_oligo.hip's process_chunk, t0 < 0 and slow"""
    o = np.asarray(offsets, np.int64)
    n = len(o) - 1
    if R < 2:                                             # (a tile of one read has no second read)
        return 0
    r0 = np.arange(R, n - 1, R)                           # tiles with at least two reads
    sh = o[r0] % LANE
    rem = o[r0 + 1] - o[r0] + sh
    len1 = o[r0 + 2] - o[r0 + 1]
    return int(((sh != 0) & (rem < LANE) & (len1 < LANE - rem)).sum())


def where(batch, i):
    """read i for a failure message: its length, its neighbours' lengths, where it starts"""
    o = batch.offsets.astype(np.int64)
    i = int(min(max(i, 0), batch.n - 1))
    s = int(o[i])
    ln = [int(o[j + 1] - o[j]) if 0 <= j < batch.n else None for j in (i - 1, i, i + 1)]
    return "read %d of %d: length %s (previous %s, next %s), start %d = %d mod 16, %d mod 32, %d mod 8192" % (
        i, batch.n, ln[1], ln[0], ln[2], s, s % 16, s % 32, s % 8192)


def read_of(batch, pos):
    """the read that holds base `pos` (the last one that starts at or before it)"""
    return int(np.searchsorted(batch.offsets.astype(np.int64), int(pos), side="right") - 1)


# ---- the oracle, read by read, into flat arrays ------------------------------------------------------------------------------

def oracle_kmers_flat(oracle, batch, k):
    """oracle.kmers of every read -> (fwd, rev, end index in the batch), in read order: one call of the oracle's kmers per
    read, each on that read's bytes alone"""
    import ctypes as C
    L = oracle.lib()
    u8p, u64p = C.POINTER(C.c_uint8), C.POINTER(C.c_uint64)
    fwd = np.zeros(batch.total + 1, np.uint64)
    rev = np.zeros(batch.total + 1, np.uint64)
    end = np.zeros(batch.total + 1, np.uint64)
    base = np.concatenate([batch.bases, np.zeros(1, np.uint8)])
    pb, pf, pr, pe = base.ctypes.data, fwd.ctypes.data, rev.ctypes.data, end.ctypes.data
    o = batch.offsets.astype(np.int64).tolist()
    got = 0
    for i in range(batch.n):
        n = o[i + 1] - o[i]
        if n < k:
            continue
        c = L.kto_kmers(C.cast(pb + o[i], u8p), n, k, C.cast(pf + 8 * got, u64p), C.cast(pr + 8 * got, u64p),
                        C.cast(pe + 8 * got, u64p))
        end[got:got + c] += np.uint64(o[i])
        got += c
    return fwd[:got].copy(), rev[:got].copy(), end[:got].copy()


def oracle_minimisers_flat(oracle, batch, w, m):
    """oracle.minimisers of every read -> (ev_offsets u64[n + 1], kmers, starts, ends); w = 0: the read's own length"""
    import ctypes as C
    L = oracle.lib()
    u8p, u64p = C.POINTER(C.c_uint8), C.POINTER(C.c_uint64)
    o = batch.offsets.astype(np.int64).tolist()
    room = max((o[i + 1] - o[i] for i in range(batch.n)), default=0) + 2
    km, st, en = np.zeros(room, np.uint64), np.zeros(room, np.uint64), np.zeros(room, np.uint64)
    base = np.concatenate([batch.bases, np.zeros(1, np.uint8)])
    pb = base.ctypes.data
    pk, ps, pe = (a.ctypes.data_as(u64p) for a in (km, st, en))
    evo = np.zeros(batch.n + 1, np.uint64)
    ks, ss, es = [], [], []
    for i in range(batch.n):
        n = o[i + 1] - o[i]
        c = L.kto_minimisers(C.cast(pb + o[i], u8p), n, w if w else n, m, pk, ps, pe) if n else 0
        evo[i + 1] = evo[i] + np.uint64(c)
        if c:
            ks.append(km[:c].copy())
            ss.append(st[:c].copy())
            es.append(en[:c].copy())
    cat = lambda parts: np.concatenate(parts) if parts else np.zeros(0, np.uint64)   # noqa: E731
    return evo, cat(ks), cat(ss), cat(es)


# ---- a brute force that shares nothing with the oracle ---------------------------------------------------------------------------

_CODE = {}
for _letters, _v in ((b"Aa", 0), (b"Cc", 1), (b"Gg", 2), (b"TtUu", 3)):
    for _x in _letters:
        _CODE[_x] = _v
for _v in range(4):
    _CODE[_v] = _v


def brute_kmers(seq, k):
    """every window of k bytes of one read: skipped when it holds a byte that is no nucleotide, else (forward value - the
    first base in the highest two bits -, value of the reverse complement, index of the window's last byte)"""
    out = []
    for s in range(len(seq) - k + 1):
        w = seq[s:s + k]
        if any(b not in _CODE for b in w):
            continue
        f = r = 0
        for b in w:
            f = (f << 2) | _CODE[b]
        for b in reversed(w):
            r = (r << 2) | (3 - _CODE[b])
        out.append((f, r, s + k - 1))
    return out


def brute_table(seqs, k):
    """{min(forward, reverse complement): occurrences} over all reads"""
    table = {}
    for s in seqs:
        for f, r, _ in brute_kmers(s, k):
            table[min(f, r)] = table.get(min(f, r), 0) + 1
    return table


def brute_oligo_rows(seqs, k, count_min):
    """per read the counts of its k-mers: a row of 4^k forward values, or of the canonical k-mers in ascending order"""
    if count_min:
        canon = sorted({min(f, r) for f in range(4 ** k) for r in [sum((3 - ((f >> (2 * j)) & 3)) << (2 * (k - 1 - j)) for j in range(k))]})
        rank = {c: i for i, c in enumerate(canon)}
    rows = np.zeros((len(seqs), len(canon) if count_min else 4 ** k), np.float64)
    for i, s in enumerate(seqs):
        for f, r, _ in brute_kmers(s, k):
            rows[i, rank[min(f, r)] if count_min else f] += 1
    return rows
