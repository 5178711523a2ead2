"""Batches of more than 2^32 bases for tests/test_big_batches.py, as plain helpers (no test in here): the plan of such a
batch - its offsets and where its pieces lie, never its bases -, the checks that say from the plan alone that the batch has
the shape it is meant to have, the assembly of the bases on the GPU, and the expected answers put together from the
oracle's answers for the small pieces.

A batch is  head | ballast | tail:
  head     probe A, a few hundred rb.noisy_reads (empty reads, reads shorter than k, N runs, a 9000-base read);
  ballast  `copies` copies of one block of BLOCK = 1 000 003 bases (a prime: every copy sits at another phase of the 16-,
           1008- and 8192-base lattices), each copy one read - equal-length reads;
  tail     probe B, another noisy_reads batch of about 2 Mbases (`straddle`: 4294 copies end 954 414 bases short of 2^32, so
           that index 2^32 falls inside a read of B), the same behind one filler read sized so that a read of B starts at
           2^32 (`aligned`), or a short B behind 4295 copies (`inside_ballast`: 2^32 falls inside a 1 Mbase read).

What is expected of a call on such a batch is what the oracle says of head, block and tail alone (three small batches):
per-read rows are the head's rows, the block's row `copies` times, the tail's rows; per-base arrays are the head's, the
block's `copies` times, the tail's; tables are the sums of the three tables, the block's counts `copies` times."""
import numpy as np

import read_batches as rb

G32 = 1 << 32
BLOCK = 1_000_003
COPIES = {"straddle": 4294, "aligned": 4294, "inside_ballast": 4295}
LAYOUTS = tuple(COPIES)
SEED = 0xb16ba7c4
A_READS, B_READS, SHORT_B_READS = 300, 10000, 300
CLEAN = (400_000, 430_000)        # the block's stretch without an invalid byte: windows of 5000 bases fill there
MIN_READ = 64                     # the read that holds base 2^32 has at least that many bases
MIN_DIFF_LEN = 16                 # reads of at least that many bases must differ from the bytes 2^32 before them
U64 = np.uint64

_memo = {}


def memo(key, fn):
    if key not in _memo:
        _memo[key] = fn()
    return _memo[key]


# ---- the pieces ---------------------------------------------------------------------------------------------------------------

def _letters_only(bases):
    """every byte that kt_cgr_points refuses replaced by a letter (a function of the byte and its position)"""
    bases = bases.copy()
    bad = np.flatnonzero(~np.isin(bases, rb.LETTERS))
    bases[bad] = rb.LETTERS[(bases[bad].astype(np.int64) + bad) % len(rb.LETTERS)]
    return bases


def _of_seqs(name, seqs, letters):
    bases = np.frombuffer(b"".join(seqs), np.uint8).copy()
    return rb.Batch.of_lens(name, _letters_only(bases) if letters else bases, [len(s) for s in seqs])


def probe(which, letters=False):
    """"A", "B" or "short_B": different rb.noisy_reads batches; letters: the same with letters only (rb.LETTERS)"""
    seed, n = {"A": (SEED + 1, A_READS), "B": (SEED + 2, B_READS), "short_B": (SEED + 3, SHORT_B_READS)}[which]
    return memo(("probe", which, letters), lambda: _of_seqs("probe %s%s" % (which, ", letters" if letters else ""),
                                                             rb.noisy_reads(seed, n), letters))


def block(letters=False):
    """one read of BLOCK bases: random ACGT with a few N, lower case, U, raw codes and IUPAC letters (rb._sprinkle), none of
    the invalid ones inside CLEAN"""
    def make():
        rng = np.random.default_rng(SEED)
        plain = rb._random_bases(rng, BLOCK, False)
        bases = rb._sprinkle(rng, plain.copy())
        lo, hi = CLEAN
        bad = np.flatnonzero(~np.isin(bases[lo:hi], rb.VALID)) + lo
        bases[bad] = plain[bad]
        return rb.Batch.of_lens("block%s" % (", letters" if letters else ""), _letters_only(bases) if letters else bases, [BLOCK])
    return memo(("block", letters), make)


def _tail(layout, head_total, letters):
    if layout == "inside_ballast":
        return probe("short_B", letters), 0
    b = probe("B", letters)
    if layout == "straddle":
        return b, 0
    # aligned: one filler read in front of B such that the last read of B with at least MIN_READ bases that can start at
    # 2^32 does
    gap = G32 - head_total - COPIES[layout] * BLOCK
    o, lens = b.offsets.astype(np.int64), b.lens
    j = max(i for i in range(b.n) if o[i] + 1 <= gap and lens[i] >= MIN_READ)
    fill = gap - int(o[j])
    rng = np.random.default_rng(SEED + 4)
    filler = (rb.LETTERS if letters else rb.ACGT)[rng.integers(0, 4, size=fill)]
    return rb.Batch.of_lens("filler of %d + %s" % (fill, b.name), np.concatenate([filler, b.bases]),
                            np.concatenate([[fill], lens])), 1


class Plan:
    """where everything lies in a batch of the given layout: offsets (u64, n + 1) and the pieces; no bases"""

    def __init__(self, layout, letters=False):
        self.layout, self.letters, self.copies = layout, letters, COPIES[layout]
        self.head, self.block = probe("A", letters), block(letters)
        self.tail, self.n_filler = _tail(layout, self.head.total, letters)
        self.n_head, self.n_tail = self.head.n, self.tail.n
        self.n = self.n_head + self.copies + self.n_tail
        self.o_ball = self.head.total
        self.o_tail = self.o_ball + self.copies * BLOCK
        self.total = self.o_tail + self.tail.total
        self.first_b = self.n_head + self.copies + self.n_filler          # the first read of B
        self.offsets = np.concatenate([self.head.offsets[:-1].astype(np.int64),
                                       self.o_ball + BLOCK * np.arange(self.copies, dtype=np.int64),
                                       self.o_tail + self.tail.offsets.astype(np.int64)]).astype(U64)
        self.name = "%s%s: %d + %d x %d + %d bases, %d reads" % (layout, ", letters" if letters else "", self.o_ball, self.copies,
                                                               BLOCK, self.tail.total, self.n)

    def read_of(self, g):
        """the read that holds base g (the last one that starts at or before it)"""
        return int(np.searchsorted(self.offsets, U64(g), side="right") - 1)

    def bytes(self, lo, hi):
        """the bases [lo, hi) of the batch, from the pieces"""
        g = np.arange(lo, hi, dtype=np.int64)
        out = np.empty(len(g), np.uint8)
        h, b, t = g < self.o_ball, (g >= self.o_ball) & (g < self.o_tail), g >= self.o_tail
        out[h] = self.head.bases[g[h]]
        out[b] = self.block.bases[(g[b] - self.o_ball) % BLOCK]
        out[t] = self.tail.bases[g[t] - self.o_tail]
        return out


def plan(layout, letters=False):
    return memo(("plan", layout, letters), lambda: Plan(layout, letters))


def check_plan(p):
    """from the offsets and the pieces alone: the batch crosses 2^32 where its layout says, and no read that touches a base
    index >= 2^32 holds what lies 2^32 bases before it.  -> the numbers, for the record"""
    o = p.offsets.astype(np.int64)
    assert len(o) == p.n + 1 and o[0] == 0 and (np.diff(o) >= 0).all() and int(o[-1]) == p.total, p.name
    assert p.total > G32 and p.o_ball < BLOCK and p.n < 16000, p.name
    assert np.array_equal(o[p.n_head:p.n_head + p.copies + 1] - p.o_ball, BLOCK * np.arange(p.copies + 1)), p.name
    lens = np.diff(o)
    i = p.read_of(G32)
    assert o[i] <= G32 < o[i + 1] and lens[i] >= MIN_READ, (p.name, i, lens[i])
    before, after = int((o[p.first_b + 1:] <= G32).sum()), int((o[p.first_b:-1] >= G32).sum())   # reads of B wholly on a side
    if p.layout == "inside_ballast":
        assert p.n_head <= i < p.n_head + p.copies and min(G32 - o[i], o[i + 1] - G32) >= MIN_READ, (p.name, i)
        assert after == p.n_tail, p.name
    else:
        assert i >= p.first_b and before >= 1000 and after >= 1000, (p.name, i, before, after)
        if p.layout == "straddle":
            assert o[i] < G32 and p.n_filler == 0, (p.name, i)
        else:
            assert o[i] == G32 and p.n_filler == 1 and (o == G32).sum() >= 1, (p.name, i)
    # what a kernel that dropped bit 32 of a base index would read instead: never the same
    hi = p.bytes(int(o[i]), p.total)
    lo = p.bytes(int(o[i]) - G32 if o[i] >= G32 else 0, p.total - G32)
    lo = np.concatenate([np.full(len(hi) - len(lo), 0xFF, np.uint8), lo])     # (the containing read's bases below 2^32: no alias)
    differs = hi != lo
    assert differs[max(G32 - int(o[i]), 0):].mean() > 0.7, p.name
    c = np.concatenate(([0], np.cumsum(differs)))
    s, e = o[i:-1] - o[i], o[i + 1:] - o[i]
    s = np.maximum(s, G32 - o[i])                                             # the part of each read at or past 2^32
    long_enough = e - s >= MIN_DIFF_LEN
    frac = (c[e] - c[s])[long_enough] / (e - s)[long_enough]
    assert long_enough.sum() >= (2 if p.layout == "inside_ballast" else 1000) and frac.min() > 0.25, (p.name, frac.min())
    return {"total": p.total, "read_at_2_32": i, "its_length": int(lens[i]), "b_reads_before": before, "b_reads_after": after}


# ---- the batch on the GPU -----------------------------------------------------------------------------------------------------

def assemble(torch, p):
    """-> (bases u8[total], offsets i64[n + 1]) on the device: the two probes and the block uploaded, the copies made there"""
    bases = torch.empty(p.total, dtype=torch.uint8, device="cuda")
    bases[:p.o_ball].copy_(torch.from_numpy(p.head.bases))
    bases[p.o_ball:p.o_tail].view(p.copies, BLOCK).copy_(torch.from_numpy(p.block.bases).cuda())
    bases[p.o_tail:].copy_(torch.from_numpy(p.tail.bases))
    offsets = torch.from_numpy(p.offsets.astype(np.int64)).cuda()
    torch.cuda.synchronize()
    return bases, offsets


# ---- expected answers from the pieces --------------------------------------------------------------------------------------------

def pieces(p):
    """the three small batches, in batch order"""
    return p.head, p.block, p.tail


def merged_table(p, table_of):
    """table_of(piece) -> (keys, counts): the table of the whole batch, keys ascending, counts as u64 (the block's `copies`
    times)"""
    ks, cs = [], []
    for piece, times in zip(pieces(p), (1, p.copies, 1)):
        k, c = table_of(piece)
        ks.append(np.asarray(k, U64))
        cs.append(np.asarray(c).astype(U64) * U64(times))
    keys, inv = np.unique(np.concatenate(ks), return_inverse=True)
    counts = np.zeros(len(keys), U64)
    np.add.at(counts, inv, np.concatenate(cs))
    return keys, counts
