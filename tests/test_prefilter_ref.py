"""tests/prefilter_ref.py on the CPU: the hash pinned to splitmix64's published outputs, the numpy model pinned to a
brute force over Python integers on inputs of a few dozen k-mers taken from strings, and the conditions the GPU tests
(tests/test_prefilter.py) rely on - per batch, a case whose E (the k-mers seen once that may reach the table) is at most a
quarter of the k-mers seen once, and at least one case whose E is not empty, so that the false-positive path runs."""
import collections

import numpy as np
import pytest

import card_ref
import prefilter_ref as ref
from read_batches import brute_kmers


def test_mix64_is_splitmix64():
    # the first three outputs of splitmix64 from state 0 (Steele, Lea, Flood 2014; the reference implementation's test vector):
    # output i is the finaliser of i + 1 times the golden gamma, which is what mix64 adds before it mixes
    gamma = 0x9E3779B97F4A7C15
    want = [0xE220A8397B1DCDAF, 0x6E789E6AA1B965F4, 0x06C45D188009454F]
    got = [card_ref.mix64_int((i * gamma) & card_ref.MASK) for i in range(3)]
    assert got == want
    assert ref.mix64(np.array([(i * gamma) & card_ref.MASK for i in range(3)], np.uint64)).tolist() == want


def test_pattern_and_word_by_hand():
    # h = bit fields 5, 63, 5, 0 (from the low end) under a top word of all ones
    h = 5 | (63 << 6) | (5 << 12) | (0 << 18) | (0xFFFFF << 44)
    assert int(ref.pattern_of(np.array([h], np.uint64))[0]) == (1 << 5) | (1 << 63) | (1 << 0)
    assert int(ref.pattern_of(np.array([0], np.uint64))[0]) == 1
    z = card_ref.unmix64(h)                       # the k-mer ^ seed whose hash is h
    w, p, hh = ref.once_of(np.array([z ^ ref.SEED], np.uint64), 10)
    assert int(hh[0]) == h and int(w[0]) == 1023 and int(p[0]) == (1 << 5) | (1 << 63) | 1
    w, _, _ = ref.once_of(np.array([z ^ ref.SEED], np.uint64), 34)
    assert int(w[0]) == h >> 30


def _string_counts(seqs, k):
    c = collections.Counter()
    for s in seqs:
        for f, r, _ in brute_kmers(s, k):
            c[min(f, r)] += 1
    return dict(c)


@pytest.mark.parametrize("k, a, b, seed", [(5, 10, 10, 1), (15, 10, 10, 2), (31, 11, 10, 3)])
def test_model_against_brute_force(k, a, b, seed):
    """a few dozen k-mers - and, so that words are shared and U differs from L, the same with every word index folded onto
    four words: the model on hashes whose top bits are forced"""
    rng = np.random.default_rng(seed)
    seqs = [ref.ACGT[rng.integers(0, 4, size=L)].tobytes() for L in (k + 20, k + 9, k - 1, 0, k + 14)]
    seqs += [seqs[0][3:k + 8], seqs[1]]
    seqs[0] = seqs[0][:7] + b"N" + seqs[0][8:]
    counts = _string_counts(seqs, k)
    assert 24 <= len(counts) <= 96 and 1 in counts.values() and max(counts.values()) >= 2
    keys = np.array(sorted(counts), np.uint64)
    m = ref.Model(keys, np.array([counts[int(x)] for x in keys]), a, b)
    once, L, U, E = ref.brute(counts, a, b)
    assert m.once.tolist() == once and m.L.tolist() == L and m.U.tolist() == U and set(m.E.tolist()) == E
    q0, q1lo, q1hi = m.query(keys)
    assert q0.all() and q1lo[m.counts >= 2].all() and (q1hi | ~q1lo).all()


def test_model_against_brute_force_on_crowded_words():
    """k-mers chosen by their hashes, so that four words of `once` take all of them and some k-mers seen once are covered by
    the others: U grows beyond L and E is not empty"""
    rng = np.random.default_rng(9)
    counts = {}
    while len(counts) < 80:
        h = (int(rng.integers(0, 4)) << 54) | int(rng.integers(0, 1 << 24))
        h |= int(rng.integers(0, 1 << 30)) << 24                       # (bits the pattern and a = 10 do not look at)
        counts[card_ref.unmix64(h) ^ ref.SEED] = 1 if len(counts) % 3 else 2
    keys = np.array(sorted(counts), np.uint64)
    m = ref.Model(keys, np.array([counts[int(x)] for x in keys]), 10, 10)
    once, L, U, E = ref.brute(counts, 10, 10)
    assert m.once.tolist() == once and m.L.tolist() == L and m.U.tolist() == U and set(m.E.tolist()) == E
    assert np.count_nonzero(m.once) <= 4 and m.may_promote.any() and U != L and E


def test_gpu_inputs_meet_their_conditions(oracle):
    per_batch, nonempty = collections.defaultdict(list), 0
    for name, k, a, b in ref.CASES:
        m = ref.model(oracle, name, k, a, b)
        singles = int(m.single.sum())
        print("%-7s k=%-2d a=%-2d b=%-2d distinct %7d seen once %7d E %7d" % (name, k, a, b, len(m.keys), singles, len(m.E)))
        if (name, k, a, b) in ref.SELECTIVE:
            assert 4 * len(m.E) <= singles, (name, k, a, b, len(m.E), singles)
            per_batch[name].append((k, a, b))
            nonempty += len(m.E) > 0
        assert ref.popcount(m.L) <= ref.popcount(m.U) and m.min_promotions <= int((m.counts >= 2).sum())
    assert set(per_batch) == {c[0] for c in ref.CASES}      # every batch has such a case
    assert nonempty >= 1
    # the batches are what they are said to be
    assert ref.model(oracle, "noisy", 31, 14, 12).single.sum() > 50000
    assert not ref.model(oracle, "twins", 31, 10, 10).single.any() and not ref.model(oracle, "apart", 31, 12, 10).single.any()
    k5, c5 = ref.table_of(oracle, "fives1", 5)
    assert len(k5) == 512 and (c5 == 1).all() and (ref.table_of(oracle, "fives2", 5)[1] == 2).all()
    kh, ch = ref.table_of(oracle, "homo", 31)
    assert len(kh) == 1 and int(kh[0]) == 0 and int(ch[0]) == 67 * 120 + 100000 - 30 + 1
    apart = ref.batch("apart")
    assert int(apart.offsets[apart.n // 2]) > 8192 + 150
