"""The oracle against a brute force that shares no code with it: every window of every read sliced in Python, skipped when
it holds a byte that is no nucleotide, min(forward, reverse complement) taken - so that the oracle and the kernels cannot
share one misreading of "a k-mer may not span a read start".  3000 reads of family A (tests/read_batches.py: reads of
0..8, 0..2k and 12..34 bases with N, lower case, U, raw codes and IUPAC letters), k = 3, 5, 7: the k-mers of every read,
the oligo rows (raw and canonical) and the count table.  Then the content families of tests/test_read_content.py - every
byte value at every position of an item, alone and with a raw code behind it, and reads of the 14 valid bytes - at
k = 4, 16, 17, 31 on every 37th read and the reads of the bytes that are most like a nucleotide: what entitles the GPU
tests to take the oracle as their reference for bytes that no fixture of the reference holds.  At the end: the comparisons
the GPU tests report with (first_flat_diff, first_row_diff, table_diff) on doctored arrays - one bit, one ulp, one element
or key missing or added."""
import numpy as np
import pytest

import read_batches as rb


@pytest.fixture(scope="module")
def sample():
    out = {}
    for k in (3, 5, 7):
        b = rb.tiny_batch(0xb0a7 + k, k, 4000)
        pick = np.sort(np.random.default_rng(k).choice(b.n, size=3000, replace=False))
        out[k] = rb.Batch("%s[3000 of them]" % b.name, [b.seqs[i] for i in pick])
        lens = out[k].lens
        assert (lens == 0).sum() > 100 and (lens < k).sum() > 500 and (lens >= k).sum() > 500
    return out


@pytest.mark.parametrize("k", [3, 5, 7])
def test_oracle_kmers_equal_the_brute_force(oracle, sample, k):
    b = sample[k]
    some = 0
    for i, s in enumerate(b.seqs):
        f, r, e = oracle.kmers(s, k)
        want = rb.brute_kmers(s, k)
        assert list(zip(f.tolist(), r.tolist(), e.tolist())) == want, (k, rb.where(b, i), s)
        some += len(want)
    wf, wr, we = rb.oracle_kmers_flat(oracle, b, k)          # the flat form the GPU tests compare against
    flat = [(f, r, e + int(o)) for s, o in zip(b.seqs, b.offsets[:-1]) for f, r, e in rb.brute_kmers(s, k)]
    assert some > 5000 and list(zip(wf.tolist(), wr.tolist(), we.tolist())) == flat


@pytest.mark.parametrize("count_min", [True, False])
@pytest.mark.parametrize("k", [3, 5, 7])
def test_oracle_oligo_rows_equal_the_brute_force(oracle, sample, k, count_min):
    b = sample[k]
    got = oracle.oligo_batch(b.bases, b.offsets, k, count_min, False, 1.0)
    want = rb.brute_oligo_rows(b.seqs, k, count_min)
    assert got.shape == want.shape
    bad = np.flatnonzero((got != want).any(axis=1))
    assert not len(bad), (k, count_min, rb.where(b, bad[0]), b.seqs[bad[0]])
    norm = oracle.oligo_batch(b.bases, b.offsets, k, count_min, True, 1.0)
    assert np.array_equal(norm, want / np.maximum(1.0, want.sum(axis=1, keepdims=True)))


@pytest.mark.parametrize("k", [3, 5, 7])
def test_oracle_count_table_equals_the_brute_force(oracle, sample, k):
    b = sample[k]
    keys, counts = oracle.count_reads(b.bases, b.offsets, k)
    want = rb.brute_table(b.seqs, k)
    assert dict(zip(keys.tolist(), counts.tolist())) == want and len(keys) == len(want)


# ---- the content families: every byte value, with and without a raw code next to it -----------------------------------------

# the bytes one bit, a case fold or a sign away from a nucleotide, the raw codes, load_guarded's 0xFF
NEAR_NUCLEOTIDES = sorted({0, 1, 2, 3, 4, 0x14, 0x21, 0x40, 0x60, 0x7B, 0x80, 0x83, 0xFF} | set(b"ACGTUacgtuBEFVWNnRSsdw")
                          | {x | 0x80 for x in b"ACGTUacgtu"})
CONTENT = ("alphabet", "alphabet_ragged", "alphabet_raw", "alphabet_raw_ragged", "valid_mix")


@pytest.fixture(scope="module")
def content_sample():
    out = {}
    for j, name in enumerate(CONTENT):
        if name == "valid_mix":
            b = rb.valid_mix_batch(0xb17e, 1400)
            rb.check_valid_mix(b)
            pick = list(range(j, b.n, 37))
        else:
            raw = "raw" in name
            b = rb.alphabet_batch(0xb17e + j, raw_neighbour=raw, ragged="ragged" in name)
            assert rb.check_alphabet(b, raw) >= 256 * 32
            pick = sorted(set(range(j, b.n, 37)) | set(NEAR_NUCLEOTIDES))
        out[name] = rb.Batch("%s[%d of them]" % (b.name, len(pick)), [b.seqs[i] for i in pick])
        out[name].meta["picked"] = pick
    return out


@pytest.mark.parametrize("k", [4, 16, 17, 31])
@pytest.mark.parametrize("name", CONTENT)
def test_oracle_equals_the_brute_force_on_every_byte_value(oracle, content_sample, name, k):
    b = content_sample[name]
    flat = []
    for i, (s, o) in enumerate(zip(b.seqs, b.offsets[:-1])):
        f, r, e = oracle.kmers(s, k)
        want = rb.brute_kmers(s, k)
        assert list(zip(f.tolist(), r.tolist(), e.tolist())) == want, (name, k, "read %d" % b.meta["picked"][i], rb.where(b, i))
        flat += [(f_, r_, e_ + int(o)) for f_, r_, e_ in want]
    if name != "valid_mix":                                   # 32 occurrences of an invalid byte leave 33 stretches of 32 bases
        assert len(flat) > 33 * max(0, 33 - k) * 20
    else:
        assert len(flat) == int(np.maximum(b.lens - k + 1, 0).sum()) > 1000      # every window is a k-mer
    wf, wr, we = rb.oracle_kmers_flat(oracle, b, k)
    assert list(zip(wf.tolist(), wr.tolist(), we.tolist())) == flat
    keys, counts = oracle.count_reads(b.bases, b.offsets, k)
    table = rb.brute_table(b.seqs, k)
    assert dict(zip(keys.tolist(), counts.tolist())) == table and len(keys) == len(table)


def test_alphabet_check_notices_a_missing_pair():
    """check_alphabet on doctored batches: one occurrence replaced, its neighbourhood spoiled, its raw code taken away"""
    for raw in (False, True):
        b = rb.alphabet_batch(5, raw_neighbour=raw)
        assert rb.check_alphabet(b, raw) >= 256 * 32
        v, i = 0x56, 7
        p = v * rb.ALPHA_LEN + rb.ALPHA_FIRST + rb.ALPHA_STEP * i
        assert b.bases[p] == v
        spoil = ((p + 1 + (v + i) % 15, ord("C")),) if raw else ((p - 32, 2), (p + 32, 1))
        for at, byte in ((p, ord("A")), (p - 31, ord("N")), (p + 31, ord("N"))) + spoil:
            doctored = rb.Batch.of_lens(b.name, b.bases.copy(), b.lens)
            doctored.bases[at] = byte
            with pytest.raises(AssertionError):
                rb.check_alphabet(doctored, raw)
    b = rb.alphabet_batch(5, ragged=True, values=rb.LETTERS)
    assert b.n == 10 and len(set(b.lens)) > 1 and np.isin(b.bases, rb.LETTERS).all()
    assert rb.check_alphabet(b, False, rb.LETTERS) >= 10 * 32
    with pytest.raises(AssertionError):
        rb.check_alphabet(b, False)


# ---- the comparisons of tests/test_read_boundaries.py notice a doctored answer and say where -------------------------------

def test_flat_and_row_comparisons_find_the_first_difference():
    from test_read_boundaries import first_flat_diff, first_row_diff
    a = (np.arange(10, dtype=np.uint64), np.arange(10, dtype=np.uint64) * 3)
    assert first_flat_diff(a, (a[0].copy(), a[1].copy())) is None
    b = (a[0].copy(), a[1].copy())
    b[1][7] ^= np.uint64(1)                                  # one bit of one element of the second array
    assert first_flat_diff(a, b) == 7 and first_flat_diff(b, a) == 7
    assert first_flat_diff((a[0][:9], a[1][:9]), a) == 9     # one element missing at the end
    assert first_flat_diff(a, (a[0][:4], a[1][:4])) == 4
    empty = (a[0][:0], a[1][:0])
    assert first_flat_diff(empty, empty) is None and first_flat_diff(empty, a) == 0
    rows = np.arange(12.0).reshape(4, 3)
    other = rows.copy()
    assert first_row_diff(rows.view(np.uint64), other.view(np.uint64)) is None
    other[2, 1] = np.nextafter(other[2, 1], 100.0)           # one ulp
    assert first_row_diff(rows.view(np.uint64), other.view(np.uint64)) == 2
    assert first_row_diff(np.arange(5), np.array([0, 1, 2, 9, 9])) == 3


@pytest.mark.parametrize("k", [3, 7])
def test_table_comparison_names_the_read(oracle, sample, k):
    from test_read_boundaries import table_diff
    b = sample[k]
    wk, wc = oracle.count_reads(b.bases, b.offsets, k)
    assert table_diff(oracle, b, k, wk.copy(), wc.copy(), wk, wc) is None
    assert table_diff(oracle, b, k, wk.copy(), 2 * wc, wk, wc, times=2) is None
    assert table_diff(oracle, b, k, wk.copy(), wc.copy(), wk, wc, times=2) is not None
    f, r, e = rb.oracle_kmers_flat(oracle, b, k)
    j = len(f) // 2
    key, i = min(int(f[j]), int(r[j])), rb.read_of(b, int(e[j]))
    first = int(e[np.flatnonzero(np.minimum(f, r) == np.uint64(key))[0]])     # the first k-mer with that key, in batch order
    at = int(np.searchsorted(wk, np.uint64(key)))
    gc = wc.copy()
    gc[at] += 1                                              # one count off by one
    msg = table_diff(oracle, b, k, wk.copy(), gc, wk, wc)
    assert msg and "%#x" % key in msg and "ends at base %d" % first in msg and rb.where(b, rb.read_of(b, first)) in msg, (msg, i)
    msg = table_diff(oracle, b, k, np.delete(wk, at), np.delete(wc, at), wk, wc)       # one key missing
    assert msg and "%#x" % key in msg and "count 0" in msg, msg
    ghost = np.uint64(4 ** k - 1 if np.uint64(4 ** k - 1) not in wk else 4 ** k)      # (k = 3 holds every canonical 3-mer)
    gk = np.sort(np.append(wk, ghost))
    msg = table_diff(oracle, b, k, gk, np.insert(wc, int(np.searchsorted(wk, ghost)), 1), wk, wc)
    assert msg and "no read holds" in msg and "%#x" % int(ghost) in msg, msg
