"""Scaled (FracMinHash) sketches: kt_scaled_batch (every distinct hash of a read at or below the threshold, with its
abundance), kt_scaled_merge (unions, abundances summed and saturating), kt_ctr_scaled (the sketch of a table's entries in a
count range, in every form a table can be in) and kt_scaled_pairs (the shared hashes of every pair of rows) against the
numpy restatement of tests/scaled_ref.py over the oracle's k-mers: the threshold's two sides, ragged batches over the segment
edges, repeats, the sort's tile and digit-pass edges, merges, the four table forms, rows shorter and longer than what LDS
holds, the size conventions, views and fences, argument errors; and `kmertools sketch --scaled` end to end against files
restated from the parsed records.  Everything is integers and compared exactly; the floats of sketch.contain within 1e-12."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ktab_ref  # noqa: E402
import read_batches as rb  # noqa: E402
import scaled_ref as sr  # noqa: E402
import table_model as tm  # noqa: E402
import test_sketch as ts  # noqa: E402
import test_table_forms as tf  # noqa: E402
import test_table_lifecycle as tl  # noqa: E402
from test_buffer_views import Fenced, HostFenced, bases_view, host_bases_view, noisy_reads, offsets_view  # noqa: E402

pytestmark = pytest.mark.gpu

U = np.uint64
ACGT = np.frombuffer(b"ACGT", np.uint8)
HPAT, APAT, OPAT = 0x5A5A5A5A5A5A5A5A, 0x6B6B6B6B, 0x7C7C7C7C7C7C7C7C
SAT = 0xFFFFFFFF


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    return torch


@pytest.fixture(scope="module")
def ctx(torch_mod):
    from kmertools_amd import device
    c = device.Context(0, stream=torch_mod.cuda.current_stream().cuda_stream)
    yield c
    c.close()


_MEMO = {}


def hashes_of(oracle, batch_key, bases, offsets, k, seed):
    """the windows' hashes of every read, computed once per (batch, k, seed) and shared"""
    key = (batch_key, k, seed)
    if key not in _MEMO:
        _MEMO[key] = sr.read_hashes(oracle, bases, offsets, k, seed)
    return _MEMO[key]


def dev(torch, a):
    a = np.ascontiguousarray(a)
    a = a.view({np.dtype(np.uint64): np.int64, np.dtype(np.uint32): np.int32}.get(a.dtype, a.dtype))
    return torch.from_numpy(a if a.size else np.zeros(1, a.dtype)).cuda()


def dev_batch(torch, ctx, bases, offsets, k, scaled, seed):
    """kt_scaled_batch in device mode: a count-only call, then one into prefilled arrays of exactly that size + a guard"""
    n = len(offsets) - 1
    d_b, d_o = dev(torch, bases), dev(torch, offsets)
    ro0 = torch.full((n + 1,), OPAT, dtype=torch.int64, device="cuda")
    n_out = ctx.scaled_sketch(d_b, d_o, n, k, scaled, None, None, 0, ro0, None, seed)
    h = torch.full((n_out + 3,), HPAT, dtype=torch.int64, device="cuda")
    a = torch.full((n_out + 3,), APAT, dtype=torch.int32, device="cuda")
    ro = torch.full((n + 1,), OPAT, dtype=torch.int64, device="cuda")
    nk = torch.full((n,), APAT, dtype=torch.int32, device="cuda")
    got = ctx.scaled_sketch(d_b, d_o, n, k, scaled, h, a, max(n_out, 1), ro, nk, seed)
    torch.cuda.synchronize()
    assert got == n_out
    hh, aa = tl.u64(h), tl.u32(a)
    assert (hh[n_out:] == HPAT).all() and (aa[n_out:] == APAT).all(), "written behind the result"
    assert tl.same(tl.u64(ro0), tl.u64(ro)), "the count-only call's row_offsets differ"
    return hh[:n_out], aa[:n_out], tl.u64(ro), tl.u32(nk)


def check_batch(torch, ctx, rows, bases, offsets, k, scaled, seed, mode, tag=""):
    wh, wa, wo, wn = sr.csr(rows)
    if mode == "host":
        gh, ga, go, gn = ctx.scaled_sketch_host(bases, offsets, k, scaled, seed)
    else:
        gh, ga, go, gn = dev_batch(torch, ctx, bases, offsets, k, scaled, seed)
    assert tl.same(go, wo), (tag, mode, "row_offsets", np.flatnonzero(go != wo)[:5])
    assert tl.same(gn, wn), (tag, mode, "n_kmers", np.flatnonzero(gn != wn)[:5])
    assert tl.same(gh, wh), (tag, mode, "hashes", len(gh), len(wh))
    assert tl.same(ga, wa), (tag, mode, "abunds", np.flatnonzero(ga != wa)[:5])
    return gh, ga, go, gn


def random_seq(rng, L):
    return ACGT[rng.integers(0, 4, size=L)].tobytes()


# ---- the boundary of the threshold ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("scaled", [2, 1000])
def test_threshold_is_inclusive(torch_mod, ctx, oracle, scaled):
    from kmertools_amd.device import to_csr
    k = 21
    rng = np.random.default_rng(scaled)
    seqs = [random_seq(rng, 60), random_seq(rng, k), b"", random_seq(rng, 300)]
    bases, offsets = to_csr(seqs)
    f, r, _ = oracle.kmers(seqs[1], k)
    x, mh = int(min(f[0], r[0])), sr.max_hash(scaled)
    for h, kept in ((mh, True), (mh + 1, False)):
        seed = sr.inv_mix64(h) ^ x
        assert sr.mix64_int(x ^ seed) == h
        rows = sr.read_rows(oracle, bases, offsets, k, scaled, seed)
        assert (len(rows[1][1]) == 1) == kept and (not kept or int(rows[1][1][0]) == mh)
        for mode in ("device", "host"):
            gh, ga, go, gn = check_batch(torch_mod, ctx, rows, bases, offsets, k, scaled, seed, mode)
            assert int(go[2] - go[1]) == (1 if kept else 0)
            assert (gh <= U(mh)).all()


def test_scaled_1_keeps_every_window_and_a_huge_scaled_none(torch_mod, ctx, oracle):
    from kmertools_amd.device import to_csr
    rng = np.random.default_rng(3)
    seqs = [random_seq(rng, 5000), random_seq(rng, 40), b"ACGTN" * 30]
    bases, offsets = to_csr(seqs)
    for k in (5, 21):
        hs = sr.read_hashes(oracle, bases, offsets, k, 9)
        for mode in ("device", "host"):
            gh, ga, go, gn = check_batch(torch_mod, ctx, sr.rows_of(hs, 1), bases, offsets, k, 1, 9, mode)
            for i in range(len(seqs)):
                assert int(ga[int(go[i]):int(go[i + 1])].astype(np.uint64).sum()) == int(gn[i])
            rows = sr.rows_of(hs, 1 << 62)
            assert all(len(h) == 0 for _, h, _ in rows)
            gh, ga, go, gn = check_batch(torch_mod, ctx, rows, bases, offsets, k, 1 << 62, 9, mode)
            assert len(gh) == 0 and not go.any()


# ---- read membership ----------------------------------------------------------------------------------------------------------

def membership_batches():
    rng = np.random.default_rng(77)
    spanning = [random_seq(rng, L) for L in (100, 15, 16, 17, 30_000, 40, 0, 0, 8192 * 2 + 5, 33)]
    return {"tiny": lambda k: rb.tiny_batch(5, k, 300),
            "empty_runs": lambda k: rb.empty_runs_batch(6),
            "lattice": lambda k: rb.lattice_batch(7, k, poly_a=True),
            "noisy": lambda k: rb.Batch("noisy", noisy_reads(8, 120) + spanning)}


@pytest.mark.parametrize("k", [1, 5, 16, 17, 21, 31])
@pytest.mark.parametrize("family", ["tiny", "empty_runs", "lattice", "noisy"])
def test_read_membership(torch_mod, ctx, oracle, family, k):
    b = membership_batches()[family](k)
    seed = 1000 + k
    hs = hashes_of(oracle, b.name, b.bases, b.offsets, k, seed)
    for i, scaled in enumerate((1, 3, 50)):
        mode = ("device", "host")[(i + k) % 2]
        check_batch(torch_mod, ctx, sr.rows_of(hs, scaled), b.bases, b.offsets, k, scaled, seed, mode, (family, k, scaled))


# ---- repeats -------------------------------------------------------------------------------------------------------------------

def test_repeats_have_their_multiplicities(torch_mod, ctx, oracle):
    from kmertools_amd.device import to_csr
    rng = np.random.default_rng(4)
    half = random_seq(rng, 40)
    rc = bytes(b"TGCA"[b"ACGT".index(c)] for c in reversed(half))
    seqs = [b"A" * 3000, b"ACG" * 6000, half + rc, b"A" * 20, b"AT" * 100, random_seq(rng, 200)]
    bases, offsets = to_csr(seqs)
    for k in (4, 21):
        hs = sr.read_hashes(oracle, bases, offsets, k, 0)
        rows = sr.rows_of(hs, 1)
        assert len(rows[0][1]) == 1 and int(rows[0][2][0]) == 3000 - k + 1  # poly-A: one k-mer, every window
        assert len(rows[1][1]) <= 3 and int(rows[1][2].sum()) == 18000 - k + 1
        # its own reverse complement: a window and its mirror image are one k-mer (the window on the centre, for an even k,
        # is its own mirror image)
        assert (rows[2][2] >= 2).sum() >= len(rows[2][2]) - 1 and int(rows[2][2].sum()) == 80 - k + 1
        for mode in ("device", "host"):
            for scaled in (1, 3):
                check_batch(torch_mod, ctx, sr.rows_of(hs, scaled), bases, offsets, k, scaled, 0, mode, (k, scaled))


# ---- the sort's paths --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kept", [1, 4095, 4096, 4097, 20_001])
@pytest.mark.parametrize("rows_", ["one row", "three rows"])
def test_kept_counts_around_the_sorts_tiles(torch_mod, ctx, oracle, kept, rows_):
    """scaled = 1 keeps every window: `kept` windows in all, in one read (the single-row form: no second sort) or in three"""
    from kmertools_amd.device import to_csr
    k = 21
    rng = np.random.default_rng(kept)
    if rows_ == "one row" or kept < 3:
        seqs = [random_seq(rng, kept + k - 1)]
    else:
        a, b = kept // 3, kept // 2
        seqs = [random_seq(rng, a + k - 1), random_seq(rng, b + k - 1), random_seq(rng, kept - a - b + k - 1)]
    bases, offsets = to_csr(seqs)
    hs = sr.read_hashes(oracle, bases, offsets, k, 1)
    assert sum(len(h) for h in hs) == kept
    for mode in ("device", "host"):
        check_batch(torch_mod, ctx, sr.rows_of(hs, 1), bases, offsets, k, 1, 1, mode)


@pytest.mark.parametrize("n", [1, 255, 256, 257, 1023, 1024, 1025, 262_143, 262_144, 262_145, 1_048_577 + 4096])
@pytest.mark.parametrize("rows_", ["one row, one group", "three rows, two groups"])
def test_merge_sizes_around_the_scans_tiles(torch_mod, ctx, n, rows_):
    """n distinct hashes with abundances through the merge (its sort and its scans), at the edges of the workgroup scan
    that the two share: the workgroup's 256 threads, the scan's tile of 1024 items, 256 such tiles - one more and the
    one-workgroup scan of the tiles' sums takes a second chunk - and more than 256 wave tiles of 4096 pairs, where the
    sort's scan of a digit's histogram row takes a second chunk"""
    rng = np.random.default_rng(n)
    h = np.unique(rng.integers(0, 1 << 63, size=n + 64, dtype=np.uint64))
    assert len(h) >= n
    h = rng.permutation(h)[:n]
    a = rng.integers(1, 1000, size=n).astype(np.uint32)
    if rows_ == "one row, one group":
        order = np.argsort(h)
        check_merge(torch_mod, ctx, h[order], a[order], np.array([0, n], U), [0, 1], (n, rows_))
    else:
        row = rng.integers(0, 3, size=n)
        order = np.lexsort((h, row))  # by row, ascending inside a row
        ro = np.concatenate([[0], np.cumsum(np.bincount(row, minlength=3))]).astype(U)
        check_merge(torch_mod, ctx, h[order], a[order], ro, [0, 2, 3], (n, rows_))


def test_more_rows_than_one_digit_pair_of_the_row_sort(torch_mod, ctx, oracle):
    """70 000 reads of k + 3 bases, scaled = 1: the row ids take 17 bits, so the stable sort by row makes four digit passes"""
    k, n, L = 5, 70_000, 8
    rng = np.random.default_rng(12)
    codes = rng.integers(0, 4, size=(n, L)).astype(np.uint64)
    codes[::1000] = 0  # poly-A reads: one hash of abundance 4
    bases = ACGT[codes.astype(np.int64)].reshape(-1)
    offsets = (np.arange(n + 1, dtype=np.uint64) * U(L))
    # the restatement, vectorised over the equal-length reads (checked against the oracle's on a sample below)
    w = L - k + 1
    f = np.zeros((n, w), np.uint64)
    r = np.zeros((n, w), np.uint64)
    for j in range(k):
        f = f * U(4) + codes[:, j:j + w]
        r = r + (U(3) - codes[:, j:j + w]) * U(4 ** j)
    with np.errstate(over="ignore"):
        h = sr.mix64(np.minimum(f, r) ^ U(2))
    h.sort(axis=1)
    rows = []
    for i in range(n):
        u, c = np.unique(h[i], return_counts=True)
        rows.append((w, u, c.astype(np.uint32)))
    sample = np.arange(0, n, 997)
    so = np.zeros(len(sample) + 1, np.uint64)
    so[1:] = np.cumsum(np.full(len(sample), L))
    sb = np.concatenate([bases[i * L:(i + 1) * L] for i in sample])
    for (w1, h1, a1), i in zip(sr.read_rows(oracle, sb, so, k, 1, 2), sample):
        assert w1 == w and tl.same(h1, rows[i][1]) and tl.same(a1, rows[i][2])
    gh, ga, go, gn = check_batch(torch_mod, ctx, rows, bases, offsets, k, 1, 2, "device")
    assert int(ga[int(go[1000]):int(go[1001])][0]) == 4
    check_batch(torch_mod, ctx, rows, bases, offsets, k, 1, 2, "host")


# ---- merge -----------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def merge_batch(oracle):
    rng = np.random.default_rng(21)
    genome = ACGT[rng.integers(0, 4, size=3000)]
    seqs = []
    for i in range(40):
        L = int(rng.integers(0, 400)) if i % 7 else 0
        a = int(rng.integers(0, len(genome) - L))
        seqs.append(genome[a:a + L].tobytes())
    from kmertools_amd.device import to_csr
    bases, offsets = to_csr(seqs)
    return seqs, bases, offsets


def dev_merge(torch, ctx, hashes, abunds, ro, go):
    d_h, d_a, d_r, d_g = dev(torch, hashes), None if abunds is None else dev(torch, abunds), dev(torch, ro), dev(torch, go)
    oo0 = torch.full((len(go),), OPAT, dtype=torch.int64, device="cuda")
    from kmertools_amd._lib import KT_MEM_DEVICE
    n_out = ctx.scaled_merge(d_h, d_a, d_r, d_g, None, None, 0, oo0, KT_MEM_DEVICE)
    oh = torch.full((n_out + 3,), HPAT, dtype=torch.int64, device="cuda")
    oa = torch.full((n_out + 3,), APAT, dtype=torch.int32, device="cuda")
    oo = torch.full((len(go),), OPAT, dtype=torch.int64, device="cuda")
    assert ctx.scaled_merge(d_h, d_a, d_r, d_g, oh, oa, max(n_out, 1), oo, KT_MEM_DEVICE) == n_out
    torch.cuda.synchronize()
    hh, aa = tl.u64(oh), tl.u32(oa)
    assert (hh[n_out:] == HPAT).all() and (aa[n_out:] == APAT).all() and tl.same(tl.u64(oo0), tl.u64(oo))
    return hh[:n_out], aa[:n_out], tl.u64(oo)


def check_merge(torch, ctx, hashes, abunds, ro, go, tag=""):
    go = np.asarray(go, np.uint64)
    wh, wa, wo = sr.merge(hashes, abunds, ro, go)
    for mode in ("host", "device"):
        if mode == "host":
            gh, ga, goo = ctx.scaled_merge(hashes, abunds, ro, go)
        else:
            gh, ga, goo = dev_merge(torch, ctx, hashes, abunds, ro, go)
        assert tl.same(goo, wo), (tag, mode, "offsets")
        assert tl.same(gh, wh), (tag, mode, "hashes")
        assert tl.same(ga, wa), (tag, mode, "abunds")
    return wh, wa, wo


@pytest.mark.parametrize("scaled", [1, 5])
def test_merge(torch_mod, ctx, oracle, merge_batch, scaled):
    from kmertools_amd.device import to_csr
    seqs, bases, offsets = merge_batch
    k, seed, n = 15, 3, len(seqs)
    h, a, ro, nk = sr.csr(sr.read_rows(oracle, bases, offsets, k, scaled, seed))
    # groups of 0, 1 and many rows; groups that leave rows out at both ends
    check_merge(torch_mod, ctx, h, a, ro, [0, 0, 1, 1, 8, 30, 30, n], "cover")
    check_merge(torch_mod, ctx, h, a, ro, [3, 4, 4, 20], "inner")
    check_merge(torch_mod, ctx, h, a, ro, [5, 5], "one empty group")
    check_merge(torch_mod, ctx, h, None, ro, [0, 2, 2, n], "abunds NULL")
    # the union of a batch's rows = the sketch of the reads taken as one read's windows, abundances summed
    uh, ua, uo = check_merge(torch_mod, ctx, h, a, ro, [0, n], "all")
    hs = sr.read_hashes(oracle, bases, offsets, k, seed)
    (_, wh, wa), = sr.rows_of([np.concatenate(hs)], scaled)
    assert tl.same(uh, wh) and tl.same(ua, wa)
    # a batch in two calls, merged pairwise, is the whole batch
    cut = 17
    b1, o1 = to_csr(seqs[:cut])
    b2, o2 = to_csr(seqs[cut:])
    h1, a1, r1, _ = ctx.scaled_sketch_host(b1, o1, k, scaled, seed)
    h2, a2, r2, _ = ctx.scaled_sketch_host(b2, o2, k, scaled, seed)
    assert tl.same(np.concatenate([h1, h2]), h) and tl.same(np.concatenate([r1, r2[1:] + r1[-1]]), ro)
    mh, ma, mo = ctx.scaled_merge(np.concatenate([uh, uh]), np.concatenate([ua, ua]), np.array([0, len(uh), 2 * len(uh)], U), [0, 2])
    assert tl.same(mh, uh) and tl.same(ma, np.minimum(ua.astype(U) * U(2), U(SAT)).astype(np.uint32))
    m1 = sr.merge(h1, a1, r1, [0, cut])
    m2 = sr.merge(h2, a2, r2, [0, n - cut])
    both_h, both_a = np.concatenate([m1[0], m2[0]]), np.concatenate([m1[1], m2[1]])
    gh, ga, go = ctx.scaled_merge(both_h, both_a, np.array([0, len(m1[0]), len(both_h)], U), [0, 2])
    assert tl.same(gh, uh) and tl.same(ga, ua)


def test_merge_saturates(torch_mod, ctx):
    h = np.array([3, 9, 11, 3, 9, 11, 12, 11], np.uint64)
    a = np.array([SAT, 0x80000000, 7, 1, 0x80000000, SAT - 7, 5, 1], np.uint32)
    ro = np.array([0, 3, 7, 8], U)
    wh, wa, wo = check_merge(torch_mod, ctx, h, a, ro, [0, 3])
    assert wh.tolist() == [3, 9, 11, 12] and wa.tolist() == [SAT, SAT, SAT, 5]
    wh, wa, wo = check_merge(torch_mod, ctx, h, a, ro, [0, 1, 3])
    assert wa.tolist() == [SAT, 0x80000000, 7, 1, 0x80000000, SAT - 6, 5]


@pytest.mark.parametrize("groups", [[0, 2, 1], [1, 0], [0, 4], [5, 5]])
def test_merge_rejects_bad_group_offsets(torch_mod, ctx, groups):
    from kmertools_amd._lib import KT_ERR_ARG, KT_MEM_DEVICE
    h, ro = np.array([1, 2, 3], np.uint64), np.array([0, 1, 2, 3], U)
    go = np.array(groups, U)
    tl.refused(lambda: ctx.scaled_merge(h, None, ro, go), KT_ERR_ARG, "host")
    oh = torch_mod.full((8,), HPAT, dtype=torch_mod.int64, device="cuda")
    oo = torch_mod.full((8,), OPAT, dtype=torch_mod.int64, device="cuda")
    tl.refused(lambda: ctx.scaled_merge(dev(torch_mod, h), None, dev(torch_mod, ro), dev(torch_mod, go), oh, None, 8, oo, KT_MEM_DEVICE),
               KT_ERR_ARG, "device")
    torch_mod.cuda.synchronize()
    assert bool((oh == HPAT).all()) and bool((oo == OPAT).all())


# ---- the table ----------------------------------------------------------------------------------------------------------------------

FORM_READS = {"stale": None, "image": "small2", "dense": "bulk1", "target": "bulk1"}


@pytest.mark.parametrize("form", tf.FORMS)
@pytest.mark.parametrize("k", [15, 31])
def test_table_sketch_in_every_form(tf_rigs, torch_mod, oracle, monkeypatch, capfd, k, form):
    from kmertools_amd._lib import KT_MEM_DEVICE
    R = tf_rigs(k)
    scaled, seed = 7, 5
    c, m = tf.build(R, monkeypatch, capfd, form)
    try:
        wk, wc = m.stage(1)
        n_staged = c.export_stage_range(1, None)
        assert n_staged == len(wk)
        for lo, hi in ((1, None), (2, None), (2, 3)):
            wh, wa, wt = sr.table_sketch(m.keys, m.counts, lo, SAT if hi is None else hi, scaled, seed)
            gh, ga, gt = c.scaled_sketch(scaled, lo, hi, seed)
            assert tl.same(gh, wh) and tl.same(ga, wa) and gt == wt, (form, lo, hi, "host")
            dh, da = R.full(len(wh) + 3, HPAT, 64), R.full(len(wh) + 3, APAT, 32)
            dt = R.full(2, OPAT, 64)
            assert c.scaled_sketch(scaled, lo, hi, seed, None, None, 0, None, KT_MEM_DEVICE) == len(wh)
            assert c.scaled_sketch(scaled, lo, hi, seed, dh, da, len(wh) + 1, dt, KT_MEM_DEVICE) == len(wh)
            torch_mod.cuda.synchronize()
            assert tl.same(tl.u64(dh)[:len(wh)], wh) and tl.same(tl.u32(da)[:len(wh)], wa), (form, lo, hi, "device")
            assert (tl.u64(dh)[len(wh):] == HPAT).all() and tuple(int(x) for x in tl.u64(dt)) == wt
        assert (form == "stale") == (len(m.keys) == 0)
        # the other road to the same sketch: the reads' sketches, merged
        if FORM_READS[form]:
            bases, offsets = R.P.csr[FORM_READS[form]]
            bh, ba, bo, _ = R.ctx.scaled_sketch_host(bases, offsets, k, scaled, seed)
            mh, ma, _ = R.ctx.scaled_merge(bh, ba, bo, [0, len(offsets) - 1])
            th, ta, _ = c.scaled_sketch(scaled, 1, None, seed)
            assert len(th) > 100 and tl.same(mh, th) and tl.same(ma, ta), form
        # the walk imaged nothing and ended no stage; the table is what it was
        gk, gc = tl.by_key(*c.export_fetch(0, n_staged))
        assert tl.same(gk, wk) and tl.same(gc, wc), form + ": the staged export did not survive"
        assert c.size() == m.size
        gk, gc = c.export_host()
        assert tl.same(gk, m.keys) and tl.same(gc, m.counts), form
    finally:
        c.close()


@pytest.fixture(scope="module")
def tf_rigs():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    made = {}

    def rig(k):
        if k not in made:
            made[k] = tl.Rig(torch, tl.plan(k), own_stream=False)
        return made[k]
    yield rig
    for R in made.values():
        R.close()


def test_table_sketch_of_an_overflowed_table_and_bad_arguments(tf_rigs, torch_mod, monkeypatch):
    from kmertools_amd._lib import KT_ERR_ARG, KT_ERR_FULL, KT_MEM_DEVICE
    R = tf_rigs(15)
    tl.env_probing(monkeypatch)
    t = R.counter(1024)
    dh, da, dt = R.full(16, HPAT, 64), R.full(16, APAT, 32), R.full(2, OPAT, 64)
    try:
        t.add_pairs_host(np.arange(1, 300, dtype=np.uint64) * U(7919), np.ones(299, np.uint32))
        for lo, hi, scaled in ((0, None, 5), (3, 2, 5), (1, None, 0)):
            tl.refused(lambda: t.scaled_sketch(scaled, lo, hi, 0), KT_ERR_ARG, (lo, hi, scaled))
            tl.refused(lambda: t.scaled_sketch(scaled, lo, hi, 0, dh, da, 16, dt, KT_MEM_DEVICE), KT_ERR_ARG, (lo, hi, scaled))
        # a result that does not fit: nothing written, the size reported
        n = len(t.scaled_sketch(1, 1, None, 0)[0])
        assert n == 299
        tl.refused(lambda: t.scaled_sketch(1, 1, None, 0, dh, da, 16, dt, KT_MEM_DEVICE), KT_ERR_ARG, "too small")
        t.add_pairs_host(np.arange(1, 5000, dtype=np.uint64) * U(7919), np.ones(4999, np.uint32))
        tl.refused(lambda: t.scaled_sketch(5, 1, None, 0), KT_ERR_FULL, "host")
        tl.refused(lambda: t.scaled_sketch(5, 1, None, 0, dh, da, 16, dt, KT_MEM_DEVICE), KT_ERR_FULL, "device")
        torch_mod.cuda.synchronize()
        assert bool((dh == HPAT).all()) and bool((da == APAT).all()) and bool((dt == OPAT).all())
    finally:
        t.close()


# ---- pairs ---------------------------------------------------------------------------------------------------------------------------

def csr_of(rows):
    offsets = np.zeros(len(rows) + 1, np.uint64)
    offsets[1:] = np.cumsum([len(r) for r in rows])
    return np.concatenate(rows + [np.zeros(0, np.uint64)]).astype(np.uint64), offsets


def want_shared(a_rows, b_rows):
    return np.array([[len(np.intersect1d(a, b)) for b in b_rows] for a in a_rows], np.uint32).reshape(len(a_rows), len(b_rows))


@pytest.fixture(scope="module")
def pair_rows(oracle):
    """rows of 0, 1, 63, 64, 65 hashes drawn from one pool (so that they overlap), disjoint and identical ones, and the
    sketch of a 40 kb sequence at scaled = 1: about 40 000 hashes, more than a tile of 16 384"""
    rng = np.random.default_rng(31)
    seq = ACGT[rng.integers(0, 4, size=40_000)]
    (_, long_row, _), = sr.read_rows(oracle, seq, np.array([0, len(seq)], U), 21, 1, 0)
    assert len(long_row) > 2 * 16384
    pool = np.unique(np.concatenate([long_row[::37], rng.integers(0, 1 << 63, size=300).astype(np.uint64)]))
    rows = [np.sort(rng.choice(pool, size=L, replace=False)) for L in (0, 1, 63, 64, 65, 0, 200, 64)]
    rows.append(rows[3].copy())                                   # identical to another row
    rows.append(np.array([1, 5, 1 << 63], np.uint64))             # disjoint from the pool (odd low values, a top bit)
    rows.append(long_row[16384 - 3:16384 + 3].copy())             # around the first tile's edge
    rows.append(np.array([long_row[0], long_row[16383], long_row[16384], long_row[-1]], np.uint64))
    return rows, long_row


def test_pairs(torch_mod, ctx, pair_rows):
    from kmertools_amd._lib import KT_MEM_DEVICE
    rows, long_row = pair_rows
    a_rows = rows + [long_row]
    b_rows = [long_row[5::3].copy(), rows[2], np.zeros(0, np.uint64), long_row] + rows[6:]
    ah, ao = csr_of(a_rows)
    bh, bo = csr_of(b_rows)
    want = want_shared(a_rows, b_rows)
    assert want[-1, 3] == len(long_row) and want[-1, 0] == len(long_row[5::3])
    assert tl.same(ctx.scaled_pairs_host(ah, ao, bh, bo), want)
    sh = Fenced(torch_mod, (len(a_rows), len(b_rows)), torch_mod.int32)
    ctx.scaled_pairs(dev(torch_mod, ah), dev(torch_mod, ao), len(a_rows), dev(torch_mod, bh), dev(torch_mod, bo), len(b_rows), sh.t,
                     KT_MEM_DEVICE)
    torch_mod.cuda.synchronize()
    sh.check("pairs")
    assert tl.same(sh.np(np.uint32), want)
    # a == b: symmetric, the diagonal the sizes
    self_want = want_shared(a_rows, a_rows)
    got = ctx.scaled_pairs_host(ah, ao)
    assert tl.same(got, self_want) and tl.same(got, got.T.copy())
    assert got.diagonal().tolist() == [len(r) for r in a_rows]
    d_h, d_o = dev(torch_mod, ah), dev(torch_mod, ao)
    sq = torch_mod.full((len(a_rows), len(a_rows)), APAT, dtype=torch_mod.int32, device="cuda")
    ctx.scaled_pairs(d_h, d_o, len(a_rows), d_h, d_o, len(a_rows), sq, KT_MEM_DEVICE)
    torch_mod.cuda.synchronize()
    assert tl.same(tl.u32(sq), self_want)
    # a block of rows of A, as the command line takes them: the offsets keep their origin
    assert tl.same(ctx.scaled_pairs_host(ah, ao[4:9], bh, bo), want[4:8])


# ---- the conventions -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shift", [0, 1, 3, 4, 15, 17])
def test_batch_on_views_into_fenced_outputs(torch_mod, ctx, oracle, shift):
    from kmertools_amd._lib import KT_ERR_ARG, KT_MEM_HOST
    b = rb.Batch("views", noisy_reads(40 + shift, 60))
    k, scaled, seed = 17, 4, 6
    rows = sr.rows_of(hashes_of(oracle, b.name + str(shift), b.bases, b.offsets, k, seed), scaled)
    wh, wa, wo, wn = sr.csr(rows)
    n, n_out = b.n, len(wh)
    assert n_out > 100
    # device
    bv, ov = bases_view(torch_mod, b.bases, shift), offsets_view(torch_mod, b.offsets)
    fh = Fenced(torch_mod, n_out, torch_mod.int64, align=8 * (shift % 2))
    fa = Fenced(torch_mod, n_out, torch_mod.int32, align=4 * (shift % 4))
    fo = Fenced(torch_mod, n + 1, torch_mod.int64, align=8)
    fn = Fenced(torch_mod, n, torch_mod.int32, align=4)
    assert ctx.scaled_sketch(bv, ov, n, k, scaled, fh.t, fa.t, n_out, fo.t, fn.t, seed) == n_out
    torch_mod.cuda.synchronize()
    for f_, w, dt in ((fh, wh, np.uint64), (fa, wa, np.uint32), (fo, wo, np.uint64), (fn, wn, np.uint32)):
        f_.check("device shift %d" % shift)
        assert tl.same(f_.np(dt), w)
    # too small by one: nothing is written, the size is exact
    for f_ in (fh, fa, fo, fn):
        f_.t.fill_(0x11)
    tl.refused(lambda: ctx.scaled_sketch(bv, ov, n, k, scaled, fh.t, fa.t, n_out - 1, fo.t, fn.t, seed), KT_ERR_ARG, "too small")
    torch_mod.cuda.synchronize()
    for f_ in (fh, fa, fo, fn):
        f_.check("too small")
        assert bool((f_.t == 0x11).all())
    # host
    hb = host_bases_view(b.bases, shift)
    gh, ga = HostFenced(n_out, np.uint64), HostFenced(n_out, np.uint32)
    go, gn = HostFenced(n + 1, np.uint64), HostFenced(n, np.uint32)
    assert ctx.scaled_sketch(hb, b.offsets, n, k, scaled, gh.a, ga.a, n_out, go.a, gn.a, seed, KT_MEM_HOST) == n_out
    for g, w in ((gh, wh), (ga, wa), (go, wo), (gn, wn)):
        g.check("host shift %d" % shift)
        assert tl.same(g.a, w)
    # abunds and n_kmers left out
    go2 = HostFenced(n + 1, np.uint64)
    assert ctx.scaled_sketch(hb, b.offsets, n, k, scaled, gh.a, None, n_out, go2.a, None, seed, KT_MEM_HOST) == n_out
    assert tl.same(go2.a, wo) and tl.same(gh.a, wh)


def test_too_small_reports_the_exact_size(torch_mod, ctx, oracle):
    from kmertools_amd import _lib
    import ctypes as C
    b = rb.Batch("small", noisy_reads(3, 30))
    k, scaled = 11, 2
    wh = sr.csr(sr.read_rows(oracle, b.bases, b.offsets, k, scaled, 0))[0]
    h, a = np.full(len(wh), HPAT, np.uint64), np.full(len(wh), APAT, np.uint32)
    ro, nk = np.full(b.n + 1, OPAT, np.uint64), np.full(b.n, APAT, np.uint32)
    n_out = C.c_uint64(12345)
    rc = _lib.lib().kt_scaled_batch(ctx._h, b.bases.ctypes.data, b.offsets.ctypes.data, b.n, k, scaled, 0, h.ctypes.data, a.ctypes.data,
                                    len(wh) - 1, ro.ctypes.data, nk.ctypes.data, C.byref(n_out), _lib.KT_MEM_HOST)
    assert rc == _lib.KT_ERR_ARG and n_out.value == len(wh)
    assert (h == HPAT).all() and (a == APAT).all() and (ro == OPAT).all() and (nk == APAT).all()


def _small():
    from kmertools_amd.device import to_csr
    return to_csr([b"ACGTACGTTGCAACGTAGCTAGCTAGGATCGA", b"ACGT"])


def test_argument_errors_leave_the_outputs_alone(torch_mod, ctx):
    from kmertools_amd._lib import KT_ERR_ARG, KT_MEM_HOST
    bases, offsets = _small()
    h, a = np.full(64, HPAT, np.uint64), np.full(64, APAT, np.uint32)
    ro, nk = np.full(3, OPAT, np.uint64), np.full(2, APAT, np.uint32)

    def batch(k=5, scaled=2, mem=KT_MEM_HOST, hashes=h, row_offsets=ro, offs=offsets, max_out=64):
        return lambda: ctx.scaled_sketch(bases, offs, 2, k, scaled, hashes, a, max_out, row_offsets, nk, 0, mem)
    for k in (0, 32, -1):
        tl.refused(batch(k=k), KT_ERR_ARG, "k")
    tl.refused(batch(scaled=0), KT_ERR_ARG, "scaled 0")
    tl.refused(batch(mem=7), KT_ERR_ARG, "mem")
    tl.refused(batch(hashes=None), KT_ERR_ARG, "null hashes with max_out")
    tl.refused(batch(row_offsets=None), KT_ERR_ARG, "null row_offsets")
    tl.refused(batch(offs=None), KT_ERR_ARG, "null offsets")
    sh = np.full((2, 2), APAT, np.uint32)
    tl.refused(lambda: ctx.scaled_pairs(h, None, 2, h, ro, 2, sh, KT_MEM_HOST), KT_ERR_ARG, "pairs: null offsets")
    tl.refused(lambda: ctx.scaled_pairs(h, np.array([0, 1, 2], U), 2, h, np.array([0, 1, 2], U), 2, None, KT_MEM_HOST), KT_ERR_ARG,
               "pairs: null shared")
    tl.refused(lambda: ctx.scaled_pairs(h, np.array([0, 1, 2], U), 2, h, np.array([0, 1, 2], U), 2, sh, 9), KT_ERR_ARG, "pairs: mem")
    tl.refused(lambda: ctx.scaled_pairs(h, np.array([0, 1 << 32, 1 << 32], U), 2, h, np.array([0, 1, 2], U), 2, sh, KT_MEM_HOST),
               KT_ERR_ARG, "pairs: a row of 2^32")
    assert (h == HPAT).all() and (a == APAT).all() and (ro == OPAT).all() and (nk == APAT).all() and (sh == APAT).all()
    # nothing to do is no error
    assert ctx.scaled_sketch(None, None, 0, 5, 2, None, None, 0, None, None, 0, KT_MEM_HOST) == 0
    ctx.scaled_pairs(None, None, 0, None, None, 0, None, KT_MEM_HOST)


# ---- the command line --------------------------------------------------------------------------------------------------------------------

def scaled_lines(oracle, recs, k, scaled, seed, abund):
    from kmertools_amd import device
    bases, offsets = device.to_csr([q for _, q in recs])
    rows = sr.read_rows(oracle, bases, offsets, k, scaled, seed)
    lines = []
    for (name, q), (w, h, a) in zip(recs, rows):
        line = "%s\t%d\t%d\t%d\t%s" % (name, len(q), w, len(h), ",".join(str(int(x)) for x in h))
        lines.append(line + ("\t" + ",".join(str(int(x)) for x in a) if abund else ""))
    return lines, rows


def check_contain(path, pairs, k, min_contain=0.0):
    """pairs: (id_a, id_b, hashes of a, hashes of b) in the order of the file, before --min-contain"""
    want = []
    for ida, idb, ha, hb in pairs:
        sh, sa, sb = len(np.intersect1d(ha, hb)), len(ha), len(hb)
        ca, cb = (sh / sa if sa else 0.0), (sh / sb if sb else 0.0)
        if max(ca, cb) < min_contain:
            continue
        size = sa if ca >= cb else sb
        ani = 0.0 if not sh or not size else 1.0 if sh == size else math.pow(sh / size, 1.0 / k)
        want.append((ida, idb, sh, sa, sb, sh / (sa + sb - sh) if sa + sb - sh else 0.0, ca, cb, ani))
    got = [line.split("\t") for line in open(path).read().splitlines()]
    assert len(got) == len(want), (len(got), len(want))
    for g, w in zip(got, want):
        assert len(g) == 9 and (g[0], g[1]) == w[:2] and tuple(int(x) for x in g[2:5]) == w[2:5], (g, w)
        for x, y in zip(g[5:], w[5:]):
            assert abs(float(x) - y) <= 1e-12, (g, w)
    return len(want)


def test_cli_scaled_end_to_end(oracle, tmp_path):
    k, scaled, seed = 15, 5, 5
    recs = ts.cli_records(1, 17)
    fa = tmp_path / "a.fa"
    ts.write_fasta(fa, recs)
    lines, rows = scaled_lines(oracle, recs, k, scaled, seed, False)
    lines_ab, _ = scaled_lines(oracle, recs, k, scaled, seed, True)
    out = tmp_path / "one"
    r = ts.cli_run("sketch", "-i", fa, "-o", out, "-k", k, "--scaled", scaled, "--seed", seed, "--contain")
    assert r.returncode == 0, r.stderr
    assert open(out / "sketch.tsv").read().splitlines() == lines
    pairs = [(recs[i][0], recs[j][0], rows[i][1], rows[j][1]) for i in range(len(recs)) for j in range(i + 1, len(recs))]
    assert check_contain(out / "sketch.contain", pairs, k) == len(pairs)
    assert not (out / "sketch.dist").exists()
    out2 = tmp_path / "two"
    r = ts.cli_run("sketch", "-i", fa, "-o", out2, "-k", k, "--scaled", scaled, "--seed", seed, "--abund", env={"KT_CLI_BATCH_READS": "4"})
    assert r.returncode == 0, r.stderr
    assert open(out2 / "sketch.tsv").read().splitlines() == lines_ab
    assert not (out2 / "sketch.contain").exists()
    # --single: several merges give what one gives, the union of the records with the abundances summed
    bases = [q for _, q in recs]
    from kmertools_amd import device
    hs = sr.read_hashes(oracle, *device.to_csr(bases), k, seed)
    (w, uh, ua), = sr.rows_of([np.concatenate(hs)], scaled)
    want = "a.fa\t%d\t%d\t%d\t%s\t%s" % (sum(len(q) for q in bases), w, len(uh), ",".join(str(int(x)) for x in uh),
                                          ",".join(str(int(x)) for x in ua))
    for name, env in (("s1", {}), ("s2", {"KT_CLI_BATCH_READS": "3"})):
        o = tmp_path / name
        r = ts.cli_run("sketch", "-i", fa, "-o", o, "-k", k, "--scaled", scaled, "--seed", seed, "--single", "--abund", env=env)
        assert r.returncode == 0, r.stderr
        assert open(o / "sketch.tsv").read().splitlines() == [want], name
    # without --scaled the command writes what it wrote before
    o = tmp_path / "plain"
    r = ts.cli_run("sketch", "-i", fa, "-o", o, "-k", k, "-s", 64, "--seed", seed)
    assert r.returncode == 0, r.stderr
    assert open(o / "sketch.tsv").read().splitlines() == ts.want_tsv(oracle, recs, k, 64, seed)[0]


def test_cli_table_against_genomes(oracle, tmp_path):
    """the case this is for: the solid k-mers of a read set's table against genomes"""
    from kmertools_amd import device
    k, scaled, seed = 21, 5, 0
    rng = np.random.default_rng(9)
    genomes = [("g%d" % i, ACGT[rng.integers(0, 4, size=L)].tobytes()) for i, L in enumerate((3000, 5000, 800, 0))]
    reads = []
    for name, g in genomes[:2]:  # reads of the first two genomes, 8x, with errors; the third genome is absent
        for _ in range(8 * len(g) // 100):
            a = int(rng.integers(0, len(g) - 100))
            q = bytearray(g[a:a + 100])
            if rng.random() < 0.5:
                q[int(rng.integers(0, 100))] = ord("ACGT"[int(rng.integers(0, 4))])
            reads.append(bytes(q))
    model = tm.Model(k)
    model.add_reads(*device.to_csr(reads))
    half = len(model.keys) // 2  # two sections, as an out-of-core count writes them
    tab = tmp_path / "reads.ktab"
    ktab_ref.write_file(tab, k, [(model.keys[:half], model.counts[:half]), (model.keys[half:], model.counts[half:])])
    fa = tmp_path / "genomes.fa"
    ts.write_fasta(fa, genomes)
    out = tmp_path / "out"
    r = ts.cli_run("sketch", "--scaled", scaled, "--table", tab, "--min-count", 2, "-a", fa, "-o", out, "-k", k, "--contain",
                   "--min-contain", "0.1", "--abund")
    assert r.returncode == 0, r.stderr
    th, ta, (entries, occ) = sr.table_sketch(model.keys, model.counts, 2, SAT, scaled, seed)
    assert len(th) > 200
    want = "reads.ktab\t0\t%d\t%d\t%s\t%s" % (occ, len(th), ",".join(str(int(x)) for x in th), ",".join(str(int(x)) for x in ta))
    assert open(out / "sketch.tsv").read().splitlines() == [want]
    lines, rows = scaled_lines(oracle, genomes, k, scaled, seed, True)
    assert open(out / "sketch.alt.tsv").read().splitlines() == lines
    pairs = [("reads.ktab", name, th, rows[j][1]) for j, (name, _) in enumerate(genomes)]
    assert check_contain(out / "sketch.contain", pairs, k, 0.1) == 2  # the two genomes the reads came from
    got = [line.split("\t") for line in open(out / "sketch.contain").read().splitlines()]
    assert [g[1] for g in got] == ["g0", "g1"] and all(float(g[7]) > 0.8 for g in got)
    # --max-count: the count range's other end
    out2 = tmp_path / "out2"
    r = ts.cli_run("sketch", "--scaled", scaled, "--table", tab, "--min-count", 1, "--max-count", 1, "-o", out2, "-k", k)
    assert r.returncode == 0, r.stderr
    th1, _, (_, occ1) = sr.table_sketch(model.keys, model.counts, 1, 1, scaled, seed)
    assert open(out2 / "sketch.tsv").read().splitlines() == ["reads.ktab\t0\t%d\t%d\t%s" % (occ1, len(th1), ",".join(str(int(x)) for x in th1))]
