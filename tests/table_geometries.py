"""The contents tests/test_table_geometries.py puts into tables of every shape, decided on the CPU.

A table's shape (kt_table.hpp kttab::Geom, restated as tests/table_model.py geometry / home_of / layout) follows from the
capacity asked for: one small range, one or two ranges of 8192 slots, or a row of ranges of 1024 * m8 slots, m8 in 5..8.
Random keys at load 0.85 hardly ever probe past the end of a range, so plan() draws keys whose home is in a range's last
slots (keys_homed_at) and proves with the placement simulation that their probe sequences wrap:

  high   k-mers of noisy reads of a small genome (graph structure) + random canonical k-mers up to load 0.85 + per
         clustered range (the first, the last, one in the middle) 24 keys homed in its last 4 slots and, where needed, a
         ramp of keys homed just before them, until the longest displacement is 64 or more.  `base`: what reads spell
         (counts 1..3); `pairs`: the add_pairs call on top that brings the counts to 1..9, 255, 256 and 0xFFFFFFFF
  low    load 0.3 of the same kind, so few k-mers per range that a fresh dense build keeps claim lists (LIST_KEYS)
  brim   one range exactly full of keys homed in it, every other range nearly empty, one more key of that range
  absent keys no content holds, some of them homed in the last slots of every clustered range and in the full range

Every content is a tests/table_model.py Model; `reads_of` spells any (keys, counts) as reads of exactly k bases."""
import functools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import graph_ref as gr  # noqa: E402
import table_model as tm  # noqa: E402
from test_table_lifecycle import genome_of, sample_reads  # noqa: E402

U32 = 0xFFFFFFFF
LIST_KEYS = 3072  # kt_bulk.hip: a range of more k-mers than this is built by the packed variant
# request -> (capacity, ranges, m8)
SHAPES = {1024: (1024, 1, 8), 4096: (4096, 1, 8), 8192: (8192, 1, 8), 16384: (16384, 2, 8), 20000: (20480, 4, 5),
          24000: (24576, 4, 6), 28000: (28672, 4, 7), 32768: (32768, 4, 8), 40000: (40960, 8, 5), 81920: (81920, 16, 5)}
REQUESTS = tuple(SHAPES)
BULK_FROM = 20000  # the bulk build takes tables of four ranges or more (split_bits)
# every shape with a 32-bit and a 64-bit key width; the first of a pair meets every writer and reader, the second the core
WIDTHS = {1024: (31, 15), 4096: (15, 21), 8192: (21, 15), 16384: (15, 31), 20000: (31, 15), 24000: (15, 21), 28000: (21, 15),
          32768: (15, 31), 40000: (31, 15), 81920: (15, 21)}
# the table a content is saved from / compared with has another shape
OTHER = {1024: 20000, 4096: 24000, 8192: 28000, 16384: 40000, 20000: 4096, 24000: 20000, 28000: 40000, 32768: 24000,
         40000: 28000, 81920: 20000}
# the table a content is saved from has another shape too, one with room for it: request -> (request, its capacity)
FILE_FROM = {1024: (20000, 20480), 4096: (24000, 24576), 8192: (28000, 28672), 16384: (40000, 40960), 20000: (24000, 24576),
             24000: (28000, 28672), 28000: (40000, 40960), 32768: (40000, 40960), 40000: (81920, 81920),
             81920: (100000, 114688)}
CLUSTER, CLUSTER_IN, LAST = 32, 24, 4  # keys drawn per clustered range, of them in the contents, homed in the last LAST slots


def bulk_eligible(request):
    return request >= BULK_FROM


def clustered_ranges(g):
    return sorted({0, g.n_ranges - 1} | ({g.n_ranges // 2} if g.n_ranges > 2 else set()))


def reads_of(keys, counts, k, rng):
    """one read of exactly k bases per occurrence (either strand, in random order) -> list of bytes"""
    keys = np.repeat(np.asarray(keys, np.uint64), np.asarray(counts, np.int64))
    flip = rng.random(len(keys)) < 0.5
    keys = np.where(flip, gr.rc_np(keys, k), keys)[rng.permutation(len(keys))]
    shifts = np.uint64(2) * np.arange(k - 1, -1, -1, dtype=np.uint64)
    text = np.frombuffer(b"ACGT", np.uint8)[((keys[:, None] >> shifts[None, :]) & np.uint64(3)).astype(np.int64)]
    return [row.tobytes() for row in text]


def per_range_occurrences(m, g):
    r, _ = tm.home_of(m.keys, m.k, g)
    return np.bincount(r, weights=m.counts.astype(np.float64), minlength=g.n_ranges).astype(np.int64)


class Plan:
    pass


def model_of_reads(k, seqs):
    from kmertools_amd.device import to_csr
    m = tm.Model(k)
    m.add_reads(*to_csr(seqs))
    return m


def grown_reads(rng, genome, k, target, err, step):
    """noisy reads of the genome, `step` more at a time, until they hold `target` distinct k-mers -> (reads, their Model)"""
    seqs = []
    while True:
        seqs += sample_reads(rng, genome, step, k, err)[:step]
        m = model_of_reads(k, seqs)
        if m.size >= target:
            return seqs, m


@functools.lru_cache(maxsize=None)
def plan(request, k):
    from kmertools_amd.device import to_csr
    P = Plan()
    P.request, P.k = request, k
    g = P.g = tm.geometry(request, k)
    cap, rs = g.cap, g.range_slots
    assert (cap, g.n_ranges, g.m8) == SHAPES[request]
    rng = np.random.default_rng(1000 * request + k)
    P.clustered = clustered_ranges(g)
    P.clusters, P.cluster_in, P.cluster_out = {}, {}, {}
    for r in P.clustered:
        ck = tm.keys_homed_at(k, g, r, (rs - LAST, rs - 1), CLUSTER)
        P.clusters[r], P.cluster_in[r], P.cluster_out[r] = ck, ck[:CLUSTER_IN], ck[CLUSTER_IN:]
    clusters_in = np.concatenate([P.cluster_in[r] for r in P.clustered])
    every_cluster = np.concatenate([P.clusters[r] for r in P.clustered])

    # ---- high ---------------------------------------------------------------------------------------------------------
    genome = genome_of(rng, max(600, cap * 2 // 5))
    P.graph_reads, gm = grown_reads(rng, genome, k, int(0.42 * cap), 0.01, max(2, cap // 6000))
    assert gm.size <= 0.65 * cap and not gm.count(every_cluster).any()
    pool = np.setdiff1d(tm.canonical_keys(rng, k, cap + 6000), np.concatenate([gm.keys, every_cluster]))
    pool = pool[rng.permutation(len(pool))]
    n_random = int(0.85 * cap) - gm.size - len(clusters_in)
    random_in, pool = pool[:n_random], pool[n_random:]
    spelled = np.concatenate([random_in, clusters_in])
    spelled_counts = rng.integers(1, 4, size=len(spelled)).astype(np.uint32)
    # the ramp: keys homed in the 60 slots before a cluster's, 8 more per clustered range at a time
    ramp = np.zeros(0, np.uint64)
    for round_ in range(12):
        keys = np.concatenate([gm.keys, spelled, ramp])
        L = tm.layout(keys, k, g)
        if int(L.displacement.max()) >= 64:
            break
        more = [tm.keys_homed_at(k, g, r, (rs - LAST - 60, rs - LAST - 1), 8 * (round_ + 1), seed=11) for r in P.clustered]
        ramp = np.setdiff1d(np.concatenate(more), np.concatenate([gm.keys, spelled, every_cluster]))
    P.ramp = ramp
    spelled = np.concatenate([spelled, ramp])
    spelled_counts = np.concatenate([spelled_counts, rng.integers(1, 4, size=len(ramp)).astype(np.uint32)])
    P.spelled_reads = reads_of(spelled, spelled_counts, k, rng)
    P.high_reads = P.graph_reads + P.spelled_reads
    order = rng.permutation(len(P.high_reads))
    P.high_reads = [P.high_reads[i] for i in order]
    base = tm.Model(k)
    base._merge(gm.keys, gm.counts)
    base._merge(spelled, spelled_counts)
    P.base = base
    pool = np.setdiff1d(pool, ramp)
    # the pairs on top: a quarter of the keys gets 1..6 more, three keys each end at 255, 256 and 0xFFFFFFFF, one of
    # them a cluster key of every clustered range; a few pairs with count 0 of absent keys, a few keys twice
    raised = rng.choice(base.keys, base.size // 4, replace=False)
    pk, pc = [raised], [rng.integers(1, 7, size=len(raised)).astype(np.uint32)]
    rest = np.setdiff1d(base.keys, raised)
    edge_keys = np.concatenate([rng.choice(np.setdiff1d(rest, clusters_in), 9 - len(P.clustered), replace=False),
                                [np.setdiff1d(P.cluster_in[r], raised)[0] for r in P.clustered]]).astype(np.uint64)
    assert len(edge_keys) == 9
    edge_to = np.array([255, 256, U32] * 3, np.uint64)
    pk.append(edge_keys)
    pc.append((edge_to - base.count(edge_keys)).astype(np.uint32))
    P.edge_keys = edge_keys
    pk, pc = np.concatenate(pk), np.concatenate(pc)
    assert len(np.unique(pk)) == len(pk)
    twice = pk[:5]
    pk, pc = np.concatenate([pk, twice, pool[:4]]), np.concatenate([pc, np.full(5, 2, np.uint32), np.zeros(4, np.uint32)])
    pool = pool[4:]
    order = rng.permutation(len(pk))
    P.pairs = (pk[order], pc[order])
    high = base.copy()
    high.add_pairs(*P.pairs)
    P.high = high
    assert np.array_equal(high.keys, base.keys)
    P.high_layout = tm.layout(high.keys, k, g)

    # ---- low ----------------------------------------------------------------------------------------------------------
    n_low = 0
    while model_of_reads(k, P.graph_reads[:n_low]).size < 0.12 * cap:
        n_low += max(2, cap // 6000)
    low_graph = model_of_reads(k, P.graph_reads[:n_low])
    few = np.concatenate([P.cluster_in[r][:8] for r in P.clustered])
    low_random = random_in[:max(0, int(0.3 * cap) - low_graph.size - len(few))]
    P.low_reads = P.graph_reads[:n_low] + reads_of(np.concatenate([low_random, few]), np.ones(len(low_random) + len(few), np.int64), k, rng)
    order = rng.permutation(len(P.low_reads))
    P.low_reads = [P.low_reads[i] for i in order]
    low = low_graph.copy()
    low._merge(np.concatenate([low_random, few]), np.ones(len(low_random) + len(few), np.uint32))
    P.low = low

    # ---- brim ---------------------------------------------------------------------------------------------------------
    P.brim_range = b = g.n_ranges // 2
    bk = tm.keys_homed_at(k, g, b, None, rs + 1 + 40, seed=13)
    bk = bk[np.random.default_rng(request + k).permutation(len(bk))]  # (ascending keys are not spread over the k-mers)
    P.brim_full, P.brim_extra, P.brim_absent = bk[:rs], bk[rs:rs + 1], bk[rs + 1:]
    others = [tm.keys_homed_at(k, g, r, None, 60, seed=13) for r in range(g.n_ranges) if r != b]
    P.brim_others = np.concatenate(others) if others else np.zeros(0, np.uint64)
    brim_keys = np.concatenate([P.brim_full, P.brim_others])
    P.brim = tm.Model(k)
    P.brim.add_pairs(brim_keys, rng.integers(1, 10, size=len(brim_keys)).astype(np.uint32))
    P.brim_reads = reads_of(P.brim.keys, np.minimum(P.brim.counts, 2), k, rng)
    P.brim_read_model = tm.Model(k, P.brim.keys, np.minimum(P.brim.counts, 2))

    # ---- absent keys: random ones, the clusters' last eight, the ramp's neighbours ------------------------------------------
    held = np.concatenate([high.keys, brim_keys, P.brim_extra, P.brim_absent])
    P.absent = np.setdiff1d(np.concatenate([pool[:1500], every_cluster]), held)
    P.absent = P.absent[rng.permutation(len(P.absent))]

    # ---- erase: a third of the keys, half of them added back ------------------------------------------------------------------
    L = P.high_layout
    must = []
    for r in P.clustered:
        ck = P.cluster_in[r]
        at = np.searchsorted(high.keys, ck)
        wrapped = L.wrapped[at]
        # the first and a middle cluster key, the last one that stayed before the range's end and the first that wrapped
        must += [ck[0], ck[len(ck) // 2]] + list(ck[~wrapped][-1:]) + list(ck[wrapped][:1])
        in_r = L.range == r
        must += list(high.keys[in_r & (L.slot == rs - 1)]) + list(high.keys[in_r & (L.slot == 0)])
    must = np.unique(np.array(must, np.uint64))
    n_gone = high.size // 3
    rest = np.setdiff1d(high.keys, must)
    gone = np.concatenate([must, rng.choice(rest, n_gone - len(must), replace=False)])
    P.erase_must = must
    P.gone = gone[rng.permutation(len(gone))]
    back = np.concatenate([must[::2], rng.choice(np.setdiff1d(gone, must), n_gone // 2 - len(must[::2]), replace=False)])
    P.back = (back, rng.integers(1, 10, size=len(back)).astype(np.uint32))
    keep = ~np.isin(high.keys, gone)
    P.erased = tm.Model(k, high.keys[keep], high.counts[keep])
    P.erased_back = P.erased.copy()
    P.erased_back.add_pairs(*P.back)

    # ---- halves for the merge: the reads dealt out, the cluster keys' reads fall to both -----------------------------------------
    P.half_reads = (P.high_reads[0::2], P.high_reads[1::2])
    P.half_models = tuple(model_of_reads(k, h) for h in P.half_reads)

    # ---- what the readers of tests/test_table_lifecycle.py take from a plan -----------------------------------------------------
    prof = sample_reads(rng, genome, 14, k, 0.01) + [b"", b"ACGTN" * 9]
    prof += reads_of(np.concatenate([clusters_in[::5], P.absent[:6], edge_keys]), np.ones(len(clusters_in[::5]) + 6 + 9, np.int64), k, rng)
    P.seqs = {"profile": prof}
    P.csr = {"profile": to_csr(prof), "high": to_csr(P.high_reads), "low": to_csr(P.low_reads), "brim": to_csr(P.brim_reads),
             "half0": to_csr(P.half_reads[0]), "half1": to_csr(P.half_reads[1])}
    # the partner of compare / setop, a table of another shape: half its keys are the content's
    half = rng.choice(high.keys, min(1500, high.size // 2), replace=False)
    pkeys = np.unique(np.concatenate([half, pool[1500:2500]] + [P.clusters[r][CLUSTER_IN - 3:CLUSTER_IN + 2] for r in P.clustered]))
    P.partner = tm.Model(k)
    P.partner.add_pairs(pkeys, rng.integers(1, 8, size=len(pkeys)).astype(np.uint32))
    P.partner_request = OTHER[request]
    assert P.partner.size <= 0.7 * SHAPES[P.partner_request][0] and len(pool) >= 2500
    P.cluster = every_cluster  # (what lookup_keys appends to its keys as P.cluster)
    return P


def check_plan(P):
    """what the GPU tests rest on, asserted without a GPU: the loads, the wraps in every clustered range, the longest
    displacement, the claim-list threshold, the full range of brim, the absent keys' homes, the erase set, the reads"""
    g, k, rs = P.g, P.k, P.g.range_slots
    for name, m in (("high", P.high), ("base", P.base)):
        assert abs(m.size / g.cap - 0.85) <= 0.02, (name, m.size / g.cap)
    L = P.high_layout
    assert L.fill.max() <= 0.95 * rs, L.fill
    for r in P.clustered:
        assert int((L.wrapped & (L.range == r)).sum()) >= 16, (r, int((L.wrapped & (L.range == r)).sum()))
        rr, pp = tm.home_of(P.clusters[r], k, g)
        assert (rr == r).all() and (pp >= rs - LAST).all() and len(np.unique(P.clusters[r])) == CLUSTER
        assert P.high.count(P.cluster_in[r]).all() and not P.high.count(P.cluster_out[r]).any()
        assert P.low.count(P.cluster_in[r][:8]).all()
    assert int(L.displacement.max()) >= 64, int(L.displacement.max())
    for v in (255, 256, U32):
        assert int((P.high.counts == v).sum()) >= 3, v
    assert P.base.counts.max() < 250 and set(range(1, 10)) <= set(P.high.counts.tolist())
    assert P.clustered == ([0] if g.n_ranges == 1 else [0, 1] if g.n_ranges == 2 else [0, g.n_ranges // 2, g.n_ranges - 1])
    # low: load 0.3, few k-mers per range; high: more than the claim lists take
    assert abs(P.low.size / g.cap - 0.3) <= 0.03, P.low.size / g.cap
    if bulk_eligible(P.request):
        assert per_range_occurrences(P.low, g).max() <= LIST_KEYS, per_range_occurrences(P.low, g)
        assert tm.layout(P.high.keys, k, g).fill.min() > LIST_KEYS
        for h in P.half_models:
            assert h.occurrences >= 0.3 * g.cap
    # brim: one range exactly full of its own keys, 100 keys or fewer in every other, the extra key is the full range's
    B = tm.layout(P.brim.keys, k, g)
    assert B.fill[P.brim_range] == rs and all(f <= 100 for r, f in enumerate(B.fill) if r != P.brim_range), B.fill
    for keys in (P.brim_extra, P.brim_absent):
        assert (tm.home_of(keys, k, g)[0] == P.brim_range).all() and not P.brim.count(keys).any()
    assert len(P.brim_extra) == 1 and len(P.brim_absent) == 40
    assert int(B.wrapped.sum()) >= 1
    # absent keys: in no content, some homed in the last slots of every clustered range
    for m in (P.high, P.low, P.brim):
        assert not m.count(P.absent).any()
    ar, ap = tm.home_of(P.absent, k, g)
    for r in P.clustered:
        assert int(((ar == r) & (ap >= rs - LAST)).sum()) >= CLUSTER - CLUSTER_IN
    # erase: a third, with the keys at the wrap of every clustered range; half of them back
    assert abs(len(P.gone) / P.high.size - 1 / 3) < 0.01 and len(np.unique(P.gone)) == len(P.gone)
    assert np.isin(P.erase_must, P.gone).all() and abs(len(P.back[0]) / len(P.gone) - 0.5) < 0.01
    assert np.isin(P.back[0], P.gone).all()
    for r in P.clustered:
        for s in (0, rs - 1):
            at = high_key_at(P, r, s)
            assert at is None or at in P.gone
        assert int(np.isin(P.cluster_in[r], P.gone).sum()) >= 4
    # the reads spell the contents
    for name, m in (("high", P.base), ("low", P.low), ("brim", P.brim_read_model)):
        got = tm.Model(k)
        got.add_reads(*P.csr[name])
        assert np.array_equal(got.keys, m.keys) and np.array_equal(got.counts, m.counts), name
    both = P.half_models[0].copy()
    both._merge(P.half_models[1].keys, P.half_models[1].counts)
    assert np.array_equal(both.keys, P.base.keys) and np.array_equal(both.counts, P.base.counts)
    for r in P.clustered:
        assert P.half_models[0].count(P.cluster_in[r]).any() and P.half_models[1].count(P.cluster_in[r]).any()


def high_key_at(P, r, slot):
    L = P.high_layout
    at = np.flatnonzero((L.range == r) & (L.slot == slot))
    return int(P.high.keys[at[0]]) if len(at) else None
