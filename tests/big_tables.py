"""The contents tests/test_big_tables.py puts into tables of 2^32 bytes and more, decided on the CPU.

A slot is 16 bytes: its byte offset leaves 32 bits at slot 2^28, its index a signed 32-bit int at 2^31 and an unsigned one
at 2^32 - the EDGES.  A table of 2^28 .. 2^33 slots has 2^15 .. 2^20 ranges, far too many to fill: the contents are sparse
and steered.  The hash is invertible (table_model.hash_inverse), so the keys are built, not searched for
(table_model.keys_built_at).  plan(name) of a k = 31 shape holds

  fills     the range that straddles every edge inside the table, range 0 and the last range, each at load 0.85
  clusters  per edge 72 keys homed in the 8 positions just below it - 64 in the content, which pile across the edge (a
            carry lost between a 64-bit range base and a 32-bit offset shows there), 8 left out -, and the same in the
            last 8 positions of range 0 and of the last range: their probe sequences wrap, the last range's at the table's
            very last slot
  graph     the k-mers of noisy reads of a 20 kb genome (table_geometries.grown_reads), homed all over the table, and a
            path of 40 k-mers through every cluster key of the content, so that neighbour probes start at the edges
  counts    1 .. 300: the fills and clusters are spelled as reads of exactly k bases, one per occurrence

and what the writers and readers of tests/test_table_geometries.py take from a plan: the reads as CSR batches (whole and
in two halves), absent keys (the clusters' left-out ones first), a partner table, an erase set with the keys at the edges,
profile reads.  plan(name, 1) is a second, smaller content of other keys for the same shape (what follows a clear).
direct_plan(name): the k <= 16 tables of exactly 4^k slots, where the slot is the home - the canonical k-mers of
nhash_inv(s) for the slots s on either side of the edges, the first and last 64 and a few thousand at random.

check_plan / check_direct_plan prove the conditions with table_model.layout alone; they run in the CPU suite."""
import functools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import graph_ref as gr  # noqa: E402
import table_geometries as tg  # noqa: E402
import table_model as tm  # noqa: E402
from test_table_lifecycle import genome_of, sample_reads  # noqa: E402

# name -> (request, k, n, m8, slots)
SHAPES = {"A": (1 << 28, 31, 28, 8, 1 << 28), "B": (5 << 26, 31, 29, 5, 5 << 26), "E": (5 << 30, 31, 33, 5, 5 << 30),
          "D14": (4 ** 14, 14, 28, 8, 1 << 28), "D16": (4 ** 16, 16, 32, 8, 1 << 32)}
PROBED = ("A", "B", "E")
DIRECT = ("D14", "D16")
EDGES = (1 << 28, 1 << 31, 1 << 32)
EDGE_AT = {1 << 28: (52428, 4096), 1 << 31: (419430, 2048), 1 << 32: (838860, 4096)}  # (range, position) in the m8 = 5 shapes
SMALL_REQUEST, SMALL_SLOTS = 40000, 40960  # the partner's shape
# the small table of the same content (table files): the steered keys of a range share their top hash bits, so in ANY smaller
# table they fall into one range, homed at one position - 4416 of them and that range's share of the rest do not fit a range
# of 5120 slots (40 960 slots: 8 such ranges); a table of 8 ranges of 8192 slots holds them
FILE_REQUEST, FILE_SLOTS = 65536, 65536
LOAD = 0.85
CLUSTER, CLUSTER_IN, BELOW = 72, 64, 8
PATH = 40
GRAPH_KMERS = 10000
# bases of N among the reads: no k-mer more, and a job planned for enough keys that the level-1 bucket of a filled range -
# 4416 keys, 44 000 occurrences or so, all of them one bucket's - fits its region, level 1 stays paged and level 2 gets the
# fixed room its write-combining kernel wants (level2_of; check_plan proves it from the plan's own numbers)
BALLAST = {"A": 16 << 20, "B": 4 << 20, "E": 56 << 20}


def geometry(name):
    request, k, n, m8, slots = SHAPES[name]
    g = tm.geometry(request, k)
    assert (g.cap, g.n, g.m8) == (slots, n, m8), (name, g)
    return g


def edges_of(name):
    return [e for e in EDGES if e < SHAPES[name][4]]


def bytes_of(name):
    return SHAPES[name][4] * 16


# ---- the bulk job's own rules, restated (kt_bulk.hip: split_bits, region_room, kt_bulk_job::plan / arm_paged / level2) -----------

def split_bits(n, b1_env=0):
    """how the n hash bits above a range's 13 split between the two partition levels -> (b1, b2)"""
    fb = n - 13
    b1 = min((fb + 1) // 2, 10)
    if fb >= 16 and fb - b1 < 9:
        b1 = fb - 9
    if b1_env and b1_env <= 10 and b1_env < fb and fb - b1_env <= 11:
        b1 = b1_env
    return b1, fb - b1


def swwc_lds(B2):
    """SwwcShared<K>::bytes: a line and two words per fine bucket"""
    return B2 * 128 + B2 * 8 + 64


def level2_of(max_keys, n, key_bytes, b1_env=0, level1="paged"):
    """the `l2=` of a job's verbose line: level 2 has fixed room per fine bucket only behind a paged level 1 and where a
    bucket's room, split B2 ways, is a cache line of keys or more - then whole lines out of LDS (swwc) where one line per
    fine bucket fits 160 KB, else the sort buffer (fast); without fixed room the exact kernel takes every bucket (general)"""
    b1, b2 = split_bits(n, b1_env)
    B1, B2 = 1 << b1, 1 << b2
    cap1 = (max_keys // B1 + max_keys // B1 // 8 + 16 * 256 + 255) // 256 * 256
    per_line = 128 // key_bytes
    cap2 = cap1 // B2 // per_line * per_line if level1 == "paged" and cap1 * key_bytes < 1 << 31 else 0
    if not cap2:
        return "general"
    return "swwc" if B2 >= 512 and swwc_lds(B2) <= 160 * 1024 else "fast"


def level2_of_line(line, n, key_bytes, b1_env=0):
    f = dict(x.split("=") for x in line.split()[1:] if "=" in x and "<=" not in x)
    max_keys = int([x for x in line.split() if x.startswith("keys<=")][0][6:])
    return level2_of(max_keys, n, key_bytes, b1_env, f["level1"])


# ---- pieces of a content ------------------------------------------------------------------------------------------------------------

ACGT = np.frombuffer(b"ACGT", np.uint8)


def counts_for(rng, n):
    """1 .. 300: most small, one in twenty anywhere up to 300, both ends present"""
    c = rng.integers(1, 5, size=n)
    big = rng.random(n) < 0.05
    c[big] = rng.integers(5, 301, size=int(big.sum()))
    c[:2] = (1, 300)
    return c.astype(np.uint32)


def path_reads(keys, k, rng):
    """per key one read of k + PATH - 1 bases that holds it (on either strand) as its 21st k-mer"""
    keys = np.asarray(keys, np.uint64)
    keys = np.where(rng.random(len(keys)) < 0.5, gr.rc_np(keys, k), keys)
    shifts = np.uint64(2) * np.arange(k - 1, -1, -1, dtype=np.uint64)
    mid = ((keys[:, None] >> shifts[None, :]) & np.uint64(3)).astype(np.int64)
    left, right = rng.integers(0, 4, size=(len(keys), PATH // 2)), rng.integers(0, 4, size=(len(keys), PATH - 1 - PATH // 2))
    return [row.tobytes() for row in ACGT[np.concatenate([left, mid, right], axis=1)]]


def global_slots(L, g):
    return L.range * g.range_slots + L.home, L.range * g.range_slots + L.slot


class Plan:
    pass


def clusters_of(name):
    """{tag: (range, first position, last position)}: below every edge, at the end of range 0 and of the last range"""
    g = geometry(name)
    at = {"edge 2^%d" % (e.bit_length() - 1): (e // g.range_slots, e % g.range_slots - BELOW, e % g.range_slots - 1) for e in edges_of(name)}
    at["range 0"] = (0, g.range_slots - BELOW, g.range_slots - 1)
    at["last range"] = (g.n_ranges - 1, g.range_slots - BELOW, g.range_slots - 1)
    return at


@functools.lru_cache(maxsize=None)
def plan(name, variant=0):
    from kmertools_amd.device import to_csr
    P = Plan()
    request, k, _, _, _ = SHAPES[name]
    P.name, P.variant, P.request, P.k = name, variant, request, k
    g = P.g = geometry(name)
    rs = g.range_slots
    rng = np.random.default_rng([sum(name.encode()), variant, 20])
    P.edges = edges_of(name)
    for e in P.edges:
        assert (e // rs, e % rs) == EDGE_AT[e] and g.m8 == 5
    P.cluster_at = clusters_of(name)
    P.clusters, P.cluster_in, P.cluster_out, fills = {}, {}, {}, []
    for tag, (r, lo, hi) in P.cluster_at.items():
        ck = tm.keys_built_at(k, g, r, (lo, hi), CLUSTER, rng)
        ck = ck[rng.permutation(CLUSTER)]
        P.clusters[tag], P.cluster_in[tag], P.cluster_out[tag] = ck, ck[:CLUSTER_IN], ck[CLUSTER_IN:]
        fills.append(np.setdiff1d(tm.keys_built_at(k, g, r, None, int(LOAD * rs), rng), ck))
    P.filled = sorted(r for r, _, _ in P.cluster_at.values())
    clusters_in = np.concatenate(list(P.cluster_in.values()))
    every_cluster = np.concatenate(list(P.clusters.values()))
    spelled = np.concatenate(fills + [clusters_in])
    spelled_counts = counts_for(rng, len(spelled))
    # the graph: noisy reads of a small genome (variant 1, the content behind a clear: none), a path through every cluster key
    genome = genome_of(rng, 20000)
    if variant == 0:
        P.graph_reads, _ = tg.grown_reads(rng, genome, k, GRAPH_KMERS, 0.01, 20)
    else:
        P.graph_reads = []
    P.path_reads = path_reads(clusters_in, k, rng)
    P.spelled_reads = tg.reads_of(spelled, spelled_counts, k, rng)
    P.ballast_reads = [b"N" * (BALLAST[name] // 8)] * 8 if variant == 0 else []
    reads = P.graph_reads + P.path_reads + P.spelled_reads + P.ballast_reads
    order = rng.permutation(len(reads))
    P.high_reads = [reads[i] for i in order]
    base = tg.model_of_reads(k, P.graph_reads + P.path_reads)
    assert not base.count(np.concatenate(list(P.cluster_out.values()))).any()
    base._merge(spelled, spelled_counts)
    P.base, P.spelled, P.spelled_counts = base, spelled, spelled_counts
    P.layout = tm.layout(base.keys, k, g)
    P.half_reads = (P.high_reads[0::2], P.high_reads[1::2])

    # absent keys: the clusters' left-out ones, more keys homed on either side of every edge, random ones
    near = [tm.keys_built_at(k, g, e // rs, (e % rs - BELOW, e % rs + BELOW - 1), 16, rng) for e in P.edges]
    pool = tm.canonical_keys(rng, k, 6000)
    P.absent = np.concatenate([np.concatenate(list(P.cluster_out.values()))] + near + [pool[:2500]])
    P.absent = P.absent[~np.isin(P.absent, base.keys)]
    _, idx = np.unique(P.absent, return_index=True)
    P.absent = P.absent[np.sort(idx)]  # (the steered ones stay first: lookup_keys takes the first thousand)
    pool = np.setdiff1d(pool[2500:], base.keys)

    # the pairs on top, as tests/table_geometries.py has them: a quarter of the keys gets 1..6 more, nine keys - one of every
    # cluster among them - end at 255, 256 and 0xFFFFFFFF, five keys come twice, four absent keys come with count 0
    raised = rng.choice(base.keys, base.size // 4, replace=False)
    rest = np.setdiff1d(base.keys[base.counts < 200], raised)
    from_clusters = [np.intersect1d(P.cluster_in[tag], rest)[0] for tag in P.cluster_at]
    edge_keys = np.concatenate([rng.choice(np.setdiff1d(rest, clusters_in), 9 - len(from_clusters), replace=False),
                                from_clusters]).astype(np.uint64)
    assert len(edge_keys) == 9
    P.edge_keys = edge_keys
    pk = np.concatenate([raised, edge_keys])
    pc = np.concatenate([rng.integers(1, 7, size=len(raised)).astype(np.uint32),
                         (np.array([255, 256, tg.U32] * 3, np.uint64) - base.count(edge_keys)).astype(np.uint32)])
    pk, pc = np.concatenate([pk, pk[:5], pool[:4]]), np.concatenate([pc, np.full(5, 2, np.uint32), np.zeros(4, np.uint32)])
    pool = pool[4:]
    order = rng.permutation(len(pk))
    P.pairs = (pk[order], pc[order])
    high = P.high = base.copy()
    high.add_pairs(*P.pairs)
    assert np.array_equal(high.keys, base.keys)

    # erase: a third of the keys - per cluster its first and a middle key, whatever sits either side of every edge, in slot
    # 0 and in the table's last slot - and half of them added back
    home, slot = global_slots(P.layout, g)
    must = []
    for tag in P.cluster_at:
        must += [P.cluster_in[tag][0], P.cluster_in[tag][CLUSTER_IN // 2]]
    for s in [0, g.cap - 1] + [e - 1 for e in P.edges] + list(P.edges):
        must += high.keys[slot == s].tolist()
    for e in P.edges:  # one key that crossed the edge, one that stayed below it
        must += high.keys[(home < e) & (slot >= e)][:1].tolist() + high.keys[(home < e) & (slot < e) & (home >= e - BELOW)][:1].tolist()
    must = np.unique(np.array(must, np.uint64))
    n_gone = high.size // 3
    gone = np.concatenate([must, rng.choice(np.setdiff1d(high.keys, must), n_gone - len(must), replace=False)])
    P.erase_must, P.gone = must, gone[rng.permutation(len(gone))]
    back = np.concatenate([must[::2], rng.choice(np.setdiff1d(gone, must), n_gone // 2 - len(must[::2]), replace=False)])
    P.back = (back, counts_for(rng, len(back)))
    keep = ~np.isin(high.keys, gone)
    P.erased = tm.Model(k, high.keys[keep], high.counts[keep])
    P.erased_back = P.erased.copy()
    P.erased_back.add_pairs(*P.back)

    # what the readers take: profile reads (the genome's, cluster keys' paths, absent keys), a partner of the small shape
    prof = sample_reads(rng, genome, 14, k, 0.01) + [b"", b"ACGTN" * 9] + P.path_reads[::16]
    prof += tg.reads_of(np.concatenate([clusters_in[::7], P.absent[:12]]), np.ones(len(clusters_in[::7]) + 12, np.int64), k, rng)
    P.seqs = {"profile": prof}
    P.csr = {"profile": to_csr(prof), "high": to_csr(P.high_reads), "half0": to_csr(P.half_reads[0]), "half1": to_csr(P.half_reads[1])}
    half = rng.choice(base.keys, 1500, replace=False)
    pkeys = np.unique(np.concatenate([half, pool[:1000]] + [c[CLUSTER_IN - 3:CLUSTER_IN + 2] for c in P.clusters.values()]))
    P.partner = tm.Model(k)
    P.partner.add_pairs(pkeys, rng.integers(1, 8, size=len(pkeys)).astype(np.uint32))
    P.partner_request = SMALL_REQUEST
    P.cluster = every_cluster  # (what lookup_keys appends to its keys)
    return P


def check_plan(P):
    """what the GPU tests rest on, by table_model.layout alone: for every edge the slots edge - 1 and edge are taken and 8
    keys or more have home < edge <= slot; 8 keys or more wrapped in range 0 and in the last range; the table's last slot
    is taken; no range is above 0.9; the filled ranges are at 0.85; counts 1 .. 300; the absent keys are absent, 8 or more
    of them homed within 8 slots of every edge; the erase set holds the keys at the edges; the reads spell the content"""
    g, k, rs, L = P.g, P.k, P.g.range_slots, P.layout
    home, slot = global_slots(L, g)
    taken = set(slot.tolist())
    assert len(taken) == P.base.size
    for e in P.edges:
        assert e - 1 in taken and e in taken, e
        crossed = int(((home < e) & (slot >= e)).sum())
        assert crossed >= 8, (e, crossed)
        assert (L.range[(home < e) & (slot >= e)] == e // rs).all()
    last = g.n_ranges - 1
    for r in (0, last):
        assert int((L.wrapped & (L.range == r)).sum()) >= 8, r
    assert g.cap - 1 in taken and 0 in taken
    assert L.fill.max() <= 0.9 * rs, L.fill.max()
    for r in P.filled:
        assert 0.85 * rs <= L.fill[r] <= 0.9 * rs, (r, L.fill[r])
    assert sorted(P.filled) == sorted({0, last} | {e // rs for e in P.edges})
    for tag, (r, lo, hi) in P.cluster_at.items():
        rr, pp = tm.home_of(P.clusters[tag], k, g)
        assert (rr == r).all() and (pp >= lo).all() and (pp <= hi).all() and len(np.unique(P.clusters[tag])) == CLUSTER, tag
        assert P.base.count(P.cluster_in[tag]).all() and not P.base.count(P.cluster_out[tag]).any(), tag
        assert np.isin(P.cluster_out[tag], P.absent).all()
    assert P.base.counts.min() == 1 and P.base.counts.max() >= 300 and len(np.unique(P.base.counts)) > 50
    assert P.base.counts.max() < 2000 and (P.base.count(P.edge_keys) < 200).all()
    assert np.array_equal(P.high.count(P.edge_keys), np.array([255, 256, tg.U32] * 3, np.uint32))
    assert not P.high.count(P.pairs[0][P.pairs[1] == 0]).any() and int((P.pairs[1] == 0).sum()) == 4
    if P.variant == 0:
        if P.name != "E":  # the small table of the same content has room, range by range
            small = tm.geometry(FILE_REQUEST, k)
            assert (small.cap, small.range_slots) == (FILE_SLOTS, 8192) and P.base.size <= 0.6 * FILE_SLOTS, P.base.size
            if P.name == "B":
                assert tm.layout(P.base.keys, k, small).fill.max() <= 0.9 * small.range_slots
        r_all = np.unique(L.range)
        assert len(r_all) > 5000  # the graph's k-mers are homed all over the table
    assert not P.base.count(P.absent).any() and len(np.unique(P.absent)) == len(P.absent) >= 2000
    ah, _ = global_slots(tm.layout(P.absent[:200], k, g), g)
    for e in P.edges:
        assert int((np.abs(ah - e) <= BELOW).sum()) >= 8, e
    # the erase set
    assert abs(len(P.gone) / P.base.size - 1 / 3) < 0.01 and len(np.unique(P.gone)) == len(P.gone)
    assert np.isin(P.erase_must, P.gone).all() and np.isin(P.back[0], P.gone).all() and abs(len(P.back[0]) / len(P.gone) - 0.5) < 0.01
    for s in [0, g.cap - 1] + [e - 1 for e in P.edges] + list(P.edges):
        assert np.isin(P.base.keys[slot == s], P.gone).all()
    # the reads spell the content, the halves add up to it
    got = tg.model_of_reads(k, P.high_reads)
    assert np.array_equal(got.keys, P.base.keys) and np.array_equal(got.counts, P.base.counts)
    halves = [tg.model_of_reads(k, h) for h in P.half_reads]
    both = halves[0].copy()
    both._merge(halves[1].keys, halves[1].counts)
    assert np.array_equal(both.keys, P.base.keys) and np.array_equal(both.counts, P.base.counts)
    for tag in P.cluster_at:
        assert halves[0].count(P.cluster_in[tag]).any() and halves[1].count(P.cluster_in[tag]).any()
    assert P.partner.size <= 0.7 * SMALL_SLOTS
    if P.variant == 0:  # a bulk build from the reads stays paged and level 2 gets fixed room: the fullest level-1 bucket fits
        b1, b2 = split_bits(g.n)
        bases = int(P.csr["high"][1][-1])
        max_keys = (bases + 8191) // 8192 * 8192
        room1 = (max_keys // (1 << b1) + max_keys // (1 << b1) // 8 + 16 * 256 + 255) // 256 * 256
        load = np.bincount(L.range >> b2, weights=P.base.counts.astype(np.float64), minlength=1 << b1)
        assert load.max() <= 0.9 * room1, (load.max(), room1)
        assert (1 << b2, level2_of(max_keys, g.n, 8)) == {"A": (128, "fast"), "B": (512, "swwc"), "E": (1024, "swwc")}[P.name]
    return {"keys": P.base.size, "reads": len(P.high_reads), "bases": int(P.csr["high"][1][-1])}


# ---- the direct-addressed shapes -----------------------------------------------------------------------------------------------------

WINDOW = 64


@functools.lru_cache(maxsize=None)
def direct_plan(name):
    from kmertools_amd.device import to_csr
    P = Plan()
    request, k, n, _, cap = SHAPES[name]
    P.name, P.request, P.k = name, request, k
    g = P.g = geometry(name)
    assert cap == 4 ** k and n == 2 * k
    rng = np.random.default_rng([sum(name.encode()), 21])
    P.edges = edges_of(name)
    slots = [np.arange(0, WINDOW), np.arange(cap - WINDOW, cap)] + [np.arange(e - WINDOW, e + WINDOW) for e in P.edges]
    slots.append(rng.integers(0, cap, size=4000))
    slots = np.unique(np.concatenate(slots)).astype(np.uint64)
    words = tm.hash_inverse(slots, k)
    canon = words <= gr.rc_np(words, k)
    P.slots, keys = slots[canon], words[canon]
    counts = counts_for(rng, len(keys))
    genome = genome_of(rng, 3000)
    P.reads = sample_reads(rng, genome, 60, k, 0.01) + tg.reads_of(keys, counts, k, rng)
    P.reads = [P.reads[i] for i in rng.permutation(len(P.reads))]
    P.csr = to_csr(P.reads)
    P.model = tg.model_of_reads(k, P.reads)
    P.steered = keys
    # absent: the canonical words of other slots, those between the steered ones at the edges among them
    other = np.setdiff1d(rng.integers(0, cap, size=3000).astype(np.uint64), slots)
    aw = tm.hash_inverse(np.concatenate([slots[~canon], other]), k)
    aw = gr.canon_np(aw, k)
    P.absent = np.setdiff1d(aw, P.model.keys)
    return P


def check_direct_plan(P):
    """the slot is the home: every steered key's home is the slot it was built for; both sides of every edge, the first
    and the last slots of the table hold keys"""
    g, k = P.g, P.k
    r, p = tm.home_of(P.steered, k, g)
    assert g.m8 == 8 and np.array_equal(r * 8192 + p, P.slots.astype(np.int64))
    assert P.model.count(P.steered).all() and not P.model.count(P.absent).any() and len(P.absent) > 2000
    L = tm.layout(P.model.keys, k, g)
    assert not L.displacement.any()  # (a bijection: nothing ever probes)
    home = set((L.range * 8192 + L.home).tolist())
    for lo, hi in [(0, WINDOW), (g.cap - WINDOW, g.cap)] + [(e - WINDOW, e) for e in P.edges] + [(e, e + WINDOW) for e in P.edges]:
        assert sum(s in home for s in range(lo, hi)) >= 16, (lo, hi)
    assert int(P.model.counts.max()) >= 300 and P.model.size > 2000
    return {"keys": P.model.size, "reads": len(P.reads)}
