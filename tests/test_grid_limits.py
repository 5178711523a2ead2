"""Every GPU entry point of Context and Counter with the context's grids held to a few workgroups.

Almost every launch is sized min(work, CUs * a small factor) and its kernel strides over the work by gridDim.x.  On the card
the cap is some 2048 workgroups, the suite's inputs are smaller than that, so nearly every grid-stride loop of the library
is gone round exactly once by the other tests.  Here the context's workgroup budget is lowered (Context.cu_limit: 1 CU = 8
workgroups at the usual factor, 3 CUs = 24, a stride that is a multiple of no tile size) and every entry point is compared
with the reference its own test file uses, exactly, under that file's canonicalisation - on inputs that give every strided
loop at least three full trips and a ragged last one at limit 1.  Where the order of an output is defined, the limited run's
arrays are also the unlimited run's byte for byte.

The sizes are fixed here and proved from the offsets and counts alone, without a GPU (sizes()): a batch of 31 segments of
8192 bases, 1201 reads, tables of 8 ranges with 34 816 entries, key arrays of more than 6144 elements that are no multiple
of 2048, more than 6144 unitigs, profiles of short, middle and long sequences for the three forms of kt_profile_stats, more
than 24 sketch groups, 30 x 30 sketch pairs.  Where the one table's content leaves a loop with fewer trips, sizes() says so
with the number and an input of its own follows: a link graph of 12 498 links (the per-link kernels), a table of 7000 het
pairs (het_gather_kernel), a dense table of 64 ranges (the walkers of the dense form), 26 long profile sequences
(long_select_kernel).

CASES is the table: name -> (the call and its comparison, the methods of device.py it goes through).  A test compares it
with the public methods of the two classes; the few that launch nothing are listed in EXCLUDED with the reason."""
import contextlib
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import card_ref  # noqa: E402
import component_ref as cr  # noqa: E402
import ktab_ref  # noqa: E402
import read_batches as rb  # noqa: E402
import scaled_ref as sr  # noqa: E402
import table_geometries as tg  # noqa: E402
import test_correct as tc  # noqa: E402
import test_gpu_parity as tgp  # noqa: E402
import test_profile as tp  # noqa: E402
import test_scaled_sketch as tss  # noqa: E402
import test_sketch as ts  # noqa: E402
import test_table_geometries as tgeo  # noqa: E402
import test_table_lifecycle as lc  # noqa: E402
import test_unitig_components as tuc  # noqa: E402
import thread_ref as thr  # noqa: E402
import tip_ref as tr  # noqa: E402
import bubble_ref as br  # noqa: E402
import count_edges as ce  # noqa: E402
import unitig_link_ref as lr  # noqa: E402
from test_table_lifecycle import by_key, same  # noqa: E402

LIMITS = (1, 3)
U32 = 0xFFFFFFFF
NO = 0xFFFFFFFF
SEG = 8192            # bases per workgroup of a read walk (kt_segment.hpp)
PER_CU = 8            # workgroups per CU of the usual grid (ktl::grid_for's callers)
FLAT = PER_CU * 256   # items a flat kernel takes per trip at limit 1
SEED = 0x6719
N_READS = 1200
N_SPELLED = 5500
K = 21                # the read walks that need no table
REQUEST, TK = 40000, 31   # the table: 8 ranges of 5120 slots, load 0.85 (tests/table_geometries.py)
WALK_PER_CU = 4       # workgroups per CU of a table walk (kt_ctr.hip launch_walk), of het_scan_kernel and het_verify_kernel
WALK_UNROLLS = (2, 4, 8)   # kt_ctr.hip: GRAPH_UNROLL; SPEC_, HET_, SCALED_UNROLL; CMP_ and SET_UNROLL
SHORT_MAX, MID_MAX, CHUNK = 256, 2048, 16384   # kt_profile.hip: the three forms of kt_profile_stats, a long sequence's chunk


# ---- the inputs, made once, and the proof of their sizes ---------------------------------------------------------------------

def n_seg(total):
    return (total + SEG - 1) // SEG


def trips_ok(n, per_trip, what):
    """at limit 1 a loop over n items, per_trip of them a trip, takes three full trips at least and a ragged last one;
    at limit 3 (three times the items a trip) the last trip is ragged too"""
    assert n >= 3 * per_trip + 1 and n % per_trip != 0 and n % (3 * per_trip) != 0, (what, n, per_trip)


@functools.lru_cache(maxsize=None)
def reads():
    """read_batches.noisy_reads at about 30 segments: empty reads, reads shorter than k, N runs, a 9000- and an 8192-base
    read, a tail off every 16-byte boundary"""
    return rb.Batch("grid", rb.noisy_reads(SEED, N_READS))


@functools.lru_cache(maxsize=None)
def letter_reads():
    """the same offsets, every byte kt_cgr_points refuses turned into a letter"""
    b = reads()
    bases = np.where(np.isin(b.bases, rb.LETTERS), b.bases, np.uint8(ord("A"))).astype(np.uint8)
    return rb.Batch.of_lens("grid_letters", bases, b.lens)


@functools.lru_cache(maxsize=None)
def plan():
    """table_geometries.plan(40000, 31) with a profile batch of read-walk size: the noisy reads (their k-mers are not the
    table's) around the reads the table's graph was grown from and 5500 reads of one k-mer of the table each (a run of
    kt_thread_runs each).  A copy: the cached plan is left as it is."""
    import copy
    from kmertools_amd.device import to_csr
    P = tg.plan(REQUEST, TK)
    Q = copy.copy(P)
    Q.__dict__.pop("refs", None)
    b = reads()
    prof = b.seqs[:b.n // 2] + list(P.graph_reads) + list(P.spelled_reads[:N_SPELLED]) + b.seqs[b.n // 2:]
    Q.seqs = {"profile": prof}
    Q.csr = dict(P.csr, profile=to_csr(prof))
    return Q


@functools.lru_cache(maxsize=None)
def refs():
    P = plan()
    return {name: tgeo.ref_of(P, name) for name in ("base", "high", "erased")}


@functools.lru_cache(maxsize=None)
def dense_ref():
    return lc.Ref(dense_plan()["model"])


class Stub:
    """what the reference-side helpers of test_table_geometries.py read of a rig, for use without a GPU"""
    def __init__(self, P):
        self.P, self.k = P, P.k


@functools.lru_cache(maxsize=None)
def graph():
    """the high content as strings, its unitigs and links (unitig_link_ref), the unitigs as arrays, the links as arrays"""
    table, us, ls = tgeo.graph_strings(Stub(plan()), refs()["high"])
    ub, uo = thr.csr([u[0] for u in us])
    lo, lt = lr.as_arrays(ls)
    return {"table": table, "us": us, "ls": ls, "ub": ub, "uo": uo, "usum": np.array([u[1] for u in us], np.uint64).reshape(-1),
            "loff": lo, "lto": lt}


@functools.lru_cache(maxsize=None)
def thread_inputs():
    """the profile batch's hits on the index of the high content's unitigs, their runs, the components: all the references'"""
    P, g = plan(), graph()
    qb, qo = P.csr["profile"]
    hits = thr.hits_np(thr.index_np(g["ub"], g["uo"], TK), qb, qo, TK)
    runs = thr.runs_np(hits, qo, g["uo"], TK)
    comps = cr.components(g["loff"], g["lto"], g["uo"], g["usum"], TK)
    return {"hits": hits, "runs": runs, "comps": comps}


@functools.lru_cache(maxsize=None)
def stats_profile():
    """a synthetic profile for kt_profile_stats: short sequences (one wave each, 32 a trip at limit 1), 70 middle ones
    (20 a trip), 26 long ones: three of 9, 17 and 26 chunks (long_hist_kernel takes 8 chunks a trip in x at limit 1 and
    one sequence a trip in y) and 23 of one chunk, so that long_select_kernel, one workgroup per long sequence, takes three
    trips of 8 and one of 2 at limit 1, one of 24 and one of 2 at limit 3"""
    rng = np.random.default_rng(SEED + 1)
    lens = [int(x) for x in rng.integers(0, SHORT_MAX + 1, size=130)] + [0, 1, SHORT_MAX, SHORT_MAX]
    lens += [int(x) for x in rng.integers(SHORT_MAX + 1, MID_MAX + 1, size=68)] + [SHORT_MAX + 1, MID_MAX]
    lens += [8 * CHUNK + 5, 16 * CHUNK + CHUNK // 2, 26 * CHUNK]
    lens += [int(x) for x in rng.integers(MID_MAX + 1, 6000, size=21)] + [MID_MAX + 1, CHUNK]
    order = rng.permutation(len(lens))
    lens = np.array(lens, np.int64)[order]
    offsets = np.zeros(len(lens) + 1, np.uint64)
    offsets[1:] = np.cumsum(lens)
    total = int(offsets[-1])
    prof = rng.integers(0, 6, size=total).astype(np.uint32)
    big = rng.random(total) < 0.02
    prof[big] = rng.integers(0, 1 << 32, size=int(big.sum()), dtype=np.uint64).astype(np.uint32)
    prof[rng.random(total) < 0.1] = NO
    return prof, offsets, lens


@functools.lru_cache(maxsize=None)
def sketch_sets():
    """the distinct hashes of the first 120 reads' k-mers (test_sketch.hash_sets): rows that are empty, short and full"""
    from oracle import kt_oracle
    b = reads()
    return ts.hash_sets(kt_oracle, b.bases, b.offsets[:121], K, 7)


GROUPS = [0, 0, 1, 1] + list(range(4, 100, 3)) + [100, 100, 118, 120]   # groups of no, one and several rows
PAIR_S = 64


@functools.lru_cache(maxsize=None)
def scaled_rows():
    """scaled = 1 rows of 30 reads and, as test_scaled_sketch.py builds it, one of a 40 kb sequence: more than an LDS tile"""
    from oracle import kt_oracle
    b = reads()
    rows = sr.read_rows(kt_oracle, b.bases, b.offsets[:121], K, 1, 3)
    rng = np.random.default_rng(31)
    seq = tss.ACGT[rng.integers(0, 4, size=40_000)]
    (_, long_row, _), = sr.read_rows(kt_oracle, seq, np.array([0, len(seq)], np.uint64), K, 1, 3)
    return rows, long_row


@functools.lru_cache(maxsize=None)
def link_graph():
    """9001 unitigs, most of them linked to an earlier one nearby - a third of the links with their mirror, some twice, some
    to the unitig itself - and every 40th to none: chains of a few dozen unitigs among single ones"""
    rng = np.random.default_rng(SEED + 2)
    n = 9001
    links = {}
    for i in range(1, n):
        if i % 40 == 0:
            continue
        j = int(rng.integers(max(0, i - 3), i)) if i % 7 else i
        links.setdefault(2 * i + (i & 1), []).append(2 * j)
        if i % 3 == 0:
            links.setdefault(2 * j + 1, []).append(2 * i + ((i & 1) ^ 1))
        if i % 11 == 0:
            links.setdefault(2 * i + ((i & 1) ^ 1), []).append(2 * j + 1)
    loff, lto = tuc.arrays((n, links))
    uoff = np.zeros(n + 1, np.uint64)
    uoff[1:] = np.cumsum(rng.integers(TK, 400, size=n))
    usum = rng.integers(1, 1 << 40, size=n).astype(np.uint64)
    want = cr.components(loff, lto, uoff, usum, TK)
    cr.check_labels(loff, lto, want["component"])
    return {"n": n, "loff": loff, "lto": lto, "uo": uoff, "usum": usum, "want": want}


@functools.lru_cache(maxsize=None)
def het_content():
    """7000 random canonical k-mers and, of each, the k-mer with one base substituted: about 7000 het pairs"""
    import table_model as tm
    rng = np.random.default_rng(SEED + 3)
    a = tm.canonical_keys(rng, TK, 7000)
    pos = rng.integers(0, TK, size=len(a)).astype(np.uint64)
    b = tm.gr.canon_np(a ^ (rng.integers(1, 4, size=len(a)).astype(np.uint64) << (np.uint64(2) * pos)), TK)
    keys = np.unique(np.concatenate([a, b]))
    m = tm.Model(TK, keys, rng.integers(1, 60, size=len(keys)).astype(np.uint32))
    return {"model": m, "want": tgeo.hr.restate(m.keys, m.counts, TK)}


DENSE_REQUEST = 300000   # 64 ranges of 5120 slots


@functools.lru_cache(maxsize=None)
def dense_plan():
    """1200 synthetic reads of 150 bases for a fresh bulk build into a table of 64 ranges, which it leaves dense"""
    import table_model as tm
    from oracle import kt_oracle
    bases, offsets = kt_oracle.synth_reads(SEED, 1200, 150, noise=True)
    m = tm.Model(TK)
    m.add_reads(bases, offsets)
    return {"csr": (bases, offsets), "model": m, "g": tm.geometry(DENSE_REQUEST, TK)}


@functools.lru_cache(maxsize=None)
def sizes():

    """every size precondition, from offsets and counts alone"""
    b, P, g = reads(), plan(), graph()
    # the read walks: one workgroup per segment
    for name, total in (("reads", b.total), ("profile batch", int(P.csr["profile"][1][-1])), ("high reads", int(P.csr["high"][1][-1]))):
        trips_ok(n_seg(total), PER_CU, name)
    assert (b.lens[:8] == (0, 1, 2, 31, 64, 0, 9000, 8192)).all() and b.total % 16 != 0
    # the wave-per-read kernels: 8 workgroups of 4 waves a trip
    for name, n in (("reads", b.n), ("profile batch", len(P.csr["profile"][1]) - 1)):
        trips_ok(n, PER_CU * 4, name)
    prof, offsets, lens = stats_profile()
    trips_ok(len(lens), PER_CU * 4, "kt_profile_stats' sequences")
    assert int(((lens > SHORT_MAX) & (lens <= MID_MAX)).sum()) >= 70    # stats_wave_kernel<true>: 5 * 4 waves a trip
    long_ = lens[lens > MID_MAX]
    assert int((long_ > PER_CU * CHUNK).sum()) >= 3                      # long_hist_kernel: more chunks than the x grid
    trips_ok(len(long_), PER_CU, "long sequences")                       # long_select_kernel, long_hist_kernel's y loop
    # the table: four ranges or more (the bulk job takes it), flat kernels over its entries and key arrays
    assert P.g.n_ranges >= 4 and tg.bulk_eligible(P.request)
    n = P.base.size
    for name, m in (("add_pairs, first call", n - 100), ("add_pairs, second call", 100 + len(P.pairs[0])), ("erase", len(P.gone) + 9),
                    ("lookup", P.high.size + len(P.absent)),
                    ("thread_runs' hits", len(thread_inputs()["hits"]))):
        trips_ok(m, FLAT, name)
    # the table walkers over the probing image (kt_ctr.hip launch_walk): 4 workgroups per CU over tiles of 256 x the
    # kernel's unroll slots.  The table has 5 * 2^13 slots, so at limit 1 (4 workgroups) every walker takes a whole number
    # of trips, 5 at least; the ragged last trip comes at limit 3 (12 workgroups)
    for unroll in WALK_UNROLLS:
        tiles = -(-P.g.cap // (256 * unroll))
        assert tiles >= 3 * WALK_PER_CU + 1 and tiles % WALK_PER_CU == 0 and tiles % (3 * WALK_PER_CU) != 0, (unroll, tiles)
    # ... and over the dense form, four ranges a workgroup: the 8 ranges of this table are 2 workgroups at every limit,
    # one trip.  dense_plan()'s table has 64 ranges: four whole trips at limit 1, one and a ragged one at limit 3
    assert -(-P.g.n_ranges // 4) == 2
    D = dense_plan()
    assert D["g"].n_ranges == 64 and -(-D["g"].n_ranges // 4) == 4 * WALK_PER_CU and (D["g"].n_ranges // 4) % (3 * WALK_PER_CU) != 0
    assert D["model"].size < 0.7 * D["g"].cap and D["model"].occurrences >= D["g"].cap // 8
    # the per-unitig and per-link kernels
    nu = len(g["us"])
    trips_ok(nu, FLAT, "unitigs")
    # most unitigs of this content are single random k-mers: its graph has some 900 links, so the kernels that take one
    # thread per LINK (link_source_kernel, hook_kernel) make one ragged trip on it at every limit.  link_graph() is for
    # them: a graph of its own with three full trips of links and a ragged one
    assert 500 < len(g["lto"]) < FLAT
    L = link_graph()
    trips_ok(len(L["lto"]), FLAT, "the link graph's links")
    trips_ok(L["n"], FLAT, "the link graph's unitigs")
    assert 100 < len(L["want"]["stats"]) < L["n"] // 2 and int(L["want"]["tally"][2]) > 20
    # the het pairs: the high content has 2684 (het_gather_kernel: one full trip and a ragged one at limit 1, one trip at
    # limit 3); het_content() has three full trips of pairs and a ragged one.  het_scan_kernel and het_verify_kernel take
    # 4 workgroups per CU over the nodes and the candidates: 1024 a trip at limit 1
    assert FLAT < len(refs()["high"].memo("hetmers", lambda: tgeo.hr.restate(P.high.keys, P.high.counts, TK)).a) < 2 * FLAT
    H = het_content()
    trips_ok(len(H["want"].a), FLAT, "het pairs")
    trips_ok(H["model"].size, WALK_PER_CU * 256, "het nodes")
    assert sum(1 for fs in g["ls"] if len(fs) > 1) > 100, "branching ends"
    ti = thread_inputs()
    assert len(ti["runs"]["run_len"]) > 3 * FLAT and int(ti["runs"]["tally"][1]) > 10000
    assert len(ti["comps"]["stats"]) > 3 * FLAT
    # sketches: more groups than 24, some empty; 30 x 30 pairs against limit 1's 8 x 1 grid
    assert len(GROUPS) - 1 > 3 * PER_CU and (len(GROUPS) - 1) % PER_CU != 0 and sum(a == b_ for a, b_ in zip(GROUPS, GROUPS[1:])) >= 3
    assert GROUPS[-1] == len(sketch_sets())
    rows, long_row = scaled_rows()
    assert len(long_row) > 2 * 16384 and len(rows) == 120
    return True


def test_the_sizes_give_every_loop_three_trips_and_a_ragged_one(oracle):
    assert sizes()


# ---- the seam ------------------------------------------------------------------------------------------------------------------

def test_cu_limit_without_a_context(monkeypatch):
    """What can be tested without a device, where no kt_ctx can be made: of the library, that a null context is KT_ERR_ARG,
    named as the other entry points name it; of Context.cu_limit, that it puts the value from before back, also on an
    exception - against a stand-in that records the calls.  That 0 restores and that a limit above the device's count is
    clamped is the library's arithmetic: test_cu_limit_on_a_context checks it on a real context (the stand-in only copies
    it so that cu_count has something to report)."""
    import ctypes
    from kmertools_amd import _lib, device
    L = _lib.lib()
    assert L.kt_ctx_set_cu_limit(None, 3) == _lib.KT_ERR_ARG and _lib.last_error() == "kt_ctx_set_cu_limit: null ctx"
    assert L.kt_ctx_cu_limit(None, None, None) == _lib.KT_ERR_ARG and _lib.last_error() == "kt_ctx_cu_limit: null ctx"

    class Fake:
        dev, cur, calls = 256, 256, []

        def kt_ctx_set_cu_limit(self, h, n):
            self.calls.append(n)
            self.cur = self.dev if n == 0 or n > self.dev else n
            return 0

        def kt_ctx_cu_limit(self, h, a, b):
            for ref, v in ((a, self.cur), (b, self.dev)):
                ctypes.cast(ref, ctypes.POINTER(ctypes.c_uint32))[0] = v
            return 0

    fake = Fake()
    ctx = device.Context.__new__(device.Context)
    ctx._h = None
    monkeypatch.setattr(_lib, "lib", lambda: fake)
    with ctx.cu_limit(3):
        assert ctx.cu_count() == (3, 256)
        with pytest.raises(RuntimeError):
            with ctx.cu_limit(1):
                assert ctx.cu_count() == (1, 256)
                raise RuntimeError("inside")
        assert ctx.cu_count() == (3, 256)
        with ctx.cu_limit(1000):
            assert ctx.cu_count() == (256, 256)
        assert ctx.cu_count() == (3, 256)
    assert ctx.cu_count() == (256, 256) and fake.calls == [3, 1, 3, 1000, 3, 0]


@pytest.mark.gpu
def test_cu_limit_on_a_context():
    """no kernel is launched: 0 after a limit restores the device's count, a limit above it is clamped to it"""
    from kmertools_amd import _lib, device
    ctx = device.Context(0)
    try:
        L = _lib.lib()
        n, dev = ctx.cu_count()
        assert n == dev >= 1
        for ask, want in ((3 if dev > 3 else 1, 3 if dev > 3 else 1), (0, dev), (dev + 1, dev), (1, 1), (U32, dev), (dev, dev)):
            assert L.kt_ctx_set_cu_limit(ctx._h, ask) == 0 and ctx.cu_count() == (want, dev), ask
        assert L.kt_ctx_cu_limit(ctx._h, None, None) == 0
        with pytest.raises(ZeroDivisionError):
            with ctx.cu_limit(1):
                assert ctx.cu_count() == (1, dev)
                1 // 0
        assert ctx.cu_count() == (dev, dev)
    finally:
        ctx.close()


# ---- the rig -------------------------------------------------------------------------------------------------------------------

class Env:
    """a context on a stream of its own for the calls with host arrays, test_table_geometries' rig (a context on torch's
    stream, the partner table) for the table's, and the table that holds the high content"""

    def __init__(self, torch, oracle):
        from kmertools_amd import device
        self.torch, self.oracle = torch, oracle
        self.hctx = device.Context(0)
        self.R = tgeo.Rig(torch, plan())
        self.P = self.R.P
        self.ref = refs()
        self.table = self.R.table()
        self.table.add_pairs_host(self.P.high.keys, self.P.high.counts)
        self.unlimited = {}
        self.mp = self.capfd = self.tmp = None

    @contextlib.contextmanager
    def limit(self, n):
        with self.hctx.cu_limit(n), self.R.ctx.cu_limit(n):
            yield

    def close(self):
        self.R.close()
        self.hctx.close()


@pytest.fixture(scope="module")
def env(oracle):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    assert sizes()
    e = Env(torch, oracle)
    yield e
    e.close()


CASES = {}


def case(name, *covers):
    def add(fn):
        CASES[name] = (fn, covers)
        return fn
    return add


def eq(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    bad = np.flatnonzero((got != want).reshape(-1))
    assert not len(bad), "%s: %d elements differ, the first at %d: got %s, expected %s" % (
        what, len(bad), bad[0], got.reshape(-1)[bad[0]], want.reshape(-1)[bad[0]])


# ---- Context: the read walks ----------------------------------------------------------------------------------------------------

@case("kmers", "Context.kmers", "Context.kmers_host")
def c_kmers(E):
    b = reads()
    wf, wr, we = E.ref["high"].memo("grid_kmers", lambda: rb.oracle_kmers_flat(E.oracle, b, K))
    gf, gr_, ge = E.hctx.kmers_host(b.bases, b.offsets, K)
    eq(ge, we, "end"), eq(gf, wf, "fwd"), eq(gr_, wr, "rev")
    return gf, gr_, ge


@case("route", "Context.route", "Context.route_host")
def c_route(E):
    """the oracle's canonical k-mers, each once, grouped by owner (the order inside a group is not defined)"""
    b, owners = reads(), 3
    f, r, _ = E.ref["high"].memo("grid_kmers", lambda: rb.oracle_kmers_flat(E.oracle, b, K))
    keys, counts = E.hctx.route_host(b.bases, b.offsets, K, owners)
    own = tc.owner_of(keys, owners)
    assert int(counts.sum()) == len(f) and same(own, np.repeat(np.arange(owners), counts.astype(np.int64)).astype(own.dtype))
    eq(np.sort(keys), np.sort(np.minimum(f, r)), "keys")
    return (counts,)


@case("minimisers", "Context.minimisers", "Context.minimisers_host")
def c_minimisers(E):
    b = reads()
    out = []
    for w, m in ((31, 7), (200, 15)):
        want = E.ref["high"].memo(("grid_min", w, m), lambda: rb.oracle_minimisers_flat(E.oracle, b, w, m))
        got = E.hctx.minimisers_host(b.bases, b.offsets, w, m)
        for g, x, name in zip(got, want, ("ev_offsets", "kmers", "starts", "ends")):
            eq(g, x, (name, w, m))
        out += list(got)
    return out


def oligo(E, k, count_min):
    b = reads()
    raw = E.ref["high"].memo(("grid_oligo", k, count_min, 0), lambda: E.oracle.oligo_batch(b.bases, b.offsets, k, count_min, False))
    nrm = E.ref["high"].memo(("grid_oligo", k, count_min, 1), lambda: E.oracle.oligo_batch(b.bases, b.offsets, k, count_min, True))
    g_u32 = E.hctx.oligo_host(b.bases, b.offsets, k, count_min, False, 1, "u32")
    g_f64 = E.hctx.oligo_host(b.bases, b.offsets, k, count_min, True, 1, "f64")
    eq(g_u32.astype(np.float64), raw, ("oligo counts", k, count_min))
    eq(g_f64.view(np.uint64), nrm.view(np.uint64), ("oligo f64", k, count_min))
    return g_u32, g_f64


@case("oligo_lds", "Context.oligo", "Context.oligo_host")
def c_oligo_lds(E):
    """k = 4 (the dense kernel), 5 and 7 (the tile kernels): histograms in LDS"""
    return [a for k, cm in ((4, True), (5, False), (7, True)) for a in oligo(E, k, cm)]


@case("oligo_generic", "Context.oligo", "Context.oligo_host")
def c_oligo_generic(E):
    """k outside 3..7: histograms in global memory"""
    return [a for k, cm in ((2, True), (1, False)) for a in oligo(E, k, cm)]


@case("cgr", "Context.cgr", "Context.cgr_host")
def c_cgr(E):
    b = letter_reads()
    want = E.ref["high"].memo("grid_cgr", lambda: E.oracle.cgr_batch(b.bases, b.offsets, 16))
    got = E.hctx.cgr_host(b.bases, b.offsets, 16)
    eq(got.view(np.uint64), want.view(np.uint64), "cgr")
    return (got,)


@case("card_add", "Context.card_add", "Context.card_host")
def c_card(E):
    b, p, seed = reads(), 10, 5
    wreg, wn = E.ref["high"].memo("grid_card", lambda: card_ref.registers(E.oracle, b.bases, b.offsets, K, p, seed))
    reg, n = E.hctx.card_host(b.bases, b.offsets, K, p, seed)
    assert n == wn
    eq(reg, wreg, "registers")
    return (reg,)


@case("sketch", "Context.sketch", "Context.sketch_host")
def c_sketch(E):
    b, s, seed = reads(), 16, 0x5eed
    want = E.ref["high"].memo("grid_sketch", lambda: ts.rows_of(ts.hash_sets(E.oracle, b.bases, b.offsets, K, seed), s))
    got = E.hctx.sketch_host(b.bases, b.offsets, K, s, seed)
    for g, w, name in zip(got, want, ("hashes", "sizes", "n_kmers")):
        eq(g, w, name)
    return got


@case("scaled_sketch", "Context.scaled_sketch", "Context.scaled_sketch_host")
def c_scaled_sketch(E):
    b, scaled, seed = reads(), 4, 9
    want = E.ref["high"].memo("grid_scaled", lambda: sr.csr(sr.read_rows(E.oracle, b.bases, b.offsets, K, scaled, seed)))
    got = E.hctx.scaled_sketch_host(b.bases, b.offsets, K, scaled, seed)
    for g, w, name in zip(got, want, ("hashes", "abunds", "row_offsets", "n_kmers")):
        eq(g, w, name)
    return got


@case("synth_reads", "Context.synth_reads")
def c_synth(E):
    """25 353 reads of 11 bases: the bases take 34 trips of 8192 at limit 1, the offsets three and a ragged one"""
    torch = E.torch
    n, L, seed, first = 3 * 8192 + 777, 11, 0x6b6d6572, 12345
    out = []
    for noise, genome in ((True, 0), (True, 5000)):
        bases = torch.empty(n * L, dtype=torch.uint8, device="cuda")
        offsets = torch.empty(n + 1, dtype=torch.int64, device="cuda")
        E.R.ctx.synth_reads(seed, n, L, bases, offsets, noise=noise, genome_len=genome, first_read=first)
        torch.cuda.synchronize()
        want, woff = E.ref["high"].memo(("grid_synth", genome), lambda: E.oracle.synth_reads(seed, n, L, noise=noise, genome_len=genome,
                                                                                          first_read=first))
        got, goff = bases.cpu().numpy(), offsets.cpu().numpy().astype(np.uint64)
        eq(got, want, "bases"), eq(goff, woff, "offsets")
        out += [got, goff]
    return out


@case("selftest_quotient", "Context.selftest_quotient")
def c_quotient(E):
    """one workgroup per divisor, 16 per CU: 300 divisors"""
    n, bad, chk = E.hctx.selftest_quotient(1, 300)
    assert n == sum(d + 1 for d in range(1, 301)) and bad == 0 and chk == tgp.quotient_checksum(1, 300)


# ---- Context: sketches' unions and pairs, profile statistics, the decision, runs and components --------------------------------------

@case("sketch_merge", "Context.sketch_merge")
def c_sketch_merge(E):
    sets, s = sketch_sets(), 16
    rows, sz, _ = ts.rows_of(sets, s)
    unions = [(0, np.unique(np.concatenate([sets[i][1] for i in range(a, b)] + [np.zeros(0, np.uint64)])))
              for a, b in zip(GROUPS, GROUPS[1:])]
    wh, wz, _ = ts.rows_of(unions, s)
    gh, gz = E.hctx.sketch_merge(rows, sz, np.array(GROUPS, np.uint64))
    eq(gz, wz, "sizes"), eq(gh, wh, "hashes")
    return gh, gz


@case("sketch_pairs", "Context.sketch_pairs", "Context.sketch_pairs_host")
def c_sketch_pairs(E):
    sets = sketch_sets()
    pick = [i for i, (_, h) in enumerate(sets) if len(h)][:28] + [i for i, (_, h) in enumerate(sets) if not len(h)][:2]
    assert len(pick) == 30
    ah, asz, _ = ts.rows_of([sets[i] for i in pick], PAIR_S)
    bh, bsz, _ = ts.rows_of([sets[i] for i in pick[::-1]], PAIR_S)
    ws, wd = E.ref["high"].memo("grid_pairs", lambda: ts.want_pairs(ah, asz, bh, bsz, PAIR_S))
    gs, gd = E.hctx.sketch_pairs_host(ah, asz, bh, bsz)
    eq(gs, ws, "shared"), eq(gd, wd, "denom")
    return gs, gd


@case("scaled_merge", "Context.scaled_merge")
def c_scaled_merge(E):
    rows, _ = scaled_rows()
    h, a, ro, _ = sr.csr(rows)
    want = sr.merge(h, a, ro, GROUPS)
    got = E.hctx.scaled_merge(h, a, ro, np.array(GROUPS, np.uint64))
    for g, w, name in zip(got, want, ("hashes", "abunds", "offsets")):
        eq(g, w, name)
    return got


@case("scaled_pairs", "Context.scaled_pairs", "Context.scaled_pairs_host")
def c_scaled_pairs(E):
    rows, long_row = scaled_rows()
    a_rows = [h for _, h, _ in rows if len(h)][:28] + [np.zeros(0, np.uint64), long_row]
    b_rows = [long_row[5::3].copy(), np.zeros(0, np.uint64)] + a_rows[2:]
    assert len(a_rows) == len(b_rows) == 30
    ah, ao = tss.csr_of(a_rows)
    bh, bo = tss.csr_of(b_rows)
    want = tss.want_shared(a_rows, b_rows)
    assert want[-1, -1] == len(long_row) and want[-1, 0] == len(long_row[5::3])
    got = E.hctx.scaled_pairs_host(ah, ao, bh, bo)
    eq(got, want, "shared")
    return (got,)


@case("profile_stats", "Context.profile_stats", "Context.profile_stats_host")
def c_profile_stats(E):
    prof, offsets, _ = stats_profile()
    want = E.ref["high"].memo("grid_stats", lambda: tp.want_stats(prof, offsets))
    got = E.hctx.profile_stats_host(prof, offsets)
    tp.assert_stats(got, want, "profile_stats")
    return [got[name] for name in tp.NAMES]


@case("correct_apply", "Context.correct_apply")
def c_correct_apply(E):
    """support words of every class over the noisy reads: per-read counts and the rewritten bases"""
    b = reads()
    sup = tc.pattern_support(np.random.default_rng(5), b.total, np.array([0, 1, 2, 3, 31, 254, 255]))
    out = []
    for ms, mc in ((1, 0), (2, 3)):
        want = tc.want_apply(b.bases, b.offsets, sup, ms, mc)
        got = tc.apply_host(E.hctx, b.bases, b.offsets, sup, ms, mc)
        tc.same(got, want, ("correct_apply", ms, mc))
        out += list(got)
    return out


@case("thread_runs", "Context.thread_runs", "Context.thread_runs_host")
def c_thread_runs(E):
    g, ti = graph(), thread_inputs()
    qo = plan().csr["profile"][1]
    nu = len(g["uo"]) - 1
    uh, ur_ = np.zeros(nu, np.uint64), np.zeros(nu, np.uint64)
    got = E.hctx.thread_runs_host(ti["hits"], qo, g["uo"], TK, uh, ur_)
    got["unitig_hits"], got["unitig_runs"] = uh, ur_
    names = ("run_offsets", "run_start", "run_len", "run_unitig", "run_upos", "unitig_hits", "unitig_runs", "tally")
    for name in names:
        eq(got[name], ti["runs"][name], name)
    return [got[name] for name in names]


@case("Context.unitig_components", "Context.unitig_components", "Context.unitig_components_host")
def c_components(E):
    g, ti = graph(), thread_inputs()
    got = E.hctx.unitig_components_host(g["loff"], g["lto"], g["uo"], g["usum"], TK)
    cr.check_labels(g["loff"], g["lto"], got["component"])
    tuc.same(got, ti["comps"], "unitig_components")
    return got["component"], got["stats"], got["tally"][:5]


@case("Context.unitig_components: a graph of many links", "Context.unitig_components", "Context.unitig_components_host")
def c_components_links(E):
    """link_source_kernel and hook_kernel, one thread per link: 6 trips of links and a ragged one at limit 1"""
    L = link_graph()
    got = E.hctx.unitig_components_host(L["loff"], L["lto"], L["uo"], L["usum"], TK)
    cr.check_labels(L["loff"], L["lto"], got["component"])
    tuc.same(got, L["want"], "the link graph")
    return got["component"], got["stats"], got["tally"][:5]


@case("thread_read_components", "Context.thread_read_components", "Context.thread_read_components_host")
def c_read_components(E):
    ti = thread_inputs()
    runs, comp = ti["runs"], ti["comps"]["component"]
    nc = len(ti["comps"]["stats"])
    w_reads, w_hits = np.zeros(nc, np.uint64), np.zeros(nc, np.uint64)
    want = cr.read_components(runs["run_unitig"], runs["run_len"], runs["run_offsets"], comp, nc, w_reads, w_hits)
    g_reads, g_hits = np.zeros(nc, np.uint64), np.zeros(nc, np.uint64)
    got = E.hctx.thread_read_components_host(runs["run_unitig"], runs["run_len"], runs["run_offsets"], comp, nc, g_reads, g_hits)
    assert int(want["tally"][0]) > 100 and int(want["tally"][1]) > 100
    for name in ("read_component", "read_mixed", "tally"):
        eq(got[name], np.asarray(want[name]).astype(got[name].dtype), name)
    eq(g_reads, np.asarray(w_reads, np.uint64), "comp_reads"), eq(g_hits, np.asarray(w_hits, np.uint64), "comp_hits")
    return got["read_component"], got["read_mixed"], got["tally"], g_reads, g_hits


# ---- Counter: the writers --------------------------------------------------------------------------------------------------------

def holds(c, m, what):
    gk, gc = c.export_host()
    assert c.size() == m.size, what
    eq(gk, m.keys, (what, "keys")), eq(gc, m.counts, (what, "counts"))
    return gk, gc


@case("add_pairs", "Counter.add_pairs", "Counter.add_pairs_host", "Counter.clear", "Counter.size", "Counter.export", "Counter.export_host")
def c_add_pairs(E):
    P = E.P
    lc.env_probing(E.mp)
    c = E.R.table()
    order = np.random.default_rng(5).permutation(P.base.size)
    k1, c1 = P.base.keys[order], P.base.counts[order]
    for round_ in range(2):   # (the second time into the cleared table)
        c.add_pairs_host(k1[:-100], c1[:-100])
        c.add_pairs_host(np.concatenate([k1[-100:], P.pairs[0]]), np.concatenate([c1[-100:], P.pairs[1]]))
        out = holds(c, P.high, "add_pairs")
        c.clear()
        assert c.size() == 0
    c.close()
    return out


@case("add_reads_probing", "Counter.add_reads_host", "Counter.add_reads_part")
def c_add_reads_probing(E):
    lc.env_probing(E.mp)
    c = E.R.table()
    c.add_reads_host(*E.P.csr["high"])
    out = holds(c, E.P.base, "add_reads, probing")
    c.close()
    return out


@case("add_reads_parts", "Counter.add_reads_part")
def c_add_reads_parts(E):
    """three hash partitions, one call each: together the whole batch"""
    lc.env_probing(E.mp)
    c = E.R.table()
    before = 0
    for part in range(3):
        c.add_reads_host(*E.P.csr["high"], n_parts=3, part=part)
        assert c.size() > before
        before = c.size()
    out = holds(c, E.P.base, "add_reads_part")
    c.close()
    return out


@case("add_reads_bulk", "Counter.add_reads")
def c_add_reads_bulk(E):
    """the bulk job (pack_segments / count_records, the partition passes, the dense range build); the walkers read the dense
    form, a prober images it, the walkers read the image"""
    c = tgeo.w_bulk_reads(E.R, E.P, E.mp, E.capfd)
    tgeo.check(E.R, c, E.ref["base"], tgeo.WALKERS, "dense")
    tgeo.check(E.R, c, E.ref["base"], ("lookup",) + tgeo.WALKERS, "imaged")
    out = holds(c, E.P.base, "add_reads, bulk")
    c.close()
    return out


@case("add_reads_bulk_merge", "Counter.add_reads")
def c_add_reads_bulk_merge(E):
    c = tgeo.w_bulk_merge(E.R, E.P, E.mp, E.capfd)
    out = holds(c, E.P.base, "add_reads, bulk, merged")
    c.close()
    return out


@case("export_target", "Counter.export_target")
def c_export_target(E):
    R, P = E.R, E.P
    n = P.base.size
    room = n + 9
    xk, xc = R.full(room + lc.GUARD, lc.KPAT, 64), R.full(room + lc.GUARD, lc.CPAT, 32)
    tgeo.env_bulk(E.mp)
    c = R.table()
    c.export_target(xk, xc, room)
    E.capfd.readouterr()
    tgeo.add_device(R, c, "high")
    tgeo.bulk_line(E.capfd, P, "export target", "build", "dense-ext")
    E.torch.cuda.synchronize()
    hk, hc = lc.u64(xk), lc.u32(xc)
    assert (hk[room:] == lc.KPAT).all() and (hc[room:] == lc.CPAT).all()
    gk, gc = by_key(hk[:n], hc[:n])
    eq(gk, P.base.keys, "keys"), eq(gc, P.base.counts, "counts")
    c.export_target(None, None, 0)
    out = holds(c, P.base, "target dropped")
    c.close()
    return out


@case("erase", "Counter.erase", "Counter.erase_device")
def c_erase(E):
    P = E.P
    lc.env_probing(E.mp)
    c = E.R.table()
    c.add_pairs_host(P.high.keys, P.high.counts)
    arg = np.concatenate([P.gone, P.gone[:7], np.array([2 ** 64 - 1, 4 ** TK], np.uint64)])
    assert len(arg) == len(P.gone) + 9
    assert c.erase(arg) == len(P.gone)
    out = holds(c, P.erased, "erase")
    assert not c.lookup_host(P.gone).any()
    c.close()
    return out


@case("table_files", "Counter.save", "Counter.add_file", "Counter.from_file")
def c_table_files(E):
    from kmertools_amd import device
    P, m = E.P, E.P.high
    path = str(E.tmp / "high.ktab")
    assert E.table.save(path) == m.size
    with open(path, "rb") as f:
        data = f.read()
    assert data == ktab_ref.encode(TK, m.keys, m.counts), "the saved file is not ktab_ref's"
    t = device.Counter.from_file(E.R.ctx, path, slots=REQUEST)
    try:
        out = holds(t, m, "from_file")
        assert t.add_file(path) == m.size
        twice = m.copy()
        twice.counts = np.minimum(m.counts.astype(np.uint64) * 2, U32).astype(np.uint32)
        keep = m.counts < 2 ** 31   # (past 0xFFFFFFFF occurrences the count is unspecified)
        gk, gc = t.export_host()
        eq(gk, m.keys, "keys after add_file"), eq(gc[keep], twice.counts[keep], "counts after add_file")
    finally:
        t.close()
    return out


# ---- Counter: the readers of test_table_lifecycle.py and test_table_geometries.py on the table that holds the high content -----

READER_COVERS = {
    "size": ("Counter.size",), "export_host": ("Counter.export_host", "Counter.export"), "export_device": ("Counter.export",),
    "stage_pieces": ("Counter.export_stage_range", "Counter.export_fetch"), "stage_2_5": ("Counter.export_stage_range", "Counter.export_fetch"),
    "spectrum_host": ("Counter.spectrum_into",), "spectrum_device": ("Counter.spectrum_into",),
    "compare(t, partner)": ("Counter.compare_into",), "compare(partner, t)": ("Counter.compare_into",),
    "intersect(t, partner)": ("Counter.setop",), "intersect(partner, t)": ("Counter.setop_device",),
    "xor(t, partner)": ("Counter.setop",), "xor(partner, t)": ("Counter.setop_device",),
    "lookup": ("Counter.lookup", "Counter.lookup_host"), "profile": ("Counter.profile",),
    "graph(1)": ("Counter.graph_device",), "graph(2)": ("Counter.graph_device",),
    "cov": ("Counter.cov", "Counter.cov_host"), "read_solidity": ("Counter.read_solidity", "Counter.read_solidity_host"),
    "correct_support": ("Counter.correct_support",), "hetmers": ("Counter.hetmers",),
    "unitigs+links": ("Counter.unitigs", "Counter.unitig_links"), "unitig_tips": ("Counter.unitig_tips",),
    "unitig_bubbles": ("Counter.unitig_bubbles",),
}
assert set(READER_COVERS) == set(tgeo.READERS)


def reader_case(name):
    def fn(E):
        tgeo.read(E.R, E.table, E.ref["high"], name, "the high content")
    return fn


for _name in tgeo.READERS:
    CASES["read: " + _name] = (reader_case(_name), READER_COVERS[_name])


@case("lookup_all", "Counter.lookup", "Counter.lookup_host")
def c_lookup_all(E):
    """every key of the table and the absent ones, shuffled: 17 trips and a ragged one at limit 1"""
    P = E.P
    keys = np.concatenate([P.high.keys, P.absent])
    keys = keys[np.random.default_rng(3).permutation(len(keys))]
    want = P.high.count(keys)
    got = E.table.lookup_host(keys)
    eq(got, want, "host")
    dk, out = E.R.dev(keys), E.R.full(len(keys) + 1, lc.CPAT, 32)
    E.table.lookup(dk, len(keys), out)
    E.torch.cuda.synchronize()
    d = lc.u32(out)
    eq(d[:-1], want, "device")
    assert d[-1] == lc.CPAT
    return (got,)


@case("setop", "Counter.setop", "Counter.setop_device")
def c_setop(E):
    """intersect, subtract, union and xor, sorted (the order is defined) and as the walk leaves them"""
    out = []
    for op in ("intersect", "subtract", "union", "xor"):
        wk, wc = E.ref["high"].memo(("grid_setop", op), lambda: E.P.high.setop(E.R.pm, op, "sum"))
        gk, gc = E.table.setop(E.R.partner, op, count="sum", sort=True)
        eq(gk, wk, (op, "keys")), eq(gc, wc, (op, "counts"))
        out += [gk, gc]
        uk, uc = by_key(*E.table.setop(E.R.partner, op, count="sum", sort=False))
        eq(uk, wk, (op, "unsorted, keys")), eq(uc, wc, (op, "unsorted, counts"))
    return out


@case("spectrum_and_compare", "Counter.spectrum", "Counter.compare")
def c_spectrum_compare(E):
    m = E.P.high
    hist, tot = E.table.spectrum(300, totals=True)
    wh, wt = m.spectrum(300)
    eq(hist, wh, "spectrum")
    assert tot == wt
    mat, totals = E.table.compare(E.R.partner, 300, 9, totals=True)
    wm, wtot = E.ref["high"].memo("grid_compare", lambda: m.compare(E.R.pm, 300, 9))
    eq(mat, wm, "compare")
    assert [totals[n] for n in E.table.COMPARE_TOTALS] == [int(x) for x in wtot]
    return hist, mat


@case("graph_host_and_hetmers_device", "Counter.graph", "Counter.hetmers_device")
def c_graph_hetmers(E):
    torch = E.torch
    wk, wi, wc, wcen = E.ref["high"].memo("graph1", lambda: E.P.high.graph(1, None))
    gk, gi, gc, cen = E.table.graph(census=True)
    eq(gk, wk, "graph keys"), eq(gi, wi, "graph info"), eq(gc, wc, "graph counts")
    eq(cen, wcen, "graph census")
    w = E.ref["high"].memo("hetmers", lambda: tgeo.hr.restate(E.P.high.keys, E.P.high.counts, TK))
    n = len(w.a)
    room = n + 3
    ka, kb = E.R.full(room, lc.KPAT, 64), E.R.full(room, lc.KPAT, 64)
    ca, cb = E.R.full(room, lc.CPAT, 32), E.R.full(room, lc.CPAT, 32)
    got = E.table.hetmers_device(ka, kb, ca, cb, room)
    torch.cuda.synchronize()
    assert got == n
    eq(lc.u64(ka)[:n], w.a, "hetmers a"), eq(lc.u64(kb)[:n], w.b, "hetmers b")
    eq(lc.u32(ca)[:n], w.ca, "hetmers ca"), eq(lc.u32(cb)[:n], w.cb, "hetmers cb")
    assert (lc.u64(ka)[n:] == lc.KPAT).all()
    return gk, gi, gc


@case("hetmers: many pairs", "Counter.hetmers")
def c_hetmers_many(E):
    """a table of some 7000 het pairs: het_gather_kernel's later trips, het_scan_kernel's and het_verify_kernel's"""
    H = het_content()
    lc.env_probing(E.mp)
    c = E.R.table()
    c.add_pairs_host(H["model"].keys, H["model"].counts)
    w = H["want"]
    a, b, ca, cb, cen = c.hetmers(census=True)
    eq(a, w.a, "a"), eq(b, w.b, "b"), eq(ca, w.ca, "counts a"), eq(cb, w.cb, "counts b")
    eq(cen[:len(w.census)], w.census, "census")
    ua, ub_ = c.hetmers(sort=False)[:2]
    order = np.argsort(ua, kind="stable")
    eq(ua[order], w.a, "unsorted, a"), eq(ub_[order], w.b, "unsorted, b")
    c.close()
    return a, b, ca, cb, cen


@case("dense walkers: 64 ranges", "Counter.add_reads")
def c_dense_walkers(E):
    """a fresh bulk build into a table of 64 ranges; the walkers read the dense form four ranges a workgroup: four trips at
    limit 1, one and a ragged one at limit 3"""
    D = dense_plan()
    tgeo.env_bulk(E.mp)
    c = E.R.counter(DENSE_REQUEST)
    assert c.capacity() == D["g"].cap
    bases, offsets = D["csr"]
    db, do = E.R.dev(bases), E.R.dev(offsets)
    E.capfd.readouterr()
    c.add_reads(db, do, len(offsets) - 1)
    E.torch.cuda.synchronize()
    lines = lc.bulk_lines(E.capfd)
    assert len(lines) == 1 and lines[0].split()[5] == "build" and lines[0].split()[-1] == "build=dense", lines
    tgeo.check(E.R, c, dense_ref(), tgeo.WALKERS, "dense, 64 ranges")
    out = holds(c, D["model"], "dense, 64 ranges")
    c.close()
    return out


@case("unitigs_on_device", "Counter.unitigs_device", "Counter.unitigs_linked_device", "Counter.unitig_tips_device",
      "Counter.unitig_bubbles_device")
def c_unitigs_device(E):
    """the unitig stages into device tensors: unitigs, links, tip and bubble marks, each sized by a counting call"""
    torch, g, t = E.torch, graph(), E.table
    us, ls = g["us"], g["ls"]
    nu, nb, nl = t.unitigs_linked_device(None, 0, None, None, None, 0, None, None, 0)
    assert (nu, nb, nl) == (len(us), len(g["ub"]), len(g["lto"]))
    bases = torch.empty(nb + 1, dtype=torch.uint8, device="cuda")
    offs, sums = torch.empty(nu + 1, dtype=torch.int64, device="cuda"), torch.empty(nu, dtype=torch.int64, device="cuda")
    flags = torch.empty(nu, dtype=torch.int32, device="cuda")
    lo, lt = torch.empty(2 * nu + 1, dtype=torch.int64, device="cuda"), torch.empty(nl, dtype=torch.int32, device="cuda")
    assert t.unitigs_linked_device(bases, nb, offs, sums, flags, nu, lo, lt, nl) == (nu, nb, nl)
    torch.cuda.synchronize()
    out = [bases.cpu().numpy()[:nb], lc.u64(offs), lc.u64(sums), lc.u32(flags), lc.u64(lo), lc.u32(lt)]
    eq(out[0], g["ub"], "bases"), eq(out[1], g["uo"], "offsets"), eq(out[2], g["usum"], "count sums")
    assert out[3].tolist() == [u[2] for u in us]
    eq(out[4], g["loff"], "link offsets"), eq(out[5], g["lto"], "link_to")
    b2 = torch.empty(nb + 1, dtype=torch.uint8, device="cuda")
    o2, s2, f2 = torch.empty_like(offs), torch.empty_like(sums), torch.empty_like(flags)
    got = t.unitigs_device(b2, nb, o2, s2, f2, nu)
    torch.cuda.synchronize()
    assert tuple(got)[:2] == (nu, nb)
    eq(b2.cpu().numpy()[:nb], g["ub"], "unitigs: bases"), eq(lc.u64(o2), g["uo"], "unitigs: offsets")
    eq(lc.u64(s2), g["usum"], "unitigs: sums"), eq(lc.u32(f2), out[3], "unitigs: flags")
    n, cs, circ = tgeo.shape_of(us)
    wt = E.ref["high"].memo("tips", lambda: (lambda m: (m, tr.tally_of(m, n)))(tr.marks_of(n, cs, circ, ls, TK)))
    wb = E.ref["high"].memo("bubbles", lambda: (lambda mb: (mb[0], br.tally_of(mb[0], n, cs, mb[1])))(br.marks_of(n, cs, circ, ls, 2 * TK)))
    for fn, (wm, wtally), arg in ((t.unitig_tips_device, wt, TK), (t.unitig_bubbles_device, wb, 2 * TK)):
        marks = torch.full((nu + 1,), 0x5A, dtype=torch.uint8, device="cuda")
        tally = torch.zeros(4, dtype=torch.int64, device="cuda")
        assert fn(marks, nu, tally, arg) == nu
        torch.cuda.synchronize()
        hm = marks.cpu().numpy()
        assert hm[:nu].tolist() == wm and hm[nu] == 0x5A and [int(x) for x in lc.u64(tally)] == wtally
        out.append(hm[:nu])
    return out


@case("Counter.unitig_components", "Counter.unitig_components")
def c_counter_components(E):
    got = E.table.unitig_components()
    want = thread_inputs()["comps"]
    assert got["n_unitigs"] == len(graph()["us"])
    tuc.same(got, want, "Counter.unitig_components")
    return got["component"], got["stats"]


@case("clip_tips", "Counter.clip_tips")
def c_clip_tips(E):
    c, ref, table, us, ls = tgeo.copy_of_high(E.R, E.mp)
    left, stats, _ = ref.memo("clip", lambda: tr.clip(table, TK, TK, 1, True))
    got = c.clip_tips(TK, 1, True)
    want = dict(zip(tr.STATS, stats[:6] + [1 - stats[6]]))
    assert {n: got[n] for n in want} == want and want["tips"] > 0 and want["isolated"] > 0, (got, want)
    gk, gc = c.export_host()
    assert ce.strings_of(gk, gc, TK) == left
    c.close()
    return gk, gc


@case("simplify", "Counter.simplify")
def c_simplify(E):
    c, ref, table, us, ls = tgeo.copy_of_high(E.R, E.mp)
    left, stats, _ = ref.memo("simplify", lambda: br.simplify(table, TK, TK, 2 * TK, 1, False))
    got = c.simplify(TK, 2 * TK, 1, False)
    want = dict(zip(br.STATS, list(stats[:9]) + [1 - stats[9]]))
    assert {n: got[n] for n in want} == want and want["tips"] > 0, (got, want)
    gk, gc = c.export_host()
    assert ce.strings_of(gk, gc, TK) == left
    c.close()
    return gk, gc


@case("index_and_thread_hits", "Counter.index_sequences", "Counter.index_sequences_host", "Counter.thread_hits",
      "Counter.thread_hits_host")
def c_index(E):
    g, ti = graph(), thread_inputs()
    qb, qo = E.P.csr["profile"]
    lc.env_probing(E.mp)
    t = E.R.table()
    assert t.index_sequences_host(g["ub"], g["uo"]) == E.P.high.size
    got = t.thread_hits_host(qb, qo)
    eq(got, ti["hits"], "hits")
    gk, _ = t.export_host()
    eq(gk, E.P.high.keys, "the index's keys")
    t.close()
    return (got,)


@case("Counter.scaled_sketch", "Counter.scaled_sketch")
def c_table_sketch(E):
    m = E.P.high
    out = []
    for lo, hi, scaled in ((1, None, 2), (2, 5, 1)):
        wh, wa, wt = sr.table_sketch(m.keys, m.counts, lo, U32 if hi is None else hi, scaled, 5)
        gh, ga, gt = E.table.scaled_sketch(scaled, lo, hi, 5)
        eq(gh, wh, "hashes"), eq(ga, wa, "abunds")
        assert gt == wt
        out += [gh, ga]
    return out


@case("cov_part", "Counter.cov_part")
def c_cov_part(E):
    """three hash partitions added into one array of u32 bin counts: the oracle's raw coverage histograms"""
    from kmertools_amd._lib import KT_MEM_HOST
    bases, offsets = E.P.csr["profile"]
    n = len(offsets) - 1

    def make():
        oc = E.oracle.Counter(1)
        oc.add_pairs(E.P.high.keys, E.P.high.counts)
        return oc.cov_batch(bases, offsets, TK, 3, 5, norm=False)
    want = E.ref["high"].memo("grid_cov_part", make)
    counts = np.zeros((n, 5), np.uint32)
    for part in range(3):
        E.table.cov_part(bases, offsets, n, 3, 5, counts, 3, part, KT_MEM_HOST)
    eq(counts, want.astype(np.uint32), "cov_part")
    return (counts,)


@case("correct_host", "Counter.correct_host", "Counter.profile_host", "Context.correct_apply")
def c_correct_host(E):
    """profile, support and the decision in one call: the restatements of test_correct.py chained the same way"""
    from oracle import kt_oracle
    bases, offsets = E.P.csr["profile"]
    ref = E.ref["high"]
    prof = tgeo.profile_want(E.R, ref)
    sup = ref.memo("support", lambda: tgeo.want_support(kt_oracle, bases, offsets, TK, ref.m, prof, *tgeo.SOLID))
    want = tc.want_apply(bases, offsets, sup, 1, 0)
    assert (want[0] != bases).any() and (want[1] > 0).sum() > 20
    got = E.table.correct_host(bases, offsets, tgeo.SOLID[0], tgeo.SOLID[1])
    tc.same(got, want, "correct_host")
    return got


# ---- the table of cases against the two classes ------------------------------------------------------------------------------------

EXCLUDED = {
    "Context.close": "destroys the context", "Context.sync": "waits for the stream", "Context.cu_count": "the seam's getter",
    "Context.cu_limit": "the seam itself (test_cu_limit_on_a_context)",
    "Context.alloc_placed": "allocates; launches only what its caller's probe launches",
    "Context.oligo_tuning": "sets a flag of the context", "Context.oligo_launch_info": "reads the context's measurements",
    "Counter.close": "destroys the table", "Counter.capacity": "reads a field of the table",
}


def public_methods():
    from kmertools_amd import device
    return {"%s.%s" % (cls.__name__, name) for cls in (device.Context, device.Counter)
            for name, v in vars(cls).items() if not name.startswith("_") and (callable(v) or isinstance(v, classmethod))}


def test_the_case_table_names_every_entry_point():
    covered = {m for _, covers in CASES.values() for m in covers}
    public = public_methods()
    assert not covered & set(EXCLUDED), covered & set(EXCLUDED)
    assert covered | set(EXCLUDED) == public, ("without a case: %s; no such method: %s" % (
        sorted(public - covered - set(EXCLUDED)), sorted((covered | set(EXCLUDED)) - public)))


# ---- the test ------------------------------------------------------------------------------------------------------------------------

def flat(out):
    return [] if out is None else [np.ascontiguousarray(a) for a in out]


@pytest.mark.gpu
@pytest.mark.parametrize("limit", LIMITS)
@pytest.mark.parametrize("name", list(CASES))
def test_entry_point_under_a_grid_limit(env, monkeypatch, capfd, tmp_path, name, limit):
    E = env
    E.mp, E.capfd, E.tmp = monkeypatch, capfd, tmp_path
    fn = CASES[name][0]
    dev = E.hctx.cu_count()[1]
    assert dev >= limit
    with E.limit(limit):
        assert E.hctx.cu_count() == (limit, dev) and E.R.ctx.cu_count() == (limit, dev)
        got = flat(fn(E))
    assert E.hctx.cu_count() == (dev, dev) and E.R.ctx.cu_count() == (dev, dev)
    # where the order of an output is defined: the unlimited run's arrays, byte for byte (that run meets the reference too)
    if name not in E.unlimited:
        E.unlimited[name] = flat(fn(E))
    base = E.unlimited[name]
    assert len(got) == len(base)
    for i, (g, b) in enumerate(zip(got, base)):
        assert g.dtype == b.dtype and g.shape == b.shape and g.tobytes() == b.tobytes(), (name, limit, "output %d" % i)
