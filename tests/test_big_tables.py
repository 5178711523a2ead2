"""Tables past 2^32 bytes and past 2^32 slots through every table writer and reader.

A slot is 16 bytes, so a slot's byte offset leaves 32 bits at slot 2^28, its index a signed int at 2^31 and an unsigned one
at 2^32.  A slot index cut to 32 bits gives a lower address inside the same allocation: a wrong answer, not a fault.  The
shapes (tests/big_tables.py SHAPES; k = 31 unless stated):

  A    2^28 slots      = exactly 2^32 bytes      the byte size wraps to 0 in 32 bits, the last slot is at 2^32 - 16
  B    5 * 2^26 slots  = 5 GiB, m8 = 5           slot 2^28 inside range 52428; every writer, every reader
  E    5 * 2^30 slots  = 80 GiB, m8 = 5          slots 2^28, 2^31 and 2^32 inside ranges; level 2 fans out 1024 ways
  D14  4^14 slots, k = 14 = 2^32 bytes           the direct-addressed build at the 4 GiB size
  D16  4^16 slots, k = 16 = 64 GiB               the direct build with kbits == 32, slot indices up to 2^32 - 1

The contents are sparse and steered (big_tables.plan): the ranges that straddle the edges, range 0 and the last range at
load 0.85, 64 keys homed in the 8 positions below every edge so that they pile across it, a small read set's de Bruijn
graph all over the table and paths through the edge keys.  The conditions are proved on the CPU by the tests at the top
(table_model.layout), the restated hash is pinned at these sizes to kt_table.hpp by golden/table_homes_big.json
(tools/table_homes.cpp big).  The expected answer is always a table_model.Model of the plan's pairs read through the
restatements of tests/test_table_geometries.py, whose writers and reader matrix are used as they are; outputs are primed
with poison there.  After every writer: the size, every key of the plan looked up, absent keys - homed at the edges among
them - looked up to 0.

Every GPU test works out the bytes it needs and skips, with both numbers in the reason, only when the card has less free
(test_big_batches.room); after each test `big: ...` is printed: its seconds, the device bytes seen in use (mark) and the
`[bulk]` lines of its jobs.

The tests that write a table E share one allocation (E_pool: getting 80 GiB from the driver took 0.3 to 17 s a time when
every test asked for its own), handed out cleared with the last test's content still in its slots; the tests that only
read E share a second one (E_dense).  With both alive and a table B beside them 175 GiB are in use.

Measured on an idle MI355X (34 passed, none skipped, 29 s in all, the restatements' work on the CPU included; GB of
device memory seen in use, the shared tables E counted in; the [bulk] lines are the jobs' own, `keys<=` what a job was
planned for - the reads' bases, the N ballast of big_tables.BALLAST included):
  B every writer, every reader, 6 writers     0.5 s each (probing reads 2.0)       5.4-5.6 GB
       [bulk] k=31 keys<=8372224 level1=paged level2=fixed build spilled=0 l1=scatter1y l2=swwc build=dense | image
       routed keys: keys<=154128 level1=exact level2=exact l1=exact l2=general build=dense (a filled range's keys
       outgrow the level-1 region of so small a job: the skewed-batch fallback)
       halves: keys<=3670016 ... l2=swwc build=dense, keys<=4710400 ... merge ... l2=swwc build=merge
  B dense, probers first (7 tables)            1.8 s                                5.6 GB    7 x build=dense as above
  B export target, then imaged                 0.7 s                                6.5 GB    ... l2=swwc build=dense-ext
  B add_file and the reverse                   1.6 s                                5.4 GB
  B erase, both forms                          1.6 s                                5.4 GB (marked after the tables closed: 0.07)
  B clear then another plan, probing / bulk    0.6 / 0.5 s                          5.4 / 5.6 GB
  B table files                                0.4 s                                5.4 GB    dense, then the halves' build and merge
  B clip_tips / simplify / index_sequences     1.2 / 1.2 / 0.3 s                    5.4 GB
  E writers: pairs / reads / merge / routed    0.7 / 0.3 / 0.4 / 0.3 s              85.9-87.5 GB
       [bulk] k=31 keys<=65642496 level1=paged level2=fixed build spilled=0 l1=scatter1y l2=swwc build=dense
       [bulk] k=31 keys<=32825344 level1=paged level2=fixed build | merge spilled=0 l1=scatter1y l2=swwc build=dense | merge
       [bulk] k=31 keys<=247227 level1=exact level2=exact build spilled=0 l1=exact l2=general build=dense
  E walkers while dense / of the image         0.04 / 0.3 s                         85.9 GB
  E table probers / graph probers              0.4 / 2.0 s                          85.9 GB
  E compare and setop against B                0.3 s                                85.9 GB + B
  E saved file against B's                     0.03 s                               85.9 GB + B
  E erase with add-back / clear and refill     1.1 / 0.6 s                          86.7 / 85.9 GB
  A pairs / bulk reads, clear, smaller plan    0.9 / 0.5 s                          4.3 / 4.8 GB
       [bulk] k=31 keys<=21471232 level1=paged level2=fixed build spilled=0 l1=scatter1y l2=fast build=dense
  A export into a target                       0.5 s                                5.7 GB    ... l2=fast build=dense-ext
  D14 direct / KT_BUILD_DIRECT=0               0.4 / 0.4 s                          5.2 GB
       [bulk] k=14 keys<=311296 level1=paged level2=fixed build spilled=0 l1=scatter1y l2=fast build=direct | dense,
       then ... merge ... build=merge and ... build=direct-ext | dense-ext
  D16                                          1.5 s                                69.7 GB
       [bulk] k=16 keys<=352256 level1=paged level2=exact build spilled=0 l1=scatter1x l2=general build=direct,
       then ... merge ... build=merge and ... build=direct-ext
A whole walk of E's 80 GiB image (export_host) takes 19 ms, imaging it in place 14 ms.

That the tests bite was seen once each with three scratch builds that truncate (every address stays inside the table):
  Probe::slot() returns (uint32_t)(base + rel): 7 tests failed, all of E - the three bulk writers (their true places
      against the probers' truncated ones), the table and graph probers, compare / setop against B, clear and refill
      (9912 of the 44903 keys look up to 0); every test of B, A, D14 and D16 passed (D16's indices end at 2^32 - 1), and so
      did E's probing pairs and erase, where writer and reader truncate alike, and E's walkers and saved file: a walker
      finds an entry wherever it lies
  table_export_kernel reads slot i at byte (uint32_t)(i * 16): 28 failed - every test of B and of E but the walkers
      of the dense form, and D16; the 6 that passed are A's three and D14's two (their last byte offset is 2^32 - 16)
      and E's walkers while dense
  table_wipe clears (uint32_t)(cap * 16) / 16 slots (none of A's, a fifth of B's): 22 failed, all of A's among them -
      after the bulk build, A's clear-then-a-smaller-plan finds keys from before the clear; the probing writer on the
      never-cleared fresh table is refused as full - and the tests of B, E, D14 and D16 that write by probing or clear;
      the 12 that passed build B and E in bulk, which writes every slot, and only read
No kernel of the library was wrong.
"""
import gc
import json
import os
import sys
import time

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import big_tables as bt  # noqa: E402
import ktab_ref  # noqa: E402
import table_model as tm  # noqa: E402
import test_big_batches as bbt  # noqa: E402
import test_table_geometries as ttg  # noqa: E402
import test_table_lifecycle as lc  # noqa: E402
from test_table_lifecycle import same  # noqa: E402

gpu = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "table_homes_big.json")
GIB = 1 << 30
KPAT, CPAT = 0xA5A5A5A5A5A5A5A5 - (1 << 64), 0xA5A5A5A5 - (1 << 32)  # poison, as torch's signed integers


# ---- without a GPU ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("request_,k", [(5 << 30, 31), (5 << 26, 31), (1 << 28, 31), (81920, 31), (1 << 34, 30), (1 << 20, 29),
                                        (4 ** 16, 16), (4 ** 14, 14), (1 << 20, 15), (5 << 17, 12)])
def test_inverse_of_the_hash_against_home_of(request_, k):
    """hash_inverse undoes khash / nhash, and keys_built_at gives canonical k-mers whose home_of is what was asked for: a
    range and one position, a window, anywhere in the range - also in the last range, at its last position"""
    g = tm.geometry(request_, k)
    rng = np.random.default_rng(request_ % 1000 + k)
    keys = tm.canonical_keys(rng, k, 500)
    if k <= 16:
        t = ((keys & np.uint64(0xFFFFFFFF)) * np.uint64(0x9E3779B1)) & np.uint64(0xFFFFFFFF)
        t = (t << np.uint64(32 - 2 * k)) & np.uint64(0xFFFFFFFF)
        x = (t ^ (t >> np.uint64(k))) >> np.uint64(32 - 2 * k)
    else:
        x = keys * np.uint64(0x9E3779B97F4A7C15)
        x ^= x >> np.uint64(32)
    assert same(tm.hash_inverse(x, k), keys)
    rs, last = g.range_slots, g.n_ranges - 1
    few = k <= 16 and 2 * k - g.n < 8  # (a narrow hash leaves few bits below the table's: few keys per position)
    for r, at in ((0, 0), (last, rs - 1), (last // 2, (rs // 2 - 8, rs // 2 - 1)), (last // 3, None), (last, (rs - 8, rs - 1))):
        n = 1 if few and at is not None else 40
        if few and not isinstance(at, tuple) and at is not None:
            continue
        got = tm.keys_built_at(k, g, r, at, n, rng)
        rr, pp = tm.home_of(got, k, g)
        lo, hi = (0, rs - 1) if at is None else at if isinstance(at, tuple) else (at, at)
        assert len(np.unique(got)) == n and (rr == r).all() and (pp >= lo).all() and (pp <= hi).all(), (r, at)
        assert same(got, tm.gr.canon_np(got, k)) and (got < np.uint64(4 ** k)).all()


def test_restated_geometry_and_homes_equal_the_headers_at_these_sizes():
    """tools/table_homes.cpp big printed make_geom and probe_of for the five shapes: the mixer's keys and, per edge, a key
    homed in the slot below it and one homed at it, built there with khash_inv / nhash_inv"""
    with open(GOLDEN) as f:
        gold = json.load(f)
    assert [t["name"] for t in gold["tables"]] == list(bt.SHAPES)
    for t in gold["tables"]:
        request_, k, n, m8, slots = bt.SHAPES[t["name"]]
        g = tm.geometry(t["request"], t["k"])
        assert (t["request"], t["k"], t["cap"], 64 - t["shift"], t["m8"]) == (request_, k, slots, n, m8), t["name"]
        assert (g.cap, g.shift, g.m8, g.range_slots) == (t["cap"], t["shift"], t["m8"], t["range_slots"]), t["name"]
        assert t["kbits"] == (2 * k if k <= 16 else 0)
        keys = np.array(t["keys"], np.uint64)
        assert len(keys) == 12 + 2 * len(bt.edges_of(t["name"])) and same(keys, tm.gr.canon_np(keys, k))
        r, p = tm.home_of(keys, k, g)
        assert (r * g.range_slots).tolist() == t["base"] and p.tolist() == t["rel"], t["name"]
        home = [b + q for b, q in zip(t["base"], t["rel"])]
        steered = home[10:]
        if k > 16:
            want = [s for e in bt.edges_of(t["name"]) for s in (e - 1, e)] + [g.range_slots - 1, g.cap - 1]
            assert steered == want, (t["name"], steered)
        else:  # (the one word of a slot may not be canonical: the nearest slot below / above whose word is)
            want = [s for e in bt.edges_of(t["name"]) for s in (e - 1, e)] + [g.range_slots - 1, g.cap - 1]
            assert all(abs(a - b) <= 8 for a, b in zip(steered, want)), (t["name"], steered)
            for e, (a, b) in zip(bt.edges_of(t["name"]), zip(steered[0::2], steered[1::2])):
                assert a < e <= b
        assert max(home) == g.cap - 1 or k <= 16


@pytest.mark.parametrize("name,variant", [(n, v) for n in bt.PROBED for v in (0, 1)])
def test_plan_conditions_hold(oracle, name, variant):
    """both sides of every edge taken, keys that crossed it, wraps in range 0 and at the table's last slot, no range over 0.9"""
    P = bt.plan(name, variant)
    nums = bt.check_plan(P)
    assert nums["keys"] < 50000 and nums["bases"] < (8 << 20) + (bt.BALLAST[name] if variant == 0 else 0)
    if name == "E":
        assert [e.bit_length() - 1 for e in P.edges] == [28, 31, 32]
        Q = bt.plan.__wrapped__(name, variant)  # seeded: a second construction gives the same content
        assert same(Q.base.keys, P.base.keys) and same(Q.base.counts, P.base.counts) and same(Q.gone, P.gone) and same(Q.absent, P.absent)
    if name == "A":
        assert P.edges == [] and bt.bytes_of(name) == 1 << 32
    other = bt.plan(name, 1 - variant)
    assert not np.isin(other.base.keys, P.base.keys).any()  # (what follows a clear shares no key with what was there)


@pytest.mark.parametrize("name", bt.DIRECT)
def test_direct_plan_conditions_hold(oracle, name):
    bt.check_direct_plan(bt.direct_plan(name))


def test_level2_rule_restated():
    """split_bits and the choice of the level-2 kernel (kt_bulk.hip) at the shapes here: the default split of E's 33 hash
    bits gives level 2 a fan-out of 1024, of 34 bits 2048; one line per fine bucket (136 bytes with its two words) fits the
    160 KB of LDS up to 1024 buckets; a job planned for too few keys gives a fine bucket less than a line of fixed room
    and level 2 runs the exact kernel alone"""
    assert [bt.split_bits(n) for n in (28, 29, 32, 33, 34)] == [(8, 7), (7, 9), (10, 9), (10, 10), (10, 11)]
    assert bt.split_bits(24, 1) == (1, 10) and bt.split_bits(25, 1) == (1, 11) and bt.split_bits(23, 1) == (1, 9)
    assert bt.split_bits(35)[1] > 11  # (past what two passes resolve: the build declines)
    assert bt.swwc_lds(512) == 69696 and bt.swwc_lds(1024) == 139328 <= 160 * 1024 < bt.swwc_lds(2048) == 278592
    E = bt.plan("E")
    bases = int(E.csr["high"][1][-1])
    assert bt.level2_of(bases - bt.BALLAST["E"], 33, 8) == "general"  # 7 M keys over 1024 buckets: 11 keys of room per fine bucket
    assert bt.level2_of(bases, 33, 8) == "swwc"                        # with the ballast: 71 -> 64, four lines
    assert bt.level2_of(bases, 33, 8, level1="exact") == "general"
    assert bt.level2_of(int(bt.plan("B").csr["high"][1][-1]), 29, 8) == "swwc"
    for k_bytes in (8, 4):
        assert bt.level2_of(600_000, 24, k_bytes, 1) == "swwc" and bt.level2_of(600_000, 25, k_bytes, 1) == "fast"
        assert bt.level2_of(600_000, 23, k_bytes, 1) == "swwc"
    assert bt.level2_of(100_000, 25, 4, 1) == "general"  # (29 keys of room: less than a line of 32-bit keys)
    line = "[bulk] k=31 keys<=19504025 level1=paged level2=fixed build spilled=0 l1=scatter1y l2=swwc build=dense"
    assert bt.level2_of_line(line, 33, 8) == "swwc" and bt.level2_of_line(line.replace("paged", "exact"), 33, 8) == "general"


# ---- the rig ---------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    return torch


class Rig(lc.Rig):
    """test_table_geometries' rig for a big plan: torch's stream, the partner a small table of another shape"""

    def __init__(self, torch, P):
        from kmertools_amd import device
        self.torch, self.P, self.k, self.own = torch, P, P.k, False
        self.ctx = device.Context(0, stream=torch.cuda.current_stream().cuda_stream)
        self.made = []
        self.pm = P.partner
        self.partner = self.counter(P.partner_request)
        assert self.partner.capacity() == bt.SMALL_SLOTS
        self.partner.add_pairs_host(self.pm.keys, self.pm.counts)
        self.prof_csr = P.csr["profile"]

    pooled = None

    def use(self, P):
        """the rig's plan: the readers take their reads, absent keys and partner from it"""
        if self.P is not P or self.pm is not P.partner:
            self.P, self.pm, self.prof_csr = P, P.partner, P.csr["profile"]
            self.partner.clear()
            self.partner.add_pairs_host(self.pm.keys, self.pm.counts)

    def table(self, request_=None):
        """the geometry from Counter.capacity() and from table_model.geometry.  A pooled table (E: allocating 80 GiB takes
        seconds) is handed out cleared, with whatever the test before left in its slots under the pending clear"""
        if self.pooled is not None:
            self.pooled.export_target(None, None, 0)
            self.pooled.clear()
            return self.pooled
        c = self.counter(self.P.request)
        assert c.capacity() == self.P.g.cap == tm.geometry(self.P.request, self.k).cap == bt.SHAPES[self.P.name][4]
        return c

    def file_source(self):
        c = self.counter(bt.FILE_REQUEST)
        assert c.capacity() == bt.FILE_SLOTS
        return c

    def drop(self, c):
        c.close()
        self.made.remove(c)


_lines = []


@pytest.fixture
def big(torch_mod, oracle, request, monkeypatch):
    """big(P, need, what) -> a Rig, after room(); prints the test's seconds, memory and [bulk] lines when it ends"""
    torch = torch_mod
    made = []
    bbt._use.clear()
    del _lines[:]
    t0 = time.time()
    seen = lc.bulk_lines

    def recording(capfd):
        lines = seen(capfd)
        _lines.extend(lines)
        return lines
    monkeypatch.setattr(lc, "bulk_lines", recording)

    def make(P, need, what):
        if P.name == "E":  # one allocation for all the tests that write a table E
            R = request.getfixturevalue("E_pool")
            R.use(P)
            bbt._use.update(need=int(need), start=bbt.free_bytes(R.ctx) + bt.bytes_of("E"), low=bbt.free_bytes(R.ctx))
            return R
        R = Rig(torch, P)
        made.append(R)
        bbt.room(torch, R.ctx, need, what)
        return R

    yield make
    torch.cuda.synchronize()
    for R in made:
        R.close()
    gc.collect()
    torch.cuda.empty_cache()
    print("big: %s: %.1f s, %d bytes needed by its own count, %d bytes seen in use%s" % (
        request.node.name, time.time() - t0, bbt._use.get("need", 0), bbt._use.get("start", 0) - bbt._use.get("low", 0),
        "".join("\n     " + line for line in _lines)))


def need_of(name, tables=1, extra=4 * GIB):
    return tables * bt.bytes_of(name) + extra


def after_writer(R, c, m, tag):
    """the size, every key of the content, the absent keys; the memory mark"""
    assert c.size() == m.size, (tag, "size")
    got = c.lookup_host(m.keys)
    bad = np.flatnonzero(got != m.counts)
    assert not len(bad), "%s: %d of %d keys look up wrong, the first %#x: %d for %d" % (
        tag, len(bad), m.size, int(m.keys[bad[0]]), int(got[bad[0]]), int(m.counts[bad[0]]))
    assert not c.lookup_host(R.P.absent).any(), (tag, "absent keys")
    bbt.mark(R.torch, R.ctx)


def l2_is_the_rule(P, b1_env=0):
    """every [bulk] line the test has seen names the level-2 kernel the restated rule gives"""
    assert _lines
    for line in _lines:
        if "redone" not in line:
            assert line.split()[-2] == "l2=" + bt.level2_of_line(line, P.g.n, 8 if P.k > 16 else 4, b1_env), line


# ---- B: every writer, then every reader --------------------------------------------------------------------------------------------------

def w_bulk_image(R, P, mp, capfd):
    ttg.env_bulk(mp)
    mp.setenv("KT_BULK_DENSE", "0")
    c = R.table()
    capfd.readouterr()
    ttg.add_device(R, c, "high")
    ttg.bulk_line(capfd, P, "bulk build, imaged at once", "build", "image")
    return c


B_WRITERS = {"probing_reads": ttg.w_probing_reads, "probing_pairs": ttg.w_probing_pairs, "bulk_reads": ttg.w_bulk_reads,
             "bulk_image": w_bulk_image, "bulk_routed": ttg.w_bulk_routed, "bulk_merge": ttg.w_bulk_merge}


@gpu
@pytest.mark.parametrize("writer", list(B_WRITERS))
def test_B_every_writer_then_every_reader(big, monkeypatch, capfd, writer):
    """bulk_reads leaves the table dense: the walkers of the reader matrix come first and read that form, the first prober
    images it in place (kt_table_image)"""
    P = bt.plan("B")
    R = big(P, need_of("B"), "table B")
    tag = "B writer " + writer
    c = B_WRITERS[writer](R, P, monkeypatch, capfd)
    if writer == "bulk_reads":
        ttg.check(R, c, ttg.ref_of(P, "base"), ttg.WALKERS, tag + " while dense")
    after_writer(R, c, P.base, tag)
    ttg.finish(R, P, c, ttg.readers_for(True), tag)
    after_writer(R, c, P.high, tag + " (the pairs on top)")
    if writer.startswith("bulk"):
        l2_is_the_rule(P)


@gpu
def test_B_dense_build_read_by_probers_first(big, monkeypatch, capfd):
    """the first call on the dense table is a prober: kt_table_image in place, then the walkers read the image"""
    P = bt.plan("B")
    R = big(P, need_of("B"), "table B")
    c = ttg.w_bulk_reads(R, P, monkeypatch, capfd)
    ref = ttg.ref_of(P, "base")
    probers = ttg.TABLE_PROBERS + ttg.GRAPH_PROBERS
    for names in (probers[:1], ttg.WALKERS, probers):
        ttg.check(R, c, ref, names, "B dense, probers first")
    after_writer(R, c, P.base, "B dense, probers first")
    for name in ("compare(partner, t)", "xor(t, partner)", "graph(1)", "cov", "hetmers", "unitigs+links"):
        d = ttg.w_bulk_reads(R, P, monkeypatch, capfd)  # each prober that images through its own entry point, first once
        ttg.check(R, d, ref, (name,) + ttg.WALKERS[:3], "B dense, first prober " + name)
        R.drop(d)
    bbt.mark(R.torch, R.ctx)


@gpu
def test_B_bulk_build_into_an_export_target_then_imaged_from_the_pairs(big, monkeypatch, capfd):
    P = bt.plan("B")
    R = big(P, need_of("B"), "table B")
    ttg.test_bulk_build_into_an_export_target(lambda request_, k: R, monkeypatch, capfd, P.request, P.k)
    bbt.mark(R.torch, R.ctx)


@gpu
def test_B_add_file_of_a_small_table_and_the_reverse(big, monkeypatch, capfd, tmp_path):
    """a file saved from a 65 536-slot table of the same content loaded into B; B's file loaded into the small table"""
    P = bt.plan("B")
    R = big(P, need_of("B"), "table B")
    c = ttg.w_add_file(R, P, monkeypatch, capfd, tmp_path)
    after_writer(R, c, P.base, "B add_file")
    ttg.finish(R, P, c, ttg.readers_for(True), "B add_file")
    path = str(tmp_path / "big.ktab")
    assert c.save(path) == P.high.size
    s = R.file_source()
    assert s.add_file(path) == P.high.size
    after_writer(R, s, P.high, "the small table from B's file")
    ttg.check(R, s, ttg.ref_of(P, "high"), ttg.WALKERS + ttg.TABLE_PROBERS, "the small table from B's file")


@gpu
def test_B_erase_a_third_then_add_half_of_it_back(big, monkeypatch, capfd):
    """the erased keys include those in the slots either side of slot 2^28, keys that crossed it, slot 0 and the last slot"""
    P = bt.plan("B")
    R = big(P, need_of("B"), "table B")
    ttg.test_erase_a_third_then_add_half_of_it_back(lambda request_, k: R, monkeypatch, capfd, P.request, P.k)
    bbt.mark(R.torch, R.ctx)


def clear_then_another_content(R, c, P, Q, tag, readers):
    """c holds P's content: cleared, Q's content added by the probing path; nothing of P shows through"""
    c.clear()
    assert c.size() == 0
    assert not c.lookup_host(P.base.keys[::3]).any(), tag
    order = np.random.default_rng(8).permutation(Q.base.size)
    c.add_pairs_host(Q.base.keys[order], Q.base.counts[order])
    after_writer(R, c, Q.base, tag)
    assert not c.lookup_host(P.base.keys).any(), tag + ": a key from before the clear"
    R.use(Q)
    ttg.check(R, c, ttg.ref_of(Q, "base"), readers, tag)


@gpu
@pytest.mark.parametrize("first", ["probing", "bulk"])
def test_B_clear_then_a_different_plan(big, monkeypatch, capfd, first):
    P, Q = bt.plan("B"), bt.plan("B", 1)
    R = big(P, need_of("B"), "table B")
    c = (ttg.w_probing_pairs if first == "probing" else ttg.w_bulk_reads)(R, P, monkeypatch, capfd)
    after_writer(R, c, P.base, "B before the clear")
    ttg.env_probing(monkeypatch)
    clear_then_another_content(R, c, P, Q, "B cleared, " + first, ttg.WALKERS + ttg.TABLE_PROBERS)


@gpu
def test_B_table_files_are_byte_identical_to_the_small_tables(big, monkeypatch, capfd, tmp_path):
    P = bt.plan("B")
    R = big(P, need_of("B"), "table B")
    ttg.test_table_files_are_byte_identical_from_every_shape_and_form(lambda request_, k: R, monkeypatch, capfd, tmp_path, P.request, P.k)
    bbt.mark(R.torch, R.ctx)


@gpu
@pytest.mark.parametrize("what", ["clip_tips", "simplify", "index_sequences"])
def test_B_on_a_copy(big, monkeypatch, what):
    P = bt.plan("B")
    R = big(P, need_of("B", 2), "two tables B")
    fn = {"clip_tips": ttg.test_clip_tips_on_a_copy, "simplify": ttg.test_simplify_on_a_copy,
          "index_sequences": ttg.test_the_table_as_the_index_of_its_own_unitigs}[what]
    fn(lambda request_, k: R, monkeypatch, P.request, P.k)
    bbt.mark(R.torch, R.ctx)


# ---- E: past 2^31 and 2^32 slots ---------------------------------------------------------------------------------------------------------

def w_E_dense(R, P, mp, capfd):
    """the default split of E's 33 hash bits: level 2 fans out 1024 ways, whole lines out of LDS"""
    c = ttg.w_bulk_reads(R, P, mp, capfd)
    assert bt.split_bits(P.g.n) == (10, 10) and _lines[-1].split()[-2] == "l2=swwc" and "level1=paged level2=fixed" in _lines[-1], _lines
    return c


E_WRITERS = {"probing_pairs": ttg.w_probing_pairs, "bulk_reads": w_E_dense, "bulk_merge": ttg.w_bulk_merge, "bulk_routed": ttg.w_bulk_routed}
E_NEED = need_of("E", extra=4 * GIB)  # (seen in use: 81.5 GiB at most)


@gpu
@pytest.mark.parametrize("writer", list(E_WRITERS))
def test_E_writers(big, monkeypatch, capfd, writer):
    """one table per writer: the size, every key, the absent keys, both exports and the spectrum"""
    P = bt.plan("E")
    R = big(P, E_NEED, "table E")
    c = E_WRITERS[writer](R, P, monkeypatch, capfd)
    ref = ttg.ref_of(P, "base")
    if writer.startswith("bulk"):
        ttg.check(R, c, ref, ("size", "export_host", "export_device", "spectrum_host"), "E writer %s, as built" % writer)
        l2_is_the_rule(P)
    after_writer(R, c, P.base, "E writer " + writer)
    ttg.check(R, c, ref, ("export_host", "stage_pieces", "spectrum_device"), "E writer " + writer)


@pytest.fixture(scope="module")
def E_pool(torch_mod, oracle):
    """a rig whose table() is one table E, cleared for every test that asks"""
    torch = torch_mod
    R = Rig(torch, bt.plan("E"))
    gc.collect()
    torch.cuda.empty_cache()
    free = bbt.free_bytes(R.ctx)
    if 2 * E_NEED + need_of("B") > free:
        R.close()
        pytest.skip("two tables E and a table B need %d bytes of device memory, %d are free" % (2 * E_NEED + need_of("B"), free))
    R.pooled = R.table()
    yield R
    R.close()
    gc.collect()
    torch.cuda.empty_cache()


@pytest.fixture(scope="module")
def E_dense(torch_mod, oracle):
    """one table E from the dense build, shared by the tests that only read it"""
    torch = torch_mod
    P = bt.plan("E")
    R = Rig(torch, P)
    gc.collect()
    torch.cuda.empty_cache()
    free = bbt.free_bytes(R.ctx)
    if E_NEED + need_of("B") > free:
        R.close()
        pytest.skip("table E and table B need %d bytes of device memory, %d are free" % (E_NEED + need_of("B"), free))
    mp = pytest.MonkeyPatch()
    ttg.env_bulk(mp)
    mp.setenv("KT_BULK_VERBOSE", "0")
    c = R.table()
    ttg.add_device(R, c, "high")
    mp.undo()
    yield R, c
    R.close()
    gc.collect()
    torch.cuda.empty_cache()


@pytest.fixture
def timed(torch_mod, request):
    bbt._use.clear()
    t0 = time.time()
    yield
    torch_mod.cuda.synchronize()
    print("big: %s: %.1f s, %d bytes seen in use" % (request.node.name, time.time() - t0, bbt._use.get("start", 0) - bbt._use.get("low", 0)))


def shared(E_dense):
    R, c = E_dense
    bbt._use.update(start=bbt.free_bytes(R.ctx) + bt.bytes_of("E"), low=bbt.free_bytes(R.ctx))
    return R, c, ttg.ref_of(R.P, "base")


@gpu
def test_E_walkers_while_dense(E_dense, timed):
    R, c, ref = shared(E_dense)
    ttg.check(R, c, ref, ttg.WALKERS, "E dense")
    bbt.mark(R.torch, R.ctx)


@gpu
def test_E_table_probers(E_dense, timed):
    """the first of them images the table in place: 2^20 ranges, the ones that straddle 2^28, 2^31 and 2^32 among them"""
    R, c, ref = shared(E_dense)
    ttg.check(R, c, ref, ttg.TABLE_PROBERS, "E")
    after_writer(R, c, R.P.base, "E imaged")


@gpu
def test_E_graph_probers(E_dense, timed):
    R, c, ref = shared(E_dense)
    ttg.check(R, c, ref, ttg.GRAPH_PROBERS, "E")
    bbt.mark(R.torch, R.ctx)


@gpu
def test_E_walkers_of_the_image(E_dense, timed):
    R, c, ref = shared(E_dense)
    c.lookup_host(R.P.absent[:4])  # (a prober: the table is the probing image from here on, whichever test ran before)
    ttg.check(R, c, ref, ttg.WALKERS, "E imaged")
    bbt.mark(R.torch, R.ctx)


@gpu
def test_E_compare_and_setop_in_both_roles_against_B(E_dense, timed, monkeypatch):
    """B holds its own plan's content and the partner's keys of E's plan on top, so that the two tables share keys at E's edges"""
    R, c, ref = shared(E_dense)
    P, PB = R.P, bt.plan("B")
    ttg.env_probing(monkeypatch)
    b = R.counter(PB.request)
    assert b.capacity() == PB.g.cap
    bm = PB.base.copy()
    bm.add_pairs(P.partner.keys, P.partner.counts)
    b.add_pairs_host(bm.keys, bm.counts)
    assert b.size() == bm.size
    old = R.partner, R.pm
    R.partner, R.pm = b, bm
    try:
        fresh = lc.Ref(P.base)  # (the memoised answers of `ref` are those against the small partner)
        ttg.check(R, c, fresh, ("compare(t, partner)", "compare(partner, t)", "intersect(t, partner)", "intersect(partner, t)",
                                "xor(t, partner)", "xor(partner, t)"), "E against B")
        shared_keys = np.intersect1d(bm.keys, P.base.keys)
        assert len(shared_keys) >= 1500 and np.isin(np.concatenate(list(P.cluster_in.values())), shared_keys).sum() >= 3 * len(P.cluster_in)
    finally:
        R.partner, R.pm = old
        R.drop(b)
    bbt.mark(R.torch, R.ctx)


@gpu
def test_E_saved_file_is_byte_identical_to_Bs_of_the_same_content(E_dense, timed, monkeypatch, tmp_path):
    R, c, ref = shared(E_dense)
    P = R.P
    want = ktab_ref.encode(P.k, P.base.keys, P.base.counts)
    path = str(tmp_path / "e.ktab")
    assert c.save(path) == P.base.size
    with open(path, "rb") as f:
        e_bytes = f.read()
    ttg.env_probing(monkeypatch)
    b = R.counter(bt.SHAPES["B"][0])
    assert b.capacity() == bt.SHAPES["B"][4]
    b.add_pairs_host(P.base.keys, P.base.counts)
    path_b = str(tmp_path / "b.ktab")
    assert b.save(path_b) == P.base.size
    with open(path_b, "rb") as f:
        b_bytes = f.read()
    R.drop(b)
    assert e_bytes == b_bytes, "the file saved from E is not the file saved from B"
    assert e_bytes == want, "the file saved from E is not ktab_ref's"
    bbt.mark(R.torch, R.ctx)


@gpu
def test_E_erase_with_add_back(big, monkeypatch, capfd):
    P = bt.plan("E")
    R = big(P, E_NEED, "table E")
    c = ttg.w_probing_pairs(R, P, monkeypatch, capfd)
    c.add_pairs_host(*P.pairs)
    arg = np.concatenate([P.gone, P.gone[:7], P.absent[:50], np.array([2 ** 64 - 1, 4 ** P.k], np.uint64)])
    assert c.erase(arg) == len(P.gone)
    after_writer(R, c, P.erased, "E erased")
    assert not c.lookup_host(P.gone).any()
    ttg.check(R, c, ttg.ref_of(P, "erased"), ttg.WALKERS + ttg.TABLE_PROBERS, "E erased")
    c.add_pairs_host(*P.back)
    after_writer(R, c, P.erased_back, "E erased, half back")
    assert not c.lookup_host(np.setdiff1d(P.gone, P.back[0])).any()
    ttg.check(R, c, ttg.ref_of(P, "erased_back"), ttg.WALKERS[:4] + ttg.TABLE_PROBERS[:2], "E erased, half back")


@gpu
def test_E_clear_and_refill(big, monkeypatch, capfd):
    P, Q = bt.plan("E"), bt.plan("E", 1)
    R = big(P, E_NEED, "table E")
    c = ttg.w_bulk_routed(R, P, monkeypatch, capfd)
    after_writer(R, c, P.base, "E before the clear")
    ttg.env_probing(monkeypatch)
    clear_then_another_content(R, c, P, Q, "E cleared", ttg.WALKERS[:6] + ttg.TABLE_PROBERS[:2])


# ---- A: exactly 2^32 bytes ---------------------------------------------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize("writer", ["probing_pairs", "bulk_reads"])
def test_A_writers_walkers_lookup_clear_and_a_smaller_plan(big, monkeypatch, capfd, writer):
    """the table's bytes are 2^32 - 0 in 32 bits - and its last slot, taken by a key whose probe sequence wrapped or ended
    there, lies at byte 2^32 - 16.  After the clear a smaller content of other keys: nothing stale shows through, in any
    slot - the exports and the spectrum walk them all"""
    P, Q = bt.plan("A"), bt.plan("A", 1)
    assert Q.base.size < P.base.size
    R = big(P, need_of("A"), "table A")
    c = B_WRITERS[writer](R, P, monkeypatch, capfd)
    ref = ttg.ref_of(P, "base")
    ttg.check(R, c, ref, ttg.WALKERS, "A writer " + writer)
    after_writer(R, c, P.base, "A writer " + writer)
    ttg.check(R, c, ref, ("lookup",) + ttg.WALKERS, "A writer %s, after the look-up" % writer)
    ttg.env_probing(monkeypatch)
    clear_then_another_content(R, c, P, Q, "A cleared after " + writer, ttg.WALKERS + ("lookup",))


@gpu
def test_A_export_into_a_target(big, monkeypatch, capfd):
    P = bt.plan("A")
    R = big(P, need_of("A"), "table A")
    ref = ttg.ref_of(P, "base")
    n = ref.m.size
    room = n + 9
    xk, xc = R.full(room + lc.GUARD, lc.KPAT, 64), R.full(room + lc.GUARD, lc.CPAT, 32)
    ttg.env_bulk(monkeypatch)
    c = R.table()
    c.export_target(xk, xc, room)
    capfd.readouterr()
    ttg.add_device(R, c, "high")
    ttg.bulk_line(capfd, P, "A export target", "build", "dense-ext")
    ttg.check(R, c, ref, ttg.WALKERS, "A export target")
    R.torch.cuda.synchronize()
    hk, hc = lc.u64(xk), lc.u32(xc)
    assert (hk[room:] == lc.KPAT).all() and (hc[room:] == lc.CPAT).all()
    gk, gc_ = lc.by_key(hk[:n], hc[:n])
    assert same(gk, ref.m.keys) and same(gc_, ref.m.counts)
    after_writer(R, c, P.base, "A export target, imaged from the pairs")
    ttg.check(R, c, ref, ttg.WALKERS, "A export target, imaged")


# ---- D14, D16: the direct-addressed build -------------------------------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize("name,direct", [("D14", "1"), ("D14", "0"), ("D16", "1")])
def test_direct_addressed_tables_at_these_sizes(torch_mod, oracle, monkeypatch, capfd, request, name, direct):
    """as test_ctr_direct_addressed_tables, on 4^14 slots (2^32 bytes) and 4^16 slots (kbits == 32: every `32 - kbits` shift
    is 0, slot indices reach 2^32 - 1): the batch's k-mers sit in the slots either side of 2^28 and 2^31 and in the
    table's first and last - build=direct and, into a target, build=direct-ext; the export, look-ups, cov with the
    batch's reads, a second batch on top"""
    from kmertools_amd import device
    torch = torch_mod
    P = bt.direct_plan(name)
    k, cap = P.k, P.g.cap
    bases, offsets = P.csr
    m = P.model
    oc = oracle.Counter(1)
    oc.add_pairs(m.keys, m.counts)
    want_cov = oc.cov_batch(bases, offsets, k, 2, 9, False)
    probe = np.concatenate([m.keys, P.absent])
    want_probe = m.count(probe)
    monkeypatch.setenv("KT_BULK_MIN_BASES", "0")
    monkeypatch.setenv("KT_BULK_VERBOSE", "1")
    monkeypatch.setenv("KT_BULK_MERGE_DIV", "1000000000")  # (the second batch rebuilds the ranges whatever its size)
    monkeypatch.setenv("KT_BUILD_DIRECT", direct)
    ctx = device.Context(0, stream=torch.cuda.current_stream().cuda_stream)
    t0 = time.time()
    lines = []
    try:
        bbt._use.clear()
        bbt.room(torch, ctx, need_of(name), "table " + name)
        ctr = device.Counter(ctx, k, cap)
        assert ctr.capacity() == cap == 4 ** k == tm.geometry(P.request, k).cap
        capfd.readouterr()
        ctr.add_reads_host(bases, offsets)
        lines += lc.bulk_lines(capfd)
        assert len(lines) == 1 and lines[0].split()[-1] == "build=" + ("direct" if direct == "1" else "dense"), lines
        assert ctr.size() == m.size
        gk, gc_ = ctr.export_host()
        assert same(gk, m.keys) and same(gc_, m.counts), (name, direct)
        assert same(ctr.lookup_host(probe), want_probe)
        assert np.array_equal(ctr.cov_host(bases, offsets, 2, 9, False), want_cov)
        bbt.mark(torch, ctx)
        ctr.add_reads_host(bases, offsets)  # on top: every range rebuilt from what it holds + the batch
        lines += lc.bulk_lines(capfd)
        assert len(lines) == 2 and lines[1].split()[5] == "merge", lines
        gk, gc_ = ctr.export_host()
        assert same(gk, m.keys) and same(gc_, 2 * m.counts)
        assert same(ctr.lookup_host(probe), 2 * want_probe)
        bbt.mark(torch, ctx)
        # cleared, then straight into an export target (the same allocation: a table of 64 GiB takes seconds to get)
        ctr.clear()
        c2 = ctr
        room_ = m.size + 5
        xk = torch.full((room_ + 3,), KPAT, dtype=torch.int64, device="cuda")
        xc = torch.full((room_ + 3,), CPAT, dtype=torch.int32, device="cuda")
        c2.export_target(xk, xc, room_)
        db, do = torch.from_numpy(bases).cuda(), torch.from_numpy(offsets.astype(np.int64)).cuda()
        c2.add_reads(db, do, len(offsets) - 1)
        lines += lc.bulk_lines(capfd)
        assert len(lines) == 3 and lines[2].split()[-1] == "build=" + ("direct-ext" if direct == "1" else "dense-ext"), lines
        d = c2.size()
        assert d == m.size and c2.export(xk, xc, room_) == d
        torch.cuda.synchronize()
        hk, hc = lc.u64(xk), lc.u32(xc)
        assert (hk[room_:] == np.uint64(0xA5A5A5A5A5A5A5A5)).all() and (hc[room_:] == np.uint32(0xA5A5A5A5)).all()
        gk, gc_ = lc.by_key(hk[:d], hc[:d])
        assert same(gk, m.keys) and same(gc_, m.counts)
        assert same(c2.lookup_host(probe), want_probe)
        bbt.mark(torch, ctx)
        c2.close()
    finally:
        torch.cuda.synchronize()
        ctx.close()
        gc.collect()
        torch.cuda.empty_cache()
        print("big: %s: %.1f s, %d bytes needed by its own count, %d bytes seen in use%s" % (
            request.node.name, time.time() - t0, bbt._use.get("need", 0), bbt._use.get("start", 0) - bbt._use.get("low", 0),
            "".join("\n     " + line for line in lines)))
