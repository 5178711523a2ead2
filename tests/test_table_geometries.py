"""Every table geometry through every table writer and every table reader.

kttab::make_geom gives a table one small range (1024 .. 4096 slots), one or two ranges of 8192 slots, or - from 2^15 slots
on - a row of ranges of 1024 * m8 slots with m8 in 5..8; probing wraps at the end of a range.  The other tests build their
tables at whole powers of two and at loads where a probe sequence almost never reaches a range's end.  Here every shape of
tests/table_geometries.py SHAPES is filled to load 0.85 with keys steered to the ends of ranges (plan(): the conditions are
checked on the CPU by the tests at the top), by every writer, and every reader is compared with tests/table_model.py Model
and the restatements the other reader tests keep - exactly: everything is integers.

The restated hash that steers the keys (table_model.geometry / home_of) is itself compared with what kt_table.hpp answers
when compiled for the host: tests/golden/table_homes.json, written by tools/table_homes.cpp."""
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bubble_ref as br  # noqa: E402
import count_edges as ce  # noqa: E402
import hetmer_ref as hr  # noqa: E402
import ktab_ref  # noqa: E402
import table_geometries as tg  # noqa: E402
import table_model as tm  # noqa: E402
import test_table_lifecycle as lc  # noqa: E402
import thread_ref as thr  # noqa: E402
import tip_ref as tr  # noqa: E402
import unitig_link_ref as lr  # noqa: E402
import unitig_ref as ur  # noqa: E402
from test_correct import want_support  # noqa: E402
from test_count_edges import check_unitigs  # noqa: E402
from test_table_lifecycle import refused, same  # noqa: E402

U32 = 0xFFFFFFFF
NO = 0xFFFFFFFF
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "table_homes.json")
MAIN = [(r, tg.WIDTHS[r][0]) for r in tg.REQUESTS]    # every writer, every reader
SECOND = [(r, tg.WIDTHS[r][1]) for r in tg.REQUESTS]  # the other key width: the probing and the bulk writers, the table readers
BULK_MAIN = [(r, k) for r, k in MAIN if tg.bulk_eligible(r)]


# ---- without a GPU: the restatement against the library's own header, the conditions of every plan ---------------------------

def test_restated_geometry_and_homes_equal_the_headers():
    """tools/table_homes.cpp printed make_geom and probe_of for every shape and k in {7, 8, 15, 16, 17, 21, 31}"""
    with open(GOLDEN) as f:
        gold = json.load(f)
    assert sorted({t["request"] for t in gold["tables"]}) == sorted(tg.REQUESTS)
    assert sorted(int(k) for k in gold["keys"]) == [7, 8, 15, 16, 17, 21, 31] and len(gold["tables"]) == 70
    for k, keys in gold["keys"].items():
        k, keys = int(k), np.array(keys, np.uint64)
        assert len(keys) >= 200 and keys[0] == 0 and same(keys, tm.gr.canon_np(keys, k))
        top = int(keys[1])  # the largest canonical k-mer: T..T [C] A..A
        assert tm.gr.str_of(top, k) == "T" * (k // 2) + "C" * (k % 2) + "A" * (k // 2)
        if k <= 8:
            x = np.arange(4 ** k, dtype=np.uint64)
            assert top == int(tm.gr.canon_np(x, k).max())
    for t in gold["tables"]:
        g = tm.geometry(t["request"], t["k"])
        tag = (t["request"], t["k"])
        assert (g.cap, g.shift, g.m8, g.range_slots) == (t["cap"], t["shift"], t["m8"], t["range_slots"]), tag
        assert g.n_ranges * g.range_slots == g.cap and t["kbits"] == (2 * t["k"] if t["k"] <= 16 else 0), tag
        r, p = tm.home_of(np.array(gold["keys"][str(t["k"])], np.uint64), t["k"], g)
        assert (r * g.range_slots).tolist() == t["base"] and p.tolist() == t["rel"], tag
        assert max(t["rel"]) < g.range_slots and max(t["base"]) < g.cap, tag
    # the power-of-two signature the older tests use is the same function
    keys = np.array(gold["keys"]["31"], np.uint64)
    a, b = tm.home_of(keys, 31, 15), tm.home_of(keys, 31, tm.geometry(32768, 31))
    assert same(a[0], b[0]) and same(a[1], b[1])


@pytest.mark.parametrize("request_", tg.REQUESTS)
def test_shape_of_every_request(request_):
    g = tm.geometry(request_)
    assert (g.cap, g.n_ranges, g.m8) == tg.SHAPES[request_]
    assert g.range_slots == (g.cap if g.cap < 8192 else 1024 * g.m8) and request_ <= g.cap <= 1.25 * request_


def test_layout_against_a_plain_loop():
    """tm.layout on a table of two ranges and on one small range: the slots a list-of-lists linear probing takes"""
    for request_, k, n in ((16384, 21, 15000), (1024, 15, 1000)):
        g = tm.geometry(request_, k)
        keys = tm.canonical_keys(np.random.default_rng(request_), k, n)
        keys = np.concatenate([keys, tm.keys_homed_at(k, g, g.n_ranges - 1, g.range_slots - 1, 5, seed=3)])
        L = tm.layout(keys, k, g)
        r, h = tm.home_of(keys, k, g)
        taken = [[False] * g.range_slots for _ in range(g.n_ranges)]
        for i in range(len(keys)):
            s, d = int(h[i]), 0
            while taken[r[i]][s]:
                s, d = (s + 1) % g.range_slots, d + 1
            taken[r[i]][s] = True
            assert (int(L.slot[i]), int(L.displacement[i]), bool(L.wrapped[i])) == (s, d, s < h[i]), i
        assert L.fill.tolist() == [sum(t) for t in taken] and L.wrapped[-4:].all()


@pytest.mark.parametrize("request_,k", MAIN + SECOND)
def test_plan_conditions_hold(oracle, request_, k):
    """loads, wraps in every clustered range, the longest displacement, the claim-list threshold, brim, the erase set"""
    P = tg.plan(request_, k)
    tg.check_plan(P)
    # seeded: a second construction gives the same content
    if request_ == 4096:
        Q = tg.plan.__wrapped__(request_, k)
        assert same(Q.high.keys, P.high.keys) and same(Q.high.counts, P.high.counts) and same(Q.gone, P.gone)
        assert Q.high_reads == P.high_reads and same(Q.absent, P.absent)


def test_every_shape_has_both_key_widths_and_another_shape_beside_it():
    for r in tg.REQUESTS:
        a, b = tg.WIDTHS[r]
        assert (a <= 16) != (b <= 16) and tg.SHAPES[tg.OTHER[r]] != tg.SHAPES[r]
        assert tg.SHAPES[tg.OTHER[r]][2] != tg.SHAPES[r][2] or tg.SHAPES[tg.OTHER[r]][1] != tg.SHAPES[r][1]


# ---- the rig --------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    return torch


class Rig(lc.Rig):
    """test_table_lifecycle's rig on torch's stream, its partner table of another shape than the table under test"""

    def __init__(self, torch, P):
        from kmertools_amd import device
        self.torch, self.P, self.k, self.own = torch, P, P.k, False
        self.ctx = device.Context(0, stream=torch.cuda.current_stream().cuda_stream)
        self.made = []
        self.pm = P.partner
        self.partner = self.counter(P.partner_request)
        assert self.partner.capacity() == tg.SHAPES[P.partner_request][0]
        self.partner.add_pairs_host(self.pm.keys, self.pm.counts)
        self.prof_csr = P.csr["profile"]

    def table(self, request_=None):
        request_ = self.P.request if request_ is None else request_
        c = self.counter(request_)
        assert c.capacity() == tg.SHAPES[request_][0]
        return c

    def file_source(self):
        """an empty table of another shape, with room for the plan's content"""
        request_, cap = tg.FILE_FROM[self.P.request]
        c = self.counter(request_)
        assert c.capacity() == cap == tm.geometry(request_).cap != self.P.g.cap
        return c


@pytest.fixture
def rig(torch_mod, oracle):
    made = []

    def make(request_, k):
        made.append(Rig(torch_mod, tg.plan(request_, k)))
        return made[-1]

    yield make
    for R in made:
        R.close()


def ref_of(P, name):
    """the frozen model `name` of a plan with its memoised answers, shared by every test of the plan"""
    refs = P.__dict__.setdefault("refs", {})
    if name not in refs:
        refs[name] = lc.Ref(getattr(P, name))
    return refs[name]


# ---- the readers test_table_lifecycle.py does not have ------------------------------------------------------------------------------

COV_BINS = ((1, 12), (3, 5), (1 << 28, 16))


def r_cov(R, c, ref):
    from oracle import kt_oracle
    bases, offsets = R.prof_csr

    def make():
        oc = kt_oracle.Counter(1)
        oc.add_pairs(ref.m.keys, ref.m.counts)
        return {(b, norm): oc.cov_batch(bases, offsets, R.k, b[0], b[1], norm=norm) for b in COV_BINS for norm in (False, True)}
    want = ref.memo("cov", make)
    for b in COV_BINS:
        raw = want[(b, False)]
        assert same(c.cov_host(bases, offsets, b[0], b[1], norm=False, dtype="u32"), raw.astype(np.uint32)), b
        assert same(c.cov_host(bases, offsets, b[0], b[1], norm=False, dtype="f64").view(np.uint64), raw.view(np.uint64)), b
        g64 = c.cov_host(bases, offsets, b[0], b[1], norm=True, dtype="f64")
        assert same(g64.view(np.uint64), want[(b, True)].view(np.uint64)), b
        g32 = c.cov_host(bases, offsets, b[0], b[1], norm=True, dtype="f32")
        assert g32.dtype == np.float32 and float(np.abs(g32.astype(np.float64) - want[(b, True)]).max(initial=0)) <= 1e-6, b


def profile_want(R, ref):
    return ref.memo("profile", lambda: ref.m.profile(R.P.seqs["profile"]))


SOLID = (2, 1000)


def r_read_solidity(R, c, ref):
    """per read: its k-mers, those with SOLID[0] <= count <= SOLID[1], the start of the first other one - from the profile"""
    bases, offsets = R.prof_csr
    prof = profile_want(R, ref)

    def make():
        nk, ns, fw = [], [], []
        for o, e in zip(offsets[:-1].tolist(), offsets[1:].tolist()):
            seg = prof[o:e]
            valid = seg != NO
            solid = valid & (seg >= SOLID[0]) & (seg <= SOLID[1])
            weak = np.flatnonzero(valid & ~solid)
            nk.append(int(valid.sum())), ns.append(int(solid.sum())), fw.append(int(weak[0]) if len(weak) else NO)
        return np.array(nk, np.uint32), np.array(ns, np.uint32), np.array(fw, np.uint32)
    want = ref.memo("solidity", make)
    got = c.read_solidity_host(bases, offsets, *SOLID)
    for g, w, name in zip(got, want, ("n_kmers", "n_solid", "first_weak")):
        assert same(g, w), name


def r_correct_support(R, c, ref):
    from oracle import kt_oracle
    bases, offsets = R.prof_csr
    prof = profile_want(R, ref)
    want = ref.memo("support", lambda: want_support(kt_oracle, bases, offsets, R.k, ref.m, prof, *SOLID))
    sup = np.zeros(len(bases), np.uint32)
    c.correct_support(bases, offsets, len(offsets) - 1, prof, SOLID[0], SOLID[1], sup, mem=0)
    assert same(sup, want)


def r_hetmers(R, c, ref):
    w = ref.memo("hetmers", lambda: hr.restate(ref.m.keys, ref.m.counts, R.k))
    a, b, ca, cb, cen = c.hetmers(census=True)
    assert same(a, w.a) and same(b, w.b) and same(ca, w.ca) and same(cb, w.cb)
    assert same(cen[:len(w.census)], w.census)


def graph_strings(R, ref):
    """the table as {canonical string: count}, its unitigs and links - what the string restatements take, made once"""
    def make():
        table = ce.strings_of(ref.m.keys, ref.m.counts, R.k)
        return (table,) + tuple(lr.links(table, R.k))
    return ref.memo("links", make)


def r_unitigs_and_links(R, c, ref):
    _, us, ls = graph_strings(R, ref)
    check_unitigs(c, (us, ls), 1, U32, "unitigs")


def shape_of(us):
    return [u[3] for u in us], [u[1] for u in us], [bool(u[2] & ur.CIRCULAR) for u in us]


def r_unitig_tips(R, c, ref):
    _, us, ls = graph_strings(R, ref)

    def make():
        n, cs, circ = shape_of(us)
        m = tr.marks_of(n, cs, circ, ls, R.k)
        return m, tr.tally_of(m, n)
    marks, tally = ref.memo("tips", make)
    gm, gt = c.unitig_tips(R.k)
    assert gm.tolist() == marks and [int(x) for x in gt] == tally


def r_unitig_bubbles(R, c, ref):
    _, us, ls = graph_strings(R, ref)

    def make():
        n, cs, circ = shape_of(us)
        m, bubbles = br.marks_of(n, cs, circ, ls, 2 * R.k)
        return m, br.tally_of(m, n, cs, bubbles)
    marks, tally = ref.memo("bubbles", make)
    gm, gt = c.unitig_bubbles(2 * R.k)
    assert gm.tolist() == marks and [int(x) for x in gt] == tally


READERS = dict(lc.READERS)
READERS.update({"cov": r_cov, "read_solidity": r_read_solidity, "correct_support": r_correct_support, "hetmers": r_hetmers,
                "unitigs+links": r_unitigs_and_links, "unitig_tips": r_unitig_tips, "unitig_bubbles": r_unitig_bubbles})
WALKERS = lc.WALKERS
TABLE_PROBERS = lc.PROBERS + ("cov", "read_solidity", "correct_support")
GRAPH_PROBERS = ("hetmers", "unitigs+links", "unitig_tips", "unitig_bubbles")
assert set(WALKERS) | set(TABLE_PROBERS) | set(GRAPH_PROBERS) == set(READERS)


def read(R, c, ref, name, tag):
    """one reader against the model, and the content it left: the size and the sorted export"""
    try:
        READERS[name](R, c, ref)
        assert c.size() == ref.m.size, "the size afterwards"
        gk, gc = c.export_host()
        assert same(gk, ref.m.keys) and same(gc, ref.m.counts), "the content afterwards"
    except Exception as e:  # noqa: BLE001 (an error code of the library is a finding like a mismatch)
        raise AssertionError("%s: reader %s: %s: %s" % (tag, name, type(e).__name__, e)) from e


def check(R, c, ref, names, tag):
    for name in names:
        read(R, c, ref, name, tag)


def readers_for(k_is_main):
    return WALKERS + TABLE_PROBERS + (GRAPH_PROBERS if k_is_main else ())


def absent_are_absent(R, c, tag):
    """the absent keys - those homed in the last slots of the clustered ranges among them - through the look-up"""
    assert not c.lookup_host(R.P.absent).any(), tag


# ---- the writers: each leaves a table that holds P.base, every reader follows, then P.pairs on top and every reader again ------

def env_probing(mp):
    mp.setenv("KT_BULK", "0")
    mp.setenv("KT_BULK_VERBOSE", "1")


def env_bulk(mp):
    lc.env_bulk(mp)


def add_device(R, c, name):
    lc.add_device(R, c, name)


def bulk_line(capfd, P, tag, what="build", built=None):
    """the job's verbose line: one, naming `what` (build | merge), on the shapes the bulk build takes - none on the others"""
    lines = lc.bulk_lines(capfd)
    if not tg.bulk_eligible(P.request):
        assert lines == [], (tag, "the bulk build took a table of fewer than four ranges", lines)
        return None
    assert len(lines) == 1 and lines[0].split()[5] == what, (tag, lines)
    if built is not None:
        assert lines[0].split()[-1] == "build=" + built, (tag, lines)
    return lines[0]


def w_probing_reads(R, P, mp, capfd):
    env_probing(mp)
    c = R.table()
    c.add_reads_host(*P.csr["high"])
    assert lc.bulk_lines(capfd) == []
    return c


def w_probing_pairs(R, P, mp, capfd):
    env_probing(mp)
    c = R.table()
    order = np.random.default_rng(5).permutation(P.base.size)
    c.add_pairs_host(P.base.keys[order], P.base.counts[order])
    assert lc.bulk_lines(capfd) == []
    return c


def w_bulk_reads(R, P, mp, capfd, content="high"):
    """a fresh bulk build from reads: dense on the shapes the bulk build takes, the probing path's table on the others"""
    env_bulk(mp)
    c = R.table()
    capfd.readouterr()
    add_device(R, c, content)
    bulk_line(capfd, P, "bulk build from reads", "build", "dense")
    return c


def w_bulk_routed(R, P, mp, capfd):
    env_bulk(mp)
    c = R.table()
    keys = np.repeat(P.base.keys, P.base.counts.astype(np.int64))
    keys = keys[np.random.default_rng(6).permutation(len(keys))]
    capfd.readouterr()
    c.add_pairs_host(keys, None)
    bulk_line(capfd, P, "bulk build from routed keys", "build", "dense")
    return c


def w_bulk_merge(R, P, mp, capfd):
    env_bulk(mp)
    c = R.table()
    capfd.readouterr()
    add_device(R, c, "half0")
    bulk_line(capfd, P, "first half", "build", "dense")
    add_device(R, c, "half1")
    bulk_line(capfd, P, "second half", "merge")
    return c


def w_add_file(R, P, mp, capfd, tmp_path):
    env_probing(mp)
    src = R.file_source()
    src.add_pairs_host(P.base.keys, P.base.counts)
    path = str(tmp_path / "base.ktab")
    assert src.save(path) == P.base.size
    c = R.table()
    assert c.add_file(path) == P.base.size
    return c


def w_cleared_after_overflow(R, P, mp, capfd):
    from kmertools_amd._lib import KT_ERR_FULL
    env_probing(mp)
    c = R.table()
    many = np.arange(1, P.g.cap + 700, dtype=np.uint64) * np.uint64(7919)
    many = np.unique(tm.gr.canon_np(many & np.uint64((1 << (2 * P.k)) - 1), P.k))
    assert len(many) > P.g.cap
    c.add_pairs_host(many, np.ones(len(many), np.uint32))
    refused(c.size, KT_ERR_FULL, "an overflowed table")
    c.clear()
    order = np.random.default_rng(8).permutation(P.base.size)
    c.add_pairs_host(P.base.keys[order], P.base.counts[order])
    return c


PLAIN_WRITERS = {"probing_reads": w_probing_reads, "probing_pairs": w_probing_pairs, "bulk_reads": w_bulk_reads,
                 "bulk_routed": w_bulk_routed, "bulk_merge": w_bulk_merge, "cleared_after_overflow": w_cleared_after_overflow}


def finish(R, P, c, names, tag):
    """every table reader on the base content, the pairs on top (the u32 edges), every reader, the absent keys"""
    check(R, c, ref_of(P, "base"), [n for n in names if n not in GRAPH_PROBERS], tag + " (the reads' content)")
    absent_are_absent(R, c, tag)
    c.add_pairs_host(*P.pairs)
    check(R, c, ref_of(P, "high"), names, tag + " (the pairs on top)")
    absent_are_absent(R, c, tag)
    assert same(c.lookup_host(P.edge_keys), np.array([255, 256, U32] * 3, np.uint32)), tag


@pytest.mark.gpu
@pytest.mark.parametrize("writer", list(PLAIN_WRITERS))
@pytest.mark.parametrize("request_,k", MAIN)
def test_every_writer_then_every_reader(rig, monkeypatch, capfd, request_, k, writer):
    """on the shapes of fewer than four ranges the bulk writers assert that the build declined: the probing path answers"""
    R = rig(request_, k)
    P = R.P
    c = PLAIN_WRITERS[writer](R, P, monkeypatch, capfd)
    finish(R, P, c, readers_for(True), "request %d k=%d writer %s" % (request_, k, writer))


@pytest.mark.gpu
@pytest.mark.parametrize("writer", ["probing_reads", "bulk_reads"])
@pytest.mark.parametrize("request_,k", SECOND)
def test_the_other_key_width(rig, monkeypatch, capfd, request_, k, writer):
    R = rig(request_, k)
    P = R.P
    c = PLAIN_WRITERS[writer](R, P, monkeypatch, capfd)
    finish(R, P, c, readers_for(False), "request %d k=%d writer %s" % (request_, k, writer))


@pytest.mark.gpu
@pytest.mark.parametrize("request_,k", MAIN)
def test_add_file_of_a_table_saved_from_another_shape(rig, monkeypatch, capfd, tmp_path, request_, k):
    R = rig(request_, k)
    c = w_add_file(R, R.P, monkeypatch, capfd, tmp_path)
    finish(R, R.P, c, readers_for(True), "request %d k=%d writer add_file" % (request_, k))


@pytest.mark.gpu
@pytest.mark.parametrize("content", ["high", "low"])
@pytest.mark.parametrize("order", ["walkers_first", "probers_first"])
@pytest.mark.parametrize("request_,k", BULK_MAIN + [(20000, 15)])
def test_dense_build_read_while_dense_and_after_the_first_prober(rig, monkeypatch, capfd, request_, k, order, content):
    """a fresh bulk build leaves every range packed at the front of its slots: the walkers read that form when they come
    first; the first prober rewrites the table in place as the probing image (materialize_kernel places every key by the
    shape's m8) and the walkers then read the image.  `low`: so few k-mers per range that the build keeps claim lists,
    `high`: the packed variant."""
    R = rig(request_, k)
    P = R.P
    tag = "request %d k=%d dense %s %s" % (request_, k, content, order)
    c = w_bulk_reads(R, P, monkeypatch, capfd, content)
    ref = ref_of(P, "base" if content == "high" else "low")
    probers = TABLE_PROBERS + (GRAPH_PROBERS if (request_, k) in MAIN else ())
    for names in ((WALKERS, probers, WALKERS) if order == "walkers_first" else (probers[:1], WALKERS, probers)):
        check(R, c, ref, names, tag)
    absent_are_absent(R, c, tag)
    # every prober as the first one on a dense table of its own would be the lifecycle test over again: here each of the
    # probers that image the table through its own entry point is the first once, on the m8 = 5 shape
    if request_ == 20000 and order == "probers_first":
        for name in ("compare(partner, t)", "xor(t, partner)", "graph(1)", "cov", "hetmers", "unitigs+links")[:4 if k == 15 else 6]:
            d = w_bulk_reads(R, P, monkeypatch, capfd, content)
            check(R, d, ref, (name,) + WALKERS[:3], tag + " first prober " + name)
            d.close()


@pytest.mark.gpu
@pytest.mark.parametrize("request_,k", BULK_MAIN)
def test_bulk_build_into_an_export_target(rig, monkeypatch, capfd, request_, k):
    R = rig(request_, k)
    P, torch = R.P, R.torch
    tag = "request %d k=%d export target" % (request_, k)
    ref = ref_of(P, "base")
    n = ref.m.size
    room = n + 9
    xk, xc = R.full(room + lc.GUARD, lc.KPAT, 64), R.full(room + lc.GUARD, lc.CPAT, 32)
    env_bulk(monkeypatch)
    c = R.table()
    c.export_target(xk, xc, room)
    capfd.readouterr()
    add_device(R, c, "high")
    bulk_line(capfd, P, tag, "build", "dense-ext")
    check(R, c, ref, WALKERS, tag)
    torch.cuda.synchronize()
    hk, hc = lc.u64(xk), lc.u32(xc)
    # (what the arrays hold between the entries and max_out is unspecified; they are never written past max_out)
    assert (hk[room:] == lc.KPAT).all() and (hc[room:] == lc.CPAT).all(), tag
    gk, gc = lc.by_key(hk[:n], hc[:n])
    assert same(gk, ref.m.keys) and same(gc, ref.m.counts), tag
    check(R, c, ref, readers_for(True), tag + " imaged")
    c.export_target(None, None, 0)
    finish(R, P, c, WALKERS + TABLE_PROBERS, tag + " target dropped")


@pytest.mark.gpu
@pytest.mark.parametrize("request_,k", MAIN)
def test_erase_a_third_then_add_half_of_it_back(rig, monkeypatch, capfd, request_, k):
    """the erased keys include, per clustered range, the first and a middle cluster key, the keys either side of the wrap
    and whatever sits in the range's last and first slot; the rebuild behind the erase places the survivors again"""
    R = rig(request_, k)
    P = R.P
    tag = "request %d k=%d erase" % (request_, k)
    for form in ("probing", "bulk"):
        c = (w_probing_pairs if form == "probing" else w_bulk_reads)(R, P, monkeypatch, capfd)
        c.add_pairs_host(*P.pairs)
        arg = np.concatenate([P.gone, P.gone[:7], P.absent[:50], np.array([2 ** 64 - 1, 4 ** k], np.uint64)])
        assert c.erase(arg) == len(P.gone), (tag, form)
        check(R, c, ref_of(P, "erased"), readers_for(form == "probing"), tag + " " + form)
        assert not c.lookup_host(P.gone).any(), (tag, form)
        absent_are_absent(R, c, tag)
        c.add_pairs_host(*P.back)
        check(R, c, ref_of(P, "erased_back"), readers_for(False), tag + " " + form + " half back")
        assert not c.lookup_host(np.setdiff1d(P.gone, P.back[0])).any(), (tag, form)
        c.close()


# ---- on a copy: clip_tips, simplify, the table as an index of its own unitigs -------------------------------------------------------

def copy_of_high(R, monkeypatch):
    """(a fresh table of the plan's shape that holds the high content, its Ref, the content as strings, unitigs, links)"""
    ref = ref_of(R.P, "high")
    env_probing(monkeypatch)
    c = R.table()
    c.add_pairs_host(ref.m.keys, ref.m.counts)
    return (c, ref) + graph_strings(R, ref)


@pytest.mark.gpu
@pytest.mark.parametrize("request_,k", MAIN)
def test_clip_tips_on_a_copy(rig, monkeypatch, request_, k):
    """tips and isolated short unitigs erased in place; every round of the restatement walks the whole table's strings:
    two rounds at most, one on the shapes above 2^15 slots"""
    R = rig(request_, k)
    c, ref, table, us, ls = copy_of_high(R, monkeypatch)
    rounds = 2 if R.P.g.cap <= 32768 else 1
    left, stats, _ = ref.memo("clip", lambda: tr.clip(table, k, k, rounds, True))
    got = c.clip_tips(k, rounds, True)
    want = dict(zip(tr.STATS, stats[:6] + [1 - stats[6]]))
    assert {n: got[n] for n in want} == want, (request_, k, got, want)
    assert want["tips"] > 0 and want["isolated"] > 0
    gk, gc = c.export_host()
    assert ce.strings_of(gk, gc, k) == left, (request_, k)


@pytest.mark.gpu
@pytest.mark.parametrize("request_,k", MAIN)
def test_simplify_on_a_copy(rig, monkeypatch, request_, k):
    """one round of both rules"""
    R = rig(request_, k)
    c, ref, table, us, ls = copy_of_high(R, monkeypatch)
    left, stats, _ = ref.memo("simplify", lambda: br.simplify(table, k, k, 2 * k, 1, False))
    got = c.simplify(k, 2 * k, 1, False)
    want = dict(zip(br.STATS, list(stats[:9]) + [1 - stats[9]]))
    assert {n: got[n] for n in want} == want, (request_, k, got, want)
    assert want["tips"] > 0
    gk, gc = c.export_host()
    assert ce.strings_of(gk, gc, k) == left, (request_, k)


@pytest.mark.gpu
@pytest.mark.parametrize("request_,k", MAIN)
def test_the_table_as_the_index_of_its_own_unitigs(rig, monkeypatch, request_, k):
    """index_sequences of the high content's unitigs into a table of the same shape - as many keys with the same homes,
    their values positions - and thread_hits of a few reads"""
    R = rig(request_, k)
    P = R.P
    ref = ref_of(P, "high")
    _, us, ls = graph_strings(R, ref)
    ub, uo = thr.csr([u[0] for u in us])
    qb, qo = P.csr["profile"]
    want_hits = thr.hits_np(thr.index_np(ub, uo, k), qb, qo, k)
    t = R.table()
    assert t.index_sequences_host(ub, uo) == ref.m.size
    assert same(t.thread_hits_host(qb, qo), want_hits)
    assert int(((want_hits != 0) & (want_hits != NO)).sum()) > 20 and int((want_hits == 0).sum()) > 0
    gk, gc = t.export_host()
    assert same(gk, ref.m.keys)


# ---- table files: the bytes depend on k and the entries alone ------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("request_,k", MAIN)
def test_table_files_are_byte_identical_from_every_shape_and_form(rig, monkeypatch, capfd, tmp_path, request_, k):
    R = rig(request_, k)
    P = R.P
    want = ktab_ref.encode(k, P.base.keys, P.base.counts)
    want_high = ktab_ref.encode(k, P.high.keys, P.high.counts)
    forms = [("probing", w_probing_pairs), ("bulk, dense", w_bulk_reads), ("bulk, merged", w_bulk_merge)]
    for name, writer in forms:
        c = writer(R, P, monkeypatch, capfd)
        path = str(tmp_path / "t.ktab")
        assert c.save(path) == P.base.size, (request_, k, name)
        with open(path, "rb") as f:
            assert f.read() == want, "request %d k=%d: the file saved from the %s table is not ktab_ref's" % (request_, k, name)
        if name == "bulk, dense":  # ... and from the probing image the first prober made of it
            assert same(c.lookup_host(P.edge_keys), P.base.count(P.edge_keys))
            assert c.save(path) == P.base.size
            with open(path, "rb") as f:
                assert f.read() == want, (request_, k, "imaged")
        c.add_pairs_host(*P.pairs)  # counts of 255 and more are the file's overflow entries
        assert c.save(path) == P.high.size
        with open(path, "rb") as f:
            assert f.read() == want_high, (request_, k, name, "the pairs on top")
        c.close()
    # the other shape's file of the same content
    src = R.file_source()
    src.add_pairs_host(P.base.keys, P.base.counts)
    path = str(tmp_path / "o.ktab")
    src.save(path)
    with open(path, "rb") as f:
        assert f.read() == want


# ---- brim: a range, not the table, must have room ---------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("path", ["probing", "bulk"])
@pytest.mark.parametrize("request_,k", MAIN + [(20000, 15), (81920, 21)])
def test_one_range_filled_to_the_brim(rig, monkeypatch, capfd, request_, k, path):
    """one range holds exactly as many keys as it has slots, all homed in it, the others 60 keys each: everything is
    found, absent keys of the full range are absent after one trip round it, one more key of that range is KT_ERR_FULL -
    and would have fitted had the restated home_of named another range.  After clear() the table works again."""
    from kmertools_amd._lib import KT_ERR_FULL
    R = rig(request_, k)
    P = R.P
    tag = "request %d k=%d brim %s" % (request_, k, path)
    c = R.table()
    if path == "probing":
        env_probing(monkeypatch)
        c.add_pairs_host(P.brim.keys, P.brim.counts)
        m = P.brim
    else:
        env_bulk(monkeypatch)
        capfd.readouterr()
        add_device(R, c, "brim")
        bulk_line(capfd, P, tag, "build", "dense")
        m = P.brim_read_model
    assert P.brim.size < 0.5 * P.g.cap or P.g.n_ranges <= 2
    ref = lc.Ref(m)
    check(R, c, ref, ("size", "export_host", "export_device", "stage_pieces", "spectrum_host"), tag)
    assert same(c.lookup_host(m.keys), m.counts), tag
    assert len(P.brim_absent) <= 64 and not c.lookup_host(P.brim_absent).any(), tag
    assert not c.lookup_host(P.brim_extra).any(), tag
    check(R, c, ref, ("size", "export_host"), tag + " after the look-ups")
    # one more key of the full range
    if path == "probing":
        c.add_pairs_host(P.brim_extra, np.ones(1, np.uint32))
    else:
        one = tg.reads_of(P.brim_extra, [1], k, np.random.default_rng(1))
        from kmertools_amd.device import to_csr
        c.add_reads_host(*to_csr(one + one))
    refused(c.size, KT_ERR_FULL, tag + ": one key more than the range has slots")
    c.clear()
    env_probing(monkeypatch)
    c.add_pairs_host(P.brim_others, np.ones(len(P.brim_others), np.uint32))
    c.add_pairs_host(P.brim_extra, np.full(1, 3, np.uint32))
    after = tm.Model(k)
    after.add_pairs(np.concatenate([P.brim_others, P.brim_extra]), np.concatenate([np.ones(len(P.brim_others), np.uint32), [3]]))
    check(R, c, lc.Ref(after), ("size", "export_host", "lookup"), tag + " after clear")
    assert c.lookup_host(P.brim_extra)[0] == 3


# ---- the narrow hash's corners: n = 2k and n > 2k on an m8 = 5 shape, never the direct-addressed build ----------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("request_,k", [(40000, 8), (20000, 7)])
def test_all_canonical_kmers_of_a_small_k_on_an_m8_5_table(rig, torch_mod, oracle, monkeypatch, capfd, request_, k):
    """k = 8 at 40 960 slots: n = 16 = 2k hash bits, all 32 896 canonical 8-mers, load 0.80; k = 7 at 20 480 slots: n = 15 is
    more than the 14 bits a 7-mer has.  A fresh bulk build gives the oracle's table, a second batch twice the counts, and
    the build's verbose line does not name the direct variant (that one needs m8 = 8 and exactly 4^k slots)."""
    from kmertools_amd import device
    g = tm.geometry(request_, k)
    assert g.m8 == 5 and (g.n == 2 * k if k == 8 else g.n > 2 * k)
    x = np.arange(4 ** k, dtype=np.uint64)
    keys = np.unique(tm.gr.canon_np(x, k))
    assert len(keys) == {8: 32896, 7: 8192}[k]
    L = tm.layout(keys, k, g)  # (no range over its slots: layout would have raised)
    rng = np.random.default_rng(k)
    counts = rng.integers(1, 4, size=len(keys))
    seqs = tg.reads_of(keys, counts, k, rng) + [b"ACGTN" * 30, b"A" * 100]
    bases, offsets = device.to_csr(seqs)
    wk, wc = oracle.count_reads(bases, offsets, k)
    assert same(wk, keys) and int(L.fill.sum()) == len(keys)
    ctx = device.Context(0, stream=torch_mod.cuda.current_stream().cuda_stream)
    try:
        lc.env_bulk(monkeypatch)
        c = device.Counter(ctx, k, request_)
        assert c.capacity() == g.cap
        capfd.readouterr()
        c.add_reads_host(bases, offsets)
        lines = lc.bulk_lines(capfd)
        assert len(lines) == 1 and lines[0].split()[5] == "build" and lines[0].split()[-1] == "build=dense", lines
        gk, gc = c.export_host()
        assert same(gk, wk) and same(gc, wc)
        assert same(c.lookup_host(keys[::-1]), wc[::-1])
        c.add_reads_host(bases, offsets)
        lines = lc.bulk_lines(capfd)
        assert len(lines) == 1 and lines[0].split()[5] == "merge" and "direct" not in lines[0], lines
        gk, gc = c.export_host()
        assert same(gk, wk) and same(gc, 2 * wc)
        hist, tot = c.spectrum(8, totals=True)
        assert same(hist, lc.tm.want_spectrum(2 * wc, 8)) and tot == (len(wk), int(2 * wc.astype(np.uint64).sum()))
        c.close()
    finally:
        ctx.close()
