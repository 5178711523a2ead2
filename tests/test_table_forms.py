"""What becomes of a staged export, in every form a table can be in, after every kind of call.

A kt_ctr is in one of four forms (kt_internal.hpp, DESIGN.md "The table's forms"): Stale (cleared, the clear still pending over
old data), Image (the probing image), Dense (packed ranges, what a fresh bulk build leaves) and Target (the entries are the
caller's export-target arrays).  kt_ctr_export_stage[_range] stages the entries - into the table's own buffers, or, for the
unfiltered stage of a Target-form table, by pointing at the target's arrays - and kt_ctr_export_fetch hands them out until a
call ends the stage.  tests/test_table_lifecycle.py accepts either outcome of a fetch after such a call (fetch_or_refuse);
here the outcome is fixed, per form, per stage and per call:

  a walker (spectrum), an add of no reads, add_pairs of no pairs      the stage stays
  a prober (lookup), an erase that finds none of its keys             the stage stays - but the table is imaged, and the
                                                                      unfiltered stage of a Target-form table were the
                                                                      target's arrays, which are the caller's again: refused
  an add of reads without bases, a probing add, a bulk add,
  add_pairs, an erase that removes something, clear,
  export_target (the same arrays, other arrays, none)                 the stage is gone: KT_ERR_ARG
  a second stage                                                      replaces the first

A cleared table stages nothing, and a fetch of nothing is never refused.  After every call the table's size and sorted
export are the model's (tests/table_model.py).  One table of the lifecycle test's 2^17 slots per case; everything is integers."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import table_model as tm  # noqa: E402
import test_table_lifecycle as tl  # noqa: E402

FORMS = ("stale", "image", "dense", "target")
STAGES = {"all": 1, "min2": 2}  # the stage's min_count


@pytest.fixture(scope="module")
def rigs():
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


def build(R, mp, capfd, form):
    """a table in `form`, reached as the lifecycle test reaches it, and the model of its content"""
    P = R.P
    c, m = R.counter(tl.SLOTS), tm.Model(P.k)
    if form == "stale":
        tl.env_probing(mp)
        c.add_reads_host(*P.csr["small5"])
        c.clear()
    elif form == "image":
        tl.env_probing(mp)
        c.add_reads_host(*P.csr["small2"])
        m.add_reads(*P.csr["small2"])
    else:
        if form == "target":
            c.export_target(R.full(P.target_room, tl.KPAT, 64), R.full(P.target_room, tl.CPAT, 32), P.target_room)
        tl.env_bulk(mp)
        capfd.readouterr()
        tl.add_device(R, c, "bulk1")
        lines = tl.bulk_lines(capfd)  # (one line, a build: nothing was redone into the table)
        assert len(lines) == 1 and lines[0].split()[5] == "build", lines
        m.add_reads(*P.csr["bulk1"])
    return c, m


# ---- the events: each applies one call to the table and the model --------------------------------------------------------

def e_spectrum(R, mp, c, m):
    hist = np.zeros(tl.N_BINS, np.uint64)
    from kmertools_amd._lib import KT_MEM_HOST
    c.spectrum_into(hist, tl.N_BINS, None, KT_MEM_HOST)
    assert tl.same(hist, m.spectrum(tl.N_BINS)[0])


def e_lookup(R, mp, c, m):
    keys = np.concatenate([m.keys[::5][:500], R.P.absent[:500]])
    assert tl.same(c.lookup_host(keys), m.count(keys))


def e_add_no_reads(R, mp, c, m):
    from kmertools_amd._lib import KT_MEM_HOST
    c.add_reads(np.zeros(1, np.uint8), np.zeros(1, np.uint64), 0, KT_MEM_HOST)


def e_add_no_bases(R, mp, c, m):
    from kmertools_amd._lib import KT_MEM_HOST
    c.add_reads(np.zeros(1, np.uint8), np.zeros(3, np.uint64), 2, KT_MEM_HOST)


def e_probing_add(R, mp, c, m):
    tl.env_probing(mp)
    c.add_reads_host(*R.P.csr["small8"])
    m.add_reads(*R.P.csr["small8"])


def e_bulk_add(R, mp, c, m):
    tl.env_bulk(mp)
    tl.add_device(R, c, "bulk2")
    m.add_reads(*R.P.csr["bulk2"])


def e_pairs_none(R, mp, c, m):
    from kmertools_amd._lib import KT_MEM_HOST
    c.add_pairs(R.P.pairs3[0][:1].copy(), R.P.pairs3[1][:1].copy(), 0, KT_MEM_HOST)


def e_pairs_some(R, mp, c, m):
    pk, pc = R.P.pairs3[0][:300], R.P.pairs3[1][:300]
    c.add_pairs_host(pk, pc)
    m.add_pairs(pk, pc)


def e_erase_absent(R, mp, c, m):
    gone = R.P.cluster[24:]  # (keys that are never in any table of the plan)
    assert not m.count(gone).any() and c.erase(gone) == 0


def e_erase_present(R, mp, c, m):
    gone = m.keys[::3]
    assert c.erase(np.concatenate([gone, R.P.cluster[24:]])) == len(gone)
    keep = ~np.isin(m.keys, gone)
    m.keys, m.counts = m.keys[keep], m.counts[keep]


def e_clear(R, mp, c, m):
    c.clear()
    m.clear()


def e_target_same(R, mp, c, m):
    xt = getattr(c, "_xt", None)
    c.export_target(xt[0] if xt else None, xt[1] if xt else None, R.P.target_room)


def e_target_other(R, mp, c, m):
    c.export_target(R.full(R.P.walk_room, tl.KPAT2, 64), R.full(R.P.walk_room, tl.CPAT2, 32), R.P.walk_room)


def e_target_none(R, mp, c, m):
    c.export_target(None, None, 0)


KEEPS, IMAGES, DROPS = "keeps", "images", "drops"  # what a call does to the stage ("images": see the table at the top)
EVENTS = {
    "spectrum": (e_spectrum, KEEPS), "lookup": (e_lookup, IMAGES),
    "add_no_reads": (e_add_no_reads, KEEPS), "add_no_bases": (e_add_no_bases, DROPS),
    "probing_add": (e_probing_add, DROPS), "bulk_add": (e_bulk_add, DROPS),
    "pairs_none": (e_pairs_none, KEEPS), "pairs_some": (e_pairs_some, DROPS),
    "erase_absent": (e_erase_absent, IMAGES), "erase_present": (e_erase_present, DROPS),
    "clear": (e_clear, DROPS),
    "target_same": (e_target_same, DROPS), "target_other": (e_target_other, DROPS), "target_none": (e_target_none, DROPS),
    "second_stage": (None, None),
}


@pytest.mark.gpu
@pytest.mark.parametrize("event", sorted(EVENTS))
@pytest.mark.parametrize("stage", sorted(STAGES))
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("k", [15, 31])
def test_fetch_after_one_call(rigs, oracle, monkeypatch, capfd, k, form, stage, event):
    from kmertools_amd._lib import KT_ERR_ARG
    R = rigs(k)
    tag = "k=%d %s table, %s staged, then %s" % (k, form, stage, event)
    c, m = build(R, monkeypatch, capfd, form)
    try:
        lo = STAGES[stage]
        wk, wc = m.stage(lo)
        n = c.export_stage_range(lo, None)
        assert n == len(wk), tag
        assert (n == 0) == (form == "stale"), tag  # (every other form holds entries, and entries seen twice)
        if event == "second_stage":
            lo2 = STAGES["min2" if stage == "all" else "all"]
            wk, wc = m.stage(lo2)
            n = c.export_stage_range(lo2, None)
            assert n == len(wk), tag
            alive = True
        else:
            fn, effect = EVENTS[event]
            fn(R, monkeypatch, c, m)
            torch_sync(R)
            alive = effect == KEEPS or (effect == IMAGES and not (form == "target" and stage == "all"))
        if alive or n == 0:
            gk, gc = tl.by_key(*c.export_fetch(0, n))
            assert tl.same(gk, wk) and tl.same(gc, wc), tag + ": the fetch is not what was staged"
        else:
            tl.refused(lambda: c.export_fetch(0, n), KT_ERR_ARG, tag)
        tl.refused(lambda: c.export_fetch(0, n + 1), KT_ERR_ARG, tag)
        assert c.size() == m.size, tag
        gk, gc = c.export_host()
        assert tl.same(gk, m.keys) and tl.same(gc, m.counts), tag + ": the content afterwards"
    finally:
        c.close()


def torch_sync(R):
    R.torch.cuda.synchronize()
