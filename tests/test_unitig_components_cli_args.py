"""`kmertools unitigs --components` and `kmertools thread --components` on the CPU: the help texts name the flag, the files and
their fields; a value behind the flag is refused, exit 2 with a clap-style message before any device is opened or the directory is
made; the flag passes with --stats-only, --gfa, --links, --clip-tips and --pop-bubbles; the binding declares both calls.  And the
reference the GPU tests compare against (tests/component_ref.py): it reproduces the worked answers of
tests/golden/components_known.json, keeps its assertions (the union-find and the breadth-first search agree - asserted inside
every call -, every link's two unitigs share a component, first occurrences ascend, the columns of stats sum to the totals) over
a few hundred random small tables (k = 2..7 and 9, alphabets of two letters, circularised genomes, hairpins, min_count 1 and 2),
its synchronous play of the round scheme ends on the same labels, and its read fold and file formats hold on worked rows."""
import functools
import json
import pathlib
import sys

import numpy as np
import pytest

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests"))
import component_ref as cr  # noqa: E402
import graph_ref as gr  # noqa: E402
import test_ctr_clip_tips_cli_args as tca  # noqa: E402  (its cli fixture, run() and random_reads())
import unitig_link_ref as lr  # noqa: E402

cli = tca.cli
run = tca.run
FASTA = ">a\nACGTACGTACGTACGTACGTACGTACGTAAACCCGGGTTT\n"


@pytest.fixture(scope="module", autouse=True)
def the_library_has_the_calls():
    """the reference below is the yardstick of two calls of the library: without them nothing here has anything to measure"""
    from kmertools_amd import _lib
    missing = [name for name in ("kt_unitig_components", "kt_thread_read_components") if name not in _lib.SYMBOLS]
    assert not missing, "the binding does not declare %s" % missing


def test_unitigs_help_names_the_components_flag(cli):
    for h in ("--help", "-h"):
        r = run(cli, "unitigs", h)
        assert r.returncode == 0
        for text in ("--components", "unitigs.components", "unitigs.components.stats", "unitigs.links.stats",
                     "component<TAB>unitigs<TAB>nodes<TAB>bases<TAB>count_sum<TAB>km<TAB>links<TAB>first_unitig",
                     "components, singletons (components of one unitig), largest_unitigs, largest_nodes and largest_share",
                     "CC:i:{component}", "(allowed with --stats-only)", "numbered by their", "--clip-tips / --pop-bubbles"):
            assert text in r.stdout, text


def test_thread_help_names_the_components_flag(cli):
    for h in ("--help", "-h"):
        r = run(cli, "thread", h)
        assert r.returncode == 0
        for text in ("--components", "thread.reads", "thread.components", "unitigs.components", "name<TAB>component|*<TAB>mixed<TAB>hits",
                     "component<TAB>unitigs<TAB>nodes<TAB>reads<TAB>hits", "reads_with_component, reads_mixed, components_hit",
                     "unitigs --gfa --components", "CC:i:"):
            assert text in r.stdout, text


@pytest.mark.parametrize("command, extra, what", [
    ("unitigs", ("--components", "yes"), "yes"),
    ("unitigs", ("--component",), "--component"),
    ("thread", ("--components", "yes"), "yes"),
    ("thread", ("--components", "--gfa"), "--gfa"),
    ("unitigs", ("--components", "--stats-only", "--gfa"), "--stats-only"),
])
def test_component_flags_that_are_refused(cli, tmp_path, command, extra, what):
    fa, out = tmp_path / "a.fa", tmp_path / "out"
    fa.write_text(FASTA)
    r = run(cli, command, "-i", fa, "-o", out, "-k", "15", *extra)
    assert r.returncode == 2 and r.stderr.startswith("error: ") and what in r.stderr, r.stderr
    assert "For more information, try '--help'." in r.stderr
    assert not out.exists()


@pytest.mark.parametrize("command, extra", [
    ("unitigs", ("--components",)), ("unitigs", ("--components", "--stats-only")), ("unitigs", ("--components", "--gfa", "--links")),
    ("unitigs", ("--components", "--clip-tips", "--pop-bubbles")), ("thread", ("--components",)), ("thread", ("--components", "--stats-only")),
])
def test_component_flags_that_pass(cli, tmp_path, command, extra):
    """the arguments are taken: the run gets as far as the device (and, where there is one, through)"""
    fa, out = tmp_path / "a.fa", tmp_path / "out"
    fa.write_text(FASTA)
    r = run(cli, command, "-i", fa, "-o", out, "-k", "15", *extra)
    assert r.returncode in (0, 101) and not r.stderr.startswith("error: "), r.stderr
    assert out.exists()


def test_the_binding_declares_the_calls():
    from kmertools_amd import _lib, device
    for name in ("unitig_components", "unitig_components_host", "thread_read_components", "thread_read_components_host"):
        assert callable(getattr(device.Context, name)), name
    assert callable(device.Counter.unitig_components)
    assert device.NO_COMPONENT == cr.NO_COMPONENT == 0xFFFFFFFF and device.COMPONENT_FIELDS == len(cr.FIELDS) == 5
    assert device.COMPONENT_STATS_NAMES == cr.FIELDS
    for name in ("kt_unitig_components", "kt_thread_read_components"):
        assert name in _lib.SYMBOLS and hasattr(_lib.lib(), name)
    header = (ROOT / "include" / "kmertools_hip.h").read_text()
    for text in ("#define KT_NO_COMPONENT 0xFFFFFFFFu", "#define KT_COMPONENT_FIELDS 5", "#define KT_COMPONENT_TALLY 6",
                 "#define KT_READ_COMPONENT_TALLY 4"):
        assert text in header, text
    assert (_lib.KT_NO_COMPONENT, _lib.KT_COMPONENT_FIELDS, _lib.KT_COMPONENT_TALLY, _lib.KT_READ_COMPONENT_TALLY) == (0xFFFFFFFF, 5, 6, 4)


# ---- the reference ----------------------------------------------------------------------------------------------------------

KNOWN = json.loads((ROOT / "tests" / "golden" / "components_known.json").read_text())["cases"]


def arrays_of(table, k, lo=1):
    us, ls = lr.links(table, k, lo)
    loff, lto = lr.as_arrays(ls)
    off = np.cumsum([0] + [len(u[0]) for u in us]).astype(np.uint64)
    return us, ls, loff, lto, off, np.array([u[1] for u in us], np.uint64)


@pytest.mark.parametrize("case", KNOWN, ids=lambda c: c["name"])
def test_reference_reproduces_the_worked_answers(case):
    k = case["k"]
    us, ls, loff, lto, off, sums = arrays_of(gr.count_strings(case["reads"], k), k)
    assert [u[0] for u in us] == case["unitigs"] and ls == case["links"]
    got = cr.components(loff, lto, off, sums, k)
    assert got["component"].tolist() == case["component"]
    assert got["stats"].tolist() == case["stats"] and got["tally"].tolist() == case["tally"] + [0]
    labels, rounds = cr.sync_rounds(loff, lto)
    assert [case["stats"][c][4] for c in case["component"]] == labels.tolist() and 1 <= rounds <= 3


def test_the_worked_answers_cover_the_definition():
    by = {c["name"]: c for c in KNOWN}
    assert sorted(by) == ["a bubble", "a cycle", "a fork with a tip", "a hairpin", "two genomes with no shared k-mer"]
    assert by["a cycle"]["links"] == [[0], [1]] and by["a cycle"]["stats"] == [[1, 3, 15, 2, 0]]  # its two closing links join nothing
    assert by["a hairpin"]["links"] == [[], [0]] and by["a hairpin"]["stats"][0][3] == 1
    assert by["a fork with a tip"]["component"] == [0, 0, 0] and by["a fork with a tip"]["tally"] == [1, 0, 3, 13, 0]
    assert by["a bubble"]["stats"] == [[4, 18, 26, 8, 0]]
    two = by["two genomes with no shared k-mer"]
    assert two["component"] == [0, 1, 1, 1] and two["tally"] == [2, 1, 3, 13, 0] and two["stats"][1][4] == 1
    assert two["stats"][1][:4] == by["a fork with a tip"]["stats"][0][:4]  # the same graph beside another one


SWEEP_KS = (2, 3, 4, 5, 6, 7, 9)


@functools.lru_cache(maxsize=None)
def sweep(k):
    """48 random tables at k through the reference -> what they held"""
    seen = dict(tables=0, several=0, singletons=0, big=0, self_links=0, slow=0)
    rng = np.random.default_rng(5100 + k)
    for trial in range(24):
        reads = tca.random_reads(rng, k, "ACGT" if trial % 3 else "AC")
        reads += ["".join(rng.choice(list("ACGT"), size=k + int(rng.integers(0, 6)))) for _ in range(int(rng.integers(0, 4)))]
        table = gr.count_strings(reads, k)
        for lo in (1, 2):
            us, ls, loff, lto, off, sums = arrays_of(table, k, lo)
            got = cr.components(loff, lto, off, sums, k)
            comp, stats, tally = got["component"], got["stats"], got["tally"]
            cr.check_labels(loff, lto, comp)
            for e, fs in enumerate(ls):  # every link's two unitigs share a component
                assert all(comp[e >> 1] == comp[f >> 1] for f in fs)
            nc = len(stats)
            assert nc == (int(comp.max()) + 1 if len(us) else 0) == int(tally[0])
            assert [int(x) for x in stats.sum(axis=0)[:4]] == [len(us), sum(u[3] for u in us), sum(u[1] for u in us), len(lto)] or not nc
            assert all(int(stats[c][4]) == int(np.flatnonzero(comp == c)[0]) for c in range(nc))
            assert int(tally[1]) == int((stats[:, 0] == 1).sum()) and int(tally[4]) == 0
            if nc:
                assert int(tally[2]) == int(stats[:, 0].max()) and int(tally[3]) == int(stats[:, 1].max())
            labels, rounds = cr.sync_rounds(loff, lto)
            assert labels.tolist() == [int(stats[c][4]) for c in comp] and rounds <= len(us) + 1
            seen["tables"] += 1
            seen["several"] += nc >= 2
            seen["singletons"] += int(tally[1]) > 0
            seen["big"] += nc > 0 and int(tally[2]) >= 5
            seen["self_links"] += any(f >> 1 == e >> 1 for e, fs in enumerate(ls) for f in fs)
            seen["slow"] += rounds >= 3
    return seen


@pytest.mark.parametrize("k", SWEEP_KS)
def test_the_reference_keeps_its_assertions(k):
    assert sweep(k)["tables"] == 48


def test_the_sweep_saw_what_it_is_for():
    seen = {name: sum(sweep(k)[name] for k in SWEEP_KS) for name in sweep(SWEEP_KS[0])}
    assert seen["tables"] == 7 * 48 and all(seen.values()), seen
    assert seen["several"] > 100 and seen["self_links"] > 50, seen


def test_bad_links_and_missing_mirrors_in_the_reference():
    # 4 unitigs: 0 -> 2 without a mirror, 1 alone with a link to itself, 3 with two bad links
    loff, lto = lr.as_arrays([[4], [], [2], [], [], [], [8, 0xFFFFFFFF], []])
    got = cr.components(loff, lto, np.array([0, 10, 30, 35, 50], np.uint64), np.array([7, 8, 9, 10], np.uint64), 5)
    assert got["component"].tolist() == [0, 1, 0, 2]
    assert got["stats"].tolist() == [[2, 7, 16, 1, 0], [1, 16, 8, 1, 1], [1, 11, 10, 0, 3]] and got["tally"].tolist() == [3, 2, 2, 16, 2, 0]
    none = cr.components(np.zeros(1, np.uint64), np.zeros(0, np.uint32))
    assert none["component"].shape == (0,) and none["stats"].shape == (0, 5) and not none["tally"].any()
    assert cr.sync_rounds(np.zeros(1, np.uint64), np.zeros(0, np.uint32))[1] == 0


def test_the_synchronous_play_on_a_path():
    """a path numbered along its length is the worst case of plain label propagation (as many rounds as unitigs); the two hooks
    and the shortcut take a logarithmic number"""
    for n in (2, 3, 17, 256, 1000):
        ls = [[] for _ in range(2 * n)]
        for u in range(n - 1):
            ls[2 * u].append(2 * u + 2)
            ls[2 * u + 3].append(2 * u + 1)
        labels, rounds = cr.sync_rounds(*lr.as_arrays(ls))
        assert not labels.any() and rounds <= 2 * int(np.ceil(np.log2(n))) + 2, (n, rounds)


def test_the_read_fold_on_worked_rows():
    comp = [0, 1, 1, 2, 7]  # (7: a component the caller says is not there)
    run_unitig = [2, 5, 4, 3, 12, 9, 0, 6, 6]
    run_len = [5, 1, 2, 3, 9, 4, 6, 7, 8]
    run_offsets = [0, 2, 2, 4, 7, 9]
    reads, hits = [10, 0, 0], [0, 0, 100]
    got = cr.read_components(run_unitig, run_len, run_offsets, comp, 3, reads, hits)
    # read 0: components 1 then 1; read 1: no run; read 2: 1 then 1; read 3: bad (unitig 6), bad (component 7), 0; read 4: 2, 2
    assert got["read_component"].tolist() == [1, cr.NO_COMPONENT, 1, 0, 2] and got["read_mixed"].tolist() == [0, 0, 0, 0, 0]
    assert got["tally"].tolist() == [4, 1, 0, 2] and reads == [11, 2, 1] and hits == [6, 11, 115]
    got = cr.read_components([2, 0, 2, 6], [1, 1, 1, 1], [0, 4], comp, 3)
    assert got["read_component"].tolist() == [1] and got["read_mixed"].tolist() == [1] and got["tally"].tolist() == [1, 0, 1, 0]


def test_the_file_formats():
    stats = np.array([[3, 13, 15, 4, 0], [1, 11, 11, 0, 3]], np.uint64)
    assert cr.want_components(stats, 5) == b"0\t3\t13\t25\t15\t1.2\t4\t0\n1\t1\t11\t15\t11\t1.0\t0\t3\n"
    assert cr.want_components_stats(stats, [2, 1, 3, 13, 0, 4]) == \
        b"components\t2\nsingletons\t1\nlargest_unitigs\t3\nlargest_nodes\t13\nlargest_share\t0.5417\n"
    assert cr.want_components_stats(stats[:0], [0] * 6).endswith(b"largest_share\t0.0000\n")
    assert cr.tagged_fa(b">0 LN:i:5 KC:i:1 km:f:1.0\nACGTA\n>1 LN:i:5 KC:i:1 km:f:1.0 CL:i:1 L:+:1:+\nCCCCC\n", [0, 1]) == \
        b">0 LN:i:5 KC:i:1 km:f:1.0 CC:i:0\nACGTA\n>1 LN:i:5 KC:i:1 km:f:1.0 CL:i:1 L:+:1:+ CC:i:1\nCCCCC\n"
    assert cr.tagged_gfa(b"H\tVN:Z:1.0\nS\t0\tACGTA\tLN:i:5\tKC:i:1\tkm:f:1.0\nL\t0\t+\t0\t-\t4M\n", [0]) == \
        b"H\tVN:Z:1.0\nS\t0\tACGTA\tLN:i:5\tKC:i:1\tkm:f:1.0\tCC:i:0\nL\t0\t+\t0\t-\t4M\n"
    assert cr.want_thread_reads(["a", "b"], [1, cr.NO_COMPONENT], [1, 0], [4, 5], [0, 2, 2]) == b"a\t1\t1\t9\nb\t*\t0\t0\n"
    assert cr.want_thread_components(stats, [7, 0], [90, 0]) == b"0\t3\t13\t7\t90\n1\t1\t11\t0\t0\n"
    assert cr.want_thread_stats_lines([5, 1, 2, 0], [90, 0]) == b"reads_with_component\t5\nreads_mixed\t2\ncomponents_hit\t1\n"
