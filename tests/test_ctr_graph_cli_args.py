"""`kmertools graph` on the CPU: listed in the main --help, its own --help lists every flag and both output files, every
usage error exits 2 with a clap-style message before any device is opened or the output directory is made, an input of an
unknown extension exits 101.  And the restatement the GPU tests compare against (tests/graph_ref.py): its numpy form and
its string-level brute force agree with the worked answers of tests/golden/graph_known.json and with each other, and the
rule they state is mutual - a side that is not an end has exactly one neighbour, whose facing side is not an end either."""
import json
import pathlib
import subprocess
import sys

import numpy as np
import pytest

ROOT = pathlib.Path(__file__).resolve().parent.parent
CLI = ROOT / "kmertools_amd" / "bin" / "kmertools"
sys.path.insert(0, str(ROOT / "tests"))
import graph_ref as gr  # noqa: E402


@pytest.fixture(scope="module")
def cli():
    if not CLI.exists():
        subprocess.check_call(["make", "-C", str(ROOT / "kmertools_amd" / "csrc"), "-j4"], stdout=subprocess.DEVNULL)
    return str(CLI)


def run(cli, *args):
    return subprocess.run([cli, *map(str, args)], capture_output=True, text=True, timeout=300)


def test_main_help_lists_graph(cli):
    r = run(cli, "--help")
    assert r.returncode == 0
    assert "  graph " in r.stdout
    for cmd in ("comp", "cov", "min", "ctr", "filter", "correct", "compare", "profile", "setop", "sketch", "help"):
        assert "  %s " % cmd in r.stdout, cmd


def test_graph_help_lists_every_flag(cli):
    for h in ("--help", "-h"):
        r = run(cli, "graph", h)
        assert r.returncode == 0
        for flag in ("-i, --input <INPUT>", "-o, --output <OUTPUT>", "-k, --k-size <K_SIZE>", "--min-count <N>", "--max-count <N>",
                     "--acgt", "--stats-only", "-m, --memory <MEMORY>", "-t, --threads <THREADS>", "--device <DEVICE>",
                     "-h, --help", "graph.nodes", "graph.stats"):
            assert flag in r.stdout, flag
        assert "--devices" not in r.stdout and "--alt-input" not in r.stdout


@pytest.fixture
def inputs(tmp_path):
    fa = tmp_path / "a.fa"
    fa.write_text(">a\nACGTACGTACGTACGTACGTACGTACGTAAACCCGGGTTT\n")
    return fa, tmp_path / "out"


@pytest.mark.parametrize("extra, what", [
    (("--k-size", "9"), "--k-size"),
    (("--k-size", "32"), "--k-size"),
    (("--k-size", "x"), "--k-size"),
    (("--min-count", "0"), "--min-count"),
    (("--max-count", "0"), "--max-count"),
    (("--min-count", "5", "--max-count", "4"), "--min-count"),
    (("--min-count", "-3"), "--min-count"),
    (("--max-count", "ten"), "--max-count"),
    (("--max-count", "4294967296"), "--max-count"),
    (("--memory", "5"), "--memory"),
    (("--threads", "x"), "--threads"),
    (("--device", "64"), "--device"),
    (("--devices", "2"), "--devices"),
    (("--alt-input", "b.fa"), "--alt-input"),
    (("--bogus",), "--bogus"),
    (("-z",), "-z"),
    (("--max-count",), "--max-count"),
    (("stray",), "stray"),
])
def test_graph_usage_errors(cli, inputs, extra, what):
    fa, out = inputs
    args = ["graph", "-i", fa, "-o", out]
    args += [] if "--k-size" in extra else ["-k", "15"]
    r = run(cli, *args, *extra)
    assert r.returncode == 2, r.stderr
    assert r.stderr.startswith("error: ") and what in r.stderr and "For more information, try '--help'." in r.stderr
    assert not out.exists()


@pytest.mark.parametrize("drop", ["-i", "-o", "-k"])
def test_graph_required_flags(cli, inputs, drop):
    fa, out = inputs
    flags = {"-i": fa, "-o": out, "-k": 15}
    args = ["graph"] + [x for f, v in flags.items() if f != drop for x in (f, v)]
    r = run(cli, *args)
    assert r.returncode == 2
    long_ = {"-i": "--input", "-o": "--output", "-k": "--k-size"}[drop]
    assert "required arguments were not provided" in r.stderr and long_ in r.stderr
    assert not out.exists()


def test_graph_bad_extension(cli, inputs, tmp_path):
    # (min == max, the largest count and every switch are allowed: the call gets past the argument checks)
    _, out = inputs
    bad = tmp_path / "reads.txt"
    bad.write_text(">x\nACGTACGTACGTACGTACGT\n")
    r = run(cli, "graph", "-i", bad, "-o", out, "-k", "31", "--min-count", "4294967295", "--max-count", "4294967295", "--acgt",
            "--stats-only")
    assert r.returncode == 101
    assert r.stderr.startswith("Error: unsupported input extension") and "reads.txt" in r.stderr
    assert not out.exists()


# ---- the restatement ------------------------------------------------------------------------------------------------------

KNOWN = json.loads((ROOT / "tests" / "golden" / "graph_known.json").read_text())["cases"]


def table_arrays(table):
    keys = np.array([gr.key_of(s) for s in table], np.uint64)
    counts = np.array([table[s] for s in table], np.uint32)
    return keys, counts


@pytest.mark.parametrize("case", KNOWN, ids=lambda c: "k%d_%s_min%d" % (c["k"], "+".join(c["reads"])[:24], c["min_count"]))
def test_restatements_reproduce_the_worked_answers(case):
    k, lo = case["k"], case["min_count"]
    table = gr.count_strings(case["reads"], k)
    want = [tuple(n) for n in case["nodes"]]
    cen = list(case["census"]) + [0] * 25
    for cell, v in case["cells"].items():
        dl, dr = map(int, cell.split(","))
        cen[7 + 5 * dl + dr] = v
    nodes = gr.brute(table, k, lo)
    assert nodes == want
    assert gr.census_of(nodes) == cen
    F, info, c, census = gr.restate(*table_arrays(table), k, lo)
    assert list(zip(F.tolist(), c.tolist(), info.tolist())) == want
    assert census.tolist() == cen
    assert all(i != 0 and i < 1 << 10 for _, _, i in nodes)


def test_the_fast_reverse_complement_is_the_plain_one():
    rng = np.random.default_rng(7)
    for k in (1, 2, 3, 4, 5, 15, 16, 17, 30, 31):
        x = rng.integers(0, 1 << 62, size=500, dtype=np.uint64) & np.uint64((1 << (2 * k)) - 1)
        x[:3] = (0, (1 << (2 * k)) - 1, 1)
        assert np.array_equal(gr.rc_np(x, k), gr.rc_np_loop(x, k)), k
        assert all(gr.str_of(r, k) == gr.rc_s(gr.str_of(v, k)) for v, r in zip(x[:40], gr.rc_np(x[:40], k))), k


def random_reads(rng, k):
    """short reads of a small random genome with errors, plus what breaks a naive rule: homopolymers, (AT)n, (ACGT)n, a
    read and its reverse complement, a hairpin"""
    g = "".join(rng.choice(list("ACGT"), size=int(rng.integers(k + 2, 60))))
    reads = []
    for _ in range(int(rng.integers(1, 12))):
        a = int(rng.integers(0, len(g) - k))
        s = list(g[a:a + int(rng.integers(k, 3 * k + 4))])
        if rng.random() < 0.4:
            s[int(rng.integers(0, len(s)))] = "ACGT"[int(rng.integers(0, 4))]
        reads.append("".join(s))
    n = k + int(rng.integers(0, 4))
    reads += ["ACGT"[int(rng.integers(0, 4))] * n, ("AT" * n)[:n + 1], ("ACGT" * n)[:n + 2], gr.rc_s(reads[0])]
    half = reads[0][:k]
    reads.append(half + gr.rc_s(half))
    return reads


@pytest.mark.parametrize("k", [3, 4, 5, 6, 11])
def test_the_rule_is_mutual_and_the_restatements_agree(k):
    rng = np.random.default_rng(1000 + k)
    odd = 0
    for trial in range(60 if k < 11 else 25):
        table = gr.count_strings(random_reads(rng, k), k)
        for lo, hi in ((1, gr.U32), (2, gr.U32), (1, 1), (2, 3)):
            nodes = gr.brute(table, k, lo, hi)
            assert gr.mutual_failures(nodes, k) == [], (k, trial, lo, hi)
            F, info, c, census = gr.restate(*table_arrays(table), k, lo, hi)
            assert list(zip(F.tolist(), c.tolist(), info.tolist())) == nodes, (k, trial, lo, hi)
            cen = gr.census_of(nodes)
            assert census.tolist() == cen
            assert cen[0] == sum(cen[7:]) and cen[4] == cen[7] and all(i for _, _, i in nodes)
            odd += cen[3] & 1
    if k in (3, 5, 11):
        assert odd  # (odd k: a hairpin joins a side to itself, so the end sides need not pair up)


def test_info_text_is_the_library_binding_s():
    from kmertools_amd import device
    assert list(device.GRAPH_CENSUS_NAMES) == gr.CENSUS_NAMES and len(gr.CENSUS_NAMES) == 32
    for info in (0x11, 0x208, 0x300, 0x238, 0xFF | 0x300, 0x1A5):
        assert device.graph_info_text(info) == gr.info_text(info)
    assert device.graph_info_text(0x238) == ("AC..", "...T", "L.")
