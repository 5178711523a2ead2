"""`kmertools unitigs` on the CPU: listed in the main --help, its own --help lists every flag and both output files, every
usage error exits 2 with a clap-style message before any device is opened or the output directory is made, an input of an
unknown extension exits 101.  And the string-level reference the GPU tests compare against (tests/unitig_ref.py): it
reproduces the worked answers of tests/golden/unitig_known.json, and its own invariants - joins are mutual, the unitigs'
k-mers are the nodes each exactly once, every unitig starts with its start node - hold over a few hundred random small
tables (k = 3..7, reads and their reverse complements, circularised genomes, min_count 1 and 2)."""
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
import unitig_ref as ur  # noqa: E402


@pytest.fixture(scope="module")
def cli():
    if not CLI.exists():
        subprocess.check_call(["make", "-C", str(ROOT / "kmertools_amd" / "csrc"), "-j4"], stdout=subprocess.DEVNULL)
    return str(CLI)


def run(cli, *args):
    return subprocess.run([cli, *map(str, args)], capture_output=True, text=True, timeout=300)


def test_main_help_lists_unitigs(cli):
    r = run(cli, "--help")
    assert r.returncode == 0
    assert "  unitigs " in r.stdout
    for cmd in ("comp", "cov", "min", "ctr", "filter", "correct", "compare", "profile", "setop", "graph", "sketch", "help"):
        assert "  %s " % cmd in r.stdout, cmd


def test_unitigs_help_lists_every_flag(cli):
    for h in ("--help", "-h"):
        r = run(cli, "unitigs", h)
        assert r.returncode == 0
        for flag in ("-i, --input <INPUT>", "-o, --output <OUTPUT>", "-k, --k-size <K_SIZE>", "--min-count <N>", "--max-count <N>",
                     "--stats-only", "-m, --memory <MEMORY>", "-t, --threads <THREADS>", "--device <DEVICE>", "-h, --help",
                     "unitigs.fa", "unitigs.stats", "LN:i:", "KC:i:", "km:f:", "CL:i:1", "n50"):
            assert flag in r.stdout, flag
        assert "--devices" not in r.stdout and "--alt-input" not in r.stdout and "--acgt" not in r.stdout


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
    (("--acgt",), "--acgt"),
    (("--bogus",), "--bogus"),
    (("-z",), "-z"),
    (("--max-count",), "--max-count"),
    (("stray",), "stray"),
])
def test_unitigs_usage_errors(cli, inputs, extra, what):
    fa, out = inputs
    args = ["unitigs", "-i", fa, "-o", out]
    args += [] if "--k-size" in extra else ["-k", "15"]
    r = run(cli, *args, *extra)
    assert r.returncode == 2, r.stderr
    assert r.stderr.startswith("error: ") and what in r.stderr and "For more information, try '--help'." in r.stderr
    assert not out.exists()


@pytest.mark.parametrize("drop", ["-i", "-o", "-k"])
def test_unitigs_required_flags(cli, inputs, drop):
    fa, out = inputs
    flags = {"-i": fa, "-o": out, "-k": 15}
    args = ["unitigs"] + [x for f, v in flags.items() if f != drop for x in (f, v)]
    r = run(cli, *args)
    assert r.returncode == 2
    long_ = {"-i": "--input", "-o": "--output", "-k": "--k-size"}[drop]
    assert "required arguments were not provided" in r.stderr and long_ in r.stderr
    assert not out.exists()


def test_unitigs_bad_extension(cli, inputs, tmp_path):
    # (min == max, the largest count and every switch are allowed: the call gets past the argument checks)
    _, out = inputs
    bad = tmp_path / "reads.txt"
    bad.write_text(">x\nACGTACGTACGTACGTACGT\n")
    r = run(cli, "unitigs", "-i", bad, "-o", out, "-k", "31", "--min-count", "4294967295", "--max-count", "4294967295",
            "--stats-only")
    assert r.returncode == 101
    assert r.stderr.startswith("Error: unsupported input extension") and "reads.txt" in r.stderr
    assert not out.exists()


# ---- the reference ----------------------------------------------------------------------------------------------------------

KNOWN = json.loads((ROOT / "tests" / "golden" / "unitig_known.json").read_text())["cases"]


@pytest.mark.parametrize("case", KNOWN, ids=lambda c: "k%d_%s" % (c["k"], "+".join(c["reads"])[:24]))
def test_reference_reproduces_the_worked_answers(case):
    k = case["k"]
    got = ur.unitigs(gr.count_strings(case["reads"], k), k)
    assert [[s, c, f] for s, c, f, _ in got] == case["unitigs"]
    assert all(len(s) == n + k - 1 for s, _, _, n in got)


def test_the_worked_answers_cover_the_rule():
    flat = [u for c in KNOWN for u in c["unitigs"]]
    assert any(f & ur.CIRCULAR for _, _, f in flat) and any(not f for _, _, f in flat)
    assert any(len(c["unitigs"]) > 1 for c in KNOWN)
    assert any(len(s) == c["k"] for c in KNOWN for s, _, _ in c["unitigs"])      # a single node
    assert any(gr.rc_s(s) == s for c in KNOWN for s, _, _ in c["unitigs"])       # a palindromic node


def random_reads(rng, k):
    """reads of a small random genome with errors, their reverse complements, a circularised genome (once or several times
    around), and what breaks a naive rule: homopolymers, (AT)n, (ACGT)n, a hairpin"""
    g = "".join(rng.choice(list("ACGT"), size=int(rng.integers(k + 2, 60))))
    reads = []
    for _ in range(int(rng.integers(1, 10))):
        a = int(rng.integers(0, len(g) - k))
        s = list(g[a:a + int(rng.integers(k, 3 * k + 4))])
        if rng.random() < 0.4:
            s[int(rng.integers(0, len(s)))] = "ACGT"[int(rng.integers(0, 4))]
        reads.append("".join(s))
        if rng.random() < 0.5:
            reads.append(gr.rc_s(reads[-1]))
    c = "".join(rng.choice(list("ACGT"), size=int(rng.integers(2, 24))))
    reads.append(c * int(rng.integers(1, 4)) + c[:k - 1])
    if rng.random() < 0.5:
        n = k + int(rng.integers(0, 4))
        reads += ["ACGT"[int(rng.integers(0, 4))] * n, ("AT" * n)[:n + 1], ("ACGT" * n)[:n + 2]]
        half = reads[0][:k]
        reads.append(half + gr.rc_s(half))
    return reads


@pytest.mark.parametrize("k", [3, 4, 5, 6, 7])
def test_the_reference_keeps_its_invariants(k):
    rng = np.random.default_rng(2000 + k)
    seen = dict(circular=0, paths=0, singletons=0, long=0)
    for trial in range(60):
        table = gr.count_strings(random_reads(rng, k), k)
        for lo in (1, 2):
            us = ur.unitigs(table, k, lo)  # (asserts mutual joins, the k-mer cover and the start rule)
            nodes = gr.brute(table, k, lo)
            assert sum(n for _, _, _, n in us) == len(nodes)
            assert sum(c for _, c, _, _ in us) == sum(c for _, c, _ in nodes)
            starts = [gr.canon_s(s[:k]) for s, _, _, _ in us]
            assert starts == sorted(starts) and len(set(starts)) == len(starts)
            for s, _, f, n in us:
                if f & ur.CIRCULAR:
                    # linearised at its smallest node, spelled as that node's own string
                    assert n >= 2 and s[:k] == min(gr.canon_s(s[j:j + k]) for j in range(n))
                elif n > 1:
                    assert gr.canon_s(s[:k]) < gr.canon_s(s[-k:])
                else:
                    assert s == gr.canon_s(s)
                seen["circular"] += bool(f & ur.CIRCULAR)
                seen["paths"] += not f
                seen["singletons"] += n == 1
                seen["long"] += n > 3
    assert seen["paths"] and seen["singletons"]
    if k >= 5:  # (at k = 3 and 4 the 32 and 136 possible nodes of these inputs leave next to nothing unbranched)
        assert all(seen.values()), seen


def test_n50_and_the_rendered_files():
    assert ur.n50([]) == 0 and ur.n50([5]) == 5 and ur.n50([2, 2, 2, 10]) == 10 and ur.n50([4, 3, 3]) == 3 and ur.n50([5, 5]) == 5
    fa, stats = ur.want_files(gr.count_strings(["CGTAAAAAAAGTC", "CTCTCTCTCTCTCTCTCT"], 5), 5)
    assert fa.startswith(b">0 LN:i:5 KC:i:3 km:f:3.0\nAAAAA\n") and b" CL:i:1\n" in fa
    assert [ln.split(b"\t")[0] for ln in stats.splitlines()] == [b"unitigs", b"bases", b"nodes", b"occurrences", b"circular",
                                                                 b"singletons", b"longest", b"n50"]


def test_the_binding_s_flag_is_the_reference_s():
    from kmertools_amd import device
    assert device.UNITIG_CIRCULAR == ur.CIRCULAR == 1
