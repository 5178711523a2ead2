"""`kmertools thread` on the CPU: the help text names the files and the GAF columns; usage errors exit 2 with a clap-style
message before any device is opened or the directory is made.  And the reference the GPU tests compare against
(tests/thread_ref.py): it reproduces the worked answers of tests/golden/thread_known.json; over a few hundred random small
tables (k = 1..7 and 9, as the link tests use) its position-by-position runs agree with a string-level brute force (str.find
of each read k-mer and its reverse complement in the unitig strings); threading the unitigs themselves gives exactly one run
>u per unitig, covering it; threading the counted reads at min_count 1 gives no miss; every chain's GAF coordinates spell the
read's substring when the path's unitigs are concatenated with k - 1 overlap."""
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
import thread_ref as tr  # noqa: E402
import unitig_ref as ur  # noqa: E402
from test_ctr_unitig_links_cli_args import random_reads  # noqa: E402


@pytest.fixture(scope="module")
def cli():
    if not CLI.exists():
        subprocess.check_call(["make", "-C", str(ROOT / "kmertools_amd" / "csrc"), "-j4"], stdout=subprocess.DEVNULL)
    return str(CLI)


def run(cli, *args):
    return subprocess.run([cli, *map(str, args)], capture_output=True, text=True, timeout=300)


def test_thread_help_names_the_files_and_the_columns(cli):
    for h in ("--help", "-h"):
        r = run(cli, "thread", h)
        assert r.returncode == 0
        for text in ("--alt-input", "--table", "--min-count", "--max-count", "--stats-only", "--estimate-size", "unitigs.fa",
                     "unitigs.gfa", "thread.gaf", "thread.unitigs", "thread.stats", "unitigs --gfa", "qstart", "qend", "'>u'", "'<u'",
                     "path length", "start on the path", "end on the path", "255", "reads_one_chain_end_to_end", "unitigs_hit",
                     "hits / nodes", "count sum"):
            assert text in r.stdout, text
    assert "thread" in run(cli, "--help").stdout


@pytest.mark.parametrize("args, what", [
    (("-o", "OUT", "-k", "15"), "--input"),
    (("-i", "IN", "-k", "15"), "--output"),
    (("-i", "IN", "-o", "OUT"), "--k-size"),
    (("-i", "IN", "-o", "OUT", "-k", "9"), "9"),
    (("-i", "IN", "-o", "OUT", "-k", "32"), "32"),
    (("-i", "IN", "-o", "OUT", "-k", "15", "--min-count", "0"), "--min-count"),
    (("-i", "IN", "-o", "OUT", "-k", "15", "--min-count", "3", "--max-count", "2"), "3 is greater than 2"),
    (("-i", "IN", "-o", "OUT", "-k", "15", "--gfa"), "--gfa"),
    (("-i", "IN", "-o", "OUT", "-k", "15", "--stats-only", "yes"), "yes"),
    (("-i", "IN", "-o", "OUT", "-k", "15", "--estimate-precision", "12"), "--estimate-size"),
    (("-i", "IN", "-a", "IN", "-o", "OUT", "-k", "15", "--table", "TABLE"), "--alt-input"),
    (("-i", "IN", "-o", "OUT", "-k", "15", "--table", "TABLE", "--estimate-size"), "--estimate-size"),
    (("-i", "IN", "-o", "OUT", "-k", "15", "--table", "MISSING"), "none.ktab"),
    (("-i", "IN", "-o", "OUT", "-k", "15", "--device", "64"), "64"),
])
def test_thread_usage_errors(cli, tmp_path, args, what):
    fa, out, table = tmp_path / "a.fa", tmp_path / "out", tmp_path / "t.ktab"
    fa.write_text(">a\nACGTACGTACGTACGTACGTACGTACGTAAACCCGGGTTT\n")
    table.write_bytes(b"not a table file")
    subst = {"IN": fa, "OUT": out, "TABLE": table, "MISSING": tmp_path / "none.ktab"}
    r = run(cli, "thread", *[subst.get(a, a) for a in args])
    assert r.returncode == 2, r.stderr
    assert r.stderr.startswith("error: ") and what in r.stderr and "For more information, try '--help'." in r.stderr
    assert not out.exists()


# ---- the reference ----------------------------------------------------------------------------------------------------------

KNOWN = json.loads((ROOT / "tests" / "golden" / "thread_known.json").read_text())["cases"]


@pytest.mark.parametrize("case", KNOWN, ids=lambda c: c["name"])
def test_reference_reproduces_the_worked_answers(case):
    k = case["k"]
    table = gr.count_strings(case["graph_reads"], k)
    unitigs = [u[0] for u in ur.unitigs(table, k)]
    assert unitigs == case["unitigs"]
    res, _ = tr.thread(unitigs, case["reads"], k)
    ro = res["run_offsets"]
    assert [[list(r) for r in res["runs"][ro[i]:ro[i + 1]]] for i in range(len(case["reads"]))] == case["runs"]
    ids = ["r%d" % i for i in range(len(case["reads"]))]
    assert tr.want_files(table, k, ids, case["reads"])["thread.gaf"].decode().splitlines() == case["gaf"]


def test_the_worked_answers_cover_the_rule():
    by = {c["name"]: c for c in KNOWN}
    assert set(by) >= {"reverse complement of a unitig", "a read crossing a fork", "twice round a cycle", "an even-k palindromic node",
                       "a read with an N", "a read with one substitution"}
    assert all(3 <= c["k"] <= 5 for c in KNOWN)
    rc = by["reverse complement of a unitig"]
    assert rc["reads"][1] == gr.rc_s(rc["unitigs"][0]) and rc["runs"][1] == [[11, 7, 1, 6]] and "<0" in rc["gaf"][1]
    assert ">2>0" in by["a read crossing a fork"]["gaf"][0] and "<1<2" in by["a read crossing a fork"]["gaf"][1]
    cyc = by["twice round a cycle"]
    assert len(cyc["runs"][0]) == 3 and ">0>0>0" in cyc["gaf"][0] and "<0<0<0" in cyc["gaf"][1]  # a new run where it wraps
    pal = by["an even-k palindromic node"]
    assert pal["k"] % 2 == 0 and gr.rc_s(pal["unitigs"][0]) == pal["unitigs"][0]
    assert [r[2] for r in pal["runs"][0]] == [3, 0, 4] and [r[2] for r in pal["runs"][1]] == [5, 0, 2]  # the palindrome: never '<'
    assert "N" in by["a read with an N"]["reads"][0] and len(by["a read with an N"]["gaf"]) == 2
    sub = by["a read with one substitution"]
    assert sub["runs"][0] == [[0, 5, 0, 0], [10, 2, 0, 10]] and len(sub["gaf"]) == 2  # k misses between the two runs


def threaded_reads(rng, reads, k):
    """what is threaded onto the graph of `reads`: the reads, reverse complements, reads with an N or a substitution, a short
    one, an empty one and a foreign one"""
    out = list(reads)
    out += [gr.rc_s(r) for r in reads[:3]]
    for r in reads[:2]:
        s = list(r)
        s[int(rng.integers(0, len(s)))] = "N" if rng.random() < 0.5 else "ACGT"[int(rng.integers(0, 4))]
        out.append("".join(s))
    out += ["", reads[0][:max(0, k - 1)], "".join(rng.choice(list("ACGT"), size=3 * k + 2))]
    return out


@pytest.mark.parametrize("k", [1, 2, 3, 4, 5, 6, 7, 9])
def test_the_reference_agrees_with_the_string_brute_force(k):
    rng = np.random.default_rng(5200 + k)
    seen = dict(tables=0, runs=0, anti=0, chains_multi=0, misses=0, circular=0)
    for trial in range(24):
        reads = random_reads(rng, k, "ACGT" if trial % 3 else "AC")
        table = gr.count_strings(reads, k)
        for lo in (1, 2):
            us = ur.unitigs(table, k, lo)
            unitigs = [u[0] for u in us]
            ulen = [len(s) for s in unitigs]
            q = threaded_reads(rng, reads, k)
            res, hits = tr.thread(unitigs, q, k)
            b_runs, b_off, _ = tr.brute_runs(unitigs, q, k)
            assert b_runs == res["runs"] and b_off == res["run_offsets"]
            # ... and the array form the GPU tests use
            (ub, uo), (qb, qo) = tr.csr(unitigs), tr.csr(q)
            assert np.array_equal(tr.hits_np(tr.index_np(ub, uo, k), qb, qo, k), hits)
            r2 = tr.runs_np(hits, qo, uo, k)
            assert list(zip(r2["run_start"].tolist(), r2["run_len"].tolist(), r2["run_unitig"].tolist(), r2["run_upos"].tolist())) == res["runs"]
            assert r2["run_offsets"].tolist() == res["run_offsets"] and r2["tally"].tolist() == res["tally"]
            assert r2["unitig_hits"].tolist() == res["unitig_hits"] and r2["unitig_runs"].tolist() == res["unitig_runs"]
            t = res["tally"]
            assert t[0] == t[1] + t[2] and t[3] == 0 and t[1] == sum(r[1] for r in res["runs"]) == sum(res["unitig_hits"])
            assert t[4] == len(res["runs"]) == sum(res["unitig_runs"])
            # every chain's GAF coordinates spell the read's substring on the path
            base = 0
            for i, (r, cs) in enumerate(zip(q, res["chains"])):
                for c in cs:
                    f = tr.gaf_line("r", len(r), base, c, ulen, k).rstrip("\n").split("\t")
                    path = tr.path_string(unitigs, c, k)
                    assert len(path) == int(f[6]) and path[int(f[7]):int(f[8])] == r[int(f[2]):int(f[3])], (unitigs, r, f)
                    seen["chains_multi"] += len(c) > 1
                base += len(r)
            # the unitigs themselves: exactly one run >u per unitig, covering it
            own, _ = tr.thread(unitigs, unitigs, k)
            pos = np.cumsum([0] + ulen)
            assert own["runs"] == [(int(pos[u]), ulen[u] - k + 1, 2 * u, 0) for u in range(len(unitigs))]
            assert all(len(cs) == 1 for cs in own["chains"])
            # the counted reads at min_count 1: no miss
            if lo == 1:
                mine, _ = tr.thread(unitigs, reads, k)
                assert mine["tally"][2] == 0 and mine["tally"][0] == mine["tally"][1] == sum(table.values())
            seen["tables"] += 1
            seen["runs"] += len(res["runs"])
            seen["anti"] += sum(r[2] & 1 for r in res["runs"])
            seen["misses"] += t[2]
            seen["circular"] += sum(1 for u in us if u[2] & ur.CIRCULAR)
    assert seen["tables"] == 48 and seen["runs"] and seen["anti"], seen
    if k >= 3:  # (at k = 1 every letter is in the graph)
        assert seen["chains_multi"] and seen["misses"], seen
    if k >= 5:
        assert seen["circular"], seen


def test_the_rendered_files():
    case = next(c for c in KNOWN if c["name"] == "a read crossing a fork")
    k, table = case["k"], gr.count_strings(case["graph_reads"], case["k"])
    files = tr.want_files(table, k, ["first", "second"], case["reads"])
    assert files["thread.gaf"] == (b"first\t16\t0\t16\t+\t>2>0\t16\t0\t16\t16\t16\t255\n"
                                   b"second\t9\t0\t9\t+\t<1<2\t11\t0\t9\t9\t9\t255\n")
    assert files["thread.unitigs"] == (b"0\t10\t6\t6\t6\t1\t1.000000\n1\t5\t1\t1\t1\t1\t1.000000\n2\t10\t6\t8\t10\t2\t1.666667\n")
    assert files["thread.stats"] == (b"reads\t2\nbases\t25\nwindows\t17\nhits\t17\nmisses\t0\nruns\t4\nchains\t2\nreads_with_hit\t2\n"
                                     b"reads_one_chain_end_to_end\t2\nunitigs_hit\t3\n")
    assert files["unitigs.fa"] == ur.want_files(table, k)[0] and files["unitigs.gfa"].startswith(b"H\tVN:Z:1.0\nS\t0\tAATGCTTAGC\t")


def test_the_binding_declares_the_calls():
    from kmertools_amd import _lib, device
    assert callable(device.Counter.index_sequences) and callable(device.Counter.thread_hits) and callable(device.Context.thread_runs)
    assert callable(device.UnitigIndex.thread_host)
    assert {"kt_ctr_index_sequences", "kt_ctr_thread_hits", "kt_thread_runs"} <= set(_lib.SYMBOLS)
