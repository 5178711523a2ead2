"""`kmertools unitigs --gfa / --links` on the CPU: the help text names both flags, the three files and the L line; the
refused combinations with --stats-only exit 2 with a clap-style message before any device is opened or the directory is
made.  And the reference the GPU tests compare against (tests/unitig_link_ref.py): it reproduces the worked answers of
tests/golden/unitig_links_known.json, and its own invariants - the string rule and the node rule give the same links, every
neighbour stands at an end of its unitig, no link leads into a cycle, every link has its mirror - hold over a few hundred
random small tables (k = 1..7 and 9, alphabets of two letters, circularised genomes, hairpins, min_count 1 and 2); its
array form agrees with it; the files it renders are what the formats say."""
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
import unitig_link_ref as lr  # noqa: E402
import unitig_ref as ur  # noqa: E402


@pytest.fixture(scope="module")
def cli():
    if not CLI.exists():
        subprocess.check_call(["make", "-C", str(ROOT / "kmertools_amd" / "csrc"), "-j4"], stdout=subprocess.DEVNULL)
    return str(CLI)


def run(cli, *args):
    return subprocess.run([cli, *map(str, args)], capture_output=True, text=True, timeout=300)


def test_unitigs_help_names_the_link_outputs(cli):
    for h in ("--help", "-h"):
        r = run(cli, "unitigs", h)
        assert r.returncode == 0
        for text in ("--gfa", "--links", "unitigs.gfa", "unitigs.links.stats", "unitigs.fa", "L<TAB>{u}<TAB>{su}<TAB>{v}<TAB>{sv}<TAB>{k-1}M",
                     "L:{su}:{v}:{sv}", "H<TAB>VN:Z:1.0", "links, edges", "dead_ends", "isolated", "self_links", "max_end_degree"):
            assert text in r.stdout, text


@pytest.mark.parametrize("extra, what", [
    (("--stats-only", "--gfa"), "--gfa"),
    (("--stats-only", "--links"), "--links"),
    (("--gfa", "--links", "--stats-only"), "--stats-only"),
    (("--gfa", "yes"), "yes"),
])
def test_unitigs_link_flag_usage_errors(cli, tmp_path, extra, what):
    fa, out = tmp_path / "a.fa", tmp_path / "out"
    fa.write_text(">a\nACGTACGTACGTACGTACGTACGTACGTAAACCCGGGTTT\n")
    r = run(cli, "unitigs", "-i", fa, "-o", out, "-k", "15", *extra)
    assert r.returncode == 2, r.stderr
    assert r.stderr.startswith("error: ") and what in r.stderr and "For more information, try '--help'." in r.stderr
    assert not out.exists()


# ---- the reference ----------------------------------------------------------------------------------------------------------

KNOWN = json.loads((ROOT / "tests" / "golden" / "unitig_links_known.json").read_text())["cases"]


@pytest.mark.parametrize("case", KNOWN, ids=lambda c: c["name"])
def test_reference_reproduces_the_worked_answers(case):
    k = case["k"]
    us, ls = lr.links(gr.count_strings(case["reads"], k), k)
    assert [s for s, _, _, _ in us] == case["unitigs"]
    assert ls == case["links"]
    # the worked answers are written down from the sentence of the rule: check them against it once more, pair by pair
    o = lr.oriented(us)
    for e in range(len(o)):
        for f in range(len(o)):
            assert (o[e][len(o[e]) - (k - 1):] == o[f][:k - 1]) == (f in case["links"][e]), (e, f)


def test_the_worked_answers_cover_the_rule():
    names = {c["name"] for c in KNOWN}
    assert names >= {"Y branch", "bubble", "homopolymer", "hairpin", "cycle", "palindromic node", "ends linked to each other"}
    by = {c["name"]: c for c in KNOWN}
    assert by["hairpin"]["links"][1] == [0]                                       # (u, -) -> (u, +): its own mirror
    assert by["cycle"]["links"] == by["homopolymer"]["links"] == [[0], [1]]      # (u, +) -> (u, +) and the mirror
    pal = by["palindromic node"]
    assert gr.rc_s(pal["unitigs"][0]) == pal["unitigs"][0] and pal["links"][3] == [0, 1]  # linked under both signs
    assert 0 in by["ends linked to each other"]["links"][0] and len(by["ends linked to each other"]["unitigs"][0]) > 5
    assert any(len(fs) == 2 for fs in by["Y branch"]["links"]) and any(not fs for fs in by["Y branch"]["links"])


def random_reads(rng, k, letters):
    """reads of a small random genome with errors, their reverse complements, a circularised genome (once or several times
    around), homopolymers, repeats of two and four letters and a hairpin appended to a read"""
    L = list(letters)
    g = "".join(rng.choice(L, size=int(rng.integers(k + 2, 50))))
    reads = []
    for _ in range(int(rng.integers(1, 8))):
        a = int(rng.integers(0, len(g) - k))
        s = list(g[a:a + int(rng.integers(k, 3 * k + 4))])
        if rng.random() < 0.4:
            s[int(rng.integers(0, len(s)))] = L[int(rng.integers(0, len(L)))]
        reads.append("".join(s))
        if rng.random() < 0.5:
            reads.append(gr.rc_s(reads[-1]))
    c = "".join(rng.choice(L, size=int(rng.integers(2, 20))))
    reads.append(c * int(rng.integers(1, 4)) + c[:k - 1])
    if rng.random() < 0.5:
        n = k + int(rng.integers(0, 4))
        reads += [L[int(rng.integers(0, len(L)))] * n, ("AT" * n)[:n + 1], ("ACGT" * n)[:n + 2]]
        half = reads[0][:k]
        reads.append(half + gr.rc_s(half))
    return reads


@pytest.mark.parametrize("k", [1, 2, 3, 4, 5, 6, 7, 9])
def test_the_reference_keeps_its_invariants(k):
    rng = np.random.default_rng(4100 + k)
    seen = dict(links=0, self_mirror=0, five=0, circular=0, dead=0, tables=0)
    for trial in range(24):
        table = gr.count_strings(random_reads(rng, k, "ACGT" if trial % 3 else "AC"), k)
        for lo in (1, 2):
            us, ls = lr.links(table, k, lo)  # (asserts the two rules' agreement, ends, cycles, mirrors, the degree bound)
            assert len(ls) == 2 * len(us) and all(fs == sorted(set(fs)) and all(f < len(ls) for f in fs) for fs in ls)
            if k >= 2 and us:
                off, to = lr.as_arrays(ls)
                text = "".join(u[0] for u in us).encode()
                o2, t2 = lr.links_of_arrays(np.frombuffer(text, np.uint8), np.cumsum([0] + [len(u[0]) for u in us]), k)
                assert np.array_equal(off, o2) and np.array_equal(to, t2) and t2.dtype == np.uint32 and o2.dtype == np.uint64
            seen["links"] += sum(map(len, ls))
            seen["self_mirror"] += sum(1 for e, fs in enumerate(ls) for f in fs if f == e ^ 1)
            seen["five"] += sum(1 for fs in ls if len(fs) == 5)
            seen["circular"] += sum(1 for u in us if u[2] & ur.CIRCULAR)
            seen["dead"] += sum(1 for fs in ls if not fs)
            seen["tables"] += 1
    assert seen["links"] and seen["tables"] == 48, seen
    if k >= 5:
        assert seen["circular"] and seen["dead"], seen
    # (u, +) -> (u, -) needs k - 1 bases that are their own reverse complement: odd k only (k = 1: no bases, every pair)
    assert (seen["self_mirror"] > 0) == (k % 2 == 1), seen
    if k in (2, 4):
        assert seen["five"], seen


def test_k_1_links_every_pair():
    for reads in (["A"], ["AC"], ["ACGT"]):
        us, ls = lr.links(gr.count_strings(reads, 1), 1)
        assert len(us) in (1, 2) and all(fs == list(range(2 * len(us))) for fs in ls)


def test_the_rendered_files():
    case = next(c for c in KNOWN if c["name"] == "palindromic node")
    table, k = gr.count_strings(case["reads"], case["k"]), case["k"]
    assert lr.want_gfa(table, k) == (b"H\tVN:Z:1.0\n"
                                     b"S\t0\tACGT\tLN:i:4\tKC:i:1\tkm:f:1.0\n"
                                     b"S\t1\tCGTAA\tLN:i:5\tKC:i:2\tkm:f:1.0\n"
                                     b"S\t2\tCGTCC\tLN:i:5\tKC:i:2\tkm:f:1.0\n"
                                     b"L\t0\t+\t1\t+\t3M\nL\t0\t+\t2\t+\t3M\nL\t0\t-\t1\t+\t3M\nL\t0\t-\t2\t+\t3M\n")
    assert lr.want_fa_links(table, k) == (b">0 LN:i:4 KC:i:1 km:f:1.0 L:+:1:+ L:+:2:+ L:-:1:+ L:-:2:+\nACGT\n"
                                          b">1 LN:i:5 KC:i:2 km:f:1.0 L:-:0:+ L:-:0:-\nCGTAA\n"
                                          b">2 LN:i:5 KC:i:2 km:f:1.0 L:-:0:+ L:-:0:-\nCGTCC\n")
    assert lr.want_link_stats(table, k) == b"links\t8\nedges\t4\ndead_ends\t2\nisolated\t0\nself_links\t0\nmax_end_degree\t2\n"
    # a cycle's S line carries CL:i:1 last, its closing link is written once; a hairpin's link is its own mirror
    cyc = gr.count_strings(["TCATCATCATCATCATCATCA"], 7)
    assert lr.want_gfa(cyc, 7) == b"H\tVN:Z:1.0\nS\t0\tATCATCATC\tLN:i:9\tKC:i:15\tkm:f:5.0\tCL:i:1\nL\t0\t+\t0\t+\t6M\n"
    assert lr.want_fa_links(cyc, 7) == b">0 LN:i:9 KC:i:15 km:f:5.0 CL:i:1 L:+:0:+ L:-:0:-\nATCATCATC\n"
    assert lr.want_link_stats(cyc, 7) == b"links\t2\nedges\t1\ndead_ends\t0\nisolated\t0\nself_links\t2\nmax_end_degree\t1\n"
    hp = gr.count_strings(["GACGTCA"], 5)
    assert lr.want_gfa(hp, 5).endswith(b"L\t0\t-\t0\t+\t4M\n") and lr.want_gfa(hp, 5).count(b"\nL\t") == 1
    # without the fields the record lines are unitig_ref's
    assert lr.want_fa_links(gr.count_strings(["ACGGTCAATGC"], 5), 5) == ur.want_files(gr.count_strings(["ACGGTCAATGC"], 5), 5)[0]


def test_the_binding_declares_the_call():
    from kmertools_amd import device
    assert callable(device.Counter.unitig_links) and callable(device.Counter.unitigs_linked_device)
