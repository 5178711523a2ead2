"""`kmertools hetmers` on the CPU: listed in the main --help, its own --help lists every flag and the four output files,
every usage error exits 2 with a clap-style message before any device is opened or the output directory is made, an input
of an unknown extension exits 101; kt_ctr_hetmers is declared in the header, bound in _lib.SYMBOLS and documented in
INTEGRATION.md.  And the restatement the GPU tests compare against (tests/hetmer_ref.py): its numpy form and its
string-level brute force agree with the worked answers of tests/golden/hetmers_known.json and with each other on random
subsets of all canonical k-mers, and the rule they state is symmetric."""
import json
import pathlib
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = pathlib.Path(__file__).resolve().parent.parent
CLI = ROOT / "kmertools_amd" / "bin" / "kmertools"
sys.path.insert(0, str(ROOT / "tests"))
import hetmer_ref as hr  # noqa: E402

FILES = ("hetmers.pairs", "hetmers.cov", "hetmers.matrix", "hetmers.stats")


@pytest.fixture(scope="module")
def cli():
    if not CLI.exists():
        subprocess.check_call(["make", "-C", str(ROOT / "kmertools_amd" / "csrc"), "-j4"], stdout=subprocess.DEVNULL)
    return str(CLI)


def run(cli, *args):
    return subprocess.run([cli, *map(str, args)], capture_output=True, text=True, timeout=300)


def test_main_help_lists_hetmers(cli):
    r = run(cli, "--help")
    assert r.returncode == 0
    assert "  hetmers " in r.stdout
    for cmd in ("comp", "cov", "min", "ctr", "filter", "correct", "compare", "profile", "setop", "graph", "unitigs", "sketch",
                "card", "help"):
        assert "  %s " % cmd in r.stdout, cmd


def test_hetmers_help_lists_every_flag_and_file(cli):
    for h in ("--help", "-h"):
        r = run(cli, "hetmers", h)
        assert r.returncode == 0
        for flag in ("-i, --input <INPUT>", "-o, --output <OUTPUT>", "-k, --k-size <K_SIZE>", "--min-count <N>", "--max-count <N>",
                     "--middle", "--max-minor <N>", "--max-major <N>", "--stats-only", "-m, --memory <MEMORY>",
                     "-t, --threads <THREADS>", "--device <DEVICE>", "--estimate-size", "--estimate-precision", "-h, --help") + FILES:
            assert flag in r.stdout, flag
        # the flag value is the last row / column index, as compare's --max-a / --max-b
        assert "the last row counts N or more [default: 500]" in r.stdout
        assert "the last column counts N or more [default: 1000]" in r.stdout
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
    (("--k-size", "16", "--middle"), "--middle"),
    (("--k-size", "30", "--middle"), "--middle"),
    (("--min-count", "0"), "--min-count"),
    (("--max-count", "0"), "--max-count"),
    (("--min-count", "5", "--max-count", "4"), "--min-count"),
    (("--min-count", "-3"), "--min-count"),
    (("--max-count", "4294967296"), "--max-count"),
    (("--max-minor", "0"), "--max-minor"),
    (("--max-major", "0"), "--max-major"),
    (("--max-minor", "x"), "--max-minor"),
    (("--max-major", "16777216"), "--max-major"),
    (("--max-minor", "4095", "--max-major", "4096"), "--max-minor"),
    (("--max-minor", "16777215", "--max-major", "1"), "--max-major"),
    (("--middle", "yes"), "yes"),
    (("--estimate-precision", "12"), "--estimate-size"),
    (("--estimate-size", "--estimate-precision", "3"), "--estimate-precision"),
    (("--estimate-size", "--estimate-precision", "17"), "--estimate-precision"),
    (("--estimate-size", "--estimate-precision", "x"), "--estimate-precision"),
    (("--memory", "5"), "--memory"),
    (("--threads", "x"), "--threads"),
    (("--device", "64"), "--device"),
    (("--devices", "2"), "--devices"),
    (("--acgt",), "--acgt"),
    (("--bogus",), "--bogus"),
    (("--max-minor",), "--max-minor"),
    (("stray",), "stray"),
])
def test_hetmers_usage_errors(cli, inputs, extra, what):
    fa, out = inputs
    args = ["hetmers", "-i", fa, "-o", out]
    args += [] if "--k-size" in extra else ["-k", "15"]
    r = run(cli, *args, *extra)
    assert r.returncode == 2, r.stderr
    assert r.stderr.startswith("error: ") and what in r.stderr and "For more information, try '--help'." in r.stderr
    assert not out.exists()


@pytest.mark.parametrize("drop", ["-i", "-o", "-k"])
def test_hetmers_required_flags(cli, inputs, drop):
    fa, out = inputs
    flags = {"-i": fa, "-o": out, "-k": 15}
    args = ["hetmers"] + [x for f, v in flags.items() if f != drop for x in (f, v)]
    r = run(cli, *args)
    assert r.returncode == 2
    long_ = {"-i": "--input", "-o": "--output", "-k": "--k-size"}[drop]
    assert "required arguments were not provided" in r.stderr and long_ in r.stderr
    assert not out.exists()


def test_hetmers_bad_extension(cli, inputs, tmp_path):
    # (min == max, the widest matrix that fits and every switch are allowed: the call gets past the argument checks)
    _, out = inputs
    bad = tmp_path / "reads.txt"
    bad.write_text(">x\nACGTACGTACGTACGTACGT\n")
    r = run(cli, "hetmers", "-i", bad, "-o", out, "-k", "31", "--min-count", "4294967295", "--max-count", "4294967295", "--middle",
            "--max-minor", "4095", "--max-major", "4095", "--stats-only", "--estimate-size")
    assert r.returncode == 101
    assert r.stderr.startswith("Error: unsupported input extension") and "reads.txt" in r.stderr
    assert not out.exists()


def test_the_symbol_is_declared_bound_and_documented():
    from kmertools_amd import _lib, device
    header = (ROOT / "include" / "kmertools_hip.h").read_text()
    m = re.search(r"\nint kt_ctr_hetmers\(([^;]*)\);", header)
    assert m, "the header does not declare kt_ctr_hetmers"
    params = [p.strip() for p in m.group(1).replace("\n", " ").split(",")]
    assert [p.split()[-1].lstrip("*") for p in params] == [
        "table", "min_count", "max_count", "positions", "keys_a", "keys_b", "counts_a", "counts_b", "max_out", "n_out", "matrix",
        "n_rows", "n_cols", "census", "mem", "sorted"]
    for name, value in (("KT_HET_ALL", 0), ("KT_HET_MIDDLE", 1), ("KT_HET_CENSUS", 8)):
        assert re.search(r"#define %s %d\b" % (name, value), header), name
        assert getattr(_lib, name) == value
    assert "Device scratch:" in header[header.index("The heterozygous k-mer pairs"):m.start()]
    res, args = _lib.SYMBOLS["kt_ctr_hetmers"]
    assert res is _lib._i and len(args) == len(params) == 16
    integration = (ROOT / "INTEGRATION.md").read_text()
    assert "pub fn kt_ctr_hetmers(table: *mut KtCtr, min_count: u32, max_count: u32, positions: c_int," in integration
    assert list(device.HET_CENSUS_NAMES) == hr.CENSUS_NAMES and len(hr.CENSUS_NAMES) == _lib.KT_HET_CENSUS
    assert callable(device.Counter.hetmers) and callable(device.Counter.hetmers_device)


# ---- the restatement ------------------------------------------------------------------------------------------------------

KNOWN = json.loads((ROOT / "tests" / "golden" / "hetmers_known.json").read_text())["cases"]


def table_arrays(table):
    return np.array([hr.key_of(s) for s in table], np.uint64), np.array(list(table.values()), np.uint32)


def pairs_of(r):
    return list(zip(r.a.tolist(), r.b.tolist(), r.ca.tolist(), r.cb.tolist()))


def test_the_golden_file_holds_the_cases_it_must():
    names = " | ".join(c["name"] for c in KNOWN)
    for must in ("one pair", "alone", "chain", "broken by the count range"):
        assert must in names, must


@pytest.mark.parametrize("case", KNOWN, ids=lambda c: c["name"].replace(" ", "_"))
def test_restatements_reproduce_the_worked_answers(case):
    k, lo, hi, middle = case["k"], case["min_count"], case["max_count"], case["middle"]
    want = [(hr.key_of(a), hr.key_of(b), ca, cb) for a, b, ca, cb in case["pairs"]]
    assert all(a < b for a, b, _, _ in want)
    pairs, census, nbrs = hr.brute(case["table"], k, lo, hi, middle)
    assert pairs == want and census == case["census"]
    r = hr.restate(*table_arrays(case["table"]), k, lo, hi, middle)
    assert pairs_of(r) == want and r.census.tolist() == case["census"]


def test_the_worked_example_of_the_rule():
    # N(ACCGT) = {ACAGT}: reached by C->A and by C->T (ACTGT = rc(ACAGT)); C->G gives rc(ACCGT), ACCGT itself
    assert hr.rc_s("ACAGT") == "ACTGT" and hr.rc_s("ACCGT") == "ACGGT"
    _, census, nbrs = hr.brute({"ACAGT": 1, "ACCGT": 1}, 5)
    assert nbrs == {"ACAGT": ["ACCGT"], "ACCGT": ["ACAGT"]} and census[3] == 2 and census[5] == 1
    r = hr.restate(*table_arrays({"ACAGT": 1, "ACCGT": 1}), 5)
    assert r.subs.tolist() == [2, 2] and r.deg.tolist() == [1, 1]  # two substitutions, one neighbour
    w, pos = hr.written_b(hr.key_of("AAGT"), hr.key_of("ACTG"), 4, False)
    assert (hr.str_of(w, 4), pos) == ("CAGT", 0)


def test_the_fast_reverse_complement_is_the_plain_one():
    rng = np.random.default_rng(7)
    for k in (1, 2, 3, 4, 5, 15, 16, 17, 30, 31):
        x = rng.integers(0, 1 << 62, size=500, dtype=np.uint64) & np.uint64((1 << (2 * k)) - 1)
        x[:3] = (0, (1 << (2 * k)) - 1, 1)
        assert np.array_equal(hr.rc_fast(x, k), hr.rc_np(x, k)), k
        assert all(hr.str_of(r, k) == hr.rc_s(hr.str_of(v, k)) for v, r in zip(x[:40], hr.rc_np(x[:40], k))), k


@pytest.mark.parametrize("k", [3, 4, 5, 6])
def test_the_rule_is_symmetric_and_the_restatements_agree(k):
    rng = np.random.default_rng(2000 + k)
    every = hr.canonical_kmers(k)
    seen_pairs = seen_double = 0
    for trial in range(40 if k < 6 else 12):
        density = (0.05, 0.2, 0.5)[trial % 3]
        keys = every[rng.random(len(every)) < density]
        counts = rng.integers(1, 6, size=len(keys)).astype(np.uint32)
        table = {hr.str_of(v, k): int(c) for v, c in zip(keys, counts)}
        for lo, hi in ((1, None), (2, None), (1, 1), (2, 3)):
            for middle in ((False, True) if k % 2 else (False,)):
                pairs, census, nbrs = hr.brute(table, k, lo, hi, middle)
                assert hr.asymmetries(nbrs) == [], (k, trial, lo, hi, middle)
                r = hr.restate(keys, counts, k, lo, hi, middle)
                assert pairs_of(r) == pairs and r.census.tolist() == census, (k, trial, lo, hi, middle)
                assert [hr.str_of(v, k) for v in r.F] == sorted(nbrs)
                assert r.deg.tolist() == [len(nbrs[s]) for s in sorted(nbrs)]
                assert census[0] == census[2] + census[3] + census[4] and 2 * census[5] <= census[3]
                seen_pairs += census[5]
                seen_double += int((r.subs != r.deg).sum())
                for a, b, _, _ in pairs:
                    w, pos = hr.written_b(a, b, k, middle)
                    sa, sw = hr.str_of(a, k), hr.str_of(w, k)
                    assert [i for i in range(k) if sa[i] != sw[i]] == [pos] and hr.canon_s(sw) == hr.str_of(b, k)
    assert seen_pairs and seen_double


def test_middle_needs_an_odd_k():
    with pytest.raises(AssertionError):
        hr.restate(np.array([1], np.uint64), np.array([1], np.uint32), 4, middle=True)
