"""`kmertools setop` on the CPU: listed in the main --help, its own --help lists every flag and both output files, every
usage error exits 2 with a clap-style message before any device is opened or the output directory is made, and an input
of an unknown extension exits 101 (as in `compare`)."""
import pathlib
import subprocess

import pytest

ROOT = pathlib.Path(__file__).resolve().parent.parent
CLI = ROOT / "kmertools_amd" / "bin" / "kmertools"


@pytest.fixture(scope="module")
def cli():
    if not CLI.exists():
        subprocess.check_call(["make", "-C", str(ROOT / "kmertools_amd" / "csrc"), "-j4"], stdout=subprocess.DEVNULL)
    return str(CLI)


def run(cli, *args):
    return subprocess.run([cli, *map(str, args)], capture_output=True, text=True, timeout=300)


def test_main_help_lists_setop(cli):
    r = run(cli, "--help")
    assert r.returncode == 0
    assert "  setop " in r.stdout
    for cmd in ("comp", "cov", "min", "ctr", "filter", "compare", "profile", "help"):
        assert "  %s " % cmd in r.stdout, cmd


def test_setop_help_lists_every_flag(cli):
    for h in ("--help", "-h"):
        r = run(cli, "setop", h)
        assert r.returncode == 0
        for flag in ("-i, --input <INPUT>", "-a, --alt-input <ALT_INPUT>", "-o, --output <OUTPUT>", "-k, --k-size <K_SIZE>",
                     "--op <OP>", "--count <COUNT>", "--min-a <N>", "--max-a <N>", "--min-b <N>", "--max-b <N>", "--acgt",
                     "-m, --memory <MEMORY>", "-t, --threads <THREADS>", "--device <DEVICE>", "-h, --help",
                     "intersect", "subtract", "union", "xor", "first", "min", "max", "sum", "kmers.counts", "setop.stats"):
            assert flag in r.stdout, flag


@pytest.fixture
def inputs(tmp_path):
    fa = tmp_path / "a.fa"
    fa.write_text(">a\nACGTACGTACGTACGTACGTACGTACGTAAACCCGGGTTT\n")
    fq = tmp_path / "b.fq"
    fq.write_text("@b\nACGTACGTACGTACGTACGTACGTACGTTT\n+\nIIIIIIIIIIIIIIIIIIIIIIIIIIIIII\n")
    return fa, fq, tmp_path / "out"


@pytest.mark.parametrize("extra, what", [
    (("--k-size", "9"), "--k-size"),
    (("--k-size", "32"), "--k-size"),
    (("--k-size", "x"), "--k-size"),
    (("--op", "both"), "--op"),
    (("--op", ""), "--op"),
    (("--op", "Intersect"), "--op"),
    (("--count", "avg"), "--count"),
    (("--min-a", "0"), "--min-a"),
    (("--min-b", "0"), "--min-b"),
    (("--max-a", "0"), "--max-a"),
    (("--min-b", "5", "--max-b", "4"), "--min-b"),
    (("--min-a", "3", "--max-a", "2"), "--min-a"),
    (("--min-a", "-3"), "--min-a"),
    (("--max-b", "ten"), "--max-b"),
    (("--max-a", "4294967296"), "--max-a"),
    (("--memory", "5"), "--memory"),
    (("--threads", "x"), "--threads"),
    (("--device", "64"), "--device"),
    (("--bogus",), "--bogus"),
    (("-z",), "-z"),
    (("--max-a",), "--max-a"),
    (("--count",), "--count"),
    (("stray",), "stray"),
])
def test_setop_usage_errors(cli, inputs, extra, what):
    fa, fq, out = inputs
    args = ["setop", "-i", fa, "-a", fq, "-o", out]
    args += [] if "--k-size" in extra else ["-k", "15"]
    args += [] if "--op" in extra else ["--op", "intersect"]
    r = run(cli, *args, *extra)
    assert r.returncode == 2, r.stderr
    assert r.stderr.startswith("error: ") and what in r.stderr and "For more information, try '--help'." in r.stderr
    assert not out.exists()


def test_setop_op_without_value(cli, inputs):
    fa, fq, out = inputs
    r = run(cli, "setop", "-i", fa, "-a", fq, "-o", out, "-k", "15", "--op")
    assert r.returncode == 2
    assert r.stderr.startswith("error: a value is required for '--op'")
    assert not out.exists()


@pytest.mark.parametrize("drop", ["-i", "-a", "-o", "-k", "--op"])
def test_setop_required_flags(cli, inputs, drop):
    fa, fq, out = inputs
    flags = {"-i": fa, "-a": fq, "-o": out, "-k": 15, "--op": "union"}
    args = ["setop"] + [x for f, v in flags.items() if f != drop for x in (f, v)]
    r = run(cli, *args)
    assert r.returncode == 2
    long_ = {"-i": "--input", "-a": "--alt-input", "-o": "--output", "-k": "--k-size", "--op": "--op"}[drop]
    assert "required arguments were not provided" in r.stderr and long_ in r.stderr
    assert not out.exists()


def test_setop_widest_ranges_are_not_a_usage_error(cli, inputs, tmp_path):
    # min == max and the largest count are allowed: the call gets past the argument checks (to the extension check here)
    fa, fq, out = inputs
    bad = tmp_path / "b.txt"
    bad.write_text(">x\nACGT\n")
    r = run(cli, "setop", "-i", fa, "-a", bad, "-o", out, "-k", "15", "--op", "xor", "--count", "sum", "--min-a", "4294967295",
            "--max-a", "4294967295", "--min-b", "4", "--max-b", "4", "--acgt")
    assert r.returncode == 101 and r.stderr.startswith("Error: unsupported input extension")
    assert not out.exists()


@pytest.mark.parametrize("which", ["input", "alt"])
def test_setop_bad_extension(cli, inputs, tmp_path, which):
    fa, fq, out = inputs
    bad = tmp_path / "reads.txt"
    bad.write_text(">x\nACGTACGTACGTACGTACGT\n")
    a, b = (bad, fq) if which == "input" else (fa, bad)
    r = run(cli, "setop", "-i", a, "-a", b, "-o", out, "-k", "15", "--op", "subtract")
    assert r.returncode == 101
    assert r.stderr.startswith("Error: unsupported input extension") and "reads.txt" in r.stderr
    assert not (out / "kmers.counts").exists()
