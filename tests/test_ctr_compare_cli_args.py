"""`kmertools compare` on the CPU: listed in the main --help, its own --help lists every flag, every usage error exits 2
with a clap-style message before any device is opened or the output directory is made, and an input of an unknown
extension exits 101 (as in `cov` and `filter`)."""
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


def test_main_help_lists_compare(cli):
    r = run(cli, "--help")
    assert r.returncode == 0
    assert "  compare " in r.stdout
    for cmd in ("comp", "cov", "min", "ctr", "filter", "help"):
        assert "  %s " % cmd in r.stdout, cmd


def test_compare_help_lists_every_flag(cli):
    for h in ("--help", "-h"):
        r = run(cli, "compare", h)
        assert r.returncode == 0
        for flag in ("-i, --input <INPUT>", "-a, --alt-input <ALT_INPUT>", "-o, --output <OUTPUT>", "-k, --k-size <K_SIZE>",
                     "--max-a <N>", "--max-b <N>", "-m, --memory <MEMORY>", "-t, --threads <THREADS>", "--device <DEVICE>",
                     "-h, --help", "compare.matrix", "compare.stats"):
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
    (("--max-a", "0"), "--max-a"),
    (("--max-b", "0"), "--max-b"),
    (("--max-a", "-3"), "--max-a"),
    (("--max-b", "ten"), "--max-b"),
    (("--max-a", "4096", "--max-b", "4096"), "--max-a"),
    (("--max-a", "16777215", "--max-b", "1"), "--max-a"),
    (("--max-a", "99999999999"), "--max-a"),
    (("--memory", "5"), "--memory"),
    (("--threads", "x"), "--threads"),
    (("--device", "64"), "--device"),
    (("--bogus",), "--bogus"),
    (("-z",), "-z"),
    (("--max-a",), "--max-a"),
    (("stray",), "stray"),
])
def test_compare_usage_errors(cli, inputs, extra, what):
    fa, fq, out = inputs
    args = ["compare", "-i", fa, "-a", fq, "-o", out] + ([] if "--k-size" in extra else ["-k", "15"]) + list(extra)
    r = run(cli, *args)
    assert r.returncode == 2, r.stderr
    assert r.stderr.startswith("error: ") and what in r.stderr and "For more information, try '--help'." in r.stderr
    assert not out.exists()


@pytest.mark.parametrize("drop", ["-i", "-a", "-o", "-k"])
def test_compare_required_flags(cli, inputs, drop):
    fa, fq, out = inputs
    flags = {"-i": fa, "-a": fq, "-o": out, "-k": 15}
    args = ["compare"] + [x for f, v in flags.items() if f != drop for x in (f, v)]
    r = run(cli, *args)
    assert r.returncode == 2
    long_ = {"-i": "--input", "-a": "--alt-input", "-o": "--output", "-k": "--k-size"}[drop]
    assert "required arguments were not provided" in r.stderr and long_ in r.stderr
    assert not out.exists()


def test_compare_largest_matrix_is_not_a_usage_error(cli, inputs, tmp_path):
    # (max_a + 1) * (max_b + 1) == 2^24 is allowed: the call gets past the argument checks (to the extension check here)
    fa, fq, out = inputs
    bad = tmp_path / "b.txt"
    bad.write_text(">x\nACGT\n")
    r = run(cli, "compare", "-i", fa, "-a", bad, "-o", out, "-k", "15", "--max-a", "8388607", "--max-b", "1")
    assert r.returncode == 101 and r.stderr.startswith("Error: unsupported input extension")


@pytest.mark.parametrize("which", ["input", "alt"])
def test_compare_bad_extension(cli, inputs, tmp_path, which):
    fa, fq, out = inputs
    bad = tmp_path / "reads.txt"
    bad.write_text(">x\nACGTACGTACGTACGTACGT\n")
    a, b = (bad, fq) if which == "input" else (fa, bad)
    r = run(cli, "compare", "-i", a, "-a", b, "-o", out, "-k", "15")
    assert r.returncode == 101
    assert r.stderr.startswith("Error: unsupported input extension") and "reads.txt" in r.stderr
    assert not (out / "compare.matrix").exists()
