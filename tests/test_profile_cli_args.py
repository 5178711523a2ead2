"""`kmertools profile` on the CPU: listed in the main --help, its own --help lists every flag, and every usage error exits 2
(an unknown input extension 101, as in `filter`) before any device is opened or the output directory is made.  Also the
bookkeeping of the two new C entry points: declared in the header, bound in _lib.SYMBOLS, shown in INTEGRATION.md."""
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


def run(cli, *args, env=None):
    return subprocess.run([cli, *map(str, args)], capture_output=True, text=True, timeout=300, env=env)


def test_main_help_lists_profile(cli):
    r = run(cli, "--help")
    assert r.returncode == 0
    assert "  profile " in r.stdout
    for cmd in ("comp", "cov", "min", "ctr", "filter", "compare", "help"):
        assert "  %s " % cmd in r.stdout, cmd


def test_profile_help_lists_every_flag(cli):
    r = run(cli, "profile", "--help")
    assert r.returncode == 0
    for flag in ("-i, --input <INPUT>", "-o, --output <OUTPUT>", "-k, --k-size <K_SIZE>", "-a, --alt-input <ALT_INPUT>",
                 "--positions", "-m, --memory <MEMORY>", "-t, --threads <THREADS>", "--device <DEVICE>", "-h, --help"):
        assert flag in r.stdout, flag
    # what an out-of-core count keeps on the host is said here
    assert "4 bytes per base" in r.stdout and "passes" in r.stdout
    assert "profile.stats" in r.stdout and "profile.counts" in r.stdout and "median" in r.stdout


@pytest.mark.parametrize("extra, what", [
    (("--k-size", "0"), "--k-size"),
    (("--k-size", "32"), "--k-size"),
    (("--k-size", "-3"), "--k-size"),
    (("--k-size", "x"), "--k-size"),
    (("--k-size",), "--k-size"),
    (("--memory", "5"), "--memory"),
    (("--threads", "many"), "--threads"),
    (("--device", "64"), "--device"),
    (("--min-count", "2"), "--min-count"),
    (("--bogus",), "--bogus"),
])
def test_profile_usage_errors(cli, tmp_path, extra, what):
    fa = tmp_path / "r.fa"
    fa.write_text(">a\nACGTACGTACGTACGTACGTACGTACGT\n")
    out = tmp_path / "out"
    args = ["profile", "-i", fa, "-o", out] + ([] if "--k-size" in extra else ["-k", "15"]) + list(extra)
    r = run(cli, *args)
    assert r.returncode == 2, r.stderr
    assert r.stderr.startswith("error: ") and what in r.stderr and "For more information, try '--help'." in r.stderr
    assert not out.exists()


@pytest.mark.parametrize("missing", ["-i", "-o", "-k"])
def test_profile_needs_its_required_flags(cli, tmp_path, missing):
    fa = tmp_path / "r.fa"
    fa.write_text(">a\nACGTACGTACGTACGTACGTACGTACGT\n")
    out = tmp_path / "out"
    args = {"-i": fa, "-o": out, "-k": "15"}
    del args[missing]
    r = run(cli, "profile", *[x for kv in args.items() for x in kv])
    long_name = {"-i": "--input", "-o": "--output", "-k": "--k-size"}[missing]
    assert r.returncode == 2 and long_name in r.stderr
    assert not out.exists()


@pytest.mark.parametrize("which", ["input", "alt-input", "stdin"])
def test_profile_unknown_extension(cli, tmp_path, which):
    fa = tmp_path / "r.fa"
    fa.write_text(">a\nACGTACGTACGTACGTACGTACGTACGT\n")
    bad = tmp_path / "r.txt"
    bad.write_text(">a\nACGTACGTACGTACGTACGTACGTACGT\n")
    out = tmp_path / "out"
    if which == "input":
        args = ("-i", bad)
    elif which == "alt-input":
        args = ("-i", fa, "-a", bad)
    else:
        args = ("-i", "-")
    r = run(cli, "profile", *args, "-o", out, "-k", "15")
    assert r.returncode == 101, r.stderr
    assert "unsupported input extension" in r.stderr
    assert not out.exists()


def test_profile_symbols_are_declared_bound_and_documented():
    from kmertools_amd import _lib
    header = (ROOT / "include" / "kmertools_hip.h").read_text()
    integ = (ROOT / "INTEGRATION.md").read_text()
    for name in ("kt_ctr_profile", "kt_profile_stats"):
        assert "int %s(" % name in header, name
        assert name in _lib.SYMBOLS, name
        assert "pub fn %s(" % name in integ, name
        assert hasattr(_lib.lib(), name)
    assert "#define KT_NO_KMER 0xFFFFFFFFu" in header and "n_kmers / 2" in header and "khmer" in header
