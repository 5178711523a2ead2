"""`kmertools ctr`'s output filters and spectrum flags on the CPU: listed in --help, and values out of range refused
with a usage error (exit 2) before any device is opened."""
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
    return subprocess.run([cli, *map(str, args)], capture_output=True, text=True, timeout=120)


def test_ctr_help_lists_the_spectrum_flags(cli):
    r = run(cli, "ctr", "--help")
    assert r.returncode == 0
    for flag in ("--min-count <N>", "--max-count <N>", "--histo ", "--histo-max <H>", "--histo-only"):
        assert flag in r.stdout, flag


@pytest.mark.parametrize("extra, what", [
    (("--min-count", "3", "--max-count", "2"), "--min-count"),
    (("--histo-max", "0"), "--histo-max"),
    (("--histo-max", str(1 << 24)), "--histo-max"),
    (("--min-count", "-1"), "--min-count"),
    (("--min-count", "0"), "--min-count"),
    (("--max-count", "4294967296"), "--max-count"),
    (("--max-count",), "--max-count"),
])
def test_ctr_spectrum_flags_out_of_range(cli, tmp_path, extra, what):
    fa = tmp_path / "r.fa"
    fa.write_text(">a\nACGTACGTACGTACGTACGTACGTACGT\n")
    out = tmp_path / "out"
    # nothing here may reach the device: the usage error comes first, before the output directory is made
    r = run(cli, "ctr", "-i", fa, "-o", out, "-k", "15", *extra)
    assert r.returncode == 2, r.stderr
    assert r.stderr.startswith("error: ") and what in r.stderr and "For more information, try '--help'." in r.stderr
    assert not out.exists()
