"""`--prefilter [--prefilter-bits N]` of ctr, graph, unitigs and hetmers on the CPU: the help texts, the refusals (below
--min-count 2, with --table, with --devices above 1, bits of 0, bits without the flag: usage errors, exit 2, before the
output directory is made; a filter of more than 2^34 words: refused from the input's size, before a device is opened), and the
host side of the sizing - the plan arithmetic, the stats writer - through the hidden `debug-prefilter`, under the plain build
and the address + undefined-behaviour sanitizer build of the command line.  No GPU."""
import pathlib
import subprocess

import pytest

from test_oracle_sanitize import BIN, CSRC, SAN_ENV, _clean

ROOT = pathlib.Path(__file__).resolve().parent.parent
CLI = ROOT / "kmertools_amd" / "bin" / "kmertools"
FASTA = ">a\nACGTACGTACGTACGTACGTACGTACGTACGTACGTACGTACGT\n"
COMMANDS = ("ctr", "graph", "unitigs", "hetmers")


@pytest.fixture(scope="module")
def cli():
    if not CLI.exists():
        subprocess.check_call(["make", "-C", str(CSRC), "-j4"], stdout=subprocess.DEVNULL)
    return str(CLI)


def run(cli, *args, env=None):
    return subprocess.run([cli, *map(str, args)], capture_output=True, text=True, timeout=300, env=env)


def is_usage_error(r, what):
    return (r.returncode == 2 and r.stderr.startswith("error: ") and what in r.stderr and
            "For more information, try '--help'." in r.stderr)


@pytest.mark.parametrize("cmd", COMMANDS)
def test_help_lists_the_flags(cli, cmd):
    r = run(cli, cmd, "--help")
    assert r.returncode == 0
    for text in ("--prefilter ", "--prefilter-bits <N>", "[default: 16]", "prefilter.stats", "KT_PREFILTER_SCALE", "Not with --table"):
        assert text in r.stdout, (cmd, text)
    assert ("--devices above 1.  KT_PREFILTER_SCALE" in r.stdout) == (cmd == "ctr")
    assert ("1<TAB>0" in r.stdout) == (cmd == "ctr")          # what --histo writes for count 1


@pytest.mark.parametrize("cmd", ("cov", "filter", "correct", "profile", "compare", "setop", "thread", "sketch", "card"))
def test_other_commands_do_not_take_it(cli, tmp_path, cmd):
    r = run(cli, cmd, "-i", tmp_path / "r.fa", "-o", tmp_path / "out", "--prefilter")
    assert is_usage_error(r, "--prefilter"), (cmd, r.stderr)


@pytest.mark.parametrize("cmd", COMMANDS)
@pytest.mark.parametrize("extra, what", [
    (("--prefilter",), "requires '--min-count <N>' of 2 or above"),                       # the default is 1
    (("--prefilter", "--min-count", "1"), "requires '--min-count <N>' of 2 or above"),
    (("--prefilter", "--min-count", "2", "--prefilter-bits", "0"), "--prefilter-bits"),
    (("--prefilter", "--min-count", "2", "--prefilter-bits", "x"), "--prefilter-bits"),
    (("--prefilter", "--min-count", "2", "--prefilter-bits"), "--prefilter-bits"),
    (("--min-count", "2", "--prefilter-bits", "8"), "requires '--prefilter'"),
])
def test_usage_errors(cli, tmp_path, cmd, extra, what):
    fa = tmp_path / "r.fa"
    fa.write_text(FASTA)
    out = tmp_path / "out"
    r = run(cli, cmd, "-i", fa, "-o", out, "-k", "21", *extra)
    assert is_usage_error(r, what), (cmd, r.returncode, r.stderr)
    assert not out.exists()


@pytest.mark.parametrize("cmd", COMMANDS)
def test_refused_with_a_table_file(cli, tmp_path, cmd):
    out = tmp_path / "out"
    r = run(cli, cmd, "--table", tmp_path / "t.kt", "-o", out, "-k", "21", "--prefilter", "--min-count", "2")
    assert is_usage_error(r, "'--prefilter' cannot be used with '--table <FILE>'"), (cmd, r.stderr)
    assert not out.exists()


def test_refused_with_several_devices(cli, tmp_path):
    fa = tmp_path / "r.fa"
    fa.write_text(FASTA)
    out = tmp_path / "out"
    r = run(cli, "ctr", "-i", fa, "-o", out, "-k", "21", "--prefilter", "--min-count", "2", "--devices", "2")
    assert is_usage_error(r, "'--prefilter' cannot be used with '--devices <N>' above 1"), r.stderr
    assert not out.exists()
    r = run(cli, "ctr", "-i", fa, "-o", out, "-k", "21", "--prefilter", "--min-count", "2", "--devices", "1", "--prefilter-bits", "1" + "0" * 13)
    assert is_usage_error(r, "--prefilter-bits")               # beyond the flag's range


@pytest.mark.parametrize("cmd", COMMANDS)
def test_a_filter_beyond_2_34_words_is_refused(cli, tmp_path, cmd):
    """45 bases bound the k-mers; 2^40 bits for each of them are 45 x 2^34 words.  Refused from the file's size: the message
    comes before a device is looked for (this machine has none: any device work would fail with another text)"""
    fa = tmp_path / "r.fa"
    fa.write_text(FASTA)
    out = tmp_path / "out"
    r = run(cli, cmd, "-i", fa, "-o", out, "-k", "21", "--prefilter", "--min-count", "2", "--prefilter-bits", 1 << 40)
    assert r.returncode == 101 and r.stderr.startswith("Error: --prefilter-bits 1099511627776"), (cmd, r.stderr)
    assert "more than 2^34 words" in r.stderr
    assert not out.exists() or not any(out.iterdir())


@pytest.mark.parametrize("which", ["plain", "asan"])
def test_host_side_of_the_sizing(tmp_path, which):
    subprocess.check_call(["make", "-C", str(CSRC), "asan"], stdout=subprocess.DEVNULL)
    exe = BIN / {"plain": "kmertools", "asan": "kmertools_asan"}[which]
    r = subprocess.run([str(exe), "debug-prefilter", str(tmp_path)], capture_output=True, env=SAN_ENV, timeout=600)
    _clean(r.stderr)
    assert r.returncode == 0, r.stdout[-500:] + r.stderr[-2000:]
    assert r.stderr == b"", r.stderr[-2000:]
    assert r.stdout == b"prefilter ok\n"
    assert list(tmp_path.iterdir()) == []        # it removes what it wrote
