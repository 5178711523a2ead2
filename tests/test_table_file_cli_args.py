"""`ctr --save-table` and `--table` / `--alt-table` on the CPU: the help texts of all nine commands list the flags, and every
usage error exits 2 with a clap-style message before any device is opened or the output directory is made."""
import pathlib
import subprocess
import sys

import numpy as np
import pytest

ROOT = pathlib.Path(__file__).resolve().parent.parent
CLI = ROOT / "kmertools_amd" / "bin" / "kmertools"
sys.path.insert(0, str(ROOT / "tests"))
import ktab_ref as R  # noqa: E402

WHOLE = ("graph", "unitigs", "hetmers")           # --table stands in for --input
LOOKUP = ("cov", "filter", "correct", "profile")  # --table stands in for --alt-input, the counted input
PAIRS = ("compare", "setop")                      # --table for --input (A), --alt-table for --alt-input (B)
K = 21


@pytest.fixture(scope="module")
def cli():
    if not CLI.exists():
        subprocess.check_call(["make", "-C", str(ROOT / "kmertools_amd" / "csrc"), "-j4"], stdout=subprocess.DEVNULL)
    return str(CLI)


def run(cli, *args):
    return subprocess.run([cli, *map(str, args)], capture_output=True, text=True, timeout=300)


@pytest.fixture
def files(tmp_path):
    fa = tmp_path / "a.fa"
    fa.write_text(">a\nACGTACGTACGTACGTACGTACGTACGTAAACCCGGGTTT\n")
    tab = tmp_path / "k21.ktab"
    R.write_file(tab, K, [(np.array([5, 9], np.uint64), np.array([1, 300], np.uint32))])
    return fa, tab, tmp_path / "out"


def base_args(cmd, fa, out):
    """the command's other required arguments (the read-level commands keep their --input)"""
    extra = {"setop": ["--op", "union"]}.get(cmd, [])
    return (["-i", fa] if cmd in LOOKUP else []) + ["-o", out, *extra]


def test_help_lists_the_flags(cli):
    r = run(cli, "ctr", "--help")
    assert r.returncode == 0 and "--save-table <FILE>" in r.stdout and "--table <FILE>" in r.stdout
    for cmd in WHOLE + LOOKUP + PAIRS:
        r = run(cli, cmd, "--help")
        assert r.returncode == 0 and "--table <FILE>" in r.stdout and "ctr --save-table" in r.stdout, cmd
        assert "--save-table <FILE>" not in r.stdout, cmd
        assert ("--alt-table <FILE>" in r.stdout) == (cmd in PAIRS), cmd


def usage_error(r, out, *words):
    assert r.returncode == 2, (r.returncode, r.stderr)
    assert r.stderr.startswith("error: ") and "For more information, try '--help'." in r.stderr, r.stderr
    for w in words:
        assert w in r.stderr, (w, r.stderr)
    assert r.stdout == "" and not out.exists()


def test_save_table_with_devices_above_one(cli, files):
    fa, tab, out = files
    r = run(cli, "ctr", "-i", fa, "-o", out, "-k", K, "--save-table", out.parent / "s.ktab", "--devices", 2)
    usage_error(r, out, "'--save-table <FILE>' cannot be used with '--devices <N>' above 1")
    assert not (out.parent / "s.ktab").exists()
    r = run(cli, "ctr", "-i", fa, "-o", out, "-k", K, "--save-table")
    usage_error(r, out, "a value is required for '--save-table'")


@pytest.mark.parametrize("cmd", ("ctr",) + WHOLE + LOOKUP + PAIRS)
def test_table_usage_errors(cli, files, cmd):
    fa, tab, out = files
    rest = base_args(cmd, fa, out) + (["-a", fa] if cmd in PAIRS else [])
    # --table beside the input it replaces: -a where -a is the counted input, else -i
    replaced = ["-a", fa] if cmd in LOOKUP else ["-i", fa]
    text = "'--alt-input <ALT_INPUT>'" if cmd in LOOKUP else "'--input <INPUT>'"
    usage_error(run(cli, cmd, "--table", tab, *replaced, *rest, "-k", K), out, "'--table <FILE>' cannot be used with " + text)
    usage_error(run(cli, cmd, "--table", tab, *rest, "-k", K, "--estimate-size"), out, "'--table <FILE>' cannot be used with '--estimate-size'")
    usage_error(run(cli, cmd, "--table", tab, *rest, "-k", 23), out, "invalid value '23' for '--k-size <K_SIZE>'", "holds k = 21")
    if cmd != "cov":  # (cov's -k has a default, 15, as before: it then differs from the file's)
        usage_error(run(cli, cmd, "--table", tab, *rest), out, "--k-size")  # -k stays required
    else:
        usage_error(run(cli, cmd, "--table", tab, *rest), out, "invalid value '15' for '--k-size <K_SIZE>'", "holds k = 21")
    usage_error(run(cli, cmd, "--table", out.parent / "absent.ktab", *rest, "-k", K), out, "'--table <FILE>'", "cannot open")
    usage_error(run(cli, cmd, "--table", fa, *rest, "-k", K), out, "'--table <FILE>'", "bad magic")
    bad = out.parent / "short.ktab"
    bad.write_bytes(tab.read_bytes()[:-1])
    usage_error(run(cli, cmd, "--table", bad, *rest, "-k", K), out, "truncated")
    if cmd in ("ctr", "cov"):  # the commands that have --devices
        usage_error(run(cli, cmd, "--table", tab, *rest, "-k", K, "--devices", 2), out,
                    "'--table <FILE>' cannot be used with '--devices <N>' above 1")
    else:  # the others have no --devices: a sharded table cannot be loaded
        usage_error(run(cli, cmd, "--table", tab, *rest, "-k", K, "--devices", 2), out, "unexpected argument '--devices'")
    if cmd not in LOOKUP:  # without --table the input stays required
        usage_error(run(cli, cmd, "-o", out, "-k", K, *(["-a", fa] if cmd in PAIRS else []), *(["--op", "union"] if cmd == "setop" else [])),
                    out, "--input")


@pytest.mark.parametrize("cmd", PAIRS)
def test_alt_table_usage_errors(cli, files, cmd):
    fa, tab, out = files
    op = ["--op", "union"] if cmd == "setop" else []
    usage_error(run(cli, cmd, "-i", fa, "--alt-table", tab, "-a", fa, "-o", out, "-k", K, *op), out,
                "'--alt-table <FILE>' cannot be used with '--alt-input <ALT_INPUT>'")
    usage_error(run(cli, cmd, "-i", fa, "--alt-table", tab, "-o", out, "-k", K, *op, "--estimate-size"), out,
                "'--alt-table <FILE>' cannot be used with '--estimate-size'")
    usage_error(run(cli, cmd, "--table", tab, "--alt-table", tab, "-o", out, "-k", 22, *op), out, "holds k = 21")
    usage_error(run(cli, cmd, "-i", fa, "--alt-table", fa, "-o", out, "-k", K, *op), out, "'--alt-table <FILE>'", "bad magic")
    usage_error(run(cli, cmd, "-i", fa, "-o", out, "-k", K, *op), out, "--alt-input")  # without --alt-table B stays required
