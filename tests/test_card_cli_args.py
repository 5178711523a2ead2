"""`kmertools card` and `--estimate-size` on the CPU: the help texts, every usage error (exit 2, an unknown input extension
101) before any device is opened or the output directory is made - the two sizing flags on each of the nine table commands
included -, the bookkeeping of the four new C entry points, and the three host functions against tests/card_ref.py:
kt_card_estimate within 1e-12 relative, kt_card_merge and kt_card_rel_error exactly.  The restatement itself is held to
the estimator's own error (5 standard errors on seeded inputs, so that a change of the formula cannot pass silently) and to
a pure-Python integer brute force of the registers."""
import math
import pathlib
import subprocess

import numpy as np
import pytest

import card_ref
from read_batches import brute_kmers

ROOT = pathlib.Path(__file__).resolve().parent.parent
CLI = ROOT / "kmertools_amd" / "bin" / "kmertools"
FASTA = ">a\nACGTACGTACGTACGTACGTACGTACGTACGTACGTACGTACGT\n"
KT_ERR_ARG = 1
TABLE_COMMANDS = ("ctr", "cov", "filter", "correct", "compare", "profile", "setop", "graph", "unitigs")


@pytest.fixture(scope="module")
def cli():
    if not CLI.exists():
        subprocess.check_call(["make", "-C", str(ROOT / "kmertools_amd" / "csrc"), "-j4"], stdout=subprocess.DEVNULL)
    return str(CLI)


def run(cli, *args, env=None):
    return subprocess.run([cli, *map(str, args)], capture_output=True, text=True, timeout=300, env=env)


def is_usage_error(r, what):
    return (r.returncode == 2 and r.stderr.startswith("error: ") and what in r.stderr and
            "For more information, try '--help'." in r.stderr)


# ---- card ------------------------------------------------------------------------------------------------------------------

def test_main_help_lists_card(cli):
    r = run(cli, "--help")
    assert r.returncode == 0
    assert "  card " in r.stdout
    for cmd in ("comp", "cov", "min", "ctr", "filter", "correct", "compare", "profile", "setop", "graph", "unitigs", "sketch", "help"):
        assert "  %s " % cmd in r.stdout, cmd


def test_card_help_lists_every_flag(cli):
    r = run(cli, "card", "--help")
    assert r.returncode == 0
    for flag in ("-i, --input <INPUT>", "-o, --output <OUTPUT>", "-k, --k-size <K_SIZE>", "-p, --precision <P>", "--seed <SEED>",
                 "-a, --alt-input <ALT_INPUT>", "-t, --threads <THREADS>", "--device <DEVICE>", "-h, --help"):
        assert flag in r.stdout, flag
    for name in ("card.stats", "card.registers", "card.alt.registers", "sequences", "bases", "kmers", "precision", "registers",
                 "zero_registers", "distinct_estimate", "rel_std_error", "slots_wanted", "alt_", "union_estimate",
                 "intersection_estimate", "jaccard_estimate"):
        assert name in r.stdout, name
    assert "[default: 14]" in r.stdout and "[default: 0]" in r.stdout and "4..16" in r.stdout and "1..31" in r.stdout


@pytest.mark.parametrize("extra, what", [
    (("-k", "0"), "--k-size"),
    (("-k", "32"), "--k-size"),
    (("-k", "-3"), "--k-size"),
    (("-k", "x"), "--k-size"),
    (("-k",), "-k"),
    ((), "--k-size"),                                   # required
    (("-k", "31", "-p", "3"), "--precision"),
    (("-k", "31", "-p", "17"), "--precision"),
    (("-k", "31", "--precision", "many"), "--precision"),
    (("-k", "31", "--precision"), "--precision"),
    (("-k", "31", "--seed", "x"), "--seed"),
    (("-k", "31", "--seed"), "--seed"),
    (("-k", "31", "--threads", "many"), "--threads"),
    (("-k", "31", "--device", "64"), "--device"),
    (("-k", "31", "-a"), "-a"),
    (("-k", "31", "--bogus"), "--bogus"),
    (("-k", "31", "--estimate-size"), "--estimate-size"),   # the table commands' flag, not card's
])
def test_card_usage_errors(cli, tmp_path, extra, what):
    fa = tmp_path / "r.fa"
    fa.write_text(FASTA)
    out = tmp_path / "out"
    r = run(cli, "card", "-i", fa, "-o", out, *extra)
    assert is_usage_error(r, what), (r.returncode, r.stderr)
    assert not out.exists()


@pytest.mark.parametrize("missing", ["-i", "-o"])
def test_card_needs_its_required_flags(cli, tmp_path, missing):
    fa = tmp_path / "r.fa"
    fa.write_text(FASTA)
    out = tmp_path / "out"
    args = {"-i": fa, "-o": out}
    del args[missing]
    r = run(cli, "card", "-k", "21", *[x for kv in args.items() for x in kv])
    assert r.returncode == 2 and {"-i": "--input", "-o": "--output"}[missing] in r.stderr
    assert not out.exists()


@pytest.mark.parametrize("which", ["input", "alt-input", "stdin"])
def test_card_unknown_extension(cli, tmp_path, which):
    fa = tmp_path / "r.fa"
    fa.write_text(FASTA)
    bad = tmp_path / "r.txt"
    bad.write_text(FASTA)
    out = tmp_path / "out"
    args = {"input": ("-i", bad), "alt-input": ("-i", fa, "-a", bad), "stdin": ("-i", "-")}[which]
    r = run(cli, "card", *args, "-o", out, "-k", "21")
    assert r.returncode == 101, r.stderr
    assert "unsupported input extension" in r.stderr
    assert not out.exists()


# ---- --estimate-size / --estimate-precision on the nine table commands ----------------------------------------------------------

def table_args(cmd, fa, out):
    args = ["-i", fa, "-o", out]
    if cmd != "cov":
        args += ["-k", "21"]
    if cmd in ("compare", "setop"):
        args += ["-a", fa]
    if cmd == "setop":
        args += ["--op", "intersect"]
    return args


@pytest.mark.parametrize("cmd", TABLE_COMMANDS)
def test_table_command_help_lists_the_sizing_flags(cli, cmd):
    r = run(cli, cmd, "--help")
    assert r.returncode == 0
    assert "--estimate-size " in r.stdout and "--estimate-precision <P>" in r.stdout, cmd
    assert "[default: 14]" in r.stdout and "4..16" in r.stdout, cmd
    # the sharded path keeps its bound: said where there is one
    assert ("--devices above 1" in r.stdout) == (cmd in ("ctr", "cov")), cmd


@pytest.mark.parametrize("cmd", TABLE_COMMANDS)
@pytest.mark.parametrize("extra, what", [
    (("--estimate-precision", "12"), "requires '--estimate-size'"),
    (("--estimate-size", "--estimate-precision", "3"), "--estimate-precision"),
    (("--estimate-size", "--estimate-precision", "17"), "--estimate-precision"),
    (("--estimate-size", "--estimate-precision", "x"), "--estimate-precision"),
    (("--estimate-size", "--estimate-precision"), "--estimate-precision"),
])
def test_table_command_sizing_usage_errors(cli, tmp_path, cmd, extra, what):
    fa = tmp_path / "r.fa"
    fa.write_text(FASTA)
    out = tmp_path / "out"
    r = run(cli, cmd, *table_args(cmd, fa, out), *extra)
    assert is_usage_error(r, what), (cmd, r.returncode, r.stderr)
    assert not out.exists()


@pytest.mark.parametrize("cmd", ["ctr", "cov"])
def test_estimate_size_refuses_several_devices(cli, tmp_path, cmd):
    fa = tmp_path / "r.fa"
    fa.write_text(FASTA)
    out = tmp_path / "out"
    r = run(cli, cmd, *table_args(cmd, fa, out), "--estimate-size", "--devices", "2")
    assert is_usage_error(r, "--estimate-size") and "--devices" in r.stderr, (r.returncode, r.stderr)
    assert not out.exists()


# ---- the symbols -------------------------------------------------------------------------------------------------------------

def test_card_symbols_are_declared_bound_and_documented():
    from kmertools_amd import _lib
    header = (ROOT / "include" / "kmertools_hip.h").read_text()
    integ = (ROOT / "INTEGRATION.md").read_text()
    for name in ("kt_card_add_reads", "kt_card_merge", "kt_card_estimate"):
        assert "int %s(" % name in header, name
    assert "double kt_card_rel_error(" in header
    for name in ("kt_card_add_reads", "kt_card_merge", "kt_card_estimate", "kt_card_rel_error"):
        assert name in _lib.SYMBOLS, name
        assert "pub fn %s(" % name in integ, name
        assert hasattr(_lib.lib(), name)
    assert "#define KT_CARD_MIN_P 4" in header and "#define KT_CARD_MAX_P 16" in header
    assert (_lib.KT_CARD_MIN_P, _lib.KT_CARD_MAX_P) == (4, 16) == (card_ref.MIN_P, card_ref.MAX_P)
    for text in ("q = 64 - p", "j = h >> q", "sigma(x)", "tau(x)", "(m*m / (2 ln 2)) / z", "1.04 / sqrt(2^p)"):
        assert text in header, text


# ---- the host functions against the restatement --------------------------------------------------------------------------------

def close(got, want):
    if math.isinf(want) or want == 0.0:
        return got == want
    return abs(got - want) <= 1e-12 * abs(want)


def random_registers(p, n, seed):
    """the registers of n distinct random 62-bit words (what k-mers of k = 31 are), through the restated hash"""
    rng = np.random.default_rng(seed)
    x = np.unique(rng.integers(0, 1 << 62, size=n + n // 8 + 8, dtype=np.uint64))
    x = x[rng.permutation(len(x))][:n]
    assert len(x) == n
    return card_ref.registers_of_hashes(card_ref.mix64(x), p)


# (p, regime, seed): n = m / 100 distinct k-mers (at least 1: linear counting) and n = 20 m (the raw estimator)
SEEDED = [(p, regime, 11 * p + i) for p in (4, 10, 14, 16) for i, regime in enumerate(("linear", "raw"))]


def n_of(p, regime):
    m = 1 << p
    return max(1, m // 100) if regime == "linear" else 20 * m


@pytest.mark.parametrize("p, regime, seed", SEEDED)
def test_estimate_on_seeded_inputs(p, regime, seed):
    from kmertools_amd import device
    n = n_of(p, regime)
    reg = random_registers(p, n, seed)
    want, want_zeros = card_ref.estimate(reg)
    got, zeros = device.card_estimate(reg)
    assert zeros == want_zeros == int((reg == 0).sum())
    assert close(got, want), (got, want)
    # the restatement itself: within five standard errors of the truth (seeds chosen so that it is)
    assert abs(want / n - 1.0) <= 5.0 * 1.04 / math.sqrt(1 << p), (p, regime, n, want)


@pytest.mark.parametrize("p", [4, 5, 10, 14, 16])
def test_estimate_edges(p):
    from kmertools_amd import _lib, device
    m, q = 1 << p, 64 - p
    zero = np.zeros(m, np.uint8)
    got, zeros = device.card_estimate(zero)
    assert got == 0.0 and zeros == m and card_ref.estimate(zero) == (0.0, m)
    full = np.full(m, q + 1, np.uint8)
    got, zeros = device.card_estimate(full)
    assert zeros == 0 and close(got, card_ref.estimate(full)[0])
    for j, v in ((0, 1), (m - 1, q + 1), (m // 2, q), (1, 7)):
        one = np.zeros(m, np.uint8)
        one[j] = v
        got, zeros = device.card_estimate(one)
        want, _ = card_ref.estimate(one)
        assert zeros == m - 1 and close(got, want) and 0.9 < got < 1.2, (j, v, got, want)
    over = np.zeros(m, np.uint8)
    over[m - 1] = q + 2
    with pytest.raises(_lib.KmertoolsError) as e:
        device.card_estimate(over)
    assert e.value.code == KT_ERR_ARG
    with pytest.raises(ValueError):
        card_ref.estimate(over)
    # every count vector the loop sees: a staircase of all values 0..q+1
    stairs = (np.arange(m) % (q + 2)).astype(np.uint8)
    assert close(device.card_estimate(stairs)[0], card_ref.estimate(stairs)[0])


def test_estimate_refuses_other_lengths():
    from kmertools_amd import device
    from kmertools_amd import _lib
    for m in (0, 24):                      # no power of two
        with pytest.raises(ValueError):
            device.card_estimate(np.zeros(m, np.uint8))
    for m in (8, 1 << 17):                 # p = 3 and p = 17
        with pytest.raises(_lib.KmertoolsError) as e:
            device.card_estimate(np.zeros(m, np.uint8))
        assert e.value.code == KT_ERR_ARG


@pytest.mark.parametrize("p", [4, 9, 16])
def test_merge_is_the_maximum(p):
    from kmertools_amd import device
    rng = np.random.default_rng(p)
    a = rng.integers(0, 64 - p + 2, size=1 << p).astype(np.uint8)
    b = rng.integers(0, 64 - p + 2, size=1 << p).astype(np.uint8)
    want = np.maximum(a, b)
    b0 = b.copy()
    out = device.card_merge(a, b)
    assert out is a and np.array_equal(a, want) and np.array_equal(b, b0)
    # the registers of a union are the merged registers of its parts
    x, y = random_registers(p, 500, 1), random_registers(p, 700, 2)
    assert np.array_equal(device.card_merge(x.copy(), y), np.maximum(x, y))
    with pytest.raises(ValueError):
        device.card_merge(a, b[:len(b) // 2])


def test_rel_error():
    from kmertools_amd import device
    for p in range(4, 17):
        assert device.card_rel_error(p) == 1.04 / math.sqrt(float(1 << p)) == card_ref.rel_error(p)


# ---- the restatement against a brute force -------------------------------------------------------------------------------------

def test_unmix64_inverts_the_finaliser():
    rng = np.random.default_rng(5)
    for h in [0, 1, (1 << 64) - 1, 1 << 63, 0x9E3779B97F4A7C15] + [int(x) for x in rng.integers(0, 1 << 63, size=200, dtype=np.uint64)]:
        z = card_ref.unmix64(h)
        assert card_ref.mix64_int(z) == h and int(card_ref.mix64(np.array([z], np.uint64))[0]) == h


@pytest.mark.parametrize("k", [1, 5, 31])
@pytest.mark.parametrize("p", [4, 11, 16])
def test_restated_registers_against_brute_force(oracle, k, p):
    rng = np.random.default_rng(100 * k + p)
    seqs = []
    for L in (0, 3, 40, 200, 31, 64):
        s = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, size=L)].copy()
        if L > 50:
            s[rng.integers(0, L, size=3)] = ord("N")
            s[5:9] |= 0x20
        seqs.append(s.tobytes())
    from kmertools_amd import device
    bases, offsets = device.to_csr(seqs)
    seed = 0x1234567 * p
    got, windows = card_ref.registers(oracle, bases, offsets, k, p, seed)
    kmers = [min(f, r) for s in seqs for f, r, _ in brute_kmers(s, k)]
    assert windows == len(kmers) and (k > 5 or windows > 200)
    assert np.array_equal(got, card_ref.brute_registers(kmers, p, seed))
    # ranks at the edges: a low word of zero, of one, with its top bit set
    q = 64 - p
    h = np.array([(3 << q) | 0, (3 << q) | 1, (3 << q) | (1 << (q - 1)), (1 << q) - 1], np.uint64)
    j, r = card_ref.ranks_of(h, p)
    assert j.tolist() == [3, 3, 3, 0] and r.tolist() == [q + 1, q, 1, 1]
