"""`kmertools sketch --scaled` on the CPU: the help lists every new flag and sketch.contain, every usage error exits 2
before any device is opened or the output directory is made; the bookkeeping of the new C entry points - declared in the
header, bound in _lib.SYMBOLS, shown in INTEGRATION.md; the two host helpers, kt_scaled_max_hash against Python integers and
kt_containment_ani against math.pow; and the restatement the GPU suite compares with (tests/scaled_ref.py): mix64 and its
inverse round-trip, and its kept sets and abundances are those of a string-level pure-Python brute force."""
import math
import pathlib
import subprocess

import numpy as np
import pytest

import scaled_ref as sr

ROOT = pathlib.Path(__file__).resolve().parent.parent
CLI = ROOT / "kmertools_amd" / "bin" / "kmertools"
FASTA = ">a\nACGTACGTACGTACGTACGTACGTACGT\n"
NEW_SYMBOLS = ("kt_scaled_batch", "kt_scaled_merge", "kt_ctr_scaled", "kt_scaled_pairs", "kt_scaled_max_hash", "kt_containment_ani")


@pytest.fixture(scope="module")
def cli():
    if not CLI.exists():
        subprocess.check_call(["make", "-C", str(ROOT / "kmertools_amd" / "csrc"), "-j4"], stdout=subprocess.DEVNULL)
    return str(CLI)


def run(cli, *args, env=None):
    return subprocess.run([cli, *map(str, args)], capture_output=True, text=True, timeout=300, env=env)


def test_sketch_help_lists_the_scaled_flags(cli):
    r = run(cli, "sketch", "--help")
    assert r.returncode == 0
    for flag in ("--scaled <N>", "--abund", "--table <FILE>", "--min-count <L>", "--max-count <U>", "--contain", "--min-contain <C>",
                 "--single", "-a, --alt-input <ALT_INPUT>", "-s, --sketch-size <S>", "--dist", "--max-dist <D>"):
        assert flag in r.stdout, flag
    for name in ("sketch.tsv", "sketch.alt.tsv", "sketch.dist", "sketch.contain"):
        assert name in r.stdout, name
    assert "id_a<TAB>id_b<TAB>shared<TAB>size_a<TAB>size_b<TAB>jaccard<TAB>a_in_b<TAB>b_in_a<TAB>ani" in r.stdout
    m = run(cli, "--help")
    assert m.returncode == 0 and "  sketch " in m.stdout and "scaled" in m.stdout


@pytest.mark.parametrize("extra, what", [
    (("--scaled", "0"), "--scaled"),
    (("--scaled", "x"), "--scaled"),
    (("--scaled", "-1"), "--scaled"),
    (("--scaled",), "--scaled"),
    (("--scaled", "10", "-s", "100"), "--sketch-size"),          # exclusive
    (("--scaled", "10", "--sketch-size", "100"), "--sketch-size"),
    (("--scaled", "10", "--dist"), "--dist"),
    (("--scaled", "10", "--dist", "--max-dist", "0.5"), "--dist"),
    (("--scaled", "10", "--max-dist", "0.5"), "--max-dist"),
    (("--abund",), "--abund"),                                   # without --scaled
    (("--contain",), "--contain"),
    (("--contain", "--min-contain", "0.5"), "--contain"),
    (("--min-contain", "0.5"), "--min-contain"),
    (("--scaled", "10", "--min-contain", "0.5"), "--min-contain"),  # without --contain
    (("--scaled", "10", "--contain", "--min-contain", "1.5"), "--min-contain"),
    (("--scaled", "10", "--contain", "--min-contain", "-0.1"), "--min-contain"),
    (("--scaled", "10", "--contain", "--min-contain", "x"), "--min-contain"),
    (("--scaled", "10", "--contain", "--min-contain", "nan"), "--min-contain"),
    (("--scaled", "10", "--min-count", "2"), "--min-count"),     # without --table
    (("--scaled", "10", "--max-count", "2"), "--max-count"),
    (("--min-count", "2"), "--min-count"),
])
def test_scaled_usage_errors(cli, tmp_path, extra, what):
    fa = tmp_path / "r.fa"
    fa.write_text(FASTA)
    out = tmp_path / "out"
    r = run(cli, "sketch", "-i", fa, "-o", out, *extra)
    assert r.returncode == 2, r.stderr
    assert r.stderr.startswith("error: ") and what in r.stderr and "For more information, try '--help'." in r.stderr
    assert not out.exists()


@pytest.mark.parametrize("case", ["no scaled", "with input", "not a table file", "other k", "min above max", "min 0"])
def test_table_flag_usage_errors(cli, tmp_path, case):
    import ktab_ref
    fa = tmp_path / "r.fa"
    fa.write_text(FASTA)
    tab = tmp_path / "t.ktab"
    ktab_ref.write_file(tab, 21, [(np.array([5, 9], np.uint64), np.array([1, 2], np.uint32))])
    out = tmp_path / "out"
    args = {"no scaled": ("--table", tab),
            "with input": ("--scaled", 10, "--table", tab, "-i", fa),
            "not a table file": ("--scaled", 10, "--table", fa),
            "other k": ("--scaled", 10, "--table", tab, "-k", 15),
            "min above max": ("--scaled", 10, "--table", tab, "--min-count", 5, "--max-count", 4),
            "min 0": ("--scaled", 10, "--table", tab, "--min-count", 0)}[case]
    r = run(cli, "sketch", "-o", out, *args)
    assert r.returncode == 2, (case, r.stderr)
    assert r.stderr.startswith("error: ") and not out.exists()


def test_scaled_symbols_are_declared_bound_and_documented():
    from kmertools_amd import _lib, device
    header = (ROOT / "include" / "kmertools_hip.h").read_text()
    integ = (ROOT / "INTEGRATION.md").read_text()
    for name in ("kt_scaled_batch", "kt_scaled_merge", "kt_ctr_scaled", "kt_scaled_pairs"):
        assert "int %s(" % name in header, name
    assert "uint64_t kt_scaled_max_hash(uint64_t scaled);" in header
    assert "double kt_containment_ani(uint64_t shared, uint64_t size, int k);" in header
    for name in NEW_SYMBOLS:
        assert name in _lib.SYMBOLS, name
        assert "pub fn %s(" % name in integ, name
        assert hasattr(_lib.lib(), name)
    for name in ("scaled_sketch", "scaled_sketch_host", "scaled_merge", "scaled_pairs", "scaled_pairs_host"):
        assert hasattr(device.Context, name), name
    assert hasattr(device.Counter, "scaled_sketch")
    assert callable(device.scaled_max_hash) and callable(device.containment_ani)
    assert "0xFFFFFFFFFFFFFFFF / scaled" in header and "row_offsets[0] == 0" in header and "not sourmash's" in header


def test_scaled_max_hash_against_python_integers():
    from kmertools_amd import device
    for scaled in (1, 2, 3, 1000, 1 << 32, 1 << 63, (1 << 64) - 1):
        assert device.scaled_max_hash(scaled) == ((1 << 64) - 1) // scaled == sr.max_hash(scaled), scaled
    assert device.scaled_max_hash(0) == 0
    assert device.scaled_max_hash(1) == (1 << 64) - 1 and device.scaled_max_hash((1 << 64) - 1) == 1


def test_containment_ani_against_the_formula():
    from kmertools_amd import device
    for k in (1, 4, 15, 21, 31):
        assert device.containment_ani(0, 0, k) == 0.0
        assert device.containment_ani(0, 1000, k) == 0.0
        assert device.containment_ani(5, 0, k) == 0.0
        for size in (1, 2, 3, 17, 1000, 123457, 1 << 40):
            assert device.containment_ani(size, size, k) == 1.0
            for shared in sorted({1, size // 3, size // 2, size - 1}):
                if not 0 < shared < size:
                    continue
                got, want = device.containment_ani(shared, size, k), math.pow(shared / size, 1.0 / k)
                assert abs(got - want) <= 1e-12, (shared, size, k, got, want)
                assert 0.0 < got < 1.0 or size > 1 << 39


def test_mix64_and_its_inverse_round_trip():
    rng = np.random.default_rng(5)
    values = [0, 1, 2, (1 << 64) - 1, (1 << 63), sr.C0, sr.max_hash(1000), sr.max_hash(1000) + 1] + [int(x) for x in
                                                                                                       rng.integers(0, 1 << 63, 200)]
    for v in values:
        assert sr.mix64_int(sr.inv_mix64(v)) == v, v
        assert sr.inv_mix64(sr.mix64_int(v)) == v, v
    arr = np.array(values, np.uint64)
    with np.errstate(over="ignore"):
        assert [int(x) for x in sr.mix64(arr)] == [sr.mix64_int(v) for v in values]


def test_restatement_against_a_string_level_brute_force(oracle):
    from kmertools_amd.device import to_csr
    rng = np.random.default_rng(11)
    seqs = ["", "A", "ACGT", "A" * 40, "AC" * 25, "ACGTACGT" * 5, "ACGTTGCAACGT" + "N" + "ACGTTGCAACGT", "GAATTC" * 7]
    for _ in range(32):
        L = int(rng.integers(0, 90))
        s = "".join("ACGT"[i] for i in rng.integers(0, 4, L))
        if L > 20 and rng.random() < 0.4:
            p = int(rng.integers(0, L))
            s = s[:p] + "N" + s[p + 1:]
        seqs.append(s)
    bases, offsets = to_csr([s.encode() for s in seqs])
    for k in (1, 5, 16, 17, 21, 31):
        for scaled in (1, 3, 50):
            seed = int(rng.integers(0, 1 << 63))
            rows = sr.read_rows(oracle, bases, offsets, k, scaled, seed)
            for s, (windows, h, a) in zip(seqs, rows):
                bw, kept = sr.brute_row(s, k, scaled, seed)
                assert windows == bw, (s, k)
                assert [int(x) for x in h] == sorted(kept), (s, k, scaled)
                assert [int(x) for x in a] == [kept[x] for x in sorted(kept)], (s, k, scaled)
    # unions: abundances add up and saturate
    h, a = sr.union([(np.array([3, 9], np.uint64), np.array([0xFFFFFFFF, 0x80000000], np.uint32)),
                     (np.array([3, 9, 11], np.uint64), np.array([1, 0x80000000, 7], np.uint32)),
                     (np.array([11], np.uint64), None)])
    assert h.tolist() == [3, 9, 11] and a.tolist() == [0xFFFFFFFF, 0xFFFFFFFF, 8]
