"""`--prefilter` end to end on the GPU, on the 20 kb genome at 30x with 1 % substitutions (tests/prefilter_ref.py): graph,
unitigs, hetmers and ctr write with the flag what they write without it; a table bound under which `unitigs --min-count 2`
is refused today is enough with the flag; a plan scaled down to a hundredth retries with larger tables and still writes
the same; the lines of prefilter.stats agree with each other.

kmers.counts is compared as a set of lines: its lines follow the table's slots, so their order changes with the table's
size - between a run with --prefilter and one without as between any two sizes - while the table file (sorted) and
kmers.histo are compared byte for byte."""
import os
import pathlib
import subprocess

import pytest

import prefilter_ref as ref

pytestmark = pytest.mark.gpu
ROOT = pathlib.Path(__file__).resolve().parent.parent
CLI = ROOT / "kmertools_amd" / "bin" / "kmertools"
K = 21
STATS = ("windows", "once_words", "twice_words", "once_bits_set", "twice_bits_set", "promotions", "table_slots", "table_keys",
         "table_retries")


@pytest.fixture(scope="module")
def cli():
    if not CLI.exists():
        subprocess.check_call(["make", "-C", str(ROOT / "kmertools_amd" / "csrc"), "-j4"], stdout=subprocess.DEVNULL)
    return str(CLI)


@pytest.fixture(scope="module")
def fasta(tmp_path_factory):
    fa = tmp_path_factory.mktemp("prefilter_cli") / "reads.fasta"
    fa.write_bytes(b"".join(b">r%d\n%s\n" % (i, s) for i, s in enumerate(ref.genome_reads())))
    return fa


def run(cli, *args, env=None):
    r = subprocess.run([cli, *map(str, args)], capture_output=True, timeout=600, env=dict(os.environ, **(env or {})))
    return r


def files(d):
    return {p.name: p.read_bytes() for p in sorted(pathlib.Path(d).iterdir())}


def stats_of(d):
    rows = [line.split("\t") for line in (pathlib.Path(d) / "prefilter.stats").read_text().splitlines()]
    assert tuple(r[0] for r in rows) == STATS and all(len(r) == 2 for r in rows)
    st = {name: int(v) for name, v in rows}
    assert st["table_keys"] <= st["table_slots"]
    assert st["once_bits_set"] <= 64 * st["once_words"] and st["twice_bits_set"] <= 64 * st["twice_words"]
    assert st["twice_words"] == max(1024, st["once_words"] // 4) and st["once_words"] & (st["once_words"] - 1) == 0
    assert 0 < st["promotions"] <= st["windows"] and st["twice_bits_set"] <= 4 * st["promotions"]
    assert st["promotions"] <= st["table_keys"]      # (a k-mer is promoted once at most, and pass 2 counts every promoted k-mer)
    return st


def same_but_stats(with_flag, without):
    a, b = files(with_flag), files(without)
    assert "prefilter.stats" in a and "prefilter.stats" not in b
    del a["prefilter.stats"]
    assert a.keys() == b.keys() and len(a) >= 2, (sorted(a), sorted(b))
    for name in a:
        assert a[name] == b[name], name


COMMANDS = {
    "graph": ["graph", "--min-count", 2],
    "unitigs_links": ["unitigs", "--min-count", 2, "--gfa", "--links", "--components"],
    "unitigs_simplify": ["unitigs", "--min-count", 3, "--max-count", 1000, "--clip-tips", "--pop-bubbles"],
    "hetmers": ["hetmers", "--min-count", 2],
}


@pytest.mark.parametrize("name", sorted(COMMANDS))
def test_same_files_with_the_flag(cli, fasta, tmp_path, name):
    cmd = COMMANDS[name]
    for d, extra in ((tmp_path / "plain", []), (tmp_path / "pre", ["--prefilter"])):
        r = run(cli, cmd[0], "-i", fasta, "-o", d, "-k", K, *cmd[1:], *extra)
        assert r.returncode == 0, r.stderr[-2000:]
    same_but_stats(tmp_path / "pre", tmp_path / "plain")
    st = stats_of(tmp_path / "pre")
    assert st["table_retries"] == 0 and st["windows"] == sum(len(s) - K + 1 for s in ref.genome_reads())
    # the table holds a fraction of the input's distinct k-mers
    assert st["table_keys"] < 30000


@pytest.mark.parametrize("bits", [None, 4])
def test_ctr_same_output(cli, fasta, tmp_path, bits):
    """--prefilter-bits 4: a filter small enough for false positives, which --min-count 2 leaves out of every file"""
    extra = ["--prefilter"] + (["--prefilter-bits", bits] if bits else [])
    for d, more in ((tmp_path / "plain", []), (tmp_path / "pre", extra)):
        r = run(cli, "ctr", "-i", fasta, "-o", d, "-k", K, "--min-count", 2, "--max-count", 50, "--histo", "--save-table", d / "t.kt", *more)
        assert r.returncode == 0, r.stderr[-2000:]
    a, b = files(tmp_path / "pre"), files(tmp_path / "plain")
    assert sorted(a) == ["kmers.counts", "kmers.histo", "prefilter.stats", "t.kt"] and sorted(b) == ["kmers.counts", "kmers.histo", "t.kt"]
    assert a["t.kt"] == b["t.kt"]
    assert sorted(a["kmers.counts"].splitlines()) == sorted(b["kmers.counts"].splitlines()) and len(a["kmers.counts"]) > 100000
    ha, hb = a["kmers.histo"].split(b"\n", 1), b["kmers.histo"].split(b"\n", 1)
    assert ha[0] == b"1\t0" and hb[0].startswith(b"1\t") and hb[0] != b"1\t0" and ha[1] == hb[1]
    st = stats_of(tmp_path / "pre")
    if bits:
        assert st["once_words"] < 1 << 17


def test_fits_where_the_unfiltered_table_is_refused(cli, fasta, tmp_path):
    """KT_CTR_MAX_SLOTS bounds the table below what the input's size asks for: `unitigs --min-count 2` is refused, with
    --prefilter the table of the k-mers seen twice fits and the files are those of the run without a bound"""
    env = {"KT_CTR_MAX_SLOTS": str(1 << 17)}
    r = run(cli, "unitigs", "-i", fasta, "-o", tmp_path / "refused", "-k", K, "--min-count", 2, env=env)
    assert r.returncode == 101 and b"unitigs needs the whole table on the device" in r.stderr and b"--prefilter" in r.stderr
    r = run(cli, "unitigs", "-i", fasta, "-o", tmp_path / "pre", "-k", K, "--min-count", 2, "--prefilter", env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    r = run(cli, "unitigs", "-i", fasta, "-o", tmp_path / "plain", "-k", K, "--min-count", 2)
    assert r.returncode == 0, r.stderr[-2000:]
    same_but_stats(tmp_path / "pre", tmp_path / "plain")
    assert stats_of(tmp_path / "pre")["table_slots"] <= 1 << 17


@pytest.mark.parametrize("cmd", ["unitigs", "ctr"])
def test_a_plan_too_small_retries(cli, fasta, tmp_path, cmd):
    more = ["--save-table", tmp_path / "t.kt"] if cmd == "ctr" else []
    r = run(cli, cmd, "-i", fasta, "-o", tmp_path / "pre", "-k", K, "--min-count", 2, "--prefilter", *more, env={"KT_PREFILTER_SCALE": "0.01"})
    assert r.returncode == 0, r.stderr[-2000:]
    st = stats_of(tmp_path / "pre")
    assert st["table_retries"] >= 1 and st["table_keys"] > 20000
    if cmd == "ctr":
        want = tmp_path / "t.kt"
        more = ["--save-table", tmp_path / "u.kt"]
    r = run(cli, cmd, "-i", fasta, "-o", tmp_path / "plain", "-k", K, "--min-count", 2, *more)
    assert r.returncode == 0, r.stderr[-2000:]
    if cmd == "ctr":
        assert want.read_bytes() == (tmp_path / "u.kt").read_bytes()
        a, b = files(tmp_path / "pre"), files(tmp_path / "plain")
        assert sorted(a["kmers.counts"].splitlines()) == sorted(b["kmers.counts"].splitlines())
    else:
        same_but_stats(tmp_path / "pre", tmp_path / "plain")


def test_with_estimate_size(cli, fasta, tmp_path):
    """the filter sized from the HyperLogLog estimate instead of the input's size"""
    for d, extra in ((tmp_path / "plain", []), (tmp_path / "pre", ["--prefilter", "--estimate-size"])):
        r = run(cli, "graph", "-i", fasta, "-o", d, "-k", K, "--min-count", 2, *extra)
        assert r.returncode == 0, r.stderr[-2000:]
    same_but_stats(tmp_path / "pre", tmp_path / "plain")
    # about 115 000 distinct k-mers at 16 bits: 2^15 words; the input's 600 000 bases would have taken 2^18
    assert stats_of(tmp_path / "pre")["once_words"] == 1 << 15
