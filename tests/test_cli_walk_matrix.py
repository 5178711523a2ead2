"""Batches x passes of the command line: every command that walks its input batch by batch and can count its table out of
core writes the same files whether the input comes in one batch or in tens (KT_CLI_BATCH_READS=7), whether the table is
resident or takes several passes (KT_CTR_MAX_SLOTS), and with both at once.  That the plain run is right is what each
command's own test establishes against its Python model; this one asserts the invariance only, four process launches a
case.  The files are compared byte for byte - except kmers.counts, whose line order is the table's (ctr, cov: unspecified,
as the reference's; setop: ascending within a pass, the passes one after the other): the same lines in any order, and for
setop the same bytes as long as the tables are resident."""
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "kmertools_amd", "bin", "kmertools")
K = 15


@pytest.fixture(scope="module")
def cli_bin():
    if not os.path.exists(CLI):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "kmertools_amd", "csrc"), "-j4"], stdout=subprocess.DEVNULL)
    return CLI


def sample_reads(rng, genome, n):
    """n reads of 40..120 bases of the genome with 1 % substitutions"""
    reads = []
    for _ in range(n):
        length = int(rng.integers(40, 121))
        start = int(rng.integers(0, len(genome) - length + 1))
        read = genome[start:start + length].copy()
        hit = rng.random(length) < 0.01
        read[hit] = (read[hit] + rng.integers(1, 4, int(hit.sum()))) % 4
        reads.append(bytes(b"ACGT"[c] for c in read))
    return reads


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    """the same ~300 reads as FASTA and as FASTQ, and a second FASTA that shares half of them (the two-table commands)"""
    rng = np.random.default_rng(20240607)
    genome = rng.integers(0, 4, 3000)
    reads = sample_reads(rng, genome, 300)
    reads[17] = reads[17][:K - 1]                                        # shorter than k: no k-mer
    reads[101] = reads[101][:30] + b"N" * 9 + reads[101][39:]             # an N run
    reads[202] = reads[202].lower()                                      # lower case
    other = reads[150:] + sample_reads(rng, (genome + (rng.random(3000) < 0.05)) % 4, 60)
    d = tmp_path_factory.mktemp("walk_matrix")
    fa, fq, fb = d / "reads.fasta", d / "reads.fastq", d / "other.fa"
    fa.write_bytes(b"".join(b">r%d lane=%d  x\n%s\n" % (i, i % 3, s) for i, s in enumerate(reads)))
    fb.write_bytes(b"".join(b">o%d\n%s\n" % (i, s) for i, s in enumerate(other)))
    quals = [bytes(rng.integers(35, 74, len(s)).astype(np.uint8)) for s in reads]
    fq.write_bytes(b"".join(b"@r%d lane=%d  x\n%s\n+\n%s\n" % (i, i % 3, s, q) for i, (s, q) in enumerate(zip(reads, quals))))
    return {"fa": fa, "fq": fq, "fb": fb}


def slots_wanted(path):
    """what the command line wants for a plain file: 1.9 slots per base of its size (FASTQ: of half its size)"""
    size = path.stat().st_size
    bases = size // 2 if path.suffix == ".fastq" else size
    return bases + bases // 10 * 9


# name -> (arguments with {placeholders}, the inputs whose tables are counted, the files written)
CASES = {
    "ctr": (["ctr", "-i", "{fa}", "-o", "{out}", "-k", K, "-a", "--histo"], ["fa"], ["kmers.counts", "kmers.histo"]),
    "cov": (["cov", "-i", "{fa}", "-o", "{out}", "-k", K], ["fa"], ["kmers.vectors", "kmers.counts"]),
    "cov-raw": (["cov", "-i", "{fq}", "-o", "{out}", "-k", K, "--counts", "-p", "tsv"], ["fq"], ["kmers.vectors", "kmers.counts"]),
    "filter": (["filter", "-i", "{fq}", "-o", "{out}/kept.fastq", "-k", K], ["fq"], ["kept.fastq"]),
    "filter-trim": (["filter", "-i", "{fa}", "-o", "{out}/kept.fasta", "-k", K, "--trim"], ["fa"], ["kept.fasta"]),
    "profile": (["profile", "-i", "{fa}", "-o", "{out}", "-k", K, "--positions"], ["fa"], ["profile.stats", "profile.counts"]),
    "correct": (["correct", "-i", "{fq}", "-o", "{out}/fixed.fastq", "-k", K, "--stats", "{out}/correct.stats"], ["fq"],
                ["fixed.fastq", "correct.stats"]),
    "compare": (["compare", "-i", "{fa}", "-a", "{fb}", "-o", "{out}", "-k", K], ["fa", "fb"], ["compare.matrix", "compare.stats"]),
    "setop": (["setop", "-i", "{fq}", "-a", "{fb}", "-o", "{out}", "--op", "union", "-k", K], ["fq", "fb"],
              ["kmers.counts", "setop.stats"]),
}


@pytest.mark.parametrize("name", list(CASES))
def test_same_files_in_one_batch_or_many_resident_or_in_passes(cli_bin, inputs, tmp_path, name):
    args, counted, files = CASES[name]
    # a quarter of the smallest table wanted: at least 4 passes, and far above the floor of 1024 slots
    slots = min(slots_wanted(inputs[c]) for c in counted) // 4 + 1
    assert slots > 6 * 1024
    modes = {"plain": {}, "batches": {"KT_CLI_BATCH_READS": "7"}, "passes": {"KT_CTR_MAX_SLOTS": str(slots)},
             "both": {"KT_CLI_BATCH_READS": "7", "KT_CTR_MAX_SLOTS": str(slots)}}
    got = {}
    for mode, extra in modes.items():
        out = tmp_path / mode
        out.mkdir()
        argv = [str(a).format(out=out, **inputs) for a in args]
        r = subprocess.run([cli_bin, *argv], capture_output=True, timeout=300, cwd=tmp_path,
                           env=dict(os.environ, KT_CLI_TIMING="1", **extra))
        assert r.returncode == 0, (name, mode, r.stderr)
        passes = int(r.stderr.decode().split(" pass(es)")[0].split()[-1])
        print(name, mode, "passes", passes)
        assert passes >= 3 if "KT_CTR_MAX_SLOTS" in extra else passes == 1, (name, mode)
        got[mode] = {f: (out / f).read_bytes() for f in files}
    assert all(len(data) > 50 for data in got["plain"].values()), name  # (nothing is compared over empty files)
    for mode in ("batches", "passes", "both"):
        for f in files:
            if f == "kmers.counts" and not (name == "setop" and mode == "batches"):
                assert sorted(got[mode][f].splitlines()) == sorted(got["plain"][f].splitlines()), (name, mode, f)
            else:
                assert got[mode][f] == got["plain"][f], (name, mode, f)
    assert sorted(os.listdir(tmp_path)) == sorted(modes), name  # nothing beside the output directories (cwd: no stray kmers.counts)
