"""What the command line says and leaves behind when an output file cannot be written: the file is /dev/full (through a
symlink of its name in the output directory, or given as the output path), or the output directory cannot be made.  Two
inputs: 30 random reads of 80 bp, whose small files fail when they are closed, and 3000, whose files fail at a write.
The expected values are what the command line printed and left before its files went through one writer (OutFile):
exit status, the `Error:` lines, the other files of the command that exist afterwards.  Commands whose files go through
the ordered writer (comp oligo, min) report no write error and exit 0: that is recorded here as it is."""
import os
import pathlib
import subprocess

import numpy as np
import pytest

ROOT = pathlib.Path(__file__).resolve().parent.parent
CLI = ROOT / "kmertools_amd" / "bin" / "kmertools"
K = "11"
N_READS = {"small": 30, "large": 3000}

# case -> (the file that is /dev/full: a name in the output directory, PATH for an output path, MISSING for an output
# directory below one that does not exist; the command line, {fa} the input, {out} the output directory or path)
PATH, MISSING = "<path>", "<missing>"
CASES = {
    "graph.nodes": ("graph.nodes", ["graph", "-i", "{fa}", "-o", "{out}", "-k", K]),
    "hetmers.pairs": ("hetmers.pairs", ["hetmers", "-i", "{fa}", "-o", "{out}", "-k", K]),
    "hetmers.cov": ("hetmers.cov", ["hetmers", "-i", "{fa}", "-o", "{out}", "-k", K]),
    "unitigs.fa": ("unitigs.fa", ["unitigs", "-i", "{fa}", "-o", "{out}", "-k", K]),
    "unitigs.gfa": ("unitigs.gfa", ["unitigs", "-i", "{fa}", "-o", "{out}", "-k", K, "--gfa"]),
    "thread.gaf": ("thread.gaf", ["thread", "-i", "{fa}", "-a", "{fa}", "-o", "{out}", "-k", K]),
    "thread.reads": ("thread.reads", ["thread", "-i", "{fa}", "-a", "{fa}", "-o", "{out}", "-k", K, "--components"]),
    "profile.stats": ("profile.stats", ["profile", "-i", "{fa}", "-o", "{out}", "-k", K]),
    "profile.counts": ("profile.counts", ["profile", "-i", "{fa}", "-o", "{out}", "-k", K, "--positions"]),
    "setop kmers.counts": ("kmers.counts", ["setop", "-i", "{fa}", "-a", "{fa}", "-o", "{out}", "-k", K, "--op", "union"]),
    "sketch.tsv": ("sketch.tsv", ["sketch", "-i", "{fa}", "-o", "{out}", "-k", K]),
    "filter": (PATH, ["filter", "-i", "{fa}", "-o", "{out}", "-k", K, "--min-count", "1"]),  # (every read is kept)
    "correct": (PATH, ["correct", "-i", "{fa}", "-o", "{out}", "-k", K]),
    "min": (PATH, ["min", "-i", "{fa}", "-o", "{out}"]),
    "oligo": (PATH, ["comp", "oligo", "-i", "{fa}", "-o", "{out}"]),
    "unitigs, no directory": (MISSING, ["unitigs", "-i", "{fa}", "-o", "{out}", "-k", K]),
    "graph, no directory": (MISSING, ["graph", "-i", "{fa}", "-o", "{out}", "-k", K]),
}

# case -> size -> (exit status, the Error: lines of stderr, the command's other files in the output directory)
_FULL = (101, ["Error: Unable to write to file: /dev/full"], [])
_SILENT = (0, [], [])
_NO_DIR = (101, ["Error: unable to create directory: {tmp}/missing/out"], [])


def _file(name, left=()):
    return (101, ["Error: Unable to write to file: {tmp}/out/" + name], list(left))


def _both(x):
    return {"small": x, "large": x}


_PROFILE_DIR = ["Error: Unable to write to directory: {tmp}/out"]
EXPECTED = {
    "graph.nodes": _both(_file("graph.nodes")),
    "hetmers.pairs": _both(_file("hetmers.pairs", ["hetmers.cov"])),
    "hetmers.cov": _both(_file("hetmers.cov", ["hetmers.pairs"])),
    "unitigs.fa": _both(_file("unitigs.fa")),
    "unitigs.gfa": _both(_file("unitigs.gfa", ["unitigs.fa"])),
    "thread.gaf": _both(_file("thread.gaf", ["unitigs.fa", "unitigs.gfa"])),
    "thread.reads": _both(_file("thread.reads", ["thread.gaf", "unitigs.components", "unitigs.fa", "unitigs.gfa"])),
    # (a batch's lines that fail at the write name the directory, the header line that fails at close names the file)
    "profile.stats": {"small": _file("profile.stats"), "large": (101, _PROFILE_DIR, [])},
    "profile.counts": _both((101, _PROFILE_DIR, ["profile.stats"])),
    "setop kmers.counts": _both((101, ["Error: Unable to write the table's lines"], [])),
    "sketch.tsv": _both(_file("sketch.tsv")),
    "filter": _both(_FULL),
    "correct": _both(_FULL),
    "min": _both(_SILENT),
    "oligo": _both(_SILENT),
    "unitigs, no directory": _both(_NO_DIR),
    "graph, no directory": _both(_NO_DIR),
}


def write_reads(path, n):
    rng = np.random.default_rng(20 + n)
    seqs = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, size=(n, 80))]
    with open(path, "wb") as f:
        for i in range(n):
            f.write(b">r%d\n%s\n" % (i, seqs[i].tobytes()))


def run_case(cli, case, fa, tmp):
    """-> (exit status, Error: lines with the temporary directory as {tmp}, sorted names of the other files written)"""
    target, args = CASES[case]
    out = tmp / "out"
    if target == PATH:
        out = pathlib.Path("/dev/full")
    elif target == MISSING:
        out = tmp / "missing" / "out"
    else:
        out.mkdir()
        os.symlink("/dev/full", out / target)
    r = subprocess.run([str(cli)] + [a.format(fa=fa, out=out) for a in args], capture_output=True, timeout=300)
    errors = [ln.replace(str(tmp), "{tmp}") for ln in r.stderr.decode("utf-8", "replace").splitlines() if ln.startswith("Error:")]
    left = sorted(p.name for p in (tmp / "out").iterdir() if p.name != target) if (tmp / "out").is_dir() else []
    return r.returncode, errors, left


@pytest.fixture(scope="module")
def reads(tmp_path_factory):
    d = tmp_path_factory.mktemp("reads")
    for size, n in N_READS.items():
        write_reads(d / (size + ".fa"), n)
    return {size: d / (size + ".fa") for size in N_READS}


@pytest.mark.gpu
@pytest.mark.parametrize("size", list(N_READS))
@pytest.mark.parametrize("case", list(CASES))
def test_output_file_cannot_be_written(case, size, reads, tmp_path):
    got = run_case(CLI, case, reads[size], tmp_path)
    print(case, size, got)
    assert got == EXPECTED[case][size]
