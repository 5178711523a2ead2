"""`kmertools filter` on the CPU: listed in the main --help, its own --help lists every flag, and every usage error exits 2
(an unknown input extension 101, as in `cov`) before any device is opened or the output is made.  Also the reader's
whole-record mode (keep_records, which the filter writes back from): headers and FASTQ qualities in the serial, the
parallel and the gzip reader, and batches without it exactly as before."""
import gzip
import os
import pathlib
import subprocess

import numpy as np
import pytest

ROOT = pathlib.Path(__file__).resolve().parent.parent
CLI = ROOT / "kmertools_amd" / "bin" / "kmertools"
GOLDEN = ROOT / "tests" / "golden"


@pytest.fixture(scope="module")
def cli():
    if not CLI.exists():
        subprocess.check_call(["make", "-C", str(ROOT / "kmertools_amd" / "csrc"), "-j4"], stdout=subprocess.DEVNULL)
    return str(CLI)


def run(cli, *args, env=None):
    return subprocess.run([cli, *map(str, args)], capture_output=True, text=True, timeout=300, env=env)


def test_main_help_lists_filter(cli):
    r = run(cli, "--help")
    assert r.returncode == 0
    assert "  filter  " in r.stdout
    for cmd in ("comp", "cov", "min", "ctr", "help"):
        assert "  %s " % cmd in r.stdout, cmd


def test_filter_help_lists_every_flag(cli):
    r = run(cli, "filter", "--help")
    assert r.returncode == 0
    for flag in ("-i, --input <INPUT>", "-o, --output <OUTPUT>", "-k, --k-size <K_SIZE>", "-a, --alt-input <ALT_INPUT>",
                 "--min-count <N>", "--max-count <N>", "--min-solid <F>", "--trim", "-m, --memory <MEMORY>",
                 "-t, --threads <THREADS>", "--device <DEVICE>", "-h, --help"):
        assert flag in r.stdout, flag


@pytest.mark.parametrize("extra, what", [
    (("--trim", "--min-solid", "0.5"), "--trim"),
    (("--min-solid", "0.5", "--trim"), "--trim"),
    (("--min-count", "0"), "--min-count"),
    (("--min-count", "5", "--max-count", "4"), "--min-count"),
    (("--min-count", "-1"), "--min-count"),
    (("--max-count", "4294967296"), "--max-count"),
    (("--max-count", "0"), "--max-count"),
    (("--min-solid", "1.5"), "--min-solid"),
    (("--min-solid", "-0.1"), "--min-solid"),
    (("--min-solid", "nan"), "--min-solid"),
    (("--min-solid", "half"), "--min-solid"),
    (("--min-solid",), "--min-solid"),
    (("--k-size", "9"), "--k-size"),
    (("--k-size", "32"), "--k-size"),
    (("--memory", "5"), "--memory"),
    (("--bogus",), "--bogus"),
])
def test_filter_usage_errors(cli, tmp_path, extra, what):
    fa = tmp_path / "r.fa"
    fa.write_text(">a\nACGTACGTACGTACGTACGTACGTACGT\n")
    out = tmp_path / "kept.fa"
    args = ["filter", "-i", fa, "-o", out] + ([] if "--k-size" in extra else ["-k", "15"]) + list(extra)
    r = run(cli, *args)
    assert r.returncode == 2, r.stderr
    assert r.stderr.startswith("error: ") and what in r.stderr and "For more information, try '--help'." in r.stderr
    assert not out.exists()


def test_filter_needs_k(cli, tmp_path):
    fa = tmp_path / "r.fa"
    fa.write_text(">a\nACGTACGTACGTACGTACGTACGTACGT\n")
    out = tmp_path / "kept.fa"
    r = run(cli, "filter", "-i", fa, "-o", out)
    assert r.returncode == 2 and "--k-size" in r.stderr
    assert not out.exists()


@pytest.mark.parametrize("which", ["input", "alt-input", "stdin"])
def test_filter_unknown_extension(cli, tmp_path, which):
    fa = tmp_path / "r.fa"
    fa.write_text(">a\nACGTACGTACGTACGTACGTACGTACGT\n")
    bad = tmp_path / "r.txt"
    bad.write_text(">a\nACGTACGTACGTACGTACGTACGTACGT\n")
    out = tmp_path / "kept.fa"
    if which == "input":
        args = ("-i", bad)
    elif which == "alt-input":
        args = ("-i", fa, "-a", bad)
    else:
        args = ("-i", "-")
    r = run(cli, "filter", *args, "-o", out, "-k", "15")
    assert r.returncode == 101, r.stderr
    assert "unsupported input extension" in r.stderr
    assert not out.exists()


# ---- the reader's whole records ---------------------------------------------------------------------------------------

def records_of(data):
    """(id, header, sequence, quality or None) of every record: the header line without '>' / '@' and its trailing
    whitespace, sequence (and quality) lines joined with their trailing whitespace removed"""
    ws = b" \t\r\n\v\f"
    lines = data.split(b"\n")
    if lines and lines[-1] == b"":
        lines.pop()
    out = []
    i = 0
    if data[:1] == b">":
        while i < len(lines):
            h = lines[i].rstrip(ws)
            i += 1
            if not h:
                continue
            seq = []
            while i < len(lines) and not lines[i].startswith(b">"):
                seq.append(lines[i].rstrip(ws))
                i += 1
            tok = h[1:].split()
            out.append((tok[0] if tok else b"", h[1:], b"".join(seq), None))
    else:
        while i < len(lines):
            h = lines[i].rstrip(ws)
            if not h:
                i += 1
                continue
            tok = h[1:].split()
            out.append((tok[0] if tok else b"", h[1:], lines[i + 1].rstrip(ws), lines[i + 3].rstrip(ws)))
            i += 4
    return out


def debug_read(cli, path, records, threads=None):
    env = dict(os.environ)
    if records:
        env["KT_DEBUG_READ_RECORDS"] = "1"
    if threads:
        env["KT_READER_THREADS"] = str(threads)
    r = subprocess.run([cli, "debug-read", str(path)], capture_output=True, timeout=600, env=env)
    assert r.returncode == 0, r.stderr
    return [ln for ln in r.stdout.split(b"\n") if ln and not ln.startswith(b"#")]


def want_lines(recs, records):
    out = []
    for i, (rid, hdr, seq, qual) in enumerate(recs):
        f = [str(i).encode(), rid] + ([hdr] if records else []) + [seq]
        if records and qual is not None:
            f.append(qual)
        out.append(b"\t".join(f))
    return out


def noisy_fastq(seed, n, max_len=300):
    rng = np.random.default_rng(seed)
    alpha = np.frombuffer(b"ACGTNacgt", np.uint8)
    quals = np.frombuffer(b"!#+5?I", np.uint8)
    recs = []
    for i in range(n):
        L = int(rng.integers(0, max_len))
        s = alpha[rng.integers(0, len(alpha), size=L)].tobytes()
        q = quals[rng.integers(0, len(quals), size=L)].tobytes()
        recs.append(b"@r%d  lane:%d sample x=%d\tend\n%s\n+\n%s\n" % (i, i % 7, i * 3, s, q))
    return b"".join(recs)


@pytest.mark.parametrize("name", ["reads.fq", "reads.fa", "reads.fq.gz", "noisy.fastq", "noisy.fq.gz", "wrapped.fa"])
def test_reader_keep_records(cli, tmp_path, name):
    if name.startswith("reads"):
        path = GOLDEN / name
        data = gzip.decompress(path.read_bytes()) if name.endswith(".gz") else path.read_bytes()
    elif name == "wrapped.fa":
        data = b">c1 first contig  \nACGTN\nacgt  \n\n>c2\n>c3 x\r\nAC\nGT\n"
        path = tmp_path / name
        path.write_bytes(data)
    else:
        data = noisy_fastq(3, 400)
        path = tmp_path / name
        path.write_bytes(gzip.compress(data) if name.endswith(".gz") else data)
    recs = records_of(data)
    assert recs
    # without keep_records: exactly the batches of before (id and sequence, no headers or qualities)
    assert debug_read(cli, path, False) == want_lines(recs, False)
    assert debug_read(cli, path, True) == want_lines(recs, True)


def test_reader_keep_records_parallel(cli, tmp_path):
    """a plain file of 32 MB or more is parsed in pieces by several threads: headers and qualities come along"""
    block = noisy_fastq(4, 2000, max_len=400)
    reps = (33 << 20) // len(block) + 1
    data = block * reps
    path = tmp_path / "big.fastq"
    path.write_bytes(data)
    recs = records_of(block) * reps
    want = want_lines(recs, True)
    got = debug_read(cli, path, True, threads=4)
    assert len(got) == len(want)
    assert got == want
    assert debug_read(cli, path, False, threads=4) == want_lines(recs, False)
