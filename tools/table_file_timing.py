"""Times table files: what saving a counted table costs and what loading it saves, on a 30x read set (--reads x 150 bp
synthetic noisy reads of a genome of reads * 150 / 30 bases; the README's set is 10 M reads), k = 21 and k = 31.

  library   the table counted from the reads on the device; then, median of --reps runs each (wall clock around calls that
            synchronise): Counter.save, Counter.from_file and table_file_check.  The kernels are not separable from here:
            `rocprofv3 --kernel-trace --stats -- python tools/table_file_timing.py --reps 1 --no-cli` gives the times
            of sort_*_kernel, tf_offsets_kernel, tf_pack_kernel, tf_keys_kernel and the scan kernels.
            Reported: entries, bytes written, bytes per entry, the size the format's formula gives.
  cli       `ctr` wall time with and without --save-table, `graph --stats-only` and `hetmers --stats-only` counting from
            the reads against --table: after one untimed run, the two forms in turn --reps times, in both orders, the
            median of each (every run kept; KT_CLI_TIMING lines of the last run kept).

    python tools/table_file_timing.py [--reads 10000000] [--reps 5] [--no-cli] [--out profiles/table_file.txt]
"""
import argparse
import json
import os
import pathlib
import subprocess
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from kmertools_amd import device  # noqa: E402

CLI = ROOT / "kmertools_amd" / "bin" / "kmertools"


def median_s(fn, reps):
    fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append(time.perf_counter() - t0)
    return round(float(np.median(t)), 4)


def write_fastq(path, bases, n, L):
    """the device batch as a FASTQ file (for the command line)"""
    host = bases.cpu().numpy().reshape(n, L)
    qual = b"I" * L
    with open(path, "wb") as f:
        for i0 in range(0, n, 1 << 16):
            f.write(b"".join(b"@r%d\n%s\n+\n%s\n" % (i, host[i].tobytes(), qual) for i in range(i0, min(n, i0 + (1 << 16)))))


def timed_cli(*args, env=None):
    t0 = time.perf_counter()
    r = subprocess.run([str(CLI), *map(str, args)], capture_output=True, text=True, env=dict(os.environ, KT_CLI_TIMING="1", **(env or {})))
    dt = time.perf_counter() - t0
    if r.returncode != 0:
        raise SystemExit("%s failed: %s" % (args[0], r.stderr))
    return round(dt, 3), [ln for ln in r.stderr.splitlines() if "table" in ln or "save" in ln]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=10_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-cli", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    n, L = a.reads, 150
    ctx = device.Context(0, stream=torch.cuda.current_stream().cuda_stream)
    bases = torch.empty(n * L, dtype=torch.uint8, device="cuda")
    offsets = torch.empty(n + 1, dtype=torch.int64, device="cuda")
    ctx.synth_reads(0x6b746162, n, L, bases, offsets, noise=True, genome_len=n * L // 30)
    torch.cuda.synchronize()
    results = {"reads": n, "read_len": L}
    with tempfile.TemporaryDirectory() as tmp:
        tmp = pathlib.Path(tmp)
        for k in (21, 31):
            row = {}
            c = device.Counter(ctx, k, max(1 << 20, n * L // 2))  # (the errors' k-mers outnumber the genome's many times)
            c.add_reads(bases, offsets, n)
            row["entries"] = c.size()
            path = tmp / ("k%d.ktab" % k)
            row["save_s"] = median_s(lambda: c.save(path), a.reps)
            row["bytes"] = path.stat().st_size
            row["bytes_per_entry"] = round(row["bytes"] / max(1, row["entries"]), 3)
            info = device.table_file_info(path)
            assert info["entries"] == row["entries"]

            def load():
                device.Counter.from_file(ctx, path).close()
            row["load_s"] = median_s(load, a.reps)
            # ... and its two halves apart: making (and dropping) a table of that size, adding the file to one that exists
            slots = max(1024, info["entries"] + info["entries"] // 10 * 9)
            row["create_s"] = median_s(lambda: device.Counter(ctx, k, slots).close(), a.reps)
            t = device.Counter(ctx, k, slots)

            def add():
                t.clear()
                t.add_file(path)
                t.size()
            row["add_file_s"] = median_s(add, a.reps)
            t.close()
            row["check_s"] = median_s(lambda: device.table_file_check(path), a.reps)
            c.close()
            results["k%d" % k] = row
        if not a.no_cli:
            fq = tmp / "reads.fq"
            write_fastq(fq, bases, n, L)
            for k in (21, 31):
                row = results["k%d" % k]
                tab = tmp / ("cli_k%d.ktab" % k)
                # one untimed run first (the reads enter the page cache), then the two forms in turn, --reps times each, in
                # both orders: the median of every form
                timed_cli("ctr", "-i", fq, "-o", tmp / "c0", "-k", k, "--histo-only")
                plain, saved = [], []
                for rep in range(a.reps):
                    for form in ((0, 1) if rep % 2 == 0 else (1, 0)):
                        if form == 0:
                            plain.append(timed_cli("ctr", "-i", fq, "-o", tmp / "c0", "-k", k, "--histo-only")[0])
                        else:
                            dt, row["ctr_lines"] = timed_cli("ctr", "-i", fq, "-o", tmp / "c1", "-k", k, "--histo-only", "--save-table", tab)
                            saved.append(dt)
                row["ctr_s"], row["ctr_save_table_s"] = round(float(np.median(plain)), 3), round(float(np.median(saved)), 3)
                row["ctr_all"], row["ctr_save_table_all"] = plain, saved
                for cmd in ("graph", "hetmers"):
                    from_reads, from_table = [], []
                    for rep in range(a.reps):
                        for form in ((0, 1) if rep % 2 == 0 else (1, 0)):
                            if form == 0:
                                from_reads.append(timed_cli(cmd, "-i", fq, "-o", tmp / (cmd + "0"), "-k", k, "--stats-only")[0])
                            else:
                                dt, row[cmd + "_lines"] = timed_cli(cmd, "--table", tab, "-o", tmp / (cmd + "1"), "-k", k, "--stats-only")
                                from_table.append(dt)
                    row[cmd + "_reads_s"], row[cmd + "_table_s"] = round(float(np.median(from_reads)), 3), round(float(np.median(from_table)), 3)
                    row[cmd + "_reads_all"], row[cmd + "_table_all"] = from_reads, from_table
    text = json.dumps(results, indent=1)
    print(text)
    if a.out:
        pathlib.Path(a.out).write_text(text + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
