"""Times the HyperLogLog pre-pass next to what it is meant to be cheap beside.  One process, device-resident synthetic reads
(kt_synth_reads: 10 M x 150 bp sampled from a 50 Mbase genome, 1 % errors - 30x coverage), k = 31, events around every call,
warm-ups first, the median and the spread of the runs:

  card p = 14 / p = 16   kt_card_add_reads into zeroed registers;
  solidity               kt_ctr_read_solidity of the same batch against its own table: the same staging and hashing plus one
                         table probe per k-mer;
  add_reads              kt_ctr_add_reads of the batch into a fitting, cleared table (the clear is not timed).
The pre-pass pays when card < add_reads and card <= solidity, and when p changes only the combine step.

With --e2e also the command line on one FASTQ of about 1 Gbase written from such reads: `ctr` and `ctr --estimate-size` under
KT_CLI_TIMING, their stderr timing lines and wall times - what the extra walk costs on the host side.

    python tools/card_bench.py [--reads 10000000] [--e2e] [--out profiles/card_kernel.txt]
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

K, L, GENOME, SEED = 31, 150, 50_000_000, 0x63617264


def timed(fn, warm, reps, before=None):
    ms = []
    for i in range(warm + reps):
        if before:
            before()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        if i >= warm:
            ms.append(a.elapsed_time(b))
    return dict(ms=round(float(np.median(ms)), 3), min_ms=round(min(ms), 3), max_ms=round(max(ms), 3), runs=reps)


def kernels(ctx, n, emit):
    bases = torch.empty(n * L, dtype=torch.uint8, device="cuda")
    offsets = torch.empty(n + 1, dtype=torch.int64, device="cuda")
    ctx.synth_reads(SEED, n, L, bases, offsets, genome_len=GENOME)
    torch.cuda.synchronize()
    gb = n * L / 1e9
    for p in (14, 16):
        regs = torch.zeros(1 << p, dtype=torch.uint8, device="cuda")
        nk = torch.zeros(1, dtype=torch.int64, device="cuda")
        r = timed(lambda: ctx.card_add(bases, offsets, n, K, regs, p, 0, nk), 3, 10, before=regs.zero_)
        est, zeros = device.card_estimate(regs.cpu().numpy())
        r.update(what="kt_card_add_reads", p=p, gbases_per_s=round(gb / r["ms"] * 1e3, 2), estimate=round(est), zero_registers=zeros)
        emit(r)
    # a fitting table: every erroneous base makes up to k new k-mers
    ctr = device.Counter(ctx, K, 1 << 30)
    r = timed(lambda: ctr.add_reads(bases, offsets, n), 1, 3, before=ctr.clear)
    distinct = ctr.size()
    r.update(what="kt_ctr_add_reads", slots=1 << 30, distinct=distinct, gbases_per_s=round(gb / r["ms"] * 1e3, 2))
    emit(r)
    n_k = torch.zeros(n, dtype=torch.int32, device="cuda")
    n_s = torch.zeros(n, dtype=torch.int32, device="cuda")
    r = timed(lambda: ctr.read_solidity(bases, offsets, n, 2, 0xFFFFFFFF, n_k, n_s), 2, 5)
    r.update(what="kt_ctr_read_solidity", gbases_per_s=round(gb / r["ms"] * 1e3, 2))
    emit(r)
    ctr.close()
    return distinct


def write_fastq(path, n, ctx):
    """n reads of L bases as fixed-width records '@r\\n' bases '\\n+\\n' qualities '\\n', in pieces of a million reads"""
    piece = 1_000_000
    with open(path, "wb") as f:
        for first in range(0, n, piece):
            m = min(piece, n - first)
            bases = torch.empty(m * L, dtype=torch.uint8, device="cuda")
            ctx.synth_reads(SEED, m, L, bases, None, genome_len=GENOME, first_read=first)
            torch.cuda.synchronize()
            rec = np.empty((m, 3 + L + 3 + L + 1), np.uint8)
            rec[:, 0:3] = np.frombuffer(b"@r\n", np.uint8)
            rec[:, 3:3 + L] = bases.cpu().numpy().reshape(m, L)
            rec[:, 3 + L:6 + L] = np.frombuffer(b"\n+\n", np.uint8)
            rec[:, 6 + L:6 + 2 * L] = ord("I")
            rec[:, -1] = ord("\n")
            rec.tofile(f)


def end_to_end(ctx, emit, note):
    n = 1_000_000_000 // L
    cli = ROOT / "kmertools_amd" / "bin" / "kmertools"
    with tempfile.TemporaryDirectory() as d:
        fq = os.path.join(d, "reads.fq")
        write_fastq(fq, n, ctx)
        for flags in ((), ("--estimate-size",)):
            out = os.path.join(d, "out" + "_est" * len(flags))
            t0 = time.perf_counter()
            r = subprocess.run([str(cli), "ctr", "-i", fq, "-o", out, "-k", str(K), "--histo-only", *flags], capture_output=True, text=True,
                               env=dict(os.environ, KT_CLI_TIMING="1"))
            wall = time.perf_counter() - t0
            emit(dict(what="kmertools ctr --histo-only " + " ".join(flags), reads=n, bases=n * L, exit=r.returncode, wall_s=round(wall, 2)))
            for line in r.stderr.splitlines():
                if line.startswith(("[timing]", "[card]", "Error")) and ("setup" in line or "card" in line or "ctr count" in line or "Error" in line):
                    note(line)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=10_000_000)
    ap.add_argument("--e2e", action="store_true")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "card_kernel.txt"))
    args = ap.parse_args()
    lines = ["# tools/card_bench.py, %s, %d reads x %d bp from a %d-base genome, k = %d" % (torch.cuda.get_device_name(0), args.reads, L, GENOME, K)]

    def emit(r):
        print(json.dumps(r), flush=True)
        lines.append(json.dumps(r))

    def note(s):
        print(s, flush=True)
        lines.append(s)

    ctx = device.Context(0, stream=torch.cuda.current_stream().cuda_stream)
    kernels(ctx, args.reads, emit)
    if args.e2e:
        end_to_end(ctx, emit, note)
    ctx.close()
    pathlib.Path(args.out).parent.mkdir(exist_ok=True)
    pathlib.Path(args.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
