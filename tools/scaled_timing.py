"""Times the scaled-sketch calls beside their neighbours (profiles/scaled_kernel.txt is this script's output with notes):

  batch   kt_scaled_batch at --scaled 1000 beside kt_card_add_reads p = 14 (the same walk and hash: the floor) and
          kt_sketch_batch at s = 1000 (what there was before) on one batch of --reads x 150 bp synthetic reads (bench.py's
          seed), k = 31;
  batch1  kt_scaled_batch at scaled = 1 on --reads1 x 150 bp: every window is kept, the call is its sorts;
  table   kt_ctr_scaled at --scaled beside kt_ctr_spectrum on the table counted from the first batch (the same walk);
  pairs   kt_scaled_pairs over --rows x --rows rows of --row-hashes hashes beside kt_sketch_pairs at s = 4096 over as many rows.

One process, everything in device memory; the calls of a comparison alternate after a warm-up of each, a time is the span
between two device events around the call (the scaled calls wait for the stream themselves to learn their sizes, so the span
is the call), and the record is the median of --reps with minimum and maximum.  --only runs one case (for a profiler).

    python tools/scaled_timing.py [--reads 10000000] [--out profiles/scaled_kernel.txt]
"""
import argparse
import json
import pathlib
import subprocess
import sys

import numpy as np
import torch

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from kmertools_amd import device  # noqa: E402

SEED = 0x6b6d6572  # bench.py's


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def alternating(fns, reps):
    for f in fns:
        f()
    times = [[] for _ in fns]
    for _ in range(reps):
        for t, f in zip(times, fns):
            t.append(timed(f))
    return [dict(median_ms=round(float(np.median(t)), 3), min_ms=round(min(t), 3), max_ms=round(max(t), 3)) for t in times]


def empty(n, dtype):
    return torch.empty(max(int(n), 1), dtype=dtype, device="cuda")


def reads(ctx, n, L, genome):
    bases = torch.empty(n * L, dtype=torch.uint8, device="cuda")
    offsets = torch.empty(n + 1, dtype=torch.int64, device="cuda")
    ctx.synth_reads(SEED, n, L, bases, offsets, genome_len=genome)
    return bases, offsets


def scaled_call(ctx, bases, offsets, n, k, scaled):
    ro, nk = empty(n + 1, torch.int64), empty(n, torch.int32)
    n_out = ctx.scaled_sketch(bases, offsets, n, k, scaled, None, None, 0, ro, nk)
    h, a = empty(n_out, torch.int64), empty(n_out, torch.int32)
    return n_out, lambda: ctx.scaled_sketch(bases, offsets, n, k, scaled, h, a, max(n_out, 1), ro, nk)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=10_000_000)
    ap.add_argument("--reads1", type=int, default=1_000_000)
    ap.add_argument("--genome", type=int, default=50_000_000)
    ap.add_argument("--scaled", type=int, default=1000)
    ap.add_argument("--rows", type=int, default=1000)
    ap.add_argument("--row-hashes", type=int, default=5000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only", choices=["batch", "batch1", "table", "pairs"])
    ap.add_argument("--out", default=str(ROOT / "profiles" / "scaled_kernel.txt"))
    args = ap.parse_args()
    k, L = 31, 150
    try:
        commit = subprocess.run(["git", "-C", str(ROOT), "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip()
    except OSError:
        commit = ""
    ctx = device.Context(0, stream=torch.cuda.current_stream().cuda_stream)
    want = lambda case: args.only in (None, case)  # noqa: E731
    rows = []

    def record(r):
        print(json.dumps(r), flush=True)
        rows.append(r)

    n = args.reads
    if want("batch") or want("table"):
        bases, offsets = reads(ctx, n, L, args.genome)
    if want("batch"):
        r = dict(case="batch", reads=n, length=L, genome=args.genome, k=k, scaled=args.scaled)
        r["hashes_out"], scaled_fn = scaled_call(ctx, bases, offsets, n, k, args.scaled)
        regs, nkm = torch.zeros(1 << 14, dtype=torch.uint8, device="cuda"), torch.zeros(1, dtype=torch.int64, device="cuda")
        fns = [scaled_fn, lambda: ctx.card_add(bases, offsets, n, k, regs, 14, 0, nkm)]
        names = ["kt_scaled_batch", "kt_card_add_reads"]
        try:  # (n x 1000 x 8 bytes of rows: 80 GB at 10 M reads)
            s = 1000
            sh, sz, snk = empty(n * s, torch.int64), empty(n, torch.int32), empty(n, torch.int32)
            fns.append(lambda: ctx.sketch(bases, offsets, n, k, s, sh, sz, snk))
            names.append("kt_sketch_batch")
        except RuntimeError as e:
            r["kt_sketch_batch"] = "not run: %s" % str(e).splitlines()[0]
        for name, t in zip(names, alternating(fns, args.reps)):
            r[name] = t
        r["scaled_over_card"] = round(r["kt_scaled_batch"]["median_ms"] / r["kt_card_add_reads"]["median_ms"], 3)
        if "median_ms" in r.get("kt_sketch_batch", ""):
            r["scaled_over_sketch"] = round(r["kt_scaled_batch"]["median_ms"] / r["kt_sketch_batch"]["median_ms"], 3)
        record(r)
        sh = sz = snk = None
        torch.cuda.empty_cache()
    if want("table"):
        table = device.Counter(ctx, k, int(1.9 * n * (L - k + 1)) + (1 << 20))
        table.add_reads(bases, offsets, n)
        r = dict(case="table", reads=n, k=k, scaled=args.scaled, entries=table.size())
        hist, tot = torch.zeros(10001, dtype=torch.int64, device="cuda"), torch.zeros(2, dtype=torch.int64, device="cuda")
        n_out = table.scaled_sketch(args.scaled, mem=device.KT_MEM_DEVICE)
        th, ta, tt = empty(n_out, torch.int64), empty(n_out, torch.int32), empty(2, torch.int64)
        r["hashes_out"] = n_out
        r["kt_ctr_scaled"], r["kt_ctr_spectrum"] = alternating(
            [lambda: table.scaled_sketch(args.scaled, 1, None, 0, th, ta, max(n_out, 1), tt, device.KT_MEM_DEVICE),
             lambda: table.spectrum_into(hist, 10001, tot)], args.reps)
        r["scaled_over_spectrum"] = round(r["kt_ctr_scaled"]["median_ms"] / r["kt_ctr_spectrum"]["median_ms"], 3)
        record(r)
        table.close()
    bases = offsets = None
    torch.cuda.empty_cache()
    if want("batch1"):
        n1 = args.reads1
        b1, o1 = reads(ctx, n1, L, args.genome)
        r = dict(case="batch1", reads=n1, length=L, k=k, scaled=1)
        r["hashes_out"], fn = scaled_call(ctx, b1, o1, n1, k, 1)
        r["kt_scaled_batch"], = alternating([fn], args.reps)
        record(r)
        b1 = o1 = None
        torch.cuda.empty_cache()
    if want("pairs"):
        m, w, s = args.rows, args.row_hashes, 4096
        g = torch.Generator(device="cuda").manual_seed(SEED)
        pool = torch.randint(0, 1 << 62, (m, w), dtype=torch.int64, device="cuda", generator=g).sort(dim=1).values.contiguous()
        off = torch.arange(m + 1, dtype=torch.int64, device="cuda") * w
        shared = empty(m * m, torch.int32)
        fixed = pool[:, :s].contiguous()
        sizes = torch.full((m,), s, dtype=torch.int32, device="cuda")
        sh2, dn2 = empty(m * m, torch.int32), empty(m * m, torch.int32)
        r = dict(case="pairs", rows=m, row_hashes=w, sketch_s=s)
        r["kt_scaled_pairs"], r["kt_sketch_pairs"] = alternating(
            [lambda: ctx.scaled_pairs(pool, off, m, pool, off, m, shared),
             lambda: ctx.sketch_pairs(fixed, sizes, m, fixed, sizes, m, s, sh2, dn2)], args.reps)
        r["scaled_over_sketch_pairs"] = round(r["kt_scaled_pairs"]["median_ms"] / r["kt_sketch_pairs"]["median_ms"], 3)
        record(r)
    ctx.close()
    head = "# tools/scaled_timing.py, commit %s (+ working tree), %s, medians of %d between events, the calls of a comparison alternating" % (
        commit or "unknown", torch.cuda.get_device_name(0), args.reps)
    pathlib.Path(args.out).parent.mkdir(exist_ok=True)
    pathlib.Path(args.out).write_text(head + "\n" + "".join(json.dumps(r) + "\n" for r in rows))


if __name__ == "__main__":
    main()
