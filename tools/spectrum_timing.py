"""Times kt_ctr_spectrum and the filtered stage (kt_ctr_export_stage_range) per table form at the benchmark's geometries:
ctr k=31 (25 M x 150 bp reads, a table of 1.9x the k-mers) and ctr k=15 (50 M x 150 bp, the direct-addressed 2^30-slot
table), each as an export target's arrays (what bench.py counts into), as the dense ranges of a bulk build, and as the
probing image (the dense table after one more add).  Reports ms per call (median of --reps) and the fraction of 8 TB/s
over the bytes the form must read: probing 16 B per slot, dense 4 B per entry + 4 B per range, export target 4 B per
entry (the filtered stage also writes 12 B per kept entry; its figure is over the same read bytes).

    python tools/spectrum_timing.py [--k 31 15] [--reads-k31 25000000] [--reads-k15 50000000] [--genome 0] [--reps 20]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from kmertools_amd import device  # noqa: E402

HBM = 8e12


def timed_device(fn, reps):
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    fn()
    torch.cuda.synchronize()
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return float(np.median([a.elapsed_time(b) for a, b in ev]))


def timed_host(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts))


def measure(ctr, form, read_bytes, reps, n_bins=10001):
    hist = torch.zeros(n_bins, dtype=torch.int64, device="cuda")
    tot = torch.zeros(2, dtype=torch.int64, device="cuda")
    ms = timed_device(lambda: ctr.spectrum_into(hist, n_bins, tot), reps)
    ms_stage = timed_host(lambda: ctr.export_stage_range(2, None), max(3, reps // 4))
    h = ctr.spectrum(n_bins)
    return dict(form=form, distinct=ctr.size(), capacity=ctr.capacity(), read_bytes=read_bytes,
                spectrum_ms=round(ms, 4), spectrum_hbm_frac=round(read_bytes / (ms * 1e-3) / HBM, 3),
                stage_2_max_ms=round(ms_stage, 3), stage_hbm_frac=round(read_bytes / (ms_stage * 1e-3) / HBM, 3),
                kept_2_max=int(h[2:].sum()), singletons=int(h[1]),
                peak_bin=int(np.argmax(h[1:]) + 1))


def run_k(ctx, k, n, L, genome, reps):
    bases = torch.empty(n * L, dtype=torch.uint8, device="cuda")
    offsets = torch.empty(n + 1, dtype=torch.int64, device="cuda")
    ctx.synth_reads(0x6b6d6572 + k, n, L, bases, offsets, genome_len=genome)
    kpr = L - k + 1
    max_distinct = min(n * kpr, (4 ** k + 2 ** k) // 2)
    cap = int(1.9 * max_distinct)
    out = []
    # export target (the benchmark's ctr step)
    xk = torch.empty(max_distinct, dtype=torch.int64, device="cuda")
    xc = torch.empty(max_distinct, dtype=torch.int32, device="cuda")
    ctr = device.Counter(ctx, k, cap)
    ctr.export_target(xk, xc, max_distinct)
    ctr.add_reads(bases, offsets, n)
    d = ctr.size()
    out.append(measure(ctr, "export target", d * 4, reps))
    ctr.close()
    del xk, xc
    torch.cuda.empty_cache()
    # dense ranges, then the probing image of the same table
    ctr = device.Counter(ctx, k, cap)
    ctr.add_reads(bases, offsets, n)
    d = ctr.size()
    rs = 1024 * 8 if ctr.capacity() >= 8192 else ctr.capacity()
    n_ranges = ctr.capacity() // rs
    out.append(measure(ctr, "dense", d * 4 + n_ranges * 4, reps))
    ctr.add_pairs_host(np.array([1], np.uint64), np.array([1], np.uint32))
    out.append(measure(ctr, "probing", ctr.capacity() * 16, reps))
    ctr.close()
    del bases, offsets
    torch.cuda.empty_cache()
    for r in out:
        r.update(k=k, reads=n, read_len=L, genome_len=genome)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--k", type=int, nargs="+", default=[31, 15])
    ap.add_argument("--reads-k31", type=int, default=25_000_000)
    ap.add_argument("--reads-k15", type=int, default=50_000_000)
    ap.add_argument("--genome", type=int, nargs="+", default=[0], help="0: uniform random reads; > 0: sampled from a genome")
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    ctx = device.Context(0, stream=torch.cuda.current_stream().cuda_stream)
    rows = []
    for genome in args.genome:
        for k in args.k:
            n = args.reads_k31 if k > 15 else args.reads_k15
            for r in run_k(ctx, k, n, 150, genome, args.reps):
                print(json.dumps(r), flush=True)
                rows.append(r)
    ctx.close()
    return rows


if __name__ == "__main__":
    main()
