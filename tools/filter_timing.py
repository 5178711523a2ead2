"""Times kt_ctr_read_solidity (the read filter's lookup pass) against kt_cov_batch on the same table at bench.py's cov_k15
geometry: 10 M x 150 bp synthetic reads, k = 15, the table of the same reads (the direct-addressed 2^30-slot table), every
array on the device.  Reports ms per call (median of --reps, CUDA events) for:
  cov          kt_cov_batch, bin_size 16 x 16 bins, normalised f64 rows (bench.py's cov step)
  cov_u32      kt_cov_batch_part into u32 rows (the lookup pass alone, without the f64 finalisation)
  solidity     kt_ctr_read_solidity with first_weak
  solidity_nf  kt_ctr_read_solidity with first_weak = NULL (the fraction mode's call)
and each solidity figure over cov's.

    python tools/filter_timing.py [--k 15] [--reads 10000000] [--genome 0] [--reps 20]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from kmertools_amd import device  # noqa: E402


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


def run_k(ctx, k, n, L, genome, reps):
    bases = torch.empty(n * L, dtype=torch.uint8, device="cuda")
    offsets = torch.empty(n + 1, dtype=torch.int64, device="cuda")
    ctx.synth_reads(0x6b6d6572 + 5, n, L, bases, offsets, genome_len=genome)
    kpr = L - k + 1
    max_distinct = min(n * kpr, (4 ** k + 2 ** k) // 2)
    cap = 1 << max(20, (2 * max_distinct - 1).bit_length())  # bench.py's cov table
    ctr = device.Counter(ctx, k, cap)
    ctr.add_reads(bases, offsets, n)
    bins = 16
    out = torch.empty((n, bins), dtype=torch.float64, device="cuda")
    rows = torch.zeros((n, bins), dtype=torch.int32, device="cuda")
    nk = torch.zeros(n, dtype=torch.int32, device="cuda")
    ns = torch.zeros(n, dtype=torch.int32, device="cuda")
    fw = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    r = dict(k=k, reads=n, read_len=L, genome_len=genome, capacity=ctr.capacity(), distinct=ctr.size())
    r["cov_ms"] = timed_device(lambda: ctr.cov(bases, offsets, n, 16, bins, out, norm=True, dtype="f64"), reps)
    r["cov_u32_ms"] = timed_device(lambda: ctr.cov_part(bases, offsets, n, 16, bins, rows), reps)
    r["solidity_ms"] = timed_device(lambda: ctr.read_solidity(bases, offsets, n, 2, 0xFFFFFFFF, nk, ns, fw), reps)
    r["solidity_nf_ms"] = timed_device(lambda: ctr.read_solidity(bases, offsets, n, 2, 0xFFFFFFFF, nk, ns, None), reps)
    for key in ("cov_ms", "cov_u32_ms", "solidity_ms", "solidity_nf_ms"):
        r[key] = round(r[key], 3)
    r["solidity_over_cov"] = round(r["solidity_ms"] / r["cov_ms"], 3)
    r["solidity_nf_over_cov"] = round(r["solidity_nf_ms"] / r["cov_ms"], 3)
    # (a sanity figure: one more call into cleared arrays counts every read's k-mers once)
    nk.zero_()
    ns.zero_()
    ctr.read_solidity(bases, offsets, n, 2, 0xFFFFFFFF, nk, ns, None)
    r["kmers_per_read"] = round(float(nk.to(torch.float64).mean()), 3)
    ctr.close()
    del bases, offsets, out, rows, nk, ns, fw
    torch.cuda.empty_cache()
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--k", type=int, nargs="+", default=[15])
    ap.add_argument("--reads", type=int, default=10_000_000)
    ap.add_argument("--genome", type=int, nargs="+", default=[0], help="0: uniform random reads; > 0: sampled from a genome")
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    ctx = device.Context(0, stream=torch.cuda.current_stream().cuda_stream)
    rows = []
    for genome in args.genome:
        for k in args.k:
            r = run_k(ctx, k, args.reads, 150, genome, args.reps)
            print(json.dumps(r), flush=True)
            rows.append(r)
    ctx.close()
    return rows


if __name__ == "__main__":
    main()
