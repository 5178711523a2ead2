"""Times kt_ctr_compare per form of table A against a probing table B, next to the unfused equivalent: kt_ctr_lookup of A's
exported keys (already on the device) in B plus kt_ctr_spectrum(B) - what the fused call replaces, and which still needs
A's keys as an array (the time of that export, kt_ctr_export to device arrays, is reported next to it).  Pairs: k = 31
uniform random reads (10 M x 150 bp each side: two tables of the ctr_k31 benchmark's 25 M reads would not fit the HBM
together), k = 31 reads sampled from one 20 Mbp genome (disjoint read ids, 10 M each),
and k = 15 at the benchmark's direct geometry (50 M x 150 bp each side, 2^30-slot tables).  A is each of: an export
target's arrays, the dense ranges of the bulk build, the probing image (after one more add).  hipEvent medians of --reps,
one JSON line per (pair, form).

    python tools/compare_timing.py [--pairs k31 k31_genome k15] [--reads-k31 10000000] [--reads-k15 50000000] [--reps 20]
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


def reads(ctx, seed, n, L, genome, first):
    bases = torch.empty(n * L, dtype=torch.uint8, device="cuda")
    offsets = torch.empty(n + 1, dtype=torch.int64, device="cuda")
    ctx.synth_reads(seed, n, L, bases, offsets, noise=genome > 0, genome_len=genome, first_read=first)
    return bases, offsets


def measure(a, b, form, reps, n_rows=1001, n_cols=101):
    m = torch.zeros((n_rows, n_cols), dtype=torch.int64, device="cuda")
    t = torch.zeros(6, dtype=torch.int64, device="cuda")
    ms = timed_device(lambda: a.compare_into(b, m, n_rows, n_cols, t), reps)
    # the unfused pair: A's keys exported (timed on its own), then lookup in B + B's spectrum
    d = a.size()
    xk = torch.empty(d, dtype=torch.int64, device="cuda")
    xc = torch.empty(d, dtype=torch.int32, device="cuda")
    ms_export = timed_device(lambda: a.export(xk, xc, d), max(3, reps // 2))
    hits = torch.empty(d, dtype=torch.int32, device="cuda")
    hist = torch.zeros(n_cols, dtype=torch.int64, device="cuda")
    tot = torch.zeros(2, dtype=torch.int64, device="cuda")

    def unfused():
        b.lookup(xk, d, hits)
        b.spectrum_into(hist, n_cols, tot)

    ms_lookup = timed_device(lambda: b.lookup(xk, d, hits), reps)
    ms_unfused = timed_device(unfused, reps)
    mat, tt = a.compare(b, n_rows, n_cols, totals=True)
    del xk, xc, hits
    torch.cuda.empty_cache()
    return dict(form=form, distinct_a=d, distinct_b=b.size(), capacity_a=a.capacity(), capacity_b=b.capacity(),
                shared=tt["shared"], compare_ms=round(ms, 3), lookup_ms=round(ms_lookup, 3),
                lookup_plus_spectrum_ms=round(ms_unfused, 3), fused_over_unfused=round(ms / ms_unfused, 3),
                export_ms=round(ms_export, 3), fused_over_export_lookup_spectrum=round(ms / (ms_export + ms_unfused), 3),
                peak_cell=[int(v) for v in np.unravel_index(np.argmax(mat[1:, 1:]), mat[1:, 1:].shape)])


def run_pair(ctx, k, n, genome, reps):
    L = 150
    seed = 0x6b6d6572 + k
    kpr = L - k + 1
    max_distinct = min(n * kpr, (4 ** k + 2 ** k) // 2)
    cap = int(1.9 * max_distinct)
    bb, bo = reads(ctx, seed, n, L, genome, n)
    b = device.Counter(ctx, k, cap)
    b.add_reads(bb, bo, n)
    del bb, bo
    torch.cuda.empty_cache()
    ab, ao = reads(ctx, seed, n, L, genome, 0)
    out = []
    # A as an export target's arrays (the benchmark's ctr step)
    xk = torch.empty(max_distinct, dtype=torch.int64, device="cuda")
    xc = torch.empty(max_distinct, dtype=torch.int32, device="cuda")
    a = device.Counter(ctx, k, cap)
    a.export_target(xk, xc, max_distinct)
    a.add_reads(ab, ao, n)
    out.append(measure(a, b, "export target", reps))
    a.close()
    del xk, xc
    torch.cuda.empty_cache()
    # A's dense ranges, then its probing image
    a = device.Counter(ctx, k, cap)
    a.add_reads(ab, ao, n)
    del ab, ao
    torch.cuda.empty_cache()
    out.append(measure(a, b, "dense", reps))
    a.add_pairs_host(np.array([1], np.uint64), np.array([1], np.uint32))
    out.append(measure(a, b, "probing", reps))
    a.close()
    b.close()
    torch.cuda.empty_cache()
    for r in out:
        r.update(k=k, reads_each=n, read_len=L, genome_len=genome)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", nargs="+", default=["k31", "k31_genome", "k15"])
    ap.add_argument("--reads-k31", type=int, default=10_000_000)
    ap.add_argument("--reads-k15", type=int, default=50_000_000)
    ap.add_argument("--genome", type=int, default=20_000_000)
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    ctx = device.Context(0, stream=torch.cuda.current_stream().cuda_stream)
    rows = []
    for p in args.pairs:
        k = 15 if p == "k15" else 31
        n = args.reads_k15 if k == 15 else args.reads_k31
        for r in run_pair(ctx, k, n, args.genome if p.endswith("genome") else 0, args.reps):
            r["pair"] = p
            print(json.dumps(r), flush=True)
            rows.append(r)
    ctx.close()
    return rows


if __name__ == "__main__":
    main()
