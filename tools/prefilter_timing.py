"""Times the two passes of the pre-filter beside the calls they stand next to, and records what the filter keeps out of the
table (profiles/prefilter_kernel.txt is this script's output with notes).

The read set is bench.py's: --reads x 150 bp synthetic reads with errors sampled from a random genome of --genome bases
(10 M reads of 50 Mbase: 30x), at k = 31 and k = 21.  One process, everything in device memory; the two calls of a pair
alternate after a warm-up of each, a time is the span between two device events around the call, and the record is the
median of --reps with minimum and maximum.  The pairs:
  pass 1 (kt_prefilter_add_reads into a cleared filter)  beside kt_card_add_reads (p = 14)
  pass 1                                                 beside kt_ctr_add_reads by probing (KT_BULK=0) into a cleared table
  pass 2 (kt_ctr_add_reads_filtered, cleared table)      beside kt_ctr_add_reads by probing, and beside the default bulk build
(a cleared table is wiped by the first probing insert: the wipe of each table's slots is inside its time - the filtered
table is the smaller one, as it would be in use).  Sizes: the table's keys with and without the filter, the k-mers seen
once that got in as a share of all of them at --bits 8, 16 and 32 per distinct k-mer, the shares of the bits set.

    python tools/prefilter_timing.py [--reads 10000000] [--genome 50000000] [--out profiles/prefilter_kernel.txt]
"""
import argparse
import json
import os
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


def alternating(f, g, reps):
    f(), g()
    tf, tg = [], []
    for _ in range(reps):
        tf.append(timed(f))
        tg.append(timed(g))
    return [dict(median_ms=round(float(np.median(t)), 3), min_ms=round(min(t), 3), max_ms=round(max(t), 3)) for t in (tf, tg)]


def log2_words(kmers, bits):
    """the command line's sizing: bits per k-mer, rounded up to a power of two of 64-bit words, at least 2^10"""
    a = 10
    while (64 << a) < kmers * bits:
        a += 1
    return a


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=10_000_000)
    ap.add_argument("--genome", type=int, default=50_000_000)
    ap.add_argument("--k", type=int, action="append")
    ap.add_argument("--bits", type=int, action="append")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "prefilter_kernel.txt"))
    args = ap.parse_args()
    L, n = 150, args.reads
    total = n * L
    try:
        commit = subprocess.run(["git", "-C", str(ROOT), "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip()
    except OSError:
        commit = ""
    ctx = device.Context(0, stream=torch.cuda.current_stream().cuda_stream)
    bases = torch.empty(total, dtype=torch.uint8, device="cuda")
    offsets = torch.empty(n + 1, dtype=torch.int64, device="cuda")
    ctx.synth_reads(SEED, n, L, bases, offsets, noise=True, genome_len=args.genome)
    rows = []
    for k in args.k or [31, 21]:
        windows = n * (L - k + 1)
        r = dict(reads=n, length=L, genome=args.genome, k=k)   # (windows: below - a read with an unknown base has fewer)
        os.environ["KT_BULK"] = "1"
        full = device.Counter(ctx, k, int(1.9 * windows) + (1 << 20))   # (room for every window to be distinct)
        full.add_reads(bases, offsets, n)
        hist, (distinct, occurrences) = full.spectrum(3, totals=True)
        once_true = int(hist[1])
        r.update(windows=occurrences, table_keys_unfiltered=distinct, seen_once=once_true, seen_twice_or_more=distinct - once_true)
        registers = torch.zeros(1 << 14, dtype=torch.uint8, device="cuda")

        def card():
            ctx.card_add(bases, offsets, n, k, registers, 14)

        def probing():
            os.environ["KT_BULK"] = "0"
            full.clear()
            full.add_reads(bases, offsets, n)

        def bulk():
            os.environ["KT_BULK"] = "1"
            full.clear()
            full.add_reads(bases, offsets, n)

        for bits in args.bits or [16, 8, 32]:
            a = log2_words(distinct, bits)
            b = max(10, a - 2)
            f = device.Prefilter(ctx, k, a, b, 0)

            def pass1():
                f.clear()
                f.add_reads(bases, offsets, n)

            pass1()
            st = f.stats()
            small = device.Counter(ctx, k, int(1.9 * (st["promotions"] + (st["twice_bits_set"] / (64.0 * (1 << b))) ** 4 * distinct)) + 1024)

            def pass2():
                small.clear()
                small.add_reads_filtered(f, bases, offsets, n)

            pass2()
            h2, (keys2, _) = small.spectrum(3, totals=True)
            assert st["windows"] == occurrences
            s = dict(bits_per_kmer=bits, log2_once=a, log2_twice=b, promotions=st["promotions"],
                     once_fill=round(st["once_bits_set"] / (64.0 * (1 << a)), 4), twice_fill=round(st["twice_bits_set"] / (64.0 * (1 << b)), 4),
                     table_slots_filtered=small.capacity(), table_keys_filtered=keys2, seen_once_that_got_in=int(h2[1]),
                     share_of_seen_once=round(int(h2[1]) / max(once_true, 1), 6),
                     exact_part_matches=bool(keys2 - int(h2[1]) == distinct - once_true))
            if bits == (args.bits or [16])[0]:   # the timings, at the first size
                s["pass1"], s["kt_card_add_reads"] = alternating(pass1, card, args.reps)
                s["pass1_again"], s["kt_ctr_add_reads_probing"] = alternating(pass1, probing, args.reps)
                s["pass2"], s["kt_ctr_add_reads_probing_again"] = alternating(pass2, probing, args.reps)
                s["pass2_again"], s["kt_ctr_add_reads_bulk"] = alternating(pass2, bulk, args.reps)
                s["pass1_over_card"] = round(s["pass1"]["median_ms"] / s["kt_card_add_reads"]["median_ms"], 3)
                s["pass1_over_probing"] = round(s["pass1_again"]["median_ms"] / s["kt_ctr_add_reads_probing"]["median_ms"], 3)
                s["pass2_over_probing"] = round(s["pass2"]["median_ms"] / s["kt_ctr_add_reads_probing_again"]["median_ms"], 3)
                s["pass2_over_bulk"] = round(s["pass2_again"]["median_ms"] / s["kt_ctr_add_reads_bulk"]["median_ms"], 3)
            row = dict(r, **s)
            print(json.dumps(row), flush=True)
            rows.append(row)
            small.close()
            f.close()
        os.environ["KT_BULK"] = "1"
        full.close()
        torch.cuda.empty_cache()
    ctx.close()
    head = "# tools/prefilter_timing.py, commit %s (+ working tree), %s, medians of %d between events, the calls of a pair alternating" % (
        commit or "unknown", torch.cuda.get_device_name(0), args.reps)
    pathlib.Path(args.out).parent.mkdir(exist_ok=True)
    pathlib.Path(args.out).write_text(head + "\n" + "".join(json.dumps(r) + "\n" for r in rows))


if __name__ == "__main__":
    main()
