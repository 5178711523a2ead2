"""Times kt_unitig_components beside kt_ctr_unitigs_linked on the same table, and kt_thread_read_components beside
kt_thread_runs on the same batch (profiles/components_kernel.txt is this script's output with notes).

The read set is the `thread` benchmark's (tools/measure_thread.py): --reads x 150 bp synthetic reads (bench.py's seed) sampled
from a random genome of --genome bases, k = 31; the graph is that of the k-mers with count >= --min-count (given several
times: 2, then 1), the batch the same reads threaded onto its unitigs.  One process, everything in device memory; the two
calls of a pair alternate after a warm-up of each, a time is the span between two device events around the call (both calls
of either pair wait for the stream themselves to learn their sizes, so the span is the call), and the record is the median
of --reps with minimum and maximum, the two pairs side by side.

    python tools/components_timing.py [--reads 10000000] [--genome 50000000] [--out profiles/components_kernel.txt]
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


def alternating(f, g, reps):
    f(), g()
    tf, tg = [], []
    for _ in range(reps):
        tf.append(timed(f))
        tg.append(timed(g))
    return [dict(median_ms=round(float(np.median(t)), 3), min_ms=round(min(t), 3), max_ms=round(max(t), 3)) for t in (tf, tg)]


def empty(n, dtype):
    return torch.empty(max(int(n), 1), dtype=dtype, device="cuda")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=10_000_000)
    ap.add_argument("--genome", type=int, default=50_000_000)
    ap.add_argument("--min-count", type=int, action="append")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "components_kernel.txt"))
    args = ap.parse_args()
    k, L = 31, 150
    n, total = args.reads, args.reads * L
    try:
        commit = subprocess.run(["git", "-C", str(ROOT), "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip()
    except OSError:
        commit = ""
    ctx = device.Context(0, stream=torch.cuda.current_stream().cuda_stream)
    bases = torch.empty(total, dtype=torch.uint8, device="cuda")
    offsets = torch.empty(n + 1, dtype=torch.int64, device="cuda")
    ctx.synth_reads(SEED, n, L, bases, offsets, genome_len=args.genome)
    table = device.Counter(ctx, k, int(1.9 * n * (L - k + 1)) + (1 << 20))  # (room for every window to be distinct)
    table.add_reads(bases, offsets, n)
    rows = []
    for lo in args.min_count or [2, 1]:
        r = dict(reads=n, length=L, genome=args.genome, k=k, min_count=lo, entries=table.size())
        nu, nb, nl = table.unitigs_linked_device(None, 0, None, None, None, 0, None, None, 0, lo)
        ub, uo, us, uf = empty(nb, torch.uint8), empty(nu + 1, torch.int64), empty(nu, torch.int64), empty(nu, torch.int32)
        lo_, lt = empty(2 * nu + 1, torch.int64), empty(nl, torch.int32)
        comp, stats, tally = empty(nu, torch.int32), empty(5 * nu, torch.int64), empty(6, torch.int64)
        got = {}

        def linked():
            table.unitigs_linked_device(ub, nb, uo, us, uf, nu, lo_, lt, nl, lo)

        def components():
            got["nc"] = ctx.unitig_components(lo_, lt, nu, comp, uo, us, k, stats, nu, tally)

        linked()
        r["kt_ctr_unitigs_linked"], r["kt_unitig_components"] = alternating(linked, components, args.reps)
        nc = got["nc"]
        t = tally.cpu().numpy()
        r.update(unitigs=nu, unitig_bases=nb, links=nl, components=nc, singletons=int(t[1]), largest_unitigs=int(t[2]),
                 largest_nodes=int(t[3]), nodes=nb - nu * (k - 1), rounds=int(t[5]))
        r["components_over_linked"] = round(r["kt_unitig_components"]["median_ms"] / r["kt_ctr_unitigs_linked"]["median_ms"], 4)
        print(json.dumps(r), flush=True)

        # the same reads threaded onto those unitigs
        try:
            index = device.Counter(ctx, k, max(1 << 20, int(1.9 * (nb - nu * (k - 1)))))
            index.index_sequences(ub, uo, nu)
            hits = torch.full((total,), -1, dtype=torch.int32, device="cuda")
            index.thread_hits(bases, offsets, n, hits)
            index.close()
            roff, rtally = empty(n + 1, torch.int64), empty(6, torch.int64)
            nr = ctx.thread_runs(hits, offsets, n, uo, nu, k, run_offsets=roff, tally=rtally)
            rs, rl, ru, rp = empty(nr, torch.int64), empty(nr, torch.int32), empty(nr, torch.int32), empty(nr, torch.int32)
            rcomp, rmixed = empty(n, torch.int32), empty(n, torch.uint8)
            creads, chits = torch.zeros(max(nc, 1), dtype=torch.int64, device="cuda"), torch.zeros(max(nc, 1), dtype=torch.int64, device="cuda")
            ctally = empty(4, torch.int64)

            def runs():
                ctx.thread_runs(hits, offsets, n, uo, nu, k, rs, rl, ru, rp, roff, nr, None, None, rtally)

            def read_components():
                ctx.thread_read_components(ru, rl, roff, n, comp, nu, nc, rcomp, rmixed, creads, chits, ctally)

            runs()
            r["kt_thread_runs"], r["kt_thread_read_components"] = alternating(runs, read_components, args.reps)
            t = ctally.cpu().numpy()
            r.update(runs=nr, reads_with_component=int(t[0]), reads_without=int(t[1]), reads_mixed=int(t[2]),
                     components_hit=int((chits != 0).sum().item()))
            r["read_components_over_runs"] = round(r["kt_thread_read_components"]["median_ms"] / r["kt_thread_runs"]["median_ms"], 4)
        except device._lib.KmertoolsError as e:  # (the unitigs of a graph with every error k-mer may pass the index's 2^31 - 2 bases)
            r["thread"] = "not run: %s" % e
        print(json.dumps(r), flush=True)
        rows.append(r)
        del ub, uo, us, uf, lo_, lt, comp, stats
        hits = rs = rl = ru = rp = rcomp = rmixed = roff = None
        torch.cuda.empty_cache()
    table.close()
    ctx.close()
    head = "# tools/components_timing.py, commit %s (+ working tree), %s, medians of %d between events, the calls of a pair alternating" % (
        commit or "unknown", torch.cuda.get_device_name(0), args.reps)
    pathlib.Path(args.out).parent.mkdir(exist_ok=True)
    pathlib.Path(args.out).write_text(head + "\n" + "".join(json.dumps(r) + "\n" for r in rows))


if __name__ == "__main__":
    main()
