"""Times kt_ctr_thread_hits against kt_ctr_profile on the same batch and the same table, and kt_thread_runs and
kt_ctr_index_sequences beside them (profiles/thread_kernel.txt is this script's output with notes).

The batch is the benchmark's: --reads x 150 bp synthetic reads (bench.py's seed), k = 31; with --genome G the reads are
sampled from a random genome of G bases, so that most k-mers occur more than once.  The table the two kernels probe is the
index of the unitigs of that read set at --min-count 2.  Both calls run on device memory; a time is the span between two
device events around the call (the segment index kernel and the probing kernel; one 8-byte read-back of the batch's size in
front), alternating the two calls, after warm-up.  kt_thread_runs and kt_ctr_index_sequences synchronise themselves and are
timed with the host clock.

    python tools/measure_thread.py --reads 10000000 --genome 50000000 --out thread_kernel.txt
"""
import argparse
import pathlib
import sys
import time

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
SEED = 0x6b6d6572


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=10_000_000)
    ap.add_argument("--genome", type=int, default=0)
    ap.add_argument("--k", type=int, default=31)
    ap.add_argument("--min-count", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch

    from kmertools_amd import device
    assert torch.cuda.is_available(), "needs a GPU"
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    ctx = device.Context(0, stream=torch.cuda.current_stream().cuda_stream)
    n, L, k = a.reads, 150, a.k
    total = n * L
    bases = torch.empty(total, dtype=torch.uint8, device="cuda")
    offsets = torch.empty(n + 1, dtype=torch.int64, device="cuda")
    ctx.synth_reads(SEED, n, L, bases, offsets, genome_len=a.genome)
    say("batch: %d x %d bp synthetic reads (seed %#x, genome %s), k = %d, %d bases" % (n, L, SEED, a.genome or "none: random reads", k, total))

    table = device.Counter(ctx, k, int(1.9 * n * (L - k + 1)) + (1 << 20))  # (room for every window to be distinct)
    table.add_reads(bases, offsets, n)
    distinct = table.size()
    nu, nb = table.unitigs_device(None, 0, None, None, None, 0, min_count=a.min_count)
    ub = torch.empty(max(nb, 1), dtype=torch.uint8, device="cuda")
    uo = torch.zeros(nu + 1, dtype=torch.int64, device="cuda")
    if nu:
        table.unitigs_device(ub, nb, uo, None, None, nu, min_count=a.min_count)
    table.close()
    windows = nb - nu * (k - 1)
    say("graph: %d distinct k-mers counted, %d unitigs of %d bases (%d k-mers) at min-count %d" % (distinct, nu, nb, windows, a.min_count))

    index = device.Counter(ctx, k, max(1 << 20, int(1.9 * windows)))
    t_index = []
    for rep in range(3):
        index.clear()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        got = index.index_sequences(ub, uo, nu)
        torch.cuda.synchronize()
        t_index.append(time.perf_counter() - t0)
        assert got == windows
    say("kt_ctr_index_sequences (device memory, host clock, synchronised; 3 runs after a clear): %s ms"
        % ", ".join("%.2f" % (1e3 * t) for t in t_index))

    out = torch.empty(total, dtype=torch.int32, device="cuda")

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    def run_profile():
        out.fill_(-1)
        return timed(lambda: index.profile(bases, offsets, n, out))

    def run_hits():
        out.fill_(-1)
        return timed(lambda: index.thread_hits(bases, offsets, n, out))

    for _ in range(2):
        run_profile(), run_hits()
    tp, th = [], []
    for _ in range(a.repeats):
        tp.append(run_profile())
        th.append(run_hits())

    def row(name, t):
        t = np.array(t)
        say("%-22s median %.3f ms  min %.3f  max %.3f  spread (max - min) / median %.2f %%  -> %.1f Gbases/s at the median"
            % (name, np.median(t), t.min(), t.max(), 100 * (t.max() - t.min()) / np.median(t), total / np.median(t) / 1e6))

    say("device events around the call, %d alternating repeats after 2 warm-ups:" % a.repeats)
    row("kt_ctr_profile", tp)
    row("kt_ctr_thread_hits", th)
    say("ratio thread_hits / profile (medians): %.4f" % (np.median(th) / np.median(tp)))

    # the runs: a counting call, then one sized by it (hits are in `out` from the last run_hits)
    n_hit = int((out > 0).sum().item()) if total <= (1 << 31) else -1
    off = torch.empty(n + 1, dtype=torch.int64, device="cuda")
    tally = torch.empty(6, dtype=torch.int64, device="cuda")
    t_count, t_fill = [], []
    for rep in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        nr = ctx.thread_runs(out, offsets, n, uo, nu, k, run_offsets=off, tally=tally)
        torch.cuda.synchronize()
        t_count.append(time.perf_counter() - t0)
        rs = torch.empty(max(nr, 1), dtype=torch.int64, device="cuda")
        rl, ru, rp = (torch.empty(max(nr, 1), dtype=torch.int32, device="cuda") for _ in range(3))
        uh = torch.zeros(max(nu, 1), dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if nr:
            ctx.thread_runs(out, offsets, n, uo, nu, k, rs, rl, ru, rp, off, nr, uh, None, tally)
        torch.cuda.synchronize()
        t_fill.append(time.perf_counter() - t0)
        del rs, rl, ru, rp
    say("hits %d of %d windows; runs %d; tally %s" % (n_hit, n * (L - k + 1), nr, tally.cpu().numpy().tolist()))
    say("kt_thread_runs, counting call (host clock, synchronised; 3 runs): %s ms" % ", ".join("%.2f" % (1e3 * t) for t in t_count))
    say("kt_thread_runs, call that writes the runs (3 runs): %s ms" % ", ".join("%.2f" % (1e3 * t) for t in t_fill))
    index.close()
    ctx.close()
    if a.out:
        pathlib.Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n\n")


if __name__ == "__main__":
    main()
