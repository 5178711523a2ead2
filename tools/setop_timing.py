"""kt_ctr_setop beside kt_ctr_compare on the full-size test's pair (k = 31, A = 10 M x 150 bp, B = 4 M reads of the same
20 Mbase genome): hipEvents round every call on the context's stream, warm-up calls first, medians.  One JSON document on
stdout."""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from kmertools_amd import device  # noqa: E402


def timed(fn, warm=2, reps=7):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    ts.sort()
    return dict(median_ms=ts[len(ts) // 2], min_ms=ts[0], max_ms=ts[-1])


def main():
    ctx = device.Context(0, stream=torch.cuda.current_stream().cuda_stream)
    k, L, genome = 31, 150, 20_000_000
    tabs = []
    for n, seed in ((10_000_000, 0x5E70A), (4_000_000, 0x5E70B)):
        bases = torch.empty(n * L, dtype=torch.uint8, device="cuda")
        offsets = torch.empty(n + 1, dtype=torch.int64, device="cuda")
        ctx.synth_reads(seed, n, L, bases, offsets, noise=True, genome_len=genome)
        c = device.Counter(ctx, k, int(1.9 * n * (L - k + 1)))
        c.add_reads(bases, offsets, n)
        tabs.append(c)
        del bases, offsets
        torch.cuda.empty_cache()
    a, b = tabs
    res = dict(size_a=a.size(), size_b=b.size(), slots_a=a.capacity(), slots_b=b.capacity())
    m = torch.zeros((1001, 101), dtype=torch.int64, device="cuda")
    t6 = torch.zeros(6, dtype=torch.int64, device="cuda")
    res["compare"] = timed(lambda: a.compare_into(b, m, 1001, 101, t6))  # (the warm-up makes B's probing image)
    for op in ("subtract", "intersect", "union"):  # union last: it turns A into its probing image
        n = a.setop_device(b, op, None, None, 0, sort=False)
        keys = torch.empty(n, dtype=torch.int64, device="cuda")
        counts = torch.empty(n, dtype=torch.int32, device="cuda")
        r = dict(n_out=n)
        r["count_only"] = timed(lambda: a.setop_device(b, op, None, None, 0, sort=False))
        r["unsorted"] = timed(lambda: a.setop_device(b, op, keys, counts, n, sort=False))
        r["sorted"] = timed(lambda: a.setop_device(b, op, keys, counts, n, sort=True), warm=1, reps=3)
        r["sort_ms_per_million"] = (r["sorted"]["median_ms"] - r["unsorted"]["median_ms"]) / (n / 1e6)
        r["probes_per_s"] = (res["size_a"] + (res["size_b"] if op == "union" else 0)) / (r["unsorted"]["median_ms"] * 1e-3)
        res[op] = r
        del keys, counts
        torch.cuda.empty_cache()
    src = torch.empty(res["subtract"]["n_out"] * 12, dtype=torch.uint8, device="cuda")
    dst = torch.empty_like(src)
    res["copy_of_subtract_bytes"] = timed(lambda: dst.copy_(src))
    print(json.dumps(res, indent=1))
    a.close()
    b.close()
    ctx.close()


if __name__ == "__main__":
    main()
