"""Times kt_ctr_graph on the device beside kt_ctr_compare(a, a) on the same table - the same entry walk with 1 probe per
entry where the graph makes 14 per node.  One process, warm-ups first, medians between events on the context's stream, per
table:

  compare     kt_ctr_compare(a, a) into a 4 x 4 matrix: ns per probe = time / entries;
  count only  kt_ctr_graph with max_out = 0 (the walk, the 14 probes, the census; nothing stored);
  unsorted    ... with the (key, info) pairs compacted and the counts looked up;
  sorted      ... and the pairs sorted by key; ns per probe = time / (14 x nodes).
Tables: bench.py's ctr_k31 (25 M x 150 bases, uniform reads: nearly every 31-mer once) and ctr_k15 (50 M x 150 bases: nearly
every canonical 15-mer, the complete graph), the tables sized as the benchmark sizes them.

    python tools/graph_timing.py [--scale 1.0] [--out profiles/graph_timing.txt]
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


def timed(fn, warm, reps):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return dict(median_ms=round(float(np.median(ms)), 3), min_ms=round(min(ms), 3), max_ms=round(max(ms), 3))


def table_shape(ctx, name, k, n, L, cfg, emit):
    bases = torch.empty(n * L, dtype=torch.uint8, device="cuda")
    offsets = torch.empty(n + 1, dtype=torch.int64, device="cuda")
    ctx.synth_reads(SEED + cfg, n, L, bases, offsets)
    max_distinct = min(n * (L - k + 1), (4 ** k + 2 ** k) // 2)
    t = device.Counter(ctx, k, max(1 << 20, int(1.9 * max_distinct)))
    t.add_reads(bases, offsets, n)
    del bases, offsets
    torch.cuda.empty_cache()
    size, slots = t.size(), t.capacity()
    r = dict(table=name, k=k, reads=n, length=L, entries=size, slots=slots)
    m = torch.zeros((4, 4), dtype=torch.int64, device="cuda")
    t6 = torch.zeros(6, dtype=torch.int64, device="cuda")
    r["compare"] = timed(lambda: t.compare_into(t, m, 4, 4, t6), 2, 5)  # (the warm-up makes the probing image)
    r["compare_ns_per_probe"] = round(r["compare"]["median_ms"] * 1e6 / size, 4)
    cen = torch.zeros(32, dtype=torch.int64, device="cuda")
    nodes = t.graph_device(None, None, None, 0, census=cen)
    census = cen.cpu().numpy()
    r.update(nodes=nodes, census={device.GRAPH_CENSUS_NAMES[j]: int(census[j]) for j in range(32) if census[j]})
    r["count_only"] = timed(lambda: t.graph_device(None, None, None, 0, census=cen), 1, 5)
    keys = torch.empty(nodes, dtype=torch.int64, device="cuda")
    info = torch.empty(nodes, dtype=torch.int32, device="cuda")
    counts = torch.empty(nodes, dtype=torch.int32, device="cuda")
    r["unsorted_no_counts"] = timed(lambda: t.graph_device(keys, info, None, nodes, sort=False, census=cen), 1, 5)
    r["unsorted"] = timed(lambda: t.graph_device(keys, info, counts, nodes, sort=False, census=cen), 1, 5)
    r["sorted"] = timed(lambda: t.graph_device(keys, info, counts, nodes, sort=True, census=cen), 1, 3)
    for what in ("count_only", "unsorted", "sorted"):
        r[what + "_ns_per_probe"] = round(r[what]["median_ms"] * 1e6 / (14 * nodes), 4)
        r[what + "_ns_per_node"] = round(r[what]["median_ms"] * 1e6 / nodes, 4)
    r["sort_ms_per_million"] = round((r["sorted"]["median_ms"] - r["unsorted"]["median_ms"]) / (nodes / 1e6), 4)
    r["probe_time_over_compare"] = round(r["unsorted_ns_per_probe"] / r["compare_ns_per_probe"], 3)
    emit(r)
    del keys, info, counts
    t.close()
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0, help="shrinks the read counts (a quick look)")
    ap.add_argument("--only", choices=("ctr_k31", "ctr_k15"), help="one of the two tables")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "graph_timing.txt"))
    args = ap.parse_args()
    try:
        commit = subprocess.run(["git", "-C", str(ROOT), "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip()
    except OSError:
        commit = ""
    lines = ["# tools/graph_timing.py, commit %s (+ working tree), %s, scale %g, medians between events" % (
        commit or "unknown", torch.cuda.get_device_name(0), args.scale)]

    def emit(r):
        print(json.dumps(r), flush=True)
        lines.append(json.dumps(r))

    ctx = device.Context(0, stream=torch.cuda.current_stream().cuda_stream)
    for name, k, n, L, cfg in (("ctr_k31", 31, 25_000_000, 150, 3), ("ctr_k15", 15, 50_000_000, 150, 2)):
        if args.only in (None, name):
            table_shape(ctx, name, k, int(n * args.scale), L, cfg, emit)
    ctx.close()
    pathlib.Path(args.out).parent.mkdir(exist_ok=True)
    pathlib.Path(args.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
