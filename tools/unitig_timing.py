"""Times kt_ctr_unitigs on the device beside kt_ctr_graph (sorted, with counts) on the same table: reads sampled by
kt_synth_reads from a random genome (both strands, 1 % substitutions), k = 31, min_count = 2 - the solid k-mers of a
sequenced genome, the table an assembler compacts.  One process, warm-ups first, medians between events on the context's
stream.  kt_ctr_unitigs calls kt_ctr_graph for its nodes, so its time contains the graph's; the per-stage split of the rest
comes from a kernel trace of this same script (the kernels are named unitig_<stage>_kernel).

    python tools/unitig_timing.py [--genome 20000000] [--coverage 30] [--out profiles/unitig_timing.txt]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genome", type=int, default=20_000_000)
    ap.add_argument("--coverage", type=float, default=30.0)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "unitig_timing.txt"))
    args = ap.parse_args()
    k, L, lo = 31, 150, 2
    n = int(args.genome * args.coverage / L)
    try:
        commit = subprocess.run(["git", "-C", str(ROOT), "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip()
    except OSError:
        commit = ""
    ctx = device.Context(0, stream=torch.cuda.current_stream().cuda_stream)
    bases = torch.empty(n * L, dtype=torch.uint8, device="cuda")
    offsets = torch.empty(n + 1, dtype=torch.int64, device="cuda")
    ctx.synth_reads(SEED + 7, n, L, bases, offsets, genome_len=args.genome)
    # every read carries about 1.5 errors, each up to k new k-mers
    t = device.Counter(ctx, k, max(1 << 20, int(1.9 * (2 * args.genome + n * 1.5 * k * 1.1))))
    t.add_reads(bases, offsets, n)
    del bases, offsets
    torch.cuda.empty_cache()
    r = dict(genome=args.genome, reads=n, length=L, k=k, min_count=lo, entries=t.size(), slots=t.capacity())
    cen = torch.zeros(32, dtype=torch.int64, device="cuda")
    nodes = t.graph_device(None, None, None, 0, lo, census=cen)
    census = cen.cpu().numpy()
    r.update(nodes=nodes, census={device.GRAPH_CENSUS_NAMES[j]: int(census[j]) for j in range(7)})
    keys = torch.empty(nodes, dtype=torch.int64, device="cuda")
    info = torch.empty(nodes, dtype=torch.int32, device="cuda")
    counts = torch.empty(nodes, dtype=torch.int32, device="cuda")
    r["graph_sorted_counts"] = timed(lambda: t.graph_device(keys, info, counts, nodes, lo, sort=True), 2, args.reps)
    del keys, info, counts
    nu, nb = t.unitigs_device(None, 0, None, None, None, 0, lo)
    r.update(unitigs=nu, bases=nb)
    r["unitigs_count_only"] = timed(lambda: t.unitigs_device(None, 0, None, None, None, 0, lo), 1, args.reps)
    ub = torch.empty(nb, dtype=torch.uint8, device="cuda")
    uo = torch.empty(nu + 1, dtype=torch.int64, device="cuda")
    us = torch.empty(nu, dtype=torch.int64, device="cuda")
    uf = torch.empty(nu, dtype=torch.int32, device="cuda")
    r["unitigs"] = timed(lambda: t.unitigs_device(ub, nb, uo, us, uf, nu, lo), 1, args.reps)
    lens = (uo[1:] - uo[:-1]).cpu().numpy()
    r.update(longest=int(lens.max()), circular=int((uf & 1).sum().item()), singletons=int((lens == k).sum()),
             occurrences=int(us.sum().item()))
    assert int(lens.sum()) == nb and nb == nodes + nu * (k - 1) and r["occurrences"] == int(census[1])
    r["unitigs_over_graph"] = round(r["unitigs"]["median_ms"] / r["graph_sorted_counts"]["median_ms"], 3)
    r["ns_per_node_beyond_graph"] = round((r["unitigs"]["median_ms"] - r["graph_sorted_counts"]["median_ms"]) * 1e6 / nodes, 3)
    print(json.dumps(r), flush=True)
    t.close()
    ctx.close()
    head = "# tools/unitig_timing.py, commit %s (+ working tree), %s, medians between events" % (
        commit or "unknown", torch.cuda.get_device_name(0))
    pathlib.Path(args.out).parent.mkdir(exist_ok=True)
    pathlib.Path(args.out).write_text(head + "\n" + json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
