"""Times kt_ctr_hetmers on the device beside kt_ctr_graph on the same table.  One process, device-resident synthetic reads
(kt_synth_reads: 10 M x 150 bp sampled from a 50 Mbase genome, 1 % errors - 30x coverage, tools/card_bench.py's read set),
counted at k = 21 and k = 31; warm-ups first, medians between events on the context's stream.  Per table and count range:

  hetmers count only   kt_ctr_hetmers with max_out = 0: the three kernels, the census and the matrix, nothing stored;
  hetmers middle       ... the middle base alone (3 probes per node instead of 3k);
  hetmers sorted       ... with the pairs compacted, sorted by their first key and both counts looked up;
  graph count only     kt_ctr_graph with max_out = 0 (14 probes per node), for scale;
  probes per node      the kernel's stopping rule replayed on the host for a sample of the nodes (their 3k variants looked
                       up with kt_ctr_lookup; a lane stops issuing groups of HET_POS positions once it has seen two distinct
                       solid neighbours), beside the 3k a node without early stop would issue.
The stages' own times are the kernels' (het_nodes_kernel, het_scan_kernel, het_verify_kernel) in a kernel trace of `--trace` (a short run of
the count-only calls alone, to be started under the profiler).

    python tools/hetmer_timing.py [--scale 1.0] [--out profiles/hetmers_timing.txt] [--trace]
"""
import argparse
import json
import pathlib
import sys

import numpy as np
import torch

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from kmertools_amd import device  # noqa: E402

L, GENOME, SEED = 150, 50_000_000, 0x63617264  # tools/card_bench.py's
HET_POS = 5  # kt_ctr.hip's group: positions per Probed::counts call


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
    return dict(median_ms=round(float(np.median(ms)), 3), min_ms=round(min(ms), 3), max_ms=round(max(ms), 3), runs=reps)


def rc(x, k):
    u = np.uint64
    x = ~x
    for sh, m in ((2, 0x3333333333333333), (4, 0x0F0F0F0F0F0F0F0F), (8, 0x00FF00FF00FF00FF), (16, 0x0000FFFF0000FFFF)):
        x = ((x >> u(sh)) & u(m)) | ((x & u(m)) << u(sh))
    x = (x >> u(32)) | (x << u(32))
    return x >> u(64 - 2 * k)


def probes_issued(t, k, lo, hi, sample):
    """the scan's probes for `sample` of the nodes: (nodes sampled, probes issued, probes without the early stop)"""
    n = t.export_stage_range(lo, hi)
    F, _ = t.export_fetch(0, min(n, sample))
    F = F[:min(n, sample)]
    top = 0xFFFFFFFF if hi is None else hi
    issued = np.zeros(len(F), np.int64)
    whole = np.zeros(len(F), np.int64)
    first = np.full(len(F), np.uint64(0xFFFFFFFFFFFFFFFF))
    have, multi = np.zeros(len(F), bool), np.zeros(len(F), bool)
    for i0 in range(0, k, HET_POS):
        cand = []
        for i in range(i0, min(i0 + HET_POS, k)):
            for d in (1, 2, 3):
                f = F ^ np.uint64(d << 2 * (k - 1 - i))
                cand.append(np.minimum(f, rc(f, k)))
        cand = np.stack(cand, axis=1)
        counts = t.lookup_host(cand.reshape(-1)).reshape(cand.shape)
        want = cand != F[:, None]
        whole += want.sum(axis=1)
        issued += np.where(multi, 0, want.sum(axis=1))
        solid = want & (counts >= lo) & (counts <= top)
        for j in range(cand.shape[1]):  # in the kernel's order
            s, c = solid[:, j], cand[:, j]
            fresh = s & ~have
            first[fresh] = c[fresh]
            multi |= s & have & ~fresh & (c != first)
            have |= s
    return len(F), int(issued.sum()), int(whole.sum())


def table_shape(ctx, k, n, emit, trace, sample):
    bases = torch.empty(n * L, dtype=torch.uint8, device="cuda")
    offsets = torch.empty(n + 1, dtype=torch.int64, device="cuda")
    ctx.synth_reads(SEED, n, L, bases, offsets, genome_len=GENOME)
    t = device.Counter(ctx, k, 1 << 30)
    t.add_reads(bases, offsets, n)
    del bases, offsets
    torch.cuda.empty_cache()
    size, slots = t.size(), t.capacity()
    cen = torch.zeros(8, dtype=torch.int64, device="cuda")
    gcen = torch.zeros(32, dtype=torch.int64, device="cuda")
    m = torch.zeros((501, 1001), dtype=torch.int64, device="cuda")
    for lo, hi in ((1, None), (2, None)):
        r = dict(k=k, reads=n, length=L, genome=GENOME, entries=size, slots=slots, min_count=lo, max_count=hi)
        count_only = lambda middle=False: t.hetmers_device(None, None, None, None, 0, lo, hi, middle=middle, matrix=m, n_rows=501,
                                                           n_cols=1001, census=cen)
        if trace:  # the kernels' own times come from the profiler's trace of these calls
            timed(count_only, 1, 3)
            timed(lambda: t.graph_device(None, None, None, 0, lo, hi, census=gcen), 1, 3)
            emit(dict(r, traced="3 count-only calls of kt_ctr_hetmers and of kt_ctr_graph after one warm-up each"))
            continue
        cen.zero_()
        pairs = count_only()
        census = cen.cpu().numpy()
        r.update(pairs=pairs, census={device.HET_CENSUS_NAMES[j]: int(census[j]) for j in range(8)})
        r["candidates_at_most"] = int(census[3])  # (verify runs for the degree-1 nodes with F < n1: about half of them)
        r["hetmers_count_only"] = timed(count_only, 1, 5)
        r["hetmers_count_only_ns_per_node"] = round(r["hetmers_count_only"]["median_ms"] * 1e6 / max(1, int(census[0])), 4)
        r["hetmers_middle_count_only"] = timed(lambda: count_only(True), 1, 5)
        ka, kb = (torch.empty(max(1, pairs), dtype=torch.int64, device="cuda") for _ in range(2))
        ca, cb = (torch.empty(max(1, pairs), dtype=torch.int32, device="cuda") for _ in range(2))
        if pairs:
            r["hetmers_sorted"] = timed(lambda: t.hetmers_device(ka, kb, ca, cb, pairs, lo, hi, sort=True), 1, 3)
        r["graph_count_only"] = timed(lambda: t.graph_device(None, None, None, 0, lo, hi, census=gcen), 1, 5)
        r["hetmers_over_graph"] = round(r["hetmers_count_only"]["median_ms"] / r["graph_count_only"]["median_ms"], 3)
        ns, issued, whole = probes_issued(t, k, lo, hi, sample)
        r.update(probe_sample_nodes=ns, probes_per_node_issued=round(issued / max(1, ns), 3),
                 probes_per_node_without_early_stop=round(whole / max(1, ns), 3), probes_per_node_3k=3 * k)
        if ns:
            r["hetmers_count_only_ns_per_probe_issued"] = round(r["hetmers_count_only_ns_per_node"] / (issued / ns), 4)
        emit(r)
        del ka, kb, ca, cb
    t.close()
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0, help="shrinks the read count (a quick look)")
    ap.add_argument("--sample", type=int, default=200_000, help="nodes whose probes are replayed on the host")
    ap.add_argument("--trace", action="store_true", help="only a few count-only calls, for a kernel trace")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "hetmers_timing.txt"))
    args = ap.parse_args()
    n = int(10_000_000 * args.scale)
    lines = ["# tools/hetmer_timing.py%s, %s, %d reads x %d bp from a %d-base genome, medians between events" % (
        " --trace" if args.trace else "", torch.cuda.get_device_name(0), n, L, GENOME)]

    def emit(r):
        print(json.dumps(r), flush=True)
        lines.append(json.dumps(r))

    ctx = device.Context(0, stream=torch.cuda.current_stream().cuda_stream)
    for k in (21, 31):
        table_shape(ctx, k, n, emit, args.trace, args.sample)
    ctx.close()
    pathlib.Path(args.out).parent.mkdir(exist_ok=True)
    pathlib.Path(args.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
