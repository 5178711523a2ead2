"""Times kt_ctr_unitigs_linked on the device beside kt_ctr_unitigs on the same table (tools/unitig_timing.py's: reads sampled
by kt_synth_reads from a random genome, both strands, 1 % substitutions, k = 31, min_count = 2), everything written in both.
One process, warm-ups first, medians of 5 between events on the context's stream, with minimum and maximum.  The linked
call contains the unlinked one; what the link stages add comes from a kernel trace of this same script (unitig_end_*_kernel,
and scan2_tile_scan_kernel once more per linked call) beside stage b's unitig_link_kernel in the same trace.

    python tools/unitig_links_timing.py [--genome 20000000] [--coverage 30] [--out profiles/unitig_links_timing.txt]

--unlinked-only times kt_ctr_unitigs alone and needs no kt_ctr_unitigs_linked in the library: with KT_LIB pointing at a build
from before the links it gives the figure the first line is compared with.
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
from kmertools_amd import _lib, device  # noqa: E402

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
    ap.add_argument("--unlinked-only", action="store_true")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "unitig_links_timing.txt"))
    args = ap.parse_args()
    if args.unlinked_only:
        _lib.SYMBOLS.pop("kt_ctr_unitigs_linked", None)
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
    r = dict(library=str(_lib.LIB_PATH.name if _lib.LIB_PATH.parent == ROOT / "kmertools_amd" else _lib.LIB_PATH), genome=args.genome,
             reads=n, length=L, k=k, min_count=lo, entries=t.size(), slots=t.capacity())
    nu, nb = t.unitigs_device(None, 0, None, None, None, 0, lo)
    r.update(unitigs=nu, bases=nb, nodes=nb - nu * (k - 1))
    ub = torch.empty(nb, dtype=torch.uint8, device="cuda")
    uo = torch.empty(nu + 1, dtype=torch.int64, device="cuda")
    us = torch.empty(nu, dtype=torch.int64, device="cuda")
    uf = torch.empty(nu, dtype=torch.int32, device="cuda")
    r["unitigs"] = timed(lambda: t.unitigs_device(ub, nb, uo, us, uf, nu, lo), 2, args.reps)
    if not args.unlinked_only:
        plain = [x.clone() for x in (ub, uo, us, uf)]
        nu2, nb2, nl = t.unitigs_linked_device(None, 0, None, None, None, 0, None, None, 0, lo)
        assert (nu2, nb2) == (nu, nb)
        lo_ = torch.empty(2 * nu + 1, dtype=torch.int64, device="cuda")
        lt = torch.empty(nl, dtype=torch.int32, device="cuda")
        r["unitigs_linked"] = timed(lambda: t.unitigs_linked_device(ub, nb, uo, us, uf, nu, lo_, lt, nl, lo), 2, args.reps)
        assert all(torch.equal(a, b) for a, b in zip(plain, (ub, uo, us, uf))), "the linked call spells other unitigs"
        deg = (lo_[1:] - lo_[:-1]).cpu().numpy()
        assert int(lo_[-1].item()) == nl == int(deg.sum())
        r.update(links=nl, dead_ends=int((deg == 0).sum()), max_end_degree=int(deg.max()),
                 end_degrees={str(d): int((deg == d).sum()) for d in range(int(deg.max()) + 1)},
                 self_links=int(((lt.cpu().numpy().view(np.uint32) >> 1) == np.repeat(np.arange(2 * nu) >> 1, deg)).sum()))
        r["linked_over_unlinked"] = round(r["unitigs_linked"]["median_ms"] / r["unitigs"]["median_ms"], 4)
        r["links_ms"] = round(r["unitigs_linked"]["median_ms"] - r["unitigs"]["median_ms"], 3)
    print(json.dumps(r), flush=True)
    t.close()
    ctx.close()
    head = "# tools/unitig_links_timing.py, commit %s (+ working tree), %s, medians between events" % (
        commit or "unknown", torch.cuda.get_device_name(0))
    pathlib.Path(args.out).parent.mkdir(exist_ok=True)
    pathlib.Path(args.out).write_text(head + "\n" + json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
