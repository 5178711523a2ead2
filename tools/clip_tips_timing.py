"""Times tip clipping on the device: one round and the whole of kt_ctr_clip_tips, beside kt_ctr_unitigs_linked, kt_ctr_unitigs,
the read-only kt_ctr_unitig_tips and the count of the same table.  The table is bench.py's genome-sampled ctr_k31 (reads of 150 bases
sampled by kt_synth_reads from a random genome, both strands, 1 % substitutions, 3.75-fold coverage, k = 31, every k-mer a
node), scaled: bench.py's 25 M reads from 1 Gbp hold more than the 2^31 - 2 entries the unitig calls take.  One process,
events on the context's stream round each call.  A clip changes the table, so a round is measured once: the first round as
kt_ctr_clip_tips with max_rounds = 1, the rest of the job as a second call.

    python tools/clip_tips_timing.py [--scale 0.04] [--out profiles/clip_tips_timing.txt]

--linked-only times the count and kt_ctr_unitigs_linked alone and needs none of the new calls in the library: with KT_LIB
pointing at a build from before them it gives the figure the round is set beside.
"""
import argparse
import json
import pathlib
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from kmertools_amd import _lib, device  # noqa: E402

SEED = 0x6b6d6572  # bench.py's
READS, LENGTH, GENOME, CFG = 25_000_000, 150, 1_000_000_000, 3  # bench.py's ctr_k31, genome-sampled


def once(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return round(a.elapsed_time(b), 3), out


def timed(fn, warm, reps):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ms = [once(fn)[0] for _ in range(reps)]
    return dict(median_ms=round(float(np.median(ms)), 3), min_ms=round(min(ms), 3), max_ms=round(max(ms), 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=0.04, help="of bench.py's reads and genome")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--linked-only", action="store_true")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "clip_tips_timing.txt"))
    args = ap.parse_args()
    if args.linked_only:
        for name in ("kt_ctr_erase", "kt_ctr_unitig_tips", "kt_ctr_clip_tips"):
            _lib.SYMBOLS.pop(name, None)
    k, L = 31, LENGTH
    n, genome = int(READS * args.scale), int(GENOME * args.scale)
    try:
        commit = subprocess.run(["git", "-C", str(ROOT), "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip()
    except OSError:
        commit = ""
    ctx = device.Context(0, stream=torch.cuda.current_stream().cuda_stream)
    bases = torch.empty(n * L, dtype=torch.uint8, device="cuda")
    offsets = torch.empty(n + 1, dtype=torch.int64, device="cuda")
    ctx.synth_reads(SEED + CFG, n, L, bases, offsets, genome_len=genome)
    slots = max(1 << 20, int(1.9 * n * (L - k + 1)))
    warm = device.Counter(ctx, k, slots)  # (the first count of a process pays for its buffers)
    warm.add_reads(bases, offsets, n)
    warm.close()
    t = device.Counter(ctx, k, slots)
    torch.cuda.synchronize()
    t0 = time.perf_counter()  # (the host's clock, up to the size being known: what a caller waits for)
    t.add_reads(bases, offsets, n)
    entries = t.size()
    torch.cuda.synchronize()
    count_ms = round((time.perf_counter() - t0) * 1e3, 3)
    del bases, offsets
    torch.cuda.empty_cache()
    r = dict(scale=args.scale, genome=genome, reads=n, length=L, k=k, entries=entries, slots=t.capacity(), count_ms=count_ms)
    nu, nb, nl = t.unitigs_linked_device(None, 0, None, None, None, 0, None, None, 0)
    r.update(unitigs=nu, bases=nb, links=nl)
    ub = torch.empty(nb, dtype=torch.uint8, device="cuda")
    uo = torch.empty(nu + 1, dtype=torch.int64, device="cuda")
    us = torch.empty(nu, dtype=torch.int64, device="cuda")
    uf = torch.empty(nu, dtype=torch.int32, device="cuda")
    lo_ = torch.empty(2 * nu + 1, dtype=torch.int64, device="cuda")
    lt = torch.empty(nl, dtype=torch.int32, device="cuda")
    r["unitigs_linked"] = timed(lambda: t.unitigs_linked_device(ub, nb, uo, us, uf, nu, lo_, lt, nl), 1, args.reps)
    r["unitigs_unlinked"] = timed(lambda: t.unitigs_device(ub, nb, uo, us, uf, nu), 1, args.reps)
    del ub, uo, us, uf, lo_, lt
    if args.linked_only:
        r["library"] = str(_lib.LIB_PATH)
        print(json.dumps(r), flush=True)
        pathlib.Path(args.out).parent.mkdir(exist_ok=True)
        pathlib.Path(args.out).write_text(json.dumps(r) + "\n")
        t.close()
        ctx.close()
        return
    marks = torch.empty(nu, dtype=torch.uint8, device="cuda")
    tally = torch.zeros(4, dtype=torch.int64, device="cuda")
    r["unitig_tips"] = timed(lambda: t.unitig_tips_device(marks, nu, tally), 1, args.reps)
    r["tally"] = tally.cpu().numpy().tolist()
    del marks
    some = torch.from_numpy(t.export_fetch(0, min(1000, t.export_stage_range()))[0].view(np.int64)).cuda()
    r["erase_1000_keys_ms"], gone = once(lambda: t.erase_device(some, len(some)))
    r["erased"] = gone
    r["first_round_ms"], first = once(lambda: t.clip_tips(max_rounds=1))
    r["first_round"] = first
    r["other_rounds_ms"], rest = once(lambda: t.clip_tips(max_rounds=64))
    r["other_rounds"] = rest
    r["clip_tips_ms"] = round(r["first_round_ms"] + r["other_rounds_ms"], 3)
    r["entries_after"] = t.size()
    r["round_over_linked_plus_count"] = round(r["first_round_ms"] / (r["unitigs_linked"]["median_ms"] + count_ms), 3)
    print(json.dumps(r), flush=True)
    t.close()
    ctx.close()
    head = "# tools/clip_tips_timing.py, commit %s (+ working tree), %s, events round each call" % (
        commit or "unknown", torch.cuda.get_device_name(0))
    pathlib.Path(args.out).parent.mkdir(exist_ok=True)
    pathlib.Path(args.out).write_text(head + "\n" + json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
