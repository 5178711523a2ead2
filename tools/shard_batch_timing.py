"""Times the host side of a sharded batch where it shows: --rounds x (kt_sharded_clear, kt_sharded_add_reads of one device
batch of --reads x 150 bases, kt_sharded_finalize, kt_ctr_size) on one GPU, a single rank made to take the routed path
(KT_SHARD_FORCE, 3 unless the environment says otherwise), after --warm unmeasured rounds.  The batch is small (4.2 Mbases):
a round is a few dozen launches and the calls around them, so a change to the host half of kt_shard.hip is a visible part
of it.  One process, wall clock round the loop (every round ends in kt_ctr_size's read-back: nothing is left in flight).

    python tools/shard_batch_timing.py [--k 31] [--rounds 200] [--warm 20] [--label "this build"]

With KT_LIB pointing at another build of the library, in a process of its own, it gives the figures this build's are set
beside; profiles/shard_batch_refactor_timing.txt is put together from such processes, the two libraries alternately.  Prints
one JSON line.
"""
import argparse
import json
import os
import pathlib
import sys
import time

import torch

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
os.environ.setdefault("KT_SHARD_FORCE", "3")
from kmertools_amd import _lib, device  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--k", type=int, default=31)
    ap.add_argument("--reads", type=int, default=28000)
    ap.add_argument("--rounds", type=int, default=200)
    ap.add_argument("--warm", type=int, default=20)
    ap.add_argument("--label", default="", help="names the library in the output instead of its path")
    args = ap.parse_args()
    n, L = args.reads, 150
    ctx = device.Context(0, stream=torch.cuda.current_stream().cuda_stream)
    bases = torch.empty(n * L, dtype=torch.uint8, device="cuda")
    offsets = torch.empty(n + 1, dtype=torch.int64, device="cuda")
    ctx.synth_reads(0x73686172, n, L, bases, offsets, noise=True)
    sh = device.Sharded(ctx, args.k, 1 << 23, n * L, 1, 0, None)

    def one_round():
        sh.clear()
        sh.add_reads(bases, offsets, n)
        sh.finalize()
        return sh.table.size()

    for _ in range(args.warm):
        entries = one_round()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.rounds):
        one_round()
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3
    rec, km = sh.route_stats()
    lib_path = pathlib.Path(_lib.LIB_PATH).resolve()
    print(json.dumps(dict(tool="shard_batch_timing", library=args.label or lib_path.name, k=args.k, owners=len(rec), bases=n * L,
                          rounds=args.rounds, warm=args.warm, loop_ms=round(ms, 3), ms_per_round=round(ms / args.rounds, 4),
                          entries=entries, kmers=int(km.sum()), records=int(rec.sum()))), flush=True)
    sh.close()
    ctx.close()


if __name__ == "__main__":
    main()
