"""The scenarios whose kernel launches profiles/shard_batch_refactor_launches.txt lists: one process, one GPU, a single rank
made to take the routed path (KT_SHARD_FORCE) into 1, 3 and 8 owners' regions, in 1 and 4 pieces, every time a batch into
an empty table and the same batch again on top (the range build, then the merge); a flood into regions of two blocks
(KT_SHARD_ROOM_BLOCKS=2: mostly poly-A and (AC)n, and enough random reads that kt_sharded_finalize needs more than one
round); and a batch small enough for the probing path.  Prints one JSON line per exported table: entries, sum of counts,
xor of keys.

    rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/shard_batch_launches.py > tables.jsonl
    python tools/shard_batch_launches.py --list DIR/.../*_kernel_trace.csv      # the launches, one per line

Run once with KT_LIB pointing at the parent commit's library and once with this tree's: the two lists and the two sets of
tables must be the same.
"""
import csv
import json
import os
import pathlib
import sys

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))


def short_name(name):
    """the kernel's name with its template arguments, without `void`, the anonymous namespace and the parameter list"""
    name = name.replace("(anonymous namespace)::", "")
    if name.startswith("void "):
        name = name[5:]
    depth = 0
    for i, ch in enumerate(name):
        depth += (ch == "<") - (ch == ">")
        if ch == "(" and depth == 0:
            return name[:i]
    return name


def list_launches(path):
    """the library's launches in the order they started; the runtime's own fill and copy kernels (hipMemsetAsync,
    hipMemcpyAsync) are counted, with their sizes, in one last line"""
    rows = list(csv.DictReader(open(path)))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    shape = "grid=%sx%sx%s block=%sx%sx%s lds=%s"
    cols = ("Grid_Size_X", "Grid_Size_Y", "Grid_Size_Z", "Workgroup_Size_X", "Workgroup_Size_Y", "Workgroup_Size_Z", "LDS_Block_Size")
    runtime = {}
    for r in rows:
        name, where = short_name(r["Kernel_Name"]), shape % tuple(r[c] for c in cols)
        if name.startswith("__amd_rocclr_"):
            runtime[name, where] = runtime.get((name, where), 0) + 1
        else:
            print(name, where)
    for (name, where), n in sorted(runtime.items()):
        print("# runtime: %d x %s %s" % (n, name, where))


def main():
    import torch
    from kmertools_amd import device
    ctx = device.Context(0, stream=torch.cuda.current_stream().cuda_stream)

    def table_line(name, sh):
        sh.finalize()
        keys, counts = sh.table.export_host()
        print(json.dumps(dict(scenario=name, entries=len(keys), sum_of_counts=int(counts.astype(np.uint64).sum()),
                              xor_of_keys=int(np.bitwise_xor.reduce(keys)) if len(keys) else 0)), flush=True)

    def env(**kw):
        for name in ("KT_SHARD_FORCE", "KT_SHARD_SLICES", "KT_SHARD_ROOM_BLOCKS", "KT_BULK_MIN_BASES"):
            os.environ.pop(name, None)
        os.environ.update({k: str(v) for k, v in kw.items()})

    n, L, k = 20000, 150, 31
    bases = torch.empty(n * L, dtype=torch.uint8, device="cuda")
    offsets = torch.empty(n + 1, dtype=torch.int64, device="cuda")
    ctx.synth_reads(0x6c61756e, n, L, bases, offsets, noise=True, genome_len=400000)
    for owners in (1, 3, 8):
        for slices in (1, 4):
            env(KT_SHARD_FORCE=owners, KT_SHARD_SLICES=slices, KT_BULK_MIN_BASES=0)
            sh = device.Sharded(ctx, k, 1 << 22, n * L, 1, 0, None)
            for batch in ("first", "second"):
                sh.add_reads(bases, offsets, n)
                table_line("owners %d, slices %d, %s batch" % (owners, slices, batch), sh)
            sh.close()
    rng = np.random.default_rng(7)
    alpha = np.frombuffer(b"ACGT", np.uint8)
    flood = [b"A" * 150] * 500 + [b"AC" * 75] * 400 + [alpha[rng.integers(0, 4, size=150)].tobytes() for _ in range(3000)]
    fb, fo = device.to_csr(flood)
    env(KT_SHARD_FORCE=2, KT_SHARD_ROOM_BLOCKS=2, KT_BULK_MIN_BASES=0)
    sh = device.Sharded(ctx, k, 1 << 22, int(fo[-1]), 1, 0, None)
    sh.add_reads_host(fb, fo)
    table_line("flood into regions of two blocks", sh)
    sh.close()
    env(KT_SHARD_FORCE=3)
    sh = device.Sharded(ctx, k, 1 << 22, n * L, 1, 0, None)
    sh.add_reads(bases[:2000 * L], offsets[:2001], 2000)
    table_line("a batch for the probing path", sh)
    sh.close()
    ctx.close()


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--list":
        list_launches(sys.argv[2])
    else:
        main()
