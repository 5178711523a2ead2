"""The scenario whose kernel launches profiles/table_forms_refactor_launches.txt lists: one process, one GPU, at k = 15 and
k = 31 one table driven through every form it can be in (cleared with the clear pending, the probing image, dense ranges,
its entries in an export target) and, in every form, through every export path: kt_ctr_export to device and to host memory
(with room, with too little, with none), kt_ctr_export_stage, kt_ctr_export_stage_range and kt_ctr_export_fetch - with the
calls that move a table from form to form in between (probing and bulk adds, a merge, a prober, add_pairs, erase, a change
of target).  Prints one JSON line per export: entries, sum of counts, xor of keys.

    rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/table_forms_launches.py > tables.jsonl
    python tools/table_forms_launches.py --list DIR/.../*_kernel_trace.csv      # the launches, one per line

Run once with KT_LIB pointing at the parent commit's library and once with this tree's: the two lists and the two sets of
lines must be the same.
"""
import json
import os
import pathlib
import sys

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))
from shard_batch_launches import list_launches  # noqa: E402


def main():
    import torch
    from kmertools_amd import device
    from kmertools_amd._lib import KT_ERR_ARG, KT_MEM_HOST, KmertoolsError
    ctx = device.Context(0, stream=torch.cuda.current_stream().cuda_stream)
    n, L = 6000, 150
    bases = torch.empty(n * L, dtype=torch.uint8, device="cuda")
    offsets = torch.empty(n + 1, dtype=torch.int64, device="cuda")
    ctx.synth_reads(0x666f726d, n, L, bases, offsets, noise=True, genome_len=150000)
    small = (bases[:300 * L], offsets[:301], 300)
    whole = (bases, offsets, n)

    def line(what, keys, counts):
        keys, counts = np.asarray(keys, np.uint64), np.asarray(counts, np.uint32)
        print(json.dumps(dict(export=what, entries=len(keys), sum_of_counts=int(counts.astype(np.uint64).sum()),
                              xor_of_keys=int(np.bitwise_xor.reduce(keys)) if len(keys) else 0)), flush=True)

    def env(bulk):
        os.environ["KT_BULK"] = "1" if bulk else "0"
        os.environ["KT_BULK_MIN_BASES"] = "0"
        os.environ["KT_BULK_MERGE_DIV"] = "1000000000"

    def every_export(c, tag, room):
        """the table's entries by every road, in the form the table is in at each call"""
        dk = torch.zeros(room, dtype=torch.int64, device="cuda")
        dc = torch.zeros(room, dtype=torch.int32, device="cuda")
        for name, max_out in (("device", room), ("device, room for 100", 100), ("device, no room", 0)):
            try:
                got = c.export(dk, dc, max_out)
            except KmertoolsError as e:
                assert e.code == KT_ERR_ARG, e
                got = max_out
            torch.cuda.synchronize()
            if max_out == room:
                line("%s: export %s" % (tag, name), dk[:got].cpu().numpy().view(np.uint64), dc[:got].cpu().numpy().view(np.uint32))
        hk, hc = np.zeros(room, np.uint64), np.zeros(room, np.uint32)
        got = c.export(hk, hc, room, KT_MEM_HOST)
        line("%s: export host" % tag, hk[:got], hc[:got])
        for lo, hi in ((1, None), (2, None), (1, 1), (3, 40)):
            m = c.export_stage_range(lo, hi)
            a = m // 3
            k1, c1 = c.export_fetch(a, m - a)
            k0, c0 = c.export_fetch(0, a)
            line("%s: stage %d..%s" % (tag, lo, hi), np.concatenate([k0, k1]), np.concatenate([c0, c1]))
        c.spectrum(64)

    def lookup(c):
        keys = torch.arange(1, 4097, dtype=torch.int64, device="cuda") * 977
        c.lookup(keys, 4096, torch.zeros(4096, dtype=torch.int32, device="cuda"))
        torch.cuda.synchronize()

    for k in (15, 31):
        room = 1 << 20
        c = device.Counter(ctx, k, 1 << 21)
        every_export(c, "k=%d created" % k, room)
        env(bulk=False)
        c.add_reads(*small)
        every_export(c, "k=%d probing add" % k, room)
        c.clear()
        every_export(c, "k=%d cleared over old data" % k, room)
        env(bulk=True)
        c.add_reads(*whole)
        every_export(c, "k=%d dense" % k, room)
        lookup(c)
        every_export(c, "k=%d dense, imaged" % k, room)
        c.add_reads(*whole)
        every_export(c, "k=%d merged" % k, room)
        env(bulk=False)
        c.add_reads(*small)
        every_export(c, "k=%d probing add on top" % k, room)
        hk, hc = c.export_host()
        c.add_pairs_host(hk[::7], hc[::7])
        assert c.erase(hk[::5]) == len(hk[::5])
        c.add_reads(np.zeros(1, np.uint8), np.zeros(3, np.uint64), 2, KT_MEM_HOST)
        every_export(c, "k=%d pairs added, keys erased" % k, room)
        # into an export target: read where it is, copied elsewhere, filtered, imaged by a prober
        xk = torch.zeros(room, dtype=torch.int64, device="cuda")
        xc = torch.zeros(room, dtype=torch.int32, device="cuda")
        env(bulk=True)
        c.export_target(xk, xc, room)
        c.clear()
        c.add_reads(*whole)
        got = c.export(xk, xc, room)
        torch.cuda.synchronize()
        line("k=%d target: export into the target" % k, xk[:got].cpu().numpy().view(np.uint64), xc[:got].cpu().numpy().view(np.uint32))
        every_export(c, "k=%d target" % k, room)
        lookup(c)
        every_export(c, "k=%d target, imaged" % k, room)
        c.clear()
        c.add_reads(*whole)
        c.export_stage_range(1, None)
        c.export_target(None, None, 0)  # (the table takes its own copy)
        every_export(c, "k=%d target switched off" % k, room)
        # a target too small for the table: the build goes into the slots after all
        c.export_target(xk, xc, 1000)
        c.clear()
        try:
            c.add_reads(*whole)
        except KmertoolsError as e:
            assert e.code == KT_ERR_ARG, e
        every_export(c, "k=%d target too small" % k, room)
        c.close()
    ctx.close()


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--list":
        list_launches(sys.argv[2])
    else:
        main()
