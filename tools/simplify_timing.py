"""Times bubble popping on the device beside tip clipping, on tools/clip_tips_timing.py's table (bench.py's genome-sampled
ctr_k31, scaled): the read-only kt_ctr_unitig_tips and kt_ctr_unitig_bubbles, one clip round (kt_ctr_clip_tips, max_rounds 1),
one bubble-only round and one round with both rules (kt_ctr_simplify, max_rounds 1), and the whole kt_ctr_simplify.  One
process, events on the context's stream round each call, warm-ups first, the median of --reps with minimum and maximum.  A
round changes the table, so every repeat of one starts from the table counted again (kt_ctr_clear, kt_ctr_add_reads).

    python tools/simplify_timing.py [--scale 0.04] [--reps 3] [--out profiles/simplify_timing.txt]

--tips-only times kt_ctr_unitig_tips and the clip round alone and needs none of the new calls in the library: with KT_LIB
pointing at a build from before them, in a process of its own, it gives the figures this build's are set beside.  Its default
output is profiles/simplify_timing_tips_only.txt, so that it does not overwrite the full run's file.  --label names the
library in the output ("this build", "parent commit"); without it the path relative to the repository is written.

The committed profiles/simplify_timing.txt is put together from several runs: the two lines the full run writes; under a
comment line, the JSON line of each --tips-only process, the parent commit's library and this build alternately; under another,
the rows of unitig_tip_class_kernel, unitig_tip_mark_kernel, unitig_bubble_mark_kernel and unitig_tip_list_kernel from the
kernel stats of one `rocprofv3 --kernel-trace --stats` run of the full script (--reps 1) on its own.
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
sys.path.insert(0, str(ROOT / "tools"))
from kmertools_amd import _lib, device  # noqa: E402
from clip_tips_timing import CFG, GENOME, LENGTH, READS, SEED, once, timed  # noqa: E402


def spread(ms):
    return dict(median_ms=round(float(np.median(ms)), 3), min_ms=round(min(ms), 3), max_ms=round(max(ms), 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=0.04, help="of bench.py's reads and genome")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--tips-only", action="store_true")
    ap.add_argument("--label", default="", help="names the library in the output instead of its path")
    ap.add_argument("--out", default="", help="default: profiles/simplify_timing.txt, with --tips-only profiles/simplify_timing_tips_only.txt")
    args = ap.parse_args()
    out = args.out or str(ROOT / "profiles" / ("simplify_timing_tips_only.txt" if args.tips_only else "simplify_timing.txt"))
    if args.tips_only:
        for name in ("kt_ctr_unitig_bubbles", "kt_ctr_simplify"):
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
    t = device.Counter(ctx, k, max(1 << 20, int(1.9 * n * (L - k + 1))))

    def counted():
        t.clear()
        t.add_reads(bases, offsets, n)
        return t.size()

    entries = counted()
    lib_path = pathlib.Path(_lib.LIB_PATH).resolve()
    r = dict(scale=args.scale, genome=genome, reads=n, length=L, k=k, entries=entries, slots=t.capacity(),
             library=args.label or (str(lib_path.relative_to(ROOT)) if ROOT in lib_path.parents else lib_path.name))
    nu = t.unitig_tips_device(None, 0)
    r["unitigs"] = nu
    marks = torch.empty(nu, dtype=torch.uint8, device="cuda")
    tally = torch.zeros(4, dtype=torch.int64, device="cuda")
    r["unitig_tips"] = timed(lambda: t.unitig_tips_device(marks, nu, tally), 1, args.reps)
    r["tip_tally"] = tally.cpu().numpy().tolist()

    def rounds_of(fn):
        """fn on the freshly counted table, a warm-up and --reps repeats -> (the spread, the last result)"""
        ms, out = [], None
        for i in range(args.reps + 1):
            counted()
            torch.cuda.synchronize()
            ms1, out = once(fn)
            if i:
                ms.append(ms1)
        return spread(ms), out

    r["clip_round"], r["clip_round_stats"] = rounds_of(lambda: t.clip_tips(max_rounds=1))
    if not args.tips_only:
        counted()
        r["unitig_bubbles"] = timed(lambda: t.unitig_bubbles_device(marks, nu, tally), 1, args.reps)
        r["bubble_tally"] = tally.cpu().numpy().tolist()
        r["bubble_round"], r["bubble_round_stats"] = rounds_of(lambda: t.simplify(0, None, 1))
        r["both_round"], r["both_round_stats"] = rounds_of(lambda: t.simplify(None, None, 1))
        r["both_over_clip_plus_bubble"] = round(r["both_round"]["median_ms"] /
                                                (r["clip_round"]["median_ms"] + r["bubble_round"]["median_ms"]), 3)
        counted()
        r["simplify_ms"], r["simplify_stats"] = once(lambda: t.simplify(None, None, 64))
        r["entries_after"] = t.size()
        r["unitigs_after"] = t.unitig_tips_device(None, 0)
    print(json.dumps(r), flush=True)
    t.close()
    ctx.close()
    head = "# tools/simplify_timing.py, commit %s (+ working tree), %s, events round each call" % (
        commit or "unknown", torch.cuda.get_device_name(0))
    pathlib.Path(out).parent.mkdir(exist_ok=True)
    pathlib.Path(out).write_text(head + "\n" + json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
