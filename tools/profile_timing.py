"""Times the k-mer count profile on the device and the `kmertools profile` command end to end.  Three figures:

  profile vs solidity   kt_ctr_profile beside kt_ctr_read_solidity (with first_weak): the same batch (10 M x 150 bp synthetic
                        reads), the same table (of those reads), k = 31 and k = 15, the same process, the calls
                        interleaved, median of --reps runs each (CUDA events).  Same staging, same probes; the profile
                        adds a 4-byte store per base and drops the LDS image.
  stats vs copy         kt_profile_stats beside a device-to-device copy of the same profile array: the short-read
                        form on the 10 M x 150 bp profile, the long form (four histogram passes) on four sequences of
                        20 Mbases; also without the median (one pass).
  cli                   `kmertools profile --positions` on --cli-reads reads with KT_CLI_TIMING=1: where the time goes
                        (the count's phases, then read / device / format / write of the profile pass).

    python tools/profile_timing.py [--reads 10000000] [--reps 9] [--cli-reads 8000000] [--out profiles/profile_timing.txt]
"""
import argparse
import json
import os
import pathlib
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from kmertools_amd import device  # noqa: E402


def interleaved(fns, reps):
    """median ms of each of `fns`, run in turn `reps` times (one warm-up round first)"""
    for fn in fns.values():
        fn()
    torch.cuda.synchronize()
    ms = {name: [] for name in fns}
    for _ in range(reps):
        for name, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            ms[name].append(a.elapsed_time(b))
    return {name: round(float(np.median(v)), 3) for name, v in ms.items()}


def stats_figures(ctx, prof, offsets, n, reps, tag):
    out32 = [torch.empty(n, dtype=torch.int32, device="cuda") for _ in range(5)]
    out64 = torch.empty(n, dtype=torch.int64, device="cuda")
    copy = torch.empty_like(prof)
    r = interleaved({
        "stats_ms": lambda: ctx.profile_stats(prof, offsets, n, *out32, out64),
        "stats_no_median_ms": lambda: ctx.profile_stats(prof, offsets, n, out32[0], out32[1], out32[2], None, out32[4], out64),
        "copy_ms": lambda: copy.copy_(prof),
    }, reps)
    r = dict(what="stats vs copy, " + tag, sequences=n, entries=int(prof.numel()), **r)
    r["stats_over_copy"] = round(r["stats_ms"] / r["copy_ms"], 2)
    r["stats_no_median_over_copy"] = round(r["stats_no_median_ms"] / r["copy_ms"], 2)
    return r


def device_figures(ctx, n, L, reps, emit):
    bases = torch.empty(n * L, dtype=torch.uint8, device="cuda")
    offsets = torch.empty(n + 1, dtype=torch.int64, device="cuda")
    ctx.synth_reads(0x6b6d6572 + 5, n, L, bases, offsets, noise=True, genome_len=20_000_000)
    prof = torch.full((n * L,), -1, dtype=torch.int32, device="cuda")
    nk = torch.zeros(n, dtype=torch.int32, device="cuda")
    ns = torch.zeros(n, dtype=torch.int32, device="cuda")
    fw = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    for k in (31, 15):
        kpr = L - k + 1
        max_distinct = min(n * kpr, (4 ** k + 2 ** k) // 2)
        ctr = device.Counter(ctx, k, 1 << max(20, (2 * max_distinct - 1).bit_length()) if k <= 15 else int(1.9 * max_distinct))
        ctr.add_reads(bases, offsets, n)
        r = interleaved({
            "profile_ms": lambda: ctr.profile(bases, offsets, n, prof),
            "solidity_ms": lambda: ctr.read_solidity(bases, offsets, n, 2, 0xFFFFFFFF, nk, ns, fw),
        }, reps)
        r = dict(what="profile vs solidity", k=k, reads=n, read_len=L, capacity=ctr.capacity(), distinct=ctr.size(), **r)
        r["profile_over_solidity"] = round(r["profile_ms"] / r["solidity_ms"], 3)
        emit(r)
        if k == 31:
            prof.fill_(-1)
            ctr.profile(bases, offsets, n, prof)
            emit(stats_figures(ctx, prof, offsets, n, reps, "%d x %d bp (k = 31)" % (n, L)))
        ctr.close()
    del bases, offsets, prof, nk, ns, fw
    torch.cuda.empty_cache()
    # four sequences of 20 Mbases (tools/min_wide_timing.py's), profiled against their own k = 31 table
    n, L, k = 4, 20_000_000, 31
    g = torch.Generator(device="cuda").manual_seed(7)
    bases = torch.tensor(list(b"ACGT"), dtype=torch.uint8, device="cuda")[torch.randint(0, 4, (n * L,), device="cuda", generator=g)]
    offsets = torch.arange(0, (n + 1) * L, L, dtype=torch.int64, device="cuda")
    ctr = device.Counter(ctx, k, int(1.9 * n * L))
    ctr.add_reads(bases, offsets, n)
    ctr.add_reads(bases, offsets, 2)  # (counts 1 and 2)
    prof = torch.full((n * L,), -1, dtype=torch.int32, device="cuda")
    ctr.profile(bases, offsets, n, prof)
    emit(stats_figures(ctx, prof, offsets, n, reps, "4 x 20 Mbases (k = 31)"))
    ctr.close()
    del bases, offsets, prof
    torch.cuda.empty_cache()


def cli_figure(n, L, emit):
    cli = ROOT / "kmertools_amd" / "bin" / "kmertools"
    tmp = pathlib.Path(os.environ.get("TMPDIR", "/tmp")) / "kt_profile_timing"
    tmp.mkdir(exist_ok=True)
    fa = tmp / "reads.fa"
    rng = np.random.default_rng(1)
    genome = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, size=20_000_000)]
    starts = rng.integers(0, len(genome) - L, size=n)
    rec = np.empty((n, L + 12), np.uint8)  # ">" + 9-digit id + "\n" + L bases + "\n" (tools/cli_e2e.py's file)
    rec[:, 0] = ord(">")
    rec[:, 1:10] = np.frombuffer("".join(np.char.zfill(np.arange(n).astype(str), 9)).encode(), np.uint8).reshape(n, 9)
    rec[:, 10] = ord("\n")
    rec[:, 11:11 + L] = genome[starts[:, None] + np.arange(L)[None, :]]
    rec[:, 11 + L] = ord("\n")
    fa.write_bytes(rec.tobytes())
    del rec
    env = dict(os.environ, KT_CLI_TIMING="1")
    for name, extra in (("profile k=31", []), ("profile k=31 --positions", ["--positions"])):
        out = tmp / "out"
        t0 = time.perf_counter()
        r = subprocess.run([str(cli), "profile", "-i", str(fa), "-o", str(out), "-k", "31"] + extra, env=env, capture_output=True, text=True)
        dt = time.perf_counter() - t0
        sizes = {f.name: round(f.stat().st_size / 1e6, 1) for f in out.glob("*")} if out.exists() else {}
        emit(dict(what="cli", command=name, reads=n, read_len=L, seconds=round(dt, 2), gbases_per_s=round(n * L / dt / 1e9, 3),
                  rc=r.returncode, output_mb=sizes, timing=[ln for ln in r.stderr.splitlines()]))
        for f in out.glob("*"):
            f.unlink()
    fa.unlink()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=10_000_000)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--cli-reads", type=int, default=8_000_000, help="0: skip the command line figure")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "profile_timing.txt"))
    args = ap.parse_args()
    try:
        commit = subprocess.run(["git", "-C", str(ROOT), "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip()
    except OSError:
        commit = ""
    lines = ["# tools/profile_timing.py, commit %s (+ working tree), %s" % (commit or "unknown", torch.cuda.get_device_name(0))]

    def emit(r):
        print(json.dumps(r), flush=True)
        lines.append(json.dumps(r))

    ctx = device.Context(0, stream=torch.cuda.current_stream().cuda_stream)
    device_figures(ctx, args.reads, 150, args.reps, emit)
    ctx.close()
    if args.cli_reads:
        cli_figure(args.cli_reads, 150, emit)
    pathlib.Path(args.out).parent.mkdir(exist_ok=True)
    pathlib.Path(args.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
