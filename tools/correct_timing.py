"""Times read error correction on the device and the `kmertools correct` command end to end.  Three figures:

  support vs profile    kt_ctr_correct_support beside kt_ctr_profile: the same batch (10 M x 150 bp noisy synthetic reads), the
                        same table (of those reads), k = 31 and k = 15, the same process, the calls interleaved, median of
                        --reps runs each (CUDA events) - with the number of table probes each makes, i.e. the time per
                        probe.  Both probe with random 16-byte reads; the profile issues them from a regular walk (one per
                        window start), the support kernel from a compacted list of (window, uncovered base) pairs, three
                        each (four where the base is an N).  With KT_LIB set to another build of the library that has these
                        calls, that build is measured.
  apply vs copy         kt_correct_apply (counts and corrected bases) beside a device-to-device copy of bases + support,
                        the bytes it reads.
  cli                   `kmertools correct` on --cli-reads reads with KT_CLI_TIMING=1, beside `kmertools filter` on the
                        same file.

    python tools/correct_timing.py [--reads 10000000] [--reps 9] [--cli-reads 8000000] [--out profiles/correct_timing.txt]
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


def probe_counts(bases, prof, n, L, k, lo):
    """table probes of the two calls on n reads of L bases: the profile's valid windows; the support call's three per (window
    of one read, uncovered base in it) where every other base is valid, four where the base itself is not a nucleotide"""
    valid = torch.zeros(256, dtype=torch.bool, device="cuda")
    valid[torch.tensor(list(b"ACGTUacgtu\x00\x01\x02\x03"), device="cuda")] = True
    inv = (~valid[bases.view(n, L).long()]).to(torch.int32)
    solid = ((prof != -1) & (prof >= lo)).view(n, L).to(torch.int32)
    pad = torch.nn.functional.pad
    g = torch.arange(L, device="cuda")
    c = pad(torch.cumsum(solid, dim=1), (1, 0))
    unc = ((c[:, g + 1] - c[:, torch.clamp(g - k + 1, min=0)]) == 0).to(torch.int32)
    j = torch.arange(L - k + 1, device="cuda")
    cu, ci = pad(torch.cumsum(unc, dim=1), (1, 0)), pad(torch.cumsum(inv, dim=1), (1, 0))
    n_unc, n_inv = cu[:, j + k] - cu[:, j], ci[:, j + k] - ci[:, j]
    clean = int(torch.where(n_inv == 0, n_unc, torch.zeros_like(n_unc)).sum())
    one_n = int((n_inv == 1).sum())
    return int((prof != -1).sum()), 3 * clean + 4 * one_n, int(unc.sum())


def device_figures(ctx, n, L, reps, emit):
    bases = torch.empty(n * L, dtype=torch.uint8, device="cuda")
    offsets = torch.empty(n + 1, dtype=torch.int64, device="cuda")
    ctx.synth_reads(0x6b6d6572 + 5, n, L, bases, offsets, noise=True, genome_len=20_000_000)
    prof = torch.full((n * L,), -1, dtype=torch.int32, device="cuda")
    sup = torch.zeros(n * L, dtype=torch.int32, device="cuda")
    lo = 2
    for k in (31, 15):
        kpr = L - k + 1
        max_distinct = min(n * kpr, (4 ** k + 2 ** k) // 2)
        ctr = device.Counter(ctx, k, 1 << max(20, (2 * max_distinct - 1).bit_length()) if k <= 15 else int(1.9 * max_distinct))
        ctr.add_reads(bases, offsets, n)
        prof.fill_(-1)
        ctr.profile(bases, offsets, n, prof)
        r = interleaved({
            "profile_ms": lambda: ctr.profile(bases, offsets, n, prof),
            "support_ms": lambda: ctr.correct_support(bases, offsets, n, prof, lo, 0xFFFFFFFF, sup),
        }, reps)
        p_probes, s_probes, uncovered = probe_counts(bases, prof, n, L, k, lo)
        r = dict(what="support vs profile", k=k, reads=n, read_len=L, capacity=ctr.capacity(), distinct=ctr.size(), min_count=lo,
                 uncovered_bases=uncovered, profile_probes=p_probes, support_probes=s_probes, **r)
        r["profile_ns_per_probe"] = round(r["profile_ms"] * 1e6 / p_probes, 4)
        r["support_ns_per_probe"] = round(r["support_ms"] * 1e6 / max(s_probes, 1), 4)
        r["support_over_profile_per_probe"] = round(r["support_ns_per_probe"] / r["profile_ns_per_probe"], 2)
        emit(r)
        if k == 31:
            sup.zero_()
            ctr.correct_support(bases, offsets, n, prof, lo, 0xFFFFFFFF, sup)
            out = torch.empty_like(bases)
            ns = torch.empty(n, dtype=torch.int32, device="cuda")
            na = torch.empty(n, dtype=torch.int32, device="cuda")
            cb, cs = torch.empty_like(bases), torch.empty_like(sup)

            def copy():
                cb.copy_(bases)
                cs.copy_(sup)

            a = interleaved({
                "apply_ms": lambda: ctx.correct_apply(bases, offsets, n, sup, 1, 0, out, ns, na),
                "apply_limit_ms": lambda: ctx.correct_apply(bases, offsets, n, sup, 1, 2, out, ns, na),
                "apply_bases_only_ms": lambda: ctx.correct_apply(bases, offsets, n, sup, 1, 0, out, None, None),
                "copy_ms": copy,
            }, reps)
            a = dict(what="apply vs copy of bases + support", reads=n, read_len=L, bases_corrected=int(ns.sum()),
                     positions_ambiguous=int(na.sum()), **a)
            a["apply_over_copy"] = round(a["apply_ms"] / a["copy_ms"], 2)
            emit(a)
            del out, ns, na, cb, cs
        ctr.close()
    del bases, offsets, prof, sup
    torch.cuda.empty_cache()


def cli_figure(n, L, emit):
    cli = ROOT / "kmertools_amd" / "bin" / "kmertools"
    tmp = pathlib.Path(os.environ.get("TMPDIR", "/tmp")) / "kt_correct_timing"
    tmp.mkdir(exist_ok=True)
    fa = tmp / "reads.fa"
    rng = np.random.default_rng(1)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    genome = rng.integers(0, 4, size=20_000_000).astype(np.uint8)
    starts = rng.integers(0, len(genome) - L, size=n)
    rec = np.empty((n, L + 12), np.uint8)  # ">" + 9-digit id + "\n" + L bases + "\n" (tools/cli_e2e.py's file)
    rec[:, 0] = ord(">")
    rec[:, 1:10] = np.frombuffer("".join(np.char.zfill(np.arange(n).astype(str), 9)).encode(), np.uint8).reshape(n, 9)
    rec[:, 10] = ord("\n")
    step = 1 << 20
    for a in range(0, n, step):  # 1 % substitutions
        codes = genome[starts[a:a + step, None] + np.arange(L)[None, :]]
        err = rng.random(codes.shape) < 0.01
        codes = (codes + err * rng.integers(1, 4, size=codes.shape)) & 3
        rec[a:a + step, 11:11 + L] = acgt[codes]
    rec[:, 11 + L] = ord("\n")
    fa.write_bytes(rec.tobytes())
    del rec
    env = dict(os.environ, KT_CLI_TIMING="1")
    for name in ("correct", "filter"):
        out = tmp / "out.fa"
        t0 = time.perf_counter()
        r = subprocess.run([str(cli), name, "-i", str(fa), "-o", str(out), "-k", "31"], env=env, capture_output=True, text=True)
        dt = time.perf_counter() - t0
        emit(dict(what="cli", command=name + " k=31", reads=n, read_len=L, seconds=round(dt, 2), gbases_per_s=round(n * L / dt / 1e9, 3),
                  rc=r.returncode, output_mb=round(out.stat().st_size / 1e6, 1) if out.exists() else None,
                  timing=[ln for ln in r.stderr.splitlines()]))
        if out.exists():
            out.unlink()
    fa.unlink()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=10_000_000)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--cli-reads", type=int, default=8_000_000, help="0: skip the command line figure")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "correct_timing.txt"))
    args = ap.parse_args()
    try:
        commit = subprocess.run(["git", "-C", str(ROOT), "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip()
    except OSError:
        commit = ""
    lines = ["# tools/correct_timing.py, commit %s (+ working tree), %s" % (commit or "unknown", torch.cuda.get_device_name(0))]

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
