"""Times the MinHash sketch calls on the device.  One process, 3 warm-ups, median of 10 runs between events, per shape:

  sketch      kt_sketch_batch at k = 21, s = 1000 (s = 16 for the short reads), in Gbases/s;
  s = 1       the same call at s = 1 - the front end, the sort and a minimum: the floor of this code's structure;
  minimisers  kt_minimisers with w = 31, m = 7 on the same bases: the nearest existing kernel of the same class;
  numpy       the restatement of the sketch on the host (the k-mers through kt_kmers, hashed, np.unique per sequence), on a
              part of the input when it is large, scaled to the whole.
Shapes: 4 x 20 Mbases, 1 x 80 Mbases (must not be slower than 4 x 20: one sequence has to spread over the device),
100 000 x 5000 bases, 10 M x 150 bases; and kt_sketch_pairs over 10 000 x 10 000 sketches of 1000, in pairs/s.

    python tools/sketch_timing.py [--scale 1.0] [--out profiles/sketch_timing.txt]     (run it twice for the spread)
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
from kmertools_amd import device  # noqa: E402

WARM, REPS = 3, 10
M = np.uint64


def median_ms(fn):
    for _ in range(WARM):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(REPS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms)), float(min(ms)), float(max(ms))


def mix64(z):
    z = z + M(0x9E3779B97F4A7C15)
    z = (z ^ (z >> M(30))) * M(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> M(27))) * M(0x94D049BB133111EB)
    return z ^ (z >> M(31))


def numpy_seconds(ctx, bases, offsets, n, k, s, max_bases=40_000_000):
    """the restatement over the first sequences that hold at most max_bases bases, scaled to the whole input"""
    off = offsets.cpu().numpy().astype(np.uint64)
    m = max(1, int(np.searchsorted(off, max_bases, side="right")) - 1)
    m = min(m, n)
    hb = bases[:int(off[m])].cpu().numpy()
    fwd, rev, idx = ctx.kmers_host(hb, off[:m + 1], k)  # (the k-mers themselves come from the device: only the sketch is timed as numpy)
    t1 = time.perf_counter()
    h = mix64(np.minimum(fwd, rev))
    cut = np.searchsorted(idx, off[:m + 1])
    for i in range(m):
        np.unique(h[cut[i]:cut[i + 1]])[:s]
    t2 = time.perf_counter()
    return (t2 - t1) * float(off[n]) / float(off[m])


def sketch_shape(ctx, name, n, L, s, emit, synth):
    if synth:
        bases = torch.empty(n * L, dtype=torch.uint8, device="cuda")
        offsets = torch.empty(n + 1, dtype=torch.int64, device="cuda")
        ctx.synth_reads(0x5CE7C4, n, L, bases, offsets, noise=True)
    else:
        rng = np.random.default_rng(7)
        bases = torch.from_numpy(np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, size=n * L)]).cuda()
        offsets = torch.arange(0, (n + 1) * L, L, dtype=torch.int64, device="cuda")
    k = 21
    h = torch.empty((n, s), dtype=torch.int64, device="cuda")
    z = torch.empty(n, dtype=torch.int32, device="cuda")
    nk = torch.empty(n, dtype=torch.int32, device="cuda")
    r = dict(what="sketch", shape=name, sequences=n, length=L, k=k, s=s)
    med, lo, hi = median_ms(lambda: ctx.sketch(bases, offsets, n, k, s, h, z, nk))
    r.update(sketch_ms=round(med, 3), sketch_min_ms=round(lo, 3), sketch_max_ms=round(hi, 3), sketch_gbases_per_s=round(n * L / med / 1e6, 3))
    med, _, _ = median_ms(lambda: ctx.sketch(bases, offsets, n, k, 1, h, z, nk))
    r.update(s1_ms=round(med, 3), s1_gbases_per_s=round(n * L / med / 1e6, 3))
    evo = torch.empty(n + 1, dtype=torch.int64, device="cuda")
    dummy = torch.empty(1, dtype=torch.int64, device="cuda")
    cnt = ctx.minimisers(bases, offsets, n, 31, 7, evo, dummy, dummy, dummy, 0)
    mk, ms_, me = (torch.empty(cnt, dtype=torch.int64, device="cuda") for _ in range(3))
    med, _, _ = median_ms(lambda: ctx.minimisers(bases, offsets, n, 31, 7, evo, mk, ms_, me, cnt))
    r.update(minimisers_ms=round(med, 3), minimisers_gbases_per_s=round(n * L / med / 1e6, 3))
    del mk, ms_, me
    sec = numpy_seconds(ctx, bases, offsets, n, k, s)
    r.update(numpy_s=round(sec, 2), numpy_gbases_per_s=round(n * L / sec / 1e9, 4))
    emit(r)
    del bases, offsets, h, z, nk
    torch.cuda.empty_cache()
    return r


def pairs_shape(ctx, n, s, emit):
    g = torch.Generator(device="cuda").manual_seed(3)
    # rows that share hashes: sorted distinct draws from a pool of 4 s values spread over the 63 bits
    pool = torch.sort(torch.randint(0, 2**62, (4 * s,), device="cuda", generator=g, dtype=torch.int64)).values
    pool = torch.unique(pool)
    rows = torch.empty((n, s), dtype=torch.int64, device="cuda")
    for i0 in range(0, n, 1000):
        m = min(1000, n - i0)
        pick = torch.rand((m, pool.numel()), device="cuda", generator=g).argsort(dim=1)[:, :s]
        rows[i0:i0 + m] = torch.sort(pool[pick], dim=1).values
    sizes = torch.full((n,), s, dtype=torch.int32, device="cuda")
    shared = torch.empty((n, n), dtype=torch.int32, device="cuda")
    denom = torch.empty((n, n), dtype=torch.int32, device="cuda")
    med, lo, hi = median_ms(lambda: ctx.sketch_pairs(rows, sizes, n, rows, sizes, n, s, shared, denom))
    r = dict(what="pairs", sketches=n, s=s, pairs_ms=round(med, 3), pairs_min_ms=round(lo, 3), pairs_max_ms=round(hi, 3),
             mpairs_per_s=round(n * n / med / 1e3, 1), mean_shared=round(float(shared.float().mean()), 1))
    # the host beside it: numpy's set operations on a few pairs, scaled
    hr = rows[:8].cpu().numpy().view(np.uint64)
    t0 = time.perf_counter()
    for i in range(8):
        for j in range(8):
            u = np.union1d(hr[i], hr[j])[:s]
            np.isin(np.intersect1d(hr[i], hr[j]), u).sum()
    r["numpy_mpairs_per_s"] = round(64 / (time.perf_counter() - t0) / 1e6, 6)
    emit(r)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0, help="shrinks every shape (a quick look)")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "sketch_timing.txt"))
    args = ap.parse_args()
    try:
        commit = subprocess.run(["git", "-C", str(ROOT), "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip()
    except OSError:
        commit = ""
    lines = ["# tools/sketch_timing.py, commit %s (+ working tree), %s, %d warm-ups, median of %d" % (
        commit or "unknown", torch.cuda.get_device_name(0), WARM, REPS)]

    def emit(r):
        print(json.dumps(r), flush=True)
        lines.append(json.dumps(r))

    sc = args.scale
    ctx = device.Context(0, stream=torch.cuda.current_stream().cuda_stream)
    a = sketch_shape(ctx, "4 x 20 Mbases", 4, int(20_000_000 * sc), 1000, emit, False)
    b = sketch_shape(ctx, "1 x 80 Mbases", 1, int(80_000_000 * sc), 1000, emit, False)
    emit(dict(what="one sequence vs four", ratio_1x80_over_4x20=round(b["sketch_ms"] / a["sketch_ms"], 3),
              spread_4x20=round(a["sketch_max_ms"] / a["sketch_min_ms"], 3), spread_1x80=round(b["sketch_max_ms"] / b["sketch_min_ms"], 3)))
    sketch_shape(ctx, "100 000 x 5000 bases", int(100_000 * sc), 5000, 1000, emit, True)
    sketch_shape(ctx, "10 M x 150 bases", int(10_000_000 * sc), 150, 16, emit, True)
    pairs_shape(ctx, int(10_000 * sc), 1000, emit)
    ctx.close()
    pathlib.Path(args.out).parent.mkdir(exist_ok=True)
    pathlib.Path(args.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
