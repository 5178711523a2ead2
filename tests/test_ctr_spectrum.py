"""The counter's abundance spectrum (kt_ctr_spectrum) and count-range export (kt_ctr_export_stage_range) in every form a
table can be in - the probing image, the dense ranges of a bulk build, an export target's arrays, the direct-addressed
k <= 15 build - against the oracle's table (its counts binned with saturation), plus passes, shards and the CLI's
--histo / --min-count / --max-count / --histo-only."""
import ctypes as C
import os
import subprocess
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "kmertools_amd", "bin", "kmertools")
U32_MAX = 0xFFFFFFFF


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    return torch


@pytest.fixture(scope="module")
def ctx(torch_mod):
    from kmertools_amd import device
    c = device.Context(0, stream=torch_mod.cuda.current_stream().cuda_stream)
    yield c
    c.close()


def want_spectrum(counts, n_bins):
    h = np.bincount(np.minimum(counts.astype(np.int64), n_bins - 1), minlength=n_bins).astype(np.uint64)
    h[0] = 0
    return h


def reads(seed, n, max_len=600):
    rng = np.random.default_rng(seed)
    alpha = np.frombuffer(b"ACGTN", np.uint8)
    seqs = [alpha[rng.choice(5, size=int(L), p=[.2475, .2475, .2475, .2475, .01])].tobytes()
            for L in rng.integers(0, max_len, size=n)]
    seqs += [b"A" * 2500, b"ACGT" * 300, b"ACGGT" * 200] + seqs[: n // 5]  # heavy hitters and repeats
    return seqs


def check_table(ctr, wk, wc, tag):
    """spectrum + totals, and the filtered stage for several ranges; the table is unchanged afterwards"""
    for n_bins in (2, 7, 10001):
        hist, (d, occ) = ctr.spectrum(n_bins, totals=True)
        assert np.array_equal(hist, want_spectrum(wc, n_bins)), (tag, n_bins)
        assert d == len(wk) and occ == int(wc.astype(np.uint64).sum()), tag
    top = int(wc.max()) if len(wc) else 0
    for lo, hi in ((1, 1), (2, None), (3, 7), (top + 1, None), (1, None), (2, 2)):
        n = ctr.export_stage_range(lo, hi)
        gk, gc = ctr.export_fetch(0, n)
        order = np.argsort(gk, kind="stable")
        sel = (wc >= lo) & (wc <= (U32_MAX if hi is None else hi))
        assert np.array_equal(gk[order], wk[sel]) and np.array_equal(gc[order], wc[sel]), (tag, lo, hi)
    assert ctr.size() == len(wk), tag
    gk, gc = ctr.export_host()
    assert np.array_equal(gk, wk) and np.array_equal(gc, wc), tag
    gk, gc = ctr.export_host(min_count=3, max_count=7)
    sel = (wc >= 3) & (wc <= 7)
    assert np.array_equal(gk, wk[sel]) and np.array_equal(gc, wc[sel]), tag


@pytest.mark.parametrize("k", [11, 15, 21, 31])
def test_spectrum_and_filtered_stage_in_every_form(torch_mod, ctx, oracle, monkeypatch, k):
    torch = torch_mod
    from kmertools_amd import device
    from kmertools_amd.device import to_csr
    seqs = reads(100 + k, 1500)
    bases, offsets = to_csr(seqs)
    wk, wc = oracle.count_reads(bases, offsets, k)
    cap = max(1 << 16, 2 * len(wk))
    # the probing image: (key, count) pairs through the atomic path
    ctr = device.Counter(ctx, k, cap)
    ctr.add_pairs_host(wk, wc)
    check_table(ctr, wk, wc, ("probing", k))
    ctr.add_pairs_host(wk, wc)  # a later add behaves as before
    assert np.array_equal(ctr.export_host()[1], 2 * wc)
    ctr.close()
    # the dense ranges of a fresh bulk build
    monkeypatch.setenv("KT_BULK_MIN_BASES", "0")
    ctr = device.Counter(ctx, k, cap)
    ctr.add_reads_host(bases, offsets)
    check_table(ctr, wk, wc, ("dense", k))
    ctr.add_reads_host(bases, offsets)
    assert np.array_equal(ctr.export_host()[1], 2 * wc)
    ctr.close()
    # an export target's arrays (one entry of offset: the counts start off a 16-byte boundary)
    m = len(wk) + 9
    xk = torch.zeros(m + 1, dtype=torch.int64, device="cuda")
    xc = torch.zeros(m + 1, dtype=torch.int32, device="cuda")
    ctr = device.Counter(ctx, k, cap)
    ctr.export_target(xk[1:], xc[1:], m)
    db = torch.from_numpy(bases).cuda()
    do = torch.from_numpy(offsets.astype(np.int64)).cuda()
    ctr.add_reads(db, do, len(seqs))
    before = (xk.clone(), xc.clone())
    check_table(ctr, wk, wc, ("export target", k))
    assert torch.equal(before[0], xk) and torch.equal(before[1], xc)  # the target's arrays are not touched
    ctr.close()
    # the direct-addressed build: exactly 4^k slots (k <= 13 here; k = 15 at full size below)
    if k <= 13:
        ctr = device.Counter(ctx, k, 4 ** k)
        assert ctr.capacity() == 4 ** k
        ctr.add_reads_host(bases, offsets)
        check_table(ctr, wk, wc, ("direct", k))
        assert np.array_equal(ctr.lookup_host(wk[:100]), wc[:100])
        ctr.close()


def test_spectrum_bins_edges_and_accumulation(torch_mod, ctx, oracle, monkeypatch):
    torch = torch_mod
    from kmertools_amd import device
    from kmertools_amd._lib import lib
    k = 21
    rng = np.random.default_rng(5)
    keys = np.unique(rng.integers(0, 1 << 40, size=30000, dtype=np.uint64))
    counts = rng.integers(1, 9000, size=len(keys)).astype(np.uint32)
    counts[:3000] = 1
    counts[3000:5000] = 2
    counts[7] = (1 << 21) + 5  # a flood of one k-mer
    ctr = device.Counter(ctx, k, 1 << 17)
    # empty table: nothing is added
    h, (d, occ) = ctr.spectrum(10, totals=True)
    assert not h.any() and d == 0 and occ == 0
    ctr.add_pairs_host(keys, counts)
    order = np.argsort(keys)
    wk, wc = keys[order], counts[order]
    for n_bins in (2, 3, 4096, 4097, 5000, 1 << 22):  # below, at and above the LDS bins; the flood's own bin
        hist = ctr.spectrum(n_bins)
        assert np.array_equal(hist, want_spectrum(wc, n_bins)), n_bins
    # device arrays, accumulated over two calls (hist[0] untouched)
    dh = torch.full((5001,), 0, dtype=torch.int64, device="cuda")
    dh[0] = 12345
    dt = torch.zeros(2, dtype=torch.int64, device="cuda")
    for _ in range(2):
        ctr.spectrum_into(dh, 5001, dt)
    torch.cuda.synchronize()
    got = dh.cpu().numpy().view(np.uint64)
    want = 2 * want_spectrum(wc, 5001)
    want[0] = 12345
    assert np.array_equal(got, want)
    assert dt.cpu().tolist() == [2 * len(wk), 2 * int(wc.astype(np.int64).sum())]
    # host arrays accumulate too
    hh = np.zeros(100, np.uint64)
    ht = np.zeros(2, np.uint64)
    for _ in range(3):
        assert lib().kt_ctr_spectrum(ctr._h, hh.ctypes.data, 100, ht.ctypes.data, 0) == 0
    assert np.array_equal(hh, 3 * want_spectrum(wc, 100)) and ht.tolist() == [3 * len(wk), 3 * int(wc.astype(np.int64).sum())]
    n = ctr.export_stage_range((1 << 21) + 5, (1 << 21) + 5)
    assert n == 1 and ctr.export_fetch(0, 1)[0][0] == keys[7]
    ctr.close()


def test_spectrum_errors(ctx):
    from kmertools_amd import device
    from kmertools_amd._lib import lib
    ctr = device.Counter(ctx, 21, 1024)
    h = np.zeros((1 << 24) + 1, np.uint64)
    for bad in (0, 1, (1 << 24) + 1):
        assert lib().kt_ctr_spectrum(ctr._h, h.ctypes.data, bad, None, 0) == 1  # KT_ERR_ARG
    assert lib().kt_ctr_spectrum(ctr._h, h.ctypes.data, 1 << 24, None, 0) == 0
    n = C.c_uint64()
    assert lib().kt_ctr_export_stage_range(ctr._h, 3, 2, C.byref(n)) == 1
    from kmertools_amd._lib import KmertoolsError
    with pytest.raises(KmertoolsError):
        ctr.export_stage_range(9, 8)
    # an overflowed table (far more distinct keys than slots): KT_ERR_FULL, as kt_ctr_size
    ctr.add_pairs_host(np.arange(1, 5000, dtype=np.uint64) * 7919, np.ones(4999, np.uint32))
    assert lib().kt_ctr_spectrum(ctr._h, h.ctypes.data, 16, None, 0) == 4
    assert lib().kt_ctr_export_stage_range(ctr._h, 2, 5, C.byref(n)) == 4
    ctr.close()


def test_spectrum_passes_add_up(ctx, oracle):
    from kmertools_amd import device
    from kmertools_amd.device import to_csr
    seqs = reads(7, 2000)
    bases, offsets = to_csr(seqs)
    wk, wc = oracle.count_reads(bases, offsets, 25)
    ctr = device.Counter(ctx, 25, len(wk))  # room for a third of the distinct k-mers and more
    hist = np.zeros(50, np.uint64)
    tot = np.zeros(2, np.uint64)
    from kmertools_amd._lib import lib
    kept = []
    for part in range(3):
        ctr.clear()
        ctr.add_reads_host(bases, offsets, 3, part)
        assert lib().kt_ctr_spectrum(ctr._h, hist.ctypes.data, 50, tot.ctypes.data, 0) == 0
        kept.append(ctr.export_host(min_count=2, max_count=9))
    assert np.array_equal(hist, want_spectrum(wc, 50))
    assert tot.tolist() == [len(wk), int(wc.astype(np.int64).sum())]
    gk = np.concatenate([k_ for k_, _ in kept])
    gc = np.concatenate([c_ for _, c_ in kept])
    order = np.argsort(gk)
    sel = (wc >= 2) & (wc <= 9)
    assert np.array_equal(gk[order], wk[sel]) and np.array_equal(gc[order], wc[sel])
    ctr.close()


def _run_ranks(n_ranks, k, bases, offsets, n_bins):
    """n_ranks host-transport ranks of one sharded counter on the one GPU, one thread each; returns the summed spectrum
    and the union of every shard's filtered entries"""
    from kmertools_amd import device
    barrier = threading.Barrier(n_ranks, timeout=120)
    sends = [0] * n_ranks

    def alltoall_for(rank):
        def fn(send, recv, nbytes):
            try:
                sends[rank] = send
                barrier.wait()
                for p in range(n_ranks):
                    C.memmove(recv + p * nbytes, sends[p] + rank * nbytes, nbytes)
                barrier.wait()
                return 0
            except Exception:
                barrier.abort()
                return 1
        return fn

    n = len(offsets) - 1
    per = (n + n_ranks - 1) // n_ranks
    out, errs = [None] * n_ranks, [None] * n_ranks

    def worker(rank):
        try:
            c = device.Context(0)
            sh = device.Sharded(c, k, 1 << 20, int(offsets[-1]) + 1, n_ranks, rank, ("host", alltoall_for(rank)))
            lo, hi = min(n, rank * per), min(n, (rank + 1) * per)
            o = offsets[lo:hi + 1] - offsets[lo]
            sh.add_reads_host(bases[int(offsets[lo]):int(offsets[hi])], o)
            sh.finalize()
            h, t = sh.table.spectrum(n_bins, totals=True)
            out[rank] = (h, t, sh.table.export_host(min_count=2, max_count=9))
            sh.close()
            c.close()
        except Exception as e:  # (reported below; the barrier is broken so that no peer waits for ever)
            errs[rank] = e
            barrier.abort()

    threads = [threading.Thread(target=worker, args=(r,)) for r in range(n_ranks)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(300)
    assert not any(t.is_alive() for t in threads)
    assert not any(errs), errs
    hist = sum(o[0] for o in out)
    tot = (sum(o[1][0] for o in out), sum(o[1][1] for o in out))
    gk = np.concatenate([o[2][0] for o in out])
    gc = np.concatenate([o[2][1] for o in out])
    order = np.argsort(gk)
    return hist, tot, gk[order], gc[order]


def test_spectrum_shards_add_up(ctx, oracle):
    from kmertools_amd.device import to_csr
    seqs = reads(11, 1200)
    bases, offsets = to_csr(seqs)
    k = 23
    wk, wc = oracle.count_reads(bases, offsets, k)
    sel = (wc >= 2) & (wc <= 9)
    for n_ranks in (2, 3):
        hist, tot, gk, gc = _run_ranks(n_ranks, k, bases, offsets, 40)
        assert np.array_equal(hist, want_spectrum(wc, 40)), n_ranks
        assert tot == (len(wk), int(wc.astype(np.int64).sum()))
        assert np.array_equal(gk, wk[sel]) and np.array_equal(gc, wc[sel]), n_ranks


def test_spectrum_direct_k15_full_size(torch_mod, ctx, oracle):
    """the k = 15 direct-addressed table at the benchmark's request of 1.9 x 2^29 slots (2^30 slots, 16 GB): the sums of
    the spectrum against the table's size and the reads' k-mers, the saturated bin against the filtered stage, and a
    sub-batch in the same table against the oracle"""
    torch = torch_mod
    from kmertools_amd import device
    k, n, L, seed = 15, 4_000_000, 150, 0x5eed
    bases = torch.empty(n * L, dtype=torch.uint8, device="cuda")
    offsets = torch.empty(n + 1, dtype=torch.int64, device="cuda")
    ctx.synth_reads(seed, n, L, bases, offsets)
    ctr = device.Counter(ctx, k, int(1.9 * 2 ** 29))
    assert ctr.capacity() == 4 ** k
    ctr.add_reads(bases, offsets, n)
    H = 10001
    hist, (d, occ) = ctr.spectrum(H, totals=True)
    assert d == ctr.size() and int(hist.sum()) == d
    assert occ == n * (L - k + 1)
    ns = ctr.export_stage_range(H - 1, None)
    sk, sc = ctr.export_fetch(0, ns)
    assert ns == int(hist[H - 1])
    c = np.arange(H, dtype=np.uint64)
    assert int((c[:-1] * hist[:-1]).sum()) + int(sc.astype(np.uint64).sum()) == occ
    # filtered stage of the dense direct table against the spectrum
    assert ctr.export_stage_range(1, 1) == int(hist[1])
    assert ctr.export_stage_range(2, 5) == int(hist[2:6].sum())
    # a sub-batch of the same reads into the same (cleared) table, against the oracle
    m = 20000
    hb = bases[: m * L].cpu().numpy()
    ho = np.arange(m + 1, dtype=np.uint64) * L
    wk, wc = oracle.count_reads(hb, ho, k)
    ctr.clear()
    ctr.add_reads(bases[: m * L], offsets[: m + 1], m)
    check_table(ctr, wk, wc, "k15 full-size table, sub-batch")
    ctr.close()
    del bases, offsets
    torch.cuda.empty_cache()


# ---- the CLI --------------------------------------------------------------------------------------------------------

def run(*args, env=None):
    return subprocess.run([CLI, *map(str, args)], capture_output=True, text=True, timeout=300, env=env)


def histo_text(counts, H):
    h = want_spectrum(counts, H + 1)
    return "".join("%d\t%d\n" % (c, h[c]) for c in range(1, H + 1))


def test_ctr_cli_histo_and_count_range(oracle, tmp_path):
    if not os.path.exists(CLI):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "kmertools_amd", "csrc"), "-j4"], stdout=subprocess.DEVNULL)
    seqs = [s.decode() for s in reads(23, 4000)]
    fq = tmp_path / "r.fastq"
    fq.write_text("".join("@s%d\n%s\n+\n%s\n" % (i, s, "I" * len(s)) for i, s in enumerate(seqs)))
    bases, offsets = oracle.to_csr(seqs)
    keys, counts = oracle.count_reads(bases, offsets, 21, n_parts=4, threads=4)
    all_lines = oracle.counts_lines(keys, counts)
    sel = (counts >= 2) & (counts <= 9)
    kept_lines = oracle.counts_lines(keys[sel], counts[sel])
    env = dict(os.environ, KT_CLI_TIMING="1")
    # without the new flags: the oracle's lines and no kmers.histo
    d0 = tmp_path / "plain"
    r = run("ctr", "-i", fq, "-o", d0, "-k", "21", env=env)
    assert r.returncode == 0, r.stderr
    assert sorted((d0 / "kmers.counts").read_text().splitlines()) == all_lines
    assert not (d0 / "kmers.histo").exists()
    small = str(max(1024, int(1.4 * len(keys) / 4)))
    for tag, extra_env, extra in (("one", {}, ()), ("passes", {"KT_CTR_MAX_SLOTS": small}, ()),
                                  ("dev2", {"KT_CLI_SHARE_GPU": "1"}, ("--devices", "2")),
                                  ("dense", {"KT_BULK_MIN_BASES": "0"}, ())):
        e = dict(env, **extra_env)
        d = tmp_path / tag
        r = run("ctr", "-i", fq, "-o", d, "-k", "21", "--histo", "--histo-max", "50", "--min-count", "2", "--max-count", "9",
                *extra, env=e)
        assert r.returncode == 0, (tag, r.stderr)
        if tag == "passes":
            assert int(r.stderr.split(" pass(es)")[0].split()[-1]) >= 4
        assert (d / "kmers.histo").read_text() == histo_text(counts, 50), tag
        assert sorted((d / "kmers.counts").read_text().splitlines()) == kept_lines, tag
        d2 = tmp_path / (tag + "_only")
        r = run("ctr", "-i", fq, "-o", d2, "-k", "21", "--histo-only", *extra, env=e)
        assert r.returncode == 0, (tag, r.stderr)
        assert (d2 / "kmers.histo").read_text() == histo_text(counts, 10000), tag
        assert not (d2 / "kmers.counts").exists(), tag
