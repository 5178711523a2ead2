"""HyperLogLog registers on the GPU: kt_card_add_reads against the numpy restatement of tests/card_ref.py over the oracle's
k-mers - registers and the number of windows compared exactly everywhere: inputs whose hashes are chosen (ranks at both
ends of their range, the first and the last register), noisy reads at the smallest and the largest register arrays, poly-A
(every lane of every wave on one register), the hard read shapes, accumulation in pieces and in either order, a batch that
fills the grid through shifted views with fenced outputs, every argument error; then `kmertools card` end to end against
files restated from the parsed records, and `--estimate-size` on the table commands: the same files as without it, from
a smaller table, where the input's bound is refused, and after an estimate made too small on purpose (KT_CARD_SCALE)."""
import functools
import gzip
import os
import re
import subprocess

import numpy as np
import pytest

import card_ref
import read_batches as rb
from test_buffer_views import Fenced, HostFenced, bases_view, host_bases_view, noisy_reads, offsets_view

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "kmertools_amd", "bin", "kmertools")
ACGT = np.frombuffer(b"ACGT", np.uint8)
KT_ERR_ARG = 1
KT_MEM_HOST, KT_MEM_DEVICE = 0, 1


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


# ---- helpers -----------------------------------------------------------------------------------------------------------------

def want_of(oracle, batch, k, p, seed=0, into=None):
    """-> (registers, windows) of a read_batches.Batch"""
    f, r, _ = rb.oracle_kmers_flat(oracle, batch, k)
    return card_ref.registers_of_hashes(card_ref.mix64(np.minimum(f, r) ^ np.uint64(seed)), p, into), len(f)


def dev_card(torch, ctx, bases, offsets, k, p, seed=0, regs=None, n_kmers=0):
    """kt_card_add_reads in device mode; regs: the registers to combine into (default zeros); n_kmers: its start value, None:
    a null pointer.  -> (registers, n_kmers or None)"""
    n = len(offsets) - 1
    d_b = torch.from_numpy(np.array(bases, np.uint8) if len(bases) else np.zeros(1, np.uint8)).cuda()
    d_o = torch.from_numpy(np.asarray(offsets).astype(np.int64)).cuda()
    d_r = torch.from_numpy(np.zeros(1 << p, np.uint8) if regs is None else np.ascontiguousarray(regs)).cuda()
    d_n = None if n_kmers is None else torch.full((1,), int(n_kmers), dtype=torch.int64, device="cuda")
    ctx.card_add(d_b, d_o, n, k, d_r, p, seed, d_n)
    torch.cuda.synchronize()
    return d_r.cpu().numpy(), None if d_n is None else int(d_n.cpu().numpy()[0])


def check(torch, ctx, oracle, batch, k, p, seed=0, modes=("device", "host")):
    want, windows = want_of(oracle, batch, k, p, seed)
    for mode in modes:
        if mode == "device":
            got, n = dev_card(torch, ctx, batch.bases, batch.offsets, k, p, seed)
        else:
            got, n = ctx.card_host(batch.bases, batch.offsets, k, p, seed)
        bad = np.flatnonzero(got != want)
        assert not len(bad), (batch.name, mode, k, p, len(bad), bad[:8], got[bad[:8]], want[bad[:8]])
        assert n == windows, (batch.name, mode, k, p, n, windows)
    return want, windows


# ---- inputs whose hashes are chosen --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("p", [4, 16])
@pytest.mark.parametrize("k", [31, 1])
def test_crafted_hashes(torch_mod, ctx, oracle, p, k):
    """one read of exactly k bases; seed = unmix64((j << q) | w) ^ x puts its one k-mer x into register j with the low word w"""
    rng = np.random.default_rng(31 * p + k)
    m, q = 1 << p, 64 - p
    seq = ACGT[rng.integers(0, 4, size=k)].tobytes()
    f, r, _ = oracle.kmers(seq, k)
    x = int(min(f[0], r[0]))
    bases, offsets = np.frombuffer(seq, np.uint8), np.array([0, k], np.uint64)
    for j in (0, m - 1, m // 2 + 1):
        for w, rank in ((0, q + 1), (1, q), (1 << (q - 1), 1), (3, q - 1), ((1 << q) - 1, 1)):
            seed = card_ref.unmix64((j << q) | w) ^ x
            want = np.zeros(m, np.uint8)
            want[j] = rank
            assert np.array_equal(card_ref.registers(oracle, bases, offsets, k, p, seed)[0], want)   # (the restatement agrees)
            got, n = dev_card(torch_mod, ctx, bases, offsets, k, p, seed)
            assert np.array_equal(got, want) and n == 1, (p, k, j, w, np.flatnonzero(got), got[got != 0])
            got, n = ctx.card_host(bases, offsets, k, p, seed)
            assert np.array_equal(got, want) and n == 1, (p, k, j, w)


# ---- noisy reads, every size of the register array's edge cases -------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def noisy_batch():
    return rb.Batch("noisy_reads(3, 400)", noisy_reads(3, 400))


@functools.lru_cache(maxsize=None)
def noisy_kmers(k):
    from oracle import kt_oracle
    f, r, _ = rb.oracle_kmers_flat(kt_oracle, noisy_batch(), k)
    return np.minimum(f, r)


@pytest.mark.parametrize("k", [1, 15, 16, 31])
@pytest.mark.parametrize("p", [4, 5, 14, 16])
def test_noisy_reads(torch_mod, ctx, oracle, p, k):
    """p = 4: all 16 registers share four LDS words in every wave; p = 16: the largest LDS array"""
    b, seed = noisy_batch(), 0x5EED0000 + p
    km = noisy_kmers(k)
    want = card_ref.registers_of_hashes(card_ref.mix64(km ^ np.uint64(seed)), p)
    got, n = dev_card(torch_mod, ctx, b.bases, b.offsets, k, p, seed)
    assert np.array_equal(got, want) and n == len(km), (p, k, np.flatnonzero(got != want)[:8])
    got, n = ctx.card_host(b.bases, b.offsets, k, p, seed)
    assert np.array_equal(got, want) and n == len(km), (p, k)


# ---- every lane on one register --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("p", [4, 14])
@pytest.mark.parametrize("unit", [b"A", b"AC"])
def test_repeats(torch_mod, ctx, oracle, p, unit):
    """2 000 x 150 poly-A: every lane of every wave raises the same register, and the call returns with its exact value;
    (AC)n: two k-mers"""
    n_reads, L, k = 2000, 150, 31
    read = (unit * L)[:L]
    one = rb.Batch("one", [read])
    f, r, _ = rb.oracle_kmers_flat(oracle, one, k)
    canon = np.minimum(f, r)
    assert len(np.unique(canon)) == len(unit) and len(canon) == L - k + 1
    want = card_ref.registers_of_hashes(card_ref.mix64(canon), p)
    assert 1 <= int((want != 0).sum()) <= len(unit)
    bases = np.frombuffer(read * n_reads, np.uint8)
    offsets = np.arange(n_reads + 1, dtype=np.uint64) * np.uint64(L)
    got, n = dev_card(torch_mod, ctx, bases, offsets, k, p)
    assert np.array_equal(got, want) and n == n_reads * (L - k + 1), (np.flatnonzero(got != want), got[got != want])


# ---- the hard read shapes --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", ["tiny", "empty_runs", "lattice", "long_read"])
def test_read_shapes(torch_mod, ctx, oracle, shape):
    k, p = 31, 12
    if shape == "tiny":          # thousands of reads shorter than k and shorter than a 16-base lane
        b = rb.tiny_batch(11, k, 4000)
        assert rb.shape_numbers(b.offsets)["segments_over_512"] >= 1
    elif shape == "empty_runs":  # runs of empty reads, at the start, the end and behind segment ends
        b = rb.empty_runs_batch(12)
    elif shape == "lattice":     # read ends on the structural constants
        b = rb.lattice_batch(13, k, poly_a=True)
    else:                        # one read of 300 000 bases between two short ones
        rng = np.random.default_rng(14)
        seqs = [ACGT[rng.integers(0, 4, size=L)].copy() for L in (40, 300_000, 33)]
        seqs[1][rng.integers(0, 300_000, size=200)] = ord("N")
        b = rb.Batch("long_read", [s.tobytes() for s in seqs])
    _, windows = check(torch_mod, ctx, oracle, b, k, p, seed=7)
    assert windows > 0
    if shape in ("tiny", "lattice"):
        check(torch_mod, ctx, oracle, b, 15, 16, seed=8, modes=("device",))


# ---- accumulation ----------------------------------------------------------------------------------------------------------------

def test_accumulation(torch_mod, ctx, oracle):
    torch, k, p, seed = torch_mod, 21, 10, 99
    a = rb.Batch("a", noisy_reads(21, 120))
    b = rb.Batch("b", noisy_reads(22, 150))
    ab = rb.Batch("ab", a.seqs + b.seqs)
    want, windows = want_of(oracle, ab, k, p, seed)
    wa, na = want_of(oracle, a, k, p, seed)
    one, n1 = dev_card(torch, ctx, ab.bases, ab.offsets, k, p, seed)
    assert np.array_equal(one, want) and n1 == windows
    for first, second in ((a, b), (b, a)):
        r1, c1 = dev_card(torch, ctx, first.bases, first.offsets, k, p, seed, n_kmers=5)
        r2, c2 = dev_card(torch, ctx, second.bases, second.offsets, k, p, seed, regs=r1, n_kmers=c1)
        assert np.array_equal(r2, want) and c2 == windows + 5
    assert not np.array_equal(wa, want)   # (the second batch raised something)
    # host mode accumulates into the caller's arrays in the same way
    regs, nk = np.zeros(1 << p, np.uint8), np.full(1, 5, np.uint64)
    ctx.card_add(a.bases, a.offsets, a.n, k, regs, p, seed, nk, KT_MEM_HOST)
    assert np.array_equal(regs, wa) and int(nk[0]) == na + 5
    ctx.card_add(b.bases, b.offsets, b.n, k, regs, p, seed, nk, KT_MEM_HOST)
    assert np.array_equal(regs, want) and int(nk[0]) == windows + 5
    # registers preset to 255 stay, the others are raised as before
    preset = np.zeros(1 << p, np.uint8)
    at = np.array([0, 1, 2, 3, 517, (1 << p) - 1])
    preset[at] = 255
    got, _ = dev_card(torch, ctx, ab.bases, ab.offsets, k, p, seed, regs=preset)
    assert np.array_equal(got, np.maximum(want, preset))
    host = preset.copy()
    ctx.card_add(ab.bases, ab.offsets, ab.n, k, host, p, seed, None, KT_MEM_HOST)   # (n_kmers NULL is accepted)
    assert np.array_equal(host, np.maximum(want, preset))
    got, none = dev_card(torch, ctx, ab.bases, ab.offsets, k, p, seed, n_kmers=None)
    assert np.array_equal(got, want) and none is None


def test_no_reads_touches_nothing(torch_mod, ctx):
    torch, p = torch_mod, 8
    regs = Fenced(torch, 1 << p, torch.uint8, align=3)
    nk = Fenced(torch, 1, torch.int64, align=8)
    d_o = torch.zeros(1, dtype=torch.int64, device="cuda")
    ctx.card_add(None, d_o, 0, 31, regs.t, p, 0, nk.t)
    ctx.card_add(None, None, 0, 31, None, p, 0, None)
    torch.cuda.synchronize()
    regs.check()
    nk.check()
    assert (regs.np(np.uint8) == rb.GUARD).all() and (nk.np(np.uint8) == rb.GUARD).all()
    # reads without a base: the same
    d_o = torch.zeros(6, dtype=torch.int64, device="cuda")
    ctx.card_add(None, d_o, 5, 31, regs.t, p, 0, nk.t)
    torch.cuda.synchronize()
    assert (regs.np(np.uint8) == rb.GUARD).all() and (nk.np(np.uint8) == rb.GUARD).all()
    h = HostFenced(1 << p, np.uint8)
    ctx.card_add(np.zeros(1, np.uint8), np.zeros(1, np.uint64), 0, 31, h.a, p, 0, None, KT_MEM_HOST)
    ctx.card_add(np.zeros(1, np.uint8), np.zeros(4, np.uint64), 3, 31, h.a, p, 0, None, KT_MEM_HOST)
    h.check()
    assert (h.a == rb.GUARD).all()


# ---- a batch that fills the grid ---------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def full_batch():
    from oracle import kt_oracle
    bases, offsets = kt_oracle.synth_reads(0x63617264, 40_000, 150, noise=True)
    b = rb.Batch.of_lens("synth(40000 x 150)", bases, np.full(40_000, 150))
    f, r, _ = rb.oracle_kmers_flat(kt_oracle, b, 31)
    return b, np.minimum(f, r)


def test_full_size_device_views(torch_mod, ctx):
    """732 segments on the 512 workgroups of p = 16: bases at 3 past a 256-byte boundary, offsets at 8 mod 16, the registers at
    an odd address between guard bands, the count between guard bands"""
    torch, k, p, seed = torch_mod, 31, 16, 1
    b, canon = full_batch()
    want = card_ref.registers_of_hashes(card_ref.mix64(canon ^ np.uint64(seed)), p)
    d_b, d_o = bases_view(torch, b.bases, 3), offsets_view(torch, b.offsets)
    regs = Fenced(torch, 1 << p, torch.uint8, align=1, prefill=np.zeros(1 << p, np.uint8))
    nk = Fenced(torch, 1, torch.int64, align=8, prefill=np.array([1000], np.int64))
    ctx.card_add(d_b, d_o, b.n, k, regs.t, p, seed, nk.t)
    torch.cuda.synchronize()
    regs.check("registers")
    nk.check("n_kmers")
    got = regs.np(np.uint8)
    assert np.array_equal(got, want), np.flatnonzero(got != want)[:8]
    assert int(nk.np(np.int64)[0]) == 1000 + len(canon)
    # the estimate of these registers lies within five standard errors of the truth (the restatement's does: asserted on the CPU)
    from kmertools_amd import device
    est, _ = device.card_estimate(got)
    assert abs(est / card_ref.estimate(want)[0] - 1.0) <= 1e-12
    assert abs(est / len(np.unique(canon)) - 1.0) <= 5 * card_ref.rel_error(p)


def test_full_size_host(ctx):
    k, p, seed = 31, 14, 2
    b, canon = full_batch()
    want = card_ref.registers_of_hashes(card_ref.mix64(canon ^ np.uint64(seed)), p)
    regs = HostFenced(1 << p, np.uint8, prefill=0)
    nk = HostFenced(1, np.uint64, prefill=0)
    ctx.card_add(host_bases_view(b.bases, 5), b.offsets, b.n, k, regs.a, p, seed, nk.a, KT_MEM_HOST)
    regs.check("registers")
    nk.check("n_kmers")
    assert np.array_equal(regs.a, want) and int(nk.a[0]) == len(canon)


# ---- argument errors -------------------------------------------------------------------------------------------------------------

def test_argument_errors_touch_nothing(torch_mod, ctx):
    from kmertools_amd import _lib
    torch, p = torch_mod, 10
    seq = ACGT[np.random.default_rng(1).integers(0, 4, size=100)]
    d_b = torch.from_numpy(seq.copy()).cuda()
    d_o = torch.tensor([0, 100], dtype=torch.int64, device="cuda")
    regs = Fenced(torch, 1 << 16, torch.uint8, align=1)     # room for every p that is tried
    nk = Fenced(torch, 1, torch.int64, align=8)

    def refused(fn):
        with pytest.raises(_lib.KmertoolsError) as e:
            fn()
        assert e.value.code == KT_ERR_ARG, e.value
        torch.cuda.synchronize()
        regs.check()
        nk.check()
        assert (regs.np(np.uint8) == rb.GUARD).all() and (nk.np(np.uint8) == rb.GUARD).all()

    for k in (0, 32, -1):
        refused(lambda: ctx.card_add(d_b, d_o, 1, k, regs.t, p, 0, nk.t))
    for bad_p in (3, 17, 0, -1, 64):
        refused(lambda: ctx.card_add(d_b, d_o, 1, 31, regs.t, bad_p, 0, nk.t))
    for mem in (2, -1):
        refused(lambda: ctx.card_add(d_b, d_o, 1, 31, regs.t, p, 0, nk.t, mem))
    refused(lambda: ctx.card_add(d_b, None, 1, 31, regs.t, p, 0, nk.t))
    refused(lambda: ctx.card_add(d_b, d_o, 1, 31, None, p, 0, nk.t))
    refused(lambda: ctx.card_add(None, d_o, 1, 31, regs.t, p, 0, nk.t))
    # a read of 2^32 bases: refused from the offsets alone, in both memory kinds
    long_o = np.array([0, 10, 10 + (1 << 32)], np.uint64)
    refused(lambda: ctx.card_add(d_b, torch.from_numpy(long_o.astype(np.int64)).cuda(), 2, 31, regs.t, p, 0, nk.t))
    h = HostFenced(1 << p, np.uint8)
    hn = HostFenced(1, np.uint64)
    with pytest.raises(_lib.KmertoolsError) as e:
        ctx.card_add(seq, long_o, 2, 31, h.a, p, 0, hn.a, KT_MEM_HOST)
    assert e.value.code == KT_ERR_ARG
    for fn in (lambda: ctx.card_add(seq, np.array([0, 100], np.uint64), 1, 32, h.a, p, 0, hn.a, KT_MEM_HOST),
               lambda: ctx.card_add(seq, np.array([0, 100], np.uint64), 1, 31, h.a, 17, 0, hn.a, KT_MEM_HOST),
               lambda: ctx.card_add(None, np.array([0, 100], np.uint64), 1, 31, h.a, p, 0, hn.a, KT_MEM_HOST)):
        with pytest.raises(_lib.KmertoolsError) as e:
            fn()
        assert e.value.code == KT_ERR_ARG
    h.check()
    hn.check()
    assert (h.a == rb.GUARD).all() and (hn.raw == rb.GUARD).all()


# ---- the command line --------------------------------------------------------------------------------------------------------------

def cli_run(*args, env=None):
    e = dict(os.environ)
    e.update(env or {})
    return subprocess.run([CLI, *map(str, args)], capture_output=True, text=True, timeout=600, env=e)


def write_fasta(path, recs, width=70):
    opener = gzip.open if str(path).endswith(".gz") else open
    with opener(path, "wt") as f:
        for name, seq in recs:
            f.write(">%s some description\n" % name)
            for a in range(0, len(seq), width):
                f.write(seq[a:a + width].decode() + "\n")


def write_fastq(path, recs):
    with open(path, "wt") as f:
        for name, seq in recs:
            f.write("@%s\n%s\n+\n%s\n" % (name, seq.decode(), "I" * len(seq)))


def cli_records(seed, n, genome_seed=0):
    rng = np.random.default_rng(seed)
    genome = ACGT[np.random.default_rng(1000 + genome_seed).integers(0, 4, size=30_000)]
    recs = []
    for i in range(n):
        L = int(rng.integers(0, 9_000)) if i % 5 else (0, 10, 15_000)[i // 5 % 3]
        a = int(rng.integers(0, len(genome) - L))
        seq = genome[a:a + L].copy()
        if L > 50:
            seq[rng.integers(0, L, size=3)] = ord("N")
            seq[10:20] |= 0x20
        recs.append(("rec%d" % i, seq.tobytes()))
    return recs


def bound_bases(path, recs):
    """what the table plan takes for the input's bases without reading a plain file: its size, half of it for FASTQ"""
    if str(path).endswith(".gz"):
        return sum(len(q) for _, q in recs)
    size = os.path.getsize(path)
    return size // 2 if str(path).endswith((".fq", ".fastq")) else size


def want_card_files(oracle, path, recs, k, p, seed, prefix=""):
    from kmertools_amd import device
    bases, offsets = device.to_csr([q for _, q in recs])
    reg, windows = card_ref.registers(oracle, bases, offsets, k, p, seed)
    est, zeros = card_ref.estimate(reg)
    want = min(card_ref.bound_slots(bound_bases(path, recs), k), card_ref.slots_for_estimate(est, p))
    rows = [("sequences", len(recs)), ("bases", len(bases)), ("kmers", windows), ("precision", p), ("registers", 1 << p),
            ("zero_registers", zeros), ("distinct_estimate", int(np.floor(est + 0.5))), ("rel_std_error", "%.6f" % card_ref.rel_error(p)),
            ("slots_wanted", want)]
    stats = "".join("%s%s\t%s\n" % (prefix, a, b) for a, b in rows)
    registers = "%d\t%d\t%d\n" % (p, seed, k) + "".join("%d\n" % v for v in reg)
    return stats, registers, reg, est


@pytest.mark.parametrize("alt", [False, True])
def test_cli_card(oracle, tmp_path, alt):
    k, p, seed = 21, 12, 77
    recs_a, recs_b = [r for r in cli_records(1, 17) if r[1]], cli_records(2, 9)   # (FASTQ: no record without a base)
    fq, fa = tmp_path / "a.fq", tmp_path / "b.fa.gz"
    write_fastq(fq, recs_a)
    write_fasta(fa, recs_b)
    out = tmp_path / "out"
    r = cli_run("card", "-i", fq, "-o", out, "-k", k, "-p", p, "--seed", seed, *(("-a", fa) if alt else ()))
    assert r.returncode == 0, r.stderr
    stats_a, regs_a, reg_a, est_a = want_card_files(oracle, fq, recs_a, k, p, seed)
    assert (out / "card.registers").read_text() == regs_a
    if not alt:
        assert (out / "card.stats").read_text() == stats_a
        assert sorted(os.listdir(out)) == ["card.registers", "card.stats"]
        # the defaults: p = 14, seed 0, from the gzipped FASTA
        out2 = tmp_path / "out2"
        r = cli_run("card", "-i", fa, "-o", out2, "-k", 31)
        assert r.returncode == 0, r.stderr
        stats_b, regs_b, _, _ = want_card_files(oracle, fa, recs_b, 31, 14, 0)
        assert (out2 / "card.stats").read_text() == stats_b and (out2 / "card.registers").read_text() == regs_b
        return
    stats_b, regs_b, reg_b, est_b = want_card_files(oracle, fa, recs_b, k, p, seed, "alt_")
    uni = card_ref.estimate(np.maximum(reg_a, reg_b))[0]
    inter = max(0.0, est_a + est_b - uni)
    tail = "union_estimate\t%d\nintersection_estimate\t%d\njaccard_estimate\t%.6f\n" % (
        int(np.floor(uni + 0.5)), int(np.floor(inter + 0.5)), inter / uni if uni > 0 else 0.0)
    assert (out / "card.stats").read_text() == stats_a + stats_b + tail
    assert (out / "card.alt.registers").read_text() == regs_b
    assert inter > 0   # (both inputs are cut from one genome)


# ---- --estimate-size ---------------------------------------------------------------------------------------------------------------

K_SIZING = 31


@pytest.fixture(scope="module")
def sized(tmp_path_factory):
    """about 2 000 reads of 100 bp sampled from a 20 kb random genome with a few errors (FASTQ), a second such sample, and the
    two wants of the first: from the input's bound and from the restated estimate"""
    from oracle import kt_oracle
    from kmertools_amd import device
    d = tmp_path_factory.mktemp("sizing")
    rng = np.random.default_rng(2024)
    genome = ACGT[rng.integers(0, 4, size=20_000)]
    samples = []
    for name in ("a", "b"):
        recs = []
        for i in range(2000):
            s = int(rng.integers(0, len(genome) - 100))
            seq = genome[s:s + 100].copy()
            if rng.random() < 0.3:
                seq[int(rng.integers(0, 100))] = ACGT[int(rng.integers(0, 4))]
            recs.append(("%s%d" % (name, i), seq.tobytes()))
        path = d / ("%s.fq" % name)
        write_fastq(path, recs)
        samples.append((path, recs))
    path, recs = samples[0]
    bases, offsets = device.to_csr([q for _, q in recs])
    reg, _ = card_ref.registers(kt_oracle, bases, offsets, K_SIZING, 14, 0)
    est = card_ref.estimate(reg)[0]
    bound = card_ref.bound_slots(bound_bases(path, recs), K_SIZING)
    want = card_ref.slots_for_estimate(est, 14)
    assert 2 * want < bound, (want, bound)
    # the files of the runs without the flag
    base = {}
    for cmd, extra in (("unitigs", ()), ("ctr", ()), ("compare", ("-a", samples[1][0])),
                       ("filter", ("-a", samples[1][0], "--min-count", 1))):
        out = d / ("plain_" + cmd)
        r = cli_run(cmd, "-i", path, "-o", (out if cmd != "filter" else d / "plain_kept.fq"), "-k", K_SIZING, *extra,
                    env={"KT_CLI_TIMING": "1"})
        assert r.returncode == 0, (cmd, r.stderr)
        base[cmd] = (out if cmd != "filter" else d / "plain_kept.fq", r.stderr)
    return {"dir": d, "a": path, "b": samples[1][0], "bound": bound, "want": want, "est": est, "plain": base}


def table_slots(stderr):
    """the slots of the tables a run reports under KT_CLI_TIMING, summed"""
    m = re.search(r"tables? of (\d+)(?: \+ (\d+))? slots", stderr)
    assert m, stderr
    return int(m.group(1)) + int(m.group(2) or 0)


def sorted_lines(path):
    return sorted(open(path, "rb").read().splitlines())


@pytest.mark.parametrize("cmd", ["unitigs", "ctr", "compare", "filter"])
def test_cli_estimate_size_same_files_smaller_table(sized, cmd):
    d, (plain, plain_err) = sized["dir"], sized["plain"][cmd]
    extra = {"compare": ("-a", sized["b"]), "filter": ("-a", sized["b"], "--min-count", 1)}.get(cmd, ())
    out = d / ("est_" + cmd) if cmd != "filter" else d / "est_kept.fq"
    r = cli_run(cmd, "-i", sized["a"], "-o", out, "-k", K_SIZING, "--estimate-size", *extra, env={"KT_CLI_TIMING": "1"})
    assert r.returncode == 0, r.stderr
    assert "[card]" not in r.stderr
    if cmd == "unitigs":
        assert (out / "unitigs.fa").read_bytes() == (plain / "unitigs.fa").read_bytes()
        assert (out / "unitigs.stats").read_bytes() == (plain / "unitigs.stats").read_bytes()
    elif cmd == "ctr":
        assert sorted_lines(out / "kmers.counts") == sorted_lines(plain / "kmers.counts")
        assert len(sorted_lines(out / "kmers.counts")) > 20_000 - K_SIZING
    elif cmd == "compare":
        assert (out / "compare.matrix").read_bytes() == (plain / "compare.matrix").read_bytes()
        assert (out / "compare.stats").read_bytes() == (plain / "compare.stats").read_bytes()
    else:
        assert out.read_bytes() == plain.read_bytes() and out.stat().st_size > 0
    assert table_slots(r.stderr) < table_slots(plain_err), (r.stderr, plain_err)
    m = re.findall(r"\[timing\] card pre-pass: [0-9.]+ s, estimate (\d+), slots wanted (\d+) \(bound: (\d+)\)", r.stderr)
    assert len(m) == (2 if cmd == "compare" else 1), r.stderr
    if cmd in ("unitigs", "ctr"):    # (counted from the input itself: the restated numbers)
        assert [int(x) for x in m[0]] == [int(np.floor(sized["est"] + 0.5)), sized["want"], sized["bound"]]
    assert "card pre-pass" not in plain_err


def test_cli_estimate_size_where_the_bound_is_refused(sized):
    """KT_CTR_MAX_SLOTS between the two wants: unitigs refuses the bound's plan of several passes, and runs with the estimate"""
    d, mid = sized["dir"], (sized["want"] + sized["bound"]) // 2
    env = {"KT_CTR_MAX_SLOTS": str(mid)}
    out = d / "refused"
    r = cli_run("unitigs", "-i", sized["a"], "-o", out, "-k", K_SIZING, env=env)
    assert r.returncode == 101, r.stderr
    assert "unitigs needs the whole table on the device" in r.stderr
    assert "(%d slots wanted, room for %d)" % (sized["bound"], mid) in r.stderr
    out = d / "fits"
    r = cli_run("unitigs", "-i", sized["a"], "-o", out, "-k", K_SIZING, "--estimate-size", env=env)
    assert r.returncode == 0, r.stderr
    plain = sized["plain"]["unitigs"][0]
    assert (out / "unitigs.fa").read_bytes() == (plain / "unitigs.fa").read_bytes()
    # ... and graph in the same way
    r = cli_run("graph", "-i", sized["a"], "-o", d / "graph_refused", "-k", K_SIZING, "--stats-only", env=env)
    assert r.returncode == 101 and "graph needs the whole table on the device" in r.stderr
    r = cli_run("graph", "-i", sized["a"], "-o", d / "graph_fits", "-k", K_SIZING, "--stats-only", "--estimate-size", env=env)
    assert r.returncode == 0, r.stderr
    r = cli_run("graph", "-i", sized["a"], "-o", d / "graph_plain", "-k", K_SIZING, "--stats-only")
    assert r.returncode == 0, r.stderr
    assert (d / "graph_fits" / "graph.stats").read_bytes() == (d / "graph_plain" / "graph.stats").read_bytes()


@pytest.mark.parametrize("cmd", ["ctr", "unitigs"])
def test_cli_estimate_too_small_counts_again(sized, cmd):
    """KT_CARD_SCALE=0.01: a table of 1024 slots for tens of thousands of k-mers; the command says so once, starts over with the
    bound's plan and ends as a run without the flag ends"""
    d, plain = sized["dir"], sized["plain"][cmd][0]
    out = d / ("again_" + cmd)
    r = cli_run(cmd, "-i", sized["a"], "-o", out, "-k", K_SIZING, "--estimate-size", env={"KT_CARD_SCALE": "0.01", "KT_CLI_TIMING": "1"})
    assert r.returncode == 0, r.stderr
    said = [line for line in r.stderr.splitlines() if line.startswith("[card]")]
    scaled = int(np.floor(sized["est"] * 0.01 + 0.5))
    assert said == ["[card] estimate %d was too small for this input: counting again with the input's bound" % scaled], r.stderr
    assert "Error" not in r.stderr
    if cmd == "ctr":
        assert sorted_lines(out / "kmers.counts") == sorted_lines(plain / "kmers.counts")
    else:
        assert (out / "unitigs.fa").read_bytes() == (plain / "unitigs.fa").read_bytes()
        assert (out / "unitigs.stats").read_bytes() == (plain / "unitigs.stats").read_bytes()
    # the second run's table is the bound's
    slots = [int(x) for x in re.findall(r"table of (\d+) slots", r.stderr)]
    assert len(slots) == 2 and slots[0] < slots[1] == table_slots(sized["plain"][cmd][1]), r.stderr
