"""The read filter: kt_ctr_read_solidity (per read: k-mers, solid k-mers, start of the first weak one) against a Python
restatement of its definition over the oracle's k-mers and table, in host and device mode, with and without first_weak,
in every form a table can be in, over hash partitions, at full size; its argument errors; and `kmertools filter` end to
end, byte for byte against the restated expected file."""
import gzip
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "kmertools_amd", "bin", "kmertools")
GOLDEN = os.path.join(ROOT, "tests", "golden")
U32_MAX = 0xFFFFFFFF
RANGES = ((1, 1), (2, U32_MAX), (3, 5))


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


# ---- the restatement ----------------------------------------------------------------------------------------------------

class Table:
    """the oracle's table of some reads: count of a canonical k-mer (0 when absent)"""

    def __init__(self, oracle, bases, offsets, k):
        wk, wc = oracle.count_reads(bases, offsets, k)
        order = np.argsort(wk)
        self.keys, self.counts = wk[order], wc[order]

    def count(self, keys):
        if not len(self.keys):
            return np.zeros(len(keys), np.uint32)
        i = np.minimum(np.searchsorted(self.keys, keys), len(self.keys) - 1)
        return np.where(self.keys[i] == keys, self.counts[i], 0).astype(np.uint32)


def solidity_of(oracle, seq, k, count_of, lo, hi):
    """(n_kmers, n_solid, first_weak) of one read: count_of(canonical keys) -> counts"""
    f, r, end = oracle.kmers(seq, k)
    if not len(f):
        return 0, 0, U32_MAX
    cnt = count_of(np.minimum(f, r))
    solid = (cnt >= lo) & (cnt <= hi)
    weak = np.flatnonzero(~solid)
    return len(f), int(solid.sum()), int(end[weak[0]]) - k + 1 if len(weak) else U32_MAX


def want_solidity(oracle, seqs, k, table, lo, hi):
    out = np.array([solidity_of(oracle, s, k, table.count, lo, hi) for s in seqs], np.uint64).reshape(-1, 3)
    return out[:, 0].astype(np.uint32), out[:, 1].astype(np.uint32), out[:, 2].astype(np.uint32)


def mixed_reads(seed, n, k):
    """random reads with N runs and lower case, repeated so that counts 1..5 and more occur, reads shorter than k, empty
    reads, reads of 10 kbases and more (many segments each)"""
    rng = np.random.default_rng(seed)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    seqs = []
    for L in rng.integers(0, 400, size=n):
        s = acgt[rng.integers(0, 4, size=int(L))].copy()
        if L > 40 and rng.random() < 0.3:
            a = int(rng.integers(0, L - 20))
            s[a:a + int(rng.integers(1, 20))] = ord("N")
        if L > 40 and rng.random() < 0.2:
            a = int(rng.integers(0, L - 30))
            s[a:a + 30] = np.frombuffer(bytes(s[a:a + 30]).lower(), np.uint8)
        seqs.append(s.tobytes())
    seqs += [b"", b"ACGTACG", b"acgtn" * 2, b"A" * (k - 1), b"", b"C" * k]
    for L in (10_000, 17_321, 25_000):
        s = acgt[rng.integers(0, 4, size=L)].copy()
        s[L // 3:L // 3 + 5] = ord("N")
        seqs.append(s.tobytes())
    seqs += seqs[: n // 4] * 2 + seqs[: n // 10] * 2 + [b"A" * 2500]  # counts up to ~5 and a flood
    order = rng.permutation(len(seqs))
    return [seqs[i] for i in order]


def tiny_reads(seed, n, k, donors):
    """n short reads (20 bases, k + 1 when that is more): a segment holds more of them than its LDS image, so they take
    the global-atomics path; half are slices of the donor reads (present in the table)"""
    rng = np.random.default_rng(seed)
    L = max(20, k + 1)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    long_ = [d for d in donors if len(d) >= L]
    out = []
    for i in range(n):
        if i % 2 and long_:
            d = long_[int(rng.integers(0, len(long_)))]
            a = int(rng.integers(0, len(d) - L + 1))
            out.append(d[a:a + L])
        else:
            out.append(acgt[rng.integers(0, 4, size=L)].tobytes())
    return out


def solidity_device(torch, ctr, bases, offsets, lo, hi, first=True):
    n = len(offsets) - 1
    db = torch.from_numpy(bases if bases.size else np.zeros(1, np.uint8)).cuda()
    do = torch.from_numpy(offsets.astype(np.int64)).cuda()
    nk = torch.zeros(n, dtype=torch.int32, device="cuda")
    ns = torch.zeros(n, dtype=torch.int32, device="cuda")
    fw = torch.full((n,), -1, dtype=torch.int32, device="cuda") if first else None
    ctr.read_solidity(db, do, n, lo, hi, nk, ns, fw)
    torch.cuda.synchronize()
    u = lambda t: t.cpu().numpy().view(np.uint32)
    return u(nk), u(ns), (u(fw) if first else None)


def solidity_host_nofirst(ctr, bases, offsets, lo, hi):
    from kmertools_amd._lib import KT_MEM_HOST
    n = len(offsets) - 1
    nk = np.zeros(n, np.uint32)
    ns = np.zeros(n, np.uint32)
    ctr.read_solidity(bases if bases.size else np.zeros(1, np.uint8), offsets, n, lo, hi, nk, ns, None, KT_MEM_HOST)
    return nk, ns


def check_all_modes(torch, ctr, bases, offsets, want, lo, hi, tag):
    wn, ws, ww = want
    got = ctr.read_solidity_host(bases, offsets, lo, hi)
    for g, w, what in zip(got, want, ("n_kmers", "n_solid", "first_weak")):
        assert np.array_equal(g, w), (tag, lo, hi, "host", what, np.flatnonzero(g != w)[:5])
    nk, ns = solidity_host_nofirst(ctr, bases, offsets, lo, hi)
    assert np.array_equal(nk, wn) and np.array_equal(ns, ws), (tag, lo, hi, "host, no first_weak")
    nk, ns, fw = solidity_device(torch, ctr, bases, offsets, lo, hi)
    assert np.array_equal(nk, wn) and np.array_equal(ns, ws) and np.array_equal(fw, ww), (tag, lo, hi, "device")
    nk, ns, _ = solidity_device(torch, ctr, bases, offsets, lo, hi, first=False)
    assert np.array_equal(nk, wn) and np.array_equal(ns, ws), (tag, lo, hi, "device, no first_weak")


# ---- 1. the ABI against the restatement -----------------------------------------------------------------------------------

@pytest.mark.parametrize("k", [11, 15, 21, 31])
def test_read_solidity_against_restatement(torch_mod, ctx, oracle, k):
    from kmertools_amd import device
    from kmertools_amd.device import to_csr
    seqs = mixed_reads(300 + k, 1200, k)
    tiny = tiny_reads(400 + k, 4000, k, seqs)
    table = Table(oracle, *to_csr(seqs + tiny), k)
    assert (table.counts >= 3).any() and (table.counts == 1).any()
    ctr = device.Counter(ctx, k, max(1 << 16, 2 * len(table.keys)))
    ctr.add_pairs_host(table.keys, table.counts)
    for batch, tag in ((seqs, "mixed"), (tiny, "tiny reads")):
        bases, offsets = to_csr(batch)
        for lo, hi in RANGES:
            want = want_solidity(oracle, batch, k, table, lo, hi)
            assert want[0].any() and want[1].any()
            check_all_modes(torch_mod, ctr, bases, offsets, want, lo, hi, (tag, k))
    # the arrays are combined into, not overwritten: a second call adds n_kmers / n_solid, first_weak stays
    bases, offsets = to_csr(seqs)
    want = want_solidity(oracle, seqs, k, table, 2, U32_MAX)
    nk, ns, fw = ctr.read_solidity_host(bases, offsets, 2, None)
    from kmertools_amd._lib import KT_MEM_HOST
    ctr.read_solidity(bases, offsets, len(seqs), 2, U32_MAX, nk, ns, fw, KT_MEM_HOST)
    assert np.array_equal(nk, 2 * want[0]) and np.array_equal(ns, 2 * want[1]) and np.array_equal(fw, want[2])
    # no reads, and reads with no bases at all
    assert all(len(a) == 0 for a in ctr.read_solidity_host(np.zeros(0, np.uint8), np.zeros(1, np.uint64)))
    nk, ns, fw = ctr.read_solidity_host(np.zeros(0, np.uint8), np.zeros(4, np.uint64))
    assert not nk.any() and not ns.any() and (fw == U32_MAX).all()
    ctr.close()


# ---- 2. every table form -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", [13, 21])
def test_read_solidity_every_table_form(torch_mod, ctx, oracle, monkeypatch, k):
    torch = torch_mod
    from kmertools_amd import device
    from kmertools_amd.device import to_csr
    seqs = mixed_reads(500 + k, 1500, k)
    bases, offsets = to_csr(seqs)
    table = Table(oracle, bases, offsets, k)
    cap = max(1 << 16, 2 * len(table.keys))
    want = {r: want_solidity(oracle, seqs, k, table, *r) for r in RANGES}
    forms = []

    def check(ctr, tag):
        assert ctr.size() == len(table.keys), tag
        for lo, hi in RANGES:
            got = ctr.read_solidity_host(bases, offsets, lo, hi)
            for g, w in zip(got, want[(lo, hi)]):
                assert np.array_equal(g, w), (tag, k, lo, hi)
            nk, ns, fw = solidity_device(torch, ctr, bases, offsets, lo, hi)
            assert all(np.array_equal(a, b) for a, b in zip((nk, ns, fw), want[(lo, hi)])), (tag, k, lo, hi, "device")
        forms.append(tag)

    # the probing image, counted from a small batch
    ctr = device.Counter(ctx, k, cap)
    ctr.add_reads_host(bases, offsets)
    check(ctr, "probing")
    ctr.close()
    # (key, count) pairs
    ctr = device.Counter(ctx, k, cap)
    ctr.add_pairs_host(table.keys, table.counts)
    check(ctr, "add_pairs")
    ctr.close()
    # the dense ranges of a bulk build
    monkeypatch.setenv("KT_BULK", "1")
    monkeypatch.setenv("KT_BULK_MIN_BASES", "0")
    ctr = device.Counter(ctx, k, cap)
    ctr.add_reads_host(bases, offsets)
    check(ctr, "bulk")
    ctr.close()
    # an export target's arrays
    m = len(table.keys) + 9
    xk = torch.zeros(m, dtype=torch.int64, device="cuda")
    xc = torch.zeros(m, dtype=torch.int32, device="cuda")
    ctr = device.Counter(ctx, k, cap)
    ctr.export_target(xk, xc, m)
    ctr.add_reads(torch.from_numpy(bases).cuda(), torch.from_numpy(offsets.astype(np.int64)).cuda(), len(seqs))
    check(ctr, "export target")
    ctr.close()
    # the direct-addressed build: 4^k slots
    if k <= 15:
        ctr = device.Counter(ctx, k, 4 ** k)
        assert ctr.capacity() == 4 ** k
        ctr.add_reads_host(bases, offsets)
        check(ctr, "direct")
        ctr.close()
    assert len(forms) == (5 if k <= 15 else 4)


# ---- 3. hash partitions -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", [15, 31])
def test_read_solidity_partitions_combine(torch_mod, ctx, oracle, k):
    torch = torch_mod
    from kmertools_amd import device
    from kmertools_amd._lib import KT_MEM_HOST
    from kmertools_amd.device import to_csr
    seqs = mixed_reads(700 + k, 1000, k)
    bases, offsets = to_csr(seqs)
    table = Table(oracle, bases, offsets, k)
    n = len(seqs)
    db = torch.from_numpy(bases).cuda()
    do = torch.from_numpy(offsets.astype(np.int64)).cuda()
    for lo, hi in RANGES:
        want = want_solidity(oracle, seqs, k, table, lo, hi)
        for n_parts in (2, 3):
            nk = np.zeros(n, np.uint32)
            ns = np.zeros(n, np.uint32)
            fw = np.full(n, U32_MAX, np.uint32)
            dnk = torch.zeros(n, dtype=torch.int32, device="cuda")
            dns = torch.zeros(n, dtype=torch.int32, device="cuda")
            dfw = torch.full((n,), -1, dtype=torch.int32, device="cuda")
            sizes = 0
            for part in range(n_parts):
                ctr = device.Counter(ctx, k, max(1 << 16, 2 * len(table.keys)))
                ctr.add_reads_host(bases, offsets, n_parts, part)
                sizes += ctr.size()
                ctr.read_solidity(bases, offsets, n, lo, hi, nk, ns, fw, KT_MEM_HOST, n_parts, part)
                ctr.read_solidity(db, do, n, lo, hi, dnk, dns, dfw, n_parts=n_parts, part=part)
                torch.cuda.synchronize()
                ctr.close()
            assert sizes == len(table.keys)
            for g, w in zip((nk, ns, fw), want):
                assert np.array_equal(g, w), (k, lo, hi, n_parts)
            for g, w in zip((dnk, dns, dfw), want):
                assert np.array_equal(g.cpu().numpy().view(np.uint32), w), (k, lo, hi, n_parts, "device")


# ---- 4. errors -------------------------------------------------------------------------------------------------------------

def test_read_solidity_errors(torch_mod, ctx):
    torch = torch_mod
    from kmertools_amd import device
    from kmertools_amd._lib import KT_ERR_ARG, KT_MEM_DEVICE, KT_MEM_HOST, lib
    L = lib()
    k = 21
    ctr = device.Counter(ctx, k, 1 << 16)
    bases = np.frombuffer(b"ACGTACGTACGTACGTACGTACGTACGTACGTACGT", np.uint8).copy()
    offsets = np.array([0, 20, len(bases)], np.uint64)
    nk = np.zeros(2, np.uint32)
    ns = np.zeros(2, np.uint32)
    fw = np.full(2, U32_MAX, np.uint32)
    p = lambda a: a.ctypes.data if a is not None else None

    def call(h=ctr._h, b=bases, o=offsets, n=2, lo=2, hi=U32_MAX, a=nk, s=ns, w=fw, mem=KT_MEM_HOST, parts=1, part=0):
        return L.kt_ctr_read_solidity(h, p(b), p(o), n, lo, hi, p(a), p(s), p(w), mem, parts, part)

    assert call() == 0
    bad = [dict(h=None), dict(lo=0), dict(lo=0, hi=0), dict(lo=6, hi=5), dict(parts=2, part=2), dict(parts=0, part=0),
           dict(mem=7), dict(o=None), dict(a=None), dict(s=None), dict(b=None)]
    for kw in bad:
        assert call(**kw) == KT_ERR_ARG, kw
        assert L.kt_last_error(), kw
    assert call(a=None, s=None, w=None, o=None, n=0) == 0  # no reads: nothing to check
    # a read of 2^32 bases: positions would not fit - refused from the offsets alone, host and device
    big = np.array([0, 5, 5 + (1 << 32)], np.uint64)
    assert call(o=big) == KT_ERR_ARG and b"2^32" in L.kt_last_error()
    db = torch.from_numpy(bases).cuda()
    dbig = torch.from_numpy(big.astype(np.int64)).cuda()
    dn = torch.zeros(2, dtype=torch.int32, device="cuda")
    assert L.kt_ctr_read_solidity(ctr._h, db.data_ptr(), dbig.data_ptr(), 2, 2, U32_MAX, dn.data_ptr(), dn.data_ptr(), None,
                                  KT_MEM_DEVICE, 1, 0) == KT_ERR_ARG
    assert b"2^32" in L.kt_last_error()
    assert call() == 0  # the context is still good
    ctr.close()
    # one shard of a sharded table (allocated as rank 0 of 2, never connected): refused, shards are out of scope
    sh = device.Sharded(ctx, k, 1 << 16, 1 << 16, 2, 0, ("host", lambda s, r, n: 1), connect=False)
    rc = L.kt_ctr_read_solidity(sh.table._h, p(bases), p(offsets), 2, 2, U32_MAX, p(nk), p(ns), p(fw), KT_MEM_HOST, 1, 0)
    assert rc == KT_ERR_ARG and b"shard" in L.kt_last_error()
    sh.close()


# ---- 5. full size -----------------------------------------------------------------------------------------------------------

def test_read_solidity_full_size_k31(torch_mod, ctx, oracle):
    """10 M x 150 bp at k = 31 through the bulk build, sampled from a genome with sequencing errors (solid and weak
    k-mers both): the k-mers sum to the table's occurrences, and 20 000 sampled reads agree with kt_ctr_lookup"""
    torch = torch_mod
    from kmertools_amd import device
    k, n, L = 31, 10_000_000, 150
    kpr = L - k + 1
    bases = torch.empty(n * L, dtype=torch.uint8, device="cuda")
    offsets = torch.empty(n + 1, dtype=torch.int64, device="cuda")
    ctx.synth_reads(0xF117E5, n, L, bases, offsets, noise=True, genome_len=20_000_000)
    ctr = device.Counter(ctx, k, int(1.9 * n * kpr))
    ctr.add_reads(bases, offsets, n)
    nk = torch.zeros(n, dtype=torch.int32, device="cuda")
    ns = torch.zeros(n, dtype=torch.int32, device="cuda")
    fw = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    lo, hi = 2, U32_MAX
    ctr.read_solidity(bases, offsets, n, lo, hi, nk, ns, fw)
    torch.cuda.synchronize()
    _, (d, occ) = ctr.spectrum(2, totals=True)
    assert int(nk.to(torch.int64).sum()) == occ
    nk, ns, fw = (t.cpu().numpy().view(np.uint32) for t in (nk, ns, fw))
    assert (ns < nk).any() and (ns == nk).any()
    rng = np.random.default_rng(7)
    sample = np.sort(rng.choice(n, size=20000, replace=False))
    hb = bases.view(n, L)[torch.from_numpy(sample).cuda()].cpu().numpy()
    seqs = [hb[i].tobytes() for i in range(len(sample))]
    per = [oracle.kmers(s, k) for s in seqs]
    keys = np.concatenate([np.minimum(f, r) for f, r, _ in per])
    counts = ctr.lookup_host(keys)
    at = 0
    for j, (f, r, end) in enumerate(per):
        cnt = counts[at:at + len(f)]
        at += len(f)
        solid = (cnt >= lo) & (cnt <= hi)
        weak = np.flatnonzero(~solid)
        i = sample[j]
        assert nk[i] == len(f) and ns[i] == int(solid.sum()), j
        assert fw[i] == (int(end[weak[0]]) - k + 1 if len(weak) else U32_MAX), j
    ctr.close()
    del bases, offsets
    torch.cuda.empty_cache()


# ---- 6. the CLI end to end ----------------------------------------------------------------------------------------------------

def run(*args, env=None, cwd=None):
    return subprocess.run([CLI, *map(str, args)], capture_output=True, timeout=600, env=env, cwd=cwd)


def parse_records(data):
    """(header without '>' / '@', sequence, quality or None): what the reader keeps with keep_records"""
    ws = b" \t\r\n\v\f"
    lines = data.split(b"\n")
    out = []
    i = 0
    if data[:1] == b">":
        while i < len(lines):
            h = lines[i].rstrip(ws)
            i += 1
            if not h:
                continue
            seq = []
            while i < len(lines) and not lines[i].startswith(b">"):
                seq.append(lines[i].rstrip(ws))
                i += 1
            out.append((h[1:], b"".join(seq), None))
    else:
        while i + 3 < len(lines) + 1 and i < len(lines):
            h = lines[i].rstrip(ws)
            if not h:
                i += 1
                continue
            out.append((h[1:], lines[i + 1].rstrip(ws), lines[i + 3].rstrip(ws)))
            i += 4
    return out


def read_file(path):
    data = open(path, "rb").read()
    return gzip.decompress(data) if str(path).endswith(".gz") else data


def want_filtered(oracle, recs, count_recs, k, lo, hi, frac=1.0, trim=False):
    table = Table(oracle, *oracle.to_csr([s for _, s, _ in count_recs]), k)
    out = []
    for hdr, seq, qual in recs:
        n, s, w = solidity_of(oracle, seq, k, table.count, lo, hi)
        if n == 0:
            continue
        keep = len(seq)
        if trim:
            if w != U32_MAX:
                keep = w + k - 1
            if keep < k:
                continue
        elif not (float(s) >= frac * float(n)):
            continue
        if qual is None:
            out.append(b">" + hdr + b"\n" + seq[:keep] + b"\n")
        else:
            out.append(b"@" + hdr + b"\n" + seq[:keep] + b"\n+\n" + qual[:keep] + b"\n")
    return b"".join(out)


def noisy_fastq(seed, n):
    """reads sampled from a small genome with substitutions, N and lower case, multi-word headers, some shorter than k"""
    rng = np.random.default_rng(seed)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    genome = acgt[rng.integers(0, 4, size=20000)]
    quals = np.frombuffer(b"!#+5?I", np.uint8)
    out = []
    for i in range(n):
        L = int(rng.integers(0, 220)) if i % 10 == 0 else int(rng.integers(60, 220))
        a = int(rng.integers(0, len(genome) - L))
        s = genome[a:a + L].copy()
        err = rng.random(L) < 0.01
        s[err] = acgt[rng.integers(0, 4, size=int(err.sum()))]
        if L > 50 and rng.random() < 0.1:
            s[int(rng.integers(0, L))] = ord("N")
        if L > 50 and rng.random() < 0.1:
            b = int(rng.integers(0, L - 20))
            s[b:b + 20] = np.frombuffer(bytes(s[b:b + 20]).lower(), np.uint8)
        q = quals[rng.integers(0, len(quals), size=L)].tobytes()
        out.append(b"@read%d lane=%d  sample x\n%s\n+\n%s\n" % (i, i % 5, s.tobytes(), q))
    return b"".join(out)


@pytest.fixture(scope="module")
def cli_bin():
    if not os.path.exists(CLI):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "kmertools_amd", "csrc"), "-j4"], stdout=subprocess.DEVNULL)
    return CLI


def test_filter_cli_golden_inputs(cli_bin, oracle, tmp_path):
    for name in ("reads.fq", "reads.fa", "reads.fq.gz"):
        src = os.path.join(GOLDEN, name)
        recs = parse_records(read_file(src))
        for extra, lo, hi, frac, trim in ((("--min-count", "1"), 1, U32_MAX, 1.0, False),
                                          (("--min-solid", "0"), 2, U32_MAX, 0.0, False),
                                          ((), 2, U32_MAX, 1.0, False),
                                          ((), 2, U32_MAX, 1.0, True),
                                          (("--min-count", "1", "--trim"), 1, U32_MAX, 1.0, True)):
            out = tmp_path / ("kept_" + name.replace(".gz", ""))
            r = run("filter", "-i", src, "-o", out, "-k", "15", *extra)
            assert r.returncode == 0, r.stderr
            want = want_filtered(oracle, recs, recs, 15, lo, hi, frac, trim)
            assert out.read_bytes() == want, (name, extra)
        # every k-mer of the file is in its own table: --min-count 1 keeps every read with a k-mer, whole
        run("filter", "-i", src, "-o", out, "-k", "15", "--min-count", "1")
        assert len(parse_records(out.read_bytes())) == len(recs)


def test_filter_cli_noisy_fastq(cli_bin, oracle, tmp_path):
    fq = tmp_path / "noisy.fastq"
    fq.write_bytes(noisy_fastq(11, 3000))
    recs = parse_records(fq.read_bytes())
    k = 21
    seen = {}
    cases = [(("--min-solid", "0"), 2, U32_MAX, 0.0, False),
             (("--min-solid", "0.5"), 2, U32_MAX, 0.5, False),
             (("--min-solid", "1"), 2, U32_MAX, 1.0, False),
             ((), 2, U32_MAX, 1.0, False),
             (("--trim",), 2, U32_MAX, 1.0, True),
             (("--trim", "--min-count", "3", "--max-count", "40"), 3, 40, 1.0, True),
             (("--min-count", "3", "--max-count", "40", "--min-solid", "0.9"), 3, 40, 0.9, False)]
    for extra, lo, hi, frac, trim in cases:
        out = tmp_path / "kept.fastq"
        r = run("filter", "-i", fq, "-o", out, "-k", k, *extra)
        assert r.returncode == 0, r.stderr
        want = want_filtered(oracle, recs, recs, k, lo, hi, frac, trim)
        got = out.read_bytes()
        assert got == want, extra
        kept = parse_records(got)
        assert 0 < len(kept) < len(recs), extra
        if trim:  # qualities cut with their sequences, and some reads really cut
            full = {h: s for h, s, _ in recs}
            assert all(len(s) == len(q) for _, s, q in kept)
            assert any(len(s) < len(full[h]) for h, s, _ in kept)
        seen[extra] = got
    assert seen[()] == seen[("--min-solid", "1")]  # the default
    assert len(set(seen.values())) == len(cases) - 1  # every other setting made a difference
    # out-of-core passes: the same bytes as the single pass
    size = fq.stat().st_size
    want_slots = size // 2 + size // 2 // 10 * 9
    env = dict(os.environ, KT_CTR_MAX_SLOTS=str(want_slots // 4 + 1), KT_CLI_TIMING="1")
    for extra, lo, hi, frac, trim in (cases[1], cases[4], cases[5]):
        out = tmp_path / "kept_passes.fastq"
        r = run("filter", "-i", fq, "-o", out, "-k", k, *extra, env=env, cwd=tmp_path)
        assert r.returncode == 0, r.stderr
        assert int(r.stderr.decode().split(" pass(es)")[0].split()[-1]) >= 4
        assert out.read_bytes() == want_filtered(oracle, recs, recs, k, lo, hi, frac, trim), extra
    assert not (tmp_path / "kmers.counts").exists() and not (tmp_path / "kmers.histo").exists()


def test_filter_cli_alt_input_and_fasta(cli_bin, oracle, tmp_path):
    """-a: the table is counted from another file (here a FASTA of every other read, so the rest is looked up against
    k-mers it did not contribute); FASTA in, FASTA out"""
    recs = parse_records(noisy_fastq(12, 2000))
    fa = tmp_path / "reads.fa"
    fa.write_bytes(b"".join(b">" + h + b"\n" + s[:40] + b"\n" + s[40:] + b"\n" for h, s, _ in recs))
    alt = tmp_path / "alt.fasta"
    alt.write_bytes(b"".join(b">a%d\n%s\n" % (i, s) for i, (_, s, _) in enumerate(recs[::2])))
    fa_recs = [(h, s, None) for h, s, _ in recs]
    alt_recs = [(b"", s, None) for _, s, _ in recs[::2]]
    k = 25
    for extra, lo, hi, frac, trim in ((("--min-count", "1"), 1, U32_MAX, 1.0, False),
                                      (("--min-count", "2", "--min-solid", "0.5"), 2, U32_MAX, 0.5, False),
                                      (("--min-count", "1", "--trim"), 1, U32_MAX, 1.0, True)):
        out = tmp_path / "kept.fa"
        r = run("filter", "-i", fa, "-a", alt, "-o", out, "-k", k, *extra)
        assert r.returncode == 0, r.stderr
        want = want_filtered(oracle, fa_recs, alt_recs, k, lo, hi, frac, trim)
        assert out.read_bytes() == want, extra
        assert 0 < len(parse_records(want)) < len(recs)
