"""Parity tests proper: the HIP path (through the C ABI) against the CPU oracle on the same
seeded inputs, against the reference's golden fixtures, and - at BASELINE sizes - through
size-independent properties.  Integer results are compared bit-exactly; f64 rows are
bit-exact too (one IEEE division of exact integers); f32 rows within 1e-6."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


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


@pytest.fixture(scope="module")
def hctx():
    """private-stream context used with host arrays"""
    from kmertools_amd import device
    c = device.Context(0)
    yield c
    c.close()


def ragged_reads(seed, n, max_len=400, noise=True, special=True):
    rng = np.random.default_rng(seed)
    lens = rng.integers(0, max_len, size=n)
    if special and n >= 8:
        lens[0] = 0
        lens[1] = 1
        lens[2] = 2
        lens[3] = 31
        lens[4] = 64
        lens[5] = 0
        lens[6] = 9000      # crosses a ctr segment and many oligo chunks
        lens[7] = 8192
    alpha = np.frombuffer(b"ACGT", np.uint8)
    seqs = []
    for L in lens:
        s = alpha[rng.integers(0, 4, size=L)].copy()
        if noise and L:
            m = rng.random(L)
            s[m < 0.01] = ord("N")
            low = (m > 0.01) & (m < 0.05)
            s[low] |= 0x20
            s[(m > 0.05) & (m < 0.055)] = ord("U")
            s[(m > 0.055) & (m < 0.057)] = 2       # raw byte code (kmer.rs:7 first row)
            s[(m > 0.057) & (m < 0.059)] = ord("R")  # IUPAC -> invalid
        seqs.append(s.tobytes())
    return seqs


def oracle_kmers_batch(oracle, seqs, k):
    fs, rs, es = [], [], []
    off = 0
    for s in seqs:
        f, r, e = oracle.kmers(s, k)
        fs.append(f)
        rs.append(r)
        es.append(e + np.uint64(off))
        off += len(s)
    return np.concatenate(fs), np.concatenate(rs), np.concatenate(es)


# ---------------------------------------------------------------------------------------------
# synthetic generator

@pytest.mark.parametrize("noise,genome", [(False, 0), (True, 0), (False, 5000), (True, 100000)])
def test_synth_matches_oracle(torch_mod, ctx, oracle, noise, genome):
    torch = torch_mod
    n, L, seed, first = 777, 150, 0x6b6d6572, 12345
    bases = torch.empty(n * L, dtype=torch.uint8, device="cuda")
    offsets = torch.empty(n + 1, dtype=torch.int64, device="cuda")
    ctx.synth_reads(seed, n, L, bases, offsets, noise=noise, genome_len=genome, first_read=first)
    torch.cuda.synchronize()
    want, woff = oracle.synth_reads(seed, n, L, noise=noise, genome_len=genome, first_read=first)
    assert np.array_equal(bases.cpu().numpy(), want)
    assert np.array_equal(offsets.cpu().numpy().astype(np.uint64), woff)


# ---------------------------------------------------------------------------------------------
# KmerGenerator surface (kt_kmers)

@pytest.mark.parametrize("k", [1, 2, 3, 4, 7, 15, 16, 17, 21, 30, 31])
def test_kmers_vs_oracle(hctx, oracle, k):
    from kmertools_amd import device
    seqs = ragged_reads(100 + k, 300)
    bases, offsets = device.to_csr(seqs)
    f, r, e = hctx.kmers_host(bases, offsets, k)
    wf, wr, we = oracle_kmers_batch(oracle, seqs, k)
    assert np.array_equal(e, we)
    assert np.array_equal(f, wf)
    assert np.array_equal(r, wr)


def test_kmers_golden(hctx, oracle, kat):
    from kmertools_amd import device
    for case in kat["kmers"]:
        b, o = device.to_csr([case["seq"]])
        f, r, _ = hctx.kmers_host(b, o, case["k"])
        assert [[int(x), int(y)] for x, y in zip(f, r)] == case["pairs"]
    c = kat["k31"]
    b, o = device.to_csr([c["seq"]])
    f, r, _ = hctx.kmers_host(b, o, 31)
    got = [device.numeric_to_kmer(int(min(x, y)), 31) for x, y in zip(f, r)]
    assert got == c["canonical_kmers_in_order"]


def test_kmers_empty_and_short(hctx):
    from kmertools_amd import device
    for seqs in ([], [b""], [b"", b""], [b"AC"], [b"ACG", b"", b"T"]):
        b, o = device.to_csr(seqs)
        f, r, e = hctx.kmers_host(b, o, 4)
        assert len(f) == 0 and len(r) == 0 and len(e) == 0


# ---------------------------------------------------------------------------------------------
# comp oligo / comp cgr -k  (kt_oligo_batch)

@pytest.mark.parametrize("k", [3, 4, 5, 6, 7])
@pytest.mark.parametrize("count_min", [True, False])
def test_oligo_vs_oracle(hctx, oracle, k, count_min):
    from kmertools_amd import device
    n = 300 if k <= 5 else 60
    seqs = ragged_reads(7 * k + count_min, n)
    bases, offsets = device.to_csr(seqs)
    # total_step = 2 is the python binding's raw-mode quirk (pybindings/src/oligo.rs:61); the
    # reference never applies it to canonical bins, so the oracle only models it for raw mode
    for norm, step in [(True, 1), (False, 1)] + ([] if count_min else [(True, 2)]):
        want = oracle.oligo_batch(bases, offsets, k, count_min, norm, float(step))
        got = hctx.oligo_host(bases, offsets, k, count_min, norm, step, "f64")
        assert got.shape == want.shape
        assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), (k, count_min, norm, step)
    want = oracle.oligo_batch(bases, offsets, k, count_min, True, 1.0)
    got32 = hctx.oligo_host(bases, offsets, k, count_min, True, 1, "f32")
    assert got32.dtype == np.float32
    assert np.max(np.abs(got32.astype(np.float64) - want)) <= 1e-6   # north_star tolerance
    cnt = oracle.oligo_batch(bases, offsets, k, count_min, False, 1.0)
    gotu = hctx.oligo_host(bases, offsets, k, count_min, False, 1, "u32")
    assert np.array_equal(gotu.astype(np.float64), cnt)


def test_oligo_golden_files(hctx, oracle, golden):
    from kmertools_amd import device
    recs = oracle.read_records(golden / "reads.fq")
    bases, offsets = device.to_csr([s for _, s in recs])
    norm = hctx.oligo_host(bases, offsets, 4, True, True)
    assert oracle.oligo_text(norm, True) == (golden / "expected_fa.kmers").read_bytes()
    cnt = hctx.oligo_host(bases, offsets, 4, True, False)
    assert oracle.oligo_text(cnt, False) == (golden / "expected_fa_batch_unnorm.kmers").read_bytes()
    hdr = [device.numeric_to_kmer(int(x), 4) for x in device.pos_map(4)[1]]
    assert oracle.oligo_text(norm, True, header_line=hdr) == (golden / "expected_fa_header.kmers").read_bytes()
    xy = device.cgr_coords(4, 16)
    assert oracle.oligocgr_text(cnt, xy) == (golden / "expected_reads.k4.cgr").read_bytes()
    # multi-line FASTA gives the same rows (ktio/src/seq.rs:165-233)
    recs_fa = oracle.read_records(golden / "reads.fa")
    b2, o2 = device.to_csr([s for _, s in recs_fa])
    assert np.array_equal(hctx.oligo_host(b2, o2, 4, True, True), norm)


def test_oligo_inline_kat(hctx, kat):
    from kmertools_amd import device
    c = kat["oligo_one"]
    b, o = device.to_csr([c["seq"]])
    assert hctx.oligo_host(b, o, 4, False, True).shape[1] == c["raw_len"]
    assert hctx.oligo_host(b, o, 4, True, True)[0, 0] == c["canon_norm_v0"]
    un = hctx.oligo_host(b, o, 4, True, False)[0]
    assert un[0] == c["canon_unnorm_v0"] and un.sum() == c["canon_unnorm_sum"]
    g = kat["oligocgr_one"]
    b, o = device.to_csr([g["seq"]])
    assert hctx.oligo_host(b, o, 4, True, True)[0, 0] == 1.0 / g["norm_first_freq_den"]


def test_oligo_empty_inputs(hctx):
    from kmertools_amd import device
    for seqs in ([], [b""], [b"AC", b"", b"NNNNNNNN"]):
        b, o = device.to_csr(seqs)
        out = hctx.oligo_host(b, o, 4)
        assert out.shape == (len(seqs), 136) and not out.any()   # total = 0 -> divisor 1 -> zero row


def test_oligo_device_tensors_many_tiles(torch_mod, ctx, oracle):
    """device-pointer path, several tiles per workgroup, noise reads, all dtypes"""
    torch = torch_mod
    n, L = 200_000, 150
    bases = torch.empty(n * L, dtype=torch.uint8, device="cuda")
    offsets = torch.empty(n + 1, dtype=torch.int64, device="cuda")
    ctx.synth_reads(42, n, L, bases, offsets, noise=True)
    out = torch.empty((n, 136), dtype=torch.float64, device="cuda")
    ctx.oligo(bases, offsets, n, 4, out)
    torch.cuda.synchronize()
    hb, ho = oracle.synth_reads(42, n, L, noise=True)
    want = oracle.oligo_batch(hb, ho, 4, True, True, 1.0, threads=8)
    assert np.array_equal(out.cpu().numpy().view(np.uint64), want.view(np.uint64))
    # determinism: repeated launches give identical bits
    out2 = torch.empty_like(out)
    ctx.oligo(bases, offsets, n, 4, out2)
    torch.cuda.synchronize()
    assert torch.equal(out, out2)


_CAPTURE_SCRIPT = r"""
import sys, torch
sys.path.insert(0, sys.argv[1])
from kmertools_amd import device
n, L, k = 7_000_000, 150, 4
side = torch.cuda.Stream()
with torch.cuda.stream(side):
    c = device.Context(0, stream=side.cuda_stream)
    bases = torch.empty(n * L, dtype=torch.uint8, device="cuda")
    offsets = torch.empty(n + 1, dtype=torch.int64, device="cuda")
    c.synth_reads(0x6b6d6572 + 21, n, L, bases, offsets)
    ref = torch.empty((n, 136), dtype=torch.float32, device="cuda")
    for _ in range(26):   # past the warm-up launches: the next one would be a trial with events around it
        c.oligo(bases, offsets, n, k, ref, dtype="f32")
    side.synchronize()
    out = torch.zeros((n, 136), dtype=torch.float32, device="cuda")
    side.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        c.oligo(bases, offsets, n, k, out, dtype="f32")
    assert not c.oligo_launch_info()["measured"]
    for _ in range(2):
        out.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, ref)
    c.close()
print("captured ok")
"""


def test_oligo_launches_can_be_captured_into_a_graph(torch_mod):
    """a k = 4 launch large enough to take part in the launch-shape measurement, made while its stream is being captured:
    no event is recorded or queried (that would invalidate the capture), the graph replays, the rows are the plain launch's.
    In a process of its own: a torch graph capture in the test process left the device-wide synchronize of a later test
    (the launch-shape one) waiting for ever - torch's capture state, not the library's: the same suite without this test,
    and this test alone, are both green."""
    import subprocess, sys, pathlib
    root = str(pathlib.Path(__file__).resolve().parent.parent)
    r = subprocess.run([sys.executable, "-c", _CAPTURE_SCRIPT, root], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "captured ok" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])


def test_capture_then_launch_trials_without_torch():
    """round 4 saw a later test's device-wide synchronize wait for ever after a graph capture made through torch in the same
    process, and moved the capture test into a child process without knowing whose the hang was.  tools/capture_repro.cpp
    does the same sequence with the HIP runtime and the C ABI alone - 26 launches on a non-blocking side stream,
    hipStreamBeginCapture / kt_oligo_batch / EndCapture, two replays, rows equal to the plain launch's; then contexts on
    the NULL stream whose large launches take part in the launch-shape trials (events recorded and polled around them)
    with hipDeviceSynchronize between - under a watchdog: it does not hang and every round decides its launch shape, so
    the library's event trials are not what hung (it needs torch's capture in the process: the capture test above stays in
    a process of its own)"""
    import subprocess, pathlib
    exe = pathlib.Path(__file__).resolve().parent.parent / "kmertools_amd" / "bin" / "capture_repro"
    assert exe.exists(), "kmertools_amd/bin/capture_repro is built by make -C kmertools_amd/csrc (__graft_entry__.build)"
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    assert "captured, replayed twice, rows equal" in r.stdout and "no hang (with a capture before the trials)" in r.stdout
    assert r.stdout.count("decided 1") == 3, r.stdout


@pytest.mark.parametrize("count_min", [True, False])
def test_oligo_k7_producer_wave_many_tiles_per_workgroup(hctx, oracle, monkeypatch, count_min):
    """comp cgr k=7 runs with a producer wave (four store waves that never load + one wave that reads the input and
    publishes each tile a tile ahead).  One workgroup per CU (KT_OLIGO_OVERSUB=1) walks dozens of tiles: 150-bp tiles of
    one chunk, ragged ones, tiles of several chunks (long reads: the store waves count too, from the published tile), empty
    reads, a last tile that is not full - all rows against the oracle, and against the kernel without the producer wave"""
    from kmertools_amd import device
    rng = np.random.default_rng(77 + count_min)
    alpha = np.frombuffer(b"ACGTN", np.uint8)
    lens = np.full(12_001, 150)
    lens[1000:1400] = rng.integers(0, 400, size=400)          # ragged tiles, empty reads
    lens[5000:5040] = rng.integers(900, 6000, size=40)        # tiles of many chunks
    lens[5040:5048] = 0
    lens[9_000:9_016] = 1008                                  # exactly a chunk per read
    seqs = [alpha[rng.choice(5, size=L, p=[.2475, .2475, .2475, .2475, .01])].tobytes() for L in lens]
    bases, offsets = device.to_csr(seqs)
    want = oracle.oligo_batch(bases, offsets, 7, count_min, False, 1.0, threads=8)
    got = {}
    for pw in ("7", "8"):
        monkeypatch.setenv("KT_OLIGO_OVERSUB", "1")
        monkeypatch.setenv("KT_OLIGO_PW", pw)
        c = device.Context()
        got[pw] = c.oligo_host(bases, offsets, 7, count_min, False, 1, "u32")
        if pw == "7":
            f64 = c.oligo_host(bases, offsets, 7, count_min, True, 1, "f64")
        c.close()
        assert np.array_equal(got[pw].astype(np.float64), want), pw
    assert np.array_equal(got["7"], got["8"])
    wantn = oracle.oligo_batch(bases, offsets, 7, count_min, True, 1.0, threads=8)
    assert np.array_equal(f64.view(np.uint64), wantn.view(np.uint64))


def test_pykmertools_surface(oracle, golden, kat):
    """the reference's own python tests (tests/test_oligo.py, test_kmers.py, test_utils.py)"""
    from kmertools_amd import pykmertools as kt
    seqs = [s.decode() for _, s in oracle.read_records(golden / "reads.fq")]
    gen = kt.OligoComputer(4)
    got = [[round(x, 6) for x in row] for row in gen.vectorise_batch(seqs)]
    truth = [list(map(float, ln.split())) for ln in (golden / "expected_fa.kmers").read_text().splitlines()]
    assert got == truth
    assert len(gen.get_header()) == 136 and len(gen.get_header(False)) == 256
    assert gen.get_header()[0] == "AAAA" and gen.get_header()[135] == "TTAA"
    kmers = list(kt.KmerGenerator("ACGTCC", 3))
    assert [kt.utils.to_acgt(f, 3) for f, _ in kmers] == kat["py_kmers"]["fwd_acgt"]
    assert kmers == [(6, 27), (27, 6), (45, 33), (53, 40)]
    assert kt.utils.to_acgt(111, 5) == "ACGTT" and kt.utils.to_acgt(27, 5) == "AACGT"
    assert kt.utils.to_numeric("ACGTT") == (111, 27)
    with pytest.raises(ValueError):
        kt.utils.to_numeric("A" * 33)
    # python raw-mode quirk: normalised raw vectors sum to 0.5 (pybindings/src/oligo.rs:61)
    v = gen.vectorise_one(seqs[0], norm=True, mins=False)
    assert abs(sum(v) - 0.5) < 1e-12
    want = oracle.oligo_one(seqs[0], 4, count_min=False, norm=True, total_step=2.0)
    assert np.array_equal(np.array(v), want)
    m, pos_kmer, count = kt.KmerGenerator("ACGT", 4).kmer_pos_maps()
    assert count == 136 and len(m) == 256 and pos_kmer[135] == oracle.kmer_to_numeric("TTAA")[0]


# ---------------------------------------------------------------------------------------------
# ctr (kt_ctr_*)

@pytest.mark.parametrize("k", [4, 10, 15, 21, 31])
def test_ctr_vs_oracle(hctx, oracle, k):
    from kmertools_amd import device
    seqs = ragged_reads(1000 + k, 400)
    # repeat some reads (and a reverse-complemented copy) so counts > 1 occur at every k
    comp = bytes.maketrans(b"ACGTacgt", b"TGCAtgca")
    seqs += seqs[10:60] + [s.translate(comp)[::-1] for s in seqs[20:40]]
    bases, offsets = device.to_csr(seqs)
    wk, wc = oracle.count_reads(bases, offsets, k)
    ctr = device.Counter(hctx, k, max(4096, 3 * len(wk)))
    ctr.add_reads_host(bases, offsets)
    assert ctr.size() == len(wk)
    gk, gc = ctr.export_host()
    assert np.array_equal(gk, wk) and np.array_equal(gc, wc)
    assert wc.max() > 1
    # chunked adds (= the reference's chunks) give the same table
    ctr.clear()
    half = len(seqs) // 2
    b1, o1 = device.to_csr(seqs[:half])
    b2, o2 = device.to_csr(seqs[half:])
    ctr.add_reads_host(b1, o1)
    ctr.add_reads_host(b2, o2)
    gk, gc = ctr.export_host()
    assert np.array_equal(gk, wk) and np.array_equal(gc, wc)
    ctr.close()


def test_ctr_golden_files(hctx, oracle, golden):
    from kmertools_amd import device
    recs = oracle.read_records(golden / "reads.fq")
    bases, offsets = device.to_csr([s for _, s in recs])
    ctr = device.Counter(hctx, 15, 4096)
    ctr.add_reads_host(bases, offsets)
    k, c = ctr.export_host()
    assert oracle.counts_lines(k, c) == sorted((golden / "expected_counts.part_0_chunk_0").read_text().splitlines())
    ctr.close()
    # merge fixtures: plain u32 sums per key (counter/src/lib.rs:201-210)
    ctr = device.Counter(hctx, 15, 4096)
    for f in sorted((golden / "computed_counts_test").iterdir()):
        rows = [ln.split("\t") for ln in f.read_text().splitlines() if ln.strip()]
        ctr.add_pairs_host([int(a) for a, _ in rows], [int(b) for _, b in rows])
    k, c = ctr.export_host()
    assert oracle.counts_lines(k, c) == sorted((golden / "expected_counts_test.counts").read_text().splitlines())
    acgt = sorted("%s\t%d" % (device.numeric_to_kmer(int(a), 15), int(b)) for a, b in zip(k, c))
    assert acgt == sorted((golden / "expected_counts_acgt_test.counts").read_text().splitlines())
    ctr.close()


def test_ctr_table_full_is_loud(hctx):
    from kmertools_amd import _lib, device
    seqs = ragged_reads(5, 200, special=False)
    b, o = device.to_csr(seqs)
    ctr = device.Counter(hctx, 21, 1024)
    ctr.add_reads_host(b, o)
    with pytest.raises(_lib.KmertoolsError) as ei:
        ctr.size()
    assert ei.value.code == _lib.KT_ERR_FULL
    ctr.close()


@pytest.mark.parametrize("n_owners", [1, 2, 3, 8])
def test_route_partitions_by_owner(hctx, oracle, n_owners):
    from kmertools_amd import device
    k = 31
    seqs = ragged_reads(77, 300)
    bases, offsets = device.to_csr(seqs)
    keys, counts = hctx.route_host(bases, offsets, k, n_owners)
    wf, wr, _ = oracle_kmers_batch(oracle, seqs, k)
    canon = np.minimum(wf, wr)
    assert counts.sum() == len(canon)
    assert np.array_equal(np.sort(keys), np.sort(canon))      # same multiset
    start = 0
    for o in range(n_owners):
        grp = keys[start:start + int(counts[o])]
        owners = {device.owner_of(int(x), n_owners) for x in grp[:2000]}
        assert owners <= {o}
        start += int(counts[o])
    # routed keys counted by their owners == counting the reads directly
    ctr = device.Counter(hctx, k, 4 * len(canon) + 1024)
    ctr.add_pairs_host(keys, None)
    gk, gc = ctr.export_host()
    wk, wc = oracle.count_reads(bases, offsets, k)
    assert np.array_equal(gk, wk) and np.array_equal(gc, wc)
    ctr.close()


# ---------------------------------------------------------------------------------------------
# BASELINE-size property checks (size-independent invariants, no oracle pass over the full set)

def test_cfg2_full_size_properties(torch_mod, ctx, oracle):
    """comp oligo k=4, 10 M x 150 bp: row sums, totals, sampled rows vs oracle"""
    torch = torch_mod
    n, L, k, seed = 10_000_000, 150, 4, 0x6b6d6572 + 1
    bases = torch.empty(n * L, dtype=torch.uint8, device="cuda")
    offsets = torch.empty(n + 1, dtype=torch.int64, device="cuda")
    ctx.synth_reads(seed, n, L, bases, offsets)
    cnt = torch.empty((n, 136), dtype=torch.int32, device="cuda")
    ctx.oligo(bases, offsets, n, k, cnt, norm=False, dtype="u32")
    torch.cuda.synchronize()
    # all-ACGT reads: every row holds exactly L-k+1 k-mers
    assert bool((cnt.sum(dim=1) == L - k + 1).all())
    del cnt
    out = torch.empty((n, 136), dtype=torch.float64, device="cuda")
    ctx.oligo(bases, offsets, n, k, out)
    torch.cuda.synchronize()
    s = out.sum(dim=1)
    assert float((s - 1.0).abs().max()) < 1e-12
    # sampled slices against the oracle, bit-exact
    for first in (0, 1_234_567, n - 4096):
        hb, ho = oracle.synth_reads(seed, 4096, L, first_read=first)
        want = oracle.oligo_batch(hb, ho, k, True, True, 1.0, threads=4)
        got = out[first:first + 4096].cpu().numpy()
        assert np.array_equal(got.view(np.uint64), want.view(np.uint64))


def test_oligo_launch_shape_is_measured_and_results_do_not_depend_on_it(torch_mod, monkeypatch):
    """k = 4 picks its workgroups per resident slot per output array by timing early large launches
    (kt_oligo_launch_info): a context that synchronises between launches has decided after WARM + 9 of them into an array, and the
    rows are the same bits under every setting and while measuring"""
    torch = torch_mod
    from kmertools_amd import device
    n, L, k, seed = 8_000_000, 150, 4, 0x6b6d6572 + 11
    unmeasured = {"wgs_per_slot": 96, "measured": False, "ns_per_read": {32: 0.0, 96: 0.0, 200: 0.0}}
    c0 = device.Context()
    bases = torch.empty(n * L, dtype=torch.uint8, device="cuda")
    offsets = torch.empty(n + 1, dtype=torch.int64, device="cuda")
    c0.synth_reads(seed, n, L, bases, offsets)
    ref = None
    for setting in ("32", "96", "200"):
        monkeypatch.setenv("KT_OLIGO_OVERSUB", setting)
        c = device.Context()
        o = torch.empty((n, 136), dtype=torch.float32, device="cuda")
        c.oligo(bases, offsets, n, k, o, dtype="f32")
        torch.cuda.synchronize()
        info = c.oligo_launch_info()
        assert info["wgs_per_slot"] == int(setting) and not info["measured"]
        c.close()
        if ref is None:
            ref = o
        else:
            assert torch.equal(o, ref)
            del o
    monkeypatch.delenv("KT_OLIGO_OVERSUB")
    c = device.Context()
    outs = [torch.empty((n, 136), dtype=torch.float32, device="cuda") for _ in range(2)]
    assert c.oligo_launch_info() == unmeasured
    for i in range(36):
        for out in outs:   # two output arrays, measured independently
            out.zero_()
            torch.cuda.synchronize()   # the context launches on its own stream
            c.oligo(bases, offsets, n, k, out, dtype="f32")
            torch.cuda.synchronize()
            assert torch.equal(out, ref), i
            info = c.oligo_launch_info()
            assert info["measured"] == (i >= 24 + 9 - 1), (i, info)   # WARM launches, then nine trials
    for out in outs:
        c.oligo(bases, offsets, n, k, out, dtype="f32")
        torch.cuda.synchronize()
        info = c.oligo_launch_info()
        ns = info["ns_per_read"]
        assert info["measured"] and all(0.05 < v < 1.0 for v in ns.values()), info   # ~0.2 ns per read
        best = min(ns, key=ns.get)
        want = best if ns[best] < 0.99 * ns[96] else 96
        assert info["wgs_per_slot"] == want, info
    # a caller comparing shapes itself: forced shapes give the same rows and leave the measurement alone
    for mode in (32, 200, 0):
        c.oligo_tuning(mode)
        outs[1].zero_()
        torch.cuda.synchronize()
        c.oligo(bases, offsets, n, k, outs[1], dtype="f32")
        torch.cuda.synchronize()
        assert torch.equal(outs[1], ref), mode
    c.oligo_tuning(1)
    assert c.oligo_launch_info() == info
    # small launches neither measure nor are affected
    c2 = device.Context()
    for _ in range(30):
        c2.oligo(bases, offsets, 100_000, k, outs[0], dtype="f32")
    torch.cuda.synchronize()
    assert c2.oligo_launch_info() == unmeasured
    # KT_OLIGO_TUNE=0: the default stays
    monkeypatch.setenv("KT_OLIGO_TUNE", "0")
    c3 = device.Context()
    for _ in range(20):
        c3.oligo(bases, offsets, n, k, outs[0], dtype="f32")
        torch.cuda.synchronize()
    assert c3.oligo_launch_info() == unmeasured
    for x in (c, c2, c3, c0):
        x.close()


def test_ctr_k31_large_checksums(torch_mod, ctx, oracle):
    """ctr k=31 on 0.5 M x 150 bp genome-sampled reads: distinct / sum(count) / sum(key*count)
    checksums against the oracle, and export == re-import idempotence"""
    torch = torch_mod
    from kmertools_amd import device
    n, L, k, seed, G = 500_000, 150, 31, 0x6b6d6572 + 3, 1_000_000
    bases = torch.empty(n * L, dtype=torch.uint8, device="cuda")
    offsets = torch.empty(n + 1, dtype=torch.int64, device="cuda")
    ctx.synth_reads(seed, n, L, bases, offsets, genome_len=G)
    ctr = device.Counter(ctx, k, 1 << 27)
    ctr.add_reads(bases, offsets, n)
    distinct = ctr.size()
    keys = torch.empty(distinct, dtype=torch.int64, device="cuda")
    counts = torch.empty(distinct, dtype=torch.int32, device="cuda")
    assert ctr.export(keys, counts, distinct) == distinct
    total = int(counts.to(torch.int64).sum())
    assert total == n * (L - k + 1)
    hb, ho = oracle.synth_reads(seed, n, L, genome_len=G)
    wk, wc = oracle.count_reads(hb, ho, k, n_parts=8, threads=8)
    assert distinct == len(wk)
    gk = keys.cpu().numpy().view(np.uint64)
    gc = counts.cpu().numpy().view(np.uint32)
    order = np.argsort(gk)
    assert np.array_equal(gk[order], wk) and np.array_equal(gc[order], wc)
    # checksum of checksums (wraps mod 2^64 on both sides)
    assert int((gk * gc.astype(np.uint64)).sum()) == int((wk * wc.astype(np.uint64)).sum())
    # merge idempotence: importing the exported pairs into an empty table reproduces it
    ctr2 = device.Counter(ctx, k, 1 << 27)
    ctr2.add_pairs(keys, counts, distinct)
    assert ctr2.size() == distinct
    ctr.close()
    ctr2.close()


# ---------------------------------------------------------------------------------------------
# N > 1 path on one GPU: two ranks share cuda:0, route on the GPU, exchange (gloo, host-staged),
# count on the GPU.  Union of the shards must equal the oracle's counts of all reads.

_SHARD_CASES = {"genome": (2, 31), "skewed": (2, 31), "narrow3": (3, 15), "flood": (2, 31), "flood3": (3, 21), "localfail": (2, 31),
                "uneven3": (3, 21), "empty_rank": (3, 31), "k10": (2, 10), "probing": (2, 25), "five": (5, 27),
                "unlike": (2, 31), "eight": (8, 31), "uniform": (2, 31)}   # case -> (ranks, k)


def _shard_batch(case, rank, n, L, synth):
    """rank's reads for a sharded-counter case: (bases, offsets, reads to use) - `synth(first_read)` makes n reads"""
    bases, offsets = synth(rank * n)
    nr = n
    if case == "skewed" and rank == 1:
        bases[: 8000 * L] = ord("A")           # 40 % of rank 1's batch is one k-mer: one owner gets all of its records
    if case.startswith("flood"):
        # rank 1: 19 000 reads of one k-mer and 1000 ordinary ones, the others 2000 ordinary reads - the ordinary records fit
        # the 40-block regions of these cases several times over, the flood is seven times a region's room
        if rank == 1:
            bases[: 19000 * L] = ord("A")
        else:
            nr = 2000
    if case == "uneven3":
        nr = n // (rank + 1)
    if case == "empty_rank" and rank == 1:
        nr = 0
    return bases, offsets, nr


def _two_rank_worker(rank, port, q, case):
    import os
    import torch
    import torch.distributed as dist
    world, k = _SHARD_CASES[case]
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    if case != "probing":
        os.environ["KT_BULK_MIN_BASES"] = "0"   # what arrives takes the partition + range build even at this size
    if case in ("narrow3", "flood3"):
        os.environ["KT_SHARD_SLICES"] = "3"
    if case == "five":
        os.environ["KT_SHARD_SLICES"] = "1"
    if case.startswith("flood"):
        os.environ["KT_SHARD_ROOM_BLOCKS"] = "40"   # 40 960 records of room per owner: the flooded owner's region overflows
    if case == "localfail":
        os.environ["KT_SHARD_FAIL_LOCAL"] = "1:1"   # rank 1's second call fails while it sets the batch up
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from kmertools_amd import device, dist as ktdist
        torch.cuda.set_device(0)
        ctx = device.Context(0, stream=torch.cuda.current_stream().cuda_stream)
        n, L = 20000, 150

        def synth(first):
            bases = torch.empty(n * L, dtype=torch.uint8, device="cuda")
            offsets = torch.empty(n + 1, dtype=torch.int64, device="cuda")
            ctx.synth_reads(4242, n, L, bases, offsets, noise=case != "uniform", genome_len=0 if case == "uniform" else 200000, first_read=first)
            return bases, offsets
        bases, offsets, nr = _shard_batch(case, rank, n, L, synth)
        if case == "unlike":
            # the ranks made their counters for different batch sizes: EVERY rank must say so at the first batch - in the
            # same round of the exchange - and none may be left waiting
            from kmertools_amd import _lib
            sc = ktdist.ShardedCounter(ctx, k, 1 << 23, group=dist.group.WORLD, max_batch_bases=n * L * (1 + 7 * rank))
            try:
                sc.add_reads(bases, offsets, n)
                raise AssertionError("rank %d did not notice that the counters differ" % rank)
            except _lib.KmertoolsError as e:
                assert e.code == _lib.KT_ERR_ARG and "differ" in str(e), (rank, e.code, str(e))
            sc.close()
            q.put((rank, None, None, 0, 1, True))
            ctx.close()
            return
        sc = ktdist.ShardedCounter(ctx, k, 1 << 23, group=dist.group.WORLD, max_batch_bases=n * L)
        # uneven3: the ranks' batches differ in size; empty_rank: one rank has no reads at all (it still takes part, and
        # still counts what the others send it)
        sc.add_reads(bases[: nr * L], offsets[: nr + 1], nr)
        m = 100 if rank == 0 else 0                 # a second "chunk" that only rank 0 has reads for
        if case == "localfail":
            # one rank cannot take part (a local failure ahead of the exchange): EVERY rank must come back with an error -
            # none may be left waiting in the exchange - nothing of the batch is counted, and the counter goes on working
            from kmertools_amd import _lib
            try:
                sc.add_reads(bases[: 100 * L], offsets[:101], m)
                raise AssertionError("the injected failure was not reported on rank %d" % rank)
            except _lib.KmertoolsError as e:
                assert e.code == (_lib.KT_ERR_FULL if rank == 1 else _lib.KT_ERR_ARG), (rank, e.code, str(e))
        sc.add_reads(bases[: 100 * L], offsets[:101], m)
        sc.finalize()
        keys, counts = sc.export_local()
        total = sc.size_global()
        mine = all(sc.sharded.owner_of(int(x)) == rank for x in keys[:300])
        sent = sc.sharded.exchanged_bytes()
        sc.close()
        q.put((rank, keys, counts, total, sent, mine))
        ctx.close()
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("case", sorted(_SHARD_CASES))
def test_two_ranks_one_gpu_sharded_ctr(oracle, case):
    """the C ABI's sharded counter with several ranks on cuda:0 and the host all-to-all transport over gloo: the route
    pass on the GPU (owner by minimiser, records of at most 8 k-mers), the exchange of the owners' regions in pieces,
    the ordinary partition + range build over the records that arrived, finalize; the union of the shards is the oracle's
    table of all reads and every k-mer lies on the rank its minimiser gives it (the library's host function AND
    tests/shard_ref.py's restatement).  `skewed`: 40 % of a rank's batch is one k-mer; `flood` / `flood3`: the same with
    regions of 40 blocks, so that the flooded owner's region overflows - the pending table and several finalize rounds
    run; `narrow3`: three ranks, three pieces, k=15 (32-bit keys through the partition, w = 8); `k10`: w = 2, `five`: five
    ranks, one piece, k=27; `probing`: the batch is below the partition passes' size, the records take the probing
    path; `eight`: eight ranks; `uniform`: i.i.d. reads without noise (BASELINE's distribution); `localfail`: one rank's batch set-up fails (injected) - every rank returns an error, nobody hangs, the next call
    works; `uneven3`: three ranks whose batches differ in size; `empty_rank`: a rank without reads; `unlike`: counters
    made for different batch sizes - every rank reports it, nobody hangs"""
    import os
    import socket
    import sys
    import torch.multiprocessing as mp
    from kmertools_amd import device
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import shard_ref
    world, k = _SHARD_CASES[case]
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    mpctx = mp.get_context("spawn")
    q = mpctx.Queue()
    procs = [mpctx.Process(target=_two_rank_worker, args=(r, port, q, case)) for r in range(world)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=300) for _ in range(world)], key=lambda x: x[0])
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    if case == "unlike":
        return
    n, L = 20000, 150
    ctr = oracle.Counter(4)
    n_kmers = 0
    for rank in range(world):
        def synth(first):
            hb, ho = oracle.synth_reads(4242, n, L, noise=case != "uniform", genome_len=0 if case == "uniform" else 200000, first_read=first)
            return hb.copy(), ho
        hb, ho, nr = _shard_batch(case, rank, n, L, synth)
        ctr.add_reads(hb[: nr * L], ho[: nr + 1], k, threads=4)
        n_kmers += nr * (L - k + 1)
        if rank == 0:
            ctr.add_reads(hb[: 100 * L], ho[:101], k)
    wk, wc = ctr.export()
    keys = np.concatenate([r[1] for r in res])
    counts = np.concatenate([r[2] for r in res])
    for rank, rk, _, total, sent, mine in res:
        assert total == len(wk)
        assert mine                                      # every k-mer of a shard is owned by its rank (by its minimiser)
        assert all(device.shard_owner_of(int(x), k, world) == rank for x in rk[:300])
        assert np.all(shard_ref.owner_of_kmers(rk[:2000], k, world) == rank)
    order = np.argsort(keys)
    assert np.array_equal(keys[order], wk) and np.array_equal(counts[order], wc)
    if case == "genome":
        # what crossed between the ranks: 2-bit bases in records of up to 8 k-mers, not k-mers at 8 bytes - less than a third
        # of the raw keys' bytes even at this size (whole 10 KB blocks per piece; 1.7 bytes per k-mer at BASELINE sizes)
        # (finalize's one round of fixed-size messages - 1.5 MB per peer, empty here - is not records)
        sent = sum(r[4] for r in res) - world * (world - 1) * (8 + (1 << 17) + (1 << 16)) * 8
        assert 0 < sent < 0.25 * 8 * n_kmers * (world - 1) / world, (sent, n_kmers)
    if case == "empty_rank":
        # the rank without reads sent no records - only the words ahead of every batch and finalize's one round of (empty)
        # fixed-size messages - and still owns its share of the k-mers
        assert res[1][4] <= 2 * (8 + (1 << 17) + (1 << 16)) * 8 + 4096 and len(res[1][1]) > 0


@pytest.mark.parametrize("owners", [1, 8, 3])
def test_sharded_single_rank_through_rccl(torch_mod, ctx, oracle, monkeypatch, owners):
    """librccl really is loaded and driven from the C ABI: a one-rank communicator (ncclCommInitRank), and with
    KT_SHARD_FORCE=n the routed path (route into n owners' regions -> level 1 over the regions piece by piece -> range
    build) instead of the single-GPU shortcut - the launches a rank of n makes, all of them on this GPU; the table must be
    the oracle's, twice over (the second batch merges into a table that holds data)"""
    torch = torch_mod
    from kmertools_amd import device
    assert len(device.Sharded.unique_id()) == 128
    monkeypatch.setenv("KT_SHARD_FORCE", str(owners))
    monkeypatch.setenv("KT_BULK_MIN_BASES", "0")
    n, L, k = 30000, 150, 21
    bases = torch.empty(n * L, dtype=torch.uint8, device="cuda")
    offsets = torch.empty(n + 1, dtype=torch.int64, device="cuda")
    ctx.synth_reads(77, n, L, bases, offsets, noise=True, genome_len=300000)
    sh = device.Sharded(ctx, k, 1 << 23, n * L, 1, 0, None)
    hb, ho = oracle.synth_reads(77, n, L, noise=True, genome_len=300000)
    wk, wc = oracle.count_reads(hb, ho, k, n_parts=4, threads=4)
    for _ in range(2):
        sh.add_reads(bases, offsets, n)
        sh.finalize()
        gk, gc = sh.table.export_host()
        assert np.array_equal(gk, wk) and np.array_equal(gc, wc)
        sh.add_reads(bases, offsets, n)
        sh.finalize()
        gk, gc = sh.table.export_host()
        assert np.array_equal(gk, wk) and np.array_equal(gc, 2 * wc)
        # what a rank of `owners` would have sent: the regions of the other owners, whole blocks
        assert (sh.exchanged_bytes() > 0) == (owners > 1)
        sh.clear()
    sh.close()


_PIECE_K = 31
_piece_cache = {}


def _piece_batches(oracle):
    """the batches of test_sharded_piece_arithmetic_edges with the oracle's table of each - made once, never changed:
    zero reads; one read shorter than k (bases, no record); 40 ragged reads (less than a block of records per owner: most
    pieces are empty); 800 reads of 150 bases (a handful of blocks per owner); and, for the flood case, mostly poly-A (owner 0
    of 2) with (AC)n (owner 1 of 2: the region whose overflow the room cuts off what leaves)"""
    from kmertools_amd import device
    if not _piece_cache:
        rng = np.random.default_rng(20260)
        alpha = np.frombuffer(b"ACGT", np.uint8)
        lists = {"edges": [[], [b"ACGTTGCAAC"], ragged_reads(97, 40, max_len=120, special=False), _random_reads(98, 800)],
                 "flood": [[b"A" * 150] * 500 + [b"AC" * 75] * 400 + _random_reads(99, 100) +
                           [alpha[rng.integers(0, 4, size=int(n))].tobytes() for n in rng.integers(31, 90, size=50)]]}
        for name, seq_lists in lists.items():
            out = []
            for seqs in seq_lists:
                bases, offsets = device.to_csr(seqs) if seqs else (np.zeros(0, np.uint8), np.zeros(1, np.uint64))
                wk, wc = oracle.count_reads(bases, offsets, _PIECE_K) if seqs else (np.zeros(0, np.uint64), np.zeros(0, np.uint32))
                out.append((bases, offsets, wk, wc))
            _piece_cache[name] = out
    return _piece_cache


def _tables_added(ak, ac, bk, bc):
    """the sorted (k-mer, count) table of two such tables' sum"""
    keys, inv = np.unique(np.concatenate([ak, bk]), return_inverse=True)
    counts = np.zeros(len(keys), np.uint64)
    np.add.at(counts, inv, np.concatenate([ac, bc]).astype(np.uint64))
    return keys, counts.astype(np.uint32)


def _add_and_check(sh, batches, room):
    """every batch in turn into the counter `sh`: after each, what left (exchanged_bytes) is every block of the owners >= 1
    exactly once, the route pass saw the oracle's k-mers, and the finalized table is the oracle's of everything so far"""
    have_k, have_c = sh.table.export_host()
    for bases, offsets, wk, wc in batches:
        before = sh.exchanged_bytes()
        sh.add_reads_host(bases, offsets)
        rec, km = sh.route_stats()
        blocks = [-(-min(int(r), room) // 1024) for r in rec[1:]]
        assert sh.exchanged_bytes() - before == 10240 * sum(blocks), (rec, blocks)
        assert int(km.sum()) == int(wc.astype(np.uint64).sum())
        sh.finalize()
        have_k, have_c = _tables_added(have_k, have_c, wk, wc)
        gk, gc = sh.table.export_host()
        assert np.array_equal(gk, have_k) and np.array_equal(gc, have_c)
    return rec


@pytest.mark.parametrize("owners,slices,room_blocks", [(o, p, 0) for o in (1, 2, 7) for p in (1, 3, 64)] + [(2, 4, 2)])
def test_sharded_piece_arithmetic_edges(ctx, oracle, monkeypatch, owners, slices, room_blocks):
    """the pieces the regions are counted in, at the edges of their arithmetic (one process, KT_SHARD_FORCE): 1, 3 and 64
    pieces - 64 is the clamp, more pieces than any region here has blocks - of 1, 2 and 7 owners' regions that hold no
    record, less than a block, a few blocks; through the range build (KT_BULK_MIN_BASES=0) and then, on the same counter,
    through the probing path, which counts every run behind the last piece.  Regions hold 65 blocks at least: nothing
    overflows, min(records, room) is the records - but in the last case, regions of two blocks that a batch of mostly
    poly-A overflows: what leaves is the room's two blocks, the rest is counted aside and delivered by finalize."""
    from kmertools_amd import device
    batches = _piece_batches(oracle)["flood" if room_blocks else "edges"]
    room = (room_blocks or 65) * 1024
    monkeypatch.setenv("KT_SHARD_FORCE", str(owners))
    monkeypatch.setenv("KT_SHARD_SLICES", str(slices))
    if room_blocks:
        monkeypatch.setenv("KT_SHARD_ROOM_BLOCKS", str(room_blocks))
    sh = device.Sharded(ctx, _PIECE_K, 1 << 21, max(int(b[1][-1]) for b in batches), 1, 0, None)
    monkeypatch.setenv("KT_BULK_MIN_BASES", "0")
    rec = _add_and_check(sh, batches, room)
    assert len(rec) == owners and (int(rec[1]) > room if room_blocks else int(rec.max()) < room)
    monkeypatch.delenv("KT_BULK_MIN_BASES")
    _add_and_check(sh, batches, room)
    sh.close()


def test_route_pass_records_match_restatement(torch_mod, ctx, oracle, monkeypatch):
    """the route pass over ragged reads (N runs, lower case, raw codes, reads shorter than k, a 9000-base read, poly-A and
    ACGT-repeat reads longer than a segment - runs of one owner that span whole threads and segments) into 1 .. 7 owners'
    regions, counted: the oracle's table for every window / minimiser shape (w = 16, 8, 4, 2, 1; k <= 8: the k-mer is its
    own minimiser), whatever the cut into records"""
    torch = torch_mod
    from kmertools_amd import device
    monkeypatch.setenv("KT_BULK_MIN_BASES", "0")
    seqs = ragged_reads(4321, 600) + [b"A" * 20000, b"ACGT" * 3000, b"", b"ACG", b"N" * 100, ragged_reads(5, 1)[0] * 40]
    bases, offsets = device.to_csr(seqs)
    for k, owners in ((31, 7), (23, 2), (22, 5), (15, 3), (11, 4), (9, 2), (8, 3), (5, 2), (1, 2), (31, 1)):
        monkeypatch.setenv("KT_SHARD_FORCE", str(owners))
        sh = device.Sharded(ctx, k, 1 << 21, int(offsets[-1]), 1, 0, None)
        sh.add_reads_host(bases, offsets)
        sh.finalize()
        gk, gc = sh.table.export_host()
        wk, wc = oracle.count_reads(bases, offsets, k)
        assert np.array_equal(gk, wk) and np.array_equal(gc, wc), (k, owners)
        sh.close()


# ---------------------------------------------------------------------------------------------
# bulk table construction (kt_bulk.hip): partition + LDS build must give exactly the table the
# incremental (atomic) path gives, and incremental adds must keep working on top of it

@pytest.mark.parametrize("k,cap_request", [(31, 3 << 16), (21, 190_000), (15, 390_000), (9, 190_000), (31, 3 << 19), (31, 320_000), (21, 450_000)])
def test_ctr_odd_capacity_requests(hctx, oracle, monkeypatch, k, cap_request):
    """capacity requests that are not powers of two (the library rounds them up to 5..8 eighths of one): bulk build, incremental adds on
    top, look-ups (cov) and the incremental path alone"""
    from kmertools_amd import device
    seqs = ragged_reads(7000 + k, 450)
    seqs += seqs[10:60] + [b"A" * 2000, b"ACGT" * 500]
    bases, offsets = device.to_csr(seqs)
    wk, wc = oracle.count_reads(bases, offsets, k)
    assert len(wk) < 0.55 * cap_request
    oc = oracle.Counter(1)
    oc.add_reads(bases, offsets, k)
    for bulk in ("0", str(1 << 40)):          # bulk build, then atomics only
        monkeypatch.setenv("KT_BULK_MIN_BASES", bulk)
        ctr = device.Counter(hctx, k, cap_request)
        cap = ctr.capacity()
        assert cap_request <= cap <= 1.25 * cap_request and (cap & (cap - 1) == 0 or (cap >> (cap.bit_length() - 3)) in (5, 6, 7))
        ctr.add_reads_host(bases, offsets)
        gk, gc = ctr.export_host()
        assert np.array_equal(gk, wk) and np.array_equal(gc, wc)
        assert np.array_equal(ctr.cov_host(bases, offsets, 1, 12, False), oc.cov_batch(bases, offsets, k, 1, 12, False))
        ctr.add_reads_host(bases, offsets)
        gk, gc = ctr.export_host()
        assert np.array_equal(gk, wk) and np.array_equal(gc, 2 * wc)
        ctr.close()


@pytest.mark.parametrize("k", [31, 16, 15, 5, 1])
def test_ctr_level1_over_packed_reads_and_over_staged_reads(hctx, oracle, monkeypatch, k):
    """the bulk build's level 1 reads the reads as a pass of their own packed them (pack_segments_kernel -> PackedSource: the
    default) or stages them itself (KT_BULK_PACK=0: ReadsSource): ragged noisy reads - N runs, lower case, raw codes, reads
    shorter than k, empty reads, reads that cross segments, a batch that ends inside a 32-base item - give the oracle's
    table either way, also with a second batch merged on top"""
    from kmertools_amd import device
    monkeypatch.setenv("KT_BULK_MIN_BASES", "0")
    seqs = ragged_reads(77 + k, 1500) + [b"ACGTN" * 1700, b"", b"AC", ragged_reads(3, 9)[8][:13]]
    bases, offsets = device.to_csr(seqs)
    assert len(bases) % 32 != 0 and len(bases) > 5 * 8192
    wk, wc = oracle.count_reads(bases, offsets, k)
    for pack in ("1", "0"):
        monkeypatch.setenv("KT_BULK_PACK", pack)
        ctr = device.Counter(hctx, k, 1 << 21)
        ctr.add_reads_host(bases, offsets)
        gk, gc = ctr.export_host()
        assert np.array_equal(gk, wk) and np.array_equal(gc, wc), (k, pack)
        ctr.add_reads_host(bases, offsets)
        gk, gc = ctr.export_host()
        assert np.array_equal(gk, wk) and np.array_equal(gc, 2 * wc), (k, pack)
        ctr.close()


@pytest.mark.parametrize("k", [8, 10, 12, 13])
def test_ctr_direct_addressed_tables(torch_mod, ctx, oracle, monkeypatch, capfd, k):
    """a table of exactly 4^k slots (k <= 15: the hash of a k-mer is a bijection onto the slots - ktd::nhash - and the bulk
    build's ranges are counters alone, keys coming back from the slots' indices): the oracle's table from ragged noisy
    reads with repeats, into the table and into an export target; look-ups, cov and a second batch on top (the dense table
    becomes a probing image under the same hash, the rebuild merges into it); the same with KT_BUILD_DIRECT=0 (probing
    build of the same geometry).  The job's verbose line names the build that ran."""
    torch = torch_mod
    from kmertools_amd import device
    monkeypatch.setenv("KT_BULK_MIN_BASES", "0")
    monkeypatch.setenv("KT_BULK_VERBOSE", "1")
    rng = np.random.default_rng(k)
    seqs = ragged_reads(900 + k, 3000) + [b"ACGT" * 400, b"A" * 3000]
    bases, offsets = device.to_csr(seqs)
    wk, wc = oracle.count_reads(bases, offsets, k)
    oc = oracle.Counter(1)
    oc.add_reads(bases, offsets, k)
    probe = np.concatenate([wk[:: max(1, len(wk) // 500)], rng.integers(0, 4 ** k, size=300, dtype=np.uint64)])
    want_probe = np.array([dict(zip(wk.tolist(), wc.tolist())).get(int(x), 0) for x in probe], dtype=np.uint32)
    for direct in ("1", "0"):
        monkeypatch.setenv("KT_BUILD_DIRECT", direct)
        ctr = device.Counter(ctx, k, 4 ** k)
        assert ctr.capacity() == 4 ** k
        capfd.readouterr()
        ctr.add_reads_host(bases, offsets)
        lines = _bulk_lines(capfd)
        assert len(lines) == 1 and _field(lines[0], "build") == ("direct" if direct == "1" else "dense"), lines
        gk, gc = ctr.export_host()
        assert np.array_equal(gk, wk) and np.array_equal(gc, wc), (k, direct)
        assert np.array_equal(ctr.lookup_host(probe), want_probe)
        assert np.array_equal(ctr.cov_host(bases, offsets, 2, 9, False), oc.cov_batch(bases, offsets, k, 2, 9, False))
        ctr.add_reads_host(bases, offsets)      # on top: every range rebuilt from what it holds + the batch
        gk, gc = ctr.export_host()
        assert np.array_equal(gk, wk) and np.array_equal(gc, 2 * wc)
        ctr.close()
        # straight into an export target
        c2 = device.Counter(ctx, k, 4 ** k)
        xk = torch.zeros(len(wk) + 5, dtype=torch.int64, device="cuda")
        xc = torch.zeros(len(wk) + 5, dtype=torch.int32, device="cuda")
        c2.export_target(xk, xc, len(wk) + 5)
        db = torch.from_numpy(bases).cuda()
        do = torch.from_numpy(offsets.astype(np.int64)).cuda()
        capfd.readouterr()
        c2.add_reads(db, do, len(seqs))
        lines = _bulk_lines(capfd)
        assert len(lines) == 1 and _field(lines[0], "build") == ("direct-ext" if direct == "1" else "dense-ext"), lines
        d = c2.size()
        assert d == len(wk) and c2.export(xk, xc, len(wk) + 5) == d
        gk2 = xk[:d].cpu().numpy().view(np.uint64)
        order = np.argsort(gk2)
        assert np.array_equal(gk2[order], wk) and np.array_equal(xc[:d].cpu().numpy().view(np.uint32)[order], wc)
        assert np.array_equal(c2.lookup_host(probe), want_probe)
        c2.close()


@pytest.mark.parametrize("paged", ["1", "0"])
@pytest.mark.parametrize("k,log2cap", [(31, 17), (21, 18), (15, 19), (4, 14), (31, 20)])
def test_ctr_bulk_build_matches_oracle(hctx, oracle, monkeypatch, k, log2cap, paged):
    from kmertools_amd import device
    monkeypatch.setenv("KT_BULK_MIN_BASES", "0")       # force the bulk path on a small batch
    monkeypatch.setenv("KT_BULK_PAGED", paged)         # level 1 through pages (default) / through exact offsets
    seqs = ragged_reads(4000 + k + log2cap, 500)
    comp = bytes.maketrans(b"ACGTacgt", b"TGCAtgca")
    seqs += seqs[10:80] + [s.translate(comp)[::-1] for s in seqs[20:60]] + [b"A" * 3000, b"ACGT" * 700]
    bases, offsets = device.to_csr(seqs)
    wk, wc = oracle.count_reads(bases, offsets, k)
    assert len(wk) < 0.6 * (1 << log2cap)
    ctr = device.Counter(hctx, k, 1 << log2cap)
    ctr.add_reads_host(bases, offsets)                  # bulk (table empty)
    assert ctr.size() == len(wk)
    gk, gc = ctr.export_host()
    assert np.array_equal(gk, wk) and np.array_equal(gc, wc)
    assert wc.max() > 100                               # heavy hitters (poly-A, repeats) went through
    # incremental adds on top of a bulk-built table: lookups must find the bulk-placed keys
    ctr.add_reads_host(bases, offsets)
    gk, gc = ctr.export_host()
    assert np.array_equal(gk, wk) and np.array_equal(gc, 2 * wc)
    # clear + bulk again (no explicit table clear happens in between)
    ctr.clear()
    half = len(seqs) // 2
    b1, o1 = device.to_csr(seqs[:half])
    b2, o2 = device.to_csr(seqs[half:])
    ctr.add_reads_host(b1, o1)                          # bulk
    ctr.add_reads_host(b2, o2)                          # incremental
    gk, gc = ctr.export_host()
    assert np.array_equal(gk, wk) and np.array_equal(gc, wc)
    ctr.close()


def _bulk_lines(capfd):
    """the jobs' lines of KT_BULK_VERBOSE=1 since the last read of stderr, one per job"""
    return [l for l in capfd.readouterr().err.splitlines() if l.startswith("[bulk] k=")]


def _field(line, name):
    """the value of ` name=value` in a [bulk] line"""
    return dict(f.split("=", 1) for f in line.split() if "=" in f)[name]


def _level1_kernel(k, log2_slots, s1y=True):
    """the level-1 kernel a paged job launches, by the code's own rule (kt_bulk.hip, kt_bulk_job::level1_paged): scatter1y
    where KT_S1Y is on and Scatter1YShared<K, 1024>::bytes(B1) fits 160 KB of LDS, else scatter1x.  B1 as split_bits
    gives it without KT_BULK_B1: 13 hash bits per range, the rest halved between the levels."""
    key = 4 if k <= 16 else 8
    fb = log2_slots - 13
    b1 = min((fb + 1) // 2, 10)
    if fb >= 16 and fb - b1 < 9:
        b1 = fb - 9
    half_per = (32 if key == 4 else 16) // 2                      # half_per<K>(): keys per thread and round
    slots = (1024 * half_per + (1 << b1) * (16 // key - 1) + 63) // 64 * 64
    lds = 2 * slots * key + 1024 * (2 if key == 8 else 4) + 3 * 1024 * 4 + 16 * 4 + 16
    return "scatter1y" if s1y and lds <= 160 * 1024 else "scatter1x"


@pytest.mark.parametrize("k", [31, 15])
@pytest.mark.parametrize("shape", ["wide", "sets8", "sets2", "one_buffer", "one_buffer_sets8", "part2_small", "image"])
def test_ctr_bulk_kernel_shapes_and_odd_batches(hctx, oracle, monkeypatch, capfd, k, shape):
    """every shape of the partition kernels on batches that do not fill them: one short read, a batch of less than one
    segment, segments in numbers that are not a multiple of the four a level-1 workgroup takes, a read that ends a
    segment exactly, N runs, an empty read - and an empty batch.  wide = scatter1y (two sort buffers, the copy-out of a round
    spread over the next) + the 1024-thread part2 (default: a small batch appends through ONE cursor set), sets8 / sets2 =
    the cursor sets of a large batch forced on the small one (one per XCD / the XCDs folded onto two: lines dealt
    round-robin to the sets, tails padded, a set that runs out of its eighth of a region falls back to exact offsets),
    one_buffer = scatter1x (KT_S1Y=0: the shape 32-bit keys with 1024 buckets keep, whose two buffers do not fit the LDS),
    part2_small = the 512-thread level 2 for 64-bit keys, image = the
    probing image written at once instead of the dense state.  The job's verbose line names the kernels that ran: the
    level-1 kernel of the shape, the build of the shape, the sort-buffer level 2 (a fan-out of 4)."""
    from kmertools_amd import device
    monkeypatch.setenv("KT_BULK_MIN_BASES", "0")
    monkeypatch.setenv("KT_BULK_VERBOSE", "1")
    want_l1 = _level1_kernel(k, 18, s1y=not shape.startswith("one_buffer"))
    if k == 31:
        assert want_l1 == ("scatter1x" if shape.startswith("one_buffer") else "scatter1y")

    def l1_of(line):
        # forced cursor sets leave a set an eighth (a half) of a small batch's region: where one runs out, the job says
        # level1=exact - it has redone level 1 with exact offsets, and the table stays with them - and l1 must say the same
        return "exact" if "sets" in shape and "level1=exact" in line else want_l1
    if shape.startswith("one_buffer"):
        monkeypatch.setenv("KT_S1Y", "0")
    if "sets" in shape:
        monkeypatch.setenv("KT_S1X_SETS", shape.split("sets")[1])
    if shape == "part2_small":
        monkeypatch.setenv("KT_P2_BIG64", "0")
        monkeypatch.setenv("KT_P2_BIG32", "1")
    if shape == "image":
        monkeypatch.setenv("KT_BULK_DENSE", "0")
    rng = np.random.default_rng(77 + k)
    acgt = np.frombuffer(b"ACGT", np.uint8)

    def read(n):
        return bytes(rng.choice(acgt, size=n))
    batches = [
        [read(k)],                                            # one k-mer
        [read(k - 1), b"", read(40)],                         # a read too short for a k-mer, an empty read
        [read(8192), read(8192 - 7), read(7)],                # reads ending on / straddling segment boundaries
        [read(300) for _ in range(137)],                      # 5.02 segments
        [read(150) + b"NNNN" + read(90) for _ in range(400)],  # ~12 segments, N runs
        [read(1000) for _ in range(74)],                      # 9.03 segments
    ]
    for seqs in batches:
        bases, offsets = device.to_csr(seqs)
        wk, wc = oracle.count_reads(bases, offsets, k)
        ctr = device.Counter(hctx, k, 1 << 18)
        assert ctr.capacity() == 1 << 18
        capfd.readouterr()
        ctr.add_reads_host(bases, offsets)
        lines = _bulk_lines(capfd)
        assert len(lines) == 1, lines
        assert _field(lines[0], "l1") == l1_of(lines[0])
        assert _field(lines[0], "build") == ("image" if shape == "image" else "dense")
        if shape == "part2_small":
            assert _field(lines[0], "l2") == "fast"
        assert ctr.size() == len(wk)
        gk, gc = ctr.export_host()
        assert np.array_equal(gk, wk) and np.array_equal(gc, wc)
        ctr.add_reads_host(bases, offsets)                    # and on top of itself (merge or probing path)
        for line in _bulk_lines(capfd):                       # (merge: the bulk path again)
            assert _field(line, "l1") == l1_of(line) and _field(line, "build") == "merge"
        gk, gc = ctr.export_host()
        assert np.array_equal(gk, wk) and np.array_equal(gc, 2 * wc)
        ctr.close()
    ctr = device.Counter(hctx, k, 1 << 18)                    # an empty batch leaves an empty table
    ctr.add_reads_host(np.zeros(0, np.uint8), np.zeros(1, np.uint64))
    assert ctr.size() == 0
    ctr.close()


@pytest.mark.parametrize("k", [31, 15])
def test_ctr_bulk_build_skewed_batch_falls_back(hctx, oracle, monkeypatch, k):
    """a batch dominated by one k-mer overflows its paged level-1 bucket: the build must notice and redo level 1
    with exact offsets; the table keeps working (and stops trying pages) afterwards"""
    from kmertools_amd import device
    monkeypatch.setenv("KT_BULK_MIN_BASES", "0")
    seqs = [b"A" * 6000] * 60 + ragged_reads(99 + k, 300) + [b"ACGT" * 2000] * 20
    bases, offsets = device.to_csr(seqs)
    wk, wc = oracle.count_reads(bases, offsets, k)
    assert wc.max() > 300_000
    ctr = device.Counter(hctx, k, 1 << 19)
    for _ in range(2):
        ctr.add_reads_host(bases, offsets)
        gk, gc = ctr.export_host()
        assert np.array_equal(gk, wk) and np.array_equal(gc, wc)
        ctr.clear()
    ctr.close()


@pytest.mark.parametrize("k,repeat", [(31, 600), (15, 600), (31, 60000)])
def test_ctr_bulk_build_heavy_hitters_in_fixed_regions(hctx, oracle, monkeypatch, capfd, k, repeat):
    """k-mers that occur far more often than a fine bucket's fixed room: level 2 notices that a fine bucket outgrows
    its room and redoes that level-1 bucket with exact boundaries; a level-1 region that overflows redoes level 1"""
    from kmertools_amd import device
    monkeypatch.setenv("KT_BULK_MIN_BASES", "0")
    monkeypatch.setenv("KT_BULK_VERBOSE", "1")
    rng = np.random.default_rng(5 + k)
    seqs = [bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), size=1000)) for _ in range(400)]
    seqs += [bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), size=40)) * repeat for _ in range(4)]
    bases, offsets = device.to_csr(seqs)
    wk, wc = oracle.count_reads(bases, offsets, k)
    ctr = device.Counter(hctx, k, 1 << 21)
    capfd.readouterr()
    ctr.add_reads_host(bases, offsets)
    lines = [l for l in capfd.readouterr().err.splitlines() if l.startswith("[bulk]")]
    gk, gc = ctr.export_host()
    assert np.array_equal(gk, wk) and np.array_equal(gc, wc)
    assert len(lines) == 1
    if repeat == 600:
        assert "level1=paged level2=fixed" in lines[0]
    ctr.close()


@pytest.mark.parametrize("k", [31, 15])
@pytest.mark.parametrize("mix", ["uniform", "heavy"])
def test_ctr_level2_write_combining_small(hctx, oracle, monkeypatch, capfd, k, mix):
    """part2_swwc_kernel, and behind it part2_exact_kernel over the buckets it gave up, at the smallest shape that selects
    it: level 2 writes whole lines out of LDS only for fan-outs of 512 and more, which the default split of the hash bits
    reaches at 2^31 slots.  KT_BULK_B1=1 on a table of 2^23 slots (128 MB) gives 10 fine bits, b1 = 1, b2 = 9: B1 = 2,
    B2 = 512.  (B1 = 2 is within what the kernels take: scatter1y / scatter1x mask a digit with B1 - 1 and guard their
    per-bucket work with d < B1, their scan takes any count of buckets, xcd_tails and level 2 loop over B1 buckets, and
    digit1h needs b1 >= 1 only - a power of two is all they ask.)
    uniform: 300 random reads of 1000 bases, about 285 keys for each fine bucket's 336 keys of room.  heavy: four reads of
    one 40-mer 600 times on top, so that some fine buckets outgrow their room and their level-1 buckets are redone with
    exact boundaries - still the swwc choice, the redo is part of it.  Then the same batch on top: a merge."""
    from kmertools_amd import device
    monkeypatch.setenv("KT_BULK_MIN_BASES", "0")
    monkeypatch.setenv("KT_BULK_VERBOSE", "1")
    monkeypatch.setenv("KT_BULK_B1", "1")
    monkeypatch.setenv("KT_BULK_MERGE_DIV", "1000000000")   # (the second batch rebuilds the ranges whatever its size)
    rng = np.random.default_rng(300 + k)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    seqs = [bytes(rng.choice(acgt, size=1000)) for _ in range(300)]
    if mix == "heavy":
        seqs += [bytes(rng.choice(acgt, size=40)) * 600 for _ in range(4)]
    bases, offsets = device.to_csr(seqs)
    wk, wc = oracle.count_reads(bases, offsets, k)
    assert (wc.max() > 500) == (mix == "heavy")
    ctr = device.Counter(hctx, k, 1 << 23)
    assert ctr.capacity() == 1 << 23
    capfd.readouterr()
    ctr.add_reads_host(bases, offsets)
    lines = _bulk_lines(capfd)
    assert len(lines) == 1, lines
    assert _field(lines[0], "l2") == "swwc" and _field(lines[0], "build") == "dense"
    assert ctr.size() == len(wk)
    gk, gc = ctr.export_host()
    assert np.array_equal(gk, wk) and np.array_equal(gc, wc)
    ctr.add_reads_host(bases, offsets)
    lines = _bulk_lines(capfd)
    assert len(lines) == 1, lines
    assert _field(lines[0], "l2") == "swwc" and _field(lines[0], "build") == "merge"
    gk, gc = ctr.export_host()
    assert np.array_equal(gk, wk) and np.array_equal(gc, 2 * wc)
    ctr.close()


@pytest.mark.parametrize("k", [31, 15])
@pytest.mark.parametrize("mix", ["uniform", "heavy"])
@pytest.mark.parametrize("log2_slots,B2", [(24, 1024), (25, 2048)])
def test_ctr_level2_fan_outs_of_huge_tables_small(hctx, oracle, monkeypatch, capfd, k, mix, log2_slots, B2):
    """the level-2 fan-outs that only tables of 2^33 and 2^34 slots select by default, 1024 and 2048, at the smallest shapes
    that give them: KT_BULK_B1=1 on 2^24 slots (256 MB) leaves level 2 ten hash bits, on 2^25 slots (512 MB) eleven.  The
    line's l2= is what tests/big_tables.py restates of kt_bulk_job (level2_of): one line per fine bucket in LDS where
    SwwcShared<K>::bytes(B2) fits 160 KB - 1024 buckets do, 2048 do not: the sort-buffer kernel -, behind a paged level 1
    that left every fine bucket a cache line of fixed room or more.  600 random reads of 1000 bases: 290 (145) keys per
    fine bucket for 320 (160) keys of room, so some buckets outgrow it and are redone with exact boundaries; heavy: four
    reads of one 40-mer 600 times on top.  Then the same batch merged on top."""
    import big_tables as bt
    from kmertools_amd import device
    monkeypatch.setenv("KT_BULK_MIN_BASES", "0")
    monkeypatch.setenv("KT_BULK_VERBOSE", "1")
    monkeypatch.setenv("KT_BULK_B1", "1")
    monkeypatch.setenv("KT_BULK_MERGE_DIV", "1000000000")
    rng = np.random.default_rng(700 + k + log2_slots)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    seqs = [bytes(rng.choice(acgt, size=1000)) for _ in range(600)]
    if mix == "heavy":
        seqs += [bytes(rng.choice(acgt, size=40)) * 600 for _ in range(4)]
    bases, offsets = device.to_csr(seqs)
    wk, wc = oracle.count_reads(bases, offsets, k)
    assert (wc.max() > 500) == (mix == "heavy")
    assert bt.split_bits(log2_slots, 1) == (1, B2.bit_length() - 1)
    want_l2 = "swwc" if bt.swwc_lds(B2) <= 160 * 1024 else "fast"
    assert want_l2 == {1024: "swwc", 2048: "fast"}[B2]
    ctr = device.Counter(hctx, k, 1 << log2_slots)
    assert ctr.capacity() == 1 << log2_slots
    capfd.readouterr()
    ctr.add_reads_host(bases, offsets)
    lines = _bulk_lines(capfd)
    assert len(lines) == 1, lines
    assert _field(lines[0], "l2") == want_l2 == bt.level2_of_line(lines[0], log2_slots, 8 if k > 16 else 4, 1), lines
    assert _field(lines[0], "build") == "dense"
    assert ctr.size() == len(wk)
    gk, gc = ctr.export_host()
    assert np.array_equal(gk, wk) and np.array_equal(gc, wc)
    ctr.add_reads_host(bases, offsets)
    lines = _bulk_lines(capfd)
    assert len(lines) == 1, lines
    assert _field(lines[0], "l2") == want_l2 == bt.level2_of_line(lines[0], log2_slots, 8 if k > 16 else 4, 1), lines
    assert _field(lines[0], "build") == "merge"
    gk, gc = ctr.export_host()
    assert np.array_equal(gk, wk) and np.array_equal(gc, 2 * wc)
    ctr.close()


@pytest.mark.parametrize("k", [31, 15])
def test_ctr_bulk_build_deep_coverage(hctx, oracle, monkeypatch, capfd, k):
    """few distinct k-mers, each seen hundreds of times (deep coverage of a small genome): fine buckets are far from
    evenly filled, so the fixed-room attempt of level 2 gives way to exact boundaries bucket by bucket"""
    from kmertools_amd import device
    monkeypatch.setenv("KT_BULK_MIN_BASES", "0")
    monkeypatch.setenv("KT_BULK_VERBOSE", "1")
    rng = np.random.default_rng(70 + k)
    genome = rng.choice(np.frombuffer(b"ACGT", np.uint8), size=3000)
    at = rng.integers(0, len(genome) - 100, size=30000)
    seqs = [bytes(genome[a:a + 100]) for a in at]
    bases, offsets = device.to_csr(seqs)
    wk, wc = oracle.count_reads(bases, offsets, k)
    assert len(wk) < 6100 and np.median(wc) > 100
    ctr = device.Counter(hctx, k, 1 << 20)
    capfd.readouterr()
    ctr.add_reads_host(bases, offsets)
    lines = [l for l in capfd.readouterr().err.splitlines() if l.startswith("[bulk]")]
    gk, gc = ctr.export_host()
    assert np.array_equal(gk, wk) and np.array_equal(gc, wc)
    assert len(lines) == 1      # (level 1 may or may not have fitted its regions; level 2 never needs a second build)
    ctr.close()


@pytest.mark.parametrize("k,log2cap", [(31, 18), (15, 19), (9, 18)])
def test_ctr_bulk_build_from_routed_keys(hctx, oracle, monkeypatch, k, log2cap):
    """kt_ctr_add_pairs(keys, counts=NULL) into an empty table = what a GPU does with the k-mers routed to it:
    takes the bulk path too (duplicates, KT_EMPTY_KEY padding and a ragged tail included)"""
    from kmertools_amd import device
    monkeypatch.setenv("KT_BULK_MIN_BASES", "0")
    seqs = ragged_reads(5000 + k, 600)
    bases, offsets = device.to_csr(seqs + seqs[:100])
    f, r, _ = hctx.kmers_host(bases, offsets, k)
    canon = np.minimum(f, r)
    keys = np.concatenate([canon, np.full(777, 0xFFFFFFFFFFFFFFFF, np.uint64), canon[:5000]])
    rng = np.random.default_rng(k)
    rng.shuffle(keys)
    wk, wc = np.unique(np.concatenate([canon, canon[:5000]]), return_counts=True)
    assert len(wk) < 0.6 * (1 << log2cap)
    ctr = device.Counter(hctx, k, 1 << log2cap)
    ctr.add_pairs_host(keys, None)                      # bulk (table empty, no counts)
    gk, gc = ctr.export_host()
    assert np.array_equal(gk, wk) and np.array_equal(gc, wc.astype(np.uint32))
    ctr.add_pairs_host(keys, None)                      # incremental on top
    gk, gc = ctr.export_host()
    assert np.array_equal(gk, wk) and np.array_equal(gc, (2 * wc).astype(np.uint32))
    ctr.close()


def _random_reads(seed, n, L=150):
    rng = np.random.default_rng(seed)
    alpha = np.frombuffer(b"ACGT", np.uint8)
    return [alpha[rng.integers(0, 4, size=L)].tobytes() for _ in range(n)]


@pytest.mark.parametrize("k,log2cap,load", [(31, 15, 0.5), (31, 15, 0.8), (31, 16, 0.92), (31, 17, 0.93), (15, 15, 0.9),
                                            (21, 17, 0.94)])
def test_ctr_range_build_high_load(hctx, oracle, monkeypatch, k, log2cap, load):
    """the range build places keys where range-circular linear probing would (kt_table.hpp) at any load factor:
    the export is the oracle's table, every key is found again by the lookups of cov and by the probing insert path
    (entries that wrapped round the end of their range included), and the size counter follows"""
    from kmertools_amd import device
    monkeypatch.setenv("KT_BULK_MIN_BASES", "0")
    cap = 1 << log2cap
    n = int(load * cap / (150 - k + 1)) + 1
    seqs = _random_reads(1000 + k + log2cap, n)
    bases, offsets = device.to_csr(seqs)
    wk, wc = oracle.count_reads(bases, offsets, k)
    ctr = device.Counter(hctx, k, cap)
    assert ctr.capacity() == cap and abs(len(wk) / cap - load) < 0.03
    ctr.add_reads_host(bases, offsets)                      # range build
    assert ctr.size() == len(wk)
    gk, gc = ctr.export_host()
    assert np.array_equal(gk, wk) and np.array_equal(gc, wc)
    oc = oracle.Counter(1)
    oc.add_reads(bases, offsets, k)
    probe = _random_reads(77, 50) + seqs[::7]              # absent k-mers and present ones
    pb, po = device.to_csr(probe)
    want = oc.cov_batch(pb, po, k, 1, 8, True)
    got = ctr.cov_host(pb, po, 1, 8)
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64))
    monkeypatch.setenv("KT_BULK", "0")                      # the probing path on top of the built ranges
    ctr.add_reads_host(bases, offsets)
    assert ctr.size() == len(wk)
    gk, gc = ctr.export_host()
    assert np.array_equal(gk, wk) and np.array_equal(gc, 2 * wc)
    ctr.close()


@pytest.mark.parametrize("k,log2cap", [(31, 17), (15, 16), (21, 18)])
def test_ctr_range_rebuild_merges_batches(hctx, oracle, monkeypatch, k, log2cap):
    """batches after the first are merged by rebuilding every range from what it holds + the new keys (no per-k-mer
    atomics): four overlapping batches, a batch through the probing path in between, against the oracle"""
    from kmertools_amd import device
    monkeypatch.setenv("KT_BULK_MIN_BASES", "0")
    monkeypatch.setenv("KT_BULK_MERGE_DIV", "1000000000")   # every batch is worth a rebuild
    monkeypatch.setenv("KT_BULK_VERBOSE", "1")
    cap = 1 << log2cap
    per = int(0.17 * cap / (150 - k + 1))
    seqs = (ragged_reads(31 + k, 200, max_len=100 if log2cap < 18 else 400, special=log2cap >= 18)
            + _random_reads(5 + k, 4 * per) + [b"A" * 2000, b"ACGT" * 500])
    batches = [seqs[i::4] + seqs[:50] for i in range(4)]    # the first 50 reads are in every batch
    oc = oracle.Counter(3)
    ctr = device.Counter(hctx, k, cap)
    for i, b in enumerate(batches):
        bb, bo = device.to_csr(b)
        oc.add_reads(bb, bo, k)
        if i == 2:
            monkeypatch.setenv("KT_BULK", "0")              # one batch through the atomics, then rebuilds again
        ctr.add_reads_host(bb, bo)
        monkeypatch.setenv("KT_BULK", "1")
        wk, wc = oc.export()
        assert ctr.size() == len(wk)
        gk, gc = ctr.export_host()
        assert np.array_equal(gk, wk) and np.array_equal(gc, wc)
    assert 0.6 < len(wk) / cap < 0.9
    # routed keys (no counts) merge the same way
    f, r, _ = hctx.kmers_host(*device.to_csr(batches[0]), k)
    canon = np.minimum(f, r)
    ctr.add_pairs_host(canon, None)
    oc.add_pairs(canon, np.ones(len(canon), np.uint32))
    wk, wc = oc.export()
    gk, gc = ctr.export_host()
    assert np.array_equal(gk, wk) and np.array_equal(gc, wc)
    ctr.close()


@pytest.mark.parametrize("k", [31, 15])
def test_ctr_dense_table_state(hctx, oracle, monkeypatch, k):
    """KT_BULK_DENSE=1: a fresh range build leaves every range packed (no probing image): size and export read that
    directly, and the first thing that probes (cov, an incremental add, a merge) turns it into the image in place"""
    from kmertools_amd import device
    monkeypatch.setenv("KT_BULK_MIN_BASES", "0")
    monkeypatch.setenv("KT_BULK_DENSE", "1")
    monkeypatch.setenv("KT_BULK_VERBOSE", "1")
    seqs = ragged_reads(9 + k, 400) + _random_reads(k, 300) + [b"A" * 3000]
    bases, offsets = device.to_csr(seqs)
    wk, wc = oracle.count_reads(bases, offsets, k)
    for after in ("export", "cov", "atomic", "merge"):
        ctr = device.Counter(hctx, k, 1 << 18)
        ctr.add_reads_host(bases, offsets)
        assert ctr.size() == len(wk)
        if after == "cov":
            oc = oracle.Counter(1)
            oc.add_reads(bases, offsets, k)
            pb, po = device.to_csr(seqs[::5] + _random_reads(1, 20))
            got = ctr.cov_host(pb, po, 2, 6)
            assert np.array_equal(got.view(np.uint64), oc.cov_batch(pb, po, k, 2, 6, True).view(np.uint64))
        mult = 1
        if after in ("atomic", "merge"):
            monkeypatch.setenv("KT_BULK", "0" if after == "atomic" else "1")
            monkeypatch.setenv("KT_BULK_MERGE_DIV", "1000000000")
            ctr.add_reads_host(bases, offsets)
            monkeypatch.setenv("KT_BULK", "1")
            mult = 2
        gk, gc = ctr.export_host()
        assert np.array_equal(gk, wk) and np.array_equal(gc, mult * wc)
        assert ctr.size() == len(wk)
        ctr.close()


@pytest.mark.parametrize("k", [31, 15, 21])
def test_ctr_export_target(torch_mod, ctx, oracle, monkeypatch, capfd, k):
    """kt_ctr_export_target: the range build writes its packed (key, count) pairs straight into the caller's device
    arrays (no export pass); the table stays usable - size, export to the same or to other arrays, cov, further adds
    (probing path and range rebuild) first rebuild the probing image from those arrays; a target that is too small is
    reported, not silently truncated; the target is sticky across clears.  The job's verbose line names the build that
    produced the table: into the target, or - redone - into the table's own slots."""
    from kmertools_amd import device, _lib
    torch = torch_mod
    monkeypatch.setenv("KT_BULK_MIN_BASES", "0")
    monkeypatch.setenv("KT_BULK_VERBOSE", "1")
    seqs = ragged_reads(19 + k, 500) + _random_reads(k + 1, 400) + [b"C" * 2500] + _random_reads(k + 1, 50)
    hb, ho = device.to_csr(seqs)
    wk, wc = oracle.count_reads(hb, ho, k)
    bases = torch.from_numpy(hb).cuda()
    offsets = torch.from_numpy(ho.astype(np.int64)).cuda()
    n = len(seqs)
    room = len(wk) + 100
    xk = torch.full((room,), -1, dtype=torch.int64, device="cuda")
    xc = torch.zeros(room, dtype=torch.int32, device="cuda")

    def sorted_pairs(tk, tc, cnt):
        gk = tk[:cnt].cpu().numpy().view(np.uint64)
        gc = tc[:cnt].cpu().numpy().view(np.uint32)
        o = np.argsort(gk, kind="stable")
        return gk[o], gc[o]

    for after in ("same", "other", "host", "cov", "atomic", "merge", "retarget", "uneven"):
        if after == "uneven":
            # no scratch behind the arrays: the build notices that its blocks do not fit and is redone into the table
            monkeypatch.setenv("KT_EXT_OVF_BLOCKS", "1")
        ctr = device.Counter(ctx, k, 1 << 18)
        ctr.export_target(xk, xc, room)
        for rep in range(2):            # sticky: the second round (after a clear) takes the same road
            xk.fill_(-1)
            ctr.clear()
            capfd.readouterr()
            ctr.add_reads(bases, offsets, n)
            lines = _bulk_lines(capfd)
            assert len(lines) == 1 and _field(lines[0], "build") == ("dense" if after == "uneven" else "dense-ext"), lines
            assert ctr.size() == len(wk)
            got = ctr.export(xk, xc, room)
            assert got == len(wk)
            gk, gc = sorted_pairs(xk, xc, got)
            assert np.array_equal(gk, wk) and np.array_equal(gc, wc), (after, rep)
        mult = 1
        if after == "other":
            yk = torch.empty(room, dtype=torch.int64, device="cuda")
            yc = torch.empty(room, dtype=torch.int32, device="cuda")
            got = ctr.export(yk, yc, room)
            gk, gc = sorted_pairs(yk, yc, got)
            assert np.array_equal(gk, wk) and np.array_equal(gc, wc)
        elif after == "cov":
            oc = oracle.Counter(1)
            oc.add_reads(hb, ho, k)
            pb, po = device.to_csr(seqs[::7] + _random_reads(2, 20))
            got = ctr.cov_host(pb, po, 2, 6)
            assert np.array_equal(got.view(np.uint64), oc.cov_batch(pb, po, k, 2, 6, True).view(np.uint64))
        elif after in ("atomic", "merge"):
            monkeypatch.setenv("KT_BULK", "0" if after == "atomic" else "1")
            monkeypatch.setenv("KT_BULK_MERGE_DIV", "1000000000")
            before = xk.clone()
            ctr.add_reads(bases, offsets, n)                 # (rebuilds the probing image from the arrays first)
            assert bool((xk == before).all())                # a merge does not write to the export arrays ...
            xk.fill_(-1)                                     # ... and the table no longer refers to them
            monkeypatch.setenv("KT_BULK", "1")
            mult = 2
        elif after == "retarget":
            ctr.export_target(None, None, 0)                 # the table takes its own copy before the target goes away
            xk.fill_(-1)
        gk, gc = ctr.export_host()
        assert np.array_equal(gk, wk) and np.array_equal(gc, mult * wc), after
        assert ctr.size() == len(wk)
        ctr.close()
    monkeypatch.delenv("KT_EXT_OVF_BLOCKS")
    # too small: loud - the call that counted says so - the arrays are not written past their end, and the table is NOT
    # lost: its counts are in its own slots, size and an export into large enough arrays work
    for small in (len(wk) // 2, len(wk) - 1):
        sk = torch.full((len(wk),), -1, dtype=torch.int64, device="cuda")
        sc = torch.zeros(len(wk), dtype=torch.int32, device="cuda")
        ctr = device.Counter(ctx, k, 1 << 18)
        ctr.export_target(sk, sc, small)
        with pytest.raises(_lib.KmertoolsError) as e:
            ctr.add_reads(bases, offsets, n)
        assert e.value.code == _lib.KT_ERR_ARG
        assert int((sk[small:] != -1).sum()) == 0
        assert ctr.size() == len(wk)
        ctr.export_target(None, None, 0)
        gk, gc = ctr.export_host()
        assert np.array_equal(gk, wk) and np.array_equal(gc, wc)
        ctr.add_reads(bases, offsets, n)                     # ... and it is a table like any other afterwards
        gk, gc = ctr.export_host()
        assert np.array_equal(gk, wk) and np.array_equal(gc, 2 * wc)
        ctr.close()
    # arrays with slack and a scratch too small for the blocks of unevenly filled workgroups: the build must notice that
    # the patch pass cannot reach every block and fall back, not drop entries
    monkeypatch.setenv("KT_EXT_OVF_BLOCKS", "2")
    monkeypatch.setenv("KT_BUILD_WGS_EXT", "1")
    big = 8 * len(wk)
    bk = torch.full((big,), -1, dtype=torch.int64, device="cuda")
    bc = torch.zeros(big, dtype=torch.int32, device="cuda")
    ctr = device.Counter(ctx, k, 1 << 18)
    ctr.export_target(bk, bc, big)
    capfd.readouterr()
    ctr.add_reads(bases, offsets, n)
    lines = _bulk_lines(capfd)
    assert len(lines) == 1 and _field(lines[0], "build") == "dense", lines
    assert ctr.size() == len(wk)
    gk, gc = ctr.export_host()
    assert np.array_equal(gk, wk) and np.array_equal(gc, wc)
    ctr.close()
    monkeypatch.delenv("KT_EXT_OVF_BLOCKS")
    monkeypatch.delenv("KT_BUILD_WGS_EXT")


def test_ctr_range_build_full_table_is_loud(hctx, monkeypatch):
    """more distinct k-mers than slots: the range build must report KT_ERR_FULL, not drop keys or hang"""
    from kmertools_amd import device, _lib
    monkeypatch.setenv("KT_BULK_MIN_BASES", "0")
    seqs = _random_reads(3, 600)                             # 72 000 distinct 31-mers into 32 768 slots
    bases, offsets = device.to_csr(seqs)
    ctr = device.Counter(hctx, 31, 1 << 15)
    ctr.add_reads_host(bases, offsets)
    with pytest.raises(_lib.KmertoolsError) as e:
        ctr.size()
    assert e.value.code == _lib.KT_ERR_FULL
    ctr.close()


def test_ctr_bulk_overfull_ranges_spill(hctx, oracle, monkeypatch):
    """load factor ~0.85: keys run past the end of their range and wrap to its front"""
    from kmertools_amd import device
    monkeypatch.setenv("KT_BULK_MIN_BASES", "0")
    rng = np.random.default_rng(11)
    alpha = np.frombuffer(b"ACGT", np.uint8)
    seqs = [alpha[rng.integers(0, 4, size=150)].tobytes() for _ in range(470)]   # ~56 k distinct 31-mers
    bases, offsets = device.to_csr(seqs)
    wk, wc = oracle.count_reads(bases, offsets, 31)
    ctr = device.Counter(hctx, 31, 1 << 16)
    assert 0.8 < len(wk) / (1 << 16) < 0.95
    ctr.add_reads_host(bases, offsets)
    gk, gc = ctr.export_host()
    assert np.array_equal(gk, wk) and np.array_equal(gc, wc)
    ctr.close()


# ---------------------------------------------------------------------------------------------
# cov (kt_cov_batch): coverage/src/lib.rs:165-184 against the resident table
def test_cov_golden_files(hctx, oracle, golden):
    """k=4, bin_size 2, bin_count 3 on reads.fq = the reference's own test (coverage/src/lib.rs:196-242)"""
    from kmertools_amd import device
    recs = oracle.read_records(golden / "reads.fq")
    bases, offsets = oracle.to_csr([s for _, s in recs])
    ctr = device.Counter(hctx, 4, 4096)
    ctr.add_reads_host(bases, offsets)
    norm = ctr.cov_host(bases, offsets, 2, 3, True)
    assert oracle.oligo_text(norm, True) == (golden / "expected_counts.vectors").read_bytes()
    cnt = ctr.cov_host(bases, offsets, 2, 3, False)
    assert oracle.oligo_text(cnt, False) == (golden / "expected_counts_unnorm.vectors").read_bytes()
    u = ctr.cov_host(bases, offsets, 2, 3, False, dtype="u32")
    assert np.array_equal(u.astype(np.float64), cnt)
    ctr.close()


@pytest.mark.parametrize("k,bin_size,bin_count", [(7, 1, 5), (11, 2, 16), (15, 16, 16), (21, 3, 7), (31, 5, 64),
                                                   (9, 1, 1), (13, 1 << 33, 4), (12, 2, 700)])
def test_cov_vs_oracle(hctx, oracle, k, bin_size, bin_count):
    """ragged reads (empty, 1-base, N runs, lower case, >1 segment) counted from a DIFFERENT read set
    than the one that is vectorised, so absent k-mers (count 0) and repeats both occur"""
    from kmertools_amd import device
    table_reads = ragged_reads(100 + k, 300, max_len=600)
    query = table_reads[::2] + ragged_reads(200 + k, 200, max_len=300) + table_reads[:40] * 3
    tb, to = oracle.to_csr(table_reads * 2)  # every table k-mer at least twice
    qb, qo = oracle.to_csr(query)
    want_ctr = oracle.Counter(3)
    want_ctr.add_reads(tb, to, k)
    ctr = device.Counter(hctx, k, 1 << 20)
    ctr.add_reads_host(tb, to)
    for norm in (True, False):
        want = want_ctr.cov_batch(qb, qo, k, bin_size, bin_count, norm)
        got = ctr.cov_host(qb, qo, bin_size, bin_count, norm)
        assert got.shape == want.shape
        assert np.array_equal(got, want), (k, bin_size, bin_count, norm)
    got32 = ctr.cov_host(qb, qo, bin_size, bin_count, True, dtype="f32")
    assert np.abs(got32.astype(np.float64) - want_ctr.cov_batch(qb, qo, k, bin_size, bin_count, True)).max() <= 1e-6
    ctr.close()


@pytest.mark.parametrize("k,n_parts", [(15, 4), (31, 3), (9, 5)])
def test_cov_over_hash_partitions(hctx, oracle, monkeypatch, k, n_parts):
    """kt_cov_batch_part: a table that holds one hash partition of the k-mers (an out-of-core pass) answers for that
    partition only; the raw rows summed over the passes are the rows of the whole table (every k-mer binned once -
    absent k-mers too, by the pass their hash belongs to), host and device rows alike"""
    from kmertools_amd import device
    monkeypatch.setenv("KT_BULK_MIN_BASES", "0")
    seqs = ragged_reads(40 + k, 500) + _random_reads(k, 200)
    bases, offsets = device.to_csr(seqs)
    pb, po = device.to_csr(seqs[::3] + _random_reads(k + 1, 60) + [b"", b"ACG"])
    oc = oracle.Counter(1)
    oc.add_reads(bases, offsets, k)
    want = oc.cov_batch(pb, po, k, 3, 7, False).astype(np.uint32)
    n = len(po) - 1
    acc = np.zeros((n, 7), np.uint32)
    for part in range(n_parts):
        ctr = device.Counter(hctx, k, 1 << 18)
        ctr.add_reads_host(bases, offsets, n_parts, part)
        ctr.cov_part(pb if pb.size else np.zeros(1, np.uint8), po, n, 3, 7, acc, n_parts, part, mem=0)
        ctr.close()
    assert np.array_equal(acc, want)


def test_cov_tiny_reads_and_empty_table(hctx, oracle):
    """segments holding more bin cells than the LDS image (thousands of k-length reads) take the
    direct path; an empty table puts every k-mer in bin 0"""
    from kmertools_amd import device
    rng = np.random.default_rng(9)
    k = 9
    seqs = ["".join(rng.choice(list("ACGT"), size=int(L))) for L in rng.integers(0, 14, size=6000)]
    b, o = oracle.to_csr(seqs)
    want_ctr = oracle.Counter(1)
    want_ctr.add_reads(b, o, k)
    ctr = device.Counter(hctx, k, 1 << 18)
    got0 = ctr.cov_host(b, o, 1, 8, False)
    nk = np.array([max(0, len(s) - k + 1) for s in seqs], np.float64)
    assert np.array_equal(got0[:, 0], nk) and not got0[:, 1:].any()
    ctr.add_reads_host(b, o)
    for bc in (8, 40):
        assert np.array_equal(ctr.cov_host(b, o, 1, bc, True), want_ctr.cov_batch(b, o, k, 1, bc, True))
    with pytest.raises(Exception):
        ctr.cov_host(b, o, 0, 8)
    with pytest.raises(Exception):
        ctr.cov_host(b, o, 1, 0)
    with pytest.raises(Exception):
        ctr.cov_host(b, o, 1, 8, True, dtype="u32")
    assert ctr.cov_host(np.zeros(0, np.uint8), np.zeros(1, np.uint64), 1, 8).shape == (0, 8)
    ctr.close()


def test_cov_full_size_properties(torch_mod, ctx):
    """2 M x 150 bp genome-sampled reads, k=15: every row of raw counts sums to the read's k-mer
    count (136 here: ACGT-only reads), a read set vectorised against its own table never lands in
    bin 0 with bin_size 1, and the normalised rows are the raw rows / 136 bit-for-bit"""
    from kmertools_amd import device
    torch = torch_mod
    n, L, k = 2_000_000, 150, 15
    bases = torch.empty(n * L, dtype=torch.uint8, device="cuda")
    offsets = torch.empty(n + 1, dtype=torch.int64, device="cuda")
    ctx.synth_reads(11, n, L, bases, offsets, noise=False, genome_len=1 << 22)
    ctr = device.Counter(ctx, k, 1 << 26)
    ctr.add_reads(bases, offsets, n)
    raw = torch.empty((n, 16), dtype=torch.int32, device="cuda")
    ctr.cov(bases, offsets, n, 1, 16, raw, norm=False, dtype="u32")
    nrm = torch.empty((n, 16), dtype=torch.float64, device="cuda")
    ctr.cov(bases, offsets, n, 1, 16, nrm, norm=True)
    ctx.sync()
    assert bool((raw.sum(dim=1) == L - k + 1).all())
    assert int(raw[:, 0].sum()) == 0
    den = torch.full((1, 1), float(L - k + 1), dtype=torch.float64, device="cuda")  # tensor divisor: a true division
    assert torch.equal(nrm, raw.to(torch.float64) / den)
    # a wide bin collapses everything into bin 0
    ctr.cov(bases, offsets, n, 1 << 40, 16, raw, norm=False, dtype="u32")
    ctx.sync()
    assert bool((raw[:, 0] == L - k + 1).all()) and int(raw[:, 1:].sum()) == 0
    ctr.close()


# ---------------------------------------------------------------------------------------------
# whole-sequence CGR (kt_cgr_points): composition/src/cgr.rs:127-144
def _cgr_seqs(seed, n, max_len, alphabet=b"ACGTUacgtu"):
    rng = np.random.default_rng(seed)
    alpha = np.frombuffer(alphabet, np.uint8)
    lens = rng.integers(0, max_len, size=n)
    if n >= 8:
        lens[:8] = [0, 1, 2, 127, 128, 129, 0, 20000]   # chunk edges, empties, > 2 segments
    return [alpha[rng.integers(0, len(alpha), size=int(L))].tobytes() for L in lens]


@pytest.mark.parametrize("vecsize", [1, 16, 100, 3, 0])
def test_cgr_vs_oracle(hctx, oracle, vecsize):
    seqs = _cgr_seqs(40 + vecsize, 400, 700)
    # adversarial for the bracketing start: long single-letter runs (the two bounds only meet at the run's end),
    # alternating corners, a 30 kb poly-A and a 30 kb poly-G read
    seqs += [b"A" * 5000 + b"T" + b"A" * 3000, b"T" * 4000 + b"a" * 1200 + b"G" * 777, b"AT" * 3000, b"GC" * 2500 + b"U",
             b"A" * 30000, b"G" * 30000, b"C" * 129 + b"G" * 1500 + b"c"]
    bases, offsets = oracle.to_csr(seqs)
    got = hctx.cgr_host(bases, offsets, vecsize)
    want = np.concatenate([oracle.cgr_points(s, vecsize) for s in seqs if len(s)])
    assert got.shape == want.shape
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64))   # bit-identical, signed zeros included


def test_cgr_golden_and_python_surface(hctx, oracle, golden):
    from kmertools_amd import pykmertools as kt
    recs = oracle.read_records(golden / "reads.fq")
    seqs = [s.decode() for _, s in recs]
    rows = kt.CgrComputer(1).vectorise_batch(seqs)
    assert oracle.cgr_text(rows) == (golden / "expected_reads.cgr").read_bytes()
    # tests/test_cgr.py:8-24 compares the parsed fixture with the batch result
    truth = [[tuple(map(float, p.strip("()").split(","))) for p in ln.split()] for ln in
             (golden / "expected_reads.cgr").read_text().splitlines()]
    assert rows == truth
    one = kt.CgrComputer(1).vectorise_one("atgatgaaatagagagactttat")
    assert one[0] == (0.25, 0.25) and one[-1] == (0.7239444851875305, 0.020756304264068604) and len(one) == 23
    assert kt.CgrComputer(4).vectorise_batch([]) == [] and kt.CgrComputer(4).vectorise_one("") == []
    for bad in ("ACGNT", "AC\x01T", "ACG T"):
        with pytest.raises(ValueError, match="Bad nucleotide"):
            kt.CgrComputer(1).vectorise_one(bad)
    with pytest.raises(ValueError):
        kt.CgrComputer(1).vectorise_batch(["ACGT" * 100, "A" * 9000 + "N", "GG"])


def test_cgr_bad_position_and_full_size(torch_mod, ctx, oracle):
    """4 M x 150 bp on the device path: spot rows against the oracle, a checksum of all markers against a
    torch restatement of the walk (150 vectorised steps over reads), and the bad-byte position report"""
    torch = torch_mod
    n, L = 4_000_000, 150
    bases = torch.empty(n * L, dtype=torch.uint8, device="cuda")
    offsets = torch.empty(n + 1, dtype=torch.int64, device="cuda")
    ctx.synth_reads(21, n, L, bases, offsets)
    xy = torch.empty((n * L, 2), dtype=torch.float64, device="cuda")
    bad = torch.zeros(1, dtype=torch.int64, device="cuda")
    ctx.cgr(bases, offsets, n, 1, xy, bad)
    ctx.sync()
    assert int(bad.item()) == -1
    b2 = bases.view(n, L)
    m = torch.full((n, 2), 0.5, dtype=torch.float64, device="cuda")
    half = torch.full((1, 1), 2.0, dtype=torch.float64, device="cuda")
    ref = torch.empty((n, L, 2), dtype=torch.float64, device="cuda")
    for i in range(L):
        c = b2[:, i]
        cx = ((c == ord("T")) | (c == ord("G"))).to(torch.float64)
        cy = ((c == ord("G")) | (c == ord("C"))).to(torch.float64)
        m = (torch.stack([cx, cy], dim=1) + m) / half
        ref[:, i] = m
    assert torch.equal(xy.view(n, L, 2), ref)
    hb = bases[: 3 * L].cpu().numpy().tobytes()
    for r in range(3):
        assert np.array_equal(xy[r * L:(r + 1) * L].cpu().numpy(), oracle.cgr_points(hb[r * L:(r + 1) * L], 1))
    del ref
    pos = 123_456_789
    bases[pos] = ord("N")
    bases[pos + 4000] = ord("x")
    ctx.cgr(bases, offsets, n, 1, xy, bad)
    ctx.sync()
    assert int(bad.item()) == pos


def test_cgr_long_sequence(hctx, oracle):
    """one 3 Mbp sequence (a genome-like record: one read spanning hundreds of wave spans) plus short
    neighbours; every chunk start is recovered by the bracketing walk"""
    rng = np.random.default_rng(77)
    alpha = np.frombuffer(b"ACGTacgu", np.uint8)
    big = alpha[rng.integers(0, 8, size=3_000_001)].tobytes()
    seqs = [b"ACGT", big, b"", b"TTTTGGGG" * 9]
    bases, offsets = oracle.to_csr(seqs)
    got = hctx.cgr_host(bases, offsets, 7)
    want = np.concatenate([oracle.cgr_points(s, 7) for s in seqs if len(s)])
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64))


# ---------------------------------------------------------------------------------------------
# minimisers (kt_minimisers): kmer/src/minimiser.rs:61-175
def _min_triples(hctx, seqs, w, m):
    from kmertools_amd import device
    bases, offsets = device.to_csr(seqs)
    evo, k, s, e = hctx.minimisers_host(bases, offsets, w, m)
    assert len(evo) == len(seqs) + 1 and int(evo[0]) == 0 and int(evo[-1]) == len(k)
    return [[(int(k[j]), int(s[j]), int(e[j])) for j in range(int(evo[i]), int(evo[i + 1]))] for i in range(len(seqs))]


def test_minimisers_reference_cases(hctx, oracle, golden):
    seq = ("ATGCGATATCGTAGGCGTCGATGGAGAGCTAGATCGATCGATCTAAATCCCGATCGATTCCGAGCGCGATCAAAGCGCGATAGGCTAGCTAAAG"
           "CTAGCA")
    assert _min_triples(hctx, [seq], 31, 7)[0] == oracle.minimisers(seq, 31, 7)
    seq2 = "ATGCGATATCGNTAGGCGTCGATGGA"
    assert _min_triples(hctx, [seq2], 8, 5)[0] == oracle.minimisers(seq2, 8, 5)
    recs = [(i, s.decode()) for i, s in oracle.read_records(golden / "reads.fq")]
    for w, m in ((31, 7), (0, 10)):
        got = _min_triples(hctx, [s for _, s in recs], w, m)
        assert got == [oracle.minimisers(s, w, m) for _, s in recs]


@pytest.mark.parametrize("w,m", [(31, 7), (8, 5), (5, 5), (12, 3), (40, 28), (200, 15), (1040, 17), (0, 10), (0, 7),
                                  (64, 31), (33, 1)])
def test_minimisers_vs_oracle(hctx, oracle, w, m):
    """ragged reads with N runs, lower case, raw codes, empty reads, reads shorter than m / w, reads that end in
    N or right after a window filled, and reads longer than several tiles"""
    rng = np.random.default_rng(1000 * w + m)
    seqs = [s.decode("latin-1") for s in ragged_reads(300 + w + m, 400, max_len=500)]
    alpha = np.array(list("ACGT"))
    for L in (m - 1 if m > 1 else 1, m, m + 1, max(w, m), max(w, m) + 1, 3071, 3072, 3073, 4096, 10000, 25000):
        seqs.append("".join(rng.choice(alpha, size=L)))
        if L > 4:
            s = list(seqs[-1])
            s[L // 2] = "N"
            seqs.append("".join(s))
            seqs.append(seqs[-2] + "N")
    seqs += ["A" * 5000, "ACGT" * 2000 + "N" + "TTTTT" * 300, "", "N", "NNNN" + "ACGTTGCA" * 100]
    if w == 0:
        seqs = [s for s in seqs if len(s) >= m]   # shorter reads: the reference's arithmetic underflows
    got = _min_triples(hctx, seqs, w, m)
    for i, s in enumerate(seqs):
        assert got[i] == oracle.minimisers(s, w, m), (i, len(s), w, m)


def test_minimisers_arguments(hctx):
    from kmertools_amd import device
    b, o = device.to_csr(["ACGTACGTACGT"])
    for w, m in ((3, 5), (10, 0), (10, 32)):
        with pytest.raises(Exception):
            hctx.minimisers_host(b, o, w, m)
    evo, k, s, e = hctx.minimisers_host(np.zeros(0, np.uint8), np.zeros(1, np.uint64), 31, 7)
    assert len(k) == 0 and list(evo) == [0]


@pytest.mark.parametrize("w,m,serial", [(5000, 7, "0"), (4200, 17, "0"), (9000, 31, "0"), (20000, 10, "0"), (4096 + 7, 8, "0"),
                                        (8192 + 6, 7, "0"), (12288 + 30, 31, "0"), (70_000, 12, "0"), (33_000, 20, "0"),
                                        (5000, 7, "1"), (4200, 17, "1"), (9000, 31, "1"), (20000, 10, "1")])
def test_minimisers_windows_wider_than_4096(hctx, oracle, monkeypatch, w, m, serial):
    """windows of more than 4096 m-mers: the sliding minimum in two levels in front of the tile kernel (4096-m-mer minima
    from the tiles, doubling over the stride-4096 sequence: wide_window_act - windows of exactly one, two, three and
    seventeen times 4096 m-mers and in between), and the iterator itself, one read per thread (KT_MIN_SERIAL=1:
    min_serial_kernel) - reads shorter than, equal to and several times the window, N runs, lower case, the quirks on the
    last base, ties all along"""
    from kmertools_amd import device
    monkeypatch.setenv("KT_MIN_SERIAL", serial)
    rng = np.random.default_rng(w + m)
    alpha = np.frombuffer(b"ACGT", np.uint8)
    seqs = []
    for L in [0, 1, m - 1, m, w - 1, w, w + 1, w + m, 2 * w + 17, 3 * w, 60, 25_000, 61_000] + ([4 * w + 4095] if w > 30_000 else []):
        s = alpha[rng.integers(0, 4, size=L)].copy()
        if L > 200 and rng.random() < 0.7:
            for at in rng.integers(0, L, size=3):
                s[at:at + int(rng.integers(1, 4))] = ord("N")
        if L > 10:
            s[rng.integers(0, L, size=L // 50 + 1)] |= 0x20
        seqs.append(s.tobytes())
    seqs.append(b"A" * (w + 500))                       # one m-mer all along: ties everywhere
    seqs.append((b"ACGTTGCA" * (w // 4))[: 2 * w + 3])
    bases, offsets = device.to_csr(seqs)
    evo, k, s_, e = hctx.minimisers_host(bases, offsets, w, m)
    for i, seq in enumerate(seqs):
        got = [(int(k[j]), int(s_[j]), int(e[j])) for j in range(int(evo[i]), int(evo[i + 1]))]
        assert got == oracle.minimisers(seq, w, m), (i, len(seq))


def test_minimisers_full_size(torch_mod, ctx, oracle):
    """2 M x 150 bp on the device path, w=31 m=7: spot reads against the oracle, and the structural properties
    of the whole result (offsets monotone, windows inside the read, consecutive windows of a read overlap)"""
    torch = torch_mod
    n, L, w, m = 2_000_000, 150, 31, 7
    bases = torch.empty(n * L, dtype=torch.uint8, device="cuda")
    offsets = torch.empty(n + 1, dtype=torch.int64, device="cuda")
    ctx.synth_reads(33, n, L, bases, offsets, noise=True)
    evo = torch.empty(n + 1, dtype=torch.int64, device="cuda")
    dummy = torch.empty(1, dtype=torch.int64, device="cuda")
    cnt = ctx.minimisers(bases, offsets, n, w, m, evo, dummy, dummy, dummy, 0)
    assert cnt > n
    k = torch.empty(cnt, dtype=torch.int64, device="cuda")
    s = torch.empty(cnt, dtype=torch.int64, device="cuda")
    e = torch.empty(cnt, dtype=torch.int64, device="cuda")
    assert ctx.minimisers(bases, offsets, n, w, m, evo, k, s, e, cnt) == cnt
    assert int(evo[0]) == 0 and int(evo[-1]) == cnt and bool((evo[1:] >= evo[:-1]).all())
    assert bool((s >= 0).all()) and bool((e <= L).all()) and bool((s < e).all())
    hb = bases[: 200 * L].cpu().numpy().tobytes()
    he, hk, hs, hend = evo[:201].cpu().numpy(), k[: int(evo[200])].cpu().numpy(), s[: int(evo[200])].cpu().numpy(), \
        e[: int(evo[200])].cpu().numpy()
    for r in range(200):
        got = [(int(np.uint64(hk[j])), int(hs[j]), int(hend[j])) for j in range(int(he[r]), int(he[r + 1]))]
        assert got == oracle.minimisers(hb[r * L:(r + 1) * L], w, m), r


def test_minimiser_python_surface(hctx, oracle):
    from kmertools_amd import pykmertools as kt
    # tests/test_min.py:7-24
    seq = ("ATGCGATATCGTAGGCGTCGATGGAGAGCTAGATCGATCGATCTAAATCCCGATCGATTCCGAGCGCGATCAAAGCGCGATAGGCTAGCTAAAG"
           "CTAGCA")
    g = kt.MinimiserGenerator(seq, 31, 7)
    got = list(g)
    assert [g.to_acgt(k) for k, _, _ in got] == ["ACGATAT", "ACGCCTA", "AGAGCTA", "AAATCCC", "AATCCCG", "AATCGAT", "AAAGCGC"]
    assert got == oracle.minimisers(seq, 31, 7)
    with pytest.raises(ValueError):
        kt.MinimiserGenerator(seq, 3, 7)


@pytest.mark.parametrize("workload,ranks,plain", [("comp_oligo_k4", 2, False), ("ctr_k31", 2, True),
                                                  ("ctr_k31", 8, True), ("ctr_k15", 3, False)])
def test_bench_two_rank_launch(workload, ranks, plain):
    """bench.py with several ranks (all on GPU 0, gloo collectives) - through torch.distributed.run, the launch contract
    the driver uses for --gpus N, and (`plain`) typed as it stands, `python bench.py --gpus N`: bench.py then starts the
    ranks itself as a child process (the plain command used to exit).  One JSON line from rank 0, whole-job
    value, n_gpus = N.  Eight ranks: eight owners' regions per rank, 4 pieces x 7 senders of records per rank; three
    ranks: an odd number of owners; bench.py's own output check (the counts of all ranks sum to reads x (L - k + 1), and
    a sample of rank 0's reads counted by the oracle is found on the owners' ranks) is what certifies the result.  ctr
    lines say what carried the exchange and how many bytes a rank sent per step."""
    import json, os, subprocess, sys, pathlib
    root = pathlib.Path(__file__).resolve().parents[1]
    env = dict(os.environ, KT_BENCH_SHARE_GPU="1", KT_BULK_MIN_BASES="0")
    for var in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT"):
        env.pop(var, None)
    import socket
    sock = socket.socket()
    sock.bind(("127.0.0.1", 0))
    port = sock.getsockname()[1]
    sock.close()
    tail = [str(root / "bench.py"), "--gpus", str(ranks), "--steps", "2", "--warmup", "1", "--workload", workload, "--reads", "200000",
            "--full"]
    if plain:
        cmd = [sys.executable] + tail
    else:
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(ranks), "--master-addr",
               "127.0.0.1", "--master-port", str(port)] + tail
    r = subprocess.run(cmd, capture_output=True, text=True, env=env, cwd=root, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    j = json.loads(lines[0])
    assert j["n_gpus"] == ranks and j["steps"] == 2 and j["warmup"] == 1 and j["scaling"] == "weak"
    assert j["value"] > 0 and "roofline" in j and "cpu_baseline" not in j and j["config"]["reduced"] is True
    assert j["output_check"]["ok"] is True
    if workload.startswith("ctr"):
        k = 31 if workload == "ctr_k31" else 15
        assert j["output_check"]["sum_of_counts"] == ranks * 200000 * (150 - k + 1)
        # ranks that share a GPU exchange over the host transport (RCCL refuses two ranks on one device): no RCCL
        # communicator, so no RCCL rank count - on N GPUs the line carries rccl_ranks == N or bench.py exits
        assert j["transport"] == "host" and j["rccl_ranks"] == 0 and j["exchanged_bytes_per_rank"] > 0


def test_alloc_placed_c_abi(torch_mod, ctx):
    """kt_device_alloc_placed / kt_device_free: the array the library keeps is the fastest of its candidates under the
    caller's probe - never slower than candidate 0, the plain allocation -, the probe sees every candidate, results
    written into the kept array are the kernel's, a probe that raises is reported, no probe = a plain allocation"""
    torch = torch_mod
    from kmertools_amd import device
    n, L, k = 200000, 150, 4
    bases = torch.empty(n * L, dtype=torch.uint8, device="cuda")
    offsets = torch.empty(n + 1, dtype=torch.int64, device="cuda")
    ctx.synth_reads(77, n, L, bases, offsets)
    bins = device.bins(k, True)
    seen = []

    def probe(addr):
        seen.append(addr)
        ctx.oligo(bases, offsets, n, k, addr, count_min=True, norm=True, total_step=1, dtype="f64")
    arr, info = ctx.alloc_placed(n * bins * 8, probe, candidates=4, launches=3)
    assert 1 <= info["candidates"] <= 4 and len(info["ms"]) == info["candidates"]
    assert info["ms"][info["picked"]] <= info["ms"][0] and arr.ptr in seen
    assert len(set(seen)) == info["candidates"]
    out = arr.tensor((n, bins), torch.float64)
    want = torch.empty((n, bins), dtype=torch.float64, device="cuda")
    ctx.oligo(bases, offsets, n, k, out, count_min=True, norm=True, total_step=1, dtype="f64")
    ctx.oligo(bases, offsets, n, k, want, count_min=True, norm=True, total_step=1, dtype="f64")
    torch.cuda.synchronize()
    assert torch.equal(out, want)
    del out
    arr.close()
    plain, info = ctx.alloc_placed(1 << 20)
    assert info["candidates"] == 1 and info["picked"] == 0 and plain.ptr
    plain.close()

    def bad(addr):
        raise RuntimeError("probe failed")
    with pytest.raises(RuntimeError):
        ctx.alloc_placed(1 << 20, bad, candidates=3)


def test_bench_places_its_arrays():
    """bench.py on one GPU, reduced size: the oligo workload's output and input arrays are chosen among candidate
    allocations by the library (kt_device_alloc_placed), the line says which and what the plain allocation would have
    given, the output check and the oracle's slice check pass; with --no-place the objects are absent"""
    import json, os, subprocess, sys, pathlib
    root = pathlib.Path(__file__).resolve().parents[1]
    for flag in ([], ["--no-place"]):
        cmd = [sys.executable, str(root / "bench.py"), "--steps", "2", "--warmup", "1", "--workload", "comp_oligo_k4",
               "--reads", "300000", "--cpu-seconds", "1", "--full"] + flag
        r = subprocess.run(cmd, capture_output=True, text=True, cwd=root, timeout=900)
        assert r.returncode == 0, r.stderr[-2000:]
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
        assert len(lines) == 1
        j = json.loads(lines[0])
        assert j["output_check"]["ok"] is True and j["config"]["reduced"] is True
        assert j["output_check"]["oracle_slice"]["ok"] is True
        if flag:
            assert "output_placement" not in j and "input_placement" not in j
        else:
            for key in ("output_placement", "input_placement"):
                p = j[key]
                assert p["candidates"] == len(p["ms"]) >= 1 and 0 <= p["picked"] < p["candidates"]
                assert p["ms"][p["picked"]] == min(p["ms"])
            assert 0 < j["roofline"]["frac_plain_allocation"] <= j["roofline"]["frac"] + 1e-9


def test_bench_plain_run_dumps_its_outputs(tmp_path, oracle):
    """a plain bench.py run (no --full) times the headline workload alone - no other workload, output check or CPU
    baseline - for exactly --steps steps, and --dump-outputs writes the seeded row sample of its last step's output: the
    oracle's rows for the same reads, bit for bit"""
    import importlib.util, json, subprocess, sys, pathlib
    root = pathlib.Path(__file__).resolve().parents[1]
    n, L = 300000, 150
    cmd = [sys.executable, str(root / "bench.py"), "--steps", "3", "--warmup", "1", "--reads", str(n),
           "--dump-outputs", str(tmp_path)]
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=root, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    j = json.loads(lines[0])
    assert j["steps"] == 3 and j["ms_per_step"] > 0 and j["dtype"] == "f64" and j["higher_is_better"] is True
    assert not {"ctr_k31", "ctr_k15", "comp_cgr_k7", "cpu_baseline", "output_check"} & set(j)
    assert sorted(p.name for p in tmp_path.iterdir()) == ["comp_oligo_k4.npy"]
    got = np.load(tmp_path / "comp_oligo_k4.npy")
    spec = importlib.util.spec_from_file_location("bench", root / "bench.py")
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    idx = bench.sample_index(n, bench.DUMP_BYTES // (136 * 8))
    assert got.dtype == np.float64 and got.shape == (len(idx), 136) and got.nbytes <= bench.DUMP_BYTES
    hb, _ = oracle.synth_reads(bench.SEED + bench.WORKLOADS["comp_oligo_k4"]["cfg"], n, L)
    sb = np.ascontiguousarray(hb.reshape(n, L)[idx]).reshape(-1)
    want = oracle.oligo_batch(sb, np.arange(len(idx) + 1, dtype=np.uint64) * np.uint64(L), 4, True, True, 1.0, threads=8)
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64))


def test_ctr_cfg3_full_size_properties(torch_mod, ctx):
    """BASELINE cfg3 at full size (50 M x 150 bp, k=15) through the bulk build: every k-mer instance is
    counted exactly once (sum of counts = n * 136), no key is outside the canonical 15-mer space or stored
    twice, and re-counting the exported pairs into a second table reproduces the first"""
    from kmertools_amd import device
    torch = torch_mod
    n, L, k = 50_000_000, 150, 15
    bases = torch.empty(n * L, dtype=torch.uint8, device="cuda")
    offsets = torch.empty(n + 1, dtype=torch.int64, device="cuda")
    ctx.synth_reads(0x6b6d6572 + 2, n, L, bases, offsets)
    canon_space = (4 ** k) // 2            # odd k: no palindromes
    ctr = device.Counter(ctx, k, 1 << 31)
    ctr.add_reads(bases, offsets, n)
    distinct = ctr.size()
    assert 0.9 * canon_space < distinct <= canon_space   # 6.8 G draws over 0.54 G canonical 15-mers
    keys = torch.empty(distinct, dtype=torch.int64, device="cuda")
    counts = torch.empty(distinct, dtype=torch.int32, device="cuda")
    assert ctr.export(keys, counts, distinct) == distinct
    assert int(counts.to(torch.int64).sum()) == n * (L - k + 1)
    assert int(keys.min()) >= 0 and int(keys.max()) < 4 ** k
    sk = torch.sort(keys).values
    assert bool((sk[1:] != sk[:-1]).all())
    del sk, bases, offsets
    ctr.clear()
    ctr.add_pairs(keys, counts, distinct)
    assert ctr.size() == distinct
    k2 = torch.empty(distinct, dtype=torch.int64, device="cuda")
    c2 = torch.empty(distinct, dtype=torch.int32, device="cuda")
    ctr.export(k2, c2, distinct)
    # exact integer checksum: keys < 2^30 and the total stays below 2^63 (a float64 sum depends on the export order)
    assert int((k2 * c2.to(torch.int64)).sum()) == int((keys * counts.to(torch.int64)).sum())
    assert int(c2.to(torch.int64).sum()) == n * (L - k + 1)
    ctr.close()


def test_minimisers_wide_window_run_start_before_halo(hctx, oracle):
    """w > 1024 (W <= 1024 still): a run that starts a few bases in front of a tile's halo must keep its exact
    length for the tile's first positions (found by tools/fuzz_parity.py: w=1050, m=27)"""
    rng = np.random.default_rng(5)
    alpha = np.array(list("ACGT"))
    seqs = []
    for d in (1, 5, 26, 27, 40, 200):
        s = rng.choice(alpha, size=40000)
        for tile in range(1, 5):
            for unit in (3072, 7168):                 # tile sizes this kernel has used
                p = tile * unit - 1024 - d
                if 0 <= p < len(s):
                    s[p] = "N"
        seqs.append("".join(s))
    for w, m in ((1050, 27), (1054, 31), (1030, 7)):
        got = _min_triples(hctx, seqs, w, m)
        for i, s in enumerate(seqs):
            assert got[i] == oracle.minimisers(s, w, m), (i, w, m)


def test_minimisers_windows_wider_than_a_granule(hctx, oracle):
    """1024 < W <= 4096 runs on tiles with a four-granule halo: reads that span several tiles, breaks near the tile
    and halo boundaries, windows right up to the tile path's limit; one m-mer more takes the one-read-per-thread path"""
    rng = np.random.default_rng(11)
    alpha = np.array(list("ACGT"))
    seqs = []
    for d in (0, 1, 30, 500):
        s = rng.choice(alpha, size=30000)
        for p in (4096 - d, 8192 - d, 8192 + d, 12288 - 17 - d):
            s[p] = "N"
        seqs.append("".join(s))
    seqs += ["".join(rng.choice(alpha, size=n)) for n in (5000, 4126, 4127, 100, 0, 9000)]
    for w, m in ((1040, 15), (2000, 31), (3000, 9), (4100, 5), (4126, 31), (4111, 16)):
        got = _min_triples(hctx, seqs, w, m)
        for i, s in enumerate(seqs):
            assert got[i] == oracle.minimisers(s, w, m), (i, w, m)
    got = _min_triples(hctx, seqs, 4127, 31)
    for i, s in enumerate(seqs):
        assert got[i] == oracle.minimisers(s, 4127, 31), (i, 4127, 31)


def test_all_empty_reads_everywhere(hctx, oracle):
    """a batch that holds reads but no bases (every read empty): every entry point returns the empty answer"""
    from kmertools_amd import device
    seqs = ["", "", ""]
    bases, offsets = device.to_csr(seqs)
    assert not hctx.oligo_host(bases, offsets, 4).any() and hctx.oligo_host(bases, offsets, 4).shape == (3, 136)
    ctr = device.Counter(hctx, 21, 4096)
    ctr.add_reads_host(bases, offsets)
    assert ctr.size() == 0
    cov = ctr.cov_host(bases, offsets, 2, 5, True)
    assert cov.shape == (3, 5) and not cov.any()
    ctr.close()
    assert hctx.cgr_host(bases, offsets, 1).shape == (0, 2)
    for w in (0, 31):
        evo, k, s, e = hctx.minimisers_host(bases, offsets, w, 7)
        assert list(evo) == [0, 0, 0, 0] and len(k) == 0
    f, r, idx = hctx.kmers_host(bases, offsets, 5)
    assert len(f) == 0
    keys, counts = hctx.route_host(bases, offsets, 21, 4)
    assert len(keys) == 0 and not counts.any()


# ---------------------------------------------------------------------------------------------
# BASELINE configs at full size that round 1 only exercised through bench.py

def test_cfg5_device_ring_sampled_rows(torch_mod, ctx, oracle):
    """comp cgr k=7 (cfg5) the way bench.py runs it: 10 M x 150 bp through the device-pointer path in 1 M-read
    batches that reuse one f32 output ring; every row sums to 1, three 4096-row slices match the oracle <= 1e-6"""
    torch = torch_mod
    n, L, k, B, seed = 10_000_000, 150, 7, 1_000_000, 0x6b6d6572 + 4
    bases = torch.empty(n * L, dtype=torch.uint8, device="cuda")
    offsets = torch.empty(n + 1, dtype=torch.int64, device="cuda")
    ctx.synth_reads(seed, n, L, bases, offsets)
    ring = torch.empty((B, 8192), dtype=torch.float32, device="cuda")
    samples = {0: 0, 4: 4_567_890, 9: n - 4096}     # batch -> first read of the sampled slice
    for b in range(n // B):
        r0 = b * B
        o = (offsets[r0:r0 + B + 1] - offsets[r0]).contiguous()
        ring.fill_(-1.0)                              # a row the kernel skipped would show
        ctx.oligo(bases[r0 * L:], o, B, k, ring, dtype="f32")
        torch.cuda.synchronize()
        s = ring.sum(dim=1, dtype=torch.float64)
        assert float((s - 1.0).abs().max()) < 1e-5
        assert float(ring.min()) >= 0.0
        if b in samples:
            first = samples[b]
            hb, ho = oracle.synth_reads(seed, 4096, L, first_read=first)
            want = oracle.oligo_batch(hb, ho, k, True, True, 1.0, threads=4)
            got = ring[first - r0:first - r0 + 4096].cpu().numpy()
            assert np.abs(got.astype(np.float64) - want).max() <= 1e-6     # north_star tolerance for f32 rows
            assert np.array_equal(got != 0, want != 0)


def test_ctr_cfg4_per_gpu_shard_properties(torch_mod, ctx, oracle):
    """BASELINE cfg4's per-GPU shard (25 M x 150 bp, k=31, about 3 G distinct keys): every k-mer instance counted
    once, no key stored twice, export -> re-import idempotent, and three 1 M-read sub-batches against the oracle
    (their own tables bit-exact; every one of their keys present in the big table with at least that count)"""
    from kmertools_amd import device
    torch = torch_mod
    n, L, k, seed = 25_000_000, 150, 31, 0x6b6d6572 + 3
    kpr = L - k + 1
    torch.cuda.empty_cache()      # the table, its build scratch and the export arrays need ~200 GB
    bases = torch.empty(n * L, dtype=torch.uint8, device="cuda")
    offsets = torch.empty(n + 1, dtype=torch.int64, device="cuda")
    ctx.synth_reads(seed, n, L, bases, offsets)
    ctr = device.Counter(ctx, k, int(1.9 * n * kpr))
    ctr.add_reads(bases, offsets, n)
    distinct = ctr.size()
    assert 0.99 * n * kpr < distinct <= n * kpr          # uniform reads: nearly every 31-mer is unique
    keys = torch.empty(distinct, dtype=torch.int64, device="cuda")
    counts = torch.empty(distinct, dtype=torch.int32, device="cuda")
    assert ctr.export(keys, counts, distinct) == distinct
    ctr.close()                                            # the table and the build scratch: ~160 GB back
    assert int(counts.to(torch.int64).sum()) == n * kpr
    assert int(keys.min()) >= 0 and int(keys.max()) < 4 ** k
    # torch.sort takes at most 2^31 - 1 elements: sort the export in pieces of 2^30 (a key stored twice would show
    # inside a piece here, or across pieces as a smaller table after the re-import below)
    pieces = []
    for s0 in range(0, distinct, 1 << 30):
        sk, order = torch.sort(keys[s0:s0 + (1 << 30)])
        assert bool((sk[1:] != sk[:-1]).all())
        pieces.append((sk, counts[s0:s0 + (1 << 30)][order]))
        del order
    # sampled sub-batches
    sub = 1_000_000
    small = device.Counter(ctx, k, 1 << 28)
    for first in (0, 11_000_000, n - sub):
        hb, ho = oracle.synth_reads(seed, sub, L, first_read=first)
        wk, wc = oracle.count_reads(hb, ho, k, n_parts=64, threads=8)
        small.clear()
        small.add_reads(bases[first * L:(first + sub) * L], offsets[:sub + 1], sub)
        d = small.size()
        gk = torch.empty(d, dtype=torch.int64, device="cuda")
        gc = torch.empty(d, dtype=torch.int32, device="cuda")
        small.export(gk, gc, d)
        gk, o2 = torch.sort(gk)
        gc = gc[o2]
        assert np.array_equal(gk.cpu().numpy().view(np.uint64), wk)
        assert np.array_equal(gc.cpu().numpy().view(np.uint32), wc)
        hits = torch.zeros(d, dtype=torch.int32, device="cuda")
        big = torch.zeros(d, dtype=torch.int32, device="cuda")
        for sk, sc in pieces:
            pos = torch.searchsorted(sk, gk).clamp(max=sk.numel() - 1)
            hit = sk[pos] == gk
            hits += hit.to(torch.int32)
            big += torch.where(hit, sc[pos], torch.zeros_like(gc))
        assert bool((hits == 1).all()) and bool((big >= gc).all())
        del gk, gc, o2, hits, big
    small.close()
    del pieces, sk, sc, bases, offsets
    torch.cuda.empty_cache()
    # merge idempotence at full size: the exported pairs into an empty table
    ctr2 = device.Counter(ctx, k, int(1.9 * n * kpr))
    ctr2.add_pairs(keys, counts, distinct)
    assert ctr2.size() == distinct
    k2 = torch.empty(distinct, dtype=torch.int64, device="cuda")
    c2 = torch.empty(distinct, dtype=torch.int32, device="cuda")
    assert ctr2.export(k2, c2, distinct) == distinct
    ctr2.close()
    assert int(c2.to(torch.int64).sum()) == n * kpr
    # order-independent exact checksums (int64 arithmetic wraps mod 2^64 on both sides)
    assert int((k2 * c2.to(torch.int64)).sum()) == int((keys * counts.to(torch.int64)).sum())
    assert int((k2 ^ (k2 >> 29)).sum()) == int((keys ^ (keys >> 29)).sum())


def test_ctr_cfg4_routed_into_8_owners_full_size(torch_mod, ctx, oracle, monkeypatch):
    """BASELINE cfg4's geometry on one GPU: a rank's 25 M x 150 bp reads routed into the regions of 8 owners (KT_SHARD_FORCE=8:
    what one rank of eight does - route pass, the regions counted piece by piece by the single-GPU pipeline over records), all
    of them counted here.  What a rank of eight would have put on the wires - 7 of the 8 regions, whole blocks - is under
    5 GB (the raw k-mers were 21 GB); every k-mer instance is counted once; the table equals the one the
    ordinary path builds from the same reads (order-independent exact checksums over all 3 G entries); a 1 M-read sub-batch
    counted by the oracle is in it; the owners' regions are balanced"""
    from kmertools_amd import device
    torch = torch_mod
    n, L, k, seed = 25_000_000, 150, 31, 0x6b6d6572 + 3
    kpr = L - k + 1
    torch.cuda.empty_cache()
    bases = torch.empty(n * L, dtype=torch.uint8, device="cuda")
    offsets = torch.empty(n + 1, dtype=torch.int64, device="cuda")
    ctx.synth_reads(seed, n, L, bases, offsets)
    monkeypatch.setenv("KT_SHARD_FORCE", "8")
    sh = device.Sharded(ctx, k, int(1.9 * n * kpr), n * L, 1, 0, None)
    keys = torch.empty(n * kpr, dtype=torch.int64, device="cuda")
    counts = torch.empty(n * kpr, dtype=torch.int32, device="cuda")
    sh.table.export_target(keys, counts, n * kpr)
    sh.add_reads(bases, offsets, n)
    sh.finalize()
    sent = sh.exchanged_bytes()
    assert 0 < sent <= 5_000_000_000, sent
    assert 1.4 < sent / (n * kpr * 7 / 8) < 2.0   # ~1.7 bytes per k-mer on the wires (8 as raw keys), 7 of the 8 regions
    distinct = sh.table.size()
    assert sh.table.export(keys, counts, n * kpr) == distinct
    assert 0.99 * n * kpr < distinct <= n * kpr
    assert int(counts[:distinct].to(torch.int64).sum()) == n * kpr
    ka, ca = keys[:distinct], counts[:distinct].to(torch.int64)
    sums = (int((ka * ca).sum()), int((ka ^ (ka >> 29)).sum()), int(ca.sum()))
    # a sub-batch against the oracle, looked up where the routed table has it
    sub = 1_000_000
    hb, ho = oracle.synth_reads(seed, sub, L, first_read=7_000_000)
    wk, wc = oracle.count_reads(hb, ho, k, n_parts=64, threads=8)
    dk = torch.from_numpy(wk.view(np.int64).copy()).cuda()
    got = torch.zeros(len(wk), dtype=torch.int32, device="cuda")
    sh.table.lookup(dk, len(wk), got)
    assert bool((got >= torch.from_numpy(wc.astype(np.int32)).cuda()).all())
    del dk, got
    sh.close()
    # the same reads through the ordinary path: the same table
    monkeypatch.delenv("KT_SHARD_FORCE")
    ctr = device.Counter(ctx, k, int(1.9 * n * kpr))
    ctr.export_target(keys, counts, n * kpr)
    ctr.add_reads(bases, offsets, n)
    d2 = ctr.size()
    assert ctr.export(keys, counts, n * kpr) == d2 == distinct
    ka, ca = keys[:d2], counts[:d2].to(torch.int64)
    assert sums == (int((ka * ca).sum()), int((ka ^ (ka >> 29)).sum()), int(ca.sum()))
    ctr.close()


def quotient_checksum(d_lo, d_hi):
    """the sum, modulo 2^64, of the bit patterns of numpy's c / d for all 0 <= c <= d, d_lo <= d <= d_hi"""
    want = 0
    for d in range(d_lo, d_hi + 1):
        q = np.arange(d + 1, dtype=np.float64) / np.float64(d)
        want = (want + int(q.view(np.uint64).sum(dtype=np.uint64))) % (1 << 64)
    return want


def test_quotient_exhaustive(hctx):
    """the reciprocal + fma normalisation against the IEEE division for every count / divisor pair a read of up to
    32 768 k-mers can produce (total_step 1 and 2: d = total_step * kmers, c <= kmers), and the device division
    itself against numpy on the pairs with d <= 2048"""
    n, bad, _ = hctx.selftest_quotient(1, 32768)
    assert n == sum(d + 1 for d in range(1, 32769)) and bad == 0
    n, bad, chk = hctx.selftest_quotient(1, 2048)
    assert bad == 0 and chk == quotient_checksum(1, 2048)
