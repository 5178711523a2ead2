"""kt_ctr_index_sequences, kt_ctr_thread_hits, kt_thread_runs and `kmertools thread` on the GPU against tests/thread_ref.py
(which tests/test_thread_cli_args.py pins, on the CPU, to worked answers, to a string-level brute force and to its own
invariants).  Every comparison is exact."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "kmertools_amd", "bin", "kmertools")
sys.path.insert(0, os.path.join(ROOT, "tests"))
import graph_ref as gr  # noqa: E402
import read_batches as rb  # noqa: E402
import thread_ref as tr  # noqa: E402

NO, HOST, DEVICE = 0xFFFFFFFF, 0, 1
ACGT = np.frombuffer(b"ACGT", np.uint8)
RUN_KEYS = ("run_start", "run_len", "run_unitig", "run_upos")
KNOWN = json.load(open(os.path.join(ROOT, "tests", "golden", "thread_known.json")))["cases"]


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    return torch


@pytest.fixture(scope="module")
def device():
    from kmertools_amd import device
    return device


@pytest.fixture(scope="module")
def ctx(torch_mod, device):
    c = device.Context(0, stream=torch_mod.cuda.current_stream().cuda_stream)
    yield c
    c.close()


def rc_bytes(s):
    return bytes(s).translate(bytes.maketrans(b"ACGTacgt", b"TGCAtgca"))[::-1]


def random_seq(rng, n):
    return ACGT[rng.integers(0, 4, size=n)].tobytes()


def graph_unitigs(device, ctx, k, reads):
    """the library's unitigs of the reads' k-mers (host arrays): every canonical k-mer in exactly one of them, once"""
    b, o = device.to_csr(reads)
    c = device.Counter(ctx, k, max(1 << 12, 2 * len(b)))
    try:
        c.add_reads_host(b, o)
        ub, uo, _, _ = c.unitigs()
    finally:
        c.close()
    return ub, uo


def reference(k, ub, uo, qb, qo):
    index = tr.index_np(ub, uo, k)
    hits = tr.hits_np(index, qb, qo, k)
    return index, hits, tr.runs_np(hits, qo, uo, k)


def same_runs(got, want, what=""):
    for name in RUN_KEYS + ("run_offsets", "tally"):
        assert got[name].dtype == want[name].dtype and np.array_equal(got[name], want[name]), (what, name, got[name][:8], want[name][:8])


def device_thread(torch, ui, ctx, qb, qo, hits_align=0, shift=0, max_runs=None):
    """hits and runs through device memory: fenced outputs, the hits at `hits_align` past a 256-byte boundary, the bases
    `shift` bytes past one, the offsets 8 past a 16-byte boundary"""
    n, total, nu = len(qo) - 1, int(qo[-1]), len(ui.offsets) - 1
    db = rb.bases_view(torch, qb, shift)
    do = rb.offsets_view(torch, qo)
    du = torch.from_numpy(ui.offsets.astype(np.int64)).cuda()
    fh = rb.Fenced(torch, total, torch.int32, align=hits_align, prefill=torch.full((total,), -1, dtype=torch.int32))
    ui.table.thread_hits(db, do, n, fh.t)
    f_off = rb.Fenced(torch, n + 1, torch.int64)
    f_tally = rb.Fenced(torch, 6, torch.int64, align=8)
    nr = ctx.thread_runs(fh.t, do, n, du, nu, ui.k, run_offsets=f_off.t, tally=f_tally.t)
    room = nr if max_runs is None else max_runs
    fs = rb.Fenced(torch, room, torch.int64, align=8)
    fl, fu, fp = (rb.Fenced(torch, room, torch.int32, align=a) for a in (4, 8, 12))
    uh = torch.zeros(max(nu, 1), dtype=torch.int64, device="cuda")
    ur = torch.zeros(max(nu, 1), dtype=torch.int64, device="cuda")
    counted = (f_off.np(np.uint64).copy(), f_tally.np(np.uint64).copy())
    if room:
        assert ctx.thread_runs(fh.t, do, n, du, nu, ui.k, fs.t, fl.t, fu.t, fp.t, f_off.t, room, uh, ur, f_tally.t) == nr
    torch.cuda.synchronize()
    for f in (fh, f_off, f_tally, fs, fl, fu, fp):
        f.check()
    out = {"hits": fh.np(np.uint32), "run_start": fs.np(np.uint64)[:nr], "run_len": fl.np(np.uint32)[:nr],
           "run_unitig": fu.np(np.uint32)[:nr], "run_upos": fp.np(np.uint32)[:nr], "run_offsets": f_off.np(np.uint64),
           "tally": f_tally.np(np.uint64), "unitig_hits": uh.cpu().numpy().view(np.uint64)[:nu],
           "unitig_runs": ur.cpu().numpy().view(np.uint64)[:nu]}
    # the counting call filled run_offsets and tally already
    assert np.array_equal(counted[0], out["run_offsets"]) and np.array_equal(counted[1], out["tally"])
    return out


def check_both(torch, device, ctx, k, ub, uo, qb, qo, what="", **dev):
    """index, hits and runs through both memory kinds against the reference; -> the reference's runs"""
    index, want_hits, want = reference(k, ub, uo, qb, qo)
    ui = device.UnitigIndex(ctx, k, ub, uo)
    try:
        assert ui.n_kmers == index[2] == ui.table.size()
        keys, vals = ui.table.export_host()
        assert np.array_equal(keys, index[0]) and np.array_equal(vals, index[1]), (what, "the index")
        uh, ur = np.zeros(len(uo) - 1, np.uint64), np.zeros(len(uo) - 1, np.uint64)
        got = ui.thread_host(qb, qo, uh, ur)
        assert np.array_equal(got["hits"], want_hits), (what, "hits, host", np.flatnonzero(got["hits"] != want_hits)[:8])
        same_runs(got, want, what + " host")
        assert np.array_equal(uh, want["unitig_hits"]) and np.array_equal(ur, want["unitig_runs"]), (what, "per unitig, host")
        got = device_thread(torch, ui, ctx, qb, qo, **dev)
        assert np.array_equal(got["hits"], want_hits), (what, "hits, device", np.flatnonzero(got["hits"] != want_hits)[:8])
        same_runs(got, want, what + " device")
        assert np.array_equal(got["unitig_hits"], want["unitig_hits"]) and np.array_equal(got["unitig_runs"], want["unitig_runs"]), what
    finally:
        ui.close()
    return want


# ---- 1. the worked answers ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", KNOWN, ids=lambda c: c["name"])
def test_thread_known_answers(torch_mod, device, ctx, case):
    k = case["k"]
    ub, uo = graph_unitigs(device, ctx, k, case["graph_reads"])
    assert [ub[int(uo[i]):int(uo[i + 1])].tobytes().decode() for i in range(len(uo) - 1)] == case["unitigs"]
    qb, qo = device.to_csr(case["reads"])
    want = check_both(torch_mod, device, ctx, k, ub, uo, qb, qo, case["name"])
    runs = list(zip(*(want[n].tolist() for n in RUN_KEYS)))
    ro = want["run_offsets"].tolist()
    assert [[list(r) for r in runs[ro[i]:ro[i + 1]]] for i in range(len(case["reads"]))] == case["runs"]


# ---- 2. every k that takes another path; orientations ------------------------------------------------------------------------------

def graph_reads(rng, k, genome_len=3000, n=120):
    """reads of a small genome with errors, a cycle, a k-mer that follows itself and a hairpin"""
    genome = random_seq(rng, genome_len)
    reads = []
    for _ in range(n):
        a = int(rng.integers(0, genome_len - 150))
        s = bytearray(genome[a:a + int(rng.integers(k, 150))])
        if rng.random() < 0.3:
            s[int(rng.integers(0, len(s)))] = ACGT[int(rng.integers(0, 4))]
        reads.append(bytes(s))
    cyc = random_seq(rng, 40 + k)
    half = random_seq(rng, k)
    return reads, [cyc * 2 + cyc[:k - 1], b"A" * (k + 5), half + rc_bytes(half)]


@pytest.mark.parametrize("k", [1, 2, 4, 15, 16, 17, 31])
def test_thread_every_k(torch_mod, device, ctx, k):
    rng = np.random.default_rng(700 + k)
    reads, special = graph_reads(rng, k)
    ub, uo = graph_unitigs(device, ctx, k, reads + special)
    # what is threaded: the reads, antiparallel ones, the cycle twice around, the self-link, the hairpin, the unitigs
    # themselves, reads with an N / lower case / a substitution, short and empty ones, a foreign one
    q = reads[:60] + [rc_bytes(r) for r in reads[:40]] + special + [rc_bytes(s) for s in special]
    q += [ub[int(uo[i]):int(uo[i + 1])].tobytes() for i in range(min(len(uo) - 1, 50))]
    for r in reads[60:80]:
        s = bytearray(r)
        s[len(s) // 2] = ord("N") if len(q) % 2 else ACGT[(list(ACGT).index(s[len(s) // 2]) + 1) % 4]
        q += [bytes(s), r.lower()]
    q += [b"", reads[0][:k - 1], b"", random_seq(rng, 200), b""]
    qb, qo = device.to_csr(q)
    want = check_both(torch_mod, device, ctx, k, ub, uo, qb, qo, "k = %d" % k, hits_align=4, shift=3)
    t = want["tally"]
    assert t[1] > 0 and t[3] == 0 and (want["run_unitig"] & 1).any() and not (want["run_unitig"] & 1).all()
    if k >= 15:
        assert t[2] > 0 and t[5] < len(q)
        # the cycle walked twice: more than one run on one unitig within the read, each a whole turn or its rest
        i = 60 + 40
        ro = want["run_offsets"]
        cyc_runs = want["run_unitig"][int(ro[i]):int(ro[i + 1])]
        assert len(cyc_runs) >= 2 and len(set(cyc_runs.tolist())) == 1


# ---- 3. reads against the walk's structural constants ------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def long_graph():
    """k = 31: one unitig longer than two segments and a few short ones, random (no k-mer twice: the reference asserts it)"""
    rng = np.random.default_rng(31)
    seqs = [random_seq(rng, 20000)] + [random_seq(rng, int(n)) for n in (31, 32, 33, 64, 100, 257, 1000)]
    return 31, seqs, rb.Batch("long graph", seqs)


def test_thread_structural_positions(torch_mod, device, ctx, long_graph):
    k, seqs, g = long_graph
    big = seqs[0]
    index = tr.index_np(g.bases, g.offsets, k)
    ui = device.UnitigIndex(ctx, k, g.bases, g.offsets)
    try:
        assert ui.n_kmers == index[2]
        for p in (7, 8, 9, 31, 32, 33, 8191, 8192, 8193):
            # a read that ends at p (a run from base 0 when it holds a k-mer), a run that starts at p, antiparallel, and one run
            # that spans two segments after it
            q = [big[100:100 + p], rc_bytes(seqs[6][:90]), big[3000:3000 + 8300], b"", seqs[3][:k - 1], big[50:50 + k]]
            qb, qo = device.to_csr(q)
            want_hits = tr.hits_np(index, qb, qo, k)
            want = tr.runs_np(want_hits, qo, g.offsets, k)
            got = ui.thread_host(qb, qo)
            assert np.array_equal(got["hits"], want_hits), p
            same_runs(got, want, "p = %d host" % p)
            assert p in want["run_start"].tolist() and 8270 in want["run_len"].tolist()
            if p in (9, 33, 8193):
                got = device_thread(torch_mod, ui, ctx, qb, qo, hits_align=12, shift=1)
                assert np.array_equal(got["hits"], want_hits), p
                same_runs(got, want, "p = %d device" % p)
    finally:
        ui.close()


@pytest.mark.parametrize("family", ["tiny", "empty_runs"])
def test_thread_tiny_and_empty_reads(torch_mod, device, ctx, family):
    """tens of thousands of tiny reads (segments with hundreds of read starts), long runs of empty reads: k = 4, onto the
    unitigs of a part of themselves, so that hits, misses and one-k-mer runs mix"""
    k = 4
    b = rb.tiny_batch(11, k, 24000) if family == "tiny" else rb.empty_runs_batch(12)
    assert b.n > (30000 if family == "tiny" else 6000)
    rng = np.random.default_rng(5)
    ub, uo = graph_unitigs(device, ctx, k, [random_seq(rng, 60), random_seq(rng, 45)])
    want = check_both(torch_mod, device, ctx, k, ub, uo, b.bases, b.offsets, b.name)
    assert want["tally"][1] > 1000 and want["tally"][2] > 1000 and (want["run_len"] == 1).any() and (want["run_len"] > 1).any()


# ---- 4. the scan: items on either side of a tile, and of the one-workgroup tile scan's first round ---------------------------------

@pytest.mark.parametrize("total", [1022, 1023, 1024, 1025, 2047, 2048, 256 * 1024 - 2, 256 * 1024 - 1, 256 * 1024, 256 * 1024 + 1])
def test_thread_runs_scan_sizes(torch_mod, device, ctx, total):
    """kt_scan.hpp scans total + 1 items in tiles of 1024, the tiles' sums 256 at a time.  The hits are made up: a function of
    arrays needs no table.  Runs of 1..5 positions, both orientations, misses, bad values and sentinels between them, and a
    run that ends on the last position."""
    rng = np.random.default_rng(total)
    k, uo = 3, np.array([0, 40, 40, 47, 300], np.uint64)  # (an empty unitig among them)
    hits = np.full(total, NO, np.uint32)
    j = 0
    while j < total:
        n = int(rng.integers(1, 6))
        kind = rng.random()
        if kind < 0.7:
            a = int(rng.integers(0, 2))
            G = int(rng.integers(0, 300 - 8))
            for x in range(min(n, total - j)):
                hits[j + x] = 1 + 2 * (G + x if a == 0 else G + 5 - x) + a
        elif kind < 0.85:
            hits[j:j + n] = 0
        elif kind < 0.9:
            hits[j] = 1 + 2 * int(rng.integers(300, 1 << 30))
        j += n
    if total % 2:
        hits[total - 2:] = (1 + 2 * 10, 1 + 2 * 11)
    lens = rng.integers(0, 60, size=total // 25)
    lens = lens[np.cumsum(lens) < total]
    qo = np.concatenate(([0], np.cumsum(lens), [total])).astype(np.uint64)
    want = tr.runs_np(hits, qo, uo, k)
    assert want["tally"][3] > 0 and want["tally"][4] > total // 10
    got = ctx.thread_runs_host(hits, qo, uo, k)
    same_runs(got, want, "host")
    dh, do, du = torch_mod.from_numpy(hits.view(np.int32)).cuda(), rb.offsets_view(torch_mod, qo), torch_mod.from_numpy(uo.astype(np.int64)).cuda()
    nr = int(want["tally"][4])
    out = [torch_mod.empty(nr, dtype=torch_mod.int64, device="cuda")] + [torch_mod.empty(nr, dtype=torch_mod.int32, device="cuda") for _ in range(3)]
    d_off = torch_mod.empty(len(qo), dtype=torch_mod.int64, device="cuda")
    d_tally = torch_mod.empty(6, dtype=torch_mod.int64, device="cuda")
    assert ctx.thread_runs(dh, do, len(qo) - 1, du, len(uo) - 1, k, *out, d_off, nr, tally=d_tally) == nr
    torch_mod.cuda.synchronize()
    got = {n: t.cpu().numpy().view(want[n].dtype) for n, t in zip(RUN_KEYS + ("run_offsets", "tally"), out + [d_off, d_tally])}
    same_runs(got, want, "device")


# ---- 5. the protocol and the argument errors -----------------------------------------------------------------------------------------

def small_case(device, ctx, k=15, seed=3):
    rng = np.random.default_rng(seed)
    reads, special = graph_reads(rng, k, 1500, 40)
    ub, uo = graph_unitigs(device, ctx, k, reads + special)
    qb, qo = device.to_csr(reads[:30] + [rc_bytes(r) for r in reads[:10]] + [b"", random_seq(rng, 90)])
    return k, ub, uo, qb, qo


def err_code(device, fn):
    from kmertools_amd._lib import KmertoolsError
    with pytest.raises(KmertoolsError) as e:
        fn()
    return e.value.code, str(e.value)


def test_thread_runs_protocol_and_errors(torch_mod, device, ctx):
    k, ub, uo, qb, qo = small_case(device, ctx)
    _, hits, want = reference(k, ub, uo, qb, qo)
    n, nu, nr = len(qo) - 1, len(uo) - 1, int(want["tally"][4])
    assert nr > 3
    # the counting call: the number, run_offsets and tally; nothing else is asked for
    off, tally = np.zeros(n + 1, np.uint64), np.zeros(6, np.uint64)
    assert ctx.thread_runs(hits, qo, n, uo, nu, k, run_offsets=off, tally=tally, mem=HOST) == nr
    assert np.array_equal(off, want["run_offsets"]) and np.array_equal(tally, want["tally"])
    assert ctx.thread_runs(hits, qo, n, uo, nu, k, mem=HOST) == nr  # (every output NULL)
    # a room one too small: KT_ERR_ARG, the number set, guards and outputs untouched - both memory kinds
    L = __import__("kmertools_amd._lib", fromlist=["lib"]).lib()
    import ctypes as C
    for mem in (HOST, DEVICE):
        if mem == HOST:
            f = [rb.HostFenced(nr - 1, dt) for dt in (np.uint64, np.uint32, np.uint32, np.uint32)] + [rb.HostFenced(n + 1, np.uint64),
                 rb.HostFenced(nu, np.uint64), rb.HostFenced(nu, np.uint64), rb.HostFenced(6, np.uint64)]
            ptr = [C.c_void_p(x.a.ctypes.data) for x in f]
            ins = [C.c_void_p(a.ctypes.data) for a in (hits, qo, uo)]
            keep = None
        else:
            f = [rb.Fenced(torch_mod, nr - 1, dt) for dt in (torch_mod.int64, torch_mod.int32, torch_mod.int32, torch_mod.int32)] + [
                rb.Fenced(torch_mod, n + 1, torch_mod.int64), rb.Fenced(torch_mod, nu, torch_mod.int64), rb.Fenced(torch_mod, nu, torch_mod.int64),
                rb.Fenced(torch_mod, 6, torch_mod.int64)]
            ptr = [C.c_void_p(x.t.data_ptr()) for x in f]
            keep = [torch_mod.from_numpy(a.view(np.int32 if a.dtype == np.uint32 else np.int64)).cuda() for a in (hits, qo, uo)]
            ins = [C.c_void_p(t.data_ptr()) for t in keep]
        got = C.c_uint64(0)
        rc = L.kt_thread_runs(ctx._h, ins[0], ins[1], n, ins[2], nu, k, ptr[0], ptr[1], ptr[2], ptr[3], ptr[4], nr - 1, C.byref(got), ptr[5],
                              ptr[6], ptr[7], mem)
        torch_mod.cuda.synchronize()
        assert rc == 1 and got.value == nr, (mem, rc, got.value)
        for x in f:
            x.check("room one too small")
            body = x.a.view(np.uint8) if mem == HOST else x.t.view(torch_mod.uint8).cpu().numpy()
            assert (body == rb.GUARD).all(), "an output was written"
    # every argument error; the outputs stay as they were
    o = {name: want[name].copy() for name in RUN_KEYS}
    off2 = np.full(n + 1, 77, np.uint64)
    args = dict(hits=hits, read_offsets=qo, n_reads=n, unitig_offsets=uo, n_unitigs=nu, k=k, run_start=o["run_start"], run_len=o["run_len"],
                run_unitig=o["run_unitig"], run_upos=o["run_upos"], run_offsets=off2, max_runs=nr, mem=HOST)
    for change, text in ((dict(mem=2), "bad mem"), (dict(k=0), "k must be"), (dict(k=32), "k must be"), (dict(read_offsets=None), "null buffer"),
                         (dict(unitig_offsets=None), "null buffer"), (dict(hits=None), "null hits"), (dict(run_start=None), "null run array"),
                         (dict(run_len=None), "null run array"), (dict(run_unitig=None), "null run array"), (dict(run_upos=None), "null run array"),
                         (dict(n_unitigs=1 << 31), "unitigs")):
        code, msg = err_code(device, lambda: ctx.thread_runs(**{**args, **change}))
        assert code == 1 and text in msg and "kt_thread_runs" in msg, (change, msg)
        assert all(np.array_equal(o[name], want[name]) for name in RUN_KEYS) and (off2 == 77).all(), change
    big_u = np.array([0, 1 << 31], np.uint64)
    code, msg = err_code(device, lambda: ctx.thread_runs(**{**args, "unitig_offsets": big_u, "n_unitigs": 1}))
    assert code == 1 and "unitig bases" in msg
    assert L.kt_thread_runs(None, None, None, 0, None, 0, k, None, None, None, None, None, 0, C.byref(got), None, None, None, HOST) == 1
    assert L.kt_thread_runs(ctx._h, None, None, 0, None, 0, k, None, None, None, None, None, 0, None, None, None, None, HOST) == 1
    # no reads: no runs, run_offsets[0] = 0 and a zero tally
    off1, t1 = np.full(1, 9, np.uint64), np.full(6, 9, np.uint64)
    assert ctx.thread_runs(None, None, 0, uo, nu, k, run_offsets=off1, tally=t1, mem=HOST) == 0 and off1[0] == 0 and not t1.any()


def test_thread_hits_and_index_argument_errors(torch_mod, device, ctx):
    k, ub, uo, qb, qo = small_case(device, ctx)
    ui = device.UnitigIndex(ctx, k, ub, uo)
    try:
        hits = np.full(int(qo[-1]), NO, np.uint32)
        for fn, text in ((lambda: ui.table.thread_hits(qb, qo, len(qo) - 1, hits, 2), "bad mem"),
                         (lambda: ui.table.thread_hits(qb, None, 3, hits, HOST), "null buffer"),
                         (lambda: ui.table.thread_hits(qb, qo, len(qo) - 1, None, HOST), "null buffer"),
                         (lambda: ui.table.thread_hits(None, qo, len(qo) - 1, hits, HOST), "null bases"),
                         (lambda: ui.table.index_sequences(ub, uo, len(uo) - 1, 2), "bad mem")):
            code, msg = err_code(device, fn)
            assert code == 1 and text in msg, msg
        assert (hits == NO).all()
        # a non-empty index is refused, and stays what it was
        before = ui.table.export_host()
        code, msg = err_code(device, lambda: ui.table.index_sequences_host(ub, uo))
        assert code == 1 and "not empty" in msg
        after = ui.table.export_host()
        assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
        ui.table.thread_hits(qb, qo, 0, None, HOST)  # no reads: nothing to do
    finally:
        ui.close()
    # a sequence set with a repeated k-mer (the second time as its reverse complement) is refused, the table left empty
    rng = np.random.default_rng(9)
    s = random_seq(rng, 200)
    for dup in (s[50:50 + k], rc_bytes(s[120:120 + k])):
        b, o = device.to_csr([s, random_seq(rng, 40) + dup + random_seq(rng, 10)])
        t = device.Counter(ctx, k, 1 << 12)
        try:
            code, msg = err_code(device, lambda: t.index_sequences_host(b, o))
            assert code == 1 and "more than once" in msg and t.size() == 0
            assert t.index_sequences_host(*device.to_csr([s])) == 200 - k + 1  # (and is usable)
        finally:
            t.close()
    # offsets[n] = 2^31 - 1 is refused from the offsets alone: a real buffer of that size, so that nothing wrong reads invalid memory
    big = torch_mod.empty((1 << 31) - 1, dtype=torch_mod.uint8, device="cuda")
    o = torch_mod.tensor([0, (1 << 31) - 1], dtype=torch_mod.int64, device="cuda")
    t = device.Counter(ctx, 31, 1 << 12)
    try:
        code, msg = err_code(device, lambda: t.index_sequences(big, o, 1))
        assert code == 1 and "2^31 - 2" in msg and t.size() == 0
    finally:
        t.close()
        del big


# ---- 6. accumulation over batches, scratch between other entry points, the table's life --------------------------------------------

def test_thread_tallies_accumulate_over_two_batches(torch_mod, device, ctx):
    k, ub, uo, qb, qo = small_case(device, ctx, seed=4)
    _, _, want = reference(k, ub, uo, qb, qo)
    ui = device.UnitigIndex(ctx, k, ub, uo)
    try:
        uh, ur = np.zeros(len(uo) - 1, np.uint64), np.zeros(len(uo) - 1, np.uint64)
        half, tally = (len(qo) - 1) // 2, np.zeros(6, np.uint64)
        cut = int(qo[half])
        for b, o in ((qb[:cut], qo[:half + 1]), (qb[cut:], qo[half:] - qo[half])):
            tally += ui.thread_host(b, o, uh, ur)["tally"]
        assert np.array_equal(tally, want["tally"]) and np.array_equal(uh, want["unitig_hits"]) and np.array_equal(ur, want["unitig_runs"])
    finally:
        ui.close()


def test_thread_between_other_entry_points(torch_mod, device, ctx):
    """the calls claim every scratch buffer of the context; other entry points before, between and after them"""
    k, ub, uo, qb, qo = small_case(device, ctx, seed=6)
    index, want_hits, want = reference(k, ub, uo, qb, qo)
    c = device.Counter(ctx, k, 1 << 14)
    c.add_reads_host(qb, qo)
    prof = c.profile_host(qb, qo)
    ui = device.UnitigIndex(ctx, k, ub, uo)
    try:
        km = ctx.kmers_host(qb, qo, k)
        hits = ui.table.thread_hits_host(qb, qo)
        st = ctx.profile_stats_host(prof, qo)
        got = ctx.thread_runs_host(hits, qo, uo, k)
        assert np.array_equal(c.profile_host(qb, qo), prof)
        got2 = ui.thread_host(qb, qo)
        assert np.array_equal(hits, want_hits) and np.array_equal(got2["hits"], want_hits)
        same_runs(got, want), same_runs(got2, want)
        assert all(np.array_equal(a, b) for a, b in zip(km, ctx.kmers_host(qb, qo, k)))
        assert all(np.array_equal(st[n], v) for n, v in ctx.profile_stats_host(prof, qo).items())
        assert np.array_equal(np.concatenate(c.unitigs()[:2]), np.concatenate(graph_unitigs(device, ctx, k, [qb[int(qo[i]):int(qo[i + 1])].tobytes() for i in range(len(qo) - 1)])))
    finally:
        ui.close()
        c.close()


def test_thread_index_through_the_tables_life(torch_mod, device, ctx, tmp_path):
    """an index of the unitigs after clip_tips, and of a table loaded with Counter.from_file"""
    k = 17
    rng = np.random.default_rng(8)
    reads, special = graph_reads(rng, k, 2500, 200)
    b, o = device.to_csr(reads + special)
    c = device.Counter(ctx, k, 1 << 16)
    try:
        c.add_reads_host(b, o)
        c.save(str(tmp_path / "t.ktab"))
        c.clip_tips()
        ub, uo, _, _ = c.unitigs()
    finally:
        c.close()
    qb, qo = device.to_csr(reads[:80] + [rc_bytes(r) for r in reads[80:120]])
    clipped = check_both(torch_mod, device, ctx, k, ub, uo, qb, qo, "after clip_tips")
    f = device.Counter.from_file(ctx, str(tmp_path / "t.ktab"))
    try:
        ub2, uo2, _, _ = f.unitigs()
    finally:
        f.close()
    whole = check_both(torch_mod, device, ctx, k, ub2, uo2, qb, qo, "from_file")
    # the counted reads miss nothing in their own graph; clipping can only take hits away
    assert whole["tally"][2] == 0 and whole["tally"][0] == clipped["tally"][0] and clipped["tally"][1] <= whole["tally"][1]


# ---- 7. the CLI end to end -----------------------------------------------------------------------------------------------------------

def run(*args):
    return subprocess.run([CLI, *map(str, args)], capture_output=True, timeout=600)


@pytest.mark.parametrize("k", [15, 31])
def test_thread_cli_end_to_end(oracle, tmp_path, k):
    import test_ctr_unitigs as tu
    assert os.path.exists(CLI)
    rng = np.random.default_rng(k)
    graph_fa, reads_fq = tmp_path / "graph.fasta", tmp_path / "reads.fastq"
    cyc = random_seq(rng, 300)
    sample = tu.noisy_reads(90 + k, 300, k, 3000) + [cyc + cyc[:k - 1]] * 2
    graph_fa.write_bytes(b"".join(b">rec%d lane=%d\n%s\n" % (i, i % 5, s) for i, s in enumerate(sample)))
    threaded = sample[:100] + [rc_bytes(s) for s in sample[100:150]] + [cyc * 2 + cyc[:k - 1], random_seq(rng, 120), b"ACGT"]
    reads_fq.write_bytes(b"".join(b"@q%d extra words\n%s\n+\n%s\n" % (i, s, b"I" * len(s)) for i, s in enumerate(threaded)))
    tk, tc = tu.sorted_table(*oracle.count_reads(*oracle.to_csr([s for _, s in oracle.read_records(str(graph_fa))]), k))
    table = tu.strings_table(tk, tc, k)
    ids, reads = ["q%d" % i for i in range(len(threaded))], [s.decode() for s in threaded]
    for lo, hi, flags in ((1, gr.U32, []), (2, 6, ["--min-count", 2, "--max-count", 6])):
        want = tr.want_files(table, k, ids, reads, lo, hi)
        d = tmp_path / ("out%d" % lo)
        r = run("thread", "-i", reads_fq, "-a", graph_fa, "-o", d, "-k", k, *flags)
        assert r.returncode == 0, r.stderr
        assert sorted(os.listdir(d)) == sorted(want)
        for name, text in want.items():
            assert (d / name).read_bytes() == text, (k, lo, name)
        # (the narrow range keeps a part of the graph only)
        assert want["thread.gaf"].count(b"\n") > (100 if lo == 1 else 20) and b"<" in want["thread.gaf"] and b">" in want["thread.gaf"]
        if lo == 1:
            # the files of `unitigs --gfa` for the same table and range, byte for byte
            r = run("unitigs", "-i", graph_fa, "-o", tmp_path / "u", "-k", k, "--gfa")
            assert r.returncode == 0, r.stderr
            for name in ("unitigs.fa", "unitigs.gfa"):
                assert (tmp_path / "u" / name).read_bytes() == (d / name).read_bytes()
            # --table gives the same bytes as -a; --stats-only writes the two statistics files alone
            r = run("ctr", "-i", graph_fa, "-o", tmp_path / "c", "-k", k, "--save-table", tmp_path / "t.ktab")
            assert r.returncode == 0, r.stderr
            r = run("thread", "-i", reads_fq, "--table", tmp_path / "t.ktab", "-o", tmp_path / "viatable", "-k", k)
            assert r.returncode == 0, r.stderr
            for name, text in want.items():
                assert (tmp_path / "viatable" / name).read_bytes() == text, (k, "--table", name)
            r = run("thread", "-i", reads_fq, "-a", graph_fa, "-o", tmp_path / "so", "-k", k, "--stats-only")
            assert r.returncode == 0, r.stderr
            assert sorted(os.listdir(tmp_path / "so")) == ["thread.stats", "thread.unitigs"]
            for name in ("thread.stats", "thread.unitigs"):
                assert (tmp_path / "so" / name).read_bytes() == want[name]
