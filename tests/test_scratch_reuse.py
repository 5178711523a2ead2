"""The context's scratch buffers across calls: every host-memory entry point that kmertools_amd.device reaches, called on
ONE context interleaved with all the others and three times each - a small batch, a large one, the small one again - must
give bit for bit what the same call gives on a fresh context of its own; the same with a device-memory call of another
entry point between the host calls; the three entry points that add into their caller's arrays, over two hash partitions
into pre-filled arrays, on both memory kinds; and `mem` = 2 is refused by the five entry points that used not to look.

The small batch (3 reads of 40, 0 and 70 bases) is one 8192-base segment; the large one (96 reads of 50..400 bases, some N)
is more than two, and asks every one of the six buffers for more than the small round left there (a buffer keeps
request * 1.125 + 256 bytes), so every buffer is freed and grown between the first and the second round and the third
round runs in buffers larger than it asks for."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

K = 11            # the tables' and the sketches' k
CAP = 1 << 16     # slots of a table
S = 8             # hashes per sketch
SEG = 8192        # ktseg::SEG
ACGT = np.frombuffer(b"ACGT", np.uint8)
HOST, DEVICE = 0, 1


class Reads:
    def __init__(self, lens, seed, n_every):
        rng = np.random.default_rng(seed)
        lens = np.asarray(lens, np.uint64)
        self.n = len(lens)
        self.offsets = np.zeros(self.n + 1, np.uint64)
        self.offsets[1:] = np.cumsum(lens, dtype=np.uint64)
        self.total = int(self.offsets[-1])
        self.clean = ACGT[rng.integers(0, 4, self.total)]   # (cgr refuses anything but ACGT)
        self.bases = self.clean.copy()
        if n_every:
            # some N; and the first 50 bases again at the start of the last two reads, the last with one base changed:
            # k-mers that occur twice (solid at min_count 2) and a base that correct_support finds support for
            self.bases[n_every // 2::n_every] = ord("N")
            for i in (self.n - 2, self.n - 1):
                self.bases[int(self.offsets[i]): int(self.offsets[i]) + 50] = self.bases[:50]
            at = int(self.offsets[self.n - 1]) + 35
            self.bases[at] = ACGT[(int(np.nonzero(ACGT == self.bases[at])[0][0]) + 1) % 4]
        half = self.n // 2 if self.n > 3 else 1              # the reads of the second table of compare / setop
        self.head_offsets = self.offsets[: half + 1].copy()
        self.head_bases = self.bases[: int(self.head_offsets[-1])].copy()


SMALL = Reads([40, 0, 70], 1, 0)
LARGE = Reads(np.random.default_rng(2).integers(50, 401, 96), 3, 37)
MEDIUM = Reads([1000] * 20, 4, 0)   # what the device-memory calls between the host calls work on


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    return torch


@pytest.fixture(scope="module")
def device():
    from kmertools_amd import device
    return device


def table(device, ctx, bases, offsets):
    t = device.Counter(ctx, K, CAP)
    t.add_reads_host(bases, offsets)
    return t


# ---- the host-memory calls: name -> (entry points, fn(device, ctx, reads) -> tuple of arrays) ---------------------------

def op_kmers(device, ctx, r):
    return ctx.kmers_host(r.bases, r.offsets, K)


def op_oligo4(device, ctx, r):
    return (ctx.oligo_host(r.bases, r.offsets, 4),)


def op_oligo9(device, ctx, r):
    return (ctx.oligo_host(r.bases, r.offsets, 9, dtype="f32"),)


def op_cgr(device, ctx, r):
    return (ctx.cgr_host(r.clean, r.offsets, 1),)


def op_min_whole(device, ctx, r):
    return ctx.minimisers_host(r.bases, r.offsets, 0, 7)


def op_min_w15(device, ctx, r):
    return ctx.minimisers_host(r.bases, r.offsets, 15, 7)


def op_min_count(device, ctx, r):
    evo, empty = np.zeros(r.n + 1, np.uint64), np.zeros(1, np.uint64)
    cnt = ctx.minimisers(r.bases, r.offsets, r.n, 15, 7, evo, empty, empty, empty, 0, HOST)
    return (np.array([cnt], np.uint64), evo)


def op_add_reads_export(device, ctx, r):
    t = table(device, ctx, r.bases, r.offsets)
    full = t.export_host()
    ranged = t.export_host(min_count=2)
    t.close()
    return full + ranged


def op_add_pairs(device, ctx, r):
    t = table(device, ctx, r.bases, r.offsets)
    keys, counts = t.export_host()
    t.close()
    t2 = device.Counter(ctx, K, CAP)
    t2.add_pairs_host(keys, counts)
    t2.add_pairs_host(keys[: len(keys) // 2])   # (without counts: one occurrence each)
    out = t2.export_host()
    t2.close()
    return out


def op_lookup(device, ctx, r):
    t = table(device, ctx, r.bases, r.offsets)
    fwd, rev, _ = ctx.kmers_host(r.clean, r.offsets, K)
    out = t.lookup_host(np.minimum(fwd, rev))
    t.close()
    return (out,)


def op_spectrum(device, ctx, r):
    t = table(device, ctx, r.bases, r.offsets)
    hist, tot = t.spectrum(16, totals=True)
    t.close()
    return (hist, np.array(tot, np.uint64))


def op_cov(device, ctx, r):
    t = table(device, ctx, r.bases, r.offsets)
    out = (t.cov_host(r.bases, r.offsets, 2, 4), t.cov_host(r.bases, r.offsets, 2, 4, norm=False, dtype="u32"))
    t.close()
    return out


def op_cov_part(device, ctx, r):
    t = table(device, ctx, r.bases, r.offsets)
    counts = np.zeros((r.n, 4), np.uint32)
    t.cov_part(r.bases, r.offsets, r.n, 2, 4, counts, 1, 0, HOST)
    t.close()
    return (counts,)


def op_read_solidity(device, ctx, r):
    t = table(device, ctx, r.bases, r.offsets)
    out = t.read_solidity_host(r.bases, r.offsets, 2)
    t.close()
    return out


def op_profile(device, ctx, r):
    t = table(device, ctx, r.bases, r.offsets)
    prof = t.profile_host(r.bases, r.offsets)
    stats = ctx.profile_stats_host(prof, r.offsets)
    t.close()
    return (prof,) + tuple(stats[name] for name in ("n_kmers", "n_present", "min", "median", "max", "sum"))


def op_correct(device, ctx, r):
    t = table(device, ctx, r.bases, r.offsets)
    prof = t.profile_host(r.bases, r.offsets)
    sup = np.zeros(r.total, np.uint32)
    t.correct_support(r.bases, r.offsets, r.n, prof, 2, 0xFFFFFFFF, sup, HOST)
    out, ns, na = r.bases.copy(), np.zeros(r.n, np.uint32), np.zeros(r.n, np.uint32)
    ctx.correct_apply(r.bases, r.offsets, r.n, sup, 1, 0, out, ns, na, HOST)
    t.close()
    return (sup, out, ns, na)


def op_sketch(device, ctx, r):
    return ctx.sketch_host(r.bases, r.offsets, K, S)


def op_sketch_merge(device, ctx, r):
    hashes, sizes, _ = ctx.sketch_host(r.bases, r.offsets, K, S)
    groups = np.array([0, r.n // 3, r.n // 3, r.n], np.uint64)   # (the last group of the large batch takes more than two rounds: both buffers of the tree)
    return ctx.sketch_merge(hashes, sizes, groups)


def op_sketch_pairs(device, ctx, r):
    hashes, sizes, _ = ctx.sketch_host(r.bases, r.offsets, K, S)
    return ctx.sketch_pairs_host(hashes, sizes) + ctx.sketch_pairs_host(hashes, sizes, hashes[::-1].copy(), sizes[::-1].copy())


def op_route(device, ctx, r):
    keys, counts = ctx.route_host(r.bases, r.offsets, K, 4)
    keys = keys.copy()
    ends = np.cumsum(counts).astype(np.int64)
    for lo, hi in zip(np.concatenate(([0], ends[:-1])), ends):   # (the order inside an owner's region is not fixed)
        keys[lo:hi].sort()
    return (keys, counts)


def op_compare(device, ctx, r):
    a, b = table(device, ctx, r.bases, r.offsets), table(device, ctx, r.head_bases, r.head_offsets)
    m, tot = a.compare(b, 4, 4, totals=True)
    a.close(), b.close()
    return (m, np.array([tot[name] for name in device.Counter.COMPARE_TOTALS], np.uint64))


def op_setop(device, ctx, r):
    a, b = table(device, ctx, r.bases, r.offsets), table(device, ctx, r.head_bases, r.head_offsets)
    out = a.setop(b, "union", "sum") + a.setop(b, "subtract")
    a.close(), b.close()
    return out


OPS = [
    ("kmers", ("kt_kmers",), op_kmers),
    ("oligo k=4", ("kt_oligo_batch",), op_oligo4),
    ("add_reads, export", ("kt_ctr_add_reads_part", "kt_ctr_export"), op_add_reads_export),
    ("cgr", ("kt_cgr_points",), op_cgr),
    ("sketch", ("kt_sketch_batch",), op_sketch),
    ("lookup", ("kt_ctr_lookup", "kt_kmers"), op_lookup),
    ("minimisers w=0", ("kt_minimisers",), op_min_whole),
    ("cov", ("kt_cov_batch",), op_cov),
    ("oligo k=9", ("kt_oligo_batch",), op_oligo9),
    ("route", ("kt_ctr_route",), op_route),
    ("read_solidity", ("kt_ctr_read_solidity",), op_read_solidity),
    ("minimisers w=15", ("kt_minimisers",), op_min_w15),
    ("profile, profile_stats", ("kt_ctr_profile", "kt_profile_stats"), op_profile),
    ("add_pairs", ("kt_ctr_add_pairs",), op_add_pairs),
    ("sketch_merge", ("kt_sketch_merge", "kt_sketch_batch"), op_sketch_merge),
    ("spectrum", ("kt_ctr_spectrum",), op_spectrum),
    ("correct_support, correct_apply", ("kt_ctr_correct_support", "kt_correct_apply", "kt_ctr_profile"), op_correct),
    ("minimisers count only", ("kt_minimisers",), op_min_count),
    ("cov_part", ("kt_cov_batch_part",), op_cov_part),
    ("setop", ("kt_ctr_setop",), op_setop),
    ("sketch_pairs", ("kt_sketch_pairs", "kt_sketch_batch"), op_sketch_pairs),
    ("compare", ("kt_ctr_compare",), op_compare),
]
ROUNDS = (("small", SMALL), ("large", LARGE), ("small again", SMALL))


@pytest.fixture(scope="module")
def alone(torch_mod, device):
    """every call's result on a fresh context of its own: (name, round) -> tuple of arrays"""
    want = {}
    for tag, reads in ROUNDS[:2]:
        for name, _, fn in OPS:
            ctx = device.Context(0)
            want[name, tag] = fn(device, ctx, reads)
            ctx.close()
    for name, _, _ in OPS:
        want[name, "small again"] = want[name, "small"]
    return want


def same(got, want, what):
    assert len(got) == len(want), what
    for i, (g, w) in enumerate(zip(got, want)):
        g, w = np.asarray(g), np.asarray(w)
        assert g.dtype == w.dtype and g.shape == w.shape, (what, i, g.dtype, w.dtype, g.shape, w.shape)
        assert g.tobytes() == w.tobytes(), (what, i)


def test_the_large_batch_outgrows_what_the_small_round_leaves_in_every_buffer(device):
    """the largest request of the small round per buffer (of every call in OPS, by the formulas of the entry points), and
    one request of the large round that is more than 1.125 x that + 256 bytes"""
    assert SMALL.total == 110 and (SMALL.total + SEG - 1) // SEG == 1
    assert LARGE.n == 96 and LARGE.total > 2 * SEG
    bins9 = device.bins(9, True)

    def a256(x):
        return (x + 255) & ~255

    def distinct(r):   # the canonical k-mers of the reads
        code = np.full(256, -1, np.int64)
        code[[65, 67, 71, 84]] = [0, 1, 2, 3]
        place = 4 ** np.arange(K - 1, -1, -1, dtype=np.int64)
        keys = set()
        for i in range(r.n):
            c = code[r.bases[int(r.offsets[i]): int(r.offsets[i + 1])]]
            if len(c) < K:
                continue
            w = np.lib.stride_tricks.sliding_window_view(c, K)
            w = w[(w >= 0).all(1)]
            keys.update(np.minimum((w * place).sum(1), ((3 - w[:, ::-1]) * place).sum(1)).tolist())
        return len(keys)

    d_small, d_large = distinct(SMALL), distinct(LARGE)
    s, lg = SMALL, LARGE
    events_small = s.total  # (at most one minimiser event per base)
    small = {
        "BASES": max(s.total + 64, 4 * s.total + 4, 2 * s.n * S * 8 + 8),                        # stage; profile_stats; sketch_pairs
        "OFFSETS": max((s.n + 1) * 8, 2 * s.n * 4 + 8),                                          # stage; sketch_pairs
        "OUT": max(s.n * bins9 * 4, 17 * s.total, a256((s.n + 1) * 8) + 3 * a256(events_small * 8) + 256),  # oligo k=9; kmers; minimisers
        "AUX0": max((1 + 2) * 8, (256 * 1 + 256) * 8),                                           # segment index; setop's sort of <= 4096 pairs
        "AUX1": max(s.n * bins9 * 4, 8 * s.total, 8 * d_small, 16 * 256 + 8 * 256 * 2),           # oligo k=9; route; pairs; minimisers' internals
        "AUX2": max(2 * 64 * 8, a256(events_small * 32) + events_small + 256, 4 * s.total),       # route; minimiser events; correct_support
    }
    large = {
        "BASES": lg.total + 64,                              # stage_batch
        "OFFSETS": (lg.n + 1) * 8,                           # stage_batch
        "OUT": lg.n * bins9 * 4,                             # oligo k=9, f32 rows
        "AUX0": (256 * ((d_large + 4095) // 4096) + 256) * 8,  # setop's sort of the union: one histogram per 4096 pairs
        "AUX1": lg.n * bins9 * 4,                            # oligo k=9, the u32 counters
        "AUX2": 4 * lg.total,                                # correct_support's support array
    }
    assert d_large > 4096
    for buf in small:
        assert large[buf] > small[buf] * 1.125 + 256, (buf, small[buf], large[buf])


def test_interleaved_host_calls_on_one_context(torch_mod, device, alone):
    ctx = device.Context(0)
    for tag, reads in ROUNDS:
        for name, _, fn in OPS:
            same(fn(device, ctx, reads), alone[name, tag], (name, tag))
    ctx.close()


def test_device_calls_between_the_host_calls(torch_mod, device, alone):
    torch = torch_mod
    ctx = device.Context(0, stream=torch.cuda.current_stream().cuda_stream)
    r = MEDIUM
    d_bases = torch.from_numpy(r.bases).cuda()
    d_offsets = torch.from_numpy(r.offsets.view(np.int64)).cuda()
    solo = device.Context(0)
    want_kmers = solo.kmers_host(r.bases, r.offsets, K)
    want_sketch = solo.sketch_host(r.bases, r.offsets, K, S)
    want_oligo = solo.oligo_host(r.bases, r.offsets, 9, dtype="f32")
    solo.close()

    def dev_kmers():
        fwd, rev = torch.zeros(r.total, dtype=torch.int64, device="cuda"), torch.zeros(r.total, dtype=torch.int64, device="cuda")
        valid = torch.zeros(r.total, dtype=torch.uint8, device="cuda")
        ctx.kmers(d_bases, d_offsets, r.n, K, fwd, rev, valid, DEVICE)
        torch.cuda.synchronize()
        idx = np.nonzero(valid.cpu().numpy())[0]
        same((fwd.cpu().numpy().view(np.uint64)[idx], rev.cpu().numpy().view(np.uint64)[idx], idx.astype(np.uint64)), want_kmers, "device kmers")

    def dev_sketch():
        hashes = torch.zeros((r.n, S), dtype=torch.int64, device="cuda")
        sizes, nk = torch.zeros(r.n, dtype=torch.int32, device="cuda"), torch.zeros(r.n, dtype=torch.int32, device="cuda")
        ctx.sketch(d_bases, d_offsets, r.n, K, S, hashes, sizes, nk, 0, DEVICE)
        torch.cuda.synchronize()
        same((hashes.cpu().numpy().view(np.uint64), sizes.cpu().numpy().view(np.uint32), nk.cpu().numpy().view(np.uint32)), want_sketch,
             "device sketch")

    def dev_oligo():
        out = torch.zeros((r.n, device.bins(9, True)), dtype=torch.float32, device="cuda")
        ctx.oligo(d_bases, d_offsets, r.n, 9, out, dtype="f32", mem=DEVICE)
        torch.cuda.synchronize()
        same((out.cpu().numpy(),), (want_oligo,), "device oligo")

    between = [("kt_kmers", dev_kmers), ("kt_sketch_batch", dev_sketch), ("kt_oligo_batch", dev_oligo)]
    turn = 0
    for tag, reads in ROUNDS:
        for i, (name, entries, fn) in enumerate(OPS):
            same(fn(device, ctx, reads), alone[name, tag], (name, tag))
            after = OPS[(i + 1) % len(OPS)][1]
            for j in range(len(between)):   # the next device-memory call that is neither neighbour's entry point
                entry, call = between[(turn + j) % len(between)]
                if entry not in entries and entry not in after:
                    call()
                    turn += j + 1
                    break
            else:
                raise AssertionError("no device call fits between %s and its successor" % name)
    ctx.close()


@pytest.mark.parametrize("mem", [HOST, DEVICE], ids=["host", "device"])
def test_adding_entry_points_over_two_partitions_into_prefilled_arrays(torch_mod, device, mem):
    torch = torch_mod
    r = LARGE
    ctx = device.Context(0, stream=torch.cuda.current_stream().cuda_stream)
    t = table(device, ctx, r.bases, r.offsets)
    rng = np.random.default_rng(5)
    prof = t.profile_host(r.bases, r.offsets)
    if mem == DEVICE:
        bases, offsets = torch.from_numpy(r.bases).cuda(), torch.from_numpy(r.offsets.view(np.int64)).cuda()
        d_prof = torch.from_numpy(prof.view(np.int32)).cuda()
    else:
        bases, offsets, d_prof = r.bases, r.offsets, prof

    def arr(a):   # a u32 array where the calls take it
        return torch.from_numpy(a.view(np.int32).copy()).cuda() if mem == DEVICE else a.copy()

    def back(x):
        if mem == DEVICE:
            torch.cuda.synchronize()
            return x.cpu().numpy().view(np.uint32)
        return x

    # cov_part
    pre = rng.integers(0, 1000, (r.n, 4)).astype(np.uint32)
    one, two = arr(np.zeros_like(pre)), arr(pre)
    t.cov_part(bases, offsets, r.n, 2, 4, one, 1, 0, mem)
    for part in (0, 1):
        t.cov_part(bases, offsets, r.n, 2, 4, two, 2, part, mem)
    one = back(one)
    assert one.sum() > 0
    assert np.array_equal(back(two), pre + one)

    # read_solidity: n_kmers and n_solid add, first_weak takes the minimum
    pre_k, pre_s = rng.integers(0, 1000, r.n).astype(np.uint32), rng.integers(0, 1000, r.n).astype(np.uint32)
    pre_w = np.where(rng.integers(0, 2, r.n) == 1, rng.integers(0, 400, r.n), 0xFFFFFFFF).astype(np.uint32)
    one = [arr(np.zeros(r.n, np.uint32)), arr(np.zeros(r.n, np.uint32)), arr(np.full(r.n, 0xFFFFFFFF, np.uint32))]
    two = [arr(pre_k), arr(pre_s), arr(pre_w)]
    t.read_solidity(bases, offsets, r.n, 2, 0xFFFFFFFF, one[0], one[1], one[2], mem, 1, 0)
    for part in (0, 1):
        t.read_solidity(bases, offsets, r.n, 2, 0xFFFFFFFF, two[0], two[1], two[2], mem, 2, part)
    one, two = [back(x) for x in one], [back(x) for x in two]
    assert one[0].sum() > 0 and one[1].sum() > 0 and (one[2] != 0xFFFFFFFF).any()
    assert np.array_equal(two[0], pre_k + one[0])
    assert np.array_equal(two[1], pre_s + one[1])
    assert np.array_equal(two[2], np.minimum(pre_w, one[2]))

    # correct_support (bytes of an entry are counters of their own: a prefill that leaves them room)
    pre = (rng.integers(0, 64, r.total).astype(np.uint32) * 0x01010101).astype(np.uint32)
    one, two = arr(np.zeros(r.total, np.uint32)), arr(pre)
    t.correct_support(bases, offsets, r.n, d_prof, 2, 0xFFFFFFFF, one, mem, 1, 0)
    for part in (0, 1):
        t.correct_support(bases, offsets, r.n, d_prof, 2, 0xFFFFFFFF, two, mem, 2, part)
    one = back(one)
    assert one.any()
    assert np.array_equal(back(two), pre + one)
    t.close()
    ctx.close()


def test_mem_2_is_refused_by_the_five_entry_points_that_used_not_to_check(torch_mod, device):
    """zero-length input: no kernel can come to touch a host pointer, whatever the call makes of `mem`"""
    from kmertools_amd import _lib
    L = _lib.lib()
    ctx = device.Context(0)
    t = device.Counter(ctx, K, CAP)
    n = C.c_uint64()
    owner_counts = np.zeros(4, np.uint64)
    calls = {
        "kt_ctr_add_reads": lambda: L.kt_ctr_add_reads(t._h, None, None, 0, 2),
        "kt_ctr_add_reads_part": lambda: L.kt_ctr_add_reads_part(t._h, None, None, 0, 2, 1, 0),
        "kt_ctr_add_pairs": lambda: L.kt_ctr_add_pairs(t._h, None, None, 0, 2),
        "kt_ctr_export": lambda: L.kt_ctr_export(t._h, None, None, 0, C.byref(n), 2),
        "kt_ctr_route": lambda: L.kt_ctr_route(ctx._h, None, None, 0, K, 4, None, C.c_void_p(owner_counts.ctypes.data), 2),
        "kt_kmers": lambda: L.kt_kmers(ctx._h, None, None, 0, K, None, None, None, 2),
    }
    for name, call in calls.items():
        assert call() == _lib.KT_ERR_ARG, name
        assert "bad mem" in _lib.last_error(), (name, _lib.last_error())
    t.close()
    ctx.close()
