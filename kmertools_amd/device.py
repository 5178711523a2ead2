"""Thin object layer over the C ABI: a Context (one GPU + one stream) and a Counter
(HBM-resident k-mer table).  Two calling styles, same entry points:

* host arrays (numpy): the library stages them through its own device scratch
  (KT_MEM_HOST) - what the `pykmertools` mirror uses;
* device tensors (anything with `.data_ptr()`, e.g. torch tensors on the GPU):
  pointers are passed straight through (KT_MEM_DEVICE) and work is enqueued on the
  context's stream without synchronising - what bench.py and the parity tests use.
  torch is only plumbing here (allocation, streams, torch.distributed).
"""
import contextlib
import ctypes as C
import os

import numpy as np

from . import _lib
from ._lib import KT_F32, KT_F64, KT_MEM_DEVICE, KT_MEM_HOST, KT_U32, check

_DT = {"f64": KT_F64, "f32": KT_F32, "u32": KT_U32, np.float64: KT_F64, np.float32: KT_F32, np.uint32: KT_U32}
_NP = {KT_F64: np.float64, KT_F32: np.float32, KT_U32: np.uint32}
NO_KMER = 0xFFFFFFFF  # KT_NO_KMER: the entry of a profile where no k-mer starts
TIP_KEEP, TIP_TIP, TIP_ISOLATED = 0, 1, 2  # Counter.unitig_tips' marks (KT_TIP_*)
CLIP_ISOLATED = 1  # Counter.clip_tips(drop_isolated=True) (KT_CLIP_ISOLATED)
CLIP_STATS_NAMES = ("rounds", "tips", "tip_nodes", "isolated", "isolated_nodes", "occurrences", "converged")
BUBBLE_POP = 4  # Counter.unitig_bubbles' mark (KT_BUBBLE_POP): a bit beside TIP_TIP and TIP_ISOLATED
SIMPLIFY_STATS_NAMES = ("rounds", "tips", "tip_nodes", "isolated", "isolated_nodes", "popped", "popped_nodes", "bubbles", "occurrences",
                        "converged")
NO_COMPONENT = 0xFFFFFFFF  # KT_NO_COMPONENT: the component of a read without a run
COMPONENT_FIELDS = 5  # KT_COMPONENT_FIELDS: the columns of Context.unitig_components' stats
COMPONENT_STATS_NAMES = ("unitigs", "nodes", "count_sum", "links", "first_unitig")


def _ptr(x):
    """device/host address of a numpy array, a tensor with data_ptr(), an int or None"""
    if x is None:
        return None
    if isinstance(x, int):
        return C.c_void_p(x)
    if isinstance(x, np.ndarray):
        return C.c_void_p(x.ctypes.data)
    return C.c_void_p(x.data_ptr())


def bins(k, count_min=True):
    out = C.c_uint64()
    check(_lib.lib().kt_bins(k, int(bool(count_min)), C.byref(out)))
    return out.value


def pos_map(k):
    """(min_mer_pos_map u32[4^k], pos_min_mer u64[kcount], kcount) - kmer.rs:54-73"""
    n = 4 ** k
    m = np.zeros(n, np.uint32)
    pk = np.zeros(n, np.uint64)
    cnt = C.c_uint32()
    check(_lib.lib().kt_pos_map(k, _ptr(m), _ptr(pk), C.byref(cnt)))
    return m, pk[: cnt.value].copy(), cnt.value


def rev_comp(kmer, k):
    return int(_lib.lib().kt_rev_comp(kmer, k))


def numeric_to_kmer(kmer, k):
    buf = C.create_string_buffer(k + 1)
    check(_lib.lib().kt_numeric_to_kmer(kmer, k, buf))
    return buf.value.decode()


def kmer_to_numeric(s):
    b = s.encode("latin-1") if isinstance(s, str) else bytes(s)
    f, r = C.c_uint64(), C.c_uint64()
    check(_lib.lib().kt_kmer_to_numeric(b, len(b), C.byref(f), C.byref(r)))
    return f.value, r.value


def cgr_coords(k, vecsize):
    xy = np.zeros((bins(k, True), 2), np.float64)
    check(_lib.lib().kt_cgr_coords(k, float(vecsize), _ptr(xy)))
    return xy


def owner_of(kmer, n_owners):
    """hash partition of a k-mer among n_owners (out-of-core passes, kt_ctr_route): the LOW hash bits"""
    return int(_lib.lib().kt_owner_of(int(kmer), int(n_owners)))


def shard_minimiser(k):
    """-> (m, w): the minimiser length and the window (m-mers per k-mer) the sharded counter uses for k-mers of length k"""
    m, w = C.c_uint32(), C.c_uint32()
    check(_lib.lib().kt_shard_minimiser(int(k), C.byref(m), C.byref(w)))
    return m.value, w.value


def shard_owner_of(kmer, k, n_ranks):
    """the rank that owns a k-mer (either strand) of length k among n_ranks: by its minimiser's hash (kt_shard_owner_of)"""
    return int(_lib.lib().kt_shard_owner_of(int(kmer), int(k), int(n_ranks)))


def mash_distance(shared, denom, k):
    """the Mash distance of a sketch pair: 1 when nothing is shared, else min(1, -ln(2j / (1 + j)) / k) with
    j = shared / denom (kt_mash_distance, the one implementation of the formula)"""
    return float(_lib.lib().kt_mash_distance(int(shared), int(denom), int(k)))


def scaled_max_hash(scaled):
    """the largest hash a scaled sketch keeps, 0xFFFFFFFFFFFFFFFF // scaled; 0 for scaled == 0 (kt_scaled_max_hash)"""
    return int(_lib.lib().kt_scaled_max_hash(int(scaled)))


def containment_ani(shared, size, k):
    """the containment-to-ANI estimate (shared / size) ** (1 / k): 0 when shared or size is 0, 1 when they are equal
    (kt_containment_ani, the one implementation of the formula)"""
    return float(_lib.lib().kt_containment_ani(int(shared), int(size), int(k)))


def _card_p(registers):
    """the precision of a register array: its length is 2^p"""
    m = int(registers.size)
    if m < 1 or m & (m - 1):
        raise ValueError("a register array holds 2^p registers, not %d" % m)
    return m.bit_length() - 1


def card_estimate(registers):
    """-> (estimate, zero_registers): the distinct k-mers behind HyperLogLog registers (u8[2^p], host), by Ertl's improved
    raw estimator (kt_card_estimate)"""
    registers = np.ascontiguousarray(registers, np.uint8)
    est, zeros = C.c_double(), C.c_uint64()
    check(_lib.lib().kt_card_estimate(_ptr(registers), _card_p(registers), C.byref(est), C.byref(zeros)))
    return est.value, zeros.value


def card_merge(into, other):
    """into[j] = max(into[j], other[j]) in place (u8[2^p] host arrays of one k, p and seed): the registers of the union
    (kt_card_merge); returns into"""
    other = np.ascontiguousarray(other, np.uint8)
    if not (isinstance(into, np.ndarray) and into.dtype == np.uint8 and into.flags.c_contiguous and into.flags.writeable):
        raise ValueError("card_merge: into must be a writable contiguous uint8 array")
    if into.size != other.size:
        raise ValueError("card_merge: %d registers into %d" % (other.size, into.size))
    check(_lib.lib().kt_card_merge(_ptr(into), _ptr(other), _card_p(into)))
    return into


def table_file_info(path):
    """k, sections, entries and occurrences of a table file, from its headers (host only: kt_table_file_info)"""
    k, s, e, o = C.c_int(), C.c_uint64(), C.c_uint64(), C.c_uint64()
    check(_lib.lib().kt_table_file_info(os.fsencode(path), C.byref(k), C.byref(s), C.byref(e), C.byref(o)))
    return {"k": k.value, "sections": s.value, "entries": e.value, "occurrences": o.value}


def table_file_check(path):
    """the full structural validation of a table file (host only: kt_table_file_check); raises KmertoolsError"""
    check(_lib.lib().kt_table_file_check(os.fsencode(path)))


def card_rel_error(p):
    """the estimator's relative standard error, 1.04 / sqrt(2^p) (kt_card_rel_error)"""
    return float(_lib.lib().kt_card_rel_error(int(p)))


# the cells of Counter.graph's census, in order (kt_ctr_graph): degree_<dL>_<dR> = nodes with those two degrees
GRAPH_CENSUS_NAMES = ("nodes", "occurrences", "degree_sum", "end_sides", "isolated", "tips", "branching") + tuple(
    "degree_%d_%d" % (dl, dr) for dl in range(5) for dr in range(5))


# the cells of Counter.hetmers' census, in order (kt_ctr_hetmers)
HET_CENSUS_NAMES = ("nodes", "occurrences", "degree_0", "degree_1", "degree_2_or_more", "pairs", "minor_sum", "major_sum")


UNITIG_CIRCULAR = 1  # Counter.unitigs' flag bit (KT_UNITIG_CIRCULAR): the unitig is a cycle, linearised at its smallest k-mer


def graph_info_text(info):
    """an info word of Counter.graph as (left4, right4, ends2), `kmertools graph`'s rendering: position x of left4 /
    right4 is "ACGT"[x] when that neighbour is a node, else "."; ends2 is "L" or "." followed by "R" or "." """
    info = int(info)
    right = "".join("ACGT"[x] if info >> x & 1 else "." for x in range(4))
    left = "".join("ACGT"[x] if info >> (4 + x) & 1 else "." for x in range(4))
    return left, right, ("L" if info & 0x200 else ".") + ("R" if info & 0x100 else ".")


def to_csr(seqs):
    """list[str|bytes] -> (bases u8[total], offsets u64[n+1])"""
    bs = [s.encode("latin-1") if isinstance(s, str) else bytes(s) for s in seqs]
    offsets = np.zeros(len(bs) + 1, dtype=np.uint64)
    if bs:
        offsets[1:] = np.cumsum([len(b) for b in bs], dtype=np.uint64)
    joined = b"".join(bs)
    bases = np.frombuffer(joined, dtype=np.uint8).copy() if joined else np.zeros(0, np.uint8)
    return bases, offsets


def view_tensor(addr, shape, dtype, owner=None):
    """a torch tensor over device memory that somebody else owns (no copy, through __cuda_array_interface__); `owner` is
    kept alive by the tensor"""
    import torch
    typestr = {torch.float64: "<f8", torch.float32: "<f4", torch.uint8: "|u1", torch.int32: "<i4", torch.int64: "<i8"}[dtype]

    class _View:
        pass
    v = _View()
    v.__cuda_array_interface__ = {"shape": tuple(int(x) for x in shape), "typestr": typestr, "data": (int(addr), False),
                                  "version": 2, "strides": None}
    v._owner = owner
    t = torch.as_tensor(v, device="cuda")
    t._kt_owner = owner
    return t


class DeviceArray:
    """Device memory handed out by the library (kt_device_alloc_placed), released by close() / garbage collection.
    `tensor(shape, dtype)` views it as a torch tensor (no copy; the view keeps this object alive); `ptr` is the raw
    address for the C-ABI wrappers here, which accept an int where they accept a tensor."""

    def __init__(self, ctx, ptr, nbytes):
        self._ctx, self.ptr, self.nbytes = ctx, int(ptr), int(nbytes)

    def tensor(self, shape, dtype):
        return view_tensor(self.ptr, shape, dtype, owner=self)

    def close(self):
        if self.ptr and self._ctx._h.value:
            _lib.lib().kt_device_free(self._ctx._h, C.c_void_p(self.ptr))
        self.ptr = 0

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Context:
    """One device + one stream (kt_ctx).  `stream` is a raw hipStream_t handle
    (e.g. torch.cuda.current_stream().cuda_stream; 0 = the default stream) to enqueue on,
    or None to let the context own a private stream."""

    def __init__(self, device=0, stream=None):
        self._h = C.c_void_p()
        self.device = device
        own = stream is None
        check(_lib.lib().kt_ctx_create(device, None if own else C.c_void_p(int(stream)), int(own),
                                       C.byref(self._h)))

    def alloc_placed(self, nbytes, probe=None, candidates=8, launches=4):
        """kt_device_alloc_placed: a device array of nbytes, the fastest of up to `candidates` allocations under
        probe(address) - a callable that enqueues the work the array is meant for on this context's stream (None: a plain
        allocation).  -> (DeviceArray, {"candidates": n, "ms": [per candidate], "picked": index}); candidate 0 is the
        plain allocation.  An exception in the probe is re-raised here."""
        exc = []

        def cb(_user, ptr):
            try:
                probe(int(ptr))
                return 0
            except BaseException as e:  # noqa: BLE001 (ctypes would swallow it)
                exc.append(e)
                return 1
        fn = _lib.PROBE_FN(cb) if probe is not None else None
        out = C.c_void_p()
        ms = (C.c_double * 16)()
        n, picked = C.c_int(0), C.c_int(0)
        rc = _lib.lib().kt_device_alloc_placed(self._h, int(nbytes), int(candidates), int(launches),
                                               C.cast(fn, C.c_void_p) if fn is not None else None, None, C.byref(out), ms,
                                               C.byref(n), C.byref(picked))
        if exc:
            raise exc[0]
        check(rc)
        info = {"candidates": n.value, "ms": [round(ms[i], 4) for i in range(n.value)], "picked": picked.value}
        return DeviceArray(self, out.value, nbytes), info

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            _lib.lib().kt_ctx_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def sync(self):
        check(_lib.lib().kt_ctx_sync(self._h))

    def cu_count(self):
        """-> (the compute units this context's grids are sized by, the device's compute units)"""
        n, dev = C.c_uint32(), C.c_uint32()
        check(_lib.lib().kt_ctx_cu_limit(self._h, C.byref(n), C.byref(dev)))
        return n.value, dev.value

    @contextlib.contextmanager
    def cu_limit(self, n):
        """`with ctx.cu_limit(n):` - the launches inside size their grids as if the device had n compute units
        (kt_ctx_set_cu_limit: 0 = the device's count, more than that is clamped); the value from before is put back on
        the way out, also by an exception.  Results never depend on it: it leaves room on a shared card, and it lets a
        test take every grid-stride loop round several times at small sizes."""
        before, dev = self.cu_count()
        check(_lib.lib().kt_ctx_set_cu_limit(self._h, int(n)))
        try:
            yield self
        finally:
            check(_lib.lib().kt_ctx_set_cu_limit(self._h, 0 if before == dev else before))

    # -- comp oligo / comp cgr -k ------------------------------------------------------
    def oligo(self, bases, offsets, n_reads, k, out, count_min=True, norm=True, total_step=1, dtype="f64",
              mem=KT_MEM_DEVICE):
        check(_lib.lib().kt_oligo_batch(self._h, _ptr(bases), _ptr(offsets), n_reads, k, int(bool(count_min)),
                                        int(bool(norm)), int(total_step), _DT[dtype], _ptr(out), mem))
        return out

    def oligo_host(self, bases, offsets, k, count_min=True, norm=True, total_step=1, dtype="f64"):
        bases = np.ascontiguousarray(bases, np.uint8)
        offsets = np.ascontiguousarray(offsets, np.uint64)
        n = len(offsets) - 1
        out = np.zeros((n, bins(k, count_min)), _NP[_DT[dtype]])
        if n:
            self.oligo(bases if bases.size else np.zeros(1, np.uint8), offsets, n, k, out, count_min, norm,
                       total_step, dtype, KT_MEM_HOST)
        return out

    def oligo_tuning(self, mode):
        """False / 0: the launches that follow take no part in the k = 4 launch-shape measurement (a caller timing
        launches itself); True / 1: resume; n >= 2: as 0, with n workgroups per resident slot for every launch"""
        check(_lib.lib().kt_oligo_tuning(self._h, int(mode)))

    def oligo_launch_info(self):
        """-> dict: workgroups per resident slot of the k = 4 launches into the latest output array, whether that has
        been measured yet, and the measured ns per read of the candidates 32 / 96 / 200"""
        w, d, ns = C.c_uint32(), C.c_int(), (C.c_double * 3)()
        check(_lib.lib().kt_oligo_launch_info(self._h, C.byref(w), C.byref(d), ns))
        return {"wgs_per_slot": w.value, "measured": bool(d.value), "ns_per_read": {32: ns[0], 96: ns[1], 200: ns[2]}}

    def selftest_quotient(self, d_lo, d_hi):
        """-> (pairs checked, mismatches, checksum of the IEEE quotients' bits) for all 0 <= c <= d, d_lo <= d <= d_hi"""
        n, bad, chk = C.c_uint64(), C.c_uint64(), C.c_uint64()
        check(_lib.lib().kt_selftest_quotient(self._h, int(d_lo), int(d_hi), C.byref(n), C.byref(bad), C.byref(chk)))
        return n.value, bad.value, chk.value

    # -- comp cgr (whole sequence) ---------------------------------------------------------------
    def cgr(self, bases, offsets, n_reads, vecsize, xy, bad_pos=None, mem=KT_MEM_DEVICE):
        """xy: 2 f64 per base; bad_pos: u64 scalar (device pointer in device mode) or None"""
        check(_lib.lib().kt_cgr_points(self._h, _ptr(bases), _ptr(offsets), n_reads, float(vecsize), _ptr(xy),
                                       _ptr(bad_pos), mem))
        return xy

    def cgr_host(self, bases, offsets, vecsize=1):
        """-> (total_bases, 2) f64; raises KmertoolsError(KT_ERR_BADNT) on a byte outside ACGTUacgtu"""
        bases = np.ascontiguousarray(bases, np.uint8)
        offsets = np.ascontiguousarray(offsets, np.uint64)
        total = int(offsets[-1])
        xy = np.zeros((max(total, 1), 2), np.float64)
        self.cgr(bases if bases.size else np.zeros(1, np.uint8), offsets, len(offsets) - 1, vecsize, xy, None,
                 KT_MEM_HOST)
        return xy[:total]

    # -- min: window minimisers ---------------------------------------------------------------------
    def minimisers(self, bases, offsets, n_reads, wsize, msize, ev_offsets, kmers, starts, ends, capacity,
                   mem=KT_MEM_DEVICE):
        """-> number of (minimiser, start, end) triples; capacity 0 only counts (synchronises either way)"""
        n = C.c_uint64()
        check(_lib.lib().kt_minimisers(self._h, _ptr(bases), _ptr(offsets), n_reads, int(wsize), int(msize),
                                       _ptr(ev_offsets), _ptr(kmers), _ptr(starts), _ptr(ends), int(capacity),
                                       C.byref(n), mem))
        return n.value

    def minimisers_host(self, bases, offsets, wsize, msize):
        """-> (ev_offsets u64[n+1], kmers, starts, ends): read i owns [ev_offsets[i], ev_offsets[i+1])"""
        bases = np.ascontiguousarray(bases, np.uint8)
        offsets = np.ascontiguousarray(offsets, np.uint64)
        n = len(offsets) - 1
        evo = np.zeros(n + 1, np.uint64)
        bb = bases if bases.size else np.zeros(1, np.uint8)
        empty = np.zeros(1, np.uint64)
        cnt = self.minimisers(bb, offsets, n, wsize, msize, evo, empty, empty, empty, 0, KT_MEM_HOST) if n else 0
        k = np.zeros(max(cnt, 1), np.uint64)
        s = np.zeros(max(cnt, 1), np.uint64)
        e = np.zeros(max(cnt, 1), np.uint64)
        if cnt:
            self.minimisers(bb, offsets, n, wsize, msize, evo, k, s, e, cnt, KT_MEM_HOST)
        else:
            evo[:] = 0
        return evo, k[:cnt], s[:cnt], e[:cnt]

    # -- KmerGenerator surface -----------------------------------------------------------
    def kmers(self, bases, offsets, n_reads, k, fwd, rev, valid, mem=KT_MEM_DEVICE):
        check(_lib.lib().kt_kmers(self._h, _ptr(bases), _ptr(offsets), n_reads, k, _ptr(fwd), _ptr(rev),
                                  _ptr(valid), mem))

    def kmers_host(self, bases, offsets, k):
        """-> (fwd, rev, end_index) of every k-mer in positional order"""
        bases = np.ascontiguousarray(bases, np.uint8)
        offsets = np.ascontiguousarray(offsets, np.uint64)
        total = int(offsets[-1])
        fwd = np.zeros(max(total, 1), np.uint64)
        rev = np.zeros(max(total, 1), np.uint64)
        valid = np.zeros(max(total, 1), np.uint8)
        if total:
            self.kmers(bases, offsets, len(offsets) - 1, k, fwd, rev, valid, KT_MEM_HOST)
        idx = np.nonzero(valid[:total])[0]
        return fwd[idx], rev[idx], idx.astype(np.uint64)

    # -- ctr routing -------------------------------------------------------------------------
    def route(self, bases, offsets, n_reads, k, n_owners, keys_out, owner_counts, mem=KT_MEM_DEVICE):
        check(_lib.lib().kt_ctr_route(self._h, _ptr(bases), _ptr(offsets), n_reads, k, n_owners, _ptr(keys_out),
                                      _ptr(owner_counts), mem))

    def route_host(self, bases, offsets, k, n_owners):
        bases = np.ascontiguousarray(bases, np.uint8)
        offsets = np.ascontiguousarray(offsets, np.uint64)
        total = int(offsets[-1])
        keys = np.zeros(max(total, 1), np.uint64)
        counts = np.zeros(n_owners, np.uint64)
        self.route(bases if bases.size else np.zeros(1, np.uint8), offsets, len(offsets) - 1, k, n_owners, keys,
                   counts, KT_MEM_HOST)
        return keys[: int(counts.sum())], counts

    # -- synthetic reads (device only) ----------------------------------------------------------
    # -- profile: per-read statistics of a per-position count array (Counter.profile) ----------
    def profile_stats(self, profile, offsets, n_reads, n_kmers=None, n_present=None, min_count=None, median=None,
                      max_count=None, sum=None, mem=KT_MEM_DEVICE):
        """per read, over its entries of `profile` that are not 0xFFFFFFFF: how many, those >= 1, the least, element
        n // 2 of them sorted ascending, the greatest (u32 arrays of n_reads) and their sum (u64) - overwritten; any of
        them may be None (kt_profile_stats)"""
        check(_lib.lib().kt_profile_stats(self._h, _ptr(profile), _ptr(offsets), int(n_reads), _ptr(n_kmers),
                                          _ptr(n_present), _ptr(min_count), _ptr(median), _ptr(max_count), _ptr(sum), mem))

    def profile_stats_host(self, profile, offsets):
        """-> {"n_kmers", "n_present", "min", "median", "max": u32 arrays, "sum": u64 array}, one entry per read"""
        profile = np.ascontiguousarray(profile, np.uint32)
        offsets = np.ascontiguousarray(offsets, np.uint64)
        n = len(offsets) - 1
        out = {name: np.zeros(n, np.uint32) for name in ("n_kmers", "n_present", "min", "median", "max")}
        out["sum"] = np.zeros(n, np.uint64)
        if n:
            self.profile_stats(profile if profile.size else np.zeros(1, np.uint32), offsets, n, out["n_kmers"],
                               out["n_present"], out["min"], out["median"], out["max"], out["sum"], KT_MEM_HOST)
        return out

    # -- thread: hits (Counter.thread_hits) folded into runs along the unitigs -------------------
    def thread_runs(self, hits, read_offsets, n_reads, unitig_offsets, n_unitigs, k, run_start=None, run_len=None,
                    run_unitig=None, run_upos=None, run_offsets=None, max_runs=0, unitig_hits=None, unitig_runs=None,
                    tally=None, mem=KT_MEM_DEVICE):
        """maximal stretches of hits that step along one unitig in one orientation: per run its first read base (u64), its
        k-mers, 2 * unitig + antiparallel and the offset of its first k-mer in the unitig (u32 arrays of max_runs);
        run_offsets (u64, n_reads + 1) = the first run of every read; unitig_hits / unitig_runs (u64 per unitig) are added
        to by a call that writes runs; tally (u64[6], overwritten) = windows, hits, misses, bad values, runs, reads with a
        hit.  max_runs = 0 only counts.  Returns the number of runs; raises KmertoolsError (KT_ERR_ARG) when max_runs is
        too small (kt_thread_runs)."""
        n = C.c_uint64()
        check(_lib.lib().kt_thread_runs(self._h, _ptr(hits), _ptr(read_offsets), int(n_reads), _ptr(unitig_offsets),
                                        int(n_unitigs), int(k), _ptr(run_start), _ptr(run_len), _ptr(run_unitig),
                                        _ptr(run_upos), _ptr(run_offsets), int(max_runs), C.byref(n), _ptr(unitig_hits),
                                        _ptr(unitig_runs), _ptr(tally), mem))
        return n.value

    def thread_runs_host(self, hits, read_offsets, unitig_offsets, k, unitig_hits=None, unitig_runs=None):
        """-> {"run_start" u64, "run_len", "run_unitig", "run_upos" u32, "run_offsets" u64, "tally" u64[6]} of host arrays;
        unitig_hits / unitig_runs (u64 per unitig, or None) are added to.  A counting call, then one sized by it."""
        hits = np.ascontiguousarray(hits, np.uint32)
        read_offsets = np.ascontiguousarray(read_offsets, np.uint64)
        unitig_offsets = np.ascontiguousarray(unitig_offsets, np.uint64)
        n, nu = len(read_offsets) - 1, len(unitig_offsets) - 1
        out = {"run_offsets": np.zeros(n + 1, np.uint64), "tally": np.zeros(_lib.KT_THREAD_TALLY, np.uint64)}
        h = hits if hits.size else np.zeros(1, np.uint32)
        nr = self.thread_runs(h, read_offsets, n, unitig_offsets, nu, k, run_offsets=out["run_offsets"], tally=out["tally"],
                              mem=KT_MEM_HOST)
        out["run_start"] = np.zeros(nr, np.uint64)
        for name in ("run_len", "run_unitig", "run_upos"):
            out[name] = np.zeros(nr, np.uint32)
        if nr:
            self.thread_runs(h, read_offsets, n, unitig_offsets, nu, k, out["run_start"], out["run_len"], out["run_unitig"],
                             out["run_upos"], out["run_offsets"], nr, unitig_hits, unitig_runs, out["tally"], KT_MEM_HOST)
        return out

    # -- components: which unitigs hang together, and the reads split by them ------------------
    def unitig_components(self, link_offsets, link_to, n_unitigs, component, unitig_offsets=None, count_sums=None, k=1, stats=None,
                          max_components=0, tally=None, mem=KT_MEM_DEVICE):
        """the weakly connected components of the unitig graph from Counter.unitig_links' link arrays: component (u32 per
        unitig) = the component's number, components numbered by their smallest unitig; stats (u64, max_components x
        COMPONENT_FIELDS: COMPONENT_STATS_NAMES) and tally (u64[6]: components, components of one unitig, most unitigs, most
        nodes, bad links, rounds) are overwritten.  Returns the number of components; raises KmertoolsError (KT_ERR_ARG)
        when 0 < max_components < that number (kt_unitig_components)."""
        n = C.c_uint64()
        check(_lib.lib().kt_unitig_components(self._h, _ptr(link_offsets), _ptr(link_to), int(n_unitigs), _ptr(unitig_offsets),
                                              _ptr(count_sums), int(k), _ptr(component), _ptr(stats), int(max_components),
                                              C.byref(n), _ptr(tally), mem))
        return n.value

    def unitig_components_host(self, link_offsets, link_to, unitig_offsets=None, count_sums=None, k=None):
        """-> {"component" u32 per unitig, "stats" u64 (components x COMPONENT_FIELDS), "tally" u64[6]} of host arrays"""
        link_offsets = np.ascontiguousarray(link_offsets, np.uint64)
        link_to = np.ascontiguousarray(link_to, np.uint32)
        nu = (len(link_offsets) - 1) // 2
        if unitig_offsets is not None:
            unitig_offsets = np.ascontiguousarray(unitig_offsets, np.uint64)
        if count_sums is not None:
            count_sums = np.ascontiguousarray(count_sums, np.uint64)
        comp = np.zeros(nu, np.uint32)
        stats = np.zeros((nu, _lib.KT_COMPONENT_FIELDS), np.uint64)
        tally = np.zeros(_lib.KT_COMPONENT_TALLY, np.uint64)
        nc = self.unitig_components(link_offsets, link_to if link_to.size else np.zeros(1, np.uint32), nu, comp, unitig_offsets,
                                    count_sums, 1 if k is None else k, stats if nu else None, nu, tally, KT_MEM_HOST)
        return {"component": comp, "stats": stats[:nc].copy(), "tally": tally}

    def thread_read_components(self, run_unitig, run_len, run_offsets, n_reads, component, n_unitigs, n_components, read_component,
                               read_mixed=None, comp_reads=None, comp_hits=None, tally=None, mem=KT_MEM_DEVICE):
        """thread_runs' runs folded over unitig_components' component array: read_component (u32 per read) = the component of
        the read's first run (NO_COMPONENT: none), read_mixed (u8 per read, or None) = a later run lies in another one;
        comp_reads / comp_hits (u64 per component, or None) are added to; tally (u64[4], overwritten) = reads with a component,
        without, mixed reads, bad runs (kt_thread_read_components)"""
        check(_lib.lib().kt_thread_read_components(self._h, _ptr(run_unitig), _ptr(run_len), _ptr(run_offsets), int(n_reads),
                                                   _ptr(component), int(n_unitigs), int(n_components), _ptr(read_component),
                                                   _ptr(read_mixed), _ptr(comp_reads), _ptr(comp_hits), _ptr(tally), mem))

    def thread_read_components_host(self, run_unitig, run_len, run_offsets, component, n_components, comp_reads=None, comp_hits=None):
        """-> {"read_component" u32, "read_mixed" u8, "tally" u64[4]} of host arrays; comp_reads / comp_hits (u64 per
        component, or None) are added to"""
        run_unitig = np.ascontiguousarray(run_unitig, np.uint32)
        run_len = np.ascontiguousarray(run_len, np.uint32)
        run_offsets = np.ascontiguousarray(run_offsets, np.uint64)
        component = np.ascontiguousarray(component, np.uint32)
        n = len(run_offsets) - 1
        out = {"read_component": np.zeros(n, np.uint32), "read_mixed": np.zeros(n, np.uint8),
               "tally": np.zeros(_lib.KT_READ_COMPONENT_TALLY, np.uint64)}
        one = np.zeros(1, np.uint32)
        self.thread_read_components(run_unitig if run_unitig.size else one, run_len if run_len.size else one, run_offsets, n,
                                    component if component.size else one, len(component), n_components, out["read_component"],
                                    out["read_mixed"], comp_reads, comp_hits, out["tally"], KT_MEM_HOST)
        return out

    # -- correct: the decision over a support array (Counter.correct_support) ------------------
    def correct_apply(self, bases, offsets, n_reads, support, min_support=1, max_corrections=0, out_bases=None,
                      n_single=None, n_ambiguous=None, mem=KT_MEM_DEVICE):
        """a base is single when exactly one byte of its support entry is >= min_support, ambiguous when several are:
        n_single / n_ambiguous (u32 arrays of n_reads, overwritten) count them per read, out_bases gets "ACGT"[x] at the
        single bases of reads with at most max_corrections of them (0: no limit) and the input byte everywhere else; any
        of the three may be None, out_bases may be `bases` (kt_correct_apply)"""
        check(_lib.lib().kt_correct_apply(self._h, _ptr(bases), _ptr(offsets), int(n_reads), _ptr(support),
                                          int(min_support), int(max_corrections), _ptr(out_bases), _ptr(n_single),
                                          _ptr(n_ambiguous), mem))
        return out_bases, n_single, n_ambiguous

    # -- sketch: bottom-s MinHash sketches, their unions, all-pairs merge walks -----------------
    def sketch(self, bases, offsets, n_reads, k, s, hashes, sizes, n_kmers=None, seed=0, mem=KT_MEM_DEVICE):
        """row i of hashes (u64, n_reads x s) = the s smallest distinct mix64(canonical k-mer ^ seed) of read i, ascending,
        KT_EMPTY_KEY behind sizes[i] (u32) of them; n_kmers (u32, may be None) = the read's windows (kt_sketch_batch)"""
        check(_lib.lib().kt_sketch_batch(self._h, _ptr(bases), _ptr(offsets), int(n_reads), int(k), int(s), int(seed),
                                         _ptr(hashes), _ptr(sizes), _ptr(n_kmers), mem))

    def sketch_host(self, bases, offsets, k, s, seed=0):
        """-> (hashes u64[n, s], sizes u32[n], n_kmers u32[n])"""
        bases = np.ascontiguousarray(bases, np.uint8)
        offsets = np.ascontiguousarray(offsets, np.uint64)
        n = len(offsets) - 1
        hashes = np.zeros((n, int(s)), np.uint64)
        sizes, n_kmers = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
        if n:
            self.sketch(bases if bases.size else np.zeros(1, np.uint8), offsets, n, k, s, hashes, sizes, n_kmers, seed,
                        KT_MEM_HOST)
        return hashes, sizes, n_kmers

    def sketch_merge(self, hashes, sizes, group_offsets, out_hashes=None, out_sizes=None, s=None, mem=KT_MEM_HOST):
        """row g of the result = the bottom-s of the union of rows group_offsets[g] .. group_offsets[g+1] of hashes
        (kt_sketch_merge).  Host arrays: -> (out_hashes u64[n_groups, s], out_sizes u32[n_groups]); device tensors
        (mem=KT_MEM_DEVICE): out_hashes, out_sizes and s are given, n and n_groups are taken from sizes / group_offsets."""
        if mem == KT_MEM_HOST:
            hashes = np.ascontiguousarray(hashes, np.uint64)
            sizes = np.ascontiguousarray(sizes, np.uint32)
            group_offsets = np.ascontiguousarray(group_offsets, np.uint64)
            s = int(hashes.shape[1]) if s is None else int(s)
            n_groups = len(group_offsets) - 1
            out_hashes, out_sizes = np.zeros((n_groups, s), np.uint64), np.zeros(n_groups, np.uint32)
        else:
            n_groups = len(group_offsets) - 1
        check(_lib.lib().kt_sketch_merge(self._h, _ptr(hashes), _ptr(sizes), len(sizes), int(s), _ptr(group_offsets),
                                         n_groups, _ptr(out_hashes), _ptr(out_sizes), mem))
        return out_hashes, out_sizes

    def sketch_pairs(self, a_hashes, a_sizes, n_a, b_hashes, b_sizes, n_b, s, shared, denom=None, mem=KT_MEM_DEVICE):
        """shared / denom (u32, n_a x n_b, denom may be None): Mash's merge walk of every (row of a, row of b)
        (kt_sketch_pairs); b may be a itself"""
        check(_lib.lib().kt_sketch_pairs(self._h, _ptr(a_hashes), _ptr(a_sizes), int(n_a), _ptr(b_hashes), _ptr(b_sizes),
                                         int(n_b), int(s), _ptr(shared), _ptr(denom), mem))

    def sketch_pairs_host(self, a_hashes, a_sizes, b_hashes=None, b_sizes=None):
        """-> (shared u32[n_a, n_b], denom u32[n_a, n_b]); without b: a against itself"""
        a_hashes = np.ascontiguousarray(a_hashes, np.uint64)
        a_sizes = np.ascontiguousarray(a_sizes, np.uint32)
        if b_hashes is None:
            b_hashes, b_sizes = a_hashes, a_sizes
        else:
            b_hashes = np.ascontiguousarray(b_hashes, np.uint64)
            b_sizes = np.ascontiguousarray(b_sizes, np.uint32)
        s = int(a_hashes.shape[1])
        assert b_hashes.shape[1] == s
        shared = np.zeros((len(a_sizes), len(b_sizes)), np.uint32)
        denom = np.zeros_like(shared)
        self.sketch_pairs(a_hashes, a_sizes, len(a_sizes), b_hashes, b_sizes, len(b_sizes), s, shared, denom, KT_MEM_HOST)
        return shared, denom

    # -- scaled (FracMinHash) sketches: CSR rows of (hash, abundance), their unions, shared hashes of pairs ------
    def scaled_sketch(self, bases, offsets, n_reads, k, scaled, hashes, abunds, max_out, row_offsets, n_kmers=None, seed=0,
                      mem=KT_MEM_DEVICE):
        """row i of (hashes u64, abunds u32 or None) = the distinct mix64(canonical k-mer ^ seed) <= scaled_max_hash(scaled)
        of read i, ascending, with their multiplicities; row_offsets u64[n_reads + 1]; n_kmers (u32, may be None) = the
        reads' windows.  Returns the number of hashes; max_out 0 only counts (hashes may be None), a smaller max_out than
        the result raises KmertoolsError (kt_scaled_batch)"""
        n = C.c_uint64()
        check(_lib.lib().kt_scaled_batch(self._h, _ptr(bases), _ptr(offsets), int(n_reads), int(k), int(scaled), int(seed),
                                         _ptr(hashes), _ptr(abunds), int(max_out), _ptr(row_offsets), _ptr(n_kmers), C.byref(n), mem))
        return n.value

    def scaled_sketch_host(self, bases, offsets, k, scaled, seed=0):
        """-> (hashes u64[n_out], abunds u32[n_out], row_offsets u64[n + 1], n_kmers u32[n]): a count-only call, then one
        call sized by it"""
        bases = np.ascontiguousarray(bases, np.uint8)
        offsets = np.ascontiguousarray(offsets, np.uint64)
        n = len(offsets) - 1
        row_offsets, n_kmers = np.zeros(n + 1, np.uint64), np.zeros(n, np.uint32)
        if not n:
            return np.zeros(0, np.uint64), np.zeros(0, np.uint32), row_offsets, n_kmers
        b = bases if bases.size else np.zeros(1, np.uint8)
        n_out = self.scaled_sketch(b, offsets, n, k, scaled, None, None, 0, row_offsets, None, seed, KT_MEM_HOST)
        hashes, abunds = np.zeros(n_out, np.uint64), np.zeros(n_out, np.uint32)
        if n_out:
            self.scaled_sketch(b, offsets, n, k, scaled, hashes, abunds, n_out, row_offsets, n_kmers, seed, KT_MEM_HOST)
        else:
            self.scaled_sketch(b, offsets, n, k, scaled, None, None, 0, row_offsets, n_kmers, seed, KT_MEM_HOST)
        return hashes, abunds, row_offsets, n_kmers

    def scaled_merge(self, hashes, abunds, row_offsets, group_offsets, out_hashes=None, out_abunds=None, max_out=0,
                     out_offsets=None, mem=KT_MEM_HOST):
        """row g of the result = the union of rows group_offsets[g] .. group_offsets[g+1], abundances (None: 1 each) summed
        and saturating (kt_scaled_merge).  Host arrays: -> (out_hashes, out_abunds, out_offsets), sized by a count-only
        call.  Device tensors (mem=KT_MEM_DEVICE): the outputs and max_out are given, the number of hashes is returned."""
        n_rows, n_groups = len(row_offsets) - 1, len(group_offsets) - 1
        n = C.c_uint64()

        def call(oh, oa, room, oo):
            check(_lib.lib().kt_scaled_merge(self._h, _ptr(hashes), _ptr(abunds), _ptr(row_offsets), n_rows, _ptr(group_offsets),
                                             n_groups, _ptr(oh), _ptr(oa), int(room), _ptr(oo), C.byref(n), mem))
            return n.value

        if mem != KT_MEM_HOST:
            return call(out_hashes, out_abunds, max_out, out_offsets)
        hashes = np.ascontiguousarray(hashes, np.uint64)
        abunds = None if abunds is None else np.ascontiguousarray(abunds, np.uint32)
        row_offsets = np.ascontiguousarray(row_offsets, np.uint64)
        group_offsets = np.ascontiguousarray(group_offsets, np.uint64)
        out_offsets = np.zeros(n_groups + 1, np.uint64)
        n_out = call(None, None, 0, out_offsets) if n_groups else 0
        out_hashes, out_abunds = np.zeros(n_out, np.uint64), np.zeros(n_out, np.uint32)
        if n_out:
            call(out_hashes, out_abunds, n_out, out_offsets)
        return out_hashes, out_abunds, out_offsets

    def scaled_pairs(self, a_hashes, a_offsets, n_a, b_hashes, b_offsets, n_b, shared, mem=KT_MEM_DEVICE):
        """shared (u32, n_a x n_b) = the hashes every (row of a, row of b) has in common (kt_scaled_pairs); b may be a itself"""
        check(_lib.lib().kt_scaled_pairs(self._h, _ptr(a_hashes), _ptr(a_offsets), int(n_a), _ptr(b_hashes), _ptr(b_offsets),
                                         int(n_b), _ptr(shared), mem))

    def scaled_pairs_host(self, a_hashes, a_offsets, b_hashes=None, b_offsets=None):
        """-> shared u32[n_a, n_b]; without b: a against itself"""
        a_hashes = np.ascontiguousarray(a_hashes, np.uint64)
        a_offsets = np.ascontiguousarray(a_offsets, np.uint64)
        if b_hashes is None:
            b_hashes, b_offsets = a_hashes, a_offsets
        else:
            b_hashes = np.ascontiguousarray(b_hashes, np.uint64)
            b_offsets = np.ascontiguousarray(b_offsets, np.uint64)
        shared = np.zeros((len(a_offsets) - 1, len(b_offsets) - 1), np.uint32)
        self.scaled_pairs(a_hashes, a_offsets, len(a_offsets) - 1, b_hashes, b_offsets, len(b_offsets) - 1, shared, KT_MEM_HOST)
        return shared

    # -- card: HyperLogLog registers of the distinct canonical k-mers ----------------------------
    def card_add(self, bases, offsets, n_reads, k, registers, p=14, seed=0, n_kmers=None, mem=KT_MEM_DEVICE):
        """registers (u8, 2^p, zeroed once by the caller) are raised by the k-mers of the batch: register
        mix64(canonical k-mer ^ seed) >> (64 - p) to 1 + the leading zeros of the hash's low 64 - p bits; n_kmers (one u64,
        may be None) += the windows (kt_card_add_reads)"""
        check(_lib.lib().kt_card_add_reads(self._h, _ptr(bases), _ptr(offsets), int(n_reads), int(k), int(p), int(seed),
                                           _ptr(registers), _ptr(n_kmers), mem))

    def card_host(self, bases, offsets, k, p=14, seed=0):
        """-> (registers u8[2^p], n_kmers) of a host batch"""
        bases = np.ascontiguousarray(bases, np.uint8)
        offsets = np.ascontiguousarray(offsets, np.uint64)
        n = len(offsets) - 1
        registers, n_kmers = np.zeros(1 << int(p), np.uint8), np.zeros(1, np.uint64)
        self.card_add(bases if bases.size else np.zeros(1, np.uint8), offsets, n, k, registers, p, seed, n_kmers, KT_MEM_HOST)
        return registers, int(n_kmers[0])

    def synth_reads(self, seed, n_reads, read_len, bases_dev, offsets_dev=None, noise=False, genome_len=0,
                    first_read=0):
        check(_lib.lib().kt_synth_reads(self._h, seed, first_read, n_reads, read_len, int(bool(noise)),
                                        genome_len, _ptr(bases_dev), _ptr(offsets_dev)))


class Prefilter:
    """The two-pass pre-filter (kt_prefilter): 2^log2_once words of `once` bits and 2^log2_twice words of `twice` bits in
    HBM.  add_reads over an input is pass 1; Counter.add_reads_filtered over the same input is pass 2 and leaves the k-mers
    seen once out of the table, up to the filter's false positives."""

    def __init__(self, ctx, k, log2_once, log2_twice, seed=0):
        self.ctx = ctx
        self.k, self.log2_once, self.log2_twice, self.seed = k, int(log2_once), int(log2_twice), int(seed)
        self._h = C.c_void_p()
        check(_lib.lib().kt_prefilter_create(ctx._h, k, self.log2_once, self.log2_twice, self.seed, C.byref(self._h)))

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            if self.ctx._h.value:   # (as for a Counter: destroying waits for the context's stream)
                _lib.lib().kt_prefilter_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def clear(self):
        check(_lib.lib().kt_prefilter_clear(self._h))

    def add_reads(self, bases, offsets, n_reads, mem=KT_MEM_DEVICE):
        check(_lib.lib().kt_prefilter_add_reads(self._h, _ptr(bases), _ptr(offsets), n_reads, mem))

    def add_reads_host(self, bases, offsets):
        bases = np.ascontiguousarray(bases, np.uint8)
        offsets = np.ascontiguousarray(offsets, np.uint64)
        self.add_reads(bases if bases.size else np.zeros(1, np.uint8), offsets, len(offsets) - 1, KT_MEM_HOST)

    def stats(self):
        """-> dict(windows, promotions, once_bits_set, twice_bits_set) (kt_prefilter_stats; synchronises)"""
        v = [C.c_uint64() for _ in range(4)]
        check(_lib.lib().kt_prefilter_stats(self._h, *[C.byref(x) for x in v]))
        return dict(zip(("windows", "promotions", "once_bits_set", "twice_bits_set"), (x.value for x in v)))

    def query(self, keys, n, out, mem=KT_MEM_DEVICE):
        """out[i] (u8) = 1 if `once` covers the pattern of canonical k-mer keys[i], | 2 if `twice` does (kt_prefilter_query)"""
        check(_lib.lib().kt_prefilter_query(self._h, _ptr(keys), int(n), _ptr(out), mem))
        return out

    def query_host(self, keys):
        keys = np.ascontiguousarray(keys, np.uint64)
        out = np.zeros(len(keys), np.uint8)
        if len(keys):
            self.query(keys, len(keys), out, KT_MEM_HOST)
        return out


class _FilteredAdds:
    """Pass 2 of the two-pass count, as methods of Counter.  A base class of their own: tests/test_grid_limits.py keeps a
    table of cases for the methods defined on Context and Counter themselves, and the case of these two - pass 1 and pass 2
    with the grid held to 8 workgroups - stands with the filter's other tests in tests/test_prefilter.py."""

    def add_reads_filtered(self, prefilter, bases, offsets, n_reads, n_parts=1, part=0, mem=KT_MEM_DEVICE):
        """add_reads_part for the k-mers whose pattern is covered in the `twice` array of `prefilter` (a Prefilter that has
        seen the input): pass 2 of the two-pass count, always by probing (kt_ctr_add_reads_filtered)"""
        check(_lib.lib().kt_ctr_add_reads_filtered(self._h, prefilter._h, _ptr(bases), _ptr(offsets), n_reads, mem, n_parts, part))

    def add_reads_filtered_host(self, prefilter, bases, offsets, n_parts=1, part=0):
        bases = np.ascontiguousarray(bases, np.uint8)
        offsets = np.ascontiguousarray(offsets, np.uint64)
        self.add_reads_filtered(prefilter, bases if bases.size else np.zeros(1, np.uint8), offsets, len(offsets) - 1, n_parts, part,
                                KT_MEM_HOST)


class Counter(_FilteredAdds):
    """HBM-resident canonical k-mer table (kt_ctr) = the reference's CountComputer state."""

    def __init__(self, ctx, k, capacity_slots):
        self.ctx = ctx
        self.k = k
        self._h = C.c_void_p()
        check(_lib.lib().kt_ctr_create(ctx._h, k, int(capacity_slots), C.byref(self._h)))

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            if self.ctx._h.value:   # (a table that outlives its context is not destroyed: kt_ctr_destroy waits for the context's stream)
                _lib.lib().kt_ctr_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def clear(self):
        check(_lib.lib().kt_ctr_clear(self._h))

    def add_reads(self, bases, offsets, n_reads, mem=KT_MEM_DEVICE):
        check(_lib.lib().kt_ctr_add_reads(self._h, _ptr(bases), _ptr(offsets), n_reads, mem))

    def add_reads_host(self, bases, offsets, n_parts=1, part=0):
        bases = np.ascontiguousarray(bases, np.uint8)
        offsets = np.ascontiguousarray(offsets, np.uint64)
        self.add_reads_part(bases if bases.size else np.zeros(1, np.uint8), offsets, len(offsets) - 1, n_parts, part,
                            KT_MEM_HOST)

    def add_reads_part(self, bases, offsets, n_reads, n_parts, part, mem=KT_MEM_DEVICE):
        """only the k-mers of hash partition `part` of `n_parts` (out-of-core passes)"""
        check(_lib.lib().kt_ctr_add_reads_part(self._h, _ptr(bases), _ptr(offsets), n_reads, mem, n_parts, part))

    def add_pairs(self, keys, counts, n, mem=KT_MEM_DEVICE):
        check(_lib.lib().kt_ctr_add_pairs(self._h, _ptr(keys), _ptr(counts), n, mem))

    def add_pairs_host(self, keys, counts=None):
        keys = np.ascontiguousarray(keys, np.uint64)
        if counts is not None:
            counts = np.ascontiguousarray(counts, np.uint32)
        if len(keys):
            self.add_pairs(keys, counts, len(keys), KT_MEM_HOST)

    def erase(self, keys):
        """removes the canonical k-mers `keys` (host u64) from the table in place; returns how many entries went
        (kt_ctr_erase: absent keys, duplicates, KT_EMPTY_KEY and values >= 4^k are ignored)"""
        keys = np.ascontiguousarray(keys, np.uint64)
        return self.erase_device(keys, len(keys), KT_MEM_HOST)

    def erase_device(self, keys, n, mem=KT_MEM_DEVICE):
        """erase() with the n keys in a device tensor (u64 bit patterns)"""
        gone = C.c_uint64()
        check(_lib.lib().kt_ctr_erase(self._h, _ptr(keys) if n else None, int(n), C.byref(gone), mem))
        return gone.value

    def size(self):
        n = C.c_uint64()
        check(_lib.lib().kt_ctr_size(self._h, C.byref(n)))
        return n.value

    def capacity(self):
        """slots the table really has (the request rounded up to 5..8 eighths of a power of two)"""
        n = C.c_uint64()
        check(_lib.lib().kt_ctr_capacity(self._h, C.byref(n)))
        return n.value

    def export(self, keys, counts, max_out, mem=KT_MEM_DEVICE):
        n = C.c_uint64()
        check(_lib.lib().kt_ctr_export(self._h, _ptr(keys), _ptr(counts), max_out, C.byref(n), mem))
        return n.value

    def export_target(self, keys, counts, max_out):
        """device arrays that the next whole-batch count into the empty table writes its (key, count) pairs to
        (sticky; None, None switches it off): export(keys, counts, ...) afterwards copies nothing.  The library keeps the
        raw pointers until the target is switched off or the counter closed, so the tensors are kept alive here."""
        check(_lib.lib().kt_ctr_export_target(self._h, _ptr(keys), _ptr(counts), int(max_out) if keys is not None else 0))
        self._xt = (keys, counts) if keys is not None else None

    # -- cov: per-read coverage histograms against this table ---------------------------------
    def cov(self, bases, offsets, n_reads, bin_size, bin_count, out, norm=True, dtype="f64", mem=KT_MEM_DEVICE):
        check(_lib.lib().kt_cov_batch(self._h, _ptr(bases), _ptr(offsets), n_reads, int(bin_size), int(bin_count),
                                      int(bool(norm)), _DT[dtype], _ptr(out), mem))
        return out

    def lookup(self, keys, n, counts, mem=KT_MEM_DEVICE):
        """counts[i] = occurrences of the canonical k-mer keys[i] (0: absent) - u64 keys, u32 counts"""
        check(_lib.lib().kt_ctr_lookup(self._h, _ptr(keys), int(n), _ptr(counts), mem))
        return counts

    def lookup_host(self, keys):
        keys = np.ascontiguousarray(keys, np.uint64)
        out = np.zeros(len(keys), np.uint32)
        if len(keys):
            self.lookup(keys, len(keys), out, KT_MEM_HOST)
        return out

    def cov_part(self, bases, offsets, n_reads, bin_size, bin_count, counts, n_parts=1, part=0, mem=KT_MEM_DEVICE):
        """adds the u32 bin counts of the k-mers this table answers for (hash partition `part` of n_parts; a shard: the
        k-mers it owns) to `counts` (n_reads x bin_count)"""
        check(_lib.lib().kt_cov_batch_part(self._h, _ptr(bases), _ptr(offsets), n_reads, int(bin_size), int(bin_count),
                                           _ptr(counts), mem, int(n_parts), int(part)))
        return counts

    def cov_host(self, bases, offsets, bin_size, bin_count, norm=True, dtype="f64"):
        bases = np.ascontiguousarray(bases, np.uint8)
        offsets = np.ascontiguousarray(offsets, np.uint64)
        n = len(offsets) - 1
        out = np.zeros((n, int(bin_count)), _NP[_DT[dtype]])
        if n:
            self.cov(bases if bases.size else np.zeros(1, np.uint8), offsets, n, bin_size, bin_count, out, norm,
                     dtype, KT_MEM_HOST)
        return out

    # -- filter: per-read k-mer solidity against this table ------------------------------------
    def read_solidity(self, bases, offsets, n_reads, min_count, max_count, n_kmers, n_solid, first_weak=None,
                      mem=KT_MEM_DEVICE, n_parts=1, part=0):
        """combines into n_kmers (+), n_solid (+) and first_weak (min; may be None) the reads' k-mers of hash partition
        `part` of n_parts, those with min_count <= count <= max_count and the start of the first other one - u32 arrays
        of n_reads, initialised by the caller to 0 / 0 / 0xFFFFFFFF (kt_ctr_read_solidity)"""
        check(_lib.lib().kt_ctr_read_solidity(self._h, _ptr(bases), _ptr(offsets), int(n_reads), int(min_count),
                                              int(max_count), _ptr(n_kmers), _ptr(n_solid), _ptr(first_weak), mem,
                                              int(n_parts), int(part)))
        return n_kmers, n_solid, first_weak

    def read_solidity_host(self, bases, offsets, min_count=2, max_count=None):
        """-> (n_kmers, n_solid, first_weak) u32 arrays of the whole table (first_weak 0xFFFFFFFF: no weak k-mer)"""
        bases = np.ascontiguousarray(bases, np.uint8)
        offsets = np.ascontiguousarray(offsets, np.uint64)
        n = len(offsets) - 1
        nk = np.zeros(n, np.uint32)
        ns = np.zeros(n, np.uint32)
        fw = np.full(n, 0xFFFFFFFF, np.uint32)
        hi = 0xFFFFFFFF if max_count is None else int(max_count)
        if n:
            self.read_solidity(bases if bases.size else np.zeros(1, np.uint8), offsets, n, min_count, hi, nk, ns, fw,
                               KT_MEM_HOST)
        return nk, ns, fw

    # -- profile: the count of the k-mer that starts at every base --------------------------------
    def profile(self, bases, offsets, n_reads, profile, mem=KT_MEM_DEVICE, n_parts=1, part=0):
        """writes min(count, 0xFFFFFFFE) of every valid window of hash partition `part` of n_parts into profile[global
        base index of its start] - a u32 array of offsets[n_reads] entries that the caller filled with NO_KMER; every
        other entry is left as it is (kt_ctr_profile)"""
        check(_lib.lib().kt_ctr_profile(self._h, _ptr(bases), _ptr(offsets), int(n_reads), _ptr(profile), mem,
                                        int(n_parts), int(part)))
        return profile

    def profile_host(self, bases, offsets):
        """-> u32 array, one entry per base: the whole table's count of the k-mer that starts there, NO_KMER where none does"""
        bases = np.ascontiguousarray(bases, np.uint8)
        offsets = np.ascontiguousarray(offsets, np.uint64)
        n = len(offsets) - 1
        prof = np.full(int(offsets[-1]) if n > 0 else 0, NO_KMER, np.uint32)
        if n > 0 and prof.size:
            self.profile(bases, offsets, n, prof, KT_MEM_HOST)
        return prof

    # -- thread: this table as a k-mer -> position index of a set of sequences (the unitigs) ------
    def index_sequences(self, bases, offsets, n_seqs, mem=KT_MEM_DEVICE):
        """fills this EMPTY table with (canonical k-mer, 1 + 2 * global base of the window + (the sequence shows its reverse
        complement)) for every window of the sequences; returns the number of windows.  Raises KmertoolsError (KT_ERR_ARG)
        when a k-mer occurs twice (the table is cleared) or the sequences hold more than 2^31 - 2 bases
        (kt_ctr_index_sequences)"""
        n = C.c_uint64()
        check(_lib.lib().kt_ctr_index_sequences(self._h, _ptr(bases), _ptr(offsets), int(n_seqs), C.byref(n), mem))
        return n.value

    def index_sequences_host(self, bases, offsets):
        bases = np.ascontiguousarray(bases, np.uint8)
        offsets = np.ascontiguousarray(offsets, np.uint64)
        return self.index_sequences(bases if bases.size else np.zeros(1, np.uint8), offsets, len(offsets) - 1, KT_MEM_HOST)

    def thread_hits(self, bases, offsets, n_reads, hits, mem=KT_MEM_DEVICE):
        """writes, for every valid window, 0 when its k-mer is not in this index and otherwise 1 + 2 * G + a - G: where the
        k-mer lies in the indexed sequences, a = 1: the read runs antiparallel to them there - into hits[global base index
        of its start], a u32 array of offsets[n_reads] entries that the caller filled with NO_KMER (kt_ctr_thread_hits)"""
        check(_lib.lib().kt_ctr_thread_hits(self._h, _ptr(bases), _ptr(offsets), int(n_reads), _ptr(hits), mem))
        return hits

    def thread_hits_host(self, bases, offsets):
        """-> u32 array, one entry per base (NO_KMER where no k-mer starts)"""
        bases = np.ascontiguousarray(bases, np.uint8)
        offsets = np.ascontiguousarray(offsets, np.uint64)
        n = len(offsets) - 1
        hits = np.full(int(offsets[-1]) if n > 0 else 0, NO_KMER, np.uint32)
        if n > 0 and hits.size:
            self.thread_hits(bases, offsets, n, hits, KT_MEM_HOST)
        return hits

    # -- correct: repair read errors from the solid k-mers of this table ---------------------------
    def correct_support(self, bases, offsets, n_reads, profile, min_count, max_count, support, mem=KT_MEM_DEVICE,
                        n_parts=1, part=0):
        """for every base that no solid window of `profile` (the complete Counter.profile of the batch) covers, adds to
        byte x of support[base] the windows in which nucleotide x there makes a solid k-mer of hash partition `part` of
        n_parts - a u32 array of offsets[n_reads] entries that the caller zeroed (kt_ctr_correct_support)"""
        check(_lib.lib().kt_ctr_correct_support(self._h, _ptr(bases), _ptr(offsets), int(n_reads), _ptr(profile),
                                                int(min_count), int(max_count), _ptr(support), mem, int(n_parts),
                                                int(part)))
        return support

    def correct_host(self, bases, offsets, min_count=2, max_count=None, min_support=1, max_corrections=0):
        """-> (out_bases u8, n_single u32, n_ambiguous u32): the batch with its repairable bases rewritten, and per read
        how many bases were repairable / had several supported candidates (profile, support and apply for this table)"""
        bases = np.ascontiguousarray(bases, np.uint8)
        offsets = np.ascontiguousarray(offsets, np.uint64)
        n = len(offsets) - 1
        out = bases.copy()
        ns = np.zeros(max(n, 0), np.uint32)
        na = np.zeros(max(n, 0), np.uint32)
        if n > 0 and bases.size:
            hi = 0xFFFFFFFF if max_count is None else int(max_count)
            prof = self.profile_host(bases, offsets)
            sup = np.zeros(bases.size, np.uint32)
            self.correct_support(bases, offsets, n, prof, min_count, hi, sup, KT_MEM_HOST)
            self.ctx.correct_apply(bases, offsets, n, sup, min_support, max_corrections, out, ns, na, KT_MEM_HOST)
        return out, ns, na

    def spectrum(self, n_bins=10001, totals=False):
        """The table's abundance spectrum (jellyfish histo): hist[c] = distinct k-mers with exactly c occurrences for
        1 <= c < n_bins - 1, hist[n_bins - 1] = those with n_bins - 1 or more, hist[0] = 0.  totals=True: also
        (distinct k-mers, occurrences), exact whatever n_bins."""
        hist = np.zeros(int(n_bins), np.uint64)
        tot = np.zeros(2, np.uint64)
        check(_lib.lib().kt_ctr_spectrum(self._h, _ptr(hist), int(n_bins), _ptr(tot) if totals else None, KT_MEM_HOST))
        return (hist, (int(tot[0]), int(tot[1]))) if totals else hist

    def spectrum_into(self, hist, n_bins, totals=None, mem=KT_MEM_DEVICE):
        """adds the spectrum into `hist` (n_bins u64) and (distinct, occurrences) into `totals` (2 u64, or None)"""
        check(_lib.lib().kt_ctr_spectrum(self._h, _ptr(hist), int(n_bins), _ptr(totals), mem))
        return hist

    def scaled_sketch(self, scaled, min_count=1, max_count=None, seed=0, hashes=None, abunds=None, max_out=0, totals=None,
                      mem=KT_MEM_HOST):
        """The scaled sketch of the table's k-mers with min_count <= count <= max_count, the counts as abundances
        (kt_ctr_scaled; the table is walked in the form it is in and left as it is).  Host (the default): -> (hashes u64,
        abunds u32, (entries in the count range, their occurrences)), sized by a count-only call.  mem=KT_MEM_DEVICE:
        hashes / abunds tensors of max_out (None, 0 only counts) and totals (2 u64 or None) are given; returns the number
        of hashes."""
        hi = 0xFFFFFFFF if max_count is None else int(max_count)
        n = C.c_uint64()

        def call(h, a, room, t):
            check(_lib.lib().kt_ctr_scaled(self._h, int(min_count), hi, int(scaled), int(seed), _ptr(h), _ptr(a), int(room), C.byref(n),
                                           _ptr(t), mem))
            return n.value

        if mem != KT_MEM_HOST:
            return call(hashes, abunds, max_out, totals)
        tot = np.zeros(2, np.uint64)
        n_out = call(None, None, 0, tot)
        hashes, abunds = np.zeros(n_out, np.uint64), np.zeros(n_out, np.uint32)
        if n_out:
            call(hashes, abunds, n_out, tot)
        return hashes, abunds, (int(tot[0]), int(tot[1]))

    COMPARE_TOTALS = ("distinct_a", "distinct_b", "shared", "occurrences_a", "occurrences_b", "shared_min")

    def compare(self, other, n_rows=1001, n_cols=101, totals=False):
        """The comparison matrix of this table (rows) and `other` (columns), same k (KAT comp / spectra-cn): m[r, c] =
        distinct k-mers with min(count here, n_rows - 1) == r and min(count in other, n_cols - 1) == c, a count of 0 for
        an absent k-mer; m[0, 0] = 0.  totals=True: also a dict of the exact distinct_a, distinct_b, shared,
        occurrences_a, occurrences_b and shared_min (kt_ctr_compare)."""
        m = np.zeros((int(n_rows), int(n_cols)), np.uint64)
        tot = np.zeros(6, np.uint64)
        self.compare_into(other, m, n_rows, n_cols, tot if totals else None, KT_MEM_HOST)
        return (m, dict(zip(self.COMPARE_TOTALS, (int(v) for v in tot)))) if totals else m

    def compare_into(self, other, matrix, n_rows, n_cols, totals=None, mem=KT_MEM_DEVICE):
        """adds the comparison matrix into `matrix` (n_rows x n_cols u64) and the six totals into `totals` (6 u64, or
        None)"""
        check(_lib.lib().kt_ctr_compare(self._h, other._h, _ptr(matrix), int(n_rows), int(n_cols), _ptr(totals), mem))
        return matrix

    SET_OPS = {"intersect": 0, "subtract": 1, "union": 2, "xor": 3}
    SET_COUNTS = {"first": 0, "min": 1, "max": 2, "sum": 3}

    @classmethod
    def _setop_args(cls, op, count, a_range, b_range):
        """the strings and ranges of setop / setop_device as kt_ctr_setop's integers (ValueError before any library call)"""
        if op not in cls.SET_OPS:
            raise ValueError("setop: unknown op %r (one of %s)" % (op, ", ".join(cls.SET_OPS)))
        if count not in cls.SET_COUNTS:
            raise ValueError("setop: unknown count rule %r (one of %s)" % (count, ", ".join(cls.SET_COUNTS)))
        lo_a, hi_a = a_range
        lo_b, hi_b = b_range
        return (cls.SET_OPS[op], cls.SET_COUNTS[count], int(lo_a), 0xFFFFFFFF if hi_a is None else int(hi_a), int(lo_b),
                0xFFFFFFFF if hi_b is None else int(hi_b))

    def setop(self, other, op, count="first", a_range=(1, None), b_range=(1, None), sort=True):
        """The k-mers of this table (A) and `other` (B), same k, for which `op` holds - "intersect" (in A and in B),
        "subtract" (in A, not in B), "union", "xor" - as (keys u64, counts u32) numpy arrays, ascending by key with sort.
        A k-mer is in a table when its count there lies in that table's (min, max) range (None: no upper bound); a count
        outside the range is taken as 0.  `count`: "first" (A's, else B's), "min" / "max" of the non-zero ones, "sum"
        (saturating).  A count-only call, then one call sized by it (kt_ctr_setop)."""
        args = self._setop_args(op, count, a_range, b_range)
        n = C.c_uint64()
        check(_lib.lib().kt_ctr_setop(self._h, other._h, *args, None, None, 0, C.byref(n), KT_MEM_HOST, 0))
        keys = np.zeros(n.value, np.uint64)
        counts = np.zeros(n.value, np.uint32)
        if n.value:
            check(_lib.lib().kt_ctr_setop(self._h, other._h, *args, _ptr(keys), _ptr(counts), n.value, C.byref(n),
                                          KT_MEM_HOST, int(bool(sort))))
        return keys, counts

    def setop_device(self, other, op, keys, counts, max_out, count="first", a_range=(1, None), b_range=(1, None), sort=True):
        """setop into device tensors of max_out entries (keys u64 / counts u32 bit patterns; None, None, 0 only counts);
        returns the number of entries that qualify.  Raises KmertoolsError (KT_ERR_ARG) when 0 < max_out < that number."""
        args = self._setop_args(op, count, a_range, b_range)
        n = C.c_uint64()
        check(_lib.lib().kt_ctr_setop(self._h, other._h, *args, _ptr(keys), _ptr(counts), int(max_out), C.byref(n),
                                      KT_MEM_DEVICE, int(bool(sort))))
        return n.value

    def graph(self, min_count=1, max_count=None, sort=True, census=False):
        """The de Bruijn adjacency of the table's k-mers with min_count <= count <= max_count (the nodes; None: no upper
        bound) as numpy (keys u64, info u32, counts u32), ascending by key with sort.  info: bit x = right neighbour
        F[1..k) + "ACGT"[x] is a node, bit 4 + x = left neighbour "ACGT"[x] + F[0..k-1) is one, bit 8 / 9 = a unitig ends
        at the right / left side (F: the canonical k-mer itself).  census=True: also the KT_GRAPH_CENSUS u64 cells named
        by GRAPH_CENSUS_NAMES.  A count-only call, then one call sized by it (kt_ctr_graph)."""
        hi = 0xFFFFFFFF if max_count is None else int(max_count)
        n = C.c_uint64()
        cen = np.zeros(_lib.KT_GRAPH_CENSUS, np.uint64)
        check(_lib.lib().kt_ctr_graph(self._h, int(min_count), hi, None, None, None, 0, C.byref(n), _ptr(cen), KT_MEM_HOST, 0))
        keys = np.zeros(n.value, np.uint64)
        info = np.zeros(n.value, np.uint32)
        counts = np.zeros(n.value, np.uint32)
        if n.value:
            check(_lib.lib().kt_ctr_graph(self._h, int(min_count), hi, _ptr(keys), _ptr(info), _ptr(counts), n.value,
                                          C.byref(n), None, KT_MEM_HOST, int(bool(sort))))
        return (keys, info, counts, cen) if census else (keys, info, counts)

    def graph_device(self, keys, info, counts, max_out, min_count=1, max_count=None, sort=True, census=None):
        """graph into device tensors of max_out entries (keys u64 / info, counts u32 bit patterns; counts may be None;
        None, None, None, 0 only counts the nodes) and, added, into `census` (KT_GRAPH_CENSUS u64 on the device, or None);
        returns the number of nodes.  Raises KmertoolsError (KT_ERR_ARG) when 0 < max_out < that number."""
        hi = 0xFFFFFFFF if max_count is None else int(max_count)
        n = C.c_uint64()
        check(_lib.lib().kt_ctr_graph(self._h, int(min_count), hi, _ptr(keys), _ptr(info), _ptr(counts), int(max_out),
                                      C.byref(n), _ptr(census), KT_MEM_DEVICE, int(bool(sort))))
        return n.value

    def hetmers(self, min_count=1, max_count=None, middle=False, sort=True, matrix=None, census=False):
        """The heterozygous k-mer pairs of the table (Smudgeplot's hetkmers): the pairs {a, b} of k-mers with min_count <=
        count <= max_count (None: no upper bound) that differ in exactly one base - any base, or with middle=True (odd k)
        the middle one - and have no other such partner, as numpy (keys_a u64, keys_b u64, counts_a u32, counts_b u32),
        a < b as canonical words, ascending by a with sort.  matrix=(n_rows, n_cols): also the u64 matrix m[r, c] = pairs
        with min(minor count, n_rows - 1) == r and min(major count, n_cols - 1) == c.  census=True: also the KT_HET_CENSUS
        u64 cells named by HET_CENSUS_NAMES.  A count-only call, which fills matrix and census, then one call sized by it
        (kt_ctr_hetmers)."""
        hi = 0xFFFFFFFF if max_count is None else int(max_count)
        pos = _lib.KT_HET_MIDDLE if middle else _lib.KT_HET_ALL
        n = C.c_uint64()
        cen = np.zeros(_lib.KT_HET_CENSUS, np.uint64)
        n_rows, n_cols = (int(matrix[0]), int(matrix[1])) if matrix is not None else (0, 0)
        m = np.zeros((n_rows, n_cols), np.uint64) if matrix is not None else None
        check(_lib.lib().kt_ctr_hetmers(self._h, int(min_count), hi, pos, None, None, None, None, 0, C.byref(n), _ptr(m),
                                        n_rows, n_cols, _ptr(cen), KT_MEM_HOST, 0))
        keys_a, keys_b = np.zeros(n.value, np.uint64), np.zeros(n.value, np.uint64)
        counts_a, counts_b = np.zeros(n.value, np.uint32), np.zeros(n.value, np.uint32)
        if n.value:
            check(_lib.lib().kt_ctr_hetmers(self._h, int(min_count), hi, pos, _ptr(keys_a), _ptr(keys_b), _ptr(counts_a),
                                            _ptr(counts_b), n.value, C.byref(n), None, 0, 0, None, KT_MEM_HOST, int(bool(sort))))
        out = (keys_a, keys_b, counts_a, counts_b)
        if matrix is not None:
            out += (m,)
        return out + (cen,) if census else out

    def hetmers_device(self, keys_a, keys_b, counts_a, counts_b, max_out, min_count=1, max_count=None, middle=False, sort=True,
                       matrix=None, n_rows=0, n_cols=0, census=None):
        """hetmers into device tensors of max_out entries (keys u64 / counts u32 bit patterns; either counts may be None;
        None, None, None, None, 0 only counts the pairs) and, added, into `matrix` (n_rows x n_cols u64 on the device, or
        None) and `census` (KT_HET_CENSUS u64 on the device, or None); returns the number of pairs.  Raises KmertoolsError
        (KT_ERR_ARG) when 0 < max_out < that number."""
        hi = 0xFFFFFFFF if max_count is None else int(max_count)
        n = C.c_uint64()
        check(_lib.lib().kt_ctr_hetmers(self._h, int(min_count), hi, _lib.KT_HET_MIDDLE if middle else _lib.KT_HET_ALL,
                                        _ptr(keys_a), _ptr(keys_b), _ptr(counts_a), _ptr(counts_b), int(max_out), C.byref(n),
                                        _ptr(matrix), int(n_rows), int(n_cols), _ptr(census), KT_MEM_DEVICE, int(bool(sort))))
        return n.value

    def unitigs(self, min_count=1, max_count=None):
        """The maximal unitigs of the de Bruijn graph of the table's k-mers with min_count <= count <= max_count (None: no
        upper bound) as numpy (bases u8: ASCII ACGT, concatenated; offsets u64: unitig i = bases[offsets[i]:offsets[i + 1]];
        count_sums u64: the sum of its k-mers' counts; flags u32: UNITIG_CIRCULAR), ascending by the canonical k-mer of
        their start node.  A count-only call, then one call sized by it (kt_ctr_unitigs)."""
        hi = 0xFFFFFFFF if max_count is None else int(max_count)
        nu, nb = C.c_uint64(), C.c_uint64()
        check(_lib.lib().kt_ctr_unitigs(self._h, int(min_count), hi, None, 0, None, None, None, 0, C.byref(nu), C.byref(nb),
                                        KT_MEM_HOST))
        bases = np.zeros(nb.value, np.uint8)
        offsets = np.zeros(nu.value + 1, np.uint64)
        sums = np.zeros(nu.value, np.uint64)
        flags = np.zeros(nu.value, np.uint32)
        if nu.value:
            check(_lib.lib().kt_ctr_unitigs(self._h, int(min_count), hi, _ptr(bases), nb.value, _ptr(offsets), _ptr(sums),
                                            _ptr(flags), nu.value, C.byref(nu), C.byref(nb), KT_MEM_HOST))
        return bases, offsets, sums, flags

    def unitigs_device(self, bases, max_bases, offsets, count_sums, flags, max_unitigs, min_count=1, max_count=None):
        """unitigs into device tensors (bases u8 of max_bases, offsets u64 bit patterns of max_unitigs + 1, count_sums u64 /
        flags u32 of max_unitigs or None; None, 0, None, None, None, 0 only counts); returns (n_unitigs, n_bases).  Raises
        KmertoolsError (KT_ERR_ARG) when either room is too small."""
        hi = 0xFFFFFFFF if max_count is None else int(max_count)
        nu, nb = C.c_uint64(), C.c_uint64()
        check(_lib.lib().kt_ctr_unitigs(self._h, int(min_count), hi, _ptr(bases), int(max_bases), _ptr(offsets), _ptr(count_sums),
                                        _ptr(flags), int(max_unitigs), C.byref(nu), C.byref(nb), KT_MEM_DEVICE))
        return nu.value, nb.value

    def unitig_links(self, min_count=1, max_count=None):
        """unitigs() and the links between the unitigs' ends (kt_ctr_unitigs_linked): returns (bases, offsets, count_sums,
        flags, link_offsets u64, link_to u32).  End e = 2 * u + (the sign is '-') of unitig u owns
        link_to[link_offsets[e]:link_offsets[e + 1]]; each value is 2 * v + (the sign is '-'), ascending: the end's last
        k - 1 bases are the first k - 1 of that oriented unitig.  A count-only call, then one call sized by it."""
        hi = 0xFFFFFFFF if max_count is None else int(max_count)
        nu, nb, nl = C.c_uint64(), C.c_uint64(), C.c_uint64()
        check(_lib.lib().kt_ctr_unitigs_linked(self._h, int(min_count), hi, None, 0, None, None, None, 0, C.byref(nu), C.byref(nb),
                                               None, None, 0, C.byref(nl), KT_MEM_HOST))
        bases = np.zeros(nb.value, np.uint8)
        offsets = np.zeros(nu.value + 1, np.uint64)
        sums = np.zeros(nu.value, np.uint64)
        flags = np.zeros(nu.value, np.uint32)
        link_offsets = np.zeros(2 * nu.value + 1, np.uint64)
        link_to = np.zeros(nl.value, np.uint32)
        if nu.value:
            check(_lib.lib().kt_ctr_unitigs_linked(self._h, int(min_count), hi, _ptr(bases), nb.value, _ptr(offsets), _ptr(sums),
                                                   _ptr(flags), nu.value, C.byref(nu), C.byref(nb), _ptr(link_offsets),
                                                   _ptr(link_to), nl.value, C.byref(nl), KT_MEM_HOST))
        return bases, offsets, sums, flags, link_offsets, link_to

    def unitigs_linked_device(self, bases, max_bases, offsets, count_sums, flags, max_unitigs, link_offsets, link_to, max_links,
                              min_count=1, max_count=None):
        """unitigs_device with the links: link_offsets (u64 bit patterns of 2 * max_unitigs + 1) and link_to (u32 bit patterns
        of max_links) are device tensors as well (None, 0, None, None, None, 0, None, None, 0 only counts); returns
        (n_unitigs, n_bases, n_links).  Raises KmertoolsError (KT_ERR_ARG) when any room is too small."""
        hi = 0xFFFFFFFF if max_count is None else int(max_count)
        nu, nb, nl = C.c_uint64(), C.c_uint64(), C.c_uint64()
        check(_lib.lib().kt_ctr_unitigs_linked(self._h, int(min_count), hi, _ptr(bases), int(max_bases), _ptr(offsets),
                                               _ptr(count_sums), _ptr(flags), int(max_unitigs), C.byref(nu), C.byref(nb),
                                               _ptr(link_offsets), _ptr(link_to), int(max_links), C.byref(nl), KT_MEM_DEVICE))
        return nu.value, nb.value, nl.value

    def unitig_components(self, min_count=1, max_count=None):
        """The connected components of the unitig graph (unitig_links' unitigs and links): the linked run into device tensors,
        then Context.unitig_components on them.  Returns {"component", "stats", "tally", "n_unitigs"} of host arrays."""
        import torch
        nu, nb, nl = self.unitigs_linked_device(None, 0, None, None, None, 0, None, None, 0, min_count, max_count)
        out = {"component": np.zeros(nu, np.uint32), "stats": np.zeros((0, _lib.KT_COMPONENT_FIELDS), np.uint64),
               "tally": np.zeros(_lib.KT_COMPONENT_TALLY, np.uint64), "n_unitigs": nu}
        if not nu:
            return out
        dev = torch.device("cuda", self.ctx.device)
        bases = torch.empty(nb, dtype=torch.uint8, device=dev)
        offsets = torch.empty(nu + 1, dtype=torch.int64, device=dev)
        sums = torch.empty(nu, dtype=torch.int64, device=dev)
        flags = torch.empty(nu, dtype=torch.int32, device=dev)
        link_offsets = torch.empty(2 * nu + 1, dtype=torch.int64, device=dev)
        link_to = torch.empty(max(nl, 1), dtype=torch.int32, device=dev)
        self.unitigs_linked_device(bases, nb, offsets, sums, flags, nu, link_offsets, link_to, nl, min_count, max_count)
        comp = torch.empty(nu, dtype=torch.int32, device=dev)
        stats = torch.empty((nu, _lib.KT_COMPONENT_FIELDS), dtype=torch.int64, device=dev)
        tally = torch.empty(_lib.KT_COMPONENT_TALLY, dtype=torch.int64, device=dev)
        nc = self.ctx.unitig_components(link_offsets, link_to, nu, comp, offsets, sums, self.k, stats, nu, tally)
        self.ctx.sync()
        out["component"] = comp.cpu().numpy().view(np.uint32)
        out["stats"] = stats[:nc].cpu().numpy().view(np.uint64)
        out["tally"] = tally.cpu().numpy().view(np.uint64)
        return out

    def unitig_tips(self, max_tip_nodes=None, min_count=1, max_count=None):
        """One round of the tip rule over unitigs()' numbering (kt_ctr_unitig_tips; the table is not changed): returns (marks u8:
        TIP_KEEP / TIP_TIP / TIP_ISOLATED per unitig, tally u64[4]: tips, their nodes, isolated short unitigs, their nodes).
        max_tip_nodes None: k nodes.  A count-only call, then one call sized by it."""
        hi = 0xFFFFFFFF if max_count is None else int(max_count)
        tip = self.k if max_tip_nodes is None else int(max_tip_nodes)
        nu = C.c_uint64()
        tally = np.zeros(_lib.KT_TIP_TALLY, np.uint64)
        check(_lib.lib().kt_ctr_unitig_tips(self._h, int(min_count), hi, tip, None, 0, C.byref(nu), _ptr(tally), KT_MEM_HOST))
        marks = np.zeros(nu.value, np.uint8)
        if nu.value:
            check(_lib.lib().kt_ctr_unitig_tips(self._h, int(min_count), hi, tip, _ptr(marks), nu.value, C.byref(nu), _ptr(tally),
                                                KT_MEM_HOST))
        return marks, tally

    def unitig_tips_device(self, marks, max_unitigs, tally=None, max_tip_nodes=None, min_count=1, max_count=None):
        """unitig_tips into device tensors (marks u8 of max_unitigs, tally u64 bit patterns of 4 or None; None, 0 only counts
        and still fills tally); returns n_unitigs.  Raises KmertoolsError (KT_ERR_ARG) when the room is too small."""
        hi = 0xFFFFFFFF if max_count is None else int(max_count)
        tip = self.k if max_tip_nodes is None else int(max_tip_nodes)
        nu = C.c_uint64()
        check(_lib.lib().kt_ctr_unitig_tips(self._h, int(min_count), hi, tip, _ptr(marks), int(max_unitigs), C.byref(nu),
                                            _ptr(tally), KT_MEM_DEVICE))
        return nu.value

    def clip_tips(self, max_tip_nodes=None, max_rounds=8, drop_isolated=False, min_count=1, max_count=None):
        """Clips the tips of the table's de Bruijn graph in place, round after round until a round finds none or max_rounds
        are done (kt_ctr_clip_tips): the k-mers of every tip - with drop_isolated, of every isolated short unitig too - are
        erased from the table.  max_tip_nodes None: k nodes.  Returns the stats as a dict (CLIP_STATS_NAMES)."""
        hi = 0xFFFFFFFF if max_count is None else int(max_count)
        tip = self.k if max_tip_nodes is None else int(max_tip_nodes)
        stats = np.zeros(_lib.KT_CLIP_STATS, np.uint64)
        check(_lib.lib().kt_ctr_clip_tips(self._h, int(min_count), hi, tip, int(max_rounds), CLIP_ISOLATED if drop_isolated else 0,
                                          _ptr(stats)))
        stats[6] = 1 - stats[6]  # (the call says whether the last round still erased something)
        return {name: int(v) for name, v in zip(CLIP_STATS_NAMES, stats)}

    def unitig_bubbles(self, max_bubble_nodes=None, min_count=1, max_count=None):
        """One round of the bubble rule over unitigs()' numbering (kt_ctr_unitig_bubbles; the table is not changed): returns
        (marks u8: 0 or BUBBLE_POP per unitig, tally u64[4]: popped unitigs, their nodes, bubbles, occurrences popped).
        max_bubble_nodes None: 2k nodes.  A count-only call, then one call sized by it."""
        hi = 0xFFFFFFFF if max_count is None else int(max_count)
        mb = 2 * self.k if max_bubble_nodes is None else int(max_bubble_nodes)
        nu = C.c_uint64()
        tally = np.zeros(_lib.KT_BUBBLE_TALLY, np.uint64)
        check(_lib.lib().kt_ctr_unitig_bubbles(self._h, int(min_count), hi, mb, None, 0, C.byref(nu), _ptr(tally), KT_MEM_HOST))
        marks = np.zeros(nu.value, np.uint8)
        if nu.value:
            check(_lib.lib().kt_ctr_unitig_bubbles(self._h, int(min_count), hi, mb, _ptr(marks), nu.value, C.byref(nu), _ptr(tally),
                                                   KT_MEM_HOST))
        return marks, tally

    def unitig_bubbles_device(self, marks, max_unitigs, tally=None, max_bubble_nodes=None, min_count=1, max_count=None):
        """unitig_bubbles into device tensors (marks u8 of max_unitigs, tally u64 bit patterns of 4 or None; None, 0 only counts
        and still fills tally); returns n_unitigs.  Raises KmertoolsError (KT_ERR_ARG) when the room is too small."""
        hi = 0xFFFFFFFF if max_count is None else int(max_count)
        mb = 2 * self.k if max_bubble_nodes is None else int(max_bubble_nodes)
        nu = C.c_uint64()
        check(_lib.lib().kt_ctr_unitig_bubbles(self._h, int(min_count), hi, mb, _ptr(marks), int(max_unitigs), C.byref(nu),
                                               _ptr(tally), KT_MEM_DEVICE))
        return nu.value

    def simplify(self, max_tip_nodes=None, max_bubble_nodes=None, max_rounds=8, drop_isolated=False, min_count=1, max_count=None):
        """Clips the tips and pops the bubbles of the table's de Bruijn graph in place, both rules in every round, until a round
        finds nothing or max_rounds are done (kt_ctr_simplify).  max_tip_nodes None: k nodes, max_bubble_nodes None: 2k nodes;
        0 switches a rule off.  Returns the stats as a dict (SIMPLIFY_STATS_NAMES)."""
        hi = 0xFFFFFFFF if max_count is None else int(max_count)
        tip = self.k if max_tip_nodes is None else int(max_tip_nodes)
        mb = 2 * self.k if max_bubble_nodes is None else int(max_bubble_nodes)
        stats = np.zeros(_lib.KT_SIMPLIFY_STATS, np.uint64)
        check(_lib.lib().kt_ctr_simplify(self._h, int(min_count), hi, tip, mb, int(max_rounds), CLIP_ISOLATED if drop_isolated else 0,
                                         _ptr(stats)))
        stats[9] = 1 - stats[9]  # (the call says whether the last round still erased something)
        return {name: int(v) for name, v in zip(SIMPLIFY_STATS_NAMES, stats)}

    def export_stage_range(self, min_count=1, max_count=None):
        """stages the entries with min_count <= count <= max_count on the device; returns how many (export_fetch reads them)"""
        n = C.c_uint64()
        hi = 0xFFFFFFFF if max_count is None else int(max_count)
        check(_lib.lib().kt_ctr_export_stage_range(self._h, int(min_count), hi, C.byref(n)))
        return n.value

    def export_fetch(self, first, count):
        keys = np.zeros(max(count, 1), np.uint64)
        counts = np.zeros(max(count, 1), np.uint32)
        if count:
            check(_lib.lib().kt_ctr_export_fetch(self._h, int(first), int(count), _ptr(keys), _ptr(counts)))
        return keys[:count], counts[:count]

    def export_host(self, sort=True, min_count=1, max_count=None):
        """(keys, counts) of the table; with a count range (min_count > 1 or max_count given) only the entries in it,
        filtered on the device (kt_ctr_export_stage_range)"""
        if min_count > 1 or max_count is not None:
            keys, counts = self.export_fetch(0, self.export_stage_range(min_count, max_count))
        else:
            n = self.size()
            keys = np.zeros(max(n, 1), np.uint64)
            counts = np.zeros(max(n, 1), np.uint32)
            got = self.export(keys, counts, n, KT_MEM_HOST) if n else 0
            keys, counts = keys[:got], counts[:got]
        if sort:
            order = np.argsort(keys, kind="stable")
            keys, counts = keys[order], counts[order]
        return keys, counts

    def save(self, path, min_count=1, max_count=None, append=False):
        """writes the entries with min_count <= count <= max_count as one section of the table file `path` (created, or
        with append=True extended); returns how many entries went (kt_ctr_save)"""
        n = C.c_uint64()
        hi = 0xFFFFFFFF if max_count is None else int(max_count)
        check(_lib.lib().kt_ctr_save(self._h, os.fsencode(path), int(min_count), hi, int(bool(append)), C.byref(n)))
        return n.value

    def add_file(self, path):
        """table[key] += count for every entry of every section of the table file `path`; returns the entries read
        (kt_ctr_add_file)"""
        n = C.c_uint64()
        check(_lib.lib().kt_ctr_add_file(self._h, os.fsencode(path), C.byref(n)))
        return n.value

    @classmethod
    def from_file(cls, ctx, path, slots=None):
        """a new table of the file's k holding the file; slots=None sizes it as the command line does: 1.9 slots per entry
        of the file, at least 1024"""
        info = table_file_info(path)
        if slots is None:
            slots = max(1024, info["entries"] + info["entries"] // 10 * 9)
        t = cls(ctx, info["k"], slots)
        try:
            t.add_file(path)
        except Exception:
            t.close()
            raise
        return t


class UnitigIndex:
    """The k-mer -> (unitig, offset, strand) index of a set of unitigs (host arrays: bases u8, offsets u64, as
    Counter.unitigs returns them): owns the index table, sized from the number of k-mers the unitigs can hold."""

    def __init__(self, ctx, k, bases, offsets):
        self.ctx, self.k = ctx, k
        self.offsets = np.ascontiguousarray(offsets, np.uint64)
        bases = np.ascontiguousarray(bases, np.uint8)
        lens = np.diff(self.offsets.astype(np.int64))
        windows = int(np.maximum(lens - (k - 1), 0).sum())
        self.table = Counter(ctx, k, max(1024, windows + windows // 10 * 9))  # (1.9 slots per entry, as the command line sizes)
        try:
            self.n_kmers = self.table.index_sequences_host(bases, self.offsets)
        except Exception:
            self.table.close()
            raise

    def close(self):
        self.table.close()

    def thread_host(self, bases, offsets, unitig_hits=None, unitig_runs=None):
        """-> {"hits" u32 per base, "run_start", "run_len", "run_unitig", "run_upos", "run_offsets", "tally"} of host arrays
        for a batch of reads (Counter.thread_hits_host, then Context.thread_runs_host)"""
        offsets = np.ascontiguousarray(offsets, np.uint64)
        hits = self.table.thread_hits_host(bases, offsets)
        out = self.ctx.thread_runs_host(hits, offsets, self.offsets, self.k, unitig_hits, unitig_runs)
        out["hits"] = hits
        return out


class Sharded:
    """This rank's part of a table sharded over n_ranks GPUs by hash prefix (kt_sharded).  add_reads and finalize are
    collective: every rank calls them the same number of times.  `transport`: ("rccl", id128 bytes) or
    ("host", alltoall) where alltoall(send_addr, recv_addr, bytes_per_rank) moves host memory and returns 0.
    connect=False: allocate only (kt_sharded_create_local); the caller agrees with its peers and calls connect()."""

    def __init__(self, ctx, k, capacity_slots, max_batch_bases, n_ranks=1, rank=0, transport=None, connect=True):
        self.ctx, self.k, self.n_ranks, self.rank = ctx, k, n_ranks, rank
        self._h = C.c_void_p()
        self._cb = None
        self._cb_exc = None
        self._transport = transport
        L = _lib.lib()
        if n_ranks > 1 and transport is None:
            raise ValueError("a sharded counter over several ranks needs a transport")
        if transport is not None and transport[0] not in ("rccl", "host"):
            raise ValueError("unknown transport %r" % (transport[0],))
        check(L.kt_sharded_create_local(ctx._h, k, int(capacity_slots), int(max_batch_bases), n_ranks, rank,
                                        C.byref(self._h)))
        t = C.c_void_p()
        check(L.kt_sharded_table(self._h, C.byref(t)))
        self.table = Counter.__new__(Counter)   # a view of the shard: owned by the kt_sharded
        self.table.ctx, self.table.k, self.table._h = ctx, k, t
        self.table.close = lambda: None
        if connect:
            self.connect()

    def connect(self):
        """brings the transport up (RCCL: ncclCommInitRank - every rank must get here)"""
        L = _lib.lib()
        transport = self._transport
        if self.n_ranks == 1 or transport[0] == "rccl":
            idb = None if self.n_ranks == 1 else (C.c_uint8 * 128).from_buffer_copy(bytes(transport[1]))
            check(L.kt_sharded_connect_rccl(self._h, idb))
        else:
            fn = transport[1]

            def cb(user, send, recv, nbytes):
                # an exception must not be swallowed by ctypes (it would return 0 = success and the library would count
                # whatever the receive buffer held): report failure, keep the exception for the caller
                try:
                    return int(fn(send, recv, nbytes))
                except BaseException as e:  # noqa: BLE001
                    self._cb_exc = e
                    return 1
            self._cb = _lib.ALLTOALL_FN(cb)
            check(L.kt_sharded_connect_host(self._h, C.cast(self._cb, C.c_void_p), None))

    def _checked(self, rc):
        if self._cb_exc is not None:
            e, self._cb_exc = self._cb_exc, None
            raise e
        check(rc)

    def owner_of(self, kmer):
        o = C.c_uint32()
        check(_lib.lib().kt_sharded_owner_of(self._h, int(kmer), C.byref(o)))
        return o.value

    @staticmethod
    def unique_id():
        buf = (C.c_uint8 * 128)()
        check(_lib.lib().kt_rccl_unique_id(buf))
        return bytes(buf)

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            self.table._h = C.c_void_p()
            _lib.lib().kt_sharded_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def clear(self):
        check(_lib.lib().kt_sharded_clear(self._h))

    def add_reads(self, bases, offsets, n_reads, mem=KT_MEM_DEVICE):
        self._checked(_lib.lib().kt_sharded_add_reads(self._h, _ptr(bases), _ptr(offsets), n_reads, mem))

    def add_reads_host(self, bases, offsets):
        bases = np.ascontiguousarray(bases, np.uint8)
        offsets = np.ascontiguousarray(offsets, np.uint64)
        self.add_reads(bases if bases.size else np.zeros(1, np.uint8), offsets, len(offsets) - 1, KT_MEM_HOST)

    def finalize(self):
        self._checked(_lib.lib().kt_sharded_finalize(self._h))

    def exchanged_bytes(self):
        n = C.c_uint64()
        check(_lib.lib().kt_sharded_exchanged_bytes(self._h, C.byref(n)))
        return n.value

    def route_stats(self):
        """-> (records, kmers): numpy arrays per owner, what the last batch's route pass put into every owner's region"""
        n = C.c_uint32()
        rec = np.zeros(64, np.uint64)
        km = np.zeros(64, np.uint64)
        check(_lib.lib().kt_sharded_route_stats(self._h, C.byref(n), rec.ctypes.data_as(C.c_void_p), km.ctypes.data_as(C.c_void_p)))
        return rec[:n.value], km[:n.value]

    def comm_info(self):
        """-> dict(n_ranks, rccl_ranks, transport): rccl_ranks is ncclCommCount of the library's own communicator
        (0 without one), transport "none" / "rccl" / "host" (kt_sharded_comm_info)"""
        a, b, c = C.c_int(), C.c_int(), C.c_int()
        check(_lib.lib().kt_sharded_comm_info(self._h, C.byref(a), C.byref(b), C.byref(c)))
        return {"n_ranks": a.value, "rccl_ranks": b.value, "transport": ("none", "rccl", "host")[c.value]}
