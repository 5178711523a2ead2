// kt_thread.hip - reads threaded onto the unitigs of a table: which unitigs a read walks through, where and in which
// orientation (`kmertools thread`; what Bifrost query, GGCAT query and GraphAligner's exact mode answer on the CPU).
//
// A kt_ctr table stores a u32 beside every key, so a table whose "count" is the k-mer's position in the unitigs is the whole
// k-mer -> (unitig, offset, strand) index.  Three calls:
//   kt_ctr_index_sequences  walks the sequences (the unitigs) once on the segment front-end and writes, per base G, the pair
//                           (canonical k-mer of the window at G, 1 + 2 G + S) - S: the sequence shows the reverse complement of
//                           the canonical k-mer -, KT_EMPTY_KEY where no window starts; kt_ctr_add_pairs' device path places
//                           them.  A k-mer that occurs twice shows as a table smaller than the number of windows.
//   kt_ctr_thread_hits      kt_ctr_profile's kernel with another sink: the probe pipeline (kt_probe.hpp) hands the strand of
//                           the read's k-mer along with the stored value, and the entry is the value with the two strands
//                           combined: 1 + ((value - 1) ^ t).
//   kt_thread_runs          a pure function of that array: maximal stretches of positions that step along one unitig in one
//                           orientation.  A position's class and whether it continues the one before are functions of the
//                           entries at j - 1, j, j + 1 and of two bit arrays made first (where in the unitigs a window may
//                           start; where a read starts), so the run starts and run ends are flagged without a search; one
//                           scan (kt_scan.hpp) numbers both, the apply pass writes every run's first and last position, and
//                           only then one thread per RUN looks its unitig up in unitig_offsets.
#include "kt_internal.hpp"
#include "kt_launch.hpp"
#include "kt_probe.hpp"
#include "kt_scan.hpp"
#include "kt_segment.hpp"
#include "kt_table.hpp"

namespace {

using ktseg::SegArgs;
using ktseg::SegShared;
using kttab::Probed;

constexpr int BLOCK = ktseg::BLOCK;
constexpr uint32_t GROUP = ktprobe::GROUP;
constexpr uint32_t NO = KT_NO_KMER;
constexpr uint64_t MAX_INDEX_BASES = 0x7FFFFFFEull;  // 1 + 2 G + S <= 0xFFFFFFFE

// ---- kt_ctr_index_sequences: the (key, value) pair of every base -----------------------------------------------------------
// Every base below the batch's end gets a pair, so the arrays need no fill: KT_EMPTY_KEY (which kt_ctr_add_pairs skips)
// where no window starts.
__global__ __launch_bounds__(BLOCK) void index_pairs_kernel(SegArgs a, uint64_t total, uint64_t *__restrict__ keys,
                                                            uint32_t *__restrict__ vals, unsigned long long *__restrict__ n_windows) {
    __shared__ SegShared sm;
    const uint32_t tid = threadIdx.x;
    uint32_t mine = 0;
    for (uint64_t g = blockIdx.x; g < a.n_seg; g += gridDim.x) {
        ktseg::stage_segment(a, g, sm);
        ktseg::Window w(sm, tid, a.k);
        const uint64_t s0 = g * ktseg::SEG + (uint64_t)ktseg::PER_THREAD * tid;
        mine += (uint32_t)__builtin_popcount(w.okm);
#pragma unroll 4
        for (uint32_t j = 0; j < ktseg::PER_THREAD; j++) {
            const uint64_t s = s0 + j;
            if (s < total) {
                const bool ok = w.ok(j);
                // (s <= 2^31 - 2: checked by the caller)
                keys[s] = ok ? (w.f < w.r ? w.f : w.r) : KT_EMPTY_KEY;
                vals[s] = ok ? 1u + 2u * (uint32_t)s + (uint32_t)(w.f > w.r) : 0u;
            }
            w.step();
        }
        __syncthreads();  // sm is restaged by the next segment
    }
    mine = ktd::wave_all_sum(mine);
    if ((tid & 63u) == 0 && mine) atomicAdd(n_windows, (unsigned long long)mine);
}

// ---- kt_ctr_thread_hits: profile_kernel's stores, the value oriented ----------------------------------------------------------
struct HitsArgs {
    Probed t;
    uint32_t *hits;  // offsets[n_reads] entries, indexed by global base index
};

__global__ __launch_bounds__(BLOCK) void thread_hits_kernel(SegArgs a, HitsArgs c) {
    __shared__ SegShared sm;
    const uint32_t tid = threadIdx.x;
    const bool aligned = ((uintptr_t)c.hits & 15u) == 0;

    for (uint64_t g = blockIdx.x; g < a.n_seg; g += gridDim.x) {
        ktseg::stage_segment(a, g, sm);
        ktseg::Window w(sm, tid, a.k);
        if (w.okm) {
            // (a valid window lies inside the batch, so every entry written is below offsets[n_reads])
            uint32_t *dst = c.hits + g * ktseg::SEG + (uint64_t)ktseg::PER_THREAD * tid;
            ktprobe::probe_windows<true>(c.t, w, [&](uint32_t jj, uint32_t wr, const uint32_t (&cnt)[GROUP], uint32_t rc) {
                // stored value v = 1 + 2 G + S; the read's strand t flips S: 1 + ((v - 1) ^ t), 0 for an absent k-mer (the
                // sentinel is no position: an index never holds v = 0xFFFFFFFF)
                auto oriented = [&](uint32_t u) {
                    const uint32_t v = cnt[u] ? 1u + ((cnt[u] - 1u) ^ ((rc >> u) & 1u)) : 0u;
                    return v < NO ? v : NO - 1u;
                };
#pragma unroll
                for (uint32_t q = 0; q < GROUP; q += 4) {
                    const uint32_t m = (wr >> q) & 15u;
                    if (m == 15u && aligned) {
                        *reinterpret_cast<uint4 *>(dst + jj + q) = make_uint4(oriented(q), oriented(q + 1), oriented(q + 2), oriented(q + 3));
                    } else {
#pragma unroll
                        for (uint32_t u = 0; u < 4; u++)
                            if ((m >> u) & 1u) dst[jj + q + u] = oriented(q + u);
                    }
                }
            });
        }
        __syncthreads();  // sm is restaged by the next segment
    }
}

// ---- kt_thread_runs -------------------------------------------------------------------------------------------------------------
// ubits: one bit per base G of the unitigs.  k >= 2: set = a window may start at G (it lies inside its unitig); two hits at
// G and G + 1 are then in one unitig, for the last k - 1 bases of every unitig are clear.  k = 1: every base below the end is
// a window start, and set = G is the first base of a unitig, which is what a step from G - 1 to G must not cross.
// rbits: one bit per base of the batch and one more: set = a read starts here (the bit at `total` is always set: the reads
// that end the batch without a base, and run_offsets[n_reads], are written from there).
struct RunArgs {
    const uint32_t *hits;
    const uint32_t *ubits, *rbits;
    uint64_t total, ub;  // bases of the batch, bases of the unitigs
    uint32_t k;
};

enum Kind : uint32_t { NONE = 0, MISS = 1, BAD = 2, HIT = 3 };

__device__ __forceinline__ uint32_t bit_at(const uint32_t *bits, uint64_t i) { return (bits[i >> 5] >> (i & 31u)) & 1u; }

__device__ __forceinline__ uint32_t classify(const RunArgs &c, uint64_t j, uint32_t &a, uint64_t &G) {
    const uint32_t v = c.hits[j];
    if (v == NO) return NONE;
    if (v == 0u) return MISS;
    a = (v - 1u) & 1u;
    G = (uint64_t)((v - 1u) >> 1);
    if (G >= c.ub) return BAD;
    return c.k == 1u || bit_at(c.ubits, G) ? HIT : BAD;
}

// does the hit (a, G) at j continue the position before it?  (a1, G1) at j - 1 must be a hit of the same read that lies one
// step back along the oriented unitig
__device__ __forceinline__ bool continues(const RunArgs &c, uint64_t j, uint32_t a, uint64_t G) {
    if (j == 0 || bit_at(c.rbits, j)) return false;
    uint32_t a1 = 0;
    uint64_t G1 = 0;
    if (classify(c, j - 1, a1, G1) != HIT || a1 != a) return false;
    if (a == 0u ? G != G1 + 1 : G + 1 != G1) return false;
    return c.k != 1u || !bit_at(c.ubits, a == 0u ? G : G1);
}

// bit 0: a run starts at j, bit 1: a run ends at j, bit 2: a read starts at j, bits 4..5: the position's Kind
__device__ __forceinline__ uint32_t run_word(const RunArgs &c, uint64_t j) {
    if (j >= c.total) return j == c.total ? 4u : 0u;
    uint32_t a = 0, a2 = 0;
    uint64_t G = 0, G2 = 0;
    const uint32_t kind = classify(c, j, a, G);
    uint32_t w = (bit_at(c.rbits, j) << 2) | (kind << 4);
    if (kind == HIT) {
        if (!continues(c, j, a, G)) w |= 1u;
        if (!(j + 1 < c.total && classify(c, j + 1, a2, G2) == HIT && continues(c, j + 1, a2, G2))) w |= 2u;
    }
    return w;
}

// the scan's functor: sum a = run starts, sum b = run ends before an item (the r-th end closes the r-th start)
struct RunScan {
    RunArgs c;
    const uint64_t *read_offsets;
    uint64_t n_reads;
    uint64_t *run_start;   // null: nothing is written per run (the counting call)
    uint32_t *run_last;    // the low 32 bits of the run's last position (run_len's array, until runs_finish_kernel)
    uint64_t *run_offsets;
    __device__ __forceinline__ uint32_t word(uint64_t i) const { return run_word(c, i); }
    __device__ __forceinline__ void add(uint32_t w, uint64_t &a, uint64_t &b) const {
        a += w & 1u;
        b += (w >> 1) & 1u;
    }
    __device__ __forceinline__ void put(uint64_t i, uint64_t a, uint64_t b) const {
        const uint32_t w = run_word(c, i);
        if (run_start) {
            if (w & 1u) run_start[a] = i;
            if (w & 2u) run_last[b] = (uint32_t)i;
        }
        if (w & 4u) {
            // the reads that start at i (empty ones first, then the one that holds base i): `a` runs lie before them
            uint64_t lo = 0, hi = n_reads + 1;  // the first r with read_offsets[r] >= i
            while (lo < hi) {
                const uint64_t mid = (lo + hi) >> 1;
                if (read_offsets[mid] < i) lo = mid + 1; else hi = mid;
            }
            for (uint64_t r = lo; r <= n_reads && read_offsets[r] == i; r++) run_offsets[r] = a;
        }
    }
    __device__ __forceinline__ void total() const {}
};

// one thread per unitig: the bits of ubits that differ from the fill (k >= 2: all ones, k = 1: all zeros)
__global__ __launch_bounds__(BLOCK) void unitig_bits_kernel(const uint64_t *__restrict__ uoff, uint64_t n_unitigs, uint32_t k,
                                                            uint32_t *__restrict__ ubits) {
    for (uint64_t u = (uint64_t)blockIdx.x * BLOCK + threadIdx.x; u < n_unitigs; u += (uint64_t)gridDim.x * BLOCK) {
        const uint64_t lo = uoff[u], hi = uoff[u + 1];
        if (hi <= lo) continue;
        if (k == 1u) {
            atomicOr(&ubits[lo >> 5], 1u << (lo & 31u));
        } else {
            // no window starts at the last k - 1 bases (a unitig shorter than k holds none at all)
            for (uint64_t G = hi - lo >= k ? hi - (k - 1u) : lo; G < hi; G++) atomicAnd(&ubits[G >> 5], ~(1u << (G & 31u)));
        }
    }
}

__global__ __launch_bounds__(BLOCK) void read_bits_kernel(const uint64_t *__restrict__ roff, uint64_t n_reads, uint32_t *__restrict__ rbits) {
    for (uint64_t r = (uint64_t)blockIdx.x * BLOCK + threadIdx.x; r <= n_reads; r += (uint64_t)gridDim.x * BLOCK) {
        // (the offsets' last entry marks the batch's end)
        if (r == n_reads || roff[r + 1] > roff[r]) atomicOr(&rbits[roff[r] >> 5], 1u << (roff[r] & 31u));
    }
}

// tally[0..3] += windows, hits, misses, bad values
__global__ __launch_bounds__(BLOCK) void runs_tally_kernel(RunArgs c, unsigned long long *__restrict__ tally) {
    uint32_t n[4] = {0, 0, 0, 0};
    // (a thread's positions are below 2^32 in number: the grid is at least a workgroup wide)
    for (uint64_t j = (uint64_t)blockIdx.x * BLOCK + threadIdx.x; j < c.total; j += (uint64_t)gridDim.x * BLOCK) {
        uint32_t a;
        uint64_t G;
        const uint32_t kind = classify(c, j, a, G);
        n[0] += kind != NONE;
        n[1] += kind == HIT;
        n[2] += kind == MISS;
        n[3] += kind == BAD;
    }
#pragma unroll
    for (int q = 0; q < 4; q++) {
        const uint32_t v = ktd::wave_all_sum(n[q]);
        if ((threadIdx.x & 63u) == 0 && v) atomicAdd(&tally[q], (unsigned long long)v);
    }
}

// one thread per run: its length, and - the one search - its unitig and the offset in it; the per-unitig sums
__global__ __launch_bounds__(BLOCK) void runs_finish_kernel(RunArgs c, const uint64_t *__restrict__ uoff, uint64_t n_unitigs,
                                                            uint64_t n_runs, const uint64_t *__restrict__ run_start,
                                                            uint32_t *__restrict__ run_len, uint32_t *__restrict__ run_unitig,
                                                            uint32_t *__restrict__ run_upos, unsigned long long *__restrict__ unitig_hits,
                                                            unsigned long long *__restrict__ unitig_runs) {
    for (uint64_t r = (uint64_t)blockIdx.x * BLOCK + threadIdx.x; r < n_runs; r += (uint64_t)gridDim.x * BLOCK) {
        const uint64_t j = run_start[r];
        const uint32_t len = run_len[r] - (uint32_t)j + 1u;  // (run_len held the last position mod 2^32; a read has fewer bases than that)
        const uint32_t v = c.hits[j] - 1u;
        const uint64_t G = (uint64_t)(v >> 1);
        uint64_t lo = 0, hi = n_unitigs;  // the last u with uoff[u] <= G (an empty unitig before it shares the offset)
        while (hi - lo > 1) {
            const uint64_t mid = (lo + hi) >> 1;
            if (uoff[mid] <= G) lo = mid; else hi = mid;
        }
        run_len[r] = len;
        run_unitig[r] = 2u * (uint32_t)lo + (v & 1u);
        run_upos[r] = (uint32_t)(G - uoff[lo]);
        if (unitig_hits) atomicAdd(&unitig_hits[lo], (unsigned long long)len);
        if (unitig_runs) atomicAdd(&unitig_runs[lo], 1ull);
    }
}

// tally[5] += the reads that own a run
__global__ __launch_bounds__(BLOCK) void reads_hit_kernel(const uint64_t *__restrict__ run_offsets, uint64_t n_reads,
                                                          unsigned long long *__restrict__ tally) {
    uint32_t n = 0;
    for (uint64_t r = (uint64_t)blockIdx.x * BLOCK + threadIdx.x; r < n_reads; r += (uint64_t)gridDim.x * BLOCK)
        n += run_offsets[r + 1] > run_offsets[r];
    n = ktd::wave_all_sum(n);
    if ((threadIdx.x & 63u) == 0 && n) atomicAdd(&tally[5], (unsigned long long)n);
}

}  // namespace

using namespace ktl;

extern "C" int kt_ctr_index_sequences(kt_ctr *index, const uint8_t *bases, const uint64_t *offsets, uint64_t n_seqs,
                                      uint64_t *n_kmers, int mem) {
    if (!index) return kt::fail(KT_ERR_ARG, "kt_ctr_index_sequences: null index");
    kt_ctx *ctx = index->ctx;
    Call call(ctx, mem, "kt_ctr_index_sequences");
    if (int rc = call.enter()) return rc;
    if (int rc = call.refuse_shard(index)) return rc;
    if (!n_kmers) return call.fail("null n_kmers");
    if (n_seqs && !offsets) return call.fail("null buffer");
    uint64_t held = 0;
    if (int rc = kt_ctr_size(index, &held)) return rc;  // (KT_ERR_FULL for an overflowed table)
    if (held) return call.fail("the index table is not empty");
    *n_kmers = 0;
    if (n_seqs == 0) return KT_OK;
    if (int rc = call.batch(bases, offsets, n_seqs)) return rc;
    if (call.total > MAX_INDEX_BASES)
        return call.fail("more than 2^31 - 2 bases: a position, 1 + 2 * base + strand, is a u32 below 0xFFFFFFFF");
    if (!call.total) return KT_OK;
    if (int rc = call.stage()) return rc;
    const uint64_t total = call.total;
    uint64_t *d_keys = nullptr;
    uint32_t *d_vals = nullptr;
    if (int rc = call.scratch(kt::AUX1, (total + 1) * 8, &d_keys)) return rc;  // (+ the window counter)
    if (int rc = call.scratch(kt::AUX2, total * 4, &d_vals)) return rc;
    unsigned long long *d_n = (unsigned long long *)(d_keys + total);
    KT_HIP(hipMemsetAsync(d_n, 0, 8, ctx->stream));
    SegArgs a;
    if (int rc = make_seg_args(ctx, call.bases, call.offsets, n_seqs, total, index->k, &a)) return rc;
    hipLaunchKernelGGL(index_pairs_kernel, dim3(grid_for(ctx, a.n_seg, 8)), dim3(BLOCK), 0, ctx->stream, a, total, d_keys, d_vals, d_n);
    KT_HIP(hipGetLastError());
    if (int rc = kt_ctr_add_pairs(index, d_keys, d_vals, total, KT_MEM_DEVICE)) return rc;
    uint64_t windows = 0;
    KT_HIP(hipMemcpyAsync(&windows, d_n, 8, hipMemcpyDeviceToHost, ctx->stream));
    if (int rc = kt_ctr_size(index, &held)) return rc;  // (waits for the stream; KT_ERR_FULL as in kt_ctr_add_pairs)
    *n_kmers = windows;
    if (held != windows) {
        if (int rc = kt_ctr_clear(index)) return rc;
        return call.fail(("a k-mer occurs more than once in the sequences (" + std::to_string(held) + " distinct k-mers in " +
                          std::to_string(windows) + " windows): the positions of a repeated k-mer added up, so the table was cleared")
                             .c_str());
    }
    return KT_OK;
}

extern "C" int kt_ctr_thread_hits(kt_ctr *index, const uint8_t *bases, const uint64_t *offsets, uint64_t n_reads, uint32_t *hits,
                                  int mem) {
    if (!index) return kt::fail(KT_ERR_ARG, "kt_ctr_thread_hits: null index");
    kt_ctx *ctx = index->ctx;
    Call call(ctx, mem, "kt_ctr_thread_hits");
    if (int rc = call.enter()) return rc;
    if (int rc = call.refuse_shard(index)) return rc;
    if (n_reads == 0) return KT_OK;
    if (!offsets || !hits) return call.fail("null buffer");
    if (int rc = call.batch(bases, offsets, n_reads)) return rc;
    if (!call.total) return KT_OK;
    if (int rc = table_ready(index)) return rc;
    if (int rc = call.stage()) return rc;
    // (host: the caller's entries go up and come back: what is not written stays as it was)
    uint32_t *d_hits = nullptr;
    if (int rc = call.out(kt::OUT, hits, call.total, &d_hits)) return rc;
    if (int rc = call.up(d_hits, (const uint32_t *)hits, call.total)) return rc;
    SegArgs a;
    if (int rc = make_seg_args(ctx, call.bases, call.offsets, n_reads, call.total, index->k, &a)) return rc;
    HitsArgs c{probed_of(index), d_hits};
    hipLaunchKernelGGL(thread_hits_kernel, dim3(grid_for(ctx, a.n_seg, 8)), dim3(BLOCK), 0, ctx->stream, a, c);
    KT_HIP(hipGetLastError());
    return call.finish();
}


extern "C" int kt_thread_runs(kt_ctx *ctx, const uint32_t *hits, const uint64_t *read_offsets, uint64_t n_reads,
                              const uint64_t *unitig_offsets, uint64_t n_unitigs, int k, uint64_t *run_start, uint32_t *run_len,
                              uint32_t *run_unitig, uint32_t *run_upos, uint64_t *run_offsets, uint64_t max_runs, uint64_t *n_runs,
                              uint64_t *unitig_hits, uint64_t *unitig_runs, uint64_t *tally, int mem) {
    if (!ctx) return kt::fail(KT_ERR_ARG, "kt_thread_runs: null ctx");
    Call call(ctx, mem, "kt_thread_runs");
    if (int rc = call.enter()) return rc;
    if (!n_runs) return call.fail("null n_runs");
    if (k < 1 || k > 31) return call.fail("k must be in 1..31");
    if (n_unitigs > 0x7FFFFFFFull) return call.fail("more than 2^31 - 1 unitigs (2 * unitig + orientation is a u32)");
    if ((n_reads && !read_offsets) || (n_unitigs && !unitig_offsets)) return call.fail("null buffer");
    if (max_runs && (!run_start || !run_len || !run_unitig || !run_upos)) return call.fail("null run array with max_runs > 0");
    hipStream_t st = ctx->stream;
    if (n_reads == 0) {  // no read, no run
        *n_runs = 0;
        if (call.host()) {
            if (run_offsets) run_offsets[0] = 0;
            if (tally)
                for (int q = 0; q < KT_THREAD_TALLY; q++) tally[q] = 0;
        } else {
            if (run_offsets) KT_HIP(hipMemsetAsync(run_offsets, 0, 8, st));
            if (tally) KT_HIP(hipMemsetAsync(tally, 0, KT_THREAD_TALLY * 8, st));
        }
        return KT_OK;
    }
    if (int rc = call.batch(nullptr, read_offsets, n_reads, nullptr)) return rc;
    const uint64_t total = call.total;
    if (total && !hits) return call.fail("null hits");
    if (int rc = call.refuse_long_reads("a run's length is a u32")) return rc;
    uint64_t ub = 0;  // the unitigs' bases
    if (n_unitigs) {
        if (call.host()) {
            ub = unitig_offsets[n_unitigs];
        } else {
            KT_HIP(hipMemcpyAsync(&ub, unitig_offsets + n_unitigs, 8, hipMemcpyDeviceToHost, st));
            KT_HIP(hipStreamSynchronize(st));
        }
    }
    if (ub > 0x7FFFFFFFull) return call.fail("more than 2^31 - 1 unitig bases (a position holds 31 bits of one)");

    // the inputs on the device
    const uint32_t *d_hits = nullptr;
    const uint64_t *d_roff = nullptr;
    if (total)
        if (int rc = call.in(kt::BASES, hits, total, &d_hits)) return rc;
    if (int rc = call.in(kt::OFFSETS, read_offsets, n_reads + 1, &d_roff)) return rc;
    // working arrays: AUX0 = the scan's tiles and the tally, AUX1 = the bit arrays, a host call's unitig offsets and the run
    // offsets when the caller keeps none on the device
    const uint64_t n_items = total + 1, n_tiles = scan2_tiles(n_items);
    const uint64_t uwords = ub / 32 + 1, rwords = total / 32 + 1;
    const bool own_roff = call.host() || !run_offsets;
    const uint64_t n_uoff = call.host() && n_unitigs ? n_unitigs + 1 : 0, n_own = own_roff ? n_reads + 1 : 0;
    uint64_t *tiles = nullptr, *d_tally = nullptr, *d_uoff_w = nullptr, *own = nullptr, *d_run_offsets = run_offsets;
    uint32_t *ubits = nullptr, *rbits = nullptr;
    uint8_t *p = nullptr;
    if (int rc = call.scratch(kt::AUX0, carve_parts<16>(nullptr, &tiles, 2 * n_tiles, &d_tally, (uint64_t)8), &p)) return rc;
    carve_parts<16>(p, &tiles, 2 * n_tiles, &d_tally, (uint64_t)8);
    if (int rc = call.scratch(kt::AUX1, carve_parts<16>(nullptr, &d_uoff_w, n_uoff, &own, n_own, &ubits, uwords, &rbits, rwords), &p))
        return rc;
    carve_parts<16>(p, &d_uoff_w, n_uoff, &own, n_own, &ubits, uwords, &rbits, rwords);
    if (own_roff) d_run_offsets = own;
    const uint64_t *d_uoff = unitig_offsets;
    if (n_uoff) {
        if (int rc = call.up(d_uoff_w, unitig_offsets, n_unitigs + 1)) return rc;
        d_uoff = d_uoff_w;
    }
    KT_HIP(hipMemsetAsync(ubits, k == 1 ? 0 : 0xFF, uwords * 4, st));
    KT_HIP(hipMemsetAsync(rbits, 0, rwords * 4, st));
    KT_HIP(hipMemsetAsync(d_tally, 0, 64, st));
    if (n_unitigs)
        if (int rc = launch(unitig_bits_kernel, dim3(grid_for(ctx, (n_unitigs + BLOCK - 1) / BLOCK, 8)), dim3(BLOCK), 0, st, d_uoff,
                            n_unitigs, (uint32_t)k, ubits))
            return rc;
    if (int rc = launch(read_bits_kernel, dim3(grid_for(ctx, (n_reads + BLOCK) / BLOCK, 8)), dim3(BLOCK), 0, st, d_roff, n_reads, rbits))
        return rc;

    // run starts and run ends, counted: the totals land in the tally ([4] runs; [6] the ends, as many)
    const RunArgs c{d_hits, ubits, rbits, total, ub, (uint32_t)k};
    RunScan scan{c, d_roff, n_reads, nullptr, nullptr, d_run_offsets};
    if (int rc = scan2_sums(st, scan, n_items, tiles, &d_tally[4], &d_tally[6])) return rc;
    uint64_t nr = 0;
    KT_HIP(hipMemcpyAsync(&nr, &d_tally[4], 8, hipMemcpyDeviceToHost, st));
    KT_HIP(hipStreamSynchronize(st));
    *n_runs = nr;
    if (max_runs && max_runs < nr) return call.fail("max_runs is smaller than the number of runs (*n_runs is set)");

    // the outputs: the caller's arrays, or (host) their images in OUT
    const bool write = max_runs != 0;
    uint64_t *d_start = run_start, *d_uh = write ? unitig_hits : nullptr, *d_ur = write ? unitig_runs : nullptr;
    uint32_t *d_len = run_len, *d_unitig = run_unitig, *d_upos = run_upos;
    if (write && call.host()) {
        const uint64_t n_uh = d_uh ? n_unitigs : 0, n_ur = d_ur ? n_unitigs : 0;
        if (int rc = call.scratch(kt::OUT, carve_parts<16>(nullptr, &d_start, nr, &d_uh, n_uh, &d_ur, n_ur, &d_len, nr, &d_unitig, nr, &d_upos, nr), &p))
            return rc;
        carve_parts<16>(p, &d_start, nr, &d_uh, n_uh, &d_ur, n_ur, &d_len, nr, &d_unitig, nr, &d_upos, nr);
        if (!n_uh) d_uh = nullptr;
        if (!n_ur) d_ur = nullptr;
        // (they are added to: the caller's sums go up and come back)
        if (d_uh)
            if (int rc = call.up(d_uh, (const uint64_t *)unitig_hits, n_unitigs)) return rc;
        if (d_ur)
            if (int rc = call.up(d_ur, (const uint64_t *)unitig_runs, n_unitigs)) return rc;
    }
    if (write && nr) {
        scan.run_start = d_start;
        scan.run_last = d_len;
    }
    if (int rc = scan2_apply(st, scan, n_items, tiles)) return rc;
    if (write && nr)
        if (int rc = launch(runs_finish_kernel, dim3(grid_for(ctx, (nr + BLOCK - 1) / BLOCK, 8)), dim3(BLOCK), 0, st, c, d_uoff, n_unitigs,
                            nr, (const uint64_t *)d_start, d_len, d_unitig, d_upos, (unsigned long long *)d_uh, (unsigned long long *)d_ur))
            return rc;
    if (tally) {
        if (total)
            if (int rc = launch(runs_tally_kernel, dim3(grid_for(ctx, (total + BLOCK - 1) / BLOCK, 8)), dim3(BLOCK), 0, st, c,
                                (unsigned long long *)d_tally))
                return rc;
        if (int rc = launch(reads_hit_kernel, dim3(grid_for(ctx, (n_reads + BLOCK - 1) / BLOCK, 8)), dim3(BLOCK), 0, st,
                            (const uint64_t *)d_run_offsets, n_reads, (unsigned long long *)d_tally))
            return rc;
        if (!call.host()) KT_HIP(hipMemcpyAsync(tally, d_tally, KT_THREAD_TALLY * 8, hipMemcpyDeviceToDevice, st));
    }
    if (write) {
        call.back(run_start, (const uint64_t *)d_start, nr);
        call.back(run_len, (const uint32_t *)d_len, nr);
        call.back(run_unitig, (const uint32_t *)d_unitig, nr);
        call.back(run_upos, (const uint32_t *)d_upos, nr);
        call.back(unitig_hits, (const uint64_t *)d_uh, d_uh ? n_unitigs : 0);
        call.back(unitig_runs, (const uint64_t *)d_ur, d_ur ? n_unitigs : 0);
    }
    call.back(run_offsets, (const uint64_t *)d_run_offsets, n_reads + 1);
    call.back(tally, (const uint64_t *)d_tally, (uint64_t)KT_THREAD_TALLY);
    return call.finish();
}
