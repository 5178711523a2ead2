// kt_cov.hip - per-read k-mer coverage histograms against the HBM-resident count table.
//
// Replaces CovComputer::vectorise_one (reference coverage/src/lib.rs:165-184): for every
// canonical k-mer of a read, look its count up (0 when absent), bin = min(count / bin_size,
// bin_count - 1), histogram the bins, optionally divide by max(1, #k-mers).  The reference
// re-reads kmers.counts into a host HashMap; here the table built by kt_ctr_add_reads is
// probed where it lies.  HBM-bound random 16-byte reads; no MFMA.
//
// Same segment front-end as the counting kernels.  A thread walks its 32 window starts in groups (probe_windows):
// generate GROUP canonical k-mers, issue their home-slot loads together, then add into a per-segment LDS image
// of the bin rows of the reads that touch the segment (row = read id - first read of the
// segment); the image is flushed with one global atomic per non-zero cell, so a read that
// straddles segments is still summed exactly.  Segments made of very many tiny reads (image
// larger than the LDS budget) add to global memory directly.
//
// The read filter's kt_ctr_read_solidity keeps three numbers per read instead (solidity_kernel), kt_ctr_profile the count
// itself, one u32 per window start (profile_kernel); what is made of those per read - the median among them - is
// kt_profile.hip's.
#include "kt_internal.hpp"
#include "kt_launch.hpp"
#include "kt_probe.hpp"
#include "kt_segment.hpp"
#include "kt_table.hpp"

namespace {

using ktprobe::GROUP;
using ktprobe::probe_windows;  // the probe pipeline (kt_probe.hpp; kt_thread.hip takes the strand from it as well)
using ktseg::SegArgs;
using ktseg::SegShared;
using kttab::Probed;

constexpr int BLOCK = ktseg::BLOCK;
constexpr uint32_t ROWS_LDS = 6144;  // u32 cells of bin rows staged per segment (24 KB)

struct CovArgs {
    Probed t;
    uint32_t bin_size;   // 0 = wider than any u32 count: every k-mer falls in bin 0
    uint32_t bin_count;
    uint32_t *counts;    // n_reads x bin_count, zeroed
    uint32_t shard;      // the table is a shard of a sharded table (1; 2: the first shard - see cov_kernel): the rows are summed over the shards
};

__global__ __launch_bounds__(BLOCK) void cov_kernel(SegArgs a, CovArgs c) {
    __shared__ SegShared sm;
    __shared__ uint32_t rows[ROWS_LDS];
    const uint32_t tid = threadIdx.x;
    for (uint32_t i = tid; i < ROWS_LDS; i += BLOCK) rows[i] = 0;
    const uint32_t last_bin = c.bin_count - 1u;

    for (uint64_t g = blockIdx.x; g < a.n_seg; g += gridDim.x) {
        ktseg::stage_segment(a, g, sm);  // its barriers also order the rows[] zeroing
        ktseg::Window w(sm, tid, a.k);

        // reads that can own a k-mer starting in this segment: [rbase, r_hi)
        const uint64_t r_first = a.seg_first[g];
        const uint64_t r_hi = a.seg_first[g + 1];
        const uint64_t rbase = r_first ? r_first - 1 : 0;  // offsets[rbase] <= g * SEG
        const uint64_t cells = (r_hi - rbase) * (uint64_t)c.bin_count;
        const bool in_lds = cells <= ROWS_LDS;

        if (w.okm) {
            // the read of the thread's first valid window start, then walk forward
            const uint64_t s0 = g * ktseg::SEG + (uint64_t)ktseg::PER_THREAD * tid;
            ktseg::ReadCursor rd(a.offsets, a.seg_first, g, s0 + (uint32_t)__builtin_ctz(w.okm));
            auto add = [&](uint32_t b, uint32_t n) {
                if (in_lds) atomicAdd(&rows[(uint32_t)(rd.rid - rbase) * c.bin_count + b], n);
                else atomicAdd(&c.counts[rd.rid * c.bin_count + b], n);
            };
            probe_windows(c.t, w, [&](uint32_t jj, uint32_t wr, const uint32_t (&cnt)[GROUP]) {
#pragma unroll
                for (uint32_t u = 0; u < GROUP; u++) {
                    if (!((wr >> u) & 1u)) continue;
                    uint32_t bin = c.bin_size ? cnt[u] / c.bin_size : 0u;  // coverage/src/lib.rs:172
                    bin = bin < last_bin ? bin : last_bin;                 // :173
                    rd.advance(s0 + jj + u);
                    if (!c.shard) {
                        add(bin, 1u);
                    } else {
                        // one shard of a table spread over several GPUs by minimiser (kt_shard.hip): a k-mer this shard does
                        // not hold is not "absent" - it may be elsewhere.  Shard 0's pass puts every k-mer into bin 0 (as if
                        // absent everywhere); the one shard that holds a k-mer moves it from there to its bin.  The shards'
                        // rows, summed modulo 2^32 (u32 cells), are the rows of the whole table.
                        if (c.shard == 2u) add(0u, 1u);
                        if (cnt[u] && bin) {
                            add(bin, 1u);
                            add(0u, 0xFFFFFFFFu);
                        }
                    }
                }
            });
        }
        __syncthreads();  // sm is restaged by the next segment; rows[] is complete
        if (in_lds) {
            uint32_t *dst = c.counts + rbase * c.bin_count;
            for (uint32_t i = tid; i < (uint32_t)cells; i += BLOCK) {
                const uint32_t n = rows[i];
                if (n) {
                    atomicAdd(&dst[i], n);
                    rows[i] = 0;
                }
            }
        }
    }
}

// occurrences of keys[i] in the table (0: absent), one thread per key
__global__ __launch_bounds__(BLOCK) void lookup_kernel(Probed t, const uint64_t *__restrict__ keys, uint64_t n,
                                                       uint32_t *__restrict__ out) {
    for (uint64_t i = (uint64_t)blockIdx.x * BLOCK + threadIdx.x; i < n; i += (uint64_t)gridDim.x * BLOCK) {
        const uint64_t key = keys[i];
        out[i] = key == KT_EMPTY_KEY ? 0u : t.count(t.home(key), key);
    }
}

// ---- per-read k-mer solidity (kt_ctr_read_solidity: the read filter) ------------------------------------------------
// Per read only three numbers, each combining with an add or a min: the k-mers, the solid ones (min_count <= count <=
// max_count) and the start in the read of the first weak one.  A thread's 32 window starts
// are consecutive, so it keeps a running (read, n, solid, first weak) in registers and flushes it when the read changes
// and at the end - one flush per read boundary, not one per k-mer.  A flush goes to a per-segment LDS image of the
// segment's reads (3 cells per read: add, add, min), which is flushed with one global atomic per non-default cell.  A
// segment of more than READS_LDS reads (reads below ~32 bases) flushes to global memory directly.
constexpr uint32_t READS_LDS = 256;
constexpr uint32_t NO_POS = 0xFFFFFFFFu;

struct SolidArgs {
    Probed t;
    uint32_t min_count, max_count;  // 1 <= min_count <= max_count: an absent k-mer (count 0) is weak
    uint32_t *n_kmers, *n_solid, *first_weak;  // n_reads each, combined into (first_weak only when FIRST)
};

template <bool FIRST>
__global__ __launch_bounds__(BLOCK) void solidity_kernel(SegArgs a, SolidArgs c) {
    __shared__ SegShared sm;
    __shared__ uint32_t img_n[READS_LDS], img_s[READS_LDS], img_w[READS_LDS];
    const uint32_t tid = threadIdx.x;
    for (uint32_t i = tid; i < READS_LDS; i += BLOCK) {
        img_n[i] = 0;
        img_s[i] = 0;
        img_w[i] = NO_POS;
    }

    for (uint64_t g = blockIdx.x; g < a.n_seg; g += gridDim.x) {
        ktseg::stage_segment(a, g, sm);  // its barriers also order the image's initialisation / reset
        ktseg::Window w(sm, tid, a.k);

        // reads that can own a k-mer starting in this segment: [rbase, r_hi) (as in cov_kernel)
        const uint64_t r_first = a.seg_first[g];
        const uint64_t r_hi = a.seg_first[g + 1];
        const uint64_t rbase = r_first ? r_first - 1 : 0;
        const uint64_t n_img = r_hi - rbase;
        const bool in_lds = n_img <= READS_LDS;

        if (w.okm) {
            const uint64_t s0 = g * ktseg::SEG + (uint64_t)ktseg::PER_THREAD * tid;
            ktseg::ReadCursor rd(a.offsets, a.seg_first, g, s0 + (uint32_t)__builtin_ctz(w.okm));
            // the running read: `run` (~0: none yet), its k-mers, solid k-mers and first weak start seen by this thread
            uint64_t run = ~0ull;
            uint32_t n = 0, sol = 0, weak = NO_POS;
            auto flush = [&]() {
                if (in_lds) {
                    const uint32_t i = (uint32_t)(run - rbase);
                    atomicAdd(&img_n[i], n);
                    if (sol) atomicAdd(&img_s[i], sol);
                    if (FIRST && weak != NO_POS) atomicMin(&img_w[i], weak);
                } else {
                    atomicAdd(&c.n_kmers[run], n);
                    if (sol) atomicAdd(&c.n_solid[run], sol);
                    if (FIRST && weak != NO_POS) atomicMin(&c.first_weak[run], weak);
                }
            };
            probe_windows(c.t, w, [&](uint32_t jj, uint32_t wr, const uint32_t (&cnt)[GROUP]) {
#pragma unroll
                for (uint32_t u = 0; u < GROUP; u++) {
                    if (!((wr >> u) & 1u)) continue;
                    const uint64_t s = s0 + jj + u;
                    rd.advance(s);
                    if (rd.rid != run) {
                        if (run != ~0ull) flush();
                        run = rd.rid;
                        n = sol = 0;
                        weak = NO_POS;
                    }
                    n++;
                    if (cnt[u] >= c.min_count && cnt[u] <= c.max_count) sol++;
                    else if (FIRST && weak == NO_POS) weak = (uint32_t)(s - rd.start);  // starts ascend: the first is the least
                }
            });
            if (run != ~0ull) flush();
        }
        __syncthreads();  // sm is restaged by the next segment; the image is complete
        if (in_lds) {
            for (uint32_t i = tid; i < (uint32_t)n_img; i += BLOCK) {
                const uint32_t nk = img_n[i];
                if (!nk) continue;  // (a read with no k-mer here has no solid or weak one either)
                atomicAdd(&c.n_kmers[rbase + i], nk);
                img_n[i] = 0;
                if (const uint32_t ns = img_s[i]) {
                    atomicAdd(&c.n_solid[rbase + i], ns);
                    img_s[i] = 0;
                }
                if (FIRST) {
                    if (const uint32_t wp = img_w[i]; wp != NO_POS) {
                        atomicMin(&c.first_weak[rbase + i], wp);
                        img_w[i] = NO_POS;
                    }
                }
            }
        }
    }
}

// ---- per-position k-mer counts (kt_ctr_profile) --------------------------------------------------------------------
// The simplest sink there is: the count of the window that starts at global base s goes to profile[s] - no read lookup, no
// LDS image, nothing combined.  Only the valid windows of this hash partition are stored (the caller's fill stays everywhere
// else), so the thread's 32 consecutive entries go out group by group: four at a time as one 16-byte store where all four
// are written and the array is 16-byte aligned, one by one otherwise.
struct ProfileArgs {
    Probed t;
    uint32_t *profile;  // offsets[n_reads] entries, indexed by global base index
};

__global__ __launch_bounds__(BLOCK) void profile_kernel(SegArgs a, ProfileArgs c) {
    __shared__ SegShared sm;
    const uint32_t tid = threadIdx.x;
    const bool aligned = ((uintptr_t)c.profile & 15u) == 0;

    for (uint64_t g = blockIdx.x; g < a.n_seg; g += gridDim.x) {
        ktseg::stage_segment(a, g, sm);
        ktseg::Window w(sm, tid, a.k);
        if (w.okm) {
            // (a valid window lies inside the batch, so every entry written is below offsets[n_reads])
            uint32_t *dst = c.profile + g * ktseg::SEG + (uint64_t)ktseg::PER_THREAD * tid;
            probe_windows(c.t, w, [&](uint32_t jj, uint32_t wr, const uint32_t (&cnt)[GROUP]) {
                auto capped = [&](uint32_t u) { return cnt[u] < KT_NO_KMER ? cnt[u] : KT_NO_KMER - 1u; };  // (the sentinel is no count)
#pragma unroll
                for (uint32_t q = 0; q < GROUP; q += 4) {
                    const uint32_t m = (wr >> q) & 15u;
                    if (m == 15u && aligned) {
                        *reinterpret_cast<uint4 *>(dst + jj + q) = make_uint4(capped(q), capped(q + 1), capped(q + 2), capped(q + 3));
                    } else {
#pragma unroll
                        for (uint32_t u = 0; u < 4; u++)
                            if ((m >> u) & 1u) dst[jj + q + u] = capped(q + u);
                    }
                }
            });
        }
        __syncthreads();  // sm is restaged by the next segment
    }
}

// one thread per read: total = sum of the row, out = count / max(1, total) (:180-182)
template <class T>
__global__ __launch_bounds__(BLOCK) void cov_finalize_kernel(const uint32_t *__restrict__ counts, uint64_t n_reads,
                                                             uint32_t bin_count, int norm, T *__restrict__ out) {
    const uint64_t r = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (r >= n_reads) return;
    const uint32_t *row = counts + r * bin_count;
    T *o = out + r * bin_count;
    double d = 1.0;
    if (norm) {
        uint64_t total = 0;
        for (uint32_t b = 0; b < bin_count; b++) total += row[b];
        d = total > 1 ? (double)total : 1.0;
    }
    for (uint32_t b = 0; b < bin_count; b++) {
        const double x = (double)row[b];
        o[b] = (T)(norm ? x / d : x);
    }
}

}  // namespace

using namespace ktl;

// the lookup pass: u32 bin counts of the reads' k-mers (those of hash partition `part` of n_parts) into d_counts
static int cov_counts(kt_ctr *table, kt_ctx *ctx, const uint8_t *d_bases, const uint64_t *d_offsets, uint64_t n_reads,
                      uint64_t total, uint64_t bin_size, uint64_t bin_count, uint32_t *d_counts, uint32_t n_parts,
                      uint32_t part) {
    if (!total) return KT_OK;
    SegArgs a;
    if (int rc = make_seg_args(ctx, d_bases, d_offsets, n_reads, total, table->k, &a)) return rc;
    CovArgs c{probed_of(table, n_parts, part), bin_size > 0xFFFFFFFFull ? 0u : (uint32_t)bin_size, (uint32_t)bin_count, d_counts,
              table->n_owners > 1 ? (table->owner == 0 ? 2u : 1u) : 0u};
    hipLaunchKernelGGL(cov_kernel, dim3(grid_for(ctx, a.n_seg, 8)), dim3(BLOCK), 0, ctx->stream, a, c);
    KT_HIP(hipGetLastError());
    return KT_OK;
}

extern "C" int kt_cov_batch_part(kt_ctr *table, const uint8_t *bases, const uint64_t *offsets, uint64_t n_reads,
                                 uint64_t bin_size, uint64_t bin_count, uint32_t *counts, int mem, uint32_t n_parts,
                                 uint32_t part) {
    if (!table) return kt::fail(KT_ERR_ARG, "kt_cov_batch_part: null table");
    if (bin_size == 0) return kt::fail(KT_ERR_ARG, "kt_cov_batch_part: bin_size must be >= 1");
    if (bin_count == 0 || bin_count > 0xFFFFFFFFull) return kt::fail(KT_ERR_ARG, "kt_cov_batch_part: bin_count must be in 1..2^32-1");
    kt_ctx *ctx = table->ctx;
    Call call(ctx, mem, "kt_cov_batch_part");
    if (int rc = call.check_part(n_parts, part)) return rc;
    if (int rc = call.enter()) return rc;
    if (n_reads == 0) return KT_OK;
    if (!offsets || !counts) return call.fail("null buffer");
    if (int rc = table_ready(table)) return rc;
    if (int rc = call.batch(bases, offsets, n_reads)) return rc;
    const uint64_t n_cells = n_reads * bin_count;
    uint32_t *d_counts = counts;
    if (call.host()) {  // host rows: this call's counts are made on the device from zero and added to the caller's
        if (call.total)
            if (int rc = call.stage()) return rc;
        if (int rc = call.scratch(kt::AUX1, n_cells * 4, &d_counts)) return rc;
        KT_HIP(hipMemsetAsync(d_counts, 0, n_cells * 4, ctx->stream));
    }
    if (int rc = cov_counts(table, ctx, call.bases, call.offsets, n_reads, call.total, bin_size, bin_count, d_counts, n_parts, part)) return rc;
    if (!call.host()) return KT_OK;
    std::unique_ptr<uint32_t[]> h;
    if (int rc = call.fetch((const uint32_t *)d_counts, n_cells, &h)) return rc;
    for (uint64_t i = 0; i < n_cells; i++) counts[i] += h[i];
    return KT_OK;
}

int ktl::lookup_counts(kt_ctr *table, const uint64_t *d_keys, uint64_t n, uint32_t *d_counts) {
    kt_ctx *ctx = table->ctx;
    hipLaunchKernelGGL(lookup_kernel, dim3(grid_for(ctx, (n + BLOCK - 1) / BLOCK, 8)), dim3(BLOCK), 0, ctx->stream,
                       probed_of(table), d_keys, n, d_counts);
    KT_HIP(hipGetLastError());
    return KT_OK;
}

extern "C" int kt_ctr_lookup(kt_ctr *table, const uint64_t *keys, uint64_t n, uint32_t *counts, int mem) {
    if (!table) return kt::fail(KT_ERR_ARG, "kt_ctr_lookup: null table");
    kt_ctx *ctx = table->ctx;
    Call call(ctx, mem, "kt_ctr_lookup");
    if (int rc = call.enter()) return rc;
    if (n == 0) return KT_OK;
    if (!keys || !counts) return call.fail("null buffer");
    if (int rc = table_ready(table)) return rc;  // (a densely packed table gets its probing image first)
    const uint64_t *d_keys = nullptr;
    uint32_t *d_counts = nullptr;
    if (int rc = call.in(kt::AUX1, keys, n, &d_keys)) return rc;
    if (int rc = call.out(kt::AUX2, counts, n, &d_counts)) return rc;
    if (int rc = lookup_counts(table, d_keys, n, d_counts)) return rc;
    return call.finish();
}

extern "C" int kt_cov_batch(kt_ctr *table, const uint8_t *bases, const uint64_t *offsets, uint64_t n_reads,
                            uint64_t bin_size, uint64_t bin_count, int norm, int out_dtype, void *out, int mem) {
    if (!table) return kt::fail(KT_ERR_ARG, "kt_cov_batch: null table");
    if (bin_size == 0) return kt::fail(KT_ERR_ARG, "kt_cov_batch: bin_size must be >= 1");
    if (bin_count == 0 || bin_count > 0xFFFFFFFFull) return kt::fail(KT_ERR_ARG, "kt_cov_batch: bin_count must be in 1..2^32-1");
    if (out_dtype != KT_F64 && out_dtype != KT_F32 && out_dtype != KT_U32)
        return kt::fail(KT_ERR_ARG, "kt_cov_batch: bad out_dtype");
    if (out_dtype == KT_U32 && norm) return kt::fail(KT_ERR_ARG, "kt_cov_batch: KT_U32 output needs norm = 0");
    kt_ctx *ctx = table->ctx;
    Call call(ctx, mem, "kt_cov_batch");
    if (int rc = call.enter()) return rc;
    if (n_reads == 0) return KT_OK;
    if (!offsets || !out) return call.fail("null buffer");
    if (table->n_owners > 1) return call.fail("the table is one shard of a sharded table - kt_cov_batch_part on every shard, summed");
    if (int rc = table_ready(table)) return rc;
    if (int rc = call.batch(bases, offsets, n_reads)) return rc;

    const uint64_t n_cells = n_reads * bin_count;
    const size_t esz = out_dtype == KT_F64 ? 8 : 4;
    if (call.total)
        if (int rc = call.stage()) return rc;
    char *d_out = nullptr;
    if (int rc = call.out(kt::OUT, (char *)out, n_cells * esz, &d_out)) return rc;
    // u32 bin counts: the output itself for KT_U32, otherwise scratch
    uint32_t *d_counts = (uint32_t *)d_out;
    if (out_dtype != KT_U32)
        if (int rc = call.scratch(kt::AUX1, n_cells * 4, &d_counts)) return rc;
    KT_HIP(hipMemsetAsync(d_counts, 0, n_cells * 4, ctx->stream));
    if (int rc = cov_counts(table, ctx, call.bases, call.offsets, n_reads, call.total, bin_size, bin_count, d_counts, 1, 0)) return rc;
    const uint32_t fb = (uint32_t)((n_reads + BLOCK - 1) / BLOCK);
    if (out_dtype == KT_F64)
        hipLaunchKernelGGL(cov_finalize_kernel<double>, dim3(fb), dim3(BLOCK), 0, ctx->stream, d_counts, n_reads,
                           (uint32_t)bin_count, norm, (double *)d_out);
    else if (out_dtype == KT_F32)
        hipLaunchKernelGGL(cov_finalize_kernel<float>, dim3(fb), dim3(BLOCK), 0, ctx->stream, d_counts, n_reads,
                           (uint32_t)bin_count, norm, (float *)d_out);
    KT_HIP(hipGetLastError());
    return call.finish();
}

// the solidity pass into device arrays (combined into: add, add, min)
static int solidity_counts(kt_ctr *table, kt_ctx *ctx, const uint8_t *d_bases, const uint64_t *d_offsets, uint64_t n_reads,
                           uint64_t total, uint32_t min_count, uint32_t max_count, uint32_t *d_n, uint32_t *d_s, uint32_t *d_w,
                           uint32_t n_parts, uint32_t part) {
    if (!total) return KT_OK;
    SegArgs a;
    if (int rc = make_seg_args(ctx, d_bases, d_offsets, n_reads, total, table->k, &a)) return rc;
    SolidArgs c{probed_of(table, n_parts, part), min_count, max_count, d_n, d_s, d_w};
    if (d_w)
        hipLaunchKernelGGL(solidity_kernel<true>, dim3(grid_for(ctx, a.n_seg, 8)), dim3(BLOCK), 0, ctx->stream, a, c);
    else
        hipLaunchKernelGGL(solidity_kernel<false>, dim3(grid_for(ctx, a.n_seg, 8)), dim3(BLOCK), 0, ctx->stream, a, c);
    KT_HIP(hipGetLastError());
    return KT_OK;
}

extern "C" int kt_ctr_read_solidity(kt_ctr *table, const uint8_t *bases, const uint64_t *offsets, uint64_t n_reads,
                                    uint32_t min_count, uint32_t max_count, uint32_t *n_kmers, uint32_t *n_solid,
                                    uint32_t *first_weak, int mem, uint32_t n_parts, uint32_t part) {
    if (!table) return kt::fail(KT_ERR_ARG, "kt_ctr_read_solidity: null table");
    if (min_count == 0) return kt::fail(KT_ERR_ARG, "kt_ctr_read_solidity: min_count must be >= 1");
    if (min_count > max_count) return kt::fail(KT_ERR_ARG, "kt_ctr_read_solidity: min_count > max_count");
    kt_ctx *ctx = table->ctx;
    Call call(ctx, mem, "kt_ctr_read_solidity");
    if (int rc = call.check_part(n_parts, part)) return rc;
    if (int rc = call.enter()) return rc;
    if (int rc = call.refuse_shard(table)) return rc;
    if (n_reads == 0) return KT_OK;
    if (!offsets || !n_kmers || !n_solid) return call.fail("null buffer");
    if (int rc = call.batch(bases, offsets, n_reads)) return rc;
    if (int rc = call.refuse_long_reads("positions are u32")) return rc;
    if (int rc = table_ready(table)) return rc;
    if (!call.host())
        return solidity_counts(table, ctx, bases, offsets, n_reads, call.total, min_count, max_count, n_kmers, n_solid, first_weak,
                               n_parts, part);
    // host arrays: this call's numbers are made on the device from 0 / 0 / NO_POS and combined into the caller's
    if (!call.total) return KT_OK;
    if (int rc = call.stage()) return rc;
    const uint64_t n_arr = first_weak ? 3 : 2;
    uint32_t *d_n = nullptr;
    if (int rc = call.scratch(kt::AUX1, n_reads * 4 * n_arr, &d_n)) return rc;
    uint32_t *d_s = d_n + n_reads, *d_w = first_weak ? d_s + n_reads : nullptr;
    KT_HIP(hipMemsetAsync(d_n, 0, n_reads * 8, ctx->stream));
    if (d_w) KT_HIP(hipMemsetAsync(d_w, 0xFF, n_reads * 4, ctx->stream));
    if (int rc = solidity_counts(table, ctx, call.bases, call.offsets, n_reads, call.total, min_count, max_count, d_n, d_s, d_w, n_parts, part))
        return rc;
    std::unique_ptr<uint32_t[]> h;
    if (int rc = call.fetch((const uint32_t *)d_n, n_reads * n_arr, &h)) return rc;
    const uint32_t *tn = h.get(), *ts = tn + n_reads, *tw = ts + n_reads;
    for (uint64_t i = 0; i < n_reads; i++) {
        n_kmers[i] += tn[i];
        n_solid[i] += ts[i];
        if (first_weak && tw[i] < first_weak[i]) first_weak[i] = tw[i];
    }
    return KT_OK;
}

extern "C" int kt_ctr_profile(kt_ctr *table, const uint8_t *bases, const uint64_t *offsets, uint64_t n_reads, uint32_t *profile,
                              int mem, uint32_t n_parts, uint32_t part) {
    if (!table) return kt::fail(KT_ERR_ARG, "kt_ctr_profile: null table");
    kt_ctx *ctx = table->ctx;
    Call call(ctx, mem, "kt_ctr_profile");
    if (int rc = call.check_part(n_parts, part)) return rc;
    if (int rc = call.enter()) return rc;
    if (int rc = call.refuse_shard(table)) return rc;
    if (n_reads == 0) return KT_OK;
    if (!offsets || !profile) return call.fail("null buffer");
    if (int rc = call.batch(bases, offsets, n_reads)) return rc;
    if (!call.total) return KT_OK;
    if (int rc = table_ready(table)) return rc;
    if (int rc = call.stage()) return rc;
    // (host: the caller's entries go up and come back: what this part does not write stays as it was)
    uint32_t *d_profile = nullptr;
    if (int rc = call.out(kt::OUT, profile, call.total, &d_profile)) return rc;
    if (int rc = call.up(d_profile, (const uint32_t *)profile, call.total)) return rc;
    SegArgs a;
    if (int rc = make_seg_args(ctx, call.bases, call.offsets, n_reads, call.total, table->k, &a)) return rc;
    ProfileArgs c{probed_of(table, n_parts, part), d_profile};
    hipLaunchKernelGGL(profile_kernel, dim3(grid_for(ctx, a.n_seg, 8)), dim3(BLOCK), 0, ctx->stream, a, c);
    KT_HIP(hipGetLastError());
    return call.finish();
}
