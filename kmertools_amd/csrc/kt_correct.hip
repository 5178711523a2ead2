// kt_correct.hip - k-mer spectrum error correction of reads against the HBM-resident count table
// (kt_ctr_correct_support, kt_correct_apply; `kmertools correct`).  Nothing in the reference does this.
//
// The rule (include/kmertools_hip.h states it in full): a base is COVERED when a solid window of its read contains it
// and is then never touched; for an uncovered base g and a candidate x, s(g, x) counts the windows of the read that
// contain g, hold no invalid byte elsewhere and whose canonical k-mer, with x written at g, is solid; a base with exactly
// one candidate of s >= min_support is rewritten.  Everything is taken from the uncorrected read, so no order matters.
//
// Three kernels:
//   todo_kernel     one thread per 32 bases: which of them are uncovered bases of a read of at least k bases - from the
//                   caller's profile (kt_ctr_profile's array) and the offsets alone, no probe.  A bit per base in scratch.
//   support_kernel  the probes.  One 256-thread workgroup per 8192-base segment (kt_segment.hpp), window-centric: a window
//                   start of the segment serves the uncovered bases it contains, so only the forward halo is needed.  The
//                   work is sparse and lumpy - most windows contain no uncovered base, one that does costs three probes for
//                   each - so the (window, base) pairs of the segment are compacted: every thread counts the pairs of its 32
//                   window starts from the bit masks alone, a workgroup scan numbers them, they go to an LDS list (in rounds
//                   of LIST when a segment has more) and are dealt to the lanes, PAIRS per lane and round with all their
//                   home-slot loads in flight together (kttab::Probed's home, then count, as kt_cov.hip's probe_windows).  The substituted k-mer is the
//                   window's forward / reverse word with one 2-bit field replaced.  A pair ends in one 32-bit atomic add on
//                   support[g]: byte x gains 1 when candidate x is solid there.
//   apply_*_kernel  the decision, streaming passes over support (+ bases): counts per read and the corrected bytes.  The
//                   read of a base is looked up (ktseg::ReadCursor) only where a candidate is supported.
#include "kt_internal.hpp"
#include "kt_launch.hpp"
#include "kt_segment.hpp"
#include "kt_table.hpp"

#ifndef KT_CORR_PAIRS
#define KT_CORR_PAIRS 3
#endif

namespace {

using ktseg::SegArgs;
using ktseg::SegShared;

constexpr int BLOCK = ktseg::BLOCK;
constexpr uint32_t WAVES = BLOCK / 64;
constexpr uint32_t PAIRS = KT_CORR_PAIRS;  // (window, base) pairs per lane and round: 3 * PAIRS table probes in flight
constexpr uint32_t LIST = 4096;            // pairs of a segment listed in LDS at a time (16 KB)

struct TodoArgs {
    const uint32_t *profile;  // offsets[n_reads] entries
    uint32_t min_count, max_count;
    uint32_t *todo;    // n_words words: bit q of word w = base 32 w + q is an uncovered base of a read of >= k bases
    uint64_t n_words;  // 256 per segment and one more: the halo item of the last segment
};

__device__ __forceinline__ uint64_t solid_bit(uint32_t v, const TodoArgs &c) {
    return (v != KT_NO_KMER && v >= c.min_count && v <= c.max_count) ? 1ull : 0ull;
}

__global__ __launch_bounds__(BLOCK) void todo_kernel(SegArgs a, TodoArgs c) {
    const uint64_t total = a.offsets[a.n_reads];
    const uint32_t k = a.k;
    const bool aligned = ((uintptr_t)c.profile & 15u) == 0;
    for (uint64_t w = (uint64_t)blockIdx.x * BLOCK + threadIdx.x; w < c.n_words; w += (uint64_t)gridDim.x * BLOCK) {
        const uint64_t p0 = 32ull * w;
        uint32_t bits = 0;
        if (p0 < total) {
            // S: bit b = the window that starts at base p0 - 32 + b is solid by the profile (the k - 1 behind, the 32 here)
            uint64_t S = 0;
            const uint32_t back = p0 < k - 1 ? (uint32_t)p0 : k - 1;
            for (uint32_t b = 32 - back; b < 32; b++) S |= solid_bit(c.profile[p0 - 32 + b], c) << b;
            const uint32_t n = total - p0 < 32 ? (uint32_t)(total - p0) : 32u;
            if (n == 32 && aligned) {
#pragma unroll
                for (uint32_t q = 0; q < 32; q += 4) {
                    const uint4 v = *reinterpret_cast<const uint4 *>(c.profile + p0 + q);
                    S |= (solid_bit(v.x, c) | solid_bit(v.y, c) << 1 | solid_bit(v.z, c) << 2 | solid_bit(v.w, c) << 3) << (32 + q);
                }
            } else {
                for (uint32_t q = 0; q < n; q++) S |= solid_bit(c.profile[p0 + q], c) << (32 + q);
            }
            // the read of the first base, then walk forward
            ktseg::ReadCursor rd(a.offsets, a.seg_first, p0 / ktseg::SEG, p0);
            for (uint32_t q = 0; q < n; q++) {
                const uint64_t g = p0 + q;
                rd.advance(g);
                const uint64_t start = rd.start, next = rd.next;
                if (next - start < k) continue;  // (a read shorter than k has no window: nothing to do)
                // the windows of the read that contain g: starts [max(start, g - k + 1), min(g, next - k)]
                uint64_t wl = g + 1 >= k ? g + 1 - k : 0;
                wl = wl > start ? wl : start;
                const uint64_t wh = g < next - k ? g : next - k;
                const uint32_t lb = (uint32_t)(wl + 32 - p0), hb = (uint32_t)(wh + 32 - p0);  // 2 <= lb <= hb <= 63
                const uint64_t m = (~0ull << lb) & (~0ull >> (63u - hb));
                if (!(S & m)) bits |= 1u << q;
            }
        }
        c.todo[w] = bits;
    }
}

struct SupportArgs {
    kttab::Probed t;                // (its hash partition: only the substituted k-mers of that one are looked at)
    const uint32_t *todo;           // todo_kernel's bits
    uint32_t min_count, max_count;  // 1 <= min_count <= max_count
    uint32_t *support;              // offsets[n_reads] entries, added into
};

__global__ __launch_bounds__(BLOCK) void support_kernel(SegArgs a, SupportArgs c) {
    __shared__ SegShared sm;
    __shared__ uint32_t todo[ktseg::NITEM + 1];
    __shared__ uint32_t list[LIST];  // a pair: (window start in the segment) << 5 | offset of the base in the window
    __shared__ uint32_t wave_total[WAVES];
    const uint32_t tid = threadIdx.x;
    const uint32_t k = a.k;
    const uint64_t km = (1ull << k) - 1ull;
    const uint64_t total = a.offsets[a.n_reads];

    for (uint64_t g = blockIdx.x; g < a.n_seg; g += gridDim.x) {
        ktseg::stage_segment(a, g, sm);
        for (uint32_t i = tid; i < ktseg::NITEM; i += BLOCK) todo[i] = c.todo[g * BLOCK + i];
        ktd::lds_barrier();
        const uint64_t B0 = g * ktseg::SEG;
        const uint64_t iv = (uint64_t)sm.inv[tid] | ((uint64_t)sm.inv[tid + 1] << 32);
        const uint64_t bd = (uint64_t)sm.bnd[tid] | ((uint64_t)sm.bnd[tid + 1] << 32);
        const uint64_t td = (uint64_t)todo[tid] | ((uint64_t)todo[tid + 1] << 32);
        // the bases window start jj (0..31) of this thread serves, as a mask of offsets in the window: the uncovered ones when
        // the window lies in one read and holds no invalid byte, the invalid byte itself when it holds exactly one and that
        // one is uncovered (it always is), none otherwise.  (Bases past the batch's end are staged invalid and are not `todo`.)
        auto served = [&](uint32_t jj) -> uint32_t {
            const uint32_t T = (uint32_t)((td >> jj) & km);
            const uint32_t I = (uint32_t)((iv >> jj) & km);
            const uint32_t R = (uint32_t)((bd >> (jj + 1)) & (km >> 1));  // a read starts at window offset 1 .. k - 1
            if (R || !T) return 0u;
            if (!I) return T;
            return (I & (I - 1u)) ? 0u : (T & I);
        };
        uint32_t cnt = 0;
        if (td)
            for (uint32_t jj = 0; jj < ktseg::PER_THREAD; jj++) cnt += (uint32_t)__builtin_popcount(served(jj));
        // number the pairs: this thread's are [first, first + cnt) of the segment's n_pairs
        const uint32_t incl = ktd::wave_incl_scan(cnt);
        if ((tid & 63u) == 63u) wave_total[tid >> 6] = incl;
        ktd::lds_barrier();
        uint32_t first = incl - cnt, n_pairs = 0;
#pragma unroll
        for (uint32_t wv = 0; wv < WAVES; wv++) {
            const uint32_t t = wave_total[wv];
            if (wv < (tid >> 6)) first += t;
            n_pairs += t;
        }

        for (uint32_t r0 = 0; r0 < n_pairs; r0 += LIST) {  // (n_pairs is the same for the whole workgroup)
            if (cnt && first < r0 + LIST && first + cnt > r0) {
                uint32_t idx = first;
                for (uint32_t jj = 0; jj < ktseg::PER_THREAD; jj++) {
                    uint32_t E = served(jj);
                    while (E) {
                        const uint32_t d = (uint32_t)__builtin_ctz(E);
                        E &= E - 1u;
                        if (idx >= r0 && idx - r0 < LIST) list[idx - r0] = ((ktseg::PER_THREAD * tid + jj) << 5) | d;
                        idx++;
                    }
                }
            }
            ktd::lds_barrier();
            const uint32_t n = n_pairs - r0 < LIST ? n_pairs - r0 : LIST;
#pragma unroll 1
            for (uint32_t i0 = 0; i0 < n; i0 += BLOCK * PAIRS) {
                uint64_t key[PAIRS][3];
                uint4 v[PAIRS][3];
                uint32_t e[PAIRS];
                uint64_t f0[PAIRS], r0w[PAIRS];  // the window's words with the base's field cleared
                uint32_t code[PAIRS];            // the base's own code, 4: it is no nucleotide (then all four candidates count)
#pragma unroll
                for (uint32_t u = 0; u < PAIRS; u++) {
                    const uint32_t i = i0 + u * BLOCK + tid;
                    e[u] = i < n ? list[i] : 0u;  // (a lane without a pair computes on pair 0 of the segment and adds nothing)
                    const uint32_t j = e[u] >> 5, d = e[u] & 31u;
                    const uint32_t item = j >> 5, off = j & 31u;
                    const uint64_t hi = sm.codes[item], lo = sm.codes[item + 1];
                    const uint64_t w = off ? (hi << (2u * off)) | (lo >> (64u - 2u * off)) : hi;
                    const uint64_t f = w >> (64u - 2u * k);
                    const uint64_t r = ktd::rev_comp(f, (int)k);
                    const uint32_t sf = 2u * (k - 1u - d), sr = 2u * d;
                    const uint32_t bad = (sm.inv[(j + d) >> 5] >> ((j + d) & 31u)) & 1u;
                    code[u] = bad ? 4u : (uint32_t)(f >> sf) & 3u;
                    f0[u] = f & ~(3ull << sf);
                    r0w[u] = r & ~(3ull << sr);
#pragma unroll
                    for (uint32_t t = 0; t < 3; t++) {
                        const uint32_t x = bad ? t : (code[u] + 1u + t) & 3u;
                        const uint64_t fx = f0[u] | ((uint64_t)x << sf), rx = r0w[u] | ((uint64_t)(3u - x) << sr);
                        key[u][t] = fx < rx ? fx : rx;
                        v[u][t] = c.t.home(key[u][t]);
                    }
                }
#pragma unroll
                for (uint32_t u = 0; u < PAIRS; u++) {
                    if (i0 + u * BLOCK + tid >= n) continue;
                    const uint32_t j = e[u] >> 5, d = e[u] & 31u;
                    uint32_t inc = 0;
                    auto solid = [&](uint64_t key_x, uint4 home) -> uint32_t {
                        if (!c.t.mine(key_x)) return 0u;
                        const uint32_t n_occ = c.t.count(home, key_x);
                        return (n_occ >= c.min_count && n_occ <= c.max_count) ? 1u : 0u;
                    };
#pragma unroll
                    for (uint32_t t = 0; t < 3; t++) {
                        const uint32_t x = code[u] == 4u ? t : (code[u] + 1u + t) & 3u;
                        inc |= solid(key[u][t], v[u][t]) << (8u * x);
                    }
                    if (code[u] == 4u) {  // an N and its like: the fourth candidate, T
                        const uint32_t sf = 2u * (k - 1u - d);
                        const uint64_t fx = f0[u] | (3ull << sf), rx = r0w[u];
                        const uint64_t key_x = fx < rx ? fx : rx;
                        inc |= solid(key_x, c.t.home(key_x)) << 24;
                    }
                    const uint64_t pos = B0 + j + d;
                    if (inc && pos < total) atomicAdd(&c.support[pos], inc);
                }
            }
            ktd::lds_barrier();  // the list is refilled by the next round, sm restaged by the next segment
        }
        ktd::lds_barrier();
    }
}

// ---- the decision (kt_correct_apply) ---------------------------------------------------------------------------------
struct ApplyArgs {
    const uint8_t *bases;
    const uint64_t *offsets;
    const uint64_t *seg_first;  // per 8192 bases: the first read that starts at or behind them (kt_segment.hpp's index)
    uint64_t n_reads, total;
    const uint32_t *support;
    uint32_t min_support, max_corrections;
    uint8_t *out;                     // WRITE
    uint32_t *n_single, *n_ambiguous; // COUNT: added into (either may be null); WRITE with max_corrections: n_single is read
};

// 0: no candidate has min_support, 1 + x: only x has, 5: two or more have
__device__ __forceinline__ uint32_t decide(uint32_t s, uint32_t min_support) {
    if (!s) return 0u;
    uint32_t m = 0;
#pragma unroll
    for (uint32_t x = 0; x < 4; x++) m |= (((s >> (8u * x)) & 255u) >= min_support ? 1u : 0u) << x;
    if (!m) return 0u;
    return (m & (m - 1u)) ? 5u : 1u + (uint32_t)__builtin_ctz(m);
}

// the read that holds base g < offsets[n_reads] (empty reads hold nothing)
__device__ __forceinline__ uint64_t read_of(const ApplyArgs &a, uint64_t g) {
    return ktseg::ReadCursor(a.offsets, a.seg_first, g / ktseg::SEG, g).rid;
}

// n_single[i] / n_ambiguous[i] += the single / ambiguous bases of read i.  One base per lane; a wave whose decided bases all lie
// in one read (the usual case of a long read) adds once per wave.
__global__ __launch_bounds__(BLOCK) void apply_count_kernel(ApplyArgs a) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t step = (uint64_t)gridDim.x * BLOCK;
    // (whole waves stay in the loop together: the ballots below want every lane)
    for (uint64_t g0 = (uint64_t)blockIdx.x * BLOCK + (threadIdx.x & ~63u); g0 < a.total; g0 += step) {
        const uint64_t g = g0 + lane;
        const uint32_t dec = g < a.total ? decide(a.support[g], a.min_support) : 0u;
        const uint64_t any = __ballot(dec != 0u);
        if (!any) continue;
        uint64_t rid = 0;
        if (dec) rid = read_of(a, g);
        const int leader = __ffsll((unsigned long long)any) - 1;
        const uint64_t rid0 = ((uint64_t)(uint32_t)__shfl((int)(uint32_t)(rid >> 32), leader) << 32) | (uint32_t)__shfl((int)(uint32_t)rid, leader);
        const uint64_t amb = __ballot(dec == 5u);
        if (__ballot(dec != 0u && rid == rid0) == any) {
            if ((int)lane == leader) {
                const uint32_t ns = (uint32_t)__popcll(any & ~amb), na = (uint32_t)__popcll(amb);
                if (a.n_single && ns) atomicAdd(&a.n_single[rid0], ns);
                if (a.n_ambiguous && na) atomicAdd(&a.n_ambiguous[rid0], na);
            }
        } else if (dec) {
            uint32_t *dst = dec == 5u ? a.n_ambiguous : a.n_single;
            if (dst) atomicAdd(&dst[rid], 1u);
        }
    }
}

// out[g] = "ACGT"[x] at the single bases of reads within max_corrections (n_single[] complete), bases[g] everywhere else.  Four
// bases per thread: a 16-byte read of support, a dword of bases in and out where the arrays are aligned for it.
__global__ __launch_bounds__(BLOCK) void apply_write_kernel(ApplyArgs a) {
    const bool s_al = ((uintptr_t)a.support & 15u) == 0, b_al = ((uintptr_t)a.bases & 3u) == 0, o_al = ((uintptr_t)a.out & 3u) == 0;
    const uint64_t n_quads = (a.total + 3) / 4;
    for (uint64_t q = (uint64_t)blockIdx.x * BLOCK + threadIdx.x; q < n_quads; q += (uint64_t)gridDim.x * BLOCK) {
        const uint64_t g0 = 4 * q;
        const uint32_t n = a.total - g0 < 4 ? (uint32_t)(a.total - g0) : 4u;
        uint32_t s[4] = {0, 0, 0, 0}, b = 0;
        if (n == 4 && s_al) {
            const uint4 v = *reinterpret_cast<const uint4 *>(a.support + g0);
            s[0] = v.x, s[1] = v.y, s[2] = v.z, s[3] = v.w;
        } else {
            for (uint32_t e = 0; e < n; e++) s[e] = a.support[g0 + e];
        }
        if (n == 4 && b_al) {
            b = *reinterpret_cast<const uint32_t *>(a.bases + g0);
        } else {
            for (uint32_t e = 0; e < n; e++) b |= (uint32_t)a.bases[g0 + e] << (8u * e);
        }
#pragma unroll
        for (uint32_t e = 0; e < 4; e++) {
            const uint32_t dec = decide(s[e], a.min_support);  // (s is 0 past the batch's end)
            if (dec == 0u || dec == 5u) continue;
            if (a.max_corrections && a.n_single[read_of(a, g0 + e)] > a.max_corrections) continue;
            b = (b & ~(255u << (8u * e))) | ((0x54474341u >> (8u * (dec - 1u))) & 255u) << (8u * e);  // "ACGT"
        }
        if (n == 4 && o_al) {
            *reinterpret_cast<uint32_t *>(a.out + g0) = b;
        } else {
            for (uint32_t e = 0; e < n; e++) a.out[g0 + e] = (uint8_t)(b >> (8u * e));
        }
    }
}

}  // namespace

using namespace ktl;

// the support pass over device arrays: d_todo has room for 256 words per segment and one more
static int support_device(kt_ctr *table, kt_ctx *ctx, const uint8_t *d_bases, const uint64_t *d_offsets, uint64_t n_reads,
                          uint64_t total, const uint32_t *d_profile, uint32_t min_count, uint32_t max_count, uint32_t *d_support,
                          uint32_t n_parts, uint32_t part) {
    SegArgs a;
    if (int rc = make_seg_args(ctx, d_bases, d_offsets, n_reads, total, table->k, &a)) return rc;
    const uint64_t n_words = a.n_seg * BLOCK + 1;
    uint32_t *d_todo = nullptr;
    if (int rc = ctx->claim(kt::AUX1, n_words * 4, "kt_ctr_correct_support", &d_todo)) return rc;
    TodoArgs t{d_profile, min_count, max_count, d_todo, n_words};
    hipLaunchKernelGGL(todo_kernel, dim3(grid_for(ctx, (n_words + BLOCK - 1) / BLOCK, 8)), dim3(BLOCK), 0, ctx->stream, a, t);
    KT_HIP(hipGetLastError());
    SupportArgs c{probed_of(table, n_parts, part), d_todo, min_count, max_count, d_support};
    hipLaunchKernelGGL(support_kernel, dim3(grid_for(ctx, a.n_seg, 8)), dim3(BLOCK), 0, ctx->stream, a, c);
    KT_HIP(hipGetLastError());
    return KT_OK;
}

extern "C" int kt_ctr_correct_support(kt_ctr *table, const uint8_t *bases, const uint64_t *offsets, uint64_t n_reads,
                                      const uint32_t *profile, uint32_t min_count, uint32_t max_count, uint32_t *support, int mem,
                                      uint32_t n_parts, uint32_t part) {
    if (!table) return kt::fail(KT_ERR_ARG, "kt_ctr_correct_support: null table");
    if (min_count == 0) return kt::fail(KT_ERR_ARG, "kt_ctr_correct_support: min_count must be >= 1");
    if (min_count > max_count) return kt::fail(KT_ERR_ARG, "kt_ctr_correct_support: min_count > max_count");
    kt_ctx *ctx = table->ctx;
    Call call(ctx, mem, "kt_ctr_correct_support");
    if (int rc = call.check_part(n_parts, part)) return rc;
    if (int rc = call.enter()) return rc;
    if (int rc = call.refuse_shard(table)) return rc;
    if (n_reads == 0) return KT_OK;
    if (!offsets || !profile || !support) return call.fail("null buffer");
    if (int rc = call.batch(bases, offsets, n_reads)) return rc;
    const uint64_t total = call.total;
    if (!total) return KT_OK;
    if (int rc = table_ready(table)) return rc;
    if (int rc = call.stage()) return rc;
    const uint32_t *d_profile = nullptr;
    uint32_t *d_support = support;
    if (int rc = call.in(kt::OUT, profile, total, &d_profile)) return rc;
    if (call.host()) {  // host arrays: this call's support is made on the device from zero and added to the caller's
        if (int rc = call.scratch(kt::AUX2, total * 4, &d_support)) return rc;
        KT_HIP(hipMemsetAsync(d_support, 0, total * 4, ctx->stream));
    }
    if (int rc = support_device(table, ctx, call.bases, call.offsets, n_reads, total, d_profile, min_count, max_count, d_support, n_parts, part))
        return rc;
    if (!call.host()) return KT_OK;
    std::unique_ptr<uint32_t[]> h;
    if (int rc = call.fetch((const uint32_t *)d_support, total, &h)) return rc;
    for (uint64_t i = 0; i < total; i++)
        if (h[i]) support[i] += h[i];
    return KT_OK;
}

// the decision over device arrays; d_single: n_reads entries whenever counts are wanted or max_corrections is set
static int apply_device(kt_ctx *ctx, const uint8_t *d_bases, const uint64_t *d_offsets, uint64_t n_reads, uint64_t total,
                        const uint32_t *d_support, uint32_t min_support, uint32_t max_corrections, uint8_t *d_out, uint32_t *d_single,
                        uint32_t *d_ambiguous) {
    if (d_single) KT_HIP(hipMemsetAsync(d_single, 0, n_reads * 4, ctx->stream));
    if (d_ambiguous) KT_HIP(hipMemsetAsync(d_ambiguous, 0, n_reads * 4, ctx->stream));
    if (!total) return KT_OK;
    SegArgs seg;  // (for its index of the reads by segment alone: read_of)
    if (int rc = make_seg_args(ctx, d_bases, d_offsets, n_reads, total, 1, &seg)) return rc;
    ApplyArgs a{d_bases, d_offsets, seg.seg_first, n_reads, total, d_support, min_support, max_corrections, d_out, d_single, d_ambiguous};
    if (d_single || d_ambiguous)
        hipLaunchKernelGGL(apply_count_kernel, dim3(grid_for(ctx, (total + BLOCK - 1) / BLOCK, 8)), dim3(BLOCK), 0, ctx->stream, a);
    if (d_out)
        hipLaunchKernelGGL(apply_write_kernel, dim3(grid_for(ctx, ((total + 3) / 4 + BLOCK - 1) / BLOCK, 8)), dim3(BLOCK), 0,
                           ctx->stream, a);
    KT_HIP(hipGetLastError());
    return KT_OK;
}

extern "C" int kt_correct_apply(kt_ctx *ctx, const uint8_t *bases, const uint64_t *offsets, uint64_t n_reads, const uint32_t *support,
                                uint32_t min_support, uint32_t max_corrections, uint8_t *out_bases, uint32_t *n_single,
                                uint32_t *n_ambiguous, int mem) {
    if (!ctx) return kt::fail(KT_ERR_ARG, "kt_correct_apply: null ctx");
    if (min_support == 0 || min_support > 255) return kt::fail(KT_ERR_ARG, "kt_correct_apply: min_support must be in 1..255");
    Call call(ctx, mem, "kt_correct_apply");
    if (int rc = call.enter()) return rc;
    if (n_reads == 0) return KT_OK;
    if (!offsets) return call.fail("null buffer");
    if (int rc = call.batch(bases, offsets, n_reads, "null buffer")) return rc;
    const uint64_t total = call.total;
    if (total && !support) return call.fail("null buffer");
    if (int rc = call.refuse_long_reads("the numbers of bases are u32")) return rc;
    if (!out_bases && !n_single && !n_ambiguous) return KT_OK;
    const bool limit = max_corrections != 0 && out_bases;  // the write pass then needs n_single whether the caller wants it or not

    if (!call.host()) {
        uint32_t *d_single = n_single;
        if (!d_single && limit)
            if (int rc = call.scratch(kt::AUX2, n_reads * 4, &d_single)) return rc;
        return apply_device(ctx, bases, offsets, n_reads, total, support, min_support, max_corrections, out_bases, d_single, n_ambiguous);
    }
    // host arrays: staged in ctx scratch, the outputs the caller asked for made there and copied back
    if (int rc = call.stage()) return rc;
    uint32_t *d_support = nullptr, *d_counts = nullptr;  // d_counts: single | ambiguous in one buffer
    uint8_t *d_room = nullptr;
    if (int rc = call.scratch(kt::AUX1, total * 4 + 4, &d_support)) return rc;
    if (int rc = call.scratch(kt::OUT, total + 4, &d_room)) return rc;
    if (int rc = call.scratch(kt::AUX2, n_reads * 8, &d_counts)) return rc;
    uint8_t *d_out = out_bases ? d_room : nullptr;
    uint32_t *d_single = (n_single || limit) ? d_counts : nullptr;
    uint32_t *d_ambiguous = n_ambiguous ? d_counts + n_reads : nullptr;
    if (int rc = call.up(d_support, support, total)) return rc;
    if (int rc = apply_device(ctx, call.bases, call.offsets, n_reads, total, d_support, min_support, max_corrections, d_out, d_single, d_ambiguous))
        return rc;
    call.back(out_bases, (const uint8_t *)d_out, total);
    call.back(n_single, (const uint32_t *)d_single, n_reads);
    call.back(n_ambiguous, (const uint32_t *)d_ambiguous, n_reads);
    return call.finish();
}
