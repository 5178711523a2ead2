// kt_profile.hip - per-sequence statistics of a k-mer count profile (kt_profile_stats): how many k-mers a sequence has, how
// many of them are in the table, the least, the median and the greatest count and their exact sum.
//
// The profile is kt_ctr_profile's array (kt_cov.hip): one u32 per base of a CSR batch, the count of the k-mer that starts
// there, KT_NO_KMER where none does.  Nothing here knows a table or a k - the statistics are a function of that array and
// the offsets, which is what lets the array be filled by several tables in turn (hash partitions) before they are taken.
//
// n, present, min, max and sum are reductions.  The median is element n / 2 of the sequence's counts in ascending order
// (khmer's get_median_count); it is SELECTED, never sorted for, by narrowing a prefix of the answer's bits from the top:
// among the entries that still match the prefix, count those whose next digit is smaller than d for every d; the digit
// whose range holds the wanted rank is the answer's, and the rank is reduced by what lies below it.  KT_NO_KMER entries
// never match a prefix of a count (a count is below 0xFFFFFFFF), so they need no compaction.  Three forms, by the length
// of the sequence in bases (= its entries in the array):
//   <= SHORT_MAX (256)   one wave per sequence, the entries in four registers per lane (stats_wave_kernel<false>).  Digits
//                        of one bit: the count per digit is a ballot and a population count on the scalar unit, and the
//                        walk starts at the top bit of the maximum - six rounds for counts below 64, not 32.
//   <= MID_MAX (2048)    the same wave, the entries in its 8 KB slice of LDS instead (each lane reads back only what it
//                        wrote itself: no barrier) - stats_wave_kernel<true>, launched only when such a sequence exists.
//   longer               digits of eight bits, four passes over the sequence.  A pass cuts the sequence into chunks of
//                        CHUNK entries; a workgroup takes a chunk, histograms the digit of the matching entries in LDS and
//                        adds the non-zero bins to the sequence's 256 global bins (long_hist_kernel); one workgroup per
//                        sequence then scans the bins, fixes the digit and clears them (long_select_kernel).  The chunks of
//                        one sequence go to as many workgroups as there are, so four contigs of 20 Mbases use the whole
//                        device, and ten thousand sequences of 5000 bases do too.  n / present / min / max / sum fall out of
//                        the first pass.
// Which sequence takes which form is a function of its length alone, so every sequence is written by exactly one kernel.
#include "kt_internal.hpp"
#include "kt_launch.hpp"

namespace {

constexpr int BLOCK = 256;
constexpr uint32_t WAVE = 64;
constexpr uint32_t WAVES = BLOCK / WAVE;
constexpr uint32_t SHORT_PER_LANE = 4;
constexpr uint32_t SHORT_MAX = WAVE * SHORT_PER_LANE;  // entries a wave keeps in registers
constexpr uint32_t MID_MAX = 2048;                     // entries a wave keeps in LDS (8 KB; 32 KB per workgroup)
constexpr uint32_t CHUNK = 16384;                      // entries of a long sequence per workgroup and pass
constexpr uint32_t NO = KT_NO_KMER;

struct StatsOut {
    uint32_t *n_kmers, *n_present, *min_count, *median, *max_count;
    uint64_t *sum;
};

// what the classification pass tells the host
struct Classes {
    uint32_t n_long;   // sequences longer than MID_MAX: their indices are list[0 .. n_long)
    uint32_t any_mid;  // a sequence of SHORT_MAX < length <= MID_MAX exists
    uint64_t max_len;  // the longest of the long ones
};

// a long sequence's running numbers between the passes
struct LongAcc {
    uint64_t sum;
    uint32_t n, present, mn, mx;
    uint32_t rank;    // of the median among the entries that match `prefix`
    uint32_t prefix;  // the median's top 8 * (passes done) bits
};

__global__ __launch_bounds__(BLOCK) void classify_kernel(const uint64_t *__restrict__ offsets, uint64_t n_reads, Classes *cls,
                                                         uint64_t *__restrict__ list) {
    const uint32_t lane = threadIdx.x & (WAVE - 1);
    const uint64_t step = (uint64_t)gridDim.x * BLOCK;
    // (whole waves stay in the loop together: the ballots below want every lane)
    for (uint64_t i0 = (uint64_t)blockIdx.x * BLOCK + (threadIdx.x & ~(WAVE - 1)); i0 < n_reads; i0 += step) {
        const uint64_t i = i0 + lane;
        const uint64_t len = i < n_reads ? offsets[i + 1] - offsets[i] : 0;
        const bool is_long = len > MID_MAX;
        const uint64_t mid = __ballot(len > SHORT_MAX && !is_long), lng = __ballot(is_long);
        const uint32_t first_mid = mid ? (uint32_t)__ffsll((unsigned long long)mid) - 1u : WAVE;
        if (lane == first_mid) cls->any_mid = 1u;
        if (lng) {
            const uint32_t leader = (uint32_t)__ffsll((unsigned long long)lng) - 1u;
            uint32_t base = 0;
            if (lane == leader) base = atomicAdd(&cls->n_long, (uint32_t)__popcll(lng));
            base = (uint32_t)__shfl((int)base, (int)leader);
            if (is_long) {
                list[base + (uint32_t)__popcll(lng & ((1ull << lane) - 1ull))] = i;
                atomicMax((unsigned long long *)&cls->max_len, (unsigned long long)len);
            }
        }
    }
}

// One wave per sequence of at most SHORT_MAX (MID = false) / of SHORT_MAX + 1 .. MID_MAX (MID = true) entries.
template <bool MID>
__global__ __launch_bounds__(BLOCK) void stats_wave_kernel(const uint32_t *__restrict__ profile, const uint64_t *__restrict__ offsets,
                                                           uint64_t n_reads, StatsOut o) {
    __shared__ uint32_t lds[MID ? WAVES * MID_MAX : 1];
    const uint32_t lane = threadIdx.x & (WAVE - 1), wv = threadIdx.x / WAVE;
    uint32_t *mine = lds + (MID ? wv * MID_MAX : 0);
    for (uint64_t i = (uint64_t)blockIdx.x * WAVES + wv; i < n_reads; i += (uint64_t)gridDim.x * WAVES) {
        const uint64_t o0 = offsets[i], len = offsets[i + 1] - o0;
        if (MID ? (len <= SHORT_MAX || len > MID_MAX) : (len > SHORT_MAX)) continue;
        const uint32_t L = (uint32_t)len;
        const uint32_t *src = profile + o0;
        const uint32_t E = MID ? (L + WAVE - 1) / WAVE : SHORT_PER_LANE;
        uint32_t x[SHORT_PER_LANE];
        uint32_t n = 0, pres = 0, mn = NO, mx = 0;
        uint64_t sum = 0;
        auto take = [&](uint32_t v) {
            const bool valid = v != NO;
            n += (uint32_t)__popcll(__ballot(valid));
            pres += (uint32_t)__popcll(__ballot(valid && v != 0));
            if (valid) {
                mn = min(mn, v);
                mx = max(mx, v);
                sum += v;
            }
        };
        if constexpr (MID) {
            for (uint32_t e = 0; e < E; e++) {
                const uint32_t idx = lane + WAVE * e;
                const uint32_t v = idx < L ? src[idx] : NO;
                mine[idx] = v;
                take(v);
            }
        } else {
#pragma unroll
            for (uint32_t e = 0; e < SHORT_PER_LANE; e++) {
                const uint32_t idx = lane + WAVE * e;
                x[e] = idx < L ? src[idx] : NO;
            }
#pragma unroll
            for (uint32_t e = 0; e < SHORT_PER_LANE; e++) take(x[e]);
        }
        mx = ktd::wave_all_max(mx);
        uint32_t med = 0;
        if (o.median && n && mx) {
            // one bit per round from the top bit of the maximum down: entries that match the prefix and have a 0 next
            uint32_t r = n / 2, prefix = 0;
            for (int b = 31 - __builtin_clz(mx); b >= 0; b--) {
                const uint32_t m = ~0u << b;
                uint32_t c0 = 0;
                if constexpr (MID) {
                    for (uint32_t e = 0; e < E; e++) c0 += (uint32_t)__popcll(__ballot((mine[lane + WAVE * e] & m) == prefix));
                } else {
#pragma unroll
                    for (uint32_t e = 0; e < SHORT_PER_LANE; e++) c0 += (uint32_t)__popcll(__ballot((x[e] & m) == prefix));
                }
                if (r >= c0) {
                    r -= c0;
                    prefix |= 1u << b;
                }
            }
            med = prefix;
        }
        if (o.min_count) mn = ktd::wave_all_min(mn);
        if (o.sum) sum = ktd::wave_all_sum<uint64_t>(sum);
        if (lane == 0) {
            if (o.n_kmers) o.n_kmers[i] = n;
            if (o.n_present) o.n_present[i] = pres;
            if (o.min_count) o.min_count[i] = n ? mn : 0u;
            if (o.median) o.median[i] = med;
            if (o.max_count) o.max_count[i] = mx;
            if (o.sum) o.sum[i] = sum;
        }
    }
}

__global__ __launch_bounds__(BLOCK) void long_init_kernel(LongAcc *acc, uint32_t n_long) {
    const uint32_t j = blockIdx.x * BLOCK + threadIdx.x;
    if (j < n_long) acc[j] = LongAcc{0, 0, 0, NO, 0, 0, 0};
}

// pass PASS of the long form: the 8-bit digit below the PASS * 8 bits already fixed, histogrammed over the entries that match
// them; blockIdx.y strides over the long sequences, blockIdx.x over the chunks of one
template <int PASS>
__global__ __launch_bounds__(BLOCK) void long_hist_kernel(const uint32_t *__restrict__ profile, const uint64_t *__restrict__ offsets,
                                                          const uint64_t *__restrict__ list, uint32_t n_long, LongAcc *acc,
                                                          uint32_t *hist) {
    __shared__ uint32_t h[256];
    const uint32_t tid = threadIdx.x, lane = tid & (WAVE - 1);
    constexpr uint32_t SH = 24 - 8 * PASS;  // the digit's shift
    for (uint32_t j = blockIdx.y; j < n_long; j += gridDim.y) {
        const uint64_t i = list[j];
        const uint64_t o0 = offsets[i], len = offsets[i + 1] - o0;
        const uint64_t n_chunks = (len + CHUNK - 1) / CHUNK;
        uint32_t prefix = 0;
        if (PASS > 0) {
            if (acc[j].n == 0) continue;  // (no k-mer: nothing to select)
            prefix = acc[j].prefix;
        }
        for (uint64_t c = blockIdx.x; c < n_chunks; c += gridDim.x) {
            h[tid] = 0;
            __syncthreads();
            const uint32_t *src = profile + o0 + c * CHUNK;
            const uint64_t left = len - c * CHUNK;
            const uint32_t m = left < CHUNK ? (uint32_t)left : CHUNK;
            uint32_t n = 0, pres = 0, mn = NO, mx = 0;
            uint64_t sum = 0;
            for (uint32_t e = 0; e < CHUNK; e += BLOCK) {  // (the same trip count for every lane: the ballots want them all)
                if (e >= m) break;
                const uint32_t idx = e + tid;
                const uint32_t v = idx < m ? src[idx] : NO;
                bool act = v != NO;
                if constexpr (PASS == 0) {
                    if (act) {
                        n++;
                        pres += v != 0;
                        mn = min(mn, v);
                        mx = max(mx, v);
                        sum += v;
                    }
                } else {
                    act = act && (v >> (SH + 8)) == prefix;
                }
                // neighbouring k-mers have like counts, and most counts are small: the usual wave agrees on its digit
                const uint32_t d = (v >> SH) & 255u;
                const uint64_t am = __ballot(act);
                if (am) {
                    const uint32_t leader = (uint32_t)__ffsll((unsigned long long)am) - 1u;
                    const uint32_t d0 = (uint32_t)__shfl((int)d, (int)leader);
                    if (__ballot(act && d == d0) == am) {
                        if (lane == leader) atomicAdd(&h[d0], (uint32_t)__popcll(am));
                    } else if (act) {
                        atomicAdd(&h[d], 1u);
                    }
                }
            }
            __syncthreads();
            if (const uint32_t v = h[tid]) atomicAdd(&hist[(uint64_t)j * 256 + tid], v);
            if (PASS == 0) {
                n = (uint32_t)ktd::wave_all_sum<uint64_t>(n);
                if (n) {  // (wave-uniform)
                    pres = (uint32_t)ktd::wave_all_sum<uint64_t>(pres);
                    mn = ktd::wave_all_min(mn);
                    mx = ktd::wave_all_max(mx);
                    sum = ktd::wave_all_sum<uint64_t>(sum);
                    if (lane == 0) {
                        atomicAdd(&acc[j].n, n);
                        if (pres) atomicAdd(&acc[j].present, pres);
                        atomicMin(&acc[j].mn, mn);
                        atomicMax(&acc[j].mx, mx);
                        atomicAdd((unsigned long long *)&acc[j].sum, (unsigned long long)sum);
                    }
                }
            }
            __syncthreads();  // h[] is cleared for the next chunk
        }
    }
}

// behind pass PASS: the digit whose bins hold the wanted rank joins the prefix; the bins are cleared for the next pass.  The
// first one writes what the first pass reduced, the last one the median.
template <int PASS>
__global__ __launch_bounds__(BLOCK) void long_select_kernel(const uint64_t *__restrict__ list, uint32_t n_long, LongAcc *acc,
                                                            uint32_t *hist, StatsOut o) {
    __shared__ uint32_t sc[2][256];
    const uint32_t tid = threadIdx.x;
    for (uint32_t j = blockIdx.x; j < n_long; j += gridDim.x) {
        const uint64_t i = list[j];
        const LongAcc a = acc[j];
        const uint32_t v = hist[(uint64_t)j * 256 + tid];
        hist[(uint64_t)j * 256 + tid] = 0;
        const uint32_t r = PASS == 0 ? a.n / 2 : a.rank;
        // inclusive scan of the 256 bins (a sequence has fewer than 2^32 entries: no overflow)
        uint32_t incl = v;
        int cur = 0;
        sc[0][tid] = incl;
        __syncthreads();
        for (uint32_t d = 1; d < 256; d <<= 1) {
            if (tid >= d) incl += sc[cur][tid - d];
            cur ^= 1;
            sc[cur][tid] = incl;
            __syncthreads();
        }
        if (a.n && v && incl - v <= r && r < incl) {  // exactly one bin
            const uint32_t prefix = (a.prefix << 8) | tid;
            acc[j].rank = r - (incl - v);
            acc[j].prefix = prefix;
            if (PASS == 3 && o.median) o.median[i] = prefix;
        }
        if (PASS == 0 && tid == 0) {
            if (o.n_kmers) o.n_kmers[i] = a.n;
            if (o.n_present) o.n_present[i] = a.present;
            if (o.min_count) o.min_count[i] = a.n ? a.mn : 0u;
            if (o.max_count) o.max_count[i] = a.mx;
            if (o.sum) o.sum[i] = a.sum;
            if (o.median && !a.n) o.median[i] = 0;
        }
        __syncthreads();  // sc[] is reused by the next sequence
    }
}

}  // namespace

using namespace ktl;

// the statistics of a device-resident profile into device arrays (any of them null)
static int stats_device(kt_ctx *ctx, const uint32_t *profile, const uint64_t *offsets, uint64_t n_reads, uint64_t total,
                        const StatsOut &o) {
    // which forms are needed: the long sequences' indices (at most total / (MID_MAX + 1) of them), whether a middle one exists
    const uint64_t list_cap = total / (MID_MAX + 1) + 1;
    Classes *d_cls = nullptr;
    if (int rc = ctx->claim(kt::AUX1, sizeof(Classes) + list_cap * 8, "kt_profile_stats", &d_cls)) return rc;
    uint64_t *d_list = (uint64_t *)(d_cls + 1);
    Classes cls{};
    KT_HIP(hipMemsetAsync(d_cls, 0, sizeof(Classes), ctx->stream));
    hipLaunchKernelGGL(classify_kernel, dim3(grid_for(ctx, (n_reads + BLOCK - 1) / BLOCK, 8)), dim3(BLOCK), 0, ctx->stream, offsets,
                       n_reads, d_cls, d_list);
    KT_HIP(hipGetLastError());
    KT_HIP(hipMemcpyAsync(&cls, d_cls, sizeof(Classes), hipMemcpyDeviceToHost, ctx->stream));
    // (the short form does not wait for the answer)
    hipLaunchKernelGGL(stats_wave_kernel<false>, dim3(grid_for(ctx, (n_reads + WAVES - 1) / WAVES, 8)), dim3(BLOCK), 0, ctx->stream,
                       profile, offsets, n_reads, o);
    KT_HIP(hipGetLastError());
    KT_HIP(hipStreamSynchronize(ctx->stream));
    if (cls.any_mid) {
        hipLaunchKernelGGL(stats_wave_kernel<true>, dim3(grid_for(ctx, (n_reads + WAVES - 1) / WAVES, 5)), dim3(BLOCK), 0, ctx->stream,
                           profile, offsets, n_reads, o);
        KT_HIP(hipGetLastError());
    }
    if (!cls.n_long) return KT_OK;

    const uint32_t n_long = cls.n_long;
    LongAcc *d_acc = nullptr;
    if (int rc = ctx->claim(kt::AUX2, (uint64_t)n_long * (sizeof(LongAcc) + 256 * 4), "kt_profile_stats", &d_acc)) return rc;
    uint32_t *d_hist = (uint32_t *)(d_acc + n_long);
    KT_HIP(hipMemsetAsync(d_hist, 0, (uint64_t)n_long * 256 * 4, ctx->stream));
    hipLaunchKernelGGL(long_init_kernel, dim3((n_long + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, ctx->stream, d_acc, n_long);
    const uint32_t wgs = (uint32_t)ctx->n_cu * 8u;
    const uint64_t chunks = (cls.max_len + CHUNK - 1) / CHUNK;
    const uint32_t gx = (uint32_t)(chunks < wgs ? chunks : wgs);
    uint32_t gy = wgs / gx ? wgs / gx : 1u;
    if (gy > n_long) gy = n_long;
    if (gy > 65535u) gy = 65535u;
    const dim3 hg(gx, gy), sg(n_long < wgs ? n_long : wgs);
#define KT_LONG_PASS(P)                                                                                                         \
    hipLaunchKernelGGL(long_hist_kernel<P>, hg, dim3(BLOCK), 0, ctx->stream, profile, offsets, d_list, n_long, d_acc, d_hist);  \
    hipLaunchKernelGGL(long_select_kernel<P>, sg, dim3(BLOCK), 0, ctx->stream, d_list, n_long, d_acc, d_hist, o);
    KT_LONG_PASS(0)
    if (o.median) {
        KT_LONG_PASS(1)
        KT_LONG_PASS(2)
        KT_LONG_PASS(3)
    }
#undef KT_LONG_PASS
    KT_HIP(hipGetLastError());
    return KT_OK;
}

extern "C" int kt_profile_stats(kt_ctx *ctx, const uint32_t *profile, const uint64_t *offsets, uint64_t n_reads, uint32_t *n_kmers,
                                uint32_t *n_present, uint32_t *min_count, uint32_t *median, uint32_t *max_count, uint64_t *sum,
                                int mem) {
    if (!ctx) return kt::fail(KT_ERR_ARG, "kt_profile_stats: null ctx");
    Call call(ctx, mem, "kt_profile_stats");
    if (int rc = call.enter()) return rc;
    if (n_reads == 0) return KT_OK;
    if (!offsets) return call.fail("null buffer");
    if (int rc = call.batch(nullptr, offsets, n_reads, nullptr)) return rc;
    const uint64_t total = call.total;
    if (total && !profile) return call.fail("null profile");
    if (int rc = call.refuse_long_reads("the numbers of k-mers are u32")) return rc;
    uint32_t *const out32[5] = {n_kmers, n_present, min_count, median, max_count};
    if (!n_kmers && !n_present && !min_count && !median && !max_count && !sum) return KT_OK;

    if (!call.host()) return stats_device(ctx, profile, offsets, n_reads, total, StatsOut{n_kmers, n_present, min_count, median, max_count, sum});

    // host arrays: the profile in BASES, the offsets in OFFSETS, sum | the five u32 outputs in OUT
    uint32_t *d_profile = nullptr;
    const uint64_t *d_offsets = nullptr;
    uint64_t *d_sum = nullptr;
    if (int rc = call.scratch(kt::BASES, total * 4 + 4, &d_profile)) return rc;
    if (int rc = call.in(kt::OFFSETS, offsets, n_reads + 1, &d_offsets)) return rc;
    if (int rc = call.scratch(kt::OUT, n_reads * (8 + 5 * 4), &d_sum)) return rc;
    if (int rc = call.up(d_profile, profile, total)) return rc;
    uint32_t *d32 = (uint32_t *)(d_sum + n_reads);
    StatsOut o{n_kmers ? d32 : nullptr,
               n_present ? d32 + n_reads : nullptr,
               min_count ? d32 + 2 * n_reads : nullptr,
               median ? d32 + 3 * n_reads : nullptr,
               max_count ? d32 + 4 * n_reads : nullptr,
               sum ? d_sum : nullptr};
    if (int rc = stats_device(ctx, d_profile, d_offsets, n_reads, total, o)) return rc;
    for (int q = 0; q < 5; q++) call.back(out32[q], (const uint32_t *)d32 + (uint64_t)q * n_reads, n_reads);
    call.back(sum, (const uint64_t *)d_sum, n_reads);
    return call.finish();
}
