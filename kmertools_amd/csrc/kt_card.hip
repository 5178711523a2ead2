// kt_card.hip - HyperLogLog registers of the distinct canonical k-mers of a CSR batch (kt_card_add_reads) and what the host
// does with such registers: the register-wise max of two arrays (kt_card_merge), Ertl's improved raw estimator
// (kt_card_estimate) and the estimator's relative standard error (kt_card_rel_error).
//
// m = 2^p registers of one byte, q = 64 - p.  A window's hash is h = mix64(canonical k-mer ^ seed) (kt_sketch_batch's), its
// register j = h >> q, its rank r = 1 + the leading zeros of the low q bits of h taken as a q-bit word (q + 1 when they are
// all zero), and registers[j] = max(registers[j], r).  Max does not care about order, so the registers are a function of
// the input alone, and adding a batch in pieces, in any order, gives what one call with all of it gives.
//
//   card_kernel          a persistent grid over the 8192-base segments of the ktseg front end.  Every workgroup keeps a
//                        whole register array in LDS (m bytes of dynamic LDS next to SegShared: 64 KiB at p = 16), four
//                        registers to a word.  A k-mer reads its register first and leaves when it already holds r or
//                        more - a register is raised at most q + 1 times, so after the first segments nearly every k-mer
//                        leaves here.  A raise is a compare-and-swap of the word: the lane that loses takes the word the
//                        winner left and tests its byte again, so the loop ends as soon as the byte is >= r, and of the
//                        lanes that swap the same word one wins in every round (64 lanes on one register, poly-A input:
//                        the first swap wins, the other 63 find their byte raised and leave).  At the end the workgroup
//                        writes its array to row blockIdx.x of a slab [grid][m] and adds its windows, summed per wave,
//                        to *n_kmers once.
//   card_combine_kernel  the column-wise max of the slab's rows, combined into the caller's registers byte by byte (the
//                        caller's array may lie at any address).
// The slab, not global atomics: an atomicMax wants 32-bit cells, which is 4 m bytes of internal array to zero, raise and
// pack again per call and one atomic per raise per workgroup on 2^p hot words; the slab is written once with whole-line
// stores and read once (32 MiB at p = 16 on a 512-workgroup grid), and the combine step is the only place that touches the
// caller's memory.
#include <math.h>

#include "kt_internal.hpp"
#include "kt_launch.hpp"

namespace {

using ktseg::SegArgs;
using ktseg::SegShared;
constexpr uint32_t BLOCK = ktseg::BLOCK;
constexpr uint32_t WAVE = 64;
constexpr uint32_t LDS_PER_CU = 160u << 10;

// per-byte max of two words of four registers
__device__ __forceinline__ uint32_t max4(uint32_t a, uint32_t b) {
    uint32_t r = 0;
#pragma unroll
    for (uint32_t s = 0; s < 32; s += 8) {
        const uint32_t x = (a >> s) & 0xFFu, y = (b >> s) & 0xFFu;
        r |= (x > y ? x : y) << s;
    }
    return r;
}

__global__ __launch_bounds__(BLOCK) void card_kernel(SegArgs a, uint64_t seed, uint32_t p, uint32_t *__restrict__ slab,
                                                     unsigned long long *n_kmers) {
    extern __shared__ uint32_t regs[];  // m / 4 words
    __shared__ SegShared sm;
    __shared__ uint32_t wg_kmers[2];    // the workgroup's windows, low and high word
    const uint32_t tid = threadIdx.x, words = (1u << p) >> 2, q = 64u - p;
    for (uint32_t i = tid; i < words; i += BLOCK) regs[i] = 0;
    if (tid < 2) wg_kmers[tid] = 0;
    // (the staging barriers of the first segment order this initialisation before the first update)

    uint64_t mine = 0;  // windows this thread has seen
    for (uint64_t g = blockIdx.x; g < a.n_seg; g += gridDim.x) {
        ktseg::for_each_kmer(a, g, sm, [&](uint64_t f, uint64_t r, uint64_t) {
            mine++;
            const uint64_t h = ktd::mix64((f < r ? f : r) ^ seed);
            const uint32_t j = (uint32_t)(h >> q);
            // the low q bits on top, a one right below them: the leading zeros stop at q
            const uint32_t rank = 1u + (uint32_t)__builtin_clzll((h << p) | (1ull << (p - 1)));
            const uint32_t sh = (j & 3u) * 8u;
            uint32_t *wp = &regs[j >> 2];
            uint32_t cur = __atomic_load_n(wp, __ATOMIC_RELAXED);
            while (((cur >> sh) & 0xFFu) < rank) {
                const uint32_t old = atomicCAS(wp, cur, (cur & ~(0xFFu << sh)) | (rank << sh));
                if (old == cur) break;
                cur = old;
            }
        });
    }

    // windows: per wave, then once per workgroup
    mine = ktd::wave_sum(mine);
    if ((tid & (WAVE - 1)) == 0 && mine) {
        const uint32_t lo = (uint32_t)mine;
        const uint32_t before = atomicAdd(&wg_kmers[0], lo);
        atomicAdd(&wg_kmers[1], (uint32_t)(mine >> 32) + (before + lo < before ? 1u : 0u));
    }
    ktd::lds_barrier();  // every update and every wave's count is in
    uint32_t *row = slab + (uint64_t)blockIdx.x * words;
    for (uint32_t i = tid; i < words; i += BLOCK) row[i] = regs[i];
    if (tid == 0 && n_kmers) {
        const uint64_t n = ((uint64_t)wg_kmers[1] << 32) | wg_kmers[0];
        if (n) atomicAdd(n_kmers, (unsigned long long)n);
    }
}

// registers[4 w .. 4 w + 4) = max(themselves, column w of the slab's rows).  A workgroup takes `wpb` words (a power of two,
// at most 64) and deals the rows to its BLOCK / wpb thread rows; LDS brings the thread rows together.
__global__ __launch_bounds__(BLOCK) void card_combine_kernel(const uint32_t *__restrict__ slab, uint32_t rows, uint32_t words,
                                                             uint32_t wpb, uint8_t *registers) {
    __shared__ uint32_t part[BLOCK];
    const uint32_t tid = threadIdx.x, col = tid & (wpb - 1), lane_row = tid / wpb, lane_rows = BLOCK / wpb;
    const uint32_t w = blockIdx.x * wpb + col;  // (words is a multiple of wpb: both are powers of two, wpb <= words)
    uint32_t acc = 0;
    for (uint32_t r = lane_row; r < rows; r += lane_rows) acc = max4(acc, slab[(uint64_t)r * words + w]);
    part[tid] = acc;
    __syncthreads();
    if (lane_row) return;
    for (uint32_t r = 1; r < lane_rows; r++) acc = max4(acc, part[r * wpb + col]);
    uint8_t *out = registers + 4ull * w;
#pragma unroll
    for (uint32_t b = 0; b < 4; b++) {
        const uint8_t v = (uint8_t)(acc >> (8 * b));
        if (v > out[b]) out[b] = v;
    }
}

// Ertl's helper series (New cardinality estimation algorithms for HyperLogLog sketches, 2017), as Redis evaluates them
double card_sigma(double x) {
    if (x == 1.0) return INFINITY;
    double y = 1.0, z = x, zp;
    do {
        x *= x;
        zp = z;
        z += x * y;
        y += y;
    } while (zp != z);
    return z;
}

double card_tau(double x) {
    if (x == 0.0 || x == 1.0) return 0.0;
    double y = 1.0, z = 1.0 - x, zp;
    do {
        x = sqrt(x);
        zp = z;
        y *= 0.5;
        z -= (1.0 - x) * (1.0 - x) * y;
    } while (zp != z);
    return z / 3.0;
}

bool card_bad_p(int p) { return p < KT_CARD_MIN_P || p > KT_CARD_MAX_P; }

}  // namespace

using namespace ktl;

extern "C" int kt_card_add_reads(kt_ctx *ctx, const uint8_t *bases, const uint64_t *offsets, uint64_t n_reads, int k, int p,
                                 uint64_t seed, uint8_t *registers, uint64_t *n_kmers, int mem) {
    if (!ctx) return kt::fail(KT_ERR_ARG, "kt_card_add_reads: null ctx");
    if (k < 1 || k > 31) return kt::fail(KT_ERR_ARG, "kt_card_add_reads: k must be in 1..31");
    if (card_bad_p(p)) return kt::fail(KT_ERR_ARG, "kt_card_add_reads: p must be in KT_CARD_MIN_P..KT_CARD_MAX_P");
    Call call(ctx, mem, "kt_card_add_reads");
    if (int rc = call.enter()) return rc;
    if (n_reads == 0) return KT_OK;
    if (!offsets || !registers) return call.fail("null buffer");
    if (int rc = call.batch(bases, offsets, n_reads)) return rc;
    if (int rc = call.refuse_long_reads("the walk's positions in a read are u32")) return rc;
    if (!call.total) return KT_OK;
    if (int rc = call.stage()) return rc;

    const uint32_t m = 1u << p, words = m / 4;
    uint8_t *d_regs = registers;
    unsigned long long *d_n = (unsigned long long *)n_kmers;
    if (call.host()) {  // registers | n_kmers in one buffer: the caller's values go up, are combined into and come back
        if (int rc = call.scratch(kt::OUT, m + 8, &d_regs)) return rc;
        if (int rc = call.up(d_regs, (const uint8_t *)registers, m)) return rc;
        call.back(registers, (const uint8_t *)d_regs, m);
        if (n_kmers) {
            d_n = (unsigned long long *)(d_regs + m);
            if (int rc = call.up((uint64_t *)d_n, (const uint64_t *)n_kmers, 1)) return rc;
            call.back(n_kmers, (const uint64_t *)d_n, 1);
        }
    }
    SegArgs a;
    if (int rc = make_seg_args(ctx, call.bases, call.offsets, n_reads, call.total, k, &a)) return rc;
    // workgroups a CU holds: the register array and the staged segment in LDS, at most 8 of 4 waves (32 waves per CU)
    uint32_t per_cu = LDS_PER_CU / (m + (uint32_t)sizeof(SegShared) + 512u);
    per_cu = per_cu > 8 ? 8 : per_cu;
    const uint32_t grid = grid_for(ctx, a.n_seg, per_cu);
    uint32_t *slab = nullptr;
    if (int rc = call.scratch(kt::AUX1, (size_t)grid * m, &slab)) return rc;
    if (int rc = launch(card_kernel, dim3(grid), dim3(BLOCK), m, ctx->stream, a, seed, (uint32_t)p, slab, d_n)) return rc;
    const uint32_t wpb = words < 64 ? words : 64;
    if (int rc = launch(card_combine_kernel, dim3(words / wpb), dim3(BLOCK), 0, ctx->stream, (const uint32_t *)slab, grid, words, wpb,
                        d_regs))
        return rc;
    return call.finish();
}

extern "C" int kt_card_merge(uint8_t *into, const uint8_t *from, int p) {
    if (card_bad_p(p)) return kt::fail(KT_ERR_ARG, "kt_card_merge: p must be in KT_CARD_MIN_P..KT_CARD_MAX_P");
    if (!into || !from) return kt::fail(KT_ERR_ARG, "kt_card_merge: null buffer");
    for (uint32_t j = 0; j < (1u << p); j++)
        if (from[j] > into[j]) into[j] = from[j];
    return KT_OK;
}

extern "C" int kt_card_estimate(const uint8_t *registers, int p, double *estimate, uint64_t *zero_registers) {
    if (card_bad_p(p)) return kt::fail(KT_ERR_ARG, "kt_card_estimate: p must be in KT_CARD_MIN_P..KT_CARD_MAX_P");
    if (!registers || !estimate) return kt::fail(KT_ERR_ARG, "kt_card_estimate: null buffer");
    const uint32_t m = 1u << p, q = 64u - (uint32_t)p;
    uint64_t C[64 - KT_CARD_MIN_P + 2] = {};
    for (uint32_t j = 0; j < m; j++) {
        if (registers[j] > q + 1) return kt::fail(KT_ERR_ARG, "kt_card_estimate: a register above 64 - p + 1");
        C[registers[j]]++;
    }
    const double md = (double)m;
    double z = md * card_tau(1.0 - (double)C[q + 1] / md);
    for (uint32_t v = q; v >= 1; v--) z = 0.5 * (z + (double)C[v]);
    z += md * card_sigma((double)C[0] / md);
    *estimate = (md * md / (2.0 * log(2.0))) / z;
    if (zero_registers) *zero_registers = C[0];
    return KT_OK;
}

extern "C" double kt_card_rel_error(int p) { return 1.04 / sqrt((double)(1ull << (p < 0 ? 0 : p > 63 ? 63 : p))); }
