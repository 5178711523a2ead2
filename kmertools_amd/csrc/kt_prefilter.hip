// kt_prefilter.hip - the two-pass pre-filter that keeps k-mers seen once out of a table: two arrays of 64-bit words in HBM,
// `once` and `twice` (kt_prefilter.hpp: where a k-mer's bits lie).  Pass 1 is here; pass 2 is kt_ctr_add_reads_filtered
// (kt_ctr.hip), count_reads_kernel with the filter's test in front of its insert.
//
//   prefilter_add_kernel    a persistent grid over the 8192-base segments of the ktseg front end, as card_kernel walks
//                           them.  Per k-mer: load the once word; not covered -> atomicOr, and the k-mer is done when the
//                           value that came back was not covered either (first sighting).  Covered, by the load or by what
//                           the atomic returned: the k-mer goes to `twice` - load, and an atomicOr only when the word does
//                           not cover the pattern yet; a promotion is an atomicOr whose return value did not cover it.
//                           The bits only ever get set, so a stale load (the XCDs' L2s are not coherent) can only send a
//                           k-mer to the atomic, which is coherent and decides.  Two lanes with the same k-mer meet at one
//                           atomic of one word, whichever wave, workgroup or XCD they are in: the second sees the first,
//                           so no k-mer with two occurrences misses `twice`.  After its second sighting a k-mer costs two
//                           loads and no atomic.  (Poly-A: 64 lanes on one word - the first atomicOr sets it, the others
//                           of later segments find it covered by the load.)
//   prefilter_popcount_kernel  the set bits of both arrays, summed per wave (ktd::wave_sums), one atomic per wave.
//   prefilter_query_kernel  the membership test for a list of keys.
#include "kt_internal.hpp"
#include "kt_launch.hpp"
#include "kt_prefilter.hpp"

namespace {

using ktpf::pattern_of;
using ktpf::View;
using ktseg::SegArgs;
using ktseg::SegShared;
constexpr uint32_t BLOCK = ktseg::BLOCK;
typedef unsigned long long ull;

__device__ __forceinline__ uint64_t peek(const uint64_t *w) { return __hip_atomic_load(w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ uint64_t set_bits(uint64_t *w, uint64_t p) { return atomicOr(reinterpret_cast<ull *>(w), (ull)p); }

__global__ __launch_bounds__(BLOCK) void prefilter_add_kernel(SegArgs a, View f, uint64_t *__restrict__ sums) {
    __shared__ SegShared sm;
    uint64_t windows = 0, promoted = 0;
    for (uint64_t g = blockIdx.x; g < a.n_seg; g += gridDim.x) {
        ktseg::for_each_kmer(a, g, sm, [&](uint64_t fw, uint64_t rc, uint64_t) {
            windows++;
            const uint64_t h = f.once_hash(fw < rc ? fw : rc), p1 = pattern_of(h);
            uint64_t *w1 = f.once_word(h);
            if ((peek(w1) & p1) != p1 && (set_bits(w1, p1) & p1) != p1) return;  // the first sighting
            const uint64_t h2 = f.twice_hash(h), p2 = pattern_of(h2);
            uint64_t *w2 = f.twice_word(h2);
            if ((peek(w2) & p2) != p2) promoted += (set_bits(w2, p2) & p2) != p2;
        });
    }
    ktd::wave_sums(windows, promoted);
    if (ktd::lane_id() == 0) {
        if (windows) atomicAdd(reinterpret_cast<ull *>(sums), (ull)windows);
        if (promoted) atomicAdd(reinterpret_cast<ull *>(sums + 1), (ull)promoted);
    }
}

// sums[0] += the set bits of x[0, nx), sums[1] += those of y[0, ny)
__global__ __launch_bounds__(BLOCK) void prefilter_popcount_kernel(const uint64_t *__restrict__ x, uint64_t nx,
                                                                   const uint64_t *__restrict__ y, uint64_t ny,
                                                                   uint64_t *__restrict__ sums) {
    const uint64_t first = (uint64_t)blockIdx.x * BLOCK + threadIdx.x, step = (uint64_t)gridDim.x * BLOCK;
    uint64_t bx = 0, by = 0;
    for (uint64_t i = first; i < nx; i += step) bx += (uint32_t)__popcll(x[i]);
    for (uint64_t i = first; i < ny; i += step) by += (uint32_t)__popcll(y[i]);
    ktd::wave_sums(bx, by);
    if (ktd::lane_id() == 0) {
        if (bx) atomicAdd(reinterpret_cast<ull *>(sums), (ull)bx);
        if (by) atomicAdd(reinterpret_cast<ull *>(sums + 1), (ull)by);
    }
}

__global__ __launch_bounds__(BLOCK) void prefilter_query_kernel(const uint64_t *__restrict__ keys, uint64_t n, View f,
                                                                uint8_t *__restrict__ out) {
    for (uint64_t i = (uint64_t)blockIdx.x * BLOCK + threadIdx.x; i < n; i += (uint64_t)gridDim.x * BLOCK) {
        const uint64_t h = f.once_hash(keys[i]), p1 = pattern_of(h);
        const uint64_t h2 = f.twice_hash(h), p2 = pattern_of(h2);
        out[i] = (uint8_t)(((*f.once_word(h) & p1) == p1 ? 1u : 0u) | ((*f.twice_word(h2) & p2) == p2 ? 2u : 0u));
    }
}

bool bad_log2(int e) { return e < KT_PREFILTER_MIN_LOG2 || e > KT_PREFILTER_MAX_LOG2; }
static_assert(ktpf::MIN_LOG2 == KT_PREFILTER_MIN_LOG2 && ktpf::MAX_LOG2 == KT_PREFILTER_MAX_LOG2, "the exponents' range");

}  // namespace

using namespace ktl;

extern "C" {

int kt_prefilter_create(kt_ctx *ctx, int k, int log2_once, int log2_twice, uint64_t seed, kt_prefilter **out) {
    if (!ctx || !out) return kt::fail(KT_ERR_ARG, "kt_prefilter_create: null");
    *out = nullptr;
    if (k < 1 || k > 31) return kt::fail(KT_ERR_ARG, "kt_prefilter_create: k must be in 1..31");
    if (bad_log2(log2_once) || bad_log2(log2_twice))
        return kt::fail(KT_ERR_ARG, "kt_prefilter_create: log2_once and log2_twice must be in KT_PREFILTER_MIN_LOG2..KT_PREFILTER_MAX_LOG2");
    if (int rc = ctx->use()) return rc;
    kt_prefilter *f = new (std::nothrow) kt_prefilter();
    if (!f) return kt::fail(KT_ERR_NOMEM, "kt_prefilter_create: host alloc");
    f->ctx = ctx;
    f->k = k;
    f->a = (uint32_t)log2_once;
    f->b = (uint32_t)log2_twice;
    f->seed = seed;
    hipError_t e = hipMalloc((void **)&f->once, sizeof(uint64_t) << f->a);
    if (e == hipSuccess) e = hipMalloc((void **)&f->twice, sizeof(uint64_t) << f->b);
    if (e == hipSuccess) e = hipMalloc((void **)&f->sums, 64);
    if (e != hipSuccess) {
        kt_prefilter_destroy(f);
        return kt::fail(KT_ERR_NOMEM, std::string("kt_prefilter_create: hipMalloc: ") + hipGetErrorString(e));
    }
    *out = f;
    return kt_prefilter_clear(f);
}

int kt_prefilter_destroy(kt_prefilter *f) {
    if (!f) return KT_OK;
    if (f->ctx) {
        (void)hipSetDevice(f->ctx->device);
        (void)hipStreamSynchronize(f->ctx->stream);
    }
    for (void *p : {(void *)f->once, (void *)f->twice, (void *)f->sums})
        if (p) (void)hipFree(p);
    delete f;
    return KT_OK;
}

int kt_prefilter_clear(kt_prefilter *f) {
    if (!f) return kt::fail(KT_ERR_ARG, "kt_prefilter_clear: null");
    if (int rc = f->ctx->use()) return rc;
    KT_HIP(hipMemsetAsync(f->once, 0, sizeof(uint64_t) << f->a, f->ctx->stream));
    KT_HIP(hipMemsetAsync(f->twice, 0, sizeof(uint64_t) << f->b, f->ctx->stream));
    KT_HIP(hipMemsetAsync(f->sums, 0, 64, f->ctx->stream));
    return KT_OK;
}

int kt_prefilter_add_reads(kt_prefilter *f, const uint8_t *bases, const uint64_t *offsets, uint64_t n_reads, int mem) {
    if (!f) return kt::fail(KT_ERR_ARG, "kt_prefilter_add_reads: null filter");
    kt_ctx *ctx = f->ctx;
    Call call(ctx, mem, "kt_prefilter_add_reads");
    if (int rc = call.enter()) return rc;
    if (n_reads == 0) return KT_OK;
    if (!offsets) return call.fail("null offsets");
    if (int rc = call.batch(bases, offsets, n_reads)) return rc;
    if (int rc = call.refuse_long_reads("the walk's positions in a read are u32")) return rc;
    if (!call.total) return KT_OK;
    if (int rc = call.stage()) return rc;
    SegArgs a;
    if (int rc = make_seg_args(ctx, call.bases, call.offsets, n_reads, call.total, f->k, &a)) return rc;
    if (int rc = launch(prefilter_add_kernel, dim3(grid_for(ctx, a.n_seg, 8)), dim3(BLOCK), 0, ctx->stream, a, view_of(f), f->sums))
        return rc;
    return call.finish();
}

int kt_prefilter_stats(kt_prefilter *f, uint64_t *windows, uint64_t *promotions, uint64_t *once_bits_set,
                       uint64_t *twice_bits_set) {
    if (!f) return kt::fail(KT_ERR_ARG, "kt_prefilter_stats: null filter");
    kt_ctx *ctx = f->ctx;
    if (int rc = ctx->use()) return rc;
    const uint64_t nx = 1ull << f->a, ny = 1ull << f->b;
    KT_HIP(hipMemsetAsync(f->sums + 2, 0, 16, ctx->stream));
    if (int rc = launch(prefilter_popcount_kernel, dim3(grid_for(ctx, (nx + BLOCK - 1) / BLOCK, 8)), dim3(BLOCK), 0, ctx->stream,
                        (const uint64_t *)f->once, nx, (const uint64_t *)f->twice, ny, f->sums + 2))
        return rc;
    uint64_t h[4] = {};
    KT_HIP(hipMemcpyAsync(h, f->sums, sizeof h, hipMemcpyDeviceToHost, ctx->stream));
    KT_HIP(hipStreamSynchronize(ctx->stream));
    if (windows) *windows = h[0];
    if (promotions) *promotions = h[1];
    if (once_bits_set) *once_bits_set = h[2];
    if (twice_bits_set) *twice_bits_set = h[3];
    return KT_OK;
}

int kt_prefilter_query(kt_prefilter *f, const uint64_t *keys, uint64_t n, uint8_t *out, int mem) {
    if (!f) return kt::fail(KT_ERR_ARG, "kt_prefilter_query: null filter");
    kt_ctx *ctx = f->ctx;
    Call call(ctx, mem, "kt_prefilter_query");
    if (int rc = call.enter()) return rc;
    if (n == 0) return KT_OK;
    if (!keys || !out) return call.fail("null buffer");
    const uint64_t *d_keys = nullptr;
    uint8_t *d_out = nullptr;
    if (int rc = call.in(kt::AUX1, keys, n, &d_keys)) return rc;
    if (int rc = call.out(kt::OUT, out, n, &d_out)) return rc;
    if (int rc = launch(prefilter_query_kernel, dim3(grid_for(ctx, (n + BLOCK - 1) / BLOCK, 8)), dim3(BLOCK), 0, ctx->stream, d_keys,
                        n, view_of(f), d_out))
        return rc;
    return call.finish();
}

}  // extern "C"
