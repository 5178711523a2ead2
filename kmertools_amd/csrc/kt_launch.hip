// kt_launch.hip - the definitions of kt_launch.hpp: launch helpers, shared argument checks and ktl::Call.
#include "kt_launch.hpp"

namespace {

constexpr int BLOCK = ktseg::BLOCK;

// flag |= 1 when a read holds 2^32 bases or more
__global__ __launch_bounds__(BLOCK) void long_read_kernel(const uint64_t *__restrict__ offsets, uint64_t n_reads,
                                                          uint32_t *__restrict__ flag) {
    for (uint64_t i = (uint64_t)blockIdx.x * BLOCK + threadIdx.x; i < n_reads; i += (uint64_t)gridDim.x * BLOCK)
        if (offsets[i + 1] - offsets[i] >= (1ull << 32)) atomicOr(flag, 1u);
}

}  // namespace

namespace ktl {

uint32_t grid_for(const kt_ctx *ctx, uint64_t work_items, uint32_t per_cu) {
    uint64_t g = (uint64_t)ctx->n_cu * per_cu;
    if (g > work_items) g = work_items;
    if (g < 1) g = 1;
    return (uint32_t)g;
}

dim3 pairs_grid(const kt_ctx *ctx, uint64_t n_a, uint64_t n_b, uint32_t b_per_wg) {
    const uint64_t want = (uint64_t)ctx->n_cu * 8;
    const uint64_t gx = n_a < want ? n_a : want;
    uint64_t gy = want / gx ? want / gx : 1;
    const uint64_t b_units = (n_b + b_per_wg - 1) / b_per_wg;
    if (gy > b_units) gy = b_units;
    if (gy > 65535) gy = 65535;
    return dim3((uint32_t)gx, (uint32_t)gy);
}

int make_seg_args(kt_ctx *ctx, const uint8_t *bases, const uint64_t *offsets, uint64_t n_reads,
                  uint64_t total_bases, int k, ktseg::SegArgs *out) {
    const uint64_t n_seg = (total_bases + ktseg::SEG - 1) / ktseg::SEG;
    uint64_t *seg_first = nullptr;
    if (int rc = ctx->claim(kt::AUX0, (n_seg + 2) * sizeof(uint64_t), "make_seg_args", &seg_first)) return rc;
    const uint64_t threads = n_reads + 1;
    const uint32_t blocks = (uint32_t)((threads + 255) / 256);
    hipLaunchKernelGGL(ktseg::seg_index_kernel, dim3(blocks), dim3(256), 0, ctx->stream, offsets, n_reads,
                       seg_first, n_seg);
    KT_HIP(hipGetLastError());
    *out = ktseg::SegArgs{bases, offsets, seg_first, n_reads, n_seg, (uint32_t)k};
    return KT_OK;
}

int Call::batch(const uint8_t *bases_, const uint64_t *offsets_, uint64_t n_reads_, const char *null_text) {
    bases = bases_, offsets = offsets_, n_reads = n_reads_;
    if (host()) {
        total = offsets[n_reads];
    } else {
        KT_HIP(hipMemcpyAsync(&total, offsets + n_reads, sizeof(uint64_t), hipMemcpyDeviceToHost, ctx_->stream));
        KT_HIP(hipStreamSynchronize(ctx_->stream));
    }
    if (total && !bases && null_text) return fail(null_text);
    return KT_OK;
}

int Call::stage() {
    if (!host()) return KT_OK;
    if (offsets[0] != 0) return kt::fail(KT_ERR_ARG, "offsets[0] must be 0");
    uint8_t *db = nullptr;
    uint64_t *dof = nullptr;
    if (int rc = scratch(kt::BASES, total + 64, &db)) return rc;
    if (int rc = scratch(kt::OFFSETS, (n_reads + 1) * 8, &dof)) return rc;
    if (int rc = up(db, bases, total)) return rc;
    if (int rc = up(dof, offsets, n_reads + 1)) return rc;
    bases = db, offsets = dof;
    return KT_OK;
}

int Call::refuse_long_reads(const char *why) {
    if (total < (1ull << 32)) return KT_OK;  // (below that no read can be this long)
    bool too_long = false;
    if (host()) {
        for (uint64_t i = 0; i < n_reads && !too_long; i++) too_long = offsets[i + 1] - offsets[i] >= (1ull << 32);
    } else {
        uint32_t *d_flag = nullptr, flag = 0;
        if (int rc = scratch(kt::AUX2, 4, &d_flag)) return rc;
        KT_HIP(hipMemsetAsync(d_flag, 0, 4, ctx_->stream));
        hipLaunchKernelGGL(long_read_kernel, dim3(grid_for(ctx_, (n_reads + BLOCK - 1) / BLOCK, 8)), dim3(BLOCK), 0, ctx_->stream,
                           offsets, n_reads, d_flag);
        KT_HIP(hipGetLastError());
        KT_HIP(hipMemcpyAsync(&flag, d_flag, 4, hipMemcpyDeviceToHost, ctx_->stream));
        KT_HIP(hipStreamSynchronize(ctx_->stream));
        ctx_->unclaim(kt::AUX2);  // (read back: the call's own AUX2 may follow)
        too_long = flag != 0;
    }
    return too_long ? fail((std::string("a read of 2^32 bases or more (") + why + ")").c_str()) : KT_OK;
}

int Call::fetch_bytes(void *dst, const void *dev, size_t bytes) {
    if (!dst) return kt::fail(KT_ERR_NOMEM, std::string(name_) + ": host alloc");
    hipError_t e = bytes ? hipMemcpyAsync(dst, dev, bytes, hipMemcpyDeviceToHost, ctx_->stream) : hipSuccess;
    if (e == hipSuccess) e = hipStreamSynchronize(ctx_->stream);
    if (e != hipSuccess) return kt::fail(KT_ERR_HIP, std::string(name_) + ": " + hipGetErrorString(e));
    return KT_OK;
}

int Call::finish() {
    if (!host()) return KT_OK;
    for (int i = 0; i < n_copies_; i++)
        KT_HIP(hipMemcpyAsync(copies_[i].dst, copies_[i].src, copies_[i].bytes, hipMemcpyDeviceToHost, ctx_->stream));
    n_copies_ = 0;
    KT_HIP(hipStreamSynchronize(ctx_->stream));
    return KT_OK;
}

}  // namespace ktl
