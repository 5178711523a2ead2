// kt_launch.hpp - what the host code of the extern "C" entry points shares: launch helpers of the segment front-end,
// argument checks that several entry points make in the same words, ktl::launch, ktl::carve_parts and ktl::carve (one kernel
// launch; typed arrays cut from one buffer; one claim of a scratch buffer cut that way), and ktl::Call, the one path by which an entry point moves its arguments between the
// caller's memory and the device.  Defined in kt_launch.hip, the templates here.
#pragma once
#include <memory>
#include <new>

#include "kt_internal.hpp"
#include "kt_prefilter.hpp"
#include "kt_segment.hpp"
#include "kt_table.hpp"

namespace ktl {

// min(work_items, n_cu * per_cu) workgroups, at least 1
uint32_t grid_for(const kt_ctx *ctx, uint64_t work_items, uint32_t per_cu);
// the grid of an all-pairs kernel (n_a > 0): a row of A per workgroup in x, the rows of B dealt to the waves of y, b_per_wg at
// a time - as many in y as fill the device when A is small
dim3 pairs_grid(const kt_ctx *ctx, uint64_t n_a, uint64_t n_b, uint32_t b_per_wg);
// SegArgs for a device-resident CSR batch (launches seg_index_kernel into the context's scratch AUX0)
int make_seg_args(kt_ctx *ctx, const uint8_t *bases, const uint64_t *offsets, uint64_t n_reads,
                  uint64_t total_bases, int k, ktseg::SegArgs *out);
// the table's geometry as the device functions take it (kt_table.hpp)
inline kttab::Geom geom_of(const kt_ctr *ctr) { return kttab::Geom{ctr->cap, ctr->shift, ctr->m8, ctr->kbits}; }
// the table as the kernels that probe it take it (after table_ready: the slots hold the probing image)
inline kttab::Probed probed_of(const kt_ctr *ctr, uint32_t n_parts = 1, uint32_t part = 0) {
    return kttab::Probed{(const kttab::Slot *)ctr->slots, geom_of(ctr), n_parts, part};
}
// ... and as the kernels that insert into it take it (after table_write)
inline kttab::TableRef writable_of(const kt_ctr *ctr) { return kttab::TableRef{(kttab::Slot *)ctr->slots, geom_of(ctr), ctr->flags}; }
// a pre-filter as its kernels take it (kt_prefilter.hpp)
inline ktpf::View view_of(const kt_prefilter *f) { return ktpf::View{f->once, f->twice, f->seed, f->a, f->b}; }
// The readers' gate (kt_table.hip): brings the table to its probing image - a deferred clear is carried out, a Dense or
// Target-form table imaged - and reports KT_ERR_FULL if it overflowed
int table_ready(kt_ctr *ctr);
// The probing writers' gate: drops the staged export (the table's content is about to change), brings the table to its
// probing image as table_ready does - without the wait for the overflow flag - marks it no longer fresh and hands back
// the reference the inserting kernels take.  The bulk job is the other writer (kt_bulk_job::plan, kt_ctr::built).
int table_write(kt_ctr *ctr, kttab::TableRef *t);
// every slot of the table freed (kt_table.hip's table_clear_kernel, on the context's stream); the form is the caller's business
int table_wipe(kt_ctr *ctr);
// table[d_keys[i]] += d_counts[i] (null: 1) for n > 0 device pairs through the probing path (kt_ctr.hip's add_pairs_kernel)
int add_pairs(kt_ctr *ctr, const kttab::TableRef &t, const uint64_t *d_keys, const uint32_t *d_counts, uint64_t n);
// d_counts[i] = occurrences of d_keys[i] in the table (0: absent), n > 0 device keys, on the context's stream; the table
// holds its probing image (table_ready).  kt_cov.hip's lookup_kernel.
int lookup_counts(kt_ctr *table, const uint64_t *d_keys, uint64_t n, uint32_t *d_counts);

// One kernel launch: where it asks for dynamic LDS, the kernel's limit is raised to that first (at every launch, not once
// per process: two builds of the library may be loaded side by side), and the launch's own error is the status.
template <class... P, class... A>
int launch(void (*kern)(P...), dim3 grid, dim3 block, size_t lds, hipStream_t stream, A &&...args) {
    if (lds) KT_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(kern, grid, block, lds, stream, static_cast<P>(args)...);
    KT_HIP(hipGetLastError());
    return KT_OK;
}

// carve_parts<ALIGN>(at, &a, count_a, &b, count_b, ...): typed arrays cut from one buffer in the order given, each taking
// a multiple of ALIGN bytes.  Returns their bytes; with `at` set it also puts the arrays there (null: the size alone).
template <size_t ALIGN>
size_t carve_parts(uint8_t *) { return 0; }
template <size_t ALIGN, class T, class... More>
size_t carve_parts(uint8_t *at, T **p, uint64_t count, More... more) {
    const size_t bytes = (count * sizeof(T) + ALIGN - 1) & ~(ALIGN - 1);
    if (at) *p = (T *)at;
    return bytes + carve_parts<ALIGN>(at ? at + bytes : at, more...);
}

// One call of an entry point that takes `int mem`.  It holds the call's claim scope on the context's scratch and is the
// only place that tells the two memory kinds apart: for KT_MEM_DEVICE every method hands the caller's pointer through
// and nothing waits; for KT_MEM_HOST inputs go up into a claimed scratch buffer, outputs are made in one, and finish()
// issues the copies back and waits for the stream once.
class Call {
public:
    Call(kt_ctx *ctx, int mem, const char *name) : ctx_(ctx), mem_(mem), name_(name), scope_(ctx) {}
    bool host() const { return mem_ == KT_MEM_HOST; }
    int fail(const char *what) const { return kt::fail(KT_ERR_ARG, std::string(name_) + ": " + what); }
    // "<name>: bad mem" unless mem is one of the two kinds; makes the context's device the current one
    int enter() { return mem_ == KT_MEM_HOST || mem_ == KT_MEM_DEVICE ? ctx_->use() : fail("bad mem"); }
    int check_part(uint32_t n_parts, uint32_t part) const { return part < n_parts ? KT_OK : fail("need part < n_parts"); }
    // the entry points that need every k-mer's count in one table refuse one shard of a sharded table
    int refuse_shard(const kt_ctr *t) const {
        return t->n_owners > 1 ? fail("the table is one shard of a sharded table - shards are not supported "
                                      "(a shard cannot tell a k-mer absent here from one absent everywhere)") : KT_OK;
    }

    // the CSR batch of the call, as the caller gave it until stage(): total = offsets[n_reads] (a read-back for device
    // memory); "<name>: <null_text>" when the batch has bases and `bases` is null
    const uint8_t *bases = nullptr;
    const uint64_t *offsets = nullptr;
    uint64_t n_reads = 0, total = 0;
    int batch(const uint8_t *bases, const uint64_t *offsets, uint64_t n_reads, const char *null_text = "null bases");
    // host: the batch into BASES and OFFSETS (offsets[0] must be 0); bases / offsets become the device copies
    int stage();
    // "<name>: a read of 2^32 bases or more (<why>)" when the batch holds one
    int refuse_long_reads(const char *why);

    // a scratch buffer for the call itself, whichever the memory kind
    template <class T>
    int scratch(kt::Buf slot, size_t bytes, T **d) { return ctx_->claim(slot, bytes, name_, d); }
    // host: n elements of the caller's `p` to `dev`, on the stream
    template <class T>
    int up(T *dev, const T *p, uint64_t n) {
        if (host() && n) KT_HIP(hipMemcpyAsync(dev, p, n * sizeof(T), hipMemcpyHostToDevice, ctx_->stream));
        return KT_OK;
    }
    // host: queues n elements at `dev` for finish() to copy to the caller's `p` (null: nothing) - the elements the entry
    // point filled, which may be fewer than it reserved
    template <class T>
    void back(T *p, const T *dev, uint64_t n) {
        if (host() && p && n) copies_[n_copies_++] = Copy{p, dev, n * sizeof(T)};
    }
    // an input array of n elements: the caller's pointer, or its copy in `slot`
    template <class T>
    int in(kt::Buf slot, const T *p, uint64_t n, const T **d) {
        T *s = const_cast<T *>(p);
        if (host())
            if (int rc = scratch(slot, n * sizeof(T), &s)) return rc;
        *d = s;
        return up(s, p, n);
    }
    // an output array of n elements: the caller's pointer, or `slot` and a copy back by finish()
    template <class T>
    int out(kt::Buf slot, T *p, uint64_t n, T **d) {
        *d = p;
        if (host())
            if (int rc = scratch(slot, n * sizeof(T), d)) return rc;
        back(p, (const T *)*d, n);
        return KT_OK;
    }
    // waits for the stream and hands out a host copy of n device elements: what an entry point adds into its caller's arrays
    template <class T>
    int fetch(const T *dev, uint64_t n, std::unique_ptr<T[]> *h) {
        h->reset(new (std::nothrow) T[n]);
        return fetch_bytes(h->get(), dev, n * sizeof(T));
    }
    // host: the queued copies back, then one wait for the stream; device: nothing (the call stays asynchronous)
    int finish();
    // gives the call's scratch back (a loop whose every round ends with finish() takes it anew)
    void release() { scope_.reset(); }

private:
    struct Copy { void *dst; const void *src; size_t bytes; };
    int fetch_bytes(void *dst, const void *dev, size_t bytes);
    kt_ctx *ctx_;
    int mem_;
    const char *name_;
    kt::ClaimScope scope_;
    Copy copies_[8];
    int n_copies_ = 0;
};

// carve(call, buf, &a, count_a, &b, count_b, ...): one claim of a scratch buffer, cut into typed arrays that each take a
// multiple of 16 bytes (carve_parts)
template <class... Parts>
int carve(Call &call, kt::Buf buf, Parts... parts) {
    uint8_t *b = nullptr;
    if (int rc = call.scratch(buf, carve_parts<16>(nullptr, parts...), &b)) return rc;
    carve_parts<16>(b, parts...);
    return KT_OK;
}

}  // namespace ktl
