// Internal (non-ABI) declarations shared by the translation units of libkmertools_hip.so.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>

#include "../../include/kmertools_hip.h"

namespace kt {

void set_error(const std::string &msg);
int fail(int code, const std::string &msg);

#define KT_HIP(expr)                                                                   \
    do {                                                                               \
        hipError_t _e = (expr);                                                        \
        if (_e != hipSuccess)                                                          \
            return kt::fail(KT_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(_e)); \
    } while (0)

// growable device scratch owned by a ctx (only used by the KT_MEM_HOST staging path)
struct Scratch {
    void *p = nullptr;
    size_t cap = 0;
    int reserve(size_t bytes);
    void release();
};

constexpr int KT_MAX_OLIGO_K = 7;

// the context's six scratch buffers (kt_ctx::claim)
enum Buf { BASES, OFFSETS, OUT, AUX0, AUX1, AUX2, N_BUF };

}  // namespace kt

struct kt_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    int n_cu_device = 256;  // the device's compute units: what measures the hardware or lays out a bulk job's plan
    int n_cu = 256;         // the compute units the grids are sized by: n_cu_device, or less (kt_ctx_set_cu_limit)
    uint32_t xcc_n = 0, xcc_map = 0;  // XCDs that run this device's workgroups, XCC_ID -> dense index in nibbles (kt_bulk.hip's census)
    // device copies of the canonical-bin LUT (u16[4^k], lut[f] = 4 * rank(min(f, rc f)): the byte offset of the
    // bin's u32 counter inside a row), k = 1..7
    uint16_t *lut_dev[kt::KT_MAX_OLIGO_K + 1] = {};
    uint32_t *lut32_dev[13] = {};  // canonical rank of every k-mer, k = 1..12 (the generic oligo path, kt_oligo_generic.hip)
    // Scratch shared by everything that runs on the context.  Within one outermost library call (kt::ClaimScope) a buffer
    // has one holder: claim() reserves it, notes the claim in `claimed` and refuses a second one - a helper cannot take a
    // buffer behind its caller's back, and no pointer goes stale through a later reserve of the same buffer.
    kt::Scratch scratch[kt::N_BUF];
    uint32_t claimed = 0;  // bit b: buffer b is held
    int depth = 0;         // library calls open on this context (an entry point that calls another one)
    int claim_bytes(kt::Buf b, size_t bytes, const char *who, void **p);
    template <class T>
    int claim(kt::Buf b, size_t bytes, const char *who, T **p) { return claim_bytes(b, bytes, who, (void **)p); }
    // gives a buffer up before the call ends: its holder has read its result back (or the next holder's work is queued
    // behind the last kernel that touches it), and a later step of the same call takes the buffer
    void unclaim(kt::Buf b) { claimed &= ~(1u << b); }
    struct OligoKnobs {  // KT_OLIGO_* launch tunables, read once per context (kt_oligo.hip)
        bool loaded = false, live = false;
        uint32_t shape = 104, R = 0, oversub = 0, debug = 0, pw = 7;
        bool tune = true;
    } oligo_knobs;
    // Workgroups per resident slot of the k = 4 histogram launch, chosen by measurement per OUTPUT ARRAY (kt_oligo.hip,
    // oligo_launch): a few early large launches into an array cycle through the candidates with events around them,
    // the fastest stays for that array.  Which one is fastest goes with where the array lies in the memory, not with
    // the code (profiles/r3_oligo_placement.txt): the same process sees 1.90 and 2.40 ms on two of its allocations.
    struct OligoTune {
        static constexpr int NSET = 3, RING = 9, NEED = 3, WARM = 24, GIVE_UP = 45, ARRAYS = 8;
        struct Entry {                  // one output array (keyed by its address)
            const void *out = nullptr;
            uint64_t stamp = 0;         // last use (the least recently used entry makes room)
            bool decided = false;
            uint32_t pick = 96, launches = 0;
            double ns_per_read[NSET] = {0, 0, 0};  // sums while measuring, means once decided
            uint32_t kept[NSET] = {0, 0, 0};
        } arrays[ARRAYS];
        struct Trial { hipEvent_t a = nullptr, b = nullptr; const void *out = nullptr; uint32_t which = 0; uint64_t reads = 0; bool live = false; } ring[RING];
        uint64_t clock = 0;
        bool paused = false;            // kt_oligo_tuning(ctx, 0): launches neither count nor measure until switched on again
        uint32_t forced = 0;            // kt_oligo_tuning(ctx, n >= 2): paused, and every launch uses n workgroups per slot
        const void *last = nullptr;     // the array of the latest launch (kt_oligo_launch_info reports it)
        void release();
    } oligo_tune;
    int use();  // hipSetDevice
    int canon_lut(int k, const uint16_t **out);
    int canon_lut32(int k, const uint32_t **out);
};

namespace kt {
// One library call's hold on the context's scratch: every extern "C" entry point that claims scratch, itself or through a
// helper, opens one.  The outermost scope starts with no buffer held; an entry point called from another one keeps its
// caller's claims and gives back its own when it returns (its results are in its caller's arrays by then).
struct ClaimScope {
    kt_ctx *ctx;
    uint32_t outer;
    explicit ClaimScope(kt_ctx *c) : ctx(c), outer(c->depth++ ? c->claimed : 0u) { ctx->claimed = outer; }
    ClaimScope(const ClaimScope &) = delete;
    ~ClaimScope() { reset(), ctx->depth--; }
    // gives back what was claimed under this scope so far (a loop whose every round ends with a wait for the stream)
    void reset() { ctx->claimed = outer; }
};
}  // namespace kt

// where level 2 of the partition passes reads a table's level-1 buckets from: the regions of buckets 0, 1, ... (cap1 keys of
// room each, `counts` keys used) of the level-1 output (kt_bulk.hip)
struct kt_seg_src {
    const void *keys;
    const uint64_t *counts;
    uint64_t cap1;
};

namespace kt {
// The form a table (kt_ctr) is in: where its entries are and what its buffers hold ("The table's forms").
//   Stale   the slots hold old data, cleared before anything reads or probes them; *distinct = 0
//   Image   the slots are the probing image; *distinct = occupied slots
//   Dense   every range's entries packed at its front (keys, then counts), range_counts[r] of them; *distinct = entries
//   Target  the entries are the export target's arrays [0, *distinct), as (key, occurrences); the slots: the build's scratch
// In every other form the target's arrays are the caller's.  Transitions - the functions of kt_ctr in brackets, and no other
// code assigns the form:
//   any -> Stale             kt_ctr_clear [cleared]
//   Stale -> Image           the deferred clear is carried out for the first reader or probing writer [imaged]
//   Dense, Target -> Image   kt_table_image, for whatever has to probe: the ranges materialised in place / the target's
//                            pairs loaded into the wiped slots, the arrays the caller's again [imaged]
//   Stale, Image -> Image, Dense, Target   a bulk job wrote every slot [built]: a fresh() table is left Dense - Target when
//                            a target is set and took the entries - or, KT_BULK_DENSE=0, as its Image; a table with data
//                            is imaged first and merged range by range into its Image
// fresh(): nothing was inserted since the last clear - a Stale table, or an Image only readers have touched.  Every writer
// ends it [written, built]; an erase that removes every entry does not bring it back.  A Dense or Target table is never fresh.
enum class TableForm : uint8_t { Stale, Image, Dense, Target };

// What kt_ctr_export_stage[_range] staged for kt_ctr_export_fetch: n entries in device memory - in the table's own stage
// buffers or, all the entries of a Target-form table, in the target's arrays themselves.  Dropped by every call that changes
// the table's content (ktl::table_write, the bulk job's plan, kt_ctr_clear) and by whatever hands the arrays it points at
// back to the caller (kt_table_image of a Target-form table, kt_ctr_export_target).
class Stage {
public:
    void set(const uint64_t *keys, const uint32_t *counts, uint64_t n) { keys_ = keys, counts_ = counts, n_ = n; }
    void drop() { set(nullptr, nullptr, 0); }
    bool aliases(const void *p) const { return n_ && keys_ == p; }  // the staged entries are the array at p
    const uint64_t *keys() const { return keys_; }
    const uint32_t *counts() const { return counts_; }
    uint64_t n() const { return n_; }

private:
    const uint64_t *keys_ = nullptr;
    const uint32_t *counts_ = nullptr;
    uint64_t n_ = 0;
};
}  // namespace kt

struct kt_bulk_job;  // kt_bulk.hip: the plan and buffers of a partition + range build in progress
void kt_bulk_job_free(kt_bulk_job *job);

struct kt_ctr {
    kt_ctx *ctx = nullptr;
    int k = 0;
    uint64_t cap = 0;          // m8 * 2^(n-3) slots (kttab::Geom)
    uint32_t shift = 0;        // 64 - n
    uint32_t m8 = 8;           // eighths of 2^n (slots per 4096-position range / 512)
    uint32_t kbits = 0;        // 2k when k <= 16: the table's hash is the bijection ktd::nhash (kttab::Geom)
    // the table of rank `owner` of a counter sharded over n_owners ranks (kt_shard.hip; a table of its own: 1, 0): a whole
    // table like any other - only kt_cov_batch_part looks at this (a k-mer that is not here may be on another rank)
    uint32_t n_owners = 1, owner = 0;
    // CUs the level-1 launches of a bulk job leave free (kt_shard.hip: the exchange's kernels run beside them on the comm stream,
    // and a level-1 workgroup takes a whole CU's LDS for the length of the launch)
    uint32_t l1_spare_cus = 0;
    // of the last bulk job into an export target: level-1 buckets whose keys did not fit their fixed fine regions and went
    // through the exact pass (of l2_buckets) - a caller that plans its jobs itself (kt_shard.hip) gives the next one more room
    uint32_t l2_redone = 0, l2_buckets = 0;
    bool paged_failed = false; // a bulk build overflowed a paged level-1 bucket: exact offsets from now on
    uint32_t *range_counts = nullptr;  // device, one per range: entries of the range while the table is Dense
    // export target (kt_ctr_export_target): device arrays of the caller that a fresh bulk build writes its packed
    // entries to instead of the ranges' own slots - the build's output IS the export (no copy pass afterwards)
    uint64_t *xt_keys = nullptr;
    uint32_t *xt_counts = nullptr;
    uint64_t xt_max = 0;
    kt::Stage stage;                   // what kt_ctr_export_stage[_range] staged
    kt::Scratch b_ext;                 // the export-target build's holes and the scratch behind the caller's arrays
    kt::Scratch b_stage_k, b_stage_c;  // kt_ctr_export_stage's copy of the entries (when they are not the export target's arrays)
    kt::Scratch b_keys1, b_keys2, b_meta;  // bulk-build buffers (kt_bulk.hip), kept across calls
    kt::Scratch b_pack;                    // ... the reads packed for level 1 (PackedSource, KT_BULK_PACK)
    kt::Scratch b_desc;                    // ... and the descriptors of its record sources (kt_bulk_add_records)
    kt_bulk_job *job = nullptr;
    void *slots = nullptr;     // [cap] of {u64 key (KT_EMPTY_KEY = free), u32 count, u32 pad}
    uint32_t *flags = nullptr; // [0] = overflow flag, device
    uint64_t *cursor = nullptr; // device scalar for export
    uint64_t *distinct = nullptr; // device scalar: occupied slots (kept by every insert path, so kt_ctr_size is one 8-byte read)

    // ---- the form (kt::TableForm): read by form() / fresh(), assigned by the transitions below and by nothing else
    kt::TableForm form() const { return form_; }
    // nothing was inserted since the last clear: the next bulk job builds the ranges instead of merging into them
    bool fresh() const { return fresh_; }
    void cleared() { form_ = kt::TableForm::Stale, fresh_ = true; }  // kt_ctr_clear
    void imaged() { form_ = kt::TableForm::Image; }                  // the slots hold the probing image now
    void written() { fresh_ = false; }                               // a probing writer is about to insert (ktl::table_write)
    // a bulk job has written every slot: packed ranges (`ext`: into the export target instead) or the probing image
    void built(bool dense, bool ext) {
        form_ = !dense ? kt::TableForm::Image : ext ? kt::TableForm::Target : kt::TableForm::Dense;
        fresh_ = false;
    }
    // a deferred error: the build found the target smaller than the table and went into the slots; kt_bulk_finish reports it
    void target_too_small() { xt_too_small_ = true; }
    bool take_target_too_small() { const bool was = xt_too_small_; xt_too_small_ = false; return was; }

private:
    kt::TableForm form_ = kt::TableForm::Stale;
    bool fresh_ = true;
    bool xt_too_small_ = false;
};

// kt_prefilter.hip: the `once` and `twice` bit arrays that keep k-mers seen once out of a table (kt_prefilter.hpp: the layout)
struct kt_prefilter {
    kt_ctx *ctx = nullptr;
    int k = 0;
    uint32_t a = 0, b = 0;      // log2 of the words of once / twice
    uint64_t seed = 0;
    uint64_t *once = nullptr, *twice = nullptr;
    uint64_t *sums = nullptr;   // device: [0] windows walked, [1] promotions, [2], [3] kt_prefilter_stats's popcounts
};

// kt_oligo_generic.hip: histograms for k outside 3..7, counted in global memory (device pointers, enqueued)
int kt_oligo_generic_launch(kt_ctx *ctx, const uint8_t *bases, const uint64_t *offsets, uint64_t n_reads, int k,
                            int count_min, int norm, int total_step, int dt, void *out);

// kt_sort.hip: (key, count) pairs in device memory into ascending key order (LSD radix sort over key_bits bits, on the
// context's stream; scratch: the context's OUT and AUX0)
int kt_sort_pairs(kt_ctx *ctx, uint64_t *keys, uint32_t *counts, uint64_t n, uint32_t key_bits);

namespace kt {
// kt_scaled.hip: the one routine that turns n < 2^32 (hash, abundance, row) elements in device memory into scaled sketches -
// sorted by (row, hash), equal hashes of a row made one with their abundances summed (saturating) - and hands them to the
// caller's arrays in `mem`.  kt_scaled_batch, kt_scaled_merge and kt_ctr_scaled (kt_ctr.hip) end here.
struct ScaledElems {
    uint64_t *keys;          // the n hashes, in any order; the routine sorts them in place
    const uint32_t *abunds;  // their abundances, or null: 1 each
    const uint64_t *rows;    // their rows (< n_rows), or null: all of row 0
    uint64_t n, n_rows;
};
struct ScaledOut {
    uint64_t *hashes;        // the caller's arrays, in `mem` (abunds and row_offsets may be null)
    uint32_t *abunds;
    uint64_t max_out;
    uint64_t *row_offsets;   // n_rows + 1
    uint64_t *n_out;         // host
    int mem;
};
// Scratch: OUT and AUX0 (kt_sort_pairs) and AUX2, none of which the caller may hold; the elements are the caller's (AUX1,
// BASES, ...).  Enqueues the copies into the caller's arrays and does not wait for them.  KT_ERR_ARG with *n_out set and
// nothing else written when 0 < max_out < *n_out.
int scaled_finish(kt_ctx *ctx, const char *who, const ScaledElems &e, const ScaledOut &o);
}  // namespace kt

namespace kt {
// host-side table builders (kt_host.cpp)
uint64_t rev_comp_bits(uint64_t kmer, int k);
// fills lut_full[4^k]: rank of the canonical form of every k-mer; returns kcount
uint32_t build_canon_lut(int k, uint16_t *lut_full);
}  // namespace kt
