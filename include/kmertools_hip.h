/*
 * kmertools_hip.h - C ABI of libkmertools_hip.so, the MI355X (gfx950) drop-in for
 * kmertools' k-mer hot path.
 *
 * The reference (anuradhawick/kmertools, pure Rust) has no FFI today; the entry
 * points below are what a `extern "C"` block in the reference's crates would
 * bind in place of the Rust functions cited on each declaration (paths relative
 * to the reference root).  INTEGRATION.md shows the Rust-side binding.
 *
 * Conventions
 *  - plain pointers and sizes only; the caller owns every input and output buffer;
 *    the library owns device scratch inside kt_ctx / kt_ctr.
 *  - every function returns KT_OK (0) or a KT_ERR_* code; kt_last_error() gives the
 *    message for the calling thread.  Nothing aborts or throws across the ABI.
 *  - read batches are CSR: `bases` = concatenated ASCII bytes (no separators),
 *    `offsets` = uint64[n_reads + 1], read i = bases[offsets[i] .. offsets[i+1]).
 *  - `mem` says where `bases`, `offsets` and the output buffers live:
 *    KT_MEM_DEVICE = all are device (HBM) pointers, work is enqueued on the ctx
 *    stream and the call returns without waiting for it to finish (a few calls
 *    say that they synchronise; a large batch into an empty k-mer table waits
 *    once or twice for a 4-byte flag in the middle of its kernels);
 *    KT_MEM_HOST   = all are host pointers, the library stages them through its
 *    own device scratch and returns after the results are back on the host.
 *  - k-mers are uint64 (`type Kmer = u64`, kmer/src/lib.rs:4), 2 bits per base,
 *    A=0 C=1 G=2 T=3, first base most significant.
 */
#ifndef KMERTOOLS_HIP_H
#define KMERTOOLS_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define KT_OK 0
#define KT_ERR_ARG 1      /* bad argument (k out of range, null pointer, ...) */
#define KT_ERR_HIP 2      /* a HIP runtime call failed; message has the HIP error */
#define KT_ERR_NOMEM 3    /* device or host allocation failed */
#define KT_ERR_FULL 4     /* k-mer table ran out of slots (raise capacity) */
#define KT_ERR_NODEVICE 5 /* no usable gfx950 device */
#define KT_ERR_BADNT 6    /* kt_cgr_points: a byte outside ACGTUacgtu ("Bad nucleotide, unable to proceed") */
#define KT_ERR_IO 7       /* table files: an unreadable, unwritable or malformed file; message names what was wrong */

#define KT_MEM_HOST 0
#define KT_MEM_DEVICE 1

#define KT_F64 0 /* reference's element type (Vec<f64>) */
#define KT_F32 1 /* BASELINE cfg5 output type */
#define KT_U32 2 /* raw integer counts (norm must be 0) */

#define KT_EMPTY_KEY 0xFFFFFFFFFFFFFFFFull /* never a k-mer: k <= 31 => key < 2^62 */

typedef struct kt_ctx kt_ctx; /* one device + one stream; use from one host thread at a time */
typedef struct kt_ctr kt_ctr; /* HBM-resident canonical k-mer count table */

/* ---- library ----------------------------------------------------------------- */
int kt_version(void);
const char *kt_last_error(void);
int kt_device_count(int *count);

/* own_stream == 0: enqueue on `stream`, a hipStream_t of the caller (e.g. torch's current
 * stream; NULL is the device's default stream).  own_stream != 0: `stream` is ignored and
 * the ctx creates and owns a private non-blocking stream. */
int kt_ctx_create(int device, void *stream, int own_stream, kt_ctx **out);
int kt_ctx_destroy(kt_ctx *ctx);
int kt_ctx_sync(kt_ctx *ctx);
/* The context's workgroup budget: from the next launch on, the grids of this context are sized as if the device had n
 * compute units (every grid-stride launch asks for min(work, CUs * a small factor) workgroups).  n = 0 restores the
 * device's count, n above it is clamped to it.  Results never depend on it.  Useful for leaving room on a shared card;
 * the tests use it to make every grid-stride loop take several trips at small sizes.  (What describes the hardware or a
 * bulk job's plan - the XCD census, the partition geometry - stays on the device's count.) */
int kt_ctx_set_cu_limit(kt_ctx *ctx, uint32_t n);
/* the compute units the grids follow now (*n_cu) and the device's count (*n_cu_device); either pointer may be NULL */
int kt_ctx_cu_limit(kt_ctx *ctx, uint32_t *n_cu, uint32_t *n_cu_device);
/* free / total HBM of the context's device in bytes (hipMemGetInfo): lets a caller size a table to what fits */
int kt_device_memory(kt_ctx *ctx, uint64_t *free_bytes, uint64_t *total_bytes);

/* A device array that is fast to write.  Where a large allocation lands in the HBM moves the store-bound kernels by up
 * to 20 % - reproducibly per allocation, with no difference in plain fill rate - so a caller that keeps
 * an output (or input) array for many launches can have the library choose among `candidates` allocations of `bytes`:
 * all are allocated (fewer if they would take more than 60 % of the free memory), `probe(user, array)` - the caller's
 * function, which enqueues the work the array is meant for on the context's stream, e.g. kt_oligo_batch into it - runs
 * 20 times on the first one and then `launches` times on each between two events (its first call into an array is not
 * counted), the fastest array is returned in *out and the others are freed.  ms[i] (may be NULL; room for `candidates`
 * values) = milliseconds per probe on candidate i; candidate 0 is what a plain allocation would have been; *n_tried,
 * *picked may be NULL.  probe == NULL or candidates <= 1: a plain allocation.  Release with kt_device_free.
 * No reference counterpart: the Rust side allocates its Vecs where the allocator puts them (composition/src/oligo.rs:147). */
typedef int (*kt_probe_fn)(void *user, void *candidate_dev);
int kt_device_alloc_placed(kt_ctx *ctx, uint64_t bytes, int candidates, int launches, kt_probe_fn probe, void *user,
                           void **out, double *ms, int *n_tried, int *picked);
int kt_device_free(kt_ctx *ctx, void *ptr);

/* Page-locks / releases a host buffer of the caller (hipHostRegister) so that KT_MEM_HOST calls move it
 * by DMA at full PCIe rate instead of through the driver's pageable staging.  Optional: every entry point
 * accepts ordinary pageable memory.  Worth it for buffers that are reused over many batches (the
 * reference's batch loops, composition/src/oligo.rs:147-164, reuse theirs the same way). */
int kt_host_register(kt_ctx *ctx, void *ptr, size_t bytes);
int kt_host_unregister(kt_ctx *ctx, void *ptr);

/* ---- host-side helpers (no GPU work) ------------------------------------------ */

/* number of output bins: canonical count (count_min != 0) or 4^k.
 * replaces: `kcount` from KmerGenerator::kmer_pos_maps, kmer/src/kmer.rs:54-73;
 *           the raw-mode size in composition/src/oligo.rs:232-236 */
int kt_bins(int k, int count_min, uint64_t *bins);

/* replaces: KmerGenerator::kmer_pos_maps, kmer/src/kmer.rs:54-73.
 * min_mer_pos_map[4^k]: rank of canonical k-mer among canonicals (0 in non-canonical
 * slots, as in the reference); pos_min_mer[kcount]: rank -> canonical k-mer (the
 * reference's HashMap<pos,kmer> as a dense array).  Either may be NULL. */
int kt_pos_map(int k, uint32_t *min_mer_pos_map, uint64_t *pos_min_mer, uint32_t *kcount);

/* replaces: KmerGenerator::rev_comp, kmer/src/kmer.rs:43-52 */
uint64_t kt_rev_comp(uint64_t kmer, int k);

/* replaces: numeric_to_kmer, kmer/src/lib.rs:19-34 (out: k+1 bytes, NUL-terminated) */
int kt_numeric_to_kmer(uint64_t kmer, int k, char *out);

/* replaces: kmer_to_numeric, kmer/src/lib.rs:36-50 (no validity check, like the
 * reference; len > 32 is KT_ERR_ARG = the ValueError of pybindings/src/kmer.rs:58-63) */
int kt_kmer_to_numeric(const char *kmer, uint64_t len, uint64_t *fwd, uint64_t *rev);

/* replaces: OligoCgrComputer::cgr_maps + the per-k-mer midpoint walk,
 * composition/src/oligocgr.rs:165-189, :123-143.  xy[2*i], xy[2*i+1] = CGR point of
 * canonical k-mer i; read-independent, so computed once on the host. */
int kt_cgr_coords(int k, double vecsize, double *xy);

/* ---- device hot path ----------------------------------------------------------- */

/* replaces: KmerGenerator::new + Iterator::next, kmer/src/kmer.rs:30-41, :80-106
 * (and pybindings/src/kmer.rs:22-41).  Position-parallel form: for every base index
 * g in [0, offsets[n_reads]) valid[g] = 1 iff a k-mer ends at that base (its k bases
 * lie in one read and are all ACGTU/acgtu/0..3), and then fwd[g], rev[g] hold the
 * pair the reference's iterator yields at that position.  Iterating g in order and
 * skipping valid[g]==0 reproduces the iterator.  1 <= k <= 31. */
int kt_kmers(kt_ctx *ctx, const uint8_t *bases, const uint64_t *offsets, uint64_t n_reads,
             int k, uint64_t *fwd, uint64_t *rev, uint8_t *valid, int mem);

/* replaces: OligoComputer::vectorise_one, composition/src/oligo.rs:231-259;
 *           OligoCgrComputer::seq_to_kmer, composition/src/oligocgr.rs:145-163;
 *           python OligoComputer.vectorise_one/_batch, pybindings/src/oligo.rs:39-81.
 * out: n_reads x bins row-major (bins from kt_bins), element type out_dtype.
 * count_min: merge reverse complements (canonical bins) / 0 = raw 4^k bins.
 * norm: divide every bin by max(1, total), total = total_step * (#k-mers of the read).
 * total_step: 1 (CLI crate, oligo.rs:248,251) or 2 (python raw mode, pybindings
 * oligo.rs:61).  KT_F64 results are bit-identical to the reference (integer counts,
 * one IEEE division).  1 <= k <= 12: 3..7 (the CLI range, kmertools/src/args.rs:85) is the LDS kernel; the Python
 * class takes any k (pybindings/src/oligo.rs:22-31), so the other values count in global memory - correct, not
 * fast - up to the k whose 4^k-entry rank map the reference itself could still allocate comfortably. */
int kt_oligo_batch(kt_ctx *ctx, const uint8_t *bases, const uint64_t *offsets, uint64_t n_reads,
                   int k, int count_min, int norm, int total_step, int out_dtype, void *out,
                   int mem);

/* No counterpart in the reference (a launch detail made visible): the number of workgroups per resident slot the k = 4
 * histogram launches into the output array of the latest launch use.  It is chosen by measurement, per output array
 * (which setting is fastest goes with where the array lies in the memory: DESIGN.md 4.1): a few early large launches
 * (>= ~6 M reads of 150 bases) into an array cycle through 32 / 96 / 200 with events around them, the fastest stays.
 * *decided = 0 while still measuring (then *wgs_per_slot is the default, 96, and the means are 0); ns_per_read[3] =
 * the means for 32, 96, 200 in ns per read.  Results never depend on it.  KT_OLIGO_TUNE=0 in the environment keeps
 * the default, KT_OLIGO_OVERSUB=n fixes n.  (The trial launches record a pair of events on the context's stream.  A
 * launch made while that stream is being captured into a graph records and queries nothing - it runs with what has
 * been decided for its array, or the default, like a launch after kt_oligo_tuning(ctx, 0) - and an event that cannot be
 * created or recorded drops the trial, never the call.) */
int kt_oligo_launch_info(kt_ctx *ctx, uint32_t *wgs_per_slot, int *decided, double *ns_per_read);
/* mode 0: the launches that follow neither count towards nor take part in that measurement (they use what has been
 * decided for their array, else the default) - for a caller that is timing launches itself; mode 1 resumes;
 * mode n >= 2: as 0, and every k = 4 launch uses n workgroups per resident slot (a caller comparing shapes itself). */
int kt_oligo_tuning(kt_ctx *ctx, int mode);

/* Self-test of the f64 normalisation: the kernels compute `vec[i] /= max(1, total)` (composition/src/oligo.rs:255-257)
 * as a reciprocal + two fused multiply-adds per bin instead of a division.  For every divisor d in [d_lo, d_hi]
 * and every count c in 0..d this runs that exact device code and the IEEE division side by side:
 * *n_checked pairs, *n_mismatch of them with different bits (must be 0), *checksum = sum of the division's
 * bit patterns mod 2^64 (lets a host check the device's division itself).  Synchronises. */
int kt_selftest_quotient(kt_ctx *ctx, uint32_t d_lo, uint32_t d_hi, uint64_t *n_checked, uint64_t *n_mismatch,
                         uint64_t *checksum);

/* replaces: CountComputer::new / count_chunk's table, counter/src/lib.rs:37-55, :100.
 * One HBM-resident open-addressing table (u64 keys, u32 counts - the reference's
 * types) takes the place of the reference's n_parts scc maps and chunk files.
 * capacity_slots is rounded up to the next m * 2^j with m in 5..8 (at most 1.25x the request; at least 1024);
 * keep distinct keys <= ~70 % of it. */
int kt_ctr_create(kt_ctx *ctx, int k, uint64_t capacity_slots, kt_ctr **out);
int kt_ctr_destroy(kt_ctr *ctr);
int kt_ctr_clear(kt_ctr *ctr);
/* the slots the table really has (capacity_slots after rounding) */
int kt_ctr_capacity(kt_ctr *ctr, uint64_t *slots);

/* replaces: the hot loop of count_chunk, counter/src/lib.rs:119-131:
 * for every k-mer of every read: table[min(fwd,rev)] += 1.  Repeatable (= chunks).
 * A count is a u32 and is exact while a k-mer's occurrences, over every call that adds to the table (reads, pairs, bulk
 * merges), stay <= 0xFFFFFFFF; 0xFFFFFFFF itself is reached and read back exactly.  Beyond that the result is unspecified
 * (nothing saturates; the reference's u32 wraps silently). */
int kt_ctr_add_reads(kt_ctr *ctr, const uint8_t *bases, const uint64_t *offsets,
                     uint64_t n_reads, int mem);

/* The same, restricted to one of n_parts hash partitions: only k-mers with kt_owner_of(kmer, n_parts) == part are
 * counted.  replaces: the reference's answer to "the k-mers do not fit memory" - it cuts the input into chunks, spills
 * every chunk's partitions (`min_mer % n_parts`) to temp files and merges partition by partition
 * (counter/src/lib.rs:114-118, :127, :151-167, :188-231).  Here a table that cannot hold every distinct k-mer is
 * filled n_parts times, pass p with partition p of the whole input, exported and cleared in between: the union of
 * the exports is the complete answer (every k-mer lives in exactly one partition, with all of its occurrences). */
int kt_ctr_add_reads_part(kt_ctr *ctr, const uint8_t *bases, const uint64_t *offsets, uint64_t n_reads, int mem,
                          uint32_t n_parts, uint32_t part);

/* replaces: merge's arithmetic, counter/src/lib.rs:201-210: table[keys[i]] += counts[i]
 * (counts == NULL means 1 each: raw canonical k-mers routed from another GPU).
 * A pair with count 0 adds nothing, exactly like a KT_EMPTY_KEY entry: a key the table does not hold stays absent,
 * kt_ctr_size does not grow and a later kt_ctr_erase of that key removes nothing. */
int kt_ctr_add_pairs(kt_ctr *ctr, const uint64_t *keys, const uint32_t *counts, uint64_t n,
                     int mem);

/* Removes k-mers from the table in place: every canonical k-mer of keys[0, n) that the table holds.  Afterwards an erased
 * k-mer is absent for every reader (its count reads 0, kt_ctr_size drops; lookup, cov, profile, spectrum, compare, setop,
 * graph, unitigs and the exports see the reduced content), and a later add of it starts from 0.  Keys the table does not
 * hold, duplicates in keys, KT_EMPTY_KEY entries and values >= 4^k are ignored.  *n_erased (may be NULL) = the entries
 * removed, exact.  n == 0 is KT_OK and leaves the table as it is.  The table may be in any form (dense after a bulk build,
 * the probing image, counted into an export target - whose arrays are the caller's again afterwards, as after any call that
 * probes); what kt_ctr_export_stage staged is invalidated, as by an add.  A key cannot simply be taken out of its slot (the
 * keys behind it in its probe chain would be cut off): the survivors are compacted and the probing image is built again
 * from them, so the cost is one export plus one reload of the table whatever n is - erase in batches.  Any error leaves the
 * content exactly as it was.  KT_MEM_HOST synchronises; KT_MEM_DEVICE reads keys on the context's stream and synchronises
 * once to learn *n_erased.  KT_ERR_ARG: a null table, null keys with n > 0, a bad mem, one shard of a sharded table;
 * KT_ERR_FULL: an overflowed table.  Device scratch: 12 bytes per entry and one bit per slot. */
int kt_ctr_erase(kt_ctr *table, const uint64_t *keys, uint64_t n, uint64_t *n_erased, int mem);

/* number of distinct k-mers in the table (synchronises). KT_ERR_FULL if an insert overflowed. */
int kt_ctr_size(kt_ctr *ctr, uint64_t *distinct);

/* replaces: map.scan, counter/src/lib.rs:162-165, :220-230.  Writes up to max_out
 * (key,count) pairs in unspecified order (the reference's order is unspecified too,
 * its tests sort); *n_out = number written.  Synchronises. */
int kt_ctr_export(kt_ctr *ctr, uint64_t *keys, uint32_t *counts, uint64_t max_out,
                  uint64_t *n_out, int mem);

/* The same map.scan (counter/src/lib.rs:162-165, :220-230) in pieces, for callers that must not hold a table of billions
 * of entries in host memory at once - the reference streams its scan straight into the output file (:220-230).
 * kt_ctr_export_stage gathers the entries on the DEVICE (a staging area of the library; a table counted into an export
 * target has them there already) and returns their number; kt_ctr_export_fetch then copies entries
 * [first, first + count) to host arrays, any number of times, in any order.  The staged entries stay valid until the table
 * is changed (kt_ctr_clear, adds), staged again or given another export target - and, for a table counted into an export
 * target, until a call that probes the table (kt_ctr_lookup, kt_cov_batch, kt_ctr_profile, kt_ctr_graph, a kt_ctr_compare /
 * kt_ctr_setop that probes it, ...): such a call gives the target's arrays back to the caller.  After any of these
 * kt_ctr_export_fetch is KT_ERR_ARG until the entries are staged again. */
int kt_ctr_export_stage(kt_ctr *ctr, uint64_t *n_out);
int kt_ctr_export_fetch(kt_ctr *ctr, uint64_t first, uint64_t count, uint64_t *keys_host, uint32_t *counts_host);

/* kt_ctr_export_stage restricted to the entries with min_count <= count <= max_count (kt_ctr_export_stage is
 * (1, UINT32_MAX)); kt_ctr_export_fetch then reads the kept entries.  min_count > max_count is KT_ERR_ARG. The table
 * and an export target's arrays are not changed.  (jellyfish dump -L/-U, kmc -ci/-cx: only the kept entries cross to
 * the host.) */
int kt_ctr_export_stage_range(kt_ctr *ctr, uint32_t min_count, uint32_t max_count, uint64_t *n_out);

/* The table's abundance spectrum, ADDED into hist (the caller zeroes it once; hash-partition passes and the shards
 * of a sharded counter accumulate into one array): for 1 <= c < n_bins, hist[c] += distinct k-mers with exactly c
 * occurrences; hist[n_bins - 1] += those with n_bins - 1 or more; hist[0] is not touched.  totals (may be NULL):
 * totals[0] += distinct k-mers, totals[1] += occurrences (exact, whatever n_bins).  2 <= n_bins <= 2^24, else
 * KT_ERR_ARG; an overflowed table is KT_ERR_FULL as in kt_ctr_size.  mem: where hist / totals are.  KT_MEM_HOST
 * synchronises; KT_MEM_DEVICE is enqueued on the context's stream.  The table is not changed.
 * (jellyfish histo, kmc_tools histogram) */
int kt_ctr_spectrum(kt_ctr *ctr, uint64_t *hist, uint32_t n_bins, uint64_t *totals, int mem);

/* The comparison matrix of two tables of the same k (KAT comp / spectra-cn; with the totals, the Jaccard, containment
 * and weighted Jaccard of the two k-mer sets).  Its cell [r * n_cols + c] counts the distinct canonical k-mers with
 * min(count_a, n_rows - 1) == r and min(count_b, n_cols - 1) == c, where a count of 0 means the k-mer is absent from
 * that table.  Results are ADDED into matrix (n_rows x n_cols u64, row-major); cell [0][0] is never touched, so the
 * caller keeps 0 there.  totals (may be NULL) gets 6 u64 added, exact whatever the bin counts are:
 *   distinct_a, distinct_b, shared (in both), occurrences_a, occurrences_b,
 *   shared_min (sum over shared k-mers of min(count_a, count_b)).
 * If a and b hold the same hash partition of n_parts (kt_ctr_add_reads_part), the sum over the partitions equals the
 * call on the whole tables.  a == b is allowed (the diagonal: kt_ctr_spectrum of the table).  Neither table's content
 * changes; b is probed, so a b that is densely packed or lives in its export target gets its probing image first, as in
 * kt_ctr_lookup; a is read in whatever form it is in.  Empty tables add nothing.  mem says where matrix and totals live;
 * KT_MEM_HOST synchronises, KT_MEM_DEVICE is enqueued on the context's stream.  KT_ERR_ARG: a null table or matrix,
 * different k, tables on different contexts, a table that is one shard of a sharded table (n_owners > 1: not
 * supported), n_rows < 2, n_cols < 2, n_rows * n_cols > 2^24, a bad mem.  An overflowed table is KT_ERR_FULL as in
 * kt_ctr_size. */
int kt_ctr_compare(kt_ctr *a, kt_ctr *b, uint64_t *matrix, uint32_t n_rows, uint32_t n_cols, uint64_t *totals, int mem);

/* Which k-mers kt_ctr_compare counted: the intersection, difference, union or symmetric difference of two tables of the
 * same k as (key, count) pairs (kmc_tools simple intersect / kmers_subtract / union, meryl intersect / difference /
 * union, kat filter kmer). */
#define KT_SET_INTERSECT 0   /* in A and in B            */
#define KT_SET_SUBTRACT  1   /* in A and not in B        */
#define KT_SET_UNION     2   /* in A or in B             */
#define KT_SET_XOR       3   /* in exactly one of them   */
#define KT_SETCNT_FIRST  0   /* a' if a' != 0, else b'   */
#define KT_SETCNT_MIN    1   /* the smaller of the non-zero ones among a', b' */
#define KT_SETCNT_MAX    2   /* max(a', b')              */
#define KT_SETCNT_SUM    3   /* a' + b', saturating at 0xFFFFFFFF */
/* count_a / count_b are the tables' occurrences of a canonical k-mer, 0 when absent.  The k-mer is IN A when
 * min_a <= count_a <= max_a, IN B when min_b <= count_b <= max_b (min_* >= 1: an absent k-mer is never a member;
 * (1, UINT32_MAX) is plain presence).  a' = in A ? count_a : 0, b' likewise: a count outside its range is treated as
 * absent, in the membership test and in the count rule alike, so every emitted count is >= 1.
 * Every distinct k-mer for which op(in A, in B) holds is emitted exactly once as (key, count_rule(a', b')).  sorted == 0:
 * in unspecified order (as kt_ctr_export); sorted != 0: in ascending key order (a radix sort of the result on the
 * device).  *n_out = the number of entries that qualify, always exact.  max_out == 0 (keys / counts may be NULL) only
 * counts and stores nothing.  If 0 < max_out < *n_out, nothing past max_out is written (what is written is unsorted and
 * of no use) and the call returns KT_ERR_ARG with *n_out set, so that the caller can resize and repeat.
 * If a and b hold the same hash partition of n_parts (kt_ctr_add_reads_part), the concatenation of the outputs over the
 * partitions is the whole tables' answer (a k-mer lives in exactly one partition, in both tables); with sorted, each
 * partition's output is sorted, not the concatenation.
 * a == b is allowed.  Neither table's content changes; a table that is probed gets its probing image first, as in
 * kt_ctr_lookup / kt_ctr_compare, and the walked table's form is read only after that.  Intersect and subtract walk A
 * and probe B.  Union and xor add a second walk: B's entries whose key is absent from A's TABLE (count_a == 0, not merely
 * outside A's range - those were decided in A's walk), probing A; each key is thus visited exactly once.
 * mem says where keys / counts live.  KT_MEM_HOST synchronises; KT_MEM_DEVICE writes on the context's stream, but the
 * call still synchronises once, to learn *n_out.
 * KT_ERR_ARG: a null table or n_out, different k, tables on different contexts, a table that is one shard of a sharded
 * table (n_owners > 1: not supported), an unknown op or count_rule, min_a == 0 or min_b == 0, min_a > max_a or
 * min_b > max_b, a bad mem, null outputs with max_out > 0.  An overflowed table is KT_ERR_FULL as in kt_ctr_size.  On
 * every one of these errors the output arrays are untouched. */
int kt_ctr_setop(kt_ctr *a, kt_ctr *b, int op, int count_rule, uint32_t min_a, uint32_t max_a, uint32_t min_b, uint32_t max_b,
                 uint64_t *keys, uint32_t *counts, uint64_t max_out, uint64_t *n_out, int mem, int sorted);

/* Which k-mers of the table follow which: the de Bruijn adjacency of its k-mers, the sides at which a unitig ends, and a
 * census of the nodes (BCALM / Cuttlefish start from this; the graph-cleaning stage of a short-read assembler).
 * A canonical k-mer u of the table is a NODE when min_count <= count(u) <= max_count ("solid"; an absent k-mer has
 * count 0 and min_count >= 1, so it is never solid).  F = the forward string of u, the canonical word itself, F[0..k).
 * canon(s) = the smaller of s and its reverse complement.  The node's info word, for x in 0..3 (A C G T):
 *   bit x      (right bit x)  canon(F[1..k) + x) is solid
 *   bit 4 + x  (left bit x)   canon(x + F[0..k-1)) is solid
 *   bit 8      (right end)    dR != 1 || sibR != 1
 *   bit 9      (left end)     dL != 1 || sibL != 1
 *   bits 10..31 are 0
 * with dR = popcount of bits 0..3, dL = popcount of bits 4..7, sibR = the number of y in 0..3 with canon(y + F[1..k))
 * solid (y = F[0] is u itself and counts) and sibL = the number of y with canon(F[0..k-1) + y) solid.  The counts run
 * over x and y, not over distinct k-mers, and these formulas are the whole rule: self-loops, palindromic k-mers (even k)
 * and palindromic overlaps (hairpins) get no special case.  A side that is not an end has exactly one neighbour, whose
 * facing side is not an end either.  An info word is never 0 (a side of degree 0 is an end).
 * census (may be NULL): KT_GRAPH_CENSUS u64, ADDED into the caller's array, over the nodes:
 *   [0] nodes  [1] occurrences (sum of counts)  [2] degree sum dL + dR  [3] end sides  [4] isolated (dL == 0 && dR == 0)
 *   [5] tips (exactly one of dL, dR is 0)  [6] branching (dL > 1 || dR > 1)  [7 + 5 * dL + dR] nodes of those two degrees
 * End sides may be odd: a hairpin joins a node's side to itself, so end sides / 2 is not a unitig count.
 * Every node is emitted exactly once as (keys[i], info[i]); counts[i] (counts may be NULL) is its occurrences.
 * sorted == 0: in unspecified order; sorted != 0: in ascending key order, info and counts following their keys.
 * *n_out = the number of nodes, always exact.  max_out == 0 (the outputs may be NULL) stores nothing and still fills the
 * census.  If 0 < max_out < *n_out, nothing past max_out is written (what is written is of no use) and the call returns
 * KT_ERR_ARG with *n_out set and the census added, so that the caller can resize and repeat.
 * The table's content does not change; it is probed, so it gets its probing image first, as in kt_ctr_lookup /
 * kt_ctr_compare(a, a), and is walked in the form it then has.  An empty table gives *n_out = 0 and adds nothing.
 * One hash partition of an out-of-core count (kt_ctr_add_reads_part) cannot be used: a node's neighbours live in other
 * partitions, so the answers of partitions cannot be combined - the whole table must be resident (there is no n_parts).
 * mem says where keys / info / counts / census live.  KT_MEM_HOST synchronises; KT_MEM_DEVICE writes on the context's
 * stream, but the call still synchronises once, to learn *n_out.
 * KT_ERR_ARG: a null table or n_out, min_count == 0, min_count > max_count, a bad mem, null keys or info with
 * max_out > 0, a table that is one shard of a sharded table (n_owners > 1: not supported).  An overflowed table is
 * KT_ERR_FULL as in kt_ctr_size.  On every one of these errors the output arrays and the census are untouched. */
#define KT_GRAPH_CENSUS 32
int kt_ctr_graph(kt_ctr *table, uint32_t min_count, uint32_t max_count, uint64_t *keys, uint32_t *info, uint32_t *counts,
                 uint64_t max_out, uint64_t *n_out, uint64_t *census, int mem, int sorted);

/* The heterozygous k-mer pairs of the table: the pairs of solid k-mers that differ in exactly one base and have no other
 * such partner (Smudgeplot's hetkmers; the plot of their coverages, minor against major, shows ploidy and genome structure).
 * A node is a canonical k-mer u of the table with min_count <= count(u) <= max_count ("solid").  F = its forward string,
 * the canonical word itself; canon(s) = the smaller of s and its reverse complement: exactly kt_ctr_graph's definitions.
 * The positions P depend on `positions`:
 *   KT_HET_ALL     every i in 0..k
 *   KT_HET_MIDDLE  only i = (k - 1) / 2; odd k only, KT_ERR_ARG for even k (Smudgeplot's --middle)
 * Both sets are symmetric under i -> k - 1 - i, which is what makes the relation below symmetric.
 * N(u) is a SET: { canon(F with base i replaced by b) : i in P, b != F[i] } with u itself removed, and only its solid
 * members kept.  deg(u) = |N(u)|.  Three consequences:
 *   1. self-substitution: a substitution can lead back to u.  For odd k, F = X m rc(X) with m in {A, C} has rc(F) = F with
 *      the middle complemented.  Such a candidate is not a neighbour.
 *   2. double reach: two substitutions can reach the same neighbour, because both v and rc(v) can lie at distance 1 from
 *      F.  k = 5: N(ACCGT) = {ACAGT} - ACAGT is reached by C->A and by C->T (ACTGT = rc(ACAGT)), and C->G gives rc(ACCGT),
 *      which is ACCGT itself - so deg(ACCGT) is 1, not 2 or 3.
 *   3. symmetry: v in N(u) if and only if u in N(v).
 * A PAIR is {u, v} with N(u) = {v} and N(v) = {u}.  It is emitted exactly once, as (a, b) with a < b as canonical words;
 * each node is in at most one pair, so a is a unique sort key.  A neighbour present in the table but outside the count
 * range is not a neighbour.
 * Pair i is (keys_a[i], keys_b[i]) with occurrences counts_a[i], counts_b[i] (either counts array may be NULL).
 * sorted != 0: ascending keys_a; otherwise the order is unspecified.  *n_out = the number of pairs, always exact.
 * max_out == 0 only counts (the outputs may be NULL) and still fills matrix / census.  If 0 < max_out < *n_out, nothing
 * past max_out is written (what is written is of no use) and the call returns KT_ERR_ARG with *n_out set and matrix /
 * census added to, so that the caller can resize and repeat: kt_ctr_graph's convention.
 * matrix (may be NULL): n_rows x n_cols u64, row-major, ADDED into: cell [r * n_cols + c] += the pairs with
 * min(minor, n_rows - 1) == r and min(major, n_cols - 1) == c, minor <= major the pair's two counts (the smudge plot
 * itself).  n_rows >= 2, n_cols >= 2, n_rows * n_cols <= 2^24, as in kt_ctr_compare.
 * census (may be NULL): KT_HET_CENSUS u64, ADDED into:
 *   [0] nodes  [1] occurrences of the nodes  [2] nodes with deg == 0  [3] deg == 1  [4] deg >= 2  [5] pairs
 *   [6] sum of the minor counts over the pairs  [7] sum of the major counts (exact u64; 0xFFFFFFFF is an ordinary count)
 * The table's content does not change; it is probed, so it gets its probing image first, as in kt_ctr_graph, and is
 * walked in the form it then has.  An empty table gives *n_out = 0 and adds nothing.  The whole table must be resident
 * (there is no n_parts, for kt_ctr_graph's reason).
 * mem says where the outputs, matrix and census live.  KT_MEM_HOST synchronises; KT_MEM_DEVICE writes on the context's
 * stream, but the call still synchronises once, to learn *n_out.
 * KT_ERR_ARG: a null table or n_out, min_count == 0, min_count > max_count, unknown positions, KT_HET_MIDDLE with an even
 * k, a bad mem, null keys_a or keys_b with max_out > 0, a bad matrix shape when matrix is given, a table that is one
 * shard of a sharded table, sorted output (max_out > 0) from a table of 2^33 entries or more (the sort carries a pair's
 * index as u32).  An overflowed table is KT_ERR_FULL as in kt_ctr_size.  On every one of these errors the outputs, the
 * matrix and the census are untouched.  Device scratch: 24 bytes per table entry (the nodes' keys and the candidate pairs)
 * and, when sorted, 12 bytes per pair of room, besides kt_ctr_graph's sort. */
#define KT_HET_ALL 0
#define KT_HET_MIDDLE 1
#define KT_HET_CENSUS 8
int kt_ctr_hetmers(kt_ctr *table, uint32_t min_count, uint32_t max_count, int positions, uint64_t *keys_a, uint64_t *keys_b,
                   uint32_t *counts_a, uint32_t *counts_b, uint64_t max_out, uint64_t *n_out, uint64_t *matrix,
                   uint32_t n_rows, uint32_t n_cols, uint64_t *census, int mem, int sorted);

/* The maximal unitigs of that graph: the sequences of the compacted de Bruijn graph (what BCALM / Cuttlefish write as
 * unitigs.fa), spelled on the device.  Nodes, F, canon, the info word and "solid" are exactly kt_ctr_graph's, for the same
 * (min_count, max_count).  A side of node u (R or L) is JOINED when all of these hold:
 *   - its end bit is clear; it then has exactly one neighbour string s = F[1..k) + x (right) or x + F[0..k-1) (left);
 *   - canon(s) != F (no self-links: the homopolymer loop and the hairpin are ends);
 *   - s is not its own reverse complement, and F is not its own reverse complement (both only matter for even k).
 * The facing side of v = canon(s) is v's left side if u's right side leads to s == v, v's right side if it leads to
 * rc(s) == v (mirrored for u's left side), and that side is joined back to u.  Joined sides pair up sides of distinct
 * nodes, at most one pair per side, so the nodes fall into simple PATHS and simple CYCLES, each node in exactly one:
 * the unitigs.  A unitig of n nodes is a string of n + k - 1 bases:
 *   path   its two terminals are the nodes with an unjoined side (a single node is both).  It is spelled from the terminal
 *          with the smaller canonical k-mer, oriented so that its unjoined side comes first (a single node: as F), through
 *          the joins to the other terminal; every further node adds one base.
 *   cycle  (no unjoined side anywhere) linearised at its node with the smallest canonical k-mer: it starts with that
 *          node's F, leaves through its right side and goes once around, so the last k - 1 bases repeat the first k - 1;
 *          flag KT_UNITIG_CIRCULAR is set.
 * The unitigs ascend by the canonical k-mer of their start node (the smaller terminal, the smallest node of a cycle): the
 * result is a function of the table's content and the count range alone.
 * bases: ASCII ACGT, concatenated, no separators; offsets: max_unitigs + 1 entries, unitig i = bases[offsets[i] ..
 * offsets[i + 1]); count_sums[i] (may be NULL) = the sum of its nodes' counts; flags[i] (may be NULL) = KT_UNITIG_* bits.
 * *n_unitigs and *n_bases are always exact.  max_unitigs == 0 && max_bases == 0 only counts (the outputs may be NULL).
 * When either room is too small, nothing is written and the call returns KT_ERR_ARG with both numbers set, so that the
 * caller can resize and repeat.  The table's content does not change; it gets its probing image first, as in
 * kt_ctr_graph.  An empty table, or a range with no nodes, gives 0 / 0 and offsets[0] = 0 (unless the call only counts).
 * The whole table must be resident (there is no n_parts, for kt_ctr_graph's reason).
 * KT_MEM_HOST synchronises; KT_MEM_DEVICE writes on the context's stream and synchronises only to learn the sizes.
 * KT_ERR_ARG: a null table or null size pointers, min_count == 0, min_count > max_count, a bad mem, null bases with
 * max_bases > 0, null offsets with any room > 0, a table that is one shard of a sharded table, a table of more than
 * 2^31 - 2 entries (a node's two oriented states, 2 * index + side, are u32).  An overflowed table is KT_ERR_FULL.  On every
 * one of these errors the outputs are untouched.  Device scratch: 16 bytes per table entry and 64 per node, 48 more per node when
 * the graph has cycles, besides kt_ctr_graph's sort. */
#define KT_UNITIG_CIRCULAR 1u
int kt_ctr_unitigs(kt_ctr *table, uint32_t min_count, uint32_t max_count, uint8_t *bases, uint64_t max_bases,
                   uint64_t *offsets, uint64_t *count_sums, uint32_t *flags, uint64_t max_unitigs, uint64_t *n_unitigs,
                   uint64_t *n_bases, int mem);

/* Those unitigs and the edges between them: the compacted de Bruijn graph whole (what BCALM / Cuttlefish write as L:
 * fields, GFA as L lines).  The unitigs are exactly kt_ctr_unitigs's, for the same (min_count, max_count): the same
 * numbering, the same strings, and bases / offsets / count_sums / flags as that call fills them.
 * An ORIENTED unitig (u, +) is unitig u's string U; (u, -) is the reverse complement of U.  There is a directed LINK
 * (u, su) -> (v, sv) exactly when the last k - 1 bases of oriented (u, su) equal the first k - 1 bases of oriented (v, sv);
 * for k = 1 every pair is linked.  No pair is excluded, u == v included.  The graph is node-centric, so this is the same as:
 * the first k-mer of (v, sv) is a solid neighbour, on the outward side, of the last k-mer of (u, su).  It follows that
 *   - every link has its mirror (v, !sv) -> (u, !su); a hairpin (u, +) -> (u, -) is its own mirror;
 *   - a circular unitig has exactly the two links (u, +) -> (u, +) and (u, -) -> (u, -);
 *   - a k-mer that follows itself gives (u, +) -> (u, +);
 *   - a unitig that is its own reverse complement is a single palindromic node (even k only) and is linked under both signs;
 *   - an end has at most 5 links: one per set neighbour bit of its terminal node's outward nibble and one more where that
 *     neighbour is such a palindrome (odd k: at most 4).
 * END e = 2 * u + (su is '-') owns link_to[link_offsets[e] .. link_offsets[e + 1]); each value is 2 * v + (sv is '-'),
 * ascending within an end (unitig numbers are below 2^31).  link_offsets: 2 * max_unitigs + 1 entries; link_to: max_links.
 * *n_links = the number of directed links, always exact, as *n_unitigs and *n_bases are.  max_bases == 0 && max_unitigs == 0
 * && max_links == 0 only counts (the outputs may be NULL).  When any of the three rooms is too small, nothing is written and
 * the call returns KT_ERR_ARG with all three numbers set.  No nodes: 0 / 0 / 0 and offsets[0] = link_offsets[0] = 0 (unless
 * the call only counts).  KT_MEM_HOST synchronises; KT_MEM_DEVICE writes on the context's stream and synchronises to learn the
 * sizes and, after the links are written, that every neighbour stood at an end of its unitig (if not: KT_ERR_HIP).
 * KT_ERR_ARG: what kt_ctr_unitigs refuses (a room > 0 includes max_links), a null n_links, null link_offsets with any room
 * > 0, null link_to with max_links > 0, max_links > 0 with max_unitigs == 0.  On every one of these errors the outputs are
 * untouched.  Device scratch: kt_ctr_unitigs's and 8 bytes per unitig. */
int kt_ctr_unitigs_linked(kt_ctr *table, uint32_t min_count, uint32_t max_count, uint8_t *bases, uint64_t max_bases,
                          uint64_t *offsets, uint64_t *count_sums, uint32_t *flags, uint64_t max_unitigs, uint64_t *n_unitigs,
                          uint64_t *n_bases, uint64_t *link_offsets, uint32_t *link_to, uint64_t max_links, uint64_t *n_links,
                          int mem);

/* Which of those unitigs are TIPS - the short dead ends that sequencing errors leave hanging off the true path (what
 * Bifrost -i clips and -d deletes, what BCALM / minia remove before compacting again).  One round, read-only: marks[u] is
 * for unitig u of kt_ctr_unitigs's numbering for the same (min_count, max_count).  The rule reads kt_ctr_unitigs_linked's
 * outputs alone, so it holds for every k.  n_u = unitig u's nodes (bases - k + 1), c_u = its count sum; end e = 2u + (sign is
 * '-') owns the links links[e] with values f = 2v + (sv is '-'); a link e -> f arrives at end f ^ 1 of unitig f >> 1, and its
 * mirror is (f ^ 1) -> (e ^ 1).  u is SHORT when it is not circular and n_u <= max_tip_nodes.
 *   - a short u with no link at either end: KT_TIP_ISOLATED;
 *   - a short u with no link at exactly one end is a CANDIDATE, e its live end;
 *   - w BEATS a candidate u when w is no candidate, or w is one and c_w / n_w > c_u / n_u, or the two are equal and w < u
 *     (compared exactly, as 128-bit products);
 *   - a candidate u is KT_TIP_TIP when for EVERY link f of its live end, end g = f ^ 1 has a link h != e ^ 1 whose unitig
 *     h >> 1 beats u;
 *   - everything else: KT_TIP_KEEP.
 * So at a fork whose branches are all short dead ends the best one (highest mean count, then lowest number) stays, an end
 * that had links keeps at least one of them among the unmarked unitigs, and a trunk that is itself a short dead end is not
 * clipped by its own branches.
 * tally (may be NULL; KT_TIP_TALLY values, overwritten): [0] tips, [1] their nodes, [2] isolated short unitigs, [3] their
 * nodes.  *n_unitigs is always exact.  max_unitigs == 0 only counts (marks may be NULL) and still fills tally; when
 * 0 < max_unitigs < *n_unitigs nothing is written and the call returns KT_ERR_ARG with the number set.  The table is not
 * changed (it gets its probing image first, as in kt_ctr_graph).  KT_MEM_HOST synchronises; KT_MEM_DEVICE writes marks and
 * tally on the context's stream and synchronises to learn the sizes.  KT_ERR_ARG: what kt_ctr_unitigs_linked refuses,
 * max_tip_nodes == 0, a null n_unitigs, null marks with max_unitigs > 0; KT_ERR_FULL: an overflowed table.  On every error the
 * outputs are untouched.  Device scratch: kt_ctr_unitigs_linked's with 20 + 4 * links / unitigs bytes per unitig in place
 * of the base array, and 2 bytes per unitig. */
#define KT_TIP_KEEP 0
#define KT_TIP_TIP 1
#define KT_TIP_ISOLATED 2
#define KT_TIP_TALLY 4
int kt_ctr_unitig_tips(kt_ctr *table, uint32_t min_count, uint32_t max_count, uint32_t max_tip_nodes, uint8_t *marks,
                       uint64_t max_unitigs, uint64_t *n_unitigs, uint64_t *tally, int mem);

/* Clip, recompact, repeat.  Each round takes the marks of kt_ctr_unitig_tips and erases from the table (kt_ctr_erase, the
 * keys listed on the device: no trip to the host) the nodes of every KT_TIP_TIP unitig and, with KT_CLIP_ISOLATED in flags,
 * of every KT_TIP_ISOLATED one; the next round sees the unitigs of what is left, so that a tip on a tip goes in two rounds.
 * The call stops after the first round that erases nothing, or after max_rounds rounds (1..1024).  Entries outside
 * [min_count, max_count] are no nodes and are never touched.
 * stats (host memory, may be NULL; KT_CLIP_STATS values, overwritten): [0] rounds that erased something, [1] tips clipped,
 * [2] tip nodes erased, [3] isolated unitigs dropped, [4] isolated nodes erased, [5] occurrences erased, [6] 1 if the last
 * round still erased something (stopped by max_rounds: another call may find more), else 0, [7] 0.
 * An error in round r leaves the table as rounds 0 .. r - 1 left it, and stats describes those rounds.  Synchronises.
 * KT_ERR_ARG: what kt_ctr_unitig_tips refuses, max_rounds outside 1..1024, flags other than KT_CLIP_ISOLATED.  Device
 * scratch: kt_ctr_unitig_tips's and 8 bytes per node for the list, then kt_ctr_erase's. */
#define KT_CLIP_ISOLATED 1u
#define KT_CLIP_STATS 8
int kt_ctr_clip_tips(kt_ctr *table, uint32_t min_count, uint32_t max_count, uint32_t max_tip_nodes, uint32_t max_rounds,
                     uint32_t flags, uint64_t *stats);

/* Which of those unitigs are the weaker sides of BUBBLES - the short parallel paths that a SNP, a small indel or a repeated
 * sequencing error leaves between the same two points (Velvet's tour bus, minia's and SPAdes' bulge removal, Bifrost's
 * simplification).  One round, read-only, in kt_ctr_unitig_tips' vocabulary: n_u, c_u, end e = 2u + (sign is '-') and its
 * links f = 2v + (sv is '-'); a link e -> f arrives at end f ^ 1 of unitig f >> 1, its mirror is (f ^ 1) -> (e ^ 1).  The
 * rule reads kt_ctr_unitigs_linked's outputs alone, so it holds for every k.
 *   - u is a BRANCH when it is not circular, n_u <= max_bubble_nodes, end 2u has exactly one link a, end 2u + 1 has exactly
 *     one link b, and a >> 1 != u and b >> 1 != u;
 *   - branches u != w are PARALLEL when the unordered pairs {a_u, b_u} and {a_w, b_w} are equal (unordered: w may lie the
 *     other way round between the same two ends).  Parallel is an equivalence: a branch is in exactly one class;
 *   - w OUTRANKS u when c_w / n_w > c_u / n_u, or the two are equal and w < u (compared exactly, as 128-bit products);
 *   - a branch is KT_BUBBLE_POP when some parallel branch outranks it; everything else is 0.
 * So exactly one branch of every class stays, and it keeps both anchors joined.  An anchor end (a ^ 1, b ^ 1) of a class of
 * two or more has at least two links, so an anchor is never a branch and is never popped.  A popped unitig has links at both
 * ends, so it is never a tip candidate, and an anchor that is a tip candidate is never a tip: the branch end that faces it
 * has no other link that could beat it.  KT_BUBBLE_POP is a bit of its own beside KT_TIP_TIP and KT_TIP_ISOLATED, one mark
 * byte carries both rules, and the tips' invariant holds for the union of both marks: an end of an unmarked unitig that had
 * links keeps at least one of them among the unmarked unitigs.
 * The search is one-sided: branch u looks through the at most 5 links h of end a ^ 1; w = h >> 1 != u is parallel exactly
 * when it is a branch and the single link of its end h equals b (its end h ^ 1 links to a, the mirror of h).
 * tally (may be NULL; KT_BUBBLE_TALLY values, overwritten): [0] popped unitigs, [1] their nodes, [2] bubbles (classes of two
 * or more), [3] occurrences popped.  Shapes, the count-only form, KT_ERR_ARG cases, untouched outputs on error, KT_MEM_HOST and
 * KT_MEM_DEVICE: exactly as in kt_ctr_unitig_tips, with max_bubble_nodes == 0 refused.  Device scratch: kt_ctr_unitig_tips'
 * less one byte per unitig (the rule keeps no class array). */
#define KT_BUBBLE_POP 4
#define KT_BUBBLE_TALLY 4
int kt_ctr_unitig_bubbles(kt_ctr *table, uint32_t min_count, uint32_t max_count, uint32_t max_bubble_nodes, uint8_t *marks,
                          uint64_t max_unitigs, uint64_t *n_unitigs, uint64_t *tally, int mem);

/* Clip tips and pop bubbles in the same rounds.  Each round is one linked run whose unitigs are marked by the tip rule when
 * max_tip_nodes > 0 and by the bubble rule when max_bubble_nodes > 0 (both 0: KT_ERR_ARG); one list and one kt_ctr_erase take
 * the nodes of every KT_TIP_TIP and KT_BUBBLE_POP unitig and, with KT_CLIP_ISOLATED in flags (valid only with
 * max_tip_nodes > 0), of every KT_TIP_ISOLATED one.  The next round sees the unitigs of what is left: a bubble behind a tip
 * pops in the round after the tip went.  The call stops as kt_ctr_clip_tips does.
 * stats (host memory, may be NULL; KT_SIMPLIFY_STATS values, overwritten): [0] rounds that erased something, [1] tips,
 * [2] tip nodes, [3] isolated unitigs, [4] isolated nodes, [5] unitigs popped, [6] their nodes, [7] bubbles, [8] occurrences
 * erased, [9] 1 if the last round still erased something (stopped by max_rounds), else 0, [10], [11] 0.
 * With max_bubble_nodes == 0 the table afterwards and stats [0..4], [8], [9] are kt_ctr_clip_tips' table and stats [0..4],
 * [5], [6] for the same arguments.  Errors as in kt_ctr_clip_tips: an error in round r leaves the table as rounds 0 .. r - 1
 * left it and stats describes those rounds; a refusal in round 0 leaves stats untouched.  Synchronises.  Device scratch:
 * kt_ctr_clip_tips'. */
#define KT_SIMPLIFY_STATS 12
int kt_ctr_simplify(kt_ctr *table, uint32_t min_count, uint32_t max_count, uint32_t max_tip_nodes, uint32_t max_bubble_nodes,
                    uint32_t max_rounds, uint32_t flags, uint64_t *stats);

/* Where the table's entries are wanted - told BEFORE counting, so that counting can deliver them there.
 * replaces: the same map.scan as kt_ctr_export (counter/src/lib.rs:162-165, :220-230), for the usual life of a
 * table: filled once, written out once.  keys_dev / counts_dev are DEVICE arrays of max_out entries owned by the
 * caller.  From now on (sticky; NULL, NULL, 0 switches it off) every whole-batch count into an EMPTY table
 * (kt_ctr_add_reads / kt_sharded_add_reads after creation or kt_ctr_clear) writes its (key, count) pairs straight
 * into these arrays as the last step of the build, and kt_ctr_size / kt_ctr_export(keys_dev, counts_dev, ...) then
 * only report the number of entries - no second pass over the table.  The table keeps referring to the arrays
 * (entries [0, size) in unspecified order; what lies beyond them in the arrays is unspecified) until the next call that changes or probes it (a further add, kt_cov_batch,
 * an export elsewhere, a new target), which first rebuilds its own probing copy from them: leave them untouched
 * until then, or call kt_ctr_clear.  If the arrays turn out too small, the call that counted returns KT_ERR_ARG AFTER
 * having built the table in its own slots: nothing is lost - kt_ctr_size, kt_ctr_export into arrays of that size, further
 * adds all work - and the target arrays hold nothing usable (they are never written past max_out). */
int kt_ctr_export_target(kt_ctr *ctr, uint64_t *keys_dev, uint32_t *counts_dev, uint64_t max_out);

/* ---- table files ("ktab" version 1, DESIGN.md, Table files): a counted table on disk (KMC databases, jellyfish .jf, meryl) ----
 * No reference counterpart: the reference writes text (counter/src/lib.rs:220-230) and reads nothing back.
 * A file is a 16-byte header ("KTAB", u32 version, u32 k, u32 0) and one or more SECTIONS up to its end; a section is a
 * sorted run of (canonical key, count) entries: a 32-byte header ("KSEC", u32 S, u64 n, u64 n_overflow, u64 occurrences)
 * and, with P = max(0, 2k - 8S), u64 offsets[2^P + 1], n * S suffix bytes, n count bytes (255 = the next value of the
 * overflow list), n_overflow * u32, padding to 8 bytes.  A key may appear in several sections; on load its counts add. */

/* Host only (no context, no GPU): the file's k, its sections and the sums of their headers' entries and occurrences
 * (any of the four may be NULL).  Checks the file header, the chain of section headers and every section's length against
 * the file's size.  KT_ERR_ARG: a null path; KT_ERR_IO: unreadable or malformed, kt_last_error() names the first thing
 * that was wrong. */
int kt_table_file_info(const char *path, int *k, uint64_t *sections, uint64_t *entries, uint64_t *occurrences);

/* Host only: the full structural validation - what kt_table_file_info checks, S in 1..8 and P <= 24, n_overflow <= n,
 * nothing behind the last section, and every section's offsets[]: offsets[0] == 0, never decreasing, none above n, the
 * last one == n.  Everything a kernel could index by; the content (keys ascending, canonical and below 4^k, count bytes,
 * overflow values, the sums) is validated on the device by kt_ctr_add_file.  Reads the offsets in pieces of 8 MiB. */
int kt_table_file_check(const char *path);

/* Writes the table's entries with min_count <= count <= max_count as ONE section: creates the file (written under a
 * temporary name beside it and renamed into place), or with append != 0 and an existing file adds a section to it (the
 * file must be a whole table file of the table's k; a failure truncates it back to what it was).  No error leaves a partial
 * section behind.  The entries are staged as by kt_ctr_export_stage_range (what was staged before is replaced), copied,
 * sorted and packed on the device; the parts cross to the host through two page-locked slabs of 8 MiB.  For a given k the section's bytes are
 * a function of the set of (key, count) alone: not of the table's form, capacity or history.  The table's content is not
 * changed, in whatever form it is (probing image, dense after a bulk build, counted into an export target, direct).
 * *n_saved (may be NULL) = the entries written; an empty selection writes an empty section.  Synchronises.
 * KT_ERR_ARG: a null table or path, min_count > max_count, append to a file of another k; KT_ERR_FULL: an overflowed
 * table; KT_ERR_IO: the file cannot be written (or, with append, is not a valid table file).  Device scratch: 24 bytes
 * per entry for the copy and its sort, S + 9 per entry and 8 * 2^P for the parts. */
int kt_ctr_save(kt_ctr *table, const char *path, uint32_t min_count, uint32_t max_count, int append, uint64_t *n_saved);

/* table[key] += count for every entry of every section of the file, section by section through kt_ctr_add_pairs on the
 * device (so the table may hold entries already, and keys that several sections share add up).  kt_table_file_check runs
 * before the first launch; each section's content is validated by the kernels that unpack it, with every index clamped: a
 * bad file gives KT_ERR_IO, never an access out of bounds.  A section that fails adds nothing and ends the call; the
 * sections before it stay added.  *n_added (may be NULL) = the entries of the sections added (not the growth of
 * kt_ctr_size: keys the table held stay one entry).  Synchronises.  KT_ERR_ARG: a null table or path, a file of another
 * k; KT_ERR_FULL as kt_ctr_add_pairs (seen by the next kt_ctr_size).  Device scratch: S + 17 bytes per entry of the
 * largest section and 8 * 2^P. */
int kt_ctr_add_file(kt_ctr *table, const char *path, uint64_t *n_added);

/* replaces: CgrComputer::vectorise_one, composition/src/cgr.rs:127-144 (corners from cgr_maps,
 * :12-36) and python CgrComputer.vectorise_one/_batch, pybindings/src/cgr.rs:38-62.
 * Whole-sequence chaos game walk: xy[2*g], xy[2*g+1] = marker after base g of the batch
 * (g = global base index, so read i owns xy[2*offsets[i] .. 2*offsets[i+1])); every read
 * starts from (vecsize/2, vecsize/2).  Bit-identical to the reference's serial f64 walk.
 * A byte outside ACGTUacgtu is an error for the whole call, as in the reference:
 * *bad_pos (may be NULL) = lowest offending base index, UINT64_MAX if none.  KT_MEM_HOST:
 * returns KT_ERR_BADNT in that case; KT_MEM_DEVICE: bad_pos is a device pointer the caller
 * inspects after synchronising (the call itself returns KT_OK). */
int kt_cgr_points(kt_ctx *ctx, const uint8_t *bases, const uint64_t *offsets, uint64_t n_reads,
                  double vecsize, double *xy, uint64_t *bad_pos, int mem);

/* replaces: MinimiserGenerator::new + Iterator::next, kmer/src/minimiser.rs:36-56, :61-175 (and
 * python MinimiserGenerator, pybindings/src/min.rs:24-47; the per-record loops of
 * misc/src/minimisers.rs:43-54, :124-135).  For every read, in iterator order, the triples
 * (minimiser, window start, window end) the reference yields; read i owns entries
 * [ev_offsets[i], ev_offsets[i+1]) of kmers/starts/ends (starts/ends are read-local, ends
 * exclusive).  wsize = 0 means "the read's own length" (one minimiser per read,
 * misc/src/minimisers.rs:44-48); otherwise msize <= wsize (windows of more than 4096 m-mers: a two-level
 * sliding minimum in front of the same kernel, three scratch arrays of one m-mer per base; windows of 2^30 bases and
 * more take a one-read-per-thread path: correct, and parallel across reads only).
 * 1 <= msize <= 31.  Quirks of the iterator are kept (a change on the last base swallows the
 * final window; a last run shorter than the window reports UINT64_MAX).  Reads shorter than msize
 * yield nothing with wsize = 0 (the reference's capacity arithmetic underflows there).
 * Always synchronises.  *n_events = number of triples.  capacity = room in kmers/starts/ends:
 * 0 counts only (ev_offsets is then unspecified); if 0 < capacity < *n_events the first
 * `capacity` triples are written and KT_ERR_ARG is returned. */
int kt_minimisers(kt_ctx *ctx, const uint8_t *bases, const uint64_t *offsets, uint64_t n_reads,
                  uint64_t wsize, int msize, uint64_t *ev_offsets, uint64_t *kmers,
                  uint64_t *starts, uint64_t *ends, uint64_t capacity, uint64_t *n_events, int mem);

/* replaces: CovComputer::vectorise_one, coverage/src/lib.rs:165-184 (and the HashMap
 * re-load of kmers.counts at :82-92: the table is probed where kt_ctr_add_reads left it).
 * For every canonical k-mer of a read (k = the table's k): count = table[kmer] or 0,
 * bin = min(count / bin_size, bin_count - 1); out row = histogram of the bins, divided
 * by max(1, #k-mers of the read) when norm != 0.  out: n_reads x bin_count row-major,
 * element type out_dtype (KT_U32 needs norm = 0).  KT_F64 results are bit-identical to
 * the reference (integer counts, one IEEE division).  bin_size, bin_count >= 1. */
int kt_cov_batch(kt_ctr *table, const uint8_t *bases, const uint64_t *offsets, uint64_t n_reads,
                 uint64_t bin_size, uint64_t bin_count, int norm, int out_dtype, void *out,
                 int mem);

/* counts[i] = occurrences of the canonical k-mer keys[i] in the table, 0 when it is absent (`mem` says where keys and
 * counts live).  replaces: the HashMap get of coverage/src/lib.rs:170 (`kmer_counts.get(&kmer)`), one key at a time. */
int kt_ctr_lookup(kt_ctr *table, const uint64_t *keys, uint64_t n, uint32_t *counts, int mem);

/* The same lookups against a table that holds only PART of the k-mers - one hash partition of an out-of-core count
 * (kt_ctr_add_reads_part: n_parts passes, the table refilled for each) or one shard of a sharded table (n_parts = 1).
 * Only the k-mers this table answers for are binned (a k-mer of another partition is not "absent": it is skipped), as
 * raw u32 counts ADDED to `counts` (n_reads x bin_count, zeroed by the caller before the first part; `mem` says where
 * it lives).  Summed over the parts - modulo 2^32, cell by cell - every k-mer of every read has been binned exactly
 * once: the rows kt_cov_batch gives with KT_U32; normalisation (count / max(1, sum of the row),
 * coverage/src/lib.rs:180-182) is then one division per cell.  (A shard does not know which k-mers the other shards
 * hold without their minimisers: shard 0's pass puts every k-mer into bin 0, and the shard that holds a k-mer moves it
 * from there to its bin - a shard's own rows mean nothing before they are summed.)
 * replaces: coverage/src/lib.rs:69-92 + :165-184 for inputs whose k-mers do not fit one table. */
int kt_cov_batch_part(kt_ctr *table, const uint8_t *bases, const uint64_t *offsets, uint64_t n_reads,
                      uint64_t bin_size, uint64_t bin_count, uint32_t *counts, int mem, uint32_t n_parts,
                      uint32_t part);

/* Per-read k-mer solidity against the table (the read filter, `kmertools filter`).  A read's k-mers are its valid windows
 * (a window holding a non-ACGT byte is none, as for every other k-mer walk here), canonical; a k-mer's count is the
 * table's, 0 when absent.  A k-mer is SOLID when min_count <= count <= max_count (min_count >= 1: an absent k-mer is
 * never solid), WEAK otherwise.  Per read i, for the k-mers of hash partition `part` of n_parts:
 *   n_kmers[i]    += the k-mers,
 *   n_solid[i]    += the solid ones,
 *   first_weak[i]  = min(first_weak[i], start in the read of the first weak one) - 0xFFFFFFFF when there is none.
 * The caller initialises the arrays once to 0 / 0 / 0xFFFFFFFF; combined over parts 0..n_parts-1 (the tables of an
 * out-of-core count, kt_ctr_add_reads_part) they are the whole table's answer.  first_weak may be NULL (its work is
 * then skipped).  `mem` says where bases, offsets and the three arrays live; KT_MEM_HOST synchronises.
 * KT_ERR_ARG: min_count == 0, min_count > max_count, part >= n_parts, a bad mem, a null buffer with n_reads > 0, a read
 * of 2^32 bases or more (positions are u32), or a table that is one shard of a sharded table (n_owners > 1: a shard
 * cannot tell a k-mer absent here from one absent everywhere - shards are not supported).
 * The count compared is the table's own: a k-mer with 0xFFFFFFFF occurrences is solid for max_count == 0xFFFFFFFF, also
 * with min_count == 0xFFFFFFFF.  (kt_ctr_profile caps what it writes at 0xFFFFFFFE; kt_ctr_correct_support's "covered"
 * reads that profile and so differs for exactly this k-mer - see there.) */
int kt_ctr_read_solidity(kt_ctr *table, const uint8_t *bases, const uint64_t *offsets, uint64_t n_reads,
                         uint32_t min_count, uint32_t max_count, uint32_t *n_kmers, uint32_t *n_solid,
                         uint32_t *first_weak, int mem, uint32_t n_parts, uint32_t part);

/* Per-position k-mer counts against the table (`kmertools profile`, the coverage track of a sequence).  `profile` has
 * offsets[n_reads] u32 entries, indexed by the global base index g (as the xy of the CGR points call is).  Every valid window that
 * STARTS at base g (inside one read, no non-ACGT byte - as for every other k-mer walk here) and whose canonical k-mer
 * belongs to hash partition `part` of n_parts gets profile[g] = min(count, 0xFFFFFFFE); a k-mer absent from the table
 * has count 0.  Every other entry is NOT WRITTEN: the last k-1 positions of a read, windows over an N, reads shorter
 * than k, k-mers of other partitions.  The caller fills the array with KT_NO_KMER once; after parts 0..n_parts-1 (the
 * tables of an out-of-core count) it is the whole table's answer.  There is no read-length limit: positions are global.
 * `mem` says where bases, offsets and profile live; KT_MEM_HOST synchronises, KT_MEM_DEVICE is enqueued on the
 * context's stream.
 * KT_ERR_ARG: part >= n_parts, a bad mem, a null buffer with n_reads > 0, or a table that is one shard of a sharded
 * table (as for the read solidity call). */
#define KT_NO_KMER 0xFFFFFFFFu
int kt_ctr_profile(kt_ctr *table, const uint8_t *bases, const uint64_t *offsets, uint64_t n_reads, uint32_t *profile,
                   int mem, uint32_t n_parts, uint32_t part);

/* Per-read statistics of such a profile (any u32 array of offsets[n_reads] entries: no table, no k).  For read i, over
 * its entries that are not KT_NO_KMER:
 *   n_kmers[i]   = how many there are,            n_present[i] = those with count >= 1,
 *   min_count[i] / max_count[i] = the least / greatest,   sum[i] = their exact sum (u64),
 *   median[i]    = element n_kmers / 2 (0-based) of them sorted ascending - the upper median of an even number, the
 *                  convention of khmer's get_median_count.
 * A read with no k-mer gets 0 in every output.  Any output pointer may be NULL (its work is then skipped); the others
 * are overwritten, not accumulated.  `mem` says where all the arrays live; KT_MEM_HOST synchronises.
 * KT_ERR_ARG: a bad mem, a null input with n_reads > 0, a read of 2^32 bases or more. */
int kt_profile_stats(kt_ctx *ctx, const uint32_t *profile, const uint64_t *offsets, uint64_t n_reads, uint32_t *n_kmers,
                     uint32_t *n_present, uint32_t *min_count, uint32_t *median, uint32_t *max_count, uint64_t *sum,
                     int mem);

/* k-mer spectrum error correction of reads against the table (`kmertools correct`; what Musket, Lighter and BFC do on the
 * CPU).  replaces: nothing - the reference has no such operation.  Two calls, split as kt_ctr_profile / kt_profile_stats
 * are: this one needs the table and adds over hash partitions, kt_correct_apply is a pure function of arrays.
 * The rule is decided from the UNCORRECTED read, base by base, so no order of evaluation matters.  A window is k
 * consecutive bases inside one read, named by the global index j of its first base; a k-mer is solid when
 * min_count <= count <= max_count, as in kt_ctr_read_solidity.  For base g of read [o, o') the windows that contain it
 * are j in [max(o, g - k + 1), min(g, o' - k)].
 *   covered   g is covered when one of those windows is valid and solid.  That is taken from `profile`, the COMPLETE
 *             answer of kt_ctr_profile for the same batch (offsets[n_reads] entries, all partitions done): window j counts
 *             iff profile[j] != KT_NO_KMER and min_count <= profile[j] <= max_count.  No probe is made for it, and a
 *             profile the caller made up works as well.  A covered base is trusted; so is every base of a read shorter
 *             than k.
 *   support   for an uncovered g (its own byte may be valid or not) and every nucleotide x in 0..3 other than its own
 *             code, s(g, x) = the number of those windows in which every byte other than g is valid and whose canonical
 *             k-mer, with x written at g, is solid.  Byte x (bits 8x .. 8x+7) of support[g] GAINS the part of s(g, x)
 *             whose substituted k-mers belong to hash partition `part` of n_parts.  The caller zeroes `support`
 *             (offsets[n_reads] u32 entries) once; summed over parts 0..n_parts-1 a byte is at most k <= 31, so no byte
 *             carries into the next.  Entries of covered bases and of reads shorter than k are not written.
 * `mem` says where bases, offsets, profile and support live; KT_MEM_HOST synchronises, KT_MEM_DEVICE is enqueued on the
 * context's stream.  KT_ERR_ARG: min_count == 0, min_count > max_count, part >= n_parts, a bad mem, a null buffer with
 * n_reads > 0, or a table that is one shard of a sharded table (as for the read solidity call).
 * The two ends of u32: KT_NO_KMER is 0xFFFFFFFF, so a k-mer with 0xFFFFFFFF occurrences reads as 0xFFFFFFFE in a profile.
 * "covered" sees that value: with max_count == 0xFFFFFFFF the k-mer covers for every min_count <= 0xFFFFFFFE, and with
 * min_count == 0xFFFFFFFF it does not cover - although it is solid for kt_ctr_read_solidity and, in `support`, for the
 * substituted k-mers, which are probed in the table and compared with their real count. */
int kt_ctr_correct_support(kt_ctr *table, const uint8_t *bases, const uint64_t *offsets, uint64_t n_reads,
                           const uint32_t *profile, uint32_t min_count, uint32_t max_count, uint32_t *support, int mem,
                           uint32_t n_parts, uint32_t part);

/* The decision over such a support array (no table, no k: its bytes are compared with min_support and that is all).
 * Base g is SINGLE when exactly one byte of support[g] is >= min_support, AMBIGUOUS when two or more are.
 *   n_single[i] / n_ambiguous[i] = the single / ambiguous bases of read i (overwritten; either may be NULL),
 *   out_bases[g] = "ACGT"[x] at the single bases of the reads with n_single <= max_corrections (0: no limit) - a read that
 *                  needs more repairs than that is left as it is -, bases[g] everywhere else: case, N, U and raw codes
 *                  untouched, ambiguous bases never changed.  Every byte of the batch is written.  May be NULL (counts
 *                  only) and may be `bases` itself (in place).
 * There is no second round: repairing a base cannot uncover another one, and two errors closer than k with no solid
 * window between them stay.  `mem` says where all the arrays live; KT_MEM_HOST synchronises.
 * KT_ERR_ARG: min_support == 0 or > 255, a bad mem, a null input with n_reads > 0, a read of 2^32 bases or more. */
int kt_correct_apply(kt_ctx *ctx, const uint8_t *bases, const uint64_t *offsets, uint64_t n_reads, const uint32_t *support,
                     uint32_t min_support, uint32_t max_corrections, uint8_t *out_bases, uint32_t *n_single,
                     uint32_t *n_ambiguous, int mem);

/* Reads threaded onto the unitigs of a table (`kmertools thread`; what Bifrost query, GGCAT query and GraphAligner's exact
 * mode answer on the CPU).  replaces: nothing - the reference has no such operation.  Three calls: the first makes a table
 * whose "count" is a k-mer's position in a set of sequences, the second looks a batch's k-mers up in it and orients the
 * answer, the third - a pure function of arrays, split off as kt_profile_stats and kt_correct_apply are - folds the per-base
 * answers into runs along the unitigs.
 *
 * kt_ctr_index_sequences: `index` is an EMPTY table of the sequences' k, created and sized by the caller (room for one entry
 * per window).  Every valid window (inside one sequence, ACGT only, as in every k-mer walk here) that starts at global base G
 * with forward k-mer f and reverse complement r puts key min(f, r) with value 1 + 2 * G + S into the table: S = 1 when f > r
 * (the sequence shows the reverse complement of the canonical k-mer), S = 0 otherwise, a palindrome included.  The value is
 * the key's "count" for every reader of the table (kt_ctr_lookup returns it).  *n_kmers = the number of windows.
 * The sequences must hold every canonical k-mer at most once.  That is so for the unitigs of kt_ctr_unitigs: every solid
 * k-mer lies in exactly one unitig, once; a circular unitig repeats its first k - 1 bases but no k-mer; a palindromic node is
 * a unitig of its own.  `mem` says where bases and offsets live; both kinds synchronise (the check below needs the size).
 * KT_ERR_ARG: a null index or n_kmers, a bad mem, a null buffer with n_seqs > 0, one shard of a sharded table, a table that
 * is not empty, offsets[n_seqs] > 2^31 - 2 (the value must stay at or below 0xFFFFFFFE; decided from the offsets alone, before
 * any base is read), and a table that holds fewer entries than *n_kmers after the build: a k-mer occurred twice and its values
 * added up - the message says so, *n_kmers is set and the table is cleared.  KT_ERR_FULL as in kt_ctr_add_pairs.
 * Device scratch: 12 bytes per base. */
int kt_ctr_index_sequences(kt_ctr *index, const uint8_t *bases, const uint64_t *offsets, uint64_t n_seqs, uint64_t *n_kmers,
                           int mem);

/* Oriented positions per base: kt_ctr_profile's contract (`hits` has offsets[n_reads] u32 entries indexed by global base,
 * only valid window starts are written, the caller fills with KT_NO_KMER once) with another value.  A k-mer absent from
 * the index gives 0.  A present one with table value v = 1 + 2 * G + S gives 1 + ((v - 1) ^ t): the slot's word 2 * G + S with
 * t folded into its low bit, where t = 1 when the read shows the reverse complement of the canonical k-mer (f > r) and 0
 * otherwise.  So (hits[j] - 1) >> 1 is G, and bit 0 of hits[j] - 1 is a = S ^ t: 1 means the read runs antiparallel to the
 * indexed sequence there.  The strand comes out of the one walk that makes the key; no second pass is made.
 * There is no n_parts: the index must be resident, as for kt_ctr_graph.  KT_MEM_HOST synchronises, KT_MEM_DEVICE is enqueued
 * on the context's stream.  KT_ERR_ARG: a null index, a bad mem, a null buffer with n_reads > 0, one shard of a sharded table. */
int kt_ctr_thread_hits(kt_ctr *index, const uint8_t *bases, const uint64_t *offsets, uint64_t n_reads, uint32_t *hits, int mem);

/* Such hits folded into RUNS along the unitigs (no table: a function of the arrays).  hits: read_offsets[n_reads] entries;
 * unitig_offsets: n_unitigs + 1 entries, the offsets of the sequences that were indexed; k: their k-mer size (1..31).
 * With G_j = (hits[j] - 1) >> 1 and a_j = (hits[j] - 1) & 1, position j is a HIT when hits[j] is neither 0 nor KT_NO_KMER,
 * G_j < unitig_offsets[n_unitigs] and the window lies inside its unitig: with u_j the unitig that holds base G_j
 * (unitig_offsets[u] <= G_j < unitig_offsets[u + 1]) and p_j = G_j - unitig_offsets[u_j], p_j <= len_u - k.  Any other
 * value that is neither 0 nor KT_NO_KMER is no hit and is counted as a bad value.
 * j CONTINUES j - 1 when both are hits of the same read, a_j == a_{j-1}, u_j == u_{j-1} and G_j == G_{j-1} + 1 (a = 0) or
 * G_j == G_{j-1} - 1 (a = 1).  (For k >= 2 the unitig condition follows from the others; for k = 1 it does not.)  A RUN is a
 * maximal stretch of positions each continuing the one before; a walk around a circular unitig starts a new run where it
 * wraps.  Runs are numbered by ascending j.  Per run: run_start = the global read base of its first k-mer, run_len = its
 * k-mers, run_unitig = 2 * u + a, run_upos = p of its first k-mer in read order (the greatest p of an antiparallel run).
 * run_offsets (n_reads + 1 entries, may be NULL): run_offsets[i] = the first run of read i, run_offsets[n_reads] = *n_runs.
 * unitig_hits[u] / unitig_runs[u] (n_unitigs u64 each, may be NULL) are ADDED to - the hits and the runs on unitig u -, so the
 * caller zeroes them once and accumulates over batches; they are added to by a call that writes runs (max_runs > 0) only, so
 * that the counting call and the one sized by it do not add twice.  tally (may be NULL; KT_THREAD_TALLY u64, overwritten):
 * [0] windows (entries other than KT_NO_KMER), [1] hits, [2] misses (value 0), [3] bad values, [4] runs, [5] reads with at
 * least one hit.
 * *n_runs is always exact.  max_runs == 0 only counts (the run arrays may be NULL) and still fills run_offsets and tally;
 * 0 < max_runs < *n_runs writes nothing and returns KT_ERR_ARG with the number set.  KT_MEM_HOST synchronises; KT_MEM_DEVICE
 * writes on the context's stream and synchronises to learn the sizes.  KT_ERR_ARG: a null ctx or n_runs, a bad mem, k outside
 * 1..31, a null input with n_reads > 0 (null unitig_offsets with n_unitigs > 0), a null run array with max_runs > 0, a read of
 * 2^32 bases or more, more than 2^31 - 1 unitigs or unitig bases.  On every one of these errors the outputs are untouched.
 * Device scratch: one bit per read base and per unitig base, 16 bytes per 1024 read bases. */
#define KT_THREAD_TALLY 6
int kt_thread_runs(kt_ctx *ctx, const uint32_t *hits, const uint64_t *read_offsets, uint64_t n_reads,
                   const uint64_t *unitig_offsets, uint64_t n_unitigs, int k, uint64_t *run_start, uint32_t *run_len,
                   uint32_t *run_unitig, uint32_t *run_upos, uint64_t *run_offsets, uint64_t max_runs, uint64_t *n_runs,
                   uint64_t *unitig_hits, uint64_t *unitig_runs, uint64_t *tally, int mem);

/* Which unitigs hang together: the weakly CONNECTED COMPONENTS of the unitig graph (`kmertools unitigs --components`; what
 * khmer's partitioning, Bandage's component view and every binning front end start from).  replaces: nothing - the reference
 * has no such operation.  No table: a function of the arrays kt_ctr_unitigs_linked leaves, in its vocabulary - end
 * e = 2 * u + sign owns link_to[link_offsets[e] .. link_offsets[e + 1]), and a value f joins unitig e >> 1 to unitig f >> 1.
 *   - a link joins its two unitigs whatever its direction; its mirror need not be present;
 *   - a link to oneself (a circular unitig, a hairpin) joins nothing;
 *   - a value f >= 2 * n_unitigs is a BAD link: counted, otherwise ignored (an end may own any number of links).
 * component (n_unitigs u32): components are numbered by their smallest unitig, ascending - component[0] == 0,
 * component[u] <= u, and a new number appears exactly at a component's smallest member.  The result is a function of the
 * arrays alone: two calls give the same bytes.
 * stats (may be NULL with max_components == 0): KT_COMPONENT_FIELDS u64 per component, *n_components rows overwritten:
 * [0] unitigs, [1] nodes = the sum of len - (k - 1) over its unitigs (0 when unitig_offsets is NULL; unitig_offsets:
 * n_unitigs + 1 entries as kt_ctr_unitigs gives them), [2] the sum of count_sums (0 when it is NULL), [3] the directed links its
 * ends own, bad ones not counted, [4] its smallest unitig.
 * tally (may be NULL; KT_COMPONENT_TALLY u64, overwritten): [0] components, [1] components of one unitig, [2] the most unitigs
 * in one component, [3] the most nodes in one, [4] bad links, [5] the rounds the labelling took - informational, the only
 * value that may differ between two calls.
 * *n_components is always exact and component is written whenever the call succeeds.  max_components == 0 writes no stats;
 * 0 < max_components < *n_components writes nothing and returns KT_ERR_ARG with the number set (n_unitigs rows always
 * suffice).  n_unitigs == 0: *n_components = 0, a zeroed tally, nothing is launched.  KT_MEM_HOST synchronises; KT_MEM_DEVICE
 * writes on the context's stream and synchronises to learn the sizes and, once per round, whether the labelling has settled.
 * KT_ERR_ARG, each decided before anything is read, the outputs untouched: a null ctx or n_components, a bad mem, null
 * link_offsets, link_to or component with n_unitigs > 0, null stats with max_components > 0, n_unitigs > 2^31 - 1, k outside
 * 1..32 when unitig_offsets is given; and link_offsets[0] > link_offsets[2 * n_unitigs].  KT_ERR_HIP with an internal-error
 * text if the labelling has not settled after n_unitigs + 1 rounds (it takes O(log n_unitigs)).
 * Device scratch: 4 bytes per unitig and 4 per link, 16 per 1024 unitigs, 40 per component when stats is not the caller's
 * device array; a host call's copies of its arrays besides. */
#define KT_NO_COMPONENT 0xFFFFFFFFu
#define KT_COMPONENT_FIELDS 5
#define KT_COMPONENT_TALLY 6
int kt_unitig_components(kt_ctx *ctx, const uint64_t *link_offsets, const uint32_t *link_to, uint64_t n_unitigs,
                         const uint64_t *unitig_offsets, const uint64_t *count_sums, int k, uint32_t *component,
                         uint64_t *stats, uint64_t max_components, uint64_t *n_components, uint64_t *tally, int mem);

/* The reads of a batch split by component (`kmertools thread --components`): a fold of kt_thread_runs' run arrays
 * (run_unitig, run_len: run_offsets[n_reads] entries; run_offsets: n_reads + 1) over kt_unitig_components' component array
 * (n_unitigs entries, numbers below n_components).  A run is BAD when its unitig run_unitig >> 1 is >= n_unitigs or that
 * unitig's component is >= n_components; bad runs are counted and otherwise ignored.
 * read_component[i] (u32) = the component of read i's first run that is not bad, KT_NO_COMPONENT when it has none;
 * read_mixed[i] (u8, may be NULL) = 1 when a later run of the read lies in another component, else 0.
 * comp_reads[c] / comp_hits[c] (n_components u64 each, may be NULL) are ADDED to - one per read at its component; every
 * run's run_len at that run's own component -, so the caller zeroes them once and accumulates over batches.
 * tally (may be NULL; KT_READ_COMPONENT_TALLY u64, overwritten): [0] reads with a component, [1] reads without, [2] mixed
 * reads, [3] bad runs.
 * The work is linear in the runs: a read of up to 8 runs is one lane's, a longer one is walked by its whole wave.
 * KT_MEM_HOST synchronises; KT_MEM_DEVICE writes on the context's stream and synchronises to learn the number of runs.
 * KT_ERR_ARG: a null ctx, a bad mem, null run_offsets or read_component with n_reads > 0, null component with
 * n_unitigs > 0, a null run array when there are runs, n_unitigs > 2^31 - 1, n_components > n_unitigs.  On every one of
 * these errors the outputs are untouched.  Device scratch: 64 bytes; a host call's copies of its arrays besides. */
#define KT_READ_COMPONENT_TALLY 4
int kt_thread_read_components(kt_ctx *ctx, const uint32_t *run_unitig, const uint32_t *run_len, const uint64_t *run_offsets,
                              uint64_t n_reads, const uint32_t *component, uint64_t n_unitigs, uint64_t n_components,
                              uint32_t *read_component, uint8_t *read_mixed, uint64_t *comp_reads, uint64_t *comp_hits,
                              uint64_t *tally, int mem);

/* Bottom-s MinHash sketches of the reads of a batch (`kmertools sketch`; what Mash does, and sourmash with `num`).
 * replaces: nothing - the reference has no such operation.  No table is involved.
 * A read's k-mers are its valid windows, canonical, as for every other k-mer walk here (1 <= k <= 31); a k-mer's hash is
 * splitmix64's finaliser of (k-mer ^ seed) - a bijection of the 64-bit words, so distinct k-mers have distinct hashes:
 *   z = (kmer ^ seed) + 0x9e3779b97f4a7c15; z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9;
 *   z = (z ^ (z >> 27)) * 0x94d049bb133111eb; hash = z ^ (z >> 31).
 * Row i of `hashes` (hashes[i*s .. i*s+s)) = the s smallest DISTINCT hashes of read i, ascending; sizes[i] = how many there
 * are = min(s, distinct k-mers of the read), 0 for a read shorter than k or without a valid window; the entries at and
 * after sizes[i] are KT_EMPTY_KEY.  sizes is the authority: a hash may in principle equal KT_EMPTY_KEY.  n_kmers[i] (may
 * be NULL) = the windows of read i, counted with multiplicity.  Every output element is overwritten.  The result is exact
 * for every input (repeats included) and a function of the inputs alone.
 * `mem` says where bases, offsets and the outputs live; KT_MEM_HOST synchronises, KT_MEM_DEVICE is enqueued on the
 * context's stream (after one read-back of the longest read's length).
 * KT_ERR_ARG: k outside 1..31, s outside 1..KT_SKETCH_MAX_S, a bad mem, a null buffer with n_reads > 0, a read of 2^32
 * bases or more. */
#define KT_SKETCH_MAX_S 16384
int kt_sketch_batch(kt_ctx *ctx, const uint8_t *bases, const uint64_t *offsets, uint64_t n_reads, int k, uint32_t s,
                    uint64_t seed, uint64_t *hashes, uint32_t *sizes, uint32_t *n_kmers, int mem);

/* Sketches of unions: row g of out_hashes (n_groups rows of s, out_sizes[g] entries, KT_EMPTY_KEY behind them) = the s
 * smallest distinct hashes among rows group_offsets[g] .. group_offsets[g+1] of `hashes` (n rows of s, sizes[i] entries
 * each, strictly ascending - the layout kt_sketch_batch writes; an empty group gives size 0).  Exact: the bottom-s of a
 * union of bottom-s sets is the bottom-s of the union of the sets - the sketch of a sample given in several batches, or
 * of all the records of a file.  out_hashes must not overlap hashes.  `mem` as above.
 * KT_ERR_ARG: s outside 1..KT_SKETCH_MAX_S, a bad mem, a null buffer with n_groups > 0, group_offsets that decrease or
 * end above n. */
int kt_sketch_merge(kt_ctx *ctx, const uint64_t *hashes, const uint32_t *sizes, uint64_t n, uint32_t s,
                    const uint64_t *group_offsets, uint64_t n_groups, uint64_t *out_hashes, uint32_t *out_sizes, int mem);

/* Mash's merge walk for every pair (row i of A, row j of B), both n x s in kt_sketch_batch's layout:
 *   denom[i*n_b + j]  = min(s, |A_i u B_j|)   (may be NULL),
 *   shared[i*n_b + j] = how many of the denom smallest hashes of A_i u B_j are in both.
 * The full n_a x n_b matrices, row-major; a_hashes == b_hashes is allowed (all against all: the matrix is symmetric, the
 * diagonal is (size, size)).  Rows must be strictly ascending within their size: a precondition, not checked.  `mem` as
 * above.  KT_ERR_ARG: s outside 1..KT_SKETCH_MAX_S, a bad mem, a null buffer with n_a, n_b > 0. */
int kt_sketch_pairs(kt_ctx *ctx, const uint64_t *a_hashes, const uint32_t *a_sizes, uint64_t n_a, const uint64_t *b_hashes,
                    const uint32_t *b_sizes, uint64_t n_b, uint32_t s, uint32_t *shared, uint32_t *denom, int mem);

/* The Mash distance of such a pair (host helper, the one implementation of the formula): j = shared / denom (0 when
 * denom == 0); 1 when j == 0, else min(1, -ln(2j / (1 + j)) / k); j == 1 gives 0. */
double kt_mash_distance(uint32_t shared, uint32_t denom, int k);

/* ---- scaled (FracMinHash) sketches (`kmertools sketch --scaled`; what sourmash does with `scaled`) --------------------
 * replaces: nothing - the reference has no such operation.
 *   Hash of a window: h = mix64(canonical k-mer ^ seed), the formula printed above kt_sketch_batch, 1 <= k <= 31; a window
 *   over a byte that is no nucleotide is none, as everywhere.
 *   max_hash(scaled) = 0xFFFFFFFFFFFFFFFF / scaled (integer division, scaled >= 1; scaled == 0 is KT_ERR_ARG).  A hash is
 *   KEPT when h <= max_hash; scaled = 1 keeps every k-mer.
 *   A scaled sketch is the set of kept hashes, distinct and strictly ascending.  Every hash has an ABUNDANCE, how often its
 *   k-mer occurred: a u32 that saturates at 0xFFFFFFFF where sums are formed, like KT_SETCNT_SUM.
 *   The sketches of many sequences lie CSR: hashes[row_offsets[i] .. row_offsets[i+1]), abunds parallel to it, row_offsets of
 *   n + 1 u64 with row_offsets[0] == 0.
 * So the size of a sketch follows the content, the sketch of a union is the union of the sketches, and |A n B| / |A| is
 * an unbiased estimate of the containment of A in B whatever the two sizes.  This is the project's hash, not sourmash's.
 * Sizes, as in kt_ctr_unitig_tips: *n_out (a host word) is always exact; max_out == 0 only counts - the data arrays may be
 * NULL, the offsets (and n_kmers, totals) are still filled -; with 0 < max_out < *n_out nothing else is written and the call
 * returns KT_ERR_ARG with *n_out set.  On every error the outputs are untouched.  `mem` says where every array lives;
 * KT_MEM_HOST synchronises, KT_MEM_DEVICE runs on the context's stream and synchronises only to learn sizes.
 * Every result is exact and a function of the inputs alone. */

/* the largest kept hash; 0 for scaled == 0 */
uint64_t kt_scaled_max_hash(uint64_t scaled);

/* The containment-to-ANI estimate (host helper, the one implementation of the formula): (shared / size)^(1/k); 0 when shared
 * or size is 0, 1 when shared == size. */
double kt_containment_ani(uint64_t shared, uint64_t size, int k);

/* Row i = the scaled sketch of read i, its abundances the number of windows of that read with that k-mer (abunds may be
 * NULL).  n_kmers[i] (u32 per read, may be NULL) = the read's windows with multiplicity.  n_reads == 0 sets *n_out = 0 and
 * touches nothing else.
 * KT_ERR_ARG: k outside 1..31, scaled == 0, a bad mem, a null ctx, n_out, offsets or row_offsets, null hashes with
 * max_out > 0, a read of 2^32 bases or more, a batch whose kept windows, with multiplicity, number 2^32 or more.
 * Device scratch: 16 bytes per 8192 bases, then about 70 bytes per kept window. */
int kt_scaled_batch(kt_ctx *ctx, const uint8_t *bases, const uint64_t *offsets, uint64_t n_reads, int k, uint64_t scaled,
                    uint64_t seed, uint64_t *hashes, uint32_t *abunds, uint64_t max_out, uint64_t *row_offsets, uint32_t *n_kmers,
                    uint64_t *n_out, int mem);

/* Sketches of unions: row g of the output = the union of rows group_offsets[g] .. group_offsets[g+1] of the input (n_rows
 * rows in the CSR layout above; abunds NULL = 1 each), abundances summed, saturating.  An empty group gives an empty row;
 * out_offsets has n_groups + 1 entries; out_abunds may be NULL.  n_groups == 0 sets *n_out = 0 and touches nothing else.
 * Input rows must be strictly ascending: a precondition, not checked.  Outputs must not overlap inputs.
 * KT_ERR_ARG: a bad mem, a null ctx, n_out, row_offsets, group_offsets or out_offsets, null hashes where the groups hold
 * any, null out_hashes with max_out > 0, group offsets that decrease or end above n_rows, groups that hold 2^32 hashes or
 * more in all (with multiplicity).  Device scratch: about 80 bytes per hash of the groups. */
int kt_scaled_merge(kt_ctx *ctx, const uint64_t *hashes, const uint32_t *abunds, const uint64_t *row_offsets, uint64_t n_rows,
                    const uint64_t *group_offsets, uint64_t n_groups, uint64_t *out_hashes, uint32_t *out_abunds, uint64_t max_out,
                    uint64_t *out_offsets, uint64_t *n_out, int mem);

/* The scaled sketch of the table's entries whose count lies in [min_count, max_count] - the SOLID k-mers of a read set with
 * min_count = 2 -, abunds (may be NULL) = their counts.  totals (may be NULL, in `mem`, overwritten): [0] the entries in
 * the count range, [1] the sum of their counts.  A walker like kt_ctr_spectrum: the table is read in the form it is in, is
 * not brought to its probing image, keeps a staged export and is left unchanged.
 * KT_ERR_ARG: min_count == 0 or > max_count, scaled == 0, a bad mem, a null table or n_out, null hashes with max_out > 0,
 * one shard of a sharded table, 2^32 kept entries or more; KT_ERR_FULL: an overflowed table.
 * Device scratch: about 60 bytes per kept entry. */
int kt_ctr_scaled(kt_ctr *table, uint32_t min_count, uint32_t max_count, uint64_t scaled, uint64_t seed, uint64_t *hashes,
                  uint32_t *abunds, uint64_t max_out, uint64_t *n_out, uint64_t *totals, int mem);

/* shared[i*n_b + j] (u32, n_a x n_b row-major) = |A_i n B_j| for two sets of sketches in the CSR layout above.
 * a_hashes == b_hashes (with the same offsets) is allowed: the matrix is symmetric, its diagonal the sizes.  Rows are of any
 * length, 0 included; they must be strictly ascending (a precondition).  n_a == 0 or n_b == 0 touches nothing.
 * KT_ERR_ARG: a bad mem, a null ctx, null offsets or shared, null hashes where rows hold any, a row of 2^32 entries or
 * more. */
int kt_scaled_pairs(kt_ctx *ctx, const uint64_t *a_hashes, const uint64_t *a_offsets, uint64_t n_a, const uint64_t *b_hashes,
                    const uint64_t *b_offsets, uint64_t n_b, uint32_t *shared, int mem);

/* HyperLogLog registers of the distinct canonical k-mers of a batch (`kmertools card`, `--estimate-size`; what ntCard, KMC's
 * estimator and Jellyfish's size hint give their users).  replaces: nothing - the reference has no such operation.  No
 * table is involved.
 *   m = 2^p registers of one byte, q = 64 - p.
 *   A read's k-mers are its valid windows, canonical, as for every other k-mer walk here (1 <= k <= 31).
 *   h = mix64(kmer ^ seed), the formula printed above kt_sketch_batch.
 *   Register index j = h >> q.
 *   Rank r = 1 + (number of leading zeros of the low q bits of h, taken as a q-bit word): r = q + 1 when those bits are all
 *   zero, and r lies in 1..q+1.
 *   registers[j] = max(registers[j], r).
 * Like kt_ctr_spectrum the call combines into what the caller passes: the caller zeroes the array once; batches,
 * hash-partition passes and files accumulate into one array; a batch added in two calls, in either order, gives the
 * registers of one call with both.  *n_kmers (may be NULL) += the windows, with multiplicity.
 * `mem` says where bases, offsets, registers and n_kmers live; KT_MEM_HOST synchronises, KT_MEM_DEVICE is enqueued on the
 * context's stream.  n_reads == 0 is KT_OK and touches nothing.
 * KT_ERR_ARG: k outside 1..31, p outside KT_CARD_MIN_P..KT_CARD_MAX_P, a bad mem, a null buffer with n_reads > 0, a read of
 * 2^32 bases or more. */
#define KT_CARD_MIN_P 4
#define KT_CARD_MAX_P 16
int kt_card_add_reads(kt_ctx *ctx, const uint8_t *bases, const uint64_t *offsets, uint64_t n_reads, int k, int p,
                      uint64_t seed, uint8_t *registers, uint64_t *n_kmers, int mem);

/* into[j] = max(into[j], from[j]) for the 2^p registers of two host arrays: the registers of the union of what the two
 * arrays have seen (same k, p and seed).  KT_ERR_ARG: p outside KT_CARD_MIN_P..KT_CARD_MAX_P, a null array. */
int kt_card_merge(uint8_t *into, const uint8_t *from, int p);

/* The number of distinct k-mers behind 2^p registers (a host array): Ertl's improved raw estimator, which needs no bias
 * tables, evaluated in doubles in exactly this order.  C[v] = number of registers equal to v, for v = 0..q+1 (a register
 * above q + 1 is KT_ERR_ARG), m = 2^p:
 *   z = m * tau(1 - C[q+1]/m);  for v = q down to 1: z = 0.5 * (z + C[v]);  z += m * sigma(C[0]/m)
 *   estimate = (m*m / (2 ln 2)) / z
 *   sigma(x): x == 1 -> +inf; y = 1, z = x; repeat { x *= x; z' = z; z += x*y; y += y } until z' == z
 *   tau(x):   x == 0 or x == 1 -> 0; y = 1, z = 1 - x; repeat { x = sqrt(x); z' = z; y *= 0.5; z -= (1-x)^2 * y } until z' == z;
 *             return z/3
 * All-zero registers give 0.  *zero_registers (may be NULL) = C[0].  KT_ERR_ARG also: p out of range, a null array. */
int kt_card_estimate(const uint8_t *registers, int p, double *estimate, uint64_t *zero_registers);

/* the estimator's relative standard error, 1.04 / sqrt(2^p) */
double kt_card_rel_error(int p);

/* A two-pass pre-filter that keeps k-mers seen once (in a read set: mostly sequencing errors) out of a table - what
 * BFCounter, Jellyfish's --bf-size and KMC's pre-filter give their users.  replaces: nothing - the reference has no such
 * operation.  The filter is two arrays of 64-bit words on the device, `once` of 2^log2_once words and `twice` of
 * 2^log2_twice, each exponent in KT_PREFILTER_MIN_LOG2..KT_PREFILTER_MAX_LOG2.  For a canonical k-mer m:
 *   h = mix64(m ^ seed), the formula printed above kt_sketch_batch.
 *   once word = h >> (64 - log2_once); once pattern = the OR of 1 << ((h >> 6 j) & 63) for j = 0..3.
 *   g = mix64(h); the twice word and pattern come from g the same way, with log2_twice.
 * All bits of a k-mer lie in one word of each array, so one atomic OR sets them and tells whether they were set before.
 * Pass 1 (kt_prefilter_add_reads), per valid window: when the once word does not cover the pattern it is OR-ed in, and the
 * k-mer is done if the value returned did not cover it either (first sighting).  Otherwise - the k-mer was seen before, by
 * the load or by the atomic's return value, or it is a false positive - its twice pattern is OR-ed in, unless the word covers
 * it already; a promotion is counted when the value that OR returned did not cover the pattern.  Two lanes with the same
 * k-mer serialise on one atomic of one word, so the second always sees the first.
 * Pass 2 (kt_ctr_add_reads_filtered) counts the k-mers whose twice pattern is covered.
 * The guarantee: after pass 1 over an input and pass 2 over the same input into an empty table, every k-mer with two or
 * more occurrences is in the table with its exact count; every other key of the table has count 1 and occurs exactly once
 * in the input.  Which k-mers seen once get in depends on the order of execution, how many is bounded by the false-positive
 * rate of the two arrays; nothing else is nondeterministic (`once` itself is the OR of all patterns, whatever the order).
 * So every reader that ignores count 1 (min_count >= 2) gives what it gives on the unfiltered table. */
typedef struct kt_prefilter kt_prefilter;
#define KT_PREFILTER_MIN_LOG2 10
#define KT_PREFILTER_MAX_LOG2 34
/* Both arrays zeroed.  KT_ERR_ARG: null pointers, k outside 1..31, an exponent out of range; KT_ERR_NOMEM. */
int kt_prefilter_create(kt_ctx *ctx, int k, int log2_once, int log2_twice, uint64_t seed, kt_prefilter **out);
int kt_prefilter_destroy(kt_prefilter *filter);
/* every bit and every counter back to zero */
int kt_prefilter_clear(kt_prefilter *filter);
/* Pass 1 over a CSR batch.  Batches accumulate; the final `once` array does not depend on their order.  `mem` says where
 * bases and offsets live; KT_MEM_HOST synchronises, KT_MEM_DEVICE is enqueued on the context's stream.  n_reads == 0 is
 * KT_OK.  KT_ERR_ARG: a null filter, a bad mem, a null buffer with n_reads > 0, a read of 2^32 bases or more. */
int kt_prefilter_add_reads(kt_prefilter *filter, const uint8_t *bases, const uint64_t *offsets, uint64_t n_reads, int mem);
/* Host outputs, each may be NULL: the windows walked and the promotions counted by every pass-1 call since the last clear,
 * and the bits set in the two arrays now.  Synchronises. */
int kt_prefilter_stats(kt_prefilter *filter, uint64_t *windows, uint64_t *promotions, uint64_t *once_bits_set,
                       uint64_t *twice_bits_set);
/* out[i] = (once covers the pattern of keys[i] ? 1 : 0) | (twice covers it ? 2 : 0) for n canonical k-mers: the
 * membership test of the two passes restated.  `mem` says where keys and out live. */
int kt_prefilter_query(kt_prefilter *filter, const uint64_t *keys, uint64_t n, uint8_t *out, int mem);
/* kt_ctr_add_reads_part through the filter: only k-mers whose twice pattern is covered are added.  Always the probing
 * path, so it works on a table in any form (the table is brought to its probing image first, what was staged for export is
 * dropped), and on one that already holds data.  KT_ERR_ARG also: a null filter, a filter of another context or another k. */
int kt_ctr_add_reads_filtered(kt_ctr *ctr, kt_prefilter *filter, const uint8_t *bases, const uint64_t *offsets,
                              uint64_t n_reads, int mem, uint32_t n_parts, uint32_t part);

/* Multi-GPU routing step (the reference's `min_mer % n_parts` partitioning,
 * counter/src/lib.rs:127, re-expressed as hash-prefix ownership):
 * writes every canonical k-mer of the reads into keys_out grouped by owner
 * o = kt_owner_of(kmer, n_owners); owner_counts[o] = group sizes (groups are
 * contiguous, in owner order).  keys_out needs room for offsets[n_reads] entries
 * (upper bound).  owner_counts follows `mem`.  1 <= n_owners <= 64. */
int kt_ctr_route(kt_ctx *ctx, const uint8_t *bases, const uint64_t *offsets, uint64_t n_reads,
                 int k, int n_owners, uint64_t *keys_out, uint64_t *owner_counts, int mem);

/* ---- k-mer counting sharded over the GPUs of a node (ownership by hash prefix of the k-mer's minimiser) -----------
 * replaces: the `n_parts` partitioning of counter/src/lib.rs:100,127,243-247 and the per-partition merge of
 * :188-231 - the partitions are GPUs.  Rank o (one process or thread, one kt_ctx, one GPU) counts the k-mers whose
 * MINIMISER - the canonical m-mer inside the k-mer with the smallest hash (kmer/src/minimiser.rs:61-175 defines a
 * minimiser; m = kt_shard_minimiser(k)) - hashes into its share of the hash range: owner = mix(min hash) * N >> 32,
 * kt_sharded_owner_of / kt_shard_owner_of.  Both strands of a k-mer hold the same canonical m-mers, and consecutive
 * k-mers of a read mostly share their minimiser: a read falls into a few runs of k-mers with one owner each, and what
 * the ranks send each other is the runs' bases at 2 bits (records of at most 8 k-mers in 10 bytes: ~1.7 bytes per k-mer
 * at k = 31), not the k-mers at 8 bytes.  Every rank's shard is a whole table of its own (kt_sharded_table).
 * kt_sharded_add_reads and kt_sharded_finalize are COLLECTIVE: every rank calls them the same number of times (a rank
 * without reads passes n_reads = 0).  Each rank routes its own reads into one region of records per owner, the ranks
 * tell each other the regions' sizes, the regions travel in pieces (grouped ncclSend / ncclRecv from librccl over xGMI,
 * or the caller's host all-to-all) while the partition passes of the ordinary single-GPU pipeline already run over what
 * has arrived.  Results stay sharded: the union of the ranks' exports is the answer (the reference's output order is
 * unspecified anyway).  With n_ranks == 1 everything degenerates to kt_ctr_add_reads.  A rank that cannot take part in
 * a collective call (a batch larger than agreed, a pending table that overflowed) still enters the exchange that
 * carries the ranks' status, and EVERY rank returns an error - none is left waiting. */
typedef struct kt_sharded kt_sharded;

/* 128-byte RCCL unique id (ncclGetUniqueId): rank 0 makes it, the caller hands it to the other ranks (any channel:
 * MPI, a file, torch.distributed's store) */
int kt_rccl_unique_id(uint8_t *id128);

/* capacity_slots: slots of this rank's shard (a table of its own: size it for the k-mers one rank will own - about
 * 1 / n_ranks of the distinct k-mers, more where a few minimisers dominate); max_batch_bases: the largest batch any
 * rank will pass to kt_sharded_add_reads - it fixes the room of the exchange regions, so it must be the same on every
 * rank (a mismatch is reported by every rank at the first kt_sharded_add_reads). */
int kt_sharded_create_rccl(kt_ctx *ctx, int k, uint64_t capacity_slots, uint64_t max_batch_bases, int n_ranks, int rank,
                           const uint8_t *id128, kt_sharded **out);

/* host transport: `fn(user, send, recv, bytes_per_rank)` must move block p of `send` (host memory, n_ranks blocks of
 * bytes_per_rank) to rank p and fill block p of `recv` with what rank p sent to this rank; returns 0 on success.
 * The library stages the device regions through page-locked host memory around the call. */
typedef int (*kt_alltoall_fn)(void *user, const void *send, void *recv, uint64_t bytes_per_rank);
int kt_sharded_create_host(kt_ctx *ctx, int k, uint64_t capacity_slots, uint64_t max_batch_bases, int n_ranks, int rank,
                           kt_alltoall_fn fn, void *user, kt_sharded **out);
/* The same in two steps, for callers that want to agree between them: kt_sharded_create_local allocates everything
 * (the shard, the exchange buffers) and needs no peer; once EVERY rank has succeeded (the caller's own barrier: a
 * rank whose allocation failed never enters ncclCommInitRank, where its peers would wait for it), kt_sharded_connect_rccl
 * / kt_sharded_connect_host brings the transport up. */
int kt_sharded_create_local(kt_ctx *ctx, int k, uint64_t capacity_slots, uint64_t max_batch_bases, int n_ranks, int rank,
                            kt_sharded **out);
int kt_sharded_connect_rccl(kt_sharded *s, const uint8_t *id128);
int kt_sharded_connect_host(kt_sharded *s, kt_alltoall_fn fn, void *user);
int kt_sharded_destroy(kt_sharded *s);
int kt_sharded_clear(kt_sharded *s);

/* collective.  replaces: count_chunk's loop for one chunk of this rank's records, counter/src/lib.rs:119-131 */
int kt_sharded_add_reads(kt_sharded *s, const uint8_t *bases, const uint64_t *offsets, uint64_t n_reads, int mem);

/* collective; call once after the last kt_sharded_add_reads and before reading the shard: delivers the k-mers that
 * did not fit their exchange region (batches dominated by few k-mers).  replaces: merge, counter/src/lib.rs:172-234 */
int kt_sharded_finalize(kt_sharded *s);

/* this rank's shard, an ordinary table: kt_ctr_size / kt_ctr_export / kt_cov_batch work on it (owned by `s`) */
int kt_sharded_table(kt_sharded *s, kt_ctr **table);

/* bytes this rank has sent to other ranks so far (a single rank made to route into n regions, KT_SHARD_FORCE = n: the
 * bytes of the regions a rank of n would have sent) */
int kt_sharded_exchanged_bytes(kt_sharded *s, uint64_t *bytes);

/* what the route pass of this rank's LAST batch put into every owner's region: records[o] records holding kmers[o] k-mers
 * (arrays of 64; *n_owners = the owners: n_ranks, or KT_SHARD_FORCE's regions of a single rank).  max / mean of kmers[]
 * over the owners is the imbalance the minimiser ownership costs.  (no reference counterpart: statistics) */
int kt_sharded_route_stats(kt_sharded *s, uint32_t *n_owners, uint64_t *records, uint64_t *kmers);

/* what carries the exchange: *n_ranks = the ranks this counter was created for; *rccl_ranks = what the library's own
 * RCCL communicator reports (ncclCommCount on the communicator kt_sharded_connect_rccl made; 0 when the transport is the
 * caller's host all-to-all or the counter has a single rank and no communicator); *transport = 0 none (one rank, no
 * exchange), 1 librccl ncclSend / ncclRecv, 2 the caller's host all-to-all.  A benchmark line that claims N GPUs can
 * show that RCCL saw N ranks.  (no reference counterpart: statistics) */
int kt_sharded_comm_info(kt_sharded *s, int *n_ranks, int *rccl_ranks, int *transport);

/* the rank that owns a canonical k-mer in this sharded table (host helper, the function the device uses) */
int kt_sharded_owner_of(kt_sharded *s, uint64_t kmer, uint32_t *owner);

/* The same without a counter or a GPU: the minimiser length m and the window w = k - m + 1 (m-mers per k-mer) the
 * sharded counter uses for k-mers of length k, and the rank that owns a k-mer (either strand) among n_ranks.
 * replaces: `min_mer % n_parts`, counter/src/lib.rs:127 */
int kt_shard_minimiser(int k, uint32_t *m, uint32_t *w);
uint32_t kt_shard_owner_of(uint64_t kmer, int k, uint32_t n_ranks);

/* hash partition of a canonical k-mer among n_owners (host helper, same function the device uses): what
 * kt_ctr_add_reads_part and kt_ctr_route split by - the LOW hash bits, independent of a table's slot bits. */
uint32_t kt_owner_of(uint64_t kmer, uint32_t n_owners);

/* Synthetic reads for benchmarks/parity, generated in HBM:
 * bases_dev[n_reads*read_len], offsets_dev[n_reads+1] (may be NULL).  Deterministic
 * in (seed, first_read + i, pos); genome_len == 0: i.i.d. uniform ACGT, else reads
 * sampled from a random genome_len-bp genome (both strands, 1 % substitutions);
 * noise: ~0.1 % N, ~1 % lower case.  Device pointers only. */
int kt_synth_reads(kt_ctx *ctx, uint64_t seed, uint64_t first_read, uint64_t n_reads,
                   uint32_t read_len, int noise, uint64_t genome_len, uint8_t *bases_dev,
                   uint64_t *offsets_dev);

#ifdef __cplusplus
}
#endif
#endif /* KMERTOOLS_HIP_H */
