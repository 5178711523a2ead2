// computers.hpp - C++ mirror of the reference's Rust-level operator API for the hot path:
//   OligoComputer      composition/src/oligo.rs:15-93
//   OligoCgrComputer   composition/src/oligocgr.rs:16-121
//   CgrComputer        composition/src/cgr.rs:42-144
//   CountComputer      counter/src/lib.rs:22-90, 172-234
//   CovComputer        coverage/src/lib.rs:14-184
//   seq_to_min / bin_sequences   misc/src/minimisers.rs:11-160 (free functions there too)
// Same constructor arguments, setters and entry points (vectorise / count / merge); the
// per-read / per-k-mer work goes through the C ABI (include/kmertools_hip.h) to the GPU.
// The reference's error style is kept: vectorise() returns "" on success or the message that
// the CLI prints after "Error: ".
#pragma once
#include <stdint.h>

#include <functional>
#include <string>
#include <vector>

#include "../../../include/kmertools_hip.h"

namespace kthost {

struct Batch;        // seqio.hpp
struct UnitigGraph;  // computers.cpp: the unitigs, links and components as the device calls returned them

// Rust `format!("{:.6}", x)` (oligo.rs:132-134) and `Display` for f64 (shortest round-trip,
// positional notation, integral values without ".0": oligo.rs:136, oligocgr.rs:95)
constexpr size_t FIXED6_BUF = 352;  // "%.6f" of DBL_MAX is 316 characters
size_t format_fixed6(char *buf, double x);  // buf holds FIXED6_BUF bytes; returns the length written
void append_fixed6(std::string &out, double x);
void append_display(std::string &out, double x);

double debug_emit_bench(uint64_t n_rows, uint64_t bins, bool norm, int threads, int reps);

struct Device {  // one kt_ctx per computer, created on first use
    int index = 0;
    kt_ctx *ctx = nullptr;
    ~Device();
    std::string ensure();  // "" or error message
};

struct Cursor {  // a place in an input: the reads and the bases in front of it
    uint64_t reads = 0, bases = 0;
};

// What a read-level command (cov, filter, profile, correct) keeps of its input across the passes of an out-of-core table:
// arrays indexed by read or by base.  The first walk over the input grows them and notes its reads and bases; every
// later walk - the other passes, the output loop - must stay inside them and end at the same totals.
struct KeptAcrossPasses {
    const char *cmd;  // in front of the error texts
    Cursor seen;      // the input as the first walk saw it
    explicit KeptAcrossPasses(const char *c) : cmd(c) {}
    std::string changed() const { return std::string(cmd) + ": the input changed between the passes"; }
    template <class T>
    std::string claim(bool first, std::vector<T> &v, uint64_t size, T init) const {  // v holds `size` values from here on
        if (first) v.resize(size, init);
        else if (size > v.size()) return changed();
        return "";
    }
    std::string inside(const Cursor &at, const Batch &b) const;  // the batch at `at` lies inside what the first walk saw
    std::string finish(bool first, const Cursor &end);           // after a walk: note the totals, or compare them
    // profile and correct keep bytes_per_base of `what` per base of the whole input: refused above the memory ceiling (-m)
    std::string over_ceiling(uint64_t bases, unsigned bytes_per_base, const char *what, uint32_t passes, double ceil_gb) const;
};

class OligoComputer {
  public:
    OligoComputer(std::string in_path, std::string out_path, int ksize, bool count_min);
    void set_threads(int t) { threads_ = t; }
    void set_norm(bool n) { norm_ = n; }
    void set_delim(std::string d) { delim_ = std::move(d); }
    void set_max_memory(uint64_t m) { memory_ = m; }
    void set_header(bool h) { header_ = h; }
    void set_device(int d) { dev_.index = d; }
    std::vector<std::string> get_header() const;  // oligo.rs:69-83
    std::string vectorise();                      // oligo.rs:88-93 (batch and mmap paths write identical bytes)

  private:
    std::string in_path_, out_path_, delim_ = " ";
    int ksize_, threads_ = 0;
    bool count_min_, norm_ = true, header_ = false;
    uint64_t memory_ = 4ull << 30;  // GB_4, oligo.rs:13
    Device dev_;
};

class OligoCgrComputer {
  public:
    OligoCgrComputer(std::string in_path, std::string out_path, int ksize, uint64_t vecsize);
    void set_threads(int t) { threads_ = t; }
    void set_norm(bool n) { norm_ = n; }
    void set_device(int d) { dev_.index = d; }
    std::string vectorise();  // oligocgr.rs:63-121

  private:
    std::string in_path_, out_path_;
    int ksize_, threads_ = 0;
    uint64_t vecsize_;
    bool norm_ = true;
    uint64_t memory_ = 4ull << 30;
    Device dev_;
};

class CgrComputer {
  public:
    CgrComputer(std::string in_path, std::string out_path, uint64_t vecsize);
    void set_threads(int t) { threads_ = t; }
    void set_device(int d) { dev_.index = d; }
    // cgr.rs:67-125.  "" on success; "Bad nucleotide, unable to proceed" where the reference's
    // worker unwraps that Err (:95) and the process dies
    std::string vectorise();

  private:
    std::string in_path_, out_path_;
    uint64_t vecsize_;
    int threads_ = 0;
    Device dev_;
};

class CountComputer {
  public:
    CountComputer(std::string in_path, std::string out_dir, int ksize);
    ~CountComputer();
    void set_threads(int t) { threads_ = t; }
    void set_max_memory(double gb) { memory_ceil_gb_ = gb; }  // the host ceiling: the table is written out in slabs sized by it
    void set_acgt_output(bool a) { acgt_ = a; }
    void set_device(int d) { dev_.index = d; }
    void set_devices(int n) { n_devices_ = n < 1 ? 1 : n; }  // --devices N: the table sharded over N GPUs (kt_sharded_*)
    // --min-count / --max-count: only the entries with lo <= count <= hi go to kmers.counts (filtered on the device)
    void set_count_range(uint32_t lo, uint32_t hi) { min_count_ = lo, max_count_ = hi; }
    // --histo-max H (--histo): merge() also writes {out_dir}/kmers.histo, the spectrum of the whole table in H lines (the
    // last: H or more occurrences); only = --histo-only: no kmers.counts at all
    void set_histo(uint32_t h, bool only) { histo_max_ = h, histo_only_ = only; }
    // --save-table: the entries in the count range also go to this table file (kt_ctr_save), one section per pass
    void set_save_table(const std::string &path) { save_table_ = path; }
    // --table: the input path is a table file; count() loads it (one pass, one device) instead of counting reads
    void set_input_is_table(bool on) { input_is_table_ = on; }
    // counter/src/lib.rs:69-90.  No temp files: one resident table - or, when the distinct k-mers cannot fit the HBM,
    // `passes()` passes over the input, one hash partition each, written to kmers.counts as they complete.
    std::string count();
    std::string merge(bool del);     // counter/src/lib.rs:172-234: writes {out_dir}/kmers.counts
    uint64_t seq_count() const { return seq_count_; }  // 0 when the sizing pre-pass was skipped (plain files)
    uint32_t passes() const { return passes_; }
    // out of core (passes() > 1): called with every pass's complete table before it is written out and cleared
    void set_pass_hook(std::function<std::string(uint32_t pass, uint32_t passes, kt_ctr *table)> h) { pass_hook_ = std::move(h); }
    kt_ctr *table() const { return passes_ == 1 && !sharded_done_ ? ctr_ : nullptr; }  // the resident table (after count())
    kt_ctx *context() const { return dev_.ctx; }
    // --devices N, for a caller that looks k-mers up afterwards (cov): merge() writes the shards but leaves them on their GPUs
    void set_keep_shards(bool k) { keep_shards_ = k; }
    size_t n_shards() const { return sharded_done_ ? shards_.size() : 0; }
    kt_ctr *shard_table(size_t r) const;  // shard r's table (an ordinary kt_ctr that answers for its own k-mers only)

  private:
    std::string in_path_, out_dir_;
    int ksize_, threads_ = 0;
    double memory_ceil_gb_ = 6.0;
    bool acgt_ = false;
    uint64_t seq_count_ = 0, total_length_ = 0;
    Device dev_;
    kt_ctr *ctr_ = nullptr;
    int n_devices_ = 1;
    uint32_t passes_ = 1;
    bool sharded_done_ = false, keep_shards_ = false;
    uint32_t min_count_ = 1, max_count_ = 0xFFFFFFFFu, histo_max_ = 0;  // histo_max_ = 0: no kmers.histo
    bool histo_only_ = false;
    std::vector<uint64_t> histo_;  // the spectrum, summed over passes / shards (histo_max_ + 1 bins)
    std::string add_spectrum(kt_ctr *t);
    std::string save_table_;
    bool input_is_table_ = false;
    std::string save_table(kt_ctr *t, const std::string &path, bool append);
    std::string write_histo() const;
    // --devices N: the shards stay on their GPUs after count(); merge() writes them out one after the other, in slabs
    std::vector<kt_sharded *> shards_;
    std::vector<kt_ctx *> shard_ctx_;
    void release_shards();
    std::function<std::string(uint32_t, uint32_t, kt_ctr *)> pass_hook_;
    std::string count_sharded(uint64_t max_distinct);
};

// `min -p s2m`: one line per record, "id\tMMER:start-end\t...\t\n" (misc/src/minimisers.rs:93-160).
// `min -p m2s`: one line per minimiser, "MMER\t[(\"id\", start, end), ...]\n" - Rust's {:?} of the
// Vec<(String, usize, usize)> (:11-91).  The reference's line order (and, for m2s, the order inside a
// vector) depends on thread timing; here lines follow the input (s2m) or ascending minimiser text (m2s).
// wsize 0 = one minimiser per sequence.  Return "" or the error message.
std::string seq_to_min(uint64_t wsize, int msize, const std::string &in_path, const std::string &out_path, int threads,
                       int device = 0);
std::string bin_sequences(uint64_t wsize, int msize, const std::string &in_path, const std::string &out_path, int threads,
                          int device = 0);

class CovComputer {
  public:
    CovComputer(std::string in_path, std::string out_dir, int ksize, uint64_t bin_size, uint64_t bin_count);
    void set_threads(int t) { threads_ = t; }
    void set_norm(bool n) { norm_ = n; }
    void set_delim(std::string d) { delim_ = std::move(d); }
    void set_kmer_path(std::string p) { in_path_kmer_ = std::move(p); }
    // --table: the k-mer table is loaded from this table file (kt_ctr_add_file) instead of counted
    void set_kmer_table(std::string p) { in_path_kmer_ = std::move(p), kmer_is_table_ = true; }
    void set_max_memory(double gb) { memory_ceil_gb_ = gb; }
    void set_device(int d) { device_ = d; }
    void set_devices(int n) { n_devices_ = n < 1 ? 1 : n; }  // --devices N: the table sharded over N GPUs, every read looked up in every shard
    std::string build_table();        // coverage/src/lib.rs:69-77: count + merge -> {out_dir}/kmers.counts
    std::string compute_coverages();  // coverage/src/lib.rs:79-163: writes {out_dir}/kmers.vectors

  private:
    std::string in_path_, in_path_kmer_, out_dir_, delim_ = " ";
    bool kmer_is_table_ = false;
    int ksize_, threads_ = 0, device_ = 0, n_devices_ = 1;
    uint64_t bin_size_, bin_count_;
    bool norm_ = true;
    double memory_ceil_gb_ = 6.0;
    CountComputer *ctr_ = nullptr;  // owns the HBM table the coverages are looked up in
    // a table that needed several passes (the k-mers do not fit the HBM): the reads' raw bin counts, summed over the
    // passes as each pass's table is complete (kt_cov_batch_part), normalised and written at the end
    std::vector<uint32_t> acc_rows_;
    KeptAcrossPasses kept_{"cov"};
    std::string cov_pass(uint32_t pass, uint32_t passes, kt_ctr *table);

  public:
    ~CovComputer();
    CovComputer(const CovComputer &) = delete;
    CovComputer &operator=(const CovComputer &) = delete;
};

// `filter`: drops or trims reads by the abundance of their k-mers (kmc_tools filter, BBDuk-style k-mer cleaning).  The
// table is counted from kmer_path (default: the input) as by CountComputer - resident, or out of core in passes whose
// per-read numbers are combined here -, then every read's k-mers are looked up (kt_ctr_read_solidity).  A k-mer is solid
// when min_count <= count <= max_count.  Fraction mode keeps a read with >= 1 k-mer and solid >= F * k-mers; trim mode
// keeps the prefix up to the last base before the end of the first weak k-mer ([0, first_weak + k - 1)), the whole read
// without one, and drops what is left shorter than k.  Records are written in the input's format and order, bytes as
// read (FASTA: header line + the sequence on one line; FASTQ: header, sequence, "+", the quality cut as the sequence).
class FilterComputer {
  public:
    FilterComputer(std::string in_path, std::string out_path, int ksize);
    ~FilterComputer();
    FilterComputer(const FilterComputer &) = delete;
    FilterComputer &operator=(const FilterComputer &) = delete;
    void set_kmer_path(std::string p) { in_path_kmer_ = std::move(p); }
    // --table: the k-mer table is loaded from this table file (kt_ctr_add_file) instead of counted
    void set_kmer_table(std::string p) { in_path_kmer_ = std::move(p), kmer_is_table_ = true; }
    void set_count_range(uint32_t lo, uint32_t hi) { min_count_ = lo, max_count_ = hi; }
    void set_min_solid(double f) { min_solid_ = f; }
    void set_trim(bool t) { trim_ = t; }
    void set_threads(int t) { threads_ = t; }
    void set_max_memory(double gb) { memory_ceil_gb_ = gb; }
    void set_device(int d) { device_ = d; }
    std::string filter();  // "" or the error message

  private:
    std::string in_path_, in_path_kmer_, out_path_;
    bool kmer_is_table_ = false;
    int ksize_, threads_ = 0, device_ = 0;
    uint32_t min_count_ = 2, max_count_ = 0xFFFFFFFFu;
    double min_solid_ = 1.0, memory_ceil_gb_ = 6.0;
    bool trim_ = false;
    CountComputer *ctr_ = nullptr;
    // out of core: the reads' numbers, combined over the passes as each pass's table is complete (filter_pass)
    std::vector<uint32_t> acc_n_, acc_s_, acc_w_;
    KeptAcrossPasses kept_{"filter"};
    std::string filter_pass(uint32_t pass, uint32_t passes, kt_ctr *table);
    // appends the kept records of batch b (its numbers: n, s, w) to `out`
    void emit(const Batch &b, const uint32_t *n, const uint32_t *s, const uint32_t *w, bool fastq, std::string &out) const;
};

// `correct`: repairs substitution errors of reads from the solid k-mers of a counted table (k-mer spectrum correction; what
// Musket, Lighter and BFC do on the CPU) instead of cutting the read as `filter --trim` does.  The table is counted from
// kmer_path (default: the input) as by CountComputer; per batch the positions' counts (kt_ctr_profile) say which bases lie in
// a solid k-mer, the others get their candidates' support (kt_ctr_correct_support) and the decision (kt_correct_apply).
// EVERY record is written, in the input's format and order (FASTA: header line + the sequence on one line; FASTQ: header,
// sequence, "+", quality unchanged).  Out of core the pass loop runs twice - the support needs the COMPLETE profile -: the
// first count fills the per-base counts of the whole input on the host, the second the per-base supports (8 bytes per base
// together; refused when more than the memory ceiling), and the decision runs batch by batch at the end.
class CorrectComputer {
  public:
    CorrectComputer(std::string in_path, std::string out_path, int ksize);
    ~CorrectComputer();
    CorrectComputer(const CorrectComputer &) = delete;
    CorrectComputer &operator=(const CorrectComputer &) = delete;
    void set_kmer_path(std::string p) { in_path_kmer_ = std::move(p); }
    // --table: the k-mer table is loaded from this table file (kt_ctr_add_file) instead of counted
    void set_kmer_table(std::string p) { in_path_kmer_ = std::move(p), kmer_is_table_ = true; }
    void set_count_range(uint32_t lo, uint32_t hi) { min_count_ = lo, max_count_ = hi; }
    void set_min_support(uint32_t s) { min_support_ = s; }
    void set_max_corrections(uint32_t n) { max_corrections_ = n; }  // 0: no limit
    void set_stats_path(std::string p) { stats_path_ = std::move(p); }
    void set_threads(int t) { threads_ = t; }
    void set_max_memory(double gb) { memory_ceil_gb_ = gb; }
    void set_device(int d) { device_ = d; }
    std::string correct();  // "" or the error message

  private:
    std::string in_path_, in_path_kmer_, out_path_, stats_path_;
    bool kmer_is_table_ = false;
    int ksize_, threads_ = 0, device_ = 0;
    uint32_t min_count_ = 2, max_count_ = 0xFFFFFFFFu, min_support_ = 1, max_corrections_ = 0;
    double memory_ceil_gb_ = 6.0;
    CountComputer *ctr_ = nullptr;
    // out of core: the whole input's per-base counts (first pass loop) and supports (second), filled as each pass's table is complete
    std::vector<uint32_t> acc_prof_, acc_sup_;
    KeptAcrossPasses kept_{"correct"};
    std::string table_pass(bool support, uint32_t pass, uint32_t passes, kt_ctr *table);
    CountComputer *new_counter(bool support);
};

// `profile`: how often every position of the input's sequences occurs in a counted sample (KAT sect, jellyfish query -s)
// and each sequence's k-mers, present k-mers, min / median / mean / max count (the median: element n / 2 of the sorted
// counts, khmer's get_median_count).  The table is counted from kmer_path (default: the input) as by CountComputer; every
// batch's positions are then looked up (kt_ctr_profile) and reduced per record (kt_profile_stats).  Out of core the
// per-base array of the WHOLE input (4 bytes per base) is kept on the host and filled pass by pass - a median cannot be
// combined over hash partitions, the array can -, and the statistics are taken after the last pass; an array larger than
// the memory ceiling (-m) is refused.  Writes {out_dir}/profile.stats (a header line, then per record
// name, length, kmers, present, min, median, mean, max, tab-separated) and with positions {out_dir}/profile.counts
// (per record ">name" and one line of `length` space-separated counts, -1 where no k-mer starts).
class ProfileComputer {
  public:
    ProfileComputer(std::string in_path, std::string out_dir, int ksize);
    ~ProfileComputer();
    ProfileComputer(const ProfileComputer &) = delete;
    ProfileComputer &operator=(const ProfileComputer &) = delete;
    void set_kmer_path(std::string p) { in_path_kmer_ = std::move(p); }
    // --table: the k-mer table is loaded from this table file (kt_ctr_add_file) instead of counted
    void set_kmer_table(std::string p) { in_path_kmer_ = std::move(p), kmer_is_table_ = true; }
    void set_positions(bool p) { positions_ = p; }
    void set_threads(int t) { threads_ = t; }
    void set_max_memory(double gb) { memory_ceil_gb_ = gb; }
    void set_device(int d) { device_ = d; }
    std::string profile();  // "" or the error message

  private:
    std::string in_path_, in_path_kmer_, out_dir_;
    bool kmer_is_table_ = false;
    int ksize_, threads_ = 0, device_ = 0;
    double memory_ceil_gb_ = 6.0;
    bool positions_ = false;
    CountComputer *ctr_ = nullptr;
    // out of core: the whole input's per-base counts, filled over the passes as each pass's table is complete
    std::vector<uint32_t> acc_;
    KeptAcrossPasses kept_{"profile"};
    std::string profile_pass(uint32_t pass, uint32_t passes, kt_ctr *table);
};

// `compare`: the comparison matrix of two inputs' k-mer tables (KAT comp / spectra-cn) and the similarity of their k-mer
// sets (Jaccard, containment, weighted Jaccard).  Both tables live on one Device, sized from their inputs as CountComputer
// sizes its table; when the two cannot share the HBM (or KT_CTR_MAX_SLOTS bounds a table) the inputs are counted in
// `passes()` passes, pass p holding hash partition p of both (kt_ctr_add_reads_part), and every pass's kt_ctr_compare is
// added into one matrix.  Writes {out_dir}/compare.matrix ((max_a + 1) lines of max_b + 1 tab-separated counts; the last
// row and column: that count or more) and {out_dir}/compare.stats ("name\tvalue" lines).
class CompareComputer {
  public:
    CompareComputer(std::string in_a, std::string in_b, std::string out_dir, int ksize);
    ~CompareComputer();
    CompareComputer(const CompareComputer &) = delete;
    CompareComputer &operator=(const CompareComputer &) = delete;
    void set_max_counts(uint32_t max_a, uint32_t max_b) { max_a_ = max_a, max_b_ = max_b; }
    void set_threads(int t) { threads_ = t; }
    void set_max_memory(double gb) { memory_ceil_gb_ = gb; }  // (accepted; the tables live in HBM)
    void set_device(int d) { dev_.index = d; }
    // --table / --alt-table: that side's table is loaded from a table file; the path takes the input's place
    void set_tables(bool a_is_table, bool b_is_table) { a_is_table_ = a_is_table, b_is_table_ = b_is_table; }
    std::string compare();  // "" or the error message
    uint32_t passes() const { return passes_; }

  private:
    std::string in_a_, in_b_, out_dir_;
    bool a_is_table_ = false, b_is_table_ = false;
    int ksize_, threads_ = 0;
    uint32_t max_a_ = 1000, max_b_ = 100, passes_ = 1;
    double memory_ceil_gb_ = 6.0;
    Device dev_;
    kt_ctr *ta_ = nullptr, *tb_ = nullptr;
    void release();
    std::string write(const std::vector<uint64_t> &m, const uint64_t *tot) const;
};

// `setop`: WHICH k-mers `compare` counted - the intersection, difference, union or symmetric difference of two inputs'
// k-mer tables (kmc_tools simple, meryl, kat filter kmer), counted and passed over as CompareComputer does; every pass runs
// kt_ctr_setop (sorted) on its two tables and appends its lines.  Writes {out_dir}/kmers.counts in `ctr`'s line format -
// ascending numeric key within a pass, the passes one after the other - and {out_dir}/setop.stats ("name\tvalue" lines:
// distinct_a, distinct_b, in_a, in_b, emitted, emitted_occurrences).  The host holds one pass's result as pairs (12 bytes
// an entry); its text is made a slab at a time.
class SetopComputer {
  public:
    SetopComputer(std::string in_a, std::string in_b, std::string out_dir, int ksize);
    ~SetopComputer();
    SetopComputer(const SetopComputer &) = delete;
    SetopComputer &operator=(const SetopComputer &) = delete;
    void set_op(int op, int rule) { op_ = op, rule_ = rule; }  // KT_SET_*, KT_SETCNT_*
    void set_ranges(uint32_t min_a, uint32_t max_a, uint32_t min_b, uint32_t max_b) {
        min_a_ = min_a, max_a_ = max_a, min_b_ = min_b, max_b_ = max_b;
    }
    void set_acgt_output(bool a) { acgt_ = a; }
    void set_threads(int t) { threads_ = t; }
    void set_max_memory(double gb) { memory_ceil_gb_ = gb; }  // the text slabs shrink with it; the tables live in HBM
    void set_device(int d) { dev_.index = d; }
    // --table / --alt-table: that side's table is loaded from a table file; the path takes the input's place
    void set_tables(bool a_is_table, bool b_is_table) { a_is_table_ = a_is_table, b_is_table_ = b_is_table; }
    std::string setop();  // "" or the error message

  private:
    std::string in_a_, in_b_, out_dir_;
    bool a_is_table_ = false, b_is_table_ = false;
    int ksize_, threads_ = 0, op_ = 0, rule_ = 0;
    uint32_t min_a_ = 1, max_a_ = 0xFFFFFFFFu, min_b_ = 1, max_b_ = 0xFFFFFFFFu, passes_ = 1;
    bool acgt_ = false;
    double memory_ceil_gb_ = 6.0;
    Device dev_;
    kt_ctr *ta_ = nullptr, *tb_ = nullptr;
    void release();
};

// `graph`: which k-mers of an input follow which - the de Bruijn adjacency of its counted k-mers, the unitig ends and the
// node census (kt_ctr_graph, sorted).  One table, and the whole of it on the device: a node's neighbours live in other hash
// partitions, so a count that would take several passes is refused before anything is written.  Writes
// {out_dir}/graph.nodes ("kmer\tcount\tleft4\tright4\tends2" per node, ascending numeric key; not with stats_only) and
// {out_dir}/graph.stats (the KT_GRAPH_CENSUS values as "name\tvalue" lines).
class GraphComputer {
  public:
    GraphComputer(std::string in_path, std::string out_dir, int ksize);
    ~GraphComputer();
    GraphComputer(const GraphComputer &) = delete;
    GraphComputer &operator=(const GraphComputer &) = delete;
    void set_range(uint32_t min_count, uint32_t max_count) { min_count_ = min_count, max_count_ = max_count; }
    void set_acgt_output(bool a) { acgt_ = a; }
    void set_stats_only(bool s) { stats_only_ = s; }
    // --table: the table is loaded from this table file (kt_ctr_add_file) instead of counted from the input
    void set_table_file(std::string p) { table_file_ = std::move(p); }
    void set_threads(int t) { threads_ = t; }
    void set_max_memory(double gb) { memory_ceil_gb_ = gb; }  // the text slabs shrink with it; the table lives in HBM
    void set_device(int d) { dev_.index = d; }
    std::string graph();  // "" or the error message

  private:
    std::string in_path_, out_dir_;
    std::string table_file_;
    int ksize_, threads_ = 0;
    uint32_t min_count_ = 1, max_count_ = 0xFFFFFFFFu;
    bool acgt_ = false, stats_only_ = false;
    double memory_ceil_gb_ = 6.0;
    Device dev_;
    kt_ctr *table_ = nullptr;
};

// `hetmers`: the heterozygous k-mer pairs of an input's counted k-mers (kt_ctr_hetmers, sorted) and the matrix of their
// coverages, minor against major (Smudgeplot's hetkmers and its plot): one table, the whole of it on the device, as for
// `graph`.  Writes {out_dir}/hetmers.pairs ("A\tB\tpos\tcount_a\tcount_b" per pair, ascending numeric A, B on the strand on
// which it differs from A at position pos) and {out_dir}/hetmers.cov ("minor\tmajor" per pair, the same order) - neither
// with stats_only, which moves no pairs to the host -, {out_dir}/hetmers.matrix ((max_minor + 1) lines of max_major + 1
// tab-separated counts, compare.matrix's layout) and {out_dir}/hetmers.stats ("name\tvalue" lines: k, the count range, the
// positions, the KT_HET_CENSUS values).
class HetmerComputer {
  public:
    HetmerComputer(std::string in_path, std::string out_dir, int ksize);
    ~HetmerComputer();
    HetmerComputer(const HetmerComputer &) = delete;
    HetmerComputer &operator=(const HetmerComputer &) = delete;
    void set_range(uint32_t min_count, uint32_t max_count) { min_count_ = min_count, max_count_ = max_count; }
    void set_middle(bool m) { middle_ = m; }
    void set_max_counts(uint32_t max_minor, uint32_t max_major) { max_minor_ = max_minor, max_major_ = max_major; }
    void set_stats_only(bool s) { stats_only_ = s; }
    // --table: the table is loaded from this table file (kt_ctr_add_file) instead of counted from the input
    void set_table_file(std::string p) { table_file_ = std::move(p); }
    void set_threads(int t) { threads_ = t; }
    void set_max_memory(double gb) { memory_ceil_gb_ = gb; }  // (accepted; the table lives in HBM)
    void set_device(int d) { dev_.index = d; }
    std::string hetmers();  // "" or the error message

  private:
    std::string in_path_, out_dir_;
    std::string table_file_;
    int ksize_, threads_ = 0;
    uint32_t min_count_ = 1, max_count_ = 0xFFFFFFFFu, max_minor_ = 500, max_major_ = 1000;
    bool middle_ = false, stats_only_ = false;
    double memory_ceil_gb_ = 6.0;
    Device dev_;
    kt_ctr *table_ = nullptr;
};

// `unitigs`: the maximal unitigs of the de Bruijn graph of an input's counted k-mers (kt_ctr_unitigs): one table, the whole of
// it on the device, as for `graph`.  Writes {out_dir}/unitigs.fa (">{i} LN:i:{bases} KC:i:{count sum} km:f:{count sum / nodes}"
// and " CL:i:1" on a cycle, then the sequence on one line; not with stats_only) and {out_dir}/unitigs.stats ("name\tvalue":
// unitigs, bases, nodes, occurrences, circular, singletons, longest, n50).  With set_links (kt_ctr_unitigs_linked instead):
// gfa writes {out_dir}/unitigs.gfa ("H\tVN:Z:1.0", "S\t{i}\t{seq}\tLN:i:\tKC:i:\tkm:f:" and "\tCL:i:1" on a cycle,
// "L\t{u}\t{su}\t{v}\t{sv}\t{k-1}M" for every link that is not larger than its mirror as (u, su is '-', v, sv is '-')), fa_links
// appends " L:{su}:{v}:{sv}" per directed link to the header lines of unitigs.fa; either one writes
// {out_dir}/unitigs.links.stats (links, edges, dead_ends, isolated, self_links, max_end_degree).  With set_clip the counted
// table is clipped first (kt_ctr_clip_tips), every file describes the clipped graph, and {out_dir}/unitigs.clip.stats holds
// rounds, tips, tip_nodes, isolated, isolated_nodes, occurrences, converged.  With set_bubbles the table is simplified by
// kt_ctr_simplify instead - bubbles popped, and tips clipped in the same rounds when set_clip is given too - and
// {out_dir}/unitigs.simplify.stats holds rounds, tips, tip_nodes, isolated, isolated_nodes, popped, popped_nodes, bubbles,
// occurrences, converged (and no unitigs.clip.stats is written).
class UnitigComputer {
  public:
    UnitigComputer(std::string in_path, std::string out_dir, int ksize);
    ~UnitigComputer();
    UnitigComputer(const UnitigComputer &) = delete;
    UnitigComputer &operator=(const UnitigComputer &) = delete;
    void set_range(uint32_t min_count, uint32_t max_count) { min_count_ = min_count, max_count_ = max_count; }
    void set_stats_only(bool s) { stats_only_ = s; }
    // --table: the table is loaded from this table file (kt_ctr_add_file) instead of counted from the input
    void set_table_file(std::string p) { table_file_ = std::move(p); }
    void set_links(bool gfa, bool fa_links) { gfa_ = gfa, fa_links_ = fa_links; }
    // before anything is written, the tips of at most tip_nodes k-mers (drop_isolated: the isolated unitigs that short, too)
    // are erased from the table, for at most `rounds` rounds
    void set_clip(uint32_t tip_nodes, uint32_t rounds, bool drop_isolated) {
        clip_ = true, tip_nodes_ = tip_nodes, clip_rounds_ = rounds, drop_isolated_ = drop_isolated;
    }
    // before anything is written, of the branches of at most bubble_nodes k-mers between the same two ends all but the best
    // are erased, for at most `rounds` rounds - the rounds of set_clip, where both are given
    void set_bubbles(uint32_t bubble_nodes, uint32_t rounds) { pop_ = true, bubble_nodes_ = bubble_nodes, clip_rounds_ = rounds; }
    // the connected components of the unitig graph (kt_unitig_components over the linked run's arrays, after set_clip /
    // set_bubbles did their work): {out_dir}/unitigs.components (per component: component, unitigs, nodes, bases, count_sum, km,
    // links, first_unitig) and unitigs.components.stats (components, singletons, largest_unitigs, largest_nodes, largest_share),
    // unitigs.links.stats as with gfa, and - not with stats_only - " CC:i:{c}" behind every header line of unitigs.fa and
    // "\tCC:i:{c}" behind every S line of unitigs.gfa.  With set_thread: unitigs.fa, unitigs.gfa and unitigs.components as
    // above, thread.reads (per record: name, component or *, mixed, hits; not with stats_only), thread.components (per
    // component: component, unitigs, nodes, reads, hits) and three more lines of thread.stats (kt_thread_read_components)
    void set_components(bool c) { components_ = c; }
    void set_device(int d) { dev_.index = d; }
    // `thread`: the unitigs are written as `unitigs --gfa` writes unitigs.fa and unitigs.gfa (stats_only: not at all) and no
    // other unitigs.* file; then the records of reads_path are threaded onto them (kt_ctr_index_sequences over the unitigs,
    // kt_ctr_thread_hits and kt_thread_runs per batch): {out_dir}/thread.gaf (one line per chain of runs; not with
    // stats_only), thread.unitigs (per unitig: id, bases, nodes, count sum, hits, runs, hits / nodes) and thread.stats
    void set_thread(std::string reads_path, bool stats_only) {
        thread_ = true, thread_reads_ = std::move(reads_path), gfa_ = !stats_only, fa_links_ = false, stats_only_ = stats_only;
    }
    std::string unitigs();  // "" or the error message

  private:
    std::string simplify_table();                            // set_clip / set_bubbles, and the stats file of it
    std::string fetch_unitigs(bool linked, UnitigGraph &g);  // what the device calls return
    std::string thread_onto(const UnitigGraph &g);
    bool thread_ = false;
    std::string thread_reads_;
    std::string in_path_, out_dir_;
    std::string table_file_;
    int ksize_;
    uint32_t min_count_ = 1, max_count_ = 0xFFFFFFFFu;
    bool stats_only_ = false, gfa_ = false, fa_links_ = false;
    bool clip_ = false, drop_isolated_ = false, pop_ = false, components_ = false;
    uint32_t tip_nodes_ = 0, clip_rounds_ = 8, bubble_nodes_ = 0;
    Device dev_;
    kt_ctr *table_ = nullptr;
};

// `sketch`: bottom-s MinHash sketches of the records of an input (kt_sketch_batch), of the whole input (--single: the
// batches' sketches merged by kt_sketch_merge) and the Mash distances between them (kt_sketch_pairs, a block of rows of the
// matrix at a time; the formula is kt_mash_distance).  Writes {out_dir}/sketch.tsv ("id\tlength\tkmers\tsize\th0,h1,..."
// per sketch, in input order), {out_dir}/sketch.alt.tsv for the second input and {out_dir}/sketch.dist
// ("id_a\tid_b\tshared/denom\tjaccard\tdistance": the pairs i < j of the input, or every pair (input, alt input)).
// With --scaled the sketches are scaled ones (kt_scaled_batch; --single: the running sketch and a batch's rows are one group
// of kt_scaled_merge; --table: kt_ctr_scaled of a loaded table file stands in for the input): the same files, `size` the
// row's length, with --abund a sixth column of abundances; --contain writes {out_dir}/sketch.contain
// ("id_a\tid_b\tshared\tsize_a\tsize_b\tjaccard\ta_in_b\tb_in_a\tani", kt_scaled_pairs a block of rows at a time).
class SketchComputer {
  public:
    SketchComputer(std::string in_path, std::string out_dir, int ksize, uint32_t sketch_size);
    void set_seed(uint64_t seed) { seed_ = seed; }
    void set_scaled(uint64_t scaled, bool abund) { scaled_ = scaled, abund_ = abund; }
    void set_table(std::string path, uint32_t min_count, uint32_t max_count) { table_path_ = std::move(path), min_count_ = min_count, max_count_ = max_count; }
    void set_contain(bool c, double min_contain) { contain_ = c, min_contain_ = min_contain; }
    void set_single(bool s) { single_ = s; }
    void set_alt_path(std::string p) { alt_path_ = std::move(p); }
    void set_dist(bool d, double max_dist) { dist_ = d, max_dist_ = max_dist; }
    void set_threads(int t) { threads_ = t; }
    void set_device(int d) { dev_.index = d; }
    std::string sketch();  // "" or the error message

  private:
    struct Set {  // the sketches of one input, kept for the distances
        std::vector<std::string> ids;
        std::vector<uint64_t> hashes;  // rows of s
        std::vector<uint32_t> sizes;
    };
    std::string in_path_, alt_path_, out_dir_;
    int ksize_, threads_ = 0;
    uint32_t s_;
    uint64_t seed_ = 0;
    bool single_ = false, dist_ = false;
    double max_dist_ = 1.0;
    Device dev_;
    std::string sketch_input(const std::string &path, const std::string &out_path, Set &set, bool keep);
    std::string write_dist(const Set &a, const Set *b);
    // --scaled
    struct ScaledSet {  // the scaled sketches of one input, CSR, kept for sketch.contain
        std::vector<std::string> ids;
        std::vector<uint64_t> hashes, offsets{0};
    };
    std::string table_path_;
    uint64_t scaled_ = 0;
    uint32_t min_count_ = 1, max_count_ = 0xFFFFFFFFu;
    bool abund_ = false, contain_ = false;
    double min_contain_ = 0.0;
    std::string scaled_input(const std::string &path, const std::string &out_path, ScaledSet &set, bool keep);
    std::string scaled_table(const std::string &out_path, ScaledSet &set, bool keep);
    std::string write_contain(const ScaledSet &a, const ScaledSet *b);
};

// `card`: the HyperLogLog registers of the distinct canonical k-mers of an input (kt_card_add_reads over the input walk) and
// their estimate (kt_card_estimate).  Writes {out_dir}/card.stats ("name\tvalue": sequences, bases, kmers, precision,
// registers, zero_registers, distinct_estimate, rel_std_error, slots_wanted; with a second input the same rows with an
// alt_ prefix, then union_estimate, intersection_estimate and jaccard_estimate from the merged registers) and
// {out_dir}/card.registers ("p\tseed\tk", then one register per line; card.alt.registers for the second input).
class CardComputer {
  public:
    CardComputer(std::string in_path, std::string out_dir, int ksize, int precision);
    void set_seed(uint64_t seed) { seed_ = seed; }
    void set_alt_path(std::string p) { alt_path_ = std::move(p); }
    void set_threads(int t) { threads_ = t; }
    void set_device(int d) { dev_.index = d; }
    std::string card();  // "" or the error message

  private:
    std::string in_path_, alt_path_, out_dir_;
    int ksize_, p_, threads_ = 0;
    uint64_t seed_ = 0;
    Device dev_;
};

// --estimate-size of the table commands: with it on, the table plan takes the distinct k-mers of the input it counts from
// one extra walk (kt_card_add_reads into 2^precision registers) instead of from the input's size alone.  The dispatcher
// sets it before it runs a command; when the command then fails with a full table (table_overflowed: the estimate was too
// small) it says so, switches it off and runs the command once more - with the plan of a run without the flag.
void set_estimate_size(bool on, int precision);
uint64_t estimate_size_taken();                  // the sum of the estimates the plans of this process have used
bool table_overflowed(const std::string &err);   // `err` is a command's error for a table that took more keys than slots

// --prefilter of ctr, graph, unitigs and hetmers: the input is walked twice - pass 1 into a bit filter on the device that
// remembers which k-mers were seen twice, pass 2 into a table planned from what pass 1 promoted and counting only those -
// so that the k-mers seen once take no slots.  The dispatcher sets it before it runs a command, with the filter's bits per
// k-mer expected and the directory prefilter.stats goes to.  The host side of the sizing follows (the hidden
// `debug-prefilter` runs it without a device).
void set_prefilter(bool on, uint64_t bits_per_kmer, const std::string &out_dir);
struct PrefilterStats {  // the lines of prefilter.stats, in their order
    uint64_t windows = 0, once_words = 0, twice_words = 0, once_bits_set = 0, twice_bits_set = 0, promotions = 0, table_slots = 0,
             table_keys = 0, table_retries = 0;
};
// log2 of the words of `once` and `twice` for that many k-mers, `once` capped to a quarter of free_bytes (0: no cap); "" or
// why the request is refused (0 bits, more than 2^34 words)
std::string prefilter_sizes(uint64_t expected_kmers, uint64_t bits_per_kmer, uint64_t free_bytes, int *log2_once, int *log2_twice);
// slots for the table of pass 2: 1.9 x scale x (promotions + (twice_bits_set / bits of twice)^4 x expected_kmers), at least 1024
uint64_t prefilter_table_slots(uint64_t promotions, uint64_t twice_bits_set, int log2_twice, uint64_t expected_kmers, double scale);
std::string prefilter_stats_text(const PrefilterStats &s);
std::string write_prefilter_stats(const PrefilterStats &s);  // {out_dir}/prefilter.stats

}  // namespace kthost
