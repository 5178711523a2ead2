#include "computers.hpp"

#include <malloc.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/stat.h>

#include <algorithm>
#include <atomic>
#include <charconv>
#include <chrono>
#include <condition_variable>
#include <deque>
#include <functional>
#include <mutex>
#include <optional>
#include <thread>

#include "outfile.hpp"
#include "seqio.hpp"

namespace kthost {

// ---- text formats ------------------------------------------------------------------------------
// Rust's `{:.6}` rounds the EXACT binary value half-to-even (core::num::flt2dec dragon
// format_exact), which is also what glibc's "%.6f" does; snprintf costs ~150 ns and serialises
// threads on locale state, so the common range is done by hand: N = round_half_even(x * 10^6)
// exactly, from the rounded product p and its exact error e (Dekker two-product; 10^6 has 20
// significant bits so only x needs splitting), then "<N / 10^6>.<6 digits>".
static const char DIGIT_PAIRS[] =
    "0001020304050607080910111213141516171819202122232425262728293031323334353637383940414243444546474849"
    "5051525354555657585960616263646566676869707172737475767778798081828384858687888990919293949596979899";

size_t format_fixed6(char *buf, double x) {
    if (!(x >= 0.0) || x >= 4.0e9) return (size_t)snprintf(buf, FIXED6_BUF, "%.6f", x);  // negative, NaN, inf, huge
    const double p = x * 1e6;
    const double c = 134217729.0 * x;  // 2^27 + 1
    const double xh = c - (c - x), xl = x - xh;
    const double e = (xh * 1e6 - p) + xl * 1e6;  // x * 10^6 == p + e exactly
    const double n = floor(p);
    const double d = (p - n) - 0.5;  // exact: p < 2^52, so p - n and 0.5 are multiples of ulp(p); |e| <= ulp(p)/2
    uint64_t N = (uint64_t)n;
    if (d > 0.0 || (d == 0.0 && (e > 0.0 || (e == 0.0 && (N & 1ull))))) N += 1;
    const uint64_t ip = N / 1000000ull;
    const uint32_t fp = (uint32_t)(N % 1000000ull);
    char *q = buf;
    if (ip < 10) {
        *q++ = (char)('0' + ip);
    } else {
        q = std::to_chars(q, q + 24, ip).ptr;
    }
    *q++ = '.';
    memcpy(q, DIGIT_PAIRS + 2 * (fp / 10000u), 2);
    memcpy(q + 2, DIGIT_PAIRS + 2 * ((fp / 100u) % 100u), 2);
    memcpy(q + 4, DIGIT_PAIRS + 2 * (fp % 100u), 2);
    return (size_t)(q + 6 - buf);
}

void append_fixed6(std::string &out, double x) {
    char buf[FIXED6_BUF];
    out.append(buf, format_fixed6(buf, x));
}

void append_display(std::string &out, double x) {
    char buf[400];
    if (x >= 0.0 && x < 9.0e15 && !signbit(x) && x == (double)(uint64_t)x) {  // counts: integral values print bare
        const auto r = std::to_chars(buf, buf + sizeof buf, (uint64_t)x);
        out.append(buf, (size_t)(r.ptr - buf));
        return;
    }
    const auto r = std::to_chars(buf, buf + sizeof buf, x, std::chars_format::fixed);  // shortest round-trip
    out.append(buf, (size_t)(r.ptr - buf));
}

Device::~Device() {
    if (ctx) kt_ctx_destroy(ctx);
}

std::string Device::ensure() {
    if (ctx) return "";
    if (kt_ctx_create(index, nullptr, 1, &ctx) != KT_OK) return std::string(kt_last_error());
    return "";
}

// KT_CLI_TIMING=1: busy seconds of each stage on stderr (the stages overlap, see run_pipeline)
struct PhaseTimer {
    const char *what;
    double t[4] = {0, 0, 0, 0};  // read, device, format, write - each owned by one thread
    bool on;
    explicit PhaseTimer(const char *w) : what(w), on(getenv("KT_CLI_TIMING") != nullptr) {}
    ~PhaseTimer() {
        if (on) fprintf(stderr, "[timing] %s: read %.3f s, device %.3f s, format %.3f s, write %.3f s\n", what, t[0], t[1], t[2], t[3]);
    }
};
struct Lap {
    std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
    double operator()() {
        const auto now = std::chrono::steady_clock::now();
        const double d = std::chrono::duration<double>(now - t0).count();
        t0 = now;
        return d;
    }
};

// CPUs this process may actually use: the hardware count capped by the cgroup CPU quota (a
// container with a 16-CPU quota on a 256-thread host is throttled, not sped up, by 256 workers)
static int effective_cpus() {
    static const int cached = [] {
        unsigned h = std::thread::hardware_concurrency();
        long n = h ? (long)h : 1;
        long quota = -1, period = -1;
        if (FILE *f = fopen("/sys/fs/cgroup/cpu.max", "r")) {  // cgroup v2: "<quota|max> <period>"
            char q[32];
            if (fscanf(f, "%31s %ld", q, &period) == 2 && strcmp(q, "max") != 0) quota = atol(q);
            fclose(f);
        } else if (FILE *g = fopen("/sys/fs/cgroup/cpu/cpu.cfs_quota_us", "r")) {  // cgroup v1
            if (fscanf(g, "%ld", &quota) != 1) quota = -1;
            fclose(g);
            if (FILE *pf = fopen("/sys/fs/cgroup/cpu/cpu.cfs_period_us", "r")) {
                if (fscanf(pf, "%ld", &period) != 1) period = -1;
                fclose(pf);
            }
        }
        if (quota > 0 && period > 0) {
            const long c = (quota + period - 1) / period;
            if (c < n) n = c;
        }
        return (int)(n < 1 ? 1 : n);
    }();
    return cached;
}

static int worker_count(int threads) {
    if (threads > 0) return threads;  // -t: the caller's explicit choice
    return effective_cpus();
}

// format rows [0, n) with `fn(row, out)` on `threads` workers, return the pieces in row order
template <class F>
static void format_rows(uint64_t n, int threads, size_t bytes_per_row, std::vector<std::string> &pieces, F fn) {
    int t = worker_count(threads);
    const uint64_t min_rows = 2048;  // a thread is not worth starting for less
    if ((uint64_t)t > (n + min_rows - 1) / min_rows) t = (int)((n + min_rows - 1) / min_rows);
    if (t < 1) t = 1;
    // (never fewer pieces than before: a short last batch must not free the text buffers the next full one needs)
    if (pieces.size() < (size_t)t) pieces.resize((size_t)t);
    for (size_t w = (size_t)t; w < pieces.size(); w++) pieces[w].clear();
    auto work = [&](int w) {
        const uint64_t lo = n * (uint64_t)w / (uint64_t)t, hi = n * (uint64_t)(w + 1) / (uint64_t)t;
        // build in a thread-local object: the string headers in `pieces` share cache lines, and every
        // append updates its header (measured: 8 threads slower than 1 when appending in place)
        std::string s;
        s.swap(pieces[(size_t)w]);  // keeps the capacity of the previous batch
        s.clear();
        s.reserve((hi - lo) * bytes_per_row);
        for (uint64_t r = lo; r < hi; r++) fn(r, s);
        s.swap(pieces[(size_t)w]);
    };
    // every share runs on a spawned thread: a share run on the calling thread was measured 6x slower than
    // its siblings on the GPU box (new threads start on the caller's CPU and crowd it until they migrate)
    std::vector<std::thread> pool;
    for (int w = 0; w < t; w++) pool.emplace_back(work, w);
    for (auto &th : pool) th.join();
}

// Rows [0, n) as text into one file, or side by side into several: `slab` rows at a time (the host holds one slab's text),
// each file's share of a slab formatted by fn(row, out) on the workers and written before the next file's; a failure ends it.
template <class F>
struct RowText {
    OutFile &out;
    size_t bytes_per_row;
    F fn;
    RowText(OutFile &o, size_t b, F f) : out(o), bytes_per_row(b), fn(f) {}
};
template <class... R>
static void write_rows(uint64_t n, uint64_t slab, int threads, std::vector<std::string> &pieces, R... files) {
    for (uint64_t i0 = 0; i0 < n && !(files.out.failed() || ...); i0 += slab) {
        auto one = [&](auto &f) {
            format_rows(std::min(slab, n - i0), threads, f.bytes_per_row, pieces, [&](uint64_t r, std::string &s) { f.fn(i0 + r, s); });
            f.out.write(pieces);
        };
        (one(files), ...);
    }
}

// ---- read -> device -> text pipeline ---------------------------------------------------------
// The three stages of every vectoriser (parse a batch of records; one C-ABI call that stages the
// batch to the GPU and brings the rows back; format + write the rows) run on their own threads
// over three rotating work items, so the file costs max(stage) instead of sum(stage).  Output
// order is the input order (one emit thread, FIFO hand-off).
struct Work {
    Batch b;
    std::vector<double> rows;
    std::vector<uint64_t> u64[4];  // minimisers: event offsets, m-mers, starts, ends
    uint64_t n_events = 0;

    // From its second batch on (i.e. for files of many batches, where the cost of locking is repaid) the row
    // buffer of a work item is page-locked, so the device-to-host copy of the rows - by far the largest
    // transfer - runs by DMA instead of through the driver's pageable staging.
    // (a resize that reallocates frees the registered buffer: release the page lock first, not afterwards)
    void resize_rows(size_t n) {
        if (n > rows.capacity()) unpin();
        rows.resize(n);
    }
    void pin_rows(kt_ctx *ctx) {
        if (++uses_ < 2) return;
        void *p = rows.data();
        const size_t bytes = rows.capacity() * sizeof(double);
        if (p == pin_ptr_ && bytes == pin_bytes_) return;
        unpin();
        if (bytes && kt_host_register(ctx, p, bytes) == KT_OK) {
            pin_ctx_ = ctx;
            pin_ptr_ = p;
            pin_bytes_ = bytes;
        }
    }
    void unpin() {
        if (pin_ptr_) kt_host_unregister(pin_ctx_, pin_ptr_);
        pin_ptr_ = nullptr;
        pin_bytes_ = 0;
    }
    // KT_CLI_PIN_BASES=1 (an experiment, off by default - DESIGN.md 6.1 has what it measured): the batch's bases buffer
    // page-locked as well, from the item's second batch on.  The parallel reader copies every batch into this buffer,
    // so its address is stable as long as no batch outgrows its capacity (reserved with slack at the first use).
    void pin_bases(kt_ctx *ctx) {
        static const bool on = getenv("KT_CLI_PIN_BASES") != nullptr;
        if (!on || uses_ < 2) return;
        void *p = b.bases.data();
        const size_t bytes = b.bases.capacity();
        if (p == bpin_ptr_ && bytes == bpin_bytes_) return;
        if (bpin_ptr_) kt_host_unregister(bpin_ctx_, bpin_ptr_);
        bpin_ptr_ = nullptr;
        if (bytes && kt_host_register(ctx, p, bytes) == KT_OK) {
            bpin_ctx_ = ctx;
            bpin_ptr_ = p;
            bpin_bytes_ = bytes;
        }
    }
    ~Work() {
        unpin();
        if (bpin_ptr_) kt_host_unregister(bpin_ctx_, bpin_ptr_);
    }

  private:
    uint64_t uses_ = 0;
    kt_ctx *pin_ctx_ = nullptr, *bpin_ctx_ = nullptr;
    void *pin_ptr_ = nullptr, *bpin_ptr_ = nullptr;
    size_t pin_bytes_ = 0, bpin_bytes_ = 0;
};

template <class T>
class Channel {
    std::mutex m_;
    std::condition_variable cv_;
    std::deque<T> q_;
    bool closed_ = false;

  public:
    void push(T v) {
        {
            std::lock_guard<std::mutex> l(m_);
            q_.push_back(v);
        }
        cv_.notify_one();
    }
    void close() {
        {
            std::lock_guard<std::mutex> l(m_);
            closed_ = true;
        }
        cv_.notify_all();
    }
    bool pop(T &v) {  // false once closed and drained
        std::unique_lock<std::mutex> l(m_);
        cv_.wait(l, [&] { return !q_.empty() || closed_; });
        if (q_.empty()) return false;
        v = q_.front();
        q_.pop_front();
        return true;
    }
};

// Writes formatted batches on its own thread, so formatting batch i + 1 overlaps the write of batch i.
// write() swaps the caller's pieces with a drained spare (capacities survive, nothing is reallocated)
// and blocks only when two batches are already waiting.  It takes the stream of an OutFile declared before it (leaving the
// scope finishes the writer, then closes the file) and does not look at what fwrite returns: its commands report no write error.
class AsyncWriter {
    using Pieces = std::vector<std::string>;
    FILE *out_;
    PhaseTimer &pt_;
    Pieces bufs_[3];
    Channel<Pieces *> todo_, spare_;
    std::thread th_;
    bool finished_ = false;

  public:
    AsyncWriter(FILE *out, PhaseTimer &pt) : out_(out), pt_(pt) {
        for (auto &b : bufs_) spare_.push(&b);
        th_ = std::thread([this] {
            Pieces *p = nullptr;
            while (todo_.pop(p)) {
                Lap lap;
                for (const auto &s : *p) fwrite(s.data(), 1, s.size(), out_);
                pt_.t[3] += lap();
                spare_.push(p);
            }
        });
    }
    void write(Pieces &pieces) {
        Pieces *p = nullptr;
        spare_.pop(p);
        p->swap(pieces);
        todo_.push(p);
    }
    void finish() {  // call before fclose(out)
        if (finished_) return;
        finished_ = true;
        todo_.close();
        th_.join();
    }
    ~AsyncWriter() { finish(); }
};

// Batch limits can be lowered from the environment (KT_CLI_BATCH_READS / KT_CLI_BATCH_BASES): the tests use it to
// push a small file through many batches (the rotating work items, the ordered writer, several table adds).
static uint64_t env_u64_host(const char *name, uint64_t dflt) {  // unset or empty: dflt; "0" is a value
    const char *v = getenv(name);
    return v && *v ? strtoull(v, nullptr, 10) : dflt;
}
static uint64_t env_cap(const char *name, uint64_t v) {  // lowers v only: unset, empty, 0 and anything above v leave it
    const uint64_t c = env_u64_host(name, 0);
    return c && c < v ? c : v;
}
static uint64_t cli_batch_reads(uint64_t v) { return env_cap("KT_CLI_BATCH_READS", v); }
static uint64_t cli_batch_bases(uint64_t v) { return env_cap("KT_CLI_BATCH_BASES", v); }

// device(w): fills w.rows from w.b, returns "" or an error message.  emit(w): writes the text.
static std::string run_pipeline(SeqReader &reader, uint64_t max_bases, uint64_t max_reads, PhaseTimer &pt,
                                const std::function<std::string(Work &)> &device,
                                const std::function<void(Work &)> &emit, bool keep_ids = false) {
    max_bases = cli_batch_bases(max_bases);
    max_reads = cli_batch_reads(max_reads);
    constexpr int DEPTH = 3;
    Work items[DEPTH];
    Channel<Work *> free_q, read_q, done_q;
    for (auto &w : items) free_q.push(&w);
    std::atomic<bool> stop{false};
    std::thread reader_thread([&] {
        Work *w = nullptr;
        bool more = true;
        Lap lap;
        while (more && !stop.load() && free_q.pop(w)) {
            lap();
            more = reader.next_batch(w->b, max_bases, max_reads, keep_ids);
            pt.t[0] += lap();
            if (w->b.n_reads()) read_q.push(w); else free_q.push(w);
        }
        read_q.close();
    });
    std::thread emit_thread([&] {
        Work *w = nullptr;
        while (done_q.pop(w)) {
            emit(*w);
            free_q.push(w);
        }
    });
    std::string err;
    Work *w = nullptr;
    while (read_q.pop(w)) {
        if (err.empty()) {
            Lap lap;
            err = device(*w);
            pt.t[1] += lap();
        }
        if (!err.empty()) {  // drain: let the reader see `stop` and finish
            stop.store(true);
            free_q.push(w);
            continue;
        }
        done_q.push(w);
    }
    done_q.close();
    reader_thread.join();
    emit_thread.join();
    if (err.empty() && reader.failed()) err = reader.error();
    return err;
}

static uint64_t batch_bases(uint64_t memory) {
    const uint64_t cap = 64ull << 20;  // small enough that a file of a few batches still overlaps its stages
    return memory < cap ? (memory ? memory : 1) : cap;
}

static const uint8_t *bases_ptr(const Batch &b) { return b.bases.empty() ? (const uint8_t *)"" : b.bases.data(); }

// ---- what the table commands share: small text files, the input walk, values kept across passes ------------------
// a whole small file from a string: "" or the error message
static std::string write_text_file(const std::string &path, const std::string &text) {
    OutFile out;
    if (std::string e = out.open(path); !e.empty()) return e;
    out.write(text);
    return out.close();
}

// "name\tvalue\n" lines (the *.stats files)
static void append_stats_rows(std::string &s, const char *const *names, const uint64_t *values, size_t n) {
    for (size_t j = 0; j < n; j++) s += std::string(names[j]) + '\t' + std::to_string(values[j]) + '\n';
}
// a *.stats file of such lines and nothing else
static std::string write_stats_file(const std::string &path, const char *const *names, const uint64_t *values, size_t n) {
    std::string s;
    append_stats_rows(s, names, values, n);
    return write_text_file(path, s);
}

// one FASTA / FASTQ record: header line, `len` bases on one line, for FASTQ "+" and `len` quality bytes
static void append_record(std::string &out, bool fastq, const std::string &header, const uint8_t *bases, const uint8_t *quals,
                          uint64_t len) {
    out += fastq ? '@' : '>';
    out += header;
    out += '\n';
    out.append((const char *)bases, len);
    out += '\n';
    if (fastq) {
        out += "+\n";
        out.append((const char *)quals, len);
        out += '\n';
    }
}

// a k-mer as its letters (counter/src/lib.rs:221-226) or as its number
static void append_kmer(std::string &s, uint64_t key, int k, bool acgt) {
    char buf[40];
    if (acgt) {
        kt_numeric_to_kmer(key, k, buf);
        s += buf;
    } else {
        const auto r = std::to_chars(buf, buf + sizeof buf, key);
        s.append(buf, (size_t)(r.ptr - buf));
    }
}

static void append_uint(std::string &out, uint64_t v) {
    char buf[24];
    const auto e = std::to_chars(buf, buf + sizeof buf, v);
    out.append(buf, (size_t)(e.ptr - buf));
}
static std::string matrix_text(const std::vector<uint64_t> &m, uint32_t R, uint32_t C) {  // R lines of C tab-separated counts
    std::string s;
    s.reserve((size_t)R * C * 2);
    for (uint32_t r = 0; r < R; r++)
        for (uint32_t c = 0; c < C; c++) append_uint(s, m[(size_t)r * C + c]), s += c + 1 < C ? '\t' : '\n';
    return s;
}
static void append_tab_uints(std::string &out, std::initializer_list<uint64_t> vs) {  // "\t{v}" for every v
    for (const uint64_t v : vs) out += '\t', append_uint(out, v);
}

// The input walk of every command that does not go through run_pipeline: batches of at most max_bases / max_reads
// (lowered by KT_CLI_BATCH_*, here and nowhere else) until the reader has no more, fn(b, at) for every batch with reads -
// `at`: the reads and bases in front of the batch -, nothing more after the first error, the reader's or fn's.  The
// reader and the batch are the caller's: whether they live across passes (count, compare, setop: one of each, rewound) or
// per pass (the pass hooks) is the caller's choice, and so is what fn does with a batch without bases.  pt / lap: the
// time of next_batch is booked as read time; fn books its own.  *end: the whole input's reads and bases.
template <class F>
static std::string walk(SeqReader &reader, Batch &b, uint64_t max_bases, uint64_t max_reads, bool keep_records, PhaseTimer *pt,
                        Lap *lap, Cursor *end, F fn) {
    max_bases = cli_batch_bases(max_bases);
    max_reads = cli_batch_reads(max_reads);
    Cursor at;
    for (;;) {
        const bool more = reader.next_batch(b, max_bases, max_reads, false, keep_records);
        if (pt) pt->t[0] += (*lap)();
        if (const uint64_t n = b.n_reads()) {
            if (std::string e = fn(b, at); !e.empty()) return e;
            at.reads += n;
            at.bases += b.offsets[n];
        }
        if (!more) break;
    }
    if (reader.failed()) return reader.error();
    if (end) *end = at;
    return "";
}
static const uint64_t TABLE_BATCH_BASES = 256ull << 20;  // of every walk; the table plan's reserve is a multiple of it

std::string KeptAcrossPasses::inside(const Cursor &at, const Batch &b) const {
    const uint64_t n = b.n_reads();
    return at.reads + n > seen.reads || at.bases + b.offsets[n] > seen.bases ? changed() : "";
}

std::string KeptAcrossPasses::finish(bool first, const Cursor &end) {
    if (first) seen = end;
    else if (end.reads != seen.reads || end.bases != seen.bases) return changed();
    return "";
}

std::string KeptAcrossPasses::over_ceiling(uint64_t bases, unsigned bytes_per_base, const char *what, uint32_t passes,
                                           double ceil_gb) const {
    const double bytes = (double)bases * (double)bytes_per_base;
    if (!(bytes > ceil_gb * (double)(1ull << 30))) return "";
    char msg[320];
    snprintf(msg, sizeof msg,
             "%s: the table takes %u passes, and the %s of the input kept across them (%u bytes per base, more than %.1f GB) do "
             "not fit the memory ceiling of %.0f GB: raise -m or split the input",
             cmd, passes, what, bytes_per_base, bytes / (double)(1ull << 30), ceil_gb);
    return msg;
}

// writes `rows` (n x bins) as delimited text: {:.6} when normalised, Display otherwise
static void emit_matrix(AsyncWriter &writer, const Work &w, uint64_t bins, bool norm, const std::string &delim, int threads,
                        std::vector<std::string> &pieces, PhaseTimer &pt) {
    Lap lap;
    const double *rows = w.rows.data();
    format_rows(w.b.n_reads(), threads, bins * (norm ? 9 : 4) + 1, pieces, [&](uint64_t r, std::string &s) {
        const double *row = rows + r * bins;
        char buf[FIXED6_BUF];
        for (uint64_t i = 0; i < bins; i++) {
            if (i) s += delim;
            if (norm) s.append(buf, format_fixed6(buf, row[i])); else append_display(s, row[i]);
        }
        s += '\n';
    });
    pt.t[2] += lap();
    writer.write(pieces);
}

// the same for raw counts delivered as u32 (`-c`: half the device-to-host bytes of f64 rows, integers print bare)
static void emit_counts(AsyncWriter &writer, const Work &w, uint64_t bins, const std::string &delim, int threads,
                        std::vector<std::string> &pieces, PhaseTimer &pt) {
    Lap lap;
    const uint32_t *rows = reinterpret_cast<const uint32_t *>(w.rows.data());
    const char d0 = delim.size() == 1 ? delim[0] : ' ';
    format_rows(w.b.n_reads(), threads, bins * 4 + 1, pieces, [&](uint64_t r, std::string &s) {
        const uint32_t *row = rows + r * bins;
        char buf[16];
        for (uint64_t i = 0; i < bins; i++) {
            if (i) {
                if (delim.size() == 1) s += d0; else s += delim;
            }
            const uint32_t v = row[i];
            if (v < 10) {
                s += (char)('0' + v);
            } else {
                const auto res = std::to_chars(buf, buf + sizeof buf, v);
                s.append(buf, (size_t)(res.ptr - buf));
            }
        }
        s += '\n';
    });
    pt.t[2] += lap();
    writer.write(pieces);
}

// hidden `kmertools debug-emit`: times the text stage alone on fabricated count-ratio rows
double debug_emit_bench(uint64_t n_rows, uint64_t bins, bool norm, int threads, int reps) {
    Work w;
    w.b.clear();
    for (uint64_t r = 0; r < n_rows; r++) w.b.offsets.push_back(r + 1);
    w.resize_rows(n_rows * bins);
    for (uint64_t i = 0; i < n_rows * bins; i++) {
        const double c = (double)((i * 2654435761ull >> 7) % 5);
        w.rows[i] = norm ? c / 147.0 : c;
    }
    OutFile out;
    (void)out.open("/dev/null");
    std::vector<std::string> pieces;
    PhaseTimer pt("debug-emit");
    double best = 1e30;
    for (int i = 0; i < reps; i++) {
        Lap lap;
        {
            AsyncWriter writer(out.stream(), pt);
            emit_matrix(writer, w, bins, norm, " ", threads, pieces, pt);
        }
        const double d = lap();
        if (d < best) best = d;
    }
    return best;
}

// ---------------------------------------------------------------------------------------------
OligoComputer::OligoComputer(std::string in_path, std::string out_path, int ksize, bool count_min)
    : in_path_(std::move(in_path)), out_path_(std::move(out_path)), ksize_(ksize), count_min_(count_min) {}

std::vector<std::string> OligoComputer::get_header() const {
    std::vector<std::string> h;
    char buf[40];
    if (count_min_) {
        uint64_t bins = 0;
        kt_bins(ksize_, 1, &bins);
        std::vector<uint64_t> canon(bins);
        uint32_t kcount = 0;
        kt_pos_map(ksize_, nullptr, canon.data(), &kcount);
        for (uint64_t i = 0; i < kcount; i++) {
            kt_numeric_to_kmer(canon[i], ksize_, buf);
            h.emplace_back(buf);
        }
    } else {
        const uint64_t n = 1ull << (2 * ksize_);
        for (uint64_t km = 0; km < n; km++) {
            kt_numeric_to_kmer(km, ksize_, buf);
            h.emplace_back(buf);
        }
    }
    return h;
}

std::string OligoComputer::vectorise() {
    SeqReader reader;
    // the reference sniffs the first byte on its batch path (stdin or raw counts) and trusts the
    // extension on its mmap path; an unknown extension falls back to sniffing here
    if (!reader.open(in_path_, in_path_ == "-" || !norm_)) return reader.error();
    OutFile out;
    if (std::string e = out.open(out_path_); !e.empty()) return e;
    // (the device context is created by the first device call: HIP start-up, 0.1-0.3 s, then runs while the reader
    // thread parses the first batch)
    uint64_t bins = 0;
    kt_bins(ksize_, count_min_, &bins);
    if (header_) {
        std::string line;
        const auto h = get_header();
        for (size_t i = 0; i < h.size(); i++) {
            if (i) line += delim_;
            line += h[i];
        }
        line += "\n";
        out.write(line);
    }
    std::vector<std::string> pieces;
    PhaseTimer pt("comp oligo");
    AsyncWriter writer(out.stream(), pt);
    return run_pipeline(
        reader, batch_bases(memory_), 1ull << 19, pt,
        [&](Work &w) -> std::string {
            if (std::string e = dev_.ensure(); !e.empty()) return e;
            const uint64_t n = w.b.n_reads();
            // normalised rows are f64 (the reference's type, bit-identical); raw counts travel as u32
            w.resize_rows(norm_ ? n * bins : (n * bins + 1) / 2);
            w.pin_rows(dev_.ctx);
            w.pin_bases(dev_.ctx);
            if (kt_oligo_batch(dev_.ctx, bases_ptr(w.b), w.b.offsets.data(), n, ksize_, count_min_, norm_, 1,
                               norm_ ? KT_F64 : KT_U32, w.rows.data(), KT_MEM_HOST) != KT_OK)
                return kt_last_error();
            return "";
        },
        [&](Work &w) {
            if (norm_) emit_matrix(writer, w, bins, true, delim_, threads_, pieces, pt);
            else emit_counts(writer, w, bins, delim_, threads_, pieces, pt);
        });
}

// ---------------------------------------------------------------------------------------------
OligoCgrComputer::OligoCgrComputer(std::string in_path, std::string out_path, int ksize, uint64_t vecsize)
    : in_path_(std::move(in_path)), out_path_(std::move(out_path)), ksize_(ksize), vecsize_(vecsize) {}

std::string OligoCgrComputer::vectorise() {
    SeqReader reader;
    if (!reader.open(in_path_, true)) return reader.error();  // oligocgr.rs:64-72 sniffs '>'
    OutFile out;
    if (std::string e = out.open(out_path_); !e.empty()) return e;
    if (std::string e = dev_.ensure(); !e.empty()) return e;
    uint64_t bins = 0;
    kt_bins(ksize_, 1, &bins);
    // the CGR point of every canonical k-mer is read-independent: build "(x,y," once
    std::vector<double> xy(bins * 2);
    kt_cgr_coords(ksize_, (double)vecsize_, xy.data());
    std::vector<std::string> prefix(bins);
    for (uint64_t i = 0; i < bins; i++) {
        std::string &p = prefix[i];
        p = "(";
        append_display(p, xy[2 * i]);
        p += ",";
        append_display(p, xy[2 * i + 1]);
        p += ",";
    }
    std::vector<std::string> pieces;
    PhaseTimer pt("comp cgr -k");
    AsyncWriter writer(out.stream(), pt);
    // rows are 8 * bins bytes each: bound the batch by reads as well
    const uint64_t max_reads = bins >= 2048 ? 8192 : 262144;
    return run_pipeline(
        reader, batch_bases(memory_), max_reads, pt,
        [&](Work &w) -> std::string {
            const uint64_t n = w.b.n_reads();
            w.resize_rows(n * bins);
            w.pin_rows(dev_.ctx);
            w.pin_bases(dev_.ctx);
            if (kt_oligo_batch(dev_.ctx, bases_ptr(w.b), w.b.offsets.data(), n, ksize_, 1, norm_, 1, KT_F64, w.rows.data(),
                               KT_MEM_HOST) != KT_OK)
                return kt_last_error();
            return "";
        },
        [&](Work &w) {
            Lap lap;
            const double *rows = w.rows.data();
            format_rows(w.b.n_reads(), threads_, bins * 24, pieces, [&](uint64_t r, std::string &s) {
                const double *row = rows + r * bins;
                for (uint64_t i = 0; i < bins; i++) {
                    if (i) s += ' ';
                    s += prefix[i];
                    append_display(s, row[i]);
                    s += ')';
                }
                s += '\n';
            });
            pt.t[2] += lap();
            writer.write(pieces);
        });
}

// ---------------------------------------------------------------------------------------------
CgrComputer::CgrComputer(std::string in_path, std::string out_path, uint64_t vecsize)
    : in_path_(std::move(in_path)), out_path_(std::move(out_path)), vecsize_(vecsize) {}

std::string CgrComputer::vectorise() {
    SeqReader reader;
    if (!reader.open(in_path_, true)) return reader.error();  // cgr.rs:68-76 sniffs '>'
    OutFile out;
    if (std::string e = out.open(out_path_); !e.empty()) return e;
    if (std::string e = dev_.ensure(); !e.empty()) return e;
    std::vector<std::string> pieces;
    PhaseTimer pt("comp cgr (whole sequence)");
    AsyncWriter writer(out.stream(), pt);
    // 16 bytes of points and ~40 bytes of text per base: keep the batches small
    return run_pipeline(
        reader, 16ull << 20, 1ull << 18, pt,
        [&](Work &w) -> std::string {
            const uint64_t n = w.b.n_reads();
            w.resize_rows(2 * w.b.bases.size() + 2);
            w.pin_rows(dev_.ctx);
            w.pin_bases(dev_.ctx);
            if (kt_cgr_points(dev_.ctx, bases_ptr(w.b), w.b.offsets.data(), n, (double)vecsize_, w.rows.data(), nullptr,
                              KT_MEM_HOST) != KT_OK)
                return kt_last_error();
            return "";
        },
        [&](Work &w) {
            Lap lap;
            const double *xy = w.rows.data();
            const uint64_t *off = w.b.offsets.data();
            const uint64_t n = w.b.n_reads();
            const size_t per_row = n ? (size_t)(w.b.bases.size() / n + 1) * 44 : 1;
            format_rows(n, threads_, per_row, pieces, [&](uint64_t r, std::string &s) {
                for (uint64_t g = off[r]; g < off[r + 1]; g++) {  // "({},{})" joined by " " (:97-102)
                    if (g != off[r]) s += ' ';
                    s += '(';
                    append_display(s, xy[2 * g]);
                    s += ',';
                    append_display(s, xy[2 * g + 1]);
                    s += ')';
                }
                s += '\n';
            });
            pt.t[2] += lap();
            writer.write(pieces);
        });
}

// ---------------------------------------------------------------------------------------------
CountComputer::CountComputer(std::string in_path, std::string out_dir, int ksize)
    : in_path_(std::move(in_path)), out_dir_(std::move(out_dir)), ksize_(ksize) {}

CountComputer::~CountComputer() {
    release_shards();
    if (ctr_) kt_ctr_destroy(ctr_);
}

kt_ctr *CountComputer::shard_table(size_t r) const {
    kt_ctr *t = nullptr;
    if (!sharded_done_ || r >= shards_.size() || !shards_[r] || kt_sharded_table(shards_[r], &t) != KT_OK) return nullptr;
    return t;
}

void CountComputer::release_shards() {
    for (auto *&sh : shards_)
        if (sh) kt_sharded_destroy(sh), sh = nullptr;
    for (auto *&c : shard_ctx_)
        if (c) kt_ctx_destroy(c), c = nullptr;
}

// What the process holds, from the kernel's and the allocator's books (KT_CLI_TIMING): VmHWM is the peak of the resident
// set - anonymous + file + shared pages, the HIP runtime's mappings among them -, `heap` is what malloc has handed out and
// not got back (mallinfo2: uordblks of the arenas + hblkhd of its own mmaps), which is what this program's buffers are.
struct MemReport {
    uint64_t hwm_kb = 0, rss_kb = 0, anon_kb = 0, file_kb = 0, shmem_kb = 0, heap_kb = 0, heap_free_kb = 0;
};
static uint64_t heap_in_use_kb() {
    const struct mallinfo2 mi = mallinfo2();
    return (uint64_t)(mi.uordblks + mi.hblkhd) >> 10;
}
static MemReport mem_report() {
    MemReport r;
    if (FILE *f = fopen("/proc/self/status", "r")) {
        char line[256];
        while (fgets(line, sizeof line, f)) {
            if (strncmp(line, "VmHWM:", 6) == 0) r.hwm_kb = strtoull(line + 6, nullptr, 10);
            else if (strncmp(line, "VmRSS:", 6) == 0) r.rss_kb = strtoull(line + 6, nullptr, 10);
            else if (strncmp(line, "RssAnon:", 8) == 0) r.anon_kb = strtoull(line + 8, nullptr, 10);
            else if (strncmp(line, "RssFile:", 8) == 0) r.file_kb = strtoull(line + 8, nullptr, 10);
            else if (strncmp(line, "RssShmem:", 9) == 0) r.shmem_kb = strtoull(line + 9, nullptr, 10);
        }
        fclose(f);
    }
    const struct mallinfo2 mi = mallinfo2();
    r.heap_kb = (uint64_t)(mi.uordblks + mi.hblkhd) >> 10;
    r.heap_free_kb = (uint64_t)mi.fordblks >> 10;
    return r;
}
static uint64_t peak_rss_kb() { return mem_report().hwm_kb; }

// The table's lines, a slab at a time: the entries are staged on the device and fetched `slab` entries at a time, so the
// host holds one slab of (key, count) pairs and its text whatever the table's size - the reference's map.scan streams
// into the file the same way (counter/src/lib.rs:220-230).  `ceil_gb` (-m): the slab shrinks with the ceiling.
// One writer serves every slab of every pass (and every shard of --devices N): the pair arrays and the text pieces are
// allocated once and keep their capacity, so what a pass costs in host memory does not depend on how many passes went
// before it or on how many entries the pass holds (round 4 built them anew per slab: the allocator's retention of the
// freed blocks moved the process's peak by +-100 MB from run to run).
class TableWriter {
  public:
    // --min-count / --max-count: only the entries with lo <= count <= hi are staged (kt_ctr_export_stage_range; the full
    // range is kt_ctr_export_stage itself)
    TableWriter(bool acgt, int k, int threads, double ceil_gb, uint32_t lo = 1, uint32_t hi = 0xFFFFFFFFu)
        : acgt_(acgt), k_(k), threads_(threads), lo_(lo), hi_(hi) {
        // ~64 bytes of host memory per entry of a slab (12 of pairs, the rest text in flight): a million entries at a
        // time - 64 MB, far below any ceiling -m accepts (6 .. 128 GB); a sixteenth of the ceiling if that were smaller
        slab_ = (uint64_t)(ceil_gb * (double)(1ull << 30) / 16.0 / 64.0);
        if (slab_ > (1ull << 20)) slab_ = 1ull << 20;
        if (slab_ < (1ull << 16)) slab_ = 1ull << 16;
    }
    std::string write(OutFile &out, kt_ctr *ctr, uint64_t *n_out) {
        uint64_t n = 0;
        if (kt_ctr_export_stage_range(ctr, lo_, hi_, &n) != KT_OK) return kt_last_error();
        if (n && keys_.empty()) {
            keys_.resize((size_t)slab_);
            counts_.resize((size_t)slab_);
        }
        for (uint64_t i0 = 0; i0 < n; i0 += slab_) {
            const uint64_t m = n - i0 < slab_ ? n - i0 : slab_;
            if (kt_ctr_export_fetch(ctr, i0, m, keys_.data(), counts_.data()) != KT_OK) return kt_last_error();
            if (std::string e = emit(out, keys_.data(), counts_.data(), m); !e.empty()) return e;
            slabs_++;
        }
        entries_ += n;
        if (n_out) *n_out = n;
        return "";
    }
    // the same lines from (key, count) pairs the caller holds on the host (setop's result), the text a slab at a time
    std::string write_pairs(OutFile &out, const uint64_t *keys, const uint32_t *counts, uint64_t n) {
        slabs_ += (n + slab_ - 1) / slab_;
        entries_ += n;
        return emit(out, keys, counts, n);
    }
    // bytes held in the writer's own buffers (capacities: what stays allocated between slabs)
    uint64_t buffer_bytes() const {
        uint64_t b = keys_.capacity() * 8 + counts_.capacity() * 4;
        for (const auto &p : pieces_) b += p.capacity();
        return b;
    }
    uint64_t heap_peak_kb() const { return heap_peak_kb_; }
    uint64_t slab() const { return slab_; }
    uint64_t slabs() const { return slabs_; }

  private:
    // the text of m entries, a slab at a time, formatted on the workers and written
    std::string emit(OutFile &out, const uint64_t *keys, const uint32_t *counts, uint64_t m) {
        // "{kmer}\t{count}\n" (or the ACGT form), counter/src/lib.rs:220-230
        write_rows(m, slab_, threads_, pieces_, RowText(out, acgt_ ? (size_t)k_ + 13 : 32, [&](uint64_t i, std::string &s) {
            append_kmer(s, keys[i], k_, acgt_);
            append_tab_uints(s, {counts[i]});
            s += '\n';
        }));
        const uint64_t h = heap_in_use_kb();  // with a slab's pairs and its text in hand: the writer's high point
        if (h > heap_peak_kb_) heap_peak_kb_ = h;
        return out.failed() ? "Unable to write the table's lines" : "";
    }
    bool acgt_;
    int k_, threads_;
    uint32_t lo_, hi_;
    uint64_t slab_ = 0, slabs_ = 0, entries_ = 0, heap_peak_kb_ = 0;
    std::vector<uint64_t> keys_;
    std::vector<uint32_t> counts_;
    std::vector<std::string> pieces_;
};

// --prefilter (set_prefilter; the passes: below, in front of CountComputer::count)
static struct {
    bool on = false;
    uint64_t bits = 16;
    std::string out_dir;
} g_prefilter;
void set_prefilter(bool on, uint64_t bits_per_kmer, const std::string &out_dir) {
    g_prefilter.on = on, g_prefilter.bits = bits_per_kmer, g_prefilter.out_dir = out_dir;
}

// the spectrum of table t added to histo_ (out-of-core passes and shards: one table after the other into one array)
std::string CountComputer::add_spectrum(kt_ctr *t) {
    if (histo_.empty()) histo_.assign((size_t)histo_max_ + 1, 0);
    if (kt_ctr_spectrum(t, histo_.data(), histo_max_ + 1, nullptr, KT_MEM_HOST) != KT_OK) return kt_last_error();
    return "";
}

// {out_dir}/kmers.histo: "c\tn" for c = 1..H, zeros included, the last line the k-mers with H or more occurrences
std::string CountComputer::write_histo() const {
    std::string s;
    for (uint32_t c = 1; c <= histo_max_; c++) {
        s += std::to_string(c);
        s += '\t';
        // (--prefilter: the table holds only a few of the k-mers seen once; their number is not known, and 0 is written)
        s += std::to_string(c < histo_.size() && !(c == 1 && g_prefilter.on) ? histo_[c] : 0);
        s += '\n';
    }
    return write_text_file(out_dir_ + "/kmers.histo", s);
}

// ---- the table plan ----------------------------------------------------------------------------------------------
// What an input can hold: an upper bound of its bases - a plain file gives one without being read: its size (FASTA), or
// half of it (FASTQ: as many quality bytes as bases); compressed input takes the pre-pass, which counts the records too -,
// of its distinct k-mers (at most the canonical k-mers of k <= 15), and the slots wanted for them: 1.9 per possible key =
// load factor ~0.5 at worst (the library rounds up to m * 2^j, m in 5..8)
struct InputBound {
    uint64_t n_seq = 0, bases = 0, max_distinct = 0, want = 0;  // n_seq: 0 when the pre-pass was skipped
};

// --estimate-size (set_estimate_size): the plan's `want` comes down to what the input's distinct k-mers need
static struct {
    bool on = false;
    int p = 14;
    uint64_t taken = 0;  // the sum of the estimates used so far
} g_estimate;
void set_estimate_size(bool on, int precision) { g_estimate.on = on, g_estimate.p = precision; }
uint64_t estimate_size_taken() { return g_estimate.taken; }
// (the library's text for KT_ERR_FULL, kt_ctr_size: the computers hand a failed call's message on, not its code)
bool table_overflowed(const std::string &err) { return err.find("k-mer table is full") != std::string::npos; }

// One walk over an input into HyperLogLog registers (2^p bytes, combined into; `card` and the estimate of the table plan)
static std::string card_walk(kt_ctx *ctx, const std::string &path, int k, int p, uint64_t seed, std::vector<uint8_t> &registers,
                             uint64_t *n_kmers, Cursor *end) {
    SeqReader reader;
    if (!reader.open(path, false)) return reader.error();
    Batch b;
    return walk(reader, b, TABLE_BATCH_BASES, 1ull << 22, false, nullptr, nullptr, end, [&](const Batch &bb, const Cursor &) -> std::string {
        if (!bb.bases.empty() &&
            kt_card_add_reads(ctx, bb.bases.data(), bb.offsets.data(), bb.n_reads(), k, p, seed, registers.data(), n_kmers, KT_MEM_HOST) != KT_OK)
            return kt_last_error();
        return "";
    });
}

// slots for E distinct k-mers: 5 sigma on top of the estimate (its tails are somewhat heavier than Gaussian; the 1.9 slots
// per key leave far more), then the 1.9 per key of every plan
static uint64_t slots_for_estimate(double estimate, int p) {
    const double e5 = ceil(estimate * (1.0 + 5.0 * kt_card_rel_error(p)));
    if (!(e5 < 9.0e18)) return ~0ull;
    const uint64_t e = (uint64_t)e5, want = e + e / 10 * 9;
    return want < 1024 ? 1024 : want;
}

// `dev`: the device of the estimate's walk, with --estimate-size (not used without it)
static std::string slots_wanted(const std::string &path, int k, InputBound *in, Device &dev) {
    std::string err;
    struct stat st;
    const bool plain = !(path.size() > 3 && path.compare(path.size() - 3, 3, ".gz") == 0) && stat(path.c_str(), &st) == 0 &&
                       S_ISREG(st.st_mode);
    in->n_seq = 0;
    if (plain) in->bases = format_from_path(path) == SeqFormat::Fastq ? (uint64_t)st.st_size / 2 : (uint64_t)st.st_size;
    else if (!SeqReader::seq_stats(path, in->n_seq, in->bases, err)) return err;
    in->max_distinct = in->bases;
    if (k <= 15) {
        const uint64_t n4k = 1ull << (2 * k);
        const uint64_t canon = (k & 1) ? n4k / 2 : (n4k + (1ull << k)) / 2;
        if (canon < in->max_distinct) in->max_distinct = canon;
    }
    in->want = in->max_distinct + in->max_distinct / 10 * 9;
    if (in->want < 1024) in->want = 1024;
    if (!g_estimate.on) return "";
    // one extra walk: the distinct k-mers of this input, estimated (KT_CARD_SCALE, tests: a wrong estimate)
    Lap lap;
    if (std::string e = dev.ensure(); !e.empty()) return e;
    std::vector<uint8_t> registers((size_t)1 << g_estimate.p, 0);
    if (std::string e = card_walk(dev.ctx, path, k, g_estimate.p, 0, registers, nullptr, nullptr); !e.empty()) return e;
    double estimate = 0.0;
    if (kt_card_estimate(registers.data(), g_estimate.p, &estimate, nullptr) != KT_OK) return kt_last_error();
    if (const char *s = getenv("KT_CARD_SCALE"); s && *s) estimate *= strtod(s, nullptr);
    const uint64_t bound = in->want;
    in->want = std::min(bound, slots_for_estimate(estimate, g_estimate.p));
    const uint64_t shown = estimate < 9.0e18 ? (uint64_t)(estimate + 0.5) : ~0ull;
    g_estimate.taken += shown;
    if (getenv("KT_CLI_TIMING"))
        fprintf(stderr, "[timing] card pre-pass: %.3f s, estimate %llu, slots wanted %llu (bound: %llu)\n", lap(), (unsigned long long)shown,
                (unsigned long long)in->want, (unsigned long long)bound);
    return "";
}

// How many passes the tables of a command take.  The reference bounds its memory with -m: chunks of the input, partitions
// spilled to disk, merged partition by partition (counter/src/lib.rs:114-118, 151-167, 188-231).  Here the bound is the
// HBM next to the build's buffers (two key arrays + the staging of a batch: the reserve), `bytes_per_slot` for every slot
// of every table; tables that cannot hold every distinct k-mer are filled in `passes` passes over the input, pass p
// counting hash partition p only (kt_ctr_add_reads_part).  KT_CTR_MAX_SLOTS (tests: force the passes) comes in one of two
// ways, which the commands' tests rely on: for `ctr` it REPLACES the fit - a value above what the HBM holds is taken and
// left to create_tables -; for the others it bounds every single table next to the fit (default: no bound).
struct TablePlan {
    int n = 1;                   // tables, on one device
    uint64_t want[2] = {0, 0};
    uint64_t room = 0;           // slots a pass may hold (of one table, where KT_CTR_MAX_SLOTS bounds that more tightly)
    uint32_t passes = 1;
    // a partition's share of the keys varies a little: 1 / passes + 5 sigma of room
    uint64_t capacity(int i) const { return passes == 1 ? want[i] : want[i] / passes + want[i] / passes / 16 + 4096; }
    void plan(kt_ctx *ctx, uint64_t bytes_per_slot, bool env_replaces_fit) {
        uint64_t sum = 0;
        for (int i = 0; i < n; i++) sum += want[i];
        uint64_t free_b = 0, total_b = 0, fit = sum, each = ~0ull;
        if (kt_device_memory(ctx, &free_b, &total_b) == KT_OK) {
            const uint64_t reserve = TABLE_BATCH_BASES * 20 + (1ull << 30);
            const uint64_t usable = free_b > 2 * reserve ? free_b - reserve : free_b / 2;
            fit = usable / 10 * 9 / bytes_per_slot;
        }
        if (env_replaces_fit) fit = env_u64_host("KT_CTR_MAX_SLOTS", fit);
        else each = env_u64_host("KT_CTR_MAX_SLOTS", ~0ull);
        if (fit < 1024 * (uint64_t)n) fit = 1024 * (uint64_t)n;
        if (each < 1024) each = 1024;
        uint64_t p = (sum + fit - 1) / fit;
        for (int i = 0; i < n; i++) p = std::max(p, (want[i] + each - 1) / each);
        passes = (uint32_t)std::max<uint64_t>(p, 1);
        room = std::min(fit, each);
    }
};

// The plan's tables, created.  The library rounds a request up (to m * 2^j, at most 1.25x), so tables sized to the edge of
// the free HBM may not fit after all: more passes then, with none of the tables left in between.
static std::string create_tables(kt_ctx *ctx, int k, TablePlan &plan, kt_ctr **const *tables) {
    for (;; plan.passes++) {
        int rc = KT_OK;
        for (int i = 0; i < plan.n && rc == KT_OK; i++) rc = kt_ctr_create(ctx, k, plan.capacity(i), tables[i]);
        if (rc == KT_OK) return "";
        for (int i = 0; i < plan.n; i++) {
            if (*tables[i]) kt_ctr_destroy(*tables[i]);
            *tables[i] = nullptr;
        }
        if (rc != KT_ERR_NOMEM || plan.passes >= 4096) return kt_last_error();
    }
}

// ---- --table FILE: a table file (kt_ctr_save) in place of counting (every command that makes one table) ---------------------------------------------------------
// The table of a table file: planned from the file's headers (1.9 slots per entry, as every plan), created, loaded.  The
// file must fit the device in one pass - loading in hash-partition passes is not built.
static std::string table_from_file(Device &dev, const std::string &path, int k, uint64_t bytes_per_slot, const char *name, kt_ctr **table) {
    Lap setup;
    int fk = 0;
    uint64_t sections = 0, entries = 0;
    if (kt_table_file_info(path.c_str(), &fk, &sections, &entries, nullptr) != KT_OK) return kt_last_error();
    if (fk != k) return "--table " + path + " holds k = " + std::to_string(fk) + ", not " + std::to_string(k);
    if (std::string e = dev.ensure(); !e.empty()) return e;
    TablePlan plan;
    plan.want[0] = std::max<uint64_t>(1024, entries + entries / 10 * 9);
    plan.plan(dev.ctx, bytes_per_slot, false);
    const std::string no_fit = std::string(name) + ": the table file does not fit the device in one pass, and table files are not loaded in "
                               "several passes (" + std::to_string(entries) + " entries want " + std::to_string(plan.want[0]) + " slots, room for ";
    if (plan.passes > 1) return no_fit + std::to_string(plan.room) + ")";
    if (const int rc = kt_ctr_create(dev.ctx, k, plan.want[0], table); rc != KT_OK)
        return rc == KT_ERR_NOMEM ? no_fit + "fewer: " + kt_last_error() + ")" : std::string(kt_last_error());
    const double t_setup = setup();
    uint64_t added = 0;
    if (kt_ctr_add_file(*table, path.c_str(), &added) != KT_OK) return kt_last_error();
    if (getenv("KT_CLI_TIMING")) {
        uint64_t slots = plan.want[0];
        (void)kt_ctr_capacity(*table, &slots);
        fprintf(stderr, "[timing] %s table file: table of %llu slots %.3f s, %llu section(s) with %llu entries loaded %.3f s\n", name,
                (unsigned long long)slots, t_setup, (unsigned long long)sections, (unsigned long long)added, setup());
    }
    return "";
}

// One walk over an input into a table: add(b) is the library's call (kt_ctr_add_reads, kt_ctr_add_reads_part); a batch
// whose reads have no bases is not passed on.
template <class Add>
static std::string fill_table(SeqReader &reader, Batch &b, PhaseTimer &pt, Lap &lap, Add add) {
    return walk(reader, b, TABLE_BATCH_BASES, 1ull << 22, false, &pt, &lap, nullptr, [&](const Batch &bb, const Cursor &) -> std::string {
        if (!bb.bases.empty() && add(bb) != KT_OK) return kt_last_error();
        pt.t[1] += lap();
        return "";
    });
}

// ---- --prefilter: two passes over the input, k-mers seen once kept out of the table -----------------------------------------
// Pass 1 marks every k-mer in the filter's `once` array and the ones seen again in `twice` (kt_prefilter_add_reads); the
// table is then planned from what pass 1 promoted, and pass 2 counts only the k-mers marked in `twice`
// (kt_ctr_add_reads_filtered).  The host side is arithmetic alone (prefilter_sizes, prefilter_table_slots,
// prefilter_stats_text: also behind the hidden `debug-prefilter` of main.cpp, which the sanitizer builds run).
// `once`: bits_per_kmer bits for every k-mer expected, rounded up to a power of two of 64-bit words, at least 2^10 words and,
// where that is less, at most a quarter of the free device memory (0: not known); `twice`: a quarter of `once`, at least
// 2^10 words.  A request beyond 2^34 words is refused, whatever the memory.
std::string prefilter_sizes(uint64_t expected_kmers, uint64_t bits_per_kmer, uint64_t free_bytes, int *log2_once, int *log2_twice) {
    const unsigned __int128 bits = (unsigned __int128)expected_kmers * bits_per_kmer;
    const unsigned __int128 words = (bits + 63) / 64;
    if (bits_per_kmer == 0 || words > ((unsigned __int128)1 << KT_PREFILTER_MAX_LOG2))
        return "--prefilter-bits " + std::to_string(bits_per_kmer) + ": a filter of that many bits for each of the " +
               std::to_string(expected_kmers) + " k-mers this input can hold takes more than 2^" + std::to_string(KT_PREFILTER_MAX_LOG2) +
               " words";
    int a = KT_PREFILTER_MIN_LOG2;
    while (((unsigned __int128)1 << a) < words) a++;
    if (free_bytes)
        while (a > KT_PREFILTER_MIN_LOG2 && (8ull << a) > free_bytes / 4) a--;
    *log2_once = a;
    *log2_twice = std::max(KT_PREFILTER_MIN_LOG2, a - 2);
    return "";
}

// Slots for the table of pass 2: the promotions of pass 1 plus the false positives expected among the k-mers estimated -
// a k-mer seen once gets in when its four bits of `twice` happen to be set: (the share of the bits set)^4 -, times `scale`
// (KT_PREFILTER_SCALE), then the 1.9 slots per key of every plan.  An estimate, not a bound: pass 2 may overflow the table.
uint64_t prefilter_table_slots(uint64_t promotions, uint64_t twice_bits_set, int log2_twice, uint64_t expected_kmers, double scale) {
    const double fill = (double)twice_bits_set / (64.0 * (double)(1ull << log2_twice));
    const double keys = ((double)promotions + fill * fill * fill * fill * (double)expected_kmers) * scale;
    if (!(keys < 4.0e18)) return ~0ull;
    const uint64_t e = (uint64_t)ceil(keys < 0.0 ? 0.0 : keys), want = e + e / 10 * 9;
    return want < 1024 ? 1024 : want;
}

std::string prefilter_stats_text(const PrefilterStats &s) {
    std::string t;
    const std::pair<const char *, uint64_t> rows[] = {{"windows", s.windows}, {"once_words", s.once_words}, {"twice_words", s.twice_words},
                                                      {"once_bits_set", s.once_bits_set}, {"twice_bits_set", s.twice_bits_set},
                                                      {"promotions", s.promotions}, {"table_slots", s.table_slots},
                                                      {"table_keys", s.table_keys}, {"table_retries", s.table_retries}};
    for (const auto &r : rows) t += std::string(r.first) + '\t' + std::to_string(r.second) + '\n';
    return t;
}

std::string write_prefilter_stats(const PrefilterStats &s) {
    return write_text_file(g_prefilter.out_dir + "/prefilter.stats", prefilter_stats_text(s));
}

namespace {
// One --prefilter run: the filter from its creation to the stats file
struct Prefiltered {
    kt_prefilter *filter = nullptr;
    uint64_t expected = 0;  // the k-mers the input was estimated (or bounded) to hold
    PrefilterStats st;
    int log2_twice = 0;
    Prefiltered() = default;
    Prefiltered(const Prefiltered &) = delete;
    ~Prefiltered() { if (filter) kt_prefilter_destroy(filter); }

    // the request checked against the input's bound alone: before a device is opened
    static std::string check(const std::string &path, int k) {
        InputBound in;
        const bool est = g_estimate.on;
        g_estimate.on = false;  // (the bound, not the estimate: no device work here)
        Device none;
        const std::string e = slots_wanted(path, k, &in, none);
        g_estimate.on = est;
        if (!e.empty()) return e;
        int a = 0, b = 0;
        return prefilter_sizes(in.max_distinct, g_prefilter.bits, 0, &a, &b);
    }

    // the filter sized for `in` and created, then pass 1: one walk over the reader's input
    std::string pass1(Device &dev, int k, const InputBound &in, SeqReader &reader, Batch &b, PhaseTimer &pt, Lap &lap) {
        expected = std::min(in.max_distinct, in.want / 19 * 10 + 1);  // (the plan asks 1.9 slots a key)
        uint64_t free_b = 0, total_b = 0;
        if (kt_device_memory(dev.ctx, &free_b, &total_b) != KT_OK) free_b = 0;
        int a = 0;
        if (std::string e = prefilter_sizes(expected, g_prefilter.bits, free_b, &a, &log2_twice); !e.empty()) return e;
        if (kt_prefilter_create(dev.ctx, k, a, log2_twice, 0, &filter) != KT_OK) return kt_last_error();
        st.once_words = 1ull << a, st.twice_words = 1ull << log2_twice;
        if (std::string e = fill_table(reader, b, pt, lap, [&](const Batch &bb) {
                return kt_prefilter_add_reads(filter, bb.bases.data(), bb.offsets.data(), bb.n_reads(), KT_MEM_HOST);
            });
            !e.empty())
            return e;
        if (kt_prefilter_stats(filter, &st.windows, &st.promotions, &st.once_bits_set, &st.twice_bits_set) != KT_OK) return kt_last_error();
        if (getenv("KT_CLI_TIMING"))
            fprintf(stderr, "[timing] prefilter pass 1: once 2^%d words (%llu bits set), twice 2^%d words (%llu bits set), %llu windows, %llu promotions\n",
                    a, (unsigned long long)st.once_bits_set, log2_twice, (unsigned long long)st.twice_bits_set,
                    (unsigned long long)st.windows, (unsigned long long)st.promotions);
        return "";
    }
    uint64_t table_slots() const {
        double scale = 1.0;
        if (const char *s = getenv("KT_PREFILTER_SCALE"); s && *s) scale = strtod(s, nullptr);
        return prefilter_table_slots(st.promotions, st.twice_bits_set, log2_twice, expected, scale);
    }
    int add(kt_ctr *t, const Batch &bb, uint32_t passes, uint32_t pass) const {
        return kt_ctr_add_reads_filtered(t, filter, bb.bases.data(), bb.offsets.data(), bb.n_reads(), KT_MEM_HOST, passes, pass);
    }
    // pass 2 is done: the filter's memory goes back to the device
    void done() {
        if (filter) kt_prefilter_destroy(filter);
        filter = nullptr;
    }
    std::string write_stats() const { return write_prefilter_stats(st); }
};
}  // namespace

std::string CountComputer::count() {
    // init(): pre-pass for record count and total length (counter/src/lib.rs:236-249); here it
    // sizes the HBM table instead of the reference's partition count
    Lap setup;
    if (input_is_table_) {  // --table: nothing is counted; the file must fit in one pass on one device
        if (ctr_) kt_ctr_destroy(ctr_);
        ctr_ = nullptr;
        passes_ = 1;
        return table_from_file(dev_, in_path_, ksize_, 16, "table", &ctr_);
    }
    if (in_path_ == "-") return "ctr reads its input more than once and cannot take stdin";  // (the reference panics
                                                                                            // on SeqFormat::get("-"))
    const bool prefilter = g_prefilter.on;  // (the command line refuses it with --devices above 1 and with --table)
    if (prefilter)
        if (std::string e = Prefiltered::check(in_path_, ksize_); !e.empty()) return e;
    InputBound in;
    if (std::string e = slots_wanted(in_path_, ksize_, &in, dev_); !e.empty()) return e;
    seq_count_ = in.n_seq;
    total_length_ = in.bases;
    const double t_stats = setup();
    if (n_devices_ > 1) return count_sharded(in.max_distinct);
    if (std::string e = dev_.ensure(); !e.empty()) return e;
    const double t_dev = setup();
    SeqReader reader;
    Batch b;
    Prefiltered pf;
    if (prefilter) {  // pass 1, and the table planned from what it promoted instead of from the input
        if (!reader.open(in_path_, false)) return reader.error();
        PhaseTimer pt1("ctr prefilter pass 1");
        Lap lap1;
        if (std::string e = pf.pass1(dev_, ksize_, in, reader, b, pt1, lap1); !e.empty()) return e;
        in.want = pf.table_slots();
    }
    // one table, 16 bytes a slot; each pass's table is written out and cleared
    TablePlan plan;
    plan.want[0] = in.want;
    plan.plan(dev_.ctx, 16, true);
    kt_ctr **const tables[1] = {&ctr_};
    if (std::string e = create_tables(dev_.ctx, ksize_, plan, tables); !e.empty()) return e;
    passes_ = plan.passes;
    if (getenv("KT_CLI_TIMING")) {
        uint64_t slots = plan.capacity(0);
        (void)kt_ctr_capacity(ctr_, &slots);
        fprintf(stderr, "[timing] ctr setup: sizing (pre-pass only for compressed input) %.3f s, device init %.3f s, table of %llu slots, %u pass(es) %.3f s\n",
                t_stats, t_dev, (unsigned long long)slots, passes_, setup());
    }
    OutFile out;  // kmers.counts, out of core: opened when the first pass has lines for it
    PhaseTimer pt("ctr count (after the seq_stats pre-pass)");
    const bool timing = getenv("KT_CLI_TIMING") != nullptr;
    // One reader, one batch and one table writer serve every pass: a pass rewinds the reader (its threads, cuts and
    // buffers stay) and reuses the writer's slab, so after the first pass the loop allocates nothing - the host's memory
    // is the same whether the table takes 2 passes or 200 (the reference's ceiling: counter/src/lib.rs:114-118, 220-230).
    if (prefilter ? !reader.rewind() : !reader.open(in_path_, false)) return reader.error();
    TableWriter writer(acgt_, ksize_, threads_, memory_ceil_gb_, min_count_, max_count_);
    uint64_t heap_after_first = 0, rss_after_first = 0;
    struct Partial {  // --save-table out of core: removed unless the run gets to rename it
        std::string path;
        ~Partial() { if (!path.empty()) unlink(path.c_str()); }
    } partial;
    for (uint32_t pass = 0; pass < passes_; pass++) {
        if (pass && !reader.rewind()) return reader.error();
        Lap lap;
        if (std::string e = fill_table(reader, b, pt, lap, [&](const Batch &bb) {
                if (prefilter) return pf.add(ctr_, bb, passes_, pass);
                return kt_ctr_add_reads_part(ctr_, bb.bases.data(), bb.offsets.data(), bb.n_reads(), KT_MEM_HOST, passes_, pass);
            });
            !e.empty())
            return e;
        if (prefilter && passes_ == 1) {
            // the plan was an estimate: a table that overflowed is made again with twice the slots while the device has
            // room for it in one pass, and pass 2 is repeated
            uint64_t keys = 0;
            const int rc = kt_ctr_size(ctr_, &keys);
            if (rc == KT_ERR_FULL) {
                TablePlan again;
                again.want[0] = plan.want[0] * 2;
                again.plan(dev_.ctx, 16, true);
                if (again.passes > 1) return kt_last_error();
                kt_ctr_destroy(ctr_);
                ctr_ = nullptr;
                plan = again;
                if (std::string e = create_tables(dev_.ctx, ksize_, plan, tables); !e.empty()) return e;
                if (plan.passes > 1) return "ctr --prefilter: no room for a table of " + std::to_string(plan.want[0]) + " slots in one pass";
                pf.st.table_retries++;
                pass--;  // (pass 0 again; the loop's rewind is for pass > 0)
                if (!reader.rewind()) return reader.error();
                continue;
            }
            if (rc != KT_OK) return kt_last_error();
            pf.st.table_keys = keys;
            (void)kt_ctr_capacity(ctr_, &pf.st.table_slots);
            pf.done();
            if (std::string e = pf.write_stats(); !e.empty()) return e;
        }
        if (passes_ == 1) break;  // the table stays resident: merge() (and cov) read it
        // out of core: this partition is complete - whoever needs to look k-mers up does it now (cov) -
        if (pass_hook_)
            if (std::string e = pass_hook_(pass, passes_, ctr_); !e.empty()) return e;
        // - its spectrum is added to the whole table's (a k-mer lives in one partition) -
        if (histo_max_)
            if (std::string e = add_spectrum(ctr_); !e.empty()) return e;
        // - its lines go to kmers.counts, and the table is reused
        uint64_t n_pass = 0;
        if (!histo_only_) {
            if (!out.is_open())
                if (std::string e = out.open(out_dir_ + "/kmers.counts"); !e.empty()) return e;
            if (std::string e = writer.write(out, ctr_, &n_pass); !e.empty()) return e;
        }
        if (!save_table_.empty()) {  // one section per pass (a k-mer lives in one partition), under a name of its own until
            partial.path = save_table_ + ".partial";  // the last pass is in: a run that fails leaves no file that looks whole
            if (std::string e = save_table(ctr_, partial.path, pass != 0); !e.empty()) return e;
        }
        pt.t[3] += lap();
        if (timing) {
            // the ceiling's books, per pass: the program's own buffers by their capacities, the allocator's total, and
            // the kernel's view of the process (which includes the HIP runtime's ~0.6 GB)
            const MemReport r = mem_report();
            const uint64_t own = reader.buffer_bytes() + b.bases.capacity() + b.offsets.capacity() * 8 + writer.buffer_bytes();
            if (pass == 0) heap_after_first = r.heap_kb, rss_after_first = r.rss_kb;
            fprintf(stderr, "[timing] pass %u written: entries %llu, own buffers %llu kB, malloc in use %llu kB (peak at a slab boundary %llu kB), "
                            "malloc free %llu kB, VmRSS %llu kB (anon %llu, file %llu, shmem %llu), VmHWM %llu kB\n",
                    pass, (unsigned long long)n_pass, (unsigned long long)(own >> 10), (unsigned long long)r.heap_kb,
                    (unsigned long long)writer.heap_peak_kb(), (unsigned long long)r.heap_free_kb, (unsigned long long)r.rss_kb,
                    (unsigned long long)r.anon_kb, (unsigned long long)r.file_kb, (unsigned long long)r.shmem_kb,
                    (unsigned long long)r.hwm_kb);
        }
        if (prefilter) {  // (several passes: the keys of every pass's table; an overflow is the run's error, as without the flag)
            uint64_t keys = 0;
            if (kt_ctr_size(ctr_, &keys) != KT_OK) return kt_last_error();
            pf.st.table_keys += keys;
        }
        if (kt_ctr_clear(ctr_) != KT_OK) return kt_last_error();
    }
    if (prefilter && passes_ > 1) {
        (void)kt_ctr_capacity(ctr_, &pf.st.table_slots);
        if (std::string e = pf.write_stats(); !e.empty()) return e;
    }
    if (!partial.path.empty()) {
        if (rename(partial.path.c_str(), save_table_.c_str()) != 0) return "Unable to write to file: " + save_table_;
        partial.path.clear();
    }
    if (timing && passes_ > 1) {
        const MemReport r = mem_report();
        fprintf(stderr, "[timing] ctr out of core: %u passes, slabs of %llu entries, malloc peak at a slab boundary %llu kB, growth since the end "
                        "of pass 0: malloc in use %lld kB, VmRSS %lld kB, peak host memory (VmHWM) %llu kB\n",
                passes_, (unsigned long long)writer.slab(), (unsigned long long)writer.heap_peak_kb(),
                (long long)r.heap_kb - (long long)heap_after_first, (long long)r.rss_kb - (long long)rss_after_first,
                (unsigned long long)r.hwm_kb);
    }
    return "";
}

// ---- several GPUs: the table sharded by hash prefix, one worker thread (= one rank) per device -----------------
namespace {
// host all-to-all between the rank threads of one process (KT_CLI_SHARE_GPU=1: every rank on one GPU, where RCCL
// refuses to run - tests): everybody publishes its buffers, waits, copies its blocks, waits again
struct LocalFabric {
    int n;
    std::mutex m;
    std::condition_variable cv;
    int arrived = 0;
    uint64_t gen = 0;
    std::vector<const char *> send;
    explicit LocalFabric(int n_) : n(n_), send(n_) {}
    void barrier() {
        std::unique_lock<std::mutex> lk(m);
        const uint64_t g = gen;
        if (++arrived == n) {
            arrived = 0;
            gen++;
            cv.notify_all();
        } else {
            cv.wait(lk, [&] { return gen != g; });
        }
    }
};
struct FabricEnd { LocalFabric *f; int rank; };
int local_alltoall(void *user, const void *send, void *recv, uint64_t bytes) {
    FabricEnd *e = (FabricEnd *)user;
    e->f->send[e->rank] = (const char *)send;
    e->f->barrier();
    for (int p = 0; p < e->f->n; p++) memcpy((char *)recv + (uint64_t)p * bytes, e->f->send[p] + (uint64_t)e->rank * bytes, bytes);
    e->f->barrier();
    return 0;
}
}  // namespace

std::string CountComputer::count_sharded(uint64_t max_distinct) {
    const int N = n_devices_;
    const bool share = getenv("KT_CLI_SHARE_GPU") != nullptr;
    const uint64_t batch_bases = 256ull << 20, max_batch = batch_bases * 2;  // (a batch ends with a whole record)
    uint64_t per_rank = max_distinct / N + max_distinct / N / 16 + 4096;
    uint64_t cap = per_rank + per_rank / 10 * 9;
    uint8_t id[128] = {};
    if (!share) {
        // a rank thread whose device does not exist would leave the others waiting in ncclCommInitRank
        int n_dev = 0;
        if (kt_device_count(&n_dev) != KT_OK) return kt_last_error();
        if (dev_.index + N > n_dev)
            return "--devices " + std::to_string(N) + " from device " + std::to_string(dev_.index) + ": this node has " +
                   std::to_string(n_dev) + " GPU(s)";
        if (kt_rccl_unique_id(id) != KT_OK) return kt_last_error();
    }
    LocalFabric fabric(N);
    std::atomic<int> created_ok{0};
    const char *inject = getenv("KT_CLI_FAIL_RANK");  // tests: this rank's bring-up fails
    std::vector<FabricEnd> ends(N);
    release_shards();
    shards_.assign(N, nullptr);
    shard_ctx_.assign(N, nullptr);
    // rounds: the reader fills one batch per rank, the ranks add them collectively (a rank without a batch adds 0 reads)
    std::vector<Batch> batches[2];
    batches[0].resize(N);
    batches[1].resize(N);
    std::mutex m;
    std::condition_variable cv;
    int ready_round = -1, done_count[2] = {0, 0};
    bool last_round[2] = {false, false};
    std::vector<std::string> errs(N);
    auto worker = [&](int rank) {
        kt_ctx *ctx = nullptr;
        kt_sharded *sh = nullptr;
        auto fail = [&](const std::string &e) { errs[rank] = e.empty() ? "error" : e; };
        // bring-up in two steps with an agreement in between: everything a rank can fail at on its own (its device, its
        // allocations) happens first; only when EVERY rank got through does anyone enter a collective - the communicator's
        // creation, then the counting.  Otherwise all ranks stop here with the error (no rank is left waiting for one
        // that never comes).
        int rc = kt_ctx_create(share ? dev_.index : dev_.index + rank, nullptr, 1, &ctx);
        if (rc == KT_OK) rc = kt_sharded_create_local(ctx, ksize_, cap, max_batch, N, rank, &sh);
        const bool injected = rc == KT_OK && inject && atoi(inject) == rank;
        if (rc == KT_OK && !injected) created_ok.fetch_add(1);
        else fail(injected ? "injected bring-up failure (KT_CLI_FAIL_RANK)" : kt_last_error());
        fabric.barrier();
        const bool all_up = created_ok.load() == N;
        if (all_up) {
            ends[rank] = FabricEnd{&fabric, rank};
            rc = share ? kt_sharded_connect_host(sh, local_alltoall, &ends[rank]) : kt_sharded_connect_rccl(sh, id);
            if (rc != KT_OK) fail(kt_last_error());  // (a communicator that fails on one rank fails on its peers too)
        } else {
            if (errs[rank].empty()) fail("another device's bring-up failed");
            if (sh) kt_sharded_destroy(sh);
            sh = nullptr;
        }
        for (int round = 0;; round++) {
            bool last;
            {
                std::unique_lock<std::mutex> lk(m);
                cv.wait(lk, [&] { return ready_round >= round; });
                last = last_round[round & 1];
            }
            Batch &b = batches[round & 1][rank];
            // every rank takes part in every collective call, failed or not (the others would wait for ever)
            if (sh) {
                const uint64_t n = b.bases.empty() ? 0 : b.n_reads();
                if (kt_sharded_add_reads(sh, b.bases.data(), b.offsets.data(), n, KT_MEM_HOST) != KT_OK && errs[rank].empty())
                    fail(kt_last_error());
            }
            {
                std::lock_guard<std::mutex> lk(m);
                done_count[round & 1]++;
            }
            cv.notify_all();
            if (last) break;
        }
        if (sh) {
            if (kt_sharded_finalize(sh) != KT_OK && errs[rank].empty()) fail(kt_last_error());
            kt_ctr *t = nullptr;
            uint64_t n = 0;
            if (errs[rank].empty() && (kt_sharded_table(sh, &t) != KT_OK || kt_ctr_size(t, &n) != KT_OK)) fail(kt_last_error());
        }
        // the shard stays where it is: merge() writes it out in slabs (the reference streams its partitions into the file
        // the same way, counter/src/lib.rs:220-230) - no rank's export is ever held in host memory as a whole
        shards_[rank] = sh;
        shard_ctx_[rank] = ctx;
    };
    std::vector<std::thread> threads;
    for (int r = 0; r < N; r++) threads.emplace_back(worker, r);
    SeqReader reader;
    std::string err;
    if (!reader.open(in_path_, false)) err = reader.error();
    bool more = err.empty();
    for (int round = 0;; round++) {
        {   // the buffers of this parity are free once the round that used them last has been processed
            std::unique_lock<std::mutex> lk(m);
            cv.wait(lk, [&] { return round < 2 || done_count[round & 1] == N; });
            done_count[round & 1] = 0;
        }
        for (int r = 0; r < N; r++) {
            Batch &b = batches[round & 1][r];
            b.clear();
            if (more) more = reader.next_batch(b, cli_batch_bases(batch_bases), cli_batch_reads(1ull << 22));
        }
        if (reader.failed() && err.empty()) err = reader.error();
        {
            std::lock_guard<std::mutex> lk(m);
            last_round[round & 1] = !more;
            ready_round = round;
        }
        cv.notify_all();
        if (!more) break;
    }
    for (auto &t : threads) t.join();
    for (const auto &e : errs)
        if (!e.empty() && err.empty()) err = e;
    sharded_done_ = err.empty();
    return err;
}

// --save-table: the table's entries in the count range as one section of the table file
std::string CountComputer::save_table(kt_ctr *t, const std::string &path, bool append) {
    Lap lap;
    uint64_t n = 0;
    if (kt_ctr_save(t, path.c_str(), min_count_, max_count_, append ? 1 : 0, &n) != KT_OK) return kt_last_error();
    if (getenv("KT_CLI_TIMING"))
        fprintf(stderr, "[timing] ctr --save-table: section of %llu entries %s %.3f s\n", (unsigned long long)n, append ? "appended" : "written", lap());
    return "";
}

std::string CountComputer::merge(bool /*del: no temp files exist to delete*/) {
    // out of core: count() wrote every partition's lines as it completed (and summed their spectra)
    if (passes_ > 1) return histo_max_ ? write_histo() : "";
    const std::string path = out_dir_ + "/kmers.counts";
    if (sharded_done_) {  // the shards, one after the other, each in slabs (the reference's line order is unspecified)
        OutFile out;
        if (!histo_only_)
            if (std::string e = out.open(path); !e.empty()) return e;
        std::string err;
        TableWriter writer(acgt_, ksize_, threads_, memory_ceil_gb_, min_count_, max_count_);
        for (size_t r = 0; r < shards_.size() && err.empty(); r++) {
            kt_ctr *t = nullptr;
            if (kt_sharded_table(shards_[r], &t) != KT_OK) err = kt_last_error();
            else if (histo_max_ && !(err = add_spectrum(t)).empty()) break;  // (the shards' spectra are summed)
            else if (out.is_open()) err = writer.write(out, t, nullptr);
        }
        if (err.empty() && histo_max_) err = write_histo();
        if (getenv("KT_CLI_TIMING"))
            fprintf(stderr, "[timing] ctr --devices %d written: VmHWM %llu kB\n", n_devices_, (unsigned long long)peak_rss_kb());
        if (!keep_shards_) release_shards();
        return err;
    }
    if (!ctr_) return "count() has not run";
    PhaseTimer pt("ctr merge");
    Lap lap;
    if (!save_table_.empty())
        if (std::string e = save_table(ctr_, save_table_, false); !e.empty()) return e;
    if (histo_max_) {
        if (std::string e = add_spectrum(ctr_); !e.empty()) return e;
        if (std::string e = write_histo(); !e.empty()) return e;
        if (histo_only_) return "";
    }
    OutFile out;
    if (std::string e = out.open(path); !e.empty()) return e;
    TableWriter writer(acgt_, ksize_, threads_, memory_ceil_gb_, min_count_, max_count_);
    const std::string e = writer.write(out, ctr_, nullptr);
    pt.t[2] += lap();
    (void)out.close();
    pt.t[3] += lap();
    if (getenv("KT_CLI_TIMING")) fprintf(stderr, "[timing] ctr merge: peak host memory (VmHWM) %llu kB\n", (unsigned long long)peak_rss_kb());
    return e;
}

// ---------------------------------------------------------------------------------------------
CovComputer::CovComputer(std::string in_path, std::string out_dir, int ksize, uint64_t bin_size, uint64_t bin_count)
    : in_path_(in_path), in_path_kmer_(std::move(in_path)), out_dir_(std::move(out_dir)), ksize_(ksize),
      bin_size_(bin_size), bin_count_(bin_count) {}

CovComputer::~CovComputer() { delete ctr_; }

// one pass of an out-of-core table is complete: the raw bin counts of every read's k-mers of this hash partition
std::string CovComputer::cov_pass(uint32_t pass, uint32_t passes, kt_ctr *table) {
    SeqReader reader;
    if (!reader.open(in_path_, false)) return reader.error();
    Batch batch;
    Cursor end;
    const std::string e = walk(reader, batch, TABLE_BATCH_BASES, bin_count_ >= 2048 ? 8192 : 1ull << 19, false, nullptr, nullptr, &end,
                               [&](const Batch &b, const Cursor &at) -> std::string {
        const uint64_t n = b.n_reads();
        if (std::string c = kept_.claim(pass == 0, acc_rows_, (at.reads + n) * bin_count_, 0u); !c.empty()) return c;
        if (kt_cov_batch_part(table, bases_ptr(b), b.offsets.data(), n, bin_size_, bin_count_, acc_rows_.data() + at.reads * bin_count_,
                              KT_MEM_HOST, passes, pass) != KT_OK)
            return kt_last_error();
        return "";
    });
    return e.empty() ? kept_.finish(pass == 0, end) : e;
}

std::string CovComputer::build_table() {
    delete ctr_;
    acc_rows_.clear();
    kept_.seen = Cursor();
    ctr_ = new CountComputer(in_path_kmer_, out_dir_, ksize_);
    ctr_->set_threads(threads_);
    ctr_->set_max_memory(memory_ceil_gb_);
    ctr_->set_device(device_);
    ctr_->set_devices(n_devices_);
    ctr_->set_keep_shards(true);
    ctr_->set_input_is_table(kmer_is_table_);
    ctr_->set_pass_hook([this](uint32_t pass, uint32_t passes, kt_ctr *t) { return cov_pass(pass, passes, t); });
    std::string e = ctr_->count();
    if (e.empty()) e = ctr_->merge(true);  // the reference leaves kmers.counts behind as well
    return e;
}

std::string CovComputer::compute_coverages() {
    // the reference parses kmers.counts back into a HashMap (:82-92); the table is still in HBM here
    if (ctr_ && ctr_->passes() > 1) {
        // ... unless it took several passes: the rows were summed pass by pass (cov_pass); normalise, format, write
        OutFile out;
        if (std::string e = out.open(out_dir_ + "/kmers.vectors"); !e.empty()) return e;
        PhaseTimer pt("cov (rows summed over the passes)");
        AsyncWriter writer(out.stream(), pt);
        std::vector<std::string> pieces;
        const uint64_t bins = bin_count_, slab = bins >= 2048 ? 8192 : 1ull << 19, acc_reads = kept_.seen.reads;
        Work w;
        for (uint64_t r0 = 0; r0 < acc_reads; r0 += slab) {
            const uint64_t n = acc_reads - r0 < slab ? acc_reads - r0 : slab;
            w.b.clear();
            w.b.offsets.assign(n + 1, 0);  // (emit_matrix only needs the number of reads)
            w.resize_rows(n * bins);
            for (uint64_t r = 0; r < n; r++) {
                const uint32_t *row = acc_rows_.data() + (r0 + r) * bins;
                uint64_t total = 0;
                for (uint64_t i = 0; i < bins; i++) total += row[i];
                const double d = total > 1 ? (double)total : 1.0;   // coverage/src/lib.rs:180-182
                for (uint64_t i = 0; i < bins; i++) w.rows[r * bins + i] = norm_ ? (double)row[i] / d : (double)row[i];
            }
            emit_matrix(writer, w, bins, norm_, delim_, threads_, pieces, pt);
        }
        return "";
    }
    if (ctr_ && ctr_->n_shards() > 0) {
        // --devices N: the table is N shards on N GPUs, each holding the k-mers whose minimiser it owns.  Every
        // batch of reads goes past every shard - one thread per shard, each adding raw bin counts to rows of its own
        // (kt_cov_batch_part: a k-mer a shard does not hold may be on another) -, the shards' rows are summed, normalised with one
        // division per cell and written: every k-mer of every read has been binned exactly once (the reference looks the
        // k-mers up in one map, coverage/src/lib.rs:165-184; its CountComputer built that map out of partitions the same way)
        const size_t N = ctr_->n_shards();
        SeqReader reader;
        if (!reader.open(in_path_, false)) return reader.error();
        OutFile out;
        if (std::string e = out.open(out_dir_ + "/kmers.vectors"); !e.empty()) return e;
        PhaseTimer pt("cov (rows summed over the shards)");
        AsyncWriter writer(out.stream(), pt);
        std::vector<std::string> pieces;
        const uint64_t bins = bin_count_;
        std::vector<std::vector<uint32_t>> part(N);
        std::vector<std::string> errs(N);
        Work w;
        std::string err;
        for (;;) {
            // (a batch holds N shards' u32 rows, the library's temporary of one shard's rows and the f64 rows: its reads are
            // bounded so that all of it stays under 1 GiB whatever the number of shards and bins - ADVICE r5)
            const uint64_t by_memory = std::max<uint64_t>(1024, (1ull << 30) / (bins * (4 * (uint64_t)N + 12)));
            const bool more = reader.next_batch(w.b, cli_batch_bases(256ull << 20),
                                                std::min<uint64_t>(cli_batch_reads(bins >= 2048 ? 8192 : 1ull << 19), by_memory));
            const uint64_t n = w.b.n_reads();
            if (n) {
                std::vector<std::thread> th;
                for (size_t r = 0; r < N; r++)
                    th.emplace_back([&, r] {
                        part[r].assign((size_t)(n * bins), 0u);
                        kt_ctr *t = ctr_->shard_table(r);
                        if (!t || kt_cov_batch_part(t, bases_ptr(w.b), w.b.offsets.data(), n, bin_size_, bin_count_, part[r].data(),
                                                    KT_MEM_HOST, 1, 0) != KT_OK)
                            errs[r] = t ? kt_last_error() : "cov: a shard's table is gone";
                    });
                for (auto &t : th) t.join();
                for (const auto &e : errs)
                    if (!e.empty() && err.empty()) err = e;
                if (!err.empty()) break;
                w.resize_rows(n * bins);
                for (uint64_t r = 0; r < n; r++) {
                    uint64_t total = 0;
                    for (uint64_t i = 0; i < bins; i++) {
                        uint32_t c = 0;  // (modulo 2^32: a shard's own cells mean nothing before they are summed - kt_cov_batch_part)
                        for (size_t sh = 0; sh < N; sh++) c += part[sh][r * bins + i];
                        w.rows[r * bins + i] = (double)c;
                        total += c;
                    }
                    if (norm_) {
                        const double d = total > 1 ? (double)total : 1.0;  // coverage/src/lib.rs:180-182
                        for (uint64_t i = 0; i < bins; i++) w.rows[r * bins + i] /= d;
                    }
                }
                emit_matrix(writer, w, bins, norm_, delim_, threads_, pieces, pt);
            }
            if (!more) break;
        }
        if (err.empty() && reader.failed()) err = reader.error();
        return err;
    }
    if (!ctr_ || !ctr_->table()) return "build_table() has not run";
    SeqReader reader;
    if (!reader.open(in_path_, false)) return reader.error();
    OutFile out;
    if (std::string e = out.open(out_dir_ + "/kmers.vectors"); !e.empty()) return e;
    std::vector<std::string> pieces;
    const uint64_t bins = bin_count_;
    PhaseTimer pt("cov");
    AsyncWriter writer(out.stream(), pt);
    return run_pipeline(
        reader, batch_bases(256ull << 20), bins >= 2048 ? 8192 : 1ull << 19, pt,
        [&](Work &w) -> std::string {
            const uint64_t n = w.b.n_reads();
            w.resize_rows(n * bins);
            w.pin_rows(ctr_->context());
            if (kt_cov_batch(ctr_->table(), bases_ptr(w.b), w.b.offsets.data(), n, bin_size_, bin_count_, norm_, KT_F64,
                             w.rows.data(), KT_MEM_HOST) != KT_OK)
                return kt_last_error();
            return "";
        },
        [&](Work &w) { emit_matrix(writer, w, bins, norm_, delim_, threads_, pieces, pt); });  // :112-124
}

// ---------------------------------------------------------------------------------------------
FilterComputer::FilterComputer(std::string in_path, std::string out_path, int ksize)
    : in_path_(in_path), in_path_kmer_(std::move(in_path)), out_path_(std::move(out_path)), ksize_(ksize) {}

FilterComputer::~FilterComputer() { delete ctr_; }

static constexpr uint32_t NO_WEAK = 0xFFFFFFFFu;  // first_weak of a read without a weak k-mer

// one pass of an out-of-core table is complete: every read's numbers for the k-mers of this hash partition
std::string FilterComputer::filter_pass(uint32_t pass, uint32_t passes, kt_ctr *table) {
    SeqReader reader;
    if (!reader.open(in_path_, false)) return reader.error();
    Batch batch;
    Cursor end;
    const std::string e = walk(reader, batch, TABLE_BATCH_BASES, 1ull << 20, false, nullptr, nullptr, &end,
                               [&](const Batch &b, const Cursor &at) -> std::string {
        const uint64_t n = b.n_reads(), to = at.reads + n;
        std::string c = kept_.claim(pass == 0, acc_n_, to, 0u);
        if (c.empty()) c = kept_.claim(pass == 0, acc_s_, to, 0u);
        if (c.empty() && trim_) c = kept_.claim(pass == 0, acc_w_, to, NO_WEAK);
        if (!c.empty()) return c;
        if (kt_ctr_read_solidity(table, bases_ptr(b), b.offsets.data(), n, min_count_, max_count_, acc_n_.data() + at.reads,
                                 acc_s_.data() + at.reads, trim_ ? acc_w_.data() + at.reads : nullptr, KT_MEM_HOST, passes, pass) != KT_OK)
            return kt_last_error();
        return "";
    });
    return e.empty() ? kept_.finish(pass == 0, end) : e;
}

void FilterComputer::emit(const Batch &b, const uint32_t *n, const uint32_t *s, const uint32_t *w, bool fastq, std::string &out) const {
    const uint64_t k = (uint64_t)ksize_;
    for (uint64_t i = 0; i < b.n_reads(); i++) {
        if (n[i] == 0) continue;  // no k-mer: dropped in either mode
        const uint64_t o = b.offsets[i];
        uint64_t keep = b.offsets[i + 1] - o;
        if (trim_) {
            if (w[i] != NO_WEAK) keep = (uint64_t)w[i] + k - 1;  // up to the base before the first weak k-mer's last
            if (keep < k) continue;
        } else if (!((double)s[i] >= min_solid_ * (double)n[i])) {
            continue;
        }
        append_record(out, fastq, b.headers[i], b.bases.data() + o, fastq ? b.quals.data() + o : nullptr, keep);
    }
}

// the table a read-level command looks its k-mers up in: counted as by `ctr`, no kmers.histo and no kmers.counts, `hook`
// for every complete pass of an out-of-core count
static CountComputer *make_lookup_counter(const std::string &in, bool in_is_table, int k, int threads, double memory_ceil_gb, int device,
                                          std::function<std::string(uint32_t, uint32_t, kt_ctr *)> hook) {
    CountComputer *c = new CountComputer(in, ".", k);
    c->set_threads(threads);
    c->set_max_memory(memory_ceil_gb);
    c->set_device(device);
    c->set_histo(0, true);
    c->set_input_is_table(in_is_table);
    c->set_pass_hook(std::move(hook));
    return c;
}

std::string FilterComputer::filter() {
    delete ctr_;
    acc_n_.clear();
    acc_s_.clear();
    acc_w_.clear();
    kept_.seen = Cursor();
    ctr_ = make_lookup_counter(in_path_kmer_, kmer_is_table_, ksize_, threads_, memory_ceil_gb_, device_,
                               [this](uint32_t pass, uint32_t passes, kt_ctr *t) { return filter_pass(pass, passes, t); });
    if (std::string e = ctr_->count(); !e.empty()) return e;
    const bool resident = ctr_->passes() == 1;  // else: the numbers were combined pass by pass (filter_pass)
    if (resident && !ctr_->table()) return "filter: no table";
    const bool fastq = format_from_path(in_path_) == SeqFormat::Fastq;
    SeqReader reader;
    if (!reader.open(in_path_, false)) return reader.error();
    OutFile out;
    if (std::string e = out.open(out_path_); !e.empty()) return e;
    PhaseTimer pt("filter");
    Lap lap;
    Batch batch;
    std::string text;
    std::vector<uint32_t> nk, ns, fw;
    Cursor end;
    std::string err = walk(reader, batch, TABLE_BATCH_BASES, 1ull << 20, true, &pt, &lap, &end, [&](const Batch &b, const Cursor &at) -> std::string {
        const uint64_t n = b.n_reads();
        const uint32_t *pn, *ps, *pw;
        if (resident) {
            nk.assign(n, 0u);
            ns.assign(n, 0u);
            fw.assign(trim_ ? n : 0, NO_WEAK);
            if (kt_ctr_read_solidity(ctr_->table(), bases_ptr(b), b.offsets.data(), n, min_count_, max_count_, nk.data(), ns.data(),
                                     trim_ ? fw.data() : nullptr, KT_MEM_HOST, 1, 0) != KT_OK)
                return kt_last_error();
            pn = nk.data(), ps = ns.data(), pw = fw.data();
        } else {
            if (std::string c = kept_.inside(at, b); !c.empty()) return c;
            pn = acc_n_.data() + at.reads, ps = acc_s_.data() + at.reads, pw = trim_ ? acc_w_.data() + at.reads : nullptr;
        }
        pt.t[1] += lap();
        text.clear();
        emit(b, pn, ps, pw, fastq, text);
        pt.t[2] += lap();
        if (!out.write(text)) return out.close();
        pt.t[3] += lap();
        return "";
    });
    if (err.empty() && !resident) err = kept_.finish(false, end);
    if (std::string e = out.close(); err.empty()) err = e;
    return err;
}

// ---------------------------------------------------------------------------------------------
ProfileComputer::ProfileComputer(std::string in_path, std::string out_dir, int ksize)
    : in_path_(in_path), in_path_kmer_(std::move(in_path)), out_dir_(std::move(out_dir)), ksize_(ksize) {}

ProfileComputer::~ProfileComputer() { delete ctr_; }

// one pass of an out-of-core table is complete: the positions whose k-mers belong to this hash partition
std::string ProfileComputer::profile_pass(uint32_t pass, uint32_t passes, kt_ctr *table) {
    SeqReader reader;
    if (!reader.open(in_path_, false)) return reader.error();
    Batch batch;
    Cursor end;
    const std::string e = walk(reader, batch, TABLE_BATCH_BASES, 1ull << 20, false, nullptr, nullptr, &end,
                               [&](const Batch &b, const Cursor &at) -> std::string {
        const uint64_t n = b.n_reads(), total = b.offsets[n];
        if (pass == 0)
            if (std::string c = kept_.over_ceiling(at.bases + total, 4, "per-base counts", passes, memory_ceil_gb_); !c.empty()) return c;
        if (std::string c = kept_.claim(pass == 0, acc_, at.bases + total, (uint32_t)KT_NO_KMER); !c.empty()) return c;
        if (total && kt_ctr_profile(table, bases_ptr(b), b.offsets.data(), n, acc_.data() + at.bases, KT_MEM_HOST, passes, pass) != KT_OK)
            return kt_last_error();
        return "";
    });
    return e.empty() ? kept_.finish(pass == 0, end) : e;
}

// a record's name: its header up to the first white space
static void append_name(std::string &out, const std::string &header) {
    size_t e = 0;
    while (e < header.size() && !isspace((unsigned char)header[e])) e++;
    out.append(header, 0, e);
}

std::string ProfileComputer::profile() {
    delete ctr_;
    acc_.clear();
    acc_.shrink_to_fit();
    kept_.seen = Cursor();
    ctr_ = make_lookup_counter(in_path_kmer_, kmer_is_table_, ksize_, threads_, memory_ceil_gb_, device_,
                               [this](uint32_t pass, uint32_t passes, kt_ctr *t) { return profile_pass(pass, passes, t); });
    if (std::string e = ctr_->count(); !e.empty()) return e;
    const bool resident = ctr_->passes() == 1;  // else: the positions were filled pass by pass (profile_pass)
    if (resident && !ctr_->table()) return "profile: no table";
    kt_ctx *ctx = ctr_->context();
    if (!ctx) return "profile: no device context";
    SeqReader reader;
    if (!reader.open(in_path_, false)) return reader.error();
    OutFile fs, fc;  // profile.stats, and with positions_ profile.counts
    if (std::string e = fs.open(out_dir_ + "/profile.stats"); !e.empty()) return e;
    if (std::string e = positions_ ? fc.open(out_dir_ + "/profile.counts") : ""; !e.empty()) return e;
    PhaseTimer pt("profile");
    Lap lap;
    Batch batch;
    std::string text = "#name\tlength\tkmers\tpresent\tmin\tmedian\tmean\tmax\n";
    std::vector<std::string> pieces;
    std::vector<uint32_t> prof, st;
    std::vector<uint64_t> sum;
    Cursor end;
    bool in_batch = false;  // stays set when a batch ends with an error
    std::string err = walk(reader, batch, TABLE_BATCH_BASES, 1ull << 20, true, &pt, &lap, &end, [&](const Batch &b, const Cursor &at) -> std::string {
        in_batch = true;
        const uint64_t n = b.n_reads(), total = b.offsets[n];
        const uint32_t *p;
        if (resident) {
            prof.assign(total, KT_NO_KMER);
            if (total && kt_ctr_profile(ctr_->table(), bases_ptr(b), b.offsets.data(), n, prof.data(), KT_MEM_HOST, 1, 0) != KT_OK)
                return kt_last_error();
            p = prof.data();
        } else {
            if (std::string c = kept_.inside(at, b); !c.empty()) return c;
            p = acc_.data() + at.bases;
        }
        st.resize(n * 5);
        sum.resize(n);
        uint32_t *nk = st.data(), *np = nk + n, *mn = np + n, *md = mn + n, *mx = md + n;
        if (kt_profile_stats(ctx, p, b.offsets.data(), n, nk, np, mn, md, mx, sum.data(), KT_MEM_HOST) != KT_OK) return kt_last_error();
        pt.t[1] += lap();
        for (uint64_t i = 0; i < n; i++) {
            append_name(text, b.headers[i]);
            append_tab_uints(text, {b.offsets[i + 1] - b.offsets[i], nk[i], np[i], mn[i], md[i]});
            text += '\t';
            append_fixed6(text, (double)sum[i] / (double)(nk[i] ? nk[i] : 1u));
            append_tab_uints(text, {mx[i]});
            text += '\n';
        }
        if (fc.is_open())
            format_rows(n, threads_, 512, pieces, [&](uint64_t i, std::string &s) {
                s += '>';
                append_name(s, b.headers[i]);
                s += '\n';
                for (uint64_t g = b.offsets[i]; g < b.offsets[i + 1]; g++) {
                    if (g != b.offsets[i]) s += ' ';
                    if (p[g] == KT_NO_KMER) s += "-1";
                    else append_uint(s, p[g]);
                }
                s += '\n';
            });
        pt.t[2] += lap();
        const bool ok = fs.write(text) && (!fc.is_open() || fc.write(pieces));
        text.clear();
        if (!ok) return "Unable to write to directory: " + out_dir_;
        pt.t[3] += lap();
        in_batch = false;
        return "";
    });
    // (an input without records - or none before the reader failed: the header line)
    if (!in_batch && !text.empty() && !fs.write(text) && err.empty()) err = fs.error();
    if (err.empty() && !resident) err = kept_.finish(false, end);
    if (std::string e = fs.close(); err.empty()) err = e;
    if (std::string e = fc.close(); err.empty()) err = e;
    return err;
}

// ---------------------------------------------------------------------------------------------
CorrectComputer::CorrectComputer(std::string in_path, std::string out_path, int ksize)
    : in_path_(in_path), in_path_kmer_(std::move(in_path)), out_path_(std::move(out_path)), ksize_(ksize) {}

CorrectComputer::~CorrectComputer() { delete ctr_; }

// one pass of an out-of-core table is complete.  First pass loop (support = false): the positions whose k-mers belong to this
// hash partition (the profile).  Second (support = true): the supports whose substituted k-mers do, against the complete profile.
std::string CorrectComputer::table_pass(bool support, uint32_t pass, uint32_t passes, kt_ctr *table) {
    SeqReader reader;
    if (!reader.open(in_path_, false)) return reader.error();
    const bool first = !support && pass == 0;
    Batch batch;
    Cursor end;
    const std::string e = walk(reader, batch, TABLE_BATCH_BASES, 1ull << 20, false, nullptr, nullptr, &end,
                               [&](const Batch &b, const Cursor &at) -> std::string {
        const uint64_t n = b.n_reads(), total = b.offsets[n];
        if (first)
            if (std::string c = kept_.over_ceiling(at.bases + total, 8, "per-base counts and supports", passes, memory_ceil_gb_); !c.empty())
                return c;
        if (std::string c = kept_.claim(first, acc_prof_, at.bases + total, (uint32_t)KT_NO_KMER); !c.empty()) return c;
        if (total) {
            uint32_t *prof = acc_prof_.data() + at.bases;
            const int rc = support ? kt_ctr_correct_support(table, bases_ptr(b), b.offsets.data(), n, prof, min_count_, max_count_,
                                                            acc_sup_.data() + at.bases, KT_MEM_HOST, passes, pass)
                                   : kt_ctr_profile(table, bases_ptr(b), b.offsets.data(), n, prof, KT_MEM_HOST, passes, pass);
            if (rc != KT_OK) return kt_last_error();
        }
        return "";
    });
    return e.empty() ? kept_.finish(first, end) : e;
}

CountComputer *CorrectComputer::new_counter(bool support) {
    return make_lookup_counter(in_path_kmer_, kmer_is_table_, ksize_, threads_, memory_ceil_gb_, device_, [this, support](uint32_t pass, uint32_t passes, kt_ctr *t) {
        return table_pass(support, pass, passes, t);
    });
}

std::string CorrectComputer::correct() {
    delete ctr_;
    ctr_ = nullptr;
    acc_prof_.clear();
    acc_prof_.shrink_to_fit();
    acc_sup_.clear();
    acc_sup_.shrink_to_fit();
    kept_.seen = Cursor();
    ctr_ = new_counter(false);
    if (std::string e = ctr_->count(); !e.empty()) return e;
    const bool resident = ctr_->passes() == 1;
    if (resident && !ctr_->table()) return "correct: no table";
    if (!resident) {  // the profile is complete: the tables once more, for the supports
        delete ctr_;
        ctr_ = nullptr;
        acc_sup_.assign(acc_prof_.size(), 0u);
        ctr_ = new_counter(true);
        if (std::string e = ctr_->count(); !e.empty()) return e;
        if (ctr_->passes() == 1) return "correct: the table fitted the second time only";
    }
    kt_ctx *ctx = ctr_->context();
    if (!ctx) return "correct: no device context";
    const bool fastq = format_from_path(in_path_) == SeqFormat::Fastq;
    SeqReader reader;
    if (!reader.open(in_path_, false)) return reader.error();
    OutFile out;
    if (std::string e = out.open(out_path_); !e.empty()) return e;
    PhaseTimer pt("correct");
    Lap lap;
    Batch batch;
    std::string text;
    std::vector<uint32_t> prof, sup, ns, na;
    std::vector<uint8_t> fixed;
    Cursor end;
    uint64_t reads_corrected = 0, bases_corrected = 0, ambiguous = 0, over_limit = 0;
    std::string err = walk(reader, batch, TABLE_BATCH_BASES, 1ull << 20, true, &pt, &lap, &end, [&](const Batch &b, const Cursor &at) -> std::string {
        const uint64_t n = b.n_reads(), total = b.offsets[n];
        const uint32_t *s;
        if (resident) {
            prof.assign(total, KT_NO_KMER);
            sup.assign(total, 0u);
            if (total && (kt_ctr_profile(ctr_->table(), bases_ptr(b), b.offsets.data(), n, prof.data(), KT_MEM_HOST, 1, 0) != KT_OK ||
                          kt_ctr_correct_support(ctr_->table(), bases_ptr(b), b.offsets.data(), n, prof.data(), min_count_, max_count_,
                                                 sup.data(), KT_MEM_HOST, 1, 0) != KT_OK))
                return kt_last_error();
            s = sup.data();
        } else {
            if (std::string c = kept_.inside(at, b); !c.empty()) return c;
            s = acc_sup_.data() + at.bases;
        }
        fixed.resize(total);
        ns.resize(n);
        na.resize(n);
        if (kt_correct_apply(ctx, bases_ptr(b), b.offsets.data(), n, s, min_support_, max_corrections_, fixed.data(), ns.data(), na.data(),
                             KT_MEM_HOST) != KT_OK)
            return kt_last_error();
        pt.t[1] += lap();
        text.clear();
        for (uint64_t i = 0; i < n; i++) {
            const uint64_t o = b.offsets[i], len = b.offsets[i + 1] - o;
            ambiguous += na[i];
            if (max_corrections_ && ns[i] > max_corrections_) over_limit++;
            else if (ns[i]) reads_corrected++, bases_corrected += ns[i];
            append_record(text, fastq, b.headers[i], fixed.data() + o, fastq ? b.quals.data() + o : nullptr, len);
        }
        pt.t[2] += lap();
        if (!out.write(text)) return out.close();
        pt.t[3] += lap();
        return "";
    });
    if (err.empty() && !resident) err = kept_.finish(false, end);
    if (std::string e = out.close(); err.empty()) err = e;
    if (err.empty() && !stats_path_.empty()) {
        static const char *names[6] = {"reads", "bases", "reads_corrected", "bases_corrected", "positions_ambiguous", "reads_over_limit"};
        const uint64_t values[6] = {end.reads, end.bases, reads_corrected, bases_corrected, ambiguous, over_limit};
        err = write_stats_file(stats_path_, names, values, 6);
    }
    return err;
}

// ---------------------------------------------------------------------------------------------
CompareComputer::CompareComputer(std::string in_a, std::string in_b, std::string out_dir, int ksize)
    : in_a_(std::move(in_a)), in_b_(std::move(in_b)), out_dir_(std::move(out_dir)), ksize_(ksize) {}

CompareComputer::~CompareComputer() { release(); }

void CompareComputer::release() {
    if (ta_) kt_ctr_destroy(ta_);
    if (tb_) kt_ctr_destroy(tb_);
    ta_ = tb_ = nullptr;
}

std::string CompareComputer::write(const std::vector<uint64_t> &m, const uint64_t *tot) const {
    if (std::string e = write_text_file(out_dir_ + "/compare.matrix", matrix_text(m, max_a_ + 1, max_b_ + 1)); !e.empty()) return e;
    // distinct_a, distinct_b, shared, occurrences_a, occurrences_b, shared_min; then the ratios (0 over a zero denominator)
    static const char *names[6] = {"distinct_a", "distinct_b", "shared", "occurrences_a", "occurrences_b", "shared_min"};
    std::string s;
    append_stats_rows(s, names, tot, 6);
    auto ratio = [&](const char *name, uint64_t num, uint64_t den) {
        char b[FIXED6_BUF + 64];
        snprintf(b, sizeof b, "%s\t%.6f\n", name, den ? (double)num / (double)den : 0.0);
        s += b;
    };
    const uint64_t da = tot[0], db = tot[1], sh = tot[2], oa = tot[3], ob = tot[4], smin = tot[5];
    ratio("jaccard", sh, da + db - sh);
    ratio("containment_a", sh, da);
    ratio("containment_b", sh, db);
    ratio("weighted_jaccard", smin, oa + ob - smin);
    return write_text_file(out_dir_ + "/compare.stats", s);
}

// What `compare` and `setop` share: both tables of a pass on one device, `bytes_per_slot` of HBM for every slot of either
// (16: the slot itself), pass p holding hash partition p of both.  Creates the tables; on an error none is left.
// A side that is a table file (a_is_table / b_is_table: the path is the file's) is sized from the file's headers and must be
// loaded whole: with such a side a plan of several passes is refused.
static std::string two_tables_setup(Device &dev, const std::string &in_a, bool a_is_table, const std::string &in_b, bool b_is_table, int k,
                                    uint64_t bytes_per_slot, const char *what, uint32_t *passes, kt_ctr **ta, kt_ctr **tb) {
    Lap setup;
    InputBound a, b;
    uint64_t file_entries = 0;
    for (auto [path, is_table, in] : {std::make_tuple(&in_a, a_is_table, &a), std::make_tuple(&in_b, b_is_table, &b)}) {
        if (!is_table) {
            if (std::string e = slots_wanted(*path, k, in, dev); !e.empty()) return e;
            continue;
        }
        int fk = 0;
        uint64_t entries = 0;
        if (kt_table_file_info(path->c_str(), &fk, nullptr, &entries, nullptr) != KT_OK) return kt_last_error();
        if (fk != k) return "the table file " + *path + " holds k = " + std::to_string(fk) + ", not " + std::to_string(k);
        in->want = std::max<uint64_t>(1024, entries + entries / 10 * 9);
        file_entries += entries;
    }
    if (std::string e = dev.ensure(); !e.empty()) return e;
    TablePlan plan;
    plan.n = 2;
    plan.want[0] = a.want, plan.want[1] = b.want;
    plan.plan(dev.ctx, bytes_per_slot, false);
    if ((a_is_table || b_is_table) && plan.passes > 1)
        return std::string(what) + ": the table file does not fit the device in one pass beside the other table, and table files are not "
               "loaded in several passes (" + std::to_string(file_entries) + " entries in table files, " + std::to_string(a.want + b.want) +
               " slots wanted, room for " + std::to_string(plan.room) + ")";
    kt_ctr **const tables[2] = {ta, tb};
    if (std::string e = create_tables(dev.ctx, k, plan, tables); !e.empty()) return e;
    *passes = plan.passes;
    if (getenv("KT_CLI_TIMING")) {
        uint64_t sa = plan.capacity(0), sb = plan.capacity(1);
        (void)kt_ctr_capacity(*ta, &sa);
        (void)kt_ctr_capacity(*tb, &sb);
        fprintf(stderr, "[timing] %s setup: tables of %llu + %llu slots, %u pass(es) %.3f s\n", what, (unsigned long long)sa,
                (unsigned long long)sb, *passes, setup());
    }
    return "";
}

// pass `pass` of `passes`: both tables cleared (after the first pass) and filled with their inputs' hash partition
// (a side whose reader was not opened is a table file, file_a / file_b: loaded whole - the plan has one pass then)
static std::string two_tables_count(uint32_t pass, uint32_t passes, SeqReader &ra, SeqReader &rb, const std::string *file_a,
                                    const std::string *file_b, kt_ctr *ta, kt_ctr *tb, Batch &b, PhaseTimer &pt, Lap &lap) {
    if (pass && (kt_ctr_clear(ta) != KT_OK || kt_ctr_clear(tb) != KT_OK)) return kt_last_error();
    for (auto [reader, table, file] : {std::make_tuple(&ra, ta, file_a), std::make_tuple(&rb, tb, file_b)}) {
        if (file) {
            Lap load;
            uint64_t added = 0;
            if (kt_ctr_add_file(table, file->c_str(), &added) != KT_OK) return kt_last_error();
            if (getenv("KT_CLI_TIMING"))
                fprintf(stderr, "[timing] table file: %llu entries loaded %.3f s\n", (unsigned long long)added, load());
            continue;
        }
        if (pass && !reader->rewind()) return reader->error();
        kt_ctr *t = table;  // (a structured binding cannot be captured)
        if (std::string e = fill_table(*reader, b, pt, lap, [&](const Batch &bb) {
                return kt_ctr_add_reads_part(t, bb.bases.data(), bb.offsets.data(), bb.n_reads(), KT_MEM_HOST, passes, pass);
            });
            !e.empty())
            return e;
    }
    return "";
}

std::string CompareComputer::compare() {
    release();
    if (std::string e = two_tables_setup(dev_, in_a_, a_is_table_, in_b_, b_is_table_, ksize_, 16, "compare", &passes_, &ta_, &tb_); !e.empty()) return e;
    const uint32_t R = max_a_ + 1, C = max_b_ + 1;
    std::vector<uint64_t> m((size_t)R * C, 0);
    uint64_t tot[6] = {0, 0, 0, 0, 0, 0};
    PhaseTimer pt("compare");
    SeqReader ra, rb;
    if (!a_is_table_ && !ra.open(in_a_, false)) return ra.error();
    if (!b_is_table_ && !rb.open(in_b_, false)) return rb.error();
    Batch b;
    for (uint32_t pass = 0; pass < passes_; pass++) {
        Lap lap;
        if (std::string e = two_tables_count(pass, passes_, ra, rb, a_is_table_ ? &in_a_ : nullptr, b_is_table_ ? &in_b_ : nullptr, ta_, tb_, b, pt, lap); !e.empty()) return e;
        if (kt_ctr_compare(ta_, tb_, m.data(), R, C, tot, KT_MEM_HOST) != KT_OK) return kt_last_error();
        pt.t[1] += lap();
    }
    Lap lap;
    std::string e = write(m, tot);
    pt.t[3] += lap();
    return e;
}

// ---------------------------------------------------------------------------------------------
SetopComputer::SetopComputer(std::string in_a, std::string in_b, std::string out_dir, int ksize)
    : in_a_(std::move(in_a)), in_b_(std::move(in_b)), out_dir_(std::move(out_dir)), ksize_(ksize) {}

SetopComputer::~SetopComputer() { release(); }

void SetopComputer::release() {
    if (ta_) kt_ctr_destroy(ta_);
    if (tb_) kt_ctr_destroy(tb_);
    ta_ = tb_ = nullptr;
}

std::string SetopComputer::setop() {
    release();
    // HBM per slot: the slot (16) + its share of the result and of the sort's second pair - at most every entry of both
    // tables, 12 bytes, twice, with 1.9 slots per entry: 24 / 1.9 < 13
    if (std::string e = two_tables_setup(dev_, in_a_, a_is_table_, in_b_, b_is_table_, ksize_, 16 + 13, "setop", &passes_, &ta_, &tb_); !e.empty()) return e;
    OutFile out;
    if (std::string e = out.open(out_dir_ + "/kmers.counts"); !e.empty()) return e;
    // distinct_a, distinct_b, in_a, in_b, emitted, emitted_occurrences
    uint64_t tot[6] = {0, 0, 0, 0, 0, 0};
    TableWriter writer(acgt_, ksize_, threads_, memory_ceil_gb_);
    std::vector<uint64_t> keys;
    std::vector<uint32_t> counts;
    PhaseTimer pt("setop");
    SeqReader ra, rb;
    if (!a_is_table_ && !ra.open(in_a_, false)) return ra.error();
    if (!b_is_table_ && !rb.open(in_b_, false)) return rb.error();
    Batch b;
    const bool plain_a = min_a_ == 1 && max_a_ == 0xFFFFFFFFu, plain_b = min_b_ == 1 && max_b_ == 0xFFFFFFFFu;
    for (uint32_t pass = 0; pass < passes_; pass++) {
        Lap lap;
        if (std::string e = two_tables_count(pass, passes_, ra, rb, a_is_table_ ? &in_a_ : nullptr, b_is_table_ ? &in_b_ : nullptr, ta_, tb_, b, pt, lap); !e.empty()) return e;
        uint64_t n_a = 0, n_b = 0, in_a = 0, in_b = 0, n = 0;
        if (kt_ctr_size(ta_, &n_a) != KT_OK || kt_ctr_size(tb_, &n_b) != KT_OK) return kt_last_error();
        // what can qualify at most sizes the host arrays: one call, no counting call before it
        const uint64_t bound = op_ == KT_SET_INTERSECT ? std::min(n_a, n_b) : op_ == KT_SET_SUBTRACT ? n_a : n_a + n_b;
        if (keys.size() < bound) {
            keys.resize((size_t)bound);
            counts.resize((size_t)bound);
        }
        if (bound && kt_ctr_setop(ta_, tb_, op_, rule_, min_a_, max_a_, min_b_, max_b_, keys.data(), counts.data(), bound, &n,
                                  KT_MEM_HOST, 1) != KT_OK)
            return kt_last_error();
        // the members of each side under its range: the table's size, or (a range given) the table intersected with itself
        in_a = n_a, in_b = n_b;
        if (!plain_a && n_a &&
            kt_ctr_setop(ta_, ta_, KT_SET_INTERSECT, KT_SETCNT_FIRST, min_a_, max_a_, min_a_, max_a_, nullptr, nullptr, 0, &in_a,
                         KT_MEM_HOST, 0) != KT_OK)
            return kt_last_error();
        if (!plain_b && n_b &&
            kt_ctr_setop(tb_, tb_, KT_SET_INTERSECT, KT_SETCNT_FIRST, min_b_, max_b_, min_b_, max_b_, nullptr, nullptr, 0, &in_b,
                         KT_MEM_HOST, 0) != KT_OK)
            return kt_last_error();
        pt.t[1] += lap();
        uint64_t occ = 0;
        for (uint64_t i = 0; i < n; i++) occ += counts[i];
        tot[0] += n_a, tot[1] += n_b, tot[2] += in_a, tot[3] += in_b, tot[4] += n, tot[5] += occ;
        if (std::string e = writer.write_pairs(out, keys.data(), counts.data(), n); !e.empty()) return e;
        pt.t[3] += lap();
    }
    if (std::string e = out.close(); !e.empty()) return e;
    static const char *names[6] = {"distinct_a", "distinct_b", "in_a", "in_b", "emitted", "emitted_occurrences"};
    return write_stats_file(out_dir_ + "/setop.stats", names, tot, 6);
}

// ---------------------------------------------------------------------------------------------
GraphComputer::GraphComputer(std::string in_path, std::string out_dir, int ksize)
    : in_path_(std::move(in_path)), out_dir_(std::move(out_dir)), ksize_(ksize) {}

GraphComputer::~GraphComputer() {
    if (table_) kt_ctr_destroy(table_);
}

// the census names, in kt_ctr_graph's order
static std::string graph_census_name(int j) {
    static const char *sums[7] = {"nodes", "occurrences", "degree_sum", "end_sides", "isolated", "tips", "branching"};
    if (j < 7) return sums[j];
    return "degree_" + std::to_string((j - 7) / 5) + "_" + std::to_string((j - 7) % 5);
}

// What `graph`, `hetmers` and `unitigs` share: one table, and the whole of it on the device - a plan of several passes is
// refused before anything is counted or written.  whole_table plans and creates it (`name`: the command, in the texts), or
// with a table file loads the file instead (table_from_file).
static std::string whole_text(const char *name) {
    return std::string(name) +
                              " needs the whole table on the device: a k-mer's neighbours live in other hash partitions, so the "
                              "table cannot be counted in several passes as the other commands count theirs.  --min-count is no "
                              "remedy (every k-mer is counted before the weak ones are left out): use a device with more free "
                              "memory or a smaller input - or, for --min-count 2 and above, --prefilter, which keeps the k-mers seen "
                              "once out of the table";
}
// a table of `want` slots, all of it on the device, or why there is none
static std::string create_whole(Device &dev, int k, uint64_t bytes_per_slot, const char *name, uint64_t want, kt_ctr **table) {
    TablePlan plan;
    plan.want[0] = want;
    plan.plan(dev.ctx, bytes_per_slot, false);
    const std::string whole = whole_text(name);
    if (plan.passes > 1) return whole + " (" + std::to_string(want) + " slots wanted, room for " + std::to_string(plan.room) + ")";
    if (const int rc = kt_ctr_create(dev.ctx, k, want, table); rc != KT_OK)
        return rc == KT_ERR_NOMEM ? whole + " (" + kt_last_error() + ")" : std::string(kt_last_error());
    return "";
}
static std::string whole_table(Device &dev, const std::string &path, const std::string &table_file, int k, uint64_t bytes_per_slot,
                               const char *name, kt_ctr **table) {
    if (!table_file.empty()) return table_from_file(dev, table_file, k, bytes_per_slot, name, table);
    Lap setup;
    InputBound in;
    if (std::string e = slots_wanted(path, k, &in, dev); !e.empty()) return e;
    if (std::string e = dev.ensure(); !e.empty()) return e;
    if (std::string e = create_whole(dev, k, bytes_per_slot, name, in.want, table); !e.empty()) return e;
    if (getenv("KT_CLI_TIMING")) {
        uint64_t slots = in.want;
        (void)kt_ctr_capacity(*table, &slots);
        fprintf(stderr, "[timing] %s setup: table of %llu slots %.3f s\n", name, (unsigned long long)slots, setup());
    }
    return "";
}
// How those commands begin: the table of the last run destroyed, the new one made by whole_table and, unless a file was
// loaded, the input counted into it.  A command constructs one of these first and keeps it until it returns: the reader and
// the batch are members, alive until the command is done, as the table's other users keep theirs; the phase timer exists
// only once whole_table has succeeded, so a refusal prints no phase line.
struct WholeTableRun {
    std::optional<PhaseTimer> timer;
    SeqReader reader;
    Batch b;
    Lap lap;
    std::string err;  // "" or why there is no table
    void took(int phase) { timer->t[phase] += lap(); }  // the time since the last call, booked to that phase
    // --prefilter: pass 1 over the input, the table planned from what it promoted - where a plan of one pass may now exist
    // that the input's bound did not allow -, pass 2 into it; a table that overflows (the plan is an estimate) is made again
    // with twice the slots, while that still fits the device, and pass 2 repeated.  Writes prefilter.stats.
    std::string prefiltered(Device &dev, const std::string &in_path, int k, uint64_t bytes_per_slot, const char *name, kt_ctr **table) {
        if (std::string e = Prefiltered::check(in_path, k); !e.empty()) return e;
        InputBound in;
        if (std::string e = slots_wanted(in_path, k, &in, dev); !e.empty()) return e;
        if (std::string e = dev.ensure(); !e.empty()) return e;
        if (!reader.open(in_path, false)) return reader.error();
        timer.emplace(name);
        lap = Lap();
        Prefiltered pf;
        if (std::string e = pf.pass1(dev, k, in, reader, b, *timer, lap); !e.empty()) return e;
        for (uint64_t want = pf.table_slots();; want *= 2, pf.st.table_retries++) {
            if (std::string e = create_whole(dev, k, bytes_per_slot, name, want, table); !e.empty()) return e;
            if (!reader.rewind()) return reader.error();
            if (std::string e = fill_table(reader, b, *timer, lap, [&](const Batch &bb) { return pf.add(*table, bb, 1, 0); }); !e.empty())
                return e;
            const int rc = kt_ctr_size(*table, &pf.st.table_keys);
            if (rc == KT_OK) break;
            if (rc != KT_ERR_FULL) return kt_last_error();
            kt_ctr_destroy(*table);
            *table = nullptr;
        }
        (void)kt_ctr_capacity(*table, &pf.st.table_slots);
        pf.done();
        return pf.write_stats();
    }
    WholeTableRun(Device &dev, const std::string &in_path, const std::string &table_file, int k, uint64_t bytes_per_slot, const char *name,
                  kt_ctr **table) {
        if (*table) kt_ctr_destroy(*table);
        *table = nullptr;
        if (g_prefilter.on && table_file.empty()) {
            err = prefiltered(dev, in_path, k, bytes_per_slot, name, table);
            return;
        }
        err = whole_table(dev, in_path, table_file, k, bytes_per_slot, name, table);
        if (!err.empty()) return;
        timer.emplace(name);
        lap = Lap();
        if (!table_file.empty()) return;  // (there is nothing to count)
        if (!reader.open(in_path, false)) err = reader.error();
        else err = fill_table(reader, b, *timer, lap, [&](const Batch &bb) {
            return kt_ctr_add_reads(*table, bb.bases.data(), bb.offsets.data(), bb.n_reads(), KT_MEM_HOST);
        });
    }
};

std::string GraphComputer::graph() {
    // HBM per slot: the slot (16) + its share of the result (key, info, count: 16 bytes a node) and of the sort's second
    // pair (12), with 1.9 slots per entry: 28 / 1.9 < 15
    WholeTableRun run(dev_, in_path_, table_file_, ksize_, 16 + 15, "graph", &table_);
    if (!run.err.empty()) return run.err;
    // what can be a node at most sizes the host arrays: one call, no counting call before it
    uint64_t bound = 0, n = 0, census[KT_GRAPH_CENSUS] = {};
    if (kt_ctr_size(table_, &bound) != KT_OK) return kt_last_error();
    if (stats_only_) bound = 0;
    std::vector<uint64_t> keys((size_t)bound);
    std::vector<uint32_t> info((size_t)bound), counts((size_t)bound);
    if (kt_ctr_graph(table_, min_count_, max_count_, keys.data(), info.data(), counts.data(), bound, &n, census, KT_MEM_HOST, 1) != KT_OK)
        return kt_last_error();
    run.took(1);
    if (!stats_only_) {
        OutFile out;
        if (std::string e = out.open(out_dir_ + "/graph.nodes"); !e.empty()) return e;
        // ~64 bytes of text a node, a slab at a time (TableWriter's bound)
        uint64_t slab = (uint64_t)(memory_ceil_gb_ * (double)(1ull << 30) / 16.0 / 64.0);
        slab = std::min<uint64_t>(std::max<uint64_t>(slab, 1ull << 16), 1ull << 20);
        std::vector<std::string> pieces;
        write_rows(n, slab, threads_, pieces, RowText(out, (size_t)ksize_ + 26, [&](uint64_t i, std::string &s) {
            append_kmer(s, keys[i], ksize_, acgt_);
            append_tab_uints(s, {counts[i]});
            s += '\t';
            for (int x = 0; x < 4; x++) s += info[i] >> (4 + x) & 1u ? "ACGT"[x] : '.';
            s += '\t';
            for (int x = 0; x < 4; x++) s += info[i] >> x & 1u ? "ACGT"[x] : '.';
            s += '\t';
            s += info[i] & 0x200u ? 'L' : '.';
            s += info[i] & 0x100u ? 'R' : '.';
            s += '\n';
        }));
        if (std::string e = out.close(); !e.empty()) return e;
    }
    std::string s;
    for (int j = 0; j < KT_GRAPH_CENSUS; j++) s += graph_census_name(j) + '\t' + std::to_string(census[j]) + '\n';
    if (std::string e = write_text_file(out_dir_ + "/graph.stats", s); !e.empty()) return e;
    run.took(3);
    return "";
}

// ---------------------------------------------------------------------------------------------
HetmerComputer::HetmerComputer(std::string in_path, std::string out_dir, int ksize)
    : in_path_(std::move(in_path)), out_dir_(std::move(out_dir)), ksize_(ksize) {}

HetmerComputer::~HetmerComputer() {
    if (table_) kt_ctr_destroy(table_);
}

std::string HetmerComputer::hetmers() {
    // HBM per slot: the slot (16) + its share of the nodes and candidates (24 bytes an entry), and of the result and the sort
    // (at most one pair per two entries: 24 + 12 + 12 bytes a pair), with 1.9 slots per entry: 48 / 1.9 < 26
    WholeTableRun run(dev_, in_path_, table_file_, ksize_, 16 + 26, "hetmers", &table_);
    if (!run.err.empty()) return run.err;
    // every k-mer is in at most one pair: half the entries size the host arrays, one call, no counting call before it
    uint64_t bound = 0, n = 0, census[KT_HET_CENSUS] = {};
    if (kt_ctr_size(table_, &bound) != KT_OK) return kt_last_error();
    bound = stats_only_ ? 0 : bound / 2;
    const uint32_t R = max_minor_ + 1, C = max_major_ + 1;
    std::vector<uint64_t> ka((size_t)bound), kb((size_t)bound), m((size_t)R * C);
    std::vector<uint32_t> ca((size_t)bound), cb((size_t)bound);
    if (kt_ctr_hetmers(table_, min_count_, max_count_, middle_ ? KT_HET_MIDDLE : KT_HET_ALL, ka.data(), kb.data(), ca.data(), cb.data(),
                       bound, &n, m.data(), R, C, census, KT_MEM_HOST, 1) != KT_OK)
        return kt_last_error();
    run.took(1);
    if (!stats_only_) {
        OutFile outp, outc;
        if (std::string e = outp.open(out_dir_ + "/hetmers.pairs"); !e.empty()) return e;
        if (std::string e = outc.open(out_dir_ + "/hetmers.cov"); !e.empty()) return e;
        // B as written: the strand of b that differs from A at one allowed position, and that position.  Where both strands
        // do (double reach) it is b's forward strand, the lower position first.
        const uint32_t p_lo = middle_ ? (uint32_t)(ksize_ - 1) / 2u : 0u, p_hi = middle_ ? p_lo + 1u : (uint32_t)ksize_;
        auto one_sub = [&](uint64_t x, uint32_t *pos) {
            for (uint32_t i = p_lo; i < p_hi; i++)
                if ((x & ~(3ull << 2u * ((uint32_t)ksize_ - 1u - i))) == 0) {
                    *pos = i;
                    return true;
                }
            return false;
        };
        constexpr uint64_t slab = 1ull << 18;
        std::vector<std::string> pieces;
        write_rows(n, slab, threads_, pieces,
                   RowText(outp, 2 * (size_t)ksize_ + 30, [&](uint64_t i, std::string &s) {
                       uint64_t bw = kb[i];
                       uint32_t pos = 0;
                       if (!one_sub(ka[i] ^ bw, &pos)) {
                           bw = kt_rev_comp(kb[i], ksize_);
                           (void)one_sub(ka[i] ^ bw, &pos);
                       }
                       append_kmer(s, ka[i], ksize_, true);
                       s += '\t';
                       append_kmer(s, bw, ksize_, true);
                       append_tab_uints(s, {pos, ca[i], cb[i]});
                       s += '\n';
                   }),
                   RowText(outc, 24, [&](uint64_t i, std::string &s) {
                       append_uint(s, std::min(ca[i], cb[i]));
                       append_tab_uints(s, {std::max(ca[i], cb[i])});
                       s += '\n';
                   }));
        const std::string ep = outp.close(), ec = outc.close();
        if (!ep.empty() || !ec.empty()) return ep.empty() ? ec : ep;
    }
    if (std::string e = write_text_file(out_dir_ + "/hetmers.matrix", matrix_text(m, R, C)); !e.empty()) return e;
    static const char *names[KT_HET_CENSUS] = {"nodes", "occurrences", "degree_0", "degree_1", "degree_2_or_more", "pairs", "minor_sum", "major_sum"};
    std::string s = "k\t" + std::to_string(ksize_) + "\nmin_count\t" + std::to_string(min_count_) + "\nmax_count\t" + std::to_string(max_count_) +
        "\npositions\t" + (middle_ ? "middle" : "all") + "\n";
    for (int j = 0; j < KT_HET_CENSUS; j++) s += std::string(names[j]) + '\t' + std::to_string(census[j]) + '\n';
    if (std::string e = write_text_file(out_dir_ + "/hetmers.stats", s); !e.empty()) return e;
    run.took(3);
    return "";
}

// ---------------------------------------------------------------------------------------------
UnitigComputer::UnitigComputer(std::string in_path, std::string out_dir, int ksize)
    : in_path_(std::move(in_path)), out_dir_(std::move(out_dir)), ksize_(ksize) {}

UnitigComputer::~UnitigComputer() {
    if (table_) kt_ctr_destroy(table_);
}

// What the device calls of a run returned: the unitigs (kt_ctr_unitigs), with `linked` the links of every unitig end as
// well (kt_ctr_unitigs_linked), with components the component of every unitig and a row per component.
struct UnitigGraph {
    uint64_t nu = 0, nb = 0, nl = 0, nc = 0;  // unitigs, their bases, directed links, components
    std::vector<uint8_t> bases;
    std::vector<uint64_t> offsets, sums;  // per unitig: where its bases begin (nu + 1 values), its count sum
    std::vector<uint64_t> loff, cstats;   // 2 nu + 1 offsets into lto, by unitig end; nc rows of KT_COMPONENT_FIELDS
    std::vector<uint32_t> flags, lto, comp;
    uint64_t ctally[KT_COMPONENT_TALLY] = {};
    uint64_t len(uint64_t i) const { return offsets[i + 1] - offsets[i]; }
};

// which files a run of unitigs() writes (the class comment in computers.hpp says when; `thread` has files of its own)
struct UnitigFiles { bool fa, gfa, links_stats, components, components_stats, unitigs_stats; };

// Of a link e -> f and its mirror (f ^ 1) -> (e ^ 1), the GFA and the edge count take the one that is not the larger as
// (u, su is '-', v, sv is '-'), which is the order of (e, f) as pairs of numbers; a link that is its own mirror is there once.
static bool not_larger_than_mirror(uint64_t e, uint64_t f) {
    const uint64_t me = f ^ 1, mf = e ^ 1;
    return e < me || (e == me && f <= mf);
}

// The tags of unitig i, `sep` in front of each: LN, KC, km, CL on a cycle, with fa_links (the FASTA header) an L per
// directed link, CC with `tagged`.
static void append_unitig_tags(std::string &s, const UnitigGraph &g, uint64_t i, uint64_t overlap, char sep, bool fa_links, bool tagged) {
    const uint64_t len = g.len(i);
    char buf[160];
    const int h = snprintf(buf, sizeof buf, "%cLN:i:%llu%cKC:i:%llu%ckm:f:%.1f", sep, (unsigned long long)len, sep,
                           (unsigned long long)g.sums[i], sep, (double)g.sums[i] / (double)(len - overlap));
    s.append(buf, (size_t)h);
    if (g.flags[i] & KT_UNITIG_CIRCULAR) (s += sep) += "CL:i:1";
    if (fa_links)
        for (uint64_t e = 2 * i; e < 2 * i + 2; e++)
            for (uint64_t j = g.loff[e]; j < g.loff[e + 1]; j++) {
                const int l = snprintf(buf, sizeof buf, "%cL:%c:%u:%c", sep, e & 1 ? '-' : '+', g.lto[j] >> 1, g.lto[j] & 1 ? '-' : '+');
                s.append(buf, (size_t)l);
            }
    if (tagged) ((s += sep) += "CC:i:") += std::to_string(g.comp[i]);
}

static std::string write_fa(const std::string &path, const UnitigGraph &g, uint64_t overlap, bool fa_links, bool tagged) {
    OutFile out;
    if (std::string e = out.open(path); !e.empty()) return e;
    for (uint64_t i = 0; i < g.nu && !out.failed(); i++) {
        std::string &s = out.text();
        s += '>';
        append_uint(s, i);
        append_unitig_tags(s, g, i, overlap, ' ', fa_links, tagged);
        s += '\n';
        s.append((const char *)g.bases.data() + g.offsets[i], (size_t)g.len(i));
        s += '\n';
    }
    return out.close();
}

static std::string write_gfa(const std::string &path, const UnitigGraph &g, uint64_t overlap, bool tagged) {
    OutFile out;
    if (std::string e = out.open(path); !e.empty()) return e;
    out.text() = "H\tVN:Z:1.0\n";
    for (uint64_t i = 0; i < g.nu; i++) {
        std::string &s = out.text();
        s += "S\t";
        append_uint(s, i);
        s += '\t';
        s.append((const char *)g.bases.data() + g.offsets[i], (size_t)g.len(i));
        append_unitig_tags(s, g, i, overlap, '\t', false, tagged);
        s += '\n';
    }
    for (uint64_t e = 0; e < 2 * g.nu; e++)
        for (uint64_t j = g.loff[e]; j < g.loff[e + 1]; j++) {
            const uint64_t f = g.lto[j];
            if (!not_larger_than_mirror(e, f)) continue;
            char line[160];
            const int h = snprintf(line, sizeof line, "L\t%llu\t%c\t%llu\t%c\t%lluM\n", (unsigned long long)(e >> 1), e & 1 ? '-' : '+',
                                   (unsigned long long)(f >> 1), f & 1 ? '-' : '+', (unsigned long long)overlap);
            out.text().append(line, (size_t)h);
        }
    return out.close();
}

static std::string write_links_stats(const std::string &path, const UnitigGraph &g) {
    uint64_t edges = 0, dead = 0, isolated = 0, self = 0, max_deg = 0;
    for (uint64_t e = 0; e < 2 * g.nu; e++) {
        const uint64_t d = g.loff[e + 1] - g.loff[e];
        dead += d == 0;
        isolated += (e & 1) && d == 0 && g.loff[e] == g.loff[e - 1];
        max_deg = std::max(max_deg, d);
        for (uint64_t j = g.loff[e]; j < g.loff[e + 1]; j++) {
            self += (g.lto[j] >> 1) == (e >> 1);
            edges += not_larger_than_mirror(e, g.lto[j]);
        }
    }
    static const char *names[6] = {"links", "edges", "dead_ends", "isolated", "self_links", "max_end_degree"};
    const uint64_t values[6] = {g.nl, edges, dead, isolated, self, max_deg};
    return write_stats_file(path, names, values, 6);
}

// unitigs.components: component, unitigs, nodes, bases, count_sum, km, links, first_unitig
static std::string write_components(const std::string &path, const UnitigGraph &g, uint64_t overlap) {
    std::string s;
    char line[200];
    for (uint64_t c = 0; c < g.nc; c++) {
        const uint64_t *r = &g.cstats[(size_t)c * KT_COMPONENT_FIELDS];
        const int h = snprintf(line, sizeof line, "%llu\t%llu\t%llu\t%llu\t%llu\t%.1f\t%llu\t%llu\n", (unsigned long long)c,
                               (unsigned long long)r[0], (unsigned long long)r[1], (unsigned long long)(r[1] + overlap * r[0]),
                               (unsigned long long)r[2], (double)r[2] / (double)r[1], (unsigned long long)r[3], (unsigned long long)r[4]);
        s.append(line, (size_t)h);
    }
    return write_text_file(path, s);
}

static std::string write_components_stats(const std::string &path, const UnitigGraph &g, uint64_t overlap) {
    static const char *names[4] = {"components", "singletons", "largest_unitigs", "largest_nodes"};
    const uint64_t nodes = g.nb - g.nu * overlap;
    std::string s;
    append_stats_rows(s, names, g.ctally, 4);
    char line[64];
    const int h = snprintf(line, sizeof line, "largest_share\t%.4f\n", nodes ? (double)g.ctally[3] / (double)nodes : 0.0);
    s.append(line, (size_t)h);
    return write_text_file(path, s);
}

static std::string write_unitig_stats(const std::string &path, const UnitigGraph &g, uint64_t overlap) {
    // n50: the length of the first unitig, longest first, at which twice the running sum of lengths reaches `bases`
    std::vector<uint64_t> lens((size_t)g.nu);
    uint64_t occ = 0, circular = 0, singletons = 0, longest = 0, n50 = 0;
    for (uint64_t i = 0; i < g.nu; i++) {
        lens[i] = g.len(i);
        occ += g.sums[i];
        circular += g.flags[i] & KT_UNITIG_CIRCULAR ? 1 : 0;
        singletons += lens[i] == overlap + 1;
        longest = std::max(longest, lens[i]);
    }
    std::sort(lens.begin(), lens.end(), std::greater<uint64_t>());
    for (uint64_t i = 0, run = 0; i < g.nu; i++) {
        run += lens[i];
        if (2 * run >= g.nb) {
            n50 = lens[i];
            break;
        }
    }
    static const char *names[8] = {"unitigs", "bases", "nodes", "occurrences", "circular", "singletons", "longest", "n50"};
    const uint64_t values[8] = {g.nu, g.nb, g.nb - g.nu * overlap, occ, circular, singletons, longest, n50};
    return write_stats_file(path, names, values, 8);
}

// set_bubbles / set_clip: the table is simplified or clipped in place (every file describes that graph), its stats written
std::string UnitigComputer::simplify_table() {
    const uint32_t isolated = drop_isolated_ ? KT_CLIP_ISOLATED : 0u;
    if (pop_) {  // tips (with clip_) and bubbles in the same rounds
        uint64_t st[KT_SIMPLIFY_STATS] = {};
        if (kt_ctr_simplify(table_, min_count_, max_count_, clip_ ? tip_nodes_ : 0u, bubble_nodes_, clip_rounds_, isolated, st) != KT_OK)
            return kt_last_error();
        static const char *names[10] = {"rounds", "tips", "tip_nodes", "isolated", "isolated_nodes", "popped", "popped_nodes", "bubbles",
                                        "occurrences", "converged"};
        const uint64_t values[10] = {st[0], st[1], st[2], st[3], st[4], st[5], st[6], st[7], st[8], st[9] ? 0ull : 1ull};
        return write_stats_file(out_dir_ + "/unitigs.simplify.stats", names, values, 10);
    }
    if (clip_) {
        uint64_t st[KT_CLIP_STATS] = {};
        if (kt_ctr_clip_tips(table_, min_count_, max_count_, tip_nodes_, clip_rounds_, isolated, st) != KT_OK) return kt_last_error();
        static const char *names[7] = {"rounds", "tips", "tip_nodes", "isolated", "isolated_nodes", "occurrences", "converged"};
        const uint64_t values[7] = {st[0], st[1], st[2], st[3], st[4], st[5], st[6] ? 0ull : 1ull};
        return write_stats_file(out_dir_ + "/unitigs.clip.stats", names, values, 7);
    }
    return "";
}

// g: a count-only call, then one sized by it (the links only where a file asks for them); with components_ the components
std::string UnitigComputer::fetch_unitigs(bool linked, UnitigGraph &g) {
    auto call = [&](bool sized) {
        const uint64_t cap_b = sized ? g.nb : 0, cap_u = sized ? g.nu : 0, cap_l = sized ? g.nl : 0;
        uint8_t *bases = sized ? g.bases.data() : nullptr;
        uint64_t *offsets = sized ? g.offsets.data() : nullptr, *sums = sized ? g.sums.data() : nullptr;
        uint32_t *flags = sized ? g.flags.data() : nullptr;
        return linked ? kt_ctr_unitigs_linked(table_, min_count_, max_count_, bases, cap_b, offsets, sums, flags, cap_u, &g.nu, &g.nb,
                                              sized ? g.loff.data() : nullptr, sized ? g.lto.data() : nullptr, cap_l, &g.nl, KT_MEM_HOST)
                      : kt_ctr_unitigs(table_, min_count_, max_count_, bases, cap_b, offsets, sums, flags, cap_u, &g.nu, &g.nb, KT_MEM_HOST);
    };
    if (call(false) != KT_OK) return kt_last_error();
    g.bases.resize((size_t)g.nb);
    g.offsets.resize((size_t)g.nu + 1);
    g.sums.resize((size_t)g.nu);
    g.flags.resize((size_t)g.nu);
    g.loff.resize(linked ? 2 * (size_t)g.nu + 1 : 0);
    g.lto.resize((size_t)g.nl);
    if (g.nu && call(true) != KT_OK) return kt_last_error();
    if (components_) {
        static const uint32_t no_link[1] = {0};
        g.comp.resize((size_t)g.nu);
        g.cstats.resize((size_t)g.nu * KT_COMPONENT_FIELDS);
        if (kt_unitig_components(dev_.ctx, g.loff.data(), g.nl ? g.lto.data() : no_link, g.nu, g.offsets.data(), g.sums.data(), ksize_,
                                 g.comp.data(), g.cstats.data(), g.nu, &g.nc, g.ctally, KT_MEM_HOST) != KT_OK)
            return kt_last_error();
        g.cstats.resize((size_t)g.nc * KT_COMPONENT_FIELDS);
    }
    return "";
}

std::string UnitigComputer::unitigs() {
    const bool linked = gfa_ || fa_links_ || components_;
    const UnitigFiles files = {!stats_only_, gfa_, linked && !thread_, components_ && !(thread_ && stats_only_), components_ && !thread_, !thread_};
    const bool tagged = components_ && !stats_only_;  // the CC:i: fields of unitigs.fa and unitigs.gfa
    // HBM per slot: the slot (16) + its share of what kt_ctr_unitigs keeps when every entry is a node (16 + 64 bytes, 48 more
    // on cycles, the sort's second pair 12), with 1.9 slots per entry: 140 / 1.9 < 74
    // Clipping (kt_ctr_clip_tips) adds, per entry when every entry is a single-node unitig: its offset, count sum, flags and
    // two link offsets in place of bases the run does not write (36), its class and mark (2) - the list of keys to erase (8 a
    // node) lies where the sort's keys lay, the erase's surviving pairs (12) where the nodes lay - and per slot one bit of the
    // erase's mask: 38 / 1.9 + 1 / 8 < 21.  Popping bubbles (kt_ctr_simplify) claims no more than that.
    WholeTableRun run(dev_, in_path_, table_file_, ksize_, clip_ || pop_ ? 16 + 74 + 21 : 16 + 74, "unitigs", &table_);
    if (!run.err.empty()) return run.err;
    if (std::string e = simplify_table(); !e.empty()) return e;
    UnitigGraph g;
    if (std::string e = fetch_unitigs(linked, g); !e.empty()) return e;
    run.took(1);
    const uint64_t overlap = (uint64_t)ksize_ - 1;
    std::string e;
    if (files.fa) e = write_fa(out_dir_ + "/unitigs.fa", g, overlap, fa_links_, tagged);
    if (e.empty() && files.gfa) e = write_gfa(out_dir_ + "/unitigs.gfa", g, overlap, tagged);
    if (e.empty() && files.links_stats) e = write_links_stats(out_dir_ + "/unitigs.links.stats", g);
    if (e.empty() && files.components) e = write_components(out_dir_ + "/unitigs.components", g, overlap);
    if (e.empty() && files.components_stats) e = write_components_stats(out_dir_ + "/unitigs.components.stats", g, overlap);
    if (e.empty() && files.unitigs_stats) e = write_unitig_stats(out_dir_ + "/unitigs.stats", g, overlap);
    if (!e.empty()) return e;
    run.took(3);
    return thread_ ? thread_onto(g) : "";  // (`thread` writes its own statistics)
}

// a batch's runs (kt_thread_runs): start in the batch's bases, k-mers, oriented unitig, place in it; roff: a read's runs
struct ReadRuns {
    std::vector<uint64_t> rs, roff;
    std::vector<uint32_t> rl, ru, rp;
};

// what `thread` adds up over the batches
struct ThreadTotals {
    uint64_t reads = 0, bases = 0, windows = 0, hits = 0, misses = 0, runs = 0, chains = 0, with_hit = 0, whole = 0;
    uint64_t with_comp = 0, mixed = 0;                                      // --components
    std::vector<uint64_t> unitig_hits, unitig_runs, comp_reads, comp_hits;  // per unitig, per component
};

// The runs [r0, r1) of a read that begins at base `o` of its batch, cut into chains: a chain goes on while each further run
// starts where the one before stopped, at the first k-mer of its oriented unitig, the one before having ended at the last of
// its own.  fn(r, e, qs, qe, ps, plen) per chain: its runs [r, e), its bases [qs, qe) of the read, its start in and the length of its path.
template <class F>
static void for_each_chain(const ReadRuns &R, const UnitigGraph &g, uint64_t k, uint64_t o, uint64_t r0, uint64_t r1, F fn) {
    auto ulen = [&](uint32_t e) { return g.len(e >> 1); };
    for (uint64_t r = r0; r < r1;) {
        uint64_t e = r + 1, plen = ulen(R.ru[r]);
        for (; e < r1; e++) {
            const uint64_t L = ulen(R.ru[e]), L0 = ulen(R.ru[e - 1]);
            const bool starts = R.rp[e] == (R.ru[e] & 1u ? L - k : 0);
            const bool ended = R.ru[e - 1] & 1u ? R.rp[e - 1] + 1 == R.rl[e - 1] : R.rp[e - 1] + R.rl[e - 1] - 1 == L0 - k;
            if (R.rs[e] != R.rs[e - 1] + R.rl[e - 1] || !starts || !ended) break;
            plen += L - (k - 1);
        }
        const uint64_t qs = R.rs[r] - o, qe = R.rs[e - 1] - o + R.rl[e - 1] - 1 + k;
        const uint64_t ps = R.ru[r] & 1u ? ulen(R.ru[r]) - k - R.rp[r] : R.rp[r];
        fn(r, e, qs, qe, ps, plen);
        r = e;
    }
}

// thread.gaf: the line of one chain of a read of `len` bases
static void append_gaf_line(std::string &text, const std::string &header, uint64_t len, const ReadRuns &R, uint64_t r, uint64_t e,
                            uint64_t qs, uint64_t qe, uint64_t ps, uint64_t plen) {
    append_name(text, header);
    append_tab_uints(text, {len, qs, qe});
    text += "\t+\t";
    for (uint64_t x = r; x < e; x++) {
        text += R.ru[x] & 1u ? '<' : '>';
        append_uint(text, R.ru[x] >> 1);
    }
    append_tab_uints(text, {plen, ps, ps + qe - qs, qe - qs, qe - qs, 255});
    text += '\n';
}

// thread.reads: the lines of a batch - name, component or *, mixed, hits
static void append_thread_reads(std::string &text, const Batch &b, const ReadRuns &R, const std::vector<uint32_t> &rcomp,
                                const std::vector<uint8_t> &rmixed) {
    for (uint64_t i = 0; i < b.n_reads(); i++) {
        uint64_t h = 0;
        for (uint64_t r = R.roff[i]; r < R.roff[i + 1]; r++) h += R.rl[r];
        append_name(text, b.headers[i]);
        text += '\t';
        if (rcomp[i] == KT_NO_COMPONENT) text += '*';
        else append_uint(text, rcomp[i]);
        append_tab_uints(text, {rmixed[i] ? 1u : 0u, h});
        text += '\n';
    }
}

// `thread`: the unitigs (host arrays, as kt_ctr_unitigs filled them) become the index, the records of thread_reads_ are
// walked in the usual batches.  The counted table has done its work by now and makes room for the index.
std::string UnitigComputer::thread_onto(const UnitigGraph &g) {
    PhaseTimer pt("thread");
    Lap lap;
    const std::vector<uint64_t> &offsets = g.offsets;
    const uint64_t nu = offsets.size() - 1, nb = offsets[nu], k = (uint64_t)ksize_, nc = g.cstats.size() / KT_COMPONENT_FIELDS;
    if (table_) kt_ctr_destroy(table_);
    table_ = nullptr;
    const uint64_t windows = nb - nu * (k - 1);
    if (kt_ctr_create(dev_.ctx, ksize_, std::max<uint64_t>(1024, windows + windows / 10 * 9), &table_) != KT_OK) return kt_last_error();
    uint64_t indexed = 0;
    static const uint64_t no_offsets[1] = {0};
    if (kt_ctr_index_sequences(table_, nb ? g.bases.data() : (const uint8_t *)"", nu ? offsets.data() : no_offsets, nu, &indexed, KT_MEM_HOST) != KT_OK)
        return kt_last_error();
    pt.t[1] += lap();

    SeqReader reader;
    if (!reader.open(thread_reads_, false)) return reader.error();
    // thread.gaf, and with --components thread.reads: every record's component (kt_thread_read_components over the batch's runs)
    OutFile fg, fr;
    if (!stats_only_) {
        if (std::string e = fg.open(out_dir_ + "/thread.gaf"); !e.empty()) return e;
        if (components_)
            if (std::string e = fr.open(out_dir_ + "/thread.reads"); !e.empty()) return e;
    }
    ThreadTotals T;
    T.unitig_hits.assign((size_t)nu, 0), T.unitig_runs.assign((size_t)nu, 0);
    T.comp_reads.assign((size_t)nc, 0), T.comp_hits.assign((size_t)nc, 0);
    Batch batch;
    ReadRuns R;
    std::vector<uint32_t> hits, rcomp;
    std::vector<uint8_t> rmixed;
    std::string text;
    std::string err = walk(reader, batch, TABLE_BATCH_BASES, 1ull << 20, true, &pt, &lap, nullptr, [&](const Batch &b, const Cursor &) -> std::string {
        const uint64_t n = b.n_reads(), total = b.offsets[n];
        hits.assign(total, KT_NO_KMER);
        if (total && kt_ctr_thread_hits(table_, bases_ptr(b), b.offsets.data(), n, hits.data(), KT_MEM_HOST) != KT_OK) return kt_last_error();
        // a counting call, then one sized by it
        uint64_t nr = 0, tally[KT_THREAD_TALLY] = {};
        R.roff.resize(n + 1);
        if (kt_thread_runs(dev_.ctx, hits.data(), b.offsets.data(), n, nu ? offsets.data() : no_offsets, nu, ksize_, nullptr, nullptr, nullptr,
                           nullptr, R.roff.data(), 0, &nr, nullptr, nullptr, tally, KT_MEM_HOST) != KT_OK)
            return kt_last_error();
        R.rs.resize(nr), R.rl.resize(nr), R.ru.resize(nr), R.rp.resize(nr);
        if (nr && kt_thread_runs(dev_.ctx, hits.data(), b.offsets.data(), n, offsets.data(), nu, ksize_, R.rs.data(), R.rl.data(), R.ru.data(),
                                 R.rp.data(), R.roff.data(), nr, &nr, T.unitig_hits.data(), T.unitig_runs.data(), tally, KT_MEM_HOST) != KT_OK)
            return kt_last_error();
        if (components_ && n) {
            static const uint32_t none[1] = {0};
            uint64_t t[KT_READ_COMPONENT_TALLY] = {};
            rcomp.resize(n), rmixed.resize(n);
            if (kt_thread_read_components(dev_.ctx, nr ? R.ru.data() : none, nr ? R.rl.data() : none, R.roff.data(), n, nu ? g.comp.data() : none,
                                          nu, nc, rcomp.data(), rmixed.data(), T.comp_reads.data(), T.comp_hits.data(), t, KT_MEM_HOST) != KT_OK)
                return kt_last_error();
            T.with_comp += t[0], T.mixed += t[2];
            if (fr.is_open()) {
                append_thread_reads(text, b, R, rcomp, rmixed);
                if (!fr.write(text)) return fr.close();
                text.clear();
            }
        }
        pt.t[1] += lap();
        T.reads += n, T.bases += total, T.windows += tally[0], T.hits += tally[1], T.misses += tally[2], T.runs += tally[4], T.with_hit += tally[5];
        for (uint64_t i = 0; i < n; i++) {
            const uint64_t o = b.offsets[i], len = b.offsets[i + 1] - o;
            uint64_t chains_here = 0, first_qs = 0, last_qe = 0;
            for_each_chain(R, g, k, o, R.roff[i], R.roff[i + 1], [&](uint64_t r, uint64_t e, uint64_t qs, uint64_t qe, uint64_t ps, uint64_t plen) {
                if (!chains_here++) first_qs = qs;
                last_qe = qe;
                if (fg.is_open()) append_gaf_line(text, b.headers[i], len, R, r, e, qs, qe, ps, plen);
            });
            T.chains += chains_here;
            T.whole += chains_here == 1 && first_qs == 0 && last_qe == len;
        }
        pt.t[2] += lap();
        if (!fg.write(text)) return fg.close();
        text.clear();
        pt.t[3] += lap();
        return "";
    });
    const std::string eg = fg.close(), er = fr.close();
    if (err.empty()) err = eg.empty() ? er : eg;
    if (!err.empty()) return err;

    uint64_t unitigs_hit = 0;
    for (uint64_t u = 0; u < nu; u++) {
        const uint64_t len = g.len(u), nodes = len - (k - 1);
        char line[200];
        const int h = snprintf(line, sizeof line, "%llu\t%llu\t%llu\t%llu\t%llu\t%llu\t%.6f\n", (unsigned long long)u, (unsigned long long)len,
                               (unsigned long long)nodes, (unsigned long long)g.sums[u], (unsigned long long)T.unitig_hits[u],
                               (unsigned long long)T.unitig_runs[u], (double)T.unitig_hits[u] / (double)nodes);
        text.append(line, (size_t)h);
        unitigs_hit += T.unitig_hits[u] != 0;
    }
    if (std::string e = write_text_file(out_dir_ + "/thread.unitigs", text); !e.empty()) return e;
    static const char *names[10] = {"reads", "bases", "windows", "hits", "misses", "runs", "chains", "reads_with_hit",
                                    "reads_one_chain_end_to_end", "unitigs_hit"};
    const uint64_t values[10] = {T.reads, T.bases, T.windows, T.hits, T.misses, T.runs, T.chains, T.with_hit, T.whole, unitigs_hit};
    std::string s;
    append_stats_rows(s, names, values, 10);
    if (components_) {
        uint64_t comps_hit = 0;
        text.clear();
        for (uint64_t c = 0; c < nc; c++) {
            const uint64_t *r = &g.cstats[(size_t)c * KT_COMPONENT_FIELDS];
            append_uint(text, c);
            append_tab_uints(text, {r[0], r[1], T.comp_reads[c], T.comp_hits[c]});
            text += '\n';
            comps_hit += T.comp_hits[c] != 0;
        }
        if (std::string e = write_text_file(out_dir_ + "/thread.components", text); !e.empty()) return e;
        static const char *cnames[3] = {"reads_with_component", "reads_mixed", "components_hit"};
        const uint64_t cvalues[3] = {T.with_comp, T.mixed, comps_hit};
        append_stats_rows(s, cnames, cvalues, 3);
    }
    if (std::string e = write_text_file(out_dir_ + "/thread.stats", s); !e.empty()) return e;
    pt.t[3] += lap();
    return "";
}

// ---------------------------------------------------------------------------------------------
// minimisers: one C-ABI call per batch; the capacity is a guess that is corrected on the first miss
static std::string minimiser_batch(kt_ctx *ctx, Work &w, uint64_t wsize, int msize) {
    const uint64_t n = w.b.n_reads();
    w.u64[0].resize(n + 1);
    uint64_t cap = w.u64[1].size();
    if (cap < n + 16) cap = wsize ? w.b.bases.size() / 4 + n + 16 : n + 16;
    for (int attempt = 0; attempt < 2; attempt++) {
        for (int i = 1; i < 4; i++) w.u64[i].resize(cap);
        const int rc = kt_minimisers(ctx, bases_ptr(w.b), w.b.offsets.data(), n, wsize, msize, w.u64[0].data(),
                                     w.u64[1].data(), w.u64[2].data(), w.u64[3].data(), cap, &w.n_events, KT_MEM_HOST);
        if (rc == KT_OK) return "";
        if (w.n_events <= cap) return kt_last_error();  // a real error, not a capacity miss
        cap = w.n_events;
    }
    return kt_last_error();
}

static void append_mmer(std::string &s, uint64_t kmer, int msize) {
    char buf[40];
    kt_numeric_to_kmer(kmer, msize, buf);  // u64::MAX (no full window) prints as all T, like the reference
    s += buf;
}

static std::string check_min_args(uint64_t wsize, int msize, const std::string &in_path) {
    if (msize < 1 || msize > 31) return "minimiser size must be in 1..31";
    if (wsize != 0 && wsize < (uint64_t)msize) return "window size must not be shorter than the minimiser";
    if (format_from_path(in_path) == SeqFormat::Unknown && in_path != "-")
        return "unsupported input extension (expected .fa/.fasta/.fna/.fq/.fastq[.gz]): " + in_path;  // SeqFormat::get().unwrap()
    return "";
}

std::string seq_to_min(uint64_t wsize, int msize, const std::string &in_path, const std::string &out_path, int threads,
                       int device) {
    if (std::string e = check_min_args(wsize, msize, in_path); !e.empty()) return e;
    SeqReader reader;
    if (!reader.open(in_path, false)) return reader.error();
    OutFile out;
    if (std::string e = out.open(out_path); !e.empty()) return e;
    Device dev;
    dev.index = device;
    if (std::string e = dev.ensure(); !e.empty()) return e;
    std::vector<std::string> pieces;
    PhaseTimer pt("min s2m");
    AsyncWriter writer(out.stream(), pt);
    return run_pipeline(
        reader, 64ull << 20, 1ull << 19, pt, [&](Work &w) { return minimiser_batch(dev.ctx, w, wsize, msize); },
        [&](Work &w) {
            Lap lap;
            const uint64_t *evo = w.u64[0].data(), *km = w.u64[1].data(), *st = w.u64[2].data(), *en = w.u64[3].data();
            const uint64_t n = w.b.n_reads();
            const size_t per_row = n ? (size_t)(w.n_events / n + 1) * (size_t)(msize + 12) + 24 : 1;
            format_rows(n, threads, per_row, pieces, [&](uint64_t r, std::string &s) {
                s += w.b.ids[r];  // mins.join("\t") over [id, "MMER:s-e"..., "\n"]  (:131-141)
                for (uint64_t j = evo[r]; j < evo[r + 1]; j++) {
                    s += '\t';
                    append_mmer(s, km[j], msize);
                    s += ':';
                    append_uint(s, st[j]);
                    s += '-';
                    append_uint(s, en[j]);
                }
                s += "\t\n";
            });
            pt.t[2] += lap();
            writer.write(pieces);
        },
        true);
}

// Rust's {:?} for a String: quotes, with \" \\ \t \n \r and other control characters escaped
static void append_debug_str(std::string &s, const std::string &id) {
    s += '"';
    for (unsigned char c : id) {
        switch (c) {
            case '"': s += "\\\""; break;
            case '\\': s += "\\\\"; break;
            case '\t': s += "\\t"; break;
            case '\n': s += "\\n"; break;
            case '\r': s += "\\r"; break;
            case '\'': s += "'"; break;
            default:
                if (c < 0x20 || c == 0x7f) {
                    char buf[16];
                    snprintf(buf, sizeof buf, "\\u{%x}", c);
                    s += buf;
                } else {
                    s += (char)c;
                }
        }
    }
    s += '"';
}

std::string bin_sequences(uint64_t wsize, int msize, const std::string &in_path, const std::string &out_path, int threads,
                          int device) {
    if (std::string e = check_min_args(wsize, msize, in_path); !e.empty()) return e;
    SeqReader reader;
    if (!reader.open(in_path, false)) return reader.error();
    OutFile out;
    if (std::string e = out.open(out_path); !e.empty()) return e;
    Device dev;
    dev.index = device;
    if (std::string e = dev.ensure(); !e.empty()) return e;
    // the whole file's triples are grouped by minimiser at the end, like the reference's in-memory map
    struct Hit {
        uint64_t kmer;
        uint32_t id, start, end;  // id = index into `ids`
    };
    std::vector<Hit> hits;
    std::vector<std::string> ids;
    PhaseTimer pt("min m2s");
    const std::string err = run_pipeline(
        reader, 64ull << 20, 1ull << 19, pt, [&](Work &w) { return minimiser_batch(dev.ctx, w, wsize, msize); },
        [&](Work &w) {
            Lap lap;
            const uint64_t *evo = w.u64[0].data();
            const uint32_t id0 = (uint32_t)ids.size();
            ids.insert(ids.end(), w.b.ids.begin(), w.b.ids.end());
            for (uint64_t r = 0; r < w.b.n_reads(); r++)
                for (uint64_t j = evo[r]; j < evo[r + 1]; j++)
                    hits.push_back(Hit{w.u64[1][j], id0 + (uint32_t)r, (uint32_t)w.u64[2][j], (uint32_t)w.u64[3][j]});
            pt.t[2] += lap();
        },
        true);
    if (!err.empty()) return err;
    Lap lap;
    // ascending minimiser text == ascending value of its low 2m bits (A < C < G < T is the 2-bit order)
    const uint64_t mask = msize >= 32 ? ~0ull : ((1ull << (2 * msize)) - 1ull);
    std::stable_sort(hits.begin(), hits.end(), [&](const Hit &x, const Hit &y) { return (x.kmer & mask) < (y.kmer & mask); });
    std::vector<uint64_t> group_start;
    for (uint64_t i = 0; i < hits.size(); i++)
        if (i == 0 || (hits[i].kmer & mask) != (hits[i - 1].kmer & mask)) group_start.push_back(i);
    group_start.push_back(hits.size());
    std::vector<std::string> pieces;
    const uint64_t n_groups = group_start.size() - 1;
    format_rows(n_groups, threads, (size_t)msize + 48, pieces, [&](uint64_t g, std::string &s) {
        append_mmer(s, hits[group_start[g]].kmer, msize);  // "{k}\t{v:?}\n"  (:81-84)
        s += "\t[";
        for (uint64_t i = group_start[g]; i < group_start[g + 1]; i++) {
            if (i != group_start[g]) s += ", ";
            s += '(';
            append_debug_str(s, ids[hits[i].id]);
            s += ", ";
            append_uint(s, hits[i].start);
            s += ", ";
            append_uint(s, hits[i].end);
            s += ')';
        }
        s += "]\n";
    });
    pt.t[2] += lap();
    out.write(pieces);
    (void)out.close();  // (no write error is reported here either, as with the ordered writer)
    pt.t[3] += lap();
    return "";
}

// ---------------------------------------------------------------------------------------------
SketchComputer::SketchComputer(std::string in_path, std::string out_dir, int ksize, uint32_t sketch_size)
    : in_path_(std::move(in_path)), out_dir_(std::move(out_dir)), ksize_(ksize), s_(sketch_size) {}

static void append_sketch_line(std::string &text, const std::string &id, uint64_t length, uint64_t kmers, uint32_t size,
                               const uint64_t *row) {
    text += id;
    append_tab_uints(text, {length, kmers, size});
    text += '\t';
    for (uint32_t t = 0; t < size; t++) {
        if (t) text += ',';
        append_uint(text, row[t]);
    }
    text += '\n';
}

// the sketches of one input: its lines into out_path, the sketches themselves into `set` when the distances want them
std::string SketchComputer::sketch_input(const std::string &path, const std::string &out_path, Set &set, bool keep) {
    SeqReader reader;
    if (!reader.open(path, false)) return reader.error();
    OutFile out;
    if (std::string e = out.open(out_path); !e.empty()) return e;
    PhaseTimer pt("sketch");
    Lap lap;
    Batch b;
    std::string text, err, name;
    std::vector<uint64_t> hashes, run_h, merged_h;  // run_h: --single, the sketch of everything read so far in front of the batch's rows
    std::vector<uint32_t> sizes, nk, run_s, merged_s(1);
    uint64_t all_bases = 0, all_kmers = 0;
    bool any = false;
    for (;;) {
        const bool more = reader.next_batch(b, cli_batch_bases(256ull << 20), cli_batch_reads(1ull << 20), false, true);
        pt.t[0] += lap();
        const uint64_t n = b.n_reads();
        if (n) {
            hashes.resize(n * s_);
            sizes.resize(n);
            nk.resize(n);
            if (kt_sketch_batch(dev_.ctx, bases_ptr(b), b.offsets.data(), n, ksize_, s_, seed_, hashes.data(), sizes.data(), nk.data(),
                                KT_MEM_HOST) != KT_OK) {
                err = kt_last_error();
                break;
            }
            if (single_) {
                // one group: the running sketch and the batch's rows
                const uint64_t rows = n + (any ? 1 : 0);
                run_h.resize((any ? s_ : 0));
                run_h.insert(run_h.end(), hashes.begin(), hashes.end());
                run_s.resize(any ? 1 : 0);
                run_s.insert(run_s.end(), sizes.begin(), sizes.end());
                const uint64_t go[2] = {0, rows};
                merged_h.resize(s_);
                if (kt_sketch_merge(dev_.ctx, run_h.data(), run_s.data(), rows, s_, go, 1, merged_h.data(), merged_s.data(), KT_MEM_HOST) !=
                    KT_OK) {
                    err = kt_last_error();
                    break;
                }
                run_h.assign(merged_h.begin(), merged_h.end());
                run_s.assign(1, merged_s[0]);
                any = true;
                all_bases += b.offsets[n];
                for (uint64_t i = 0; i < n; i++) all_kmers += nk[i];
                pt.t[1] += lap();
            } else {
                pt.t[1] += lap();
                text.clear();
                for (uint64_t i = 0; i < n; i++) {
                    name.clear();
                    append_name(name, b.headers[i]);
                    append_sketch_line(text, name, b.offsets[i + 1] - b.offsets[i], nk[i], sizes[i], hashes.data() + i * s_);
                    if (keep) set.ids.push_back(name);
                }
                if (keep) {
                    set.hashes.insert(set.hashes.end(), hashes.begin(), hashes.end());
                    set.sizes.insert(set.sizes.end(), sizes.begin(), sizes.end());
                }
                pt.t[2] += lap();
                if (!out.write(text)) {
                    err = out.close();
                    break;
                }
                pt.t[3] += lap();
            }
        }
        if (!more) break;
    }
    if (err.empty() && reader.failed()) err = reader.error();
    if (err.empty() && single_) {
        const size_t slash = path.find_last_of('/');
        name = slash == std::string::npos ? path : path.substr(slash + 1);
        if (!any) {
            run_h.assign(s_, KT_EMPTY_KEY);
            run_s.assign(1, 0u);
        }
        text.clear();
        append_sketch_line(text, name, all_bases, all_kmers, run_s[0], run_h.data());
        if (keep) {
            set.ids.push_back(name);
            set.hashes.assign(run_h.begin(), run_h.begin() + s_);
            set.sizes.assign(1, run_s[0]);
        }
        out.write(text);
    }
    if (std::string e = out.close(); err.empty()) err = e;
    return err;
}

// sketch.dist: the pairs i < j of `a` (b == nullptr) or every (i of a, j of b), a block of rows of the matrix at a time
std::string SketchComputer::write_dist(const Set &a, const Set *b) {
    OutFile out;
    if (std::string e = out.open(out_dir_ + "/sketch.dist"); !e.empty()) return e;
    const Set &bb = b ? *b : a;
    const uint64_t n_a = a.sizes.size(), n_b = bb.sizes.size();
    std::string err, text;
    if (n_a && n_b) {
        // the block's two u32 matrices stay within 1 GiB
        uint64_t rows = (1ull << 30) / (8 * n_b);
        rows = rows < 1 ? 1 : (rows > n_a ? n_a : rows);
        std::vector<uint32_t> shared(rows * n_b), denom(rows * n_b);
        for (uint64_t i0 = 0; i0 < n_a && err.empty(); i0 += rows) {
            const uint64_t r = n_a - i0 < rows ? n_a - i0 : rows;
            if (kt_sketch_pairs(dev_.ctx, a.hashes.data() + i0 * s_, a.sizes.data() + i0, r, bb.hashes.data(), bb.sizes.data(), n_b, s_,
                                shared.data(), denom.data(), KT_MEM_HOST) != KT_OK) {
                err = kt_last_error();
                break;
            }
            text.clear();
            for (uint64_t i = i0; i < i0 + r; i++) {
                for (uint64_t j = b ? 0 : i + 1; j < n_b; j++) {
                    const uint32_t sh = shared[(i - i0) * n_b + j], dn = denom[(i - i0) * n_b + j];
                    const double d = kt_mash_distance(sh, dn, ksize_);
                    if (d > max_dist_) continue;
                    text += a.ids[i];
                    text += '\t';
                    text += bb.ids[j];
                    text += '\t';
                    append_uint(text, sh);
                    text += '/';
                    append_uint(text, dn);
                    text += '\t';
                    append_display(text, dn ? (double)sh / (double)dn : 0.0);
                    text += '\t';
                    append_display(text, d);
                    text += '\n';
                }
            }
            if (!out.write(text)) err = out.close();
        }
    }
    if (std::string e = out.close(); err.empty()) err = e;
    return err;
}

// ---- sketch --scaled -------------------------------------------------------------------------------------------------------
static void append_scaled_line(std::string &text, const std::string &id, uint64_t length, uint64_t kmers, uint64_t size,
                               const uint64_t *row, const uint32_t *abunds) {
    text += id;
    append_tab_uints(text, {length, kmers, size});
    text += '\t';
    for (uint64_t t = 0; t < size; t++) {
        if (t) text += ',';
        append_uint(text, row[t]);
    }
    if (abunds) {
        text += '\t';
        for (uint64_t t = 0; t < size; t++) {
            if (t) text += ',';
            append_uint(text, abunds[t]);
        }
    }
    text += '\n';
}

static std::string file_name_of(const std::string &path) {
    const size_t slash = path.find_last_of('/');
    return slash == std::string::npos ? path : path.substr(slash + 1);
}

// One sized call: `call(max_out, &n_out)` is tried with the room the arrays have; a result that does not fit is refused with
// its exact size, the arrays grow to it and the call is made again.
template <class CallFn>
static int sized_call(std::vector<uint64_t> &hashes, std::vector<uint32_t> &abunds, uint64_t guess, uint64_t *n_out, CallFn call) {
    if (hashes.size() < guess) hashes.resize(guess);
    if (hashes.empty()) hashes.resize(1);
    abunds.resize(hashes.size());
    *n_out = 0;
    int rc = call(hashes.size(), n_out);
    if (rc == KT_ERR_ARG && *n_out > hashes.size()) {
        hashes.resize(*n_out);
        abunds.resize(*n_out);
        rc = call(hashes.size(), n_out);
    }
    return rc;
}

// the scaled sketches of one input: its lines into out_path, the sketches themselves into `set` when sketch.contain wants them
std::string SketchComputer::scaled_input(const std::string &path, const std::string &out_path, ScaledSet &set, bool keep) {
    SeqReader reader;
    if (!reader.open(path, false)) return reader.error();
    OutFile out;
    if (std::string e = out.open(out_path); !e.empty()) return e;
    PhaseTimer pt("sketch");
    Lap lap;
    Batch b;
    std::string text, err, name;
    std::vector<uint64_t> hashes, ro, run_h, in_h, in_o, merged_h;  // run_*: --single, the sketch of everything read so far
    std::vector<uint32_t> abunds, nk, run_a, in_a, merged_a;
    uint64_t all_bases = 0, all_kmers = 0;
    for (;;) {
        const bool more = reader.next_batch(b, cli_batch_bases(256ull << 20), cli_batch_reads(1ull << 20), false, true);
        pt.t[0] += lap();
        const uint64_t n = b.n_reads();
        if (n) {
            ro.resize(n + 1);
            nk.resize(n);
            uint64_t n_out = 0;
            const uint64_t guess = b.offsets[n] / scaled_ * 2 + 4096;
            if (sized_call(hashes, abunds, guess, &n_out, [&](uint64_t room, uint64_t *got) {
                    return kt_scaled_batch(dev_.ctx, bases_ptr(b), b.offsets.data(), n, ksize_, scaled_, seed_, hashes.data(), abunds.data(),
                                           room, ro.data(), nk.data(), got, KT_MEM_HOST);
                }) != KT_OK) {
                err = kt_last_error();
                break;
            }
            if (single_) {
                // one group: the running sketch and the batch's rows
                in_h.assign(run_h.begin(), run_h.end());
                in_h.insert(in_h.end(), hashes.begin(), hashes.begin() + n_out);
                in_a.assign(run_a.begin(), run_a.end());
                in_a.insert(in_a.end(), abunds.begin(), abunds.begin() + n_out);
                in_o.assign(1, 0);
                for (uint64_t i = 0; i <= n; i++) in_o.push_back(run_h.size() + ro[i]);
                const uint64_t go[2] = {0, n + 1};
                uint64_t mo[2] = {0, 0}, m_out = 0;
                if (sized_call(merged_h, merged_a, in_h.size(), &m_out, [&](uint64_t room, uint64_t *got) {
                        return kt_scaled_merge(dev_.ctx, in_h.data(), in_a.data(), in_o.data(), n + 1, go, 1, merged_h.data(), merged_a.data(),
                                               room, mo, got, KT_MEM_HOST);
                    }) != KT_OK) {
                    err = kt_last_error();
                    break;
                }
                run_h.assign(merged_h.begin(), merged_h.begin() + m_out);
                run_a.assign(merged_a.begin(), merged_a.begin() + m_out);
                all_bases += b.offsets[n];
                for (uint64_t i = 0; i < n; i++) all_kmers += nk[i];
                pt.t[1] += lap();
            } else {
                pt.t[1] += lap();
                text.clear();
                for (uint64_t i = 0; i < n; i++) {
                    name.clear();
                    append_name(name, b.headers[i]);
                    append_scaled_line(text, name, b.offsets[i + 1] - b.offsets[i], nk[i], ro[i + 1] - ro[i], hashes.data() + ro[i],
                                       abund_ ? abunds.data() + ro[i] : nullptr);
                    if (keep) {
                        set.ids.push_back(name);
                        set.offsets.push_back(set.hashes.size() + ro[i + 1]);
                    }
                }
                if (keep) set.hashes.insert(set.hashes.end(), hashes.begin(), hashes.begin() + n_out);
                pt.t[2] += lap();
                if (!out.write(text)) {
                    err = out.close();
                    break;
                }
                pt.t[3] += lap();
            }
        }
        if (!more) break;
    }
    if (err.empty() && reader.failed()) err = reader.error();
    if (err.empty() && single_) {
        name = file_name_of(path);
        text.clear();
        append_scaled_line(text, name, all_bases, all_kmers, run_h.size(), run_h.data(), abund_ ? run_a.data() : nullptr);
        if (keep) {
            set.ids.push_back(name);
            set.hashes = run_h;
            set.offsets = {0, run_h.size()};
        }
        out.write(text);
    }
    if (std::string e = out.close(); err.empty()) err = e;
    return err;
}

// --table: the one sketch of a table file's k-mers in the count range (the file's sections are loaded into one table)
std::string SketchComputer::scaled_table(const std::string &out_path, ScaledSet &set, bool keep) {
    kt_ctr *table = nullptr;
    if (std::string e = table_from_file(dev_, table_path_, ksize_, 16, "table", &table); !e.empty()) {
        if (table) kt_ctr_destroy(table);
        return e;
    }
    std::vector<uint64_t> hashes;
    std::vector<uint32_t> abunds;
    uint64_t entries = 0, n_out = 0, totals[2] = {0, 0};
    std::string err;
    if (kt_ctr_size(table, &entries) != KT_OK ||
        sized_call(hashes, abunds, entries / scaled_ * 2 + 4096, &n_out, [&](uint64_t room, uint64_t *got) {
            return kt_ctr_scaled(table, min_count_, max_count_, scaled_, seed_, hashes.data(), abunds.data(), room, got, totals, KT_MEM_HOST);
        }) != KT_OK)
        err = kt_last_error();
    kt_ctr_destroy(table);
    if (!err.empty()) return err;
    OutFile out;
    if (std::string e = out.open(out_path); !e.empty()) return e;
    const std::string name = file_name_of(table_path_);
    std::string text;
    append_scaled_line(text, name, 0, totals[1], n_out, hashes.data(), abund_ ? abunds.data() : nullptr);
    if (keep) {
        set.ids.push_back(name);
        set.hashes.assign(hashes.begin(), hashes.begin() + n_out);
        set.offsets = {0, n_out};
    }
    out.write(text);
    return out.close();
}

// sketch.contain: the pairs i < j of `a` (b == nullptr) or every (i of a, j of b), a block of rows of the matrix at a time
std::string SketchComputer::write_contain(const ScaledSet &a, const ScaledSet *b) {
    OutFile out;
    if (std::string e = out.open(out_dir_ + "/sketch.contain"); !e.empty()) return e;
    const ScaledSet &bb = b ? *b : a;
    const uint64_t n_a = a.ids.size(), n_b = bb.ids.size();
    std::string err, text;
    if (n_a && n_b) {
        // the block's u32 matrix stays within 1 GiB
        uint64_t rows = (1ull << 30) / (4 * n_b);
        rows = rows < 1 ? 1 : (rows > n_a ? n_a : rows);
        std::vector<uint32_t> shared(rows * n_b);
        for (uint64_t i0 = 0; i0 < n_a && err.empty(); i0 += rows) {
            const uint64_t r = n_a - i0 < rows ? n_a - i0 : rows;
            if (kt_scaled_pairs(dev_.ctx, a.hashes.data(), a.offsets.data() + i0, r, bb.hashes.data(), bb.offsets.data(), n_b, shared.data(),
                                KT_MEM_HOST) != KT_OK) {
                err = kt_last_error();
                break;
            }
            text.clear();
            for (uint64_t i = i0; i < i0 + r; i++) {
                const uint64_t size_a = a.offsets[i + 1] - a.offsets[i];
                for (uint64_t j = b ? 0 : i + 1; j < n_b; j++) {
                    const uint64_t sh = shared[(i - i0) * n_b + j], size_b = bb.offsets[j + 1] - bb.offsets[j];
                    const double ca = size_a ? (double)sh / (double)size_a : 0.0, cb = size_b ? (double)sh / (double)size_b : 0.0;
                    if ((ca >= cb ? ca : cb) < min_contain_) continue;
                    const uint64_t uni = size_a + size_b - sh;
                    text += a.ids[i];
                    text += '\t';
                    text += bb.ids[j];
                    append_tab_uints(text, {sh, size_a, size_b});
                    for (const double x : {uni ? (double)sh / (double)uni : 0.0, ca, cb,
                                           kt_containment_ani(sh, ca >= cb ? size_a : size_b, ksize_)}) {
                        text += '\t';
                        append_display(text, x);
                    }
                    text += '\n';
                }
            }
            if (!out.write(text)) err = out.close();
        }
    }
    if (std::string e = out.close(); err.empty()) err = e;
    return err;
}

std::string SketchComputer::sketch() {
    if (std::string e = dev_.ensure(); !e.empty()) return e;
    if (scaled_) {
        ScaledSet sa, sb;
        if (std::string e = table_path_.empty() ? scaled_input(in_path_, out_dir_ + "/sketch.tsv", sa, contain_)
                                                : scaled_table(out_dir_ + "/sketch.tsv", sa, contain_);
            !e.empty())
            return e;
        if (!alt_path_.empty())
            if (std::string e = scaled_input(alt_path_, out_dir_ + "/sketch.alt.tsv", sb, contain_); !e.empty()) return e;
        if (contain_) return write_contain(sa, alt_path_.empty() ? nullptr : &sb);
        return "";
    }
    Set a, b;
    if (std::string e = sketch_input(in_path_, out_dir_ + "/sketch.tsv", a, dist_); !e.empty()) return e;
    if (!alt_path_.empty())
        if (std::string e = sketch_input(alt_path_, out_dir_ + "/sketch.alt.tsv", b, dist_); !e.empty()) return e;
    if (dist_) return write_dist(a, alt_path_.empty() ? nullptr : &b);
    return "";
}

// ---- card ------------------------------------------------------------------------------------------------------------
CardComputer::CardComputer(std::string in_path, std::string out_dir, int ksize, int precision)
    : in_path_(std::move(in_path)), out_dir_(std::move(out_dir)), ksize_(ksize), p_(precision) {}

static void append_fixed6_row(std::string &s, const std::string &name, double x) {
    s += name;
    s += '\t';
    append_fixed6(s, x);
    s += '\n';
}

std::string CardComputer::card() {
    if (std::string e = dev_.ensure(); !e.empty()) return e;
    const size_t m = (size_t)1 << p_;
    std::vector<uint8_t> regs[2];
    double est[2] = {0.0, 0.0};
    std::string s;
    const int n_in = alt_path_.empty() ? 1 : 2;
    for (int i = 0; i < n_in; i++) {
        const std::string &path = i ? alt_path_ : in_path_;
        const std::string pre = i ? "alt_" : "";
        regs[i].assign(m, 0);
        uint64_t n_kmers = 0, zeros = 0;
        Cursor end;
        if (std::string e = card_walk(dev_.ctx, path, ksize_, p_, seed_, regs[i], &n_kmers, &end); !e.empty()) return e;
        if (kt_card_estimate(regs[i].data(), p_, &est[i], &zeros) != KT_OK) return kt_last_error();
        // what the table plan of this input would ask for with --estimate-size: never more than the input's bound
        InputBound in;
        if (std::string e = slots_wanted(path, ksize_, &in, dev_); !e.empty()) return e;
        const std::string names[7] = {pre + "sequences", pre + "bases", pre + "kmers", pre + "precision", pre + "registers",
                                      pre + "zero_registers", pre + "distinct_estimate"};
        const uint64_t values[7] = {end.reads, end.bases, n_kmers, (uint64_t)p_, (uint64_t)m, zeros, (uint64_t)floor(est[i] + 0.5)};
        for (int j = 0; j < 7; j++) s += names[j] + '\t' + std::to_string(values[j]) + '\n';
        append_fixed6_row(s, pre + "rel_std_error", kt_card_rel_error(p_));
        s += pre + "slots_wanted\t" + std::to_string(std::min(in.want, slots_for_estimate(est[i], p_))) + '\n';

        std::string r = std::to_string(p_) + '\t' + std::to_string(seed_) + '\t' + std::to_string(ksize_) + '\n';
        for (size_t j = 0; j < m; j++) {
            append_uint(r, regs[i][j]);
            r += '\n';
        }
        if (std::string e = write_text_file(out_dir_ + (i ? "/card.alt.registers" : "/card.registers"), r); !e.empty()) return e;
    }
    if (n_in == 2) {
        if (kt_card_merge(regs[0].data(), regs[1].data(), p_) != KT_OK) return kt_last_error();
        double uni = 0.0;
        if (kt_card_estimate(regs[0].data(), p_, &uni, nullptr) != KT_OK) return kt_last_error();
        const double inter = est[0] + est[1] - uni > 0.0 ? est[0] + est[1] - uni : 0.0;
        const char *names[2] = {"union_estimate", "intersection_estimate"};
        const uint64_t values[2] = {(uint64_t)floor(uni + 0.5), (uint64_t)floor(inter + 0.5)};
        append_stats_rows(s, names, values, 2);
        append_fixed6_row(s, "jaccard_estimate", uni > 0.0 ? inter / uni : 0.0);
    }
    return write_text_file(out_dir_ + "/card.stats", s);
}

}  // namespace kthost
