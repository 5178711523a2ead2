// kt_tablefile.hip - "ktab" table files (DESIGN.md, Table files): a counted k-mer table on disk, packed and unpacked on the device.
//
//   file     "KTAB" u32 version(1) u32 k u32 0, then sections up to the end of the file
//   section  "KSEC" u32 S u64 n u64 n_overflow u64 occurrences, then
//            u64 offsets[2^P + 1] | n * S suffix bytes | n count bytes | n_overflow * u32 | padding to 8 bytes
// with B = 2k, P = max(0, B - 8S), key = prefix << 8S | suffix, entries strictly ascending by key; bucket p (the entries
// with that prefix) is [offsets[p], offsets[p + 1]).  A count byte 1..254 is the count, 255 says "the next value of the
// overflow list" (the counts >= 255, in entry order).
//
// save:  kt_ctr_export_stage_range -> a copy of the kept pairs, sorted (kt_sort.hip) -> tf_offsets_kernel (the boundary
//        fill), tf_pack_kernel (suffix and count bytes, a wave's bytes through LDS and out as dwords), the scan of kt_scan.hpp
//        over the counts (escape ranks -> the overflow list; its two totals are n_overflow and occurrences) -> the parts
//        come down through two page-locked slabs of SLAB bytes (one is copied while the other is written) and go to the file one after the other (on the device each part is an array of
//        its own, so that every one starts aligned; the file's packed layout is made by writing them back to back).
// load:  kt_table_file_check (the host: everything a kernel could index by) -> per section the parts go up through the same two slabs ->
//        the scan over the count bytes (escape ranks -> counts[]), a second sum over counts[] (occurrences), tf_keys_kernel
//        (a search of offsets[] per entry: no value of the file is ever used as an index) -> the flag word and the totals
//        are read back -> kt_ctr_add_pairs on the device arrays, only if the section is clean.
#include <errno.h>
#include <stdio.h>
#include <string.h>
#include <sys/stat.h>
#include <unistd.h>

#include <string>
#include <vector>

#include "kt_device.hpp"
#include "kt_internal.hpp"
#include "kt_launch.hpp"
#include "kt_scan.hpp"

namespace {

constexpr int BLOCK = SCAN_BLOCK, WAVES = BLOCK / 64;
constexpr uint32_t SELF_FILL = 4;          // boundary runs up to this long are written by the lane that owns them
constexpr size_t SLAB = (size_t)8 << 20;   // host bytes in flight between the file and the device
constexpr uint32_t FILE_HDR = 16, SEC_HDR = 32, MAX_P = 24, VERSION = 1;
const char FILE_MAGIC[4] = {'K', 'T', 'A', 'B'}, SEC_MAGIC[4] = {'K', 'S', 'E', 'C'};

// what content validation found (the flag word of a load)
constexpr uint32_t BAD_RANGE = 1u, BAD_CANON = 2u, BAD_ORDER = 4u, BAD_ZERO = 8u, BAD_OVF_VALUE = 16u, BAD_RANK = 32u,
                   BAD_OFFSET = 64u;

__device__ __forceinline__ uint64_t prefix_of(uint64_t key, uint32_t S, uint32_t P) { return P ? key >> (8u * S) : 0ull; }

// ---- pack -------------------------------------------------------------------------------------------------------------

// offsets[b] = v for b in [start, start + cnt): short runs by their lane, long ones by the whole wave, one after the other
__device__ __forceinline__ void fill_runs(uint64_t *__restrict__ offsets, uint64_t start, uint64_t cnt, uint64_t v) {
    const uint32_t lane = threadIdx.x & 63u;
    if (cnt <= SELF_FILL)
        for (uint64_t b = 0; b < cnt; b++) offsets[start + b] = v;
    uint64_t m = __ballot(cnt > SELF_FILL);
    while (m) {
        const int l = __ffsll((unsigned long long)m) - 1;
        m &= m - 1;
        const uint64_t s = __shfl(start, l, 64), c = __shfl(cnt, l, 64), x = __shfl(v, l, 64);
        for (uint64_t b = lane; b < c; b += 64u) offsets[s + b] = x;
    }
}

// The boundary fill: sorted entry i writes offsets[b] = i for every bucket b in (prefix(i - 1), prefix(i)] - entry 0 from
// bucket 0 on - and entry n - 1 closes the buckets behind its own with n.  Every boundary has exactly one writer: no atomics.
__global__ __launch_bounds__(BLOCK) void tf_offsets_kernel(const uint64_t *__restrict__ keys, uint64_t n, uint32_t S, uint32_t P,
                                                           uint64_t *__restrict__ offsets) {
    const uint64_t i = (uint64_t)blockIdx.x * BLOCK + threadIdx.x, nb = 1ull << P;
    const bool valid = i < n;
    uint64_t p = 0, lo = 0;
    if (valid) {
        p = prefix_of(keys[i], S, P);
        lo = i ? prefix_of(keys[i - 1], S, P) + 1u : 0ull;
        p = p < nb ? p : nb - 1;  // (a key of the table is below 4^k: always)
    }
    fill_runs(offsets, lo, valid && p + 1 > lo ? p + 1 - lo : 0ull, i);
    const bool last = valid && i == n - 1;
    fill_runs(offsets, p + 1, last ? nb - p : 0ull, n);
}

// Suffix bytes and count bytes.  A wave's 64 entries are 64 * S contiguous suffix bytes and 64 count bytes of the section,
// both starting at a multiple of 4: the lanes lay their bytes out in LDS and the wave stores whole dwords.  (The last
// dword of the section may carry filler bytes past n * S resp. n: the arrays have that room, the file never gets them.)
__global__ __launch_bounds__(BLOCK) void tf_pack_kernel(const uint64_t *__restrict__ keys, const uint32_t *__restrict__ counts,
                                                        uint64_t n, uint32_t S, uint32_t *__restrict__ suffix,
                                                        uint32_t *__restrict__ cbytes) {
    __shared__ uint32_t sfx[WAVES][128], cb[WAVES][16];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint64_t wave_base = (uint64_t)blockIdx.x * BLOCK + wave * 64u, i = wave_base + lane;
    const uint64_t key = i < n ? keys[i] : 0ull;
    const uint32_t c = i < n ? counts[i] : 0u;
    uint8_t *sb = (uint8_t *)sfx[wave] + lane * S;
    for (uint32_t b = 0; b < S; b++) sb[b] = (uint8_t)(key >> (8u * b));
    ((uint8_t *)cb[wave])[lane] = (uint8_t)(c < 255u ? c : 255u);
    ktd::lds_barrier();
    if (wave_base >= n) return;
    const uint32_t m = n - wave_base < 64u ? (uint32_t)(n - wave_base) : 64u;
    const uint32_t dw_s = (m * S + 3u) / 4u, dw_c = (m + 3u) / 4u;
    for (uint32_t d = lane; d < dw_s; d += 64u) suffix[wave_base / 4u * S + d] = sfx[wave][d];
    if (lane < dw_c) cbytes[wave_base / 4u + lane] = cb[wave][lane];
}

// the scan of a save: (escapes, occurrences) before entry i; an escaped entry puts its count at its rank
struct PackScan {
    const uint32_t *counts;
    uint32_t *overflow;
    __device__ __forceinline__ uint32_t word(uint64_t i) const { return counts[i]; }
    __device__ __forceinline__ void add(uint32_t c, uint64_t &a, uint64_t &b) const { a += c >= 255u, b += c; }
    __device__ __forceinline__ void put(uint64_t i, uint64_t a, uint64_t) const {
        const uint32_t c = counts[i];
        if (c >= 255u) overflow[a] = c;  // (a < the number of escapes <= n: the list has room for n)
    }
    __device__ __forceinline__ void total() const {}
};

// ---- unpack -----------------------------------------------------------------------------------------------------------

// the first scan of a load: escapes before entry i -> counts[i]; the rank is clamped before it is used
struct UnpackScan {
    const uint8_t *cbytes;
    const uint32_t *overflow;
    uint64_t n_overflow;
    uint32_t *counts, *flags;
    __device__ __forceinline__ uint32_t word(uint64_t i) const { return cbytes[i]; }
    __device__ __forceinline__ void add(uint32_t w, uint64_t &a, uint64_t &) const { a += w == 255u; }
    __device__ __forceinline__ void put(uint64_t i, uint64_t a, uint64_t) const {
        uint32_t c = cbytes[i], bad = 0;
        if (c == 0u) bad = BAD_ZERO;
        if (c == 255u) {
            if (a >= n_overflow) bad |= BAD_RANK, a = n_overflow ? n_overflow - 1 : 0;
            if (n_overflow) {
                c = overflow[a];
                if (c < 255u) bad |= BAD_OVF_VALUE;
            }
        }
        counts[i] = c;
        if (bad) atomicOr(flags, bad);
    }
    __device__ __forceinline__ void total() const {}
};

// the second: the sum of the counts (tiles' sums and their scan only)
struct SumScan {
    const uint32_t *counts;
    __device__ __forceinline__ uint32_t word(uint64_t i) const { return counts[i]; }
    __device__ __forceinline__ void add(uint32_t c, uint64_t &, uint64_t &b) const { b += c; }
};

// entry i's key: its bucket is the p with offsets[p] <= i < offsets[p + 1], found by a search over offsets[1 .. 2^P] whose
// indices never leave that interval whatever the values are
__device__ __forceinline__ uint64_t key_at(uint64_t i, const uint64_t *__restrict__ offsets, const uint8_t *__restrict__ suffix,
                                           uint64_t n, uint32_t S, uint32_t P, uint32_t &bad) {
    uint64_t lo = 1, hi = 1ull << P;  // the smallest j in [lo, hi] with offsets[j] > i (hi if there is none)
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo) / 2, o = offsets[mid];
        if (o > n) bad |= BAD_OFFSET;
        if (o > i) hi = mid; else lo = mid + 1;
    }
    uint64_t sfx = 0;
    for (uint32_t b = 0; b < S; b++) sfx |= (uint64_t)suffix[i * S + b] << (8u * b);
    return P ? ((lo - 1) << (8u * S)) | sfx : sfx;
}

__global__ __launch_bounds__(BLOCK) void tf_keys_kernel(const uint64_t *__restrict__ offsets, const uint8_t *__restrict__ suffix,
                                                        uint64_t n, uint32_t S, uint32_t P, int k, uint64_t *__restrict__ keys,
                                                        uint32_t *__restrict__ flags) {
    __shared__ uint64_t tile[BLOCK + 1];  // tile[1 + t] = thread t's key, tile[0] = the key before the tile's first
    const uint64_t i = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
    uint32_t bad = 0;
    uint64_t key = 0;
    if (i < n) {
        key = key_at(i, offsets, suffix, n, S, P, bad);
        keys[i] = key;
        if (key >> (2 * k)) bad |= BAD_RANGE;
        else if (ktd::rev_comp(key, k) < key) bad |= BAD_CANON;
        if (threadIdx.x == 0 && i) tile[0] = key_at(i - 1, offsets, suffix, n, S, P, bad);
    }
    tile[1 + threadIdx.x] = key;
    ktd::lds_barrier();
    if (i < n && i && tile[threadIdx.x] >= key) bad |= BAD_ORDER;
    if (bad) atomicOr(flags, bad);
}

// ---- host: the format -------------------------------------------------------------------------------------------------

uint32_t ceil_log2(uint64_t x) {
    uint32_t l = 0;
    while (l < 64 && (1ull << l) < x) l++;
    return l;
}

// the writer's suffix bytes for n entries of k-mers of 2k bits
uint32_t pick_S(int k, uint64_t n) {
    const uint32_t B = 2u * k, cl = ceil_log2(n ? n : 1), t = cl > 3 ? (cl - 3 < MAX_P ? cl - 3 : MAX_P) : 0;
    const uint32_t S = (B - (t < B ? t : B - 1) + 7u) / 8u;
    return S ? S : 1;
}

struct Section {
    uint32_t S = 0, P = 0;
    uint64_t n = 0, n_overflow = 0, occurrences = 0;
    uint64_t off_bytes = 0, sfx_bytes = 0, ovf_bytes = 0, pad = 0, body = 0;
};

void put32(uint8_t *p, uint32_t v) { memcpy(p, &v, 4); }
void put64(uint8_t *p, uint64_t v) { memcpy(p, &v, 8); }
uint32_t get32(const uint8_t *p) { uint32_t v; memcpy(&v, p, 4); return v; }
uint64_t get64(const uint8_t *p) { uint64_t v; memcpy(&v, p, 8); return v; }

int io_fail(const char *who, const std::string &path, const std::string &what) {
    return kt::fail(KT_ERR_IO, std::string(who) + ": " + path + ": " + what);
}

// a section header's fields and the sizes that follow from them; `room` = the file's bytes behind the header
int parse_section(const char *who, const std::string &path, const uint8_t *h, int k, uint64_t room, uint64_t index, Section *s) {
    const std::string at = "section " + std::to_string(index) + ": ";
    if (memcmp(h, SEC_MAGIC, 4)) return io_fail(who, path, at + "bad section magic");
    s->S = get32(h + 4), s->n = get64(h + 8), s->n_overflow = get64(h + 16), s->occurrences = get64(h + 24);
    if (s->S < 1 || s->S > 8) return io_fail(who, path, at + "illegal S " + std::to_string(s->S) + " (suffix bytes must be 1..8)");
    const uint32_t B = 2u * k;
    s->P = B > 8 * s->S ? B - 8 * s->S : 0;
    if (s->P > MAX_P) return io_fail(who, path, at + "P > 24 (S " + std::to_string(s->S) + " leaves a prefix of " + std::to_string(s->P) + " bits)");
    if (s->n_overflow > s->n) return io_fail(who, path, at + "n_overflow > n");
    s->off_bytes = 8 * ((1ull << s->P) + 1);
    if (s->n > room / s->S) return io_fail(who, path, at + "truncated (" + std::to_string(s->n) + " entries do not fit the file)");
    s->sfx_bytes = s->n * s->S;
    s->ovf_bytes = 4 * s->n_overflow;
    const uint64_t raw = s->off_bytes + s->sfx_bytes + s->n + s->ovf_bytes;
    s->pad = (8 - raw % 8) % 8;
    s->body = raw + s->pad;
    if (s->body > room) return io_fail(who, path, at + "truncated (the section needs " + std::to_string(s->body) + " bytes, the file has " + std::to_string(room) + ")");
    return KT_OK;
}

struct File {
    FILE *f = nullptr;
    ~File() { if (f) fclose(f); }
};

int read_at(const char *who, const std::string &path, FILE *f, uint64_t pos, void *dst, size_t bytes) {
    if (fseeko(f, (off_t)pos, SEEK_SET) || fread(dst, 1, bytes, f) != bytes) return io_fail(who, path, "read failed");
    return KT_OK;
}

// opens, checks the file header, *size = the file's bytes
int open_table_file(const char *who, const std::string &path, File *file, int *k, uint64_t *size) {
    file->f = fopen(path.c_str(), "rb");
    if (!file->f) return io_fail(who, path, std::string("cannot open: ") + strerror(errno));
    struct stat st;
    if (fstat(fileno(file->f), &st) || !S_ISREG(st.st_mode)) return io_fail(who, path, "not a regular file");
    *size = (uint64_t)st.st_size;
    uint8_t h[FILE_HDR];
    if (*size < FILE_HDR) return io_fail(who, path, "truncated (no file header)");
    if (int rc = read_at(who, path, file->f, 0, h, FILE_HDR)) return rc;
    if (memcmp(h, FILE_MAGIC, 4)) return io_fail(who, path, "bad magic (not a ktab table file)");
    if (get32(h + 4) != VERSION) return io_fail(who, path, "unsupported version " + std::to_string(get32(h + 4)));
    const uint32_t fk = get32(h + 8);
    if (fk < 1 || fk > 31 || get32(h + 12) != 0) return io_fail(who, path, "bad file header (k must be 1..31, the reserved word 0)");
    *k = (int)fk;
    return KT_OK;
}

// the walk over the section chain that info, check and the loader share: visit(section, body position)
template <class Visit>
int walk_sections(const char *who, const std::string &path, FILE *f, int k, uint64_t size, Visit &&visit) {
    uint64_t pos = FILE_HDR, index = 0;
    if (pos == size) return io_fail(who, path, "truncated (no section)");
    while (pos < size) {
        if (size - pos < SEC_HDR)
            return io_fail(who, path, index ? "trailing bytes behind section " + std::to_string(index - 1) + " (or a truncated section header)"
                                            : std::string("truncated (section header)"));
        uint8_t h[SEC_HDR];
        if (int rc = read_at(who, path, f, pos, h, SEC_HDR)) return rc;
        if (index && memcmp(h, SEC_MAGIC, 4)) return io_fail(who, path, "trailing bytes behind section " + std::to_string(index - 1));
        Section s;
        if (int rc = parse_section(who, path, h, k, size - pos - SEC_HDR, index, &s)) return rc;
        if (int rc = visit(s, pos + SEC_HDR, index)) return rc;
        pos += SEC_HDR + s.body;
        index++;
    }
    return KT_OK;
}

// offsets[] of one section: starts at 0, never decreases, never exceeds n, ends at n
int check_offsets(const char *who, const std::string &path, FILE *f, const Section &s, uint64_t body, uint64_t index) {
    const std::string at = "section " + std::to_string(index) + ": ";
    std::vector<uint64_t> buf(SLAB / 8);
    const uint64_t count = (1ull << s.P) + 1;
    uint64_t prev = 0;
    for (uint64_t j0 = 0; j0 < count; j0 += buf.size()) {
        const uint64_t m = count - j0 < buf.size() ? count - j0 : buf.size();
        if (int rc = read_at(who, path, f, body + 8 * j0, buf.data(), m * 8)) return rc;
        for (uint64_t j = 0; j < m; j++) {
            const uint64_t o = buf[j];
            if (o > s.n) return io_fail(who, path, at + "an offset > n (offsets[" + std::to_string(j0 + j) + "])");
            if (j0 + j == 0 && o != 0) return io_fail(who, path, at + "offsets[0] is not 0");
            if (o < prev) return io_fail(who, path, at + "offsets decrease at " + std::to_string(j0 + j));
            prev = o;
        }
    }
    if (prev != s.n) return io_fail(who, path, at + "the last offset is not n");
    return KT_OK;
}

int table_file_scan(const char *who, const char *path, bool full, int *k, uint64_t *sections, uint64_t *entries, uint64_t *occurrences) {
    if (!path) return kt::fail(KT_ERR_ARG, std::string(who) + ": null path");
    File file;
    int fk = 0;
    uint64_t size = 0, ns = 0, ne = 0, no = 0;
    if (int rc = open_table_file(who, path, &file, &fk, &size)) return rc;
    FILE *f = file.f;
    if (int rc = walk_sections(who, path, f, fk, size, [&](const Section &s, uint64_t body, uint64_t index) {
            ns++, ne += s.n, no += s.occurrences;
            return full ? check_offsets(who, path, f, s, body, index) : KT_OK;
        }))
        return rc;
    if (k) *k = fk;
    if (sections) *sections = ns;
    if (entries) *entries = ne;
    if (occurrences) *occurrences = no;
    return KT_OK;
}

// ---- host: save -------------------------------------------------------------------------------------------------------

// The host side of the traffic between a file and the device: two page-locked slabs of SLAB bytes and an event each, so
// that the copy of one piece runs while the file is read or written for the other, and nothing proportional to n is held.
struct Slabs {
    uint8_t *buf[2] = {nullptr, nullptr};
    hipEvent_t done[2] = {nullptr, nullptr};
    int init() {
        for (int b = 0; b < 2; b++) {
            if (hipHostMalloc((void **)&buf[b], SLAB, hipHostMallocDefault) != hipSuccess)
                return kt::fail(KT_ERR_NOMEM, "table file: cannot page-lock a staging slab");
            KT_HIP(hipEventCreateWithFlags(&done[b], hipEventDisableTiming));
        }
        return KT_OK;
    }
    ~Slabs() {
        for (int b = 0; b < 2; b++) {
            if (done[b]) (void)hipEventDestroy(done[b]);
            if (buf[b]) (void)hipHostFree(buf[b]);
        }
    }
};

// `bytes` of device memory to the file: piece i comes down while piece i - 1 is written
int down(kt_ctx *ctx, FILE *f, const void *dev, uint64_t bytes, Slabs &sl, const std::string &path) {
    size_t pending = 0;  // bytes of the piece before this one, copied (or being copied) and not yet written
    uint64_t i = 0;
    for (uint64_t at = 0; at < bytes || pending; at += SLAB, i++) {
        const int b = (int)(i & 1);
        size_t m = 0;
        if (at < bytes) {
            m = bytes - at < SLAB ? (size_t)(bytes - at) : SLAB;
            KT_HIP(hipMemcpyAsync(sl.buf[b], (const uint8_t *)dev + at, m, hipMemcpyDeviceToHost, ctx->stream));
            KT_HIP(hipEventRecord(sl.done[b], ctx->stream));
        }
        if (pending) {
            KT_HIP(hipEventSynchronize(sl.done[b ^ 1]));
            if (fwrite(sl.buf[b ^ 1], 1, pending, f) != pending)
                return io_fail("kt_ctr_save", path, std::string("write failed: ") + strerror(errno));
        }
        pending = m;
    }
    return KT_OK;
}

// `bytes` of the file at `pos` to device memory: piece i is read while piece i - 1 goes up.  Returns with copies in
// flight: the kernels that follow are queued behind them on the same stream, and the slabs are waited for before reuse.
int up(kt_ctx *ctx, FILE *f, uint64_t pos, void *dev, uint64_t bytes, Slabs &sl, uint64_t *piece, const std::string &path) {
    for (uint64_t at = 0; at < bytes; at += SLAB, ++*piece) {
        const int b = (int)(*piece & 1);
        const size_t m = bytes - at < SLAB ? (size_t)(bytes - at) : SLAB;
        if (*piece >= 2) KT_HIP(hipEventSynchronize(sl.done[b]));  // (the copy that last read this slab)
        if (int rc = read_at("kt_ctr_add_file", path, f, pos + at, sl.buf[b], m)) return rc;
        KT_HIP(hipMemcpyAsync((uint8_t *)dev + at, sl.buf[b], m, hipMemcpyHostToDevice, ctx->stream));
        KT_HIP(hipEventRecord(sl.done[b], ctx->stream));
    }
    return KT_OK;
}

dim3 blocks_for(uint64_t items, uint64_t per_block) { return dim3((uint32_t)((items + per_block - 1) / per_block)); }

// one section of the table's staged entries [lo, hi] written at the file's position
int write_section(kt_ctr *ctr, FILE *f, const std::string &path, uint64_t n) {
    kt_ctx *ctx = ctr->ctx;
    hipStream_t st = ctx->stream;
    const uint32_t S = pick_S(ctr->k, n), B = 2u * ctr->k, P = B > 8 * S ? B - 8 * S : 0;
    const uint64_t nb1 = (1ull << P) + 1, T = scan2_tiles(n);
    uint8_t hdr[SEC_HDR] = {};
    memcpy(hdr, SEC_MAGIC, 4);
    put32(hdr + 4, S), put64(hdr + 8, n);
    uint64_t n_overflow = 0, occurrences = 0, raw = 8 * nb1;
    if (n == 0) {  // offsets = {0, 0} and nothing else
        const uint8_t zero16[16] = {};
        if (fwrite(hdr, 1, SEC_HDR, f) != SEC_HDR || fwrite(zero16, 1, 16, f) != 16)
            return io_fail("kt_ctr_save", path, std::string("write failed: ") + strerror(errno));
        return KT_OK;
    }
    // BASES: the kept pairs, sorted (the staged ones may be an export target's arrays: the caller's, not to be reordered)
    uint8_t *pairs = nullptr, *parts = nullptr;
    uint64_t *keys = nullptr, *offsets = nullptr, *tiles = nullptr, *sums = nullptr;
    uint32_t *counts = nullptr, *suffix = nullptr, *cbytes = nullptr, *overflow = nullptr;
    if (int rc = ctx->claim(kt::BASES, ktl::carve_parts<16>(nullptr, &keys, n, &counts, n), "kt_ctr_save", &pairs)) return rc;
    ktl::carve_parts<16>(pairs, &keys, n, &counts, n);
    KT_HIP(hipMemcpyAsync(keys, ctr->stage.keys(), n * 8, hipMemcpyDeviceToDevice, st));
    KT_HIP(hipMemcpyAsync(counts, ctr->stage.counts(), n * 4, hipMemcpyDeviceToDevice, st));
    if (int rc = kt_sort_pairs(ctx, keys, counts, n, B)) return rc;
    ctx->unclaim(kt::OUT), ctx->unclaim(kt::AUX0);  // (the sort's; what follows is queued behind it)
    const uint64_t sfx_dw = (n * S + 3) / 4, cb_dw = (n + 3) / 4;
    const size_t part_bytes = ktl::carve_parts<16>(nullptr, &offsets, nb1, &suffix, sfx_dw, &cbytes, cb_dw, &overflow, n, &tiles, 2 * T, &sums, 2);
    if (int rc = ctx->claim(kt::AUX1, part_bytes, "kt_ctr_save", &parts)) return rc;
    ktl::carve_parts<16>(parts, &offsets, nb1, &suffix, sfx_dw, &cbytes, cb_dw, &overflow, n, &tiles, 2 * T, &sums, 2);
    const dim3 G = blocks_for(n, BLOCK), Bk(BLOCK);
    hipLaunchKernelGGL(tf_offsets_kernel, G, Bk, 0, st, (const uint64_t *)keys, n, S, P, offsets);
    hipLaunchKernelGGL(tf_pack_kernel, G, Bk, 0, st, (const uint64_t *)keys, (const uint32_t *)counts, n, S, suffix, cbytes);
    const PackScan scan{counts, overflow};
    if (int rc = scan2_sums(st, scan, n, tiles, sums, sums + 1)) return rc;
    if (int rc = scan2_apply(st, scan, n, tiles)) return rc;
    uint64_t h_sums[2] = {0, 0};
    KT_HIP(hipMemcpyAsync(h_sums, sums, 16, hipMemcpyDeviceToHost, st));
    KT_HIP(hipStreamSynchronize(st));
    n_overflow = h_sums[0], occurrences = h_sums[1];
    if (n_overflow > n) return kt::fail(KT_ERR_HIP, "kt_ctr_save: internal: more escapes than entries");
    put64(hdr + 16, n_overflow), put64(hdr + 24, occurrences);
    if (fwrite(hdr, 1, SEC_HDR, f) != SEC_HDR) return io_fail("kt_ctr_save", path, std::string("write failed: ") + strerror(errno));
    Slabs slab;
    if (int rc = slab.init()) return rc;
    if (int rc = down(ctx, f, offsets, 8 * nb1, slab, path)) return rc;
    if (int rc = down(ctx, f, suffix, n * S, slab, path)) return rc;
    if (int rc = down(ctx, f, cbytes, n, slab, path)) return rc;
    if (int rc = down(ctx, f, overflow, 4 * n_overflow, slab, path)) return rc;
    raw += n * S + n + 4 * n_overflow;
    const uint8_t zeros[8] = {};
    const size_t pad = (size_t)((8 - raw % 8) % 8);
    if (pad && fwrite(zeros, 1, pad, f) != pad) return io_fail("kt_ctr_save", path, std::string("write failed: ") + strerror(errno));
    return KT_OK;
}

const char *content_error(uint32_t flags) {
    if (flags & BAD_OFFSET) return "an offset > n";
    if (flags & BAD_ZERO) return "a zero count byte";
    if (flags & BAD_RANK) return "more escapes than n_overflow";
    if (flags & BAD_OVF_VALUE) return "an overflow value < 255";
    if (flags & BAD_RANGE) return "a key >= 4^k";
    if (flags & BAD_CANON) return "a non-canonical key";
    if (flags & BAD_ORDER) return "keys not strictly ascending";
    return "unknown";
}

// one section into the table: BASES / OFFSETS = keys / counts, OUT = the section's parts (the buffers kt_ctr_add_pairs and
// what it calls leave alone)
int load_section(kt_ctr *ctr, FILE *f, const std::string &path, const Section &s, uint64_t body, uint64_t index,
                 Slabs &slab, uint64_t *piece) {
    kt_ctx *ctx = ctr->ctx;
    hipStream_t st = ctx->stream;
    const uint64_t n = s.n, nb1 = (1ull << s.P) + 1, T = scan2_tiles(n);
    uint8_t *parts = nullptr, *suffix = nullptr, *cbytes = nullptr;
    uint64_t *keys = nullptr, *offsets = nullptr, *tiles = nullptr, *sums = nullptr;
    uint32_t *counts = nullptr, *overflow = nullptr, *flags = nullptr;
    if (int rc = ctx->claim(kt::BASES, n * 8, "kt_ctr_add_file", &keys)) return rc;
    if (int rc = ctx->claim(kt::OFFSETS, n * 4, "kt_ctr_add_file", &counts)) return rc;
    const size_t part_bytes = ktl::carve_parts<16>(nullptr, &offsets, nb1, &suffix, s.sfx_bytes, &cbytes, n, &overflow, s.n_overflow + 1,
                                                   &tiles, 2 * T, &sums, 4, &flags, 4);
    if (int rc = ctx->claim(kt::OUT, part_bytes, "kt_ctr_add_file", &parts)) return rc;
    ktl::carve_parts<16>(parts, &offsets, nb1, &suffix, s.sfx_bytes, &cbytes, n, &overflow, s.n_overflow + 1, &tiles, 2 * T, &sums, 4, &flags, 4);
    uint64_t pos = body;
    if (int rc = up(ctx, f, pos, offsets, s.off_bytes, slab, piece, path)) return rc;
    pos += s.off_bytes;
    if (int rc = up(ctx, f, pos, suffix, s.sfx_bytes, slab, piece, path)) return rc;
    pos += s.sfx_bytes;
    if (int rc = up(ctx, f, pos, cbytes, n, slab, piece, path)) return rc;
    pos += n;
    if (int rc = up(ctx, f, pos, overflow, s.ovf_bytes, slab, piece, path)) return rc;
    KT_HIP(hipMemsetAsync(sums, 0, 48, st));  // (the four sums and the flag word behind them)
    const dim3 G = blocks_for(n, BLOCK), Bk(BLOCK);
    const UnpackScan scan{cbytes, overflow, s.n_overflow, counts, flags};
    if (int rc = scan2_sums(st, scan, n, tiles, sums, sums + 1)) return rc;
    if (int rc = scan2_apply(st, scan, n, tiles)) return rc;
    if (int rc = scan2_sums(st, SumScan{counts}, n, tiles, sums + 2, sums + 3)) return rc;
    hipLaunchKernelGGL(tf_keys_kernel, G, Bk, 0, st, (const uint64_t *)offsets, (const uint8_t *)suffix, n, s.S, s.P, ctr->k, keys, flags);
    KT_HIP(hipGetLastError());
    uint64_t h[6] = {};
    KT_HIP(hipMemcpyAsync(h, sums, 48, hipMemcpyDeviceToHost, st));
    KT_HIP(hipStreamSynchronize(st));
    const uint32_t bad = (uint32_t)h[4];  // (sums is 16-aligned and takes 32 bytes: flags starts at sums + 4)
    const std::string at = "section " + std::to_string(index) + ": ";
    if (bad) return io_fail("kt_ctr_add_file", path, at + content_error(bad) + " (nothing of this section was added)");
    if (h[0] != s.n_overflow)
        return io_fail("kt_ctr_add_file", path, at + "fewer escapes than n_overflow (" + std::to_string(h[0]) + " of " +
                                                    std::to_string(s.n_overflow) + "; nothing of this section was added)");
    if (h[3] != s.occurrences)
        return io_fail("kt_ctr_add_file", path, at + "the counts sum to " + std::to_string(h[3]) + ", the header's occurrences say " +
                                                    std::to_string(s.occurrences) + " (nothing of this section was added)");
    return kt_ctr_add_pairs(ctr, keys, counts, n, KT_MEM_DEVICE);
}

}  // namespace

extern "C" {

int kt_table_file_info(const char *path, int *k, uint64_t *sections, uint64_t *entries, uint64_t *occurrences) {
    return table_file_scan("kt_table_file_info", path, false, k, sections, entries, occurrences);
}

int kt_table_file_check(const char *path) {
    return table_file_scan("kt_table_file_check", path, true, nullptr, nullptr, nullptr, nullptr);
}

int kt_ctr_save(kt_ctr *ctr, const char *path, uint32_t min_count, uint32_t max_count, int append, uint64_t *n_saved) {
    if (!ctr || !path) return kt::fail(KT_ERR_ARG, "kt_ctr_save: null");
    if (min_count > max_count) return kt::fail(KT_ERR_ARG, "kt_ctr_save: min_count > max_count");
    kt_ctx *ctx = ctr->ctx;
    kt::ClaimScope scope(ctx);
    if (int rc = ctx->use()) return rc;
    const std::string dst(path);
    struct stat sb;
    const bool grow = append && stat(path, &sb) == 0;
    uint64_t old_size = 0;
    if (grow) {  // the file must be a table file of this k, whole
        int fk = 0;
        if (int rc = table_file_scan("kt_ctr_save", path, false, &fk, nullptr, nullptr, nullptr)) return rc;
        if (fk != ctr->k)
            return kt::fail(KT_ERR_ARG, "kt_ctr_save: " + dst + " holds k = " + std::to_string(fk) + ", the table k = " + std::to_string(ctr->k));
        old_size = (uint64_t)sb.st_size;
    }
    uint64_t n = 0;
    if (int rc = kt_ctr_export_stage_range(ctr, min_count, max_count, &n)) return rc;  // (KT_ERR_FULL: an overflowed table)
    const std::string tmp = dst + ".tmp" + std::to_string((long)getpid());
    File file;
    file.f = fopen(grow ? path : tmp.c_str(), grow ? "r+b" : "wb");
    if (!file.f) return io_fail("kt_ctr_save", grow ? dst : tmp, std::string("cannot open for writing: ") + strerror(errno));
    int rc = KT_OK;
    if (grow) {
        if (fseeko(file.f, 0, SEEK_END)) rc = io_fail("kt_ctr_save", dst, "seek failed");
    } else {
        uint8_t h[FILE_HDR] = {};
        memcpy(h, FILE_MAGIC, 4);
        put32(h + 4, VERSION), put32(h + 8, (uint32_t)ctr->k);
        if (fwrite(h, 1, FILE_HDR, file.f) != FILE_HDR) rc = io_fail("kt_ctr_save", tmp, std::string("write failed: ") + strerror(errno));
    }
    if (!rc) rc = write_section(ctr, file.f, dst, n);
    if (!rc && fflush(file.f)) rc = io_fail("kt_ctr_save", dst, std::string("write failed: ") + strerror(errno));
    if (rc) {  // no partial section stays behind
        const std::string msg = kt_last_error();
        if (grow) {
            (void)fflush(file.f);
            (void)!ftruncate(fileno(file.f), (off_t)old_size);
        } else {
            (void)unlink(tmp.c_str());
        }
        kt::set_error(msg);
        return rc;
    }
    {   // a write error may only show now (a quota, a network file system): the file is not finished before this succeeds
        const bool synced = fsync(fileno(file.f)) == 0;
        const bool closed = fclose(file.f) == 0;
        file.f = nullptr;
        if (!synced || !closed) {
            const int e = errno;
            if (grow) (void)!truncate(path, (off_t)old_size);
            else (void)unlink(tmp.c_str());
            return io_fail("kt_ctr_save", dst, std::string("write failed at close: ") + strerror(e));
        }
    }
    if (!grow && rename(tmp.c_str(), path)) {
        const int e = errno;
        (void)unlink(tmp.c_str());
        return io_fail("kt_ctr_save", dst, std::string("cannot rename the finished file into place: ") + strerror(e));
    }
    if (n_saved) *n_saved = n;
    return KT_OK;
}

int kt_ctr_add_file(kt_ctr *ctr, const char *path, uint64_t *n_added) {
    if (!ctr || !path) return kt::fail(KT_ERR_ARG, "kt_ctr_add_file: null");
    if (n_added) *n_added = 0;
    kt_ctx *ctx = ctr->ctx;
    kt::ClaimScope scope(ctx);
    if (int rc = ctx->use()) return rc;
    int fk = 0;
    uint64_t size = 0, added = 0;
    if (int rc = table_file_scan("kt_ctr_add_file", path, true, &fk, nullptr, nullptr, nullptr)) return rc;
    if (fk != ctr->k)
        return kt::fail(KT_ERR_ARG, std::string("kt_ctr_add_file: ") + path + " holds k = " + std::to_string(fk) + ", the table k = " + std::to_string(ctr->k));
    File file;
    if (int rc = open_table_file("kt_ctr_add_file", path, &file, &fk, &size)) return rc;
    Slabs slab;
    if (int rc = slab.init()) return rc;
    uint64_t piece = 0;  // pieces sent up so far, over all sections: which slab is next
    FILE *f = file.f;
    const std::string p(path);
    int rc = walk_sections("kt_ctr_add_file", p, f, fk, size, [&](const Section &s, uint64_t body, uint64_t index) {
        if (s.n == 0) return (int)KT_OK;
        scope.reset();  // (the section before this one ended with a wait for the stream)
        if (int r = load_section(ctr, f, p, s, body, index, slab, &piece)) return r;
        KT_HIP(hipStreamSynchronize(ctx->stream));  // (the next section's parts go into the buffers the add reads)
        added += s.n;
        if (n_added) *n_added = added;
        return (int)KT_OK;
    });
    return rc;
}

}  // extern "C"
