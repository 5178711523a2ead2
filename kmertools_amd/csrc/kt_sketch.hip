// kt_sketch.hip - bottom-s MinHash sketches of the reads of a CSR batch (kt_sketch_batch), bottom-s of unions of sketches
// (kt_sketch_merge) and the all-pairs Mash merge walk over two sets of sketches (kt_sketch_pairs).
//
// A window's hash is mix64(canonical k-mer ^ seed); a sketch is the s smallest DISTINCT hashes of a read, ascending.  No
// threshold is ever guessed from counts with multiplicity: everything below is "sort, drop equal neighbours, keep the
// first s", which is exact whatever repeats a read holds (poly-A, tandem repeats), and "bottom-s of a union of bottom-s
// sets is the bottom-s of the union", which makes the pieces of a long read combinable.
//
//   sketch_segment_kernel   one workgroup per 8192-base segment of the ktseg front end, whatever the reads are.  The
//                           segment's windows become (piece, hash) pairs in LDS - a PIECE is what one read has inside
//                           the segment, numbered by the read starts in front of it - and are sorted by a bitonic
//                           network (8192 pairs, 91 steps).  Equal neighbours are dropped, a segmented rank follows
//                           from one prefix sum, and the first s of every piece are written: to the read's row of the
//                           output when the read lies inside the segment (then the row is final: 150-base reads and
//                           5000-base contigs end here), to one of the segment's two SLOTS when it does not (at most
//                           two reads cross a segment's edges: the one that began before it and the one that goes on
//                           behind it).  So one sequence of 80 Mbases is 9766 workgroups, and 100 000 sequences of 5 kb
//                           are 61 036.
//   sketch_tree_kernel      the slots of a read that spans P segments are merged pairwise, piece p with piece p + d for
//                           d = 1, 2, 4, ...: ceil(log2 P) launches, every merge a workgroup of its own, the last one of
//                           a read writes its row.  (merge2: an element's place in the union is its index in its own list
//                           plus its lower bound in the other minus the common elements in front of it.)
//   sketch_group_kernel     the same tree over the rows of a group (kt_sketch_merge).
//   sketch_pairs_kernel     a row of A in LDS (up to 128 KiB), a wave per row of B: every lane finds the lower bound of one
//                           element of B in A; matches before it come from a ballot.  A match's rank in the union is
//                           (index in B) + (lower bound in A) - (matches before); shared = matches of rank < s - all of
//                           them when the union has at most s elements -, denom = min(s, |A| + |B| - matches).
// Integer atomics only (the window counts of the pieces of a spanning read are added up); the outputs are a function of
// the inputs alone.
#include "kt_internal.hpp"
#include "kt_launch.hpp"

namespace {

using ktseg::SEG;
constexpr uint32_t BLOCK = ktseg::BLOCK;
constexpr uint32_t WAVE = 64, WAVES = BLOCK / WAVE, CHUNKS = SEG / BLOCK;
constexpr uint32_t NOPIECE = 0xFFFFu;  // the piece of a window that is no k-mer: sorts behind every piece (there are at most 8192)
constexpr uint64_t NOREAD = ~0ull;     // the read of a slot that holds nothing
constexpr uint32_t MAX_S = KT_SKETCH_MAX_S;

struct BatchOut {
    uint64_t *hashes;   // n_reads * s
    uint32_t *sizes;    // n_reads
    uint32_t *n_kmers;  // n_reads or null; zeroed before the launch (spanning reads add to it)
    uint32_t s;
};

// two per segment: 2g = the read that began before segment g, 2g + 1 = the read that begins in it and goes on behind it
struct Slots {
    uint64_t *buf;   // 2 * n_seg rows of s
    uint32_t *size;  // 2 * n_seg
};

struct SortShared {
    uint64_t hk[SEG];     // the hashes
    uint32_t pinfo[SEG];  // per piece: (index of its first pair << 16) | distinct pairs in front of it; later (windows << 16) | size
    uint32_t prid[SEG];   // per piece: its read, relative to the segment's first
    uint16_t pc[SEG];     // the pieces of the pairs
};
union SegmentShared {
    ktseg::SegShared seg;
    SortShared srt;
};

__global__ __launch_bounds__(BLOCK) void max_len_kernel(const uint64_t *__restrict__ offsets, uint64_t n_reads, uint64_t *max_len) {
    uint64_t m = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * BLOCK + threadIdx.x; i < n_reads; i += (uint64_t)gridDim.x * BLOCK) {
        const uint64_t len = offsets[i + 1] - offsets[i];
        m = len > m ? len : m;
    }
    if (m) atomicMax((unsigned long long *)max_len, (unsigned long long)m);
}

// the rows of the reads without a base: no segment holds them
__global__ __launch_bounds__(BLOCK) void empty_reads_kernel(const uint64_t *__restrict__ offsets, uint64_t n_reads, BatchOut o) {
    for (uint64_t i = (uint64_t)blockIdx.x * BLOCK + threadIdx.x; i < n_reads; i += (uint64_t)gridDim.x * BLOCK) {
        if (offsets[i + 1] != offsets[i]) continue;
        o.sizes[i] = 0;
        for (uint32_t t = 0; t < o.s; t++) o.hashes[i * o.s + t] = KT_EMPTY_KEY;
    }
}

__global__ __launch_bounds__(BLOCK) void sketch_segment_kernel(ktseg::SegArgs a, uint64_t seed, BatchOut o, Slots sl, uint64_t *slot_rid) {
    __shared__ SegmentShared sm;
    __shared__ uint32_t wsum[WAVES];
    __shared__ uint64_t s_first;
    const uint32_t tid = threadIdx.x, s = o.s;
    const uint64_t total = a.offsets[a.n_reads];
    for (uint64_t g = blockIdx.x; g < a.n_seg; g += gridDim.x) {
        const uint64_t B0 = g * SEG;
        uint64_t keys[ktseg::PER_THREAD];
        uint32_t ok;
        ktseg::collect_kmers(a, g, sm.seg, keys, ok);  // (window start 32 tid + j; the staged segment stays until it is overwritten below)

        // ---- pieces: positions [1, lim) of the segment where a read starts, in front of each window ----------------
        const uint32_t lim = total - B0 < SEG ? (uint32_t)(total - B0) : SEG;  // positions that hold a base (>= 1)
        const uint32_t p0 = 32u * tid;
        uint32_t bw = sm.seg.bnd[tid];
        if (tid == 0) bw &= ~1u;
        if (p0 >= lim) bw = 0;
        else if (lim - p0 < 32u) bw &= (1u << (lim - p0)) - 1u;
        ktseg::ReadCursor cur(a.offsets, a.seg_first, g, p0 < lim ? B0 + p0 : B0);
        if (tid == 0) s_first = cur.rid;
        uint32_t npieces;
        const uint32_t qbase = ktd::block_excl_scan<WAVES>((uint32_t)__popc(bw), wsum, &npieces);  // (barriers: the staged masks are read)
        npieces += 1;
        const uint64_t r_first = s_first;

        // ---- the pairs, window j of thread tid at j * 256 + tid (their order does not matter to a sort) ----------
        for (uint32_t i = tid; i < SEG; i += BLOCK) sm.srt.pinfo[i] = 0;
        if (tid == 0) sm.srt.prid[0] = 0;
        for (uint32_t m = bw; m; m &= m - 1) {
            const uint32_t j = (uint32_t)__ffs((int)m) - 1u;
            cur.advance(B0 + p0 + j);
            sm.srt.prid[qbase + (uint32_t)__popc(bw & ((2u << j) - 1u))] = (uint32_t)(cur.rid - r_first);
        }
#pragma unroll
        for (uint32_t j = 0; j < ktseg::PER_THREAD; j++) {
            const bool v = (ok >> j) & 1u;
            sm.srt.hk[j * BLOCK + tid] = v ? ktd::mix64(keys[j] ^ seed) : ~0ull;
            sm.srt.pc[j * BLOCK + tid] = (uint16_t)(v ? qbase + (uint32_t)__popc(bw & ((2u << j) - 1u)) : NOPIECE);
        }
        ktd::lds_barrier();

        // ---- bitonic sort by (piece, hash) ------------------------------------------------------------------------
        for (uint32_t k2 = 2; k2 <= SEG; k2 <<= 1) {
            for (uint32_t j = k2 >> 1; j > 0; j >>= 1) {
#pragma unroll 4
                for (uint32_t t = tid; t < SEG / 2; t += BLOCK) {
                    const uint32_t i = ((t & ~(j - 1u)) << 1) | (t & (j - 1u)), l = i | j;
                    const bool up = (i & k2) == 0;
                    const uint64_t hi = sm.srt.hk[i], hl = sm.srt.hk[l];
                    const uint32_t ci = sm.srt.pc[i], cl = sm.srt.pc[l];
                    const bool gt = ci > cl || (ci == cl && hi > hl);
                    if (gt == up) {
                        sm.srt.hk[i] = hl, sm.srt.hk[l] = hi;
                        sm.srt.pc[i] = (uint16_t)cl, sm.srt.pc[l] = (uint16_t)ci;
                    }
                }
                ktd::lds_barrier();
            }
        }

        // ---- distinct pairs and their rank: thread tid looks at pair c * 256 + tid of chunk c ----------------------
        uint32_t ex[CHUNKS];  // distinct pairs in front of mine
        uint32_t fl = 0;      // bit c: mine is the first of its (piece, hash)
        uint32_t carry = 0;
#pragma unroll
        for (uint32_t c = 0; c < CHUNKS; c++) {
            const uint32_t i = c * BLOCK + tid;
            const uint32_t q = sm.srt.pc[i];
            const bool valid = q != NOPIECE;
            const bool new_piece = valid && (i == 0 || sm.srt.pc[i - 1] != q);
            const bool first = valid && (new_piece || sm.srt.hk[i - 1] != sm.srt.hk[i]);
            uint32_t tot;
            ex[c] = carry + ktd::block_excl_scan<WAVES>(first ? 1u : 0u, wsum, &tot);
            carry += tot;
            fl |= (first ? 1u : 0u) << c;
            if (new_piece) sm.srt.pinfo[q] = (i << 16) | ex[c];
        }
        ktd::lds_barrier();

        // which pieces are not whole reads: the first one when its read began before the segment, the last one when its
        // read goes on behind it
        const uint64_t r_last = r_first + sm.srt.prid[npieces - 1];
        const bool head_span = a.offsets[r_first] < B0;
        const bool tail_span = a.offsets[r_last + 1] > B0 + SEG;
        auto spans = [&](uint32_t q) { return (q == 0 && head_span) || (q == npieces - 1 && tail_span); };
        auto slot_of = [&](uint32_t q) { return 2 * g + ((q == 0 && head_span) ? 0u : 1u); };

#pragma unroll
        for (uint32_t c = 0; c < CHUNKS; c++) {
            if (!((fl >> c) & 1u)) continue;
            const uint32_t i = c * BLOCK + tid;
            const uint32_t q = sm.srt.pc[i];
            const uint32_t rank = ex[c] - (sm.srt.pinfo[q] & 0xFFFFu);
            if (rank >= s) continue;
            uint64_t *dst = spans(q) ? sl.buf + slot_of(q) * s : o.hashes + (r_first + sm.srt.prid[q]) * s;
            dst[rank] = sm.srt.hk[i];
        }
        ktd::lds_barrier();
        // the last pair of a piece leaves (windows << 16) | size
#pragma unroll
        for (uint32_t c = 0; c < CHUNKS; c++) {
            const uint32_t i = c * BLOCK + tid;
            const uint32_t q = sm.srt.pc[i];
            if (q == NOPIECE || (i + 1 < SEG && sm.srt.pc[i + 1] == q)) continue;
            const uint32_t info = sm.srt.pinfo[q];
            const uint32_t distinct = ex[c] + ((fl >> c) & 1u) - (info & 0xFFFFu);
            sm.srt.pinfo[q] = ((i - (info >> 16) + 1u) << 16) | (distinct < s ? distinct : s);
        }
        ktd::lds_barrier();

        // ---- sizes, window counts, the rest of the rows ---------------------------------------------------------------
        for (uint32_t q = tid; q < npieces; q += BLOCK) {
            const uint64_t r = r_first + sm.srt.prid[q];
            const uint32_t info = sm.srt.pinfo[q];
            if (spans(q)) {
                sl.size[slot_of(q)] = info & 0xFFFFu;
                slot_rid[slot_of(q)] = r;
                if (o.n_kmers && (info >> 16)) atomicAdd(&o.n_kmers[r], info >> 16);
            } else {
                o.sizes[r] = info & 0xFFFFu;
                if (o.n_kmers) o.n_kmers[r] = info >> 16;
            }
        }
        if (tid == 0) {
            if (!head_span) slot_rid[2 * g] = NOREAD;
            if (!(tail_span && !(npieces == 1 && head_span))) slot_rid[2 * g + 1] = NOREAD;
        }
        for (uint64_t idx = tid; idx < (uint64_t)npieces * s; idx += BLOCK) {
            const uint32_t q = (uint32_t)(idx / s), t = (uint32_t)(idx % s);
            if (spans(q) || t < (sm.srt.pinfo[q] & 0xFFFFu)) continue;
            o.hashes[(r_first + sm.srt.prid[q]) * s + t] = KT_EMPTY_KEY;
        }
        ktd::lds_barrier();  // LDS is reused by the next segment
    }
}

// out[0, *out_size) = the s smallest of the union of X[0, nx) and Y[0, ny), both strictly ascending; out is neither of
// them.  Called by the whole workgroup with the same arguments.  cm: MAX_S + 1 entries of LDS.
__device__ __forceinline__ void merge2(const uint64_t *X, uint32_t nx, const uint64_t *Y, uint32_t ny, uint32_t s, uint64_t *out,
                                       uint32_t *out_size, bool pad, uint16_t *cm, uint32_t *wsum) {
    const uint32_t tid = threadIdx.x;
    uint32_t carry = 0;  // elements of X in front of the chunk that Y holds too
    for (uint32_t c0 = 0; c0 < nx; c0 += BLOCK) {
        const uint32_t i = c0 + tid;
        const bool act = i < nx;
        uint64_t x = 0;
        uint32_t lb = 0;
        bool m = false;
        if (act) {
            x = X[i];
            lb = ktd::lower_bound(Y, ny, x);
            m = lb < ny && Y[lb] == x;
        }
        uint32_t tot;
        const uint32_t mb = carry + ktd::block_excl_scan<WAVES>(m ? 1u : 0u, wsum, &tot);
        carry += tot;
        if (act) {
            cm[i] = (uint16_t)mb;
            const uint32_t rank = i + lb - mb;
            if (rank < s) out[rank] = x;
        }
    }
    if (tid == 0) cm[nx] = (uint16_t)carry;
    ktd::lds_barrier();
    for (uint32_t j = tid; j < ny; j += BLOCK) {
        const uint64_t y = Y[j];
        const uint32_t lb = ktd::lower_bound(X, nx, y);
        if (lb < nx && X[lb] == y) continue;  // (written from X)
        const uint32_t rank = j + lb - cm[lb];
        if (rank < s) out[rank] = y;
    }
    const uint32_t uni = nx + ny - carry, size = uni < s ? uni : s;
    if (tid == 0) *out_size = size;
    if (pad)
        for (uint32_t t = size + tid; t < s; t += BLOCK) out[t] = KT_EMPTY_KEY;
    ktd::lds_barrier();  // cm is rewritten by the next merge
}

// round d of the tree over the pieces of the reads that span segments: piece p (a multiple of 2d) takes in piece p + d
__global__ __launch_bounds__(BLOCK) void sketch_tree_kernel(const uint64_t *__restrict__ offsets, const uint64_t *__restrict__ slot_rid,
                                                            uint64_t n_slots, Slots in, Slots outb, BatchOut o, uint64_t d) {
    __shared__ uint16_t cm[MAX_S + 1];
    __shared__ uint32_t wsum[WAVES];
    for (uint64_t slot = blockIdx.x; slot < n_slots; slot += gridDim.x) {
        const uint64_t rid = slot_rid[slot];
        if (rid == NOREAD) continue;
        const uint64_t o0 = offsets[rid], o1 = offsets[rid + 1];
        const uint64_t g0 = o0 / SEG, p = (slot >> 1) - g0, P = (o1 - 1) / SEG - g0 + 1;
        if (p & (2 * d - 1)) continue;   // taken in by another piece, now or earlier
        if (d > 1 && d >= P) continue;   // the read was finished by an earlier round
        const bool has = p + d < P, last = 2 * d >= P;
        const uint64_t other = 2 * (g0 + p + d);
        merge2(in.buf + slot * o.s, in.size[slot], in.buf + (has ? other : slot) * o.s, has ? in.size[other] : 0u, o.s,
               last ? o.hashes + rid * o.s : outb.buf + slot * o.s, last ? o.sizes + rid : outb.size + slot, last, cm, wsum);
    }
}

// group_offsets[0 .. n_groups] must not decrease and must end at or below n: *bad = 1 otherwise; *max_rows = the largest group
__global__ __launch_bounds__(BLOCK) void group_check_kernel(const uint64_t *__restrict__ go, uint64_t n_groups, uint64_t n,
                                                            uint32_t *bad, uint64_t *max_rows) {
    for (uint64_t g = (uint64_t)blockIdx.x * BLOCK + threadIdx.x; g < n_groups; g += (uint64_t)gridDim.x * BLOCK) {
        const uint64_t lo = go[g], hi = go[g + 1];
        if (hi < lo || hi > n) *bad = 1u;
        else if (hi - lo) atomicMax((unsigned long long *)max_rows, (unsigned long long)(hi - lo));
    }
}

__global__ __launch_bounds__(BLOCK) void empty_groups_kernel(const uint64_t *__restrict__ go, uint64_t n_groups, uint32_t s,
                                                             uint64_t *out_hashes, uint32_t *out_sizes) {
    for (uint64_t g = blockIdx.x; g < n_groups; g += gridDim.x) {
        if (go[g] != go[g + 1]) continue;
        if (threadIdx.x == 0) out_sizes[g] = 0;
        for (uint32_t t = threadIdx.x; t < s; t += BLOCK) out_hashes[g * s + t] = KT_EMPTY_KEY;
    }
}

// round d of the same tree over the rows of every group: row p of its group (a multiple of 2d) takes in row p + d
__global__ __launch_bounds__(BLOCK) void sketch_group_kernel(const uint64_t *__restrict__ go, uint64_t n_groups, const uint64_t *in_h,
                                                             const uint32_t *in_sz, uint64_t *mid_h, uint32_t *mid_sz,
                                                             uint64_t *out_hashes, uint32_t *out_sizes, uint32_t s, uint64_t d) {
    __shared__ uint16_t cm[MAX_S + 1];
    __shared__ uint32_t wsum[WAVES];
    const uint64_t t0 = go[0], t1 = go[n_groups];
    for (uint64_t t = t0 + blockIdx.x; t < t1; t += gridDim.x) {
        // the group that holds row t: the last g with go[g] <= t (empty groups in front of it share its start)
        uint64_t lo = 0, hi = n_groups;  // go[lo] <= t < go[hi]
        while (hi - lo > 1) {
            const uint64_t mid = (lo + hi) >> 1;
            if (go[mid] <= t) lo = mid; else hi = mid;
        }
        const uint64_t p = t - go[lo], P = go[lo + 1] - go[lo];
        if (p & (2 * d - 1)) continue;
        if (d > 1 && d >= P) continue;
        const bool has = p + d < P, last = 2 * d >= P;
        const uint32_t nx = in_sz[t] < s ? in_sz[t] : s;
        uint32_t ny = 0;
        if (has) ny = in_sz[t + d] < s ? in_sz[t + d] : s;
        merge2(in_h + t * s, nx, in_h + (has ? t + d : t) * s, ny, s, last ? out_hashes + lo * s : mid_h + t * s,
               last ? out_sizes + lo : mid_sz + t, last, cm, wsum);
    }
}

template <uint32_t CAP>
__global__ __launch_bounds__(BLOCK) void sketch_pairs_kernel(const uint64_t *__restrict__ A, const uint32_t *__restrict__ asz, uint64_t n_a,
                                                             const uint64_t *__restrict__ B, const uint32_t *__restrict__ bsz, uint64_t n_b,
                                                             uint32_t s, uint32_t *__restrict__ shared, uint32_t *__restrict__ denom) {
    __shared__ uint64_t arow[CAP];
    const uint32_t tid = threadIdx.x, lane = tid & (WAVE - 1), wave = tid / WAVE;
    for (uint64_t i = blockIdx.x; i < n_a; i += gridDim.x) {
        const uint32_t na = asz[i] < s ? asz[i] : s;
        for (uint32_t t = tid; t < na; t += BLOCK) arow[t] = A[i * s + t];
        ktd::lds_barrier();
        for (uint64_t j = (uint64_t)blockIdx.y * WAVES + wave; j < n_b; j += (uint64_t)gridDim.y * WAVES) {
            const uint32_t nb = bsz[j] < s ? bsz[j] : s;
            const uint64_t *brow = B + j * s;
            uint32_t common = 0, cnt = 0;
            for (uint32_t c0 = 0; c0 < nb; c0 += WAVE) {  // (the same trip count for every lane: the ballots want them all)
                const uint32_t e = c0 + lane;
                uint32_t lb = 0;
                bool m = false;
                if (e < nb) {
                    const uint64_t y = brow[e];
                    lb = ktd::lower_bound(arow, na, y);
                    m = lb < na && arow[lb] == y;
                }
                const uint64_t bal = __ballot(m);
                const uint32_t before = common + (uint32_t)__popcll(bal & ((1ull << lane) - 1ull));
                cnt += (uint32_t)__popcll(__ballot(m && e + lb - before < s));
                common += (uint32_t)__popcll(bal);
            }
            if (lane == 0) {
                shared[i * n_b + j] = cnt;
                if (denom) {
                    const uint32_t uni = na + nb - common;
                    denom[i * n_b + j] = uni < s ? uni : s;
                }
            }
        }
        ktd::lds_barrier();  // the row is replaced
    }
}

}  // namespace

using namespace ktl;

// the sketches of a device-resident batch into device arrays; max_len = the longest read
static int sketch_device(kt_ctx *ctx, const uint8_t *bases, const uint64_t *offsets, uint64_t n_reads, uint64_t total,
                         uint64_t max_len, int k, uint64_t seed, const BatchOut &o) {
    if (o.n_kmers) KT_HIP(hipMemsetAsync(o.n_kmers, 0, n_reads * 4, ctx->stream));
    hipLaunchKernelGGL(empty_reads_kernel, dim3(grid_for(ctx, (n_reads + BLOCK - 1) / BLOCK, 8)), dim3(BLOCK), 0, ctx->stream, offsets,
                       n_reads, o);
    KT_HIP(hipGetLastError());
    if (!total) return KT_OK;
    ktseg::SegArgs a;
    if (int rc = make_seg_args(ctx, bases, offsets, n_reads, total, k, &a)) return rc;
    // segments a read can touch, and the rounds that merge so many pieces
    const uint64_t max_pieces = max_len ? (max_len + SEG - 2) / SEG + 1 : 0;
    uint32_t rounds = 0;
    while ((1ull << rounds) < max_pieces) rounds++;
    const uint64_t n_slots = 2 * a.n_seg;
    const uint64_t buf_bytes = n_slots * o.s * 8, all_bytes = buf_bytes + n_slots * 4;
    char *p0 = nullptr, *p1 = nullptr;  // (p1 stays null when a single round never writes the second set of slots)
    if (int rc = ctx->claim(kt::AUX1, all_bytes + n_slots * 8, "kt_sketch_batch", &p0)) return rc;
    if (rounds >= 2)
        if (int rc = ctx->claim(kt::AUX2, all_bytes, "kt_sketch_batch", &p1)) return rc;
    Slots s0{(uint64_t *)p0, (uint32_t *)(p0 + buf_bytes + n_slots * 8)};
    uint64_t *slot_rid = (uint64_t *)(p0 + buf_bytes);
    Slots s1{(uint64_t *)p1, (uint32_t *)(p1 + buf_bytes)};
    const uint32_t seg_grid = (uint32_t)(a.n_seg < (1u << 20) ? a.n_seg : (1u << 20));
    hipLaunchKernelGGL(sketch_segment_kernel, dim3(seg_grid), dim3(BLOCK), 0, ctx->stream, a, seed, o, s0, slot_rid);
    KT_HIP(hipGetLastError());
    const uint32_t tree_grid = (uint32_t)(n_slots < (1u << 20) ? n_slots : (1u << 20));
    for (uint32_t r = 0; r < rounds; r++) {
        hipLaunchKernelGGL(sketch_tree_kernel, dim3(tree_grid), dim3(BLOCK), 0, ctx->stream, offsets, (const uint64_t *)slot_rid,
                           n_slots, (r & 1u) ? s1 : s0, (r & 1u) ? s0 : s1, o, 1ull << r);
        KT_HIP(hipGetLastError());
    }
    return KT_OK;
}

extern "C" int kt_sketch_batch(kt_ctx *ctx, const uint8_t *bases, const uint64_t *offsets, uint64_t n_reads, int k, uint32_t s,
                               uint64_t seed, uint64_t *hashes, uint32_t *sizes, uint32_t *n_kmers, int mem) {
    if (!ctx) return kt::fail(KT_ERR_ARG, "kt_sketch_batch: null ctx");
    if (k < 1 || k > 31) return kt::fail(KT_ERR_ARG, "kt_sketch_batch: k must be in 1..31");
    if (s < 1 || s > MAX_S) return kt::fail(KT_ERR_ARG, "kt_sketch_batch: s must be in 1..KT_SKETCH_MAX_S");
    Call call(ctx, mem, "kt_sketch_batch");
    if (int rc = call.enter()) return rc;
    if (n_reads == 0) return KT_OK;
    if (!offsets || !hashes || !sizes) return call.fail("null buffer");
    if (int rc = call.batch(bases, offsets, n_reads)) return rc;
    const uint64_t total = call.total;

    uint64_t max_len = 0;
    if (call.host()) {
        for (uint64_t i = 0; i < n_reads; i++) {
            if (offsets[i + 1] < offsets[i]) return kt::fail(KT_ERR_ARG, "kt_sketch_batch: offsets decrease");
            const uint64_t len = offsets[i + 1] - offsets[i];
            max_len = len > max_len ? len : max_len;
        }
    } else if (total) {
        uint64_t *d_max = nullptr;
        if (int rc = call.scratch(kt::AUX2, 8, &d_max)) return rc;
        KT_HIP(hipMemsetAsync(d_max, 0, 8, ctx->stream));
        hipLaunchKernelGGL(max_len_kernel, dim3(grid_for(ctx, (n_reads + BLOCK - 1) / BLOCK, 8)), dim3(BLOCK), 0, ctx->stream, offsets,
                           n_reads, d_max);
        KT_HIP(hipGetLastError());
        KT_HIP(hipMemcpyAsync(&max_len, d_max, 8, hipMemcpyDeviceToHost, ctx->stream));
        KT_HIP(hipStreamSynchronize(ctx->stream));
        ctx->unclaim(kt::AUX2);  // (read back: the tree's second set of slots may follow)
    }
    if (max_len >= (1ull << 32)) return kt::fail(KT_ERR_ARG, "kt_sketch_batch: a read of 2^32 bases or more (the numbers of k-mers are u32)");

    BatchOut o{hashes, sizes, n_kmers, s};
    if (call.host()) {  // hashes | sizes | n_kmers in one buffer
        if (int rc = call.stage()) return rc;
        const uint64_t rows = n_reads * (uint64_t)s;
        if (int rc = call.scratch(kt::OUT, rows * 8 + n_reads * 8, &o.hashes)) return rc;
        o.sizes = (uint32_t *)(o.hashes + rows);
        o.n_kmers = n_kmers ? o.sizes + n_reads : nullptr;
        call.back(hashes, (const uint64_t *)o.hashes, rows);
        call.back(sizes, (const uint32_t *)o.sizes, n_reads);
        call.back(n_kmers, (const uint32_t *)o.n_kmers, n_reads);
    }
    if (int rc = sketch_device(ctx, call.bases, call.offsets, n_reads, total, max_len, k, seed, o)) return rc;
    return call.finish();
}

// the merge over device arrays; max_rows = the rows of the largest group (at least 1)
static int merge_device(kt_ctx *ctx, const uint64_t *hashes, const uint32_t *sizes, uint64_t n, uint32_t s, const uint64_t *go,
                        uint64_t n_groups, uint64_t max_rows, uint64_t *out_hashes, uint32_t *out_sizes) {
    hipLaunchKernelGGL(empty_groups_kernel, dim3(grid_for(ctx, n_groups, 8)), dim3(BLOCK), 0, ctx->stream, go, n_groups, s, out_hashes,
                       out_sizes);
    KT_HIP(hipGetLastError());
    if (!max_rows) return KT_OK;
    uint32_t rounds = 1;
    while ((1ull << rounds) < max_rows) rounds++;
    const uint64_t buf_bytes = n * (uint64_t)s * 8;
    char *p0 = nullptr, *p1 = nullptr;  // (null where no round writes: a group's last round writes the output row)
    if (rounds >= 2)
        if (int rc = ctx->claim(kt::AUX1, buf_bytes + n * 4, "kt_sketch_merge", &p0)) return rc;
    if (rounds >= 3)
        if (int rc = ctx->claim(kt::AUX2, buf_bytes + n * 4, "kt_sketch_merge", &p1)) return rc;
    uint64_t *mh[2] = {(uint64_t *)p0, (uint64_t *)p1};
    uint32_t *ms[2] = {(uint32_t *)(p0 + buf_bytes), (uint32_t *)(p1 + buf_bytes)};
    const uint32_t grid = (uint32_t)(n < (1u << 20) ? (n ? n : 1) : (1u << 20));
    for (uint32_t r = 0; r < rounds; r++) {
        const uint64_t *in_h = r ? mh[(r - 1) & 1u] : hashes;
        const uint32_t *in_s = r ? ms[(r - 1) & 1u] : sizes;
        hipLaunchKernelGGL(sketch_group_kernel, dim3(grid), dim3(BLOCK), 0, ctx->stream, go, n_groups, in_h, in_s, mh[r & 1u], ms[r & 1u],
                           out_hashes, out_sizes, s, 1ull << r);
        KT_HIP(hipGetLastError());
    }
    return KT_OK;
}

extern "C" int kt_sketch_merge(kt_ctx *ctx, const uint64_t *hashes, const uint32_t *sizes, uint64_t n, uint32_t s,
                               const uint64_t *group_offsets, uint64_t n_groups, uint64_t *out_hashes, uint32_t *out_sizes, int mem) {
    if (!ctx) return kt::fail(KT_ERR_ARG, "kt_sketch_merge: null ctx");
    if (s < 1 || s > MAX_S) return kt::fail(KT_ERR_ARG, "kt_sketch_merge: s must be in 1..KT_SKETCH_MAX_S");
    Call call(ctx, mem, "kt_sketch_merge");
    if (int rc = call.enter()) return rc;
    if (n_groups == 0) return KT_OK;
    if (!group_offsets || !out_hashes || !out_sizes || (n && (!hashes || !sizes))) return call.fail("null buffer");
    const char *bad_groups = "group_offsets must not decrease and must end at or below n";
    uint64_t max_rows = 0;
    if (!call.host()) {
        uint64_t *d_chk = nullptr, chk[2] = {0, 0};  // [0]: largest group, [1]: the bad flag
        if (int rc = call.scratch(kt::AUX2, 16, &d_chk)) return rc;
        KT_HIP(hipMemsetAsync(d_chk, 0, 16, ctx->stream));
        hipLaunchKernelGGL(group_check_kernel, dim3(grid_for(ctx, (n_groups + BLOCK - 1) / BLOCK, 8)), dim3(BLOCK), 0, ctx->stream,
                           group_offsets, n_groups, n, (uint32_t *)(d_chk + 1), d_chk);
        KT_HIP(hipGetLastError());
        KT_HIP(hipMemcpyAsync(chk, d_chk, 16, hipMemcpyDeviceToHost, ctx->stream));
        KT_HIP(hipStreamSynchronize(ctx->stream));
        ctx->unclaim(kt::AUX2);  // (read back: the tree's second set of rows may follow)
        if (chk[1]) return call.fail(bad_groups);
        return merge_device(ctx, hashes, sizes, n, s, group_offsets, n_groups, chk[0], out_hashes, out_sizes);
    }
    for (uint64_t g = 0; g < n_groups; g++) {
        if (group_offsets[g + 1] < group_offsets[g] || group_offsets[g + 1] > n) return call.fail(bad_groups);
        const uint64_t rows = group_offsets[g + 1] - group_offsets[g];
        max_rows = rows > max_rows ? rows : max_rows;
    }
    const uint64_t in_bytes = n * (uint64_t)s * 8, out_bytes = n_groups * (uint64_t)s * 8;
    // hashes | sizes in BASES, the groups in OFFSETS, out_hashes | out_sizes in OUT
    uint64_t *d_h = nullptr, *d_oh = nullptr;
    const uint64_t *d_go = nullptr;
    if (int rc = call.scratch(kt::BASES, in_bytes + n * 4 + 8, &d_h)) return rc;
    if (int rc = call.in(kt::OFFSETS, group_offsets, n_groups + 1, &d_go)) return rc;
    if (int rc = call.scratch(kt::OUT, out_bytes + n_groups * 4, &d_oh)) return rc;
    uint32_t *d_sz = (uint32_t *)((char *)d_h + in_bytes), *d_os = (uint32_t *)((char *)d_oh + out_bytes);
    if (int rc = call.up(d_h, hashes, n * (uint64_t)s)) return rc;
    if (int rc = call.up(d_sz, sizes, n)) return rc;
    if (int rc = merge_device(ctx, d_h, d_sz, n, s, d_go, n_groups, max_rows, d_oh, d_os)) return rc;
    call.back(out_hashes, (const uint64_t *)d_oh, n_groups * (uint64_t)s);
    call.back(out_sizes, (const uint32_t *)d_os, n_groups);
    return call.finish();
}

static int pairs_device(kt_ctx *ctx, const uint64_t *a_h, const uint32_t *a_s, uint64_t n_a, const uint64_t *b_h, const uint32_t *b_s,
                        uint64_t n_b, uint32_t s, uint32_t *shared, uint32_t *denom) {
    const dim3 grid = ktl::pairs_grid(ctx, n_a, n_b, WAVES);
    if (s <= 2048)
        hipLaunchKernelGGL(sketch_pairs_kernel<2048>, grid, dim3(BLOCK), 0, ctx->stream, a_h, a_s, n_a, b_h, b_s, n_b, s, shared, denom);
    else
        hipLaunchKernelGGL(sketch_pairs_kernel<MAX_S>, grid, dim3(BLOCK), 0, ctx->stream, a_h, a_s, n_a, b_h, b_s, n_b, s, shared, denom);
    KT_HIP(hipGetLastError());
    return KT_OK;
}

extern "C" int kt_sketch_pairs(kt_ctx *ctx, const uint64_t *a_hashes, const uint32_t *a_sizes, uint64_t n_a, const uint64_t *b_hashes,
                               const uint32_t *b_sizes, uint64_t n_b, uint32_t s, uint32_t *shared, uint32_t *denom, int mem) {
    if (!ctx) return kt::fail(KT_ERR_ARG, "kt_sketch_pairs: null ctx");
    if (s < 1 || s > MAX_S) return kt::fail(KT_ERR_ARG, "kt_sketch_pairs: s must be in 1..KT_SKETCH_MAX_S");
    Call call(ctx, mem, "kt_sketch_pairs");
    if (int rc = call.enter()) return rc;
    if (n_a == 0 || n_b == 0) return KT_OK;
    if (!a_hashes || !a_sizes || !b_hashes || !b_sizes || !shared) return call.fail("null buffer");
    if (!call.host()) return pairs_device(ctx, a_hashes, a_sizes, n_a, b_hashes, b_sizes, n_b, s, shared, denom);

    const bool same = a_hashes == b_hashes && a_sizes == b_sizes && n_a == n_b;
    const uint64_t a_bytes = n_a * (uint64_t)s * 8, b_bytes = same ? 0 : n_b * (uint64_t)s * 8, cells = n_a * n_b;
    // A's rows | B's rows in BASES, their sizes in OFFSETS, shared | denom in OUT
    uint64_t *d_a = nullptr;
    uint32_t *d_as = nullptr, *d_sh = nullptr;
    if (int rc = call.scratch(kt::BASES, a_bytes + b_bytes + 8, &d_a)) return rc;
    if (int rc = call.scratch(kt::OFFSETS, (n_a + n_b) * 4 + 8, &d_as)) return rc;
    if (int rc = call.scratch(kt::OUT, cells * 8, &d_sh)) return rc;
    uint64_t *d_b = same ? d_a : (uint64_t *)((char *)d_a + a_bytes);
    uint32_t *d_bs = same ? d_as : d_as + n_a, *d_dn = d_sh + cells;
    if (int rc = call.up(d_a, a_hashes, n_a * (uint64_t)s)) return rc;
    if (int rc = call.up(d_as, a_sizes, n_a)) return rc;
    if (!same) {
        if (int rc = call.up(d_b, b_hashes, n_b * (uint64_t)s)) return rc;
        if (int rc = call.up(d_bs, b_sizes, n_b)) return rc;
    }
    if (int rc = pairs_device(ctx, d_a, d_as, n_a, d_b, d_bs, n_b, s, d_sh, denom ? d_dn : nullptr)) return rc;
    call.back(shared, (const uint32_t *)d_sh, cells);
    call.back(denom, (const uint32_t *)d_dn, cells);
    return call.finish();
}
