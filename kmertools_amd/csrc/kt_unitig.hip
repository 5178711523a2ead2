// kt_unitig.hip - the maximal unitigs of a table's de Bruijn graph (kt_ctr_unitigs): the nodes of kt_ctr_graph, sorted, are
// chained through their joined sides, ranked along their chains by pointer doubling and spelled into one base array.
//
// Stages, every one a plain launch over nodes or over ORIENTED STATES (state 2i + e = node i entered through side e, R = 0,
// L = 1; it leaves through side 1 - e):
//   a. nodes     kt_ctr_graph(KT_MEM_DEVICE, sorted, counts) into this call's scratch: node index = rank of the key
//   b. links     link[2i + side] = 2j + facing side of the one neighbour across a joined side (binary search of the sorted
//                keys), NIL for an unjoined side; a second launch checks that every link is answered (link[link[x]] == x)
//   c. ranking   (next, dist) per state, a terminal state (its exit side unjoined) points at itself with dist 0;
//                rounds of next = next[next], dist += dist[next] between two buffers.  The number of rounds is a function of
//                n computed on the host (ceil(log2 2n) + 1); no launch waits for convergence.  States that do not end at
//                a terminal after that lie on cycles (counted, one read-back: no cycle, no cycle stages): those get a second
//                doubling of (smallest state index in the window ahead, distance to it) - the smallest state of a directed
//                cycle is the one of its smallest node - for ceil(log2 n) rounds.
//   d. placing   a path node takes the direction whose origin terminal has the smaller index (index order is key order), a
//                cycle node the direction that meets its smallest node entered from the left; both give (start node,
//                position, orientation).  Start nodes carry their unitig's length; an exclusive scan of (is start, bases)
//                over node index numbers the unitigs in start-key order and lays out their bases.
//   e. spelling  every node writes the last base of its oriented k-mer at offset + position + k - 1, a start node its first
//                k - 1 bases, the offset and the flags as well; count sums by integer atomics.
// kt_ctr_unitigs_linked adds the edges of the compacted graph (only then: kt_ctr_unitigs launches and claims what it did):
//   f. degrees   one thread per node side; a side that is a unitig end (position 0: the - end, position len - 1: the + end,
//                outward side from the orientation bit) counts the set bits of its outward nibble, one more where a
//                neighbour string is its own reverse complement; a cycle's start node 1 per end.  deg[2 * unitig + end],
//                an exclusive scan of it (the same tile sums / one workgroup / apply) = link_offsets and the total.
//   g. emit      the same threads: every neighbour's index by stage b's search, its place and its unitig's length give
//                (v, sv); the neighbour has to be first (+) or last (-) in a unitig that is no cycle, else ERR_LINK; the at
//                most 5 values, sorted in registers, go to the end's offset.
// kt_ctr_unitig_tips and kt_ctr_clip_tips run the linked stages into this call's scratch (offsets, count sums, flags and links;
// no base is written) and go on:
//   h. classes   one thread per unitig: short (no cycle, at most max_tip_nodes nodes) and dead at both ends (isolated), at one
//                end (a candidate, and which end lives), or neither
//   i. marks     the same threads: a candidate is a tip when every link of its live end arrives at an end that has another
//                link to a unitig that beats it (no candidate, or a higher mean count as 128-bit products, then the lower
//                number): at most 5 x 5 links; the tally summed per wave, one atomic per word
//   j. list      kt_ctr_clip_tips only, one thread per node: its key where its unitig (stage d's place, ex_id) is marked
//                for erasing, else KT_EMPTY_KEY - kt_ctr_erase skips those, so the list is not compacted; it goes to
//                kt_ctr_erase as device memory, and the next round starts at stage a on what is left
// Anything the rule excludes (a link without an answer, a neighbour that is no node, a chain that is neither a path nor a
// cycle) raises a bit in the call's error word and comes back as an error: nothing spins.
#include "kt_device.hpp"
#include "kt_launch.hpp"

namespace {

using namespace ktl;

constexpr int BLOCK = 256, WAVES = BLOCK / 64;
constexpr uint32_t NIL = 0xFFFFFFFFu;
constexpr uint32_t SCAN_ITEMS = 4, SCAN_TILE = BLOCK * SCAN_ITEMS;
constexpr uint32_t CIRC = 0x80000000u;  // in slen: the unitig is a cycle; in place.y: the node is spelled forward
constexpr uint32_t ERR_DEGREE = 1u, ERR_SEARCH = 2u, ERR_MUTUAL = 4u, ERR_CHAIN = 8u, ERR_CYCLE = 16u, ERR_LINK = 32u;

// the call's device words, zeroed on the stream before the first kernel
struct Words {
    uint32_t err, pad;
    unsigned long long unresolved, n_unitigs, n_bases;
};

__device__ __forceinline__ uint64_t pack(uint32_t lo, uint32_t hi) { return (uint64_t)lo | ((uint64_t)hi << 32); }
__device__ __forceinline__ uint32_t lo32(uint64_t v) { return (uint32_t)v; }
__device__ __forceinline__ uint32_t hi32(uint64_t v) { return (uint32_t)(v >> 32); }

// the index of the first of the n ascending keys that is >= v
__device__ __forceinline__ uint64_t first_key_not_below(const uint64_t *__restrict__ keys, uint64_t n, uint64_t v) {
    uint64_t lo = 0, hi = n;
    while (lo < hi) {
        const uint64_t mid = lo + ((hi - lo) >> 1);
        if (keys[mid] < v) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// the neighbour string of F (reverse complement R) through `side` with base x: right F[1..k) + x, reverse complement
// comp(x) + R[0..k-1); left x + F[0..k-1), reverse complement R[1..k) + comp(x)
__device__ __forceinline__ void neighbour(uint64_t F, uint64_t R, uint32_t side, uint64_t x, uint32_t k, uint64_t *s, uint64_t *rs) {
    const uint32_t top = 2u * k - 2u;
    const uint64_t mask = (1ull << (2u * k)) - 1ull;
    *s = side == 0u ? ((F << 2) & mask) | x : (F >> 2) | (x << top);
    *rs = side == 0u ? (R >> 2) | ((3ull - x) << top) : ((R << 2) & mask) | (3ull - x);
}

// ---- b. links --------------------------------------------------------------------------------------------------------

// one thread per node side
__global__ __launch_bounds__(BLOCK) void unitig_link_kernel(const uint64_t *__restrict__ keys, const uint32_t *__restrict__ info,
                                                            uint64_t n, uint32_t k, uint32_t *__restrict__ link,
                                                            Words *__restrict__ w) {
    const uint64_t t = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (t >= 2 * n) return;
    const uint64_t i = t >> 1;
    const uint32_t side = (uint32_t)t & 1u;
    const uint32_t inf = info[i];
    uint32_t out = NIL;
    if (!(inf & (0x100u << side))) {
        const uint32_t bits = (inf >> (4u * side)) & 0xFu;
        if (__popc(bits) != 1) {
            atomicOr(&w->err, ERR_DEGREE);
        } else {
            const uint64_t x = (uint64_t)(__ffs((int)bits) - 1);
            const uint64_t F = keys[i], R = ktd::rev_comp(F, (int)k);
            uint64_t s, rs;
            neighbour(F, R, side, x, k, &s, &rs);
            const uint64_t v = s < rs ? s : rs;
            if (v != F && s != rs && F != R) {
                const uint64_t lo = first_key_not_below(keys, n, v);
                if (lo < n && keys[lo] == v) out = (uint32_t)(2 * lo) + (s == v ? side ^ 1u : side);
                else atomicOr(&w->err, ERR_SEARCH);
            }
        }
    }
    link[t] = out;
}

// ---- c. ranking ------------------------------------------------------------------------------------------------------

// every link is answered; state s starts at its successor, or at itself when its exit side is unjoined
__global__ __launch_bounds__(BLOCK) void unitig_rank_init_kernel(const uint32_t *__restrict__ link, uint64_t m,
                                                                 uint64_t *__restrict__ cur, Words *__restrict__ w) {
    const uint64_t s = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (s >= m) return;
    const uint32_t l = link[s];
    if (l != NIL && (l >= m || link[l] != (uint32_t)s)) atomicOr(&w->err, ERR_MUTUAL);
    const uint32_t x = link[s ^ 1ull];
    cur[s] = x == NIL || x >= m ? pack((uint32_t)s, 0u) : pack(x, 1u);
}

__global__ __launch_bounds__(BLOCK) void unitig_rank_jump_kernel(const uint64_t *__restrict__ cur, uint64_t m,
                                                                 uint64_t *__restrict__ out) {
    const uint64_t s = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (s >= m) return;
    const uint64_t p = cur[s], q = cur[lo32(p)];
    out[s] = pack(lo32(q), hi32(p) + hi32(q));
}

// the state that `res` says s ends at is a terminal
__device__ __forceinline__ bool resolved(const uint64_t *__restrict__ res, const uint32_t *__restrict__ link, uint64_t s) {
    return link[lo32(res[s]) ^ 1u] == NIL;
}

__global__ __launch_bounds__(BLOCK) void unitig_unresolved_kernel(const uint64_t *__restrict__ res, const uint32_t *__restrict__ link,
                                                                  uint64_t m, Words *__restrict__ w) {
    const uint64_t s = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
    const bool open = s < m && !resolved(res, link, s);
    const uint64_t b = __ballot(open);
    if (b && (threadIdx.x & 63u) == (uint32_t)(__ffsll((long long)b) - 1)) atomicAdd(&w->unresolved, (unsigned long long)__popcll(b));
}

// cycle states: val = (smallest state index among the next `hop` states, this one included) << 32 | distance to it
__global__ __launch_bounds__(BLOCK) void unitig_cycle_init_kernel(const uint64_t *__restrict__ res, const uint32_t *__restrict__ link,
                                                                  uint64_t m, uint64_t *__restrict__ val, uint32_t *__restrict__ nxt) {
    const uint64_t s = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (s >= m) return;
    const bool path = resolved(res, link, s);
    val[s] = path ? ~0ull : (uint64_t)s << 32;
    nxt[s] = path ? NIL : link[s ^ 1ull];
}

__global__ __launch_bounds__(BLOCK) void unitig_cycle_jump_kernel(const uint64_t *__restrict__ val, const uint32_t *__restrict__ nxt,
                                                                  uint64_t m, uint64_t hop, uint64_t *__restrict__ val_out,
                                                                  uint32_t *__restrict__ nxt_out) {
    const uint64_t s = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (s >= m) return;
    const uint32_t a = nxt[s];
    uint64_t v = val[s];
    uint32_t b = NIL;
    if (a != NIL && a < m) {
        const uint64_t c = val[a] + hop;  // (distance < hop, so the sum stays in the low word)
        v = c < v ? c : v;
        b = nxt[a];
    }
    val_out[s] = v;
    nxt_out[s] = b;
}

// ---- d. placing ------------------------------------------------------------------------------------------------------

// place[i] = (start node, position | forward << 31); slen[i] = the unitig's nodes (| CIRC) at its start node, else 0
__global__ __launch_bounds__(BLOCK) void unitig_place_kernel(const uint64_t *__restrict__ res, const uint32_t *__restrict__ link,
                                                             const uint64_t *__restrict__ cval, uint64_t n, uint2 *__restrict__ place,
                                                             uint32_t *__restrict__ slen, Words *__restrict__ w) {
    const uint64_t i = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    const uint64_t p0 = res[2 * i], p1 = res[2 * i + 1];
    const bool r0 = link[lo32(p0) ^ 1u] == NIL, r1 = link[lo32(p1) ^ 1u] == NIL;
    uint32_t start = (uint32_t)i, pos = 0, fwd = 1, len = 1, err = 0;
    if (r0 && r1) {
        // state (i, e) runs to terminal a_e in d_e steps; walking the other way, a_e is where direction 1 - e comes from
        const uint32_t a0 = lo32(p0) >> 1, a1 = lo32(p1) >> 1, d0 = hi32(p0), d1 = hi32(p1);
        fwd = a0 <= a1;
        start = fwd ? a0 : a1;
        pos = fwd ? d0 : d1;
        len = d0 + d1 + 1u;
        if (a0 == a1 && len != 1u) err = ERR_CHAIN;
    } else if (!r0 && !r1 && cval) {
        const uint64_t v0 = cval[2 * i], v1 = cval[2 * i + 1];
        const uint32_t m0 = hi32(v0), m1 = hi32(v1);  // the smallest states of the two directed cycles: one node, two entries
        fwd = m1 & 1u;
        const uint32_t d = lo32(fwd ? v1 : v0);
        start = m0 >> 1;
        const uint32_t after = start < n ? link[2ull * start] : NIL;  // the state behind (start, entered left): c - 1 from it
        if ((m0 ^ m1) != 1u || after == NIL || after >= 2 * n) {
            err = ERR_CYCLE;
            start = (uint32_t)i;
        } else {
            len = lo32(cval[after]) + 1u;
            pos = d ? len - d : 0u;
            if (d >= len || (hi32(cval[after]) | 1u) != (m0 | 1u)) err = ERR_CYCLE, pos = 0;
            len |= CIRC;
        }
    } else {
        err = ERR_CHAIN;
    }
    if (err) {
        atomicOr(&w->err, err);
        start = (uint32_t)i, pos = 0, len = 1;
    }
    place[i] = make_uint2(start, pos | (fwd << 31));
    slen[i] = pos == 0u && start == (uint32_t)i ? len : 0u;
}

// inclusive prefix sums of a and b over the workgroup's threads; *ta, *tb = the sums
__device__ __forceinline__ void block_scan2(uint64_t &a, uint64_t &b, uint64_t (*wsum)[2], uint64_t *ta, uint64_t *tb) {
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const uint64_t ua = __shfl_up(a, off, 64), ub = __shfl_up(b, off, 64);
        if (lane >= (uint32_t)off) a += ua, b += ub;
    }
    if (lane == 63u) wsum[wave][0] = a, wsum[wave][1] = b;
    ktd::lds_barrier();
    uint64_t pa = 0, pb = 0, sa = 0, sb = 0;
#pragma unroll
    for (uint32_t x = 0; x < (uint32_t)WAVES; x++) {
        const uint64_t xa = wsum[x][0], xb = wsum[x][1];
        if (x < wave) pa += xa, pb += xb;
        sa += xa, sb += xb;
    }
    ktd::lds_barrier();  // (wsum is rewritten by the next call)
    a += pa, b += pb;
    *ta = sa, *tb = sb;
}

// a start node's unitig: 1 unitig, nodes + k - 1 bases
__device__ __forceinline__ uint64_t bases_of(uint32_t sl, uint32_t k) { return sl ? (uint64_t)(sl & ~CIRC) + k - 1u : 0ull; }

// tile t (SCAN_TILE nodes) -> tiles[2t] = its unitigs, tiles[2t + 1] = its bases
__global__ __launch_bounds__(BLOCK) void unitig_tile_sum_kernel(const uint32_t *__restrict__ slen, uint64_t n, uint32_t k,
                                                                uint64_t *__restrict__ tiles) {
    __shared__ uint64_t wsum[WAVES][2];
    const uint64_t base = (uint64_t)blockIdx.x * SCAN_TILE + (uint64_t)threadIdx.x * SCAN_ITEMS;
    uint64_t a = 0, b = 0, ta, tb;
#pragma unroll
    for (uint32_t j = 0; j < SCAN_ITEMS; j++) {
        const uint32_t sl = base + j < n ? slen[base + j] : 0u;
        a += sl != 0u;
        b += bases_of(sl, k);
    }
    block_scan2(a, b, wsum, &ta, &tb);
    if (threadIdx.x == 0) tiles[2ull * blockIdx.x] = ta, tiles[2ull * blockIdx.x + 1] = tb;
}

// one workgroup: the tiles' sums into their exclusive prefixes, the totals into *sum_a and *sum_b
__global__ __launch_bounds__(BLOCK) void unitig_tile_scan_kernel(uint64_t *__restrict__ tiles, uint64_t T,
                                                                 unsigned long long *__restrict__ sum_a,
                                                                 unsigned long long *__restrict__ sum_b) {
    __shared__ uint64_t wsum[WAVES][2];
    uint64_t ca = 0, cb = 0;
    for (uint64_t c0 = 0; c0 < T; c0 += BLOCK) {
        const uint64_t t = c0 + threadIdx.x;
        const uint64_t va = t < T ? tiles[2 * t] : 0, vb = t < T ? tiles[2 * t + 1] : 0;
        uint64_t a = va, b = vb, ta, tb;
        block_scan2(a, b, wsum, &ta, &tb);
        if (t < T) tiles[2 * t] = ca + a - va, tiles[2 * t + 1] = cb + b - vb;
        ca += ta, cb += tb;
    }
    if (threadIdx.x == 0) *sum_a = ca, *sum_b = cb;
}

// ex_id[i], ex_off[i] = unitigs and bases that start at nodes before i
__global__ __launch_bounds__(BLOCK) void unitig_scan_apply_kernel(const uint32_t *__restrict__ slen, uint64_t n, uint32_t k,
                                                                  const uint64_t *__restrict__ tiles, uint32_t *__restrict__ ex_id,
                                                                  uint64_t *__restrict__ ex_off) {
    __shared__ uint64_t wsum[WAVES][2];
    const uint64_t base = (uint64_t)blockIdx.x * SCAN_TILE + (uint64_t)threadIdx.x * SCAN_ITEMS;
    uint32_t sl[SCAN_ITEMS];
    uint64_t a = 0, b = 0, ta, tb;
#pragma unroll
    for (uint32_t j = 0; j < SCAN_ITEMS; j++) {
        sl[j] = base + j < n ? slen[base + j] : 0u;
        a += sl[j] != 0u;
        b += bases_of(sl[j], k);
    }
    const uint64_t own_a = a, own_b = b;
    block_scan2(a, b, wsum, &ta, &tb);
    uint64_t ra = tiles[2ull * blockIdx.x] + a - own_a, rb = tiles[2ull * blockIdx.x + 1] + b - own_b;
#pragma unroll
    for (uint32_t j = 0; j < SCAN_ITEMS; j++) {
        if (base + j < n) ex_id[base + j] = (uint32_t)ra, ex_off[base + j] = rb;
        ra += sl[j] != 0u;
        rb += bases_of(sl[j], k);
    }
}

// ---- e. spelling -----------------------------------------------------------------------------------------------------

struct SpellArgs {
    const uint64_t *keys;
    const uint32_t *counts;
    const uint2 *place;
    const uint32_t *slen, *ex_id;
    const uint64_t *ex_off;
    uint64_t n;
    uint32_t k;
    uint8_t *bases;
    uint64_t *offsets, *count_sums;
    uint32_t *flags;
    uint64_t max_bases, max_unitigs;  // (the host launches this only when everything fits: these guard the stores all the same)
    const Words *w;
};

__device__ __forceinline__ uint8_t letter(uint64_t code) { return (uint8_t)((0x54474341u >> (8u * (uint32_t)(code & 3ull))) & 0xFFu); }  // "ACGT"

__global__ __launch_bounds__(BLOCK) void unitig_spell_kernel(SpellArgs s) {
    const uint64_t i = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i == 0 && s.w->n_unitigs <= s.max_unitigs) s.offsets[s.w->n_unitigs] = s.w->n_bases;
    if (i >= s.n) return;
    const uint2 pl = s.place[i];
    const uint32_t start = pl.x, pos = pl.y & ~CIRC, k = s.k;
    const bool fwd = pl.y & CIRC;
    const uint64_t uid = s.ex_id[start], off = s.ex_off[start];
    if (uid >= s.max_unitigs) return;
    const uint64_t F = s.keys[i];
    // the node's k-mer as the unitig reads it
    const uint64_t S = fwd ? F : ktd::rev_comp(F, (int)k);
    const uint64_t at = off + pos + k - 1u;
    if (at < s.max_bases) s.bases[at] = letter(S);
    if (s.count_sums) atomicAdd(reinterpret_cast<unsigned long long *>(s.count_sums + uid), (unsigned long long)s.counts[i]);
    if (start == (uint32_t)i && pos == 0u) {
        for (uint32_t j = 0; j + 1u < k; j++)
            if (off + j < s.max_bases) s.bases[off + j] = letter(S >> (2u * (k - 1u - j)));
        s.offsets[uid] = off;
        if (s.flags) s.flags[uid] = s.slen[i] & CIRC ? KT_UNITIG_CIRCULAR : 0u;
    }
}

// ---- f, g. the links between unitig ends -----------------------------------------------------------------------------

// the call's link words (in the link scratch: Words stays what kt_ctr_unitigs reads back)
struct LinkWords {
    unsigned long long n_links, unused;
};

struct LinkArgs {
    const uint64_t *keys;
    const uint32_t *info;
    const uint2 *place;
    const uint32_t *slen, *ex_id;
    uint64_t n, n_ends;  // n_ends = 2 * unitigs
    uint32_t k;
    uint32_t *deg;                 // f: deg[end]
    const uint64_t *link_offsets;  // g: where each end's links start, n_ends + 1 entries
    uint32_t *link_to;
    uint64_t max_links;  // (the host launches g only when everything fits: this guards the stores all the same)
    Words *w;
};

// puts v into the ascending a[0..5) (unused places hold NIL) - fixed indices only, so that a[] stays in registers
__device__ __forceinline__ void insert5(uint32_t (&a)[5], uint32_t v) {
#pragma unroll
    for (int t = 0; t < 5; t++) {
        const uint32_t lo = v < a[t] ? v : a[t];
        v = v < a[t] ? a[t] : v;
        a[t] = lo;
    }
}

// Thread t = side t & 1 of node t >> 1.  The side is the outward side of a unitig end when the node is first in its unitig
// (the - end: the string read backwards leaves through it) or last (the + end); a cycle has no such side, and its two
// closing links are given by its start node.  EMIT false: deg[2 * unitig + end] = the end's links.  EMIT true: the links.
template <bool EMIT>
__device__ __forceinline__ void unitig_end_links(const LinkArgs &a) {
    const uint64_t t = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (t >= 2 * a.n) return;
    const uint64_t i = t >> 1;
    const uint32_t side = (uint32_t)t & 1u, k = a.k;
    const uint2 pl = a.place[i];
    const uint32_t start = pl.x, pos = pl.y & ~CIRC, fwd = pl.y >> 31;
    const uint32_t sl = a.slen[start], len = sl & ~CIRC;
    // forward node: its right side ends the + string, its left side the - string; spelled backwards: the other way round
    const uint32_t end = sl & CIRC ? side : (uint32_t)(side == fwd);
    if (sl & CIRC ? start != (uint32_t)i : pos != (end ? 0u : len - 1u)) return;
    const uint64_t e = 2ull * a.ex_id[start] + end;
    if (e >= a.n_ends) return;
    uint32_t val[5] = {NIL, NIL, NIL, NIL, NIL};
    uint32_t cnt = 0, err = 0;
    if (sl & CIRC) {  // (u, +) -> (u, +) and (u, -) -> (u, -): the last k - 1 bases repeat the first
        cnt = 1;
        val[0] = (uint32_t)e;
    } else {
        const uint32_t bits = (a.info[i] >> (4u * side)) & 0xFu;
        const uint64_t F = a.keys[i], R = ktd::rev_comp(F, (int)k);
#pragma unroll
        for (uint32_t x = 0; x < 4u; x++) {
            if (!(bits >> x & 1u)) continue;
            uint64_t s, rs;
            neighbour(F, R, side, (uint64_t)x, k, &s, &rs);
            const bool twice = s == rs;  // its own reverse complement: a single node that begins both of its orientations
            cnt += twice ? 2u : 1u;
            if (!EMIT) continue;
            const uint64_t v = s < rs ? s : rs;
            const uint64_t j = first_key_not_below(a.keys, a.n, v);
            if (j >= a.n || a.keys[j] != v) {
                err |= ERR_SEARCH;
                continue;
            }
            const uint2 pj = a.place[j];
            const uint32_t sj = a.slen[pj.x], lenj = sj & ~CIRC, posj = pj.y & ~CIRC;
            const uint32_t to = 2u * a.ex_id[pj.x];
            // the end's string goes on as s through the right side, as rs through the left: the neighbour reads that way in
            // (v, +) when it is spelled as it is met, and then has to come first; else in (v, -), where it has to come last
            const bool plus = ((side == 0u ? s : rs) == v) == (bool)(pj.y >> 31);
            if ((sj & CIRC) || posj != (plus ? 0u : lenj - 1u) || (twice && lenj != 1u)) err |= ERR_LINK;
            if (twice) insert5(val, to), insert5(val, to + 1u);
            else insert5(val, to + (plus ? 0u : 1u));
        }
    }
    if (!EMIT) {
        a.deg[e] = cnt;
        return;
    }
    if (err) atomicOr(&a.w->err, err);
    const uint64_t at = a.link_offsets[e];
    if (cnt > 5u || at + cnt > a.max_links) return;
#pragma unroll
    for (uint32_t c = 0; c < 5u; c++)
        if (c < cnt) a.link_to[at + c] = val[c];
}

__global__ __launch_bounds__(BLOCK) void unitig_end_degree_kernel(LinkArgs a) { unitig_end_links<false>(a); }
__global__ __launch_bounds__(BLOCK) void unitig_end_emit_kernel(LinkArgs a) { unitig_end_links<true>(a); }

// tile t (SCAN_TILE ends) -> tiles[2t] = its links (tiles[2t + 1] = 0: the tile scan is stage d's)
__global__ __launch_bounds__(BLOCK) void unitig_end_tile_sum_kernel(const uint32_t *__restrict__ deg, uint64_t n_ends,
                                                                    uint64_t *__restrict__ tiles) {
    __shared__ uint64_t wsum[WAVES][2];
    const uint64_t base = (uint64_t)blockIdx.x * SCAN_TILE + (uint64_t)threadIdx.x * SCAN_ITEMS;
    uint64_t a = 0, b = 0, ta, tb;
#pragma unroll
    for (uint32_t j = 0; j < SCAN_ITEMS; j++) a += base + j < n_ends ? deg[base + j] : 0u;
    block_scan2(a, b, wsum, &ta, &tb);
    if (threadIdx.x == 0) tiles[2ull * blockIdx.x] = ta, tiles[2ull * blockIdx.x + 1] = tb;
}

// link_offsets[e] = the links of the ends before e; link_offsets[n_ends] = all of them
__global__ __launch_bounds__(BLOCK) void unitig_end_scan_apply_kernel(const uint32_t *__restrict__ deg, uint64_t n_ends,
                                                                      const uint64_t *__restrict__ tiles,
                                                                      const LinkWords *__restrict__ lw,
                                                                      uint64_t *__restrict__ link_offsets) {
    __shared__ uint64_t wsum[WAVES][2];
    const uint64_t base = (uint64_t)blockIdx.x * SCAN_TILE + (uint64_t)threadIdx.x * SCAN_ITEMS;
    uint32_t d[SCAN_ITEMS];
    uint64_t a = 0, b = 0, ta, tb;
#pragma unroll
    for (uint32_t j = 0; j < SCAN_ITEMS; j++) {
        d[j] = base + j < n_ends ? deg[base + j] : 0u;
        a += d[j];
    }
    const uint64_t own = a;
    block_scan2(a, b, wsum, &ta, &tb);
    uint64_t r = tiles[2ull * blockIdx.x] + a - own;
#pragma unroll
    for (uint32_t j = 0; j < SCAN_ITEMS; j++) {
        if (base + j < n_ends) link_offsets[base + j] = r;
        r += d[j];
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) link_offsets[n_ends] = lw->n_links;
}

uint32_t ceil_log2(uint64_t x) {  // the smallest r with 2^r >= x
    uint32_t r = 0;
    while (r < 63u && (1ull << r) < x) r++;
    return r;
}

dim3 blocks_for(uint64_t items, uint64_t per_block = BLOCK) { return dim3((uint32_t)((items + per_block - 1) / per_block)); }

size_t align16(size_t b) { return (b + 15u) & ~(size_t)15u; }

// ---- h, i, j. tips ---------------------------------------------------------------------------------------------------

// what the rule reads: the outputs of the linked run, on the device
struct TipArgs {
    const uint64_t *offsets, *count_sums;
    const uint32_t *flags;
    const uint64_t *link_offsets;
    const uint32_t *link_to;
    uint64_t nu;
    uint32_t k, max_tip_nodes;
};

// the round's device words: tally[0..4) as kt_ctr_unitig_tips gives them, [4] the tips' and [5] the isolated unitigs' occurrences
constexpr int TIP_WORDS = 6;
constexpr uint8_t CLS_NONE = 0, CLS_LIVE_PLUS = 1, CLS_LIVE_MINUS = 2, CLS_ISOLATED = 3;

// one tip round, as its callers ask for it and as it comes back
struct TipRun {
    uint32_t max_tip_nodes;
    uint32_t erase_marks;           // kt_ctr_clip_tips: the marks (bits) whose nodes stage j lists; 0: no stage j
    uint64_t nu = 0;                // unitigs
    uint64_t tally[TIP_WORDS] = {};
    const uint8_t *d_marks = nullptr;  // nu marks, in OUT
    const uint64_t *d_words = nullptr; // the tally on the device
    const uint64_t *d_list = nullptr;  // stage j: n_list keys, KT_EMPTY_KEY for a node that stays, in OUT
    uint64_t n_list = 0;
};

__device__ __forceinline__ uint64_t nodes_of(const TipArgs &a, uint64_t u) { return a.offsets[u + 1] - a.offsets[u] - (a.k - 1u); }

// h. one thread per unitig: short and dead at both ends (isolated), at one end (a candidate, and which end lives), or neither
__global__ __launch_bounds__(BLOCK) void unitig_tip_class_kernel(TipArgs a, uint8_t *__restrict__ cls) {
    const uint64_t u = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (u >= a.nu) return;
    const bool is_short = !(a.flags[u] & KT_UNITIG_CIRCULAR) && nodes_of(a, u) <= (uint64_t)a.max_tip_nodes;
    const uint64_t l0 = a.link_offsets[2 * u], l1 = a.link_offsets[2 * u + 1], l2 = a.link_offsets[2 * u + 2];
    const bool plus = l1 > l0, minus = l2 > l1;
    cls[u] = !is_short || (plus && minus) ? CLS_NONE : plus ? CLS_LIVE_PLUS : minus ? CLS_LIVE_MINUS : CLS_ISOLATED;
}

// w beats the candidate u: it is no candidate, or its mean count is higher (c_w / n_w > c_u / n_u as c_w n_u > c_u n_w in
// 128 bits), or the means are equal and its number is lower
__device__ __forceinline__ bool tip_beats(const TipArgs &a, const uint8_t *__restrict__ cls, uint64_t w, uint64_t u, uint64_t c_u,
                                          uint64_t n_u) {
    const uint8_t cw = cls[w];
    if (cw != CLS_LIVE_PLUS && cw != CLS_LIVE_MINUS) return true;
    const uint64_t c_w = a.count_sums[w], n_w = nodes_of(a, w);
    const uint64_t lh = __umul64hi(c_w, n_u), ll = c_w * n_u, rh = __umul64hi(c_u, n_w), rl = c_u * n_w;
    if (lh != rh) return lh > rh;
    if (ll != rl) return ll > rl;
    return w < u;
}

// i. one thread per unitig: a candidate is a tip when every link f of its live end e arrives at an end f ^ 1 that has
// another link (not the mirror e ^ 1) to a unitig that beats it; marks and the tally
__global__ __launch_bounds__(BLOCK) void unitig_tip_mark_kernel(TipArgs a, const uint8_t *__restrict__ cls, uint8_t *__restrict__ marks,
                                                                unsigned long long *__restrict__ words) {
    const uint64_t u = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
    const uint8_t c = u < a.nu ? cls[u] : CLS_NONE;  // (every lane stays for the wave's sums)
    uint8_t mark = KT_TIP_KEEP;
    if (c == CLS_ISOLATED) {
        mark = KT_TIP_ISOLATED;
    } else if (c != CLS_NONE) {
        const uint64_t e = 2 * u + (c == CLS_LIVE_MINUS), c_u = a.count_sums[u], n_u = nodes_of(a, u);
        bool tip = true;
        for (uint64_t x = a.link_offsets[e]; tip && x < a.link_offsets[e + 1]; x++) {
            const uint64_t g = (uint64_t)a.link_to[x] ^ 1ull;
            bool beaten = false;
            if (g < 2 * a.nu)
                for (uint64_t y = a.link_offsets[g]; !beaten && y < a.link_offsets[g + 1]; y++) {
                    const uint64_t h = a.link_to[y];
                    beaten = h != (e ^ 1ull) && (h >> 1) < a.nu && tip_beats(a, cls, h >> 1, u, c_u, n_u);
                }
            tip = beaten;
        }
        if (tip) mark = KT_TIP_TIP;
    }
    if (u < a.nu) marks[u] = mark;
    // the tally: summed over the wave, one atomic per word and wave that has something to add
    const bool tipped = mark == KT_TIP_TIP, alone = mark == KT_TIP_ISOLATED;
    const uint64_t nodes = mark != KT_TIP_KEEP ? nodes_of(a, u) : 0, occ = mark != KT_TIP_KEEP ? a.count_sums[u] : 0;
    uint64_t v[TIP_WORDS] = {tipped, tipped ? nodes : 0, alone, alone ? nodes : 0, tipped ? occ : 0, alone ? occ : 0};
#pragma unroll
    for (int j = 0; j < TIP_WORDS; j++) {
        for (int o = 32; o > 0; o >>= 1) v[j] += __shfl_down(v[j], o, 64);
        if ((threadIdx.x & 63) == 0 && v[j]) atomicAdd(words + j, (unsigned long long)v[j]);
    }
}

// j. one thread per node: its key where its unitig's mark is one of `erase_marks`, else KT_EMPTY_KEY (which kt_ctr_erase
// skips: the list needs no compaction)
__global__ __launch_bounds__(BLOCK) void unitig_tip_list_kernel(const uint64_t *__restrict__ keys, const uint2 *__restrict__ place,
                                                                const uint32_t *__restrict__ ex_id, uint64_t n,
                                                                const uint8_t *__restrict__ marks, uint64_t nu, uint32_t erase_marks,
                                                                uint64_t *__restrict__ list) {
    const uint64_t i = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    const uint32_t start = place[i].x;
    const uint64_t u = start < n ? ex_id[start] : nu;
    list[i] = u < nu && (marks[u] & erase_marks) ? keys[i] : KT_EMPTY_KEY;
}

// stages h to j behind a linked run, in OUT (the graph's sort has given it back): words | classes | marks | list
int tip_stages(Call &call, kt_ctx *ctx, const TipArgs &a, const uint64_t *keys, const uint2 *place, const uint32_t *ex_id,
               uint64_t n, TipRun *tr) {
    hipStream_t st = ctx->stream;
    const uint64_t nu = a.nu;
    const size_t o_cls = align16(TIP_WORDS * 8), o_marks = o_cls + align16(nu), o_list = o_marks + align16(nu);
    uint8_t *T = nullptr;
    if (int rc = call.scratch(kt::OUT, o_list + (tr->erase_marks ? n * 8 : 0), &T)) return rc;
    unsigned long long *words = (unsigned long long *)T;
    uint8_t *cls = T + o_cls, *marks = T + o_marks;
    uint64_t *list = (uint64_t *)(T + o_list);
    KT_HIP(hipMemsetAsync(words, 0, TIP_WORDS * 8, st));
    hipLaunchKernelGGL(unitig_tip_class_kernel, blocks_for(nu), dim3(BLOCK), 0, st, a, cls);
    hipLaunchKernelGGL(unitig_tip_mark_kernel, blocks_for(nu), dim3(BLOCK), 0, st, a, (const uint8_t *)cls, marks, words);
    if (tr->erase_marks)
        hipLaunchKernelGGL(unitig_tip_list_kernel, blocks_for(n), dim3(BLOCK), 0, st, keys, place, ex_id, n, (const uint8_t *)marks, nu,
                           tr->erase_marks, list);
    KT_HIP(hipGetLastError());
    KT_HIP(hipMemcpyAsync(tr->tally, words, TIP_WORDS * 8, hipMemcpyDeviceToHost, st));
    KT_HIP(hipStreamSynchronize(st));
    tr->nu = nu, tr->d_marks = marks, tr->d_words = (const uint64_t *)words;
    if (tr->erase_marks) tr->d_list = list, tr->n_list = n;
    return KT_OK;
}

// The entry points' one run of the stages, under the caller's `call`.  n_links null: kt_ctr_unitigs, which has no link outputs
// and runs no link stage.  tr set (the tip calls; call is a device call, the output pointers are null): the linked run with
// offsets, count sums, flags and links made in OFFSETS and no base written, then stages h to j.
int unitigs_run(Call &call, const char *name, kt_ctr *table, uint32_t min_count, uint32_t max_count, uint8_t *bases,
                uint64_t max_bases, uint64_t *offsets, uint64_t *count_sums, uint32_t *flags, uint64_t max_unitigs,
                uint64_t *n_unitigs, uint64_t *n_bases, uint64_t *link_offsets, uint32_t *link_to, uint64_t max_links,
                uint64_t *n_links, TipRun *tr) {
    const bool linked = n_links != nullptr;
    kt_ctx *ctx = table->ctx;
    if (int rc = call.refuse_shard(table)) return rc;
    if (min_count == 0) return call.fail("min_count must be >= 1");
    if (min_count > max_count) return call.fail("min_count > max_count");
    if (int rc = call.enter()) return rc;
    const bool store = tr || max_bases || max_unitigs || max_links;
    if (!tr) {
        if ((max_bases && !bases) || (store && !offsets)) return call.fail("null output");
        if (linked && ((store && !link_offsets) || (max_links && !link_to))) return call.fail("null link output");
        if (max_links && !max_unitigs) return call.fail("max_links > 0 with max_unitigs == 0");
    }
    uint64_t n_t = 0;
    if (int rc = kt_ctr_size(table, &n_t)) return rc;  // (KT_ERR_FULL for an overflowed table)
    if (n_t > 0x7FFFFFFEull) return call.fail("a table of more than 2^31 - 2 entries (the oriented node states are u32)");
    hipStream_t st = ctx->stream;
    // no node: no unitig and no link, and offsets[0] = link_offsets[0] = 0 where there is room for them
    auto nothing = [&]() -> int {
        *n_unitigs = 0, *n_bases = 0;
        if (linked) *n_links = 0;
        if (!store || tr) return KT_OK;
        if (call.host()) offsets[0] = 0;
        else KT_HIP(hipMemsetAsync(offsets, 0, 8, st));
        if (linked && call.host()) link_offsets[0] = 0;
        else if (linked) KT_HIP(hipMemsetAsync(link_offsets, 0, 8, st));
        return KT_OK;
    };
    if (!n_t) return nothing();

    // a. the nodes, ascending by key, in this call's AUX1, with room for every entry of the table: 16 bytes an entry
    // (kt_ctr_graph's sort takes OUT and AUX0)
    size_t at = 0;
    auto take = [&](size_t bytes) { const size_t o = at; at += align16(bytes); return o; };
    const size_t o_keys = take(n_t * 8), o_info = take(n_t * 4), o_counts = take(n_t * 4);
    uint8_t *A = nullptr;
    if (int rc = call.scratch(kt::AUX1, at, &A)) return rc;
    uint64_t *keys = (uint64_t *)(A + o_keys);
    uint32_t *info = (uint32_t *)(A + o_info), *counts = (uint32_t *)(A + o_counts);
    uint64_t n = 0;
    if (int rc = kt_ctr_graph(table, min_count, max_count, keys, info, counts, n_t, &n, nullptr, KT_MEM_DEVICE, 1)) return rc;
    if (!n) return nothing();
    // what the later stages keep per node, in AUX2: 64 bytes a node (the cycle stages: 48 more, in BASES)
    const uint64_t T_n = (n + SCAN_TILE - 1) / SCAN_TILE;
    at = 0;
    const size_t o_words = take(sizeof(Words)), o_link = take(n * 8), o_ra = take(n * 16), o_rb = take(n * 16), o_place = take(n * 8),
                 o_slen = take(n * 4), o_exid = take(n * 4), o_exoff = take(n * 8), o_tiles = take(T_n * 16);
    uint8_t *S = nullptr;
    if (int rc = call.scratch(kt::AUX2, at, &S)) return rc;
    Words *w = (Words *)(S + o_words);
    uint64_t *ra = (uint64_t *)(S + o_ra), *rb = (uint64_t *)(S + o_rb), *ex_off = (uint64_t *)(S + o_exoff),
             *tiles = (uint64_t *)(S + o_tiles);
    uint32_t *link = (uint32_t *)(S + o_link), *slen = (uint32_t *)(S + o_slen), *ex_id = (uint32_t *)(S + o_exid);
    uint2 *place = (uint2 *)(S + o_place);
    const uint64_t m = 2 * n, T = (n + SCAN_TILE - 1) / SCAN_TILE;
    const uint32_t k = (uint32_t)table->k;
    KT_HIP(hipMemsetAsync(w, 0, sizeof(Words), st));

    // b. links
    hipLaunchKernelGGL(unitig_link_kernel, blocks_for(m), dim3(BLOCK), 0, st, (const uint64_t *)keys, (const uint32_t *)info, n, k, link, w);
    // c. ranking: a number of rounds fixed by n
    hipLaunchKernelGGL(unitig_rank_init_kernel, blocks_for(m), dim3(BLOCK), 0, st, (const uint32_t *)link, m, ra, w);
    const uint32_t rounds = ceil_log2(m) + 1u;
    for (uint32_t r = 0; r < rounds; r++) {
        hipLaunchKernelGGL(unitig_rank_jump_kernel, blocks_for(m), dim3(BLOCK), 0, st, (const uint64_t *)ra, m, rb);
        uint64_t *t = ra;
        ra = rb, rb = t;
    }
    hipLaunchKernelGGL(unitig_unresolved_kernel, blocks_for(m), dim3(BLOCK), 0, st, (const uint64_t *)ra, (const uint32_t *)link, m, w);
    KT_HIP(hipGetLastError());
    Words h;
    KT_HIP(hipMemcpyAsync(&h, w, sizeof(Words), hipMemcpyDeviceToHost, st));
    KT_HIP(hipStreamSynchronize(st));
    uint64_t *cval = nullptr;
    if (h.unresolved && !h.err) {  // cycles: the smallest state of each, and every state's distance to it
        uint8_t *C = nullptr;
        if (int rc = call.scratch(kt::BASES, align16(m * 8) * 2 + align16(m * 4) * 2, &C)) return rc;
        uint64_t *va = (uint64_t *)C, *vb = (uint64_t *)(C + align16(m * 8));
        uint32_t *na = (uint32_t *)(C + 2 * align16(m * 8)), *nc = (uint32_t *)(C + 2 * align16(m * 8) + align16(m * 4));
        hipLaunchKernelGGL(unitig_cycle_init_kernel, blocks_for(m), dim3(BLOCK), 0, st, (const uint64_t *)ra, (const uint32_t *)link, m, va, na);
        const uint32_t crounds = ceil_log2(n);
        for (uint32_t r = 0; r < crounds; r++) {
            hipLaunchKernelGGL(unitig_cycle_jump_kernel, blocks_for(m), dim3(BLOCK), 0, st, (const uint64_t *)va, (const uint32_t *)na, m,
                               1ull << r, vb, nc);
            uint64_t *tv = va;
            va = vb, vb = tv;
            uint32_t *tn = na;
            na = nc, nc = tn;
        }
        cval = va;
    }
    // d. placing, ids and offsets
    hipLaunchKernelGGL(unitig_place_kernel, blocks_for(n), dim3(BLOCK), 0, st, (const uint64_t *)ra, (const uint32_t *)link,
                       (const uint64_t *)cval, n, place, slen, w);
    hipLaunchKernelGGL(unitig_tile_sum_kernel, dim3((uint32_t)T), dim3(BLOCK), 0, st, (const uint32_t *)slen, n, k, tiles);
    hipLaunchKernelGGL(unitig_tile_scan_kernel, dim3(1), dim3(BLOCK), 0, st, tiles, T, &w->n_unitigs, &w->n_bases);
    hipLaunchKernelGGL(unitig_scan_apply_kernel, dim3((uint32_t)T), dim3(BLOCK), 0, st, (const uint32_t *)slen, n, k,
                       (const uint64_t *)tiles, ex_id, ex_off);
    KT_HIP(hipGetLastError());
    KT_HIP(hipMemcpyAsync(&h, w, sizeof(Words), hipMemcpyDeviceToHost, st));
    KT_HIP(hipStreamSynchronize(st));
    if (h.err)
        return kt::fail(KT_ERR_HIP, std::string(name) + ": internal: the nodes' links do not form paths and cycles (error bits " +
                                        std::to_string(h.err) + ")");
    const uint64_t nu = h.n_unitigs;
    // f. the ends' degrees and their sum, in AUX0 (the graph's sort has given it back): 8 bytes a unitig
    const uint64_t n_ends = 2 * nu, T_e = (n_ends + SCAN_TILE - 1) / SCAN_TILE;
    LinkArgs la{keys, info, place, slen, ex_id, n, n_ends, k, nullptr, nullptr, nullptr, 0, w};
    uint64_t *ltiles = nullptr;
    LinkWords *lw = nullptr;
    LinkWords hl{0, 0};
    if (linked) {
        at = 0;
        const size_t o_lw = take(sizeof(LinkWords)), o_deg = take(n_ends * 4), o_lt = take(T_e * 16);
        uint8_t *D = nullptr;
        if (int rc = call.scratch(kt::AUX0, at, &D)) return rc;
        lw = (LinkWords *)(D + o_lw), la.deg = (uint32_t *)(D + o_deg), ltiles = (uint64_t *)(D + o_lt);
        KT_HIP(hipMemsetAsync(D, 0, o_lt, st));
        hipLaunchKernelGGL(unitig_end_degree_kernel, blocks_for(m), dim3(BLOCK), 0, st, la);
        hipLaunchKernelGGL(unitig_end_tile_sum_kernel, dim3((uint32_t)T_e), dim3(BLOCK), 0, st, (const uint32_t *)la.deg, n_ends, ltiles);
        hipLaunchKernelGGL(unitig_tile_scan_kernel, dim3(1), dim3(BLOCK), 0, st, ltiles, T_e, &lw->n_links, &lw->unused);
        KT_HIP(hipGetLastError());
        KT_HIP(hipMemcpyAsync(&hl, lw, sizeof(LinkWords), hipMemcpyDeviceToHost, st));
        KT_HIP(hipStreamSynchronize(st));
        *n_links = hl.n_links;
    }
    *n_unitigs = h.n_unitigs, *n_bases = h.n_bases;
    if (!store) return KT_OK;
    if (tr) max_unitigs = nu, max_links = hl.n_links;  // (everything is made, in this call's scratch; max_bases stays 0)
    if (!tr && linked && (h.n_unitigs > max_unitigs || h.n_bases > max_bases || hl.n_links > max_links))
        return call.fail("max_unitigs, max_bases or max_links smaller than the result (*n_unitigs, *n_bases, *n_links)");
    if (!tr && (h.n_unitigs > max_unitigs || h.n_bases > max_bases))
        return call.fail("max_unitigs or max_bases smaller than the result (*n_unitigs, *n_bases)");

    // e. spelling (host: into OFFSETS = offsets | count sums | flags | bases | link offsets | links, copied back by finish())
    uint8_t *d_bases = bases;
    uint64_t *d_offsets = offsets, *d_sums = count_sums;
    uint32_t *d_flags = flags;
    uint64_t *d_loff = link_offsets;
    uint32_t *d_lto = link_to;
    const uint64_t spelled = tr ? 0 : h.n_bases;  // a tip run reads lengths, count sums, flags and links: it writes no base
    if (call.host() || tr) {
        const size_t unlinked = (nu + 1) * 8 + nu * 8 + align16(nu * 4) + spelled;
        const size_t all = linked ? align16(unlinked) + (n_ends + 1) * 8 + hl.n_links * 4 : unlinked;
        if (int rc = call.scratch(kt::OFFSETS, all, &d_offsets)) return rc;
        d_sums = count_sums || tr ? d_offsets + nu + 1 : nullptr;
        d_flags = flags || tr ? (uint32_t *)(d_offsets + 2 * nu + 1) : nullptr;
        d_bases = (uint8_t *)(d_offsets + 2 * nu + 1) + align16(nu * 4);
        d_loff = (uint64_t *)((uint8_t *)d_offsets + align16(unlinked));
        d_lto = (uint32_t *)(d_loff + n_ends + 1);
    }
    if (d_sums) KT_HIP(hipMemsetAsync(d_sums, 0, nu * 8, st));
    const SpellArgs sp{keys, counts, place, slen, ex_id, ex_off, n, k, d_bases, d_offsets, d_sums, d_flags, spelled, nu, w};
    hipLaunchKernelGGL(unitig_spell_kernel, blocks_for(n), dim3(BLOCK), 0, st, sp);
    KT_HIP(hipGetLastError());
    call.back(bases, (const uint8_t *)d_bases, h.n_bases);
    call.back(offsets, (const uint64_t *)d_offsets, nu + 1);
    call.back(count_sums, (const uint64_t *)d_sums, nu);
    call.back(flags, (const uint32_t *)d_flags, nu);
    if (linked) {
        // g. the offsets from the degrees, then the links; the one thing left to learn is whether every neighbour stood
        // where the rule puts it
        la.link_offsets = d_loff, la.link_to = d_lto, la.max_links = hl.n_links;
        hipLaunchKernelGGL(unitig_end_scan_apply_kernel, dim3((uint32_t)T_e), dim3(BLOCK), 0, st, (const uint32_t *)la.deg, n_ends,
                           (const uint64_t *)ltiles, (const LinkWords *)lw, d_loff);
        if (hl.n_links) hipLaunchKernelGGL(unitig_end_emit_kernel, blocks_for(m), dim3(BLOCK), 0, st, la);
        KT_HIP(hipGetLastError());
        KT_HIP(hipMemcpyAsync(&h, w, sizeof(Words), hipMemcpyDeviceToHost, st));
        KT_HIP(hipStreamSynchronize(st));
        if (h.err)
            return kt::fail(KT_ERR_HIP, std::string(name) + ": internal: a unitig end's neighbour is not at an end of its own "
                                                            "unitig (error bits " + std::to_string(h.err) + ")");
        call.back(link_offsets, (const uint64_t *)d_loff, n_ends + 1);
        call.back(link_to, (const uint32_t *)d_lto, hl.n_links);
    }
    if (tr) return tip_stages(call, ctx, TipArgs{d_offsets, d_sums, d_flags, d_loff, d_lto, nu, k, tr->max_tip_nodes}, keys, place, ex_id, n, tr);
    return call.finish();
}

}  // namespace

extern "C" int kt_ctr_unitigs(kt_ctr *table, uint32_t min_count, uint32_t max_count, uint8_t *bases, uint64_t max_bases,
                              uint64_t *offsets, uint64_t *count_sums, uint32_t *flags, uint64_t max_unitigs, uint64_t *n_unitigs,
                              uint64_t *n_bases, int mem) {
    if (!table || !n_unitigs || !n_bases) return kt::fail(KT_ERR_ARG, "kt_ctr_unitigs: null");
    Call call(table->ctx, mem, "kt_ctr_unitigs");
    return unitigs_run(call, "kt_ctr_unitigs", table, min_count, max_count, bases, max_bases, offsets, count_sums, flags, max_unitigs,
                       n_unitigs, n_bases, nullptr, nullptr, 0, nullptr, nullptr);
}

extern "C" int kt_ctr_unitigs_linked(kt_ctr *table, uint32_t min_count, uint32_t max_count, uint8_t *bases, uint64_t max_bases,
                                     uint64_t *offsets, uint64_t *count_sums, uint32_t *flags, uint64_t max_unitigs,
                                     uint64_t *n_unitigs, uint64_t *n_bases, uint64_t *link_offsets, uint32_t *link_to,
                                     uint64_t max_links, uint64_t *n_links, int mem) {
    if (!table || !n_unitigs || !n_bases || !n_links) return kt::fail(KT_ERR_ARG, "kt_ctr_unitigs_linked: null");
    Call call(table->ctx, mem, "kt_ctr_unitigs_linked");
    return unitigs_run(call, "kt_ctr_unitigs_linked", table, min_count, max_count, bases, max_bases, offsets, count_sums, flags,
                       max_unitigs, n_unitigs, n_bases, link_offsets, link_to, max_links, n_links, nullptr);
}

extern "C" int kt_ctr_unitig_tips(kt_ctr *table, uint32_t min_count, uint32_t max_count, uint32_t max_tip_nodes, uint8_t *marks,
                                  uint64_t max_unitigs, uint64_t *n_unitigs, uint64_t *tally, int mem) {
    if (!table || !n_unitigs) return kt::fail(KT_ERR_ARG, "kt_ctr_unitig_tips: null");
    kt_ctx *ctx = table->ctx;
    Call call(ctx, mem, "kt_ctr_unitig_tips");
    if (int rc = call.enter()) return rc;
    if (max_tip_nodes == 0) return call.fail("max_tip_nodes must be >= 1");
    if (max_unitigs && !marks) return call.fail("null marks");
    // the run works in device memory whatever `mem` is: only the marks and the tally go to the caller
    Call run(ctx, KT_MEM_DEVICE, "kt_ctr_unitig_tips");
    TipRun tr{max_tip_nodes, 0u};
    uint64_t nu = 0, nb = 0, nl = 0;
    if (int rc = unitigs_run(run, "kt_ctr_unitig_tips", table, min_count, max_count, nullptr, 0, nullptr, nullptr, nullptr, 0, &nu, &nb,
                             nullptr, nullptr, 0, &nl, &tr))
        return rc;
    *n_unitigs = tr.nu;
    if (max_unitigs && max_unitigs < tr.nu) return call.fail("max_unitigs smaller than the result (*n_unitigs)");
    if (call.host()) {
        if (max_unitigs) call.back(marks, tr.d_marks, tr.nu);
        if (tally)
            for (int j = 0; j < KT_TIP_TALLY; j++) tally[j] = tr.tally[j];
        return call.finish();
    }
    if (max_unitigs && tr.nu) KT_HIP(hipMemcpyAsync(marks, tr.d_marks, tr.nu, hipMemcpyDeviceToDevice, ctx->stream));
    if (tally) {
        if (tr.d_words) KT_HIP(hipMemcpyAsync(tally, tr.d_words, KT_TIP_TALLY * 8, hipMemcpyDeviceToDevice, ctx->stream));
        else KT_HIP(hipMemsetAsync(tally, 0, KT_TIP_TALLY * 8, ctx->stream));
    }
    return KT_OK;
}

extern "C" int kt_ctr_clip_tips(kt_ctr *table, uint32_t min_count, uint32_t max_count, uint32_t max_tip_nodes, uint32_t max_rounds,
                                uint32_t flags, uint64_t *stats) {
    if (!table) return kt::fail(KT_ERR_ARG, "kt_ctr_clip_tips: null");
    kt_ctx *ctx = table->ctx;
    Call call(ctx, KT_MEM_DEVICE, "kt_ctr_clip_tips");
    if (max_tip_nodes == 0) return call.fail("max_tip_nodes must be >= 1");
    if (max_rounds < 1 || max_rounds > 1024) return call.fail("max_rounds must be in 1..1024");
    if (flags & ~KT_CLIP_ISOLATED) return call.fail("unknown flags");
    const bool drop = flags & KT_CLIP_ISOLATED;
    uint64_t s[KT_CLIP_STATS] = {};
    auto leave = [&](int rc) {
        if (stats)
            for (int j = 0; j < KT_CLIP_STATS; j++) stats[j] = s[j];
        return rc;
    };
    for (uint32_t r = 0; r < max_rounds; r++) {
        TipRun tr{max_tip_nodes, (uint32_t)KT_TIP_TIP | (drop ? (uint32_t)KT_TIP_ISOLATED : 0u)};
        uint64_t nu = 0, nb = 0, nl = 0;
        if (int rc = unitigs_run(call, "kt_ctr_clip_tips", table, min_count, max_count, nullptr, 0, nullptr, nullptr, nullptr, 0, &nu,
                                 &nb, nullptr, nullptr, 0, &nl, &tr))
            return r ? leave(rc) : rc;  // (an argument the first round refuses leaves stats untouched, as every refusal does)
        const uint64_t want = tr.tally[1] + (drop ? tr.tally[3] : 0);
        if (!want) {
            s[6] = 0;
            break;
        }
        // the list (in OUT) is all the erase reads: the run's other buffers are its to take, behind the run's kernels on the stream
        for (kt::Buf b : {kt::BASES, kt::OFFSETS, kt::AUX0, kt::AUX1, kt::AUX2}) ctx->unclaim(b);
        uint64_t gone = 0;
        if (int rc = kt_ctr_erase(table, tr.d_list, tr.n_list, &gone, KT_MEM_DEVICE)) return leave(rc);
        s[0]++, s[1] += tr.tally[0], s[2] += tr.tally[1], s[5] += tr.tally[4];
        if (drop) s[3] += tr.tally[2], s[4] += tr.tally[3], s[5] += tr.tally[5];
        s[6] = 1;
        if (gone != want)
            return leave(kt::fail(KT_ERR_HIP, "kt_ctr_clip_tips: internal: the table held " + std::to_string(gone) + " of the " +
                                                  std::to_string(want) + " nodes to erase"));
        call.release();
    }
    return leave(KT_OK);
}
