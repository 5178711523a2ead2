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
// kt_ctr_unitig_bubbles and kt_ctr_simplify run the same round with one more rule, alone or behind stage i on the stream:
//   k. bubbles   one thread per unitig: a branch (no cycle, at most max_bubble_nodes nodes, exactly one link at either end,
//                neither to itself) looks through the at most 5 links of the end its + link arrives at for branches between
//                the same two ends, and is popped when one of them outranks it (a higher mean count as 128-bit products,
//                then the lower number); its bit is ORed into the unitig's mark, so that stage j lists tips and popped
//                branches in one pass; no class array - the predicate is a handful of loads, made again for a neighbour
// Anything the rule excludes (a link without an answer, a neighbour that is no node, a chain that is neither a path nor a
// cycle) raises a bit in the call's error word and comes back as an error: nothing spins.
// On the host a call is a Run: its methods are the stages - nodes (a), chains (b to d), degrees (f), spell (e), emit (g),
// marks (h to k) - and every entry point says which of them it runs, and into which Outputs.
#include "kt_device.hpp"
#include "kt_launch.hpp"
#include "kt_scan.hpp"

namespace {

using namespace ktl;

constexpr int BLOCK = 256;
constexpr uint32_t NIL = 0xFFFFFFFFu;
static_assert(BLOCK == SCAN_BLOCK, "the scans of kt_scan.hpp run in this file's workgroups");
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

// a start node's unitig: 1 unitig, nodes + k - 1 bases
__device__ __forceinline__ uint64_t bases_of(uint32_t sl, uint32_t k) { return sl ? (uint64_t)(sl & ~CIRC) + k - 1u : 0ull; }

// The exclusive scan over n items, two sums at once, is written once over a functor F: word(i) is item i's one u32,
// add(word, a, b) what it contributes to the two sums (word 0, the filler past n, contributes nothing), put(i, a, b) takes
// the sums over the items before i, total() is thread 0's after the last put.  Three launches: the tiles' sums, one
// workgroup over those, and the tiles again (kt_scan.hpp).

// stage d, over nodes: (is start, bases) -> ex_id[i], ex_off[i] = unitigs and bases that start at nodes before i
struct NodeScan {
    const uint32_t *slen;
    uint32_t k;
    uint32_t *ex_id;
    uint64_t *ex_off;
    __device__ __forceinline__ uint32_t word(uint64_t i) const { return slen[i]; }
    __device__ __forceinline__ void add(uint32_t sl, uint64_t &a, uint64_t &b) const { a += sl != 0u, b += bases_of(sl, k); }
    __device__ __forceinline__ void put(uint64_t i, uint64_t a, uint64_t b) const { ex_id[i] = (uint32_t)a, ex_off[i] = b; }
    __device__ __forceinline__ void total() const {}
};

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

// stage f / g, over ends: the degree -> link_offsets[e] = the links of the ends before e, link_offsets[n_ends] = all of them.
// The second sum stays 0: the workgroup scan over a ktd::sum2 and the one-workgroup tile scan are stage d's, and carry two.
struct EndScan {
    const uint32_t *deg;
    uint64_t n_ends;
    const LinkWords *lw;
    uint64_t *link_offsets;
    __device__ __forceinline__ uint32_t word(uint64_t e) const { return deg[e]; }
    __device__ __forceinline__ void add(uint32_t d, uint64_t &a, uint64_t &) const { a += d; }
    __device__ __forceinline__ void put(uint64_t e, uint64_t a, uint64_t) const { link_offsets[e] = a; }
    __device__ __forceinline__ void total() const { link_offsets[n_ends] = lw->n_links; }
};

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
// ... and behind them, in a round with the bubble rule: tally[0..4) as kt_ctr_unitig_bubbles gives them
constexpr int BUBBLE_WORDS = 4, ROUND_WORDS = TIP_WORDS + BUBBLE_WORDS;
constexpr uint8_t CLS_NONE = 0, CLS_LIVE_PLUS = 1, CLS_LIVE_MINUS = 2, CLS_ISOLATED = 3;

// one marking round, as its callers ask for it and as it comes back
struct TipRun {
    uint32_t max_tip_nodes;         // 0: no tip rule (no stages h and i)
    uint32_t erase_marks;           // kt_ctr_clip_tips, kt_ctr_simplify: the marks (bits) whose nodes stage j lists; 0: no stage j
    uint32_t max_bubble_nodes = 0;  // 0: no bubble rule (no stage k)
    uint64_t nu = 0;                // unitigs
    uint64_t tally[ROUND_WORDS] = {};  // (the bubble words stay 0 in a round without the rule)
    uint8_t *d_marks = nullptr;             // nu marks, in OUT
    unsigned long long *d_words = nullptr;  // the tally on the device
    uint64_t *d_list = nullptr;             // stage j: n_list keys, KT_EMPTY_KEY for a node that stays, in OUT
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
        v[j] = ktd::wave_sum(v[j]);
        if ((threadIdx.x & 63) == 0 && v[j]) atomicAdd(words + j, (unsigned long long)v[j]);
    }
}

// k. u is a branch: *la, *lb = the one link of its + end and of its - end
__device__ __forceinline__ bool bubble_branch(const TipArgs &a, uint32_t max_bubble_nodes, uint64_t u, uint32_t *la, uint32_t *lb) {
    if ((a.flags[u] & KT_UNITIG_CIRCULAR) || nodes_of(a, u) > (uint64_t)max_bubble_nodes) return false;
    const uint64_t l0 = a.link_offsets[2 * u], l1 = a.link_offsets[2 * u + 1], l2 = a.link_offsets[2 * u + 2];
    if (l1 - l0 != 1 || l2 - l1 != 1) return false;
    *la = a.link_to[l0], *lb = a.link_to[l1];
    return (*la >> 1) != u && (*lb >> 1) != u;
}

// k. one thread per unitig: a branch u with links a and b looks at the links h of end a ^ 1 (its own mirror 2u + 1 among them);
// w = h >> 1 is parallel when it is a branch whose end h ^ 1 links to a (the mirror of h) and whose end h links to b; u is
// popped when a parallel w outranks it, and counts the bubble when it has a parallel branch and none outranks it.  ORs
// KT_BUBBLE_POP into marks[u]; words = the round's bubble words
__global__ __launch_bounds__(BLOCK) void unitig_bubble_mark_kernel(TipArgs a, uint32_t max_bubble_nodes, uint8_t *__restrict__ marks,
                                                                   unsigned long long *__restrict__ words) {
    const uint64_t u = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
    bool found = false, popped = false;  // (every lane stays for the wave's sums)
    uint32_t la = 0, lb = 0;
    uint64_t c_u = 0, n_u = 0;
    if (u < a.nu && bubble_branch(a, max_bubble_nodes, u, &la, &lb) && (la ^ 1u) < 2 * a.nu) {
        c_u = a.count_sums[u], n_u = nodes_of(a, u);
        const uint64_t g = la ^ 1u;
        for (uint64_t y = a.link_offsets[g]; y < a.link_offsets[g + 1]; y++) {
            const uint32_t h = a.link_to[y];
            const uint64_t w = h >> 1;
            uint32_t wa, wb;
            if (w == u || w >= a.nu || !bubble_branch(a, max_bubble_nodes, w, &wa, &wb)) continue;
            if ((h & 1u ? wa : wb) != la || (h & 1u ? wb : wa) != lb) continue;  // the links of ends h ^ 1 and h
            found = true;
            const uint64_t c_w = a.count_sums[w], n_w = nodes_of(a, w);
            const uint64_t lh = __umul64hi(c_w, n_u), ll = c_w * n_u, rh = __umul64hi(c_u, n_w), rl = c_u * n_w;
            popped = popped || (lh != rh ? lh > rh : ll != rl ? ll > rl : w < u);
        }
    }
    if (popped) marks[u] |= KT_BUBBLE_POP;
    // the tally: summed over the wave, one atomic per word and wave that has something to add
    uint64_t v[BUBBLE_WORDS] = {popped, popped ? n_u : 0, found && !popped, popped ? c_u : 0};
#pragma unroll
    for (int j = 0; j < BUBBLE_WORDS; j++) {
        v[j] = ktd::wave_sum(v[j]);
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

// ---- the stages on the host -------------------------------------------------------------------------------------------

// where stages e and g write, on the device; max_bases = the bases there is room for (0: none is spelled)
struct Outputs {
    uint8_t *bases;
    uint64_t *offsets, *count_sums;
    uint32_t *flags;
    uint64_t *link_offsets;
    uint32_t *link_to;
    uint64_t max_bases;
    // all six made in OFFSETS = offsets | count sums | flags | bases | link offsets | links (n_ends 0: no link arrays)
    int carve(Call &call, uint64_t nu, uint64_t spelled, uint64_t n_ends, uint64_t n_links) {
        const size_t unlinked = (nu + 1) * 8 + nu * 8 + align16(nu * 4) + spelled;
        if (int rc = call.scratch(kt::OFFSETS, n_ends ? align16(unlinked) + (n_ends + 1) * 8 + n_links * 4 : unlinked, &offsets)) return rc;
        count_sums = offsets + nu + 1;
        flags = (uint32_t *)(offsets + 2 * nu + 1);
        bases = (uint8_t *)flags + align16(nu * 4);
        link_offsets = (uint64_t *)((uint8_t *)offsets + align16(unlinked));
        link_to = (uint32_t *)(link_offsets + n_ends + 1);
        max_bases = spelled;
        return KT_OK;
    }
};

// One run of the stages under an entry point's `call`: a method is a stage, and leaves here and on the device what the later
// ones read.  The entry points below say which stages they run.
struct Run {
    Call &call;
    const char *name;
    kt_ctr *table;
    uint32_t min_count, max_count;
    hipStream_t st = table->ctx->stream;
    uint32_t k = (uint32_t)table->k;
    // a: the nodes, ascending by key, in AUX1 (16 bytes an entry of the table)
    uint64_t *keys = nullptr, n = 0;
    uint32_t *info = nullptr, *counts = nullptr;
    // b to d: what the later stages keep per node, in AUX2 (64 bytes a node), and the call's words as last read back
    Words *w = nullptr, h{};
    uint32_t *link = nullptr, *slen = nullptr, *ex_id = nullptr;
    uint2 *place = nullptr;
    uint64_t *ex_off = nullptr, *tiles = nullptr, nu = 0, n_bases = 0;
    // f: the link words, the ends' degrees and their tiles, in AUX0 (8 bytes a unitig)
    LinkWords *lw = nullptr;
    uint32_t *deg = nullptr;
    uint64_t *ltiles = nullptr, n_ends = 0, n_links = 0;

    // the checks every entry point makes first
    int begin() {
        if (int rc = call.refuse_shard(table)) return rc;
        if (min_count == 0) return call.fail("min_count must be >= 1");
        if (min_count > max_count) return call.fail("min_count > max_count");
        return call.enter();
    }
    // a read-back behind everything queued so far, and a wait for it
    int fetch(void *host, const void *dev, size_t bytes) {
        KT_HIP(hipGetLastError());
        KT_HIP(hipMemcpyAsync(host, dev, bytes, hipMemcpyDeviceToHost, st));
        KT_HIP(hipStreamSynchronize(st));
        return KT_OK;
    }
    // ... of the words: an error bit in them is the call's error, `what` its text
    int check_words(const char *what) {
        if (int rc = fetch(&h, w, sizeof(Words))) return rc;
        return h.err ? kt::fail(KT_ERR_HIP, std::string(name) + ": internal: " + what + " (error bits " + std::to_string(h.err) + ")") : KT_OK;
    }
    // a. n = 0: no node, and for an empty table nothing claimed or launched (kt_ctr_graph's sort takes OUT and AUX0)
    int nodes() {
        uint64_t n_t = 0;
        if (int rc = kt_ctr_size(table, &n_t)) return rc;  // (KT_ERR_FULL for an overflowed table)
        if (n_t > 0x7FFFFFFEull) return call.fail("a table of more than 2^31 - 2 entries (the oriented node states are u32)");
        if (!n_t) return KT_OK;
        if (int rc = carve(call, kt::AUX1, &keys, n_t, &info, n_t, &counts, n_t)) return rc;
        return kt_ctr_graph(table, min_count, max_count, keys, info, counts, n_t, &n, nullptr, KT_MEM_DEVICE, 1);
    }
    // b to d, for n > 0: nu and n_bases
    int chains() {
        const uint64_t m = 2 * n;
        const dim3 M = blocks_for(m), B(BLOCK);
        uint64_t *ra = nullptr, *rb = nullptr;
        if (int rc = carve(call, kt::AUX2, &w, 1, &link, m, &ra, m, &rb, m, &place, n, &slen, n, &ex_id, n, &ex_off, n, &tiles, 2 * scan2_tiles(n)))
            return rc;
        KT_HIP(hipMemsetAsync(w, 0, sizeof(Words), st));
        // b. links
        hipLaunchKernelGGL(unitig_link_kernel, M, B, 0, st, keys, info, n, k, link, w);
        // c. ranking: a number of rounds fixed by n
        hipLaunchKernelGGL(unitig_rank_init_kernel, M, B, 0, st, link, m, ra, w);
        for (uint32_t r = 0, rounds = ceil_log2(m) + 1u; r < rounds; r++) {
            hipLaunchKernelGGL(unitig_rank_jump_kernel, M, B, 0, st, ra, m, rb);
            std::swap(ra, rb);
        }
        hipLaunchKernelGGL(unitig_unresolved_kernel, M, B, 0, st, ra, link, m, w);
        if (int rc = fetch(&h, w, sizeof(Words))) return rc;
        uint64_t *cval = nullptr;
        if (h.unresolved && !h.err) {  // cycles: the smallest state of each, and every state's distance to it, in BASES (48 bytes a node)
            uint64_t *vb = nullptr;
            uint32_t *na = nullptr, *nc = nullptr;
            if (int rc = carve(call, kt::BASES, &cval, m, &vb, m, &na, m, &nc, m)) return rc;
            hipLaunchKernelGGL(unitig_cycle_init_kernel, M, B, 0, st, ra, link, m, cval, na);
            for (uint32_t r = 0, rounds = ceil_log2(n); r < rounds; r++) {
                hipLaunchKernelGGL(unitig_cycle_jump_kernel, M, B, 0, st, cval, na, m, 1ull << r, vb, nc);
                std::swap(cval, vb), std::swap(na, nc);
            }
        }
        // d. placing, ids and offsets
        hipLaunchKernelGGL(unitig_place_kernel, blocks_for(n), B, 0, st, ra, link, cval, n, place, slen, w);
        const NodeScan scan{slen, k, ex_id, ex_off};
        if (int rc = scan2_sums(st, scan, n, tiles, &w->n_unitigs, &w->n_bases)) return rc;
        if (int rc = scan2_apply(st, scan, n, tiles)) return rc;
        if (int rc = check_words("the nodes' links do not form paths and cycles")) return rc;
        nu = h.n_unitigs, n_bases = h.n_bases;
        return KT_OK;
    }
    // f. the ends' degrees and their sum (the graph's sort has given AUX0 back): n_ends and n_links
    int degrees() {
        n_ends = 2 * nu;
        const dim3 B(BLOCK);
        if (int rc = carve(call, kt::AUX0, &lw, 1, &deg, n_ends, &ltiles, 2 * scan2_tiles(n_ends))) return rc;
        KT_HIP(hipMemsetAsync(lw, 0, (uint8_t *)ltiles - (uint8_t *)lw, st));
        hipLaunchKernelGGL(unitig_end_degree_kernel, blocks_for(2 * n), B, 0, st, link_args(Outputs{}));
        if (int rc = scan2_sums(st, EndScan{deg, n_ends, lw, nullptr}, n_ends, ltiles, &lw->n_links, &lw->unused)) return rc;
        return fetch(&n_links, &lw->n_links, 8);
    }
    LinkArgs link_args(const Outputs &o) const {  // (f writes deg and reads no output; max_links guards g's stores)
        return LinkArgs{keys, info, place, slen, ex_id, n, n_ends, k, deg, o.link_offsets, o.link_to, n_links, w};
    }
    // host: e and g write into arrays made in OFFSETS instead of the caller's (*o as it comes), the optional ones only where the
    // caller has one, and finish() copies them there
    int stage(Outputs *o) {
        if (!call.host()) return KT_OK;
        const Outputs user = *o;
        if (int rc = o->carve(call, nu, n_bases, n_ends, n_links)) return rc;
        if (!user.count_sums) o->count_sums = nullptr;
        if (!user.flags) o->flags = nullptr;
        call.back(user.bases, o->bases, n_bases), call.back(user.offsets, o->offsets, nu + 1);
        call.back(user.count_sums, o->count_sums, nu), call.back(user.flags, o->flags, nu);
        call.back(user.link_offsets, o->link_offsets, n_ends + 1), call.back(user.link_to, o->link_to, n_links);
        return KT_OK;
    }
    // e. spelling (max_bases and nu guard the stores: the entry points launch this only when everything fits)
    int spell(const Outputs &o) {
        if (o.count_sums) KT_HIP(hipMemsetAsync(o.count_sums, 0, nu * 8, st));
        const SpellArgs sp{keys, counts, place, slen, ex_id, ex_off, n, k, o.bases, o.offsets, o.count_sums, o.flags, o.max_bases, nu, w};
        hipLaunchKernelGGL(unitig_spell_kernel, blocks_for(n), dim3(BLOCK), 0, st, sp);
        KT_HIP(hipGetLastError());
        return KT_OK;
    }
    // g. the offsets from the degrees, then the links; the one thing left to learn is whether every neighbour stood where the
    // rule puts it
    int emit(const Outputs &o) {
        const EndScan scan{deg, n_ends, lw, o.link_offsets};
        if (int rc = scan2_apply(st, scan, n_ends, ltiles)) return rc;
        if (n_links) hipLaunchKernelGGL(unitig_end_emit_kernel, blocks_for(2 * n), dim3(BLOCK), 0, st, link_args(o));
        return check_words("a unitig end's neighbour is not at an end of its own unitig");
    }
    // no node: offsets[0] and link_offsets[0] = 0, in a call that has room for them
    int zero(std::initializer_list<uint64_t *> firsts) {
        for (uint64_t *first : firsts)
            if (call.host()) *first = 0;
            else KT_HIP(hipMemsetAsync(first, 0, 8, st));
        return KT_OK;
    }
    // h to k behind e and g, in OUT (the graph's sort has given it back): words | classes | marks | list.  The tip rule (h, i)
    // where tip->max_tip_nodes, the bubble rule (k) where tip->max_bubble_nodes - behind i on the stream, or over zeroed marks -
    // and one list (j) of the union; the tip rule alone claims and launches what it always did
    int marks(const Outputs &o, TipRun *tip) {
        const TipArgs a{o.offsets, o.count_sums, o.flags, o.link_offsets, o.link_to, nu, k, tip->max_tip_nodes};
        const dim3 U = blocks_for(nu), B(BLOCK);
        const bool tips = tip->max_tip_nodes != 0, bubbles = tip->max_bubble_nodes != 0;
        const uint64_t words = bubbles ? ROUND_WORDS : TIP_WORDS;
        uint8_t *cls = nullptr;
        tip->nu = nu, tip->n_list = tip->erase_marks ? n : 0;
        if (int rc = carve(call, kt::OUT, &tip->d_words, words, &cls, tips ? nu : 0, &tip->d_marks, nu, &tip->d_list, tip->n_list)) return rc;
        KT_HIP(hipMemsetAsync(tip->d_words, 0, words * 8, st));
        if (tips) {
            hipLaunchKernelGGL(unitig_tip_class_kernel, U, B, 0, st, a, cls);
            hipLaunchKernelGGL(unitig_tip_mark_kernel, U, B, 0, st, a, cls, tip->d_marks, tip->d_words);
        } else {
            KT_HIP(hipMemsetAsync(tip->d_marks, 0, nu, st));
        }
        if (bubbles) hipLaunchKernelGGL(unitig_bubble_mark_kernel, U, B, 0, st, a, tip->max_bubble_nodes, tip->d_marks, tip->d_words + TIP_WORDS);
        if (tip->n_list)
            hipLaunchKernelGGL(unitig_tip_list_kernel, blocks_for(n), B, 0, st, keys, place, ex_id, n, tip->d_marks, nu, tip->erase_marks,
                               tip->d_list);
        return fetch(tip->tally, tip->d_words, words * 8);
    }
};

// One marking round under the device call `call`: the linked stages with offsets, count sums, flags and links made in OFFSETS
// and no base written, then h to k as *tip asks.  No node: *tip as it came.
int tip_round(Call &call, const char *name, kt_ctr *table, uint32_t min_count, uint32_t max_count, TipRun *tip) {
    Run r{call, name, table, min_count, max_count};
    if (int rc = r.begin()) return rc;
    if (int rc = r.nodes()) return rc;
    if (!r.n) return KT_OK;
    if (int rc = r.chains()) return rc;
    if (int rc = r.degrees()) return rc;
    Outputs o{};
    if (int rc = o.carve(call, r.nu, 0, r.n_ends, r.n_links)) return rc;
    if (int rc = r.spell(o)) return rc;
    if (int rc = r.emit(o)) return rc;
    return r.marks(o, tip);
}

// kt_ctr_unitig_tips and kt_ctr_unitig_bubbles: one round of the one rule `tr` asks for, read-only; the marks and the
// `count` words from `first` of the round's words go to the caller.  `refusal`: what is wrong with the rule's argument, or null.
int mark_call(const char *name, kt_ctr *table, uint32_t min_count, uint32_t max_count, TipRun tr, const char *refusal, int first,
              int count, uint8_t *marks, uint64_t max_unitigs, uint64_t *n_unitigs, uint64_t *tally, int mem) {
    if (!table || !n_unitigs) return kt::fail(KT_ERR_ARG, std::string(name) + ": null");
    kt_ctx *ctx = table->ctx;
    Call call(ctx, mem, name);
    if (int rc = call.enter()) return rc;
    if (refusal) return call.fail(refusal);
    if (max_unitigs && !marks) return call.fail("null marks");
    // the run works in device memory whatever `mem` is: only the marks and the tally go to the caller
    Call run(ctx, KT_MEM_DEVICE, name);
    if (int rc = tip_round(run, name, table, min_count, max_count, &tr)) return rc;
    *n_unitigs = tr.nu;
    if (max_unitigs && max_unitigs < tr.nu) return call.fail("max_unitigs smaller than the result (*n_unitigs)");
    if (call.host()) {
        if (max_unitigs) call.back(marks, tr.d_marks, tr.nu);
        if (tally)
            for (int j = 0; j < count; j++) tally[j] = tr.tally[first + j];
        return call.finish();
    }
    if (max_unitigs && tr.nu) KT_HIP(hipMemcpyAsync(marks, tr.d_marks, tr.nu, hipMemcpyDeviceToDevice, ctx->stream));
    if (tally) {
        if (tr.d_words) KT_HIP(hipMemcpyAsync(tally, tr.d_words + first, count * 8, hipMemcpyDeviceToDevice, ctx->stream));
        else KT_HIP(hipMemsetAsync(tally, 0, count * 8, ctx->stream));
    }
    return KT_OK;
}

// kt_ctr_clip_tips and kt_ctr_simplify: mark, list, erase, again - under the caller's `call`, its arguments checked.  s: the
// stats as kt_ctr_simplify gives them.  *told = s describes what was done (not so when round 0 refuses its arguments).
int erase_rounds(Call &call, const char *name, kt_ctr *table, uint32_t min_count, uint32_t max_count, uint32_t max_tip_nodes,
                 uint32_t max_bubble_nodes, uint32_t max_rounds, bool drop, uint64_t *s, bool *told) {
    kt_ctx *ctx = table->ctx;
    *told = true;
    for (uint32_t r = 0; r < max_rounds; r++) {
        TipRun tr{max_tip_nodes, (max_tip_nodes ? (uint32_t)KT_TIP_TIP : 0u) | (drop ? (uint32_t)KT_TIP_ISOLATED : 0u) |
                                     (max_bubble_nodes ? (uint32_t)KT_BUBBLE_POP : 0u),
                  max_bubble_nodes};
        if (int rc = tip_round(call, name, table, min_count, max_count, &tr)) {
            *told = r != 0;  // (an argument the first round refuses leaves stats untouched, as every refusal does)
            return rc;
        }
        const uint64_t *t = tr.tally, *b = tr.tally + TIP_WORDS;
        const uint64_t want = t[1] + (drop ? t[3] : 0) + b[1];
        if (!want) {
            s[9] = 0;
            break;
        }
        // the list (in OUT) is all the erase reads: the run's other buffers are its to take, behind the run's kernels on the stream
        for (kt::Buf buf : {kt::BASES, kt::OFFSETS, kt::AUX0, kt::AUX1, kt::AUX2}) ctx->unclaim(buf);
        uint64_t gone = 0;
        if (int rc = kt_ctr_erase(table, tr.d_list, tr.n_list, &gone, KT_MEM_DEVICE)) return rc;
        s[0]++, s[1] += t[0], s[2] += t[1], s[8] += t[4] + b[3];
        if (drop) s[3] += t[2], s[4] += t[3], s[8] += t[5];
        s[5] += b[0], s[6] += b[1], s[7] += b[2];
        s[9] = 1;
        if (gone != want)
            return kt::fail(KT_ERR_HIP, std::string(name) + ": internal: the table held " + std::to_string(gone) + " of the " +
                                            std::to_string(want) + " nodes to erase");
        call.release();
    }
    return KT_OK;
}

}  // namespace

extern "C" int kt_ctr_unitigs(kt_ctr *table, uint32_t min_count, uint32_t max_count, uint8_t *bases, uint64_t max_bases,
                              uint64_t *offsets, uint64_t *count_sums, uint32_t *flags, uint64_t max_unitigs, uint64_t *n_unitigs,
                              uint64_t *n_bases, int mem) {
    if (!table || !n_unitigs || !n_bases) return kt::fail(KT_ERR_ARG, "kt_ctr_unitigs: null");
    Call call(table->ctx, mem, "kt_ctr_unitigs");
    Run r{call, "kt_ctr_unitigs", table, min_count, max_count};
    if (int rc = r.begin()) return rc;
    const bool store = max_bases || max_unitigs;
    if ((max_bases && !bases) || (store && !offsets)) return call.fail("null output");
    if (int rc = r.nodes()) return rc;
    if (r.n)
        if (int rc = r.chains()) return rc;
    *n_unitigs = r.nu, *n_bases = r.n_bases;
    if (!store) return KT_OK;
    if (!r.n) return r.zero({offsets});
    if (r.nu > max_unitigs || r.n_bases > max_bases)
        return call.fail("max_unitigs or max_bases smaller than the result (*n_unitigs, *n_bases)");
    Outputs o{bases, offsets, count_sums, flags, nullptr, nullptr, r.n_bases};
    if (int rc = r.stage(&o)) return rc;
    if (int rc = r.spell(o)) return rc;
    return call.finish();
}

extern "C" int kt_ctr_unitigs_linked(kt_ctr *table, uint32_t min_count, uint32_t max_count, uint8_t *bases, uint64_t max_bases,
                                     uint64_t *offsets, uint64_t *count_sums, uint32_t *flags, uint64_t max_unitigs,
                                     uint64_t *n_unitigs, uint64_t *n_bases, uint64_t *link_offsets, uint32_t *link_to,
                                     uint64_t max_links, uint64_t *n_links, int mem) {
    if (!table || !n_unitigs || !n_bases || !n_links) return kt::fail(KT_ERR_ARG, "kt_ctr_unitigs_linked: null");
    Call call(table->ctx, mem, "kt_ctr_unitigs_linked");
    Run r{call, "kt_ctr_unitigs_linked", table, min_count, max_count};
    if (int rc = r.begin()) return rc;
    const bool store = max_bases || max_unitigs || max_links;
    if ((max_bases && !bases) || (store && !offsets)) return call.fail("null output");
    if ((store && !link_offsets) || (max_links && !link_to)) return call.fail("null link output");
    if (max_links && !max_unitigs) return call.fail("max_links > 0 with max_unitigs == 0");
    if (int rc = r.nodes()) return rc;
    if (r.n) {
        if (int rc = r.chains()) return rc;
        if (int rc = r.degrees()) return rc;
    }
    *n_unitigs = r.nu, *n_bases = r.n_bases, *n_links = r.n_links;
    if (!store) return KT_OK;
    if (!r.n) return r.zero({offsets, link_offsets});
    if (r.nu > max_unitigs || r.n_bases > max_bases || r.n_links > max_links)
        return call.fail("max_unitigs, max_bases or max_links smaller than the result (*n_unitigs, *n_bases, *n_links)");
    Outputs o{bases, offsets, count_sums, flags, link_offsets, link_to, r.n_bases};
    if (int rc = r.stage(&o)) return rc;
    if (int rc = r.spell(o)) return rc;
    if (int rc = r.emit(o)) return rc;
    return call.finish();
}

extern "C" int kt_ctr_unitig_tips(kt_ctr *table, uint32_t min_count, uint32_t max_count, uint32_t max_tip_nodes, uint8_t *marks,
                                  uint64_t max_unitigs, uint64_t *n_unitigs, uint64_t *tally, int mem) {
    return mark_call("kt_ctr_unitig_tips", table, min_count, max_count, TipRun{max_tip_nodes, 0u},
                     max_tip_nodes == 0 ? "max_tip_nodes must be >= 1" : nullptr, 0, KT_TIP_TALLY, marks, max_unitigs, n_unitigs, tally, mem);
}

extern "C" int kt_ctr_unitig_bubbles(kt_ctr *table, uint32_t min_count, uint32_t max_count, uint32_t max_bubble_nodes, uint8_t *marks,
                                     uint64_t max_unitigs, uint64_t *n_unitigs, uint64_t *tally, int mem) {
    return mark_call("kt_ctr_unitig_bubbles", table, min_count, max_count, TipRun{0u, 0u, max_bubble_nodes},
                     max_bubble_nodes == 0 ? "max_bubble_nodes must be >= 1" : nullptr, TIP_WORDS, KT_BUBBLE_TALLY, marks, max_unitigs,
                     n_unitigs, tally, mem);
}

extern "C" int kt_ctr_clip_tips(kt_ctr *table, uint32_t min_count, uint32_t max_count, uint32_t max_tip_nodes, uint32_t max_rounds,
                                uint32_t flags, uint64_t *stats) {
    if (!table) return kt::fail(KT_ERR_ARG, "kt_ctr_clip_tips: null");
    Call call(table->ctx, KT_MEM_DEVICE, "kt_ctr_clip_tips");
    if (max_tip_nodes == 0) return call.fail("max_tip_nodes must be >= 1");
    if (max_rounds < 1 || max_rounds > 1024) return call.fail("max_rounds must be in 1..1024");
    if (flags & ~KT_CLIP_ISOLATED) return call.fail("unknown flags");
    uint64_t s[KT_SIMPLIFY_STATS] = {};
    bool told = false;
    const int rc = erase_rounds(call, "kt_ctr_clip_tips", table, min_count, max_count, max_tip_nodes, 0u, max_rounds,
                                flags & KT_CLIP_ISOLATED, s, &told);
    if (stats && told) {
        for (int j = 0; j < 5; j++) stats[j] = s[j];
        stats[5] = s[8], stats[6] = s[9], stats[7] = 0;
    }
    return rc;
}

extern "C" int kt_ctr_simplify(kt_ctr *table, uint32_t min_count, uint32_t max_count, uint32_t max_tip_nodes, uint32_t max_bubble_nodes,
                               uint32_t max_rounds, uint32_t flags, uint64_t *stats) {
    if (!table) return kt::fail(KT_ERR_ARG, "kt_ctr_simplify: null");
    Call call(table->ctx, KT_MEM_DEVICE, "kt_ctr_simplify");
    if (max_tip_nodes == 0 && max_bubble_nodes == 0) return call.fail("max_tip_nodes and max_bubble_nodes are both 0");
    if (max_rounds < 1 || max_rounds > 1024) return call.fail("max_rounds must be in 1..1024");
    if (flags & ~KT_CLIP_ISOLATED) return call.fail("unknown flags");
    if ((flags & KT_CLIP_ISOLATED) && max_tip_nodes == 0) return call.fail("KT_CLIP_ISOLATED needs max_tip_nodes >= 1");
    uint64_t s[KT_SIMPLIFY_STATS] = {};
    bool told = false;
    const int rc = erase_rounds(call, "kt_ctr_simplify", table, min_count, max_count, max_tip_nodes, max_bubble_nodes, max_rounds,
                                flags & KT_CLIP_ISOLATED, s, &told);
    if (stats && told)
        for (int j = 0; j < KT_SIMPLIFY_STATS; j++) stats[j] = s[j];
    return rc;
}
