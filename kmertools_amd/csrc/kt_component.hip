// kt_component.hip - which unitigs hang together: the weakly connected components of the unitig graph, and the reads of a
// batch split by the component they land in (`kmertools unitigs --components`, `kmertools thread --components`; what khmer's
// partitioning and Bandage's component view answer on the CPU).  Two functions of arrays, no table:
//   kt_unitig_components       labels L[u] = u, then ROUNDS, each two launches - hook: one work item per owned link (u, v)
//                              reads lu = L[u], lv = L[v] and atomicMins the smaller into the other unitig's label and into
//                              L[the larger label] (FastSV's two hooks); shortcut: L[u] = L[L[u]] - until a round's hooks lower
//                              nothing.  A label only ever falls, stays a member of its unitig's component and stays <= the
//                              unitig, so whatever a stale read returns is a valid older label: it can cost a round, never the
//                              answer, and at the fixed point L is the component's smallest unitig.  The rounds are kernel
//                              boundaries: no wave waits for another wave's store, no loop on the device is unbounded.
//                              One scan (kt_scan.hpp) over the flags L[u] == u numbers the components; the aggregates are
//                              added once per group of lanes of a wave that share a component (grouped_add).
//   kt_thread_read_components  one lane per read for the reads of a few runs, the whole wave over the runs of every longer
//                              one (read_components_kernel): linear in the runs, and no long read sits on one lane.
#include "kt_internal.hpp"
#include "kt_launch.hpp"
#include "kt_scan.hpp"

namespace {

constexpr int BLOCK = 256;
constexpr uint32_t NONE = KT_NO_COMPONENT;
constexpr uint32_t LANE_RUNS = 8;   // a read of more runs than this is walked by its whole wave

// the links as kt_ctr_unitigs_linked leaves them; only [first, n_links) of link_to is owned by an end
struct Links {
    const uint64_t *offsets;  // 2 * nu + 1
    const uint32_t *to;
    uint64_t nu, first, n_links;
};

__device__ __forceinline__ uint32_t label(const uint32_t *L, uint64_t u) {
    // (past the CU's L1: a label another CU lowered earlier in this launch is seen sooner; an old one would do no harm)
    return __hip_atomic_load(L + u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// once: L[u] = u
__global__ __launch_bounds__(BLOCK) void label_init_kernel(uint32_t *__restrict__ L, uint64_t nu) {
    for (uint64_t u = (uint64_t)blockIdx.x * BLOCK + threadIdx.x; u < nu; u += (uint64_t)gridDim.x * BLOCK) L[u] = (uint32_t)u;
}

// once, one work item per owned link x: src[x] = the unitig whose end owns it (the one search: the last end e with
// offsets[e] <= x), NONE for a link to oneself and for a bad one, which is counted
__global__ __launch_bounds__(BLOCK) void link_source_kernel(Links g, uint32_t *__restrict__ src, unsigned long long *__restrict__ bad) {
    uint32_t n_bad = 0;
    for (uint64_t x = g.first + (uint64_t)blockIdx.x * BLOCK + threadIdx.x; x < g.n_links; x += (uint64_t)gridDim.x * BLOCK) {
        uint64_t lo = 0, hi = 2 * g.nu;
        while (hi - lo > 1) {
            const uint64_t mid = (lo + hi) >> 1;
            if (g.offsets[mid] <= x) lo = mid; else hi = mid;
        }
        const uint64_t u = lo >> 1, f = g.to[x];
        const bool is_bad = f >= 2 * g.nu;
        n_bad += is_bad;
        src[x] = is_bad || (f >> 1) == u ? NONE : (uint32_t)u;
    }
    n_bad = (uint32_t)ktd::wave_all_sum<uint64_t>(n_bad);
    if ((threadIdx.x & 63u) == 0 && n_bad) atomicAdd(bad, (unsigned long long)n_bad);
}

// a round's hooks, one work item per owned link
__global__ __launch_bounds__(BLOCK) void hook_kernel(Links g, const uint32_t *__restrict__ src, uint32_t *__restrict__ L,
                                                     uint32_t *__restrict__ changed) {
    bool lowered = false;
    for (uint64_t x = g.first + (uint64_t)blockIdx.x * BLOCK + threadIdx.x; x < g.n_links; x += (uint64_t)gridDim.x * BLOCK) {
        const uint32_t u = src[x];
        if (u == NONE) continue;
        const uint32_t v = g.to[x] >> 1;  // (< nu: link_source_kernel dropped the others)
        const uint32_t lu = label(L, u), lv = label(L, v);
        if (lu == lv) continue;
        const uint32_t lo = lu < lv ? lu : lv, hi = lu < lv ? lv : lu, far = lu < lv ? v : u;
        lowered |= atomicMin(L + far, lo) > lo;
        lowered |= atomicMin(L + hi, lo) > lo;
    }
    if (__ballot(lowered) && (threadIdx.x & 63u) == 0) atomicOr(changed, 1u);
}

// a round's shortcut: L[u] = L[L[u]]
__global__ __launch_bounds__(BLOCK) void shortcut_kernel(uint32_t *__restrict__ L, uint64_t nu) {
    for (uint64_t u = (uint64_t)blockIdx.x * BLOCK + threadIdx.x; u < nu; u += (uint64_t)gridDim.x * BLOCK) {
        const uint32_t p = label(L, u);  // (p <= u < nu)
        const uint32_t pp = label(L, p);
        if (pp < p) atomicMin(L + u, pp);
    }
}

// the scan's functor: sum a = the roots (L[u] == u) before a unitig; a root gets its number
struct RootScan {
    const uint32_t *L;
    uint32_t *component;  // null: the counting launches
    __device__ __forceinline__ uint32_t word(uint64_t i) const { return L[i] == (uint32_t)i; }
    __device__ __forceinline__ void add(uint32_t w, uint64_t &a, uint64_t &) const { a += w; }
    __device__ __forceinline__ void put(uint64_t i, uint64_t a, uint64_t) const {
        if (L[i] == (uint32_t)i) component[i] = (uint32_t)a;
    }
    __device__ __forceinline__ void total() const {}
};

// every other unitig takes its root's number (a root's entry is not written here)
__global__ __launch_bounds__(BLOCK) void number_kernel(const uint32_t *__restrict__ L, uint32_t *__restrict__ component, uint64_t nu) {
    for (uint64_t u = (uint64_t)blockIdx.x * BLOCK + threadIdx.x; u < nu; u += (uint64_t)gridDim.x * BLOCK) {
        const uint32_t r = L[u];
        if (r != (uint32_t)u) component[u] = component[r];
    }
}

// rows[c * STRIDE + q] += v[q], q < N, for every lane with c != NONE - once per group of lanes that share c: the first
// lane left gives its c, the lanes that match are summed, the first adds, until no lane is left.  Called by whole waves.
template <int N, int STRIDE>
__device__ __forceinline__ void grouped_add(unsigned long long *__restrict__ rows, uint32_t c, const uint64_t (&v)[N]) {
    uint64_t left = __ballot(c != NONE);
    const uint32_t lane = threadIdx.x & 63u;
    while (left) {  // (at most 64 turns: every turn takes its leader out)
        const int leader = __ffsll((unsigned long long)left) - 1;
        const uint32_t cl = (uint32_t)__shfl((int)c, leader, 64);
        const bool mine = c == cl;  // (cl != NONE)
        const uint64_t group = __ballot(mine);
        if (group == (1ull << leader)) {  // alone: nothing to sum
            if (mine)
#pragma unroll
                for (int q = 0; q < N; q++)
                    if (v[q]) atomicAdd(rows + (uint64_t)cl * STRIDE + q, (unsigned long long)v[q]);
        } else {
#pragma unroll
            for (int q = 0; q < N; q++) {
                const uint64_t s = ktd::wave_all_sum<uint64_t>(mine ? v[q] : 0);
                if (lane == (uint32_t)leader && s) atomicAdd(rows + (uint64_t)cl * STRIDE + q, (unsigned long long)s);
            }
        }
        left &= ~group;
    }
}

// one thread per unitig: its row of stats gets its unitig, nodes, count sum and good links; a root writes [4]
__global__ __launch_bounds__(BLOCK) void component_stats_kernel(Links g, const uint32_t *__restrict__ src, const uint64_t *__restrict__ uoff,
                                                                const uint64_t *__restrict__ csum, uint32_t k,
                                                                const uint32_t *__restrict__ L, const uint32_t *__restrict__ component,
                                                                unsigned long long *__restrict__ stats) {
    const uint64_t n_waves = (g.nu + 63) / 64;
    for (uint64_t w = ((uint64_t)blockIdx.x * BLOCK + threadIdx.x) >> 6; w < n_waves; w += ((uint64_t)gridDim.x * BLOCK) >> 6) {
        const uint64_t u = w * 64 + (threadIdx.x & 63u);  // (every lane of the wave stays for the sums)
        uint32_t c = NONE;
        uint64_t v[4] = {0, 0, 0, 0};
        if (u < g.nu) {
            c = component[u];
            v[0] = 1;
            if (uoff) {
                const uint64_t len = uoff[u + 1] - uoff[u];
                v[1] = len >= k - 1u ? len - (k - 1u) : 0;
            }
            if (csum) v[2] = csum[u];
            uint64_t x = g.offsets[2 * u], end = g.offsets[2 * u + 2];
            if (x < g.first) x = g.first;
            if (end > g.n_links) end = g.n_links;
            for (; x < end; x++) v[3] += src[x] != NONE || (g.to[x] >> 1) == u;  // (a bad link is not u's own)
            if (L[u] == (uint32_t)u) stats[(uint64_t)c * KT_COMPONENT_FIELDS + 4] = u;
        }
        grouped_add<4, KT_COMPONENT_FIELDS>(stats, c, v);
    }
}

// one thread per component: tally[1] += components of one unitig, [2] and [3] = the maxima; thread 0 writes [0] and [5]
__global__ __launch_bounds__(BLOCK) void component_tally_kernel(const unsigned long long *__restrict__ stats, uint64_t nc, uint64_t rounds,
                                                                unsigned long long *__restrict__ tally) {
    uint64_t single = 0, most_u = 0, most_n = 0;
    for (uint64_t c = (uint64_t)blockIdx.x * BLOCK + threadIdx.x; c < nc; c += (uint64_t)gridDim.x * BLOCK) {
        const uint64_t nu = stats[c * KT_COMPONENT_FIELDS], nn = stats[c * KT_COMPONENT_FIELDS + 1];
        single += nu == 1;
        most_u = nu > most_u ? nu : most_u;
        most_n = nn > most_n ? nn : most_n;
    }
    single = ktd::wave_all_sum<uint64_t>(single);
    most_u = ktd::wave_all_max(most_u), most_n = ktd::wave_all_max(most_n);
    if ((threadIdx.x & 63u) == 0) {
        if (single) atomicAdd(tally + 1, (unsigned long long)single);
        if (most_u) atomicMax(tally + 2, (unsigned long long)most_u);
        if (most_n) atomicMax(tally + 3, (unsigned long long)most_n);
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) tally[0] = nc, tally[5] = rounds;
}

// ---- kt_thread_read_components ------------------------------------------------------------------------------------------------
struct ReadArgs {
    const uint32_t *run_unitig, *run_len;
    const uint64_t *run_offsets;
    const uint32_t *component;
    uint64_t n_reads, n_runs, nu, nc;
};

// the component of run r, NONE for a bad run
__device__ __forceinline__ uint32_t run_component(const ReadArgs &a, uint64_t r) {
    const uint64_t u = a.run_unitig[r] >> 1;
    if (u >= a.nu) return NONE;
    const uint32_t c = a.component[u];
    return c < a.nc ? c : NONE;
}

// one thread per run: comp_hits[its component] += its length (grouped), tally[3] += the bad runs
__global__ __launch_bounds__(BLOCK) void run_hits_kernel(ReadArgs a, unsigned long long *__restrict__ comp_hits,
                                                         unsigned long long *__restrict__ tally) {
    const uint64_t n_waves = (a.n_runs + 63) / 64;
    uint32_t n_bad = 0;
    for (uint64_t w = ((uint64_t)blockIdx.x * BLOCK + threadIdx.x) >> 6; w < n_waves; w += ((uint64_t)gridDim.x * BLOCK) >> 6) {
        const uint64_t r = w * 64 + (threadIdx.x & 63u);
        uint32_t c = NONE;
        uint64_t v[1] = {0};
        if (r < a.n_runs) {
            c = run_component(a, r);
            n_bad += c == NONE;
            v[0] = a.run_len[r];
        }
        if (comp_hits) grouped_add<1, 1>(comp_hits, c, v);
    }
    n_bad = (uint32_t)ktd::wave_all_sum<uint64_t>(n_bad);
    if ((threadIdx.x & 63u) == 0 && n_bad) atomicAdd(tally + 3, (unsigned long long)n_bad);
}

// runs [lo, hi) of one read, walked by `lanes` lanes of which this is lane `me`: the component of the first good run this lane
// meets and its index, and whether a later one of its own differs
__device__ __forceinline__ void walk_runs(const ReadArgs &a, uint64_t lo, uint64_t hi, uint32_t me, uint32_t lanes, uint64_t *at,
                                          uint32_t *first, bool *mixed) {
    for (uint64_t r = lo + me; r < hi; r += lanes) {
        const uint32_t c = run_component(a, r);
        if (c == NONE) continue;
        if (*first == NONE) *first = c, *at = r;
        else *mixed |= c != *first;
    }
}

// one lane per read; a read of more than LANE_RUNS runs is then walked by the whole wave, one such read after the other
__global__ __launch_bounds__(BLOCK) void read_components_kernel(ReadArgs a, uint32_t *__restrict__ read_component,
                                                                uint8_t *__restrict__ read_mixed, unsigned long long *__restrict__ comp_reads,
                                                                unsigned long long *__restrict__ tally) {
    const uint64_t n_waves = (a.n_reads + 63) / 64;
    const uint32_t lane = threadIdx.x & 63u;
    uint32_t n_with = 0, n_without = 0, n_mixed = 0;
    for (uint64_t w = ((uint64_t)blockIdx.x * BLOCK + threadIdx.x) >> 6; w < n_waves; w += ((uint64_t)gridDim.x * BLOCK) >> 6) {
        const uint64_t i = w * 64 + lane;
        uint64_t lo = 0, hi = 0, at = 0;
        uint32_t c = NONE;
        bool mixed = false;
        if (i < a.n_reads) {
            lo = a.run_offsets[i], hi = a.run_offsets[i + 1];
            if (hi > a.n_runs) hi = a.n_runs;
            if (lo > hi) lo = hi;
        }
        const bool is_long = hi - lo > LANE_RUNS;
        if (!is_long) walk_runs(a, lo, hi, 0, 1, &at, &c, &mixed);
        for (uint64_t todo = __ballot(is_long); todo; todo &= todo - 1) {  // (at most 64 turns)
            const int owner = __ffsll((unsigned long long)todo) - 1;
            const uint64_t rlo = __shfl(lo, owner, 64), rhi = __shfl(hi, owner, 64);
            uint64_t my_at = ~0ull;
            uint32_t my_c = NONE;
            bool my_mixed = false;
            walk_runs(a, rlo, rhi, lane, 64, &my_at, &my_c, &my_mixed);
            const uint64_t first_at = ktd::wave_all_min(my_at);  // the read's first good run: the smallest index any lane met
            const uint64_t holder = __ballot(my_at == first_at && my_c != NONE);
            uint32_t c0 = NONE;
            bool any_mixed = false;
            if (holder) {
                c0 = (uint32_t)__shfl((int)my_c, __ffsll((unsigned long long)holder) - 1, 64);
                any_mixed = __ballot(my_c != NONE && (my_mixed || my_c != c0)) != 0;
            }
            if (lane == (uint32_t)owner) c = c0, mixed = any_mixed;
        }
        if (i < a.n_reads) {
            read_component[i] = c;
            if (read_mixed) read_mixed[i] = mixed;
            n_with += c != NONE;
            n_without += c == NONE;
            n_mixed += mixed;
        }
        if (comp_reads) {
            const uint64_t one[1] = {1};
            grouped_add<1, 1>(comp_reads, c, one);
        }
    }
    const uint32_t sums[3] = {n_with, n_without, n_mixed};
#pragma unroll
    for (int q = 0; q < 3; q++) {
        const uint64_t s = ktd::wave_all_sum<uint64_t>(sums[q]);
        if (lane == 0 && s) atomicAdd(tally + q, (unsigned long long)s);
    }
}

dim3 grid_of(const kt_ctx *ctx, uint64_t items) { return dim3(ktl::grid_for(ctx, (items + BLOCK - 1) / BLOCK, 8)); }

}  // namespace

using namespace ktl;

extern "C" int kt_unitig_components(kt_ctx *ctx, const uint64_t *link_offsets, const uint32_t *link_to, uint64_t n_unitigs,
                                    const uint64_t *unitig_offsets, const uint64_t *count_sums, int k, uint32_t *component,
                                    uint64_t *stats, uint64_t max_components, uint64_t *n_components, uint64_t *tally, int mem) {
    const char *name = "kt_unitig_components";
    if (!ctx) return kt::fail(KT_ERR_ARG, "kt_unitig_components: null ctx");
    Call call(ctx, mem, name);
    if (int rc = call.enter()) return rc;
    if (!n_components) return call.fail("null n_components");
    if (n_unitigs > 0x7FFFFFFFull) return call.fail("more than 2^31 - 1 unitigs (an end, 2 * unitig + sign, is a u32)");
    if (unitig_offsets && (k < 1 || k > 32)) return call.fail("k must be in 1..32");
    if (n_unitigs && (!link_offsets || !link_to || !component)) return call.fail("null buffer");
    if (max_components && !stats) return call.fail("null stats with max_components > 0");
    hipStream_t st = ctx->stream;
    const uint64_t nu = n_unitigs;
    if (nu == 0) {
        *n_components = 0;
        if (tally) {
            if (call.host())
                for (int q = 0; q < KT_COMPONENT_TALLY; q++) tally[q] = 0;
            else
                KT_HIP(hipMemsetAsync(tally, 0, KT_COMPONENT_TALLY * 8, st));
        }
        return KT_OK;
    }
    uint64_t ends[2] = {0, 0};  // link_offsets[0], link_offsets[2 nu]: the owned part of link_to
    if (call.host()) {
        ends[0] = link_offsets[0], ends[1] = link_offsets[2 * nu];
    } else {
        KT_HIP(hipMemcpyAsync(&ends[0], link_offsets, 8, hipMemcpyDeviceToHost, st));
        KT_HIP(hipMemcpyAsync(&ends[1], link_offsets + 2 * nu, 8, hipMemcpyDeviceToHost, st));
        KT_HIP(hipStreamSynchronize(st));
    }
    if (ends[0] > ends[1]) return call.fail("link_offsets descend");
    const uint64_t n_links = ends[1];

    // the inputs on the device
    const uint64_t *d_loff = nullptr, *d_uoff = unitig_offsets, *d_csum = count_sums;
    const uint32_t *d_lto = link_to;
    if (int rc = call.in(kt::OFFSETS, link_offsets, 2 * nu + 1, &d_loff)) return rc;
    if (n_links)
        if (int rc = call.in(kt::BASES, link_to, n_links, &d_lto)) return rc;
    if (call.host() && (unitig_offsets || count_sums)) {
        uint64_t *u = nullptr, *c = nullptr;
        if (int rc = carve(call, kt::AUX2, &u, unitig_offsets ? nu + 1 : 0, &c, count_sums ? nu : 0)) return rc;
        if (unitig_offsets) {
            if (int rc = call.up(u, unitig_offsets, nu + 1)) return rc;
            d_uoff = u;
        }
        if (count_sums) {
            if (int rc = call.up(c, count_sums, nu)) return rc;
            d_csum = c;
        }
    }
    // working arrays: the labels, every link's source unitig, the scan's tiles, the tally and the rounds' changed word
    const uint64_t n_tiles = scan2_tiles(nu);
    uint32_t *L = nullptr, *src = nullptr, *changed = nullptr;
    uint64_t *tiles = nullptr, *d_tally = nullptr;
    if (int rc = carve(call, kt::AUX0, &tiles, 2 * n_tiles, &d_tally, (uint64_t)8, &changed, (uint64_t)4, &L, nu, &src, n_links)) return rc;
    KT_HIP(hipMemsetAsync(d_tally, 0, 64, st));
    const Links g{d_loff, d_lto, nu, ends[0], n_links};
    const uint64_t owned = n_links - ends[0];
    if (int rc = launch(label_init_kernel, grid_of(ctx, nu), dim3(BLOCK), 0, st, L, nu)) return rc;
    if (owned)
        if (int rc = launch(link_source_kernel, grid_of(ctx, owned), dim3(BLOCK), 0, st, g, src, (unsigned long long *)&d_tally[4])) return rc;

    // the rounds: hook, shortcut, and the host reads whether a hook lowered a label
    uint64_t rounds = 0;
    for (bool more = owned != 0; more;) {
        if (rounds > nu)  // (a round that changes something lowers a label, and the labels can fall nu^2 times at the very most;
                          // FastSV needs O(log nu) rounds - this is a stop for a fault, not a bound that is ever met)
            return kt::fail(KT_ERR_HIP, std::string(name) + ": internal: the labelling did not settle in n_unitigs + 1 rounds");
        KT_HIP(hipMemsetAsync(changed, 0, 4, st));
        if (int rc = launch(hook_kernel, grid_of(ctx, owned), dim3(BLOCK), 0, st, g, (const uint32_t *)src, L, changed)) return rc;
        if (int rc = launch(shortcut_kernel, grid_of(ctx, nu), dim3(BLOCK), 0, st, L, nu)) return rc;
        uint32_t word = 0;
        KT_HIP(hipMemcpyAsync(&word, changed, 4, hipMemcpyDeviceToHost, st));
        KT_HIP(hipStreamSynchronize(st));
        rounds++;
        more = word != 0;
    }

    // the numbering: the roots counted, then - there being room - numbered, and every unitig given its root's number
    RootScan scan{L, nullptr};
    if (int rc = scan2_sums(st, scan, nu, tiles, &d_tally[6], &d_tally[7])) return rc;
    uint64_t nc = 0;
    KT_HIP(hipMemcpyAsync(&nc, &d_tally[6], 8, hipMemcpyDeviceToHost, st));
    KT_HIP(hipStreamSynchronize(st));
    *n_components = nc;
    if (max_components && max_components < nc) return call.fail("max_components is smaller than the number of components (*n_components is set)");

    uint32_t *d_comp = nullptr;
    if (int rc = call.out(kt::AUX1, component, nu, &d_comp)) return rc;
    scan.component = d_comp;
    if (int rc = scan2_apply(st, scan, nu, tiles)) return rc;
    if (int rc = launch(number_kernel, grid_of(ctx, nu), dim3(BLOCK), 0, st, (const uint32_t *)L, d_comp, nu)) return rc;

    // the aggregates: in the caller's rows, or - a host call, or a tally with no rows to read the maxima from - in OUT
    const bool rows = max_components != 0;
    if (rows || tally) {
        uint64_t *d_stats = stats;
        if (call.host() || !rows)
            if (int rc = call.scratch(kt::OUT, nc * KT_COMPONENT_FIELDS * 8, &d_stats)) return rc;
        KT_HIP(hipMemsetAsync(d_stats, 0, nc * KT_COMPONENT_FIELDS * 8, st));
        if (int rc = launch(component_stats_kernel, grid_of(ctx, nu), dim3(BLOCK), 0, st, g, (const uint32_t *)src, d_uoff, d_csum,
                            (uint32_t)k, (const uint32_t *)L, (const uint32_t *)d_comp, (unsigned long long *)d_stats))
            return rc;
        if (tally) {
            if (int rc = launch(component_tally_kernel, grid_of(ctx, nc), dim3(BLOCK), 0, st, (const unsigned long long *)d_stats, nc,
                                rounds, (unsigned long long *)d_tally))
                return rc;
            if (!call.host()) KT_HIP(hipMemcpyAsync(tally, d_tally, KT_COMPONENT_TALLY * 8, hipMemcpyDeviceToDevice, st));
        }
        if (rows) call.back(stats, (const uint64_t *)d_stats, nc * KT_COMPONENT_FIELDS);
    }
    call.back(tally, (const uint64_t *)d_tally, (uint64_t)KT_COMPONENT_TALLY);
    return call.finish();
}

extern "C" int kt_thread_read_components(kt_ctx *ctx, const uint32_t *run_unitig, const uint32_t *run_len, const uint64_t *run_offsets,
                                         uint64_t n_reads, const uint32_t *component, uint64_t n_unitigs, uint64_t n_components,
                                         uint32_t *read_component, uint8_t *read_mixed, uint64_t *comp_reads, uint64_t *comp_hits,
                                         uint64_t *tally, int mem) {
    if (!ctx) return kt::fail(KT_ERR_ARG, "kt_thread_read_components: null ctx");
    Call call(ctx, mem, "kt_thread_read_components");
    if (int rc = call.enter()) return rc;
    if (n_unitigs > 0x7FFFFFFFull) return call.fail("more than 2^31 - 1 unitigs (2 * unitig + orientation is a u32)");
    if (n_components > n_unitigs) return call.fail("more components than unitigs");
    if (n_reads && (!run_offsets || !read_component)) return call.fail("null buffer");
    if (n_unitigs && !component) return call.fail("null component");
    hipStream_t st = ctx->stream;
    if (n_reads == 0) {  // no read: nothing to add
        if (tally) {
            if (call.host())
                for (int q = 0; q < KT_READ_COMPONENT_TALLY; q++) tally[q] = 0;
            else
                KT_HIP(hipMemsetAsync(tally, 0, KT_READ_COMPONENT_TALLY * 8, st));
        }
        return KT_OK;
    }
    uint64_t n_runs = 0;
    if (call.host()) {
        n_runs = run_offsets[n_reads];
    } else {
        KT_HIP(hipMemcpyAsync(&n_runs, run_offsets + n_reads, 8, hipMemcpyDeviceToHost, st));
        KT_HIP(hipStreamSynchronize(st));
    }
    if (n_runs && (!run_unitig || !run_len)) return call.fail("null run array");

    ReadArgs a{run_unitig, run_len, nullptr, component, n_reads, n_runs, n_unitigs, n_components};
    if (n_runs) {
        if (int rc = call.in(kt::BASES, run_unitig, n_runs, &a.run_unitig)) return rc;
        if (int rc = call.in(kt::AUX1, run_len, n_runs, &a.run_len)) return rc;
    }
    if (int rc = call.in(kt::OFFSETS, run_offsets, n_reads + 1, &a.run_offsets)) return rc;
    if (n_unitigs)
        if (int rc = call.in(kt::AUX2, component, n_unitigs, &a.component)) return rc;
    uint64_t *d_tally = nullptr;
    if (int rc = call.scratch(kt::AUX0, 64, &d_tally)) return rc;
    KT_HIP(hipMemsetAsync(d_tally, 0, 64, st));
    // the outputs: the caller's arrays, or (host) their images in OUT; the sums are added to, so the caller's go up first
    uint32_t *d_rc = read_component;
    uint8_t *d_mixed = read_mixed;
    uint64_t *d_reads = comp_reads, *d_hits = comp_hits;
    if (call.host()) {
        const uint64_t n_cr = comp_reads ? n_components : 0, n_ch = comp_hits ? n_components : 0;
        if (int rc = carve(call, kt::OUT, &d_reads, n_cr, &d_hits, n_ch, &d_rc, n_reads, &d_mixed, read_mixed ? n_reads : 0)) return rc;
        if (!n_cr) d_reads = nullptr;
        if (!n_ch) d_hits = nullptr;
        if (!read_mixed) d_mixed = nullptr;
        if (d_reads)
            if (int rc = call.up(d_reads, (const uint64_t *)comp_reads, n_components)) return rc;
        if (d_hits)
            if (int rc = call.up(d_hits, (const uint64_t *)comp_hits, n_components)) return rc;
    } else {
        if (!n_components) d_reads = d_hits = nullptr;
    }
    if (n_runs && (d_hits || tally))
        if (int rc = launch(run_hits_kernel, grid_of(ctx, n_runs), dim3(BLOCK), 0, st, a, (unsigned long long *)d_hits,
                            (unsigned long long *)d_tally))
            return rc;
    if (int rc = launch(read_components_kernel, grid_of(ctx, n_reads), dim3(BLOCK), 0, st, a, d_rc, d_mixed, (unsigned long long *)d_reads,
                        (unsigned long long *)d_tally))
        return rc;
    if (tally && !call.host()) KT_HIP(hipMemcpyAsync(tally, d_tally, KT_READ_COMPONENT_TALLY * 8, hipMemcpyDeviceToDevice, st));
    call.back(read_component, (const uint32_t *)d_rc, n_reads);
    call.back(read_mixed, (const uint8_t *)d_mixed, d_mixed ? n_reads : 0);
    call.back(comp_reads, (const uint64_t *)d_reads, d_reads ? n_components : 0);
    call.back(comp_hits, (const uint64_t *)d_hits, d_hits ? n_components : 0);
    call.back(tally, (const uint64_t *)d_tally, (uint64_t)KT_READ_COMPONENT_TALLY);
    return call.finish();
}
