// kt_probe.hpp - the probe pipeline over a thread's window starts of a staged segment, shared by the kernels that look a
// read's k-mers up in the table: kt_cov.hip (cov, solidity, profile) and kt_thread.hip (oriented positions).
#pragma once
#include "kt_segment.hpp"
#include "kt_table.hpp"

#ifndef KT_COV_GROUP
#define KT_COV_GROUP 8
#endif

namespace ktprobe {

constexpr uint32_t GROUP = KT_COV_GROUP;  // table probes in flight per thread

// The probe pipeline over a thread's 32 window starts of a staged segment, GROUP at a time (rolled, so the k-mers never sit
// in registers all at once): the group's canonical k-mers, the home-slot loads of those that are k-mers (w.okm) of the
// table's hash partition in flight together, then sink(jj, wr, cnt): bit u of `wr` = window start jj + u was looked up,
// cnt[u] = its occurrences (0: absent).
// STRAND: the walk's own comparison of the two strands comes along - sink(jj, wr, cnt, rc): bit u of `rc` = the read shows
// the reverse complement of the canonical k-mer at window start jj + u (f > r; clear for a palindrome).
template <bool STRAND = false, class Sink>
__device__ __forceinline__ void probe_windows(const kttab::Probed &t, ktseg::Window &w, Sink &&sink) {
#pragma unroll 1
    for (uint32_t jj = 0; jj < ktseg::PER_THREAD; jj += GROUP) {
        uint64_t key[GROUP];
        uint32_t cnt[GROUP] = {};
        uint32_t wr = (w.okm >> jj) & ((1u << GROUP) - 1u);
#pragma unroll
        for (uint32_t u = 0; u < GROUP; u++) {
            key[u] = w.f < w.r ? w.f : w.r;
            // (the strands ride in the bits of `wr` above the group's: one register across the loads, not two)
            if constexpr (STRAND) wr |= (uint32_t)(w.f > w.r) << (GROUP + u);
            w.step();
            if (!t.mine(key[u])) wr &= ~(1u << u);
        }
        t.counts(key, wr, [&](uint32_t u, uint32_t n) { cnt[u] = n; });
        if constexpr (STRAND) sink(jj, wr & ((1u << GROUP) - 1u), cnt, wr >> GROUP);
        else sink(jj, wr, cnt);
    }
}

}  // namespace ktprobe
