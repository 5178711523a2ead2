// kt_prefilter.hpp - the two-array pre-filter (kt_prefilter.hip) as its kernels and the filtered add of kt_ctr.hip take it:
// where a canonical k-mer's bits lie and whether they are set.
//
//   h = mix64(kmer ^ seed)     once word  = h >> (64 - a),  pattern = OR over j = 0..3 of 1 << ((h >> 6 j) & 63)
//   g = mix64(h)               twice word = g >> (64 - b),  pattern from g the same way
// The word comes from the top bits of the hash and the pattern from its low 24, and a, b <= 34, so the two do not share
// bits.  All of a k-mer's bits lie in one 64-bit word of each array: one atomicOr sets them, and what it returns says
// whether they were all set before.
#pragma once
#include "kt_device.hpp"

namespace ktpf {

constexpr uint32_t MIN_LOG2 = 10, MAX_LOG2 = 34;  // KT_PREFILTER_MIN_LOG2 / KT_PREFILTER_MAX_LOG2

__host__ __device__ __forceinline__ uint64_t pattern_of(uint64_t h) {
    return (1ull << (h & 63u)) | (1ull << ((h >> 6) & 63u)) | (1ull << ((h >> 12) & 63u)) | (1ull << ((h >> 18) & 63u));
}

struct View {
    uint64_t *once, *twice;  // 2^a and 2^b words
    uint64_t seed;
    uint32_t a, b;
    __host__ __device__ __forceinline__ uint64_t once_hash(uint64_t kmer) const { return ktd::mix64(kmer ^ seed); }
    __host__ __device__ __forceinline__ uint64_t twice_hash(uint64_t h) const { return ktd::mix64(h); }
    __host__ __device__ __forceinline__ uint64_t *once_word(uint64_t h) const { return once + (h >> (64u - a)); }
    __host__ __device__ __forceinline__ uint64_t *twice_word(uint64_t g) const { return twice + (g >> (64u - b)); }
#ifdef __HIPCC__
    // the k-mer's pattern is covered in `twice`: a plain load (the kernel that asks runs after the ones that set the bits)
    __device__ __forceinline__ bool seen_twice(uint64_t kmer) const {
        const uint64_t g = twice_hash(once_hash(kmer)), p = pattern_of(g);
        return (*twice_word(g) & p) == p;
    }
#endif
};

// what kt_ctr.hip's count_reads_kernel asks before it adds a k-mer
struct KeepAll {
    __device__ __forceinline__ bool operator()(uint64_t) const { return true; }
};
struct KeepSeenTwice {
    View f;
    __device__ __forceinline__ bool operator()(uint64_t kmer) const { return f.seen_twice(kmer); }
};

}  // namespace ktpf
