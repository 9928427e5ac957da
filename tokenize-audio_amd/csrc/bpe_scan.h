// The scan operators of the codec-BPE decoders, shared by bpe_decode.hip (whole sequences, grid-wide scans) and
// bpe_decode_stream.hip (chunk by chunk, one workgroup per item): `+`, the composition of filter state maps, the
// workgroup's exclusive scan over either, and the binary search that takes a position back to its owner.
//
// The filter is a scan: character i is the map f_i(e) = e == cb_i ? (e + 1) % K : e on [0, K), the state before
// character i is f_{i-1} o ... o f_0, and the first character of a sequence is the constant map to (cb_0 + 1) % K,
// which absorbs everything to its left.  A map is a u64 of K <= 16 nibbles.  The operator does not commute:
// `combine(earlier, later)` keeps that order in the shuffle steps, across the waves and in every carry.
#pragma once
#include <hip/hip_runtime.h>

namespace mimi {
namespace bpe {

typedef unsigned long long u64;

constexpr int kScanThreads = 256;  // the workgroup of block_exclusive
constexpr int kMaxK = 16;          // nibbles of a u64

// ---- the two operators ---------------------------------------------------------------------------------------
struct AddOp {
    __device__ __forceinline__ u64 identity() const { return 0; }
    __device__ __forceinline__ u64 combine(u64 earlier, u64 later) const { return earlier + later; }
};

constexpr u64 kIdentityMap = 0xfedcba9876543210ull;

struct MapOp {
    int K;
    __device__ __forceinline__ u64 identity() const { return kIdentityMap; }
    // (later o earlier)(e) = later(earlier(e)); entries at and above K stay the identity's
    __device__ __forceinline__ u64 combine(u64 earlier, u64 later) const {
        u64 r = kIdentityMap;
        for (int e = 0; e < K; ++e) {
            const unsigned mid = (unsigned)(earlier >> (4 * e)) & 15u;
            const u64 to = (later >> (4 * mid)) & 15ull;
            r = (r & ~(15ull << (4 * e))) | (to << (4 * e));
        }
        return r;
    }
};

// the map of one character of codebook cb: the first of a sequence sends every state to (cb + 1) % K
__device__ __forceinline__ u64 char_map(unsigned cb, bool first, int K) {
    const u64 next = (u64)((cb + 1) % (unsigned)K);
    if (first) return next * 0x1111111111111111ull;
    return (kIdentityMap & ~(15ull << (4 * cb))) | (next << (4 * cb));
}

// exclusive scan of one value per thread over the workgroup, in thread order; total = all of them.  wtot: 4 words
template <typename Op>
__device__ __forceinline__ u64 block_exclusive(const Op& op, u64 v, u64* wtot, u64& total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    u64 x = v;  // inclusive over the wave
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const u64 y = __shfl_up(x, o);
        if (lane >= o) x = op.combine(y, x);
    }
    const u64 before = __shfl_up(x, 1);
    if (lane == 63) wtot[wave] = x;
    __syncthreads();
    u64 base = op.identity(), all = op.identity();
#pragma unroll
    for (int i = 0; i < kScanThreads / 64; ++i) {
        const u64 s = wtot[i];
        if (i < wave) base = op.combine(base, s);
        all = op.combine(all, s);
    }
    __syncthreads();  // wtot is reused by the next call
    total = all;
    return lane == 0 ? base : op.combine(base, before);
}

// the last s in [0, n) with pos[s] <= p, for pos[0] <= p < pos[n] (empty entries are skipped)
__device__ __forceinline__ int find_in(const int* pos, int n, int p) {
    int lo = 0, hi = n;  // pos[lo] <= p < pos[hi]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (pos[mid] <= p) lo = mid;
        else hi = mid;
    }
    return lo;
}

}  // namespace bpe
}  // namespace mimi
