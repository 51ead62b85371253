// Wave (64 lanes) and workgroup building blocks of the one-workgroup-per-image integer kernels (instances.hip, rle.hip, panoptic.hip): scans,
// flag ranks, wave segments, the stable counting sort and the score-order sort.  Device-only, no state.  The integer wave reductions are in common.h beside the
// float ones.  `lane` = threadIdx.x & 63, `wave` = threadIdx.x >> 6 throughout.
#pragma once
#include "common.h"

// a word that atomics of other waves of this launch have written: read at the L2 (agent scope), a plain load may hit a stale L1 line
template <typename T>
__device__ __forceinline__ T mu_ld_agent(const T* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ unsigned long long lanes_below(int lane) { return (1ull << lane) - 1ull; }

// inclusive scan over the lanes (int or unsigned); lane 63 holds the wave's sum
template <typename T>
__device__ __forceinline__ T wave_scan_incl(T v, int lane) {
    static_assert(sizeof(T) == 4, "one 32-bit shuffle per step");
    for (int o = 1; o < 64; o <<= 1) {
        const T u = (T)__shfl_up((int)v, o);
        if (lane >= o) v += u;
    }
    return v;
}

// one 64-entry turn of a longer scan: returns carry + (sum of v over the lanes below); carry advances by the wave's sum
template <typename T>
__device__ __forceinline__ T wave_scan_excl(T v, int lane, T& carry) {
    const T incl = wave_scan_incl(v, lane);
    const T excl = carry + incl - v;
    carry += (T)__shfl((int)incl, 63);
    return excl;
}

// one wave: dst[i] = sum of src[0..i) for i < n (src == dst is fine); returns the total in every lane
__device__ __forceinline__ int wave_scan_excl_array(const int* src, int* dst, int n, int lane) {
    int carry = 0;
    for (int base = 0; base < n; base += 64) {
        const int i = base + lane;
        const int e = wave_scan_excl(i < n ? src[i] : 0, lane, carry);
        if (i < n) dst[i] = e;
    }
    return carry;
}

// the contiguous range [lo, hi) of [0, n) that a wave owns: a multiple of 64 long (chunks never straddle two waves), empty past n
__device__ __forceinline__ void wave_segment(int n, int n_waves, int wave, int& lo, int& hi) {
    const int seg = ((n + n_waves * 64 - 1) / (n_waves * 64)) * 64;
    lo = min(n, wave * seg);
    hi = min(n, lo + seg);
}

// mine = what this wave counted in its segment (the same in every lane).  Returns the sum over the waves before it, `total` the sum
// over all.  wave_total = n_waves words of LDS.  Holds a barrier: every thread of the workgroup calls it.
__device__ __forceinline__ unsigned block_exclusive_base(unsigned mine, unsigned* wave_total, int lane, int wave, int n_waves,
                                                         unsigned& total) {
    if (lane == 0) wave_total[wave] = mine;
    __syncthreads();
    unsigned running = 0;
    total = 0;
    for (int v = 0; v < n_waves; ++v) {
        const unsigned t = wave_total[v];
        if (v < wave) running += t;
        total += t;
    }
    return running;
}

// rank of this lane's flag among the set flags: running + (set flags in the lanes below); running advances by the wave's set flags
__device__ __forceinline__ unsigned wave_flag_rank(bool flag, int lane, unsigned& running) {
    const unsigned long long mask = __ballot(flag);
    const unsigned rank = running + __popcll(mask & lanes_below(lane));
    running += __popcll(mask);
    return rank;
}

// sort key of row k (0-based) with score s: ascending keys = descending score, then ascending id (= k + 1, the low word)
__device__ __forceinline__ unsigned long long score_order_key(float s, int k) {
    unsigned u = __float_as_uint(s);
    u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);           // ascending-sortable float bits
    return ((unsigned long long)(~u) << 32) | (unsigned)(k + 1);
}

// bitonic sort of key[0..S), ascending, S a power of two (LDS or the workgroup's own global memory).  Holds barriers: every thread of
// the workgroup calls it; the keys written before the call need no barrier of their own, the sorted ones are visible on return.
__device__ __forceinline__ void block_sort_u64(unsigned long long* key, int S, int tid, int n_threads) {
    for (int size = 2; size <= S; size <<= 1) {
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            __syncthreads();
            for (int t = tid; t < (S >> 1); t += n_threads) {
                const int lo = ((t & ~(stride - 1)) << 1) | (t & (stride - 1)), hi = lo + stride;
                const bool up = (lo & size) == 0;
                const unsigned long long a = key[lo], c = key[hi];
                if ((a > c) == up) {
                    key[lo] = c;
                    key[hi] = a;
                }
            }
        }
    }
    __syncthreads();
}

// One 64-lane chunk of a stable counting sort: `has` = the lane holds an element, `key` its bucket, counter[] the wave's OWN counters
// (the wave owns a wave_segment of the input, so no atomics and a fixed order).  The distinct keys of the chunk are peeled off with
// ballots, one round per key.  Three steps: (1) PLACE = false over the segment counts; (2) the caller turns the counters into start
// positions (prefix over the waves, then over the keys); (3) PLACE = true, the same walk, returns the element's slot = counter[key] +
// (holders of the key in the lanes below) and advances the counter.  Returns 0 where !has.
template <bool PLACE>
__device__ __forceinline__ int wave_sort_chunk(int key, bool has, int lane, int* counter) {
    int slot = 0;
    unsigned long long rem = __ballot(has);
    while (rem) {
        const int key0 = __shfl(key, __ffsll((long long)rem) - 1);
        const unsigned long long m = __ballot(has && key == key0);
        const int at = counter[key0];
        if (PLACE && has && key == key0) slot = at + __popcll(m & lanes_below(lane));
        if (lane == 0) counter[key0] = at + __popcll(m);
        rem &= ~m;
    }
    return slot;
}
