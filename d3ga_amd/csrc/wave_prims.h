// wave_prims.h -- the wavefront and workgroup building blocks the .hip files share: the 64-lane butterfly sum, its hand-off to
// LDS, and the two-level exclusive scan of the recorder's rasterizers.  Device code only.  Nothing here but additions, integer
// operations and shuffles: no translation unit's -ffp-contract or division flags can change what these compute.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

namespace d3ga {

// The sum over the wavefront's 64 lanes, in every lane: a butterfly with partner lane ^ 32, 16, 8, 4, 2, 1.  The host mirrors
// (objective_math.h, eval_math.h, tests/loss_ref.py) add in this order.
template <typename T>
__device__ __forceinline__ T wave_sum(T v) {
    static_assert(std::is_floating_point<T>::value, "float or double");
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

// wave_sum, then lane 0 of every wavefront leaves the total in s_part[wavefront].  No barrier: a kernel that hands several
// sums over stores them all and waits once.
template <typename T>
__device__ __forceinline__ void wave_sum_to_lds(T v, T *s_part) {
    v = wave_sum(v);
    if ((threadIdx.x & 63) == 0) s_part[threadIdx.x >> 6] = v;
}
// ... and the barrier after which any lane may read s_part.  How the per-wavefront totals are then combined is the caller's
// business: the order of those additions is part of each kernel's pinned rounding.
template <typename T>
__device__ __forceinline__ void wave_sums_to_lds(T v, T *s_part) {
    wave_sum_to_lds(v, s_part);
    __syncthreads();
}

// The value lane + 1 holds, by a lane shift; lane 63 has no successor and gets `last`.  Every lane of the wavefront must call.
__device__ __forceinline__ int32_t wave_next_lane(int32_t v, int32_t last) {
    const int32_t n = __shfl_down(v, 1);
    return (threadIdx.x & 63) == 63 ? last : n;
}

__device__ __forceinline__ uint32_t wave_incl_scan_u32(uint32_t v, int lane) {
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t o = __shfl_up(v, off);
        if (lane >= off) v += o;
    }
    return v;
}

__device__ __forceinline__ uint64_t shfl_up_u64(uint64_t v, int off) {
    const uint32_t lo = __shfl_up((uint32_t)v, off), hi = __shfl_up((uint32_t)(v >> 32), off);
    return ((uint64_t)hi << 32) | lo;
}

// The exclusive prefix of `count` over a workgroup of NW wavefronts (lane order), and the workgroup's total in every lane.
// s_wave: NW words of LDS.  Every lane of the workgroup must call this (one barrier inside).
template <int NW>
__device__ __forceinline__ uint32_t block_excl_scan_u32(uint32_t count, uint32_t *s_wave, uint32_t *total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t incl = wave_incl_scan_u32(count, lane);
    if (lane == 63) s_wave[wave] = incl;
    __syncthreads();
    uint32_t before = 0, sum = 0;
#pragma unroll
    for (int w = 0; w < NW; ++w) {
        if (w < wave) before += s_wave[w];
        sum += s_wave[w];
    }
    *total = sum;
    return before + incl - count;
}

// The same over 64-bit values, inclusive: the prefix of `v` up to and including this lane, and the workgroup's total in every
// lane.  s_wave: NW 64-bit words of LDS.  Every lane of the workgroup must call this (one barrier inside).
template <int NW>
__device__ __forceinline__ uint64_t block_incl_scan_u64(uint64_t v, uint64_t *s_wave, uint64_t *total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint64_t incl = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const uint64_t o = shfl_up_u64(incl, off);
        if (lane >= off) incl += o;
    }
    if (lane == 63) s_wave[wave] = incl;
    __syncthreads();
    uint64_t before = 0, sum = 0;
#pragma unroll
    for (int w = 0; w < NW; ++w) {
        if (w < wave) before += s_wave[w];
        sum += s_wave[w];
    }
    *total = sum;
    return before + incl;
}

// The second level: ONE workgroup of BLOCK lanes turns the nblk workgroup totals (uint32_t or uint64_t) into their exclusive
// 64-bit prefix, BLOCK at a time with the running total carried along; block_start[nblk] = the total of all.  s_wave: BLOCK / 64
// words of LDS.
template <int BLOCK, typename T>
__device__ __forceinline__ void scan_block_totals(int64_t nblk, const T *__restrict__ block_total,
                                                  uint64_t *__restrict__ block_start, uint64_t *s_wave) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    uint64_t carry = 0;
    for (int64_t base = 0; base < nblk; base += BLOCK) {
        const int64_t i = base + tid;
        const uint64_t v = i < nblk ? (uint64_t)block_total[i] : 0;
        uint64_t incl = v;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const uint64_t o = shfl_up_u64(incl, off);
            if (lane >= off) incl += o;
        }
        if (lane == 63) s_wave[wave] = incl;
        __syncthreads();
        uint64_t before = 0, total = 0;
        for (int w = 0; w < BLOCK / 64; ++w) {
            if (w < wave) before += s_wave[w];
            total += s_wave[w];
        }
        if (i < nblk) block_start[i] = carry + before + incl - v;
        carry += total;
        __syncthreads();
    }
    if (tid == 0) block_start[nblk] = carry;
}

}  // namespace d3ga
