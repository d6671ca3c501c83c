// The stores of the kernels in which a lane owns 16 consecutive positions of one (B, P) row (k_mlm_bp, k_kmer_bp): 16-byte non-temporal
// stores, and for 2- to 8-byte elements through LDS so that a wave writes whole 1-KiB runs.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "bsq_device.h"

namespace bsq_dev {

// 16 elements of T to dst (n of them when n < 16); vec: dst + 16 elements lies in the matrix and the group is whole
template <typename T>
__device__ __forceinline__ void store_piece(T *dst, const T (&v)[16], uint32_t n) {
    if (n == 16) {
#pragma unroll
        for (int q = 0; q < static_cast<int>(sizeof(T)); ++q) {
            uint4 u;
            __builtin_memcpy(&u, reinterpret_cast<const char *>(v) + 16 * q, 16);
            store16_unaligned<true>(reinterpret_cast<char *>(dst) + 16 * q, u);
        }
    } else {
#pragma unroll
        for (uint32_t k = 0; k < 16; ++k)
            if (k < n) dst[k] = v[k];
    }
}

// The 16 * sizeof(T) bytes of every thread of the block to out, through LDS when STAGED (block-uniform: padlen % 16 == 0 and every thread
// of the block owns a piece, so the block's pieces are the contiguous elements [16 * first, 16 * (first + kThreads))): store q of the block
// then writes 16-byte vector q * kThreads + thread -- whole 1-KiB runs per wave instead of 64 lanes each hitting its own 16 * sizeof(T)-byte
// span (cfg5 shape, int8 inputs + int64 labels: 2.07 ms without the staging, 0.25 ms with it: profiles/r07/mlm_lab.txt).  Slots are
// rotated by the thread index to spread the LDS banks.  s_out: kThreads * sizeof(T) uint4 of LDS (unused for one-byte elements).
template <typename T>
__device__ __forceinline__ void write_out(T *out, int64_t gid, int64_t e0, const T (&v)[16], uint32_t n, bool valid, bool staged, uint4 *s_out) {
    if (sizeof(T) == 1 || !staged) {
        if (valid) store_piece(out + e0, v, n);
        return;
    }
    constexpr uint32_t SZ = sizeof(T);
    const uint32_t t = threadIdx.x;
    __syncthreads();  // (the previous output's reads of s_out are done)
#pragma unroll
    for (uint32_t q = 0; q < SZ; ++q) {
        uint4 u;
        __builtin_memcpy(&u, reinterpret_cast<const char *>(v) + 16 * q, 16);
        s_out[t * SZ + ((q + t) & (SZ - 1))] = u;
    }
    __syncthreads();
    char *base = reinterpret_cast<char *>(out + (gid - t) * 16);
#pragma unroll
    for (uint32_t q = 0; q < SZ; ++q) {
        const uint32_t idx = q * kThreads + t, owner = idx / SZ, part = idx & (SZ - 1);
        store16_unaligned<true>(base + static_cast<size_t>(idx) * 16, s_out[owner * SZ + ((part + owner) & (SZ - 1))]);
    }
}

}  // namespace bsq_dev
