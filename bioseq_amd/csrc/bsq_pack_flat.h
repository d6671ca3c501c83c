// What the output-driven kernels of the packing family share (k_pack_flat of bsq_pack.hip, k_pack_mlm_flat of bsq_pack_mlm.hip): the
// register-table lookup of a folded alphabet, the wave's search in `starts`, and the host's test for a folded alphabet.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "bsq.h"
#include "bsq_pack_dev.h"

namespace bsq_packf {

// byte i of the result = tab[byte i of cw & 31] (the 32-entry register table of k_tokens_bp8)
__device__ __forceinline__ uint32_t lookup4_perm(uint32_t cw, const uint32_t (&T)[8]) {
    const uint32_t sel = cw & 0x07070707u;
    const uint32_t r0 = __builtin_amdgcn_perm(T[1], T[0], sel);
    const uint32_t r1 = __builtin_amdgcn_perm(T[3], T[2], sel);
    const uint32_t r2 = __builtin_amdgcn_perm(T[5], T[4], sel);
    const uint32_t r3 = __builtin_amdgcn_perm(T[7], T[6], sel);
    const uint32_t s3 = ((cw >> 1) & 0x04040404u) | 0x03020100u;
    const uint32_t lo = __builtin_amdgcn_perm(r1, r0, s3);
    const uint32_t hi = __builtin_amdgcn_perm(r3, r2, s3);
    const uint32_t s4 = ((cw >> 2) & 0x04040404u) | 0x03020100u;
    return __builtin_amdgcn_perm(hi, lo, s4);
}
// 0xFF in every byte of cw that is not a letter position (0x40 .. 0x7F): those bytes are unmapped
__device__ __forceinline__ uint32_t nonletter_mask(uint32_t cw) {
    const uint32_t x = (cw ^ 0x40404040u) & 0xC0C0C0C0u;
    const uint32_t f = ((x >> 6) | (x >> 7)) & 0x01010101u;
    return (f << 8) - f;
}

// bsq_packd::find(starts, B, -1, q) for a wave-uniform q, by the 64 lanes together: every round the lanes probe 64 evenly spaced entries
// of the open interval and a ballot keeps the piece that holds the answer -- three dependent loads at 262 144 sequences where the
// gallop from -1 takes some thirty.  All 64 lanes must be active.
__device__ __forceinline__ int64_t find_wave(const int64_t *starts, int64_t B, uint64_t q) {
    const int64_t lane = threadIdx.x & 63;
    int64_t lo = -1, hi = B;  // start(lo) <= q (or lo == -1), start(hi) > q (or hi == B)
    while (hi - lo > 1) {
        const int64_t step = (hi - lo + 62) >> 6;  // ceil((hi - lo - 1) / 64) >= 1
        const int64_t m = lo + (lane + 1) * step;
        const bool le = m < hi && bsq_packd::ustart(starts, m) <= q;
        const int64_t c = __popcll(__builtin_amdgcn_ballot_w64(le));  // (starts never decrease: the lanes below c)
        const int64_t top = lo + (c + 1) * step;
        hi = top < hi ? top : hi;
        lo += c * step;
    }
    return lo;
}

// The folded table of an alphabet whose mapped bytes are letters with both cases alike (the rule of k_tokens_bp8's register table).
inline bool fold_table(const bsq_desc *d, uint32_t (&tab)[8]) {
    for (int i = 0; i < 8; ++i) tab[i] = 0;
    for (int c = 0; c < 256; ++c) {
        if (d->lut[c] < 0) continue;
        if (c < 0x40 || c >= 0x80 || d->lut[c ^ 0x20] != d->lut[c]) return false;
        const uint32_t id = static_cast<uint8_t>(d->lut[c]), sh = 8 * (c & 3);
        uint32_t &t = tab[(c & 31) >> 2];
        t = (t & ~(0xFFu << sh)) | (id << sh);
    }
    return true;
}
}  // namespace bsq_packf
