// The rule of codon translation (include/bsq.h, "codon translation"), host + device: the kernels of bsq_translate.hip and the host twin
// bsq_translate_packed_host (bsq_translate_host.cpp) compile the very same text; the numpy twin of tests/translate_twin.py mirrors the
// header's words, not this file.
//
// Inside the library bases are numbered in the order A, C, G, T -- the order one ALU expression on the letter gives -- and the caller's
// table (NCBI order T, C, A, G) is permuted ONCE on the host (make_plan).  In that order the complement of base b is 3 - b, so the index
// of the reverse codon comp(s[q]) comp(s[q - 1]) comp(s[q - 2]) is 63 - index(s[q] s[q - 1] s[q - 2]): no complement table anywhere.
//
// The byte functions come four to a word (code4, bad4: a character per byte of a uint32_t, no carry crosses a byte); the scalar forms the
// host twin and the row tails use are those words with one character in them.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "bsq.h"

namespace bsq_translated {

// base codes of four characters: A / a -> 0, C / c -> 1, G / g -> 2, T / t / U / u -> 3 (bits 1 .. 3 of the letter; any other byte: some code)
__host__ __device__ __forceinline__ uint32_t code4(uint32_t w) { return ((w >> 1) ^ (w >> 2)) & 0x03030303u; }

// the letter A, C, G or T of each code byte
__host__ __device__ __forceinline__ uint32_t canon4(uint32_t code) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_perm(0u, 0x54474341u, code);
#else
    uint32_t r = 0;
    for (int i = 0; i < 4; ++i) r |= ((0x54474341u >> (8 * ((code >> (8 * i)) & 3u))) & 0xFFu) << (8 * i);
    return r;
#endif
}

// 0x80 in every byte whose character is NO base: c & 0xDF (the case bit dropped) is compared with the letter of its own code, U as T
// (bit 0 of a code-3 character is dropped first: 'T' 0x54 and 'U' 0x55 are the only bytes that then equal 'T')
__host__ __device__ __forceinline__ uint32_t bad4(uint32_t w, uint32_t code) {
    const uint32_t t = code & (code >> 1) & 0x01010101u;       // 1 in the bytes of code 3
    const uint32_t x = ((w & 0xDFDFDFDFu) & ~t) ^ canon4(code);  // zero in the bytes that are bases
    return (((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x) & 0x80808080u;
}

__host__ __device__ __forceinline__ bool is_base(uint8_t c) { return (bad4(c, code4(c)) & 0x80u) == 0; }

// index of the codon c0 c1 c2 in the A, C, G, T order (16 * b0 + 4 * b1 + b2), or -1 when one of the three is no base
__host__ __device__ __forceinline__ int32_t codon_index(uint8_t c0, uint8_t c1, uint8_t c2) {
    const uint32_t w = uint32_t(c0) | (uint32_t(c1) << 8) | (uint32_t(c2) << 16);
    const uint32_t c = code4(w);
    if (bad4(w, c) & 0x00808080u) return -1;
    return int32_t(((c & 3u) << 4) | (((c >> 8) & 3u) << 2) | ((c >> 16) & 3u));
}

// phase and strand of a frame code 0 .. 5, and the residues of a source row of L >= 0 characters
__host__ __device__ __forceinline__ int32_t phase_of(int32_t code) { return code >= 3 ? code - 3 : code; }
__host__ __device__ __forceinline__ bool reverse_of(int32_t code) { return code >= 3; }
__host__ __device__ __forceinline__ int64_t row_length(int64_t L, int32_t phase) { return L > phase ? (L - phase) / 3 : 0; }

// index (A, C, G, T order) of residue k of row s[0 .. L) in phase f: forward the codon at f + 3k, reverse 63 - the index of the triple read
// backwards from q = L - 1 - f - 3k; -1: unknown
__host__ __device__ __forceinline__ int32_t residue_index(const uint8_t *s, int64_t L, int32_t f, bool reverse, int64_t k) {
    if (!reverse) {
        const uint8_t *p = s + f + 3 * k;
        return codon_index(p[0], p[1], p[2]);
    }
    const uint8_t *p = s + (L - 1 - f - 3 * k);
    const int32_t i = codon_index(p[0], p[-1], p[-2]);
    return i < 0 ? i : 63 - i;
}

// A bsq_translate checked and reduced to what the rows read (made on the host): the table in A, C, G, T order, four letters per word
struct Plan {
    uint32_t table[16];
    uint32_t unknown4;  // the unknown letter in all four bytes
    int32_t frame;      // 0 .. 5 or BSQ_FRAME_SIX
};

// position in the NCBI order (T, C, A, G) of base b of the A, C, G, T order
__host__ __device__ __forceinline__ constexpr uint32_t ncbi_of(uint32_t b) { return b == 0 ? 2u : b == 1 ? 1u : b == 2 ? 3u : 0u; }

// BSQ_OK and the plan, or BSQ_ERR_INVALID_ARG (message in *why) -- the argument checks every entry point runs before anything else
inline bsq_status make_plan(const bsq_translate *t, bool per_row_frames, Plan *p, const char **why) {
    if (!t) return *why = "bsq_translate is null", BSQ_ERR_INVALID_ARG;
    if (t->frame < 0 || t->frame > BSQ_FRAME_SIX) return *why = "frame must be 0 .. 5 or BSQ_FRAME_SIX", BSQ_ERR_INVALID_ARG;
    if (per_row_frames && t->frame == BSQ_FRAME_SIX) return *why = "per-row frames cannot be combined with BSQ_FRAME_SIX", BSQ_ERR_INVALID_ARG;
    for (uint32_t k = 0; k < 16; ++k) p->table[k] = 0;
    for (uint32_t i = 0; i < 64; ++i) {
        const uint32_t src = 16 * ncbi_of(i >> 4) + 4 * ncbi_of((i >> 2) & 3u) + ncbi_of(i & 3u);
        p->table[i >> 2] |= uint32_t(t->code[src]) << (8 * (i & 3u));
    }
    p->unknown4 = 0x01010101u * t->unknown;
    p->frame = t->frame;
    return BSQ_OK;
}

// the letter of index i (0 .. 63; < 0: unknown) -- the host's lookup; the kernels read the same table with v_perm_b32
__host__ __device__ __forceinline__ uint8_t letter_of(const Plan &p, int32_t i) {
    return uint8_t((i < 0 ? p.unknown4 : p.table[i >> 2] >> (8 * (i & 3))) & 0xFFu);
}

// One output row r of a call: its source row, frame code and validity.  six: r = 6 * i + c; else r = i, c = frames[i] or the plan's frame.
struct RowSrc {
    const int64_t *offsets;
    const int64_t *index;   // nullable
    const uint8_t *frames;  // nullable
    int64_t n_store;
    int32_t frame;          // 0 .. 5 or BSQ_FRAME_SIX
};
struct Row {
    int64_t base;  // position in chars of the source row's first character
    int64_t L;     // its length
    int64_t m;     // residues
    int64_t src;   // source row number i
    int32_t f;     // phase
    bool reverse, ok;
};
__host__ __device__ __forceinline__ Row row_of(const RowSrc &s, int64_t r) {
    Row v{0, 0, 0, r, 0, false, false};
    int32_t c = s.frame;
    if (s.frame == BSQ_FRAME_SIX) {
        v.src = r / 6;
        c = int32_t(r - 6 * v.src);
    } else if (s.frames) {
        c = s.frames[r];
    }
    const int64_t j = s.index ? s.index[v.src] : v.src;
    if (c > 5 || j < 0 || j >= s.n_store) return v;
    const int64_t o0 = s.offsets[j];
    const int64_t L = s.offsets[j + 1] - o0;
    v.base = o0;
    v.L = L > 0 ? L : 0;
    v.f = phase_of(c);
    v.reverse = reverse_of(c);
    v.m = row_length(v.L, v.f);
    v.ok = true;
    return v;
}

}  // namespace bsq_translated
