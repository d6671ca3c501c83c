// The rule of open reading frames (include/bsq.h, "open reading frames"), host + device: the kernels of bsq_orf.hip and the host twins
// bsq_orf_count_host / bsq_orf_emit_host (bsq_orf_host.cpp) compile the very same text; the numpy twin of tests/orf_twin.py mirrors the
// header's words, not this file.
//
// A row is walked in PIECES of 64 residues.  A piece is two 64-bit masks -- bit i: residue base + i is the stop byte / the start byte,
// bits at and past the row's end clear -- and the walk carries two positions across pieces: the last stop seen and, in start mode, the
// first start residue behind it.  Every stop bit closes its segment (piece_step), the row's end closes the last one (row_end).  The
// masks come sixteen residues at a time from four words (mask16: an exact zero-byte test on w ^ byte, no carry crosses a byte).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "bsq.h"

namespace bsq_orfs {

constexpr int kPiece = 64;  // residues of a piece
constexpr int kChunk = 16;  // residues of one mask16 (a 16-byte load)

// A bsq_orf checked and reduced to what the rows read (made on the host)
struct Rule {
    uint32_t stop4;   // the stop byte in all four bytes of a word
    uint32_t start4;  // the start byte likewise (start mode only)
    int64_t min_len;
    bool start_mode;
};

// BSQ_OK and the rule, or BSQ_ERR_INVALID_ARG (message in *why) -- the argument checks every entry point runs before anything else
inline bsq_status make_rule(const bsq_orf *o, Rule *r, const char **why) {
    if (!o) return *why = "bsq_orf is null", BSQ_ERR_INVALID_ARG;
    if (o->min_len < 1) return *why = "min_len must be >= 1", BSQ_ERR_INVALID_ARG;
    if (o->start < -1 || o->start > 255) return *why = "start must be -1 (none) or a byte value 0 .. 255", BSQ_ERR_INVALID_ARG;
    if (o->start == int32_t(o->stop)) return *why = "start and stop must differ", BSQ_ERR_INVALID_ARG;
    r->stop4 = 0x01010101u * o->stop;
    r->start_mode = o->start >= 0;
    r->start4 = r->start_mode ? 0x01010101u * uint32_t(o->start) : 0u;
    r->min_len = o->min_len;
    return BSQ_OK;
}

// bit i = (byte i of w == byte i of b4), i < 4
__host__ __device__ __forceinline__ uint32_t eq4(uint32_t w, uint32_t b4) {
    const uint32_t x = w ^ b4;                                                    // zero in the bytes that match
    const uint32_t z = ~(((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x) & 0x80808080u;    // 0x80 in exactly those bytes
    return ((z >> 7) * 0x10204080u) >> 28;                                        // bits 0, 8, 16, 24 -> bits 0 .. 3
}

// bit i = (residue i of the sixteen in w[0 .. 4) == the byte of b4)
__host__ __device__ __forceinline__ uint32_t mask16(const uint32_t *w, uint32_t b4) {
    return eq4(w[0], b4) | (eq4(w[1], b4) << 4) | (eq4(w[2], b4) << 8) | (eq4(w[3], b4) << 12);
}

// the low n bits set, n in 0 .. 16
__host__ __device__ __forceinline__ uint32_t low_bits16(int64_t n) { return n >= 16 ? 0xFFFFu : n <= 0 ? 0u : (1u << n) - 1u; }

// What a row's walk carries from piece to piece
struct Carry {
    int64_t last_stop;    // position of the last stop seen, -1: none yet
    int64_t first_start;  // start mode: position of the first start residue behind last_stop, -1: none yet
};
__host__ __device__ __forceinline__ Carry row_begin() { return Carry{-1, -1}; }

// the segment that terminator e closes: emit(s, e - s) when it yields an ORF.  t: position of the segment's first start residue or -1.
template <class Emit>
__host__ __device__ __forceinline__ void close_segment(const Rule &r, const Carry &c, int64_t t, int64_t e, Emit &emit) {
    const int64_t s = r.start_mode ? t : c.last_stop + 1;
    if (s >= 0 && e - s >= r.min_len) emit(s, e - s);
}

// One piece: the residues [base, base + 64) as stop mask S and start mask T
template <class Emit>
__host__ __device__ __forceinline__ void piece_step(const Rule &r, Carry &c, uint64_t S, uint64_t T, int64_t base, Emit &emit) {
    while (S) {
        const int b = __builtin_ctzll(S);
        int64_t t = c.first_start;
        if (r.start_mode && t < 0) {
            const uint64_t before = T & ((uint64_t(1) << b) - 1u);  // start residues of this segment in this piece
            if (before) t = base + __builtin_ctzll(before);
        }
        close_segment(r, c, t, base + b, emit);
        c.last_stop = base + b;
        c.first_start = -1;
        T &= (~uint64_t(0) << b) << 1;  // what lies behind this stop
        S &= S - 1;
    }
    if (r.start_mode && c.first_start < 0 && T) c.first_start = base + __builtin_ctzll(T);
}

// The row's end, m = its length: the last terminator
template <class Emit>
__host__ __device__ __forceinline__ void row_end(const Rule &r, const Carry &c, int64_t m, Emit &emit) {
    close_segment(r, c, c.first_start, m, emit);
}

}  // namespace bsq_orfs
