// What ONE LANE of the fast k-mer kernels does (gfx950), as one text: k_kmer_bp (bsq_kmer.hip), k_kmer_mlm_bp (bsq_kmer_mlm.hip) and the
// stride-1 sweep of the spectrum kernels (bsq_kmer_spectrum.hip) include it.  bsq_kmer_dev.h holds the value of one element and the
// predicate that picks a kernel; this file holds the host fill of the (B, P) kernels' parameter blocks and
//   roll16    the rolling id over a lane's 16 stride-1 windows,
//   lane_ids  the row-piece prologue of a lane and the 16 plain ids of its piece, for both forms.
// (The BOS / id / EOS / PAD choice of a position stays in the two store loops: behind a function the compiler reads the three special ids
// ahead of the branches instead of inside them, which moved k_kmer_bp<sk> and k_kmer_mlm_bp<sk> by +4 .. +6 % on the MI355X: LAB_NOTES.)
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>

#include "bsq.h"
#include "bsq_device.h"
#include "bsq_kmer_dev.h"

namespace bsq_kmerd {

static_assert(kFastThreads == bsq_dev::kThreads, "form_of counts workgroups of kThreads lanes");

// Params, below: the parameter block of a (B, P) k-mer kernel -- KmerParams (bsq_kmer.hip) or KmerMlmParams (bsq_kmer_mlm.hip).  Both hold
//     chars, offsets, B, P, nthreads, div_g (floor(x / pieces per row)), pieces, k_magic / k_shift / k_pow2 (fast_div by k, <sk>), g, lut
// around their own outputs, each in the member order its kernels were tuned with (the first 14 dwords reach a wave in SGPRs), so the
// shared functions are templates on the block instead of taking one embedded struct: with an embedded struct the outputs move behind
// the table, and k_kmer_mlm_bp<sk> on 8-byte elements measured 0.3 - 0.9 % slower in every run (LAB_NOTES).

// Everything of `p` but the geometry (check_shape / check_args have filled p->g): the table and the grid of row pieces
template <typename Params>
inline void fill_lane(Params *p, const bsq_desc *d, const uint8_t *chars, const int64_t *offsets, int64_t B, int64_t P) {
    std::memcpy(p->lut, d->lut, 256);
    p->chars = chars;
    p->offsets = offsets;
    p->B = B;
    p->P = P;
    const int64_t pieces = (P + 15) / 16;
    p->pieces = static_cast<uint32_t>(pieces);
    p->div_g = bsq_dev::div64_constants(static_cast<uint64_t>(pieces));
    p->nthreads = B * pieces;
    bsq_dev::div_constants(static_cast<uint32_t>(p->g.k), &p->k_magic, &p->k_shift, &p->k_pow2);
}

__device__ __forceinline__ void stage_lut(int8_t *s_lut, const int8_t (&lut)[256]) {
    s_lut[threadIdx.x] = lut[threadIdx.x];  // (kThreads == 256)
    __syncthreads();
}

__device__ __forceinline__ uint32_t byte_of(const uint32_t (&w)[4], int c) { return (w[c >> 2] >> (8 * (c & 3))) & 0xFFu; }

// The rolling id over 16 stride-1 windows.  W: the characters that start them, M: the characters, k - 1 further, that end them.
// k - 1 warm-up steps over W, then per window q: the leaving character's weight lead = A^(k-1) is taken off, the entering id added, and
// f(q, id, whole) is called -- whole: the window's k characters are all mapped (a count of mapped characters in a row; id is then the
// Horner sum of the window, < A^k).
template <typename F>
__device__ __forceinline__ void roll16(const uint32_t (&W)[4], const uint32_t (&M)[4], const int8_t *s_lut, int32_t k, int32_t A, uint32_t lead, F &&f) {
    const int32_t km1 = k - 1;
    uint32_t val = 0;
    int32_t run = 0;  // mapped characters in a row, up to the current one
#pragma unroll
    for (int c = 0; c < kMaxK - 1; ++c) {
        if (c < km1) {  // (uniform)
            const int32_t id = s_lut[byte_of(W, c)];
            val = __umul24(val, static_cast<uint32_t>(A)) + static_cast<uint32_t>(id < 0 ? 0 : id);
            run = id < 0 ? 0 : run + 1;
        }
    }
#pragma unroll
    for (int q = 0; q < 16; ++q) {
        if (q > 0) {  // the character that leaves the window
            const int32_t gone = s_lut[byte_of(W, q - 1)];
            val -= __umul24(static_cast<uint32_t>(gone < 0 ? 0 : gone), lead);
        }
        const int32_t id = s_lut[byte_of(M, q)];
        val = __umul24(val, static_cast<uint32_t>(A)) + static_cast<uint32_t>(id < 0 ? 0 : id);
        run = id < 0 ? 0 : run + 1;
        f(q, val, run >= k);
    }
}

// A lane's piece of the (B, P) matrix: 16 consecutive positions of one row (the row-piece mapping of k_mlm_bp, bsq_piece_store.h)
struct Piece {
    int64_t gid, i;  // the piece (a thread past the end computes the last piece again and stores nothing) and its row
    int32_t t0, j0;  // its first position and that position's window index (-1: the BOS of the row)
    int32_t n;       // tokens of the row
    uint32_t n_el;   // positions of the piece inside the row's padlen
    bool valid, staged;  // staged: block-uniform, write_out's
};

// The piece of this thread and ids[q] = the plain id of window j0 + q (V = UNK where a character is unmapped), which means something
// for 0 <= j0 + q < n only.
//   <s1> (SK false) stride 1: the lane's 16 windows are 16 + k - 1 consecutive characters: one 16-byte load of the characters that start a
//        window and one, k - 1 bytes further, of the characters that end one, then roll16.  Two LDS table reads per position, no loop over k.
//   <sk> stride k, 2 <= k <= 8: every window is its own unaligned 8-byte load and a Horner sum of its k characters.
// Loads are whole where they end at or before offsets[B], byte by byte behind that bound otherwise.
template <bool SK, typename Params>
__device__ __forceinline__ Piece lane_ids(const Params &p, const int8_t *s_lut, uint32_t (&ids)[16]) {
    using namespace bsq_dev;
    Piece pc;
    const int64_t first = static_cast<int64_t>(blockIdx.x) * kThreads;
    pc.staged = p.P % 16 == 0 && first + kThreads <= p.nthreads;  // (block-uniform)
    pc.gid = first + threadIdx.x;
    pc.valid = pc.gid < p.nthreads;
    if (!pc.valid) pc.gid = p.nthreads - 1;
    pc.i = static_cast<int64_t>(div64(static_cast<uint64_t>(pc.gid), p.div_g));
    pc.t0 = static_cast<int32_t>(pc.gid - pc.i * p.pieces) * 16;
    const int32_t P = static_cast<int32_t>(p.P);
    pc.n_el = static_cast<uint32_t>(P - pc.t0 < 16 ? P - pc.t0 : 16);
    const int64_t start = p.offsets[pc.i], total = p.offsets[p.B];
    const int64_t L64 = p.offsets[pc.i + 1] - start;
    const int32_t k = p.g.k, bos = p.g.bos, A = p.g.A;
    const uint32_t V = static_cast<uint32_t>(p.g.V), lead = static_cast<uint32_t>(p.g.lead);
    const int32_t room = P - bos - p.g.eos < 0 ? 0 : P - bos - p.g.eos;
    // characters of the row that can matter, as 32 bits: (room + 1) * k of them hold more than `room` windows at either stride
    const int32_t cap = (room + 1) * k;
    const int32_t L = L64 < 0 ? 0 : (L64 > cap ? cap : static_cast<int32_t>(L64));
    int32_t n;
    if (SK) n = static_cast<int32_t>(fast_div(static_cast<uint32_t>(L), p.k_magic, p.k_shift, p.k_pow2));
    else n = L < k ? 0 : L - k + 1;
    n = n < room ? n : room;
    pc.n = n;
    const int32_t j0 = pc.j0 = pc.t0 - bos;

    if (!SK) {
        // W: the characters j0 .. j0 + 15 (each starts a window of the piece), M: j0 + k - 1 .. j0 + k + 14 (each ends one)
        uint32_t W[4] = {0, 0, 0, 0}, M[4] = {0, 0, 0, 0};
        const int32_t km1 = k - 1;
        if (j0 < n) {
            const int64_t a = start + j0;
            if (a >= 0 && a + km1 + 16 <= total) {
                const u32x4_unaligned x = *reinterpret_cast<const u32x4_unaligned *>(p.chars + a);
                const u32x4_unaligned y = *reinterpret_cast<const u32x4_unaligned *>(p.chars + a + km1);
                W[0] = x.x, W[1] = x.y, W[2] = x.z, W[3] = x.w;
                M[0] = y.x, M[1] = y.y, M[2] = y.z, M[3] = y.w;
            } else {
#pragma unroll
                for (int c = 0; c < 16; ++c) {
                    const int32_t jw = j0 + c, jm = jw + km1;
                    if (jw >= 0 && jw < L && start + jw < total) W[c >> 2] |= static_cast<uint32_t>(p.chars[start + jw]) << (8 * (c & 3));
                    if (jm >= 0 && jm < L && start + jm < total) M[c >> 2] |= static_cast<uint32_t>(p.chars[start + jm]) << (8 * (c & 3));
                }
            }
        }
        roll16(W, M, s_lut, k, A, lead, [&](int q, uint32_t id, bool whole) { ids[q] = whole ? id : V; });
    } else {
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const int32_t j = j0 + q;
            uint32_t id_q = V;
            if (j >= 0 && j < n) {
                const int64_t a = start + static_cast<int64_t>(j) * k;
                uint64_t w = 0;
                if (a >= 0 && a + 8 <= total) {
                    w = *reinterpret_cast<const u64_unaligned *>(p.chars + a);
                } else {
#pragma unroll
                    for (int c = 0; c < kMaxSkK; ++c)
                        if (c < k && a + c >= 0 && a + c < total) w |= static_cast<uint64_t>(p.chars[a + c]) << (8 * c);
                }
                uint32_t val = 0;
                bool unk = false;
#pragma unroll
                for (int c = 0; c < kMaxSkK; ++c) {
                    if (c < k) {  // (uniform)
                        const int32_t id = s_lut[static_cast<uint32_t>(w >> (8 * c)) & 0xFFu];
                        unk |= id < 0;
                        val = __umul24(val, static_cast<uint32_t>(A)) + static_cast<uint32_t>(id < 0 ? 0 : id);
                    }
                }
                id_q = unk ? V : val;
            }
            ids[q] = id_q;
        }
    }
    return pc;
}

}  // namespace bsq_kmerd
