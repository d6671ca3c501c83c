// Span-corruption (T5) batches on the device (gfx950): the encoder inputs, the decoder targets and both body lengths of a packed batch in
// ONE launch.  include/bsq.h documents the rule ("span corruption"); bsq_span_dev.h holds the draw and the text of one lane, which the CPU
// twin runs too.
//
// k_span_corrupt  a wave per row, four rows per 256-thread workgroup; a row of any length in tiles of 1024 characters, 16 per lane, with
//                 (runs, input elements, target elements) so far, the last lane's anchor bits and its last cand bit carried from tile to
//                 tile.  Per tile:
//                 - one guarded unaligned 16-byte load per lane; four selection hashes per lane (its own quads); the anchor bits of the
//                   16 positions in front of the lane come from the lane before it: one __shfl_up, the only exchange the look-back needs;
//                 - cand, then the run starts (one more __shfl_up: cand of the position before the lane);
//                 - a wave scan of the run-start counts gives every position its run index, so the max_sentinels cutoff is a compare;
//                   a second scan, of both output counts in one word, gives the lane its place in the tile's two bodies;
//                 - the lane writes its elements, as int32, into the wave's own LDS region at those places (the only strided accesses,
//                   and they stay on the die); the wave then stores both bodies from LDS as 16-byte vectors aligned in memory,
//                   consecutive lanes on consecutive vectors (flush): single elements only in front of a row's first 16-byte boundary
//                   and at its very end; what a tile leaves over, less than a vector, waits at the front of the region for the next
//                   tile, and everything ends at the cut.
//                 [BOS] and [EOS] go through the same region, and the PAD / ignore_index tails leave as 16-byte vectors too (fill):
//                 every element exactly once, no memset, no atomic.  The element types are chosen at run time (pack16 / store_as:
//                 wave-uniform switches), so this is one kernel.  The four waves of a workgroup never meet after the table is staged.
//                 LDS: 256 + 4 x 2 x 1056 x 4 = 34 048 bytes, static.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>

#include "bsq.h"
#include "bsq_device.h"
#include "bsq_internal.h"
#include "bsq_span_dev.h"

namespace {

using namespace bsq_spand;
using bsq_dev::kThreads;
using bsq_dev::u32x4_unaligned;

constexpr int kRows = kThreads / 64;  // rows of a workgroup

struct SpanParams {
    const uint8_t *chars;
    const int64_t *offsets;
    void *in;   // nullable
    void *lab;  // nullable
    int32_t *in_len, *tgt_len;  // nullable
    int64_t B, P_in, P_tgt;
    int32_t in_dt, lab_dt;
    Geometry g;
    Draw dr;
    int8_t lut[256];
};

// inclusive sum over the wave
__device__ __forceinline__ uint32_t wave_scan(uint32_t x, int lane) {
#pragma unroll
    for (int dlt = 1; dlt < 64; dlt <<= 1) {
        const uint32_t y = __shfl_up(x, dlt);
        if (lane >= dlt) x += y;
    }
    return x;
}

__device__ __forceinline__ void wave_sync_lds() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

// log2 of the element size of a bsq_dtype
__device__ __forceinline__ int32_t size_log2(int32_t dt) { return dt == BSQ_I8 ? 0 : (dt == BSQ_I16 ? 1 : ((dt == BSQ_I32 || dt == BSQ_F32) ? 2 : 3)); }

// The 16 bytes that hold the 16 / size elements get(0), get(1), ... as the element type dt (a wave-uniform switch)
template <typename G>
__device__ __forceinline__ u32x4 pack16(int32_t dt, G &&get) {
    u32x4 r;
    switch (dt) {
    case BSQ_I8:
#pragma unroll
        for (int w = 0; w < 4; ++w)
            r[w] = (static_cast<uint32_t>(get(4 * w)) & 0xFFu) | ((static_cast<uint32_t>(get(4 * w + 1)) & 0xFFu) << 8) |
                   ((static_cast<uint32_t>(get(4 * w + 2)) & 0xFFu) << 16) | (static_cast<uint32_t>(get(4 * w + 3)) << 24);
        break;
    case BSQ_I16:
#pragma unroll
        for (int w = 0; w < 4; ++w) r[w] = (static_cast<uint32_t>(get(2 * w)) & 0xFFFFu) | (static_cast<uint32_t>(get(2 * w + 1)) << 16);
        break;
    case BSQ_I32:
#pragma unroll
        for (int w = 0; w < 4; ++w) r[w] = static_cast<uint32_t>(get(w));
        break;
    case BSQ_F32:
#pragma unroll
        for (int w = 0; w < 4; ++w) r[w] = __float_as_uint(static_cast<float>(get(w)));
        break;
    case BSQ_U64:
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const uint64_t v = static_cast<uint64_t>(get(k));
            r[2 * k] = static_cast<uint32_t>(v), r[2 * k + 1] = static_cast<uint32_t>(v >> 32);
        }
        break;
    default:
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const uint64_t v = static_cast<uint64_t>(__double_as_longlong(static_cast<double>(get(k))));
            r[2 * k] = static_cast<uint32_t>(v), r[2 * k + 1] = static_cast<uint32_t>(v >> 32);
        }
        break;
    }
    return r;
}

// elements of `base` in front of element e that a 16-byte boundary of memory is away (0: e starts a vector); a base that is not
// aligned to its own element size has no such boundary: `n`, so that everything goes out as single elements
__device__ __forceinline__ int64_t to_boundary(const void *base, int64_t e, int32_t lg, int64_t n) {
    const uint64_t a = reinterpret_cast<uint64_t>(base);
    if (a & ((1u << lg) - 1u)) return n;
    const uint32_t vec = 16u >> lg;
    const int64_t head = static_cast<int64_t>((vec - static_cast<uint32_t>(((a >> lg) + static_cast<uint64_t>(e)) & (vec - 1u))) & (vec - 1u));
    return head < n ? head : n;
}

// The elements buf[0 .. n) of the wave's staging region leave for elements e, e + 1, ... of `base`: single elements up to the first
// 16-byte boundary of memory (only a row's first call has any), whole 16-byte vectors from there -- lane l takes vectors l, l + 64, ... --
// and what is left, less than a vector, moves to the front of the region for the next call, which starts at a boundary again.
// Returns how many were left; `last`: they leave as single elements instead, and 0 is returned.  The caller has synchronised the region.
__device__ __noinline__ int32_t flush(int32_t dt, void *base, int64_t e, int32_t *buf, int32_t n, bool last, int lane) {
#if defined(__HIP_DEVICE_COMPILE__)
    __builtin_assume(__builtin_amdgcn_is_shared(buf));  // (a real call: the region's address space does not travel with the pointer)
#endif
    const int32_t lg = size_log2(dt), vec = 16 >> lg;
    const int32_t head = static_cast<int32_t>(to_boundary(base, e, lg, n));
    if (lane < head) store_as(dt, base, e + lane, buf[lane]);  // (head < 16, or a misaligned base: below)
    for (int32_t k = 64 + lane; k < head; k += 64) store_as(dt, base, e + k, buf[k]);
    const int32_t nvec = (n - head) / vec, from = head + nvec * vec, rest = n - from;
    char *out = static_cast<char *>(base) + ((e + head) << lg);
    for (int32_t v = lane; v < nvec; v += 64) {
        const int32_t *s = buf + head + v * vec;
        __builtin_nontemporal_store(pack16(dt, [&](int k) { return static_cast<int64_t>(s[k]); }), reinterpret_cast<u32x4 *>(out) + v);
    }
    if (last) {
        if (lane < rest) store_as(dt, base, e + from + lane, buf[from + lane]);
        return 0;
    }
    const int32_t keep = lane < rest ? buf[from + lane] : 0;  // (rest < 16)
    wave_sync_lds();
    if (lane < rest) buf[lane] = keep;
    return rest;
}

// how many of a tile's `tile` elements a body with `room` elements left takes
__device__ __forceinline__ int32_t fits(int64_t room, int32_t tile) { return room <= 0 ? 0 : (room < tile ? static_cast<int32_t>(room) : tile); }

// elements e .. e + n - 1 of `base` <- v: single elements up to a 16-byte boundary, 16-byte vectors, single elements
__device__ __noinline__ void fill(int32_t dt, void *base, int64_t e, int64_t n, int64_t v, int lane) {
    if (n <= 0) return;
    const int32_t lg = size_log2(dt), vec = 16 >> lg;
    const int64_t head = to_boundary(base, e, lg, n);
    for (int64_t k = lane; k < head; k += 64) store_as(dt, base, e + k, v);
    const int64_t nvec = (n - head) / vec, from = head + nvec * vec;
    const u32x4 x = pack16(dt, [&](int) { return v; });
    u32x4 *out = reinterpret_cast<u32x4 *>(static_cast<char *>(base) + ((e + head) << lg));
    for (int64_t k = lane; k < nvec; k += 64) __builtin_nontemporal_store(x, out + k);
    if (lane < n - from) store_as(dt, base, e + from + lane, v);
}

__global__ __launch_bounds__(kThreads) void k_span_corrupt(const SpanParams p) {
    __shared__ int8_t s_lut[256];
    __shared__ __align__(16) int32_t s_body[kRows][2][kTileOut];
    s_lut[threadIdx.x] = p.lut[threadIdx.x];  // (kThreads == 256)
    __syncthreads();
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t i = static_cast<int64_t>(blockIdx.x) * kRows + wave;  // (wave-uniform)
    if (i >= p.B) return;  // (no workgroup barrier follows)
    int32_t *s_in = s_body[wave][0], *s_tgt = s_body[wave][1];

    const int64_t start = p.offsets[i], total = p.offsets[p.B];
    const int64_t L = p.offsets[i + 1] - start < 0 ? 0 : p.offsets[i + 1] - start;
    const uint64_t h = row_key(p.dr.seed, static_cast<uint64_t>(p.dr.first_row + i));
    const int32_t bos = p.g.bos, eos = p.g.eos;
    const int64_t room_in = p.P_in - bos - eos < 0 ? 0 : p.P_in - bos - eos;
    const int64_t room_tgt = p.P_tgt - eos < 0 ? 0 : p.P_tgt - eos;
    const int64_t in0 = i * p.P_in, lab0 = i * p.P_tgt;

    int64_t n_in = 0, n_tgt = 0, runs = 0;  // of the tiles so far
    uint32_t carry_anchors = 0, carry_cand = 0;  // of lane 63 of the tile before
    // elements of each row that have left for memory, and elements that wait at the front of its staging region (less than a vector):
    // out + pend = bos + min(n_in, room_in), and = min(n_tgt, room_tgt)
    int64_t out_in = 0, out_tgt = 0;
    int32_t pend_in = 0, pend_tgt = 0;
    if (p.in && bos) {
        if (lane == 0) s_in[0] = p.g.bos_id;
        pend_in = 1;
    }

    for (int64_t t0 = 0; t0 < L; t0 += kTile) {
        const int64_t j0 = t0 + lane * kLaneChars, left = L - j0;
        uint32_t W[4] = {0, 0, 0, 0};
        uint32_t own = 0;
        if (left > 0) {
            const int64_t a = start + j0;
            if (a >= 0 && a + 16 <= total) {
                const u32x4_unaligned x = *reinterpret_cast<const u32x4_unaligned *>(p.chars + a);
                W[0] = x.x, W[1] = x.y, W[2] = x.z, W[3] = x.w;
            } else {
#pragma unroll
                for (int c = 0; c < 16; ++c)
                    if (c < left && a + c >= 0 && a + c < total) W[c >> 2] |= static_cast<uint32_t>(p.chars[a + c]) << (8 * (c & 3));
            }
            own = anchor_bits16(h, j0, L, p.dr.t_anchor);
        }
        uint32_t before = __shfl_up(own, 1);
        if (lane == 0) before = carry_anchors;
        Lane ln = lane_masks(s_lut, W, left, own, before, p.dr.span);
        const uint32_t last = (ln.cand >> 15) & 1u;
        uint32_t prev = __shfl_up(last, 1);
        if (lane == 0) prev = carry_cand;
        lane_starts(ln, prev != 0);

        const uint32_t n_starts = static_cast<uint32_t>(popc(ln.starts));
        const uint32_t starts_incl = wave_scan(n_starts, lane);
        const int64_t runs_before = runs + (starts_incl - n_starts);
        const uint32_t sel = lane_selected(ln, runs_before, p.dr.max_sentinels);
        // both counts in one word: a tile adds at most 1024 inputs and 1025 targets
        const uint32_t cnt = static_cast<uint32_t>(lane_inputs(ln, sel)) | (static_cast<uint32_t>(lane_targets(ln, sel)) << 16);
        const uint32_t cnt_incl = wave_scan(cnt, lane);
        const uint32_t excl = cnt_incl - cnt;
        int32_t *lane_in = s_in + pend_in + (excl & 0xFFFFu), *lane_tgt = s_tgt + pend_tgt + (excl >> 16);
        lane_emit(
            s_lut, W, ln, sel, runs_before, p.dr, [=](int32_t n, int32_t v) { lane_in[n] = v; }, [=](int32_t n, int32_t v) { lane_tgt[n] = v; });
        const uint32_t tile_cnt = __shfl(cnt_incl, 63);
        const int32_t tile_in = static_cast<int32_t>(tile_cnt & 0xFFFFu), tile_tgt = static_cast<int32_t>(tile_cnt >> 16);
        wave_sync_lds();
        if (p.in) {
            const int32_t n = pend_in + fits(room_in - n_in, tile_in);
            pend_in = flush(p.in_dt, p.in, in0 + out_in, s_in, n, false, lane);
            out_in += n - pend_in;
        }
        if (p.lab) {
            const int32_t n = pend_tgt + fits(room_tgt - n_tgt, tile_tgt);
            pend_tgt = flush(p.lab_dt, p.lab, lab0 + out_tgt, s_tgt, n, false, lane);
            out_tgt += n - pend_tgt;
        }
        wave_sync_lds();  // (the next tile writes the regions again, behind what waits at their fronts)
        n_in += tile_in;
        n_tgt += tile_tgt;
        runs += __shfl(starts_incl, 63);
        carry_anchors = __shfl(own, 63);
        carry_cand = __shfl(last, 63);
    }

    // what still waits, with the [EOS] behind it, then the tail
    if (p.in) {
        if (eos && out_in + pend_in < p.P_in) {
            if (lane == 0) s_in[pend_in] = p.g.eos_id;
            ++pend_in;
        }
        wave_sync_lds();
        flush(p.in_dt, p.in, in0 + out_in, s_in, pend_in, true, lane);
        out_in += pend_in;
        fill(p.in_dt, p.in, in0 + out_in, p.P_in - out_in, p.g.pad_store, lane);
    }
    if (p.lab) {
        if (eos && out_tgt + pend_tgt < p.P_tgt) {
            if (lane == 0) s_tgt[pend_tgt] = p.g.eos_id;
            ++pend_tgt;
        }
        wave_sync_lds();
        flush(p.lab_dt, p.lab, lab0 + out_tgt, s_tgt, pend_tgt, true, lane);
        out_tgt += pend_tgt;
        fill(p.lab_dt, p.lab, lab0 + out_tgt, p.P_tgt - out_tgt, p.dr.ignore, lane);
    }
    if (lane == 0) {
        if (p.in_len) p.in_len[i] = static_cast<int32_t>(n_in);
        if (p.tgt_len) p.tgt_len[i] = static_cast<int32_t>(n_tgt);
    }
}

}  // namespace

extern "C" {

const char *bsq_span_corrupt_kernel_name(const bsq_desc *d, const bsq_span_corrupt *m, int64_t B, int64_t P_in, int64_t P_tgt, bsq_dtype in_dtype,
                                         bsq_dtype label_dtype) {
    Geometry g;
    Draw dr;
    if (check_args(d, nullptr, nullptr, B, P_in, P_tgt, m, in_dtype, nullptr, label_dtype, nullptr, false, &g, &dr) != BSQ_OK) return "";
    return kernel_name();
}

bsq_status bsq_span_corrupt_device(const bsq_desc *d, const uint8_t *chars, const int64_t *offsets, int64_t B, int64_t P_in, int64_t P_tgt,
                                   const bsq_span_corrupt *m, bsq_dtype in_dtype, void *inputs_or_null, bsq_dtype label_dtype,
                                   void *labels_or_null, int32_t *in_len_or_null, int32_t *tgt_len_or_null, void *hip_stream) {
    SpanParams p;
    const bsq_status st = check_args(d, chars, offsets, B, P_in, P_tgt, m, in_dtype, inputs_or_null, label_dtype, labels_or_null, true, &p.g, &p.dr);
    if (st != BSQ_OK || B == 0) return st;
    if ((B + kRows - 1) / kRows > 0x7FFFFFFF) return bsq_internal::set_error(BSQ_ERR_INVALID_ARG, "more than 2^33 rows");
    std::memcpy(p.lut, d->lut, 256);
    p.chars = chars;
    p.offsets = offsets;
    p.in = inputs_or_null;
    p.lab = labels_or_null;
    p.in_len = in_len_or_null;
    p.tgt_len = tgt_len_or_null;
    p.B = B;
    p.P_in = P_in;
    p.P_tgt = P_tgt;
    p.in_dt = static_cast<int32_t>(in_dtype);
    p.lab_dt = static_cast<int32_t>(label_dtype);
    hipLaunchKernelGGL(k_span_corrupt, dim3(static_cast<unsigned>((B + kRows - 1) / kRows)), dim3(kThreads), 0, static_cast<hipStream_t>(hip_stream), p);
    return bsq_internal::check_launch(kernel_name());
}

}  // extern "C"
