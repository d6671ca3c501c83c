// Masked-LM batches on the device (gfx950): the masked inputs + labels of BERT's objective in one launch, and the random keep-mask of
// training/cnnpretrain.py:119-124 (the reference) as a byte mask for the masked one-hot.  The draw is bsq_mlm_dev.h (include/bsq.h documents it).
//
// k_mlm_bp   (B, P): a lane owns 16 consecutive positions of one row (rows are cut into ceil(P / 16) pieces, the last one partial -- the
//            row-piece mapping of the chunk kernels), so for P % 16 == 0 the 64 lanes of a wave cover 1024 consecutive positions: one
//            4-KiB chunk of an int8 input matrix.  One unaligned 16-byte character load, 4 selection hashes (5 with BOS), a replacement
//            hash per selected character, and 16 * sizeof(T) bytes per output as 16-byte non-temporal stores (2- to 8-byte elements
//            through LDS, so that a wave's stores are whole 1-KiB runs: write_out, bsq_piece_store.h).
// k_mlm_pb   (P, B): one thread per element, positions of a row of the matrix spread over consecutive sequences (correct, not tuned).
// k_mlm_mask one wave per sequence, a lane per 4 characters (one selection hash each).
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>

#include "bsq.h"
#include "bsq_device.h"
#include "bsq_internal.h"
#include "bsq_mlm_dev.h"
#include "bsq_piece_store.h"

namespace {

using namespace bsq_dev;  // kThreads, Div64, store16_unaligned, write_out (bsq_piece_store.h)
using bsq_mlmd::Thresholds;

struct MlmParams {
    const uint8_t *chars;
    const int64_t *offsets;
    void *in;   // nullable
    void *lab;  // nullable
    int64_t B, P, first_row, nthreads;
    uint64_t seed;
    int64_t mask_token, ignore;
    Div64 div_g;  // floor(x / pieces per row)
    uint32_t pieces;
    Thresholds th;
    int32_t nchars, room, bos, eos, bos_id, eos_id, pad_id, padchar;
    int8_t lut[256];
};

__device__ __forceinline__ void stage_lut(int8_t *s_lut, const MlmParams &p) {
    s_lut[threadIdx.x] = p.lut[threadIdx.x];  // (kThreads == 256)
    __syncthreads();
}

template <typename TI, typename TL>
__global__ __launch_bounds__(kThreads) void k_mlm_bp(const MlmParams p) {
    __shared__ int8_t s_lut[256];
    constexpr int kWide = sizeof(TI) > sizeof(TL) ? sizeof(TI) : sizeof(TL);
    __shared__ __align__(16) uint4 s_out[kWide > 1 ? kThreads * kWide : 1];
    stage_lut(s_lut, p);
    const int64_t first = static_cast<int64_t>(blockIdx.x) * kThreads;
    const bool staged = p.P % 16 == 0 && first + kThreads <= p.nthreads;  // (block-uniform)
    int64_t gid = first + threadIdx.x;
    const bool valid = gid < p.nthreads;
    if (!valid) gid = p.nthreads - 1;  // (a thread past the end computes the last piece again and stores nothing)
    const int64_t i = static_cast<int64_t>(div64(static_cast<uint64_t>(gid), p.div_g));
    const uint32_t g = static_cast<uint32_t>(gid - i * p.pieces);
    const int64_t t0 = static_cast<int64_t>(g) * 16;
    const uint32_t n = static_cast<uint32_t>(p.P - t0 < 16 ? p.P - t0 : 16);
    const int64_t start = p.offsets[i], total = p.offsets[p.B];
    int64_t L = p.offsets[i + 1] - start;
    L = L < 0 ? 0 : (L > p.room ? p.room : L);
    const int64_t j0 = t0 - p.bos;  // character index of the piece's first position (-1: the BOS of the row)

    // the characters of positions t0 .. t0 + 15: one unaligned 16-byte load when the window lies inside the buffer
    uint32_t cw[4] = {0, 0, 0, 0};
    if (j0 < L) {
        const int64_t a = start + j0;
        if (a >= 0 && a + 16 <= total) {
            const u32x4_unaligned x = *reinterpret_cast<const u32x4_unaligned *>(p.chars + a);
            cw[0] = x.x, cw[1] = x.y, cw[2] = x.z, cw[3] = x.w;
        } else {
#pragma unroll
            for (int k = 0; k < 16; ++k) {
                const int64_t j = j0 + k;
                if (j >= 0 && j < L) cw[k >> 2] |= static_cast<uint32_t>(p.chars[start + j]) << (8 * (k & 3));
            }
        }
    }

    // selection bits: the words of quads qb .. qb + 4 (qb = floor(j0 / 4)), bit 4 (q - qb) + (j & 3) for character j; position k of
    // the piece is bit k + (j0 - 4 qb) = k + 3 * bos
    const uint64_t h = bsq_mlmd::row_key(p.seed, static_cast<uint64_t>(p.first_row + i));
    const int64_t qb = (j0 + 4) / 4 - 1;  // floor for j0 >= -1
    uint32_t bits = 0;
#pragma unroll
    for (int q = 0; q < 5; ++q) {
        const int64_t qq = qb + q;
        if (qq >= 0 && qq * 4 < L && (q < 4 || p.bos)) {
            const uint64_t w = bsq_mlmd::select_word(h, static_cast<uint64_t>(qq));
#pragma unroll
            for (int l = 0; l < 4; ++l) bits |= static_cast<uint32_t>(bsq_mlmd::lane16(w, l) < p.th.sel) << (4 * q + l);
        }
    }
    bits >>= 3 * p.bos;

    const TL ign = static_cast<TL>(p.ignore);
    TI vin[16];
    TL vlab[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        const int64_t j = j0 + k;
        int64_t plain, input;
        bool sel = false;
        if (j < 0) {
            plain = p.bos_id;
        } else if (j < L) {
            const int32_t id = s_lut[(cw[k >> 2] >> (8 * (k & 3))) & 0xFFu];
            plain = id >= 0 ? id : 0;
            sel = id >= 0 && ((bits >> k) & 1u);
        } else if (p.eos && j == L) {
            plain = p.eos_id;
        } else {
            plain = p.padchar ? p.pad_id : 0;
        }
        input = plain;
        if (sel) input = bsq_mlmd::replace(bsq_mlmd::replace_word(h, static_cast<uint64_t>(j)), p.th, p.mask_token, p.nchars, plain);
        vin[k] = static_cast<TI>(input);
        vlab[k] = sel ? static_cast<TL>(plain) : ign;
    }
    const int64_t e0 = i * p.P + t0;
    if (p.in) write_out(static_cast<TI *>(p.in), gid, e0, vin, n, valid, staged, s_out);
    if (p.lab) write_out(static_cast<TL *>(p.lab), gid, e0, vlab, n, valid, staged, s_out);
}

template <typename T>
__device__ __forceinline__ void put(void *base, int64_t e, int64_t v) {
    __builtin_nontemporal_store(static_cast<T>(v), static_cast<T *>(base) + e);
}
__device__ __forceinline__ void put_as(void *base, int32_t t, int64_t e, int64_t v) {
    switch (t) {
    case BSQ_I8: put<int8_t>(base, e, v); break;
    case BSQ_I16: put<int16_t>(base, e, v); break;
    case BSQ_I32: put<int32_t>(base, e, v); break;
    case BSQ_U64: put<uint64_t>(base, e, v); break;
    case BSQ_F32: put<float>(base, e, v); break;
    default: put<double>(base, e, v); break;
    }
}

__global__ __launch_bounds__(kThreads) void k_mlm_pb(const MlmParams p, int32_t tin, int32_t tlab) {
    __shared__ int8_t s_lut[256];
    stage_lut(s_lut, p);
    const int64_t n = p.B * p.P;
    const int64_t stride = static_cast<int64_t>(gridDim.x) * kThreads;
    for (int64_t e = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x; e < n; e += stride) {
        const int64_t t = e / p.B, b = e - t * p.B;
        const int64_t start = p.offsets[b];
        int64_t L = p.offsets[b + 1] - start;
        L = L < 0 ? 0 : (L > p.room ? p.room : L);
        const int64_t j = t - p.bos;
        int64_t plain;
        bool sel = false;
        uint64_t h = 0;
        if (j < 0) {
            plain = p.bos_id;
        } else if (j < L) {
            const int32_t id = s_lut[p.chars[start + j]];
            plain = id >= 0 ? id : 0;
            if (id >= 0) {
                h = bsq_mlmd::row_key(p.seed, static_cast<uint64_t>(p.first_row + b));
                sel = bsq_mlmd::lane16(bsq_mlmd::select_word(h, static_cast<uint64_t>(j >> 2)), static_cast<uint32_t>(j)) < p.th.sel;
            }
        } else if (p.eos && j == L) {
            plain = p.eos_id;
        } else {
            plain = p.padchar ? p.pad_id : 0;
        }
        if (p.in) {
            const int64_t input =
                sel ? bsq_mlmd::replace(bsq_mlmd::replace_word(h, static_cast<uint64_t>(j)), p.th, p.mask_token, p.nchars, plain) : plain;
            put_as(p.in, tin, e, input);
        }
        if (p.lab) put_as(p.lab, tlab, e, sel ? plain : p.ignore);
    }
}

// mask[offsets[i] + j] = 0 if selected else 1; one wave per sequence (grid-stride), a lane per quad of characters
__global__ __launch_bounds__(kThreads) void k_mlm_mask(const MlmParams p, uint8_t *mask) {
    __shared__ int8_t s_lut[256];
    stage_lut(s_lut, p);
    const int lane = threadIdx.x & 63;
    const int64_t waves = static_cast<int64_t>(gridDim.x) * (kThreads / 64);
    for (int64_t i = static_cast<int64_t>(blockIdx.x) * (kThreads / 64) + (threadIdx.x >> 6); i < p.B; i += waves) {
        const int64_t start = p.offsets[i], L = p.offsets[i + 1] - start;
        const uint64_t h = bsq_mlmd::row_key(p.seed, static_cast<uint64_t>(p.first_row + i));
        for (int64_t q = lane; q * 4 < L; q += 64) {
            const uint64_t w = bsq_mlmd::select_word(h, static_cast<uint64_t>(q));
#pragma unroll
            for (int l = 0; l < 4; ++l) {
                const int64_t j = q * 4 + l;
                if (j < L) {
                    const bool sel = s_lut[p.chars[start + j]] >= 0 && bsq_mlmd::lane16(w, l) < p.th.sel;
                    mask[start + j] = sel ? 0 : 1;
                }
            }
        }
    }
}

bsq_status fill_params(MlmParams &p, const bsq_desc *d, const uint8_t *chars, const int64_t *offsets, int64_t B, int64_t P,
                       const bsq_mlm *m) {
    const char *why = "";
    if (bsq_mlmd::make_thresholds(m, &p.th, &why) != BSQ_OK) return bsq_internal::set_error(BSQ_ERR_INVALID_ARG, why);
    std::memcpy(p.lut, d->lut, 256);
    p.chars = chars;
    p.offsets = offsets;
    p.in = p.lab = nullptr;
    p.B = B;
    p.P = P;
    p.first_row = m->first_row;
    p.seed = m->seed;
    p.mask_token = m->mask_token;
    p.ignore = m->ignore_index;
    p.nchars = d->nchars;
    p.bos = d->bos ? 1 : 0;
    p.eos = d->eos ? 1 : 0;
    p.room = static_cast<int32_t>(P - p.bos - p.eos < 0 ? 0 : (P - p.bos - p.eos > INT32_MAX ? INT32_MAX : P - p.bos - p.eos));
    p.bos_id = bsq_bos_id(d);
    p.eos_id = bsq_eos_id(d);
    p.pad_id = bsq_pad_id(d);
    p.padchar = d->padchar;
    return BSQ_OK;
}

bool dtype_ok(bsq_dtype t) { return t >= BSQ_I8 && t <= BSQ_F64; }

using bsq_internal::check_launch;

template <typename TI>
bsq_status launch_bp_in(const MlmParams &p, bsq_dtype tl, unsigned grid, hipStream_t s) {
#define BSQ_MLM(TL) hipLaunchKernelGGL((k_mlm_bp<TI, TL>), dim3(grid), dim3(kThreads), 0, s, p)
    switch (tl) {
    case BSQ_I8: BSQ_MLM(int8_t); break;
    case BSQ_I16: BSQ_MLM(int16_t); break;
    case BSQ_I32: BSQ_MLM(int32_t); break;
    case BSQ_U64: BSQ_MLM(uint64_t); break;
    case BSQ_F32: BSQ_MLM(float); break;
    default: BSQ_MLM(double); break;
    }
#undef BSQ_MLM
    return check_launch("k_mlm_bp");
}

}  // namespace

extern "C" {

bsq_status bsq_mlm_tokenize_device(const bsq_desc *d, const uint8_t *chars, const int64_t *offsets, int64_t B, int64_t P,
                                   int32_t batch_first, const bsq_mlm *m, bsq_dtype in_dtype, void *inputs_or_null,
                                   bsq_dtype label_dtype, void *labels_or_null, void *hip_stream) {
    if (!d || B < 0 || P <= 0 || (B > 0 && !offsets))
        return bsq_internal::set_error(BSQ_ERR_INVALID_ARG, "null pointer, B < 0 or padlen <= 0");
    if (!inputs_or_null && !labels_or_null) return bsq_internal::set_error(BSQ_ERR_INVALID_ARG, "both outputs are null");
    if (!dtype_ok(in_dtype) || !dtype_ok(label_dtype)) return bsq_internal::set_error(BSQ_ERR_DTYPE, "bad bsq_dtype");
    MlmParams p;
    const bsq_status st = fill_params(p, d, chars, offsets, B, P, m);
    if (st != BSQ_OK) return st;
    if (B == 0) return BSQ_OK;
    if (!chars) return bsq_internal::set_error(BSQ_ERR_INVALID_ARG, "chars is null");
    p.in = inputs_or_null;
    p.lab = labels_or_null;
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    if (!batch_first) {
        const int64_t blocks = (B * P + kThreads - 1) / kThreads;
        const unsigned grid = static_cast<unsigned>(blocks > 256 * 64 ? 256 * 64 : blocks);
        hipLaunchKernelGGL(k_mlm_pb, dim3(grid), dim3(kThreads), 0, s, p, static_cast<int32_t>(in_dtype), static_cast<int32_t>(label_dtype));
        return check_launch("k_mlm_pb");
    }
    const int64_t pieces = (P + 15) / 16;
    if (pieces > INT32_MAX) return bsq_internal::set_error(BSQ_ERR_INVALID_ARG, "padlen too large");
    p.pieces = static_cast<uint32_t>(pieces);
    p.div_g = div64_constants(static_cast<uint64_t>(pieces));
    p.nthreads = B * pieces;
    const int64_t blocks = (p.nthreads + kThreads - 1) / kThreads;
    if (blocks >= (int64_t(1) << 31)) return bsq_internal::set_error(BSQ_ERR_INVALID_ARG, "batch too large");
    const unsigned grid = static_cast<unsigned>(blocks);
    switch (in_dtype) {
    case BSQ_I8: return launch_bp_in<int8_t>(p, label_dtype, grid, s);
    case BSQ_I16: return launch_bp_in<int16_t>(p, label_dtype, grid, s);
    case BSQ_I32: return launch_bp_in<int32_t>(p, label_dtype, grid, s);
    case BSQ_U64: return launch_bp_in<uint64_t>(p, label_dtype, grid, s);
    case BSQ_F32: return launch_bp_in<float>(p, label_dtype, grid, s);
    default: return launch_bp_in<double>(p, label_dtype, grid, s);
    }
}

bsq_status bsq_random_mask_device(const bsq_desc *d, const uint8_t *chars, const int64_t *offsets, int64_t B, const bsq_mlm *m,
                                  uint8_t *mask_out, void *hip_stream) {
    if (!d || B < 0 || (B > 0 && (!offsets || !mask_out))) return bsq_internal::set_error(BSQ_ERR_INVALID_ARG, "null pointer or B < 0");
    MlmParams p;
    const bsq_status st = fill_params(p, d, chars, offsets, B, 1, m);
    if (st != BSQ_OK) return st;
    if (B == 0) return BSQ_OK;
    if (!chars) return bsq_internal::set_error(BSQ_ERR_INVALID_ARG, "chars is null");
    const int64_t blocks = (B + 3) / 4;
    const unsigned grid = static_cast<unsigned>(blocks > 256 * 64 ? 256 * 64 : blocks);
    hipLaunchKernelGGL(k_mlm_mask, dim3(grid), dim3(kThreads), 0, static_cast<hipStream_t>(hip_stream), p, mask_out);
    return check_launch("k_mlm_mask");
}

bsq_status bsq_random_mask_host(const bsq_desc *d, const uint8_t *chars, const int64_t *offsets, int64_t B, const bsq_mlm *m,
                                uint8_t *mask_out) {
    if (!d || B < 0 || (B > 0 && (!offsets || !mask_out))) return bsq_internal::set_error(BSQ_ERR_INVALID_ARG, "null pointer or B < 0");
    Thresholds th;
    const char *why = "";
    if (bsq_mlmd::make_thresholds(m, &th, &why) != BSQ_OK) return bsq_internal::set_error(BSQ_ERR_INVALID_ARG, why);
    for (int64_t i = 0; i < B; ++i) {
        const int64_t start = offsets[i], L = offsets[i + 1] - start;
        if (L > 0 && !chars) return bsq_internal::set_error(BSQ_ERR_INVALID_ARG, "chars is null");
        const uint64_t h = bsq_mlmd::row_key(m->seed, static_cast<uint64_t>(m->first_row + i));
        uint64_t w = 0;
        for (int64_t j = 0; j < L; ++j) {
            if ((j & 3) == 0) w = bsq_mlmd::select_word(h, static_cast<uint64_t>(j >> 2));
            const bool sel = d->lut[chars[start + j]] >= 0 && bsq_mlmd::lane16(w, static_cast<uint32_t>(j)) < th.sel;
            mask_out[start + j] = sel ? 0 : 1;
        }
    }
    return BSQ_OK;
}

}  // extern "C"
