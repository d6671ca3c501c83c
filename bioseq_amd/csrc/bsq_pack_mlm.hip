// Masked-LM batches over sequence-packed rows (gfx950): include/bsq.h ("sequence packing", bsq_pack_mlm_tokenize_device) has the rule,
// bsq_pack_dev.h the value of one position (run_mlm_token) as host + device code, bsq_pack_host.cpp the CPU twin.
//
// k_pack_mlm_flat<TI, TL, PERM>  k_pack_flat (bsq_pack.hip) with the draw of k_mlm_bp (bsq_mlm.hip) inside: a lane owns 16 consecutive
//            positions of the flat (rows, P) output, a wave 1024; the wave's seeds come from find_wave, a Cursor carries the sequence, and
//            write_out stores whole 1-KiB runs per wave.  A lane whose 16 positions lie inside the characters of one run takes one
//            unaligned 16-byte load, the table lookup (<perm>: the folded register table with a "mapped" flag in bit 7 of every entry;
//            <lut>: the LDS byte table), the selection words of quads floor(j0 / 4) .. floor((j0 + 15) / 4) -- four when j0 % 4 == 0, five
//            otherwise: unlike a padded row, a run may start at any column, so j0 has any residue -- and one replacement word per
//            selected character.  Every other lane goes position by position through run_mlm_token.
//            Registers: what crosses from the inputs to the labels is 16 plain ids as bytes and 16 selection bits (five registers),
//            so the inputs are stored before the labels are built and only one 16-element array of the wide type is live at a time.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>

#include "bsq.h"
#include "bsq_device.h"
#include "bsq_internal.h"
#include "bsq_mlm_dev.h"
#include "bsq_pack_dev.h"
#include "bsq_pack_flat.h"
#include "bsq_piece_store.h"

namespace {

using namespace bsq_dev;    // kThreads, Div64, write_out
using namespace bsq_packf;  // lookup4_perm, nonletter_mask, find_wave, fold_table
using bsq_packd::Cursor;
using bsq_packd::Ids;
using bsq_packd::MlmDraw;

struct PackMlmParams {
    const uint8_t *chars;
    const int64_t *offsets, *starts;
    void *in, *lab;      // either may be null, not both
    int32_t *seg, *pos;  // either may be null
    int64_t B, P, total, npieces;
    Div64 div_P;
    Ids ids;
    MlmDraw draw;
    uint32_t tab[8];  // PERM: (id | 0x80) of letter (c & 31), 0 for an unmapped one
    int8_t lut[256];
};

// bit b of the result = bit 7 of byte b of w
__device__ __forceinline__ uint32_t top_bits(uint32_t w) { return ((((w >> 7) & 0x01010101u) * 0x01020408u) >> 24) & 0xFu; }

template <typename TI, typename TL, bool PERM>
__global__ __launch_bounds__(kThreads) __attribute__((amdgpu_waves_per_eu(4))) void k_pack_mlm_flat(const PackMlmParams p) {
    __shared__ int8_t s_lut[256];
    constexpr size_t kIn = sizeof(TI) > 4 ? sizeof(TI) : 4, kWide = sizeof(TL) > kIn ? sizeof(TL) : kIn;  // (seg / pos: 4-byte elements)
    __shared__ __align__(16) uint4 s_out[kThreads * kWide];
    s_lut[threadIdx.x] = p.lut[threadIdx.x];  // (kThreads == 256)
    __syncthreads();
    const int64_t first = static_cast<int64_t>(blockIdx.x) * kThreads;
    const bool staged = (first + kThreads) * 16 <= p.total;  // (block-uniform: every piece of the block is whole)
    int64_t gid = first + threadIdx.x;
    const bool valid = gid < p.npieces;
    if (!valid) gid = p.npieces - 1;  // (a thread past the end computes the last piece again and stores nothing)
    const int64_t q0 = gid * 16;
    const uint32_t n_el = static_cast<uint32_t>(p.total - q0 < 16 ? p.total - q0 : 16);
    const int64_t be = p.ids.bos + p.ids.eos, B = p.B, P = p.P;
    const int64_t nchars = B > 0 ? p.offsets[B] : 0;

    // the wave's seeds and the lane's cursor, as in k_pack_flat
    int64_t gw = first + (threadIdx.x & ~63u);
    gw = gw < p.npieces ? gw : p.npieces - 1;
    const int64_t row_w = static_cast<int64_t>(div64(static_cast<uint64_t>(gw * 16), p.div_P));
    const int64_t seed_row = find_wave(p.starts, B, static_cast<uint64_t>(row_w * P));
    const int64_t seed = find_wave(p.starts, B, static_cast<uint64_t>(gw * 16));
    const int64_t row0 = static_cast<int64_t>(div64(static_cast<uint64_t>(q0), p.div_P));
    int64_t col = q0 - row0 * P;
    int64_t i_first = row0 == row_w ? seed_row : bsq_packd::find(p.starts, B, seed_row, static_cast<uint64_t>(row0 * P));
    Cursor c = bsq_packd::cursor_at(p.offsets, p.starts, B, be, bsq_packd::find(p.starts, B, seed, static_cast<uint64_t>(q0)));
    uint64_t h = bsq_mlmd::row_key(p.draw.seed, static_cast<uint64_t>(p.draw.first_row + c.i));  // (unused while c.i == -1)

    TI vin[16];
    int32_t sg[16], ps[16];
    uint32_t pl[4] = {0, 0, 0, 0};  // the plain ids of the 16 positions, a byte each: read back for SELECTED positions only, which are mapped
                                    // characters (ids 0 .. 127, the table is int8); a BOS / EOS / PAD id beyond 255 (BYTES) is cut here unread
    uint32_t selm = 0;              // bit k: position k is a selected character
    const int64_t j0 = q0 - c.s - p.ids.bos, a0 = c.off + j0;
    const bool fast = c.i >= 0 && n_el == 16 && j0 >= 0 && j0 + 16 <= c.L && static_cast<uint64_t>(q0) + 16 <= c.e && col + 16 <= P &&
                      a0 >= 0 && a0 + 16 <= nchars;
    if (fast) {
        const u32x4_unaligned x = *reinterpret_cast<const u32x4_unaligned *>(p.chars + a0);
        const uint32_t cw[4] = {x.x, x.y, x.z, x.w};
        uint32_t mapped = 0;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            uint32_t w;  // (id | 0x80) of a mapped character, 0 of an unmapped one
            if constexpr (PERM) {
                w = lookup4_perm(cw[u], p.tab) & ~nonletter_mask(cw[u]);
            } else {
                w = 0;
#pragma unroll
                for (int b = 0; b < 4; ++b) {
                    const int32_t id = s_lut[(cw[u] >> (8 * b)) & 0xFFu];
                    w |= (id < 0 ? 0u : static_cast<uint32_t>(id) | 0x80u) << (8 * b);
                }
            }
            mapped |= top_bits(w) << (4 * u);
            pl[u] = w & 0x7F7F7F7Fu;
        }
        // selection bits of characters 4 qb .. 4 qb + 19 (qb = floor(j0 / 4)): position k of the piece is bit k + (j0 & 3)
        const uint32_t r = static_cast<uint32_t>(j0) & 3u;
        const uint64_t qb = static_cast<uint64_t>(j0) >> 2;
        uint32_t bits = 0;
#pragma unroll
        for (int q = 0; q < 5; ++q) {
            if (q < 4 || r != 0) {
                const uint64_t w = bsq_mlmd::select_word(h, qb + q);
#pragma unroll
                for (int l = 0; l < 4; ++l) bits |= static_cast<uint32_t>(bsq_mlmd::lane16(w, l) < p.draw.th.sel) << (4 * q + l);
            }
        }
        selm = (bits >> r) & mapped;
        const int32_t s = static_cast<int32_t>(1 + c.i - i_first), k0 = static_cast<int32_t>(q0 - c.s);
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            const int64_t plain = (pl[k >> 2] >> (8 * (k & 3))) & 0xFFu;
            int64_t input = plain;
            if (p.in && ((selm >> k) & 1u))
                input = bsq_mlmd::replace(bsq_mlmd::replace_word(h, static_cast<uint64_t>(j0 + k)), p.draw.th, p.draw.mask_token, p.draw.nchars, plain);
            vin[k] = static_cast<TI>(input);
            sg[k] = s;
            ps[k] = k0 + k;
        }
    } else {
#pragma unroll
        for (uint32_t k = 0; k < 16; ++k) {
            const int64_t q = q0 + k;
            int64_t x = p.ids.pad_store;
            int32_t plain = p.ids.pad_store, s = 0, n = 0;
            if (k < n_el) {
                if (static_cast<uint64_t>(q) >= c.next) {
                    c = bsq_packd::cursor_at(p.offsets, p.starts, B, be, bsq_packd::find(p.starts, B, c.i, static_cast<uint64_t>(q)));
                    h = bsq_mlmd::row_key(p.draw.seed, static_cast<uint64_t>(p.draw.first_row + c.i));
                }
                if (col == P) col = 0;
                if (col == 0) i_first = c.i;
                if (c.i >= 0 && static_cast<uint64_t>(q) < c.e) {
                    const bsq_packd::MlmToken t = bsq_packd::run_mlm_token(p.ids, s_lut, p.chars, c.off, c.L, nchars, q - c.s, h, p.draw);
                    x = t.input;
                    plain = t.plain;
                    selm |= static_cast<uint32_t>(t.sel) << k;
                    s = static_cast<int32_t>(1 + c.i - i_first);
                    n = static_cast<int32_t>(q - c.s);
                }
                ++col;
            }
            pl[k >> 2] |= (static_cast<uint32_t>(plain) & 0xFFu) << (8 * (k & 3));
            vin[k] = static_cast<TI>(x), sg[k] = s, ps[k] = n;
        }
    }
    if (p.in) write_out(static_cast<TI *>(p.in), gid, q0, vin, n_el, valid, staged, s_out);
    if (p.lab) {
        const TL ign = static_cast<TL>(p.draw.ignore);
        TL vlab[16];
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            const int64_t plain = (pl[k >> 2] >> (8 * (k & 3))) & 0xFFu;
            vlab[k] = ((selm >> k) & 1u) ? static_cast<TL>(plain) : ign;
        }
        write_out(static_cast<TL *>(p.lab), gid, q0, vlab, n_el, valid, staged, s_out);
    }
    if (p.seg) write_out(p.seg, gid, q0, sg, n_el, valid, staged, s_out);
    if (p.pos) write_out(p.pos, gid, q0, ps, n_el, valid, staged, s_out);
}

// fold_table with the "mapped" flag: bit 7 of the entry of every mapped letter (ids are at most 127: the table of a bsq_desc is int8)
bool fold_table_flagged(const bsq_desc *d, uint32_t (&tab)[8]) {
    if (!fold_table(d, tab)) return false;
    for (int c = 0x40; c < 0x60; ++c)
        if (d->lut[c] >= 0) tab[(c & 31) >> 2] |= 0x80u << (8 * (c & 3));
    return true;
}
const char *form_name(bool perm) { return perm ? "k_pack_mlm_flat<perm>" : "k_pack_mlm_flat<lut>"; }

}  // namespace

extern "C" {

const char *bsq_pack_mlm_kernel_name(const bsq_desc *d, int64_t B, int64_t rows, int64_t P, bsq_dtype in_dtype) {
    static const int64_t one[2] = {0, 0};
    static const uint8_t none[1] = {0};
    if (bsq_pack_host::check_encode(d, none, one, B, one, rows, P, in_dtype, none) != BSQ_OK) return "";
    uint32_t tab[8];
    return form_name(fold_table(d, tab));
}

bsq_status bsq_pack_mlm_tokenize_device(const bsq_desc *d, const uint8_t *chars, const int64_t *offsets, int64_t B, const int64_t *starts,
                                        int64_t rows, int64_t P, const bsq_mlm *m, bsq_dtype in_dtype, void *inputs_or_null,
                                        bsq_dtype label_dtype, void *labels_or_null, int32_t *segment_ids_or_null,
                                        int32_t *position_ids_or_null, void *hip_stream) {
    PackMlmParams p;
    bsq_status st = bsq_pack_host::check_encode_mlm(d, chars, offsets, B, starts, rows, P, m, in_dtype, inputs_or_null, label_dtype,
                                                    labels_or_null, &p.draw);
    if (st != BSQ_OK || rows == 0 || B == 0) return st;
    const bool perm = fold_table_flagged(d, p.tab);
    std::memcpy(p.lut, d->lut, 256);
    p.chars = chars;
    p.offsets = offsets;
    p.starts = starts;
    p.in = inputs_or_null;
    p.lab = labels_or_null;
    p.seg = segment_ids_or_null;
    p.pos = position_ids_or_null;
    p.B = B;
    p.P = P;
    p.total = rows * P;
    p.npieces = (p.total + 15) / 16;
    p.div_P = div64_constants(static_cast<uint64_t>(P));
    p.ids = bsq_packd::make_ids(d);
    const unsigned grid = static_cast<unsigned>((p.npieces + kThreads - 1) / kThreads);
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    st = bsq_internal::with_value_type(in_dtype, [&](auto ti) {
        using TI = decltype(ti);
        return bsq_internal::with_value_type(label_dtype, [&](auto tl) {
            using TL = decltype(tl);
            if (perm) hipLaunchKernelGGL((k_pack_mlm_flat<TI, TL, true>), dim3(grid), dim3(kThreads), 0, s, p);
            else hipLaunchKernelGGL((k_pack_mlm_flat<TI, TL, false>), dim3(grid), dim3(kThreads), 0, s, p);
            return BSQ_OK;
        });
    });
    return st != BSQ_OK ? st : bsq_internal::check_launch(form_name(perm));
}

}  // extern "C"
