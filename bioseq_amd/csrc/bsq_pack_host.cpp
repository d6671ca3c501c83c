// Sequence packing, the CPU side (include/bsq.h, "sequence packing"): the argument rules every entry point of the family shares, the
// plan as the plain sequential loop (bsq_pack_plan_host), the device plan's rounds run on the CPU (bsq_pack_plan_parallel_host: the
// arithmetic of bsq_pack_dev.h in the order the kernels of bsq_pack.hip apply it) and the encode twins (bsq_pack_tokenize_host,
// bsq_pack_mlm_tokenize_host: the cursor and the id code of the kernels).  Plain C++: this file is part of the sanitizer build of the host code.
#include <cstdint>
#include <vector>

#include "bsq.h"
#include "bsq_internal.h"
#include "bsq_pack_dev.h"

namespace bsq_pack_host {

bsq_status check_plan(const int64_t *offsets, int64_t B, int64_t P, int32_t bos, int32_t eos, int32_t mode, int64_t max_rows,
                      const int64_t *starts, const int64_t *n_rows) {
    if (B < 0 || P <= 0) return bsq_internal::set_error(BSQ_ERR_INVALID_ARG, "B < 0 or padlen <= 0");
    if (P > kMaxP) return bsq_internal::set_error(BSQ_ERR_INVALID_ARG, "padlen > 2^30 is not supported");
    if (mode != BSQ_PACK_STREAM && mode != BSQ_PACK_NEXTFIT) return bsq_internal::set_error(BSQ_ERR_INVALID_ARG, "unknown packing mode");
    if ((bos != 0 && bos != 1) || (eos != 0 && eos != 1)) return bsq_internal::set_error(BSQ_ERR_INVALID_ARG, "bos and eos are 0 or 1");
    if (max_rows < 0 || max_rows > kMaxRows) return bsq_internal::set_error(BSQ_ERR_INVALID_ARG, "max_rows < 0 or > 2^31");
    if (!starts || !n_rows || (B > 0 && !offsets)) return bsq_internal::set_error(BSQ_ERR_INVALID_ARG, "offsets, starts or n_rows is null");
    if (B > bsq_packd::kMaxPlanB) return bsq_internal::set_error(BSQ_ERR_INVALID_ARG, "more than 2^31 - 2 sequences are not supported");
    return BSQ_OK;
}

bsq_status check_encode(const bsq_desc *d, const uint8_t *chars, const int64_t *offsets, int64_t B, const int64_t *starts, int64_t rows,
                        int64_t P, bsq_dtype t, const void *tokens) {
    if (!d || B < 0 || rows < 0 || P <= 0) return bsq_internal::set_error(BSQ_ERR_INVALID_ARG, "null tokenizer description, B < 0, rows < 0 or padlen <= 0");
    if (P > kMaxP || rows > kMaxRows) return bsq_internal::set_error(BSQ_ERR_INVALID_ARG, "padlen > 2^30 or rows > 2^31 is not supported");
    if (rows * P > kMaxPositions) return bsq_internal::set_error(BSQ_ERR_INVALID_ARG, "rows * padlen > 2^40 positions is not supported");
    if (t < BSQ_I8 || t > BSQ_F64) return bsq_internal::set_error(BSQ_ERR_DTYPE, "bad bsq_dtype");
    if (rows > 0 && (!tokens || !starts)) return bsq_internal::set_error(BSQ_ERR_INVALID_ARG, "tokens or starts is null");
    if (rows > 0 && B > 0 && (!offsets || !chars)) return bsq_internal::set_error(BSQ_ERR_INVALID_ARG, "chars or offsets is null");
    return BSQ_OK;
}

bsq_status check_encode_mlm(const bsq_desc *d, const uint8_t *chars, const int64_t *offsets, int64_t B, const int64_t *starts, int64_t rows,
                            int64_t P, const bsq_mlm *m, bsq_dtype in_dtype, const void *inputs, bsq_dtype label_dtype, const void *labels,
                            bsq_packd::MlmDraw *draw) {
    if (!inputs && !labels) return bsq_internal::set_error(BSQ_ERR_INVALID_ARG, "both outputs are null");
    if (label_dtype < BSQ_I8 || label_dtype > BSQ_F64) return bsq_internal::set_error(BSQ_ERR_DTYPE, "bad bsq_dtype");
    const bsq_status st = check_encode(d, chars, offsets, B, starts, rows, P, in_dtype, inputs ? inputs : labels);
    if (st != BSQ_OK) return st;
    const char *why = "";
    if (bsq_packd::make_draw(d, m, draw, &why) != BSQ_OK) return bsq_internal::set_error(BSQ_ERR_INVALID_ARG, why);
    return BSQ_OK;
}

// The rows = N rule on a finished plan: only the prefix of runs that end inside N rows stays, the others read -1; starts[B] <- the
// end of the last run that stayed.
static void apply_limit(const int64_t *offsets, int64_t B, int64_t P, int64_t be, int32_t nextfit, int64_t max_rows, int64_t *starts,
                        int64_t *n_placed) {
    const int64_t limit = max_rows > 0 ? max_rows * P : INT64_MAX;
    int64_t placed = 0, end = 0;
    for (int64_t i = 0; i < B; ++i) {
        const int64_t e = starts[i] + bsq_packd::taken(offsets, be, P, nextfit, i);
        if (placed == i && e <= limit) ++placed, end = e;
        else starts[i] = -1;
    }
    starts[B] = end;
    if (n_placed) *n_placed = placed;
}

}  // namespace bsq_pack_host

using namespace bsq_pack_host;

extern "C" {

bsq_status bsq_pack_plan_host(const int64_t *offsets, int64_t B, int64_t P, int32_t bos, int32_t eos, int32_t mode, int64_t max_rows,
                              int64_t *starts, int64_t *n_rows, int64_t *n_placed_or_null) {
    const bsq_status st = check_plan(offsets, B, P, bos, eos, mode, max_rows, starts, n_rows);
    if (st != BSQ_OK) return st;
    const int64_t be = bos + eos;
    int64_t row = 0, col = 0, S = 0;
    for (int64_t i = 0; i < B; ++i) {
        int64_t w = bsq_packd::width(offsets, i, be);
        if (w < 0) w = 0;
        if (mode == BSQ_PACK_NEXTFIT) {
            if (i > 0 && col + w > P) ++row, col = 0;  // it does not fit any more: it opens the next row
            starts[i] = row * P + col;
            col += w;  // (a run wider than P leaves no room behind it: the next run opens a row whatever its width)
        } else {
            starts[i] = S;
        }
        S += w;
    }
    *n_rows = B == 0 ? 0 : (mode == BSQ_PACK_NEXTFIT ? row + 1 : bsq_packd::stream_rows(S, P));
    apply_limit(offsets, B, P, be, mode == BSQ_PACK_NEXTFIT, max_rows, starts, n_placed_or_null);
    return BSQ_OK;
}

bsq_status bsq_pack_plan_parallel_host(const int64_t *offsets, int64_t B, int64_t P, int32_t bos, int32_t eos, int32_t mode, int64_t max_rows,
                                       int64_t *starts, int64_t *n_rows, int64_t *n_placed_or_null) {
    const bsq_status st = check_plan(offsets, B, P, bos, eos, mode, max_rows, starts, n_rows);
    if (st != BSQ_OK) return st;
    const int64_t be = bos + eos;
    const int32_t nextfit = mode == BSQ_PACK_NEXTFIT;
    std::vector<uint8_t> mark(static_cast<size_t>(B) + 1, 0);
    if (nextfit && B > 0) {
        std::vector<int32_t> a(static_cast<size_t>(B) + 1), b(static_cast<size_t>(B) + 1);
        for (int64_t i = 0; i < B; ++i) a[i] = static_cast<int32_t>(bsq_packd::next_head(offsets, B, be, P, i));
        a[B] = static_cast<int32_t>(B);
        mark[0] = 1;
        for (int32_t r = bsq_packd::jump_rounds(B); r > 0; --r) {
            for (int64_t i = B; i >= 0; --i) bsq_packd::jump_round(a.data(), b.data(), mark.data(), i);  // (any order will do: downwards here)
            a.swap(b);
        }
    }
    int64_t heads = 0, head = 0;
    for (int64_t i = 0; i < B; ++i) {
        if (mark[i]) ++heads, head = i;
        starts[i] = bsq_packd::place(offsets, be, P, nextfit, i, heads, head);
    }
    *n_rows = B == 0 ? 0 : (nextfit ? heads : bsq_packd::stream_rows(bsq_packd::prefix(offsets, B, be), P));
    apply_limit(offsets, B, P, be, nextfit, max_rows, starts, n_placed_or_null);
    return BSQ_OK;
}

bsq_status bsq_pack_tokenize_host(const bsq_desc *d, const uint8_t *chars, const int64_t *offsets, int64_t B, const int64_t *starts,
                                  int64_t rows, int64_t P, bsq_dtype t, void *tokens, int32_t *segment_ids_or_null,
                                  int32_t *position_ids_or_null) {
    const bsq_status st = check_encode(d, chars, offsets, B, starts, rows, P, t, tokens);
    if (st != BSQ_OK || rows == 0) return st;
    const bsq_packd::Ids ids = bsq_packd::make_ids(d);
    const int64_t be = ids.bos + ids.eos, total = rows * P, nchars = B > 0 ? offsets[B] : 0;
    return bsq_internal::with_value_type(t, [&](auto tag) {
        using T = decltype(tag);
        T *o = static_cast<T *>(tokens);
        bsq_packd::Cursor c = bsq_packd::cursor_at(offsets, starts, B, be, -1);
        int64_t i_first = -1;
        for (int64_t q = 0; q < total; ++q) {
            if (static_cast<uint64_t>(q) >= c.next) c = bsq_packd::cursor_at(offsets, starts, B, be, bsq_packd::find(starts, B, c.i, static_cast<uint64_t>(q)));
            if (q % P == 0) i_first = c.i;
            const bool in = c.i >= 0 && static_cast<uint64_t>(q) < c.e;
            o[q] = static_cast<T>(in ? bsq_packd::run_token(ids, d->lut, chars, c.off, c.L, nchars, q - c.s) : ids.pad_store);
            if (segment_ids_or_null) segment_ids_or_null[q] = in ? static_cast<int32_t>(1 + c.i - i_first) : 0;
            if (position_ids_or_null) position_ids_or_null[q] = in ? static_cast<int32_t>(q - c.s) : 0;
        }
        return BSQ_OK;
    });
}

bsq_status bsq_pack_mlm_tokenize_host(const bsq_desc *d, const uint8_t *chars, const int64_t *offsets, int64_t B, const int64_t *starts,
                                      int64_t rows, int64_t P, const bsq_mlm *m, bsq_dtype in_dtype, void *inputs_or_null,
                                      bsq_dtype label_dtype, void *labels_or_null, int32_t *segment_ids_or_null,
                                      int32_t *position_ids_or_null) {
    bsq_packd::MlmDraw draw;
    const bsq_status st = check_encode_mlm(d, chars, offsets, B, starts, rows, P, m, in_dtype, inputs_or_null, label_dtype, labels_or_null, &draw);
    if (st != BSQ_OK || rows == 0 || B == 0) return st;
    const bsq_packd::Ids ids = bsq_packd::make_ids(d);
    const int64_t be = ids.bos + ids.eos, total = rows * P, nchars = offsets[B];
    return bsq_internal::with_value_type(in_dtype, [&](auto ti) {
        using TI = decltype(ti);
        return bsq_internal::with_value_type(label_dtype, [&](auto tl) {
            using TL = decltype(tl);
            TI *in = static_cast<TI *>(inputs_or_null);
            TL *lab = static_cast<TL *>(labels_or_null);
            const TL ign = static_cast<TL>(draw.ignore);
            bsq_packd::Cursor c = bsq_packd::cursor_at(offsets, starts, B, be, -1);
            uint64_t h = 0;
            int64_t i_first = -1;
            for (int64_t q = 0; q < total; ++q) {
                if (static_cast<uint64_t>(q) >= c.next) {
                    c = bsq_packd::cursor_at(offsets, starts, B, be, bsq_packd::find(starts, B, c.i, static_cast<uint64_t>(q)));
                    h = bsq_mlmd::row_key(draw.seed, static_cast<uint64_t>(draw.first_row + c.i));
                }
                if (q % P == 0) i_first = c.i;
                const bool inside = c.i >= 0 && static_cast<uint64_t>(q) < c.e;
                bsq_packd::MlmToken t;
                t.input = t.plain = ids.pad_store, t.sel = false;
                if (inside) t = bsq_packd::run_mlm_token(ids, d->lut, chars, c.off, c.L, nchars, q - c.s, h, draw);
                if (in) in[q] = static_cast<TI>(t.input);
                if (lab) lab[q] = t.sel ? static_cast<TL>(static_cast<int64_t>(t.plain)) : ign;
                if (segment_ids_or_null) segment_ids_or_null[q] = inside ? static_cast<int32_t>(1 + c.i - i_first) : 0;
                if (position_ids_or_null) position_ids_or_null[q] = inside ? static_cast<int32_t>(q - c.s) : 0;
            }
            return BSQ_OK;
        });
    });
}

}  // extern "C"
