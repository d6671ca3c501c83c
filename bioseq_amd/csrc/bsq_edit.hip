// Edit distance of row pairs on the device (include/bsq.h, "edit distance of row pairs"): k_edit_pairs<G> on the pair walk of
// bsq_pair_walk.h with 64 pattern rows (one block) a lane.
//
// Lane b of the pair's group owns block b: its vertical deltas Pv, Mv in registers and its column of the pair's match table in LDS --
// tab[class][lane], one 64-bit word per class with bit i set where pattern character 64 b + i has that class.  A lane reads and writes
// its own column only (plain read-modify-write, no atomic, no barrier), and consecutive lanes read consecutive words.
// At step t lane b takes column t - b through the block step of bsq_edit_dev.h.  What a lane needs for a column -- its class and the
// horizontal delta that left the block below -- is one 32-bit value that moves up one lane per step, and it shares its ds_bpermute with
// the tile: a lane offers (tile class << 16) | (class, delta) and reads either its lower neighbour or, as lane 0, the tile's lane.
// The update of a lane outside its columns is a select, so no lane is switched off around the cross-lane read.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "bsq.h"
#include "bsq_device.h"
#include "bsq_edit_dev.h"
#include "bsq_internal.h"
#include "bsq_pair_walk.h"
#include "bsq_row_table.h"

namespace {

using bsq_dev::kThreads;
using bsq_pairs::Kind;

struct EditParams {
    const uint8_t *chars_a, *chars_b;
    const int64_t *offsets_a, *offsets_b;
    const int64_t *row, *col;
    int32_t *dist;
    int64_t Ba, Bb, n_pairs;
    int32_t max_len, nchars;
    int8_t lut[256];
};

template <int G>
__global__ __launch_bounds__(kThreads) void k_edit_pairs(const EditParams p) {
    extern __shared__ __align__(16) uint64_t s_dyn[];  // four waves' tables of classes x 64 words, then the 256 classes of the bytes
    const int32_t C = p.nchars + 1;
    uint8_t *s_cls = reinterpret_cast<uint8_t *>(s_dyn + static_cast<size_t>(kThreads) * C);
    bsq_pairs::stage_classes(p, s_cls);
    __syncthreads();
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, b = lane & (G - 1), base = lane & ~(G - 1);
    uint64_t *tab = s_dyn + static_cast<size_t>(wave) * 64 * C + lane;  // tab[c * 64]: this lane's word of class c
    const int64_t k = bsq_pairs::pair_index<G>();

    // the pair of this lane's group: its pattern (m characters, nb blocks) and text (n characters; 0 where nothing is walked)
    bsq_pairs::Pair pair;
    const Kind kind = bsq_pairs::resolve(p, k, bsq_editd::kMaxLong, pair);
    const bool live = kind == Kind::live;
    if (kind != Kind::none && !live && b == 0)
        p.dist[k] = kind == Kind::bad_index ? BSQ_EDIT_BAD_INDEX : (kind == Kind::too_long ? BSQ_EDIT_TOO_LONG : static_cast<int32_t>(pair.n));
    const uint32_t m = pair.m, n = live ? pair.n : 0u, nb = (m + 63) >> 6;
    const uint32_t wave_steps = bsq_pairs::wave_max(live ? n + nb - 1 : 0u);
    if (wave_steps == 0) return;  // (no workgroup barrier follows)

    // this lane's column of the table: the classes of pattern characters 64 b .. 64 b + 63
    for (int32_t c = 0; c < C; ++c) tab[c * 64] = 0;
    if (live && static_cast<uint32_t>(b) < nb) {
        const int32_t mine = static_cast<int32_t>(m) - 64 * b < 64 ? static_cast<int32_t>(m) - 64 * b : 64;
        for (int q = 0; q < 4; ++q) {
            if (16 * q >= mine) break;
            uint32_t w[4];
            bsq_rowtab::load16(pair.pat, pair.pat_at + 64 * b + 16 * q, pair.pat_total, mine - 16 * q, w);
#pragma unroll
            for (int c = 0; c < 16; ++c)
                if (16 * q + c < mine) tab[s_cls[(w[c >> 2] >> (8 * (c & 3))) & 0xFFu] * 64] |= uint64_t(1) << (16 * q + c);
        }
    }

    const uint32_t top = static_cast<uint32_t>(b) + 1 == nb ? (m - 1) & 63u : 63u;
    const int src = b == 0 ? base : lane - 1;  // (lane 0 of a group adds t % G)
    uint64_t pv = ~uint64_t(0), mv = 0;
    int32_t score = static_cast<int32_t>(m);
    // the text tile of bsq_pair_walk.h, written out: with bsq_pairs::TextTile the step's class decode compiled to one instruction more
    // and whole calls ran 1.5 - 1.8 % slower (profiles/r28/pair_walk_lab.txt)
    const uint8_t *text = pair.text;
    auto fetch = [&](uint32_t at) -> uint32_t { return at < n ? text[at] : 0u; };  // (n == 0 for a lane without a text)
    uint32_t ahead = fetch(b), tile = 0, out = 0;
    for (uint32_t t = 0; t < wave_steps; ++t) {
        if ((t & (G - 1)) == 0) {  // (uniform)
            tile = s_cls[ahead];
            ahead = fetch(t + G + b);
        }
        const uint32_t got = __shfl((tile << 16) | out, b == 0 ? src + static_cast<int>(t & (G - 1)) : src);
        const uint32_t cls = b == 0 ? got >> 16 : (got >> 2) & 0x3FFFu;
        const int32_t hin = b == 0 ? 1 : static_cast<int32_t>(got & 3u) - 1;
        uint64_t npv = pv, nmv = mv;
        const int32_t hout = bsq_editd::block_step(npv, nmv, tab[cls * 64], hin, top);
        const bool on = t >= static_cast<uint32_t>(b) && t - b < n && static_cast<uint32_t>(b) < nb;
        pv = on ? npv : pv;
        mv = on ? nmv : mv;
        score += on ? hout : 0;
        out = (cls << 2) | static_cast<uint32_t>(hout + 1);
    }
    if (live && static_cast<uint32_t>(b) + 1 == nb) p.dist[k] = score;
}

}  // namespace

extern "C" {

bsq_status bsq_edit_pairs_device(const bsq_desc *d, const uint8_t *chars_a, const int64_t *offsets_a, int64_t Ba, const uint8_t *chars_b,
                                 const int64_t *offsets_b, int64_t Bb, const int64_t *row, const int64_t *col, int64_t n_pairs, const bsq_edit *e,
                                 int32_t *dist, void *hip_stream) {
    const char *why = "";
    int32_t lanes = 0;
    const bsq_status st = bsq_editd::check(d, chars_a, offsets_a, Ba, chars_b, offsets_b, Bb, row, col, n_pairs, e, dist, &lanes, &why);
    if (st != BSQ_OK) return bsq_internal::set_error(st, why);
    if (n_pairs == 0) return BSQ_OK;
    EditParams p;
    bsq_pairs::fill(p, d, chars_a, offsets_a, Ba, chars_b, offsets_b, Bb, row, col, n_pairs, e ? e->max_len : bsq_editd::kMaxLen);
    p.dist = dist;
    const size_t lds = static_cast<size_t>(kThreads) * (p.nchars + 1) * sizeof(uint64_t) + 256;
    bsq_pairs::for_lanes(lanes, [&](auto g) {
        constexpr int G = decltype(g)::value;
        bsq_pairs::launch<G>(k_edit_pairs<G>, p, lds, static_cast<hipStream_t>(hip_stream));
    });
    return bsq_internal::check_launch(bsq_editd::kernel_name(lanes));
}

}  // extern "C"
