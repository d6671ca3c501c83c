// A FRAGMENT of a function body, not a header: the statements of the two-pass one-hot's expansion kernel for one-byte elements in short
// rows (no include guard: it is meant to be included twice; the design notes are in bsq_onehot.hip, above expand_rows1_body).
// Expects in scope: the template parameters NT, NR, NIB;  uint32_t blk, the block of one batch's grid;  p, an EParams;  and what
// bsq_onehot.hip declares before it (ChunkCoord, chunk_coord, bsq_tiles.h).
// Included by k_expand_rows1 (blk = blockIdx.x) and by expand_rows1_body, which k_expand_rows1_multi calls.
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int wave_s = __builtin_amdgcn_readfirstlane(wave);
    const int64_t slot = static_cast<int64_t>(blk >> 3) * 4 + wave_s;
    const int64_t k = static_cast<int64_t>(blk & 7u) + 8 * slot;
    if (k >= p.nchunks) return;
    const int32_t rb = p.C;  // bytes per row (one-byte elements)
    const ChunkCoord cc = chunk_coord<0>(p, k, rb);
    if (!cc.live) return;
    const int32_t len = cc.len, skip = cc.skip;
    const int32_t nr_s = __builtin_amdgcn_readfirstlane(cc.nr);
    // NIB: the byte that holds the chunk's first id, and that id's half (Bp is even: the parity of t_lo * Bp + b_lo is b_lo's)
    const uint8_t *tok = NIB ? p.tok + ((cc.t_lo * p.Bp + cc.b_lo) >> 1) : p.tok + cc.t_lo * p.Bp + cc.b_lo;
    const uint32_t par0 = NIB ? static_cast<uint32_t>(cc.b_lo & 1) : 0u;
    constexpr uint32_t kNo = NIB ? 0xFu : kNone;  // "no one"
    const int64_t wrap_at = p.B - cc.b_lo;  // rows i >= wrap_at belong to position t_lo + 1 (or later)
    const bool wraps = p.Bp != p.B && wrap_at < nr_s;  // (wave-uniform) the chunk runs over the end of a position row of a PADDED id matrix
    uint8_t *g = p.out + cc.lo + cc.t_lo * p.row_gap;
    const uint32_t one = static_cast<uint32_t>(p.one_bits) & 0xFFu;
    // the id of row i of the chunk (rows behind wrap_at lie in later position rows of the matrix, Bp - B ids further each)
    auto id_of = [&](uint32_t i) -> uint32_t {
        int64_t at = i;
        if (static_cast<int64_t>(i) >= wrap_at) at += ((static_cast<int64_t>(i) - wrap_at) / p.B + 1) * (p.Bp - p.B);
        if constexpr (NIB) {
            at += par0;
            return (static_cast<uint32_t>(tok[at >> 1]) >> ((static_cast<uint32_t>(at) & 1u) << 2)) & 0xFu;
        } else {
            return static_cast<uint32_t>(tok[at]);
        }
    };
    constexpr int IDB = NIB ? 4 : 8;  // bits per id in a lane's window
    if (len == kChunk && (reinterpret_cast<uintptr_t>(g) & 15) == 0 && nr_s >= 8) {
        uint64_t ids[4];
        uint32_t ph[4];
        if (!wraps && NIB) {
            typedef uint32_t u32u __attribute__((aligned(1)));
            uint32_t w[4], sh[4];
            const uint32_t lb = (par0 + static_cast<uint32_t>(nr_s) - 1u) >> 1;  // the last byte of ids this chunk owns (>= 3: nr_s >= 8)
#pragma unroll
            for (int u = 0; u < 4; ++u) {  // the four id windows of the lane in flight together: NR <= 6 nibbles + a parity fit four bytes
                const uint32_t o = static_cast<uint32_t>(skip) + static_cast<uint32_t>(u * 1024 + lane * 16);
                const uint32_t q = fast_div(o, p.rb_magic, p.rb_shift, p.rb_pow2);
                ph[u] = o - q * static_cast<uint32_t>(rb);
                const uint32_t n0 = q + par0, bo = n0 >> 1;
                const uint32_t off = bo + 3u <= lb ? bo : lb - 3u;  // pulled back to END at the chunk's last id byte (rows < nr_s lie in bo ... lb)
                sh[u] = (bo - off) * 8u + ((n0 & 1u) << 2);
                w[u] = *reinterpret_cast<const u32u *>(tok + off);
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) ids[u] = w[u] >> sh[u];
        } else if (!wraps) {
            typedef uint32_t u32x2u __attribute__((ext_vector_type(2), aligned(1)));
            u32x2u w[4];
            uint32_t sh[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {  // the four id windows of the lane in flight together
                const uint32_t o = static_cast<uint32_t>(skip) + static_cast<uint32_t>(u * 1024 + lane * 16);
                const uint32_t q = fast_div(o, p.rb_magic, p.rb_shift, p.rb_pow2);
                ph[u] = o - q * static_cast<uint32_t>(rb);
                // the last lanes' windows are pulled back to END at the chunk's last row: never a byte beyond the ids this chunk owns
                const uint32_t off = q + 8u <= static_cast<uint32_t>(nr_s) ? q : static_cast<uint32_t>(nr_s) - 8u;
                sh[u] = (q - off) * 8u;
                w[u] = *reinterpret_cast<const u32x2u *>(tok + off);
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) ids[u] = ((static_cast<uint64_t>(w[u].y) << 32) | w[u].x) >> sh[u];
        } else {  // one chunk per position row: the NR ids of a window one by one, across the padding (all 4 NR byte loads in flight together)
            uint32_t b[4][NR];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const uint32_t o = static_cast<uint32_t>(skip) + static_cast<uint32_t>(u * 1024 + lane * 16);
                const uint32_t q = fast_div(o, p.rb_magic, p.rb_shift, p.rb_pow2);
                ph[u] = o - q * static_cast<uint32_t>(rb);
#pragma unroll
                for (int j = 0; j < NR; ++j) b[u][j] = q + j < static_cast<uint32_t>(nr_s) ? id_of(q + j) : kNo;
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                ids[u] = 0;
#pragma unroll
                for (int j = 0; j < NR; ++j) ids[u] |= static_cast<uint64_t>(b[u][j]) << (IDB * j);
            }
        }
        const uint32_t cmask = (1u << rb) - 1u;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            uint32_t bits = 0;
#pragma unroll
            for (int j = 0; j < NR; ++j) {
                const uint32_t id = static_cast<uint32_t>(ids[u] >> (IDB * j)) & (NIB ? 0xFu : 0xFFu);
                const uint32_t m = (1u << (id & 31u)) & cmask;  // id 255 (no one) -> bit 31 -> 0; nibble 15 -> bit 15 -> 0 (rows of <= 15 bytes)
                const int32_t at = j * rb;                      // wave-uniform; strings that start at bit >= 32 lie beyond the lane's bits
                if (at < 32) bits |= m << at;
            }
            bits >>= ph[u];
            uint4 o;
            o.x = (((bits >> 0) & 15u) * 0x204081u) & 0x01010101u;
            o.y = (((bits >> 4) & 15u) * 0x204081u) & 0x01010101u;
            o.z = (((bits >> 8) & 15u) * 0x204081u) & 0x01010101u;
            o.w = (((bits >> 12) & 15u) * 0x204081u) & 0x01010101u;
            if (one != 1u) {
                o.x *= one;
                o.y *= one;
                o.z *= one;
                o.w *= one;
            }
            store16<NT>(g + u * 1024 + lane * 16, o);
        }
        return;
    }
    // the clipped first / last chunk of the tensor, a result that is not 16-byte aligned: byte by byte, eight independent ids at a time
    for (int32_t o0 = lane; o0 < len; o0 += 64 * 8) {
        uint32_t idv[8], cv[8];
#pragma unroll
        for (int m = 0; m < 8; ++m) {
            const int32_t o = o0 + 64 * m;
            const uint32_t a = static_cast<uint32_t>(o + skip);
            const uint32_t i = fast_div(a, p.rb_magic, p.rb_shift, p.rb_pow2);
            cv[m] = a - i * static_cast<uint32_t>(rb);
            idv[m] = o < len ? id_of(i) : kNo;
        }
#pragma unroll
        for (int m = 0; m < 8; ++m)
            if (o0 + 64 * m < len) g[o0 + 64 * m] = idv[m] == cv[m] ? static_cast<uint8_t>(one) : uint8_t(0);
    }
