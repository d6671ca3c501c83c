// A FRAGMENT of a function body, not a header: the statements of the two-pass one-hot's expansion kernel (no include guard: it is meant to
// be included twice; the design notes are in bsq_onehot.hip, above expand_chunks_body).
// Expects in scope: the template parameters ST, NT, MATH, GATE, NIB;  uint32_t blk, the block of one batch's grid;  p, an EParams;  and
// what bsq_onehot.hip declares before it (ChunkCoord, chunk_coord, bsq_tiles.h).
// Included by k_expand_chunks (blk = blockIdx.x) and by expand_chunks_body, which k_expand_chunks_multi calls.
    constexpr int PIECE = kChunk;             // bytes per wave
    constexpr int NS = PIECE / 1024;          // 16-byte stores per lane
    __shared__ __align__(16) uint8_t s_img[4][PIECE];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    uint8_t *img = s_img[wave];
#pragma unroll
    for (int u = 0; u < NS; ++u) *reinterpret_cast<uint4 *>(img + u * 1024 + lane * 16) = uint4{0, 0, 0, 0};

    // chunk of this wave: class = blockIdx % 8 (pinned to the XCD the block lands on).  The wave index goes through
    // readfirstlane so that the chunk arithmetic below is scalar-ALU work.
    const int wave_s = MATH == 1 ? __builtin_amdgcn_readfirstlane(wave) : wave;
    int64_t group = static_cast<int64_t>(blk >> 3);
    int32_t cls = static_cast<int32_t>(blk & 7u);
    const int64_t slot = group * 4 + wave_s;
    const int64_t k = static_cast<int64_t>(cls) + 8 * slot;
    if (k >= p.nchunks) return;
    uint32_t gate = 0;
    if constexpr (GATE) gate = __hip_atomic_load(reinterpret_cast<const uint32_t *>(p.tok) + (blk & 63u), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const int32_t rowbytes = p.C * static_cast<int32_t>(sizeof(ST));
    const ST one = static_cast<ST>(p.one_bits);
    const ChunkCoord cc = chunk_coord<MATH>(p, k, rowbytes);
    if (!cc.live) return;
    const int64_t lo = cc.lo, b_lo = cc.b_lo, t_lo = cc.t_lo;
    const int32_t len = cc.len, skip = cc.skip, nr = cc.nr;
    // NIB: the byte that holds the chunk's first id, and that id's half (Bp is even: the parity of t_lo * Bp + b_lo is b_lo's)
    const uint8_t *tok = NIB ? p.tok + ((t_lo * p.Bp + b_lo) >> 1) : p.tok + t_lo * p.Bp + b_lo;
    const int32_t par0 = NIB ? static_cast<int32_t>(b_lo & 1) : 0;
    if constexpr (GATE) tok += (gate == 0xFEFEFEFDu && p.nchunks < 0) ? 1 : 0;  // never taken: the token loads wait for the gate load
    constexpr uint32_t nmask = NIB ? 0xFu : kNone;  // "no one"
    const int64_t wrap_at = p.B - b_lo;  // rows i >= wrap_at belong to position t_lo + 1 (or later)
    // scatter: row r_lo + i has its one at image byte i*rowbytes - skip + tok*sizeof(ST).
    // NS (1..4) coalesced token loads in flight per step, straight-line per NS: the number of 64-row slots a
    // step needs and the (rare) row-wrap case are wave-uniform, so they are scalar branches.
    const int32_t nr_s = __builtin_amdgcn_readfirstlane(nr);
    const bool wraps = wrap_at < nr_s;  // the piece runs over the end of position t_lo's rows
    auto step = [&](auto ns_tag, int32_t i0) {
        constexpr int NS = decltype(ns_tag)::value;
        uint32_t tk[NS];
#pragma unroll
        for (int q = 0; q < NS; ++q) {
            const int32_t i = i0 + 64 * q + lane;
            int64_t a = i;
            if (wraps && i >= wrap_at) {
                const int64_t w = (i - wrap_at) / p.B + 1;
                a = i + w * (p.Bp - p.B);
            }
            if constexpr (NIB) {
                const int64_t ia = a + par0;
                tk[q] = i < nr_s ? (static_cast<uint32_t>(tok[ia >> 1]) >> ((static_cast<uint32_t>(ia) & 1u) << 2)) & 0xFu : nmask;
            } else {
                tk[q] = i < nr_s ? static_cast<uint32_t>(tok[a]) : kNone;
            }
        }
#pragma unroll
        for (int q = 0; q < NS; ++q) {
            const int32_t i = i0 + 64 * q + lane;
            const int32_t pos = i * rowbytes - skip + static_cast<int32_t>(tk[q]) * static_cast<int32_t>(sizeof(ST));
            if (tk[q] != nmask && pos >= 0 && pos < len) *reinterpret_cast<ST *>(img + pos) = one;
        }
    };
    for (int32_t i0 = 0; i0 < nr_s; i0 += 256) {
        const int32_t left = p.force4 ? 256 : nr_s - i0;
        if (left > 192) step(std::integral_constant<int, 4>{}, i0);
        else if (left > 128) step(std::integral_constant<int, 3>{}, i0);
        else if (left > 64) step(std::integral_constant<int, 2>{}, i0);
        else step(std::integral_constant<int, 1>{}, i0);
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    uint8_t *g = p.out + lo + t_lo * p.row_gap;
    if (len == PIECE && (reinterpret_cast<uintptr_t>(g) & 15) == 0) {
        uint4 v[NS];
#pragma unroll
        for (int u = 0; u < NS; ++u) v[u] = *reinterpret_cast<const uint4 *>(img + u * 1024 + lane * 16);
#pragma unroll
        for (int u = 0; u < NS; ++u) store16<NT>(g + u * 1024 + lane * 16, v[u]);
    } else {  // clipped first / last piece of the tensor
        for (int32_t o = lane * static_cast<int32_t>(sizeof(ST)); o < len; o += 64 * static_cast<int32_t>(sizeof(ST)))
            *reinterpret_cast<ST *>(g + o) = *reinterpret_cast<const ST *>(img + o);
    }
