// BPE training, the CPU side (include/bsq.h, "BPE training"): the sizes of the workspace, the host-only kernel name, and the twin
// bsq_bpe_train_host -- one thread, one sequential walk over the symbols per merge: the previous pair replaced left to right, every pair
// counted without overlap into an open-addressing table that is cleared through the list of its used slots.  It shares the limits, the
// argument rules and the record of bsq_bpe_train_dev.h with the kernels; the walk itself is its own text.  Plain C++: no HIP headers.
#include <cstdint>
#include <vector>

#include "bsq.h"
#include "bsq_bpe_train_dev.h"

namespace bsq_internal {
bsq_status set_error(bsq_status st, const char *msg);  // (bsq_internal.h, which includes the HIP runtime's header)
}

namespace {

using namespace bsq_bpetd;

struct PairTable {
    std::vector<uint32_t> key1, count, used;
    uint32_t lg = 0;
    void reserve_for(uint32_t want_lg) {
        if (want_lg <= lg) return;
        lg = want_lg;
        key1.assign(size_t(1) << lg, 0u);
        count.assign(size_t(1) << lg, 0u);
    }
    void add(uint32_t key) {
        const uint32_t mask = (1u << lg) - 1;
        uint32_t slot = slot_of(key, lg);
        while (key1[slot] != 0 && key1[slot] != key + 1) slot = (slot + 1) & mask;  // (at most half the slots are ever taken)
        if (key1[slot] == 0) {
            key1[slot] = key + 1;
            used.push_back(slot);
        }
        ++count[slot];
    }
    uint64_t best_and_clear() {
        uint64_t best = 0;
        for (const uint32_t slot : used) {
            const uint64_t rec = record_of(key1[slot] - 1, count[slot]);
            best = rec > best ? rec : best;
            key1[slot] = 0;
            count[slot] = 0;
        }
        used.clear();
        return best;
    }
};

}  // namespace

extern "C" {

int64_t bsq_bpe_train_workspace_bytes(const bsq_desc *d, int64_t B, int64_t total_chars, const bsq_bpe_train *t) {
    Plan pl;
    const char *why = "";
    const bsq_status st = make_plan(d, B, total_chars, t, &pl, &why);
    return st != BSQ_OK ? -static_cast<int64_t>(bsq_internal::set_error(st, why)) : pl.bytes;
}

int64_t bsq_bpe_train_table_slots(const bsq_desc *d, int64_t B, int64_t total_chars, const bsq_bpe_train *t) {
    Plan pl;
    const char *why = "";
    const bsq_status st = make_plan(d, B, total_chars, t, &pl, &why);
    return st != BSQ_OK ? -static_cast<int64_t>(bsq_internal::set_error(st, why)) : (int64_t(1) << pl.slots_lg);
}

int32_t bsq_bpe_train_lds_slots(void) { return kLdsSlots; }

const char *bsq_bpe_train_kernel_name(const bsq_bpe_train *t) { return kernel_name(form_of(t)); }

bsq_status bsq_bpe_train_host(const bsq_desc *d, const uint8_t *chars, const int64_t *offsets, int64_t B, int64_t total_chars,
                              const bsq_bpe_train *t, int32_t *merges, int64_t *counts, int64_t *n_made, int64_t *skipped_rows) {
    Plan pl;
    const char *why = "";
    const bsq_status st = make_plan(d, B, total_chars, t, &pl, &why);
    if (st != BSQ_OK) return bsq_internal::set_error(st, why);
    if (!n_made || !skipped_rows || (pl.n_merges > 0 && (!merges || !counts)) || (B > 0 && (!chars || !offsets)))
        return bsq_internal::set_error(BSQ_ERR_INVALID_ARG, "chars, offsets, merges, counts, n_made or skipped_rows is null");
    // the rows that take part, their symbols back to back
    std::vector<uint16_t> sym;
    std::vector<int32_t> len(static_cast<size_t>(B), 0);
    int64_t skipped = 0, live = 0;
    for (int64_t i = 0; i < B; ++i) {
        const int64_t start = offsets[i];
        int64_t L = offsets[i + 1] - start;
        L = L < 0 ? 0 : L;
        if (L > pl.max_chars) {
            ++skipped;
            continue;
        }
        if (start < 0 || start > total_chars || L > total_chars - start) continue;  // (malformed offsets: an empty row)
        len[static_cast<size_t>(i)] = static_cast<int32_t>(L);
        live += L;
    }
    sym.reserve(static_cast<size_t>(live));
    for (int64_t i = 0; i < B; ++i)
        for (int32_t q = 0; q < len[static_cast<size_t>(i)]; ++q) {
            const int32_t id = d->lut[chars[offsets[i] + q]];
            sym.push_back(static_cast<uint16_t>(id < 0 ? kBarrier : static_cast<uint32_t>(id)));
        }
    PairTable tab;
    int64_t made = 0;
    uint32_t ml = 0, mr = 0;
    while (made < pl.n_merges) {
        const uint32_t want = need_log2(pl.C, made, live);
        tab.reserve_for(want < 31 ? want : 31);  // (fewer than 2^31 pairs exist: the table never fills)
        const bool apply = made > 0;
        const uint16_t new_id = static_cast<uint16_t>(pl.C + made - 1);
        size_t src = 0, dst = 0;
        for (int64_t i = 0; i < B; ++i) {
            const int32_t n = len[static_cast<size_t>(i)];
            uint16_t *row = sym.data() + dst;  // (rows stay back to back: dst <= src)
            int32_t j = 0;
            if (apply) {
                for (int32_t q = 0; q < n; ++j) {
                    if (q + 1 < n && sym[src + q] == ml && sym[src + q + 1] == mr) {
                        row[j] = new_id;
                        q += 2;
                    } else {
                        row[j] = sym[src + q];
                        q += 1;
                    }
                }
            } else {
                for (; j < n; ++j) row[j] = sym[src + j];
            }
            src += static_cast<size_t>(n);
            dst += static_cast<size_t>(j);
            len[static_cast<size_t>(i)] = j;
            bool prev_taken = false;  // the position in front is a pair of equal symbols that counted
            for (int32_t q = 0; q + 1 < j; ++q) {
                const uint32_t a = row[q], b = row[q + 1];
                if (a == kBarrier || b == kBarrier) {
                    prev_taken = false;
                    continue;
                }
                const bool counts_here = a != b || !prev_taken;
                prev_taken = a == b && counts_here;
                if (counts_here) tab.add((a << 16) | b);
            }
        }
        sym.resize(dst);
        const uint64_t rec = tab.best_and_clear();
        if (record_count(rec) < 2) break;
        ml = record_key(rec) >> 16;
        mr = record_key(rec) & 0xFFFFu;
        merges[2 * made] = static_cast<int32_t>(ml);
        merges[2 * made + 1] = static_cast<int32_t>(mr);
        counts[made] = record_count(rec);
        ++made;
    }
    *n_made = made;
    *skipped_rows = skipped;
    return BSQ_OK;
}

}  // extern "C"
