// len_tables.cpp — see len_tables.hpp
#include "len_tables.hpp"

#include <algorithm>
#include <numeric>
#include <vector>

namespace stn {

LenTables len_tables_layout(int B, int ve_rows, bool with_pairs, int vo_form) {
    LenTables t;
    int at = t.llen + B;
    if (ve_rows > 0) {
        t.ve_off = at; at += B + 1;
        t.ve_row_b = at; at += ve_rows;
    }
    if (with_pairs) { t.pairs = at; at += B + 2; }
    if (vo_form != LEN_VO_NONE) {
        t.vo_n = at; at += B;
        t.vo_valid = at; at += B;
        t.vo_off = at; at += B + 1;
    }
    t.total = (at + 3) & ~3;  // whole 16-byte units
    return t;
}

void len_tables_build(const LenTables& t, const int* llen, int B, int ve_rows, bool with_pairs, int vo_form, int ccf, int T, int rf, int32_t* out) {
    std::fill(out + t.llen, out + t.total, 0);
    std::copy(llen, llen + B, out + t.llen);
    if (t.ve_off >= 0) {
        int32_t* off = out + t.ve_off;
        int32_t* row_b = out + t.ve_row_b;
        off[0] = 0;
        for (int b = 0; b < B; ++b) {
            off[b + 1] = off[b] + llen[b];
            std::fill(row_b + off[b], row_b + std::min(off[b + 1], ve_rows), b);
        }
        // (dead rows behind the last utterance stay 0: sequence 0, so that per-row lookups stay in range)
    }
    if (with_pairs && t.pairs >= 0) {
        // ascending by length, ties by index (the kernel's rank); the k-th longest with the k-th shortest, -1 for the odd one out
        std::vector<int> sorted(B);
        std::iota(sorted.begin(), sorted.end(), 0);
        std::stable_sort(sorted.begin(), sorted.end(), [&](int x, int y) { return llen[x] < llen[y]; });
        int32_t* pairs = out + t.pairs;
        const int G = (B + 1) / 2;
        for (int i = 0; i < G; ++i) {
            pairs[2 * i] = sorted[B - 1 - i];
            pairs[2 * i + 1] = B - 1 - i > i ? sorted[i] : -1;
        }
    }
    if (t.vo_n >= 0) {
        int32_t* n = out + t.vo_n;
        int32_t* valid = out + t.vo_valid;
        int32_t* off = out + t.vo_off;
        off[0] = 0;
        for (int b = 0; b < B; ++b) {
            const int l6 = llen[b] * ccf;
            if (vo_form == LEN_VO_SCALED) {
                n[b] = valid[b] = l6;
            } else if (vo_form == LEN_VO_TAIL) {
                n[b] = valid[b] = l6 + rf < T ? l6 + rf : T;
            } else {
                const bool trim = l6 + 2 * rf <= T;
                n[b] = trim ? l6 + 2 * rf : T;
                valid[b] = trim ? l6 + rf : T;
            }
            off[b + 1] = off[b] + n[b];
        }
    }
}

}  // namespace stn
