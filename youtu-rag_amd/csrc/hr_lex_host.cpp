// hr_lex_host.cpp -- host half of the lexical (BM25) index: the row packing (hr_lex_pack) and the fp64 tables of
// the scoring definition (DESIGN.md "Keyword search").  Pure host code, no device call.  The BM25 expressions are
// part of a bit-exact contract with the Python reference (tests/lex_ref.py): every operation is rounded once, in
// the written order, so this file is compiled without fast-math and with contraction off (csrc/Makefile).
#include <algorithm>
#include <cmath>
#include <vector>

#include "hr_lex.hpp"

namespace hrlex {

double bm25_A(int64_t n_live, int64_t df, double k1) {
    const double num = ((double)n_live - (double)df) + 0.5;  // N - df is exact: both are small integers
    const double den = (double)df + 0.5;
    const double idf = std::log(1.0 + num / den);
    return idf * (k1 + 1.0);
}

void bm25_K_table(double k1, double b, double avgdl, int max_dl, double* out) {
    const double one_minus_b = 1.0 - b;
    for (int dl = 0; dl <= max_dl; ++dl) out[dl] = k1 * (one_minus_b + b * ((double)dl / avgdl));
}

}  // namespace hrlex

extern "C" int hr_lex_pack(const uint32_t* tokens, const int64_t* offsets, int64_t n, uint32_t* entries_out,
                           int64_t entries_cap, int64_t* row_off_out, uint16_t* dl_out) {
    using namespace hrlex;
    if (n < 0 || !row_off_out || entries_cap < 0 || (n > 0 && (!offsets || !dl_out)))
        return set_err(HR_E_INVALID, "hr_lex_pack: bad arguments");
    std::vector<uint32_t> row;
    int64_t w = 0;
    row_off_out[0] = 0;
    for (int64_t i = 0; i < n; ++i) {
        const int64_t a = offsets[i], b = offsets[i + 1];
        if (a < 0 || b < a || (b > a && !tokens)) return set_err(HR_E_INVALID, "hr_lex_pack: bad offsets");
        row.assign(tokens + a, tokens + b);
        for (uint32_t t : row)
            if (t >= kTermSpan) return set_err(HR_E_INVALID, "hr_lex_pack: token id beyond HR_LEX_TERM_BITS");
        std::sort(row.begin(), row.end());
        for (size_t p = 0; p < row.size();) {
            size_t q = p + 1;
            while (q < row.size() && row[q] == row[p]) ++q;
            if (w >= entries_cap) return set_err(HR_E_INVALID, "hr_lex_pack: entries_out is full");
            entries_out[w++] = (row[p] << kTfBits) | (uint32_t)std::min<size_t>(q - p, kTfMax);
            p = q;
        }
        row_off_out[i + 1] = w;
        dl_out[i] = (uint16_t)std::min<int64_t>(b - a, kDlMax);
    }
    return HR_OK;
}
