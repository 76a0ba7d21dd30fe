// hr_lex.hpp -- internals shared by the lexical (BM25) index's two translation units: hr_lex_host.cpp (pure host:
// row packing and the fp64 scoring tables, compiled without contraction or fast-math) and hr_lex.hip (the handle,
// the device CSR arrays and the scan kernel).
#pragma once
#include <cstdint>
#include <string>

#include "../../include/hiprag.h"

int set_err(int code, const std::string& msg);  // hr_index.hip

namespace hrlex {
constexpr uint32_t kTermSpan = 1u << HR_LEX_TERM_BITS;
constexpr int kTfBits = 10, kTfMax = 1023, kDlMax = 65535;

// A = idf * (k1 + 1), idf = log(1 + (N - df + 0.5) / (df + 0.5)): every operation rounded once, host libm log
double bm25_A(int64_t n_live, int64_t df, double k1);
// out[dl] = k1 * ((1 - b) + b * (dl / avgdl)) for dl = 0 .. max_dl
void bm25_K_table(double k1, double b, double avgdl, int max_dl, double* out);
}  // namespace hrlex
