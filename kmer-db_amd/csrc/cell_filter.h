// cell_filter.h — the device side of the -min / -max filters, shared by the compaction kernels of engine.hip and db2db.hip and the row
// selection of sample_rows.hip.  Internal to each translation unit (anonymous namespace).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace {
// Device side of the -min / -max filters: every bound is brought to one of six plain ratios of the cell
// (log-based measures are monotone in theirs) and widened by a safety margin on the host; a cell that misses a widened bound is
// dropped here, the rest is decided on the host with the reference's own arithmetic.
enum { RATIO_JACCARD = 0, RATIO_MIN, RATIO_MAX, RATIO_COSINE, RATIO_QUERY, RATIO_NUM };
constexpr int DEV_FILTER_MAX = 12;      // one bound per criterion of Params::availableMetrics (9) and a few repeats
struct DevFilter {
    int n;                          // bounds in use (0: keep every non-zero cell)
    int kind[DEV_FILTER_MAX];
    double lo[DEV_FILTER_MAX], hi[DEV_FILTER_MAX];
    const uint32_t* counts;         // [N] k-mer counts of the samples
};
// the bounds on a non-zero cell whose k-mer counts the caller holds: a of the ROW sample, b of the COLUMN sample (the two may come from
// different arrays: db2db.hip's cell of two databases)
__device__ __forceinline__ bool dev_keep_ab(const DevFilter& f, uint32_t c, uint32_t a, uint32_t b) {
    for (int i = 0; i < f.n; ++i) {
        double x;
        switch (f.kind[i]) {
        case RATIO_JACCARD: x = (double)c / (double)(uint32_t)(a + b - c); break;
        case RATIO_MIN:     x = (double)c / (double)(a < b ? a : b); break;
        case RATIO_MAX:     x = (double)c / (double)(a > b ? a : b); break;
        case RATIO_COSINE:  x = (double)c / sqrt((double)(uint32_t)(a * b)); break;
        case RATIO_QUERY:   x = (double)c / (double)a; break;
        default:            x = (double)c; break;
        }
        if (!(x >= f.lo[i] && x <= f.hi[i])) return false;      // NaN fails, as on the host
    }
    return true;
}
__device__ __forceinline__ bool dev_keep(const DevFilter& f, uint32_t c, uint32_t row, uint32_t col) {
    if (c == 0) return false;
    if (f.n == 0) return true;
    return dev_keep_ab(f, c, f.counts[row], f.counts[col]);
}
// the plain ratio of kind `kind` of a cell (the same expressions as above): what a bound is brought to, and the proxy a row selection ranks by
__device__ __forceinline__ double dev_ratio(int kind, uint32_t c, uint32_t a, uint32_t b) {
    switch (kind) {
    case RATIO_JACCARD: return (double)c / (double)(uint32_t)(a + b - c);
    case RATIO_MIN:     return (double)c / (double)(a < b ? a : b);
    case RATIO_MAX:     return (double)c / (double)(a > b ? a : b);
    case RATIO_COSINE:  return (double)c / sqrt((double)(uint32_t)(a * b));
    case RATIO_QUERY:   return (double)c / (double)a;
    default:            return (double)c;
    }
}
// Query rows (new2all) are cut into segments of this many columns, a wave each, by the compaction of new2all_sparse.hip and by the row select
// of sample_rows.hip: a row of 10 000 samples is 5 waves, a row of a million 489 — enough waves per row to fill the chip with a handful of
// queries, few enough counts (8 B each) that the scan stays small against the rows
constexpr uint32_t N2S_SEG = 2048;
constexpr uint64_t N2S_GRID_MAX = 1ull << 30;           // segments per launch of either: more go out in several launches
}  // namespace
