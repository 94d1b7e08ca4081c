// sample_rows.h — the device selection of `-sample-rows` candidates (sample_rows.hip) as the entry points of engine.hip call it.  Not installed.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <vector>

struct kmdb_sample_job {
    const uint32_t* cells = nullptr;        // device: cell `cell_lo` of the lower triangle
    uint64_t N = 0, cell_lo = 0, cell_hi = 0;
    const unsigned char* touched = nullptr; // device, or nullptr: the tile flags of the block-record pipeline (kmdb_blocks_tile_touched) ...
    uint32_t width = 64;                    // ... and the block width they were made for
    const uint32_t* counts_dev = nullptr;   // device: [N] k-mer counts of the samples
    // The second geometry: a row-major nr x nc rectangle of two sample sets (cells = cell (0, 0); N, cell_lo, cell_hi and width are not read).
    // The samples are nr + nc SLOTS: [0, nr) the row samples, whose lines list local column ids, [nr, nr + nc) the column samples, whose lines
    // list local row ids.  touched: one flag per 64 x 64 tile, tile (X, Y) at X * ceil(nc / 64) + Y (db2db.hip's d2_tile_flags_kernel).
    // counts_dev: [nr] of the row samples; col_counts_dev: [nc] of the column samples (a = the row sample's count on either line of a cell).
    bool rect = false;
    uint64_t nr = 0, nc = 0;
    const uint32_t* col_counts_dev = nullptr;
    // The third geometry: the QUERY ROWS of new2all — the flat cells [cell_lo, cell_hi) of a row-major nr x nc rectangle (nr queries, nc database
    // samples; cells = cell `cell_lo`; N, touched, width and rect are not read).  One-sided: the slots are the rows that meet the range, slot s =
    // query cell_lo / nc + s, whose line lists sample ids; the samples collect nothing.  counts_dev: [slots] the k-mer counts of THOSE queries (a);
    // col_counts_dev: [nc] of the samples (b).
    bool query_rows = false;
    size_t n_bounds = 0;                    // the widened bounds of the filters on their plain ratios (RATIO_* of cell_filter.h)
    int bound_kind[12] = {};
    double bound_lo[12] = {}, bound_hi[12] = {};
    int kind = 0, flip = 0;                 // the criterion's proxy: RATIO_*; 1: negated (the measure falls with its ratio)
    uint32_t count = 0;
};
struct kmdb_sample_result {
    std::vector<uint64_t> row_ptr;          // [N + 1] symmetric rows ([nr + nc + 1] lines of the slots of a rectangle; [slots + 1] query rows), ascending columns
    std::vector<uint32_t> col, val;
    uint64_t rows_truncated = 0, d2h_bytes = 0;
    double select_ms = 0;                   // HIP events around the passes
    uint32_t passes = 0;                    // reads of the triangle / the rectangle
};
// The candidates of every sample's symmetric row (of every slot's line).  only_rows != nullptr: the re-fetch — the listed rows (slots) whole,
// nothing of the others.
// Runs on `st` behind whatever produced the cells and returns when the result is on the host.  0, or 1 with the error set.
int kmdb_sample_candidates(hipStream_t st, const kmdb_sample_job& job, const uint32_t* only_rows, size_t n_only, kmdb_sample_result* out);
// the device's ranking key of a proxy value (order-preserving key of the proxy rounded to float; the largest key for NaN and infinities)
uint32_t kmdb_sample_proxy_key(double proxy);
