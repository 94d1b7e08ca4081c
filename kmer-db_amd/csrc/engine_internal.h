// engine_internal.h — lets the other translation units of libkmdb_amd.so (new2all.hip) reach
// the HBM-resident database that engine.hip owns.  Not installed.
#pragma once
#include "dev_mem.h"

#include <hip/hip_runtime.h>
#include <cstdint>

struct kmdb_db;

constexpr uint32_t KMDB_ID_BITS = 20, KMDB_MAX_SAMPLES = 1u << KMDB_ID_BITS;   // sample ids in the device layout (engine_state.h: kmdb_k0_pack)
constexpr uint32_t KMDB_CK_IDS = 32;   // list index of new2all: one checkpoint per 32 local ids of a long list

struct kmdb_engine_view {
    int device;
    uint64_t N, P;
    uint32_t kmer_length;
    const uint4* meta;
    const uint64_t* bitpos;
    const int32_t* parent;
    const uint32_t* w;
    const uint32_t* sub_end;
    const uint64_t* bits;
    const uint32_t* ck_ofs;        // list index of the long local lists (engine_state.h)
    const uint64_t* ck_bit;
    const uint32_t* ck_id;
    uint64_t n_buckets;
    const uint64_t* bucket_offset;
    const uint64_t* slots;
    const uint32_t* pid2dfs;
    uint32_t qs_index, qs_count;   // query shard: qs_count > 1, the tables hold the buckets b % qs_count == qs_index at b / qs_count and DFS indices as values; pid2dfs is null
    uint32_t max_depth;            // nodes on the longest root path
    // list store of db2db.hip, kept with the handle: the full sample list of every pattern as a bit set of list_sets_nb words
    // (built on the first db2db call that can afford it; the handle owns it)
    DevBuf<unsigned long long>* list_sets;
    uint32_t* list_sets_nb;
    bool* list_sets_tried;
    // run index of new2all.hip, kept with the handle: node i's local ids as runs rl_runs[rl_ofs[i] .. rl_ofs[i + 1]) (start | length << rs, n2a_run_shift)
    DevBuf<uint32_t>* rl_ofs;
    DevBuf<uint32_t>* rl_runs;
    DevBuf<uint4>* rl_node;              // and the walk's 16-byte node records {subtree end, parent, first run or the only id, min(l, 65535) | min(runs, 65535) << 16}
    bool* rl_tried;
    uint64_t* device_bytes;
    struct kmdb_db2db_stats* d2_stats;   // the last db2db call with this handle as the row database (kmdb_db2db_stats_get)
    struct kmdb_sample_stats* d2_sample_stats;   // the last sampled db2db call with this handle as the row database (kmdb_db2db_sample_stats_get)
    struct kmdb_new2all_sparse_stats* n2s_stats;   // the last sparse new2all call on the handle (kmdb_new2all_sparse_stats_get)
    struct kmdb_sample_stats* n2a_sample_stats;   // the last sampled new2all call on the handle (kmdb_new2all_sample_stats_get)
    void* stream;
    void* ev[4];
};

// also builds the v1 / new2all node arrays on first use; non-zero on failure
int kmdb_engine_get(kmdb_db* db, kmdb_engine_view* out);
void kmdb_engine_set_times(kmdb_db* db, double kernel_ms, double dominant_ms);

// ---- the sparse form of new2all (new2all_sparse.hip; node.hip compacts every device's chunk with it)
struct kmdb_sparse_rows;
struct kmdb_cell_filter;
struct kmdb_opts;
struct kmdb_new2all_sparse_stats;
// The device half of kmdb_new2all_rows_sparse_device: the cells [cell_lo, cell_hi) of a row-major nq x N buffer (cells_dev points at cell_lo,
// complete on the stream of `opts`) -> CSR of all nq rows in `out`, the widened bounds applied (a = query_kmers[row], b = sample_kmers[col]);
// no exact decision.  stats (may be null): cells, nnz_device (= nnz), d2h_bytes, compact_ms.  0, or 1 with the error set (out freed).
int kmdb_n2a_rows_compact(const char* who, kmdb_db* db, const uint32_t* cells_dev, size_t nq, uint64_t cell_lo, uint64_t cell_hi, const uint32_t* query_kmers,
                          const kmdb_cell_filter* filters, size_t n_filters, const uint32_t* sample_kmers, kmdb_sparse_rows* out, const kmdb_opts* opts,
                          kmdb_new2all_sparse_stats* stats);

// ---- the -min / -max filters of the sparse calls (engine.hip; db2db.hip uses them for its cell of two databases)
// argument checks of a filtered call, before any device work; sample_kmers: the count array (null when the caller holds none); 0, or 1 with the error set
int kmdb_check_filters(const char* who, const kmdb_cell_filter* filters, size_t n_filters, const uint32_t* sample_kmers, int measure);
// every host bound as the device's widened bound on a plain ratio (ratio_bound and its margin): kind / lo / hi of cell_filter.h's DevFilter
void kmdb_dev_bounds(const kmdb_cell_filter* filters, size_t n_filters, int kmer_length, int* kind, double* lo, double* hi);
// The exact decision on the host: every cell of `out` the device kept is decided by kmdbh_metric(metric, c, row_kmers[row], col_kmers[col], k)
// against the bounds, the rows are compacted in place and, with measure >= 0, out->measure is filled.  0, or 1 with the error set (out freed).
int kmdb_sparse_decide(const char* who, kmdb_sparse_rows* out, const kmdb_cell_filter* filters, size_t n_filters, const uint32_t* row_kmers,
                       const uint32_t* col_kmers, int measure, int kmer_length);

// ---- a cell's CSR kept in HBM (distance.hip gathers the cells of a block row of the all2all-parts grid from these)
struct kmdb_csr_dev {
    DevBuf<void> row_ptr;          // uint64[n_rows + 1]
    DevBuf<void> col, val;         // uint32[nnz]: columns local to the cell, ascending within a row; counts > 0
    uint64_t n_rows = 0, nnz = 0;
};
// kmdb_db2db_sparse_filtered without bounds and without the copy to the host: the cell (db_row, db_col) compacted where it is, complete when
// the call returns.  Retries once without the list stores on out-of-memory, as every db2db entry.  0, or 1 with the error set.
int kmdb_db2db_csr_device(const char* who, kmdb_db* db_row, kmdb_db* db_col, kmdb_csr_dev* keep, const kmdb_opts* opts);
// kmdb_all2all_sparse the same way: the lower triangle of one database
int kmdb_all2all_csr_device(const char* who, kmdb_db* db, kmdb_csr_dev* keep, const kmdb_opts* opts);

// ---- the -sample-rows selection on a rectangle of two sample sets (engine.hip over sample_rows.hip; db2db.hip selects its cell with it)
struct kmdb_sample_stats;
// argument checks of a sampled call, before any device work (sample_kmers: null when the caller lacks one of the count arrays)
int kmdb_check_sample_args(const char* who, const kmdb_cell_filter* filters, size_t n_filters, const uint32_t* sample_kmers, int criterion, uint32_t count);
// nr + nc and the tile count against the select's 31-bit sizes
int kmdb_sample_rect_check(const char* who, uint64_t nr, uint64_t nc);
// The complete candidates (selection, completeness rule, re-fetch) of a row-major nr x nc rectangle in HBM, complete on `st`; touched: one flag
// per 64 x 64 tile at row block * ceil(nc / 64) + column block, or null.  out_row: nr rows, columns local to the column set; out_col: nc rows,
// columns local to the row set; ascending columns, val = common k-mers.  stats (may be null) is filled.  0, or 1 with the error set (outs freed).
int kmdb_sample_rect(const char* who, hipStream_t st, int kmer_length, const uint32_t* cells_dev, uint64_t nr, uint64_t nc, const unsigned char* touched,
                     const kmdb_cell_filter* filters, size_t n_filters, const uint32_t* row_kmers, const uint32_t* col_kmers, int criterion, uint32_t count,
                     kmdb_sparse_rows* out_row, kmdb_sparse_rows* out_col, kmdb_sample_stats* stats);

// ---- the same selection on the query rows of new2all (engine.hip over sample_rows.hip; new2all_sparse.hip selects a batch's rows with it)
// n_cols in [1, 2^32), nq < 2^31, cell_lo <= cell_hi <= nq * n_cols — before any device work
int kmdb_sample_query_rows_check(const char* who, uint64_t nq, uint64_t n_cols, uint64_t cell_lo, uint64_t cell_hi);
// The complete candidates of the flat cells [cell_lo, cell_hi) of a row-major nq x n_cols rectangle of query rows (cells_dev points at cell_lo,
// complete on `st`): all nq rows in `out`, the rows outside the range empty, ascending sample ids, val = common k-mers, no measures.  One-sided:
// a = query_kmers[row], b = sample_kmers[col].  stats (may be null) is filled.  0, or 1 with the error set (out freed).
int kmdb_sample_query_rows(const char* who, hipStream_t st, int kmer_length, const uint32_t* cells_dev, uint64_t nq, uint64_t n_cols, uint64_t cell_lo, uint64_t cell_hi,
                           const uint32_t* query_kmers, const kmdb_cell_filter* filters, size_t n_filters, const uint32_t* sample_kmers, int criterion, uint32_t count,
                           kmdb_sparse_rows* out, kmdb_sample_stats* stats);

// ---- a band of the matrix's rows (a2a_rows.hip: kmdb_all2all_rows_device / kmdb_all2all_rows / kmdb_all2all_rows_stats_get of include/kmdb_amd.h).
// Tree form on the node arrays of kmdb_ensure_v1_arrays: a select launch (a lane per node) and an apply launch (a fixed grid of waves over the
// selected nodes) that add the cells [tri(row_lo), tri(row_hi)) and no other; the id stacks are the handle's stack_scratch, shared with a2a_v1.hip.
constexpr int KMDB_ROWS_LDS_CAP = 1024;   // a full list of up to this many ids is rebuilt on the wave's LDS stack, a longer one in global scratch
// The argument checks every band call shares (a2a_rows.hip; a2a_band.hip and a2a_rows_records.hip refuse the same cases in the same words under their
// own names): row_lo <= row_hi <= N, shard_count 1, known flag bits, no query shard; and a band of 2^32 cells or more against the device's memory
// (against_free: its free memory — the call allocates the band itself).  0, or 1 with the error set.
int kmdb_band_check(const char* who, const kmdb_db* db, uint64_t row_lo, uint64_t row_hi, const kmdb_opts* opts);
int kmdb_band_check_bytes(const char* who, uint64_t band_cells, bool against_free);
// cells in front of row i of the lower triangle (the host's; the kernels' is tri64 of device_common.h)
inline uint64_t kmdb_tri(uint64_t i) { return i ? i * (i - 1) / 2 : 0; }
// A band entry point whole (a2a_rows.hip): null handle, kmdb_band_check, null buffer for a band with cells, the device, kmdb_band_check_bytes, the stream,
// `run` — the form's own work, `out` device memory for it — and kmdb_release_staging.  host_out: `out` is host memory; the band is made on the device for
// the call, copied back and released.
typedef int (*kmdb_band_runner)(const char* who, kmdb_db* db, uint32_t* out, uint64_t row_lo, uint64_t row_hi, const kmdb_opts* opts, hipStream_t st);
int kmdb_band_call(const char* who, kmdb_db* db, uint64_t row_lo, uint64_t row_hi, void* out, bool host_out, const kmdb_opts* opts, kmdb_band_runner run);

// sort + matrix-core accumulation of block records into a dense n_rows x n_cols matrix (a2a_blocks.hip; used by db2db.hip).
// Record = 16 bytes {row mask, column mask} + key word {stream = row block * nbc + column block | (weight digit | digit index << d) << key_bits},
// d = 32 - key_bits - 2; slots never written carry the key 0xFFFFFFFF.
int kmdb_rect_sort_apply(hipStream_t st, uint32_t* wkey, void* wrec, uint32_t nslots, uint32_t nbr, uint32_t nbc, int key_bits, uint32_t* M, uint32_t n_rows,
                         uint32_t n_cols);
