/*
 * kmdb_amd.h — C ABI of the MI355X-native common-k-mer counting engine.
 *
 * Drop-in boundary for the hot path of refresh-bio/kmer-db v2.3.1.  The reference has no
 * FFI layer; its operator interface for this path is the C++ class SimilarityCalculator
 * (reference src/similarity_calculator.h:4-16) called from the mode consoles.  Each entry
 * point below replaces exactly one of those call sites (plain pointers and sizes only;
 * no torch / STL types cross this boundary).  INTEGRATION.md shows the binding a kmer-db
 * maintainer would add inside the reference's consoles.
 *
 * All functions return 0 on success, non-zero on failure; kmdb_last_error() then returns
 * the message (the front-end turns it into the reference's "ERROR: <msg>" / exit(-1),
 * reference src/main.cpp:51-59).  The GPU entry points FAIL (they never fall back to a CPU
 * path) when no gfx950 device / HIP runtime is usable.
 */
#ifndef KMDB_AMD_H
#define KMDB_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define KMDB_ABI_VERSION 8
/* ABI 8 is ABI 7 plus entry points (tree ranges; query shards; sampled rows): no struct changed its size or the order of its fields, so the library
 * also accepts a kmdb_db_view whose abi_version is 7 — a caller compiled against the previous header runs unchanged.  The sampled-rows entry points
 * (KMDB_HAS_SAMPLED_ROWS) are additive in the same way: the version number stays 8 and a caller built against an earlier ABI 8 header is served. */
#define KMDB_HAS_SAMPLED_ROWS 1
/* So is the sparse, filtered form of db2db (kmdb_db2db_sparse_filtered, kmdb_db2db_stats_get): two more entry points, the version stays 8. */
#define KMDB_HAS_DB2DB_SPARSE 1
/* And the sparse, filtered form of new2all (kmdb_new2all_batch_sparse_filtered and its relatives, kmdb_new2all_sparse_stats_get): seven more
 * entry points and one struct of their own, the version stays 8. */
#define KMDB_HAS_NEW2ALL_SPARSE_FILTERED 1
/* And the minhash mode: a k-mer extractor that needs no database (kmdb_minhash_batch_seq_alphabet and its helpers) and the reader / writer of
 * <sample>.minhash files (kmdbh_minhash_store, kmdbh_minhash_load): eight more entry points and two structs of their own, the version stays 8. */
#define KMDB_HAS_MINHASH 1
/* And the build mode: a database grown on the device from the samples' k-mer lists (kmdb_build_*) and the writer of .db files
 * (kmdbh_db_store): seven more entry points and one struct of their own, the version stays 8. */
#define KMDB_HAS_BUILD 1
/* And the seed of the build mode: a builder that starts from a stored database (kmdb_build_begin_from_db, kmdb_build_seed_stats_get): two more
 * entry points and one struct of their own, the version stays 8. */
#define KMDB_HAS_BUILD_SEED 1
/* And the hand-off of a finished builder to the engine in HBM (kmdb_build_finish_device, kmdb_build_handoff_stats_get; kmdbh_db_header_only):
 * three more entry points, same version number, no struct changed. */
#define KMDB_HAS_BUILD_HANDOFF 1
/* And the distance mode on the device: the table of common k-mer counts parsed, measured and formatted in HBM (kmdb_distance_*), and the one
 * definition of a measure's text (kmdbh_format_measure): six more entry points and three structs of their own, the version stays 8. */
#define KMDB_HAS_DISTANCE 1
/* And a second source of cells for the distance handle: a lower triangle of counts that is in HBM already — the one kmdb_all2all_dense_device
 * computes, or one the caller accumulated — measured and formatted without ever being text (kmdb_distance_take_all2all,
 * kmdb_distance_take_cells_device, kmdb_distance_matrix_rows, kmdb_distance_cells_device): four more entry points, no struct changed, the version stays 8. */
#define KMDB_HAS_DISTANCE_MATRIX 1
/* And the distance mode fed from the rows of a batch of new2all queries in HBM — computed into a rectangle the handle owns, or one the caller
 * accumulated (kmdb_distance_take_new2all_batch, kmdb_distance_take_new2all_batch_seq_alphabet, kmdb_distance_take_rows_device,
 * kmdb_distance_query_rows): four more entry points, no struct changed, the version stays 8. */
#define KMDB_HAS_DISTANCE_QUERY_ROWS 1
/* And the distance mode fed from a CSR in HBM over a run of rows — a block row of the all2all-parts grid gathered on the device from its cells'
 * CSRs, or one the caller built (kmdb_distance_parts_begin_rows, kmdb_distance_parts_add_db2db, kmdb_distance_parts_add_all2all,
 * kmdb_distance_parts_add_csr_device, kmdb_distance_take_csr_device, kmdb_distance_csr_rows, kmdb_distance_csr_device, kmdb_distance_csr_row_ptr,
 * kmdb_distance_parts_stats_get): nine more entry points and one struct of their own, the version stays 8. */
#define KMDB_HAS_DISTANCE_PARTS 1
/* And the -sample-rows selection on an off-diagonal cell of the all2all-parts grid: the candidates of a rectangle of two sample sets chosen in
 * HBM (kmdb_db2db_sampled, kmdb_sampled_from_rect_device, kmdb_db2db_sample_stats_get): three more entry points, no struct changed, the version
 * stays 8. */
#define KMDB_HAS_DB2DB_SAMPLED 1
/* And the -sample-rows selection on the query rows of new2all: every query's best database samples chosen in HBM (kmdb_new2all_batch_sampled,
 * kmdb_new2all_batch_seq_alphabet_sampled, kmdb_sampled_from_rows_device, kmdbh_query_rows_select, kmdb_new2all_sample_stats_get, and over
 * the GPUs of a node kmdb_node_new2all_batch_sampled, kmdb_node_new2all_batch_seq_alphabet_sampled, kmdb_node_new2all_sample_stats_get): eight
 * more entry points, no struct changed, the version stays 8. */
#define KMDB_HAS_NEW2ALL_SAMPLED 1
/* And long samples in the minhash extractor: a sample beyond a threshold is extracted in sections whose sorted unique lists are joined on the
 * device by a merge-union of two ascending arrays (kmdb_sorted_union_device, kmdb_sorted_union_geometry, kmdb_minhash_long_stats_get): three
 * more entry points and one struct of their own, the version stays 8. */
#define KMDB_HAS_LONG_SAMPLES 1
/* And a band of the all2all matrix's rows computed alone: the cells of rows [row_lo, row_hi) and nothing else of the triangle in HBM
 * (kmdb_all2all_rows_device, kmdb_all2all_rows, kmdb_all2all_rows_stats_get; kmdb_device_buffer_alloc, kmdb_device_buffer_free for a caller
 * without HIP of its own): five more entry points and one struct of their own, the version stays 8. */
#define KMDB_HAS_ALL2ALL_ROWS 1

/* ---------------------------------------------------------------------------------------
 * Host-side view of a loaded database = what the reference hands to SimilarityCalculator:
 *   PrefixKmerDb::getPatterns()      (prefix_kmer_db.h:112)   -> SoA pattern headers + bits
 *   PrefixKmerDb::getHashtables()    (prefix_kmer_db.h:108)   -> bucket table + slots
 *   AbstractKmerDb::getSamplesCount()(kmer_db.h:67)
 * Pattern fields mirror pattern_t (pattern.h:42-53) as stored on disk (pattern.cpp:15-46).
 * The view is read-only: unlike the reference (similarity_calculator.cpp:64-72) the engine
 * never mutates num_kmers.
 * ------------------------------------------------------------------------------------- */
typedef struct kmdb_db_view {
    uint32_t abi_version;          /* KMDB_ABI_VERSION */
    uint32_t kmer_length;
    uint64_t n_samples;
    uint64_t n_patterns;
    const int64_t*  num_kmers;     /* [P] on-disk values (not subtree sums) */
    const int64_t*  parent_id;     /* [P] -1 for roots; parent_id[p] < p */
    const uint32_t* num_samples;   /* [P] ids in node + ancestors */
    const uint32_t* num_local;     /* [P] ids stored in the node */
    const uint32_t* last_sample_id;/* [P] */
    const uint32_t* num_bits;      /* [P] gamma bitstream length */
    const uint64_t* data_offset;   /* [P] index (in uint64 words) of the node's stream in `data` */
    const uint64_t* data;          /* all gamma streams, MSB-first in little-endian uint64 words */
    uint64_t n_data_words;
    /* hashtables: needed by new2all only (all2all loads with SkipHashtables,
     * console_all2all.cpp:26); n_buckets may be 0. item = {u32 key; i32 val} packed in a
     * uint64 (key low), val == INT32_MAX means empty (hashmap_lp.h:71-78). */
    uint64_t n_buckets;
    const uint64_t* bucket_offset; /* [n_buckets+1] first slot of every bucket in `slots` */
    const uint64_t* slots;         /* capacity of bucket b = bucket_offset[b+1]-bucket_offset[b], a power of two */
} kmdb_db_view;

typedef struct kmdb_opts {
    uint32_t abi_version;          /* KMDB_ABI_VERSION */
    int32_t  device;               /* HIP device ordinal */
    /* pattern-stream sharding of ONE resident database: this call adds the pairs of the patterns in
     * slice `shard_index` of `shard_count` equal slices of the (DFS-ordered) pattern stream; partial
     * matrices from all slices sum (uint32, wrap-around) to the full result.  {0,1} = everything.
     * (Prefix-bucket shards and tree ranges, one per GPU, are made at upload: kmdb_db_upload_shard, kmdb_db_upload_range.) */
    uint32_t shard_index;
    uint32_t shard_count;
    uint32_t bubble_size;          /* all2all-sp: -bubble-size (params.h:78), kept for CLI compat; 0 = default 8000 */
    uint32_t flags;                /* KMDB_FLAG_* */
    void*    stream;               /* hipStream_t to run on, NULL = the engine's own stream */
} kmdb_opts;

#define KMDB_FLAG_FORCE_GLOBAL_ATOMICS 1u   /* A/B reference: tree-form walk, id stack in global scratch, HBM atomics (any N, any depth) */
#define KMDB_FLAG_FORCE_DIRECT         2u   /* A/B reference: tree-form walk, id stack in LDS, HBM atomics */
#define KMDB_FLAG_FORCE_TILE           4u   /* A/B reference: tree-form walk, wave-private LDS tile */
#define KMDB_FLAG_NO_FALLBACK          8u   /* fail instead of taking the HBM-atomics kernel when the block-record pipeline cannot
                                              take the database (kmdb_stats.path tells which one ran) */
#define KMDB_FLAG_ONE_SHOT             16u  /* at upload: the handle serves a process that ends after its call (the command-line front-end):
                                              the upload's host staging buffers stay mapped until kmdb_db_free / process exit instead of being
                                              unmapped by a helper thread after the first call (3.5 GB at 100 M patterns: 0.3 s of address-space
                                              work that stalls every other thread's allocations meanwhile) */
#define KMDB_FLAG_ALL                  31u  /* any other bit in kmdb_opts.flags is rejected */

/* kmdb_stats.path */
#define KMDB_PATH_NONE     0u
#define KMDB_PATH_RECORDS  1u   /* block-record pipeline (default) */
#define KMDB_PATH_TILE     2u   /* v1 LDS tile / direct kernels (forced by a flag) */
#define KMDB_PATH_GLOBAL   3u   /* v1 HBM-atomics kernel (forced, or fallback: a note goes to stderr) */

typedef struct kmdb_db kmdb_db;    /* database resident in HBM */

/* Result of the sparse calls: CSR, library-allocated, free with kmdb_sparse_free().
 * Row i lists (col, val) with val > 0, ascending col — the content of
 * SparseMatrix::data_compacted after compact2 with pass-all filters (array.h:391-446). */
typedef struct kmdb_sparse_rows {
    uint64_t  n_rows;
    uint64_t  nnz;
    uint64_t* row_ptr;             /* [n_rows+1] */
    uint32_t* col;                 /* [nnz] 0-based */
    uint32_t* val;                 /* [nnz] */
    double*   measure;             /* [nnz] or NULL: kmdb_all2all_sparse_filtered with a measure */
} kmdb_sparse_rows;

/* Similarity / distance measures of a cell (common k-mers c, k-mer counts a of the row sample and b of the column sample,
 * k-mer length k): the functions of Params::availableMetrics (params.cpp:14-42), in that order. */
#define KMDB_METRIC_JACCARD     0
#define KMDB_METRIC_MIN         1
#define KMDB_METRIC_MAX         2
#define KMDB_METRIC_COSINE      3
#define KMDB_METRIC_MASH        4
#define KMDB_METRIC_ANI         5
#define KMDB_METRIC_ANI_SHORTER 6
#define KMDB_METRIC_MASH_QUERY  7
#define KMDB_METRIC_NUM_KMERS   8
#define KMDB_METRIC_COUNT       9
/* One bound pair of a CombinedFilter (sparse_filters.h:12-61): the cell passes when lo <= metric(cell) <= hi. */
typedef struct kmdb_cell_filter {
    int32_t metric;                /* KMDB_METRIC_* */
    int32_t reserved;
    double  lo, hi;
} kmdb_cell_filter;

typedef struct kmdb_stats {        /* measurements of the LAST call on this db handle */
    double   kernel_ms;            /* HIP-event time of the whole device pipeline of the call */
    uint64_t algorithmic_bytes;    /* B_pat + 4*N(N-1)/2 (dense) */
    uint64_t tree_updates;         /* cell updates performed (tree form) */
    uint64_t sum_pairs;            /* sum_p w_p*C(n_p,2) = sum of the matrix = k-mer pair comparisons */
    uint64_t device_bytes;         /* HBM footprint of the resident db */
    uint64_t n_segments;
    uint64_t tile_flushes;
    double   k1_ms;                /* block-record pipeline: emit kernel */
    double   k2_ms;                /* block-record pipeline: apply kernel */
    uint64_t n_records;            /* block records per pass (0 when the v1 kernels ran) */
    double   k0_ms;                /* block-record pipeline: gamma decode kernels */
    double   k1n_ms;               /* ... emit, nodes with at most two blocks (DFS stream) */
    double   k1g_ms;               /* ... wide list + emit, nodes with more blocks */
    double   upload_ms;            /* wall-clock of kmdb_db_upload for this handle (host conversion + H2D + device layout) */
    uint64_t n_wide;               /* nodes with more than two blocks */
    uint64_t n_chunks;             /* record chunks = work items of the apply kernel */
    uint32_t path;                 /* KMDB_PATH_* of the last all2all call */
    uint32_t width;                /* sample ids per block */
    uint32_t sized_call;           /* 1: the last call measured its own grid sizes (first call on a handle, two host syncs more) */
    uint32_t n_joined;             /* nodes with many blocks whose records were never written: joined per tile by the second level (ABI 6; 0 when it is off) */
    uint64_t n_patterns;           /* patterns resident in HBM: all of the view's, or for kmdb_db_upload_shard only the nodes whose subtree
                                      holds a k-mer of the shard, or for kmdb_db_upload_range the nodes of the range and the ancestors of its first node */
    uint64_t h2d_bytes;            /* bytes kmdb_db_upload[_shard|_range] copied to the device (ABI 6) */
    uint64_t n_direct;             /* first-block records (X, X) with a weight below 128 that never went through the record pools, summed over the slices
                                      of the pattern stream a call takes.  Default (KMDB_K1N_MODE=2): written compacted, 12 bytes each, by the narrow kernel
                                      and read back by k2d_kernel, tile in registers, one write-back per change of block.  KMDB_K1N_MODE=1: applied where the
                                      narrow kernel emitted them, never written.  KMDB_K1N_MODE=0: always 0 (ABI 7; n_records counts the pool's records) */
} kmdb_stats;

const char* kmdb_last_error(void);
int  kmdb_abi_version(void);
/* number of usable gfx950 devices, 0 if none (never fails) */
int  kmdb_device_count(void);
/* First use of a device (runtime start, the device's context, a first allocation and stream): 0.15 - 0.3 s that depend on nothing the
 * database holds.  The front-end calls this on a helper thread while kmdbh_db_load reads the file (the reference has no counterpart:
 * console_all2all.cpp:25-29 goes straight from deserialize to the computation).  0, or 1 with kmdb_last_error() set in the calling thread. */
int  kmdb_device_prepare(int32_t device);

/* Lay the database out in HBM (replaces PrefixKmerDb living in host RAM after
 * deserialize, prefix_kmer_db.cpp:578-748).  with_hashtables != 0 also uploads the
 * bucket tables (DeserializationMode::Everything vs SkipHashtables, kmer_db.h:55-60). */
int  kmdb_db_upload(const kmdb_db_view* view, const kmdb_opts* opts, int with_hashtables, kmdb_db** out);
/* One prefix-bucket shard of the database (bucket = kmer >> 32, reference src/types.h:25-27, items
 * src/hashmap_lp.h:71-78): the pattern tree stays whole and every pattern keeps only the k-mers of the buckets b with
 * b % shard_count == shard_index, w_s[p] = #{items of those buckets with val == p}.  Partial matrices of the shards sum
 * (uint32, wrap-around) to the matrix of the whole database: one shard per GPU + one RCCL reduce.  The view must carry the
 * hashtables (load mode Everything). */
int  kmdb_db_upload_shard(const kmdb_db_view* view, const kmdb_opts* opts, int with_hashtables, uint32_t shard_index,
                          uint32_t shard_count, kmdb_db** out);
/* One tree range of the database (the pattern / subtree is the natural unit of all2all; ABI 8).  Serves the all2all call
 * sites, console_all2all.cpp:26,31-36, which load the database with SkipHashtables: the view needs NO hashtables (n_buckets may be 0).
 * The DFS pre-order of the pattern tree (children of a node, and the roots, in ascending pattern id: the order of the resident stream)
 * is cut into range_count contiguous stretches of about equal estimated cost; the handle holds the nodes of stretch range_index at their
 * on-disk num_kmers, and the ancestors of the stretch's first node that lie before it at weight 0 (they only supply sample ids):
 * kmdb_stats.n_patterns = nodes of the range + depth of its first node - 1.  Every pattern adds w_p to the cells of its own id list
 * independently of every other, so the partial matrices of the ranges sum (uint32, wrap-around) to the matrix of the whole database, and
 * kmdb_stats.sum_pairs (the range's own sum_p w_p C(n_p, 2)) is the sum of the range's matrix.  The cuts depend on (view, range_count)
 * only: processes that each upload one range agree.  An empty range (range_count > patterns) holds pattern 0 at weight 0: a zero matrix.
 * For all2all / all2all-sp only — no hashtables are copied (new2all and db2db need every pattern id); kmdb_opts.shard_index /
 * shard_count slice the handle's resident stream as on any other.  range_count == 1 is kmdb_db_upload(view, opts, 0, out). */
int  kmdb_db_upload_range(const kmdb_db_view* view, const kmdb_opts* opts, uint32_t range_index, uint32_t range_count, kmdb_db** out);
/* One QUERY shard of the database (prefix buckets are the natural new2all partition).  Makes the query call sites multi-GPU:
 * one2all / one2all_sp at console_new2all.cpp:64-95 (:82, :78) and console_one2all.cpp — a database whose tables do not fit one device
 * answers queries from several.  The handle holds the pruned tree of prefix shard shard_index of shard_count (the nodes whose subtree holds
 * a k-mer of a bucket b with b % shard_count == shard_index, at the shard's own weights, exactly as kmdb_db_upload_shard lays it out) AND
 * the slots of those buckets only: local bucket b / shard_count, capacities and slot order unchanged (probing stays slot-exact), every
 * value rewritten from the view's pattern id to the node's index in the handle's own layout (the empty marker INT32_MAX stays).  No slot
 * of a foreign bucket crosses PCIe and nothing of the size of the view's pattern or slot count stays on the device; kmdb_stats.h2d_bytes,
 * device_bytes and n_patterns report what the shard holds.  The new2all entry points on such a handle count only the k-mers of its own
 * buckets (a foreign k-mer is a miss): every k-mer belongs to one bucket, so the rows of the shards sum (uint32) to the rows of the whole
 * database, and out_kmer_counts of the sequence entry sum to the query's count.  All2all on it gives the shard's partial matrix as on
 * any prefix shard.  A shard that owns no k-mer is a valid handle (zero rows, a zero matrix; it keeps the tree at weight 0 like an empty
 * prefix shard).  The view must carry the hashtables; a value that is no pattern id of the view is refused.  shard_count == 1 is
 * kmdb_db_upload(view, opts, 1, out). */
int  kmdb_db_upload_query_shard(const kmdb_db_view* view, const kmdb_opts* opts, uint32_t shard_index, uint32_t shard_count, kmdb_db** out);
void kmdb_db_free(kmdb_db* db);
/* Waits for the handle's background housekeeping (the upload's host staging buffers are given back by a helper thread after the first
 * call).  A front-end that ends the process right after its call waits here first: the helper's threads free the pages several times
 * faster than the end of the process would. */
void kmdb_db_settle(kmdb_db* db);
int  kmdb_db_stats(const kmdb_db* db, kmdb_stats* out);
/* Why the last all2all call on this handle could not take the block-record pipeline ("" when it did, or before any call): the
 * note the engine prints once on stderr when it falls back to the HBM-atomics kernel (kmdb_stats.path == KMDB_PATH_GLOBAL), e.g.
 * a root path of more than 4096 nodes.  The pointer stays valid until the next call on the handle. */
const char* kmdb_db_fallback_reason(const kmdb_db* db);

/* Replaces SimilarityCalculator::all2all(db, LowerTriangularMatrix&)
 * (similarity_calculator.cpp:42-438; call site console_all2all.cpp:34).
 * out_lower_tri: N(N-1)/2 uint32 in HOST memory, row i at i(i-1)/2 (array.h:136-140). */
int  kmdb_all2all_dense(kmdb_db* db, uint32_t* out_lower_tri, const kmdb_opts* opts);
/* Same, result left in DEVICE memory (caller-owned, N(N-1)/2 uint32, need not be zeroed)
 * so that per-GPU partial matrices can be reduced with RCCL without a host round trip. */
int  kmdb_all2all_dense_device(kmdb_db* db, void* out_lower_tri_dev, const kmdb_opts* opts);

/* A band of that matrix: rows [row_lo, row_hi) alone (KMDB_HAS_ALL2ALL_ROWS).  The reference adds, for every local id of a pattern, the
 * pattern's subtree weight to the cells of all ids in front of it on the root path (similarity_calculator.cpp:213-233): a row of the matrix is
 * written only by the patterns that hold its sample as a LOCAL id.  The band call selects those patterns from the node arrays, rebuilds their root
 * paths and adds their rows inside the band; no cell outside it exists anywhere.  What it serves: the new rows after a collection was extended
 * (build -extend-from: rows [old N, N)), and a part of a matrix whose triangle does not fit.
 * out_cells holds tri(row_hi) - tri(row_lo) uint32, tri(i) = i (i - 1) / 2 in 64 bits: cell tri(row_lo) of the lower triangle onwards — the
 * layout kmdb_sparse_from_dense_device, kmdb_sampled_from_dense_device (cell_lo = tri(row_lo), cell_hi = tri(row_hi)) and
 * kmdb_distance_take_cells_device (row_lo) take.  Caller-owned, need not be zeroed, written on opts->stream (the handle's own when NULL); the call
 * returns when the cells are complete.  DEFINITION: exactly the cells [tri(row_lo), tri(row_hi)) of what kmdb_all2all_dense_device writes for the
 * same handle (uint32, wrap-around; adds commute, so bit-exact) — a prefix shard or a tree range gives its partial band.
 * Refused with a message: null arguments, row_lo > row_hi, row_hi > N, kmdb_opts.shard_count > 1 (a band takes the whole pattern stream), unknown
 * flag bits (the KMDB_FLAG_FORCE_* bits are accepted and mean nothing here: there is one path), a query-shard handle, and a band of 2^32 cells
 * or more whose bytes exceed the device's memory (kmdb_all2all_rows, which allocates the band: its free memory); the message names the bytes.
 * An empty band (row_lo == row_hi, or row_hi <= 1) succeeds and writes nothing.
 * Limits: a node is applied by one wave however long its list is (no node splitting); one device (a node handle has no band call). */
typedef struct kmdb_all2all_rows_stats {   /* the LAST band call on the handle */
    uint64_t nodes_selected;       /* nodes the select launch listed: a superset, chosen without decoding a list */
    uint64_t nodes_applied;        /* of those, the nodes that had a local id inside the band */
    uint64_t updates;              /* cell additions issued */
    uint64_t band_cells;           /* tri(row_hi) - tri(row_lo) */
    uint64_t scratch_bytes;        /* the call's working memory on the handle: node list, counters, per-wave id stacks */
    double   select_ms;            /* HIP events around the select launch ... */
    double   apply_ms;             /* ... and the apply launch (kmdb_stats.kernel_ms holds the whole call) */
} kmdb_all2all_rows_stats;
int  kmdb_all2all_rows_device(kmdb_db* db, uint64_t row_lo, uint64_t row_hi, void* out_cells_dev, const kmdb_opts* opts);
/* the same with the band copied to HOST memory (the device buffer lives for the call) */
int  kmdb_all2all_rows(kmdb_db* db, uint64_t row_lo, uint64_t row_hi, uint32_t* out_cells_host, const kmdb_opts* opts);
int  kmdb_all2all_rows_stats_get(const kmdb_db* db, kmdb_all2all_rows_stats* out);
/* `bytes` of device memory on `device` for a caller that links no HIP runtime (the command-line front-end holds the band of -rows in it between
 * kmdb_all2all_rows_device and the calls that read it); not zeroed; freed with kmdb_device_buffer_free (a null pointer is ignored). */
int  kmdb_device_buffer_alloc(int32_t device, uint64_t bytes, void** out);
void kmdb_device_buffer_free(int32_t device, void* p);

/* The same band, its rows summed in LDS tiles (KMDB_HAS_ALL2ALL_ROWS_TILED; a2a_band.hip).  DEFINITION: bit for bit what kmdb_all2all_rows_device
 * writes for the same arguments.  Row r is written only by the nodes that hold r as a local id; such a node (a "hit" of row r) adds its subtree
 * weight W to column c for every id c < r of its root path.  A job is (row r, a tile of KMDB_ROWS_TILE_COLS columns in front of r, a share of at
 * most KMDB_ROWS_TILE_HITS of the row's hits): one workgroup holds the tile as uint32 words in LDS, enters every run of consecutive ids [s, s + len)
 * of the hits' root paths as +W at s and -W (modulo 2^32) at s + len, takes one inclusive prefix sum over the tile and adds every non-zero cell to
 * the band once.  Both switches are read at every call: KMDB_ROWS_TILE_COLS a multiple of 64 from 64 to 40896 (160 KiB of LDS less the scan's
 * words), KMDB_ROWS_TILE_HITS 1 or more; anything else is refused.  Refusals as for kmdb_all2all_rows_device / kmdb_all2all_rows, under these names;
 * an empty band succeeds and writes nothing.
 * Limits: the list of one node is decoded by one lane per hit however long it is (no wave-cooperative decode); one device. */
#define KMDB_HAS_ALL2ALL_ROWS_TILED 1
typedef struct kmdb_all2all_rows_tiled_stats {   /* the LAST tiled band call on the handle */
    uint64_t nodes_selected;       /* nodes the select launch listed: the superset rule of the band call above */
    uint64_t nodes_applied;        /* of those, the nodes that had a local id inside the band */
    uint64_t hits;                 /* (row, node) records: local ids inside the band of the nodes selected */
    uint64_t jobs;                 /* workgroups of the apply launch: (row, column tile, share of the row's hits) */
    uint64_t runs;                 /* runs entered into a tile, clipped to it and to the row: a pair of LDS adds each (the closing one may be left out) */
    uint64_t updates;              /* cell additions the runs stand for: equal to kmdb_all2all_rows_stats.updates of the same band */
    uint64_t tile_cols;            /* columns of a tile at this call */
    uint64_t band_cells;           /* tri(row_hi) - tri(row_lo) */
    double   select_ms;            /* HIP events around the select launch, ... */
    double   hits_ms;              /* ... the hit passes and the job table (two host round trips inside), ... */
    double   apply_ms;             /* ... and the apply launch (kmdb_stats.kernel_ms holds the whole call) */
    uint64_t scratch_bytes;        /* the call's working memory on the handle: node list, counters, per-row tables, hit records, job table */
} kmdb_all2all_rows_tiled_stats;
int  kmdb_all2all_rows_tiled_device(kmdb_db* db, uint64_t row_lo, uint64_t row_hi, void* out_cells_dev, const kmdb_opts* opts);
int  kmdb_all2all_rows_tiled(kmdb_db* db, uint64_t row_lo, uint64_t row_hi, uint32_t* out_cells_host, const kmdb_opts* opts);
int  kmdb_all2all_rows_tiled_stats_get(const kmdb_db* db, kmdb_all2all_rows_tiled_stats* out);

/* Replaces SimilarityCalculator::all2all_sp(db, SparseMatrix&, CBubbleHelper&) followed by
 * SparseMatrix::compact2 with pass-all filters (similarity_calculator.cpp:442-657,
 * array.h:391-446; call sites console_all2all_sparse.cpp:44,79). */
int  kmdb_all2all_sparse(kmdb_db* db, kmdb_sparse_rows* out, const kmdb_opts* opts);
void kmdb_sparse_free(kmdb_sparse_rows* rows);
/* the same with the -min / -max filters applied before the result leaves HBM, and optionally one measure per
 * kept cell.  Replaces all2all_sp + SparseMatrix::compact2 with a CombinedFilter (array.h:391-446, sparse_filters.h:38-61;
 * call site console_all2all_sparse.cpp:44-79) and, with measure >= 0, the `distance -sparse` pass over the written table
 * (console_distance.cpp:96-171).  sample_kmers[i] = k-mer count of sample i (the table's total-kmers row; num_kmers_t =
 * uint32 in the reference).  The device drops the cells that miss a bound by more than a safety margin; the remaining
 * cells are decided, and the measures computed, by kmdbh_metric on the host — bit-identical with the reference's double
 * arithmetic (incl. its libm log).  measure: KMDB_METRIC_* or -1. */
int  kmdb_all2all_sparse_filtered(kmdb_db* db, const kmdb_cell_filter* filters, size_t n_filters, const uint32_t* sample_kmers,
                                  int measure, kmdb_sparse_rows* out, const kmdb_opts* opts);
/* Multi-GPU all2all-sp (BASELINE configs[3]; SURVEY 8e "reduce compacted tiles"): the compaction stage of the two calls above
 * on cells the CALLER accumulated — typically the sum over prefix-bucket shards, after an RCCL reduce / reduce-scatter of the
 * partial matrices of kmdb_all2all_dense_device.  cells_dev points at cell `cell_lo` of the lower triangle (row i at
 * i (i - 1) / 2, array.h:136-140) and holds the flat range [cell_lo, cell_hi) — a rank's reduce-scatter chunk can be passed as
 * it is; the whole triangle is {0, N (N - 1) / 2}.  out has all N rows; rows outside the range are empty and a row cut by a
 * range end lists only its cells inside, so the ranks' outputs concatenate row by row (rank order = ascending columns) to
 * exactly what SparseMatrix::compact2 + saveRowSparse produce (array.h:391-446, 625-637; console_all2all_sparse.cpp:44-96).
 * Filters / measure as in kmdb_all2all_sparse_filtered (the cells are complete sums here, so prefix shards may use them). */
int  kmdb_sparse_from_dense_device(kmdb_db* db, const void* cells_dev, uint64_t cell_lo, uint64_t cell_hi,
                                   const kmdb_cell_filter* filters, size_t n_filters, const uint32_t* sample_kmers, int measure,
                                   kmdb_sparse_rows* out, const kmdb_opts* opts);
/* NOTE on streams: the call reads cells_dev on opts->stream (the handle's own stream when NULL) and does NOT order itself after
 * the caller's producer: the cells must be complete on that stream (or the device idle) before the call — after an RCCL collective
 * on another stream, wait for it first (hipStreamWaitEvent / hipStreamSynchronize). */
/* kmdb_all2all_sparse_filtered walked in bands of band_rows rows (KMDB_HAS_ALL2ALL_ROWS_TILED): for every band [k R, min((k + 1) R, N)) one band
 * buffer — the largest band's, made once — is filled by the tiled band call and compacted where it lies (kmdb_sparse_from_dense_device on the cells
 * [tri(lo), tri(hi))); its rows are appended to the result.  Only one band is ever resident: the way of one device to a collection whose triangle
 * does not fit (300 000 samples are 180 GB).  DEFINITION: row_ptr, col, val and measure equal to kmdb_all2all_sparse_filtered's for the same
 * arguments.  Refused: band_rows == 0, and everything the two composed calls refuse. */
typedef struct kmdb_all2all_banded_stats {   /* the LAST banded call on the handle */
    uint64_t bands;
    uint64_t max_band_bytes;       /* the band buffer: the largest band's cells, 4 bytes each */
    uint64_t peak_device_bytes;    /* the largest kmdb_stats.device_bytes + band buffer + tiled scratch over the bands */
    uint64_t hits, runs, updates;  /* sums over the bands of kmdb_all2all_rows_tiled_stats */
    double   select_ms, hits_ms, apply_ms;
} kmdb_all2all_banded_stats;
int  kmdb_all2all_sparse_filtered_banded(kmdb_db* db, uint64_t band_rows, const kmdb_cell_filter* filters, size_t n_filters,
                                         const uint32_t* sample_kmers, int measure, kmdb_sparse_rows* out, const kmdb_opts* opts);
int  kmdb_all2all_banded_stats_get(const kmdb_db* db, kmdb_all2all_banded_stats* out);

/* The same band through the block-record pipeline (KMDB_HAS_ALL2ALL_ROWS_RECORDS; a2a_rows_records.hip, a2a_blocks.hip).  DEFINITION: bit for bit
 * what kmdb_all2all_rows_device writes for the same arguments — the cells [tri(row_lo), tri(row_hi)) of kmdb_all2all_dense_device, tri(i) =
 * i (i - 1) / 2, in the out_cells layout of the two band calls above; the band is zeroed by the call and added into, the host variant allocates it.
 * Decode, emit and the sorts run as in a whole-matrix call (same records, same launch sizes: a band call and a whole call share one warm handle);
 * the apply stage works on the block rows Xlo = row_lo / width .. Xhi = (row_hi - 1) / width alone: a stream job, a window run of stream chunks, a
 * slice's tile of first-block records or a second-level tile of another block row does no matrix-core step and no write-back, and a cell is written
 * iff row_lo <= row < row_hi, at tri(row) - tri(row_lo) + col.  The handle's working set is the whole call's less the triangle: the band is the only
 * output.  A database the pipeline cannot take (kmdb_db_fallback_reason) is served by kmdb_all2all_rows_device, and the stats say so; with
 * KMDB_FLAG_NO_FALLBACK the call fails with the reason.
 * Refused with a message, under these names: null arguments, row_lo > row_hi, row_hi > N, kmdb_opts.shard_count > 1, unknown flag bits, a
 * query-shard handle, a band whose bytes exceed the device's memory, and a handle made under KMDB_K1N_MODE=1 (its narrow kernel writes the matrix
 * itself).  A refused call leaves out_cells untouched.  An empty band succeeds and writes nothing.
 * kmdb_stats after a band call: kernel_ms and device_bytes are the band call's; path, n_records, sized_call, the stage times and the other counts
 * stay those of the last whole-matrix call on the handle — the band call's own are in kmdb_all2all_rows_records_stats.
 * Limit of this form: the pipeline's 2^22 block pairs (about 185 000 samples at width 64, 92 640 at width 32).  Beyond it the call takes band emit
 * (KMDB_HAS_ALL2ALL_BAND_EMIT, below), whose limit is 2^22 streams per BAND. */
#define KMDB_HAS_ALL2ALL_ROWS_RECORDS 1
#define KMDB_ROWS_RECORDS_PATH_NONE     0u   /* an empty band: nothing ran */
#define KMDB_ROWS_RECORDS_PATH_RECORDS  1u   /* the block-record pipeline */
#define KMDB_ROWS_RECORDS_PATH_TREE     2u   /* fallback: kmdb_all2all_rows_device ran */
typedef struct kmdb_all2all_rows_records_stats {   /* the LAST such call on the handle */
    uint32_t path;                 /* KMDB_ROWS_RECORDS_PATH_* */
    uint32_t width;                /* sample ids per block */
    uint32_t x_lo, x_hi;           /* block rows the band meets */
    uint32_t sized_call;           /* kmdb_stats.sized_call of this call */
    uint32_t slices;               /* passes over the pattern stream */
    uint64_t band_cells;           /* tri(row_hi) - tri(row_lo) */
    uint64_t records;              /* block records emitted: kmdb_stats.n_records of a whole call on the handle */
    uint64_t units_total;          /* apply units the call met: the sum of the four kinds below ... */
    uint64_t units_run;            /* ... and those inside the band's block rows, which ran */
    uint64_t jobs_total, jobs_run;         /* stream jobs over the sorted records */
    uint64_t runs_total, runs_run;         /* window runs of stream chunks */
    uint64_t slices_total, slices_run;     /* tiles of the slices' first-block records */
    uint64_t tiles_total, tiles_run;       /* second-level tiles with both lists non-empty */
    double   k0_ms, k1n_ms, k1g_ms, k2_ms, kernel_ms;   /* the stage times of kmdb_stats for this call */
    uint64_t peak_device_bytes;    /* kmdb_stats.device_bytes after the call + the band's bytes */
} kmdb_all2all_rows_records_stats;
int  kmdb_all2all_rows_records_device(kmdb_db* db, uint64_t row_lo, uint64_t row_hi, void* out_cells_dev, const kmdb_opts* opts);
int  kmdb_all2all_rows_records(kmdb_db* db, uint64_t row_lo, uint64_t row_hi, uint32_t* out_cells_host, const kmdb_opts* opts);
int  kmdb_all2all_rows_records_stats_get(const kmdb_db* db, kmdb_all2all_rows_records_stats* out);
/* kmdb_all2all_sparse_filtered_banded with the band call chosen: KMDB_BAND_PATH_TILED is that call itself, _TREE takes kmdb_all2all_rows_device,
 * _RECORDS kmdb_all2all_rows_records_device.  Same DEFINITION, same refusals (and an unknown path); kmdb_all2all_banded_stats is filled by every
 * path (its hit / run / update sums by _TILED only), the records path's own sums are in kmdb_all2all_banded_records_stats. */
#define KMDB_BAND_PATH_TILED   0
#define KMDB_BAND_PATH_TREE    1
#define KMDB_BAND_PATH_RECORDS 2
typedef struct kmdb_all2all_banded_records_stats {   /* the LAST banded call with KMDB_BAND_PATH_RECORDS on the handle */
    uint64_t bands;
    uint64_t units_total, units_run;   /* sums over the bands of kmdb_all2all_rows_records_stats */
    double   ms;                       /* sum of the bands' kernel_ms */
} kmdb_all2all_banded_records_stats;
int  kmdb_all2all_sparse_filtered_banded_path(kmdb_db* db, uint64_t band_rows, int path, const kmdb_cell_filter* filters, size_t n_filters,
                                              const uint32_t* sample_kmers, int measure, kmdb_sparse_rows* out, const kmdb_opts* opts);
int  kmdb_all2all_banded_records_stats_get(const kmdb_db* db, kmdb_all2all_banded_records_stats* out);
/* Band emit (KMDB_HAS_ALL2ALL_BAND_EMIT; a2a_blocks.hip): the second form of the records band call, additive in ABI 8.  The emit kernels write the block
 * records of the band's block rows Xlo .. Xhi alone — a record (X, Y) outside them never exists — keyed RELATIVE to the band: tri32(X) - tri32(Xlo) + Y,
 * tri32(x) = x (x + 1) / 2, with n_streams = tri32(Xhi + 1) - tri32(Xlo) keys; the sorts, the stream jobs and the second-level tiles run over the band's
 * streams, every array indexed by block row holds Xhi - Xlo + 1 rows.  The call runs on a state of its own per handle, made at the first such call and
 * made anew when a later band needs more streams or rows; its pools follow the band's share of the estimate.  The whole-matrix state is not touched:
 * whole calls before and after give the same matrix and the same counts in kmdb_stats; kmdb_stats.device_bytes counts both states.
 * Same DEFINITION, refusals and output rule as above.  Which form kmdb_all2all_rows_records[_device] takes — KMDB_BAND_EMIT, read at the handle's first
 * records band call: unset — band emit only where the whole-matrix pipeline refused the database for "too many block pairs" and nothing else (everywhere
 * else the call above, with its records, units and stats); 1 — every records band call the pipeline can take; 0 — never.
 * A band is refused by band emit when its n_streams + 1 >= min(2^22, KMDB_BAND_MAX_STREAMS) (a test switch) or when the wide kernel's lists — as many
 * entries as the collection has blocks — do not fit the LDS: the band then comes from kmdb_all2all_rows_device (path = TREE), with
 * KMDB_FLAG_NO_FALLBACK the call fails with a message that names the streams or the bytes.  kmdb_db_fallback_reason stays the whole matrix's.
 * Limits: a band of fewer than 2^22 streams (at 9 375 blocks, 300 000 samples at width 32, that is some 440 block rows: 14 000 rows per band) and a
 * collection whose blocks the wide kernel's lists hold in LDS: some 7 500 blocks, 240 000 samples at width 32, 480 000 at width 64.  Beyond either the
 * two tree forms above are the only route. */
#define KMDB_HAS_ALL2ALL_BAND_EMIT 1
#define KMDB_BAND_EMIT_FORM_NONE   0u   /* an empty band, a tree fallback or a failed call: no records path ran */
#define KMDB_BAND_EMIT_FORM_WHOLE  1u   /* decode, emit and the sorts ran whole, the apply stage culled (the call above) */
#define KMDB_BAND_EMIT_FORM_BAND   2u   /* band emit */
typedef struct kmdb_band_geometry {
    uint32_t x_lo, x_hi;           /* block rows the band meets: row_lo / width, (row_hi - 1) / width; 0, 0 for an empty band */
    uint32_t n_rows;               /* x_hi - x_lo + 1; 0 for an empty band */
    uint32_t fits;                 /* 1: n_streams + 1 < 2^22 */
    uint64_t n_streams;            /* tri32(x_hi + 1) - tri32(x_lo); 0 for an empty band */
    uint64_t stream_base;          /* tri32(x_lo) */
} kmdb_band_geometry;
/* host only, no GPU: the geometry of the band [row_lo, row_hi) of n_samples samples at block width `width` — the function the library itself calls.
 * Refused with a message: a null out, a width outside 32 .. 64, row_lo > row_hi, row_hi > n_samples. */
int  kmdbh_band_streams(uint64_t n_samples, uint32_t width, uint64_t row_lo, uint64_t row_hi, kmdb_band_geometry* out);
typedef struct kmdb_all2all_rows_band_emit_stats {   /* the LAST records band call on the handle */
    uint32_t form;                 /* KMDB_BAND_EMIT_FORM_* */
    uint32_t x_lo, x_hi, n_rows;   /* kmdb_band_geometry of the band at the handle's width */
    uint32_t key_bits;             /* stream bits of a key word: the band's under band emit, the whole matrix's otherwise */
    uint32_t row_mode;             /* 1: the many-streams record path */
    uint32_t l2_on;                /* 1: the second level is on */
    uint32_t attempts;             /* 1 + the repeats of the call (pools enlarged, launches sized anew) */
    uint64_t n_streams, stream_base;
    uint64_t records;              /* block records emitted: the band's under band emit */
    uint64_t est_records;          /* the estimate the state's pools were sized from */
    uint64_t state_bytes;          /* device bytes of the band-emit state (0: the handle has none) */
    uint64_t whole_state_bytes;    /* device bytes of the whole-matrix state, 0 where none exists */
} kmdb_all2all_rows_band_emit_stats;
int  kmdb_all2all_rows_band_emit_stats_get(const kmdb_db* db, kmdb_all2all_rows_band_emit_stats* out);
/* ---------------------------------------------------------------------------------------
 * all2all-sp -sample-rows <criterion>:<count> (params.cpp:533-557): every sample keeps its `count` best neighbours.  A pair (i, j), i > j, with
 * a non-zero cell that passes the filters has ONE score, metric(cell, kmers[i], kmers[j], k) with the triangle's row i as the row sample, and is
 * offered to sample i AND to sample j (SparseMatrix::add_to_sampler, array.h:450-540); a sample keeps the `count` best by score descending, then
 * sample id ascending (the heap order of sampler.h:45-50).  The device selects candidates on the criterion's plain ratio, widened by the margin
 * of the filters, so that neither the sparse matrix nor anything proportional to its non-zeros reaches the host; the host decides the candidates
 * with kmdbh_metric.  Rows the margin cannot settle are fetched again whole inside the call: the result is always what the reference's Sampler keeps.
 * ------------------------------------------------------------------------------------- */
typedef struct kmdb_sample_stats { /* the LAST sampled call on the handle */
    uint64_t candidates;           /* cells the device emitted (after re-fetches) */
    uint64_t rows_truncated;       /* rows cut at their count-th best proxy less the margin with cells left below the cut */
    uint64_t rows_refetched;       /* rows of `count` candidates or more that a filter bound inside the margin left undecided: fetched again whole */
    uint64_t d2h_bytes;            /* bytes copied back: row pointers, 8 per candidate, one counter */
    double   select_ms;            /* HIP events around the selection passes (kmdb_stats.kernel_ms holds the whole call) */
    uint32_t triangle_reads;       /* passes over the (touched tiles of the) triangle: 4 histogram, 1 count, 1 emit; 2 more for a re-fetch */
    uint32_t reserved;
} kmdb_sample_stats;
/* Replaces all2all_sp + add_to_sampler + Sampler::saveRowSparse (console_all2all_sparse.cpp:44,70-89; array.h:450-540; sampler.h): accumulate,
 * candidates, exact decision and re-fetch inside the call.  out: row s = the kept neighbours of sample s in ascending id, val = common k-mers,
 * measure = the score.  criterion: KMDB_METRIC_*; count >= 1; sample_kmers as in kmdb_all2all_sparse_filtered (required: every criterion but
 * num-kmers needs it).  Refused with kmdb_opts.shard_count > 1, like the filtered call. */
int  kmdb_all2all_sampled(kmdb_db* db, const kmdb_cell_filter* filters, size_t n_filters, const uint32_t* sample_kmers, int criterion,
                          uint32_t count, kmdb_sparse_rows* out, const kmdb_opts* opts);
/* The candidates of a flat cell range the CALLER accumulated (cells_dev, cell_lo, cell_hi and the stream note as in kmdb_sparse_from_dense_device):
 * the multi-GPU form of console_all2all_sparse.cpp:70-89.  out_candidates: symmetric rows, ascending columns, val = common k-mers, no measures —
 * per sample a superset of its `count` best cells among the cells of the range (exact filters included: the re-fetch happens here).  A sample's
 * best `count` within a range is a superset of its share of the global best `count`, so the candidates of several ranges go to
 * kmdbh_sample_rows_select together. */
int  kmdb_sampled_from_dense_device(kmdb_db* db, const void* cells_dev, uint64_t cell_lo, uint64_t cell_hi, const kmdb_cell_filter* filters,
                                    size_t n_filters, const uint32_t* sample_kmers, int criterion, uint32_t count,
                                    kmdb_sparse_rows* out_candidates, const kmdb_opts* opts);
int  kmdb_db_sample_stats(const kmdb_db* db, kmdb_sample_stats* out);
/* The exact decision (Sampler with strategy best, sampler.h:44-67,123-139; no GPU): any number of candidate parts of the same collection — rows of
 * (col, val) — in, per sample the `count` best cells that pass the filters out, ascending id, val = common k-mers, measure = score.  Does not depend
 * on the order of the candidates within or across parts; a pair listed twice counts once. */
int  kmdbh_sample_rows_select(int criterion, uint32_t count, int kmer_length, const uint32_t* sample_kmers, const kmdb_cell_filter* filters,
                              size_t n_filters, const kmdb_sparse_rows* const* parts, size_t n_parts, kmdb_sparse_rows* out);
/* the measure itself (params.cpp:14-42): uint32 wrap-around integer parts, double arithmetic */
double kmdbh_metric(int metric, uint32_t common, uint32_t cnt_row, uint32_t cnt_col, int kmer_length);
/* KMDB_METRIC_* of a criterion name ("jaccard", "min", ..., "num-kmers"), -1 if unknown */
int    kmdbh_metric_id(const char* name);

/* Replaces T concurrent calls of SimilarityCalculator::one2all<false>
 * (similarity_calculator.cpp:809-925; call site console_new2all.cpp:82): nq queries, each a
 * sorted, duplicate-free k-mer array (KmerHelper::unique, console_new2all.cpp:73).
 * out_dense: nq x N uint32 in host memory, row q = similarities of query q. */
int  kmdb_new2all_batch(kmdb_db* db, const uint64_t* const* kmers, const size_t* counts, size_t nq,
                        uint32_t* out_dense, const kmdb_opts* opts);
/* Replaces one2all_sp (similarity_calculator.cpp:929-1051; call site console_new2all.cpp:78):
 * row q = ascending (sample_id, count) pairs with count > 0.  = kmdb_new2all_batch_sparse_filtered without bounds: the rows are compacted
 * on the device, neither the nq x N rectangle nor its zeros cross PCIe.  (Also serves a query shard: its partial rows.) */
int  kmdb_new2all_batch_sparse(kmdb_db* db, const uint64_t* const* kmers, const size_t* counts, size_t nq,
                               kmdb_sparse_rows* out, const kmdb_opts* opts);
/* The same with the query-side loader on the device: replaces, per query, the k-mer extraction of
 * GenomeInputFile::load / KmerHelper (kmer_extract.h:13-118), the minhash filter (filter.h:28-115) and
 * KmerHelper::unique (console_new2all.cpp:73) followed by one2all<false>.  seqs[q] = the query's sequence text
 * (ASCII, records of one sample joined by any non-ACGTU symbol, e.g. '\n'); fraction / start_fraction /
 * preserve_strand are the database's filter settings (kmdbh_db_fraction, kmdbh_db_start_fraction,
 * kmdbh_db_alphabet == 1).  out_kmer_counts[q] = number of unique k-mers of query q (the CSV's total-kmers). */
int  kmdb_new2all_batch_seq(kmdb_db* db, const char* const* seqs, const size_t* seq_lens, size_t nq, double fraction,
                            double start_fraction, int preserve_strand, uint32_t* out_dense, uint64_t* out_kmer_counts,
                            const kmdb_opts* opts);
/* The same for a database over any of the reference's alphabets (ABI 7; alphabet.h:79-126, kmer_extract.h:13-97): `alphabet` =
 * kmdbh_db_alphabet (KMDB_ALPHABET_*), e.g. protein queries against the databases of test/protein.  Records of one sample are
 * joined by any byte that is not a symbol of the alphabet ('\n'). */
int  kmdb_new2all_batch_seq_alphabet(kmdb_db* db, const char* const* seqs, const size_t* seq_lens, size_t nq, double fraction,
                                     double start_fraction, int32_t alphabet, uint32_t* out_dense, uint64_t* out_kmer_counts,
                                     const kmdb_opts* opts);

/* kmdb_new2all_batch / kmdb_new2all_batch_seq_alphabet with the rows left on the device: they are ADDED (uint32) into out_dev, a
 * caller-owned, caller-zeroed nq x N uint32 buffer in DEVICE memory, on opts->stream (the handle's own stream when NULL) — what the
 * query shards of one database on one device, and the devices of a node before their reduce, accumulate into (the multi-GPU form of
 * console_new2all.cpp:78,82 and console_one2all.cpp).  Any handle with tables serves them, not only query shards.  The calls return
 * when their last kernel has ended.  On a query-shard handle out_kmer_counts[q] counts the unique k-mers of the shard's own buckets. */
int  kmdb_new2all_batch_device(kmdb_db* db, const uint64_t* const* kmers, const size_t* counts, size_t nq, void* out_dev,
                               const kmdb_opts* opts);
int  kmdb_new2all_batch_seq_alphabet_device(kmdb_db* db, const char* const* seqs, const size_t* seq_lens, size_t nq, double fraction,
                                            double start_fraction, int32_t alphabet, void* out_dev, uint64_t* out_kmer_counts,
                                            const kmdb_opts* opts);

/* Replaces one2all_sp FOLLOWED BY the CombinedFilter of the query's row, which is how the reference writes `new2all -sparse` (console_new2all.cpp:76-78:
 * one2all_sp per query; :130-148: the row's cells through CombinedFilter(metrics, queryKmersCounts, db.getSampleKmersCount(), kmerLength)).  The rows
 * of the batch are accumulated in HBM as for kmdb_new2all_batch_device and compacted there: one wave per segment of 2048 columns of a row, the
 * bounds — widened by a safety margin, as in kmdb_all2all_sparse_filtered — applied before anything leaves the device, the remaining cells decided on
 * the host with kmdbh_metric.  Only the row pointers and 8 bytes per device-kept cell cross PCIe; the call holds the whole batch's nq x N x 4 bytes
 * on the device.
 * out: n_rows = nq; row q lists (col, val) with val > 0, 0 <= col < n_samples, ascending col.
 * In every measure a = the QUERY's k-mer count — counts[q], its number of unique k-mers, truncated to uint32 like the reference's num_kmers_t —
 * and b = sample_kmers[col], the database sample's: the order of the reference's CombinedFilter; mash-query tells the two apart.
 * measure >= 0 fills out->measure per kept cell (kmdbh_metric), -1 leaves it NULL.  n_filters == 0 with measure < 0 keeps every non-zero cell and
 * allows a NULL sample_kmers; filters or a measure need it.
 * Refused before any device work, under the entry point's name: a NULL handle or out, filters or a measure without sample_kmers, an unknown metric or
 * measure, more than 12 bounds, a handle without hashtables, and a QUERY SHARD handle (kmdb_db_upload_query_shard): its cells are partial sums and
 * so are its counts — sum the shards' rows (kmdb_new2all_batch_device) and compact them with kmdb_new2all_rows_sparse_device, or use the node entry. */
int  kmdb_new2all_batch_sparse_filtered(kmdb_db* db, const uint64_t* const* kmers, const size_t* counts, size_t nq, const kmdb_cell_filter* filters,
                                        size_t n_filters, const uint32_t* sample_kmers /* [N] */, int measure /* KMDB_METRIC_* or -1 */,
                                        kmdb_sparse_rows* out, const kmdb_opts* opts);
/* The same with the query-side loader on the device (kmdb_new2all_batch_seq_alphabet): a = out_kmer_counts[q], the device extractor's unique count. */
int  kmdb_new2all_batch_seq_alphabet_sparse_filtered(kmdb_db* db, const char* const* seqs, const size_t* seq_lens, size_t nq, double fraction,
                                                     double start_fraction, int32_t alphabet, const kmdb_cell_filter* filters, size_t n_filters,
                                                     const uint32_t* sample_kmers /* [N] */, int measure, kmdb_sparse_rows* out,
                                                     uint64_t* out_kmer_counts, const kmdb_opts* opts);
/* The compaction alone, on rows the CALLER accumulated (kmdb_new2all_batch*_device, the sum over query shards, a rank's chunk after a reduce-scatter):
 * the flat range [cell_lo, cell_hi) of the row-major nq x N rectangle, cell q * N + s = query q, sample s; rows_dev points at cell `cell_lo`, as
 * cells_dev of kmdb_sparse_from_dense_device does (the whole batch is {0, nq * N}).  out has all nq rows; rows outside the range are empty and a row
 * cut by a range end lists only its cells inside, so the outputs of consecutive ranges concatenate row by row (ascending columns).
 * query_kmers: [nq] uint32 in host memory, needed with filters or a measure.  The cells are complete sums here, so any handle of the database serves,
 * a query shard included.  Also refused: cell_lo > cell_hi, cell_hi > nq * N.  The stream note of kmdb_sparse_from_dense_device applies: the call
 * reads rows_dev on opts->stream (the handle's own when NULL) and does not order itself after the caller's producer. */
int  kmdb_new2all_rows_sparse_device(kmdb_db* db, const void* rows_dev, size_t nq, uint64_t cell_lo, uint64_t cell_hi,
                                     const uint32_t* query_kmers /* [nq], host */, const kmdb_cell_filter* filters, size_t n_filters,
                                     const uint32_t* sample_kmers /* [N] */, int measure, kmdb_sparse_rows* out, const kmdb_opts* opts);
typedef struct kmdb_new2all_sparse_stats {   /* the LAST sparse new2all call on the handle / the node */
    uint64_t cells;                /* cells in the compacted range (node: summed over the devices) */
    uint64_t nnz_device;           /* cells that passed the widened bounds and left HBM */
    uint64_t nnz;                  /* cells returned after the exact decision on the host */
    uint64_t d2h_bytes;            /* result bytes copied to the host: 8 (nq + 1) + 8 nnz_device per compaction */
    double   compact_ms;           /* HIP events around count + scan + compact (node: the slowest device) */
} kmdb_new2all_sparse_stats;
int  kmdb_new2all_sparse_stats_get(const kmdb_db* db, kmdb_new2all_sparse_stats* out);

/* ---------------------------------------------------------------------------------------
 * new2all -sample-rows <criterion>:<count>: a search.  Every QUERY keeps its `count` best database samples; the database samples collect nothing.
 * The reference has no such option for new2all; the rule is the one its Sampler applies to a sparse row everywhere else (sampler.h:44-67) over the
 * row new2all -sparse writes (console_new2all.cpp:130-148).  For query q with a = its own unique k-mer count truncated to uint32 and database
 * sample s with b = sample_kmers[s]: the cell c = rows[q][s] is a candidate when c > 0 and it passes every bound (a = the QUERY's count, b = the
 * sample's, as in kmdb_new2all_batch_sparse_filtered); its score is kmdbh_metric(criterion, c, a, b, k); row q keeps the `count` candidates with
 * the largest score, ties towards the smaller sample id, listed in ascending sample id; a row of fewer candidates comes out whole.
 * The device selects on the criterion's plain ratio by the radix select of kmdb_all2all_sampled, here over per-row segments of 2048 columns, a
 * wave each; the host decides with kmdbh_metric; rows the margin cannot settle are fetched again whole inside the call.
 * ------------------------------------------------------------------------------------- */
/* Stands for T calls of one2all_sp + CombinedFilter (console_new2all.cpp:76-78, 130-148) followed by Sampler::saveRowSparse (sampler.h:123-139):
 * the rows accumulated in HBM as for kmdb_new2all_batch_device, then selection, exact decision and re-fetch inside the call.  out: row q = the
 * kept samples of query q in ascending id, val = common k-mers, measure = the score (as kmdb_all2all_sampled gives it).  criterion:
 * KMDB_METRIC_*; count >= 1; sample_kmers [N] is required.  Needs the hashtables; a query-shard handle is refused, as
 * kmdb_new2all_batch_sparse_filtered refuses it. */
int  kmdb_new2all_batch_sampled(kmdb_db* db, const uint64_t* const* kmers, const size_t* counts, size_t nq, const kmdb_cell_filter* filters,
                                size_t n_filters, const uint32_t* sample_kmers /* [N] */, int criterion, uint32_t count, kmdb_sparse_rows* out,
                                const kmdb_opts* opts);
/* The same with the queries given as sequence text (the second call site of a batch, console_new2all.cpp:60-75 with the device extractor);
 * out_kmer_counts [nq]: the unique k-mer count of every query, whose low 32 bits are a. */
int  kmdb_new2all_batch_seq_alphabet_sampled(kmdb_db* db, const char* const* seqs, const size_t* seq_lens, size_t nq, double fraction,
                                             double start_fraction, int32_t alphabet, const kmdb_cell_filter* filters, size_t n_filters,
                                             const uint32_t* sample_kmers /* [N] */, int criterion, uint32_t count, kmdb_sparse_rows* out,
                                             uint64_t* out_kmer_counts, const kmdb_opts* opts);
/* The candidates of a flat range [cell_lo, cell_hi) of a row-major nq x n_cols rectangle of query rows the CALLER accumulated (the multi-GPU form
 * of the call site above: a device's reduce-scatter chunk as it is; rows_dev = device address of cell cell_lo, as in
 * kmdb_new2all_rows_sparse_device).  db gives the device, the stream and the k-mer length, as in kmdb_sampled_from_rect_device; n_cols is
 * explicit (1 .. 2^32 - 1) and need not be the handle's sample count.  query_kmers [nq] and sample_kmers [n_cols] are host arrays.
 * out_candidates: all nq rows, ascending sample ids, val = common k-mers, no measures; rows outside the range are empty and a row cut by a range
 * end lists only its cells inside.  Per row a superset of its `count` best cells among the cells of the range (exact filters included: the
 * re-fetch happens here); a row's best `count` within a range is a superset of its share of the global best `count`, so the candidates of
 * several ranges go to kmdbh_query_rows_select together.  The stream note of kmdb_sparse_from_dense_device applies. */
int  kmdb_sampled_from_rows_device(kmdb_db* db, const void* rows_dev, size_t nq, uint64_t n_cols, uint64_t cell_lo, uint64_t cell_hi,
                                   const uint32_t* query_kmers /* [nq] */, const kmdb_cell_filter* filters, size_t n_filters,
                                   const uint32_t* sample_kmers /* [n_cols] */, int criterion, uint32_t count, kmdb_sparse_rows* out_candidates,
                                   const kmdb_opts* opts);
/* The exact one-sided decision (Sampler with strategy best, sampler.h:44-67, 123-139; no GPU): any number of candidate parts of nq rows each in,
 * per query the `count` best cells that pass the filters out — ascending id, val = common k-mers, measure = score.  Does not depend on the order
 * of the candidates within or across parts; a pair listed twice counts once.  Every candidate's column must be an index into sample_kmers. */
int  kmdbh_query_rows_select(int criterion, uint32_t count, int kmer_length, const uint32_t* query_kmers /* [nq] */, size_t nq,
                             const uint32_t* sample_kmers, const kmdb_cell_filter* filters, size_t n_filters, const kmdb_sparse_rows* const* parts,
                             size_t n_parts, kmdb_sparse_rows* out);
/* The LAST sampled new2all call on the handle (or kmdb_sampled_from_rows_device call on it): the fields of kmdb_sample_stats over the rows that
 * meet the range; triangle_reads = passes over the rows: 4 histogram, 1 count, 1 emit; 2 more for a re-fetch.  d2h_bytes: 8 per row that meets
 * the range plus 8, 8 per candidate, one counter — the working arrays are sized by those rows, not by nq. */
int  kmdb_new2all_sample_stats_get(const kmdb_db* db, kmdb_sample_stats* out);

/* Replaces SimilarityCalculator::db2db_sp(db_row, db_col, SparseMatrix&, bubbles) (similarity_calculator.cpp:1225-1540),
 * the off-diagonal cell of the all2all-parts grid (call sites console_all2all_parts.cpp:180,226): both databases
 * resident with hashtables on the same device.  out: n_samples(db_row) x n_samples(db_col) uint32, row-major, host
 * memory: out[r][c] = number of k-mers shared by sample r of db_row and sample c of db_col.
 * The first call on a handle of up to 4096 samples leaves the full sample lists of its patterns with the handle (n_samples / 8
 * bytes per pattern, at most 8 GB; counted in kmdb_stats.device_bytes, freed by kmdb_db_free): the other cells of the grid that
 * use the part read them instead of rebuilding them. */
int  kmdb_db2db_dense(kmdb_db* db_row, kmdb_db* db_col, uint32_t* out, const kmdb_opts* opts);
/* Replaces db2db_sp FOLLOWED BY SparseMatrix::compact2 with the -min / -max CombinedFilter, which is how the reference keeps a cell of the
 * all2all-parts grid (console_all2all_parts.cpp:179-195 and 225-241: db2db_sp at :180 / :226, compact2(filter) right after it; array.h:391-446,
 * sparse_filters.h:38-61).  The cell is accumulated in HBM as for kmdb_db2db_dense and compacted there: only the 64 x 64 tiles that received a
 * contribution are read, the bounds — widened by a safety margin, as in kmdb_all2all_sparse_filtered — are applied before anything leaves the
 * device, and the remaining cells are decided on the host with kmdbh_metric.  Neither the nr x nc rectangle nor its zeros cross PCIe.
 * out: n_rows = n_samples(db_row); row r lists (col, val) with val > 0, 0 <= col < n_samples(db_col), ascending col — the content of the
 * reference's SparseMatrix after db2db_sp + compact2(filter).
 * In every measure a = row_sample_kmers[r], the ROW sample's k-mer count, and b = col_sample_kmers[col], the COLUMN sample's — the order of
 * CombinedFilter(..., db_row->getSampleKmersCount(), db_col->getSampleKmersCount(), ...); mash-query tells the two apart.
 * measure >= 0 fills out->measure per kept cell (kmdbh_metric), -1 leaves it NULL.  n_filters == 0 with measure < 0 keeps every non-zero cell and
 * allows NULL count arrays; filters or a measure need both.  db_row == db_col is allowed: the full square, diagonal included, as the dense call.
 * Refused before any device work: NULL handles / out, filters or a measure without both count arrays, an unknown metric or measure, more than
 * 12 bounds; and everything kmdb_db2db_dense refuses (no hashtables, a query shard, different k-mer lengths or devices, its size limits).
 * KMDB_SP_ALL_TILES=1 reads every tile (A/B), as for all2all-sp. */
int  kmdb_db2db_sparse_filtered(kmdb_db* db_row, kmdb_db* db_col, const kmdb_cell_filter* filters, size_t n_filters,
                                const uint32_t* row_sample_kmers /* [nr] */, const uint32_t* col_sample_kmers /* [nc] */,
                                int measure /* KMDB_METRIC_* or -1 */, kmdb_sparse_rows* out, const kmdb_opts* opts);
typedef struct kmdb_db2db_stats {  /* the LAST kmdb_db2db_* call with this handle as the ROW database */
    uint64_t tiles;                /* ceil(nr / 64) * ceil(nc / 64) */
    uint64_t tiles_touched;        /* tiles that received a block record = tiles the compaction read (0 after a dense call) */
    uint64_t nnz_device;           /* cells that passed the widened bounds and left HBM */
    uint64_t nnz;                  /* cells returned after the exact decision on the host */
    uint64_t d2h_bytes;            /* result bytes copied to the host: row pointers + 8 per device-kept cell (dense call: 4 nr nc) */
    double   compact_ms;           /* HIP events around flags + count + scan + compact (kmdb_stats.kernel_ms holds the whole call) */
} kmdb_db2db_stats;
int  kmdb_db2db_stats_get(const kmdb_db* db_row, kmdb_db2db_stats* out);
/* Replaces db2db_sp + SparseMatrix::compact2(filter) + SparseMatrix::add_to_sampler for an off-diagonal cell of the all2all-parts grid under
 * -sample-rows <criterion>:<count> (console_all2all_parts.cpp:179-195 and 225-241: db2db_sp at :180 / :226, compact2(filter) and add_to_sampler
 * right after it; array.h:391-446, 450-540; sampler.h).  The cell is accumulated in HBM as for kmdb_db2db_dense, its tile flags are made as for
 * kmdb_db2db_sparse_filtered (KMDB_SP_ALL_TILES=1 reads every tile), and the radix select of kmdb_all2all_sampled runs on the flagged tiles of the
 * rectangle: neither the cell nor anything proportional to its non-zeros reaches the host.
 * A pair (r, c) has ONE score, with a = row_sample_kmers[r], the ROW sample's k-mer count, and b = col_sample_kmers[c], the COLUMN sample's, and
 * is offered to row sample r and to column sample c (mash-query tells the two apart; the bounds use the same a and b).
 * out_row_candidates: n_samples(db_row) rows, cols local to db_col; out_col_candidates: n_samples(db_col) rows, cols local to db_row.  Both as
 * kmdb_sampled_from_dense_device gives them: ascending columns, val = common k-mers, no measures — per sample a superset of its `count` best
 * cells of this cell by the exact decision, filters included (rows the margin cannot settle are fetched again whole inside the call).  A sample's
 * best `count` within a cell is a superset of its share of the global best `count`, so the candidates of all cells of a grid — with their local
 * ids shifted to global ones — go to kmdbh_sample_rows_select, or to any exact sampler, together.
 * Refused before any device work: NULL handles / outs, count 0, an unknown criterion, a missing count array (both are required), an unknown
 * metric in a filter, more than 12 bounds; everything kmdb_db2db_dense refuses (no hashtables, a query shard, different k-mer lengths or
 * devices, its size limits); and 2^31 - 2 samples in the two sets or 2^31 tiles of 64 x 64 cells, the select's 31-bit sizes. */
int  kmdb_db2db_sampled(kmdb_db* db_row, kmdb_db* db_col, const kmdb_cell_filter* filters, size_t n_filters,
                        const uint32_t* row_sample_kmers /* [nr] */, const uint32_t* col_sample_kmers /* [nc] */, int criterion, uint32_t count,
                        kmdb_sparse_rows* out_row_candidates, kmdb_sparse_rows* out_col_candidates, const kmdb_opts* opts);
/* The same on a rectangle the CALLER accumulated: cells_dev = nr x nc uint32 in device memory, row-major (cell (r, c) at r * nc + c), every tile
 * read.  db gives the device, the stream and the k-mer length, as in kmdb_sampled_from_dense_device, and the stream note of
 * kmdb_sparse_from_dense_device applies: the cells must be complete on opts->stream (the handle's own when NULL) before the call. */
int  kmdb_sampled_from_rect_device(kmdb_db* db, const void* cells_dev, uint64_t nr, uint64_t nc, const kmdb_cell_filter* filters, size_t n_filters,
                                   const uint32_t* row_sample_kmers, const uint32_t* col_sample_kmers, int criterion, uint32_t count,
                                   kmdb_sparse_rows* out_row_candidates, kmdb_sparse_rows* out_col_candidates, const kmdb_opts* opts);
/* The LAST kmdb_db2db_sampled call with this handle as the ROW database (or kmdb_sampled_from_rect_device call on it): the fields of
 * kmdb_sample_stats over the nr + nc lines of the cell — candidates of both outputs, rows truncated / re-fetched on either side, triangle_reads =
 * passes over the cell's touched tiles.  The tile counts of that call are in kmdb_db2db_stats_get (tiles, tiles_touched). */
int  kmdb_db2db_sample_stats_get(const kmdb_db* db_row, kmdb_sample_stats* out);

/* ---------------------------------------------------------------------------------------
 * One database over the GPUs of a node (north_star: prefix buckets sharded across the GPUs, one RCCL reduce of the
 * partial matrices over xGMI).  Makes the reference's single call sites multi-GPU: SimilarityCalculator::all2all at
 * console_all2all.cpp:31-36 and all2all_sp + compact2 at console_all2all_sparse.cpp:44,79.
 * kmdb_node_upload: shard s of n_shards (kmdb_db_upload_shard: the k-mers of the prefix buckets b with b % n_shards == s) goes to
 * devices[s % D], D = min(n_shards, n_devices); the view must carry the hashtables when n_shards > 1.  One host thread per
 * device inside every call; several shards of one device run one after the other and are summed on the device (a one-GPU box
 * takes any n_shards that way).  With D > 1 the partial matrices meet in ONE ncclReduceScatter (uint32 sum) over flat chunks of the
 * lower triangle — xGMI is point to point, every peer pair sums its chunk over its own link — and every device brings its own
 * chunk to the host (dense) or compacts it where it is (sparse); librccl.so is loaded with dlopen only then.
 * ------------------------------------------------------------------------------------- */
typedef struct kmdb_node kmdb_node;
typedef struct kmdb_node_stats {   /* the LAST call on the node handle; maxima over the devices */
    uint32_t n_shards, n_devices;
    int32_t  rccl_version;         /* ncclGetVersion, 0 when RCCL was not needed */
    uint32_t partition;            /* KMDB_PARTITION_* of the upload (ABI 8; the field was reserved, 0 = prefix buckets, before) */
    double   upload_s;             /* kmdb_node_upload[_partition], wall clock */
    double   plan_s;               /* of it: the host's plan of all shards (prefix: one pass over the hashtable items, one sweep over the tree;
                                      ranges: two sweeps over parent_id and num_samples) */
    double   call_ms;              /* HIP events around the slowest device's kmdb_all2all_dense_device calls (all its shards) */
    double   collective_ms;        /* HIP events around ncclReduceScatter on the slowest device */
    double   d2h_ms;               /* dense: copy of the device's chunk to the host; sparse: compaction + copy of its CSR */
} kmdb_node_stats;
/* One device slot of the node (slot < kmdb_node_stats.n_devices): what THAT device did — an imbalanced shard shows here, not in the maxima */
typedef struct kmdb_node_device_stats {
    int32_t  device;               /* HIP device of the slot */
    uint32_t n_shards;             /* shards that live on it */
    double   upload_s;             /* its thread's share of kmdb_node_upload */
    double   call_ms;              /* HIP events around its own shards' all2all calls (last call) */
    double   collective_ms;        /* ... around its ncclReduceScatter (0 without RCCL) */
    double   d2h_ms;               /* ... around the copy of its chunk / the compaction of its chunk */
    uint64_t h2d_bytes;            /* bytes its uploads sent over PCIe (sum over its shards) */
    uint64_t n_patterns;           /* nodes resident on it (sum over its shards: a prefix shard keeps only the nodes it needs) */
    uint64_t n_records;            /* block records of its shards in the last call */
} kmdb_node_device_stats;
int  kmdb_node_device_stats_get(const kmdb_node* node, uint32_t slot, kmdb_node_device_stats* out);
int  kmdb_node_upload(const kmdb_db_view* view, uint32_t n_shards, const int32_t* devices, uint32_t n_devices, kmdb_node** out);
/* The same with the partition named (ABI 8; kmdb_node_upload = KMDB_PARTITION_PREFIX).  KMDB_PARTITION_RANGE: shard s is tree range s of
 * n_shards (kmdb_db_upload_range; one plan for all of them), again on devices[s % D] — the partition of all2all / all2all-sp as the
 * reference loads them (console_all2all.cpp:26,31-36: SkipHashtables): the view needs no hashtables, and the devices together hold
 * P + sum over the ranges of (depth of the first node - 1) nodes instead of a near-whole tree per prefix shard.  Everything after the
 * upload (own shards summed on the device, reduce-scatter, dense copy / sparse compaction) is the same for both. */
#define KMDB_PARTITION_PREFIX 0
#define KMDB_PARTITION_RANGE  1
/* KMDB_PARTITION_PREFIX_TABLES: shard s is QUERY shard s of n_shards (kmdb_db_upload_query_shard: the prefix shard's pruned tree and the
 * slots of its own buckets), on devices[s % D] — the partition of new2all / one2all (console_new2all.cpp:64-95, console_one2all.cpp); the
 * view must carry the hashtables.  all2all / all2all-sp work on such a node as on a prefix node; kmdb_node_new2all_* need it. */
#define KMDB_PARTITION_PREFIX_TABLES 2
int  kmdb_node_upload_partition(const kmdb_db_view* view, uint32_t n_shards, const int32_t* devices, uint32_t n_devices, int partition,
                                kmdb_node** out);
void kmdb_node_free(kmdb_node* node);
int  kmdb_node_stats_get(const kmdb_node* node, kmdb_node_stats* out);
/* = kmdb_all2all_dense over all shards: out_lower_tri N(N-1)/2 uint32 in host memory */
int  kmdb_node_all2all_dense(kmdb_node* node, uint32_t* out_lower_tri, const kmdb_opts* opts);
/* = kmdb_all2all_sparse_filtered over all shards (filters / measure on the complete sums; n_filters 0 and measure -1: plain
 * kmdb_all2all_sparse); rows concatenate over the devices' chunks in ascending column order */
int  kmdb_node_all2all_sparse(kmdb_node* node, const kmdb_cell_filter* filters, size_t n_filters, const uint32_t* sample_kmers, int measure,
                              kmdb_sparse_rows* out, const kmdb_opts* opts);
/* = kmdb_all2all_sampled over all shards, any partition (console_all2all_sparse.cpp:70-89 over the GPUs of a node): every device selects the
 * candidates of its reduce-scatter chunk (kmdb_sampled_from_dense_device), the host decides once (kmdbh_sample_rows_select). */
int  kmdb_node_all2all_sampled(kmdb_node* node, const kmdb_cell_filter* filters, size_t n_filters, const uint32_t* sample_kmers, int criterion,
                               uint32_t count, kmdb_sparse_rows* out, const kmdb_opts* opts);
/* = kmdb_new2all_batch / _seq_alphabet / _sparse over the query shards of a node uploaded with KMDB_PARTITION_PREFIX_TABLES (any other
 * partition is refused): one2all<false> / one2all_sp of console_new2all.cpp:82 / :78 and console_one2all.cpp over the GPUs of a node.
 * Every device adds the rows of its own shards into one nq x N buffer (kmdb_new2all_batch*_device); with D > 1 the buffers meet in ONE
 * ncclReduceScatter (uint32 sum) over D flat chunks of ceil(nq N / D) cells and every device copies its chunk to out_dense.  K-mer entry:
 * a sorted query holds a bucket as one contiguous run — the host cuts every query at the bucket boundaries (kmdbh_query_shard_runs) and a
 * device receives only the runs of its own shards, so every query k-mer crosses PCIe once in all.  Sequence entry: the text goes to every
 * device and each shard keeps the positions of its own buckets before it sorts; out_kmer_counts is the sum over the shards.
 * kmdb_node_stats / kmdb_node_device_stats are filled as for all2all (call_ms: the device's own shards). */
int  kmdb_node_new2all_batch(kmdb_node* node, const uint64_t* const* kmers, const size_t* counts, size_t nq, uint32_t* out_dense,
                             const kmdb_opts* opts);
int  kmdb_node_new2all_batch_seq_alphabet(kmdb_node* node, const char* const* seqs, const size_t* seq_lens, size_t nq, double fraction,
                                          double start_fraction, int32_t alphabet, uint32_t* out_dense, uint64_t* out_kmer_counts,
                                          const kmdb_opts* opts);
int  kmdb_node_new2all_batch_sparse(kmdb_node* node, const uint64_t* const* kmers, const size_t* counts, size_t nq, kmdb_sparse_rows* out,
                                    const kmdb_opts* opts);
/* = kmdb_new2all_batch_sparse_filtered / kmdb_new2all_batch_seq_alphabet_sparse_filtered over the query shards of the node (console_new2all.cpp:76-78,
 * 130-148 over the GPUs of a node; a node of any other partition is refused under the entry point's name).  The rows meet as for
 * kmdb_node_new2all_batch; then every device compacts ITS OWN chunk of the reduce-scatter (the whole buffer with one device) on its own stream —
 * the cells are complete sums there, so the widened bounds apply —, the parts are concatenated row by row on the host and the exact decision runs
 * once.  Sequence entry: a query's count is the sum over the shards, complete only once every device has reported, so its compaction is a second
 * pass over the devices while the chunks are still resident.  kmdb_node_new2all_batch_sparse is the k-mer entry without bounds. */
int  kmdb_node_new2all_batch_sparse_filtered(kmdb_node* node, const uint64_t* const* kmers, const size_t* counts, size_t nq, const kmdb_cell_filter* filters,
                                             size_t n_filters, const uint32_t* sample_kmers /* [N] */, int measure, kmdb_sparse_rows* out,
                                             const kmdb_opts* opts);
int  kmdb_node_new2all_batch_seq_alphabet_sparse_filtered(kmdb_node* node, const char* const* seqs, const size_t* seq_lens, size_t nq, double fraction,
                                                          double start_fraction, int32_t alphabet, const kmdb_cell_filter* filters, size_t n_filters,
                                                          const uint32_t* sample_kmers /* [N] */, int measure, kmdb_sparse_rows* out,
                                                          uint64_t* out_kmer_counts, const kmdb_opts* opts);
/* the last sparse new2all call on the node: cells, nnz_device and d2h_bytes summed over the devices, the slowest device's compact_ms */
int  kmdb_node_new2all_sparse_stats_get(const kmdb_node* node, kmdb_new2all_sparse_stats* out);
/* = kmdb_new2all_batch_sampled over the query shards of the node (console_new2all.cpp:76-78, 130-148 + sampler.h:123-139 made multi-GPU): after
 * the reduce-scatter every device selects the candidates of ITS chunk of the summed rows on its own stream (kmdb_sampled_from_rows_device's
 * select), the host decides once (kmdbh_query_rows_select).  A node of another partition than KMDB_PARTITION_PREFIX_TABLES is refused;
 * argument errors are raised before any device thread starts. */
int  kmdb_node_new2all_batch_sampled(kmdb_node* node, const uint64_t* const* kmers, const size_t* counts, size_t nq, const kmdb_cell_filter* filters,
                                     size_t n_filters, const uint32_t* sample_kmers /* [N] */, int criterion, uint32_t count, kmdb_sparse_rows* out,
                                     const kmdb_opts* opts);
/* The text entry (kmdb_new2all_batch_seq_alphabet_sampled over the node): a query's count is complete only when every device has reported, so the
 * select is a second pass over the devices with the chunks still resident, as in kmdb_node_new2all_batch_seq_alphabet_sparse_filtered. */
int  kmdb_node_new2all_batch_seq_alphabet_sampled(kmdb_node* node, const char* const* seqs, const size_t* seq_lens, size_t nq, double fraction,
                                                  double start_fraction, int32_t alphabet, const kmdb_cell_filter* filters, size_t n_filters,
                                                  const uint32_t* sample_kmers /* [N] */, int criterion, uint32_t count, kmdb_sparse_rows* out,
                                                  uint64_t* out_kmer_counts, const kmdb_opts* opts);
/* the last sampled new2all call on the node: the fields of kmdb_sample_stats summed over the devices, the slowest device's select_ms */
int  kmdb_node_new2all_sample_stats_get(const kmdb_node* node, kmdb_sample_stats* out);

/* ---------------------------------------------------------------------------------------
 * Host-side helpers of the front-end (no GPU needed).  They mirror the reference's loader
 * and writer so that the CLI stays byte-compatible; exported so tests can drive them.
 * ------------------------------------------------------------------------------------- */
typedef struct kmdbh_db kmdbh_db;  /* a .db file parsed into flat host arrays */

/* PrefixKmerDb::deserialize (prefix_kmer_db.cpp:578-748). mode: 0 Everything, 2 SkipHashtables */
int  kmdbh_db_load(const char* path, int mode, kmdbh_db** out);
void kmdbh_db_free(kmdbh_db* db);
const kmdb_db_view* kmdbh_db_view(const kmdbh_db* db);
/* Once the database is on the device (kmdb_db_upload / kmdb_node_upload returned) a front-end that needs only the names and k-mer counts
 * from here on gives the pages of the pattern arrays and hashtables back (9 GB at 100 M patterns: otherwise the end of the process pays
 * for them, 0.07 s per GB).  The view's arrays must not be read afterwards; kmdbh_db_free is still due. */
void kmdbh_db_release_patterns(kmdbh_db* db);
uint32_t    kmdbh_db_kmer_length(const kmdbh_db* db);
double      kmdbh_db_fraction(const kmdbh_db* db);
double      kmdbh_db_start_fraction(const kmdbh_db* db);
int32_t     kmdbh_db_alphabet(const kmdbh_db* db);
uint64_t    kmdbh_db_n_samples(const kmdbh_db* db);
const char* kmdbh_db_sample_name(const kmdbh_db* db, uint64_t i);
uint64_t    kmdbh_db_sample_kmers(const kmdbh_db* db, uint64_t i);
uint64_t    kmdbh_db_pattern_section_bytes(const kmdbh_db* db);

/* The host's plan of the prefix shards kmdb_node_upload / kmdb_db_upload_shard work from (no GPU): for every shard s of n_shards the nodes
 * it keeps (those whose subtree holds a k-mer of a bucket b with b % n_shards == s; bucket = kmer >> 32, types.h:25-27) and the
 * k-mers it owns (items of those buckets, hashmap_lp.h:71-78).  The view must carry the hashtables. */
int  kmdbh_shard_plan_counts(const kmdb_db_view* view, uint32_t n_shards, uint64_t* kept_nodes, uint64_t* kmers);
/* The host's plan of the query shards kmdb_db_upload_query_shard / KMDB_PARTITION_PREFIX_TABLES work from (no GPU; call sites served:
 * console_new2all.cpp:64-95, console_one2all.cpp): per shard s the nodes it keeps and the k-mers it owns (as above), the slots of its own
 * bucket table (the sum of the capacities of the buckets b with b % n_shards == s, unchanged) and the number of those buckets,
 * ceil((n_buckets - s) / n_shards); local bucket = b / n_shards.  The view must carry the hashtables. */
int  kmdbh_query_shard_plan_counts(const kmdb_db_view* view, uint32_t n_shards, uint64_t* kept_nodes, uint64_t* kmers, uint64_t* slots,
                                   uint64_t* buckets);
/* The stretches of a sorted, duplicate-free query (KmerHelper::unique, console_new2all.cpp:73) that query shard `shard` of n_shards owns:
 * bucket = kmer >> 32 (types.h:25-27), so a bucket is one contiguous run and a shard's k-mers are the runs [run_begin[i], run_end[i]) —
 * maximal, ascending, disjoint; over all shards they cover the query once.  Returns the number of runs; writes the first `cap` of them
 * (run_begin / run_end may be NULL with cap 0 to count). */
size_t kmdbh_query_shard_runs(const uint64_t* kmers, size_t count, uint32_t n_shards, uint32_t shard, uint64_t* run_begin, uint64_t* run_end,
                              size_t cap);
/* The host's plan of the tree ranges kmdb_node_upload_partition / kmdb_db_upload_range work from (no GPU, no hashtables; ABI 8; call sites
 * served: console_all2all.cpp:26,31-36): from parent_id and num_samples alone, the DFS pre-order (children of a node, and the roots, in
 * ascending pattern id) cut into n_ranges contiguous stretches balanced by an estimate of the nodes' cost.  Per range s: own_nodes = nodes
 * of the stretch, first_depth = depth of its first node (a root has depth 1; 0 for an empty range), kept_nodes = own_nodes + first_depth - 1
 * (0 for an empty range), est_cost = the estimate's sum over the stretch; range_of[p] = the range of pattern p.  range_of and first_depth
 * may be NULL.  A pure function of (view, n_ranges). */
int  kmdbh_range_plan(const kmdb_db_view* view, uint32_t n_ranges, uint64_t* kept_nodes, uint64_t* own_nodes, uint64_t* est_cost,
                      uint32_t* range_of, uint32_t* first_depth);

/* KmerHelper::extract + MinHashFilter (kmer_extract.h:13-97, filter.h:28-115), nt alphabets.
 * Writes at most len k-mers to out; returns the count. */
size_t kmdbh_extract_kmers(const char* seq, size_t len, uint32_t k, double fraction, double start_fraction,
                           int preserve_strand, uint64_t* out);
/* The same over any alphabet of the reference (alphabet.h:79-86; ABI 7): `alphabet` = the database's AlphabetType as stored in the
 * file (kmdbh_db_alphabet; alphabet.h:10-18) — n-bit symbols (alphabet.h:36), k <= 64 / bits - 1 (:37), the strand preserved for
 * nt-preserve and every protein alphabet.  Returns 0 for an unknown alphabet or a k the alphabet cannot hold. */
#define KMDB_ALPHABET_NT            0
#define KMDB_ALPHABET_NT_PRESERVE   1
#define KMDB_ALPHABET_AA            2
#define KMDB_ALPHABET_AA11_DIAMOND  3
#define KMDB_ALPHABET_AA12_MMSEQS   4
#define KMDB_ALPHABET_AA6_DAYHOFF   5
#define KMDB_ALPHABET_COUNT         6
size_t kmdbh_extract_kmers_alphabet(const char* seq, size_t len, uint32_t k, int32_t alphabet, double fraction, double start_fraction,
                                    uint64_t* out);
/* Alphabet::mapping (alphabet.h:41-58): symbol code of every byte (-1: not a symbol), number of symbols, bits per symbol, strand flag.
 * 0 on success, 1 for an unknown alphabet. */
int    kmdbh_alphabet_table(int32_t alphabet, int8_t* map256, uint32_t* n_symbols, uint32_t* bits_per_symbol, int* preserve_strand);
/* The hash window of MinHashFilter (filter.h:42-43), additive in ABI 8: a k-mer is kept when lo <= hash < hi.  Both extractors above and
 * the device loader take their thresholds from here.  A bound at or beyond 2^64 (a window that ends at 1: -f 0.7 -f-start 0.3) becomes 0,
 * as in the reference built with its own flags: such a window keeps no k-mer. */
void   kmdbh_minhash_window(double fraction, double start_fraction, uint64_t* lo, uint64_t* hi);
/* KmerHelper::unique (kmer_extract.h:112-118): sort + dedupe in place, returns new count */
size_t kmdbh_sort_unique(uint64_t* kmers, size_t n);

/* ---------------------------------------------------------------------------------------
 * The minhash mode (README 2.4 of the reference: minhash every sample once into <sample>.minhash, then feed the files to build / new2all /
 * one2all with -from-minhash).  Additive in ABI 8 (KMDB_HAS_MINHASH).
 * ------------------------------------------------------------------------------------- */
/* The sorted unique k-mer words of a batch of samples: sample s holds kmers[offsets[s] .. offsets[s + 1]).  Library-allocated, free with
 * kmdb_kmer_lists_free(). */
typedef struct kmdb_kmer_lists {
    uint64_t  n_samples;
    uint64_t* offsets;             /* [n_samples + 1] */
    uint64_t* kmers;               /* [offsets[n_samples]] */
} kmdb_kmer_lists;
/* Replaces, for a whole batch of samples, the loader + KmerHelper::sortAndUnique of MinhashConsole::run (console_minhash.cpp:19-40; also what
 * console_new2all.cpp:73 and console_one2all.cpp:64-66 do per query): the device extracts the k-mers of every sample, keeps those inside the
 * hash window (kmdbh_minhash_window(fraction, start_fraction); fraction >= 1: no filter, NullFilter) and returns them sorted and unique —
 * the words of kmdbh_extract_kmers_alphabet + kmdbh_sort_unique, widening included.  No database handle is needed.
 * seqs[s]: the text of sample s, its records joined by '\n' (the form kmdb_new2all_batch_seq_alphabet takes); '\n' and every byte outside the
 * alphabet end a window.  The device (opts->device) and the stream (opts->stream, NULL: the default stream) come from opts; opts may be NULL
 * (device 0).  The words are filtered BEFORE they are stored (count, scan, write), so device memory beyond the text grows with what is kept.
 * A batch is cut into pieces at sample boundaries (KMDB_MINHASH_BASES_PER_PIECE bases, default 2^29); a sample longer than that goes alone, up
 * to KMDB_MINHASH_MAX_SAMPLE_BASES bytes of text (default 2^30; both are read at every call).  A longer sample — of any length, 2^31 bases and
 * beyond — is extracted in consecutive sections of at most the piece budget, cut wherever the budget falls: a section owns the k-mers whose last
 * symbol lies in it and is shown the symbols in front of it; its sorted unique list stays on the device and is joined into the sample's
 * running list by kmdb_sorted_union_device's kernels, so device memory is bounded by one section's scratch beside the sample's own list.
 * The words are those of the sample extracted whole.  Refused: an unknown alphabet, a k the alphabet cannot hold (alphabet.h:37). */
int  kmdb_minhash_batch_seq_alphabet(const char* const* seqs, const size_t* seq_lens, size_t n_samples, uint32_t kmer_length,
                                     double fraction, double start_fraction, int32_t alphabet, kmdb_kmer_lists* out, const kmdb_opts* opts);
void kmdb_kmer_lists_free(kmdb_kmer_lists* lists);
/* The extractor's geometry: a thread takes a run of *positions_per_thread consecutive positions of the batch's flat text, a workgroup a tile of
 * *positions_per_tile (tests place their edges by these). */
void kmdb_minhash_geometry(uint32_t* positions_per_thread, uint32_t* positions_per_tile);
typedef struct kmdb_minhash_stats {   /* the LAST kmdb_minhash_batch_seq_alphabet call of the calling thread, summed over its pieces */
    uint64_t pieces;
    uint64_t bases;                /* bytes of text */
    uint64_t kept;                 /* words that passed the filter (before sort + unique) */
    uint64_t unique;               /* words returned */
    uint64_t scratch_bytes;        /* device memory of the largest piece, text included */
    double   h2d_ms;               /* HIP events: allocation of the text + its copy to the device */
    double   count_ms;             /* pass 1 (extraction, tile counts) */
    double   scan_ms;              /* scan of the tile counts, the total to the host */
    double   write_ms;             /* pass 2 (extraction, kept words written) */
    double   sort_ms;              /* the two radix sorts */
    double   unique_ms;            /* head flags, scan, compaction, the lists to the host */
} kmdb_minhash_stats;
int  kmdb_minhash_stats_get(kmdb_minhash_stats* out);   /* (a section of a long sample counts as a piece; `unique` counts a long sample's final list) */
typedef struct kmdb_minhash_long_stats {   /* the long samples of the same call (all zero when it had none) */
    uint64_t long_samples;         /* samples extracted in sections */
    uint64_t sections;             /* their sections */
    uint64_t union_words_in;       /* words that went into the merge-unions (both sides, summed over the unions) */
    uint64_t union_words_out;      /* words they wrote */
    uint64_t union_bytes;          /* device memory traffic of the unions by construction: both inputs read twice (count, write), the union written once */
    uint64_t peak_bytes;           /* most device memory held at once: the running list + a section's scratch, or + a section's list, the union and its tables */
    double   union_ms;             /* HIP events around the unions */
} kmdb_minhash_long_stats;
int  kmdb_minhash_long_stats_get(kmdb_minhash_long_stats* out);
/* out_dev[0 .. *n_out) = the union of a_dev[0 .. na) and b_dev[0 .. nb), two STRICTLY ascending arrays of 64-bit words in device memory (compared
 * unsigned), strictly ascending: a merge — merge-path partition into tiles, per-tile counts, a 64-bit scan, a write pass — not a sort, with every
 * index 64 bits wide.  out_dev must not overlap the inputs.  The device and the stream come from opts (NULL: device 0, the default stream); the
 * call returns when the union is written.  Refused under the entry's name: out_cap < na + nb (whatever the arrays have in common), a null array
 * with a size that is not 0.  Arrays that do not ascend give an unspecified order of words and never a fault: every index is clamped to its array. */
int  kmdb_sorted_union_device(const void* a_dev, uint64_t na, const void* b_dev, uint64_t nb, void* out_dev, uint64_t out_cap, uint64_t* n_out,
                              const kmdb_opts* opts);
/* The union's geometry: a thread merges *words_per_thread words of the merged order, a workgroup a tile of *words_per_tile (tests place their edges by these). */
void kmdb_sorted_union_geometry(uint32_t* words_per_thread, uint32_t* words_per_tile);
/* Replaces MihashedInputFile::store (minhashed_input_file.h:109-118, call site console_minhash.cpp:47), byte for byte: u32 0xfedcba98, u64 count,
 * count x u64 words, u32 k, f64 fraction; little-endian, no padding.  `path` is the full file name: the caller appends ".minhash" (no GPU). */
int  kmdbh_minhash_store(const char* path, const uint64_t* kmers, size_t count, uint32_t kmer_length, double fraction);
/* Replaces MihashedInputFile::open + load (minhashed_input_file.h:58-105; call sites console_one2all.cpp:57, the loader of console_new2all.cpp
 * and console_build.cpp with -from-minhash).  The words come back as stored: no filter is applied to them.  The file's size is checked against
 * 24 + 8 * count BEFORE anything is allocated (a damaged count field is an error, not an allocation); a wrong signature is refused.
 * *kmers is library-allocated: free with kmdbh_minhash_free() (no GPU). */
int  kmdbh_minhash_load(const char* path, uint64_t** kmers, size_t* count, uint32_t* kmer_length, double* fraction);
void kmdbh_minhash_free(uint64_t* kmers);

/* ---------------------------------------------------------------------------------------
 * The build mode (console_build.cpp): genomes in, a database out.  Additive in ABI 8 (KMDB_HAS_BUILD).
 * The builder keeps the whole state of PrefixKmerDb on the device: the sorted dictionary of the distinct k-mers with the pattern id of each,
 * the pattern fields, and one (pattern, sample) event per "sample appended to the pattern's local ids".  Samples take their ids in the order
 * they are added; the pattern ids are those of the reference's addKmers run with ONE thread (prefix_kmer_db.cpp:181-240: the groups of a
 * sample in ascending old pattern id, the group of the k-mers new to the database first).  How the samples are cut into calls changes nothing.
 * Device memory: 12 bytes per distinct k-mer (twice that while a call merges new k-mers in), 24 per pattern, 8 per event, 36 per k-mer of
 * the largest sample of a call; at finish 24 more per event, 36 more per pattern, the streams and the tables.  An allocation the device
 * cannot serve is refused with the bytes it needed — the builder does not spill to the host — and leaves the builder DEAD: every later
 * call but kmdb_build_free / kmdb_build_stats_get is refused.  So does any HIP error inside a call.  A refusal that is found before the
 * state is touched (a list out of order, a sample too long, an add after finish) leaves the builder as it was.
 * ------------------------------------------------------------------------------------- */
typedef struct kmdb_builder kmdb_builder;
typedef struct kmdb_build_stats {  /* the whole life of the builder so far */
    uint64_t samples;              /* samples added (empty ones included) */
    uint64_t kmers_added;          /* sum of the samples' list lengths */
    uint64_t distinct_kmers;       /* size of the dictionary */
    uint64_t patterns;             /* pattern 0 included */
    uint64_t events;               /* (pattern, sample) pairs = sum of num_local over the patterns */
    uint64_t peak_device_bytes;    /* most device memory the builder held at once */
    double   merge_ms;             /* HIP events: new k-mers found and merged into the dictionary (once per call) */
    double   lookup_ms;            /* ... per sample: position and pattern of every k-mer */
    double   sort_ms;              /* ... per sample: radix sort by pattern */
    double   group_ms;             /* ... per sample: groups, extend / new pattern, the k-mers' new ids */
    double   encode_ms;            /* finish: events grouped by pattern, gamma streams */
    double   tables_ms;            /* finish: the prefix-bucket hashtables */
    double   copy_back_ms;         /* finish: everything to the host */
} kmdb_build_stats;
/* Replaces PrefixKmerDb's constructor + initialize (console_build.cpp:38-60; prefix_kmer_db.cpp:20-63).  fraction / start_fraction are the
 * filter of the text entry and the values of the database's header (the reference's build always stores start 0, prefix_kmer_db.cpp:454:
 * this library stores the start it used, so that new2all filters its queries with the builder's window).  opts: device and stream; NULL = device 0.
 * Refused: an unknown alphabet, a k the alphabet cannot hold (alphabet.h:37). */
int  kmdb_build_begin(uint32_t kmer_length, double fraction, double start_fraction, int32_t alphabet, const kmdb_opts* opts, kmdb_builder** out);
/* Replaces db->deserialize followed by the filter and alphabet taken from the database (console_build.cpp:48-57: `build -extend`): a builder whose
 * state is the one a builder holds after the samples of `db` were added one by one — so that extending build(A) with the samples B gives the file
 * build(A followed by B) gives.  k, fraction, start fraction, alphabet, sample names and per-sample k-mer counts are the database's; new samples
 * are numbered from its n_samples on; kmdb_build_add_*, kmdb_build_finish, kmdb_build_free and kmdb_build_stats_get behave as on that builder
 * (kmdb_build_stats: samples / distinct_kmers / patterns / events / peak_device_bytes include the seed, kmers_added and the stage times count
 * only the add calls).  Everything happens on the device: the tables' items are compacted to (k-mer, pattern id) pairs and sorted into the
 * dictionary, is_parent — which a stored database does not carry — is recomputed from parent_id, and every pattern's gamma stream is decoded
 * into its (pattern, sample) events.  Any numbering of the patterns with parent_id[p] < p is taken (a database the reference built with several
 * threads).  `db` must hold its tables (kmdbh_db_load mode 0, or the result of kmdb_build_finish) and is only read; it may be freed afterwards.
 * Refused before any device work: a database without tables, 2^31 patterns, events or distinct k-mers or more, a bucket count that is not the
 * one of k.  Refused after the device's checks, each with its own message: a table value that is 0 or no pattern id, a k-mer stored twice or
 * wider than k symbols, k-mers per pattern that differ from num_kmers, a stream that does not end at num_bits or lies outside the data words,
 * sample ids that do not ascend below n_samples, parent_id[p] >= p.  Every stream read is clamped to the pattern's own words: a damaged file
 * is a refusal, never a fault.  Device memory is accounted and limited as for every builder (KMDB_BUILD_DEVICE_BYTES); the slots go up in
 * pieces of KMDB_BUILD_SEED_SLOTS_PER_PIECE (default 2^27).  On any refusal *out stays NULL and nothing is left allocated. */
int  kmdb_build_begin_from_db(const kmdbh_db* db, const kmdb_opts* opts, kmdb_builder** out);
typedef struct kmdb_build_seed_stats {   /* what kmdb_build_begin_from_db did (zeros on a builder made by kmdb_build_begin) */
    uint64_t samples, distinct_kmers, patterns, events;   /* of the seed */
    uint64_t slots;                /* slots of the database's tables that went through the device */
    uint64_t h2d_bytes;            /* bytes copied to the device */
    double   upload_ms;            /* HIP events: the host-to-device copies */
    double   dict_ms;              /* ... flag, scan, compaction of the slots; the sort into the dictionary */
    double   tree_ms;              /* ... is_parent from parent_id */
    double   decode_ms;            /* ... scan of num_local, the gamma streams decoded into events (their checks included) */
    double   check_ms;             /* ... the dictionary's order and width, k-mers per pattern against num_kmers */
} kmdb_build_seed_stats;
int  kmdb_build_seed_stats_get(const kmdb_builder* b, kmdb_build_seed_stats* out);
/* Replaces one db.addKmers per sample (console_build.cpp:111; prefix_kmer_db.cpp:244-434) for n_samples samples: kmers[s] = the sample's k-mers,
 * STRICTLY ascending (the stored words of a <sample>.minhash, or kmdbh_extract_kmers_alphabet + kmdbh_sort_unique) — uploaded as they are and
 * checked on the device.  Refused before the builder's state changes: a list that is not strictly ascending, a sample of 2^32 k-mers or more
 * (the reference's count is 32 bits; this builder indexes a sample's k-mers with 31), an add after finish. */
int  kmdb_build_add_kmers(kmdb_builder* b, const char* const* names, const uint64_t* const* kmers, const size_t* counts, size_t n_samples);
/* The same from text (console_build.cpp:111 with the loader in front of it, genome_input_file.h): seqs[s] = the sample's records joined by '\n',
 * the form kmdb_minhash_batch_seq_alphabet takes.  Extracted, filtered with the builder's window, sorted and made unique on the device with
 * that entry's own kernels — a long sample in sections, as there; the lists never visit the host.  A sample of 2^31 k-mers or more is refused. */
int  kmdb_build_add_seq_alphabet(kmdb_builder* b, const char* const* names, const char* const* seqs, const size_t* seq_lens, size_t n_samples);
/* Replaces what PrefixKmerDb::serialize reads out of the live object (console_build.cpp:149; prefix_kmer_db.cpp:438-574): gamma streams, tables,
 * everything copied into a kmdbh_db — free it with kmdbh_db_free; upload it (kmdb_db_upload(kmdbh_db_view(h), ...)) or store it.  The
 * builder takes no more samples afterwards and can be finished once. */
int  kmdb_build_finish(kmdb_builder* b, kmdbh_db** out);
void kmdb_build_free(kmdb_builder* b);
int  kmdb_build_stats_get(const kmdb_builder* b, kmdb_build_stats* out);
/* The hand-off (KMDB_HAS_BUILD_HANDOFF): kmdb_build_finish followed by kmdb_db_upload(kmdbh_db_view(h), opts, with_hashtables, ...) without the
 * host in between.  *out_db is, in every respect, the handle that pair returns — that equivalence defines the result, the upload's refusals
 * with the upload's messages included (2^31 patterns or more, KMDB_MAX_SAMPLES samples or more, unknown bits in opts->flags, its tree and
 * header checks) — but no pattern field, stream word or table slot visits the host: one kernel narrows the builder's fields, the streams are
 * re-packed from their word-aligned pid-order places, the tables go device to device.  kmdb_stats.h2d_bytes of the handle is 0, upload_ms is
 * the time of the layout and the preparation.  opts->device must be the builder's device; another one is refused.  The refusals that need no
 * device work (flags, counts, device) leave the builder as it was; everything later ends it exactly as kmdb_build_finish does (a later add or
 * finish is refused, a failure leaves it dead), and kmdb_build_free stays the caller's job.
 * with_hashtables = 0 and host_image = 0 skips the tables altogether (bucket starts, capacities, insert), and the all2all working set is
 * prepared as for an all2all upload.  out_host may be NULL.  host_image = 1: *out_host is the image kmdb_build_finish returns (kmdbh_db_store
 * of it gives the same bytes; the tables are made whatever with_hashtables says).  host_image = 0: *out_host is a HEADER-ONLY image — names,
 * per-sample k-mer counts, k, fraction, start fraction, alphabet, kmers_count; its view has n_patterns == 0, which no stored database has
 * (pattern 0 always exists), and kmdbh_db_store and every kmdb_db_upload* refuse it with a message.
 * The builder's arrays are released as soon as their last reader has run: the unsorted events after the sort, the dictionary before the
 * layout, the tree and the per-pattern fields after the fields kernel, the tables after their copy, the pid-order stream words after the
 * re-pack (a full host image keeps all but the dictionary until it is copied). */
int  kmdb_build_finish_device(kmdb_builder* b, const kmdb_opts* opts, int with_hashtables, int host_image, kmdb_db** out_db, kmdbh_db** out_host);
typedef struct kmdb_build_handoff_stats {   /* what kmdb_build_finish_device did (zeros before it) */
    uint64_t patterns, samples;
    uint64_t peak_device_bytes;    /* most device memory builder and handle held together during the call */
    uint64_t handle_device_bytes;  /* kmdb_stats.device_bytes of the handle */
    uint64_t d2h_bytes;            /* bytes of the host image copied back (0 for a header-only image) */
    uint32_t with_hashtables, host_image;   /* as asked */
    double   encode_ms;            /* HIP events: events grouped by pattern, gamma streams */
    double   tables_ms;            /* ... the prefix-bucket hashtables (0 when they were skipped) */
    double   fields_ms;            /* wall clock: the fields kernel, the tables copied device to device */
    double   layout_ms;            /* ... DFS pre-order, node arrays, stream re-pack, slices and long nodes */
    double   prepare_ms;           /* ... the all2all working set (0 with hashtables: made by the first all2all call) */
    double   copy_back_ms;         /* HIP events: the full host image (0 otherwise) */
    double   total_ms;             /* wall clock of the call */
} kmdb_build_handoff_stats;
int  kmdb_build_handoff_stats_get(const kmdb_builder* b, kmdb_build_handoff_stats* out);
/* The header-only image of a database, as kmdb_build_finish_device returns it with host_image = 0 (names, counts, k, fractions, alphabet);
 * free it with kmdbh_db_free.  No GPU. */
int  kmdbh_db_header_only(const kmdbh_db* db, kmdbh_db** out);
/* PrefixKmerDb::serialize(file, true) (prefix_kmer_db.cpp:438-574; call site console_build.cpp:149): header fields :449-457, samples, raw tables
 * (hashmap_lp.h:481-528), patterns in blocks of at most 64 MB cut by the reference's own rule (:545-569).  is_parent goes into bytes 32..35 of
 * every pattern header, zeros into bytes 36..39 (the reference leaves those four unwritten: pattern.cpp:35-37).  Any kmdbh_db that holds its
 * tables (kmdbh_db_load mode 0, kmdb_build_finish) can be stored; no GPU. */
int  kmdbh_db_store(const kmdbh_db* db, const char* path);

/* ---------------------------------------------------------------------------------------
 * The distance mode (console_distance.cpp:7-213): the body of a table of common k-mer counts in, the table of one measure out, text to text.
 * Additive in ABI 8 (KMDB_HAS_DISTANCE).  The device classifies the bytes, parses every field, computes the measure of every cell and writes
 * the text; a cell whose six decimals or whose bounds the device's arithmetic cannot settle (kmdb_distance_stats.host_cells, about 2e-6 of
 * the cells) takes no bytes there and is computed with kmdbh_metric, formatted with kmdbh_format_measure and spliced in on the host.
 * ------------------------------------------------------------------------------------- */
#define KMDB_DISTANCE_SPARSE_OUT 1u  /* -sparse: "column:value," of the non-zero counts that pass the bounds */
#define KMDB_DISTANCE_SPARSE_IN  2u  /* the rows hold "column:count" pairs (sparse input always gives sparse output) */
#define KMDB_DISTANCE_TRIANGLE   4u  /* dense rows: row i keeps min(i, n) values (decided by the caller from row 0, console_distance.cpp:149-152) */
#define KMDB_DISTANCE_PHYLIP     8u  /* -phylip-out: blanks as separators, no bounds; dense input only */
#define KMDB_DISTANCE_FLAGS_ALL  15u
#define KMDB_DISTANCE_MAX_FILTERS 12 /* the device filter's capacity: one bound pair per criterion and a few repeats */
/* status of kmdb_distance_rows besides 0 and 1: the text is one the device path does not take; kmdb_last_error() says why, nothing was
 * written, the handle stays usable.  The caller runs the host loop instead. */
#define KMDB_DISTANCE_DECLINED 2
typedef struct kmdb_distance kmdb_distance;
typedef struct kmdb_distance_opts {
    uint32_t abi_version;          /* KMDB_ABI_VERSION */
    int32_t  device;               /* HIP device ordinal */
    int32_t  measure;              /* KMDB_METRIC_* */
    uint32_t kmer_length;
    const uint32_t* counts;        /* [n] the table's total-kmers row (copied) */
    uint64_t n;                    /* columns of the table */
    const kmdb_cell_filter* filters;   /* [n_filters] bounds, the num-kmers bounds among them (KMDB_METRIC_NUM_KMERS); copied */
    uint64_t n_filters;            /* at most KMDB_DISTANCE_MAX_FILTERS */
    uint32_t flags;                /* KMDB_DISTANCE_* */
    uint32_t reserved;
    void*    stream;               /* hipStream_t to run on, NULL = the default stream */
} kmdb_distance_opts;
typedef struct kmdb_distance_out {
    char*    text;                 /* library-allocated, free with kmdb_distance_out_free */
    size_t   len;
    uint64_t rows;                 /* rows the call took */
} kmdb_distance_out;
typedef struct kmdb_distance_stats {   /* the whole life of the handle */
    uint64_t calls;
    uint64_t rows;
    uint64_t cells_read;           /* cells of the input the row rules read */
    uint64_t cells_written;        /* values in the output, the host's included */
    uint64_t host_cells;           /* cells the device left to the host (rounding boundary, bound margin, not finite) */
    uint64_t bytes_in, bytes_out;
    uint64_t device_bytes;         /* most device memory one call held */
    double   parse_ms;             /* HIP events: classification, compactions, digits */
    double   measure_ms;           /* ... the measures, the text lengths, their scans */
    double   format_ms;            /* ... names, separators, digits written */
    double   copy_ms;              /* ... text to the device, text and the host's cells back */
} kmdb_distance_stats;
/* Replaces the setup of DistanceConsole::run (console_distance.cpp:58-72, 93-98).  Refused: an unknown measure or criterion, more than
 * KMDB_DISTANCE_MAX_FILTERS bounds, unknown flags, no usable device. */
int  kmdb_distance_begin(const kmdb_distance_opts* opts, kmdb_distance** out);
/* Replaces the row loop (console_distance.cpp:75-204) for a run of WHOLE rows: `lines` = len bytes of table text in host memory, the rows
 * first_row, first_row + 1, ... of the body; only the last row may lack its '\n'.  out->text = byte for byte what the loop writes for them
 * ('\n' for endl).  Every read is clamped to the piece: damaged text is declined or parsed as the host loop parses it, never a fault.
 * Declined (KMDB_DISTANCE_DECLINED): a line without a comma; a field of more than 10 digits or with a byte that is neither a digit nor a
 * separator; "a:b:c"; a pair without SPARSE_IN or a plain cell with it (so: rows that mix the two); PHYLIP with SPARSE_IN; 2^32 - 64 bytes or more. */
int  kmdb_distance_rows(kmdb_distance* d, const char* lines, size_t len, uint64_t first_row, kmdb_distance_out* out);
/* The same table from a matrix in HBM (KMDB_HAS_DISTANCE_MATRIX): `all2all` followed by `distance` without the table of counts in between.
 * The handle is begun with the samples' k-mer counts as `counts` (n = N: they are the rows' counts and the columns'), with
 * KMDB_DISTANCE_TRIANGLE and without KMDB_DISTANCE_SPARSE_IN — any other handle is refused by the three calls below.  What
 * kmdb_distance_matrix_rows returns for rows [row_lo, row_hi) is byte for byte what kmdb_distance_rows returns for those rows of the DENSE
 * table of counts of the matrix ("<name>,<count>,<cell>,...,\n", row i with its i cells): "<name>," and i values; with SPARSE_OUT
 * "<column + 1>:<value>," of the non-zero cells that pass the bounds (a = the row sample's count, b = the column's); with PHYLIP blanks and
 * no bounds.  The cells the device cannot settle go to the host as they do there (kmdb_distance_stats.host_cells).
 *
 * take_all2all: runs kmdb_all2all_dense_device of `db` (opts as there, NULL: the whole database; a null opts->stream means the handle's)
 *   into a triangle of N (N - 1) / 2 uint32 the HANDLE allocates and owns, freed with the handle or at the next take.  Refused: a database
 *   on another device than the handle's, or of another N than the handle's n.
 * take_cells_device: borrows cells the CALLER accumulated (a sum over shards, a tensor).  cells_dev points at the FIRST CELL OF ROW row_lo,
 *   cell row_lo (row_lo - 1) / 2 of the triangle, and holds every cell from there to the end of the triangle or of the last row asked for:
 *   a few late rows of a large matrix can be handed over without the rows in front of them (the cell_lo convention of
 *   kmdb_sparse_from_dense_device, whose stream note applies: the cells must be complete on the handle's stream).  A null pointer is taken
 *   when the rows asked for later hold no cells (row 0; N = 1).  Refused: row_lo > n.
 * Both copy `names` (n C strings) to the device once, as a blob and its offsets.
 * matrix_rows: out as with kmdb_distance_rows (kmdb_distance_out_free); row_lo == row_hi gives empty text and 0 rows.  Refused: no matrix
 *   taken; row_lo > row_hi; row_hi > n; rows in front of a borrowed pointer's row_lo; cells and a null pointer; a piece of 2^31 cells or
 *   more, or one whose working arrays (17 B a cell) do not fit the device's free memory — the message gives the bytes; ask for fewer rows.
 * kmdb_distance_stats counts these calls in its fields: cells_read = the cells of the rows, bytes_in = four times that, parse_ms stays 0. */
int  kmdb_distance_take_all2all(kmdb_distance* d, kmdb_db* db, const char* const* names, const kmdb_opts* opts);
int  kmdb_distance_take_cells_device(kmdb_distance* d, const void* cells_dev, uint64_t row_lo, const char* const* names);
int  kmdb_distance_matrix_rows(kmdb_distance* d, uint64_t row_lo, uint64_t row_hi, kmdb_distance_out* out);
/* The cells the handle reads: the first cell of the row it was taken from (row 0 after take_all2all); null before a take.  A second handle of
 * the same n — another measure, other bounds — borrows them with kmdb_distance_take_cells_device while the first one lives: one all2all
 * run serves several tables. */
const void* kmdb_distance_cells_device(const kmdb_distance* d);
/* The same table from the rows of a batch of queries in HBM (KMDB_HAS_DISTANCE_QUERY_ROWS): `new2all` followed by `distance` without the table
 * of counts in between.  The handle is begun with the DATABASE samples' k-mer counts as `counts` (n = N: the columns' counts), WITHOUT
 * KMDB_DISTANCE_TRIANGLE and without KMDB_DISTANCE_SPARSE_IN — any other handle is refused by the four calls below.  What
 * kmdb_distance_query_rows returns for rows [row_lo, row_hi) of the batch is byte for byte what kmdb_distance_rows returns for those rows of
 * the DENSE table of counts new2all writes ("<query name>,<query count>,<N cells>,\n"): "<query name>," and N values; with SPARSE_OUT
 * "<column + 1>:<value>," of the non-zero cells that pass the bounds; with PHYLIP blanks and no bounds.  In every measure and bound a = the
 * QUERY's own k-mer count truncated to uint32, b = counts[column]: mash-query tells the two apart.  The cells the device cannot settle go to
 * the host as they do for text (kmdb_distance_stats.host_cells).  The triangle rule of the distance mode (row 0 named like the first sample
 * with a first cell of 0) is the CALLER's to decide: these calls always write whole rows.
 *
 * take_new2all_batch: the HANDLE owns an nq x N rectangle of uint32, kept between takes and grown only for a larger batch; the call zeroes
 *   it on the handle's stream, runs kmdb_new2all_batch_device of `db` into it (kmers, counts, nq, opts as there; NULL opts: the defaults; a
 *   null opts->stream means the handle's) and keeps a[q] = (uint32_t)counts[q] and the nq `names` (C strings) on the device.
 * take_new2all_batch_seq_alphabet: the same through kmdb_new2all_batch_seq_alphabet_device; a[q] = the device extractor's unique count, also
 *   returned in out_kmer_counts.
 *   Both refuse: a database on another device than the handle's, or of another N than the handle's n; a handle without hashtables; a QUERY
 *   SHARD handle (kmdb_db_upload_query_shard) — its rows are partial sums and so are its counts: sum the shards' rows and hand them over
 *   with take_rows_device.
 * take_rows_device: borrows rows the CALLER accumulated (a sum over shards, a tensor, another handle's rows): rows_dev = cell 0 of a
 *   row-major nq x N rectangle of uint32 in device memory, complete on the handle's stream and alive while rows are asked for; query_kmers
 *   = the nq queries' counts in host memory.  A null pointer is taken when the rows asked for later hold no cells.  A second handle of the
 *   same n — another measure, other bounds — borrows the first one's rows: kmdb_distance_cells_device returns the address of the rows taken.
 * query_rows: out as with kmdb_distance_rows (kmdb_distance_out_free); row_lo == row_hi gives empty text and 0 rows.  Refused: nothing
 *   taken; row_lo > row_hi; row_hi > nq; cells and a null pointer; a piece of 2^31 cells or more, or one whose working arrays (17 B a cell)
 *   do not fit the device's free memory — the message gives the bytes; ask for fewer rows.
 * kmdb_distance_stats counts these calls in its fields: cells_read = the cells of the rows, bytes_in = four times that, parse_ms stays 0. */
int  kmdb_distance_take_new2all_batch(kmdb_distance* d, kmdb_db* db, const uint64_t* const* kmers, const size_t* counts, size_t nq,
                                      const char* const* names, const kmdb_opts* opts);
int  kmdb_distance_take_new2all_batch_seq_alphabet(kmdb_distance* d, kmdb_db* db, const char* const* seqs, const size_t* seq_lens, size_t nq,
                                                   double fraction, double start_fraction, int32_t alphabet, const char* const* names,
                                                   uint64_t* out_kmer_counts, const kmdb_opts* opts);
int  kmdb_distance_take_rows_device(kmdb_distance* d, const void* rows_dev, size_t nq, const uint32_t* query_kmers /* [nq], host */,
                                    const char* const* names);
int  kmdb_distance_query_rows(kmdb_distance* d, uint64_t row_lo, uint64_t row_hi, kmdb_distance_out* out);
/* The same table from a CSR in HBM (KMDB_HAS_DISTANCE_PARTS): `all2all-parts` followed by `distance -sparse` without the table of counts in
 * between.  The handle must have been begun with KMDB_DISTANCE_SPARSE_OUT, without KMDB_DISTANCE_TRIANGLE, KMDB_DISTANCE_SPARSE_IN and
 * KMDB_DISTANCE_PHYLIP, and with `counts` = the k-mer counts of the WHOLE collection (n = all samples of all parts) — any other handle is
 * refused by every call below.  The source is a CSR over nr rows, the samples of one block row of the grid: row_ptr uint64[nr + 1] ascending
 * from 0, col uint32 0-based GLOBAL columns (already shifted by the samples of the earlier parts) ascending within a row, val uint32 > 0.
 * What kmdb_distance_csr_rows returns for rows [row_lo, row_hi) is byte for byte what kmdb_distance_rows of a KMDB_DISTANCE_SPARSE_IN handle
 * returns for the "name,count,col:val,..." text of those rows: a = the ROW sample's own count, b = counts[col], the bounds and the host cells
 * as everywhere (kmdb_distance_stats.host_cells).
 *   parts_begin_rows: starts a block row of nr row samples (their k-mer counts, truncated to 32 bits as the text path truncates them, and their
 *     names) and drops the previous one.
 *   parts_add_db2db: the cell (db_row, db_col) computed as kmdb_db2db_sparse_filtered computes it, without bounds, its CSR kept in HBM; col_shift
 *     = the samples of the parts before db_col's.  Out of device memory it retries once without the list stores and then returns the library's
 *     usual out-of-memory error: the caller may evict resident parts and repeat.  The cells are kept UNFILTERED: the handle's bounds are
 *     applied cell by cell when the rows are written, so that a handle with other bounds can borrow the same CSR.
 *   parts_add_all2all: the diagonal cell, the lower triangle of `db` as kmdb_all2all_sparse computes it.
 *   parts_add_csr_device: a cell the caller computed — a CSR in HBM over the nr rows of the block row, its n_cols columns LOCAL to the cell —
 *     checked and COPIED into the block row (the caller's arrays may go when the call returns).
 *   take_csr_device: BORROWS a CSR the caller built and keeps alive (a tensor, another handle's gathered CSR).
 *   csr_rows: out as with kmdb_distance_rows (kmdb_distance_out_free); row_lo == row_hi gives empty text and 0 rows.  The first call after the
 *     adds gathers the cells into ONE CSR on the device (merged row_ptr = the sum of the cells' row_ptr; every entry copied to its place with
 *     its column shifted) and frees the cells' own.
 *   csr_device / csr_row_ptr: the gathered (or taken) CSR's device addresses, for a second handle to borrow, and its row_ptr on the host
 *     ([nr + 1]: what a caller cuts its pieces by); both gather first where cells are waiting.
 * Refused by name: null arguments; a handle of another kind; row_lo > row_hi or row_hi > nr; rows asked before anything was taken; entries
 * behind a null pointer; a row_ptr that does not ascend from 0, or a column >= n (both found on the device when the CSR is taken and reported
 * with a message, never as a fault); a database on another device; a query-shard handle; a part whose samples do not fit the columns; a piece of
 * 2^31 cells or more, or beyond the free device memory (with the bytes).  The offsets of entries are 64-bit throughout. */
typedef struct kmdb_distance_parts_stats {   /* the whole life of the handle */
    uint64_t block_rows;           /* kmdb_distance_parts_begin_rows calls */
    uint64_t grid_cells;           /* cells added */
    uint64_t cells_in;             /* entries of the cells added */
    uint64_t cells_written;        /* entries whose text the device wrote */
    uint64_t host_cells;           /* entries the host decided */
    uint64_t peak_bytes;           /* the most a block row held on the device: its cells' CSRs, the gathered CSR, a piece's working arrays */
    double   gather_ms;
} kmdb_distance_parts_stats;
int  kmdb_distance_parts_begin_rows(kmdb_distance* d, size_t nr, const uint32_t* row_kmers /* [nr], host */, const char* const* names /* [nr] */);
int  kmdb_distance_parts_add_db2db(kmdb_distance* d, kmdb_db* db_row, kmdb_db* db_col, uint64_t col_shift, const kmdb_opts* opts);
int  kmdb_distance_parts_add_all2all(kmdb_distance* d, kmdb_db* db, uint64_t col_shift, const kmdb_opts* opts);
int  kmdb_distance_parts_add_csr_device(kmdb_distance* d, const void* row_ptr_dev, const void* col_dev, const void* val_dev, uint64_t n_cols, uint64_t col_shift);
int  kmdb_distance_take_csr_device(kmdb_distance* d, const void* row_ptr_dev, const void* col_dev, const void* val_dev, size_t nr,
                                   const uint32_t* row_kmers /* [nr], host */, const char* const* names /* [nr] */);
int  kmdb_distance_csr_rows(kmdb_distance* d, uint64_t row_lo, uint64_t row_hi, kmdb_distance_out* out);
int  kmdb_distance_csr_device(kmdb_distance* d, const void** row_ptr_dev, const void** col_dev, const void** val_dev, uint64_t* nr);
int  kmdb_distance_csr_row_ptr(kmdb_distance* d, uint64_t* out /* [nr + 1], host */);
int  kmdb_distance_parts_stats_get(const kmdb_distance* d, kmdb_distance_parts_stats* out);
void kmdb_distance_out_free(kmdb_distance_out* out);
void kmdb_distance_free(kmdb_distance* d);
int  kmdb_distance_stats_get(const kmdb_distance* d, kmdb_distance_stats* out);
/* Double2PChar with six decimals as the distance console prints a measure (conversion.h:167-219, 262-268): 0 and -0.0 are "0"; anything else
 * is the sign, then x = (uint64)(|v| * 1e6 + 0.5) as x / 10^6 '.' x % 10^6 in six digits.  Returns the length; no terminator; out holds 40 bytes. */
size_t kmdbh_format_measure(double v, char* out);

/* CSV text (console_all2all.cpp:40-78, console_new2all.cpp:99-160, conversion.h:246-298).
 * Each returns bytes written to `out` (caller sizes it: 10000 + 100*N like the reference). */
size_t kmdbh_format_header(const kmdbh_db* db, char* out, size_t cap);
size_t kmdbh_format_dense_row(const char* name, uint64_t kmers, const uint32_t* row, size_t n, char* out);
size_t kmdbh_format_sparse_row(const char* name, uint64_t kmers, const uint32_t* cols, const uint32_t* vals, size_t n, char* out);

#ifdef __cplusplus
}
#endif
#endif /* KMDB_AMD_H */
