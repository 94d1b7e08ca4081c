// engine_state.h — the HBM-resident database shared by the translation units of libkmdb_amd.so
// (engine.hip: entry points, layout.hip: upload, a2a_v1.hip: scatter kernels, a2a_blocks.hip: block-record pipeline, a2a_rows.hip: a band of
// the matrix's rows, a2a_band.hip: the same band summed in LDS tiles and a run walked in bands (band_select.h: what the two share), a2a_rows_records.hip: the same band through the
// block-record pipeline, node_arrays.hip: the node arrays of the v1 kernels and of new2all).
#pragma once
#include "kmdb_amd.h"
#include "kmdb_internal.h"

#include <thread>
#include "engine_internal.h"
#include "dev_mem.h"

#include <hip/hip_runtime.h>

#include <cstdint>
#include <memory>
#include <string>
#include <utility>
#include <vector>

struct Segment { uint32_t first, end; };

// the block-record pipeline's working set and memory between calls: defined, made and destroyed in a2a_blocks.hip
struct BlocksState;
struct BlocksStateDelete { void operator()(BlocksState* b) const; };

struct kmdb_db {
    int device = 0;
    uint64_t N = 0, P = 0;
    uint32_t kmer_length = 0;
    // ---- structural layout (upload): a pure format conversion of the on-disk pattern section, DFS pre-order.
    // Nothing here depends on a decoded sample id.
    DevBuf<uint2> k0in;             // [P] local-list head of the node: l, last id, stream bits (packed: kmdb_k0_pack)
    DevBuf<uint32_t> bitrel;        // [P] stream position relative to blkbase[i / 256]
    DevBuf<uint64_t> blkbase;       // [P / 256]
    DevBuf<uint64_t> bits;          // gamma streams bit-packed back to back
    uint64_t n_bit_words = 0;
    uint32_t short_max_ids = 48;                    // (= KMDB_SHORT_MAX_IDS) local lists of more ids (or of more than KMDB_SHORT_MAX_BITS stream bits) are decoded by the long launch
    DevBuf<uint32_t> nl;            // [P] n = ids of the node's full list
    DevBuf<int32_t> parent;         // [P] DFS index of the parent, -1 for roots
    DevBuf<uint32_t> w;             // [P+1] on-disk num_kmers truncated to u32 (last = 0); a prefix shard keeps only its own k-mers
    DevBuf<uint16_t> dflag;         // [P] root path length (root = 1) | has-child << 15
    DevBuf<uint32_t> sub_end;       // [P] DFS index one past the node's subtree
    DevBuf<uint32_t> long_nodes;    // nodes whose stream does not fit the short decoder, most work first
    uint32_t n_long = 0;
    // the short decode launch's work order (kmdb_k0_key): the nodes of every window of k0_window consecutive DFS nodes by decreasing key
    DevBuf<uint16_t> k0_order;      // [windows][k0_window] offset of the node inside its window; the part-filled last window is padded (key 0)
    DevBuf<uint32_t> k0_live;       // [windows] nodes of the window the short launch decodes: the first k0_live[w] entries of its order
    uint32_t k0_window = 256;       // a power of two from 256 to 4096, fixed at upload (KMDB_K0_WINDOW)
    uint32_t nseg_nodes = 2048;     // nodes per slice of the DFS stream (one wave each)
    uint32_t n_nsegs = 0;
    DevBuf<uint32_t> nseg_anc;      // [n_nsegs][chain_cap] root path of every slice's first node
    DevBuf<uint32_t> nseg_anc_n;
    uint32_t chain_cap = 8;         // chain slots per wave = longest root path, rounded up
    uint32_t max_depth = 0, max_n = 0;
    // db2db's list store (db2db.hip): full sample list of every pattern as a bit set, list_sets_nb words per pattern
    DevBuf<unsigned long long> list_sets;
    uint32_t list_sets_nb = 0;
    bool list_sets_tried = false;
    // new2all's run index (new2all.hip): the local list of every node as runs of consecutive ids (start | length << rs), built on the
    // first new2all call of the handle
    DevBuf<uint32_t> rl_ofs;        // [P + 1]
    DevBuf<uint32_t> rl_runs;
    DevBuf<uint4> rl_node;          // [P] the node as the walk reads it, one 16-byte load: subtree end, parent, first run (or the id of a one-id list), l | runs << 16
    bool rl_tried = false;
    bool chain_ok = false;          // root paths fit the chain table of the emit kernel
    // ---- the block-record pipeline (a2a_blocks.hip): its working set and what it remembers between calls are its own (BlocksState); the handle
    // keeps what the other translation units read
    uint32_t width = 64;            // sample ids per block, picked by kmdb_blocks_prepare from a sampled estimate
    std::unique_ptr<BlocksState, BlocksStateDelete> blocks;   // made by kmdb_blocks_prepare, destroyed by kmdb_blocks_release
    uint64_t blocks_bytes_counted = 0;   // the block-record pipeline's share of stats.device_bytes as last counted (its arrays grow inside calls)
    bool last_call_sized = false;   // the last call measured launch sizes (first call on a handle / a new emit range: extra host syncs)
    // ---- v1 kernels (A/B reference, fallback) and new2all: built lazily on the device from the arrays above
    // host staging buffers of the upload, given back by a helper thread after the first call (or when the handle is freed):
    // unmapping them costs 0.3 s (the HIP runtime had them registered for the copies) and blocks every hipMalloc meanwhile
    std::vector<std::pair<void*, size_t>> staging;
    std::vector<std::pair<void*, size_t>> staging_kept;   // one-shot handle: regions whose pages were dropped but that stay mapped until kmdb_db_free
    std::thread staging_thread;    // gives the staging buffers back (kmdb_release_staging); joined by kmdb_db_settle / kmdb_db_free
    bool one_shot = false;         // KMDB_FLAG_ONE_SHOT at upload: the staging buffers stay until the handle is freed
    bool v1_ready = false;          // the arrays below exist (all of them)
    DevBuf<uint4> meta;             // {n, l, last_id, nbits} per node, DFS order
    DevBuf<uint64_t> bitpos;        // absolute bit offset of the node's gamma stream
    // new2all: index into the gamma streams of the nodes with more than KMDB_CK_IDS local ids — every KMDB_CK_IDS-th id and
    // the bit position of the code after it, so that the lanes of a workgroup decode one long list in pieces
    DevBuf<uint32_t> ck_ofs;        // [P + 1] first checkpoint of the node (a node with a short list has none)
    DevBuf<uint64_t> ck_bit;
    DevBuf<uint32_t> ck_id;
    DevBuf<uint32_t> wprefix;       // P+1, exclusive scan of w (recomputed by every call)
    DevBuf<Segment> segs;
    uint32_t n_segs = 0;
    DevBuf<void> v1_scan_tmp;
    size_t v1_scan_tmp_bytes = 0;
    DevBuf<uint32_t> stack_scratch;     // global kernel: per-wave id stacks
    size_t stack_scratch_words = 0;
    DevBuf<unsigned long long> v1_counters;      // [0] tile flushes
    // ---- a band of rows (a2a_rows.hip): made on the first band call of the handle; the id stacks are stack_scratch above
    DevBuf<uint32_t> rows_sel;          // [P] the nodes selected by the last band call
    DevBuf<unsigned long long> rows_counters;    // [0] nodes selected, [1] nodes with a band row, [2] cell additions
    uint64_t rows_bytes_counted = 0;    // the two arrays' share of stats.device_bytes as last counted
    kmdb_all2all_rows_stats rows_stats{};        // the last band call on the handle (kmdb_all2all_rows_stats_get)
    // ---- the tiled band call (a2a_band.hip): made on the first tiled call of the handle, grown when a call needs more
    DevBuf<uint32_t> band_sel;          // [P] the nodes selected by the last tiled call
    DevBuf<unsigned long long> band_counters;    // [0] nodes selected, [1] nodes with a hit, [2] hits, [3] runs, [4] cell additions
    DevBuf<uint32_t> band_rows;         // [3][rows + 1] per row of the band: hit count, its exclusive sum, the write cursor
    uint64_t band_rows_cap = 0;         // rows + 1 the three tables hold
    DevBuf<uint32_t> band_hits;         // [hits] the node of every hit, grouped by row
    uint64_t band_hits_cap = 0;
    DevBuf<uint4> band_jobs;            // [jobs] {row, first column of the tile, first hit, hits}
    uint64_t band_jobs_cap = 0;
    DevBuf<void> band_scan_tmp;         // rocPRIM's temporary storage for the scan of the hit counts
    size_t band_scan_tmp_bytes = 0;
    DevEvent band_ev;                   // between the hit passes and the apply launch (ev[0 .. 3] are the call's other marks)
    uint64_t band_bytes_counted = 0;    // these arrays' share of stats.device_bytes as last counted
    kmdb_all2all_rows_tiled_stats band_stats{};  // the last tiled call on the handle (kmdb_all2all_rows_tiled_stats_get)
    kmdb_all2all_banded_stats banded_stats{};    // the last banded call on the handle (kmdb_all2all_banded_stats_get)
    // ---- the band call through the block-record pipeline (a2a_rows_records.hip; its device state is the pipeline's own)
    kmdb_all2all_rows_records_stats rr_stats{};  // the last such call on the handle (kmdb_all2all_rows_records_stats_get)
    kmdb_all2all_banded_records_stats banded_rr_stats{};   // the last banded call on the records path (kmdb_all2all_banded_records_stats_get)
    // ---- band emit (a2a_blocks.hip): the pipeline's second state, keyed relative to a band's first stream — made by the handle's first band-emit call,
    // made anew when a later band needs more; the whole-matrix state above is not touched by it
    std::unique_ptr<BlocksState, BlocksStateDelete> band_blocks;
    std::string band_fallback_reason;   // why the last band-emit call gave up inside the pipeline ("" = it did not); fallback_reason stays the whole matrix's
    uint64_t band_max_streams = 0;      // KMDB_BAND_MAX_STREAMS as read with it (0: unset, 0 or no number — the limit is 2^22)
    int band_emit_mode = -2;            // KMDB_BAND_EMIT as read at the handle's first records band call: -1 unset, 0, 1 (-2: not read yet)
    kmdb_all2all_rows_band_emit_stats be_stats{};   // the last records band call on the handle (kmdb_all2all_rows_band_emit_stats_get)
    // hashtables (new2all)
    uint64_t n_buckets = 0;
    DevBuf<uint64_t> bucket_offset;
    DevBuf<uint64_t> slots;
    DevBuf<uint32_t> pid2dfs;       // original pattern id -> DFS index
    // query shard (kmdb_db_upload_query_shard; qs_count > 1): the tables above are those of the buckets b with b % qs_count == qs_index only
    // (local bucket b / qs_count), their values are DFS indices of this handle's own layout, and there is no pid2dfs
    uint32_t qs_index = 0, qs_count = 0;
    hipStream_t stream = nullptr;
    hipStream_t stream2 = nullptr;  // side stream: the stream chunks are sorted and applied next to the wide kernel
    DevEvent ev_side[2], ev[4];
    DevEvent ev_k[4];               // after decode / narrow / wide / apply
    kmdb_stats stats{};
    kmdb_db2db_stats d2_stats{};        // the last db2db call with this handle as the row database (kmdb_db2db_stats_get)
    kmdb_new2all_sparse_stats n2s_stats{};   // the last sparse new2all call on the handle (kmdb_new2all_sparse_stats_get)
    kmdb_sample_stats sample_stats{};   // the last sampled call on the handle (kmdb_db_sample_stats)
    kmdb_sample_stats d2_sample_stats{};   // the last sampled db2db / rectangle call with this handle as the row database (kmdb_db2db_sample_stats_get)
    kmdb_sample_stats n2a_sample_stats{};   // the last sampled new2all / query-rows call on the handle (kmdb_new2all_sample_stats_get)
    bool blocks_prepared = false;   // width estimate + working set of the block-record pipeline exist (made at upload for all2all
                                    // uploads, on the first all2all call for uploads that carry hashtables: new2all / db2db use)
    std::string fallback_reason;    // why the block-record pipeline cannot take this database ("" = it can)
};

// K0 decodes a node in the coalesced DFS-order launch when its stream is short enough to sit in three
// registers; the others (a few percent) go to a second launch, longest list first.
// Head of a node's local list as K0 reads it, 8 bytes: l and the last id in 20 bits each, the length of the gamma stream in 24 (l ids below
// 2^20 need fewer than 1.6 * 2^20 stream bits: a delta of 2 costs 3 bits, the dearest per unit of id range).  Sample ids are therefore
// below KMDB_MAX_SAMPLES; the upload checks all three fields.
constexpr uint32_t KMDB_MAX_STREAM_BITS = 1u << 24;            // (KMDB_ID_BITS, KMDB_MAX_SAMPLES: engine_internal.h)
__host__ __device__ inline uint2 kmdb_k0_pack(uint32_t l, uint32_t last, uint32_t nbits) {
    uint2 r;
    r.x = l | ((nbits >> 12) << KMDB_ID_BITS); r.y = last | ((nbits & 0xFFFu) << KMDB_ID_BITS);
    return r;
}
__host__ __device__ inline uint32_t kmdb_k0_l(uint2 km) { return km.x & (KMDB_MAX_SAMPLES - 1u); }
__host__ __device__ inline uint32_t kmdb_k0_last(uint2 km) { return km.y & (KMDB_MAX_SAMPLES - 1u); }
__host__ __device__ inline uint32_t kmdb_k0_bits(uint2 km) { return ((km.x >> KMDB_ID_BITS) << 12) | (km.y >> KMDB_ID_BITS); }
constexpr uint32_t KMDB_SHORT_MAX_IDS = 48, KMDB_SHORT_MAX_BITS = 128;     // (ids: the default of kmdb_db.short_max_ids, KMDB_SHORT_IDS at upload.  Measured, profiles/r05_j4: 32 -> 48 ids takes 0.14 ms off the decode at c2 and 0.5 ms at 10 000 samples — the lists of a clade of 50 fit —, 56 and 64 lose: the short launch walks a list that spans 64 ids or more twice)
__host__ __device__ inline bool kmdb_long_node(uint32_t l, uint32_t num_bits, uint32_t max_ids) { return l > max_ids || num_bits > KMDB_SHORT_MAX_BITS; }
// The short launch's work per node, from the header fields alone (no stream bit is read): the same for every call on a database, so the layout
// sorts by it once.  0: not the short launch's (a long node; the padding of the last window) — sorts last, outside the live count.
// 1: a single id, or an empty list (its p0_info = 0 is this launch's to write, in every call: K1n reads it).  2: a single run — l - 1 deltas in l - 1 stream bits are all 1 —; neither reads its stream.  Above: 2 + the stream bits
// beyond one per delta (~ the codes that are not "0"), capped at 63.
__host__ __device__ inline bool kmdb_k0_run_only(uint32_t l, uint32_t num_bits) { return l > 1 && num_bits <= l - 1u; }
__host__ __device__ inline uint32_t kmdb_k0_key(uint32_t l, uint32_t num_bits, uint32_t max_ids) {
    if (kmdb_long_node(l, num_bits, max_ids)) return 0u;
    if (l <= 1) return 1u;
    if (kmdb_k0_run_only(l, num_bits)) return 2u;
    const uint32_t extra = num_bits - (l - 1u);
    return extra > 61u ? 63u : 2u + extra;
}
constexpr uint32_t KMDB_K0_WINDOW_MIN = 256, KMDB_K0_WINDOW_MAX = 4096, KMDB_K0_WINDOW_DEFAULT = 256;       // (wider windows run fewer instructions and take longer: DESIGN.md §8)
constexpr int KMDB_CHAIN_MAX = 4096;  // longest root path (in nodes) the chain table of the narrow kernel holds (20 B of LDS per node and wave:
                                      // the deeper the tree, the fewer waves share a workgroup)

// ---- layout.hip: host conversion + device layout of the view (fills the structural arrays and stats)
// sel == nullptr: the whole view at its on-disk weights; else the nodes and weights of one part (a prefix shard, a tree range)
int kmdb_layout_upload(kmdb_db* db, const kmdb_db_view* v, int with_hashtables, const kmdb_kept_nodes* sel);
// kmdb_db_upload_shard with a plan the caller made for several shards at once (node.hip); plan == nullptr: the shard is planned by itself
int kmdb_db_upload_planned(const kmdb_db_view* v, const kmdb_opts* opts, int with_hashtables, uint32_t shard_index, uint32_t shard_count, kmdb_shard_plan* plan,
                           kmdb_db** out);
// kmdb_db_upload_query_shard with such a plan
int kmdb_db_upload_query_planned(const kmdb_db_view* v, const kmdb_opts* opts, uint32_t shard_index, uint32_t shard_count, kmdb_shard_plan* plan, kmdb_db** out);
// kmdb_db_upload_range with a plan the caller made for all ranges (node.hip)
int kmdb_db_upload_range_planned(const kmdb_db_view* v, const kmdb_opts* opts, uint32_t range_index, const kmdb_range_plan* plan, kmdb_db** out);

// ---- a2a_v1.hip: tree-form scatter kernels (LDS tile / HBM atomics); M is zeroed, wprefix is scanned
int kmdb_v1_run(kmdb_db* db, uint32_t* M, uint32_t seg_begin, uint32_t seg_end, uint32_t flags, hipStream_t st);

// ---- a2a_blocks.hip: block-record pipeline
// upload-time: block width from a sampled estimate, working-set allocation
int kmdb_blocks_prepare(kmdb_db* db);
// per call: decode, narrow / wide emit, apply — everything that depends on a sample id happens here
// band == nullptr: M is the whole triangle.  Else M holds the rows [row_lo, row_hi) only — `cells` words, the first of them cell `cell_lo` = tri(row_lo) of
// the triangle: decode, emit and sort run whole, the apply stage culls the block rows outside the band and windows its write-back (a2a_rows_records.hip)
// emit: the band-emit form — the call runs on the handle's second state (kmdb_blocks_band_prepare fitted it to this band): the emit kernels write the records of
// the band's block rows alone, keyed relative to its first stream, and every later stage works on the band's streams only
struct kmdb_band_desc { uint64_t row_lo, row_hi, cell_lo, cells; bool emit = false; };
int kmdb_blocks_run(kmdb_db* db, uint32_t* M, uint32_t emit_lo, uint32_t emit_hi, hipStream_t st, const kmdb_band_desc* band = nullptr);
// A give-up inside the run (the pools at what they can index, a list lost by the wide kernel) is written to the state that ran and published when the
// call returns 0: to db->fallback_reason by the whole-matrix state (sticky: the handle skips the pipeline from then on), to db->band_fallback_reason by
// the band-emit state ("" again at its next call).
// ---- band emit (a2a_blocks.hip; a2a_rows_records.hip decides which form a band call takes)
// why band emit cannot take the band g ("": it can); the state made or fitted for g, band_cells = its cells
std::string kmdb_blocks_band_refusal(const kmdb_db* db, const kmdb_band_geometry* g);
int kmdb_blocks_band_prepare(kmdb_db* db, const kmdb_band_geometry* g, uint64_t band_cells);
// ---- what a band caller reads of one of the two states (band_state: the band-emit state; else the whole-matrix state)
// the narrow kernel's mode, asked before the run (KMDB_K1N_MODE; 1 writes the matrix itself): of the state, -1 without a whole-matrix state, as a
// band-emit state yet to be made would read it (the whole-matrix state of a collection beyond 2^22 block pairs never got as far as its switches)
int kmdb_blocks_k1n_mode(const kmdb_db* db, bool band_state);
// the state's device bytes (kmdb_blocks_device_bytes is the sum of both)
uint64_t kmdb_blocks_state_bytes(const kmdb_db* db, bool band_state);
// the state's last band call; units: stream jobs, window runs of stream chunks, slices' tiles of first-block records, second-level tiles of the apply stage
struct kmdb_blocks_band_units { uint64_t jobs, jobs_run, runs, runs_run, slices, slices_run, tiles, tiles_run; };
struct kmdb_blocks_band_info { uint32_t key_bits, row_mode, l2_on, attempts, slices; uint64_t records, est_records; kmdb_blocks_band_units units; };
kmdb_blocks_band_info kmdb_blocks_band_last(const kmdb_db* db, bool band_state);
void kmdb_blocks_release(kmdb_db* db);
uint64_t kmdb_blocks_device_bytes(const kmdb_db* db);
// ---- the lines every caller of the pipeline repeats (engine.hip)
// kmdb_blocks_prepare at the handle's first call that needs it, its arrays entered into stats.device_bytes
int kmdb_blocks_ensure_prepared(kmdb_db* db);
// the last run's stage times from the call's events: ms[0 .. 3] = decode (from ev[1]), narrow emit, wide emit, apply
int kmdb_blocks_stage_ms(kmdb_db* db, float ms[4]);
// a share of stats.device_bytes whose arrays are made and grow inside calls, counted again: `counted` is what stats holds of it, `now` what is resident
inline void kmdb_recount_bytes(kmdb_db* db, uint64_t& counted, uint64_t now) {
    db->stats.device_bytes = db->stats.device_bytes - counted + now;
    counted = now;
}
// what the last kmdb_blocks_run found (the statistics of the call), and the tiles it added to: [block pairs] != 0, or null without a working set
struct kmdb_blocks_counts { uint64_t records, direct; uint32_t wide, chunks, joined; };
kmdb_blocks_counts kmdb_blocks_last_counts(const kmdb_db* db);
const unsigned char* kmdb_blocks_tile_touched(const kmdb_db* db);
// ---- node_arrays.hip: v1 / new2all node arrays, derived on the device from the compact layout
int kmdb_ensure_v1_arrays(kmdb_db* db);

// layout.hip: unmap db->staging piece by piece on a detached thread
void kmdb_release_staging(kmdb_db* db);
