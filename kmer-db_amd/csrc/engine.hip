// engine.hip — C-ABI entry points of the MI355X (gfx950) engine behind include/kmdb_amd.h.
//
// Replaces the reference's SimilarityCalculator::all2all / all2all_sp call sites
// (reference src/similarity_calculator.cpp:42-438, 442-657; console_all2all.cpp:34, console_all2all_sparse.cpp:44).
//   layout.hip      kmdb_db_upload: on-disk pattern section -> DFS pre-order layout in HBM (format conversion only)
//   a2a_blocks.hip  the block-record pipeline: every decode / count / placement step inside the call
//   a2a_v1.hip      tree-form scatter kernels: A/B reference behind flags, and the (announced) fallback
// uint32 adds wrap and commute, so any schedule is bit-exact with the reference.
#include "device_common.h"
#include "engine_internal.h"
#include "cell_filter.h"
#include "sample_rows.h"

#include "prim.h"

#include <sys/mman.h>
#include <algorithm>
#include <cmath>
#include <functional>
#include <limits>
#include <thread>
#include <vector>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>

// ------------------------------------------------------------------------------------------
// error plumbing
// ------------------------------------------------------------------------------------------
static thread_local std::string g_last_error;
int kmdb_set_error(const std::string& msg) { g_last_error = msg; return 1; }
extern "C" const char* kmdb_last_error(void) { return g_last_error.c_str(); }
extern "C" int kmdb_abi_version(void) { return KMDB_ABI_VERSION; }
static_assert(KMDB_ABI_THIS == KMDB_ABI_VERSION, "kmdb_internal.h: kmdb_abi_compatible names the header's version");

extern "C" int kmdb_device_prepare(int32_t device) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || device < 0 || device >= n) { (void)hipGetLastError(); return kmdb_set_error("kmdb_device_prepare: no such HIP device"); }
    HIP_TRY(hipSetDevice(device));
    void* p = nullptr;
    hipStream_t s = nullptr;
    HIP_TRY(hipMalloc(&p, 1 << 20));
    HIP_TRY(hipStreamCreate(&s));
    HIP_TRY(hipMemsetAsync(p, 0, 1 << 20, s));
    HIP_TRY(hipStreamSynchronize(s));
    HIP_TRY(hipStreamDestroy(s));
    HIP_TRY(hipFree(p));
    return 0;
}

extern "C" int kmdb_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) { (void)hipGetLastError(); return 0; }
    int ok = 0;
    for (int i = 0; i < n; ++i) {
        hipDeviceProp_t p;
        if (hipGetDeviceProperties(&p, i) == hipSuccess && std::strncmp(p.gcnArchName, "gfx950", 6) == 0) ++ok;
    }
    return ok;
}

namespace {
// ------------------------------------------------------------------------------------------
// dense -> CSR compaction for the sparse entry point
// ------------------------------------------------------------------------------------------
// The columns of row `row` inside the flat cell range [cell_lo, cell_hi) of the lower triangle (row i at i (i - 1) / 2,
// reference src/array.h:136-140): [j0, j1).  M points at cell `cell_lo`.
__device__ __forceinline__ void row_span(uint64_t row, uint64_t cell_lo, uint64_t cell_hi, uint64_t& j0, uint64_t& j1) {
    const uint64_t b = tri64(row), e = b + row;
    j0 = cell_lo > b ? cell_lo - b : 0;
    j1 = cell_hi < e ? (cell_hi > b ? cell_hi - b : 0) : row;
    if (j0 > j1) j0 = j1;
}
__global__ void row_nnz_kernel(const uint32_t* __restrict__ M, uint64_t row_lo, uint64_t cell_lo, uint64_t cell_hi, unsigned long long* __restrict__ row_nnz,
                               const DevFilter f) {
    const uint64_t row = row_lo + blockIdx.x;
    const uint32_t* r = M + ((int64_t)tri64(row) - (int64_t)cell_lo);      // only cells of the range are touched
    uint64_t j0, j1;
    row_span(row, cell_lo, cell_hi, j0, j1);
    uint32_t c = 0;
    for (uint64_t j = j0 + threadIdx.x; j < j1; j += blockDim.x) c += dev_keep(f, r[j], (uint32_t)row, (uint32_t)j) ? 1u : 0u;
    __shared__ uint32_t red[256];
    red[threadIdx.x] = c;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) row_nnz[row] = red[0];
}

// one block per row, ordered compaction with a block-wide running offset
__global__ void row_compact_kernel(const uint32_t* __restrict__ M, uint64_t row_lo, uint64_t cell_lo, uint64_t cell_hi,
                                   const unsigned long long* __restrict__ row_ptr, uint32_t* __restrict__ col, uint32_t* __restrict__ val, const DevFilter f) {
    const uint64_t row = row_lo + blockIdx.x;
    const uint32_t* r = M + ((int64_t)tri64(row) - (int64_t)cell_lo);
    uint64_t jb, je;
    row_span(row, cell_lo, cell_hi, jb, je);
    __shared__ uint32_t wave_cnt[4];
    __shared__ unsigned long long running;
    if (threadIdx.x == 0) running = row_ptr[row];
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (uint64_t j0 = jb; j0 < je; j0 += blockDim.x) {
        const uint64_t j = j0 + threadIdx.x;
        uint32_t v = j < je ? r[j] : 0u;
        if (!dev_keep(f, v, (uint32_t)row, (uint32_t)j)) v = 0u;
        const unsigned long long bal = __ballot(v != 0);
        if (lane == 0) wave_cnt[wave] = (uint32_t)__popcll(bal);
        __syncthreads();
        uint32_t before = 0;
        for (uint32_t k = 0; k < wave; ++k) before += wave_cnt[k];
        const unsigned long long base = running;
        if (v) {
            const unsigned long long o = base + before + (uint32_t)__popcll(bal & ((1ull << lane) - 1ull));
            col[o] = (uint32_t)j;
            val[o] = v;
        }
        __syncthreads();
        if (threadIdx.x == 0) running = base + wave_cnt[0] + wave_cnt[1] + wave_cnt[2] + wave_cnt[3];
        __syncthreads();
    }
}


// The same two passes over the TOUCHED tiles only (reference: all2all_sp is O(nnz), src/similarity_calculator.cpp:596-638, compact2
// src/array.h:391-446): the apply kernels of the block-record pipeline flag every block pair (X, Y) they add to (kmdb_db.tile_touched);
// a row of block row X looks at the flags of its X + 1 column blocks, 64 at a time, and reads only the cells of flagged tiles.  One
// wave per row (a tile holds at most 64 columns: a lane each); the row's entries come out in ascending column order.
struct TileSkip { const unsigned char* touched; uint32_t width; };
template <bool COMPACT>
__global__ __launch_bounds__(64) void row_tiles_kernel(const uint32_t* __restrict__ M, uint64_t n_rows, const TileSkip ts, unsigned long long* __restrict__ row_nnz,
                                                       const unsigned long long* __restrict__ row_ptr, uint32_t* __restrict__ col, uint32_t* __restrict__ val,
                                                       const DevFilter f) {
    const uint64_t row = blockIdx.x;
    if (row >= n_rows) return;
    const uint32_t lane = threadIdx.x;
    const uint32_t X = (uint32_t)(row / ts.width);
    const uint32_t* r = M + tri64(row);
    const unsigned char* flags = ts.touched + (size_t)X * (X + 1) / 2;
    unsigned long long out = COMPACT ? row_ptr[row] : 0ull;
    uint32_t count = 0;
    for (uint32_t Y0 = 0; Y0 <= X; Y0 += 64) {
        const uint32_t Yl = Y0 + lane;
        unsigned long long m = __ballot(Yl <= X && flags[Yl] != 0);
        while (m) {
            const uint32_t Y = Y0 + (uint32_t)__builtin_ctzll(m);
            m &= m - 1;
            const uint64_t j = (uint64_t)Y * ts.width + lane;
            uint32_t v = (lane < ts.width && j < row) ? r[j] : 0u;
            if (!dev_keep(f, v, (uint32_t)row, (uint32_t)j)) v = 0u;
            const unsigned long long bal = __ballot(v != 0);
            if (COMPACT) {
                if (v) { const unsigned long long o = out + (uint32_t)__popcll(bal & ((1ull << lane) - 1ull)); col[o] = (uint32_t)j; val[o] = v; }
                out += (uint32_t)__popcll(bal);
            } else count += (uint32_t)__popcll(bal);
        }
    }
    if (!COMPACT && lane == 0) row_nnz[row] = count;
}

}  // namespace

// ------------------------------------------------------------------------------------------
// upload (layout.hip does the conversion)
// ------------------------------------------------------------------------------------------
namespace {

// The handle of a database on `device`: streams and events, the layout (layout(db): kmdb_layout_upload, or kmdb_layout_from_device), the
// working set of all2all for a handle without hashtables, the stats.  prepare_ms (may be null): wall clock of kmdb_blocks_prepare.
template <class Layout>
int handle_make(uint64_t N, uint64_t P, uint32_t kmer_length, int device, const kmdb_opts* opts, int with_hashtables, std::chrono::steady_clock::time_point t0,
                Layout&& layout, kmdb_db** out, double* prepare_ms = nullptr) {
    auto* db = new kmdb_db();
    db->device = device; db->N = N; db->P = P; db->kmer_length = kmer_length;
    db->one_shot = opts && (opts->flags & KMDB_FLAG_ONE_SHOT);
    auto fail = [&]() { kmdb_db_free(db); return 1; };
    if (hipStreamCreate(&db->stream) != hipSuccess) { kmdb_set_error("hipStreamCreate failed"); return fail(); }
    for (auto& e : db->ev) if (e.create()) return fail();
    for (auto& e : db->ev_k) if (e.create()) return fail();
    if (hipStreamCreate(&db->stream2) != hipSuccess) { kmdb_set_error("hipStreamCreate failed"); return fail(); }
    for (auto& e : db->ev_side) if (e.create(hipEventDisableTiming)) return fail();
    // KMDB_VERBOSE: the four parts of the upload as wholes (the layout and the preparation print their own phases; what those
    // leave out — the release of their temporaries, the first use of the device by the process — shows up here)
    const bool verbose = getenv("KMDB_VERBOSE") != nullptr;
    auto t_mark = t0;
    auto part = [&](const char* what) {
        if (!verbose) return;
        const auto now = std::chrono::steady_clock::now();
        fprintf(stderr, "[kmdb] upload part: %-40s %.3f s\n", what, std::chrono::duration<double>(now - t_mark).count());
        t_mark = now;
    };
    part("streams + events (first use of the device)");
    if (layout(db)) return fail();
    part("layout incl. release of its temporaries");
    // the working set of all2all: now for an all2all upload, on the first all2all call for a new2all / db2db upload
    const auto t_prep = std::chrono::steady_clock::now();
    if (!with_hashtables && kmdb_blocks_prepare(db)) return fail();
    part("preparation of the all2all working set");
    if (hipStreamSynchronize(db->stream) != hipSuccess) { kmdb_set_error("kmdb_db_upload: device error"); return fail(); }
    part("final wait");
    if (prepare_ms) *prepare_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_prep).count();
    db->blocks_bytes_counted = kmdb_blocks_device_bytes(db);
    db->stats.device_bytes += db->blocks_bytes_counted;
    db->stats.width = db->width;
    db->stats.upload_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    if (getenv("KMDB_VERBOSE")) fprintf(stderr, "[kmdb] upload: total %.3f s (%llu patterns, %llu samples)\n", db->stats.upload_ms * 1e-3,
                                        (unsigned long long)P, (unsigned long long)N);
    *out = db;
    return 0;
}

// plan / rplan: the part of the database this handle holds — shard `shard_index` of `shard_count` prefix-bucket shards (plan == nullptr: planned
// here), or range `shard_index` of rplan's tree ranges; neither (shard_count 1): the whole database
int upload_impl(const kmdb_db_view* v, const kmdb_opts* opts, int with_hashtables, uint32_t shard_index, uint32_t shard_count, kmdb_shard_plan* plan,
                const kmdb_range_plan* rplan, kmdb_db** out, bool query_shard = false) {
    *out = nullptr;
    if (!v || !kmdb_abi_compatible(v->abi_version)) return kmdb_set_error("kmdb_db_upload: bad view / ABI version");
    if (opts && (opts->flags & ~KMDB_FLAG_ALL)) return kmdb_set_error("kmdb_db_upload: unknown bits in kmdb_opts.flags");
    const uint64_t P = v->n_patterns, N = v->n_samples;
    if (!P) return kmdb_set_error("kmdb_db_upload: the view holds no pattern, not even the empty one (a header-only image of kmdb_build_finish_device carries names and counts only)");
    if (P >= (1ull << 31)) return kmdb_set_error("kmdb_db_upload: more than 2^31 patterns");
    if (N >= KMDB_MAX_SAMPLES) return kmdb_set_error("kmdb_db_upload: " + std::to_string(KMDB_MAX_SAMPLES) + " samples or more are not supported (sample ids take " + std::to_string(KMDB_ID_BITS) + " bits in the device layout)");
    if (shard_count == 0 || shard_index >= shard_count) return kmdb_set_error("kmdb_db_upload_shard: shard_index >= shard_count");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) {
        (void)hipGetLastError();
        return kmdb_set_error("kmdb_db_upload: no HIP device available (the engine has no CPU fallback)");
    }
    const int device = opts ? opts->device : 0;
    const auto t0 = std::chrono::steady_clock::now();
    HIP_TRY(hipSetDevice(device));
    // a prefix shard uploaded by itself plans itself: its k-mer counts from its own buckets, its nodes by one sweep (host_shards.cpp)
    kmdb_shard_plan own_plan;
    if (shard_count > 1 && !plan && !rplan) {
        if (kmdb_shard_plan_build(v, shard_count, std::vector<uint32_t>{shard_index}, &own_plan)) return 1;
        plan = &own_plan;
    }
    return handle_make(N, P, v->kmer_length, device, opts, with_hashtables, t0, [&](kmdb_db* db) {
        kmdb_kept_nodes sel;
        if (rplan) sel = kmdb_kept_of_range(*rplan, shard_index);
        else if (plan && shard_count > 1) sel = kmdb_kept_of_shard(*plan, shard_index);
        if (query_shard && plan && shard_count > 1) { sel.what = "query shard"; sel.qs_index = shard_index; sel.qs_count = shard_count; }
        const bool part_of_db = rplan || (plan && shard_count > 1);
        const int rc = kmdb_layout_upload(db, v, with_hashtables, part_of_db ? &sel : nullptr);
        if (plan && shard_count > 1) plan->release_weights(shard_index);      // the shard's P counters go back
        return rc;
    }, out);
}

}  // namespace

extern "C" int kmdb_db_upload(const kmdb_db_view* v, const kmdb_opts* opts, int with_hashtables, kmdb_db** out) {
    return upload_impl(v, opts, with_hashtables, 0, 1, nullptr, nullptr, out);
}
extern "C" int kmdb_db_upload_shard(const kmdb_db_view* v, const kmdb_opts* opts, int with_hashtables, uint32_t shard_index, uint32_t shard_count,
                                    kmdb_db** out) {
    return upload_impl(v, opts, with_hashtables, shard_index, shard_count, nullptr, nullptr, out);
}
// a query shard: the prefix shard's pruned tree with the slots of its own buckets (layout.hip)
int kmdb_db_upload_query_planned(const kmdb_db_view* v, const kmdb_opts* opts, uint32_t shard_index, uint32_t shard_count, kmdb_shard_plan* plan, kmdb_db** out) {
    if (!out) return kmdb_set_error("kmdb_db_upload_query_shard: null argument");
    *out = nullptr;
    if (!v || !kmdb_abi_compatible(v->abi_version)) return kmdb_set_error("kmdb_db_upload_query_shard: bad view / ABI version");
    if (shard_count == 0 || shard_count > KMDB_MAX_SHARDS) return kmdb_set_error("kmdb_db_upload_query_shard: shard_count must be between 1 and " + std::to_string(KMDB_MAX_SHARDS));
    if (shard_index >= shard_count) return kmdb_set_error("kmdb_db_upload_query_shard: shard_index >= shard_count");
    if (shard_count == 1) return kmdb_db_upload(v, opts, 1, out);
    if (!v->n_patterns) return kmdb_set_error("kmdb_db_upload_query_shard: the view holds no pattern, not even the empty one (a header-only image of kmdb_build_finish_device carries names and counts only)");
    if (!v->n_buckets) return kmdb_set_error("kmdb_db_upload_query_shard: the view carries no hashtables (load the database with mode Everything)");
    return upload_impl(v, opts, 1, shard_index, shard_count, plan, nullptr, out, true);
}
extern "C" int kmdb_db_upload_query_shard(const kmdb_db_view* v, const kmdb_opts* opts, uint32_t shard_index, uint32_t shard_count, kmdb_db** out) {
    return kmdb_db_upload_query_planned(v, opts, shard_index, shard_count, nullptr, out);
}
extern "C" int kmdb_db_upload_range(const kmdb_db_view* v, const kmdb_opts* opts, uint32_t range_index, uint32_t range_count, kmdb_db** out) {
    if (!out) return kmdb_set_error("kmdb_db_upload_range: null argument");
    *out = nullptr;
    if (!v || !kmdb_abi_compatible(v->abi_version)) return kmdb_set_error("kmdb_db_upload_range: bad view / ABI version");
    if (range_count == 0 || range_count > KMDB_MAX_SHARDS) return kmdb_set_error("kmdb_db_upload_range: range_count must be between 1 and " + std::to_string(KMDB_MAX_SHARDS));
    if (range_index >= range_count) return kmdb_set_error("kmdb_db_upload_range: range_index >= range_count");
    if (range_count == 1) return kmdb_db_upload(v, opts, 0, out);
    if (!v->n_patterns) return kmdb_set_error("kmdb_db_upload_range: the view holds no pattern, not even the empty one (a header-only image of kmdb_build_finish_device carries names and counts only)");
    // a range uploaded by itself plans all ranges (two sweeps over parent_id and num_samples, host_ranges.cpp): the cuts are a pure function
    // of the view and the count, so processes that each upload one range of the same database agree
    try {
        kmdb_range_plan plan;
        if (kmdb_range_plan_build(v, range_count, &plan)) return 1;
        return upload_impl(v, opts, 0, range_index, range_count, nullptr, &plan, out);
    } catch (const std::exception& e) {
        return kmdb_set_error(std::string("kmdb_db_upload_range: ") + e.what());
    }
}
int kmdb_db_upload_range_planned(const kmdb_db_view* v, const kmdb_opts* opts, uint32_t range_index, const kmdb_range_plan* plan, kmdb_db** out) {
    if (!out || !plan) return kmdb_set_error("kmdb_db_upload_range: null argument");
    if (range_index >= plan->n_ranges) return kmdb_set_error("kmdb_db_upload_range: range_index >= range_count");
    return upload_impl(v, opts, 0, range_index, plan->n_ranges, nullptr, plan, out);
}
int kmdb_db_upload_planned(const kmdb_db_view* v, const kmdb_opts* opts, int with_hashtables, uint32_t shard_index, uint32_t shard_count, kmdb_shard_plan* plan,
                           kmdb_db** out) {
    if (!out) return kmdb_set_error("kmdb_db_upload_shard: null argument");
    return upload_impl(v, opts, with_hashtables, shard_index, shard_count, plan, nullptr, out);
}

// the hand-off of a finished builder (build.hip): the refusals are those of upload_impl, with its messages
int kmdb_db_from_device(kmdb_layout_device_source* src, const kmdb_opts* opts, int with_hashtables, kmdb_db** out) {
    *out = nullptr;
    if (opts && (opts->flags & ~KMDB_FLAG_ALL)) return kmdb_set_error("kmdb_db_upload: unknown bits in kmdb_opts.flags");
    const uint64_t P = src->n_patterns, N = src->n_samples;
    if (!P) return kmdb_set_error("kmdb_db_upload: the view holds no pattern, not even the empty one");
    if (P >= (1ull << 31)) return kmdb_set_error("kmdb_db_upload: more than 2^31 patterns");
    if (N >= KMDB_MAX_SAMPLES) return kmdb_set_error("kmdb_db_upload: " + std::to_string(KMDB_MAX_SAMPLES) + " samples or more are not supported (sample ids take " + std::to_string(KMDB_ID_BITS) + " bits in the device layout)");
    const int device = opts ? opts->device : 0;
    const auto t0 = std::chrono::steady_clock::now();
    HIP_TRY(hipSetDevice(device));
    return handle_make(N, P, src->kmer_length, device, opts, with_hashtables, t0, [&](kmdb_db* db) {
        const int rc = kmdb_layout_from_device(db, src, with_hashtables);
        src->layout_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        return rc;
    }, out, &src->prepare_ms);
}

extern "C" void kmdb_db_settle(kmdb_db* db) {
    if (db && db->staging_thread.joinable()) db->staging_thread.join();
}

extern "C" void kmdb_db_free(kmdb_db* db) {
    if (!db) return;
    (void)hipSetDevice(db->device);
    db->one_shot = false;
    kmdb_release_staging(db);
    if (db->staging_thread.joinable()) db->staging_thread.join();
    for (const auto& r : db->staging_kept) (void)munmap(r.first, r.second);      // a one-shot handle's regions: pages long dropped, the mappings go now
    db->staging_kept.clear();
    // The streams go first; the pipeline's state, the device arrays and the events are members and go with the handle below, while its device
    // is still current (set above).  The order does not matter: a destroyed stream finishes its work, and hipFree waits for the device.
    if (db->stream2) (void)hipStreamDestroy(db->stream2);
    if (db->stream) (void)hipStreamDestroy(db->stream);
    delete db;
}

int kmdb_engine_get(kmdb_db* db, kmdb_engine_view* o) {
    if (hipSetDevice(db->device) != hipSuccess) return kmdb_set_error("hipSetDevice failed");
    if (kmdb_ensure_v1_arrays(db)) return 1;
    o->device = db->device; o->N = db->N; o->P = db->P; o->kmer_length = db->kmer_length;
    o->meta = db->meta; o->bitpos = db->bitpos; o->parent = db->parent; o->w = db->w; o->sub_end = db->sub_end;
    o->ck_ofs = db->ck_ofs; o->ck_bit = db->ck_bit; o->ck_id = db->ck_id;
    o->bits = db->bits; o->n_buckets = db->n_buckets; o->bucket_offset = db->bucket_offset; o->slots = db->slots;
    o->pid2dfs = db->pid2dfs; o->qs_index = db->qs_index; o->qs_count = db->qs_count; o->stream = db->stream;
    o->max_depth = db->max_depth; o->list_sets = &db->list_sets; o->list_sets_nb = &db->list_sets_nb; o->list_sets_tried = &db->list_sets_tried;
    o->rl_ofs = &db->rl_ofs; o->rl_runs = &db->rl_runs; o->rl_node = &db->rl_node; o->rl_tried = &db->rl_tried;
    o->device_bytes = &db->stats.device_bytes; o->d2_stats = &db->d2_stats; o->d2_sample_stats = &db->d2_sample_stats; o->n2s_stats = &db->n2s_stats; o->n2a_sample_stats = &db->n2a_sample_stats;
    for (int i = 0; i < 4; ++i) o->ev[i] = db->ev[i];
    return 0;
}

void kmdb_engine_set_times(kmdb_db* db, double kernel_ms, double dominant_ms) {
    kmdb_release_staging(db);                                   // (end of a new2all / db2db call)
    db->stats.kernel_ms = kernel_ms;
    (void)dominant_ms;
}

extern "C" const char* kmdb_db_fallback_reason(const kmdb_db* db) { return db ? db->fallback_reason.c_str() : ""; }

extern "C" int kmdb_db_stats(const kmdb_db* db, kmdb_stats* out) {
    if (!db || !out) return kmdb_set_error("kmdb_db_stats: null argument");
    *out = db->stats;
    return 0;
}

// ------------------------------------------------------------------------------------------
// dense all2all
// ------------------------------------------------------------------------------------------
// (engine_state.h) what run_dense and the band call of a2a_rows_records.hip do before and after kmdb_blocks_run
int kmdb_blocks_ensure_prepared(kmdb_db* db) {
    if (db->blocks_prepared) return 0;
    if (kmdb_blocks_prepare(db)) return 1;
    db->blocks_bytes_counted = kmdb_blocks_device_bytes(db);
    db->stats.device_bytes += db->blocks_bytes_counted;
    db->stats.width = db->width;
    return 0;
}
int kmdb_blocks_stage_ms(kmdb_db* db, float ms[4]) {
    HIP_TRY(hipEventElapsedTime(&ms[0], db->ev[1], db->ev_k[0]));
    for (int i = 1; i < 4; ++i) HIP_TRY(hipEventElapsedTime(&ms[i], db->ev_k[i - 1], db->ev_k[i]));
    return 0;
}

namespace {

// the whole dense pipeline on `st`; M is device memory of N(N-1)/2 uint32
int run_dense(kmdb_db* db, uint32_t* M, const kmdb_opts* opts, hipStream_t st) {
    const uint64_t N = db->N, P = db->P;
    const uint64_t cells = N ? N * (N - 1) / 2 : 0;
    const uint32_t shard_index = opts ? opts->shard_index : 0, shard_count = opts && opts->shard_count ? opts->shard_count : 1;
    if (shard_index >= shard_count) return kmdb_set_error("kmdb_all2all: shard_index >= shard_count");
    const uint32_t flags = opts ? opts->flags : 0;
    if (flags & ~KMDB_FLAG_ALL) return kmdb_set_error("kmdb_all2all: unknown bits in kmdb_opts.flags");
    // slice of the DFS-ordered pattern stream whose pairs this call adds
    const uint32_t lo = (uint32_t)(P * shard_index / shard_count), hi = (uint32_t)(P * (shard_index + 1) / shard_count);

    HIP_TRY(hipEventRecord(db->ev[0], st));
    if (cells) HIP_TRY(hipMemsetAsync(M, 0, cells * 4, st));
    db->stats.path = KMDB_PATH_NONE;
    db->stats.k0_ms = db->stats.k1_ms = db->stats.k1n_ms = db->stats.k1g_ms = db->stats.k2_ms = 0;
    db->stats.n_records = 0; db->stats.n_direct = 0; db->stats.n_wide = 0; db->stats.n_chunks = 0; db->stats.tile_flushes = 0; db->stats.sized_call = 0;
    if (!cells || !P) { HIP_TRY(hipEventRecord(db->ev[1], st)); HIP_TRY(hipEventRecord(db->ev[2], st)); return 0; }
    const bool forced_v1 = (flags & (KMDB_FLAG_FORCE_GLOBAL_ATOMICS | KMDB_FLAG_FORCE_DIRECT | KMDB_FLAG_FORCE_TILE)) != 0;
    if (!forced_v1 && kmdb_blocks_ensure_prepared(db)) return 1;
    if (!forced_v1 && db->fallback_reason.empty()) {
        // block-record pipeline (flat form: on-disk weights, no subtree sums needed)
        HIP_TRY(hipEventRecord(db->ev[1], st));
        if (kmdb_blocks_run(db, M, lo, hi, st)) return 1;
        const bool sized = db->last_call_sized;
        if (db->fallback_reason.empty()) {
            HIP_TRY(hipEventRecord(db->ev[2], st));
            db->stats.path = KMDB_PATH_RECORDS;
            db->stats.sized_call = sized ? 1u : 0u;
            return 0;
        }
        if (cells) HIP_TRY(hipMemsetAsync(M, 0, cells * 4, st));          // a partial result of the abandoned attempt
    }
    if (!forced_v1) {
        // Not the fast path: say so, once per handle and reason.
        static thread_local const kmdb_db* noted = nullptr;
        if (noted != db) {
            noted = db;
            fprintf(stderr, "[kmdb] note: the block-record pipeline cannot take this database (%s); running the HBM-atomics kernel, "
                            "expect it to be far slower\n", db->fallback_reason.c_str());
        }
        if (flags & KMDB_FLAG_NO_FALLBACK) return kmdb_set_error("kmdb_all2all: block-record pipeline unavailable: " + db->fallback_reason);
        // a slice of the pattern stream means something else to the two paths (pattern ranges here, 2048-node segments there): partial
        // matrices of slices that took different paths would not add up to the whole
        if (shard_count > 1) return kmdb_set_error("kmdb_all2all: slices of the pattern stream (kmdb_opts.shard_count > 1) need the block-record pipeline: " + db->fallback_reason);
    }
    // v1 kernels: tree form, subtree weights (reference similarity_calculator.cpp:64-72) = exclusive scan of w in DFS order
    // (beyond 4096 samples every v1 call runs a2a_global_kernel, whose stack and decoder hold 32-bit ids: no sample limit of its own — round 5
    // refused 65 536 samples and more here, so a tree deeper than the chain table on such a collection had no path at all; the LDS kernels
    // with their 16-bit ids are only ever chosen up to 4096 samples, kmdb_v1_run)
    if (kmdb_ensure_v1_arrays(db)) return 1;
    HIP_TRY(hipMemsetAsync(db->v1_counters, 0, 8 * sizeof(unsigned long long), st));
    HIP_TRY(prim::exclusive_sum(db->v1_scan_tmp, db->v1_scan_tmp_bytes, db->w.get(), db->wprefix.get(), (int)(P + 1), st));
    HIP_TRY(hipEventRecord(db->ev[1], st));
    const uint32_t seg_begin = (uint32_t)((uint64_t)db->n_segs * shard_index / shard_count) / WAVES_PER_BLOCK * WAVES_PER_BLOCK;
    const uint32_t seg_end = shard_index + 1 == shard_count ? db->n_segs : (uint32_t)((uint64_t)db->n_segs * (shard_index + 1) / shard_count) / WAVES_PER_BLOCK * WAVES_PER_BLOCK;
    if (kmdb_v1_run(db, M, seg_begin, seg_end, forced_v1 ? flags : KMDB_FLAG_FORCE_GLOBAL_ATOMICS, st)) return 1;
    HIP_TRY(hipEventRecord(db->ev[2], st));
    const bool global = !forced_v1 || (flags & KMDB_FLAG_FORCE_GLOBAL_ATOMICS) || N > 4096;
    db->stats.path = global ? KMDB_PATH_GLOBAL : KMDB_PATH_TILE;
    return 0;
}

int finish_stats(kmdb_db* db, hipStream_t st) {
    HIP_TRY(hipEventRecord(db->ev[3], st));
    HIP_TRY(hipEventSynchronize(db->ev[3]));
    float a = 0;
    HIP_TRY(hipEventElapsedTime(&a, db->ev[0], db->ev[3]));
    db->stats.kernel_ms = a;
    if (db->stats.path == KMDB_PATH_RECORDS) {
        float k[4];
        if (kmdb_blocks_stage_ms(db, k)) return 1;
        db->stats.k0_ms = k[0]; db->stats.k1n_ms = k[1]; db->stats.k1g_ms = k[2]; db->stats.k1_ms = k[1] + k[2]; db->stats.k2_ms = k[3];
        const kmdb_blocks_counts last = kmdb_blocks_last_counts(db);
        db->stats.n_records = last.records; db->stats.n_wide = last.wide; db->stats.n_chunks = last.chunks;
        db->stats.n_joined = last.joined;
        db->stats.n_direct = last.direct;
        // the pipeline's arrays grow inside calls (second-level arrays on the first call, pools enlarged by a quarter or doubled): what is
        // resident NOW, not what the preparation allocated
        kmdb_recount_bytes(db, db->blocks_bytes_counted, kmdb_blocks_device_bytes(db));
    } else if (db->v1_counters && db->stats.path != KMDB_PATH_NONE) {
        unsigned long long c[8];
        HIP_TRY(hipMemcpy(c, db->v1_counters, sizeof c, hipMemcpyDeviceToHost));
        db->stats.tile_flushes = c[0];
    }
    return 0;
}

}  // namespace

extern "C" int kmdb_all2all_dense_device(kmdb_db* db, void* out_dev, const kmdb_opts* opts) {
    if (!db || !out_dev) return kmdb_set_error("kmdb_all2all_dense_device: null argument");
    HIP_TRY(hipSetDevice(db->device));
    hipStream_t st = (opts && opts->stream) ? (hipStream_t)opts->stream : db->stream;
    if (run_dense(db, (uint32_t*)out_dev, opts, st)) return 1;
    const int rc = finish_stats(db, st);
    kmdb_release_staging(db);                                   // the upload's host buffers, once the first call is through
    return rc;
}

extern "C" int kmdb_all2all_dense(kmdb_db* db, uint32_t* out, const kmdb_opts* opts) {
    if (!db || (!out && db->N > 1)) return kmdb_set_error("kmdb_all2all_dense: null argument");
    HIP_TRY(hipSetDevice(db->device));
    const uint64_t cells = db->N ? db->N * (db->N - 1) / 2 : 0;
    DevBuf<uint32_t> M;
    DEV_ALLOC(M, std::max<uint64_t>(cells, 1));
    hipStream_t st = (opts && opts->stream) ? (hipStream_t)opts->stream : db->stream;
    int rc = run_dense(db, M, opts, st);
    if (!rc) rc = finish_stats(db, st);
    if (!rc && cells && hipMemcpy(out, M, cells * 4, hipMemcpyDeviceToHost) != hipSuccess)
        rc = kmdb_set_error("kmdb_all2all_dense: copy back failed");
    M.reset();
    kmdb_release_staging(db);
    return rc;
}

// ------------------------------------------------------------------------------------------
// sparse all2all: same accumulation in HBM (tree form and flat form give the same cells,
// SURVEY §7), then on-device compaction of the non-zeros into CSR.  Bubbles
// (reference src/bubble_helper.h) only exist to spare the CPU hash maps; their contributions are part
// of the same sums, so bubble_size does not change the result.
// ------------------------------------------------------------------------------------------
namespace {
// one host bound -> the device's widened bound on a plain ratio.  mash = -(1/k) log(2 j / (1 + j)) falls with j:
// mash <= m  <=>  j >= E / (2 - E), E = exp(-k m); ani = 1 - mash.
struct RatioBound { int kind; double lo, hi; };
RatioBound ratio_bound(const kmdb_cell_filter& f, int k) {
    const double inf = std::numeric_limits<double>::infinity();
    auto j_of_mash = [k](double m) {                       // the j whose mash distance is m (0 .. inf)
        const double E = std::exp(-(double)k * m);
        if (std::isnan(E)) return std::numeric_limits<double>::quiet_NaN();
        if (E >= 2.0) return std::numeric_limits<double>::infinity();
        return E / (2.0 - E);
    };
    RatioBound r{RATIO_NUM, f.lo, f.hi};
    double mlo = f.lo, mhi = f.hi;                          // bounds on the mash distance, for the log-based measures
    bool logm = false;
    switch (f.metric) {
    case KMDB_METRIC_JACCARD: r.kind = RATIO_JACCARD; break;
    case KMDB_METRIC_MIN: r.kind = RATIO_MIN; break;
    case KMDB_METRIC_MAX: r.kind = RATIO_MAX; break;
    case KMDB_METRIC_COSINE: r.kind = RATIO_COSINE; break;
    case KMDB_METRIC_NUM_KMERS: r.kind = RATIO_NUM; break;
    case KMDB_METRIC_MASH: r.kind = RATIO_JACCARD; logm = true; break;
    case KMDB_METRIC_MASH_QUERY: r.kind = RATIO_QUERY; logm = true; break;
    case KMDB_METRIC_ANI: r.kind = RATIO_JACCARD; logm = true; mlo = 1.0 - f.hi; mhi = 1.0 - f.lo; break;
    case KMDB_METRIC_ANI_SHORTER: r.kind = RATIO_MIN; logm = true; mlo = 1.0 - f.hi; mhi = 1.0 - f.lo; break;
    default: break;
    }
    if (logm) { r.lo = j_of_mash(mhi); r.hi = j_of_mash(mlo); }
    // the margin: 1e-6 relative and a little absolute — far above any rounding difference between the two sides, far below
    // anything that costs transfer volume; a NaN bound keeps everything (the host decides)
    if (std::isnan(r.lo)) r.lo = -inf; else r.lo = r.lo - std::fabs(r.lo) * 1e-6 - 1e-300;
    if (std::isnan(r.hi)) r.hi = inf; else r.hi = r.hi + std::fabs(r.hi) * 1e-6 + 1e-300;
    return r;
}
}  // namespace

void kmdb_dev_bounds(const kmdb_cell_filter* filters, size_t n_filters, int kmer_length, int* kind, double* lo, double* hi) {
    for (size_t i = 0; i < n_filters; ++i) {
        const RatioBound rb = ratio_bound(filters[i], kmer_length);
        kind[i] = rb.kind; lo[i] = rb.lo; hi[i] = rb.hi;
    }
}

static int sparse_impl(kmdb_db* db, bool from_cells, const void* dense_dev, uint64_t cell_lo, uint64_t cell_hi, const kmdb_cell_filter* filters, size_t n_filters,
                       const uint32_t* sample_kmers, int measure, kmdb_sparse_rows* out, const kmdb_opts* opts, kmdb_csr_dev* keep = nullptr);

int kmdb_check_filters(const char* who, const kmdb_cell_filter* filters, size_t n_filters, const uint32_t* sample_kmers, int measure) {
    if ((n_filters && !filters) || ((n_filters || measure >= 0) && !sample_kmers)) return kmdb_set_error(std::string(who) + ": null argument");
    if (measure >= KMDB_METRIC_COUNT) return kmdb_set_error(std::string(who) + ": unknown measure");
    if (n_filters > (size_t)DEV_FILTER_MAX) return kmdb_set_error(std::string(who) + ": more than " + std::to_string(DEV_FILTER_MAX) + " bounds");
    for (size_t i = 0; i < n_filters; ++i)
        if (filters[i].metric < 0 || filters[i].metric >= KMDB_METRIC_COUNT) return kmdb_set_error(std::string(who) + ": unknown metric in a filter");
    return 0;
}

extern "C" int kmdb_all2all_sparse(kmdb_db* db, kmdb_sparse_rows* out, const kmdb_opts* opts) {
    return sparse_impl(db, false, nullptr, 0, ~0ull, nullptr, 0, nullptr, -1, out, opts);
}

int kmdb_all2all_csr_device(const char* who, kmdb_db* db, kmdb_csr_dev* keep, const kmdb_opts* opts) {
    if (!db || !keep) return kmdb_set_error(std::string(who) + ": null argument");
    kmdb_sparse_rows none{};
    return sparse_impl(db, false, nullptr, 0, ~0ull, nullptr, 0, nullptr, -1, &none, opts, keep);
}

extern "C" int kmdb_all2all_sparse_filtered(kmdb_db* db, const kmdb_cell_filter* filters, size_t n_filters, const uint32_t* sample_kmers, int measure,
                                            kmdb_sparse_rows* out, const kmdb_opts* opts) {
    if (kmdb_check_filters("kmdb_all2all_sparse_filtered", filters, n_filters, sample_kmers, measure)) return 1;
    // bounds are conditions on the whole cell: a slice of the pattern stream (opts->shard_*) holds partial sums only
    if ((n_filters || measure >= 0) && opts && opts->shard_count > 1) return kmdb_set_error("kmdb_all2all_sparse_filtered: filters need the whole database (shard_count must be 1)");
    return sparse_impl(db, false, nullptr, 0, ~0ull, filters, n_filters, sample_kmers, measure, out, opts);
}

extern "C" int kmdb_sparse_from_dense_device(kmdb_db* db, const void* cells_dev, uint64_t cell_lo, uint64_t cell_hi, const kmdb_cell_filter* filters,
                                             size_t n_filters, const uint32_t* sample_kmers, int measure, kmdb_sparse_rows* out, const kmdb_opts* opts) {
    if (!db || !out) return kmdb_set_error("kmdb_sparse_from_dense_device: null argument");
    if (kmdb_check_filters("kmdb_sparse_from_dense_device", filters, n_filters, sample_kmers, measure)) return 1;
    const uint64_t cells = db->N ? db->N * (db->N - 1) / 2 : 0;
    if (cell_hi > cells) cell_hi = cells;
    if (cell_lo > cell_hi) return kmdb_set_error("kmdb_sparse_from_dense_device: cell_lo > cell_hi");
    if (!cells_dev && cell_hi > cell_lo) return kmdb_set_error("kmdb_sparse_from_dense_device: null matrix");
    return sparse_impl(db, true, cells_dev, cell_lo, cell_hi, filters, n_filters, sample_kmers, measure, out, opts);
}

// The host side of a filtered sparse call: every cell that left the device is decided by the reference's own arithmetic (a = the row sample's k-mer
// count, b = the column sample's: CombinedFilter, sparse_filters.h:38-61), the rows are compacted in place and the measures computed.  The all2all
// calls pass one count array twice, db2db.hip the arrays of its two databases.
int kmdb_sparse_decide(const char* who, kmdb_sparse_rows* out, const kmdb_cell_filter* filters, size_t n_filters, const uint32_t* row_kmers,
                       const uint32_t* col_kmers, int measure, int k) {
    const uint64_t N = out->n_rows;
    const unsigned nthr = std::max(1u, std::min(32u, std::thread::hardware_concurrency()));
    std::vector<uint64_t> kept(N + 1, 0);
    auto rows_of = [&](unsigned t, auto&& fn) { for (uint64_t i = (uint64_t)N * t / nthr; i < (uint64_t)N * (t + 1) / nthr; ++i) fn(i); };
    auto parallel = [&](auto&& fn) {
        std::vector<std::thread> th;
        for (unsigned t = 0; t < nthr; ++t) th.emplace_back([&, t]() { rows_of(t, fn); });
        for (auto& x : th) x.join();
    };
    parallel([&](uint64_t i) {                             // pass 1: filter every row in place (write position <= read position)
        uint64_t w = out->row_ptr[i];
        for (uint64_t e = out->row_ptr[i]; e < out->row_ptr[i + 1]; ++e) {
            const uint32_t c = out->val[e], cj = out->col[e];
            bool ok = true;
            for (size_t q = 0; q < n_filters && ok; ++q) {
                const double x = kmdbh_metric(filters[q].metric, c, row_kmers[i], col_kmers[cj], k);
                ok = x >= filters[q].lo && x <= filters[q].hi;
            }
            if (ok) { out->col[w] = cj; out->val[w] = c; ++w; }
        }
        kept[i + 1] = w - out->row_ptr[i];
    });
    std::vector<uint64_t> new_ptr(N + 1, 0);
    for (uint64_t i = 0; i < N; ++i) new_ptr[i + 1] = new_ptr[i] + kept[i + 1];
    // pass 2: close the gaps (ascending rows; a row never moves right)
    for (uint64_t i = 0; i < N; ++i)
        if (new_ptr[i] != out->row_ptr[i] && kept[i + 1]) {
            std::memmove(out->col + new_ptr[i], out->col + out->row_ptr[i], kept[i + 1] * 4);
            std::memmove(out->val + new_ptr[i], out->val + out->row_ptr[i], kept[i + 1] * 4);
        }
    for (uint64_t i = 0; i <= N; ++i) out->row_ptr[i] = new_ptr[i];
    out->nnz = new_ptr[N];
    if (measure >= 0) {
        out->measure = (double*)std::malloc(std::max<uint64_t>(out->nnz, 1) * 8);
        if (!out->measure) { kmdb_sparse_free(out); return kmdb_set_error(std::string(who) + ": out of host memory for the measures"); }
        parallel([&](uint64_t i) {
            for (uint64_t e = out->row_ptr[i]; e < out->row_ptr[i + 1]; ++e)
                out->measure[e] = kmdbh_metric(measure, out->val[e], row_kmers[i], col_kmers[out->col[e]], k);
        });
    }
    return 0;
}

// from_cells: compact the caller's cells [cell_lo, cell_hi) (dense_dev points at cell_lo); else accumulate the whole triangle first
static int sparse_impl(kmdb_db* db, bool from_cells, const void* dense_dev, uint64_t cell_lo, uint64_t cell_hi, const kmdb_cell_filter* filters, size_t n_filters,
                       const uint32_t* sample_kmers, int measure, kmdb_sparse_rows* out, const kmdb_opts* opts, kmdb_csr_dev* keep) {
    if (!db || !out) return kmdb_set_error("kmdb_all2all_sparse: null argument");
    std::memset(out, 0, sizeof *out);
    HIP_TRY(hipSetDevice(db->device));
    const uint64_t N = db->N;
    const uint64_t cells = N ? N * (N - 1) / 2 : 0;
    DevBuf<uint32_t> M, col, val, d_counts;
    DevBuf<unsigned long long> row_nnz, row_ptr;
    DevBuf<void> tmp;
    hipStream_t st = (opts && opts->stream) ? (hipStream_t)opts->stream : db->stream;
    int rc = 0;
    DevFilter df{};
#define SP_TRY(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) { kmdb_sparse_free(out); return kmdb_set_error(std::string(#expr) + ": " + hipGetErrorString(e_)); } } while (0)
#define SP_ALLOC(buf, n) do { if ((buf).alloc((n), #buf)) { kmdb_sparse_free(out); return 1; } } while (0)
    if (!from_cells) SP_ALLOC(M, std::max<uint64_t>(cells, 1));
    SP_ALLOC(row_nnz, N + 1);
    SP_ALLOC(row_ptr, N + 1);
    if (n_filters) {
        SP_ALLOC(d_counts, std::max<uint64_t>(N, 1));
        SP_TRY(hipMemcpyAsync(d_counts, sample_kmers, N * 4, hipMemcpyHostToDevice, st));
        df.n = (int)n_filters; df.counts = d_counts;
        kmdb_dev_bounds(filters, n_filters, (int)db->kmer_length, df.kind, df.lo, df.hi);
    }
    const uint32_t* cellsp = (const uint32_t*)dense_dev;
    if (!from_cells) {
        rc = run_dense(db, M, opts, st);
        if (rc) return rc;
        cellsp = M; cell_lo = 0; cell_hi = cells;
    } else {
        SP_TRY(hipEventRecord(db->ev[0], st)); SP_TRY(hipEventRecord(db->ev[1], st)); SP_TRY(hipEventRecord(db->ev[2], st));
        db->stats.path = KMDB_PATH_NONE;
    }
    // rows that meet the range: row r holds the cells [r (r - 1) / 2, r (r + 1) / 2)
    uint64_t row_lo = 0, row_hi = 0;
    if (cell_hi > cell_lo) {
        auto row_of = [](uint64_t c) { uint64_t r = (uint64_t)((1.0 + std::sqrt(1.0 + 8.0 * (double)c)) / 2.0); while (r * (r - 1) / 2 > c) --r; while ((r + 1) * r / 2 <= c) ++r; return r; };
        row_lo = row_of(cell_lo); row_hi = row_of(cell_hi - 1) + 1;
    }
    SP_TRY(hipMemsetAsync(row_nnz, 0, (N + 1) * 8, st));
    // the block-record pipeline just told which tiles it added to: only those are scanned (KMDB_SP_ALL_TILES=1: every cell, as before — A/B)
    const unsigned char* touched = kmdb_blocks_tile_touched(db);
    const bool skip = !from_cells && db->stats.path == KMDB_PATH_RECORDS && touched && N > 1 && !getenv("KMDB_SP_ALL_TILES");
    const TileSkip ts{touched, db->width};
    if (skip) hipLaunchKernelGGL((row_tiles_kernel<false>), dim3((unsigned)N), dim3(64), 0, st, cellsp, N, ts, row_nnz, (const unsigned long long*)nullptr, (uint32_t*)nullptr,
                                 (uint32_t*)nullptr, df);
    else
    if (row_hi > row_lo) hipLaunchKernelGGL(row_nnz_kernel, dim3((unsigned)(row_hi - row_lo)), dim3(256), 0, st, cellsp, row_lo, cell_lo, cell_hi, row_nnz, df);
    size_t tmp_bytes = 0;
    SP_TRY(prim::exclusive_sum(nullptr, tmp_bytes, row_nnz.get(), row_ptr.get(), (int)(N + 1), st));
    SP_ALLOC(tmp, std::max<size_t>(tmp_bytes, 16));
    SP_TRY(prim::exclusive_sum(tmp, tmp_bytes, row_nnz.get(), row_ptr.get(), (int)(N + 1), st));
    std::vector<unsigned long long> h_ptr(N + 1, 0);
    SP_TRY(hipMemcpyAsync(h_ptr.data(), row_ptr, (N + 1) * 8, hipMemcpyDeviceToHost, st));
    SP_TRY(hipStreamSynchronize(st));
    const uint64_t nnz = h_ptr[N];
    SP_ALLOC(col, std::max<uint64_t>(nnz, 1));
    SP_ALLOC(val, std::max<uint64_t>(nnz, 1));
    if (skip) hipLaunchKernelGGL((row_tiles_kernel<true>), dim3((unsigned)N), dim3(64), 0, st, cellsp, N, ts, (unsigned long long*)nullptr, row_ptr, col, val, df);
    else
    if (row_hi > row_lo) hipLaunchKernelGGL(row_compact_kernel, dim3((unsigned)(row_hi - row_lo)), dim3(256), 0, st, cellsp, row_lo, cell_lo, cell_hi, row_ptr, col, val, df);
    rc = finish_stats(db, st);
    if (rc) return rc;
    if (keep) {                                                   // the CSR stays in HBM (kmdb_all2all_csr_device)
        keep->row_ptr.take(row_ptr); keep->col.take(col); keep->val.take(val);
        keep->n_rows = N; keep->nnz = nnz;
        kmdb_release_staging(db);
        return 0;
    }
    out->n_rows = N;
    out->nnz = nnz;
    out->row_ptr = (uint64_t*)std::malloc((N + 1) * 8);
    out->col = (uint32_t*)std::malloc(std::max<uint64_t>(nnz, 1) * 4);
    out->val = (uint32_t*)std::malloc(std::max<uint64_t>(nnz, 1) * 4);
    if (!out->row_ptr || !out->col || !out->val) { kmdb_sparse_free(out); return kmdb_set_error("kmdb_all2all_sparse: out of host memory for the result"); }
    for (uint64_t i = 0; i <= N; ++i) out->row_ptr[i] = h_ptr[i];
    if (nnz) {
        SP_TRY(hipMemcpy(out->col, col, nnz * 4, hipMemcpyDeviceToHost));
        SP_TRY(hipMemcpy(out->val, val, nnz * 4, hipMemcpyDeviceToHost));
    }
#undef SP_TRY
#undef SP_ALLOC
    kmdb_release_staging(db);
    if (n_filters || measure >= 0) return kmdb_sparse_decide("kmdb_all2all_sparse", out, filters, n_filters, sample_kmers, sample_kmers, measure, (int)db->kmer_length);
    return 0;
}

// ------------------------------------------------------------------------------------------
// -sample-rows <criterion>:<count> with the selection on the device (sample_rows.hip) and the decision on the host (host_sampler.cpp).
// Replaces all2all_sp + SparseMatrix::add_to_sampler + Sampler::saveRowSparse (console_all2all_sparse.cpp:70-89, array.h:450-540, sampler.h)
// without the full sparse matrix ever leaving HBM.
// ------------------------------------------------------------------------------------------
namespace {
struct Proxy { int kind, flip; };
// the plain ratio a criterion is monotone in (ratio_bound's mapping) and whether the criterion falls with it
Proxy proxy_of(int criterion) {
    switch (criterion) {
    case KMDB_METRIC_JACCARD: return {RATIO_JACCARD, 0};
    case KMDB_METRIC_MIN: return {RATIO_MIN, 0};
    case KMDB_METRIC_MAX: return {RATIO_MAX, 0};
    case KMDB_METRIC_COSINE: return {RATIO_COSINE, 0};
    case KMDB_METRIC_MASH: return {RATIO_JACCARD, 1};
    case KMDB_METRIC_ANI: return {RATIO_JACCARD, 0};
    case KMDB_METRIC_ANI_SHORTER: return {RATIO_MIN, 0};
    case KMDB_METRIC_MASH_QUERY: return {RATIO_QUERY, 1};
    default: return {RATIO_NUM, 0};
    }
}
double host_proxy(Proxy p, uint32_t c, uint32_t a, uint32_t b) {
    double x;
    switch (p.kind) {
    case RATIO_JACCARD: x = (double)c / (double)(uint32_t)(a + b - c); break;
    case RATIO_MIN:     x = (double)c / (double)std::min(a, b); break;
    case RATIO_MAX:     x = (double)c / (double)std::max(a, b); break;
    case RATIO_COSINE:  x = (double)c / std::sqrt((double)(uint32_t)(a * b)); break;
    case RATIO_QUERY:   x = (double)c / (double)a; break;
    default:            x = (double)c; break;
    }
    return p.flip ? -x : x;
}
int check_sample_args(const char* who, const kmdb_cell_filter* filters, size_t n_filters, const uint32_t* sample_kmers, int criterion, uint32_t count) {
    if (count == 0) return kmdb_set_error(std::string(who) + ": count must be at least 1");
    if (criterion < 0 || criterion >= KMDB_METRIC_COUNT) return kmdb_set_error(std::string(who) + ": unknown criterion");
    if (!sample_kmers) return kmdb_set_error(std::string(who) + ": sample_kmers is NULL");
    return kmdb_check_filters(who, filters, n_filters, sample_kmers, -1);
}

// The selection and its completeness rule over the lines of a job's slots (the symmetric rows of a triangle; the row and column lines of a
// rectangle): sel.res holds every line, sel.whole the lines of sel.again (ascending slots) fetched again whole.  ab(s, o, a, b): the k-mer counts
// of the ROW sample (a) and the COLUMN sample (b) of the cell that line s lists under the id o.
struct SampleSelection { kmdb_sample_result res, whole; std::vector<uint32_t> again; };
template <class AB>
int select_complete(hipStream_t st, const kmdb_sample_job& job, uint64_t n_slots, Proxy px, uint32_t count, int k, const kmdb_cell_filter* filters, size_t n_filters,
                    AB&& ab, kmdb_sample_stats& ss, SampleSelection& sel) {
    kmdb_sample_result& res = sel.res;
    if (kmdb_sample_candidates(st, job, nullptr, 0, &res)) return 1;
    ss.rows_truncated = res.rows_truncated; ss.d2h_bytes = res.d2h_bytes; ss.select_ms = res.select_ms; ss.triangle_reads = res.passes;
    // Completeness.  A row that came out whole is decided.  A truncated row holds every cell whose key is >= the key of T_s, its count-th best
    // proxy, less the margin: when `count` of its candidates at or above T_s pass the EXACT filters, no cell the device held back can be among
    // the row's best.  T_s is recomputed here from the candidates (they include all cells at or above it).  A row of fewer than `count`
    // candidates was not truncated; without filters every candidate passes.
    std::vector<uint32_t>& again = sel.again;
    if (n_filters) {
        std::vector<uint32_t> keys;
        for (uint64_t s = 0; s < n_slots; ++s) {
            const uint64_t b = res.row_ptr[s], e = res.row_ptr[s + 1];
            if (e - b < count) continue;
            keys.clear();
            for (uint64_t x = b; x < e; ++x) {
                uint32_t ca, cb;
                ab(s, res.col[x], ca, cb);
                keys.push_back(kmdb_sample_proxy_key(host_proxy(px, res.val[x], ca, cb)));
            }
            std::vector<uint32_t> sorted(keys);
            std::nth_element(sorted.begin(), sorted.begin() + (count - 1), sorted.end(), std::greater<uint32_t>());
            const uint32_t T = sorted[count - 1];
            uint64_t ok = 0;
            for (uint64_t x = b; x < e && ok < count; ++x) {
                if (keys[x - b] < T) continue;
                uint32_t ca, cb;
                ab(s, res.col[x], ca, cb);
                bool pass = true;
                for (size_t q = 0; q < n_filters && pass; ++q) {
                    const double v = kmdbh_metric(filters[q].metric, res.val[x], ca, cb, k);
                    pass = v >= filters[q].lo && v <= filters[q].hi;
                }
                ok += pass ? 1 : 0;
            }
            if (ok < count) again.push_back((uint32_t)s);
        }
    }
    if (!again.empty()) {
        if (kmdb_sample_candidates(st, job, again.data(), again.size(), &sel.whole)) return 1;
        ss.rows_refetched = again.size(); ss.d2h_bytes += sel.whole.d2h_bytes; ss.select_ms += sel.whole.select_ms; ss.triangle_reads += sel.whole.passes;
    }
    return 0;
}
// the lines of the slots [s_lo, s_hi) as the rows of `out`, a re-fetched line in place of its first form
int pack_slots(const char* who, const SampleSelection& sel, uint64_t s_lo, uint64_t s_hi, kmdb_sparse_rows* out) {
    const std::vector<uint32_t>& again = sel.again;
    const size_t a_lo = (size_t)(std::lower_bound(again.begin(), again.end(), s_lo) - again.begin());
    const uint64_t n = s_hi - s_lo;
    uint64_t nnz = 0;
    {
        size_t a = a_lo;
        for (uint64_t s = s_lo; s < s_hi; ++s) {
            const bool re = a < again.size() && again[a] == s;
            if (re) ++a;
            const kmdb_sample_result& r = re ? sel.whole : sel.res;
            nnz += r.row_ptr[s + 1] - r.row_ptr[s];
        }
    }
    out->n_rows = n; out->nnz = nnz;
    out->row_ptr = (uint64_t*)std::malloc((n + 1) * 8);
    out->col = (uint32_t*)std::malloc(std::max<uint64_t>(nnz, 1) * 4);
    out->val = (uint32_t*)std::malloc(std::max<uint64_t>(nnz, 1) * 4);
    if (!out->row_ptr || !out->col || !out->val) { kmdb_sparse_free(out); return kmdb_set_error(std::string(who) + ": out of host memory for the result"); }
    uint64_t w = 0;
    size_t a = a_lo;
    for (uint64_t s = s_lo; s < s_hi; ++s) {
        out->row_ptr[s - s_lo] = w;
        const bool re = a < again.size() && again[a] == s;
        if (re) ++a;
        const kmdb_sample_result& r = re ? sel.whole : sel.res;
        const uint64_t b = r.row_ptr[s], m = r.row_ptr[s + 1] - b;
        if (m) { std::memcpy(out->col + w, r.col.data() + b, m * 4); std::memcpy(out->val + w, r.val.data() + b, m * 4); }
        w += m;
    }
    out->row_ptr[n] = w;
    return 0;
}
void job_bounds(kmdb_sample_job& job, const kmdb_cell_filter* filters, size_t n_filters, int k) {
    job.n_bounds = n_filters;
    for (size_t i = 0; i < n_filters; ++i) {
        const RatioBound rb = ratio_bound(filters[i], k);
        job.bound_kind[i] = rb.kind; job.bound_lo[i] = rb.lo; job.bound_hi[i] = rb.hi;
    }
}

// The candidates of the symmetric rows of the cells [cell_lo, cell_hi) — complete: every row holds its `count` best cells by the exact decision
// among the cells of the range (rows the margin band could not settle are fetched again whole).
int sampled_impl(const char* who, kmdb_db* db, bool from_cells, const void* dense_dev, uint64_t cell_lo, uint64_t cell_hi, const kmdb_cell_filter* filters,
                 size_t n_filters, const uint32_t* sample_kmers, int criterion, uint32_t count, kmdb_sparse_rows* out, const kmdb_opts* opts) {
    std::memset(out, 0, sizeof *out);
    HIP_TRY(hipSetDevice(db->device));
    const uint64_t N = db->N;
    const uint64_t cells = N ? N * (N - 1) / 2 : 0;
    hipStream_t st = (opts && opts->stream) ? (hipStream_t)opts->stream : db->stream;
    DevBuf<uint32_t> M, d_counts;
    if (!from_cells) DEV_ALLOC(M, std::max<uint64_t>(cells, 1));
    DEV_ALLOC(d_counts, std::max<uint64_t>(N, 1));
    HIP_TRY(hipMemcpyAsync(d_counts, sample_kmers, N * 4, hipMemcpyHostToDevice, st));
    const int k = (int)db->kmer_length;
    const Proxy px = proxy_of(criterion);
    kmdb_sample_job job;
    job.N = N; job.counts_dev = d_counts; job.kind = px.kind; job.flip = px.flip; job.count = count;
    job_bounds(job, filters, n_filters, k);
    if (!from_cells) {
        if (run_dense(db, M, opts, st)) return 1;
        job.cells = M; job.cell_lo = 0; job.cell_hi = cells;
        // the block-record pipeline just told which tiles it added to: only those are read (KMDB_SP_ALL_TILES=1: every tile — A/B)
        const unsigned char* touched = kmdb_blocks_tile_touched(db);
        if (db->stats.path == KMDB_PATH_RECORDS && touched && N > 1 && !getenv("KMDB_SP_ALL_TILES")) { job.touched = touched; job.width = db->width; }
    } else {
        HIP_TRY(hipEventRecord(db->ev[0], st)); HIP_TRY(hipEventRecord(db->ev[1], st)); HIP_TRY(hipEventRecord(db->ev[2], st));
        db->stats.path = KMDB_PATH_NONE;
        job.cells = (const uint32_t*)dense_dev; job.cell_lo = cell_lo; job.cell_hi = cell_hi;
    }
    kmdb_sample_stats& ss = db->sample_stats;
    ss = kmdb_sample_stats{};
    try {
        SampleSelection sel;
        // (the pair's one score has the triangle's row, the larger id, as the row sample)
        auto ab = [&](uint64_t s, uint32_t o, uint32_t& a, uint32_t& b) { a = sample_kmers[std::max<uint64_t>(s, o)]; b = sample_kmers[std::min<uint64_t>(s, o)]; };
        if (select_complete(st, job, N, px, count, k, filters, n_filters, ab, ss, sel)) return 1;
        if (finish_stats(db, st)) return 1;
        kmdb_release_staging(db);
        if (pack_slots(who, sel, 0, N, out)) return 1;
        ss.candidates = out->nnz;
        return 0;
    } catch (const std::exception& e) {
        kmdb_sparse_free(out);
        return kmdb_set_error(std::string(who) + ": " + e.what());
    }
}
}  // namespace

// The same on a row-major nr x nc rectangle of two sample sets in HBM (engine_internal.h): the lines of the nr row samples into out_row (columns
// local to the column set), those of the nc column samples into out_col (columns local to the row set).  a = the row sample's count, b = the
// column sample's, on either line.
int kmdb_sample_rect(const char* who, hipStream_t st, int kmer_length, const uint32_t* cells_dev, uint64_t nr, uint64_t nc, const unsigned char* touched,
                     const kmdb_cell_filter* filters, size_t n_filters, const uint32_t* row_kmers, const uint32_t* col_kmers, int criterion, uint32_t count,
                     kmdb_sparse_rows* out_row, kmdb_sparse_rows* out_col, kmdb_sample_stats* stats) {
    std::memset(out_row, 0, sizeof *out_row);
    std::memset(out_col, 0, sizeof *out_col);
    DevBuf<uint32_t> d_rk, d_ck;
    DEV_ALLOC(d_rk, std::max<uint64_t>(nr, 1));
    DEV_ALLOC(d_ck, std::max<uint64_t>(nc, 1));
    if (nr) HIP_TRY(hipMemcpyAsync(d_rk, row_kmers, nr * 4, hipMemcpyHostToDevice, st));
    if (nc) HIP_TRY(hipMemcpyAsync(d_ck, col_kmers, nc * 4, hipMemcpyHostToDevice, st));
    const Proxy px = proxy_of(criterion);
    kmdb_sample_job job;
    job.rect = true; job.cells = cells_dev; job.nr = nr; job.nc = nc; job.touched = touched;
    job.counts_dev = d_rk; job.col_counts_dev = d_ck; job.kind = px.kind; job.flip = px.flip; job.count = count;
    job_bounds(job, filters, n_filters, kmer_length);
    kmdb_sample_stats ss{};
    try {
        SampleSelection sel;
        auto ab = [&](uint64_t s, uint32_t o, uint32_t& a, uint32_t& b) {
            if (s < nr) { a = row_kmers[s]; b = col_kmers[o]; } else { a = row_kmers[o]; b = col_kmers[s - nr]; }
        };
        if (select_complete(st, job, nr + nc, px, count, kmer_length, filters, n_filters, ab, ss, sel)) return 1;
        if (pack_slots(who, sel, 0, nr, out_row)) return 1;
        if (pack_slots(who, sel, nr, nr + nc, out_col)) { kmdb_sparse_free(out_row); return 1; }
        ss.candidates = out_row->nnz + out_col->nnz;
        if (stats) *stats = ss;
        return 0;
    } catch (const std::exception& e) {
        kmdb_sparse_free(out_row); kmdb_sparse_free(out_col);
        return kmdb_set_error(std::string(who) + ": " + e.what());
    }
}

// the limits of the select's 31-bit sizes (slots + 1 and tiles of 64 x 64), before any device work
int kmdb_sample_rect_check(const char* who, uint64_t nr, uint64_t nc) {
    if (nr >= (1ull << 31) || nc >= (1ull << 31) || nr + nc + 1 >= (1ull << 31)) return kmdb_set_error(std::string(who) + ": more than 2^31 - 2 samples in the two sets");
    if (((nr + 63) / 64) * ((nc + 63) / 64) >= (1ull << 31)) return kmdb_set_error(std::string(who) + ": more than 2^31 tiles of 64 x 64 cells");
    return 0;
}

extern "C" int kmdb_sampled_from_rect_device(kmdb_db* db, const void* cells_dev, uint64_t nr, uint64_t nc, const kmdb_cell_filter* filters, size_t n_filters,
                                             const uint32_t* row_sample_kmers, const uint32_t* col_sample_kmers, int criterion, uint32_t count,
                                             kmdb_sparse_rows* out_row_candidates, kmdb_sparse_rows* out_col_candidates, const kmdb_opts* opts) {
    const char* who = "kmdb_sampled_from_rect_device";
    if (!db || !out_row_candidates || !out_col_candidates) return kmdb_set_error(std::string(who) + ": null argument");
    if (check_sample_args(who, filters, n_filters, row_sample_kmers && col_sample_kmers ? row_sample_kmers : nullptr, criterion, count)) return 1;
    if (kmdb_sample_rect_check(who, nr, nc)) return 1;
    if (!cells_dev && nr && nc) return kmdb_set_error(std::string(who) + ": null matrix");
    HIP_TRY(hipSetDevice(db->device));
    hipStream_t st = (opts && opts->stream) ? (hipStream_t)opts->stream : db->stream;
    HIP_TRY(hipEventRecord(db->ev[0], st)); HIP_TRY(hipEventRecord(db->ev[1], st)); HIP_TRY(hipEventRecord(db->ev[2], st));
    db->stats.path = KMDB_PATH_NONE;
    db->d2_sample_stats = kmdb_sample_stats{};
    if (kmdb_sample_rect(who, st, (int)db->kmer_length, (const uint32_t*)cells_dev, nr, nc, nullptr, filters, n_filters, row_sample_kmers, col_sample_kmers, criterion,
                         count, out_row_candidates, out_col_candidates, &db->d2_sample_stats)) return 1;
    if (finish_stats(db, st)) { kmdb_sparse_free(out_row_candidates); kmdb_sparse_free(out_col_candidates); return 1; }
    kmdb_release_staging(db);
    return 0;
}

// The same on the QUERY ROWS of new2all (engine_internal.h): the flat cells [cell_lo, cell_hi) of a row-major nq x n_cols rectangle in HBM.
// One-sided: the slots are the rows that meet the range, a = the query's count, b = the sample's.  out has all nq rows.
int kmdb_sample_query_rows_check(const char* who, uint64_t nq, uint64_t n_cols, uint64_t cell_lo, uint64_t cell_hi) {
    if (n_cols == 0 || n_cols >= (1ull << 32)) return kmdb_set_error(std::string(who) + ": n_cols must be between 1 and 2^32 - 1");
    if (nq >= (1ull << 31)) return kmdb_set_error(std::string(who) + ": too many queries in one batch");
    if (cell_lo > cell_hi) return kmdb_set_error(std::string(who) + ": cell_lo > cell_hi");
    if (cell_hi > nq * n_cols) return kmdb_set_error(std::string(who) + ": cell_hi beyond the nq x n_cols cells of the batch");
    return 0;
}
int kmdb_sample_query_rows(const char* who, hipStream_t st, int kmer_length, const uint32_t* cells_dev, uint64_t nq, uint64_t n_cols, uint64_t cell_lo, uint64_t cell_hi,
                           const uint32_t* query_kmers, const kmdb_cell_filter* filters, size_t n_filters, const uint32_t* sample_kmers, int criterion, uint32_t count,
                           kmdb_sparse_rows* out, kmdb_sample_stats* stats) {
    std::memset(out, 0, sizeof *out);
    const uint64_t q_lo = cell_hi > cell_lo ? cell_lo / n_cols : 0, n_slots = cell_hi > cell_lo ? (cell_hi - 1) / n_cols + 1 - q_lo : 0;
    DevBuf<uint32_t> d_qk, d_sk;
    DEV_ALLOC(d_qk, std::max<uint64_t>(n_slots, 1));
    DEV_ALLOC(d_sk, n_cols);
    if (n_slots) HIP_TRY(hipMemcpyAsync(d_qk, query_kmers + q_lo, n_slots * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d_sk, sample_kmers, n_cols * 4, hipMemcpyHostToDevice, st));
    const Proxy px = proxy_of(criterion);
    kmdb_sample_job job;
    job.query_rows = true; job.cells = cells_dev; job.nr = nq; job.nc = n_cols; job.cell_lo = cell_lo; job.cell_hi = cell_hi;
    job.counts_dev = d_qk; job.col_counts_dev = d_sk; job.kind = px.kind; job.flip = px.flip; job.count = count;
    job_bounds(job, filters, n_filters, kmer_length);
    kmdb_sample_stats ss{};
    try {
        SampleSelection sel;
        auto ab = [&](uint64_t s, uint32_t o, uint32_t& a, uint32_t& b) { a = query_kmers[q_lo + s]; b = sample_kmers[o]; };
        if (select_complete(st, job, n_slots, px, count, kmer_length, filters, n_filters, ab, ss, sel)) return 1;
        kmdb_sparse_rows part{};
        if (pack_slots(who, sel, 0, n_slots, &part)) return 1;
        // the rows outside the range are empty
        uint64_t* ptr = (uint64_t*)std::malloc((nq + 1) * 8);
        if (!ptr) { kmdb_sparse_free(&part); return kmdb_set_error(std::string(who) + ": out of host memory for the result"); }
        for (uint64_t q = 0; q <= nq; ++q) ptr[q] = q < q_lo ? 0 : q - q_lo <= n_slots ? part.row_ptr[q - q_lo] : part.nnz;
        std::free(part.row_ptr);
        part.row_ptr = ptr; part.n_rows = nq;
        *out = part;
        ss.candidates = out->nnz;
        if (stats) *stats = ss;
        return 0;
    } catch (const std::exception& e) {
        return kmdb_set_error(std::string(who) + ": " + e.what());
    }
}

extern "C" int kmdb_sampled_from_rows_device(kmdb_db* db, const void* rows_dev, size_t nq, uint64_t n_cols, uint64_t cell_lo, uint64_t cell_hi,
                                             const uint32_t* query_kmers, const kmdb_cell_filter* filters, size_t n_filters, const uint32_t* sample_kmers,
                                             int criterion, uint32_t count, kmdb_sparse_rows* out_candidates, const kmdb_opts* opts) {
    const char* who = "kmdb_sampled_from_rows_device";
    if (!db || !out_candidates) return kmdb_set_error(std::string(who) + ": null argument");
    if (check_sample_args(who, filters, n_filters, sample_kmers, criterion, count)) return 1;
    if (nq && !query_kmers) return kmdb_set_error(std::string(who) + ": query_kmers is NULL");
    if (kmdb_sample_query_rows_check(who, nq, n_cols, cell_lo, cell_hi)) return 1;
    if (!rows_dev && cell_hi > cell_lo) return kmdb_set_error(std::string(who) + ": null rows");
    HIP_TRY(hipSetDevice(db->device));
    hipStream_t st = (opts && opts->stream) ? (hipStream_t)opts->stream : db->stream;
    HIP_TRY(hipEventRecord(db->ev[0], st)); HIP_TRY(hipEventRecord(db->ev[1], st)); HIP_TRY(hipEventRecord(db->ev[2], st));
    db->stats.path = KMDB_PATH_NONE;
    db->n2a_sample_stats = kmdb_sample_stats{};
    if (kmdb_sample_query_rows(who, st, (int)db->kmer_length, (const uint32_t*)rows_dev, nq, n_cols, cell_lo, cell_hi, query_kmers, filters, n_filters, sample_kmers,
                               criterion, count, out_candidates, &db->n2a_sample_stats)) return 1;
    if (finish_stats(db, st)) { kmdb_sparse_free(out_candidates); return 1; }
    kmdb_release_staging(db);
    return 0;
}

extern "C" int kmdb_new2all_sample_stats_get(const kmdb_db* db, kmdb_sample_stats* out) {
    if (!db || !out) return kmdb_set_error("kmdb_new2all_sample_stats_get: null argument");
    *out = db->n2a_sample_stats;
    return 0;
}

extern "C" int kmdb_db2db_sample_stats_get(const kmdb_db* db_row, kmdb_sample_stats* out) {
    if (!db_row || !out) return kmdb_set_error("kmdb_db2db_sample_stats_get: null argument");
    *out = db_row->d2_sample_stats;
    return 0;
}

// the argument checks of kmdb_db2db_sampled that need no handle (db2db.hip makes the others)
int kmdb_check_sample_args(const char* who, const kmdb_cell_filter* filters, size_t n_filters, const uint32_t* sample_kmers, int criterion, uint32_t count) {
    return check_sample_args(who, filters, n_filters, sample_kmers, criterion, count);
}

extern "C" int kmdb_sampled_from_dense_device(kmdb_db* db, const void* cells_dev, uint64_t cell_lo, uint64_t cell_hi, const kmdb_cell_filter* filters,
                                              size_t n_filters, const uint32_t* sample_kmers, int criterion, uint32_t count, kmdb_sparse_rows* out_candidates,
                                              const kmdb_opts* opts) {
    const char* who = "kmdb_sampled_from_dense_device";
    if (!db || !out_candidates) return kmdb_set_error(std::string(who) + ": null argument");
    if (check_sample_args(who, filters, n_filters, sample_kmers, criterion, count)) return 1;
    const uint64_t cells = db->N ? db->N * (db->N - 1) / 2 : 0;
    if (cell_hi > cells) cell_hi = cells;
    if (cell_lo > cell_hi) return kmdb_set_error(std::string(who) + ": cell_lo > cell_hi");
    if (!cells_dev && cell_hi > cell_lo) return kmdb_set_error(std::string(who) + ": null matrix");
    return sampled_impl(who, db, true, cells_dev, cell_lo, cell_hi, filters, n_filters, sample_kmers, criterion, count, out_candidates, opts);
}

extern "C" int kmdb_all2all_sampled(kmdb_db* db, const kmdb_cell_filter* filters, size_t n_filters, const uint32_t* sample_kmers, int criterion, uint32_t count,
                                    kmdb_sparse_rows* out, const kmdb_opts* opts) {
    const char* who = "kmdb_all2all_sampled";
    if (!db || !out) return kmdb_set_error(std::string(who) + ": null argument");
    if (check_sample_args(who, filters, n_filters, sample_kmers, criterion, count)) return 1;
    // the rank of a cell is a condition on the whole cell: a slice of the pattern stream (opts->shard_*) holds partial sums only
    if (opts && opts->shard_count > 1) return kmdb_set_error(std::string(who) + ": the selection needs the whole database (shard_count must be 1)");
    kmdb_sparse_rows cand;
    if (sampled_impl(who, db, false, nullptr, 0, ~0ull, filters, n_filters, sample_kmers, criterion, count, &cand, opts)) return 1;
    const kmdb_sparse_rows* parts[1] = {&cand};
    const int rc = kmdbh_sample_rows_select(criterion, count, (int)db->kmer_length, sample_kmers, filters, n_filters, parts, 1, out);
    kmdb_sparse_free(&cand);
    return rc;
}

extern "C" int kmdb_new2all_sparse_stats_get(const kmdb_db* db, kmdb_new2all_sparse_stats* out) {
    if (!db || !out) return kmdb_set_error("kmdb_new2all_sparse_stats_get: null argument");
    *out = db->n2s_stats;
    return 0;
}

extern "C" int kmdb_db2db_stats_get(const kmdb_db* db_row, kmdb_db2db_stats* out) {
    if (!db_row || !out) return kmdb_set_error("kmdb_db2db_stats_get: null argument");
    *out = db_row->d2_stats;
    return 0;
}

extern "C" int kmdb_db_sample_stats(const kmdb_db* db, kmdb_sample_stats* out) {
    if (!db || !out) return kmdb_set_error("kmdb_db_sample_stats: null argument");
    *out = db->sample_stats;
    return 0;
}

extern "C" void kmdb_sparse_free(kmdb_sparse_rows* rows) {
    if (!rows) return;
    std::free(rows->row_ptr); std::free(rows->col); std::free(rows->val); std::free(rows->measure);
    std::memset(rows, 0, sizeof *rows);
}

