// a2a_rows.hip — a band of rows [row_lo, row_hi) of the all2all matrix, accumulated alone: the cells [tri(row_lo), tri(row_hi)) of the lower
// triangle and nothing else of it in HBM (kmdb_all2all_rows_device / kmdb_all2all_rows, include/kmdb_amd.h).
//
// The arithmetic is the tree form of the reference (src/similarity_calculator.cpp:213-233: for every local id of a pattern, its subtree weight
// goes to the cells of all ids in front of it on the root path) as a2a_global_kernel (a2a_v1.hip) states it: node p adds W_p to M[id_t][id_u]
// for every local position t and every u < t of its root-to-leaf list.  A row of the matrix belongs to the LOCAL ids equal to it, so a band
// needs only the nodes with a local id inside it — and of those only the rows inside:
//   rows_select_kernel  a lane per DFS node: the nodes that can have a local id in the band, from the node arrays alone (nothing is decoded)
//   rows_apply_kernel   a fixed grid of waves strides over the selected nodes: the root path is rebuilt on a wave-private id stack (ancestors
//                       decoded a lane each, 64 at a time), then the band rows of the node's own ids are added with HBM atomics
// uint32 adds wrap and commute: the band is bit-exact with the same cells of kmdb_all2all_dense_device in any order.
// Not done here: a node is one wave's work however long its list is (a root with thousands of local ids under a wide band is applied by
// a single wave; splitting it is left open).
#include "band_select.h"
#include "device_common.h"
#include "engine_internal.h"

#include <algorithm>
#include <string>

namespace {

constexpr int ROWS_LDS_CAP = KMDB_ROWS_LDS_CAP;      // (engine_internal.h) a full list of up to this many ids lives on the wave's LDS stack
constexpr uint32_t ROWS_MAX_WAVES = 2048;           // the apply grid: never more waves than this ...
constexpr uint32_t ROWS_MIN_WAVES = 64;             // ... never fewer, and in between as many as ROWS_STACK_BUDGET words of id stacks allow
constexpr uint64_t ROWS_STACK_BUDGET = 64ull << 20; // words (256 MB)

struct RowsParams {
    const uint4* meta;
    const uint64_t* bitpos;
    const int32_t* parent;
    const uint32_t* sub_end;
    const uint32_t* wprefix;
    const uint64_t* bits;
    uint32_t P;
    uint32_t row_lo, row_hi;
    uint64_t cell_lo;               // tri64(row_lo): out points at this cell
    uint32_t* out;
    uint32_t* sel;                  // [P] the selected nodes, any order
    unsigned long long* counters;   // [0] nodes selected, [1] nodes with a band row, [2] cell additions
    uint32_t* stack_scratch;        // per-wave id stacks
    uint32_t stack_stride;          // words per wave (>= N)
    uint32_t n_waves;
};

// the select rule and its compaction: band_select.h
__global__ __launch_bounds__(256) void rows_select_kernel(RowsParams p) { band_select_nodes(p); }

// One selected node on the id stack `stack` (LDS or global scratch; stack[0 .. n) is the node's full list when this returns to the adds).
// GLOBAL: the stack is global memory — its writes are fenced for the wave's other lanes; an LDS stack needs the compiler kept in order only.
template <bool GLOBAL>
__device__ __forceinline__ void rows_apply_node(const RowsParams& p, uint32_t node, uint32_t n, uint32_t l, uint32_t W, uint32_t* stack, uint32_t lane,
                                                unsigned long long& applied, unsigned long long& updates) {
    // the chain node -> root, 64 nodes at a time: lane k of a batch decodes the k-th of them to its place n_k - l_k of the stack
    int32_t cur = (int32_t)node;
    while (cur >= 0) {
        int32_t mine = -1;
        for (uint32_t k = 0; k < (uint32_t)WAVE && cur >= 0; ++k) {
            if (lane == k) mine = cur;
            cur = p.parent[cur];
        }
        if (mine >= 0) {
            const uint4 m = p.meta[mine];
            decode_node<uint32_t>(p.bits, p.bitpos[mine], m.y, m.z, stack + (m.x - m.y));
        }
    }
    if (GLOBAL) wave_sync(); else lds_sync();
    // the rows: local positions [n - l, n) whose id is inside the band (ids ascend: one stretch of them)
    const uint32_t top = n - l;
    uint32_t rows = 0;
    for (uint32_t t0 = top; t0 < n; t0 += WAVE) {
        const uint32_t t = t0 + lane;
        const uint32_t id = t < n ? stack[t] : 0xFFFFFFFFu;
        unsigned long long m = __ballot(t < n && id >= p.row_lo && id < p.row_hi);
        while (m) {
            const uint32_t b = (uint32_t)__builtin_ctzll(m);
            m &= m - 1;
            const uint32_t tt = t0 + b;
            const uint64_t rb = tri64(bcast(id, b)) - p.cell_lo;
            for (uint32_t u = lane; u < tt; u += WAVE) atomicAdd(&p.out[rb + stack[u]], W);
            ++rows;
            updates += tt;
        }
        if (bcast(id, 0) >= p.row_hi) break;
    }
    applied += rows ? 1u : 0u;
    if (GLOBAL) wave_sync(); else lds_sync();
}

__global__ __launch_bounds__(WAVE * WAVES_PER_BLOCK) void rows_apply_kernel(RowsParams p) {
    __shared__ uint32_t lds_stack[WAVES_PER_BLOCK][ROWS_LDS_CAP];
    const uint32_t lane = lane_id();
    const uint32_t wave = threadIdx.x >> 6;
    const uint32_t gw = blockIdx.x * WAVES_PER_BLOCK + wave;
    if (gw >= p.n_waves) return;
    const uint32_t n_sel = (uint32_t)p.counters[0];
    uint32_t* gstack = p.stack_scratch + (size_t)gw * p.stack_stride;
    unsigned long long applied = 0, updates = 0;
    for (uint32_t s = gw; s < n_sel; s += p.n_waves) {
        const uint32_t node = __builtin_amdgcn_readfirstlane(p.sel[s]);
        const uint4 m = p.meta[node];
        const uint32_t n = __builtin_amdgcn_readfirstlane(m.x), l = __builtin_amdgcn_readfirstlane(m.y);
        const uint32_t W = __builtin_amdgcn_readfirstlane(p.wprefix[p.sub_end[node]] - p.wprefix[node]);
        if (n <= (uint32_t)ROWS_LDS_CAP) rows_apply_node<false>(p, node, n, l, W, &lds_stack[wave][0], lane, applied, updates);
        else rows_apply_node<true>(p, node, n, l, W, gstack, lane, applied, updates);
    }
    if (lane == 0 && applied) atomicAdd(&p.counters[1], applied);
    if (lane == 0 && updates) atomicAdd(&p.counters[2], updates);
}

// what the band path keeps on the handle between calls
uint64_t rows_device_bytes(const kmdb_db* db) { return db->rows_sel.bytes() + db->rows_counters.bytes(); }

int rows_run(const char*, kmdb_db* db, uint32_t* out, uint64_t row_lo, uint64_t row_hi, const kmdb_opts*, hipStream_t st) {
    const uint64_t N = db->N, P = db->P;
    const uint64_t band_cells = kmdb_tri(row_hi) - kmdb_tri(row_lo);
    kmdb_all2all_rows_stats& rs = db->rows_stats;
    rs = kmdb_all2all_rows_stats{};
    rs.band_cells = band_cells;
    HIP_TRY(hipEventRecord(db->ev[0], st));
    bool ran = false;
    if (row_hi > row_lo && P) {                                     // (row 0 alone has no cell, but a node may hold it: the stats count that node)
        if (!db->rows_sel) {
            DEV_ALLOC(db->rows_sel, P);
            DEV_ALLOC(db->rows_counters, 4);
        }
        const size_t stride = (N + 63) / 64 * 64;
        uint32_t n_waves = (uint32_t)std::min<uint64_t>(ROWS_MAX_WAVES, std::max<uint64_t>(ROWS_MIN_WAVES, ROWS_STACK_BUDGET / stride));
        n_waves = n_waves / WAVES_PER_BLOCK * WAVES_PER_BLOCK;
        const size_t words = (size_t)n_waves * stride;             // (at most ROWS_STACK_BUDGET, or ROWS_MIN_WAVES stacks)
        if (db->stack_scratch_words < words) {
            db->stack_scratch_words = 0;
            DEV_ALLOC(db->stack_scratch, words);
            db->stack_scratch_words = words;
        }
        rs.scratch_bytes = db->rows_sel.bytes() + db->rows_counters.bytes() + db->stack_scratch.bytes();
        if (band_cells) HIP_TRY(hipMemsetAsync(out, 0, band_cells * 4, st));
        HIP_TRY(hipMemsetAsync(db->rows_counters, 0, 4 * sizeof(unsigned long long), st));
        RowsParams p{};
        if (band_node_params(db, p, out, row_lo, row_hi, st)) return 1;
        p.sel = db->rows_sel; p.counters = db->rows_counters; p.stack_scratch = db->stack_scratch; p.stack_stride = (uint32_t)stride; p.n_waves = n_waves;
        HIP_TRY(hipEventRecord(db->ev[1], st));
        hipLaunchKernelGGL(rows_select_kernel, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, st, p);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipEventRecord(db->ev[2], st));
        hipLaunchKernelGGL(rows_apply_kernel, dim3(n_waves / WAVES_PER_BLOCK), dim3(WAVE * WAVES_PER_BLOCK), 0, st, p);
        HIP_TRY(hipGetLastError());
        ran = true;
    } else if (band_cells) {
        HIP_TRY(hipMemsetAsync(out, 0, band_cells * 4, st));
    }
    HIP_TRY(hipEventRecord(db->ev[3], st));
    HIP_TRY(hipEventSynchronize(db->ev[3]));
    float ms = 0;
    HIP_TRY(hipEventElapsedTime(&ms, db->ev[0], db->ev[3]));
    db->stats.kernel_ms = ms;
    if (ran) {
        HIP_TRY(hipEventElapsedTime(&ms, db->ev[1], db->ev[2]));
        rs.select_ms = ms;
        HIP_TRY(hipEventElapsedTime(&ms, db->ev[2], db->ev[3]));
        rs.apply_ms = ms;
        unsigned long long c[4];
        HIP_TRY(hipMemcpy(c, db->rows_counters, sizeof c, hipMemcpyDeviceToHost));
        rs.nodes_selected = c[0]; rs.nodes_applied = c[1]; rs.updates = c[2];
    }
    kmdb_recount_bytes(db, db->rows_bytes_counted, rows_device_bytes(db));
    return 0;
}

}  // namespace

// argument checks shared by every band call (engine_internal.h); 0, or 1 with the error set
int kmdb_band_check(const char* who, const kmdb_db* db, uint64_t row_lo, uint64_t row_hi, const kmdb_opts* opts) {
    const std::string w(who);
    if (row_lo > row_hi) return kmdb_set_error(w + ": row_lo > row_hi (" + std::to_string(row_lo) + " > " + std::to_string(row_hi) + ")");
    if (row_hi > db->N) return kmdb_set_error(w + ": row_hi " + std::to_string(row_hi) + " > the " + std::to_string(db->N) + " samples of the database");
    if (opts && opts->shard_count > 1) return kmdb_set_error(w + ": a band needs the whole pattern stream (shard_count must be 1)");
    if (opts && (opts->flags & ~KMDB_FLAG_ALL)) return kmdb_set_error(w + ": unknown bits in kmdb_opts.flags");
    if (db->qs_count > 1) return kmdb_set_error(w + ": not on a query shard (kmdb_db_upload_query_shard): its tree holds one shard's k-mers only");
    return 0;
}

// a band too large to exist: from 2^32 cells on, its bytes against `limit` bytes of device memory
int kmdb_band_check_bytes(const char* who, uint64_t band_cells, bool against_free) {
    if (band_cells < (1ull << 32)) return 0;
    size_t free_b = 0, total_b = 0;
    HIP_TRY(hipMemGetInfo(&free_b, &total_b));
    const uint64_t limit = against_free ? free_b : total_b;
    if (band_cells > limit / 4)
        return kmdb_set_error(std::string(who) + ": the band is " + std::to_string(band_cells) + " cells, " + std::to_string(band_cells * 4) + " bytes, beyond the " +
                              std::to_string(limit) + " bytes of " + (against_free ? "free device memory" : "device memory"));
    return 0;
}

// Everything the six band entry points share, in one order: the refusals — null handle; range, shard, flags, query shard; null buffer for a band with
// cells; a band beyond the device — then the stream, the form's runner (on a band buffer of the call's own when `out` is host memory: made, copied back
// and released here) and the upload's host buffers given back.
int kmdb_band_call(const char* who, kmdb_db* db, uint64_t row_lo, uint64_t row_hi, void* out, bool host_out, const kmdb_opts* opts, kmdb_band_runner run) {
    if (!db) return kmdb_set_error(std::string(who) + ": null argument");
    if (kmdb_band_check(who, db, row_lo, row_hi, opts)) return 1;
    const uint64_t band_cells = kmdb_tri(row_hi) - kmdb_tri(row_lo);
    if (!out && band_cells) return kmdb_set_error(std::string(who) + ": null argument");
    HIP_TRY(hipSetDevice(db->device));
    if (kmdb_band_check_bytes(who, band_cells, host_out)) return 1;
    DevBuf<uint32_t> band;
    if (host_out) DEV_ALLOC(band, std::max<uint64_t>(band_cells, 1));
    hipStream_t st = (opts && opts->stream) ? (hipStream_t)opts->stream : db->stream;
    int rc = run(who, db, host_out ? band.get() : (uint32_t*)out, row_lo, row_hi, opts, st);
    if (host_out && !rc && band_cells && hipMemcpy(out, band, band_cells * 4, hipMemcpyDeviceToHost) != hipSuccess)
        rc = kmdb_set_error(std::string(who) + ": copy back failed");
    band.reset();
    kmdb_release_staging(db);
    return rc;
}

extern "C" int kmdb_all2all_rows_device(kmdb_db* db, uint64_t row_lo, uint64_t row_hi, void* out_cells_dev, const kmdb_opts* opts) {
    return kmdb_band_call("kmdb_all2all_rows_device", db, row_lo, row_hi, out_cells_dev, false, opts, rows_run);
}
extern "C" int kmdb_all2all_rows(kmdb_db* db, uint64_t row_lo, uint64_t row_hi, uint32_t* out_cells_host, const kmdb_opts* opts) {
    return kmdb_band_call("kmdb_all2all_rows", db, row_lo, row_hi, out_cells_host, true, opts, rows_run);
}

// Device memory for a caller that has no HIP of its own (the command-line front-end keeps a band between the band call and its consumers)
extern "C" int kmdb_device_buffer_alloc(int32_t device, uint64_t bytes, void** out) {
    if (!out) return kmdb_set_error("kmdb_device_buffer_alloc: null argument");
    *out = nullptr;
    HIP_TRY(hipSetDevice(device));
    const hipError_t e = hipMalloc(out, std::max<uint64_t>(bytes, 1));
    if (e != hipSuccess) { *out = nullptr; return kmdb_set_error("kmdb_device_buffer_alloc: hipMalloc of " + std::to_string(bytes) + " B: " + hipGetErrorString(e)); }
    return 0;
}
extern "C" void kmdb_device_buffer_free(int32_t device, void* p) {
    if (!p) return;
    if (hipSetDevice(device) != hipSuccess) { (void)hipGetLastError(); return; }
    (void)hipFree(p);
}

extern "C" int kmdb_all2all_rows_stats_get(const kmdb_db* db, kmdb_all2all_rows_stats* out) {
    if (!db || !out) return kmdb_set_error("kmdb_all2all_rows_stats_get: null argument");
    *out = db->rows_stats;
    return 0;
}
