// a2a_band.hip — the band of rows [row_lo, row_hi) of the all2all matrix with its rows summed in LDS tiles (kmdb_all2all_rows_tiled_device /
// kmdb_all2all_rows_tiled), and a whole sparse run walked in such bands (kmdb_all2all_sparse_filtered_banded); include/kmdb_amd.h.
//
// The arithmetic is that of a2a_rows.hip: row r of the matrix is written only by the nodes that hold r as a local id, and such a node adds its
// subtree weight W to column c for every id c < r of its root path (full lists ascend strictly: "in front of r" is "id < r", no position and no id
// stack are needed).  uint32 adds form a group, so a run of consecutive ids [s, s + len) is entered into a tile as a difference, +W at s and -W
// (modulo 2^32) at s + len, and one inclusive prefix sum over the tile gives the cells exactly.
//   band_select_kernel  a lane per DFS node: the superset rule of rows_select_kernel, the same code (band_select.h)
//   band_hits_kernel    a lane per selected node walks the node's OWN list and finds its ids inside the band (a "hit" = (row, node)): a count
//                       pass, an exclusive sum of the per-row counts, a write pass — the hits grouped by row, sizes known before anything is written
//   (host)              the job table from one copy of the per-row counts: job = (row r, tile [c0, c0 + T) with c0 < r, a share of the row's hits)
//   band_apply_kernel   a workgroup per job: the tile zeroed in LDS, a wave per hit follows `parent` to the root 64 chain nodes at a time, a lane per
//                       chain node runs gamma_runs over its list and enters the runs clipped to the tile and to ids < r; after a barrier one
//                       workgroup-wide inclusive scan, and every non-zero cell goes to the zeroed band with one atomicAdd (shares of a tile meet there)
// Not done here: the list of one node is decoded by one lane per hit however long it is — a root with thousands of local ids inside the band is
// thousands of hits in different rows, spread over workgroups, but each of them decodes the list again (a wave-cooperative decode: DESIGN.md §4).
#include "band_select.h"
#include "device_common.h"
#include "engine_internal.h"
#include "prim.h"

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

namespace {

constexpr uint32_t BAND_THREADS = WAVE * WAVES_PER_BLOCK;
constexpr uint32_t BAND_TILE_COLS_MAX = 40896;          // 639 * 64 words: 160 KiB of LDS less the 256 bytes kept for the scan's and the counters' words
constexpr uint32_t BAND_TILE_COLS_DEFAULT = 16384;      // (profiles/all2all_band_ab.json)
constexpr uint32_t BAND_TILE_HITS_DEFAULT = 256;
constexpr uint32_t BAND_HITS_LDS_ROWS = 1024;           // the hit passes of a band of up to this many rows count per row in LDS (8 KB a workgroup in the write pass)

struct BandParams {
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
    unsigned long long* counters;   // [0] nodes selected, [1] nodes with a hit, [2] hits, [3] runs, [4] cell additions
    uint32_t* row_cnt;              // [rows + 1] hits of every row of the band (the last word stays 0)
    uint32_t* row_ofs;              // [rows + 1] its exclusive sum
    uint32_t* row_cur;              // [rows + 1] the write pass's cursor inside a row's group
    uint32_t* hit_node;             // [hits]
    const uint4* jobs;              // {row, c0, first hit, hits}
    uint32_t tile_cols;
    uint32_t hits_lds;              // 1: the hit passes count per row in LDS first (a band of at most BAND_HITS_LDS_ROWS rows)
};

// the select rule and its compaction: band_select.h
__global__ __launch_bounds__(256) void band_select_kernel(BandParams p) { band_select_nodes(p); }

// A lane per selected node: the ids of the node's own list inside the band.  WRITE false: they are counted per row (and the node, and its hits,
// in the counters); true: every one takes the next place of its row's group, which the count pass sized.
// A band has few rows and many hits: one HBM atomic per hit on a row's counter serialises (measured: 1.6 M hits on 16 rows, 10 ms a pass).  With
// p.hits_lds (a band of at most BAND_HITS_LDS_ROWS rows) a workgroup counts its hits per row in LDS first and goes to the row's counter once:
// with the sum (count pass), or for the base of its own stretch of the row's group, inside which its hits rank themselves in LDS (write pass).
template <bool WRITE, class F>
__device__ __forceinline__ void band_own_rows(const BandParams& p, uint32_t node, F&& hit) {
    const uint4 m = p.meta[node];
    const uint64_t pos = p.bitpos[node];
    const uint32_t first = gamma_first_id<1, true>(p.bits, pos, m.y, m.z);
    if (first >= p.row_hi) return;
    GammaCursor<1> c(p.bits, pos);
    gamma_runs(c, first, m.y, [&](uint32_t s, uint32_t len) {
        const uint32_t a = s > p.row_lo ? s : p.row_lo, b = s + len < p.row_hi ? s + len : p.row_hi;
        for (uint32_t r = a; r < b; ++r) hit(r - p.row_lo);
    });
}

template <bool WRITE>
__global__ __launch_bounds__(256) void band_hits_kernel(BandParams p) {
    extern __shared__ uint32_t rows_lds[];                          // hits_lds: [rows] counts / ranks, and for the write pass [rows] bases behind them
    const uint32_t n_sel = (uint32_t)p.counters[0];
    if (blockIdx.x * blockDim.x >= n_sel) return;                   // (the whole workgroup)
    const uint32_t tid = threadIdx.x, i = blockIdx.x * blockDim.x + tid, rows = p.row_hi - p.row_lo;
    const bool active = i < n_sel;
    const uint32_t node = active ? p.sel[i] : 0u;
    if (!p.hits_lds) {
        if (!active) return;
        uint32_t found = 0;
        band_own_rows<WRITE>(p, node, [&](uint32_t k) {
            if (WRITE) p.hit_node[p.row_ofs[k] + atomicAdd(&p.row_cur[k], 1u)] = node;
            else atomicAdd(&p.row_cnt[k], 1u);
            ++found;
        });
        if (!WRITE && found) {
            atomicAdd(&p.counters[1], 1ull);
            atomicAdd(&p.counters[2], (unsigned long long)found);
        }
        return;
    }
    __shared__ uint32_t group[2];                                   // nodes with a hit, hits of the workgroup
    uint32_t* const cnt = rows_lds;
    uint32_t* const base = rows_lds + rows;                         // (write pass only)
    for (uint32_t k = tid; k < rows; k += blockDim.x) cnt[k] = 0;
    if (tid < 2) group[tid] = 0;
    __syncthreads();
    uint32_t found = 0;
    if (active) band_own_rows<WRITE>(p, node, [&](uint32_t k) { atomicAdd(&cnt[k], 1u); ++found; });
    if (!WRITE && found) {
        atomicAdd(&group[0], 1u);
        atomicAdd(&group[1], found);
    }
    __syncthreads();
    if (!WRITE && tid == 0 && group[0]) {
        atomicAdd(&p.counters[1], (unsigned long long)group[0]);
        atomicAdd(&p.counters[2], (unsigned long long)group[1]);
    }
    for (uint32_t k = tid; k < rows; k += blockDim.x) {
        const uint32_t c = cnt[k];
        if (!WRITE) { if (c) atomicAdd(&p.row_cnt[k], c); }
        else { base[k] = c ? p.row_ofs[k] + atomicAdd(&p.row_cur[k], c) : 0u; cnt[k] = 0; }
    }
    if (!WRITE) return;
    __syncthreads();
    if (active) band_own_rows<WRITE>(p, node, [&](uint32_t k) { p.hit_node[base[k] + atomicAdd(&cnt[k], 1u)] = node; });
}

__global__ __launch_bounds__(BAND_THREADS) void band_apply_kernel(BandParams p) {
    extern __shared__ __align__(16) uint32_t tile[];                // [tile_cols]: differences, then nothing — the scan leaves through registers
    __shared__ uint32_t wsum[2][WAVES_PER_BLOCK];
    __shared__ unsigned long long done[2];                          // runs, cell additions of the workgroup
    const uint32_t tid = threadIdx.x, lane = lane_id(), wave = tid >> 6;
    const uint4 job = p.jobs[blockIdx.x];
    const uint32_t r = job.x, c0 = job.y;
    const uint32_t cend = c0 + p.tile_cols < r ? c0 + p.tile_cols : r;      // columns [c0, cend) of row r: c0 < r
    const uint32_t wlen = cend - c0, n4 = (wlen + 3u) / 4u;         // (tile_cols is a multiple of 4: 4 * n4 <= tile_cols)
    for (uint32_t i = tid; i < n4; i += BAND_THREADS) ((uint4*)tile)[i] = make_uint4(0, 0, 0, 0);
    if (tid < 2) done[tid] = 0;
    __syncthreads();

    unsigned long long runs = 0, updates = 0;
    for (uint32_t h = wave; h < job.w; h += WAVES_PER_BLOCK) {
        const uint32_t node = __builtin_amdgcn_readfirstlane(p.hit_node[job.z + h]);
        const uint32_t W = __builtin_amdgcn_readfirstlane(p.wprefix[p.sub_end[node]] - p.wprefix[node]);
        // the chain node -> root, 64 nodes at a time: lane k of a batch takes the k-th of them
        int32_t cur = (int32_t)node;
        while (cur >= 0) {
            int32_t mine = -1;
            for (uint32_t k = 0; k < (uint32_t)WAVE && cur >= 0; ++k) {
                if (lane == k) mine = cur;
                cur = p.parent[cur];
            }
            if (mine < 0) continue;
            const uint4 m = p.meta[mine];
            if (m.y == 0 || m.z < c0) continue;                      // no ids of its own, or all of them in front of the tile
            int32_t q = p.parent[mine];
            while (q >= 0 && p.meta[q].y == 0) q = p.parent[q];
            if (q >= 0 && p.meta[q].z + 1u >= cend) continue;        // its ids lie in (parent's last id, own last id]: all behind the tile
            const uint64_t pos = p.bitpos[mine];
            const uint32_t first = gamma_first_id<1, true>(p.bits, pos, m.y, m.z);
            if (first >= cend) continue;
            GammaCursor<1> c(p.bits, pos);
            gamma_runs(c, first, m.y, [&](uint32_t s, uint32_t len) {
                const uint32_t a = s > c0 ? s : c0, b = s + len < cend ? s + len : cend;
                if (a < b) {
                    atomicAdd(&tile[a - c0], W);
                    if (b < cend) atomicAdd(&tile[b - c0], 0u - W);  // (left out on the tile's end and at r: nothing is summed behind them)
                    ++runs;
                    updates += b - a;
                }
            });
        }
    }
    if (runs) { atomicAdd(&done[0], runs); atomicAdd(&done[1], updates); }
    __syncthreads();

    // the inclusive scan of the tile, 4 words a thread and 1024 a round; a cell leaves from the registers that hold its sum
    uint32_t* const row = p.out + ((tri64((uint64_t)r) - p.cell_lo) + c0);
    uint32_t carry = 0, buf = 0;
    for (uint32_t base = 0; base < n4; base += BAND_THREADS, buf ^= 1u) {
        const uint32_t i = base + tid;
        uint4 v = i < n4 ? ((const uint4*)tile)[i] : make_uint4(0, 0, 0, 0);
        v.y += v.x; v.z += v.y; v.w += v.z;
        const uint32_t incl = wave_incl_scan(v.w, lane);
        if (lane == (uint32_t)WAVE - 1u) wsum[buf][wave] = incl;
        __syncthreads();
        uint32_t off = carry + incl - v.w, total = carry;
        for (uint32_t w = 0; w < (uint32_t)WAVES_PER_BLOCK; ++w) {
            const uint32_t s = wsum[buf][w];
            if (w < wave) off += s;
            total += s;
        }
        carry = total;
        v.x += off; v.y += off; v.z += off; v.w += off;
        const uint32_t c = 4u * i;                                   // column c0 + c
        if (c < wlen && v.x) atomicAdd(&row[c], v.x);
        if (c + 1u < wlen && v.y) atomicAdd(&row[c + 1u], v.y);
        if (c + 2u < wlen && v.z) atomicAdd(&row[c + 2u], v.z);
        if (c + 3u < wlen && v.w) atomicAdd(&row[c + 3u], v.w);
    }
    if (tid == 0 && done[0]) { atomicAdd(&p.counters[3], done[0]); atomicAdd(&p.counters[4], done[1]); }
}

// what the tiled call keeps on the handle between calls
uint64_t band_device_bytes(const kmdb_db* db) {
    return db->band_sel.bytes() + db->band_counters.bytes() + db->band_rows.bytes() + db->band_hits.bytes() + db->band_jobs.bytes() + db->band_scan_tmp.bytes();
}

// KMDB_ROWS_TILE_COLS / KMDB_ROWS_TILE_HITS, read at every call (tests and A/B)
int band_switches(const char* who, uint32_t& tile_cols, uint32_t& tile_hits) {
    tile_cols = BAND_TILE_COLS_DEFAULT;
    tile_hits = BAND_TILE_HITS_DEFAULT;
    if (const char* e = std::getenv("KMDB_ROWS_TILE_COLS")) {
        char* end = nullptr;
        const unsigned long long v = std::strtoull(e, &end, 10);
        if (!*e || *end || v < 64 || v % 64 || v > BAND_TILE_COLS_MAX)
            return kmdb_set_error(std::string(who) + ": KMDB_ROWS_TILE_COLS=" + e + ": a multiple of 64 from 64 to " + std::to_string(BAND_TILE_COLS_MAX) + " is expected");
        tile_cols = (uint32_t)v;
    }
    if (const char* e = std::getenv("KMDB_ROWS_TILE_HITS")) {
        char* end = nullptr;
        const unsigned long long v = std::strtoull(e, &end, 10);
        if (!*e || *end || v < 1 || v > 0xFFFFFFFFull) return kmdb_set_error(std::string(who) + ": KMDB_ROWS_TILE_HITS=" + e + ": a count of 1 or more is expected");
        tile_hits = (uint32_t)v;
    }
    return 0;
}

int band_run(const char* who, kmdb_db* db, uint32_t* out, uint64_t row_lo, uint64_t row_hi, const kmdb_opts*, hipStream_t st) {
    const uint64_t P = db->P;
    const uint64_t band_cells = kmdb_tri(row_hi) - kmdb_tri(row_lo);
    uint32_t tile_cols = 0, tile_hits = 0;
    if (band_switches(who, tile_cols, tile_hits)) return 1;
    kmdb_all2all_rows_tiled_stats& bs = db->band_stats;
    bs = kmdb_all2all_rows_tiled_stats{};
    bs.band_cells = band_cells;
    bs.tile_cols = tile_cols;
    if (!db->band_ev && db->band_ev.create()) return 1;
    HIP_TRY(hipEventRecord(db->ev[0], st));
    bool ran = false;
    uint64_t n_jobs = 0;
    if (row_hi > row_lo && P) {                                     // (row 0 alone has no cell, but a node may hold it: the stats count that node)
        const uint64_t rows1 = row_hi - row_lo + 1;
        if (!db->band_sel) {
            DEV_ALLOC(db->band_sel, P);
            DEV_ALLOC(db->band_counters, 8);
        }
        if (db->band_rows_cap < rows1) {
            db->band_rows_cap = 0;
            DEV_ALLOC(db->band_rows, 3 * rows1);
            db->band_rows_cap = rows1;
        }
        size_t scan_bytes = 0;
        HIP_TRY(prim::exclusive_sum(nullptr, scan_bytes, (const uint32_t*)nullptr, (uint32_t*)nullptr, (size_t)rows1, st));
        if (db->band_scan_tmp_bytes < scan_bytes) {
            db->band_scan_tmp_bytes = 0;
            DEV_ALLOC_BYTES(db->band_scan_tmp, scan_bytes);
            db->band_scan_tmp_bytes = std::max<size_t>(scan_bytes, 16);
        }
        if (band_cells) HIP_TRY(hipMemsetAsync(out, 0, band_cells * 4, st));
        HIP_TRY(hipMemsetAsync(db->band_counters, 0, 8 * sizeof(unsigned long long), st));
        HIP_TRY(hipMemsetAsync(db->band_rows, 0, 3 * rows1 * sizeof(uint32_t), st));
        BandParams p{};
        if (band_node_params(db, p, out, row_lo, row_hi, st)) return 1;
        p.sel = db->band_sel; p.counters = db->band_counters;
        p.row_cnt = db->band_rows; p.row_ofs = db->band_rows + rows1; p.row_cur = db->band_rows + 2 * rows1;
        p.tile_cols = tile_cols;
        p.hits_lds = row_hi - row_lo <= BAND_HITS_LDS_ROWS ? 1u : 0u;
        const size_t hits_lds_bytes = p.hits_lds ? (size_t)(row_hi - row_lo) * sizeof(uint32_t) : 0;
        const dim3 node_grid((unsigned)((P + 255) / 256));
        HIP_TRY(hipEventRecord(db->ev[1], st));
        hipLaunchKernelGGL(band_select_kernel, node_grid, dim3(256), 0, st, p);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipEventRecord(db->ev[2], st));
        // the hits: count, scan, (sizes to the host,) write
        hipLaunchKernelGGL(band_hits_kernel<false>, node_grid, dim3(256), hits_lds_bytes, st, p);
        HIP_TRY(hipGetLastError());
        size_t tmp_bytes = db->band_scan_tmp_bytes;
        HIP_TRY(prim::exclusive_sum(db->band_scan_tmp.get(), tmp_bytes, (const uint32_t*)p.row_cnt, p.row_ofs, (size_t)rows1, st));
        unsigned long long c[8];
        std::vector<uint32_t> cnt(rows1);
        HIP_TRY(hipMemcpyAsync(c, db->band_counters, sizeof c, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(cnt.data(), p.row_cnt, rows1 * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        const uint64_t hits = c[2];
        if (hits > 0xFFFFFFFFull) return kmdb_set_error(std::string(who) + ": " + std::to_string(hits) + " local ids inside the band: more than 2^32 - 1 (take fewer rows)");
        // the job table: for a row r > 0 with hits, every tile in front of r times every share of its hits
        std::vector<uint4> jobs;
        uint64_t first_hit = 0;
        for (uint64_t k = 0; k + 1 < rows1; ++k) {
            const uint64_t r = row_lo + k, h = cnt[k];
            if (r && h)
                for (uint64_t c0 = 0; c0 < r; c0 += tile_cols)
                    for (uint64_t s = 0; s < h; s += tile_hits)
                        jobs.push_back(make_uint4((uint32_t)r, (uint32_t)c0, (uint32_t)(first_hit + s), (uint32_t)std::min<uint64_t>(tile_hits, h - s)));
            first_hit += h;
        }
        n_jobs = jobs.size();
        if (n_jobs > 0x7FFFFFFFull) return kmdb_set_error(std::string(who) + ": " + std::to_string(n_jobs) + " jobs: more than one launch takes (take fewer rows, or a larger KMDB_ROWS_TILE_HITS)");
        if (hits) {
            if (db->band_hits_cap < hits) {
                db->band_hits_cap = 0;
                DEV_ALLOC(db->band_hits, hits);
                db->band_hits_cap = hits;
            }
            p.hit_node = db->band_hits;
            hipLaunchKernelGGL(band_hits_kernel<true>, node_grid, dim3(256), 2 * hits_lds_bytes, st, p);
            HIP_TRY(hipGetLastError());
        }
        if (n_jobs) {
            if (db->band_jobs_cap < n_jobs) {
                db->band_jobs_cap = 0;
                DEV_ALLOC(db->band_jobs, n_jobs);
                db->band_jobs_cap = n_jobs;
            }
            HIP_TRY(hipMemcpyAsync(db->band_jobs, jobs.data(), n_jobs * sizeof(uint4), hipMemcpyHostToDevice, st));
            HIP_TRY(hipStreamSynchronize(st));                      // (`jobs` is pageable and ends with this scope)
            p.jobs = db->band_jobs;
        }
        HIP_TRY(hipEventRecord(db->band_ev, st));
        if (n_jobs) {
            // (the tile's words: no row of the band has more than row_hi - 1 columns, and a smaller tile lets more workgroups share a CU)
            const size_t lds = (size_t)std::min<uint64_t>(tile_cols, (row_hi - 1 + 3) / 4 * 4) * sizeof(uint32_t);
            HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(band_apply_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
            hipLaunchKernelGGL(band_apply_kernel, dim3((unsigned)n_jobs), dim3(BAND_THREADS), lds, st, p);
            HIP_TRY(hipGetLastError());
        }
        bs.scratch_bytes = band_device_bytes(db);
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
        bs.select_ms = ms;
        HIP_TRY(hipEventElapsedTime(&ms, db->ev[2], db->band_ev));
        bs.hits_ms = ms;
        HIP_TRY(hipEventElapsedTime(&ms, db->band_ev, db->ev[3]));
        bs.apply_ms = ms;
        unsigned long long c[8];
        HIP_TRY(hipMemcpy(c, db->band_counters, sizeof c, hipMemcpyDeviceToHost));
        bs.nodes_selected = c[0]; bs.nodes_applied = c[1]; bs.hits = c[2]; bs.runs = c[3]; bs.updates = c[4];
        bs.jobs = n_jobs;
    }
    kmdb_recount_bytes(db, db->band_bytes_counted, band_device_bytes(db));
    return 0;
}

}  // namespace

extern "C" int kmdb_all2all_rows_tiled_device(kmdb_db* db, uint64_t row_lo, uint64_t row_hi, void* out_cells_dev, const kmdb_opts* opts) {
    return kmdb_band_call("kmdb_all2all_rows_tiled_device", db, row_lo, row_hi, out_cells_dev, false, opts, band_run);
}
extern "C" int kmdb_all2all_rows_tiled(kmdb_db* db, uint64_t row_lo, uint64_t row_hi, uint32_t* out_cells_host, const kmdb_opts* opts) {
    return kmdb_band_call("kmdb_all2all_rows_tiled", db, row_lo, row_hi, out_cells_host, true, opts, band_run);
}

extern "C" int kmdb_all2all_rows_tiled_stats_get(const kmdb_db* db, kmdb_all2all_rows_tiled_stats* out) {
    if (!db || !out) return kmdb_set_error("kmdb_all2all_rows_tiled_stats_get: null argument");
    *out = db->band_stats;
    return 0;
}

// kmdb_all2all_sparse_filtered walked in bands: one band buffer, the band call of `path` (KMDB_BAND_PATH_*: the tiled call here, the tree call of
// a2a_rows.hip, the block-record pipeline's of a2a_rows_records.hip), the compaction of the cells where they lie, the rows appended
static int banded_run(const char* who, kmdb_db* db, uint64_t band_rows, int path, const kmdb_cell_filter* filters, size_t n_filters, const uint32_t* sample_kmers,
                      int measure, kmdb_sparse_rows* out, const kmdb_opts* opts) {
    if (!db || !out) return kmdb_set_error(std::string(who) + ": null argument");
    if (path != KMDB_BAND_PATH_TILED && path != KMDB_BAND_PATH_TREE && path != KMDB_BAND_PATH_RECORDS)
        return kmdb_set_error(std::string(who) + ": unknown path " + std::to_string(path) + " (KMDB_BAND_PATH_TILED, _TREE or _RECORDS)");
    if (band_rows == 0) return kmdb_set_error(std::string(who) + ": band_rows is 0 (a band holds one row at least)");
    if (kmdb_check_filters(who, filters, n_filters, sample_kmers, measure)) return 1;
    const uint64_t N = db->N;
    if (kmdb_band_check(who, db, 0, N, opts)) return 1;
    HIP_TRY(hipSetDevice(db->device));
    uint64_t max_cells = 0;
    for (uint64_t lo = 0; lo < N; lo += std::min<uint64_t>(band_rows, N - lo)) {
        const uint64_t hi = lo + std::min<uint64_t>(band_rows, N - lo);
        max_cells = std::max(max_cells, kmdb_tri(hi) - kmdb_tri(lo));
    }
    if (kmdb_band_check_bytes(who, max_cells, true)) return 1;
    kmdb_all2all_banded_stats bt{};
    kmdb_all2all_banded_records_stats br{};
    bt.max_band_bytes = max_cells * 4;
    DevBuf<uint32_t> band;
    DEV_ALLOC(band, std::max<uint64_t>(max_cells, 1));
    hipStream_t st = (opts && opts->stream) ? (hipStream_t)opts->stream : db->stream;
    std::vector<uint64_t> row_ptr(N + 1, 0);
    std::vector<uint32_t> col, val;
    std::vector<double> meas;
    int rc = 0;
    for (uint64_t lo = 0; lo < N && !rc;) {
        const uint64_t hi = lo + std::min<uint64_t>(band_rows, N - lo);
        if (path == KMDB_BAND_PATH_TILED) rc = band_run(who, db, band, lo, hi, opts, st);
        else if (path == KMDB_BAND_PATH_TREE) rc = kmdb_all2all_rows_device(db, lo, hi, band, opts);
        else rc = kmdb_all2all_rows_records_device(db, lo, hi, band, opts);
        if (rc) break;
        ++bt.bands;
        if (path == KMDB_BAND_PATH_TILED) {
            const kmdb_all2all_rows_tiled_stats& bs = db->band_stats;
            bt.hits += bs.hits; bt.runs += bs.runs; bt.updates += bs.updates;
            bt.select_ms += bs.select_ms; bt.hits_ms += bs.hits_ms; bt.apply_ms += bs.apply_ms;
        } else if (path == KMDB_BAND_PATH_TREE) {
            bt.updates += db->rows_stats.updates; bt.select_ms += db->rows_stats.select_ms; bt.apply_ms += db->rows_stats.apply_ms;
        } else {
            ++br.bands; br.units_total += db->rr_stats.units_total; br.units_run += db->rr_stats.units_run; br.ms += db->rr_stats.kernel_ms;
        }
        bt.peak_device_bytes = std::max<uint64_t>(bt.peak_device_bytes, db->stats.device_bytes + band.bytes());
        kmdb_sparse_rows part{};
        rc = kmdb_sparse_from_dense_device(db, band, kmdb_tri(lo), kmdb_tri(hi), filters, n_filters, sample_kmers, measure, &part, opts);
        if (rc) break;
        const uint64_t a = part.row_ptr[lo], b = part.row_ptr[hi];
        col.insert(col.end(), part.col + a, part.col + b);
        val.insert(val.end(), part.val + a, part.val + b);
        if (measure >= 0) meas.insert(meas.end(), part.measure + a, part.measure + b);
        for (uint64_t i = lo; i < hi; ++i) row_ptr[i + 1] = row_ptr[i] + (part.row_ptr[i + 1] - part.row_ptr[i]);
        kmdb_sparse_free(&part);
        lo = hi;
    }
    band.reset();
    db->banded_stats = bt;
    if (path == KMDB_BAND_PATH_RECORDS) db->banded_rr_stats = br;
    kmdb_release_staging(db);
    if (rc) return 1;
    const uint64_t nnz = col.size();
    std::memset(out, 0, sizeof *out);
    out->n_rows = N; out->nnz = nnz;
    out->row_ptr = (uint64_t*)std::malloc((N + 1) * sizeof(uint64_t));
    out->col = (uint32_t*)std::malloc(std::max<uint64_t>(nnz, 1) * sizeof(uint32_t));
    out->val = (uint32_t*)std::malloc(std::max<uint64_t>(nnz, 1) * sizeof(uint32_t));
    if (measure >= 0) out->measure = (double*)std::malloc(std::max<uint64_t>(nnz, 1) * sizeof(double));
    if (!out->row_ptr || !out->col || !out->val || (measure >= 0 && !out->measure)) {
        kmdb_sparse_free(out);
        return kmdb_set_error(std::string(who) + ": out of host memory for the result");
    }
    std::memcpy(out->row_ptr, row_ptr.data(), (N + 1) * sizeof(uint64_t));
    if (nnz) {
        std::memcpy(out->col, col.data(), nnz * sizeof(uint32_t));
        std::memcpy(out->val, val.data(), nnz * sizeof(uint32_t));
        if (measure >= 0) std::memcpy(out->measure, meas.data(), nnz * sizeof(double));
    }
    return 0;
}

extern "C" int kmdb_all2all_sparse_filtered_banded(kmdb_db* db, uint64_t band_rows, const kmdb_cell_filter* filters, size_t n_filters, const uint32_t* sample_kmers,
                                                   int measure, kmdb_sparse_rows* out, const kmdb_opts* opts) {
    return banded_run("kmdb_all2all_sparse_filtered_banded", db, band_rows, KMDB_BAND_PATH_TILED, filters, n_filters, sample_kmers, measure, out, opts);
}
extern "C" int kmdb_all2all_sparse_filtered_banded_path(kmdb_db* db, uint64_t band_rows, int path, const kmdb_cell_filter* filters, size_t n_filters,
                                                        const uint32_t* sample_kmers, int measure, kmdb_sparse_rows* out, const kmdb_opts* opts) {
    return banded_run("kmdb_all2all_sparse_filtered_banded_path", db, band_rows, path, filters, n_filters, sample_kmers, measure, out, opts);
}
extern "C" int kmdb_all2all_banded_records_stats_get(const kmdb_db* db, kmdb_all2all_banded_records_stats* out) {
    if (!db || !out) return kmdb_set_error("kmdb_all2all_banded_records_stats_get: null argument");
    *out = db->banded_rr_stats;
    return 0;
}

extern "C" int kmdb_all2all_banded_stats_get(const kmdb_db* db, kmdb_all2all_banded_stats* out) {
    if (!db || !out) return kmdb_set_error("kmdb_all2all_banded_stats_get: null argument");
    *out = db->banded_stats;
    return 0;
}
