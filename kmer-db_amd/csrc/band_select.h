// band_select.h — what the two tree forms of a band call share (a2a_rows.hip, a2a_band.hip): which nodes of the pattern tree can write into the rows
// [row_lo, row_hi), and the node arrays both forms' kernels read.  Templates on the form's parameter struct (RowsParams, BandParams), which holds
// meta, bitpos, parent, sub_end, wprefix, bits, P, row_lo, row_hi, cell_lo, out, sel and counters under these names.
#pragma once
#include "device_common.h"
#include "engine_internal.h"
#include "prim.h"

// A node's local ids lie strictly between its parent's last id and its own last id (inclusive), so: it has one (l > 0), it has a column to pair
// with (n > 1), it carries a weight, its last id is not in front of the band and its first id — behind the last id of the nearest ancestor that has
// one — can be inside it.  A superset: no list is read.
template <class Params>
__device__ __forceinline__ bool band_node_selected(const Params& p, uint32_t i) {
    const uint4 m = p.meta[i];
    const uint32_t W = p.wprefix[p.sub_end[i]] - p.wprefix[i];
    if (!(m.y > 0 && m.x > 1 && W != 0 && m.z >= p.row_lo)) return false;
    int32_t q = p.parent[i];
    while (q >= 0 && p.meta[q].y == 0) q = p.parent[q];            // (a pattern without ids of its own has no last id to go by)
    return q < 0 || (uint64_t)p.meta[q].z + 1 < p.row_hi;
}

// the body of a select kernel: a lane per DFS node, the selected nodes compacted into p.sel (any order) a ballot at a time, counted in p.counters[0]
template <class Params>
__device__ __forceinline__ void band_select_nodes(const Params& p) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t lane = lane_id();
    const bool take = i < p.P && band_node_selected(p, i);
    const unsigned long long bal = __ballot(take);
    if (bal == 0) return;
    uint32_t base = 0;
    if (lane == (uint32_t)__builtin_ctzll(bal)) base = (uint32_t)atomicAdd(&p.counters[0], (unsigned long long)__popcll(bal));
    base = bcast(base, (uint32_t)__builtin_ctzll(bal));
    if (take) p.sel[base + (uint32_t)__popcll(bal & ((1ull << lane) - 1ull))] = i;
}

// (host) the node arrays made, the subtree weights on `st` — differences of the exclusive scan of w in DFS order (reference
// similarity_calculator.cpp:64-72), as before the v1 kernels — and the band and the arrays entered into `p`
template <class Params>
int band_node_params(kmdb_db* db, Params& p, uint32_t* out, uint64_t row_lo, uint64_t row_hi, hipStream_t st) {
    if (kmdb_ensure_v1_arrays(db)) return 1;
    HIP_TRY(prim::exclusive_sum(db->v1_scan_tmp, db->v1_scan_tmp_bytes, db->w.get(), db->wprefix.get(), (int)(db->P + 1), st));
    p.meta = db->meta; p.bitpos = db->bitpos; p.parent = db->parent; p.sub_end = db->sub_end; p.wprefix = db->wprefix; p.bits = db->bits;
    p.P = (uint32_t)db->P; p.row_lo = (uint32_t)row_lo; p.row_hi = (uint32_t)row_hi; p.cell_lo = kmdb_tri(row_lo); p.out = out;
    return 0;
}
