// host_ranges.cpp — the tree ranges of a database (kmdb_internal.h: kmdb_range_plan), on the host, before anything goes to a device.
//
// all2all computes cell (i, j) = sum over the patterns p of w_p [i, j in S_p] (S_p: the ids of p and its ancestors, w_p: the on-disk
// num_kmers), every pattern on its own.  So ANY partition of the patterns gives partial matrices that sum (uint32, wrap-around) to the
// whole matrix, as long as a part also holds the ancestors of its patterns at weight 0.  Contiguous ranges of the DFS pre-order keep
// that replication minimal: a subtree is a contiguous stretch of the pre-order, so an ancestor of a node of the range that lies outside
// the range lies before it and contains the range's first node — kept = own + depth(first) - 1.
// The reference loads all2all with SkipHashtables (src/console_all2all.cpp:26); nothing here reads a hashtable.
#include "kmdb_amd.h"
#include "kmdb_internal.h"

#include <algorithm>
#include <climits>
#include <new>
#include <stdexcept>

namespace {

// Cost proxy of a node (the real block count needs decoded ids, which the host does not have): a constant for the decode and the walk,
// plus the block-record pairs of a list that spreads evenly: c (c + 1) / 2 with c = min(ceil(n / w) + 1, ceil(N / w)) blocks at a nominal
// block width w (the engine picks 32 ... 64 per handle later).
constexpr uint64_t RANGE_NODE_COST = 4, RANGE_BLOCK_WIDTH = 64;
inline uint64_t node_cost(uint64_t n, uint64_t N) {
    const uint64_t c = std::min((n + RANGE_BLOCK_WIDTH - 1) / RANGE_BLOCK_WIDTH + 1, (N + RANGE_BLOCK_WIDTH - 1) / RANGE_BLOCK_WIDTH);
    return RANGE_NODE_COST + c * (c + 1) / 2;
}

int range_plan_build_impl(const kmdb_db_view* v, uint32_t R, kmdb_range_plan* plan) {
    const uint64_t P = v->n_patterns, N = v->n_samples;
    if (P >= (1ull << 31)) return kmdb_set_error("kmdb_db_upload: more than 2^31 patterns");
    if (P && (!v->parent_id || !v->num_samples)) return kmdb_set_error("kmdb_range_plan: the view lacks parent_id / num_samples");
    plan->P = P; plan->n_ranges = R;
    plan->pre.assign(P, 0);
    plan->cut.assign((size_t)R + 1, 0);
    plan->anc.assign(R, {});
    plan->cost.assign(R, 0);
    // Two sweeps over the tree (parent_id[p] < p), nothing else walks it: children before parents for the subtree sizes and the subtree
    // costs; parents before children for a node's position and for the cost of everything before it in the pre-order — a parent's own,
    // plus the parent's and the earlier siblings' subtrees (the children of a node, and the roots, in ascending pattern id).  The cost
    // before a node grows strictly along the pre-order, so the range of a node follows from it alone: range s starts at the first
    // position whose cost prefix reaches s / R of the total.
    std::vector<uint32_t> next(P, 1);                          // subtree sizes, then a node's next free position
    std::vector<uint64_t> cnext(P);                            // subtree costs, then the cost before a node's next free position
    for (uint64_t p = 0; p < P; ++p) cnext[p] = node_cost(v->num_samples[p], N);
    for (uint64_t p = P; p-- > 0;) {
        const int64_t par = v->parent_id[p];
        if (par < 0) continue;
        if ((uint64_t)par >= p) return kmdb_set_error("kmdb_db_upload: parent_id >= pattern id");
        next[par] += next[p];
        cnext[par] += cnext[p];
    }
    uint64_t total = 0;
    for (uint64_t p = 0; p < P; ++p) if (v->parent_id[p] < 0) total += cnext[p];
    std::vector<uint64_t> start(R - 1);                        // range s >= 1 starts where the cost before a node reaches ceil(total * s / R)
    for (uint32_t s = 1; s < R; ++s) start[s - 1] = (uint64_t)(((unsigned __int128)total * s + R - 1) / R);
    uint32_t* pre = plan->pre.data();
    uint32_t next_root = 0;
    uint64_t cnext_root = 0;
    std::vector<uint32_t> first(R, 0), first_pre(R, UINT32_MAX), own(R, 0);
    for (uint64_t p = 0; p < P; ++p) {
        const int64_t par = v->parent_id[p];
        uint32_t& slot = par < 0 ? next_root : next[par];
        uint64_t& cslot = par < 0 ? cnext_root : cnext[par];
        const uint32_t pos = slot;
        const uint64_t before = cslot, own_cost = node_cost(v->num_samples[p], N);
        slot += next[p];
        cslot += cnext[p];
        pre[p] = pos;
        next[p] = pos + 1;
        cnext[p] = before + own_cost;
        const uint32_t r = (uint32_t)(std::upper_bound(start.begin(), start.end(), before) - start.begin());      // the ranges that start at or before this node
        ++own[r];
        plan->cost[r] += own_cost;
        if (pos < first_pre[r]) { first_pre[r] = pos; first[r] = (uint32_t)p; }
    }
    for (uint32_t s = 0; s < R; ++s) plan->cut[s + 1] = plan->cut[s] + own[s];
    for (uint32_t s = 0; s < R; ++s) {
        if (!own[s]) continue;
        if (first_pre[s] != plan->cut[s]) return kmdb_set_error("kmdb_range_plan: internal: a range is not a stretch of the pre-order");
        // the root path of the first node, all of it before the range
        std::vector<uint32_t>& a = plan->anc[s];
        for (int64_t q = v->parent_id[first[s]]; q >= 0; q = v->parent_id[q]) a.push_back((uint32_t)q);
        std::reverse(a.begin(), a.end());
    }
    return 0;
}

}  // namespace

int kmdb_range_plan_build(const kmdb_db_view* v, uint32_t n_ranges, kmdb_range_plan* plan) {
    if (n_ranges == 0 || n_ranges > KMDB_MAX_SHARDS) return kmdb_set_error("kmdb_db_upload_range: range_count must be between 1 and " + std::to_string(KMDB_MAX_SHARDS));
    try {
        return range_plan_build_impl(v, n_ranges, plan);
    } catch (const std::bad_alloc&) {
        return kmdb_set_error("kmdb_db_upload_range: out of host memory for the range plan");
    } catch (const std::exception& e) {
        return kmdb_set_error(std::string("kmdb_db_upload_range: ") + e.what());
    }
}

kmdb_kept_nodes kmdb_kept_of_shard(const kmdb_shard_plan& plan, uint32_t shard) {
    kmdb_kept_nodes k;
    k.what = "prefix shard";
    k.kept = plan.kept[shard];
    k.mask = plan.mask[shard >> 3];
    k.bit = (unsigned char)(1u << (shard & 7u));
    k.w = plan.w[shard];
    return k;
}

kmdb_kept_nodes kmdb_kept_of_range(const kmdb_range_plan& plan, uint32_t range) {
    static const uint32_t pattern0 = 0;
    kmdb_kept_nodes k;
    k.what = "tree range";
    k.pre = plan.pre.data();
    k.lo = plan.cut[range]; k.hi = plan.cut[range + 1];
    if (k.lo == k.hi && plan.P) { k.anc = &pattern0; k.n_anc = 1; k.kept = 1; }      // an empty range: pattern 0 (a root) at weight 0, a zero matrix
    else { k.anc = plan.anc[range].data(); k.n_anc = (uint32_t)plan.anc[range].size(); k.kept = plan.kept(range); }
    return k;
}

extern "C" int kmdbh_range_plan(const kmdb_db_view* view, uint32_t n_ranges, uint64_t* kept_nodes, uint64_t* own_nodes, uint64_t* est_cost,
                                uint32_t* range_of, uint32_t* first_depth) {
    if (!view || !kept_nodes || !own_nodes || !est_cost) return kmdb_set_error("kmdbh_range_plan: null argument");
    if (!kmdb_abi_compatible(view->abi_version)) return kmdb_set_error("kmdbh_range_plan: bad view / ABI version");
    if (n_ranges == 0) return kmdb_set_error("kmdbh_range_plan: no ranges");
    if (n_ranges > KMDB_MAX_SHARDS) return kmdb_set_error("kmdbh_range_plan: more than " + std::to_string(KMDB_MAX_SHARDS) + " ranges");
    kmdb_range_plan plan;
    if (kmdb_range_plan_build(view, n_ranges, &plan)) return 1;
    for (uint32_t s = 0; s < n_ranges; ++s) {
        kept_nodes[s] = plan.kept(s); own_nodes[s] = plan.own(s); est_cost[s] = plan.cost[s];
        if (first_depth) first_depth[s] = plan.first_depth(s);
    }
    if (range_of)
        for (uint64_t p = 0; p < plan.P; ++p)      // the one range with cut[s] <= position < cut[s + 1] (empty ranges never match)
            range_of[p] = (uint32_t)(std::upper_bound(plan.cut.begin(), plan.cut.end(), plan.pre[p]) - plan.cut.begin()) - 1u;
    return 0;
}

// ---- the geometry of a band of rows in the block-record pipeline's streams (kmdb_amd.h: kmdb_band_geometry; a2a_rows_records.hip calls this very function).
// Block (X, Y), Y <= X, of `width` sample ids a side is stream tri32(X) + Y, tri32(x) = x (x + 1) / 2; the band [row_lo, row_hi) owns the streams of the
// block rows row_lo / width .. (row_hi - 1) / width, keyed from the first of them on.
extern "C" int kmdbh_band_streams(uint64_t n_samples, uint32_t width, uint64_t row_lo, uint64_t row_hi, kmdb_band_geometry* out) {
    const char* who = "kmdbh_band_streams";
    if (!out) return kmdb_set_error(std::string(who) + ": null argument");
    if (width < 32 || width > 64) return kmdb_set_error(std::string(who) + ": a block width of " + std::to_string(width) + " lies outside 32 .. 64");
    if (row_lo > row_hi) return kmdb_set_error(std::string(who) + ": row_lo > row_hi (" + std::to_string(row_lo) + " > " + std::to_string(row_hi) + ")");
    if (row_hi > n_samples) return kmdb_set_error(std::string(who) + ": row_hi " + std::to_string(row_hi) + " > the " + std::to_string(n_samples) + " samples");
    *out = kmdb_band_geometry{};
    out->fits = 1;
    if (row_lo == row_hi) return 0;                              // an empty band owns nothing
    const uint64_t x_lo = row_lo / width, x_hi = (row_hi - 1) / width;
    if (x_hi >= (1ull << 31)) return kmdb_set_error(std::string(who) + ": more than 2^31 block rows");
    auto tri = [](uint64_t x) { return x * (x + 1) / 2; };
    out->x_lo = (uint32_t)x_lo; out->x_hi = (uint32_t)x_hi; out->n_rows = (uint32_t)(x_hi - x_lo + 1);
    out->n_streams = tri(x_hi + 1) - tri(x_lo);
    out->stream_base = tri(x_lo);
    out->fits = out->n_streams + 1 < (1ull << 22) ? 1u : 0u;
    return 0;
}
