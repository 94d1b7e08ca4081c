// kmdb_internal.h — shared by the translation units of libkmdb_amd.so (not installed).
#pragma once
#include <cstddef>
#include <cstdint>
#include <functional>
#include <string>
#include <utility>
#include <vector>

// records the message for kmdb_last_error() and returns a non-zero status
int kmdb_set_error(const std::string& msg);

// kmdb_db_view.abi_version of a caller this library serves: ABI 8 only ADDED entry points (no struct of ABI 7 changed its size or the order of
// its fields; kmdb_node_stats.reserved, always 0, became `partition`, where 0 is the prefix partition), so a program compiled against the
// header of ABI 7 — a maintainer's glue that has not been rebuilt — keeps working with this library.
constexpr uint32_t KMDB_ABI_OLDEST_COMPATIBLE = 7, KMDB_ABI_THIS = 8;
inline bool kmdb_abi_compatible(uint32_t caller) { return caller >= KMDB_ABI_OLDEST_COMPATIBLE && caller <= KMDB_ABI_THIS; }

// Gives the pages inside the regions back to the kernel, on up to `threads` threads (host_db.cpp).  madvise(MADV_DONTNEED) takes the
// address-space lock SHARED: the threads, and the page faults and allocations of every other thread, go on side by side, where a munmap
// of gigabytes holds the lock exclusively for as long as it frees pages.  The regions stay mapped (they read as zeros afterwards):
// unmapping them later, or the end of the process, finds nothing left to free.
void kmdb_drop_pages(const std::vector<std::pair<void*, size_t>>& regions, unsigned threads);

// ---- host_db.cpp: a kmdbh_db made in memory instead of parsed from a file (build.hip: the result of kmdb_build_finish).  The arrays are
// allocated at their final sizes (data: n_data_words + 2, the loader's padding pair, zeroed here) and handed out for the caller to fill;
// the view is complete on return.  nullptr with the error set when the host is out of memory.
struct kmdbh_db;
struct kmdbh_db_arrays {
    int64_t *num_kmers, *parent_id;
    uint32_t *num_samples, *num_local, *last_sample_id, *num_bits;
    uint64_t *data_offset, *data, *bucket_offset, *slots;
};
kmdbh_db* kmdbh_db_make(uint32_t kmer_length, double fraction, double start_fraction, int32_t alphabet, uint64_t kmers_count,
                        std::vector<std::string>&& names, std::vector<uint64_t>&& sample_kmers, uint64_t n_patterns, uint64_t n_data_words,
                        uint64_t n_buckets, uint64_t n_slots, kmdbh_db_arrays* arrays);

// ---- the hand-off of a finished builder to the engine (kmdb_build_finish_device, build.hip -> engine.hip -> layout.hip): the database as
// the builder holds it in HBM at the end of its finish stages (c) and (d).  Every pointer is device memory of the handle's device, every
// array in pattern-id order; the streams are word-aligned (pattern p from word data_offset[p] on, MSB first, zero behind num_bits).
// The callbacks (any may be empty) tell the builder that the last reader of a group of its arrays has run, so that it can release them:
// the tables once they are copied, the tree and the stage (c) fields once the node arrays exist, the stream words once they are re-packed.
struct kmdb_db;
struct kmdb_layout_device_source {
    uint64_t n_patterns = 0, n_samples = 0;
    uint32_t kmer_length = 0;
    const long long* num_kmers = nullptr;            // the builder's tree
    const long long* parent_id = nullptr;
    const uint32_t* num_samples = nullptr;
    const uint32_t* num_local = nullptr;             // stage (c)
    const uint32_t* last_sample_id = nullptr;
    const uint32_t* num_bits = nullptr;
    const unsigned long long* data_offset = nullptr;
    const uint64_t* data = nullptr;
    uint64_t n_data_words = 0;
    uint64_t n_buckets = 0, n_slots = 0;             // stage (d); 0 buckets: no tables were made
    const uint64_t* bucket_offset = nullptr;
    const uint64_t* slots = nullptr;
    std::function<void()> tables_done, fields_done, streams_done;
    mutable double fields_ms = 0;                    // out: wall clock of the fields kernel and the table copies
    double layout_ms = 0, prepare_ms = 0;            // out: wall clock of the whole layout (fields included) and of kmdb_blocks_prepare
};
// layout.hip: fills the handle's structural arrays and stats from the source (the device stage kmdb_db_upload ends in); 0, or 1 with the error set
int kmdb_layout_from_device(kmdb_db* db, const kmdb_layout_device_source* src, int with_hashtables);
// engine.hip: the handle kmdb_db_upload would return for the same database, made from the source; opts as for kmdb_db_upload
struct kmdb_opts;
int kmdb_db_from_device(kmdb_layout_device_source* src, const kmdb_opts* opts, int with_hashtables, kmdb_db** out);
// layout.hip (tests; not part of include/kmdb_amd.h): the short decode launch's work order read back — the window, the number of windows, every
// window's node offsets by decreasing key (n_windows * window of them), its live count, and the list heads (l, stream bits) of the P nodes in DFS
// order.  Every output may be null: a first call with the two sizes alone tells how much the others hold.
extern "C" int kmdb_debug_k0_order(const kmdb_db* db, uint32_t* window, uint64_t* n_windows, uint16_t* order, uint32_t* live, uint32_t* l, uint32_t* num_bits);

// ---- minhash.hip: the extractor behind kmdb_minhash_batch_seq_alphabet with the lists LEFT ON THE DEVICE (build.hip adds them to its
// tree from there).  The batch is cut into pieces as for the public entry; for every piece `sink` is called once, after the piece's last
// kernel has ended: d_kmers = the sorted unique words of the piece's n samples, sample s at [off[s], off[s + 1]) (off in host memory,
// off[0] = 0); the device buffer is released when the sink returns.  A non-zero return of the sink ends the call with that status.
using kmdb_device_lists_sink = std::function<int(const uint64_t* d_kmers, const uint64_t* off, size_t n, void* stream)>;
struct kmdb_opts;
int kmdb_minhash_device_lists(const char* who, const char* const* seqs, const size_t* seq_lens, size_t n_samples, uint32_t kmer_length, double fraction,
                              double start_fraction, int32_t alphabet, const kmdb_opts* opts, const kmdb_device_lists_sink& sink);

// ---- sorted_union.hip: what kmdb_sorted_union_device does once its arguments are checked and the device is set — out (room for na + nb words)
// = a ∪ b, *n_out its length; returns after the last kernel has ended.  *scratch_bytes (may be null): device bytes of the call's own tables.
int kmdb_sorted_union_on_stream(const char* who, const uint64_t* a, uint64_t na, const uint64_t* b, uint64_t nb, uint64_t* out, uint64_t* n_out, void* stream,
                                uint64_t* scratch_bytes);

// ---- host_shards.cpp: the prefix shards of one database, planned on the host in ONE pass over its hashtables and ONE sweep over its
// tree, for all shards at once (bucket = kmer >> 32, reference src/types.h:25-27; items src/hashmap_lp.h:71-78).
// Shard s owns the k-mers of the buckets b with b % n_shards == s.  w[s][p] = k-mers of pattern p in shard s; a node is kept by shard s
// when its subtree holds a k-mer of s (bit s & 7 of mask[s >> 3][p]).  Every device then receives only the nodes and streams its
// shards keep — not the whole tree and the hashtables once per device.
struct kmdb_db_view;
// prefix shards per database at most (the plan keeps a counter array per shard; a count beyond this is a caller's mistake, not a configuration)
constexpr uint32_t KMDB_MAX_SHARDS = 4096;
struct kmdb_shard_plan {
    uint64_t P = 0;
    uint32_t n_shards = 0;
    std::vector<uint32_t*> w;                  // [n_shards] -> [P]; nullptr for a shard that was not asked for (or was released)
    std::vector<unsigned char*> mask;          // [(n_shards + 7) / 8] -> [P]
    std::vector<uint64_t> kept;                // [n_shards] nodes the shard keeps
    kmdb_shard_plan() = default;
    kmdb_shard_plan(const kmdb_shard_plan&) = delete;
    kmdb_shard_plan& operator=(const kmdb_shard_plan&) = delete;
    ~kmdb_shard_plan();
    void release_weights(uint32_t shard);      // the shard has been uploaded: its P counters go back
    bool keeps(uint32_t shard, uint64_t p) const { return (mask[shard >> 3][p] >> (shard & 7u)) & 1u; }
};
// plans the listed shards (all of them: kmdb_node_upload; one: kmdb_db_upload_shard); 0, or 1 with the error set
int kmdb_shard_plan_build(const kmdb_db_view* v, uint32_t n_shards, const std::vector<uint32_t>& shards, kmdb_shard_plan* plan);

// the own bucket table of query shard `shard` of n_shards: its buckets (b % n_shards == shard, local index b / n_shards) and their slots
void kmdb_query_shard_tables(const kmdb_db_view* v, uint32_t shard, uint32_t n_shards, uint64_t* n_buckets, uint64_t* n_slots);

// The buckets of a sorted query (KmerHelper::unique; bucket = kmer >> 32, types.h:25-27): fn(bucket, begin, end) for every maximal stretch
// [begin, end) of k-mers of one bucket, ascending.  What kmdbh_query_shard_runs and the node driver's split of k-mer queries are made of.
template <class F>
inline void kmdb_for_bucket_runs(const uint64_t* kmers, size_t count, F&& fn) {
    for (size_t i = 0; i < count;) {
        const uint64_t b = kmers[i] >> 32;
        size_t e = i + 1;
        while (e < count && (kmers[e] >> 32) == b) ++e;
        fn(b, i, e);
        i = e;
    }
}

// ---- host_ranges.cpp: the tree ranges of one database (the pattern / subtree is the natural all2all unit), planned from
// parent_id and num_samples alone — no hashtables.  The DFS pre-order of the device layout (children of a node and the roots in ascending
// pattern id: layout.hip) is cut into n_ranges contiguous stretches of about equal estimated cost; range s = positions [cut[s], cut[s + 1]).
// A range also lays out the ancestors of its FIRST node that lie before it, with weight 0 (they only supply sample ids): a subtree is a
// contiguous stretch of the pre-order, so every out-of-range ancestor of any node of the range is one of those.
//   kept(s) = own(s) + depth(first node of s) - 1,   depth of a root = 1
// The plan is a pure function of (view, n_ranges): processes that each upload "range s of R" agree without talking to each other.
// It holds one 4-byte position per pattern and R short ancestor lists — no per-shard array.
struct kmdb_range_plan {
    uint64_t P = 0;
    uint32_t n_ranges = 0;
    std::vector<uint32_t> pre;                 // [P] pre-order position of every pattern
    std::vector<uint32_t> cut;                 // [n_ranges + 1] ascending, cut[0] = 0, cut[n_ranges] = P
    std::vector<std::vector<uint32_t>> anc;    // [n_ranges] pattern ids of the out-of-range ancestors of the range's first node, root first (ascending)
    std::vector<uint64_t> cost;                // [n_ranges] estimated cost of the range's own nodes
    uint64_t own(uint32_t s) const { return cut[s + 1] - cut[s]; }
    uint64_t kept(uint32_t s) const { return own(s) + anc[s].size(); }
    uint32_t first_depth(uint32_t s) const { return own(s) ? (uint32_t)anc[s].size() + 1u : 0u; }
};
// 0, or 1 with the error set
int kmdb_range_plan_build(const kmdb_db_view* v, uint32_t n_ranges, kmdb_range_plan* plan);

// ---- which nodes an upload lays out and with which weight: what the pruned branch of kmdb_layout_upload (layout.hip) asks of a plan.
// Both partitions answer through it: a prefix shard keeps the nodes whose subtree holds one of its k-mers, at its own k-mer counts; a
// tree range keeps its own nodes at their on-disk num_kmers and the out-of-range ancestors of its first node at 0.
struct kmdb_kept_nodes {
    const char* what = "";                     // "prefix shard" / "tree range" (messages)
    uint64_t kept = 0;                         // nodes to lay out
    // prefix shard
    const unsigned char* mask = nullptr;       // kmdb_shard_plan::mask[shard >> 3]
    unsigned char bit = 0;
    const uint32_t* w = nullptr;               // kmdb_shard_plan::w[shard]
    // tree range
    const uint32_t* pre = nullptr;             // kmdb_range_plan::pre
    uint32_t lo = 0, hi = 0;                   // own nodes: lo <= pre[p] < hi
    const uint32_t* anc = nullptr;             // ascending pattern ids of the zero-weight nodes (all of them before `lo` in the pre-order,
    uint32_t n_anc = 0;                        // or pattern 0 alone for an empty range: every array stays non-empty)
    // query shard (kmdb_db_upload_query_shard): a prefix shard that also carries the slots of its own buckets, qs_count > 0
    uint32_t qs_index = 0, qs_count = 0;

    bool owns(uint64_t p) const { return pre[p] - lo < hi - lo; }
    bool keeps(uint64_t p) const {
        if (mask) return (mask[p] & bit) != 0;
        if (owns(p)) return true;
        uint32_t a = 0, b = n_anc;             // (a handful of entries: the depth of the range's first node)
        while (a < b) { const uint32_t m = (a + b) / 2; if (anc[m] < p) a = m + 1; else b = m; }
        return a < n_anc && anc[a] == p;
    }
    // truncated exactly like the reference's to_add (similarity_calculator.cpp:222)
    uint32_t weight(uint64_t p, const int64_t* num_kmers) const { return mask ? w[p] : (owns(p) ? (uint32_t)num_kmers[p] : 0u); }
};
kmdb_kept_nodes kmdb_kept_of_shard(const kmdb_shard_plan& plan, uint32_t shard);
kmdb_kept_nodes kmdb_kept_of_range(const kmdb_range_plan& plan, uint32_t range);
