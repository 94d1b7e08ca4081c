// layout.hip — kmdb_db_upload: the on-disk pattern section (pid order, parent links) becomes the HBM layout of the
// engine (DFS pre-order, bit-packed streams).  A pure format conversion: nothing here decodes a sample id.
//
//   host   (threads)  narrow the header fields, validate them, pack the 128-bit padded gamma streams back to back
//                     in pid order (reference layout: src/pattern.cpp:15-46, streams src/elias_gamma.h:113-125)
//   device            subtree sizes (leaf climb with child counters), children grouped by parent (stable radix sort:
//                     pid order inside a family), pre-order offsets among siblings (scan), pre-order index / depth of
//                     every node by pointer doubling along the parent links, then one gather into DFS order and a
//                     bit-exact re-pack of the streams
// parent_id[p] < p (patterns are appended, reference src/prefix_kmer_db.cpp:219,357); children keep pid order.
// The device half (lay_device_stage) has a second source: kmdb_layout_from_device hands it a finished builder's arrays where they lie in
// HBM (kmdb_build_finish_device, build.hip) — lay_fields_kernel does what the host's narrowing loop does, and nothing visits the host.
#include "device_common.h"
#include "engine_internal.h"

#include "prim.h"

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <sys/mman.h>
#include <thread>

namespace {

struct U32toU64 { __host__ __device__ uint64_t operator()(uint32_t v) const { return v; } };

// children of every node = one run of the parent-sorted child list: first position and length per parent key
// (key = parent + 1, key 0 = the roots); no atomics (a hot parent has 10^5 children, and same-address atomics crawl)
__global__ void lay_child_runs_kernel(const uint32_t* __restrict__ skeys, uint32_t P, uint32_t* __restrict__ start, uint32_t* __restrict__ cnt) {
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= P) return;
    const uint32_t k = skeys[j];
    if (j == 0 || skeys[j - 1] != k) start[k] = j;
    if (j + 1 == P || skeys[j + 1] != k) cnt[k] = j + 1;          // run end for now; turned into a length below
}
__global__ void lay_child_len_kernel(const uint32_t* __restrict__ start, uint32_t n_keys, uint32_t* __restrict__ cnt) {
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k < n_keys && cnt[k]) cnt[k] -= start[k];
}
// subtree sizes, one tree level per launch, deepest first: size = 1 + sizes of the children (already final)
__global__ void lay_sizes_level_kernel(const uint32_t* __restrict__ dep, uint32_t level, const uint32_t* __restrict__ start, const uint32_t* __restrict__ cnt,
                                       const uint32_t* __restrict__ schild, uint32_t P, uint32_t* __restrict__ size) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= P || dep[i] != level) return;
    const uint32_t c = cnt[i + 1], s0 = start[i + 1];
    uint32_t sz = 1;
    for (uint32_t j = 0; j < c; ++j) sz += size[schild[s0 + j]];
    size[i] = sz;
}

__global__ void lay_keys_kernel(const int32_t* __restrict__ parent, uint32_t P, uint32_t* __restrict__ keys, uint32_t* __restrict__ vals) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < P) { keys[i] = (uint32_t)(parent[i] + 1); vals[i] = i; }
}
__global__ void lay_fill_kernel(uint32_t* __restrict__ dst, uint32_t n, uint32_t val) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) dst[i] = val;
}
__global__ void lay_pid2dfs_kernel(const uint32_t* __restrict__ acc, uint32_t n, uint32_t* __restrict__ out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = acc[i] - 1u;
}
// query shard: the values of its own slots, kept index -> DFS index, in place (the host wrote the kept index while it packed the shard's
// buckets; acc[i] - 1 = pre-order position of kept node i).  One slot per thread and step, the wave reads 512 contiguous bytes; only the value
// word is written back.  The empty marker stays; the host has checked every other value against the kept count.
__global__ __launch_bounds__(256) void lay_slots_to_dfs_kernel(uint64_t* __restrict__ slots, uint64_t n_slots, const uint32_t* __restrict__ acc, uint32_t P) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; j < n_slots; j += stride) {
        const uint32_t val = (uint32_t)(slots[j] >> 32);
        if (val != 0x7fffffffu && val < P) ((uint32_t*)(slots + j))[1] = acc[val] - 1u;
    }
}
__global__ void lay_gather_u32_kernel(const uint32_t* __restrict__ src, const uint32_t* __restrict__ idx, uint32_t n, uint32_t* __restrict__ dst) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) dst[i] = src[idx[i]];
}
// offset of a child inside its parent's subtree: 1 + sizes of the earlier siblings
__global__ void lay_rel_kernel(const uint32_t* __restrict__ sorted_keys, const uint32_t* __restrict__ sorted_child, const uint32_t* __restrict__ S,
                               const uint32_t* __restrict__ child_begin, uint32_t P, uint32_t* __restrict__ acc) {
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= P) return;
    acc[sorted_child[j]] = 1u + S[j] - S[child_begin[sorted_keys[j]]];
}
// one round of pointer doubling: the sum of `val` along the path to the current ancestor pointer
__global__ void lay_jump_kernel(const uint32_t* __restrict__ val_in, const int32_t* __restrict__ anc_in, uint32_t P,
                                uint32_t* __restrict__ val_out, int32_t* __restrict__ anc_out, uint32_t* __restrict__ active) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= P) return;
    const int32_t a = anc_in[i];
    uint32_t v = val_in[i];
    int32_t na = -1;
    if (a >= 0) {
        v += val_in[a]; na = anc_in[a];
        if (na >= 0) *active = 1u;
    }
    val_out[i] = v; anc_out[i] = na;
}
__global__ void lay_order_kernel(const uint32_t* __restrict__ acc, uint32_t P, uint32_t* __restrict__ order, uint32_t* __restrict__ bad) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= P) return;
    const uint32_t pre = acc[i] - 1u;                       // the virtual root sits at -1
    if (pre >= P) { *bad = 1u; return; }
    order[pre] = i;
}
struct LayStats { unsigned long long alg, upd, pairs; uint32_t max_n, max_depth, bad, n_long; };
__global__ void lay_gather_kernel(const uint32_t* __restrict__ order, const uint32_t* __restrict__ acc, const uint32_t* __restrict__ dep,
                                  const uint32_t* __restrict__ cnt, const uint32_t* __restrict__ size, const int32_t* __restrict__ parent,
                                  const uint32_t* __restrict__ h_l, const uint32_t* __restrict__ h_last, const uint32_t* __restrict__ h_n, const uint32_t* __restrict__ h_nbits,
                                  const uint32_t* __restrict__ h_w, const unsigned long long* __restrict__ h_wfull, uint32_t P, uint32_t short_ids,
                                  uint2* __restrict__ k0in, uint32_t* __restrict__ nl, int32_t* __restrict__ dparent, uint32_t* __restrict__ w,
                                  uint16_t* __restrict__ dflag, uint32_t* __restrict__ sub_end, LayStats* __restrict__ st) {
    unsigned long long alg = 0, upd = 0, pairs = 0;
    uint32_t mn = 0, md = 0, nlong = 0;
    // grid-stride: the statistics end in one atomic per block and counter, so the grid stays small
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i <= P; i += gridDim.x * blockDim.x) {
        if (i == P) { w[P] = 0; break; }
        const uint32_t pid = order[i];
        const uint32_t l = h_l[pid], n = h_n[pid], nb = h_nbits[pid];
        k0in[i] = kmdb_k0_pack(l, h_last[pid], nb);
        nl[i] = n;
        const int32_t par = parent[pid];
        dparent[i] = par < 0 ? -1 : (int32_t)(acc[par] - 1u);
        w[i] = h_w[pid];
        const uint32_t d = dep[pid];
        dflag[i] = (uint16_t)((d > 0x7FFFu ? 0x7FFFu : d) | (cnt[pid + 1] ? 0x8000u : 0u));
        sub_end[i] = i + size[pid];
        alg += 40ull + (unsigned long long)((nb + 127u) / 128u) * 16ull;
        upd += (unsigned long long)(n - l) * l + (unsigned long long)l * (l ? l - 1 : 0) / 2;
        pairs += (h_wfull ? h_wfull[pid] : (unsigned long long)h_w[pid]) * ((unsigned long long)n * (n ? n - 1 : 0) / 2);
        mn = max(mn, n); md = max(md, d); nlong += kmdb_long_node(l, nb, short_ids) ? 1u : 0u;
    }
    // block reduction of the statistics
    __shared__ unsigned long long s_alg[256], s_upd[256], s_pairs[256];
    __shared__ uint32_t s_mn[256], s_md[256], s_nl[256];
    s_alg[threadIdx.x] = alg; s_upd[threadIdx.x] = upd; s_pairs[threadIdx.x] = pairs; s_mn[threadIdx.x] = mn; s_md[threadIdx.x] = md; s_nl[threadIdx.x] = nlong;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) {
            s_alg[threadIdx.x] += s_alg[threadIdx.x + s]; s_upd[threadIdx.x] += s_upd[threadIdx.x + s]; s_pairs[threadIdx.x] += s_pairs[threadIdx.x + s];
            s_mn[threadIdx.x] = max(s_mn[threadIdx.x], s_mn[threadIdx.x + s]); s_md[threadIdx.x] = max(s_md[threadIdx.x], s_md[threadIdx.x + s]);
            s_nl[threadIdx.x] += s_nl[threadIdx.x + s];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        atomicAdd(&st->alg, s_alg[0]); atomicAdd(&st->upd, s_upd[0]); atomicAdd(&st->pairs, s_pairs[0]);
        atomicMax(&st->max_n, s_mn[0]); atomicMax(&st->max_depth, s_md[0]); atomicAdd(&st->n_long, s_nl[0]);
    }
}
__global__ void lay_nbits_dfs_kernel(const uint2* __restrict__ k0in, uint32_t P, uint32_t* __restrict__ nb) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < P) nb[i] = kmdb_k0_bits(k0in[i]);
}
__global__ void lay_blkbase_kernel(const uint64_t* __restrict__ dstpos, uint32_t P, uint64_t* __restrict__ blkbase, uint32_t* __restrict__ bitrel) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= P) return;
    const uint64_t b = dstpos[i & ~255u];
    if ((i & 255u) == 0) blkbase[i >> 8] = b;
    bitrel[i] = (uint32_t)(dstpos[i] - b);
}
// re-pack: the stream of DFS node i moves from its pid-order position to its DFS-order position (both bit-granular,
// MSB-first inside little-endian uint64 words)
__global__ void lay_copy_bits_kernel(const uint32_t* __restrict__ order, const uint64_t* __restrict__ srcpos, const uint64_t* __restrict__ dstpos,
                                     const uint2* __restrict__ k0in, const uint64_t* __restrict__ src, uint32_t P, unsigned long long* __restrict__ dst) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= P) return;
    const uint32_t nb = kmdb_k0_bits(k0in[i]);
    if (!nb) return;
    uint64_t sp = srcpos[order[i]], dp = dstpos[i];
    for (uint32_t done = 0; done < nb; done += 64) {
        const uint32_t take = nb - done < 64u ? nb - done : 64u;
        const uint32_t ss = (uint32_t)(sp & 63u);
        uint64_t chunk = src[sp >> 6] << ss;
        if (ss && take > 64u - ss) chunk |= src[(sp >> 6) + 1] >> (64u - ss);
        if (take < 64u) chunk &= ~0ull << (64u - take);
        const uint32_t ds = (uint32_t)(dp & 63u);
        atomicOr(&dst[dp >> 6], (unsigned long long)(chunk >> ds));
        if (ds && take > 64u - ds) atomicOr(&dst[(dp >> 6) + 1], (unsigned long long)(chunk << (64u - ds)));
        sp += take; dp += take;
    }
}
// long nodes: selected in DFS order (stable partition), then ordered by work
struct LongNodePred {
    const uint2* k0in;
    uint32_t short_ids;
    __host__ __device__ bool operator()(uint32_t i) const { const uint2 km = k0in[i]; return kmdb_long_node(kmdb_k0_l(km), kmdb_k0_bits(km), short_ids); }
};
__global__ void lay_long_keys_kernel(const uint2* __restrict__ k0in, const uint32_t* __restrict__ idx, uint32_t n, uint32_t* __restrict__ keys) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n) return;
    const uint2 km = k0in[idx[t]];
    const uint32_t l = kmdb_k0_l(km);
    keys[t] = kmdb_k0_bits(km) - (l ? l - 1u : 0u);                     // work of a node ~ stream bits beyond one per delta
}
// The short decode launch's work order: one workgroup per window of W consecutive DFS nodes sorts them by decreasing kmdb_k0_key (counting sort in LDS
// over the 64 keys) and writes every node's offset inside the window at its rank, and the number of nodes with a key above 0.  The slots of the last
// window behind node P - 1 count as key 0.  Reads the heads of the lists alone.
__global__ __launch_bounds__(256) void lay_k0_order_kernel(const uint2* __restrict__ k0in, uint32_t P, uint32_t W, uint32_t short_ids, uint16_t* __restrict__ order,
                                                           uint32_t* __restrict__ live) {
    __shared__ uint32_t bins[64];
    const uint64_t base = (uint64_t)blockIdx.x * W;
    auto key_of = [&](uint32_t r) -> uint32_t {
        if (base + r >= P) return 0u;
        const uint2 km = k0in[base + r];
        return kmdb_k0_key(kmdb_k0_l(km), kmdb_k0_bits(km), short_ids);
    };
    if (threadIdx.x < 64) bins[threadIdx.x] = 0;
    __syncthreads();
    for (uint32_t r = threadIdx.x; r < W; r += 256) atomicAdd(&bins[63u - key_of(r)], 1u);          // bin 0 = most work
    __syncthreads();
    if (threadIdx.x < 64) {
        const uint32_t c = bins[threadIdx.x];
        const uint32_t first = wave_incl_scan(c, threadIdx.x) - c;
        bins[threadIdx.x] = first;
        if (threadIdx.x == 63) live[blockIdx.x] = first;                                            // (bin 63 = key 0 starts where the live nodes end)
    }
    __syncthreads();
    for (uint32_t r = threadIdx.x; r < W; r += 256) order[base + atomicAdd(&bins[63u - key_of(r)], 1u)] = (uint16_t)r;
}
// root path of the first node of every slice, root first
__global__ void lay_seg_anc_kernel(const int32_t* __restrict__ parent, const uint16_t* __restrict__ dflag, uint32_t P, uint32_t nseg_nodes, uint32_t n_segs,
                                   uint32_t chain_cap, uint32_t* __restrict__ anc, uint32_t* __restrict__ anc_n) {
    const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= n_segs) return;
    int32_t cur = parent[(size_t)s * nseg_nodes];
    uint32_t d = cur < 0 ? 0u : (uint32_t)(dflag[cur] & 0x7FFFu);
    if (d > chain_cap) d = 0;                                  // deeper than the chain table: the pipeline is not used
    anc_n[s] = d;
    while (cur >= 0 && d) { anc[(size_t)s * chain_cap + (--d)] = (uint32_t)cur; cur = parent[cur]; }
}

// Host staging buffers of the upload: anonymous mappings, handed to the database handle and given back piece by piece by a helper
// thread after the first call (kmdb_release_staging).  Unmapping them right after the copies took 0.31 s of a 0.63 s upload
// (the HIP runtime has the ranges registered for its DMA), and a thread that does it meanwhile blocks every hipMalloc of the
// main thread for as long (both need the address-space lock).  (Transparent huge pages cut both the faults and
// the munmap 3 x, but one upload in ten on a fresh box then stalled 5 s in the kernel's page compaction: not used.)
struct HostRegion { void* p; size_t bytes; };
template <class T>
struct HostBuf {
    T* p = nullptr;
    size_t bytes = 0;
    explicit HostBuf(size_t n, bool zero = false) {
        (void)zero;                                             // anonymous mappings are zero-filled
        bytes = (std::max<size_t>(n, 1) * sizeof(T) + 4095) & ~(size_t)4095;
        void* q = mmap(nullptr, bytes, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS, -1, 0);
        p = q == MAP_FAILED ? nullptr : (T*)q;
    }
    ~HostBuf() { reset(); }
    void reset() { if (p) (void)munmap(p, bytes); p = nullptr; }
    HostRegion release() { HostRegion r{p, bytes}; p = nullptr; return r; }
    T& operator[](size_t i) { return p[i]; }
    HostBuf(const HostBuf&) = delete;
    HostBuf& operator=(const HostBuf&) = delete;
};

// KMDB_VERBOSE: the time since the last phase, after everything on the device has ended
struct LayPhase {
    const bool verbose = getenv("KMDB_VERBOSE") != nullptr;
    std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
    void operator()(const char* what) {
        if (!verbose) return;
        (void)hipDeviceSynchronize();
        const auto now = std::chrono::steady_clock::now();
        fprintf(stderr, "[kmdb] upload: %-34s %.3f s\n", what, std::chrono::duration<double>(now - t0).count());
        t0 = now;
    }
};

// What the device stage reads, all of it in HBM and in pid order.  The buffers are the stage's to release as soon as their last reader has run.
struct LayIn {
    uint64_t P = 0, N = 0;
    DevBuf<int32_t> parent;                  // -1 for roots
    DevBuf<uint32_t> ll, last, n, nbits, w;  // num_local, last id (0 where num_local is 0), num_samples, num_bits, weight (32 bits)
    DevBuf<unsigned long long> wfull;        // the untruncated weights, or empty (a part of a database: the plan's weights are the whole truth)
    const int64_t* wfull_host = nullptr;     // ... or still on the host: P counts the stage copies up when it needs them
    DevBuf<uint64_t> src_own;                // the stream words when the stage owns them
    const uint64_t* src = nullptr;           // the stream words: MSB first, stream p from bit srcpos[p] on
    DevBuf<uint64_t> srcpos;                 // empty: the streams lie back to back (the scan of nbits)
    uint64_t n_bit_words = 0;                // words of the DFS-order streams, the look-ahead padding included
    bool tables = false;                     // db->bucket_offset / db->slots hold the whole database's tables: pid2dfs is made
    bool qshard = false;                     // ... one query shard's, values = indices among the kept nodes
    uint64_t qs_slots = 0;
    uint64_t h2d_bytes = 0, dev_ht_bytes = 0;
    std::function<void()> streams_done;      // the source's own words behind `src` have had their last reader
};
int lay_device_stage(kmdb_db* db, LayIn& in, LayPhase& phase);

// The host loop of kmdb_layout_upload for a source that lies in HBM (kmdb_layout_from_device): one lane per pattern narrows the fields of the
// builder's state and of its finish stage (c), with the same checks — bad[0]: parent_id >= pattern id, bad[1]: inconsistent header (the
// stream's words inside the data words included: lay_copy_bits_kernel reads ceil(num_bits / 64) words from 64 * data_offset on).  The
// streams are word-aligned in pid order, so their source positions need no scan; the sum of num_bits (64 bits) sizes the DFS-order words.
__global__ __launch_bounds__(256) void lay_fields_kernel(const long long* __restrict__ num_kmers, const long long* __restrict__ parent_id, const uint32_t* __restrict__ num_samples,
                                                         const uint32_t* __restrict__ num_local, const uint32_t* __restrict__ last_id, const uint32_t* __restrict__ num_bits,
                                                         const unsigned long long* __restrict__ data_offset, uint64_t n_data_words, uint32_t P, uint32_t N,
                                                         int32_t* __restrict__ parent, uint32_t* __restrict__ ll, uint32_t* __restrict__ last, uint32_t* __restrict__ n_out,
                                                         uint32_t* __restrict__ nbits, uint32_t* __restrict__ w, unsigned long long* __restrict__ wfull,
                                                         uint64_t* __restrict__ srcpos, unsigned long long* __restrict__ total_bits, uint32_t* __restrict__ bad) {
    const uint32_t p = blockIdx.x * 256u + threadIdx.x;
    unsigned long long bits = 0;
    if (p < P) {
        const long long par = parent_id[p], nk = num_kmers[p];
        const uint32_t n = num_samples[p], l = num_local[p], nb = num_bits[p], lst = last_id[p];
        const unsigned long long off = data_offset[p], words = ((unsigned long long)nb + 63ull) / 64ull;
        if (par >= (long long)p) bad[0] = 1;
        if (l > n || n > N || (l && lst >= N) || nb >= KMDB_MAX_STREAM_BITS || off > n_data_words || words > n_data_words - off) bad[1] = 1;
        parent[p] = par < 0 ? -1 : (int32_t)par;
        ll[p] = l;
        last[p] = l ? lst : 0u;
        n_out[p] = n;
        nbits[p] = nb;
        w[p] = (uint32_t)nk;                   // truncated exactly like the reference's to_add (similarity_calculator.cpp:222)
        wfull[p] = (unsigned long long)nk;
        srcpos[p] = 64ull * off;
        bits = nb;
    }
    __shared__ unsigned long long s_bits[256];
    s_bits[threadIdx.x] = bits;
    __syncthreads();
    for (uint32_t s = 128; s > 0; s >>= 1) {
        if (threadIdx.x < s) s_bits[threadIdx.x] += s_bits[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0 && s_bits[0]) atomicAdd(total_bits, s_bits[0]);
}

}  // namespace

void kmdb_release_staging(kmdb_db* db) {
    if (db->staging.empty()) return;
    std::vector<std::pair<void*, size_t>> regions;
    regions.swap(db->staging);
    const bool unmap = !db->one_shot;
    if (db->staging_thread.joinable()) db->staging_thread.join();
    if (!unmap) db->staging_kept.insert(db->staging_kept.end(), regions.begin(), regions.end());      // unmapped by kmdb_db_free (they used to leak)
    db->staging_thread = std::thread([regions, unmap]() {
        // the pages first, on several threads under the shared address-space lock (kmdb_drop_pages); what munmap then holds the lock
        // exclusively for is the bookkeeping of empty ranges.  A one-shot handle (the front-end's) leaves even that to the end of the process.
        kmdb_drop_pages(regions, 8);
        if (unmap)
            for (const auto& r : regions) (void)munmap(r.first, r.second);
    });                                                       // joined by kmdb_db_settle / kmdb_db_free
}

int kmdb_layout_upload(kmdb_db* db, const kmdb_db_view* v, int with_hashtables, const kmdb_kept_nodes* sel) {
    const uint64_t P_view = v->n_patterns;
    // A part of the database planned on the host — a prefix shard (host_shards.cpp) or a tree range (host_ranges.cpp); `sel` says which
    // nodes and at which weight — lays out only the nodes it keeps: the fields of those nodes are narrowed, their streams packed, and
    // nothing else crosses PCIe — no hashtable slots, no node of another part of the tree.  (A prefix shard that owns no k-mer at all
    // keeps the whole tree with zero weights: every array stays non-empty.)
    // (An upload that carries the hashtables keeps the whole tree: new2all's pattern ids must all resolve.)
    // (A query shard is the exception: it carries only the slots of its own buckets, their values rewritten for the pruned layout below.)
    const bool qshard = sel && sel->qs_count > 1 && with_hashtables && v->n_buckets;
    const bool pruned = sel && (!with_hashtables || qshard) && !getenv("KMDB_SHARD_WHOLE_TREE") && sel->kept > 0 && sel->kept < P_view;
    uint64_t P = pruned ? sel->kept : P_view;                  // nodes laid out
    uint64_t h2d_bytes = 0;
    const uint64_t N = v->n_samples;
    LayPhase phase;
    const bool verbose = phase.verbose;
    hipStream_t st = db->stream;

    // ---- host: narrow + validate the header fields, pack the streams in pid order
    const unsigned hw = std::max(1u, std::thread::hardware_concurrency());
    const unsigned T = (unsigned)std::min<uint64_t>(std::min(64u, hw), std::max<uint64_t>(1, P_view / 65536));
    HostBuf<int32_t> h_parent(P);                             // not zero-filled: the pages are first touched by the worker threads
    HostBuf<uint32_t> h_ll(P), h_last(P), h_n(P), h_nbits(P), h_w(P);
    if (!h_parent.p || !h_ll.p || !h_last.p || !h_n.p || !h_nbits.p || !h_w.p) return kmdb_set_error("kmdb_db_upload: out of host memory");
    std::vector<uint64_t> part_bits(T + 1, 0);
    std::atomic<int> bad{0};
    // (the parts are ranges of the VIEW's pattern ids; a pruned shard writes the kept nodes of a part to their places in the shorter arrays)
    auto run_parts = [&](auto&& fn) {
        std::vector<std::thread> pool;
        for (unsigned t = 1; t < T; ++t) pool.emplace_back([&, t] { fn(t, P_view * t / T, P_view * (t + 1) / T); });
        fn(0u, (uint64_t)0, P_view / T);
        for (auto& th : pool) th.join();
    };
    if (sel && sel->mask && !sel->w) return kmdb_set_error("kmdb_db_upload_shard: the shard is not part of the plan");
    HostBuf<uint32_t> h_newidx(pruned ? P_view : 1);           // pruned: a kept node's index among the kept ones
    std::vector<uint64_t> part_kept(T + 1, 0);
    if (pruned) {
        if (!h_newidx.p) return kmdb_set_error("kmdb_db_upload: out of host memory");
        run_parts([&](unsigned t, uint64_t lo, uint64_t hi) {
            uint64_t c = 0;
            for (uint64_t p = lo; p < hi; ++p) c += sel->keeps(p) ? 1u : 0u;
            part_kept[t + 1] = c;
        });
        for (unsigned t = 0; t < T; ++t) part_kept[t + 1] += part_kept[t];
        if (part_kept[T] != P) return kmdb_set_error(std::string("kmdb_db_upload: internal: the count of kept nodes of the ") + sel->what + " is off");
        run_parts([&](unsigned t, uint64_t lo, uint64_t hi) {
            uint64_t o = part_kept[t];
            for (uint64_t p = lo; p < hi; ++p) if (sel->keeps(p)) h_newidx[p] = (uint32_t)o++;
        });
    }
    run_parts([&](unsigned t, uint64_t lo, uint64_t hi) {
        uint64_t nbsum = 0, o = pruned ? part_kept[t] : lo;
        for (uint64_t p = lo; p < hi; ++p) {
            if (pruned && !sel->keeps(p)) continue;
            const int64_t par = v->parent_id[p];
            const uint32_t n = v->num_samples[p], l = v->num_local[p], nb = v->num_bits[p], last = v->last_sample_id[p];
            if (par >= (int64_t)p) bad = 1;
            if (l > n || n > N || (l && last >= N) || nb >= KMDB_MAX_STREAM_BITS) bad = 2;      // (N < KMDB_MAX_SAMPLES: checked by the caller)
            h_parent[o] = par < 0 ? -1 : (pruned ? (int32_t)h_newidx[par] : (int32_t)par);         // (a kept node's parent is kept)
            h_ll[o] = l;
            h_last[o] = l ? last : 0u;
            h_n[o] = n;
            h_nbits[o] = nb;
            h_w[o] = sel ? sel->weight(p, v->num_kmers) : (uint32_t)v->num_kmers[p];     // truncated exactly like the reference's to_add (similarity_calculator.cpp:222)
            nbsum += nb;
            ++o;
        }
        part_bits[t + 1] = nbsum;
    });
    if (bad == 1) return kmdb_set_error("kmdb_db_upload: parent_id >= pattern id");
    if (bad) return kmdb_set_error("kmdb_db_upload: inconsistent pattern header");
    for (unsigned t = 0; t < T; ++t) part_bits[t + 1] += part_bits[t];
    const uint64_t total_bits = part_bits[T];
    const uint64_t n_bit_words = (total_bits + 63) / 64 + 16;       // zero padding words for the cursors' look-ahead
    HostBuf<uint64_t> h_bits(n_bit_words, /*zero=*/true);
    if (!h_bits.p) return kmdb_set_error("kmdb_db_upload: out of host memory");
    run_parts([&](unsigned t, uint64_t lo, uint64_t hi) {
        // streams of different threads can share a word at the range boundaries: OR the words in atomically
        uint64_t pos = part_bits[t];
        for (uint64_t p = lo; p < hi; ++p) {
            if (pruned && !sel->keeps(p)) continue;
            const uint32_t nb = v->num_bits[p];
            if (!nb) continue;
            const uint64_t* src = v->data + v->data_offset[p];
            for (uint32_t done = 0; done < nb; done += 64) {
                const uint32_t take = std::min<uint32_t>(64, nb - done);
                uint64_t chunk = src[done >> 6];
                if (take < 64) chunk &= ~0ull << (64 - take);
                const uint32_t sh = (uint32_t)(pos & 63);
                __atomic_fetch_or(&h_bits[pos >> 6], chunk >> sh, __ATOMIC_RELAXED);
                if (sh && take > 64 - sh) __atomic_fetch_or(&h_bits[(pos >> 6) + 1], chunk << (64 - sh), __ATOMIC_RELAXED);
                pos += take;
            }
        }
    });
    // ---- query shard: its own buckets packed back to back (local bucket b / count at the bucket's capacity, slot order kept), every value
    // rewritten to the node's index among the kept ones; the device turns that into the DFS index once the pre-order is known
    uint64_t qs_buckets = 0, qs_slots = 0;
    if (qshard) kmdb_query_shard_tables(v, sel->qs_index, sel->qs_count, &qs_buckets, &qs_slots);
    HostBuf<uint64_t> h_qoff(qs_buckets + 1), h_qslots(qs_slots);      // (one page each when the upload is no query shard)
    if (qshard) {
        HostBuf<uint64_t>& off = h_qoff;
        HostBuf<uint64_t>& sl = h_qslots;
        if (!off.p || !sl.p) return kmdb_set_error("kmdb_db_upload_query_shard: out of host memory");
        off[0] = 0;
        for (uint64_t lb = 0; lb < qs_buckets; ++lb) {
            const uint64_t b = lb * sel->qs_count + sel->qs_index;
            off[lb + 1] = off[lb] + (v->bucket_offset[b + 1] - v->bucket_offset[b]);
        }
        const unsigned TQ = (unsigned)std::min<uint64_t>(std::min(64u, hw), std::max<uint64_t>(1, qs_slots / (1u << 20)));
        std::atomic<int> bad_val{0};
        auto pack = [&](unsigned t) {
            for (uint64_t lb = qs_buckets * t / TQ; lb < qs_buckets * (t + 1) / TQ; ++lb) {
                const uint64_t b = lb * sel->qs_count + sel->qs_index;
                const uint64_t* src = v->slots + v->bucket_offset[b];
                uint64_t* dst = sl.p + off[lb];
                const uint64_t cap = off[lb + 1] - off[lb];
                for (uint64_t j = 0; j < cap; ++j) {
                    const uint64_t it = src[j];
                    const int32_t val = (int32_t)(it >> 32);
                    if (val == INT32_MAX) { dst[j] = it; continue; }
                    if (val < 0 || (uint64_t)val >= P_view || (pruned && !sel->keeps((uint64_t)val))) { bad_val = 1; dst[j] = it | (0x7fffffffull << 32); continue; }
                    dst[j] = (it & 0xFFFFFFFFull) | ((uint64_t)(pruned ? h_newidx[(uint64_t)val] : (uint32_t)val) << 32);
                }
            }
        };
        {
            std::vector<std::thread> pool;
            for (unsigned t = 1; t < TQ; ++t) pool.emplace_back(pack, t);
            pack(0u);
            for (auto& th : pool) th.join();
        }
        if (bad_val) return kmdb_set_error("kmdb_db_upload_query_shard: a hashtable value is no pattern id of the view");
    }
    phase("host: narrow fields + pack streams");

    // ---- H2D
    LayIn in;
    DevBuf<int32_t>& d_parent = in.parent;
    DevBuf<uint32_t>&d_ll = in.ll, &d_last = in.last, &d_n = in.n, &d_nbits = in.nbits, &d_w = in.w;
    DevBuf<uint64_t>& d_src = in.src_own;
    if (d_parent.alloc(std::max<size_t>(P, 1)) || d_ll.alloc(std::max<size_t>(P, 1)) || d_last.alloc(std::max<size_t>(P, 1)) || d_n.alloc(std::max<size_t>(P, 1)) || d_nbits.alloc(std::max<size_t>(P, 1)) || d_w.alloc(std::max<size_t>(P, 1)) || d_src.alloc(std::max<size_t>(n_bit_words, 1))) return 1;
    HIP_TRY(hipMemcpyAsync(d_parent.get(), h_parent.p, P * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d_ll.get(), h_ll.p, P * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d_last.get(), h_last.p, P * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d_n.get(), h_n.p, P * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d_nbits.get(), h_nbits.p, P * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d_w.get(), h_w.p, P * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d_src.get(), h_bits.p, n_bit_words * 8, hipMemcpyHostToDevice, st));
    h2d_bytes += P * 24 + n_bit_words * 8;
    DevBuf<unsigned long long>& d_wfull = in.wfull;           // sum_pairs uses the untruncated counts
    uint64_t dev_ht_bytes = 0;
    if (qshard) {
        // only the shard's own bucket table: no slot of a foreign bucket crosses PCIe, and no pid2dfs array is made (the slots hold DFS indices)
        db->n_buckets = qs_buckets; db->qs_index = sel->qs_index; db->qs_count = sel->qs_count;
        DEV_ALLOC(db->bucket_offset, qs_buckets + 1);
        DEV_ALLOC(db->slots, std::max<uint64_t>(qs_slots, 1));
        HIP_TRY(hipMemcpyAsync(db->bucket_offset, h_qoff.p, (qs_buckets + 1) * 8, hipMemcpyHostToDevice, st));
        if (qs_slots) HIP_TRY(hipMemcpyAsync(db->slots, h_qslots.p, qs_slots * 8, hipMemcpyHostToDevice, st));
        h2d_bytes += (qs_buckets + 1) * 8 + qs_slots * 8;
        dev_ht_bytes = (qs_buckets + 1) * 8 + std::max<uint64_t>(qs_slots, 1) * 8;
    } else if (with_hashtables && v->n_buckets) {
        const uint64_t n_slots = v->bucket_offset[v->n_buckets];
        db->n_buckets = v->n_buckets;
        DEV_ALLOC(db->bucket_offset, v->n_buckets + 1);
        DEV_ALLOC(db->slots, std::max<uint64_t>(n_slots, 1));
        HIP_TRY(hipMemcpyAsync(db->bucket_offset, v->bucket_offset, (v->n_buckets + 1) * 8, hipMemcpyHostToDevice, st));
        if (n_slots) HIP_TRY(hipMemcpyAsync(db->slots, v->slots, n_slots * 8, hipMemcpyHostToDevice, st));
        h2d_bytes += (v->n_buckets + 1) * 8 + n_slots * 8;
        dev_ht_bytes = (v->n_buckets + 1) * 8 + n_slots * 8 + P * 4;
    }
    // (a part of the database: the weights came from the plan — a prefix shard's own k-mer counts, a tree range's num_kmers inside the range
    // and 0 for the ancestors before it; partial matrices of all parts sum to the full one — and, unless the upload carries the hashtables
    // (new2all's pattern ids must all resolve: whole tree), only the kept nodes)
    HIP_TRY(hipStreamSynchronize(st));
    phase("H2D");
    if (pruned && verbose) fprintf(stderr, "[kmdb] upload: the %s keeps %llu of %llu patterns (%.1f MB over PCIe)\n", sel->what,
                                   (unsigned long long)P, (unsigned long long)P_view, h2d_bytes / 1e6);
    if (pruned) db->P = P;
    h_newidx.reset();
    for (HostRegion r : {h_parent.release(), h_ll.release(), h_last.release(), h_n.release(), h_nbits.release(), h_w.release(), h_bits.release(), h_qoff.release(), h_qslots.release()})
        if (r.p) db->staging.emplace_back(r.p, r.bytes);

    if (!sel) in.wfull_host = v->num_kmers;                   // (copied up by the device stage, where the node arrays are made)
    in.P = P; in.N = N; in.src = d_src.get(); in.n_bit_words = n_bit_words;
    in.qshard = qshard; in.qs_slots = qs_slots; in.tables = !qshard && with_hashtables && v->n_buckets;
    in.h2d_bytes = h2d_bytes; in.dev_ht_bytes = dev_ht_bytes;
    return lay_device_stage(db, in, phase);
}

// The device stage: from the pid-order arrays of `in` (all in HBM) to the handle's DFS-ordered layout.  Both sources end here: the host
// stage above (a view, narrowed and packed on the host, copied up) and kmdb_layout_from_device below (a builder's state, never off the device).
namespace {
int lay_device_stage(kmdb_db* db, LayIn& in, LayPhase& phase) {
    const uint64_t P = in.P, N = in.N, n_bit_words = in.n_bit_words;
    hipStream_t st = db->stream;
    if (const char* e = getenv("KMDB_SHORT_IDS")) if (*e) db->short_max_ids = (uint32_t)std::max(1, std::min(64, atoi(e)));     // (experiment, round 5)
    const unsigned B = 256;
    const unsigned G = (unsigned)((P + B - 1) / B), G1 = (unsigned)((P + 1 + B - 1) / B);
    DevBuf<int32_t>& d_parent = in.parent;
    DevBuf<uint32_t>&d_ll = in.ll, &d_last = in.last, &d_n = in.n, &d_nbits = in.nbits, &d_w = in.w;
    DevBuf<unsigned long long>& d_wfull = in.wfull;
    const bool qshard = in.qshard;
    const uint64_t qs_slots = in.qs_slots;
    // ---- device: DFS pre-order
    DevBuf<uint32_t> cnt, cstart, size, keys, vals, skeys, schild, ssz, S, acc[2], dep[2], order, flags;
    DevBuf<int32_t> anc[2];
    if (cnt.alloc(P + 2) || cstart.alloc(P + 2) || size.alloc(std::max<size_t>(P, 1)) || flags.alloc(4)) return 1;
    phase("  first device temporaries");
    HIP_TRY(hipMemsetAsync(cnt.get(), 0, (P + 2) * 4, st));
    HIP_TRY(hipMemsetAsync(cstart.get(), 0, (P + 2) * 4, st));
    HIP_TRY(hipMemsetAsync(flags.get(), 0, 16, st));
    // children grouped by parent, pid order inside a family
    if (keys.alloc(std::max<size_t>(P, 1)) || vals.alloc(std::max<size_t>(P, 1)) || skeys.alloc(std::max<size_t>(P, 1)) || schild.alloc(std::max<size_t>(P, 1))) return 1;
    HIP_TRY(hipStreamSynchronize(st));
    phase("  temporaries (hipMalloc)");
    hipLaunchKernelGGL(lay_keys_kernel, dim3(G), dim3(B), 0, st, d_parent.get(), (uint32_t)P, keys.get(), vals.get());
    {
        int end_bit = 1;
        while ((1ull << end_bit) <= P) ++end_bit;
        size_t tb = 0;
        HIP_TRY(prim::sort_pairs(nullptr, tb, keys.get(), skeys.get(), vals.get(), schild.get(), (int)P, 0, end_bit, st));
        DevBuf<unsigned char> tmp;
        if (tmp.alloc(std::max<size_t>(tb, 1))) return 1;
        HIP_TRY(hipStreamSynchronize(st));
        phase("  keys + sort temporaries");
        HIP_TRY(prim::sort_pairs(tmp.get(), tb, keys.get(), skeys.get(), vals.get(), schild.get(), (int)P, 0, end_bit, st));
        HIP_TRY(hipStreamSynchronize(st));
        phase("  radix sort");
    }
    keys.reset(); vals.reset();
    hipLaunchKernelGGL(lay_child_runs_kernel, dim3(G), dim3(B), 0, st, skeys.get(), (uint32_t)P, cstart.get(), cnt.get());
    hipLaunchKernelGGL(lay_child_len_kernel, dim3(G1), dim3(B), 0, st, cstart.get(), (uint32_t)(P + 1), cnt.get());
    phase("  sort by parent");
    // depth of every node: pointer doubling along the parent links (ping-pong buffers)
    for (int k = 0; k < 2; ++k) if (acc[k].alloc(std::max<size_t>(P, 1)) || dep[k].alloc(std::max<size_t>(P, 1)) || anc[k].alloc(std::max<size_t>(P, 1))) return 1;
    auto jump_all = [&](DevBuf<uint32_t>* val, int* cur_out) -> int {
        int cur = 0;
        HIP_TRY(hipMemcpyAsync(anc[0].get(), d_parent.get(), P * 4, hipMemcpyDeviceToDevice, st));
        for (int round = 0; round < 40; ++round) {
            HIP_TRY(hipMemsetAsync(flags.get(), 0, 4, st));
            hipLaunchKernelGGL(lay_jump_kernel, dim3(G), dim3(B), 0, st, val[cur].get(), anc[cur].get(), (uint32_t)P, val[cur ^ 1].get(), anc[cur ^ 1].get(), flags.get());
            uint32_t active = 0;
            HIP_TRY(hipMemcpyAsync(&active, flags.get(), 4, hipMemcpyDeviceToHost, st));
            HIP_TRY(hipStreamSynchronize(st));
            cur ^= 1;
            if (!active) break;
        }
        *cur_out = cur;
        return 0;
    };
    int dcur = 0;
    hipLaunchKernelGGL(lay_fill_kernel, dim3(G), dim3(B), 0, st, dep[0].get(), (uint32_t)P, 1u);
    if (jump_all(dep, &dcur)) return 1;
    dep[dcur ^ 1].reset();
    uint32_t max_depth = 0;
    {
        DevBuf<uint32_t> dmax;
        if (dmax.alloc(1)) return 1;
        size_t tb = 0;
        HIP_TRY(prim::max(nullptr, tb, dep[dcur].get(), dmax.get(), (int)P, st));
        DevBuf<unsigned char> tmp;
        if (tmp.alloc(std::max<size_t>(tb, 1))) return 1;
        HIP_TRY(prim::max(tmp.get(), tb, dep[dcur].get(), dmax.get(), (int)P, st));
        HIP_TRY(hipMemcpyAsync(&max_depth, dmax.get(), 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
    }
    phase("  depth");
    for (uint32_t level = max_depth; level >= 1; --level)
        hipLaunchKernelGGL(lay_sizes_level_kernel, dim3(G), dim3(B), 0, st, dep[dcur].get(), level, cstart.get(), cnt.get(), schild.get(), (uint32_t)P, size.get());
    HIP_TRY(hipGetLastError());
    phase("  subtree sizes");
    // pre-order offsets among siblings, then their sums along the root paths
    if (ssz.alloc(std::max<size_t>(P, 1)) || S.alloc(P + 1)) return 1;
    hipLaunchKernelGGL(lay_gather_u32_kernel, dim3(G), dim3(B), 0, st, size.get(), schild.get(), (uint32_t)P, ssz.get());
    {
        size_t tb1 = 0;
        HIP_TRY(prim::exclusive_sum(nullptr, tb1, ssz.get(), S.get(), (int)P, st));
        DevBuf<unsigned char> tmp;
        if (tmp.alloc(std::max<size_t>(tb1, 1))) return 1;
        HIP_TRY(prim::exclusive_sum(tmp.get(), tb1, ssz.get(), S.get(), (int)P, st));
        HIP_TRY(hipStreamSynchronize(st));
    }
    ssz.reset();
    hipLaunchKernelGGL(lay_rel_kernel, dim3(G), dim3(B), 0, st, skeys.get(), schild.get(), S.get(), cstart.get(), (uint32_t)P, acc[0].get());
    HIP_TRY(hipGetLastError());
    int cur = 0;
    if (jump_all(acc, &cur)) return 1;
    skeys.reset(); schild.reset(); S.reset(); cstart.reset();
    anc[0].reset(); anc[1].reset(); acc[cur ^ 1].reset();
    if (order.alloc(std::max<size_t>(P, 1))) return 1;
    HIP_TRY(hipMemsetAsync(order.get(), 0xFF, P * 4, st));
    hipLaunchKernelGGL(lay_order_kernel, dim3(G), dim3(B), 0, st, acc[cur].get(), (uint32_t)P, order.get(), flags.get() + 1);
    phase("device: DFS pre-order");

    // ---- DFS-ordered node arrays
    DEV_ALLOC(db->k0in, std::max<uint64_t>(P, 1));
    DEV_ALLOC(db->nl, std::max<uint64_t>(P, 1));
    DEV_ALLOC(db->parent, std::max<uint64_t>(P, 1));
    DEV_ALLOC(db->w, P + 1);
    DEV_ALLOC(db->dflag, std::max<uint64_t>(P, 1));
    DEV_ALLOC(db->sub_end, std::max<uint64_t>(P, 1));
    DevBuf<LayStats> d_stats;
    if (d_stats.alloc(1)) return 1;
    HIP_TRY(hipMemsetAsync(d_stats.get(), 0, sizeof(LayStats), st));
    if (in.wfull_host) {
        // the checksum sum_p w_p C(n_p, 2) is defined on the full 64-bit counts
        if (d_wfull.alloc(std::max<size_t>(P, 1))) return 1;
        HIP_TRY(hipMemcpyAsync(d_wfull.get(), in.wfull_host, P * 8, hipMemcpyHostToDevice, st));
        in.h2d_bytes += P * 8;
    }
    hipLaunchKernelGGL(lay_gather_kernel, dim3(std::min<unsigned>(G1, 2048u)), dim3(B), 0, st, order.get(), acc[cur].get(), dep[dcur].get(), cnt.get(), size.get(), d_parent.get(), d_ll.get(), d_last.get(), d_n.get(), d_nbits.get(), d_w.get(),
                       d_wfull.get(), (uint32_t)P, db->short_max_ids, db->k0in, db->nl, db->parent, db->w, db->dflag, db->sub_end, d_stats.get());
    HIP_TRY(hipGetLastError());
    LayStats hs{};
    uint32_t hflags[4] = {0, 0, 0, 0};
    HIP_TRY(hipMemcpyAsync(&hs, d_stats.get(), sizeof hs, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(hflags, flags.get(), 16, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (hflags[1]) return kmdb_set_error("kmdb_db_upload: pattern tree is not a forest");
    if (qshard) {
        if (qs_slots) {
            hipLaunchKernelGGL(lay_slots_to_dfs_kernel, dim3((unsigned)std::min<uint64_t>((qs_slots + 255) / 256, 8192)), dim3(256), 0, st, db->slots, qs_slots, acc[cur].get(), (uint32_t)P);
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipStreamSynchronize(st));
        }
    } else if (in.tables) {
        // pid -> DFS index for the hash lookups of new2all
        DEV_ALLOC(db->pid2dfs, std::max<uint64_t>(P, 1));
        hipLaunchKernelGGL(lay_pid2dfs_kernel, dim3(G), dim3(B), 0, st, acc[cur].get(), (uint32_t)P, db->pid2dfs);
        HIP_TRY(hipStreamSynchronize(st));
    }
    d_wfull.reset(); d_ll.reset(); d_last.reset(); d_n.reset(); d_w.reset(); size.reset(); cnt.reset(); dep[dcur].reset(); d_parent.reset();
    phase("device: node arrays");

    // ---- streams re-packed in DFS order
    {
        DevBuf<uint32_t> nb_dfs;
        // (a source that names its own stream positions has filled in.srcpos; the host stage packs back to back: the scan of num_bits)
        const bool packed = !in.srcpos;
        DevBuf<uint64_t>& srcpos = in.srcpos;
        DevBuf<uint64_t> dstpos;
        if (nb_dfs.alloc(std::max<size_t>(P, 1)) || (packed && srcpos.alloc(P + 1)) || dstpos.alloc(P + 1)) return 1;
        hipLaunchKernelGGL(lay_nbits_dfs_kernel, dim3(G), dim3(B), 0, st, db->k0in, (uint32_t)P, nb_dfs.get());
        rocprim::transform_iterator<uint32_t*, U32toU64, uint64_t> it_src(d_nbits.get(), U32toU64()), it_dst(nb_dfs.get(), U32toU64());
        size_t tb = 0;
        HIP_TRY(prim::exclusive_sum(nullptr, tb, it_src, srcpos.get(), (int)P, st));
        DevBuf<unsigned char> tmp;
        if (tmp.alloc(std::max<size_t>(tb, 1))) return 1;
        if (packed) HIP_TRY(prim::exclusive_sum(tmp.get(), tb, it_src, srcpos.get(), (int)P, st));
        HIP_TRY(prim::exclusive_sum(tmp.get(), tb, it_dst, dstpos.get(), (int)P, st));
        DEV_ALLOC(db->bits, n_bit_words);
        HIP_TRY(hipMemsetAsync(db->bits, 0, n_bit_words * 8, st));
        db->n_bit_words = n_bit_words;
        DEV_ALLOC(db->blkbase, (P + 255) / 256 + 1);
        DEV_ALLOC(db->bitrel, std::max<uint64_t>(P, 1));
        hipLaunchKernelGGL(lay_blkbase_kernel, dim3(G), dim3(B), 0, st, dstpos.get(), (uint32_t)P, db->blkbase, db->bitrel);
        hipLaunchKernelGGL(lay_copy_bits_kernel, dim3(G), dim3(B), 0, st, order.get(), srcpos.get(), dstpos.get(), db->k0in, in.src, (uint32_t)P,
                           (unsigned long long*)db->bits.get());
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipStreamSynchronize(st));
    }
    in.srcpos.reset(); in.src_own.reset(); in.src = nullptr; d_nbits.reset(); order.reset();
    if (in.streams_done) in.streams_done();
    phase("device: stream re-pack");

    // ---- per-slice root paths, long nodes
    db->max_n = hs.max_n; db->max_depth = hs.max_depth;
    db->chain_ok = hs.max_depth <= (uint32_t)KMDB_CHAIN_MAX;
    db->chain_cap = std::min<uint32_t>(KMDB_CHAIN_MAX, std::max<uint32_t>(8, (hs.max_depth + 7) / 8 * 8));
    // one wave per slice of 2048 nodes.  (Round 1 used about 8192 slices in all, 12 544 nodes each at the benchmark database,
    // because every wave left its open record chunks half empty; since only the first block's diagonal records go through
    // stream chunks that costs little — measured: narrow kernel 1.83 -> 1.37 ms, chunks 186 k -> 208 k, whole call -0.3 ms;
    // 1024 nodes: no faster, more chunks.)
    db->nseg_nodes = 2048;
    if (const char* e = getenv("KMDB_NSEG")) if (*e) db->nseg_nodes = (uint32_t)std::max<uint64_t>(64, strtoull(e, nullptr, 10) / 64 * 64);
    db->n_nsegs = (uint32_t)((P + db->nseg_nodes - 1) / db->nseg_nodes);
    DEV_ALLOC(db->nseg_anc, std::max<size_t>((size_t)db->n_nsegs * db->chain_cap, 1));
    DEV_ALLOC(db->nseg_anc_n, std::max<size_t>(db->n_nsegs, 1));
    if (db->n_nsegs)
        hipLaunchKernelGGL(lay_seg_anc_kernel, dim3((db->n_nsegs + 63) / 64), dim3(64), 0, st, db->parent, db->dflag, (uint32_t)P, db->nseg_nodes, db->n_nsegs,
                           db->chain_cap, db->nseg_anc, db->nseg_anc_n);
    db->n_long = hs.n_long;
    if (hs.n_long) {
        DevBuf<uint32_t> sel, lk, lk2, nsel;
        if (sel.alloc(hs.n_long + 1) || lk.alloc(std::max<size_t>(hs.n_long, 1)) || lk2.alloc(std::max<size_t>(hs.n_long, 1)) || nsel.alloc(1)) return 1;
        DEV_ALLOC(db->long_nodes, (size_t)hs.n_long);
        rocprim::counting_iterator<uint32_t> first(0u);
        size_t tb = 0;
        HIP_TRY(prim::select_if(nullptr, tb, first, sel.get(), nsel.get(), (int)P, LongNodePred{db->k0in, db->short_max_ids}, st));
        DevBuf<unsigned char> tmp;
        if (tmp.alloc(std::max<size_t>(tb, 1))) return 1;
        HIP_TRY(prim::select_if(tmp.get(), tb, first, sel.get(), nsel.get(), (int)P, LongNodePred{db->k0in, db->short_max_ids}, st));
        hipLaunchKernelGGL(lay_long_keys_kernel, dim3((hs.n_long + 255) / 256), dim3(256), 0, st, db->k0in, sel.get(), hs.n_long, lk.get());
        // most work first; the sort is stable, so equal work keeps ascending DFS order
        size_t tb2 = 0;
        HIP_TRY(prim::sort_pairs_desc(nullptr, tb2, lk.get(), lk2.get(), sel.get(), db->long_nodes.get(), (int)hs.n_long, 0, 32, st));
        DevBuf<unsigned char> tmp2;
        if (tmp2.alloc(std::max<size_t>(tb2, 1))) return 1;
        HIP_TRY(prim::sort_pairs_desc(tmp2.get(), tb2, lk.get(), lk2.get(), sel.get(), db->long_nodes.get(), (int)hs.n_long, 0, 32, st));
        HIP_TRY(hipStreamSynchronize(st));
    }
    // the short launch's work order, per window of k0_window DFS nodes (a power of two)
    db->k0_window = KMDB_K0_WINDOW_DEFAULT;
    if (const char* e = getenv("KMDB_K0_WINDOW")) if (*e) {
        const uint32_t want = (uint32_t)std::max(0, atoi(e));
        uint32_t w = KMDB_K0_WINDOW_MIN;
        while (w < KMDB_K0_WINDOW_MAX && w < want) w <<= 1;
        db->k0_window = w;
    }
    const uint64_t n_windows = (P + db->k0_window - 1) / db->k0_window;
    DEV_ALLOC(db->k0_order, std::max<uint64_t>(n_windows * db->k0_window, 1));
    DEV_ALLOC(db->k0_live, std::max<uint64_t>(n_windows, 1));
    if (n_windows) {
        hipLaunchKernelGGL(lay_k0_order_kernel, dim3((unsigned)n_windows), dim3(256), 0, st, db->k0in, (uint32_t)P, db->k0_window, db->short_max_ids,
                           db->k0_order.get(), db->k0_live.get());
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipStreamSynchronize(st));
    phase("device: slices + long nodes + decode order");

    db->stats.algorithmic_bytes = hs.alg + 4ull * (N ? N * (N - 1) / 2 : 0);
    db->stats.tree_updates = hs.upd;
    db->stats.sum_pairs = hs.pairs;
    db->stats.n_segments = db->n_nsegs;
    db->stats.n_patterns = P;
    db->stats.h2d_bytes = in.h2d_bytes;
    db->stats.device_bytes = P * (8 + 4 + 4 + 4 + 4 + 2 + 4) + n_bit_words * 8 + (uint64_t)db->n_nsegs * db->chain_cap * 4 + in.dev_ht_bytes +
                             n_windows * db->k0_window * 2 + n_windows * 4;
    return 0;
}
}  // namespace

// (tests) the short launch's work order as the handle holds it.  window / n_windows: its geometry; order: n_windows * window offsets; live: n_windows
// counts; l, num_bits: the P list heads in DFS order that the keys were made from.  Every output may be null.
extern "C" int kmdb_debug_k0_order(const kmdb_db* db, uint32_t* window, uint64_t* n_windows, uint16_t* order, uint32_t* live, uint32_t* l, uint32_t* num_bits) {
    if (!db) return kmdb_set_error("kmdb_debug_k0_order: null handle");
    const uint64_t nw = (db->P + db->k0_window - 1) / db->k0_window;
    if (window) *window = db->k0_window;
    if (n_windows) *n_windows = nw;
    HIP_TRY(hipSetDevice(db->device));
    HIP_TRY(hipStreamSynchronize(db->stream));
    if (order && nw) HIP_TRY(hipMemcpy(order, db->k0_order.get(), nw * db->k0_window * 2, hipMemcpyDeviceToHost));
    if (live && nw) HIP_TRY(hipMemcpy(live, db->k0_live.get(), nw * 4, hipMemcpyDeviceToHost));
    if ((l || num_bits) && db->P) {
        std::vector<uint2> km(db->P);
        HIP_TRY(hipMemcpy(km.data(), db->k0in.get(), db->P * sizeof(uint2), hipMemcpyDeviceToHost));
        for (uint64_t i = 0; i < db->P; ++i) {
            if (l) l[i] = kmdb_k0_l(km[i]);
            if (num_bits) num_bits[i] = kmdb_k0_bits(km[i]);
        }
    }
    return 0;
}

// The second source of the device stage: a builder's state at the end of its finish stages (c) and (d) (build.hip), read where it lies.
// No pattern field, stream word or table slot visits the host: one kernel narrows the fields, the tables go device to device, and the
// streams are re-packed from their word-aligned pid-order places (srcpos = 64 * data_offset; lay_copy_bits_kernel's tail mask drops the
// padding, and with an aligned source it never reads the word behind a stream).
int kmdb_layout_from_device(kmdb_db* db, const kmdb_layout_device_source* s, int with_hashtables) {
    const uint64_t P = s->n_patterns, N = s->n_samples;
    const auto t0 = std::chrono::steady_clock::now();
    LayPhase phase;
    hipStream_t st = db->stream;
    LayIn in;
    in.P = P; in.N = N;
    DevBuf<unsigned long long> total;
    DevBuf<uint32_t> bad;
    if (in.parent.alloc(P) || in.ll.alloc(P) || in.last.alloc(P) || in.n.alloc(P) || in.nbits.alloc(P) || in.w.alloc(P) || in.wfull.alloc(P) || in.srcpos.alloc(P + 1) ||
        total.alloc(1) || bad.alloc(2)) return 1;
    HIP_TRY(hipMemsetAsync(total.get(), 0, 8, st));
    HIP_TRY(hipMemsetAsync(bad.get(), 0, 8, st));
    hipLaunchKernelGGL(lay_fields_kernel, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, st, s->num_kmers, s->parent_id, s->num_samples, s->num_local, s->last_sample_id,
                       s->num_bits, s->data_offset, s->n_data_words, (uint32_t)P, (uint32_t)N, in.parent.get(), in.ll.get(), in.last.get(), in.n.get(), in.nbits.get(), in.w.get(),
                       in.wfull.get(), in.srcpos.get(), total.get(), bad.get());
    HIP_TRY(hipGetLastError());
    unsigned long long total_bits = 0;
    uint32_t hbad[2] = {0, 0};
    HIP_TRY(hipMemcpyAsync(&total_bits, total.get(), 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(hbad, bad.get(), 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (hbad[0]) return kmdb_set_error("kmdb_db_upload: parent_id >= pattern id");
    if (hbad[1]) return kmdb_set_error("kmdb_db_upload: inconsistent pattern header");
    if (s->fields_done) s->fields_done();                     // (the kernel has ended: nothing reads the source's fields again)
    in.n_bit_words = (total_bits + 63) / 64 + 16;             // zero padding words for the cursors' look-ahead
    in.src = s->data;
    if (with_hashtables && s->n_buckets) {
        db->n_buckets = s->n_buckets;
        DEV_ALLOC(db->bucket_offset, s->n_buckets + 1);
        DEV_ALLOC(db->slots, std::max<uint64_t>(s->n_slots, 1));
        HIP_TRY(hipMemcpyAsync(db->bucket_offset, s->bucket_offset, (s->n_buckets + 1) * 8, hipMemcpyDeviceToDevice, st));
        if (s->n_slots) HIP_TRY(hipMemcpyAsync(db->slots, s->slots, s->n_slots * 8, hipMemcpyDeviceToDevice, st));
        HIP_TRY(hipStreamSynchronize(st));
        in.tables = true;
        in.dev_ht_bytes = (s->n_buckets + 1) * 8 + s->n_slots * 8 + P * 4;
    }
    if (s->tables_done) s->tables_done();
    in.streams_done = s->streams_done;
    s->fields_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    phase("device: narrow fields");
    return lay_device_stage(db, in, phase);
}
