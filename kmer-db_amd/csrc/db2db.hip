// db2db.hip — two-database counting behind kmdb_db2db_dense (include/kmdb_amd.h).
//
// Replaces SimilarityCalculator::db2db_sp (reference src/similarity_calculator.cpp:1225-1540), the cell (row part,
// column part) of the all2all-parts grid (src/console_all2all_parts.cpp:143-331).  The reference merge-joins the
// sorted (suffix, pattern) lists of every k-mer prefix of the two databases, counts the equal (pattern_row,
// pattern_col) pairs and adds the count to every pair of samples of the two patterns.  Here:
//   probe    one thread per hashtable slot of the COLUMN database: its k-mer is looked up in the row database's
//            table of the same prefix (murmur3 fmix32 probe, src/hashmap_lp.h:53-64,308-333);
//            key = DFS index of the row pattern << cbits | DFS index of the column pattern (cbits: as many as the column
//            database's patterns need), or ~0
//   count    radix sort (of the bits in use only) + run-length encode of the keys: (pattern pair, number of shared k-mers)
//   lists    once per handle (kept with it: every cell of an all2all-parts grid uses a part many times): the FULL sample list of
//            every pattern as a bit set over blocks of 64 ids, filled top-down — list(node) = list(parent) | local ids — one
//            launch per tree level.  Parts with more than 4096 samples or a store beyond 8 GB do without it: their waves
//            climb the root path of each pattern of a pair instead (lane d decodes the d-th node of the path)
//   emit     one wave per pattern pair: both lists from the store into LDS, one BLOCK RECORD (row block, column block, row
//            mask, column mask, count) per pair of non-empty blocks into a pool, in arrival order
//   apply    kmdb_rect_sort_apply (a2a_blocks.hip): the all2all pipeline's counting sort by block pair and its matrix-core
//            accumulation kernel, writing the dense rows x columns matrix.
// kmdb_db2db_dense copies that matrix to the host.  kmdb_db2db_sparse_filtered (db2db_sp + SparseMatrix::compact2 with the -min / -max
// CombinedFilter, src/console_all2all_parts.cpp:179-195, 225-241; src/array.h:391-446) compacts it where it is:
//   flags    one byte per 64 x 64 tile of the cell, set from the key words of the emit pool: the tiles that received a block record
//   compact  one wave per row over the flagged tiles of its row block: widened bounds (cell_filter.h), per-row counts, exclusive sum,
//            (col, val) in ascending columns; the exact decision is the host's (kmdb_sparse_decide, engine.hip)
// kmdb_db2db_csr_device (engine_internal.h; the cells of `all2all-parts -distance`, distance.hip) is the same compaction without bounds whose
// three buffers stay in HBM: nothing is copied to the host and nothing is decided here.
// kmdb_db2db_sampled (db2db_sp + compact2(filter) + SparseMatrix::add_to_sampler of an off-diagonal cell with -sample-rows <criterion>:<count>,
// src/console_all2all_parts.cpp:179-195, 225-241; src/array.h:450-540) keeps the cell in HBM as well and selects there:
//   flags    as above
//   select   the radix select of sample_rows.hip on the flagged tiles of the rectangle: per row sample and per column sample a superset of its
//            `count` best cells of this cell (kmdb_sample_rect, engine.hip: selection, completeness rule, re-fetch)
#include "kmdb_amd.h"
#include "kmdb_internal.h"
#include "engine_internal.h"

#include <hip/hip_runtime.h>
#include "prim.h"
#include "hash_probe.h"
#include "cell_filter.h"
#include "device_common.h"

#include <algorithm>
#include <cstring>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

namespace {

constexpr unsigned long long D2_INVALID = ~0ull;

__device__ __forceinline__ uint32_t d2_fmix32(uint32_t h) {
    h ^= h >> 16; h *= 0x85ebca6bu; h ^= h >> 13; h *= 0xc2b2ae35u; h ^= h >> 16;
    return h;
}

struct D2Db {                                   // device pointers of one resident database
    uint64_t n_buckets;
    const uint64_t* bucket_offset;
    const uint64_t* slots;
    const uint32_t* pid2dfs;
    const uint4* meta;
    const uint64_t* bitpos;
    const int32_t* parent;
    const uint64_t* bits;
};

__global__ void d2_probe_kernel(D2Db row, D2Db col, uint64_t n_col_slots, uint32_t cbits, unsigned long long* __restrict__ keys) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_col_slots) return;
    unsigned long long key = D2_INVALID;
    const uint64_t it = col.slots[i];
    const int32_t pc = (int32_t)(it >> 32);
    if (pc != 0x7fffffff) {
        // bucket of this slot: last bucket whose offset is <= i
        uint64_t lo = 0, hi = col.n_buckets;
        while (hi - lo > 1) { const uint64_t mid = (lo + hi) >> 1; if (col.bucket_offset[mid] <= i) lo = mid; else hi = mid; }
        const uint64_t b = lo;
        if (b < row.n_buckets) {
            const uint64_t off = row.bucket_offset[b], cap = row.bucket_offset[b + 1] - off;
            if (cap) {
                const int32_t pr = kmdb_probe(row.slots, off, cap, (uint32_t)it);
                if (pr != 0x7fffffff) key = ((unsigned long long)row.pid2dfs[pr] << cbits) | col.pid2dfs[pc];
            }
        }
    }
    keys[i] = key;
}

// full list of the pattern with DFS index `node` as a bit set over the sample ids (64 per word): lane d decodes the d-th
// node of the root path and ORs its local ids in (pattern_t::decodeSamples, src/pattern.cpp:99-109: first id = last - sum of the deltas)
__device__ __forceinline__ void d2_list_bits(const D2Db& db, uint32_t node, unsigned long long* set, uint32_t lane) {
    int64_t r = node;
    uint32_t d = 0;
    while (r >= 0) {                             // every lane walks the path; lane (d mod 64) decodes node d
        if ((d & 63u) == lane) {
            const uint4 m = db.meta[r];
            const uint32_t l = m.y;
            if (l) {
                uint32_t id = m.z;
                if (l > 1) {
                    // (gamma_first_id, written out: through the helper the second loop kept a test of l — 2 % of the call, profiles/gamma_reader_ab.json)
                    GammaCursor<1> c1(db.bits, db.bitpos[r]);
                    uint32_t sum = 0;
                    for (uint32_t t = 0; t + 1 < l; ++t) sum += c1.next();
                    id = m.z - sum;
                    GammaCursor<1> c2(db.bits, db.bitpos[r]);
                    for (uint32_t t = 0; t + 1 < l; ++t) { atomicOr(&set[id >> 6], 1ull << (id & 63u)); id += c2.next(); }
                }
                atomicOr(&set[id >> 6], 1ull << (id & 63u));
            }
        }
        r = db.parent[r];
        ++d;
    }
}

// ---- the list store
// One launch per level of the tree: a node is filled in the first round that finds its parent filled by an EARLIER round
// (done[] holds round + 1; a parent filled in this very round reads as either 0 or round + 1, both mean "not yet").
constexpr uint32_t D2_SETS_MAX_NB = 64;                       // parts of up to 4096 samples
constexpr uint64_t D2_SETS_MAX_BYTES = 8ull << 30;
// (done is read and written by different threads of one launch: no __restrict__, relaxed atomic loads)
__global__ __launch_bounds__(256) void d2_sets_round_kernel(D2Db db, uint32_t P, uint32_t nb, uint32_t round, uint32_t* done,
                                                            unsigned long long* sets, uint32_t* __restrict__ n_done) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    bool fill = i < P && __atomic_load_n(&done[i], __ATOMIC_RELAXED) == 0;
    int32_t par = -1;
    if (fill) {
        par = db.parent[i];
        if (par >= 0) { const uint32_t dr = __atomic_load_n(&done[par], __ATOMIC_RELAXED); fill = dr != 0 && dr != round + 1u; }
    }
    if (fill) {
        unsigned long long* s = sets + (size_t)i * nb;
        if (par >= 0) { const unsigned long long* ps = sets + (size_t)par * nb; for (uint32_t k = 0; k < nb; ++k) s[k] = ps[k]; }
        else for (uint32_t k = 0; k < nb; ++k) s[k] = 0;
        const uint4 m = db.meta[i];
        const uint32_t l = m.y;
        if (l) {
            uint32_t id = m.z;
            if (l > 1) {
                id = gamma_first_id<1, false>(db.bits, db.bitpos[i], l, m.z);
                GammaCursor<1> c2(db.bits, db.bitpos[i]);
                uint32_t cw = id >> 6;
                unsigned long long acc = 0;
                for (uint32_t t = 0; t + 1 < l; ++t) {                    // ids ascend: one read-modify-write per word
                    const uint32_t wd = id >> 6;
                    if (wd != cw) { s[cw] |= acc; acc = 0; cw = wd; }
                    acc |= 1ull << (id & 63u);
                    id += c2.next();
                }
                if ((id >> 6) != cw) { s[cw] |= acc; acc = 0; cw = id >> 6; }
                acc |= 1ull << (id & 63u);
                s[cw] |= acc;
            } else s[id >> 6] |= 1ull << (id & 63u);
        }
        done[i] = round + 1u;
    }
    const unsigned long long bal = __ballot(fill);
    if (bal && (threadIdx.x & 63u) == (uint32_t)__ffsll((long long)bal) - 1u) atomicAdd(n_done, (uint32_t)__popcll(bal));
}

// Pattern pairs -> block records.  A pair (row pattern, column pattern, c shared k-mers) adds c to every cell (sample of the
// row pattern, sample of the column pattern): with both lists as bit sets over blocks of 64 ids that is one record
// (row block, column block, row mask, column mask, c) per pair of non-empty blocks — the record form of the all2all pipeline
// (a2a_blocks.hip), sorted by block pair and accumulated on the matrix cores by the same kernels.  (Round 1 added the cells
// one by one with HBM atomics: 100 ms for two 1000-sample databases.)
// One wave per pair, persistent waves.  COUNT: only the number of records (sizes the pool); else: records into the pool in
// arrival order, slots taken GRAB at a time from one of 256 cursors (a shared cursor would serialise: same-address atomics).
constexpr uint32_t D2_GRAB = 512, D2_CURSORS = 256;
// 64-bit words of LDS one wave of the pair kernel needs: both bit sets, both compacted mask lists, both 16-bit index lists
__host__ __device__ inline size_t d2_wave_words(uint32_t nbr, uint32_t nbc) { return (size_t)2 * (nbr + nbc) + ((size_t)(nbr + nbc) * 2 + 7) / 8; }
struct D2Pool { uint32_t* wkey; ulonglong2* wrec; uint32_t* cursor; uint32_t region; uint32_t kbits, dbits; uint32_t* overflow; };
template <bool COUNT, bool STORE>
__global__ __launch_bounds__(256) void d2_emit_kernel(D2Db row, D2Db col, const unsigned long long* __restrict__ rsets, const unsigned long long* __restrict__ csets,
                                                      const unsigned long long* __restrict__ pairs, const uint32_t* __restrict__ counts,
                                                      uint32_t npairs, uint32_t nbr, uint32_t nbc, uint32_t cbits, D2Pool pool,
                                                      unsigned long long* __restrict__ n_records) {
    extern __shared__ unsigned long long d2_lds[];          // per wave: row set [nbr], column set [nbc], the non-empty blocks of each, their block indices
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6, wpb = blockDim.x >> 6;       // 1 .. 4 waves per workgroup, by the LDS a wave needs
    const size_t per_wave = d2_wave_words(nbr, nbc);
    unsigned long long* rset = d2_lds + (size_t)wave * per_wave;
    unsigned long long* cset = rset + nbr;
    unsigned long long* rmask = cset + nbc;                   // compacted: mask of the a-th non-empty row block
    unsigned long long* cmask = rmask + nbr;
    uint16_t* ridx = (uint16_t*)(cmask + nbc);                // ... and its block index (a block index fits 16 bits up to 4 M samples)
    uint16_t* cidx = ridx + nbr;
    const uint32_t wid = blockIdx.x * wpb + wave, nwaves = gridDim.x * wpb;
    const unsigned long long lt_mask = (1ull << lane) - 1ull;
    unsigned long long mine = 0;
    uint32_t next = 0, left = 0, sub = wid % D2_CURSORS;      // the wave's current grab of pool slots
    // the pairs are sorted by row pattern: a wave takes a contiguous share and keeps the row pattern's list while it repeats
    const uint32_t i_lo = (uint32_t)((uint64_t)npairs * wid / nwaves), i_hi = (uint32_t)((uint64_t)npairs * (wid + 1u) / nwaves);
    uint32_t cached_pr = 0xFFFFFFFFu, na = 0;
    for (uint32_t i = i_lo; i < i_hi; ++i) {
        const unsigned long long key = pairs[i];
        if (key == D2_INVALID) continue;
        const uint32_t pr = (uint32_t)(key >> cbits), pc = (uint32_t)(key & ((1ull << cbits) - 1ull));
        uint32_t c = counts[i];
        const bool new_row = pr != cached_pr;
        if (STORE) {
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup"); __builtin_amdgcn_wave_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");   // (the previous pair's reads)
            if (new_row) for (uint32_t k = lane; k < nbr; k += 64u) rset[k] = rsets[(size_t)pr * nbr + k];
            for (uint32_t k = lane; k < nbc; k += 64u) cset[k] = csets[(size_t)pc * nbc + k];
        } else {
            for (uint32_t k = lane + (new_row ? 0u : nbr); k < nbr + nbc; k += 64u) rset[k] = 0;
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup"); __builtin_amdgcn_wave_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
            if (new_row) d2_list_bits(row, pr, rset, lane);
            d2_list_bits(col, pc, cset, lane);
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup"); __builtin_amdgcn_wave_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
        // the non-empty blocks of both lists, compacted in order
        uint32_t nb = 0;
        if (new_row) {
            na = 0; cached_pr = pr;
            for (uint32_t k0 = 0; k0 < nbr; k0 += 64u) {
                const uint32_t k = k0 + lane;
                const unsigned long long m = k < nbr ? rset[k] : 0ull;
                const unsigned long long bal = __ballot(m != 0);
                if (m) { const uint32_t o = na + (uint32_t)__popcll(bal & lt_mask); rmask[o] = m; ridx[o] = (uint16_t)k; }
                na += (uint32_t)__popcll(bal);
            }
        }
        for (uint32_t k0 = 0; k0 < nbc; k0 += 64u) {
            const uint32_t k = k0 + lane;
            const unsigned long long m = k < nbc ? cset[k] : 0ull;
            const unsigned long long bal = __ballot(m != 0);
            if (m) { const uint32_t o = nb + (uint32_t)__popcll(bal & lt_mask); cmask[o] = m; cidx[o] = (uint16_t)k; }
            nb += (uint32_t)__popcll(bal);
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup"); __builtin_amdgcn_wave_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
        // one record per block pair and per base-2^dbits digit of c (exact: shifted digits add up in uint32 wrap-around arithmetic)
        uint32_t nd = 0;
        for (uint32_t w = c; w; w >>= pool.dbits) ++nd;
        const uint32_t T = na * nb * nd;
        if (COUNT) { if (lane == 0) mine += T; continue; }
        const uint32_t dmask = (1u << pool.dbits) - 1u;
        for (uint32_t t0 = 0; t0 < T; t0 += 64u) {
            const uint32_t cnt = T - t0 < 64u ? T - t0 : 64u;
            if (left < cnt) {                                  // a fresh grab from the next cursor (the tail of the old one stays unwritten)
                sub = (sub + 61u) % D2_CURSORS;
                uint32_t base = 0;
                if (lane == 0) base = atomicAdd(&pool.cursor[sub * 16u], D2_GRAB);
                base = (uint32_t)__shfl((int)base, 0, 64);
                if (base + D2_GRAB > pool.region) { if (lane == 0) atomicOr(pool.overflow, 1u); base = pool.region - D2_GRAB; }
                next = sub * pool.region + base; left = D2_GRAB;
            }
            const uint32_t t = t0 + lane;
            if (t < T) {
                const uint32_t j = t % nd, ab = t / nd, a = ab / nb, b = ab - a * nb;
                const uint32_t digit = (c >> (j * pool.dbits)) & dmask;
                const uint32_t stream = (uint32_t)ridx[a] * nbc + cidx[b];
                pool.wrec[next + lane] = make_ulonglong2(rmask[a], cmask[b]);
                pool.wkey[next + lane] = stream | ((digit | (j << pool.dbits)) << pool.kbits);
            }
            next += cnt; left -= cnt;
        }
    }
    if (COUNT && lane == 0 && mine) atomicAdd(&n_records[(wid % 64u) * 8u], mine);
}

// ---- the sparse form of the cell
// The tiles that received a block record: the stream of a key word is row block * nbc + column block (d2_emit_kernel); a slot never written is
// all ones, and 2^key_bits > n_tiles + 1, so its stream lies beyond the tiles.  (Every writer stores 1: plain byte stores.)
__global__ __launch_bounds__(256) void d2_tile_flags_kernel(const uint32_t* __restrict__ wkey, uint32_t nslots, uint32_t kmask, uint32_t n_tiles,
                                                            unsigned char* __restrict__ flags) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nslots) return;
    const uint32_t s = wkey[i] & kmask;
    if (s < n_tiles) flags[s] = 1;
}

// Dense cell -> CSR over the FLAGGED tiles only, the rectangle's counterpart of row_tiles_kernel (engine.hip).  One wave per row of the cell: it
// takes the nbc flags of its row block 64 per round by ballot and reads, for every flagged tile, the row's 64 cells (a lane each).  A lane whose
// column is >= nc loads nothing — in a row-major rectangle that address is a cell of the NEXT row — and the cell offset row * nc + column is
// 64-bit (66 000 x 66 000 cells exceed 2^32).  COMPACT false: row_nnz[row] = kept cells; true: (col, val) from row_ptr[row] on, ascending columns.
template <bool COMPACT>
__global__ __launch_bounds__(64) void d2_row_tiles_kernel(const uint32_t* __restrict__ M, uint32_t nr, uint32_t nc, uint32_t nbc,
                                                          const unsigned char* __restrict__ flags, unsigned long long* __restrict__ row_nnz,
                                                          const unsigned long long* __restrict__ row_ptr, uint32_t* __restrict__ col,
                                                          uint32_t* __restrict__ val, const DevFilter f, const uint32_t* __restrict__ col_counts) {
    const uint32_t row = blockIdx.x;
    if (row >= nr) return;
    const uint32_t lane = threadIdx.x;
    const uint32_t* r = M + (uint64_t)row * nc;
    const unsigned char* fl = flags + (size_t)(row >> 6) * nbc;
    const uint32_t a = f.n ? f.counts[row] : 0u;               // the ROW sample's k-mer count
    unsigned long long out = COMPACT ? row_ptr[row] : 0ull;
    uint32_t count = 0;
    for (uint32_t Y0 = 0; Y0 < nbc; Y0 += 64u) {
        const uint32_t Yl = Y0 + lane;
        unsigned long long m = __ballot(Yl < nbc && fl[Yl] != 0);
        while (m) {
            const uint32_t Y = Y0 + (uint32_t)__builtin_ctzll(m);
            m &= m - 1;
            const uint32_t j = Y * 64u + lane;
            uint32_t v = j < nc ? r[j] : 0u;
            if (v && f.n && !dev_keep_ab(f, v, a, col_counts[j])) v = 0u;
            const unsigned long long bal = __ballot(v != 0);
            if (COMPACT) {
                if (v) { const unsigned long long o = out + (uint32_t)__popcll(bal & ((1ull << lane) - 1ull)); col[o] = j; val[o] = v; }
                out += (uint32_t)__popcll(bal);
            } else count += (uint32_t)__popcll(bal);
        }
    }
    if (!COMPACT && lane == 0) row_nnz[row] = count;
}

D2Db view_of(const kmdb_engine_view& e) {
    return D2Db{e.n_buckets, e.bucket_offset, e.slots, e.pid2dfs, e.meta, e.bitpos, e.parent, e.bits};
}

// the handle's list store (nullptr: this part does without one).  reserve: bytes the call still has to allocate after it (record pool,
// sort): a store that would leave less than that — or take more than a third of what is free — is not made (the part's pairs then climb)
const unsigned long long* d2_list_store(const kmdb_engine_view& e, hipStream_t st, uint64_t reserve) {
    if (*e.list_sets) return *e.list_sets;
    if (*e.list_sets_tried || !e.P) return nullptr;
    *e.list_sets_tried = true;
    if (getenv("KMDB_D2_NO_STORE")) return nullptr;
    const uint32_t nb = (uint32_t)((e.N + 63) / 64);
    const uint64_t bytes = e.P * nb * 8;
    if (nb > D2_SETS_MAX_NB || bytes > D2_SETS_MAX_BYTES || e.P >= (1ull << 31)) return nullptr;
    {
        size_t free_b = 0, total_b = 0;
        if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
        if (bytes + (e.P + 1) * 4 + reserve > free_b || bytes > free_b / 3) {
            if (getenv("KMDB_VERBOSE")) fprintf(stderr, "[kmdb] db2db: no list store (%.2f GB wanted, %.2f GB free, %.2f GB kept for the call)\n", bytes / 1e9, free_b / 1e9, reserve / 1e9);
            return nullptr;
        }
    }
    // (built in a local: the handle gets the store when it is complete, anything less frees itself)
    DevBuf<unsigned long long> sets;
    DevBuf<uint32_t> done;
    if (sets.alloc(e.P * nb) || done.alloc(e.P + 1)) { (void)hipGetLastError(); return nullptr; }
    bool ok = hipMemsetAsync(done, 0, (e.P + 1) * 4, st) == hipSuccess;
    const D2Db v = view_of(e);
    uint32_t filled = 0, round = 0;
    while (ok && filled < e.P && round < e.P + 1) {
        // max_depth rounds fill everything; the count is read back after them (and every 32 rounds after, if that was not so)
        const uint32_t upto = round ? round + 32u : std::max<uint32_t>(e.max_depth, 1u);
        for (; round < upto; ++round)
            hipLaunchKernelGGL(d2_sets_round_kernel, dim3((unsigned)((e.P + 255) / 256)), dim3(256), 0, st, v, (uint32_t)e.P, nb, round, done, sets, done + e.P);
        ok = hipGetLastError() == hipSuccess && hipMemcpyAsync(&filled, done + e.P, 4, hipMemcpyDeviceToHost, st) == hipSuccess && hipStreamSynchronize(st) == hipSuccess;
    }
    done.reset();
    if (!ok || filled != e.P) { (void)hipGetLastError(); return nullptr; }
    if (getenv("KMDB_VERBOSE")) fprintf(stderr, "[kmdb] db2db: list store of %llu patterns x %u words (%.2f GB) filled in %u rounds\n", (unsigned long long)e.P, nb, bytes / 1e9, round);
    *e.list_sets = std::move(sets); *e.list_sets_nb = nb; *e.device_bytes += bytes;
    return *e.list_sets;
}

}  // namespace

// what the sparse entry asks of the call (nullptr: the dense entry)
struct D2Sparse {
    const kmdb_cell_filter* filters;
    size_t n_filters;
    const uint32_t *row_kmers, *col_kmers;
    int measure;
    kmdb_sparse_rows* out;
    kmdb_csr_dev* keep;          // not null: the CSR stays in HBM (kmdb_db2db_csr_device), `out` is not filled and nothing is decided
};
// what the sampled entry asks of the call (nullptr: one of the other two)
struct D2Sampled {
    const kmdb_cell_filter* filters;
    size_t n_filters;
    const uint32_t *row_kmers, *col_kmers;
    int criterion;
    uint32_t count;
    kmdb_sparse_rows *out_row, *out_col;
};
static int db2db_impl(const char* who, kmdb_db* db_row, kmdb_db* db_col, uint32_t* out, const D2Sparse* sp, const D2Sampled* sm, const kmdb_opts* opts, bool allow_store);

// the call, and once more without the handles' list stores when it ran out of HBM
static int db2db_call(const char* who, kmdb_db* db_row, kmdb_db* db_col, uint32_t* out, const D2Sparse* sp, const D2Sampled* sm, const kmdb_opts* opts) {
    int rc = db2db_impl(who, db_row, db_col, out, sp, sm, opts, true);
    if (rc && std::strstr(kmdb_last_error(), hipGetErrorString(hipErrorOutOfMemory))) {
        // out of HBM inside the call: the handles' list stores (up to 8 GB each) are the part that can go — the pairs' lists are then built
        // by climbing, as on handles that never had a store — and the call is tried once more
        kmdb_engine_view er, ec;
        if (kmdb_engine_get(db_row, &er) || kmdb_engine_get(db_col, &ec)) return 1;
        bool freed = false;
        for (kmdb_engine_view* e : {&er, &ec})
            if (*e->list_sets) {
                (void)hipSetDevice(e->device);
                e->list_sets->reset();
                *e->device_bytes -= (uint64_t)e->P * *e->list_sets_nb * 8;
                *e->list_sets_nb = 0; *e->list_sets_tried = true;
                freed = true;
            }
        (void)hipGetLastError();
        if (freed) {
            if (getenv("KMDB_VERBOSE")) fprintf(stderr, "[kmdb] db2db: out of device memory; list stores dropped, the call is repeated on the climbing path\n");
            rc = db2db_impl(who, db_row, db_col, out, sp, sm, opts, false);
        }
    }
    return rc;
}

extern "C" int kmdb_db2db_dense(kmdb_db* db_row, kmdb_db* db_col, uint32_t* out, const kmdb_opts* opts) {
    if (!db_row || !db_col || !out) return kmdb_set_error("kmdb_db2db_dense: null argument");
    return db2db_call("kmdb_db2db_dense", db_row, db_col, out, nullptr, nullptr, opts);
}

extern "C" int kmdb_db2db_sparse_filtered(kmdb_db* db_row, kmdb_db* db_col, const kmdb_cell_filter* filters, size_t n_filters,
                                          const uint32_t* row_sample_kmers, const uint32_t* col_sample_kmers, int measure, kmdb_sparse_rows* out,
                                          const kmdb_opts* opts) {
    const char* who = "kmdb_db2db_sparse_filtered";
    if (!db_row || !db_col || !out) return kmdb_set_error(std::string(who) + ": null argument");
    // (bounds and measures need the k-mer counts of both sides: a = the row sample's, b = the column sample's)
    if (kmdb_check_filters(who, filters, n_filters, row_sample_kmers && col_sample_kmers ? row_sample_kmers : nullptr, measure)) return 1;
    std::memset(out, 0, sizeof *out);
    const D2Sparse sp{filters, n_filters, row_sample_kmers, col_sample_kmers, measure, out, nullptr};
    const int rc = db2db_call(who, db_row, db_col, nullptr, &sp, nullptr, opts);
    if (rc) kmdb_sparse_free(out);
    return rc;
}

int kmdb_db2db_csr_device(const char* who, kmdb_db* db_row, kmdb_db* db_col, kmdb_csr_dev* keep, const kmdb_opts* opts) {
    if (!db_row || !db_col || !keep) return kmdb_set_error(std::string(who) + ": null argument");
    const D2Sparse sp{nullptr, 0, nullptr, nullptr, -1, nullptr, keep};
    return db2db_call(who, db_row, db_col, nullptr, &sp, nullptr, opts);
}

extern "C" int kmdb_db2db_sampled(kmdb_db* db_row, kmdb_db* db_col, const kmdb_cell_filter* filters, size_t n_filters, const uint32_t* row_sample_kmers,
                                  const uint32_t* col_sample_kmers, int criterion, uint32_t count, kmdb_sparse_rows* out_row_candidates,
                                  kmdb_sparse_rows* out_col_candidates, const kmdb_opts* opts) {
    const char* who = "kmdb_db2db_sampled";
    if (!db_row || !db_col || !out_row_candidates || !out_col_candidates) return kmdb_set_error(std::string(who) + ": null argument");
    // (the proxy and the bounds need the k-mer counts of both sides: a = the row sample's, b = the column sample's)
    if (kmdb_check_sample_args(who, filters, n_filters, row_sample_kmers && col_sample_kmers ? row_sample_kmers : nullptr, criterion, count)) return 1;
    std::memset(out_row_candidates, 0, sizeof *out_row_candidates);
    std::memset(out_col_candidates, 0, sizeof *out_col_candidates);
    const D2Sampled sm{filters, n_filters, row_sample_kmers, col_sample_kmers, criterion, count, out_row_candidates, out_col_candidates};
    const int rc = db2db_call(who, db_row, db_col, nullptr, nullptr, &sm, opts);
    if (rc) { kmdb_sparse_free(out_row_candidates); kmdb_sparse_free(out_col_candidates); }
    return rc;
}

static int db2db_impl(const char* who_, kmdb_db* db_row, kmdb_db* db_col, uint32_t* out, const D2Sparse* sp, const D2Sampled* sm, const kmdb_opts* opts, bool allow_store) {
    const std::string who(who_);
    kmdb_engine_view er, ec;
    if (kmdb_engine_get(db_row, &er)) return 1;
    if (kmdb_engine_get(db_col, &ec)) return 1;
    if (!er.n_buckets || !er.slots || !ec.n_buckets || !ec.slots)
        return kmdb_set_error(who + ": both databases must be uploaded with hashtables");
    if (er.qs_count > 1 || ec.qs_count > 1) return kmdb_set_error(who + ": a query shard holds only its own buckets (upload the parts with kmdb_db_upload)");
    if (er.kmer_length != ec.kmer_length) return kmdb_set_error(who + ": the databases have different k-mer lengths");
    if (er.device != ec.device) return kmdb_set_error(who + ": the databases live on different devices");
    // (sample ids take 20 bits here as everywhere: round 4's limit of 65 535 samples per part — a 16-bit block index array of fixed size in the
    // pair kernel — is gone; what bounds a part now is the pair kernel's LDS and the 2^22 block pairs of the stream keys, checked below)
    HIP_TRY(hipSetDevice(er.device));
    hipStream_t st = (opts && opts->stream) ? (hipStream_t)opts->stream : (hipStream_t)er.stream;
    const uint64_t nr = er.N, nc = ec.N;
    if (sm && kmdb_sample_rect_check(who_, nr, nc)) return 1;
    uint64_t n_slots = 0;
    HIP_TRY(hipMemcpy(&n_slots, ec.bucket_offset + ec.n_buckets, 8, hipMemcpyDeviceToHost));
    if (n_slots >= (1ull << 31)) return kmdb_set_error(who + ": column database has more than 2^31 hashtable slots");
    DevBuf<void> d_keys, d_keys2, d_uniq, d_cnt, d_nruns, d_out, d_tmp, d_flag;
    DEV_ALLOC_BYTES(d_keys, n_slots * 8); DEV_ALLOC_BYTES(d_keys2, n_slots * 8); DEV_ALLOC_BYTES(d_uniq, (n_slots + 1) * 8);
    DEV_ALLOC_BYTES(d_cnt, (n_slots + 1) * 4); DEV_ALLOC_BYTES(d_nruns, 16); DEV_ALLOC_BYTES(d_out, nr * nc * 4); DEV_ALLOC_BYTES(d_flag, 16);
    HIP_TRY(hipMemsetAsync(d_out.get(), 0, std::max<uint64_t>(nr * nc * 4, 4), st));
    HIP_TRY(hipMemsetAsync(d_flag.get(), 0, 16, st));
    // the cell in tiles of 64 x 64; sparse and sampled entries: one flag byte per tile (KMDB_SP_ALL_TILES=1: every tile counts as touched, as for all2all-sp — A/B)
    const uint32_t nbr = (uint32_t)((nr + 63) / 64), nbc = (uint32_t)((nc + 63) / 64);
    const uint64_t n_tiles = (uint64_t)nbr * nbc;
    const bool tile_flags = sp || sm;
    const bool all_tiles = tile_flags && getenv("KMDB_SP_ALL_TILES");
    bool any_records = false, flags_timed = false;
    DevBuf<void> d_tiles;
    if (tile_flags) {
        DEV_ALLOC_BYTES(d_tiles, n_tiles);
        HIP_TRY(hipMemsetAsync(d_tiles.get(), all_tiles ? 1 : 0, std::max<uint64_t>(n_tiles, 1), st));
    }
    hipEvent_t ev0 = (hipEvent_t)er.ev[0], ev1 = (hipEvent_t)er.ev[1], ev2 = (hipEvent_t)er.ev[2], ev3 = (hipEvent_t)er.ev[3];
    HIP_TRY(hipEventRecord(ev0, st));
    const bool verbose = getenv("KMDB_VERBOSE") != nullptr;
    auto t_mark = std::chrono::steady_clock::now();
    auto phase = [&](const char* what) {                          // KMDB_VERBOSE: host-side wall time of the call's steps (each one waited for)
        if (!verbose) return;
        (void)hipStreamSynchronize(st);
        const auto now = std::chrono::steady_clock::now();
        fprintf(stderr, "[kmdb] db2db: %-34s %.3f ms\n", what, std::chrono::duration<double, std::milli>(now - t_mark).count());
        t_mark = now;
    };
    // bits of a key: 2^cbits > patterns of the column database, 2^rbits > patterns of the row database (so no key in use is all ones
    // in the sorted bits: the unused slots' ~0 sorts last)
    uint32_t cbits = 1, rbits = 1;
    while ((1ull << cbits) <= ec.P) ++cbits;
    while ((1ull << rbits) <= er.P) ++rbits;
    const unsigned key_end = std::min<unsigned>(64u, cbits + rbits);
    if (n_slots && nr && nc) {
        size_t tb_sort = 0, tb_rle = 0;
        HIP_TRY(prim::sort_keys(nullptr, tb_sort, static_cast<unsigned long long*>(d_keys.get()), static_cast<unsigned long long*>(d_keys2.get()),
                                                 (int)n_slots, 0, key_end, st));
        HIP_TRY(prim::run_length_encode(nullptr, tb_rle, static_cast<unsigned long long*>(d_keys2.get()), static_cast<unsigned long long*>(d_uniq.get()),
                                                     static_cast<uint32_t*>(d_cnt.get()), static_cast<uint32_t*>(d_nruns.get()), (int)n_slots, st));
        DEV_ALLOC_BYTES(d_tmp, std::max(tb_sort, tb_rle));
        const D2Db vr = view_of(er), vc = view_of(ec);
        hipLaunchKernelGGL(d2_probe_kernel, dim3((unsigned)((n_slots + 255) / 256)), dim3(256), 0, st, vr, vc, n_slots, cbits,
                           static_cast<unsigned long long*>(d_keys.get()));
        HIP_TRY(hipGetLastError());
        HIP_TRY(prim::sort_keys(d_tmp.get(), tb_sort, static_cast<unsigned long long*>(d_keys.get()), static_cast<unsigned long long*>(d_keys2.get()),
                                                 (int)n_slots, 0, key_end, st));
        HIP_TRY(prim::run_length_encode(d_tmp.get(), tb_rle, static_cast<unsigned long long*>(d_keys2.get()), static_cast<unsigned long long*>(d_uniq.get()),
                                                     static_cast<uint32_t*>(d_cnt.get()), static_cast<uint32_t*>(d_nruns.get()), (int)n_slots, st));
        uint32_t nruns = 0;
        HIP_TRY(hipMemcpyAsync(&nruns, d_nruns.get(), 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        if (nruns) {                                              // the slots without a hit are ONE run, the last (~0 sorts behind every key in use): no pattern pair
            unsigned long long last_key = 0;
            HIP_TRY(hipMemcpy(&last_key, static_cast<unsigned long long*>(d_uniq.get()) + (nruns - 1), 8, hipMemcpyDeviceToHost));
            if (last_key == D2_INVALID) --nruns;
        }
        phase("probe + sort + run lengths");
        if (nruns) {
            // pairs -> block records -> sorted by block pair -> accumulated on the matrix cores (a2a_blocks.hip)
            int key_bits = 1;
            while ((1ull << key_bits) <= (uint64_t)nbr * nbc + 1) ++key_bits;
            const uint32_t dbits = (uint32_t)(32 - key_bits - 2);
            if ((uint64_t)nbr * nbc + 1 >= (1ull << 22)) return kmdb_set_error(who + ": more than 2^22 block pairs (parts of " + std::to_string(nr) + " x " + std::to_string(nc) + " samples)");
            const size_t wave_lds = d2_wave_words(nbr, nbc) * 8;
            if (wave_lds > (size_t)(150u << 10)) return kmdb_set_error(who + ": the sample lists of a pattern pair do not fit the LDS (parts of " + std::to_string(nr) + " + " + std::to_string(nc) + " samples; about 540 000 in all is the limit)");
            const uint32_t wpb = (uint32_t)std::max<size_t>(1, std::min<size_t>(4, (size_t)(150u << 10) / wave_lds));
            const uint32_t grid = (uint32_t)std::min<uint64_t>(((uint64_t)nruns + wpb - 1) / wpb, 256 * 8);
            const size_t lds = wave_lds * wpb;
            // both parts' list stores, or neither (a wave that climbs one side's root paths gains nothing from the other's store)
            // (what the call allocates after the stores: six records of 20 bytes per pair, twice — the pool and the sort's copy — and slack)
            const uint64_t reserve = (uint64_t)nruns * 6 * 20 * 2 + (1ull << 30);
            const unsigned long long* rsets = allow_store ? d2_list_store(er, st, reserve) : nullptr;
            const unsigned long long* csets = rsets ? (db_col == db_row ? rsets : d2_list_store(ec, st, reserve)) : nullptr;
            const bool store = rsets && csets;
            phase("list stores");
            DevBuf<void> d_nrec, d_cursor;
            DEV_ALLOC_BYTES(d_nrec, 64 * 8 * 8); DEV_ALLOC_BYTES(d_cursor, D2_CURSORS * 16 * 4);
            HIP_TRY(hipMemsetAsync(d_nrec.get(), 0, 64 * 8 * 8, st));
            HIP_TRY(hipMemsetAsync(d_cursor.get(), 0, D2_CURSORS * 16 * 4, st));
            D2Pool pool{nullptr, nullptr, static_cast<uint32_t*>(d_cursor.get()), 0u, (uint32_t)key_bits, dbits, static_cast<uint32_t*>(d_flag.get()) + 1};
            HIP_TRY(hipFuncSetAttribute((const void*)d2_emit_kernel<true, false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
            HIP_TRY(hipFuncSetAttribute((const void*)d2_emit_kernel<false, false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
            HIP_TRY(hipFuncSetAttribute((const void*)d2_emit_kernel<true, true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
            HIP_TRY(hipFuncSetAttribute((const void*)d2_emit_kernel<false, true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
            // the pool: sized for six records per pair first; if that overflows, the
            // records are counted and the pool is made to measure
            DevBuf<void> d_wkey, d_wrec;
            uint64_t slots = 0;
            for (int attempt = 0; attempt < 2; ++attempt) {
                unsigned long long total = 6ull * nruns;
                if (attempt) {
                    HIP_TRY(hipMemsetAsync(d_nrec.get(), 0, 64 * 8 * 8, st));
                    if (store)
                        hipLaunchKernelGGL((d2_emit_kernel<true, true>), dim3(grid), dim3(64 * wpb), lds, st, vr, vc, rsets, csets, static_cast<unsigned long long*>(d_uniq.get()), static_cast<uint32_t*>(d_cnt.get()),
                                           nruns, nbr, nbc, cbits, pool, static_cast<unsigned long long*>(d_nrec.get()));
                    else
                        hipLaunchKernelGGL((d2_emit_kernel<true, false>), dim3(grid), dim3(64 * wpb), lds, st, vr, vc, rsets, csets, static_cast<unsigned long long*>(d_uniq.get()), static_cast<uint32_t*>(d_cnt.get()),
                                           nruns, nbr, nbc, cbits, pool, static_cast<unsigned long long*>(d_nrec.get()));
                    HIP_TRY(hipGetLastError());
                    unsigned long long h_nrec[64 * 8];
                    HIP_TRY(hipMemcpyAsync(h_nrec, d_nrec.get(), sizeof h_nrec, hipMemcpyDeviceToHost, st));
                    HIP_TRY(hipStreamSynchronize(st));
                    total = 0;
                    for (int q = 0; q < 64; ++q) total += h_nrec[q * 8];
                }
                // per cursor: its share of the records and of the grab tails (up to 63 slots per grab), one unfinished grab per wave
                // that ends there, and room for the uneven ends of the waves' round-robin over the cursors
                const uint64_t grabs = (total + total / 8) / D2_GRAB / D2_CURSORS + (uint64_t)grid * wpb / D2_CURSORS + 130;
                const uint64_t region = grabs * D2_GRAB;
                slots = region * D2_CURSORS;
                if (slots >= (1ull << 31)) return kmdb_set_error(who + ": more than 2^31 block records");
                dev_reset(d_wkey, d_wrec);                      // (a second round: the old pool goes before the larger one comes)
                DEV_ALLOC_BYTES(d_wkey, slots * 4); DEV_ALLOC_BYTES(d_wrec, slots * 16);
                HIP_TRY(hipMemsetAsync(d_wkey.get(), 0xFF, slots * 4, st));
                HIP_TRY(hipMemsetAsync(d_cursor.get(), 0, D2_CURSORS * 16 * 4, st));
                HIP_TRY(hipMemsetAsync(static_cast<uint32_t*>(d_flag.get()) + 1, 0, 4, st));
                pool.wkey = static_cast<uint32_t*>(d_wkey.get()); pool.wrec = static_cast<ulonglong2*>(d_wrec.get()); pool.region = (uint32_t)region;
                if (store)
                    hipLaunchKernelGGL((d2_emit_kernel<false, true>), dim3(grid), dim3(64 * wpb), lds, st, vr, vc, rsets, csets, static_cast<unsigned long long*>(d_uniq.get()), static_cast<uint32_t*>(d_cnt.get()),
                                       nruns, nbr, nbc, cbits, pool, static_cast<unsigned long long*>(d_nrec.get()));
                else
                    hipLaunchKernelGGL((d2_emit_kernel<false, false>), dim3(grid), dim3(64 * wpb), lds, st, vr, vc, rsets, csets, static_cast<unsigned long long*>(d_uniq.get()), static_cast<uint32_t*>(d_cnt.get()),
                                       nruns, nbr, nbc, cbits, pool, static_cast<unsigned long long*>(d_nrec.get()));
                HIP_TRY(hipGetLastError());
                uint32_t ovf = 0;
                HIP_TRY(hipMemcpyAsync(&ovf, static_cast<uint32_t*>(d_flag.get()) + 1, 4, hipMemcpyDeviceToHost, st));
                HIP_TRY(hipStreamSynchronize(st));
                if (getenv("KMDB_VERBOSE")) fprintf(stderr, "[kmdb] db2db: %u pattern pairs, pool for %llu records (%s)%s\n", nruns, total, attempt ? "counted" : "estimate", ovf ? ": too small" : "");
                if (!ovf) break;
                if (attempt) return kmdb_set_error(who + ": internal error (record pool overflow)");
            }
            phase("pool + emit");
            any_records = true;
            if (tile_flags && !all_tiles) {
                // the tiles this call adds to, from the pool's key words (before the sort takes the pool)
                HIP_TRY(hipEventRecord(ev1, st));
                hipLaunchKernelGGL(d2_tile_flags_kernel, dim3((unsigned)((slots + 255) / 256)), dim3(256), 0, st, static_cast<uint32_t*>(d_wkey.get()), (uint32_t)slots,
                                   (1u << key_bits) - 1u, (uint32_t)n_tiles, static_cast<unsigned char*>(d_tiles.get()));
                HIP_TRY(hipGetLastError());
                HIP_TRY(hipEventRecord(ev2, st));
                flags_timed = true;
            }
            if (kmdb_rect_sort_apply(st, static_cast<uint32_t*>(d_wkey.get()), d_wrec.get(), (uint32_t)slots, nbr, nbc, key_bits, static_cast<uint32_t*>(d_out.get()), (uint32_t)nr, (uint32_t)nc)) return 1;
            phase("sort + apply");
        }
    }
    kmdb_db2db_stats& ds = *er.d2_stats;
    ds = kmdb_db2db_stats{};
    ds.tiles = n_tiles;
    if (sm) {
        // ---- the sampled entry: the cell stays in d_out and the select reads its flagged tiles there (a cell without a single block record has
        // no flagged tile: every line comes out empty)
        std::vector<unsigned char> h_tiles(n_tiles, 0);
        if (n_tiles) HIP_TRY(hipMemcpyAsync(h_tiles.data(), d_tiles.get(), n_tiles, hipMemcpyDeviceToHost, st));
        kmdb_sample_stats ss{};
        *er.d2_sample_stats = ss;
        if (kmdb_sample_rect(who_, st, (int)er.kmer_length, static_cast<uint32_t*>(d_out.get()), nr, nc, static_cast<unsigned char*>(d_tiles.get()), sm->filters,
                             sm->n_filters, sm->row_kmers, sm->col_kmers, sm->criterion, sm->count, sm->out_row, sm->out_col, &ss)) return 1;
        HIP_TRY(hipEventRecord(ev3, st));
        HIP_TRY(hipEventSynchronize(ev3));
        float ms = 0, ms_flags = 0;
        HIP_TRY(hipEventElapsedTime(&ms, ev0, ev3));
        if (flags_timed) HIP_TRY(hipEventElapsedTime(&ms_flags, ev1, ev2));
        kmdb_engine_set_times(db_row, ms, ms);
        uint32_t too_long = 0;
        HIP_TRY(hipMemcpy(&too_long, d_flag.get(), 4, hipMemcpyDeviceToHost));
        if (too_long) return kmdb_set_error(who + ": internal error");
        for (unsigned char t : h_tiles) ds.tiles_touched += t != 0;
        ss.select_ms += (double)ms_flags;
        ds.nnz_device = ds.nnz = ss.candidates;
        ds.d2h_bytes = ss.d2h_bytes;
        ds.compact_ms = ss.select_ms;
        *er.d2_sample_stats = ss;
        return 0;
    }
    if (!sp) {
        HIP_TRY(hipEventRecord(ev3, st));
        HIP_TRY(hipEventSynchronize(ev3));
        float ms = 0;
        HIP_TRY(hipEventElapsedTime(&ms, ev0, ev3));
        kmdb_engine_set_times(db_row, ms, ms);
        uint32_t too_long = 0;
        HIP_TRY(hipMemcpy(&too_long, d_flag.get(), 4, hipMemcpyDeviceToHost));
        if (too_long) return kmdb_set_error(who + ": internal error");
        if (nr * nc) HIP_TRY(hipMemcpy(out, d_out.get(), nr * nc * 4, hipMemcpyDeviceToHost));
        ds.d2h_bytes = nr * nc * 4;
        return 0;
    }
    // ---- the sparse entry: the cell stays in d_out and is compacted there (count per row, exclusive sum, (col, val) in ascending columns)
    DevEvent c0, c1;
    if (c0.create()) return 1; if (c1.create()) return 1;
    DevBuf<void> d_nnz, d_ptr, d_col, d_val, d_rk, d_ck, d_scan;
    DevFilter df{};
    if (sp->n_filters) {
        DEV_ALLOC_BYTES(d_rk, nr * 4); DEV_ALLOC_BYTES(d_ck, nc * 4);
        if (nr) HIP_TRY(hipMemcpyAsync(d_rk.get(), sp->row_kmers, nr * 4, hipMemcpyHostToDevice, st));
        if (nc) HIP_TRY(hipMemcpyAsync(d_ck.get(), sp->col_kmers, nc * 4, hipMemcpyHostToDevice, st));
        df.n = (int)sp->n_filters; df.counts = static_cast<uint32_t*>(d_rk.get());
        kmdb_dev_bounds(sp->filters, sp->n_filters, (int)er.kmer_length, df.kind, df.lo, df.hi);
    }
    DEV_ALLOC_BYTES(d_nnz, (nr + 1) * 8); DEV_ALLOC_BYTES(d_ptr, (nr + 1) * 8);
    // (a cell without a single block record has no tile to read: its counts stay zero)
    const bool scan = nr && nc && (any_records || all_tiles);
    HIP_TRY(hipEventRecord(c0, st));
    HIP_TRY(hipMemsetAsync(d_nnz.get(), 0, (nr + 1) * 8, st));
    if (scan) {
        hipLaunchKernelGGL((d2_row_tiles_kernel<false>), dim3((unsigned)nr), dim3(64), 0, st, static_cast<uint32_t*>(d_out.get()), (uint32_t)nr, (uint32_t)nc, nbc,
                           static_cast<unsigned char*>(d_tiles.get()), static_cast<unsigned long long*>(d_nnz.get()), (const unsigned long long*)nullptr, (uint32_t*)nullptr,
                           (uint32_t*)nullptr, df, static_cast<uint32_t*>(d_ck.get()));
        HIP_TRY(hipGetLastError());
    }
    size_t scan_bytes = 0;
    HIP_TRY(prim::exclusive_sum(nullptr, scan_bytes, static_cast<unsigned long long*>(d_nnz.get()), static_cast<unsigned long long*>(d_ptr.get()), (size_t)(nr + 1), st));
    DEV_ALLOC_BYTES(d_scan, scan_bytes);
    HIP_TRY(prim::exclusive_sum(d_scan.get(), scan_bytes, static_cast<unsigned long long*>(d_nnz.get()), static_cast<unsigned long long*>(d_ptr.get()), (size_t)(nr + 1), st));
    std::vector<unsigned long long> h_ptr(nr + 1, 0);
    std::vector<unsigned char> h_tiles(n_tiles, 0);
    HIP_TRY(hipMemcpyAsync(h_ptr.data(), d_ptr.get(), (nr + 1) * 8, hipMemcpyDeviceToHost, st));
    if (n_tiles) HIP_TRY(hipMemcpyAsync(h_tiles.data(), d_tiles.get(), n_tiles, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    const uint64_t nnz_dev = h_ptr[nr];
    DEV_ALLOC_BYTES(d_col, nnz_dev * 4); DEV_ALLOC_BYTES(d_val, nnz_dev * 4);
    if (scan && nnz_dev) {
        hipLaunchKernelGGL((d2_row_tiles_kernel<true>), dim3((unsigned)nr), dim3(64), 0, st, static_cast<uint32_t*>(d_out.get()), (uint32_t)nr, (uint32_t)nc, nbc,
                           static_cast<unsigned char*>(d_tiles.get()), (unsigned long long*)nullptr, static_cast<unsigned long long*>(d_ptr.get()), static_cast<uint32_t*>(d_col.get()),
                           static_cast<uint32_t*>(d_val.get()), df, static_cast<uint32_t*>(d_ck.get()));
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipEventRecord(c1, st));
    HIP_TRY(hipEventRecord(ev3, st));
    HIP_TRY(hipEventSynchronize(ev3));
    float ms = 0, ms_flags = 0, ms_compact = 0;
    HIP_TRY(hipEventElapsedTime(&ms, ev0, ev3));
    HIP_TRY(hipEventElapsedTime(&ms_compact, c0, c1));
    if (flags_timed) HIP_TRY(hipEventElapsedTime(&ms_flags, ev1, ev2));
    kmdb_engine_set_times(db_row, ms, ms);
    uint32_t too_long = 0;
    HIP_TRY(hipMemcpy(&too_long, d_flag.get(), 4, hipMemcpyDeviceToHost));
    if (too_long) return kmdb_set_error(who + ": internal error");
    for (unsigned char t : h_tiles) ds.tiles_touched += t != 0;
    ds.nnz_device = nnz_dev;
    ds.compact_ms = (double)ms_flags + (double)ms_compact;
    if (sp->keep) {                                               // the CSR stays where it is: nothing crosses, nothing is decided here
        sp->keep->row_ptr = std::move(d_ptr); sp->keep->col = std::move(d_col); sp->keep->val = std::move(d_val);
        sp->keep->n_rows = nr; sp->keep->nnz = nnz_dev;
        ds.nnz = nnz_dev;
        return 0;
    }
    kmdb_sparse_rows* o = sp->out;
    o->n_rows = nr;
    o->nnz = nnz_dev;
    o->row_ptr = (uint64_t*)std::malloc((nr + 1) * 8);
    o->col = (uint32_t*)std::malloc(std::max<uint64_t>(nnz_dev, 1) * 4);
    o->val = (uint32_t*)std::malloc(std::max<uint64_t>(nnz_dev, 1) * 4);
    if (!o->row_ptr || !o->col || !o->val) return kmdb_set_error(who + ": out of host memory for the result");
    for (uint64_t i = 0; i <= nr; ++i) o->row_ptr[i] = h_ptr[i];
    if (nnz_dev) {
        HIP_TRY(hipMemcpy(o->col, d_col.get(), nnz_dev * 4, hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(o->val, d_val.get(), nnz_dev * 4, hipMemcpyDeviceToHost));
    }
    ds.d2h_bytes = (nr + 1) * 8 + nnz_dev * 8;
    // the exact decision: every cell the widened bounds let through, by the reference's arithmetic (a = row sample, b = column sample)
    if ((sp->n_filters || sp->measure >= 0) &&
        kmdb_sparse_decide(who_, o, sp->filters, sp->n_filters, sp->row_kmers, sp->col_kmers, sp->measure, (int)er.kmer_length)) return 1;
    ds.nnz = o->nnz;
    if (verbose)
        fprintf(stderr, "[kmdb] db2db: sparse cell: %llu of %llu tiles touched, %llu cells left the device, %llu kept, compaction %.3f ms\n",
                (unsigned long long)ds.tiles_touched, (unsigned long long)ds.tiles, (unsigned long long)ds.nnz_device, (unsigned long long)ds.nnz, ds.compact_ms);
    return 0;
}
