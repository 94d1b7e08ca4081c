// a2a_blocks.hip — the block-record pipeline of the dense all2all path (the whole matrix: up to about 185 000 samples, 2^22 block pairs;
// a band of rows under band emit: fewer than 2^22 streams per BAND, keyed relative to it).
//
// Replaces SimilarityCalculator::all2all (reference src/similarity_calculator.cpp:42-438, inner loop row_add
// src/simd/row_add_avx2.cpp:30-124) with a design for gfx950.  The N x N matrix is cut into blocks (X, Y), X >= Y,
// of `width` <= 64 consecutive sample ids.  A pattern's ascending id list meets a block in a contiguous run, so
// all pair updates of a pattern with weight w factor into BLOCK RECORDS
//        (X, Y, rowmask, colmask, w):   M[width*X + r][width*Y + c] += w   for r in rowmask, c in colmask
//                                                                            (c < r when X == Y).
// Flat form (all2all_sp semantics, reference similarity_calculator.cpp:596-638): every pattern with w > 0 adds its
// on-disk w to all pairs of its FULL list, i.e. one record per pair of blocks X >= Y the full list touches.
//
// Everything that depends on a decoded sample id happens inside the call (kmdb_blocks_run):
//   K0  k0_decode_kernel x2  gamma streams -> the LOCAL ids of every node as (block, 64-bit mask) pairs (thread per node; the
//                            nodes with long streams in a second launch, most work first)
//   K1n k1n_kernel           walks the DFS stream in slices of 2048 nodes, 64 nodes per wave step, one lane each.  A full list is
//                            the union of the local lists on the root path and ids ascend along it, so the list of a node with
//                            at most TWO blocks is a summary of five registers; in-batch parents by pointer doubling across
//                            lanes, earlier ones from a chain table in LDS (one slot per depth).  Emits the records of those
//                            nodes (first-block diagonal records into per-block stream chunks, the others into the wide pool),
//                            flags the nodes with more blocks and leaves them their parent's summary.
//                            The first-block records (X, X) of a slice: compacted per slice and applied by k2d_kernel on the side
//                            stream (KMDB_K1N_MODE=2, default), applied inside the kernel (1), or written to stream chunks (0).
//       wide list            the flagged nodes, compacted: the narrow kernel counts them per word and slice, wide_slices_kernel (one
//                            workgroup) scans the slices, wide_expand_kernel writes the list
//   K1w k1w_kernel           the wide nodes in runs of 256 (root paths of the runs' first nodes: wrun_anc_kernel): list = parent's
//                            list + own pairs, records into the wide pool (few streams) or per-block-row chunks (many streams);
//                            many streams with at most 256 blocks: the nodes with many blocks go to the second level instead
//                            (l2_ranks / l2_offsets / l2_lists / l2_join_apply_kernel join two blocks' lists per tile)
//   sort few streams (<= 2048): cs_hist / cs_scatter_kernel, ONE counting-sort pass over the wide pool by stream (per-workgroup
//                            LDS histograms, staged tiles).  Many streams: the chunk table grouped by key (ct_hist / ct_scatter), the
//                            row chunks grouped by row (rg_hist / rg_scatter), then a counting sort inside every block row
//                            (rs_rows / rs_hist / rs_scatter_kernel).
//   K2  k2_apply_kernel      stream chunks (side stream, next to K1w); k2j_starts[_flat] / k2j_build / k2_jobs_kernel: the sorted
//                            records stream by stream.  64 records per wave step as bit matrices, int8 MFMA into a 64 x 64 LDS tile
//                            (weights >= 128 as base-128 digit passes), one HBM atomic per non-zero cell.
// A band of rows (kmdb_blocks_run with a kmdb_band_desc; a2a_rows_records.hip): K0, K1n, K1w and the sorts run as above, the K2 stage takes its
//                            BAND instantiations (k2d_band_kernel, k2_apply_kernel<true>, k2_jobs_kernel<true>, l2_join_apply_kernel<true>): the units
//                            of block rows outside the band are culled, the write-back is windowed to the band's rows and based on its first cell.
// Band emit (kmdb_band_desc::emit; the handle's second state, kmdb_blocks_band_prepare): K1n and K1w take their BAND instantiations (k1n_band_kernel,
//                            k1w_band_kernel) and emit the records of the band's block rows [Xlo, Xhi] alone, keyed tri32(X) - tri32(Xlo) + Y; the sorts, the stream
//                            jobs and the second level's tiles run over the band's tri32(Xhi + 1) - tri32(Xlo) streams, everything indexed by block row holds
//                            Xhi - Xlo + 1 rows, and every consumer that turns a key back into (X, Y) adds the base first (band_stream, RsRows::sbase).
// db2db (kmdb_rect_sort_apply) shares cs_hist / cs_scatter and applies its sorted records with k2_sorted_kernel.
// Records are placed WITHOUT a counting pass and WITHOUT hot global atomics (same-address device atomics run at a few million
// per second on this part: measured, profiles/README.md): waves take chunks from 256 sub-pool cursors a few at a time, keep
// their open stream chunks in an LDS table indexed by block, and reserve slots for a group of lanes with a ballot.  The pools are
// sized from a sampled estimate; a pool that turns out too small is enlarged and the call repeated.
#include "device_common.h"
#include "engine_internal.h"

#include "prim.h"

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <memory>
#include <string>

// counters of the block-record pipeline, zeroed at the start of every call and read back at its end
enum : uint32_t {
    KCTR_CHUNKS = 0,        // record chunks opened
    KCTR_POOL_OVERFLOW,     // != 0: the chunk pool was too small (results invalid; the call is repeated with a larger pool)
    KCTR_PAIR_OVERFLOW,     // != 0: the pool of extra (block, mask) pairs was too small
    KCTR_NWIDE,             // nodes whose full list touches more than two blocks
    KCTR_LIST_OVERFLOW,     // != 0: a wide node's path did not fit the per-wave entry pool
    KCTR_RAW = 5,           // chunks of the wide pool in use (upper bound: busiest sub-pool x sub-pools)
    KCTR_RECORDS = 6,       // low word of the number of block records written (64-bit atomic: even index)
    KCTR_RECORDS_HI = 7,
    KCTR_SLOW = 8,          // wide nodes that took the climbing path
    KCTR_WIDE_OVERFLOW = 9, // != 0: the wide record pool was too small
    KCTR_WIDE_RECORDS = 10, // records written to the wide pool
    KCTR_ROWJOBS = 11,      // row mode: workgroups of the sort inside the block rows
    KCTR_L2_OVERFLOW = 12,  // != 0: the second level's node indices or entries ran out (results invalid; repeated with larger arrays)
    KCTR_L2_NODES = 13,     // nodes that went to the second level
    KCTR_POOL_USED = 15,    // chunks of the chunk pool in use (upper bound: busiest sub-pool x sub-pools)
    KCTR_K2JOBS = 14,       // row mode: jobs of the apply kernel over the sorted records (one stream, or one part of a long stream, each)
    KCTR_DIRECT = 16,       // first-block records the narrow kernel applied where it emitted them (never written: k1n_kernel<true>)
    KCTR_COUNT = 17
};
constexpr uint32_t KMDB_PAIR_REGIONS = 4096;   // sub-pools of the extra-pair pool (one allocation cursor each)
constexpr uint32_t KMDB_SUBPOOLS = 256;      // sub-pools of the record chunk pool (one allocation cursor each)

namespace {

__host__ __device__ __forceinline__ uint32_t tri32(uint32_t x) { return x * (x + 1u) / 2u; }

// A band of the matrix's rows as the write-back sites of the apply stage see it (kmdb_all2all_rows_records_device): M then points at cell
// tri64(row_lo) of the triangle, the band's first, and holds the rows [row_lo, row_hi) only.  [Xlo, Xhi] are the block rows the band meets: a
// stream job, a window run, a slice's tile or a second-level tile of another block row is culled (no matrix-core step, no write-back), and a cell
// of a block row that lies half inside is written iff its row is one of the band's, at tri64(row) - cell_lo + col.  units: 64 slots of BAND_UNIT_WORDS
// words, a slot per workgroup (mod 64) so that no counter is hot: BU_* of every apply unit the call met and of those it ran (the call's statistics).
// The whole-matrix instantiations (BAND = false) take BandArg<false>, which is empty: nothing of this reaches them.
struct BandWin { uint32_t row_lo, row_hi, Xlo, Xhi; uint64_t cell_lo; uint32_t* units; uint32_t sbase; };
template <bool BAND> struct BandArg {};
template <> struct BandArg<true> { BandWin w; };
enum : uint32_t { BU_JOBS = 0, BU_JOBS_RUN, BU_RUNS, BU_RUNS_RUN, BU_SLICES, BU_SLICES_RUN, BU_TILES, BU_TILES_RUN, BU_COUNT };
constexpr uint32_t BAND_UNIT_SLOTS = 64, BAND_UNIT_WORDS = 32;      // (a slot is one 128-byte line)
__device__ __forceinline__ bool band_culls(const BandWin& w, uint32_t X) { return X < w.Xlo || X > w.Xhi; }
// the stream a key names: band emit (kmdb_band_desc::emit) keys its records relative to the band's first stream, sbase = tri32(Xlo); every other call: 0
__device__ __forceinline__ uint32_t band_stream(const BandArg<false>&, uint32_t key) { return key; }
__device__ __forceinline__ uint32_t band_stream(const BandArg<true>& b, uint32_t key) { return key + b.w.sbase; }
__device__ __forceinline__ void band_unit(const BandWin& w, uint32_t slot, uint32_t kind, bool ran) {
    uint32_t* c = w.units + (size_t)(slot & (BAND_UNIT_SLOTS - 1u)) * BAND_UNIT_WORDS;
    atomicAdd(c + kind, 1u);
    if (ran) atomicAdd(c + kind + 1u, 1u);
}

// Workgroups are dealt to the eight XCDs round-robin (workgroup b runs on XCD b % 8), and every XCD has its own L2.  Where neighbouring
// work items write neighbouring memory (the sort kernels: consecutive jobs fill adjacent stretches of every stream, the cache lines at
// the seams are shared), item = xcd_contiguous(b, n) keeps every XCD on ONE contiguous range of items, so that a line is completed in
// one L2 instead of leaving two of them half written.  n must be a multiple of 8 (the launches round up).
constexpr uint32_t RS_XCD_MAP = 1;          // 0: items in workgroup order (A/B)
__device__ __forceinline__ uint32_t xcd_contiguous(uint32_t b, uint32_t n) {
    if (!RS_XCD_MAP) return b;
    return (b & 7u) * (n >> 3) + (b >> 3);
}

// A kernel's parameter block where it lies in the kernarg segment (the kernel's only argument: offset 0), behind a pointer the compiler cannot see
// through.  What is read through it is loaded where it is used (a scalar load, from the constant cache) instead of being held in scalar registers across
// the loops from the kernel's start: the emit kernels take some twenty pointers, most of them read once per batch of 64 nodes or once per run.
#define KARG(P) const P __attribute__((address_space(4)))*
template <class P> __device__ __forceinline__ KARG(P) kernarg_reread() {
    KARG(P) p = (KARG(P))__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(p));
    return p;
}

__device__ __forceinline__ unsigned long long shfl64(unsigned long long v, int src) {
    const uint32_t lo = (uint32_t)__shfl((int)(uint32_t)v, src, WAVE);
    const uint32_t hi = (uint32_t)__shfl((int)(uint32_t)(v >> 32), src, WAVE);
    return ((unsigned long long)hi << 32) | lo;
}
__device__ __forceinline__ unsigned long long shfl_up64(unsigned long long v, int d) {
    const uint32_t lo = (uint32_t)__shfl_up((int)(uint32_t)v, d, WAVE);
    const uint32_t hi = (uint32_t)__shfl_up((int)(uint32_t)(v >> 32), d, WAVE);
    return ((unsigned long long)hi << 32) | lo;
}

// ------------------------------------------------------------------------------------------
// record pool
// ------------------------------------------------------------------------------------------
constexpr uint32_t CH_SHIFT = 8, CH_REC = 1u << CH_SHIFT;      // records per stream chunk: four wave steps of K2, 4 KB contiguous
constexpr uint32_t WCH_SHIFT = 6, WCH_REC = 1u << WCH_SHIFT;   // records per chunk of the wide pool (grouped by a sort, not by chunk)
// Record of the wide pool: 16 bytes of masks, moved by the sort next to its 4-byte key word.  The key word holds the stream in
// its low `kbits` bits, above it one base-2^dbits digit of the weight and the digit's index (2 bits): a weight of more than
// dbits bits becomes one record per non-zero digit (exact: the matrix is uint32 wrap-around arithmetic, shifted digits add up).
struct __attribute__((aligned(16))) WideRec { unsigned long long rows, cols; };
struct PoolView {
    uint32_t* counters;            // KCTR_*
    uint32_t* chunk_key;           // [pool_cap] stream of the chunk (n_states: never opened)
    uint32_t* chunk_fill;          // [pool_cap] records in the chunk
    unsigned char* rec;            // record slots, 16 bytes each
    uint32_t* recw;
    uint32_t* sub_cursor;          // [KMDB_SUBPOOLS * 16] chunks taken from every sub-pool
    uint32_t sub_cap;              // chunks per sub-pool
    uint32_t pool_cap;             // chunks
    // wide pool (dense mode): records in arrival order with their stream keys; a device-wide sort groups them afterwards
    uint32_t* wkey;                // [wide slots] stream of the record, 0xFFFFFFFF = never written
    WideRec* wrec;                 // [wide slots]
    uint32_t* wsub_cursor;         // [KMDB_SUBPOOLS * 16]
    uint32_t wsub_cap;             // chunks per sub-pool of the wide pool
    uint32_t dense;
    uint32_t kbits, dbits;         // key word of the wide pool: stream bits, weight digit bits                // 1: this kernel writes into the wide pool
    uint32_t row_mode;             // 1: many streams — the wide records go to per-block-row chunks of the chunk pool instead of the arrival-order
    uint32_t n_states;             // pool, so that only the sort inside the rows remains
    uint32_t pshift;               // row mode, != 0: packed records — the weight digit (and its index) sit in the column mask word from bit `pshift` (= the
                                   // block width) on, 64 - pshift - 2 bits of digit; the key word beside the record holds the stream only and stays behind in the sort
};
// What the emit kernels hold of a PoolView: the members every record store reads, by value, and the view itself where it lies in the kernel's parameter block.
// The others (cursors, capacities, the chunk table, the counters: read once per grab of chunks or when a pool runs over) are re-read from there at their
// point of use — pool_cold() — instead of occupying scalar registers for the whole kernel.  A PoolView serves the same functions (all members by value).
struct PoolRef {
    KARG(PoolView) k;
    unsigned char* rec; uint32_t* recw;        // row mode
    uint32_t* wkey; WideRec* wrec;             // few streams
    uint32_t kbits, dbits, pshift;
};
__device__ __forceinline__ const PoolView* pool_cold(const PoolView& pv) { return &pv; }
__device__ __forceinline__ KARG(PoolView) pool_cold(const PoolRef& pv) { KARG(PoolView) k = pv.k; asm volatile("" : "+s"(k)); return k; }
struct Resv { uint32_t base1, n1, base2; };   // slots [base1, base1 + n1) and [base2, ...) for the rest
__device__ __forceinline__ uint32_t resv_slot(const Resv& r, uint32_t rank) { return rank < r.n1 ? r.base1 + rank : r.base2 + (rank - r.n1); }

// A wave's private allocator.  Chunk ids come from one of KMDB_SUBPOOLS sub-pools (sub-pool p owns the ids p, p + SUBPOOLS,
// p + 2 SUBPOOLS, ...), ARENA_GRAB at a time: one device atomic per 1024 records and wave, spread over 256 cursors (a single
// cursor would serialise: same-address atomics run at a few million per second).  The open chunks live in an LDS table,
// direct-mapped by stream (entry = stream mod table size; with at most that many streams an open chunk is only ever
// closed full, otherwise a colliding stream evicts it).  An entry = {stream, chunk id << 6 | records used}; a chunk that
// fills up is closed at once, so `used` of an open entry is below 64.
constexpr uint32_t KEY_NONE = 0xFFFFFFFFu;
constexpr uint32_t ST_MAX_BITS = 10;            // at most 1024 open chunks per wave
struct WaveArena {
    uint32_t* t_key;               // LDS [1 << tbits]; not there (direct) when every stream has its own entry
    uint32_t* t_slot;              // LDS [1 << tbits], KEY_NONE = no open chunk
    uint32_t tmask;
    uint32_t direct;
    uint32_t sub;                  // this wave's sub-pool
    uint32_t stock, next;          // wave-uniform: stream chunks left of the last grab, the next of them (index inside the sub-pool)
    uint32_t wstock, wnext, wsub;  // the same for the wide pool (its sub-pool changes with every grab)
    uint32_t dslot;                // wide pool: next slot of the wave's one open chunk (dopen == 0: none)
    uint32_t dopen;
};
constexpr uint32_t ARENA_GRAB = 4;         // stream chunks (256 records) per grab (16 per grab — a quarter of the returning device atomics, which wait for
                                           // the wave's record stores to drain — measured no faster at 10 000 samples: profiles/r05_j8)
constexpr uint32_t WIDE_GRAB = 4;          // wide-pool chunks (64 records) per grab: every wave leaves an unfinished grab behind, and the
                                           // sort reads all slots up to the busiest sub-pool's cursor (16 -> 4: -0.35 ms at the benchmark database)
__host__ __device__ inline uint32_t arena_table_bits(uint32_t n_states) {
    uint32_t b = 4;
    while (b < ST_MAX_BITS && (1u << b) < n_states) ++b;
    return b;
}
// the table is indexed by block: only the records (X, X) of a list's first block go through stream chunks
__host__ __device__ inline size_t arena_table_bytes(uint32_t tbits, uint32_t n_keys) {
    if (tbits == 0) return 16;
    return ((size_t)4 << tbits) * (n_keys <= (1u << tbits) ? 1 : 2);
}
__device__ __forceinline__ void arena_init(WaveArena& A, uint32_t* lds, uint32_t tbits, uint32_t n_states, uint32_t wave_id, uint32_t lane) {
    A.direct = n_states <= (1u << tbits) ? 1u : 0u;
    A.t_slot = lds; A.t_key = lds + (1u << tbits); A.tmask = (1u << tbits) - 1u;
    A.sub = wave_id % KMDB_SUBPOOLS; A.wsub = A.sub; A.stock = 0; A.next = 0; A.wstock = 0; A.wnext = 0; A.dslot = 0; A.dopen = 0;
    if (tbits == 0) return;                                   // dense mode: no table
    for (uint32_t e = lane; e <= A.tmask; e += WAVE) { A.t_slot[e] = KEY_NONE; if (!A.direct) A.t_key[e] = KEY_NONE; }
    lds_sync();
}
template <class PV> __device__ __forceinline__ uint32_t arena_take(WaveArena& A, const PV& pv, uint32_t s, uint32_t lane) {
    if (A.stock == 0) {
        uint32_t base = 0;
        A.sub = (A.sub + 61u) % KMDB_SUBPOOLS;                        // every grab from another sub-pool: a wave with much output does not drain one
        if (lane == 0) base = atomicAdd(&pool_cold(pv)->sub_cursor[A.sub * 16u], ARENA_GRAB);
        base = bcast(base, 0);
        if (base + ARENA_GRAB > pool_cold(pv)->sub_cap) {                        // stays in range; the call is repeated with a larger pool
            if (lane == 0) atomicOr(&pool_cold(pv)->counters[KCTR_POOL_OVERFLOW], 1u);
            base = pool_cold(pv)->sub_cap - ARENA_GRAB;
        }
        A.next = base; A.stock = ARENA_GRAB;
    }
    const uint32_t id = A.next * KMDB_SUBPOOLS + A.sub;
    ++A.next; --A.stock;
    if (lane == 0) pool_cold(pv)->chunk_key[id] = s;
    return id;
}
// next chunk of the wide pool
template <class PV> __device__ __forceinline__ uint32_t arena_take_wide(WaveArena& A, const PV& pv, uint32_t lane) {
    if (A.wstock == 0) {
        uint32_t base = 0;
        A.wsub = (A.wsub + 61u) % KMDB_SUBPOOLS;                     // every grab from another sub-pool: waves with much output do not drain one
        if (lane == 0) base = atomicAdd(&pool_cold(pv)->wsub_cursor[A.wsub * 16u], WIDE_GRAB);
        base = bcast(base, 0);
        if (base + WIDE_GRAB > pool_cold(pv)->wsub_cap) {                     // stays in range; the call is repeated with a larger pool
            if (lane == 0) atomicOr(&pool_cold(pv)->counters[KCTR_WIDE_OVERFLOW], 1u);
            base = pool_cold(pv)->wsub_cap - WIDE_GRAB;
        }
        A.wnext = base; A.wstock = WIDE_GRAB;
    }
    const uint32_t id = A.wnext * KMDB_SUBPOOLS + A.wsub;
    ++A.wnext; --A.wstock;
    return id;
}
// cnt (1..64) slots of stream s; s and cnt wave-uniform, every lane of the wave calls
// cnt (1..64) slots of the wide pool: records of all streams share the wave's one open chunk, a device-wide sort groups them
template <class PV> __device__ __forceinline__ Resv arena_reserve_wide(WaveArena& A, const PV& pv, uint32_t cnt, uint32_t lane) {
    if (!A.dopen) { A.dslot = arena_take_wide(A, pv, lane) << WCH_SHIFT; A.dopen = 1; }
    const uint32_t v = A.dslot, rem = WCH_REC - (v & (WCH_REC - 1u));
    if (cnt < rem) { A.dslot = v + cnt; return Resv{v, cnt, 0u}; }
    if (cnt == rem) { A.dopen = 0; return Resv{v, cnt, 0u}; }
    const uint32_t nv = arena_take_wide(A, pv, lane) << WCH_SHIFT;
    A.dslot = nv + (cnt - rem);
    return Resv{v, rem, nv};
}
// cnt (1..64) slots of stream s, whose open chunk lives in table entry `ent`; all arguments wave-uniform, every lane calls
__device__ __forceinline__ Resv arena_reserve(WaveArena& A, const PoolView& pv, uint32_t ent, uint32_t s, uint32_t cnt, uint32_t lane) {
    const uint32_t e = ent & A.tmask;
    uint32_t v = A.t_slot[e];
    if (A.direct) {
        if (v == KEY_NONE) v = arena_take(A, pv, s, lane) << CH_SHIFT;
    } else {
        const uint32_t key = A.t_key[e];
        if (key != s) {
            if (key != KEY_NONE && lane == 0) pv.chunk_fill[v >> CH_SHIFT] = v & (CH_REC - 1u);        // evicted partly filled
            v = arena_take(A, pv, s, lane) << CH_SHIFT;
        }
    }
    const uint32_t rem = CH_REC - (v & (CH_REC - 1u));
    Resv r{v, cnt, 0u};
    uint32_t nkey = s, nv = v + cnt;
    if (cnt >= rem) {
        if (lane == 0) pv.chunk_fill[v >> CH_SHIFT] = CH_REC;                                      // full
        if (cnt == rem) { nkey = KEY_NONE; nv = KEY_NONE; }
        else {
            nv = arena_take(A, pv, s, lane) << CH_SHIFT;
            r = Resv{v, rem, nv};
            nv += cnt - rem;
        }
    }
    if (lane == 0) { A.t_slot[e] = nv; if (!A.direct) A.t_key[e] = nkey; }
    lds_sync();
    return r;
}
template <class PV> __device__ __forceinline__ void arena_finish(const WaveArena& A, const PV& pv, uint32_t lane) {
    if (A.tmask == 0) return;                                   // no stream table
    for (uint32_t e = lane; e <= A.tmask; e += WAVE) {
        const uint32_t v = A.t_slot[e];
        if (v != KEY_NONE && (A.direct || A.t_key[e] != KEY_NONE)) pool_cold(pv)->chunk_fill[v >> CH_SHIFT] = v & (CH_REC - 1u);
    }
}
// Few streams: the key array of the wide pool is NOT filled before a call.  A slot holds a record of this call iff its chunk was handed out (its index
// inside its sub-pool lies below the sub-pool's cursor: the sort tests that, cs_chunks_handed) and the wave that took the chunk wrote the slot.  What a
// wave took and did not write — the tail of its one open chunk and the chunks left of its last grab — gets the "never written" key here: at most
// WIDE_GRAB stores per wave.  Every kernel instantiation that reserves slots of the wide pool ends with this call.
template <class PV> __device__ __forceinline__ void arena_finish_wide(const WaveArena& A, const PV& pv, uint32_t lane) {
    if (A.dopen && lane < WCH_REC - (A.dslot & (WCH_REC - 1u))) pv.wkey[A.dslot + lane] = KEY_NONE;
    for (uint32_t k = 0; k < A.wstock; ++k) pv.wkey[(((A.wnext + k) * KMDB_SUBPOOLS + A.wsub) << WCH_SHIFT) + lane] = KEY_NONE;
}

// diagonal streams (X == Y, cols == rows) pack 8-byte rows into the first half of their chunks
// the records `on` of a wave step into the wide pool: one reservation for all lanes per weight digit (nearly always one digit).
// Every lane of the wave calls.
template <class PV> __device__ __forceinline__ void wide_emit(WaveArena& A, const PV& pv, bool on, unsigned long long rows, unsigned long long cols, uint32_t w, uint32_t stream,
                                          uint32_t lane, unsigned long long lt_mask) {
    // (packed records, pv.pshift != 0: the weight digit and its index in the spare bits of the column word, the key word = the stream only)
    const uint32_t dbits = pv.pshift ? (64u - pv.pshift - 2u < 16u ? 64u - pv.pshift - 2u : 16u) : pv.dbits;
    const uint32_t dmask = (1u << dbits) - 1u;
    uint32_t j = 0;
    for (;;) {
        const unsigned long long grp = __ballot(on);
        if (!grp) break;
        const Resv r = arena_reserve_wide(A, pv, (uint32_t)__popcll(grp), lane);
        if (on) {
            const uint32_t slot = resv_slot(r, (uint32_t)__popcll(grp & lt_mask));
            if (pv.pshift) {
                pv.wrec[slot] = WideRec{rows, cols | ((unsigned long long)((w & dmask) | (j << dbits)) << pv.pshift)};
                pv.wkey[slot] = stream;
            } else {
                pv.wrec[slot] = WideRec{rows, cols};
                pv.wkey[slot] = stream | (((w & dmask) | (j << dbits)) << pv.kbits);
            }
        }
        w >>= dbits; ++j;
        on = on && w != 0;
    }
}
// weight of a sorted wide record from its key word
__device__ __forceinline__ uint32_t wide_weight(uint32_t key, uint32_t kbits, uint32_t dbits) {
    const uint32_t f = key >> kbits, dig = f & ((1u << dbits) - 1u), j = f >> dbits;
    const uint32_t sh = j * dbits;
    return sh < 32u ? dig << sh : 0u;
}
// ---- many streams (row mode): the wide records of block row X go to chunks of their own (CH_REC records, key n_states + X), so they
// arrive grouped by row and only the sort inside the rows is left.  A wave keeps, per row, the next free slot of its open chunk and
// the chunk's end in LDS; every lane reserves its slot with ONE LDS atomic (lanes that follow one another with the same row share
// one): no loop over the rows of a step.  A reservation that runs past the chunk's end is the rare case (once per CH_REC records
// and row): the row gets fresh chunks and the lanes beyond the end are renumbered.
struct RowTab { uint32_t* pos; uint32_t* end; uint32_t n; };
__host__ __device__ inline size_t rowtab_bytes(uint32_t n_rows) { return ((size_t)8 * n_rows + 15) & ~(size_t)15; }
__device__ __forceinline__ void rowtab_init(RowTab& R, uint32_t* lds, uint32_t n, uint32_t lane) {
    R.pos = lds; R.end = lds + n; R.n = n;
    for (uint32_t e = lane; e < 2u * n; e += WAVE) lds[e] = 0u;         // end == 0: no open chunk
    lds_sync();
}
template <class PV> __device__ __forceinline__ void row_emit(WaveArena& A, const PV& pv, const RowTab& R, bool on, uint32_t X, unsigned long long rows, unsigned long long cols,
                                         uint32_t w, uint32_t stream, uint32_t lane, unsigned long long lt_mask) {
    const uint32_t dbits = pv.pshift ? (64u - pv.pshift - 2u < 16u ? 64u - pv.pshift - 2u : 16u) : pv.dbits;
    const uint32_t dmask = (1u << dbits) - 1u;
    uint32_t j = 0;
    for (;;) {
        const unsigned long long onm = __ballot(on);
        if (!onm) break;
        // runs of consecutive lanes with the same row: the first lane of a run reserves for all of it (one LDS atomic per LANE instead —
        // the lanes of a row then collide in the LDS unit, the ~50 VALU instructions below are gone — measured no faster: profiles/r05_j5)
        const uint32_t pX = (uint32_t)__shfl_up((int)X, 1, WAVE);
        const bool lead = on && (lane == 0u || !((onm >> (lane - 1u)) & 1ull) || pX != X);
        const unsigned long long leaders = __ballot(lead);
        uint32_t ll = lane, cnt = 0;
        if (on) {
            ll = 63u - (uint32_t)__builtin_clzll(leaders & (lt_mask | (1ull << lane)));
            const unsigned long long above = ll == 63u ? 0ull : ~((2ull << ll) - 1ull);
            const unsigned long long after = (leaders | ~onm) & above;
            cnt = (after ? (uint32_t)__builtin_ctzll(after) : 64u) - ll;
        }
        uint32_t old = 0, end = 0;
        if (lead) { end = R.end[X]; old = atomicAdd(&R.pos[X], cnt); }
        uint32_t p = (uint32_t)__shfl((int)old, (int)ll, WAVE) + (lane - ll);
        const uint32_t e = (uint32_t)__shfl((int)end, (int)ll, WAVE);
        bool ovf = on && p >= e;
        unsigned long long pend = __ballot(ovf);
        while (pend) {
            const uint32_t l0 = (uint32_t)__builtin_ctzll(pend);
            const uint32_t X0 = bcast(X, l0), e0 = bcast(e, l0);
            lds_sync();
            const uint32_t tot = R.pos[X0];                        // after every lane's reservation
            const uint32_t over = tot - e0;                        // slots needed beyond the open chunk (no open chunk: e0 == 0, positions count from 0)
            const uint32_t nnew = (over + CH_REC - 1u) >> CH_SHIFT;
            if (lane == 0 && e0) pool_cold(pv)->chunk_fill[(e0 - 1u) >> CH_SHIFT] = CH_REC;
            const bool mine = ovf && X == X0;
            const uint32_t qv = p - e0;
            uint32_t cl = 0;
            for (uint32_t i = 0; i < nnew; ++i) {
                cl = arena_take(A, pv, pool_cold(pv)->n_states + X0, lane);        // key of a row chunk: n_states + row
                if (lane == 0 && i + 1u < nnew) pool_cold(pv)->chunk_fill[cl] = CH_REC;
                if (mine && (qv >> CH_SHIFT) == i) p = (cl << CH_SHIFT) | (qv & (CH_REC - 1u));
            }
            if (lane == 0) { R.pos[X0] = (cl << CH_SHIFT) + (over - ((nnew - 1u) << CH_SHIFT)); R.end[X0] = (cl << CH_SHIFT) + CH_REC; }
            lds_sync();
            ovf = ovf && !mine;
            pend = __ballot(ovf);
        }
        if (on) {
            if (pv.pshift) {
                ((WideRec*)pv.rec)[p] = WideRec{rows, cols | ((unsigned long long)((w & dmask) | (j << dbits)) << pv.pshift)};
                pv.recw[p] = stream;
            } else {
                ((WideRec*)pv.rec)[p] = WideRec{rows, cols};
                pv.recw[p] = stream | (((w & dmask) | (j << dbits)) << pv.kbits);
            }
        }
        w >>= dbits; ++j;
        on = on && w != 0;
    }
}
template <class PV> __device__ __forceinline__ void rowtab_finish(const RowTab& R, const PV& pv, uint32_t lane) {
    lds_sync();
    for (uint32_t X = lane; X < R.n; X += WAVE) {
        const uint32_t e = R.end[X];
        if (e) pool_cold(pv)->chunk_fill[(e - 1u) >> CH_SHIFT] = CH_REC - (e - R.pos[X]);
    }
}
// the emit path of a kernel instantiation: ROWS = many streams (row chunks), otherwise few streams (the wide pool in arrival order).  The other
// path's code, and with it the state it keeps live, does not exist in the instantiation.
template <bool ROWS, class PV>
__device__ __forceinline__ void rec_emit(WaveArena& A, const PV& pv, const RowTab& R, bool on, uint32_t X, unsigned long long rows, unsigned long long cols,
                                         uint32_t w, uint32_t stream, uint32_t lane, unsigned long long lt_mask) {
    if constexpr (ROWS) row_emit(A, pv, R, on, X, rows, cols, w, stream, lane, lt_mask);
    else wide_emit(A, pv, on, rows, cols, w, stream, lane, lt_mask);
}
// stream chunks hold the records (X, X, rows) of one block X: 8-byte rows in the first half of the chunk, weights beside
__device__ __forceinline__ void rec_store_diag(const PoolView& pv, uint32_t slot, unsigned long long rows, uint32_t w) {
    const uint32_t ch = slot >> CH_SHIFT, r = slot & (CH_REC - 1u);
    ((unsigned long long*)(pv.rec + ((size_t)ch << (CH_SHIFT + 4))))[r] = rows;
    pv.recw[slot] = w;
}

// the start of a call in ONE launch: the first n_state words of the per-call state (BlocksState::call_state) cleared, every chunk of the chunk table
// empty and never opened, and — the first attempt of a call — no tile flagged as touched
__global__ void call_prologue_kernel(uint32_t* __restrict__ state, uint32_t n_state, uint32_t* __restrict__ chunk_fill, uint32_t* __restrict__ chunk_key,
                                     uint32_t pool_cap, unsigned char* __restrict__ touched, uint32_t n_touched) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n_state) state[i] = 0u;
    if (i < pool_cap) { chunk_fill[i] = 0u; chunk_key[i] = 0xFFFFFFFFu; }
    if (i < n_touched) touched[i] = 0;
}

// ------------------------------------------------------------------------------------------
// K0: gamma streams -> local (block, mask) pairs
// ------------------------------------------------------------------------------------------
struct K0Params {
    const uint2* k0in;
    const uint32_t* bitrel;
    const uint64_t* blkbase;
    const uint64_t* bits;
    const uint32_t* perm;          // the long launch: its nodes, most work first
    const uint16_t* order;         // the short launch: the nodes of every window of 1 << win_shift DFS nodes by decreasing work (kmdb_db.k0_order) ...
    const uint32_t* live;          // ... and how many of them it decodes (kmdb_db.k0_live)
    uint32_t win_shift;
    uint32_t n_items;              // the short launch's workgroups that have a window: 256 ranks of a window each
    uint32_t P;                    // nodes of this launch
    BlockMap bm;
    unsigned long long* p0_mask;   // first pair inline
    uint32_t* p0_info;             // block | npairs << 16
    uint32_t* pair_ofs;            // further pairs: first entry in the pair pool
    uint16_t* pair_blk;
    unsigned long long* pair_mask;
    uint32_t* pair_cursor;         // [KMDB_PAIR_REGIONS * 16]
    uint32_t n_regions, region_cap, spill_cap;   // sub-pools of region_cap entries each, then a shared spill area
    uint32_t* counters;
};

constexpr int K0_RELW = 8;                 // non-empty 64-id words of a long list kept in registers (more: the list is walked twice)
constexpr int K0_SINGLE_PASS = 1;          // 0: every list spanning 64 ids or more is walked twice, as in round 3 (A/B)
template <bool LONG>
__global__ __launch_bounds__(256) void k0_decode_kernel(const K0Params q) {
    // two launches cover the nodes: the short one takes every node whose stream fits three registers, window by window of the DFS order
    // (all its global accesses stay inside the window); the few others are listed in perm, most work first, and decoded by the long
    // launch so that no wave waits on one long stream
    const uint32_t lane = threadIdx.x & 63u;
    uint32_t i = 0;
    bool live;
    if constexpr (LONG) {
        const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
        live = t < q.P;
        if (live) i = q.perm[t];
    } else {
        // The nodes of a window are dealt to its threads by decreasing amount of work, 64 to a wave, so every wave runs decode loops of
        // similar length.  The order is the layout's (it depends on the list heads alone: made once per database, lay_k0_order_kernel);
        // a wave whose ranks all lie behind the window's live count has nothing to decode.  The workgroups of a window wider than 256
        // nodes run on one XCD (the grid is a multiple of 8 windows): the lines of p0_mask / p0_info they fill together are completed in one L2.
        // (Windows go to the XCDs in turn, window w to XCD w % 8 — workgroup b runs on XCD b % 8.  One contiguous eighth of the DFS order per XCD, as
        // xcd_contiguous deals the sort's jobs, was measured slower: 2.31 / 1.82 ms against 1.95 / 1.58 ms at windows of 1024 / 4096 nodes)
        const uint32_t sub_shift = q.win_shift - 8u;                         // log2 of the workgroups per window: 0 unless KMDB_K0_WINDOW widens it
        const uint32_t k = blockIdx.x >> 3;                                  // the workgroup's place among its XCD's
        const uint32_t w = sub_shift ? ((k >> sub_shift) << 3) + (blockIdx.x & 7u) : blockIdx.x;
        if ((w << sub_shift) >= q.n_items) return;
        const uint32_t r = ((k & ((1u << sub_shift) - 1u)) << 8) + threadIdx.x;
        const uint32_t n_live = q.live[w];
        if ((r & ~63u) >= n_live) return;
        live = r < n_live;
        if (live) i = (w << q.win_shift) + q.order[((size_t)w << q.win_shift) + r];
    }
    const BlockMap bm = q.bm;
    const uint2 km = live ? q.k0in[i] : make_uint2(0u, 0u);
    const uint32_t l = kmdb_k0_l(km), last = kmdb_k0_last(km), nbits = kmdb_k0_bits(km);
    using Cursor = RunCursor32<LONG ? 16 : 6, LONG>;
    uint32_t npairs = 0, blk0 = 0, need = 0, span = 0, bit0 = 0;
    unsigned long long mask0 = 0, m1 = 0, m2 = 0;
    bool second_pass = false, from_words = false;
    uint64_t pos = 0;
    // (long launch) the non-empty 64-id words of the relative list: K0_RELW of them in registers, filled in order
    unsigned long long rel_w[K0_RELW];
    uint32_t rel_i[K0_RELW], rel_n = 0;
#pragma unroll
    for (int e = 0; e < K0_RELW; ++e) { rel_w[e] = 0; rel_i[e] = 0; }
    auto rel_push = [&](uint32_t idx, unsigned long long w) {
#pragma unroll
        for (int e = 0; e < K0_RELW; ++e) if (rel_n == (uint32_t)e) { rel_w[e] = w; rel_i[e] = idx; }     // (static register indices: no scratch)
        ++rel_n;                                                  // beyond K0_RELW: the list takes the second walk after all
    };
    // the words cut at the block boundaries: (block, mask) pairs in ascending order.  WRITE = false counts them, true stores them
    // (the first one inline, the others in the pair pool from `o` on)
    auto rel_blocks = [&](bool write, uint32_t id0, uint32_t o) -> uint32_t {
        const unsigned long long wm = bm.width == 64 ? ~0ull : (1ull << bm.width) - 1ull;
        uint32_t curblk = 0xFFFFFFFFu, cnt = 0;
        unsigned long long cacc = 0;
        auto flushb = [&]() {
            if (curblk == 0xFFFFFFFFu) return;
            if (write) { if (cnt == 0) mask0 = cacc; else { q.pair_blk[o] = (uint16_t)curblk; q.pair_mask[o] = cacc; ++o; } }
            ++cnt;
        };
#pragma unroll
        for (int e = 0; e < K0_RELW; ++e) {
            if ((uint32_t)e < rel_n) {
                const uint32_t base = id0 + 64u * rel_i[e];
                const unsigned long long word = rel_w[e];
                const uint32_t b = bm.blk(base);
                uint32_t bit = bm.bit(base, b), sh = 0;
#pragma unroll
                for (uint32_t part = 0; part < 3; ++part) {       // 64 ids meet at most three blocks (width >= 32)
                    if (sh < 64u) {
                        const unsigned long long m = ((word >> sh) << bit) & wm;
                        if (m) {
                            if (b + part != curblk) { flushb(); curblk = b + part; cacc = 0; }
                            cacc |= m;
                        }
                        sh += bm.width - bit; bit = 0;
                    }
                }
            }
        }
        flushb();
        return cnt;
    };
    if (live && l == 1) {
        blk0 = bm.blk(last); mask0 = 1ull << bm.bit(last, blk0); npairs = 1;
    } else if (live && l) {
        // Pass 1 walks the stream run by run and builds the list RELATIVE to its (still unknown) first id:
        // bit k of R <=> id_0 + k is in the list.  pattern_t::decodeSamples (reference src/pattern.cpp:99-109)
        // gets id_0 the same way: last id minus the sum of the deltas.
        unsigned long long R = 1ull;
        if (!LONG && kmdb_k0_run_only(l, nbits)) {
            // (short launch) l - 1 deltas in l - 1 bits: all of them 1, the list is one run of l <= 64 ids.  No stream word is read; these
            // lanes and the single ids sort last, so whole waves of them skip the cursor and its loop (the branch below is wave-uniform there).
            R = (2ull << (l - 1u)) - 1ull;
            span = l - 1u;
        } else {
            pos = q.blkbase[i >> 8] + q.bitrel[i];
            Cursor c(q.bits, pos);
            uint32_t rem = l - 1;
            // the long launch keeps the WHOLE relative list, not only its first 64 ids: the non-empty 64-id words (word index, mask)
            // in registers, in ascending order (ids ascend, so a word is complete when the next one starts).  A list that spans 64 ids or
            // more — four fifths of the long nodes of a 10 000-sample collection (profiles/r04_record_stats.py) — then needs no second
            // walk over its stream: its words are cut at the block boundaries once the first id is known.
            uint32_t wk = 0;
            unsigned long long acc = 1ull;
            auto add = [&](uint32_t s0, uint32_t cnt) {               // relative ids [s0, s0 + cnt), cnt >= 1
                while (cnt) {
                    const uint32_t k = s0 >> 6, o = s0 & 63u;
                    const uint32_t take = cnt < 64u - o ? cnt : 64u - o;
                    if (k != wk) { rel_push(wk, acc); wk = k; acc = 0; }
                    acc |= (take == 64u ? ~0ull : ((1ull << take) - 1ull)) << o;
                    s0 += take; cnt -= take;
                }
            };
            while (rem) {
                uint32_t z, v;
                c.step(rem, z, v);                                     // a run of z consecutive ids, then a gap of v
                if (z) {
                    if (LONG) add(span + 1u, z);
                    else if (span + z < 64u) R |= ((2ull << (z - 1)) - 1ull) << (span + 1);
                    span += z; rem -= z;
                }
                if (v) {
                    span += v; --rem;
                    if (LONG) add(span, 1u);
                    else if (span < 64u) R |= 1ull << span;
                }
            }
            if (LONG) { if (span < 64u) R = acc; else rel_push(wk, acc); }
        }
        const uint32_t id0 = last - span;
        blk0 = bm.blk(id0);
        bit0 = bm.bit(id0, blk0);
        const unsigned long long wm = bm.width == 64 ? ~0ull : (1ull << bm.width) - 1ull;
        if (span < 64u) {
            // the whole list fits the relative mask: cut it at the block boundaries (at most 3 blocks: width >= 32)
            const unsigned long long lo = R << bit0, hi = bit0 ? R >> (64u - bit0) : 0ull;
            auto ext = [&](uint32_t sh) -> unsigned long long {
                return sh == 0 ? lo : sh < 64u ? ((lo >> sh) | (hi << (64u - sh))) : sh == 64u ? hi : sh < 128u ? (hi >> (sh - 64u)) : 0ull;
            };
            mask0 = lo & wm;
            m1 = ext(bm.width) & wm; m2 = ext(2 * bm.width) & wm;
            npairs = 1u + (m1 != 0) + (m2 != 0);
            need = npairs - 1u;
        } else if (LONG && K0_SINGLE_PASS && rel_n <= (uint32_t)K0_RELW) {
            // wide list, all its words at hand: the pairs are counted now (exactly) and stored after the reservation
            from_words = true;
            npairs = rel_blocks(false, id0, 0u);
            need = npairs - 1u;
        } else {
            // wide list: second pass with absolute ids; the blocks it can touch bound the reservation
            second_pass = true;
            need = bm.blk(last) - blk0;
            need = need < l - 1u ? need : l - 1u;                 // l ids touch at most l blocks
        }
    }
    // extra pairs: one reservation per wave in the wave's region of the pair pool
    uint32_t out = 0;
    if (__ballot(need != 0u)) {                                  // (most waves of the short launch hold no list with a second block: no scan for them)
        const uint32_t incl = wave_incl_scan(need, lane);
        const uint32_t total = bcast(incl, WAVE - 1);
        if (total) {
            const uint32_t region = (blockIdx.x * 4u + (threadIdx.x >> 6)) % q.n_regions;
            uint32_t base = 0;
            if (lane == WAVE - 1) base = atomicAdd(&q.pair_cursor[region * 16u], total);
            base = bcast(base, WAVE - 1);
            if (base + total <= q.region_cap) out = region * q.region_cap + base + (incl - need);
            else {
                // the wave's sub-pool is full: the shared spill area behind the sub-pools (one cursor, rarely used)
                uint32_t sb = 0;
                if (lane == WAVE - 1) sb = atomicAdd(&q.pair_cursor[q.n_regions * 16u], total);
                sb = bcast(sb, WAVE - 1);
                if (sb + total <= q.spill_cap) out = q.n_regions * q.region_cap + sb + (incl - need);
                else {
                    if (lane == 0) atomicOr(&q.counters[KCTR_PAIR_OVERFLOW], 1u);
                    need = 0; second_pass = false; from_words = false; npairs = npairs ? 1u : 0u; m1 = m2 = 0;    // results invalid; the call is repeated with a larger pool
                }
            }
        }
    }
    if (!live) return;
    if (from_words) {
        (void)rel_blocks(true, last - span, out);
    } else if (!second_pass) {
        if (m1) { q.pair_blk[out] = (uint16_t)(blk0 + 1); q.pair_mask[out] = m1; }
        if (m2) { const uint32_t o2 = out + (m1 != 0); q.pair_blk[o2] = (uint16_t)(blk0 + 2); q.pair_mask[o2] = m2; }
    } else {
        Cursor c(q.bits, pos);
        uint32_t o = out;
        uint32_t curblk = blk0, bit = bit0, rem = l - 1;
        unsigned long long acc = 1ull << bit0;
        auto flush = [&]() {
            if (npairs == 0) mask0 = acc;
            else { q.pair_blk[o] = (uint16_t)curblk; q.pair_mask[o] = acc; ++o; }
            ++npairs;
        };
        while (rem) {
            uint32_t z, v;
            c.step(rem, z, v);
            if (z) {
                rem -= z;
                while (z) {
                    const uint32_t room = bm.width - 1u - bit;
                    const uint32_t tk = z < room ? z : room;
                    if (tk) { acc |= ((2ull << (tk - 1)) - 1ull) << (bit + 1); bit += tk; z -= tk; }
                    if (z) { flush(); ++curblk; acc = 1ull; bit = 0; --z; }
                }
            }
            if (v) {
                const uint32_t id = curblk * bm.width + bit + v;
                --rem;
                const uint32_t blk = bm.blk(id);
                if (blk != curblk) { flush(); curblk = blk; acc = 0; }
                bit = bm.bit(id, blk);
                acc |= 1ull << bit;
            }
        }
        flush();
    }
    q.p0_mask[i] = mask0;
    q.p0_info[i] = blk0 | (npairs << 16);
    if (npairs > 1) q.pair_ofs[i] = out;
}

// ------------------------------------------------------------------------------------------
// bit transposes and operand types of the matrix-core step (K1n's direct mode, K2, the second level)
// ------------------------------------------------------------------------------------------
// 64 x 64 bit-matrix transpose across the lanes of a wave: lane i holds row i on entry, column i on exit.  Six butterfly stages; stage
// 32 is one v_permlane32_swap over the two words.  Every stage below works on the 32-bit words separately: fetch the partner lane's
// word (lane ^ s), rotate it by s towards this lane's side (v_alignbit_b32: right for the upper lane of a pair, left for the lower one)
// and splice it in under a per-lane mask (v_bfi_b32) — three instructions per word and stage, with the rotate amounts and masks of
// the five stages in ten registers that are computed once per run (TrConst).  The fetches are v_permlane16_swap (stage 16) and DPP row /
// quad permutes: 35 VALU instructions per transpose, no LDS (fetching the stages 16 / 8 / 4 over the LDS crossbar with ds_swizzle_b32
// was measured slower — profiles/r05_experiment_switches.diff; round 3's version, v_perm + ds_bpermute shuffles and 64-bit mask
// arithmetic, took 72 VALU).  profiles/r04_transpose_probe.hip checks the variants against the definition and times them.
struct TrConst { uint32_t amt[5], msk[5]; };
__device__ __forceinline__ TrConst tr_const(uint32_t lane) {
    TrConst c;
    const uint32_t m[5] = {0x0000FFFFu, 0x00FF00FFu, 0x0F0F0F0Fu, 0x33333333u, 0x55555555u};
#pragma unroll
    for (int k = 0; k < 5; ++k) {
        const uint32_t s = 16u >> k;
        const bool up = (lane & s) != 0;
        c.amt[k] = up ? s : 32u - s;          // the partner's word rotated right by s (upper lane of the pair) or left by s (lower lane)
        c.msk[k] = up ? m[k] : ~m[k];         // the bits taken from the partner
    }
    return c;
}
__device__ __forceinline__ uint32_t tr_fetch(uint32_t v, int k, bool up16) {
    // the word of lane ^ (16 >> k)
    if (k == 0) {
        const auto a = __builtin_amdgcn_permlane16_swap(v, v, false, false);      // [0]: odd rows <- the even rows below them, [1]: even rows <- the odd rows above
        return up16 ? a[0] : a[1];
    }
    if (k == 1) return (uint32_t)__builtin_amdgcn_update_dpp((int)v, (int)v, 0x128, 0xF, 0xF, false);   // row_ror:8
    if (k == 2) {
        const int a = __builtin_amdgcn_update_dpp((int)v, (int)v, 0x104, 0xF, 0x5, false);      // row_shl:4 into the banks 0 and 2: lane i <- i + 4
        return (uint32_t)__builtin_amdgcn_update_dpp(a, (int)v, 0x114, 0xF, 0xA, false);        // row_shr:4 into the banks 1 and 3: lane i <- i - 4
    }
    if (k == 3) return (uint32_t)__builtin_amdgcn_update_dpp((int)v, (int)v, 0x4E, 0xF, 0xF, false);   // quad_perm [2,3,0,1]
    return (uint32_t)__builtin_amdgcn_update_dpp((int)v, (int)v, 0xB1, 0xF, 0xF, false);               // quad_perm [1,0,3,2]
}
__device__ __forceinline__ unsigned long long transpose64(unsigned long long x, const TrConst& c) {
    uint32_t lo = (uint32_t)x, hi = (uint32_t)(x >> 32);
    {
        const auto r = __builtin_amdgcn_permlane32_swap(lo, hi, false, false);
        lo = r[0]; hi = r[1];
    }
    const bool up16 = c.msk[0] == 0x0000FFFFu;                         // (lane & 16) != 0
#pragma unroll
    for (int k = 0; k < 5; ++k) {
        const uint32_t pl = tr_fetch(lo, k, up16), ph = tr_fetch(hi, k, up16);
        const uint32_t rl = __builtin_amdgcn_alignbit(pl, pl, c.amt[k]), rh = __builtin_amdgcn_alignbit(ph, ph, c.amt[k]);
        asm("v_bfi_b32 %0, %1, %2, %0" : "+v"(lo) : "v"(c.msk[k]), "v"(rl));      // (mask & partner) | (~mask & own)
        asm("v_bfi_b32 %0, %1, %2, %0" : "+v"(hi) : "v"(c.msk[k]), "v"(rh));
    }
    return ((unsigned long long)hi << 32) | lo;
}

typedef int k2_v4i __attribute__((ext_vector_type(4)));
typedef int k2_v16i __attribute__((ext_vector_type(16)));

// ------------------------------------------------------------------------------------------
// K1n: the DFS stream, nodes with at most two blocks
// ------------------------------------------------------------------------------------------
// Summary of a stretch of a root path: the first block and its mask, the second block and its mask, and whether
// there is a third one.  Ids ascend along a root path, so "the ancestors' stretch" always holds the smaller blocks.
constexpr uint32_t BNONE = 0x7FFFu;
struct NSum { unsigned long long m0, m1; uint32_t bw; };        // bw = b0 | b1 << 15 | wide << 30

__device__ __forceinline__ NSum nsum_make(uint32_t b0, unsigned long long m0, uint32_t b1, unsigned long long m1, bool wide) {
    return NSum{m0, m1, b0 | (b1 << 15) | ((wide ? 1u : 0u) << 30)};
}
// T = the stretch closer to the root, S = the stretch below it
__device__ __forceinline__ NSum nsum_merge(const NSum& T, const NSum& S) {
    const uint32_t Tb0 = T.bw & 0x7FFFu, Tb1 = (T.bw >> 15) & 0x7FFFu, Sb0 = S.bw & 0x7FFFu, Sb1 = (S.bw >> 15) & 0x7FFFu;
    bool wide = (((T.bw | S.bw) >> 30) & 1u) != 0;
    if (Tb0 == BNONE) return S;
    if (Sb0 == BNONE) return T;
    if (Sb0 == Tb0) return nsum_make(Sb0, S.m0 | T.m0, Sb1, S.m1, wide || Tb1 != BNONE);
    if (Tb1 == BNONE) return nsum_make(Tb0, T.m0, Sb0, S.m0, wide || Sb1 != BNONE);
    if (Tb1 == Sb0) return nsum_make(Tb0, T.m0, Sb0, T.m1 | S.m0, wide || Sb1 != BNONE);
    return nsum_make(Tb0, T.m0, Tb1, T.m1, true);
}
__device__ __forceinline__ NSum nsum_shfl(const NSum& s, int src) {
    return NSum{shfl64(s.m0, src), shfl64(s.m1, src), (uint32_t)__shfl((int)s.bw, src, WAVE)};
}
__device__ __forceinline__ NSum nsum_shfl_up(const NSum& s, int d) {
    return NSum{shfl_up64(s.m0, d), shfl_up64(s.m1, d), (uint32_t)__shfl_up((int)s.bw, d, WAVE)};
}

struct NParams {
    const uint32_t* nl;            // n
    const int32_t* parent;
    const uint32_t* w;
    const uint16_t* dflag;         // depth | has-child << 15
    const uint32_t* seg_anc;       // [n_segs][chain_cap] root-first ancestors of the slice's first node
    const uint32_t* seg_anc_n;
    const unsigned long long* p0_mask;
    const uint32_t* p0_info;
    const uint32_t* pair_ofs;
    const uint16_t* pair_blk;
    const unsigned long long* pair_mask;
    ulonglong2* fn_mask;           // written for the nodes with more than two blocks whose parent has at most two:
    uint32_t* fn_blk;              // the parent's (blocks, masks)
    unsigned long long* widebits;
    uint32_t* wide_base;           // [ceil(P / 64)] flagged nodes of the SLICE before every 64-node word (wide_expand_kernel adds the slices before it)
    uint32_t* wide_slice_cnt;      // [n_segs] flagged nodes of every slice
    uint32_t P, nseg_nodes, n_segs, chain_cap;
    uint32_t emit_lo, emit_hi;
    uint32_t tbits, n_keys;        // log2 of the open-chunk table, blocks
    uint32_t all_wide;             // 1: every record through the wide pool (the stream chunks did not work out)
    PoolView pool;
    // direct mode (k1n_kernel<true>): the first-block records (X, X, F0) never leave the wave — see k1n_kernel
    uint32_t* M;
    uint32_t N, bwidth;
    unsigned char* touched;
    uint32_t* direct_ctr;          // [KMDB_SUBPOOLS * 16]
    // flat mode (k1n_kernel<2>): the first-block records of slice s, compacted, in [s * nseg_nodes, + slice_cnt[s]) — applied by k2d_kernel
    unsigned long long* dmask;     // [n_segs * nseg_nodes] F0
    uint32_t* dwx;                 // [n_segs * nseg_nodes] w | X << 8
    uint32_t* slice_cnt;           // [n_segs]
    uint32_t dbg;                  // always 0 (no switch sets it).  The two tests of it in k1n_kernel<1, *> stay: without them k1n_kernel<1, 4, rows> is compiled with
                                   // 108 instead of 76 bytes of scratch per lane and measured 9.42 against 8.42 ms at C2 (profiles/a2a_cleanup_ab.json)
    // band emit (k1n_band_kernel; no other instantiation reads these): the band's block rows [band_xlo, band_xhi] and its first stream, tri32(band_xlo).
    // A record is emitted iff its block row X lies in the band, keyed tri32(X) - band_sbase + Y; n_keys then counts the band's block rows, and the open-chunk
    // table and the row tables are indexed by X - band_xlo
    uint32_t band_xlo, band_xhi, band_sbase;
};
constexpr int K1N_WAVES = 4;
__host__ __device__ inline size_t k1n_wave_bytes(uint32_t chain_cap, uint32_t tbits, uint32_t n_states, uint32_t n_rows) {
    return (((size_t)chain_cap * 20 + 15) & ~(size_t)15) + arena_table_bytes(tbits, n_states) + rowtab_bytes(n_rows);          // n_rows: 0 unless row mode
}

// The node records are fetched TWO batches ahead (pair_ofs read unconditionally with them), the second pairs one batch ahead: no load of
// the loop waits on another load of the same iteration.  (Round 4 fetched one batch ahead, the second pair of a node behind its p0_info and
// pair_ofs — three dependent round trips inside the fetch: 0.07 - 0.2 ms slower, profiles/r05_j3 / r05_j4.)
//
// DIRECT (round 6; north_star: "accumulated ... before a single HBM write-back per tile"; the reference adds a decoded pattern straight
// into the matrix rows, similarity_calculator.cpp:206-241): all nodes of a slice of the DFS stream but a handful share their first
// block X — the subtree of a root child holds the patterns whose smallest sample id is that child's (profiles/r06_tile_locality.txt:
// 99.5 % of a slice's first-block records lie in its most frequent block) — so the wave that emits the records (X, X, F0, w) applies
// them where they are: the 64 masks of a batch go through the bit transpose and the byte spreading of the apply kernels (k2_apply_mfma)
// straight from the registers that hold them, six v_mfma_i32_32x32x32_i8 add them to the lower triangle of tile (X, X), which stays
// in 48 accumulator registers for the whole slice and is written back ONCE, when the slice ends or its first block changes.  No record
// of these is written, grouped or read again (C2: 47 M of 125 M records, the whole stream-chunk path and the apply kernel beside the
// wide kernel).  The rare others — a lane whose first block is not the wave's current one, a weight of 128 or more — take the
// records' way through the wide pool / the row chunks as in all_wide mode.
// (NParams must stay the kernel's ONLY argument: kernarg_reread<NParams>() and PoolRef::k read it at offset 0 of the kernarg segment)
// The kernel's body.  BAND = false is k1n_kernel as it always was.  BAND = true (k1n_band_kernel, modes 0 and 2) is the emit filter of a band call: the
// walk — summaries, chain slots, the wide list's bits and counts, fn_* — is the whole tree's, a record (w0, w0), (w1, w0) or (w1, w1) is emitted iff its block
// row lies in [band_xlo, band_xhi], keyed relative to the band's first stream; mode 0's diagonal chunks and mode 2's per-slice compaction take the same
// filter (a slot outside the band is dropped, not culled later).
template <int MODE, bool ROWS, bool BAND>
__device__ __forceinline__ void k1n_body(const NParams& q) {
    static_assert(!BAND || MODE != 1, "mode 1 writes the whole matrix from the narrow kernel: it has no band form");
    constexpr bool DIRECT = MODE == 1, FLAT = MODE == 2;
    const uint32_t bxlo = BAND ? q.band_xlo : 0u, bsbase = BAND ? q.band_sbase : 0u;
    auto in_band = [&](uint32_t X) -> bool { if constexpr (BAND) return X >= q.band_xlo && X <= q.band_xhi; else return true; };
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    __shared__ unsigned long long lut_ff[DIRECT ? 256 : 1], lut_01[DIRECT ? 256 : 1];       // byte b -> its 8 bits spread over 8 bytes (0xFF / 0x01 where set)
    __shared__ __attribute__((aligned(16))) unsigned char wbuf[DIRECT ? K1N_WAVES : 1][64];
    const uint32_t lane = lane_id();
    const uint32_t wave = threadIdx.x >> 6;
    const uint32_t seg = blockIdx.x * (blockDim.x >> 6) + wave;            // 1 .. K1N_WAVES waves per workgroup, by the LDS a wave needs
    if (DIRECT) {
        for (uint32_t b = threadIdx.x; b < 256u; b += blockDim.x) {
            unsigned long long v = 0;
#pragma unroll
            for (int i = 0; i < 8; ++i) v |= ((b >> i) & 1u) ? 0xFFull << (8 * i) : 0ull;
            lut_ff[b] = v;
            lut_01[b] = v & 0x0101010101010101ull;
        }
        __syncthreads();
    }
    if (seg >= q.n_segs) return;
    const uint32_t n_rows = ROWS ? q.n_keys : 0u;                       // (the host picks the instantiation by the handle's row mode)
    unsigned char* wbase = lds_raw + k1n_wave_bytes(q.chain_cap, q.tbits, q.n_keys, n_rows) * wave;
    uint32_t* table = (uint32_t*)wbase;                                                      // open chunks
    ulonglong2* chain_m = (ulonglong2*)(wbase + arena_table_bytes(q.tbits, q.n_keys));      // [chain_cap] one slot per depth:
    uint32_t* chain_b = (uint32_t*)(chain_m + q.chain_cap);                                  // the latest node of that depth on the current root path
    const unsigned long long lt_mask = (1ull << lane) - 1ull;
    RowTab RT{nullptr, nullptr, 0u};
    if constexpr (ROWS) rowtab_init(RT, (uint32_t*)(wbase + (((size_t)q.chain_cap * 20 + 15) & ~(size_t)15) + arena_table_bytes(q.tbits, q.n_keys)), n_rows, lane);
    // the pool: what a record store reads is held, the rest is re-read from the parameter block where it is used (PoolRef)
    PoolRef pv{};
    pv.k = &((KARG(NParams))__builtin_amdgcn_kernarg_segment_ptr())->pool;
    pv.kbits = q.pool.kbits; pv.dbits = q.pool.dbits; pv.pshift = q.pool.pshift;
    if constexpr (ROWS) { pv.rec = q.pool.rec; pv.recw = q.pool.recw; } else { pv.wkey = q.pool.wkey; pv.wrec = q.pool.wrec; }
    const uint32_t first = seg * q.nseg_nodes;
    const uint32_t end = (q.P - first) < q.nseg_nodes ? q.P : first + q.nseg_nodes;

    auto locals = [&](uint32_t info, unsigned long long m0, uint32_t e1blk, unsigned long long e1mask) -> NSum {
        const uint32_t np = info >> 16;
        if (np == 0) return nsum_make(BNONE, 0ull, BNONE, 0ull, false);
        if (np == 1) return nsum_make(info & 0xFFFFu, m0, BNONE, 0ull, false);
        return nsum_make(info & 0xFFFFu, m0, e1blk, e1mask, np > 2);
    };

    // chain slots of the first node's ancestors: inclusive merge along the root path
    {
        KARG(NParams) qr = kernarg_reread<NParams>();                    // (once per slice: read where used, not held)
        const uint32_t d = qr->seg_anc_n[seg];
        NSum carry = nsum_make(BNONE, 0ull, BNONE, 0ull, false);
        for (uint32_t cb = 0; cb < d; cb += WAVE) {
            const uint32_t k = cb + lane;
            const bool on = k < d;
            NSum S = nsum_make(BNONE, 0ull, BNONE, 0ull, false);
            if (on) {
                const uint32_t node = qr->seg_anc[(size_t)seg * q.chain_cap + k];
                const uint32_t info = q.p0_info[node];
                uint32_t e1b = BNONE; unsigned long long e1m = 0;
                if ((info >> 16) > 1u) { const uint32_t po = q.pair_ofs[node]; e1b = q.pair_blk[po]; e1m = q.pair_mask[po]; }
                S = locals(info, q.p0_mask[node], e1b, e1m);
            }
            if (lane == 0) S = nsum_merge(carry, S);
#pragma unroll
            for (int s = 1; s < WAVE; s <<= 1) {
                const NSum o = nsum_shfl_up(S, s);
                if (lane >= (uint32_t)s) S = nsum_merge(o, S);
            }
            if (on) { chain_m[k] = make_ulonglong2(S.m0, S.m1); chain_b[k] = S.bw; }
            carry = nsum_shfl(S, WAVE - 1);
        }
        lds_sync();
    }

    // node records of the NEXT batch(es) are fetched while the current one is processed
    uint32_t nx_nl = 0, nx_w = 0, nx_info = 0, nx_df = 0, nx_e1b = BNONE, nx_po = 0;
    int32_t nx_par = -1;
    unsigned long long nx_m0 = 0, nx_e1m = 0;
    uint32_t n2_nl = 0, n2_w = 0, n2_info = 0, n2_df = 0x7FFFu, n2_po = 0;          // two batches ahead
    int32_t n2_par = -1;
    unsigned long long n2_m0 = 0;
    auto fetch2 = [&](uint32_t b0) {                                  // (pair_ofs of a node without further pairs is never written: whatever is read is not used)
        const uint32_t ii = b0 + lane;
        const bool v = ii < end;
        n2_nl = v ? q.nl[ii] : 0u;
        n2_w = v ? q.w[ii] : 0u;
        n2_par = v ? q.parent[ii] : -1;
        n2_df = v ? q.dflag[ii] : 0x7FFFu;
        n2_info = v ? q.p0_info[ii] : 0u;
        n2_m0 = v ? q.p0_mask[ii] : 0ull;
        n2_po = v ? q.pair_ofs[ii] : 0u;
    };
    auto advance = [&]() {                                            // the batch two ahead becomes the next one; its second pairs are requested
        nx_nl = n2_nl; nx_w = n2_w; nx_par = n2_par; nx_df = n2_df; nx_info = n2_info; nx_m0 = n2_m0; nx_po = n2_po;
        nx_e1b = BNONE; nx_e1m = 0;
        if ((nx_info >> 16) > 1u) { nx_e1b = q.pair_blk[nx_po]; nx_e1m = q.pair_mask[nx_po]; }
    };
    fetch2(first); advance();
    if (first + WAVE < end) fetch2(first + WAVE); else { n2_nl = 0; n2_w = 0; n2_par = -1; n2_df = 0x7FFFu; n2_info = 0; n2_m0 = 0; n2_po = 0; }
    WaveArena A;
    arena_init(A, table, MODE != 0 ? 0u : q.tbits, q.n_keys, seg, lane);
    // direct mode: the lower triangle of tile (curX, curX) — rows 0..31 x cols 0..31, rows 32..63 x cols 0..31, rows 32..63 x cols 32..63
    k2_v16i c00 = {}, c10 = {}, c11 = {};
    uint32_t curX = BNONE, n_direct = 0;
    uint32_t flat_n = 0;                                             // flat mode: records of the slice so far (wave-uniform)
    uint32_t n_flagged = 0;                                          // nodes with more than two blocks in the slice so far (wave-uniform)
    auto dflush = [&]() {
        // one HBM atomic per non-zero cell (D layout of the MFMA: col = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)).  Cell (rb + r, rb + c)
        // of the triangle sits at tri64(rb) + rb + [rb r + r (r - 1) / 2 + c]: a wave-uniform base and a 32-bit offset per lane
        const uint32_t half = lane >> 5, l31 = lane & 31u;
        const uint32_t rb = curX * q.bwidth;
        uint32_t* const Mb = q.M + (tri64((uint64_t)rb) + rb);
        const uint32_t lim = q.N - rb;                                  // rows of the block inside the matrix (masks never hold an id beyond N: belt and braces)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const uint32_t row0 = (uint32_t)((r & 3) + 8 * (r >> 2)) + 4u * half, row1 = row0 + 32u;
            const uint32_t o0 = rb * row0 + row0 * (row0 - 1u) / 2u + l31, o1 = rb * row1 + row1 * (row1 - 1u) / 2u + l31;
            const uint32_t v00 = (uint32_t)c00[r], v10 = (uint32_t)c10[r], v11 = (uint32_t)c11[r];
            if (v00 && l31 < row0 && row0 < lim) atomicAdd(Mb + o0, v00);
            if (v10 && row1 < lim) atomicAdd(Mb + o1, v10);
            if (v11 && l31 < row0 && row1 < lim) atomicAdd(Mb + o1 + 32u, v11);
            c00[r] = 0; c10[r] = 0; c11[r] = 0;
        }
        if (lane == 0 && q.touched) q.touched[tri32(curX) + curX] = 1;      // (all2all-sp scans only the tiles a call added to)
    };
    for (uint32_t base = first; base < end; base += WAVE) {
        const uint32_t idx = base + lane;
        const bool valid = idx < end;
        const uint32_t nl = nx_nl, w = nx_w, info = nx_info, df = nx_df, e1b = nx_e1b;
        const int32_t par = nx_par;
        const unsigned long long m0 = nx_m0, e1m = nx_e1m;
        if (base + WAVE < end) {
            advance();
            if (base + 2 * WAVE < end) fetch2(base + 2 * WAVE); else { n2_nl = 0; n2_w = 0; n2_par = -1; n2_df = 0x7FFFu; n2_info = 0; n2_m0 = 0; n2_po = 0; }
        }
        const uint32_t dep = df & 0x7FFFu;
        NSum S = locals(info, m0, e1b, e1m);
        if (valid && par >= 0 && par < (int32_t)base) {
            const ulonglong2 cm = chain_m[dep - 2u];
            S = nsum_merge(NSum{cm.x, cm.y, chain_b[dep - 2u]}, S);
        }
        // pointer doubling over the in-batch parents
        int pl = (valid && par >= (int32_t)base) ? (int)(par - (int32_t)base) : -1;
        while (__ballot(pl >= 0)) {
            const int src = pl >= 0 ? pl : (int)lane;
            const NSum o = nsum_shfl(S, src);
            if (pl >= 0) S = nsum_merge(o, S);
            const int npl = __shfl(pl, src, WAVE);
            pl = pl >= 0 ? npl : -1;
        }
        const bool wide = valid && ((S.bw >> 30) & 1u);
        const uint32_t w0 = S.bw & 0x7FFFu, w1 = (S.bw >> 15) & 0x7FFFu;
        const unsigned long long F0 = S.m0, F1 = w1 != BNONE ? S.m1 : 0ull;
        {
            // (the wide list's prefix sums start here: the flagged nodes of the slice so far, wave-uniform, beside the bits)
            const unsigned long long wb = __ballot(wide);
            if (lane == 0) { q.widebits[base >> 6] = wb; q.wide_base[base >> 6] = n_flagged; }
            n_flagged += (uint32_t)__popcll(wb);
        }
        if (__ballot(wide)) {
            // a node with more blocks whose parent still has at most two takes the parent's (blocks, masks) along: the wide
            // kernel starts its list from them
            const int pl0 = (valid && par >= (int32_t)base) ? (int)(par - (int32_t)base) : (int)lane;
            NSum Pp = nsum_shfl(S, pl0);
            if (valid && par >= 0 && par < (int32_t)base) { const ulonglong2 cm = chain_m[dep - 2u]; Pp = NSum{cm.x, cm.y, chain_b[dep - 2u]}; }
            if (wide && par >= 0 && !((Pp.bw >> 30) & 1u)) {
                const uint32_t pb0 = Pp.bw & 0x7FFFu, pb1 = (Pp.bw >> 15) & 0x7FFFu;
                q.fn_mask[idx] = make_ulonglong2(Pp.m0, pb1 != BNONE ? Pp.m1 : 0ull);
                q.fn_blk[idx] = (pb0 == BNONE ? 0xFFFFu : pb0) | ((pb1 == BNONE ? 0xFFFFu : pb1) << 16);
            }
        }
        // ---- records (flat form): (w0, w0, F0), and with a second block (w1, w0, F1, F0) and (w1, w1, F1).  A diagonal
        // record needs two ids to have a pair.
        const bool act = valid && !wide && w != 0 && nl >= 2u && w0 != BNONE && idx >= q.emit_lo && idx < q.emit_hi;
        auto first_block_records = [&]() {
            // (w0, w0, F0): the lanes of a batch mostly share the block — one reservation per block in that block's open chunk.
            // (In wide mode, q.all_wide, these records take the wide pool as well.)
            bool d0 = act && __popcll(F0) >= 2 && in_band(w0);
            if (FLAT) {
                // the slice's first-block records, compacted in DFS order: two coalesced stores, no reservation, no chunk table
                const bool dd = d0 && w < 128u;                          // (an int8 operand holds a weight below 128; the others take the sort)
                const unsigned long long bm = __ballot(dd);
                if (dd) {
                    const uint32_t slot = first + flat_n + (uint32_t)__popcll(bm & lt_mask);
                    q.dmask[slot] = F0; q.dwx[slot] = w | (w0 << 8);
                }
                flat_n += (uint32_t)__popcll(bm);
                d0 = d0 && !dd;
            }
            if (DIRECT) {
                const bool dd = d0 && w < 128u;                          // (an int8 operand holds a weight below 128; nearly every weight is)
                const unsigned long long pend = __ballot(dd);
                if (pend) {
                    // ONE tile per wave: the block of the slice's first such record.  (Switching tiles where a slice crosses from one root child's
                    // subtree into the next would put a second write-back — 48 conditional atomics — into the loop body; the straddling
                    // slices are 2 - 6 % of all, and what they hold of the other block takes the records' way.)
                    if (curX == BNONE) curX = bcast(w0, (uint32_t)__builtin_ctzll(pend));
                    const bool mine = dd && w0 == curX;
                    n_direct += (uint32_t)__popcll(__ballot(mine));
                    if (!(q.dbg & 2u)) {
                    const TrConst trc = tr_const(lane);                      // (ten registers: made here, not kept across the batch)
                    const unsigned long long Rt = transpose64(mine ? F0 : 0ull, trc);        // lane r: bit k <=> node k of the batch has id r of the block
                    unsigned long long ra0, ra1;
                    {
                        const auto a = __builtin_amdgcn_permlane32_swap((uint32_t)Rt, (uint32_t)Rt, false, false);                 // [0]: the lower half's words everywhere, [1]: the upper half's
                        const auto b = __builtin_amdgcn_permlane32_swap((uint32_t)(Rt >> 32), (uint32_t)(Rt >> 32), false, false);
                        ra0 = ((unsigned long long)b[0] << 32) | a[0];
                        ra1 = ((unsigned long long)b[1] << 32) | a[1];
                    }
                    wbuf[wave][lane] = (unsigned char)(mine ? w : 0u);
                    lds_sync();
                    const uint32_t half = lane >> 5;
                    auto spread = [&](unsigned long long word, uint32_t shift, const unsigned long long* lut) -> k2_v4i {
                        const uint32_t f = (uint32_t)(word >> shift) & 0xFFFFu;
                        k2_v4i r;
                        const unsigned long long lo = lut[f & 0xFFu], hi = lut[f >> 8];
                        r[0] = (int)(uint32_t)lo; r[1] = (int)(uint32_t)(lo >> 32); r[2] = (int)(uint32_t)hi; r[3] = (int)(uint32_t)(hi >> 32);
                        return r;
                    };
    #pragma unroll 1
                    for (uint32_t kh = 0; kh < 2; ++kh) {
                        const uint32_t shift = 32u * kh + 16u * half;            // nodes 32 kh + 16 half .. + 15 of the batch
                        k2_v4i a0 = spread(ra0, shift, lut_ff), a1 = spread(ra1, shift, lut_ff);
                        const k2_v4i b0 = spread(ra0, shift, lut_01), b1 = spread(ra1, shift, lut_01);
                        const k2_v4i wv = *(const k2_v4i*)(wbuf[wave] + shift);
                        a0 &= wv; a1 &= wv;
                        c00 = __builtin_amdgcn_mfma_i32_32x32x32_i8(a0, b0, c00, 0, 0, 0);
                        c10 = __builtin_amdgcn_mfma_i32_32x32x32_i8(a1, b0, c10, 0, 0, 0);
                        c11 = __builtin_amdgcn_mfma_i32_32x32x32_i8(a1, b1, c11, 0, 0, 0);
                    }
                    lds_sync();
                    }
                    d0 = d0 && !mine;                                        // what is left takes the records' way
                }
            }
            if (MODE == 0 && !q.all_wide) {
                unsigned long long pend = __ballot(d0);
                while (pend) {
                    const uint32_t X0 = bcast(w0, (uint32_t)__builtin_ctzll(pend));
                    const bool mine = d0 && w0 == X0;
                    const unsigned long long bc = __ballot(mine);
                    const Resv r = arena_reserve(A, q.pool, X0 - bxlo, tri32(X0) + X0 - bsbase, (uint32_t)__popcll(bc), lane);
                    if (mine) rec_store_diag(q.pool, resv_slot(r, (uint32_t)__popcll(bc & lt_mask)), F0, w);
                    pend &= ~bc;
                }
            } else {
                rec_emit<ROWS>(A, pv, RT, d0, w0 - bxlo, F0, F0, w, tri32(w0) + w0 - bsbase, lane, lt_mask);
            }
        };
        if (!DIRECT) first_block_records();
        // second blocks, (w1, w0, F1, F0) and (w1, w1, F1): the pairs differ from lane to lane, so these records go to the wide
        // pool in arrival order (one reservation for all lanes) and are grouped by the sort
        {
            const bool act2 = act && F1 != 0 && in_band(w1);
            if (__ballot(act2)) {
                rec_emit<ROWS>(A, pv, RT, act2, w1 - bxlo, F1, F0, w, tri32(w1) + w0 - bsbase, lane, lt_mask);
                rec_emit<ROWS>(A, pv, RT, act2 && __popcll(F1) >= 2, w1 - bxlo, F1, F1, w, tri32(w1) + w1 - bsbase, lane, lt_mask);
            }
        }
        // ---- chain slots for the next batch: the nodes on the root path of this batch's last node, i.e. the
        // lanes whose depth is smaller than the depth of every later lane
        if (base + WAVE < end) {
            uint32_t m = dep;
#pragma unroll
            for (int s = 1; s < WAVE; s <<= 1) {
                const uint32_t o = (uint32_t)__shfl_down((int)m, s, WAVE);
                if (lane + (uint32_t)s < (uint32_t)WAVE) m = o < m ? o : m;
            }
            uint32_t later = (uint32_t)__shfl_down((int)m, 1, WAVE);
            if (lane == (uint32_t)WAVE - 1u) later = 0xFFFFFFFFu;
            if (valid && dep < later) { chain_m[dep - 1u] = make_ulonglong2(S.m0, S.m1); chain_b[dep - 1u] = S.bw; }
            lds_sync();
        }
        // (direct mode: the matrix-core step comes last in the batch — nothing of the batch but F0, w0 and w is live beside its operands)
        if (DIRECT) first_block_records();
    }
    if (DIRECT && curX != BNONE && !(q.dbg & 1u)) dflush();
    KARG(NParams) qe = kernarg_reread<NParams>();                        // (the slice's end)
    if (DIRECT && lane == 0 && n_direct) atomicAdd(&qe->direct_ctr[(seg % KMDB_SUBPOOLS) * 16u], n_direct);
    if (FLAT && lane == 0) { qe->slice_cnt[seg] = flat_n; if (flat_n) atomicAdd(&qe->direct_ctr[(seg % KMDB_SUBPOOLS) * 16u], flat_n); }
    if (lane == 0) qe->wide_slice_cnt[seg] = n_flagged;
    if constexpr (MODE == 0) arena_finish(A, q.pool, lane);               // (the other modes open no stream chunk)
    if constexpr (ROWS) rowtab_finish(RT, pv, lane);
    else arena_finish_wide(A, pv, lane);
}
template <int MODE, int MINW, bool ROWS>
__global__ __launch_bounds__(WAVE * K1N_WAVES) __attribute__((amdgpu_waves_per_eu(MINW, 8))) void k1n_kernel(const NParams q) { k1n_body<MODE, ROWS, false>(q); }
// the band-emit instantiations (modes 0 and 2; compiled for four waves per SIMD as their counterparts are)
template <int MODE, bool ROWS>
__global__ __launch_bounds__(WAVE * K1N_WAVES) __attribute__((amdgpu_waves_per_eu(4, 8))) void k1n_band_kernel(const NParams q) { k1n_body<MODE, ROWS, true>(q); }

// ------------------------------------------------------------------------------------------
// K2d: the narrow kernel's first-block records, slice by slice
// ------------------------------------------------------------------------------------------
// Round 6.  The records (X, X, F0, w) of the nodes with at most two blocks are as clustered as records can be — a slice of the DFS stream is, but
// for 0.5 - 2 % of its records, ONE tile (profiles/r06_tile_locality.txt) — so they need no chunk table, no grouping and no tile in LDS: the narrow
// kernel leaves them compacted in DFS order (12 bytes per record, coalesced), and one wave per K2D_SLICES slices streams them through the
// matrix-core step of the apply kernels (bit transpose, byte spreading, six v_mfma_i32_32x32x32_i8 per 64 records: the lower triangle of the tile)
// with the tile in 48 accumulator registers, written back when the block changes: once per slice, nearly always.  Side stream, beside the wide
// kernel.  (The same step INSIDE the narrow kernel — k1n_kernel<1> — writes no record at all, but its 48 accumulators beside the narrow kernel's 95
// registers leave three waves per SIMD: the narrow kernel then takes 0.65 ms longer at C2 than this kernel costs beside the wide kernel:
// profiles/r06_j3, r06_j4.)
constexpr uint32_t K2D_SLICES = 2;
struct DParams {
    const unsigned long long* dmask;
    const uint32_t* dwx;
    const uint32_t* slice_cnt;
    uint32_t n_segs, nseg_nodes, slices;
    uint32_t* M;
    uint32_t N, bwidth;
    unsigned char* touched;
};
// (the kernel's body: BAND = false is k2d_kernel as it always was; BAND = true culls the tiles of block rows outside the band and windows the write-back)
template <bool BAND>
__device__ __forceinline__ void k2d_body(const DParams& q, const BandArg<BAND>& band) {
    __shared__ unsigned long long lut_ff[256], lut_01[256];       // byte b -> its 8 bits spread over 8 bytes (0xFF / 0x01 where set)
    __shared__ __attribute__((aligned(16))) unsigned char wbuf[4][64];
    {
        unsigned long long v = 0;
#pragma unroll
        for (int i = 0; i < 8; ++i) v |= ((threadIdx.x >> i) & 1u) ? 0xFFull << (8 * i) : 0ull;
        lut_ff[threadIdx.x] = v;
        lut_01[threadIdx.x] = v & 0x0101010101010101ull;
        __syncthreads();
    }
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t half = lane >> 5, l31 = lane & 31u;
    const uint32_t s0 = (blockIdx.x * 4u + wave) * q.slices;
    if (s0 >= q.n_segs) return;
    const uint32_t s1 = s0 + q.slices < q.n_segs ? s0 + q.slices : q.n_segs;
    const TrConst trc = tr_const(lane);
    auto spread = [&](unsigned long long word, uint32_t shift, const unsigned long long* lut) -> k2_v4i {
        const uint32_t f = (uint32_t)(word >> shift) & 0xFFFFu;
        k2_v4i r;
        const unsigned long long lo = lut[f & 0xFFu], hi = lut[f >> 8];
        r[0] = (int)(uint32_t)lo; r[1] = (int)(uint32_t)(lo >> 32); r[2] = (int)(uint32_t)hi; r[3] = (int)(uint32_t)(hi >> 32);
        return r;
    };
    // the 64 records of a step, one per lane (m, wx; pend: those not applied yet); the next step's are requested before this one is applied
    uint32_t s = s0, n = q.slice_cnt[s0], b = 0;
    auto skip_empty = [&]() { while (b >= n && s + 1u < s1) { ++s; n = q.slice_cnt[s]; b = 0; } };
    skip_empty();
    unsigned long long nm = 0; uint32_t nwx = 0;
    auto fetch = [&]() {
        nm = 0; nwx = 0;
        if (b + lane < n) { const size_t i = (size_t)s * q.nseg_nodes + b + lane; nm = q.dmask[i]; nwx = q.dwx[i]; }
    };
    if (b < n) fetch();
    unsigned long long m = 0, pend = 0;
    uint32_t wx = 0;
    auto next_step = [&]() -> bool {
        if (b >= n) return false;
        m = nm; wx = nwx;
        b += WAVE;
        skip_empty();
        if (b < n) fetch();
        pend = __ballot(m != 0ull);
        return true;
    };
    // One tile per turn of the outer loop: the accumulators are cleared at its top, take the records of block X0 for as many steps as the block lasts, and
    // are written back at its bottom.  (Cleared INSIDE a conditional write-back in the middle of the step loop, every accumulator was live on both sides of
    // the branch and the allocator kept two copies of the tile: 31 registers in scratch at 128, still 8 at 168.)
    for (;;) {
        while (!pend && next_step()) {}
        if (!pend) break;
        const uint32_t X0 = bcast(wx >> 8, (uint32_t)__builtin_ctzll(pend));
        bool culled = false;                                     // (wave-uniform) band: the tile's block row lies outside it — its records are passed over
        if constexpr (BAND) {
            culled = band_culls(band.w, X0);
            if (lane == 0) band_unit(band.w, blockIdx.x * 4u + wave, BU_SLICES, !culled);
        }
        k2_v16i c00 = {}, c10 = {}, c11 = {};
        for (;;) {
            const bool mine = ((pend >> lane) & 1ull) && (wx >> 8) == X0;
            const unsigned long long bm = __ballot(mine);
            if (!bm) break;                                      // the step's next record belongs to another tile
            pend &= ~bm;
            if constexpr (BAND) if (culled) { if (pend || !next_step()) break; continue; }
            const unsigned long long Rt = transpose64(mine ? m : 0ull, trc);        // lane r: bit k <=> record k of the step has id r of the block
            unsigned long long ra0, ra1;
            {
                const auto a = __builtin_amdgcn_permlane32_swap((uint32_t)Rt, (uint32_t)Rt, false, false);                 // [0]: the lower half's words everywhere, [1]: the upper half's
                const auto c = __builtin_amdgcn_permlane32_swap((uint32_t)(Rt >> 32), (uint32_t)(Rt >> 32), false, false);
                ra0 = ((unsigned long long)c[0] << 32) | a[0];
                ra1 = ((unsigned long long)c[1] << 32) | a[1];
            }
            wbuf[wave][lane] = (unsigned char)(mine ? (wx & 0xFFu) : 0u);
            lds_sync();
#pragma unroll 1
            for (uint32_t kh = 0; kh < 2; ++kh) {
                const uint32_t shift = 32u * kh + 16u * half;            // records 32 kh + 16 half .. + 15 of the step
                k2_v4i a0 = spread(ra0, shift, lut_ff), a1 = spread(ra1, shift, lut_ff);
                const k2_v4i b0 = spread(ra0, shift, lut_01), b1 = spread(ra1, shift, lut_01);
                const k2_v4i wv = *(const k2_v4i*)(wbuf[wave] + shift);
                a0 &= wv; a1 &= wv;
                c00 = __builtin_amdgcn_mfma_i32_32x32x32_i8(a0, b0, c00, 0, 0, 0);
                c10 = __builtin_amdgcn_mfma_i32_32x32x32_i8(a1, b0, c10, 0, 0, 0);
                c11 = __builtin_amdgcn_mfma_i32_32x32x32_i8(a1, b1, c11, 0, 0, 0);
            }
            lds_sync();
            if (pend || !next_step()) break;                     // records of another block left in the step, or the last step done
        }
        // write-back: one HBM atomic per non-zero cell (D layout of the MFMA: col = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)).  Cell (rb + r, rb + c)
        // of the triangle sits at tri64(rb) + rb + [rb r + r (r - 1) / 2 + c]: a wave-uniform base and a 32-bit offset per lane
        if constexpr (BAND) if (culled) continue;
        const uint32_t rb = X0 * q.bwidth;
        // (band: the base is relative to the band's first cell — it may lie in front of the buffer where the band starts inside this block; the row
        // window below is tested before any address made from it is used)
        uint32_t* Mb;
        if constexpr (BAND) Mb = q.M + ((int64_t)(tri64((uint64_t)rb) + rb) - (int64_t)band.w.cell_lo);
        else Mb = q.M + (tri64((uint64_t)rb) + rb);
        uint32_t lim = q.N - rb;                                        // rows of the block inside the matrix (masks never hold an id beyond N: belt and braces)
        uint32_t first = 0;                                             // band: the block's rows [first, lim) are the band's
        if constexpr (BAND) {
            first = band.w.row_lo > rb ? band.w.row_lo - rb : 0u;
            lim = band.w.row_hi - rb < lim ? band.w.row_hi - rb : lim;  // (row_hi > rb: the tile is not culled)
        }
        // (the lane's part of the 48 offsets and conditions does not depend on the tile: seen through, it is computed once before the loop and kept — some
        // hundred registers beside the 48 accumulators.  Behind the empty asm it is a few instructions per atomic, computed where it is used.)
        uint32_t h4 = 4u * half, lc = l31;
        asm volatile("" : "+v"(h4), "+v"(lc));
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const uint32_t row0 = (uint32_t)((r & 3) + 8 * (r >> 2)) + h4, row1 = row0 + 32u;
            const uint32_t o0 = rb * row0 + row0 * (row0 - 1u) / 2u + lc, o1 = rb * row1 + row1 * (row1 - 1u) / 2u + lc;
            const uint32_t v00 = (uint32_t)c00[r], v10 = (uint32_t)c10[r], v11 = (uint32_t)c11[r];
            if constexpr (BAND) {
                const bool in0 = row0 >= first && row0 < lim, in1 = row1 >= first && row1 < lim;
                if (v00 && lc < row0 && in0) atomicAdd(Mb + o0, v00);
                if (v10 && in1) atomicAdd(Mb + o1, v10);
                if (v11 && lc < row0 && in1) atomicAdd(Mb + o1 + 32u, v11);
            } else {
                if (v00 && lc < row0 && row0 < lim) atomicAdd(Mb + o0, v00);
                if (v10 && row1 < lim) atomicAdd(Mb + o1, v10);
                if (v11 && lc < row0 && row1 < lim) atomicAdd(Mb + o1 + 32u, v11);
            }
        }
        if (lane == 0 && q.touched) q.touched[tri32(X0) + X0] = 1;      // (all2all-sp scans only the tiles a call added to)
    }
}
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4, 8))) void k2d_kernel(const DParams q) { k2d_body<false>(q, BandArg<false>{}); }
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4, 8))) void k2d_band_kernel(const DParams q, const BandArg<true> band) { k2d_body<true>(q, band); }

// ------------------------------------------------------------------------------------------
// wide list: compaction of the flagged nodes
// ------------------------------------------------------------------------------------------
// The narrow kernel leaves, beside the bits, the flagged nodes of the slice before every word (wide_base) and the slice's total (slice_cnt): what is
// left of the prefix sums is the scan of the slice totals — some 50 000 numbers at C2 — in ONE workgroup: every wave takes a contiguous share, sums
// it (coalesced, eight loads under way: the kernel is one workgroup waiting for its loads), the 16 wave totals are scanned, and the wave goes over its share again with a wave scan per 64 totals.
// slice_base[s] = flagged nodes before slice s, slice_base[n_segs] = KCTR_NWIDE = wide_base[n_words] = all of them.
constexpr uint32_t WSL_THREADS = 1024;
__global__ __launch_bounds__(WSL_THREADS) void wide_slices_kernel(const uint32_t* __restrict__ slice_cnt, uint32_t n_segs, uint32_t* __restrict__ slice_base,
                                                                   uint32_t* __restrict__ wide_base, uint32_t n_words, uint32_t* __restrict__ counters) {
    __shared__ uint32_t wtot[WSL_THREADS / WAVE];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    constexpr uint32_t NW = WSL_THREADS / WAVE;
    const uint32_t share = ((n_segs + NW - 1u) / NW + 63u) & ~63u;          // a multiple of 64 per wave
    const uint32_t lo = wave * share < n_segs ? wave * share : n_segs;
    const uint32_t hi = n_segs - lo < share ? n_segs : lo + share;
    constexpr uint32_t U = 8;
    uint32_t sum = 0;
    for (uint32_t i0 = lo; i0 < hi; i0 += U * WAVE) {
        uint32_t v[U];
#pragma unroll
        for (uint32_t j = 0; j < U; ++j) { const uint32_t i = i0 + j * WAVE + lane; v[j] = i < hi ? slice_cnt[i] : 0u; }
#pragma unroll
        for (uint32_t j = 0; j < U; ++j) sum += v[j];
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) sum += (uint32_t)__shfl_xor((int)sum, d, WAVE);
    if (lane == 0) wtot[wave] = sum;
    __syncthreads();
    uint32_t run = 0, total = 0;
    for (uint32_t k = 0; k < NW; ++k) { const uint32_t t = wtot[k]; if (k < wave) run += t; total += t; }
    for (uint32_t i0 = lo; i0 < hi; i0 += U * WAVE) {
        uint32_t v[U];
#pragma unroll
        for (uint32_t j = 0; j < U; ++j) { const uint32_t i = i0 + j * WAVE + lane; v[j] = i < hi ? slice_cnt[i] : 0u; }
#pragma unroll
        for (uint32_t j = 0; j < U; ++j) {
            const uint32_t i = i0 + j * WAVE + lane;
            const uint32_t incl = wave_incl_scan(v[j], lane);
            if (i < hi) slice_base[i] = run + incl - v[j];
            run += bcast(incl, WAVE - 1u);
        }
    }
    if (threadIdx.x == 0) { slice_base[n_segs] = total; wide_base[n_words] = total; counters[KCTR_NWIDE] = total; }
}
// The wide list itself: word i's flagged nodes go to widx[slice_base[its slice] + wide_base[i] ...], and wide_base[i] becomes the absolute prefix the
// wide kernel reads.  A thread per word walks its bits.  (One wave per 64 words, lane k writing node k at its rank among the word's bits so that the stores
// of a word are contiguous, is 64 turns of a wave for 64 words against half a dozen per thread at C2, where most words hold a few flagged nodes: it measured
// slower beside k2d_kernel)  slice_shift: log2 of the words per slice (0xFFFFFFFF: not a power of two, divide).
__global__ __launch_bounds__(256) void wide_expand_kernel(const unsigned long long* __restrict__ bits, uint32_t* __restrict__ base, const uint32_t* __restrict__ slice_base,
                                                          uint32_t words_per_slice, uint32_t slice_shift, uint32_t n_words, uint32_t* __restrict__ widx, uint32_t cap) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    unsigned long long b = 0;
    uint32_t o = 0;
    if (i < n_words) {
        b = bits[i];
        o = slice_base[slice_shift != 0xFFFFFFFFu ? i >> slice_shift : i / words_per_slice] + base[i];
        base[i] = o;
    }
    while (b) {
        const uint32_t k = (uint32_t)__builtin_ctzll(b);
        b &= b - 1;
        if (o < cap) widx[o] = i * 64u + k;
        ++o;
    }
}

// ------------------------------------------------------------------------------------------
// K1w: nodes with more than two blocks
// ------------------------------------------------------------------------------------------
// Summary of a stretch of a root path as a list of (block, mask) entries: how many entries it has, its first and last block and
// the mask of its last entry.  Ids ascend along a root path, so two stretches can only share the block at their seam; stretches
// merge associatively (pointer doubling across lanes, scans along a path).
constexpr uint32_t BLK_NONE = 0xFFFFu;
struct LSum { unsigned long long lm; uint32_t c, fb, lb; };
__device__ __forceinline__ LSum lsum_none() { return LSum{0ull, 0u, BLK_NONE, BLK_NONE}; }
// A = the stretch closer to the root, B = the stretch below it
__device__ __forceinline__ LSum lsum_merge(const LSum& A, const LSum& B) {
    if (B.c == 0u) return A;
    if (A.c == 0u) return B;
    const bool seam = A.lb == B.fb;
    return LSum{(B.c == 1u && seam) ? (A.lm | B.lm) : B.lm, A.c + B.c - (seam ? 1u : 0u), A.fb, B.lb};
}
__device__ __forceinline__ LSum lsum_shfl(const LSum& s, int src) {
    return LSum{shfl64(s.lm, src), (uint32_t)__shfl((int)s.c, src, WAVE), (uint32_t)__shfl((int)s.fb, src, WAVE), (uint32_t)__shfl((int)s.lb, src, WAVE)};
}
__device__ __forceinline__ LSum lsum_shfl_up(const LSum& s, int d) {
    return LSum{shfl_up64(s.lm, d), (uint32_t)__shfl_up((int)s.c, d, WAVE), (uint32_t)__shfl_up((int)s.fb, d, WAVE), (uint32_t)__shfl_up((int)s.lb, d, WAVE)};
}
// the (blocks, masks) the narrow kernel left for a wide node whose parent has at most two blocks
__device__ __forceinline__ LSum lsum_of_fn(uint32_t fb, const ulonglong2& fm) {
    const uint32_t b0 = fb & 0xFFFFu, b1 = fb >> 16;
    if (b0 == BLK_NONE) return lsum_none();
    if (b1 == BLK_NONE) return LSum{fm.x, 1u, b0, b0};
    return LSum{fm.y, 2u, b0, b1};
}

// Second level above the block records.  A node whose full list has c >= min_blocks blocks would write c (c + 1) / 2 records; instead the wave
// that emits it takes a node index g, appends the node's c (g, block, mask) entries to an entry pool and sets bit g in the bitmap of every
// block of the list.  After the wide kernel: rank directories of the bitmaps, every entry placed in its block's list by its rank (no sort),
// and one job per tile (X, Y) that ANDs the two bitmaps, ranks the matches in both lists and feeds them, 64 at a time, to the apply step
// (l2_join_apply_kernel).  Prototype and measurements: profiles/r04_join_apply_probe.hip.
struct L2View {
    uint32_t on, min_blocks;
    uint32_t node_cap, W;          // node indices (a multiple of 64 * L2_SUB), bitmap words per block
    uint32_t ent_cap;              // entries (a multiple of L2_SUB)
    uint32_t* cursors;             // [2 * L2_SUB * 16]: node indices handed out per sub-range, then entries handed out per sub-range
    unsigned long long* bitmap;    // [blocks][W]
    uint32_t* ent_g;               // [ent_cap]
    uint16_t* ent_blk;             // [ent_cap], 0xFFFF: never written
    unsigned long long* ent_mask;  // [ent_cap]
    uint32_t* node_w;              // [node_cap]
};
struct WParams {
    const uint32_t* widx;          // the wide nodes, DFS order
    uint32_t n_wide;
    const uint32_t* nl;
    const int32_t* parent;
    const uint32_t* w;
    const uint16_t* dflag;
    const unsigned long long* widebits;
    const uint32_t* wide_base;     // [n_words + 1] wide nodes before every 64-node word of the DFS stream
    const unsigned long long* p0_mask;
    const uint32_t* p0_info;
    const uint32_t* pair_ofs;
    const uint16_t* pair_blk;
    const unsigned long long* pair_mask;
    const ulonglong2* fn_mask;
    const uint32_t* fn_blk;
    const uint32_t* seg_anc;       // [n_runs][chain_cap] root path of the first node of every run, root first (wrun_anc_kernel)
    const uint32_t* seg_anc_n;
    uint32_t run_nodes;            // wide nodes per run (a multiple of 64)
    uint32_t n_runs, n_waves;
    uint32_t* run_ctr;             // [K1W_CTRS * 16] next run of every class (run r belongs to class r % K1W_CTRS), a cache line apart
    uint32_t chain_cap, arena_cap, e_cap;
    uint32_t n_rows;               // row mode: block rows (0 otherwise)
    uint32_t emit_lo, emit_hi;
    PoolView pool;
    L2View l2;
    // band emit (k1w_band_kernel; no other instantiation reads these): as in NParams.  n_rows then counts the band's block rows.
    uint32_t band_xlo, band_xhi, band_sbase;
};
constexpr int K1W_WAVES = 2;
constexpr int K1W_MINW_FEW = 5;            // waves per SIMD the few-streams instantiation is compiled for (4 / 5 / 6 measured: DESIGN §8; 6 needs 52 bytes of scratch per lane)

constexpr uint32_t L2_MIN_BLOCKS = 24;     // nodes with that many blocks take the second level (measured at 10 000 samples: 11 -> 21.9 ms, 24 -> 20.0; KMDB_L2_MIN moves it)
constexpr uint32_t L2_NODE_GRAB = 16, L2_ENT_GRAB = 1024, L2_SUB = 16;   // node indices / entries a wave takes per device atomic, from one of L2_SUB cursors each
constexpr uint32_t K1W_QCAP = 64;          // inclusive record counts of the lanes of a batch (the owner search of the record-parallel emission)
constexpr uint32_t K1W_HEAVY = 11;         // a node with that many blocks (66 records and more) is emitted by the whole wave
constexpr uint32_t K1W_OXCAP = 96;         // further own pairs of a batch's nodes kept in LDS (with the queue and the node array trimmed the wave's LDS drops
                                           // below 10 KB at 200 blocks: 16 instead of 14 waves per CU — the kernel waits more than it issues)
constexpr uint32_t K1W_CTRS = 16;          // run counters: a wave takes its next run from the counter of its class
constexpr uint32_t K1W_ARENA_MIN = 256;    // entries of a wave's row arena at least (and always one full list: as many as there are blocks)
enum : uint32_t { WB_NONE = 0, WB_FN = 1, WB_LANE = 2, WB_CHAIN = 3 };
// LDS of one wave, carved from the dynamic allocation (the sizes depend on the database: blocks, depth of the tree)
struct K1WLds {
    unsigned long long* ent_mask;  // [arena_cap] rows of the batch's nodes, one contiguous run of entries per lane
    unsigned long long* e_mask;    // [e_cap] the chain list: the full list of the deepest node of the chain
    unsigned long long* ch_last;   // [chain_cap] per depth: the mask of the node's last entry (the chain list may hold more ids there)
    unsigned long long* own_m0;    // [64] first own pair of every lane's node
    unsigned long long* own_desc;  // [64] what a walk needs of the lane's node in ONE read: first own block | link << 16 (parent's lane, WB_LANE, or chain slot,
                                   //      WB_CHAIN) | ox << 32 (first copy of the further own pairs in ox_*, 0xFFFF: not copied) | own pairs << 48 | WB_* << 62
    uint32_t* ch_node;             // [chain_cap] the wide node of that depth on the current root path (0xFFFFFFFF: none)
    unsigned long long* ox_mask;   // [K1W_OXCAP] the batch's further own pairs (a copy: the walks read them once per descendant)
    uint32_t* own_po;              // [64] further own pairs: first entry in the pair pool
    uint32_t* st_w;                // [64]
    uint32_t* queue;               // [K1W_QCAP] (first 64: inclusive record counts of the lanes of a batch)
    uint16_t* ent_blk;             // [arena_cap]
    uint16_t* e_blk;               // [e_cap]
    uint16_t* ch_len;              // [chain_cap] entries of the node's list = a prefix of the chain list
    uint16_t* ox_blk;              // [K1W_OXCAP]
    uint16_t* st_start;            // [64] first arena entry of the lane's row
    uint16_t* st_pre;              // [64] entries of the lane's list that are NOT in its row: they are the first st_pre entries of the chain list
};
__host__ __device__ inline size_t k1w_core_bytes(uint32_t arena_cap, uint32_t e_cap, uint32_t chain_cap) {
    const size_t b = (size_t)8 * (arena_cap + e_cap + chain_cap + 2 * 64 + K1W_OXCAP) + (size_t)4 * (chain_cap + 2 * 64 + K1W_QCAP) +
                     (size_t)2 * (arena_cap + e_cap + chain_cap + 2 * 64 + K1W_OXCAP);
    return (b + 15) & ~(size_t)15;
}
__host__ __device__ inline size_t k1w_wave_bytes(uint32_t arena_cap, uint32_t e_cap, uint32_t chain_cap, uint32_t n_rows) {
    return k1w_core_bytes(arena_cap, e_cap, chain_cap) + rowtab_bytes(n_rows);
}
// The arrays of a fixed size come first: their addresses are the wave's base plus a constant, which the LDS instructions take as an immediate
// offset — only the seven arrays whose place depends on the database (arena_cap, e_cap, chain_cap) cost a register each.  Same bytes as before
// (k1w_core_bytes), every array aligned to its element.
__device__ __forceinline__ K1WLds k1w_carve(unsigned char* p, uint32_t arena_cap, uint32_t e_cap, uint32_t chain_cap) {
    K1WLds L;
    L.own_m0 = (unsigned long long*)p;  L.own_desc = L.own_m0 + 64;  L.ox_mask = L.own_desc + 64;
    L.own_po = (uint32_t*)(L.ox_mask + K1W_OXCAP);  L.st_w = L.own_po + 64;  L.queue = L.st_w + 64;
    L.st_start = (uint16_t*)(L.queue + K1W_QCAP);  L.st_pre = L.st_start + 64;  L.ox_blk = L.st_pre + 64;
    static_assert((4 * (64 + 64 + K1W_QCAP)) % 8 == 0 && (2 * (64 + 64 + K1W_OXCAP)) % 8 == 0, "the 8-byte arrays behind the fixed part stay aligned");
    L.ent_mask = (unsigned long long*)(L.ox_blk + K1W_OXCAP);  L.e_mask = L.ent_mask + arena_cap;  L.ch_last = L.e_mask + e_cap;
    L.ch_node = (uint32_t*)(L.ch_last + chain_cap);
    L.ent_blk = (uint16_t*)(L.ch_node + chain_cap);  L.e_blk = L.ent_blk + arena_cap;  L.ch_len = L.e_blk + e_cap;
    return L;
}

// root path of the first node of every run of the wide-node kernel (root first), by climbing the parent links: one thread per run,
// inside the call (the wide list depends on the decoded ids)
__global__ void wrun_anc_kernel(const uint32_t* __restrict__ widx, uint32_t n_wide, uint32_t run_nodes, const int32_t* __restrict__ parent,
                                const uint16_t* __restrict__ dflag, uint32_t chain_cap, uint32_t* __restrict__ anc, uint32_t* __restrict__ anc_n) {
    const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if ((uint64_t)r * run_nodes >= n_wide) return;
    int32_t cur = parent[widx[(size_t)r * run_nodes]];
    uint32_t d = cur < 0 ? 0u : (uint32_t)(dflag[cur] & 0x7FFFu);
    if (d > chain_cap) d = 0;
    anc_n[r] = d;
    while (cur >= 0 && d) { anc[(size_t)r * chain_cap + (--d)] = (uint32_t)cur; cur = parent[cur]; }
}

// One lane per wide node, batches of 64 consecutive nodes of the (DFS-ordered) wide list.  A run = a few consecutive batches;
// the waves take runs as they go (the records per node differ by orders of magnitude — 3 blocks: 6
// records, 200 blocks: 20 100 — and heavy nodes sit together in the DFS order).
// A wide node's parent is wide as well or has at most two blocks.  Its list = the parent's list + its own pairs:
//   parent with <= 2 blocks: the (blocks, masks) the narrow kernel left in HBM;
//   wide parent inside the batch: that lane (the lengths resolve by pointer doubling, the rows are filled by walking the in-batch
//   parents);
//   wide parent before the batch: the CHAIN — the wide nodes on the root path of the previous batch's last node.  Their lists are
//   prefixes of one another (ids ascend along a root path), so the chain is ONE list, the deepest node's, plus per depth the
//   number of entries and the mask of the node's own last entry.  At the start of a run the chain is built from the root path of
//   the slice's first node (a table made at upload): the lists of all its wide ancestors in one scan.
// No node climbs parent links, and a list may have as many entries as there are blocks.
// ROWS / L2: the record path of the call (few streams; row mode; row mode with the second level), chosen by the host: an instantiation holds
// neither the code nor the registers of the paths it does not take.
// (WParams must stay the kernel's ONLY argument: kernarg_reread<WParams>() and PoolRef::k read it at offset 0 of the kernarg segment)
// (few streams: pinned at five waves per SIMD — left to itself the allocator lands on either side of the 96 registers that five waves allow)
// The kernel's body.  BAND = false is k1w_kernel as it always was.  BAND = true (k1w_band_kernel) is the emit filter of a band call: the walk (chains, arenas,
// fn_*) is unchanged; a node's list is ascending in blocks, so its entries inside the band's block rows are ONE run [a_lo, a_hi) and its records are the
// pair indices t in [tri32(a_lo), tri32(a_hi)) of the triangular enumeration — the heavy form runs over that range, the record-parallel form takes its
// prefix sums over tri32(a_hi) - tri32(a_lo); a node with no entry in the band emits nothing.  The second level's entries are written as ever.
template <bool ROWS, bool L2, bool BAND>
__device__ __forceinline__ void k1w_body(const WParams& q) {
    static_assert(ROWS || !L2, "the second level runs in row mode only");
    const uint32_t bxlo = BAND ? q.band_xlo : 0u, bsbase = BAND ? q.band_sbase : 0u;
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    const uint32_t lane = lane_id();
    const uint32_t wave = threadIdx.x >> 6;
    const uint32_t wid = blockIdx.x * (blockDim.x >> 6) + wave;         // 1 or K1W_WAVES waves per workgroup, by the LDS a wave needs
    if (wid >= q.n_waves) return;
    unsigned char* wbase = lds_raw + k1w_wave_bytes(q.arena_cap, q.e_cap, q.chain_cap, ROWS ? q.n_rows : 0u) * wave;
    const K1WLds L = k1w_carve(wbase, q.arena_cap, q.e_cap, q.chain_cap);
    RowTab RT{nullptr, nullptr, 0u};
    if constexpr (ROWS) rowtab_init(RT, (uint32_t*)(wbase + k1w_core_bytes(q.arena_cap, q.e_cap, q.chain_cap)), q.n_rows, lane);
    // the pool: what a record store reads is held, the rest is re-read from the parameter block where it is used (PoolRef)
    PoolRef pv{};
    pv.k = &((KARG(WParams))__builtin_amdgcn_kernarg_segment_ptr())->pool;
    pv.kbits = q.pool.kbits; pv.dbits = q.pool.dbits; pv.pshift = q.pool.pshift;
    if constexpr (ROWS) { pv.rec = q.pool.rec; pv.recw = q.pool.recw; } else { pv.wkey = q.pool.wkey; pv.wrec = q.pool.wrec; }
    const unsigned long long lt_mask = (1ull << lane) - 1ull;
    WaveArena A;
    arena_init(A, nullptr, 0u, 0u, wid + 64u, lane);
    uint32_t n_miss = 0;

    uint32_t l2_nodes = 0;
    const uint32_t l2_min = L2 ? q.l2.min_blocks : 0u;
    uint32_t l2_gnext = 0, l2_gstock = 0, l2_enext = 0, l2_estock = 0;     // second level: the wave's stock of node indices and entries (wave-uniform)
    // record-parallel emission of the lanes in `on` (list of lane j: m entries from st_start[j]): a node with m blocks owns
    // m (m + 1) / 2 records (block pairs a >= b), one record per lane and step
    auto emit = [&](bool on, uint32_t m, uint32_t wv) {
        // a node with many blocks is taken by the whole wave: lane t builds pair t of the node
        {
            unsigned long long hb = __ballot(on && m >= K1W_HEAVY);
            while (hb) {
                const uint32_t j = (uint32_t)__builtin_ctzll(hb);
                hb &= hb - 1ull;
                const uint32_t mj = bcast(m, j), wj = bcast(wv, j);
                const uint32_t stj = L.st_start[j], prej = L.st_pre[j];
                // entry e of the node's list: the first prej from the chain list, the others from its row
                auto cmask = [&](uint32_t e) -> unsigned long long { return e < prej ? L.e_mask[e] : L.ent_mask[stj + e - prej]; };
                auto cblk = [&](uint32_t e) -> uint32_t { return e < prej ? (uint32_t)L.e_blk[e] : (uint32_t)L.ent_blk[stj + e - prej]; };
                if constexpr (L2) if (mj >= l2_min) {
                    KARG(WParams) ql = kernarg_reread<WParams>();                // (once per heavy node: the second level's arrays are read where used)
                    // second level: the node's entries instead of its records
                    const uint32_t sub = wid % L2_SUB;
                    if (l2_gstock == 0u) {
                        uint32_t b = 0;
                        if (lane == 0) b = atomicAdd(&ql->l2.cursors[sub * 16u], L2_NODE_GRAB);
                        b = bcast(b, 0);
                        // the grabs of the L2_SUB cursors interleave (grab n of cursor k = indices [(n L2_SUB + k) GRAB, + GRAB)): the indices in use
                        // stay dense from 0 on as long as the cursors advance alike, and the tile jobs scan the bitmaps only that far
                        const uint32_t g0 = ((b / L2_NODE_GRAB) * L2_SUB + sub) * L2_NODE_GRAB;
                        if (g0 + L2_NODE_GRAB <= ql->l2.node_cap) { l2_gnext = g0; l2_gstock = L2_NODE_GRAB; }
                    }
                    if (l2_estock < mj) {
                        uint32_t b = 0;
                        if (lane == 0) b = atomicAdd(&ql->l2.cursors[(L2_SUB + sub) * 16u], L2_ENT_GRAB);
                        b = bcast(b, 0);
                        if (b + L2_ENT_GRAB <= ql->l2.ent_cap / L2_SUB) { l2_enext = sub * (ql->l2.ent_cap / L2_SUB) + b; l2_estock = L2_ENT_GRAB; }
                        else l2_estock = 0u;
                    }
                    if (l2_gstock == 0u || l2_estock < mj) {             // out of indices or entries: the call is repeated with larger arrays
                        if (lane == 0) atomicOr(&ql->pool.counters[KCTR_L2_OVERFLOW], 1u);
                        continue;
                    }
                    const uint32_t g = l2_gnext;
                    ++l2_gnext; --l2_gstock;
                    for (uint32_t e = lane; e < mj; e += WAVE) {
                        const uint32_t idx = l2_enext + e, blk = cblk(e);
                        ql->l2.ent_g[idx] = g; ql->l2.ent_blk[idx] = (uint16_t)blk; ql->l2.ent_mask[idx] = cmask(e);
                        atomicOr(&ql->l2.bitmap[(size_t)blk * ql->l2.W + (g >> 6)], 1ull << (g & 63u));
                    }
                    l2_enext += mj; l2_estock -= mj;
                    if (lane == 0) ql->l2.node_w[g] = wj;
                    ++l2_nodes;
                    continue;
                }
                uint32_t T0 = 0, Tj = mj * (mj + 1u) / 2u;
                if constexpr (BAND) {
                    // the run of the node's entries inside the band's block rows (blocks ascend): entries below Xlo, entries up to Xhi
                    uint32_t a_lo = 0, a_hi = 0;
                    for (uint32_t e0 = 0; e0 < mj; e0 += WAVE) {
                        const uint32_t e = e0 + lane;
                        const uint32_t blk = e < mj ? cblk(e) : 0xFFFFFFFFu;
                        a_lo += (uint32_t)__popcll(__ballot(blk < q.band_xlo));
                        a_hi += (uint32_t)__popcll(__ballot(blk <= q.band_xhi));
                    }
                    T0 = tri32(a_lo); Tj = tri32(a_hi);
                }
                for (uint32_t t0 = T0; t0 < Tj; t0 += WAVE) {
                    const uint32_t t = t0 + lane;
                    bool rec_on = false;
                    uint32_t stream = 0, X = 0;
                    unsigned long long FX = 0, FY = 0;
                    if (t < Tj) {
                        uint32_t a = (uint32_t)((__fsqrt_rn(8.0f * (float)t + 1.0f) - 1.0f) * 0.5f);
                        while (tri32(a) > t) --a;
                        while (tri32(a + 1u) <= t) ++a;
                        const uint32_t b = t - tri32(a);
                        FX = cmask(a); FY = cmask(b);
                        X = cblk(a);
                        const uint32_t Y = cblk(b);
                        rec_on = a != b || __popcll(FX) >= 2;
                        if (a == b) FY = FX;
                        stream = tri32(X) + Y - bsbase;
                    }
                    rec_emit<ROWS>(A, pv, RT, rec_on, X - bxlo, FX, FY, wj, stream, lane, lt_mask);
                }
            }
            on = on && m < K1W_HEAVY;
        }
        // the others record by record: the records of the batch are numbered by a prefix sum over the lanes, lane t of a step finds
        // the owner of record t by a binary search in the prefix sums (LDS) and the pair (a, b) from the record's index inside the node.
        // (A queue of descriptors pushed by the owners cost a loop of up to 55 iterations per owner: 2/3 of the kernel's VALU work at
        // 10 000 samples.)
        uint32_t myrec = on ? m * (m + 1u) / 2u : 0u;
        uint32_t roff = 0;                                  // band: the node's first pair index inside the band, tri32(a_lo) <= 55
        if constexpr (BAND) {
            uint32_t a_lo = 0, a_hi = 0;
            if (on) {
                const uint32_t st = L.st_start[lane], pre = L.st_pre[lane];
                for (uint32_t e = 0; e < m; ++e) {
                    const uint32_t blk = e < pre ? (uint32_t)L.e_blk[e] : (uint32_t)L.ent_blk[st + e - pre];
                    a_lo += blk < q.band_xlo ? 1u : 0u;
                    a_hi += blk <= q.band_xhi ? 1u : 0u;
                }
            }
            roff = tri32(a_lo); myrec = tri32(a_hi) - roff;
        }
        const uint32_t rincl = wave_incl_scan(myrec, lane);
        const uint32_t T = bcast(rincl, WAVE - 1);
        // (band: the lane's first pair index rides in the upper half of its queue word — a batch holds fewer than 64 * 55 records)
        L.queue[lane] = BAND ? rincl | (roff << 16) : rincl;
        auto qcount = [&](uint32_t i) -> uint32_t { const uint32_t v = L.queue[i]; if constexpr (BAND) return v & 0xFFFFu; else return v; };
        L.st_w[lane] = wv;
        lds_sync();
        for (uint32_t t0 = 0; t0 < T; t0 += WAVE) {
            const uint32_t t = t0 + lane;
            bool rec_on = false, diag = false;
            uint32_t stream = 0, ww = 0, X = 0;
            unsigned long long FX = 0, FY = 0;
            if (t < T) {
                uint32_t own = 0;                               // the first lane whose inclusive sum exceeds t
#pragma unroll
                for (uint32_t sft = 32; sft >= 1u; sft >>= 1) if (qcount(own + sft - 1u) <= t) own += sft;
                uint32_t r0 = t - (own ? qcount(own - 1u) : 0u);
                if constexpr (BAND) r0 += L.queue[own] >> 16;
                uint32_t a = (uint32_t)((__fsqrt_rn(8.0f * (float)r0 + 1.0f) - 1.0f) * 0.5f);
                while (tri32(a) > r0) --a;
                while (tri32(a + 1u) <= r0) ++a;
                const uint32_t b = r0 - tri32(a);
                const uint32_t st = L.st_start[own], pre = L.st_pre[own];
                FX = a < pre ? L.e_mask[a] : L.ent_mask[st + a - pre]; FY = b < pre ? L.e_mask[b] : L.ent_mask[st + b - pre];
                X = a < pre ? (uint32_t)L.e_blk[a] : (uint32_t)L.ent_blk[st + a - pre];
                const uint32_t Y = b < pre ? (uint32_t)L.e_blk[b] : (uint32_t)L.ent_blk[st + b - pre];
                ww = L.st_w[own];
                diag = a == b;
                rec_on = !diag || __popcll(FX) >= 2;               // a diagonal record needs two ids to have a pair
                stream = tri32(X) + Y - bsbase;
            }
            // few streams: the step's records go to the wide pool in arrival order (one reservation for all lanes); many: to
            // the chunks of their block rows
            rec_emit<ROWS>(A, pv, RT, rec_on, X - bxlo, FX, diag ? FX : FY, ww, stream, lane, lt_mask);
        }
        lds_sync();
    };

    // The records per node differ by orders of magnitude (3 blocks: 6 records, 200 blocks: 20 100) and heavy nodes sit together
    // in the DFS order: runs dealt round-robin left some waves with several heavy runs (the kernel ended when the slowest wave did,
    // the average wave at half that time).  A wave takes its next run when it is done with one — from one of K1W_CTRS counters (a
    // single counter would be a hot address: same-address device atomics run at some ten million per second).
    for (;;) {
        uint32_t run = 0;
        KARG(WParams) qh = kernarg_reread<WParams>();                    // (once per run)
        const uint32_t n_cls = qh->n_waves < K1W_CTRS ? qh->n_waves : K1W_CTRS;       // classes of runs = counters in use (every class needs a wave)
        if (lane == 0) run = atomicAdd(&qh->run_ctr[(wid % n_cls) * 16u], 1u);
        run = bcast(run, 0) * n_cls + wid % n_cls;
        if (run >= qh->n_runs) break;
        const uint32_t kb = run * qh->run_nodes;
        const uint32_t ke = qh->n_wide - kb < qh->run_nodes ? qh->n_wide : kb + qh->run_nodes;
        // ---- the chain at the start of the run: the wide nodes on the root path of the run's first node.  Wide nodes are a
        // suffix of a root path; the topmost one starts from its (narrow) parent's (blocks, masks).
        {
            KARG(WParams) qr = kernarg_reread<WParams>();                // (once per run: read where used, not held)
            for (uint32_t e = lane; e < qr->chain_cap; e += WAVE) L.ch_node[e] = 0xFFFFFFFFu;
            const uint32_t d = qr->seg_anc_n[run];
            LSum carry = lsum_none();
            bool started = false;
            for (uint32_t cb = 0; cb < d; cb += WAVE) {
                const uint32_t j = cb + lane;
                const bool on = j < d;
                const uint32_t a = on ? qr->seg_anc[(size_t)run * qr->chain_cap + j] : 0u;
                const unsigned long long wb = __ballot(on && ((qr->widebits[a >> 6] >> (a & 63u)) & 1ull));
                if (!started && !wb) continue;
                const uint32_t t = started ? 0u : (uint32_t)__builtin_ctzll(wb);
                if (!started) {
                    const uint32_t at = bcast(a, t);
                    if (qr->parent[at] >= 0) {
                        const uint32_t fb = qr->fn_blk[at];
                        const ulonglong2 fm = qr->fn_mask[at];
                        carry = lsum_of_fn(fb, fm);
                        if (lane == 0) {
                            if (carry.c >= 1u) { L.e_blk[0] = (uint16_t)(fb & 0xFFFFu); L.e_mask[0] = fm.x; }
                            if (carry.c >= 2u) { L.e_blk[1] = (uint16_t)(fb >> 16); L.e_mask[1] = fm.y; }
                        }
                    }
                    started = true;
                }
                const bool act = on && lane >= t;
                const uint32_t info = act ? qr->p0_info[a] : 0u;
                const uint32_t np = info >> 16, b0 = info & 0xFFFFu;
                const unsigned long long m0 = act ? qr->p0_mask[a] : 0ull;
                const uint32_t po = np > 1u ? qr->pair_ofs[a] : 0u;
                uint32_t lb = b0;
                unsigned long long lm = m0;
                if (np > 1u) { lb = qr->pair_blk[po + np - 2u]; lm = qr->pair_mask[po + np - 2u]; }
                LSum S = np ? LSum{lm, np, b0, lb} : lsum_none();
                if (lane == t) S = lsum_merge(carry, S);
#pragma unroll
                for (int s = 1; s < WAVE; s <<= 1) {
                    const LSum o = lsum_shfl_up(S, s);
                    if (lane >= (uint32_t)s) S = lsum_merge(o, S);
                }
                LSum Pp = lsum_shfl_up(S, 1);
                if (lane == t) Pp = carry;
                const bool seam = act && np && Pp.c && Pp.lb == b0;
                const uint32_t idx0 = Pp.c - (seam ? 1u : 0u);
                if (act && np) {
                    if (!seam) { L.e_blk[idx0] = (uint16_t)b0; L.e_mask[idx0] = m0; }
                    for (uint32_t p = 1; p < np; ++p) { L.e_blk[idx0 + p] = qr->pair_blk[po + p - 1u]; L.e_mask[idx0 + p] = qr->pair_mask[po + p - 1u]; }
                }
                lds_sync();
                if (seam) atomicOr(&L.e_mask[idx0], m0);
                if (act) { L.ch_node[j] = a; L.ch_len[j] = (uint16_t)S.c; L.ch_last[j] = S.lm; }
                carry = lsum_shfl(S, WAVE - 1);
                lds_sync();
            }
            lds_sync();
        }
        // ---- the batches of the run
        for (uint32_t k0 = kb; k0 < ke; k0 += WAVE) {
            const uint32_t nv = ke - k0 < (uint32_t)WAVE ? ke - k0 : (uint32_t)WAVE;
            const bool valid = lane < nv;
            KARG(WParams) qb = kernarg_reread<WParams>();                // (once per batch: the node arrays' pointers are read where used, not held)
            const uint32_t node = valid ? qb->widx[k0 + lane] : 0u;
            const uint32_t nlv = valid ? qb->nl[node] : 0u;
            const uint32_t wv = valid ? qb->w[node] : 0u;
            const bool act = valid && wv != 0 && nlv >= 2u && node >= qb->emit_lo && node < qb->emit_hi;
            const int32_t par = valid ? qb->parent[node] : -1;
            const uint32_t dep = valid ? (uint32_t)(qb->dflag[node] & 0x7FFFu) : 0x7FFFu;
            const uint32_t info = valid ? qb->p0_info[node] : 0u;
            const uint32_t np = info >> 16, b0 = info & 0xFFFFu;
            const unsigned long long m0 = valid ? qb->p0_mask[node] : 0ull;
            // (every load that needs only `node` or `par` is requested here, whether its value will be used or not: the batch start is a chain of
            // dependent round trips — node, its fields, pair_ofs, the pairs; the parent's flags, then fn_* or wide_base — at four waves per SIMD.
            // pair_ofs of a node without further pairs and fn_* of a node with a wide parent were never written: what is read is not used.)
            const uint32_t po_raw = valid ? qb->pair_ofs[node] : 0u;
            const uint32_t fnb_raw = valid ? qb->fn_blk[node] : 0u;
            const ulonglong2 fnm_raw = valid ? qb->fn_mask[node] : make_ulonglong2(0ull, 0ull);
            const uint32_t pw = (valid && par >= 0) ? (uint32_t)par >> 6 : 0u;
            const unsigned long long pwbits = (valid && par >= 0) ? qb->widebits[pw] : 0ull;
            const uint32_t pwbase = (valid && par >= 0) ? qb->wide_base[pw] : 0u;
            const uint32_t po = np > 1u ? po_raw : 0u;
            uint32_t lb = b0;
            unsigned long long lm = m0;
            if (np > 1u) { lb = qb->pair_blk[po + np - 2u]; lm = qb->pair_mask[po + np - 2u]; }
            // ---- where the parent's list comes from
            uint32_t base = WB_NONE, link = 0, pre0 = 0;
            LSum Pb = lsum_none();
            if (valid && par >= 0) {
                if (!((pwbits >> ((uint32_t)par & 63u)) & 1ull)) {
                    base = WB_FN;
                    Pb = lsum_of_fn(fnb_raw, fnm_raw);
                } else {
                    const uint32_t prank = pwbase + (uint32_t)__popcll(pwbits & ((1ull << ((uint32_t)par & 63u)) - 1ull));
                    if (prank >= k0) { base = WB_LANE; link = prank - k0; }
                    else {
                        base = WB_CHAIN; link = dep - 2u;
                        if (link < qb->chain_cap && L.ch_node[link] == (uint32_t)par) {
                            const uint32_t cl = L.ch_len[link];
                            Pb = LSum{L.ch_last[link], cl, 0u, cl ? (uint32_t)L.e_blk[cl - 1u] : BLK_NONE};
                            pre0 = cl ? cl - 1u : 0u;              // all but the last entry of the chain node's list are taken from the chain list where they are
                        } else { base = WB_NONE; ++n_miss; }         // cannot happen (the engine treats it as an internal error)
                    }
                }
            }
            // ---- entries of every node's list: own stretch below the base, in-batch parents by pointer doubling
            LSum S = np ? LSum{lm, np, b0, lb} : lsum_none();
            if (base != WB_LANE) S = lsum_merge(Pb, S);
            // (pre: the shared prefix of the lane's TOPMOST in-batch ancestor — the lane whose base is not another lane)
            uint32_t pre = pre0, topl = lane;
            {
                int pl = base == WB_LANE ? (int)link : -1;
                while (__ballot(pl >= 0)) {
                    const int src = pl >= 0 ? pl : (int)lane;
                    const LSum o = lsum_shfl(S, src);
                    const int opl = __shfl(pl, src, WAVE);                // -1 once that lane's stretch reaches its base
                    const uint32_t opre = (uint32_t)__shfl((int)pre, src, WAVE);
                    const uint32_t otop = (uint32_t)__shfl((int)topl, src, WAVE);
                    if (pl >= 0) { S = lsum_merge(o, S); pl = opl; pre = opre; topl = otop; }
                }
            }
            // the (blocks, masks) the narrow kernel left for the topmost in-batch ancestor, fetched across the lanes NOW: a walk that ended in a
            // global load made every round of the batch wait for the record stores of the round before it (loads and stores return in order)
            const uint32_t tfnb = (uint32_t)__shfl((int)fnb_raw, (int)topl, WAVE);
            const unsigned long long tfnx = shfl64(fnm_raw.x, (int)topl), tfny = shfl64(fnm_raw.y, (int)topl);
            const uint32_t len = valid ? S.c : 0u;
            pre = valid ? pre : 0u;
            const uint32_t slen = len - pre;                               // entries of the lane's row
            L.own_m0[lane] = m0; L.own_po[lane] = po;
            {
                // the further own pairs, copied once: a node's pairs are read by every in-batch descendant's walk
                const uint32_t nx = np > 1u ? np - 1u : 0u;
                const uint32_t xincl = wave_incl_scan(nx, lane);
                const uint32_t x0 = xincl - nx;
                const bool fits = nx && xincl <= K1W_OXCAP;
                if (fits) for (uint32_t t = 0; t < nx; ++t) { L.ox_blk[x0 + t] = qb->pair_blk[po + t]; L.ox_mask[x0 + t] = qb->pair_mask[po + t]; }
                // (a walk over the in-batch parents reads one descriptor and one mask per node: the walks are chains of dependent LDS reads,
                // and five separate arrays made every step five of them — profiles/r05_j5: rows were 36 % of the kernel)
                L.own_desc[lane] = (unsigned long long)(b0 & 0xFFFFu) | ((unsigned long long)(link & 0xFFFFu) << 16) | ((unsigned long long)(fits ? x0 : 0xFFFFu) << 32) |
                                   ((unsigned long long)(np & 0x3FFFu) << 48) | ((unsigned long long)base << 62);
            }
            lds_sync();
            // ---- rows, as many lanes at a time as the arena holds, and their records.  Only the lanes that emit need a row, and
            // the last one (its list becomes the chain list).
            const bool need = valid && (act || lane == nv - 1u);
            uint32_t fin = 0, last_start = 0;
            while (fin < nv) {
                const uint32_t c = (lane >= fin && need) ? slen : 0u;
                const uint32_t incl = wave_incl_scan(c, lane);
                const unsigned long long over = __ballot(incl > qb->arena_cap);
                uint32_t hi = over ? (uint32_t)__builtin_ctzll(over) : (uint32_t)WAVE;
                if (hi <= fin) { if (lane == 0) atomicOr(&pool_cold(pv)->counters[KCTR_LIST_OVERFLOW], 1u); hi = fin + 1u; }     // a single list longer than the arena: cannot happen
                const bool on = need && lane >= fin && lane < hi && incl <= qb->arena_cap;
                const uint32_t start = incl - c;
                if (on) {
                    // fill the row right to left: own pairs, the in-batch parents' pairs, then the base
                    // (the entry being built stays in registers until the next block starts: no read-modify-write of the row)
                    uint32_t pos = start + slen, cur = 0xFFFFFFFFu;
                    unsigned long long curm = 0;
                    auto rflush = [&]() { if (cur != 0xFFFFFFFFu) { --pos; L.ent_blk[pos] = (uint16_t)cur; L.ent_mask[pos] = curm; } };
                    auto rpush = [&](uint32_t blk, unsigned long long mask) {
                        if (blk == cur) curm |= mask;
                        else { rflush(); cur = blk; curm = mask; }
                    };
                    uint32_t y = lane;
                    for (;;) {
                        const unsigned long long dsc = L.own_desc[y];
                        const unsigned long long ym0 = L.own_m0[y];
                        const uint32_t ynp = (uint32_t)(dsc >> 48) & 0x3FFFu, yb = (uint32_t)(dsc >> 62), ylink = (uint32_t)(dsc >> 16) & 0xFFFFu;
                        if (ynp > 1u) {
                            const uint32_t yox = (uint32_t)(dsc >> 32) & 0xFFFFu;
                            const uint32_t ynx = ynp - 1u;                       // (a node has fewer than 2897 pairs: fewer than 2^22 block pairs)
                            if (yox != 0xFFFFu) for (uint32_t t = ynx; t-- > 0u;) rpush(L.ox_blk[yox + t], L.ox_mask[yox + t]);
                            else {
                                const uint32_t ypo = L.own_po[y];
                                KARG(WParams) qp = kernarg_reread<WParams>();        // (the rare node whose further pairs found no room in ox_*)
                                for (uint32_t t = ynx; t-- > 0u;) rpush(qp->pair_blk[ypo + t], qp->pair_mask[ypo + t]);
                            }
                        }
                        if (ynp) rpush((uint32_t)dsc & 0xFFFFu, ym0);
                        if (yb == WB_LANE) { y = ylink; continue; }
                        if (yb == WB_FN) {                       // (y is the lane's topmost in-batch ancestor: topl)
                            if ((tfnb >> 16) != BLK_NONE) rpush(tfnb >> 16, tfny);
                            if ((tfnb & 0xFFFFu) != BLK_NONE) rpush(tfnb & 0xFFFFu, tfnx);
                        } else if (yb == WB_CHAIN) {
                            // the chain node's last entry (its mask may be the node's own: a deeper chain node can have more ids in that
                            // block); the entries before it stay in the chain list, shared by every lane that hangs below this node
                            const uint32_t cs = ylink;
                            const uint32_t cl = L.ch_len[cs];
                            if (cl) rpush(L.e_blk[cl - 1u], L.ch_last[cs]);
                        }
                        break;
                    }
                    rflush();
                }
                L.st_start[lane] = (uint16_t)start; L.st_pre[lane] = (uint16_t)pre;
                if (lane == nv - 1u && on) last_start = start;
                lds_sync();
                emit(on && act, len, wv);
                fin = hi;
            }
            // ---- the chain for the next batches: the lanes on the root path of the batch's last node, and that node's list
            {
                uint32_t mdep = dep;
#pragma unroll
                for (int sft = 1; sft < WAVE; sft <<= 1) {
                    const uint32_t o = (uint32_t)__shfl_down((int)mdep, sft, WAVE);
                    if (lane + (uint32_t)sft < (uint32_t)WAVE) mdep = o < mdep ? o : mdep;
                }
                uint32_t later = (uint32_t)__shfl_down((int)mdep, 1, WAVE);
                if (lane == (uint32_t)WAVE - 1u) later = 0xFFFFFFFFu;
                if (valid && dep < later && dep - 1u < qb->chain_cap) { L.ch_node[dep - 1u] = node; L.ch_len[dep - 1u] = (uint16_t)len; L.ch_last[dep - 1u] = S.lm; }
                // the last node's list becomes the chain list: its first entries are there already, its row follows them
                const uint32_t ll = bcast(slen, nv - 1u), ls = bcast(last_start, nv - 1u), lp = bcast(pre, nv - 1u);
                for (uint32_t e = lane; e < ll; e += WAVE) { L.e_blk[lp + e] = L.ent_blk[ls + e]; L.e_mask[lp + e] = L.ent_mask[ls + e]; }
                lds_sync();
            }
        }
    }
    arena_finish(A, pv, lane);
    if constexpr (ROWS) rowtab_finish(RT, pv, lane);
    else arena_finish_wide(A, pv, lane);
    if (lane == 0 && n_miss) atomicAdd(&pool_cold(pv)->counters[KCTR_SLOW], n_miss);
    if constexpr (L2) if (lane == 0 && l2_nodes) atomicAdd(&pool_cold(pv)->counters[KCTR_L2_NODES], l2_nodes);
}
template <bool ROWS, bool L2>
__global__ __launch_bounds__(WAVE * K1W_WAVES) __attribute__((amdgpu_waves_per_eu(ROWS ? 4 : K1W_MINW_FEW, 8))) void k1w_kernel(const WParams q) { k1w_body<ROWS, L2, false>(q); }
// the band-emit instantiations, compiled for the waves per SIMD of their counterparts
template <bool ROWS, bool L2>
__global__ __launch_bounds__(WAVE * K1W_WAVES) __attribute__((amdgpu_waves_per_eu(ROWS ? 4 : K1W_MINW_FEW, 8))) void k1w_band_kernel(const WParams q) { k1w_body<ROWS, L2, true>(q); }

// ------------------------------------------------------------------------------------------
// K2: records -> matrix
// ------------------------------------------------------------------------------------------
struct K2Item {
    uint32_t X, Y, count;                  // block pair, wave steps (64 records each) of this stream in the window
    const uint32_t* ids;                   // chunk mode: chunk ids of the run (LDS), CH_REC / 64 steps per chunk
    const uint32_t* fills;                 //             records in every chunk (LDS)
    const WideRec* srec;                   // sorted mode: the run's records, n_rec of them, contiguous
    const uint32_t* skey;                  //              their key words (weight digits)
    uint32_t kbits, dbits;
    uint32_t pshift;                       // sorted mode, != 0: packed records (PoolView::pshift): weight digit in the column word, no key words
    uint32_t rect_cols;                    // 0: lower-triangular matrix of N samples; else a dense n_rows x rect_cols matrix (db2db), N = n_rows
    uint32_t n_rec;
    const unsigned char* rec;              // record pool
    const uint32_t* recw;
};
constexpr uint32_t CH_STEPS = CH_REC / 64u;
// the 64 records of step st, one per lane (lanes beyond the fill get an empty record)
template <bool SORTED>
__device__ __forceinline__ void k2_fetch(const K2Item& it, bool diag, uint32_t st, uint32_t lane, bool weighted, unsigned long long& R,
                                         unsigned long long& Cc, uint32_t& W) {
    R = 0; Cc = 0; W = 0;
    if (st >= it.count) return;
    if (SORTED) {
        const uint32_t p = st * 64u + lane;
        if (p < it.n_rec) {
            const WideRec r = it.srec[p];
            R = r.rows; Cc = r.cols;
            if (it.pshift) {
                const uint32_t f = (uint32_t)(r.cols >> it.pshift), pd = 64u - it.pshift - 2u < 16u ? 64u - it.pshift - 2u : 16u;
                const uint32_t sh = (f >> pd) * pd;
                Cc = r.cols & ((1ull << it.pshift) - 1ull);
                W = sh < 32u ? (f & ((1u << pd) - 1u)) << sh : 0u;
            } else
            W = weighted ? wide_weight(it.skey[p], it.kbits, it.dbits) : 1u;
        }
    } else {
        const uint32_t ci = st / CH_STEPS, j = (st % CH_STEPS) * 64u + lane;
        if (j < it.fills[ci]) {
            const uint32_t id = it.ids[ci];
            const unsigned char* base = it.rec + ((size_t)id << (CH_SHIFT + 4));
            if (diag) { R = ((const unsigned long long*)base)[j]; Cc = R; }
            else { const ulonglong2 rc = ((const ulonglong2*)base)[j]; R = rc.x; Cc = rc.y; }
            W = weighted ? it.recw[((size_t)id << CH_SHIFT) + j] : 1u;
        }
    }
}

// The accumulation of a run on the matrix cores: over the 64 records of a step,
//     cell(r, c) += sum_k  w_k [r in rows_k] * [c in cols_k]    =  (A B)(r, c),   A = 64 x 64 int8 (rows x records, weighted),
//                                                                                B = 64 x 64 int8 (records x cols, 0/1)
// as eight v_mfma_i32_32x32x32_i8 (operand layout probed in profiles/r01_mfma_i8_layout_probe.hip: lane l holds
// A[l & 31][16 (l >> 5) + j], B[16 (l >> 5) + j][l & 31], j < 16; D: col = l & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (l >> 5)).
// The bit matrices R^T / C^T of the step are parked in LDS; a lane turns 16 of their bits into 16 operand bytes with two
// reads of a 256-entry byte-spreading table and ANDs the weights in.  An int8 operand holds a weight below 128: a larger
// weight is split into base-128 digits, the run is accumulated once per digit that occurs (`digit`), and the digit's tile is
// merged shifted left by 7 * digit — exact in the matrix's uint32 wrap-around arithmetic.  Almost every weight is below 128
// (99.98 % at the benchmark database), so nearly every run takes one pass.  Returns (to every thread) the OR of the weights.

template <bool DIAG, bool SORTED>
__device__ __forceinline__ uint32_t k2_apply_mfma(const K2Item& it, uint32_t digit, uint32_t* acc,
                                                  unsigned char (*wbuf)[64], const unsigned long long* lut_ff, const unsigned long long* lut_01) {
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t half = lane >> 5, l31 = lane & 31u;
    k2_v16i c00 = {}, c01 = {}, c10 = {}, c11 = {};
    auto spread = [&](unsigned long long word, uint32_t shift, const unsigned long long* lut) -> k2_v4i {
        const uint32_t f = (uint32_t)(word >> shift) & 0xFFFFu;
        k2_v4i r;
        const unsigned long long lo = lut[f & 0xFFu], hi = lut[f >> 8];
        r[0] = (int)(uint32_t)lo; r[1] = (int)(uint32_t)(lo >> 32); r[2] = (int)(uint32_t)hi; r[3] = (int)(uint32_t)(hi >> 32);
        return r;
    };
    unsigned long long nR = 0, nC = 0;
    uint32_t nW = 0, wor = 0;
    const TrConst trc = tr_const(lane);
    // this wave's steps: every fourth one; in chunk mode the steps past a chunk's fill are skipped without a fetch
    auto next_step = [&](uint32_t st) -> uint32_t {
        if (!SORTED) while (st < it.count && (st % CH_STEPS) * 64u >= it.fills[st / CH_STEPS]) st += 4;
        return st;
    };
    uint32_t cur = next_step(wave);
    k2_fetch<SORTED>(it, DIAG, cur, lane, true, nR, nC, nW);
    while (cur < it.count) {
        const unsigned long long R = nR, C = nC;
        const uint32_t W = nW;
        cur = next_step(cur + 4);
        k2_fetch<SORTED>(it, DIAG, cur, lane, true, nR, nC, nW);
        wor |= W;
        // lane r now holds row r of the step's bit matrices R^T / C^T (bit k <=> record k has row / column r).  The operand layout wants
        // in every lane the rows l31 and 32 + l31: the lower half of the wave keeps its own word and fetches the upper half's, and
        // the other way round — one v_permlane32_swap per 32-bit word, nothing parked in LDS (round 3 wrote the 64 words to LDS and read
        // four back per lane; with the byte-spreading table that made 25 LDS instructions per step and a third of the LDS cycles lost to
        // bank conflicts).
        const unsigned long long Ct = transpose64(C, trc);
        const unsigned long long Rt = DIAG ? Ct : transpose64(R, trc);           // on the diagonal rows == cols
        auto halves = [&](unsigned long long w, unsigned long long& w0, unsigned long long& w1) {
            const auto a = __builtin_amdgcn_permlane32_swap((uint32_t)w, (uint32_t)w, false, false);                 // [0]: the lower half's words everywhere, [1]: the upper half's
            const auto b = __builtin_amdgcn_permlane32_swap((uint32_t)(w >> 32), (uint32_t)(w >> 32), false, false);
            w0 = ((unsigned long long)b[0] << 32) | a[0];
            w1 = ((unsigned long long)b[1] << 32) | a[1];
        };
        unsigned long long ra0, ra1, cb0, cb1;
        halves(Rt, ra0, ra1);
        if (DIAG) { cb0 = ra0; cb1 = ra1; } else halves(Ct, cb0, cb1);
        wbuf[wave][lane] = (unsigned char)((W >> (7u * digit)) & 127u);
        lds_sync();
#pragma unroll
        for (uint32_t kh = 0; kh < 2; ++kh) {
            const uint32_t shift = 32u * kh + 16u * half;            // records 32 kh + 16 half .. + 15 of the step
            k2_v4i a0 = spread(ra0, shift, lut_ff), a1 = spread(ra1, shift, lut_ff);
            const k2_v4i b0 = spread(cb0, shift, lut_01), b1 = spread(cb1, shift, lut_01);
            const k2_v4i wv = *(const k2_v4i*)(wbuf[wave] + shift);
            a0 &= wv; a1 &= wv;
            c00 = __builtin_amdgcn_mfma_i32_32x32x32_i8(a0, b0, c00, 0, 0, 0);
            c01 = __builtin_amdgcn_mfma_i32_32x32x32_i8(a0, b1, c01, 0, 0, 0);
            c10 = __builtin_amdgcn_mfma_i32_32x32x32_i8(a1, b0, c10, 0, 0, 0);
            c11 = __builtin_amdgcn_mfma_i32_32x32x32_i8(a1, b1, c11, 0, 0, 0);
        }
        lds_sync();
    }
    // merge the four waves' tiles through the LDS block (on the diagonal only c < r)
    const uint32_t sh = 7u * digit;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const uint32_t row0 = (uint32_t)((r & 3) + 8 * (r >> 2)) + 4u * half;
        const uint32_t v00 = (uint32_t)c00[r] << sh, v01 = (uint32_t)c01[r] << sh, v10 = (uint32_t)c10[r] << sh, v11 = (uint32_t)c11[r] << sh;
        if (v00 && (!DIAG || l31 < row0)) atomicAdd(&acc[row0 * 64 + l31], v00);
        if (v01 && (!DIAG || 32u + l31 < row0)) atomicAdd(&acc[row0 * 64 + 32u + l31], v01);
        if (v10 && (!DIAG || l31 < 32u + row0)) atomicAdd(&acc[(32u + row0) * 64 + l31], v10);
        if (v11 && (!DIAG || l31 < row0)) atomicAdd(&acc[(32u + row0) * 64 + 32u + l31], v11);
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) wor |= (uint32_t)__shfl_xor((int)wor, d, WAVE);
    return wor;
}

// one run (the records of one block pair inside a window): accumulate, once per weight digit that occurs, and flush the tile
// (BAND: M is the band's buffer and a cell is written iff its row is one of the band's — BandWin; the callers cull the runs of other block rows before they get here)
template <bool SORTED, bool BAND = false>
__device__ __forceinline__ void k2_run(const K2Item& it, uint32_t* acc, uint32_t* wor_sh,
                                       unsigned char (*wbuf)[64], const unsigned long long* lut_ff, const unsigned long long* lut_01,
                                       uint32_t* __restrict__ M, uint32_t N, uint32_t bwidth, unsigned char* __restrict__ touched,
                                       const BandArg<BAND>& band = BandArg<BAND>{}) {
    for (uint32_t k = threadIdx.x; k < 64 * 64; k += 256) acc[k] = 0;
    if (threadIdx.x == 0) { *wor_sh = 0; if (touched && !it.rect_cols) touched[tri32(it.X) + it.Y] = 1; }      // (the tile gets something: all2all-sp scans only such tiles)
    __syncthreads();
    for (uint32_t digit = 0; digit < 5; ++digit) {
        const uint32_t wor = (it.X == it.Y && !it.rect_cols) ? k2_apply_mfma<true, SORTED>(it, digit, acc, wbuf, lut_ff, lut_01)
                                          : k2_apply_mfma<false, SORTED>(it, digit, acc, wbuf, lut_ff, lut_01);
        if ((threadIdx.x & 63u) == 0 && wor) atomicOr(wor_sh, wor);
        __syncthreads();
        if (digit == 4u || (*wor_sh >> (7u * (digit + 1u))) == 0) break;           // no weight has a higher digit (digit 4 is the last: a shift by 35 is not defined)
        __syncthreads();
    }
    // one HBM atomic per non-zero cell of the block
    __syncthreads();
    for (uint32_t k = threadIdx.x; k < 64 * 64; k += 256) {
        const uint32_t v = acc[k];
        if (!v) continue;
        const uint64_t row = (uint64_t)it.X * bwidth + (k >> 6), col = (uint64_t)it.Y * bwidth + (k & 63u);
        if constexpr (BAND) { if (row >= band.w.row_lo && row < band.w.row_hi && row < N && col < row) atomicAdd(&M[tri64(row) - band.w.cell_lo + col], v); }
        else
        if (it.rect_cols) { if (row < N && col < it.rect_cols) atomicAdd(&M[row * it.rect_cols + col], v); }
        else if (row < N && col < row) atomicAdd(&M[tri64(row) + col], v);
    }
    __syncthreads();
}

// ------------------------------------------------------------------------------------------
// second level above the block records: bitmaps -> rank directories -> lists -> tile joins (L2View; profiles/r04_join_apply_probe.hip)
// ------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t stream_row(uint32_t s);
// one workgroup per block: exclusive prefix popcounts of its W bitmap words, and the length of its list
__global__ __launch_bounds__(256) void l2_ranks_kernel(const unsigned long long* __restrict__ B, uint32_t W, uint32_t* __restrict__ R, uint32_t* __restrict__ len) {
    __shared__ uint32_t part[256];
    const unsigned long long* b = B + (size_t)blockIdx.x * W;
    uint32_t* r = R + (size_t)blockIdx.x * W;
    const uint32_t per = (W + 255u) / 256u, lo = threadIdx.x * per < W ? threadIdx.x * per : W, hi = lo + per < W ? lo + per : W;
    uint32_t s = 0;
    for (uint32_t w = lo; w < hi; ++w) s += (uint32_t)__popcll(b[w]);
    part[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x == 0) { uint32_t run = 0; for (uint32_t t = 0; t < 256; ++t) { const uint32_t v = part[t]; part[t] = run; run += v; } len[blockIdx.x] = run; }
    __syncthreads();
    uint32_t run = part[threadIdx.x];
    for (uint32_t w = lo; w < hi; ++w) { r[w] = run; run += (uint32_t)__popcll(b[w]); }
}
// list offsets; and loff[NB + 1] = bitmap words in use (the highest node index handed out, from the cursors' interleaved grabs)
__global__ void l2_offsets_kernel(const uint32_t* __restrict__ len, uint32_t NB, const uint32_t* __restrict__ cursors, uint32_t W, uint32_t* __restrict__ loff) {
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        uint32_t run = 0;
        for (uint32_t x = 0; x < NB; ++x) { loff[x] = run; run += len[x]; }
        loff[NB] = run;
        uint32_t top = 0;
        for (uint32_t k = 0; k < L2_SUB; ++k) {
            const uint32_t c = cursors[k * 16u];                 // indices this cursor handed out (a multiple of the grab)
            if (c) { const uint32_t end = ((c / L2_NODE_GRAB - 1u) * L2_SUB + k + 1u) * L2_NODE_GRAB; top = end > top ? end : top; }
        }
        const uint32_t wu = (top + 63u) / 64u;
        loff[NB + 1] = wu < W ? wu : W;
    }
}
// an entry's place in its block's list is its node's rank in the block's bitmap: no sort
__global__ void l2_lists_kernel(const uint32_t* __restrict__ ent_g, const uint16_t* __restrict__ ent_blk, const unsigned long long* __restrict__ ent_mask,
                                const uint32_t* __restrict__ node_w, uint32_t n, uint32_t W, const unsigned long long* __restrict__ B, const uint32_t* __restrict__ R,
                                const uint32_t* __restrict__ loff, unsigned long long* __restrict__ L, uint32_t* __restrict__ Wt, const uint32_t* __restrict__ cursors) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    // (the entry pool is sized with room to spare — four fifths of its slots were never handed out at 10 000 samples: a slot beyond its
    // sub-range's cursor is not even looked at)
    const uint32_t per_sub = n / L2_SUB, sub = i / per_sub;
    if (sub < L2_SUB && i - sub * per_sub >= cursors[(L2_SUB + sub) * 16u]) return;
    const uint32_t X = ent_blk[i];
    if (X == 0xFFFFu) return;                                 // a slot no wave wrote (the rest of a grab)
    const uint32_t g = ent_g[i];
    const unsigned long long word = B[(size_t)X * W + (g >> 6)];
    const uint32_t pos = loff[X] + R[(size_t)X * W + (g >> 6)] + (uint32_t)__popcll(word & ((1ull << (g & 63u)) - 1ull));
    L[pos] = ent_mask[i];
    Wt[pos] = node_w[g];
}
// One workgroup of four waves per tile (X, Y), X >= Y.  A lane ANDs one word of the two bitmaps (64 nodes), ranks every match in both lists
// and the wave queues (rank in L_X, rank in L_Y) in LDS, at most eight per lane and round; every 64 queued matches are one apply step — the
// masks and the weight gathered (the next step's while this one is applied), two bit transposes, byte spreading, eight MFMAs, as
// k2_apply_mfma does for 64 sorted records.  The queue's tail is drained by a last, empty round of the same loop (one call site of the step:
// inlined twice, the kernel ran at two waves per SIMD).  Weights of 128 and more: one join per base-128 digit that occurs.
// BAND (BandWin): a tile of a block row outside the band leaves before it reads a bitmap word or a list, and the write-back is windowed.
constexpr uint32_t L2_WAVES = 4, L2_QCAP = 576;
// (The whole-matrix form keeps its three waves per SIMD and the 11 registers in scratch it has there.  The band form asks for two: with the window's
// operands beside the join it would spill as well, and a band call runs the tiles of a few block rows — room per wave counts for more than waves.)
template <bool BAND>
__global__ __launch_bounds__(64 * L2_WAVES) __attribute__((amdgpu_waves_per_eu(BAND ? 2 : 3, 8)))
void l2_join_apply_kernel(const unsigned long long* __restrict__ B, const uint32_t* __restrict__ R, const unsigned long long* __restrict__ L, const uint32_t* __restrict__ Wt,
                          const uint32_t* __restrict__ loff, uint32_t w_stride, uint32_t nb_blocks, uint32_t* __restrict__ M, uint32_t N, uint32_t bwidth,
                          unsigned char* __restrict__ touched, const BandArg<BAND> band) {
    uint32_t W;
    __shared__ uint32_t q[L2_WAVES][L2_QCAP];
    __shared__ uint32_t q2[L2_WAVES][L2_QCAP];
    __shared__ unsigned long long lut_ff[256], lut_01[256];
    __shared__ uint32_t acc[64 * 64];
    __shared__ __attribute__((aligned(16))) unsigned char wbuf[L2_WAVES][64];
    __shared__ uint32_t wor_sh;
    const uint32_t t = band_stream(band, blockIdx.x);           // (band emit launches the band's tiles only, counted from its first stream)
    const uint32_t X = stream_row(t), Y = t - tri32(X);
    if (loff[X + 1] == loff[X] || loff[Y + 1] == loff[Y]) return;       // (uniform over the workgroup)
    if constexpr (BAND) {
        const bool culled = band_culls(band.w, X);
        if (threadIdx.x == 0) band_unit(band.w, t, BU_TILES, !culled);
        if (culled) return;
    }
    W = loff[nb_blocks + 1u];                       // the bitmap words in use (l2_offsets_kernel); rows of the bitmaps stay w_stride apart
    const bool diag = X == Y;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t half = lane >> 5, l31 = lane & 31u;
    {
        unsigned long long v = 0;
#pragma unroll
        for (int i = 0; i < 8; ++i) v |= ((threadIdx.x >> i) & 1u) ? 0xFFull << (8 * i) : 0ull;
        lut_ff[threadIdx.x] = v;
        lut_01[threadIdx.x] = v & 0x0101010101010101ull;
        for (uint32_t k = threadIdx.x; k < 64 * 64; k += 64 * L2_WAVES) acc[k] = 0;
        if (threadIdx.x == 0) wor_sh = 0;
        __syncthreads();
    }
    const unsigned long long* bx = B + (size_t)X * w_stride;
    const unsigned long long* by = B + (size_t)Y * w_stride;
    const uint32_t* rx = R + (size_t)X * w_stride;
    const uint32_t* ry = R + (size_t)Y * w_stride;
    const unsigned long long* lx = L + loff[X];
    const unsigned long long* ly = L + loff[Y];
    const uint32_t* wxl = Wt + loff[X];
    const TrConst trc = tr_const(lane);
    auto spread = [&](unsigned long long word, uint32_t shift, const unsigned long long* lut) -> k2_v4i {
        const uint32_t f = (uint32_t)(word >> shift) & 0xFFFFu;
        const unsigned long long lo = lut[f & 0xFFu], hi = lut[f >> 8];
        k2_v4i r;
        r[0] = (int)(uint32_t)lo; r[1] = (int)(uint32_t)(lo >> 32); r[2] = (int)(uint32_t)hi; r[3] = (int)(uint32_t)(hi >> 32);
        return r;
    };
    auto halves = [&](unsigned long long w, unsigned long long& w0, unsigned long long& w1) {
        const auto a = __builtin_amdgcn_permlane32_swap((uint32_t)w, (uint32_t)w, false, false);
        const auto b = __builtin_amdgcn_permlane32_swap((uint32_t)(w >> 32), (uint32_t)(w >> 32), false, false);
        w0 = ((unsigned long long)b[0] << 32) | a[0];
        w1 = ((unsigned long long)b[1] << 32) | a[1];
    };
    for (uint32_t digit = 0; digit < 5; ++digit) {
        k2_v16i c00 = {}, c01 = {}, c10 = {}, c11 = {};
        uint32_t qn = 0, wor = 0;                             // qn wave-uniform
        auto fetch = [&](uint32_t base, uint32_t n, unsigned long long& Rm, unsigned long long& Cm, uint32_t& Wg) {
            Rm = 0; Cm = 0; Wg = 0;
            if (lane < n) {
                const uint32_t a = q[wave][base + lane], b = q2[wave][base + lane];
                Rm = lx[a]; Cm = ly[b]; Wg = wxl[a];
            }
        };
        auto apply = [&](unsigned long long Rm, unsigned long long Cm, uint32_t Wg) {
            wor |= Wg;
            const unsigned long long Ct = transpose64(Cm, trc);
            const unsigned long long Rt = transpose64(Rm, trc);
            unsigned long long ra0, ra1, cb0, cb1;
            halves(Rt, ra0, ra1);
            halves(Ct, cb0, cb1);
            wbuf[wave][lane] = (unsigned char)((Wg >> (7u * digit)) & 127u);
            lds_sync();
#pragma unroll
            for (uint32_t kh = 0; kh < 2; ++kh) {
                const uint32_t shift = 32u * kh + 16u * half;
                k2_v4i a0 = spread(ra0, shift, lut_ff), a1 = spread(ra1, shift, lut_ff);
                const k2_v4i b0 = spread(cb0, shift, lut_01), b1 = spread(cb1, shift, lut_01);
                const k2_v4i wv = *(const k2_v4i*)(wbuf[wave] + shift);
                a0 &= wv; a1 &= wv;
                c00 = __builtin_amdgcn_mfma_i32_32x32x32_i8(a0, b0, c00, 0, 0, 0);
                c01 = __builtin_amdgcn_mfma_i32_32x32x32_i8(a0, b1, c01, 0, 0, 0);
                c10 = __builtin_amdgcn_mfma_i32_32x32x32_i8(a1, b0, c10, 0, 0, 0);
                c11 = __builtin_amdgcn_mfma_i32_32x32x32_i8(a1, b1, c11, 0, 0, 0);
            }
            lds_sync();
        };
        auto drain_steps = [&](bool all) {                    // the full steps of the queue; all: the partly filled last one too
            uint32_t head = 0;
            unsigned long long nR = 0, nC = 0; uint32_t nW = 0;
            auto avail = [&]() -> uint32_t { const uint32_t r = qn - head; return r >= 64u ? 64u : (all ? r : 0u); };
            if (avail()) fetch(0u, avail(), nR, nC, nW);
            while (avail()) {
                const unsigned long long Rm = nR, Cm = nC;
                const uint32_t Wg = nW;
                head += avail();
                if (avail()) fetch(head, avail(), nR, nC, nW);
                apply(Rm, Cm, Wg);
            }
            if (head) {
                const uint32_t rest = qn - head;
                uint32_t a = 0, b = 0;
                if (lane < rest) { a = q[wave][head + lane]; b = q2[wave][head + lane]; }
                lds_sync();
                if (lane < rest) { q[wave][lane] = a; q2[wave][lane] = b; }
                lds_sync();
                qn = rest;
            }
        };
        unsigned long long pwx = 0, pwy = 0; uint32_t pbx = 0, pby = 0;
        auto load_words = [&](uint32_t w0, unsigned long long& wx, unsigned long long& wy, uint32_t& bxr, uint32_t& byr) {
            const uint32_t w = w0 + lane;
            wx = 0; wy = 0; bxr = 0; byr = 0;
            if (w0 < W && w < W) { wx = bx[w]; wy = by[w]; bxr = rx[w]; byr = ry[w]; }
        };
        load_words(wave * 64u, pwx, pwy, pbx, pby);
        for (uint32_t w0 = wave * 64u;; w0 += 64u * L2_WAVES) {
            const bool last = w0 >= W;                        // one round past the bitmap: nothing to match, the queue's tail is drained
            const unsigned long long wx = pwx, wy = pwy;
            const uint32_t bxr = pbx, byr = pby;
            load_words(w0 + 64u * L2_WAVES, pwx, pwy, pbx, pby);
            unsigned long long m = wx & wy;
            do {
                const uint32_t left = (uint32_t)__popcll(m);
                const uint32_t k = left < 8u ? left : 8u;
                const uint32_t incl = wave_incl_scan(k, lane);
                const uint32_t total = bcast(incl, WAVE - 1);
                uint32_t pos = qn + incl - k;
                for (uint32_t j = 0; j < k; ++j) {
                    const uint32_t bit = (uint32_t)__builtin_ctzll(m);
                    m &= m - 1;
                    const unsigned long long below = (1ull << bit) - 1ull;
                    q[wave][pos] = bxr + (uint32_t)__popcll(wx & below); q2[wave][pos] = byr + (uint32_t)__popcll(wy & below);
                    ++pos;
                }
                qn += total;
                lds_sync();
                drain_steps(last);
            } while (__ballot(m != 0ull));
            if (last) break;
        }
        // the four waves' tiles merged in LDS, shifted by the digit's weight (on the diagonal only c < r)
        const uint32_t sh = 7u * digit;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const uint32_t row0 = (uint32_t)((r & 3) + 8 * (r >> 2)) + 4u * half;
            const uint32_t v00 = (uint32_t)c00[r] << sh, v01 = (uint32_t)c01[r] << sh, v10 = (uint32_t)c10[r] << sh, v11 = (uint32_t)c11[r] << sh;
            if (v00 && (!diag || l31 < row0)) atomicAdd(&acc[row0 * 64 + l31], v00);
            if (v01 && (!diag || 32u + l31 < row0)) atomicAdd(&acc[row0 * 64 + 32u + l31], v01);
            if (v10 && (!diag || l31 < 32u + row0)) atomicAdd(&acc[(32u + row0) * 64 + l31], v10);
            if (v11 && (!diag || l31 < row0)) atomicAdd(&acc[(32u + row0) * 64 + 32u + l31], v11);
        }
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) wor |= (uint32_t)__shfl_xor((int)wor, d, WAVE);
        if (lane == 0 && wor) atomicOr(&wor_sh, wor);
        __syncthreads();
        if (digit == 4u || (wor_sh >> (7u * (digit + 1u))) == 0) break;      // no weight has a higher digit (digit 4 is the last: a shift by 35 is not defined)
        __syncthreads();
    }
    // one HBM atomic per non-zero cell of the tile (the apply kernels add into the same matrix)
    if (threadIdx.x == 0 && touched) touched[t] = 1;
    for (uint32_t k = threadIdx.x; k < 64 * 64; k += 64 * L2_WAVES) {
        const uint32_t v = acc[k];
        if (!v) continue;
        const uint64_t row = (uint64_t)X * bwidth + (k >> 6), col = (uint64_t)Y * bwidth + (k & 63u);
        if constexpr (BAND) { if (row >= band.w.row_lo && row < band.w.row_hi && row < N && col < row) atomicAdd(&M[tri64(row) - band.w.cell_lo + col], v); }
        else if (row < N && col < row) atomicAdd(&M[tri64(row) + col], v);
    }
}

constexpr uint32_t K2_WIN = 32;            // sorted chunks per workgroup at most; the launch picks 16 (few streams: measured better) or 32
constexpr int K2A_MIN_WAVES = 3;
// (BAND, BandWin: a run of the window whose key names a block row outside the band is passed over before one of its records is read)
template <bool BAND>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(K2A_MIN_WAVES, 8))) void k2_apply_kernel(const unsigned char* __restrict__ rec, const uint32_t* __restrict__ recw,
                                                       const uint32_t* __restrict__ sorted_key, const uint32_t* __restrict__ sorted_id,
                                                       const uint32_t* __restrict__ chunk_fill, uint32_t n_states, const uint32_t* __restrict__ n_chunks_ptr,
                                                       uint32_t* __restrict__ M, uint32_t N, uint32_t bwidth, uint32_t win, unsigned char* __restrict__ touched,
                                                       const BandArg<BAND> band) {
    __shared__ uint32_t acc[64 * 64];
    __shared__ __attribute__((aligned(16))) unsigned char wbuf[4][64];
    __shared__ unsigned long long lut_ff[256], lut_01[256];       // byte b -> its 8 bits spread over 8 bytes (0xFF / 0x01 where set)
    __shared__ uint32_t s_key[K2_WIN], s_id[K2_WIN], s_fill[K2_WIN];
    __shared__ uint32_t wor_sh;
    // the window: K2_WIN chunks of the grouped chunk table; its head [0, *n_chunks_ptr) holds the stream chunks
    if (threadIdx.x < win) {
        const uint32_t j = blockIdx.x * win + threadIdx.x;
        const uint32_t key = j < *n_chunks_ptr ? sorted_key[j] : n_states;
        const uint32_t id = key < n_states ? sorted_id[j] : 0u;
        s_key[threadIdx.x] = key; s_id[threadIdx.x] = id; s_fill[threadIdx.x] = key < n_states ? chunk_fill[id] : 0u;
    }
    {
        unsigned long long v = 0;
#pragma unroll
        for (int i = 0; i < 8; ++i) v |= ((threadIdx.x >> i) & 1u) ? 0xFFull << (8 * i) : 0ull;
        lut_ff[threadIdx.x] = v;
        lut_01[threadIdx.x] = v & 0x0101010101010101ull;
    }
    __syncthreads();
    uint32_t a = 0;
    while (a < win && s_key[a] < n_states) {
        // one run of the window = the chunks of one stream
        const uint32_t key = s_key[a];
        uint32_t b = a + 1;
        while (b < win && s_key[b] == key) ++b;
        K2Item it;
        {
            const uint32_t bucket = band_stream(band, key);
            uint32_t X = (uint32_t)((__fsqrt_rn(8.0f * (float)bucket + 1.0f) - 1.0f) * 0.5f);
            while (tri32(X) > bucket) --X;
            while (tri32(X + 1u) <= bucket) ++X;
            it.X = X; it.Y = bucket - tri32(X);
            it.count = (b - a) * CH_STEPS; it.ids = s_id + a; it.fills = s_fill + a; it.srec = nullptr; it.n_rec = 0; it.rec = rec; it.recw = recw; it.rect_cols = 0; it.pshift = 0;
        }
        if constexpr (BAND) {
            const bool culled = band_culls(band.w, it.X);
            if (threadIdx.x == 0) band_unit(band.w, blockIdx.x, BU_RUNS, !culled);
            if (culled) { a = b; continue; }
        }
        k2_run<false, BAND>(it, acc, &wor_sh, wbuf, lut_ff, lut_01, M, N, bwidth, touched, band);
        a = b;
    }
}

// chunks of the chunk pool in use = the busiest sub-pool's share of all (one wave: a maximum over the 256 cursors)
__global__ void pool_used_kernel(const uint32_t* __restrict__ sub_cursor, const uint32_t* __restrict__ direct_ctr, uint32_t* __restrict__ counters) {
    uint32_t mx = 0, nd = 0;
    for (uint32_t p = threadIdx.x; p < KMDB_SUBPOOLS; p += 64u) { mx = max(mx, sub_cursor[p * 16u]); nd += direct_ctr[p * 16u]; }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) { mx = max(mx, (uint32_t)__shfl_xor((int)mx, d, WAVE)); nd += (uint32_t)__shfl_xor((int)nd, d, WAVE); }
    if (threadIdx.x == 0) { counters[KCTR_POOL_USED] = mx * KMDB_SUBPOOLS; counters[KCTR_DIRECT] = nd; }
}
// chunks of the wide pool in use, the same way (one wave) — and the 256 cursors side by side, clamped to the chunks a sub-pool holds, for the sort
// (cs_chunks_handed)
__global__ void count_raw_kernel(const uint32_t* __restrict__ wsub_cursor, uint32_t wsub_cap, uint32_t* __restrict__ counters, uint32_t* __restrict__ handed) {
    uint32_t mx = 0;
    for (uint32_t p = threadIdx.x; p < KMDB_SUBPOOLS; p += 64u) { const uint32_t c = wsub_cursor[p * 16u]; mx = max(mx, c); handed[p] = c < wsub_cap ? c : wsub_cap; }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) mx = max(mx, (uint32_t)__shfl_xor((int)mx, d, WAVE));
    if (threadIdx.x == 0) counters[KCTR_RAW] = mx * KMDB_SUBPOOLS;                    // chunk ids below this bound cover every written record
}

// Counting sort of the wide pool by stream: per-workgroup histograms in LDS (no device atomics), one exclusive scan over the
// table of counts, then every workgroup moves its records to its own range of every stream.  The order inside a stream is
// arbitrary (uint32 adds commute).  Two reads of the keys, one read and one write of the records per pass.
// One pass, bins = streams, for up to CS_MAX_KEYS of them: with more (10 000 samples at width 50 are 20 100 streams) a tile holds
// less than one record per stream and a scatter straight to that many destinations is bound by the number of write requests
// (measured: 25.8 ms for 495 M records).  The all2all call then takes the many-streams path (row chunks, rg_* and rs_* below);
// db2db (kmdb_rect_sort_apply) keeps rocPRIM's radix sort for more than CS_MAX_KEYS streams.
constexpr uint32_t CS_MAX_KEYS = 2048;
constexpr uint32_t CS_BLOCKS_ONE = 3072;   // workgroups of the sort (two full rounds on the chip measured better than 2048)
// block row X of stream s = tri32(X) + Y
__device__ __forceinline__ uint32_t stream_row(uint32_t s) {
    uint32_t X = (uint32_t)((__fsqrt_rn(8.0f * (float)s + 1.0f) - 1.0f) * 0.5f);
    while (tri32(X) > s) --X;
    while (tri32(X + 1u) <= s) ++X;
    return X;
}
// what one workgroup sorts: records [lo, hi); count / offset of bin (= stream) k at table[tab + k * gridDim.x]
struct CsJob { uint32_t lo, hi, tab; };
__device__ __forceinline__ CsJob cs_job(uint32_t n) {
    // equal shares of whole 1024-record tiles; the shares in XCD-contiguous order (the grids are multiples of 8)
    const uint32_t vb = (gridDim.x & 7u) ? blockIdx.x : xcd_contiguous(blockIdx.x, gridDim.x);
    CsJob j{0u, 0u, vb};
    const uint32_t per_block = ((n + gridDim.x - 1u) / gridDim.x + 1023u) / 1024u * 1024u;
    const uint32_t lo = vb * per_block;
    if (lo < n) { j.lo = lo; j.hi = n - lo < per_block ? n : lo + per_block; }
    return j;
}
__device__ __forceinline__ uint32_t cs_bin(uint32_t key, uint32_t n_valid) { return key < n_valid ? key : 0xFFFFFFFFu; }
// The all2all call's wide pool (wcur != nullptr: the chunks handed out by each of its 256 sub-pools, count_raw_kernel) comes WITHOUT pre-filled key
// words: a slot counts only if its chunk was handed out — chunk c is number c / KMDB_SUBPOOLS of sub-pool c % KMDB_SUBPOOLS (arena_take_wide), handed out
// iff that number lies below the sub-pool's cursor; what a wave took and did not write holds KEY_NONE (arena_finish_wide).  The cursors are loaded
// into LDS once per workgroup; per 2048 slots — 32 chunks, the workgroups' shares start at multiples of 1024 slots — one LDS read and a ballot give the
// wave a 32-bit mask, the test of a thread's slot is a bit of it (the four waves of a pass of 256 slots hold one chunk each).
__device__ __forceinline__ void cs_load_cursors(uint32_t* cur, const uint32_t* __restrict__ wcur) {
    if (!wcur) return;
    for (uint32_t k = threadIdx.x; k < KMDB_SUBPOOLS; k += blockDim.x) cur[k] = wcur[k];
    __syncthreads();
}
__device__ __forceinline__ uint32_t cs_chunks_handed(const uint32_t* cur, bool masked, uint32_t t0) {
    if (!masked) return 0xFFFFFFFFu;
    const uint32_t c = (t0 >> WCH_SHIFT) + (threadIdx.x & 31u);
    return (uint32_t)__ballot(c / KMDB_SUBPOOLS < cur[c % KMDB_SUBPOOLS]);
}
static_assert(WCH_REC == 64, "cs_chunks_handed: a wave's 64 consecutive slots are one chunk of the wide pool");
__global__ __launch_bounds__(256) void cs_hist_kernel(const uint32_t* __restrict__ wkey, uint32_t n, uint32_t n_valid, uint32_t n_keys,
                                                     uint32_t kmask, uint32_t* __restrict__ H, const uint32_t* __restrict__ wcur) {
    extern __shared__ uint32_t cs_lds[];
    __shared__ uint32_t cs_cur[KMDB_SUBPOOLS];
    const CsJob job = cs_job(n);
    cs_load_cursors(cs_cur, wcur);
    for (uint32_t k = threadIdx.x; k < n_keys; k += blockDim.x) cs_lds[k] = 0;
    __syncthreads();
    const uint32_t wv = threadIdx.x >> 6;
    // eight key words per thread requested together (the loop used to wait for one load per iteration)
    for (uint32_t i0 = job.lo; i0 < job.hi; i0 += 8u * blockDim.x) {
        const uint32_t handed = cs_chunks_handed(cs_cur, wcur != nullptr, i0);
        uint32_t kw[8];
#pragma unroll
        for (uint32_t j = 0; j < 8; ++j) {
            const uint32_t i = i0 + j * blockDim.x + threadIdx.x;
            kw[j] = (i < job.hi && ((handed >> (4u * j + wv)) & 1u)) ? wkey[i] : 0xFFFFFFFFu;
        }
#pragma unroll
        for (uint32_t j = 0; j < 8; ++j) {
            const uint32_t bin = kw[j] == 0xFFFFFFFFu ? 0xFFFFFFFFu : cs_bin(kw[j] & kmask, n_valid);
            if (bin < n_keys) atomicAdd(&cs_lds[bin], 1u);
        }
    }
    __syncthreads();
    for (uint32_t k = threadIdx.x; k < n_keys; k += blockDim.x) H[(size_t)job.tab + (size_t)k * gridDim.x] = cs_lds[k];
    if (blockIdx.x == 0 && threadIdx.x == 0) H[(size_t)n_keys * gridDim.x] = 0;          // the scan leaves the total here
}
// The scatter stages tiles of CS_TILE records in LDS sorted by bin, so that the records of one stream leave the tile as one
// contiguous burst.  LDS: the staged records, their destinations, and three per-bin arrays (tile histogram = rank source,
// tile offsets, the workgroup's running global cursor).
constexpr uint32_t CS_TILE = 2048, CS_THREADS = 256;
__host__ __device__ inline size_t cs_scatter_lds(uint32_t n_keys, bool packed) { return (size_t)CS_TILE * (sizeof(WideRec) + (packed ? 4 : 8)) + (size_t)n_keys * 12 + CS_THREADS * 4 + 64; }
__global__ __launch_bounds__(CS_THREADS) void cs_scatter_kernel(const uint32_t* __restrict__ wkey, const WideRec* __restrict__ wrec, uint32_t n, uint32_t n_valid,
                                                         uint32_t n_keys, uint32_t kmask, const uint32_t* __restrict__ O,
                                                         uint32_t* __restrict__ swkey, WideRec* __restrict__ swrec, uint32_t packed,
                                                         const uint32_t* __restrict__ wcur) {
    extern __shared__ __attribute__((aligned(16))) unsigned char cs_raw[];
    __shared__ uint32_t cs_cur[KMDB_SUBPOOLS];                            // (wcur: see cs_hist_kernel)
    WideRec* st_rec = (WideRec*)cs_raw;                                   // [CS_TILE]
    uint32_t* st_dst = (uint32_t*)(st_rec + CS_TILE);                     // [CS_TILE] global destination
    uint32_t* st_key = st_dst + CS_TILE;                                  // [CS_TILE]; not there for packed records: their key words (the stream only) stay behind
    uint32_t* hist = st_key + (packed ? 0u : CS_TILE);                    // [n_keys] records of the tile per bin
    uint32_t* toff = hist + n_keys;                                       // [n_keys] first staging position of the bin
    uint32_t* cursor = toff + n_keys;                                     // [n_keys] next global position of the bin for this workgroup
    uint32_t* part = cursor + n_keys;                                     // [CS_THREADS] scan scratch
    const CsJob job = cs_job(n);
    const uint32_t nb = n_keys, lo = job.lo, hi = job.hi;
    for (uint32_t k = threadIdx.x; k < nb; k += CS_THREADS) cursor[k] = O[(size_t)job.tab + (size_t)k * gridDim.x];
    constexpr uint32_t PER = CS_TILE / CS_THREADS;
    const uint32_t kper = (nb + CS_THREADS - 1u) / CS_THREADS;                              // bins per thread in the scan
    // keys and records are fetched together, and the next tile's before this one is staged (one round trip per tile, under way early)
    uint32_t nkw[PER];
    WideRec nrec[PER];
    const uint32_t wv = threadIdx.x >> 6;
    auto fetch = [&](uint32_t t0) {
        const uint32_t handed = cs_chunks_handed(cs_cur, wcur != nullptr, t0);
#pragma unroll
        for (uint32_t j = 0; j < PER; ++j) {
            const uint32_t i = t0 + j * CS_THREADS + threadIdx.x;
            nkw[j] = 0xFFFFFFFFu; nrec[j] = WideRec{0ull, 0ull};
            if (i < hi && ((handed >> (4u * j + wv)) & 1u)) { nkw[j] = wkey[i]; nrec[j] = wrec[i]; }
        }
    };
    static_assert(PER * (CS_THREADS / 64u) == 32u, "cs_chunks_handed covers the 32 chunks of a tile");
    cs_load_cursors(cs_cur, wcur);
    if (lo < hi) fetch(lo);
    for (uint32_t t0 = lo; t0 < hi; t0 += CS_TILE) {
        for (uint32_t k = threadIdx.x; k < nb; k += CS_THREADS) hist[k] = 0;
        __syncthreads();
        uint32_t key[PER], kw[PER], rank[PER];                     // bin, whole key word (stream + weight digit), rank in the tile
        WideRec rc[PER];
#pragma unroll
        for (uint32_t j = 0; j < PER; ++j) {
            kw[j] = nkw[j]; rc[j] = nrec[j];
            key[j] = cs_bin(kw[j] & kmask, n_valid);
            rank[j] = key[j] < nb ? atomicAdd(&hist[key[j]], 1u) : 0u;
        }
        if (t0 + CS_TILE < hi) fetch(t0 + CS_TILE);
        __syncthreads();
        // exclusive scan of the tile histogram: kper consecutive bins per thread, then the partial sums
        uint32_t sum = 0;
        for (uint32_t k = threadIdx.x * kper; k < nb && k < (threadIdx.x + 1u) * kper; ++k) sum += hist[k];
        // the partial sums scanned inside the waves (DPP), the four wave totals through LDS: one barrier instead of sixteen
        const uint32_t sincl = wave_incl_scan(sum, threadIdx.x & 63u);
        if ((threadIdx.x & 63u) == 63u) part[threadIdx.x >> 6] = sincl;
        __syncthreads();
        uint32_t run = sincl - sum;
        for (uint32_t k = 0; k < (threadIdx.x >> 6); ++k) run += part[k];
        const uint32_t tile_n = part[0] + part[1] + part[2] + part[3];
        for (uint32_t k = threadIdx.x * kper; k < nb && k < (threadIdx.x + 1u) * kper; ++k) { toff[k] = run; run += hist[k]; }
        __syncthreads();
        // stage: record -> its bin's run inside the tile, with its global destination
#pragma unroll
        for (uint32_t j = 0; j < PER; ++j) {
            if (key[j] < nb) {
                const uint32_t p = toff[key[j]] + rank[j];
                st_rec[p] = rc[j];
                st_dst[p] = cursor[key[j]] + rank[j];
                if (!packed) st_key[p] = kw[j];
            }
        }
        __syncthreads();
        for (uint32_t k = threadIdx.x; k < nb; k += CS_THREADS) cursor[k] += hist[k];
        for (uint32_t p = threadIdx.x; p < tile_n; p += CS_THREADS) {
            const uint32_t d = st_dst[p];
            swrec[d] = st_rec[p];
            if (!packed) swkey[d] = st_key[p];
        }
        __syncthreads();
    }
}

// ---- the chunk table grouped by key (stream chunks [0, n_states), row chunks n_states + row; n_keys = never opened) without a general
// sort: histogram, scan, scatter.  Many chunks share few keys (a thousand-sample database has twenty diagonal streams), and
// same-address device atomics run at some ten million per second: a workgroup first groups ITS chunks by key in a small LDS hash
// table (LDS atomics), then does one device atomic per distinct key.  The order of the chunks inside a key is arbitrary.
constexpr uint32_t CT_THREADS = 1024, CT_SLOTS = 2048;
// every thread's key goes into the table; returns the slot and the thread's rank among the block's chunks of that key
__device__ __forceinline__ void ct_group(uint32_t key, bool on, uint32_t* t_key, uint32_t* t_cnt, uint32_t& slot, uint32_t& rank) {
    for (uint32_t e = threadIdx.x; e < CT_SLOTS; e += CT_THREADS) { t_key[e] = 0xFFFFFFFFu; t_cnt[e] = 0u; }
    __syncthreads();
    slot = 0; rank = 0;
    if (on) {
        uint32_t h = (key * 2654435761u) >> 21;                  // 11 bits
        for (;;) {
            const uint32_t prev = atomicCAS(&t_key[h], 0xFFFFFFFFu, key);
            if (prev == 0xFFFFFFFFu || prev == key) break;
            h = (h + 1u) & (CT_SLOTS - 1u);
        }
        slot = h;
        rank = atomicAdd(&t_cnt[h], 1u);
    }
    __syncthreads();
}
__global__ __launch_bounds__(CT_THREADS) void ct_hist_kernel(const uint32_t* __restrict__ chunk_key, uint32_t n, uint32_t n_keys, uint32_t* __restrict__ hist) {
    __shared__ uint32_t t_key[CT_SLOTS], t_cnt[CT_SLOTS];
    const uint32_t i = blockIdx.x * CT_THREADS + threadIdx.x;
    const uint32_t k = i < n ? chunk_key[i] : 0xFFFFFFFFu;
    uint32_t slot, rank;
    ct_group(k, k < n_keys, t_key, t_cnt, slot, rank);
    for (uint32_t e = threadIdx.x; e < CT_SLOTS; e += CT_THREADS)
        if (t_cnt[e]) atomicAdd(&hist[t_key[e]], t_cnt[e]);
}
__global__ __launch_bounds__(CT_THREADS) void ct_scatter_kernel(const uint32_t* __restrict__ chunk_key, uint32_t n, uint32_t n_keys, uint32_t* __restrict__ cursor,
                                                               uint32_t* __restrict__ sorted_key, uint32_t* __restrict__ sorted_id) {
    __shared__ uint32_t t_key[CT_SLOTS], t_cnt[CT_SLOTS];
    const uint32_t i = blockIdx.x * CT_THREADS + threadIdx.x;
    const uint32_t k = i < n ? chunk_key[i] : 0xFFFFFFFFu;
    const bool on = k < n_keys;
    uint32_t slot, rank;
    ct_group(k, on, t_key, t_cnt, slot, rank);
    // one reservation per distinct key of the block; the base replaces the count
    for (uint32_t e = threadIdx.x; e < CT_SLOTS; e += CT_THREADS)
        if (t_cnt[e]) t_cnt[e] = atomicAdd(&cursor[t_key[e]], t_cnt[e]);
    __syncthreads();
    if (on) {
        const uint32_t o = t_cnt[slot] + rank;
        sorted_key[o] = k; sorted_id[o] = i;
    }
}
// stream chunks in use, slots of the sorted chunk table in use
__global__ void ct_count_kernel(const uint32_t* __restrict__ ct_offs, uint32_t n_states, uint32_t* __restrict__ counters) {
    counters[KCTR_CHUNKS] = ct_offs[n_states];
}

// ---- many streams: the row chunks (key n_states + row) grouped by row.  Every chunk a wave opens costs one entry here; a device
// atomic per chunk on the row's counter was measured (the narrow kernel, whose neighbouring waves open chunks of the same rows: 1.7
// -> 4.5 ms), so: counting sort without device atomics — LDS histogram per workgroup of RG_THREADS chunk ids, one scan over
// [row][workgroup], scatter with LDS cursors.  Row X's chunks: row_ids[O[X * G] .. O[(X + 1) * G]), G = workgroups (O[NB * G] = all).
constexpr uint32_t RG_THREADS = 1024;
__global__ __launch_bounds__(RG_THREADS) void rg_hist_kernel(const uint32_t* __restrict__ chunk_key, uint32_t n, uint32_t n_states, uint32_t NB, uint32_t* __restrict__ H) {
    extern __shared__ uint32_t cs_lds[];
    for (uint32_t r = threadIdx.x; r < NB; r += RG_THREADS) cs_lds[r] = 0;
    __syncthreads();
    const uint32_t i = blockIdx.x * RG_THREADS + threadIdx.x;
    const uint32_t r = (i < n ? chunk_key[i] : 0u) - n_states;
    if (i < n && r < NB) atomicAdd(&cs_lds[r], 1u);
    __syncthreads();
    for (uint32_t k = threadIdx.x; k < NB; k += RG_THREADS) H[(size_t)k * gridDim.x + blockIdx.x] = cs_lds[k];
    if (blockIdx.x == 0 && threadIdx.x == 0) H[(size_t)NB * gridDim.x] = 0;          // the scan leaves the total here
}
__global__ __launch_bounds__(RG_THREADS) void rg_scatter_kernel(const uint32_t* __restrict__ chunk_key, uint32_t n, uint32_t n_states, uint32_t NB,
                                                               const uint32_t* __restrict__ O, uint32_t* __restrict__ row_ids) {
    extern __shared__ uint32_t cs_lds[];
    for (uint32_t k = threadIdx.x; k < NB; k += RG_THREADS) cs_lds[k] = O[(size_t)k * gridDim.x + blockIdx.x];
    __syncthreads();
    const uint32_t i = blockIdx.x * RG_THREADS + threadIdx.x;
    const uint32_t r = (i < n ? chunk_key[i] : 0u) - n_states;
    if (i < n && r < NB) row_ids[atomicAdd(&cs_lds[r], 1u)] = i;
}

// ---- many streams: the sort inside the block rows.  Row X's records sit in the chunks of its part of row_ids, cut into jobs of
// RS_JOB_CHUNKS chunks, one workgroup each; bins = the row's X + 1 streams.  Counting sort as above (LDS histograms per job, one
// scan over [row][stream][job], LDS-staged scatter), reading through the chunk list, writing the dense sorted arrays
// k2_jobs_kernel walks.
constexpr uint32_t RS_JOB_CHUNKS = 64;
// (NB: the block rows the tables hold.  The whole matrix: all of them, Xlo = sbase = 0, bins = NB.  Band emit: the band's rows, row r of the tables is block row
// Xlo + r with Xlo + r + 1 streams, keyed from sbase = tri32(Xlo) on; bins = Xhi + 1, the streams of its last row)
struct RsRows { const uint32_t* O; const uint32_t* row_ids; uint32_t G, NB; const uint32_t* row_job; const uint32_t* row_tab; uint32_t Xlo, sbase, bins; };
// (the kernel's body: BAND = false is rs_rows_kernel as it always was, Xlo folded to 0)
template <bool BAND>
__device__ __forceinline__ void rs_rows_body(const uint32_t* __restrict__ O, uint32_t G, uint32_t NB, uint32_t* __restrict__ row_job, uint32_t* __restrict__ row_tab,
                                             uint32_t* __restrict__ counters, uint32_t Xlo_arg) {
    const uint32_t Xlo = BAND ? Xlo_arg : 0u;
    __shared__ uint32_t s_job[1024], s_tab[1024];
    // jobs and table entries of every row, then block-wide exclusive scans (NB may be a few thousand)
    uint32_t cj = 0, ct = 0;
    for (uint32_t base = 0; base < NB; base += 1024) {
        const uint32_t X = base + threadIdx.x;
        uint32_t nj = 0;
        if (X < NB) nj = (O[(size_t)(X + 1u) * G] - O[(size_t)X * G] + RS_JOB_CHUNKS - 1u) / RS_JOB_CHUNKS;
        s_job[threadIdx.x] = nj; s_tab[threadIdx.x] = X < NB ? nj * (X + Xlo + 1u) : 0u;
        __syncthreads();
        for (uint32_t d = 1; d < 1024; d <<= 1) {
            const uint32_t a = threadIdx.x >= d ? s_job[threadIdx.x - d] : 0u, b = threadIdx.x >= d ? s_tab[threadIdx.x - d] : 0u;
            __syncthreads();
            s_job[threadIdx.x] += a; s_tab[threadIdx.x] += b;
            __syncthreads();
        }
        if (X < NB) { row_job[X] = cj + s_job[threadIdx.x] - nj; row_tab[X] = ct + s_tab[threadIdx.x] - nj * (X + Xlo + 1u); }
        cj += s_job[1023]; ct += s_tab[1023];
        __syncthreads();
    }
    if (threadIdx.x == 0) { row_job[NB] = cj; row_tab[NB] = ct; counters[KCTR_ROWJOBS] = cj; counters[KCTR_RAW] = O[(size_t)NB * G]; }
}
__global__ void rs_rows_kernel(const uint32_t* __restrict__ O, uint32_t G, uint32_t NB, uint32_t* __restrict__ row_job, uint32_t* __restrict__ row_tab,
                               uint32_t* __restrict__ counters) { rs_rows_body<false>(O, G, NB, row_job, row_tab, counters, 0u); }
__global__ void rs_rows_band_kernel(const uint32_t* __restrict__ O, uint32_t G, uint32_t NB, uint32_t* __restrict__ row_job, uint32_t* __restrict__ row_tab,
                                    uint32_t* __restrict__ counters, uint32_t Xlo) { rs_rows_body<true>(O, G, NB, row_job, row_tab, counters, Xlo); }
struct RsJob { uint32_t X, nj, cb, ce, tab; const uint32_t* ids; };

__device__ __forceinline__ bool rs_job(const RsRows& R, uint32_t job, uint32_t job_end, RsJob& j) {
    const uint32_t NB = R.NB;
    if (job >= job_end || job >= R.row_job[NB]) return false;
    uint32_t a = 0, b = NB;                                  // last row whose first job is <= this one (rows without jobs share their successor's first job)
    while (b - a > 1u) { const uint32_t mid = (a + b) >> 1; if (R.row_job[mid] <= job) a = mid; else b = mid; }
    const uint32_t c = job - R.row_job[a];
    j.X = a; j.nj = R.row_job[a + 1] - R.row_job[a];
    j.cb = R.O[(size_t)a * R.G] + c * RS_JOB_CHUNKS;
    const uint32_t re = R.O[(size_t)(a + 1u) * R.G];
    j.ce = re - j.cb > RS_JOB_CHUNKS ? j.cb + RS_JOB_CHUNKS : re;
    j.tab = R.row_tab[a] + c;
    j.ids = R.row_ids;
    return true;
}
template <uint32_t U>                                        // chunks whose key words a thread requests together (one round trip per U chunks)
__global__ __launch_bounds__(256) void rs_hist_kernel(const RsRows R, const uint32_t* __restrict__ chunk_fill, const uint32_t* __restrict__ recw, uint32_t kmask,
                                                     uint32_t* __restrict__ H) {
    extern __shared__ uint32_t cs_lds[];
    __shared__ uint32_t s_id[RS_JOB_CHUNKS], s_fill[RS_JOB_CHUNKS];
    RsJob j;
    if (!rs_job(R, blockIdx.x, 0xFFFFFFFFu, j)) return;
    const uint32_t nb = j.X + R.Xlo + 1u, sub = tri32(j.X + R.Xlo) - R.sbase, nch = j.ce - j.cb;
    for (uint32_t k = threadIdx.x; k < nb; k += blockDim.x) cs_lds[k] = 0;
    // the job's chunk ids and fills first (one round trip), then the key words of four chunks at a time
    if (threadIdx.x < nch) { const uint32_t id = j.ids[j.cb + threadIdx.x]; s_id[threadIdx.x] = id; s_fill[threadIdx.x] = chunk_fill[id]; }
    __syncthreads();
    for (uint32_t c0 = 0; c0 < nch; c0 += U) {
        uint32_t kw[U];
#pragma unroll
        for (uint32_t jj = 0; jj < U; ++jj) {
            kw[jj] = 0xFFFFFFFFu;
            if (c0 + jj < nch && threadIdx.x < s_fill[c0 + jj]) kw[jj] = recw[((size_t)s_id[c0 + jj] << CH_SHIFT) + threadIdx.x];
        }
#pragma unroll
        for (uint32_t jj = 0; jj < U; ++jj) {
            const uint32_t bin = (kw[jj] & kmask) - sub;
            if (kw[jj] != 0xFFFFFFFFu && bin < nb) atomicAdd(&cs_lds[bin], 1u);
        }
    }
    __syncthreads();
    for (uint32_t k = threadIdx.x; k < nb; k += blockDim.x) H[(size_t)j.tab + (size_t)k * j.nj] = cs_lds[k];
}
// Per tile of CS_TILE records (four chunks): keys and records are fetched TOGETHER (the records wait in registers) and the next
// tile's are requested before this one is staged — the kernel used to pay four dependent round trips per tile (chunk id, fill, key,
// record), one workgroup-wide phase after the other.
__global__ __launch_bounds__(CS_THREADS) void rs_scatter_kernel(const RsRows R, const uint32_t* __restrict__ chunk_fill,
                                                         const uint32_t* __restrict__ recw, const WideRec* __restrict__ rec, uint32_t kmask,
                                                         const uint32_t* __restrict__ O, uint32_t cap, uint32_t* __restrict__ swkey, WideRec* __restrict__ swrec,
                                                         uint32_t* __restrict__ counters, uint32_t packed) {
    extern __shared__ __attribute__((aligned(16))) unsigned char cs_raw[];
    __shared__ uint32_t s_id[RS_JOB_CHUNKS], s_fill[RS_JOB_CHUNKS];
    RsJob job;
    // consecutive jobs write neighbouring stretches of every stream of their row (the lines at the seams are shared): workgroups are dealt
    // to the eight XCDs round-robin, so job = f(blockIdx) keeps every XCD on ONE contiguous range of jobs and the seams in one L2
    if (!rs_job(R, xcd_contiguous(blockIdx.x, gridDim.x), 0xFFFFFFFFu, job)) return;
    const uint32_t NB = R.bins;
    const uint32_t nb = job.X + R.Xlo + 1u, sub = tri32(job.X + R.Xlo) - R.sbase, nch = job.ce - job.cb;
    WideRec* st_rec = (WideRec*)cs_raw;                                   // [CS_TILE]
    uint32_t* st_dst = (uint32_t*)(st_rec + CS_TILE);                     // [CS_TILE] global destination
    uint32_t* st_key = st_dst + CS_TILE;                                  // [CS_TILE]; not there for packed records (their key words stay behind: 8 KB
    uint32_t* hist = st_key + (packed ? 0u : CS_TILE);                    //   less LDS per workgroup, one more workgroup per CU)  [nb] records of the tile per bin
    uint32_t* toff = hist + NB;                                           // [nb] first staging position of the bin
    uint32_t* cursor = toff + NB;                                         // [nb] next global position of the bin for this workgroup
    uint32_t* part = cursor + NB;                                         // [CS_THREADS] scan scratch
    for (uint32_t k = threadIdx.x; k < nb; k += CS_THREADS) cursor[k] = O[(size_t)job.tab + (size_t)k * job.nj];
    if (threadIdx.x < nch) { const uint32_t id = job.ids[job.cb + threadIdx.x]; s_id[threadIdx.x] = id; s_fill[threadIdx.x] = chunk_fill[id]; }
    __syncthreads();
    constexpr uint32_t PER = CS_TILE / CH_REC;                            // chunks per tile: thread t takes slot t of each
    static_assert(CH_REC == CS_THREADS, "a chunk per pass of the workgroup");
    const uint32_t kper = (nb + CS_THREADS - 1u) / CS_THREADS;
    uint32_t nkw[PER];
    WideRec nrec[PER];
    auto fetch = [&](uint32_t c0) {
#pragma unroll
        for (uint32_t jj = 0; jj < PER; ++jj) {
            nkw[jj] = 0xFFFFFFFFu; nrec[jj] = WideRec{0ull, 0ull};
            if (c0 + jj < nch && threadIdx.x < s_fill[c0 + jj]) {
                const size_t slot = ((size_t)s_id[c0 + jj] << CH_SHIFT) + threadIdx.x;
                nkw[jj] = recw[slot]; nrec[jj] = rec[slot];
            }
        }
    };
    fetch(0);
    for (uint32_t c0 = 0; c0 < nch; c0 += PER) {
        for (uint32_t k = threadIdx.x; k < nb; k += CS_THREADS) hist[k] = 0;
        __syncthreads();
        uint32_t key[PER], kw[PER], rank[PER];
        WideRec rc[PER];
#pragma unroll
        for (uint32_t jj = 0; jj < PER; ++jj) {
            kw[jj] = nkw[jj]; rc[jj] = nrec[jj];
            key[jj] = kw[jj] != 0xFFFFFFFFu ? (kw[jj] & kmask) - sub : 0xFFFFFFFFu;
            rank[jj] = key[jj] < nb ? atomicAdd(&hist[key[jj]], 1u) : 0u;
        }
        if (c0 + PER < nch) fetch(c0 + PER);                     // the next tile's keys and records are under way while this one is staged
        __syncthreads();
        uint32_t sum = 0;
        for (uint32_t k = threadIdx.x * kper; k < nb && k < (threadIdx.x + 1u) * kper; ++k) sum += hist[k];
        // the partial sums scanned inside the waves (DPP), the four wave totals through LDS: one barrier instead of sixteen
        const uint32_t sincl = wave_incl_scan(sum, threadIdx.x & 63u);
        if ((threadIdx.x & 63u) == 63u) part[threadIdx.x >> 6] = sincl;
        __syncthreads();
        uint32_t run = sincl - sum;
        for (uint32_t k = 0; k < (threadIdx.x >> 6); ++k) run += part[k];
        const uint32_t tile_n = part[0] + part[1] + part[2] + part[3];
        for (uint32_t k = threadIdx.x * kper; k < nb && k < (threadIdx.x + 1u) * kper; ++k) { toff[k] = run; run += hist[k]; }
        __syncthreads();
#pragma unroll
        for (uint32_t jj = 0; jj < PER; ++jj) {
            if (key[jj] < nb) {
                const uint32_t pp = toff[key[jj]] + rank[jj];
                st_rec[pp] = rc[jj];
                st_dst[pp] = cursor[key[jj]] + rank[jj];
                if (!packed) st_key[pp] = kw[jj];
            }
        }
        __syncthreads();
        for (uint32_t k = threadIdx.x; k < nb; k += CS_THREADS) cursor[k] += hist[k];
        for (uint32_t pp = threadIdx.x; pp < tile_n; pp += CS_THREADS) {
            const uint32_t d = st_dst[pp];
            if (d < cap) { swrec[d] = st_rec[pp]; if (!packed) swkey[d] = st_key[pp]; }      // (packed records carry their weight themselves)
            else atomicOr(&counters[KCTR_WIDE_OVERFLOW], 1u);            // the sorted arrays are too small: the call is repeated with larger ones
        }
        __syncthreads();
    }
}
__host__ __device__ inline size_t rs_scatter_lds(uint32_t NB, bool packed) { return (size_t)CS_TILE * (sizeof(WideRec) + (packed ? 4 : 8)) + (size_t)NB * 12 + CS_THREADS * 4 + 64; }

// K2 over db2db's records sorted by stream (kmdb_rect_sort_apply; stream = row block x rect_nbc + column block): a window of K2S_WIN sorted
// positions, run boundaries searched in the key words, one 64 x 64 tile per run of equal streams
constexpr uint32_t K2S_WIN = 4096;
constexpr int K2S_MIN_WAVES = 3;           // waves per SIMD the compiler must leave room for (4: 128 VGPRs and 104 B of scratch per lane; 3: no scratch)
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(K2S_MIN_WAVES, 8))) void k2_sorted_kernel(const uint32_t* __restrict__ swkey, const WideRec* __restrict__ swrec,
                                                        uint32_t limit, const uint32_t* __restrict__ total_ptr,
                                                        uint32_t n_states, uint32_t kbits, uint32_t dbits, uint32_t* __restrict__ M, uint32_t N,
                                                        uint32_t bwidth, uint32_t rect_nbc, uint32_t rect_cols) {
    __shared__ uint32_t acc[64 * 64];
    __shared__ __attribute__((aligned(16))) unsigned char wbuf[4][64];
    __shared__ unsigned long long lut_ff[256], lut_01[256];
    __shared__ uint16_t bnd[K2S_WIN + 2];          // run starts inside the window, then the end
    __shared__ uint32_t wor_sh;
    __shared__ uint32_t tcount[256];
    const uint32_t total = total_ptr ? (*total_ptr < limit ? *total_ptr : limit) : limit;      // counting sort: the valid records; radix sort: all slots
    const uint32_t p0 = blockIdx.x * K2S_WIN;
    const uint32_t kmask = (1u << kbits) - 1u;
    if (p0 >= total || (swkey[p0] & kmask) >= n_states) return;
    const uint32_t wend = total - p0 < K2S_WIN ? total - p0 : K2S_WIN;
    {
        unsigned long long v = 0;
#pragma unroll
        for (int i = 0; i < 8; ++i) v |= ((threadIdx.x >> i) & 1u) ? 0xFFull << (8 * i) : 0ull;
        lut_ff[threadIdx.x] = v;
        lut_01[threadIdx.x] = v & 0x0101010101010101ull;
    }
    // run starts: every thread scans 32 consecutive positions; a block scan puts them in order
    constexpr uint32_t PER = K2S_WIN / 256;
    const uint32_t t0 = threadIdx.x * PER;
    uint32_t prev = (t0 == 0 || t0 >= wend) ? 0xFFFFFFFFu : (swkey[p0 + t0 - 1] & kmask);
    uint32_t mine = 0, flags = 0;
    uint32_t kk[PER];                                              // the thread's 32 keys: 8 loads of 16 bytes in flight together
    if (t0 + PER <= wend && (p0 & 3u) == 0u) {
#pragma unroll
        for (uint32_t v = 0; v < PER / 4; ++v) {
            const uint4 q4 = ((const uint4*)(swkey + p0 + t0))[v];
            kk[4 * v] = q4.x & kmask; kk[4 * v + 1] = q4.y & kmask; kk[4 * v + 2] = q4.z & kmask; kk[4 * v + 3] = q4.w & kmask;
        }
    } else {
#pragma unroll
        for (uint32_t i = 0; i < PER; ++i) kk[i] = t0 + i < wend ? (swkey[p0 + t0 + i] & kmask) : 0xFFFFFFFFu;
    }
#pragma unroll
    for (uint32_t i = 0; i < PER; ++i) {
        if (t0 + i < wend && kk[i] != prev) { flags |= 1u << i; ++mine; }      // the first never-written slot starts a last "run" that ends the loop below
        prev = kk[i];
    }
    const uint32_t mincl = wave_incl_scan(mine, threadIdx.x & 63u);
    if ((threadIdx.x & 63u) == 63u) tcount[threadIdx.x >> 6] = mincl;
    __syncthreads();
    {
        uint32_t o = mincl - mine;
        for (uint32_t k = 0; k < (threadIdx.x >> 6); ++k) o += tcount[k];
        for (uint32_t i = 0; i < PER; ++i) if ((flags >> i) & 1u) bnd[o++] = (uint16_t)(t0 + i);
    }
    const uint32_t nb = tcount[0] + tcount[1] + tcount[2] + tcount[3];
    if (threadIdx.x == 0) bnd[nb] = (uint16_t)wend;
    __syncthreads();
    for (uint32_t r = 0; r < nb; ++r) {
        const uint32_t a = bnd[r], b = bnd[r + 1];
        const uint32_t key = swkey[p0 + a] & kmask;
        if (key >= n_states) break;
        K2Item it;
        {
            const uint32_t bucket = key;
            it.X = bucket / rect_nbc; it.Y = bucket - it.X * rect_nbc;
            it.rect_cols = rect_cols; it.pshift = 0;
            it.n_rec = b - a; it.count = (it.n_rec + 63u) / 64u; it.ids = nullptr; it.fills = nullptr; it.srec = swrec + p0 + a; it.skey = swkey + p0 + a; it.kbits = kbits; it.dbits = dbits; it.rec = nullptr; it.recw = nullptr;
        }
        k2_run<true>(it, acc, &wor_sh, wbuf, lut_ff, lut_01, M, N, bwidth, nullptr);      // (a rectangle: no tile flags)
    }
}

// Many streams (row mode): the apply step over the sorted records takes a stream — or a part of K2J_REC records of a long one — per
// workgroup instead of a window of sorted positions: a tile is written back ONCE per K2J_REC records of its stream (north_star: "a single
// HBM write-back per tile"), where the windows of 4096 positions wrote every tile they met — 1.49 GB of atomics for the 0.2 GB matrix of
// 10 000 samples.  Where a stream starts is known from the counting sort's offsets: no run boundaries are searched.
constexpr uint32_t K2J_REC = 16384;
// (O = the sort's offsets [row][stream of the row][job of the row], exclusive sums: entry (X, Y, job 0) is where stream (X, Y) starts)
// (BAND = false is k2j_starts_kernel as it always was; BAND: stream s of the band is stream s + sbase of the matrix, its block row counted from Xlo)
template <bool BAND>
__device__ __forceinline__ void k2j_starts_body(const RsRows& R, const uint32_t* __restrict__ O, uint32_t n_states, uint32_t* __restrict__ start) {
    const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s > n_states) return;
    if (s == n_states) { start[s] = O[R.row_tab[R.NB]]; return; }                         // all sorted records
    const uint32_t sa = BAND ? s + R.sbase : s;
    const uint32_t Xa = stream_row(sa), Y = sa - tri32(Xa), X = BAND ? Xa - R.Xlo : Xa;
    const uint32_t nj = R.row_job[X + 1] - R.row_job[X];                                   // a row without records has no jobs: its streams start where the next row does
    start[s] = O[(size_t)R.row_tab[X] + (size_t)Y * nj];
}
__global__ void k2j_starts_kernel(const RsRows R, const uint32_t* __restrict__ O, uint32_t n_states, uint32_t* __restrict__ start) { k2j_starts_body<false>(R, O, n_states, start); }
__global__ void k2j_starts_band_kernel(const RsRows R, const uint32_t* __restrict__ O, uint32_t n_states, uint32_t* __restrict__ start) { k2j_starts_body<true>(R, O, n_states, start); }
// few streams: O = the one-pass sort's offsets [stream][workgroup share] (+ the total): share 0 of a stream is where the stream starts
__global__ void k2j_starts_flat_kernel(const uint32_t* __restrict__ O, uint32_t n_states, uint32_t shares, uint32_t* __restrict__ start) {
    const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s <= n_states) start[s] = O[(size_t)s * shares];
}
// the jobs in any order: one reservation per workgroup of streams
__global__ __launch_bounds__(1024) void k2j_build_kernel(const uint32_t* __restrict__ start, uint32_t n_states, uint2* __restrict__ jobs, uint32_t cap,
                                                         uint32_t* __restrict__ counters) {
    __shared__ uint32_t wsum[16], base_sh;
    const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x, lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t len = s < n_states ? start[s + 1] - start[s] : 0u;
    const uint32_t nj = (len + K2J_REC - 1u) / K2J_REC;
    const uint32_t incl = wave_incl_scan(nj, lane);
    if (lane == 63u) wsum[wave] = incl;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t run = 0;
        for (uint32_t k = 0; k < 16; ++k) { const uint32_t v = wsum[k]; wsum[k] = run; run += v; }
        base_sh = run ? atomicAdd(&counters[KCTR_K2JOBS], run) : 0u;
    }
    __syncthreads();
    uint32_t o = base_sh + wsum[wave] + incl - nj;
    for (uint32_t part = 0; part < nj; ++part, ++o) if (o < cap) jobs[o] = make_uint2(s, part);
}
// (BAND, BandWin: a job whose stream lies in a block row outside the band leaves with its job word read and nothing else)
template <bool BAND>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(K2S_MIN_WAVES, 8))) void k2_jobs_kernel(const uint32_t* __restrict__ swkey, const WideRec* __restrict__ swrec,
                                                        const uint32_t* __restrict__ start, const uint2* __restrict__ jobs, const uint32_t* __restrict__ n_jobs, uint32_t cap,
                                                        uint32_t limit, uint32_t pshift, uint32_t kbits, uint32_t dbits, uint32_t* __restrict__ M, uint32_t N, uint32_t bwidth, unsigned char* __restrict__ touched,
                                                        const BandArg<BAND> band) {
    __shared__ uint32_t acc[64 * 64];
    __shared__ __attribute__((aligned(16))) unsigned char wbuf[4][64];
    __shared__ unsigned long long lut_ff[256], lut_01[256];
    __shared__ uint32_t wor_sh;
    const uint32_t nj = *n_jobs < cap ? *n_jobs : cap;
    if (blockIdx.x >= nj) return;
    const uint2 job = jobs[blockIdx.x];
    if constexpr (BAND) {
        const bool culled = band_culls(band.w, stream_row(band_stream(band, job.x)));
        if (threadIdx.x == 0) band_unit(band.w, blockIdx.x, BU_JOBS, !culled);
        if (culled) return;
    }
    {
        unsigned long long v = 0;
#pragma unroll
        for (int i = 0; i < 8; ++i) v |= ((threadIdx.x >> i) & 1u) ? 0xFFull << (8 * i) : 0ull;
        lut_ff[threadIdx.x] = v;
        lut_01[threadIdx.x] = v & 0x0101010101010101ull;
    }
    // (limit = slots of the sorted arrays: a call whose pools were too small sorted only what fitted — it is repeated with larger pools, and
    // until then nothing beyond the arrays may be read)
    const uint32_t e = start[job.x + 1] < limit ? start[job.x + 1] : limit;
    uint32_t a = start[job.x] + job.y * K2J_REC;
    a = a < e ? a : e;
    const uint32_t b = e - a > K2J_REC ? a + K2J_REC : e;
    if (a == b) return;
    K2Item it;
    const uint32_t stream = band_stream(band, job.x);
    it.X = stream_row(stream); it.Y = stream - tri32(it.X); it.rect_cols = 0; it.pshift = pshift;
    it.n_rec = b - a; it.count = (it.n_rec + 63u) / 64u; it.ids = nullptr; it.fills = nullptr; it.srec = swrec + a; it.skey = swkey + a; it.kbits = kbits; it.dbits = dbits;
    it.rec = nullptr; it.recw = nullptr;
    k2_run<true, BAND>(it, acc, &wor_sh, wbuf, lut_ff, lut_01, M, N, bwidth, touched, band);
}

// ------------------------------------------------------------------------------------------
// upload-time: sampled estimate of the number of block records per candidate width
// ------------------------------------------------------------------------------------------
constexpr int EST_NW = 10;
struct EstParams {
    const uint2* k0in;
    const uint32_t* bitrel;
    const uint64_t* blkbase;
    const uint64_t* bits;
    const int32_t* parent;
    const uint32_t* nl;
    const uint32_t* w;
    uint32_t P, stride;
    uint32_t widths[EST_NW];
    uint32_t magics[EST_NW];
    unsigned long long* out;       // [EST_NW] records of the sampled nodes with <= 2 blocks, [EST_NW] of the others, [1] nodes sampled,
                                   // [EST_NW] the part of the others that comes from nodes with l2_min blocks or more (the second level writes no records for them)
    uint32_t l2_min;
};
// One thread per sampled node: climbs the root path, decodes every node's local ids (the only decoder run outside the
// call: it looks at one node in `stride`) and counts the blocks of the full list for every candidate width.
__global__ void width_estimate_kernel(const EstParams q) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t i0 = (uint64_t)t * q.stride + (t * 2654435761u) % q.stride;
    const uint32_t node = (uint32_t)i0;
    const bool on = i0 < q.P && q.w[node] != 0 && q.nl[node] >= 2u;
    uint32_t nblk[EST_NW], lower_first[EST_NW];
#pragma unroll
    for (int c = 0; c < EST_NW; ++c) { nblk[c] = 0; lower_first[c] = 0xFFFFFFFFu; }
    int32_t y = on ? (int32_t)node : -1;
    while (y >= 0) {
        const uint2 km = q.k0in[y];
        const uint32_t l = kmdb_k0_l(km), last = kmdb_k0_last(km);
        if (l) {
            const uint64_t pos = q.blkbase[(uint32_t)y >> 8] + q.bitrel[y];
            uint32_t sum = 0;                                   // (gamma_first_id, written out here and in pair_estimate_kernel: see profiles/gamma_reader_codeobject.md)
            if (l > 1) { GammaCursor<2> c(q.bits, pos); for (uint32_t k = 0; k + 1 < l; ++k) sum += c.next(); }
            uint32_t id = last - sum;
            uint32_t fb[EST_NW], cb[EST_NW];
#pragma unroll
            for (int c = 0; c < EST_NW; ++c) { fb[c] = __umulhi(id, q.magics[c]); cb[c] = fb[c]; nblk[c] += 1; }
            if (l > 1) {
                GammaCursor<2> c2(q.bits, pos);
                for (uint32_t k = 0; k + 1 < l; ++k) {
                    id += c2.next();
#pragma unroll
                    for (int c = 0; c < EST_NW; ++c) { const uint32_t b = __umulhi(id, q.magics[c]); nblk[c] += b != cb[c]; cb[c] = b; }
                }
            }
#pragma unroll
            for (int c = 0; c < EST_NW; ++c) { nblk[c] -= cb[c] == lower_first[c]; lower_first[c] = fb[c]; }
        }
        y = q.parent[y];
    }
    // one atomic per wave and counter
    const uint32_t lane = threadIdx.x & 63u;
#pragma unroll
    for (int c = 0; c < EST_NW; ++c) {
        // a node with at most two blocks sends one record to its first block's stream chunk; all other records take the wide pool
        const unsigned long long recs = (unsigned long long)nblk[c] * (nblk[c] + 1u) / 2u;
        unsigned long long rn = on && nblk[c] >= 1u && nblk[c] <= 2u ? 1ull : 0ull;
        unsigned long long rg = on ? recs - rn : 0ull;
        unsigned long long r2 = on && nblk[c] >= q.l2_min ? recs : 0ull;
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) { rn += shfl64(rn, (int)(lane ^ (uint32_t)d)); rg += shfl64(rg, (int)(lane ^ (uint32_t)d)); r2 += shfl64(r2, (int)(lane ^ (uint32_t)d)); }
        if (lane == 0) { if (rn) atomicAdd(&q.out[c], rn); if (rg) atomicAdd(&q.out[EST_NW + c], rg); if (r2) atomicAdd(&q.out[2 * EST_NW + 1 + c], r2); }
    }
    const unsigned long long nb = __ballot(on);
    if (lane == 0 && nb) atomicAdd(&q.out[2 * EST_NW], (unsigned long long)__popcll(nb));
}

// upload-time: sampled estimate of the extra (block, mask) pairs K0 reserves (one node in `stride`, its own list only)
__global__ void pair_estimate_kernel(const uint2* __restrict__ k0in, const uint32_t* __restrict__ bitrel, const uint64_t* __restrict__ blkbase,
                                     const uint64_t* __restrict__ bits, uint32_t P, uint32_t stride, BlockMap bm, unsigned long long* __restrict__ out) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t i0 = (uint64_t)t * stride + (t * 2654435761u) % stride;
    unsigned long long need = 0;
    if (i0 < P) {
        const uint2 km = k0in[i0];
        const uint32_t l = kmdb_k0_l(km), last = kmdb_k0_last(km);
        if (l > 1) {
            GammaCursor<2> c(bits, blkbase[(uint32_t)i0 >> 8] + bitrel[i0]);
            uint32_t span = 0;
            for (uint32_t k = 0; k + 1 < l; ++k) span += c.next();
            const uint32_t nb = bm.blk(last) - bm.blk(last - span);
            need = nb < l - 1u ? nb : l - 1u;
        }
    }
    const uint32_t lane = threadIdx.x & 63u;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) need += shfl64(need, (int)(lane ^ (uint32_t)d));
    if (lane == 0 && need) atomicAdd(out, need);
}

// weight digit bits of the wide pool's key word: what the stream bits and the two digit-index bits leave (four digits cover 32 bits)
inline uint32_t wide_digit_bits(int key_bits) { return (uint32_t)(32 - key_bits - 2); }

// ------------------------------------------------------------------------------------------
// The pipeline's switches (README.md, the table of environment switches): environment variables read ONCE per handle, when its pipeline state is made
// (blocks_read_knobs at the top of blocks_prepare_impl).  An empty value counts as unset.
// ------------------------------------------------------------------------------------------
constexpr uint32_t K1W_RUN_NODES = 256;     // wide nodes per run of a wave (round-robin: heavy nodes sit together in the DFS order)
struct BlocksKnobs {
    uint32_t block_width = 0;               // KMDB_BLOCK_WIDTH: 32…64 (anything else is ignored); 0: from the sampled estimate
    bool dense_narrow = false;              // KMDB_DENSE >= 2
    int k1n_mode = 2;                       // KMDB_K1N_MODE, clamped to 0…2 (BlocksState::k1n_mode)
    int k1n_minw = 3;                       // KMDB_K1N_MINW: mode 1 at four waves per SIMD when >= 4
    int row_mode = -1;                      // KMDB_ROW_MODE: 0 / 1; -1: by the number of streams
    bool rec_packed = true;                 // KMDB_REC_PACKED=0 clears it
    bool l2 = true;                         // KMDB_L2=0 clears it
    uint32_t l2_min = L2_MIN_BLOCKS;        // KMDB_L2_MIN, at least K1W_HEAVY
    uint64_t slices = 0;                    // KMDB_SLICES, at least 1; 0: from the record estimate
    uint64_t pool_percent = 0;              // KMDB_POOL_PERCENT, at least 1; 0: unset
    uint32_t k2d_slices = K2D_SLICES;       // KMDB_K2D_SLICES, at least 1
    bool k2d_early = true;                  // KMDB_K2D_EARLY=0 clears it
    uint32_t k1w_run = K1W_RUN_NODES;       // KMDB_K1W_RUN: a multiple of 64, at least 64
    uint32_t k1w_waves = 0;                 // KMDB_K1W_WAVES, at least 1; 0: as many as the chip holds
};
BlocksKnobs blocks_read_knobs() {
    BlocksKnobs k;
    auto env = [](const char* name) -> const char* { const char* e = getenv(name); return e && *e ? e : nullptr; };
    if (const char* e = env("KMDB_BLOCK_WIDTH")) { const uint32_t w = (uint32_t)strtoul(e, nullptr, 10); if (w >= 32 && w <= 64) k.block_width = w; }
    if (const char* e = env("KMDB_DENSE")) k.dense_narrow = atoi(e) >= 2;
    if (const char* e = env("KMDB_K1N_MODE")) k.k1n_mode = std::max(0, std::min(2, atoi(e)));
    if (const char* e = env("KMDB_K1N_MINW")) k.k1n_minw = atoi(e);
    if (const char* e = env("KMDB_ROW_MODE")) k.row_mode = atoi(e) != 0;          // (tests: small databases through the many-streams path)
    if (const char* e = env("KMDB_REC_PACKED")) k.rec_packed = e[0] != '0';
    if (const char* e = env("KMDB_L2")) k.l2 = e[0] != '0';
    if (const char* e = env("KMDB_L2_MIN")) k.l2_min = std::max<uint32_t>(K1W_HEAVY, (uint32_t)atoi(e));
    if (const char* e = env("KMDB_SLICES")) k.slices = std::max<uint64_t>(1, strtoull(e, nullptr, 10));
    if (const char* e = env("KMDB_POOL_PERCENT")) k.pool_percent = std::max<uint64_t>(1, strtoull(e, nullptr, 10));
    if (const char* e = env("KMDB_K2D_SLICES")) k.k2d_slices = (uint32_t)std::max(1, atoi(e));
    if (const char* e = env("KMDB_K2D_EARLY")) k.k2d_early = e[0] != '0';
    if (const char* e = env("KMDB_K1W_RUN")) k.k1w_run = std::max<uint32_t>(64u, (uint32_t)atoi(e) / 64u * 64u);
    if (const char* e = env("KMDB_K1W_WAVES")) k.k1w_waves = std::max<uint32_t>(1u, (uint32_t)atoi(e));
    return k;
}
// the two diagnostics are read where they are used: they may be set and unset between the calls of a process
bool kmdb_verbose() { return getenv("KMDB_VERBOSE") != nullptr; }
bool kmdb_sync_debug() { return getenv("KMDB_SYNC_DEBUG") != nullptr; }      // wait after every stage and name the one that failed (no effect on results)
}  // namespace

// ------------------------------------------------------------------------------------------
// The pipeline's state: the working set of a handle (contents rebuilt by every call) and what a call remembers for the next.  The handle
// (kmdb_db.blocks) owns it; every device array is a DevBuf, so that destroying the state is all there is to releasing it.
// ------------------------------------------------------------------------------------------
struct BlocksState {
    BlocksKnobs knobs;              // the switches as they stood when the state was made
    uint32_t NB = 0, n_states = 0;  // blocks, (bucket, weight class) streams
    DevBuf<unsigned long long> p0_mask;      // [P] first (block, mask) pair of every node's local list
    DevBuf<uint32_t> p0_info;       // [P] block | npairs << 16
    DevBuf<uint32_t> pair_ofs;      // [P] first extra pair (valid when npairs > 1)
    DevBuf<uint16_t> pair_blk;      // extra pairs, KMDB_PAIR_REGIONS sub-pools
    DevBuf<unsigned long long> pair_mask;
    uint64_t pair_cap = 0;          // entries in total
    uint32_t* pair_cursor = nullptr;        // [(KMDB_PAIR_REGIONS + 1) * 16] one cursor per region, a cache line apart (in call_state)
    DevBuf<ulonglong2> fn_mask;     // [P] for a node with more than two blocks whose parent has at most two: the parent's (F0, F1)
    DevBuf<uint32_t> fn_blk;        // [P] and its blocks: first | second << 16 (0xFFFF: none)
    DevBuf<unsigned long long> widebits;     // [ceil(P / 64)] nodes with more than two blocks
    DevBuf<uint32_t> wide_base;     // [words + 1] wide nodes before every word: the narrow kernel writes them per slice, wide_expand_kernel makes them absolute
    DevBuf<uint32_t> wide_slice_cnt, wide_slice_base;   // [n_nsegs] wide nodes of every slice of the narrow kernel, [n_nsegs + 1] their exclusive scan
    DevBuf<uint32_t> widx;          // [wide_cap] the wide nodes, DFS order
    DevBuf<uint32_t> wrun_anc;      // [runs][chain_cap] root path of the first node of every run of the wide-node kernel (built by every call)
    DevBuf<uint32_t> wrun_anc_n;
    uint64_t wide_cap = 0;
    DevBuf<uint32_t> chunk_key;     // [pool_cap] stream of every chunk (n_states: never opened)
    DevBuf<uint32_t> chunk_fill;    // [pool_cap] records in the chunk
    DevBuf<uint32_t> sorted_key;    // the chunk table sorted by stream
    DevBuf<uint32_t> sorted_id;
    DevBuf<void> sort_tmp;
    size_t sort_tmp_bytes = 0;
    int key_bits = 1;
    DevBuf<unsigned char> rec;      // [pool_cap * 64] 16-byte record slots ({rows, cols}; diagonal streams pack 8-byte rows)
    DevBuf<uint32_t> recw;          // [pool_cap * 64] weights of the classes with w > 1
    uint64_t pool_cap = 0;          // chunks of 64 records, KMDB_SUBPOOLS interleaved sub-pools
    uint32_t* sub_cursor = nullptr; // [KMDB_SUBPOOLS * 16] (in call_state)
    // wide pool: records in arrival order + a device-wide sort by stream (the wide kernel always; the narrow kernel if its
    // per-stream chunks do not work out)
    bool dense_narrow = false;
    // the narrow kernel's first-block records (X, X): 0 stream chunks + k2_apply_kernel (round 5), 1 applied inside the narrow kernel (tile in its
    // registers, nothing written), 2 compacted per slice in DFS order + k2d_kernel on the side stream (default).  1 and 2: what they cannot take
    // (weights of 128 and more) goes the dense_narrow way, nothing uses stream chunks
    int k1n_mode = 2;
    DevBuf<unsigned long long> dmask;       // mode 2: [n_nsegs * nseg_nodes] F0 of the slice's records
    DevBuf<uint32_t> dwx;                   //         w | X << 8
    DevBuf<uint32_t> slice_cnt;             //         [n_nsegs] records of every slice
    uint32_t* direct_ctr = nullptr; // [KMDB_SUBPOOLS * 16] records applied directly, counted per wave on spread addresses (in call_state)
    uint64_t last_n_direct = 0;
    DevBuf<uint32_t> wkey, swkey;     // wide pool: stream of every record slot (0xFFFFFFFF = never written), and sorted
    DevBuf<WideRec> wrec, swrec;       // wide pool: 16-byte records {rows, cols} (weight digit in the key word), and sorted by stream
    uint64_t wide_pool_cap = 0;     // chunks of 64 records
    uint32_t* wsub_cursor = nullptr;                   // (in call_state)
    DevBuf<uint32_t> wide_handed;     // [KMDB_SUBPOOLS] chunks every sub-pool of the wide pool handed out in this call (count_raw_kernel, for the sort)
    uint32_t* run_ctr = nullptr;    // wide-node kernel: next run of every class (in call_state)
    // many streams ("row mode"): the wide records go to per-block-row chunks of the chunk pool; the chunk table grouped by key, then a
    // counting sort inside every row
    bool row_mode = false;
    uint32_t rec_pshift = 0;        // many streams, block width <= 54: the weight digit of a block record lives in the spare bits of its column mask (from
                                    // this bit on) and the record travels as 16 bytes; 0: 16 bytes of masks + the 4-byte key word
    // the chunk table grouped by key: the keys are the streams (row chunks, keyed n_states + row, sit in their rows' lists: rg_*); n_states = never opened
    uint32_t* ct_hist = nullptr;                       // [n_states + 2] (in call_state)
    DevBuf<uint32_t> ct_offs, ct_cursor;            // [n_states + 2]
    DevBuf<void> ct_tmp;
    size_t ct_tmp_bytes = 0;
    DevBuf<uint32_t> rg_hist, rg_offs;   // row chunks grouped by row: [NB][rg_blocks] counts / offsets (+ total)
    DevBuf<uint32_t> row_ids;                          // the row chunks' ids, grouped by row
    uint32_t rg_blocks = 0;
    DevBuf<void> rg_tmp;
    size_t rg_tmp_bytes = 0;
    DevBuf<uint32_t> rs_rows;                          // [2][NB + 1] first job / first table entry of every row
    DevBuf<uint32_t> rs_hist, rs_offs;   // [rs_entries] per row [stream][job] counts / offsets
    uint64_t rs_entries = 0;
    DevBuf<void> rs_tmp;
    size_t rs_tmp_bytes = 0;
    uint64_t sorted_cap = 0;                           // records the sorted arrays (swkey / swrec) hold
    uint32_t last_n_rowjobs = 0, last_n_sorted = 0, last_n_k2jobs = 0, k1w_waves = 0, k1w_slots = 0;   // (k1w_waves: most the pools are sized for; k1w_slots: waves the chip holds at once)
    DevBuf<uint32_t> cs_hist, cs_offs;   // counting sort of the wide pool: [stream][block] counts / offsets (+ total)
    DevBuf<void> cs_tmp;
    size_t cs_tmp_bytes = 0;
    // What every call starts from zero lies in ONE array, cleared by the call's first launch (call_prologue_kernel): the counters, the cursors of the
    // sub-pools, the run and direct counters, the chunk table's histogram and — last, cleared only by a call that decodes — the pair pool's cursors.
    DevBuf<uint32_t> call_state;
    uint32_t call_state_n = 0, call_state_n_decode = 0;    // words a call clears: without / with the pair cursors
    uint32_t* counters = nullptr;   // [KCTR_COUNT] (in call_state)
    uint32_t* h_counters = nullptr; // pinned host copy
    // ---- second level above the block records (a2a_blocks.hip, L2View): the nodes with many blocks write (node, block, mask) entries instead of
    // their c (c + 1) / 2 records; a tile job joins two blocks' lists and applies the matches.  Row mode with few enough blocks only.
    bool l2_on = false;
    uint32_t l2_min_blocks = 24, l2_node_cap = 0, l2_ent_cap = 0, last_l2_nodes = 0;
    DevBuf<uint32_t> l2_cursors;                       // [32 * 16]
    DevBuf<unsigned long long> l2_bitmap;              // [NB][l2_node_cap / 64]
    DevBuf<uint32_t> l2_rank, l2_len, l2_loff;   // [NB][W] rank directory, [NB] list lengths, [NB + 1] list offsets
    DevBuf<uint32_t> l2_ent_g, l2_node_w, l2_list_w;
    DevBuf<uint16_t> l2_ent_blk;
    DevBuf<unsigned long long> l2_ent_mask, l2_list_mask;
    uint64_t est_records = 0;       // sampled estimate for the chosen width
    // what the previous call found (the pipeline is deterministic per database: grid sizes of the next call)
    bool have_counts = false;
    uint32_t last_n_wide = 0, last_n_chunks = 0, last_n_raw = 0;
    uint64_t last_records = 0;
    uint32_t n_slices = 1;          // passes over the pattern stream per call (a database whose records do not fit one)
    struct SliceCounts { bool valid = false; uint32_t lo = 0, hi = 0, n_wide = 0, n_chunks = 0, n_raw = 0, n_rowjobs = 0, n_sorted = 0, n_k2jobs = 0; };
    std::vector<SliceCounts> slice_counts;   // what the previous call found, per slice of the pattern stream
    DevBuf<unsigned char> tile_touched;      // [n_states] != 0: the last call's apply kernels added something to the tile of that block pair (the sparse
                                             // entry point scans only those tiles)
    DevBuf<uint32_t> k2j_start;     // [n_states + 1] many streams: where every stream starts in the sorted arrays
    DevBuf<uint2> k2j_jobs;         // [k2j_cap] jobs of the apply kernel: {stream, part of K2J_REC records}
    uint64_t k2j_cap = 0;
    // ---- a call for a band of rows (kmdb_blocks_run with a kmdb_band_desc): the band as the apply kernels take it, for the call's duration, and the
    // units they counted (BandWin::units; made on the handle's first band call)
    bool band_on = false;
    BandWin band{};
    DevBuf<uint32_t> band_units;    // [BAND_UNIT_SLOTS * BAND_UNIT_WORDS]
    kmdb_blocks_band_units last_band_units{};
    // ---- the geometry the stream-sized and row-sized arrays follow.  The handle's whole-matrix state (kmdb_db.blocks): g_rows = g_bins = NB, g_xlo =
    // g_sbase = 0 and the capacities equal n_states / NB, for good.  The band-emit state (kmdb_db.band_blocks, emit_band): the block rows [g_xlo, g_xhi] of the
    // call's band — n_states = its streams tri32(g_xhi + 1) - g_sbase, g_sbase = tri32(g_xlo), g_rows = g_xhi - g_xlo + 1, g_bins = g_xhi + 1 (the streams of its
    // last row) — set per call inside the capacities the state was made for; a band that needs more gets a new state (kmdb_blocks_band_prepare).
    // NB stays the blocks of the whole collection in both: the lists of the wide kernel and the second level are indexed by block.
    bool emit_band = false;
    uint32_t g_rows = 0, g_bins = 0, g_xlo = 0, g_xhi = 0, g_sbase = 0;
    uint32_t cap_states = 0, cap_rows = 0, cap_bins = 0;
    uint32_t digit_bits = 0;        // != 0: the weight digit bits of an unpacked key word (band emit: the whole call's, so that a weight makes as many records); 0: wide_digit_bits(key_bits)
    uint64_t est_n0 = 0, est_g0 = 0, est_l20 = 0;   // the sampled estimate as the width estimate left it: narrow, wide, and the part the second level replaces
    uint32_t est_stride = 1;
    uint32_t attempts = 0;          // attempts of the last call (1 + repeats)
    std::string gave_up;            // why the last call's attempt gave up at run time ("" = it did not): kmdb_blocks_run publishes it to the handle
    int forced_row_mode = -1;      // band emit: the record path kmdb_blocks_band_prepare chose for the state (0 / 1); -1: by the streams and KMDB_ROW_MODE

    ~BlocksState() { if (h_counters) (void)hipHostFree(h_counters); }
};
void BlocksStateDelete::operator()(BlocksState* b) const { delete b; }

namespace {

inline uint32_t state_digit_bits(const BlocksState& b) { return b.digit_bits ? b.digit_bits : wide_digit_bits(b.key_bits); }
PoolView pool_view(const BlocksState& b, bool dense) {
    return PoolView{b.counters, b.chunk_key, b.chunk_fill, b.rec, b.recw, b.sub_cursor, (uint32_t)(b.pool_cap / KMDB_SUBPOOLS),
                    (uint32_t)b.pool_cap, b.wkey, b.wrec, b.wsub_cursor, (uint32_t)(b.wide_pool_cap / KMDB_SUBPOOLS), dense ? 1u : 0u,
                    (uint32_t)b.key_bits, state_digit_bits(b), b.row_mode ? 1u : 0u, b.n_states, b.rec_pshift};
}
// the tile flags as the apply kernels index them, by absolute stream tri32(X) + Y: the band-emit state holds the flags of the band's streams only, from its
// first stream on (the kernels it launches touch no tile outside the band)
inline unsigned char* touched_view(const BlocksState& b) {
    return b.tile_touched ? (unsigned char*)((uintptr_t)b.tile_touched.get() - (uintptr_t)b.g_sbase) : nullptr;
}

// ---- the emit kernels' instantiations: ONE place maps a handle's record path to the function that is configured, queried and launched
struct K1nPick { void (*fn)(const NParams); const char* name; };
K1nPick k1n_pick(int mode, int minw, bool rows) {
    if (mode == 2) return rows ? K1nPick{k1n_kernel<2, 4, true>, "k1n<2, rows>"} : K1nPick{k1n_kernel<2, 4, false>, "k1n<2, no rows>"};
    if (mode == 0) return rows ? K1nPick{k1n_kernel<0, 4, true>, "k1n<0, rows>"} : K1nPick{k1n_kernel<0, 4, false>, "k1n<0, no rows>"};
    if (minw >= 4) return rows ? K1nPick{k1n_kernel<1, 4, true>, "k1n<1, 4 waves, rows>"} : K1nPick{k1n_kernel<1, 4, false>, "k1n<1, 4 waves, no rows>"};
    return rows ? K1nPick{k1n_kernel<1, 3, true>, "k1n<1, 3 waves, rows>"} : K1nPick{k1n_kernel<1, 3, false>, "k1n<1, 3 waves, no rows>"};
}
struct K1wPick { void (*fn)(const WParams); const char* name; };
K1wPick k1w_pick(bool rows, bool l2) {
    if (!rows) return K1wPick{k1w_kernel<false, false>, "k1w<no rows, no L2>"};
    return l2 ? K1wPick{k1w_kernel<true, true>, "k1w<rows, L2>"} : K1wPick{k1w_kernel<true, false>, "k1w<rows, no L2>"};
}
// the band-emit instantiations (the state's k1n_mode is 0 or 2: kmdb_blocks_band_prepare)
K1nPick k1n_band_pick(int mode, bool rows) {
    if (mode == 2) return rows ? K1nPick{k1n_band_kernel<2, true>, "k1n band<2, rows>"} : K1nPick{k1n_band_kernel<2, false>, "k1n band<2, no rows>"};
    return rows ? K1nPick{k1n_band_kernel<0, true>, "k1n band<0, rows>"} : K1nPick{k1n_band_kernel<0, false>, "k1n band<0, no rows>"};
}
K1wPick k1w_band_pick(bool rows, bool l2) {
    if (!rows) return K1wPick{k1w_band_kernel<false, false>, "k1w band<no rows, no L2>"};
    return l2 ? K1wPick{k1w_band_kernel<true, true>, "k1w band<rows, L2>"} : K1wPick{k1w_band_kernel<true, false>, "k1w band<rows, no L2>"};
}

constexpr uint32_t K1W_MAX_WAVES = 8192;
struct U32toU64 { __host__ __device__ unsigned long long operator()(uint32_t v) const { return v; } };
struct ValidKey { uint32_t n_states, kmask; __host__ __device__ uint32_t operator()(uint32_t k) const { return (k & kmask) < n_states ? 1u : 0u; } };

// Record slots a pool can index.  Slot numbers are 32-bit; the few-streams path hands slot counts to rocPRIM as int (2^31).  The many-streams
// path (row mode) is the engine's own kernels throughout: 2^32 minus a margin (the slot after the last chunk must not wrap to the
// "no open chunk" value 0 of the row tables, and the windows of the apply kernel round the record count up).
inline uint64_t pool_slot_limit(const BlocksState& b) { return b.row_mode ? (1ull << 32) - (1ull << 20) : (1ull << 31); }

int alloc_record_pool(BlocksState& b, hipStream_t st, uint64_t chunks) {
    // (all the old arrays go before the first new one comes)
    dev_reset(b.chunk_key, b.chunk_fill, b.sorted_key, b.sorted_id, b.rec, b.recw, b.sort_tmp, b.rs_hist, b.rs_offs, b.rs_tmp);
    b.pool_cap = 0;
    chunks = (chunks + (uint64_t)KMDB_SUBPOOLS * ARENA_GRAB - 1) / ((uint64_t)KMDB_SUBPOOLS * ARENA_GRAB) * ((uint64_t)KMDB_SUBPOOLS * ARENA_GRAB);
    if (chunks >= pool_slot_limit(b) >> CH_SHIFT) return kmdb_set_error("kmdb: record pool would exceed its " + std::to_string(pool_slot_limit(b)) + " record slots");
    DEV_ALLOC(b.chunk_key, chunks);
    DEV_ALLOC(b.chunk_fill, chunks);
    DEV_ALLOC(b.sorted_key, chunks);
    DEV_ALLOC(b.sorted_id, chunks);
    DEV_ALLOC(b.rec, (chunks << CH_SHIFT) * 16);
    DEV_ALLOC(b.recw, chunks << CH_SHIFT);
    {
        rocprim::transform_iterator<uint32_t*, U32toU64, unsigned long long> it(b.chunk_fill, U32toU64());
        HIP_TRY(prim::sum(nullptr, b.sort_tmp_bytes, it, (unsigned long long*)nullptr, (int)chunks, st));
    }
    DEV_ALLOC(b.sort_tmp, std::max<size_t>(b.sort_tmp_bytes, 16));
    if (b.row_mode) {
        // the row chunks grouped by row: [row][workgroup of RG_THREADS chunk ids] counts / offsets, the grouped ids
        dev_reset(b.rg_hist, b.rg_offs, b.rg_tmp, b.row_ids);
        b.rg_blocks = (uint32_t)((chunks + RG_THREADS - 1) / RG_THREADS);
        const size_t rg_ne = (size_t)b.cap_rows * b.rg_blocks + 1;
        DEV_ALLOC(b.rg_hist, rg_ne);
        DEV_ALLOC(b.rg_offs, rg_ne);
        DEV_ALLOC(b.row_ids, chunks);
        HIP_TRY(prim::exclusive_sum(nullptr, b.rg_tmp_bytes, b.rg_hist.get(), b.rg_offs.get(), (int)rg_ne, st));
        DEV_ALLOC(b.rg_tmp, std::max<size_t>(b.rg_tmp_bytes, 16));
        // the sort inside the rows: at most chunks / RS_JOB_CHUNKS + NB jobs, every one with at most NB bins (band emit: the band's rows, the bins of its last row)
        b.rs_entries = (chunks / RS_JOB_CHUNKS + b.cap_rows + 1) * (uint64_t)b.cap_bins + 1;
        if (b.rs_entries >= (1ull << 31)) return kmdb_set_error("kmdb: the table of the sort inside the block rows would exceed 2^31 entries");
        DEV_ALLOC(b.rs_hist, b.rs_entries);
        DEV_ALLOC(b.rs_offs, b.rs_entries);
        HIP_TRY(prim::exclusive_sum(nullptr, b.rs_tmp_bytes, b.rs_hist.get(), b.rs_offs.get(), (int)b.rs_entries, st));
        DEV_ALLOC(b.rs_tmp, std::max<size_t>(b.rs_tmp_bytes, 16));
    }
    b.pool_cap = chunks;
    return 0;
}
// few streams: the wide pool (records in arrival order + their stream keys) and the sorted copies; many streams (row mode): the
// sorted arrays only — the wide records travel through row chunks of the chunk pool
int alloc_wide_pool(BlocksState& b, hipStream_t st, uint64_t chunks) {
    dev_reset(b.wkey, b.wrec, b.swkey, b.swrec);
    b.wide_pool_cap = 0; b.sorted_cap = 0;
    // (a pool handed out through the 256 sub-pools holds a whole grab of each.  The band-emit state on the many-streams path has no such pool: its wide records
    // travel through row chunks, what is allocated here are the sorted arrays alone, and those are sized for the band's records to the chunk)
    if (!(b.emit_band && b.row_mode))
        chunks = (chunks + (uint64_t)KMDB_SUBPOOLS * WIDE_GRAB - 1) / ((uint64_t)KMDB_SUBPOOLS * WIDE_GRAB) * ((uint64_t)KMDB_SUBPOOLS * WIDE_GRAB);
    chunks = std::max<uint64_t>(chunks, 1);
    const uint64_t slots = chunks << WCH_SHIFT;
    if (slots >= pool_slot_limit(b)) return kmdb_set_error("kmdb: wide record pool would exceed its " + std::to_string(pool_slot_limit(b)) + " record slots");
    DEV_ALLOC(b.swkey, slots);
    DEV_ALLOC(b.swrec, slots);
    b.sorted_cap = slots;
    // jobs of the apply kernel: every stream at least one, a long one a job per K2J_REC records
    b.k2j_cap = slots / K2J_REC + b.cap_states + 1;
    DEV_ALLOC(b.k2j_jobs, b.k2j_cap);
    if (b.row_mode) {
        b.wide_pool_cap = chunks;
        return 0;
    }
    DEV_ALLOC(b.wkey, slots);
    DEV_ALLOC(b.wrec, slots);
    if (!b.cs_hist) {
        // one pass: [stream][workgroup]
        const size_t ne = (size_t)b.cap_states * CS_BLOCKS_ONE + 1;
        DEV_ALLOC(b.cs_hist, ne);
        DEV_ALLOC(b.cs_offs, ne);
        HIP_TRY(prim::exclusive_sum(nullptr, b.cs_tmp_bytes, b.cs_hist.get(), b.cs_offs.get(), (int)ne, st));
        DEV_ALLOC(b.cs_tmp, std::max<size_t>(b.cs_tmp_bytes, 16));
    }
    b.wide_pool_cap = chunks;
    return 0;
}
int alloc_pair_pool(BlocksState& b, uint64_t entries) {
    dev_reset(b.pair_blk, b.pair_mask);
    entries = (entries + KMDB_PAIR_REGIONS - 1) / KMDB_PAIR_REGIONS * KMDB_PAIR_REGIONS;
    if (entries >= (1ull << 32)) return kmdb_set_error("kmdb: pair pool would exceed 2^32 entries");
    DEV_ALLOC(b.pair_blk, entries + 32);            // (64 bytes beyond the entries, as for the masks)
    DEV_ALLOC(b.pair_mask, entries + 8);
    b.pair_cap = entries;
    return 0;
}

}  // namespace

// ------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------
// db2db (csrc/db2db.hip): records (row block, column block, row mask, column mask, weight digit in the key word) of the pairs of
// patterns that share k-mers, in arrival order in [0, nslots) with never-written slots keyed all-ones -> sorted by stream and
// accumulated into the dense n_rows x n_cols matrix M by the same sort and matrix-core kernels as the all2all's wide pool.
int kmdb_rect_sort_apply(hipStream_t st, uint32_t* wkey, void* wrec, uint32_t nslots, uint32_t nbr, uint32_t nbc, int key_bits, uint32_t* M, uint32_t n_rows,
                         uint32_t n_cols) {
    if (!nslots) return 0;
    const uint32_t n_states = nbr * nbc, kmask = (1u << key_bits) - 1u;
    DevBuf<uint32_t> swkey, hist, offs;
    DevBuf<WideRec> swrec;
    DevBuf<void> tmp;
    DEV_ALLOC(swkey, (size_t)nslots);
    DEV_ALLOC(swrec, (size_t)nslots);
    const uint32_t* total_ptr = nullptr;
    if (n_states <= CS_MAX_KEYS) {
        const size_t ne = (size_t)n_states * CS_BLOCKS_ONE + 1;
        size_t tb = 0;
        DEV_ALLOC(hist, ne);
        DEV_ALLOC(offs, ne);
        HIP_TRY(prim::exclusive_sum(nullptr, tb, hist.get(), offs.get(), (int)ne, st));
        DEV_ALLOC(tmp, std::max<size_t>(tb, 16));
        hipLaunchKernelGGL(cs_hist_kernel, dim3(CS_BLOCKS_ONE), dim3(256), n_states * 4, st, wkey, nslots, n_states, n_states, kmask, hist,
                           (const uint32_t*)nullptr);              // (this pool's key words are filled by its owner)
        HIP_TRY(prim::exclusive_sum(tmp, tb, hist.get(), offs.get(), (int)ne, st));
        HIP_TRY(hipFuncSetAttribute((const void*)cs_scatter_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)cs_scatter_lds(n_states, false)));
        hipLaunchKernelGGL(cs_scatter_kernel, dim3(CS_BLOCKS_ONE), dim3(CS_THREADS), cs_scatter_lds(n_states, false), st, wkey, (const WideRec*)wrec, nslots, n_states, n_states,
                           kmask, offs, swkey, swrec, 0u, (const uint32_t*)nullptr);
        total_ptr = offs + (ne - 1);
    } else {
        size_t tb = 0;
        HIP_TRY(prim::sort_pairs(nullptr, tb, wkey, swkey.get(), (WideRec*)wrec, swrec.get(), (int)nslots, 0, key_bits, st));
        DEV_ALLOC(tmp, std::max<size_t>(tb, 16));
        HIP_TRY(prim::sort_pairs(tmp, tb, wkey, swkey.get(), (WideRec*)wrec, swrec.get(), (int)nslots, 0, key_bits, st));
    }
    hipLaunchKernelGGL(k2_sorted_kernel, dim3((nslots + K2S_WIN - 1) / K2S_WIN), dim3(256), 0, st, swkey, (const WideRec*)swrec, nslots, total_ptr,
                       n_states, (uint32_t)key_bits, wide_digit_bits(key_bits), M, n_rows, 64u, nbc, n_cols);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(st));
    return 0;
}

static int blocks_prepare_impl(kmdb_db* db);
static uint64_t state_device_bytes(const kmdb_db* db, const BlocksState& b);
static int blocks_alloc_working_set(kmdb_db* db, BlocksState& b, uint64_t est_n, uint64_t est_g, uint64_t est_l2, uint32_t stride,
                                    const std::function<void(const char*)>& phase);
// (the flag is set only when every allocation succeeded: a failed lazy preparation inside a call leaves nothing half made behind)
int kmdb_blocks_prepare(kmdb_db* db) {
    db->blocks.reset(new BlocksState());
    if (blocks_prepare_impl(db)) { kmdb_blocks_release(db); return 1; }
    db->blocks_prepared = true;
    return 0;
}
static int blocks_prepare_impl(kmdb_db* db) {
    BlocksState& b = *db->blocks;
    b.knobs = blocks_read_knobs();
    const BlocksKnobs& knobs = b.knobs;
    const uint64_t N = db->N, P = db->P;
    db->fallback_reason.clear();
    if (N < 2 || P == 0) { db->fallback_reason = "fewer than two samples"; return 0; }
    if (!db->chain_ok) {
        db->fallback_reason = "a root path of " + std::to_string(db->max_depth) + " nodes exceeds the chain table (" + std::to_string(KMDB_CHAIN_MAX) + ")";
        return 0;
    }
    const bool verbose = kmdb_verbose();
    auto t_mark = std::chrono::steady_clock::now();
    auto phase = [&](const char* what) {                        // where the preparation's time goes (hipMalloc of tens of GB is not free)
        if (!verbose) return;
        (void)hipStreamSynchronize(db->stream);
        const auto now = std::chrono::steady_clock::now();
        fprintf(stderr, "[kmdb] prepare: %-36s %.3f s\n", what, std::chrono::duration<double>(now - t_mark).count());
        t_mark = now;
    };
    // ---- block width: fewer sample ids per block than 64 pay off when the samples cluster (clades, species) in id
    // ranges that a 64-id grid would cut in two.  One node in `stride` is decoded along its whole root path and its
    // blocks are counted for every candidate at once; the candidate with the fewest records wins.
    const uint32_t cands[EST_NW] = {64, 60, 56, 52, 50, 48, 44, 40, 36, 32};
    const uint32_t forced = knobs.block_width;
    const uint32_t stride = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(1024, P / 65536));
    uint64_t est_n = 0, est_g = 0, est_l2 = 0;                  // records of the nodes with <= 2 blocks, of the others, and of those the part the second level replaces
    {
        EstParams q{};
        q.k0in = db->k0in; q.bitrel = db->bitrel; q.blkbase = db->blkbase; q.bits = db->bits; q.parent = db->parent; q.nl = db->nl; q.w = db->w;
        q.P = (uint32_t)P; q.stride = stride;
        for (int c = 0; c < EST_NW; ++c) { q.widths[c] = cands[c]; q.magics[c] = (uint32_t)((1ull << 32) / cands[c]) + 1u; }
        q.l2_min = knobs.l2_min;
        DevBuf<unsigned long long> d_out;
        DEV_ALLOC(d_out, 3 * EST_NW + 1);
        q.out = d_out;
        HIP_TRY(hipMemsetAsync(q.out, 0, (3 * EST_NW + 1) * 8, db->stream));
        const uint64_t nthreads = (P + stride - 1) / stride;
        hipLaunchKernelGGL(width_estimate_kernel, dim3((unsigned)((nthreads + 63) / 64)), dim3(64), 0, db->stream, q);
        HIP_TRY(hipGetLastError());
        unsigned long long h[3 * EST_NW + 1];
        HIP_TRY(hipMemcpyAsync(h, q.out, sizeof h, hipMemcpyDeviceToHost, db->stream));
        HIP_TRY(hipStreamSynchronize(db->stream));
        int best = 0;
        for (int c = 1; c < EST_NW; ++c) if (h[c] + h[EST_NW + c] < h[best] + h[EST_NW + best]) best = c;
        if (forced) {
            db->width = forced;
            best = 0;
            for (int c = 0; c < EST_NW; ++c) if (cands[c] >= forced) best = c;
        } else db->width = cands[best];
        est_n = h[best] * stride; est_g = h[EST_NW + best] * stride; est_l2 = h[2 * EST_NW + 1 + best] * stride;
        b.est_records = est_n + est_g;
        b.est_n0 = est_n; b.est_g0 = est_g; b.est_l20 = est_l2; b.est_stride = stride;      // (kept for the band-emit state, which scales them to its band)
        if (verbose) {
            fprintf(stderr, "[kmdb] width estimate (1 node in %u, %llu sampled):", stride, h[2 * EST_NW]);
            for (int c = 0; c < EST_NW; ++c) fprintf(stderr, " %u:%llu", cands[c], (h[c] + h[EST_NW + c]) * stride);
            fprintf(stderr, " -> width %u\n", db->width);
        }
    }
    b.NB = (uint32_t)((N + db->width - 1) / db->width);
    const uint64_t n_states = (uint64_t)b.NB * (b.NB + 1) / 2;          // streams = block pairs
    if (n_states + 1 >= (1ull << 22)) { db->fallback_reason = "too many block pairs"; return 0; }          // 22 stream bits + 8-bit weight digits in a key word
    static_assert((1ull << 22) < (uint64_t)BNONE * (BNONE + 1ull) / 2ull, "fewer than 2^22 block pairs keep the block index (< 2897) below BNONE and inside pair_blk's 16 bits");
    b.n_states = (uint32_t)n_states;
    if (k1w_wave_bytes(std::max<uint32_t>(K1W_ARENA_MIN, (b.NB + 2u + 63u) & ~63u), (b.NB + 2u + 3u) & ~3u, db->chain_cap, b.NB) > (size_t)(152u << 10)) {
        db->fallback_reason = "the lists of the wide-node kernel do not fit the LDS (" + std::to_string(b.NB) + " blocks, root paths of up to " +
                              std::to_string(db->max_depth) + " nodes)";
        return 0;
    }
    phase("block width estimate");
    // (the whole matrix: every block row, every stream, for good)
    b.cap_states = b.n_states; b.g_rows = b.g_bins = b.cap_rows = b.cap_bins = b.NB; b.g_xlo = 0; b.g_xhi = b.NB - 1u; b.g_sbase = 0;
    return blocks_alloc_working_set(db, b, est_n, est_g, est_l2, stride, phase);
}
// The working set of a state whose geometry is set (NB, n_states, the g_* and cap_* of BlocksState) from the sampled estimate of ITS records: the per-node
// arrays, the per-call state, the pair pool, the record paths chosen, the arrays sized by streams and rows, the pools.  The whole-matrix state and the
// band-emit state are both made here.
static int blocks_alloc_working_set(kmdb_db* db, BlocksState& b, uint64_t est_n, uint64_t est_g, uint64_t est_l2, uint32_t stride,
                                    const std::function<void(const char*)>& phase) {
    const BlocksKnobs& knobs = b.knobs;
    const uint64_t P = db->P;
    const bool verbose = kmdb_verbose();
    // ---- working set
    DEV_ALLOC(b.p0_mask, P);
    DEV_ALLOC(b.p0_info, P);
    DEV_ALLOC(b.pair_ofs, P);
    DEV_ALLOC(b.fn_mask, P);
    DEV_ALLOC(b.fn_blk, P);
    const uint64_t n_words = (P + 63) / 64;
    DEV_ALLOC(b.widebits, n_words);
    DEV_ALLOC(b.wide_base, n_words + 1);
    DEV_ALLOC(b.wide_slice_cnt, std::max<size_t>(db->n_nsegs, 1));
    DEV_ALLOC(b.wide_slice_base, (size_t)db->n_nsegs + 1);
    DEV_ALLOC(b.wide_handed, KMDB_SUBPOOLS);
    {
        // the per-call state at fixed offsets (the chunk table's keys are the streams)
        uint32_t o = 0;
        auto take = [&](uint32_t n) { const uint32_t at = o; o += (n + 15u) & ~15u; return at; };
        const uint32_t o_ctr = take(KCTR_COUNT), o_sub = take(KMDB_SUBPOOLS * 16), o_wsub = take(KMDB_SUBPOOLS * 16), o_run = take(K1W_CTRS * 16),
                       o_dir = take(KMDB_SUBPOOLS * 16), o_cth = take(b.cap_states + 2);
        b.call_state_n = o;
        const uint32_t o_pair = take((KMDB_PAIR_REGIONS + 1) * 16);
        b.call_state_n_decode = o;
        DEV_ALLOC(b.call_state, o);
        uint32_t* s = b.call_state;
        b.counters = s + o_ctr; b.sub_cursor = s + o_sub; b.wsub_cursor = s + o_wsub; b.run_ctr = s + o_run; b.direct_ctr = s + o_dir; b.ct_hist = s + o_cth;
        b.pair_cursor = s + o_pair;
    }
    HIP_TRY(hipHostMalloc((void**)&b.h_counters, KCTR_COUNT * 4));
    phase("per-node arrays (hipMalloc)");
    {
        // extra pairs: sampled with the chosen width (K0 reserves min(l - 1, blocks spanned) per list that is not a single short run)
        DevBuf<unsigned long long> d_need;
        DEV_ALLOC(d_need, 1);
        HIP_TRY(hipMemsetAsync(d_need, 0, 8, db->stream));
        const BlockMap bm{db->width, (uint32_t)((1ull << 32) / db->width) + 1u};
        const uint64_t nthreads = (P + stride - 1) / stride;
        hipLaunchKernelGGL(pair_estimate_kernel, dim3((unsigned)((nthreads + 63) / 64)), dim3(64), 0, db->stream, db->k0in, db->bitrel, db->blkbase, db->bits,
                           (uint32_t)P, stride, bm, d_need);
        unsigned long long h_need = 0;
        HIP_TRY(hipMemcpyAsync(&h_need, d_need, 8, hipMemcpyDeviceToHost, db->stream));
        HIP_TRY(hipStreamSynchronize(db->stream));
        d_need.reset();
        const uint64_t est_pairs = h_need * stride;
        if (verbose) fprintf(stderr, "[kmdb] extra (block, mask) pairs, sampled: %llu\n", (unsigned long long)est_pairs);
        // (twice the estimate: three quarters of the pool are wave-private sub-pools, and a sub-pool that runs out sends its waves to the shared
        // rest behind ONE cursor — with 1.25 x the estimate the sub-pools were nearly full and the decode launches took 3.9 instead of 2.2 ms at C2,
        // profiles/r06_j6: same-address device atomics)
        if (alloc_pair_pool(b, std::max<uint64_t>(est_pairs * 2 + P / 4, (uint64_t)KMDB_PAIR_REGIONS * 64))) return 1;
    }
    phase("pair estimate + pair pool");
    // Where the records go.  The narrow kernel's first-block diagonal records follow the clustering of the DFS stream: per-stream
    // chunks (an open chunk per block and wave), applied straight from the grouped chunk table.  The other records spread over
    // many streams, a few per stream and wave:
    //   few streams (<= CS_MAX_KEYS):  arrival order into the wide pool, ONE counting-sort pass by stream (measured: 5 x faster than
    //                                  per-stream reservations);
    //   many streams ("row mode"):     per-BLOCK-ROW chunks (an open chunk per row and wave, slots by LDS atomics), so the records
    //                                  arrive grouped by row and only the counting sort inside the rows remains (a scatter straight
    //                                  to 20 100 streams is bound by the number of write requests: measured 25.8 ms for 495 M records;
    //                                  grouping by row in a pass of its own cost another 7.5 ms).
    // With more streams than the narrow kernel's open-chunk table holds it sends its diagonal records the same way, if its chunks turn
    // out to be evicted nearly empty.
    b.dense_narrow = knobs.dense_narrow;
    // Round 6: the narrow kernel's first-block records no longer travel through stream chunks (BlocksState: k1n_mode; KMDB_K1N_MODE=0 / 1 / 2
    // for the A/B): compacted per slice and applied by k2d_kernel beside the wide kernel (2, default), or applied inside the narrow kernel (1).
    b.k1n_mode = knobs.k1n_mode;
    if (b.k1n_mode) b.dense_narrow = true;
    if (b.k1n_mode == 2) {
        const size_t slots = (size_t)db->n_nsegs * db->nseg_nodes;
        DEV_ALLOC(b.dmask, std::max<size_t>(slots, 1));
        DEV_ALLOC(b.dwx, std::max<size_t>(slots, 1));
        DEV_ALLOC(b.slice_cnt, std::max<size_t>(db->n_nsegs, 1));
    }
    b.row_mode = b.n_states > CS_MAX_KEYS;
    if (knobs.row_mode >= 0) b.row_mode = knobs.row_mode != 0;
    if (b.forced_row_mode >= 0) b.row_mode = b.forced_row_mode != 0;          // (the band-emit state: decided with the one-pass sort's LDS in view)
    // packed records: a block width of at most 54 leaves the column mask 10 spare bits and more — an 8-bit weight digit at least and the digit's
    // index — so the records of the many-streams path travel as 16 bytes through the sort and the apply step (KMDB_REC_PACKED=0: 16 + 4, A/B)
    // (round 5, later: the few-streams path as well — its one-pass sort moves 16 bytes per record and leaves the key words behind)
    b.rec_pshift = (db->width <= 54u && knobs.rec_packed) ? db->width : 0u;
    // The second level: many streams, few enough blocks that a tile job's bitmap scan stays small (tiles x nodes: quadratic in the blocks);
    // KMDB_L2=0 switches it off, KMDB_L2_MIN=c moves the threshold.  It writes no records for the nodes with L2_MIN_BLOCKS blocks or more — 52 % of the
    // estimate at 10 000 samples.  Round 5 sized the pools from the estimate before it: 110 GB for 616 M records of 16 bytes.
    b.l2_on = b.row_mode && b.NB <= 256u && knobs.l2;
    b.l2_min_blocks = knobs.l2_min;
    if (b.l2_on) {
        if (verbose) fprintf(stderr, "[kmdb] block records estimated: %llu, of them %llu from nodes the second level joins per tile instead\n",
                             (unsigned long long)(est_n + est_g), (unsigned long long)est_l2);
        est_g -= std::min(est_g, est_l2);
    }
    {
        int key_bits = 1;
        while ((1ull << key_bits) <= (uint64_t)b.n_states + 1) ++key_bits;          // streams; all-ones = never written
        b.key_bits = key_bits;
    }
    DEV_ALLOC(b.tile_touched, (size_t)b.cap_states + 1);
    DEV_ALLOC(b.ct_offs, (size_t)b.cap_states + 2);
    DEV_ALLOC(b.ct_cursor, (size_t)b.cap_states + 2);
    HIP_TRY(prim::exclusive_sum(nullptr, b.ct_tmp_bytes, b.ct_hist, b.ct_offs.get(), (int)(b.cap_states + 1), db->stream));
    DEV_ALLOC(b.ct_tmp, std::max<size_t>(b.ct_tmp_bytes, 16));
    // A database whose records do not fit one pass (2^31 record slots, or the memory left) is taken in SLICES of the pattern stream:
    // every slice emits the records of its own patterns only, the partial matrices add up in place (the engine's own version of
    // kmdb_opts.shard_index / shard_count; the reference blocks by `-buffer` the same way, similarity_calculator.cpp:290-325).
    {
        uint64_t slices = 1;
        const uint64_t slots = (est_n + est_g) * 3 / 2;
        const uint64_t usable = pool_slot_limit(b) / 4 * 3;                                            // three quarters of the slots a pool can index
        slices = std::max<uint64_t>(slices, (slots + usable - 1) / usable);
        size_t free_b = 0, total_b = 0;
        if (hipMemGetInfo(&free_b, &total_b) == hipSuccess && free_b)
            slices = std::max<uint64_t>(slices, (slots * 44 + free_b / 2) / std::max<size_t>(free_b * 6 / 10, 1));     // pool + sorted copy: 44 B per slot, 60 % of what is free
        if (knobs.slices) slices = knobs.slices;
        b.n_slices = (uint32_t)std::min<uint64_t>(slices, 1u << 16);
        if (verbose && b.n_slices > 1) fprintf(stderr, "[kmdb] %llu block records estimated: %u slices of the pattern stream per call\n",
                                                 (unsigned long long)(est_n + est_g), b.n_slices);
        est_n = est_n / b.n_slices + 1; est_g = est_g / b.n_slices + 1;
    }
    if (knobs.pool_percent) {
        // (tests: pools far too small, so that the first call takes the enlarge-and-repeat path on every one of them)
        const uint64_t pct = knobs.pool_percent;
        est_n = est_n * pct / 100 + 1; est_g = est_g * pct / 100 + 1;
    }
    // waves of the wide-node kernel: in row mode every wave may end with an open chunk per block row
    b.k1w_waves = K1W_MAX_WAVES;
    if (b.row_mode) {
        b.k1w_waves = std::min<uint32_t>(b.k1w_waves, std::max<uint32_t>(256u, std::min<uint32_t>(4096u, (1u << 21) / std::max<uint32_t>(b.cap_rows, 1u))));
        DEV_ALLOC(b.rs_rows, (size_t)2 * (b.cap_rows + 1));
    }
    DEV_ALLOC(b.k2j_start, (size_t)b.cap_states + 2);
    // stream chunks: the narrow estimate at two thirds average fill, plus what the waves hold when they end (open chunks, an
    // unfinished grab); wide records: the wide estimate at two thirds (+ a grab / the open row chunks per wave)
    // (modes 1 and 2: of the narrow kernel's first-block records only the stragglers go to the pools — weights of 128 and more, in mode 1 also a
    // slice's nodes outside its tile: a sixteenth of the estimate is generous, and a pool that is too small is enlarged as ever)
    if (b.k1n_mode) { est_g += est_n / 16 + 1; est_n = 0; }
    if (b.row_mode) {
        // the estimate (one node in `stride`, exact per node) plus a quarter, plus what the waves hold when they end (open chunks, unfinished grabs); the
        // sorted copy holds the records themselves: the estimate plus an eighth.  A pool that turns out too small is enlarged and the call repeated.
        // (chunks, not records, are what runs out: every wave keeps an open chunk per block row it writes to — the wide kernel's waves all rows, a
        // slice of the narrow kernel the rows of its nodes' second blocks, up to 48 counted here — and leaves it partly filled.  Round 5's pools hid
        // that behind the records the second level no longer writes; with the estimate after the second level and 12 chunks per slice the first
        // call at 10 000 samples ran out and doubled its pool: profiles/r06_close_bench.err)
        if (alloc_record_pool(b, db->stream, (est_n + est_g) * 5 / 4 / CH_REC + (uint64_t)db->n_nsegs * std::min<uint32_t>(b.cap_rows, 48u) + (uint64_t)b.k1w_waves * (b.cap_rows + ARENA_GRAB) + 4096)) return 1;
        // (the band-emit state: the sorted arrays follow the BAND's records — its estimate plus an eighth plus 4096 records for what a sampled estimate
        // of a few rows misses, the margin under KMDB_POOL_PERCENT at that percentage too — not the 4096 chunks the whole matrix's arrays start from)
        const uint64_t sorted_chunks = b.emit_band ? ((est_n + est_g) * 9 / 8 + 4096 * (knobs.pool_percent ? std::min<uint64_t>(knobs.pool_percent, 100) : 100) / 100) / WCH_REC + 1
                                                   : (est_n + est_g) * 9 / 8 / WCH_REC + 4096;
        if (alloc_wide_pool(b, db->stream, sorted_chunks)) return 1;
    } else {
        if (alloc_record_pool(b, db->stream, est_n * 3 / 2 / CH_REC + (b.dense_narrow ? 0u : (uint64_t)db->n_nsegs * 8) + 4096)) return 1;
        if (alloc_wide_pool(b, db->stream, est_g * 3 / 2 / WCH_REC + (uint64_t)(K1W_MAX_WAVES + 64) * (WIDE_GRAB + 2) + (uint64_t)db->n_nsegs * (WIDE_GRAB / 2) + 1024)) return 1;
    }
    if (verbose) fprintf(stderr, "[kmdb] prepare: record pools %.2f GB\n", state_device_bytes(db, b) / 1e9);
    phase("record pools (hipMalloc)");
    return 0;
}

// the state's destructor frees every array it holds
void kmdb_blocks_release(kmdb_db* db) { db->blocks.reset(); }

static uint64_t state_device_bytes(const kmdb_db* db, const BlocksState& b) {
    if (!b.counters) return 0;
    return db->P * (8 + 4 + 4 + 16 + 4) + (b.dmask ? (uint64_t)db->n_nsegs * db->nseg_nodes * 12 : 0u) + b.pair_cap * 10 + ((b.pool_cap << CH_SHIFT) * 20) + b.pool_cap * 16 + b.wide_cap * 4 + (db->P / 64) * 12 + (uint64_t)db->n_nsegs * 8 +
           (uint64_t)b.call_state_n_decode * 4 +
           (b.wide_pool_cap << WCH_SHIFT) * (b.row_mode ? 20 : 40) + b.rs_entries * 8 + (uint64_t)b.cap_states * 12 +
           (uint64_t)b.NB * (b.l2_node_cap / 64u) * 12 + (uint64_t)b.l2_ent_cap * 26 + (uint64_t)b.l2_node_cap * 4;
}
uint64_t kmdb_blocks_state_bytes(const kmdb_db* db, bool band_state) {
    const BlocksState* s = band_state ? db->band_blocks.get() : db->blocks.get();
    return s ? state_device_bytes(db, *s) : 0u;
}
// both states of the handle: the whole matrix's and, once a band-emit call made it, the band's
uint64_t kmdb_blocks_device_bytes(const kmdb_db* db) { return kmdb_blocks_state_bytes(db, false) + kmdb_blocks_state_bytes(db, true); }

namespace {

// second level (L2View): arrays for node_cap node indices and ent_cap entries; frees what was there
int alloc_l2(BlocksState& b, uint32_t node_cap, uint32_t ent_cap) {
    dev_reset(b.l2_cursors, b.l2_bitmap, b.l2_rank, b.l2_len, b.l2_loff, b.l2_ent_g, b.l2_node_w, b.l2_list_w, b.l2_ent_blk, b.l2_ent_mask, b.l2_list_mask);
    b.l2_node_cap = 0; b.l2_ent_cap = 0;
    node_cap = (node_cap + 64u * L2_SUB - 1u) / (64u * L2_SUB) * (64u * L2_SUB);
    ent_cap = (ent_cap + L2_ENT_GRAB * L2_SUB - 1u) / (L2_ENT_GRAB * L2_SUB) * (L2_ENT_GRAB * L2_SUB);
    const size_t W = node_cap / 64u, NB = b.NB;
    DEV_ALLOC(b.l2_cursors, 2 * L2_SUB * 16);
    DEV_ALLOC(b.l2_bitmap, NB * W);
    DEV_ALLOC(b.l2_rank, NB * W);
    DEV_ALLOC(b.l2_len, NB);
    DEV_ALLOC(b.l2_loff, NB + 2);
    DEV_ALLOC(b.l2_ent_g, (size_t)ent_cap);
    DEV_ALLOC(b.l2_ent_blk, (size_t)ent_cap);
    DEV_ALLOC(b.l2_ent_mask, (size_t)ent_cap);
    DEV_ALLOC(b.l2_list_mask, (size_t)ent_cap);
    DEV_ALLOC(b.l2_list_w, (size_t)ent_cap);
    DEV_ALLOC(b.l2_node_w, (size_t)node_cap);
    b.l2_node_cap = node_cap; b.l2_ent_cap = ent_cap;
    return 0;
}

// ---- One attempt of the whole pipeline (blocks_attempt, below) as its stages, in the order the call runs them.
// Sizes of the launches: measured by the previous call on this handle.  What the narrow kernel produces repeats exactly; where
// the wide kernel's records land depends on which wave took which run, so the chunk counts behind it vary a little from call
// to call: those launches get some slack, every kernel takes the true counts from device memory, and the call is repeated with
// upper bounds if a true count exceeded its launch (checked at the end).
struct Launched { uint32_t raw = 0, rowjobs = 0, k2jobs = 0; };
inline uint32_t with_slack(uint32_t v) { return v + v / 8u + 1024u; }
// KMDB_SYNC_DEBUG: wait after every stage and name the one that failed (debugging aid, no effect on results)
int stage_done(hipStream_t s, const char* name) {
    if (!kmdb_sync_debug()) return 0;
    const hipError_t e = hipStreamSynchronize(s);
    fprintf(stderr, "[kmdb] stage %-14s %s\n", name, e == hipSuccess ? "ok" : hipGetErrorString(e));
    return e == hipSuccess ? 0 : kmdb_set_error(std::string("stage ") + name + ": " + hipGetErrorString(e));
}
// ---- 1. the call's state in one launch: counters, cursors and the chunk table's histogram cleared (the pair pool's cursors with them when this
// attempt decodes: later slices of a call reuse the decode), every chunk empty and never opened.  The host is not ahead of the queue yet: every
// further submission here is a gap on the device (profiles/prologue_c2_timeline_*.md).  The wide pool's key words are not touched: which slots
// hold a record of this call follows from the sub-pools' cursors (cs_chunks_handed, arena_finish_wide).
void a2a_prologue(BlocksState& b, hipStream_t st, bool decode) {
    // (the attempt that decodes is the first of its call: the tiles the call adds to, all its slices, are flagged from here on)
    const uint32_t pool_cap = (uint32_t)b.pool_cap;
    const uint32_t n_state = decode ? b.call_state_n_decode : b.call_state_n, n_touched = decode && b.tile_touched ? b.n_states + 1u : 0u;
    hipLaunchKernelGGL(call_prologue_kernel, dim3((std::max(std::max(n_state, pool_cap), n_touched) + 255u) / 256u), dim3(256), 0, st, b.call_state.get(), n_state,
                       b.chunk_fill.get(), b.chunk_key.get(), pool_cap, b.tile_touched.get(), n_touched);
}
// ---- 2. K0  (the two launches one after the other: both are bound by instruction issue, side by side on two streams they take
// exactly as long — measured, profiles/r03_k0side_ab.sh)
int a2a_decode(kmdb_db* db, BlocksState& b, hipStream_t st) {
    const uint32_t P = (uint32_t)db->P;
    K0Params q{};
    q.k0in = db->k0in; q.bitrel = db->bitrel; q.blkbase = db->blkbase; q.bits = db->bits; q.perm = nullptr; q.P = P;
    q.bm = BlockMap{db->width, (uint32_t)((1ull << 32) / db->width) + 1u};
    q.p0_mask = b.p0_mask; q.p0_info = b.p0_info; q.pair_ofs = b.pair_ofs; q.pair_blk = b.pair_blk; q.pair_mask = b.pair_mask;
    // sub-pools of the pair pool: enough of them that their cursors are not hot, few enough that one wave's need fits a share
    uint32_t nreg = 1;
    while (nreg < KMDB_PAIR_REGIONS && (uint64_t)nreg * 16384 < P) nreg <<= 1;
    // three quarters of the pool in sub-pools, the rest shared
    q.pair_cursor = b.pair_cursor; q.n_regions = nreg; q.region_cap = (uint32_t)(b.pair_cap * 3 / 4 / nreg);
    q.spill_cap = (uint32_t)(b.pair_cap - (uint64_t)q.region_cap * nreg); q.counters = b.counters;
    // the short launch: 256 ranks of a window per workgroup.  A window wider than that (reached through KMDB_K0_WINDOW alone: the default is 256) takes
    // several workgroups, and the grid is rounded up to whole groups of 8 windows: the kernel deals the windows to the 8 XCDs in turn
    q.order = db->k0_order; q.live = db->k0_live;
    q.win_shift = 8;
    while ((1u << q.win_shift) < db->k0_window) ++q.win_shift;
    const uint32_t wgs_per_win = db->k0_window >> 8;
    q.n_items = (uint32_t)((db->P + db->k0_window - 1) / db->k0_window) * wgs_per_win;
    const uint32_t grid = wgs_per_win > 1 ? (q.n_items + 8u * wgs_per_win - 1u) / (8u * wgs_per_win) * (8u * wgs_per_win) : q.n_items;
    if (grid) hipLaunchKernelGGL((k0_decode_kernel<false>), dim3(grid), dim3(256), 0, st, q);
    if (db->n_long) {
        q.perm = db->long_nodes; q.P = db->n_long;
        hipLaunchKernelGGL((k0_decode_kernel<true>), dim3((db->n_long + 255) / 256), dim3(256), 0, st, q);
    }
    HIP_TRY(hipGetLastError());
    return 0;
}
// ---- 3. K1n
int a2a_narrow_emit(kmdb_db* db, BlocksState& b, uint32_t* M, uint32_t emit_lo, uint32_t emit_hi, hipStream_t st) {
    NParams q{};
    q.nl = db->nl; q.parent = db->parent; q.w = db->w; q.dflag = db->dflag; q.seg_anc = db->nseg_anc; q.seg_anc_n = db->nseg_anc_n;
    q.p0_mask = b.p0_mask; q.p0_info = b.p0_info; q.pair_ofs = b.pair_ofs; q.pair_blk = b.pair_blk; q.pair_mask = b.pair_mask;
    q.fn_mask = b.fn_mask; q.fn_blk = b.fn_blk; q.widebits = b.widebits; q.wide_base = b.wide_base; q.wide_slice_cnt = b.wide_slice_cnt;
    q.P = (uint32_t)db->P; q.nseg_nodes = db->nseg_nodes; q.n_segs = db->n_nsegs; q.chain_cap = db->chain_cap;
    // (g_rows: the block rows the open-chunk table and the row tables are indexed by — all NB of them, or the band's under band emit)
    q.emit_lo = emit_lo; q.emit_hi = emit_hi; q.tbits = b.dense_narrow ? 0u : arena_table_bits(b.g_rows); q.n_keys = b.g_rows;
    q.all_wide = b.dense_narrow ? 1u : 0u;
    q.pool = pool_view(b, b.dense_narrow);
    q.band_xlo = b.g_xlo; q.band_xhi = b.g_xhi; q.band_sbase = b.g_sbase;
    // a wave's chain table grows with the depth of the tree: as many waves per workgroup as 144 KB of LDS hold
    const size_t wave_lds = k1n_wave_bytes(q.chain_cap, q.tbits, q.n_keys, b.row_mode ? b.g_rows : 0u);
    const uint32_t waves = (uint32_t)std::max<size_t>(1, std::min<size_t>(K1N_WAVES, (144u << 10) / wave_lds));
    const size_t lds = wave_lds * waves;
    q.M = M; q.N = (uint32_t)db->N; q.bwidth = db->width; q.touched = touched_view(b); q.direct_ctr = b.direct_ctr;
    q.dmask = b.dmask; q.dwx = b.dwx; q.slice_cnt = b.slice_cnt;
    // (mode 1 holds 48 accumulator registers beside the narrow kernel's 95: three waves per SIMD without spills, or four with 72 bytes of
    // scratch per lane, 76 in row mode — KMDB_K1N_MINW=4, A/B)
    // the instantiation of the call's record path: the attribute and the launch take the same function
    const K1nPick pick = b.emit_band ? k1n_band_pick(b.k1n_mode, b.row_mode) : k1n_pick(b.k1n_mode, b.knobs.k1n_minw, b.row_mode);
    HIP_TRY(hipFuncSetAttribute((const void*)pick.fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    const dim3 grid((q.n_segs + waves - 1) / waves), block(WAVE * waves);
    if (!b.have_counts && kmdb_verbose())
        fprintf(stderr, "[kmdb] narrow kernel: %u slices, %zu B of LDS per wave, %u per workgroup, instantiation %s\n", q.n_segs, wave_lds, waves, pick.name);
    hipLaunchKernelGGL(pick.fn, grid, block, lds, st, q);
    HIP_TRY(hipGetLastError());
    return 0;
}
// ---- 4. mode 2: the slices' first-block records through k2d_kernel, on the side stream beside the wide kernel
// (It starts right behind the narrow kernel, beside the wide list's small kernels — scan, expand, root paths of the runs, which then take
// 0.28 ms at C2 instead of their own 0.05.  KMDB_K2D_EARLY=0 starts it with the wide kernel: the wide stage gains 0.1 ms, the sort beside which
// the kernel then ends loses them — profiles/r06_j13: 6.70 / 6.98 against 6.86 / 6.93 ms at C2, 18.45 against 19.11 at 10 000 samples)
int a2a_slice_apply(kmdb_db* db, BlocksState& b, uint32_t* M, hipStream_t st, hipStream_t s2) {
    HIP_TRY(hipEventRecord(db->ev_side[0], st));
    HIP_TRY(hipStreamWaitEvent(s2, db->ev_side[0], 0));
    DParams d{};
    d.dmask = b.dmask; d.dwx = b.dwx; d.slice_cnt = b.slice_cnt; d.n_segs = db->n_nsegs; d.nseg_nodes = db->nseg_nodes;
    const uint32_t sl = b.knobs.k2d_slices;
    d.slices = sl; d.M = M; d.N = (uint32_t)db->N; d.bwidth = db->width; d.touched = touched_view(b);
    const uint32_t waves = (db->n_nsegs + sl - 1u) / sl;
    if (waves) {
        if (b.band_on) hipLaunchKernelGGL(k2d_band_kernel, dim3((waves + 3u) / 4u), dim3(256), 0, s2, d, BandArg<true>{b.band});
        else hipLaunchKernelGGL(k2d_kernel, dim3((waves + 3u) / 4u), dim3(256), 0, s2, d);
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(db->ev_side[1], s2));               // (the call's end waits for the side stream; many streams: recorded again behind the chunk table's work)
    (void)stage_done(s2, "slice apply");
    return 0;
}
// ---- 5. The chunk table grouped by key (on stream `cs`), then on the side stream the stream chunks applied.  Few streams: right behind the
// narrow kernel, next to the wide kernel (which writes no chunks).  Many streams: after the wide kernel (it writes the row chunks), next to
// the sort inside the rows.
int a2a_group_and_apply_chunks(kmdb_db* db, BlocksState& b, uint32_t* M, hipStream_t cs, hipStream_t s2) {
    const uint32_t pool_cap = (uint32_t)b.pool_cap;
    hipLaunchKernelGGL(ct_hist_kernel, dim3((pool_cap + CT_THREADS - 1) / CT_THREADS), dim3(CT_THREADS), 0, cs, b.chunk_key, pool_cap, b.n_states, b.ct_hist);
    size_t tb = b.ct_tmp_bytes;
    HIP_TRY(prim::exclusive_sum(b.ct_tmp, tb, b.ct_hist, b.ct_offs.get(), (int)(b.n_states + 1), cs));
    HIP_TRY(hipMemcpyAsync(b.ct_cursor, b.ct_offs, ((size_t)b.n_states + 1) * 4, hipMemcpyDeviceToDevice, cs));
    hipLaunchKernelGGL(ct_scatter_kernel, dim3((pool_cap + CT_THREADS - 1) / CT_THREADS), dim3(CT_THREADS), 0, cs, b.chunk_key, pool_cap, b.n_states, b.ct_cursor, b.sorted_key, b.sorted_id);
    hipLaunchKernelGGL(ct_count_kernel, dim3(1), dim3(1), 0, cs, b.ct_offs, b.n_states, b.counters);
    if (cs != s2) { HIP_TRY(hipEventRecord(db->ev_side[0], cs)); HIP_TRY(hipStreamWaitEvent(s2, db->ev_side[0], 0)); }
    {
        rocprim::transform_iterator<uint32_t*, U32toU64, unsigned long long> it(b.chunk_fill, U32toU64());
        HIP_TRY(prim::sum(b.sort_tmp, b.sort_tmp_bytes, it, (unsigned long long*)(b.counters + KCTR_RECORDS), (int)pool_cap, s2));
    }
    const uint32_t win = b.n_states <= CS_MAX_KEYS ? 16u : 32u;      // (8 / 32 / 64 chunks at few streams: within the boxes' noise, profiles/r05_j5)
    uint32_t grid = (pool_cap + win - 1) / win;
    if (b.have_counts) grid = std::min(grid, (b.last_n_chunks + win - 1) / win);
    if (grid) {
        if (b.band_on)
            hipLaunchKernelGGL(k2_apply_kernel<true>, dim3(grid), dim3(256), 0, s2, b.rec, b.recw, b.sorted_key, b.sorted_id, b.chunk_fill, b.n_states,
                               b.ct_offs + b.n_states, M, (uint32_t)db->N, db->width, win, touched_view(b), BandArg<true>{b.band});
        else
            hipLaunchKernelGGL(k2_apply_kernel<false>, dim3(grid), dim3(256), 0, s2, b.rec, b.recw, b.sorted_key, b.sorted_id, b.chunk_fill, b.n_states,
                               b.ct_offs + b.n_states, M, (uint32_t)db->N, db->width, win, touched_view(b), BandArg<false>{});
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(db->ev_side[1], s2));
    (void)stage_done(s2, "chunk apply");
    return 0;
}
// ---- 6. wide list: the flagged nodes, compacted.  The narrow kernel counted them per word and slice: one workgroup scans the slices' totals, no
// device-wide scan.  A handle's first call (or one whose list outgrew its arrays) waits for the device here and reads the number of wide nodes, as
// the few-streams sort of such a call reads the chunks in use; later calls take the previous call's counts (checked at the end of the call).
int a2a_wide_list(kmdb_db* db, BlocksState& b, hipStream_t st, uint32_t* n_wide_out) {
    const uint32_t n_words = ((uint32_t)db->P + 63) / 64;
    hipLaunchKernelGGL(wide_slices_kernel, dim3(1), dim3(WSL_THREADS), 0, st, b.wide_slice_cnt.get(), db->n_nsegs, b.wide_slice_base.get(), b.wide_base.get(), n_words,
                       b.counters);
    uint32_t n_wide;
    if (b.have_counts && b.wide_cap >= b.last_n_wide) n_wide = b.last_n_wide;
    else {
        HIP_TRY(hipMemcpyAsync(b.h_counters, b.counters + KCTR_NWIDE, 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        n_wide = b.h_counters[0];
        if (n_wide > b.wide_cap) {
            dev_reset(b.widx, b.wrun_anc, b.wrun_anc_n);
            b.wide_cap = 0;
            DEV_ALLOC(b.widx, (size_t)n_wide);
            DEV_ALLOC(b.wrun_anc, ((size_t)n_wide / 64 + 1) * db->chain_cap);
            DEV_ALLOC(b.wrun_anc_n, (size_t)n_wide / 64 + 1);
            b.wide_cap = n_wide;
        }
    }
    if (!b.widx) { DEV_ALLOC(b.widx, 1); b.wide_cap = std::max<uint64_t>(b.wide_cap, 1); }
    const uint32_t wps = db->nseg_nodes / 64u;
    hipLaunchKernelGGL(wide_expand_kernel, dim3((n_words + 255) / 256), dim3(256), 0, st, b.widebits.get(), b.wide_base.get(),
                       b.wide_slice_base.get(), wps, (wps & (wps - 1u)) ? 0xFFFFFFFFu : (uint32_t)__builtin_ctz(wps), n_words, b.widx.get(), (uint32_t)b.wide_cap);
    *n_wide_out = n_wide;
    return 0;
}
// ---- 7. K1w, and behind it the second level (BlocksState::l2_on)
int a2a_wide_emit(kmdb_db* db, BlocksState& b, uint32_t* M, uint32_t emit_lo, uint32_t emit_hi, uint32_t n_wide, hipStream_t st) {
    WParams q{};
    q.widx = b.widx; q.n_wide = n_wide; q.nl = db->nl; q.parent = db->parent; q.w = db->w; q.widebits = b.widebits;
    q.dflag = db->dflag; q.wide_base = b.wide_base;
    q.p0_mask = b.p0_mask; q.p0_info = b.p0_info; q.pair_ofs = b.pair_ofs; q.pair_blk = b.pair_blk; q.pair_mask = b.pair_mask;
    q.fn_mask = b.fn_mask; q.fn_blk = b.fn_blk; q.emit_lo = emit_lo; q.emit_hi = emit_hi; q.pool = pool_view(b, true);
    if (b.l2_on && !b.l2_bitmap) {
        // a first guess from the wide list (at 10 000 samples 2 % of the wide nodes have 24 blocks or more); a call that runs out doubles both
        // (KMDB_POOL_PERCENT, tests: the smallest arrays there are, so that the doubling path runs)
        const bool tiny = b.knobs.pool_percent != 0;
        if (alloc_l2(b, tiny ? 1u : std::max<uint32_t>(64u * L2_SUB * 4u, n_wide / 16u), tiny ? 1u : std::max<uint32_t>(L2_ENT_GRAB * L2_SUB * 4u, n_wide / 16u * 48u))) return 1;
    }
    q.l2 = L2View{};
    if (b.l2_on) {
        q.l2.on = 1u; q.l2.min_blocks = b.l2_min_blocks; q.l2.node_cap = b.l2_node_cap; q.l2.W = b.l2_node_cap / 64u; q.l2.ent_cap = b.l2_ent_cap;
        q.l2.cursors = b.l2_cursors; q.l2.bitmap = b.l2_bitmap; q.l2.ent_g = b.l2_ent_g; q.l2.ent_blk = b.l2_ent_blk; q.l2.ent_mask = b.l2_ent_mask;
        q.l2.node_w = b.l2_node_w;
        HIP_TRY(hipMemsetAsync(b.l2_cursors, 0, 2 * L2_SUB * 16 * 4, st));
        HIP_TRY(hipMemsetAsync(b.l2_bitmap, 0, (size_t)b.NB * q.l2.W * 8, st));
        HIP_TRY(hipMemsetAsync(b.l2_ent_blk, 0xFF, (size_t)b.l2_ent_cap * 2, st));
    }
    q.run_nodes = b.knobs.k1w_run;
    q.n_runs = (n_wide + q.run_nodes - 1) / q.run_nodes;
    // root paths of the runs' first nodes (the table is sized with the wide list, for runs of 64 nodes at least)
    hipLaunchKernelGGL(wrun_anc_kernel, dim3((q.n_runs + 63) / 64), dim3(64), 0, st, b.widx, n_wide, q.run_nodes, db->parent, db->dflag, db->chain_cap,
                       b.wrun_anc, b.wrun_anc_n);
    q.seg_anc = b.wrun_anc; q.seg_anc_n = b.wrun_anc_n;
    // LDS of a wave: rows of a batch (at least one full list: as many entries as there are blocks), the chain list, the chain
    q.chain_cap = db->chain_cap; q.e_cap = (b.NB + 2u + 3u) & ~3u; q.arena_cap = std::max<uint32_t>(K1W_ARENA_MIN, (b.NB + 2u + 63u) & ~63u);
    q.n_rows = b.row_mode ? b.g_rows : 0u;
    q.band_xlo = b.g_xlo; q.band_xhi = b.g_xhi; q.band_sbase = b.g_sbase;
    const size_t wave_lds = k1w_wave_bytes(q.arena_cap, q.e_cap, q.chain_cap, q.n_rows);
    const uint32_t waves = wave_lds * K1W_WAVES <= (size_t)(64u << 10) ? (uint32_t)K1W_WAVES : 1u;
    // the instantiation of the call's record path: the attribute, the occupancy query and the launch take the same function
    const K1wPick pick = b.emit_band ? k1w_band_pick(b.row_mode, b.l2_on) : k1w_pick(b.row_mode, b.l2_on);
    HIP_TRY(hipFuncSetAttribute((const void*)pick.fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(wave_lds * waves)));
    // As many waves as the chip holds at once, each with an equal share of the runs (dealt round-robin): with more, the waves
    // beyond the first round start when the first ones end, and all take equally long — 1.6 rounds cost 2 (measured at 10 000
    // samples: 4096 waves at 10 per CU took 8.8 ms, of which every wave ran 4.4).
    // (the count is kept on the handle: its instantiation and its LDS do not change between the calls)
    if (!b.k1w_slots) {
        int per_cu = 0, dev = 0;
        hipDeviceProp_t prop;
        HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, (const void*)pick.fn, (int)(WAVE * waves), wave_lds * waves));
        HIP_TRY(hipGetDevice(&dev));
        HIP_TRY(hipGetDeviceProperties(&prop, dev));
        b.k1w_slots = (uint32_t)std::max(1, per_cu) * waves * (uint32_t)std::max(1, prop.multiProcessorCount);
    }
    q.n_waves = std::min<uint32_t>(std::min<uint32_t>(b.k1w_slots, b.k1w_waves), q.n_runs);
    q.run_ctr = b.run_ctr;
    if (b.knobs.k1w_waves) q.n_waves = std::max<uint32_t>(1u, std::min<uint32_t>(std::min<uint32_t>(b.k1w_waves, q.n_runs), b.knobs.k1w_waves));
    if (!b.have_counts && kmdb_verbose())
        fprintf(stderr, "[kmdb] wide kernel: %u wide nodes in %u runs, %u waves (%u fit the chip, %zu B of LDS per wave, %u per workgroup), instantiation %s\n", n_wide,
                q.n_runs, q.n_waves, b.k1w_slots, wave_lds, waves, pick.name);
    hipLaunchKernelGGL(pick.fn, dim3((q.n_waves + waves - 1) / waves), dim3(WAVE * waves), wave_lds * waves, st, q);
    if (b.l2_on) {
        // rank directories, list offsets, lists, and the tile joins adding into M (a tile whose blocks have no list leaves at once)
        const uint32_t NB = b.NB, W = b.l2_node_cap / 64u;
        hipLaunchKernelGGL(l2_ranks_kernel, dim3(NB), dim3(256), 0, st, b.l2_bitmap, W, b.l2_rank, b.l2_len);
        hipLaunchKernelGGL(l2_offsets_kernel, dim3(1), dim3(64), 0, st, b.l2_len, NB, b.l2_cursors, W, b.l2_loff);
        hipLaunchKernelGGL(l2_lists_kernel, dim3((b.l2_ent_cap + 255u) / 256u), dim3(256), 0, st, b.l2_ent_g, b.l2_ent_blk, b.l2_ent_mask, b.l2_node_w,
                           b.l2_ent_cap, W, b.l2_bitmap, b.l2_rank, b.l2_loff, b.l2_list_mask, b.l2_list_w, b.l2_cursors);
        // (the tiles: every block pair, or — band emit — the band's streams alone, counted from its first: BandWin::sbase)
        if (b.band_on)
            hipLaunchKernelGGL(l2_join_apply_kernel<true>, dim3(b.emit_band ? b.n_states : NB * (NB + 1u) / 2u), dim3(64 * L2_WAVES), 0, st, b.l2_bitmap, b.l2_rank, b.l2_list_mask,
                               b.l2_list_w, b.l2_loff, W, NB, M, (uint32_t)db->N, db->width, touched_view(b), BandArg<true>{b.band});
        else
            hipLaunchKernelGGL(l2_join_apply_kernel<false>, dim3(NB * (NB + 1u) / 2u), dim3(64 * L2_WAVES), 0, st, b.l2_bitmap, b.l2_rank, b.l2_list_mask, b.l2_list_w,
                               b.l2_loff, W, NB, M, (uint32_t)db->N, db->width, touched_view(b), BandArg<false>{});
    }
    return 0;
}
// the sorted records applied stream by stream (a long stream in parts of K2J_REC records): one write-back of a tile per job.  k2j_start holds where
// the streams start (from the sort's offsets: no run boundaries searched, no key word read for packed records)
void a2a_apply_stream_jobs(kmdb_db* db, BlocksState& b, uint32_t* M, hipStream_t st, Launched& L) {
    hipLaunchKernelGGL(k2j_build_kernel, dim3((b.n_states + 1023u) / 1024u), dim3(1024), 0, st, b.k2j_start, b.n_states, b.k2j_jobs, (uint32_t)b.k2j_cap, b.counters);
    L.k2jobs = b.have_counts ? b.last_n_k2jobs : (uint32_t)b.k2j_cap;       // (the streams' lengths repeat exactly from call to call)
    if (L.k2jobs) {
        if (b.band_on)
            hipLaunchKernelGGL(k2_jobs_kernel<true>, dim3(L.k2jobs), dim3(256), 0, st, b.swkey, (const WideRec*)b.swrec, b.k2j_start, b.k2j_jobs, b.counters + KCTR_K2JOBS,
                               (uint32_t)b.k2j_cap, (uint32_t)b.sorted_cap, b.rec_pshift, (uint32_t)b.key_bits, state_digit_bits(b), M, (uint32_t)db->N, db->width,
                               touched_view(b), BandArg<true>{b.band});
        else
            hipLaunchKernelGGL(k2_jobs_kernel<false>, dim3(L.k2jobs), dim3(256), 0, st, b.swkey, (const WideRec*)b.swrec, b.k2j_start, b.k2j_jobs, b.counters + KCTR_K2JOBS,
                               (uint32_t)b.k2j_cap, (uint32_t)b.sorted_cap, b.rec_pshift, (uint32_t)b.key_bits, state_digit_bits(b), M, (uint32_t)db->N, db->width,
                               touched_view(b), BandArg<false>{});
    }
}
// ---- 8. many streams: chunk table grouped (stream chunks -> side stream), then the sort inside the block rows and its apply
int a2a_sort_apply_rows(kmdb_db* db, BlocksState& b, uint32_t* M, hipStream_t st, hipStream_t s2, Launched& L) {
    if (a2a_group_and_apply_chunks(db, b, M, st, s2)) return 1;
    // (NB: the block rows of the tables — all of them, or the band's under band emit; bins: the streams of the last of them)
    const uint32_t NB = b.g_rows, bins = b.g_bins, pool_cap = (uint32_t)b.pool_cap, kmask = (1u << b.key_bits) - 1u;
    uint32_t* row_job = b.rs_rows, *row_tab = b.rs_rows + (NB + 1);
    {
        // the row chunks grouped by row
        const size_t rg_ne = (size_t)NB * b.rg_blocks + 1;
        hipLaunchKernelGGL(rg_hist_kernel, dim3(b.rg_blocks), dim3(RG_THREADS), NB * 4, st, b.chunk_key, pool_cap, b.n_states, NB, b.rg_hist);
        size_t tbg = b.rg_tmp_bytes;
        HIP_TRY(prim::exclusive_sum(b.rg_tmp, tbg, b.rg_hist.get(), b.rg_offs.get(), (int)rg_ne, st));
        hipLaunchKernelGGL(rg_scatter_kernel, dim3(b.rg_blocks), dim3(RG_THREADS), NB * 4, st, b.chunk_key, pool_cap, b.n_states, NB, b.rg_offs, b.row_ids);
    }
    if (b.emit_band) hipLaunchKernelGGL(rs_rows_band_kernel, dim3(1), dim3(1024), 0, st, b.rg_offs, b.rg_blocks, NB, row_job, row_tab, b.counters, b.g_xlo);
    else hipLaunchKernelGGL(rs_rows_kernel, dim3(1), dim3(1024), 0, st, b.rg_offs, b.rg_blocks, NB, row_job, row_tab, b.counters);
    const RsRows R{b.rg_offs, b.row_ids, b.rg_blocks, NB, row_job, row_tab, b.g_xlo, b.g_sbase, bins};
    // jobs and table entries: measured by the previous call, else their upper bounds (workgroups beyond the last job leave at once)
    const uint32_t jobs_bound = (uint32_t)(pool_cap / RS_JOB_CHUNKS + NB + 1);
    const uint32_t jobs = b.have_counts ? std::min<uint32_t>(jobs_bound, with_slack(b.last_n_rowjobs)) : jobs_bound;
    L.rowjobs = jobs;
    const size_t ne = std::min<size_t>(b.rs_entries, (size_t)jobs * bins + 1);
    HIP_TRY(hipMemsetAsync(b.rs_hist, 0, ne * 4, st));
    // (16 chunks' key words requested together; 4, round 4's, and 8 at 10 000 samples: apply step 6.08 / 5.88 against 5.85 ms, profiles/r05_j14 — the
    // kernel waits for its loads)
    hipLaunchKernelGGL(rs_hist_kernel<16>, dim3(jobs), dim3(256), bins * 4, st, R, b.chunk_fill, b.recw, kmask, b.rs_hist);
    size_t tb = b.rs_tmp_bytes;
    HIP_TRY(prim::exclusive_sum(b.rs_tmp, tb, b.rs_hist.get(), b.rs_offs.get(), (int)ne, st));
    const uint32_t* total_ptr = b.rs_offs + (ne - 1);
    HIP_TRY(hipMemcpyAsync(b.counters + KCTR_WIDE_RECORDS, total_ptr, 4, hipMemcpyDeviceToDevice, st));
    // (Sorting and applying bands of block rows side by side on two streams was measured at 10 000 samples: 2 / 4 / 8 bands 18.4 / 17.0 /
    // 18.7 ms against 16.5 for one — the two kernels do not complement each other.)
    HIP_TRY(hipFuncSetAttribute((const void*)rs_scatter_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)rs_scatter_lds(bins, b.rec_pshift != 0)));
    hipLaunchKernelGGL(rs_scatter_kernel, dim3((jobs + 7u) & ~7u), dim3(CS_THREADS), rs_scatter_lds(bins, b.rec_pshift != 0), st, R, b.chunk_fill, b.recw, (const WideRec*)b.rec.get(), kmask,
                       b.rs_offs, (uint32_t)b.sorted_cap, b.swkey, (WideRec*)b.swrec, b.counters, b.rec_pshift ? 1u : 0u);
    if (b.emit_band) hipLaunchKernelGGL(k2j_starts_band_kernel, dim3((b.n_states + 1u + 255u) / 256u), dim3(256), 0, st, R, b.rs_offs, b.n_states, b.k2j_start);
    else hipLaunchKernelGGL(k2j_starts_kernel, dim3((b.n_states + 1u + 255u) / 256u), dim3(256), 0, st, R, b.rs_offs, b.n_states, b.k2j_start);
    a2a_apply_stream_jobs(db, b, M, st, L);
    HIP_TRY(hipGetLastError());
    return 0;
}
// ---- 9. few streams: the wide pool sorted by stream in one counting-sort pass (the sort moves the 16-byte records, with their key words unless
// they are packed), then applied stream by stream as on the many-streams path
int a2a_sort_apply_flat(kmdb_db* db, BlocksState& b, uint32_t* M, hipStream_t st, Launched& L) {
    hipLaunchKernelGGL(count_raw_kernel, dim3(1), dim3(64), 0, st, b.wsub_cursor, (uint32_t)(b.wide_pool_cap / KMDB_SUBPOOLS), b.counters, b.wide_handed.get());
    uint32_t n_raw;
    if (b.have_counts) n_raw = L.raw;
    else {
        HIP_TRY(hipMemcpyAsync(b.h_counters, b.counters, KCTR_COUNT * 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        n_raw = std::min<uint32_t>(b.h_counters[KCTR_RAW], (uint32_t)b.wide_pool_cap);
    }
    if (!n_raw) return 0;
    const uint32_t nslots = (uint32_t)((uint64_t)n_raw << WCH_SHIFT), kmask = (1u << b.key_bits) - 1u;
    const size_t ne = (size_t)b.n_states * CS_BLOCKS_ONE + 1;
    hipLaunchKernelGGL(cs_hist_kernel, dim3(CS_BLOCKS_ONE), dim3(256), b.n_states * 4, st, b.wkey, nslots, b.n_states, b.n_states, kmask, b.cs_hist, b.wide_handed.get());
    size_t tb = b.cs_tmp_bytes;
    HIP_TRY(prim::exclusive_sum(b.cs_tmp, tb, b.cs_hist.get(), b.cs_offs.get(), (int)ne, st));
    const bool packed = b.rec_pshift != 0;
    HIP_TRY(hipFuncSetAttribute((const void*)cs_scatter_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)cs_scatter_lds(b.n_states, packed)));
    hipLaunchKernelGGL(cs_scatter_kernel, dim3(CS_BLOCKS_ONE), dim3(CS_THREADS), cs_scatter_lds(b.n_states, packed), st, b.wkey, (const WideRec*)b.wrec, nslots,
                       b.n_states, b.n_states, kmask, b.cs_offs, b.swkey, (WideRec*)b.swrec, packed ? 1u : 0u, b.wide_handed.get());
    const uint32_t* total_ptr = b.cs_offs + (ne - 1);
    HIP_TRY(hipMemcpyAsync(b.counters + KCTR_WIDE_RECORDS, total_ptr, 4, hipMemcpyDeviceToDevice, st));
    hipLaunchKernelGGL(k2j_starts_flat_kernel, dim3((b.n_states + 1u + 255u) / 256u), dim3(256), 0, st, b.cs_offs, b.n_states, CS_BLOCKS_ONE, b.k2j_start);
    a2a_apply_stream_jobs(db, b, M, st, L);
    HIP_TRY(hipGetLastError());
    return 0;
}
// a pool ran over (results invalid): it is enlarged — or, at the limit of what a pool can index, the call takes more slices of the pattern stream —
// and the call repeated.  Leaves b.gave_up when neither is possible.
int a2a_enlarge_pools(kmdb_db* db, BlocksState& b, const uint32_t* c) {
    const bool verbose = kmdb_verbose();
    if (c[KCTR_PAIR_OVERFLOW]) {
        if (verbose) fprintf(stderr, "[kmdb] pair pool too small (%llu entries): doubling\n", (unsigned long long)b.pair_cap);
        if (alloc_pair_pool(b, b.pair_cap * 2)) return 1;
    }
    if (c[KCTR_WIDE_OVERFLOW]) {
        const uint64_t want = b.wide_pool_cap * 2;
        if ((want << WCH_SHIFT) >= pool_slot_limit(b)) {
            if (b.n_slices >= (1u << 16)) { b.gave_up = "more block records than a pool can index from the nodes with many blocks in a 65536th of the patterns"; return 0; }
            b.n_slices *= 2;                                  // the pools stay as they are: half as many patterns per pass
            if (verbose) fprintf(stderr, "[kmdb] wide record pool at its limit: %u slices of the pattern stream per call\n", b.n_slices);
            return 0;
        }
        if (verbose) fprintf(stderr, "[kmdb] wide record pool too small (%llu chunks): doubling\n", (unsigned long long)b.wide_pool_cap);
        if (alloc_wide_pool(b, db->stream, want)) return 1;
    }
    if (c[KCTR_POOL_OVERFLOW]) {
        uint64_t want = b.pool_cap * 2;
        if (!b.row_mode && !b.dense_narrow && b.n_states > (1u << ST_MAX_BITS) && (b.pool_cap << CH_SHIFT) > 8 * (b.est_records + (1u << 22))) {
            // the estimate is long covered: the narrow kernel's chunks are being evicted nearly empty.  Wide pool for it as well.
            b.dense_narrow = true;
            if (verbose) fprintf(stderr, "[kmdb] record chunks of the narrow kernel are evicted nearly empty: its records go through the sort too\n");
            if (alloc_wide_pool(b, db->stream, b.wide_pool_cap + b.est_records * 5 / 4 / WCH_REC + (uint64_t)db->n_nsegs * (WIDE_GRAB + 2))) return 1;
            want = 0;
        } else if (b.row_mode && !b.dense_narrow && b.g_rows > (1u << ST_MAX_BITS) && (b.pool_cap << CH_SHIFT) > 8 * (b.est_records + (1u << 22))) {
            // the same with row chunks: the diagonal records join the rows
            b.dense_narrow = true;
            if (verbose) fprintf(stderr, "[kmdb] record chunks of the narrow kernel are evicted nearly empty: its records go through the row chunks too\n");
            if (alloc_wide_pool(b, db->stream, b.wide_pool_cap + b.est_records * 5 / 4 / WCH_REC)) return 1;
            want = 0;
        } else if ((want << CH_SHIFT) >= pool_slot_limit(b)) {
            if (b.n_slices >= (1u << 16)) {
                b.gave_up = "more block records than a pool can index in a 65536th of the patterns (" + std::to_string(b.n_states) + " streams, " + std::to_string(b.pool_cap) + " chunks were not enough)";
                return 0;
            }
            b.n_slices *= 2;
            if (verbose) fprintf(stderr, "[kmdb] record pool at its limit: %u slices of the pattern stream per call\n", b.n_slices);
            return 0;
        }
        if (want) {
            if (verbose) fprintf(stderr, "[kmdb] record pool too small (%llu chunks): %llu\n", (unsigned long long)b.pool_cap, (unsigned long long)want);
            if (alloc_record_pool(b, db->stream, want)) return 1;
        }
    }
    return 0;
}
// ---- 10. what the call found: the counters read back (the call's end), then — a pool or the second level ran over: enlarged (or more slices), retry;
// a launch sized too small: retry with upper bounds; headroom growth; what the next call remembers.  *retry: the attempt's results are invalid.
int a2a_settle(kmdb_db* db, BlocksState& b, hipStream_t st, const Launched& L, bool* retry) {
    const bool row_mode = b.row_mode;
    HIP_TRY(hipMemcpyAsync(b.h_counters, b.counters, KCTR_COUNT * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    const uint32_t* c = b.h_counters;
    if (c[KCTR_LIST_OVERFLOW] || c[KCTR_SLOW]) {
        b.gave_up = "internal: the wide-node kernel lost a list (chain miss " + std::to_string(c[KCTR_SLOW]) + ", arena overflow " + std::to_string(c[KCTR_LIST_OVERFLOW]) + ")";
        return 0;
    }
    if (c[KCTR_L2_OVERFLOW]) {
        if (kmdb_verbose()) fprintf(stderr, "[kmdb] second level out of node indices or entries (%u / %u): doubling\n", b.l2_node_cap, b.l2_ent_cap);
        if (alloc_l2(b, b.l2_node_cap * 2u, b.l2_ent_cap * 2u)) return 1;
        b.have_counts = false; *retry = true;
        return 0;
    }
    if (c[KCTR_PAIR_OVERFLOW] || c[KCTR_POOL_OVERFLOW] || c[KCTR_WIDE_OVERFLOW]) {
        if (a2a_enlarge_pools(db, b, c)) return 1;
        if (b.gave_up.empty()) { b.have_counts = false; *retry = true; }
        return 0;
    }
    if (b.have_counts && (c[KCTR_NWIDE] != b.last_n_wide || c[KCTR_CHUNKS] != b.last_n_chunks ||
                            (row_mode ? (c[KCTR_ROWJOBS] > L.rowjobs || c[KCTR_WIDE_RECORDS] != b.last_n_sorted || c[KCTR_K2JOBS] > L.k2jobs)
                                      : (c[KCTR_RAW] > L.raw || c[KCTR_K2JOBS] > L.k2jobs)))) {
        // the exact counts cannot differ for an unchanged database and emit range, and the varying ones stay inside their slack in
        // practice; if not: redo the call with upper bounds
        if (kmdb_verbose())
            fprintf(stderr, "[kmdb] a launch was sized too small (wide nodes %u / %u, chunks %u / %u, row jobs %u / %u, sorted %u / %u, apply jobs %u / %u, raw %u / %u): the call is repeated\n",
                    c[KCTR_NWIDE], b.last_n_wide, c[KCTR_CHUNKS], b.last_n_chunks, c[KCTR_ROWJOBS], L.rowjobs, c[KCTR_WIDE_RECORDS], b.last_n_sorted, c[KCTR_K2JOBS],
                    L.k2jobs, c[KCTR_RAW], L.raw);
        b.have_counts = false; *retry = true;
        return 0;
    }
    // Headroom: where the wide kernel's records land depends on which wave took which run, so a pool that was just large enough this time may
    // be too small next time (a warm call would then take the enlarge-and-repeat path: seen once in the tests with pools of 1 %).  A pool
    // more than 85 % in use grows by a quarter now, while nothing runs.
    if ((uint64_t)c[KCTR_POOL_USED] * 100 > b.pool_cap * 85) {
        if (kmdb_verbose()) fprintf(stderr, "[kmdb] record pool %u of %llu chunks in use: enlarged by a quarter\n", c[KCTR_POOL_USED], (unsigned long long)b.pool_cap);
        const uint64_t want = b.pool_cap + b.pool_cap / 4;
        if (((want + (uint64_t)KMDB_SUBPOOLS * ARENA_GRAB) << CH_SHIFT) < pool_slot_limit(b) && alloc_record_pool(b, db->stream, want)) return 1;
    }
    if (!row_mode && (uint64_t)c[KCTR_RAW] * 100 > b.wide_pool_cap * 85) {
        if (kmdb_verbose()) fprintf(stderr, "[kmdb] wide record pool %u of %llu chunks in use: enlarged by a quarter\n", c[KCTR_RAW], (unsigned long long)b.wide_pool_cap);
        const uint64_t want = b.wide_pool_cap + b.wide_pool_cap / 4;
        if (((want + (uint64_t)KMDB_SUBPOOLS * WIDE_GRAB) << WCH_SHIFT) < pool_slot_limit(b) && alloc_wide_pool(b, db->stream, want)) return 1;
    }
    if (!b.have_counts && kmdb_verbose())
        fprintf(stderr, "[kmdb] record pool: %u of %llu chunks in use (busiest sub-pool x sub-pools); wide pool / sorted arrays: %llu slots\n", c[KCTR_POOL_USED],
                (unsigned long long)b.pool_cap, (unsigned long long)b.sorted_cap);
    b.last_n_wide = c[KCTR_NWIDE]; b.last_n_chunks = c[KCTR_CHUNKS]; b.last_n_raw = c[KCTR_RAW];
    b.last_n_rowjobs = c[KCTR_ROWJOBS]; b.last_n_sorted = c[KCTR_WIDE_RECORDS]; b.last_l2_nodes = c[KCTR_L2_NODES]; b.last_n_k2jobs = c[KCTR_K2JOBS];
    if (b.l2_on && !b.have_counts && kmdb_verbose())
        fprintf(stderr, "[kmdb] second level: %u nodes with %u blocks or more joined per tile (indices for %u, entries for %u)\n", c[KCTR_L2_NODES], b.l2_min_blocks,
                b.l2_node_cap, b.l2_ent_cap);
    b.last_records = ((uint64_t)c[KCTR_RECORDS] | ((uint64_t)c[KCTR_RECORDS_HI] << 32)) + (row_mode ? 0u : c[KCTR_WIDE_RECORDS]);
    b.last_n_direct = c[KCTR_DIRECT];
    return 0;
}
// one attempt of the whole pipeline; *retry is set when a pool was too small (it has been enlarged)
// decode: run K0 (the first slice of a call does; what it leaves — the local (block, mask) pairs of every node — serves all slices)
// band (may be null): M holds that band of rows only — the emit stages run as ever, every apply launch takes its BAND instantiation
int blocks_attempt(kmdb_db* db, BlocksState& b, uint32_t* M, uint32_t emit_lo, uint32_t emit_hi, bool decode, hipStream_t st, bool* retry, const kmdb_band_desc* band) {
    hipStream_t s2 = db->stream2;
    *retry = false;
    b.band_on = band != nullptr;
    if (band) {
        // (row_lo < row_hi <= N: the caller's checks; an empty band never gets here.  sbase: 0 but for the band-emit state, whose keys count from its first stream)
        b.band = BandWin{(uint32_t)band->row_lo, (uint32_t)band->row_hi, (uint32_t)(band->row_lo / db->width), (uint32_t)((band->row_hi - 1) / db->width), band->cell_lo,
                         b.band_units.get(), b.g_sbase};
    }
    Launched L;
    if (b.have_counts) L.raw = (uint32_t)std::min<uint64_t>(with_slack(b.last_n_raw), b.row_mode ? 0xFFFFFFFFull : b.wide_pool_cap);
    a2a_prologue(b, st, decode);
    if (stage_done(st, "init")) return 1;
    if (decode && a2a_decode(db, b, st)) return 1;
    if (stage_done(st, "decode")) return 1;
    HIP_TRY(hipEventRecord(db->ev_k[0], st));
    if (a2a_narrow_emit(db, b, M, emit_lo, emit_hi, st)) return 1;
    if (stage_done(st, "narrow emit")) return 1;
    HIP_TRY(hipEventRecord(db->ev_k[1], st));
    if (b.k1n_mode == 2 && b.knobs.k2d_early && a2a_slice_apply(db, b, M, st, s2)) return 1;
    if (!b.row_mode) {
        if (!b.dense_narrow) {
            HIP_TRY(hipEventRecord(db->ev_side[0], st));
            HIP_TRY(hipStreamWaitEvent(s2, db->ev_side[0], 0));
            if (a2a_group_and_apply_chunks(db, b, M, s2, s2)) return 1;
        } else HIP_TRY(hipEventRecord(db->ev_side[1], s2));        // (no stream chunk is ever opened: nothing to group; the side stream holds the slices' apply kernel or nothing)
    }
    uint32_t n_wide = 0;
    if (a2a_wide_list(db, b, st, &n_wide)) return 1;
    if (b.k1n_mode == 2 && !b.knobs.k2d_early && a2a_slice_apply(db, b, M, st, s2)) return 1;
    if (n_wide && a2a_wide_emit(db, b, M, emit_lo, emit_hi, n_wide, st)) return 1;
    HIP_TRY(hipGetLastError());
    if (stage_done(st, "wide emit")) return 1;
    HIP_TRY(hipEventRecord(db->ev_k[2], st));
    if (b.row_mode ? a2a_sort_apply_rows(db, b, M, st, s2, L) : a2a_sort_apply_flat(db, b, M, st, L)) return 1;
    if (stage_done(st, b.row_mode ? "row sort+apply" : "sorted apply")) return 1;
    HIP_TRY(hipStreamWaitEvent(st, db->ev_side[1], 0));          // the side stream's tiles are in the matrix too
    hipLaunchKernelGGL(pool_used_kernel, dim3(1), dim3(64), 0, st, b.sub_cursor, b.direct_ctr, b.counters);
    HIP_TRY(hipEventRecord(db->ev_k[3], st));
    return a2a_settle(db, b, st, L, retry);
}

}  // namespace

// an attempt that fails half way may have work under way on the side streams: nothing of it may outlive the call (the caller frees M)
static void blocks_join_side_streams(kmdb_db* db) {
    if (db->stream2) (void)hipStreamSynchronize(db->stream2);
}

// the band call's unit counters, summed over their slots
static int blocks_read_band_units(BlocksState& b, hipStream_t st) {
    std::vector<uint32_t> h((size_t)BAND_UNIT_SLOTS * BAND_UNIT_WORDS);
    HIP_TRY(hipMemcpyAsync(h.data(), b.band_units, h.size() * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    uint64_t c[BU_COUNT] = {};
    for (uint32_t s = 0; s < BAND_UNIT_SLOTS; ++s) for (uint32_t k = 0; k < BU_COUNT; ++k) c[k] += h[(size_t)s * BAND_UNIT_WORDS + k];
    b.last_band_units = kmdb_blocks_band_units{c[BU_JOBS], c[BU_JOBS_RUN], c[BU_RUNS], c[BU_RUNS_RUN], c[BU_SLICES], c[BU_SLICES_RUN], c[BU_TILES], c[BU_TILES_RUN]};
    return 0;
}

int kmdb_blocks_run(kmdb_db* db, uint32_t* M, uint32_t emit_lo, uint32_t emit_hi, hipStream_t st, const kmdb_band_desc* band) {
    // band emit runs on the handle's second state (made and fitted to the band by kmdb_blocks_band_prepare); nothing of the whole-matrix state is touched,
    // the reason the handle may hold — why the whole matrix cannot go through the pipeline — included: an attempt that gives up says so on the state it
    // ran on (gave_up), and that is published to the reason of this call's form
    const bool emit = band && band->emit;
    BlocksState& b = emit ? *db->band_blocks : *db->blocks;
    b.gave_up.clear();
    if (emit) db->band_fallback_reason.clear();                     // (per call; the whole matrix's is empty, or its callers would not be here, and sticks)
    // what a repeated round zeroes: the words of M — the whole triangle, or the band's cells only
    const uint64_t cells = band ? band->cells : db->N * (db->N - 1) / 2;
    if (band && !b.band_units) DEV_ALLOC(b.band_units, (size_t)BAND_UNIT_SLOTS * BAND_UNIT_WORDS);
    struct BandOff { BlocksState& b; ~BandOff() { b.band_on = false; } } band_off{b};      // (the state never names a band beyond its call)
    b.attempts = 0;
    for (int round = 0; round < 64; ++round) {
        ++b.attempts;
        if (band) HIP_TRY(hipMemsetAsync(b.band_units, 0, (size_t)BAND_UNIT_SLOTS * BAND_UNIT_WORDS * 4, st));
        // (the tiles this call adds to, all its slices: tile_touched is cleared by the prologue of the round's first attempt, the one that decodes)
        // the slices of [emit_lo, emit_hi) one after the other, adding into the same matrix; a pass that had to enlarge a pool (or
        // asked for more slices) leaves a partial sum behind: everything again from a zeroed matrix
        const uint32_t S = std::max<uint32_t>(1u, b.n_slices);
        bool again = false;
        uint64_t records = 0, direct = 0;
        // the launch sizes a call measures belong to one emit range: kept per slice, so that a sliced database reaches the warm path too
        if (b.slice_counts.size() != S) b.slice_counts.assign(S, BlocksState::SliceCounts{});
        bool decoded = false;
        db->last_call_sized = false;
        for (uint32_t k = 0; k < S && !again; ++k) {
            const uint32_t lo = emit_lo + (uint32_t)((uint64_t)(emit_hi - emit_lo) * k / S), hi = emit_lo + (uint32_t)((uint64_t)(emit_hi - emit_lo) * (k + 1) / S);
            if (lo == hi) continue;
            BlocksState::SliceCounts& sc = b.slice_counts[k];
            b.have_counts = sc.valid && sc.lo == lo && sc.hi == hi;
            if (b.have_counts) { b.last_n_wide = sc.n_wide; b.last_n_chunks = sc.n_chunks; b.last_n_raw = sc.n_raw; b.last_n_rowjobs = sc.n_rowjobs; b.last_n_sorted = sc.n_sorted; b.last_n_k2jobs = sc.n_k2jobs; }
            if (!b.have_counts) db->last_call_sized = true;
            bool retry = false;
            if (blocks_attempt(db, b, M, lo, hi, !decoded, st, &retry, band)) { blocks_join_side_streams(db); return 1; }
            decoded = true;
            if (!b.gave_up.empty()) { (emit ? db->band_fallback_reason : db->fallback_reason) = b.gave_up; return 0; }
            if (retry) { again = true; for (auto& c : b.slice_counts) c.valid = false; }
            else {
                sc = BlocksState::SliceCounts{true, lo, hi, b.last_n_wide, b.last_n_chunks, b.last_n_raw, b.last_n_rowjobs, b.last_n_sorted, b.last_n_k2jobs};
                records += b.last_records;
                direct += b.last_n_direct;
            }
        }
        if (!again) {
            b.last_records = records; b.last_n_direct = direct; b.have_counts = true;
            return band ? blocks_read_band_units(b, st) : 0;
        }
        if (cells) HIP_TRY(hipMemsetAsync(M, 0, cells * 4, st));
    }
    return kmdb_set_error("kmdb_blocks_run: the record pools did not converge");
}

// ---- what the other translation units read of the last call (engine_state.h)
kmdb_blocks_counts kmdb_blocks_last_counts(const kmdb_db* db) {
    const BlocksState& b = *db->blocks;
    return kmdb_blocks_counts{b.last_records, b.last_n_direct, b.last_n_wide, b.last_n_chunks, b.l2_on ? b.last_l2_nodes : 0u};
}
const unsigned char* kmdb_blocks_tile_touched(const kmdb_db* db) { return db->blocks ? db->blocks->tile_touched.get() : nullptr; }
int kmdb_blocks_k1n_mode(const kmdb_db* db, bool band_state) {
    if (!band_state) return db->blocks ? db->blocks->k1n_mode : -1;
    return db->band_blocks ? db->band_blocks->knobs.k1n_mode : blocks_read_knobs().k1n_mode;
}

// ------------------------------------------------------------------------------------------
// band emit: the handle's second state (kmdb_db.band_blocks), keyed relative to the band
// ------------------------------------------------------------------------------------------

// Why band emit cannot take this band ("": it can).  The streams: relative keys must leave all-ones free in 22 bits of a key word (KMDB_BAND_MAX_STREAMS, a
// test switch, lowers the limit; values above 2^22 are clamped).  The bytes: a list of the wide kernel may have as many entries as the collection has blocks.
std::string kmdb_blocks_band_refusal(const kmdb_db* db, const kmdb_band_geometry* g) {
    const uint64_t cap = std::min<uint64_t>(1ull << 22, db->band_max_streams ? db->band_max_streams : 1ull << 22);      // (read once per handle: a2a_rows_records.hip)
    if (g->n_streams + 1 >= cap)
        return "the band's " + std::to_string(g->n_streams) + " streams (block rows " + std::to_string(g->x_lo) + " to " + std::to_string(g->x_hi) + " of width " +
               std::to_string(db->width) + ") reach the limit of " + std::to_string(cap) + " streams of a band";
    const uint32_t NB = (uint32_t)((db->N + db->width - 1) / db->width);
    if (NB >= BNONE) return "the collection's " + std::to_string(NB) + " blocks exceed the " + std::to_string(BNONE) + " a block index holds";
    const size_t bytes = k1w_wave_bytes(std::max<uint32_t>(K1W_ARENA_MIN, (NB + 2u + 63u) & ~63u), (NB + 2u + 3u) & ~3u, db->chain_cap, g->n_rows);
    if (bytes > (size_t)(152u << 10))
        return "the lists of the wide-node kernel need " + std::to_string(bytes) + " bytes of LDS per wave (" + std::to_string(NB) + " blocks, root paths of up to " +
               std::to_string(db->max_depth) + " nodes, " + std::to_string(g->n_rows) + " block rows in the band), beyond the " + std::to_string(152u << 10) + " bytes there are";
    return "";
}

// The band-emit state fitted to the band `g` (not refused: kmdb_blocks_band_refusal): made at the handle's first such call, made anew — what it held is
// released first — when a band needs more streams, block rows or bins than it was made for or takes the other record path (the path follows the BAND's streams
// against CS_MAX_KEYS; KMDB_ROW_MODE forces it).  Its pools follow the whole matrix's sampled estimate scaled to the band's share of the cells.
int kmdb_blocks_band_prepare(kmdb_db* db, const kmdb_band_geometry* g, uint64_t band_cells) {
    const uint32_t n_streams = (uint32_t)g->n_streams, n_rows = g->n_rows, bins = g->x_hi + 1u;
    BlocksState* old = db->band_blocks.get();
    const BlocksKnobs knobs = old ? old->knobs : blocks_read_knobs();
    if (knobs.k1n_mode == 1) return kmdb_set_error("kmdb_blocks_band_prepare: KMDB_K1N_MODE=1 has no band form");
    bool row_mode = n_streams > CS_MAX_KEYS;
    if (knobs.row_mode >= 0) row_mode = knobs.row_mode != 0;
    // (KMDB_ROW_MODE=0 is followed as far as the one-pass sort's LDS — 160 KB, 1 KB of them the kernel's own — holds a cursor per stream of the band:
    // some 10 000 streams of packed records, 9 400 of unpacked ones; beyond that the band takes the many-streams path whatever the switch says)
    const bool packed = db->width <= 54u && knobs.rec_packed;
    if (!row_mode && cs_scatter_lds(n_streams, packed) + 1024u > (size_t)(160u << 10)) row_mode = true;
    const bool fits = old && old->row_mode == row_mode && n_streams <= old->cap_states && n_rows <= old->cap_rows && bins <= old->cap_bins;
    if (!fits) {
        // A state that is outgrown doubles the streams and the bins it held, up to what the whole collection has: the bands of a run walked top-down each need more streams than
        // the one before, and a state made anew per band would free and allocate the per-node arrays and the pools every time.  (Few streams: the sort's
        // tables are [streams][3072 workgroups], so the capacity stays at what its LDS can hold.)
        const uint32_t NB_all = (uint32_t)((db->N + db->width - 1) / db->width);
        const uint64_t whole_states = std::min<uint64_t>((uint64_t)NB_all * (NB_all + 1) / 2, (1ull << 22) - 2);
        uint64_t grow_states = old ? std::min<uint64_t>(2ull * old->cap_states, whole_states) : 0;
        if (!row_mode) grow_states = std::min<uint64_t>(grow_states, 8192);
        const uint32_t cap_states = (uint32_t)std::max<uint64_t>(n_streams, grow_states),
                       cap_rows = std::max(n_rows, old ? old->cap_rows : 0u),          // (the pools hold an open chunk per row and wave: rows are not doubled)
                       cap_bins = std::max(bins, old ? std::min(2u * old->cap_bins, NB_all) : 0u);
        if (old && kmdb_verbose())
            fprintf(stderr, "[kmdb] band emit: the band state is made anew for %u streams, %u block rows (it held %u, %u)\n", cap_states, cap_rows, old->cap_states, old->cap_rows);
        db->band_blocks.reset();
        std::unique_ptr<BlocksState, BlocksStateDelete> nb(new BlocksState());
        BlocksState& b = *nb;
        b.knobs = knobs;
        b.emit_band = true;
        b.forced_row_mode = row_mode ? 1 : 0;
        b.NB = (uint32_t)((db->N + db->width - 1) / db->width);
        b.n_states = n_streams; b.cap_states = cap_states; b.cap_rows = cap_rows; b.cap_bins = cap_bins;
        b.g_rows = n_rows; b.g_bins = bins; b.g_xlo = g->x_lo; b.g_xhi = g->x_hi; b.g_sbase = (uint32_t)g->stream_base;
        // the band's share of the whole matrix's sampled estimate (a block row's records go with its cells, roughly; too small is enlarged as ever)
        const BlocksState* w = db->blocks.get();
        const uint64_t total = db->N * (db->N - 1) / 2;
        const double frac = total ? std::min(1.0, (double)band_cells / (double)total) : 1.0;
        const uint64_t est_n = w ? (uint64_t)((double)w->est_n0 * frac) + 1 : 1, est_g = w ? (uint64_t)((double)w->est_g0 * frac) + 1 : 1,
                       est_l2 = w ? (uint64_t)((double)w->est_l20 * frac) : 0;
        b.est_records = est_n + est_g;
        b.est_n0 = est_n; b.est_g0 = est_g; b.est_l20 = est_l2; b.est_stride = w ? w->est_stride : 1u;
        if (blocks_alloc_working_set(db, b, est_n, est_g, est_l2, b.est_stride, [](const char*) {})) return 1;
        db->band_blocks = std::move(nb);
    }
    BlocksState& b = *db->band_blocks;
    if (b.g_xlo != g->x_lo || b.g_xhi != g->x_hi || !fits) {
        // another band: what the last call measured (launch sizes, the waves the chip holds of the wide kernel at its LDS) belongs to its geometry
        for (auto& c : b.slice_counts) c.valid = false;
        b.have_counts = false; b.k1w_slots = 0;
    }
    b.n_states = n_streams;
    b.g_rows = n_rows; b.g_bins = bins; b.g_xlo = g->x_lo; b.g_xhi = g->x_hi; b.g_sbase = (uint32_t)g->stream_base;
    {
        int key_bits = 1;
        while ((1ull << key_bits) <= (uint64_t)b.n_states + 1) ++key_bits;          // streams; all-ones = never written
        b.key_bits = key_bits;
        // the weight digits of an unpacked key word as the whole-matrix call cuts them (its stream bits, 22 beyond its limit): a weight then makes as many
        // records in a band as in the whole call, and the bands' records add up to the whole call's
        int whole_bits = 1;
        const uint64_t whole_states = (uint64_t)b.NB * (b.NB + 1) / 2;
        while (whole_bits < 22 && (1ull << whole_bits) <= whole_states + 1) ++whole_bits;
        b.digit_bits = wide_digit_bits(std::max(whole_bits, key_bits));
    }
    return 0;
}

kmdb_blocks_band_info kmdb_blocks_band_last(const kmdb_db* db, bool band_state) {
    kmdb_blocks_band_info o{};
    const BlocksState* s = band_state ? db->band_blocks.get() : db->blocks.get();
    if (!s) return o;
    const BlocksState& b = *s;
    o.key_bits = (uint32_t)b.key_bits; o.row_mode = b.row_mode ? 1u : 0u; o.l2_on = b.l2_on ? 1u : 0u; o.attempts = b.attempts;
    o.slices = std::max<uint32_t>(1u, b.n_slices);
    o.records = b.last_records; o.est_records = b.est_records;
    o.units = b.last_band_units;
    return o;
}
