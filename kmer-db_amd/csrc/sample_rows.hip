// sample_rows.hip — the candidates of `-sample-rows <criterion>:<count>` chosen on the device (replaces the nnz-sized half of
// SparseMatrix::add_to_sampler + Sampler, reference src/array.h:450-540, src/sampler.h; call site console_all2all_sparse.cpp:70-89).
//
// A pair (i, j), i > j, with a non-zero cell that passes the widened filters is offered to sample i and to sample j with one score.  The device
// ranks by the criterion's PROXY — the plain ratio the measure is monotone in (cell_filter.h), negated for the measures that fall with it — and
// per sample s finds T_s, the count-th largest proxy of its symmetric row, by a radix select: four 8-bit passes over the order-preserving 32-bit
// key of the proxy rounded to float (rounding is monotone, so the count-th largest key is the key of the count-th largest proxy; 1 KB of
// histogram per sample: 51 MB at 50 000 samples).  It then emits every cell whose key is >= the key of T_s narrowed by the margin of the
// filters (1e-6 relative) plus the float rounding (2^-22): ties and the margin band come out, a row with fewer than `count` cells comes out whole.
// The host decides (host_sampler.cpp) with the reference's double arithmetic.
//
// A cell whose proxy is infinite or NaN (a sample k-mer count of 0 beside a non-zero cell, a + b - c wrapping to 0) has no rank the device can
// know: the host scores it +inf under jaccard / min / max / cosine and NaN — below every number — under the four log measures.  A row that
// holds ANY such cell therefore comes out whole (a flag per sample, set in the first histogram pass and read at digit 0), so that the host
// still sees a superset of the row's true best `count` whichever way it ranks the cell.
//
// Every pass reads the triangle in row order, one workgroup per tile of width x width cells: the tile's keys go to LDS once and every one of
// its 2 x width samples — `width` row samples, `width` column samples — reads its own line of the tile from there (a wave per sample, the
// column lines through a padded stride), so no pass walks a column of the triangle.  Passes: 4 histogram, 1 count, 1 emit = 6 reads of the
// (touched tiles of the) triangle.  The emit appends through one cursor per sample; a rank sort inside every row then gives ascending columns.
//
// The same passes select on a RECTANGLE of two sample sets, the off-diagonal cell of the all2all-parts grid (db2db_sp + compact2(filter) +
// add_to_sampler, reference src/console_all2all_parts.cpp:179-195, 225-241): the tile kernel is a template over the source of its cells
// (TriSamples / RectSamples below) and everything else works on SLOTS — the N samples of a triangle, the nr row samples followed by the nc
// column samples of a rectangle.  A pair of a rectangle has one score with the cell's row as the row sample, on either of its two lines.
//
// The QUERY ROWS of new2all (RowSegs, sr_segment_kernel) are the third source, and the one-sided one: a query keeps its best database samples,
// the database samples collect nothing.  A row has no column line, so the tile transpose buys nothing; the rows are cut as new2all_sparse.hip
// cuts them — a wave per segment of N2S_SEG columns of one row — and the same six passes run over the segments.  The histogram pass folds the
// 32 lines of a segment into the wave's own 256 bins in LDS and adds the non-zero bins to the row's global histogram once per segment; the
// count pass writes one count per segment, a scan over the segments gives the emit its places, and columns come out ascending by construction:
// no per-row cursor and no rank sort (a query row that comes out whole can hold 10^5 entries, and the rank sort is quadratic in a row).
#include "device_common.h"
#include "cell_filter.h"
#include "sample_rows.h"

#include "prim.h"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <vector>

namespace {

constexpr uint32_t SR_W = 64;           // widest tile: a lane per column
constexpr uint32_t SR_KEY_BEST = 0xFFFFFFFFu;
enum { SR_HIST = 0, SR_COUNT, SR_EMIT };

struct SrJob {                          // what every source of cells shares
    const unsigned char* touched;       // [tiles] or nullptr: only flagged tiles are read
    DevFilter f;                        // widened bounds (f.counts is not read here: the k-mer counts come from the source)
    int kind, flip;                     // RATIO_* of the criterion; 1: the measure falls with its ratio
    uint32_t count;
};
// The source of the cells — the one thing of a pass that knows a geometry (as distance.hip's TextCells / TriangleCells / RowCells): which tile is
// where, which cell a lane loads, whose k-mer counts a and b are, and which slot of hist / state / thr / len / cursor / row_ptr a line belongs to.
// TriSamples: the lower triangle of N samples, flat cells [cell_lo, cell_hi); tile (X, Y), Y <= X, has the index X (X + 1) / 2 + Y as in
// kmdb_db.tile_touched; the slot of a row line and of a column line is the sample itself.
struct TriSamples {
    const uint32_t* M;                  // cell `cell_lo` of the lower triangle
    uint64_t N, cell_lo, cell_hi;
    uint32_t W;                         // tile width (the block width of the handle when its tile flags are used, else SR_W)
    const uint32_t* counts;             // [N] k-mer counts of the samples
    __device__ __forceinline__ uint32_t width() const { return W; }
    __device__ __forceinline__ bool tile(uint32_t t, uint64_t& i0, uint64_t& j0) const {       // false: no cell of the tile is in the range
        uint32_t X = (uint32_t)((sqrt(8.0 * (double)t + 1.0) - 1.0) * 0.5);
        while ((uint64_t)X * (X + 1) / 2 > t) --X;
        while ((uint64_t)(X + 1) * (X + 2) / 2 <= t) ++X;
        const uint32_t Y = t - (uint32_t)((uint64_t)X * (X + 1) / 2);
        i0 = (uint64_t)X * W; j0 = (uint64_t)Y * W;
        if (i0 >= N) return false;
        // the tile's rows against the flat range: rows [i0, i1], cells tri(i0) + j0 .. tri(i1) + i1 - 1
        const uint64_t i1 = (i0 + W < N ? i0 + W : N) - 1;
        return !(tri64(i1) + i1 <= cell_lo || tri64(i0 ? i0 : 1) + j0 >= cell_hi);
    }
    __device__ __forceinline__ uint32_t load(uint64_t i, uint64_t j, uint32_t lane) const {
        if (lane < W && i < N && j < i) {
            const uint64_t flat = tri64(i) + j;
            if (flat >= cell_lo && flat < cell_hi) return M[flat - cell_lo];
        }
        return 0u;
    }
    __device__ __forceinline__ uint32_t a(uint64_t i) const { return counts[i]; }
    __device__ __forceinline__ uint32_t b(uint64_t j) const { return counts[j]; }
    __device__ __forceinline__ bool row_slot(uint64_t i, uint64_t& s) const { s = i; return i < N; }
    __device__ __forceinline__ bool col_slot(uint64_t j, uint64_t& s) const { s = j; return j < N; }
};
// RectSamples: a row-major nr x nc rectangle of two sample sets, cell (r, c) at r * nc + c (64-bit: 66 000 x 66 000 cells exceed 2^32).  Tile t is
// (t / nbc, t % nbc), the stream numbering of db2db.hip's d2_emit_kernel / d2_tile_flags_kernel, always 64 wide.  Slots [0, nr) are the row
// samples, [nr, nr + nc) the column samples; a is ALWAYS the row sample's count and b the column sample's, whichever line ranks the cell.
struct RectSamples {
    const uint32_t* M;
    uint32_t nr, nc, nbc;
    const uint32_t *row_counts, *col_counts;
    __device__ __forceinline__ uint32_t width() const { return SR_W; }
    __device__ __forceinline__ bool tile(uint32_t t, uint64_t& i0, uint64_t& j0) const {
        i0 = (uint64_t)(t / nbc) * SR_W; j0 = (uint64_t)(t % nbc) * SR_W;
        return i0 < nr;
    }
    // (a lane whose column is >= nc loads nothing: in a row-major rectangle that address is a cell of the NEXT row — d2_row_tiles_kernel)
    __device__ __forceinline__ uint32_t load(uint64_t i, uint64_t j, uint32_t) const { return i < nr && j < nc ? M[i * nc + j] : 0u; }
    __device__ __forceinline__ uint32_t a(uint64_t i) const { return row_counts[i]; }
    __device__ __forceinline__ uint32_t b(uint64_t j) const { return col_counts[j]; }
    __device__ __forceinline__ bool row_slot(uint64_t i, uint64_t& s) const { s = i; return i < nr; }
    __device__ __forceinline__ bool col_slot(uint64_t j, uint64_t& s) const { s = (uint64_t)nr + j; return j < nc; }
};
struct SrState { uint32_t prefix, k, done, total; };   // done: 1 the row comes out whole, 2 cut at T_s; total: cells of the row that pass the widened filters

// order-preserving key of the proxy: 0 is kept for "no cell", SR_KEY_BEST for a NaN or infinite proxy (its whole row goes to the host)
__device__ __forceinline__ uint32_t sr_key(const SrJob& q, uint32_t c, uint32_t a, uint32_t b) {
    double x = dev_ratio(q.kind, c, a, b);
    if (q.flip) x = -x;
    if (!(fabs(x) <= 1.7976931348623157e308)) return SR_KEY_BEST;
    const uint32_t u = __float_as_uint((float)x);
    if ((u & 0x7F800000u) == 0x7F800000u) return SR_KEY_BEST;
    return (u >> 31) ? ~u : (u | 0x80000000u);
}
__host__ __device__ inline float sr_key_float(uint32_t key) {
    const uint32_t u = (key >> 31) ? (key & 0x7FFFFFFFu) : ~key;
    float f;
#if defined(__HIP_DEVICE_COMPILE__)
    f = __uint_as_float(u);
#else
    std::memcpy(&f, &u, 4);
#endif
    return f;
}
__host__ __device__ inline uint32_t sr_float_key(float f) {
    uint32_t u;
#if defined(__HIP_DEVICE_COMPILE__)
    u = __float_as_uint(f);
#else
    std::memcpy(&u, &f, 4);
#endif
    return (u >> 31) ? ~u : (u | 0x80000000u);
}

// One workgroup (4 waves) per tile of the source.
//   SR_HIST : digit `digit` (0 = top 8 bits) of the keys that share the sample's prefix goes to hist[s][256]; at digit 0 a line that holds
//             an SR_KEY_BEST key sets unrankable[s]
//   SR_COUNT: len[s] += cells with key >= thr[s]            (thr 0: the sample is skipped)
//   SR_EMIT : those cells appended at row_ptr[s] + cursor[s]++ (a row line carries the column's id, a column line the row's)
template <int MODE, class Cells>
__global__ __launch_bounds__(256) void sr_tile_kernel(const Cells src, const SrJob q, uint32_t digit, const SrState* __restrict__ state, uint32_t* __restrict__ hist,
                                                      const uint32_t* __restrict__ thr, unsigned long long* __restrict__ len,
                                                      const unsigned long long* __restrict__ row_ptr, uint32_t* __restrict__ cursor,
                                                      uint32_t* __restrict__ ocol, uint32_t* __restrict__ oval, uint32_t* __restrict__ unrankable) {
    __shared__ uint32_t s_key[SR_W][SR_W + 1];
    __shared__ uint32_t s_val[SR_W][SR_W + 1];
    const uint32_t t = blockIdx.x;
    if (q.touched && !q.touched[t]) return;
    const uint32_t W = src.width(), lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint64_t i0, j0;
    if (!src.tile(t, i0, j0)) return;
    uint32_t any = 0;
    for (uint32_t r = wave; r < W; r += 4) {
        const uint64_t i = i0 + r, j = j0 + lane;
        const uint32_t v = src.load(i, j, lane);
        uint32_t key = 0;
        if (v) {
            const uint32_t a = src.a(i), b = src.b(j);
            if (q.f.n == 0 || dev_keep_ab(q.f, v, a, b)) key = sr_key(q, v, a, b);
        }
        s_key[r][lane] = key;
        s_val[r][lane] = v;
        any |= key;
    }
    if (!__syncthreads_or((int)(any != 0))) return;
    // the 2 W samples of the tile, a wave each: slots [0, W) the row samples, [W, 2 W) the column samples
    for (uint32_t slot = wave; slot < 2 * W; slot += 4) {
        const bool isrow = slot < W;
        const uint32_t a = isrow ? slot : slot - W;
        uint64_t s;
        if (!(isrow ? src.row_slot(i0 + a, s) : src.col_slot(j0 + a, s))) continue;
        uint32_t key = 0, v = 0;
        if (lane < W) {
            key = isrow ? s_key[a][lane] : s_key[lane][a];
            v = isrow ? s_val[a][lane] : s_val[lane][a];
        }
        const uint32_t other = (uint32_t)(isrow ? j0 + lane : i0 + lane);
        if (MODE == SR_HIST) {
            const SrState st = state[s];
            if (st.done) continue;
            if (digit == 0 && __ballot(key == SR_KEY_BEST) && lane == 0) unrankable[s] = 1u;
            bool on = key != 0 && (digit == 0 || (key >> (32 - 8 * digit)) == st.prefix);
            const uint32_t bin = (key >> (24 - 8 * digit)) & 255u;
            unsigned long long m = __ballot(on);
            while (m) {                                        // one atomic per distinct bin of the line
                const int lead = __builtin_ctzll(m);
                const uint32_t lb = (uint32_t)__shfl((int)bin, lead, 64);
                const unsigned long long same = __ballot(on && bin == lb);
                if ((int)lane == lead) atomicAdd(&hist[s * 256 + lb], (uint32_t)__popcll(same));
                m &= ~same;
            }
        } else {
            const uint32_t th = thr[s];
            const bool on = th != 0 && key >= th;
            const unsigned long long m = __ballot(on);
            if (!m) continue;
            const uint32_t n = (uint32_t)__popcll(m);
            if (MODE == SR_COUNT) {
                if (lane == 0) atomicAdd(&len[s], (unsigned long long)n);
            } else {
                uint32_t base = 0;
                if (lane == 0) base = atomicAdd(&cursor[s], n);
                base = (uint32_t)__shfl((int)base, 0, 64);
                if (on) {
                    const unsigned long long o = row_ptr[s] + base + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
                    ocol[o] = other;
                    oval[o] = v;
                }
            }
        }
    }
}

// After histogram pass `digit`: the bin that holds the sample's k-th largest key extends its prefix; the histogram is zeroed for the next pass.
// After the last digit the prefix IS the key of T_s, and thr[s] the key of T_s narrowed by the margin.
__global__ void sr_select_kernel(uint32_t* __restrict__ hist, SrState* __restrict__ state, uint32_t* __restrict__ thr, const uint32_t* __restrict__ unrankable,
                                 uint64_t N, uint32_t digit, uint32_t count) {
    const uint64_t s = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= N) return;
    SrState st = state[s];
    if (st.done) return;
    uint32_t* h = hist + s * 256;
    if (digit == 0) {
        unsigned long long total = 0;
        for (int b = 0; b < 256; ++b) total += h[b];
        st.total = (uint32_t)total;
        // fewer than `count` cells, or a cell the device cannot rank: everything is kept
        if (total < count || unrankable[s]) { st.done = 1; state[s] = st; thr[s] = total ? 1u : 0u; return; }
        st.k = count; st.prefix = 0;
    }
    uint32_t acc = 0;
    for (int b = 255; b >= 0; --b) {
        const uint32_t c = h[b];
        h[b] = 0;
        if (st.k && acc + c >= st.k) { st.prefix = (st.prefix << 8) | (uint32_t)b; st.k -= acc; acc = 0; for (int z = b - 1; z >= 0; --z) h[z] = 0; break; }
        acc += c;
    }
    if (digit == 3) {                                                     // (the keys of a row that reaches this are all finite floats)
        const double T = (double)sr_key_float(st.prefix);
        const double narrowed = T - fabs(T) * (1e-6 + 2.384185791015625e-07);
        float f = (float)narrowed;
        if ((double)f > narrowed) f = nextafterf(f, -INFINITY);
        uint32_t key = sr_float_key(f);
        if (key == 0) key = 1;
        thr[s] = key;
        st.done = 2;
    }
    state[s] = st;
}

// rows that were truncated: cut at T_s with something left below the cut
__global__ void sr_truncated_kernel(const SrState* __restrict__ state, const unsigned long long* __restrict__ len, uint64_t N, unsigned long long* __restrict__ n_truncated) {
    const uint64_t s = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (s < N && state[s].done == 2 && len[s] < state[s].total) atomicAdd(n_truncated, 1ull);
}

// the appended entries of every row into ascending columns: rank of an entry = entries of the row with a smaller column (columns are distinct)
__global__ __launch_bounds__(64) void sr_sort_rows_kernel(const unsigned long long* __restrict__ row_ptr, const uint32_t* __restrict__ tcol,
                                                          const uint32_t* __restrict__ tval, uint32_t* __restrict__ col, uint32_t* __restrict__ val) {
    __shared__ uint32_t s_c[1024];
    const unsigned long long b = row_ptr[blockIdx.x], e = row_ptr[blockIdx.x + 1];
    const uint64_t n = e - b;
    if (!n) return;
    for (uint64_t m0 = 0; m0 < n; m0 += 64) {                     // 64 entries at a time, ranked against the row in chunks of 1024
        const uint64_t m = m0 + threadIdx.x;
        const uint32_t mine = m < n ? tcol[b + m] : 0u;
        uint64_t rank = 0;
        for (uint64_t c0 = 0; c0 < n; c0 += 1024) {
            const uint32_t cn = (uint32_t)(n - c0 < 1024 ? n - c0 : 1024);
            __syncthreads();
            for (uint32_t x = threadIdx.x; x < cn; x += 64) s_c[x] = tcol[b + c0 + x];
            __syncthreads();
            if (m < n) for (uint32_t x = 0; x < cn; ++x) rank += s_c[x] < mine ? 1u : 0u;
        }
        if (m < n) { col[b + rank] = mine; val[b + rank] = tval[b + m]; }
    }
}

// RowSegs: the flat cells [cell_lo, cell_hi) of a row-major nq x N rectangle of QUERY rows (cell q * N + s = query q, database sample s; M points
// at cell cell_lo — the convention of kmdb_new2all_rows_sparse_device).  The slots are the rows that meet the range: slot = q - q_lo.  Segment
// slot * nseg + s holds the columns [s * N2S_SEG, min(N, (s + 1) * N2S_SEG)) of its row.  a = the QUERY's k-mer count, b = the sample's.
struct RowSegs {
    const uint32_t* M;
    uint32_t N, nseg;
    uint64_t q_lo, cell_lo, cell_hi;
    const uint32_t* query_counts;       // [slots] the k-mer counts of the queries q_lo ...
    const uint32_t* counts;             // [N] of the database samples
};

// One wave (a workgroup of its own) per segment `seg0 + blockIdx.x`: 32 lines of 64 consecutive cells.  A lane whose column is beyond the row,
// or whose cell lies outside [cell_lo, cell_hi), loads nothing (that address is a cell of the next row, of another device's chunk, or of
// nothing at all); cell offsets are 64-bit.
//   SR_HIST : the ballot loop of sr_tile_kernel folds every line into s_hist, the wave's OWN 256 bins: the leading lane of a bin does a plain
//             add — within a line every bin is added to once, and the barrier after the line (the workgroup IS the wave: no other wave waits
//             on it, it only orders the wave's LDS accesses) puts the next line's reads of a bin behind this line's write, whichever lane
//             made it.  The segment ends with one global atomicAdd per non-zero bin: up to 32 times fewer than one per line.
//   SR_COUNT: seg_len[seg] = cells with key >= thr[slot]   (seg_len is zeroed: a skipped slot writes nothing; no atomics)
//   SR_EMIT : those cells from seg_ptr[seg] on, line after line at the running ballot prefix: ascending columns by construction
template <int MODE>
__global__ __launch_bounds__(64) void sr_segment_kernel(const RowSegs src, const SrJob q, uint32_t digit, uint64_t seg0, uint64_t seg_end,
                                                        const SrState* __restrict__ state, uint32_t* __restrict__ hist, const uint32_t* __restrict__ thr,
                                                        unsigned long long* __restrict__ seg_len, const unsigned long long* __restrict__ seg_ptr,
                                                        uint32_t* __restrict__ ocol, uint32_t* __restrict__ oval, uint32_t* __restrict__ unrankable) {
    __shared__ uint32_t s_hist[256];
    const uint64_t seg = seg0 + blockIdx.x;
    if (seg >= seg_end) return;
    const uint32_t lane = threadIdx.x;
    const uint64_t slot = seg / src.nseg;
    const uint32_t s = (uint32_t)(seg - slot * src.nseg);
    const uint32_t c0 = s * N2S_SEG, c1 = src.N - c0 < N2S_SEG ? src.N : c0 + N2S_SEG;      // (s < nseg: c0 < N)
    const uint64_t base = (src.q_lo + slot) * (uint64_t)src.N;
    SrState st{};
    uint32_t th = 0;
    if (MODE == SR_HIST) {
        st = state[slot];
        if (st.done) return;
        for (uint32_t b = lane; b < 256u; b += 64u) s_hist[b] = 0u;
        __syncthreads();
    } else {
        th = thr[slot];
        if (th == 0) return;
    }
    const uint32_t a = src.query_counts[slot];                   // once per wave
    unsigned long long out = MODE == SR_EMIT ? seg_ptr[seg] : 0ull;
    uint32_t count = 0;
    bool best = false, any = false;
    for (uint32_t j0 = c0; j0 < c1; j0 += 64u) {
        const uint32_t j = j0 + lane;
        const uint64_t cell = base + j;
        uint32_t v = 0;
        if (j < c1 && cell >= src.cell_lo && cell < src.cell_hi) v = src.M[cell - src.cell_lo];
        if (!__ballot(v != 0)) continue;                         // (most lines of a sparse row)
        uint32_t key = 0;
        if (v) {
            const uint32_t b = src.counts[j];
            if (q.f.n == 0 || dev_keep_ab(q.f, v, a, b)) key = sr_key(q, v, a, b);
        }
        if (MODE == SR_HIST) {
            best |= key == SR_KEY_BEST;
            const bool on = key != 0 && (digit == 0 || (key >> (32 - 8 * digit)) == st.prefix);
            const uint32_t bin = (key >> (24 - 8 * digit)) & 255u;
            unsigned long long m = __ballot(on);
            if (!m) continue;
            any = true;
            while (m) {                                          // one step per distinct bin of the line
                const int lead = __builtin_ctzll(m);
                const uint32_t lb = (uint32_t)__shfl((int)bin, lead, 64);
                const unsigned long long same = __ballot(on && bin == lb);
                if ((int)lane == lead) s_hist[lb] += (uint32_t)__popcll(same);
                m &= ~same;
            }
            __syncthreads();
        } else {
            const bool on = key >= th;                           // (th >= 1: a key of 0 is no cell)
            const unsigned long long m = __ballot(on);
            if (MODE == SR_EMIT) {
                if (on) { const unsigned long long o = out + (uint32_t)__popcll(m & ((1ull << lane) - 1ull)); ocol[o] = j; oval[o] = v; }
                out += (uint32_t)__popcll(m);
            } else count += (uint32_t)__popcll(m);
        }
    }
    if (MODE == SR_HIST) {
        if (digit == 0 && __ballot(best) && lane == 0) unrankable[slot] = 1u;
        if (any)                                                 // (wave-uniform; the last line's barrier stands before these reads)
            for (uint32_t b = lane; b < 256u; b += 64u) {
                const uint32_t n = s_hist[b];
                if (n) atomicAdd(&hist[slot * 256 + b], n);
            }
    } else if (MODE == SR_COUNT) {
        if (lane == 0) seg_len[seg] = count;
    }
}

// row_ptr[slot] = the scan at the first segment of the slot's row (row_ptr[N] = the scan's last entry, the total), len[slot] = the row's cells
__global__ void sr_seg_row_ptr_kernel(const unsigned long long* __restrict__ seg_ptr, uint32_t nseg, uint64_t N, unsigned long long* __restrict__ row_ptr,
                                      unsigned long long* __restrict__ len) {
    const uint64_t s = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (s > N) return;
    const unsigned long long b = seg_ptr[s * nseg];
    row_ptr[s] = b;
    if (s < N) len[s] = seg_ptr[(s + 1) * nseg] - b;
}

// The passes over the query rows: N slots (out->row_ptr is sized and zeroed), N * nseg segments per pass, at most N2S_GRID_MAX per launch.
template <int MODE>
int sr_segments_launch(hipStream_t st, const RowSegs& src, const SrJob& q, uint32_t digit, uint64_t n_segs, const SrState* state, uint32_t* hist, const uint32_t* thr,
                       unsigned long long* seg_len, const unsigned long long* seg_ptr, uint32_t* ocol, uint32_t* oval, uint32_t* unrankable) {
    for (uint64_t s0 = 0; s0 < n_segs; s0 += N2S_GRID_MAX) {
        hipLaunchKernelGGL((sr_segment_kernel<MODE>), dim3((unsigned)std::min(N2S_GRID_MAX, n_segs - s0)), dim3(64), 0, st, src, q, digit, s0, n_segs, state, hist, thr,
                           seg_len, seg_ptr, ocol, oval, unrankable);
        HIP_TRY(hipGetLastError());
    }
    return 0;
}
int sr_run_rows(hipStream_t st, const RowSegs& src, const SrJob& q, uint64_t N, const uint32_t* only_rows, size_t n_only, kmdb_sample_result* out) {
    const uint64_t n_segs = N * src.nseg;
    DevBuf<uint32_t> hist, thr, col, val, unrankable;
    DevBuf<SrState> state;
    DevBuf<unsigned long long> seg_len, seg_ptr, len, row_ptr, ntr;
    DevBuf<char> tmp;
    DevEvent e0, e1;
    if (e0.create() || e1.create()) return 1;
    DEV_ALLOC(thr, N);
    DEV_ALLOC(seg_len, n_segs + 1);
    DEV_ALLOC(seg_ptr, n_segs + 1);
    DEV_ALLOC(len, N);
    DEV_ALLOC(row_ptr, N + 1);
    DEV_ALLOC(ntr, 1);
    HIP_TRY(hipEventRecord(e0, st));
    HIP_TRY(hipMemsetAsync(seg_len, 0, (n_segs + 1) * 8, st));
    HIP_TRY(hipMemsetAsync(ntr, 0, 8, st));
    if (only_rows) {
        // the re-fetch: the listed rows whole, every other row skipped
        std::vector<uint32_t> h_thr(N, 0);
        for (size_t i = 0; i < n_only; ++i) h_thr[only_rows[i]] = 1u;
        HIP_TRY(hipMemcpyAsync(thr, h_thr.data(), N * 4, hipMemcpyHostToDevice, st));
        HIP_TRY(hipStreamSynchronize(st));
    } else {
        DEV_ALLOC(hist, N * 256);
        DEV_ALLOC(state, N);
        DEV_ALLOC(unrankable, N);
        HIP_TRY(hipMemsetAsync(hist, 0, N * 256 * 4, st));
        HIP_TRY(hipMemsetAsync(state, 0, N * sizeof(SrState), st));
        HIP_TRY(hipMemsetAsync(thr, 0, N * 4, st));
        HIP_TRY(hipMemsetAsync(unrankable, 0, N * 4, st));
        for (uint32_t d = 0; d < 4; ++d) {
            if (sr_segments_launch<SR_HIST>(st, src, q, d, n_segs, state, hist, nullptr, nullptr, nullptr, nullptr, nullptr, unrankable)) return 1;
            hipLaunchKernelGGL(sr_select_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, st, hist, state, thr, (const uint32_t*)unrankable.get(), N, d, q.count);
            HIP_TRY(hipGetLastError());
            ++out->passes;
        }
    }
    if (sr_segments_launch<SR_COUNT>(st, src, q, 0u, n_segs, nullptr, nullptr, thr, seg_len, nullptr, nullptr, nullptr, nullptr)) return 1;
    ++out->passes;
    size_t tmp_bytes = 0;
    HIP_TRY(prim::exclusive_sum(nullptr, tmp_bytes, seg_len.get(), seg_ptr.get(), (size_t)(n_segs + 1), st));
    DEV_ALLOC(tmp, std::max<size_t>(tmp_bytes, 16));
    HIP_TRY(prim::exclusive_sum(tmp, tmp_bytes, seg_len.get(), seg_ptr.get(), (size_t)(n_segs + 1), st));
    hipLaunchKernelGGL(sr_seg_row_ptr_kernel, dim3((unsigned)((N + 1 + 255) / 256)), dim3(256), 0, st, (const unsigned long long*)seg_ptr.get(), src.nseg, N, row_ptr.get(), len.get());
    if (!only_rows) hipLaunchKernelGGL(sr_truncated_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, st, state, (const unsigned long long*)len.get(), N, ntr);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(out->row_ptr.data(), row_ptr, (N + 1) * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    out->d2h_bytes += (N + 1) * 8;
    const uint64_t nnz = out->row_ptr[N];
    if (nnz > src.cell_hi - src.cell_lo) return kmdb_set_error("kmdb_sample_candidates: internal error (more candidates than cells)");
    if (nnz) {
        DEV_ALLOC(col, nnz);
        DEV_ALLOC(val, nnz);
        if (sr_segments_launch<SR_EMIT>(st, src, q, 0u, n_segs, nullptr, nullptr, thr, nullptr, seg_ptr, col, val, nullptr)) return 1;
        ++out->passes;
    }
    HIP_TRY(hipEventRecord(e1, st));
    if (nnz) {
        out->col.resize(nnz); out->val.resize(nnz);
        HIP_TRY(hipMemcpyAsync(out->col.data(), col, nnz * 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(out->val.data(), val, nnz * 4, hipMemcpyDeviceToHost, st));
        out->d2h_bytes += nnz * 8;
        if (!only_rows) {
            unsigned long long h_ntr = 0;
            HIP_TRY(hipMemcpyAsync(&h_ntr, ntr, 8, hipMemcpyDeviceToHost, st));
            HIP_TRY(hipStreamSynchronize(st));
            out->rows_truncated = h_ntr;
            out->d2h_bytes += 8;
        }
    }
    HIP_TRY(hipStreamSynchronize(st));
    float ms = 0;
    HIP_TRY(hipEventElapsedTime(&ms, e0, e1));
    out->select_ms = ms;
    return 0;
}

// the passes over one source of cells: N slots (out->row_ptr is sized and zeroed), `tiles` workgroups per pass
template <class Cells>
int sr_run(hipStream_t st, const Cells& src, const SrJob& q, uint64_t N, uint64_t tiles, const uint32_t* only_rows, size_t n_only, kmdb_sample_result* out) {
    DevBuf<uint32_t> hist, thr, cursor, tcol, tval, col, val, unrankable;
    DevBuf<SrState> state;
    DevBuf<unsigned long long> len, row_ptr, ntr;
    DevBuf<char> tmp;
    DevEvent e0, e1;
    if (e0.create() || e1.create()) return 1;
    DEV_ALLOC(thr, std::max<uint64_t>(N, 1));
    DEV_ALLOC(len, N + 1);
    DEV_ALLOC(row_ptr, N + 1);
    DEV_ALLOC(cursor, std::max<uint64_t>(N, 1));
    DEV_ALLOC(ntr, 1);
    HIP_TRY(hipEventRecord(e0, st));
    HIP_TRY(hipMemsetAsync(len, 0, (N + 1) * 8, st));
    HIP_TRY(hipMemsetAsync(cursor, 0, N * 4, st));
    HIP_TRY(hipMemsetAsync(ntr, 0, 8, st));
    const dim3 grid((unsigned)tiles), block(256);
    if (only_rows) {
        // the re-fetch: the listed rows whole, every other sample skipped
        std::vector<uint32_t> h_thr(N, 0);
        for (size_t i = 0; i < n_only; ++i) h_thr[only_rows[i]] = 1u;
        HIP_TRY(hipMemcpyAsync(thr, h_thr.data(), N * 4, hipMemcpyHostToDevice, st));
        HIP_TRY(hipStreamSynchronize(st));
    } else {
        DEV_ALLOC(hist, std::max<uint64_t>(N * 256, 1));
        DEV_ALLOC(state, std::max<uint64_t>(N, 1));
        HIP_TRY(hipMemsetAsync(hist, 0, N * 256 * 4, st));
        HIP_TRY(hipMemsetAsync(state, 0, N * sizeof(SrState), st));
        HIP_TRY(hipMemsetAsync(thr, 0, N * 4, st));
        DEV_ALLOC(unrankable, std::max<uint64_t>(N, 1));
        HIP_TRY(hipMemsetAsync(unrankable, 0, N * 4, st));
        for (uint32_t d = 0; d < 4; ++d) {
            hipLaunchKernelGGL((sr_tile_kernel<SR_HIST, Cells>), grid, block, 0, st, src, q, d, state, hist, (const uint32_t*)nullptr, (unsigned long long*)nullptr,
                               (const unsigned long long*)nullptr, (uint32_t*)nullptr, (uint32_t*)nullptr, (uint32_t*)nullptr, unrankable.get());
            hipLaunchKernelGGL(sr_select_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, st, hist, state, thr, (const uint32_t*)unrankable.get(), N, d, q.count);
            ++out->passes;
        }
        HIP_TRY(hipGetLastError());
    }
    hipLaunchKernelGGL((sr_tile_kernel<SR_COUNT, Cells>), grid, block, 0, st, src, q, 0u, (const SrState*)nullptr, (uint32_t*)nullptr, thr, len, (const unsigned long long*)nullptr,
                       (uint32_t*)nullptr, (uint32_t*)nullptr, (uint32_t*)nullptr, (uint32_t*)nullptr);
    ++out->passes;
    if (!only_rows) hipLaunchKernelGGL(sr_truncated_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, st, state, len, N, ntr);
    size_t tmp_bytes = 0;
    HIP_TRY(prim::exclusive_sum(nullptr, tmp_bytes, len.get(), row_ptr.get(), (int)(N + 1), st));
    DEV_ALLOC(tmp, std::max<size_t>(tmp_bytes, 16));
    HIP_TRY(prim::exclusive_sum(tmp, tmp_bytes, len.get(), row_ptr.get(), (int)(N + 1), st));
    static_assert(sizeof(unsigned long long) == sizeof(uint64_t), "row pointers are copied as they are");
    HIP_TRY(hipMemcpyAsync(out->row_ptr.data(), row_ptr, (N + 1) * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    out->d2h_bytes += (N + 1) * 8;
    const uint64_t nnz = out->row_ptr[N];
    if (nnz) {
        DEV_ALLOC(tcol, std::max<uint64_t>(nnz, 1));
        DEV_ALLOC(tval, std::max<uint64_t>(nnz, 1));
        DEV_ALLOC(col, std::max<uint64_t>(nnz, 1));
        DEV_ALLOC(val, std::max<uint64_t>(nnz, 1));
        hipLaunchKernelGGL((sr_tile_kernel<SR_EMIT, Cells>), grid, block, 0, st, src, q, 0u, (const SrState*)nullptr, (uint32_t*)nullptr, thr, (unsigned long long*)nullptr, row_ptr, cursor,
                           tcol, tval, (uint32_t*)nullptr);
        ++out->passes;
        hipLaunchKernelGGL(sr_sort_rows_kernel, dim3((unsigned)N), dim3(64), 0, st, row_ptr, tcol, tval, col, val);
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipEventRecord(e1, st));
    if (nnz) {
        out->col.resize(nnz); out->val.resize(nnz);
        HIP_TRY(hipMemcpyAsync(out->col.data(), col, nnz * 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(out->val.data(), val, nnz * 4, hipMemcpyDeviceToHost, st));
        out->d2h_bytes += nnz * 8;
        if (!only_rows) {
            unsigned long long h_ntr = 0;
            HIP_TRY(hipMemcpyAsync(&h_ntr, ntr, 8, hipMemcpyDeviceToHost, st));
            HIP_TRY(hipStreamSynchronize(st));
            out->rows_truncated = h_ntr;
            out->d2h_bytes += 8;
        }
    }
    HIP_TRY(hipStreamSynchronize(st));
    float ms = 0;
    HIP_TRY(hipEventElapsedTime(&ms, e0, e1));
    out->select_ms = ms;
    return 0;
}

}  // namespace

int kmdb_sample_candidates(hipStream_t st, const kmdb_sample_job& j, const uint32_t* only_rows, size_t n_only, kmdb_sample_result* out) {
    const bool rect = j.rect, rows = j.query_rows;
    // (query rows: the slots are the rows that meet the range)
    const uint64_t q_lo = rows && j.cell_hi > j.cell_lo && j.nc ? j.cell_lo / j.nc : 0;
    const uint64_t N = rows ? (j.cell_hi > j.cell_lo && j.nc ? (j.cell_hi - 1) / j.nc + 1 - q_lo : 0) : rect ? j.nr + j.nc : j.N;
    out->row_ptr.assign(N + 1, 0);
    out->col.clear(); out->val.clear();
    out->rows_truncated = 0; out->d2h_bytes = 0; out->select_ms = 0; out->passes = 0;
    if (rows ? N == 0 : rect ? (j.nr == 0 || j.nc == 0) : (N < 2 || j.cell_hi <= j.cell_lo)) return 0;
    if (N + 1 >= (1ull << 31)) return kmdb_set_error("kmdb_sample_candidates: too many samples");
    SrJob q{};
    q.touched = j.touched;
    q.f.n = (int)j.n_bounds; q.f.counts = j.counts_dev;
    for (size_t i = 0; i < j.n_bounds; ++i) { q.f.kind[i] = j.bound_kind[i]; q.f.lo[i] = j.bound_lo[i]; q.f.hi[i] = j.bound_hi[i]; }
    q.kind = j.kind; q.flip = j.flip; q.count = j.count;
    if (rows) {
        if (j.nc >= (1ull << 32)) return kmdb_set_error("kmdb_sample_candidates: too many samples");
        const uint32_t nseg = (uint32_t)((j.nc + N2S_SEG - 1) / N2S_SEG);
        const RowSegs src{j.cells, (uint32_t)j.nc, nseg, q_lo, j.cell_lo, j.cell_hi, j.counts_dev, j.col_counts_dev};
        return sr_run_rows(st, src, q, N, only_rows, n_only, out);
    }
    if (rect) {
        if (j.nr >= (1ull << 32) || j.nc >= (1ull << 32)) return kmdb_set_error("kmdb_sample_candidates: too many samples");
        const uint64_t nbr = (j.nr + SR_W - 1) / SR_W, nbc = (j.nc + SR_W - 1) / SR_W, tiles = nbr * nbc;
        if (tiles >= (1ull << 31)) return kmdb_set_error("kmdb_sample_candidates: too many tiles");
        const RectSamples src{j.cells, (uint32_t)j.nr, (uint32_t)j.nc, (uint32_t)nbc, j.counts_dev, j.col_counts_dev};
        return sr_run(st, src, q, N, tiles, only_rows, n_only, out);
    }
    const uint32_t W = j.touched ? j.width : SR_W;
    if (W == 0 || W > SR_W) return kmdb_set_error("kmdb_sample_candidates: tile width out of range");
    const uint64_t B = (N + W - 1) / W, tiles = B * (B + 1) / 2;
    if (tiles >= (1ull << 31)) return kmdb_set_error("kmdb_sample_candidates: too many tiles");
    const TriSamples src{j.cells, N, j.cell_lo, j.cell_hi, W, j.counts_dev};
    return sr_run(st, src, q, N, tiles, only_rows, n_only, out);
}

// the key the device ranks by, from the host's own proxy: what the completeness rule of the entry points compares (engine.hip)
uint32_t kmdb_sample_proxy_key(double proxy) {
    if (!(std::fabs(proxy) <= 1.7976931348623157e308)) return SR_KEY_BEST;
    const float f = (float)proxy;
    if (std::isinf(f) || std::isnan(f)) return SR_KEY_BEST;
    return sr_float_key(f);
}
