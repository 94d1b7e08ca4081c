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

struct SrJob {
    const uint32_t* M;                  // cell `cell_lo` of the lower triangle
    uint64_t N, cell_lo, cell_hi;
    uint32_t W;                         // tile width (the block width of the handle when its tile flags are used, else SR_W)
    const unsigned char* touched;       // [tiles] or nullptr: only flagged tiles are read
    DevFilter f;                        // widened bounds; f.counts is always set (the proxy needs the k-mer counts)
    int kind, flip;                     // RATIO_* of the criterion; 1: the measure falls with its ratio
    uint32_t count;
};
struct SrState { uint32_t prefix, k, done, total; };   // done: 1 the row comes out whole, 2 cut at T_s; total: cells of the row that pass the widened filters

// order-preserving key of the proxy: 0 is kept for "no cell", SR_KEY_BEST for a NaN or infinite proxy (its whole row goes to the host)
__device__ __forceinline__ uint32_t sr_key(const SrJob& q, uint32_t c, uint32_t row, uint32_t col) {
    double x = dev_ratio(q.kind, c, q.f.counts[row], q.f.counts[col]);
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

// One workgroup (4 waves) per tile (X, Y), Y <= X, tile index X (X + 1) / 2 + Y as in kmdb_db.tile_touched.
//   SR_HIST : digit `digit` (0 = top 8 bits) of the keys that share the sample's prefix goes to hist[s][256]; at digit 0 a line that holds
//             an SR_KEY_BEST key sets unrankable[s]
//   SR_COUNT: len[s] += cells with key >= thr[s]            (thr 0: the sample is skipped)
//   SR_EMIT : those cells appended at row_ptr[s] + cursor[s]++
template <int MODE>
__global__ __launch_bounds__(256) void sr_tile_kernel(const SrJob q, uint32_t digit, const SrState* __restrict__ state, uint32_t* __restrict__ hist,
                                                      const uint32_t* __restrict__ thr, unsigned long long* __restrict__ len,
                                                      const unsigned long long* __restrict__ row_ptr, uint32_t* __restrict__ cursor,
                                                      uint32_t* __restrict__ ocol, uint32_t* __restrict__ oval, uint32_t* __restrict__ unrankable) {
    __shared__ uint32_t s_key[SR_W][SR_W + 1];
    __shared__ uint32_t s_val[SR_W][SR_W + 1];
    const uint32_t t = blockIdx.x;
    if (q.touched && !q.touched[t]) return;
    uint32_t X = (uint32_t)((sqrt(8.0 * (double)t + 1.0) - 1.0) * 0.5);
    while ((uint64_t)X * (X + 1) / 2 > t) --X;
    while ((uint64_t)(X + 1) * (X + 2) / 2 <= t) ++X;
    const uint32_t Y = t - (uint32_t)((uint64_t)X * (X + 1) / 2);
    const uint32_t W = q.W, lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint64_t i0 = (uint64_t)X * W, j0 = (uint64_t)Y * W;
    if (i0 >= q.N) return;
    {
        // the tile's rows against the flat range: rows [i0, i1], cells tri(i0) + j0 .. tri(i1) + i1 - 1
        const uint64_t i1 = (i0 + W < q.N ? i0 + W : q.N) - 1;
        if (tri64(i1) + i1 <= q.cell_lo || tri64(i0 ? i0 : 1) + j0 >= q.cell_hi) return;
    }
    uint32_t any = 0;
    for (uint32_t r = wave; r < W; r += 4) {
        const uint64_t i = i0 + r, j = j0 + lane;
        uint32_t v = 0, key = 0;
        if (lane < W && i < q.N && j < i) {
            const uint64_t flat = tri64(i) + j;
            if (flat >= q.cell_lo && flat < q.cell_hi) {
                v = q.M[flat - q.cell_lo];
                if (dev_keep(q.f, v, (uint32_t)i, (uint32_t)j)) key = sr_key(q, v, (uint32_t)i, (uint32_t)j);
            }
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
        const uint64_t s = isrow ? i0 + a : j0 + a;
        if (s >= q.N) continue;
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

}  // namespace

int kmdb_sample_candidates(hipStream_t st, const kmdb_sample_job& j, const uint32_t* only_rows, size_t n_only, kmdb_sample_result* out) {
    const uint64_t N = j.N;
    out->row_ptr.assign(N + 1, 0);
    out->col.clear(); out->val.clear();
    out->rows_truncated = 0; out->d2h_bytes = 0; out->select_ms = 0; out->passes = 0;
    if (N < 2 || j.cell_hi <= j.cell_lo) return 0;
    SrJob q{};
    q.M = j.cells; q.N = N; q.cell_lo = j.cell_lo; q.cell_hi = j.cell_hi;
    q.W = j.touched ? j.width : SR_W; q.touched = j.touched;
    if (q.W == 0 || q.W > SR_W) return kmdb_set_error("kmdb_sample_candidates: tile width out of range");
    q.f.n = (int)j.n_bounds; q.f.counts = j.counts_dev;
    for (size_t i = 0; i < j.n_bounds; ++i) { q.f.kind[i] = j.bound_kind[i]; q.f.lo[i] = j.bound_lo[i]; q.f.hi[i] = j.bound_hi[i]; }
    q.kind = j.kind; q.flip = j.flip; q.count = j.count;
    const uint64_t B = (N + q.W - 1) / q.W, tiles = B * (B + 1) / 2;
    if (tiles >= (1ull << 31)) return kmdb_set_error("kmdb_sample_candidates: too many tiles");
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
            hipLaunchKernelGGL((sr_tile_kernel<SR_HIST>), grid, block, 0, st, q, d, state, hist, (const uint32_t*)nullptr, (unsigned long long*)nullptr,
                               (const unsigned long long*)nullptr, (uint32_t*)nullptr, (uint32_t*)nullptr, (uint32_t*)nullptr, unrankable.get());
            hipLaunchKernelGGL(sr_select_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, st, hist, state, thr, (const uint32_t*)unrankable.get(), N, d, q.count);
            ++out->passes;
        }
        HIP_TRY(hipGetLastError());
    }
    hipLaunchKernelGGL((sr_tile_kernel<SR_COUNT>), grid, block, 0, st, q, 0u, (const SrState*)nullptr, (uint32_t*)nullptr, thr, len, (const unsigned long long*)nullptr,
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
        hipLaunchKernelGGL((sr_tile_kernel<SR_EMIT>), grid, block, 0, st, q, 0u, (const SrState*)nullptr, (uint32_t*)nullptr, thr, (unsigned long long*)nullptr, row_ptr, cursor,
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

// the key the device ranks by, from the host's own proxy: what the completeness rule of the entry points compares (engine.hip)
uint32_t kmdb_sample_proxy_key(double proxy) {
    if (!(std::fabs(proxy) <= 1.7976931348623157e308)) return SR_KEY_BEST;
    const float f = (float)proxy;
    if (std::isinf(f) || std::isnan(f)) return SR_KEY_BEST;
    return sr_float_key(f);
}
