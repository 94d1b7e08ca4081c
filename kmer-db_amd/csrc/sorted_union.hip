// sorted_union.hip — A ∪ B of two strictly ascending arrays of 64-bit words in device memory (kmdb_sorted_union_device, include/kmdb_amd.h).
//
// What joins the sorted unique lists of the sections of a long sample (minhash.hip): no sort — rocPRIM's sizes are ints here and the list of a
// genome passes 2^31 words — but a merge, and every index that counts words of a whole array is 64 bits wide.
//
//   merged order  the words of A and B in ascending order, a word of A in front of an equal word of B.  A word of B is a duplicate exactly
//                 when the last word of A in front of it equals it (A ascends strictly: no earlier word of A can): one look at A[i - 1].
//   partition     the merged order is cut into tiles of UN_T words.  un_partition_kernel finds, once per tile border and with one binary search
//                 (the merge path), how many words of A lie in front of the border; both passes below read that table.
//   count, scan,  a workgroup loads its stretch of A and of B into LDS with coalesced loads, a thread finds the start of its UN_R merged words
//   write         with one search in LDS and merges them from there: pass 1 stores the tile's number of kept words, a 64-bit exclusive scan gives
//                 every tile its offset and the call its total, pass 2 repeats the merge, ranks the kept words inside the tile, stages them in
//                 LDS in output order and writes them out coalesced.  Each pass reads both inputs once; the union is written once.
//   bounds        every index is clamped to its array whatever the words are: input that does not ascend gives words in an unspecified order
//                 (both passes still agree on the counts — they run the same code on the same words), never an access outside A, B or
//                 out[0, na + nb).
#include "kmdb_amd.h"
#include "kmdb_internal.h"
#include "dev_mem.h"

#include <hip/hip_runtime.h>
#include "prim.h"

#include <algorithm>
#include <exception>
#include <string>

namespace {

constexpr uint32_t UN_R = 8;                       // merged words per thread
constexpr uint32_t UN_THREADS = 256;
constexpr uint32_t UN_T = UN_THREADS * UN_R;       // merged words per workgroup (a tile): 16 KiB of LDS

// words of A in front of diagonal d of the merged order (d words in front of it): the least i with A[i] > B[d - 1 - i], searched in
// [max(0, d - nb), min(d, na)] — inside both arrays for any words
__device__ __forceinline__ uint64_t un_merge_path(const unsigned long long* __restrict__ A, uint64_t na, const unsigned long long* __restrict__ B, uint64_t nb, uint64_t d) {
    uint64_t lo = d > nb ? d - nb : 0, hi = d < na ? d : na;
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo) / 2;   // mid < hi <= na; d - 1 - mid: >= 0 as mid < d, < nb as mid >= lo >= d - nb
        if (A[mid] <= B[d - 1 - mid]) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// split[t] = words of A in front of tile t, t = 0 .. n_tiles (the entry behind the last tile is na)
__global__ void un_partition_kernel(const unsigned long long* __restrict__ A, uint64_t na, const unsigned long long* __restrict__ B, uint64_t nb, uint64_t n_tiles,
                                    uint64_t* __restrict__ split) {
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t > n_tiles) return;
    split[t] = un_merge_path(A, na, B, nb, std::min<uint64_t>(t * UN_T, na + nb));
}

// WRITE == false: tile_cnt[tile] = kept words of the tile.  WRITE == true: the kept words at out[tile_off[tile] ..), ascending.
template <bool WRITE>
__global__ __launch_bounds__(UN_THREADS) void un_merge_kernel(const unsigned long long* __restrict__ A, uint64_t na, const unsigned long long* __restrict__ B, uint64_t nb,
                                                              const uint64_t* __restrict__ split, uint64_t* __restrict__ tile_cnt, const uint64_t* __restrict__ tile_off,
                                                              unsigned long long* __restrict__ out) {
    __shared__ unsigned long long words[UN_T];     // the tile's words of A, then its words of B; in the write pass then the kept words in output order
    __shared__ uint32_t wave_cnt[UN_THREADS / 64];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wv = tid >> 6;
    const uint64_t n = na + nb;
    const uint64_t d0 = (uint64_t)blockIdx.x * UN_T;
    const uint32_t len = (uint32_t)std::min<uint64_t>(UN_T, n - d0);                 // (the grid has ceil(n / UN_T) tiles: d0 < n)
    // the tile's stretch of A, clamped so that both stretches lie inside their arrays and hold `len` words together whatever the table says
    const uint64_t i0 = std::min<uint64_t>(split[blockIdx.x], std::min<uint64_t>(na, d0));      // j0 = d0 - i0 >= 0
    uint64_t i_lo = d0 + len > nb ? d0 + len - nb : 0;                               // at least this many words of A in front of the tile's end
    uint64_t i1 = std::min<uint64_t>(std::max<uint64_t>(split[blockIdx.x + 1], std::max<uint64_t>(i0, i_lo)), std::min<uint64_t>(i0 + len, na));
    if (i1 < i_lo) i1 = i_lo;                      // (only where i0 itself lies below the search range of its diagonal: never for a table un_partition_kernel wrote)
    const uint64_t j0 = std::min<uint64_t>(d0 - i0, nb);
    const uint32_t nat = (uint32_t)std::min<uint64_t>(i1 > i0 ? i1 - i0 : 0, len);
    const uint32_t nbt = (uint32_t)std::min<uint64_t>(len - nat, nb - j0);
    for (uint32_t x = tid; x < nat; x += UN_THREADS) words[x] = A[i0 + x];           // (i0 + nat <= na)
    for (uint32_t x = tid; x < nbt; x += UN_THREADS) words[nat + x] = B[j0 + x];     // (j0 + nbt <= nb)
    __syncthreads();
    const unsigned long long* sa = words;
    const unsigned long long* sb = words + nat;
    // the thread's diagonal inside the tile, and its words of A in front of it (the merge path again, in LDS)
    const uint32_t total = nat + nbt;
    const uint32_t d = std::min<uint32_t>(tid * UN_R, total);
    uint32_t lo = d > nbt ? d - nbt : 0, hi = d < nat ? d : nat;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) / 2;
        if (sa[mid] <= sb[d - 1 - mid]) lo = mid + 1; else hi = mid;
    }
    uint32_t ai = lo, bi = d - lo;
    // the last word of A in front of the thread's first word: in the tile, or the one in front of the tile
    bool have_last = false;
    unsigned long long last = 0;
    if (ai > 0) { last = sa[ai - 1]; have_last = true; }
    else if (i0 > 0) { last = A[i0 - 1]; have_last = true; }
    unsigned long long kv[WRITE ? UN_R : 1];
    uint32_t keep_mask = 0, mine = 0;
#pragma unroll
    for (uint32_t it = 0; it < UN_R; ++it) {
        const bool has_a = ai < nat, has_b = bi < nbt;
        if (d + it < total && (has_a || has_b)) {
            const unsigned long long a = has_a ? sa[ai] : 0ull, b = has_b ? sb[bi] : 0ull;
            const bool take_a = has_a && (!has_b || a <= b);                         // unsigned: alphabets that widen their words set the top bit
            bool keep = true;
            if (take_a) { last = a; have_last = true; ++ai; }
            else { keep = !(have_last && last == b); ++bi; }
            if constexpr (WRITE) kv[it] = take_a ? a : b;
            if (keep) { keep_mask |= 1u << it; ++mine; }
        }
    }
    // rank of the thread's first kept word inside the tile: prefix over the wave's lanes, then over the waves
    uint32_t incl = mine;
#pragma unroll
    for (uint32_t s = 1; s < 64; s <<= 1) {
        const uint32_t v = __shfl_up(incl, s, 64);
        if (lane >= s) incl += v;
    }
    if (lane == 63) wave_cnt[wv] = incl;
    __syncthreads();                               // (also: every thread has taken its words out of `words`)
    uint32_t tile_total = 0, base = 0;
#pragma unroll
    for (uint32_t w = 0; w < UN_THREADS / 64; ++w) { if (w < wv) base += wave_cnt[w]; tile_total += wave_cnt[w]; }
    if constexpr (!WRITE) {
        if (tid == 0) tile_cnt[blockIdx.x] = tile_total;
    } else {
        uint32_t r = base + incl - mine;
#pragma unroll
        for (uint32_t it = 0; it < UN_R; ++it)
            if (keep_mask & (1u << it)) words[r++] = kv[it];                          // (r < tile_total <= total <= UN_T)
        __syncthreads();
        const uint64_t o0 = tile_off[blockIdx.x];                                    // (o0 + tile_total <= the scan's total <= na + nb)
        for (uint32_t x = tid; x < tile_total; x += UN_THREADS) out[o0 + x] = words[x];
    }
}

}  // namespace

extern "C" void kmdb_sorted_union_geometry(uint32_t* words_per_thread, uint32_t* words_per_tile) {
    if (words_per_thread) *words_per_thread = UN_R;
    if (words_per_tile) *words_per_tile = UN_T;
}

int kmdb_sorted_union_on_stream(const char* who, const uint64_t* a, uint64_t na, const uint64_t* b, uint64_t nb, uint64_t* out, uint64_t* n_out, void* stream,
                                uint64_t* scratch_bytes) {
    hipStream_t st = (hipStream_t)stream;
    *n_out = 0;
    if (scratch_bytes) *scratch_bytes = 0;
    const uint64_t n = na + nb;
    if (!n) return 0;
    const uint64_t n_tiles = (n + UN_T - 1) / UN_T;
    if (n_tiles >= (1ull << 31)) return kmdb_set_error(std::string(who) + ": 2^42 words or more");
    DevBuf<uint64_t> d_split, d_cnt, d_off;
    DevBuf<void> d_tmp;
    DEV_ALLOC(d_split, n_tiles + 1); DEV_ALLOC(d_cnt, n_tiles + 1); DEV_ALLOC(d_off, n_tiles + 1);
    const unsigned long long *A = (const unsigned long long*)a, *B = (const unsigned long long*)b;
    HIP_TRY(hipMemsetAsync(d_cnt.get(), 0, (n_tiles + 1) * 8, st));
    hipLaunchKernelGGL(un_partition_kernel, dim3((unsigned)((n_tiles + 1 + 255) / 256)), dim3(256), 0, st, A, na, B, nb, n_tiles, d_split.get());
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(un_merge_kernel<false>, dim3((unsigned)n_tiles), dim3(UN_THREADS), 0, st, A, na, B, nb, (const uint64_t*)d_split.get(), d_cnt.get(), (const uint64_t*)nullptr,
                       (unsigned long long*)nullptr);
    HIP_TRY(hipGetLastError());
    size_t tb = 0;
    HIP_TRY(prim::exclusive_sum(nullptr, tb, d_cnt.get(), d_off.get(), n_tiles + 1, st));
    DEV_ALLOC_BYTES(d_tmp, tb);
    HIP_TRY(prim::exclusive_sum(d_tmp.get(), tb, d_cnt.get(), d_off.get(), n_tiles + 1, st));
    uint64_t total = 0;
    HIP_TRY(hipMemcpyAsync(&total, d_off.get() + n_tiles, 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (total > n) return kmdb_set_error(std::string(who) + ": internal error (more words in the union than in its inputs)");
    hipLaunchKernelGGL(un_merge_kernel<true>, dim3((unsigned)n_tiles), dim3(UN_THREADS), 0, st, A, na, B, nb, (const uint64_t*)d_split.get(), (uint64_t*)nullptr,
                       (const uint64_t*)d_off.get(), (unsigned long long*)out);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(st));             // (the tables above are freed on return)
    *n_out = total;
    if (scratch_bytes) *scratch_bytes = d_split.bytes() + d_cnt.bytes() + d_off.bytes() + d_tmp.bytes();
    return 0;
}

extern "C" int kmdb_sorted_union_device(const void* a_dev, uint64_t na, const void* b_dev, uint64_t nb, void* out_dev, uint64_t out_cap, uint64_t* n_out,
                                        const kmdb_opts* opts) {
    const char* who = "kmdb_sorted_union_device";
    try {
        if (!n_out) return kmdb_set_error(std::string(who) + ": null argument");
        *n_out = 0;
        if (opts && opts->abi_version && !kmdb_abi_compatible(opts->abi_version)) return kmdb_set_error(std::string(who) + ": kmdb_opts.abi_version is not served by this library");
        if ((na && !a_dev) || (nb && !b_dev)) return kmdb_set_error(std::string(who) + ": a null array with a size that is not 0");
        if (na > ~0ull - nb || out_cap < na + nb)
            return kmdb_set_error(std::string(who) + ": the output holds " + std::to_string(out_cap) + " words, fewer than the " + std::to_string(na) + " + " + std::to_string(nb) +
                                  " of the inputs (the capacity must cover the case of no common word)");
        if (na + nb && !out_dev) return kmdb_set_error(std::string(who) + ": a null array with a size that is not 0");
        HIP_TRY(hipSetDevice(opts ? opts->device : 0));
        return kmdb_sorted_union_on_stream(who, (const uint64_t*)a_dev, na, (const uint64_t*)b_dev, nb, (uint64_t*)out_dev, n_out, opts ? opts->stream : nullptr, nullptr);
    } catch (const std::exception& e) {
        return kmdb_set_error(std::string(who) + ": " + e.what());
    }
}
