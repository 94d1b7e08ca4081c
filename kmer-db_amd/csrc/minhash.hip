// minhash.hip — a stand-alone k-mer extractor behind kmdb_minhash_batch_seq_alphabet (include/kmdb_amd.h): no database handle.
//
// Replaces, for a batch of samples, what MinhashConsole::run does per sample on the host (reference src/console_minhash.cpp:19-52):
// the loader's KmerHelper::extract under a MinHashFilter (src/kmer_extract.h:13-97, src/filter.h:28-115) followed by
// KmerHelper::sortAndUnique (:40).  The words are bit for bit those of kmdbh_extract_kmers_alphabet + kmdbh_sort_unique (csrc/host_kmers.cpp)
// and of n2a_extract_kernel (csrc/new2all.hip): symbol codes, canonical choice, widening and hash are restated here, the window [lo, hi)
// comes from kmdbh_minhash_window on the host.
//
//   text     the samples of a piece, each followed by one '\n', in one flat buffer with MH_PAD bytes of '\n' in front and a tail of '\n' up
//            to a whole tile: '\n' is outside every alphabet, so no window crosses a sample, and no kernel checks a bound on the text
//   extract  a workgroup takes a tile of T = 256 * R positions.  It maps the tile's bytes (and the MH_PAD in front) to symbol codes through
//            the alphabet table in LDS, once, with coalesced 16-byte loads; a thread then takes a run of R consecutive positions: it warms up
//            on the k - 1 codes in front of the run and advances the forward word and its reverse complement by ONE symbol per position
//            (two shift / or steps, not a k-step loop), counting the valid symbols since the last invalid one: a position yields a word
//            when that count is at least k.  The hash is computed for those positions only.
//   filter   BEFORE anything is stored — count, scan, write: pass 1 stores the tile's number of kept words and nothing else, an exclusive
//            scan gives every tile its offset and the call the exact total, pass 2 repeats the extraction, ranks its kept words with wave
//            ballots and writes (word, sample) at tile offset + rank.  No atomics, no overflow path, a deterministic order, and every
//            allocation from here on is sized by what is KEPT (at the mode's default fraction 0.01: a hundredth of the positions).
//   sort     two stable radix sorts over the kept words only (by word, then by sample), head flags, scan, compaction: the sorted unique
//            words sample by sample, and the per-sample offsets.
#include "kmdb_amd.h"
#include "kmdb_internal.h"
#include "dev_mem.h"

#include <hip/hip_runtime.h>
#include "prim.h"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <exception>
#include <string>
#include <vector>

namespace {

constexpr uint32_t MH_R = 16;                      // positions per thread (a run)
constexpr uint32_t MH_THREADS = 256;
constexpr uint32_t MH_T = MH_THREADS * MH_R;       // positions per workgroup (a tile)
constexpr uint32_t MH_PAD = 32;                    // bytes of '\n' in front of the text: the warm-up of the first run (k - 1 <= 30) reads them
static_assert(MH_R == 16, "a run is one 16-byte LDS read");

__device__ __forceinline__ uint64_t mh_mix64(uint64_t v) {
    v ^= v >> 33; v *= 0xff51afd7ed558ccdull;
    v ^= v >> 33; v *= 0xc4ceb9fe1a85ec53ull;
    v ^= v >> 33;
    return v;
}

struct MhParams {
    const unsigned char* text;     // MH_PAD + n_tiles * MH_T bytes; position i is text[MH_PAD + i]
    const int8_t* map;             // Alphabet::mapping (alphabet.h:41-58), 256 entries in device memory
    const uint64_t* soff;          // [n_samples + 1] first position of every sample (sample s ends with the '\n' at soff[s + 1] - 1)
    uint32_t n_samples;
    uint32_t k, bits, size, widen;
    int preserve, subsample;
    uint64_t lo, hi;               // kmdbh_minhash_window
    uint64_t seed;                 // 42 ^ ceil(k / 4): the part of the hash that does not depend on the word, folded on the host
    uint64_t word_mask;            // 2^(bits * k) - 1
};

// WRITE == false: tile_cnt[tile] = kept words of the tile.  WRITE == true: (word, sample) of every kept word at tile_off[tile] + rank.
template <bool WRITE>
__global__ __launch_bounds__(MH_THREADS) void mh_extract_kernel(MhParams p, uint32_t* __restrict__ tile_cnt, const uint32_t* __restrict__ tile_off,
                                                                unsigned long long* __restrict__ kmer_out, uint32_t* __restrict__ sid_out) {
    __shared__ int8_t tab[256];
    __shared__ uint4 code4[(MH_PAD + MH_T) / 16];      // symbol codes of the positions [tile0 - MH_PAD, tile0 + MH_T), -1: no symbol
    __shared__ uint32_t wave_cnt[MH_THREADS / 64];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wv = tid >> 6;
    const uint64_t tile0 = (uint64_t)blockIdx.x * MH_T;
    tab[tid] = p.map[tid];
    __syncthreads();
    // (text + tile0 is the byte of position tile0 - MH_PAD: 16-byte aligned, MH_T and MH_PAD being multiples of 16)
    const uint4* __restrict__ src = (const uint4*)(p.text + tile0);
    for (uint32_t w = tid; w < (MH_PAD + MH_T) / 16; w += MH_THREADS) {
        const uint4 v = src[w];
        const uint32_t in[4] = {v.x, v.y, v.z, v.w};
        uint32_t o[4];
#pragma unroll
        for (int q = 0; q < 4; ++q)
            o[q] = (uint32_t)(uint8_t)tab[in[q] & 255u] | ((uint32_t)(uint8_t)tab[(in[q] >> 8) & 255u] << 8) |
                   ((uint32_t)(uint8_t)tab[(in[q] >> 16) & 255u] << 16) | ((uint32_t)(uint8_t)tab[in[q] >> 24] << 24);
        code4[w] = make_uint4(o[0], o[1], o[2], o[3]);
    }
    __syncthreads();
    const int8_t* code = (const int8_t*)code4;
    const uint32_t r0 = MH_PAD + tid * MH_R;           // LDS index of the run's first position
    const uint32_t top = p.bits * (p.k - 1);
    uint64_t fwd = 0, rc = 0;
    uint32_t valid = 0;                                // valid symbols since the last invalid one (a tile is far below 2^32 positions)
    auto step = [&](int c) {
        if (c < 0) { c = 0; valid = 0; } else ++valid;
        fwd = ((fwd << p.bits) | (uint64_t)c) & p.word_mask;
        rc = (rc >> p.bits) | ((uint64_t)(p.size - 1u - (uint32_t)c) << top);         // (kmer_extract.h:73; compared only where the strand is not preserved: nt)
    };
    for (uint32_t j = r0 - (p.k - 1); j < r0; ++j) step(code[j]);                    // warm-up: k - 1 <= MH_PAD - 2
    const uint4 mine4 = code4[r0 / 16];
    const uint32_t cw[4] = {mine4.x, mine4.y, mine4.z, mine4.w};
    unsigned long long kv[WRITE ? MH_R : 1];
    uint32_t rank[WRITE ? MH_R : 1];
    uint32_t mine = 0;                                 // kept words of this wave so far (the same in all its lanes)
#pragma unroll
    for (uint32_t it = 0; it < MH_R; ++it) {
        step((int)(int8_t)((cw[it / 4] >> (8 * (it % 4))) & 255u));
        bool keep = valid >= p.k;
        uint64_t w = 0;
        if (keep) {
            w = (p.preserve || fwd < rc) ? fwd : rc;
            w = (w << p.widen) | (w & ((1ull << p.widen) - 1ull));
            if (p.subsample) {                                                       // MinHashFilter (filter.h:96-115)
                uint64_t a = w * 0x87c37b91114253d5ull;
                a = (a << 31) | (a >> 33);
                a *= 0x4cf5ad432745937full;
                uint64_t h1 = a ^ p.seed, h2 = p.seed;
                h1 += h2; h2 += h1;
                h1 = mh_mix64(h1); h2 = mh_mix64(h2);
                h1 += h2; h2 += h1;
                const uint64_t h = h1 ^ h2;
                keep = h >= p.lo && h < p.hi;
            }
        }
        const unsigned long long bal = __ballot(keep);
        if constexpr (WRITE) {
            kv[it] = w;
            rank[it] = keep ? mine + (uint32_t)__popcll(bal & ((1ull << lane) - 1ull)) : 0xFFFFFFFFu;
        }
        mine += (uint32_t)__popcll(bal);
    }
    if (lane == 0) wave_cnt[wv] = mine;
    __syncthreads();
    if constexpr (!WRITE) {
        if (tid == 0) tile_cnt[blockIdx.x] = wave_cnt[0] + wave_cnt[1] + wave_cnt[2] + wave_cnt[3];
    } else {
    uint64_t base = tile_off[blockIdx.x];
    for (uint32_t w2 = 0; w2 < wv; ++w2) base += wave_cnt[w2];
    // the sample of the run's first position; a kept word further on belongs to a later sample when its position passed that sample's end
    const uint64_t pos0 = tile0 + (uint64_t)tid * MH_R;
    uint32_t s = 0;
    bool searched = false;
#pragma unroll
    for (uint32_t it = 0; it < MH_R; ++it) {
        if (rank[it] == 0xFFFFFFFFu) continue;
        const uint64_t pos = pos0 + it;
        if (!searched) {
            uint32_t a = 0, b = p.n_samples;           // the last sample with soff[s] <= pos (pos < soff[n_samples]: a kept position is a symbol of a sample)
            while (b - a > 1) { const uint32_t mid = (a + b) / 2; if (p.soff[mid] <= pos) a = mid; else b = mid; }
            s = a;
            searched = true;
        } else {
            while (pos >= p.soff[s + 1]) ++s;          // (s + 1 <= n_samples, as above)
        }
        kmer_out[base + rank[it]] = kv[it];            // (base + rank < the scan's total = the size of both arrays)
        sid_out[base + rank[it]] = s;
    }
    }
}

// head of a run of equal (sample, k-mer) among the sorted kept words
__global__ void mh_heads_kernel(const unsigned long long* __restrict__ kmer, const uint32_t* __restrict__ sid, uint64_t n, uint32_t* __restrict__ head) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    head[i] = (i == 0 || sid[i - 1] != sid[i] || kmer[i - 1] != kmer[i]) ? 1u : 0u;
}

__global__ void mh_compact_kernel(const unsigned long long* __restrict__ kmer, const uint32_t* __restrict__ head, const uint32_t* __restrict__ hscan,
                                  uint64_t n, uint64_t* __restrict__ out) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n && head[i]) out[hscan[i]] = kmer[i];
}

// off[s] = number of unique k-mers of the samples before s = scanned heads at the first sorted word of a sample >= s
__global__ void mh_sample_offsets_kernel(const uint32_t* __restrict__ sid, const uint32_t* __restrict__ hscan, uint64_t n, uint32_t n_samples,
                                         uint64_t* __restrict__ off) {
    const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s > n_samples) return;
    uint64_t lo = 0, hi = n;
    while (lo < hi) { const uint64_t mid = (lo + hi) / 2; if (sid[mid] < s) lo = mid + 1; else hi = mid; }
    off[s] = hscan[lo];                            // hscan has n + 1 entries
}


thread_local kmdb_minhash_stats g_stats;
thread_local kmdb_minhash_long_stats g_long;

}  // namespace

// bases per piece (one longer sample still goes alone, up to mh_max_sample()).  At fraction 1 the device holds about 42 bytes per base
// (DESIGN 4), and the kept words of a piece — at most its bases — stay below 2^31, the size rocPRIM's sorts are given as an int here.
static uint64_t mh_budget() {
    if (const char* e = getenv("KMDB_MINHASH_BASES_PER_PIECE")) return std::max<uint64_t>(1, strtoull(e, nullptr, 10));
    return 512ull << 20;
}
// a sample with more bytes of text than this is extracted in sections of at most the budget (mh_long_sample)
static uint64_t mh_max_sample() {
    if (const char* e = getenv("KMDB_MINHASH_MAX_SAMPLE_BASES")) return std::max<uint64_t>(1, strtoull(e, nullptr, 10));
    return 1ull << 30;
}
// the most a piece can hold: its text and the '\n' behind it stay below the 2^31 - 2 positions the 32-bit counts of a piece are good for
constexpr uint64_t MH_PIECE_LIMIT = (1ull << 31) - 2;

extern "C" void kmdb_minhash_geometry(uint32_t* positions_per_thread, uint32_t* positions_per_tile) {
    if (positions_per_thread) *positions_per_thread = MH_R;
    if (positions_per_tile) *positions_per_tile = MH_T;
}

extern "C" void kmdb_kmer_lists_free(kmdb_kmer_lists* lists) {
    if (!lists) return;
    free(lists->offsets);
    free(lists->kmers);
    lists->offsets = nullptr; lists->kmers = nullptr; lists->n_samples = 0;
}

extern "C" int kmdb_minhash_stats_get(kmdb_minhash_stats* out) {
    if (!out) return kmdb_set_error("kmdb_minhash_stats_get: null argument");
    *out = g_stats;
    return 0;
}

extern "C" int kmdb_minhash_long_stats_get(kmdb_minhash_long_stats* out) {
    if (!out) return kmdb_set_error("kmdb_minhash_long_stats_get: null argument");
    *out = g_long;
    return 0;
}

// one piece: the samples [0, n) of the arguments; their unique words are appended to `kmers` (`total` words so far) and off[s + 1] is set
// (with a sink the words stay on the device: the sink reads them there and nothing of the piece's lists is copied to the host).
// A section of a long sample is a piece of one sample (n = 1) with `section` set: the `front_len` <= MH_PAD bytes of the sample in front of
// it go into the pad, so that the warm-up of its first runs sees them; its list goes to section->list, not to the host, the sink or `off`.
struct MhSection { const char* front; size_t front_len; DevBuf<void> list; uint64_t count = 0, scratch = 0; };
static int mh_once(const char* const* seqs, const size_t* seq_lens, size_t n, const MhParams& proto, const int8_t* d_map, hipStream_t st,
                   uint64_t** kmers, uint64_t* total, uint64_t* off, const kmdb_device_lists_sink* sink, MhSection* section = nullptr) {
    std::vector<uint64_t> soff(n + 1, 0);
    for (size_t s = 0; s < n; ++s) soff[s + 1] = soff[s] + seq_lens[s] + 1;        // (the '\n' behind every sample)
    const uint64_t L = soff[n];
    const uint64_t n_tiles = (L + MH_T - 1) / MH_T;
    uint64_t scratch = 0;
    DevBuf<void> d_text, d_soff, d_cnt, d_off, d_kA, d_kB, d_sA, d_sB, d_head, d_hscan, d_uniq, d_uoff, d_tmp;
    DevEvent ev[7];
    for (auto& e : ev) if (e.create()) return 1;
    HIP_TRY(hipEventRecord(ev[0], st));
    const size_t text_bytes = MH_PAD + n_tiles * MH_T;
    DEV_ALLOC_BYTES(d_text, text_bytes); scratch += d_text.bytes();
    DEV_ALLOC_BYTES(d_soff, (n + 1) * 8); scratch += d_soff.bytes();
    DEV_ALLOC_BYTES(d_cnt, (n_tiles + 1) * 4); scratch += d_cnt.bytes();
    DEV_ALLOC_BYTES(d_off, (n_tiles + 1) * 4); scratch += d_off.bytes();
    DEV_ALLOC_BYTES(d_uoff, (n + 1) * 8); scratch += d_uoff.bytes();
    HIP_TRY(hipMemsetAsync(d_text.get(), '\n', text_bytes, st));
    if (section && section->front_len)             // (front_len <= MH_PAD: the bytes end where position 0 begins)
        HIP_TRY(hipMemcpyAsync(static_cast<char*>(d_text.get()) + MH_PAD - section->front_len, section->front, section->front_len, hipMemcpyHostToDevice, st));
    for (size_t s = 0; s < n; ++s)
        if (seq_lens[s]) HIP_TRY(hipMemcpyAsync(static_cast<char*>(d_text.get()) + MH_PAD + soff[s], seqs[s], seq_lens[s], hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d_soff.get(), soff.data(), (n + 1) * 8, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemsetAsync(d_cnt.get(), 0, (n_tiles + 1) * 4, st));
    HIP_TRY(hipEventRecord(ev[1], st));
    MhParams p = proto;
    p.text = static_cast<unsigned char*>(d_text.get()); p.map = d_map; p.soff = static_cast<uint64_t*>(d_soff.get()); p.n_samples = (uint32_t)n;
    // pass 1: the tiles' counts; their scan: every tile's offset and, in the entry behind the last tile, the total
    hipLaunchKernelGGL(mh_extract_kernel<false>, dim3((unsigned)n_tiles), dim3(MH_THREADS), 0, st, p, static_cast<uint32_t*>(d_cnt.get()), (const uint32_t*)nullptr,
                       (unsigned long long*)nullptr, (uint32_t*)nullptr);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(ev[2], st));
    size_t tb0 = 0;
    HIP_TRY(prim::exclusive_sum(nullptr, tb0, static_cast<uint32_t*>(d_cnt.get()), static_cast<uint32_t*>(d_off.get()), n_tiles + 1, st));
    DEV_ALLOC_BYTES(d_tmp, tb0); scratch += d_tmp.bytes();
    HIP_TRY(prim::exclusive_sum(d_tmp.get(), tb0, static_cast<uint32_t*>(d_cnt.get()), static_cast<uint32_t*>(d_off.get()), n_tiles + 1, st));
    uint32_t kept32 = 0;
    HIP_TRY(hipMemcpyAsync(&kept32, static_cast<uint32_t*>(d_off.get()) + n_tiles, 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    const uint64_t kept = kept32;
    if (kept > L) return kmdb_set_error("kmdb_minhash_batch_seq_alphabet: internal error (more kept words than positions)");
    HIP_TRY(hipEventRecord(ev[3], st));
    uint64_t n_unique = 0;
    std::vector<uint64_t> uoff(n + 1, 0);
    if (kept) {
        DEV_ALLOC_BYTES(d_kA, kept * 8); scratch += d_kA.bytes(); DEV_ALLOC_BYTES(d_kB, kept * 8); scratch += d_kB.bytes();
        DEV_ALLOC_BYTES(d_sA, kept * 4); scratch += d_sA.bytes(); DEV_ALLOC_BYTES(d_sB, kept * 4); scratch += d_sB.bytes();
        DEV_ALLOC_BYTES(d_head, (kept + 1) * 4); scratch += d_head.bytes(); DEV_ALLOC_BYTES(d_hscan, (kept + 1) * 4); scratch += d_hscan.bytes();
        unsigned long long *kA = static_cast<unsigned long long*>(d_kA.get()), *kB = static_cast<unsigned long long*>(d_kB.get());
        uint32_t *sA = static_cast<uint32_t*>(d_sA.get()), *sB = static_cast<uint32_t*>(d_sB.get());
        // pass 2: the same extraction, the kept words written at tile offset + rank
        hipLaunchKernelGGL(mh_extract_kernel<true>, dim3((unsigned)n_tiles), dim3(MH_THREADS), 0, st, p, (uint32_t*)nullptr, (const uint32_t*)static_cast<uint32_t*>(d_off.get()), kA, sA);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipEventRecord(ev[4], st));
        const unsigned blocks = (unsigned)((kept + 255) / 256);
        const int kbits = (int)std::min<uint32_t>(64u, p.bits * p.k + p.widen);
        int sbits = 1;
        while (sbits < 32 && (1ull << sbits) < n) ++sbits;          // the sample ids in use: only those bits are sorted
        size_t tb1 = 0, tb2 = 0, tb3 = 0;
        HIP_TRY(prim::sort_pairs(nullptr, tb1, kA, kB, sA, sB, (int)kept, 0, kbits, st));
        HIP_TRY(prim::sort_pairs(nullptr, tb2, sB, sA, kB, kA, (int)kept, 0, sbits, st));
        HIP_TRY(prim::exclusive_sum(nullptr, tb3, static_cast<uint32_t*>(d_head.get()), static_cast<uint32_t*>(d_hscan.get()), (int)(kept + 1), st));
        DevBuf<void> d_tmp2;
        DEV_ALLOC_BYTES(d_tmp2, std::max(tb1, std::max(tb2, tb3))); scratch += d_tmp2.bytes();
        HIP_TRY(prim::sort_pairs(d_tmp2.get(), tb1, kA, kB, sA, sB, (int)kept, 0, kbits, st));
        HIP_TRY(prim::sort_pairs(d_tmp2.get(), tb2, sB, sA, kB, kA, (int)kept, 0, sbits, st));     // stable: the words stay ascending inside a sample
        HIP_TRY(hipEventRecord(ev[5], st));
        HIP_TRY(hipMemsetAsync(d_head.get(), 0, (kept + 1) * 4, st));
        hipLaunchKernelGGL(mh_heads_kernel, dim3(blocks), dim3(256), 0, st, kA, sA, kept, static_cast<uint32_t*>(d_head.get()));
        HIP_TRY(prim::exclusive_sum(d_tmp2.get(), tb3, static_cast<uint32_t*>(d_head.get()), static_cast<uint32_t*>(d_hscan.get()), (int)(kept + 1), st));
        uint32_t nu32 = 0;
        HIP_TRY(hipMemcpyAsync(&nu32, static_cast<uint32_t*>(d_hscan.get()) + kept, 4, hipMemcpyDeviceToHost, st));
        hipLaunchKernelGGL(mh_sample_offsets_kernel, dim3((unsigned)((n + 1 + 255) / 256)), dim3(256), 0, st, sA, static_cast<uint32_t*>(d_hscan.get()), kept, (uint32_t)n,
                           static_cast<uint64_t*>(d_uoff.get()));
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipStreamSynchronize(st));
        n_unique = nu32;
        if (n_unique > kept) return kmdb_set_error("kmdb_minhash_batch_seq_alphabet: internal error (more unique words than kept words)");
        DEV_ALLOC_BYTES(d_uniq, n_unique * 8); scratch += d_uniq.bytes();
        hipLaunchKernelGGL(mh_compact_kernel, dim3(blocks), dim3(256), 0, st, kA, static_cast<uint32_t*>(d_head.get()), static_cast<uint32_t*>(d_hscan.get()), kept, static_cast<uint64_t*>(d_uniq.get()));
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(uoff.data(), d_uoff.get(), (n + 1) * 8, hipMemcpyDeviceToHost, st));
        if (!sink && !section) {
            uint64_t* grown = (uint64_t*)realloc(*kmers, std::max<uint64_t>(1, *total + n_unique) * 8);
            if (!grown) return kmdb_set_error("kmdb_minhash_batch_seq_alphabet: out of host memory");
            *kmers = grown;
            if (n_unique) HIP_TRY(hipMemcpyAsync(grown + *total, d_uniq.get(), n_unique * 8, hipMemcpyDeviceToHost, st));
        }
        HIP_TRY(hipStreamSynchronize(st));
        if (uoff[n] != n_unique) return kmdb_set_error("kmdb_minhash_batch_seq_alphabet: internal error (the sample offsets do not end at the unique count)");
    } else {
        HIP_TRY(hipEventRecord(ev[4], st));
        HIP_TRY(hipEventRecord(ev[5], st));
    }
    HIP_TRY(hipEventRecord(ev[6], st));
    HIP_TRY(hipEventSynchronize(ev[6]));
    if (section) {
        section->list.take(d_uniq);
        section->count = n_unique;
        section->scratch = scratch;
    } else if (sink) {
        // the sorts' double buffers and the flags are done with: the sink's own work gets their memory
        dev_reset(d_kA, d_kB, d_sA, d_sB, d_head, d_hscan, d_text, d_cnt, d_off);
        if (const int rc = (*sink)(static_cast<uint64_t*>(d_uniq.get()), uoff.data(), n, (void*)st)) return rc;
    }
    if (!section) {
        for (size_t s = 0; s < n; ++s) off[s + 1] = *total + uoff[s + 1];
        *total += n_unique;
        g_stats.unique += n_unique;
    }
    float ms[6] = {0, 0, 0, 0, 0, 0};
    for (int i = 0; i < 6; ++i) HIP_TRY(hipEventElapsedTime(&ms[i], ev[i], ev[i + 1]));
    g_stats.pieces += 1; g_stats.bases += L - n; g_stats.kept += kept;
    g_stats.scratch_bytes = std::max<uint64_t>(g_stats.scratch_bytes, scratch);
    g_stats.h2d_ms += ms[0]; g_stats.count_ms += ms[1]; g_stats.scan_ms += ms[2]; g_stats.write_ms += ms[3]; g_stats.sort_ms += ms[4]; g_stats.unique_ms += ms[5];
    return 0;
}

// One sample in consecutive sections of at most the budget, cut wherever the budget falls.  A section owns the k-mers whose LAST symbol lies in
// it — every window of the sample is counted once by its position — and sees the k - 1 symbols in front of its first position in the pad.
// Its sorted unique list stays on the device and is joined into the sample's running list by the merge-union (sorted_union.hip): the words of
// the whole sample are counted with 64 bits, those of a section with 32.  After the last section the list goes where a piece's lists go.
static int mh_long_sample(const char* who, const char* seq, size_t len, const MhParams& proto, const int8_t* d_map, hipStream_t st, uint64_t** kmers,
                          uint64_t* total, uint64_t* off, const kmdb_device_lists_sink* sink) {
    const uint64_t step = std::min<uint64_t>(mh_budget(), MH_PIECE_LIMIT - 1);
    DevBuf<void> d_run;                            // the running list: the union of the sections so far
    uint64_t n_run = 0;
    DevEvent ev[2];
    for (auto& e : ev) if (e.create()) return 1;
    auto peak = [&](uint64_t bytes) { g_long.peak_bytes = std::max<uint64_t>(g_long.peak_bytes, bytes); };
    g_long.long_samples += 1;
    for (uint64_t at = 0; at < len; at += step) {
        MhSection sec;
        const size_t sec_len = (size_t)std::min<uint64_t>(step, len - at);
        const char* text = seq + at;
        sec.front_len = (size_t)std::min<uint64_t>(MH_PAD, at);
        sec.front = text - sec.front_len;
        if (const int rc = mh_once(&text, &sec_len, 1, proto, d_map, st, nullptr, nullptr, nullptr, nullptr, &sec)) return rc;
        g_long.sections += 1;
        peak(d_run.bytes() + sec.scratch);
        if (!n_run) { d_run.take(sec.list); n_run = sec.count; continue; }        // (the first list, or the first that holds a word)
        if (!sec.count) continue;
        DevBuf<void> d_join;
        DEV_ALLOC_BYTES(d_join, (n_run + sec.count) * 8);
        uint64_t n_join = 0, tables = 0;
        HIP_TRY(hipEventRecord(ev[0], st));
        if (const int rc = kmdb_sorted_union_on_stream(who, static_cast<const uint64_t*>(d_run.get()), n_run, static_cast<const uint64_t*>(sec.list.get()), sec.count,
                                                       static_cast<uint64_t*>(d_join.get()), &n_join, (void*)st, &tables)) return rc;
        HIP_TRY(hipEventRecord(ev[1], st));
        HIP_TRY(hipEventSynchronize(ev[1]));
        float ms = 0;
        HIP_TRY(hipEventElapsedTime(&ms, ev[0], ev[1]));
        g_long.union_ms += ms;
        g_long.union_words_in += n_run + sec.count; g_long.union_words_out += n_join;
        g_long.union_bytes += (2 * (n_run + sec.count) + n_join) * 8;               // both inputs read by the count pass and by the write pass, the union written
        peak(d_run.bytes() + sec.list.bytes() + d_join.bytes() + tables);
        d_run.take(d_join);
        n_run = n_join;
    }
    if (sink) {
        const uint64_t one[2] = {0, n_run};
        if (const int rc = (*sink)(static_cast<const uint64_t*>(d_run.get()), one, 1, (void*)st)) return rc;
    } else {
        uint64_t* grown = (uint64_t*)realloc(*kmers, std::max<uint64_t>(1, *total + n_run) * 8);
        if (!grown) return kmdb_set_error(std::string(who) + ": out of host memory");
        *kmers = grown;
        if (n_run) HIP_TRY(hipMemcpyAsync(grown + *total, d_run.get(), n_run * 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
    }
    off[1] = *total + n_run;
    *total += n_run;
    g_stats.unique += n_run;
    return 0;
}

// out: the lists on the host (the public entry); sink: the lists on the device, piece by piece (kmdb_minhash_device_lists) — one of the two
static int mh_batch(const char* who, const char* const* seqs, const size_t* seq_lens, size_t n_samples, uint32_t k, double fraction, double start_fraction,
                    int32_t alphabet, kmdb_kmer_lists* out, const kmdb_opts* opts, const kmdb_device_lists_sink* sink) {
    if ((!out && !sink) || (n_samples && (!seqs || !seq_lens))) return kmdb_set_error(std::string(who) + ": null argument");
    if (out) { out->n_samples = 0; out->offsets = nullptr; out->kmers = nullptr; }
    if (alphabet < 0 || alphabet >= KMDB_ALPHABET_COUNT) return kmdb_set_error(std::string(who) + ": unknown alphabet " + std::to_string(alphabet));
    if (opts && opts->abi_version && !kmdb_abi_compatible(opts->abi_version)) return kmdb_set_error(std::string(who) + ": kmdb_opts.abi_version is not served by this library");
    int8_t map[256];
    MhParams p{};
    if (kmdbh_alphabet_table(alphabet, map, &p.size, &p.bits, &p.preserve)) return kmdb_set_error(std::string(who) + ": unknown alphabet");
    if (k == 0 || k > 64u / p.bits - 1u) return kmdb_set_error(std::string(who) + ": k-mer length must be 1.." + std::to_string(64u / p.bits - 1u) + " for this alphabet (alphabet.h:37)");
    static_assert(MH_PAD >= 32, "the warm-up of a run reads k - 1 <= 30 codes in front of it");
    if (n_samples >= (1ull << 31)) return kmdb_set_error(std::string(who) + ": too many samples in one batch");
    for (size_t s = 0; s < n_samples; ++s) {
        if (seq_lens[s] && !seqs[s]) return kmdb_set_error(std::string(who) + ": null argument");
    }
    g_stats = kmdb_minhash_stats{};
    g_long = kmdb_minhash_long_stats{};
    uint64_t* offsets = (uint64_t*)calloc(n_samples + 1, 8);
    if (!offsets) return kmdb_set_error(std::string(who) + ": out of host memory");
    uint64_t* kmers = nullptr;
    uint64_t total = 0;
    struct Guard { uint64_t*& a; uint64_t*& b; bool armed = true; ~Guard() { if (armed) { free(a); free(b); } } } guard{offsets, kmers};
    if (n_samples) {
        const int prefix_bits = (int)(p.bits * k) - 32;
        p.k = k;
        p.widen = prefix_bits < 8 ? (uint32_t)(8 - prefix_bits) : 0u;
        p.subsample = fraction < 1.0;
        kmdbh_minhash_window(fraction, start_fraction, &p.lo, &p.hi);               // src/filter.h:38-51; the host's one definition (host_kmers.cpp)
        p.seed = 42ull ^ (uint64_t)std::ceil((double)k / 4.0);
        p.word_mask = (1ull << (p.bits * k)) - 1ull;                                // (bits * k <= 63)
        HIP_TRY(hipSetDevice(opts ? opts->device : 0));
        hipStream_t st = (opts && opts->stream) ? (hipStream_t)opts->stream : (hipStream_t) nullptr;
        DevBuf<void> d_map;
        DEV_ALLOC_BYTES(d_map, 256);
        HIP_TRY(hipMemcpyAsync(d_map.get(), map, 256, hipMemcpyHostToDevice, st));
        HIP_TRY(hipStreamSynchronize(st));                                           // (`map` lives on this frame)
        // samples are independent: cut the batch where the accumulated bases pass the budget; a long sample is cut itself, the pieces around it
        // are made as if it were a batch's end
        const uint64_t budget = mh_budget(), max_sample = mh_max_sample();
        auto is_long = [&](size_t s) { return seq_lens[s] > max_sample || seq_lens[s] >= MH_PIECE_LIMIT; };
        for (size_t s0 = 0; s0 < n_samples;) {
            if (is_long(s0)) {
                if (const int rc = mh_long_sample(who, seqs[s0], seq_lens[s0], p, static_cast<int8_t*>(d_map.get()), st, &kmers, &total, offsets + s0, sink)) return rc;
                ++s0;
                continue;
            }
            size_t s1 = s0;
            uint64_t bases = 0;
            do { bases += seq_lens[s1] + 1; ++s1; } while (s1 < n_samples && !is_long(s1) && bases + seq_lens[s1] + 1 <= budget && bases + seq_lens[s1] + 1 < MH_PIECE_LIMIT);
            if (const int rc = mh_once(seqs + s0, seq_lens + s0, s1 - s0, p, static_cast<int8_t*>(d_map.get()), st, &kmers, &total, offsets + s0, sink)) return rc;
            s0 = s1;
        }
    }
    if (sink) return 0;                            // (the guard frees the offsets; no words came to the host)
    if (!kmers) kmers = (uint64_t*)malloc(8);
    if (!kmers) return kmdb_set_error(std::string(who) + ": out of host memory");
    guard.armed = false;
    out->n_samples = n_samples; out->offsets = offsets; out->kmers = kmers;
    return 0;
}

extern "C" int kmdb_minhash_batch_seq_alphabet(const char* const* seqs, const size_t* seq_lens, size_t n_samples, uint32_t kmer_length, double fraction,
                                               double start_fraction, int32_t alphabet, kmdb_kmer_lists* out, const kmdb_opts* opts) {
    try {
        return mh_batch("kmdb_minhash_batch_seq_alphabet", seqs, seq_lens, n_samples, kmer_length, fraction, start_fraction, alphabet, out, opts, nullptr);
    } catch (const std::exception& e) {
        return kmdb_set_error(std::string("kmdb_minhash_batch_seq_alphabet: ") + e.what());
    }
}

int kmdb_minhash_device_lists(const char* who, const char* const* seqs, const size_t* seq_lens, size_t n_samples, uint32_t kmer_length, double fraction,
                              double start_fraction, int32_t alphabet, const kmdb_opts* opts, const kmdb_device_lists_sink& sink) {
    return mh_batch(who, seqs, seq_lens, n_samples, kmer_length, fraction, start_fraction, alphabet, nullptr, opts, &sink);
}
