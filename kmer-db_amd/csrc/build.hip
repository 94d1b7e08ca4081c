// build.hip — the build mode: the state of PrefixKmerDb grown on the device (kmdb_build_* in include/kmdb_amd.h).
//
// Replaces db.addKmers per sample (reference src/console_build.cpp:111; src/prefix_kmer_db.cpp:244-434, its two workers :67-240) and what
// serialize reads out of the live object (:438-574).  The pattern ids are those of the reference run with ONE thread: one pattern task
// walks the sample's k-mers grouped by ascending old pattern id and hands out new ids in that order (:198-233).
//
//   state    D     the sorted dictionary of all distinct k-mers seen, and cur[i] = the pattern id of D[i] (0: none yet) — the reference's
//                  hashtables, kept as one sorted array while the tree grows
//            here / num_samples / parent / is_parent per pattern (pattern_t, pattern.h:42-53); pattern 0 is the empty pattern (:24)
//            events (pattern, sample): "the sample was appended to the pattern's local ids" (pattern_t::expand and the constructor :106-114)
//   a call   (a) the call's k-mers are sorted together; those that start a run and are not in D are the new ones; D and the new ones are
//                merged in ONE pass (every element finds its place by a binary search in the other list), old entries keep their cur
//            (b) per sample, in input order, a fixed chain of kernels with no host decision between them: position and pattern of every
//                k-mer; radix sort of (pattern, position) by pattern; head flags, their scan and the group starts; per group: extend in place
//                iff the group takes every k-mer of a childless pattern (:210), else a new pattern whose id is P + the group's rank among
//                the sample's new groups; the k-mers of new groups get the new id.  A pattern is in at most one group of a sample, so a
//                group's thread owns its pattern and its new pattern: no atomics.  The pattern and event cursors stay on the device, one
//                pair per sample of the call; capacity is reserved per call from new patterns <= groups <= k-mers of the sample.
//   finish   (c) events sorted by pattern (stable: a pattern's samples stay ascending); one thread per EVENT computes the length of its
//                gamma code and later writes it (elias_gamma.h; MSB first in little-endian 64-bit words, two words when it straddles) — no
//                thread loops over a pattern's list; a scan of the lengths gives every code its bit and every pattern its num_bits
//            (d) prefix-bucket tables from (D, cur): bucket = kmer >> 32 is a contiguous stretch of D; capacity = the least power of two
//                >= 16 that keeps the fill at or below 0.8 (hashmap_lp.h:420-437); home slot and probing as csrc/hash_probe.h reads them;
//                placement by 64-bit atomic minimum: linear probing with priorities, one table whatever the order of arrival
//            (e) everything copied into a kmdbh_db
//   hand-off     kmdb_build_finish_device: (c), (d) only if somebody reads the tables, then the engine's layout straight from these arrays
//                (kmdb_db_from_device -> kmdb_layout_from_device, layout.hip), (e) only for a full host image
//   seed     (f) kmdb_build_begin_from_db: the reverse of (c) - (e), a stored database loaded into the state above (bd_seed, further down)
// Wave-64, 256 threads per block, one element per thread; every kernel checks its own bounds and no kernel uses scratch (the compile's
// resource remarks are read by tests/test_build.py).
#include "kmdb_amd.h"
#include "kmdb_internal.h"

#include <hip/hip_runtime.h>
#include "hash_probe.h"
#include "prim.h"
#include "device_common.h"
#include "dev_mem.h"
#include "engine_internal.h"

#include <algorithm>
#include <chrono>
#include <cstdlib>
#include <cstring>
#include <exception>
#include <string>
#include <vector>

namespace {

constexpr uint32_t BD_THREADS = 256;
constexpr uint64_t BD_EMPTY = (uint64_t)0x7fffffffu << 32;      // key 0, val INT32_MAX (hashmap_lp.h:78)
constexpr uint64_t BD_PIECE_KMERS = 1ull << 30;                 // k-mers of a piece of a call (one longer sample goes alone): the sorts take 31-bit sizes
constexpr size_t BD_PIECE_SAMPLES = 1024;                       // non-empty samples of a piece: four timing events each

__device__ __forceinline__ uint64_t bd_lower_bound(const uint64_t* __restrict__ a, uint64_t n, uint64_t x) {
    uint64_t lo = 0, hi = n;
    while (lo < hi) { const uint64_t mid = (lo + hi) / 2; if (a[mid] < x) lo = mid + 1; else hi = mid; }
    return lo;
}

// bad = the first sample with two neighbours out of strictly ascending order (0xFFFFFFFF: none)
__global__ __launch_bounds__(BD_THREADS) void bd_check_kernel(const uint64_t* __restrict__ K, uint64_t T, const uint64_t* __restrict__ off, uint32_t n,
                                                              uint32_t* __restrict__ bad) {
    const uint64_t i = (uint64_t)blockIdx.x * BD_THREADS + threadIdx.x;
    if (i == 0 || i >= T || K[i - 1] < K[i]) return;
    uint32_t a = 0, b = n;                             // the last sample with off[s] <= i (off[0] = 0)
    while (b - a > 1) { const uint32_t mid = (a + b) / 2; if (off[mid] <= i) a = mid; else b = mid; }
    if (off[a] != i) atomicMin(bad, a);                // (i is not the first k-mer of its sample)
}

// flag[i] = S[i] starts a run of equal k-mers of the sorted call AND is not in the dictionary
__global__ __launch_bounds__(BD_THREADS) void bd_flag_new_kernel(const uint64_t* __restrict__ S, uint64_t T, const uint64_t* __restrict__ D, uint64_t nD,
                                                                 uint32_t* __restrict__ flag) {
    const uint64_t i = (uint64_t)blockIdx.x * BD_THREADS + threadIdx.x;
    if (i >= T) return;
    const uint64_t x = S[i];
    uint32_t f = 0;
    if (i == 0 || S[i - 1] != x) {
        const uint64_t pos = bd_lower_bound(D, nD, x);
        f = (pos == nD || D[pos] != x) ? 1u : 0u;
    }
    flag[i] = f;
}

__global__ __launch_bounds__(BD_THREADS) void bd_compact_kernel(const uint64_t* __restrict__ S, const uint32_t* __restrict__ flag, const uint32_t* __restrict__ fscan,
                                                                uint64_t T, uint64_t nN, uint64_t* __restrict__ out) {
    const uint64_t i = (uint64_t)blockIdx.x * BD_THREADS + threadIdx.x;
    if (i < T && flag[i] && fscan[i] < nN) out[fscan[i]] = S[i];
}

// the merge: D and the new k-mers are disjoint, so an element's place is its own index plus the number of smaller elements of the other list
__global__ __launch_bounds__(BD_THREADS) void bd_merge_old_kernel(const uint64_t* __restrict__ D, const uint32_t* __restrict__ cur, uint64_t nD,
                                                                  const uint64_t* __restrict__ Nw, uint64_t nN, uint64_t* __restrict__ D2, uint32_t* __restrict__ cur2) {
    const uint64_t i = (uint64_t)blockIdx.x * BD_THREADS + threadIdx.x;
    if (i >= nD) return;
    const uint64_t x = D[i], pos = i + bd_lower_bound(Nw, nN, x);           // (< nD + nN)
    D2[pos] = x;
    cur2[pos] = cur[i];
}
__global__ __launch_bounds__(BD_THREADS) void bd_merge_new_kernel(const uint64_t* __restrict__ Nw, uint64_t nN, const uint64_t* __restrict__ D, uint64_t nD,
                                                                  uint64_t* __restrict__ D2, uint32_t* __restrict__ cur2) {
    const uint64_t j = (uint64_t)blockIdx.x * BD_THREADS + threadIdx.x;
    if (j >= nN) return;
    const uint64_t x = Nw[j], pos = j + bd_lower_bound(D, nD, x);
    D2[pos] = x;
    cur2[pos] = 0;
}

// (b) 1: every k-mer of the sample is in D by now
__global__ __launch_bounds__(BD_THREADS) void bd_lookup_kernel(const uint64_t* __restrict__ K, uint32_t c, const uint64_t* __restrict__ D, uint64_t nD,
                                                               const uint32_t* __restrict__ cur, uint32_t* __restrict__ pid, uint32_t* __restrict__ slot) {
    const uint32_t i = blockIdx.x * BD_THREADS + threadIdx.x;
    if (i >= c) return;
    uint64_t s = bd_lower_bound(D, nD, K[i]);
    if (s >= nD) s = nD - 1;                           // (cannot happen after the merge; keeps the read inside D)
    slot[i] = (uint32_t)s;
    pid[i] = cur[s];
}

// (b) 3: head[i], i <= c (head[c] = 0: the scans run over c + 1 entries)
__global__ __launch_bounds__(BD_THREADS) void bd_heads_kernel(const uint32_t* __restrict__ pid, uint32_t c, uint32_t* __restrict__ head) {
    const uint32_t i = blockIdx.x * BD_THREADS + threadIdx.x;
    if (i > c) return;
    head[i] = (i < c && (i == 0 || pid[i - 1] != pid[i])) ? 1u : 0u;
}
// gstart[g] = first element of group g, gstart[G] = c; G = hscan[c]
__global__ __launch_bounds__(BD_THREADS) void bd_group_starts_kernel(const uint32_t* __restrict__ head, const uint32_t* __restrict__ hscan, uint32_t c,
                                                                     uint32_t* __restrict__ gstart) {
    const uint32_t i = blockIdx.x * BD_THREADS + threadIdx.x;
    if (i > c) return;
    if (i == c || head[i]) gstart[hscan[i]] = i;       // (hscan[i] <= i <= c)
}

struct BdTree {
    long long* here;               // k-mers AT the pattern (pattern_t::num_kmers)
    uint32_t* nsam;
    long long* parent;
    uint32_t* isp;
    uint64_t cap;                  // patterns the arrays hold
    uint32_t* ev_pid;
    uint32_t* ev_sid;
    uint64_t ev_cap;
    uint64_t* curs;                // [2 * (samples of the piece + 1)]: pattern count and event count BEFORE the j-th non-empty sample
    uint32_t* overflow;            // set when a reserved capacity would be passed (a bug: the reservations are upper bounds)
};

// (b) 4: isnew[g] for g < G, 0 up to c
__global__ __launch_bounds__(BD_THREADS) void bd_decide_kernel(const uint32_t* __restrict__ pid, const uint32_t* __restrict__ gstart, const uint32_t* __restrict__ hscan,
                                                               uint32_t c, BdTree t, uint32_t* __restrict__ isnew) {
    const uint32_t g = blockIdx.x * BD_THREADS + threadIdx.x;
    if (g > c) return;
    uint32_t v = 0;
    if (g < hscan[c]) {
        const uint32_t p = pid[gstart[g]], cnt = gstart[g + 1] - gstart[g];
        const bool extend = p != 0 && t.here[p] == (long long)cnt && !t.isp[p];       // prefix_kmer_db.cpp:210
        v = extend ? 0u : 1u;
    }
    isnew[g] = v;
}

// (b) 4 / 5: one thread per group
__global__ __launch_bounds__(BD_THREADS) void bd_apply_kernel(const uint32_t* __restrict__ pid, const uint32_t* __restrict__ gstart, const uint32_t* __restrict__ hscan,
                                                              const uint32_t* __restrict__ isnew, const uint32_t* __restrict__ nrank, uint32_t c, BdTree t,
                                                              uint32_t j, uint32_t sample) {
    const uint32_t g = blockIdx.x * BD_THREADS + threadIdx.x;
    const uint32_t G = hscan[c];
    if (g >= G) return;
    const uint64_t P0 = t.curs[2 * j], E0 = t.curs[2 * j + 1];
    const uint32_t n_new = nrank[c];                   // (isnew is 0 from G on)
    if (P0 + n_new > t.cap || E0 + G > t.ev_cap) { *t.overflow = 1; return; }
    const uint32_t p = pid[gstart[g]], cnt = gstart[g + 1] - gstart[g];
    uint32_t id = p;
    if (!isnew[g]) {
        t.nsam[p] += 1;                                // pattern_t::expand (:210-215)
    } else {
        id = (uint32_t)P0 + nrank[g];                  // :216-231, pattern.h:106-114
        const uint32_t ns = t.nsam[p];
        t.nsam[id] = ns + 1;
        t.parent[id] = ns > 0 ? (long long)p : -1ll;
        if (ns > 0) t.isp[p] = 1;
        t.isp[id] = 0;
        t.here[id] = cnt;
        if (p) t.here[p] -= cnt;
    }
    t.ev_pid[E0 + g] = id;
    t.ev_sid[E0 + g] = sample;
    if (g == G - 1) { t.curs[2 * (j + 1)] = P0 + n_new; t.curs[2 * (j + 1) + 1] = E0 + G; }
}

// (b) 5, last line: the k-mers of new groups point at the new pattern
__global__ __launch_bounds__(BD_THREADS) void bd_setcur_kernel(const uint32_t* __restrict__ slot, const uint32_t* __restrict__ head, const uint32_t* __restrict__ hscan,
                                                               const uint32_t* __restrict__ isnew, const uint32_t* __restrict__ nrank, uint32_t c, BdTree t, uint32_t j,
                                                               uint32_t* __restrict__ cur, uint64_t nD) {
    const uint32_t i = blockIdx.x * BD_THREADS + threadIdx.x;
    if (i >= c || *t.overflow) return;
    const uint32_t g = hscan[i] + head[i] - 1u;        // (head[0] = 1)
    if (isnew[g] && slot[i] < nD) cur[slot[i]] = (uint32_t)t.curs[2 * j] + nrank[g];
}

// (c) length of the event's gamma code: 0 for the first id of a pattern (it is not coded, pattern.h:195-203), else 2 L - 1, L = bits of the delta
__global__ __launch_bounds__(BD_THREADS) void bd_code_len_kernel(const uint32_t* __restrict__ spid, const uint32_t* __restrict__ ssid, uint64_t E,
                                                                 unsigned long long* __restrict__ clen) {
    const uint64_t i = (uint64_t)blockIdx.x * BD_THREADS + threadIdx.x;
    if (i > E) return;
    unsigned long long v = 0;
    if (i < E && i > 0 && spid[i - 1] == spid[i]) {
        const uint32_t d = ssid[i] - ssid[i - 1];      // >= 1: a pattern's samples ascend
        if (d) v = 2ull * (32u - (uint32_t)__clz((int)d)) - 1ull;
    }
    clen[i] = v;
}

// per pattern: its stretch [lo, hi) of the sorted events -> num_local, last id, num_bits, words of the padded stream, first bit of its codes
__global__ __launch_bounds__(BD_THREADS) void bd_pattern_fields_kernel(const uint32_t* __restrict__ spid, const uint32_t* __restrict__ ssid, uint64_t E,
                                                                       const unsigned long long* __restrict__ bitpos, uint64_t P, uint32_t* __restrict__ num_local,
                                                                       uint32_t* __restrict__ last_id, uint32_t* __restrict__ num_bits, unsigned long long* __restrict__ words,
                                                                       unsigned long long* __restrict__ pbit0, uint32_t* __restrict__ too_long) {
    const uint64_t p = (uint64_t)blockIdx.x * BD_THREADS + threadIdx.x;
    if (p > P) return;
    if (p == P) { words[P] = 0; return; }
    uint64_t lo = 0, hi = E;
    while (lo < hi) { const uint64_t mid = (lo + hi) / 2; if (spid[mid] < p) lo = mid + 1; else hi = mid; }
    uint64_t e = lo, hi2 = E;
    while (e < hi2) { const uint64_t mid = (e + hi2) / 2; if (spid[mid] <= p) e = mid + 1; else hi2 = mid; }
    const unsigned long long bits = bitpos[e] - bitpos[lo];
    if (bits > 0xFFFFFFFFull) *too_long = 1;           // num_bits is 32 bits wide (pattern.h:49)
    num_local[p] = (uint32_t)(e - lo);
    last_id[p] = e > lo ? ssid[e - 1] : 0u;
    num_bits[p] = (uint32_t)bits;
    words[p] = bits ? ((bits + 127ull) / 128ull) * 2ull : 0ull;            // pattern.h:79-81
    pbit0[p] = bitpos[lo];
}

// one thread per event writes its code: L - 1 ones, a zero, the L - 1 low bits of the delta (elias_gamma.h), MSB first
__global__ __launch_bounds__(BD_THREADS) void bd_write_codes_kernel(const uint32_t* __restrict__ spid, const uint32_t* __restrict__ ssid, uint64_t E,
                                                                    const unsigned long long* __restrict__ bitpos, const unsigned long long* __restrict__ pbit0,
                                                                    const unsigned long long* __restrict__ data_offset, unsigned long long* __restrict__ data,
                                                                    uint64_t n_words) {
    const uint64_t i = (uint64_t)blockIdx.x * BD_THREADS + threadIdx.x;
    if (i >= E || i == 0 || spid[i - 1] != spid[i]) return;
    const uint32_t p = spid[i];
    const uint32_t d = ssid[i] - ssid[i - 1];
    if (!d) return;
    const uint32_t L = 32u - (uint32_t)__clz((int)d), len = 2u * L - 1u;                  // len <= 63
    const unsigned long long code = (((1ull << (L - 1u)) - 1ull) << L) | ((unsigned long long)d - (1ull << (L - 1u)));
    const unsigned long long b = data_offset[p] * 64ull + (bitpos[i] - pbit0[p]);
    const uint64_t w = b >> 6;
    const uint32_t room = 64u - (uint32_t)(b & 63ull);
    if (w >= n_words) return;                          // (cannot happen: the stream's words were counted from the same lengths)
    if (len <= room) {
        atomicOr(&data[w], code << (room - len));
    } else {
        const uint32_t rem = len - room;               // the code straddles two words
        atomicOr(&data[w], code >> rem);
        if (w + 1 < n_words) atomicOr(&data[w + 1], (code & ((1ull << rem) - 1ull)) << (64u - rem));
    }
}

// (d) bstart[b] = first k-mer of bucket b in D, b <= nb
__global__ __launch_bounds__(BD_THREADS) void bd_bucket_starts_kernel(const uint64_t* __restrict__ D, uint64_t nD, uint64_t nb, unsigned long long* __restrict__ bstart) {
    const uint64_t b = (uint64_t)blockIdx.x * BD_THREADS + threadIdx.x;
    if (b > nb) return;
    bstart[b] = b == nb ? nD : bd_lower_bound(D, nD, b << 32);
}
__global__ __launch_bounds__(BD_THREADS) void bd_bucket_caps_kernel(const unsigned long long* __restrict__ bstart, uint64_t nb, unsigned long long* __restrict__ caps) {
    const uint64_t b = (uint64_t)blockIdx.x * BD_THREADS + threadIdx.x;
    if (b > nb) return;
    unsigned long long cap = 0;
    if (b < nb) {
        const unsigned long long cnt = bstart[b + 1] - bstart[b];
        cap = 16;                                      // INITIAL_SIZE; doubled while filled > 0.8 * allocated (hashmap_lp.h:429-437): 5 filled > 4 allocated
        while (5ull * cnt > 4ull * cap) cap *= 2;
    }
    caps[b] = cap;
}
__global__ __launch_bounds__(BD_THREADS) void bd_fill_empty_kernel(unsigned long long* __restrict__ slots, uint64_t n) {
    const uint64_t i = (uint64_t)blockIdx.x * BD_THREADS + threadIdx.x;
    if (i < n) slots[i] = BD_EMPTY;
}
__global__ __launch_bounds__(BD_THREADS) void bd_insert_kernel(const uint64_t* __restrict__ D, const uint32_t* __restrict__ cur, uint64_t nD, uint64_t nb,
                                                               const unsigned long long* __restrict__ boff, unsigned long long* __restrict__ slots,
                                                               uint32_t* __restrict__ failed) {
    const uint64_t i = (uint64_t)blockIdx.x * BD_THREADS + threadIdx.x;
    if (i >= nD) return;
    const uint64_t x = D[i], b = x >> 32;
    if (b >= nb) { *failed = 1; return; }              // a k-mer wider than k symbols: the caller's list was not made with the builder's k
    const uint32_t key = (uint32_t)x;
    const unsigned long long off = boff[b], cap = boff[b + 1] - off, item = (unsigned long long)key | ((unsigned long long)cur[i] << 32);
    unsigned long long h = (unsigned long long)kmdb_fmix32(key) & (cap - 1);
    // Linear probing with priorities: a slot keeps the SMALLER of its item and the one passing by (the empty marker is larger than every
    // item: val < INT32_MAX), the larger one moves on.  Whatever order the threads arrive in, the table that results is the same one — it
    // depends on the bucket's items and its capacity only, not on how the samples were cut into calls — and every item still lies between
    // its home slot and the next empty slot, which is all hash_map_lp::find asks (hashmap_lp.h:308-333).
    unsigned long long carry = item;
    for (unsigned long long step = 0; step < 2 * cap; ++step) {                        // the fill is at most 0.8: an empty slot ends every walk
        const unsigned long long old = atomicMin(&slots[off + h], carry);
        if (old == BD_EMPTY) return;
        if (old > carry) carry = old;                  // (we took the slot; its item goes on from here, as its own probe would)
        h = (h + 1) & (cap - 1);
    }
    *failed = 1;
}

// ---- the seed: a stored database back into the state above (kmdb_build_begin_from_db) ------------------------------------------------
// One word per check of the seed; all of them are read once, after the last kernel.
enum : uint32_t { BD_BAD_VALUE = 0, BD_BAD_TWICE, BD_BAD_WIDE, BD_BAD_COUNT, BD_BAD_STREAM, BD_BAD_IDS, BD_BAD_PARENT, BD_BAD_WORDS };

// (a) the inverse of bd_insert_kernel, a piece of the slots at a time: flag[i] = slot i of the piece holds an item, i <= m (flag[m] = 0)
__global__ __launch_bounds__(BD_THREADS) void bd_seed_flag_kernel(const unsigned long long* __restrict__ slots, uint64_t m, uint64_t P, uint32_t* __restrict__ flag,
                                                                  uint32_t* __restrict__ bad) {
    const uint64_t i = (uint64_t)blockIdx.x * BD_THREADS + threadIdx.x;
    if (i > m) return;
    uint32_t f = 0;
    if (i < m) {
        const uint32_t val = (uint32_t)(slots[i] >> 32);
        f = val != 0x7fffffffu ? 1u : 0u;
        if (f && (val == 0 || val >= P)) bad[BD_BAD_VALUE] = 1;        // (every writer stores the same value)
    }
    flag[i] = f;
}
// the item of slot slot0 + i goes to place base + fscan[i]: k-mer = its bucket (the last b with boff[b] <= slot) << 32 | key, pid = val
__global__ __launch_bounds__(BD_THREADS) void bd_seed_compact_kernel(const unsigned long long* __restrict__ slots, const uint32_t* __restrict__ flag,
                                                                     const uint32_t* __restrict__ fscan, uint64_t m, uint64_t slot0,
                                                                     const unsigned long long* __restrict__ boff, uint64_t nb, uint64_t base, uint64_t nD,
                                                                     uint64_t* __restrict__ K, uint32_t* __restrict__ pid) {
    const uint64_t i = (uint64_t)blockIdx.x * BD_THREADS + threadIdx.x;
    if (i >= m || !flag[i]) return;
    const uint64_t at = base + fscan[i], s = slot0 + i;
    if (at >= nD) return;                              // (more items than the patterns count: the host compares the totals)
    uint64_t lo = 0, hi = nb;                          // boff[0] = 0 <= s < boff[nb]
    while (hi - lo > 1) { const uint64_t mid = (lo + hi) / 2; if (boff[mid] <= s) lo = mid; else hi = mid; }
    const unsigned long long item = slots[i];
    K[at] = (lo << 32) | (item & 0xffffffffull);
    pid[at] = (uint32_t)(item >> 32);
}

// (b) is_parent is not in a stored database: a pattern is a parent iff some pattern names it (pattern.h:106-114).  isp is zeroed before.
__global__ __launch_bounds__(BD_THREADS) void bd_seed_isp_kernel(const long long* __restrict__ parent, uint64_t P, uint32_t* __restrict__ isp, uint32_t* __restrict__ bad) {
    const uint64_t p = (uint64_t)blockIdx.x * BD_THREADS + threadIdx.x;
    if (p >= P) return;
    const long long q = parent[p];
    if (q < -1 || q >= (long long)p) { bad[BD_BAD_PARENT] = 1; return; }
    if (q >= 0) isp[q] = 1;
}

// (d) the sorted dictionary: strictly ascending, inside kbits; hist[p] = k-mers whose pattern is p
__global__ __launch_bounds__(BD_THREADS) void bd_seed_dict_check_kernel(const uint64_t* __restrict__ D, const uint32_t* __restrict__ cur, uint64_t nD, uint32_t kbits,
                                                                        uint64_t P, uint32_t* __restrict__ hist, uint32_t* __restrict__ bad) {
    const uint64_t i = (uint64_t)blockIdx.x * BD_THREADS + threadIdx.x;
    if (i >= nD) return;
    const uint64_t x = D[i];
    if (i && D[i - 1] >= x) bad[BD_BAD_TWICE] = 1;
    if (kbits < 64 && (x >> kbits)) bad[BD_BAD_WIDE] = 1;
    const uint32_t c = cur[i];
    if (c && c < P) atomicAdd(&hist[c], 1u);           // (0 and >= P were flagged where the slots were read)
}
__global__ __launch_bounds__(BD_THREADS) void bd_seed_count_check_kernel(const uint32_t* __restrict__ hist, const long long* __restrict__ here, uint64_t P,
                                                                         uint32_t* __restrict__ bad) {
    const uint64_t p = (uint64_t)blockIdx.x * BD_THREADS + threadIdx.x;
    if (p < P && (long long)hist[p] != here[p]) bad[BD_BAD_COUNT] = 1;
}

// 64 bits of a pattern's stream from bit `pos` on, MSB first; words past the pattern's own read as zeros
__device__ __forceinline__ uint64_t bd_seed_window(const uint64_t* __restrict__ s, uint64_t words, uint64_t pos) {
    const uint64_t w = pos >> 6;
    const uint32_t sh = (uint32_t)pos & 63u;
    const uint64_t c0 = w < words ? s[w] : 0ull, c1 = w + 1 < words ? s[w + 1] : 0ull;
    return sh ? (c0 << sh) | (c1 >> (64u - sh)) : c0;
}
// (c) one thread per pattern: its num_local - 1 codes (what bd_write_codes_kernel writes) back into its stretch of the events, ascending.
// The deltas' running sums go down first; once their total is known, id[0] = last_sample_id - total is added to each.
__global__ __launch_bounds__(BD_THREADS) void bd_seed_decode_kernel(const uint32_t* __restrict__ num_local, const uint32_t* __restrict__ estart,
                                                                    const uint32_t* __restrict__ last_id, const uint32_t* __restrict__ num_bits,
                                                                    const unsigned long long* __restrict__ data_offset, const uint64_t* __restrict__ data,
                                                                    uint64_t n_words, uint64_t P, uint64_t E, uint64_t n_samples, uint32_t* __restrict__ ev_pid,
                                                                    uint32_t* __restrict__ ev_sid, uint32_t* __restrict__ bad) {
    const uint64_t p = (uint64_t)blockIdx.x * BD_THREADS + threadIdx.x;
    if (p >= P) return;
    const uint32_t n = num_local[p], bits = num_bits[p];
    if (!n) { if (bits) bad[BD_BAD_STREAM] = 1; return; }
    const uint64_t e0 = estart[p], off = data_offset[p], words = bits ? (((uint64_t)bits + 127ull) / 128ull) * 2ull : 0ull;
    if (e0 + n > E) { bad[BD_BAD_STREAM] = 1; return; }                        // (cannot happen: E is the sum of num_local)
    if (off > n_words || words > n_words - off) { bad[BD_BAD_WORDS] = 1; return; }
    const uint32_t last = last_id[p];
    if (last >= n_samples) { bad[BD_BAD_IDS] = 1; return; }
    const uint64_t* __restrict__ s = data + off;
    uint64_t pos = 0, total = 0;
    ev_pid[e0] = (uint32_t)p;
    ev_sid[e0] = 0;
    for (uint32_t i = 1; i < n; ++i) {
        if (pos >= bits) { bad[BD_BAD_STREAM] = 1; return; }
        const uint64_t win = bd_seed_window(s, words, pos);
        if ((uint32_t)(win >> 32) == ~0u) { bad[BD_BAD_STREAM] = 1; return; }  // a delta is 32 bits wide: at most 31 leading ones, never clamped here
        const GammaCode g = gamma_code(win);
        pos += g.len();
        total += g.value();
        if (pos > bits) { bad[BD_BAD_STREAM] = 1; return; }
        if (total > last) { bad[BD_BAD_IDS] = 1; return; }                     // the first id would be negative
        ev_pid[e0 + i] = (uint32_t)p;
        ev_sid[e0 + i] = (uint32_t)total;
    }
    if (pos != bits) { bad[BD_BAD_STREAM] = 1; return; }
    const uint32_t first = last - (uint32_t)total;
    for (uint32_t i = 0; i < n; ++i) ev_sid[e0 + i] += first;
}

// ---- host side ----------------------------------------------------------------------------------------------------------------------
struct Acct {
    uint64_t live = 0, peak = 0, limit = 0;            // limit: KMDB_BUILD_DEVICE_BYTES, 0 = what the device has
};

struct BBuf {
    void* p = nullptr;
    size_t bytes = 0;
    Acct* a = nullptr;
    BBuf() = default;
    BBuf(const BBuf&) = delete;
    BBuf& operator=(const BBuf&) = delete;
    ~BBuf() { release(); }
    void release() {
        if (p) { (void)hipFree(p); a->live -= bytes; if (dev_mem_meter) dev_mem_meter->sub(bytes); }
        p = nullptr; bytes = 0;
    }
    void swap(BBuf& o) { std::swap(p, o.p); std::swap(bytes, o.bytes); std::swap(a, o.a); }
    // 0, or 1 with the error set: the bytes asked for are named, never a bare hipMalloc failure
    int alloc(Acct& acct, size_t b, const char* what) {
        release();
        b = std::max<size_t>(b, 16);
        size_t free_b = 0, total_b = 0;
        const hipError_t q = hipMemGetInfo(&free_b, &total_b);
        if (q != hipSuccess) return kmdb_set_error(std::string("kmdb_build: hipMemGetInfo: ") + hipGetErrorString(q));
        bool fits = b <= free_b && (!acct.limit || acct.live + b <= acct.limit);
        if (fits && hipMalloc(&p, b) != hipSuccess) { (void)hipGetLastError(); p = nullptr; fits = false; }
        if (!fits)
            return kmdb_set_error("kmdb_build: the collection's state does not fit the device: " + std::to_string(b) + " bytes needed for " + what + ", the builder holds " +
                                  std::to_string(acct.live) + ", " + std::to_string(acct.limit ? std::min<uint64_t>(free_b, acct.limit > acct.live ? acct.limit - acct.live : 0) : free_b) +
                                  " are free");
        bytes = b; a = &acct;
        acct.live += b;
        acct.peak = std::max(acct.peak, acct.live);
        if (dev_mem_meter) dev_mem_meter->add(b);
        return 0;
    }
    template <class T> T* as() const { return (T*)p; }
};

inline unsigned bd_blocks(uint64_t n) { return (unsigned)((n + BD_THREADS - 1) / BD_THREADS); }
inline unsigned bd_bits(uint64_t below) { unsigned b = 1; while (b < 64 && (1ull << b) < below) ++b; return b; }      // bits that hold every value < below

}  // namespace

#define BD_TRY(expr)                                                                            \
    do {                                                                                        \
        hipError_t e_ = (expr);                                                                 \
        if (e_ != hipSuccess)                                                                   \
            return kmdb_set_error(std::string("kmdb_build: ") + #expr + ": " + hipGetErrorString(e_)); \
    } while (0)
#define BD_DO(expr) do { if (const int rc_ = (expr)) return rc_; } while (0)

struct kmdb_builder {
    int device = 0;
    hipStream_t st = nullptr;
    uint32_t k = 0, bits = 0, kbits = 0;
    int32_t alphabet = 0;
    double fraction = 1.0, start_fraction = 0.0;
    bool finished = false, dead = false;
    std::vector<std::string> names;
    std::vector<uint64_t> counts;
    Acct acct;
    BBuf D, cur;                   // nD entries each
    uint64_t nD = 0;
    BBuf here, nsam, parent, isp;  // cap_p entries each
    uint64_t P = 1, cap_p = 0;
    BBuf ev_pid, ev_sid;           // cap_e entries each
    uint64_t E = 0, cap_e = 0;
    BBuf overflow;                 // one flag
    kmdb_build_stats stats{};
    kmdb_build_seed_stats seed{};  // zeros unless the builder was seeded
    kmdb_build_handoff_stats handoff{};   // zeros unless the builder ended in kmdb_build_finish_device
    std::vector<hipEvent_t> events;
    ~kmdb_builder() { for (hipEvent_t e : events) (void)hipEventDestroy(e); }
};

namespace {

// the arrays of the tree hold `need` entries at least (their first `used` are kept)
int bd_grow(kmdb_builder* b, BBuf& buf, size_t elem, uint64_t used, uint64_t need, const char* what) {
    BBuf nb;
    BD_DO(nb.alloc(b->acct, (size_t)need * elem, what));
    if (used && buf.p) BD_TRY(hipMemcpyAsync(nb.p, buf.p, (size_t)used * elem, hipMemcpyDeviceToDevice, b->st));
    BD_TRY(hipStreamSynchronize(b->st));
    buf.swap(nb);
    return 0;
}

// room for `more_p` patterns and `more_e` events beyond what is there; grown by half as much again at least, so that a collection added
// in many small calls copies its arrays a logarithmic number of times
int bd_reserve(kmdb_builder* b, uint64_t more_p, uint64_t more_e) {
    if (b->P + more_p > b->cap_p || !b->here.p) {
        const uint64_t cap = std::max<uint64_t>(b->P + more_p, b->cap_p + b->cap_p / 2);
        BD_DO(bd_grow(b, b->here, 8, b->P, cap, "the patterns' k-mer counts"));
        BD_DO(bd_grow(b, b->nsam, 4, b->P, cap, "the patterns' sample counts"));
        BD_DO(bd_grow(b, b->parent, 8, b->P, cap, "the patterns' parents"));
        BD_DO(bd_grow(b, b->isp, 4, b->P, cap, "the patterns' parent flags"));
        b->cap_p = cap;
    }
    if (b->E + more_e > b->cap_e || !b->ev_pid.p) {
        const uint64_t cap = std::max<uint64_t>(b->E + more_e, b->cap_e + b->cap_e / 2);
        BD_DO(bd_grow(b, b->ev_pid, 4, b->E, cap, "the events' patterns"));
        BD_DO(bd_grow(b, b->ev_sid, 4, b->E, cap, "the events' samples"));
        b->cap_e = cap;
    }
    return 0;
}

hipEvent_t bd_event(kmdb_builder* b, size_t i) {
    while (b->events.size() <= i) {
        hipEvent_t e = nullptr;
        if (hipEventCreate(&e) != hipSuccess) return nullptr;
        b->events.push_back(e);
    }
    return b->events[i];
}
#define BD_MARK(i)                                                                       \
    do {                                                                                 \
        hipEvent_t ev_ = bd_event(b, (i));                                               \
        if (!ev_) return kmdb_set_error("kmdb_build: hipEventCreate failed");            \
        BD_TRY(hipEventRecord(ev_, b->st));                                              \
    } while (0)

double bd_ms(kmdb_builder* b, size_t i0, size_t i1) {
    float ms = 0;
    return hipEventElapsedTime(&ms, b->events[i0], b->events[i1]) == hipSuccess ? (double)ms : 0.0;
}

// One piece of a call: n samples whose lists lie one behind the other in d_K (device), sample s at [off[s], off[s + 1]) (off: host).
// The lists are strictly ascending (checked by the caller, or made by the extractor).  Names and counts are the caller's business.
int bd_add_device(kmdb_builder* b, const uint64_t* d_K, const uint64_t* off, size_t n, uint64_t first_sample_id) {
    const uint64_t T = off[n];
    if (!T) return 0;
    if (T >= (1ull << 31)) return kmdb_set_error("kmdb_build: internal error (a piece of 2^31 k-mers or more)");
    hipStream_t st = b->st;
    uint32_t cmax = 0;
    size_t nonempty = 0;
    for (size_t s = 0; s < n; ++s) { cmax = std::max<uint32_t>(cmax, (uint32_t)(off[s + 1] - off[s])); nonempty += off[s + 1] > off[s]; }
    if (b->nD + T >= 0xFFFFFFFFull) return kmdb_set_error("kmdb_build: 2^32 distinct k-mers or more: the dictionary's positions are 32 bits wide");
    if (b->P + T >= 0x7FFFFFFFull) return kmdb_set_error("kmdb_build: 2^31 patterns or more: pattern ids are 31 bits wide (hashmap_lp.h:78)");
    if (b->E + T >= 0x7FFFFFFFull) return kmdb_set_error("kmdb_build: 2^31 (pattern, sample) events or more: the sort at finish takes 31-bit sizes");
    BD_MARK(0);
    // ---- (a) the new k-mers, merged into the dictionary in one pass
    {
        BBuf S, flag, fscan, tmp, Nw;
        BD_DO(S.alloc(b->acct, T * 8, "the call's sorted k-mers"));
        BD_DO(flag.alloc(b->acct, (T + 1) * 4, "the new k-mer flags"));
        BD_DO(fscan.alloc(b->acct, (T + 1) * 4, "the new k-mer ranks"));
        size_t tb1 = 0, tb2 = 0;
        BD_TRY(prim::sort_keys(nullptr, tb1, d_K, S.as<uint64_t>(), T, 0, b->kbits, st));
        BD_TRY(prim::exclusive_sum(nullptr, tb2, flag.as<uint32_t>(), fscan.as<uint32_t>(), T + 1, st));
        BD_DO(tmp.alloc(b->acct, std::max(tb1, tb2), "the sort's temporary storage"));
        BD_TRY(prim::sort_keys(tmp.p, tb1, d_K, S.as<uint64_t>(), T, 0, b->kbits, st));
        BD_TRY(hipMemsetAsync(flag.p, 0, (T + 1) * 4, st));
        hipLaunchKernelGGL(bd_flag_new_kernel, dim3(bd_blocks(T)), dim3(BD_THREADS), 0, st, S.as<uint64_t>(), T, b->D.as<uint64_t>(), b->nD, flag.as<uint32_t>());
        BD_TRY(hipGetLastError());
        BD_TRY(prim::exclusive_sum(tmp.p, tb2, flag.as<uint32_t>(), fscan.as<uint32_t>(), T + 1, st));
        uint32_t nN32 = 0;
        BD_TRY(hipMemcpyAsync(&nN32, fscan.as<uint32_t>() + T, 4, hipMemcpyDeviceToHost, st));
        BD_TRY(hipStreamSynchronize(st));
        const uint64_t nN = nN32;
        if (nN > T) return kmdb_set_error("kmdb_build: internal error (more new k-mers than k-mers)");
        if (nN) {
            BBuf D2, cur2;
            BD_DO(Nw.alloc(b->acct, nN * 8, "the new k-mers"));
            BD_DO(D2.alloc(b->acct, (b->nD + nN) * 8, "the dictionary"));
            BD_DO(cur2.alloc(b->acct, (b->nD + nN) * 4, "the k-mers' pattern ids"));
            hipLaunchKernelGGL(bd_compact_kernel, dim3(bd_blocks(T)), dim3(BD_THREADS), 0, st, S.as<uint64_t>(), flag.as<uint32_t>(), fscan.as<uint32_t>(), T, nN, Nw.as<uint64_t>());
            if (b->nD)
                hipLaunchKernelGGL(bd_merge_old_kernel, dim3(bd_blocks(b->nD)), dim3(BD_THREADS), 0, st, b->D.as<uint64_t>(), b->cur.as<uint32_t>(), b->nD, Nw.as<uint64_t>(), nN,
                                   D2.as<uint64_t>(), cur2.as<uint32_t>());
            hipLaunchKernelGGL(bd_merge_new_kernel, dim3(bd_blocks(nN)), dim3(BD_THREADS), 0, st, Nw.as<uint64_t>(), nN, b->D.as<uint64_t>(), b->nD, D2.as<uint64_t>(), cur2.as<uint32_t>());
            BD_TRY(hipGetLastError());
            BD_TRY(hipStreamSynchronize(st));
            b->D.swap(D2);
            b->cur.swap(cur2);
            b->nD += nN;
        }
    }
    BD_MARK(1);
    // ---- (b) the samples, one after the other
    uint64_t bound_p = 0;
    for (size_t s = 0; s < n; ++s) bound_p += std::min<uint64_t>(off[s + 1] - off[s], b->P + bound_p);       // new groups <= min(k-mers, patterns)
    BD_DO(bd_reserve(b, bound_p, T));
    const unsigned pid_bits = bd_bits(b->P + bound_p);
    BBuf pidA, pidB, slotA, slotB, head, hscan, gstart, isnew, nrank, tmp, curs;
    const size_t c1 = (size_t)cmax + 1;
    BD_DO(pidA.alloc(b->acct, c1 * 4, "a sample's pattern ids"));
    BD_DO(pidB.alloc(b->acct, c1 * 4, "a sample's sorted pattern ids"));
    BD_DO(slotA.alloc(b->acct, c1 * 4, "a sample's dictionary positions"));
    BD_DO(slotB.alloc(b->acct, c1 * 4, "a sample's sorted dictionary positions"));
    BD_DO(head.alloc(b->acct, c1 * 4, "a sample's group flags"));
    BD_DO(hscan.alloc(b->acct, c1 * 4, "a sample's group indices"));
    BD_DO(gstart.alloc(b->acct, c1 * 4, "a sample's group starts"));
    BD_DO(isnew.alloc(b->acct, c1 * 4, "a sample's new-pattern flags"));
    BD_DO(nrank.alloc(b->acct, c1 * 4, "a sample's new-pattern ranks"));
    BD_DO(curs.alloc(b->acct, (nonempty + 1) * 16, "the cursors"));
    size_t tbs = 0, tbc = 0;
    BD_TRY(prim::sort_pairs(nullptr, tbs, pidA.as<uint32_t>(), pidB.as<uint32_t>(), slotA.as<uint32_t>(), slotB.as<uint32_t>(), cmax, 0, pid_bits, st));
    BD_TRY(prim::exclusive_sum(nullptr, tbc, head.as<uint32_t>(), hscan.as<uint32_t>(), c1, st));
    BD_DO(tmp.alloc(b->acct, std::max(tbs, tbc), "the sort's temporary storage"));
    const uint64_t cursor0[2] = {b->P, b->E};
    BD_TRY(hipMemcpyAsync(curs.p, cursor0, 16, hipMemcpyHostToDevice, st));
    BdTree t{b->here.as<long long>(), b->nsam.as<uint32_t>(), b->parent.as<long long>(), b->isp.as<uint32_t>(), b->cap_p,
             b->ev_pid.as<uint32_t>(), b->ev_sid.as<uint32_t>(), b->cap_e, curs.as<uint64_t>(), b->overflow.as<uint32_t>()};
    uint32_t j = 0;
    for (size_t s = 0; s < n; ++s) {
        const uint32_t c = (uint32_t)(off[s + 1] - off[s]);
        if (!c) continue;                              // an empty sample keeps its id and launches nothing
        const unsigned gc = bd_blocks(c), gc1 = bd_blocks((uint64_t)c + 1);
        size_t need_s = 0, need_c = 0;
        BD_TRY(prim::sort_pairs(nullptr, need_s, pidA.as<uint32_t>(), pidB.as<uint32_t>(), slotA.as<uint32_t>(), slotB.as<uint32_t>(), c, 0, pid_bits, st));
        BD_TRY(prim::exclusive_sum(nullptr, need_c, head.as<uint32_t>(), hscan.as<uint32_t>(), (size_t)c + 1, st));
        if (std::max(need_s, need_c) > tmp.bytes) BD_DO(tmp.alloc(b->acct, std::max(need_s, need_c), "the sort's temporary storage"));
        BD_MARK(2 + 4 * j);
        hipLaunchKernelGGL(bd_lookup_kernel, dim3(gc), dim3(BD_THREADS), 0, st, d_K + off[s], c, b->D.as<uint64_t>(), b->nD, b->cur.as<uint32_t>(), pidA.as<uint32_t>(), slotA.as<uint32_t>());
        BD_MARK(3 + 4 * j);
        BD_TRY(prim::sort_pairs(tmp.p, need_s, pidA.as<uint32_t>(), pidB.as<uint32_t>(), slotA.as<uint32_t>(), slotB.as<uint32_t>(), c, 0, pid_bits, st));
        BD_MARK(4 + 4 * j);
        hipLaunchKernelGGL(bd_heads_kernel, dim3(gc1), dim3(BD_THREADS), 0, st, pidB.as<uint32_t>(), c, head.as<uint32_t>());
        BD_TRY(prim::exclusive_sum(tmp.p, need_c, head.as<uint32_t>(), hscan.as<uint32_t>(), (size_t)c + 1, st));
        hipLaunchKernelGGL(bd_group_starts_kernel, dim3(gc1), dim3(BD_THREADS), 0, st, head.as<uint32_t>(), hscan.as<uint32_t>(), c, gstart.as<uint32_t>());
        hipLaunchKernelGGL(bd_decide_kernel, dim3(gc1), dim3(BD_THREADS), 0, st, pidB.as<uint32_t>(), gstart.as<uint32_t>(), hscan.as<uint32_t>(), c, t, isnew.as<uint32_t>());
        BD_TRY(prim::exclusive_sum(tmp.p, need_c, isnew.as<uint32_t>(), nrank.as<uint32_t>(), (size_t)c + 1, st));
        hipLaunchKernelGGL(bd_apply_kernel, dim3(gc), dim3(BD_THREADS), 0, st, pidB.as<uint32_t>(), gstart.as<uint32_t>(), hscan.as<uint32_t>(), isnew.as<uint32_t>(), nrank.as<uint32_t>(), c, t,
                           j, (uint32_t)(first_sample_id + s));
        hipLaunchKernelGGL(bd_setcur_kernel, dim3(gc), dim3(BD_THREADS), 0, st, slotB.as<uint32_t>(), head.as<uint32_t>(), hscan.as<uint32_t>(), isnew.as<uint32_t>(), nrank.as<uint32_t>(), c, t, j,
                           b->cur.as<uint32_t>(), b->nD);
        BD_TRY(hipGetLastError());
        BD_MARK(5 + 4 * j);
        ++j;
    }
    uint64_t cursor1[2] = {0, 0};
    uint32_t over = 0;
    BD_TRY(hipMemcpyAsync(cursor1, curs.as<uint64_t>() + 2 * (size_t)j, 16, hipMemcpyDeviceToHost, st));
    BD_TRY(hipMemcpyAsync(&over, b->overflow.p, 4, hipMemcpyDeviceToHost, st));
    BD_TRY(hipStreamSynchronize(st));
    if (over || cursor1[0] < b->P || cursor1[0] > b->cap_p || cursor1[1] < b->E || cursor1[1] > b->cap_e)
        return kmdb_set_error("kmdb_build: internal error (a reserved capacity was passed)");
    b->P = cursor1[0];
    b->E = cursor1[1];
    b->stats.merge_ms += bd_ms(b, 0, 1);
    for (uint32_t q = 0; q < j; ++q) {
        b->stats.lookup_ms += bd_ms(b, 2 + 4 * q, 3 + 4 * q);
        b->stats.sort_ms += bd_ms(b, 3 + 4 * q, 4 + 4 * q);
        b->stats.group_ms += bd_ms(b, 4 + 4 * q, 5 + 4 * q);
    }
    return 0;
}

int bd_usable(kmdb_builder* b, const char* who) {
    if (!b) return kmdb_set_error(std::string(who) + ": null argument");
    if (b->dead) return kmdb_set_error(std::string(who) + ": the builder is dead after an earlier error; free it");
    if (b->finished) return kmdb_set_error(std::string(who) + ": the builder was finished; it takes no more samples");
    return 0;
}

struct BdSeedPlan {                // what the host reads off a kmdbh_db before any device work
    const kmdbh_db* db;
    const kmdb_db_view* v;
    uint64_t nD, E, n_slots;       // sum of num_kmers, sum of num_local, bucket_offset[n_buckets]
};
int bd_seed(kmdb_builder* b, const BdSeedPlan& plan, const char* who);

int bd_begin(const char* who, uint32_t k, double fraction, double start_fraction, int32_t alphabet, const kmdb_opts* opts, const BdSeedPlan* seed, kmdb_builder** out) {
    if (!out) return kmdb_set_error(std::string(who) + ": null argument");
    *out = nullptr;
    if (opts && opts->abi_version && !kmdb_abi_compatible(opts->abi_version)) return kmdb_set_error(std::string(who) + ": kmdb_opts.abi_version is not served by this library");
    int8_t map[256];
    uint32_t size = 0, bits = 0;
    int preserve = 0;
    if (alphabet < 0 || alphabet >= KMDB_ALPHABET_COUNT || kmdbh_alphabet_table(alphabet, map, &size, &bits, &preserve))
        return kmdb_set_error(std::string(who) + ": unknown alphabet " + std::to_string(alphabet));
    if (k == 0 || k > 64u / bits - 1u) return kmdb_set_error(std::string(who) + ": k-mer length must be 1.." + std::to_string(64u / bits - 1u) + " for this alphabet (alphabet.h:37)");
    if (!(fraction > 0.0) || !(start_fraction >= 0.0)) return kmdb_set_error(std::string(who) + ": the fraction must be positive and the start fraction not negative");
    BD_TRY(hipSetDevice(opts ? opts->device : 0));
    kmdb_builder* b = new kmdb_builder();
    struct Hold { kmdb_builder* b; ~Hold() { delete b; } } hold{b};
    b->device = opts ? opts->device : 0;
    b->st = (opts && opts->stream) ? (hipStream_t)opts->stream : (hipStream_t) nullptr;
    b->k = k; b->bits = bits; b->alphabet = alphabet; b->fraction = fraction; b->start_fraction = start_fraction;
    const int prefix_bits = (int)(bits * k) - 32;
    b->kbits = std::min<uint32_t>(64u, bits * k + (prefix_bits < 8 ? (uint32_t)(8 - prefix_bits) : 0u));       // the widened word (kmer_extract.h:86-90)
    if (const char* e = getenv("KMDB_BUILD_DEVICE_BYTES")) b->acct.limit = strtoull(e, nullptr, 10);
    BD_DO(b->overflow.alloc(b->acct, 4, "a flag"));
    BD_TRY(hipMemsetAsync(b->overflow.p, 0, 4, b->st));
    if (seed) {
        BD_DO(bd_seed(b, *seed, who));
        hold.b = nullptr;
        *out = b;
        return 0;
    }
    BD_DO(bd_reserve(b, 1u << 16, 1u << 16));
    // pattern 0 = the empty pattern (prefix_kmer_db.cpp:24; pattern_t(): parent -1, everything else 0)
    const long long zero64 = 0, minus1 = -1;
    const uint32_t zero32 = 0;
    BD_TRY(hipMemcpyAsync(b->here.p, &zero64, 8, hipMemcpyHostToDevice, b->st));
    BD_TRY(hipMemcpyAsync(b->parent.p, &minus1, 8, hipMemcpyHostToDevice, b->st));
    BD_TRY(hipMemcpyAsync(b->nsam.p, &zero32, 4, hipMemcpyHostToDevice, b->st));
    BD_TRY(hipMemcpyAsync(b->isp.p, &zero32, 4, hipMemcpyHostToDevice, b->st));
    BD_TRY(hipStreamSynchronize(b->st));
    hold.b = nullptr;
    *out = b;
    return 0;
}

// The seed (replaces db->deserialize + the filter and alphabet taken from the database, console_build.cpp:48-57): the arrays of a kmdbh_db
// become the state a builder would hold after the database's samples, so that the add and finish paths go on from it unchanged.
//   (a) the slots go up a piece at a time (KMDB_BUILD_SEED_SLOTS_PER_PIECE, default 2^27: the whole table is never resident); flag, scan,
//       compact to (k-mer, pattern id); the pieces' buffers are released before the sort's are allocated; sort_pairs over kbits -> D, cur
//   (b) here / nsam / parent are the stored num_kmers / num_samples / parent_id; isp is recomputed from parent
//   (d) D strictly ascending and inside kbits, the k-mers per pattern against num_kmers
//   (c) a scan of num_local gives every pattern its stretch of the events; one thread per pattern decodes its stream into it
// Held at the peak of (a): 12 bytes per distinct k-mer twice over (the pairs before and after the sort) plus the sort's storage; afterwards
// the builder's own 12 per k-mer, 24 per pattern and 8 per event, and while (c) runs 28 per pattern and the streams.
int bd_seed(kmdb_builder* b, const BdSeedPlan& plan, const char* who) {
    const kmdb_db_view* v = plan.v;
    const uint64_t P = v->n_patterns, N = v->n_samples, nb = v->n_buckets, n_words = v->n_data_words, nD = plan.nD, E = plan.E, n_slots = plan.n_slots;
    hipStream_t st = b->st;
    kmdb_build_seed_stats& ss = b->seed;
    ss.slots = n_slots;
    BBuf bad;
    BD_DO(bad.alloc(b->acct, 8 * 4, "the seed's flags"));
    BD_TRY(hipMemsetAsync(bad.p, 0, 8 * 4, st));
    uint32_t* d_bad = bad.as<uint32_t>();
    auto h2d = [&](void* dst, const void* src, size_t bytes) -> hipError_t { ss.h2d_bytes += bytes; return hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, st); };
    // ---- (a) the dictionary from the tables
    {
        BBuf Kin, Pin;
        BD_DO(Kin.alloc(b->acct, nD * 8, "the tables' k-mers"));
        BD_DO(Pin.alloc(b->acct, nD * 4, "the tables' pattern ids"));
        uint64_t found = 0;
        {
            uint64_t piece = 1ull << 27;
            if (const char* e = getenv("KMDB_BUILD_SEED_SLOTS_PER_PIECE")) piece = std::min<uint64_t>(std::max<uint64_t>(strtoull(e, nullptr, 10), 1), 1ull << 30);
            piece = std::min(piece, std::max<uint64_t>(n_slots, 1));
            BBuf boff, chunk, flag, fscan, tmp;
            BD_DO(boff.alloc(b->acct, (nb + 1) * 8, "bucket_offset"));
            BD_DO(chunk.alloc(b->acct, piece * 8, "a piece of the hashtables' slots"));
            BD_DO(flag.alloc(b->acct, (piece + 1) * 4, "the slots' flags"));
            BD_DO(fscan.alloc(b->acct, (piece + 1) * 4, "the slots' ranks"));
            size_t tb = 0;
            BD_TRY(prim::exclusive_sum(nullptr, tb, flag.as<uint32_t>(), fscan.as<uint32_t>(), piece + 1, st));
            BD_DO(tmp.alloc(b->acct, tb, "the scan's temporary storage"));
            BD_MARK(0);
            BD_TRY(h2d(boff.p, v->bucket_offset, (nb + 1) * 8));
            BD_MARK(1);
            BD_TRY(hipStreamSynchronize(st));
            ss.upload_ms += bd_ms(b, 0, 1);
            for (uint64_t s0 = 0; s0 < n_slots; s0 += piece) {
                const uint64_t m = std::min(piece, n_slots - s0);
                size_t need = 0;
                BD_TRY(prim::exclusive_sum(nullptr, need, flag.as<uint32_t>(), fscan.as<uint32_t>(), m + 1, st));
                if (need > tmp.bytes) BD_DO(tmp.alloc(b->acct, need, "the scan's temporary storage"));
                BD_MARK(0);
                BD_TRY(h2d(chunk.p, v->slots + s0, m * 8));
                BD_MARK(1);
                hipLaunchKernelGGL(bd_seed_flag_kernel, dim3(bd_blocks(m + 1)), dim3(BD_THREADS), 0, st, chunk.as<unsigned long long>(), m, P, flag.as<uint32_t>(), d_bad);
                BD_TRY(prim::exclusive_sum(tmp.p, need, flag.as<uint32_t>(), fscan.as<uint32_t>(), m + 1, st));
                hipLaunchKernelGGL(bd_seed_compact_kernel, dim3(bd_blocks(m)), dim3(BD_THREADS), 0, st, chunk.as<unsigned long long>(), flag.as<uint32_t>(), fscan.as<uint32_t>(), m, s0,
                                   boff.as<unsigned long long>(), nb, found, nD, Kin.as<uint64_t>(), Pin.as<uint32_t>());
                BD_TRY(hipGetLastError());
                BD_MARK(2);
                uint32_t cnt = 0;
                BD_TRY(hipMemcpyAsync(&cnt, fscan.as<uint32_t>() + m, 4, hipMemcpyDeviceToHost, st));
                BD_TRY(hipStreamSynchronize(st));
                found += cnt;
                ss.upload_ms += bd_ms(b, 0, 1);
                ss.dict_ms += bd_ms(b, 1, 2);
            }
        }
        if (found != nD)
            return kmdb_set_error(std::string(who) + ": the database's tables hold " + std::to_string(found) + " k-mers, the num_kmers of its patterns add up to " + std::to_string(nD));
        BD_DO(b->D.alloc(b->acct, nD * 8, "the dictionary"));
        BD_DO(b->cur.alloc(b->acct, nD * 4, "the k-mers' pattern ids"));
        if (nD) {
            BBuf tmp;
            size_t tb = 0;
            BD_TRY(prim::sort_pairs(nullptr, tb, Kin.as<uint64_t>(), b->D.as<uint64_t>(), Pin.as<uint32_t>(), b->cur.as<uint32_t>(), nD, 0, b->kbits, st));
            BD_DO(tmp.alloc(b->acct, tb, "the sort's temporary storage"));
            BD_MARK(0);
            BD_TRY(prim::sort_pairs(tmp.p, tb, Kin.as<uint64_t>(), b->D.as<uint64_t>(), Pin.as<uint32_t>(), b->cur.as<uint32_t>(), nD, 0, b->kbits, st));
            BD_MARK(1);
            BD_TRY(hipStreamSynchronize(st));
            ss.dict_ms += bd_ms(b, 0, 1);
        }
        b->nD = nD;
    }
    // ---- (b) the tree.  b->P is still 1 and b->E 0: bd_reserve allocates, there is nothing to keep
    BD_DO(bd_reserve(b, (P - 1) + (1u << 16), E + (1u << 16)));
    BD_MARK(0);
    BD_TRY(h2d(b->here.p, v->num_kmers, P * 8));
    BD_TRY(h2d(b->parent.p, v->parent_id, P * 8));
    BD_TRY(h2d(b->nsam.p, v->num_samples, P * 4));
    BD_MARK(1);
    BD_TRY(hipMemsetAsync(b->isp.p, 0, P * 4, st));
    hipLaunchKernelGGL(bd_seed_isp_kernel, dim3(bd_blocks(P)), dim3(BD_THREADS), 0, st, b->parent.as<long long>(), P, b->isp.as<uint32_t>(), d_bad);
    BD_TRY(hipGetLastError());
    BD_MARK(2);
    // ---- (d) the dictionary against the tree
    {
        BBuf hist;
        BD_DO(hist.alloc(b->acct, P * 4, "the patterns' k-mer counters"));
        BD_TRY(hipMemsetAsync(hist.p, 0, P * 4, st));
        if (nD) hipLaunchKernelGGL(bd_seed_dict_check_kernel, dim3(bd_blocks(nD)), dim3(BD_THREADS), 0, st, b->D.as<uint64_t>(), b->cur.as<uint32_t>(), nD, b->kbits, P, hist.as<uint32_t>(), d_bad);
        hipLaunchKernelGGL(bd_seed_count_check_kernel, dim3(bd_blocks(P)), dim3(BD_THREADS), 0, st, hist.as<uint32_t>(), b->here.as<long long>(), P, d_bad);
        BD_TRY(hipGetLastError());
        BD_MARK(3);
        BD_TRY(hipStreamSynchronize(st));
    }
    ss.upload_ms += bd_ms(b, 0, 1);
    ss.tree_ms = bd_ms(b, 1, 2);
    ss.check_ms = bd_ms(b, 2, 3);
    // ---- (c) the events from the gamma streams
    uint32_t flags[8] = {0};
    {
        BBuf num_local, estart, last_id, num_bits, data_off, data, tmp;
        BD_DO(num_local.alloc(b->acct, (P + 1) * 4, "num_local"));
        BD_DO(estart.alloc(b->acct, (P + 1) * 4, "the patterns' first events"));
        BD_DO(last_id.alloc(b->acct, P * 4, "last_sample_id"));
        BD_DO(num_bits.alloc(b->acct, P * 4, "num_bits"));
        BD_DO(data_off.alloc(b->acct, P * 8, "data_offset"));
        BD_DO(data.alloc(b->acct, n_words * 8, "the gamma streams"));
        size_t tb = 0;
        BD_TRY(prim::exclusive_sum(nullptr, tb, num_local.as<uint32_t>(), estart.as<uint32_t>(), P + 1, st));
        BD_DO(tmp.alloc(b->acct, tb, "the scan's temporary storage"));
        BD_MARK(0);
        BD_TRY(hipMemsetAsync(num_local.as<uint32_t>() + P, 0, 4, st));
        BD_TRY(h2d(num_local.p, v->num_local, P * 4));
        BD_TRY(h2d(last_id.p, v->last_sample_id, P * 4));
        BD_TRY(h2d(num_bits.p, v->num_bits, P * 4));
        BD_TRY(h2d(data_off.p, v->data_offset, P * 8));
        if (n_words) BD_TRY(h2d(data.p, v->data, n_words * 8));
        BD_MARK(1);
        BD_TRY(prim::exclusive_sum(tmp.p, tb, num_local.as<uint32_t>(), estart.as<uint32_t>(), P + 1, st));
        hipLaunchKernelGGL(bd_seed_decode_kernel, dim3(bd_blocks(P)), dim3(BD_THREADS), 0, st, num_local.as<uint32_t>(), estart.as<uint32_t>(), last_id.as<uint32_t>(), num_bits.as<uint32_t>(),
                           data_off.as<unsigned long long>(), data.as<uint64_t>(), n_words, P, E, N, b->ev_pid.as<uint32_t>(), b->ev_sid.as<uint32_t>(), d_bad);
        BD_TRY(hipGetLastError());
        BD_MARK(2);
        BD_TRY(hipMemcpyAsync(flags, bad.p, sizeof flags, hipMemcpyDeviceToHost, st));
        BD_TRY(hipStreamSynchronize(st));
        ss.upload_ms += bd_ms(b, 0, 1);
        ss.decode_ms = bd_ms(b, 1, 2);
    }
    static const char* const why[8] = {"a value of its tables is 0 or no pattern id", "a k-mer is stored twice in its tables", "a k-mer of its tables is wider than k symbols",
                                       "the k-mers its tables give a pattern differ from the pattern's num_kmers", "a pattern's stream does not end at its num_bits",
                                       "a pattern's sample ids are not strictly ascending below the number of samples", "a pattern's parent_id is not below its own id",
                                       "a pattern's stream lies outside the stream words"};
    for (int i = 0; i < 8; ++i)
        if (flags[i]) return kmdb_set_error(std::string(who) + ": the database cannot seed a builder: " + why[i]);
    b->P = P;
    b->E = E;
    for (uint64_t i = 0; i < N; ++i) { b->names.emplace_back(kmdbh_db_sample_name(plan.db, i)); b->counts.push_back(kmdbh_db_sample_kmers(plan.db, i)); }
    ss.samples = N; ss.distinct_kmers = nD; ss.patterns = P; ss.events = E;
    return 0;
}

// what can be refused before any device work
int bd_begin_from_db(const kmdbh_db* db, const kmdb_opts* opts, kmdb_builder** out) {
    const char* who = "kmdb_build_begin_from_db";
    if (!out) return kmdb_set_error(std::string(who) + ": null argument");
    *out = nullptr;
    if (!db) return kmdb_set_error(std::string(who) + ": null argument");
    BdSeedPlan plan{db, kmdbh_db_view(db), 0, 0, 0};
    const kmdb_db_view* v = plan.v;
    if (!v->n_buckets || !v->bucket_offset || !v->slots)
        return kmdb_set_error(std::string(who) + ": the database holds no hashtables (it was loaded with SkipHashtables): the k-mers of its patterns are in them");
    const uint64_t P = v->n_patterns;
    if (!P) return kmdb_set_error(std::string(who) + ": the database holds no pattern, not even the empty one");
    if (v->n_samples >= 0xFFFFFFFFull) return kmdb_set_error(std::string(who) + ": 2^32 samples or more");
    if (P >= 0x7FFFFFFFull) return kmdb_set_error(std::string(who) + ": 2^31 patterns or more: pattern ids are 31 bits wide (hashmap_lp.h:78)");
    for (uint64_t p = 0; p < P; ++p) {
        if (v->num_kmers[p] < 0) return kmdb_set_error(std::string(who) + ": a pattern with a negative num_kmers");
        plan.nD += (uint64_t)v->num_kmers[p];
        plan.E += v->num_local[p];
        if (plan.nD >= 0x7FFFFFFFull) return kmdb_set_error(std::string(who) + ": 2^31 distinct k-mers or more: the seed's sort takes 31-bit sizes");
        if (plan.E >= 0x7FFFFFFFull) return kmdb_set_error(std::string(who) + ": 2^31 (pattern, sample) events or more: the sort at finish takes 31-bit sizes");
    }
    plan.n_slots = v->bucket_offset[v->n_buckets];
    const uint32_t k = kmdbh_db_kmer_length(db);
    const int32_t alphabet = kmdbh_db_alphabet(db);
    int8_t map[256];
    uint32_t size = 0, bits = 0;
    if (alphabet >= 0 && alphabet < KMDB_ALPHABET_COUNT && !kmdbh_alphabet_table(alphabet, map, &size, &bits, nullptr)) {
        const uint64_t want = 1ull << std::max(8, (int)(bits * k) - 32);                  // prefix_kmer_db.cpp:54-62
        if (v->n_buckets != want)
            return kmdb_set_error(std::string(who) + ": the database has " + std::to_string(v->n_buckets) + " prefix buckets, k = " + std::to_string(k) + " takes " + std::to_string(want));
    }                                                                                      // (an unknown alphabet is refused by bd_begin)
    return bd_begin(who, k, kmdbh_db_fraction(db), kmdbh_db_start_fraction(db), alphabet, opts, &plan, out);
}

// the pieces of a call: [s0, s1) with at most BD_PIECE_KMERS k-mers (a longer sample alone) and BD_PIECE_SAMPLES non-empty samples
template <class CountOf>
size_t bd_piece_end(size_t s0, size_t n, CountOf&& count_of) {
    uint64_t T = 0;
    size_t nonempty = 0, s1 = s0;
    while (s1 < n) {
        const uint64_t c = count_of(s1);
        if (s1 > s0 && c && (T + c > BD_PIECE_KMERS || nonempty + 1 > BD_PIECE_SAMPLES)) break;
        T += c; nonempty += c != 0; ++s1;
    }
    return s1;
}

int bd_add_kmers(kmdb_builder* b, const char* const* names, const uint64_t* const* kmers, const size_t* counts, size_t n) {
    const char* who = "kmdb_build_add_kmers";
    BD_DO(bd_usable(b, who));
    if (n && (!names || !kmers || !counts)) return kmdb_set_error(std::string(who) + ": null argument");
    for (size_t s = 0; s < n; ++s) {
        if (!names[s] || (counts[s] && !kmers[s])) return kmdb_set_error(std::string(who) + ": null argument");
        if (counts[s] >= (1ull << 31))
            return kmdb_set_error(std::string(who) + ": sample " + names[s] + " has 2^31 k-mers or more (the reference's count is 32 bits; this builder indexes a sample with 31)");
    }
    if (b->names.size() + n >= 0xFFFFFFFFull) return kmdb_set_error(std::string(who) + ": 2^32 samples or more");
    BD_TRY(hipSetDevice(b->device));
    hipStream_t st = b->st;
    auto count_of = [&](size_t s) { return (uint64_t)counts[s]; };
    const bool one_piece = bd_piece_end(0, n, count_of) == n;
    // pass 0 checks every piece on the device before the state changes; pass 1 adds.  A call of one piece uploads once.
    for (int pass = one_piece ? 1 : 0; pass < 2; ++pass) {
        for (size_t s0 = 0; s0 < n;) {
            const size_t s1 = bd_piece_end(s0, n, count_of), m = s1 - s0;
            std::vector<uint64_t> off(m + 1, 0);
            for (size_t s = 0; s < m; ++s) off[s + 1] = off[s] + counts[s0 + s];
            const uint64_t T = off[m];
            if (T) {
                BBuf K, d_off, bad;
                struct Dead { kmdb_builder* b; bool armed; ~Dead() { if (armed) b->dead = true; } } dead{b, pass == 1};      // an error from here on leaves the state half-changed
                BD_DO(K.alloc(b->acct, T * 8, "the call's k-mers"));
                for (size_t s = 0; s < m; ++s)
                    if (counts[s0 + s]) BD_TRY(hipMemcpyAsync(K.as<uint64_t>() + off[s], kmers[s0 + s], counts[s0 + s] * 8, hipMemcpyHostToDevice, st));
                if (pass == 0 || one_piece) {
                    BD_DO(d_off.alloc(b->acct, (m + 1) * 8, "the samples' offsets"));
                    BD_DO(bad.alloc(b->acct, 4, "a flag"));
                    BD_TRY(hipMemcpyAsync(d_off.p, off.data(), (m + 1) * 8, hipMemcpyHostToDevice, st));
                    BD_TRY(hipMemsetAsync(bad.p, 0xFF, 4, st));
                    hipLaunchKernelGGL(bd_check_kernel, dim3(bd_blocks(T)), dim3(BD_THREADS), 0, st, K.as<uint64_t>(), T, d_off.as<uint64_t>(), (uint32_t)m, bad.as<uint32_t>());
                    BD_TRY(hipGetLastError());
                    uint32_t first_bad = 0xFFFFFFFFu;
                    BD_TRY(hipMemcpyAsync(&first_bad, bad.p, 4, hipMemcpyDeviceToHost, st));
                    BD_TRY(hipStreamSynchronize(st));
                    if (first_bad != 0xFFFFFFFFu) {
                        dead.armed = false;            // nothing was added yet: the builder stays as it was
                        return kmdb_set_error(std::string(who) + ": the k-mers of sample " + names[s0 + std::min<size_t>(first_bad, m - 1)] +
                                              " are not strictly ascending (sort them and drop the duplicates: kmdbh_sort_unique)");
                    }
                }
                if (pass == 1) BD_DO(bd_add_device(b, K.as<uint64_t>(), off.data(), m, b->names.size()));
                dead.armed = false;
            }
            if (pass == 1)
                for (size_t s = s0; s < s1; ++s) { b->names.emplace_back(names[s]); b->counts.push_back(counts[s]); b->stats.kmers_added += counts[s]; }
            s0 = s1;
        }
    }
    return 0;
}

int bd_add_seq(kmdb_builder* b, const char* const* names, const char* const* seqs, const size_t* seq_lens, size_t n) {
    const char* who = "kmdb_build_add_seq_alphabet";
    BD_DO(bd_usable(b, who));
    if (n && (!names || !seqs || !seq_lens)) return kmdb_set_error(std::string(who) + ": null argument");
    for (size_t s = 0; s < n; ++s)
        if (!names[s]) return kmdb_set_error(std::string(who) + ": null argument");
    if (b->names.size() + n >= 0xFFFFFFFFull) return kmdb_set_error(std::string(who) + ": 2^32 samples or more");
    kmdb_opts o{};
    o.abi_version = KMDB_ABI_VERSION; o.device = b->device; o.shard_count = 1; o.stream = (void*)b->st;
    size_t done = 0;
    bool touched = false;
    // the extractor hands over its pieces in input order; a piece of the extractor may still be cut into pieces of the builder
    kmdb_device_lists_sink sink = [&](const uint64_t* d_kmers, const uint64_t* off, size_t m, void*) -> int {
        touched = true;
        auto count_of = [&](size_t s) { return off[s + 1] - off[s]; };
        for (size_t s0 = 0; s0 < m;) {
            const size_t s1 = bd_piece_end(s0, m, count_of);
            std::vector<uint64_t> rel(s1 - s0 + 1, 0);
            for (size_t s = s0; s < s1; ++s) {
                if (count_of(s) >= (1ull << 31)) return kmdb_set_error(std::string(who) + ": sample " + names[done + s] + " has 2^31 k-mers or more");
                rel[s - s0 + 1] = off[s + 1] - off[s0];
            }
            BD_DO(bd_add_device(b, rel.back() ? d_kmers + off[s0] : nullptr, rel.data(), s1 - s0, b->names.size()));
            for (size_t s = s0; s < s1; ++s) { b->names.emplace_back(names[done + s]); b->counts.push_back(count_of(s)); b->stats.kmers_added += count_of(s); }
            s0 = s1;
        }
        done += m;
        return 0;
    };
    const int rc = kmdb_minhash_device_lists(who, seqs, seq_lens, n, b->k, b->fraction, b->start_fraction, b->alphabet, &o, sink);
    if (rc && touched) b->dead = true;                 // (a refusal of the extractor's own checks comes before the first piece)
    return rc;
}

// what the finish stages (c) and (d) leave in HBM: the rest of a stored database next to the builder's own here / parent / nsam
struct BdFinish {
    BBuf flag;                     // [0] a stream of 2^32 bits or more, [1] a k-mer outside the prefix buckets
    BBuf num_local, last_id, num_bits, data_off, data;
    uint64_t n_words = 0;
    BBuf boff, slots;
    uint64_t nb = 0, n_slots = 0;  // nb == 0: stage (d) has not run
};

// (c); HIP events e0, e0 + 1 around it
int bd_finish_encode(kmdb_builder* b, const char* who, BdFinish& f, size_t e0) {
    hipStream_t st = b->st;
    const uint64_t P = b->P, E = b->E;
    BD_MARK(e0);
    // ---- (c) the gamma streams
    BBuf spid, ssid, clen, bitpos, words, pbit0;
    BBuf &num_local = f.num_local, &last_id = f.last_id, &num_bits = f.num_bits, &data_off = f.data_off, &data = f.data, &flag = f.flag;
    BD_DO(flag.alloc(b->acct, 8, "two flags"));
    BD_TRY(hipMemsetAsync(flag.p, 0, 8, st));
    BD_DO(spid.alloc(b->acct, (E + 1) * 4, "the sorted events' patterns"));
    BD_DO(ssid.alloc(b->acct, (E + 1) * 4, "the sorted events' samples"));
    BD_DO(clen.alloc(b->acct, (E + 1) * 8, "the codes' lengths"));
    BD_DO(bitpos.alloc(b->acct, (E + 1) * 8, "the codes' bit positions"));
    if (E) {
        BBuf tmp;
        size_t tb = 0;
        BD_TRY(prim::sort_pairs(nullptr, tb, b->ev_pid.as<uint32_t>(), spid.as<uint32_t>(), b->ev_sid.as<uint32_t>(), ssid.as<uint32_t>(), E, 0, bd_bits(P), st));
        BD_DO(tmp.alloc(b->acct, tb, "the sort's temporary storage"));
        BD_TRY(prim::sort_pairs(tmp.p, tb, b->ev_pid.as<uint32_t>(), spid.as<uint32_t>(), b->ev_sid.as<uint32_t>(), ssid.as<uint32_t>(), E, 0, bd_bits(P), st));
        BD_TRY(hipStreamSynchronize(st));
    }
    b->ev_pid.release();                               // the builder takes no more samples: the unsorted events are done with
    b->ev_sid.release();
    hipLaunchKernelGGL(bd_code_len_kernel, dim3(bd_blocks(E + 1)), dim3(BD_THREADS), 0, st, spid.as<uint32_t>(), ssid.as<uint32_t>(), E, clen.as<unsigned long long>());
    BD_TRY(hipGetLastError());
    {
        BBuf tmp;
        size_t tb = 0;
        BD_TRY(prim::exclusive_sum(nullptr, tb, clen.as<unsigned long long>(), bitpos.as<unsigned long long>(), E + 1, st));
        BD_DO(tmp.alloc(b->acct, tb, "the scan's temporary storage"));
        BD_TRY(prim::exclusive_sum(tmp.p, tb, clen.as<unsigned long long>(), bitpos.as<unsigned long long>(), E + 1, st));
        BD_TRY(hipStreamSynchronize(st));
    }
    clen.release();
    BD_DO(num_local.alloc(b->acct, P * 4, "num_local"));
    BD_DO(last_id.alloc(b->acct, P * 4, "last_sample_id"));
    BD_DO(num_bits.alloc(b->acct, P * 4, "num_bits"));
    BD_DO(words.alloc(b->acct, (P + 1) * 8, "the streams' lengths"));
    BD_DO(pbit0.alloc(b->acct, (P + 1) * 8, "the streams' first bits"));
    BD_DO(data_off.alloc(b->acct, (P + 1) * 8, "data_offset"));
    hipLaunchKernelGGL(bd_pattern_fields_kernel, dim3(bd_blocks(P + 1)), dim3(BD_THREADS), 0, st, spid.as<uint32_t>(), ssid.as<uint32_t>(), E, bitpos.as<unsigned long long>(), P,
                       num_local.as<uint32_t>(), last_id.as<uint32_t>(), num_bits.as<uint32_t>(), words.as<unsigned long long>(), pbit0.as<unsigned long long>(), flag.as<uint32_t>());
    BD_TRY(hipGetLastError());
    uint64_t& n_words = f.n_words;
    {
        BBuf tmp;
        size_t tb = 0;
        BD_TRY(prim::exclusive_sum(nullptr, tb, words.as<unsigned long long>(), data_off.as<unsigned long long>(), P + 1, st));
        BD_DO(tmp.alloc(b->acct, tb, "the scan's temporary storage"));
        BD_TRY(prim::exclusive_sum(tmp.p, tb, words.as<unsigned long long>(), data_off.as<unsigned long long>(), P + 1, st));
        uint32_t too_long = 0;
        BD_TRY(hipMemcpyAsync(&n_words, data_off.as<uint64_t>() + P, 8, hipMemcpyDeviceToHost, st));
        BD_TRY(hipMemcpyAsync(&too_long, flag.p, 4, hipMemcpyDeviceToHost, st));
        BD_TRY(hipStreamSynchronize(st));
        if (too_long) return kmdb_set_error(std::string(who) + ": a pattern's stream has 2^32 bits or more (num_bits is 32 bits wide, pattern.h:49)");
    }
    BD_DO(data.alloc(b->acct, (n_words + 2) * 8, "the gamma streams"));
    BD_TRY(hipMemsetAsync(data.p, 0, (n_words + 2) * 8, st));
    if (E) hipLaunchKernelGGL(bd_write_codes_kernel, dim3(bd_blocks(E)), dim3(BD_THREADS), 0, st, spid.as<uint32_t>(), ssid.as<uint32_t>(), E, bitpos.as<unsigned long long>(),
                              pbit0.as<unsigned long long>(), data_off.as<unsigned long long>(), data.as<unsigned long long>(), n_words);
    BD_TRY(hipGetLastError());
    BD_MARK(e0 + 1);
    BD_TRY(hipStreamSynchronize(st));
    spid.release(); ssid.release(); bitpos.release(); words.release(); pbit0.release();
    return 0;
}

// (d); HIP events e0, e0 + 1 around it
int bd_finish_tables(kmdb_builder* b, const char* who, BdFinish& f, size_t e0) {
    hipStream_t st = b->st;
    const uint64_t nD = b->nD;
    BD_MARK(e0);
    // ---- (d) the tables
    const int prefix_bits = std::max(8, (int)(b->bits * b->k) - 32);                      // prefix_kmer_db.cpp:54-62
    const uint64_t nb = f.nb = 1ull << prefix_bits;
    BBuf bstart, caps;
    BBuf &boff = f.boff, &slots = f.slots, &flag = f.flag;
    BD_DO(bstart.alloc(b->acct, (nb + 1) * 8, "the buckets' first k-mers"));
    BD_DO(caps.alloc(b->acct, (nb + 1) * 8, "the buckets' capacities"));
    BD_DO(boff.alloc(b->acct, (nb + 1) * 8, "bucket_offset"));
    hipLaunchKernelGGL(bd_bucket_starts_kernel, dim3(bd_blocks(nb + 1)), dim3(BD_THREADS), 0, st, b->D.as<uint64_t>(), nD, nb, bstart.as<unsigned long long>());
    hipLaunchKernelGGL(bd_bucket_caps_kernel, dim3(bd_blocks(nb + 1)), dim3(BD_THREADS), 0, st, bstart.as<unsigned long long>(), nb, caps.as<unsigned long long>());
    BD_TRY(hipGetLastError());
    uint64_t& n_slots = f.n_slots;
    {
        BBuf tmp;
        size_t tb = 0;
        BD_TRY(prim::exclusive_sum(nullptr, tb, caps.as<unsigned long long>(), boff.as<unsigned long long>(), nb + 1, st));
        BD_DO(tmp.alloc(b->acct, tb, "the scan's temporary storage"));
        BD_TRY(prim::exclusive_sum(tmp.p, tb, caps.as<unsigned long long>(), boff.as<unsigned long long>(), nb + 1, st));
        BD_TRY(hipMemcpyAsync(&n_slots, boff.as<uint64_t>() + nb, 8, hipMemcpyDeviceToHost, st));
        BD_TRY(hipStreamSynchronize(st));
    }
    bstart.release(); caps.release();
    BD_DO(slots.alloc(b->acct, n_slots * 8, "the hashtables' slots"));
    hipLaunchKernelGGL(bd_fill_empty_kernel, dim3(bd_blocks(n_slots)), dim3(BD_THREADS), 0, st, slots.as<unsigned long long>(), n_slots);
    if (nD) hipLaunchKernelGGL(bd_insert_kernel, dim3(bd_blocks(nD)), dim3(BD_THREADS), 0, st, b->D.as<uint64_t>(), b->cur.as<uint32_t>(), nD, nb, boff.as<unsigned long long>(),
                               slots.as<unsigned long long>(), flag.as<uint32_t>() + 1);
    BD_TRY(hipGetLastError());
    BD_MARK(e0 + 1);
    uint32_t failed = 0;
    BD_TRY(hipMemcpyAsync(&failed, flag.as<uint32_t>() + 1, 4, hipMemcpyDeviceToHost, st));
    BD_TRY(hipStreamSynchronize(st));
    if (failed) return kmdb_set_error(std::string(who) + ": a k-mer does not fit the prefix buckets of k = " + std::to_string(b->k) + " (the lists were made with another k or alphabet)");
    return 0;
}

// (e); HIP events e0, e0 + 1 around it.  *out is the caller's to free.
int bd_finish_copy_back(kmdb_builder* b, BdFinish& f, size_t e0, kmdbh_db** out) {
    hipStream_t st = b->st;
    const uint64_t P = b->P, nD = b->nD, n_words = f.n_words, nb = f.nb, n_slots = f.n_slots;
    BBuf &num_local = f.num_local, &last_id = f.last_id, &num_bits = f.num_bits, &data_off = f.data_off, &data = f.data, &boff = f.boff, &slots = f.slots;
    BD_MARK(e0);
    // ---- (e) to the host
    kmdbh_db_arrays a{};
    std::vector<std::string> names = b->names;
    std::vector<uint64_t> counts = b->counts;
    kmdbh_db* h = kmdbh_db_make(b->k, b->fraction, b->start_fraction, b->alphabet, nD, std::move(names), std::move(counts), P, n_words, nb, n_slots, &a);
    if (!h) return 1;
    struct HoldDb { kmdbh_db* h; ~HoldDb() { if (h) kmdbh_db_free(h); } } hold{h};
    BD_TRY(hipMemcpyAsync(a.num_kmers, b->here.p, P * 8, hipMemcpyDeviceToHost, st));
    BD_TRY(hipMemcpyAsync(a.parent_id, b->parent.p, P * 8, hipMemcpyDeviceToHost, st));
    BD_TRY(hipMemcpyAsync(a.num_samples, b->nsam.p, P * 4, hipMemcpyDeviceToHost, st));
    BD_TRY(hipMemcpyAsync(a.num_local, num_local.p, P * 4, hipMemcpyDeviceToHost, st));
    BD_TRY(hipMemcpyAsync(a.last_sample_id, last_id.p, P * 4, hipMemcpyDeviceToHost, st));
    BD_TRY(hipMemcpyAsync(a.num_bits, num_bits.p, P * 4, hipMemcpyDeviceToHost, st));
    BD_TRY(hipMemcpyAsync(a.data_offset, data_off.p, P * 8, hipMemcpyDeviceToHost, st));
    BD_TRY(hipMemcpyAsync(a.data, data.p, (n_words + 2) * 8, hipMemcpyDeviceToHost, st));
    BD_TRY(hipMemcpyAsync(a.bucket_offset, boff.p, (nb + 1) * 8, hipMemcpyDeviceToHost, st));
    if (n_slots) BD_TRY(hipMemcpyAsync(a.slots, slots.p, n_slots * 8, hipMemcpyDeviceToHost, st));
    BD_MARK(e0 + 1);
    BD_TRY(hipStreamSynchronize(st));
    hold.h = nullptr;
    *out = h;
    return 0;
}

int bd_finish(kmdb_builder* b, kmdbh_db** out) {
    const char* who = "kmdb_build_finish";
    if (!out) return kmdb_set_error(std::string(who) + ": null argument");
    *out = nullptr;
    BD_DO(bd_usable(b, who));
    BD_TRY(hipSetDevice(b->device));
    b->finished = true;
    struct Dead { kmdb_builder* b; bool armed = true; ~Dead() { if (armed) b->dead = true; } } dead{b};
    BdFinish f;
    BD_DO(bd_finish_encode(b, who, f, 0));
    BD_DO(bd_finish_tables(b, who, f, 2));
    BD_DO(bd_finish_copy_back(b, f, 4, out));
    b->stats.encode_ms = bd_ms(b, 0, 1);
    b->stats.tables_ms = bd_ms(b, 2, 3);
    b->stats.copy_back_ms = bd_ms(b, 4, 5);
    dead.armed = false;
    return 0;
}

// kmdb_build_finish_device: stages (c) and, when somebody reads the tables, (d); then the engine's layout straight from the builder's arrays
// (kmdb_db_from_device); then, for a full host image, (e).  Every array of the builder goes as soon as its last reader has run.
int bd_finish_device(kmdb_builder* b, const kmdb_opts* opts, int with_hashtables, int host_image, kmdb_db** out_db, kmdbh_db** out_host) {
    const char* who = "kmdb_build_finish_device";
    if (out_host) *out_host = nullptr;
    if (!out_db) return kmdb_set_error(std::string(who) + ": null argument");
    *out_db = nullptr;
    BD_DO(bd_usable(b, who));
    // what kmdb_db_upload refuses of the finished database, with its messages, and a foreign device: found before the state is touched, the
    // builder stays as it was (kmdb_build_finish still serves it)
    if (opts && opts->abi_version && !kmdb_abi_compatible(opts->abi_version)) return kmdb_set_error(std::string(who) + ": kmdb_opts.abi_version is not served by this library");
    if (opts && (opts->flags & ~KMDB_FLAG_ALL)) return kmdb_set_error("kmdb_db_upload: unknown bits in kmdb_opts.flags");
    if (b->P >= (1ull << 31)) return kmdb_set_error("kmdb_db_upload: more than 2^31 patterns");
    if (b->names.size() >= KMDB_MAX_SAMPLES)
        return kmdb_set_error("kmdb_db_upload: " + std::to_string(KMDB_MAX_SAMPLES) + " samples or more are not supported (sample ids take " + std::to_string(KMDB_ID_BITS) + " bits in the device layout)");
    if ((opts ? opts->device : 0) != b->device)
        return kmdb_set_error(std::string(who) + ": kmdb_opts.device is " + std::to_string(opts ? opts->device : 0) + ", the builder lives on device " + std::to_string(b->device) +
                              " (the hand-off moves nothing between devices)");
    BD_TRY(hipSetDevice(b->device));
    hipStream_t st = b->st;
    b->finished = true;
    struct Dead { kmdb_builder* b; bool armed = true; ~Dead() { if (armed) b->dead = true; } } dead{b};
    DevMemMeter meter;
    meter.live = meter.peak = (long long)b->acct.live;
    struct Metered { DevMemMeter* was; explicit Metered(DevMemMeter* m) : was(dev_mem_meter) { dev_mem_meter = m; } ~Metered() { dev_mem_meter = was; } } metered{&meter};
    const auto t0 = std::chrono::steady_clock::now();
    kmdb_build_handoff_stats& hs = b->handoff;
    hs = kmdb_build_handoff_stats{};
    hs.with_hashtables = with_hashtables ? 1 : 0; hs.host_image = host_image ? 1 : 0;
    const bool tables = with_hashtables || host_image;
    BdFinish f;
    BD_DO(bd_finish_encode(b, who, f, 0));
    if (tables) BD_DO(bd_finish_tables(b, who, f, 2));
    b->D.release();                                    // the dictionary and its pattern ids: read by stage (d) only
    b->cur.release();
    BD_TRY(hipStreamSynchronize(st));
    kmdb_layout_device_source src;
    src.n_patterns = b->P; src.n_samples = b->names.size(); src.kmer_length = b->k;
    src.num_kmers = b->here.as<long long>(); src.parent_id = b->parent.as<long long>(); src.num_samples = b->nsam.as<uint32_t>();
    src.num_local = f.num_local.as<uint32_t>(); src.last_sample_id = f.last_id.as<uint32_t>(); src.num_bits = f.num_bits.as<uint32_t>();
    src.data_offset = f.data_off.as<unsigned long long>(); src.data = f.data.as<uint64_t>(); src.n_data_words = f.n_words;
    if (with_hashtables) { src.n_buckets = f.nb; src.n_slots = f.n_slots; src.bucket_offset = f.boff.as<uint64_t>(); src.slots = f.slots.as<uint64_t>(); }
    if (!host_image) {
        src.tables_done = [&] { f.boff.release(); f.slots.release(); };
        src.fields_done = [&] { b->here.release(); b->parent.release(); b->nsam.release(); b->isp.release(); f.num_local.release(); f.last_id.release(); f.num_bits.release(); f.data_off.release(); };
        src.streams_done = [&] { f.data.release(); };
    }
    kmdb_db* db = nullptr;
    BD_DO(kmdb_db_from_device(&src, opts, with_hashtables, &db));
    struct HoldHandle { kmdb_db* db; ~HoldHandle() { if (db) kmdb_db_free(db); } } hold_db{db};
    kmdbh_db* h = nullptr;
    if (host_image) {
        BD_DO(bd_finish_copy_back(b, f, 4, &h));
        hs.copy_back_ms = bd_ms(b, 4, 5);
        hs.d2h_bytes = b->P * 40 + (f.n_words + 2) * 8 + (f.nb + 1) * 8 + f.n_slots * 8;
    } else if (out_host) {
        kmdbh_db_arrays a{};
        std::vector<std::string> names = b->names;
        std::vector<uint64_t> counts = b->counts;
        h = kmdbh_db_make(b->k, b->fraction, b->start_fraction, b->alphabet, b->nD, std::move(names), std::move(counts), 0, 0, 0, 0, &a);
        if (!h) return 1;
    }
    hs.patterns = b->P; hs.samples = b->names.size();
    hs.encode_ms = bd_ms(b, 0, 1);
    hs.tables_ms = tables ? bd_ms(b, 2, 3) : 0.0;
    hs.fields_ms = src.fields_ms;
    hs.layout_ms = src.layout_ms - src.fields_ms;
    hs.prepare_ms = src.prepare_ms;
    hs.total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    hs.peak_device_bytes = (uint64_t)meter.peak;
    kmdb_stats ds{};
    if (!kmdb_db_stats(db, &ds)) hs.handle_device_bytes = ds.device_bytes;
    b->stats.encode_ms = hs.encode_ms; b->stats.tables_ms = hs.tables_ms; b->stats.copy_back_ms = hs.copy_back_ms;
    dead.armed = false;
    hold_db.db = nullptr;
    *out_db = db;
    if (out_host) *out_host = h;
    else if (h) kmdbh_db_free(h);
    return 0;
}

}  // namespace

#define BD_GUARD(who, call)                                                          \
    try {                                                                            \
        return call;                                                                 \
    } catch (const std::exception& e) {                                              \
        return kmdb_set_error(std::string(who) + ": " + e.what());                   \
    }

extern "C" int kmdb_build_begin(uint32_t kmer_length, double fraction, double start_fraction, int32_t alphabet, const kmdb_opts* opts, kmdb_builder** out) {
    BD_GUARD("kmdb_build_begin", bd_begin("kmdb_build_begin", kmer_length, fraction, start_fraction, alphabet, opts, nullptr, out))
}
extern "C" int kmdb_build_begin_from_db(const kmdbh_db* db, const kmdb_opts* opts, kmdb_builder** out) {
    BD_GUARD("kmdb_build_begin_from_db", bd_begin_from_db(db, opts, out))
}
extern "C" int kmdb_build_seed_stats_get(const kmdb_builder* b, kmdb_build_seed_stats* out) {
    if (!b || !out) return kmdb_set_error("kmdb_build_seed_stats_get: null argument");
    *out = b->seed;
    return 0;
}
extern "C" int kmdb_build_add_kmers(kmdb_builder* b, const char* const* names, const uint64_t* const* kmers, const size_t* counts, size_t n_samples) {
    BD_GUARD("kmdb_build_add_kmers", bd_add_kmers(b, names, kmers, counts, n_samples))
}
extern "C" int kmdb_build_add_seq_alphabet(kmdb_builder* b, const char* const* names, const char* const* seqs, const size_t* seq_lens, size_t n_samples) {
    BD_GUARD("kmdb_build_add_seq_alphabet", bd_add_seq(b, names, seqs, seq_lens, n_samples))
}
extern "C" int kmdb_build_finish(kmdb_builder* b, kmdbh_db** out) {
    BD_GUARD("kmdb_build_finish", bd_finish(b, out))
}
extern "C" int kmdb_build_finish_device(kmdb_builder* b, const kmdb_opts* opts, int with_hashtables, int host_image, kmdb_db** out_db, kmdbh_db** out_host) {
    BD_GUARD("kmdb_build_finish_device", bd_finish_device(b, opts, with_hashtables, host_image, out_db, out_host))
}
extern "C" int kmdb_build_handoff_stats_get(const kmdb_builder* b, kmdb_build_handoff_stats* out) {
    if (!b || !out) return kmdb_set_error("kmdb_build_handoff_stats_get: null argument");
    *out = b->handoff;
    return 0;
}
extern "C" void kmdb_build_free(kmdb_builder* b) {
    if (!b) return;
    (void)hipSetDevice(b->device);
    delete b;
}
extern "C" int kmdb_build_stats_get(const kmdb_builder* b, kmdb_build_stats* out) {
    if (!b || !out) return kmdb_set_error("kmdb_build_stats_get: null argument");
    *out = b->stats;
    out->samples = b->names.size();
    out->distinct_kmers = b->nD;
    out->patterns = b->P;
    out->events = b->E;
    out->peak_device_bytes = std::max<uint64_t>(b->acct.peak, b->handoff.peak_device_bytes);
    return 0;
}
