// new2all_sparse.hip — the sparse, filtered form of new2all behind kmdb_new2all_batch_sparse_filtered and its relatives (include/kmdb_amd.h).
//
// Replaces one2all_sp FOLLOWED BY the CombinedFilter of the query row (reference src/similarity_calculator.cpp:929-1051;
// src/console_new2all.cpp:76-78, 130-148): the reference keeps, per query, the samples with a non-zero count that pass -min / -max.  The
// rows of a batch are accumulated in HBM by the walk of new2all.hip (kmdb_new2all_batch*_device) and compacted where they are:
//   count    one wave per SEGMENT of N2S_SEG columns of one row, 64 columns per round: cells that are non-zero and pass the widened bounds
//            (cell_filter.h; a = the QUERY's k-mer count, b = the sample's), ranked by ballot and popcount; one count per segment
//   scan     exclusive sum over the nq * nseg + 1 counts; row_ptr[q] = the scan at the row's first segment
//   compact  the same pass again: (col, val) at scan + running rank — ascending columns follow from the order of segments and rounds
// Only row_ptr and 8 bytes per device-kept cell cross PCIe; the exact decision is the host's (kmdb_sparse_decide, engine.hip).
// The cells are a FLAT range [cell_lo, cell_hi) of the row-major nq x N rectangle (cell q * N + s = query q, sample s): a device of a
// node compacts its reduce-scatter chunk as it is (node.hip), the convention of kmdb_sparse_from_dense_device.
#include "kmdb_amd.h"
#include "kmdb_internal.h"
#include "engine_internal.h"

#include <hip/hip_runtime.h>
#include "prim.h"
#include "cell_filter.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

namespace {

// (N2S_SEG, the columns per segment, lives in cell_filter.h: the row select of sample_rows.hip cuts the same rows the same way)

// One wave per segment `seg0 + blockIdx.x` = row * nseg + s: the columns [s * N2S_SEG, min(N, (s + 1) * N2S_SEG)) of query `row`.  `cells`
// points at cell cell_lo.  A lane whose column is beyond the row, or whose cell lies outside [cell_lo, cell_hi), loads nothing: that address
// is a cell of the next row, of another device's chunk, or of nothing at all.  Cell offsets are 64-bit.  Rows start at any multiple of 4
// bytes (N odd): plain coalesced 4-byte loads.  COMPACT false: seg_cnt[seg] = kept cells; true: (col, val) from seg_ptr[seg] on.
template <bool COMPACT>
__global__ __launch_bounds__(64) void n2s_segments_kernel(const uint32_t* __restrict__ cells, uint32_t N, uint32_t nseg, uint64_t seg0, uint64_t seg_end,
                                                          uint64_t cell_lo, uint64_t cell_hi, unsigned long long* __restrict__ seg_cnt,
                                                          const unsigned long long* __restrict__ seg_ptr, uint32_t* __restrict__ col,
                                                          uint32_t* __restrict__ val, const DevFilter f, const uint32_t* __restrict__ sample_counts) {
    const uint64_t seg = seg0 + blockIdx.x;
    if (seg >= seg_end) return;
    const uint32_t lane = threadIdx.x;
    const uint32_t row = (uint32_t)(seg / nseg), s = (uint32_t)(seg - (uint64_t)row * nseg);
    const uint32_t c0 = s * N2S_SEG, c1 = N - c0 < N2S_SEG ? N : c0 + N2S_SEG;      // (s < nseg: c0 < N)
    const uint64_t base = (uint64_t)row * N;
    const uint32_t a = f.n ? f.counts[row] : 0u;                 // the QUERY's k-mer count: first, as in CombinedFilter(..., queryKmersCounts, db counts, ...)
    unsigned long long out = COMPACT ? seg_ptr[seg] : 0ull;
    uint32_t count = 0;
    for (uint32_t j0 = c0; j0 < c1; j0 += 64u) {
        const uint32_t j = j0 + lane;
        const uint64_t cell = base + j;
        uint32_t v = 0;
        if (j < c1 && cell >= cell_lo && cell < cell_hi) v = cells[cell - cell_lo];
        unsigned long long bal = __ballot(v != 0);
        if (!bal) continue;                                      // (most rounds of a sparse row: nothing to filter, nothing to rank)
        if (f.n) {
            if (v && !dev_keep_ab(f, v, a, sample_counts[j])) v = 0u;
            bal = __ballot(v != 0);
        }
        if (COMPACT) {
            if (v) { const unsigned long long o = out + (uint32_t)__popcll(bal & ((1ull << lane) - 1ull)); col[o] = j; val[o] = v; }
            out += (uint32_t)__popcll(bal);
        } else count += (uint32_t)__popcll(bal);
    }
    if (!COMPACT && lane == 0) seg_cnt[seg] = count;
}

// row_ptr[q] = the scan at the first segment of row q; row_ptr[nq] = the scan's last entry, the total
__global__ void n2s_row_ptr_kernel(const unsigned long long* __restrict__ seg_ptr, uint32_t nseg, uint64_t nq, unsigned long long* __restrict__ row_ptr) {
    const uint64_t q = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q <= nq) row_ptr[q] = seg_ptr[q * nseg];
}


hipStream_t stream_of(const kmdb_engine_view& e, const kmdb_opts* opts) { return (opts && opts->stream) ? (hipStream_t)opts->stream : (hipStream_t)e.stream; }

}  // namespace

// what every entry refuses on its arguments alone, before the handle is looked at
static int n2s_check_args(const char* who, const void* handle, const kmdb_sparse_rows* out, const kmdb_cell_filter* filters, size_t n_filters,
                          const uint32_t* sample_kmers, int measure) {
    if (!handle || !out) return kmdb_set_error(std::string(who) + ": null argument");
    return kmdb_check_filters(who, filters, n_filters, sample_kmers, measure);
}

// The device half: count, scan, compact, copy back.  `out` is zeroed here and freed on failure.  The cells must be complete on `st`.
int kmdb_n2a_rows_compact(const char* who_, kmdb_db* db, const uint32_t* cells_dev, size_t nq, uint64_t cell_lo, uint64_t cell_hi, const uint32_t* query_kmers,
                          const kmdb_cell_filter* filters, size_t n_filters, const uint32_t* sample_kmers, kmdb_sparse_rows* out, const kmdb_opts* opts,
                          kmdb_new2all_sparse_stats* stats) {
    const std::string who(who_);
    std::memset(out, 0, sizeof *out);
    kmdb_engine_view e;
    if (kmdb_engine_get(db, &e)) return 1;
    const uint64_t N = e.N;
    if (cell_lo > cell_hi) return kmdb_set_error(who + ": cell_lo > cell_hi");
    if (cell_hi > (uint64_t)nq * N) return kmdb_set_error(who + ": cell_hi beyond the nq x N cells of the batch");
    if (!cells_dev && cell_hi > cell_lo) return kmdb_set_error(who + ": null rows");
    if (n_filters && !query_kmers && nq) return kmdb_set_error(who + ": null argument");
    if (nq >= (1ull << 31)) return kmdb_set_error(who + ": too many queries in one batch");
    HIP_TRY(hipSetDevice(e.device));
    hipStream_t st = stream_of(e, opts);
    const uint32_t nseg = (uint32_t)std::max<uint64_t>(1, (N + N2S_SEG - 1) / N2S_SEG);
    const uint64_t n_segs = (uint64_t)nq * nseg;
    DevEvent c0, c1, c2, c3;
    if (c0.create()) return 1; if (c1.create()) return 1; if (c2.create()) return 1; if (c3.create()) return 1;
    DevBuf<void> d_cnt, d_scan, d_ptr, d_tmp, d_col, d_val, d_qk, d_sk;
    DevFilter df{};
    if (n_filters) {
        DEV_ALLOC_BYTES(d_qk, nq * 4); DEV_ALLOC_BYTES(d_sk, N * 4);
        if (nq) HIP_TRY(hipMemcpyAsync(d_qk.get(), query_kmers, nq * 4, hipMemcpyHostToDevice, st));
        if (N) HIP_TRY(hipMemcpyAsync(d_sk.get(), sample_kmers, N * 4, hipMemcpyHostToDevice, st));
        df.n = (int)n_filters; df.counts = static_cast<uint32_t*>(d_qk.get());
        kmdb_dev_bounds(filters, n_filters, (int)e.kmer_length, df.kind, df.lo, df.hi);
    }
    DEV_ALLOC_BYTES(d_cnt, (n_segs + 1) * 8); DEV_ALLOC_BYTES(d_scan, (n_segs + 1) * 8); DEV_ALLOC_BYTES(d_ptr, (nq + 1) * 8);
    size_t scan_bytes = 0;
    HIP_TRY(prim::exclusive_sum(nullptr, scan_bytes, static_cast<unsigned long long*>(d_cnt.get()), static_cast<unsigned long long*>(d_scan.get()), (size_t)(n_segs + 1), st));
    DEV_ALLOC_BYTES(d_tmp, scan_bytes);
    // the segments of the rows that meet the range (the others keep a count of zero)
    uint64_t seg_lo = 0, seg_hi = 0;
    if (cell_hi > cell_lo && N) { seg_lo = cell_lo / N * nseg; seg_hi = ((cell_hi - 1) / N + 1) * nseg; }
    HIP_TRY(hipEventRecord(c0, st));
    HIP_TRY(hipMemsetAsync(d_cnt.get(), 0, (n_segs + 1) * 8, st));
    for (uint64_t s0 = seg_lo; s0 < seg_hi; s0 += N2S_GRID_MAX) {
        hipLaunchKernelGGL((n2s_segments_kernel<false>), dim3((unsigned)std::min(N2S_GRID_MAX, seg_hi - s0)), dim3(64), 0, st, cells_dev, (uint32_t)N, nseg, s0, seg_hi,
                           cell_lo, cell_hi, static_cast<unsigned long long*>(d_cnt.get()), (const unsigned long long*)nullptr, (uint32_t*)nullptr, (uint32_t*)nullptr, df,
                           static_cast<uint32_t*>(d_sk.get()));
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipEventRecord(c1, st));
    HIP_TRY(prim::exclusive_sum(d_tmp.get(), scan_bytes, static_cast<unsigned long long*>(d_cnt.get()), static_cast<unsigned long long*>(d_scan.get()), (size_t)(n_segs + 1), st));
    hipLaunchKernelGGL(n2s_row_ptr_kernel, dim3((unsigned)((nq + 1 + 255) / 256)), dim3(256), 0, st, static_cast<unsigned long long*>(d_scan.get()), nseg, (uint64_t)nq,
                       static_cast<unsigned long long*>(d_ptr.get()));
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(c2, st));
    std::vector<unsigned long long> h_ptr(nq + 1, 0);
    HIP_TRY(hipMemcpyAsync(h_ptr.data(), d_ptr.get(), (nq + 1) * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    const uint64_t nnz_dev = h_ptr[nq];
    if (nnz_dev > cell_hi - cell_lo) return kmdb_set_error(who + ": internal error (more kept cells than cells)");
    DEV_ALLOC_BYTES(d_col, nnz_dev * 4); DEV_ALLOC_BYTES(d_val, nnz_dev * 4);
    if (nnz_dev)
        for (uint64_t s0 = seg_lo; s0 < seg_hi; s0 += N2S_GRID_MAX) {
            hipLaunchKernelGGL((n2s_segments_kernel<true>), dim3((unsigned)std::min(N2S_GRID_MAX, seg_hi - s0)), dim3(64), 0, st, cells_dev, (uint32_t)N, nseg, s0, seg_hi,
                               cell_lo, cell_hi, (unsigned long long*)nullptr, static_cast<unsigned long long*>(d_scan.get()), static_cast<uint32_t*>(d_col.get()), static_cast<uint32_t*>(d_val.get()), df,
                               static_cast<uint32_t*>(d_sk.get()));
            HIP_TRY(hipGetLastError());
        }
    HIP_TRY(hipEventRecord(c3, st));
    HIP_TRY(hipEventSynchronize(c3));
    float ms = 0;
    HIP_TRY(hipEventElapsedTime(&ms, c0, c3));
    out->n_rows = nq;
    out->nnz = nnz_dev;
    out->row_ptr = (uint64_t*)std::malloc((nq + 1) * 8);
    out->col = (uint32_t*)std::malloc(std::max<uint64_t>(nnz_dev, 1) * 4);
    out->val = (uint32_t*)std::malloc(std::max<uint64_t>(nnz_dev, 1) * 4);
    if (!out->row_ptr || !out->col || !out->val) { kmdb_sparse_free(out); return kmdb_set_error(who + ": out of host memory for the result"); }
    for (uint64_t i = 0; i <= nq; ++i) out->row_ptr[i] = h_ptr[i];
    if (nnz_dev) {
        hipError_t rc = hipMemcpyAsync(out->col, d_col.get(), nnz_dev * 4, hipMemcpyDeviceToHost, st);
        if (rc == hipSuccess) rc = hipMemcpyAsync(out->val, d_val.get(), nnz_dev * 4, hipMemcpyDeviceToHost, st);
        if (rc == hipSuccess) rc = hipStreamSynchronize(st);
        if (rc != hipSuccess) { kmdb_sparse_free(out); return kmdb_set_error(who + ": copy of the compacted rows: " + hipGetErrorString(rc)); }
    }
    if (stats) {
        stats->cells = cell_hi - cell_lo; stats->nnz_device = nnz_dev; stats->nnz = nnz_dev;
        stats->d2h_bytes = ((uint64_t)nq + 1) * 8 + nnz_dev * 8; stats->compact_ms = ms;
    }
    return 0;
}

// One batch on one handle: the rows into a zeroed nq x N buffer of the call's own (fill), compacted there, decided on the host.
// allow_query_shard: the plain entry (no bounds) also serves a query shard's partial rows, as it always did.
template <class Fill>
static int n2s_batch(const char* who_, kmdb_db* db, size_t nq, const kmdb_cell_filter* filters, size_t n_filters, const uint32_t* sample_kmers, int measure,
                     kmdb_sparse_rows* out, const kmdb_opts* opts, bool allow_query_shard, Fill&& fill) {
    const std::string who(who_);
    std::memset(out, 0, sizeof *out);
    kmdb_engine_view e;
    if (kmdb_engine_get(db, &e)) return 1;
    if ((!e.n_buckets && e.qs_count <= 1) || !e.slots) return kmdb_set_error(who + ": database was uploaded without hashtables");
    if (e.qs_count > 1 && !allow_query_shard)
        return kmdb_set_error(who + ": a query shard holds partial sums and partial k-mer counts (compact the summed rows with kmdb_new2all_rows_sparse_device, or use kmdb_node_new2all_batch_sparse_filtered)");
    if (nq >= (1ull << 31)) return kmdb_set_error(who + ": too many queries in one batch");
    HIP_TRY(hipSetDevice(e.device));
    hipStream_t st = stream_of(e, opts);
    const uint64_t cells = (uint64_t)nq * e.N;
    DevBuf<void> rows;
    DEV_ALLOC_BYTES(rows, cells * 4);
    if (cells) HIP_TRY(hipMemsetAsync(rows.get(), 0, cells * 4, st));
    kmdb_opts o{};
    if (opts) o = *opts; else { o.abi_version = KMDB_ABI_VERSION; o.device = e.device; o.shard_count = 1; }
    o.stream = st;
    std::vector<uint32_t> qk;
    try { qk.assign(std::max<size_t>(nq, 1), 0); } catch (const std::exception&) { return kmdb_set_error(who + ": out of host memory"); }
    if (fill(static_cast<uint32_t*>(rows.get()), &o, qk.data())) return 1;
    kmdb_stats before{};
    (void)kmdb_db_stats(db, &before);
    kmdb_new2all_sparse_stats ns{};
    if (kmdb_n2a_rows_compact(who_, db, static_cast<uint32_t*>(rows.get()), nq, 0, cells, qk.data(), filters, n_filters, sample_kmers, out, &o, &ns)) return 1;
    kmdb_engine_set_times(db, before.kernel_ms + ns.compact_ms, before.kernel_ms + ns.compact_ms);
    if ((n_filters || measure >= 0) && kmdb_sparse_decide(who_, out, filters, n_filters, qk.data(), sample_kmers, measure, (int)e.kmer_length)) return 1;
    ns.nnz = out->nnz;
    *e.n2s_stats = ns;
    return 0;
}

static int n2s_kmers(const char* who, kmdb_db* db, const uint64_t* const* kmers, const size_t* counts, size_t nq, const kmdb_cell_filter* filters, size_t n_filters,
                     const uint32_t* sample_kmers, int measure, kmdb_sparse_rows* out, const kmdb_opts* opts, bool allow_query_shard) {
    if (n2s_check_args(who, db, out, filters, n_filters, sample_kmers, measure)) return 1;
    if (nq && (!kmers || !counts)) return kmdb_set_error(std::string(who) + ": null argument");
    return n2s_batch(who, db, nq, filters, n_filters, sample_kmers, measure, out, opts, allow_query_shard, [&](uint32_t* rows, const kmdb_opts* o, uint32_t* qk) -> int {
        for (size_t q = 0; q < nq; ++q) qk[q] = (uint32_t)counts[q];
        return kmdb_new2all_batch_device(db, kmers, counts, nq, rows, o);
    });
}

extern "C" int kmdb_new2all_batch_sparse_filtered(kmdb_db* db, const uint64_t* const* kmers, const size_t* counts, size_t nq, const kmdb_cell_filter* filters,
                                                  size_t n_filters, const uint32_t* sample_kmers, int measure, kmdb_sparse_rows* out, const kmdb_opts* opts) {
    return n2s_kmers("kmdb_new2all_batch_sparse_filtered", db, kmers, counts, nq, filters, n_filters, sample_kmers, measure, out, opts, false);
}

// one2all_sp without bounds (console_new2all.cpp:78): the same path, every non-zero cell
extern "C" int kmdb_new2all_batch_sparse(kmdb_db* db, const uint64_t* const* kmers, const size_t* counts, size_t nq, kmdb_sparse_rows* out, const kmdb_opts* opts) {
    return n2s_kmers("kmdb_new2all_batch_sparse", db, kmers, counts, nq, nullptr, 0, nullptr, -1, out, opts, true);
}

extern "C" int kmdb_new2all_batch_seq_alphabet_sparse_filtered(kmdb_db* db, const char* const* seqs, const size_t* seq_lens, size_t nq, double fraction,
                                                               double start_fraction, int32_t alphabet, const kmdb_cell_filter* filters, size_t n_filters,
                                                               const uint32_t* sample_kmers, int measure, kmdb_sparse_rows* out, uint64_t* out_kmer_counts,
                                                               const kmdb_opts* opts) {
    const char* who = "kmdb_new2all_batch_seq_alphabet_sparse_filtered";
    if (n2s_check_args(who, db, out, filters, n_filters, sample_kmers, measure)) return 1;
    if (nq && (!seqs || !seq_lens || !out_kmer_counts)) return kmdb_set_error(std::string(who) + ": null argument");
    if (alphabet < 0 || alphabet >= KMDB_ALPHABET_COUNT) return kmdb_set_error(std::string(who) + ": unknown alphabet " + std::to_string(alphabet));
    return n2s_batch(who, db, nq, filters, n_filters, sample_kmers, measure, out, opts, false, [&](uint32_t* rows, const kmdb_opts* o, uint32_t* qk) -> int {
        // the query counts are the device extractor's unique counts
        if (kmdb_new2all_batch_seq_alphabet_device(db, seqs, seq_lens, nq, fraction, start_fraction, alphabet, rows, out_kmer_counts, o)) return 1;
        for (size_t q = 0; q < nq; ++q) qk[q] = (uint32_t)out_kmer_counts[q];
        return 0;
    });
}

// ------------------------------------------------------------------------------------------
// new2all -sample-rows <criterion>:<count>: every query keeps its `count` best database samples (the rule of Sampler, reference
// src/sampler.h:44-67, applied to the sparse row console_new2all.cpp:130-148 writes).  The rows of a batch are accumulated as above, the
// candidates selected where they are (kmdb_sample_query_rows: sample_rows.hip, the completeness rule and the re-fetch of engine.hip), the
// decision is the host's (kmdbh_query_rows_select).  Only the candidates leave HBM.
// ------------------------------------------------------------------------------------------
template <class Fill>
static int n2s_batch_sampled(const char* who_, kmdb_db* db, size_t nq, const kmdb_cell_filter* filters, size_t n_filters, const uint32_t* sample_kmers, int criterion,
                             uint32_t count, kmdb_sparse_rows* out, const kmdb_opts* opts, Fill&& fill) {
    const std::string who(who_);
    std::memset(out, 0, sizeof *out);
    kmdb_engine_view e;
    if (kmdb_engine_get(db, &e)) return 1;
    if ((!e.n_buckets && e.qs_count <= 1) || !e.slots) return kmdb_set_error(who + ": database was uploaded without hashtables");
    if (e.qs_count > 1)
        return kmdb_set_error(who + ": a query shard holds partial sums and partial k-mer counts (select on the summed rows with kmdb_sampled_from_rows_device)");
    if (e.N == 0) return kmdb_set_error(who + ": the database holds no samples");
    if (kmdb_sample_query_rows_check(who_, nq, e.N, 0, (uint64_t)nq * e.N)) return 1;
    HIP_TRY(hipSetDevice(e.device));
    hipStream_t st = stream_of(e, opts);
    const uint64_t cells = (uint64_t)nq * e.N;
    DevBuf<void> rows;
    DEV_ALLOC_BYTES(rows, cells * 4);
    if (cells) HIP_TRY(hipMemsetAsync(rows.get(), 0, cells * 4, st));
    kmdb_opts o{};
    if (opts) o = *opts; else { o.abi_version = KMDB_ABI_VERSION; o.device = e.device; o.shard_count = 1; }
    o.stream = st;
    std::vector<uint32_t> qk;
    try { qk.assign(std::max<size_t>(nq, 1), 0); } catch (const std::exception&) { return kmdb_set_error(who + ": out of host memory"); }
    if (fill(static_cast<uint32_t*>(rows.get()), &o, qk.data())) return 1;
    kmdb_stats before{};
    if (kmdb_db_stats(db, &before)) return 1;                    // (kernel_ms of the accumulation that has just ended)
    kmdb_sample_stats ss{};
    kmdb_sparse_rows cand;
    if (kmdb_sample_query_rows(who_, st, (int)e.kmer_length, static_cast<uint32_t*>(rows.get()), nq, e.N, 0, cells, qk.data(), filters, n_filters, sample_kmers, criterion,
                               count, &cand, &ss)) return 1;
    // kernel_ms of the call = accumulation + selection.  (kmdb_engine_set_times keeps no second figure any more: its dominant_ms argument is
    // not read, and every caller passes the call's total for it, as n2s_batch does.)
    const double call_ms = before.kernel_ms + ss.select_ms;
    kmdb_engine_set_times(db, call_ms, call_ms);
    *e.n2a_sample_stats = ss;
    const kmdb_sparse_rows* parts[1] = {&cand};
    const int rc = kmdbh_query_rows_select(criterion, count, (int)e.kmer_length, qk.data(), nq, sample_kmers, filters, n_filters, parts, 1, out);
    kmdb_sparse_free(&cand);
    return rc;
}

extern "C" int kmdb_new2all_batch_sampled(kmdb_db* db, const uint64_t* const* kmers, const size_t* counts, size_t nq, const kmdb_cell_filter* filters,
                                          size_t n_filters, const uint32_t* sample_kmers, int criterion, uint32_t count, kmdb_sparse_rows* out,
                                          const kmdb_opts* opts) {
    const char* who = "kmdb_new2all_batch_sampled";
    if (!db || !out) return kmdb_set_error(std::string(who) + ": null argument");
    if (kmdb_check_sample_args(who, filters, n_filters, sample_kmers, criterion, count)) return 1;
    if (nq && (!kmers || !counts)) return kmdb_set_error(std::string(who) + ": null argument");
    return n2s_batch_sampled(who, db, nq, filters, n_filters, sample_kmers, criterion, count, out, opts, [&](uint32_t* rows, const kmdb_opts* o, uint32_t* qk) -> int {
        for (size_t q = 0; q < nq; ++q) qk[q] = (uint32_t)counts[q];
        return kmdb_new2all_batch_device(db, kmers, counts, nq, rows, o);
    });
}

extern "C" int kmdb_new2all_batch_seq_alphabet_sampled(kmdb_db* db, const char* const* seqs, const size_t* seq_lens, size_t nq, double fraction,
                                                       double start_fraction, int32_t alphabet, const kmdb_cell_filter* filters, size_t n_filters,
                                                       const uint32_t* sample_kmers, int criterion, uint32_t count, kmdb_sparse_rows* out,
                                                       uint64_t* out_kmer_counts, const kmdb_opts* opts) {
    const char* who = "kmdb_new2all_batch_seq_alphabet_sampled";
    if (!db || !out) return kmdb_set_error(std::string(who) + ": null argument");
    if (kmdb_check_sample_args(who, filters, n_filters, sample_kmers, criterion, count)) return 1;
    if (nq && (!seqs || !seq_lens || !out_kmer_counts)) return kmdb_set_error(std::string(who) + ": null argument");
    if (alphabet < 0 || alphabet >= KMDB_ALPHABET_COUNT) return kmdb_set_error(std::string(who) + ": unknown alphabet " + std::to_string(alphabet));
    return n2s_batch_sampled(who, db, nq, filters, n_filters, sample_kmers, criterion, count, out, opts, [&](uint32_t* rows, const kmdb_opts* o, uint32_t* qk) -> int {
        // the query counts are the device extractor's unique counts
        if (kmdb_new2all_batch_seq_alphabet_device(db, seqs, seq_lens, nq, fraction, start_fraction, alphabet, rows, out_kmer_counts, o)) return 1;
        for (size_t q = 0; q < nq; ++q) qk[q] = (uint32_t)out_kmer_counts[q];
        return 0;
    });
}

extern "C" int kmdb_new2all_rows_sparse_device(kmdb_db* db, const void* rows_dev, size_t nq, uint64_t cell_lo, uint64_t cell_hi, const uint32_t* query_kmers,
                                               const kmdb_cell_filter* filters, size_t n_filters, const uint32_t* sample_kmers, int measure,
                                               kmdb_sparse_rows* out, const kmdb_opts* opts) {
    const char* who = "kmdb_new2all_rows_sparse_device";
    if (n2s_check_args(who, db, out, filters, n_filters, sample_kmers, measure)) return 1;
    if ((n_filters || measure >= 0) && nq && !query_kmers) return kmdb_set_error(std::string(who) + ": null argument");
    if (cell_lo > cell_hi) return kmdb_set_error(std::string(who) + ": cell_lo > cell_hi");
    kmdb_engine_view e;
    if (kmdb_engine_get(db, &e)) return 1;
    kmdb_new2all_sparse_stats ns{};
    if (kmdb_n2a_rows_compact(who, db, (const uint32_t*)rows_dev, nq, cell_lo, cell_hi, query_kmers, filters, n_filters, sample_kmers, out, opts, &ns)) return 1;
    // (a call of its own: the device pipeline of the call is the compaction)
    kmdb_engine_set_times(db, ns.compact_ms, ns.compact_ms);
    if ((n_filters || measure >= 0) && kmdb_sparse_decide(who, out, filters, n_filters, query_kmers, sample_kmers, measure, (int)e.kmer_length)) return 1;
    ns.nnz = out->nnz;
    *e.n2s_stats = ns;
    return 0;
}
