// host_sampler.cpp — the exact decision of `-sample-rows <criterion>:<count>` (reference src/sampler.h: Sampler with strategy `best`, filled by
// SparseMatrix::add_to_sampler, src/array.h:450-540; call site console_all2all_sparse.cpp:70-89).  Host code: the score of a pair is
// kmdbh_metric — the reference's double arithmetic — and the order is the sampler's own total order (sampler.h:45-50: score descending, then
// sample id ascending), so what is kept does not depend on the order in which the candidates arrive.  The device only proposes candidates
// (sample_rows.hip); any superset of a row's true best `count` gives the same rows here.
#include "kmdb_amd.h"
#include "kmdb_internal.h"

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <exception>
#include <string>
#include <vector>

namespace {
struct Item { uint32_t id, val; double score; };
// sampler.h:45-50; a NaN score (the reference's comparison is no order there) ranks below every number, so that this stays a strict weak order
inline bool better(const Item& x, const Item& y) {
    const bool nx = x.score != x.score, ny = y.score != y.score;
    if (nx || ny) return nx != ny ? ny : x.id < y.id;
    return x.score != y.score ? x.score > y.score : x.id < y.id;
}
// a non-zero cell against every bound (the CombinedFilter of the sparse calls: closed bounds, a NaN measure fails)
inline bool passes(const kmdb_cell_filter* filters, size_t n_filters, uint32_t c, uint32_t a, uint32_t b, int kmer_length) {
    bool ok = c != 0;
    for (size_t q = 0; q < n_filters && ok; ++q) {
        const double x = kmdbh_metric(filters[q].metric, c, a, b, kmer_length);
        ok = x >= filters[q].lo && x <= filters[q].hi;
    }
    return ok;
}
// a row's candidates -> what the sampler keeps of them, in ascending id (a pair listed twice counts once)
inline void keep_best(std::vector<Item>& row, uint32_t count) {
    std::sort(row.begin(), row.end(), [](const Item& x, const Item& y) { return x.id < y.id; });
    row.erase(std::unique(row.begin(), row.end(), [](const Item& x, const Item& y) { return x.id == y.id; }), row.end());
    if (row.size() > count) {
        std::nth_element(row.begin(), row.begin() + (std::ptrdiff_t)count, row.end(), better);
        row.resize(count);
        std::sort(row.begin(), row.end(), [](const Item& x, const Item& y) { return x.id < y.id; });
    }
}
// the kept items of all rows as a kmdb_sparse_rows with measures
int give(const char* who, uint64_t N, const std::vector<uint64_t>& ptr, const std::vector<Item>& kept, kmdb_sparse_rows* out) {
    const uint64_t nnz = kept.size();
    out->n_rows = N; out->nnz = nnz;
    out->row_ptr = (uint64_t*)std::malloc((N + 1) * 8);
    out->col = (uint32_t*)std::malloc(std::max<uint64_t>(nnz, 1) * 4);
    out->val = (uint32_t*)std::malloc(std::max<uint64_t>(nnz, 1) * 4);
    out->measure = (double*)std::malloc(std::max<uint64_t>(nnz, 1) * 8);
    if (!out->row_ptr || !out->col || !out->val || !out->measure) {
        std::free(out->row_ptr); std::free(out->col); std::free(out->val); std::free(out->measure);
        std::memset(out, 0, sizeof *out);
        return kmdb_set_error(std::string(who) + ": out of host memory for the result");
    }
    std::memcpy(out->row_ptr, ptr.data(), (N + 1) * 8);
    for (uint64_t e = 0; e < nnz; ++e) { out->col[e] = kept[e].id; out->val[e] = kept[e].val; out->measure[e] = kept[e].score; }
    return 0;
}
}  // namespace

extern "C" int kmdbh_sample_rows_select(int criterion, uint32_t count, int kmer_length, const uint32_t* sample_kmers, const kmdb_cell_filter* filters,
                                        size_t n_filters, const kmdb_sparse_rows* const* parts, size_t n_parts, kmdb_sparse_rows* out) {
    if (!out) return kmdb_set_error("kmdbh_sample_rows_select: null argument");
    std::memset(out, 0, sizeof *out);
    if (count == 0) return kmdb_set_error("kmdbh_sample_rows_select: count must be at least 1");
    if (criterion < 0 || criterion >= KMDB_METRIC_COUNT) return kmdb_set_error("kmdbh_sample_rows_select: unknown criterion");
    if (!sample_kmers) return kmdb_set_error("kmdbh_sample_rows_select: sample_kmers is NULL");
    if ((n_filters && !filters) || (n_parts && !parts)) return kmdb_set_error("kmdbh_sample_rows_select: null argument");
    for (size_t q = 0; q < n_filters; ++q)
        if (filters[q].metric < 0 || filters[q].metric >= KMDB_METRIC_COUNT) return kmdb_set_error("kmdbh_sample_rows_select: unknown metric in a filter");
    uint64_t N = 0;
    for (size_t p = 0; p < n_parts; ++p) {
        if (!parts[p] || (parts[p]->n_rows && !parts[p]->row_ptr)) return kmdb_set_error("kmdbh_sample_rows_select: null part");
        if (parts[p]->n_rows) {
            if (N && parts[p]->n_rows != N) return kmdb_set_error("kmdbh_sample_rows_select: the parts have different numbers of rows");
            N = parts[p]->n_rows;
        }
    }
    try {
        std::vector<uint64_t> ptr(N + 1, 0);
        std::vector<Item> kept, row;
        for (uint64_t s = 0; s < N; ++s) {
            row.clear();
            for (size_t p = 0; p < n_parts; ++p) {
                const kmdb_sparse_rows& r = *parts[p];
                if (!r.n_rows) continue;
                for (uint64_t e = r.row_ptr[s]; e < r.row_ptr[s + 1]; ++e) {
                    const uint32_t o = r.col[e], c = r.val[e];
                    if (o >= N || o == s) return kmdb_set_error("kmdbh_sample_rows_select: a candidate's column is no other sample of the collection");
                    // the pair's cell lives in the triangle's row max(s, o): that sample is the measure's row sample (array.h:450-540)
                    const uint32_t a = sample_kmers[s > o ? s : o], b = sample_kmers[s > o ? o : s];
                    if (passes(filters, n_filters, c, a, b, kmer_length)) row.push_back(Item{o, c, kmdbh_metric(criterion, c, a, b, kmer_length)});
                }
            }
            keep_best(row, count);
            kept.insert(kept.end(), row.begin(), row.end());
            ptr[s + 1] = kept.size();
        }
        return give("kmdbh_sample_rows_select", N, ptr, kept, out);
    } catch (const std::exception& e) {
        return kmdb_set_error(std::string("kmdbh_sample_rows_select: ") + e.what());
    }
}

// The one-sided form for the query rows of new2all (the same Sampler, sampler.h:44-67, over the sparse row of console_new2all.cpp:130-148): row q
// keeps the `count` best database samples of query q; a = the query's k-mer count, b = the sample's; the samples collect nothing.
extern "C" int kmdbh_query_rows_select(int criterion, uint32_t count, int kmer_length, const uint32_t* query_kmers, size_t nq, const uint32_t* sample_kmers,
                                       const kmdb_cell_filter* filters, size_t n_filters, const kmdb_sparse_rows* const* parts, size_t n_parts,
                                       kmdb_sparse_rows* out) {
    const char* who = "kmdbh_query_rows_select";
    if (!out) return kmdb_set_error(std::string(who) + ": null argument");
    std::memset(out, 0, sizeof *out);
    if (count == 0) return kmdb_set_error(std::string(who) + ": count must be at least 1");
    if (criterion < 0 || criterion >= KMDB_METRIC_COUNT) return kmdb_set_error(std::string(who) + ": unknown criterion");
    if (!sample_kmers) return kmdb_set_error(std::string(who) + ": sample_kmers is NULL");
    if (nq && !query_kmers) return kmdb_set_error(std::string(who) + ": query_kmers is NULL");
    if ((n_filters && !filters) || (n_parts && !parts)) return kmdb_set_error(std::string(who) + ": null argument");
    for (size_t q = 0; q < n_filters; ++q)
        if (filters[q].metric < 0 || filters[q].metric >= KMDB_METRIC_COUNT) return kmdb_set_error(std::string(who) + ": unknown metric in a filter");
    for (size_t p = 0; p < n_parts; ++p) {
        if (!parts[p] || (parts[p]->n_rows && !parts[p]->row_ptr)) return kmdb_set_error(std::string(who) + ": null part");
        if (parts[p]->n_rows && parts[p]->n_rows != nq) return kmdb_set_error(std::string(who) + ": a part does not have nq rows");
    }
    try {
        std::vector<uint64_t> ptr(nq + 1, 0);
        std::vector<Item> kept, row;
        for (uint64_t s = 0; s < nq; ++s) {
            row.clear();
            const uint32_t a = query_kmers[s];
            for (size_t p = 0; p < n_parts; ++p) {
                const kmdb_sparse_rows& r = *parts[p];
                if (!r.n_rows) continue;
                for (uint64_t e = r.row_ptr[s]; e < r.row_ptr[s + 1]; ++e) {
                    const uint32_t o = r.col[e], c = r.val[e], b = sample_kmers[o];
                    if (passes(filters, n_filters, c, a, b, kmer_length)) row.push_back(Item{o, c, kmdbh_metric(criterion, c, a, b, kmer_length)});
                }
            }
            keep_best(row, count);
            kept.insert(kept.end(), row.begin(), row.end());
            ptr[s + 1] = kept.size();
        }
        return give(who, nq, ptr, kept, out);
    } catch (const std::exception& e) {
        return kmdb_set_error(std::string(who) + ": " + e.what());
    }
}
