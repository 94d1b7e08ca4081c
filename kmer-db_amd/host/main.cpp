// kmer-db-amd — command line front-end for the MI355X engine.
//
// Drop-in for the three kmer-db modes on the hot path:
//     kmer-db-amd all2all    [-sparse [-min [m:]v] [-max [m:]v]] <db> <out.csv>
//     kmer-db-amd all2all-sp [-min [m:]v] [-max [m:]v]           <db> <out.csv>
//     kmer-db-amd all2all | all2all-sp [-sparse] [-phylip-out] [-min ...] [-max ...] -distance <measure> <db> <out>
//     kmer-db-amd all2all | all2all-sp -rows <lo>:<hi> | new [the forms above] <db> <out>
//     kmer-db-amd all2all | all2all-sp -band-rows <R> [the forms above] <db> <out>
//     kmer-db-amd all2all | all2all-sp -rows ... | -band-rows <R> -band-path <tree|tiled|records> [the forms above] <db> <out>
//     kmer-db-amd new2all    [-multisample-fasta] [-sparse ...]  <db> <sample-list> <out.csv>
//     kmer-db-amd new2all    [-multisample-fasta] [-sparse] [-phylip-out] [-min ...] [-max ...] -distance <measure> <db> <sample-list> <out>
//     kmer-db-amd one2all    <db> <sample> <out.csv>
//     kmer-db-amd all2all-parts [-min ...] [-max ...] <db-list> <out.csv>
//     kmer-db-amd all2all-parts [-min ...] [-max ...] [-gpus W] -distance <measure> <db-list> <out>
//     kmer-db-amd minhash    [-f <fraction>] [-k <kmer-length>] [-alphabet <name>] <samples>
//     kmer-db-amd build      [-k <kmer-length>] [-f <fraction>] [-alphabet <name>] [-multisample-fasta | -from-minhash] <samples> <db>
//     kmer-db-amd build      -extend-from <old.db> [-multisample-fasta | -from-minhash] <samples> <db>
// mirroring the reference consoles (reference src/console_all2all.cpp, console_all2all_sparse.cpp,
// console_new2all.cpp) around the calls that the C ABI replaces.  Options that only tune the
// reference's CPU engine (-t, -rt, -buffer, -bubble-size) are accepted; -t also sizes the
// query-parsing thread pool.  Output files are byte-identical to the reference's.
// Everything below the three kmdb_* compute calls runs on the GPU; there is no CPU engine here.
#include "kmdb_amd.h"

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <functional>
#include <iostream>
#include <exception>
#include <map>
#include <mutex>
#include <random>
#include <sstream>
#include <stdexcept>
#include <string>
#include <memory>
#include <ctime>
#include <unistd.h>
#include <thread>
#include <vector>

#include <zlib.h>

namespace {

using clk = std::chrono::high_resolution_clock;
double since(clk::time_point t0) { return std::chrono::duration<double>(clk::now() - t0).count(); }

struct usage_error : std::runtime_error { using std::runtime_error::runtime_error; };

// ---- option helpers (same removal semantics as Params::findSwitch/findOption, params.h) -------
bool take_switch(std::vector<std::string>& a, const std::string& name) {
    for (size_t i = 0; i < a.size(); ++i)
        if (a[i] == name) { a.erase(a.begin() + i); return true; }
    return false;
}
bool take_option(std::vector<std::string>& a, const std::string& name, std::string& value) {
    for (size_t i = 0; i + 1 < a.size(); ++i)
        if (a[i] == name) { value = a[i + 1]; a.erase(a.begin() + i, a.begin() + i + 2); return true; }
    return false;
}

// ---- -min / -max filters (params.cpp:14-42, 418-455; sparse_filters.h) ---------------------------
using metric_fn = std::function<double(uint32_t, uint32_t, uint32_t, int)>;

// the nine measures by name: ONE implementation, the library's kmdbh_metric (csrc/host_metrics.cpp: the reference's arithmetic,
// params.cpp:14-42) — the front-end's filters and its `distance` mode must agree with it bit for bit
std::map<std::string, metric_fn> metrics() {
    std::map<std::string, metric_fn> m;
    for (const char* name : {"jaccard", "min", "max", "cosine", "mash", "ani", "ani-shorter", "mash-query", "num-kmers"}) {
        const int id = kmdbh_metric_id(name);
        if (id < 0) throw std::runtime_error(std::string("internal: the library does not know the measure ") + name);
        m[name] = [id](uint32_t c, uint32_t a, uint32_t b, int k) { return kmdbh_metric(id, c, a, b, k); };
    }
    return m;
}

struct Filters {
    struct Bound { metric_fn fn; double lo = std::numeric_limits<double>::lowest(), hi = std::numeric_limits<double>::max(); };
    std::map<std::string, Bound> metric;
    uint32_t kmer_lo = 0, kmer_hi = std::numeric_limits<uint32_t>::max();
    size_t given = 0;                        // -min / -max options read: never fewer than the bounds they fold into (one lo / hi pair per measure)

    void parse(std::vector<std::string>& args) {
        auto avail = metrics();
        const char* names[2] = {"-min", "-max"};
        for (int which = 0; which < 2; ++which) {
            std::string v;
            while (take_option(args, names[which], v)) {
                std::string metric_name = "num-kmers", num = v;
                auto sep = v.rfind(':');
                if (sep != std::string::npos) { metric_name = v.substr(0, sep); num = v.substr(sep + 1); }
                std::istringstream iss(num);
                double value;
                if (!(iss >> value)) throw std::runtime_error("Filtering error - unable to parse numerical value: " + v);
                ++given;
                if (metric_name == "num-kmers") {
                    (which == 0 ? kmer_lo : kmer_hi) = (uint32_t)std::lrint(value);
                } else if (avail.count(metric_name)) {
                    auto& b = metric[metric_name];
                    b.fn = avail[metric_name];
                    (which == 0 ? b.lo : b.hi) = value;
                } else {
                    throw std::runtime_error("Filtering error - unknown metric: " + metric_name);
                }
            }
        }
    }
    bool pass(uint32_t common, uint32_t row_cnt, uint32_t col_cnt, int k) const {
        for (auto& kv : metric) {
            double x = kv.second.fn(common, row_cnt, col_cnt, k);
            if (!(x >= kv.second.lo && x <= kv.second.hi)) return false;
        }
        return common >= kmer_lo && common <= kmer_hi;
    }
};
// the -min / -max bounds as a call takes them (the library applies at most 8: every site decides what it passes beyond that)
std::vector<kmdb_cell_filter> cell_filters(const Filters& f) {
    std::vector<kmdb_cell_filter> fl;
    for (auto& kv : f.metric) fl.push_back(kmdb_cell_filter{kmdbh_metric_id(kv.first.c_str()), 0, kv.second.lo, kv.second.hi});
    if (f.kmer_lo != 0 || f.kmer_hi != std::numeric_limits<uint32_t>::max())
        fl.push_back(kmdb_cell_filter{KMDB_METRIC_NUM_KMERS, 0, (double)f.kmer_lo, (double)f.kmer_hi});
    return fl;
}

// -sample-rows [<criterion>:]<count> (all2all-sp, all2all-parts; reference src/sampler.h, src/params.cpp:533-557, src/array.h:450-540): every
// sample keeps at most `count` of its neighbours — every pair (i, j) that passes the filters is offered to row i AND to row j, so the sampled
// rows are symmetric rows, not rows of the triangle.  With a criterion: the `count` best by score, ties towards the smaller sample id — what
// the reference's heap (sampler.h:44-67: score descending, item ascending) leaves whatever the order of its insertions, so the output is
// byte-identical.  Without one the reference keeps a RANDOM subset (sampler.h:69-79: mt19937_64 with the default seed per sample, drawn in the
// order in which its hash tables happen to list a row): here the same draws, over the pairs in ascending order of the other sample — the same
// kind of subset, not the same bytes.
// all2all-sp with a criterion never fills this sampler: the candidates are selected on the device and decided by the library
// (kmdb_all2all_sampled / kmdb_node_all2all_sampled).  all2all-parts does, from several workers at once.  With a criterion it is given the
// CANDIDATES of every cell only — per sample a superset of its `count` best of that cell, selected on the device (kmdb_db2db_sampled; the diagonal
// cells by kmdb_all2all_sampled), each side of a pair where it was selected — and finish_row, exact on any superset, decides.  Every kept pair of
// every cell goes through it only on the host path: the random strategy, KMDB_PARTS_DENSE_CELLS=1, KMDB_PARTS_HOST_SAMPLER=1 or more than 12
// bounds.  add() takes the lock of the sample's stripe, and with a criterion a row is pruned to its `cap` best whenever it reaches
// 2 * cap items (the order is total, so what is left at the end is the same: never more than 2 * cap items per sample, as the reference's heap
// never holds more than cap + 1).
struct RowSampler {
    struct Item { uint32_t item, value; double score; };
    size_t cap = 0;
    bool best = false;
    int criterion_id = -1;
    metric_fn criterion = nullptr;
    static constexpr size_t STRIPES = 1024;
    std::unique_ptr<std::mutex[]> stripes{new std::mutex[STRIPES]};
    std::vector<std::vector<Item>> rows;
    std::vector<size_t> seen;
    std::vector<std::mt19937_64> rng;
    bool on() const { return cap != 0; }
    void parse(std::vector<std::string>& args) {
        std::string v;
        if (!take_option(args, "-sample-rows", v)) return;
        std::string num = v;
        auto sep = v.rfind(':');
        if (sep != std::string::npos) {
            const std::string name = v.substr(0, sep);
            auto avail = metrics();
            if (!avail.count(name)) throw std::runtime_error("Sampling parameters error - unknown measure: " + name);
            criterion = avail[name]; best = true; criterion_id = kmdbh_metric_id(name.c_str());
            num = v.substr(sep + 1);
        }
        std::istringstream iss(num);
        if (!(iss >> cap)) throw std::runtime_error("Sampling parameters error - unable to parse numerical value: " + v);
    }
    void init(size_t n) { rows.assign(n, {}); if (!best) { seen.assign(n, 0); rng.assign(n, std::mt19937_64()); } }
    static bool better(const Item& x, const Item& y) { return x.score != y.score ? x.score > y.score : x.item < y.item; }
    void add(size_t sample, uint32_t item, uint32_t value, double score) {
        std::lock_guard<std::mutex> g(stripes[sample % STRIPES]);
        auto& r = rows[sample];
        r.push_back(Item{item, value, score});
        if (best) {
            if (r.size() >= 2 * cap) { std::nth_element(r.begin(), r.begin() + (std::ptrdiff_t)cap, r.end(), better); r.resize(cap); }
            return;
        }
        ++seen[sample];
        if (r.size() <= cap) return;
        if (rng[sample]() % seen[sample] != 0) { const size_t id = rng[sample]() % cap; r[id] = r.back(); }      // sampler.h:69-79
        r.pop_back();
    }
    // the row as the reference writes it: ascending sample ids (sampler.h:123-139)
    void finish_row(size_t sample, std::vector<uint32_t>& cols, std::vector<uint32_t>& vals) {
        auto& r = rows[sample];
        if (best && r.size() > cap) { std::partial_sort(r.begin(), r.begin() + (std::ptrdiff_t)cap, r.end(), better); r.resize(cap); }
        std::sort(r.begin(), r.end(), [](const Item& x, const Item& y) { return x.item < y.item; });
        cols.clear(); vals.clear();
        for (auto& x : r) { cols.push_back(x.item); vals.push_back(x.value); }
        std::vector<Item>().swap(r);
    }
    double score(uint32_t common, uint32_t row_cnt, uint32_t col_cnt, int k) const { return criterion ? criterion(common, row_cnt, col_cnt, k) : 1.0; }
};

void check(int rc) {
    if (rc) throw std::runtime_error(kmdb_last_error());
}

struct Db {
    kmdbh_db* h = nullptr;
    kmdb_db* d = nullptr;
    kmdb_node* node = nullptr;               // -gpus N: the database sharded over the devices of the node (prefix buckets or tree ranges)
    std::thread dropper;                     // gives the host image's pages back while the run goes on (uploaded())
    // the database is on the device: from here on only names and k-mer counts are read from the host image
    void uploaded() { if (h && !dropper.joinable()) dropper = std::thread([hh = h]() { kmdbh_db_release_patterns(hh); }); }
    ~Db() { if (dropper.joinable()) dropper.join(); if (node) kmdb_node_free(node); if (d) kmdb_db_free(d); if (h) kmdbh_db_free(h); }
};

// -rows <lo>:<hi> | new (all2all, all2all-sp): only the lines of samples lo .. hi - 1 of the table, from a band of the matrix computed alone
// (kmdb_all2all_rows_device; reference similarity_calculator.cpp:213-233 adds a row only from the patterns that hold its sample as a local id).
// 0-based sample indices, either side may be empty; `new` (with -from-samples -extend-from <old.db>): from the sample count of <old.db> to N.
struct RowBand {
    bool on = false, is_new = false, lo_open = false, hi_open = false;
    uint64_t lo = 0, hi = 0;
    void parse(const std::string& v) {
        on = true;
        if (v == "new") { is_new = true; return; }
        const std::string what = "-rows expects <lo>:<hi> (0-based sample indices, either side may be empty) or new: " + v;
        const size_t sep = v.find(':');
        if (sep == std::string::npos || v.find(':', sep + 1) != std::string::npos) throw std::runtime_error(what);
        auto side = [&](const std::string& t, bool& open, uint64_t& x) {
            open = t.empty();
            if (t.size() > 18 || t.find_first_not_of("0123456789") != std::string::npos) throw std::runtime_error(what);
            if (!open) x = std::strtoull(t.c_str(), nullptr, 10);
        };
        side(v.substr(0, sep), lo_open, lo);
        side(v.substr(sep + 1), hi_open, hi);
        if (!lo_open && !hi_open && lo > hi) throw std::runtime_error("-rows " + v + ": lo > hi");
    }
    // the band of a collection of n samples (seed_samples: those of -extend-from's database); refused: hi > n
    void resolve(uint64_t n, uint64_t seed_samples, uint64_t& r_lo, uint64_t& r_hi) const {
        r_lo = is_new ? seed_samples : lo_open ? 0 : lo;
        r_hi = is_new || hi_open ? n : hi;
        if (r_hi > n) throw std::runtime_error("-rows: " + std::to_string(r_hi) + " is beyond the " + std::to_string(n) + " samples of the database");
        if (r_lo > r_hi) throw std::runtime_error("-rows: lo > hi (" + std::to_string(r_lo) + " > " + std::to_string(r_hi) + ") with the " + std::to_string(n) + " samples of the database");
    }
};
uint64_t tri(uint64_t i) { return i ? i * (i - 1) / 2 : 0; }
// the band in device memory, for the calls that read it there
struct DeviceBand {
    int device = 0;
    void* p = nullptr;
    DeviceBand(int dev, uint64_t cells) : device(dev) { if (kmdb_device_buffer_alloc(dev, std::max<uint64_t>(cells, 1) * 4, &p)) throw std::runtime_error(kmdb_last_error()); }
    ~DeviceBand() { if (p) kmdb_device_buffer_free(device, p); }
    DeviceBand(const DeviceBand&) = delete;
    DeviceBand& operator=(const DeviceBand&) = delete;
};
// KMDB_VERBOSE: what the last band call on the handle did
void report_rows_stats(const kmdb_db* d, uint64_t, uint64_t) {
    kmdb_all2all_rows_stats rs{};
    if (!std::getenv("KMDB_VERBOSE") || kmdb_all2all_rows_stats_get(d, &rs)) return;
    std::cerr << "[kmdb] all2all rows: " << rs.band_cells << " cells, nodes selected / applied / updates " << rs.nodes_selected << " / " << rs.nodes_applied << " / "
              << rs.updates << ", select " << rs.select_ms << " ms, apply " << rs.apply_ms << " ms, " << rs.scratch_bytes << " bytes of scratch" << std::endl;
}

// the same for the tiled band call
void report_rows_tiled_stats(const kmdb_db* d, uint64_t lo, uint64_t hi) {
    kmdb_all2all_rows_tiled_stats bs{};
    if (!std::getenv("KMDB_VERBOSE") || kmdb_all2all_rows_tiled_stats_get(d, &bs)) return;
    std::cerr << "[kmdb] all2all rows tiled: rows " << lo << " to " << hi << ", " << bs.band_cells << " cells, nodes selected / applied " << bs.nodes_selected << " / "
              << bs.nodes_applied << ", hits / jobs / runs / updates " << bs.hits << " / " << bs.jobs << " / " << bs.runs << " / " << bs.updates << ", tiles of "
              << bs.tile_cols << " columns, select " << bs.select_ms << " ms, hits " << bs.hits_ms << " ms, apply " << bs.apply_ms << " ms, " << bs.scratch_bytes
              << " bytes of scratch" << std::endl;
}
// the same for the band call through the block-record pipeline (-band-path records)
void report_rows_records_stats(const kmdb_db* d, uint64_t lo, uint64_t hi) {
    kmdb_all2all_rows_records_stats rs{};
    if (!std::getenv("KMDB_VERBOSE") || kmdb_all2all_rows_records_stats_get(d, &rs)) return;
    std::cerr << "[kmdb] all2all rows records: rows " << lo << " to " << hi << ", " << rs.band_cells << " cells, "
              << (rs.path == KMDB_ROWS_RECORDS_PATH_RECORDS ? "block records" : rs.path == KMDB_ROWS_RECORDS_PATH_TREE ? "tree fallback" : "nothing to do")
              << ", block rows " << rs.x_lo << " to " << rs.x_hi << " of width " << rs.width << ", " << rs.records << " records, apply units run / total " << rs.units_run
              << " / " << rs.units_total << ", " << rs.slices << " slices, sized call " << rs.sized_call << ", decode " << rs.k0_ms << " ms, narrow " << rs.k1n_ms
              << " ms, wide " << rs.k1g_ms << " ms, apply " << rs.k2_ms << " ms, call " << rs.kernel_ms << " ms, peak " << rs.peak_device_bytes << " bytes";
    // the form the call took (KMDB_BAND_EMIT; beyond 2^22 block pairs band emit by itself), the band's streams and the band-emit state
    kmdb_all2all_rows_band_emit_stats be{};
    if (!kmdb_all2all_rows_band_emit_stats_get(d, &be))
        std::cerr << ", form " << (be.form == KMDB_BAND_EMIT_FORM_BAND ? "band emit" : be.form == KMDB_BAND_EMIT_FORM_WHOLE ? "whole emit" : "none") << ", " << be.n_streams
                  << " streams from " << be.stream_base << " in " << be.key_bits << " key bits, " << be.attempts << " attempts, band state " << be.state_bytes
                  << " bytes, whole state " << be.whole_state_bytes << " bytes";
    std::cerr << std::endl;
}
// -band-path <tree|tiled|records>: the band call of -rows / -band-rows
enum class BandPath { unset, tree, tiled, records };
BandPath parse_band_path(const std::string& v) {
    if (v == "tree") return BandPath::tree;
    if (v == "tiled") return BandPath::tiled;
    if (v == "records") return BandPath::records;
    throw std::runtime_error("-band-path expects tree, tiled or records: " + v);
}
// -band-rows <R>: a number of rows, 1 or more
uint64_t parse_band_rows(const std::string& v) {
    if (v.empty() || v.size() > 18 || v.find_first_not_of("0123456789") != std::string::npos || std::strtoull(v.c_str(), nullptr, 10) == 0)
        throw std::runtime_error("-band-rows expects <R>, a number of rows of 1 or more: " + v);
    return std::strtoull(v.c_str(), nullptr, 10);
}
// the largest band of [lo, hi) walked R rows at a time, in cells
uint64_t largest_band_cells(uint64_t lo, uint64_t hi, uint64_t R) {
    uint64_t cells = 0;
    for (uint64_t b = lo; b < hi; b += std::min(R, hi - b)) cells = std::max(cells, tri(b + std::min(R, hi - b)) - tri(b));
    return cells;
}
// the stripe of rows [i0, i1) a table is written by: the rows from i0 that hold `budget` cells together (row i has i), one at least, none from `hi` on
uint64_t next_stripe(uint64_t i0, uint64_t hi, uint64_t budget) {
    uint64_t i1 = i0, cells = 0;
    while (i1 < hi && (i1 == i0 || cells + i1 <= budget)) { cells += i1; ++i1; }
    return i1;
}

struct BuildInput;
struct Common {
    RowBand rows;                            // all2all | all2all-sp -rows
    uint64_t band_rows = 0;                  // all2all | all2all-sp -band-rows <R>: the rows are walked in bands of R, one band resident at a time (0: off)
    // the tiled band call: every band of -band-rows; with KMDB_ROWS_TILED=1 also the band of plain -rows (A/B with the same bytes)
    // -band-path <tree|tiled|records> names the call instead (unset: the defaults above)
    BandPath band_path = BandPath::unset;
    bool tiled() const {
        if (band_path != BandPath::unset) return band_path == BandPath::tiled;
        const char* e = std::getenv("KMDB_ROWS_TILED");
        return band_rows != 0 || (e && e[0] == '1');
    }
    // the band call this run takes: its device form, its host form, its KMDB_VERBOSE report
    struct BandCall {
        int (*to_device)(kmdb_db*, uint64_t, uint64_t, void*, const kmdb_opts*);
        int (*to_host)(kmdb_db*, uint64_t, uint64_t, uint32_t*, const kmdb_opts*);
        void (*report)(const kmdb_db*, uint64_t, uint64_t);
    };
    BandCall band_call() const {
        if (band_path == BandPath::records) return {kmdb_all2all_rows_records_device, kmdb_all2all_rows_records, report_rows_records_stats};
        if (tiled()) return {kmdb_all2all_rows_tiled_device, kmdb_all2all_rows_tiled, report_rows_tiled_stats};
        return {kmdb_all2all_rows_device, kmdb_all2all_rows, report_rows_stats};
    }
    // the band [lo, hi) into device memory at `dev`, or into host memory
    void band_to_device(kmdb_db* d, uint64_t lo, uint64_t hi, void* dev, const kmdb_opts& o) const {
        const BandCall b = band_call();
        check(b.to_device(d, lo, hi, dev, &o));
        b.report(d, lo, hi);
    }
    void band_to_host(kmdb_db* d, uint64_t lo, uint64_t hi, uint32_t* host, const kmdb_opts& o) const {
        const BandCall b = band_call();
        check(b.to_host(d, lo, hi, host, &o));
        b.report(d, lo, hi);
    }
    uint64_t seed_samples = 0;               // -from-samples -extend-from <old.db>: the samples of <old.db> (set by open_database)
    std::shared_ptr<BuildInput> from_samples;     // all2all | all2all-sp -from-samples: build's input switches; the "database" argument is the sample list
    std::string keep_db;                     // -keep-db <database>: the file `build` would have written, stored next to the table
    int threads = 0;
    int device = 0;
    int gpus = 0;                            // -gpus N: N prefix-bucket shards over the node's devices (0: one device, no sharding)
    int partition = KMDB_PARTITION_PREFIX;   // -partition prefix|range: what a shard of -gpus N is (all2all, all2all-sp)
    bool sparse = false;
    Filters filters;
    RowSampler sampler;
};

// -gpus N (all2all, all2all-sp): the database is read WITH its hashtables (the shard weights come from the items' prefix buckets),
// shard s of N goes to device s % D of the D devices the node has (from -gpu on), and the partial matrices meet in one RCCL
// reduce-scatter (kmdb_node_*).  On a node with fewer devices than shards the shards of a device run one after the other.
// -partition range: shard s is range s of N ranges of the pattern tree instead; nothing of it needs a hashtable, so the database is read
// with mode 2 (SkipHashtables) as the reference's all2all reads it (console_all2all.cpp:26).
// new2all / one2all -gpus N: query shards (KMDB_PARTITION_PREFIX_TABLES) — a shard holds the prefix shard's pruned tree and the slots of its own
// buckets, so the database is always read with its hashtables.
void node_upload(Db& db, const std::string& path, const Common& c) {
    const bool ranges = c.partition == KMDB_PARTITION_RANGE, tables = c.partition == KMDB_PARTITION_PREFIX_TABLES;
    check(kmdbh_db_load(path.c_str(), tables || (c.gpus > 1 && !ranges) ? 0 : 2, &db.h));
    const int have = kmdb_device_count();
    if (have <= c.device) throw std::runtime_error("no usable GPU (device " + std::to_string(c.device) + ")");
    std::vector<int32_t> devs;
    for (int d = c.device; d < have && (int)devs.size() < c.gpus; ++d) devs.push_back(d);
    check(kmdb_node_upload_partition(kmdbh_db_view(db.h), (uint32_t)c.gpus, devs.data(), (uint32_t)devs.size(), c.partition, &db.node));
    kmdb_node_stats st{};
    check(kmdb_node_stats_get(db.node, &st));
    if (ranges) std::cerr << "Database loaded without hashtables and sharded by range of the pattern tree: ";
    else if (tables) std::cerr << "Database sharded by k-mer prefix bucket, every shard with the tables of its own buckets: ";
    else std::cerr << "Database sharded by k-mer prefix bucket: ";
    std::cerr << st.n_shards << " shards on " << st.n_devices << " GPU(s)" << std::endl;
}
void node_report(const Db& db) {
    kmdb_node_stats st{};
    if (kmdb_node_stats_get(db.node, &st)) return;
    std::cerr << "  partition: " << (st.partition == KMDB_PARTITION_RANGE ? "range" : st.partition == KMDB_PARTITION_PREFIX_TABLES ? "prefix-tables" : "prefix") << " (plan " << st.plan_s << " s)" << std::endl;
    std::cerr << "  per device: compute " << st.call_ms << " ms, RCCL reduce-scatter " << st.collective_ms << " ms";
    if (st.rccl_version) std::cerr << " (RCCL " << st.rccl_version << ")";
    std::cerr << ", result to host " << st.d2h_ms << " ms" << std::endl;
    // every device by itself (an imbalanced shard shows here, not in the maxima above)
    for (uint32_t slot = 0; slot < st.n_devices; ++slot) {
        kmdb_node_device_stats ds{};
        if (kmdb_node_device_stats_get(db.node, slot, &ds)) break;
        std::cerr << "  GPU " << ds.device << ": " << ds.n_shards << " shard(s), " << ds.n_patterns << " nodes, " << ds.h2d_bytes / 1000000 << " MB over PCIe in " << ds.upload_s
                  << " s; " << ds.n_records << " block records, compute " << ds.call_ms << " ms, reduce-scatter " << ds.collective_ms << " ms, result " << ds.d2h_ms << " ms"
                  << std::endl;
    }
}

// seconds since the kernel started this process (exec, dynamic loading and static initialisers included; 10 ms resolution)
double since_process_start() {
    std::ifstream st("/proc/self/stat");
    std::string line;
    std::getline(st, line);
    const size_t rp = line.rfind(')');                          // the command name may hold spaces
    if (rp == std::string::npos) return -1;
    std::istringstream is(line.substr(rp + 2));
    std::string tok;
    for (int f = 3; f <= 22 && (is >> tok); ++f) {}            // field 22: starttime in clock ticks since boot
    timespec ts{};
    clock_gettime(CLOCK_BOOTTIME, &ts);
    return (double)ts.tv_sec + ts.tv_nsec * 1e-9 - std::strtod(tok.c_str(), nullptr) / (double)sysconf(_SC_CLK_TCK);
}

// End of a one-database run: the table is on disk.  Taking the process down piece by piece (the host image of the database — 9 GB at 100 M
// patterns —, the device pools allocation by allocation, the runtime's own teardown) only adds to the wall clock of the command: the OS and
// the driver reclaim everything at once when the process ends.  KMDB_FULL_TEARDOWN=1 keeps the ordinary exit (profilers that write their
// files from exit handlers need it).
// What the kernel would have to free at the end is given back first, on many threads (the host image: Db::uploaded; the upload's staging
// buffers: kmdb_db_settle): the end of the process frees pages on one thread, at 0.07 s per GB.
int finish(Db& db, std::ofstream& ofs, const std::string& path) {
    ofs.close();
    if (!ofs) throw std::runtime_error("Cannot write the output file " + path);
    if (db.dropper.joinable()) db.dropper.join();              // (its threads free the host image many times faster than the end of the process would)
    if (db.d) kmdb_db_settle(db.d);                            // the same for the upload's staging buffers
    std::cerr << "Process up for " << since_process_start() << " s" << std::endl;
    std::cout.flush();
    std::cerr.flush();
    const char* e = std::getenv("KMDB_FULL_TEARDOWN");
    if (!(e && e[0] == '1')) std::_Exit(0);
    return 0;
}

void write_header(const Db& db, std::ofstream& ofs) {
    uint64_t n = kmdbh_db_n_samples(db.h);
    std::vector<char> buf(10000 + n * 100);
    for (uint64_t i = 0; i < n; ++i) buf.resize(buf.size() + std::strlen(kmdbh_db_sample_name(db.h, i)));
    size_t len = kmdbh_format_header(db.h, buf.data(), buf.size());
    ofs.write(buf.data(), (std::streamsize)len);
}

// all2all / all2all-sp -distance <measure> (below, with the distance mode): every "-distance <measure>" taken from the arguments
std::vector<std::string> take_distance_measures(std::vector<std::string>& args) {
    std::vector<std::string> measures;
    for (std::string v; take_option(args, "-distance", v);) measures.push_back(v);
    return measures;
}
int run_all2all_distance(std::vector<std::string>& args, Common& c, const std::vector<std::string>& measures, bool sparse_forced, const char* mode);
int run_new2all_distance(std::vector<std::string>& args, Common& c, const std::vector<std::string>& measures);

// The opening of all2all, all2all-sp and their -distance form (further down, behind build): `db` holds the database on the device and what the
// rest of the run reads of it on the host — names, k-mer counts, k, fraction
void open_database(Db& db, const std::string& source, Common& c, const kmdb_opts& o);

// all2all -sparse | all2all-sp with -rows: the band is accumulated and compacted where it lies (kmdb_all2all_rows_device, then
// kmdb_sparse_from_dense_device on the cells [tri(lo), tri(hi))), the host applies every bound again as the full run does, and the header and the
// lines of samples lo .. hi - 1 are written.  Neither the triangle nor the band exists on the host.
// The lines of a sparse table, one sample's at a time: its cells in cols / vals — filter() takes those of row i of `sp` that pass every bound —
// formatted, written and counted.
struct SparseRowWriter {
    Db& db;
    const Filters& filters;
    std::ofstream& ofs;
    const uint64_t n = kmdbh_db_n_samples(db.h);
    const int k = (int)kmdbh_db_kmer_length(db.h);
    std::vector<char> row = std::vector<char>(10000 + n * 100);
    std::vector<uint32_t> cols, vals;
    size_t saved = 0;
    void filter(const kmdb_sparse_rows& sp, uint64_t i) {
        for (uint64_t e = sp.row_ptr[i]; e < sp.row_ptr[i + 1]; ++e)   // compact2's filter (array.h:424-427)
            if (filters.pass(sp.val[e], (uint32_t)kmdbh_db_sample_kmers(db.h, i), (uint32_t)kmdbh_db_sample_kmers(db.h, sp.col[e]), k)) {
                cols.push_back(sp.col[e]); vals.push_back(sp.val[e]);
            }
    }
    void write(uint64_t i) {
        const char* name = kmdbh_db_sample_name(db.h, i);
        if (row.size() < 10000 + n * 100 + std::strlen(name)) row.resize(10000 + n * 100 + std::strlen(name));
        size_t len = kmdbh_format_sparse_row(name, kmdbh_db_sample_kmers(db.h, i), cols.data(), vals.data(), cols.size(), row.data());
        ofs.write(row.data(), (std::streamsize)len);
        saved += cols.size();
        cols.clear(); vals.clear();
    }
};

int write_sparse_band(Db& db, Common& c, const kmdb_opts& o, std::ofstream& ofs, const std::string& path, uint64_t lo, uint64_t hi) {
    const uint64_t n = kmdbh_db_n_samples(db.h);
    // -band-rows <R>: the same for every band of R rows in turn — one band buffer on the device, the header once, the bands' lines one after another
    const bool banded = c.band_rows != 0;
    const uint64_t R = banded ? c.band_rows : std::max<uint64_t>(hi - lo, 1);
    std::cerr << "Calculating rows " << lo << " to " << hi << " of the matrix of common k-mers";
    if (banded) std::cerr << " in bands of " << R << " rows, storing them in " << path;
    std::cerr << "...";
    auto t0 = clk::now();
    std::vector<kmdb_cell_filter> fl = cell_filters(c.filters);
    if (fl.size() > 8) fl.clear();                              // (the host-side pass below applies every bound anyway)
    std::vector<uint32_t> counts(std::max<uint64_t>(n, 1));
    for (uint64_t i = 0; i < n; ++i) counts[i] = (uint32_t)kmdbh_db_sample_kmers(db.h, i);
    SparseRowWriter w{db, c.filters, ofs};
    {
        DeviceBand band(c.device, largest_band_cells(lo, hi, R));
        for (uint64_t b_lo = lo;;) {                            // (an empty range: one empty band, so that the header is written)
            const uint64_t b_hi = b_lo + std::min(R, hi - b_lo);
            kmdb_sparse_rows sp{};
            c.band_to_device(db.d, b_lo, b_hi, band.p, o);
            check(kmdb_sparse_from_dense_device(db.d, band.p, tri(b_lo), tri(b_hi), fl.data(), fl.size(), counts.data(), -1, &sp, &o));
            if (b_lo == lo) {
                if (!banded) {
                    std::cerr << "OK (" << since(t0) << " seconds)" << std::endl;
                    std::cerr << "Storing rows of the matrix of common k-mers in " << path << "...";
                    t0 = clk::now();
                }
                db.uploaded();
                write_header(db, ofs);
            }
            for (uint64_t i = b_lo; i < b_hi; ++i) { w.filter(sp, i); w.write(i); }
            kmdb_sparse_free(&sp);
            b_lo = b_hi;
            if (b_lo >= hi) break;
        }
    }
    std::cerr << "OK (" << since(t0) << " seconds)" << std::endl;
    std::cerr << "No. saved pairs: " << w.saved << std::endl;
    return finish(db, ofs, path);
}

// ---- all2all (console_all2all.cpp:7-89) -----------------------------------------------------------
int run_all2all(std::vector<std::string>& args, Common& c) {
    std::string v;
    take_option(args, "-buffer", v);
    take_option(args, "-bubble-size", v);
    const std::vector<std::string> measures = take_distance_measures(args);
    if (!measures.empty()) return run_all2all_distance(args, c, measures, false, "all2all");
    c.sparse = take_switch(args, "-sparse");
    if (c.sparse) c.filters.parse(args);
    if (args.size() != 2) throw usage_error("all2all");
    std::cerr << "All versus all comparison" << std::endl;
    Db db;
    std::ofstream ofs(args[1]);
    kmdb_opts o{}; o.abi_version = KMDB_ABI_VERSION; o.device = c.device; o.shard_count = 1; o.flags = KMDB_FLAG_ONE_SHOT;
    open_database(db, args[0], c, o);
    const uint64_t n = kmdbh_db_n_samples(db.h);
    const int k = (int)kmdbh_db_kmer_length(db.h);
    uint64_t r_lo = 0, r_hi = n;                                 // the rows written: all of them, or the band of -rows
    if (c.rows.on) c.rows.resolve(n, c.seed_samples, r_lo, r_hi);
    if ((c.rows.on || c.band_rows) && c.sparse) return write_sparse_band(db, c, o, ofs, args[1], r_lo, r_hi);
    // -band-rows <R>: the rows are computed and written R at a time; m holds one band (the largest one's cells) and is used again for the next
    const uint64_t R = c.band_rows ? c.band_rows : std::max<uint64_t>(r_hi - r_lo, 1);
    uint64_t cell_lo = tri(r_lo);                                // m holds the cells from here on
    std::cerr << "Calculating matrix of common k-mers..." << std::endl;
    auto t0 = clk::now();
    std::vector<uint32_t> m(largest_band_cells(r_lo, r_hi, R) + 1);
    if (db.node) { check(kmdb_node_all2all_dense(db.node, m.data(), nullptr)); node_report(db); }
    else if (c.band_rows) c.band_to_host(db.d, r_lo, r_lo + std::min(R, r_hi - r_lo), m.data(), o);      // (the first band; the others as the rows are written)
    else if (c.rows.on) c.band_to_host(db.d, r_lo, r_hi, m.data(), o);
    else {
        check(kmdb_all2all_dense(db.d, m.data(), &o));
        kmdb_stats st{};
        if (!kmdb_db_stats(db.d, &st) && st.path == KMDB_PATH_GLOBAL)
            std::cerr << "WARNING: the fast pipeline could not take this database (" << kmdb_db_fallback_reason(db.d) << "); the slow HBM-atomics kernel ran" << std::endl;
    }
    std::cerr << "OK (" << since(t0) << " seconds)" << std::endl;
    db.uploaded();                                             // (after the call: the page drop and the call's first allocations get in each other's way)
    std::cerr << "Storing matrix of common k-mers in " << args[1] << "...";
    t0 = clk::now();
    write_header(db, ofs);
    // rows formatted by a pool of threads, a stripe of rows at a time (about 32 M cells: the text of a 10 000-sample table is 300 MB), and
    // written in order (console_all2all.cpp:53-75 formats and writes row by row on one thread)
    const int nthr = (int)std::max<size_t>(1, std::min<size_t>(c.threads > 0 ? (size_t)c.threads : 16, std::thread::hardware_concurrency() ? std::thread::hardware_concurrency() : 1));
    size_t name_max = 0;
    for (uint64_t i = 0; i < n; ++i) name_max = std::max(name_max, std::strlen(kmdbh_db_sample_name(db.h, i)));
    for (uint64_t b_lo = r_lo; b_lo < r_hi;) {
        const uint64_t b_hi = b_lo + std::min(R, r_hi - b_lo);     // (one band: the whole range unless -band-rows cuts it)
        if (b_lo != r_lo) c.band_to_host(db.d, b_lo, b_hi, m.data(), o);
        cell_lo = tri(b_lo);
        for (uint64_t i0 = b_lo; i0 < b_hi;) {
            const uint64_t i1 = next_stripe(i0, b_hi, 32u << 20);
            std::vector<std::vector<char>> text(nthr);
            std::atomic<int> failed{0};
            auto work = [&](int t) {
                // thread t: the rows [a, b) of the stripe holding its share of the cells
                auto cut = [&](int q) -> uint64_t {
                    const double lo = (double)i0 * (double)i0, hi = (double)i1 * (double)i1;
                    uint64_t r = (uint64_t)std::sqrt(lo + (hi - lo) * q / nthr);
                    return std::min<uint64_t>(i1, std::max<uint64_t>(i0, r));
                };
                const uint64_t a = t == 0 ? i0 : cut(t), b = t + 1 == nthr ? i1 : cut(t + 1);
                std::vector<char>& out = text[t];
                std::vector<uint32_t> cols, vals;
                size_t used = 0;
                for (uint64_t i = a; i < b; ++i) {
                    const uint32_t* r = m.data() + (tri(i) - cell_lo);
                    const char* name = kmdbh_db_sample_name(db.h, i);
                    const size_t need = 64 + name_max + i * (c.sparse ? 22 : 11);
                    if (out.size() < used + need) out.resize(std::max(out.size() * 2, used + need));
                    if (c.sparse) {
                        cols.clear(); vals.clear();
                        for (uint64_t j = 0; j < i; ++j)     // LowerTriangularMatrix::compact + saveRowSparse (array.h:169-181,259-262)
                            if (r[j] && c.filters.pass(r[j], (uint32_t)kmdbh_db_sample_kmers(db.h, i), (uint32_t)kmdbh_db_sample_kmers(db.h, j), k)) {
                                cols.push_back((uint32_t)j); vals.push_back(r[j]);
                            }
                        used += kmdbh_format_sparse_row(name, kmdbh_db_sample_kmers(db.h, i), cols.data(), vals.data(), cols.size(), out.data() + used);
                    } else {
                        used += kmdbh_format_dense_row(name, kmdbh_db_sample_kmers(db.h, i), r, i, out.data() + used);
                    }
                }
                out.resize(used);
            };
            std::vector<std::thread> pool;
            for (int t = 1; t < nthr; ++t) pool.emplace_back([&, t]() { try { work(t); } catch (...) { failed = 1; } });
            work(0);
            for (auto& th : pool) th.join();
            if (failed) throw std::runtime_error("out of memory while formatting the table");
            for (auto& tx : text) ofs.write(tx.data(), (std::streamsize)tx.size());
            i0 = i1;
        }
        b_lo = b_hi;
    }
    std::cerr << "OK (" << since(t0) << " seconds)" << std::endl;
    return finish(db, ofs, args[1]);
}

// ---- all2all-sp (console_all2all_sparse.cpp:13-111) -------------------------------------------------
int run_all2all_sp(std::vector<std::string>& args, Common& c) {
    std::string v;
    take_option(args, "-buffer", v);
    uint32_t bubble = 8000;
    if (take_option(args, "-bubble-size", v)) bubble = (uint32_t)std::strtoul(v.c_str(), nullptr, 10);
    const std::vector<std::string> measures = take_distance_measures(args);
    if (!measures.empty()) return run_all2all_distance(args, c, measures, true, "all2all-sp");
    take_switch(args, "-sparse");
    c.filters.parse(args);
    c.sampler.parse(args);
    if (args.size() != 2) throw usage_error("all2all-sp");
    std::cerr << "All versus all comparison (sparse computation)" << std::endl;
    Db db;
    std::ofstream ofs(args[1], std::ios::binary);
    kmdb_opts o{}; o.abi_version = KMDB_ABI_VERSION; o.device = c.device; o.shard_count = 1; o.bubble_size = bubble; o.flags = KMDB_FLAG_ONE_SHOT;
    open_database(db, args[0], c, o);
    const uint64_t n = kmdbh_db_n_samples(db.h);
    const int k = (int)kmdbh_db_kmer_length(db.h);
    if (c.rows.on || c.band_rows) {
        uint64_t r_lo = 0, r_hi = n;
        if (c.rows.on) c.rows.resolve(n, c.seed_samples, r_lo, r_hi);
        return write_sparse_band(db, c, o, ofs, args[1], r_lo, r_hi);
    }
    std::cerr << "Calculating matrix of common k-mers...";
    auto t0 = clk::now();
    kmdb_sparse_rows sp{};
    {
        // the -min / -max filters go with the call: cells that miss a bound never leave the device
        std::vector<kmdb_cell_filter> fl = cell_filters(c.filters);
        std::vector<uint32_t> counts(n);
        for (uint64_t i = 0; i < n; ++i) counts[i] = (uint32_t)kmdbh_db_sample_kmers(db.h, i);
        if (c.sampler.on() && c.sampler.best) {
            // -sample-rows <criterion>:<count> (console_all2all_sparse.cpp:70-89): candidates on the device, the exact decision in the library —
            // `sp` holds the sampled rows themselves, every bound applied
            if (db.node) { check(kmdb_node_all2all_sampled(db.node, fl.data(), fl.size(), counts.data(), c.sampler.criterion_id, (uint32_t)std::min<size_t>(c.sampler.cap, 0xFFFFFFFFu), &sp, nullptr)); node_report(db); }
            else {
                check(kmdb_all2all_sampled(db.d, fl.data(), fl.size(), counts.data(), c.sampler.criterion_id, (uint32_t)std::min<size_t>(c.sampler.cap, 0xFFFFFFFFu), &sp, &o));
                kmdb_sample_stats ss{};
                if (!kmdb_db_sample_stats(db.d, &ss))
                    std::cerr << "(" << ss.candidates << " candidates, " << ss.rows_truncated << " rows truncated, " << ss.rows_refetched << " fetched again, selection "
                              << ss.select_ms << " ms, " << ss.d2h_bytes << " bytes to the host) ";
            }
        } else {
        if (fl.size() > 8) fl.clear();                          // (the host-side pass below applies every bound anyway)
        if (db.node) { check(kmdb_node_all2all_sparse(db.node, fl.data(), fl.size(), counts.data(), -1, &sp, nullptr)); node_report(db); }
        else if (fl.empty()) check(kmdb_all2all_sparse(db.d, &sp, &o));
        else check(kmdb_all2all_sparse_filtered(db.d, fl.data(), fl.size(), counts.data(), -1, &sp, &o));
        }
    }
    std::cerr << "OK (" << since(t0) << " seconds)" << std::endl;
    db.uploaded();                                             // (after the call: the page drop and the call's first allocations get in each other's way)
    std::cerr << "Storing matrix of common k-mers in " << args[1] << "...";
    t0 = clk::now();
    write_header(db, ofs);
    SparseRowWriter w{db, c.filters, ofs};
    const bool sampled_rows = c.sampler.on() && c.sampler.best;      // `sp` holds the rows to write
    if (c.sampler.on() && !sampled_rows) {
        // -sample-rows <count>, the random strategy (console_all2all_sparse.cpp:70-76, array.h:450-540): every pair that passes the filters is
        // offered to both its samples
        c.sampler.init(n);
        for (uint64_t i = 0; i < n; ++i)
            for (uint64_t e = sp.row_ptr[i]; e < sp.row_ptr[i + 1]; ++e) {
                const uint32_t ci = (uint32_t)kmdbh_db_sample_kmers(db.h, i), cj = (uint32_t)kmdbh_db_sample_kmers(db.h, sp.col[e]);
                if (!c.filters.pass(sp.val[e], ci, cj, k)) continue;
                const double sc = c.sampler.score(sp.val[e], ci, cj, k);
                c.sampler.add(i, sp.col[e], sp.val[e], sc);
                c.sampler.add(sp.col[e], (uint32_t)i, sp.val[e], sc);
            }
    }
    for (uint64_t i = 0; i < n; ++i) {
        if (sampled_rows) { w.cols.assign(sp.col + sp.row_ptr[i], sp.col + sp.row_ptr[i + 1]); w.vals.assign(sp.val + sp.row_ptr[i], sp.val + sp.row_ptr[i + 1]); }
        else if (c.sampler.on()) c.sampler.finish_row(i, w.cols, w.vals);
        else w.filter(sp, i);
        w.write(i);
    }
    kmdb_sparse_free(&sp);
    std::cerr << "OK (" << since(t0) << " seconds)" << std::endl;
    std::cerr << "No. saved pairs: " << w.saved << std::endl;
    return finish(db, ofs, args[1]);
}

// ---- all2all-parts (console_all2all_parts.cpp:21-399): a collection split into several databases --------------
// Grid of cells (row part, column part <= row part): the diagonal cells are all2all_sp of one database, the others
// db2db_sp + compact2 of two (similarity_calculator.cpp:1225-1540, console_all2all_parts.cpp:179-195 -> kmdb_db2db_sparse_filtered).  Row k of row part i is written as the
// concatenation of its cells' sparse rows with the column index shifted by the samples of the earlier parts
// (:292-310), which is the sparse lower-triangular matrix of the whole collection.
// the list of database files and what every mode over the grid needs of the whole collection (console_all2all_parts.cpp:60-100): every database
// is read once up front for its names and k-mer counts
struct PartsCollection {
    std::vector<std::string> files, names;
    std::vector<uint64_t> counts, part_n;
    uint32_t k = 0;
    double fraction = 0;
};
PartsCollection read_parts_collection(const std::string& list) {
    PartsCollection pc;
    std::ifstream lst(list);
    if (!lst) throw std::runtime_error("Cannot open file with list of database files " + list);
    for (std::string ln; std::getline(lst, ln);) {
        while (!ln.empty() && (ln.back() == '\r' || ln.back() == ' ')) ln.pop_back();
        if (!ln.empty()) pc.files.push_back(ln);
    }
    if (pc.files.empty()) throw std::runtime_error("Empty list of database files");
    for (size_t i = 0; i < pc.files.size(); ++i) {
        Db d;
        if (kmdbh_db_load(pc.files[i].c_str(), 2, &d.h)) throw std::runtime_error("Cannot open k-mer database " + pc.files[i]);
        if (i == 0) { pc.k = kmdbh_db_kmer_length(d.h); pc.fraction = kmdbh_db_fraction(d.h); }
        else if (pc.k != kmdbh_db_kmer_length(d.h) || pc.fraction != kmdbh_db_fraction(d.h))
            throw std::runtime_error("Databases have different k-mer lengths or fractions");
        const uint64_t n = kmdbh_db_n_samples(d.h);
        pc.part_n.push_back(n);
        for (uint64_t s = 0; s < n; ++s) { pc.names.push_back(kmdbh_db_sample_name(d.h, s)); pc.counts.push_back(kmdbh_db_sample_kmers(d.h, s)); }
    }
    return pc;
}

int run_all2all_parts_distance(std::vector<std::string>& args, Common& c, const std::vector<std::string>& measures);

int run_all2all_parts(std::vector<std::string>& args, Common& c) {
    const std::vector<std::string> measures = take_distance_measures(args);
    if (!measures.empty()) return run_all2all_parts_distance(args, c, measures);
    std::string v;
    take_option(args, "-buffer", v);
    take_option(args, "-bubble-size", v);
    take_switch(args, "-sparse");
    c.filters.parse(args);
    c.sampler.parse(args);
    if (args.size() != 2) throw usage_error("all2all-parts");
    std::cerr << "All versus all comparison (parts)" << std::endl;
    PartsCollection pc = read_parts_collection(args[0]);
    const std::vector<std::string>& files = pc.files;
    const std::vector<std::string>& names = pc.names;
    const std::vector<uint64_t>&counts = pc.counts, &part_n = pc.part_n;
    const uint32_t k = pc.k;
    const double fraction = pc.fraction;
    kmdb_opts o{}; o.abi_version = KMDB_ABI_VERSION; o.device = c.device; o.shard_count = 1;
    std::ofstream ofs(args[1], std::ios::binary);
    {
        char head[128];
        std::snprintf(head, sizeof head, "kmer-length: %u fraction: %g ,db-samples ,", k, fraction);
        ofs << head;
        for (auto& nm : names) ofs << nm << ",";
        ofs << "\nquery-samples,total-kmers,";
        for (auto cnt : counts) ofs << cnt << ",";
        ofs << "\n";
    }
    // Every part serves as the row database once and as a column database for all later rows: uploaded parts stay resident while HBM
    // lasts (an upload that fails evicts the others and is tried again).
    // -gpus W ("the grid maps to a multi-GPU grid of cells"; reference console_all2all_parts.cpp:143-331 walks the cells on
    // one CPU): the block rows of the grid are dealt to W workers — worker t takes the rows t, t + W, ... on device `-gpu` + t % (devices of
    // the node), its parts resident on ITS device — and the rows' text is written in order as the blocks complete.  Cell (i, j) needs
    // both parts on one device, so a part lives on every device whose rows reach it; nothing crosses between devices.
    std::vector<uint64_t> row_start(files.size() + 1, 0);
    for (size_t i = 0; i < files.size(); ++i) row_start[i + 1] = row_start[i] + part_n[i];
    const int have = std::max(1, kmdb_device_count());
    const size_t W = c.gpus > 0 ? std::min<size_t>((size_t)c.gpus, files.size()) : 1;
    struct Worker {
        kmdb_opts o{};
        std::vector<std::unique_ptr<Db>> resident;
    };
    std::vector<Worker> workers(W);
    for (size_t t = 0; t < W; ++t) {
        workers[t].o = o;
        workers[t].o.device = c.device + (int)(t % (size_t)std::max(1, have - c.device));
        workers[t].resident.resize(files.size());
    }
    if (W > 1) std::cerr << "Block rows of the grid dealt to " << W << " workers on " << std::min<size_t>(W, (size_t)std::max(1, have - c.device)) << " GPU(s)" << std::endl;
    std::vector<std::string> block_text(files.size());
    std::vector<size_t> block_saved(files.size(), 0);
    std::vector<char> block_done(files.size(), 0);
    std::mutex mu;
    std::condition_variable cv;
    std::exception_ptr failure;
    // the -min / -max bounds go with every cell's call (as for all2all-sp); the k-mer counts as the library takes them (num_kmers_t = uint32)
    std::vector<kmdb_cell_filter> fl = cell_filters(c.filters);
    const std::vector<kmdb_cell_filter> fl_all = fl;             // every bound: what a sampled call takes (a selection without a bound is no superset)
    if (fl.size() > 8) fl.clear();                                // (the rows are checked with every bound below anyway)
    std::vector<uint32_t> counts32(counts.begin(), counts.end());
    const bool dense_cells = std::getenv("KMDB_PARTS_DENSE_CELLS") != nullptr;
    // -sample-rows <criterion>:<count>: every cell's candidates are selected on the device (kmdb_db2db_sampled, kmdb_all2all_sampled on the
    // diagonal) and only those reach the sampler.  The random strategy, KMDB_PARTS_DENSE_CELLS=1, more bounds than the device takes and
    // KMDB_PARTS_HOST_SAMPLER=1 (A/B) keep the host path: every kept pair of every cell goes through the sampler.  The bytes written are the same.
    // (The device takes 12 bounds.  Every -min / -max given counts as one here, before a measure's two fold into one lo / hi pair — the cautious
    // reading: the folded list, at most one pair per measure, could never exceed 12 by itself.)
    const bool device_sampler = c.sampler.on() && c.sampler.best && !dense_cells && c.filters.given <= 12 && fl_all.size() <= 12 &&
                                std::getenv("KMDB_PARTS_HOST_SAMPLER") == nullptr;
    const bool verbose = std::getenv("KMDB_VERBOSE") != nullptr;
    auto block_row = [&](Worker& wk, size_t i) {
        auto get = [&](size_t p, size_t keep) -> Db& {
            if (wk.resident[p]) return *wk.resident[p];
            auto d = std::make_unique<Db>();
            check(kmdbh_db_load(files[p].c_str(), 0, &d->h));
            if (kmdb_db_upload(kmdbh_db_view(d->h), &wk.o, 1, &d->d)) {
                for (size_t j = 0; j < wk.resident.size(); ++j) if (j != keep) wk.resident[j].reset();
                check(kmdb_db_upload(kmdbh_db_view(d->h), &wk.o, 1, &d->d));
            }
            kmdbh_db_free(d->h); d->h = nullptr;                   // the host copy is not needed once the part is in HBM
            wk.resident[p] = std::move(d);
            return *wk.resident[p];
        };
        std::vector<char> row(10000 + names.size() * 100);
        std::vector<uint32_t> cols, vals;
        std::string text;
        size_t saved = 0;
        const uint64_t row_shift = row_start[i];
        Db& drow = get(i, i);
        const uint64_t nr = part_n[i];
        if (device_sampler) {
            // (console_all2all_parts.cpp:179-195, 225-241 with a sampler: db2db_sp, compact2(filter), add_to_sampler.)  A sample's best `count` of
            // one cell is a superset of its share of its best `count` overall, and finish_row is exact on any superset.  A pair has one score, the
            // later part's sample being the row sample; each side of a pair is added only where the device selected it for that side.
            const uint32_t cap = (uint32_t)std::min<size_t>(c.sampler.cap, 0xFFFFFFFFu);
            const uint32_t* row_counts = counts32.data() + row_shift;
            for (size_t j = 0; j < i; ++j) {
                { std::lock_guard<std::mutex> g(mu); std::cerr << "Processing cell (" << i + 1 << "," << j + 1 << ")" << std::endl; }
                Db& dcol = get(j, i);
                const uint64_t shift_j = row_start[j], nc = part_n[j];
                const uint32_t* col_counts = counts32.data() + shift_j;
                std::vector<kmdb_sparse_rows> cand(2, kmdb_sparse_rows{});      // [0]: the row samples' candidates, [1]: the column samples'
                struct FreeRows { std::vector<kmdb_sparse_rows>& v; ~FreeRows() { for (auto& x : v) kmdb_sparse_free(&x); } } free_cand{cand};
                auto sampled = [&]() {
                    return kmdb_db2db_sampled(drow.d, dcol.d, fl_all.data(), fl_all.size(), row_counts, col_counts, c.sampler.criterion_id, cap, &cand[0], &cand[1], &wk.o);
                };
                if (sampled()) {
                    for (size_t q = 0; q < wk.resident.size(); ++q) if (q != i && q != j) wk.resident[q].reset();
                    check(sampled());
                }
                for (uint64_t r = 0; r < nr; ++r)
                    for (uint64_t e = cand[0].row_ptr[r]; e < cand[0].row_ptr[r + 1]; ++e) {
                        const uint32_t col = cand[0].col[e], v = cand[0].val[e], a = row_counts[r], b = col_counts[col];
                        if (c.filters.pass(v, a, b, (int)k)) c.sampler.add(row_shift + r, (uint32_t)(shift_j + col), v, c.sampler.score(v, a, b, (int)k));
                    }
                for (uint64_t cs = 0; cs < nc; ++cs)
                    for (uint64_t e = cand[1].row_ptr[cs]; e < cand[1].row_ptr[cs + 1]; ++e) {
                        const uint32_t rw = cand[1].col[e], v = cand[1].val[e], a = row_counts[rw], b = col_counts[cs];
                        if (c.filters.pass(v, a, b, (int)k)) c.sampler.add(shift_j + cs, (uint32_t)(row_shift + rw), v, c.sampler.score(v, a, b, (int)k));
                    }
                if (verbose) {
                    kmdb_sample_stats ss{};
                    kmdb_db2db_stats ds{};
                    if (!kmdb_db2db_sample_stats_get(drow.d, &ss) && !kmdb_db2db_stats_get(drow.d, &ds)) {
                        std::lock_guard<std::mutex> g(mu);
                        std::fprintf(stderr, "[kmdb] all2all-parts: sampled cell (%zu,%zu): %llu of %llu tiles touched, %llu candidates, %llu rows truncated, %llu re-fetched, selection %.3f ms\n",
                                     i + 1, j + 1, (unsigned long long)ds.tiles_touched, (unsigned long long)ds.tiles, (unsigned long long)ss.candidates,
                                     (unsigned long long)ss.rows_truncated, (unsigned long long)ss.rows_refetched, ss.select_ms);
                    }
                }
            }
            { std::lock_guard<std::mutex> g(mu); std::cerr << "Processing cell (" << i + 1 << "," << i + 1 << ")" << std::endl; }
            // the diagonal cell: the part's own symmetric rows, selected and decided by the library
            kmdb_sparse_rows sp{};
            auto diagonal = [&]() { return kmdb_all2all_sampled(drow.d, fl_all.data(), fl_all.size(), row_counts, c.sampler.criterion_id, cap, &sp, &wk.o); };
            if (diagonal()) {
                for (size_t q = 0; q < wk.resident.size(); ++q) if (q != i) wk.resident[q].reset();
                check(diagonal());
            }
            for (uint64_t s = 0; s < nr; ++s)
                for (uint64_t e = sp.row_ptr[s]; e < sp.row_ptr[s + 1]; ++e) {
                    const uint32_t o = sp.col[e], v = sp.val[e], a = row_counts[std::max<uint64_t>(s, o)], b = row_counts[std::min<uint64_t>(s, o)];
                    if (c.filters.pass(v, a, b, (int)k)) c.sampler.add(row_shift + s, (uint32_t)(row_shift + o), v, c.sampler.score(v, a, b, (int)k));
                }
            kmdb_sparse_free(&sp);
            std::lock_guard<std::mutex> g(mu);
            block_text[i].clear(); block_saved[i] = 0; block_done[i] = 1;
            cv.notify_all();
            return;
        }
        // A cell is kept as the reference keeps it (:179-195, 225-241: db2db_sp, then compact2 with the -min / -max filter): compacted and filtered
        // on the device, a CSR per earlier part of the block row.  KMDB_PARTS_DENSE_CELLS=1: the dense rectangles of kmdb_db2db_dense, scanned on the
        // host (the previous path, for A/B); the bytes written are the same.
        std::vector<kmdb_sparse_rows> cross_sp(dense_cells ? 0 : i, kmdb_sparse_rows{});
        std::vector<std::vector<uint32_t>> cross(dense_cells ? i : 0);   // cross[j]: nr x part_n[j]
        struct FreeRows { std::vector<kmdb_sparse_rows>& v; ~FreeRows() { for (auto& x : v) kmdb_sparse_free(&x); } } free_rows{cross_sp};
        const uint32_t* row_counts = counts32.data() + row_shift;
        for (size_t j = 0; j < i; ++j) {
            { std::lock_guard<std::mutex> g(mu); std::cerr << "Processing cell (" << i + 1 << "," << j + 1 << ")" << std::endl; }
            Db& dcol = get(j, i);
            if (dense_cells) {
                cross[j].resize(nr * part_n[j] + 1);
                if (kmdb_db2db_dense(drow.d, dcol.d, cross[j].data(), &wk.o)) {
                    // out of HBM inside the call (its scratch, lazily made working sets): the other resident parts go, one more try
                    for (size_t q = 0; q < wk.resident.size(); ++q) if (q != i && q != j) wk.resident[q].reset();
                    check(kmdb_db2db_dense(drow.d, dcol.d, cross[j].data(), &wk.o));
                }
                continue;
            }
            const uint32_t* col_counts = counts32.data() + row_start[j];
            if (kmdb_db2db_sparse_filtered(drow.d, dcol.d, fl.data(), fl.size(), row_counts, col_counts, -1, &cross_sp[j], &wk.o)) {
                for (size_t q = 0; q < wk.resident.size(); ++q) if (q != i && q != j) wk.resident[q].reset();
                check(kmdb_db2db_sparse_filtered(drow.d, dcol.d, fl.data(), fl.size(), row_counts, col_counts, -1, &cross_sp[j], &wk.o));
            }
        }
        { std::lock_guard<std::mutex> g(mu); std::cerr << "Processing cell (" << i + 1 << "," << i + 1 << ")" << std::endl; }
        kmdb_sparse_rows sp{};
        auto diagonal = [&]() {
            if (dense_cells || fl.empty()) return kmdb_all2all_sparse(drow.d, &sp, &wk.o);
            return kmdb_all2all_sparse_filtered(drow.d, fl.data(), fl.size(), row_counts, -1, &sp, &wk.o);
        };
        if (diagonal()) {
            for (size_t q = 0; q < wk.resident.size(); ++q) if (q != i) wk.resident[q].reset();
            check(diagonal());
        }
        for (uint64_t r = 0; r < nr; ++r) {
            cols.clear(); vals.clear();
            const uint32_t cr = (uint32_t)counts[row_shift + r];
            uint64_t shift = 0;
            for (size_t j = 0; j < i; ++j) {
                if (dense_cells) {
                    const uint32_t* m = cross[j].data() + r * part_n[j];
                    for (uint64_t cidx = 0; cidx < part_n[j]; ++cidx)
                        if (m[cidx] && c.filters.pass(m[cidx], cr, (uint32_t)counts[shift + cidx], (int)k)) {
                            cols.push_back((uint32_t)(shift + cidx)); vals.push_back(m[cidx]);
                        }
                } else {
                    // (the bounds were applied inside the call; pass() is the front-end's own statement of them and costs a look per KEPT cell)
                    const kmdb_sparse_rows& x = cross_sp[j];
                    for (uint64_t e = x.row_ptr[r]; e < x.row_ptr[r + 1]; ++e)
                        if (c.filters.pass(x.val[e], cr, (uint32_t)counts[shift + x.col[e]], (int)k)) {
                            cols.push_back((uint32_t)(shift + x.col[e])); vals.push_back(x.val[e]);
                        }
                }
                shift += part_n[j];
            }
            for (uint64_t e = sp.row_ptr[r]; e < sp.row_ptr[r + 1]; ++e)
                if (c.filters.pass(sp.val[e], cr, (uint32_t)counts[shift + sp.col[e]], (int)k)) {
                    cols.push_back((uint32_t)(shift + sp.col[e])); vals.push_back(sp.val[e]);
                }
            if (c.sampler.on()) {
                // -sample-rows (console_all2all_parts.cpp:137,191,237,275): the pairs go to the sampler (both samples of a pair), the rows are
                // written when every cell is done — the pairs of one sample arrive from several block rows: add() locks the sample's stripe
                for (size_t e = 0; e < cols.size(); ++e) {
                    const double sc = c.sampler.score(vals[e], cr, (uint32_t)counts[cols[e]], (int)k);
                    c.sampler.add(row_shift + r, cols[e], vals[e], sc);
                    c.sampler.add(cols[e], (uint32_t)(row_shift + r), vals[e], sc);
                }
                continue;
            }
            const std::string& name = names[row_shift + r];
            if (row.size() < 10000 + names.size() * 100 + name.size()) row.resize(10000 + names.size() * 100 + name.size());
            size_t len = kmdbh_format_sparse_row(name.c_str(), counts[row_shift + r], cols.data(), vals.data(), cols.size(), row.data());
            text.append(row.data(), len);
            saved += cols.size();
        }
        kmdb_sparse_free(&sp);
        std::lock_guard<std::mutex> g(mu);
        block_text[i] = std::move(text); block_saved[i] = saved; block_done[i] = 1;
        cv.notify_all();
    };
    if (c.sampler.on()) c.sampler.init(names.size());
    std::vector<std::thread> pool;
    for (size_t t = 0; t < W; ++t)
        pool.emplace_back([&, t]() {
            try {
                for (size_t i = t; i < files.size(); i += W) {
                    { std::lock_guard<std::mutex> g(mu); if (failure) return; }
                    block_row(workers[t], i);
                }
            } catch (...) {
                std::lock_guard<std::mutex> g(mu);
                if (!failure) failure = std::current_exception();
                cv.notify_all();
            }
        });
    size_t saved = 0;
    for (size_t i = 0; i < files.size(); ++i) {
        std::unique_lock<std::mutex> g(mu);
        cv.wait(g, [&] { return block_done[i] || failure; });
        if (!block_done[i]) break;
        std::string text = std::move(block_text[i]);
        saved += block_saved[i];
        g.unlock();
        ofs.write(text.data(), (std::streamsize)text.size());
    }
    for (auto& th : pool) th.join();
    workers.clear();                                              // (the parts' handles go before the process ends)
    if (failure) std::rethrow_exception(failure);
    if (c.sampler.on()) {
        // the sampled rows, every cell being in (console_all2all_parts.cpp:333-345).  (Random strategy: the subset of a row depends on the order
        // its pairs arrived in — block rows in the workers' order; with a criterion the rows do not depend on it.)
        std::vector<char> row(10000 + names.size() * 100);
        std::vector<uint32_t> cols, vals;
        for (size_t sidx = 0; sidx < names.size(); ++sidx) {
            c.sampler.finish_row(sidx, cols, vals);
            if (row.size() < 10000 + names.size() * 100 + names[sidx].size()) row.resize(10000 + names.size() * 100 + names[sidx].size());
            const size_t len = kmdbh_format_sparse_row(names[sidx].c_str(), counts[sidx], cols.data(), vals.data(), cols.size(), row.data());
            ofs.write(row.data(), (std::streamsize)len);
            saved += cols.size();
        }
    }
    std::cerr << "No. saved pairs: " << saved << std::endl;
    return 0;
}

// ---- query loading (genome_input_file.h:60-137, 287-337; loader_ex.cpp:22-124,168) ------------------
bool slurp(const std::string& base, std::string& data) {
    static const char* exts[] = {"", ".fa", ".fna", ".fasta", ".gz", ".fa.gz", ".fna.gz", ".fasta.gz"};
    for (const char* e : exts) {
        std::string p = base + e;
        if (FILE* f = std::fopen(p.c_str(), "rb")) {
            std::fclose(f);
            gzFile g = gzopen(p.c_str(), "rb");          // transparent for plain text
            if (!g) return false;
            data.clear();
            char buf[1 << 16];
            int n;
            while ((n = gzread(g, buf, sizeof buf)) > 0) data.append(buf, (size_t)n);
            gzclose(g);
            return true;
        }
    }
    return false;
}

struct Record { std::string header, seq; };

void split_fasta(const std::string& data, std::vector<Record>& recs) {
    size_t pos = data.find('>');
    while (pos != std::string::npos) {
        size_t eol = data.find('\n', pos);
        if (eol == std::string::npos) eol = data.size();
        Record r;
        r.header = data.substr(pos + 1, eol - pos - 1);
        if (!r.header.empty() && r.header.back() == '\r') r.header.pop_back();
        size_t sp = r.header.find(' ');
        if (sp != std::string::npos) r.header.resize(sp);        // header up to the first space
        size_t next = data.find('>', eol);
        size_t end = next == std::string::npos ? data.size() : next;
        r.seq.reserve(end > eol ? end - eol : 0);
        for (size_t i = eol + 1; i < end; ++i) {
            char ch = data[i];
            if (ch != '\n' && ch != '\r') r.seq.push_back(ch);
        }
        recs.push_back(std::move(r));
        pos = next;
    }
}

struct Query {
    std::string name;
    std::vector<uint64_t> kmers;             // from_kmers: sorted unique k-mers (the host loader; a long query: the stand-alone device extractor)
    std::string text;                        // else: records joined by '\n' (device-side extraction)
    bool from_kmers = false;
    std::string error;                       // a device extraction that failed on a reader thread: thrown where the query is handed on
};
// the loader inside the new2all call indexes positions with 32 bits: the k-mers of a longer query are extracted by the stand-alone extractor
// (kmdb_minhash_batch_seq_alphabet: in sections, on the device) and enter as a k-mer list.  KMDB_LONG_QUERY_BASES lowers the threshold (tests).
constexpr size_t LONG_QUERY_BASES = 1800u << 20;
// KMDB_VERBOSE: what the last extractor call of this thread did with its long samples
void report_long_samples(const char* mode) {
    kmdb_minhash_long_stats ls{};
    if (!std::getenv("KMDB_VERBOSE") || kmdb_minhash_long_stats_get(&ls) || !ls.long_samples) return;
    std::cerr << "[kmdb] " << mode << ": " << ls.long_samples << " long samples in " << ls.sections << " sections; unions " << ls.union_words_in << " words in, "
              << ls.union_words_out << " out, " << ls.union_ms << " ms; peak " << ls.peak_bytes << " device bytes" << std::endl;
}
size_t long_query_bases() {
    if (const char* e = std::getenv("KMDB_LONG_QUERY_BASES")) return (size_t)std::max<unsigned long long>(1, std::strtoull(e, nullptr, 10));
    return LONG_QUERY_BASES;
}
// the sorted unique k-mers of one long query, by the device extractor with the database's own k, window and alphabet
void extract_long_query(const std::string& text, uint32_t k, int32_t alphabet, double fraction, double fstart, int device, std::vector<uint64_t>& kmers) {
    static std::mutex one_at_a_time;         // (the reader threads: one long text on the device at a time)
    std::lock_guard<std::mutex> lock(one_at_a_time);
    kmdb_opts o{}; o.abi_version = KMDB_ABI_VERSION; o.device = device; o.shard_count = 1;
    const char* tp = text.data();
    const size_t tl = text.size();
    kmdb_kmer_lists lists{};
    check(kmdb_minhash_batch_seq_alphabet(&tp, &tl, 1, k, fraction, fstart, alphabet, &lists, &o));
    report_long_samples("long query");
    struct FreeLists { kmdb_kmer_lists& l; ~FreeLists() { kmdb_kmer_lists_free(&l); } } free_lists{lists};
    kmers.assign(lists.kmers, lists.kmers + lists.offsets[1]);
}

std::string basename_of(const std::string& p) {
    size_t s = p.find_last_of('/');
    return s == std::string::npos ? p : p.substr(s + 1);
}

const char* const KMC_REFUSAL = "KMC k-mer input (-from-kmers) is not supported by the GPU front-end";

// <entry>.minhash as MihashedInputFile::open reads it (minhashed_input_file.h:58-84): false when it cannot be opened or is damaged
bool load_minhash(const std::string& entry, std::vector<uint64_t>& kmers, uint32_t& k) {
    uint64_t* p = nullptr;
    size_t n = 0;
    double f = 0;
    if (kmdbh_minhash_load((entry + ".minhash").c_str(), &p, &n, &k, &f)) return false;
    try { kmers.assign(p, p + n); } catch (...) { kmdbh_minhash_free(p); throw; }
    kmdbh_minhash_free(p);
    return true;
}

// ---- minhash (console_minhash.cpp:7-52, params.cpp:674-716): every sample's filtered, sorted, unique k-mers into <sample>.minhash --------
// The loader + KmerHelper::sortAndUnique run on the device for a batch of samples at a time (kmdb_minhash_batch_seq_alphabet);
// a sample of any length goes there (a long one in sections); -host-extract takes kmdbh_extract_kmers_alphabet + kmdbh_sort_unique and
// never touches a device.  The files are MihashedInputFile::store's, byte for byte (kmdbh_minhash_store).
int run_minhash(std::vector<std::string>& args, Common& c) {
    if (take_switch(args, "-from-kmers")) throw std::runtime_error(KMC_REFUSAL);
    if (take_switch(args, "-multisample-fasta"))
        throw std::runtime_error("minhash -multisample-fasta is not supported: the reference stores every sample of the file under the file's own name, and only the last one survives");
    const bool host_extract = take_switch(args, "-host-extract");
    double fraction = 0.01;                                        // the mode's own default (params.cpp:130-133)
    uint32_t k = 18;
    std::string v;
    if (take_option(args, "-f", v)) { std::istringstream iss(v); if (!(iss >> fraction)) throw std::runtime_error("Unable to parse the fraction: " + v); }
    take_option(args, "-f-start", v);                              // accepted and ignored: the mode's filter starts at 0 (console_minhash.cpp:19)
    if (take_option(args, "-k", v)) k = (uint32_t)std::strtoul(v.c_str(), nullptr, 10);
    int32_t alphabet = KMDB_ALPHABET_NT;
    if (take_option(args, "-alphabet", v)) {
        static const char* names[KMDB_ALPHABET_COUNT] = {"nt", "nt-preserve", "aa", "aa11_diamond", "aa12_mmseqs", "aa6_dayhoff"};      // alphabet.h:79-86
        alphabet = -1;
        for (int a = 0; a < KMDB_ALPHABET_COUNT; ++a) if (v == names[a]) alphabet = a;
        if (alphabet < 0) throw std::runtime_error("Unknown alphabet: " + v);
    }
    if (take_switch(args, "-preserve-strand")) {
        if (alphabet != KMDB_ALPHABET_NT) throw std::runtime_error("Switch -preserve-strand applies only to nt alphabet");
        alphabet = KMDB_ALPHABET_NT_PRESERVE;
    }
    if (args.size() != 1) throw usage_error("minhash");
    {
        int8_t map[256];
        uint32_t size = 0, bits = 0;
        kmdbh_alphabet_table(alphabet, map, &size, &bits, nullptr);
        if (k == 0 || k > 64u / bits - 1u) throw std::runtime_error("k-mer length must be 1.." + std::to_string(64u / bits - 1u) + " for this alphabet");
    }
    std::cerr << "Minhashing samples..." << std::endl;
    // LoaderEx::configure (loader_ex.cpp:87-122): a FASTA file is one sample, anything else a list of samples
    std::vector<std::string> entries;
    bool is_fasta = false;
    for (const char* ext : {".fa", ".fna", ".fasta", ".fastq", ".gz", ".fa.gz", ".fna.gz", ".fasta.gz", ".fastq.gz"}) {
        const size_t n = std::strlen(ext);
        if (args[0].size() >= n && args[0].compare(args[0].size() - n, n, ext) == 0) is_fasta = true;
    }
    if (is_fasta) entries.push_back(args[0]);
    else {
        std::ifstream lst(args[0]);
        if (!lst) throw std::runtime_error("Unable to open input file " + args[0]);
        for (std::string e; lst >> e;) entries.push_back(e);
    }
    const auto total0 = clk::now();
    kmdb_opts o{}; o.abi_version = KMDB_ABI_VERSION; o.device = c.device; o.shard_count = 1;
    const int nthreads = c.threads > 0 ? c.threads : (int)std::max(1u, std::thread::hardware_concurrency());
    struct Sample { std::string entry, text; std::vector<uint64_t> kmers; bool ok = false, on_host = false; };
    auto store = [&](const std::string& entry, const uint64_t* km, size_t n) {
        check(kmdbh_minhash_store((entry + ".minhash").c_str(), km, n, k, fraction));      // console_minhash.cpp:47
    };
    size_t stored = 0;
    const size_t BATCH = 64, BATCH_BASES = 512u << 20;             // by count and by bases, as new2all batches its queries
    for (size_t base = 0; base < entries.size();) {
        // the next batch: read and split on a pool of threads (the host path extracts there too), in input order
        const size_t cnt = std::min(BATCH, entries.size() - base);
        std::vector<Sample> ss(cnt);
        std::atomic<size_t> next{0};
        std::atomic<int> failed{0};
        auto worker = [&]() {
            try {
                for (size_t i; (i = next.fetch_add(1)) < cnt;) {
                    Sample& s = ss[i];
                    s.entry = entries[base + i];
                    std::string data;
                    if (!slurp(s.entry, data)) continue;
                    std::vector<Record> recs;
                    split_fasta(data, recs);
                    size_t bytes = 0, total = 0;
                    for (auto& r : recs) { bytes += r.seq.size() + 1; total += r.seq.size(); }
                    s.on_host = host_extract;
                    if (s.on_host) {
                        s.kmers.resize(total + 1);
                        size_t n = 0;
                        for (auto& r : recs) n += kmdbh_extract_kmers_alphabet(r.seq.data(), r.seq.size(), k, alphabet, fraction, 0.0, s.kmers.data() + n);
                        s.kmers.resize(kmdbh_sort_unique(s.kmers.data(), n));        // KmerHelper::sortAndUnique (console_minhash.cpp:40)
                    } else {
                        s.text.reserve(bytes);
                        for (auto& r : recs) { s.text += r.seq; s.text += '\n'; }
                    }
                    s.ok = true;
                }
            } catch (...) { failed = 1; }
        };
        std::vector<std::thread> pool;
        for (int t = 0; t < std::min<int>(nthreads, (int)cnt); ++t) pool.emplace_back(worker);
        for (auto& t : pool) t.join();
        if (failed) throw std::runtime_error("out of memory while reading the samples");
        // device calls over stretches of the batch of at most BATCH_BASES bases (a longer sample is a stretch of its own)
        for (size_t i0 = 0; i0 < cnt;) {
            std::vector<size_t> idx;
            size_t bases = 0, i1 = i0;
            for (; i1 < cnt && (idx.empty() || bases + ss[i1].text.size() <= BATCH_BASES); ++i1)
                if (ss[i1].ok && !ss[i1].on_host) { idx.push_back(i1); bases += ss[i1].text.size(); }
            kmdb_kmer_lists lists{};
            if (!idx.empty()) {
                std::vector<const char*> ptrs(idx.size());
                std::vector<size_t> lens(idx.size());
                for (size_t t = 0; t < idx.size(); ++t) { ptrs[t] = ss[idx[t]].text.data(); lens[t] = ss[idx[t]].text.size(); }
                check(kmdb_minhash_batch_seq_alphabet(ptrs.data(), lens.data(), idx.size(), k, fraction, 0.0, alphabet, &lists, &o));
                report_long_samples("minhash");
            }
            struct FreeLists { kmdb_kmer_lists& l; ~FreeLists() { kmdb_kmer_lists_free(&l); } } free_lists{lists};
            size_t t = 0;
            for (size_t i = i0; i < i1; ++i) {
                const Sample& s = ss[i];
                if (!s.ok) { std::cerr << "failed:" << s.entry << std::endl; continue; }
                if (s.on_host) store(s.entry, s.kmers.data(), s.kmers.size());
                else { store(s.entry, lists.kmers + lists.offsets[t], (size_t)(lists.offsets[t + 1] - lists.offsets[t])); ++t; }
                ++stored;
            }
            i0 = i1;
        }
        base += cnt;
    }
    std::cerr << stored << " of " << entries.size() << " samples minhashed" << std::endl;
    std::cerr << std::endl << std::endl << "EXECUTION TIMES" << std::endl << "Total: " << since(total0) << std::endl;
    return 0;
}


// ---- build (console_build.cpp:33-158, params.cpp:459-513, loader_ex.cpp:86-124, 165-168): genomes (or <sample>.minhash files) in, a database out ----
// db.addKmers per sample (:111) is kmdb_build_add_seq_alphabet / kmdb_build_add_kmers for a batch of samples, serialize (:149) is
// kmdb_build_finish + kmdbh_db_store.  The samples take their ids in input order; a file that cannot be opened prints "failed:<path>" and takes none.
// build's input switches (params.cpp:459-513), with build's defaults, checks and messages: `build` and `all2all | all2all-sp -from-samples` read them
struct BuildInput {
    bool from_minhash = false, host_extract = false, multi = false, extend = false;
    double fraction = 1.0, fstart = 0.0;
    uint32_t k = 18;
    int32_t alphabet = KMDB_ALPHABET_NT;
    std::string seed_path;
    void parse(std::vector<std::string>& args);
};
void BuildInput::parse(std::vector<std::string>& args) {
    const bool from_kmers = take_switch(args, "-from-kmers");
    from_minhash = take_switch(args, "-from-minhash");
    if (from_kmers && from_minhash) throw std::runtime_error("-from-kmers and -from-minhash switches exclude one another.");      // params.cpp:499-502
    if (from_kmers) throw std::runtime_error(KMC_REFUSAL);
    if (take_switch(args, "-extend")) throw std::runtime_error("build -extend is not supported: rebuild from the sample list");
    host_extract = take_switch(args, "-host-extract");
    std::string v;
    // -extend-from <old.db>: the builder starts from a stored database (console_build.cpp:48-57).  k, fraction, start fraction and alphabet are
    // the database's own; -k, -f, -f-start, -alphabet and -preserve-strand are accepted and ignored, as the reference's -extend does
    extend = take_option(args, "-extend-from", seed_path);
    if (extend) {
        take_option(args, "-f", v); take_option(args, "-f-start", v); take_option(args, "-alphabet", v); take_option(args, "-k", v);
        take_switch(args, "-preserve-strand");
        multi = take_switch(args, "-multisample-fasta");
    } else if (!from_minhash) {
        if (take_option(args, "-f", v)) { std::istringstream iss(v); if (!(iss >> fraction)) throw std::runtime_error("Unable to parse the fraction: " + v); }
        if (take_option(args, "-f-start", v)) { std::istringstream iss(v); if (!(iss >> fstart)) throw std::runtime_error("Unable to parse the start fraction: " + v); }
        multi = take_switch(args, "-multisample-fasta");
        if (take_option(args, "-alphabet", v)) {
            static const char* names[KMDB_ALPHABET_COUNT] = {"nt", "nt-preserve", "aa", "aa11_diamond", "aa12_mmseqs", "aa6_dayhoff"};      // alphabet.h:79-86
            alphabet = -1;
            for (int a = 0; a < KMDB_ALPHABET_COUNT; ++a) if (v == names[a]) alphabet = a;
            if (alphabet < 0) throw std::runtime_error("Unknown alphabet: " + v);
        }
        if (take_switch(args, "-preserve-strand")) {
            if (alphabet != KMDB_ALPHABET_NT) throw std::runtime_error("Switch -preserve-strand applies only to nt alphabet");
            alphabet = KMDB_ALPHABET_NT_PRESERVE;
        }
        if (take_option(args, "-k", v)) k = (uint32_t)std::strtoul(v.c_str(), nullptr, 10);
        int8_t map[256];
        uint32_t size = 0, bits = 0;
        kmdbh_alphabet_table(alphabet, map, &size, &bits, nullptr);
        if (k == 0 || k > 64u / bits - 1u) throw std::runtime_error("K-mer length for the given alphabet cannot exceed " + std::to_string(64u / bits - 1u));
    }
}

struct BuilderHold { kmdb_builder* b = nullptr; ~BuilderHold() { kmdb_build_free(b); } };

// The sample-feeding loop of build: the seed (-extend-from) is loaded, the list read, every sample extracted and added in input order; bld.b
// is the fed builder, not yet finished.  k, fraction and alphabet of `in` end as the builder's (a seed's, a .minhash file's).
void build_feed(BuildInput& in, const std::string& input, Common& c, BuilderHold& bld) {
    const bool from_minhash = in.from_minhash, host_extract = in.host_extract, multi = in.multi, extend = in.extend;
    double &fraction = in.fraction, &fstart = in.fstart;
    uint32_t& k = in.k;
    int32_t& alphabet = in.alphabet;
    const std::string& seed_path = in.seed_path;
    struct HostDb { kmdbh_db* h = nullptr; ~HostDb() { if (h) kmdbh_db_free(h); } } old;
    if (extend) {                                                  // read with its tables, before anything else is opened and before any device is touched
        std::cerr << "Loading k-mer database " << seed_path << "..." << std::endl;
        if (kmdbh_db_load(seed_path.c_str(), 0, &old.h)) throw std::runtime_error("Cannot open k-mer database " + seed_path);
        k = kmdbh_db_kmer_length(old.h); fraction = kmdbh_db_fraction(old.h); fstart = kmdbh_db_start_fraction(old.h); alphabet = kmdbh_db_alphabet(old.h);
    }
    // LoaderEx::configure (loader_ex.cpp:87-122): a FASTA file is one input file, anything else a list of them
    std::vector<std::string> entries;
    bool is_fasta = false;
    for (const char* ext : {".fa", ".fna", ".fasta", ".fastq", ".gz", ".fa.gz", ".fna.gz", ".fasta.gz", ".fastq.gz"}) {
        const size_t n = std::strlen(ext);
        if (input.size() >= n && input.compare(input.size() - n, n, ext) == 0) is_fasta = true;
    }
    if (is_fasta) entries.push_back(input);
    else {
        std::ifstream lst(input);
        if (!lst) throw std::runtime_error("Unable to open input file " + input);
        for (std::string e; lst >> e;) entries.push_back(e);
    }
    std::cerr << "Processing samples..." << std::endl;
    const auto total0 = clk::now();
    double extract_s = 0, update_s = 0;
    kmdb_opts o{}; o.abi_version = KMDB_ABI_VERSION; o.device = c.device; o.shard_count = 1;
    const int nthreads = c.threads > 0 ? c.threads : (int)std::max(1u, std::thread::hardware_concurrency());
    if (extend) {
        check(kmdb_build_begin_from_db(old.h, &o, &bld.b));
        kmdbh_db_free(old.h);                                      // the builder holds the state now
        old.h = nullptr;
        kmdb_build_seed_stats ss{};
        if (std::getenv("KMDB_VERBOSE") && !kmdb_build_seed_stats_get(bld.b, &ss))
            std::cerr << "[kmdb] build: seeded from " << ss.samples << " samples, " << ss.distinct_kmers << " distinct k-mers, " << ss.patterns << " patterns, " << ss.events
                      << " events, " << ss.slots << " slots, " << ss.h2d_bytes << " bytes to the device; upload " << ss.upload_ms << " dictionary " << ss.dict_ms << " tree "
                      << ss.tree_ms << " decode " << ss.decode_ms << " checks " << ss.check_ms << " ms" << std::endl;
    }
    struct Sample { std::string name, text; std::vector<uint64_t> kmers; bool on_host = false; };
    struct File { std::string entry; std::vector<Sample> samples; bool ok = false; uint32_t k = 0; double fraction = 0; };
    size_t added = 0;
    const size_t BATCH = 64, BATCH_BASES = 512u << 20;             // by count and by bases, as the minhash mode batches its samples
    for (size_t base = 0; base < entries.size();) {
        const size_t cnt = std::min(BATCH, entries.size() - base);
        std::vector<File> files(cnt);
        std::atomic<size_t> next{0};
        std::atomic<int> failed{0};
        const auto t_read = clk::now();
        auto worker = [&]() {
            try {
                for (size_t i; (i = next.fetch_add(1)) < cnt;) {
                    File& f = files[i];
                    f.entry = entries[base + i];
                    if (from_minhash) {
                        Sample s;
                        s.on_host = true;
                        s.name = basename_of(f.entry);
                        uint64_t* p = nullptr;
                        size_t n = 0;
                        if (kmdbh_minhash_load((f.entry + ".minhash").c_str(), &p, &n, &f.k, &f.fraction)) continue;
                        try { s.kmers.assign(p, p + n); } catch (...) { kmdbh_minhash_free(p); throw; }
                        kmdbh_minhash_free(p);
                        f.samples.push_back(std::move(s));
                        f.ok = true;
                        continue;
                    }
                    std::string data;
                    if (!slurp(f.entry, data)) continue;
                    std::vector<Record> recs;
                    split_fasta(data, recs);
                    // one sample per file, named after the file (loader_ex.cpp:165-168) — or, with -multisample-fasta, one per record, named by its header
                    const size_t ns = multi ? recs.size() : 1;
                    for (size_t r0 = 0; r0 < ns; ++r0) {
                        const size_t r1 = multi ? r0 + 1 : recs.size();
                        Sample s;
                        s.name = multi ? recs[r0].header : basename_of(f.entry);
                        size_t bytes = 0, total = 0;
                        for (size_t r = r0; r < r1; ++r) { bytes += recs[r].seq.size() + 1; total += recs[r].seq.size(); }
                        s.on_host = host_extract;
                        if (s.on_host) {
                            s.kmers.resize(total + 1);
                            size_t n = 0;
                            for (size_t r = r0; r < r1; ++r) n += kmdbh_extract_kmers_alphabet(recs[r].seq.data(), recs[r].seq.size(), k, alphabet, fraction, fstart, s.kmers.data() + n);
                            s.kmers.resize(kmdbh_sort_unique(s.kmers.data(), n));      // console_build.cpp:97-102
                        } else {
                            s.text.reserve(bytes);
                            for (size_t r = r0; r < r1; ++r) { s.text += recs[r].seq; s.text += '\n'; }
                        }
                        f.samples.push_back(std::move(s));
                    }
                    f.ok = true;
                }
            } catch (...) { failed = 1; }
        };
        std::vector<std::thread> pool;
        for (int t = 0; t < std::min<int>(nthreads, (int)cnt); ++t) pool.emplace_back(worker);
        for (auto& t : pool) t.join();
        if (failed) throw std::runtime_error("out of memory while reading the samples");
        extract_s += since(t_read);
        // the batch's samples in input order
        std::vector<Sample*> ss;
        for (File& f : files) {
            if (!f.ok) { std::cerr << "failed:" << f.entry << std::endl; continue; }
            if (from_minhash) {
                if (!bld.b) { k = f.k; fraction = f.fraction; }                // (a seeded builder is there already: the files must match the database)
                // AbstractKmerDb::addKmers (kmer_db.h:116-121)
                if (f.k != k) throw std::runtime_error("Error in AbstractKmerDb::addKmers(): adding kmers of different length");
                if (f.fraction != fraction) throw std::runtime_error("Error in AbstractKmerDb::addKmers(): adding kmers of different minhash fraction");
            }
            if (!bld.b) check(kmdb_build_begin(k, fraction, fstart, alphabet, &o, &bld.b));
            for (Sample& s : f.samples) ss.push_back(&s);
        }
        // stretches of one kind (text: at most BATCH_BASES bases), one call each: the sample ids follow the input order
        const auto t_add = clk::now();
        for (size_t i0 = 0; i0 < ss.size();) {
            size_t i1 = i0, bases = 0;
            const bool on_host = ss[i0]->on_host;
            for (; i1 < ss.size() && ss[i1]->on_host == on_host && (on_host || i1 == i0 || bases + ss[i1]->text.size() <= BATCH_BASES); ++i1) bases += ss[i1]->text.size();
            const size_t m = i1 - i0;
            std::vector<const char*> names(m);
            for (size_t t = 0; t < m; ++t) names[t] = ss[i0 + t]->name.c_str();
            if (on_host) {
                std::vector<const uint64_t*> ptrs(m);
                std::vector<size_t> kc(m);
                for (size_t t = 0; t < m; ++t) { ptrs[t] = ss[i0 + t]->kmers.data(); kc[t] = ss[i0 + t]->kmers.size(); }
                check(kmdb_build_add_kmers(bld.b, names.data(), ptrs.data(), kc.data(), m));
            } else {
                std::vector<const char*> ptrs(m);
                std::vector<size_t> lens(m);
                for (size_t t = 0; t < m; ++t) { ptrs[t] = ss[i0 + t]->text.data(); lens[t] = ss[i0 + t]->text.size(); }
                check(kmdb_build_add_seq_alphabet(bld.b, names.data(), ptrs.data(), lens.data(), m));
                report_long_samples("build");
            }
            added += m;
            i0 = i1;
        }
        update_s += since(t_add);
        base += cnt;
    }
    std::cerr << added << "/" << added << "                      " << std::endl;
    if (!bld.b) throw std::runtime_error("no sample could be read: the database would be empty");
    std::cerr << std::endl << std::endl << "EXECUTION TIMES" << std::endl << "Total: " << since(total0) << std::endl
              << "Kmer sorting/unique time: " << extract_s << std::endl << "Database update time:" << update_s << std::endl;
}

int run_build(std::vector<std::string>& args, Common& c) {
    BuildInput in;
    in.parse(args);
    if (args.size() != 2) throw usage_error("build");
    std::cerr << "Building database (from " << (in.from_minhash ? "minhashed k-mers" : "fasta genomes") << ")" << std::endl;
    struct HostDb { kmdbh_db* h = nullptr; ~HostDb() { if (h) kmdbh_db_free(h); } } built;
    BuilderHold bld;
    build_feed(in, args[0], c, bld);
    check(kmdb_build_finish(bld.b, &built.h));
    kmdb_build_stats st{};
    if (std::getenv("KMDB_VERBOSE") && !kmdb_build_stats_get(bld.b, &st))
        std::cerr << "[kmdb] build: " << st.samples << " samples, " << st.kmers_added << " k-mers, " << st.distinct_kmers << " distinct, " << st.patterns << " patterns, "
                  << st.events << " events, peak " << st.peak_device_bytes << " device bytes; merge " << st.merge_ms << " lookup " << st.lookup_ms << " sort " << st.sort_ms
                  << " group " << st.group_ms << " encode " << st.encode_ms << " tables " << st.tables_ms << " copy-back " << st.copy_back_ms << " ms" << std::endl;
    std::cerr << "Serializing database..." << std::endl;
    check(kmdbh_db_store(built.h, args[1].c_str()));
    return 0;
}

void open_database(Db& db, const std::string& source, Common& c, const kmdb_opts& o) {
    if (c.from_samples) {
        // -from-samples: `source` is build's sample list.  The builder is fed as by `build`, then handed to the engine where it lies
        // (kmdb_build_finish_device): db.h is the header-only image, or with -keep-db the full one, stored at once — finish() leaves through _Exit
        BuildInput& in = *c.from_samples;
        std::cerr << "Building database (from " << (in.from_minhash ? "minhashed k-mers" : "fasta genomes") << ")" << std::endl;
        BuilderHold bld;
        build_feed(in, source, c, bld);
        kmdb_build_seed_stats seed{};
        if (in.extend && !kmdb_build_seed_stats_get(bld.b, &seed)) c.seed_samples = seed.samples;      // (-rows new starts here)
        const auto tu = clk::now();
        const bool keep = !c.keep_db.empty();
        check(kmdb_build_finish_device(bld.b, &o, 0, keep ? 1 : 0, &db.d, &db.h));
        std::cerr << "Database handed to the engine in " << since(tu) << " s" << std::endl;
        kmdb_build_handoff_stats hs{};
        if (std::getenv("KMDB_VERBOSE") && !kmdb_build_handoff_stats_get(bld.b, &hs))
            std::cerr << "[kmdb] hand-off: " << hs.samples << " samples, " << hs.patterns << " patterns, peak " << hs.peak_device_bytes << " device bytes (handle "
                      << hs.handle_device_bytes << "), " << hs.d2h_bytes << " bytes to the host; encode " << hs.encode_ms << " tables " << hs.tables_ms << " fields "
                      << hs.fields_ms << " layout " << hs.layout_ms << " prepare " << hs.prepare_ms << " copy-back " << hs.copy_back_ms << " total " << hs.total_ms << " ms"
                      << std::endl;
        if (keep) {
            std::cerr << "Serializing database..." << std::endl;
            check(kmdbh_db_store(db.h, c.keep_db.c_str()));
        }
        return;
    }
    std::cerr << "Loading k-mer database " << source << "..." << std::endl;
    if (c.gpus > 0) { node_upload(db, source, c); return; }
    const auto tl = clk::now();
    std::thread warm([&]() { (void)kmdb_device_prepare(c.device); });      // the device's first use, next to the read of the file (an error shows at the upload)
    const int load_rc = kmdbh_db_load(source.c_str(), 2, &db.h);
    const std::string load_err = load_rc ? kmdb_last_error() : "";
    warm.join();
    if (load_rc) throw std::runtime_error(load_err);
    const double load_s = since(tl);
    const auto tu = clk::now();
    check(kmdb_db_upload(kmdbh_db_view(db.h), &o, 0, &db.d));
    std::cerr << "Database loaded in " << load_s << " s, uploaded in " << since(tu) << " s" << std::endl;
}

// The queries of a new2all run (console_new2all.cpp:64-74): read, extracted and handed on in input order, in batches of 64 queries — flushed by
// size as well as by count: the engine's scratch grows with the bases.  flush() takes what `batch` holds and clears it.  A list entry that
// cannot be read is announced as "failed:<path>" and left out.
struct QuerySource {
    bool from_minhash, multi, host_extract;
    uint32_t k;
    int32_t alphabet;
    double fraction, fstart;
    int nthreads;
    int device;                              // where a long query's k-mers are extracted
};
template <class Flush>
void new2all_queries(const std::vector<std::string>& entries, const QuerySource& s, std::vector<Query>& batch, Flush&& flush) {
    const bool from_minhash = s.from_minhash, multi = s.multi, host_extract = s.host_extract;
    const uint32_t k = s.k;
    const int32_t alphabet = s.alphabet;
    const double fraction = s.fraction, fstart = s.fstart;
    const int nthreads = s.nthreads;
    size_t batch_bases = 0;
    auto make_query = [&](const std::string& name, const std::vector<const std::string*>& seqs) {
        Query q;
        q.name = name;
        size_t bytes = 0;
        for (auto* s : seqs) bytes += s->size() + 1;
        const bool long_query = bytes >= long_query_bases();
        q.from_kmers = host_extract || long_query;
        if (!host_extract) {
            q.text.reserve(bytes);
            for (auto* s : seqs) { q.text += *s; q.text += '\n'; }
            if (!long_query) return q;
            // the same window, k and alphabet as the call's own loader; the query enters as the k-mer list a long query always entered as
            try { extract_long_query(q.text, k, alphabet, fraction, fstart, s.device, q.kmers); } catch (const std::exception& e) { q.error = e.what(); }
            std::string().swap(q.text);
            return q;
        }
        size_t total = 0;
        for (auto* s : seqs) total += s->size();
        q.kmers.resize(total + 1);
        size_t cnt = 0;
        for (auto* s : seqs) cnt += kmdbh_extract_kmers_alphabet(s->data(), s->size(), k, alphabet, fraction, fstart, q.kmers.data() + cnt);
        cnt = kmdbh_sort_unique(q.kmers.data(), cnt);              // KmerHelper::unique (console_new2all.cpp:73)
        q.kmers.resize(cnt);
        return q;
    };

    const size_t BATCH = 64, BATCH_BASES = 512u << 20;
    auto add = [&](Query&& q) {
        if (!q.error.empty()) throw std::runtime_error(q.error);
        batch_bases += q.text.size() + q.kmers.size();
        batch.push_back(std::move(q));
        if (batch.size() == BATCH || batch_bases >= BATCH_BASES) { flush(); batch_bases = 0; }
    };
    if (multi) {
        for (auto& e : entries) {
            std::string data;
            if (!slurp(e, data)) { std::cerr << "failed:" << e << std::endl; continue; }
            std::vector<Record> recs;
            split_fasta(data, recs);
            for (auto& r : recs) {
                add(make_query(r.header, {&r.seq}));
            }
        }
    } else {
        for (size_t base = 0; base < entries.size(); base += BATCH) {
            size_t cntq = std::min(BATCH, entries.size() - base);
            std::vector<Query> qs(cntq);
            std::vector<char> okv(cntq, 0);
            std::atomic<size_t> next{0};
            auto worker = [&]() {
                for (size_t i; (i = next.fetch_add(1)) < cntq;) {
                    if (from_minhash) {
                        uint32_t fk = 0;
                        if (!load_minhash(entries[base + i], qs[i].kmers, fk)) continue;      // (cannot be opened, or damaged)
                        qs[i].name = basename_of(entries[base + i]);
                        qs[i].from_kmers = true;
                        okv[i] = 1;
                        continue;
                    }
                    std::string data;
                    if (!slurp(entries[base + i], data)) continue;
                    std::vector<Record> recs;
                    split_fasta(data, recs);
                    std::vector<const std::string*> seqs;
                    for (auto& r : recs) seqs.push_back(&r.seq);
                    qs[i] = make_query(basename_of(entries[base + i]), seqs);
                    okv[i] = 1;
                }
            };
            std::vector<std::thread> pool;
            for (int t = 0; t < std::min<int>(nthreads, (int)cntq); ++t) pool.emplace_back(worker);
            for (auto& t : pool) t.join();
            for (size_t i = 0; i < cntq; ++i) {
                if (!okv[i]) { std::cerr << "failed:" << entries[base + i] << std::endl; continue; }
                add(std::move(qs[i]));
            }
        }
    }
    flush();
}

// ---- new2all (console_new2all.cpp:12-174) ---------------------------------------------------------
int run_new2all(std::vector<std::string>& args, Common& c) {
    if (take_switch(args, "-from-kmers")) throw std::runtime_error(KMC_REFUSAL);
    const bool sample_rows = std::find(args.begin(), args.end(), "-sample-rows") != args.end();
    const std::vector<std::string> measures = take_distance_measures(args);
    if (!measures.empty() && sample_rows) throw std::runtime_error("new2all: -sample-rows does not go with -distance: sampled rows are no rows of the table");
    if (!measures.empty()) return run_new2all_distance(args, c, measures);
    // -sample-rows <criterion>:<count>: a search — every query keeps its `count` best database samples (the rule of sampler.h:44-67 on the sparse
    // row; the database samples collect nothing).  The output is always the sparse form.
    c.sampler.parse(args);
    if (sample_rows && !c.sampler.best)
        throw std::runtime_error("new2all: -sample-rows needs <criterion>:<count>: the random strategy (a count alone) has no meaning for a search");
    // -from-minhash: every list entry names <entry>.minhash; its words go to the k-mer entries AS STORED — the database's filter is not applied
    // again (MihashedInputFile::load, minhashed_input_file.h:88-105)
    const bool from_minhash = take_switch(args, "-from-minhash");
    const bool multi = take_switch(args, "-multisample-fasta");
    if (multi && from_minhash) throw usage_error("new2all");
    const bool host_extract = take_switch(args, "-host-extract");   // k-mer extraction on the host instead of the device
    c.sparse = take_switch(args, "-sparse") || c.sampler.on();
    if (c.sparse) c.filters.parse(args);
    if (args.size() != 3) throw usage_error("new2all");
    std::cerr << "Set of new samples  (from " << (from_minhash ? "minhashed k-mers" : "genomes") << ") versus entire database comparison" << std::endl;
    Db db;
    std::cerr << "Loading k-mer database " << args[0] << "..." << std::endl;
    auto t0 = clk::now();
    kmdb_opts o{}; o.abi_version = KMDB_ABI_VERSION; o.device = c.device; o.shard_count = 1;
    // -gpus N: N query shards over the node's devices (console_new2all.cpp:64-95 made multi-GPU: kmdb_node_new2all_*)
    if (c.gpus > 0) { c.partition = KMDB_PARTITION_PREFIX_TABLES; node_upload(db, args[0], c); }
    else {
        check(kmdbh_db_load(args[0].c_str(), 0, &db.h));
        check(kmdb_db_upload(kmdbh_db_view(db.h), &o, 1, &db.d));
    }
    std::cerr << "OK (" << since(t0) << " seconds)" << std::endl;
    const uint64_t n = kmdbh_db_n_samples(db.h);
    const uint32_t k = kmdbh_db_kmer_length(db.h);
    const double fraction = kmdbh_db_fraction(db.h), fstart = kmdbh_db_start_fraction(db.h);
    const int32_t alphabet = kmdbh_db_alphabet(db.h);              // AlphabetType as the file stores it (alphabet.h:10-18): nt, nt-preserve, four protein alphabets
    if (alphabet < 0 || alphabet >= KMDB_ALPHABET_COUNT) throw std::runtime_error("Invalid alphabet type");

    std::ifstream lst(args[1]);
    if (!lst) throw std::runtime_error("Unable to open sample list " + args[1]);
    std::vector<std::string> entries;
    for (std::string ln; std::getline(lst, ln);) {
        while (!ln.empty() && (ln.back() == '\r' || ln.back() == ' ')) ln.pop_back();
        if (!ln.empty()) entries.push_back(ln);
    }
    std::cerr << "Processing queries..." << std::endl;
    auto total0 = clk::now();
    std::ofstream ofs(args[2]);
    write_header(db, ofs);
    std::vector<char> row(10000 + n * 100);
    int nthreads = c.threads > 0 ? c.threads : (int)std::max(1u, std::thread::hardware_concurrency());

    // queries are produced in input order; similarities are computed in batches on the GPU and rows
    // written in the same order (the reference re-orders through a priority queue, :60,114-117)
    std::vector<Query> batch;
    // -sparse: the rows are compacted and the -min / -max bounds applied on the device (kmdb_new2all_batch*_sparse_filtered: one2all_sp + the row's
    // CombinedFilter, console_new2all.cpp:76-78, 130-148); KMDB_N2A_DENSE_ROWS=1 keeps the dense rows and the host's filter (A/B, same bytes)
    // -sample-rows: the candidates of every query are selected on the device and decided by the library (kmdb_new2all_batch*_sampled);
    // KMDB_N2A_HOST_SAMPLER=1 takes the filtered sparse rows to the host's RowSampler instead (A/B, same bytes)
    const bool sampled_on_device = c.sampler.on() && !std::getenv("KMDB_N2A_HOST_SAMPLER");
    const uint32_t sample_cap = (uint32_t)std::min<size_t>(c.sampler.cap, 0xFFFFFFFFu);
    const bool sparse_on_device = c.sparse && (c.sampler.on() || !std::getenv("KMDB_N2A_DENSE_ROWS"));
    const bool verbose = std::getenv("KMDB_VERBOSE") != nullptr;
    std::vector<kmdb_cell_filter> fl;
    std::vector<uint32_t> sample_counts(n);
    for (uint64_t j = 0; j < n; ++j) sample_counts[j] = (uint32_t)kmdbh_db_sample_kmers(db.h, j);
    if (sparse_on_device) fl = cell_filters(c.filters);
    auto flush = [&]() {
        if (batch.empty()) return;
        std::vector<size_t> cnts(batch.size());
        std::vector<uint32_t> out(sparse_on_device ? 1 : batch.size() * n + 1);
        // a query is either sequence text (loader + KmerHelper::unique + one2all on the device, kmdb_new2all_batch_seq) or,
        // with -host-extract and for genomes beyond the call's own loader (2^31 positions; extracted on the device beforehand), a k-mer list (kmdb_new2all_batch)
        std::vector<size_t> by_text, by_kmers;
        for (size_t q = 0; q < batch.size(); ++q) (batch[q].from_kmers ? by_kmers : by_text).push_back(q);
        // sparse rows of the two halves, and where query q's row is: {half, row}
        struct Rows { kmdb_sparse_rows r{}; ~Rows() { kmdb_sparse_free(&r); } } sp[2];
        std::vector<std::pair<int, size_t>> where(batch.size());
        kmdb_new2all_sparse_stats tot{};
        kmdb_sample_stats stot{};
        auto account = [&]() {
            if (sampled_on_device) {
                kmdb_sample_stats st{};
                if (db.node ? kmdb_node_new2all_sample_stats_get(db.node, &st) : kmdb_new2all_sample_stats_get(db.d, &st)) return;
                stot.candidates += st.candidates; stot.rows_truncated += st.rows_truncated; stot.rows_refetched += st.rows_refetched;
                stot.d2h_bytes += st.d2h_bytes; stot.select_ms += st.select_ms;
                return;
            }
            kmdb_new2all_sparse_stats st{};
            if (db.node ? kmdb_node_new2all_sparse_stats_get(db.node, &st) : kmdb_new2all_sparse_stats_get(db.d, &st)) return;
            tot.cells += st.cells; tot.nnz_device += st.nnz_device; tot.nnz += st.nnz; tot.d2h_bytes += st.d2h_bytes; tot.compact_ms += st.compact_ms;
        };
        if (!by_kmers.empty()) {
            std::vector<const uint64_t*> ptrs(by_kmers.size());
            std::vector<size_t> kc(by_kmers.size());
            for (size_t t = 0; t < by_kmers.size(); ++t) { ptrs[t] = batch[by_kmers[t]].kmers.data(); kc[t] = batch[by_kmers[t]].kmers.size(); }
            if (sparse_on_device) {
                if (sampled_on_device) {
                    if (db.node)
                        check(kmdb_node_new2all_batch_sampled(db.node, ptrs.data(), kc.data(), by_kmers.size(), fl.data(), fl.size(), sample_counts.data(),
                                                              c.sampler.criterion_id, sample_cap, &sp[0].r, nullptr));
                    else
                        check(kmdb_new2all_batch_sampled(db.d, ptrs.data(), kc.data(), by_kmers.size(), fl.data(), fl.size(), sample_counts.data(),
                                                         c.sampler.criterion_id, sample_cap, &sp[0].r, &o));
                }
                else if (db.node) check(kmdb_node_new2all_batch_sparse_filtered(db.node, ptrs.data(), kc.data(), by_kmers.size(), fl.data(), fl.size(), sample_counts.data(), -1, &sp[0].r, nullptr));
                else check(kmdb_new2all_batch_sparse_filtered(db.d, ptrs.data(), kc.data(), by_kmers.size(), fl.data(), fl.size(), sample_counts.data(), -1, &sp[0].r, &o));
                account();
                for (size_t t = 0; t < by_kmers.size(); ++t) { cnts[by_kmers[t]] = kc[t]; where[by_kmers[t]] = {0, t}; }
            } else {
            std::vector<uint32_t> part(by_kmers.size() * n + 1);
            if (db.node) check(kmdb_node_new2all_batch(db.node, ptrs.data(), kc.data(), by_kmers.size(), part.data(), nullptr));
            else check(kmdb_new2all_batch(db.d, ptrs.data(), kc.data(), by_kmers.size(), part.data(), &o));
            for (size_t t = 0; t < by_kmers.size(); ++t) {
                cnts[by_kmers[t]] = kc[t];
                std::copy(part.begin() + t * n, part.begin() + (t + 1) * n, out.begin() + by_kmers[t] * n);
            }
            }
        }
        if (!by_text.empty()) {
            std::vector<const char*> ptrs(by_text.size());
            std::vector<size_t> lens(by_text.size());
            std::vector<uint64_t> uniq(by_text.size());
            for (size_t t = 0; t < by_text.size(); ++t) { ptrs[t] = batch[by_text[t]].text.data(); lens[t] = batch[by_text[t]].text.size(); }
            if (sparse_on_device) {
                if (sampled_on_device) {
                    if (db.node)
                        check(kmdb_node_new2all_batch_seq_alphabet_sampled(db.node, ptrs.data(), lens.data(), by_text.size(), fraction, fstart, alphabet, fl.data(),
                                                                           fl.size(), sample_counts.data(), c.sampler.criterion_id, sample_cap, &sp[1].r, uniq.data(),
                                                                           nullptr));
                    else
                        check(kmdb_new2all_batch_seq_alphabet_sampled(db.d, ptrs.data(), lens.data(), by_text.size(), fraction, fstart, alphabet, fl.data(), fl.size(),
                                                                      sample_counts.data(), c.sampler.criterion_id, sample_cap, &sp[1].r, uniq.data(), &o));
                }
                else if (db.node) check(kmdb_node_new2all_batch_seq_alphabet_sparse_filtered(db.node, ptrs.data(), lens.data(), by_text.size(), fraction, fstart, alphabet, fl.data(), fl.size(), sample_counts.data(), -1, &sp[1].r, uniq.data(), nullptr));
                else check(kmdb_new2all_batch_seq_alphabet_sparse_filtered(db.d, ptrs.data(), lens.data(), by_text.size(), fraction, fstart, alphabet, fl.data(), fl.size(), sample_counts.data(), -1, &sp[1].r, uniq.data(), &o));
                account();
                for (size_t t = 0; t < by_text.size(); ++t) { cnts[by_text[t]] = (size_t)uniq[t]; where[by_text[t]] = {1, t}; }
            } else {
            std::vector<uint32_t> part(by_text.size() * n + 1);
            if (db.node) check(kmdb_node_new2all_batch_seq_alphabet(db.node, ptrs.data(), lens.data(), by_text.size(), fraction, fstart, alphabet, part.data(), uniq.data(), nullptr));
            else check(kmdb_new2all_batch_seq_alphabet(db.d, ptrs.data(), lens.data(), by_text.size(), fraction, fstart, alphabet, part.data(), uniq.data(), &o));
            for (size_t t = 0; t < by_text.size(); ++t) {
                cnts[by_text[t]] = (size_t)uniq[t];
                std::copy(part.begin() + t * n, part.begin() + (t + 1) * n, out.begin() + by_text[t] * n);
            }
            }
        }
        if (sampled_on_device && verbose)
            std::cerr << "[kmdb] new2all: sampled batch of " << batch.size() << " queries: " << stot.candidates << " candidates, " << stot.rows_truncated
                      << " rows truncated, " << stot.rows_refetched << " fetched again, select " << stot.select_ms << " ms, " << stot.d2h_bytes
                      << " bytes to the host" << std::endl;
        else
        if (sparse_on_device && verbose)
            std::cerr << "[kmdb] new2all: sparse batch of " << batch.size() << " queries: " << tot.cells << " cells, " << tot.nnz_device << " left the device, "
                      << tot.nnz << " kept, compaction " << tot.compact_ms << " ms, " << tot.d2h_bytes << " bytes to the host" << std::endl;
        std::vector<uint32_t> cols, vals;
        for (size_t q = 0; q < batch.size(); ++q) {
            if (row.size() < 10000 + n * 100 + batch[q].name.size()) row.resize(10000 + n * 100 + batch[q].name.size());
            size_t len;
            if (sparse_on_device) {
                // the library decided every cell with kmdbh_metric; the front-end's own filter sees the same cells and agrees bit for bit
                const kmdb_sparse_rows& r = sp[where[q].first].r;
                cols.clear(); vals.clear();
                for (uint64_t e = r.row_ptr[where[q].second]; e < r.row_ptr[where[q].second + 1]; ++e)
                    if (c.filters.pass(r.val[e], (uint32_t)cnts[q], sample_counts[r.col[e]], (int)k)) { cols.push_back(r.col[e]); vals.push_back(r.val[e]); }
                if (c.sampler.on() && !sampled_on_device) {
                    // the host's sampler on the filtered row: the query's row alone collects (a = the query's count, b = the sample's)
                    c.sampler.init(1);
                    for (size_t e = 0; e < cols.size(); ++e) c.sampler.add(0, cols[e], vals[e], c.sampler.score(vals[e], (uint32_t)cnts[q], sample_counts[cols[e]], (int)k));
                    c.sampler.finish_row(0, cols, vals);
                }
                len = kmdbh_format_sparse_row(batch[q].name.c_str(), cnts[q], cols.data(), vals.data(), cols.size(), row.data());
            } else if (c.sparse) {
                const uint32_t* r = out.data() + q * n;
                cols.clear(); vals.clear();
                for (uint64_t j = 0; j < n; ++j)           // one2all_sp keeps count>0 (:1040-1047), then the filter (:131-148)
                    if (r[j] && c.filters.pass(r[j], (uint32_t)cnts[q], (uint32_t)kmdbh_db_sample_kmers(db.h, j), (int)k)) {
                        cols.push_back((uint32_t)j); vals.push_back(r[j]);
                    }
                len = kmdbh_format_sparse_row(batch[q].name.c_str(), cnts[q], cols.data(), vals.data(), cols.size(), row.data());
            } else {
                len = kmdbh_format_dense_row(batch[q].name.c_str(), cnts[q], out.data() + q * n, n, row.data());
            }
            ofs.write(row.data(), (std::streamsize)len);
        }
        batch.clear();
    };

    new2all_queries(entries, QuerySource{from_minhash, multi, host_extract, k, alphabet, fraction, fstart, nthreads, c.device}, batch, flush);
    if (db.node) node_report(db);                                  // (the last batch's call)
    std::cerr << std::endl << std::endl << "EXECUTION TIMES" << std::endl << "Total: " << since(total0) << std::endl;
    return 0;
}

// ---- one2all (console_one2all.cpp:12-96): one sample against the database --------------------------
// Same engine call as new2all with a batch of one; the row is labelled with the path as given on the
// command line and the file does not end with a newline (console_one2all.cpp:88-93).
int run_one2all(std::vector<std::string>& args, Common& c) {
    if (take_switch(args, "-from-kmers")) throw std::runtime_error(KMC_REFUSAL);
    // (the table one2all writes has no final newline, and the distance loop then drops a one-digit last cell: not reproduced here)
    if (!take_distance_measures(args).empty()) throw std::runtime_error("one2all does not take -distance: run one2all and distance");
    const bool from_minhash = take_switch(args, "-from-minhash");      // the sample argument names <sample>.minhash (console_one2all.cpp:55-58)
    if (from_minhash && take_switch(args, "-multisample-fasta")) throw usage_error("one2all");
    if (args.size() != 3) throw usage_error("one2all");
    std::cerr << "One new sample  (from " << (from_minhash ? "minhashed k-mers" : "genomes") << ") versus entire database comparison" << std::endl;
    Db db;
    std::cerr << "Loading k-mer database " << args[0] << ":" << std::endl;
    auto t0 = clk::now();
    kmdb_opts o{}; o.abi_version = KMDB_ABI_VERSION; o.device = c.device; o.shard_count = 1;
    // -gpus N: N query shards over the node's devices (console_one2all.cpp made multi-GPU: kmdb_node_new2all_*)
    if (c.gpus > 0) { c.partition = KMDB_PARTITION_PREFIX_TABLES; node_upload(db, args[0], c); }
    else {
        check(kmdbh_db_load(args[0].c_str(), 0, &db.h));
        check(kmdb_db_upload(kmdbh_db_view(db.h), &o, 1, &db.d));
    }
    std::cerr << "OK (" << since(t0) << " seconds)" << std::endl;
    const uint64_t n = kmdbh_db_n_samples(db.h);
    const uint32_t k = kmdbh_db_kmer_length(db.h);
    const int32_t alphabet = kmdbh_db_alphabet(db.h);
    if (alphabet < 0 || alphabet >= KMDB_ALPHABET_COUNT) throw std::runtime_error("Invalid alphabet type");
    std::string data;
    std::vector<uint64_t> stored;
    uint32_t stored_k = 0;
    if (from_minhash) {
        if (!load_minhash(args[1], stored, stored_k)) throw std::runtime_error("Cannot open sample file: " + args[1]);
        if (stored_k != k) throw std::runtime_error("Sample and database k-mer length differ");      // console_one2all.cpp:67-69
    } else if (!slurp(args[1], data)) throw std::runtime_error("Cannot open sample file: " + args[1]);
    std::vector<Record> recs;
    split_fasta(data, recs);
    // loader (kmer_extract.h, filter.h), KmerHelper::sortAndUnique (console_one2all.cpp:64-66) and one2all on the device; a genome beyond
    // the call's own loader (32-bit positions) is extracted by the stand-alone extractor first, on the device too, and enters as a k-mer list
    size_t bases = 0;
    for (auto& r : recs) bases += r.seq.size() + 1;
    uint64_t cnt = 0;
    std::vector<uint32_t> sims(n + 1);
    std::cerr << "Calculating similarity vector..." << std::endl;
    if (from_minhash) {
        // the words as stored: already sorted and unique (console_minhash.cpp:40), the total is the stored count
        const uint64_t* kp = stored.data();
        size_t kc = stored.size();
        if (db.node) check(kmdb_node_new2all_batch(db.node, &kp, &kc, 1, sims.data(), nullptr));
        else check(kmdb_new2all_batch(db.d, &kp, &kc, 1, sims.data(), &o));
        cnt = kc;
    } else if (bases < long_query_bases()) {
        std::string text;
        text.reserve(bases);
        for (auto& r : recs) { text += r.seq; text += '\n'; }
        const char* tp = text.data();
        size_t tl = text.size();
        if (db.node) check(kmdb_node_new2all_batch_seq_alphabet(db.node, &tp, &tl, 1, kmdbh_db_fraction(db.h), kmdbh_db_start_fraction(db.h), alphabet, sims.data(), &cnt, nullptr));
        else check(kmdb_new2all_batch_seq_alphabet(db.d, &tp, &tl, 1, kmdbh_db_fraction(db.h), kmdbh_db_start_fraction(db.h), alphabet, sims.data(), &cnt, &o));
    } else {
        std::string text;
        text.reserve(bases);
        for (auto& r : recs) { text += r.seq; text += '\n'; }
        std::vector<uint64_t> kmers;
        extract_long_query(text, k, alphabet, kmdbh_db_fraction(db.h), kmdbh_db_start_fraction(db.h), c.device, kmers);
        size_t kc = kmers.size();
        const uint64_t* kp = kmers.data();
        if (db.node) check(kmdb_node_new2all_batch(db.node, &kp, &kc, 1, sims.data(), nullptr));
        else check(kmdb_new2all_batch(db.d, &kp, &kc, 1, sims.data(), &o));
        cnt = kc;
    }
    if (db.node) node_report(db);
    std::cerr << "Number of k-mers: " << cnt << std::endl;
    std::ofstream ofs(args[2]);
    write_header(db, ofs);
    std::vector<char> row(10000 + n * 100 + args[1].size());
    size_t len = kmdbh_format_dense_row(args[1].c_str(), cnt, sims.data(), n, row.data());
    if (len && row[len - 1] == '\n') --len;
    ofs.write(row.data(), (std::streamsize)len);
    std::cerr << "OK" << std::endl;
    return 0;
}

// ---- distance (console_distance.cpp:7-213, params.cpp:603-668) ----------------------------------------
// Text in, text out: the table of common k-mer counts that all2all / all2all-sp / new2all wrote -> one similarity / distance
// measure per cell.  Same row semantics as the reference: a dense triangle (first row named like the first sample, no counts
// in it) keeps i values in row i, any other dense table whole rows; sparse input or -sparse give "column:value" pairs of the
// non-zero counts that pass the filters; a bound without a criterion filters the chosen measure.
// Two paths write the same bytes.  The host loop below takes one line at a time.  The device path (distance_on_device, kmdb_distance_*)
// parses, measures and formats whole pieces of the table in HBM; the header lines, the names, the counts, the bounds and the triangle test
// stay here.  KMDB_DISTANCE_DEVICE=1 forces the device path (no usable device: an error), KMDB_DISTANCE_DEVICE=0 or -host the host loop.
// Otherwise the host loop runs, unless KMDB_DISTANCE_MIN_BYTES is set: then the device path takes a table of at least that many bytes when a
// device is usable (the threshold has not been measured, so none is built in; no usable device: the host loop, silently).  A table the device
// path declines (kmdb_amd.h) is announced on stderr and written by the host loop from the start, the output file reopened.

// a measure in the reference's fixed notation (conversion.h:167-219, 262-268): exactly 0 is "0", everything else has six
// decimals, rounded half up on the magnitude
size_t put_measure(double v, char* out) {
    if (v == 0) { *out = '0'; return 1; }
    char* p = out;
    if (v < 0) { *p++ = '-'; v = -v; }
    const unsigned long long x = (unsigned long long)(v * 1000000.0 + 0.5);
    p += std::snprintf(p, 40, "%llu.%06llu", x / 1000000ull, x % 1000000ull);
    return (size_t)(p - out);
}
size_t put_uint(unsigned long long v, char* out) { return (size_t)std::snprintf(out, 24, "%llu", v); }

// ---- distance on the device (kmdb_distance_*) -----------------------------------------------------------------------------------------------
// The body of the table goes through the device in pieces of whole lines (KMDB_DISTANCE_BYTES_PER_PIECE, default 256 MiB: a size chosen for
// memory, not tuned; a longer line goes alone): a reader thread fills piece n + 1 and a writer thread writes piece n - 1 while piece n is
// on the device.  What the host loop decides from the rows it has seen is decided here from the first piece: the triangle from row 0, sparse
// input from the first row that has cells.  Rows in front of that row hold no cells and are written as the host loop writes them — as DENSE
// rows when -sparse was not given (the loop turns to sparse output only at the first pair it meets), through a handle of their own.
template <class T>
class Channel {                                  // a bounded queue between two threads; close() from either side ends both
public:
    bool push(T&& v) {
        std::unique_lock<std::mutex> l(m_);
        cv_.wait(l, [&] { return closed_ || q_.size() < 2; });
        if (closed_) return false;
        q_.push_back(std::move(v));
        cv_.notify_all();
        return true;
    }
    bool pop(T& v) {
        std::unique_lock<std::mutex> l(m_);
        cv_.wait(l, [&] { return done_ || closed_ || !q_.empty(); });
        if (closed_ || q_.empty()) return false;
        v = std::move(q_.front());
        q_.erase(q_.begin());
        cv_.notify_all();
        return true;
    }
    void finish() { std::lock_guard<std::mutex> l(m_); done_ = true; cv_.notify_all(); }      // the producer has no more
    void close() { std::lock_guard<std::mutex> l(m_); closed_ = true; cv_.notify_all(); }      // give up: nobody waits any longer
    template <class F> void drain(F&& f) { std::lock_guard<std::mutex> l(m_); for (auto& v : q_) f(v); q_.clear(); }   // what nobody took
private:
    std::mutex m_;
    std::condition_variable cv_;
    std::vector<T> q_;
    bool done_ = false, closed_ = false;
};

struct DistanceSetup {
    int device = 0, measure = 0;
    uint32_t k = 0;
    std::vector<uint32_t> counts;
    std::vector<kmdb_cell_filter> filters;
    bool sparse_out = false, phylip = false;
    std::string first_name;                      // of the header's sample names; empty: none
    bool has_names = false;
};

struct DistanceHandle {
    kmdb_distance* d = nullptr;
    ~DistanceHandle() { if (d) kmdb_distance_free(d); }
    void begin(const DistanceSetup& s, uint32_t flags) {
        kmdb_distance_opts o{};
        o.abi_version = KMDB_ABI_VERSION; o.device = s.device; o.measure = s.measure; o.kmer_length = s.k;
        o.counts = s.counts.data(); o.n = s.counts.size(); o.filters = s.filters.data(); o.n_filters = s.filters.size(); o.flags = flags;
        check(kmdb_distance_begin(&o, &d));
    }
};

// ---- what the three -distance forms (all2all, new2all, all2all-parts) share ------------------------------------------------------------------
// the pieces' budget of cells: KMDB_DISTANCE_CELLS_PER_PIECE, default 2^25 (chosen for memory — 17 B of working arrays a cell and the text —,
// not tuned), at least 1 and below the 2^31 cells the library takes in one call
uint64_t distance_cell_budget() {
    uint64_t budget = 1ull << 25;
    if (const char* e = std::getenv("KMDB_DISTANCE_CELLS_PER_PIECE")) budget = std::max<unsigned long long>(1, std::strtoull(e, nullptr, 10));
    return std::min<uint64_t>(budget, (1ull << 31) - 1);
}

// the header of a measure's table as run_distance writes it for a table without ",db-samples" and total-kmers line
template <class Names>
void write_distance_header(std::ostream& os, bool phylip, uint32_t k, double fraction, const Names& names, uint64_t n) {
    if (!phylip) {
        os << "kmer-length: " << k << " fraction: " << fraction << " ,";
        for (uint64_t i = 0; i < n; ++i) os << names[i] << ',';
        os << std::endl;
    } else os << n << std::endl;
}

// One output file and the thread that writes it: piece n - 1 goes to the file while piece n is on the device.  A text pushed belongs to the
// writer; stop() ends the thread (ok: everything pushed is written first; otherwise at once) and frees what nobody wrote.
struct Text { kmdb_distance_out o{}; };
struct TableWriter {
    std::ofstream ofs;
    Channel<Text> texts;
    std::thread thread;
    bool write_failed = false;
    ~TableWriter() { stop(false); }
    std::ofstream& open(const std::string& path) {              // (the caller writes the header lines before start())
        ofs.open(path, std::ios::binary);
        return ofs;
    }
    void start() {
        thread = std::thread([this]() {
            Text t;
            while (texts.pop(t)) {
                if (t.o.len) ofs.write(t.o.text, (std::streamsize)t.o.len);
                kmdb_distance_out_free(&t.o);
                if (!ofs) { write_failed = true; texts.close(); break; }
            }
        });
    }
    bool push(kmdb_distance_out& o) {                           // false: the writer has given up
        Text t;
        t.o = o;
        o = kmdb_distance_out{};
        if (texts.push(std::move(t))) return true;
        kmdb_distance_out_free(&t.o);
        return false;
    }
    void stop(bool ok) {
        if (ok) texts.finish(); else texts.close();
        if (thread.joinable()) thread.join();
        texts.drain([](Text& t) { kmdb_distance_out_free(&t.o); });
    }
};

// the KMDB_VERBOSE line of a handle's statistics; from_text: the fields of the text source too
void report_distance_stats(const char* lead_in, const kmdb_distance* d, bool from_text) {
    kmdb_distance_stats st{};
    if (!std::getenv("KMDB_VERBOSE") || !d || kmdb_distance_stats_get(d, &st)) return;
    std::cerr << "[kmdb] " << lead_in << ": calls " << st.calls << ", rows " << st.rows << ", cells read " << st.cells_read << ", cells written " << st.cells_written
              << ", host cells " << st.host_cells;
    if (from_text) std::cerr << ", bytes in " << st.bytes_in;
    std::cerr << ", bytes out " << st.bytes_out;
    if (from_text) std::cerr << ", parse " << st.parse_ms << " ms";
    std::cerr << ", measure " << st.measure_ms << " ms, format " << st.format_ms << " ms, copies " << st.copy_ms << " ms" << std::endl;
}

// true: the output is written; false: the device path declined (why), the caller starts over with the host loop
bool distance_on_device(const std::string& path, long long body, std::ostream& out, const DistanceSetup& s, std::string& why) {
    size_t piece_bytes = 256ull << 20;
    if (const char* e = std::getenv("KMDB_DISTANCE_BYTES_PER_PIECE")) piece_bytes = std::max<unsigned long long>(1, std::strtoull(e, nullptr, 10));
    piece_bytes = std::min<size_t>(piece_bytes, 3ull << 30);
    struct Piece { std::string text; bool last = false; };
    Channel<Piece> pieces;
    Channel<Text> texts;
    std::string read_error;
    std::thread reader([&]() {
        FILE* f = std::fopen(path.c_str(), "rb");
        if (!f || fseeko(f, (off_t)body, SEEK_SET)) { read_error = "Cannot open common k-mers table: " + path; if (f) std::fclose(f); pieces.close(); return; }
        std::string buf;
        size_t pos = 0;                                            // buf[pos ..): read and not yet handed on
        bool eof = false;
        for (bool last = false; !last;) {
            size_t cut = std::string::npos;
            for (;;) {
                const size_t have = buf.size() - pos;
                if (have >= piece_bytes || eof) {                   // the last line end inside the piece; none: the line goes alone, whatever its length
                    const size_t lim = pos + std::min(have, piece_bytes);
                    size_t nl = lim > pos ? buf.rfind('\n', lim - 1) : std::string::npos;
                    if (nl == std::string::npos || nl < pos) nl = buf.find('\n', lim > pos ? lim - 1 : pos);
                    if (nl != std::string::npos) { cut = nl + 1; break; }
                    if (eof) { cut = buf.size(); break; }
                }
                buf.erase(0, pos);
                pos = 0;
                const size_t old = buf.size(), want = std::max<size_t>(old < piece_bytes ? piece_bytes - old : 0, 1 << 16);
                buf.resize(old + want);
                const size_t got = std::fread(&buf[old], 1, want, f);
                buf.resize(old + got);
                if (got < want) eof = true;
            }
            Piece p;
            p.text.assign(buf, pos, cut - pos);
            pos = cut;
            last = p.last = eof && pos == buf.size();
            if (!pieces.push(std::move(p))) break;
        }
        std::fclose(f);
        pieces.finish();
    });
    bool write_failed = false;
    std::thread writer([&]() {
        Text t;
        while (texts.pop(t)) {
            if (t.o.len) out.write(t.o.text, (std::streamsize)t.o.len);
            kmdb_distance_out_free(&t.o);
            if (!out) { write_failed = true; texts.close(); pieces.close(); break; }
        }
    });
    auto stop = [&]() { pieces.close(); texts.close(); reader.join(); writer.join(); texts.drain([](Text& t) { kmdb_distance_out_free(&t.o); }); };
    DistanceHandle lead, body_handle;
    uint64_t row = 0, lead_rows = 0;
    bool decided = false, declined = false, triangle = false;
    std::string pending;                                           // the rows seen before the first row with cells (they hold none), and that row's piece
    size_t scanned = 0;
    std::string error;
    try {
        Piece p;
        while (pieces.pop(p)) {
            const char* text = p.text.data();
            size_t len = p.text.size();
            if (!decided) {
                // row 0: the triangle; the first row with cells: sparse or dense input
                if (pending.empty()) pending = std::move(p.text); else pending += p.text;
                bool sparse_in = false, found = false;
                size_t at = scanned;
                while (at < pending.size() && !found) {
                    const char* b = pending.data() + at;
                    const char* nl = (const char*)std::memchr(b, '\n', pending.size() - at);
                    const char* end = nl ? nl : pending.data() + pending.size();
                    const char* comma = std::find(b, end, ',');
                    const char* q = comma < end ? comma + 1 : end;
                    while (q < end && *q >= '0' && *q <= '9') ++q;
                    if (q < end) ++q;
                    unsigned long long v = 0;
                    bool pair = false;
                    if (end - q > 1) {
                        found = true;
                        while (q < end && *q >= '0' && *q <= '9') v = v * 10 + (unsigned)(*q++ - '0');
                        pair = q < end && *q == ':';
                        sparse_in = pair;
                    }
                    if (at == 0)
                        triangle = !s.sparse_out && s.has_names && std::string(b, comma) == s.first_name && (s.counts.empty() || pair || (uint32_t)v == 0);
                    if (!found) { ++lead_rows; at = (size_t)(end - pending.data()) + (nl ? 1 : 0); }
                }
                scanned = at;
                if (!found && !p.last) continue;
                decided = true;
                text = pending.data();
                len = pending.size();
                const uint32_t tri = triangle ? KMDB_DISTANCE_TRIANGLE : 0u;
                body_handle.begin(s, tri | (s.sparse_out ? KMDB_DISTANCE_SPARSE_OUT : 0u) | (sparse_in ? KMDB_DISTANCE_SPARSE_IN : 0u) | (s.phylip ? KMDB_DISTANCE_PHYLIP : 0u));
                if (sparse_in && !s.sparse_out && !s.phylip && lead_rows) {
                    lead.begin(s, tri);
                    Text t;
                    const int rc = kmdb_distance_rows(lead.d, text, scanned, 0, &t.o);
                    if (rc == KMDB_DISTANCE_DECLINED) { why = kmdb_last_error(); declined = true; break; }
                    check(rc);
                    if (!texts.push(std::move(t))) { kmdb_distance_out_free(&t.o); break; }
                    row = lead_rows; text += scanned; len -= scanned;
                }
            }
            Text t;
            const int rc = kmdb_distance_rows(body_handle.d, text, len, row, &t.o);
            if (rc == KMDB_DISTANCE_DECLINED) { why = kmdb_last_error(); declined = true; break; }
            check(rc);
            row += t.o.rows;
            if (!texts.push(std::move(t))) { kmdb_distance_out_free(&t.o); break; }
        }
    } catch (std::exception& e) {
        error = e.what();
    }
    if (declined || !error.empty()) { stop(); if (!error.empty()) throw std::runtime_error(error); return false; }
    texts.finish();
    reader.join();
    writer.join();
    if (!read_error.empty()) throw std::runtime_error(read_error);
    if (write_failed) throw std::runtime_error("Cannot write the output table");
    for (const DistanceHandle* h : {&lead, &body_handle}) report_distance_stats("distance on the device", h->d, true);
    return true;
}


// the -min / -max list as the distance mode reads it (params.cpp:603-668): a bare bound ("?") belongs to the chosen measure, num-kmers: is the count
struct DistanceBound { metric_fn fn; double lo = std::numeric_limits<double>::lowest(), hi = std::numeric_limits<double>::max(); };
void take_distance_bounds(std::vector<std::string>& args, std::map<std::string, metric_fn>& avail, std::map<std::string, DistanceBound>& bounds, long& kmer_lo, long& kmer_hi) {
    const char* names[2] = {"-min", "-max"};
    for (int which = 0; which < 2; ++which) {
        std::string v;
        while (take_option(args, names[which], v)) {
            std::string crit = "?", num = v;
            const auto sep = v.rfind(':');
            if (sep != std::string::npos) { crit = v.substr(0, sep); num = v.substr(sep + 1); }
            std::istringstream iss(num);
            double value;
            if (!(iss >> value)) throw std::runtime_error("Filtering error - unable to parse numerical value: " + v);
            if (crit == "num-kmers") (which == 0 ? kmer_lo : kmer_hi) = std::lrint(value);
            else if (crit == "?" || avail.count(crit)) (which == 0 ? bounds[crit].lo : bounds[crit].hi) = value;
            else throw std::runtime_error("Filtering error - unknown metric: " + crit);
        }
    }
}
// a bare bound belongs to the measure of the run
void own_bare_bound(std::map<std::string, DistanceBound>& bounds, const std::string& measure) {
    if (!bounds.count("?")) return;
    const DistanceBound b = bounds["?"];
    bounds.erase("?");
    bounds[measure] = b;
}
// the bounds of one run as the library takes them
std::vector<kmdb_cell_filter> distance_filters(const std::map<std::string, DistanceBound>& bounds, long kmer_lo, long kmer_hi) {
    std::vector<kmdb_cell_filter> fl;
    for (auto& kv : bounds) fl.push_back(kmdb_cell_filter{kmdbh_metric_id(kv.first.c_str()), 0, kv.second.lo, kv.second.hi});
    if (kmer_lo != 0 || kmer_hi != (long)std::numeric_limits<uint32_t>::max())
        fl.push_back(kmdb_cell_filter{KMDB_METRIC_NUM_KMERS, 0, (double)kmer_lo, (double)kmer_hi});
    return fl;
}
// ... of the run of one measure out of several over the same -min / -max list
std::vector<kmdb_cell_filter> distance_filters(std::map<std::string, DistanceBound> bounds, const std::string& measure, long kmer_lo, long kmer_hi) {
    own_bare_bound(bounds, measure);
    return distance_filters(bounds, kmer_lo, kmer_hi);
}

// ---- all2all -distance <measure>: the measure's table straight from the matrix in HBM ---------------------------------------------------------
// `all2all D T` followed by `distance O <measure> T out`, byte for byte, without T: the library computes the triangle into memory the first
// measure's handle owns (kmdb_distance_take_all2all), every further measure borrows it, and the rows come back as text in pieces cut by a
// budget of cells (KMDB_DISTANCE_CELLS_PER_PIECE, default 2^25: chosen for memory — 17 B of working arrays a cell and the text —, not tuned).
// The writer thread writes piece n - 1 while piece n is on the device.  The header lines come from the host, as run_distance writes them
// for a triangle table: no ",db-samples", no total-kmers line.  The -min / -max list is read by the DISTANCE mode's rule.
int run_all2all_distance(std::vector<std::string>& args, Common& c, const std::vector<std::string>& measures, bool sparse_forced, const char* mode) {
    auto avail = metrics();
    for (auto& m : measures)
        if (!avail.count(m)) throw std::runtime_error("unknown measure: " + m);
    if (c.gpus > 0) throw std::runtime_error(std::string("-distance does not go with -gpus <N>: the node's shards keep their triangle to themselves (run ") + mode + " and distance)");
    for (auto& a : args)
        if (a == "-sample-rows") throw std::runtime_error("-distance does not go with -sample-rows: sampled rows are no rows of the triangle");
    bool sparse = take_switch(args, "-sparse") || sparse_forced;
    const bool phylip = take_switch(args, "-phylip-out");
    if (phylip) sparse = false;
    std::map<std::string, DistanceBound> bounds;
    long kmer_lo = 0, kmer_hi = std::numeric_limits<uint32_t>::max();
    take_distance_bounds(args, avail, bounds, kmer_lo, kmer_hi);
    if (args.size() != 2) throw usage_error(mode);
    const uint64_t budget = distance_cell_budget();

    std::cerr << "All versus all comparison, " << (measures.size() == 1 ? "measure " + measures[0] : std::to_string(measures.size()) + " measures") << std::endl;
    Db db;
    kmdb_opts o{}; o.abi_version = KMDB_ABI_VERSION; o.device = c.device; o.shard_count = 1; o.flags = KMDB_FLAG_ONE_SHOT;
    open_database(db, args[0], c, o);
    const uint64_t n = kmdbh_db_n_samples(db.h);
    // -rows: the band is computed once into memory this run holds, every measure's handle borrows it from its first row on and only its rows are asked for
    uint64_t r_lo = 0, r_hi = n;
    if (c.rows.on) c.rows.resolve(n, c.seed_samples, r_lo, r_hi);
    std::unique_ptr<DeviceBand> band;
    DistanceSetup s;
    s.device = c.device; s.k = kmdbh_db_kmer_length(db.h); s.sparse_out = sparse; s.phylip = phylip;
    s.counts.resize(n);
    std::vector<const char*> names(std::max<uint64_t>(n, 1), "");
    for (uint64_t i = 0; i < n; ++i) { s.counts[i] = (uint32_t)kmdbh_db_sample_kmers(db.h, i); names[i] = kmdbh_db_sample_name(db.h, i); }
    const uint32_t flags = KMDB_DISTANCE_TRIANGLE | (sparse ? KMDB_DISTANCE_SPARSE_OUT : 0u) | (phylip ? KMDB_DISTANCE_PHYLIP : 0u);

    // -band-rows <R>: every measure's table is open at once; a band is computed once, every measure's handle borrows it in turn and its rows go to
    // that measure's writer — one band buffer for the whole run
    if (c.band_rows) {
        const uint64_t R = c.band_rows;
        const size_t nm = measures.size();
        if (!nm) throw usage_error(mode);
        std::vector<DistanceSetup> setups(nm, s);
        std::vector<DistanceHandle> hs(nm);
        std::vector<std::unique_ptr<TableWriter>> ws(nm);
        std::vector<std::string> paths(nm);
        for (size_t mi = 0; mi < nm; ++mi) {
            setups[mi].measure = kmdbh_metric_id(measures[mi].c_str());
            setups[mi].filters = distance_filters(bounds, measures[mi], kmer_lo, kmer_hi);
            hs[mi].begin(setups[mi], flags);
            paths[mi] = nm == 1 ? args[1] : args[1] + "." + measures[mi];
            ws[mi].reset(new TableWriter);
            write_distance_header(ws[mi]->open(paths[mi]), phylip, s.k, kmdbh_db_fraction(db.h), names, n);
            ws[mi]->start();
        }
        std::cerr << "Calculating rows " << r_lo << " to " << r_hi << " of the matrix of common k-mers in bands of " << R << " rows, storing "
                  << (nm == 1 ? "the " + measures[0] + " table" : std::to_string(nm) + " tables") << " in " << args[1] << (nm == 1 ? "" : ".<measure>") << "...";
        const auto t0 = clk::now();
        band.reset(new DeviceBand(c.device, largest_band_cells(r_lo, r_hi, R)));
        std::string error;
        try {
            for (uint64_t b_lo = r_lo; b_lo < r_hi;) {
                const uint64_t b_hi = b_lo + std::min(R, r_hi - b_lo);
                c.band_to_device(db.d, b_lo, b_hi, band->p, o);
                if (b_lo == r_lo) db.uploaded();
                for (size_t mi = 0; mi < nm; ++mi) {
                    check(kmdb_distance_take_cells_device(hs[mi].d, band->p, b_lo, names.data()));
                    for (uint64_t i0 = b_lo; i0 < b_hi;) {
                        const uint64_t i1 = next_stripe(i0, b_hi, budget);
                        kmdb_distance_out piece{};
                        check(kmdb_distance_matrix_rows(hs[mi].d, i0, i1, &piece));
                        if (!ws[mi]->push(piece)) throw std::runtime_error("Cannot write the output file " + paths[mi]);
                        i0 = i1;
                    }
                }
                b_lo = b_hi;
            }
        } catch (std::exception& e) {
            error = e.what();
        }
        for (auto& w : ws) w->stop(error.empty());
        if (!error.empty()) throw std::runtime_error(error);
        for (size_t mi = 0; mi < nm; ++mi)
            if (ws[mi]->write_failed) throw std::runtime_error("Cannot write the output file " + paths[mi]);
        std::cerr << "OK (" << since(t0) << " seconds)" << std::endl;
        for (size_t mi = 0; mi < nm; ++mi) report_distance_stats("distance from the matrix", hs[mi].d, false);
        for (size_t mi = 0; mi + 1 < nm; ++mi) {
            ws[mi]->ofs.close();
            if (!ws[mi]->ofs) throw std::runtime_error("Cannot write the output file " + paths[mi]);
        }
        return finish(db, ws[nm - 1]->ofs, paths[nm - 1]);
    }

    DistanceHandle owner;                                          // the first measure's handle holds the triangle for all of them
    std::unique_ptr<TableWriter> w;                                // one per measure in turn
    std::string path;
    for (size_t mi = 0; mi < measures.size(); ++mi) {
        const std::string& measure = measures[mi];
        s.measure = kmdbh_metric_id(measure.c_str());
        s.filters = distance_filters(bounds, measure, kmer_lo, kmer_hi);
        DistanceHandle borrower;
        DistanceHandle& h = mi == 0 ? owner : borrower;
        h.begin(s, flags);
        if (c.rows.on) {
            if (!band) {
                std::cerr << "Calculating rows " << r_lo << " to " << r_hi << " of the matrix of common k-mers..." << std::endl;
                const auto t0 = clk::now();
                band.reset(new DeviceBand(c.device, tri(r_hi) - tri(r_lo)));
                c.band_to_device(db.d, r_lo, r_hi, band->p, o);
                std::cerr << "OK (" << since(t0) << " seconds)" << std::endl;
                db.uploaded();
            }
            check(kmdb_distance_take_cells_device(h.d, band->p, r_lo, names.data()));
        } else if (mi == 0) {
            std::cerr << "Calculating matrix of common k-mers..." << std::endl;
            const auto t0 = clk::now();
            check(kmdb_distance_take_all2all(h.d, db.d, names.data(), &o));
            kmdb_stats st{};
            if (!kmdb_db_stats(db.d, &st) && st.path == KMDB_PATH_GLOBAL)
                std::cerr << "WARNING: the fast pipeline could not take this database (" << kmdb_db_fallback_reason(db.d) << "); the slow HBM-atomics kernel ran" << std::endl;
            std::cerr << "OK (" << since(t0) << " seconds)" << std::endl;
            db.uploaded();
        } else check(kmdb_distance_take_cells_device(h.d, kmdb_distance_cells_device(owner.d), 0, names.data()));

        path = measures.size() == 1 ? args[1] : args[1] + "." + measure;
        std::cerr << "Storing the " << measure << " table in " << path << "...";
        const auto t0 = clk::now();
        w.reset(new TableWriter);
        write_distance_header(w->open(path), phylip, s.k, kmdbh_db_fraction(db.h), names, n);
        w->start();
        std::string error;
        try {
            for (uint64_t i0 = r_lo; i0 < r_hi;) {
                const uint64_t i1 = next_stripe(i0, r_hi, budget);
                kmdb_distance_out piece{};
                check(kmdb_distance_matrix_rows(h.d, i0, i1, &piece));
                if (!w->push(piece)) break;
                i0 = i1;
            }
        } catch (std::exception& e) {
            error = e.what();
        }
        w->stop(error.empty());
        if (!error.empty()) throw std::runtime_error(error);
        if (w->write_failed) throw std::runtime_error("Cannot write the output file " + path);
        std::cerr << "OK (" << since(t0) << " seconds)" << std::endl;
        report_distance_stats("distance from the matrix", h.d, false);
        if (mi + 1 < measures.size()) {
            w->ofs.close();
            if (!w->ofs) throw std::runtime_error("Cannot write the output file " + path);
        }
    }
    if (!w) throw usage_error(mode);                               // (no measure: the callers give one at least)
    return finish(db, w->ofs, path);
}

// ---- new2all -distance <measure>: the measure's table straight from the query rows in HBM ------------------------------------------------------
// `new2all D Q T` followed by `distance -host <measure> T out`, byte for byte, without T (T the DENSE table of counts, whatever -sparse says
// about the output).  The queries are read, extracted and batched as in new2all.  Per batch the rows are computed once, into a rectangle the
// first measure's handle owns (kmdb_distance_take_new2all_batch*: the k-mer half and the text half of a batch are two takes); every further
// measure borrows them (kmdb_distance_take_rows_device).  The rows come back as text in pieces cut at row ends by a budget of cells
// (KMDB_DISTANCE_CELLS_PER_PIECE, as for the matrix) and are written in input order by a writer thread per measure, while the device has the
// next batch.  The header lines are the ones run_distance writes for such a table: no ",db-samples", no total-kmers line.  The -min / -max
// list is read by the DISTANCE mode's rule.
// The triangle rule (run_distance: row 0 named like the first sample with a first cell of 0 makes row i keep min(i, N) values) would cut the
// rows of such a table; it is decided here from query 0 of the first batch before any output file exists, and where it would fire the run is
// refused.  In the sparse form the rule changes no byte, so nothing is decided.
int run_new2all_distance(std::vector<std::string>& args, Common& c, const std::vector<std::string>& measures) {
    auto avail = metrics();
    for (auto& m : measures)
        if (!avail.count(m)) throw std::runtime_error("unknown measure: " + m);
    if (c.gpus > 0) throw std::runtime_error("-distance does not go with -gpus <N>: the node's query rows live in the chunks of a reduce-scatter (run new2all and distance)");
    const bool from_minhash = take_switch(args, "-from-minhash");
    const bool multi = take_switch(args, "-multisample-fasta");
    if (multi && from_minhash) throw usage_error("new2all");
    const bool host_extract = take_switch(args, "-host-extract");
    bool sparse = take_switch(args, "-sparse");
    const bool phylip = take_switch(args, "-phylip-out");
    if (phylip) sparse = false;
    std::map<std::string, DistanceBound> bounds;
    long kmer_lo = 0, kmer_hi = std::numeric_limits<uint32_t>::max();
    take_distance_bounds(args, avail, bounds, kmer_lo, kmer_hi);
    if (args.size() != 3) throw usage_error("new2all");
    const uint64_t budget = distance_cell_budget();

    std::cerr << "Set of new samples  (from " << (from_minhash ? "minhashed k-mers" : "genomes") << ") versus entire database comparison, "
              << (measures.size() == 1 ? "measure " + measures[0] : std::to_string(measures.size()) + " measures") << std::endl;
    Db db;
    std::cerr << "Loading k-mer database " << args[0] << "..." << std::endl;
    auto t0 = clk::now();
    kmdb_opts o{}; o.abi_version = KMDB_ABI_VERSION; o.device = c.device; o.shard_count = 1;
    check(kmdbh_db_load(args[0].c_str(), 0, &db.h));
    check(kmdb_db_upload(kmdbh_db_view(db.h), &o, 1, &db.d));
    std::cerr << "OK (" << since(t0) << " seconds)" << std::endl;
    const uint64_t n = kmdbh_db_n_samples(db.h);
    const uint32_t k = kmdbh_db_kmer_length(db.h);
    const double fraction = kmdbh_db_fraction(db.h), fstart = kmdbh_db_start_fraction(db.h);
    const int32_t alphabet = kmdbh_db_alphabet(db.h);
    if (alphabet < 0 || alphabet >= KMDB_ALPHABET_COUNT) throw std::runtime_error("Invalid alphabet type");

    std::ifstream lst(args[1]);
    if (!lst) throw std::runtime_error("Unable to open sample list " + args[1]);
    std::vector<std::string> entries;
    for (std::string ln; std::getline(lst, ln);) {
        while (!ln.empty() && (ln.back() == '\r' || ln.back() == ' ')) ln.pop_back();
        if (!ln.empty()) entries.push_back(ln);
    }
    const int nthreads = c.threads > 0 ? c.threads : (int)std::max(1u, std::thread::hardware_concurrency());

    DistanceSetup s;
    s.device = c.device; s.k = k; s.sparse_out = sparse; s.phylip = phylip;
    s.counts.resize(n);
    std::vector<std::string> sample_names(n);
    for (uint64_t i = 0; i < n; ++i) { s.counts[i] = (uint32_t)kmdbh_db_sample_kmers(db.h, i); sample_names[i] = kmdbh_db_sample_name(db.h, i); }
    const uint32_t flags = (sparse ? KMDB_DISTANCE_SPARSE_OUT : 0u) | (phylip ? KMDB_DISTANCE_PHYLIP : 0u);

    // one handle, one output file and one writer thread per measure; handle 0 owns the rows of the batch
    struct Table {
        std::string measure, path;
        DistanceHandle h;
        TableWriter w;
    };
    std::vector<std::unique_ptr<Table>> tables;
    for (auto& measure : measures) {
        s.measure = kmdbh_metric_id(measure.c_str());
        s.filters = distance_filters(bounds, measure, kmer_lo, kmer_hi);
        tables.emplace_back(new Table);
        Table& t = *tables.back();
        t.measure = measure;
        t.path = measures.size() == 1 ? args[2] : args[2] + "." + measure;
        t.h.begin(s, flags);
    }
    bool opened = false;
    auto open_tables = [&]() {
        if (opened) return;
        opened = true;
        for (auto& tp : tables) {
            write_distance_header(tp->w.open(tp->path), phylip, k, fraction, sample_names, n);
            tp->w.start();
        }
    };
    auto stop_tables = [&](bool ok) {
        for (auto& tp : tables) tp->w.stop(ok);
    };

    // the first cell of the first row taken, through a probe of its own: num-kmers is the count itself, and only a count of 0 is written "0"
    auto first_cell_is_zero = [&](const uint32_t* a, const char* const* names) {
        if (n == 0) return true;
        DistanceSetup ps = s;
        ps.measure = KMDB_METRIC_NUM_KMERS; ps.filters.clear();
        DistanceHandle probe;
        probe.begin(ps, 0);
        check(kmdb_distance_take_rows_device(probe.d, kmdb_distance_cells_device(tables[0]->h.d), 1, a, names));
        Text x;
        check(kmdb_distance_query_rows(probe.d, 0, 1, &x.o));
        const size_t at = std::strlen(names[0]) + 1;
        const bool zero = x.o.len > at + 1 && x.o.text[at] == '0' && x.o.text[at + 1] == ',';
        kmdb_distance_out_free(&x.o);
        return zero;
    };

    std::cerr << "Processing queries..." << std::endl;
    auto total0 = clk::now();
    std::vector<Query> batch;
    bool first_take = true;
    uint64_t n_queries = 0;
    auto flush = [&]() {
        if (batch.empty()) return;
        std::vector<size_t> halves[2];                             // [0] k-mer lists (-host-extract, -from-minhash, long genomes), [1] sequence text
        for (size_t q = 0; q < batch.size(); ++q) halves[batch[q].from_kmers ? 0 : 1].push_back(q);
        // the text of every table, as pieces of consecutive queries keyed by the first one's place in the batch
        std::vector<std::map<size_t, Text>> pieces(tables.size());
        try {
            for (int half = 0; half < 2; ++half) {
                const std::vector<size_t>& idx = halves[half];
                if (idx.empty()) continue;
                const size_t nq = idx.size();
                std::vector<const char*> names(nq);
                std::vector<uint32_t> a(nq);
                for (size_t t = 0; t < nq; ++t) names[t] = batch[idx[t]].name.c_str();
                if (half == 0) {
                    std::vector<const uint64_t*> ptrs(nq);
                    std::vector<size_t> kc(nq);
                    for (size_t t = 0; t < nq; ++t) { ptrs[t] = batch[idx[t]].kmers.data(); kc[t] = batch[idx[t]].kmers.size(); a[t] = (uint32_t)kc[t]; }
                    check(kmdb_distance_take_new2all_batch(tables[0]->h.d, db.d, ptrs.data(), kc.data(), nq, names.data(), &o));
                } else {
                    std::vector<const char*> ptrs(nq);
                    std::vector<size_t> lens(nq);
                    std::vector<uint64_t> uniq(nq);
                    for (size_t t = 0; t < nq; ++t) { ptrs[t] = batch[idx[t]].text.data(); lens[t] = batch[idx[t]].text.size(); }
                    check(kmdb_distance_take_new2all_batch_seq_alphabet(tables[0]->h.d, db.d, ptrs.data(), lens.data(), nq, fraction, fstart, alphabet, names.data(), uniq.data(), &o));
                    for (size_t t = 0; t < nq; ++t) a[t] = (uint32_t)uniq[t];
                }
                // the triangle rule, from query 0 of the run (dense and phylip forms only)
                if (first_take && idx[0] == 0 && !sparse && n > 0 && batch[0].name == sample_names[0] && first_cell_is_zero(a.data(), names.data()))
                    throw std::runtime_error("new2all -distance: the first query, " + batch[0].name + ", is named like the first sample of the database, " + sample_names[0]
                                             + ", and shares no k-mer with it: the distance mode takes such a table for a triangle and cuts its rows; run new2all and distance");
                for (size_t ti = 0; ti < tables.size(); ++ti) {
                    kmdb_distance* h = tables[ti]->h.d;
                    if (ti) check(kmdb_distance_take_rows_device(h, kmdb_distance_cells_device(tables[0]->h.d), nq, a.data(), names.data()));
                    // pieces: rows of the half that follow each other in the batch, within the budget of cells
                    const uint64_t rows_max = std::max<uint64_t>(1, budget / std::max<uint64_t>(n, 1));
                    for (size_t r0 = 0; r0 < nq;) {
                        size_t r1 = r0 + 1;
                        while (r1 < nq && idx[r1] == idx[r1 - 1] + 1 && r1 - r0 < rows_max) ++r1;
                        Text x;
                        check(kmdb_distance_query_rows(h, r0, r1, &x.o));
                        pieces[ti][idx[r0]] = x;
                        r0 = r1;
                    }
                }
            }
        } catch (...) {
            for (auto& m : pieces) for (auto& kv : m) kmdb_distance_out_free(&kv.second.o);
            throw;
        }
        first_take = false;
        open_tables();
        for (size_t ti = 0; ti < tables.size(); ++ti)
            for (auto& kv : pieces[ti]) (void)tables[ti]->w.push(kv.second.o);
        n_queries += batch.size();
        batch.clear();
    };
    try {
        new2all_queries(entries, QuerySource{from_minhash, multi, host_extract, k, alphabet, fraction, fstart, nthreads, c.device}, batch, flush);
        open_tables();                                             // (no query at all: the header lines alone, as the two commands write them)
    } catch (...) {
        stop_tables(false);
        throw;
    }
    stop_tables(true);
    for (auto& tp : tables) {
        tp->w.ofs.close();
        if (tp->w.write_failed || !tp->w.ofs) throw std::runtime_error("Cannot write the output file " + tp->path);
        std::cerr << "Stored the " << tp->measure << " table of " << n_queries << " queries in " << tp->path << std::endl;
        report_distance_stats("distance from the query rows", tp->h.d, false);
    }
    std::cerr << std::endl << std::endl << "EXECUTION TIMES" << std::endl << "Total: " << since(total0) << std::endl;
    return 0;
}

// ---- all2all-parts -distance <measure>: the measure's table straight from the block rows' CSRs in HBM ------------------------------------------
// `all2all-parts L T` followed by `distance -sparse <bounds> <measure> T out`, byte for byte, without T.  Every cell of a block row leaves its CSR
// in HBM (kmdb_distance_parts_add_db2db, kmdb_distance_parts_add_all2all), the first measure's handle gathers them into one CSR there, every
// further measure borrows it (kmdb_distance_csr_device, kmdb_distance_take_csr_device), and the rows come back as text in pieces cut at row ends
// by a budget of cells (KMDB_DISTANCE_CELLS_PER_PIECE, default 2^25, as for the other two -distance forms).  The cells are computed WITHOUT
// bounds — the table T of the pair of commands is written without any — and the -min / -max list is read by the DISTANCE mode's rule.  The header
// is the one run_distance writes for such a table: no ",db-samples", no total-kmers line.  The output is always the sparse form: the rows in
// front of the table's first pair, which the distance loop writes as dense rows when -sparse is not given, are not reproduced.
// -gpus W as in all2all-parts: the block rows dealt to W workers, every worker with its own handles on its device; this thread is the writer: it
// takes the block rows in order and writes a piece while the device has the next one.
int run_all2all_parts_distance(std::vector<std::string>& args, Common& c, const std::vector<std::string>& measures) {
    auto avail = metrics();
    for (auto& m : measures)
        if (!avail.count(m)) throw std::runtime_error("unknown measure: " + m);
    for (auto& a : args) {
        if (a == "-sample-rows") throw std::runtime_error("-distance does not go with -sample-rows: sampled rows are no rows of the grid's table");
        if (a == "-phylip-out") throw std::runtime_error("-distance does not go with -phylip-out under all2all-parts: phylip output from sparse input is declined");
    }
    std::string v;
    take_option(args, "-buffer", v);
    take_option(args, "-bubble-size", v);
    take_switch(args, "-sparse");
    std::map<std::string, DistanceBound> bounds;
    long kmer_lo = 0, kmer_hi = std::numeric_limits<uint32_t>::max();
    take_distance_bounds(args, avail, bounds, kmer_lo, kmer_hi);
    if (args.size() != 2) throw usage_error("all2all-parts");
    const uint64_t budget = distance_cell_budget();

    std::cerr << "All versus all comparison (parts), " << (measures.size() == 1 ? "measure " + measures[0] : std::to_string(measures.size()) + " measures") << std::endl;
    const PartsCollection pc = read_parts_collection(args[0]);
    const size_t n_parts = pc.files.size(), M = measures.size();
    std::vector<uint64_t> row_start(n_parts + 1, 0);
    for (size_t i = 0; i < n_parts; ++i) row_start[i + 1] = row_start[i] + pc.part_n[i];
    const std::vector<uint32_t> counts32(pc.counts.begin(), pc.counts.end());
    std::vector<const char*> name_ptrs(std::max<size_t>(pc.names.size(), 1), "");
    for (size_t i = 0; i < pc.names.size(); ++i) name_ptrs[i] = pc.names[i].c_str();
    std::vector<DistanceSetup> setups(M);
    for (size_t mi = 0; mi < M; ++mi) {
        setups[mi].k = pc.k; setups[mi].sparse_out = true; setups[mi].counts = counts32;
        setups[mi].measure = kmdbh_metric_id(measures[mi].c_str());
        setups[mi].filters = distance_filters(bounds, measures[mi], kmer_lo, kmer_hi);
    }
    std::vector<std::ofstream> ofs(M);
    std::vector<std::string> paths(M);
    for (size_t mi = 0; mi < M; ++mi) {
        paths[mi] = M == 1 ? args[1] : args[1] + "." + measures[mi];
        ofs[mi].open(paths[mi], std::ios::binary);
        write_distance_header(ofs[mi], false, pc.k, pc.fraction, pc.names, pc.names.size());
    }

    const int have = std::max(1, kmdb_device_count());
    const size_t W = c.gpus > 0 ? std::min<size_t>((size_t)c.gpus, n_parts) : 1;
    struct Worker {
        kmdb_opts o{};
        std::vector<std::unique_ptr<Db>> resident;
        std::vector<std::unique_ptr<DistanceHandle>> h;            // one per measure, on the worker's device; [0] gathers, the others borrow
    };
    std::vector<Worker> workers(W);
    for (size_t t = 0; t < W; ++t) {
        workers[t].o.abi_version = KMDB_ABI_VERSION; workers[t].o.shard_count = 1;
        workers[t].o.device = c.device + (int)(t % (size_t)std::max(1, have - c.device));
        workers[t].resident.resize(n_parts);
    }
    if (W > 1) std::cerr << "Block rows of the grid dealt to " << W << " workers on " << std::min<size_t>(W, (size_t)std::max(1, have - c.device)) << " GPU(s)" << std::endl;
    // the text of a block row: per measure the pieces the writer has not taken yet, in order (under mu)
    struct BlockOut {
        std::vector<std::vector<kmdb_distance_out>> pieces;
        bool done = false;
        ~BlockOut() { for (auto& m : pieces) for (auto& o : m) kmdb_distance_out_free(&o); }
    };
    std::vector<BlockOut> block_out(n_parts);
    for (auto& b : block_out) b.pieces.resize(M);
    std::mutex mu;
    std::condition_variable cv;
    std::exception_ptr failure;
    const bool verbose = std::getenv("KMDB_VERBOSE") != nullptr;
    auto block_row = [&](Worker& wk, size_t i) {
        auto get = [&](size_t p, size_t keep) -> Db& {
            if (wk.resident[p]) return *wk.resident[p];
            auto d = std::make_unique<Db>();
            check(kmdbh_db_load(pc.files[p].c_str(), 0, &d->h));
            if (kmdb_db_upload(kmdbh_db_view(d->h), &wk.o, 1, &d->d)) {
                for (size_t j = 0; j < wk.resident.size(); ++j) if (j != keep) wk.resident[j].reset();
                check(kmdb_db_upload(kmdbh_db_view(d->h), &wk.o, 1, &d->d));
            }
            kmdbh_db_free(d->h); d->h = nullptr;                   // the host copy is not needed once the part is in HBM
            wk.resident[p] = std::move(d);
            return *wk.resident[p];
        };
        if (wk.h.empty())
            for (size_t mi = 0; mi < M; ++mi) {
                DistanceSetup s = setups[mi];
                s.device = wk.o.device;
                wk.h.push_back(std::make_unique<DistanceHandle>());
                wk.h.back()->begin(s, KMDB_DISTANCE_SPARSE_OUT);
            }
        kmdb_distance* h0 = wk.h[0]->d;
        const uint64_t row_shift = row_start[i], nr = pc.part_n[i];
        const uint32_t* row_counts = counts32.data() + row_shift;
        const char* const* row_names = name_ptrs.data() + row_shift;
        Db& drow = get(i, i);
        check(kmdb_distance_parts_begin_rows(h0, nr, row_counts, row_names));
        for (size_t j = 0; j < i; ++j) {
            { std::lock_guard<std::mutex> g(mu); std::cerr << "Processing cell (" << i + 1 << "," << j + 1 << ")" << std::endl; }
            Db& dcol = get(j, i);
            if (kmdb_distance_parts_add_db2db(h0, drow.d, dcol.d, row_start[j], &wk.o)) {
                // out of HBM inside the call: the other resident parts go, one more try
                for (size_t q = 0; q < wk.resident.size(); ++q) if (q != i && q != j) wk.resident[q].reset();
                check(kmdb_distance_parts_add_db2db(h0, drow.d, dcol.d, row_start[j], &wk.o));
            }
        }
        { std::lock_guard<std::mutex> g(mu); std::cerr << "Processing cell (" << i + 1 << "," << i + 1 << ")" << std::endl; }
        if (kmdb_distance_parts_add_all2all(h0, drow.d, row_shift, &wk.o)) {
            for (size_t q = 0; q < wk.resident.size(); ++q) if (q != i) wk.resident[q].reset();
            check(kmdb_distance_parts_add_all2all(h0, drow.d, row_shift, &wk.o));
        }
        std::vector<uint64_t> ptr(nr + 1, 0);
        check(kmdb_distance_csr_row_ptr(h0, ptr.data()));          // (gathers)
        for (size_t mi = 0; mi < M; ++mi) {
            kmdb_distance* h = wk.h[mi]->d;
            if (mi) {
                const void *rp = nullptr, *co = nullptr, *va = nullptr;
                uint64_t rows = 0;
                check(kmdb_distance_csr_device(h0, &rp, &co, &va, &rows));
                check(kmdb_distance_take_csr_device(h, rp, co, va, (size_t)rows, row_counts, row_names));
            }
            for (uint64_t r0 = 0; r0 < nr;) {
                uint64_t r1 = r0 + 1;
                while (r1 < nr && ptr[r1 + 1] - ptr[r0] <= budget) ++r1;
                kmdb_distance_out piece{};
                check(kmdb_distance_csr_rows(h, r0, r1, &piece));
                { std::lock_guard<std::mutex> g(mu); block_out[i].pieces[mi].push_back(piece); }
                cv.notify_all();                                   // the writer takes the piece while the device has the next
                r0 = r1;
            }
        }
        std::lock_guard<std::mutex> g(mu);
        block_out[i].done = true;
        cv.notify_all();
    };
    std::vector<std::thread> pool;
    for (size_t t = 0; t < W; ++t)
        pool.emplace_back([&, t]() {
            try {
                for (size_t i = t; i < n_parts; i += W) {
                    { std::lock_guard<std::mutex> g(mu); if (failure) return; }
                    block_row(workers[t], i);
                }
            } catch (...) {
                std::lock_guard<std::mutex> g(mu);
                if (!failure) failure = std::current_exception();
                cv.notify_all();
            }
        });
    bool write_failed = false;
    for (size_t i = 0; i < n_parts && !write_failed;) {
        std::unique_lock<std::mutex> g(mu);
        BlockOut& b = block_out[i];
        auto any = [&] { for (auto& m : b.pieces) if (!m.empty()) return true; return false; };
        cv.wait(g, [&] { return any() || b.done || failure; });
        if (!any() && !b.done) break;                              // (a failure: nothing more comes)
        std::vector<std::vector<kmdb_distance_out>> take(M);
        for (size_t mi = 0; mi < M; ++mi) take[mi].swap(b.pieces[mi]);
        const bool last = b.done;
        g.unlock();
        for (size_t mi = 0; mi < M; ++mi) {
            for (auto& o : take[mi]) {
                if (o.len) ofs[mi].write(o.text, (std::streamsize)o.len);
                kmdb_distance_out_free(&o);
            }
            if (!ofs[mi]) write_failed = true;
        }
        if (last) ++i;
    }
    if (write_failed) { std::lock_guard<std::mutex> g(mu); if (!failure) failure = std::make_exception_ptr(std::runtime_error("Cannot write the output file " + args[1])); }
    for (auto& th : pool) th.join();
    if (verbose && !failure)
        for (size_t t = 0; t < W; ++t) {
            kmdb_distance_parts_stats ps{};
            if (workers[t].h.empty() || kmdb_distance_parts_stats_get(workers[t].h[0]->d, &ps)) continue;
            std::cerr << "[kmdb] distance from the grid, worker " << t << ": block rows " << ps.block_rows << ", cells " << ps.grid_cells << ", entries in " << ps.cells_in
                      << ", written by the device " << ps.cells_written << ", host cells " << ps.host_cells << ", gather " << ps.gather_ms << " ms, peak "
                      << ps.peak_bytes << " B" << std::endl;
        }
    workers.clear();                                              // (the handles and the parts go before the process ends)
    if (failure) std::rethrow_exception(failure);
    for (size_t mi = 0; mi < M; ++mi) {
        ofs[mi].close();
        if (!ofs[mi]) throw std::runtime_error("Cannot write the output file " + paths[mi]);
    }
    return 0;
}

int run_distance(std::vector<std::string>& args, const Common& c) {
    const bool host_only = take_switch(args, "-host");
    bool sparse_out = take_switch(args, "-sparse");
    const bool phylip = take_switch(args, "-phylip-out");
    if (phylip) sparse_out = false;
    auto avail = metrics();
    using Bound = DistanceBound;
    std::map<std::string, Bound> bounds;
    long kmer_lo = 0, kmer_hi = std::numeric_limits<uint32_t>::max();
    take_distance_bounds(args, avail, bounds, kmer_lo, kmer_hi);
    if (args.empty()) throw std::runtime_error("No distance/similarity metric specified");
    const std::string measure_name = args.front();
    args.erase(args.begin());
    if (args.size() < 2) throw usage_error("distance");
    if (!avail.count(measure_name)) throw std::runtime_error("unknown measure: " + measure_name);
    own_bare_bound(bounds, measure_name);
    for (auto& kv : bounds) kv.second.fn = avail[kv.first];
    const metric_fn measure = avail[measure_name];

    std::ifstream in(args[0]);
    if (!in) throw std::runtime_error("Cannot open common k-mers table: " + args[0]);
    std::ofstream out(args[1]);
    std::string tok, rest;
    uint32_t k = 0;
    double fraction = 0;
    in >> tok >> k >> tok >> fraction >> tok;                  // "kmer-length: K fraction: F db-samples"
    std::getline(in, rest);                                    // ",name,name,..."
    if (!phylip) out << "kmer-length: " << k << " fraction: " << fraction << rest << std::endl;
    const std::string header_rest = rest;
    std::vector<std::string> sample_names;
    {
        std::string t = rest;
        std::replace(t.begin(), t.end(), ',', ' ');
        std::istringstream iss(t);
        for (std::string w; iss >> w;) sample_names.push_back(w);
    }
    std::vector<uint32_t> db_counts;
    {
        std::getline(in, rest);                                // "query-samples,total-kmers,c0,c1,..."
        std::replace(rest.begin(), rest.end(), ',', ' ');
        std::istringstream iss(rest);
        iss >> tok >> tok;
        for (unsigned long long c; iss >> c;) db_counts.push_back((uint32_t)c);
    }
    const size_t n = db_counts.size();
    if (phylip) out << n << std::endl;

    {
        const char* forced = std::getenv("KMDB_DISTANCE_DEVICE");
        const char* min_bytes = std::getenv("KMDB_DISTANCE_MIN_BYTES");
        bool on_device = false;
        if (host_only || (forced && forced[0] == '0')) on_device = false;
        else if (forced && forced[0] == '1') {
            if (kmdb_device_count() <= c.device) throw std::runtime_error("KMDB_DISTANCE_DEVICE=1: no usable GPU (device " + std::to_string(c.device) + ")");
            on_device = true;
        } else if (min_bytes) {
            std::ifstream sz(args[0], std::ios::binary | std::ios::ate);
            on_device = sz && (unsigned long long)sz.tellg() >= std::strtoull(min_bytes, nullptr, 10) && kmdb_device_count() > c.device;
        }
        const long long body = (long long)in.tellg();
        if (on_device && body >= 0) {
            DistanceSetup s;
            s.device = c.device; s.measure = kmdbh_metric_id(measure_name.c_str()); s.k = k; s.counts = db_counts; s.sparse_out = sparse_out; s.phylip = phylip;
            s.has_names = !sample_names.empty();
            if (s.has_names) s.first_name = sample_names[0];
            s.filters = distance_filters(bounds, kmer_lo, kmer_hi);
            std::string why;
            out.flush();
            if (distance_on_device(args[0], body, out, s, why)) { out.flush(); return 0; }
            std::cerr << "WARNING: distance: the device path declined this table (" << why << "); the host loop runs" << std::endl;
            out.close();
            out.open(args[1]);                                     // from the start: the header lines again, then every row
            if (!phylip) out << "kmer-length: " << k << " fraction: " << fraction << header_rest << std::endl;
            else out << n << std::endl;
        }
    }

    auto pass = [&](uint32_t common, uint32_t qcnt, size_t col) {
        for (auto& kv : bounds) {
            const double x = kv.second.fn(common, qcnt, db_counts[col], (int)k);
            if (!(x >= kv.second.lo && x <= kv.second.hi)) return false;
        }
        return (long)common >= kmer_lo && (long)common <= kmer_hi;
    };
    auto read_uint = [](const char*& p) { unsigned long long v = 0; while (*p >= '0' && *p <= '9') v = v * 10 + (unsigned)(*p++ - '0'); return v; };

    std::vector<uint32_t> dense(n, 0);
    std::vector<std::pair<size_t, uint32_t>> hits;
    std::vector<char> obuf;
    bool triangle = false;
    std::string line;
    for (size_t row = 0; std::getline(in, line); ++row) {
        const char* p = line.c_str();
        const char* end = p + line.size();
        const char* comma = std::find(p, end, ',');
        const std::string qname(p, comma);
        p = comma < end ? comma + 1 : end;
        const uint32_t qcnt = (uint32_t)read_uint(p);
        if (p < end) ++p;
        size_t n_read = 0;
        for (; end - p > 1; ++n_read) {
            const unsigned long long v = read_uint(p);
            if (*p == ':') {                                   // sparse input: 1-based column, count
                ++p;
                const uint32_t common = (uint32_t)read_uint(p);
                if (phylip) { if (v >= 1 && v <= n) dense[v - 1] = common; }
                else {
                    sparse_out = true;                         // sparse input always gives sparse output
                    if (common > 0 && v >= 1 && v <= n && pass(common, qcnt, v - 1)) hits.emplace_back(v - 1, common);
                }
            } else if (sparse_out) {
                if (v > 0 && n_read < n && pass((uint32_t)v, qcnt, n_read)) hits.emplace_back(n_read, (uint32_t)v);
            } else if (n_read < n) dense[n_read] = (uint32_t)v;
            if (p < end) ++p;
        }
        const bool empty_first = sparse_out ? hits.empty() : (n == 0 || dense[0] == 0);
        if (row == 0 && !sample_names.empty() && qname == sample_names[0] && empty_first) triangle = true;
        const size_t n_proc = sparse_out ? hits.size() : (triangle ? std::min(row, n) : n);
        obuf.resize(qname.size() + 64 + (phylip ? n_read : n_proc) * 48);
        char* o = obuf.data();
        std::memcpy(o, qname.data(), qname.size());
        o += qname.size();
        if (phylip) {
            *o++ = ' ';
            for (size_t c = 0; c < n_read && c < n; ++c) { o += put_measure(c < n_proc ? measure(dense[c], qcnt, db_counts[c], (int)k) : 0.0, o); *o++ = ' '; }
        } else {
            *o++ = ',';
            if (sparse_out)
                for (auto& h : hits) { o += put_uint(h.first + 1, o); *o++ = ':'; o += put_measure(measure(h.second, qcnt, db_counts[h.first], (int)k), o); *o++ = ','; }
            else
                for (size_t c = 0; c < n_proc; ++c) { o += put_measure(measure(dense[c], qcnt, db_counts[c], (int)k), o); *o++ = ','; }
        }
        out.write(obuf.data(), o - obuf.data());
        out << std::endl;
        if (sparse_out && !phylip) hits.clear(); else std::fill(dense.begin(), dense.end(), 0u);
    }
    return 0;
}

void usage() {
    std::cerr << "kmer-db-amd (MI355X engine for kmer-db's all2all / all2all-sp / new2all)\n"
                 "USAGE\n"
                 "    kmer-db-amd all2all [-sparse [-min [<criterion>:]<v>] [-max [<criterion>:]<v>]] <database> <common_table>\n"
                 "    kmer-db-amd all2all-sp [-min ...] [-max ...] <database> <common_table>\n"
                 "    kmer-db-amd new2all [-multisample-fasta | -from-minhash] [-sparse [-min ...] [-max ...]] <database> <sample_list> <common_table>\n"
                 "    kmer-db-amd one2all [-from-minhash] <database> <sample> <similarity_vector>\n"
                 "    kmer-db-amd minhash [-f <fraction>] [-k <kmer-length>] [-alphabet <name>] [-preserve-strand] [-host-extract] <samples>\n"
                 "    kmer-db-amd build [-k <kmer-length>] [-f <fraction>] [-f-start <v>] [-alphabet <name>] [-preserve-strand] [-multisample-fasta] [-host-extract] <sample_list | fasta> <database>\n"
                 "    kmer-db-amd build -from-minhash <sample_list> <database>\n"
                 "    kmer-db-amd build -extend-from <old.db> [-from-minhash] [-multisample-fasta] [-host-extract] <sample_list | fasta> <database>\n"
                 "    kmer-db-amd all2all-parts [-min ...] [-max ...] <db_list> <common_table>\n"
                 "    kmer-db-amd distance [-sparse] [-phylip-out] [-host] [-min [<criterion>:]<v>]* [-max [<criterion>:]<v>]* <measure> <common_table> <output>\n"
                 "Common options: -t <threads>, -gpu <device>\n"
                 "all2all / all2all-sp: -gpus <N>  the k-mer space in N prefix-bucket shards over the node's GPUs (from -gpu on), partial matrices\n"
                 "                                  summed by one RCCL reduce-scatter; more shards than devices: a device runs its shards in turn\n"
                 "                      -partition prefix|range  (with -gpus) what a shard is: the k-mers of a set of prefix buckets (default; the\n"
                 "                                  database is read with its hashtables), or a range of the pattern tree (read without them)\n"
                 "new2all / one2all: -gpus <N>     the database in N query shards over the node's GPUs (from -gpu on): a shard holds the tree and the\n"
                 "                                  hashtable slots of its own prefix buckets; the rows of the shards are summed by one RCCL reduce-scatter\n"
                 "                   -from-minhash the samples are <sample>.minhash files (written by the minhash mode): their k-mers are used as stored\n"
                 "new2all: -sample-rows <criterion>:<count>  a search: every query keeps its <count> best database samples by <criterion> among the cells\n"
                 "                                  that pass -min / -max (sparse output; ties towards the smaller sample id), selected on the GPU;\n"
                 "                                  KMDB_N2A_HOST_SAMPLER=1 keeps the sampler on the host (same bytes).  With -gpus <N> every GPU selects\n"
                 "                                  on its share of the rows.  Refused with -distance and without a criterion.\n"
                 "minhash: <samples> is a list of FASTA files (or one FASTA file); <sample>.minhash = its k-mers that pass the filter (-f, default 0.01),\n"
                 "                   sorted and unique, extracted on the GPU; -host-extract extracts them on the host and needs no GPU\n"
                 "build: the database is grown on the GPU from the samples in input order and written in the reference's format; -from-minhash takes\n"
                 "                   <sample>.minhash files (k and fraction from the files); -extend-from <old.db> starts from a stored database (its k,\n"
                 "                   fraction and alphabet; <database> may be <old.db>); -extend and -from-kmers are refused\n"
                 "distance: KMDB_DISTANCE_DEVICE=1 parses, measures and formats the table on the GPU (-gpu <device>; same bytes); -host and\n"
                 "                   KMDB_DISTANCE_DEVICE=0 keep it on the host, which is also what runs when neither is given\n"
                 "all2all-parts: -gpus <W>         the block rows of the grid dealt to W workers over the node's GPUs (parts resident per device)\n"
                 "               -sample-rows <criterion>:<count>  every cell's candidates are selected on the GPU (same bytes); KMDB_PARTS_HOST_SAMPLER=1,\n"
                 "                                  KMDB_PARTS_DENSE_CELLS=1, more than 12 bounds and -sample-rows <count> (random) keep the sampler on the host\n"
                 "    kmer-db-amd all2all | all2all-sp [-sparse] [-phylip-out] [-min [<criterion>:]<v>]* [-max [<criterion>:]<v>]* -distance <measure> [-distance <measure>]* <database> <output>\n"
                 "all2all / all2all-sp -distance:  the table of <measure> straight from the matrix on the GPU: the file `all2all` followed by `distance`\n"
                 "                                  writes, without the table of counts in between; all2all-sp forces -sparse.  Several -distance: one all2all\n"
                 "                                  run, a file <output>.<measure> each.  -min / -max are read as the DISTANCE mode reads them here: a bare\n"
                 "                                  bound belongs to <measure> (NOT to num-kmers as in all2all -sparse), num-kmers:<v> bounds the count.\n"
                 "                                  Refused with -gpus <N> and with -sample-rows.\n"
                 "    kmer-db-amd new2all [-sparse] [-phylip-out] [-min ...]* [-max ...]* [-multisample-fasta | -from-minhash] [-host-extract] -distance <measure> [-distance <measure>]* <database> <sample_list> <output>\n"
                 "new2all -distance:               the table of <measure> straight from the query rows on the GPU: the file `new2all` followed by `distance`\n"
                 "                                  writes, without the table of counts in between; several -distance and the -min / -max list as above.\n"
                 "                                  Refused with -gpus <N>, and where the distance mode would take the table for a triangle (the first query\n"
                 "                                  named like the first sample and sharing no k-mer with it; -sparse is not affected).\n"
                 "    kmer-db-amd all2all-parts [-min ...]* [-max ...]* [-gpus <W>] -distance <measure> [-distance <measure>]* <db_list> <output>\n"
                 "all2all-parts -distance:         the table of <measure> straight from the block rows of the grid on the GPU: the file `all2all-parts`\n"
                 "                                  followed by `distance -sparse` writes, without the table of counts in between; always the sparse form\n"
                 "                                  (-sparse changes nothing).  Several -distance and the -min / -max list as above; -gpus <W> as in\n"
                 "                                  all2all-parts.  Refused with -sample-rows and with -phylip-out.\n"
                 "    kmer-db-amd all2all | all2all-sp -from-samples [build's input switches] [-keep-db <database>] [the mode's own switches] <sample_list | fasta> <output>\n"
                 "all2all / all2all-sp -from-samples: the samples in, the table out: the database is grown on the GPU as by build and handed to the engine in\n"
                 "                                  HBM, no .db in between; <output> holds what build followed by the mode writes.  Build's input switches:\n"
                 "                                  -k -f -f-start -alphabet -preserve-strand -multisample-fasta -from-minhash -host-extract -extend-from <old.db>;\n"
                 "                                  the mode's own, -distance <measure> included, as on one GPU.  -keep-db <database> also stores the file\n"
                 "                                  build would have written.  Refused with -gpus <N>, -from-kmers and -extend; -keep-db needs -from-samples.\n"
                 "                                  Not offered: new2all / one2all -from-samples, all2all-parts, any -gpus.\n"
                 "    kmer-db-amd all2all | all2all-sp -rows <lo>:<hi> [the mode's own switches] <database> <output>\n"
                 "all2all / all2all-sp -rows <lo>:<hi>: only the rows of samples lo .. hi - 1 (0-based, either side may be empty: 100: is 100 to N) are computed,\n"
                 "                                  as a band of the matrix of its own on the GPU; <output> holds the header lines of the full run and exactly\n"
                 "                                  its lines of those samples.  Dense, -sparse / all2all-sp with the -min / -max list, and -distance <measure>.\n"
                 "                                  -rows new (with -from-samples -extend-from <old.db>): the rows of the samples added to <old.db>.\n"
                 "                                  Refused with -gpus <N>, -sample-rows and -phylip-out, and when hi exceeds the sample count.\n"
                 "    kmer-db-amd all2all | all2all-sp -band-rows <R> [the mode's own switches] <database> <output>\n"
                 "all2all / all2all-sp -band-rows <R>: the whole run walked in bands of R rows — one band of the matrix is resident at a time, its rows summed\n"
                 "                                  in LDS tiles on the GPU; <output> holds, byte for byte, what the same command without -band-rows writes:\n"
                 "                                  the way of one GPU to a collection whose triangle does not fit its memory.  Dense, -sparse / all2all-sp\n"
                 "                                  with the -min / -max list, and -distance <measure> (repeated too).  With -rows <lo>:<hi> | new that range\n"
                 "                                  is walked in bands; with -from-samples [-extend-from <old.db>] as well.  Refused with -gpus <N>, -sample-rows\n"
                 "                                  and -phylip-out, and when R is 0 or no number.  KMDB_ROWS_TILE_COLS / KMDB_ROWS_TILE_HITS: a tile's columns\n"
                 "                                  and the hits of a share; KMDB_ROWS_TILED=1: plain -rows takes the tiled call too.  Not offered: a long\n"
                 "                                  pattern's list decoded by several lanes.\n"
                 "    kmer-db-amd all2all | all2all-sp -rows <lo>:<hi> | -band-rows <R> -band-path <tree|tiled|records> [...] <database> <output>\n"
                 "all2all / all2all-sp -band-path <tree|tiled|records>: the call every band of -rows / -band-rows comes from — tree: the pattern tree walked,\n"
                 "                                  rows added cell by cell (the default of -rows); tiled: rows summed in LDS tiles (the default of\n"
                 "                                  -band-rows); records: the block-record pipeline of the whole-matrix call (decode, emit and sort run whole,\n"
                 "                                  the matrix-core apply on the band's block rows alone).  <output> holds the same bytes in all three.\n"
                 "                                  Refused without -rows / -band-rows, with any other value and in any other mode; KMDB_K1N_MODE=1 is\n"
                 "                                  refused.  Beyond 2^22 block pairs (about 185 000 samples at width 64) records takes band emit by itself:\n"
                 "                                  the records of the band's block rows alone, keyed relative to the band — fewer than 2^22 streams per band\n"
                 "                                  and at most some 7 500 blocks (240 000 samples at width 32, 480 000 at width 64), else the band comes from\n"
                 "                                  tree.  KMDB_BAND_EMIT=1 | 0: band emit for every band | never.  KMDB_VERBOSE: one line per band with the\n"
                 "                                  form (whole emit | band emit), the band's streams and the band state's bytes.\n";
}

}  // namespace

int main(int argc, char** argv) {
    const double up_at_main = since_process_start();
    if (std::getenv("KMDB_VERBOSE")) std::cerr << "[kmdb] main() entered " << up_at_main << " s after the process started" << std::endl;
    std::vector<std::string> args(argv + 1, argv + argc);
    try {
        if (args.empty()) { usage(); return 0; }
        std::string mode = args[0];
        args.erase(args.begin());
        Common c;
        std::string v;
        if (take_option(args, "-t", v)) c.threads = std::atoi(v.c_str());
        take_option(args, "-rt", v);
        if (take_option(args, "-gpu", v)) c.device = std::atoi(v.c_str());
        if (take_option(args, "-gpus", v)) {
            c.gpus = std::atoi(v.c_str());
            if (c.gpus < 1 || c.gpus > 4096) throw std::runtime_error("-gpus expects a number of prefix-bucket shards (1 or more)");
            if (mode != "all2all" && mode != "all2all-sp" && mode != "all2all-parts" && mode != "new2all" && mode != "one2all") throw std::runtime_error("-gpus applies to all2all, all2all-sp, all2all-parts, new2all and one2all");
        }
        if (take_option(args, "-partition", v)) {
            if (v == "prefix") c.partition = KMDB_PARTITION_PREFIX;
            else if (v == "range") c.partition = KMDB_PARTITION_RANGE;
            else throw std::runtime_error("-partition expects prefix or range");
            if (mode != "all2all" && mode != "all2all-sp") throw std::runtime_error("-partition applies to all2all and all2all-sp");
            if (c.gpus < 1) throw std::runtime_error("-partition goes with -gpus <N>");
        }
        take_switch(args, "-v");
        take_switch(args, "-vv");
        // all2all | all2all-sp -from-samples: refused by name here, before any file is read or any device touched
        const bool keep_db = take_option(args, "-keep-db", c.keep_db);
        if ((mode == "all2all" || mode == "all2all-sp") && take_switch(args, "-from-samples")) {
            if (c.gpus > 0) throw std::runtime_error("-from-samples does not go with -gpus <N>: the builder hands its database to the engine on its own device (run build, then " + mode + " -gpus)");
            for (auto& a : args) {
                if (a == "-from-kmers") throw std::runtime_error(KMC_REFUSAL);
                if (a == "-extend") throw std::runtime_error("-from-samples does not go with -extend: start from a stored database with -extend-from <old.db>");
            }
            c.from_samples = std::make_shared<BuildInput>();
            c.from_samples->parse(args);
        } else if (keep_db) throw std::runtime_error("-keep-db <database> goes with all2all | all2all-sp -from-samples only: it names the file build would have written");
        // -rows <lo>:<hi> | new: what it does not go with is refused by name here, before any file is read or any device touched
        if (take_option(args, "-rows", v)) {
            if (mode != "all2all" && mode != "all2all-sp") throw std::runtime_error("-rows applies to all2all and all2all-sp");
            if (c.gpus > 0) throw std::runtime_error("-rows does not go with -gpus <N>: a band is computed on one device from the whole pattern tree");
            for (auto& a : args) {
                if (a == "-sample-rows") throw std::runtime_error("-rows does not go with -sample-rows: a pair is offered to both its samples, so a band of rows does not hold a sample's candidates");
                if (a == "-phylip-out") throw std::runtime_error("-rows does not go with -phylip-out: a phylip table is a whole triangle");
            }
            c.rows.parse(v);
            if (c.rows.is_new && !(c.from_samples && c.from_samples->extend))
                throw std::runtime_error("-rows new goes with -from-samples -extend-from <old.db> only: it means the rows of the samples added to <old.db>");
        }
        // -band-rows <R>: the same
        if (std::find(args.begin(), args.end(), "-band-rows") != args.end()) {
            if (mode != "all2all" && mode != "all2all-sp") throw std::runtime_error("-band-rows applies to all2all and all2all-sp");
            if (c.gpus > 0) throw std::runtime_error("-band-rows does not go with -gpus <N>: a band is computed on one device from the whole pattern tree");
            for (auto& a : args) {
                if (a == "-sample-rows") throw std::runtime_error("-band-rows does not go with -sample-rows: a pair is offered to both its samples, so a band of rows does not hold a sample's candidates");
                if (a == "-phylip-out") throw std::runtime_error("-band-rows does not go with -phylip-out: a phylip table is a whole triangle");
            }
            if (!take_option(args, "-band-rows", v)) throw std::runtime_error("-band-rows expects <R>, a number of rows of 1 or more");
            c.band_rows = parse_band_rows(v);
        }
        // -band-path <tree|tiled|records>: the band call of the two switches above, refused by name without them
        if (std::find(args.begin(), args.end(), "-band-path") != args.end()) {
            if (mode != "all2all" && mode != "all2all-sp") throw std::runtime_error("-band-path applies to all2all and all2all-sp");
            if (!take_option(args, "-band-path", v)) throw std::runtime_error("-band-path expects tree, tiled or records");
            c.band_path = parse_band_path(v);
            if (!c.rows.on && !c.band_rows) throw std::runtime_error("-band-path goes with -rows <lo>:<hi> | new and / or -band-rows <R> only: it names the call a band of rows comes from");
        }
        if (mode == "all2all") return run_all2all(args, c);
        if (mode == "all2all-sp") return run_all2all_sp(args, c);
        if (mode == "new2all") return run_new2all(args, c);
        if (mode == "one2all") return run_one2all(args, c);
        if (mode == "all2all-parts") return run_all2all_parts(args, c);
        if (mode == "distance") return run_distance(args, c);
        if (mode == "minhash") return run_minhash(args, c);
        if (mode == "build") return run_build(args, c);
        usage();
        return -1;
    } catch (usage_error&) {
        usage();
        return -1;
    } catch (std::exception& e) {
        std::cerr << "ERROR: " << e.what() << std::endl;       // main.cpp:56-59
        return -1;
    }
}
