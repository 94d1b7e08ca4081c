// distance.hip — the distance mode on the device (console_distance.cpp:75-204): a run of whole table rows, text in and text out.
//
//   classify  a lane per byte, a wave per 64-byte window: ballots of '\n' and of the separators, the windows' counts scanned (prim.h).  The
//             rows come out of the '\n' count, a row's first comma (the end of its name) out of one atomicMin per window and row, the
//             fields ("tokens": what follows a ',' or ':' behind the name) out of the separator count.  Nothing walks a row.
//   parse     a lane per token: at most 10 digits into 64 bits, truncated to uint32 as the host loop truncates; the row rules' flags.
//   measure   a lane per OUTPUT cell (dense: n or min(row, n) per row whatever the row holds; otherwise one per token): kmdbh_metric's
//             expressions in double with contraction off, the bounds, the text length.  A cell the device's arithmetic cannot settle
//             (dev_code) takes no bytes and is listed for the host.
//   format    one scan of the lengths, the output allocated to its size, a lane per cell writes its digits, a wave per row its name.
//
// The cells have two sources behind the same measure and format stages: the tokens parsed from text (TextCells), and a lower triangle of
// counts that is in HBM already (TriangleCells: kmdb_distance_take_* and kmdb_distance_matrix_rows) — output cell ci of a piece of rows IS
// matrix cell piece_lo + ci, consecutive lanes read consecutive uint32, nothing is classified or parsed and the names come from a blob.
// A third source is the row-major nq x N rectangle of a batch of new2all queries (RowCells: kmdb_distance_take_new2all_batch*,
// kmdb_distance_take_rows_device and kmdb_distance_query_rows) — the same, with whole rows of N cells, a = the QUERY's own count and the
// names of the queries.  A fourth is a CSR in HBM over a run of rows (CsrCells: kmdb_distance_parts_*, kmdb_distance_take_csr_device and
// kmdb_distance_csr_rows) — a block row of the all2all-parts grid, gathered from its cells' CSRs by the two kernels at the end of this file:
// output cell ci IS entry piece_lo + ci, its row found in the rebased row_ptr, a = the ROW sample's own count.
// The three sources in HBM share their host side too (dist_piece): a source is a struct that says what a cell is (at), where a row's name
// lies (name) and how many cells a row has (row_cells), and a lambda of its entry point that sets the fields of DistParams these read.
//
// Every position is below the piece's length by construction and clamped to it again where it is used: damaged text is declined
// (KMDB_DISTANCE_DECLINED) or parsed as the host loop parses it, and never read or written outside the buffers.
#include "kmdb_amd.h"
#include "dev_mem.h"
#include "engine_internal.h"
#include "engine_state.h"
#include "prim.h"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <vector>

// hipcc contracts v * 1e6 + 0.5 into an fma by default; the host compiler of the reference does not
#pragma clang fp contract(off)

static_assert(KMDB_DISTANCE_MAX_FILTERS == 12, "cell_filter.h's DEV_FILTER_MAX");

namespace {

constexpr int DT = 256;                         // threads per workgroup, four windows
constexpr uint32_t NONE = 0xFFFFFFFFu;

enum { MODE_DENSE = 0, MODE_SPARSE_OUT, MODE_SPARSE_IN, MODE_PHYLIP };
// why a piece is declined (the largest code wins: any will do)
enum { DECL_NONE = 0, DECL_NO_COMMA, DECL_DIGITS, DECL_CHAR, DECL_COLONS, DECL_PAIR, DECL_PLAIN };
// token flags
enum : uint8_t { TF_OPEN_COLON = 1, TF_TERM_COLON = 2, TF_READ = 4, TF_OVER32 = 8 };
// cell codes: bits 0..59 x = (uint64)(|v| * 1e6 + 0.5)
constexpr uint64_t C_ZERO = 1ull << 60, C_NEG = 1ull << 61, C_HOST = 1ull << 62, C_SKIP = 1ull << 63, C_X = (1ull << 60) - 1;

struct DistParams {
    const unsigned char* text;
    uint32_t L;                 // bytes
    uint32_t R;                 // rows
    uint32_t M;                 // tokens
    uint32_t n;                 // columns
    const uint32_t* counts;     // [n]
    int mode, measure, k, triangle;
    uint64_t first_row;
    int n_filters;
    int f_metric[KMDB_DISTANCE_MAX_FILTERS];
    double f_lo[KMDB_DISTANCE_MAX_FILTERS], f_hi[KMDB_DISTANCE_MAX_FILTERS];
    // classification
    const uint32_t* weol;       // [NW + 1] '\n' before the window
    const uint32_t* wsep;       // [NW + 1] separators before the window
    uint32_t* fc;               // [R] first comma of the row, NONE: none
    uint32_t* row_end;          // [R] the row's '\n', L for a last row without one
    uint32_t* row_first;        // [R + 1] the row's first token (its own k-mer count); [R] = M
    uint32_t* sep_pos;          // [M] the separator in front of the token
    uint32_t* sep_row;          // [M]
    uint32_t* tok_val;          // [M]
    uint8_t* tok_flags;         // [M]
    // rows and cells
    uint64_t* oc;               // [R + 1] output cells of the row, scanned in place: the first cell of the row, [R] = all
    uint64_t* rowfix;           // [R + 1] name + separator + '\n', scanned in place
    uint64_t n_cells;
    uint64_t* code;             // [n_cells]
    uint8_t* len;               // [n_cells]
    uint64_t* off;              // [n_cells + 1] scanned lengths
    unsigned int* decline;
    unsigned long long* counters;   // [0] cells read [1] cells the device wrote [2] cells for the host [3] entries appended
    // counts that lie in HBM as the source of cells.  TriangleCells: the lower triangle, row i at cell i (i - 1) / 2; RowCells: the row-major
    // nq x n rectangle of a batch of queries.  The piece's rows are first_row .. first_row + R of either.
    const uint32_t* cells;          // source cell cells_lo and what follows it
    uint64_t cells_lo, cells_len;   // the first source cell behind `cells` (the rectangle: 0), and how many there are
    uint64_t piece_lo;              // the source cell (CsrCells: the entry) of the piece's output cell 0
    const unsigned char* names;     // the rows' names back to back: the samples' (TriangleCells), the queries' or the row samples' (RowCells, CsrCells)
    const uint64_t* name_off;       // [n + 1] or [rows_nq + 1] where a name begins
    const uint32_t* row_counts;     // [rows_nq] RowCells, CsrCells: the rows' own k-mer counts
    uint64_t rows_nq;
    // a CSR as the source of cells (CsrCells): entry piece_lo + ci of csr_col / csr_val
    const uint64_t* csr_ptr;        // [rows_nq + 1] row_ptr, ascending from 0 to csr_nnz (dist_csr_adopt has seen to it)
    const uint32_t* csr_col;        // 0-based global columns, ascending within a row
    const uint32_t* csr_val;
    uint64_t csr_nnz;
};

// a cell the host decides: where its text goes, and what it is
struct HostCell {
    uint64_t ci;                // output cell index: the order of the text
    uint64_t off;               // byte offset in the device's text
    uint32_t col;               // 0-based column
    uint32_t count, a;
    uint32_t pad;
};

__device__ __forceinline__ uint64_t lanes_below() { return (1ull << (threadIdx.x & 63)) - 1; }

// ---- classify ---------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(DT) dist_eol_count_kernel(const unsigned char* text, uint32_t L, uint32_t* wcnt) {
    const uint64_t i = (uint64_t)blockIdx.x * DT + threadIdx.x;
    const bool eol = i < L && text[i] == '\n';
    const uint64_t m = __ballot(eol);
    if ((threadIdx.x & 63) == 0 && i < L) wcnt[i >> 6] = (uint32_t)__popcll(m);
}

// the rows' ends and first commas: one atomicMin per window and row (the first comma of the row inside the window)
__global__ void __launch_bounds__(DT) dist_rows_kernel(DistParams p) {
    const uint64_t i = (uint64_t)blockIdx.x * DT + threadIdx.x;
    const bool in = i < p.L;
    const unsigned char ch = in ? p.text[i] : 0;
    const uint64_t eols = __ballot(in && ch == '\n'), commas = __ballot(in && ch == ',');
    if (!in) return;
    const uint64_t below = lanes_below();
    const uint32_t row = p.weol[i >> 6] + (uint32_t)__popcll(eols & below);
    if (row >= p.R) return;                                     // (cannot happen: R counts the '\n' and a last row without one)
    if (ch == '\n') p.row_end[row] = (uint32_t)i;
    else if (ch == ',') {
        const uint64_t e = eols & below;
        const uint64_t since = e ? ~((2ull << (63 - __clzll(e))) - 1) : ~0ull;      // the lanes behind the last '\n' in front of this one
        if (!(commas & below & since)) atomicMin(&p.fc[row], (uint32_t)i);
    }
}

__device__ __forceinline__ bool dist_is_sep(const DistParams& p, uint64_t i, bool in, unsigned char ch, uint64_t eols, uint32_t* row_out) {
    if (!in) return false;
    const uint32_t row = p.weol[i >> 6] + (uint32_t)__popcll(eols & lanes_below());
    *row_out = row;
    return (ch == ',' || ch == ':') && row < p.R && i >= p.fc[row];
}

__global__ void __launch_bounds__(DT) dist_sep_count_kernel(DistParams p, uint32_t* wcnt) {
    const uint64_t i = (uint64_t)blockIdx.x * DT + threadIdx.x;
    const bool in = i < p.L;
    const unsigned char ch = in ? p.text[i] : 0;
    const uint64_t eols = __ballot(in && ch == '\n');
    uint32_t row = 0;
    const uint64_t seps = __ballot(dist_is_sep(p, i, in, ch, eols, &row));
    if ((threadIdx.x & 63) == 0 && in) wcnt[i >> 6] = (uint32_t)__popcll(seps);
}

__global__ void __launch_bounds__(DT) dist_sep_write_kernel(DistParams p) {
    const uint64_t i = (uint64_t)blockIdx.x * DT + threadIdx.x;
    const bool in = i < p.L;
    const unsigned char ch = in ? p.text[i] : 0;
    const uint64_t eols = __ballot(in && ch == '\n');
    uint32_t row = 0;
    const bool sep = dist_is_sep(p, i, in, ch, eols, &row);
    const uint64_t seps = __ballot(sep);
    if (!sep) return;
    const uint32_t j = p.wsep[i >> 6] + (uint32_t)__popcll(seps & lanes_below());
    if (j >= p.M) return;
    p.sep_pos[j] = (uint32_t)i;
    p.sep_row[j] = row;
    if (i == p.fc[row]) p.row_first[row] = j;
}

// ---- parse ------------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void dist_decline(const DistParams& p, unsigned int why) { atomicMax(p.decline, why); }

__global__ void __launch_bounds__(DT) dist_parse_kernel(DistParams p) {
    const uint64_t j = (uint64_t)blockIdx.x * DT + threadIdx.x;
    bool counted = false;
    if (j < p.M) {
        const uint32_t pos = min(p.sep_pos[j], p.L - 1), r = min(p.sep_row[j], p.R - 1);
        const uint32_t rend = min(p.row_end[r], p.L);
        const bool more = j + 1 < p.M && p.sep_row[j + 1] == r;
        const uint32_t start = min(pos + 1, rend);
        const uint32_t stop = more ? max(start, min(p.sep_pos[j + 1], rend)) : rend;
        uint8_t fl = 0;
        if (p.text[pos] == ':') fl |= TF_OPEN_COLON;
        if (more && p.text[min(p.sep_pos[j + 1], p.L - 1)] == ':') fl |= TF_TERM_COLON;
        if (rend - start > 1) fl |= TF_READ;                    // console_distance.cpp:100: a cell is read while end - p > 1
        const uint32_t len = stop - start;
        if (len > 10) dist_decline(p, DECL_DIGITS);
        unsigned long long v = 0;
        for (uint32_t q = 0; q < min(len, 10u); ++q) {
            const unsigned char ch = p.text[start + q];
            if (ch < '0' || ch > '9') { dist_decline(p, DECL_CHAR); break; }
            v = v * 10 + (unsigned)(ch - '0');
        }
        if (v >> 32) fl |= TF_OVER32;
        p.tok_val[j] = (uint32_t)v;
        p.tok_flags[j] = fl;
        const uint32_t first = p.row_first[r];
        if ((fl & TF_TERM_COLON) && (j == first || (fl & TF_OPEN_COLON))) dist_decline(p, DECL_COLONS);     // "count:x", "a:b:c"
        if (j != first && !(fl & TF_OPEN_COLON) && (fl & TF_READ)) {                                         // a cell the row rules read
            counted = true;
            const bool pair = fl & TF_TERM_COLON;
            if (pair && p.mode != MODE_SPARSE_IN) dist_decline(p, DECL_PAIR);
            if (!pair && p.mode == MODE_SPARSE_IN) dist_decline(p, DECL_PLAIN);
        }
    }
    const uint64_t m = __ballot(counted);
    if ((threadIdx.x & 63) == 0 && m) atomicAdd(&p.counters[0], (unsigned long long)__popcll(m));
}

// a lane per row of the text: a row without a comma is declined; the output cells of the row and the bytes around them
__global__ void __launch_bounds__(DT) dist_text_row_sizes_kernel(DistParams p) {
    const uint64_t r = (uint64_t)blockIdx.x * DT + threadIdx.x;
    if (r >= p.R) return;
    const uint32_t fc = p.fc[r];
    if (fc == NONE) { dist_decline(p, DECL_NO_COMMA); p.oc[r] = 0; p.rowfix[r] = 0; return; }
    const uint32_t start = r ? min(p.row_end[r - 1] + 1, p.L) : 0;
    const uint32_t tb = p.row_first[r], te = p.row_first[r + 1];
    uint64_t cells;
    if (p.mode == MODE_DENSE) cells = p.triangle ? min((uint64_t)p.n, p.first_row + r) : (uint64_t)p.n;
    else cells = te > tb ? te - tb - 1 : 0;
    p.oc[r] = cells;
    p.rowfix[r] = (uint64_t)(fc >= start ? fc - start : 0) + 2;
}

// ---- measure ----------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ double dev_mash(double j, int k) { return j == 0 ? 1.0 : (-1.0 / k) * log((2 * j) / (j + 1)); }

// kmdbh_metric's expressions (host_metrics.cpp).  *exact: the value is the host's bit for bit (correctly rounded operations only);
// *zero_ok: a result of 0 is one the host computes as 0 too.
__device__ double dev_metric(int metric, uint32_t c, uint32_t a, uint32_t b, int k, bool* exact, bool* zero_ok) {
    *exact = true; *zero_ok = true;
    switch (metric) {
    case KMDB_METRIC_JACCARD:     return (double)c / (double)(uint32_t)(a + b - c);
    case KMDB_METRIC_MIN:         return (double)c / (double)(a < b ? a : b);
    case KMDB_METRIC_MAX:         return (double)c / (double)(a > b ? a : b);
    case KMDB_METRIC_COSINE:      *exact = false; return (double)c / sqrt((double)(uint32_t)(a * b));
    case KMDB_METRIC_MASH:        *exact = false; return dev_mash((double)c / (double)(uint32_t)(a + b - c), k);     // 0 only where the log's argument is 1
    case KMDB_METRIC_ANI:         { *exact = false; const double j = (double)c / (double)(uint32_t)(a + b - c); *zero_ok = j == 0; return 1.0 - dev_mash(j, k); }
    case KMDB_METRIC_ANI_SHORTER: { *exact = false; const double j = (double)c / (double)(a < b ? a : b); *zero_ok = j == 0; return 1.0 - dev_mash(j, k); }
    case KMDB_METRIC_MASH_QUERY:  *exact = false; return dev_mash((double)c / (double)a, k);
    default:                      return (double)c;
    }
}

// The text of a value, or C_HOST where the device's few ulp could change it: t = |v| * 1e6 + 0.5 within 2^-20 of an integer — for a log /
// sqrt measure within t * 2^-44 where that is more: a few hundred ulp of t, whatever its size — v not finite or of 10^12 and more, a
// value below 10^-9 that is not an exact zero (its sign and its being zero are not settled here).
__device__ uint64_t dev_code(double v, bool exact, bool zero_ok) {
    if (v == 0) return zero_ok ? C_ZERO : C_HOST;
    const double m = fabs(v);
    if (!(m < 1e12)) return C_HOST;                             // NaN and infinities too
    if (!exact && m < 1e-9) return C_HOST;
    const double t = m * 1000000.0 + 0.5;
    if (fabs(t - rint(t)) <= (exact ? 0x1p-20 : fmax(0x1p-20, t * 0x1p-44))) return C_HOST;
    return (uint64_t)t | (v < 0 ? C_NEG : 0);
}

__device__ __forceinline__ uint32_t dev_digits(uint64_t v) {
    uint32_t n = 1;
    while (v >= 10) { v /= 10; ++n; }
    return n;
}

// 0: the bounds drop the cell; 1: they keep it; 2: a bound lies within 1e-9 * max(1, |bound|) of the device's value: the host decides
__device__ int dev_bounds(const DistParams& p, uint32_t c, uint32_t a, uint32_t b) {
    int verdict = 1;
    for (int i = 0; i < p.n_filters; ++i) {
        bool exact, zero_ok;
        const double x = dev_metric(p.f_metric[i], c, a, b, p.k, &exact, &zero_ok), lo = p.f_lo[i], hi = p.f_hi[i];
        if (p.f_metric[i] == KMDB_METRIC_NUM_KMERS) { if (!(x >= lo && x <= hi)) return 0; continue; }      // an integer: nothing to settle
        if (!(fabs(x) <= 1.7e308)) { verdict = 2; continue; }
        if (fabs(x - lo) <= 1e-9 * fmax(1.0, fabs(lo)) || fabs(x - hi) <= 1e-9 * fmax(1.0, fabs(hi))) { verdict = 2; continue; }
        if (!(x >= lo && x <= hi)) return 0;                    // clear of every margin: dropped whatever the undecided bounds say
    }
    return verdict;
}

struct Cell {
    uint32_t row, col, count, a;
    uint32_t prefix;            // the column printed in front of the value, 0: none
    bool emit;                  // the row rules write it (bounds aside)
    bool zero;                  // phylip: a value beyond the row's processed count
};

// the row of an output cell: the last row whose first cell is at or below it (rows without cells share their successor's)
__device__ __forceinline__ uint32_t dev_row_of(const uint64_t* base, uint32_t R, uint64_t ci) {
    uint32_t lo = 0, hi = R;                                    // base[lo] <= ci < base[hi]
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (base[mid] <= ci) lo = mid; else hi = mid;
    }
    return lo;
}

// ---- the sources of cells: what output cell ci is, and where the name of row r lies -------------------------------------------------------
struct TextCells {
    static __device__ Cell at(const DistParams& p, uint64_t ci);
    static __device__ __forceinline__ const unsigned char* name(const DistParams& p, uint32_t r, uint32_t* nlen) {
        const uint32_t start = r ? min(p.row_end[r - 1] + 1, p.L) : 0;
        const uint32_t fc = min(p.fc[r], p.L);
        *nlen = fc >= start ? fc - start : 0;
        return p.text + start;
    }
};

__device__ Cell TextCells::at(const DistParams& p, uint64_t ci) {
    Cell x{};
    const uint32_t r = dev_row_of(p.oc, p.R, ci);
    const uint64_t c = ci - p.oc[r];
    const uint32_t tb = min(p.row_first[r], p.M - 1), te = min(p.row_first[r + 1], p.M);
    const uint64_t j = (uint64_t)tb + 1 + c;
    const bool has = j < te && (p.tok_flags[j] & TF_READ);
    x.row = r;
    x.a = p.tok_val[tb];
    switch (p.mode) {
    case MODE_DENSE:                                            // every cell of the row's processed count, 0 where the row holds none
        x.col = (uint32_t)c; x.count = has ? p.tok_val[j] : 0; x.emit = c < p.n;
        break;
    case MODE_PHYLIP: {                                         // min(n_read, n) values; 0 beyond the processed count
        const uint64_t n_proc = p.triangle ? min((uint64_t)p.n, p.first_row + r) : (uint64_t)p.n;
        x.col = (uint32_t)c; x.emit = has && c < p.n; x.count = has ? p.tok_val[j] : 0; x.zero = c >= n_proc;
        break;
    }
    case MODE_SPARSE_OUT:
        // (the loop tests v > 0 on the 64 bits it read and keeps the 32 it stores: 2^32 is a cell of count 0)
        x.col = (uint32_t)c; x.count = has ? p.tok_val[j] : 0; x.emit = has && c < p.n && (x.count > 0 || (p.tok_flags[j] & TF_OVER32)); x.prefix = (uint32_t)c + 1;
        break;
    default: {                                                  // pairs: the column token (opened by ','), its count in the next one
        const bool pair = has && !(p.tok_flags[j] & TF_OPEN_COLON) && (p.tok_flags[j] & TF_TERM_COLON) && j + 1 < te;
        const uint32_t col = pair ? p.tok_val[j] : 0;
        const bool ok = pair && !(p.tok_flags[j] & TF_OVER32) && col >= 1 && col <= p.n;
        x.count = ok ? p.tok_val[j + 1] : 0; x.col = ok ? col - 1 : 0; x.prefix = col; x.emit = ok && x.count > 0;
        break;
    }
    }
    return x;
}

// the row i of the triangle that holds matrix cell g: i (i - 1) / 2 <= g < i (i + 1) / 2 (i >= 1; 64 bits: i (i - 1) passes 2^32 from row 65 537 on)
__device__ __forceinline__ uint64_t dev_tri_row(uint64_t g) {
    uint64_t i = (uint64_t)((1.0 + sqrt(1.0 + 8.0 * (double)g)) * 0.5);
    if (i < 1) i = 1;
    while (i > 1 && i * (i - 1) / 2 > g) --i;                   // (the square root of a number of 2^40 and more is a unit or so off)
    while (i * (i + 1) / 2 <= g) ++i;
    return i;
}

struct TriangleCells {
    // every cell of the piece is a cell of the matrix: the count is read where it lies, the row's own count is a = counts[row]
    static __device__ Cell at(const DistParams& p, uint64_t ci) {
        Cell x{};
        const uint64_t g = p.piece_lo + ci;
        uint64_t i = dev_tri_row(g);
        i = min(max(i, p.first_row), p.first_row + p.R - 1);    // clamped to the piece
        const uint64_t c = min(g - min(g, i * (i - 1) / 2), (uint64_t)p.n - 1);
        x.row = (uint32_t)(i - p.first_row);
        x.col = (uint32_t)c;
        x.a = p.counts[min(i, (uint64_t)p.n - 1)];
        x.count = p.cells[min(g - p.cells_lo, p.cells_len - 1)];
        x.emit = p.mode != MODE_SPARSE_OUT || x.count > 0;
        x.prefix = p.mode == MODE_SPARSE_OUT ? (uint32_t)c + 1 : 0;
        return x;
    }
    static __device__ __forceinline__ const unsigned char* name(const DistParams& p, uint32_t r, uint32_t* nlen) {
        const uint64_t s = min(p.first_row + r, (uint64_t)p.n - 1);
        *nlen = (uint32_t)(p.name_off[s + 1] - p.name_off[s]);
        return p.names + p.name_off[s];
    }
    static __device__ __forceinline__ uint64_t row_cells(const DistParams& p, uint32_t r) { return min(p.first_row + r, (uint64_t)p.n); }
};

struct RowCells {
    // every cell of the piece is a cell of the rectangle: row = ci / n in 32 bits (a piece holds fewer than 2^31 cells; a 64-bit divide is a
    // long software sequence), the row's own count is a = row_counts[first_row + row], b = counts[col] as everywhere
    static __device__ Cell at(const DistParams& p, uint64_t ci) {
        Cell x{};
        const uint32_t c32 = (uint32_t)ci;
        const uint32_t row = min(c32 / p.n, p.R - 1);           // clamped to the piece
        const uint32_t col = min(c32 - row * p.n, p.n - 1);
        x.row = row;
        x.col = col;
        x.a = p.row_counts[min(p.first_row + row, p.rows_nq - 1)];
        x.count = p.cells[min(p.piece_lo + ci, p.cells_len - 1)];
        x.emit = p.mode != MODE_SPARSE_OUT || x.count > 0;
        x.prefix = p.mode == MODE_SPARSE_OUT ? col + 1 : 0;
        return x;
    }
    static __device__ __forceinline__ const unsigned char* name(const DistParams& p, uint32_t r, uint32_t* nlen) {
        const uint64_t s = min(p.first_row + r, p.rows_nq - 1);
        *nlen = (uint32_t)(p.name_off[s + 1] - p.name_off[s]);
        return p.names + p.name_off[s];
    }
    static __device__ __forceinline__ uint64_t row_cells(const DistParams& p, uint32_t) { return p.n; }
};

struct CsrCells {
    // every cell of the piece is an entry of the CSR: consecutive lanes read consecutive col / val; the row is the last one whose first entry is
    // at or below ci (64-bit offsets throughout: row_ptr, piece_lo and the entry index)
    static __device__ Cell at(const DistParams& p, uint64_t ci) {
        Cell x{};
        const uint64_t e = min(p.piece_lo + ci, p.csr_nnz - 1);   // clamped to the entries
        const uint32_t row = dev_row_of(p.oc, p.R, ci);
        const uint32_t col = min(p.csr_col[e], p.n - 1);            // (a column >= n is refused when the CSR is taken)
        x.row = row;
        x.col = col;
        x.a = p.row_counts[min(p.first_row + row, p.rows_nq - 1)];
        x.count = p.csr_val[e];
        x.emit = x.count > 0;                                       // (a stored zero is the pair "col:0" of the text: not written)
        x.prefix = col + 1;
        return x;
    }
    static __device__ __forceinline__ const unsigned char* name(const DistParams& p, uint32_t r, uint32_t* nlen) { return RowCells::name(p, r, nlen); }
    static __device__ __forceinline__ uint64_t row_cells(const DistParams& p, uint32_t r) {
        const uint64_t s = min(p.first_row + r, p.rows_nq - 1);     // clamped to the rows: row_ptr holds rows_nq + 1 values
        return p.csr_ptr[s + 1] - p.csr_ptr[s];
    }
};

// A lane per row of a piece whose cells lie in HBM, whatever the source: the row's output cells, and the bytes of its name, the separator
// behind it and the '\n'.  The host closes both arrays with a 0 and scans them in place.
template <class Source>
__global__ void __launch_bounds__(DT) dist_row_sizes_kernel(DistParams p) {
    const uint64_t r = (uint64_t)blockIdx.x * DT + threadIdx.x;
    if (r >= p.R) return;
    p.oc[r] = Source::row_cells(p, (uint32_t)r);
    uint32_t nlen = 0;
    (void)Source::name(p, (uint32_t)r, &nlen);
    p.rowfix[r] = (uint64_t)nlen + 2;
}

// what a CSR must be to be read without a fault: row_ptr ascending from 0 (a lane per row), every column below n (a lane per entry)
enum : unsigned int { CSR_BAD_PTR = 1, CSR_BAD_COL = 2 };
__global__ void __launch_bounds__(DT) dist_csr_check_kernel(const uint64_t* row_ptr, uint64_t nr, const uint32_t* col, uint64_t nnz, uint32_t n, unsigned int* bad,
                                                            unsigned int* bad_col) {
    const uint64_t i = (uint64_t)blockIdx.x * DT + threadIdx.x;
    if (i < nr && row_ptr[i] > row_ptr[i + 1]) atomicOr(bad, CSR_BAD_PTR);
    if (i == 0 && (row_ptr[0] != 0 || row_ptr[nr] != nnz)) atomicOr(bad, CSR_BAD_PTR);
    if (i < nnz && col[i] >= n) { atomicOr(bad, CSR_BAD_COL); atomicMax(bad_col, col[i]); }
}

// ---- the gather: the CSRs of the cells of a block row -> ONE CSR --------------------------------------------------------------------------
// merged row_ptr[r] = the sum over the cells of their row_ptr[r] (a sum of exclusive sums is the exclusive sum of the sums): a lane per row
__global__ void __launch_bounds__(DT) dist_gather_ptr_kernel(const uint64_t* const* cell_ptr, uint32_t n_cells, uint64_t nr, uint64_t* merged, uint64_t* base) {
    const uint64_t r = (uint64_t)blockIdx.x * DT + threadIdx.x;
    if (r > nr) return;
    uint64_t sum = 0;
    for (uint32_t c = 0; c < n_cells; ++c) sum += cell_ptr[c][r];
    merged[r] = sum;
    base[r] = sum;
}

// One cell into its place, a lane per ENTRY of the cell: its row by search of the cell's row_ptr (a row of 10^5 entries is 10^5 lanes, 10^5
// rows without entries are never visited), its place = where the cells before this one left the row (base[row]) + its rank in the cell's row,
// its column shifted by the samples of the earlier parts.  Consecutive lanes read and — inside a row — write consecutive words.
__global__ void __launch_bounds__(DT) dist_gather_copy_kernel(const uint64_t* ptr, const uint32_t* col, const uint32_t* val, uint64_t nr, uint64_t nnz, uint32_t shift,
                                                              const uint64_t* base, uint32_t* out_col, uint32_t* out_val, uint64_t out_nnz) {
    const uint64_t e = (uint64_t)blockIdx.x * DT + threadIdx.x;
    if (e >= nnz) return;
    const uint32_t r = dev_row_of(ptr, (uint32_t)nr, e);
    const uint64_t first = ptr[r];
    const uint64_t at = base[r] + (e >= first ? e - first : 0);
    if (at >= out_nnz) return;                                  // (cannot happen: the merged row_ptr is the sum of the cells')
    out_col[at] = col[e] + shift;
    out_val[at] = val[e];
}

// ... and the rows' places move behind it: a lane per row
__global__ void __launch_bounds__(DT) dist_gather_advance_kernel(const uint64_t* ptr, uint64_t nr, uint64_t* base) {
    const uint64_t r = (uint64_t)blockIdx.x * DT + threadIdx.x;
    if (r < nr) base[r] += ptr[r + 1] - ptr[r];
}

template <class Source>
__global__ void __launch_bounds__(DT) dist_measure_kernel(DistParams p) {
    const uint64_t ci = (uint64_t)blockIdx.x * DT + threadIdx.x;
    bool wrote = false, host = false;
    if (ci < p.n_cells) {
        const Cell x = Source::at(p, ci);
        uint64_t code = C_SKIP;
        uint32_t len = 0;
        if (x.emit) {
            const uint32_t b = p.counts[min(x.col, p.n - 1)];
            const int keep = x.prefix ? dev_bounds(p, x.count, x.a, b) : 1;         // the bounds belong to the sparse forms
            if (keep == 2) code = C_HOST;
            else if (keep == 1) {
                bool exact = true, zero_ok = true;
                const double v = x.zero ? 0.0 : dev_metric(p.measure, x.count, x.a, b, p.k, &exact, &zero_ok);
                code = dev_code(v, exact, zero_ok);
            }
            if (code == C_HOST) host = true;
            else if (code != C_SKIP) {
                wrote = true;
                len = (code & C_ZERO) ? 1 : ((code & C_NEG) ? 1 : 0) + dev_digits((code & C_X) / 1000000ull) + 7;
                if (x.prefix) len += dev_digits(x.prefix) + 1;
                len += 1;                                       // the separator behind the value
            }
        }
        p.code[ci] = code;
        p.len[ci] = (uint8_t)len;
    }
    const uint64_t mw = __ballot(wrote), mh = __ballot(host);
    if ((threadIdx.x & 63) == 0) {
        if (mw) atomicAdd(&p.counters[1], (unsigned long long)__popcll(mw));
        if (mh) atomicAdd(&p.counters[2], (unsigned long long)__popcll(mh));
    }
}

// ---- format -----------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ unsigned char* dev_put_uint(unsigned char* o, uint64_t v) {
    const uint32_t n = dev_digits(v);
    for (uint32_t i = n; i-- > 0;) { o[i] = (unsigned char)('0' + v % 10); v /= 10; }
    return o + n;
}

// where the cells of row r begin in the output: its name and the separator behind it in front of them
__device__ __forceinline__ uint64_t dev_cells_at(const DistParams& p, uint32_t r) { return p.rowfix[r] + (p.rowfix[r + 1] - p.rowfix[r] - 1); }

template <class Source>
__global__ void __launch_bounds__(DT) dist_write_kernel(DistParams p, unsigned char* out, uint64_t out_bytes, HostCell* host, uint64_t host_cap) {
    const uint64_t ci = (uint64_t)blockIdx.x * DT + threadIdx.x;
    if (ci >= p.n_cells) return;
    const uint64_t code = p.code[ci];
    if (code == C_SKIP) return;
    const Cell x = Source::at(p, ci);
    const uint64_t at = dev_cells_at(p, x.row) + p.off[ci];
    if (code == C_HOST) {
        const unsigned long long e = atomicAdd(&p.counters[3], 1ull);
        if (e < host_cap) host[e] = HostCell{ci, at, x.col, x.count, x.a, 0};
        return;
    }
    const uint32_t len = p.len[ci];
    if (at + len > out_bytes) return;                           // (cannot happen: the buffer has the scanned size)
    unsigned char* o = out + at;
    if (x.prefix) { o = dev_put_uint(o, x.prefix); *o++ = ':'; }
    if (code & C_ZERO) *o++ = '0';
    else {
        if (code & C_NEG) *o++ = '-';
        const uint64_t v = code & C_X;
        o = dev_put_uint(o, v / 1000000ull);
        *o++ = '.';
        uint32_t f = (uint32_t)(v % 1000000ull);
        for (int i = 5; i >= 0; --i) { o[i] = (unsigned char)('0' + f % 10u); f /= 10u; }
        o += 6;
    }
    *o = p.mode == MODE_PHYLIP ? ' ' : ',';
}

// a wave per row: the name, the separator behind it, the '\n' behind the row's cells
template <class Source>
__global__ void __launch_bounds__(DT) dist_names_kernel(DistParams p, unsigned char* out, uint64_t out_bytes) {
    const uint64_t r = ((uint64_t)blockIdx.x * DT + threadIdx.x) >> 6;
    const uint32_t lane = threadIdx.x & 63;
    if (r >= p.R) return;
    uint32_t nlen = 0;
    const unsigned char* name = Source::name(p, (uint32_t)r, &nlen);
    const uint64_t at = p.rowfix[r] + p.off[p.oc[r]];           // the row's first byte: the fixed bytes and the cells of the rows before
    const uint64_t nl = p.rowfix[r + 1] - 1 + p.off[p.oc[r + 1]];
    if (at + nlen + 1 > out_bytes || nl >= out_bytes) return;
    for (uint32_t q = lane; q < nlen; q += 64) out[at + q] = name[q];
    if (lane == 0) { out[at + nlen] = p.mode == MODE_PHYLIP ? ' ' : ','; out[nl] = '\n'; }
}

template <class T>
__global__ void dist_fill_kernel(T* a, uint64_t n, T v) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) a[i] = v;
}

const char* decline_text(unsigned int why) {
    switch (why) {
    case DECL_NO_COMMA: return "a line has no comma";
    case DECL_DIGITS:   return "a field has more than 10 digits";
    case DECL_CHAR:     return "a field holds a byte that is neither a digit nor a separator";
    case DECL_COLONS:   return "a ':' where the row rules know no pair";
    case DECL_PAIR:     return "a column:count pair in a table taken for dense";
    case DECL_PLAIN:    return "a plain cell in a table taken for sparse";
    default:            return "unknown";
    }
}

inline unsigned blocks_for(uint64_t n) { return (unsigned)std::max<uint64_t>(1, (n + DT - 1) / DT); }

}  // namespace

struct kmdb_distance {
    int device = 0;
    hipStream_t stream = nullptr;
    int measure = 0, k = 0, mode = MODE_DENSE, triangle = 0;
    uint32_t flags = 0;
    std::vector<uint32_t> counts;
    std::vector<kmdb_cell_filter> filters;
    DevBuf<uint32_t> d_counts;
    // the triangle taken as the source of cells (kmdb_distance_take_*): the handle's own (take_all2all) or the caller's (take_cells_device)
    bool taken = false;
    DevBuf<uint32_t> own_tri;
    const uint32_t* tri = nullptr;      // the first cell of row tri_row_lo; may be null when no row asked for holds a cell
    uint64_t tri_row_lo = 0;
    DevBuf<unsigned char> d_names;
    DevBuf<uint64_t> d_name_off;
    // the rows of a batch of queries taken as the source of cells (kmdb_distance_take_new2all_batch*: the handle's own buffer, kept between
    // takes and grown only for a larger batch; kmdb_distance_take_rows_device: the caller's)
    bool rows_taken = false;
    DevBuf<uint32_t> own_rows;
    const uint32_t* rows = nullptr;     // cell 0 of the nq x n rectangle; may be null when it holds no cell
    uint64_t rows_nq = 0;
    DevBuf<uint32_t> d_row_counts;      // [rows_nq] the queries' own counts
    DevBuf<unsigned char> d_qnames;
    DevBuf<uint64_t> d_qname_off;
    // a CSR taken as the source of cells: the caller's (kmdb_distance_take_csr_device) or the handle's own, gathered from the cells of a block row
    // (kmdb_distance_parts_*).  The row samples' counts and names share d_row_counts / d_qnames / d_qname_off with the query rows.
    bool csr_taken = false;
    bool parts_open = false;            // a block row was begun and its cells are not gathered yet
    const uint64_t* csr_ptr = nullptr;
    const uint32_t *csr_col = nullptr, *csr_val = nullptr;
    uint64_t csr_nr = 0, csr_nnz = 0;
    std::vector<uint64_t> csr_host_ptr; // [csr_nr + 1] the row_ptr on the host: the pieces' sizes
    DevBuf<uint64_t> own_ptr;
    DevBuf<uint32_t> own_col, own_val;
    struct PartCell { kmdb_csr_dev csr; uint32_t shift = 0; };
    std::vector<PartCell> parts;
    uint64_t parts_bytes = 0;           // the cells' CSRs held now
    kmdb_distance_stats st{};
    kmdb_distance_parts_stats pst{};
};

static int dist_splice(kmdb_distance* d, std::vector<HostCell>& cells, const char* dev_text, size_t dev_len, kmdb_distance_out* out, uint64_t* written);
static void dist_csr_drop(kmdb_distance* d);       // a take of another source drops the CSR: the row samples' arrays are shared

namespace {

// exclusive sum with the library's temporary storage
template <class In, class Out>
int dist_scan(In* in, Out* outp, size_t n, DevBuf<void>& d_tmp, uint64_t& held, hipStream_t st) {
    size_t tb = 0;
    HIP_TRY(prim::exclusive_sum(nullptr, tb, in, outp, n, st));
    if (tb > d_tmp.bytes()) { held += tb; DEV_ALLOC_BYTES(d_tmp, tb); }
    HIP_TRY(prim::exclusive_sum(d_tmp.get(), tb, in, outp, n, st));
    return 0;
}

struct DistTail {
    unsigned long long counters[4];
    uint64_t written, n_host;
    uint64_t held;              // dist_piece: the device bytes of the call
    float measure_ms, format_ms, copy_ms;
};

// what every piece takes from the handle, whatever the source of its cells: the columns and their counts, the form, the measure and the bounds
DistParams dist_params(const kmdb_distance* d, uint64_t first_row) {
    DistParams p{};
    p.n = (uint32_t)d->counts.size(); p.counts = d->d_counts; p.mode = d->mode; p.measure = d->measure; p.k = d->k; p.triangle = d->triangle; p.first_row = first_row;
    p.n_filters = (int)d->filters.size();
    for (int i = 0; i < p.n_filters; ++i) { p.f_metric[i] = d->filters[i].metric; p.f_lo[i] = d->filters[i].lo; p.f_hi[i] = d->filters[i].hi; }
    return p;
}

// The rows' sizes (p.oc and p.rowfix, a value per row) become their places: both closed with a 0 and scanned in place, the two totals back on
// the host.  `done` (may be null) is recorded behind the copies; the stream is synchronised once.
int dist_scan_rows(const DistParams& p, DevBuf<void>& d_tmp, uint64_t& held, hipStream_t st, hipEvent_t done, uint64_t* n_cells, uint64_t* fix_bytes) {
    HIP_TRY(hipMemsetAsync(p.oc + p.R, 0, 8, st));
    HIP_TRY(hipMemsetAsync(p.rowfix + p.R, 0, 8, st));
    if (dist_scan(p.oc, p.oc, (size_t)p.R + 1, d_tmp, held, st)) return 1;
    if (dist_scan(p.rowfix, p.rowfix, (size_t)p.R + 1, d_tmp, held, st)) return 1;
    HIP_TRY(hipMemcpyAsync(n_cells, p.oc + p.R, 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(fix_bytes, p.rowfix + p.R, 8, hipMemcpyDeviceToHost, st));
    if (done) HIP_TRY(hipEventRecord(done, st));
    HIP_TRY(hipStreamSynchronize(st));
    return 0;
}

// a call without rows returns a text of no bytes
int dist_empty_piece(const char* who, kmdb_distance_out* out) {
    out->text = (char*)malloc(1);
    if (!out->text) return kmdb_set_error(std::string(who) + "out of host memory");
    return 0;
}

// a piece into the handle's statistics (the call itself is counted where it begins)
void dist_account(kmdb_distance* d, uint32_t R, uint64_t cells_read, uint64_t bytes_in, uint64_t held, const DistTail& t, const kmdb_distance_out* out) {
    d->st.rows += R; d->st.cells_read += cells_read; d->st.cells_written += t.written; d->st.host_cells += t.n_host;
    d->st.bytes_in += bytes_in; d->st.bytes_out += out->len; d->st.device_bytes = std::max<uint64_t>(d->st.device_bytes, held);
    d->st.copy_ms += t.copy_ms; d->st.measure_ms += t.measure_ms; d->st.format_ms += t.format_ms;
}

// what the four *_rows entry points do around their work: the arguments, an `out` that is empty until the call succeeds, no exception outside
template <class Body>
int dist_rows_entry(const char* who, bool args_ok, kmdb_distance_out* out, Body&& body) {
    if (!args_ok) return kmdb_set_error(std::string(who) + "null argument");
    out->text = nullptr; out->len = 0; out->rows = 0;
    int rc;
    try {
        rc = body();
    } catch (const std::exception& e) {
        rc = kmdb_set_error(std::string(who) + e.what());
    }
    if (rc) kmdb_distance_out_free(out);
    return rc;
}

// The measure and format stages of a piece whose rows and cells are laid out (p.R, p.oc and p.rowfix scanned, p.n_cells, fix_bytes): whatever
// the source of the cells.  `begun` was recorded on the stream where the stages begin.  out->text and out->len are set.
template <class Source>
int dist_measure_format(kmdb_distance* d, const char* who, DistParams& p, uint64_t fix_bytes, DevBuf<void>& d_tmp, uint64_t& held, hipEvent_t begun,
                        kmdb_distance_out* out, DistTail* tail) {
    hipStream_t st = d->stream;
    const uint32_t R = p.R;
    const uint64_t n_cells = p.n_cells;
    DevEvent ev[3];
    for (auto& e : ev) if (e.create()) return 1;
    DevBuf<uint8_t> d_len;
    DevBuf<uint64_t> d_code, d_off;
    DevBuf<unsigned char> d_out;
    DevBuf<HostCell> d_host;

    // measure
    DEV_ALLOC(d_code, (size_t)n_cells); DEV_ALLOC(d_len, (size_t)n_cells + 1); DEV_ALLOC(d_off, (size_t)n_cells + 1);
    held += n_cells * 17;
    p.code = d_code; p.len = d_len; p.off = d_off;
    if (n_cells) {
        hipLaunchKernelGGL(dist_measure_kernel<Source>, dim3(blocks_for(n_cells)), dim3(DT), 0, st, p);
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipMemsetAsync(d_len.get() + n_cells, 0, 1, st));
    if (dist_scan(d_len.get(), d_off.get(), (size_t)n_cells + 1, d_tmp, held, st)) return 1;
    uint64_t cell_bytes = 0;
    unsigned long long* counters = tail->counters;
    HIP_TRY(hipMemcpyAsync(&cell_bytes, d_off.get() + n_cells, 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(counters, p.counters, 32, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipEventRecord(ev[0], st));
    HIP_TRY(hipStreamSynchronize(st));
    if (cell_bytes > n_cells * 64 || counters[2] > n_cells) return kmdb_set_error(std::string(who) + "internal error (the cells' text is longer than they can write)");

    // format
    const uint64_t out_bytes = fix_bytes + cell_bytes, n_host = counters[2];
    DEV_ALLOC(d_out, (size_t)out_bytes); DEV_ALLOC(d_host, (size_t)n_host);
    held += out_bytes + n_host * sizeof(HostCell);
    if (n_cells) hipLaunchKernelGGL(dist_write_kernel<Source>, dim3(blocks_for(n_cells)), dim3(DT), 0, st, p, d_out.get(), out_bytes, d_host.get(), n_host);
    hipLaunchKernelGGL(dist_names_kernel<Source>, dim3(blocks_for((uint64_t)R * 64)), dim3(DT), 0, st, p, d_out.get(), out_bytes);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(ev[1], st));
    char* text = (char*)malloc(std::max<uint64_t>(1, out_bytes));
    if (!text) return kmdb_set_error(std::string(who) + "out of host memory");
    std::vector<HostCell> cells;
    int rc = [&]() -> int {
        try { cells.resize(n_host); } catch (const std::exception&) { return kmdb_set_error(std::string(who) + "out of host memory"); }
        if (out_bytes) HIP_TRY(hipMemcpyAsync(text, d_out.get(), out_bytes, hipMemcpyDeviceToHost, st));
        if (n_host) HIP_TRY(hipMemcpyAsync(cells.data(), d_host.get(), n_host * sizeof(HostCell), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipEventRecord(ev[2], st));
        HIP_TRY(hipStreamSynchronize(st));
        return 0;
    }();
    tail->written = counters[1];
    tail->n_host = n_host;
    if (!rc) {
        if (n_host) {
            rc = dist_splice(d, cells, text, out_bytes, out, &tail->written);
            free(text);
        } else { out->text = text; out->len = out_bytes; }
    } else free(text);
    if (rc) return rc;
    HIP_TRY(hipEventElapsedTime(&tail->measure_ms, begun, ev[0]));
    HIP_TRY(hipEventElapsedTime(&tail->format_ms, ev[0], ev[1]));
    HIP_TRY(hipEventElapsedTime(&tail->copy_ms, ev[1], ev[2]));
    return 0;
}

// One piece of R >= 1 rows (row_lo and what follows) whose n_cells cells lie in HBM, from the check of its size to the handle's statistics.
// A Source says what the cells, the names and the rows' sizes are (at, name, row_cells); `fill` sets the fields of DistParams the Source reads.
// bytes_per_cell: what a cell counts for in the statistics' bytes_in.
template <class Source, class Fill>
int dist_piece(kmdb_distance* d, const char* who, uint64_t row_lo, uint32_t R, uint64_t n_cells, uint64_t bytes_per_cell, Fill&& fill, kmdb_distance_out* out, DistTail* tail) {
    if (n_cells >= (1ull << 31)) return kmdb_set_error(std::string(who) + "a piece of 2^31 cells or more (" + std::to_string(n_cells) + "): ask for fewer rows a call");
    HIP_TRY(hipSetDevice(d->device));
    hipStream_t st = d->stream;
    // the working arrays: code, length and offset of every cell, two sums per row; the text comes on top (DevBuf refuses with its own size)
    const uint64_t need = n_cells * 17 + 9 + ((uint64_t)R + 1) * 16 + 64;
    size_t mem_free = 0, mem_total = 0;
    HIP_TRY(hipMemGetInfo(&mem_free, &mem_total));
    if (need > mem_free) return kmdb_set_error(std::string(who) + "a piece of " + std::to_string(n_cells) + " cells needs " + std::to_string(need) + " B of working arrays on the device, "
                                              + std::to_string(mem_free) + " B are free: ask for fewer rows a call");
    uint64_t held = ((uint64_t)R + 1) * 16 + 32;                // (the cells' arrays and the text are counted where they are allocated)
    DevEvent begun;
    if (begun.create()) return 1;
    DevBuf<uint64_t> d_oc, d_rowfix;
    DevBuf<unsigned long long> d_counters;
    DevBuf<void> d_tmp;
    DEV_ALLOC(d_oc, (size_t)R + 1); DEV_ALLOC(d_rowfix, (size_t)R + 1); DEV_ALLOC(d_counters, 4);
    HIP_TRY(hipEventRecord(begun, st));
    HIP_TRY(hipMemsetAsync(d_counters.get(), 0, 32, st));
    DistParams p = dist_params(d, row_lo);
    p.R = R; p.n_cells = n_cells; p.counters = d_counters; p.oc = d_oc; p.rowfix = d_rowfix;
    fill(p);
    hipLaunchKernelGGL(dist_row_sizes_kernel<Source>, dim3(blocks_for(R)), dim3(DT), 0, st, p);
    HIP_TRY(hipGetLastError());
    uint64_t oc_all = 0, fix_bytes = 0;
    if (dist_scan_rows(p, d_tmp, held, st, nullptr, &oc_all, &fix_bytes)) return 1;
    if (oc_all != n_cells) return kmdb_set_error(std::string(who) + "internal error (the rows' cells do not add up to the piece)");
    if (dist_measure_format<Source>(d, who, p, fix_bytes, d_tmp, held, begun, out, tail)) return 1;
    out->rows = R;
    tail->held = held;
    dist_account(d, R, n_cells, n_cells * bytes_per_cell, held, *tail, out);
    return 0;
}

}  // namespace

extern "C" int kmdb_distance_begin(const kmdb_distance_opts* opts, kmdb_distance** out) {
    const char* who = "kmdb_distance_begin: ";
    if (!opts || !out) return kmdb_set_error(std::string(who) + "null argument");
    *out = nullptr;
    if (opts->abi_version && !kmdb_abi_compatible(opts->abi_version)) return kmdb_set_error(std::string(who) + "kmdb_distance_opts.abi_version is not served by this library");
    if (opts->measure < 0 || opts->measure >= KMDB_METRIC_COUNT) return kmdb_set_error(std::string(who) + "unknown measure " + std::to_string(opts->measure));
    if (opts->flags & ~KMDB_DISTANCE_FLAGS_ALL) return kmdb_set_error(std::string(who) + "unknown flags");
    if (opts->n_filters > KMDB_DISTANCE_MAX_FILTERS) return kmdb_set_error(std::string(who) + "more than " + std::to_string(KMDB_DISTANCE_MAX_FILTERS) + " bounds");
    if ((opts->n && !opts->counts) || (opts->n_filters && !opts->filters)) return kmdb_set_error(std::string(who) + "null argument");
    if (opts->n >= 0xFFFFFFFFull) return kmdb_set_error(std::string(who) + "2^32 - 1 columns or more");
    for (uint64_t i = 0; i < opts->n_filters; ++i)
        if (opts->filters[i].metric < 0 || opts->filters[i].metric >= KMDB_METRIC_COUNT) return kmdb_set_error(std::string(who) + "unknown criterion " + std::to_string(opts->filters[i].metric));
    if (kmdb_device_count() <= 0) return kmdb_set_error(std::string(who) + "no usable gfx950 device");
    kmdb_distance* d = new (std::nothrow) kmdb_distance;
    if (!d) return kmdb_set_error(std::string(who) + "out of host memory");
    int rc = 0;
    try {
        d->device = opts->device; d->stream = (hipStream_t)opts->stream; d->measure = opts->measure; d->k = (int)opts->kmer_length; d->flags = opts->flags;
        d->triangle = (opts->flags & KMDB_DISTANCE_TRIANGLE) ? 1 : 0;
        d->mode = (opts->flags & KMDB_DISTANCE_PHYLIP) ? MODE_PHYLIP : (opts->flags & KMDB_DISTANCE_SPARSE_IN) ? MODE_SPARSE_IN
                : (opts->flags & KMDB_DISTANCE_SPARSE_OUT) ? MODE_SPARSE_OUT : MODE_DENSE;
        d->counts.assign(opts->counts, opts->counts + opts->n);
        d->filters.assign(opts->filters, opts->filters + opts->n_filters);
        rc = [&]() -> int {
            HIP_TRY(hipSetDevice(d->device));
            DEV_ALLOC(d->d_counts, d->counts.size());
            if (!d->counts.empty()) HIP_TRY(hipMemcpy(d->d_counts.get(), d->counts.data(), d->counts.size() * 4, hipMemcpyHostToDevice));
            return 0;
        }();
    } catch (const std::exception& e) {
        rc = kmdb_set_error(std::string(who) + e.what());
    }
    if (rc) { delete d; return rc; }
    *out = d;
    return 0;
}

extern "C" void kmdb_distance_free(kmdb_distance* d) {
    if (!d) return;
    (void)hipSetDevice(d->device);
    delete d;
}

extern "C" void kmdb_distance_out_free(kmdb_distance_out* out) {
    if (!out) return;
    free(out->text);
    out->text = nullptr; out->len = 0; out->rows = 0;
}

extern "C" int kmdb_distance_stats_get(const kmdb_distance* d, kmdb_distance_stats* out) {
    if (!d || !out) return kmdb_set_error("kmdb_distance_stats_get: null argument");
    *out = d->st;
    return 0;
}

// the cells the device left open, in the order of the text: computed, bounded and formatted as the host loop does it, spliced in
static int dist_splice(kmdb_distance* d, std::vector<HostCell>& cells, const char* dev_text, size_t dev_len, kmdb_distance_out* out, uint64_t* written) {
    std::sort(cells.begin(), cells.end(), [](const HostCell& x, const HostCell& y) { return x.ci < y.ci; });
    char* text = (char*)malloc(std::max<size_t>(1, dev_len + cells.size() * 64));
    if (!text) return kmdb_set_error("kmdb_distance_rows: out of host memory");
    size_t o = 0, from = 0;
    const bool bounded = d->mode == MODE_SPARSE_OUT || d->mode == MODE_SPARSE_IN;
    for (const HostCell& c : cells) {
        const size_t at = (size_t)std::min<uint64_t>(c.off, dev_len);
        if (at > from) { std::memcpy(text + o, dev_text + from, at - from); o += at - from; from = at; }
        const uint32_t b = d->counts[c.col];
        bool keep = true;
        if (bounded)
            for (const kmdb_cell_filter& f : d->filters) {
                const double x = kmdbh_metric(f.metric, c.count, c.a, b, d->k);
                if (!(x >= f.lo && x <= f.hi)) { keep = false; break; }
            }
        if (!keep) continue;
        if (bounded) { o += (size_t)std::snprintf(text + o, 24, "%llu", (unsigned long long)c.col + 1); text[o++] = ':'; }
        o += kmdbh_format_measure(kmdbh_metric(d->measure, c.count, c.a, b, d->k), text + o);
        text[o++] = d->mode == MODE_PHYLIP ? ' ' : ',';
        ++*written;
    }
    std::memcpy(text + o, dev_text + from, dev_len - from);
    o += dev_len - from;
    out->text = text; out->len = o;
    return 0;
}

static int dist_rows(kmdb_distance* d, const char* lines, size_t len, uint64_t first_row, kmdb_distance_out* out) {
    const char* who = "kmdb_distance_rows: ";
    if (d->mode == MODE_PHYLIP && (d->flags & KMDB_DISTANCE_SPARSE_IN)) { kmdb_set_error(std::string(who) + "declined: phylip output from sparse input"); return KMDB_DISTANCE_DECLINED; }
    if (len >= 0xFFFFFFFFull - 64) { kmdb_set_error(std::string(who) + "declined: a piece of 2^32 - 64 bytes or more"); return KMDB_DISTANCE_DECLINED; }
    d->st.calls += 1;
    if (len == 0) return dist_empty_piece(who, out);
    HIP_TRY(hipSetDevice(d->device));
    hipStream_t st = d->stream;
    const uint32_t L = (uint32_t)len;
    const uint64_t NW = ((uint64_t)L + 63) / 64;
    uint64_t held = 0;
    DevEvent ev[3];
    for (auto& e : ev) if (e.create()) return 1;
    DevBuf<unsigned char> d_text;
    DevBuf<uint32_t> d_wcnt, d_weol, d_wsep, d_fc, d_row_end, d_row_first, d_sep_pos, d_sep_row, d_tok_val;
    DevBuf<uint8_t> d_tok_flags;
    DevBuf<uint64_t> d_oc, d_rowfix;
    DevBuf<unsigned int> d_decline;
    DevBuf<unsigned long long> d_counters;
    DevBuf<void> d_tmp;
    auto scan = [&](auto* in, auto* outp, size_t n) -> int { return dist_scan(in, outp, n, d_tmp, held, st); };

    HIP_TRY(hipEventRecord(ev[0], st));
    DEV_ALLOC(d_text, (size_t)L); DEV_ALLOC(d_wcnt, NW + 1); DEV_ALLOC(d_weol, NW + 1); DEV_ALLOC(d_wsep, NW + 1); DEV_ALLOC(d_decline, 1); DEV_ALLOC(d_counters, 4);
    held += L + 3 * (NW + 1) * 4;
    HIP_TRY(hipMemcpyAsync(d_text.get(), lines, L, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemsetAsync(d_decline.get(), 0, 4, st));
    HIP_TRY(hipMemsetAsync(d_counters.get(), 0, 32, st));
    HIP_TRY(hipMemsetAsync(d_wcnt.get(), 0, (NW + 1) * 4, st));
    HIP_TRY(hipEventRecord(ev[1], st));

    // classify: rows
    DistParams p = dist_params(d, first_row);
    p.text = d_text; p.L = L; p.decline = d_decline; p.counters = d_counters;
    hipLaunchKernelGGL(dist_eol_count_kernel, dim3(blocks_for(L)), dim3(DT), 0, st, (const unsigned char*)d_text.get(), L, d_wcnt.get());
    HIP_TRY(hipGetLastError());
    if (scan(d_wcnt.get(), d_weol.get(), NW + 1)) return 1;
    uint32_t n_eol = 0;
    HIP_TRY(hipMemcpyAsync(&n_eol, d_weol.get() + NW, 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (n_eol > L) return kmdb_set_error(std::string(who) + "internal error (more line ends than bytes)");
    const uint32_t R = n_eol + (lines[len - 1] != '\n' ? 1u : 0u);
    p.R = R; p.weol = d_weol;
    DEV_ALLOC(d_fc, (size_t)R); DEV_ALLOC(d_row_end, (size_t)R); DEV_ALLOC(d_row_first, (size_t)R + 1); DEV_ALLOC(d_oc, (size_t)R + 1); DEV_ALLOC(d_rowfix, (size_t)R + 1);
    held += (uint64_t)R * 28;
    p.fc = d_fc; p.row_end = d_row_end; p.row_first = d_row_first; p.oc = d_oc; p.rowfix = d_rowfix;
    hipLaunchKernelGGL(dist_fill_kernel<uint32_t>, dim3(blocks_for(R)), dim3(DT), 0, st, d_fc.get(), (uint64_t)R, NONE);
    hipLaunchKernelGGL(dist_fill_kernel<uint32_t>, dim3(blocks_for(R)), dim3(DT), 0, st, d_row_end.get(), (uint64_t)R, L);
    hipLaunchKernelGGL(dist_rows_kernel, dim3(blocks_for(L)), dim3(DT), 0, st, p);
    HIP_TRY(hipGetLastError());
    // classify: tokens
    HIP_TRY(hipMemsetAsync(d_wcnt.get(), 0, (NW + 1) * 4, st));
    hipLaunchKernelGGL(dist_sep_count_kernel, dim3(blocks_for(L)), dim3(DT), 0, st, p, d_wcnt.get());
    HIP_TRY(hipGetLastError());
    if (scan(d_wcnt.get(), d_wsep.get(), NW + 1)) return 1;
    uint32_t M = 0;
    HIP_TRY(hipMemcpyAsync(&M, d_wsep.get() + NW, 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (M > L) return kmdb_set_error(std::string(who) + "internal error (more separators than bytes)");
    p.M = M; p.wsep = d_wsep;
    const auto declined = [&](unsigned int why) {
        kmdb_set_error(std::string(who) + "declined: " + decline_text(why));
        return KMDB_DISTANCE_DECLINED;
    };
    if (M == 0) return declined(DECL_NO_COMMA);                 // (R >= 1 here: no row has a comma)
    DEV_ALLOC(d_sep_pos, (size_t)M); DEV_ALLOC(d_sep_row, (size_t)M); DEV_ALLOC(d_tok_val, (size_t)M); DEV_ALLOC(d_tok_flags, (size_t)M);
    held += (uint64_t)M * 13;
    p.sep_pos = d_sep_pos; p.sep_row = d_sep_row; p.tok_val = d_tok_val; p.tok_flags = d_tok_flags;
    hipLaunchKernelGGL(dist_fill_kernel<uint32_t>, dim3(blocks_for((uint64_t)R + 1)), dim3(DT), 0, st, d_row_first.get(), (uint64_t)R + 1, M);
    hipLaunchKernelGGL(dist_sep_write_kernel, dim3(blocks_for(L)), dim3(DT), 0, st, p);
    HIP_TRY(hipGetLastError());
    // parse
    hipLaunchKernelGGL(dist_text_row_sizes_kernel, dim3(blocks_for(R)), dim3(DT), 0, st, p);
    hipLaunchKernelGGL(dist_parse_kernel, dim3(blocks_for(M)), dim3(DT), 0, st, p);
    HIP_TRY(hipGetLastError());
    unsigned int why = 0;
    uint64_t n_cells = 0, fix_bytes = 0;
    HIP_TRY(hipMemcpyAsync(&why, d_decline.get(), 4, hipMemcpyDeviceToHost, st));      // (the two kernels that decline are on the stream)
    if (dist_scan_rows(p, d_tmp, held, st, ev[2], &n_cells, &fix_bytes)) return 1;
    if (why) return declined(why);
    if (fix_bytes > (uint64_t)L + 2ull * R) return kmdb_set_error(std::string(who) + "internal error (names longer than the text)");

    // measure and format
    p.n_cells = n_cells;
    DistTail t{};
    if (dist_measure_format<TextCells>(d, who, p, fix_bytes, d_tmp, held, ev[2], out, &t)) return 1;
    out->rows = R;
    float ms[2] = {0, 0};
    for (int i = 0; i < 2; ++i) HIP_TRY(hipEventElapsedTime(&ms[i], ev[i], ev[i + 1]));
    dist_account(d, R, t.counters[0], len, held, t, out);
    d->st.copy_ms += ms[0]; d->st.parse_ms += ms[1];           // the text's way to the device, and its classify and parse stages
    return 0;
}

extern "C" int kmdb_distance_rows(kmdb_distance* d, const char* lines, size_t len, uint64_t first_row, kmdb_distance_out* out) {
    return dist_rows_entry("kmdb_distance_rows: ", d && out && (!len || lines), out, [&] { return dist_rows(d, lines, len, first_row, out); });
}

// ---- the triangle as the source of cells -------------------------------------------------------------------------------------------------
static inline uint64_t tri_cells_before(uint64_t row) { return row ? row * (row - 1) / 2 : 0; }

static int dist_take_check(const kmdb_distance* d, const std::string& who) {
    if (!(d->flags & KMDB_DISTANCE_TRIANGLE)) return kmdb_set_error(who + "the handle was not begun with KMDB_DISTANCE_TRIANGLE: a matrix is a lower triangle");
    if (d->flags & KMDB_DISTANCE_SPARSE_IN) return kmdb_set_error(who + "the handle was begun with KMDB_DISTANCE_SPARSE_IN: a matrix holds no column:count pairs");
    return 0;
}

// the names to the device once: a blob and the offsets of its n + 1 ends
static int dist_names_to_device(kmdb_distance* d, const char* const* names, size_t n, DevBuf<unsigned char>& d_blob, DevBuf<uint64_t>& d_off, const std::string& who) {
    std::vector<uint64_t> off(n + 1, 0);
    for (size_t i = 0; i < n; ++i) {
        if (!names[i]) return kmdb_set_error(who + "null name");
        off[i + 1] = off[i] + std::strlen(names[i]);
    }
    std::string blob;
    blob.reserve((size_t)off[n]);
    for (size_t i = 0; i < n; ++i) blob.append(names[i]);
    HIP_TRY(hipSetDevice(d->device));
    DEV_ALLOC(d_blob, blob.size()); DEV_ALLOC(d_off, n + 1);
    if (!blob.empty()) HIP_TRY(hipMemcpy(d_blob.get(), blob.data(), blob.size(), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_off.get(), off.data(), (n + 1) * 8, hipMemcpyHostToDevice));
    return 0;
}
static int dist_take_names(kmdb_distance* d, const char* const* names, const std::string& who) {
    return dist_names_to_device(d, names, d->counts.size(), d->d_names, d->d_name_off, who);
}

extern "C" int kmdb_distance_take_all2all(kmdb_distance* d, kmdb_db* db, const char* const* names, const kmdb_opts* opts) {
    const std::string who = "kmdb_distance_take_all2all: ";
    if (!d || !db || (!names && !d->counts.empty())) return kmdb_set_error(who + "null argument");
    try {
        if (dist_take_check(d, who)) return 1;
        if (db->device != d->device) return kmdb_set_error(who + "the database lives on device " + std::to_string(db->device) + ", the handle on device " + std::to_string(d->device));
        if (db->N != d->counts.size()) return kmdb_set_error(who + "the database holds " + std::to_string(db->N) + " samples, the handle was begun with " + std::to_string(d->counts.size()));
        d->taken = false; d->tri = nullptr; d->tri_row_lo = 0;
        d->own_tri.reset();                                     // the triangle of the take before goes first
        if (dist_take_names(d, names, who)) return 1;
        DEV_ALLOC(d->own_tri, (size_t)std::max<uint64_t>(1, tri_cells_before(db->N)));
        kmdb_opts o{};
        if (opts) o = *opts;
        else { o.abi_version = KMDB_ABI_VERSION; o.shard_count = 1; }
        o.device = d->device;
        if (!o.stream) o.stream = d->stream;                    // (null still: the database's own stream, complete when the call returns)
        if (kmdb_all2all_dense_device(db, d->own_tri.get(), &o)) return 1;
        if (o.stream != (void*)d->stream) HIP_TRY(hipStreamSynchronize((hipStream_t)o.stream));
        d->tri = d->own_tri.get(); d->taken = true;
        return 0;
    } catch (const std::exception& e) {
        return kmdb_set_error(who + e.what());
    }
}

extern "C" int kmdb_distance_take_cells_device(kmdb_distance* d, const void* cells_dev, uint64_t row_lo, const char* const* names) {
    const std::string who = "kmdb_distance_take_cells_device: ";
    if (!d || (!names && !d->counts.empty())) return kmdb_set_error(who + "null argument");
    try {
        if (dist_take_check(d, who)) return 1;
        if (row_lo > d->counts.size()) return kmdb_set_error(who + "row_lo " + std::to_string(row_lo) + " lies behind the " + std::to_string(d->counts.size()) + " rows");
        d->taken = false; d->tri = nullptr; d->tri_row_lo = 0;
        d->own_tri.reset();
        if (dist_take_names(d, names, who)) return 1;
        d->tri = (const uint32_t*)cells_dev; d->tri_row_lo = row_lo; d->taken = true;
        return 0;
    } catch (const std::exception& e) {
        return kmdb_set_error(who + e.what());
    }
}

extern "C" const void* kmdb_distance_cells_device(const kmdb_distance* d) { return !d ? nullptr : d->taken ? d->tri : d->rows_taken ? d->rows : nullptr; }

static int dist_matrix_rows(kmdb_distance* d, uint64_t row_lo, uint64_t row_hi, kmdb_distance_out* out) {
    const char* who = "kmdb_distance_matrix_rows: ";
    const uint64_t n = d->counts.size();
    if (dist_take_check(d, who)) return 1;
    if (!d->taken) return kmdb_set_error(std::string(who) + "no matrix was taken (kmdb_distance_take_all2all, kmdb_distance_take_cells_device)");
    if (row_lo > row_hi) return kmdb_set_error(std::string(who) + "row_lo > row_hi");
    if (row_hi > n) return kmdb_set_error(std::string(who) + "row_hi " + std::to_string(row_hi) + " > " + std::to_string(n) + " rows");
    if (row_lo < row_hi && row_lo < d->tri_row_lo) return kmdb_set_error(std::string(who) + "row " + std::to_string(row_lo) + " lies in front of the cells taken (from row " + std::to_string(d->tri_row_lo) + " on)");
    d->st.calls += 1;
    if (row_lo == row_hi) return dist_empty_piece(who, out);
    const uint64_t n_cells = tri_cells_before(row_hi) - tri_cells_before(row_lo);
    if (n_cells && !d->tri) return kmdb_set_error(std::string(who) + "the rows hold " + std::to_string(n_cells) + " cells and a null pointer was taken");
    DistTail t{};
    return dist_piece<TriangleCells>(d, who, row_lo, (uint32_t)(row_hi - row_lo), n_cells, 4, [&](DistParams& p) {
        p.cells = d->tri; p.cells_lo = tri_cells_before(d->tri_row_lo); p.cells_len = tri_cells_before(n) - p.cells_lo; p.piece_lo = tri_cells_before(row_lo);
        p.names = d->d_names; p.name_off = d->d_name_off;
    }, out, &t);
}

extern "C" int kmdb_distance_matrix_rows(kmdb_distance* d, uint64_t row_lo, uint64_t row_hi, kmdb_distance_out* out) {
    return dist_rows_entry("kmdb_distance_matrix_rows: ", d && out, out, [&] { return dist_matrix_rows(d, row_lo, row_hi, out); });
}

// ---- the rows of a batch of queries as the source of cells -------------------------------------------------------------------------------
static int dist_rows_check(const kmdb_distance* d, const std::string& who) {
    if (d->flags & KMDB_DISTANCE_TRIANGLE) return kmdb_set_error(who + "the handle was begun with KMDB_DISTANCE_TRIANGLE: the rows of queries are whole rows");
    if (d->flags & KMDB_DISTANCE_SPARSE_IN) return kmdb_set_error(who + "the handle was begun with KMDB_DISTANCE_SPARSE_IN: the rows of queries hold no column:count pairs");
    return 0;
}

// what a take keeps besides the cells: the queries' own counts and their names
static int dist_take_queries(kmdb_distance* d, const uint32_t* a, size_t nq, const char* const* names, const std::string& who) {
    if (dist_names_to_device(d, names, nq, d->d_qnames, d->d_qname_off, who)) return 1;
    DEV_ALLOC(d->d_row_counts, nq);
    if (nq) HIP_TRY(hipMemcpy(d->d_row_counts.get(), a, nq * 4, hipMemcpyHostToDevice));
    return 0;
}

// One batch into the handle's own rectangle: zeroed on the handle's stream, filled by `fill` (kmdb_new2all_batch*_device, which returns when
// its last kernel has ended), a[q] = what fill reports as the query's count.
template <class Fill>
static int dist_take_batch(kmdb_distance* d, kmdb_db* db, size_t nq, const char* const* names, const kmdb_opts* opts, const std::string& who, Fill&& fill) {
    if (dist_rows_check(d, who)) return 1;
    kmdb_engine_view e;
    if (kmdb_engine_get(db, &e)) return 1;
    if (e.device != d->device) return kmdb_set_error(who + "the database lives on device " + std::to_string(e.device) + ", the handle on device " + std::to_string(d->device));
    if (e.N != d->counts.size()) return kmdb_set_error(who + "the database holds " + std::to_string(e.N) + " samples, the handle was begun with " + std::to_string(d->counts.size()));
    if (e.qs_count > 1) return kmdb_set_error(who + "a query shard holds partial sums and partial k-mer counts (sum the shards' rows with kmdb_new2all_batch_device and hand them to kmdb_distance_take_rows_device)");
    if (!e.n_buckets || !e.slots) return kmdb_set_error(who + "database was uploaded without hashtables");
    if (nq >= (1ull << 31)) return kmdb_set_error(who + "too many queries in one batch");
    d->rows_taken = false; d->rows = nullptr; d->rows_nq = 0; dist_csr_drop(d);
    HIP_TRY(hipSetDevice(d->device));
    const uint64_t cells = (uint64_t)nq * e.N;
    if (d->own_rows.bytes() < cells * 4 || !d->own_rows) DEV_ALLOC(d->own_rows, (size_t)std::max<uint64_t>(1, cells));
    if (cells) HIP_TRY(hipMemsetAsync(d->own_rows.get(), 0, cells * 4, d->stream));
    kmdb_opts o{};
    if (opts) o = *opts;
    else { o.abi_version = KMDB_ABI_VERSION; o.shard_count = 1; }
    o.device = d->device;
    if (!o.stream) o.stream = d->stream;                        // (null still: the database's own stream)
    const hipStream_t runs_on = o.stream ? (hipStream_t)o.stream : (hipStream_t)e.stream;
    if (runs_on != d->stream) HIP_TRY(hipStreamSynchronize(d->stream));     // the zeros first
    std::vector<uint32_t> a(std::max<size_t>(nq, 1), 0);
    if (fill(d->own_rows.get(), &o, a.data())) return 1;
    if (dist_take_queries(d, a.data(), nq, names, who)) return 1;
    d->rows = d->own_rows.get(); d->rows_nq = nq; d->rows_taken = true;
    return 0;
}

extern "C" int kmdb_distance_take_new2all_batch(kmdb_distance* d, kmdb_db* db, const uint64_t* const* kmers, const size_t* counts, size_t nq,
                                                const char* const* names, const kmdb_opts* opts) {
    const std::string who = "kmdb_distance_take_new2all_batch: ";
    if (!d || !db || (nq && (!kmers || !counts || !names))) return kmdb_set_error(who + "null argument");
    try {
        return dist_take_batch(d, db, nq, names, opts, who, [&](uint32_t* rows, const kmdb_opts* o, uint32_t* a) -> int {
            for (size_t q = 0; q < nq; ++q) a[q] = (uint32_t)counts[q];
            return kmdb_new2all_batch_device(db, kmers, counts, nq, rows, o);
        });
    } catch (const std::exception& e) {
        return kmdb_set_error(who + e.what());
    }
}

extern "C" int kmdb_distance_take_new2all_batch_seq_alphabet(kmdb_distance* d, kmdb_db* db, const char* const* seqs, const size_t* seq_lens, size_t nq,
                                                             double fraction, double start_fraction, int32_t alphabet, const char* const* names,
                                                             uint64_t* out_kmer_counts, const kmdb_opts* opts) {
    const std::string who = "kmdb_distance_take_new2all_batch_seq_alphabet: ";
    if (!d || !db || (nq && (!seqs || !seq_lens || !names || !out_kmer_counts))) return kmdb_set_error(who + "null argument");
    if (alphabet < 0 || alphabet >= KMDB_ALPHABET_COUNT) return kmdb_set_error(who + "unknown alphabet " + std::to_string(alphabet));
    try {
        return dist_take_batch(d, db, nq, names, opts, who, [&](uint32_t* rows, const kmdb_opts* o, uint32_t* a) -> int {
            // the query counts are the device extractor's unique counts
            if (kmdb_new2all_batch_seq_alphabet_device(db, seqs, seq_lens, nq, fraction, start_fraction, alphabet, rows, out_kmer_counts, o)) return 1;
            for (size_t q = 0; q < nq; ++q) a[q] = (uint32_t)out_kmer_counts[q];
            return 0;
        });
    } catch (const std::exception& e) {
        return kmdb_set_error(who + e.what());
    }
}

extern "C" int kmdb_distance_take_rows_device(kmdb_distance* d, const void* rows_dev, size_t nq, const uint32_t* query_kmers, const char* const* names) {
    const std::string who = "kmdb_distance_take_rows_device: ";
    if (!d || (nq && (!query_kmers || !names))) return kmdb_set_error(who + "null argument");
    try {
        if (dist_rows_check(d, who)) return 1;
        if (nq >= (1ull << 31)) return kmdb_set_error(who + "too many queries in one batch");
        d->rows_taken = false; d->rows = nullptr; d->rows_nq = 0; dist_csr_drop(d);
        HIP_TRY(hipSetDevice(d->device));
        if (dist_take_queries(d, query_kmers, nq, names, who)) return 1;
        d->rows = (const uint32_t*)rows_dev; d->rows_nq = nq; d->rows_taken = true;
        return 0;
    } catch (const std::exception& e) {
        return kmdb_set_error(who + e.what());
    }
}

static int dist_query_rows(kmdb_distance* d, uint64_t row_lo, uint64_t row_hi, kmdb_distance_out* out) {
    const char* who = "kmdb_distance_query_rows: ";
    const uint64_t n = d->counts.size();
    if (dist_rows_check(d, who)) return 1;
    if (!d->rows_taken) return kmdb_set_error(std::string(who) + "no rows were taken (kmdb_distance_take_new2all_batch, kmdb_distance_take_new2all_batch_seq_alphabet, kmdb_distance_take_rows_device)");
    if (row_lo > row_hi) return kmdb_set_error(std::string(who) + "row_lo > row_hi");
    if (row_hi > d->rows_nq) return kmdb_set_error(std::string(who) + "row_hi " + std::to_string(row_hi) + " > " + std::to_string(d->rows_nq) + " rows");
    d->st.calls += 1;
    if (row_lo == row_hi) return dist_empty_piece(who, out);
    const uint32_t R = (uint32_t)(row_hi - row_lo);
    const uint64_t n_cells = (uint64_t)R * n;
    if (n_cells && !d->rows) return kmdb_set_error(std::string(who) + "the rows hold " + std::to_string(n_cells) + " cells and a null pointer was taken");
    DistTail t{};
    return dist_piece<RowCells>(d, who, row_lo, R, n_cells, 4, [&](DistParams& p) {
        p.cells = d->rows; p.cells_lo = 0; p.cells_len = d->rows_nq * n; p.piece_lo = row_lo * n;
        p.names = d->d_qnames; p.name_off = d->d_qname_off; p.row_counts = d->d_row_counts; p.rows_nq = d->rows_nq;
    }, out, &t);
}

extern "C" int kmdb_distance_query_rows(kmdb_distance* d, uint64_t row_lo, uint64_t row_hi, kmdb_distance_out* out) {
    return dist_rows_entry("kmdb_distance_query_rows: ", d && out, out, [&] { return dist_query_rows(d, row_lo, row_hi, out); });
}

// ---- a CSR as the source of cells: a block row of the all2all-parts grid -----------------------------------------------------------------
static int dist_csr_check(const kmdb_distance* d, const std::string& who) {
    if (!(d->flags & KMDB_DISTANCE_SPARSE_OUT)) return kmdb_set_error(who + "the handle was not begun with KMDB_DISTANCE_SPARSE_OUT: the entries of a CSR are written as column:value pairs");
    if (d->flags & KMDB_DISTANCE_TRIANGLE) return kmdb_set_error(who + "the handle was begun with KMDB_DISTANCE_TRIANGLE: a CSR holds the entries it holds");
    if (d->flags & KMDB_DISTANCE_SPARSE_IN) return kmdb_set_error(who + "the handle was begun with KMDB_DISTANCE_SPARSE_IN: a CSR is no text of column:count pairs");
    if (d->flags & KMDB_DISTANCE_PHYLIP) return kmdb_set_error(who + "the handle was begun with KMDB_DISTANCE_PHYLIP: phylip output from sparse input is declined");
    return 0;
}

static void dist_csr_drop(kmdb_distance* d) {
    d->csr_taken = false; d->parts_open = false;
    d->csr_ptr = nullptr; d->csr_col = nullptr; d->csr_val = nullptr; d->csr_nr = 0; d->csr_nnz = 0;
    d->csr_host_ptr.clear();
    d->parts.clear(); d->parts_bytes = 0;
    dev_reset(d->own_ptr, d->own_col, d->own_val);
}

// the CSR at (row_ptr, col, val) becomes the source of cells once the device found it sound: row_ptr ascending from 0 to nnz, every column < n
static int dist_csr_adopt(kmdb_distance* d, const uint64_t* row_ptr, const uint32_t* col, const uint32_t* val, uint64_t nr, const std::string& who) {
    hipStream_t st = d->stream;
    const uint64_t n = d->counts.size();
    std::vector<uint64_t> h_ptr(nr + 1, 0);
    if (nr) {
        if (!row_ptr) return kmdb_set_error(who + std::to_string(nr) + " rows and a null row_ptr");
        HIP_TRY(hipMemcpyAsync(h_ptr.data(), row_ptr, (nr + 1) * 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
    }
    const uint64_t nnz = h_ptr[nr];
    if (nnz && (!col || !val)) return kmdb_set_error(who + "the rows hold " + std::to_string(nnz) + " entries and a null pointer was taken");
    if (nr) {
        DevBuf<unsigned int> d_bad;
        DEV_ALLOC(d_bad, 2);
        HIP_TRY(hipMemsetAsync(d_bad.get(), 0, 8, st));
        hipLaunchKernelGGL(dist_csr_check_kernel, dim3(blocks_for(std::max(nr, nnz))), dim3(DT), 0, st, row_ptr, nr, col, nnz, (uint32_t)n, d_bad.get(), d_bad.get() + 1);
        HIP_TRY(hipGetLastError());
        unsigned int bad[2] = {0, 0};
        HIP_TRY(hipMemcpyAsync(bad, d_bad.get(), 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        if (bad[0] & CSR_BAD_PTR) return kmdb_set_error(who + "row_ptr does not ascend from 0 to its last value");
        if (bad[0] & CSR_BAD_COL) return kmdb_set_error(who + "a column of the CSR (" + std::to_string(bad[1]) + ") is not below the " + std::to_string(n) + " columns the handle was begun with");
    }
    d->csr_ptr = row_ptr; d->csr_col = col; d->csr_val = val; d->csr_nr = nr; d->csr_nnz = nnz;
    d->csr_host_ptr = std::move(h_ptr);
    d->csr_taken = true;
    return 0;
}

extern "C" int kmdb_distance_parts_begin_rows(kmdb_distance* d, size_t nr, const uint32_t* row_kmers, const char* const* names) {
    const std::string who = "kmdb_distance_parts_begin_rows: ";
    if (!d || (nr && (!row_kmers || !names))) return kmdb_set_error(who + "null argument");
    try {
        if (dist_csr_check(d, who)) return 1;
        if (nr >= (1ull << 31)) return kmdb_set_error(who + "too many rows in one block row");
        HIP_TRY(hipSetDevice(d->device));
        dist_csr_drop(d);                                       // the block row before goes first
        if (dist_take_queries(d, row_kmers, nr, names, who)) return 1;
        d->rows_taken = false; d->rows = nullptr;               // (the row samples' arrays are shared with the query rows: one source at a time)
        d->rows_nq = nr; d->csr_nr = nr; d->parts_open = true;
        d->pst.block_rows += 1;
        return 0;
    } catch (const std::exception& e) {
        return kmdb_set_error(who + e.what());
    }
}

// what both adds ask of the handle and of a database
static int dist_parts_add_check(kmdb_distance* d, kmdb_db* db, uint64_t col_shift, const std::string& who, bool rows_side) {
    if (dist_csr_check(d, who)) return 1;
    if (!d->parts_open) return kmdb_set_error(who + "no block row is open (kmdb_distance_parts_begin_rows; the rows asked for close it)");
    kmdb_engine_view e;
    if (kmdb_engine_get(db, &e)) return 1;
    if (e.device != d->device) return kmdb_set_error(who + "the database lives on device " + std::to_string(e.device) + ", the handle on device " + std::to_string(d->device));
    if (e.qs_count > 1) return kmdb_set_error(who + "a query shard holds only its own buckets (upload the parts with kmdb_db_upload)");
    if (rows_side && e.N != d->csr_nr) return kmdb_set_error(who + "the row database holds " + std::to_string(e.N) + " samples, the block row was begun with " + std::to_string(d->csr_nr));
    if (!rows_side && col_shift + e.N > d->counts.size())
        return kmdb_set_error(who + "col_shift " + std::to_string(col_shift) + " + " + std::to_string(e.N) + " samples lie behind the " + std::to_string(d->counts.size()) + " columns the handle was begun with");
    return 0;
}

static int dist_parts_keep(kmdb_distance* d, kmdb_distance::PartCell&& cell) {
    const uint64_t bytes = (cell.csr.n_rows + 1) * 8 + cell.csr.nnz * 8;
    d->parts_bytes += bytes;
    d->pst.cells_in += cell.csr.nnz; d->pst.grid_cells += 1;
    d->pst.peak_bytes = std::max<uint64_t>(d->pst.peak_bytes, d->parts_bytes);
    d->parts.push_back(std::move(cell));
    return 0;
}

extern "C" int kmdb_distance_parts_add_db2db(kmdb_distance* d, kmdb_db* db_row, kmdb_db* db_col, uint64_t col_shift, const kmdb_opts* opts) {
    const std::string who = "kmdb_distance_parts_add_db2db: ";
    if (!d || !db_row || !db_col) return kmdb_set_error(who + "null argument");
    try {
        if (dist_parts_add_check(d, db_row, 0, who, true) || dist_parts_add_check(d, db_col, col_shift, who, false)) return 1;
        kmdb_opts o{};
        if (opts) o = *opts;
        else { o.abi_version = KMDB_ABI_VERSION; o.shard_count = 1; }
        o.device = d->device;
        kmdb_distance::PartCell cell;
        cell.shift = (uint32_t)col_shift;
        // (the library's out-of-memory error passes through: the caller evicts resident parts and repeats)
        if (kmdb_db2db_csr_device("kmdb_distance_parts_add_db2db", db_row, db_col, &cell.csr, &o)) return 1;
        return dist_parts_keep(d, std::move(cell));
    } catch (const std::exception& e) {
        return kmdb_set_error(who + e.what());
    }
}

extern "C" int kmdb_distance_parts_add_all2all(kmdb_distance* d, kmdb_db* db, uint64_t col_shift, const kmdb_opts* opts) {
    const std::string who = "kmdb_distance_parts_add_all2all: ";
    if (!d || !db) return kmdb_set_error(who + "null argument");
    try {
        if (dist_parts_add_check(d, db, 0, who, true) || dist_parts_add_check(d, db, col_shift, who, false)) return 1;
        kmdb_opts o{};
        if (opts) o = *opts;
        else { o.abi_version = KMDB_ABI_VERSION; o.shard_count = 1; }
        o.device = d->device;
        kmdb_distance::PartCell cell;
        cell.shift = (uint32_t)col_shift;
        if (kmdb_all2all_csr_device("kmdb_distance_parts_add_all2all", db, &cell.csr, &o)) return 1;
        return dist_parts_keep(d, std::move(cell));
    } catch (const std::exception& e) {
        return kmdb_set_error(who + e.what());
    }
}

extern "C" int kmdb_distance_parts_add_csr_device(kmdb_distance* d, const void* row_ptr_dev, const void* col_dev, const void* val_dev, uint64_t n_cols, uint64_t col_shift) {
    const std::string who = "kmdb_distance_parts_add_csr_device: ";
    if (!d) return kmdb_set_error(who + "null argument");
    try {
        if (dist_csr_check(d, who)) return 1;
        if (!d->parts_open) return kmdb_set_error(who + "no block row is open (kmdb_distance_parts_begin_rows; the rows asked for close it)");
        if (col_shift + n_cols > d->counts.size())
            return kmdb_set_error(who + "col_shift " + std::to_string(col_shift) + " + " + std::to_string(n_cols) + " columns lie behind the " + std::to_string(d->counts.size()) + " columns the handle was begun with");
        HIP_TRY(hipSetDevice(d->device));
        hipStream_t st = d->stream;
        const uint64_t nr = d->csr_nr;
        if (nr && !row_ptr_dev) return kmdb_set_error(who + std::to_string(nr) + " rows and a null row_ptr");
        kmdb_distance::PartCell cell;
        cell.shift = (uint32_t)col_shift;
        cell.csr.n_rows = nr;
        DEV_ALLOC_BYTES(cell.csr.row_ptr, (nr + 1) * 8);
        if (nr) HIP_TRY(hipMemcpyAsync(cell.csr.row_ptr.get(), row_ptr_dev, (nr + 1) * 8, hipMemcpyDeviceToDevice, st));
        else HIP_TRY(hipMemsetAsync(cell.csr.row_ptr.get(), 0, 8, st));
        uint64_t nnz = 0;
        HIP_TRY(hipMemcpyAsync(&nnz, (const uint64_t*)cell.csr.row_ptr.get() + nr, 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        if (nnz && (!col_dev || !val_dev)) return kmdb_set_error(who + "the rows hold " + std::to_string(nnz) + " entries and a null pointer was given");
        if (nnz >= (1ull << 40)) return kmdb_set_error(who + "row_ptr does not ascend from 0 to its last value");
        // the cell is checked where it was given (row_ptr ascending from 0, every column below n_cols) and then copied
        DevBuf<unsigned int> d_bad;
        DEV_ALLOC(d_bad, 2);
        HIP_TRY(hipMemsetAsync(d_bad.get(), 0, 8, st));
        if (nr) hipLaunchKernelGGL(dist_csr_check_kernel, dim3(blocks_for(std::max(nr, nnz))), dim3(DT), 0, st, (const uint64_t*)row_ptr_dev, nr, (const uint32_t*)col_dev, nnz,
                                   (uint32_t)n_cols, d_bad.get(), d_bad.get() + 1);
        HIP_TRY(hipGetLastError());
        unsigned int bad[2] = {0, 0};
        HIP_TRY(hipMemcpyAsync(bad, d_bad.get(), 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        if (bad[0] & CSR_BAD_PTR) return kmdb_set_error(who + "row_ptr does not ascend from 0 to its last value");
        if (bad[0] & CSR_BAD_COL) return kmdb_set_error(who + "a column of the cell (" + std::to_string(bad[1]) + ") is not below its " + std::to_string(n_cols) + " columns");
        cell.csr.nnz = nnz;
        DEV_ALLOC_BYTES(cell.csr.col, nnz * 4); DEV_ALLOC_BYTES(cell.csr.val, nnz * 4);
        if (nnz) {
            HIP_TRY(hipMemcpyAsync(cell.csr.col.get(), col_dev, nnz * 4, hipMemcpyDeviceToDevice, st));
            HIP_TRY(hipMemcpyAsync(cell.csr.val.get(), val_dev, nnz * 4, hipMemcpyDeviceToDevice, st));
            HIP_TRY(hipStreamSynchronize(st));
        }
        return dist_parts_keep(d, std::move(cell));
    } catch (const std::exception& e) {
        return kmdb_set_error(who + e.what());
    }
}

// the cells of the open block row -> the handle's own CSR; the cells' CSRs are freed
static int dist_parts_gather(kmdb_distance* d, const std::string& who) {
    HIP_TRY(hipSetDevice(d->device));
    hipStream_t st = d->stream;
    const uint64_t nr = d->csr_nr;
    const uint32_t nc = (uint32_t)d->parts.size();
    uint64_t nnz = 0;
    for (auto& c : d->parts) {
        if (c.csr.n_rows != nr) return kmdb_set_error(who + "internal error (a cell of " + std::to_string(c.csr.n_rows) + " rows in a block row of " + std::to_string(nr) + ")");
        nnz += c.csr.nnz;
    }
    DevEvent g0, g1;
    if (g0.create() || g1.create()) return 1;
    DevBuf<uint64_t> d_base;
    DevBuf<const uint64_t*> d_tab;
    DEV_ALLOC(d->own_ptr, (size_t)nr + 1); DEV_ALLOC(d->own_col, (size_t)nnz); DEV_ALLOC(d->own_val, (size_t)nnz);
    DEV_ALLOC(d_base, (size_t)nr + 1); DEV_ALLOC(d_tab, (size_t)std::max<uint32_t>(nc, 1));
    d->pst.peak_bytes = std::max<uint64_t>(d->pst.peak_bytes, d->parts_bytes + (nr + 1) * 16 + nnz * 8);
    std::vector<const uint64_t*> tab(std::max<uint32_t>(nc, 1), nullptr);
    for (uint32_t c = 0; c < nc; ++c) tab[c] = (const uint64_t*)d->parts[c].csr.row_ptr.get();
    HIP_TRY(hipEventRecord(g0, st));
    HIP_TRY(hipMemcpyAsync(d_tab.get(), tab.data(), tab.size() * sizeof(tab[0]), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(dist_gather_ptr_kernel, dim3(blocks_for(nr + 1)), dim3(DT), 0, st, (const uint64_t* const*)d_tab.get(), nc, nr, d->own_ptr.get(), d_base.get());
    for (uint32_t c = 0; c < nc; ++c) {
        const kmdb_csr_dev& x = d->parts[c].csr;
        if (!x.nnz) continue;
        hipLaunchKernelGGL(dist_gather_copy_kernel, dim3(blocks_for(x.nnz)), dim3(DT), 0, st, (const uint64_t*)x.row_ptr.get(), (const uint32_t*)x.col.get(),
                           (const uint32_t*)x.val.get(), nr, x.nnz, d->parts[c].shift, (const uint64_t*)d_base.get(), d->own_col.get(), d->own_val.get(), nnz);
        if (c + 1 < nc) hipLaunchKernelGGL(dist_gather_advance_kernel, dim3(blocks_for(nr)), dim3(DT), 0, st, (const uint64_t*)x.row_ptr.get(), nr, d_base.get());
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(g1, st));
    HIP_TRY(hipStreamSynchronize(st));                          // (tab and the cells live until here)
    float ms = 0;
    HIP_TRY(hipEventElapsedTime(&ms, g0, g1));
    d->pst.gather_ms += ms;
    d->parts.clear(); d->parts_bytes = 0; d->parts_open = false;
    if (dist_csr_adopt(d, d->own_ptr.get(), d->own_col.get(), d->own_val.get(), nr, who)) return 1;
    if (d->csr_nnz != nnz) { d->csr_taken = false; return kmdb_set_error(who + "internal error (the gathered rows do not add up to the cells)"); }
    return 0;
}

extern "C" int kmdb_distance_take_csr_device(kmdb_distance* d, const void* row_ptr_dev, const void* col_dev, const void* val_dev, size_t nr, const uint32_t* row_kmers,
                                             const char* const* names) {
    const std::string who = "kmdb_distance_take_csr_device: ";
    if (!d || (nr && (!row_kmers || !names))) return kmdb_set_error(who + "null argument");
    try {
        if (dist_csr_check(d, who)) return 1;
        if (nr >= (1ull << 31)) return kmdb_set_error(who + "too many rows in one block row");
        HIP_TRY(hipSetDevice(d->device));
        dist_csr_drop(d);
        if (dist_take_queries(d, row_kmers, nr, names, who)) return 1;
        d->rows_taken = false; d->rows = nullptr; d->rows_nq = nr;
        return dist_csr_adopt(d, (const uint64_t*)row_ptr_dev, (const uint32_t*)col_dev, (const uint32_t*)val_dev, nr, who);
    } catch (const std::exception& e) {
        return kmdb_set_error(who + e.what());
    }
}

// the source is there: taken, or gathered now from the cells of the open block row
static int dist_csr_ready(kmdb_distance* d, const std::string& who) {
    if (dist_csr_check(d, who)) return 1;
    if (d->parts_open) return dist_parts_gather(d, who);
    if (!d->csr_taken) return kmdb_set_error(who + "no CSR was taken (kmdb_distance_parts_begin_rows and its adds, kmdb_distance_take_csr_device)");
    return 0;
}

extern "C" int kmdb_distance_csr_device(kmdb_distance* d, const void** row_ptr_dev, const void** col_dev, const void** val_dev, uint64_t* nr) {
    const std::string who = "kmdb_distance_csr_device: ";
    if (!d || !row_ptr_dev || !col_dev || !val_dev || !nr) return kmdb_set_error(who + "null argument");
    try {
        if (dist_csr_ready(d, who)) return 1;
        *row_ptr_dev = d->csr_ptr; *col_dev = d->csr_col; *val_dev = d->csr_val; *nr = d->csr_nr;
        return 0;
    } catch (const std::exception& e) {
        return kmdb_set_error(who + e.what());
    }
}

extern "C" int kmdb_distance_csr_row_ptr(kmdb_distance* d, uint64_t* out) {
    const std::string who = "kmdb_distance_csr_row_ptr: ";
    if (!d || !out) return kmdb_set_error(who + "null argument");
    try {
        if (dist_csr_ready(d, who)) return 1;
        std::copy(d->csr_host_ptr.begin(), d->csr_host_ptr.end(), out);
        return 0;
    } catch (const std::exception& e) {
        return kmdb_set_error(who + e.what());
    }
}

extern "C" int kmdb_distance_parts_stats_get(const kmdb_distance* d, kmdb_distance_parts_stats* out) {
    if (!d || !out) return kmdb_set_error("kmdb_distance_parts_stats_get: null argument");
    *out = d->pst;
    return 0;
}

static int dist_csr_rows(kmdb_distance* d, uint64_t row_lo, uint64_t row_hi, kmdb_distance_out* out) {
    const char* who = "kmdb_distance_csr_rows: ";
    const uint64_t n = d->counts.size();
    if (dist_csr_check(d, who)) return 1;
    if (row_lo > row_hi) return kmdb_set_error(std::string(who) + "row_lo > row_hi");
    if (!d->parts_open && !d->csr_taken) return kmdb_set_error(std::string(who) + "no CSR was taken (kmdb_distance_parts_begin_rows and its adds, kmdb_distance_take_csr_device)");
    if (row_hi > d->csr_nr) return kmdb_set_error(std::string(who) + "row_hi " + std::to_string(row_hi) + " > " + std::to_string(d->csr_nr) + " rows");
    if (dist_csr_ready(d, who)) return 1;
    d->st.calls += 1;
    if (row_lo == row_hi) return dist_empty_piece(who, out);
    const uint64_t piece_lo = d->csr_host_ptr[row_lo], n_cells = d->csr_host_ptr[row_hi] - piece_lo;    // 64-bit offsets, as row_ptr holds them
    if (n_cells && n == 0) return kmdb_set_error(std::string(who) + "the rows hold " + std::to_string(n_cells) + " entries and the handle was begun with no column");
    DistTail t{};
    if (dist_piece<CsrCells>(d, who, row_lo, (uint32_t)(row_hi - row_lo), n_cells, 8, [&](DistParams& p) {
            p.csr_ptr = d->csr_ptr; p.csr_col = d->csr_col; p.csr_val = d->csr_val; p.csr_nnz = d->csr_nnz; p.piece_lo = piece_lo;
            p.names = d->d_qnames; p.name_off = d->d_qname_off; p.row_counts = d->d_row_counts; p.rows_nq = d->csr_nr;
        }, out, &t)) return 1;
    d->pst.cells_written += t.counters[1]; d->pst.host_cells += t.n_host;
    d->pst.peak_bytes = std::max<uint64_t>(d->pst.peak_bytes, (d->csr_ptr == d->own_ptr.get() ? (d->csr_nr + 1) * 8 + d->csr_nnz * 8 : 0) + t.held);
    return 0;
}

extern "C" int kmdb_distance_csr_rows(kmdb_distance* d, uint64_t row_lo, uint64_t row_hi, kmdb_distance_out* out) {
    return dist_rows_entry("kmdb_distance_csr_rows: ", d && out, out, [&] { return dist_csr_rows(d, row_lo, row_hi, out); });
}
