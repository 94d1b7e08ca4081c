// a2a_rows_records.hip — a band of rows [row_lo, row_hi) of the all2all matrix through the block-record pipeline
// (kmdb_all2all_rows_records_device / kmdb_all2all_rows_records / kmdb_all2all_rows_records_stats_get, include/kmdb_amd.h).
//
// DEFINITION: bit for bit what kmdb_all2all_rows_device (a2a_rows.hip) writes for the same arguments: the cells [tri(row_lo), tri(row_hi)) of
// kmdb_all2all_dense_device.  The two tree forms (a2a_rows.hip, a2a_band.hip) walk the pattern tree and add cell by cell; this call hands the
// band to kmdb_blocks_run (a2a_blocks.hip) as a kmdb_band_desc: decode, emit and the sorts run whole, the apply stage — the matrix cores — runs
// the stream jobs, window runs, slice tiles and second-level tiles of the band's block rows alone and writes the cells of the band's rows
// relative to the band's first cell.  No triangle exists anywhere: the band is the call's only output.
// BAND EMIT (KMDB_BAND_EMIT): the second form of the same call.  The emit kernels write the records of the band's block rows alone, keyed
// relative to the band's first stream, on a state of its own per handle — the route of a collection beyond the whole-matrix pipeline's 2^22 block pairs, where
// the parent form has no key for a stream.  A band it refuses (its streams, the wide kernel's lists) comes from the tree form.
// What this file holds: rr_run — which form a call takes, its refusals, the run on that form's state —, rr_finish — the statistics of a call that went
// through the pipeline, on either state — and rr_from_tree — the fallback to the tree form where the pipeline cannot take the database or the band.
// The argument checks are kmdb_band_call's (a2a_rows.hip).
#include "device_common.h"
#include "engine_internal.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <string>

namespace {

// the geometry part of the band-emit statistics (a non-empty band of a handle whose width is set)
void be_geometry(kmdb_all2all_rows_band_emit_stats& be, const kmdb_band_geometry& g) {
    be.x_lo = g.x_lo; be.x_hi = g.x_hi; be.n_rows = g.n_rows; be.n_streams = g.n_streams; be.stream_base = g.stream_base;
}

// A call that went through the pipeline, on the band-emit state (emit) or the whole-matrix state: the events to stage times, what the state ran to both
// statistics, the pipeline's device bytes counted again.  rs, be: as rr_run filled them so far.
int rr_finish(kmdb_db* db, hipStream_t st, bool emit, uint64_t row_lo, uint64_t row_hi, bool sized, kmdb_all2all_rows_records_stats rs,
              kmdb_all2all_rows_band_emit_stats be) {
    HIP_TRY(hipEventRecord(db->ev[3], st));
    HIP_TRY(hipEventSynchronize(db->ev[3]));
    float all = 0, k[4];
    HIP_TRY(hipEventElapsedTime(&all, db->ev[0], db->ev[3]));
    if (kmdb_blocks_stage_ms(db, k)) return 1;
    const kmdb_blocks_band_info bi = kmdb_blocks_band_last(db, emit);
    rs.path = KMDB_ROWS_RECORDS_PATH_RECORDS;
    rs.sized_call = sized ? 1u : 0u;
    rs.slices = bi.slices;
    rs.records = bi.records;
    const kmdb_blocks_band_units& u = bi.units;
    rs.jobs_total = u.jobs; rs.jobs_run = u.jobs_run; rs.runs_total = u.runs; rs.runs_run = u.runs_run;
    rs.slices_total = u.slices; rs.slices_run = u.slices_run; rs.tiles_total = u.tiles; rs.tiles_run = u.tiles_run;
    rs.units_total = u.jobs + u.runs + u.slices + u.tiles;
    rs.units_run = u.jobs_run + u.runs_run + u.slices_run + u.tiles_run;
    rs.k0_ms = k[0]; rs.k1n_ms = k[1]; rs.k1g_ms = k[2]; rs.k2_ms = k[3]; rs.kernel_ms = all;
    db->stats.kernel_ms = all;
    // (the pipeline's arrays are made and grow inside calls: what is resident now — both states)
    kmdb_recount_bytes(db, db->blocks_bytes_counted, kmdb_blocks_device_bytes(db));
    rs.peak_device_bytes = db->stats.device_bytes + rs.band_cells * 4;
    db->rr_stats = rs;
    if (!emit) {                                                    // (band emit: rr_run had the geometry before the run; its own state's bytes after it)
        kmdb_band_geometry g{};
        if (!kmdbh_band_streams(db->N, db->width, row_lo, row_hi, &g)) be_geometry(be, g);
        be.whole_state_bytes = kmdb_blocks_state_bytes(db, false);
    }
    be.form = emit ? KMDB_BAND_EMIT_FORM_BAND : KMDB_BAND_EMIT_FORM_WHOLE;
    be.key_bits = bi.key_bits; be.row_mode = bi.row_mode; be.l2_on = bi.l2_on; be.attempts = bi.attempts;
    be.records = bi.records; be.est_records = bi.est_records;
    db->be_stats = be;
    return 0;
}

// The band from the tree form (what the pipeline may have left in `out` is zeroed by that call).  be.form stays KMDB_BAND_EMIT_FORM_NONE.
int rr_from_tree(kmdb_db* db, uint32_t* out, uint64_t row_lo, uint64_t row_hi, const kmdb_opts* opts, kmdb_all2all_rows_records_stats rs,
                 const kmdb_all2all_rows_band_emit_stats& be) {
    if (kmdb_all2all_rows_device(db, row_lo, row_hi, out, opts)) return 1;
    rs.path = KMDB_ROWS_RECORDS_PATH_TREE;
    rs.kernel_ms = db->stats.kernel_ms;
    rs.peak_device_bytes = db->stats.device_bytes + rs.band_cells * 4;
    db->rr_stats = rs;
    db->be_stats = be;
    return 0;
}

int rr_run(const char* who, kmdb_db* db, uint32_t* out, uint64_t row_lo, uint64_t row_hi, const kmdb_opts* opts, hipStream_t st) {
    const uint64_t P = db->P;
    const uint64_t cell_lo = kmdb_tri(row_lo), band_cells = kmdb_tri(row_hi) - cell_lo;
    const bool no_fallback = opts && (opts->flags & KMDB_FLAG_NO_FALLBACK);
    kmdb_all2all_rows_records_stats rs{};
    rs.band_cells = band_cells;
    rs.path = KMDB_ROWS_RECORDS_PATH_NONE;
    db->rr_stats = rs;
    db->be_stats = kmdb_all2all_rows_band_emit_stats{};
    if (!band_cells) return 0;                                      // an empty band: nothing is written (row 0 has no cell)
    if (P && kmdb_blocks_ensure_prepared(db)) return 1;
    // ---- which form the call takes (KMDB_BAND_EMIT, read once per handle): band emit — the records of the band's block rows alone, keyed relative to the
    // band, on the handle's second state — or the parent form: decode, emit and the sorts whole, the apply stage culled
    if (db->band_emit_mode == -2) {
        const char* e = std::getenv("KMDB_BAND_EMIT");
        db->band_emit_mode = (e && *e) ? (e[0] != '0' ? 1 : 0) : -1;
        const char* m = std::getenv("KMDB_BAND_MAX_STREAMS");        // (a test switch; 0 or no number: ignored)
        db->band_max_streams = (m && *m) ? std::strtoull(m, nullptr, 10) : 0;
    }
    kmdb_all2all_rows_band_emit_stats be{};
    be.whole_state_bytes = kmdb_blocks_state_bytes(db, false);
    be.state_bytes = kmdb_blocks_state_bytes(db, true);
    db->be_stats = be;
    const bool beyond = db->fallback_reason == "too many block pairs";
    const bool emit = P && (db->band_emit_mode == 1 ? (beyond || db->fallback_reason.empty()) : db->band_emit_mode == -1 && beyond);
    const std::string unavailable = std::string(who) + (emit ? ": band emit unavailable: " : ": block-record pipeline unavailable: ");
    // ---- the refusals: every one comes before the caller's buffer is touched.  refused: why the pipeline will not run this band ("": it will) — the band
    // itself under band emit (its streams, the wide kernel's lists), the database in the parent form
    if (P && (emit || db->fallback_reason.empty()) && kmdb_blocks_k1n_mode(db, emit) == 1)
        return kmdb_set_error(std::string(who) + ": this handle was made under KMDB_K1N_MODE=1, whose narrow kernel writes the whole matrix itself; a band needs mode 0 or 2");
    kmdb_band_geometry g{};
    std::string refused;
    if (emit) {
        if (kmdbh_band_streams(db->N, db->width, row_lo, row_hi, &g)) return 1;
        be_geometry(be, g);
        rs.width = db->width; rs.x_lo = g.x_lo; rs.x_hi = g.x_hi;
        refused = kmdb_blocks_band_refusal(db, &g);
    } else if (P) refused = db->fallback_reason;
    if (!refused.empty() && no_fallback) return kmdb_set_error(unavailable + refused);
    HIP_TRY(hipEventRecord(db->ev[0], st));
    HIP_TRY(hipMemsetAsync(out, 0, band_cells * 4, st));
    if (!P) { HIP_TRY(hipStreamSynchronize(st)); return 0; }
    if (!emit) {
        rs.width = db->width;
        rs.x_lo = (uint32_t)(row_lo / db->width); rs.x_hi = (uint32_t)((row_hi - 1) / db->width);
    }
    // ---- the run, on the form's state; a give-up inside it is the form's reason on the handle when the call returns
    if (refused.empty()) {
        if (emit && kmdb_blocks_band_prepare(db, &g, band_cells)) return 1;
        HIP_TRY(hipEventRecord(db->ev[1], st));
        const kmdb_band_desc band{row_lo, row_hi, cell_lo, band_cells, emit};
        if (kmdb_blocks_run(db, out, 0u, (uint32_t)P, st, &band)) return 1;
        const bool sized = db->last_call_sized;
        if (emit) {                                                 // (its state was made or made anew for this band, whatever became of the run)
            kmdb_recount_bytes(db, db->blocks_bytes_counted, kmdb_blocks_device_bytes(db));
            be.state_bytes = kmdb_blocks_state_bytes(db, true);
        }
        refused = emit ? db->band_fallback_reason : db->fallback_reason;
        if (refused.empty()) return rr_finish(db, st, emit, row_lo, row_hi, sized, rs, be);
        if (no_fallback) return kmdb_set_error(unavailable + refused);
    }
    if (std::getenv("KMDB_VERBOSE"))
        fprintf(stderr, "[kmdb] %s: %s (%s): the band comes from kmdb_all2all_rows_device\n", who,
                emit ? "band emit cannot take this band" : "the block-record pipeline cannot take this database", refused.c_str());
    return rr_from_tree(db, out, row_lo, row_hi, opts, rs, be);
}

}  // namespace

extern "C" int kmdb_all2all_rows_records_device(kmdb_db* db, uint64_t row_lo, uint64_t row_hi, void* out_cells_dev, const kmdb_opts* opts) {
    return kmdb_band_call("kmdb_all2all_rows_records_device", db, row_lo, row_hi, out_cells_dev, false, opts, rr_run);
}
extern "C" int kmdb_all2all_rows_records(kmdb_db* db, uint64_t row_lo, uint64_t row_hi, uint32_t* out_cells_host, const kmdb_opts* opts) {
    return kmdb_band_call("kmdb_all2all_rows_records", db, row_lo, row_hi, out_cells_host, true, opts, rr_run);
}

extern "C" int kmdb_all2all_rows_band_emit_stats_get(const kmdb_db* db, kmdb_all2all_rows_band_emit_stats* out) {
    if (!db || !out) return kmdb_set_error("kmdb_all2all_rows_band_emit_stats_get: null argument");
    *out = db->be_stats;
    return 0;
}

extern "C" int kmdb_all2all_rows_records_stats_get(const kmdb_db* db, kmdb_all2all_rows_records_stats* out) {
    if (!db || !out) return kmdb_set_error("kmdb_all2all_rows_records_stats_get: null argument");
    *out = db->rr_stats;
    return 0;
}
