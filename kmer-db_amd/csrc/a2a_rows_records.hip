// a2a_rows_records.hip — a band of rows [row_lo, row_hi) of the all2all matrix through the block-record pipeline
// (kmdb_all2all_rows_records_device / kmdb_all2all_rows_records / kmdb_all2all_rows_records_stats_get, include/kmdb_amd.h).
//
// DEFINITION: bit for bit what kmdb_all2all_rows_device (a2a_rows.hip) writes for the same arguments: the cells [tri(row_lo), tri(row_hi)) of
// kmdb_all2all_dense_device.  The two tree forms (a2a_rows.hip, a2a_band.hip) walk the pattern tree and add cell by cell; this call hands the
// band to kmdb_blocks_run (a2a_blocks.hip) as a kmdb_band_desc: decode, emit and the sorts run whole, the apply stage — the matrix cores — runs
// the stream jobs, window runs, slice tiles and second-level tiles of the band's block rows alone and writes the cells of the band's rows
// relative to the band's first cell.  No triangle exists anywhere: the band is the call's only output.
// BAND EMIT (KMDB_BAND_EMIT; rr_run_emit): the second form of the same call.  The emit kernels write the records of the band's block rows alone, keyed
// relative to the band's first stream, on a state of its own per handle — the route of a collection beyond the whole-matrix pipeline's 2^22 block pairs, where
// the parent form has no key for a stream.  A band it refuses (its streams, the wide kernel's lists) comes from the tree form.
// What this file holds: the argument checks, which form a call takes, the fallback to the tree form where the pipeline cannot take the database or the
// band, and the statistics.
#include "device_common.h"
#include "engine_internal.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <string>

namespace {

uint64_t tri_h(uint64_t i) { return i ? i * (i - 1) / 2 : 0; }

// the geometry part of the band-emit statistics (a non-empty band of a handle whose width is set)
void be_geometry(kmdb_all2all_rows_band_emit_stats& be, const kmdb_band_geometry& g) {
    be.x_lo = g.x_lo; be.x_hi = g.x_hi; be.n_rows = g.n_rows; be.n_streams = g.n_streams; be.stream_base = g.stream_base;
}

// The call in its band-emit form (include/kmdb_amd.h, KMDB_HAS_ALL2ALL_BAND_EMIT): the whole-matrix state exists (it gave the width and the estimate)
// and either can take the database or refused it for its block pairs alone.  Every refusal comes before the caller's buffer is touched.
int rr_run_emit(const char* who, kmdb_db* db, uint32_t* out, uint64_t row_lo, uint64_t row_hi, const kmdb_opts* opts, hipStream_t st,
                kmdb_all2all_rows_records_stats rs, kmdb_all2all_rows_band_emit_stats be) {
    const uint64_t cell_lo = tri_h(row_lo), band_cells = rs.band_cells;
    const uint32_t flags = opts ? opts->flags : 0;
    if (kmdb_blocks_band_k1n_mode(db) == 1)
        return kmdb_set_error(std::string(who) + ": this handle was made under KMDB_K1N_MODE=1, whose narrow kernel writes the whole matrix itself; a band needs mode 0 or 2");
    kmdb_band_geometry g{};
    if (kmdbh_band_streams(db->N, db->width, row_lo, row_hi, &g)) return 1;
    be_geometry(be, g);
    rs.width = db->width; rs.x_lo = g.x_lo; rs.x_hi = g.x_hi;
    std::string refused = kmdb_blocks_band_refusal(db, &g);
    if (!refused.empty() && (flags & KMDB_FLAG_NO_FALLBACK)) return kmdb_set_error(std::string(who) + ": band emit unavailable: " + refused);
    HIP_TRY(hipEventRecord(db->ev[0], st));
    HIP_TRY(hipMemsetAsync(out, 0, band_cells * 4, st));
    if (refused.empty()) {
        if (kmdb_blocks_band_prepare(db, &g, band_cells)) return 1;
        HIP_TRY(hipEventRecord(db->ev[1], st));
        const kmdb_band_desc band{row_lo, row_hi, cell_lo, band_cells, true};
        if (kmdb_blocks_run(db, out, 0u, (uint32_t)db->P, st, &band)) return 1;
        const bool sized = db->last_call_sized;
        // (the state's arrays are made and grow inside calls: what is resident now — both states)
        const uint64_t now = kmdb_blocks_device_bytes(db);
        db->stats.device_bytes = db->stats.device_bytes - db->blocks_bytes_counted + now;
        db->blocks_bytes_counted = now;
        be.state_bytes = kmdb_blocks_band_state_bytes(db);
        if (db->band_fallback_reason.empty()) {
            HIP_TRY(hipEventRecord(db->ev[3], st));
            HIP_TRY(hipEventSynchronize(db->ev[3]));
            float all = 0, k0 = 0, k1n = 0, k1g = 0, k2 = 0;
            HIP_TRY(hipEventElapsedTime(&all, db->ev[0], db->ev[3]));
            HIP_TRY(hipEventElapsedTime(&k0, db->ev[1], db->ev_k[0]));
            HIP_TRY(hipEventElapsedTime(&k1n, db->ev_k[0], db->ev_k[1]));
            HIP_TRY(hipEventElapsedTime(&k1g, db->ev_k[1], db->ev_k[2]));
            HIP_TRY(hipEventElapsedTime(&k2, db->ev_k[2], db->ev_k[3]));
            const kmdb_blocks_band_info bi = kmdb_blocks_band_last(db, true);
            rs.path = KMDB_ROWS_RECORDS_PATH_RECORDS;
            rs.sized_call = sized ? 1u : 0u;
            rs.slices = bi.slices;
            rs.records = bi.records;
            const kmdb_blocks_band_units& u = bi.units;
            rs.jobs_total = u.jobs; rs.jobs_run = u.jobs_run; rs.runs_total = u.runs; rs.runs_run = u.runs_run;
            rs.slices_total = u.slices; rs.slices_run = u.slices_run; rs.tiles_total = u.tiles; rs.tiles_run = u.tiles_run;
            rs.units_total = u.jobs + u.runs + u.slices + u.tiles;
            rs.units_run = u.jobs_run + u.runs_run + u.slices_run + u.tiles_run;
            rs.k0_ms = k0; rs.k1n_ms = k1n; rs.k1g_ms = k1g; rs.k2_ms = k2; rs.kernel_ms = all;
            db->stats.kernel_ms = all;
            rs.peak_device_bytes = db->stats.device_bytes + band_cells * 4;
            db->rr_stats = rs;
            be.form = KMDB_BAND_EMIT_FORM_BAND;
            be.key_bits = bi.key_bits; be.row_mode = bi.row_mode; be.l2_on = bi.l2_on; be.attempts = bi.attempts;
            be.records = bi.records; be.est_records = bi.est_records;
            db->be_stats = be;
            return 0;
        }
        refused = db->band_fallback_reason;
        if (flags & KMDB_FLAG_NO_FALLBACK) return kmdb_set_error(std::string(who) + ": band emit unavailable: " + refused);
        // (the abandoned attempt's partial sums are zeroed by the tree call below)
    }
    if (std::getenv("KMDB_VERBOSE"))
        fprintf(stderr, "[kmdb] %s: band emit cannot take this band (%s): the band comes from kmdb_all2all_rows_device\n", who, refused.c_str());
    if (kmdb_all2all_rows_device(db, row_lo, row_hi, out, opts)) return 1;
    rs.path = KMDB_ROWS_RECORDS_PATH_TREE;
    rs.kernel_ms = db->stats.kernel_ms;
    rs.peak_device_bytes = db->stats.device_bytes + band_cells * 4;
    db->rr_stats = rs;
    be.form = KMDB_BAND_EMIT_FORM_NONE;
    db->be_stats = be;
    return 0;
}

int rr_run(const char* who, kmdb_db* db, uint32_t* out, uint64_t row_lo, uint64_t row_hi, const kmdb_opts* opts, hipStream_t st) {
    const uint64_t P = db->P;
    const uint64_t cell_lo = tri_h(row_lo), band_cells = tri_h(row_hi) - cell_lo;
    const uint32_t flags = opts ? opts->flags : 0;
    kmdb_all2all_rows_records_stats rs{};
    rs.band_cells = band_cells;
    rs.path = KMDB_ROWS_RECORDS_PATH_NONE;
    db->rr_stats = rs;
    db->be_stats = kmdb_all2all_rows_band_emit_stats{};
    if (!band_cells) return 0;                                      // an empty band: nothing is written (row 0 has no cell)
    if (P && !db->blocks_prepared) {
        if (kmdb_blocks_prepare(db)) return 1;
        db->blocks_bytes_counted = kmdb_blocks_device_bytes(db);
        db->stats.device_bytes += db->blocks_bytes_counted;
        db->stats.width = db->width;
    }
    // ---- which form the call takes (KMDB_BAND_EMIT, read once per handle): band emit — the records of the band's block rows alone, keyed relative to the
    // band, on the handle's second state (rr_run_emit) — or the parent form below: decode, emit and the sorts whole, the apply stage culled
    if (db->band_emit_mode == -2) {
        const char* e = std::getenv("KMDB_BAND_EMIT");
        db->band_emit_mode = (e && *e) ? (e[0] != '0' ? 1 : 0) : -1;
        const char* m = std::getenv("KMDB_BAND_MAX_STREAMS");        // (a test switch; 0 or no number: ignored)
        db->band_max_streams = (m && *m) ? std::strtoull(m, nullptr, 10) : 0;
    }
    kmdb_all2all_rows_band_emit_stats be{};
    be.whole_state_bytes = kmdb_blocks_whole_state_bytes(db);
    be.state_bytes = kmdb_blocks_band_state_bytes(db);
    db->be_stats = be;
    const bool beyond = db->fallback_reason == "too many block pairs";
    if (P && (db->band_emit_mode == 1 ? (beyond || db->fallback_reason.empty()) : db->band_emit_mode == -1 && beyond))
        return rr_run_emit(who, db, out, row_lo, row_hi, opts, st, rs, be);
    // (every refusal comes before the caller's buffer is touched)
    if (P && db->fallback_reason.empty() && kmdb_blocks_k1n_mode(db) == 1)
        return kmdb_set_error(std::string(who) + ": this handle was made under KMDB_K1N_MODE=1, whose narrow kernel writes the whole matrix itself; a band needs mode 0 or 2");
    if (P && !db->fallback_reason.empty() && (flags & KMDB_FLAG_NO_FALLBACK))
        return kmdb_set_error(std::string(who) + ": block-record pipeline unavailable: " + db->fallback_reason);
    HIP_TRY(hipEventRecord(db->ev[0], st));
    HIP_TRY(hipMemsetAsync(out, 0, band_cells * 4, st));
    if (!P) { HIP_TRY(hipStreamSynchronize(st)); return 0; }
    rs.width = db->width;
    rs.x_lo = (uint32_t)(row_lo / db->width); rs.x_hi = (uint32_t)((row_hi - 1) / db->width);
    if (db->fallback_reason.empty()) {
        HIP_TRY(hipEventRecord(db->ev[1], st));
        const kmdb_band_desc band{row_lo, row_hi, cell_lo, band_cells};
        if (kmdb_blocks_run(db, out, 0u, (uint32_t)P, st, &band)) return 1;
        const bool sized = db->last_call_sized;
        if (db->fallback_reason.empty()) {
            HIP_TRY(hipEventRecord(db->ev[3], st));
            HIP_TRY(hipEventSynchronize(db->ev[3]));
            float all = 0, k0 = 0, k1n = 0, k1g = 0, k2 = 0;
            HIP_TRY(hipEventElapsedTime(&all, db->ev[0], db->ev[3]));
            HIP_TRY(hipEventElapsedTime(&k0, db->ev[1], db->ev_k[0]));
            HIP_TRY(hipEventElapsedTime(&k1n, db->ev_k[0], db->ev_k[1]));
            HIP_TRY(hipEventElapsedTime(&k1g, db->ev_k[1], db->ev_k[2]));
            HIP_TRY(hipEventElapsedTime(&k2, db->ev_k[2], db->ev_k[3]));
            rs.path = KMDB_ROWS_RECORDS_PATH_RECORDS;
            rs.sized_call = sized ? 1u : 0u;
            rs.slices = kmdb_blocks_n_slices(db);
            rs.records = kmdb_blocks_last_counts(db).records;
            const kmdb_blocks_band_units u = kmdb_blocks_last_band_units(db);
            rs.jobs_total = u.jobs; rs.jobs_run = u.jobs_run; rs.runs_total = u.runs; rs.runs_run = u.runs_run;
            rs.slices_total = u.slices; rs.slices_run = u.slices_run; rs.tiles_total = u.tiles; rs.tiles_run = u.tiles_run;
            rs.units_total = u.jobs + u.runs + u.slices + u.tiles;
            rs.units_run = u.jobs_run + u.runs_run + u.slices_run + u.tiles_run;
            rs.k0_ms = k0; rs.k1n_ms = k1n; rs.k1g_ms = k1g; rs.k2_ms = k2; rs.kernel_ms = all;
            db->stats.kernel_ms = all;
            // (the pipeline's arrays grow inside calls: what is resident now)
            const uint64_t now = kmdb_blocks_device_bytes(db);
            db->stats.device_bytes = db->stats.device_bytes - db->blocks_bytes_counted + now;
            db->blocks_bytes_counted = now;
            rs.peak_device_bytes = db->stats.device_bytes + band_cells * 4;
            db->rr_stats = rs;
            kmdb_band_geometry g{};
            if (!kmdbh_band_streams(db->N, db->width, row_lo, row_hi, &g)) be_geometry(be, g);
            const kmdb_blocks_band_info wi = kmdb_blocks_band_last(db, false);
            be.form = KMDB_BAND_EMIT_FORM_WHOLE;
            be.key_bits = wi.key_bits; be.row_mode = wi.row_mode; be.l2_on = wi.l2_on; be.attempts = wi.attempts;
            be.records = rs.records; be.est_records = wi.est_records;
            be.whole_state_bytes = kmdb_blocks_whole_state_bytes(db);
            db->be_stats = be;
            return 0;
        }
        // (the abandoned attempt's partial sums are zeroed by the tree call below)
    }
    if (flags & KMDB_FLAG_NO_FALLBACK) return kmdb_set_error(std::string(who) + ": block-record pipeline unavailable: " + db->fallback_reason);
    if (std::getenv("KMDB_VERBOSE"))
        fprintf(stderr, "[kmdb] %s: the block-record pipeline cannot take this database (%s): the band comes from kmdb_all2all_rows_device\n", who, db->fallback_reason.c_str());
    if (kmdb_all2all_rows_device(db, row_lo, row_hi, out, opts)) return 1;
    rs.path = KMDB_ROWS_RECORDS_PATH_TREE;
    rs.kernel_ms = db->stats.kernel_ms;
    rs.peak_device_bytes = db->stats.device_bytes + band_cells * 4;
    db->rr_stats = rs;
    return 0;
}

}  // namespace

extern "C" int kmdb_all2all_rows_records_device(kmdb_db* db, uint64_t row_lo, uint64_t row_hi, void* out_cells_dev, const kmdb_opts* opts) {
    const char* who = "kmdb_all2all_rows_records_device";
    if (!db) return kmdb_set_error(std::string(who) + ": null argument");
    if (kmdb_band_check(who, db, row_lo, row_hi, opts)) return 1;
    const uint64_t band_cells = tri_h(row_hi) - tri_h(row_lo);
    if (!out_cells_dev && band_cells) return kmdb_set_error(std::string(who) + ": null argument");
    HIP_TRY(hipSetDevice(db->device));
    if (kmdb_band_check_bytes(who, band_cells, false)) return 1;
    hipStream_t st = (opts && opts->stream) ? (hipStream_t)opts->stream : db->stream;
    const int rc = rr_run(who, db, (uint32_t*)out_cells_dev, row_lo, row_hi, opts, st);
    kmdb_release_staging(db);
    return rc;
}

extern "C" int kmdb_all2all_rows_records(kmdb_db* db, uint64_t row_lo, uint64_t row_hi, uint32_t* out_cells_host, const kmdb_opts* opts) {
    const char* who = "kmdb_all2all_rows_records";
    if (!db) return kmdb_set_error(std::string(who) + ": null argument");
    if (kmdb_band_check(who, db, row_lo, row_hi, opts)) return 1;
    const uint64_t band_cells = tri_h(row_hi) - tri_h(row_lo);
    if (!out_cells_host && band_cells) return kmdb_set_error(std::string(who) + ": null argument");
    HIP_TRY(hipSetDevice(db->device));
    if (kmdb_band_check_bytes(who, band_cells, true)) return 1;
    DevBuf<uint32_t> band;
    DEV_ALLOC(band, std::max<uint64_t>(band_cells, 1));
    hipStream_t st = (opts && opts->stream) ? (hipStream_t)opts->stream : db->stream;
    int rc = rr_run(who, db, band, row_lo, row_hi, opts, st);
    if (!rc && band_cells && hipMemcpy(out_cells_host, band, band_cells * 4, hipMemcpyDeviceToHost) != hipSuccess)
        rc = kmdb_set_error(std::string(who) + ": copy back failed");
    band.reset();
    kmdb_release_staging(db);
    return rc;
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
