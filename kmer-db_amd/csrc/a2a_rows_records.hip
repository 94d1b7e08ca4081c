// a2a_rows_records.hip — a band of rows [row_lo, row_hi) of the all2all matrix through the block-record pipeline
// (kmdb_all2all_rows_records_device / kmdb_all2all_rows_records / kmdb_all2all_rows_records_stats_get, include/kmdb_amd.h).
//
// DEFINITION: bit for bit what kmdb_all2all_rows_device (a2a_rows.hip) writes for the same arguments: the cells [tri(row_lo), tri(row_hi)) of
// kmdb_all2all_dense_device.  The two tree forms (a2a_rows.hip, a2a_band.hip) walk the pattern tree and add cell by cell; this call hands the
// band to kmdb_blocks_run (a2a_blocks.hip) as a kmdb_band_desc: decode, emit and the sorts run whole, the apply stage — the matrix cores — runs
// the stream jobs, window runs, slice tiles and second-level tiles of the band's block rows alone and writes the cells of the band's rows
// relative to the band's first cell.  No triangle exists anywhere: the band is the call's only output.
// What this file holds: the argument checks, the fallback to the tree form where the pipeline cannot take the database, and the statistics.
#include "device_common.h"
#include "engine_internal.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <string>

namespace {

uint64_t tri_h(uint64_t i) { return i ? i * (i - 1) / 2 : 0; }

int rr_run(const char* who, kmdb_db* db, uint32_t* out, uint64_t row_lo, uint64_t row_hi, const kmdb_opts* opts, hipStream_t st) {
    const uint64_t P = db->P;
    const uint64_t cell_lo = tri_h(row_lo), band_cells = tri_h(row_hi) - cell_lo;
    const uint32_t flags = opts ? opts->flags : 0;
    kmdb_all2all_rows_records_stats rs{};
    rs.band_cells = band_cells;
    rs.path = KMDB_ROWS_RECORDS_PATH_NONE;
    db->rr_stats = rs;
    if (!band_cells) return 0;                                      // an empty band: nothing is written (row 0 has no cell)
    if (P && !db->blocks_prepared) {
        if (kmdb_blocks_prepare(db)) return 1;
        db->blocks_bytes_counted = kmdb_blocks_device_bytes(db);
        db->stats.device_bytes += db->blocks_bytes_counted;
        db->stats.width = db->width;
    }
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

extern "C" int kmdb_all2all_rows_records_stats_get(const kmdb_db* db, kmdb_all2all_rows_records_stats* out) {
    if (!db || !out) return kmdb_set_error("kmdb_all2all_rows_records_stats_get: null argument");
    *out = db->rr_stats;
    return 0;
}
