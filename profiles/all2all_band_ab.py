"""A/B of the tiled band call (kmdb_all2all_rows_tiled_device: rows summed in LDS tiles) against the band call of the parent commit
(kmdb_all2all_rows_device: one HBM atomic per cell addition), and of the banded sparse run against the whole one.  README has the figures.

    python profiles/all2all_band_ab.py --inputs clade256,c3part --out profiles/all2all_band_ab.json

Inputs, both through kmer-db_amd/synth.py, each uploaded once:

    clade256   synth.CladeGenomes 256 x 1 Mbp, clades of 16; the band is the last 16 samples
    c3part     bench.py's c3part parameters (10 000 x 300 kbp, clades of 50); the bands are the last 100 samples and 100 rows in the middle

Arms on the same handle, in one process, each timed with the wall clock around the call (every call ends with its own wait) and with
kmdb_stats.kernel_ms:

    a        kmdb_all2all_rows_device                                                  the parent commit
    b16k     kmdb_all2all_rows_tiled_device, KMDB_ROWS_TILE_COLS=16384                 this commit
    bmax     the same, KMDB_ROWS_TILE_COLS=40896 (the largest tile 160 KiB of LDS take)
    (--tile-cols adds arms at other tile widths, --tile-hits arms b16k at other KMDB_ROWS_TILE_HITS)
    c        c3part only: kmdb_all2all_sparse_filtered_banded with R = 1000 against kmdb_all2all_sparse_filtered (no bounds)

The outputs are compared first (cell for cell; row_ptr, col, val for c).  Then one warm-up round and --runs rounds (5) in which the arms
ALTERNATE.  The json gives every run, the median and the spread (min, max) per arm, the tiled call's stats (hits, jobs, runs, updates, stage
times), the peak device bytes, and whether an arm lies below arm a beyond the spread of both.  No ratio is a condition."""
import argparse
import contextlib
import importlib
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

INPUTS = {"clade256": dict(samples=256, clade_size=16, length=1_000_000, bands={"last": (240, 256)}, banded=0),
          "c3part": dict(samples=10000, clade_size=50, length=300_000, bands={"last": (9900, 10000), "middle": (5000, 5100)}, banded=1000)}
TILE_MAX = 40896


def log(msg):
    print(msg, file=sys.stderr, flush=True)


def tri(i):
    return i * (i - 1) // 2 if i else 0


@contextlib.contextmanager
def switches(cols, hits):
    keys = {"KMDB_ROWS_TILE_COLS": cols, "KMDB_ROWS_TILE_HITS": hits}
    old = {k: os.environ.get(k) for k in keys}
    try:
        for k, v in keys.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = str(v)
        yield
    finally:
        for k, v in old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def summary(runs_of):
    out = {}
    for which, runs in runs_of.items():
        for key in ("wall_ms", "kernel_ms"):
            v = [o[key] for o in runs]
            out.setdefault(which, {})[key] = {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}
        out[which]["peak_device_bytes"] = max(o["peak_device_bytes"] for o in runs)
    return out


def one_band(d, torch, device, dev, name, lo, hi, arms, runs):
    band_buf = torch.empty(max(1, tri(hi) - tri(lo)), dtype=torch.int32, device=device)
    torch.cuda.synchronize(dev)

    def arm(which):
        cols, hits = arms[which]
        t1 = time.perf_counter()
        if which == "a":
            d.all2all_rows_device(band_buf.data_ptr(), lo, hi)
        else:
            with switches(cols, hits):
                d.all2all_rows_tiled_device(band_buf.data_ptr(), lo, hi)
        out = {"wall_ms": (time.perf_counter() - t1) * 1e3}
        st = d.stats()
        out["kernel_ms"] = st["kernel_ms"]
        out["stats"] = d.all2all_rows_stats() if which == "a" else d.all2all_rows_tiled_stats()
        out["peak_device_bytes"] = int(st["device_bytes"]) + 4 * (tri(hi) - tri(lo)) + (int(out["stats"]["scratch_bytes"]) if which == "a" else 0)
        return out

    res = {"rows": [lo, hi], "band_bytes": 4 * (tri(hi) - tri(lo))}
    arm("a")                                                        # equality first (this is the warm-up round as well)
    want = band_buf.cpu().numpy().copy()
    for which in arms:
        if which != "a":
            band_buf.fill_(-1)
            arm(which)
            assert np.array_equal(band_buf.cpu().numpy(), want), "%s %s: arm %s differs from the band call" % (name, (lo, hi), which)
    res["equal"] = True
    runs_of = {x: [] for x in arms}
    for r in range(runs):
        for which in arms:
            o = arm(which)
            runs_of[which].append(o)
            log("%s rows %d:%d run %d arm %s: wall %.3f ms, device %.3f ms" % (name, lo, hi, r, which, o["wall_ms"], o["kernel_ms"]))
    res["runs"] = runs_of
    res["summary"] = sm = summary(runs_of)
    res["stats"] = {x: runs_of[x][-1]["stats"] for x in arms}
    for which in arms:
        if which != "a":
            res["%s_below_a" % which] = sm[which]["wall_ms"]["max"] < sm["a"]["wall_ms"]["min"]        # beyond the spread of both
            res["a_below_%s" % which] = sm["a"]["wall_ms"]["max"] < sm[which]["wall_ms"]["min"]
            res["%s_over_a" % which] = round(sm[which]["wall_ms"]["median"] / sm["a"]["wall_ms"]["median"], 4)
    del band_buf
    torch.cuda.empty_cache()
    return res


def banded_run(d, name, N, R, runs):
    counts = np.zeros(N, np.uint32)                                 # (no bound and no measure reads them)

    def arm(which):
        t1 = time.perf_counter()
        rows = d.all2all_sparse_filtered([], counts) if which == "whole" else d.all2all_sparse_filtered_banded(R, [], counts)
        out = {"wall_ms": (time.perf_counter() - t1) * 1e3, "kernel_ms": d.stats()["kernel_ms"], "nnz": int(rows.nnz)}
        if which == "whole":
            out["peak_device_bytes"] = int(d.stats()["device_bytes"]) + 4 * tri(N)
        else:
            out["stats"] = d.all2all_banded_stats()
            out["peak_device_bytes"] = int(out["stats"]["peak_device_bytes"])
        return out, rows

    _, want = arm("whole")
    _, got = arm("banded")
    assert np.array_equal(got.row_ptr, want.row_ptr) and np.array_equal(got.col, want.col) and np.array_equal(got.val, want.val), "the banded run differs"
    del want, got
    runs_of = {"whole": [], "banded": []}
    for r in range(runs):
        for which in runs_of:
            o, _ = arm(which)
            runs_of[which].append(o)
            log("%s sparse run %d arm %s: wall %.3f ms" % (name, r, which, o["wall_ms"]))
    sm = summary(runs_of)
    return {"band_rows": R, "equal": True, "runs": runs_of, "summary": sm, "stats": runs_of["banded"][-1]["stats"],
            "banded_over_whole": round(sm["banded"]["wall_ms"]["median"] / sm["whole"]["wall_ms"]["median"], 4)}


def one_input(K, S, torch, name, spec, k, seed, runs, dev, arms):
    device = torch.device("cuda", dev)
    N = spec["samples"]
    t0 = time.perf_counter()
    g = S.CladeGenomes(N, spec["clade_size"], spec["length"], seed=seed, device=device)
    pat = S.build_patterns(lambda i: S.kmers_of(g.sample(i), k), N, device)
    arr = S.to_view_arrays(pat)
    view = K.make_view(k, N, arr["num_kmers"], arr["parent_id"], arr["num_samples"], arr["num_local"], arr["last_sample_id"], arr["num_bits"],
                       arr["data_offset"], arr["data"])
    res = {"samples": N, "patterns": int(pat["num_kmers"].numel()), "k": k, "triangle_bytes": 4 * tri(N), "bands": {}}
    del pat, g
    torch.cuda.empty_cache()
    d = K.DeviceDB(view, device=dev)
    log("%s: %d patterns, database and upload %.1f s" % (name, res["patterns"], time.perf_counter() - t0))
    for label, (lo, hi) in spec["bands"].items():
        res["bands"][label] = one_band(d, torch, device, dev, name, lo, hi, arms, runs)
    if spec["banded"]:
        res["sparse"] = banded_run(d, name, N, spec["banded"], runs)
    d.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--inputs", default="clade256,c3part")
    ap.add_argument("--k", type=int, default=18)
    ap.add_argument("--seed", type=int, default=20260928)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--tile-hits", default="", help="further arms: b16k at these KMDB_ROWS_TILE_HITS (comma separated)")
    ap.add_argument("--tile-cols", default="", help="further arms: tiles of these many columns (comma separated)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert args.runs >= 3, "three runs an arm at the least"
    import torch
    from _kmerdb_loader import import_kmerdb_amd
    K = import_kmerdb_amd()
    S = importlib.import_module("kmerdb_amd.synth")
    assert K.device_count() > 0, "needs an MI355X"
    arms = {"a": (None, None), "b16k": (16384, None), "bmax": (TILE_MAX, None)}
    for t in [x for x in args.tile_cols.split(",") if x]:
        arms["b%s" % t] = (int(t), None)
    for h in [x for x in args.tile_hits.split(",") if x]:
        arms["b16k_h%s" % h] = (16384, int(h))
    res = {"arms": {"a": "kmdb_all2all_rows_device", "b16k": "kmdb_all2all_rows_tiled_device, tiles of 16384 columns", "bmax": "the same, tiles of %d columns" % TILE_MAX,
                    "whole / banded": "kmdb_all2all_sparse_filtered / kmdb_all2all_sparse_filtered_banded"}, "inputs": {}}
    for name in args.inputs.split(","):
        res["inputs"][name] = one_input(K, S, torch, name, INPUTS[name], args.k, args.seed, args.runs, args.device, arms)
        if args.out:
            open(args.out, "w").write(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
