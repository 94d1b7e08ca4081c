"""A/B of the band call through the block-record pipeline (kmdb_all2all_rows_records_device) against the parent commit's ways to a band of rows,
and of the banded sparse run over its three band paths against the whole sparse call.  README has the figures.

    python profiles/all2all_band_records_ab.py --inputs clade256,c3part --out profiles/all2all_band_records_ab.json

Inputs, both through kmer-db_amd/synth.py, each uploaded once (one handle per input, one process):

    clade256   synth.CladeGenomes 256 x 1 Mbp, clades of 16; the band is the last 16 samples
    c3part     bench.py's c3part parameters (10 000 x 300 kbp, clades of 50); the bands are the last 100 samples and the rows 5000 .. 5100;
               the banded sparse run at R = 1000

Arms on the same handle, each timed with the wall clock around a call that ends in its own wait (the slice of arm a: a device-to-device copy
and a synchronize):

    a   kmdb_all2all_dense_device into a whole triangle, then the band's cells copied out of it      the parent commit
    b   kmdb_all2all_rows_device                                                                     the parent commit
    c   kmdb_all2all_rows_tiled_device                                                               the parent commit
    d   kmdb_all2all_rows_records_device                                                             this commit
    sparse: kmdb_all2all_sparse_filtered (whole) against kmdb_all2all_sparse_filtered_banded_path over tiled / tree / records

The outputs are compared first (cell for cell; row_ptr, col, val for the sparse runs), which is the warm-up round as well.  Then --runs rounds
(5) in which the arms ALTERNATE; --slow-runs sets the rounds of the sparse run's tiled and tree paths alone (they take seconds each).  The json
gives every run, the median and the range per arm, arm d's stats (units run / total, stage times, peak device bytes), and whether d lies below
b and below a beyond the spread of both.  No ratio is a condition."""
import argparse
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
ARMS = {"a": "kmdb_all2all_dense_device + a copy of the band's cells", "b": "kmdb_all2all_rows_device", "c": "kmdb_all2all_rows_tiled_device",
        "d": "kmdb_all2all_rows_records_device"}


def log(msg):
    print(msg, file=sys.stderr, flush=True)


def tri(i):
    return i * (i - 1) // 2 if i else 0


def spread(v):
    return {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}


def one_band(d, torch, device, dev, name, N, lo, hi, runs):
    cells = tri(hi) - tri(lo)
    band_buf = torch.empty(max(1, cells), dtype=torch.int32, device=device)
    whole = torch.empty(max(1, tri(N)), dtype=torch.int32, device=device)
    torch.cuda.synchronize(dev)

    def arm(which):
        t1 = time.perf_counter()
        if which == "a":
            d.all2all_dense_device(whole.data_ptr())
            band_buf.copy_(whole[tri(lo): tri(hi)])
            torch.cuda.synchronize(dev)
        elif which == "b":
            d.all2all_rows_device(band_buf.data_ptr(), lo, hi)
        elif which == "c":
            d.all2all_rows_tiled_device(band_buf.data_ptr(), lo, hi)
        else:
            d.all2all_rows_records_device(band_buf.data_ptr(), lo, hi)
        out = {"wall_ms": (time.perf_counter() - t1) * 1e3}
        st = d.stats()
        out["kernel_ms"] = st["kernel_ms"]
        if which == "a":
            out["peak_device_bytes"] = int(st["device_bytes"]) + 4 * tri(N) + 4 * cells
            out["stats"] = {k: st[k] for k in ("k0_ms", "k1n_ms", "k1g_ms", "k2_ms", "n_records", "sized_call")}
        elif which == "b":
            out["stats"] = d.all2all_rows_stats()
            out["peak_device_bytes"] = int(st["device_bytes"]) + 4 * cells + int(out["stats"]["scratch_bytes"])
        elif which == "c":
            out["stats"] = d.all2all_rows_tiled_stats()
            out["peak_device_bytes"] = int(st["device_bytes"]) + 4 * cells
        else:
            out["stats"] = d.all2all_rows_records_stats()
            out["peak_device_bytes"] = int(out["stats"]["peak_device_bytes"])
        return out

    res = {"rows": [lo, hi], "band_bytes": 4 * cells}
    arm("b")                                                        # equality first (this is the warm-up round as well)
    want = band_buf.cpu().numpy().copy()
    for which in ("a", "c", "d"):
        band_buf.fill_(-1)
        arm(which)
        assert np.array_equal(band_buf.cpu().numpy(), want), "%s %s: arm %s differs from the band call" % (name, (lo, hi), which)
    res["equal"] = True
    runs_of = {x: [] for x in ARMS}
    for r in range(runs):
        for which in ARMS:
            o = arm(which)
            runs_of[which].append(o)
            log("%s rows %d:%d run %d arm %s: wall %.3f ms, device %.3f ms" % (name, lo, hi, r, which, o["wall_ms"], o["kernel_ms"]))
    res["runs"] = runs_of
    res["summary"] = sm = {x: {"wall_ms": spread([o["wall_ms"] for o in runs_of[x]]), "kernel_ms": spread([o["kernel_ms"] for o in runs_of[x]]),
                               "peak_device_bytes": max(o["peak_device_bytes"] for o in runs_of[x])} for x in ARMS}
    res["stats"] = {x: runs_of[x][-1]["stats"] for x in ARMS}
    for other in ("a", "b", "c"):
        res["d_below_%s" % other] = sm["d"]["wall_ms"]["max"] < sm[other]["wall_ms"]["min"]        # beyond the spread of both
        res["%s_below_d" % other] = sm[other]["wall_ms"]["max"] < sm["d"]["wall_ms"]["min"]
        res["d_over_%s" % other] = round(sm["d"]["wall_ms"]["median"] / sm[other]["wall_ms"]["median"], 4)
    del band_buf, whole
    torch.cuda.empty_cache()
    return res


def banded_run(d, name, N, R, runs, slow_runs):
    counts = np.zeros(N, np.uint32)                                 # (no bound and no measure reads them)
    paths = ("whole", "records", "tree", "tiled")

    def arm(which):
        t1 = time.perf_counter()
        rows = d.all2all_sparse_filtered([], counts) if which == "whole" else d.all2all_sparse_filtered_banded(R, [], counts, path=which)
        out = {"wall_ms": (time.perf_counter() - t1) * 1e3, "nnz": int(rows.nnz)}
        if which == "whole":
            out["peak_device_bytes"] = int(d.stats()["device_bytes"]) + 4 * tri(N)
        else:
            out["stats"] = d.all2all_banded_stats()
            out["peak_device_bytes"] = int(out["stats"]["peak_device_bytes"])
            if which == "records":
                out["records_stats"] = d.all2all_banded_records_stats()
        return out, rows

    _, want = arm("whole")
    for which in paths[1:]:
        _, got = arm(which)
        assert np.array_equal(got.row_ptr, want.row_ptr) and np.array_equal(got.col, want.col) and np.array_equal(got.val, want.val), "the banded run over %s differs" % which
        del got
    del want
    runs_of = {x: [] for x in paths}
    for r in range(runs):
        for which in paths:
            if which in ("tree", "tiled") and r >= slow_runs:
                continue
            o, _ = arm(which)
            runs_of[which].append(o)
            log("%s sparse run %d arm %s: wall %.3f ms" % (name, r, which, o["wall_ms"]))
    sm = {x: {"wall_ms": spread([o["wall_ms"] for o in runs_of[x]]), "runs": len(runs_of[x]), "peak_device_bytes": max(o["peak_device_bytes"] for o in runs_of[x])}
          for x in paths if runs_of[x]}
    out = {"band_rows": R, "equal": True, "runs": runs_of, "summary": sm}
    for x in paths[1:]:
        if x in sm:
            out["%s_over_whole" % x] = round(sm[x]["wall_ms"]["median"] / sm["whole"]["wall_ms"]["median"], 4)
    return out


def one_input(K, S, torch, name, spec, k, seed, runs, slow_runs, dev):
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
        res["bands"][label] = one_band(d, torch, device, dev, name, N, lo, hi, runs)
    if spec["banded"]:
        res["sparse"] = banded_run(d, name, N, spec["banded"], runs, slow_runs)
    d.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--inputs", default="clade256,c3part")
    ap.add_argument("--k", type=int, default=18)
    ap.add_argument("--seed", type=int, default=20260928)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--slow-runs", type=int, default=None, help="rounds of the sparse run's tree and tiled paths (default: --runs)")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert args.runs >= 3, "three runs an arm at the least"
    import torch
    from _kmerdb_loader import import_kmerdb_amd
    K = import_kmerdb_amd()
    S = importlib.import_module("kmerdb_amd.synth")
    assert K.device_count() > 0, "needs an MI355X"
    res = {"arms": dict(ARMS, sparse="kmdb_all2all_sparse_filtered (whole) / kmdb_all2all_sparse_filtered_banded_path (records, tree, tiled)"),
           "runs": args.runs, "slow_runs": args.runs if args.slow_runs is None else args.slow_runs, "inputs": {}}
    for name in args.inputs.split(","):
        res["inputs"][name] = one_input(K, S, torch, name, INPUTS[name], args.k, args.seed, args.runs, res["slow_runs"], args.device)
        if args.out:
            open(args.out, "w").write(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
