"""A/B of band emit (KMDB_BAND_EMIT=1: the records band call emitting the band's block records alone, keyed relative to the band) against the
parent form of the same call and against the tree band call.  README has the figures.

    python profiles/all2all_band_emit_ab.py --input c3part --out profiles/all2all_band_emit_ab.c3part.json

ONE process per input (--input); the inputs are those of profiles/all2all_band_records_ab.py, through kmer-db_amd/synth.py, and one beyond 2^22
block pairs:

    clade256   synth.CladeGenomes 256 x 1 Mbp, clades of 16; the band is the last 16 samples
    c3part     bench.py's c3part parameters (10 000 x 300 kbp, clades of 50); the bands are the last 100 samples and the rows 5000 .. 5100;
               the banded sparse run at R = 1000
    far100k    100 000 x 3 kbp, clades of 50, KMDB_BLOCK_WIDTH=32: 3 125 blocks, 4.88 M block pairs — the whole-matrix pipeline refuses it
               ("too many block pairs"), so arm a does not exist and arm c was the parent's only route; the bands are the last 100 samples and the
               rows 50 000 .. 50 100

Arms, each timed with the wall clock around a call that ends in its own wait:

    a   STAND-IN for the parent commit's call: kmdb_all2all_rows_records_device on a handle made under KMDB_BAND_EMIT=0, the parent form — decode, emit and the sorts whole, the apply
        stage culled.  (It is this commit's library, not a build of the parent commit: the kernels that form launches are the parent's in every
        resource figure, profiles/all2all_band_emit_resources.md; the two libraries cannot alternate inside one process.)
    b   the same call on a handle made under KMDB_BAND_EMIT=1: band emit
    c   kmdb_all2all_rows_device (the tree call), on handle b
    sparse: kmdb_all2all_sparse_filtered_banded_path(records) on handle a against handle b

The outputs are compared first (cell for cell; row_ptr, col, val for the sparse runs), which is the warm-up round as well.  Then --runs rounds (5) in
which the arms ALTERNATE.  The json gives every run, the median and the range per arm, the stage times, `records`, the band state's bytes against the
whole state's, and peak device bytes.  No ratio is a condition."""
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

INPUTS = {"clade256": dict(samples=256, clade_size=16, length=1_000_000, bands={"last": (240, 256)}, banded=0, width=None),
          "c3part": dict(samples=10000, clade_size=50, length=300_000, bands={"last": (9900, 10000), "middle": (5000, 5100)}, banded=1000, width=None),
          "far100k": dict(samples=100000, clade_size=50, length=3000, bands={"last": (99900, 100000), "middle": (50000, 50100)}, banded=0, width=32)}
ARMS = {"a": "kmdb_all2all_rows_records_device, KMDB_BAND_EMIT=0 (the parent form: a STAND-IN for the parent commit's build, this commit's library)", "b": "kmdb_all2all_rows_records_device, KMDB_BAND_EMIT=1 (band emit)",
        "c": "kmdb_all2all_rows_device (tree)"}


def log(msg):
    print(msg, file=sys.stderr, flush=True)


def tri(i):
    return i * (i - 1) // 2 if i else 0


def spread(v):
    return {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}


def one_band(handles, torch, device, name, lo, hi, runs):
    cells = tri(hi) - tri(lo)
    band_buf = torch.empty(max(1, cells), dtype=torch.int32, device=device)
    torch.cuda.synchronize(device)
    arms = [x for x in ARMS if x != "a" or "a" in handles]

    def arm(which):
        d = handles["a" if which == "a" else "b"]
        t1 = time.perf_counter()
        if which == "c":
            d.all2all_rows_device(band_buf.data_ptr(), lo, hi)
        else:
            d.all2all_rows_records_device(band_buf.data_ptr(), lo, hi)
        out = {"wall_ms": (time.perf_counter() - t1) * 1e3, "kernel_ms": d.stats()["kernel_ms"]}
        if which == "c":
            out["stats"] = d.all2all_rows_stats()
            out["peak_device_bytes"] = int(d.stats()["device_bytes"]) + 4 * cells + int(out["stats"]["scratch_bytes"])
        else:
            out["stats"] = d.all2all_rows_records_stats()
            out["band_emit"] = d.all2all_rows_band_emit_stats()
            out["peak_device_bytes"] = int(out["stats"]["peak_device_bytes"])
        return out

    res = {"rows": [lo, hi], "band_bytes": 4 * cells}
    arm("c")                                                        # equality first (this is the warm-up round as well)
    want = band_buf.cpu().numpy().copy()
    for which in arms[:-1]:
        band_buf.fill_(-1)
        o = arm(which)
        assert np.array_equal(band_buf.cpu().numpy(), want), "%s %s: arm %s differs from the tree call" % (name, (lo, hi), which)
        assert o["band_emit"]["form"] == (1 if which == "a" else 2), (which, o["band_emit"])
    res["equal"] = True
    runs_of = {x: [] for x in arms}
    for r in range(runs):
        for which in arms:
            o = arm(which)
            runs_of[which].append(o)
            log("%s rows %d:%d run %d arm %s: wall %.3f ms, device %.3f ms" % (name, lo, hi, r, which, o["wall_ms"], o["kernel_ms"]))
    res["runs"] = runs_of
    res["summary"] = sm = {x: {"wall_ms": spread([o["wall_ms"] for o in runs_of[x]]), "kernel_ms": spread([o["kernel_ms"] for o in runs_of[x]]),
                               "peak_device_bytes": max(o["peak_device_bytes"] for o in runs_of[x])} for x in arms}
    res["stats"] = {x: runs_of[x][-1]["stats"] for x in arms}
    res["band_emit"] = {x: runs_of[x][-1]["band_emit"] for x in arms if x != "c"}
    for other in arms:
        if other != "b":
            res["b_below_%s" % other] = sm["b"]["wall_ms"]["max"] < sm[other]["wall_ms"]["min"]        # beyond the spread of both
            res["%s_below_b" % other] = sm[other]["wall_ms"]["max"] < sm["b"]["wall_ms"]["min"]
            res["b_over_%s" % other] = round(sm["b"]["wall_ms"]["median"] / sm[other]["wall_ms"]["median"], 4)
    del band_buf
    torch.cuda.empty_cache()
    return res


def banded_run(handles, name, N, R, runs):
    counts = np.zeros(N, np.uint32)                                 # (no bound and no measure reads them)

    def arm(which):
        d = handles[which]
        t1 = time.perf_counter()
        rows = d.all2all_sparse_filtered_banded(R, [], counts, path="records")
        out = {"wall_ms": (time.perf_counter() - t1) * 1e3, "nnz": int(rows.nnz), "stats": d.all2all_banded_stats(), "records_stats": d.all2all_banded_records_stats(),
               "band_emit": d.all2all_rows_band_emit_stats()}
        out["peak_device_bytes"] = int(out["stats"]["peak_device_bytes"])
        return out, rows

    _, want = arm("a")
    _, got = arm("b")
    assert np.array_equal(got.row_ptr, want.row_ptr) and np.array_equal(got.col, want.col) and np.array_equal(got.val, want.val), "the banded run under band emit differs"
    del got, want
    runs_of = {"a": [], "b": []}
    for r in range(runs):
        for which in ("a", "b"):
            o, _ = arm(which)
            runs_of[which].append(o)
            log("%s sparse run %d arm %s: wall %.3f ms, band calls %.3f ms" % (name, r, which, o["wall_ms"], o["records_stats"]["ms"]))
    sm = {x: {"wall_ms": spread([o["wall_ms"] for o in runs_of[x]]), "band_calls_ms": spread([o["records_stats"]["ms"] for o in runs_of[x]]),
              "peak_device_bytes": max(o["peak_device_bytes"] for o in runs_of[x])} for x in runs_of}
    return {"band_rows": R, "equal": True, "runs": runs_of, "summary": sm, "b_over_a": round(sm["b"]["wall_ms"]["median"] / sm["a"]["wall_ms"]["median"], 4),
            "b_over_a_band_calls": round(sm["b"]["band_calls_ms"]["median"] / sm["a"]["band_calls_ms"]["median"], 4)}


def one_input(K, S, torch, name, spec, k, seed, runs, dev):
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
    if spec["width"]:
        os.environ["KMDB_BLOCK_WIDTH"] = str(spec["width"])
    handles = {}
    lo, hi = next(iter(spec["bands"].values()))
    probe = torch.empty(max(1, tri(hi) - tri(lo)), dtype=torch.int32, device=device)
    for which, value in (("a", "0"), ("b", "1")):
        os.environ["KMDB_BAND_EMIT"] = value                        # (read at the handle's first records band call: made here)
        d = K.DeviceDB(view, device=dev)
        d.all2all_rows_records_device(probe.data_ptr(), lo, hi)
        st = d.all2all_rows_records_stats()
        if st["path"] != 1:
            log("%s: arm %s takes the tree call (%s): the arm is left out" % (name, which, d.fallback_reason()))
            d.close()
            continue
        handles[which] = d
    del probe
    assert "b" in handles, "band emit did not take the input"
    res["fallback_reason"] = handles["b"].fallback_reason()
    log("%s: %d patterns, database and upload %.1f s, arms %s" % (name, res["patterns"], time.perf_counter() - t0, sorted(handles)))
    for label, (lo, hi) in spec["bands"].items():
        res["bands"][label] = one_band(handles, torch, device, name, lo, hi, runs)
    if spec["banded"] and "a" in handles:
        res["sparse"] = banded_run(handles, name, N, spec["banded"], runs)
    for d in handles.values():
        d.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--input", default="clade256", choices=sorted(INPUTS))
    ap.add_argument("--k", type=int, default=18)
    ap.add_argument("--seed", type=int, default=20260928)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert args.runs >= 3, "three runs an arm at the least"
    import torch
    from _kmerdb_loader import import_kmerdb_amd
    K = import_kmerdb_amd()
    S = importlib.import_module("kmerdb_amd.synth")
    assert K.device_count() > 0, "needs an MI355X"
    res = {"arms": dict(ARMS, sparse="kmdb_all2all_sparse_filtered_banded_path(records) under KMDB_BAND_EMIT=0 (a) and =1 (b)"), "runs": args.runs,
           "input": args.input, "result": one_input(K, S, torch, args.input, INPUTS[args.input], args.k, args.seed, args.runs, args.device)}
    if args.out:
        open(args.out, "w").write(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
