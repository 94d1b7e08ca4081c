"""A/B of the band call (kmdb_all2all_rows_device) against the two routes the parent commit offers to the last rows of a matrix.  README has the
figures.

    python profiles/all2all_rows_ab.py --inputs clade256,c3part --out profiles/all2all_rows_ab.json

Inputs, both through kmer-db_amd/synth.py, each uploaded once WITH its hashtables (arm b needs them; a and c do not read them):

    clade256   synth.CladeGenomes 256 x 1 Mbp, clades of 16; the band is the last 16 samples
    c3part     bench.py's c3part parameters (10 000 x 300 kbp, clades of 50); the band is the last 100 samples

Three arms on the same handle, in one process, each timed with the wall clock around the call (the device is idle before and after: every
call ends with its own wait) and with kmdb_stats.kernel_ms, the HIP-event time of the call's device work:

    a  kmdb_all2all_dense_device into a triangle of N (N - 1) / 2 cells, the band = its tail             what the parent commit offers
    b  kmdb_new2all_batch of the band samples' k-mer lists against the database (the lists are ready)     the other existing route
    c  kmdb_all2all_rows_device into a band of tri(N) - tri(N - band) cells                               this commit

The outputs are compared first: the band of c equals the tail of a cell for cell, and row i of b equals row N - band + i of the matrix in
the columns in front of it.  Then one warm-up round and --runs rounds (5) in which the arms ALTERNATE (a b c, a b c, ...).  Peak device bytes
of an arm: the output buffer it needs plus what kmdb_stats.device_bytes reports after its call (the handle's resident arrays), and for c the
scratch of kmdb_all2all_rows_stats.  The json gives every run, the median and the spread (min, max) per arm, the stats of c and whether c
lies below a and below b beyond the spread of both.  No ratio is a condition: the change claims the capability and the memory."""
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

INPUTS = {"clade256": dict(samples=256, clade_size=16, length=1_000_000, band=16),
          "c3part": dict(samples=10000, clade_size=50, length=300_000, band=100)}


def log(msg):
    print(msg, file=sys.stderr, flush=True)


def tri(i):
    return i * (i - 1) // 2 if i else 0


def one_input(K, S, torch, name, spec, k, seed, runs, dev):
    device = torch.device("cuda", dev)
    N, band = spec["samples"], spec["band"]
    lo = N - band
    t0 = time.perf_counter()
    g = S.CladeGenomes(N, spec["clade_size"], spec["length"], seed=seed, device=device)
    pat = S.build_patterns(lambda i: S.kmers_of(g.sample(i), k), N, device)
    arr = S.to_view_arrays(pat)
    tables = S.build_hashtables(pat["dictionary"], pat["kmer_pid"], k)
    view = K.make_view(k, N, arr["num_kmers"], arr["parent_id"], arr["num_samples"], arr["num_local"], arr["last_sample_id"], arr["num_bits"],
                       arr["data_offset"], arr["data"], bucket_offset=tables[0], slots=tables[1])
    queries = [K.sort_unique(S.kmers_of(g.sample(i), k).cpu().numpy().view(np.uint64)) for i in range(lo, N)]
    res = {"samples": N, "band_rows": band, "patterns": int(pat["num_kmers"].numel()), "k": k,
           "triangle_bytes": 4 * tri(N), "band_bytes": 4 * (tri(N) - tri(lo)), "query_kmers": int(sum(q.size for q in queries))}
    del pat, tables
    torch.cuda.empty_cache()
    d = K.DeviceDB(view, device=dev, with_hashtables=True)
    log("%s: %d patterns, database and upload %.1f s" % (name, res["patterns"], time.perf_counter() - t0))
    tri_buf = torch.empty(max(1, tri(N)), dtype=torch.int32, device=device)
    band_buf = torch.empty(max(1, tri(N) - tri(lo)), dtype=torch.int32, device=device)
    torch.cuda.synchronize(dev)

    def arm(which):
        t1 = time.perf_counter()
        if which == "a":
            d.all2all_dense_device(tri_buf.data_ptr())
            out = {"output_bytes": 4 * tri(N)}
        elif which == "b":
            rows = d.new2all(queries)
            out = {"output_bytes": 4 * band * N, "rows": rows}
        else:
            d.all2all_rows_device(band_buf.data_ptr(), lo, N)
            out = {"output_bytes": 4 * (tri(N) - tri(lo))}
        out["wall_ms"] = (time.perf_counter() - t1) * 1e3
        st = d.stats()
        out["kernel_ms"] = st["kernel_ms"]
        out["peak_device_bytes"] = int(st["device_bytes"]) + out["output_bytes"]
        if which == "c":
            out["stats"] = d.all2all_rows_stats()
            out["peak_device_bytes"] += int(out["stats"]["scratch_bytes"])
        return out

    # equality first (this is the warm-up round as well)
    arm("a")
    full_tail = tri_buf[tri(lo):].cpu().numpy().view(np.uint32)
    rows = arm("b").pop("rows")
    arm("c")
    got = band_buf.cpu().numpy().view(np.uint32)
    res["equal_c_a"] = bool(np.array_equal(got, full_tail))
    assert res["equal_c_a"], "the band differs from the tail of the whole matrix"
    res["equal_b_a"] = all(np.array_equal(rows[i - lo, :i], full_tail[tri(i) - tri(lo): tri(i) - tri(lo) + i]) for i in range(lo, N))
    assert res["equal_b_a"], "the new2all rows differ from the rows of the matrix"
    del rows
    out_runs = {x: [] for x in "abc"}
    for r in range(runs):
        for which in "abc":
            o = arm(which)
            o.pop("rows", None)
            out_runs[which].append(o)
            log("%s run %d arm %s: wall %.3f ms, device %.3f ms" % (name, r, which, o["wall_ms"], o["kernel_ms"]))
    res["runs"] = out_runs
    res["summary"] = {}
    for which in "abc":
        for key in ("wall_ms", "kernel_ms"):
            v = [o[key] for o in out_runs[which]]
            res["summary"].setdefault(which, {})[key] = {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}
        res["summary"][which]["peak_device_bytes"] = max(o["peak_device_bytes"] for o in out_runs[which])
    sm = res["summary"]
    res["stats_c"] = out_runs["c"][-1]["stats"]
    for other in "ab":
        res["c_below_%s" % other] = sm["c"]["wall_ms"]["max"] < sm[other]["wall_ms"]["min"]           # beyond the spread of both
        res["%s_below_c" % other] = sm[other]["wall_ms"]["max"] < sm["c"]["wall_ms"]["min"]
        res["c_over_%s" % other] = round(sm["c"]["wall_ms"]["median"] / sm[other]["wall_ms"]["median"], 4)
    sc = res["stats_c"]
    res["dominant_stage_c"] = "apply_ms" if sc["apply_ms"] >= sc["select_ms"] else "select_ms"
    d.close()
    del tri_buf, band_buf
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--inputs", default="clade256,c3part")
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
    res = {"arms": {"a": "kmdb_all2all_dense_device + slice", "b": "kmdb_new2all_batch of the band samples' k-mer lists", "c": "kmdb_all2all_rows_device"}, "inputs": {}}
    for name in args.inputs.split(","):
        res["inputs"][name] = one_input(K, S, torch, name, INPUTS[name], args.k, args.seed, args.runs, args.device)
        text = json.dumps(res, indent=1)
        if args.out:
            open(args.out, "w").write(text + "\n")
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
