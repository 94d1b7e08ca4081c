"""A/B of `all2all-parts -sample-rows jaccard:<count>` on a grid of a few parts: the front-end of the PARENT commit (every off-diagonal cell
compacted by kmdb_db2db_sparse_filtered, every kept pair copied over PCIe, scored on the host and pushed twice into the sampler) against this
one (every cell's candidates selected on the device: kmdb_db2db_sampled, kmdb_all2all_sampled on the diagonal).  A third arm, this commit with
KMDB_PARTS_HOST_SAMPLER=1, is the parent's path in this binary.  README has the numbers.

    git worktree add /tmp/parent HEAD~1 && make -C /tmp/parent/kmer-db_amd -j8
    python profiles/parts_sample_ab.py --parent-exe /tmp/parent/kmer-db_amd/bin/kmer-db-amd --out profiles/parts_sample_ab.json

The collection is synth.py's clade genomes at bench.py's c3part parameters (clades of 50, 300 kbp, k = 18, r1 = 0.10), `--parts` parts of
`--part-samples` samples each, sample i in part i % parts so that every clade has members in every part.  Every arm is a process over the
same part files; measured end to end: the wall clock of the process and its peak RSS (wait4).  One warm-up run per arm, then `--rounds` rounds
with the arms alternating; the outputs are compared byte for byte BEFORE anything is timed.  One more run of this commit under KMDB_VERBOSE
(not timed) gives the per-cell lines: tiles, candidates, rows truncated / re-fetched, selection ms.  Everything is reported, nothing judged."""
import argparse
import importlib
import json
import os
import re
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402

log = bench.log


def run_cli(exe, args, env=None):
    """one front-end process: wall clock, peak RSS from the kernel's accounting of that child (wait4), its stderr"""
    t0 = time.perf_counter()
    with tempfile.TemporaryFile(mode="w+") as err:
        p = subprocess.Popen([exe] + args, stdout=subprocess.DEVNULL, stderr=err, env=dict(os.environ, **(env or {})))
        _, status, ru = os.wait4(p.pid, 0)
        wall = time.perf_counter() - t0
        err.seek(0)
        stderr = err.read()
    if os.waitstatus_to_exitcode(status) != 0:
        raise SystemExit("front-end failed: " + stderr[-2000:])
    saved = re.search(r"No. saved pairs: (\d+)", stderr)
    return {"wall_s": wall, "peak_rss_mb": ru.ru_maxrss / 1024.0, "saved_pairs": int(saved.group(1)) if saved else None}, stderr


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-exe", default=None, help="kmer-db-amd built from the parent commit (without it only this commit's two arms are measured)")
    ap.add_argument("--parts", type=int, default=4)
    ap.add_argument("--part-samples", type=int, default=1000)
    ap.add_argument("--sample-rows", default="jaccard:10")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--k", type=int, default=18)
    ap.add_argument("--seed", type=int, default=20260928)
    ap.add_argument("--tmp", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "parts_sample_ab.json"))
    args = ap.parse_args()
    import torch
    from _kmerdb_loader import import_kmerdb_amd
    import_kmerdb_amd()
    S = importlib.import_module("kmerdb_amd.synth")
    wl = bench.WORKLOADS["c3part"]
    device = torch.device("cuda", args.device)
    P, n = args.parts, args.part_samples
    N = P * n
    g = S.CladeGenomes(N, wl["clade_size"], wl["length"], r1=0.10, seed=args.seed, device=device)
    res = {"workload": "%d parts of %d synthetic %g Mbp genomes (clades of %d over all parts, r1 = 0.10), k=%d, all2all-parts -sample-rows %s"
                       % (P, n, wl["length"] / 1e6, wl["clade_size"], args.k, args.sample_rows),
           "cells": P * (P + 1) // 2, "off_diagonal_cells": P * (P - 1) // 2, "runs": {}}
    with tempfile.TemporaryDirectory(dir=args.tmp) as td:
        t0 = time.time()
        paths = []
        for p in range(P):
            ids = list(range(p, N, P))
            pat = S.build_patterns(lambda i: S.kmers_of(g.sample(ids[i]), args.k), n, device, progress=None)
            arr = S.to_view_arrays(pat)
            tables = S.build_hashtables(pat["dictionary"], pat["kmer_pid"], args.k)
            paths.append(os.path.join(td, "part%d.db" % p))
            S.write_db(paths[-1], args.k, 1.0, [g.name(i) for i in ids], pat["sample_counts"], arr, kmers_count=int(pat["dictionary"].numel()), tables=tables)
            log("part %d: %d k-mers, %d patterns, %.1f s so far" % (p, int(pat["dictionary"].numel()), len(arr["num_kmers"]), time.time() - t0))
            del pat, arr, tables
        del g
        torch.cuda.empty_cache()
        lst = os.path.join(td, "db.list")
        with open(lst, "w") as f:
            f.write("\n".join(paths) + "\n")
        this = os.path.join(ROOT, "kmer-db_amd", "bin", "kmer-db-amd")
        arms = {"this": (this, None), "this_host_sampler": (this, {"KMDB_PARTS_HOST_SAMPLER": "1"})}
        if args.parent_exe:
            arms["parent"] = (args.parent_exe, None)
        cli = ["all2all-parts", "-sample-rows", args.sample_rows, "-gpu", str(args.device), lst]
        # warm-up, and the outputs compared before anything is timed
        outs = {}
        for arm, (exe, env) in arms.items():
            csv = os.path.join(td, arm + ".csv")
            r, _ = run_cli(exe, cli + [csv], env)
            log("warm-up", arm, json.dumps(r))
            with open(csv, "rb") as f:
                outs[arm] = f.read()
            os.unlink(csv)
            res["runs"][arm] = []
        for arm in arms:
            assert outs[arm] == outs["this"], "the front-ends wrote different files: " + arm
        res["outputs_equal"] = True
        res["output_bytes"] = len(outs["this"])
        for rnd in range(args.rounds):
            for arm, (exe, env) in arms.items():
                csv = os.path.join(td, arm + ".csv")
                r, _ = run_cli(exe, cli + [csv], env)
                os.unlink(csv)
                res["runs"][arm].append(r)
                log("round %d" % rnd, arm, json.dumps(r))
        # the per-cell lines of the device path (not timed)
        csv = os.path.join(td, "verbose.csv")
        _, stderr = run_cli(this, cli + [csv], {"KMDB_VERBOSE": "1"})
        cells = [dict(tiles_touched=int(m.group(1)), tiles=int(m.group(2)), candidates=int(m.group(3)), rows_truncated=int(m.group(4)), rows_refetched=int(m.group(5)),
                      select_ms=float(m.group(6)))
                 for m in re.finditer(r"sampled cell \(\d+,\d+\): (\d+) of (\d+) tiles touched, (\d+) candidates, (\d+) rows truncated, (\d+) re-fetched, selection ([0-9.eE+-]+) ms", stderr)]
        res["sampled_cells"] = cells
        _, stderr = run_cli(this, cli + [csv], {"KMDB_VERBOSE": "1", "KMDB_PARTS_HOST_SAMPLER": "1"})
        res["host_path_cells_left_the_device"] = [int(x) for x in re.findall(r"sparse cell: \d+ of \d+ tiles touched, (\d+) cells left the device", stderr)]
    for arm, runs in res["runs"].items():
        res[arm + "_summary"] = {k: {"median": float(np.median([x[k] for x in runs])), "min": float(min(x[k] for x in runs)), "max": float(max(x[k] for x in runs))}
                                 for k in ("wall_s", "peak_rss_mb")}
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps({k: v for k, v in res.items() if k != "runs"}))


if __name__ == "__main__":
    main()
