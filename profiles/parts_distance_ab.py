"""A/B of `all2all-parts -distance jaccard` on a grid of a few parts, end to end:

    a  the PARENT commit's `all2all-parts L T` followed by its `distance -host -sparse jaccard T out` (the table of counts written, read and
       parsed, the measure on the host)
    b  the parent's pair with KMDB_DISTANCE_DEVICE=1 (the table parsed, measured and formatted on the device)
    c  this commit's `all2all-parts -distance jaccard L out` (the block rows' CSRs gathered and measured in HBM, no table of counts)

    git worktree add /tmp/parent HEAD~1 && make -C /tmp/parent/kmer-db_amd -j8
    python profiles/parts_distance_ab.py --parent-exe /tmp/parent/kmer-db_amd/bin/kmer-db-amd --out profiles/parts_distance_ab.json

The collection is the one of profiles/parts_sample_ab.py: synth.py's clade genomes at bench.py's c3part parameters (clades of 50, 300 kbp,
k = 18, r1 = 0.10), `--parts` parts of `--part-samples` samples each, sample i in part i % parts.  An arm is one or two processes over the same
part files; measured is the wall clock from the start of its first process to the end of its last, every file it writes included (the table of
counts of arms a and b too).  One warm-up run per arm, then `--rounds` rounds with the arms alternating; the outputs are compared byte for byte
BEFORE anything is timed.  Reported: medians and ranges, the ratios c / a and c / b of the medians, and whether every run of c lies below every
run of the other arm.  Nothing is judged and no default depends on the outcome: the path runs only under the new switch."""
import argparse
import importlib
import json
import os
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
    p = subprocess.run([exe] + args, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, text=True, env=dict(os.environ, **(env or {})))
    if p.returncode != 0:
        raise SystemExit("front-end failed: " + p.stderr[-2000:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-exe", default=None, help="kmer-db-amd built from the parent commit (without it the pair of commands runs in this commit's binary)")
    ap.add_argument("--parts", type=int, default=4)
    ap.add_argument("--part-samples", type=int, default=1000)
    ap.add_argument("--measure", default="jaccard")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--k", type=int, default=18)
    ap.add_argument("--seed", type=int, default=20260928)
    ap.add_argument("--tmp", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "parts_distance_ab.json"))
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
    this = os.path.join(ROOT, "kmer-db_amd", "bin", "kmer-db-amd")
    pair_exe = args.parent_exe or this
    res = {"workload": "%d parts of %d synthetic %g Mbp genomes (clades of %d over all parts, r1 = 0.10), k=%d, %s, end-to-end wall clock of the processes"
                       % (P, n, wl["length"] / 1e6, wl["clade_size"], args.k, args.measure),
           "pair_of_commands_from": "the parent commit" if args.parent_exe else "THIS commit (no --parent-exe)", "rounds": args.rounds, "runs": {}}
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
        gpu = ["-gpu", str(args.device)]

        def pair(env):
            def run(out):
                table = out + ".counts"
                run_cli(pair_exe, ["all2all-parts"] + gpu + [lst, table])
                run_cli(pair_exe, ["distance"] + gpu + (["-host"] if env is None else []) + ["-sparse", args.measure, table, out], env)
                size = os.path.getsize(table)
                os.unlink(table)
                return size
            return run

        def fused(out):
            run_cli(this, ["all2all-parts"] + gpu + ["-distance", args.measure, lst, out])
            return 0

        arms = {"a_pair_host": pair(None), "b_pair_device": pair({"KMDB_DISTANCE_DEVICE": "1"}), "c_fused": fused}

        def once(arm):
            out = os.path.join(td, arm + ".out")
            t = time.perf_counter()
            table_bytes = arms[arm](out)
            wall = time.perf_counter() - t
            with open(out, "rb") as f:
                data = f.read()
            os.unlink(out)
            return {"wall_s": wall, "table_of_counts_bytes": table_bytes}, data

        # warm-up, and the outputs compared before anything is timed
        outs = {}
        for arm in arms:
            r, outs[arm] = once(arm)
            log("warm-up", arm, json.dumps(r))
            res["runs"][arm] = []
        for arm in arms:
            assert outs[arm] == outs["c_fused"], "the arms wrote different files: " + arm
        res["outputs_equal"] = True
        res["output_bytes"] = len(outs["c_fused"])
        res["output_pairs"] = outs["c_fused"].count(b":") - 2
        del outs
        for rnd in range(args.rounds):
            for arm in arms:
                r, _ = once(arm)
                res["runs"][arm].append(r)
                log("round %d" % rnd, arm, json.dumps(r))
    walls = {arm: [x["wall_s"] for x in runs] for arm, runs in res["runs"].items()}
    for arm, w in walls.items():
        res[arm + "_summary"] = {"wall_s": {"median": float(np.median(w)), "min": float(min(w)), "max": float(max(w))},
                                 "table_of_counts_bytes": res["runs"][arm][0]["table_of_counts_bytes"]}
    for other, key in (("a_pair_host", "c_over_a"), ("b_pair_device", "c_over_b")):
        res[key] = {"ratio_of_medians": float(np.median(walls["c_fused"]) / np.median(walls[other])),
                    "every_run_of_c_below_every_run_of_the_other": bool(max(walls["c_fused"]) < min(walls[other]))}
    res["not_measured"] = ["other measures", "sparse cells (bounds that drop most pairs)", "larger grids", "-gpus"]
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps({k: v for k, v in res.items() if k != "runs"}))


if __name__ == "__main__":
    main()
