"""A/B of `new2all -distance <measure>` against the two commands it replaces.  DESIGN section 4 has the paragraph.

    git worktree add <scratch>/parent HEAD~1 && make -C <scratch>/parent/kmer-db_amd -j8
    python profiles/new2all_distance_ab.py --parent-exe <scratch>/parent/kmer-db_amd/bin/kmer-db-amd --out profiles/new2all_distance_ab.json

The database is synthetic: --samples samples (10 000: the sample count and genome parameters of bench.py's c5part workload) through
kmer-db_amd/synth.py, written once in the reference's format WITH its hashtables; the --queries queries (1 000) are fresh strains of 20 of
its clades, as bench.py draws them, written as one FASTA file each and named in a sample list.  Three arms, each END TO END as a user runs
it — processes, wall clock, the device's first use, the database read and upload, the genomes read and every file written included:

    a  the parent's `new2all D Q T`, then the parent's `distance -host <measure> T out`
    b  the parent's `new2all D Q T`, then the parent's `distance <measure> T out` with KMDB_DISTANCE_DEVICE=1
    c  this commit's `new2all -distance <measure> D Q out`

One warm-up round, then --runs rounds (3 at least) in which the arms ALTERNATE (a b c, a b c, ...), all in this one call; every process
runs under its own time limit and a process that faults, aborts or runs out of time ends the script.  The three output files are compared
equal before anything is timed.  Without --parent-exe the arms a and b run this commit's binary and the json says so.  The json gives
every run, the median and the spread (min, max) per arm, and the two ratios."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
THIS_EXE = os.path.join(ROOT, "kmer-db_amd", "bin", "kmer-db-amd")


def log(*a):
    print(*a, file=sys.stderr, flush=True)


def write_inputs(td, samples, clade_size, length, k, seed, queries):
    """the database (with hashtables) and the query genomes -> paths of the database and of the sample list, number of patterns"""
    import importlib

    import torch

    from _kmerdb_loader import import_kmerdb_amd
    import_kmerdb_amd()
    S = importlib.import_module("kmerdb_amd.synth")
    device = torch.device("cuda:0")
    t0 = time.time()
    g = S.CladeGenomes(samples, clade_size, length, seed=seed, device=device)
    pat = S.build_patterns(lambda i: S.kmers_of(g.sample(i), k, 1.0), samples, device, progress=None)
    arr = S.to_view_arrays(pat)
    tables = S.build_hashtables(pat["dictionary"], pat["kmer_pid"], k)
    db = os.path.join(td, "db.db")
    S.write_db(db, k, 1.0, [g.name(i) for i in range(samples)], pat["sample_counts"], arr, kmers_count=int(pat["dictionary"].numel()), tables=tables)
    log("database: %d samples, %d patterns, %d bytes in %.1f s" % (samples, arr["num_kmers"].size, os.path.getsize(db), time.time() - t0))
    # queries = fresh strains of 20 clades of the collection, as bench.py's new2all mode draws them
    t0 = time.time()
    n_clades = max(1, samples // clade_size)
    chosen = [int(c) for c in np.random.default_rng(seed + 1000).choice(n_clades, size=min(20, n_clades), replace=False)]
    letters = np.frombuffer(b"ACGT", np.uint8)
    os.makedirs(os.path.join(td, "q"))
    lst = os.path.join(td, "queries.list")
    with open(lst, "w") as fl:
        for i in range(queries):
            codes = g.strain(chosen[i * len(chosen) // queries], samples + i).cpu().numpy()
            path = os.path.join(td, "q", "q%05d" % i)
            with open(path + ".fasta", "wb") as f:
                f.write(b">q%05d\n" % i + letters[codes].tobytes() + b"\n")
            fl.write(path + "\n")
    log("queries: %d genomes of %d bases in %.1f s" % (queries, length, time.time() - t0))
    return db, lst, int(arr["num_kmers"].size)


def run(argv, env, limit):
    t0 = time.perf_counter()
    r = subprocess.run(argv, capture_output=True, text=True, env=env, timeout=limit)
    dt = time.perf_counter() - t0
    if r.returncode != 0:
        log(r.stderr[-2000:])
        sys.exit("a run ended with %d: nothing further is started" % r.returncode)
    return dt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-exe", default=None, help="kmer-db-amd built from the parent commit, for the arms a and b")
    ap.add_argument("--samples", type=int, default=10000)
    ap.add_argument("--clade-size", type=int, default=50)
    ap.add_argument("--length", type=int, default=100_000)
    ap.add_argument("--queries", type=int, default=1000)
    ap.add_argument("--k", type=int, default=18)
    ap.add_argument("--seed", type=int, default=20260929)
    ap.add_argument("--measure", default="jaccard")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--limit", type=float, default=300.0, help="seconds a single process may take")
    ap.add_argument("--tmp", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert args.runs >= 3, "three runs an arm at the least"
    old = args.parent_exe or THIS_EXE
    env = dict(os.environ)
    env.pop("KMDB_DISTANCE_DEVICE", None)
    dev_env = dict(env, KMDB_DISTANCE_DEVICE="1")
    res = {"samples": args.samples, "clade_size": args.clade_size, "length": args.length, "queries": args.queries, "k": args.k, "measure": args.measure,
           "arms_a_b_binary": "parent commit" if args.parent_exe else "THIS commit (no --parent-exe given)",
           "arms": {"a": "new2all; distance -host", "b": "new2all; distance with KMDB_DISTANCE_DEVICE=1", "c": "new2all -distance"}}
    with tempfile.TemporaryDirectory(dir=args.tmp) as td:
        db, lst, res["patterns"] = write_inputs(td, args.samples, args.clade_size, args.length, args.k, args.seed, args.queries)
        table = os.path.join(td, "counts.csv")
        outs = {arm: os.path.join(td, "out." + arm) for arm in "abc"}

        def arm(name):
            """-> seconds of the whole arm and of its parts"""
            if name == "c":
                t = run([THIS_EXE, "new2all", "-distance", args.measure, db, lst, outs["c"]], env, args.limit)
                return {"total_s": t}
            t1 = run([old, "new2all", db, lst, table], env, args.limit)
            t2 = run([old, "distance"] + (["-host"] if name == "a" else []) + [args.measure, table, outs[name]], env if name == "a" else dev_env, args.limit)
            return {"total_s": t1 + t2, "new2all_s": t1, "distance_s": t2}

        for name in "abc":                                            # the warm-up round; its files are the ones compared
            arm(name)
        res["table_bytes"] = os.path.getsize(table)
        res["output_bytes"] = os.path.getsize(outs["c"])
        want = open(outs["a"], "rb").read()
        res["equal"] = all(open(outs[name], "rb").read() == want for name in "bc")
        assert res["equal"], "the arms wrote different files"
        del want
        runs = {name: [] for name in "abc"}
        for i in range(args.runs):
            for name in "abc":
                runs[name].append(arm(name))
                log("run %d arm %s: %s" % (i, name, json.dumps(runs[name][-1])))
    res["runs"] = runs
    res["summary"] = {}
    for name in "abc":
        tot = [r["total_s"] for r in runs[name]]
        res["summary"][name] = {"median_s": round(statistics.median(tot), 4), "min_s": round(min(tot), 4), "max_s": round(max(tot), 4)}
    med = {name: res["summary"][name]["median_s"] for name in "abc"}
    res["c_over_a"] = round(med["c"] / med["a"], 4)
    res["c_over_b"] = round(med["c"] / med["b"], 4)
    res["c_beats_b"] = res["summary"]["c"]["max_s"] < res["summary"]["b"]["min_s"]      # beyond the spread of both
    text = json.dumps(res, indent=1)
    if args.out:
        open(args.out, "w").write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
