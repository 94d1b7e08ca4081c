"""A/B of the three fused -distance forms across a refactor of their shared plumbing: the PARENT commit's front-end and library against this
commit's, the same command in both, end to end as processes.

    git worktree add <scratch>/parent HEAD~1 && make -C <scratch>/parent/kmer-db_amd -j8
    python profiles/distance_refactor_ab.py --parent-exe <scratch>/parent/kmer-db_amd/bin/kmer-db-amd --out profiles/distance_refactor_ab.json

    all2all        `all2all -distance jaccard D out`            the database of profiles/all2all_distance_ab.py (10 000 samples)
    new2all        `new2all -distance jaccard D Q out`          the database and the 1 000 queries of profiles/new2all_distance_ab.py
    all2all-parts  `all2all-parts -distance jaccard L out`      the 4 parts of 1 000 samples of profiles/parts_distance_ab.py

Per form: one warm-up run of each binary, whose two output files are compared byte for byte BEFORE anything is timed, then --rounds rounds (5
at least) in which the binaries alternate (parent, this, parent, this, ...).  Measured is the wall clock of the process, the device's first
use, the read and upload of the databases and the file written included.  Every process runs under its own time limit, and one that faults,
aborts or runs out of time ends the script.

The condition, per form: the median of this commit's runs lies within the parent's own range (min .. max) over the rounds, or below it.  It is
wall clock on a machine others use, so the parent's spread is the margin.  The json holds every run and `holds` per form."""
import argparse
import importlib
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import all2all_distance_ab as A2A  # noqa: E402
import new2all_distance_ab as N2A  # noqa: E402

THIS_EXE = A2A.THIS_EXE
log = A2A.log


def write_parts(td, parts, part_samples, k, seed):
    """the collection of profiles/parts_distance_ab.py: clade genomes at bench.py's c3part parameters, sample i in part i % parts -> the list file"""
    import torch

    import bench
    from _kmerdb_loader import import_kmerdb_amd
    import_kmerdb_amd()
    S = importlib.import_module("kmerdb_amd.synth")
    wl = bench.WORKLOADS["c3part"]
    device = torch.device("cuda:0")
    N = parts * part_samples
    g = S.CladeGenomes(N, wl["clade_size"], wl["length"], r1=0.10, seed=seed, device=device)
    paths = []
    for p in range(parts):
        ids = list(range(p, N, parts))
        pat = S.build_patterns(lambda i: S.kmers_of(g.sample(ids[i]), k), part_samples, device, progress=None)
        arr = S.to_view_arrays(pat)
        tables = S.build_hashtables(pat["dictionary"], pat["kmer_pid"], k)
        paths.append(os.path.join(td, "part%d.db" % p))
        S.write_db(paths[-1], k, 1.0, [g.name(i) for i in ids], pat["sample_counts"], arr, kmers_count=int(pat["dictionary"].numel()), tables=tables)
        del pat, arr, tables
    del g
    torch.cuda.empty_cache()
    lst = os.path.join(td, "db.list")
    with open(lst, "w") as f:
        f.write("\n".join(paths) + "\n")
    return lst


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-exe", required=True, help="kmer-db-amd built from the parent commit")
    ap.add_argument("--forms", default="all2all,new2all,all2all-parts")
    ap.add_argument("--measure", default="jaccard")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--limit", type=float, default=300.0, help="seconds a single process may take")
    ap.add_argument("--tmp", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "distance_refactor_ab.json"))
    args = ap.parse_args()
    assert args.rounds >= 5, "five rounds at the least"
    env = dict(os.environ)
    exes = {"parent": args.parent_exe, "this": THIS_EXE}
    res = {"measure": args.measure, "rounds": args.rounds, "measured": "wall clock of the process, end to end", "forms": {}}
    for form in args.forms.split(","):
        with tempfile.TemporaryDirectory(dir=args.tmp) as td:
            t0 = time.time()
            if form == "all2all":
                db = os.path.join(td, "db.db")
                A2A.write_database(db, 10000, 50, 300_000, 18, 20260929)
                inputs = [db]
            elif form == "new2all":
                db, lst, _ = N2A.write_inputs(td, 10000, 50, 100_000, 18, 20260929, 1000)
                inputs = [db, lst]
            else:
                inputs = [write_parts(td, 4, 1000, 18, 20260928)]
            log("%s: inputs written in %.1f s" % (form, time.time() - t0))
            outs = {who: os.path.join(td, "out." + who) for who in exes}

            def once(who):
                return A2A.run([exes[who], form, "-distance", args.measure] + inputs + [outs[who]], env, args.limit)

            for who in exes:                                          # the warm-up; its files are the ones compared
                once(who)
            want = open(outs["parent"], "rb").read()
            assert open(outs["this"], "rb").read() == want, form + ": the two binaries wrote different files"
            runs = {who: [] for who in exes}
            for i in range(args.rounds):
                for who in exes:
                    runs[who].append(round(once(who), 4))
                    log("%s round %d %s: %.4f s" % (form, i, who, runs[who][-1]))
            summary = {who: {"median_s": statistics.median(r), "min_s": min(r), "max_s": max(r)} for who, r in runs.items()}
            res["forms"][form] = {"command": form + " -distance " + args.measure, "output_bytes": len(want), "outputs_equal": True, "runs_s": runs, "summary": summary,
                                  "this_over_parent": round(summary["this"]["median_s"] / summary["parent"]["median_s"], 4),
                                  "holds": summary["this"]["median_s"] <= summary["parent"]["max_s"]}
            del want
    res["condition"] = "the median of this commit's runs is not above the parent's slowest run of the same rounds"
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps({form: {k: v for k, v in r.items() if k != "runs_s"} for form, r in res["forms"].items()}))


if __name__ == "__main__":
    main()
