"""A/B of `new2all -sample-rows <criterion>:<count>` against the sparse table it is cut from and against the host sampler.  README has the figures.

    git worktree add <scratch>/parent HEAD~1 && make -C <scratch>/parent/kmer-db_amd -j8
    python profiles/new2all_sampled_ab.py --parent-exe <scratch>/parent/kmer-db_amd/bin/kmer-db-amd --out profiles/new2all_sampled_ab.json

The input is that of profiles/new2all_distance_ab.py (its write_inputs): --samples samples (10 000, the genome parameters of bench.py's c5part
workload) through kmer-db_amd/synth.py, written once in the reference's format with its hashtables, and --queries queries (1 000), fresh
strains of 20 of its clades, one FASTA file each.  Three arms, each END TO END as a user runs it — one process, wall clock, the device's first
use, the database read and upload, the genomes read and the file written included:

    a  the parent's `new2all -sparse D Q out`                     every non-zero cell leaves HBM and is written
    b  this commit's `new2all -sample-rows <criterion>:<count> D Q out`
    c  arm b with KMDB_N2A_HOST_SAMPLER=1                          the filtered sparse rows leave HBM, the host's sampler cuts them

One warm-up round, then --runs rounds (5) in which the arms ALTERNATE (a b c, a b c, ...), all in this one call; every process runs under its
own time limit and a process that faults, aborts or runs out of time ends the script.  The files of b and c are compared equal before
anything is timed (a writes another file: the uncut table).  b runs with KMDB_VERBOSE=1 so that its per-batch lines give the selection's
HIP-event time and the candidates that left the device.  Without --parent-exe arm a runs this commit's binary and the json says so.  The
json gives every run, the median and the spread (min, max) per arm, the ratios, and whether b beats c beyond the spread of both."""
import argparse
import json
import os
import re
import statistics
import subprocess
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from new2all_distance_ab import THIS_EXE, log, write_inputs  # noqa: E402

LINE = re.compile(r"sampled batch of (\d+) queries: (\d+) candidates, (\d+) rows truncated, (\d+) fetched again, select ([0-9.eE+-]+) ms, (\d+) bytes to the host")


def run(argv, env, limit):
    """-> (seconds, stderr); a run that fails ends the script"""
    t0 = time.perf_counter()
    r = subprocess.run(argv, capture_output=True, text=True, env=env, timeout=limit)
    dt = time.perf_counter() - t0
    if r.returncode != 0:
        log(r.stderr[-2000:])
        sys.exit("a run ended with %d: nothing further is started" % r.returncode)
    return dt, r.stderr


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-exe", default=None, help="kmer-db-amd built from the parent commit, for arm a")
    ap.add_argument("--samples", type=int, default=10000)
    ap.add_argument("--clade-size", type=int, default=50)
    ap.add_argument("--length", type=int, default=100_000)
    ap.add_argument("--queries", type=int, default=1000)
    ap.add_argument("--k", type=int, default=18)
    ap.add_argument("--seed", type=int, default=20260929)
    ap.add_argument("--sample-rows", default="jaccard:10")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--limit", type=float, default=300.0, help="seconds a single process may take")
    ap.add_argument("--tmp", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert args.runs >= 3, "three runs an arm at the least"
    old = args.parent_exe or THIS_EXE
    env = dict(os.environ)
    for name in ("KMDB_N2A_HOST_SAMPLER", "KMDB_N2A_DENSE_ROWS", "KMDB_VERBOSE"):
        env.pop(name, None)
    res = {"samples": args.samples, "clade_size": args.clade_size, "length": args.length, "queries": args.queries, "k": args.k, "sample_rows": args.sample_rows,
           "arm_a_binary": "parent commit" if args.parent_exe else "THIS commit (no --parent-exe given)",
           "arms": {"a": "new2all -sparse", "b": "new2all -sample-rows " + args.sample_rows, "c": "b with KMDB_N2A_HOST_SAMPLER=1"}}
    with tempfile.TemporaryDirectory(dir=args.tmp) as td:
        db, lst, res["patterns"] = write_inputs(td, args.samples, args.clade_size, args.length, args.k, args.seed, args.queries)
        outs = {arm: os.path.join(td, "out." + arm) for arm in "abc"}

        def arm(name):
            if name == "a":
                return {"total_s": run([old, "new2all", "-sparse", db, lst, outs["a"]], env, args.limit)[0]}
            e = dict(env, KMDB_VERBOSE="1") if name == "b" else dict(env, KMDB_N2A_HOST_SAMPLER="1")
            t, err = run([THIS_EXE, "new2all", "-sample-rows", args.sample_rows, db, lst, outs[name]], e, args.limit)
            out = {"total_s": t}
            if name == "b":
                m = [x.groups() for x in map(LINE.search, err.splitlines()) if x]
                assert m, "arm b printed no line of the device path"
                out.update(batches=len(m), candidates=sum(int(x[1]) for x in m), rows_truncated=sum(int(x[2]) for x in m), rows_refetched=sum(int(x[3]) for x in m),
                           select_ms=round(sum(float(x[4]) for x in m), 4), d2h_bytes=sum(int(x[5]) for x in m))
            return out

        for name in "abc":                                            # the warm-up round; its files are the ones compared
            arm(name)
        res["output_bytes"] = {name: os.path.getsize(outs[name]) for name in "abc"}
        res["equal_b_c"] = open(outs["b"], "rb").read() == open(outs["c"], "rb").read()
        assert res["equal_b_c"], "the device path and the host sampler wrote different files"
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
    res["b_over_a"] = round(med["b"] / med["a"], 4)
    res["b_over_c"] = round(med["b"] / med["c"], 4)
    res["b_beats_c"] = res["summary"]["b"]["max_s"] < res["summary"]["c"]["min_s"]      # beyond the spread of both
    res["c_beats_b"] = res["summary"]["c"]["max_s"] < res["summary"]["b"]["min_s"]
    text = json.dumps(res, indent=1)
    if args.out:
        open(args.out, "w").write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
