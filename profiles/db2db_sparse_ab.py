"""A/B of `all2all-parts` over two part databases: the front-end of the PARENT commit (every off-diagonal cell comes to the host as a dense
rectangle from kmdb_db2db_dense and is scanned there) against this one (the cell is compacted and filtered on the device,
kmdb_db2db_sparse_filtered).  DESIGN section 4 has the table.

    git worktree add /tmp/parent HEAD~1 && make -C /tmp/parent/kmer-db_amd -j8
    python profiles/db2db_sparse_ab.py --parent-exe /tmp/parent/kmer-db_amd/bin/kmer-db-amd --out profiles/db2db_sparse_ab.json

The parent side is ALWAYS the parent commit's own binary, never this tree's KMDB_PARTS_DENSE_CELLS switch.  Two splits:
  parts   the two parts `bench.py --mode db2db` uses: 2000 x 0.3 Mbp genomes, clades of 50, r1 = 0.10, even / odd ids (every cell non-zero)
  sparse  two 5000-sample parts (even / odd ids) of a collection whose clade roots are independent (r1 = 0.75): only cells inside a clade are non-zero
Both front-ends run as processes on the same files, in alternation, --runs times each; per run: wall clock and the peak RSS of the process
(wait4).  In process, on this commit: kmdb_db2db_stats (d2h_bytes, compact_ms, tiles) and kernel_ms of the sparse call, kernel_ms of the dense
call; the parent's bytes to the host are the rectangle, 4 nr nc.  The two outputs must be equal byte for byte.  Nothing is judged against a
threshold fixed in advance: the json states the spread of the parent's runs and whether this commit's median wall clock lies within it."""
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
SPLITS = {
    "parts": dict(dict(k=18, r1=0.10), **bench.WORKLOADS["parts"]),
    "sparse": dict(samples=10000, clade_size=50, length=30_000, k=18, r1=0.75),
}


def run_cli(exe, args):
    """one front-end process: wall clock, and the peak RSS from the kernel's accounting of that child (wait4)"""
    t0 = time.time()
    with tempfile.TemporaryFile(mode="w+") as err:
        p = subprocess.Popen([exe] + args, stdout=subprocess.DEVNULL, stderr=err)
        _, status, ru = os.wait4(p.pid, 0)
        p.returncode = os.waitstatus_to_exitcode(status)
        err.seek(0)
        stderr = err.read()
    wall = time.time() - t0
    if p.returncode != 0:
        raise SystemExit("front-end failed: " + stderr[-2000:])
    return {"wall_s": wall, "peak_rss_mb": ru.ru_maxrss / 1024.0}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-exe", default=None, help="kmer-db-amd built from the parent commit (without it only this commit is measured)")
    ap.add_argument("--splits", default="parts,sparse")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--seed", type=int, default=20260928 + 1)
    ap.add_argument("--tmp", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "db2db_sparse_ab.json"))
    args = ap.parse_args()
    import torch
    from _kmerdb_loader import import_kmerdb_amd
    K = import_kmerdb_amd()
    S = importlib.import_module("kmerdb_amd.synth")
    device = torch.device("cuda", args.device)
    exes = {"this": os.path.join(ROOT, "kmer-db_amd", "bin", "kmer-db-amd")}
    if args.parent_exe:
        exes["parent"] = args.parent_exe
    res = {"runs_per_side": args.runs, "splits": {}}
    for name in args.splits.split(","):
        wl = SPLITS[name]
        N, k = wl["samples"], wl["k"]
        g = S.CladeGenomes(N, wl["clade_size"], wl["length"], r1=wl["r1"], seed=args.seed, device=device)
        out = {"workload": "%d synthetic %g Mbp genomes (clades of %d, r1=%g), k=%d, two parts of even / odd ids, all2all-parts" %
                           (N, wl["length"] / 1e6, wl["clade_size"], wl["r1"], k), "runs": {s: [] for s in exes}}
        with tempfile.TemporaryDirectory(dir=args.tmp) as td:
            paths = []
            t0 = time.time()
            for tag, ids in (("a", list(range(0, N, 2))), ("b", list(range(1, N, 2)))):
                pat = S.build_patterns(lambda i: S.kmers_of(g.sample(ids[i]), k), len(ids), device, progress=None)
                arr = S.to_view_arrays(pat)
                tables = S.build_hashtables(pat["dictionary"], pat["kmer_pid"], k)
                paths.append(os.path.join(td, tag + ".db"))
                S.write_db(paths[-1], k, 1.0, [g.name(i) for i in ids], pat["sample_counts"], arr, kmers_count=int(pat["dictionary"].numel()), tables=tables)
                del pat, arr, tables
            bench.release_generator_memory(0)
            log("%s: two part databases in %.1f s" % (name, time.time() - t0))
            lst = os.path.join(td, "parts.list")
            with open(lst, "w") as f:
                f.write("".join(p + "\n" for p in paths))
            # in process: the cell (part b = rows, part a = columns), sparse and dense entry
            ha, hb = K.HostDB(paths[0]), K.HostDB(paths[1])
            da, db = K.DeviceDB(ha, device=args.device, with_hashtables=True), K.DeviceDB(hb, device=args.device, with_hashtables=True)
            nr, nc = db.N, da.N
            inproc = []
            for _ in range(args.runs + 1):
                sp = db.db2db_sparse(da)
                st = dict(db.db2db_stats(), kernel_ms=db.stats()["kernel_ms"])
                db.db2db(da)
                st["dense_kernel_ms"] = db.stats()["kernel_ms"]
                inproc.append(st)
            out["cell"] = {"rows": nr, "cols": nc, "nnz": int(sp.nnz), "parent_d2h_bytes": 4 * nr * nc, "in_process": inproc[1:]}      # (the first call builds the list stores)
            del sp
            da.close(); db.close(); ha.close(); hb.close()
            outs = {}
            for r in range(args.runs):
                for side, exe in exes.items():
                    csv = os.path.join(td, side + ".csv")
                    out["runs"][side].append(run_cli(exe, ["all2all-parts", lst, csv]))
                    log(name, side, json.dumps(out["runs"][side][-1]))
                    with open(csv, "rb") as f:
                        outs[side] = f.read()
                    os.unlink(csv)
            if len(outs) == 2:
                assert outs["parent"] == outs["this"], "the two front-ends wrote different files"
                out["outputs_equal"] = True
        for side in exes:
            w = [x["wall_s"] for x in out["runs"][side]]
            out[side] = {"wall_s_median": float(np.median(w)), "wall_s_min": min(w), "wall_s_max": max(w), "wall_s_spread": max(w) - min(w),
                         "peak_rss_mb_median": float(np.median([x["peak_rss_mb"] for x in out["runs"][side]]))}
        ip = out["cell"]["in_process"]
        out["this"].update(d2h_bytes=int(ip[-1]["d2h_bytes"]), compact_ms_median=float(np.median([x["compact_ms"] for x in ip])),
                           kernel_ms_median=float(np.median([x["kernel_ms"] for x in ip])))
        if "parent" in out:
            out["parent"].update(d2h_bytes=out["cell"]["parent_d2h_bytes"], kernel_ms_median=float(np.median([x["dense_kernel_ms"] for x in ip])))
            out["claim"] = {"bytes_to_host_fall": out["this"]["d2h_bytes"] < out["parent"]["d2h_bytes"],
                            "peak_rss_falls": out["this"]["peak_rss_mb_median"] < out["parent"]["peak_rss_mb_median"],
                            "wall_within_parent_spread": out["this"]["wall_s_median"] - out["parent"]["wall_s_median"] <= out["parent"]["wall_s_spread"]}
        res["splits"][name] = out
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
