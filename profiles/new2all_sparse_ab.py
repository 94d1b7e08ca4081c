"""A/B of `new2all -sparse`: the front-end of the PARENT commit (dense rows from kmdb_new2all_batch[_seq_alphabet], every cell of the nq x N rows
copied to the host and filtered there on one thread) against this one (the rows are compacted and filtered on the device,
kmdb_new2all_batch[_seq_alphabet]_sparse_filtered).  DESIGN section 4 has the table.

    git worktree add /tmp/parent HEAD~1 && make -C /tmp/parent/kmer-db_amd -j8
    python profiles/new2all_sparse_ab.py --parent-exe /tmp/parent/kmer-db_amd/bin/kmer-db-amd --out profiles/new2all_sparse_ab.json

The parent side is ALWAYS the parent commit's own binary, never this tree's KMDB_N2A_DENSE_ROWS switch.  Two shapes, each run without a bound
and with `-min jaccard:0.3`:
  c5part  `bench.py`'s c5part: 10 000 x 0.1 Mbp genomes, clades of 50, r1 = 0.10, 1000 queries (fresh strains of 20 clades): rows mostly non-zero
  sparse  a collection whose clade roots are independent (r1 = 0.75, c4sparse's model at a sample count that fits the sitting), written with
          hashtables, a few hundred queries: a query touches its own clade only
Both front-ends run as processes on the same files, in alternation, --runs times each; per run: the wall clock of "Processing queries" (the
front-end's own "Total:" line), the process's wall clock and its peak RSS (wait4).  In process, on this commit: kmdb_new2all_sparse_stats
(d2h_bytes, compact_ms, cells off the device / kept) and kernel_ms of the sparse call per batch of 64 queries, as the front-end cuts them, and
kernel_ms of the dense call; the parent's bytes to the host are the rows, 4 nq N.  The two outputs must be equal byte for byte.  Nothing is
judged against a threshold fixed in advance: the json states the spread of the parent's runs and whether this commit's median lies within it."""
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
SHAPES = {
    "c5part": dict(dict(k=18, r1=0.10), **bench.WORKLOADS["c5part"]),
    "sparse": dict(samples=20000, clade_size=50, length=30_000, k=18, r1=0.75, queries=300),
}
BOUNDS = {"plain": [], "minj": ["-min", "jaccard:0.3"]}
BATCH = 64                                                      # queries per batch of the front-end (host/main.cpp)


def run_cli(exe, args):
    """one front-end process: its "Total:" line (the wall clock of "Processing queries"), the process's wall clock, and the peak RSS from the
    kernel's accounting of that child (wait4)"""
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
    m = re.search(r"^Total: ([0-9.eE+-]+)", stderr, re.M)
    return {"queries_s": float(m.group(1)) if m else None, "wall_s": wall, "peak_rss_mb": ru.ru_maxrss / 1024.0}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-exe", default=None, help="kmer-db-amd built from the parent commit (without it only this commit is measured)")
    ap.add_argument("--shapes", default="c5part,sparse")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--seed", type=int, default=20260928 + 1)
    ap.add_argument("--tmp", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "new2all_sparse_ab.json"))
    args = ap.parse_args()
    import torch
    from _kmerdb_loader import import_kmerdb_amd
    K = import_kmerdb_amd()
    S = importlib.import_module("kmerdb_amd.synth")
    device = torch.device("cuda", args.device)
    exes = {"this": os.path.join(ROOT, "kmer-db_amd", "bin", "kmer-db-amd")}
    if args.parent_exe:
        exes["parent"] = args.parent_exe
    acgt = np.frombuffer(b"ACGT", np.uint8)
    res = {"runs_per_side": args.runs, "shapes": {}}
    for name in args.shapes.split(","):
        wl = SHAPES[name]
        N, k, NQ, cs = wl["samples"], wl["k"], wl["queries"], wl["clade_size"]
        g = S.CladeGenomes(N, cs, wl["length"], r1=wl["r1"], seed=args.seed, device=device)
        shape = {"workload": "%d synthetic %g Mbp genomes (clades of %d, r1=%g), k=%d, with hashtables; %d queries (fresh strains of 20 clades), new2all -sparse" %
                             (N, wl["length"] / 1e6, cs, wl["r1"], k, NQ), "bounds": {}}
        with tempfile.TemporaryDirectory(dir=args.tmp) as td:
            t0 = time.time()
            pat = S.build_patterns(lambda i: S.kmers_of(g.sample(i), k), N, device, progress=None)
            arr = S.to_view_arrays(pat)
            tables = S.build_hashtables(pat["dictionary"], pat["kmer_pid"], k)
            path = os.path.join(td, "db.db")
            S.write_db(path, k, 1.0, [g.name(i) for i in range(N)], pat["sample_counts"], arr, kmers_count=int(pat["dictionary"].numel()), tables=tables)
            del pat, arr, tables
            # the queries of bench.py's new2all workload: fresh strains of 20 clades, as FASTA files and as k-mer lists
            n_clades = max(1, N // cs)
            chosen = [int(c) for c in np.random.default_rng(args.seed + 1000).choice(n_clades, size=min(20, n_clades), replace=False)]
            qs, lst = [], os.path.join(td, "queries.list")
            with open(lst, "w") as fl:
                for i in range(NQ):
                    codes = g.strain(chosen[i * len(chosen) // NQ], N + i)
                    qs.append(S.kmers_of(codes, k).cpu().numpy().view(np.uint64).copy())
                    with open(os.path.join(td, "q%04d.fasta" % i), "w") as f:
                        f.write(">q%04d\n%s\n" % (i, acgt[codes.cpu().numpy()].tobytes().decode()))
                    fl.write(os.path.join(td, "q%04d" % i) + "\n")
            bench.release_generator_memory(0)
            log("%s: database and %d queries in %.1f s" % (name, NQ, time.time() - t0))
            h = K.HostDB(path)
            d = K.DeviceDB(h, device=args.device, with_hashtables=True)
            cnt = h.sample_kmers.astype(np.uint32)
            d.new2all(qs[:2])                                    # (the first call on a handle builds its run index)
            for tag, opt in BOUNDS.items():
                filters = [("jaccard", 0.3, None)] if opt else []
                out = {"runs": {s: [] for s in exes}}
                # in process, batch by batch as the front-end cuts them
                ip = {"d2h_bytes": 0, "compact_ms": 0.0, "kernel_ms": 0.0, "dense_kernel_ms": 0.0, "cells": 0, "nnz_device": 0, "nnz": 0}
                for b in range(0, NQ, BATCH):
                    d.new2all_sparse_filtered(qs[b:b + BATCH], filters, cnt if filters else None)
                    st = d.new2all_sparse_stats()
                    for f in ("d2h_bytes", "compact_ms", "cells", "nnz_device", "nnz"):
                        ip[f] += st[f]
                    ip["kernel_ms"] += d.stats()["kernel_ms"]
                    d.new2all(qs[b:b + BATCH])
                    ip["dense_kernel_ms"] += d.stats()["kernel_ms"]
                out["in_process"] = dict(ip, parent_d2h_bytes=4 * NQ * N)
                outs = {}
                for r in range(args.runs):
                    for side, exe in exes.items():
                        csv = os.path.join(td, side + ".csv")
                        out["runs"][side].append(run_cli(exe, ["new2all", "-sparse"] + opt + [path, lst, csv]))
                        log(name, tag, side, json.dumps(out["runs"][side][-1]))
                        with open(csv, "rb") as f:
                            outs[side] = f.read()
                        os.unlink(csv)
                if len(outs) == 2:
                    assert outs["parent"] == outs["this"], "the two front-ends wrote different files"
                    out["outputs_equal"] = True
                for side in exes:
                    w = [x["queries_s"] if x["queries_s"] is not None else x["wall_s"] for x in out["runs"][side]]
                    out[side] = {"queries_s_median": float(np.median(w)), "queries_s_min": min(w), "queries_s_max": max(w), "queries_s_spread": max(w) - min(w),
                                 "peak_rss_mb_median": float(np.median([x["peak_rss_mb"] for x in out["runs"][side]]))}
                out["this"].update(d2h_bytes=int(ip["d2h_bytes"]), compact_ms=ip["compact_ms"], kernel_ms=ip["kernel_ms"])
                if "parent" in out:
                    out["parent"].update(d2h_bytes=4 * NQ * N, kernel_ms=ip["dense_kernel_ms"])
                    out["found"] = {"bytes_to_host_fall": out["this"]["d2h_bytes"] < out["parent"]["d2h_bytes"],
                                    "peak_rss_falls": out["this"]["peak_rss_mb_median"] < out["parent"]["peak_rss_mb_median"],
                                    "wall_within_parent_spread": out["this"]["queries_s_median"] - out["parent"]["queries_s_median"] <= out["parent"]["queries_s_spread"]}
                shape["bounds"][tag] = out
            d.close()
            h.close()
        res["shapes"][name] = shape
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
