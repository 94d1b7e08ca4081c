"""A/B of `all2all-sp -sample-rows jaccard:10` at the 10 000-sample shape bench.py builds for extra.c3part: the front-end of the PARENT commit
(the whole filtered CSR crosses PCIe and every pair sits twice in the host sampler) against this one (candidates selected on the device,
csrc/sample_rows.hip).  DESIGN section 4 has the table.

    git worktree add /tmp/parent HEAD~1 && make -C /tmp/parent/kmer-db_amd -j8
    python profiles/sample_rows_ab.py --parent-exe /tmp/parent/kmer-db_amd/bin/kmer-db-amd --out profiles/sample_rows_ab.json

Both front-ends run as processes on the same database file, in alternation; reported per side: the seconds of the "Calculating" and "Storing"
phases (the front-end's own clock), the peak RSS of the process (getrusage of the child) and the bytes that crossed device -> host (parent:
the CSR it receives = 8 B per non-zero cell + row pointers, from its "No. saved pairs"-independent unsampled run; this commit:
kmdb_sample_stats.d2h_bytes).  In process, on this commit: the selection's HIP-event ms next to the call's kernel_ms, and the reads of the
triangle.  The two outputs must be equal byte for byte; everything else is reported, not judged."""
import argparse
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


def run_cli(exe, args):
    """one front-end process: phases from its stderr, peak RSS from the kernel's accounting of that child (wait4)"""
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
    secs = [float(x) for x in re.findall(r"OK \(([0-9.eE+-]+) seconds\)", stderr)]
    m = re.search(r"\((\d+) candidates, (\d+) rows truncated, (\d+) fetched again, selection ([0-9.eE+-]+) ms, (\d+) bytes to the host\)", stderr)
    out = {"wall_s": wall, "calculating_s": secs[0] if secs else None, "storing_s": secs[1] if len(secs) > 1 else None,
           "peak_rss_mb": ru.ru_maxrss / 1024.0}
    if m:
        out.update(candidates=int(m.group(1)), rows_truncated=int(m.group(2)), rows_refetched=int(m.group(3)), select_ms=float(m.group(4)), d2h_bytes=int(m.group(5)))
    saved = re.search(r"No. saved pairs: (\d+)", stderr)
    out["saved_pairs"] = int(saved.group(1)) if saved else None
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-exe", default=None, help="kmer-db-amd built from the parent commit (without it only this commit is measured)")
    ap.add_argument("--workload", default="c3part")
    ap.add_argument("--sample-rows", default="jaccard:10")
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--k", type=int, default=18)
    ap.add_argument("--seed", type=int, default=20260928)
    ap.add_argument("--tmp", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sample_rows_ab.json"))
    args = ap.parse_args()
    import torch
    from _kmerdb_loader import import_kmerdb_amd
    K = import_kmerdb_amd()
    import importlib
    S = importlib.import_module("kmerdb_amd.synth")
    wl = bench.WORKLOADS[args.workload]
    device = torch.device("cuda", args.device)
    arr, names, counts, nk, _ = bench.generate_in_child(args.device, n_samples=wl["samples"], clade_size=wl["clade_size"], length=wl["length"], k=args.k,
                                                        seed=args.seed, rank=0, world=1)
    bench.release_generator_memory(0)
    N = wl["samples"]
    criterion, count = args.sample_rows.split(":")
    res = {"workload": "%s: %d synthetic %g Mbp genomes (clades of %d), k=%d, all2all-sp -sample-rows %s" % (args.workload, N, wl["length"] / 1e6, wl["clade_size"], args.k, args.sample_rows),
           "pairs": N * (N - 1) // 2, "runs": {"parent": [], "this": []}}
    with tempfile.TemporaryDirectory(dir=args.tmp) as td:
        path = os.path.join(td, "full.db")
        S.write_db_fast(path, args.k, 1.0, names, counts, arr, kmers_count=nk, device=device)
        # in process: the selection next to the accumulation
        h = K.HostDB(path, skip_hashtables=True)
        db = K.DeviceDB(h, device=args.device)
        kmers = h.sample_kmers
        inproc = []
        for _ in range(args.rounds + 1):
            rows = db.all2all_sampled(criterion, int(count), kmers)
            st, ss = db.stats(), db.sample_stats()
            inproc.append({"kernel_ms": st["kernel_ms"], "accumulate_ms": st["k0_ms"] + st["k1_ms"] + st["k2_ms"], "select_ms": ss["select_ms"],
                           "triangle_reads": ss["triangle_reads"], "candidates": ss["candidates"], "rows_truncated": ss["rows_truncated"],
                           "rows_refetched": ss["rows_refetched"], "d2h_bytes": ss["d2h_bytes"], "rows_nnz": rows.nnz})
        sp = db.all2all_sparse()
        res["nnz"] = int(sp.nnz)
        res["parent_d2h_bytes"] = int(sp.nnz) * 8 + (N + 1) * 8      # what kmdb_all2all_sparse copies back: col + val per non-zero cell, row pointers
        res["parent_sampler_bytes"] = int(sp.nnz) * 2 * 16            # every pair twice, 16 B per item, until its row is written
        del sp
        db.close()
        h.close()
        res["in_process"] = inproc[1:]                                # (the first call sizes its launches)
        exes = {"this": os.path.join(ROOT, "kmer-db_amd", "bin", "kmer-db-amd")}
        if args.parent_exe:
            exes["parent"] = args.parent_exe
        outs = {}
        for r in range(args.rounds):
            for side, exe in exes.items():
                csv = os.path.join(td, side + ".csv")
                res["runs"][side].append(run_cli(exe, ["all2all-sp", "-sample-rows", args.sample_rows, path, csv]))
                log(side, json.dumps(res["runs"][side][-1]))
                with open(csv, "rb") as f:
                    outs[side] = f.read()
                os.unlink(csv)
        if len(outs) == 2:
            assert outs["parent"] == outs["this"], "the two front-ends wrote different files"
            res["outputs_equal"] = True
    for side in ("parent", "this"):
        runs = res["runs"][side]
        if runs:
            res[side + "_median"] = {k: float(np.median([x[k] for x in runs])) for k in ("calculating_s", "storing_s", "wall_s", "peak_rss_mb")}
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
