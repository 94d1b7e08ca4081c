"""A/B of the `distance` mode: the front-end of the PARENT commit (the host loop: one thread, one line at a time) against this one with
KMDB_DISTANCE_DEVICE=1 (the table parsed, measured and formatted on the device, kmdb_distance_*).  DESIGN section 4 has the paragraph.

    git worktree add <scratch>/parent HEAD~1 && make -C <scratch>/parent/kmer-db_amd -j8
    python profiles/distance_ab.py --parent-exe <scratch>/parent/kmer-db_amd/bin/kmer-db-amd --out profiles/distance_ab.json

The parent side is ALWAYS the parent commit's own binary, never this tree's -host switch.  The tables are written by numpy, no database is
needed: a dense triangle of --samples samples (10 000: about 50 M cells), its whole-matrix form at 0.4 x --samples rows, a sparse triangle
of about as many pairs; and, for the threshold, dense triangles of about 1, 8, 64 and 512 MiB.  Measures: jaccard and mash.  Each side runs
once after one warm-up run, as a process (so the device's first use is inside this commit's wall clock), each under its own time limit; a
side that faults, aborts or runs out of time ends the script.  The two outputs must be equal byte for byte.  From this commit's stderr
(KMDB_VERBOSE) come the stage times of kmdb_distance_stats and the share of the cells the host decided.  The json states the figures and,
from the four sizes, `min_bytes_default`: twice the smallest size at which the device path won, rounded up to a power of two (null: it won
at none)."""
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
THIS_EXE = os.path.join(ROOT, "kmer-db_amd", "bin", "kmer-db-amd")


def log(*a):
    print(*a, file=sys.stderr, flush=True)


def write_table(path, rng, n, rows, form):
    """form: triangle (row r holds r cells), whole (rows x n), sparse (triangle, pairs of the non-zero third of the cells)"""
    counts = rng.integers(3_000_000, 6_000_000, n)
    with open(path, "wb") as f:
        f.write(b"kmer-length: 18 fraction: 1 ,db-samples ," + b"".join(b"s%d," % i for i in range(n)) + b"\n")
        f.write(b"query-samples,total-kmers," + b"".join(b"%d," % c for c in counts) + b"\n")
        cells = 0
        for r in range(rows):
            width = n if form == "whole" else r
            v = rng.integers(1000, 3_000_000, width)
            if form == "sparse":
                cols = np.flatnonzero(rng.random(width) < 1.0 / 3) + 1
                body = b"".join(b"%d:%d," % (c, x) for c, x in zip(cols.tolist(), v[cols - 1].tolist()))
                cells += cols.size
            else:
                body = b",".join(b"%d" % x for x in v.tolist()) + (b"," if width else b"")
                cells += width
            f.write(b"s%d,%d," % (r, counts[r % n]) + body + b"\n")
    return cells


def run(exe, args, env, limit):
    t0 = time.perf_counter()
    r = subprocess.run([exe] + args, capture_output=True, text=True, env=env, timeout=limit)
    dt = time.perf_counter() - t0
    if r.returncode != 0:
        log(r.stderr[-2000:])
        sys.exit("a run ended with %d: nothing further is started" % r.returncode)
    return dt, r.stderr


def stats_of(stderr):
    keys = ("rows", "cells_read", "cells_written", "host_cells", "bytes_in", "bytes_out", "parse_ms", "measure_ms", "format_ms", "copy_ms")
    pat = (r"distance on the device: calls \d+, rows (\d+), cells read (\d+), cells written (\d+), host cells (\d+), bytes in (\d+), bytes out (\d+), "
           r"parse ([\d.e+-]+) ms, measure ([\d.e+-]+) ms, format ([\d.e+-]+) ms, copies ([\d.e+-]+) ms")
    tot = dict.fromkeys(keys, 0.0)
    for m in re.findall(pat, stderr):
        for k, v in zip(keys, m):
            tot[k] += float(v)
    tot["host_share"] = tot["host_cells"] / tot["cells_written"] if tot["cells_written"] else None
    return tot


def ab(table, opts, measure, parent_exe, limit, td):
    out = {"opts": opts + [measure], "table_bytes": os.path.getsize(table)}
    files = {}
    for side, exe, env in (("parent", parent_exe, dict(os.environ)), ("device", THIS_EXE, dict(os.environ, KMDB_DISTANCE_DEVICE="1", KMDB_VERBOSE="1"))):
        if exe is None:
            continue
        files[side] = os.path.join(td, "out." + side)
        for attempt in ("warm-up", "timed"):
            dt, err = run(exe, ["distance"] + opts + [measure, table, files[side]], env, limit)
        out[side + "_s"] = round(dt, 4)
        if side == "device":
            out["declined"] = "declined" in err
            out["stats"] = stats_of(err)
    if len(files) == 2:
        out["equal"] = open(files["parent"], "rb").read() == open(files["device"], "rb").read()
        assert out["equal"], "the two front-ends wrote different files"
        out["device_wins"] = out["device_s"] < out["parent_s"]
    log(json.dumps(out))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-exe", default=None, help="kmer-db-amd built from the parent commit (without it only this commit is measured)")
    ap.add_argument("--samples", type=int, default=10000)
    ap.add_argument("--sizes-mib", default="1,8,64,512")
    ap.add_argument("--limit", type=float, default=600.0, help="seconds a single run may take")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    rng = np.random.default_rng(1)
    res = {"samples": args.samples, "big": [], "sizes": []}
    with tempfile.TemporaryDirectory() as td:
        n = args.samples
        for form, rows in (("triangle", n), ("whole", int(0.4 * n)), ("sparse", n)):
            table = os.path.join(td, form + ".csv")
            cells = write_table(table, rng, n, rows, form)
            for measure in ("jaccard", "mash"):
                res["big"].append(dict(ab(table, [], measure, args.parent_exe, args.limit, td), form=form, cells=int(cells)))
            os.remove(table)
        for mib in [float(x) for x in args.sizes_mib.split(",")]:
            m = max(2, int((2 * mib * (1 << 20) / 7.9) ** 0.5))          # a triangle of m samples: m^2 / 2 cells of about 7.9 bytes
            table = os.path.join(td, "size.csv")
            cells = write_table(table, rng, m, m, "triangle")
            for measure in ("jaccard", "mash"):
                res["sizes"].append(dict(ab(table, [], measure, args.parent_exe, args.limit, td), target_mib=mib, samples=m, cells=int(cells)))
            os.remove(table)
    won = sorted(r["table_bytes"] for r in res["sizes"] if r.get("device_wins"))
    lost = [r["table_bytes"] for r in res["sizes"] if r.get("device_wins") is False]
    smallest = next((b for b in won if all(x < b for x in lost)), None)     # the smallest size from which the device path wins throughout
    res["min_bytes_default"] = None if smallest is None else 1 << (2 * smallest - 1).bit_length()
    text = json.dumps(res, indent=1)
    if args.out:
        open(args.out, "w").write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
