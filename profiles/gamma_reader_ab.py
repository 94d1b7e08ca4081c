#!/usr/bin/env python3
"""A/B of the merge of the 64-bit gamma readers (GammaCursor, gamma_first_id, gamma_runs in csrc/device_common.h): the PARENT commit's
libkmdb_amd.so against this tree's, on the calls whose kernels came out with other instruction text (profiles/gamma_reader_codeobject.md).

    git worktree add <scratch>/parent HEAD~1 && make -C <scratch>/parent/kmer-db_amd -j8
    python profiles/gamma_reader_ab.py --parent-lib <scratch>/parent/kmer-db_amd/libkmdb_amd.so --out profiles/gamma_reader_ab.json

    new2all   the shape of `bench.py --mode new2all` (c5part): the first call on a handle (it builds the run index: n2a_runs_kernel), the steady
              call (n2a_walk_kernel<*, RUNIDX>), and on a second handle under KMDB_N2A_NO_RUNS=1 the steady call from the checkpoints
              (ck_fill_kernel, the inline decode and the queued lists of n2a_walk_kernel<*, no RUNIDX>)
    db2db     the shape of `bench.py --mode db2db` (parts): the first call (the list store: d2_sets_round_kernel) and the steady call.  The
              steady call under KMDB_D2_NO_STORE=1 (d2_list_bits in d2_emit_kernel<*, false>) is NOT run any more: with gamma_first_id in
              d2_list_bits it was measured 2 % slower (the json keeps those runs under "reverted"), the first pass is written out there
              again and both instantiations are instruction-identical to the parent's
    upload    kmdb_db_upload of c2 (width_estimate_kernel, pair_estimate_kernel), three uploads per process; with it the sizing: the
              KMDB_VERBOSE estimate lines and the chosen block width at c2 and at gamma collection A (tests/gamma_cases.py).  NOT in the
              default lines any more: with gamma_first_id in the two kernels the wall clock of the upload passed in one run of the script
              and missed in the next (the json keeps both under "reverted", and the sizing); the first pass is written out there again
              and both kernels are instruction-identical to the parent's
    v1        a forced v1 all2all: NOT run, the five kernels of a2a_v1.hip are instruction-identical in both builds

Per line the inputs are generated once, by a process of its own, into --tmp.  Then one warm-up process per library, whose outputs (sha256) are
compared BEFORE anything is timed, and --rounds rounds (5 at least) in which the libraries alternate (parent, this, parent, this, ...).  Every
process runs under its own time limit; one that faults, aborts or runs out of time ends the script.

The condition, per figure: the median of this tree's runs is not above the parent's slowest run of the same rounds (within the parent's own
min .. max, or below it): a machine others use, so the parent's spread is the margin.  The json holds every run and `holds` per figure."""
import argparse
import hashlib
import importlib
import json
import os
import re
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SEED = 20260929
STEADY = 5
SIZING = re.compile(r"\[kmdb\] (width estimate|extra \(block, mask\) pairs|block records estimated|\d+ block records estimated)")


def log(*a):
    print("[gamma_reader_ab]", *a, file=sys.stderr, flush=True)


def _modules(libpath=None):
    import bench as B
    K = B.import_kmerdb_amd()
    if libpath is not None:
        importlib.import_module("kmerdb_amd.capi").lib_path = lambda: libpath
    return B, K, importlib.import_module("kmerdb_amd.synth")


def _save(d, name, arr, tables=None):
    import numpy as np
    for key, a in arr.items():
        np.save(os.path.join(d, "%s.%s.npy" % (name, key)), a)
    if tables is not None:
        np.save(os.path.join(d, name + ".bucket_offset.npy"), tables[0])
        np.save(os.path.join(d, name + ".slots.npy"), tables[1])


def _view(K, d, name, n, k=18):
    import numpy as np
    a = {f[len(name) + 1:-4]: np.load(os.path.join(d, f)) for f in os.listdir(d) if f.startswith(name + ".") and f.endswith(".npy")}
    return K.make_view(k, n, a["num_kmers"], a["parent_id"], a["num_samples"], a["num_local"], a["last_sample_id"], a["num_bits"], a["data_offset"],
                       a["data"], bucket_offset=a.get("bucket_offset"), slots=a.get("slots"))


def prepare(line, d):
    """the inputs of one line, as .npy files in d"""
    import numpy as np
    import torch
    B, K, S = _modules()
    device = torch.device("cuda", 0)
    if line == "upload":
        wl = B.WORKLOADS["c2"]
        arr = B.generate_in_child(0, n_samples=wl["samples"], clade_size=wl["clade_size"], length=wl["length"], k=18, seed=SEED, rank=0, world=1)[0]
        _save(d, "c2", arr)
        return
    wl = B.WORKLOADS["c5part" if line == "new2all" else "parts"]
    N, cs = wl["samples"], wl["clade_size"]
    g = S.CladeGenomes(N, cs, wl["length"], r1=0.10, seed=SEED, device=device)

    def make(ids):
        pat = S.build_patterns(lambda i: S.kmers_of(g.sample(ids[i]), 18, 1.0), len(ids), device, progress=None)
        return S.to_view_arrays(pat), S.build_hashtables(pat["dictionary"], pat["kmer_pid"], 18)

    if line == "new2all":
        _save(d, "db", *make(list(range(N))))
        NQ, n_clades = wl["queries"], max(1, N // cs)                      # fresh strains of 20 clades, as bench.py takes them
        chosen = [int(c) for c in np.random.default_rng(SEED + 1000).choice(n_clades, size=min(20, n_clades), replace=False)]
        qs = [S.kmers_of(g.strain(chosen[i * len(chosen) // NQ], N + i), 18, 1.0).cpu().numpy().view(np.uint64) for i in range(NQ)]
        np.save(os.path.join(d, "q.ptr.npy"), np.cumsum([0] + [q.size for q in qs]).astype(np.int64))
        np.save(os.path.join(d, "q.kmers.npy"), np.concatenate(qs))
    else:
        _save(d, "a", *make(list(range(0, N, 2))))
        _save(d, "b", *make(list(range(1, N, 2))))


def child(line, libpath, d):
    import numpy as np
    B, K, S = _modules(libpath)
    out, sha = {}, hashlib.sha256()

    def steady(fn, handle):
        fn()
        ms, wall = [], []
        for _ in range(STEADY):
            t0 = time.perf_counter()
            got = fn()
            wall.append((time.perf_counter() - t0) * 1e3)
            ms.append(handle.stats()["kernel_ms"])
        sha.update(np.ascontiguousarray(got).tobytes())
        return round(float(np.mean(ms)), 4), round(float(np.mean(wall)), 3)

    if line == "new2all":
        wl = B.WORKLOADS["c5part"]
        ptr, km = np.load(os.path.join(d, "q.ptr.npy")), np.load(os.path.join(d, "q.kmers.npy"))
        qs = [km[ptr[i]:ptr[i + 1]] for i in range(ptr.size - 1)]
        view = _view(K, d, "db", wl["samples"])
        h = K.DeviceDB(view, device=0, with_hashtables=True)
        t0 = time.perf_counter()
        sha.update(h.new2all(qs).tobytes())
        out["first_call_ms"] = round((time.perf_counter() - t0) * 1e3, 3)
        out["steady_ms"], out["steady_wall_ms"] = steady(lambda: h.new2all(qs), h)
        h.close()
        os.environ["KMDB_N2A_NO_RUNS"] = "1"
        h = K.DeviceDB(view, device=0, with_hashtables=True)
        out["no_runs_steady_ms"], out["no_runs_steady_wall_ms"] = steady(lambda: h.new2all(qs), h)
        h.close()
    elif line == "db2db":
        n = B.WORKLOADS["parts"]["samples"]
        da = K.DeviceDB(_view(K, d, "a", len(range(0, n, 2))), device=0, with_hashtables=True)
        db = K.DeviceDB(_view(K, d, "b", len(range(1, n, 2))), device=0, with_hashtables=True)
        t0 = time.perf_counter()
        sha.update(db.db2db(da).tobytes())
        out["first_call_ms"] = round((time.perf_counter() - t0) * 1e3, 3)
        out["steady_ms"], out["steady_wall_ms"] = steady(lambda: db.db2db(da), db)
        da.close(), db.close()
    else:
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import gamma_cases as G
        import variant_cases as V
        os.environ["KMDB_VERBOSE"] = "1"                                    # the driver reads the estimate lines from stderr
        view = _view(K, d, "c2", B.WORKLOADS["c2"]["samples"])
        ups = []
        for _ in range(3):
            t0 = time.perf_counter()
            h = K.DeviceDB(view, device=0)
            ups.append((time.perf_counter() - t0) * 1e3)
            out["c2_width"] = int(h.stats()["width"])
            h.close()
        out["upload_ms"] = round(statistics.median(ups), 3)
        print("[kmdb] ---- collection A", file=sys.stderr, flush=True)
        pat, _, N = G.collection("A")
        h = K.DeviceDB(V.make_view(K, S, pat, N)[1], device=0)
        out["A_width"] = int(h.stats()["width"])
        h.close()
        sha.update(b"%d %d" % (out["c2_width"], out["A_width"]))
    out["sha"] = sha.hexdigest()[:16]
    print("AB " + json.dumps(out), flush=True)


FIGURES = {"new2all": ("first_call_ms", "steady_ms", "no_runs_steady_ms"), "db2db": ("first_call_ms", "steady_ms"), "upload": ("upload_ms",)}


def main():
    if sys.argv[1] == "--prepare":
        return prepare(sys.argv[2], sys.argv[3])
    if sys.argv[1] == "--child":
        return child(sys.argv[2], sys.argv[3], sys.argv[4])
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", required=True, help="libkmdb_amd.so built from the parent commit")
    ap.add_argument("--lines", default="new2all,db2db")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--limit", type=int, default=240, help="seconds a single process may take")
    ap.add_argument("--tmp", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gamma_reader_ab.json"))
    args = ap.parse_args()
    assert args.rounds >= 5, "five rounds at the least"
    libs = {"parent": os.path.abspath(args.parent_lib), "this": os.path.join(ROOT, "kmer-db_amd", "libkmdb_amd.so")}
    me = os.path.abspath(__file__)

    def run(argv, limit):
        r = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, me] + argv, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
        if r.returncode != 0:
            sys.stderr.write(r.stderr[-4000:])
            raise SystemExit("gamma_reader_ab: %s ended with %d: stopping" % (argv[:3], r.returncode))
        ab = [ln for ln in r.stdout.splitlines() if ln.startswith("AB ")]
        return (json.loads(ab[-1][3:]) if ab else None), r.stderr

    res = {"rounds": args.rounds, "steady_calls_per_process": STEADY, "lines": {},
           "skipped": {"v1": "a forced v1 all2all on gamma collection A: a2a_tile_kernel<*>, a2a_direct_kernel<*> and a2a_global_kernel are "
                             "instruction-identical in the parent's build and in this tree's",
                       "db2db under KMDB_D2_NO_STORE=1": "d2_emit_kernel<false / true, false> (d2_list_bits) are instruction-identical since the first "
                                                         "pass is written out there again",
                       "upload": "width_estimate_kernel and pair_estimate_kernel are instruction-identical since the first pass is written out there again"},
           "measured": "*_ms: HIP events around the call's kernels (kmdb_stats.kernel_ms), mean of the steady calls of a process; first_call_ms, "
                       "upload_ms: wall clock of the call",
           "condition": "the median of this tree's runs is not above the parent's slowest run of the same rounds"}
    for line in args.lines.split(","):
        with tempfile.TemporaryDirectory(dir=args.tmp) as td:
            t0 = time.time()
            run(["--prepare", line, td], 900)
            log("%s: inputs written in %.1f s" % (line, time.time() - t0))
            warm = {who: run(["--child", line, lib, td], args.limit) for who, lib in libs.items()}
            assert warm["parent"][0]["sha"] == warm["this"][0]["sha"], line + ": the two libraries gave different outputs"
            entry = {"outputs_equal": True, "sha": warm["this"][0]["sha"]}
            if line == "upload":
                sizing = {who: [ln for ln in err.splitlines() if SIZING.search(ln) or ln.startswith("[kmdb] ----")] for who, (_, err) in warm.items()}
                assert sizing["parent"] == sizing["this"] and sizing["this"], "the upload's estimates differ:\n%s" % json.dumps(sizing, indent=1)
                entry["sizing"] = {"equal": True, "c2_width": warm["this"][0]["c2_width"], "A_width": warm["this"][0]["A_width"], "lines": sizing["this"]}
            runs = {who: [] for who in libs}
            for i in range(args.rounds):
                for who, lib in libs.items():
                    got = run(["--child", line, lib, td], args.limit)[0]
                    assert got["sha"] == entry["sha"], "%s round %d %s: other outputs" % (line, i, who)
                    runs[who].append(got)
                    log("%s round %d %s: %s" % (line, i, who, {f: got[f] for f in FIGURES[line]}))
            entry["runs"] = runs
            entry["figures"] = {}
            for f in FIGURES[line]:
                p, t = [r[f] for r in runs["parent"]], [r[f] for r in runs["this"]]
                entry["figures"][f] = {"parent": {"median": statistics.median(p), "min": min(p), "max": max(p)},
                                       "this": {"median": statistics.median(t), "min": min(t), "max": max(t)},
                                       "this_over_parent": round(statistics.median(t) / statistics.median(p), 4), "holds": statistics.median(t) <= max(p)}
            res["lines"][line] = entry
        with open(args.out, "w") as f:                                    # after every line: what was measured stays if a later line stops the script
            json.dump(res, f, indent=1)
            f.write("\n")
    print(json.dumps({line: e["figures"] for line, e in res["lines"].items()}))


if __name__ == "__main__":
    main()
