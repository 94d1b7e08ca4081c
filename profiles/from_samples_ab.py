"""A/B of `all2all -from-samples`: genomes in, table out, as processes and by their wall clock.  README 'Hand-off' quotes the figures.

    python profiles/from_samples_ab.py --parent-exe <kmer-db-amd of the parent commit> --out profiles/from_samples_ab.json

  arm (a)   `build -k K <list> T.db` followed by `all2all T.db out.csv` with the PARENT commit's front-end (--parent-exe; without it this
            commit's, and the json says so: build and all2all of the two commits differ only in where the layout's device stage is called from)
  arm (b)   this commit's `all2all -from-samples -k K <list> out.csv`
The outputs are compared equal first.  One warm-up per arm, then --rounds rounds with the arms alternating (a b, b a, ...), every process
timed from its start to its end.  Two collections from synth.CladeGenomes, written as FASTA files: --big (256 x 1 Mbp, build_ab's) and
--many (1000 x 300 kbp).  Next to the wall clocks: what KMDB_VERBOSE reports of the last round — the hand-off's stage times and peak bytes
for (b); the builder's finish stages, the store (build's wall clock minus its sample loop), the load and the upload for (a).
Nothing is judged against a threshold: the json states every run."""
import argparse
import importlib
import json
import os
import re
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
EXE = os.path.join(ROOT, "kmer-db_amd", "bin", "kmer-db-amd")


def log(*a):
    print(*a, file=sys.stderr, flush=True)


def run(exe, *args):
    """(wall clock of the process, its stderr)"""
    env = dict(os.environ, KMDB_VERBOSE="1")
    t0 = time.perf_counter()
    r = subprocess.run([exe] + list(args), capture_output=True, text=True, env=env)
    dt = time.perf_counter() - t0
    if r.returncode != 0:
        raise SystemExit("%s %s failed:\n%s" % (exe, " ".join(args), r.stderr[-2000:]))
    return dt, r.stderr


def reported(stderr):
    """the figures the front-end prints about the hand-over, whichever way it went"""
    out = {}
    m = re.search(r"\[kmdb\] hand-off: .* peak (\d+) device bytes \(handle (\d+)\), (\d+) bytes to the host; encode (\S+) tables (\S+) fields (\S+) layout (\S+) "
                  r"prepare (\S+) copy-back (\S+) total (\S+) ms", stderr)
    if m:
        keys = ("peak_device_bytes", "handle_device_bytes", "d2h_bytes", "encode_ms", "tables_ms", "fields_ms", "layout_ms", "prepare_ms", "copy_back_ms", "total_ms")
        out["handoff"] = {k: float(v) if k.endswith("_ms") else int(v) for k, v in zip(keys, m.groups())}
    m = re.search(r"\[kmdb\] build: .* peak (\d+) device bytes; .* encode (\S+) tables (\S+) copy-back (\S+) ms", stderr)
    if m:
        out["finish"] = {"peak_device_bytes": int(m.group(1)), "encode_ms": float(m.group(2)), "tables_ms": float(m.group(3)), "copy_back_ms": float(m.group(4))}
    m = re.search(r"Database loaded in (\S+) s, uploaded in (\S+) s", stderr)
    if m:
        out["load_s"], out["upload_s"] = float(m.group(1)), float(m.group(2))
    m = re.search(r"EXECUTION TIMES\nTotal: (\S+)", stderr)
    if m:
        out["sample_loop_s"] = float(m.group(1))
    m = re.search(r"Database handed to the engine in (\S+) s", stderr)
    if m:
        out["handed_over_s"] = float(m.group(1))
    return out


def spread(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "runs": xs}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--big", default="256,16,1000000", help="samples,clade,length of the first collection")
    ap.add_argument("--many", default="1000,20,300000", help="... of the second")
    ap.add_argument("--k", type=int, default=18)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--parent-exe", default=None)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "from_samples_ab.json"))
    args = ap.parse_args()
    import torch
    from _kmerdb_loader import import_kmerdb_amd
    import_kmerdb_amd()
    S = importlib.import_module("kmerdb_amd.synth")
    exe_a = args.parent_exe or EXE
    res = {"arm_a_exe": "the parent commit's" if args.parent_exe else "THIS commit's (no --parent-exe given)", "k": args.k, "rounds": args.rounds, "collections": {}}
    acgt = np.frombuffer(b"ACGT", np.uint8)
    gen_dev = "cuda:%d" % args.device if torch.cuda.is_available() else "cpu"
    for tag, spec in (("big", args.big), ("many", args.many)):
        n, clade, length = [int(x) for x in spec.split(",")]
        with tempfile.TemporaryDirectory() as td:
            g = S.CladeGenomes(n, clade, length, device=gen_dev)
            lst = os.path.join(td, "samples.list")
            with open(lst, "w") as fl:
                for i in range(n):
                    base = os.path.join(td, g.name(i))
                    with open(base + ".fasta", "wb") as fa:
                        fa.write(b">" + g.name(i).encode() + b"\n" + acgt[g.sample(i).cpu().numpy()].tobytes() + b"\n")
                    fl.write(base + "\n")
            del g
            k, gpu = str(args.k), str(args.device)
            db, out_a, out_b = os.path.join(td, "T.db"), os.path.join(td, "a.csv"), os.path.join(td, "b.csv")

            def arm_a():
                t1, e1 = run(exe_a, "build", "-gpu", gpu, "-k", k, lst, db)
                t2, e2 = run(exe_a, "all2all", "-gpu", gpu, db, out_a)
                return t1 + t2, {"build_s": t1, "all2all_s": t2, "build": reported(e1), "all2all": reported(e2)}

            def arm_b():
                t, e = run(EXE, "all2all", "-from-samples", "-gpu", gpu, "-k", k, lst, out_b)
                return t, reported(e)

            arm_a()                                                 # warm-ups: code objects, the page cache of the genomes
            arm_b()
            with open(out_a, "rb") as fa, open(out_b, "rb") as fb:
                assert fa.read() == fb.read(), "the two arms wrote different tables"
            a_s, b_s, a_last, b_last = [], [], None, None
            for r in range(args.rounds):
                for arm in ("ab" if r % 2 == 0 else "ba"):
                    if arm == "a":
                        t, a_last = arm_a()
                        a_s.append(t)
                    else:
                        t, b_last = arm_b()
                        b_s.append(t)
                log("%s round %d: a %.3f s, b %.3f s" % (tag, r, a_s[-1], b_s[-1]))
            a_last["store_s"] = a_last["build_s"] - a_last["build"].get("sample_loop_s", 0.0)      # finish + store + the process around them
            res["collections"][tag] = {"workload": "%d synthetic genomes of %g Mbp in clades of %d (synth.CladeGenomes)" % (n, length / 1e6, clade),
                                       "db_bytes": os.path.getsize(db), "a_build_then_all2all_s": spread(a_s), "b_from_samples_s": spread(b_s),
                                       "every_b_below_every_a": max(b_s) < min(a_s), "a_last_round": a_last, "b_last_round": b_last}
            log(tag, json.dumps(res["collections"][tag]))
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
