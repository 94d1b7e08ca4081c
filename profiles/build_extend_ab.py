"""A/B of extending a stored database: the seeded builder (kmdb_build_begin_from_db, csrc/build.hip) against the only alternative the parent
commit has, a full rebuild of the whole collection with the unchanged add path.  README 'build -extend-from' and DESIGN §4 quote the figures.

    python profiles/build_extend_ab.py --out profiles/build_extend_ab.json

A synthetic clade collection (synth.CladeGenomes: --samples genomes of --length bases in clades of --clade), k = 18, fraction 1.  The first
--seed-samples genomes are built and stored; then
  extend    kmdbh_db_load of that file (host only, reported on its own), kmdb_build_begin_from_db, ONE kmdb_build_add_kmers with the remaining
            samples, kmdb_build_finish: wall clock of each, the seed's HIP-event split (kmdb_build_seed_stats_get), the add stages
            (kmdb_build_stats_get) and the builder's peak device bytes
  rebuild   kmdb_build_begin + ONE kmdb_build_add_kmers with every sample + kmdb_build_finish, sorted unique lists in host memory in
Both run once after a warm-up (a build of 8 samples, stored, loaded, seeded and extended by one sample).  The two stored files must be equal
byte for byte.  What the rebuild needs and the extension does not — reading and extracting the old genomes again — is outside both figures.
Nothing is judged against a threshold: the json states the figures."""
import argparse
import importlib
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def log(*a):
    print(*a, file=sys.stderr, flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=256)
    ap.add_argument("--seed-samples", type=int, default=240)
    ap.add_argument("--clade", type=int, default=16)
    ap.add_argument("--length", type=int, default=1_000_000)
    ap.add_argument("--k", type=int, default=18)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "build_extend_ab.json"))
    args = ap.parse_args()
    import torch
    from _kmerdb_loader import import_kmerdb_amd
    K = import_kmerdb_amd()
    S = importlib.import_module("kmerdb_amd.synth")
    gen_dev = "cuda:%d" % args.device if torch.cuda.is_available() else "cpu"
    g = S.CladeGenomes(args.samples, args.clade, args.length, device=gen_dev)
    names = [g.name(i) for i in range(args.samples)]
    lists = [S.kmers_of(g.sample(i), args.k, 1.0).cpu().numpy().view(np.uint64).copy() for i in range(args.samples)]
    n0 = args.seed_samples
    res = {"workload": "%d synthetic genomes of %g Mbp in clades of %d (synth.CladeGenomes), k=%d, fraction 1: the first %d stored, the last %d added"
                       % (args.samples, args.length / 1e6, args.clade, args.k, n0, args.samples - n0),
           "kmers_in_lists": int(sum(x.size for x in lists)), "kmers_in_added_lists": int(sum(x.size for x in lists[n0:]))}

    def rebuild(n):
        t0 = time.perf_counter()
        b = K.Builder(args.k, 1.0, 0.0, "nt", device=args.device)
        t1 = time.perf_counter()
        b.add_kmers(names[:n], lists[:n])
        t2 = time.perf_counter()
        h = b.finish()
        t3 = time.perf_counter()
        st = b.stats()
        b.close()
        return h, st, {"begin_s": t1 - t0, "add_s": t2 - t1, "finish_s": t3 - t2, "total_s": t3 - t0}

    def extend(path, lo, hi):
        t0 = time.perf_counter()
        old = K.HostDB(path)
        t1 = time.perf_counter()
        b = K.Builder.from_db(old, device=args.device)
        t2 = time.perf_counter()
        old.close()
        b.add_kmers(names[lo:hi], lists[lo:hi])
        t3 = time.perf_counter()
        h = b.finish()
        t4 = time.perf_counter()
        st, seed = b.stats(), b.seed_stats()
        b.close()
        return h, st, seed, {"load_s": t1 - t0, "seed_s": t2 - t1, "add_s": t3 - t2, "finish_s": t4 - t3, "total_s": t4 - t1}

    with tempfile.TemporaryDirectory() as td:
        p = lambda n: os.path.join(td, n)                       # noqa: E731
        h, _, _ = rebuild(8)                                    # warm-up: the device's first use, code objects, rocPRIM's first launches
        h.store(p("warm.db"))
        h.close()
        h, _, _, _ = extend(p("warm.db"), 8, 9)
        h.close()
        h, st_head, _ = rebuild(n0)
        h.store(p("head.db"))
        h.close()
        res["stored_db_bytes"] = os.path.getsize(p("head.db"))
        h, st, seed, t = extend(p("head.db"), n0, args.samples)
        h.store(p("ext.db"))
        h.close()
        res["extend"] = dict(t, seed_stages_ms={key: seed[key] for key in seed if key.endswith("_ms")}, seed_h2d_bytes=int(seed["h2d_bytes"]),
                             seed_slots=int(seed["slots"]), add_finish_stages_ms={key: st[key] for key in st if key.endswith("_ms")},
                             peak_device_bytes=int(st["peak_device_bytes"]))
        log("extend:", json.dumps(res["extend"]))
        h, st_full, t = rebuild(args.samples)
        h.store(p("full.db"))
        h.close()
        res["rebuild"] = dict(t, stages_ms={key: st_full[key] for key in st_full if key.endswith("_ms")}, peak_device_bytes=int(st_full["peak_device_bytes"]))
        log("rebuild:", json.dumps(res["rebuild"]))
        for key in ("samples", "distinct_kmers", "patterns", "events"):
            assert st[key] == st_full[key], key
            res[key] = int(st[key])
        with open(p("ext.db"), "rb") as a, open(p("full.db"), "rb") as b:
            assert a.read() == b.read(), "the extended file is not the rebuilt file"
        res["files_equal"] = True
        res["rebuild_over_extend"] = res["rebuild"]["total_s"] / res["extend"]["total_s"]
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
