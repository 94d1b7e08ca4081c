"""A/B of the build mode: the device builder (csrc/build.hip) against the reference's own PrefixKmerDb::addKmers (oracle/_ref/ref_driver build)
on the same k-mer lists — the baseline, since a new mode has no parent commit.  README 'build' quotes the figures.

    python profiles/build_ab.py --out profiles/build_ab.json

A synthetic clade collection (synth.CladeGenomes: --samples genomes of --length bases in clades of --clade), k = 18, at fraction 1 and 0.1.
Per fraction:
  lists_in     wall clock of kmdb_build_begin + ONE kmdb_build_add_kmers with every sample + kmdb_build_finish: sorted unique lists in host
               memory in, a kmdbh_db in host memory out (after one warm-up build of the first 8 samples); the library's HIP-event split
               (kmdb_build_stats_get) and its counts
  text_in      the same with kmdb_build_add_seq_alphabet in calls of 64 samples: the genomes' text in, extraction on the device
  store_s      kmdbh_db_store of the result (host only)
  reference    `ref_driver build` at 1, 4 and 16 threads: the seconds it reports around its addKmers loop (reading the lists and serialize
               are outside, as store_s is outside ours); the best of the three is kept
The pattern and k-mer counts of the two must agree.  Nothing is judged against a threshold: the json states the figures."""
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
    ap.add_argument("--clade", type=int, default=16)
    ap.add_argument("--length", type=int, default=1_000_000)
    ap.add_argument("--k", type=int, default=18)
    ap.add_argument("--fractions", default="1,0.1")
    ap.add_argument("--ref-threads", default="1,4,16")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "build_ab.json"))
    args = ap.parse_args()
    import torch
    from _kmerdb_loader import import_kmerdb_amd
    from oracle import oracle as O
    K = import_kmerdb_amd()
    S = importlib.import_module("kmerdb_amd.synth")
    assert O.have_ref(), "oracle/_ref/ref_driver is missing: build it first (make -C oracle)"
    gen_dev = "cuda:%d" % args.device if torch.cuda.is_available() else "cpu"
    g = S.CladeGenomes(args.samples, args.clade, args.length, device=gen_dev)
    names = [g.name(i) for i in range(args.samples)]
    acgt = np.frombuffer(b"ACGT", np.uint8)
    texts = [acgt[g.sample(i).cpu().numpy()].tobytes() + b"\n" for i in range(args.samples)]
    res = {"workload": "%d synthetic genomes of %g Mbp in clades of %d (synth.CladeGenomes), k=%d" % (args.samples, args.length / 1e6, args.clade, args.k),
           "fractions": {}}

    def build_lists(lists, n=None):
        b = K.Builder(args.k, f, 0.0, "nt", device=args.device)
        t0 = time.perf_counter()
        b.add_kmers(names[:n], lists[:n])
        t1 = time.perf_counter()
        h = b.finish()
        t2 = time.perf_counter()
        st = b.stats()
        b.close()
        return h, st, t1 - t0, t2 - t1

    def build_text():
        b = K.Builder(args.k, f, 0.0, "nt", device=args.device)
        t0 = time.perf_counter()
        for s0 in range(0, args.samples, 64):
            b.add_seqs(names[s0: s0 + 64], texts[s0: s0 + 64])
        t1 = time.perf_counter()
        h = b.finish()
        t2 = time.perf_counter()
        st = b.stats()
        b.close()
        return h, st, t1 - t0, t2 - t1

    for f in [float(x) for x in args.fractions.split(",")]:
        lists = [S.kmers_of(g.sample(i), args.k, f).cpu().numpy().view(np.uint64).copy() for i in range(args.samples)]
        total = int(sum(x.size for x in lists))
        log("f = %g: %d k-mers in the lists" % (f, total))
        h, _, _, _ = build_lists(lists, 8)                      # warm-up: the device's first use, code objects, rocPRIM's first launches
        h.close()
        h, st, add_s, fin_s = build_lists(lists)
        r = {"kmers_in_lists": total, "distinct_kmers": int(st["distinct_kmers"]), "patterns": int(st["patterns"]), "events": int(st["events"]),
             "peak_device_bytes": int(st["peak_device_bytes"]),
             "lists_in": {"add_s": add_s, "finish_s": fin_s, "total_s": add_s + fin_s,
                          "stages_ms": {key: st[key] for key in st if key.endswith("_ms")}}}
        with tempfile.TemporaryDirectory() as td:
            t0 = time.perf_counter()
            h.store(os.path.join(td, "ours.db"))
            r["store_s"] = time.perf_counter() - t0
            r["db_bytes"] = os.path.getsize(os.path.join(td, "ours.db"))
            h.close()
            h2, st2, add2_s, fin2_s = build_text()
            h2.close()
            assert (st2["distinct_kmers"], st2["patterns"], st2["events"]) == (st["distinct_kmers"], st["patterns"], st["events"]), "text in and lists in differ"
            r["text_in"] = {"add_s": add2_s, "finish_s": fin2_s, "total_s": add2_s + fin2_s, "stages_ms": {key: st2[key] for key in st2 if key.endswith("_ms")}}
            O.write_kmers_bin(os.path.join(td, "k.bin"), args.k, f, list(zip(names, lists)))
            ref = {}
            for t in [int(x) for x in args.ref_threads.split(",")]:
                w0 = time.perf_counter()
                info = O.ref_build(os.path.join(td, "k.bin"), os.path.join(td, "r.db"), t)
                ref["%d" % t] = {"addkmers_s": info["seconds"], "process_s": time.perf_counter() - w0}
                assert (info["patterns"], info["kmers"]) == (st["patterns"], st["distinct_kmers"]), "the reference built another tree"
                log("  reference, %d threads: %s" % (t, json.dumps(ref["%d" % t])))
            best = min(ref, key=lambda t: ref[t]["addkmers_s"])
            r["reference"] = {"threads": ref, "best_threads": int(best), "best_addkmers_s": ref[best]["addkmers_s"]}
            r["reference_over_device_lists_in"] = ref[best]["addkmers_s"] / (add_s + fin_s)
            r["reference_over_device_text_in"] = ref[best]["addkmers_s"] / (add2_s + fin2_s)
        log("f = %g:" % f, json.dumps(r))
        res["fractions"]["%g" % f] = r
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
