"""A/B of the minhash mode's extractor: kmdb_minhash_batch_seq_alphabet (csrc/minhash.hip: rolling extraction, filter before store, sorts over the
kept words only) against the host path it replaces, kmdbh_extract_kmers_alphabet + kmdbh_sort_unique per sample on a pool of threads — the baseline,
since a new entry point has no parent commit.  DESIGN section 4 has the table.

    python profiles/minhash_ab.py --out profiles/minhash_ab.json

64 synthetic 5 Mbp nt genomes (uniform ACGT, seeded), k = 18, fraction 0.01 (the mode's default), 0.1 and 1, window start 0.  Per fraction:
  device       wall clock of the C call alone, host memory to host memory: the text goes up, the lists come back (median, min, max of --runs calls
               after one warm-up call)
  stages       the same calls split by the library's HIP events (kmdb_minhash_stats_get): text to the device, pass 1 (extraction + tile counts),
               scan, pass 2 (extraction + write), the two radix sorts, heads + scan + compaction + lists to the host; kept and unique words, and
               the device bytes per base
  host         wall clock of extraction + sort-unique of all samples on --threads threads (ctypes releases the GIL around both calls)
The two results must be equal word for word.  Nothing is judged against a threshold: the json states the figures."""
import argparse
import ctypes as C
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def log(*a):
    print(*a, file=sys.stderr, flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=64)
    ap.add_argument("--length", type=int, default=5_000_000)
    ap.add_argument("--k", type=int, default=18)
    ap.add_argument("--fractions", default="0.01,0.1,1")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--host-runs", type=int, default=2)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--seed", type=int, default=20261018)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "minhash_ab.json"))
    args = ap.parse_args()
    from _kmerdb_loader import import_kmerdb_amd
    K = import_kmerdb_amd()
    capi = K.capi
    L = K.lib()
    rng = np.random.default_rng(args.seed)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    texts = [acgt[rng.integers(0, 4, args.length, dtype=np.uint8)].tobytes() for _ in range(args.samples)]
    keep, ptrs, lens, n = capi._text_queries(texts)
    opts = capi._opts(args.device)
    R, T = K.minhash_geometry()
    res = {"workload": "%d synthetic %g Mbp nt genomes (uniform ACGT), k=%d, window start 0" % (args.samples, args.length / 1e6, args.k),
           "positions_per_thread": R, "positions_per_tile": T, "runs": args.runs, "host_threads": args.threads, "fractions": {}}

    def device_call(f):
        out = capi._KmerLists()
        t0 = time.perf_counter()
        rc = L.kmdb_minhash_batch_seq_alphabet(ptrs, lens, n, args.k, f, 0.0, 0, C.byref(out), C.byref(opts))
        dt = time.perf_counter() - t0
        capi._check(rc)
        return out, dt

    def host_sample(t, f):
        return K.sort_unique(K.extract_kmers_alphabet(t, args.k, 0, f, 0.0))

    for f in [float(x) for x in args.fractions.split(",")]:
        out, _ = device_call(f)                                 # warm-up: the device's first use, code objects, rocPRIM's first launches
        off = np.ctypeslib.as_array(out.offsets, shape=(n + 1,)).copy()
        flat = np.ctypeslib.as_array(out.kmers, shape=(int(off[n]),)).copy() if off[n] else np.zeros(0, np.uint64)
        L.kmdb_kmer_lists_free(C.byref(out))
        wall, stages = [], []
        for _ in range(args.runs):
            out, dt = device_call(f)
            L.kmdb_kmer_lists_free(C.byref(out))
            wall.append(dt)
            stages.append(K.minhash_stats())
        host = []
        with ThreadPoolExecutor(args.threads) as pool:
            for _ in range(args.host_runs):
                t0 = time.perf_counter()
                want = list(pool.map(lambda t: host_sample(t, f), texts))
                host.append(time.perf_counter() - t0)
        assert all(np.array_equal(flat[int(off[s]): int(off[s + 1])], want[s]) for s in range(n)), "device and host lists differ"
        st = {key: float(np.median([s[key] for s in stages])) for key in stages[0]}
        bases = st["bases"]
        r = {"device_s": {"median": float(np.median(wall)), "min": min(wall), "max": max(wall)},
             "host_s": {"median": float(np.median(host)), "min": min(host), "max": max(host)},
             "host_over_device": float(np.median(host)) / float(np.median(wall)),
             "stages_ms": {key: st[key] for key in ("h2d_ms", "count_ms", "scan_ms", "write_ms", "sort_ms", "unique_ms")},
             "bases": int(bases), "kept": int(st["kept"]), "unique": int(st["unique"]), "pieces": int(st["pieces"]),
             "device_bytes_per_base": st["scratch_bytes"] / bases, "lists_equal": True}
        log("f = %g:" % f, json.dumps(r))
        res["fractions"]["%g" % f] = r
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
