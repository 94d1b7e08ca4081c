"""A/B of one long sample: the path the front-end took for a sample of 1800 MiB or more before the extractor cut such samples into sections
— kmdbh_extract_kmers_alphabet + kmdbh_sort_unique on ONE host thread — against kmdb_minhash_batch_seq_alphabet, which now extracts the sample
on the device in sections and joins their lists with the merge-union (csrc/sorted_union.hip).  README (Minhash) has the table.

    python profiles/long_sample_ab.py --out profiles/long_sample_ab.json

One synthetic nt sample of --length bases (default 2.2e9: uniform ACGT, seeded, one record), k = 18, window start 0, fractions 0.01 and 1, host
memory to host memory in both arms.  Per fraction: the two lists are compared first (the warm-up calls), then --rounds rounds with the arms
alternating.  Reported:
  device_s / host_s   wall clock of the arm, median and range over the rounds
  sections, pieces    of the device call (kmdb_minhash_long_stats_get, kmdb_minhash_stats_get)
  union               HIP-event ms around the unions (their table allocations and the read of the total included), words in and out, bytes by
                      construction (both inputs read twice — count pass, write pass — and the union written once), bytes / s, and that against
                      the device-to-device copy bandwidth bench.py --full measures (bench.measured_copy_gbs, run here on the same device)
  peak_device_bytes   the running list + a section's scratch, or + a section's list, the union and its tables, whichever was larger
Nothing is judged against a threshold: the json states the figures.  The host arm at fraction 1 sorts --length words on one thread and needs
8 bytes of host memory per base: --fractions 0.01 leaves it out."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def log(*a):
    print(*a, file=sys.stderr, flush=True)


def spread(x):
    return {"median": float(np.median(x)), "min": float(min(x)), "max": float(max(x))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--length", type=int, default=2_200_000_000)
    ap.add_argument("--k", type=int, default=18)
    ap.add_argument("--fractions", default="0.01,1")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--seed", type=int, default=20261020)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "long_sample_ab.json"))
    args = ap.parse_args()
    from _kmerdb_loader import import_kmerdb_amd
    K = import_kmerdb_amd()
    capi = K.capi
    L = K.lib()
    rng = np.random.default_rng(args.seed)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    text = np.empty(args.length, np.uint8)
    for at in range(0, args.length, 1 << 28):                      # in blocks: the random indices of the whole text would take as much memory again
        n = min(1 << 28, args.length - at)
        text[at: at + n] = acgt[rng.integers(0, 4, n, dtype=np.uint8)]
    log("text ready: %d bases" % text.size)
    keep, ptrs, lens, n = capi._sample_texts([text])
    opts = capi._opts(args.device)
    copy_gbs = None
    try:
        import torch  # noqa: F401
        import bench
        copy_gbs = float(bench.measured_copy_gbs("cuda:%d" % args.device))
    except Exception as e:                                          # the figures below stand without it
        log("copy bandwidth not measured:", repr(e))
    res = {"workload": "one synthetic nt sample of %g Gbp (uniform ACGT, one record), k=%d, window start 0, host memory to host memory" % (args.length / 1e9, args.k),
           "rounds": args.rounds, "measured_copy_GBs": copy_gbs,
           "not_measured": "real assemblies (runs of N, repeats, many records), protein alphabets, the builder's sink, the front-end's reading and "
                           "splitting of the FASTA file, more than one long sample in a batch, the host arm on more than one thread",
           "fractions": {}}

    def device_call(f):
        out = capi._KmerLists()
        t0 = time.perf_counter()
        rc = L.kmdb_minhash_batch_seq_alphabet(ptrs, lens, n, args.k, f, 0.0, 0, C.byref(out), C.byref(opts))
        dt = time.perf_counter() - t0
        capi._check(rc)
        return out, dt

    def host_call(f):
        words = np.empty(args.length + 1, np.uint64)
        t0 = time.perf_counter()
        cnt = L.kmdbh_extract_kmers_alphabet(C.c_void_p(text.ctypes.data), text.size, args.k, 0, f, 0.0, words.ctypes.data)
        cnt = L.kmdbh_sort_unique(words.ctypes.data, cnt)
        return words[:cnt], time.perf_counter() - t0

    L.kmdbh_extract_kmers_alphabet.argtypes = [C.c_void_p, C.c_size_t, C.c_uint32, C.c_int32, C.c_double, C.c_double, C.c_void_p]
    L.kmdbh_extract_kmers_alphabet.restype = C.c_size_t
    for f in [float(x) for x in args.fractions.split(",")]:
        out, dt = device_call(f)                                    # warm-up of the device arm; its list is the one compared
        log("f = %g: device warm-up %.2f s" % (f, dt))
        total = int(out.offsets[1])
        got = np.ctypeslib.as_array(out.kmers, shape=(max(total, 1),))[:total]
        want, dt = host_call(f)                                     # warm-up of the host arm
        log("f = %g: host warm-up %.2f s, %d words" % (f, dt, want.size))
        equal = bool(got.size == want.size and np.array_equal(got, want))
        L.kmdb_kmer_lists_free(C.byref(out))
        del want, got
        assert equal, "device and host lists differ at fraction %g" % f
        dev, host, stats, longs = [], [], [], []
        for _ in range(args.rounds):
            out, dt = device_call(f)
            L.kmdb_kmer_lists_free(C.byref(out))
            dev.append(dt)
            stats.append(K.minhash_stats())
            longs.append(K.minhash_long_stats())
            _, dt = host_call(f)
            host.append(dt)
            log("f = %g: round device %.2f s, host %.2f s" % (f, dev[-1], dt))
        med = lambda rows, key: float(np.median([r[key] for r in rows]))      # noqa: E731
        union_ms, union_bytes = med(longs, "union_ms"), med(longs, "union_bytes")
        union_gbs = union_bytes / (union_ms * 1e-3) / 1e9 if union_ms > 0 else None
        r = {"lists_equal": equal, "device_s": spread(dev), "host_s": spread(host), "host_over_device": float(np.median(host) / np.median(dev)),
             "sections": int(longs[0]["sections"]), "pieces": int(stats[0]["pieces"]), "kept": int(stats[0]["kept"]), "unique": int(stats[0]["unique"]),
             "union": {"ms": spread([x["union_ms"] for x in longs]), "words_in": int(longs[0]["union_words_in"]), "words_out": int(longs[0]["union_words_out"]),
                       "bytes": int(union_bytes), "GBs": union_gbs, "of_measured_copy": (union_gbs / copy_gbs) if union_gbs and copy_gbs else None},
             "peak_device_bytes": int(max(x["peak_bytes"] for x in longs)), "section_scratch_bytes": int(max(s["scratch_bytes"] for s in stats)),
             "stages_ms": {key: med(stats, key) for key in ("h2d_ms", "count_ms", "scan_ms", "write_ms", "sort_ms", "unique_ms")}}
        log("f = %g:" % f, json.dumps(r))
        res["fractions"]["%g" % f] = r
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
