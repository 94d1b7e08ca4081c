"""new2all on query shards against the unsharded handle, on ONE device and in ONE process (DESIGN section 6 has the table).

    python profiles/node_new2all_ab.py --workload c5part --shards 8 --rounds 5 [--parent-lib <libkmdb_amd.so of the parent commit>]

The workload is bench.py's shape (bench.WORKLOADS: samples, clade size, genome length, queries — fresh strains of 20 clades, as bench.py's
new2all row makes them).  Every call runs on one torch stream handed to the engine as kmdb_opts.stream; times are HIP-event times around
calls that end in a synchronise, no profiler attached, every shape warmed up first.  The whole call's interval splits into `probe + walk`
(kmdb_stats.kernel_ms: probe, hit sort, count, walk) and the rest (`extract + sorts`: the text's H2D copy, extraction, the own-position
compaction on a shard, two radix sorts, unique compaction, and the call's allocations).

Exact conditions are asserted: the rows of the shards sum to the unsharded rows, the shards' slots sum to the table's, their unique k-mer
counts to the queries', their hits (computed on the host from the database's dictionary) to the unsharded hit count.  The one timing
condition — the unsharded kmdb_new2all_batch_seq is not slower than the parent commit's — is measured against the parent's library on the
same inputs, alternating, and judged by the spread the parent shows against itself; both spreads and the difference are written out.
The sharded sum on one device extracts the same text `shards` times by construction: it is not a scaling figure."""
import argparse
import ctypes as C
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402

log = bench.log


def spread(xs):
    xs = [float(x) for x in xs]
    return {"median": float(np.median(xs)), "min": min(xs), "max": max(xs), "rounds": xs}


class RawLib:
    """kmdb_db_upload / kmdb_new2all_batch_seq / kmdb_db_stats of ANY build of the library (the parent commit's has no newer symbol)"""

    def __init__(self, K, path):
        self.K, cap = K, K.capi
        self.L = L = C.CDLL(path)
        L.kmdb_last_error.restype = C.c_char_p
        L.kmdb_db_upload.argtypes = [C.POINTER(cap._View), C.POINTER(cap._Opts), C.c_int, C.POINTER(C.c_void_p)]
        L.kmdb_db_free.argtypes = [C.c_void_p]
        L.kmdb_db_stats.argtypes = [C.c_void_p, C.POINTER(cap._Stats)]
        L.kmdb_new2all_batch_seq.argtypes = [C.c_void_p, C.POINTER(C.c_char_p), C.POINTER(C.c_size_t), C.c_size_t, C.c_double, C.c_double, C.c_int,
                                             C.c_void_p, C.c_void_p, C.POINTER(cap._Opts)]

    def check(self, rc):
        if rc:
            raise RuntimeError(self.L.kmdb_last_error().decode(errors="replace"))

    def upload(self, view, dev):
        h = C.c_void_p()
        o = self.K.capi._opts(dev)
        self.check(self.L.kmdb_db_upload(C.pointer(view[0]), C.byref(o), 1, C.byref(h)))
        return h

    def seq(self, h, dev, texts, out, cnt, stream):
        nq = len(texts)
        ptrs = (C.c_char_p * nq)(*texts)
        lens = (C.c_size_t * nq)(*[len(t) for t in texts])
        o = self.K.capi._opts(dev, stream=stream)
        self.check(self.L.kmdb_new2all_batch_seq(h, ptrs, lens, nq, 1.0, 0.0, 0, out.ctypes.data, cnt.ctypes.data, C.byref(o)))

    def kernel_ms(self, h):
        s = self.K.capi._Stats()
        self.check(self.L.kmdb_db_stats(h, C.byref(s)))
        return float(s.kernel_ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="c5part")
    ap.add_argument("--samples", type=int, default=0, help="override the workload's shape (recorded in the output)")
    ap.add_argument("--length", type=int, default=0)
    ap.add_argument("--queries", type=int, default=0)
    ap.add_argument("--shards", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--parent-lib", default="", help="libkmdb_amd.so built from the parent commit (the A/B of the unsharded sequence entry)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "node_new2all_ab.json"))
    args = ap.parse_args()
    import torch
    K = bench.import_kmerdb_amd()
    S = importlib.import_module("kmerdb_amd.synth")
    if K.device_count() == 0:
        raise SystemExit("node_new2all_ab.py needs an MI355X")
    dev = args.device
    torch.cuda.set_device(dev)
    device = torch.device("cuda", dev)
    wl = dict(bench.WORKLOADS[args.workload])
    N, cs, k = args.samples or wl["samples"], wl["clade_size"], wl.get("k", 18)
    Lg, NQ, R = args.length or wl["length"], args.queries or wl["queries"], args.shards
    seed = 20260928
    t0 = time.time()
    g = S.CladeGenomes(N, cs, Lg, seed=seed, device=device)
    pat = S.build_patterns(lambda i: S.kmers_of(g.sample(i), k, 1.0), N, device, progress=None)
    arr = S.to_view_arrays(pat)
    tables = S.build_hashtables(pat["dictionary"], pat["kmer_pid"], k)
    log("synth db + hashtables: %d k-mers, %d patterns in %.1f s" % (pat["dictionary"].numel(), arr["num_kmers"].size, time.time() - t0))
    view = K.make_view(k, N, arr["num_kmers"], arr["parent_id"], arr["num_samples"], arr["num_local"], arr["last_sample_id"], arr["num_bits"],
                       arr["data_offset"], arr["data"], bucket_offset=tables[0], slots=tables[1])
    n_clades = max(1, N // cs)
    chosen = [int(c) for c in np.random.default_rng(seed + 1000).choice(n_clades, size=min(20, n_clades), replace=False)]
    codes = [g.strain(chosen[i * len(chosen) // NQ], N + i) for i in range(NQ)]
    lut = np.frombuffer(b"ACGT", dtype=np.uint8)
    texts = [lut[c.cpu().numpy().astype(np.int64)].tobytes() for c in codes]
    # hits per shard, on the host side of things: the queries' k-mers that the database's dictionary holds, by bucket
    dictionary = pat["dictionary"]
    hits = np.zeros(R, np.int64)
    uniq_own = np.zeros((R, NQ), np.int64)
    for i, c in enumerate(codes):
        q = S.kmers_of(c, k, 1.0)
        pos = torch.searchsorted(dictionary, q).clamp_(max=dictionary.numel() - 1)
        found = dictionary[pos] == q
        sh = (q >> 32) % R
        hits += torch.bincount(sh[found], minlength=R).cpu().numpy()
        uniq_own[:, i] = torch.bincount(sh, minlength=R).cpu().numpy()
    del pat, g, codes
    bench.release_generator_memory(0)
    torch.cuda.empty_cache()

    stream = torch.cuda.Stream(device=device)
    sp = stream.cuda_stream

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        fn()
        e1.record(stream)
        e1.synchronize()
        return float(e0.elapsed_time(e1))

    out = {"what": "new2all sequence entry: unsharded handle vs %d query shards on one device, one process" % R, "device": torch.cuda.get_device_name(dev),
           "workload": args.workload, "samples": N, "genome_length_bp": Lg, "queries": NQ, "k": k, "shards": R, "rounds": args.rounds,
           "patterns": int(arr["num_kmers"].size), "slots": int(tables[1].size), "buckets": int(tables[0].size - 1)}

    # ---- unsharded: this build (and the parent's, alternating)
    new = RawLib(K, K.capi.lib_path())
    libs = {"this": new}
    if args.parent_lib:
        libs["parent"] = RawLib(K, args.parent_lib)
    handles = {name: lib.upload(view, dev) for name, lib in libs.items()}
    rows = {name: np.zeros((NQ, N), np.uint32) for name in libs}
    cnt = {name: np.zeros(NQ, np.uint64) for name in libs}
    call = {name: (lambda name=name: libs[name].seq(handles[name], dev, texts, rows[name], cnt[name], sp)) for name in libs}
    for name in libs:                                           # warm up: run index, allocator
        call[name]()
        call[name]()
    order = ["parent", "this", "parent"] if args.parent_lib else ["this"]      # the parent twice per round: its spread against itself
    ms = {"this": [], "parent_a": [], "parent_b": []}
    kms = {"this": [], "parent_a": [], "parent_b": []}
    for _ in range(args.rounds):
        for j, name in enumerate(order):
            key = name if name == "this" else ("parent_a" if j == 0 else "parent_b")
            ms[key].append(timed(call[name]))
            kms[key].append(libs[name].kernel_ms(handles[name]))
    exp, exp_cnt = rows["this"].copy(), cnt["this"].copy()
    un = {"call_ms": spread(ms["this"]), "probe_walk_ms": spread(kms["this"])}
    un["extract_sorts_ms"] = un["call_ms"]["median"] - un["probe_walk_ms"]["median"]
    if args.parent_lib:
        assert np.array_equal(rows["parent"], exp) and np.array_equal(cnt["parent"], exp_cnt)
        pa, pb = np.array(ms["parent_a"]), np.array(ms["parent_b"])
        parent_self = float(np.max(np.abs(pa - pb)))            # the parent against itself, same rounds, same number of repeats
        parent_med = float(np.median(np.concatenate([pa, pb])))
        diff = un["call_ms"]["median"] - parent_med
        out["refactor_ab"] = {"parent_call_ms_a": spread(pa), "parent_call_ms_b": spread(pb), "this_call_ms": un["call_ms"],
                              "parent_spread_against_itself_ms": parent_self, "this_spread_ms": un["call_ms"]["max"] - un["call_ms"]["min"],
                              "this_minus_parent_median_ms": diff, "parent_probe_walk_ms": spread(kms["parent_a"] + kms["parent_b"]),
                              "rows_equal": True, "not_slower_within_parent_spread": bool(diff <= parent_self)}
        log("unsharded seq call: this %.2f ms, parent %.2f ms (difference %.2f ms, the parent against itself %.2f ms)" % (
            un["call_ms"]["median"], parent_med, diff, parent_self))
        libs["parent"].L.kmdb_db_free(handles.pop("parent"))
    st = K.capi._Stats()
    new.check(new.L.kmdb_db_stats(handles["this"], C.byref(st)))
    un.update(resident_bytes=int(st.device_bytes), nodes=int(st.n_patterns), h2d_bytes=int(st.h2d_bytes), slots=int(tables[1].size),
              unique_kmers=int(exp_cnt.sum()), hits=int(hits.sum()))
    new.L.kmdb_db_free(handles.pop("this"))
    out["unsharded"] = un

    # ---- query shards, all resident on the one device, adding into one buffer
    kept, kmers, slots, buckets = [np.zeros(R, np.uint64) for _ in range(4)]
    K.capi._check(K.capi.lib().kmdbh_query_shard_plan_counts(C.pointer(view[0]), R, kept.ctypes.data, kmers.ctypes.data, slots.ctypes.data, buckets.ctypes.data))
    assert int(slots.sum()) == int(tables[1].size)
    shards = [K.DeviceDB(view, device=dev, query_shard=(s, R)) for s in range(R)]
    buf = torch.zeros((NQ, N), dtype=torch.int32, device=device)
    per = [{"shard": s, "call_ms": [], "probe_walk_ms": []} for s in range(R)]
    total_cnt = np.zeros(NQ, np.uint64)
    for rnd in range(args.rounds + 1):                          # round 0 warms every shard up
        buf.zero_()
        torch.cuda.synchronize()
        for s, d in enumerate(shards):
            c = [None]
            t = timed(lambda: c.__setitem__(0, d.new2all_seq_device(texts, buf.data_ptr(), stream=sp)))
            if rnd:
                per[s]["call_ms"].append(t)
                per[s]["probe_walk_ms"].append(d.stats()["kernel_ms"])
            else:
                assert np.array_equal(c[0].astype(np.int64), uniq_own[s]), s
                total_cnt += c[0]
        got = buf.cpu().numpy().view(np.uint32)
        assert np.array_equal(got, exp), "the rows of the shards do not sum to the unsharded rows"
    assert np.array_equal(total_cnt, exp_cnt)
    sum_call = [sum(p["call_ms"][r] for p in per) for r in range(args.rounds)]
    sum_pw = [sum(p["probe_walk_ms"][r] for p in per) for r in range(args.rounds)]
    for s, d in enumerate(shards):
        stt = d.stats()
        per[s].update(call_ms=spread(per[s]["call_ms"]), probe_walk_ms=spread(per[s]["probe_walk_ms"]), resident_bytes=int(stt["device_bytes"]),
                      nodes=int(stt["n_patterns"]), h2d_bytes=int(stt["h2d_bytes"]), slots=int(slots[s]), buckets=int(buckets[s]), own_kmers=int(kmers[s]),
                      unique_query_kmers=int(uniq_own[s].sum()), hits=int(hits[s]))
        assert int(stt["n_patterns"]) == int(kept[s])
        d.close()
    sh = {"sum_call_ms": spread(sum_call), "sum_probe_walk_ms": spread(sum_pw), "per_shard": per,
          "sum_resident_bytes": sum(p["resident_bytes"] for p in per), "max_resident_bytes": max(p["resident_bytes"] for p in per),
          "sum_nodes": sum(p["nodes"] for p in per), "sum_slots": sum(p["slots"] for p in per), "sum_h2d_bytes": sum(p["h2d_bytes"] for p in per),
          "sum_hits": sum(p["hits"] for p in per), "sum_unique_kmers": int(total_cnt.sum())}
    sh["sum_extract_sorts_ms"] = sh["sum_call_ms"]["median"] - sh["sum_probe_walk_ms"]["median"]
    assert sh["sum_slots"] == un["slots"] and sh["sum_hits"] == un["hits"] and sh["sum_unique_kmers"] == un["unique_kmers"]
    out["query_shards"] = sh
    out["rows_equal"] = True
    out["sharded_sum_over_unsharded"] = sh["sum_call_ms"]["median"] / un["call_ms"]["median"]
    out["largest_shard_over_whole_resident_bytes"] = sh["max_resident_bytes"] / un["resident_bytes"]
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    if args.parent_lib and not out["refactor_ab"]["not_slower_within_parent_spread"]:
        raise SystemExit("the unsharded kmdb_new2all_batch_seq is slower than the parent's by %.3f ms, more than the parent's spread against itself (%.3f ms)" % (
            out["refactor_ab"]["this_minus_parent_median_ms"], out["refactor_ab"]["parent_spread_against_itself_ms"]))
    log("unsharded %.2f ms (probe + walk %.2f); %d shards in turn %.2f ms (probe + walk %.2f); largest shard holds %.1f %% of the whole handle's bytes" % (
        un["call_ms"]["median"], un["probe_walk_ms"]["median"], R, sh["sum_call_ms"]["median"], sh["sum_probe_walk_ms"]["median"],
        100 * out["largest_shard_over_whole_resident_bytes"]))


if __name__ == "__main__":
    main()
