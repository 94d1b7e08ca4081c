"""A/B of the two partitions of a database over the GPUs of a node, on ONE device and in ONE process: the unsharded handle, the node driver
with 8 prefix-bucket shards and the node driver with 8 tree ranges run the same all2all in alternation (DESIGN section 6 has the table).

    python profiles/partition_ab.py --workloads c3gpu,c3part --rounds 5 --out profiles/partition_ab.json

The workloads are bench.py's (bench.WORKLOADS / bench.generate_in_child: the generator runs in a process of its own).  Times are HIP-event
times from kmdb_stats / kmdb_node_stats.  Exact conditions are asserted (the three matrices are equal; the ranges hold P + sum(depth - 1)
nodes); everything else is reported, not judged."""
import argparse
import ctypes
import json
import lzma
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402

log = bench.log


def spread(xs):
    xs = [float(x) for x in xs]
    return {"median": float(np.median(xs)), "min": min(xs), "max": max(xs)}


def per_shard(K, torch, view, dev, kind, R, buf, reps=3):
    """every shard of a partition as a handle of its own: nodes, records and the call's HIP-event time (median of `reps` warm calls)"""
    rows = []
    for s in range(R):
        d = K.DeviceDB(view, device=dev, **{kind: (s, R)})
        d.all2all_dense_device(buf.data_ptr())
        torch.cuda.synchronize()
        ms = []
        for _ in range(reps):
            d.all2all_dense_device(buf.data_ptr())
            torch.cuda.synchronize()
            ms.append(d.stats()["kernel_ms"])
        st = d.stats()
        rows.append({"shard": s, "call_ms": float(np.median(ms)), "nodes": int(st["n_patterns"]), "records": int(st["n_records"] + st["n_direct"]),
                     "h2d_bytes": int(st["h2d_bytes"]), "sum_pairs": int(st["sum_pairs"])})
        d.close()
    return rows


def run_workload(K, torch, name, R, rounds, dev, together=True):
    wl = bench.WORKLOADS[name]
    k = wl.get("k", 18)
    arr, names, counts, nk, items = bench.generate_in_child(dev, n_samples=wl["samples"], clade_size=wl["clade_size"], length=wl["length"], k=k,
                                                            seed=20260928 + 1, rank=0, world=1, progress=100, with_items=True,
                                                            fraction=wl.get("fraction", 1.0))
    bench.release_generator_memory(0)
    N, P = wl["samples"], int(arr["num_kmers"].size)
    fields = [arr[f] for f in ("num_kmers", "parent_id", "num_samples", "num_local", "last_sample_id", "num_bits", "data_offset", "data")]
    view_ht = K.make_view(k, N, *fields, bucket_offset=items[0], slots=items[1])
    view = K.make_view(k, N, *fields)                          # what a load with SkipHashtables gives
    plan = K.range_plan(ctypes.pointer(view[0]), R)
    ne = plan["own"] > 0
    formula = P + int((plan["first_depth"][ne].astype(np.int64) - 1).sum())
    assert int(plan["kept"].sum()) == formula
    out = {"workload": name, "samples": N, "patterns": P, "shards": R, "rounds": rounds, "distinct_kmers": int(nk),
           "range_plan": {"kept": [int(x) for x in plan["kept"]], "own": [int(x) for x in plan["own"]], "first_depth": [int(x) for x in plan["first_depth"]],
                          "est_cost": [int(x) for x in plan["cost"]], "sum_kept": formula}}
    views = {"unsharded": view, "prefix": view_ht, "range": view}
    handles, res, ms = {}, {p: {} for p in views}, {p: [] for p in views}
    buf = torch.empty(max(1, N * (N - 1) // 2), dtype=torch.int32, device="cuda:%d" % dev)
    ref = {}

    def open_handle(part):
        t0 = time.perf_counter()
        hd = K.DeviceDB(views[part], device=dev) if part == "unsharded" else K.NodeDB(views[part], R, [dev], partition=part)
        res[part].setdefault("upload_s", time.perf_counter() - t0)
        res[part].setdefault("plan_s", 0.0 if part == "unsharded" else hd.stats()["plan_s"])
        assert part == "unsharded" or hd.stats()["partition"] == part
        # cold first call, and the matrix: equal to the unsharded handle's (exact)
        t0 = time.perf_counter()
        m = hd.all2all_dense()
        res[part].setdefault("cold_call_wall_ms", (time.perf_counter() - t0) * 1e3)
        if "m" not in ref:
            ref["m"] = m
        assert np.array_equal(m, ref["m"]), part
        handles[part] = hd
        return hd

    def call(part):
        if part == "unsharded":
            handles[part].all2all_dense_device(buf.data_ptr())
            torch.cuda.synchronize()
            return handles[part].stats()["kernel_ms"]
        handles[part].all2all_dense()
        return handles[part].stats()["call_ms"]

    def close_handle(part):
        hd = handles.pop(part)
        if part == "unsharded":
            st = hd.stats()
            res[part].update(resident_nodes=int(st["n_patterns"]), records=int(st["n_records"] + st["n_direct"]), h2d_bytes=int(st["h2d_bytes"]), width=int(st["width"]))
        else:
            ds = hd.stats()["devices"]
            res[part].update(resident_nodes=int(sum(x["n_patterns"] for x in ds)), records=int(sum(x["n_records"] for x in ds)),
                             h2d_bytes=int(sum(x["h2d_bytes"] for x in ds)))
        hd.close()

    if together:
        for part in views:
            open_handle(part)
        for part in views:                                      # warm up each
            call(part)
        for _ in range(rounds):                                 # alternate the three
            for part in views:
                ms[part].append(call(part))
        for part in views:
            close_handle(part)
    else:
        # the three working sets do not fit the device side by side: one handle at a time, the unsharded one before and after the two
        # node handles (its spread over both visits is the noise floor)
        for part in ("unsharded", "prefix", "range", "unsharded"):
            open_handle(part)
            call(part)
            for _ in range(rounds):
                ms[part].append(call(part))
            close_handle(part)
    out["handles_resident_together"] = bool(together)
    assert res["range"]["resident_nodes"] == formula           # exact
    out["matrices_equal"] = True
    out["sum_matrix"] = int(ref["m"].astype(np.uint64).sum())
    ref.clear()
    for part in views:
        res[part]["sum_call_ms"] = spread(ms[part])
        res[part]["sum_call_ms_rounds"] = [float(x) for x in ms[part]]
    res["prefix"]["per_shard"] = per_shard(K, torch, view_ht, dev, "prefix_shard", R, buf)
    res["range"]["per_shard"] = per_shard(K, torch, view, dev, "tree_range", R, buf)
    for part in ("prefix", "range"):
        c = [r["call_ms"] for r in res[part]["per_shard"]]
        res[part]["per_shard_imbalance_max_over_mean"] = max(c) / (sum(c) / len(c))
    cost = plan["cost"].astype(np.float64)
    res["range"]["est_cost_imbalance_max_over_mean"] = float(cost.max() / cost.mean())
    un = res["unsharded"]["sum_call_ms"]
    out["noise_floor_ms"] = un["max"] - un["min"]              # the spread of the unsharded call across the rounds
    out["range_over_unsharded"] = res["range"]["sum_call_ms"]["median"] / un["median"]
    out["prefix_over_unsharded"] = res["prefix"]["sum_call_ms"]["median"] / un["median"]
    out["prefix_minus_range_ms"] = res["prefix"]["sum_call_ms"]["median"] - res["range"]["sum_call_ms"]["median"]
    out["partitions"] = res
    return out


def load_times(K, reps=7):
    """kmdbh_db_load with the hashtables (mode 0) and without (mode 2) on the largest database the repository carries with real hashtables"""
    src = os.path.join(ROOT, "tests", "golden", "clade64.db.xz")
    with tempfile.TemporaryDirectory() as td:
        path = os.path.join(td, "clade64.db")
        with lzma.open(src) as f, open(path, "wb") as o:
            o.write(f.read())
        t = {0: [], 2: []}
        for _ in range(reps):
            for mode in (0, 2):
                t0 = time.perf_counter()
                h = K.HostDB(path, skip_hashtables=mode == 2)
                t[mode].append(time.perf_counter() - t0)
                h.close()
        return {"file": "tests/golden/clade64.db", "bytes": os.path.getsize(path), "mode0_everything_s": spread(t[0]), "mode2_skip_hashtables_s": spread(t[2])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="c3gpu")
    ap.add_argument("--shards", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--one-at-a-time", action="store_true", help="one handle resident at a time (c3gpu: the three working sets do not fit side by side)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "partition_ab.json"))
    args = ap.parse_args()
    import torch
    K = bench.import_kmerdb_amd()
    if K.device_count() == 0:
        raise SystemExit("partition_ab.py needs an MI355X")
    torch.cuda.set_device(args.device)
    out = {"what": "unsharded handle vs node driver x prefix buckets vs node driver x tree ranges, one device, one process, alternating rounds",
           "device": torch.cuda.get_device_name(args.device), "db_load": load_times(K), "workloads": []}
    for name in args.workloads.split(","):
        out["workloads"].append(run_workload(K, torch, name, args.shards, args.rounds, args.device, together=not args.one_at_a_time))
        with open(args.out, "w") as f:                          # (written after every workload: a later one that runs out of time loses nothing)
            json.dump(out, f, indent=1)
        w = out["workloads"][-1]
        log("%s: unsharded %.2f ms, prefix x%d %.2f ms, range x%d %.2f ms (noise floor %.2f ms)" % (
            name, w["partitions"]["unsharded"]["sum_call_ms"]["median"], args.shards, w["partitions"]["prefix"]["sum_call_ms"]["median"],
            args.shards, w["partitions"]["range"]["sum_call_ms"]["median"], w["noise_floor_ms"]))


if __name__ == "__main__":
    main()
