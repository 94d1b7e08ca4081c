#!/usr/bin/env python3
"""Same-box A/B of library BUILDS (the parent commit's libkmdb_amd.so, this tree's, builds with one constant changed) and of run-time switches:
the workload's database is generated once (kept in shared memory), every variant runs in a process of its own with its library: 3 warm calls, then
20 timed ones; prints one "AB {...}" line per variant — call and stage times from the engine's HIP events, sha256 of the matrix (equal across builds).

    python profiles/emit_specialisation_ab.py [--fresh] c2 <parent>/libkmdb_amd.so kmer-db_amd/libkmdb_amd.so <variant>.so:KMDB_K1W_RUN=128 ...
(library paths relative to the repository root; `--child` is the other side of the driver loop).  profiles/emit_specialisation_ab.json holds the lines."""
import hashlib
import json
import os
import subprocess
import sys

SEED = 20260929
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))          # the repository root (this file lives in profiles/)
sys.path.insert(0, ROOT)


def child(wl_name, libpath, steps):
    import numpy as np
    import torch
    import bench as B
    K = B.import_kmerdb_amd()
    import importlib
    capi = importlib.import_module("kmerdb_amd.capi")
    capi.lib_path = lambda: libpath
    wl = B.WORKLOADS[wl_name]
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    # the generated arrays, kept for the other processes of the job: keyed by everything the generator is given; --fresh (AB_FRESH) generates anew
    cache = "/dev/shm/kmdb_ab_%s_n%d_c%d_l%d_k18_seed%d" % (wl_name, wl["samples"], wl["clade_size"], wl["length"], SEED)
    if os.environ.get("AB_FRESH") == "1" and os.path.isdir(cache):
        import shutil
        shutil.rmtree(cache)
    if os.path.exists(os.path.join(cache, "done")):
        arr = {nm[:-4]: np.load(os.path.join(cache, nm)) for nm in os.listdir(cache) if nm.endswith(".npy")}
    else:
        arr, names, counts, nk, _ = B.generate_in_child(0, n_samples=wl["samples"], clade_size=wl["clade_size"], length=wl["length"], k=18, seed=SEED, rank=0, world=1)
        os.makedirs(cache, exist_ok=True)
        for nm, a in arr.items():
            np.save(os.path.join(cache, nm + ".npy"), a)
        open(os.path.join(cache, "done"), "w").close()
    db, up = B.upload(K, arr, wl["samples"], 18, 0)
    cells = db.tri_size()
    M = torch.zeros(max(cells, 1), dtype=torch.int32, device=dev)
    stream = torch.cuda.current_stream().cuda_stream
    for _ in range(3):
        db.all2all_dense_device(M.data_ptr(), stream=stream)
    torch.cuda.synchronize()
    ms, parts = [], []
    for _ in range(steps):
        db.all2all_dense_device(M.data_ptr(), stream=stream)
        s = db.stats()
        ms.append(s["kernel_ms"])
        parts.append((s["k0_ms"], s["k1n_ms"], s["k1g_ms"], s["k2_ms"]))
    torch.cuda.synchronize()
    got = M[:cells].cpu().numpy()
    st = db.stats()
    pk = np.mean(np.array(parts), axis=0)
    line = {"lib": os.path.relpath(libpath, ROOT), "env": os.environ.get("AB_ENV", ""), "workload": wl_name, "ms": round(float(np.mean(ms)), 4), "min_ms": round(float(np.min(ms)), 4),
            "max_ms": round(float(np.max(ms)), 4), "step_kernel_ms": [round(float(x), 3) for x in ms], "decode": round(float(pk[0]), 4), "narrow": round(float(pk[1]), 4), "wide": round(float(pk[2]), 4), "sort_apply": round(float(pk[3]), 4),
            "records": st["n_records"], "path": st.get("path"), "fallback": db.fallback_reason(), "sized_call": st.get("sized_call"),
            "sha": hashlib.sha256(got.tobytes()).hexdigest()[:16], "checksum_ok": int(got.view(np.uint32).astype(np.uint64).sum()) == int(st["sum_pairs"])}
    print("AB " + json.dumps(line), flush=True)
    db.close()


def main():
    if sys.argv[1] == "--child":
        child(sys.argv[2], sys.argv[3], int(sys.argv[4]))
        return
    args = [a for a in sys.argv[1:] if a != "--fresh"]
    wl = args[0]
    steps = 20
    fresh = "--fresh" in sys.argv                                 # the first variant's process generates the database anew
    for n, spec in enumerate(args[1:]):
        lib, _, envs = spec.partition(":")
        env = dict(os.environ)
        for kv in envs.split(","):
            if kv:
                k, _, v = kv.partition("=")
                env[k] = v
        env["AB_ENV"] = envs
        env["AB_FRESH"] = "1" if fresh and n == 0 else "0"
        r = subprocess.run(["timeout", "-k", "10", "300", sys.executable, os.path.abspath(__file__), "--child", wl, os.path.join(ROOT, lib), str(steps)], env=env)
        if r.returncode != 0:
            print("AB variant %s ended with %d: stopping" % (spec, r.returncode), flush=True)
            sys.exit(r.returncode)


if __name__ == "__main__":
    main()
