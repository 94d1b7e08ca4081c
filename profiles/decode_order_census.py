#!/usr/bin/env python3
"""Census of the short decode launch's work on the arrays bench.py's generator makes, with torch on the device; no engine call.

    python profiles/decode_order_census.py [--fresh] c2 c3part   -> profiles/decode_order_census.json (one entry per workload)
    python profiles/decode_order_census.py --selftest       (CPU: the DFS order and the step counts against plain Python on a small forest)

Per workload: the shares of the nodes with l == 1, of the single runs (l > 1, stream bits == l - 1) and of the long nodes (more than 48 ids or 128
bits); the distribution of the decode steps of the short class — a step of RunCursor32 is a run of "0" codes and the code behind it, so a list
takes one step per delta above 1 plus one for a trailing run —; and the wave-iterations per 256 nodes of the decode loop when the nodes of every
window of W consecutive DFS nodes are sorted by the order's key and dealt 64 to a wave (a wave runs as many iterations as its slowest lane):
"before" = windows of 256 with a single run taking its one loop turn (the kernel that sorted inside the call), "after" = single runs take none.

The generated arrays are kept under /dev/shm/kmdb_ab_<workload>_..._seed<seed> — the cache profiles/emit_specialisation_ab.py keeps, so that one job
generates a workload once — beside a stamp of the generator's sources (kmer-db_amd/synth.py, bench.py); arrays without the stamp of THIS tree's generator
are made anew, and --fresh does so in any case.  Every census entry names where its arrays came from.
"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SEED = 20260929
SHORT_IDS, SHORT_BITS = 48, 128


def dfs_index(parent):
    """pre-order index of every pattern: roots in pattern order, children in pattern order inside a family (the layout's order)"""
    P = parent.numel()
    dev = parent.device
    ar = torch.arange(P, device=dev)

    def along_paths(val):
        """val[i] summed over the root path of i (pointer doubling)"""
        val, anc = val.clone(), parent.clone()
        while True:
            m = anc >= 0
            if not bool(m.any()):
                return val
            a = anc[m]
            val[m] += val[a]
            anc[m] = anc[a]
    depth = along_paths(torch.ones(P, dtype=torch.int64, device=dev))
    size = torch.ones(P, dtype=torch.int64, device=dev)
    by_depth = torch.argsort(depth, stable=True)
    counts = torch.bincount(depth)
    ends = torch.cumsum(counts, 0).tolist()
    for level in range(int(depth.max()), 1, -1):
        nodes = by_depth[ends[level - 1]: ends[level]]
        size.index_add_(0, parent[nodes], size[nodes])
    fam = torch.argsort(parent, stable=True)                     # families one after the other (the roots first), pattern order inside
    csum = torch.cumsum(size[fam], 0) - size[fam]
    fp = parent[fam]
    first = torch.ones(P, dtype=torch.bool, device=dev)
    first[1:] = fp[1:] != fp[:-1]
    start = torch.cummax(torch.where(first, torch.arange(P, device=dev), torch.zeros((), dtype=torch.int64, device=dev)), 0)[0]
    rel = torch.empty(P, dtype=torch.int64, device=dev)
    rel[fam] = csum - csum[start] + (fp >= 0).to(torch.int64)    # a child: behind its parent and its earlier siblings' subtrees
    del ar
    return along_paths(rel)


def decode_steps(nl, nb, doff, data):
    """steps of every list that has a stream (l > 1), 0 elsewhere; checks that every stream ends where its header says"""
    dev = nl.device
    u = np.ascontiguousarray(data.view(np.uint32).reshape(-1, 2)[:, ::-1]).reshape(-1).astype(np.int64)      # 32-bit units, first bits first
    U = torch.from_numpy(np.concatenate([u, np.zeros(2, np.int64)])).to(dev)
    idx = torch.nonzero(nl > 1).squeeze(1)
    pos0 = doff[idx] * 64
    pos, left = pos0.clone(), nl[idx] - 1
    steps = torch.zeros(nl.numel(), dtype=torch.int64, device=dev)
    zero_behind = torch.zeros(nl.numel(), dtype=torch.bool, device=dev)
    bad = 0
    while idx.numel():
        k, s = pos >> 5, pos & 31
        v = (((U[k] << 32) | U[k + 1]) >> (32 - s)) & 0xFFFFFFFF
        inv = (~v) & 0xFFFFFFFF
        assert bool((inv > 0).all()), "a code of 32 ones or more"
        ones = 32 - torch.frexp(inv.double())[1].to(torch.int64)          # leading ones of the 32-bit window
        pos = pos + 2 * ones + 1
        steps[idx] += (ones > 0).to(torch.int64)
        zero_behind[idx] = ones == 0
        left = left - 1
        done = left == 0
        if bool(done.any()):
            bad += int((pos[done] - pos0[done] != nb[idx[done]]).sum())
            keep = ~done
            idx, pos, pos0, left = idx[keep], pos[keep], pos0[keep], left[keep]
    assert bad == 0, "%d streams do not end where num_bits says" % bad
    return steps + zero_behind.to(torch.int64)


def keys_of(nl, nb):
    long_ = (nl > SHORT_IDS) | (nb > SHORT_BITS)
    extra = nb - (nl - 1)
    key = torch.clamp(2 + extra, max=63)
    key = torch.where(extra == 0, torch.full_like(key, 2), key)
    key = torch.where(nl == 1, torch.ones_like(key), key)
    return torch.where(long_ | (nl == 0), torch.zeros_like(key), key), long_


def wave_iterations(key, steps, W):
    """per 256 nodes: every window of W nodes sorted by decreasing key, 64 to a wave, a wave takes the most steps among its lanes"""
    P = key.numel()
    pad = (-P) % W
    k = torch.cat([key, torch.zeros(pad, dtype=key.dtype, device=key.device)])
    s = torch.cat([steps, torch.zeros(pad, dtype=steps.dtype, device=key.device)])
    win = torch.arange(k.numel(), device=key.device) // W
    order = torch.argsort(win * 64 + (63 - k), stable=True)
    return float(s[order].view(-1, 64).max(dim=1)[0].sum()) * 256.0 / P


def census(arr, dev):
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a.astype(np.int64))).to(dev)      # noqa: E731
    parent, nl, nb, doff = t(arr["parent_id"]), t(arr["num_local"]), t(arr["num_bits"]), t(arr["data_offset"])
    P = nl.numel()
    pre = dfs_index(parent)
    assert bool((torch.sort(pre)[0] == torch.arange(P, device=dev)).all()), "the pre-order is a permutation"
    steps_pid = decode_steps(nl, nb, doff, arr["data"])
    inv = torch.empty_like(pre)
    inv[pre] = torch.arange(P, device=dev)
    nl, nb, steps = nl[inv], nb[inv], steps_pid[inv]             # DFS order from here on
    key, long_ = keys_of(nl, nb)
    run_only = (nl > 1) & (nb == nl - 1) & ~long_
    short = key > 0
    steps = torch.where(short, steps, torch.zeros_like(steps))
    after = torch.where(run_only, torch.zeros_like(steps), steps)
    coded = short & ~run_only & (nl > 1)
    hist = torch.bincount(torch.clamp(steps[coded], max=32), minlength=33).tolist()
    out = {"patterns": P, "share_l1": float((nl == 1).sum()) / P, "share_run_only": float(run_only.sum()) / P, "share_long": float(long_.sum()) / P,
           "share_empty": float((nl == 0).sum()) / P, "mean_steps_short": float(steps[short].sum()) / max(int(short.sum()), 1),
           "mean_steps_coded": float(steps[coded].sum()) / max(int(coded.sum()), 1), "steps_hist_coded_0_to_32plus": hist,
           "wave_iterations_per_256": {"before_256": wave_iterations(key, steps, 256)}}
    for W in (256, 1024, 4096):
        out["wave_iterations_per_256"]["after_%d" % W] = wave_iterations(key, after, W)
    out["wave_iterations_per_256"]["after_ideal"] = float(after.sum()) / 64.0 * 256.0 / P
    live_waves = {}
    for W in (256, 1024, 4096):                                  # waves that hold a node to decode / waves that read a stream, per 256 nodes
        pad = (-P) % W
        k = torch.cat([key, torch.zeros(pad, dtype=key.dtype, device=dev)]).view(-1, W)
        n_live, n_coded = (k > 0).sum(1), (k > 2).sum(1)
        live_waves[str(W)] = {"live": float(((n_live + 63) // 64).sum()) * 256.0 / P, "reading_a_stream": float(((n_coded + 63) // 64).sum()) * 256.0 / P}
    out["waves_per_256"] = live_waves
    return out


def generator_stamp():
    import hashlib
    h = hashlib.sha256()
    for fn in (os.path.join(ROOT, "kmer-db_amd", "synth.py"), os.path.join(ROOT, "bench.py")):
        with open(fn, "rb") as f:
            h.update(f.read())
    return h.hexdigest()[:16]


def arrays_of(name, fresh=False):
    """-> (arrays, where they came from)"""
    import shutil
    import bench as B
    wl = B.WORKLOADS[name]
    cache = "/dev/shm/kmdb_ab_%s_n%d_c%d_l%d_k18_seed%d" % (name, wl["samples"], wl["clade_size"], wl["length"], SEED)      # (emit_specialisation_ab.py's)
    stamp_file, stamp = os.path.join(cache, "generator_sha16"), generator_stamp()
    if os.path.exists(os.path.join(cache, "done")):
        if not fresh and os.path.exists(stamp_file) and open(stamp_file).read().strip() == stamp:
            return {nm[:-4]: np.load(os.path.join(cache, nm)) for nm in os.listdir(cache) if nm.endswith(".npy")}, "cache %s (generator %s)" % (cache, stamp)
        shutil.rmtree(cache)
    arr = B.generate_in_child(0, n_samples=wl["samples"], clade_size=wl["clade_size"], length=wl["length"], k=18, seed=SEED, rank=0, world=1)[0]
    os.makedirs(cache, exist_ok=True)
    for nm, a in arr.items():
        np.save(os.path.join(cache, nm + ".npy"), a)
    with open(stamp_file, "w") as f:
        f.write(stamp + "\n")
    open(os.path.join(cache, "done"), "w").close()
    return arr, "generated (generator %s)" % stamp


def selftest():
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from _kmerdb_loader import import_kmerdb_amd
    import_kmerdb_amd()
    import importlib
    S = importlib.import_module("kmerdb_amd.synth")
    g, pat = S.synth_database(60, 7, 3000, k=18, seed=5, device="cpu")
    arr = S.to_view_arrays(pat)
    parent = arr["parent_id"]
    P = parent.size
    kids = [[] for _ in range(P)]
    roots = []
    for p in range(P):
        (kids[parent[p]] if parent[p] >= 0 else roots).append(p)
    pre, stack, n = np.zeros(P, np.int64), roots[::-1], 0
    while stack:
        p = stack.pop()
        pre[p] = n
        n += 1
        stack.extend(kids[p][::-1])
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a.astype(np.int64)))      # noqa: E731
    assert np.array_equal(dfs_index(t(parent)).numpy(), pre), "DFS order"
    lp, ids = pat["local_ptr"].numpy(), pat["local_ids"].numpy()
    want = np.zeros(P, np.int64)
    for p in range(P):
        d = np.diff(ids[lp[p]: lp[p + 1]])
        want[p] = int((d > 1).sum()) + int(d.size > 0 and d[-1] == 1)
    got = decode_steps(t(arr["num_local"]), t(arr["num_bits"]), t(arr["data_offset"]), arr["data"]).numpy()
    assert np.array_equal(got, want), "steps"
    c = census(arr, torch.device("cpu"))
    print("selftest ok:", json.dumps(c))


def main():
    if sys.argv[1:] == ["--selftest"]:
        return selftest()
    dev = torch.device("cuda", 0)
    path = os.path.join(ROOT, "profiles", "decode_order_census.json")
    out = {}
    if os.path.exists(path):
        with open(path) as f:
            out = json.load(f)
    fresh = "--fresh" in sys.argv
    for name in [a for a in sys.argv[1:] if a != "--fresh"]:
        arr, source = arrays_of(name, fresh)
        out[name] = dict(census(arr, dev), arrays=source)
        print("CENSUS %s %s" % (name, json.dumps(out[name])), flush=True)
        torch.cuda.empty_cache()
    dst = os.environ.get("CENSUS_OUT", path)
    with open(dst, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
