"""Inputs of test_call_prologue.py — forests that put the wide list's edges in play, the host count of the wide nodes, the call sequence that
leaves stale keys in the wide pool — and a __main__ for the settings that belong to a process of their own: test_call_prologue.py starts
`python tests/prologue_cases.py <label> <case> ...` with the switches in the child's environment.

Everything is compared with the flat-form definition in numpy (variant_cases.definition), never with a second run of the engine."""
import functools
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import variant_cases as V  # noqa: E402

WIDE_P = (63, 64, 65, 2047, 2048, 2049, 4097)


# ------------------------------------------------------------------------------------------------------------------------------------
# forests
# ------------------------------------------------------------------------------------------------------------------------------------
def padded_forest(width, N, P):
    """P patterns in all: three roots over three and four blocks with two children each (wide nodes at the stream's start), a wide pair at
    the stream's end, one-id root children between them — a last 64-node word of 63, 64, 1 nodes, a last slice that is short."""
    assert N >= 4 * width
    F = V._Forest()
    for t in range(3):
        r = F.add([t, width + t, 2 * width + t], -1, 2 + t)                      # three blocks: the wide kernel's
        F.add([2 * width + t + 1], r, 127 + t)
        c = F.add([3 * width + t], r, 3)                                         # four blocks
        F.add([3 * width + t + 1], c, 1)
    tail = 2
    pat_n = P - tail
    assert len(F.locs) <= pat_n
    i = 0
    while len(F.locs) < pat_n:
        F.add([(7 * i) % N], -1, 1 + i % 3)
        i += 1
    r = F.add([1, width + 1, 3 * width + 1], -1, 5)
    F.add([3 * width + 2], r, 128)
    assert len(F.locs) == P
    return F.pat()


def fan_forest(width, N, fans, children, root_blocks=3):
    """`fans` roots over `root_blocks` blocks (one id in each), each with `children` leaves of one further id: every node is wide, and with
    children in the thousands the nodes of several whole slices of the stream are — every word of wide bits all ones, every slice total the
    slice's size.  A two-id root child in front moves the fans off the slice boundary.  (Roots over eleven blocks and 65 000 children: five
    million records of 78 per node, more than the smallest wide pool holds.)"""
    last = (root_blocks - 1) * width
    assert N > last + 2
    F = V._Forest()
    F.add([0, 1], -1, 1)
    for f in range(fans):
        r = F.add([k * width + f % width for k in range(root_blocks - 1)] + [last], -1, 1 + f)
        for j in range(children):
            F.add([last + 1 + (j + f) % (N - last - 1)], r, (1, 2, 127, 128, 3)[j % 5])
    return F.pat()


def chain_forest(width, N, chains=2):
    """chains of one-id nodes through all samples: from the node of the third block on every node is wide, slice after slice"""
    F = V._Forest()
    for c in range(chains):
        par = -1
        for i in range(c, N):
            par = F.add([i], par, (1, 2, 127, 128, 3, 255)[(i + c) % 6])
    return F.pat()


def n_wide_of(pat, width):
    """nodes whose full list has more than two blocks, counted on the host"""
    return sum(1 for full in V.full_lists(pat) if full.size and np.unique(full // width).size > 2)


@functools.lru_cache(maxsize=None)
def case(name, width, N, *args):
    """forest, definition and wide-node count of a named case: computed once per process, shared, never written to"""
    make = {"edge": lambda: V.edge_forest(width, N), "light": lambda: V.light_forest(width, N), "padded": lambda: padded_forest(width, N, *args),
            "fan": lambda: fan_forest(width, N, *args), "chain": lambda: chain_forest(width, N, *args)}[name]
    pat = make()
    exp = V.definition(pat, N)
    exp.setflags(write=False)
    return {"pat": pat, "exp": exp, "n_wide": n_wide_of(pat, width), "P": len(pat["parent"])}


# ------------------------------------------------------------------------------------------------------------------------------------
# call sequences (the caller has set the environment)
# ------------------------------------------------------------------------------------------------------------------------------------
def _synth():
    import importlib
    from _kmerdb_loader import import_kmerdb_amd
    K = import_kmerdb_amd()
    return K, importlib.import_module("kmerdb_amd.synth")


def stale_key_sequence(K, S, c, N, width, tag, more=5, shards=4):
    """On ONE handle: a full call, the calls shard=(i, shards) summed into a zeroed matrix, a full call, `more` further full calls; every result
    against the definition, n_wide of every full call against the host's count.  After a full call nearly every slot of the wide pool holds a
    valid-looking key; a sliced call writes a fraction of them.  Returns the failures as strings."""
    NF, REC = K.capi.FLAG_NO_FALLBACK, K.capi.PATH_RECORDS
    exp, bad = c["exp"], []
    _, view = V.make_view(K, S, c["pat"], N)
    d = K.DeviceDB(view, device=0)

    def check(what, got, full_call=True):
        st = d.stats()
        if st["path"] != REC or (width is not None and st["width"] != width):
            bad.append("%s %s: not the block-record pipeline at width %s: %s" % (tag, what, width, st))
        if got.shape != exp.shape or not np.array_equal(got, exp):
            bad.append("%s %s: %s" % (tag, what, V.describe_mismatch(got, exp, N) if got.shape == exp.shape else "shapes differ"))
        if full_call and st["n_wide"] != c["n_wide"]:
            bad.append("%s %s: n_wide %d, the host counts %d" % (tag, what, st["n_wide"], c["n_wide"]))

    check("first full call", d.all2all_dense(flags=NF))
    acc = np.zeros_like(exp)
    for s in range(shards):
        acc += d.all2all_dense(shard=(s, shards), flags=NF)
    check("%d shards summed" % shards, acc, full_call=False)
    for k in range(1 + more):
        check("full call %d after the shards" % (k + 1), d.all2all_dense(flags=NF))
    d.close()
    return bad


CHILD_CASES = {
    # the stale-key sequence on the three forests of the in-process test
    "stale": lambda K, S: [("edge", w, n) for w, n in ((50, 151), (32, 127), (64, 255))],
    # the wide list's edges
    "wide": lambda K, S: [("light", 50, 151), ("fan", 32, 200, 3, 2300), ("chain", 32, 300, 2)] + [("padded", 32, 130, p) for p in WIDE_P],
    # more records than the smallest wide pool holds: with KMDB_POOL_PERCENT=1 the first call takes the enlarge-and-repeat path
    "pools": lambda K, S: [("fan", 32, 400, 1, 65000, 11)],
    # many streams: 66 blocks of 32 samples are 2211 block pairs
    "rows": lambda K, S: [("fan", 32, 2081, 2, 100), ("padded", 32, 2081, 2049), ("padded", 32, 2081, 4097)],
}


def _child(label, names):
    sys.path.insert(0, ROOT)
    K, S = _synth()
    assert K.device_count() > 0, "needs an MI355X"
    cases, bad = 0, []
    for nm in names:
        for key in CHILD_CASES[nm](K, S):
            c = case(*key)
            width, N = key[1], key[2]
            os.environ["KMDB_BLOCK_WIDTH"] = str(width)
            bad += stale_key_sequence(K, S, c, N, width, "%s %s" % (label, key), more=5 if nm == "stale" else 1)
            cases += 1
    for b in bad:
        print("MISMATCH " + b, flush=True)
    print("%d cases, %d mismatches" % (cases, len(bad)), flush=True)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(_child(sys.argv[1], sys.argv[2:]))
