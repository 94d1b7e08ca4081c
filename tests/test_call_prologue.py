"""The start of the all2all call and its wide list: the per-call state cleared by one launch, a wide pool whose key words are NOT filled before
the call (which slots hold a record follows from the sub-pools' cursors and from what the emitting waves mark when they end), and the wide list
built from the narrow kernel's own counts (per 64-node word, per slice).  Every matrix is compared with the flat-form definition in numpy,
kmdb_stats.n_wide with the host's count of the nodes whose full list has more than two blocks (prologue_cases.n_wide_of: the level sweep of
profiles/r04_record_stats.py, from the forest)."""
import os
import subprocess
import sys

import pytest

import prologue_cases as C
from conftest import ROOT
from test_kernel_variants import SWITCHES, dev, env        # noqa: F401  (fixtures)


def _run(K, c, key, tag, more):
    _, S = C._synth()
    bad = C.stale_key_sequence(K, S, c, key[2], key[1], tag, more=more)
    assert not bad, "\n".join(bad)


# ------------------------------------------------------------------------------------------------------------------------------------
# 1. stale keys
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("width,N", [(50, 151), (32, 127), (64, 255)])
def test_stale_keys_of_earlier_calls_are_not_taken_for_records(K, dev, env, width, N):
    """Few streams (4 blocks, 10 streams), one handle: a full call, the four calls shard=(i, 4) summed into a zeroed matrix, a full call, five
    more full calls — each result equal to the definition.  After a full call nearly every slot of the wide pool holds a valid-looking key of
    that call; a sliced call writes a fraction of them and the wide kernel's dynamic run hand-out moves records between calls: a slot
    wrongly taken as written changes the matrix."""
    env(KMDB_BLOCK_WIDTH=width)
    key = ("edge", width, N)
    _run(K, C.case(*key), key, "stale keys", more=5)


# ------------------------------------------------------------------------------------------------------------------------------------
# 2. / 3. / 4. child processes: pools of one percent, the other record paths of the narrow kernel, slices of 64 nodes, many streams
# ------------------------------------------------------------------------------------------------------------------------------------
def _child(extra, names):
    e = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    e.update(extra)
    e["KMDB_VERBOSE"] = "1"
    label = " ".join("%s=%s" % kv for kv in sorted(extra.items())) or "default"
    try:
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "prologue_cases.py"), label] + list(names), env=e, capture_output=True, text=True, timeout=120)
    except subprocess.TimeoutExpired as x:
        pytest.fail("child '%s' timed out\nstderr: %s" % (label, (x.stderr or b"")[-3000:]))
    assert r.returncode == 0, "child '%s' exited with %d%s\nstdout: %s\nstderr: %s" % (
        label, r.returncode, " (killed by a signal)" if r.returncode < 0 else "", r.stdout[-3000:], r.stderr[-3000:])
    last = r.stdout.strip().splitlines()[-1]
    assert last.endswith(" cases, 0 mismatches") and int(last.split()[0]) > 0, (label, r.stdout[-2000:])
    return r


@pytest.mark.gpu
@pytest.mark.parametrize("extra", [{"KMDB_POOL_PERCENT": "1"}, {"KMDB_K1N_MODE": "0"}, {"KMDB_K1N_MODE": "1"}, {"KMDB_POOL_PERCENT": "1", "KMDB_K1N_MODE": "0"}],
                         ids=lambda x: ",".join("%s=%s" % kv for kv in sorted(x.items())))
def test_stale_keys_with_the_switches_of_a_process(dev, extra):
    """The sequence of test 1 in a process of its own: KMDB_POOL_PERCENT=1 (and a forest of five million records, more than the smallest
    wide pool holds: its first call takes the enlarge-and-repeat path — the prologue runs again, the repeated attempt starts from the cursors and
    keys of the one that ran over), KMDB_K1N_MODE 0 and 1 (the narrow kernel's other record
    paths: every one reserves slots of the wide pool and marks what it leaves unwritten)."""
    r = _child(extra, ["stale", "pools"] if "KMDB_POOL_PERCENT" in extra else ["stale"])
    if "KMDB_POOL_PERCENT" in extra:
        assert "wide record pool too small" in r.stderr, r.stderr[-2000:]          # (KMDB_VERBOSE: the first call of the "pools" forest was repeated)


@pytest.mark.gpu
@pytest.mark.parametrize("width,N,name,args", [(50, 151, "light", ()), (32, 200, "fan", (3, 2300)), (32, 300, "chain", (2,))] +
                         [(32, 130, "padded", (p,)) for p in C.WIDE_P], ids=lambda x: str(x).replace(" ", ""))
def test_wide_list_from_the_narrow_kernels_counts(K, dev, env, width, N, name, args):
    """n_wide == the host's count and the matrix == the definition, at the default slices of 2048 nodes: a forest without any wide node; fans in
    which every node of three whole slices is wide; chains whose nodes are wide slice after slice; P of 63, 64, 65, 2047, 2048, 2049 and
    4097 patterns (a last word of 63 / 64 / 1 nodes, a second slice of one node) with wide nodes at both ends of the stream."""
    env(KMDB_BLOCK_WIDTH=width)
    key = (name, width, N) + tuple(args)
    c = C.case(*key)
    assert name != "light" or c["n_wide"] == 0
    assert name != "fan" or c["n_wide"] == c["P"] - 2 > 3 * 2048
    assert name != "padded" or c["P"] == args[0]
    _run(K, c, key, "wide list", more=1)


@pytest.mark.gpu
@pytest.mark.parametrize("extra", [{"KMDB_NSEG": "64"}, {"KMDB_NSEG": "64", "KMDB_K1N_MODE": "0"}, {"KMDB_NSEG": "192"}],
                         ids=lambda x: ",".join("%s=%s" % kv for kv in sorted(x.items())))
def test_wide_list_with_slices_of_64_nodes(dev, extra):
    """The same forests with slices of 64 nodes (one word of wide bits per slice: every slice total is one word's count, a hundred slices are all
    wide), and with slices of 192 nodes, three words each: no power of two, the expand kernel divides instead of shifting."""
    _child(extra, ["wide"])


@pytest.mark.gpu
@pytest.mark.parametrize("rowmode_env", [{"KMDB_ROW_MODE": "1"}, {"KMDB_ROW_MODE": "1", "KMDB_L2": "0"}], ids=["second level", "no second level"])
def test_many_streams_path_forced_on_the_edge_forests(K, dev, env, rowmode_env):
    """The full / sliced / full sequence through the row-mode prologue (the chunk table is all there is: no wide pool) on the edge forests."""
    for width, N in ((50, 151), (64, 255)):
        env(KMDB_BLOCK_WIDTH=width, **rowmode_env)
        key = ("edge", width, N)
        _run(K, C.case(*key), key, "row mode %s" % rowmode_env, more=1)


@pytest.mark.gpu
def test_many_streams_handle_of_more_than_2048_block_pairs(dev):
    """66 blocks of 32 samples: 2211 streams, the many-streams path by itself, in a child (KMDB_BLOCK_WIDTH).  (edge_forest(32, 2081) holds a chain
    through all samples whose definition alone takes numpy nearly a minute: fans and padded forests over the same blocks instead, and the edge
    forests through the same path in the test above.)"""
    r = _child({}, ["rows"])
    assert "rows>" in r.stderr, r.stderr[-2000:]          # the instantiations of the many-streams path ran
