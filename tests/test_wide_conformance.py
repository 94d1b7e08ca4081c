"""Conformance of the wide-node kernel (k1w_kernel), the second level above the block records (l2_*) and the sorts and stream jobs behind them
(cs_*, rs_*, k2j_*) at their thresholds.  The inputs (tests/wide_cases.py) are deterministic forests that hold every threshold from both
sides on purpose, and a census on the host proves it before anything runs on a device: the parent sources of a wide node (none, a parent of
one or two blocks, a wide parent in the batch, in an earlier batch, in an earlier run), seams, the whole-wave emission from 11 blocks on, the
second level's threshold, the LDS copy of the further own pairs (96), the row arena (256 entries), batch and run boundaries, root paths of
more than 64 wide nodes, more than 576 matches per tile, 63 | 64 and 256 | 257 blocks, 16 384 | 16 385 records of one stream.  KMDB_K1W_RUN
and KMDB_K1W_WAVES are set here.  Every matrix is compared with the flat-form definition in numpy (variant_cases.definition); all
comparisons are exact uint32 equality; kmdb_stats.n_wide, n_joined and n_records are held to the host's counts."""
import importlib
import re

import numpy as np
import pytest

import prologue_cases as C
import variant_cases as V
import wide_cases as W
from test_kernel_variants import _oracle_of

SWITCHES = ("KMDB_K1N_MODE", "KMDB_ROW_MODE", "KMDB_BLOCK_WIDTH", "KMDB_SLICES", "KMDB_L2_MIN", "KMDB_L2", "KMDB_POOL_PERCENT", "KMDB_REC_PACKED",
            "KMDB_K1W_RUN", "KMDB_K1W_WAVES", "KMDB_VERBOSE")


@pytest.fixture(scope="module")
def dev(K):
    assert K.device_count() > 0, "the -m gpu tests need an MI355X; the engine has no CPU fallback"
    return 0


@pytest.fixture
def env(monkeypatch):
    """set(name=value, ...) replaces ALL of the engine's switches by the ones given (None: unset)"""
    def set_(**kw):
        for name in SWITCHES:
            monkeypatch.delenv(name, raising=False)
        for name, value in kw.items():
            assert name in SWITCHES, name
            if value is not None:
                monkeypatch.setenv(name, str(value))
    set_()
    return set_


def _S():
    from _kmerdb_loader import import_kmerdb_amd
    import_kmerdb_amd()
    return importlib.import_module("kmerdb_amd.synth")


# ------------------------------------------------------------------------------------------------------------------------------------
# 1. host only: the forests hold their edges, the references agree
# ------------------------------------------------------------------------------------------------------------------------------------
def _feasible_shapes(c):
    """(own pairs as a class 1 / 2 / 5-and-more, seam) a node of c blocks can have under a WIDE parent: the parent has c - pairs + seam >= 3 blocks"""
    return [(k, seam) for k in (1, 2, 5) for seam in (False, True) if c - k + int(seam) >= 3]


@pytest.mark.parametrize("l2_min", [11, 24])
@pytest.mark.parametrize("run_nodes", [64, 256])
def test_wide_forest_holds_every_threshold_from_both_sides(run_nodes, l2_min):
    """the census of wide_forest at KMDB_K1W_RUN 64 / 256 and KMDB_L2_MIN 11 / 24: every class and every threshold occurs"""
    for width in (32, 50, 64):
        c = W.census_of("wide", (width, False), run_nodes, l2_min)
        cls = c["classes"]
        have = lambda blocks, source, seam=None, pairs=None: sum(n for (b, s, sm, k), n in cls.items() if b == blocks and s == source and      # noqa: E731
                                                                 (seam is None or sm == seam) and (pairs is None or k == pairs))
        assert 1000 < c["nodes"] < 5000
        chains = ("CHAIN_EARLIER_RUN",) if run_nodes == 64 else ("CHAIN_SAME_RUN", "CHAIN_EARLIER_RUN")
        assert run_nodes != 64 or not any(s == "CHAIN_SAME_RUN" for (_, s, _, _) in cls)          # (a run of 64 nodes is one batch)
        for blocks in W.CS_FULL:
            assert have(blocks, "NONE") >= 1, (blocks, "root")
            for source in ("FN1", "FN2"):
                assert have(blocks, source, seam=False) >= 1 and have(blocks, source, seam=True) >= 1, (blocks, source)
            for source in ("LANE",) + chains:
                for pairs, seam in _feasible_shapes(blocks):
                    assert have(blocks, source, seam, pairs) >= 1, (width, run_nodes, blocks, source, pairs, seam)
        # whole-wave emission from K1W_HEAVY blocks on, the second level from l2_min blocks on; diagonal pairs of a single id; in one batch
        # owners without records (no weight, or heavy) between owners of the record-parallel emission
        ab = c["acting_blocks"]
        assert ab.get(W.K1W_HEAVY - 1, 0) >= 1 and ab.get(W.K1W_HEAVY, 0) >= 1 and ab.get(l2_min - 1, 0) >= 1 and ab.get(l2_min, 0) >= 1, ab
        assert c["single_id_diagonals"] >= 1 and any(b["owners_without_records_between_owners"] for b in c["batches"])
        assert c["n_wide"] - sum(ab.values()) >= 10                                # wide nodes that do not act: ancestors whose lists are needed
        # the further own pairs of a batch: exactly K1W_OXCAP, and more with an in-batch descendant of a node that found no room
        assert any(b["ox"] == W.K1W_OXCAP for b in c["batches"]), [b["ox"] for b in c["batches"]]
        assert any(b["ox"] > W.K1W_OXCAP and b["walks_memory"] >= 1 for b in c["batches"])
        # the rows of a batch of 64 acting nodes that share nothing with the chain: exactly the arena, and more (several rounds)
        cap = W.arena_cap(36)
        assert cap == 256
        assert any(b["all_acting_narrow_based"] and b["rows"] == cap for b in c["batches"]), [b["rows"] for b in c["batches"]]
        assert any(b["all_acting_narrow_based"] and b["rows"] > cap for b in c["batches"])
        # batch and run edges; a root path of narrow ancestors first and then more than 64 wide ones at a run's start (second pass of the scan)
        assert c["child_at_lane0_of_parent_at_lane63"] >= 2 and c["child_at_run_start_of_parent_at_run_end"] >= 1, c
        assert any(narrow >= 1 and wides > W.WAVE for narrow, wides in c["run_starts"]), c["run_starts"]
        assert any(narrow == 0 and wides >= 1 for narrow, wides in c["run_starts"])
        # one class of runs (KMDB_K1W_WAVES=1): one cursor of L2_SUB hands out the node indices [0, 16), [256, 272), ...: more joined nodes than
        # one grab, and more than one cursor's share of the first arrays (4096 / L2_SUB = 256: the arrays are doubled and the call repeated)
        assert c["n_joined"] > 4096 // W.L2_SUB > W.L2_NODE_GRAB, c["n_joined"]


def test_wide_positions_63_to_65_and_255_to_257_are_one_root_path():
    pat = W.case("wide", 32, False)["pat"]
    par = pat["parent"].numpy().tolist()
    blocks = [np.unique(f // 32).size for f in V.full_lists(pat)]
    wide = [p for p in W.preorder(par) if blocks[p] > 2]
    for at in (63, 255):
        assert par[wide[at]] < 0 and par[wide[at + 1]] == wide[at] and par[wide[at + 2]] == wide[at + 1], at


def test_wide_forest_and_the_references_agree(O):
    """definition == the oracle's tree form == its flat form, for the wide forest (all weights, and the copy of one digit) at three widths"""
    for key in (("wide", 32, False), ("wide", 32, True), ("wide", 50, False), ("wide", 64, False)):
        c = W.case(*key)
        tree, flat = _oracle_of(O, c["pat"], c["N"])
        assert np.array_equal(tree, flat) and np.array_equal(tree, c["exp"]), (key, V.describe_mismatch(tree, c["exp"], c["N"]))
    w = W.case("wide", 32, True)["pat"]["num_kmers"].numpy()[1:]
    assert w.min() >= 1 and w.max() <= 127


def test_join_forest_holds_its_edges_and_the_references_agree(O):
    c = W.case("join")
    pat, N, width = c["pat"], c["N"], c["width"]
    assert N == 40 * 32
    tree, flat = _oracle_of(O, pat, N)
    assert np.array_equal(tree, flat) and np.array_equal(tree, c["exp"])
    tiles = W.join_census(pat, width)
    for t in ((7, 3), (3, 3), (7, 7)):
        assert tiles[t] == 700 + (70 if t == (3, 3) else 0) and tiles[t] > W.L2_QCAP, (t, tiles[t])
    # the 70 share one block pair with the 700, (3, 3), and no other
    heavy = [np.unique(f // width).tolist() for f in V.full_lists(pat)[1:]]
    assert all(len(b) == 11 for b in heavy)
    main, lone = [set(b) for b in heavy[:700]], [set(b) for b in heavy[700:]]
    assert all({3, 7} <= b for b in main) and len(lone) == 70
    assert set().union(*main) & set().union(*lone) == {3}
    cen = W.census(pat, width, 256, 11)
    assert cen["n_joined"] == 770 == cen["n_wide"] and cen["n_joined"] > 4096 // W.L2_SUB
    w = pat["num_kmers"].numpy()[1:]
    assert set(w.tolist()) == set(W.JOIN_WEIGHTS)
    digits = {max(1, (int(x).bit_length() + 6) // 7) for x in w}
    assert {1, 2, 3, 5} <= digits, digits
    exact = V.definition(pat, N, dtype=np.uint64)
    assert int((exact >= (1 << 32)).sum()) >= 1


def test_stream_forests_hold_16384_and_16385_records_of_one_stream(O):
    for n in (W.K2J_REC, W.K2J_REC + 1):
        for wide in (False, True):
            c = W.case("stream", n, wide)
            streams, rows = W.stream_census(c["pat"], c["width"])
            assert streams[(1, 0)] == n, streams[(1, 0)]
            assert streams[(1, 0)] > W.CS_TILE
            assert (rows[1] > W.RS_JOB_CHUNKS * W.CH_REC) == (n > W.K2J_REC), rows[1]      # 64 full chunks, or more
            cen = W.census(c["pat"], c["width"])
            assert (cen["n_wide"] > 0) == wide
    c = W.case("stream", 16385, True)
    tree, flat = _oracle_of(O, c["pat"], c["N"])
    assert np.array_equal(tree, flat) and np.array_equal(tree, c["exp"])
    c = W.case("stream", 17000, False)
    assert W.stream_census(c["pat"], 32)[0][(1, 0)] == 17000
    w = c["pat"]["num_kmers"].numpy()
    assert int((w >= 128).sum()) >= 3 and int(((w >= 1) & (w <= 127)).sum()) == 17000


def test_boundary_forests_hold_63_64_256_257_blocks(O):
    """N 2016 | 2017: 63 | 64 blocks of 32, 2016 | 2080 block pairs against CS_MAX_KEYS; N 8192 | 8193: 256 | 257 blocks.  Each holds the wide
    families (every source, seams, both sides of K1W_HEAVY and of the second level's threshold) and patterns with an id in every block."""
    for N, NB in zip(W.BOUNDARY_N, (63, 64, 256, 257)):
        c = W.case("boundary", N)
        assert (N + 31) // 32 == NB
        assert (NB * (NB + 1) // 2 <= W.CS_MAX_KEYS) == (NB == 63)
        cen = W.census(c["pat"], 32)
        srcs = {s for (_, s, _, _) in cen["classes"]}
        assert srcs == set(W.SOURCES), srcs
        ab = cen["acting_blocks"]
        assert all(ab.get(x, 0) >= 1 for x in (3, 10, 11, 23, 24)) and ab.get(NB, 0) >= 1 and ab.get(NB - 1, 0) + ab.get(NB, 0) >= 2, (N, sorted(ab))
        assert any(sm for (_, _, sm, _) in cen["classes"]) and any(not sm for (_, _, sm, _) in cen["classes"])
        if NB <= 64:
            tree, flat = _oracle_of(O, c["pat"], N)
            assert np.array_equal(tree, flat) and np.array_equal(tree, c["exp"]), N


def test_census_and_the_prologues_count_agree_on_n_wide():
    """prologue_cases.n_wide_of and wide_cases.census count the same nodes"""
    for key in (("chain", 32, 300, 2), ("padded", 32, 130, 65), ("padded", 32, 130, 2049), ("fan", 32, 200, 3, 2300), ("edge", 50, 151)):
        c = C.case(*key)
        assert W.census(c["pat"], key[1])["n_wide"] == c["n_wide"], key
    c = W.case("wide", 32, False)
    assert C.n_wide_of(c["pat"], 32) == W.census_of("wide", (32, False), 256, 24)["n_wide"]


# ------------------------------------------------------------------------------------------------------------------------------------
# 2. on the device
# ------------------------------------------------------------------------------------------------------------------------------------
def _same(got, exp, N, tag):
    assert got.shape == exp.shape and np.array_equal(got, exp), (tag, V.describe_mismatch(got, exp, N))


def _conform(K, dev, env, c, sw, tag, n_wide=None, n_joined=None, n_records=None, slices=True):
    """One handle under FLAG_NO_FALLBACK: a cold call, a warm call (sized_call == 0), three shards summed, the rows of all2all_sparse(); then a
    fresh handle under KMDB_SLICES=3 — each equal to the definition, each on the block-record pipeline.  n_wide of the full calls, n_joined and
    n_records of the warm full call against the host's counts.  Returns the warm call's stats."""
    exp, N = c["exp"], c["N"]
    NF, REC = K.capi.FLAG_NO_FALLBACK, K.capi.PATH_RECORDS
    _, view = V.make_view(K, _S(), c["pat"], N)
    env(**sw)
    d = K.DeviceDB(view, device=dev)
    got = d.all2all_dense(flags=NF)
    st = d.stats()
    assert st["path"] == REC and d.fallback_reason() == "" and st["width"] == c["width"], (tag, st, d.fallback_reason())
    _same(got, exp, N, tag + " cold call")
    assert n_wide is None or st["n_wide"] == n_wide, (tag, "cold call", st["n_wide"], n_wide)
    got = d.all2all_dense(flags=NF)
    warm = d.stats()
    assert warm["path"] == REC and warm["sized_call"] == 0, (tag, warm)
    _same(got, exp, N, tag + " warm call")
    print("%s: n_wide %d n_joined %d n_records %d n_direct %d (host: %s %s %s)" % (tag, warm["n_wide"], warm["n_joined"], warm["n_records"], warm["n_direct"],
                                                                                  n_wide, n_joined, n_records))
    assert n_wide is None or warm["n_wide"] == n_wide, (tag, "warm call", warm["n_wide"], n_wide)
    assert n_joined is None or warm["n_joined"] == n_joined, (tag, "n_joined", warm["n_joined"], n_joined)
    assert n_records is None or warm["n_records"] == n_records, (tag, "n_records", warm["n_records"], n_records)
    acc = np.zeros_like(exp)
    for s in range(3):
        acc += d.all2all_dense(shard=(s, 3), flags=NF)
        assert d.stats()["path"] == REC, (tag, s)
    _same(acc, exp, N, tag + " three shards")
    del acc
    sp = d.all2all_sparse()
    assert d.stats()["path"] == REC, tag
    rp, col, val = c["sparse"]
    assert np.array_equal(sp.row_ptr, rp) and np.array_equal(sp.col, col) and np.array_equal(sp.val, val), tag + " sparse rows"
    d.close()
    if slices:
        env(KMDB_SLICES=3, **sw)                                     # nodes outside the emitting range still feed the lists of nodes inside it
        d = K.DeviceDB(view, device=dev)
        got = d.all2all_dense(flags=NF)
        assert d.stats()["path"] == REC, tag
        _same(got, exp, N, tag + " KMDB_SLICES=3")
        d.close()
    return warm


MODES = {"few streams": {}, "rows, no L2": dict(KMDB_ROW_MODE=1, KMDB_L2=0), "rows, L2 from 11": dict(KMDB_ROW_MODE=1, KMDB_L2_MIN=11),
         "rows, L2 from 24": dict(KMDB_ROW_MODE=1)}
L2_MIN_OF = {"few streams": None, "rows, no L2": None, "rows, L2 from 11": 11, "rows, L2 from 24": 24}


@pytest.mark.gpu
@pytest.mark.parametrize("waves", [1, None])
@pytest.mark.parametrize("run_nodes", [64, 256])
@pytest.mark.parametrize("mode", list(MODES))
def test_wide_forest(K, dev, env, mode, run_nodes, waves):
    """wide_forest at width 32 over {few streams, row mode without / with the second level from 11 / from 24 blocks} x KMDB_K1W_RUN 64 / 256 x
    KMDB_K1W_WAVES 1 / unset: the matrix, n_wide and n_joined (acting nodes of l2_min blocks or more; 0 without the second level)"""
    c = W.case("wide", 32, False)
    l2_min = L2_MIN_OF[mode]
    cen = W.census_of("wide", (32, False), run_nodes, l2_min or 24)
    sw = dict(MODES[mode], KMDB_BLOCK_WIDTH=32, KMDB_K1W_RUN=run_nodes, KMDB_K1W_WAVES=waves)
    _conform(K, dev, env, c, sw, "wide forest, %s, run %d, waves %s" % (mode, run_nodes, waves), n_wide=cen["n_wide"],
             n_joined=cen["n_joined"] if l2_min else 0)


@pytest.mark.gpu
@pytest.mark.parametrize("width", [50, 64])
def test_wide_forest_at_other_widths(K, dev, env, width):
    """the same families rebuilt for blocks of 50 and of 64 ids (64: unpacked records), few streams"""
    c = W.case("wide", width, False)
    cen = W.census_of("wide", (width, False), 256, 24)
    _conform(K, dev, env, c, dict(KMDB_BLOCK_WIDTH=width), "wide forest, width %d" % width, n_wide=cen["n_wide"], n_joined=0)


@pytest.mark.gpu
@pytest.mark.parametrize("rowmode", [0, 1])
def test_n_records_is_the_hosts_record_count(K, dev, env, rowmode):
    """KMDB_K1N_MODE=0 (every record of the narrow kernel goes through the pools), no second level, every weight in 1 .. 127 (one digit): a
    warm full call's n_records == the census's record total over ALL acting nodes, the narrow ones included — block pairs a >= b of the full
    list, a diagonal pair only with two ids or more in the block."""
    c = W.case("wide", 32, True)
    cen = W.census_of("wide", (32, True), 256, 24)
    sw = dict(KMDB_BLOCK_WIDTH=32, KMDB_K1N_MODE=0, KMDB_ROW_MODE=rowmode, KMDB_L2=0)
    _conform(K, dev, env, c, sw, "n_records, row mode %d" % rowmode, n_wide=cen["n_wide"], n_joined=0, n_records=cen["n_records"])


@pytest.mark.gpu
@pytest.mark.parametrize("sw", [dict(KMDB_K1W_WAVES=1), {}, dict(KMDB_POOL_PERCENT=1)], ids=["one wave", "default", "pools of 1 %"])
def test_join_forest(K, dev, env, capfd, sw):
    """join_forest under KMDB_ROW_MODE=1 KMDB_L2_MIN=11: 770 nodes joined, more than L2_QCAP matches in three tiles, weights of one to five
    digits, cells that wrap.  With one wave (one cursor of L2_SUB in use) and with the smallest arrays (KMDB_POOL_PERCENT=1) the node indices run
    out: the arrays are doubled and the call repeated.  The same view then on a handle without the second level (the pipeline's switches are
    read once per handle)."""
    c = W.case("join")
    full = dict(sw, KMDB_BLOCK_WIDTH=32, KMDB_ROW_MODE=1, KMDB_L2_MIN=11, KMDB_VERBOSE=1)
    capfd.readouterr()
    _conform(K, dev, env, c, full, "join forest %s" % sw, n_wide=770, n_joined=770)
    err = capfd.readouterr().err
    assert "k1w<rows, L2>" in err, err[-2000:]
    if sw:
        assert "second level out of node indices or entries" in err, err[-2000:]
    _conform(K, dev, env, c, dict(full, KMDB_L2=0), "join forest %s, no second level" % sw, n_wide=770, n_joined=0, slices=False)


@pytest.mark.gpu
@pytest.mark.parametrize("packed", [None, 0])
@pytest.mark.parametrize("rowmode", [0, 1])
@pytest.mark.parametrize("n", [16384, 16385])
def test_stream_forest(K, dev, env, n, rowmode, packed):
    """one stream of exactly K2J_REC records and of one more (one job or two, two write-backs of one tile), more than CS_TILE records of one bin,
    a block row of more than RS_JOB_CHUNKS chunks; KMDB_K1W_WAVES=1: a wave's reservations run past the ends of its row chunks"""
    c = W.case("stream", n, bool(rowmode))
    _conform(K, dev, env, c, dict(KMDB_BLOCK_WIDTH=32, KMDB_ROW_MODE=rowmode, KMDB_REC_PACKED=packed, KMDB_K1W_WAVES=1),
             "stream forest %d, row mode %d, packed %s" % (n, rowmode, packed))


@pytest.mark.gpu
@pytest.mark.parametrize("N,wide", zip(W.BOUNDARY_N, ("k1w<no rows, no L2>", "k1w<rows, L2>", "k1w<rows, L2>", "k1w<rows, no L2>")))
def test_block_count_boundaries_by_the_engines_own_choice(K, dev, env, capfd, N, wide):
    """63 | 64 blocks (2016 | 2080 block pairs against CS_MAX_KEYS: few streams | row mode) and 256 | 257 blocks (second level | none), with neither
    KMDB_ROW_MODE nor KMDB_L2 set: the handle's first call names the instantiation, the matrix equals the definition"""
    c = W.case("boundary", N)
    cen = W.census(c["pat"], 32)
    capfd.readouterr()
    st = _conform(K, dev, env, c, dict(KMDB_BLOCK_WIDTH=32, KMDB_VERBOSE=1), "boundary N %d" % N, n_wide=cen["n_wide"],
                  n_joined=cen["n_joined"] if "<rows, L2>" in wide else 0)
    err = capfd.readouterr().err
    said = set(re.findall(r"\[kmdb\] wide kernel: .*instantiation (k1w<[^>]*>)", err))
    assert said == {wide}, (N, said, err[-2000:])
    assert st["width"] == 32
