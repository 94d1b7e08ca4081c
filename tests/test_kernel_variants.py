"""Every kernel variant of all2all and new2all that a switch of the engine selects, not only the ones the default configuration launches:
the three ways of the narrow kernel's first-block records (KMDB_K1N_MODE 0 / 1 / 2: stream chunks and k2_apply_kernel, the matrix-core
step inside k1n_kernel<1, *>, compacted slices and k2d_kernel), few and many streams under each, KMDB_K1N_MINW, KMDB_K2D_SLICES, KMDB_K2D_EARLY and
KMDB_SYNC_DEBUG in child processes, the two launches of the decode kernel either side of
KMDB_SHORT_IDS, the sort inside the block rows on a random forest and a clade collection, and the eight instantiations of new2all's walk.  The inputs (tests/variant_cases.py) hold the edges
of these kernels on purpose — the int8 operand limit, the 32 / 32 split of the matrix-core tile, partial last blocks, changes of the first
block inside a slice — and a census on the host proves it before anything runs on a device.  All comparisons are exact (uint32 sums)."""
import functools
import importlib
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import variant_cases as V
from conftest import ROOT
from test_gpu_parity import _random_forest

SWITCHES = ("KMDB_K1N_MODE", "KMDB_ROW_MODE", "KMDB_BLOCK_WIDTH", "KMDB_NSEG", "KMDB_DENSE", "KMDB_SLICES", "KMDB_L2_MIN", "KMDB_L2", "KMDB_POOL_PERCENT",
            "KMDB_SHORT_IDS", "KMDB_REC_PACKED", "KMDB_N2A_NO_RUNS", "KMDB_N2A_NO_NODES", "KMDB_N2A_THREADS",
            "KMDB_K1N_MINW", "KMDB_K2D_SLICES", "KMDB_K2D_EARLY", "KMDB_SYNC_DEBUG", "KMDB_SP_ALL_TILES")


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
    import_kmerdb_amd()                                          # (registers the package under its importable name)
    return importlib.import_module("kmerdb_amd.synth")


def _oracle_of(O, pat, N):
    """the oracle's tree form and flat form of a forest (through a .db file in the reference's format)"""
    S = _S()
    arr = S.to_view_arrays(pat)
    with tempfile.TemporaryDirectory() as td:
        path = os.path.join(td, "f.db")
        S.write_db(path, 18, 1.0, ["s%d" % i for i in range(N)], [1] * N, arr)
        odb = O.OracleDB(path, skip_hashtables=True)
        tree, flat = odb.all2all_dense(), odb.all2all_flat()
        odb.close()
    return tree, flat


@functools.lru_cache(maxsize=None)
def _edge_case(width, N, light=False):
    """forest, definition, census and sparse rows of an edge forest (or light forest): computed once, shared by all tests, never written to"""
    pat = (V.light_forest if light else V.edge_forest)(width, N)
    exp = V.definition(pat, N)
    exp.setflags(write=False)
    return {"pat": pat, "exp": exp, "census": V.census(pat, width, N), "sparse": V.sparse_rows(exp, N)}


@functools.lru_cache(maxsize=None)
def _random_case(seed, N, P, max_local, chain):
    from oracle import oracle as O
    pat = _random_forest(np.random.default_rng(seed), N, P, max_local, heavy_frac=0.4, chain_frac=chain)
    exp, flat = _oracle_of(O, pat, N)
    assert np.array_equal(exp, flat)
    exp.setflags(write=False)
    return pat, exp


@functools.lru_cache(maxsize=None)
def _random_n_flat(case, width):
    """eligible first-block records with a weight below 128 of a random forest at a block width (host census)"""
    return V.census(_random_case(*case)[0], width, case[1], wrapped=False)["n_flat"]


RANDOM = ((41, 1000, 6000, 60, 0.2), (42, 2048, 3000, 300, 0.5), (43, 3000, 20000, 3, 0.9))


# ------------------------------------------------------------------------------------------------------------------------------------
# 1. host only: the references agree, the inputs hold their edges
# ------------------------------------------------------------------------------------------------------------------------------------
def test_edge_forests_hold_their_edges_and_the_references_agree(O):
    """Every edge forest (7 widths x 2 sample counts): the oracle's tree form == its flat form == variant_cases.definition, and the census
    of the host finds what the GPU tests rely on — eligible first-block records of weight 127 and of weight 128 (the int8 operand limit
    from both sides), cells whose exact sum passes 2^32 (the wrap-around), a partial last block (one sample / one short), weights on both
    sides of 128 among the eligible records (n_flat < n_first)."""
    for width in V.WIDTHS:
        for N in V.edge_sizes(width):
            case = _edge_case(width, N)
            pat, c = case["pat"], case["census"]
            assert pat["parent"].numel() <= 3000
            tree, flat = _oracle_of(O, pat, N)
            assert np.array_equal(tree, flat), (width, N)
            assert np.array_equal(tree, case["exp"]), (width, N, V.describe_mismatch(tree, case["exp"], N))
            assert c["w127"] >= 1 and c["w128"] >= 1, (width, N, c)
            assert c["wrapped"] >= 1, (width, N, c)
            assert c["last_block"] == (1 if N == 3 * width + 1 else width - 1) and c["last_block"] < width, (width, N, c)
            assert 0 < c["n_flat"] < c["n_first"], (width, N, c)
            # the sparse reference is the dense one, row by row
            rp, col, val = case["sparse"]
            for i in (1, 31, 32, width, N - 1):
                row = O.tri_row(case["exp"], i)
                assert np.array_equal(col[rp[i]: rp[i + 1]], np.nonzero(row)[0]) and np.array_equal(val[rp[i]: rp[i + 1]], row[np.nonzero(row)[0]])


def test_light_forests_leave_the_diagonal_tiles_to_the_first_block_kernels(O):
    """the light forests: references agree; every eligible first-block record has a weight below 128 (n_flat == n_first), and no node has two
    ids in a second block (no record (Y, Y) through the pools), so that only the first-block kernels add to — and flag — the diagonal tiles"""
    for width in V.WIDTHS:
        N = 3 * width + 1
        case = _edge_case(width, N, True)
        pat, c = case["pat"], case["census"]
        tree, flat = _oracle_of(O, pat, N)
        assert np.array_equal(tree, flat) and np.array_equal(tree, case["exp"]), (width, N)
        assert 0 < c["n_flat"] == c["n_first"] and c["w127"] >= 1 and c["w128"] == 0, (width, c)
        assert int(pat["num_kmers"].max()) < 128
        for full in V.full_lists(pat):
            blk = full // width
            assert full.size == 0 or (np.unique(blk).size <= 2 and (blk[-1] == blk[0] or int((blk == blk[-1]).sum()) == 1)), (width, full)
        for X in range(3):                                      # every full block's diagonal tile holds cells
            i = X * width + width - 1
            assert O.tri_row(case["exp"], i)[X * width:].any(), (width, X)


def test_decode_forest_holds_the_list_lengths_and_deltas(O):
    """the decode forest: local lists of 1, 2, 47, 48, 49, 63, 64, 65 and 128 ids, each in three delta shapes, as a root and under a parent
    of 40 ids; every delta 2^j - 1 and 2^j, j = 1 .. 11, occurs; ids 0 and N - 1 occur; oracle tree form == flat form == definition"""
    N = 4096
    pat = V.decode_forest(N)
    nl = pat["num_local"].numpy()
    par = pat["parent"].numpy()
    for L in (1, 2, 47, 48, 49, 63, 64, 65, 128):
        assert int(((nl == L) & (par < 0)).sum()) == 3 and int(((nl == L) & (par > 0)).sum()) == 3, L
    lp, ids = pat["local_ptr"].numpy(), pat["local_ids"].numpy()
    deltas = set()
    for p in range(1, len(nl)):
        deltas |= set(np.diff(ids[lp[p]: lp[p + 1]]).tolist())
    assert all((1 << j) - 1 in deltas and (1 << j) in deltas for j in range(1, 12))
    assert ids.min() == 0 and ids.max() == N - 1
    tree, flat = _oracle_of(O, pat, N)
    exp = V.definition(pat, N)
    assert np.array_equal(tree, flat) and np.array_equal(tree, exp)


# ------------------------------------------------------------------------------------------------------------------------------------
# 2. first-block modes on the edge forests
# ------------------------------------------------------------------------------------------------------------------------------------
def _same(got, exp, N, tag):
    assert got.shape == exp.shape and np.array_equal(got, exp), (tag, V.describe_mismatch(got, exp, N))


def _direct_ok(mode, nseg, n_direct, n_flat, tag):
    """kmdb_stats.n_direct against the census: mode 0 writes every record to the pools; mode 2 compacts every eligible record with a weight
    below 128; mode 1 applies those of a slice's FIRST block only — with slices of 64 nodes whose first blocks change, fewer than all"""
    if mode == 0:
        assert n_direct == 0, (tag, n_direct)
    elif mode == 2:
        assert n_direct == n_flat, (tag, n_direct, n_flat)
    elif nseg == 64:
        assert 0 < n_direct < n_flat, (tag, n_direct, n_flat)
    else:
        assert 0 < n_direct <= n_flat, (tag, n_direct, n_flat)


def _edge_run(K, dev, env, mode, rowmode, width, N, nseg, dense=None, light=False):
    case = _edge_case(width, N, light)
    exp, n_flat = case["exp"], case["census"]["n_flat"]
    _, view = V.make_view(K, _S(), case["pat"], N)
    NF, REC = K.capi.FLAG_NO_FALLBACK, K.capi.PATH_RECORDS
    tag = "%smode %d row mode %d width %d N %d nseg %s dense %s: " % ("light forest " if light else "", mode, rowmode, width, N, nseg, dense)
    sw = dict(KMDB_K1N_MODE=mode, KMDB_ROW_MODE=rowmode, KMDB_BLOCK_WIDTH=width, KMDB_NSEG=nseg, KMDB_DENSE=dense)
    env(**sw)
    d = K.DeviceDB(view, device=dev)
    got = d.all2all_dense(flags=NF)
    st = d.stats()
    assert st["path"] == REC and st["width"] == width, (tag, st)
    _same(got, exp, N, tag + "cold call")
    _direct_ok(mode, nseg, st["n_direct"], n_flat, tag + "cold call")
    got = d.all2all_dense(flags=NF)
    st = d.stats()
    assert st["path"] == REC and st["width"] == width and st["sized_call"] == 0, (tag, st)
    _same(got, exp, N, tag + "warm call")
    _direct_ok(mode, nseg, st["n_direct"], n_flat, tag + "warm call")
    acc, direct = np.zeros_like(exp), 0
    for s in range(3):
        acc += d.all2all_dense(shard=(s, 3), flags=NF)
        st = d.stats()
        assert st["path"] == REC and st["width"] == width, (tag, s, st)
        direct += st["n_direct"]
    _same(acc, exp, N, tag + "three shards")
    _direct_ok(mode, None if mode == 1 else nseg, direct, n_flat, tag + "three shards")       # (mode 1: a shard's first record decides its slices' tiles)
    sp = d.all2all_sparse()                                      # only the tiles the call flagged are scanned: a missed flag drops cells
    assert d.stats()["path"] == REC, tag
    rp, col, val = case["sparse"]
    assert np.array_equal(sp.row_ptr, rp) and np.array_equal(sp.col, col) and np.array_equal(sp.val, val), tag + "sparse rows"
    d.close()
    env(KMDB_SLICES=3, **sw)                                     # the call takes the pattern stream in three passes
    d = K.DeviceDB(view, device=dev)
    got = d.all2all_dense(flags=NF)
    st = d.stats()
    assert st["path"] == REC and st["width"] == width, (tag, st)
    _same(got, exp, N, tag + "KMDB_SLICES=3")
    _direct_ok(mode, None if mode == 1 else nseg, st["n_direct"], n_flat, tag + "KMDB_SLICES=3")
    d.close()


@pytest.mark.gpu
@pytest.mark.parametrize("rowmode", [0, 1])
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_first_block_modes_on_the_edge_forests(K, dev, env, mode, rowmode):
    """KMDB_K1N_MODE x KMDB_ROW_MODE over the edge forests: seven block widths, a last block of one sample and one short by one, slices of
    2048 and of 64 nodes (KMDB_NSEG; mode 0 also with KMDB_DENSE=2, its records through the sort).  Per handle, all on the block-record
    pipeline at the width set: cold call, warm call (sized_call == 0), three shards summed, a fresh handle under KMDB_SLICES=3 — each equal
    to the definition — the rows of all2all_sparse() equal to its non-zeros (row_ptr, col, val: tile_touched as written by dflush, k2d's
    flush and k2_apply), and kmdb_stats.n_direct against the census of the host (_direct_ok), summed over shards and over slices.  Per width
    also the light forest, whose diagonal tiles no other kernel flags."""
    for width in V.WIDTHS:
        for N in V.edge_sizes(width):
            for nseg in (None, 64):
                _edge_run(K, dev, env, mode, rowmode, width, N, nseg)
            if mode == 0:
                _edge_run(K, dev, env, mode, rowmode, width, N, 64, dense=2)
        _edge_run(K, dev, env, mode, rowmode, width, 3 * width + 1, 64, light=True)


# ------------------------------------------------------------------------------------------------------------------------------------
# 3. modes 0 and 1 on random and clade-shaped data
# ------------------------------------------------------------------------------------------------------------------------------------
def _against_oracle(K, dev, view, exp, N, tag, O):
    """cold call, warm call, sparse rows at seven sample rows; returns the cold call's stats"""
    NF = K.capi.FLAG_NO_FALLBACK
    d = K.DeviceDB(view, device=dev)
    got = d.all2all_dense(flags=NF)
    st = d.stats()
    assert st["path"] == K.capi.PATH_RECORDS, (tag, st)
    _same(got, exp, N, tag + " cold call")
    _same(d.all2all_dense(flags=NF), exp, N, tag + " warm call")
    assert d.stats()["sized_call"] == 0, tag
    sp = d.all2all_sparse()
    for i in range(0, N, max(1, N // 7)):
        c, v = sp.row(i)
        row = O.tri_row(exp, i)
        nz = np.nonzero(row)[0]
        assert np.array_equal(c, nz) and np.array_equal(v, row[nz]), (tag, "sparse row", i)
    d.close()
    return st


@pytest.mark.gpu
@pytest.mark.parametrize("rowmode", [0, 1])
@pytest.mark.parametrize("mode", [0, 1])
def test_modes_0_and_1_on_random_forests(K, O, dev, env, mode, rowmode):
    """What the suite gives mode 2 through the default configuration, for the stream chunks (0) and the in-kernel matrix-core step (1): random
    forests with weights of up to 32 bits, shallow and deep, short and long lists, at the estimated width, 32 and 64, few and many streams; in row
    mode at width 32 also under the second level (KMDB_L2_MIN=11: nodes joined per tile beside the modes' records)."""
    for seed, N, P, max_local, chain in RANDOM:
        pat, exp = _random_case(seed, N, P, max_local, chain)
        _, view = V.make_view(K, _S(), pat, N)
        for width in (None, 32, 64):
            env(KMDB_K1N_MODE=mode, KMDB_ROW_MODE=rowmode, KMDB_BLOCK_WIDTH=width)
            tag = "mode %d row mode %d seed %d width %s" % (mode, rowmode, seed, width)
            st = _against_oracle(K, dev, view, exp, N, tag, O)
            assert width is None or st["width"] == width, (tag, st)
            # mode 1 applies, of every slice, the eligible light records of its first such record's block: some if there are any, never more
            n_flat = _random_n_flat((seed, N, P, max_local, chain), st["width"])
            assert st["n_direct"] == 0 if mode == 0 or n_flat == 0 else 0 < st["n_direct"] <= n_flat, (tag, n_flat, st)
        if rowmode:
            env(KMDB_K1N_MODE=mode, KMDB_ROW_MODE=1, KMDB_BLOCK_WIDTH=32, KMDB_L2_MIN=11)
            st = _against_oracle(K, dev, view, exp, N, "mode %d row mode 1 seed %d width 32 second level" % (mode, seed), O)
            assert seed != 42 or st["n_joined"] > 0, st


@pytest.fixture(scope="module")
def clade(K, O, dev, tmp_path_factory):
    """the clade collection of test_pools_too_small_are_enlarged_and_the_call_repeated: 1200 samples in clades of 50; (view arrays, oracle)"""
    import torch
    S = _S()
    N, cs, L, k = 1200, 50, 3000, 18
    device = torch.device("cuda", dev)
    g, pat = S.synth_database(N, cs, L, k=k, seed=5, device=device)
    arr = S.to_view_arrays(pat)
    path = str(tmp_path_factory.mktemp("clade") / "s.db")
    S.write_db_fast(path, k, 1.0, [g.name(i) for i in range(N)], pat["sample_counts"], arr, device=device)
    exp = O.OracleDB(path, skip_hashtables=True).all2all_dense()
    exp.setflags(write=False)
    return N, k, arr, exp


def _clade_view(K, clade):
    N, k, arr, exp = clade
    return K.make_view(k, N, arr["num_kmers"], arr["parent_id"], arr["num_samples"], arr["num_local"], arr["last_sample_id"], arr["num_bits"],
                       arr["data_offset"], arr["data"])


@pytest.mark.gpu
@pytest.mark.parametrize("rowmode", [0, 1])
@pytest.mark.parametrize("mode", [0, 1])
def test_modes_0_and_1_on_a_clade_collection(K, O, dev, env, clade, mode, rowmode):
    """a clade collection whole, and with record pools of 1 % of the estimate: in mode 0 the chunk pool of the stream chunks goes through
    enlarge-and-repeat, in mode 1 the pools of the stragglers"""
    N, k, arr, exp = clade
    view = _clade_view(K, clade)
    for pct in (None, 1):
        env(KMDB_K1N_MODE=mode, KMDB_ROW_MODE=rowmode, KMDB_POOL_PERCENT=pct)
        st = _against_oracle(K, dev, view, exp, N, "mode %d row mode %d clades pools %s %%" % (mode, rowmode, pct), O)
        assert (st["n_direct"] > 0) == (mode == 1) and st["n_records"] > 0, st


# ------------------------------------------------------------------------------------------------------------------------------------
# 4. the switches read once per process
# ------------------------------------------------------------------------------------------------------------------------------------
CHILDREN = ({"KMDB_K1N_MODE": "1", "KMDB_K1N_MINW": "4"},            # k1n_kernel<1, 4>: four waves per SIMD, scratch
            {"KMDB_K2D_SLICES": "1"},
            {"KMDB_K2D_SLICES": "7", "KMDB_K2D_EARLY": "0"},          # 7 does not divide the number of slices; k2d_kernel started with the wide kernel
            {"KMDB_SYNC_DEBUG": "1", "KMDB_K1N_MODE": "0"},
            {"KMDB_SYNC_DEBUG": "1", "KMDB_K1N_MODE": "1"},
            {"KMDB_SYNC_DEBUG": "1", "KMDB_K1N_MODE": "2"})


@pytest.mark.gpu
def test_process_static_switches_in_child_processes(dev):
    """KMDB_K1N_MINW, KMDB_K2D_SLICES, KMDB_K2D_EARLY and KMDB_SYNC_DEBUG are read into static locals: one process each (variant_cases.py's
    __main__: edge forests of widths 50 and 64 against the definition, a random forest against the v1 kernel; cold, warm, sparse rows).  One
    after the other; the first child that fails ends the test — after a child that died nothing more is started on the device."""
    for extra in CHILDREN:
        e = {k: v for k, v in os.environ.items() if k not in SWITCHES}
        e.update(extra)
        label = " ".join("%s=%s" % kv for kv in sorted(extra.items()))
        try:
            r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "variant_cases.py"), label], env=e, capture_output=True, text=True, timeout=240)
        except subprocess.TimeoutExpired as x:
            pytest.fail("child '%s' timed out; no further child started\nstderr: %s" % (label, (x.stderr or b"")[-3000:]))
        if r.returncode != 0:
            pytest.fail("child '%s' exited with %d%s; no further child started\nstdout: %s\nstderr: %s" %
                        (label, r.returncode, " (killed by a signal)" if r.returncode < 0 else "", r.stdout[-3000:], r.stderr[-3000:]))
        last = r.stdout.strip().splitlines()[-1]
        assert last.endswith(" cases, 0 mismatches") and int(last.split()[0]) > 0, (label, r.stdout[-2000:])
        if "KMDB_SYNC_DEBUG" in extra:
            stages = [ln for ln in r.stderr.splitlines() if ln.startswith("[kmdb] stage ")]
            assert any(ln.split()[2:4] == ["narrow", "emit"] for ln in stages) and all(ln.endswith(" ok") for ln in stages), (label, r.stderr[-2000:])


# ------------------------------------------------------------------------------------------------------------------------------------
# 5. decode boundary, row histogram
# ------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _decode_case():
    from oracle import oracle as O
    N = 4096
    pat = V.decode_forest(N)
    exp = V.definition(pat, N)
    tree, flat = _oracle_of(O, pat, N)
    assert np.array_equal(tree, exp) and np.array_equal(flat, exp)
    exp.setflags(write=False)
    return N, pat, exp


@pytest.mark.gpu
@pytest.mark.parametrize("short_ids", [None, 1, 47, 64])
def test_decode_launches_either_side_of_the_short_list_boundary(K, dev, env, short_ids):
    """k0_decode_kernel<false> takes the lists of up to KMDB_SHORT_IDS ids (48), k0_decode_kernel<true> the longer ones: lists of 47 / 48 / 49 and
    63 / 64 / 65 ids, deltas where the gamma code changes length, the first and the last sample id — with the boundary at 48, at 1 (every list but
    the single ids is long), 47 and 64 (no list of one wave is long) — against the definition (== the oracle), and the three v1 kernels with them"""
    N, pat, exp = _decode_case()
    _, view = V.make_view(K, _S(), pat, N)
    env(KMDB_SHORT_IDS=short_ids)
    d = K.DeviceDB(view, device=dev)
    _same(d.all2all_dense(flags=K.capi.FLAG_NO_FALLBACK), exp, N, "short ids %s" % short_ids)
    assert d.stats()["path"] == K.capi.PATH_RECORDS
    for fl in (K.capi.FLAG_FORCE_TILE, K.capi.FLAG_FORCE_GLOBAL_ATOMICS, K.capi.FLAG_FORCE_DIRECT):
        _same(d.all2all_dense(flags=fl), exp, N, "short ids %s, v1 flag %d" % (short_ids, fl))
    d.close()


@pytest.mark.gpu
def test_row_histogram_on_random_and_clade_inputs(K, O, dev, env, clade):
    """rs_hist_kernel<16> and the rest of the many-streams path in the default mode of the narrow kernel: a random forest and a clade collection"""
    seed, N, P, max_local, chain = RANDOM[1]
    pat, exp = _random_case(seed, N, P, max_local, chain)
    _, view = V.make_view(K, _S(), pat, N)
    env(KMDB_ROW_MODE=1)
    _against_oracle(K, dev, view, exp, N, "row mode seed %d" % seed, O)
    _against_oracle(K, dev, _clade_view(K, clade), clade[3], clade[0], "row mode clades", O)


# ------------------------------------------------------------------------------------------------------------------------------------
# 6. new2all: the eight instantiations of the walk
# ------------------------------------------------------------------------------------------------------------------------------------
N2A_VARIANTS = ({}, {"KMDB_N2A_NO_RUNS": 1}, {"KMDB_N2A_NO_NODES": 1}, {"KMDB_N2A_THREADS": 1024}, {"KMDB_N2A_NO_RUNS": 1, "KMDB_N2A_THREADS": 1024})


@pytest.mark.gpu
@pytest.mark.parametrize("N,P,max_local", [(700, 600, 60), (10000, 3000, 300), (12000, 3000, 400)])
def test_new2all_walk_variants(K, O, dev, env, tmp_path, N, P, max_local):
    """n2a_walk_kernel<lds_hist, threads, 1024, runs>: the per-query histogram in LDS or in memory (N 4 + 16384 + threads 8 + 1024 <= 65536: 700
    samples inside for both thread counts, 10 000 inside for 512 and outside for 1024, 12 000 outside for both), 512 / 1024 threads
    (KMDB_N2A_THREADS), with the run index and without (KMDB_N2A_NO_RUNS: what a handle without memory for the index does), and the climb
    over the engine's arrays (KMDB_N2A_NO_NODES).  A fresh handle per variant (the index is tried once per handle).  Forests with fabricated
    dictionaries; queries half present and half absent, all absent, a single k-mer, none.  new2all == the oracle's one2all, the rows of
    new2all_sparse == its non-zeros; and the same over two query shards, summed."""
    import torch
    S = _S()
    rng = np.random.default_rng(6000 + N)
    k, n_kmers = 18, 5000
    pat = _random_forest(rng, N, P, max_local, chain_frac=0.4)
    pids = np.sort(rng.integers(1, P, size=n_kmers))
    pat["num_kmers"] = torch.from_numpy(np.bincount(pids, minlength=P).astype(np.int64))
    universe = rng.choice(1 << 36, size=9000, replace=False).astype(np.uint64)
    present, absent = universe[:n_kmers], universe[n_kmers:]
    kmers = np.sort(present)
    arr = S.to_view_arrays(pat)
    tables = S.build_hashtables(torch.from_numpy(kmers.astype(np.int64)), torch.from_numpy(rng.permutation(pids).astype(np.int64)), k)
    path = str(tmp_path / "n.db")
    S.write_db(path, k, 1.0, ["s%d" % i for i in range(N)], [1] * N, arr, kmers_count=n_kmers, tables=tables)
    qs = [K.sort_unique(np.concatenate([rng.choice(present, m, replace=False), rng.choice(absent, m, replace=False)])) for m in (40, 300, 900, 1500, 2500)]
    qs += [K.sort_unique(absent[:500]), kmers[:1].copy(), np.zeros(0, np.uint64)]
    odb = O.OracleDB(path)
    exp = np.stack([odb.one2all(q) for q in qs])
    assert exp[:5].any(axis=1).all() and not exp[5].any() and exp[6].any() and not exp[7].any()
    nz = [np.nonzero(r)[0] for r in exp]
    h = K.HostDB(path)

    def check(d, tag):
        got = d.new2all(qs)
        assert np.array_equal(got, exp), (tag, [int((g != e).sum()) for g, e in zip(got, exp)])
        sp = d.new2all_sparse(qs)
        assert sp.n_rows == len(qs), tag
        for qi in range(len(qs)):
            c, v = sp.row(qi)
            assert np.array_equal(c, nz[qi]) and np.array_equal(v, exp[qi][nz[qi]]), (tag, qi)
        assert np.array_equal(d.new2all(qs), exp), (tag, "second call")

    for variant in N2A_VARIANTS:
        env(**variant)
        d = K.DeviceDB(h, device=dev, with_hashtables=True)
        check(d, (N, variant))
        d.close()
    for variant in ({}, {"KMDB_N2A_NO_RUNS": 1, "KMDB_N2A_THREADS": 1024}):
        env(**variant)
        acc = np.zeros_like(exp)
        for s in range(2):
            d = K.DeviceDB(h, device=dev, query_shard=(s, 2))
            one = d.new2all(qs)
            assert one.any(), (N, variant, s)
            acc += one
            d.close()
        assert np.array_equal(acc, exp), (N, variant, "query shards")
