"""The emit kernels are compiled once per record path (few streams; row mode; row mode with the second level): every path gives the
definition's matrix bit for bit on a cold and on a warm call, and the handle says which instantiation it launched — on the lines KMDB_VERBOSE
prints with a handle's first call ("[kmdb] narrow kernel: ... instantiation k1n<2, no rows>", "[kmdb] wide kernel: ... instantiation
k1w<no rows, no L2>").  A handle of another path in the same process must not inherit what the first one's instantiation was asked (the
number of waves the chip holds, the dynamic-LDS attribute).  Inputs and references: tests/variant_cases.py."""
import functools
import importlib
import re

import numpy as np
import pytest

import variant_cases as V
from test_gpu_parity import _random_forest

SWITCHES = ("KMDB_K1N_MODE", "KMDB_ROW_MODE", "KMDB_BLOCK_WIDTH", "KMDB_NSEG", "KMDB_DENSE", "KMDB_SLICES", "KMDB_L2_MIN", "KMDB_L2", "KMDB_POOL_PERCENT",
            "KMDB_REC_PACKED", "KMDB_K1W_RUN", "KMDB_K1W_WAVES", "KMDB_VERBOSE")
WIDTH = 50
FEW = dict(KMDB_BLOCK_WIDTH=WIDTH)
ROWS = dict(KMDB_BLOCK_WIDTH=WIDTH, KMDB_ROW_MODE=1, KMDB_L2=0)
ROWS_L2 = dict(KMDB_ROW_MODE=1, KMDB_BLOCK_WIDTH=32, KMDB_L2_MIN=11)


@pytest.fixture(scope="module")
def dev(K):
    assert K.device_count() > 0, "the -m gpu tests need an MI355X; the engine has no CPU fallback"
    return 0


@pytest.fixture
def env(monkeypatch):
    """set(name=value, ...) replaces the engine's switches by the ones given, and KMDB_VERBOSE=1"""
    def set_(**kw):
        for name in SWITCHES:
            monkeypatch.delenv(name, raising=False)
        for name, value in dict(kw, KMDB_VERBOSE=1).items():
            assert name in SWITCHES, name
            monkeypatch.setenv(name, str(value))
    return set_


def _S():
    from _kmerdb_loader import import_kmerdb_amd
    import_kmerdb_amd()
    return importlib.import_module("kmerdb_amd.synth")


@functools.lru_cache(maxsize=None)
def _edge(N):
    pat = V.edge_forest(WIDTH, N)
    exp = V.definition(pat, N)
    exp.setflags(write=False)
    return pat, exp


@functools.lru_cache(maxsize=None)
def _random41():
    """the forest of test_modes_0_and_1_on_random_forests' second-level case: at 32 blocks of 32 it has nodes of 11 blocks and more"""
    N = 1000
    pat = _random_forest(np.random.default_rng(41), N, 6000, 60, heavy_frac=0.4, chain_frac=0.2)
    exp = V.definition(pat, N)
    exp.setflags(write=False)
    return pat, exp, N


def _run(K, dev, capfd, pat, exp, N, tag, wide, narrow):
    """one handle: cold and warm call against the definition, the instantiations named on the first call's lines; returns the warm call's stats"""
    NF = K.capi.FLAG_NO_FALLBACK
    _, view = V.make_view(K, _S(), pat, N)
    capfd.readouterr()
    d = K.DeviceDB(view, device=dev)
    got = d.all2all_dense(flags=NF)
    st = d.stats()
    err = capfd.readouterr().err
    assert st["path"] == K.capi.PATH_RECORDS and d.fallback_reason() == "", (tag, st, d.fallback_reason())
    assert np.array_equal(got, exp), (tag, "cold call", V.describe_mismatch(got, exp, N))
    got = d.all2all_dense(flags=NF)
    st = d.stats()
    assert np.array_equal(got, exp), (tag, "warm call", V.describe_mismatch(got, exp, N))
    assert st["path"] == K.capi.PATH_RECORDS and st["sized_call"] == 0, (tag, st)
    d.close()
    said_w = set(re.findall(r"\[kmdb\] wide kernel: .*instantiation (k1w<[^>]*>)", err))
    said_n = set(re.findall(r"\[kmdb\] narrow kernel: .*instantiation (k1n<[^>]*>)", err))
    assert said_w == {wide} and said_n == {narrow}, (tag, said_w, said_n, err[-2000:])
    return st


@pytest.mark.gpu
@pytest.mark.parametrize("N", V.edge_sizes(WIDTH))
def test_few_streams(K, dev, env, capfd, N):
    env(**FEW)
    pat, exp = _edge(N)
    _run(K, dev, capfd, pat, exp, N, "few streams N %d" % N, "k1w<no rows, no L2>", "k1n<2, no rows>")


@pytest.mark.gpu
@pytest.mark.parametrize("N", V.edge_sizes(WIDTH))
def test_row_mode_without_second_level(K, dev, env, capfd, N):
    env(**ROWS)
    pat, exp = _edge(N)
    st = _run(K, dev, capfd, pat, exp, N, "row mode N %d" % N, "k1w<rows, no L2>", "k1n<2, rows>")
    assert st["n_joined"] == 0, st


@pytest.mark.gpu
def test_row_mode_with_second_level(K, dev, env, capfd):
    env(**ROWS_L2)
    pat, exp, N = _random41()
    st = _run(K, dev, capfd, pat, exp, N, "row mode, second level", "k1w<rows, L2>", "k1n<2, rows>")
    assert st["width"] == 32 and st["n_joined"] > 0, st          # (no node joined: the second-level branch did not run and the case proves nothing)


@pytest.mark.gpu
def test_path_change_between_handles(K, dev, env, capfd):
    """few streams, handle closed, then row mode (without and with the second level) in the same process, and few streams again"""
    N = V.edge_sizes(WIDTH)[1]
    pat, exp = _edge(N)
    env(**FEW)
    _run(K, dev, capfd, pat, exp, N, "first handle, few streams", "k1w<no rows, no L2>", "k1n<2, no rows>")
    env(**ROWS)
    _run(K, dev, capfd, pat, exp, N, "second handle, row mode", "k1w<rows, no L2>", "k1n<2, rows>")
    env(**ROWS_L2)
    rpat, rexp, rN = _random41()
    st = _run(K, dev, capfd, rpat, rexp, rN, "third handle, second level", "k1w<rows, L2>", "k1n<2, rows>")
    assert st["n_joined"] > 0, st
    env(**FEW)
    _run(K, dev, capfd, pat, exp, N, "fourth handle, few streams", "k1w<no rows, no L2>", "k1n<2, no rows>")
