"""The short decode launch's work order: k0_decode_kernel<false> takes its nodes window by window in the order the layout made at
upload (lay_k0_order_kernel, KMDB_K0_WINDOW), waves behind a window's live count leave at once, and single ids and single runs never read their stream.
Whole matrices against variant_cases.definition, exactly; the order itself read back through kmdb_debug_k0_order.  Inputs: tests/decode_order_cases.py."""
import ctypes as C
import importlib

import numpy as np
import pytest

import all2all_rows_cases as RC
import build_cases as BC
import decode_order_cases as D
import variant_cases as V

SWITCHES = ("KMDB_K0_WINDOW", "KMDB_SHORT_IDS", "KMDB_BLOCK_WIDTH", "KMDB_K1N_MODE", "KMDB_ROW_MODE", "KMDB_NSEG", "KMDB_DENSE")


@pytest.fixture(scope="module")
def dev(K):
    assert K.device_count() > 0, "the -m gpu tests need an MI355X; the engine has no CPU fallback"
    return 0


@pytest.fixture
def env(monkeypatch):
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


def _order(K, d):
    """kmdb_debug_k0_order -> (W, order [windows][W], live [windows], l [P], stream bits [P])"""
    f = K.lib().kmdb_debug_k0_order
    f.argtypes = [C.c_void_p] * 7
    f.restype = C.c_int
    W, n_win = C.c_uint32(), C.c_uint64()
    assert f(d._d, C.byref(W), C.byref(n_win), None, None, None, None) == 0
    W, n_win = int(W.value), int(n_win.value)
    order, live = np.zeros((n_win, W), np.uint16), np.zeros(n_win, np.uint32)
    l, nbits = np.zeros(d.P, np.uint32), np.zeros(d.P, np.uint32)
    assert f(d._d, None, None, order.ctypes.data, live.ctypes.data, l.ctypes.data, nbits.ctypes.data) == 0
    return W, order, live, l, nbits


def _upload(K, dev, pat):
    arr, view = V.make_view(K, _S(), pat, D.N)
    return arr, K.DeviceDB(view, device=dev)


def _same(got, exp, tag):
    assert got.shape == exp.shape and np.array_equal(got, exp), (tag, V.describe_mismatch(got, exp, D.N))


def _checked_order(K, d, arr, W, short_ids=48):
    got_w, order, live, l, nbits = _order(K, d)
    assert got_w == W
    # all but one node are roots: the layout keeps the pattern order, its list heads are the view's
    assert np.array_equal(l, arr["num_local"].astype(np.uint32)) and np.array_equal(nbits, arr["num_bits"].astype(np.uint32))
    return D.check_order(W, d.P, order, live, l, nbits, short_ids), order, live


def test_the_cases_hold_what_they_say():
    """host: the lists either side of the long test, the keys at the cap, and the contents of the windows"""
    for name, want in (("47 ids 128 bits", (47, 128)), ("47 ids 130 bits", (47, 130)), ("48 ids 127 bits", (48, 127)), ("48 ids 129 bits", (48, 129)),
                       ("run l=48", (48, 47)), ("run l=2", (2, 1)), ("l=49", (49, 48))):
        make = dict(D.SHAPES)[name]
        assert all(D.header(make(i)) == want for i in range(1, 300)), name
    for extra in (58, 60, 62, 64, 66):
        make = dict(D.SHAPES)["extra %d" % extra]
        for i in range(1, 300):
            l, nb = D.header(make(i))
            assert nb - (l - 1) == extra and l <= 48 and nb <= 128 and D.key_of(l, nb) == min(2 + extra, 63)
    assert D.header(D.heavy(5)) == (48, 93) and D.header(D.long_bits(4)) == (46, 129)
    for W in D.WINDOWS:
        pat, names = D.window_forest(W)
        nl = pat["num_local"].numpy()
        assert nl.size == 6 * W + 3 * len(D.SHAPES) + 5 and nl[0] == 0 and (nl[1: 2 * W] == 1).all()
        ids, lp = pat["local_ids"].numpy(), pat["local_ptr"].numpy()
        keys = np.array([D.key_of(*D.header(ids[lp[p]: lp[p + 1]])) if nl[p] else D.key_of(0, 0) for p in range(nl.size)])
        win = lambda name: keys[names[name] * W: (names[name] + 1) * W]      # noqa: E731
        assert (win("singles") == 1).all() and (win("runs") == 2).all() and (win("long") == 0).all()
        assert (win("one") > 0).sum() == 1 and win("one")[77] > 2 and (win("heavy64") > 2).sum() == 64
        assert set(keys[6 * W:]) >= {0, 1, 2, 60, 62, 63}


@pytest.mark.gpu
@pytest.mark.parametrize("W", D.WINDOWS)
def test_node_counts_around_the_window_edges(K, dev, env, W):
    """P = 1, 63 .. 65, 255 .. 257, W - 1 .. W + 1 and 2 W + 5 patterns of mixed lists: the last window is part-filled, the window, workgroup and wave
    edges fall inside data; cold and warm call == the definition, the order holds for every P"""
    for P in D.node_counts(W):
        pat, exp = D.mixed_case(P)
        env(KMDB_K0_WINDOW=W)
        arr, d = _upload(K, dev, pat)
        _checked_order(K, d, arr, W)
        for call in ("cold", "warm"):
            _same(d.all2all_dense(flags=K.capi.FLAG_NO_FALLBACK), exp, "W %d, P %d, %s call" % (W, P, call))
        assert d.stats()["path"] == K.capi.PATH_RECORDS
        d.close()


@pytest.mark.gpu
@pytest.mark.parametrize("width", [None, 32])
@pytest.mark.parametrize("W", D.WINDOWS)
def test_window_contents(K, dev, env, W, width):
    """windows of single ids alone, of runs alone, of long nodes alone (live count 0), of long nodes and one decodable node, of 64 heavy nodes among
    trivial ones, and a part-filled one with the keys at the cap; block width 32 puts one and two block boundaries inside the runs"""
    pat, names, exp = D.window_case(W)
    env(KMDB_K0_WINDOW=W, KMDB_BLOCK_WIDTH=width)
    arr, d = _upload(K, dev, pat)
    keys, order, live = _checked_order(K, d, arr, W)
    assert live[names["singles0"]] == W and live[names["singles"]] == W and live[names["runs"]] == W
    assert live[names["long"]] == 0 and live[names["one"]] == 1 and order[names["one"], 0] == 77
    w = names["heavy64"]
    assert (keys[w, order[w, :64].astype(np.int64)] > 2).all() and (keys[w, order[w, 64:].astype(np.int64)] <= 2).all(), "the heavy nodes share one wave"
    _same(d.all2all_dense(flags=K.capi.FLAG_NO_FALLBACK), exp, "W %d, width %s" % (W, width))
    _same(d.all2all_dense(flags=K.capi.FLAG_NO_FALLBACK), exp, "W %d, width %s, warm call" % (W, width))
    d.close()


@pytest.mark.gpu
@pytest.mark.parametrize("short_ids", [32, 64])
def test_short_ids_rebuild_the_order(K, dev, env, short_ids):
    """KMDB_SHORT_IDS moves the long test: at 32 the lists of 33 .. 48 ids leave the order, at 64 the runs of 49 .. 51 ids join it as single runs"""
    W = 1024
    pat, names, exp = D.window_case(W)
    env(KMDB_K0_WINDOW=W, KMDB_SHORT_IDS=short_ids)
    arr, d = _upload(K, dev, pat)
    keys, order, live = _checked_order(K, d, arr, W, short_ids)
    if short_ids == 64:
        assert live[names["long"]] == W // 2 and (keys[names["long"]] == 2).sum() == W // 2
    else:
        assert 0 < live[names["runs"]] < W
    _same(d.all2all_dense(flags=K.capi.FLAG_NO_FALLBACK), exp, "short ids %d" % short_ids)
    d.close()


@pytest.mark.gpu
@pytest.mark.parametrize("W", D.WINDOWS)
def test_a_handed_over_builder_gets_the_order(K, dev, env, W):
    """kmdb_layout_from_device (Builder.finish_device) makes the order as the upload of the host view does: both handles' matrices == the definition
    of the finished image's forest, the orders have the same keys"""
    names, lists = BC.shape_lists(BC.SHAPES[0])
    env(KMDB_K0_WINDOW=W)
    b1, b2 = K.Builder(BC.SHAPES[0][3], BC.SHAPES[0][4]), K.Builder(BC.SHAPES[0][3], BC.SHAPES[0][4])
    try:
        b1.add_kmers(names, lists)
        b2.add_kmers(names, lists)
        h1 = b1.finish()
        d1 = K.DeviceDB(h1, device=dev)
        d2, h2 = b2.finish_device()
    finally:
        b1.close()
        b2.close()
    exp = V.definition(RC.pat_of_host(h1), d1.N)
    got = []
    for d in (d1, d2):
        got_w, order, live, l, nbits = _order(K, d)
        assert got_w == W
        D.check_order(W, d.P, order, live, l, nbits)
        got.append((live, l, nbits))
        m = d.all2all_dense(flags=K.capi.FLAG_NO_FALLBACK)
        assert np.array_equal(m, exp), V.describe_mismatch(m, exp, d.N)
    assert all(np.array_equal(a, b) for a, b in zip(*got))
    d1.close()
    d2.close()
