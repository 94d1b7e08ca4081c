"""`-sample-rows <criterion>:<count>` with the candidates selected on the device (sample_rows.hip) and decided on the host
(kmdbh_sample_rows_select).  Expected rows never come from the code under test: they are the reference's own goldens
(tests/golden/*.sr_*.ref.txt, written by the reference's Sampler), or the oracle's matrix plus a python restatement of the sampler's total
order (score descending, then sample id ascending; reference src/sampler.h:45-50) over kmdbh_metric, which other tests pin to the reference."""
import ctypes
import importlib
import os

import numpy as np
import pytest

from conftest import ROOT

GOLDENS = [("virus_k18", "sr_jaccard5", "jaccard", 5, ()), ("virus_k18", "sr_numkmers3_min", "num-kmers", 3, (("jaccard", 0.02, None),)),
           ("clade64", "sr_ani7", "ani", 7, ()), ("clade64", "sr_max2", "max", 2, (("num-kmers", 0.0, 3000.0),))]
CRITERIA = ["jaccard", "min", "max", "cosine", "mash", "ani", "ani-shorter", "mash-query", "num-kmers"]
COUNTS = [1, 5, 20, 149, 1000]
# the plain ratio a criterion is monotone in and whether it falls with it: the device's proxy
PROXY = {"jaccard": ("jaccard", 1), "min": ("min", 1), "max": ("max", 1), "cosine": ("cosine", 1), "mash": ("jaccard", -1), "ani": ("jaccard", 1),
         "ani-shorter": ("min", 1), "mash-query": ("query", -1), "num-kmers": ("num", 1)}
FMAX = float(np.finfo(np.float64).max)


@pytest.fixture(scope="module")
def S(K):
    return importlib.import_module("kmerdb_amd.synth")


@pytest.fixture(scope="module")
def dev(K):
    assert K.device_count() > 0, "the -m gpu tests need an MI355X; the engine has no CPU fallback"
    return 0


def golden_rows(golden_dir, stem, tag):
    rows = []
    for ln in open(os.path.join(golden_dir, "%s.%s.ref.txt" % (stem, tag)), "rb").read().split(b"\n")[:-1]:
        rows.append([(int(c.split(b":")[0]) - 1, int(c.split(b":")[1])) for c in ln.split(b",")[:-1]])
    return rows


def rows_of(sp):
    return [list(zip(*(a.tolist() for a in sp.row(i)))) for i in range(sp.n_rows)]


def pairs_of(tri, N):
    """the non-zero cells of the lower triangle: arrays (i, j, c), i > j, in flat order"""
    i = np.repeat(np.arange(N, dtype=np.int64), np.arange(N))
    j = np.concatenate([np.arange(r, dtype=np.int64) for r in range(N)]) if N else np.zeros(0, np.int64)
    nz = np.flatnonzero(tri)
    return i[nz], j[nz], tri[nz].astype(np.int64)


def metric_of(K, name, c, a, b, k):
    L = K.lib()
    m = K.capi.METRICS.index(name)
    return np.array([L.kmdbh_metric(m, int(x), int(y), int(z), int(k)) for x, y, z in zip(c, a, b)], dtype=np.float64)


def passing(K, i, j, c, kmers, k, filters):
    ok = np.ones(len(c), bool)
    for name, lo, hi in filters:
        x = metric_of(K, name, c, kmers[i], kmers[j], k)
        ok &= (x >= (-FMAX if lo is None else lo)) & (x <= (FMAX if hi is None else hi))
    return ok


def expected_rows(K, tri, N, kmers, k, criterion, count, filters=()):
    """the sampler's rows from the full matrix: every passing pair offered to both its samples with one score (the triangle's row sample first),
    the `count` best by (score descending, id ascending), written in ascending id.  A NaN score ranks below every number and among NaN scores
    the smaller id wins: host_sampler.cpp's own rule (the reference's comparison is no order there)"""
    i, j, c = pairs_of(tri, N)
    ok = passing(K, i, j, c, kmers, k, filters)
    i, j, c = i[ok], j[ok], c[ok]
    sc = metric_of(K, criterion, c, kmers[i], kmers[j], k)
    per = [[] for _ in range(N)]
    for a, b, v, s in zip(i.tolist(), j.tolist(), c.tolist(), sc.tolist()):
        nan = s != s
        per[a].append((nan, 0.0 if nan else -s, b, v))
        per[b].append((nan, 0.0 if nan else -s, a, v))
    return [sorted((o, v) for _, _, o, v in sorted(r)[:count]) for r in per]


def full_part(tri, N):
    """the whole matrix as one candidate part: symmetric rows in ascending columns"""
    i, j, c = pairs_of(tri, N)
    s = np.concatenate([i, j]); o = np.concatenate([j, i]); v = np.concatenate([c, c])
    order = np.lexsort((o, s))
    ptr = np.zeros(N + 1, np.uint64)
    ptr[1:] = np.cumsum(np.bincount(s, minlength=N))
    return ptr, o[order].astype(np.uint32), v[order].astype(np.uint32)


def proxy_of(criterion, c, a, b):
    """the device's proxy of a cell with row-sample count a and column-sample count b (uint32 integer parts, as in kmdbh_metric)"""
    kind, sign = PROXY[criterion]
    c, a, b = c.astype(np.uint32), a.astype(np.uint32), b.astype(np.uint32)
    with np.errstate(all="ignore"):
        d = {"jaccard": (a + b - c).astype(np.float64), "min": np.minimum(a, b).astype(np.float64), "max": np.maximum(a, b).astype(np.float64),
             "cosine": np.sqrt((a * b).astype(np.float64)), "query": a.astype(np.float64), "num": np.ones(len(c))}[kind]
        return sign * c.astype(np.float64) / d


def model_candidates(K, tri, N, kmers, k, criterion, count, filters=(), widen=1e-6, band=1e-6, refetch=True):
    """numpy model of the device's candidate rule and of the completeness rule: cells that pass the WIDENED filters; per sample T_s = the count-th
    largest proxy; emitted: proxy >= T_s - |T_s| band.  A row with a T_s in which fewer than `count` candidates at or above T_s pass the exact
    filters is fetched again whole.  Returns (part, rows truncated, rows fetched again)."""
    i, j, c = pairs_of(tri, N)
    wide = np.ones(len(c), bool)
    for name, lo, hi in filters:
        assert name == "jaccard"                                  # (the model widens the one bound the tests use)
        x = proxy_of("jaccard", c, kmers[i], kmers[j])
        lo = -np.inf if lo is None else lo - abs(lo) * widen - 1e-300
        hi = np.inf if hi is None else hi + abs(hi) * widen + 1e-300
        wide &= (x >= lo) & (x <= hi)
    i, j, c = i[wide], j[wide], c[wide]
    exact = passing(K, i, j, c, kmers, k, filters)
    p = proxy_of(criterion, c, kmers[i], kmers[j])
    s = np.concatenate([i, j]); o = np.concatenate([j, i]); v = np.concatenate([c, c]); p2 = np.concatenate([p, p]); e2 = np.concatenate([exact, exact])
    keep = np.zeros(len(s), bool)
    truncated = again = 0
    for r in range(N):
        idx = np.flatnonzero(s == r)
        if len(idx) < count:
            keep[idx] = True
            continue
        T = np.sort(p2[idx])[::-1][count - 1]
        em = idx[p2[idx] >= T - abs(T) * band]
        truncated += len(em) < len(idx)                           # (a row of `count` cells or more has a T_s; truncated: something lies below the cut)
        if refetch and np.count_nonzero(e2[em] & (p2[em] >= T)) < count:
            em = idx
            again += 1
        keep[em] = True
    s, o, v = s[keep], o[keep], v[keep]
    order = np.lexsort((o, s))
    ptr = np.zeros(N + 1, np.uint64)
    ptr[1:] = np.cumsum(np.bincount(s, minlength=N))
    return (ptr, o[order].astype(np.uint32), v[order].astype(np.uint32)), truncated, again


def split_parts(part, N, cuts, rng):
    """the entries of a part dealt to len(cuts) + 1 parts at entry boundaries `cuts`, shuffled inside every row of every part"""
    ptr, col, val = part
    row = np.repeat(np.arange(N), np.diff(ptr).astype(np.int64))
    out = []
    for a, b in zip([0] + list(cuts), list(cuts) + [len(col)]):
        r, c, v = row[a:b], col[a:b], val[a:b]
        perm = rng.permutation(len(r))
        perm = perm[np.argsort(r[perm], kind="stable")]
        p = np.zeros(N + 1, np.uint64)
        p[1:] = np.cumsum(np.bincount(r, minlength=N))
        out.append((p, c[perm], v[perm]))
    return out


@pytest.fixture(scope="module")
def golden_db(K, O, golden_dir):
    """per golden database: (path, N, k, sample k-mer counts, the oracle's matrix)"""
    out = {}
    for stem in ("virus_k18", "clade64"):
        path = os.path.join(golden_dir, stem + ".db")
        h = K.HostDB(path, skip_hashtables=True)
        out[stem] = (path, h.N, h.k, h.sample_kmers.astype(np.int64), O.OracleDB(path, skip_hashtables=True).all2all_dense().copy())
    return out


@pytest.fixture(scope="module")
def synth150(K, O, S, tmp_path_factory):
    """S.synth_database(150, 10, 4000, k=18, seed=5): three block rows at any width <= 64, every pair non-zero; every sample has the same true
    k-mer count, so the tests pass their own counts (true + i * 37 % 1000) to pull the ratios away from the order of the cells"""
    N, k = 150, 18
    g, pat = S.synth_database(N, 10, 4000, k=k, seed=5)
    arr = S.to_view_arrays(pat)
    path = str(tmp_path_factory.mktemp("sr") / "s150.db")
    S.write_db(path, k, 1.0, [g.name(i) for i in range(N)], pat["sample_counts"], arr)
    tri = O.OracleDB(path, skip_hashtables=True).all2all_dense().copy()
    assert np.count_nonzero(tri) == N * (N - 1) // 2
    kmers = np.asarray(pat["sample_counts"], dtype=np.int64) + np.arange(N) * 37 % 1000
    view = K.make_view(k, N, arr["num_kmers"], arr["parent_id"], arr["num_samples"], arr["num_local"], arr["last_sample_id"], arr["num_bits"],
                       arr["data_offset"], arr["data"])
    return dict(N=N, k=k, tri=tri, kmers=kmers, view=view, path=path, expected={})


def synth_expected(K, d, criterion, count, filters=()):
    key = (criterion, count, tuple(filters))
    if key not in d["expected"]:
        d["expected"][key] = expected_rows(K, d["tri"], d["N"], d["kmers"], d["k"], criterion, count, filters)
    return d["expected"][key]


# ---- CPU ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stem,tag,criterion,count,filters", GOLDENS)
def test_select_reproduces_the_goldens(K, golden_dir, golden_db, stem, tag, criterion, count, filters):
    """1. the oracle's full matrix as ONE candidate part -> the rows the reference's own Sampler wrote"""
    _, N, k, kmers, tri = golden_db[stem]
    want = golden_rows(golden_dir, stem, tag)
    got = K.sample_rows_select(criterion, count, k, kmers, [full_part(tri, N)], filters)
    assert rows_of(got) == want
    # (the python restatement the other tests expect from agrees with the reference's goldens too)
    assert expected_rows(K, tri, N, kmers, k, criterion, count, filters) == want
    # measure = the score of the kept cell, the triangle's row sample first
    for s in range(N):
        for (o, v), m in zip(want[s], got.measure[int(got.row_ptr[s]):int(got.row_ptr[s + 1])]):
            assert m == K.lib().kmdbh_metric(K.capi.METRICS.index(criterion), v, int(kmers[max(s, o)]), int(kmers[min(s, o)]), k)


@pytest.mark.parametrize("stem,tag,criterion,count,filters", GOLDENS)
def test_select_does_not_depend_on_parts_or_order(K, golden_dir, golden_db, stem, tag, criterion, count, filters):
    """2. the same candidates cut into 3 parts at arbitrary entry boundaries (rows cut mid-way), shuffled inside the parts"""
    _, N, k, kmers, tri = golden_db[stem]
    part = full_part(tri, N)
    n = len(part[1])
    parts = split_parts(part, N, [n // 3 + 1, 2 * n // 3 + 7], np.random.default_rng(7))
    assert all(len(p[1]) for p in parts)
    assert rows_of(K.sample_rows_select(criterion, count, k, kmers, parts, filters)) == golden_rows(golden_dir, stem, tag)
    # an empty part among them, and a pair listed by two parts, change nothing
    empty = (np.zeros(N + 1, np.uint64), np.zeros(0, np.uint32), np.zeros(0, np.uint32))
    assert rows_of(K.sample_rows_select(criterion, count, k, kmers, parts + [empty, parts[0]], filters)) == golden_rows(golden_dir, stem, tag)


def test_select_on_the_candidates_of_the_device_rule(K, synth150):
    """3. a numpy model of the device's candidate rule (proxy, T_s, margin band, re-fetch) on the oracle's matrix, then select: the rows of the
    full matrix — far fewer candidates than cells, every criterion, and a filter bound that sits inside the margin of a row's best cell"""
    d = synth150
    N, k, tri, kmers = d["N"], d["k"], d["tri"], d["kmers"]
    for criterion in CRITERIA:
        part, truncated, again = model_candidates(K, tri, N, kmers, k, criterion, 5)
        assert truncated == N and again == 0 and len(part[1]) < 8 * N
        assert rows_of(K.sample_rows_select(criterion, 5, k, kmers, [part])) == synth_expected(K, d, criterion, 5)
    # a bound one ulp above the jaccard of a row's best cell: the cell passes the widened bound and fails the exact one
    flt = refetch_filter(K, d)
    part, truncated, again = model_candidates(K, tri, N, kmers, k, "jaccard", 5, flt)
    assert again >= 1
    assert rows_of(K.sample_rows_select("jaccard", 5, k, kmers, [part], flt)) == synth_expected(K, d, "jaccard", 5, flt)
    # and a case in which the re-fetch is NEEDED: ranked by num-kmers, bounded by jaccard — a cell among a row's best 3 fails the exact bound,
    # and the cell that takes its place was held back by the device
    criterion, count, flt = needed_refetch_case(K, d)
    want = synth_expected(K, d, criterion, count, flt)
    part, truncated, again = model_candidates(K, tri, N, kmers, k, criterion, count, flt)
    assert again >= 1 and rows_of(K.sample_rows_select(criterion, count, k, kmers, [part], flt)) == want
    cut, _, _ = model_candidates(K, tri, N, kmers, k, criterion, count, flt, widen=1e-6, band=1e-6, refetch=False)
    assert rows_of(K.sample_rows_select(criterion, count, k, kmers, [cut], flt)) != want


def score(K, d, name, s, o, v):
    return K.lib().kmdbh_metric(K.capi.METRICS.index(name), int(v), int(d["kmers"][max(s, o)]), int(d["kmers"][min(s, o)]), d["k"])


def refetch_filter(K, d, count=5):
    """-min jaccard one ulp above the score of some row's best cell: the first row r whose best cell (r, o) is exactly the count-th best of row o,
    so that row o has a T_s — that cell's proxy — and only count - 1 candidates that pass the exact bound"""
    ranked = [[o for _, o, _ in sorted((-score(K, d, "jaccard", s, o, v), o, v) for o, v in row)] for s, row in enumerate(synth_expected(K, d, "jaccard", d["N"]))]
    for r in range(d["N"]):
        o = ranked[r][0]
        if ranked[o].index(r) == count - 1:
            v = dict(synth_expected(K, d, "jaccard", d["N"])[r])[o]
            return (("jaccard", float(np.nextafter(score(K, d, "jaccard", r, o, v), 2.0)), None),)
    raise AssertionError("no row's best cell is the count-th best of its partner's row")


def needed_refetch_case(K, d, count=3):
    """("num-kmers", count, -min jaccard bound): a row s and a cell X of it such that at least `count` cells of the row have a larger jaccard
    than X and X has more common k-mers than the count-th of them: with the bound one ulp above X's jaccard, X is among the device's best
    `count` of the row, fails the exact bound, and the row's true count-th cell lies below the device's cut"""
    rows = synth_expected(K, d, "jaccard", d["N"])
    for s, row in enumerate(rows):
        js = sorted(((score(K, d, "jaccard", s, o, v), v, o) for o, v in row), reverse=True)
        for n in range(count, len(js)):
            above = sorted((v for _, v, _ in js[:n]), reverse=True)
            if js[n][0] < js[n - 1][0] and js[n][1] > above[count - 1] * (1 + 1e-5) and js[n][0] > 0.2:
                return "num-kmers", count, (("jaccard", float(np.nextafter(js[n][0], 2.0)), None),)
    raise AssertionError("no such row")


def test_select_refuses_bad_arguments(K):
    """11 (host half). count 0, unknown criteria, no k-mer counts: return code and message, inside the C boundary"""
    part = (np.zeros(3, np.uint64), np.zeros(0, np.uint32), np.zeros(0, np.uint32))
    kmers = np.array([5, 6], np.uint32)
    with pytest.raises(K.KmdbError, match="kmdbh_sample_rows_select: count must be at least 1"):
        K.sample_rows_select("jaccard", 0, 18, kmers, [part])
    for bad in (K.capi.METRICS.__len__(), -1, 77):
        with pytest.raises(K.KmdbError, match="kmdbh_sample_rows_select: unknown criterion"):
            K.sample_rows_select(bad, 3, 18, kmers, [part])
    with pytest.raises(K.KmdbError, match="kmdbh_sample_rows_select: sample_kmers is NULL"):
        K.sample_rows_select("jaccard", 3, 18, None, [part])
    assert K.sample_rows_select("jaccard", 3, 18, kmers, [part]).nnz == 0


def test_header_declares_the_sampled_entry_points(K):
    hdr = open(os.path.join(ROOT, "include", "kmdb_amd.h")).read()
    L = ctypes.CDLL(K.lib_path())
    for name in ("kmdb_all2all_sampled", "kmdb_sampled_from_dense_device", "kmdb_node_all2all_sampled", "kmdb_db_sample_stats", "kmdbh_sample_rows_select"):
        assert name in K.capi.EXPORTS and name + "(" in hdr and hasattr(L, name), name
    assert ctypes.sizeof(K.capi._SampleStats) == 48 and "} kmdb_sample_stats;" in hdr


# ---- GPU ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("stem,tag,criterion,count,filters", GOLDENS)
def test_goldens_through_the_api(K, golden_dir, golden_db, dev, stem, tag, criterion, count, filters):
    """4. DeviceDB.all2all_sampled against the reference's own sampled rows"""
    path, N, k, kmers, _ = golden_db[stem]
    db = K.DeviceDB(K.HostDB(path, skip_hashtables=True), device=dev)
    got = db.all2all_sampled(criterion, count, kmers, filters)
    assert rows_of(got) == golden_rows(golden_dir, stem, tag)
    st = db.sample_stats()
    assert st["candidates"] >= got.nnz and st["triangle_reads"] >= 6 and st["select_ms"] > 0
    db.close()


@pytest.fixture(scope="module")
def synth150_dev(K, synth150, dev):
    db = K.DeviceDB(synth150["view"], device=dev)
    yield db
    db.close()


@pytest.mark.gpu
@pytest.mark.parametrize("criterion", CRITERIA)
def test_synthetic_all_criteria(K, synth150, synth150_dev, criterion):
    """5. + 9.: 150 samples, every pair non-zero, the test's own k-mer counts; counts 1 / 5 / 20 truncate every row (ties across the cut are broken
    by id), 149 and 1000 leave every row whole.  The candidates stay within `count` plus the cells within 1e-5 (relative) of the row's count-th
    best proxy, and what is copied back within 16 bytes per candidate plus the row pointers."""
    d, db = synth150, synth150_dev
    N, k, tri, kmers = d["N"], d["k"], d["tri"], d["kmers"]
    i, j, c = pairs_of(tri, N)
    p = proxy_of(criterion, c, kmers[i], kmers[j])
    P = np.full((N, N), -np.inf)
    P[i, j] = p
    P[j, i] = p
    for count in COUNTS:
        got = db.all2all_sampled(criterion, count, kmers)
        assert rows_of(got) == synth_expected(K, d, criterion, count), (criterion, count)
        st = db.sample_stats()
        assert st["rows_refetched"] == 0
        assert st["rows_truncated"] == (N if count < N - 1 else 0)
        assert st["d2h_bytes"] <= 16 * st["candidates"] + 8 * (N + 1)
        if count >= N - 1:
            assert st["candidates"] == N * (N - 1)
            continue
        # per row, from the candidates themselves (the whole triangle as a flat range: a matrix the caller accumulated)
        import torch
        cells = torch.from_numpy(tri.astype(np.int32)).cuda()
        cand = db.sampled_from_dense_device(cells.data_ptr(), criterion, count, kmers)
        assert cand.measure is None and cand.nnz == db.sample_stats()["candidates"] == st["candidates"]
        for s in range(N):
            row = np.sort(P[s][np.isfinite(P[s])])[::-1]
            T = row[count - 1]
            cols, vals = cand.row(s)
            assert cols.tolist() == sorted(cols.tolist()) and np.array_equal(vals, tri[np.maximum(cols, s) * (np.maximum(cols, s) - 1) // 2 + np.minimum(cols, s)])
            assert count <= len(cols) <= count + np.count_nonzero(np.abs(row - T) <= 1e-5 * abs(T)), (criterion, count, s)
            assert set(o for o, _ in synth_expected(K, d, criterion, count)[s]) <= set(cols.tolist())


@pytest.mark.gpu
def test_filter_inside_the_margin_is_fetched_again(K, synth150, synth150_dev):
    """6. jaccard:5 with -min jaccard one ulp above the score of row 77's best cell: the cell passes the widened bound on the device and fails
    the exact one on the host, so a row is fetched again; a bound far from every cell needs none"""
    d, db = synth150, synth150_dev
    flt = refetch_filter(K, d)
    got = db.all2all_sampled("jaccard", 5, d["kmers"], flt)
    assert rows_of(got) == synth_expected(K, d, "jaccard", 5, flt)
    st = db.sample_stats()
    assert st["rows_refetched"] >= 1 and st["triangle_reads"] == 8
    # ranked by num-kmers, bounded by jaccard: here the cell that replaces the failing one was held back by the device
    criterion, count, flt3 = needed_refetch_case(K, d)
    assert rows_of(db.all2all_sampled(criterion, count, d["kmers"], flt3)) == synth_expected(K, d, criterion, count, flt3)
    assert db.sample_stats()["rows_refetched"] >= 1
    i, j, c = pairs_of(d["tri"], d["N"])
    sc = metric_of(K, "jaccard", c, d["kmers"][i], d["kmers"][j], d["k"])
    u = np.unique(sc)
    g = int(np.argmax(np.diff(u) / u[1:]))
    far = float((u[g] + u[g + 1]) / 2)                             # the middle of the widest gap between two cells' scores
    assert np.min(np.abs(sc - far) / far) > 1e-5 and np.count_nonzero(sc >= far) > 5 * d["N"] // 2
    flt2 = (("jaccard", far, None),)
    got = db.all2all_sampled("jaccard", 5, d["kmers"], flt2)
    assert rows_of(got) == synth_expected(K, d, "jaccard", 5, flt2)
    assert db.sample_stats()["rows_refetched"] == 0


@pytest.mark.gpu
def test_mostly_untouched_tiles(K, O, S, dev, tmp_path, monkeypatch):
    """7. clades from independent roots (the c4sparse workload's model): only the blocks on the diagonal are non-zero, so most tiles were never
    touched and are not read; rows with fewer than `count` neighbours and rows with none; the same with every tile read"""
    N, cs, k = 301, 6, 25
    g, pat = S.synth_database(N, cs, 3000, k=k, seed=41, r1=0.75)
    arr = S.to_view_arrays(pat)
    path = str(tmp_path / "sparse.db")
    S.write_db(path, k, 1.0, [g.name(i) for i in range(N)], pat["sample_counts"], arr)
    tri = O.OracleDB(path, skip_hashtables=True).all2all_dense().copy()
    kmers = np.asarray(pat["sample_counts"], dtype=np.int64)
    nb = np.zeros(N, np.int64)
    i, j, _ = pairs_of(tri, N)
    np.add.at(nb, i, 1)
    np.add.at(nb, j, 1)
    assert (nb == 0).any() and (nb == cs - 1).any() and np.count_nonzero(tri) < 4 * N
    view = K.make_view(k, N, arr["num_kmers"], arr["parent_id"], arr["num_samples"], arr["num_local"], arr["last_sample_id"], arr["num_bits"],
                       arr["data_offset"], arr["data"])
    db = K.DeviceDB(view, device=dev)
    for criterion, count in (("jaccard", 3), ("mash", 8), ("num-kmers", 5)):
        want = expected_rows(K, tri, N, kmers, k, criterion, count)
        assert any(len(r) == 0 for r in want) and (count <= cs - 1 or any(0 < len(r) < count for r in want))
        monkeypatch.delenv("KMDB_SP_ALL_TILES", raising=False)
        got = db.all2all_sampled(criterion, count, kmers)
        assert db.stats()["path"] == K.capi.PATH_RECORDS
        assert rows_of(got) == want
        st = db.sample_stats()
        monkeypatch.setenv("KMDB_SP_ALL_TILES", "1")
        assert rows_of(db.all2all_sampled(criterion, count, kmers)) == want
        assert db.sample_stats()["candidates"] == st["candidates"] and db.sample_stats()["rows_truncated"] == st["rows_truncated"]
    db.close()


@pytest.mark.gpu
def test_flat_ranges_and_node(K, golden_dir, golden_db, synth150, synth150_dev, dev):
    """8. three uneven flat ranges that cut rows mid-way, merged by select = the one-call result; a node of 3 shards on one device under every
    partition = the same rows"""
    import torch
    d, db = synth150, synth150_dev
    N, k, tri, kmers = d["N"], d["k"], d["tri"], d["kmers"]
    cells = torch.from_numpy(tri.astype(np.int32)).cuda()
    cuts = [0, 1234, 7001, len(tri)]
    assert all(any(r * (r - 1) // 2 < c < r * (r + 1) // 2 for r in range(N)) for c in cuts[1:-1])
    for criterion, count in (("jaccard", 5), ("mash-query", 20), ("num-kmers", 1)):
        parts = [db.sampled_from_dense_device(cells.data_ptr() + 4 * lo, criterion, count, kmers, cell_lo=lo, cell_hi=hi) for lo, hi in zip(cuts, cuts[1:])]
        assert all(p.nnz for p in parts)
        merged = K.sample_rows_select(criterion, count, k, kmers, parts)
        assert rows_of(merged) == synth_expected(K, d, criterion, count) == rows_of(db.all2all_sampled(criterion, count, kmers))
    path, N, k, kmers, _ = golden_db["virus_k18"]
    h = K.HostDB(path)
    for partition in K.capi.PARTITIONS:
        nd = K.NodeDB(h, 3, (dev,), partition=partition)
        for stem, tag, criterion, count, filters in GOLDENS[:2]:
            assert rows_of(nd.all2all_sampled(criterion, count, kmers, filters)) == golden_rows(golden_dir, stem, tag), (partition, tag)
        nd.close()


@pytest.mark.gpu
def test_front_end(K, golden_dir, dev, tmp_path):
    """10. all2all-sp -gpus 3 -sample-rows, with both partitions, writes the golden rows; all2all-parts -sample-rows jaccard:1 (the host sampler,
    pruned at 2 x count items per row) writes the rows of all2all-sp over the whole collection"""
    from test_gpu_parity import _cli
    g = lambda n: os.path.join(golden_dir, n)   # noqa: E731
    t = lambda n: str(tmp_path / n)             # noqa: E731

    def rows(csv):
        return [b",".join(ln.split(b",")[2:]) for ln in open(csv, "rb").read().split(b"\n")[2:] if ln]

    want = open(g("virus_k18.sr_jaccard5.ref.txt"), "rb").read().split(b"\n")[:-1]
    for extra in ([], ["-gpus", "3"], ["-gpus", "3", "-partition", "range"]):
        _cli("all2all-sp", *extra, "-sample-rows", "jaccard:5", g("virus_k18.db"), t("sr.csv"))
        assert rows(t("sr.csv")) == want, extra
    with open(t("db.list"), "w") as f:
        f.write(g("virus_k18_part1.db") + "\n" + g("virus_k18_part2.db") + "\n")
    _cli("all2all-sp", "-sample-rows", "jaccard:1", g("virus_k18.db"), t("one.csv"))
    for extra in ([], ["-gpus", "2"]):
        _cli("all2all-parts", "-sample-rows", "jaccard:1", *extra, t("db.list"), t("parts.csv"))
        assert rows(t("parts.csv")) == rows(t("one.csv")) and any(rows(t("one.csv")))


@pytest.mark.gpu
def test_argument_errors(K, golden_db, dev):
    """11. count 0, unknown criteria (KMDB_METRIC_COUNT and negative values among them), no k-mer counts: refused with a message, by every entry"""
    path, N, k, kmers, tri = golden_db["clade64"]
    h = K.HostDB(path)
    db = K.DeviceDB(h, device=dev)
    nd = K.NodeDB(h, 1, (dev,))
    import torch
    cells = torch.from_numpy(tri.astype(np.int32)).cuda()
    calls = {"kmdb_all2all_sampled": lambda c, n, km: db.all2all_sampled(c, n, km),
             "kmdb_sampled_from_dense_device": lambda c, n, km: db.sampled_from_dense_device(cells.data_ptr(), c, n, km),
             "kmdb_node_all2all_sampled": lambda c, n, km: nd.all2all_sampled(c, n, km)}
    for who, call in calls.items():
        with pytest.raises(K.KmdbError, match=who + ": count must be at least 1"):
            call("jaccard", 0, kmers)
        for bad in (len(K.capi.METRICS), -1, 1 << 20):
            with pytest.raises(K.KmdbError, match=who + ": unknown criterion"):
                call(bad, 3, kmers)
        with pytest.raises(K.KmdbError, match=who + ": sample_kmers is NULL"):
            call("jaccard", 3, None)
    with pytest.raises(K.KmdbError, match="kmdb_all2all_sampled: the selection needs the whole database"):
        db.all2all_sampled("jaccard", 3, kmers, shard=(0, 2))
    # the handles are as usable as before
    assert db.all2all_sampled("jaccard", 3, kmers).nnz > 0 and nd.all2all_sampled("jaccard", 3, kmers).nnz > 0
    nd.close()
    db.close()
