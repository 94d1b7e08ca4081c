"""What the three sources of cells that lie in HBM share on the host side of csrc/distance.hip (kmdb_distance_matrix_rows, kmdb_distance_query_rows,
kmdb_distance_csr_rows): where a table is cut into pieces changes no byte of it, and the handle's statistics are the same function of the input
for every source.  The standard is the host loop's bytes (the row rules restated in tests/distance_cases.py), never the code under test; the
tables hold no cell the device leaves to the host, which test_the_tables_are_what_they_are_named_for decides on the CPU."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import distance_cases as DC
import distance_parts_cases as PC
import distance_pieces_cases as XC
import distance_query_cases as QC
from conftest import ROOT

EXE = os.path.join(ROOT, "kmer-db_amd", "bin", "kmer-db-amd")
FORMS = QC.FORMS


@pytest.fixture(scope="module")
def L(K):
    lib = K.capi.lib()
    lib.kmdbh_metric.restype = ctypes.c_double
    return lib


@pytest.fixture(scope="module")
def tables():
    return {"triangle": XC.triangle(), "rows": XC.rectangle(), "csr": XC.csr(), "csr-empty": XC.csr_without_entries()}


# ---- no device -------------------------------------------------------------------------------------------------------------------------------
def test_the_tables_are_what_they_are_named_for(L, tables):
    assert XC.CUTS == [(0, 1), (1, 256), (5, 5), (256, 257), (257, 258)]
    t = tables["triangle"]
    assert t["n"] == 258 and t["tri"].size == 258 * 257 // 2 and t["counts"].min() > 0
    q = tables["rows"]
    assert (q["nq"], q["n"]) == (258, 3) and q["counts"].min() > 0 and q["query_counts"].min() > 0
    c = tables["csr"]
    lengths = np.diff(c["ptr"].astype(np.int64))
    assert (c["nr"], c["n"]) == (258, 300) and [int(lengths[r]) for r in XC.CSR_EMPTY_ROWS] == [0, 0, 0, 0] and lengths[XC.CSR_LONG_ROW] == 257 == lengths.max()
    assert int((c["val"] == 0).sum()) == 1 and c["counts"].min() > 0
    e = tables["csr-empty"]
    assert e["nr"] == 258 and e["ptr"][-1] == 0 and e["text"].count(b"\n") == 258 and b":" not in e["text"]
    for measure in XC.MEASURES:
        assert XC.margin_hits(L, measure, XC.K_TRI, XC.triangle_triples(t)) == [], measure
        assert XC.margin_hits(L, measure, QC.K_LEN, XC.rectangle_triples(q)) == [], measure
        assert XC.margin_hits(L, measure, PC.K_LEN, XC.csr_triples(c)) == [], measure


# ---- the library -------------------------------------------------------------------------------------------------------------------------------
def to_device(a, dtype=np.uint32):
    import torch
    a = np.ascontiguousarray(a, dtype)
    return torch.from_numpy(a.view(np.int64 if dtype == np.uint64 else np.int32)).cuda() if a.size else None


class Source:
    """One table in HBM behind a handle: what the test needs of a source, whichever it is."""

    def __init__(self, K, L, kind, t, measure, form):
        self.t, self.kind = t, kind
        if kind == "triangle":
            self.keep = [to_device(t["tri"])]
            self.d = K.Distance(measure, XC.K_TRI, t["counts"], triangle=True, **FORMS[form][0])
            self.d.take_cells(self.keep[0].data_ptr(), 0, t["names"])
            self.pieces, self.bytes_per_cell = self.d.matrix_rows, 4
            self.want = DC.Rules(L, measure, XC.K_TRI, t["counts"], triangle=True, cache=t["cache"], **FORMS[form][1]).rows(t["text"])
            self.first_cell = [r * (r - 1) // 2 if r else 0 for r in range(XC.ROWS + 1)]
        elif kind == "rows":
            self.keep = [to_device(t["flat"])]
            self.d = K.Distance(measure, QC.K_LEN, t["counts"], **FORMS[form][0])
            self.d.take_rows(self.keep[0].data_ptr(), t["nq"], t["query_counts"], t["names"])
            self.pieces, self.bytes_per_cell = self.d.query_rows, 4
            self.want = QC.witness(L, t, measure, form)
            self.first_cell = [r * t["n"] for r in range(XC.ROWS + 1)]
        else:
            assert form == "sparse"
            self.keep = [to_device(t["ptr"], np.uint64), to_device(t["col"]), to_device(t["val"])]
            self.d = K.Distance(measure, PC.K_LEN, t["counts"], sparse_out=True)
            self.d.take_csr(*[x.data_ptr() if x is not None else None for x in self.keep], t["nr"], t["row_counts"], t["row_names"])
            self.pieces, self.bytes_per_cell = self.d.csr_rows, 8
            self.want = PC.witness(L, t, measure)
            self.first_cell = [int(x) for x in t["ptr"]]

    def close(self):
        self.d.close()
        self.keep = None


CASES = [(kind, form) for kind in ("triangle", "rows") for form in sorted(FORMS)] + [("csr", "sparse"), ("csr-empty", "sparse")]


@pytest.mark.gpu
@pytest.mark.parametrize("measure", XC.MEASURES)
@pytest.mark.parametrize("kind,form", CASES, ids=["%s-%s" % c for c in CASES])
def test_cuts_change_no_byte_and_the_statistics_follow_the_input(K, L, tables, kind, form, measure):
    t = tables[kind]
    whole = Source(K, L, kind, t, measure, form)
    assert whole.pieces(0, XC.ROWS) == whole.want                  # the standard: the host loop's bytes
    whole.close()
    s = Source(K, L, kind, t, measure, form)
    texts = [s.pieces(lo, hi) for lo, hi in XC.CUTS]
    assert texts[XC.CUTS.index((5, 5))] == b"" and b"".join(texts) == s.want
    cells = sum(s.first_cell[hi] - s.first_cell[lo] for lo, hi in XC.CUTS)
    assert cells == s.first_cell[XC.ROWS] and (cells == 0) == (kind == "csr-empty")
    st = s.d.stats()
    assert st["calls"] == len(XC.CUTS) and st["rows"] == XC.ROWS and st["cells_read"] == cells and st["bytes_in"] == s.bytes_per_cell * cells, st
    assert st["bytes_out"] == sum(len(x) for x in texts) and st["host_cells"] == 0, st
    if kind.startswith("csr"):
        assert s.d.parts_stats()["cells_written"] == int((t["val"] > 0).sum()) == s.want.count(b":"), s.d.parts_stats()
    s.close()


# ---- the front-end's budget of cells, at both ends of its range ------------------------------------------------------------------------------------
@pytest.mark.gpu                                                    # (the front-end's -distance forms have no host path: the table comes from the device)
@pytest.mark.parametrize("budget,one_call", [("0", False), (str((1 << 31) + 12345), True), (str(1 << 40), True)], ids=["zero", "above-2^31", "2^40"])
def test_cli_the_budget_of_cells_is_clamped(golden_dir, tmp_path, budget, one_call):
    """KMDB_DISTANCE_CELLS_PER_PIECE below 1 is 1 (a row a piece, and what fits next to row 0), above 2^31 - 1 is 2^31 - 1 (the library refuses a
    piece of 2^31 cells): both are accepted and write the golden bytes"""
    out = tmp_path / "out"
    r = subprocess.run([EXE, "all2all", "-distance", "mash", os.path.join(golden_dir, "synth_k21.db"), str(out)], capture_output=True, text=True,
                       env=dict(os.environ, KMDB_VERBOSE="1", KMDB_DISTANCE_CELLS_PER_PIECE=budget))
    assert r.returncode == 0, r.stderr
    assert out.read_bytes() == open(os.path.join(golden_dir, "synth.a2a.mash"), "rb").read()
    m = re.search(r"distance from the matrix: calls (\d+), rows (\d+), cells read (\d+)", r.stderr)
    assert m and int(m.group(2)) == 5 and int(m.group(3)) == 10 and (int(m.group(1)) == 1) == one_call and 1 <= int(m.group(1)) <= 5, r.stderr
