#!/usr/bin/env python3
"""Fixture for the db2db restatement: the REAL reference's db2db_sp + compact2 (oracle/_ref/ref_driver db2db_sp) of
virus_k18_part2.db (rows) against virus_k18_part1.db (columns), written as virus_k18_part2_x_part1.db2db_sp.ref.txt.
Run where the reference is built (make -C oracle): python tests/golden/make_fixture_db2db.py"""
import lzma
import os
import shutil
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from oracle import oracle as O      # noqa: E402

assert O.have_ref(), "build oracle/_ref first (make -C oracle)"
td = tempfile.mkdtemp()
try:
    paths = []
    for stem in ("virus_k18_part2", "virus_k18_part1"):
        paths.append(os.path.join(td, stem + ".db"))
        with lzma.open(os.path.join(HERE, stem + ".db.xz")) as f, open(paths[-1], "wb") as o:
            o.write(f.read())
    txt, _ = O.ref_db2db_sp(paths[0], paths[1], os.path.join(td, "o.txt"), threads=2)
finally:
    shutil.rmtree(td)
out = os.path.join(HERE, "virus_k18_part2_x_part1.db2db_sp.ref.txt")
with open(out, "wb") as f:
    f.write(txt)
print(os.path.basename(out), len(txt), "bytes")
