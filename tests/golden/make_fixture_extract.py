#!/usr/bin/env python3
"""Fixtures of tests/test_loader_conformance.py.  Run in the build container (needs the reference's sources and oracle/_ref, `make -C oracle`):
python tests/golden/make_fixture_extract.py

  loader_extract.npz ............. the texts of tests/loader_cases.py and, for every (alphabet, k, hash window), the words the reference's OWN
                                   KmerHelper::extract (oracle/_ref/ref_extract) gives for them, in extraction order; the thresholds its
                                   MinHashFilter held for every window (a window that ends at 1 has the upper threshold 0 under the reference's
                                   build flags: it keeps nothing — recorded here)
  loader_<alphabet>_k<k>.db.xz ... three protein databases for the device loader at widenings 10, 4 and 0: the records of
                                   loader_cases.protein_records() as samples, k-mers by ref_extract, built by the real reference
                                   (ref_driver build -> PrefixKmerDb::addKmers + serialize)
Everything written is DATA (inputs and recorded outputs)."""
import lzma
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import loader_cases as LC           # noqa: E402
import make_fixtures as MF          # noqa: E402
from oracle import oracle as O      # noqa: E402

assert O.have_ref() and O.have_ref_extract(), "build oracle/_ref first (make -C oracle)"
arrays = LC.build_fixture_arrays(O.ref_extract, O.ref_window)
np.savez_compressed(LC.FIXTURE, **arrays)
print(os.path.basename(LC.FIXTURE), os.path.getsize(LC.FIXTURE), "bytes;", arrays["text_len"].size, "texts,", arrays["words"].size, "words")
for f, (lo, hi) in zip(LC.WINDOWS, zip(arrays["window_lo"], arrays["window_hi"])):
    print("  window", f, "lo", int(lo), "hi", int(hi))

recs = LC.protein_records()
for alphabet, k in LC.GPU_PROTEIN:
    samples = [(h, LC.sort_unique(w)) for (h, _), w in zip(recs, O.ref_extract(alphabet, k, 1.0, 0.0, [t for _, t in recs]))]
    name = "loader_%s_k%d.db" % (alphabet, k)
    db = MF.build_db(samples, k, 1.0, name, threads=1, alphabet=alphabet)
    with open(db, "rb") as f, lzma.open(db + ".xz", "wb", preset=9) as g:
        g.write(f.read())
    os.remove(db)
    print(name + ".xz", os.path.getsize(db + ".xz"), "bytes")
