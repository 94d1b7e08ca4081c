"""The distance mode off the device: the witness the device tests compare with (tests/distance_cases.py) reproduces every golden of the
reference, kmdbh_format_measure is the console's notation, `distance -host` is the host loop, and the ABI exports the new entry points."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import distance_cases as DC
from conftest import ROOT
from test_host_cpu import DISTANCE_CASES

EXE = os.path.join(ROOT, "kmer-db_amd", "bin", "kmer-db-amd")


@pytest.fixture(scope="module")
def L(K):
    lib = K.capi.lib()
    lib.kmdbh_metric.restype = ctypes.c_double
    return lib


def test_the_restatement_reproduces_the_references_goldens(L, golden_dir):
    assert len(DISTANCE_CASES) == 19
    for opts, src, want in DISTANCE_CASES:
        data = open(os.path.join(golden_dir, src), "rb").read()
        assert DC.distance_file(L, data, opts) == open(os.path.join(golden_dir, want), "rb").read(), (opts, src)


def test_format_measure_is_the_consoles_notation(K):
    f = K.format_measure
    assert f(0.0) == b"0" and f(-0.0) == b"0"
    assert f(5e-7) == DC.fmt_measure(5e-7) and f(4.9999999e-7) == b"0.000000"
    assert f(0.9999995) == DC.fmt_measure(0.9999995) and f(0.99999949) == b"0.999999"
    assert f(-0.25) == b"-0.250000" and f(-1e-9) == b"-0.000000" and f(-123456.7890125) == DC.fmt_measure(-123456.7890125)
    assert f(1.0) == b"1.000000" and f(4294967295.0) == b"4294967295.000000" and f(12345678901.5) == b"12345678901.500000"
    rng = np.random.default_rng(11)
    vals = np.concatenate([rng.random(400_000), -rng.random(100_000), rng.random(200_000) * 10.0 ** rng.integers(-9, 10, 200_000),
                           (rng.integers(0, 2_000_000, 200_000) + 0.5) / 1e6,                      # the rounding boundaries themselves
                           np.nextafter((rng.integers(0, 2_000_000, 100_000) + 0.5) / 1e6, 0.0)])
    assert vals.size == 1_000_000
    lib = K.capi.lib()
    buf = ctypes.create_string_buffer(48)
    for v in vals.tolist():
        n = lib.kmdbh_format_measure(v, buf)
        assert buf.raw[:n] == DC.fmt_measure(v), v


@pytest.mark.parametrize("case", DISTANCE_CASES, ids=lambda c: c[2] + ":" + "_".join(c[0]))
def test_cli_distance_host_switch_gives_the_goldens(golden_dir, tmp_path, case):
    opts, src, want = case
    out = tmp_path / "out"
    r = subprocess.run([EXE, "distance", "-host"] + opts + [os.path.join(golden_dir, src), str(out)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert out.read_bytes() == open(os.path.join(golden_dir, want), "rb").read()


def test_abi_exports_the_distance_entry_points(K):
    hdr = open(os.path.join(ROOT, "include", "kmdb_amd.h")).read()
    assert re.search(r"^#define KMDB_HAS_DISTANCE 1$", hdr, re.M) and "#define KMDB_ABI_VERSION 8" in hdr
    lib = ctypes.CDLL(K.lib_path())
    for name in ("kmdb_distance_begin", "kmdb_distance_rows", "kmdb_distance_out_free", "kmdb_distance_free", "kmdb_distance_stats_get", "kmdbh_format_measure"):
        assert hasattr(lib, name) and name in K.capi.EXPORTS, name
    assert K.capi.DISTANCE_DECLINED == int(re.search(r"#define KMDB_DISTANCE_DECLINED (\d+)", hdr).group(1))
    # arguments are checked before a device is touched
    L = K.capi.lib()
    assert L.kmdb_distance_begin(None, None) != 0 and b"kmdb_distance_begin" in L.kmdb_last_error()
    assert L.kmdb_distance_rows(None, None, 0, 0, None) != 0 and b"kmdb_distance_rows" in L.kmdb_last_error()
    assert L.kmdb_distance_stats_get(None, None) != 0
    with pytest.raises(K.KmdbError, match="unknown measure"):
        K.Distance(17, 18, [1, 2])
    with pytest.raises(K.KmdbError, match="bounds"):
        K.Distance("mash", 18, [1, 2], filters=[("mash", 0.0, 1.0)] * 13)


def test_forced_device_path_needs_a_device_and_host_switch_wins(K, golden_dir, tmp_path):
    env = dict(os.environ, KMDB_DISTANCE_DEVICE="1")
    if K.device_count() == 0:
        r = subprocess.run([EXE, "distance", "mash", os.path.join(golden_dir, "synth.a2a"), str(tmp_path / "o")], capture_output=True, text=True, env=env)
        assert r.returncode != 0 and "no usable GPU" in r.stderr
    # -host wins over the variable; no variable and no device: the host loop, silently
    r = subprocess.run([EXE, "distance", "-host", "mash", os.path.join(golden_dir, "synth.a2a"), str(tmp_path / "o")], capture_output=True, text=True, env=env)
    assert r.returncode == 0 and r.stderr == ""
    assert (tmp_path / "o").read_bytes() == open(os.path.join(golden_dir, "synth.a2a.mash"), "rb").read()
