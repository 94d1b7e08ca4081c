"""What the compiler needs for the emit kernels of the all2all call, read from the resource remarks the build writes beside the objects
(kmer-db_amd/build/a2a_blocks.resources.txt: registers, spills, scratch, occupancy and LDS per kernel — no instruction is looked at).

The bounds are the figures of the kernels BEFORE they were compiled per record path (one body for few streams / row mode / second level:
k1w_kernel 126 VGPRs, 123 scalar spills, four waves per SIMD; k1n_kernel<2, 4> 93 / 30, five waves; k2d_kernel 88 bytes of scratch per lane)
and what folding the unused paths away reached on those sources (95 VGPRs = five waves, 71 = seven waves): an instantiation that needs
more than the one body did, or a default instantiation that falls back below the occupancy the folding alone gave, is a regression."""
import os
import re

import pytest

from conftest import ROOT

RESOURCES = os.path.join(ROOT, "kmer-db_amd", "build", "a2a_blocks.resources.txt")
FIELDS = {"VGPRs": "vgpr", "AGPRs": "agpr", "ScratchSize [bytes/lane]": "scratch", "Occupancy [waves/SIMD]": "occupancy", "SGPRs Spill": "sgpr_spill",
          "VGPRs Spill": "vgpr_spill", "LDS Size [bytes/block]": "lds"}


def _kernel(mangled):
    """(kernel, template arguments) of a mangled name of a2a_blocks.hip's anonymous namespace: ("k1w_kernel", (0, 0))"""
    m = re.match(r"_ZN12_GLOBAL__N_1\d+([A-Za-z0-9_]+?_kernel)(?:I((?:L[bi]\d+E)+)E)?", mangled)
    if not m:
        return None
    return m.group(1), tuple(int(a) for a in re.findall(r"L[bi](\d+)E", m.group(2) or ""))


@pytest.fixture(scope="module")
def table():
    assert os.path.exists(RESOURCES), ("%s is missing: the build writes it (make -C kmer-db_amd, or __graft_entry__.build()) from the compiler's "
                                       "-Rpass-analysis=kernel-resource-usage remarks" % RESOURCES)
    out, cur = {}, None
    with open(RESOURCES, errors="replace") as f:
        for line in f:
            m = re.search(r"remark: Function Name: (\S+)", line)
            if m:
                key = _kernel(m.group(1))
                cur = out.setdefault(key, {}) if key else None
                continue
            m = re.search(r"remark:\s+(.+?): (\d+) \[-Rpass-analysis", line)
            if m and cur is not None and m.group(1) in FIELDS:
                cur[FIELDS[m.group(1)]] = int(m.group(2))
    emit = {k: v for k, v in out.items() if k[0] in ("k1w_kernel", "k1n_kernel", "k2d_kernel")}
    assert emit, "no emit kernel in %s" % RESOURCES
    for (name, targs), r in sorted(emit.items()):
        assert set(r) == set(FIELDS.values()), (name, targs, r)
    return emit


def test_the_table_goes_on_record(table, capsys, record_property):
    """the whole table in the log of a passing run too (printed past pytest's capture, and as properties of the junit record): the scalar-spill counts
    that were reached are on record"""
    lines = ["%-34s %5s %5s %11s %11s %8s %10s %6s" % ("kernel", "VGPRs", "AGPRs", "SGPR spills", "VGPR spills", "scratch", "waves/SIMD", "LDS")]
    for (name, targs), r in sorted(table.items()):
        label = "%s<%s>" % (name, ", ".join(map(str, targs)))
        lines.append("%-34s %5d %5d %11d %11d %8d %10d %6d" % (label, r["vgpr"], r["agpr"], r["sgpr_spill"], r["vgpr_spill"], r["scratch"], r["occupancy"], r["lds"]))
        record_property(label, dict(r))
    with capsys.disabled():
        print("\n" + "\n".join(lines))


def test_the_few_streams_wide_kernel_holds_five_waves(table):
    """k1w_kernel<no rows, no L2>, the benchmark's: no scratch, five waves per SIMD or more (the folding alone reached 95 VGPRs)"""
    r = table[("k1w_kernel", (0, 0))]
    assert r["scratch"] == 0 and r["occupancy"] >= 5, r


def test_the_default_narrow_kernel_holds_six_waves(table):
    """k1n_kernel<2, 4, no rows>, the benchmark's: no scratch, six waves per SIMD or more (the folding alone reached 71 VGPRs)"""
    r = table[("k1n_kernel", (2, 4, 0))]
    assert r["scratch"] == 0 and r["occupancy"] >= 6, r


def test_no_instantiation_needs_more_than_the_one_body_did(table):
    """all three paths of the wide kernel and both of the default narrow kernel exist; none above the VGPRs and scalar spills of the kernel that held
    every path at once; no scratch but in k1n_kernel<1, 4, *> (the A/B variant that trades 60 - 90 bytes of scratch for a fourth wave)"""
    wide = {k[1]: r for k, r in table.items() if k[0] == "k1w_kernel"}
    assert set(wide) == {(0, 0), (1, 0), (1, 1)}, sorted(wide)
    for targs, r in wide.items():
        assert r["vgpr"] <= 126 and r["sgpr_spill"] <= 123 and r["scratch"] == 0, (targs, r)
    narrow = {k[1]: r for k, r in table.items() if k[0] == "k1n_kernel"}
    assert {(2, 4, 0), (2, 4, 1)} <= set(narrow), sorted(narrow)
    for targs, r in narrow.items():
        if targs[0] == 2:
            assert r["vgpr"] <= 93 and r["sgpr_spill"] <= 30, (targs, r)
        if targs[:2] != (1, 4):
            assert r["scratch"] == 0, (targs, r)


def test_the_slice_apply_kernel_has_no_scratch(table):
    r = table[("k2d_kernel", ())]
    assert r["scratch"] == 0 and r["vgpr_spill"] == 0, r
