"""The DSIM_OPT_MEM_DERIVED instances in the gfx950 assembly of dsim_step.hip (CPU only: hipcc cross-compiles, ~20 s): each
issues exactly six global_load_dword fewer than the sibling that reads last_vel / last_rates and as many stores, none uses
scratch, and none runs fewer waves per SIMD than that sibling.  (The quad instances that read all ten target fields would:
71 VGPRs, 7 waves against 64 / 8 — they do not exist, dsim_step ignores the bit there.)"""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    """{mangled kernel name: {"ld", "st", "NumVgprs", "ScratchSize", "Occupancy"}} of dsim_step.hip, the build's flags."""
    import __graft_entry__ as ge
    flags = [f for f in ge.HIPCC_FLAGS if f not in ("-shared", "-fPIC")]
    out = tmp_path_factory.mktemp("isa") / "dsim_step.s"
    subprocess.check_call(["/opt/rocm/bin/hipcc", *flags, "-S", "--cuda-device-only", "-o", str(out),
                           os.path.join(ge.CSRC, "dsim_step.hip")], stderr=subprocess.DEVNULL)
    ks, cur = {}, None
    for ln in out.read_text().split("\n"):
        m = re.match(r"^(_Z\w+):", ln)
        if m:
            cur = m.group(1)
            ks[cur] = {"ld": 0, "st": 0}
            continue
        if cur is None:
            continue
        op = ln.strip().split(" ")[0] if ln.startswith("\t") else ""
        if op == "global_load_dword":
            ks[cur]["ld"] += 1
        elif op == "global_store_dword":
            ks[cur]["st"] += 1
        m = re.match(r"\s*;\s*(NumVgprs|ScratchSize|Occupancy): (\d+)", ln)
        if m:
            ks[cur][m.group(1)] = int(m.group(2))
    return ks


def _b(x):
    return "Lb1E" if x else "Lb0E"


def _fast(noise, nt, tc, md):
    # k_step_fast<NOISE, NT, EXT = false, CH = false, SUB = 1, ACT = false, TC, MD>
    return f"_Z11k_step_fastI{_b(noise)}{_b(nt)}Lb0ELb0ELi1ELb0E{_b(tc)}{_b(md)}Ev5StepK"


def _hexa(noise, nt, md):
    # k_step_hexa<NOISE, NT, S1 = true, ACT = false, MD>
    return f"_Z11k_step_hexaI{_b(noise)}{_b(nt)}Lb1ELb0E{_b(md)}Ev5StepK"


PAIRS = ([(_fast(n, s, True, True), _fast(n, s, True, False)) for n in (0, 1) for s in (0, 1)]
         + [(_hexa(n, s, True), _hexa(n, s, False)) for n in (0, 1) for s in (0, 1)])


def test_all_eight_instances_exist(kernels):
    missing = [md for md, _ in PAIRS if md not in kernels] + [sib for _, sib in PAIRS if sib not in kernels]
    assert not missing, missing
    # ... and no others: the looped, waypoint, explicit-action and ten-target-field instances ignore the bit
    md_all = [k for k in kernels if re.match(r"_Z11k_step_(fast|hexa)I.*Lb1EEv5StepK$", k) and
              (k.startswith("_Z11k_step_fast") and k.count("Lb") == 7 or k.startswith("_Z11k_step_hexa") and k.count("Lb") == 5)]
    assert sorted(md_all) == sorted(md for md, _ in PAIRS)


@pytest.mark.parametrize("md,sib", PAIRS)
def test_six_loads_fewer_same_stores_no_scratch(kernels, md, sib):
    a, b = kernels[md], kernels[sib]
    assert a["ld"] == b["ld"] - 6, (a, b)
    assert a["st"] == b["st"], (a, b)
    assert a["ScratchSize"] == 0


@pytest.mark.parametrize("md,sib", PAIRS)
def test_waves_per_simd_not_below_the_sibling(kernels, md, sib):
    a, b = kernels[md], kernels[sib]
    assert a["Occupancy"] >= b["Occupancy"], (a, b)


def test_headline_instance(kernels):
    a, b = kernels[_fast(1, 1, 1, True)], kernels[_fast(1, 1, 1, False)]
    assert a["Occupancy"] == b["Occupancy"] == 8, (a, b)
    assert a["NumVgprs"] <= 64
