"""The one-launch loop stays off scratch memory, by the compiler's own account.

k_loop at 72 vector registers (7 waves per SIMD) has no register to spare: whatever the compiler can prove invariant
across the iteration loop — a lane index from threadIdx, a predicate from the set-up's scalars, an fp64 literal — it
hoists in front of the loop and then parks in scratch memory or in the lanes of a reserved register, and whether the
reloads land inside the pass (c2-cold 5 % slower, profiles/r20/README.md) was up to the register allocation.  Since
round 21 nothing of that kind lives across the loop (loop_kernel.h, "THE RULE"): every k_loop compiles
to ScratchSize 0 with no spilled scalar.  This test holds it there — an edit that brings a spill back fails here, on the
CPU, before anybody has to find a 5 % regression on the GPU.

One device-only compile of csrc/kernels.hip for gfx950 with build.py's flags plus -Rpass-analysis=kernel-resource-usage
(half a minute); the remarks are read as tools/resource_usage.sh reads them.  Compiler remarks only: the assembly is
neither produced nor looked at."""
import importlib.util
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")

# k_loop<LW, FILT>: these run the benchmark's workloads and the mid-size frames — no scratch, no spilled scalar, <= 72
# registers, 7 waves per SIMD
REQUIRED = [(2, True), (2, False), (3, False), (4, False)]
# bytes of scratch per lane of every k_loop<LW, FILT>, from round 21's build: none may take more
SCRATCH = {(1, True): 0, (1, False): 0, (2, True): 0, (2, False): 0, (3, True): 0, (3, False): 0, (4, True): 0, (4, False): 0}


def _flags():
    spec = importlib.util.spec_from_file_location("_sageicp_build", os.path.join(ROOT, "sage-icp_amd", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return list(mod.FLAGS)


def _remarks():
    """-> {mangled kernel name: {"vgpr", "agpr", "sgpr", "scratch", "occ", "sgpr_spill", "vgpr_spill", "lds"}}"""
    cmd = [HIPCC] + _flags() + ["--cuda-device-only", "-c", os.path.join(ROOT, "sage-icp_amd", "csrc", "kernels.hip"),
                                "-o", os.devnull, "-Rpass-analysis=kernel-resource-usage"]
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-4000:]
    keys = [("TotalSGPRs:", "sgpr"), (" VGPRs:", "vgpr"), ("AGPRs:", "agpr"), ("ScratchSize", "scratch"), ("Occupancy", "occ"),
            ("SGPRs Spill:", "sgpr_spill"), ("VGPRs Spill:", "vgpr_spill")]
    out, name, cur = {}, None, {}
    for line in r.stderr.splitlines():
        if "remark:" not in line:
            continue
        line = re.sub(r" \[-Rpass.*", "", line)
        last = line.split()[-1]
        if "Function Name:" in line:
            name, cur = last, {}
            continue
        for pat, key in keys:
            if pat in line:
                cur[key] = int(last)
        if "LDS Size" in line and name is not None:       # (the last remark of a kernel, as in tools/resource_usage.sh)
            cur["lds"] = int(last)
            out[name] = cur
    return out


@pytest.fixture(scope="module")
def remarks():
    if not (os.path.exists(HIPCC) or shutil.which(HIPCC)):
        pytest.skip("needs hipcc (%s)" % HIPCC)
    return _remarks()


def _loops(remarks):
    loops = {}
    for name, v in remarks.items():
        m = re.search(r"6k_loopILi(\d)ELb([01])EEE", name)
        if m:
            loops[(int(m.group(1)), m.group(2) == "1")] = v
    return loops


def test_the_loop_kernels_that_run_the_workloads_use_no_scratch(remarks):
    loops = _loops(remarks)
    assert set(loops) == set(SCRATCH), sorted(loops)
    for key in REQUIRED:
        v = loops[key]
        print("k_loop<%d, %s>" % key, v)
        assert v["scratch"] == 0 and v["sgpr_spill"] == 0 and v["vgpr_spill"] == 0, (key, v)
        assert v["vgpr"] <= 72 and v["agpr"] == 0 and v["occ"] == 7, (key, v)


def test_no_loop_kernel_takes_more_scratch_than_recorded(remarks):
    for key, v in sorted(_loops(remarks).items()):
        print("k_loop<%d, %s>" % key, v)
        assert v["scratch"] <= SCRATCH[key], (key, v)
        assert v["vgpr"] <= 72 and v["occ"] == 7, (key, v)


def test_the_launch_per_iteration_kernels_use_no_scratch(remarks):
    icp = {n: v for n, v in remarks.items() if re.search(r"5k_icpILi\d", n)}
    assert len(icp) == 28, sorted(icp)           # every instantiation kernels.hip dispatches to
    for n, v in sorted(icp.items()):
        assert v["scratch"] == 0, (n, v)
