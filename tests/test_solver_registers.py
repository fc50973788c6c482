"""k_loop_solve<8> runs beside k_loop's grid on one SIMD: the grid's residency margin was measured with the solving
wave at 152 vector registers (allocated in steps of 8), so it must not take more.  Its publish hides the lane index
from the optimiser (kernels.hip, lane_now) to stay there: 160 otherwise.  k_loop itself: 72 registers, 7 waves per SIMD."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# bytes of scratch per lane of k_loop<LW, FILT> before the pose had a copy per XCD (profiles/r15/resource_usage.txt): no more now
PARENT_SCRATCH = {"1, true": 44, "1, false": 24, "2, true": 52, "2, false": 52, "3, true": 68, "3, false": 36,
                  "4, true": 68, "4, false": 32}
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


@pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which("hipcc")), reason="needs hipcc")
def test_register_budget_of_the_one_launch_loop():
    r = subprocess.run(["bash", os.path.join(ROOT, "tools", "resource_usage.sh"),
                        os.path.join(ROOT, "sage-icp_amd", "csrc", "kernels.hip")], capture_output=True, text=True, cwd=ROOT)
    assert r.returncode == 0, r.stdout + r.stderr
    rows = {}
    for line in r.stdout.splitlines():
        m = re.match(r"(?:void )?(\S.*?) vgpr (\d+) agpr \d+ sgpr \d+ scratch (\d+) occ (\d+)", line)
        if m:
            rows[m.group(1)] = (int(m.group(2)), int(m.group(3)), int(m.group(4)))
    solve = [v for k, v in rows.items() if "k_loop_solve<8>" in k]
    assert len(solve) == 1, r.stdout + r.stderr
    print("k_loop_solve<8>:", solve[0])
    assert solve[0][0] <= 152 and solve[0][1] == 0
    loops = {k: v for k, v in rows.items() if re.search(r"k_loop<\d", k)}
    assert set(PARENT_SCRATCH) == {re.search(r"k_loop<(\d, \w+)>", k).group(1) for k in loops}, sorted(loops)
    for k, (vgpr, scratch, occ) in loops.items():
        print(k, vgpr, scratch, occ)
        assert vgpr <= 72 and occ >= 7, (k, vgpr, occ)
        assert scratch <= PARENT_SCRATCH[re.search(r"k_loop<(\d, \w+)>", k).group(1)], (k, scratch)
