"""csrc/row_shift.h on the CPU: tests/row_shift_check.cpp (its own main) includes the header directly and checks, for all
26 shifts of a home voxel into a neighbouring one, the number of new voxels (9, 15, 19), rank -> voxel, the lanes'
dealing at 4, 8 and 16 lanes, the old position of every kept voxel and the shifted occupancy mask against the mask
built voxel by voxel (a seeded million masks per shift).  Compiled with g++ into a temporary directory (nothing is
written into the tree); once more with the address and undefined-behaviour sanitizers."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "row_shift_check.cpp")
INC = os.path.join(ROOT, "sage-icp_amd", "csrc")


@pytest.mark.parametrize("flags", [("-O2",), ("-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all")],
                         ids=["plain", "sanitized"])
def test_row_shift_arithmetic_is_exact(tmp_path, flags):
    exe = str(tmp_path / "row_shift_check")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", *flags, "-I", INC, SRC, "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    last = r.stdout.strip().splitlines()[-1]
    assert last.startswith("row_shift_check: OK "), last
    # 26 shifts x a million masks, and the structural checks on top
    assert int(last.split()[-1]) > 26 * 1000000
