"""csrc/prefetch.h on the CPU: tests/prefetch_check.cpp (its own main) includes the header directly and drives the
pipeline's announce / prepare state through the transitions its entries make — announce then register promotes and
starts the worker, the next register of the same buffer takes the prepared frame and flips the side; a refilled buffer
(first, last, a sampled middle row), another n, a device frame, a message and a deskewed frame do not; a failing
worker's rc and text come back from the call that consumes its frame; cancel and the deskew switch drop both records,
the dynamic-filter switch the prepared one only; a failed call consumes the announcement; wait keeps the prepared
frame; destruction joins a worker in flight — at 1, 63, 64, 65 and 200 rows.  Compiled with g++ into a temporary
directory (nothing is written into the tree): plain, with the address and undefined-behaviour sanitizers, and with the
thread sanitizer; each a stand-alone program."""
import os
import platform
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "prefetch_check.cpp")
INC = os.path.join(ROOT, "sage-icp_amd", "csrc")


def _without_address_randomisation(cmd):
    """gcc's thread sanitizer runtime does not start where the kernel randomises mappings over more bits than it knows
    ("FATAL: ThreadSanitizer: unexpected memory mapping", or a fault before main): the program runs with randomisation
    off for its own process, where setarch may do that."""
    setarch = shutil.which("setarch")
    if setarch and subprocess.run([setarch, platform.machine(), "-R", "true"], capture_output=True).returncode == 0:
        return [setarch, platform.machine(), "-R"] + cmd
    return cmd


@pytest.mark.parametrize("flags", [("-O2",),
                                   ("-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"),
                                   ("-O1", "-g", "-fsanitize=thread")],
                         ids=["plain", "sanitized", "thread-sanitized"])
def test_prefetch_state_follows_its_entries(tmp_path, flags):
    exe = str(tmp_path / "prefetch_check")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", *flags, "-pthread", "-I", INC, SRC, "-o", exe])
    cmd = _without_address_randomisation([exe]) if "-fsanitize=thread" in flags else [exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    last = r.stdout.strip().splitlines()[-1]
    assert last.startswith("prefetch_check: OK "), last
    # five frame sizes x the five groups of cases
    assert int(last.split()[-1]) > 5 * 40
