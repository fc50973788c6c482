"""csrc/knobs.h on the CPU, and the tree against its table.

tests/knobs_check.cpp (its own main) includes the header alone and checks the table (49 names, each once), every integer
knob unset / set / clamped / unset again over texts that decide (atoi's answers included), the three parsed knobs
(SAGEICP_DEVICES against the strtol loop sageicp_map_create had, SAGEICP_CU_SHARE, SAGEICP_MAP_ARCHIVE_MAX_ROWS) and
SAGEICP_SIZE_CLASSES, that a reference outlives a reload and an unchanged environment publishes nothing, and eight
reading threads beside a reloading one.  Compiled with g++ into a temporary directory (nothing is written into the
tree): plain, with the address and undefined-behaviour sanitizers, and with the thread sanitizer; each a stand-alone
program.

Three checks of the tree need no library: the table and INTEGRATION.md's knob section name the same knobs; every
SAGEICP_* name a test or a probe puts into an environment exists; the environment is read in knobs.h only."""
import ast
import glob
import os
import platform
import re
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "knobs_check.cpp")
INC = os.path.join(ROOT, "sage-icp_amd", "csrc")
NAME = r"SAGEICP_[A-Z0-9_]+"

# read by bench.py and the Python loader, not by the library
NOT_THE_LIBRARYS = {"SAGEICP_BENCH_DEVICE", "SAGEICP_BENCH_BACKEND", "SAGEICP_FORCE_COMM", "SAGEICP_NO_RCCL",
                    "SAGEICP_NO_P2P", "SAGEICP_VARIANT_LIB"}


def _without_address_randomisation(cmd):
    """gcc's thread sanitizer runtime does not start where the kernel randomises mappings over more bits than it knows:
    the program runs with randomisation off for its own process, where setarch may do that."""
    setarch = shutil.which("setarch")
    if setarch and subprocess.run([setarch, platform.machine(), "-R", "true"], capture_output=True).returncode == 0:
        return [setarch, platform.machine(), "-R"] + cmd
    return cmd


@pytest.mark.parametrize("flags", [("-O2",),
                                   ("-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"),
                                   ("-O1", "-g", "-fsanitize=thread")],
                         ids=["plain", "sanitized", "thread-sanitized"])
def test_knobs_load_clamp_and_publish(tmp_path, flags):
    exe = str(tmp_path / "knobs_check")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", *flags, "-pthread", "-I", INC, SRC, "-o", exe])
    cmd = _without_address_randomisation([exe]) if "-fsanitize=thread" in flags else [exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert "ThreadSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    last = r.stdout.strip().splitlines()[-1]
    assert last.startswith("knobs_check: OK "), last
    # 45 integer knobs x 16 texts x 3 checks, and the rest on top
    assert int(last.split()[-1]) > 45 * 16 * 3


def _read(path):
    with open(path, encoding="utf-8") as f:
        return f.read()


def _table_names():
    names = re.findall(r'"(%s)"' % NAME, _read(os.path.join(INC, "knobs.h")))
    assert len(names) == len(set(names)) == 49, sorted(names)
    return set(names)


def test_integration_md_lists_the_table():
    text = _read(os.path.join(ROOT, "INTEGRATION.md"))
    section = text[text.index("## 6a. Environment variables"):text.index("## 7. Python")]
    listed = set(re.findall(NAME, section)) - {"SAGEICP_VARIANT_LIB"}
    table = _table_names()
    assert not table - listed, "in knobs.h, not in INTEGRATION.md 6a: %s" % sorted(table - listed)
    assert not listed - table, "in INTEGRATION.md 6a, not in knobs.h: %s" % sorted(listed - table)


def _names_set_by_python(text):
    """the names a Python source puts into an environment: as text — setenv("N", environ["N"], env["N"],
    dict(os.environ, N=...) — and as syntax: a keyword argument N=..., a key of a dict display, a stored subscript"""
    found = set(re.findall(r"setenv\(\s*[\"'](%s)[\"']" % NAME, text))
    found |= set(re.findall(r"environ\[\s*[\"'](%s)[\"']\s*\]" % NAME, text))
    found |= set(re.findall(r"\benv\[\s*[\"'](%s)[\"']\s*\]" % NAME, text))
    for args in re.findall(r"dict\(\s*os\.environ\s*,([^)]*)\)", text):
        found |= set(re.findall(r"\b(%s)\s*=" % NAME, args))
    for node in ast.walk(ast.parse(text)):
        if isinstance(node, ast.keyword) and node.arg and re.fullmatch(NAME, node.arg):
            found.add(node.arg)
        elif isinstance(node, ast.Dict):
            found |= {k.value for k in node.keys
                      if isinstance(k, ast.Constant) and isinstance(k.value, str) and re.fullmatch(NAME, k.value)}
        elif isinstance(node, ast.Subscript) and isinstance(node.ctx, ast.Store):
            k = node.slice
            if isinstance(k, ast.Constant) and isinstance(k.value, str) and re.fullmatch(NAME, k.value):
                found.add(k.value)
    return found


def test_every_knob_a_test_or_probe_sets_exists():
    known = _table_names() | NOT_THE_LIBRARYS
    files = sorted(glob.glob(os.path.join(HERE, "**", "*.py"), recursive=True) +
                   glob.glob(os.path.join(ROOT, "profiles", "*.py")))
    assert len(files) > 100
    unknown = {}
    n_set = 0
    for path in files:
        names = _names_set_by_python(_read(path))
        n_set += len(names)
        if names - known:
            unknown[os.path.relpath(path, ROOT)] = sorted(names - known)
    for path in sorted(glob.glob(os.path.join(HERE, "**", "*.cpp"), recursive=True)):
        names = set(re.findall(r"setenv\(\s*\"(%s)\"" % NAME, _read(path)))
        n_set += len(names)
        if names - known:
            unknown[os.path.relpath(path, ROOT)] = sorted(names - known)
    assert not unknown, unknown
    assert n_set > 100          # (the matcher finds what the tests set: 37 files select their code paths this way)


def test_only_knobs_h_reads_the_environment():
    gone = re.compile(r"env_int\(|env_cached\(|EnvKnob")
    for path in sorted(glob.glob(os.path.join(INC, "*"))):
        text = _read(path)
        assert not gone.search(text), path
        if os.path.basename(path) != "knobs.h":
            assert "getenv" not in text, path
    assert "getenv" in _read(os.path.join(INC, "knobs.h"))
