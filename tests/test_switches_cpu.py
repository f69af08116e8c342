"""The developer switches (CDFO_* environment variables) have ONE declaration, cdfo_amd/switches.py.  These CPU tests keep the
table, the reads in the sources and the table in INTEGRATION.md in step, pin the lookup's rules, and check that the kernels'
developer ablations are compiled only with -DCDFO_DEV_ABLATIONS.  Nothing here imports torch: the sources are read as text."""
import os
import re
import subprocess
import tempfile

import pytest

from cdfo_amd import switches

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cdfo_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
HARNESS_NAMES = {"CDFO_BENCH_BACKEND", "CDFO_BENCH_PG_TIMEOUT_S", "CDFO_FORKSERVER"}     # read by bench.py / tests/conftest.py themselves
ROWS = {s.name: s for s in switches.TABLE}


def _files(*dirs, ext):
    for d in dirs:
        for base, _, names in os.walk(os.path.join(ROOT, d)):
            for n in sorted(names):
                if n.endswith(ext):
                    yield os.path.join(base, n)


def _reads(paths, call):
    """{name: [files]} of every CDFO_* name that is the first argument of `call(` in the given files."""
    found = {}
    for p in paths:
        for name in re.findall(call + r'\(\s*"(CDFO_[A-Z0-9_]+)"', open(p).read()):
            found.setdefault(name, []).append(os.path.relpath(p, ROOT))
    return found


def test_every_read_is_a_row_of_its_layer_and_every_row_is_read():
    hip = _reads(_files("cdfo_amd/csrc", ext=(".hip", ".h")), r"\b(?:getenv|cdfo_switch)")
    py = _reads(_files("cdfo_amd", "arch", "ops", ext=".py"), r"\bswitches\.get")
    assert hip and py
    for layer, found in (("hip", hip), ("python", py)):
        for name, where in found.items():
            assert name in ROWS, f"{name} ({where}) is not declared in cdfo_amd/switches.py"
            assert ROWS[name].layer == layer, f"{name} is read by the {layer} layer ({where}) but declared as {ROWS[name].layer}"
    for s in switches.TABLE:
        assert s.name in (hip if s.layer == "hip" else py), f"{s.name} is declared ({s.layer}) but nothing reads it"
        assert s.kind in (switches.ONOFF, switches.INT, switches.PATH) and s.layer in ("python", "hip") and s.meaning
        assert s.kind != switches.ONOFF or s.default in (0, 1)
    assert len(ROWS) == len(switches.TABLE)          # no name twice
    assert not HARNESS_NAMES & set(ROWS)


def test_hip_defaults_match_the_table():
    """cdfo_switch("NAME", dflt): the default written at the call site is the row's default."""
    for p in _files("cdfo_amd/csrc", ext=(".hip", ".h")):
        for name, dflt in re.findall(r'cdfo_switch\(\s*"(CDFO_[A-Z0-9_]+)"\s*,\s*(-?\d+)\s*\)', open(p).read()):
            assert int(dflt) == ROWS[name].default, (name, p)


def test_integration_md_lists_exactly_the_table():
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    header = open(os.path.join(ROOT, "include", "cdfo_hip.h")).read()
    abi_constants = set(re.findall(r"\bCDFO_[A-Z0-9_]+", header))                 # CDFO_EINVAL, CDFO_STORE_*, ...: not environment variables
    named = set(re.findall(r"(?<!-D)\bCDFO_[A-Z0-9_]+", text)) - abi_constants     # (-DCDFO_DEV_ABLATIONS is a compiler define)
    assert named - HARNESS_NAMES == set(ROWS), (sorted(named - HARNESS_NAMES - set(ROWS)), sorted(set(ROWS) - named))
    assert HARNESS_NAMES <= named
    for s in switches.TABLE:          # the row itself: | `NAME` | default | kind | layer | meaning |
        row = re.search(r"^\| `%s` \|.*$" % s.name, text, re.M)
        assert row and f"| {s.kind}" in row.group(0) and f"| {s.layer} |" in row.group(0), s.name


def test_no_environment_read_outside_the_two_readers():
    allowed = {os.path.join("cdfo_amd", "switches.py"): "os.environ.get(",                 # the Python reader
               os.path.join("cdfo_amd", "csrc", "common.h"): "getenv(name)",               # the HIP reader (cdfo_switch)
               os.path.join("cdfo_amd", "build.py"): 'os.environ.get("HIPCC"'}             # the compiler's path: not a switch
    bad = []
    for p in _files("cdfo_amd", "arch", "ops", ext=(".py", ".hip", ".h")):
        rel = os.path.relpath(p, ROOT)
        for i, line in enumerate(open(p), 1):
            if re.search(r"\bos\.environ\b|\bgetenv\s*\(", line) and allowed.get(rel, "\0") not in line:
                bad.append(f"{rel}:{i}: {line.strip()}")
    assert not bad, "\n".join(bad)


def test_lookup_rules(monkeypatch):
    get = switches.get
    with pytest.raises(KeyError):
        get("CDFO_NOT_A_SWITCH")
    with pytest.raises(KeyError):
        get("CDFO_WS_RING")                      # a row, but the library's: Python does not read it
    for name, env, want in (("CDFO_WINO", None, True), ("CDFO_WINO", "0", False), ("CDFO_WINO", "1", True),
                            ("CDFO_FEA_R_1PASS", None, False), ("CDFO_FEA_R_1PASS", "1", True), ("CDFO_FEA_R_1PASS", "0", False),
                            ("CDFO_LIB_PATH", None, None), ("CDFO_LIB_PATH", "/x/lib.so", "/x/lib.so")):
        get.cache_clear()
        monkeypatch.delenv(name, raising=False) if env is None else monkeypatch.setenv(name, env)
        assert get(name) is want or get(name) == want, (name, env)
    for bad in ("", "2", "yes", "01"):           # one truth rule: anything but "0" / "1" is an error naming the variable
        get.cache_clear()
        monkeypatch.setenv("CDFO_UDSA_N16", bad)
        with pytest.raises(ValueError, match="CDFO_UDSA_N16"):
            get("CDFO_UDSA_N16")
    # read once per process: a later change of the environment is not seen
    get.cache_clear()
    monkeypatch.setenv("CDFO_TRUNK_SIDE", "0")
    assert get("CDFO_TRUNK_SIDE") is False
    monkeypatch.setenv("CDFO_TRUNK_SIDE", "1")
    assert get("CDFO_TRUNK_SIDE") is False
    get.cache_clear()
    # the library's own switches obey the same rules when the library is loaded
    monkeypatch.setenv("CDFO_WS_WAVES", "8")
    monkeypatch.setenv("CDFO_ATTN_XCD", "0")
    switches.check_hip_environment()
    monkeypatch.setenv("CDFO_WS_WAVES", "10")
    with pytest.raises(ValueError, match="CDFO_WS_WAVES"):
        switches.check_hip_environment()
    monkeypatch.setenv("CDFO_WS_WAVES", "12")
    monkeypatch.setenv("CDFO_RING_SPLIT", "")
    with pytest.raises(ValueError, match="CDFO_RING_SPLIT"):
        switches.check_hip_environment()


def _ring_kernel_dbg_arguments(*defines):
    """The DBG template arguments of the kernels that conv3x3_ring.hip instantiates, from the (mangled) kernel symbols of its gfx950 assembly."""
    with tempfile.TemporaryDirectory() as td:
        out = os.path.join(td, "k.s")
        r = subprocess.run([HIPCC, "-O3", "--offload-arch=gfx950", "-std=c++17", "-ffp-contract=fast", *defines, "-S", "--cuda-device-only",
                            "-o", out, os.path.join(CSRC, "conv3x3_ring.hip")], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
        mangled = re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", open(out).read(), re.M)
    dbg = [int(m.group(1)) for n in mangled for m in [re.search(r"conv3x3_ring(?:_split)?_kernelILb[01]ELi(\d+)E", n)] if m]
    assert len(dbg) == len(mangled) >= 3, mangled      # dense, four-tap, wave-specialised four-tap
    return dbg


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc (cross-compiles without a GPU)")
def test_ablation_kernels_exist_only_in_the_developer_build():
    assert set(_ring_kernel_dbg_arguments()) == {0}
    dev = _ring_kernel_dbg_arguments("-DCDFO_DEV_ABLATIONS")
    assert 0 in dev and {1, 2, 4, 8, 9, 10, 16} <= set(dev)
