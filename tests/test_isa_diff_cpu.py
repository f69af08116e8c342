"""tools/isa_diff.py compares two compilations of cdfo_amd/csrc after dropping the lines that name hipcc's per-file __hip_cuid_
symbol.  The normaliser must hide exactly that and nothing else: compiles nothing."""
import os, sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

ASM = """\t.text
\t.protected\t_ZN1kE
_ZN1kE:
\ts_load_dwordx2 s[0:1], s[4:5], 0x0
\ts_waitcnt lgkmcnt(0)
\tv_mov_b32_e32 v0, 0
\ts_endpgm
\t.type\t__hip_cuid_{cuid},@object
\t.globl\t__hip_cuid_{cuid}
__hip_cuid_{cuid}:
\t.byte\t0
\t.size\t__hip_cuid_{cuid}, 1
"""


def test_cuid_only_is_equal():
    from isa_diff import diff, normalise
    a, b = ASM.format(cuid="1c5e0d3a9b7f2e44"), ASM.format(cuid="9a8b7c6d5e4f3a21")
    assert a != b
    assert diff("k.hip", a, b) == []
    assert normalise(a) == normalise(b) and "\tv_mov_b32_e32 v0, 0" in normalise(a)


def test_one_instruction_is_different():
    from isa_diff import diff
    a = ASM.format(cuid="1c5e0d3a9b7f2e44")
    b = ASM.format(cuid="9a8b7c6d5e4f3a21").replace("v_mov_b32_e32 v0, 0", "v_mov_b32_e32 v0, 1")
    d = diff("k.hip", a, b)
    assert "-\tv_mov_b32_e32 v0, 0" in d and "+\tv_mov_b32_e32 v0, 1" in d
    assert not any("__hip_cuid_" in l for l in d)
    # a changed wait count is an instruction change too
    assert diff("k.hip", a, a.replace("lgkmcnt(0)", "lgkmcnt(1)"))
