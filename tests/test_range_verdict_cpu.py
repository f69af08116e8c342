"""CPU check of the fp16 range guard's decision (``CVSR_V8._range_verdict``), shared by the eager forward and the captured
forwards of cdfo_amd/graph.py: four host int32 probe words -> accept, or repeat the forward in bf16x3.  No GPU, no HIP library
(cdfo_amd.kernels loads it lazily)."""
import torch

from cdfo_amd.cvsr_v8 import CVSR_V8


def _probe(amax, in_nonfinite=0, out_amax=0.0, out_nonfinite=0):
    bits = lambda v: torch.tensor([v], dtype=torch.float32).view(torch.int32).item()
    return torch.tensor([bits(amax), in_nonfinite, bits(out_amax), out_nonfinite], dtype=torch.int32)


def test_range_verdict_window_edges_nonfinite_flags_and_instance_override():
    m = CVSR_V8()
    lo, hi = m.FP16_WINDOW
    assert (lo, hi) == (2.0 ** -6, 2.0 ** 11)
    v = m._range_verdict(_probe(0.0))                      # an all-zero trunk input fits any format
    assert v == {"trunk_input_amax": 0.0, "nonfinite": False, "fallback": False}
    for amax in (lo, hi, 1.0):                             # both edges are inside
        assert m._range_verdict(_probe(amax, out_amax=1e30)) == {"trunk_input_amax": amax, "nonfinite": False, "fallback": False}
    for amax in (torch.nextafter(torch.tensor(lo), torch.tensor(0.0)).item(),
                 torch.nextafter(torch.tensor(hi), torch.tensor(float("inf"))).item()):   # one fp32 ulp outside either edge
        v = m._range_verdict(_probe(amax))
        assert v["fallback"] and not v["nonfinite"] and v["trunk_input_amax"] == amax
    for flags in ((1, 0), (0, 1), (1, 1)):                 # a NaN / infinity at the trunk's input or output
        v = m._range_verdict(_probe(1.0, flags[0], 1.0, flags[1]))
        assert v["fallback"] and v["nonfinite"]
    m.FP16_WINDOW = (1e-30, 1e-29)                         # read from the instance (tests/test_gpu_graph.py overrides it there)
    assert m._range_verdict(_probe(1.0))["fallback"]
    assert not m._range_verdict(_probe(5e-30))["fallback"]
    assert not CVSR_V8()._range_verdict(_probe(1.0))["fallback"]
