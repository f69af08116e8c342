"""The host-side schedule switches of CVSR_V8's neighbour pipelines that no other test moves off their defaults:
``neighbour_streams`` (1 = everything on the caller's stream, 2 = one side stream per group), ``neighbour_group`` (frames per
group: 1 instead of 3) and, on the cached B = 1 path, ``overlap_new_frame`` / ``new_frame_alone`` (where the new frame's feature
extraction and its neighbour pipeline are enqueued).  The stream and new-frame switches issue the same launches on other
streams or in another order between independent launches: bit-identical results.  ``neighbour_group`` changes the batch size of
the group launches: held to the reference's golden outputs within the bound tests/test_gpu_cvsr_v8.py applies to these fixtures,
and to the bits of the default grouping (every kernel of a group launch works image by image).
fp16x2, injected noise (what the fixtures carry)."""
import itertools
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
TOL = 1e-3
GOLD = {"fresh": "cvsr_v8_b1_8x8.npz", "cached": "cvsr_v8_b1_16x16_cached.npz"}
_runs = {}


def _run(which, streams=2, group=3, overlap=False, alone=False):
    """(out, L1_fea, golden) of one forward on the fixture `which` under the given schedule; computed once per schedule."""
    key = (which, streams, group, overlap, alone)
    if key in _runs:
        return _runs[key]
    from arch.SIDECVSR_our import CVSR_V8
    from oracle.cvsr_v8_ref import make_inputs, make_state_dict
    g = np.load(os.path.join(os.path.dirname(__file__), "golden", GOLD[which]))
    model = CVSR_V8()
    model.load_state_dict(make_state_dict(int(g["wseed"])), strict=True)
    model = model.cuda().eval()
    model.precision = "fp16x2"
    model.neighbour_streams, model.neighbour_group, model.overlap_new_frame, model.new_frame_alone = streams, group, overlap, alone
    inp = make_inputs(int(g["B"]), int(g["H"]), int(g["W"]), int(g["iseed"]), str(g["layout"]))
    dev = {k: v.cuda() for k, v in inp.items() if k != "gumbel_u"}
    pre = torch.from_numpy(g["pre_L1_fea"]).cuda() if int(g["cached"]) else None
    with torch.no_grad():
        out, L1 = model(dev["x"], dev["mvs0"], dev["mvs1"], dev["pms"], dev["rms"], dev["ufs"], pre,
                        gumbel_uniform=[u.cuda() for u in inp["gumbel_u"]])
    torch.cuda.synchronize()
    assert model.last_range is not None and not model.last_range["fallback"]        # the fp16x2 schedule itself ran
    _runs[key] = (out.cpu(), L1.cpu().contiguous(), g)
    return _runs[key]


@pytest.mark.parametrize("which", ["fresh", "cached"])
def test_one_stream_equals_two_side_streams(which):
    out1, l1_1, _ = _run(which, streams=1)
    out2, l1_2, _ = _run(which, streams=2)
    assert torch.equal(out1, out2) and torch.equal(l1_1, l1_2)


@pytest.mark.parametrize("overlap,alone", [c for c in itertools.product((False, True), repeat=2) if c != (False, False)])
def test_new_frame_schedules_equal_the_plain_one(overlap, alone):
    out0, l1_0, _ = _run("cached")
    out, l1, _ = _run("cached", overlap=overlap, alone=alone)
    assert torch.equal(out, out0) and torch.equal(l1, l1_0)


@pytest.mark.parametrize("which", ["fresh", "cached"])
def test_groups_of_one_frame_match_the_golden_outputs(which):
    out, l1, g = _run(which, group=1)
    err_out = (out - torch.from_numpy(g["out"])).abs().max().item()
    err_l1 = (l1 - torch.from_numpy(g["L1_fea"])).abs().max().item()
    out3, l1_3, _ = _run(which, group=3)
    print(f"{which}: neighbour_group = 1 vs golden: out {err_out:.2e} L1_fea {err_l1:.2e}; bit-identical to neighbour_group = 3: "
          f"out {torch.equal(out, out3)}, L1_fea {torch.equal(l1, l1_3)} (max |diff| {(out - out3).abs().max().item():.2e})")
    assert err_out <= TOL and err_l1 <= TOL
    # every kernel of the group launches works image by image: measured bit-identical on an MI355X on both fixtures, so held to that
    assert torch.equal(out, out3) and torch.equal(l1, l1_3)
