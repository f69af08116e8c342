"""`cdfo_amd.optim.DeviceAdam` on the parameters of ``CVSR_V8(SCGs=8)``: three steps of given random gradients against the fp64
statement's trajectory (tests/adam_ref.py), its state through a fresh object and from ``torch.optim.Adam``, the version counters that
the model's packed-weight caches are keyed on, and the errors."""
import numpy as np
import pytest
import torch

import adam_ref as ref

pytestmark = pytest.mark.gpu
LR, WD, STEPS = 1e-2, 1e-5, 3


@pytest.fixture(scope="module")
def world():
    """The model's initial parameters, four steps' gradients, the fp64 trajectory of three steps and the fp32 floor: computed once."""
    from arch.SIDECVSR_our import CVSR_V8
    torch.manual_seed(3)
    model = CVSR_V8(SCGs=8)
    names = [k for k, _ in model.named_parameters()]
    p0 = [p.detach().numpy().copy() for p in model.parameters()]
    rs = np.random.RandomState(7)
    grads = []
    for s in range(STEPS + 1):
        step = []
        for a in p0:
            g = (10.0 ** -s * 1e-2 * rs.standard_normal(a.shape)).astype(np.float32)
            g[rs.randint(0, 7, a.shape) == 0] = 0.0
            step.append(g)
        grads.append(step)
    zeros = [np.zeros_like(a) for a in p0]
    traj, (p, m, v, step) = [], (p0, zeros, zeros, 0)
    for s in range(STEPS):
        p, m, v, step, _, norm = ref.adam_step_ref(p, grads[s], m, v, step, 0, lr=LR, wd=WD)
        traj.append((p, m, v, norm))
    params = [torch.from_numpy(a.copy()) for a in p0]
    opt = torch.optim.Adam(params, lr=LR, betas=ref.BETAS, eps=ref.EPS, weight_decay=WD, foreach=False)
    for s in range(STEPS):
        for t, g in zip(params, grads[s]):
            t.grad = torch.from_numpy(g.copy())
        opt.step()
    diff = lambda got, want: max(float(np.abs(a.astype(np.float64) - b).max()) for a, b in zip(got, want))  # noqa: E731
    floor = (diff([t.numpy() for t in params], p), diff([opt.state[t]["exp_avg"].numpy() for t in params], m),
             diff([opt.state[t]["exp_avg_sq"].numpy() for t in params], v))
    return dict(names=names, p0=p0, grads=grads, traj=traj, floor=floor)


def _on_device(arrays):
    return [torch.from_numpy(a.copy()).cuda() for a in arrays]


def _give(params, grads):
    for p, g in zip(params, grads):
        p.grad = torch.from_numpy(g).cuda()


def _check(world, params, sd, what):
    p, m, v, _ = world["traj"][-1]
    worst = [0.0, 0.0, 0.0]
    for i in range(len(params)):
        for k, (got, want) in enumerate(((params[i], p[i]), (sd["exp_avg"][i], m[i]), (sd["exp_avg_sq"][i], v[i]))):
            d = np.abs(got.detach().cpu().numpy().astype(np.float64) - want)
            assert np.isfinite(d).all(), (what, world["names"][i])
            worst[k] = max(worst[k], float(d.max()))
            assert d.max() <= 16.0 * world["floor"][k], (what, world["names"][i], "pmv"[k], float(d.max()), world["floor"][k])
    print("%s: error p %.3e m %.3e v %.3e | floor p %.3e m %.3e v %.3e" % ((what,) + tuple(worst) + world["floor"]))


def test_three_steps_follow_the_fp64_trajectory_and_the_state_round_trips(world):
    from cdfo_amd.optim import DeviceAdam
    params = _on_device(world["p0"])
    opt = DeviceAdam(zip(world["names"], params), lr=LR, betas=ref.BETAS, eps=ref.EPS, weight_decay=WD)
    for s in range(STEPS):
        _give(params, world["grads"][s])
        opt.step()
        want = world["traj"][s][3]
        assert abs(float(opt.grad_norm) - want) <= 1e-12 * want
    assert opt.steps == STEPS and opt.skipped == 0
    sd = opt.state_dict()
    assert sd["step"] == STEPS and sd["skipped"] == 0 and len(sd["exp_avg"]) == len(sd["exp_avg_sq"]) == len(params) == len(world["names"])
    assert [tuple(t.shape) for t in sd["exp_avg"]] == [tuple(p.shape) for p in params]
    _check(world, params, sd, "DeviceAdam, three steps")
    # state_dict -> fresh object -> load_state_dict -> one more step: the bits of the uninterrupted object
    twins = [p.clone() for p in params]
    fresh = DeviceAdam(twins, lr=LR, betas=ref.BETAS, eps=ref.EPS, weight_decay=WD)
    fresh.load_state_dict({k: ([t.cpu() if isinstance(t, torch.Tensor) else t for t in v] if isinstance(v, list) else v) for k, v in sd.items()})
    for o, ps in ((opt, params), (fresh, twins)):
        _give(ps, world["grads"][STEPS])
        o.step()
    a, b = opt.state_dict(), fresh.state_dict()
    assert (a["step"], a["skipped"]) == (b["step"], b["skipped"]) == (STEPS + 1, 0)
    for x, y in zip(params + a["exp_avg"] + a["exp_avg_sq"], twins + b["exp_avg"] + b["exp_avg_sq"]):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))
    assert float(opt.grad_norm) == float(fresh.grad_norm)


def test_a_torch_adam_state_loads_and_continues(world):
    from cdfo_amd.optim import DeviceAdam, load_into_torch_adam
    params = _on_device(world["p0"])
    theirs = torch.optim.Adam(params, lr=LR, betas=ref.BETAS, eps=ref.EPS, weight_decay=WD)
    for s in range(STEPS - 1):
        _give(params, world["grads"][s])
        theirs.step()
    opt = DeviceAdam(params, lr=1.0, betas=(0.5, 0.5), eps=1.0, weight_decay=1.0)          # the state's hyper-parameters replace these
    opt.load_state_dict(theirs.state_dict())
    assert opt.steps == STEPS - 1 and (opt.lr, opt.betas, opt.eps, opt.weight_decay) == (LR, ref.BETAS, ref.EPS, WD)
    _give(params, world["grads"][STEPS - 1])
    opt.step()
    _check(world, params, opt.state_dict(), "torch.optim.Adam two steps, DeviceAdam the third")
    # and back: the device state continues on torch.optim.Adam
    back = torch.optim.Adam(params, lr=LR, betas=ref.BETAS, eps=ref.EPS, weight_decay=WD)
    load_into_torch_adam(back, opt.state_dict())
    assert all(float(back.state[p]["step"]) == STEPS for p in params)
    assert all(torch.equal(back.state[p]["exp_avg"], m) for p, m in zip(params, opt.state_dict()["exp_avg"]))


def test_a_step_bumps_the_version_counters_the_weight_caches_are_keyed_on():
    from arch.SIDECVSR_our import CVSR_V8
    from cdfo_amd.optim import DeviceAdam
    from oracle.cvsr_v8_ref import make_inputs
    dev = torch.device("cuda", 0)
    inp = {k: (v.to(dev) if isinstance(v, torch.Tensor) else v) for k, v in make_inputs(1, 16, 24, 55).items()}
    forward = lambda mdl: mdl(inp["x"], None, inp["mvs1"], inp["pms"], inp["rms"], inp["ufs"])[0]  # noqa: E731
    torch.manual_seed(5)
    model = CVSR_V8(SCGs=8).to(dev).eval()
    with torch.no_grad():
        forward(model)                                                                   # the packed-weight caches now hold the old weights
    opt = DeviceAdam(model.named_parameters(), lr=1e-2)
    versions = [p._version for p in model.parameters()]
    g = torch.Generator(device=dev).manual_seed(1)
    for p in model.parameters():
        p.grad = torch.randn(p.shape, device=dev, generator=g)
    opt.step()
    assert all(p._version > v for p, v in zip(model.parameters(), versions))
    torch.manual_seed(9)
    with torch.no_grad():
        stepped = forward(model)
    fresh = CVSR_V8(SCGs=8)
    fresh.load_state_dict({k: v.cpu() for k, v in model.state_dict().items()})
    fresh = fresh.to(dev).eval()
    torch.manual_seed(9)
    with torch.no_grad():
        want = forward(fresh)
    assert torch.equal(stepped.view(torch.int32), want.view(torch.int32))


def test_errors_come_before_any_launch():
    from cdfo_amd.optim import DeviceAdam
    dev = torch.device("cuda", 0)
    ok = torch.zeros(8, device=dev)
    for bad in ([], [torch.zeros(8)], [torch.zeros(8, device=dev, dtype=torch.float64)], [torch.zeros(4, 4, device=dev).t()],
                [torch.zeros(8, device=dev, dtype=torch.float16)]):
        with pytest.raises(ValueError):
            DeviceAdam(bad)
    # parameters on two devices: the branch needs a second GPU, which the one-GPU test machine does not have; there it stays unrun
    # (a CPU tensor beside a device tensor is refused by the check above it, not by this one)
    if torch.cuda.device_count() > 1:
        with pytest.raises(ValueError, match="cuda:1"):
            DeviceAdam([ok, torch.zeros(8, device="cuda:1")])
    for mn in (0.0, -1.0, float("inf"), float("nan"), True, "1"):
        with pytest.raises(ValueError, match="max_grad_norm"):
            DeviceAdam([ok], max_grad_norm=mn)
    a, b = torch.ones(8, device=dev), torch.ones(4, 4, device=dev)
    opt = DeviceAdam([("first.weight", a), ("second.weight", b)], lr=1e-2)
    a.grad = torch.ones(8, device=dev)
    with pytest.raises(ValueError, match="second.weight .*no gradient"):
        opt.step()
    b.grad = torch.ones(4, 4, device=dev, dtype=torch.float32).t().contiguous().t()      # not contiguous
    assert not b.grad.is_contiguous()
    with pytest.raises(ValueError, match="second.weight"):
        opt.step()
    b.grad = None
    b.grad = torch.ones(4, 4, device=dev)
    a.grad = None
    with pytest.raises(ValueError, match="first.weight .*no gradient"):
        opt.step()
    torch.cuda.synchronize()
    assert opt.steps == 0 and opt.skipped == 0 and bool((a == 1).all()) and bool((b == 1).all())   # nothing was launched
    a.grad = torch.ones(8, device=dev)
    opt.step()
    assert opt.steps == 1 and bool((a < 1).all()) and bool((b < 1).all())
    opt.zero_grad()
    assert a.grad is None and b.grad is None
