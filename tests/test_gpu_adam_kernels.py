"""csrc/adam.hip on the device, through `DeviceAdam` (a table builder over the three entry points) and the C ABI: the cases of
tests/adam_ref.py against the fp64 statement, on views inside NaN-filled buffers, one of them starting at an odd element."""
import ctypes as C

import numpy as np
import pytest
import torch

import adam_ref as ref

pytestmark = pytest.mark.gpu


def _views(arrays, dev):
    """Each array as a view inside a NaN-filled device buffer (GUARD elements either side; tensor ODD one element further)."""
    bufs, views = [], []
    for t, a in enumerate(arrays):
        s = ref.GUARD + (1 if t == ref.ODD else 0)
        b = torch.full((a.size + 2 * ref.GUARD + 1,), float("nan"), dtype=torch.float32, device=dev)
        b[s:s + a.size] = torch.from_numpy(np.array(a)).to(dev)
        bufs.append(b)
        views.append(b[s:s + a.size])
    return bufs, views


def _guards_intact(bufs, sizes):
    for t, (b, n) in enumerate(zip(bufs, sizes)):
        s = ref.GUARD + (1 if t == ref.ODD else 0)
        if not (bool(torch.isnan(b[:s]).all()) and bool(torch.isnan(b[s + n:]).all())):
            return False
    return True


def run(name, grads_seq=None, max_norm="case", wd=None):
    """The case on the device -> dict of what it left."""
    from cdfo_amd.optim import DeviceAdam
    dev = torch.device("cuda", 0)
    x = ref.inputs(name)
    sizes = [a.size for a in x["p"]]
    pbufs, params = _views(x["p"], dev)
    mn = x["max_norm"] if max_norm == "case" else max_norm
    opt = DeviceAdam(params, lr=ref.LR, betas=ref.BETAS, eps=ref.EPS, weight_decay=x["wd"] if wd is None else wd, max_grad_norm=mn or None)
    if x["step0"]:
        opt.load_state_dict({"step": x["step0"], "skipped": 0, "exp_avg": [torch.from_numpy(np.array(a)) for a in x["m"]],
                             "exp_avg_sq": [torch.from_numpy(np.array(a)) for a in x["v"]]})
    if grads_seq is None:
        grads_seq = ([ref.poisoned(x["g"])] if x["skip_first"] else []) + [x["g"]]
    g_kept = True
    for grads in grads_seq:
        gbufs, gviews = _views(grads, dev)
        before = [b.clone() for b in gbufs]
        for p, g in zip(params, gviews):
            p.grad = g
        opt.step()
        g_kept = g_kept and all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(before, gbufs))
    sd = opt.state_dict()
    return dict(p=[p.cpu().numpy() for p in params], m=[t.cpu().numpy() for t in sd["exp_avg"]], v=[t.cpu().numpy() for t in sd["exp_avg_sq"]],
                step=opt.steps, skipped=opt.skipped, norm=float(opt.grad_norm), guards=_guards_intact(pbufs, sizes), g_kept=g_kept,
                aligned=[p.data_ptr() % 16 == 0 for p in params])


def _same_bits(a, b):
    return all(np.array_equal(x.view(np.int32), y.view(np.int32)) for k in "pmv" for x, y in zip(a[k], b[k]))


@pytest.mark.parametrize("name", ref.CASE_NAMES)
def test_case_matches_the_fp64_statement(name):
    """Every case within 16 x its fp32 floor; guards and g keep their bits; the norm within 1e-12; a second run gives equal bits."""
    got, again = run(name), run(name)
    want = ref.expected(name)
    ok, figures = ref.within_bound(name, got["p"], got["m"], got["v"], show=print)
    assert ok, figures
    assert got["aligned"] == [t != ref.ODD for t in range(7)]                      # the odd view takes the scalar path, the others the vector path
    assert got["guards"] and got["g_kept"] and (got["step"], got["skipped"]) == (want[3], want[4])
    print("norm %.17g, statement %.17g" % (got["norm"], want[5]))
    assert abs(got["norm"] - want[5]) <= 1e-12 * want[5]
    assert _same_bits(got, again) and got["norm"] == again["norm"]


def test_zero_gradients_leave_the_parameters():
    x = ref.inputs("g1_t1")
    got = run("g1_t1", grads_seq=[[np.zeros_like(g) for g in x["g"]]], wd=0.0)
    assert all(np.array_equal(a.view(np.int32), b.view(np.int32)) for a, b in zip(got["p"], x["p"]))
    assert got["step"] == 1 and got["norm"] == 0.0 and all(not a.any() for a in got["m"] + got["v"])


def test_a_max_norm_above_the_norm_changes_no_bit():
    x = ref.inputs("g1_t1_clip_above")
    assert x["max_norm"] > x["norm"]
    assert _same_bits(run("g1_t1_clip_above"), run("g1_t1_clip_above", max_norm=0.0))


def test_a_max_norm_of_half_the_norm_matches_the_statement():
    name = "g1e-3_t2_wd_clip_half"
    x = ref.inputs(name)
    assert abs(x["max_norm"] - 0.5 * x["norm"]) < 1e-12 * x["norm"]
    got = run(name)
    ok, figures = ref.within_bound(name, got["p"], got["m"], got["v"], show=print)
    assert ok, figures
    assert not _same_bits(got, run(name, max_norm=0.0))                                  # and the clip did something


@pytest.mark.parametrize("bad", [float("nan"), float("inf"), -float("inf")])
@pytest.mark.parametrize("where", ["one-element tensor", "last element of the last tensor"])
def test_a_non_finite_gradient_skips_the_step(bad, where):
    name = "g1_t2_wd"                                                                     # moments from a loaded state, step 1 made
    x = ref.inputs(name)
    grads = [g.copy() for g in x["g"]]
    t = [g.size for g in grads].index(1) if where.startswith("one") else len(grads) - 1
    grads[t][-1] = bad
    got = run(name, grads_seq=[grads])
    assert (got["step"], got["skipped"]) == (x["step0"], 1) and got["guards"] and got["g_kept"]
    assert all(np.array_equal(a.view(np.int32), b.view(np.int32)) for k in "pmv" for a, b in zip(got[k], x[k]))
    # the next finite step is the statement's step t, not t + 1 (the case itself makes a skipped step first)
    after = run(name, grads_seq=[grads, x["g"]])
    want = ref.expected(name)
    ok, figures = ref.within_bound(name, after["p"], after["m"], after["v"])
    assert ok and (after["step"], after["skipped"]) == (want[3], 1), figures


def test_entry_points_refuse_bad_arguments():
    from cdfo_amd import _lib
    from cdfo_amd.optim import chunk_table
    lib = _lib.lib()
    dev = torch.device("cuda", 0)
    p, g = torch.zeros(8, device=dev), torch.zeros(8, device=dev)
    offsets, chunks, total = chunk_table([8])
    host = torch.tensor([[p.data_ptr(), g.data_ptr(), 0, 8]], dtype=torch.int64)
    table, ch = host.to(dev), torch.from_numpy(chunks).to(dev)
    m, v = torch.zeros(total, device=dev), torch.zeros(total, device=dev)
    partials, scal, cnt = torch.zeros(1, dtype=torch.float64, device=dev), torch.zeros(6, dtype=torch.float64, device=dev), torch.zeros(2, dtype=torch.int64, device=dev)
    P = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    norm = lambda h=host, tb=table, nt=1, c=ch, nc=1, pa=partials: lib.cdfo_grad_norm_partials(  # noqa: E731
        None if h is None else h.data_ptr(), None if tb is None else P(tb), nt, None if c is None else P(c), nc, None if pa is None else P(pa), None)
    step = lambda h=host, nt=1, nc=1, mm=m, tot=total, s=scal: lib.cdfo_adam_step(  # noqa: E731
        None if h is None else h.data_ptr(), P(table), nt, P(ch), nc, None if mm is None else P(mm), P(v), tot, None if s is None else P(s),
        0.9, 0.999, 1e-8, 0.0, None)
    scalars = lambda pa=partials, nc=1, b1=0.9, c=cnt, s=scal, lr=1e-3: lib.cdfo_adam_scalars(  # noqa: E731
        None if pa is None else P(pa), nc, lr, b1, 0.999, 0.0, None if c is None else P(c), None if s is None else P(s), None)
    assert norm() == 0 and scalars() == 0 and step() == 0
    assert [norm(h=None), norm(tb=None), norm(c=None), norm(pa=None), norm(nt=0), norm(nt=-1), norm(nc=0), norm(nc=-2)] == [-1] * 8
    assert [step(h=None), step(mm=None), step(s=None), step(nt=0), step(nc=0), step(tot=0), step(tot=-4), step(tot=6), step(tot=4)] == [-1] * 9
    assert [scalars(pa=None), scalars(c=None), scalars(s=None), scalars(nc=0), scalars(nc=-1), scalars(b1=1.0), scalars(lr=-1.0)] == [-1] * 7
    for col, value in ((0, 0), (1, 0), (2, 2), (2, -4), (3, -1)):                        # null p, null g, offset % 4, offset < 0, n < 0
        bad = host.clone()
        bad[0, col] = value
        assert norm(h=bad) == -1 and step(h=bad) == -1
    torch.cuda.synchronize()
    assert int(cnt[0]) == 1 and int(cnt[1]) == 0 and not bool(p.any())
