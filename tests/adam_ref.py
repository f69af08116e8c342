"""The fp64 statement of one step of the device Adam (csrc/adam.hip, cdfo_amd/optim.py), written from its specification with numpy
alone: the gradient's norm, the skip, the clip coefficient and the five lines of the update.  Also the case list of the Adam tests,
the fp32 inputs of a case, and the bound of a case.

The bound of `p`, `m` and `v` is 16 x the fp32 floor, measured when the test runs: the largest difference between
``torch.optim.Adam(foreach=False)`` in fp32 on the CPU and the fp64 statement from the same fp32 inputs (an absolute difference over the
case's seven tensors; normalising both sides by the case's largest |p|, |m|, |v| changes nothing).  The cases make a wrong update visible
above ulp(p): lr = 1e-2 with |p| <= 1."""
import functools
import math

import numpy as np

CHUNK = 4096                                      # CDFO_ADAM_CHUNK
LR, BETAS, EPS = 1e-2, (0.9, 0.999), 1e-8
SIZES_A = (1, 3, 4, 5, 63, CHUNK - 1, 3 * CHUNK + 7)
SIZES_B = (65, CHUNK, CHUNK + 1, 4, 5, 1, 63)
ODD = 3                                           # the tensor whose view starts at an odd element of its buffer
GUARD = 8                                         # NaN elements on either side of a view

# name, sizes, gradient scale, the step this update makes, weight decay, max_norm as a multiple of the norm (None: off),
# and whether a skipped step (a NaN in the last element of the last tensor) comes first
CASES = [
    dict(name="g1e-6_t1_wd", sizes=SIZES_A, gscale=1e-6, step=1, wd=1e-5, clip=None, skip_first=False),
    dict(name="g1e-3_t1", sizes=SIZES_B, gscale=1e-3, step=1, wd=0.0, clip=None, skip_first=False),
    dict(name="g1_t1", sizes=SIZES_B, gscale=1.0, step=1, wd=0.0, clip=None, skip_first=True),
    dict(name="g1e3_t1_wd", sizes=SIZES_A, gscale=1e3, step=1, wd=1e-5, clip=None, skip_first=False),
    dict(name="g1_t2_wd", sizes=SIZES_A, gscale=1.0, step=2, wd=1e-5, clip=None, skip_first=True),
    dict(name="g1e-3_t2", sizes=SIZES_B, gscale=1e-3, step=2, wd=0.0, clip=None, skip_first=False),
    dict(name="g1_t1000_wd", sizes=SIZES_B, gscale=1.0, step=1000, wd=1e-5, clip=None, skip_first=False),
    dict(name="g1e3_t1000", sizes=SIZES_A, gscale=1e3, step=1000, wd=0.0, clip=None, skip_first=False),
    dict(name="g1e-6_t1000_wd", sizes=SIZES_A, gscale=1e-6, step=1000, wd=1e-5, clip=None, skip_first=False),
    dict(name="g1e-3_t2_wd_clip_half", sizes=SIZES_A, gscale=1e-3, step=2, wd=1e-5, clip=0.5, skip_first=False),
    dict(name="g1_t1_clip_above", sizes=SIZES_B, gscale=1.0, step=1, wd=0.0, clip=2.0, skip_first=False),
]
CASE_NAMES = [c["name"] for c in CASES]


def case(name):
    return CASES[CASE_NAMES.index(name)]


def grad_norm_ref(g):
    """(sum of squares, norm) of the fp32 gradients ``g`` in fp64."""
    total = math.fsum(float(np.square(np.asarray(gi, np.float64)).sum()) for gi in g)        # numpy's pairwise sum per tensor
    return total, math.sqrt(total) if total >= 0 else float("nan")


def clip_coefficient(norm, max_norm):
    """1 when clipping is off or the norm is inside; else max_norm / (norm + 1e-6) in fp64, rounded once to fp32."""
    if max_norm <= 0 or norm <= max_norm:
        return 1.0
    return float(np.float32(max_norm / (norm + 1e-6)))


def adam_step_ref(p, g, m, v, step, skipped, lr=LR, betas=BETAS, eps=EPS, wd=0.0, max_norm=0.0):
    """One step in fp64.  p, g, m, v: lists of arrays (any float type; taken to fp64); ``step`` steps were made before.  Returns
    (p, m, v, step, skipped, norm), the lists fp64; a non-finite sum of squares leaves p, m, v and step, and counts in skipped."""
    p, g, m, v = ([np.asarray(a, np.float64) for a in x] for x in (p, g, m, v))
    with np.errstate(all="ignore"):
        total = sum(float(np.square(gi).sum()) for gi in g)
    if not math.isfinite(total):
        return p, m, v, step, skipped + 1, math.sqrt(total) if total > 0 else float("nan")
    total, norm = grad_norm_ref(g)
    coef = clip_coefficient(norm, max_norm)
    step += 1
    b1, b2 = betas
    step_size = lr / (1.0 - b1 ** step)
    inv_bc2_sqrt = 1.0 / math.sqrt(1.0 - b2 ** step)
    po, mo, vo = [], [], []
    for pi, gi, mi, vi in zip(p, g, m, v):
        gi = coef * gi
        gi = gi + wd * pi
        mi = mi + (1.0 - b1) * (gi - mi)
        vi = b2 * vi + (1.0 - b2) * gi * gi
        pi = pi - step_size * mi / (np.sqrt(vi) * inv_bc2_sqrt + eps)
        po.append(pi), mo.append(mi), vo.append(vi)
    return po, mo, vo, step, skipped, norm


@functools.lru_cache(maxsize=None)
def inputs(name):
    """The fp32 inputs of a case: lists p, g, m, v (read-only arrays), ``step0`` steps made before, ``max_norm`` (0.0: off)."""
    c = case(name)
    rs = np.random.RandomState(1000 + CASE_NAMES.index(name))
    p, g, m, v = [], [], [], []
    for n in c["sizes"]:
        pi = rs.uniform(-1.0, 1.0, n).astype(np.float32)
        gi = (c["gscale"] * rs.standard_normal(n)).astype(np.float32)
        gi[rs.randint(0, 7, n) == 0] = 0.0                                   # a seventh of the gradients exactly 0
        if c["step"] == 1:
            mi, vi = np.zeros(n, np.float32), np.zeros(n, np.float32)
        elif c["step"] == 2:                                                  # what one step from zero moments leaves
            g0 = (c["gscale"] * rs.standard_normal(n)).astype(np.float32)
            mi, vi = (np.float32(0.1) * g0).astype(np.float32), (np.float32(0.001) * g0 * g0).astype(np.float32)
        else:
            mi = (0.5 * c["gscale"] * rs.standard_normal(n)).astype(np.float32)
            vi = (0.5 * np.square(c["gscale"] * rs.standard_normal(n))).astype(np.float32)
        for a, lst in ((pi, p), (gi, g), (mi, m), (vi, v)):
            a.setflags(write=False)
            lst.append(a)
    norm = grad_norm_ref(g)[1]
    return dict(p=p, g=g, m=m, v=v, step0=c["step"] - 1, wd=c["wd"], max_norm=0.0 if c["clip"] is None else c["clip"] * norm,
                skip_first=c["skip_first"], norm=norm)


@functools.lru_cache(maxsize=None)
def expected(name):
    """The fp64 statement's (p, m, v, step, skipped, norm) of a case; a case with ``skip_first`` makes the skipped step first."""
    x = inputs(name)
    step, skipped = x["step0"], 0
    if x["skip_first"]:
        p, m, v, step, skipped, _ = adam_step_ref(x["p"], poisoned(x["g"]), x["m"], x["v"], step, skipped, wd=x["wd"], max_norm=x["max_norm"])
        assert step == x["step0"] and skipped == 1 and all(np.array_equal(a, b) for a, b in zip(p + m + v, x["p"] + x["m"] + x["v"]))
    return adam_step_ref(x["p"], x["g"], x["m"], x["v"], step, skipped, wd=x["wd"], max_norm=x["max_norm"])


def poisoned(g, value=float("nan")):
    """The gradients with ``value`` in the last element of the last tensor."""
    g = [a.copy() for a in g]
    g[-1][-1] = value
    return g


@functools.lru_cache(maxsize=None)
def floor(name):
    """The fp32 floor of a case: max |torch.optim.Adam(foreach=False), fp32, CPU - the fp64 statement| for (p, m, v).  torch has no
    clip inside its step: the gradient is scaled by the fp32 coefficient first, as ``clip_grad_norm_`` does."""
    import torch
    x = inputs(name)
    params = [torch.from_numpy(a.copy()) for a in x["p"]]
    coef = np.float32(clip_coefficient(x["norm"], x["max_norm"]))
    for t, gi in zip(params, x["g"]):
        t.grad = torch.from_numpy((coef * gi).astype(np.float32) if coef != 1 else gi.copy())
    opt = torch.optim.Adam(params, lr=LR, betas=BETAS, eps=EPS, weight_decay=x["wd"], foreach=False)
    if x["step0"]:
        for t, mi, vi in zip(params, x["m"], x["v"]):
            opt.state[t] = {"step": torch.tensor(float(x["step0"])), "exp_avg": torch.from_numpy(mi.copy()), "exp_avg_sq": torch.from_numpy(vi.copy())}
    opt.step()
    pe, me, ve = expected(name)[:3]
    diff = lambda got, want: max(float(np.abs(a.astype(np.float64) - b).max()) for a, b in zip(got, want))  # noqa: E731
    return (diff([t.numpy() for t in params], pe), diff([opt.state[t]["exp_avg"].numpy() for t in params], me),
            diff([opt.state[t]["exp_avg_sq"].numpy() for t in params], ve))


def errors(name, p, m, v):
    """max |got - the fp64 statement| of (p, m, v), lists of arrays; a non-finite value where the statement is finite is inf."""
    out = []
    for got, want in zip((p, m, v), expected(name)[:3]):
        worst = 0.0
        for a, b in zip(got, want):
            d = np.abs(np.asarray(a, np.float64) - b)
            worst = max(worst, float("inf") if not np.isfinite(d).all() else float(d.max()))
        out.append(worst)
    return tuple(out)


def within_bound(name, p, m, v, show=None):
    """(ok, figures): every error of the case within 16 x its floor."""
    err, fl = errors(name, p, m, v), floor(name)
    figures = "%s: error p %.3e m %.3e v %.3e | floor p %.3e m %.3e v %.3e" % ((name,) + err + fl)
    if show is not None:
        show(figures)
    return all(e <= 16.0 * f for e, f in zip(err, fl)), figures
