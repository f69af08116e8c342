"""The LPIPS loss tests' shared cases: the committed (widths, size, seeds) table the device's gradient is checked on, and, computed once
per process on the CPU from the statement alone (tests/lpips_loss_ref.py), the fp64 gradient and the fp32-trunk gradient whose
distance is the floor the device test takes its bound from.  Nothing here ever looks at a device result.

The table's frame seeds are CHOSEN: a gradient through a ReLU or a max-pool is discontinuous where a pre-activation is 0 or a
window's two largest elements are equal, and an fp32 trunk may sit on the other side of such a kink than the fp64 statement.  So every
case satisfies the kink condition (tests/test_lpips_loss_cpu.py asserts it): the smallest |pre-activation| and the smallest gap
between the two largest elements of a live pool window, in the fp64 statement, are at least 8 x the largest pre-activation difference
between the fp32-trunk and the fp64-trunk statements.  The ratios found when the seeds were searched (seeds 0 .. 47) are beside them."""
import functools

import numpy as np
import torch
import torch.nn.functional as F

import lpips_loss_ref as ref

W1 = (16, 16, 32, 32, 16)
W2 = (16, 32, 32, 48, 64)

# name: (widths, model seed, size, frames, frame seed, upstream gradient per frame)        ratio found
CASES = {
    "w1-16x16-n3": (W1, 21, (16, 16), 3, 6, (1.0, 0.5, 2.0)),      # 20.0   stage 5 is 1 x 1
    "w2-16x16-n1": (W2, 22, (16, 16), 1, 2, (1.0,)),               # 46.0
    "w1-17x19-n1": (W1, 21, (17, 19), 1, 3, (0.75,)),              # 43.7   every pool floors
    "w2-17x19-n3": (W2, 22, (17, 19), 3, 3, (2.0, 1.0, 0.25)),     # 10.8
    "w1-24x41-n1": (W1, 21, (24, 41), 1, 40, (1.0,)),              # 15.5   several tiles of the stem, stage 5 is 1 x 2
    "w2-24x41-n1": (W2, 22, (24, 41), 1, 45, (1.5,)),              # 29.1
}


@functools.lru_cache(maxsize=None)
def model(widths, seed):
    from cdfo_amd import metrics as M
    return M.lpips_random_params(widths, seed)


@functools.lru_cache(maxsize=None)
def case(name):
    """(params, sr, hr, weights) of a case: fp32 numpy [n,h,w] stacks and fp32 [n] upstream gradients, shared and read-only."""
    widths, mseed, size, n, fseed, weights = CASES[name]
    sr, hr = ref.frames(size, n, fseed)
    weights = np.array(weights, dtype=np.float32)
    for a in (sr, hr, weights):
        a.setflags(write=False)
    return model(widths, mseed), sr, hr, weights


@functools.lru_cache(maxsize=None)
def gradients(name):
    """(fp64 gradient [n,h,w], the fp32-trunk statement's gradient, the floor: their largest difference over the largest |gradient|)."""
    params, sr, hr, weights = case(name)
    g64 = ref.gradient(sr, hr, params, weights)
    g32 = ref.gradient(sr, hr, params, weights, trunk_dtype=torch.float32)
    for a in (g64, g32):
        a.setflags(write=False)
    return g64, g32, err(g32, g64)


def err(got, want) -> float:
    """max |got - want| / max |want|"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return float(np.abs(got - want).max() / np.abs(want).max())


# ---- the adjoint kernels' cases and their oracles: torch's autograd on the CPU in fp64 ----
def dist_bwd_autograd(pre, fb, lin, gscale, gin=None):
    """d(sum_n gscale_n d_n(relu(pre_n), fb_n) + sum gin relu(pre)) / d pre by autograd on the statement: [N,h,w,C] fp64."""
    p = torch.from_numpy(pre).to(torch.float64).requires_grad_(True)
    A = F.relu(p)
    loss = sum(float(gscale[n]) * ref.layer_distance(A[n].permute(2, 0, 1), torch.from_numpy(fb[n]).permute(2, 0, 1), lin) for n in range(len(pre)))
    out = torch.autograd.grad(loss, A, retain_graph=True)[0]
    if gin is not None:
        out = out + torch.from_numpy(gin)
    A.backward(out)
    return p.grad.numpy()


@functools.lru_cache(maxsize=None)
def dist_case(C, h, w, N=3):
    """(pre-activation, fa = relu(pre), fb, lin, gscale, gin): pixel (0, 0) of frame 0 all zero in fa, the last pixel of the last
    frame all zero in fb, a NaN in gin under a non-positive fa; gscale (1.5, 0, 0.25)[:N]."""
    rs = np.random.RandomState(C + 7 * h + w)
    pre = rs.randn(N, h, w, C).astype(np.float32)
    pre[0, 0, 0] = -np.abs(pre[0, 0, 0])
    fb = np.maximum(rs.randn(N, h, w, C), 0).astype(np.float32)
    fb[-1, -1, -1] = 0
    lin = rs.rand(C)
    gin = rs.randn(N, h, w, C).astype(np.float32)
    gin[0, 0, 0, 1] = np.nan
    return pre, np.maximum(pre, 0), fb, lin, np.array((1.5, 0.0, 0.25), dtype=np.float32)[:N], gin


@functools.lru_cache(maxsize=None)
def pool_case(H, W, C):
    """x with ties (values from a set of five), a NaN, and two NaNs in one window where the size allows; g random."""
    rs = np.random.RandomState(C + 7 * H + W)
    x = rs.randint(0, 5, (2, H, W, C)).astype(np.float32)
    x[0, 0, 1, 0] = np.nan
    x[1, 1, 0, 1], x[1, 0, 1, 1] = np.nan, np.nan
    x[1, 0, 0, 2], x[1, 1, 1, 2] = np.nan, np.nan
    return x, rs.randn(2, H // 2, W // 2, C).astype(np.float32)


def torch_pool2_bwd(x, g):
    t = torch.from_numpy(x).permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    F.max_pool2d(t, 2, 2).backward(torch.from_numpy(g).permute(0, 3, 1, 2).contiguous())
    return t.grad.permute(0, 2, 3, 1).contiguous().numpy()


@functools.lru_cache(maxsize=None)
def stem_bwd_case(h, w, C0, normalize):
    """(stem weights fp32 [C0,3,3,3], g fp32 [2,h,w,C0] with zeros as a ReLU mask leaves them, the fp64 statement's gradient at the
    samples [2,h,w], the fp32 statement's distance from it as a fraction of the largest |gradient|)."""
    params = model((C0, 16, 16, 16, 16), 23)
    rs = np.random.RandomState(C0 + 7 * h + w)
    g = (rs.randn(2, h, w, C0) * (rs.rand(2, h, w, C0) < 0.6)).astype(np.float32)
    w0 = np.array(params.weights[0])

    def grad(dtype):
        x = torch.zeros(2, h, w, dtype=dtype, requires_grad=True)
        y = torch.cat([F.conv2d(ref.trunk_input(x[j], normalize), torch.from_numpy(w0).to(dtype), padding=1) for j in range(2)])
        (y * torch.from_numpy(g).to(dtype).permute(0, 3, 1, 2)).sum().backward()
        return x.grad.to(torch.float64).numpy()

    want = grad(torch.float64)
    return w0, g, want, err(grad(torch.float32), want)
