"""LPIPS as this project defines it, stated with torch on the CPU in fp64 throughout.  The device path
(`cdfo_amd.metrics.lpips_layers_u8`) is tested against this file; `tests/test_lpips_cpu.py` holds a second, numpy-only statement
that shares nothing with it.

Two 8-bit luma frames, result ``a`` and ground truth ``b``, over their common top-left region, no border dropped.  A sample v becomes
x = v / 255, with ``normalize`` 2 x - 1, then three channels (x - shift_c) / scale_c.  The trunk is VGG-shaped: five stages of 2, 2, 3,
3, 3 convolutions (3 x 3, zeros round the SCALED tensor, bias, ReLU), a 2 x 2 / 2 max-pool that floors odd sizes in front of stages
2 .. 5, the taps behind each stage.  Per tap, with n(F) = F / (sqrt(sum_c F_c^2) + 1e-10): d_k = mean over pixels of sum_c lin_k[c]
(n(A)_c - n(B)_c)^2, and LPIPS = (((d_0 + d_1) + d_2) + d_3) + d_4.

``trunk_dtype=torch.float32`` runs the trunk -- the scaling and the convolutions, up to and including the ReLU outputs -- in fp32, as
the device does; everything behind the features stays fp64.  The difference to the fp64 trunk is the fp32 floor the device tests take
their bounds from.  Parity with the ``lpips`` package is unpinned: neither it nor torchvision nor any weights are available."""
import numpy as np
import torch
import torch.nn.functional as F

SHIFT = (-.030, -.088, -.188)
SCALE = (.458, .448, .450)
STAGES = (2, 2, 3, 3, 3)


def common(a, b):
    """The two frames cut to their common top-left region, as numpy uint8 [h,w]."""
    a, b = np.asarray(a), np.asarray(b)
    assert a.dtype == np.uint8 and b.dtype == np.uint8 and a.ndim == 2 and b.ndim == 2
    h, w = min(a.shape[0], b.shape[0]), min(a.shape[1], b.shape[1])
    assert h >= 16 and w >= 16
    return a[:h, :w], b[:h, :w]


def trunk_input(frame, normalize: bool = True, dtype=torch.float64) -> torch.Tensor:
    """uint8 [h,w] -> [1,3,h,w] of ``dtype``, every operation in that type."""
    x = torch.from_numpy(np.array(frame)).to(dtype) / 255
    if normalize:
        x = 2 * x - 1
    shift, scale = torch.tensor(SHIFT, dtype=dtype), torch.tensor(SCALE, dtype=dtype)
    return ((x[None, :, :] - shift[:, None, None]) / scale[:, None, None])[None]


def _conv(x, params, i, dtype):
    w, b = torch.from_numpy(np.array(params.weights[i])).to(dtype), torch.from_numpy(np.array(params.biases[i])).to(dtype)
    return F.relu(F.conv2d(x, w, b, padding=1))


def stem(frame, params, normalize: bool = True, dtype=torch.float64) -> torch.Tensor:
    """ReLU(conv1_1) of one frame, [C0,h,w] of ``dtype``."""
    return _conv(trunk_input(frame, normalize, dtype), params, 0, dtype)[0]


def features(frame, params, normalize: bool = True, dtype=torch.float64):
    """The five taps of one frame, [C_k,h_k,w_k] each, of ``dtype``."""
    x, i, taps = trunk_input(frame, normalize, dtype), 0, []
    for k, convs in enumerate(STAGES):
        if k:
            x = F.max_pool2d(x, 2, 2)
        for _ in range(convs):
            x = _conv(x, params, i, dtype)
            i += 1
        taps.append(x[0])
    return taps


def layer_distance(A, B, lin) -> float:
    """d_k of two taps [C,h,w] (any float type; everything from here on is fp64) and lin [C]."""
    A, B = A.to(torch.float64), B.to(torch.float64)
    lin = torch.from_numpy(np.array(lin, dtype=np.float64))
    nA = A / (torch.sqrt((A * A).sum(dim=0, keepdim=True)) + 1e-10)
    nB = B / (torch.sqrt((B * B).sum(dim=0, keepdim=True)) + 1e-10)
    return float(((lin[:, None, None] * (nA - nB) ** 2).sum(dim=0)).mean())


def layers(a, b, params, normalize: bool = True, trunk_dtype=torch.float64) -> np.ndarray:
    """fp64 [5]: the layer distances of result ``a`` and ground truth ``b`` (uint8 [h,w], possibly of different sizes)."""
    a, b = common(a, b)
    fa, fb = features(a, params, normalize, trunk_dtype), features(b, params, normalize, trunk_dtype)
    return np.array([layer_distance(fa[k], fb[k], params.lins[k]) for k in range(5)], dtype=np.float64)


def total(d) -> float:
    d = np.asarray(d, dtype=np.float64)
    return float((((d[..., 0] + d[..., 1]) + d[..., 2]) + d[..., 3]) + d[..., 4])


def lpips(a, b, params, normalize: bool = True, trunk_dtype=torch.float64) -> float:
    return total(layers(a, b, params, normalize, trunk_dtype))
