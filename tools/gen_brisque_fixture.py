"""Write tests/golden/brisque_ref.npz from the REAL reference's BRISQUE (run once, on the CPU; no test runs it).

    python tools/gen_brisque_fixture.py --reference DIR [--model-out FILE]

Imports DIR/metric/brisque.py (torch and PIL) and runs ``brisque(x)`` the way its docstring says, x [1,3,H,W] RGB in [0,1] with
R = G = B = u / 255, with DIR/metric/weight/brisque_svm_weights.pth, on five seeded 8-bit frames, blurred noise plus white noise
scaled to 0 .. 255 (the generator of tools/gen_niqe_fixture.py); a sixth, all zeros, is stored without reference output, since the
reference asserts on it:

    a  16 x 16    the minimum; one tile, one strip; scale 2 is 8 x 8
    b  37 x 83    both sizes odd, half image 19 x 42, ragged tiles
    c  70 x 130   several strips and tiles, so the circular partners cross workgroups in both directions; sizes 2 mod 4
    d  70 x 130   a second frame of c's size (the GPU tests launch c, d and z together)
    z  70 x 130   all zeros
    e  96 x 160   contrast stretched so that large areas clip at 0 and 255

The model is recorded from the running reference and typed nowhere: the support vectors and their coefficients through
``torch.load``, the 36 feature ranges from the list ``scale_features`` hands to ``torch.tensor``, gamma from the call of
``rbf_kernel`` and rho from the subtraction behind it (a tensor subclass sees the scalar).  Per frame the reference's 36 features are
hooked at ``scale_features``' input and the luma it saw at ``natural_scene_statistics``' first call; the luma is asserted equal to u,
and each of the ten table indices (the alphas' places in the table) equal to the numpy statement's (tests/brisque_ref.py): a search on
a near-tie belongs in no parity fixture -- change the frame's seed or gain, not the statement.

The file holds data only.  ``--model-out FILE`` also writes the model alone, in the format `cdfo_amd.metrics.brisque_params` reads
(sv [n,36], sv_coef [n], feature_ranges [36,2], gamma, rho; fp64): a user's own model file, which is not committed."""
import argparse
import importlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from gen_niqe_fixture import _frame  # noqa: E402  (tools/ is this script's directory)

def frames():
    rs = np.random.RandomState(36)
    f = dict(a=_frame(rs, 16, 16), b=_frame(rs, 37, 83), c=_frame(rs, 70, 130), d=_frame(rs, 70, 130), e=_frame(rs, 96, 160, 2.5))
    f["z"] = np.zeros((70, 130), np.uint8)
    return f


class _Spy(torch.Tensor):
    """A tensor that notes the Python scalars of the operations it takes part in."""
    seen = []

    @classmethod
    def __torch_function__(cls, func, types, args=(), kwargs=None):
        cls.seen.append((getattr(func, "__name__", str(func)), [a for a in args if isinstance(a, float)]))
        return super().__torch_function__(func, types, args, kwargs or {})


class _Torch:
    """The torch module as the reference sees it, with ``tensor`` noting the nested lists it is given."""

    def __init__(self):
        self.lists = []

    def __getattr__(self, name):
        return getattr(torch, name)

    def tensor(self, data, *a, **k):
        if isinstance(data, list):
            self.lists.append(data)
        return torch.tensor(data, *a, **k)


def write_model(path, held):
    """The model alone, fp64, under the five keys `cdfo_amd.metrics.brisque_params` reads."""
    np.savez(path, **{k: np.asarray(held[k], np.float64) for k in ("sv", "sv_coef", "feature_ranges", "gamma", "rho")})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True)
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "brisque_ref.npz"))
    ap.add_argument("--model-out")
    args = ap.parse_args()
    sys.path.insert(0, args.reference)
    ref = importlib.import_module("metric.brisque")
    import brisque_ref as st
    weights = os.path.join(args.reference, "metric", "weight", "brisque_svm_weights.pth")
    sv_coef, sv = torch.load(weights)
    out = dict(sv=sv.numpy().copy(), sv_coef=sv_coef.numpy().reshape(-1).copy())
    assert out["sv"].ndim == 2 and out["sv"].shape[1] == 36 and out["sv_coef"].shape == (out["sv"].shape[0],), (sv.shape, sv_coef.shape)
    seen = dict(features=[], luma=[], gamma=[])
    spy_torch = _Torch()
    ref.torch = spy_torch
    inner_scale, inner_nss, inner_rbf = ref.scale_features, ref.natural_scene_statistics, ref.rbf_kernel

    def scale_features(features):
        seen["features"].append(features.numpy().copy())
        return inner_scale(features)

    def natural_scene_statistics(luma, *a, **k):
        seen["luma"].append(luma.numpy().copy())
        return inner_nss(luma, *a, **k)

    def rbf_kernel(features, sv, gamma):
        seen["gamma"].append(gamma)
        return inner_rbf(features=features, sv=sv, gamma=gamma).as_subclass(_Spy)

    ref.scale_features, ref.natural_scene_statistics, ref.rbf_kernel = scale_features, natural_scene_statistics, rbf_kernel
    tab = st.table()
    gam = tab[0]
    for name, u in frames().items():
        out["frame_" + name] = u
        if name == "z":
            continue
        for v in seen.values():
            del v[:]
        del _Spy.seen[:], spy_torch.lists[:]
        x = torch.from_numpy(u.astype(np.float32) / np.float32(255.0))[None, None].repeat(1, 3, 1, 1)
        with torch.no_grad():
            s = ref.brisque(x, pretrained_model_path=weights)
        s = float(torch.Tensor(s).reshape(-1)[0]) if isinstance(s, torch.Tensor) else float(s)
        assert len(seen["features"]) == 1 and len(seen["luma"]) == 2 and len(seen["gamma"]) == 1 and np.isfinite(s), name
        luma = seen["luma"][0][0, 0]
        assert luma.shape == u.shape and np.array_equal(luma.astype(np.float64), u.astype(np.float64)), name   # the luma IS the frame
        F = seen["features"][0].reshape(36).astype(np.float64)
        ranges = [l for l in spy_torch.lists if np.shape(l) == (36, 2)]
        subs = [a for f, a in _Spy.seen if "sub" in f and a]
        assert len(ranges) == 1 and len(subs) == 1 and len(subs[0]) == 1, (name, len(ranges), _Spy.seen)
        model = dict(feature_ranges=np.array(ranges[0], np.float64), gamma=np.float64(seen["gamma"][0]), rho=np.float64(subs[0][0]))
        for k, v in model.items():
            assert k not in out or np.array_equal(out[k], v), k
            out[k] = v
        p = st.pieces(u, tab)
        index = np.searchsorted(gam, F[list(st.ALPHAS)])
        assert np.array_equal(gam[index], F[list(st.ALPHAS)]), name                      # the reference's alphas are table entries
        assert np.array_equal(index, p["index"].reshape(-1)), (name, index, p["index"].reshape(-1), p["gap"])
        as_ref = (out["sv"], out["sv_coef"]) + tuple(np.asarray(out[k]).astype(np.float32).astype(np.float64)
                                                      for k in ("feature_ranges", "gamma", "rho"))
        rel = np.abs(p["features"] - F) / np.abs(F)
        out["luma_" + name], out["features_" + name], out["score_" + name] = luma.astype(np.uint8), F, np.float64(s)
        print(name, u.shape, "clipped %.2f" % np.mean((u == 0) | (u == 255)), "score %.6f" % s, "statement %.6f" % st.score(p["features"], *as_ref),
              "features worst %.2e relative" % rel.max(), "smallest gap %.2e" % p["gap"].min())
    pz = st.pieces(out["frame_z"], tab)
    assert np.isnan(pz["features"]).any() and (pz["index"] == 0).all()
    np.savez_compressed(args.out, **out)
    print(args.out, os.path.getsize(args.out), "bytes;", out["sv"].shape[0], "support vectors")
    if args.model_out:
        write_model(args.model_out, out)
        print(args.model_out, "written")


if __name__ == "__main__":
    main()
