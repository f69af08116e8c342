"""Write tests/golden/train_batch_ra_ref.npz from the REAL reference's random-access training transforms (run once, on the CPU; no test
runs it).

    python tools/gen_train_batch_ra_fixture.py --reference DIR

The random-access twin of tools/gen_train_batch_fixture.py, whose dimensions, crop origins, scripted draws and runner it uses: it
imports DIR/opt/data_RA_bi.py, builds one synthetic sample of seven frames, H = 12, W = 16, and runs
``RandomCrop(8) -> Augment() -> ToTensor()`` plus the training script's ``permute`` and ``/32`` (train_RA_37.py:383-386) for all eight
flag combinations at two crop origins.  Both lists' reference components are drawn from -99 (the marker of a block without a reference
in that list, twice as likely as any other value), 0 and distances of both signs, over a lattice of zero vectors, so the outputs hold
the four marker classes, infinities and negative zeros and no NaN; the script asserts all of that before it writes.  The file holds
data only: the inputs, both fields, the plans (rows as ``ClipSet.batch`` takes them) and the seven outputs per case."""
import argparse
import importlib
import os

import numpy as np

import gen_train_batch_fixture as G

REFS = (-99, -99, 0, 1, 2, 3, -1, -2, 4, 8)


def _sample(rs):
    d = dict(lr=rs.randint(0, 256, (7, G.H, G.W)).astype(np.uint8), pms=rs.randint(0, 256, (7, G.H, G.W)).astype(np.uint8),
             rms=rs.randint(-128, 128, (7, G.H, G.W)).astype(np.int8), ufs=rs.randint(0, 256, (7, G.H + 2, G.W)).astype(np.uint8),
             hr=rs.randint(0, 256, (1, 4 * G.H, 4 * G.W)).astype(np.uint8))
    for name in ("mvl0", "mvl1"):
        mv = rs.randint(-128, 128, (1, G.H, G.W, 3)).astype(np.int8)
        mv[..., 2] = rs.choice(REFS, size=(1, G.H, G.W))
        mv[0, ::3, ::2, :2] = 0                                    # zero vectors, under every kind of reference component
        d[name] = mv
    return d


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden",
                                                  "train_batch_ra_ref.npz"))
    args = ap.parse_args()
    G._import_reference(args.reference)                            # stubs the file reader's imports, puts DIR on the path
    ref = importlib.import_module("opt.data_RA_bi")
    d = _sample(np.random.RandomState(5))
    plans, outs = [], {}
    for top, left in G.ORIGINS:
        for bits in range(8):
            hf, vf, rot = bits & 1, (bits >> 1) & 1, (bits >> 2) & 1
            plans.append((0, 0, top, left, hf, vf, rot, 0))
            with np.errstate(divide="ignore", invalid="ignore"):
                for k, v in G._run(ref, {k: v.copy() for k, v in d.items()}, top, left, (hf, vf, rot)).items():
                    outs.setdefault(k, []).append(v.contiguous().numpy().astype(np.float32)[0])
    out = {"out_" + k: np.stack(v) for k, v in outs.items()}
    mvs = out["out_mvs0"]
    assert np.isinf(mvs).any() and not np.isnan(mvs).any() and ((mvs == 0) & np.signbit(mvs)).any()
    assert np.array_equal(mvs.view(np.uint32), out["out_mvs1"].view(np.uint32))
    for top, left in G.ORIGINS:                                    # every window holds the four marker classes
        no0, no1 = (d[k][0, top:top + G.CROP, left:left + G.CROP, 2] == -99 for k in ("mvl0", "mvl1"))
        assert {(a, b) for a, b in zip(no0.ravel().tolist(), no1.ravel().tolist())} == {(x, y) for x in (False, True) for y in (False, True)}
    np.savez_compressed(args.out, plans=np.array(plans, np.int32), crop=np.int32(G.CROP), **{"in_" + k: v for k, v in d.items()}, **out)
    print(args.out, os.path.getsize(args.out), "bytes")


if __name__ == "__main__":
    main()
