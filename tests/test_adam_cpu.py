"""The device Adam without a GPU: a numpy fp32 restatement of csrc/adam.hip's three kernels (chunks, fp64 norm partials, the skip, the
clip, the update on views inside NaN-filled buffers) with switchable defects.  The defect-free form is within the bound of every case
of tests/adam_ref.py; every defect misses at least one, so the cases and the bound can tell the kernels' plausible mistakes.  Also
`optim.chunk_table`, the state file's helpers and the errors of ``fit(resume=...)`` that need no device."""
import math
import os

import numpy as np
import pytest
import torch

import adam_ref as ref

DEFECTS = ["bc_step_minus_1", "bc2_no_sqrt", "eps_in_root", "wd_after_moments", "coef_after_wd", "coef_unclamped", "norm_no_tail",
           "step_on_skip", "moments_on_skip", "drop_last_float4", "unaligned_offset"]
F = np.float32


def _update(p, g, m, v, k, defect):
    """The five lines on fp32 arrays; k: the step's fp32 constants."""
    if defect == "coef_after_wd":
        g = k["coef"] * (g + k["wd"] * p)
    elif defect == "wd_after_moments":
        g = k["coef"] * g
    else:
        g = k["coef"] * g
        g = g + k["wd"] * p
    m = m + k["b1c"] * (g - m)
    v = k["b2"] * v + k["b2c"] * g * g
    if defect == "eps_in_root":
        denom = np.sqrt(v * k["ib"] * k["ib"] + k["eps"])
    else:
        denom = np.sqrt(v) * k["ib"] + k["eps"]
    p = p - k["step_size"] * (m / denom)
    if defect == "wd_after_moments":
        p = p - k["lr"] * k["wd"] * p
    return p.astype(F), m.astype(F), v.astype(F)


def adam32(name, defect=None):
    """The case through the restatement -> (p, m, v lists, step, skipped, guards intact)."""
    from cdfo_amd.optim import chunk_table
    x = ref.inputs(name)
    sizes = [a.size for a in x["p"]]
    offsets, chunks, total = chunk_table(sizes, ref.CHUNK)
    starts = [ref.GUARD + (1 if t == ref.ODD else 0) for t in range(len(sizes))]
    pbuf = [np.full(n + 2 * ref.GUARD + 1, np.nan, F) for n in sizes]
    for b, s, a in zip(pbuf, starts, x["p"]):
        b[s:s + a.size] = a
    m, v = np.zeros(total, F), np.zeros(total, F)
    for o, mi, vi in zip(offsets, x["m"], x["v"]):
        m[o:o + mi.size], v[o:o + vi.size] = mi, vi
    step, skipped = x["step0"], 0
    b1, b2 = ref.BETAS
    for grads in ([ref.poisoned(x["g"])] if x["skip_first"] else []) + [x["g"]]:
        gbuf = [np.full(n + 2 * ref.GUARD + 1, np.nan, F) for n in sizes]
        for b, s, a in zip(gbuf, starts, grads):
            b[s:s + a.size] = a
        partials = []
        for t, first in chunks:
            cnt = min(ref.CHUNK, sizes[t] - first)
            if defect == "norm_no_tail":
                cnt -= cnt % 4
            partials.append(float(np.square(gbuf[t][starts[t] + first:starts[t] + first + cnt].astype(np.float64)).sum()))
        total_sq = 0.0
        for s in partials:
            total_sq += s
        skip = not math.isfinite(total_sq)
        if skip:
            skipped += 1
            if defect == "step_on_skip":
                step += 1
            if defect != "moments_on_skip":
                continue
        norm = math.sqrt(total_sq) if total_sq >= 0 else float("nan")
        coef = 1.0
        if x["max_norm"] > 0 and (not norm <= x["max_norm"] or defect == "coef_unclamped"):
            coef = x["max_norm"] / (norm + 1e-6)
        if not skip:
            step += 1
        tb = np.float64(step - 1 if defect == "bc_step_minus_1" else step)
        with np.errstate(all="ignore"):
            bc2 = 1.0 - np.float64(b2) ** tb
            k = dict(coef=F(coef), wd=F(x["wd"]), b1c=F(1.0 - b1), b2=F(b2), b2c=F(1.0 - b2), eps=F(ref.EPS), lr=F(ref.LR),
                     step_size=F(np.float64(ref.LR) / (1.0 - np.float64(b1) ** tb)),
                     ib=F(1.0 / bc2 if defect == "bc2_no_sqrt" else 1.0 / np.sqrt(bc2)))
            for t, first in chunks:
                cnt = min(ref.CHUNK, sizes[t] - first)
                todo = np.ones(cnt, bool)
                if defect == "drop_last_float4" and cnt >= 4:
                    todo[4 * (cnt // 4 - 1):4 * (cnt // 4)] = False
                base = starts[t] - (starts[t] % 4 if defect == "unaligned_offset" else 0) + first
                sl, ms = slice(base, base + cnt), slice(offsets[t] + first, offsets[t] + first + cnt)
                pn, mn, vn = _update(pbuf[t][sl], gbuf[t][sl], m[ms], v[ms], k, defect)
                if skip:                                               # (the moments_on_skip defect: p is spared, m and v are not)
                    m[ms], v[ms] = np.where(todo, mn, m[ms]), np.where(todo, vn, v[ms])
                else:
                    pbuf[t][sl], m[ms], v[ms] = np.where(todo, pn, pbuf[t][sl]), np.where(todo, mn, m[ms]), np.where(todo, vn, v[ms])
    guards = all(np.isnan(b[:s]).all() and np.isnan(b[s + n:]).all() for b, s, n in zip(pbuf, starts, sizes))
    return ([b[s:s + n] for b, s, n in zip(pbuf, starts, sizes)], [m[o:o + n] for o, n in zip(offsets, sizes)],
            [v[o:o + n] for o, n in zip(offsets, sizes)], step, skipped, guards)


def _passes(name, defect=None):
    p, m, v, step, skipped, guards = adam32(name, defect)
    want = ref.expected(name)
    ok, figures = ref.within_bound(name, p, m, v)
    return ok and guards and (step, skipped) == (want[3], want[4]), figures


def test_case_list_covers_what_the_checks_need():
    sizes = {n for c in ref.CASES for n in c["sizes"]}
    assert sizes >= {1, 3, 4, 5, 63, 65, ref.CHUNK - 1, ref.CHUNK, ref.CHUNK + 1, 3 * ref.CHUNK + 7}
    assert {c["gscale"] for c in ref.CASES} == {1e-6, 1e-3, 1.0, 1e3} and {c["step"] for c in ref.CASES} == {1, 2, 1000}
    assert {c["wd"] for c in ref.CASES} == {0.0, 1e-5} and all(len(c["sizes"]) == 7 for c in ref.CASES)
    for name in ref.CASE_NAMES:
        x = ref.inputs(name)
        zeros = sum(int((g == 0).sum()) for g in x["g"]) / sum(g.size for g in x["g"])
        assert 0.10 < zeros < 0.19 and max(float(np.abs(p).max()) for p in x["p"]) <= 1.0
        assert all(f > 0 for f in ref.floor(name)), (name, ref.floor(name))


@pytest.mark.parametrize("name", ref.CASE_NAMES)
def test_the_restatement_without_a_defect_is_within_every_bound(name):
    ok, figures = _passes(name)
    print(figures)
    assert ok, figures


@pytest.mark.parametrize("defect", DEFECTS)
def test_every_defect_misses_a_bound(defect):
    missed = [name for name in ref.CASE_NAMES if not _passes(name, defect)[0]]
    print(defect, "misses", missed)
    assert missed, f"no case of adam_ref sees the defect {defect}"


def test_statement_skips_and_clips():
    x = ref.inputs("g1_t1")
    for bad in (float("nan"), float("inf"), -float("inf")):
        p, m, v, step, skipped, _ = ref.adam_step_ref(x["p"], ref.poisoned(x["g"], bad), x["m"], x["v"], 5, 2)
        assert (step, skipped) == (5, 3) and all(np.array_equal(a, b) for a, b in zip(p + m + v, x["p"] + x["m"] + x["v"]))
    assert ref.clip_coefficient(2.0, 0.0) == 1.0 and ref.clip_coefficient(2.0, 2.0) == 1.0 and ref.clip_coefficient(2.0, 3.0) == 1.0
    assert ref.clip_coefficient(2.0, 1.0) == float(np.float32(1.0 / (2.0 + 1e-6)))


@pytest.mark.parametrize("chunk", [4, 8, 64, 4096])
def test_chunk_table_covers_every_element_once(chunk):
    from cdfo_amd.optim import chunk_table
    sizes = [1, chunk - 1, chunk, chunk + 1, 3, 3 * chunk + 7, 2, 1]
    offsets, chunks, total = chunk_table(sizes, chunk)
    assert offsets.dtype == np.int64 and chunks.dtype == np.int32 and chunks.shape[1] == 2
    assert all(o % 4 == 0 for o in offsets) and total % 4 == 0 and offsets[0] == 0
    assert all(offsets[t] + sizes[t] <= (offsets[t + 1] if t + 1 < len(sizes) else total) for t in range(len(sizes)))
    seen = [np.zeros(n, int) for n in sizes]
    for t, first in chunks:
        assert first % chunk == 0 and 0 <= first < sizes[t]
        seen[t][first:first + chunk] += 1
    assert all((s == 1).all() for s in seen)
    assert len(chunks) == sum(-(-n // chunk) for n in sizes)
    assert [tuple(r) for r in chunks] == sorted(tuple(r) for r in chunks)               # tensor by tensor, in element order


def test_chunk_table_refuses_what_it_cannot_lay_out():
    from cdfo_amd.optim import chunk_table
    for sizes, chunk in (([], 4096), ([0], 4096), ([-1], 4096), ([4], 6), ([4], 0), ([2 ** 31], 4096), ([True], 4096)):
        with pytest.raises(ValueError):
            chunk_table(sizes, chunk)


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="invented device addresses: where a GPU is present, tests/test_gpu_adam_kernels.py "
                    "makes these checks with real allocations, and a regressed check could not launch on them")
def test_entry_points_refuse_bad_arguments_without_a_gpu():
    import ctypes as C
    from cdfo_amd import _lib
    lib = _lib.lib()
    table = (C.c_longlong * 4)(64, 128, 0, 4)
    host, dev = C.addressof(table), 256
    assert lib.cdfo_grad_norm_partials(None, dev, 1, 512, 1, 1024, None) == -1
    assert lib.cdfo_grad_norm_partials(host, dev, 0, 512, 1, 1024, None) == -1          # an empty table
    assert lib.cdfo_grad_norm_partials(host, dev, 1, 512, -1, 1024, None) == -1
    assert lib.cdfo_adam_step(host, dev, 1, 512, 1, 1024, 2048, 3, 4096, 0.9, 0.999, 1e-8, 0.0, None) == -1   # total not a multiple of 4
    table[2] = 2                                                                         # an offset that is not a multiple of 4
    assert lib.cdfo_grad_norm_partials(host, dev, 1, 512, 1, 1024, None) == -1
    assert lib.cdfo_adam_step(host, dev, 1, 512, 1, 1024, 2048, 8, 4096, 0.9, 0.999, 1e-8, 0.0, None) == -1
    table[2], table[3] = 0, -1                                                           # a negative size
    assert lib.cdfo_grad_norm_partials(host, dev, 1, 512, 1, 1024, None) == -1
    assert lib.cdfo_adam_scalars(None, 1, 1e-3, 0.9, 0.999, 0.0, 512, 1024, None) == -1
    assert lib.cdfo_adam_scalars(256, 0, 1e-3, 0.9, 0.999, 0.0, 512, 1024, None) == -1
    assert lib.cdfo_adam_scalars(256, 1, 1e-3, 1.0, 0.999, 0.0, 512, 1024, None) == -1


def test_generator_states_round_trip():
    from cdfo_amd.train import generator_states, set_generator_states
    rng = np.random.default_rng(4)
    rng.integers(0, 100, 7)
    torch.manual_seed(11)
    torch.rand(3)
    states = generator_states(rng)
    want = (rng.integers(0, 1 << 30, 5).tolist(), rng.permutation(9).tolist(), torch.rand(4), torch.randint(0, 99, (3,)))
    path = None
    import tempfile
    with tempfile.TemporaryDirectory() as td:
        path = os.path.join(td, "s.pth")
        torch.save({"generators": states}, path)
        back = torch.load(path)["generators"]                                            # torch.load's defaults read it
    other = np.random.default_rng(99)
    torch.manual_seed(5)
    set_generator_states(other, back)
    got = (other.integers(0, 1 << 30, 5).tolist(), other.permutation(9).tolist(), torch.rand(4), torch.randint(0, 99, (3,)))
    assert got[0] == want[0] and got[1] == want[1] and torch.equal(got[2], want[2]) and torch.equal(got[3], want[3])


def _state_file(tmp_path, run, epoch=2, weights=True):
    from cdfo_amd.train import generator_states, state_path
    os.makedirs(tmp_path / "ckpt", exist_ok=True)
    path = state_path(str(tmp_path), epoch)
    torch.save({"optimizer": {"step": 4, "skipped": 0, "exp_avg": [], "exp_avg_sq": []}, "optimizer_kind": "device", "epoch": epoch,
                "averages": [1.0, 0.5], "generators": generator_states(np.random.default_rng(4)), "run": run}, path)
    if weights:
        torch.save({}, str(tmp_path / "ckpt" / f"epoch-{epoch}.pth"))
    return path


def test_resume_refuses_another_run(tmp_path):
    from cdfo_amd.train import RUN_ARGUMENTS, read_state, run_arguments, weights_beside
    run = run_arguments(2, 8, 1e-4, 1e-5, 4, "LD", 0.0, 0.0, 1.0, None)
    assert tuple(run) == RUN_ARGUMENTS
    path = _state_file(tmp_path, run)
    assert weights_beside(path) == str(tmp_path / "ckpt" / "epoch-2.pth")
    state = read_state(path, dict(run), 4)
    assert state["epoch"] == 2 and state["averages"] == [1.0, 0.5] and state["weights"].endswith("epoch-2.pth")
    for name, other in (("batch_size", 3), ("crop", 16), ("lr", 2e-4), ("weight_decay", 0.0), ("seed", 5), ("coding", "RA"),
                        ("lpips_weight", 0.1), ("ffl_weight", 1.0), ("max_grad_norm", 1.0)):
        with pytest.raises(ValueError, match=rf"\b{name} = "):
            read_state(path, dict(run, **{name: other}), 4)
    with pytest.raises(ValueError, match="batch_size = "):                               # the first difference is the one named
        read_state(path, dict(run, batch_size=3, seed=5), 4)
    for epochs in (1, 2):
        with pytest.raises(ValueError, match="nothing to run"):
            read_state(path, dict(run), epochs)
    with pytest.raises(ValueError, match="state file"):
        read_state(str(tmp_path / "ckpt" / "epoch-2.pth"), dict(run), 4)
    with pytest.raises(ValueError, match="no state file"):
        read_state(str(tmp_path / "ckpt" / "epoch-9.state.pth"), dict(run), 4)
    lone = _state_file(tmp_path / "lone", run, weights=False)
    with pytest.raises(ValueError, match="weights .* missing"):
        read_state(lone, dict(run), 4)


def test_fit_refuses_bad_keywords_before_touching_anything(tmp_path):
    from cdfo_amd.train import fit

    class Clips:
        coding = "LD"
    for kw in (dict(optimizer="sgd"), dict(max_grad_norm=1.0), dict(optimizer="device", max_grad_norm=0.0),
               dict(optimizer="device", max_grad_norm=float("inf")), dict(optimizer="device", max_grad_norm=True),
               dict(resume=str(tmp_path / "ckpt" / "epoch-1.state.pth"), start_epoch=1),
               dict(resume=str(tmp_path / "ckpt" / "epoch-1.state.pth"))):
        with pytest.raises(ValueError):
            fit(None, Clips(), 2, str(tmp_path / "out"), **kw)
    assert not os.path.exists(tmp_path / "out")
