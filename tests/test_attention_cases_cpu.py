"""Do the attention tests' inputs and tolerances bite?  (No GPU.)

tests/test_gpu_attention.py compares the kernels with fp64 references on the inputs of attn_cases.py, within the tolerances
of attn_cases.py.  Here DEFECTIVE fp64 computations -- the mistakes such kernels make -- are put through the same inputs and
the same tolerance functions and must miss them by a wide margin, so that nobody can soften an input family or a tolerance
without this file noticing.  Only the CPU reference stands on the passing side: no emulation of the correct arithmetic is
asserted to pass.  The preconditions of the GPU tests that need no GPU (the near-tie distance of the mask inputs, the
known-answer vectors of the Philox implementation the generator contract is checked with) are asserted here as well."""
import numpy as np
import pytest
import torch

import attn_cases as AC

TAIL_LENGTHS = [L for L in AC.SEQ_LENGTHS if L % 32 and L > 1]
SWAP_LENGTHS = [L for L in AC.SEQ_LENGTHS if L > 1]


def _ratios(bad, family, mode10, H, W):
    """error / tolerance of a defective result under the three-pass rule and under the PV1 bound."""
    q, v, ref, pav = AC.seq_case(family, mode10, 2, H, W)
    L, vmax = AC.seq_len(mode10, H, W), v.abs().max().item()
    return AC.seq_ratio(bad, ref, pav, mode10, L, vmax), AC.seq_ratio(bad, ref, pav, 20 + mode10, L, vmax)


@pytest.mark.parametrize("L", TAIL_LENGTHS)
@pytest.mark.parametrize("mode10", [0, 1])
def test_an_unmasked_tail_breaks_both_tolerances(L, mode10):
    """Defect (i): the masked keys of the last 32-key sub-tile (copies of key L - 1, as the kernel loads them) take part in
    the softmax.  On the `spread` inputs it misses the three-pass tolerance and the PV1 bound by more than 10x at every
    tested key count with a partial last sub-tile.  L = 1 is no such case and is left out: every key is then the same key,
    and the softmax of copies returns v_0 whatever is masked -- L = 8 is the smallest sequence that can show the defect.

    Why `spread` exists: under `peaked` (q = 0.5 randn) the median self-weight is 1.000, the attention is one-hot, and the
    MEDIAN output element moves by less than the tolerance under this defect (fp64, rows of 8 / 37 / 272 / 490 keys: median
    shift 4e-6 / 4e-6 / 2e-6 / 3e-6 against a tolerance of 8e-5 - 1e-4; the maximum still shows it, in a few outlier queries).
    Under `spread` the median self-weight is 0.37 / 0.10 / 0.015 / 0.008 and the median element moves by 0.47 / 0.23 / 0.036 /
    0.027."""
    H, W = AC.seq_shape(mode10, L)
    q, v, _, _ = AC.seq_case("spread", mode10, 2, H, W)
    three, pv1 = _ratios(AC.seq_ref_unmasked_tail(q, v, mode10), "spread", mode10, H, W)
    assert three >= 10.0 and pv1 >= 10.0, (three, pv1)


def test_peaked_inputs_hide_an_unmasked_tail_from_the_median_element():
    """The figures of the docstring above, kept true: the median element's shift, relative to the three-pass tolerance, is
    under 1 with `peaked` and over 10 with `spread` at the same shape."""
    med = {}
    for family in ("peaked", "spread"):
        q, v, ref, _ = AC.seq_case(family, 0, 2, AC.OTHER, 37)
        med[family] = (AC.seq_ref_unmasked_tail(q, v, 0) - ref).abs().median().item() / AC.tol_three_pass(ref)
    assert med["peaked"] < 1.0 and med["spread"] > 10.0, med


@pytest.mark.parametrize("L", SWAP_LENGTHS)
@pytest.mark.parametrize("mode10", [0, 1])
def test_two_exchanged_values_break_both_tolerances(L, mode10):
    """Defect (ii): the values of keys 0 and 1 exchanged, a slot-order error of the transposed V staging.  `spread` inputs."""
    H, W = AC.seq_shape(mode10, L)
    q, v, _, _ = AC.seq_case("spread", mode10, 2, H, W)
    three, pv1 = _ratios(AC.seq_ref_swapped_values(q, v, mode10), "spread", mode10, H, W)
    assert three >= 10.0 and pv1 >= 10.0, (three, pv1)


@pytest.mark.parametrize("H,W", AC.WINDOW_SHAPES)
def test_two_exchanged_values_break_the_window_tolerances(H, W):
    q, v, _, _ = AC.seq_case("spread", 2, 2, H, W)
    three, pv1 = _ratios(AC.seq_ref_swapped_values(q, v, 2, 9, 10), "spread", 2, H, W)
    assert three >= 10.0 and pv1 >= 10.0, (three, pv1)


TIE_SHAPES = [(0, 3, 37), (1, 37, 3), (2, 8, 16)]


@pytest.mark.parametrize("mode10,H,W", TIE_SHAPES)
def test_two_roundings_of_the_query_split_break_the_three_pass_tolerance(mode10, H, W):
    """Defect (iv): hi of the scaled query rounded twice, from the exact and from the fp32 product.  On random inputs it shows
    in one element of 8192 only (which is how `offset` at 37 keys found it in the MFMA kernel, at 2.2x the tolerance); on the
    tie inputs, where most elements are exact fp16 ties, it misses the three-pass tolerance by more than 10x.  (It stays
    inside the PV1 bound, which allows 2^-10 relative: modes 20-22 cannot see it and do not need to.)"""
    q, v, ref, pav, share = AC.tie_case(mode10, 2, H, W)
    assert share > 0.5, share
    bad = AC.seq_ref_two_roundings_of_hi(q, v, mode10)
    assert AC.seq_ratio(bad, ref, pav, mode10, AC.seq_len(mode10, H, W), v.abs().max().item()) >= 10.0


# ------------------------------------------------------------------------------------------------------------ rdab_prep
@pytest.mark.parametrize("B,H,W", AC.RDAB_SHAPES)
def test_rdab_inputs_keep_clear_of_the_threshold_and_mask_both_ends(B, H, W):
    """Preconditions of the exact-mask demand: no softmax within 1e-5 of 0.5 (the kernel decides in fp32), no zero q (the
    mask is recovered as qwin == 0).  And the inputs do what they are for: a good share of the pixels has a masked channel,
    channels 0 and 63 among them, so the channel conv's zero padding meets non-zero neighbours at both ends."""
    xq, vmax, u, wW, bW = AC.rdab_inputs(B, H, W)
    assert AC.rdab_tie_distance(vmax, u) > 1e-5
    assert (xq[..., :64] != 0).all() and 0.0 < u.min().item() and u.max().item() < 1.0
    mask = AC.rdab_ref(xq, vmax, u, wW, bW)["mask"]
    share = mask.amax(-1).mean().item()
    assert 0.15 < share < 0.6, share
    assert mask[..., 0].sum() >= 1 and mask[..., 63].sum() >= 1, (mask[..., 0].sum(), mask[..., 63].sum())


@pytest.mark.parametrize("B,H,W", AC.RDAB_SHAPES)
def test_flipped_taps_and_a_shifted_threshold_break_the_rdab_checks(B, H, W):
    """Defect (iii).  Taps reversed: sq and vrow leave the tolerance, the mask is untouched.  Threshold 0.45: the mask differs."""
    xq, vmax, u, wW, bW = AC.rdab_inputs(B, H, W)
    want = AC.rdab_ref(xq, vmax, u, wW, bW)
    bad = AC.rdab_ref(xq, vmax, u, wW, bW, flip_taps=True)
    r = AC.rdab_check(bad["sq"], bad["vrow"], bad["qwin"], want)
    assert r["mask_mismatches"] == 0 and r["sq"] >= 10.0 and r["vrow"] >= 10.0, r
    with pytest.raises(AssertionError):
        AC.rdab_assert(bad["sq"], bad["vrow"], bad["qwin"], want)
    bad = AC.rdab_ref(xq, vmax, u, wW, bW, threshold=0.45)
    r = AC.rdab_check(bad["sq"], bad["vrow"], bad["qwin"], want)
    assert r["mask_mismatches"] >= 1 and r["qwin"] > 0.0, r
    with pytest.raises(AssertionError):
        AC.rdab_assert(bad["sq"], bad["vrow"], bad["qwin"], want)


def test_philox_known_answers():
    """The NumPy Philox4x32-10 against Random123's three known-answer vectors, one at a time and as one array call."""
    for ctr, key, want in AC.PHILOX_KAT:
        assert tuple(int(x) for x in AC.philox4x32_10(*ctr, *key)) == want
    cols = [np.array(c, dtype=np.uint64) for c in zip(*[ctr + key for ctr, key, _ in AC.PHILOX_KAT])]
    got = np.stack(AC.philox4x32_10(*cols), axis=1)
    assert (got == np.array([w for _, _, w in AC.PHILOX_KAT], dtype=np.uint64)).all()


def test_rdab_noise_layout():
    """rdab_noise places word c & 3 of counter (p, b, c >> 2, draw) at [b, c, p], on the open grid (k + 0.5) 2^-24."""
    seed, draw = 0x299F31D0A4093822, 5
    u = AC.rdab_noise(2, 64, seed, draw)
    assert tuple(u.shape) == (2, 64, 64) and u.dtype == torch.float32
    for b, c, p in ((0, 0, 0), (1, 63, 63), (1, 6, 17)):
        word = int(AC.philox4x32_10(p, b, c >> 2, draw, seed & 0xFFFFFFFF, seed >> 32)[c & 3])
        assert u[b, c, p].item() == float(np.float32(((word >> 8) + 0.5) * 2.0 ** -24))
    assert not torch.equal(u, AC.rdab_noise(2, 64, seed, draw + 1)) and not torch.equal(u, AC.rdab_noise(2, 64, seed + 1, draw))


# ------------------------------------------------------------------------------------------------------------- colconv9
@pytest.mark.parametrize("H", AC.COL_HEIGHTS)
def test_the_two_column_references_agree(H):
    """col_ref_taps (used where the tensor is too large for the conv2d form) is the same function as col_ref."""
    w, b = AC.col_weights()
    x = torch.randn(2, H, 5, 64, generator=torch.Generator().manual_seed(H))
    assert (AC.col_ref(x, w, b) - AC.col_ref_taps(x, w, b)).abs().max().item() < 1e-12
