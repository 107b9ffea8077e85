"""The exact-operand cases of ``bf16_exact_cases.py`` without a GPU: every case of every table meets the precondition under which
fp32 accumulation is exact, its expected outputs exercise rounding (at least 5 % are not bf16 values) and ties (at least 50 in
each direction), and the checker catches planted errors.  These are conditions on the INPUTS of ``test_bf16_exact_gpu.py``,
not on the code under test: a case that misses one gets another grid or seed, never another condition.  (They do not apply to
the weight gradient, whose fp32 outputs are exact integers, nor to the statistics cases: per channel the sum of z^2 must stay
below 2^24 units, and a value that needs rounding is at least 257 units, so an exact sum of squares has room for at most 254
of them among thousands of voxels; those cases store small integers, and the rounding of that store is the forward table's.)"""
import pytest
import torch

import bf16_exact_cases as X

MIN_ROUNDED, MIN_TIES = 0.05, 50


def _check_profile(y64, name):
    share, up, down = X.rounding_profile(y64)
    assert share >= MIN_ROUNDED, f"{name}: only {share:.1%} of the expected outputs need rounding"
    assert up >= MIN_TIES and down >= MIN_TIES, f"{name}: {up} / {down} exact ties (even neighbour larger / smaller)"


@pytest.mark.parametrize("case", X.FORWARD_CASES, ids=[c.name for c in X.FORWARD_CASES])
def test_forward_case_is_exact_in_fp32_and_exercises_rounding(case):
    ops = X.forward_operands(case)
    y, total = X.forward_reference(case, *ops)
    X.assert_exact_in_fp32(X.FORWARD_Q, total, *ops)
    X.assert_faces_nonzero(ops[0], f"{case.name}: x")
    X.rne_bf16(y)
    _check_profile(y, case.name)


@pytest.mark.parametrize("case", X.DGRAD_CASES, ids=[c.name for c in X.DGRAD_CASES])
def test_input_gradient_case_is_exact_in_fp32_and_exercises_rounding(case):
    w, dz = X.dgrad_operands(case)
    dx, total, reached = X.dgrad_reference(case, w, dz)
    X.assert_exact_in_fp32(X.DGRAD_Q, total, w, dz)
    X.assert_faces_nonzero(dz, f"{case.name}: dz")
    assert bool((dx[~reached] == 0).all())
    X.rne_bf16(dx)
    _check_profile(dx, case.name)


@pytest.mark.parametrize("case", X.WGRAD_CASES, ids=[c.name for c in X.WGRAD_CASES])
def test_weight_gradient_case_is_exact_in_fp32(case):
    x, dz = X.wgrad_operands(case)
    dw, total = X.wgrad_reference(case, x, dz)
    X.assert_exact_in_fp32(X.WGRAD_Q, total, x, dz)
    X.assert_faces_nonzero(x, f"{case.name}: x")
    X.assert_faces_nonzero(dz, f"{case.name}: dz")
    assert torch.equal(dw.float().double(), dw) and torch.equal(dw.round(), dw)
    assert float(dw.abs().max()) > 0


@pytest.mark.parametrize("case", X.STATS_CASES, ids=[c.name for c in X.STATS_CASES])
def test_statistics_case_keeps_both_sums_exact(case):
    """Per channel, in the channel's unit (its weight scale): sum |z| and sum z^2 of the STORED values stay below 2^24, so every
    fp32 partial sum of the epilogue -- in lane, across lanes, across waves -- is exact.  The rounding conditions are not asked of
    these cases ("exact operands": a sum of squares below 2^24 leaves no room for values that need rounding; the
    forward table carries the rounding, and the GPU test ties the two stores together).  The thinned weights must still let a
    lost border voxel show: the faces of x are non-zero, and every tap carries a non-zero weight in at least half of the output
    channels."""
    x, w, scale = X.stats_operands(case)
    z, total = X.stats_reference(case, x, w, scale)
    X.assert_exact_in_fp32(1, total, x, w * scale.view(-1, 1, 1, 1, 1))
    X.assert_faces_nonzero(x, f"{case.name}: x")
    assert float((w != 0).any(dim=1).double().mean(dim=0).min()) >= 0.5, "a tap has zero weights in most output channels"
    stored = X.rne_bf16(z).double() / scale.view(1, -1, 1, 1, 1)
    assert torch.equal(stored.round(), stored)
    assert float(stored.abs().sum(dim=(0, 2, 3, 4)).max()) < 2.0 ** 24
    assert float((stored * stored).sum(dim=(0, 2, 3, 4)).max()) < 2.0 ** 24
    assert float((stored * stored).sum(dim=(0, 2, 3, 4)).min()) > 0


def test_the_full_size_weight_gradient_bound():
    """x, dz in {-2..2} over the 22 x 16 x 56 x 56 voxels of the benchmarked step: sum |terms| <= 4 * 1 103 872 < 2^24."""
    assert 4 * 22 * 16 * 56 * 56 < 2 ** 24


# ---- the checker catches planted errors ----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small_forward():
    case = X.FORWARD_CASES[9]                      # 5 x 32 -> 33 on 1 x 3 x 3: the smallest
    ops = X.forward_operands(case)
    y, _ = X.forward_reference(case, *ops)
    return case, ops, y


def test_checker_passes_the_reference_and_ignores_the_sign_of_zero(small_forward):
    _, _, y = small_forward
    want = X.rne_bf16(y)
    X.assert_same_values(want.clone(), want, y)
    X.assert_same_values(torch.tensor([-0.0, 1.0], dtype=torch.bfloat16), torch.tensor([0.0, 1.0], dtype=torch.bfloat16))


def test_checker_catches_one_element_on_the_neighbouring_code(small_forward):
    _, _, y = small_forward
    want = X.rne_bf16(y)
    got = want.clone()
    flat = got.view(-1).view(torch.int16)
    i = int((want.view(-1).float().abs() > 1).nonzero()[7])
    flat[i] += 1                                   # one code up in magnitude
    with pytest.raises(AssertionError, match="1 of"):
        X.assert_same_values(got, want, y, "planted")


def test_checker_catches_a_dropped_border_voxel(small_forward):
    case, (x, w, scale, shift, res), y = small_forward
    x2 = x.clone()
    assert x2[0, 0, 0, 0, 0] != 0
    x2[0, 0, 0, 0, 0] = 0
    y2, _ = X.forward_reference(case, x2, w, scale, shift, res)
    with pytest.raises(AssertionError, match="values differ"):
        X.assert_same_values(X.rne_bf16(y2), X.rne_bf16(y), y, "planted")


def test_checker_catches_ties_rounded_away_from_even(small_forward):
    _, _, y = small_forward
    _, up, down = X.rounding_profile(y)
    want, away = X.rne_bf16(y), X.ties_away_bf16(y)
    assert int((away.double() != want.double()).sum()) == down          # only the ties whose even neighbour is the smaller one move
    with pytest.raises(AssertionError, match=f"{down} of"):
        X.assert_same_values(away, want, y, "planted")


def test_bn_apply_reference_order_of_operations():
    """Identity coefficients return z; the residual is added before the ReLU and the rounding comes last: 3 + 2^-7 is not a
    bf16 value and ties to the even code 3."""
    z = torch.tensor([[-1.5, 0.25, 3.0]], dtype=torch.float64)
    one, zero = torch.ones(3, dtype=torch.float64), torch.zeros(3, dtype=torch.float64)
    assert torch.equal(X.bn_apply_reference(z, one, zero, None, False).double(), z)
    r = torch.tensor([[2.0, -1.0, 2.0 ** -7]], dtype=torch.float64)
    y = X.bn_apply_reference(z, one, zero, r, True)
    assert y.dtype == torch.bfloat16 and y.tolist() == [[0.5, 0.0, 3.0]]
