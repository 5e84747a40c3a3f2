"""CPU tier: tests.gpu_util.assert_nonfinite_match, the comparison of the non-finite parity tests (tests/test_gpu_nonfinite.py), fails
where a kernel would be wrong about a NaN or an inf and passes where it is right."""
import pytest
import torch

from tests.gpu_util import assert_nonfinite_match

NAN, INF = float('nan'), float('inf')


def _ref():
    return torch.tensor([1.0, -2.0, NAN, INF, -INF, 0.5], dtype=torch.float64)


def test_matching_masks_and_values_pass():
    ref = _ref()
    got = ref.float().clone()
    got[0] = 1.0 + 1e-6
    got[2] = -NAN                               # (the sign and payload of a NaN are not part of the contract)
    assert_nonfinite_match(got, ref, 1e-4)
    assert_nonfinite_match(got, ref, 1e-4, exact=False)


@pytest.mark.parametrize('exact', [True, False])
def test_a_swallowed_nan_fails(exact):
    got = _ref().clone(); got[2] = 0.0                 # what fmaxf(NaN, 0) does
    with pytest.raises(AssertionError):
        assert_nonfinite_match(got, _ref(), 1e-4, exact=exact)


def test_a_nan_where_an_inf_belongs_fails_only_when_exact():
    got = _ref().clone(); got[3] = NAN
    with pytest.raises(AssertionError):
        assert_nonfinite_match(got, _ref(), 1e-4)
    assert_nonfinite_match(got, _ref(), 1e-4, exact=False)


def test_a_flipped_inf_sign_fails_only_when_exact():
    got = _ref().clone(); got[4] = INF
    with pytest.raises(AssertionError):
        assert_nonfinite_match(got, _ref(), 1e-4)
    assert_nonfinite_match(got, _ref(), 1e-4, exact=False)


@pytest.mark.parametrize('exact', [True, False])
def test_an_inf_where_a_finite_value_belongs_fails(exact):
    got = _ref().clone(); got[1] = -INF
    with pytest.raises(AssertionError):
        assert_nonfinite_match(got, _ref(), 1e-4, exact=exact)


def test_finite_elements_still_meet_the_tolerance():
    got = _ref().clone(); got[5] = 0.6
    with pytest.raises(AssertionError):
        assert_nonfinite_match(got, _ref(), 1e-4)
