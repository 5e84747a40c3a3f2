"""One D0 train pass at 512 x 512, B = 2, with the short pixel tile (TUNE_SHORT_TILE) off and on: both losses and every parameter gradient
are torch.equal -- a tile shape does not enter the arithmetic -- and the step really takes the short-tile instances with the knob on
(counted through ops.PROFILE's kernel names) and none with it off."""
import pytest
import torch

from tests.test_gpu_sparse_reg_grad import _model, _targets
from tests.test_gpu_wgrad_pair import _step

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('arith', ['f32_hf16x3_bwd_bf16x3', 'f32'])
def test_train_pass_is_bit_identical_and_takes_the_short_tile(arith):
    from efficientdet.pytorch_amd import ops, _lib as L
    from oracle import effdet_oracle as O
    m = _model(arith)
    img = O.synthetic_batch(2, 512, seed=2, num_classes=8)[0].cuda()
    ann = _targets('empty_and_eight').cuda()
    outs, short = [], []
    old = ops.tuning_set(L.TUNE_SHORT_TILE, 0)
    old_profile = ops.PROFILE
    try:
        for on in (0, 1):
            ops.tuning_set(L.TUNE_SHORT_TILE, on)
            ops.PROFILE = ops.LaunchProfile()
            outs.append(_step(m, img, ann))
            names = [r[0] for r in ops.PROFILE.records]
            short.append(sum(1 for n in names if n.startswith('conv_igemm_kernel<') and ',short' in n))
            assert all(n.startswith('conv_') for n in names if 'igemm' in n)
    finally:
        ops.PROFILE = old_profile
        ops.tuning_set(L.TUNE_SHORT_TILE, old)
    print('short-tile launches per pass (%s): off %d, on %d' % (arith, short[0], short[1]))
    assert short[0] == 0 and short[1] > 0
    a, b = outs
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert a[2].keys() == b[2].keys() and len(a[2]) == 274
    bad = [k for k in a[2] if not torch.equal(a[2][k], b[2][k])]
    assert not bad, bad[:8]
