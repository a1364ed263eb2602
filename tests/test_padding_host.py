"""Host: why the padding of the gradient buffer has to be exactly 0, not merely tiny.

The Adam sweep runs over the padded buffers, and for a gradient so small that its square underflows, v stays 0 and the
update is lr_t * m / eps: eps = 1e-8 multiplies whatever survives in m by 1e8.  The persistent BPTT used to leave
subnormal leftovers of its epoch bits in dG of the padded units (up to 32 T units of 2^-149 per frame row); summed over
the T * B rows of a batch they seed the padded biases with a gradient that Adam turns into a non-zero parameter.  This
file reproduces that arithmetic in fp32 with the suite's own model of TF's Adam (grad_clip_ref.adam_tf)."""
import numpy as np
import pytest

import grad_clip_ref as R

UNIT = np.float32(2.0 ** -149)          # the smallest fp32 subnormal


def run_adam(k, steps, lr=1e-3):
    """the parameter after each of `steps` fp32 Adam updates from p = m = v = 0 with the constant gradient k * 2^-149.
    Every operand is fp32 (the step count too, so that lr_t is), as in the sweep of optim.hip."""
    f = np.float32
    g = np.array([f(k) * UNIT], f)
    assert g[0] == k * 2.0 ** -149 and g.dtype == f          # exactly representable: k < 2^24
    p, m, v = np.zeros(1, f), np.zeros(1, f), np.zeros(1, f)
    out = []
    with np.errstate(under='ignore'):
        for t in range(1, steps + 1):
            p, m, v = R.adam_tf(p, g, m, v, f(t), f(lr))
            assert p.dtype == f and m.dtype == f and v.dtype == f
            assert v[0] == 0                                 # g * g underflows: Adam divides by eps alone
            out.append(float(p[0]))
    return out


@pytest.mark.parametrize('k', [16, 1000])
def test_a_few_units_are_flushed(k):
    """lr_t * m rounds to 0 while m is below about a thousand units: the parameter stays 0 (which is why parity tests of a
    handful of steps at small T * B never saw the padding move)"""
    assert run_adam(k, 5) == [0.0] * 5


@pytest.mark.parametrize('k,first', [(10 ** 5, -4.2e-37), (10 ** 7, -4.4e-35)])
def test_a_workload_sized_sum_leaves_zero(k, first):
    """at 1e5 units and more the parameter is non-zero after ONE step, thousands of times the gradient's own size
    (lr_t (1 - beta1) / eps = 3.2e3 at step 1)"""
    p = run_adam(k, 5)
    print(k, p)
    assert all(x != 0.0 for x in p)
    assert p[0] == pytest.approx(first, rel=0.05)
    assert abs(p[0]) > 1e3 * k * 2.0 ** -149


def test_the_former_bound_on_padded_dg_cannot_keep_the_padding_at_zero():
    """What rec_ref.check_backward allowed the persistent BPTT in a padded unit's dG, 32 T units of 2^-149 per frame row,
    summed over the T * B rows that the bias gradient sums: at the workload's T 500, B 64 that admits 5e8 units, far above
    the 1e5 at which the parameter leaves 0.  A bound of that form is no contract; the contract is +0 (pad_limit = 0)."""
    T, B = 500, 64
    per_row = 32 * T
    assert per_row * T * B > 1e5
    # and already the least the mechanism produces - 32 partial sums of one unit each in a frame row, on every other step
    assert 32 * (T // 2) * B > 1e5
