"""screen_operands_kernel (dc_debug_screen_operands; docs/SEMANTICS.md, "Training step"): the decode screen's two operands made
on the device from the fp32 lm_out_w rows, as dc_train_step remakes them.  The bf16 bits are dc_load_weights' host rule's; the
padding is zero; the fp16 norm is an upper bound of the row's true 2-norm (what DESIGN.md §4.1c's proof uses) and not loose."""
import numpy as np
import pytest

from tests import optim_rules as R

pytestmark = pytest.mark.gpu

F32 = np.float32


@pytest.fixture(scope="module")
def ctx():
    from densecap_amd import Context
    c = Context(0)
    yield c
    c.close()


def _weights(V1, Hd, seed):
    rng = np.random.RandomState(seed)
    W = (rng.randn(V1, Hd) * 10.0 ** rng.uniform(-3, 1, (V1, 1))).astype(F32)
    W[0, 1] = np.nan                                     # a NaN, an infinity, a denormal row, a zero row, a row past fp16's range
    W[1, Hd - 1] = np.inf
    W[2] = (rng.randn(Hd) * 1e-40).astype(F32)
    W[3] = 0.0
    W[4] = 3e4
    W.view(np.uint32)[5, ::2] = 0x7f800001               # a signalling NaN: the host rule quiets it
    return W


@pytest.mark.parametrize("V1,Hd", [(6, 32), (130, 96), (1000, 512)])
def test_screen_operands_follow_the_host_rule(ctx, V1, Hd):
    from densecap_amd import ops
    W = _weights(V1, Hd, seed=V1)
    wb, wn = ops.screen_operands(ctx, W)
    V1pad, Kp = (V1 + 63) // 64 * 64, (Hd + 63) // 64 * 64
    assert wb.shape == (V1pad, Kp) and wn.shape == (V1pad,)
    assert np.array_equal(wb[:V1, :Hd], R.bf16_bits_host_rule(W))
    assert not wb[V1:].any() and not wb[:, Hd:].any() and not wn[V1:].any()
    got = wn[:V1].view(np.float16).astype(np.float64)
    with np.errstate(all="ignore"):
        norm = np.sqrt((W.astype(np.float64) ** 2).sum(1))
    nan = np.isnan(norm)
    assert nan[0] and nan[5] and np.isnan(got[nan]).all() and not np.isnan(got[~nan]).any()
    ok = ~nan
    assert (got[ok] >= norm[ok]).all()
    # not loose: at most the first fp16 value above norm * (1 + 1e-6)
    with np.errstate(over="ignore"):
        h = (norm[ok] * (1 + 1e-6)).astype(np.float16)
    up = np.where(h.astype(np.float64) > norm[ok] * (1 + 1e-6), h, np.nextafter(h, np.float16(np.inf)))
    assert (got[ok] <= up.astype(np.float64)).all()
    assert np.isinf(got[1]) and np.isinf(got[4]) and got[3] == 0.0 and 0.0 < got[2] <= 2.0 ** -24 * 2
