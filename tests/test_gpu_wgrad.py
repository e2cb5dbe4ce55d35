"""The kernels of the language model's backward pass, each alone through its hook (include/densecap_debug_grad.h): the
weight-gradient MFMA kernel, the embedding segment sum, the softmax-gradient rows and the LSTM cell backward."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

U = 2.0 ** -24                     # fp32 unit round-off
# N not a multiple of 32; M on both sides of the 64-row slice floor and of the 16-row staging round; M large enough to be split
# over workgroups with the partials reduced; K an odd multiple of 32
WGRAD_SHAPES = [(1, 32, 32), (2, 6, 32), (63, 71, 1056), (65, 71, 544), (257, 778, 768), (4352, 201, 512)]


@pytest.fixture(scope="module")
def ctx():
    from densecap_amd.ops import Context
    c = Context(0)
    yield c
    c.close()


@pytest.mark.parametrize("M,N,K", WGRAD_SHAPES, ids=["%dx%dx%d" % s for s in WGRAD_SHAPES])
def test_wgrad_within_the_fp32_summation_bound(ctx, M, N, K):
    """|C - C64| <= (M + 2) u (|A|^T |B|) per element: the bound of ANY fp32 summation order of M products (an f32 MFMA is an
    fmaf chain), and the same bits from a second call."""
    from densecap_amd import ops
    rng = np.random.default_rng(M * 7 + N)
    A = rng.standard_normal((M, N)).astype(np.float32)
    B = rng.standard_normal((M, K)).astype(np.float32)
    C = ops.wgrad(ctx, A, B)
    ref = A.astype(np.float64).T @ B.astype(np.float64)
    bound = (M + 2) * U * (np.abs(A).astype(np.float64).T @ np.abs(B).astype(np.float64))
    err = np.abs(C - ref)
    print("wgrad %dx%dx%d: worst err/bound %.3f" % (M, N, K, float((err / bound).max())))
    assert (err <= bound).all()
    assert np.array_equal(C.view(np.uint32), ops.wgrad(ctx, A, B).view(np.uint32))


@pytest.mark.parametrize("M,N,K", [(65, 71, 544), (4352, 201, 512)], ids=["one_slice", "split_rows"])
def test_wgrad_one_hot_returns_rows_of_b_bit_for_bit(ctx, M, N, K):
    """A one-hot A (each row one 1.0, each column hit at most once) selects rows of B: exact, and unhit columns give +0.0."""
    from densecap_amd import ops
    rng = np.random.default_rng(3)
    B = rng.standard_normal((M, K)).astype(np.float32)
    hit = min(M, N - 5)                                  # some columns stay unhit, some rows of A stay zero when M > N
    rows = rng.permutation(M)[:hit]
    cols = rng.permutation(N)[:hit]
    A = np.zeros((M, N), np.float32)
    A[rows, cols] = 1.0
    C = ops.wgrad(ctx, A, B)
    want = np.zeros((N, K), np.float32)
    want[cols] = B[rows]
    assert np.array_equal(C.view(np.uint32), want.view(np.uint32))


def test_embedding_segment_sum(ctx):
    """Duplicate tokens within and across rows, absent tokens exactly +0.0, |sum - sum64| <= (count + 2) u sum|term|."""
    from densecap_amd import ops
    rng = np.random.default_rng(8)
    E, rows_out = 544, 40
    tok = np.array([7, 7, 3, 40, 7, 1, 3, 3, 3, 12, 40, 7] + [5] * 70, np.int32)
    dx = rng.standard_normal((len(tok), E)).astype(np.float32)
    got = ops.embed_segsum(ctx, dx, tok, rows_out)
    for t in range(1, rows_out + 1):
        sel = dx[tok == t].astype(np.float64)
        if len(sel) == 0:
            assert np.array_equal(got[t - 1].view(np.uint32), np.zeros(E, np.uint32)), t
            continue
        bound = (len(sel) + 2) * U * np.abs(sel).sum(0)
        assert (np.abs(got[t - 1] - sel.sum(0)) <= bound).all(), t
    assert np.array_equal(got.view(np.uint32), ops.embed_segsum(ctx, dx, tok, rows_out).view(np.uint32))
    # a token fed once returns its row bit for bit
    assert np.array_equal(got[0], dx[5]) and np.array_equal(got[11], dx[9])


@pytest.mark.parametrize("V1", [6, 71, 778, 20001])
def test_softmax_gradient_rows(ctx, V1):
    """(softmax - onehot) scale against the float64 formula at 1e-6 of the row's largest entry; the padding columns come back
    as zeros; the log-sum-exp within 1e-6."""
    from densecap_amd import ops
    rng = np.random.default_rng(V1)
    ld = (V1 + 63) // 64 * 64
    x = np.full((3, ld), 7.5, np.float32)                        # the padding holds something that must not survive
    x[:, :V1] = (rng.standard_normal((3, V1)) * np.array([[1.0], [4.0], [0.1]])).astype(np.float32)
    tgt = np.array([1, V1, 1 + V1 // 2], np.int32)
    scale = 0.37
    got, lse = ops.softmax_grad(ctx, x, tgt, scale, V1=V1)
    x64 = x[:, :V1].astype(np.float64)
    mx = x64.max(1, keepdims=True)
    lse64 = mx[:, 0] + np.log(np.exp(x64 - mx).sum(1))
    ref = np.exp(x64 - lse64[:, None])
    ref[np.arange(3), tgt - 1] -= 1.0
    ref *= np.float64(np.float32(scale))
    assert not got[:, V1:].any()
    for r in range(3):
        assert np.abs(got[r, :V1] - ref[r]).max() <= 1e-6 * np.abs(ref[r]).max(), r
    assert np.abs(lse - lse64).max() <= 1e-6


@pytest.mark.parametrize("Hd", [32, 1056])
def test_lstm_cell_backward(ctx, Hd):
    """dgates and dc_prev against the float64 formulas at 1e-6 of the row's largest entry."""
    from densecap_amd import ops
    rng = np.random.default_rng(Hd)
    rows = 5
    a = (rng.standard_normal((rows, 4 * Hd)) * 1.5).astype(np.float32)
    c_prev = rng.standard_normal((rows, Hd)).astype(np.float32)
    sig = lambda v: 1.0 / (1.0 + np.exp(-v))
    a64 = a.astype(np.float64)
    i, f, o, g = sig(a64[:, :Hd]), sig(a64[:, Hd:2 * Hd]), sig(a64[:, 2 * Hd:3 * Hd]), np.tanh(a64[:, 3 * Hd:])
    c = (f * c_prev + i * g).astype(np.float32)                   # the c the forward kept
    dh = rng.standard_normal((rows, Hd)).astype(np.float32)
    dc = rng.standard_normal((rows, Hd)).astype(np.float32)
    dg, dcp = ops.lstm_cell_bwd(ctx, a, c_prev, c, dh, dc)
    tc = np.tanh(c.astype(np.float64))
    dct = dc + dh * o * (1 - tc * tc)
    ref = np.concatenate([dct * g * i * (1 - i), dct * c_prev * f * (1 - f), dh * tc * o * (1 - o), dct * i * (1 - g * g)], 1)
    for r in range(rows):
        assert np.abs(dg[r] - ref[r]).max() <= 1e-6 * np.abs(ref[r]).max(), r
        assert np.abs(dcp[r] - (dct * f)[r]).max() <= 1e-6 * np.abs((dct * f)[r]).max(), r
