"""Who owns the host layer's device scratch, seen from outside through dc_debug_fetch "scratch" = [call-scoped blocks alive
now, bytes held by the context's seven grow-only buffers, (re)allocations of those buffers so far].

Every entry point that takes scratch of its own is called once on the smallest model the loader admits (test_gpu_dims'
"minimal" set) with a handful of rows -- 5 codes, 40 boxes, 3 ground-truth boxes, a 64 x 96 image: after every call, a refused
one included, no call-scoped block is alive; a repeated call at the same shapes reallocates nothing; a larger shape grows the
kept buffers once and going back keeps them."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

H, W = 64, 96
N_CODES, N_BOXES = 5, 40


@pytest.fixture(scope="module")
def model():
    from densecap_amd import DenseCapModel
    from tests.test_gpu_dims import set_weights
    m = DenseCapModel(set_weights("minimal"), device=0)
    m.setTestArgs(num_proposals=20)
    yield m
    m.ctx.close()


def scratch(m):
    v, n = m.debug_fetch("scratch", (3,), np.int64)
    assert n == 3
    return [int(x) for x in v]


def _image(h=H, w=W, seed=1):
    from densecap_amd.weights import make_synthetic_image
    return make_synthetic_image(h, w, seed)


def _boxes(rng, n, h=H, w=W):
    """(n, 4) xcycwh inside an h x w image"""
    wh = rng.uniform(8, 40, (n, 2))
    c = np.stack([rng.uniform(wh[:, 0] / 2 + 1, w - wh[:, 0] / 2), rng.uniform(wh[:, 1] / 2 + 1, h - wh[:, 1] / 2)], 1)
    return np.concatenate([c, wh], 1).astype(np.float32)


def _xyxy(b):
    return np.concatenate([b[:, :2] - b[:, 2:] / 2, b[:, :2] + b[:, 2:] / 2], 1).astype(np.float32)


GT = np.array([[40, 30, 20, 20], [60, 40, 30, 24], [30, 40, 40, 30]], np.float32)
LOSS_OPTS = dict(batch_size=64, seed=3, remove_outbounds=0)


def _labels(m, G, seed=2):
    rng = np.random.default_rng(seed)
    lab = np.zeros((G, 2), np.int32)
    lab[:, 0] = rng.integers(1, m.vocab_size + 1, G)
    return lab


def _calls(m):
    """(name, call) for every converted entry point, in the order of the tour"""
    from densecap_amd import ops
    from tests.test_gpu_sample import _greedy
    ctx, D, Hd, V, T = m.ctx, m.fc_dim, m.ctx.lm_dims["Hd"], m.vocab_size, m.seq_length
    rng = np.random.default_rng(5)
    codes = np.maximum(rng.standard_normal((N_CODES, D)), 0).astype(np.float32)
    boxes = _boxes(rng, N_BOXES)
    scores = rng.standard_normal(N_BOXES).astype(np.float32)
    queries = rng.integers(1, V + 1, (2, 2)).astype(np.int32)
    img = _image()
    fh, fw = ops.feature_size(ctx, H, W)
    feat512 = rng.standard_normal((512, fh, fw)).astype(np.float32)
    rois = _boxes(rng, N_CODES)
    x32 = rng.standard_normal((N_CODES, 32)).astype(np.float32)
    w32 = rng.standard_normal((8, 32)).astype(np.float32)

    def nms_empty():
        cnt = ctx.to_device(np.array([7], np.int32)); dummy = ctx.empty((4,), np.float32); picks = ctx.empty((1,), np.int32)
        ops.check(ctx.h, ctx.lib.dc_op_nms(ctx.h, dummy.ptr, dummy.ptr, None, 0, C.c_float(0.5), -1, picks.ptr, cnt.ptr), "dc_op_nms")
        assert cnt.numpy()[0] == 0

    def lm_sample_beam():
        m.setBeamSize(2)
        try:
            _greedy(m, codes)
        finally:
            m.setBeamSize(0)

    def linear_split_bf16():
        m.setMathMode(1)                      # the per-op call makes temporary planes of its weight
        try:
            ops.linear(ctx, x32, w32, np.zeros(8, np.float32))
        finally:
            m.setMathMode(0)

    def rescore_tail():
        h = rng.standard_normal((N_CODES, Hd)).astype(np.float32)
        hb, hn, sc = ops.screen_scores(ctx, h, V)
        ops.rescore_tail(ctx, sc[:N_CODES], h, hn[:N_CODES], c=rng.standard_normal((N_CODES, Hd)).astype(np.float32),
                         gates_pre=rng.standard_normal((N_CODES, 4 * Hd)).astype(np.float32))

    def beam_std_finish():
        beams = rng.integers(1, V + 2, (3, 2, T)).astype(np.int32)
        ops.beam_std_finish(ctx, -rng.uniform(0, 5, (3, 2)).astype(np.float32), beams, np.full((3, 2), T, np.int32), 2, 0.7)

    return [
        ("nms n=0", nms_empty),
        ("nms n=40", lambda: ops.nms(ctx, np.concatenate([_xyxy(boxes), scores[:, None]], 1), 0.5)),
        ("nms_multi", lambda: ops.nms_multi(ctx, _xyxy(boxes), rng.standard_normal((N_BOXES, 2)), 0.5, 5)),
        ("box_sampler", lambda: ops.box_sampler(ctx, boxes, GT, H, W, **LOSS_OPTS)),
        ("eval_match", lambda: ops.eval_match(ctx, [boxes], [scores], [GT])),
        ("lm_sample greedy", lambda: _greedy(m, codes)),
        ("lm_sample beam 2", lm_sample_beam),
        ("lm_score", lambda: ops.lm_score(ctx, codes, queries)),
        ("lm_sample_n", lambda: ops.lm_sample_n(ctx, codes, 2, seed=1)),
        ("lm_sample_n top_k", lambda: ops.lm_sample_n(ctx, codes, 2, seed=1, top_k=2)),
        ("lm_beam_n", lambda: ops.lm_beam_n(ctx, codes, 2)),
        ("lm_grad", lambda: ops.lm_grad(ctx, codes, _labels(m, N_CODES))),
        ("linear", lambda: ops.linear(ctx, x32, w32, np.zeros(8, np.float32))),
        ("linear split-bf16", linear_split_bf16),
        ("conv3x3", lambda: ops.conv3x3(ctx, rng.standard_normal((1, 32, 6, 8)), rng.standard_normal((8, 32, 3, 3)), np.zeros(8))),
        ("roi_pool_grad", lambda: ops.roi_pool_grad(ctx, feat512[:4], rois, H, W, rng.standard_normal((N_CODES, 4, 7, 7)))),
        ("recog_grad", lambda: ops.recog_grad(ctx, feat512, rois, 2, rois[:2] + 1, H, W, **LOSS_OPTS)),
        ("forward_losses", lambda: m.forward_losses(img, GT, _labels(m, 3), **LOSS_OPTS)),
        ("loss_gradients", lambda: m.loss_gradients(img, GT, _labels(m, 3), **LOSS_OPTS)),
        ("localize_captions", lambda: m.localizeCaptions(img, queries)),
        ("beam_captions", lambda: m.beamCaptions(img, 2)),
        ("preprocess_u8", lambda: ops.preprocess_u8(ctx, rng.integers(0, 256, (50, 70, 3)).astype(np.uint8), 96)),
        ("densecap_debug.h: rescore_tail", rescore_tail),
        ("densecap_debug.h: sample noise", lambda: m.debug_fetch("sample_gumbel@0", (16,), np.float32)),
        ("densecap_debug_sample.h: sample_trunc_rows",
         lambda: ops.sample_trunc_rows(ctx, rng.standard_normal((N_CODES, V + 1)), np.zeros((N_CODES, 2), np.int32), 1, 1, 1.0, top_k=2)),
        ("densecap_debug_beam.h: beam_std_finish", beam_std_finish),
        ("densecap_debug_grad.h: wgrad", lambda: ops.wgrad(ctx, rng.standard_normal((N_CODES, 8)), rng.standard_normal((N_CODES, 32)))),
        ("densecap_debug_grad.h: embed_segsum",
         lambda: ops.embed_segsum(ctx, rng.standard_normal((N_CODES, 32)), np.array([2, 1, 2, 3, 1], np.int32), 4)),
        ("densecap_debug_bwd.h: wgrad_ld",
         lambda: ops.wgrad_ld(ctx, rng.standard_normal((N_CODES, 9)), rng.standard_normal((N_CODES, 33)), 8, 32, np.zeros((8, 34)))),
        ("densecap_debug_recog.h: roi_tap_index", lambda: ops.roi_tap_index(ctx, rois, fh, fw, H, W)),
    ]


def test_no_call_leaves_a_scoped_block_behind(model):
    m = model
    assert scratch(m)[0] == 0
    for name, call in _calls(m):
        call()
        assert scratch(m)[0] == 0, name


def test_refusals_past_the_allocation_leave_nothing_and_the_context_works_on(model):
    from densecap_amd import ops
    from densecap_amd._lib import DenseCapError
    m = model
    rng = np.random.default_rng(6)
    boxes = _boxes(rng, N_BOXES)
    img, lab = _image(), _labels(m, 3)
    free = ops.box_sampler(m.ctx, boxes, GT, H, W, **LOSS_OPTS)
    with pytest.raises(DenseCapError, match=r"\(-1\).*outside the candidate lists"):
        ops.box_sampler(m.ctx, boxes, GT, H, W, forced_pos=[free["total_pos"]], **LOSS_OPTS)
    assert scratch(m)[0] == 0
    again = ops.box_sampler(m.ctx, boxes, GT, H, W, **LOSS_OPTS)
    assert np.array_equal(again["pos_input_idx"], free["pos_input_idx"]) and scratch(m)[0] == 0
    good = m.forward_losses(img, GT, lab, **LOSS_OPTS)
    kept = scratch(m)
    with pytest.raises(DenseCapError, match=r"\(-1\).*outside the candidate lists"):
        m.forward_losses(img, GT, lab, forced_pos=[good["total_pos"]], **LOSS_OPTS)
    assert scratch(m) == kept and kept[0] == 0
    again = m.forward_losses(img, GT, lab, **LOSS_OPTS)
    assert (again["num_pos"], again["num_neg"]) == (good["num_pos"], good["num_neg"]) and again["num_pos"] > 0
    assert scratch(m) == kept


def test_kept_buffers_grow_once_per_larger_shape(model):
    from densecap_amd import ops
    m, ctx = model, model.ctx
    rng = np.random.default_rng(7)

    def calls(h, w, rows, C_, opts):
        img, lab = _image(h, w), _labels(m, 3)
        fh, fw = ops.feature_size(ctx, h, w)
        feat = rng.standard_normal((512, fh, fw)).astype(np.float32)
        rois = _boxes(rng, rows, h, w)
        u8 = rng.integers(0, 256, (h - 14, w - 26, 3)).astype(np.uint8)
        return [("forward_losses", lambda: m.forward_losses(img, GT, lab, **opts)),
                ("loss_gradients", lambda: m.loss_gradients(img, GT, lab, **opts)),
                ("recog_grad", lambda: ops.recog_grad(ctx, feat, rois, 2, rois[:2] + 1, h, w, **opts)),
                ("roi_pool_grad", lambda: ops.roi_pool_grad(ctx, feat[:C_], rois, h, w, rng.standard_normal((rows, C_, 7, 7)))),
                ("preprocess_u8", lambda: ops.preprocess_u8(ctx, u8, w))]

    small = calls(H, W, N_CODES, 4, LOSS_OPTS)
    for _, call in small:
        call()
    base = scratch(m)
    assert base[0] == 0 and base[1] > 0 and base[2] > 0
    for name, call in small:                                   # the same shapes again: every buffer fits
        call()
        assert scratch(m) == base, name
    # Larger shapes, one entry point at a time, each past everything before it: bytes and count both rise.  The losses' scratch
    # goes by the anchor count (24 at 64 x 96, then 96, then 192); the recognition backward's by its rows (at most batch_size =
    # 64 so far, then 100); the RoI index's by rows x taps (100 rows so far, then 150, on 512 channels as the backward runs
    # it); the preprocessing buffers by the input image.
    big = dict(LOSS_OPTS, batch_size=128)
    larger = [calls(128, 192, N_CODES, 4, LOSS_OPTS)[0], calls(192, 256, N_CODES, 4, LOSS_OPTS)[1], calls(192, 256, 100, 4, big)[2],
              calls(192, 256, 150, 512, big)[3], calls(192, 256, N_CODES, 4, LOSS_OPTS)[4]]
    last = base
    for name, call in larger:
        call()
        now = scratch(m)
        assert now[0] == 0 and now[1] > last[1] and now[2] > last[2], (name, last, now)
        last = now
    for name, call in small:                                   # back to the small shapes: nothing shrinks, nothing moves
        call()
        assert scratch(m) == last, name
