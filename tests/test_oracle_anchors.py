"""The oracle's forward takes its anchor table from the weights (LocalizationLayer.lua:611-621: `opt.anchors`, or the
default table times `anchor_scale`; k = the number of columns), and make_synthetic_weights can build such a model.  CPU only.

What is pinned: with the default table nothing moves (the forward with the table passed explicitly, the forward of a weights
dict that carries no table, and rpn_decode called as it always was give the same arrays, exactly); with k = 5, k = 1 and
twelve anchors of other sizes the RPN stage has k * fh * fw rows and its boxes are make_boxes on the same box head."""
import numpy as np
import pytest
import torch

from densecap_amd.weights import DEFAULT_ANCHORS, make_synthetic_image, make_synthetic_weights
from oracle import densecap_oracle as O

H, W = 96, 128                      # conv5_3 map 6 x 8
SMALL = dict(vocab_size=30, seq_length=4, rpn_hidden=32, enc_size=32, rnn_size=32, fc_dim=256)
ANCHORS_K5 = np.array([[30, 60, 90, 45, 120], [30, 40, 45, 90, 100]], np.float32)
ANCHORS_K1 = np.array([[64], [48]], np.float32)
ANCHORS_K12_OTHER = (DEFAULT_ANCHORS * np.float32(0.5) + np.float32(3)).astype(np.float32)   # twelve, none of them a default size


def _forward(Wt, **kw):
    st = {}
    out = O.forward_test(make_synthetic_image(H, W, 2), Wt, 0.7, 0.3, 40, Wt["seq_length"], stages=st, **kw)
    return out, st


def test_default_anchors_draw_the_same_stream_and_an_anchor_table_sizes_the_heads():
    a = make_synthetic_weights(seed=9, **SMALL)
    b = make_synthetic_weights(seed=9, anchors=DEFAULT_ANCHORS.copy(), **SMALL)
    for key in a:
        va, vb = a[key], b[key]
        if isinstance(va, list):
            assert all(torch.equal(x, y) for x, y in zip(va, vb)), key
        elif isinstance(va, torch.Tensor):
            assert torch.equal(va, vb), key
        else:
            assert va == vb, key
    for anchors in (ANCHORS_K5, ANCHORS_K1, ANCHORS_K12_OTHER):
        k = anchors.shape[1]
        w = make_synthetic_weights(seed=9, anchors=anchors, **SMALL)
        assert tuple(w["rpn_box_w"].shape) == (4 * k, 32, 1, 1) and tuple(w["rpn_box_b"].shape) == (4 * k,)
        assert tuple(w["rpn_score_w"].shape) == (2 * k, 32, 1, 1) and tuple(w["rpn_score_b"].shape) == (2 * k,)
        np.testing.assert_array_equal(w["anchors"].numpy(), anchors)
        from densecap_amd.weights import check_weight_shapes
        check_weight_shapes(w)
        # the tensors drawn before the RPN heads do not depend on k
        assert torch.equal(w["rpn_conv_w"], a["rpn_conv_w"]) and torch.equal(w["conv_w"][12], a["conv_w"][12])
    for bad in (np.zeros((2, 0), np.float32), np.zeros((3, 4), np.float32), np.zeros((12,), np.float32)):
        with pytest.raises(ValueError):
            make_synthetic_weights(seed=9, anchors=bad, **SMALL)


def test_forward_with_the_default_table_is_unchanged():
    Wt = make_synthetic_weights(seed=9, **SMALL)
    explicit = dict(Wt, anchors=torch.from_numpy(O.DEFAULT_ANCHORS.copy()))
    without = {k: v for k, v in Wt.items() if k != "anchors"}
    (b0, s0, t0), st0 = _forward(Wt)
    assert len(b0) > 0
    for other in (explicit, without):
        (b1, s1, t1), st1 = _forward(other)
        np.testing.assert_array_equal(b1, b0); np.testing.assert_array_equal(s1, s0); np.testing.assert_array_equal(t1, t0)
        for key in ("boxes", "anchors", "trans", "scores2", "x1y1x2y2", "p", "rows", "valid"):
            np.testing.assert_array_equal(st1["rpn"][key], st0["rpn"][key], err_msg=key)
    # ... and the RPN stage is rpn_decode called without a table, as the forward called it before
    d = O.rpn_decode(st0["box_head"], st0["score_head"], H, W)
    for key in d:
        np.testing.assert_array_equal(st0["rpn"][key], d[key], err_msg=key)


@pytest.mark.parametrize("anchors", [ANCHORS_K5, ANCHORS_K1, ANCHORS_K12_OTHER], ids=["k5", "k1", "k12_other_sizes"])
def test_forward_takes_k_and_the_anchor_sizes_from_the_weights(anchors):
    k = anchors.shape[1]
    Wt = make_synthetic_weights(seed=9, anchors=anchors, **SMALL)
    (boxes, scores, tokens), st = _forward(Wt)
    fh, fw = st["feat"].shape[1:]
    assert (fh, fw) == (6, 8)
    assert st["box_head"].shape == (4 * k, fh, fw) and st["score_head"].shape == (2 * k, fh, fw)
    assert st["rpn"]["valid"].shape == (k * fh * fw,) and st["rpn"]["valid"].any()
    assert len(boxes) > 0 and tokens.shape == (len(boxes), 4)
    # unclipped: every one of the k * fh * fw rows survives, and the boxes are make_boxes on the same box head
    (_, _, _), su = _forward(Wt, clip_boxes=False)
    want = O.make_boxes(su["box_head"], *O.VGG16_FIELD_CENTERS, anchors)
    assert su["rpn"]["boxes"].shape == (k * fh * fw, 4)
    np.testing.assert_array_equal(su["rpn"]["boxes"], want)
    np.testing.assert_array_equal(su["rpn"]["rows"], np.arange(k * fh * fw))
    # the anchor sizes are the table's: row b = a * fh * fw + y * fw + x carries (w, h) of anchor a
    np.testing.assert_array_equal(su["rpn"]["anchors"][:, 2], np.repeat(anchors[0], fh * fw))
    np.testing.assert_array_equal(su["rpn"]["anchors"][:, 3], np.repeat(anchors[1], fh * fw))
    # the clipped stage keeps a subset of those rows, with the same anchors
    np.testing.assert_array_equal(st["rpn"]["anchors"], su["rpn"]["anchors"][st["rpn"]["rows"]])
    if k == 12:
        d = O.rpn_decode(st["box_head"], st["score_head"], H, W)          # the default table on the same heads: other boxes
        assert d["valid"].shape == st["rpn"]["valid"].shape
        assert not np.array_equal(d["anchors"], st["rpn"]["anchors"])


def test_lm_sample_returns_its_state_on_request():
    Wt = make_synthetic_weights(seed=9, **SMALL)
    codes = torch.relu(torch.randn(7, 256, generator=torch.Generator().manual_seed(1)))
    seq = O.lm_sample(codes, Wt, 4)
    seq2, state = O.lm_sample(codes, Wt, 4, return_state=True)
    seq3, logits, state3 = O.lm_sample(codes, Wt, 4, return_logits=True, return_state=True)
    np.testing.assert_array_equal(seq2, seq); np.testing.assert_array_equal(seq3, seq)
    assert len(logits) == 4
    assert state["enc"].shape == (7, 32) and state["h"].shape == (7, 32) and state["c"].shape == (7, 32)
    np.testing.assert_array_equal(state["enc"], torch.relu(codes @ Wt["lm_enc_w"].t() + Wt["lm_enc_b"]).numpy())
    # h after step T is what the last logits were formed from
    want = torch.from_numpy(state["h"]) @ Wt["lm_out_w"].t() + Wt["lm_out_b"]
    np.testing.assert_array_equal(want.numpy(), logits[-1].numpy())
    for key in state:
        np.testing.assert_array_equal(state[key], state3[key])
