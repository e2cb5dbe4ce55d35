"""LM:beamsearch on the GPU, kernel by kernel and step by step (densecap_amd/csrc/beam.hip; the hooks of include/densecap_debug.h).

  a. beam_logsoftmax_topk_kernel against oracle._log_softmax_thnn + a stable top-k (tests/beam_rules.py::topk_ref) on inputs
     whose reference has no near tie (a permutation of arange(V1) / 1024: log-probability gaps of 9.8e-4 against a float ulp of at
     most 3.8e-6), with exact duplicates where ties are wanted: indices equal, values within one ulp (the device adds the double
     exponentials in another order).  Every row width at which the kernel takes another path, both sides of the 64 KiB dynamic
     LDS limit, the largest row the device grants, a padded row stride, the finished mask, an all-NaN row.
  b. beam_merge_kernel against merge_ref, bit for bit, on multiples of 0.25 (exact sums, ties everywhere -- at beam 32 across
     all four 256-strides of the candidate array), with finished parents, END chosen at t and END already in the row.
  c. every step of every proposal, teacher-forced on the oracle's trajectory (beam_rules.oracle_walk): the oracle's fp32 state
     goes into dc_debug_beam_start / dc_debug_beam_step, the lists that come back meet the rank-wise rule of
     beam_rules.check_lists against the oracle's log-probabilities, the merge outputs are merge_ref of the device's own lists bit
     for bit, the re-indexed state is the oracle's at the device's parents within parity.REL.
  d. the hooks are the production loop: chained on the device's own outputs they end in the tokens of dc_op_lm_sample.
  e. non-finite codes: the row has no word (docs/SEMANTICS.md, "Rows without a word"), every other row is untouched.

Nothing in this module excuses a row, a step or a rank; (c) prints `excused 0` with the worst figures it saw.

Measured on an MI355X (70 proposals, V = 300, T = 7; value = |top_lp - oracle| worst, slack = worst rank slack, both against
TOKEN_TOL = 2e-5 / 2 x TOKEN_TOL):
  beam  1:   487 live lists, value 1.9e-06, slack 0          beam 20: 5036 live lists, value 3.6e-06, slack 1.9e-06
  beam  5:  2091 live lists, value 2.9e-06, slack 0          beam 32: 7617 live lists, value 3.1e-06, slack 0
  minimal (beam 2, T = 1): 70 lists, value 2.4e-07, slack 0;  big_vocab (beam 3, V = 20000): 700 lists, value 2.9e-06, slack 0
No row, step or rank excused.  Three value-only mutations of beam.hip (tie rule of arg_better flipped; j % beam for j / beam in
the merge's candidate sum; finished mask ignored in the top-k kernel) each fail (a) or (b) and (c) of this module.
"""
import numpy as np
import pytest

from tests import beam_rules as R
from tests import parity

pytestmark = pytest.mark.gpu
V, T, N = 300, 7, 70
END = V + 1


@pytest.fixture(scope="module")
def model():
    """The model of test_gpu_e2e.py::test_beamsearch_teacher_forced.  One small forward first, so that the ctx's fault word
    exists and reads 0 from then on."""
    from densecap_amd import DenseCapModel
    from densecap_amd.weights import make_synthetic_image, make_synthetic_weights
    parity.oracle_threads()
    W = make_synthetic_weights(seed=5, vocab_size=V, seq_length=T)
    m = DenseCapModel(W, device=0)
    m.setTestArgs(rpn_nms_thresh=0.7, final_nms_thresh=0.3, num_proposals=20)
    m.forward_raw(make_synthetic_image(96, 128, 0))
    assert _fault_word(m) == 0
    yield m, W
    m.ctx.close()


def _fault_word(m):
    return int(m.debug_fetch("fault_word", (1,), np.int32)[0][0])


def _max_vocab():
    """beam_topk_max_vocab() of beam.hip from the device attribute: the per-block LDS less 1 KiB, in floats."""
    import torch
    return (int(torch.cuda.get_device_properties(0).shared_memory_per_block) - 1024) // 4


# ---- a. the top-k kernel -------------------------------------------------------------------------------------------------------
def _perm_rows(rows, V1, seed):
    """Every row a permutation of arange(V1) / 1024 - 3: exact in fp32, all gaps multiples of 2^-10."""
    rng = np.random.default_rng(seed)
    base = (np.arange(V1, dtype=np.float64) / 1024 - 3).astype(np.float32)
    return np.stack([base[rng.permutation(V1)] for _ in range(rows)])


def _check_topk(ctx, x, k, finished=None, ld=None, what=""):
    from densecap_amd import ops
    lp, idx = ops.beam_topk(ctx, x, k, finished, ld)
    rlp, ridx, _ = R.topk_ref(x, k, finished)
    np.testing.assert_array_equal(idx, ridx, err_msg="%s: top_idx" % what)
    ulp = np.spacing(np.abs(rlp))
    bad = np.abs(lp.astype(np.float64) - rlp) > ulp
    assert not bad.any(), "%s: top_lp off by more than one ulp at %s: %r vs %r" % (
        what, np.argwhere(bad)[0].tolist(), lp[bad][0], rlp[bad][0])
    if finished is not None:
        f = np.asarray(finished, bool)
        assert (lp[f].view(np.uint32) == 0).all() and (idx[f] == np.arange(1, k + 1)).all()
    return lp, idx


@pytest.mark.parametrize("V1", [1, 2, 6, 255, 256, 257, 301, 1025, 16384, 16385, 20001])
def test_topk_row_widths(model, V1):
    """One value short of, at and past a 256-thread pass; 16384 floats are exactly the 64 KiB a launch gets without asking,
    16385 the first row that needs the raised limit.  k = 1, 5, 32 where the row has that many; k == V1 empties the row."""
    ctx = model[0].ctx
    for k in sorted({1, min(5, V1), min(32, V1)} | ({V1} if V1 <= 6 else set())):
        _check_topk(ctx, _perm_rows(3, V1, V1 + k), k, what="V1 %d k %d" % (V1, k))


@pytest.mark.parametrize("rows", [1, 70, 300])
def test_topk_row_counts_and_stride(model, rows):
    ctx = model[0].ctx
    x = _perm_rows(rows, 301, rows)
    _check_topk(ctx, x, 5, what="rows %d" % rows)
    if rows == 70:
        _check_topk(ctx, x, 5, ld=301 + 7, what="ld = V1 + 7")


def test_topk_largest_row_and_refusals(model):
    """The largest row the device grants runs; one more float, or k > V1, is refused before anything is launched (the outputs
    keep what they held)."""
    from densecap_amd._lib import DenseCapError, check
    m = model[0]
    ctx = m.ctx
    vmax = _max_vocab()
    assert vmax > 20001
    _check_topk(ctx, _perm_rows(2, vmax, 1), 32, what="V1 %d (largest)" % vmax)
    for V1, k in ((vmax + 1, 5), (6, 7), (6, 0)):
        xd = ctx.to_device(np.zeros((1, V1), np.float32))
        lp = ctx.to_device(np.full((1, 8), 7.0, np.float32)); idx = ctx.to_device(np.full((1, 8), -7, np.int32))
        with pytest.raises(DenseCapError):
            check(ctx.h, ctx.lib.dc_debug_beam_topk(ctx.h, xd.ptr, 1, V1, V1, None, k, lp.ptr, idx.ptr), "dc_debug_beam_topk")
        assert (lp.numpy() == 7.0).all() and (idx.numpy() == -7).all()
    _check_topk(ctx, _perm_rows(2, 301, 2), 5, what="after the refusals")


def test_topk_ties(model):
    """Equal values come out in ascending index: a flat row gives 1..k; the row maximum planted at columns 5, 70, 261 and 300
    of 301 ties within a thread (5 and 261 = 5 + 256: its first and second pass), across waves (70) and at the last column."""
    ctx = model[0].ctx
    for V1, k in ((301, 32), (6, 6), (1025, 5)):
        lp, idx = _check_topk(ctx, np.full((4, V1), 0.375, np.float32), k, what="flat V1 %d" % V1)
        assert (idx == np.arange(1, k + 1)).all() and len(np.unique(lp)) == 1
    x = _perm_rows(6, 301, 9)
    cols = [5, 70, 261, 300]
    x[:, cols] = np.float32(2.0)                                       # above every other entry (max 300 / 1024 - 3)
    x[3, cols] = x[3].min() - np.float32(1)                             # and once the row minimum: never picked
    lp, idx = _check_topk(ctx, x, 5, what="planted maximum")
    for r in (0, 1, 2, 4, 5):
        assert idx[r, :4].tolist() == [6, 71, 262, 301]
    assert not set(idx[3].tolist()) & {6, 71, 262, 301}


def test_topk_finished_mask(model):
    """Finished rows give k zeros and 1..k whatever their logits hold (a NaN row among them); live rows are not affected."""
    ctx = model[0].ctx
    x = _perm_rows(70, 301, 4)
    fin = (np.random.default_rng(4).random(70) < 0.4).astype(np.uint8)
    fin[:3] = (1, 0, 1)
    x[0] = np.nan
    for k in (1, 5, 32):
        _check_topk(ctx, np.where(np.isnan(x), np.float32(0), x), k, fin, what="finished mask k %d" % k)   # reference: finite
        from densecap_amd import ops
        lp, idx = ops.beam_topk(ctx, x, k, fin)
        assert (lp[0].view(np.uint32) == 0).all() and (idx[0] == np.arange(1, k + 1)).all()


def test_topk_all_nan_row_has_no_word(model):
    """A row of NaNs has no comparable candidate: every rank is word 0 with a NaN log-probability -- not a stale or repeated
    index --, the rows around it are what they are without it, and nothing is reported through the fault word."""
    from densecap_amd import ops
    m = model[0]
    x = _perm_rows(5, 301, 5)
    clean_lp, clean_idx = _check_topk(m.ctx, x, 5, what="clean")
    x[2] = np.nan
    for k, V1 in ((5, 301), (32, 301), (1, 301)):
        lp, idx = ops.beam_topk(m.ctx, x[:, :V1], k)
        assert (idx[2] == 0).all() and np.isnan(lp[2]).all(), (idx[2], lp[2])
        if k == 5:
            np.testing.assert_array_equal(idx[[0, 1, 3, 4]], clean_idx[[0, 1, 3, 4]])
            np.testing.assert_array_equal(lp[[0, 1, 3, 4]], clean_lp[[0, 1, 3, 4]])
    assert _fault_word(m) == 0


# ---- b. the merge kernel -------------------------------------------------------------------------------------------------------
def _merge_case(nprop, beam, t, seed):
    """Inputs of a merge at column t on multiples of 0.25.  Parents are finished with probability 0.3 (END in a column below t,
    lists of zeros / 1..beam as the top-k kernel makes them); live lists hold END now and then, at any rank."""
    rng = np.random.default_rng(seed)
    beam_lp = -np.sort(rng.integers(0, 12, (nprop, beam)), axis=1).astype(np.float32) * np.float32(0.25)
    beams = np.ones((nprop, beam, T), np.int32)
    beams[:, :, :t] = rng.integers(1, END, (nprop, beam, t))
    fin = rng.random((nprop, beam)) < 0.3
    fin[0, 0] = beam > 1 and nprop > 1                               # the best parent of the first proposal is finished
    for p, b in np.argwhere(fin):
        beams[p, b, rng.integers(0, t)] = END
    top_lp = -np.sort(rng.integers(0, 8, (nprop, beam, beam)), axis=2).astype(np.float32) * np.float32(0.25)
    top_idx = np.stack([np.stack([rng.permutation(END - 1)[:beam] + 1 for _ in range(beam)]) for _ in range(nprop)]).astype(np.int32)
    put_end = rng.random((nprop, beam)) < 0.5
    for p, b in np.argwhere(put_end):
        top_idx[p, b, rng.integers(0, beam)] = END
    top_idx[-1, 0, 0] = END                                          # END chosen at t, as the best word of the best parent
    top_lp[fin] = 0
    top_idx[fin] = np.arange(1, beam + 1)
    return top_lp, top_idx, beam_lp, beams


@pytest.mark.parametrize("beam", [1, 2, 3, 5, 20, 31, 32])
def test_merge_is_the_restatement_bit_for_bit(model, beam):
    from densecap_amd import ops
    ctx = model[0].ctx
    for nprop in (1, 70):
        for t in (1, T - 1):
            top_lp, top_idx, beam_lp, beams = _merge_case(nprop, beam, t, 100 * beam + 10 * t + nprop)
            out = ops.beam_merge(ctx, top_lp, top_idx, beam_lp, beams, t, END)
            what = "merge beam %d nprop %d t %d" % (beam, nprop, t)
            R.check_merge(out, top_lp, top_idx, beam_lp, beams, t, END, what)
            want = R.merge_ref(top_lp, top_idx, beam_lp, beams, t, END)
            cand = (top_lp + beam_lp[:, :, None]).reshape(nprop, -1)
            if beam >= 20 and nprop == 70:                            # the cases are what they claim to be
                assert any(len(np.unique(c)) < len(c) / 4 for c in cand)                       # ties everywhere
                assert want["fin"].any() and not want["fin"].all()
                assert (want["tok"] == END).any(), "END is never chosen at t"
                assert ((want["beams"][:, :, :t] == END).any(axis=2)).any(), "no chosen parent carries END already"
    if beam == 32:
        # a tie over the whole candidate array: all 1024 sums equal, the picks are flat 0..31 -- across all four 256-strides a
        # wrong tie order in any of them would surface
        top_lp = np.zeros((2, 32, 32), np.float32); beam_lp = np.full((2, 32), -1.25, np.float32)
        top_idx = np.tile(np.arange(1, 33, dtype=np.int32), (2, 32, 1))
        beams = np.ones((2, 32, T), np.int32)
        out = ops.beam_merge(ctx, top_lp, top_idx, beam_lp, beams, 1, END)
        R.check_merge(out, top_lp, top_idx, beam_lp, beams, 1, END, "flat merge")
        assert (out["parent"] == 0).all() and (out["tok"] == np.arange(1, 33)).all()
        # and with the best sums only in the last stride: parents 24..31
        beam_lp = np.where(np.arange(32) >= 24, np.float32(-0.5), np.float32(-1.25))[None].repeat(2, 0).astype(np.float32)
        out = ops.beam_merge(ctx, top_lp, top_idx, beam_lp, beams, 1, END)
        R.check_merge(out, top_lp, top_idx, beam_lp, beams, 1, END, "last-stride merge")
        assert (out["parent"] == 24).all()


# ---- c. every step, teacher-forced on the oracle's trajectory --------------------------------------------------------------------
def _teacher_forced(m, W, codes, beam, T_, V_, name):
    """The module docstring's (c) for one model and beam.  Returns (live lists, worst value difference, worst rank slack)."""
    from densecap_amd import ops
    Hd = W["lstm_w"].shape[1] // 4
    n = len(codes)
    end = V_ + 1
    walk = R.oracle_walk(codes, W, T_, beam)
    m.setBeamSize(beam)
    tol = parity.TOKEN_TOL
    state, top_lp, top_idx = ops.beam_start(m.ctx, codes, beam, Hd, T_)
    what = "%s beam %d start" % (name, beam)
    wv, ws, lists = R.check_lists(top_lp, top_idx, walk["lp0"], None, tol, what)
    R.check_same(state, R.init_ref(top_lp, top_idx, T_, end), what)
    assert (state["h"].view(np.uint32) == state["c"].view(np.uint32)).all(), "%s: h rows are not the cell rows" % what
    c0 = walk["c0"][:, None, :]
    R.check_gather(state["h"], state["c"], state["parent"], c0, c0, parity.REL, what)
    for t in range(1, T_):
        st = walk["steps"][t]
        fed = st["state"]                                            # always the oracle's, never the device's
        out, top_lp, top_idx = ops.beam_step(m.ctx, fed, t)
        what = "%s beam %d step %d" % (name, beam, t)
        v, s, k = R.check_lists(top_lp.reshape(n * beam, beam), top_idx.reshape(n * beam, beam), st["lp"], fed["fin"], tol, what)
        R.check_merge(out, top_lp, top_idx, fed["beam_lp"], fed["beams"], t, end, what)
        R.check_gather(out["h"], out["c"], out["parent"], st["h_post"], st["c_post"], parity.REL, what)
        wv, ws, lists = max(wv, v), max(ws, s), lists + k
    print("%s beam %d: %d proposals x %d steps, %d live lists, worst value difference %.3g, worst rank slack %.3g; "
          "excused 0 rows, 0 steps, 0 ranks" % (name, beam, n, T_, lists, wv, ws))
    return lists, wv, ws


@pytest.mark.parametrize("beam", [1, 5, 20, 32])
def test_every_step_teacher_forced(model, beam):
    m, W = model
    codes = np.maximum(np.random.default_rng(beam).standard_normal((N, 4096)), 0).astype(np.float32)
    lists, _, _ = _teacher_forced(m, W, codes, beam, T, V, "default")
    assert lists >= N * (1 + beam)                                   # the first two steps have no finished row at all


@pytest.mark.parametrize("name", ["minimal", "big_vocab"])
def test_every_step_teacher_forced_other_dimensions(name):
    """minimal: T = 1 (the start is the whole search), V + 1 = 6, beam 2.  big_vocab: an 80 KB LDS row, beam 3."""
    from densecap_amd import DenseCapModel
    from tests.test_gpu_dims import SETS, _oracle_codes, set_weights
    parity.oracle_threads()
    s = SETS[name]
    W = set_weights(name)
    m = DenseCapModel(W, device=0)
    try:
        lists, _, _ = _teacher_forced(m, W, _oracle_codes(N, s["D"], 0), s["beam"], s["T"], s["V"], name)
        assert lists >= N
    finally:
        m.ctx.close()


# ---- d. the hooks are the production loop ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("beam", [5, 32])
def test_chained_hooks_end_in_the_tokens_of_lm_sample(model, beam):
    """dc_debug_beam_start and T - 1 dc_debug_beam_step calls on the device's own outputs, at the default chunking (70 proposals
    advance together in both paths: the same GEMM plans): beam 0 of the last state is dc_op_lm_sample's row, bit for bit --
    which covers the ping-pong buffers and beam_best."""
    from densecap_amd import ops
    from tests.test_gpu_sample import _greedy
    m, W = model
    codes = np.maximum(np.random.default_rng(beam).standard_normal((N, 4096)), 0).astype(np.float32)
    m.setBeamSize(beam)
    seq = _greedy(m, codes)
    state, _, _ = ops.beam_start(m.ctx, codes, beam, W["lstm_w"].shape[1] // 4, T)
    for t in range(1, T):
        state, _, _ = ops.beam_step(m.ctx, state, t)
    np.testing.assert_array_equal(state["beams"][:, 0], seq)
    assert (np.diff(state["beam_lp"].astype(np.float64), axis=1) <= 0).all()
    np.testing.assert_array_equal(_greedy(m, codes), seq)            # and the hooks left the lane's scratch usable


def test_state_hooks_refuse_what_they_cannot_run(model):
    from densecap_amd import ops
    from densecap_amd._lib import DenseCapError, check
    m, W = model
    Hd = W["lstm_w"].shape[1] // 4
    codes = np.zeros((65, 4096), np.float32)
    m.setBeamSize(0)
    with pytest.raises(DenseCapError, match="dc_set_beam_size first"):
        ops.beam_start(m.ctx, codes, 2, Hd, T)
    m.setBeamSize(2)
    state, _, _ = ops.beam_start(m.ctx, codes[:3], 2, Hd, T)
    for t in (0, T):
        with pytest.raises(DenseCapError, match="is not in"):
            ops.beam_step(m.ctx, state, t)
    for word in (0, -1, END + 1):                                    # a word selects an embedding row by address
        with pytest.raises(DenseCapError, match="is not a word id"):
            ops.beam_step(m.ctx, dict(state, tok=np.full_like(state["tok"], word)), 1)
    check(m.ctx.h, m.lib.dc_debug_set(m.ctx.h, b"beam_chunk_floats", 1), "dc_debug_set")      # chunks of 64 proposals
    try:
        with pytest.raises(DenseCapError, match="not one chunk"):
            ops.beam_start(m.ctx, codes, 2, Hd, T)
    finally:
        check(m.ctx.h, m.lib.dc_debug_set(m.ctx.h, b"beam_chunk_floats", 1 << 28), "dc_debug_set")
    ops.beam_step(m.ctx, state, 1)


# ---- e. non-finite codes -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("beam", [0, 3, 32])
def test_non_finite_codes_give_the_row_no_word(model, beam):
    """The construction of test_gpu_sample.py::test_non_finite_codes_end_the_row_cleanly (its docstring accounts for the rows):
    one Inf among the codes of row 29 makes every score of its first step NaN.  The row then has no word -- seq[29][0] == 0,
    the empty caption --, every id written anywhere is in [0, V + 1], the call succeeds, the other rows are bit-identical to a
    run without the bad rows, nothing is reported through the fault word and a clean call afterwards reproduces the clean
    tokens.  Rows 3, 17 and 18 (a row of Infs, NaNs) do not reach NaN scores: the encoder's ReLU clamps them."""
    from tests.test_gpu_sample import _codes, _greedy
    m, W = model
    m.setBeamSize(beam)
    codes = _codes(40, m.fc_dim, 6)
    base = _greedy(m, codes)
    assert base.min() >= 1 and base.max() <= END
    bad = codes.copy()
    bad[3, :] = np.inf
    bad[29, 100] = np.inf
    bad[17, 5] = np.nan
    bad[18, :] = np.nan
    got = _greedy(m, bad)                                            # _lib.check: any code but DC_OK raises
    good = np.setdiff1d(np.arange(40), [3, 17, 18, 29])
    np.testing.assert_array_equal(got[good], base[good])
    assert got[29, 0] == 0 and m.decodeSequence(got[29:30]) == [""], got[29]
    assert got.min() >= 0 and got.max() <= END, (got.min(), got.max())
    assert _fault_word(m) == 0
    np.testing.assert_array_equal(_greedy(m, codes), base)
