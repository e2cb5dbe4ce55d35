"""Host-side mirror of the reference's `DenseCapModel` for the test-time path.

Same method names, argument meaning and error behaviour as
densecap/DenseCapModel.lua (setTestArgs :185-191, convert :198-208, evaluate,
forward_test :319-327, extractFeatures :285-304) and LanguageModel:decodeSequence
(LanguageModel.lua:86-103), so the callers `run_model.lua:145-164`,
`webcam/daemon.lua:46-85` and `eval/eval_utils.lua:62` change only their constructor
line.  All numerics run in libdensecap_hip.so (HIP, gfx950); this file only marshals
pointers.  The LuaJIT twin of this class is lua/DenseCapModelHIP.lua.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import DcResult, DcWeights, check
from .ops import Context


def _np32(t):
    if hasattr(t, "detach"):
        t = t.detach().cpu().numpy()
    return np.ascontiguousarray(t, dtype=np.float32)


def decode_sequence(seq, idx_to_token, vocab_size):
    """LanguageModel:decodeSequence (LanguageModel.lua:86-103): per row, join idx_to_token[tok] with ' ' until the END
    token (vocab_size + 1) or a 0.  idx_to_token: dict or list keyed by the 1-based token id (int or str keys, as the
    checkpoint's JSON-born table has them); None -> the ids themselves."""
    end = int(vocab_size) + 1
    caps = []
    for row in np.asarray(seq):
        words = []
        for tok in row:
            tok = int(tok)
            if tok == end or tok == 0:
                break
            if idx_to_token is None:
                words.append(str(tok))
            elif isinstance(idx_to_token, dict):
                words.append(idx_to_token[tok] if tok in idx_to_token else idx_to_token[str(tok)])
            else:
                words.append(idx_to_token[tok])
        caps.append(" ".join(words))
    return caps


# preprocess.py::words_preprocess: these replacements, lower case, punctuation removed, split on whitespace
_WORD_REPLACEMENTS = ((u"\u00bd", u"half"), (u"\u2014", u"-"), (u"\u2122", u""), (u"\u00a2", u"cent"), (u"\u00e7", u"c"),
                      (u"\u00fb", u"u"), (u"\u00e9", u"e"), (u"\u00b0", u" degree"), (u"\u00e8", u"e"), (u"\u2026", u""))


def words_preprocess(phrase):
    """preprocess.py::words_preprocess: replace a few characters, lower case, drop ASCII punctuation, split on whitespace."""
    import string
    for k, v in _WORD_REPLACEMENTS:
        phrase = phrase.replace(k, v)
    return phrase.lower().translate({ord(c): None for c in string.punctuation}).split()


def encode_captions(texts, idx_to_token, max_len):
    """Query phrases -> (Q, max_len) int32 of 1-based word ids, zero-padded (preprocess.py::encode_caption).  A word the
    vocabulary lacks maps to <UNK> if the vocabulary has it, else ValueError; so does a phrase of more than max_len words.
    texts: strings, or sequences of ids (taken as they are, zero-padded)."""
    if isinstance(texts, str):
        texts = [texts]
    token_to_idx = {}
    for k, v in (idx_to_token or {}).items():
        token_to_idx[str(v)] = int(k)
    out = np.zeros((len(texts), max_len), np.int32)
    for i, t in enumerate(texts):
        if isinstance(t, str):
            ids = []
            for w in words_preprocess(t):
                if w in token_to_idx:
                    ids.append(token_to_idx[w])
                elif "<UNK>" in token_to_idx:
                    ids.append(token_to_idx["<UNK>"])
                else:
                    raise ValueError("query %d: word %r is not in the vocabulary (and it has no <UNK>)" % (i, w))
        else:
            ids = [int(v) for v in np.asarray(t).reshape(-1)]
            while ids and ids[-1] == 0:
                ids.pop()
        if len(ids) > max_len:
            raise ValueError("query %d has %d words; at most %d" % (i, len(ids), max_len))
        out[i, :len(ids)] = ids
    return out


def flatten_train_state(state):
    """train_state()'s dict -> the flat .npz keys m/<name>, v/<name>, t, cnn_t"""
    flat = {"t": np.int64(state["t"]), "cnn_t": np.int64(state["cnn_t"])}
    for mom in ("m", "v"):
        for k, a in state[mom].items():
            flat["%s/%s" % (mom, k)] = np.ascontiguousarray(a, dtype=np.float32)
    return flat


def unflatten_train_state(flat):
    """the inverse of flatten_train_state on a mapping (an open .npz file serves); a key outside the scheme raises"""
    state = {"m": {}, "v": {}, "t": int(flat["t"]), "cnn_t": int(flat["cnn_t"])}
    for key in (flat.files if hasattr(flat, "files") else flat):
        if key in ("t", "cnn_t"):
            continue
        mom, _, name = key.partition("/")
        if mom not in ("m", "v") or not name:
            raise ValueError("training state: unknown key %r" % key)
        state[mom][name] = np.ascontiguousarray(flat[key], dtype=np.float32)
    return state


def getopt(opt, key, default_value=None):
    """utils.getopt (densecap/utils.lua:67-75): opt[key], or the default when the key is absent / nil (None here);
    a missing key without a default is an error, as in the reference."""
    v = None if opt is None else opt.get(key)
    if v is None:
        if default_value is None:
            raise KeyError("error: required key %s was not provided in an opt." % key)
        return default_value
    return v


class LocalizationLayerTestArgs:
    """`model.nets.localization_layer` as far as the test-time path reads it: the three fields that
    LocalizationLayer:setTestArgs writes (LocalizationLayer.lua:233-238) and _forward_test reads (:250-256).  A call
    re-derives ALL three -- an omitted key goes back to its default (true / 0.7 / 300), it is not retained."""

    def __init__(self, stored=None):
        self.setTestArgs()                               # LocalizationLayer.lua:155: the constructor's own call
        for k in ("test_clip_boxes", "test_nms_thresh", "test_max_proposals"):
            if stored and stored.get(k) is not None:     # the deserialised object's fields (a checkpoint stores them)
                setattr(self, k, stored[k])

    def setTestArgs(self, args=None, **kw):
        args = dict(args or {}, **kw)
        self.test_clip_boxes = bool(getopt(args, "clip_boxes", True))
        self.test_nms_thresh = float(getopt(args, "nms_thresh", 0.7))
        self.test_max_proposals = int(getopt(args, "max_proposals", 300))
        return self


class _Nets:
    def __init__(self, localization_layer):
        self.localization_layer = localization_layer


class DenseCapModel:
    def __init__(self, weights, device=0, ctx=None):
        """weights: dict in checkpoint layouts (see densecap_amd/weights.py); device: HIP index
        (utils.setup_gpus(gpu) with gpu >= 0; there is no `-gpu -1` CPU mode here).
        weights["test_args"] (optional; t7.weights_from_checkpoint fills it): the test-time state the checkpoint OBJECT
        carries -- localization_layer.test_clip_boxes / test_nms_thresh / test_max_proposals and opt.final_nms_thresh --
        which is what the model runs with until somebody calls setTestArgs."""
        from .weights import check_weight_shapes
        check_weight_shapes(weights)                  # before any pointer crosses the ABI: dc_load_weights trusts the shapes
        self.ctx = ctx or Context(device)
        self.lib = self.ctx.lib
        stored = dict(weights.get("test_args") or {})
        self.nets = _Nets(LocalizationLayerTestArgs(stored))
        # DenseCapModel.lua:31: opt.final_nms_thresh defaults to 0.3 at construction; forward reads self.opt at call time
        self.opt = dict(final_nms_thresh=float(getopt(stored, "final_nms_thresh", 0.3)))
        self.vocab_size = int(weights["vocab_size"])
        self.seq_length = int(weights["seq_length"])
        self.idx_to_token = weights.get("idx_to_token")
        self.captions_after_final_nms = False
        self._keep = []  # host arrays referenced by the struct during dc_load_weights
        w = DcWeights()

        def ptr(a):
            a = _np32(a)
            self._keep.append(a)
            return a.ctypes.data_as(_lib.c_float_p)

        for i in range(_lib.DC_NUM_VGG_CONVS):
            w.conv_w[i] = ptr(weights["conv_w"][i])
            w.conv_b[i] = ptr(weights["conv_b"][i])
        for name in ("rpn_conv_w", "rpn_conv_b", "rpn_box_w", "rpn_box_b", "rpn_score_w", "rpn_score_b", "fc6_w",
                     "fc6_b", "fc7_w", "fc7_b", "obj_w", "obj_b", "boxreg_w", "boxreg_b", "lm_enc_w", "lm_enc_b",
                     "lm_emb", "lstm_w", "lstm_b", "lm_out_w", "lm_out_b", "anchors"):
            setattr(w, name, ptr(weights[name]))
        for i, v in enumerate(weights["field_centers"]):
            w.field_centers[i] = float(v)
        w.num_anchors = int(_np32(weights["anchors"]).shape[1])
        self.num_anchors = int(w.num_anchors)
        w.rpn_hidden = int(_np32(weights["rpn_conv_w"]).shape[0])
        w.vocab_size = self.vocab_size
        w.seq_length = self.seq_length
        w.enc_size = int(_np32(weights["lm_enc_w"]).shape[0])
        w.rnn_size = int(_np32(weights["lstm_w"]).shape[1] // 4)
        w.fc_dim = int(_np32(weights["fc7_w"]).shape[0])
        self.fc_dim = w.fc_dim
        check(self.ctx.h, self.lib.dc_load_weights(self.ctx.h, C.byref(w)), "dc_load_weights")
        self.ctx.seq_length = self.seq_length          # ops.lm_sample_n sizes its outputs by it
        self.ctx.lm_dims = dict(E=int(w.enc_size), Hd=int(w.rnn_size), D=int(w.fc_dim), V=self.vocab_size, k=int(w.num_anchors),
                                R=int(w.rpn_hidden))   # ops.lm_grad, ops.recog_grad, ops.rpn_grad: their buffers
        self._keep = []
        # what get_weights needs to hand the weights back in the shapes they came in, and the keys it passes through
        self._weight_shapes = {n: tuple(_np32(weights[n]).shape) for n in
                               ("rpn_conv_w", "rpn_conv_b", "rpn_box_w", "rpn_box_b", "rpn_score_w", "rpn_score_b", "fc6_w", "fc6_b",
                                "fc7_w", "fc7_b", "obj_w", "obj_b", "boxreg_w", "boxreg_b", "lm_enc_w", "lm_enc_b", "lm_emb", "lstm_w",
                                "lstm_b", "lm_out_w", "lm_out_b", "anchors")}
        self._weight_shapes["conv_w"] = [tuple(_np32(a).shape) for a in weights["conv_w"]]
        self._weight_shapes["conv_b"] = [tuple(_np32(a).shape) for a in weights["conv_b"]]
        self._weight_meta = {"field_centers": tuple(float(v) for v in weights["field_centers"]), "vocab_size": self.vocab_size,
                             "seq_length": self.seq_length, "idx_to_token": self.idx_to_token}
        self._push_test_args()

    # ---- reference API ---------------------------------------------------------------------
    def setTestArgs(self, args=None, **kw):
        """DenseCapModel:setTestArgs{rpn_nms_thresh=, final_nms_thresh=, num_proposals=} (DenseCapModel.lua:185-191), as
        written: EVERY call re-derives all three values -- rpn 0.7, num_proposals 1000, final 0.3 for the keys that are
        absent -- and, because it calls the layer's setTestArgs without a `clip_boxes` key, turns box clipping back on.
        Keys it does not know are ignored (evaluate_model.lua:39-43 passes `max_proposals=`, which the reference never
        reads: that caller runs with 1000 proposals)."""
        kwargs = dict(args or {}, **kw)
        ll = self.nets.localization_layer
        # a value the library refuses (num_proposals = 0, 2000000 ...) must not stay behind in the object: every later
        # forward would re-raise in _push_test_args (advisor finding, round 4).  The previous state comes back on failure.
        saved = (ll.test_clip_boxes, ll.test_nms_thresh, ll.test_max_proposals, self.opt["final_nms_thresh"])
        try:
            ll.setTestArgs(nms_thresh=getopt(kwargs, "rpn_nms_thresh", 0.7),
                           max_proposals=getopt(kwargs, "num_proposals", 1000))
            self.opt["final_nms_thresh"] = float(getopt(kwargs, "final_nms_thresh", 0.3))
            self._push_test_args()
        except Exception:
            ll.test_clip_boxes, ll.test_nms_thresh, ll.test_max_proposals, self.opt["final_nms_thresh"] = saved
            raise
        return self

    def _push_test_args(self):
        """The reference reads localization_layer.test_* and opt.final_nms_thresh when forward runs
        (LocalizationLayer.lua:250-256, DenseCapModel.lua:261) -- callers such as train.lua:139-143 write them directly --
        so the current values travel to the library before every forward."""
        ll = self.nets.localization_layer
        check(self.ctx.h, self.lib.dc_set_test_args(self.ctx.h, float(ll.test_nms_thresh),
                                                    float(self.opt["final_nms_thresh"]),
                                                    int(ll.test_max_proposals)), "dc_set_test_args")
        if not ll.test_clip_boxes:
            check(self.ctx.h, self.lib.dc_set_localization_test_args(self.ctx.h, 0, float(ll.test_nms_thresh),
                                                                     int(ll.test_max_proposals)),
                  "dc_set_localization_test_args")

    def setLanes(self, lanes):
        """Streams dc_forward_batch pipelines images over (1 = serial kernels)."""
        check(self.ctx.h, self.lib.dc_set_lanes(self.ctx.h, int(lanes)), "dc_set_lanes")
        return self

    def autotuneLanes(self, dev_ptr, n, H, W, candidates=(2, 3, 4), reps=2):
        """Pick the number of lanes (>= 2: all give bit-identical results, only the overlap of the images' kernels
        changes) that gives the best throughput on THIS device for n resident images; which count wins differs
        between otherwise identical GPUs (measured: 3 lanes 171 vs 2 lanes 162 images/s on one box, 160 vs 167 on
        another).  Returns {lanes: images/s}; the best one is left set."""
        import time
        rates = {}
        for lanes in candidates:
            self.setLanes(lanes)
            self.forward_batch_device(dev_ptr, min(n, lanes), H, W)          # lane workspaces exist before timing
            best = 0.0
            for _ in range(reps):
                t0 = time.perf_counter()
                self.forward_batch_device(dev_ptr, n, H, W)
                best = max(best, n / (time.perf_counter() - t0))
            rates[lanes] = best
        self.setLanes(max(rates, key=rates.get))
        return rates

    def autotuneSchedule(self, dev_ptr, n, H, W, lanes=(2, 3, 4), groups=(1, 2, 4, 8), reps=2):
        """Pick the lane count AND the images per group together (both are pure scheduling knobs: results are bit-identical
        for any lanes >= 2 and any group): the best lane count depends on the group size -- 300 proposals: 2 lanes x groups
        of four 312 images/s, 4 lanes x groups of four 299, 2 lanes x single images 285.  Returns {(lanes, group): images/s};
        the best pair is left set."""
        import time
        rates = {}
        for l in lanes:
            for g in groups:
                self.setLanes(l); self.setGroup(g)
                self.forward_batch_device(dev_ptr, min(n, l * g), H, W)      # workspaces of this shape exist before timing
                best = 0.0
                for _ in range(reps):
                    t0 = time.perf_counter()
                    self.forward_batch_device(dev_ptr, n, H, W)
                    best = max(best, n / (time.perf_counter() - t0))
                rates[(l, g)] = best
        l, g = max(rates, key=rates.get)
        self.setLanes(l); self.setGroup(g)
        return rates

    def autotuneGroup(self, dev_ptr, n, H, W, candidates=(1, 2, 4, 8), reps=2):
        """Pick the images-per-group setting (dc_set_group: a scheduling knob like the lane count -- results are
        bit-identical) at the current lane count.  With few proposals per image the RoI stages of one image leave the
        chip's tile rounds badly filled and a group of four shares them (300 proposals: +9 % images/s at two lanes); at
        1000 proposals groups change nothing.  Returns {group: images/s}; the best one is left set."""
        import time
        rates = {}
        for g in candidates:
            self.setGroup(g)
            self.forward_batch_device(dev_ptr, min(n, 2 * g), H, W)
            best = 0.0
            for _ in range(reps):
                t0 = time.perf_counter()
                self.forward_batch_device(dev_ptr, n, H, W)
                best = max(best, n / (time.perf_counter() - t0))
            rates[g] = best
        self.setGroup(max(rates, key=rates.get))
        return rates

    def setCaptionOrder(self, after_final_nms):
        """False (default): decode all proposals then NMS, as the reference does.  True: final NMS first,
        decode only the survivors (bit-identical outputs, less LSTM work)."""
        check(self.ctx.h, self.lib.dc_set_caption_order(self.ctx.h, int(bool(after_final_nms))), "dc_set_caption_order")
        self.captions_after_final_nms = bool(after_final_nms)
        return self

    def setMathMode(self, mode):
        """dc_set_math_mode: 0 = fp32 MFMA (default; the arithmetic results are bit-compared in), 1 = split-bf16 (every
        operand as three bf16 planes, six partial products on the bf16 matrix cores, fp32 accumulate: fp32-class error at
        2.67x the matrix rate).  Opt-in; may be switched between forwards."""
        check(self.ctx.h, self.lib.dc_set_math_mode(self.ctx.h, int(mode)), "dc_set_math_mode")
        self.math_mode = int(mode)
        return self

    def setGraphReplay(self, on):
        """dc_set_graph_replay: repeated forwards of one shape on a lane are captured once and relaunched as a hipGraph
        (bit-identical; pays with one image in flight -- run_model on single images, the webcam daemon)."""
        check(self.ctx.h, self.lib.dc_set_graph_replay(self.ctx.h, int(bool(on))), "dc_set_graph_replay")
        return self

    def setGroup(self, images):
        """Images per group inside a batch call: 0/1 = every image on its own (default), 2..8 = the images of a group share
        the launches of the dense stages (bit-identical results; 1000 proposals: +4.5 % images/s on one lane, nothing with
        two or more lanes; 300 proposals: +9 % at two lanes with groups of four)."""
        check(self.ctx.h, self.lib.dc_set_group(self.ctx.h, int(images)), "dc_set_group")
        return self

    def setBeamSize(self, beam_size):
        """language_model.beam_size (LanguageModel.lua:129-131): None/0 = greedy sample, n = beam search with n beams."""
        check(self.ctx.h, self.lib.dc_set_beam_size(self.ctx.h, int(beam_size or 0)), "dc_set_beam_size")
        return self

    def convert(self, dtype=None, use_cudnn=None):
        """model:convert(dtype, use_cudnn): the HIP path is always fp32 on the ctx's device."""
        return self

    def evaluate(self):
        return self

    def _check_input(self, img):
        img = np.asarray(img)
        if img.ndim == 4:
            assert img.shape[0] == 1 and img.shape[1] == 3, "input must be (1,3,H,W)"  # DenseCapModel.lua:244
            img = img[0]
        assert img.ndim == 3 and img.shape[0] == 3, "input must be (1,3,H,W)"
        return np.ascontiguousarray(img, dtype=np.float32)

    def _new_result(self, P):
        T = self.seq_length
        boxes = np.zeros((P, 4), np.float32); scores = np.zeros((P,), np.float32)
        tokens = np.zeros((P, T), np.int32)
        r = DcResult()
        r.capacity = P
        r.boxes = boxes.ctypes.data_as(_lib.c_float_p)
        r.scores = scores.ctypes.data_as(_lib.c_float_p)
        r.tokens = tokens.ctypes.data_as(_lib.c_int32_p)
        return r, boxes, scores, tokens

    def _capacity(self, H, W):
        P = int(self.nets.localization_layer.test_max_proposals)
        if P != -1:
            return P
        for _ in range(4):                       # four ceil-mode 2x2 pools (conv5_3 map)
            H, W = (H + 1) // 2, (W + 1) // 2
        return self.num_anchors * H * W

    def _results(self, caps, copy=True):
        """A DcResult array for images of these capacities, and a function that slices each image's K rows back after the
        call: [(boxes, scores, tokens)], copies or (copy=False) views of the arrays the library wrote."""
        made = [self._new_result(P) for P in caps]
        res = (DcResult * len(made))(*[m[0] for m in made])

        def rows():
            return [tuple(x[:r.K].copy() if copy else x[:r.K] for x in m[1:]) for r, m in zip(res, made)]
        return res, rows

    @staticmethod
    def _image_list(imgs):
        """(pointers, H, W) ctypes arrays of a list of (3,H,W) host arrays or ops.DeviceArrays."""
        n = len(imgs)
        ptrs = (C.c_void_p * n)(*[a.ctypes.data if isinstance(a, np.ndarray) else a.ptr.value for a in imgs])
        return ptrs, (C.c_int * n)(*[a.shape[1] for a in imgs]), (C.c_int * n)(*[a.shape[2] for a in imgs])

    def forward_raw(self, img):
        """forward_test without string decoding: (boxes (K,4) xcycwh, scores (K,), tokens (K,T))."""
        self._push_test_args()
        img = self._check_input(img)
        res, rows = self._results([self._capacity(img.shape[1], img.shape[2])])
        check(self.ctx.h, self.lib.dc_forward_test(self.ctx.h, img.ctypes.data, img.shape[1], img.shape[2], 0, res),
              "dc_forward_test")
        return rows()[0]

    def forward_test(self, img):
        """Returns final_boxes (K,4), objectness_scores (K,1), captions (list of K strings)."""
        boxes, scores, tokens = self.forward_raw(img)
        return boxes, scores[:, None], self.decodeSequence(tokens)

    def forward_batch_device(self, imgs_dev_ptr, n, H, W):
        """run_model.lua's image loop over n device-resident images of one size; returns a list of
        (boxes, scores, tokens).  imgs_dev_ptr: device pointer to (n,3,H,W) fp32."""
        self._push_test_args()
        res, rows = self._results([self._capacity(H, W)] * n, copy=False)
        check(self.ctx.h, self.lib.dc_forward_batch(self.ctx.h, imgs_dev_ptr, n, H, W, 1, res), "dc_forward_batch")
        return rows()

    def forward_batch(self, imgs):
        self._push_test_args()
        imgs = np.ascontiguousarray(imgs, dtype=np.float32)
        n, c, H, W = imgs.shape
        assert c == 3
        res, rows = self._results([self._capacity(H, W)] * n)
        check(self.ctx.h, self.lib.dc_forward_batch(self.ctx.h, imgs.ctypes.data, n, H, W, 0, res), "dc_forward_batch")
        return rows()

    def forward_images(self, imgs):
        """run_model.lua's loop over a list of images of DIFFERENT sizes, pipelined over the lanes (dc_forward_images);
        imgs: sequence of (3,H,W) / (1,3,H,W) arrays.  Returns a list of (boxes, scores, tokens)."""
        self._push_test_args()
        return self._forward_images([self._check_input(im) for im in imgs], 0)

    def forward_images_device(self, dev_imgs):
        """forward_images on images that are ALREADY on the device: dev_imgs = sequence of ops.DeviceArray (3,H,W) float32
        (ops.preprocess_u8 makes them).  Runs of equal-sized images travel as groups (setGroup)."""
        self._push_test_args()
        return self._forward_images(dev_imgs, 1)

    def _forward_images(self, imgs, on_device):
        if len(imgs) == 0:
            return []
        res, rows = self._results([self._capacity(a.shape[1], a.shape[2]) for a in imgs])
        check(self.ctx.h, self.lib.dc_forward_images(self.ctx.h, *self._image_list(imgs), len(imgs), on_device, res),
              "dc_forward_images")
        return rows()

    # ---- caller-supplied boxes (dc_forward_boxes*, docs/SEMANTICS.md "Caller-supplied boxes") -----------------------------
    @staticmethod
    def _box_lists(boxes_list, caps):
        """A DcBoxList array for one (n,4) xcycwh box array per image, each checked as the library checks it (1 <= n <=
        capacity, finite coordinates, w, h > 0), the int32 `src` arrays the library fills, and the fp32 box arrays (to be
        kept alive over the call)."""
        kept, srcs = [], []
        bl = (_lib.DcBoxList * len(caps))()
        for i, (b, P) in enumerate(zip(boxes_list, caps)):
            b = _np32(b)
            if b.ndim != 2 or b.shape[1] != 4 or b.shape[0] < 1:
                raise ValueError("image %d: boxes must be (n,4) xc,yc,w,h with n >= 1 (got shape %s)" % (i, b.shape))
            if b.shape[0] > P:
                raise ValueError("image %d: %d boxes exceed the row capacity %d of a forward; raise num_proposals "
                                 "(setTestArgs)" % (i, b.shape[0], P))
            bad = np.flatnonzero(~(np.isfinite(b).all(axis=1) & (b[:, 2] > 0) & (b[:, 3] > 0)))
            if bad.size:
                raise ValueError("image %d: box %d %s needs finite xc, yc and finite w, h > 0" % (i, bad[0], b[bad[0]].tolist()))
            src = np.full((P,), -1, np.int32)
            bl[i].boxes = b.ctypes.data_as(_lib.c_float_p)
            bl[i].n = b.shape[0]
            bl[i].src = src.ctypes.data_as(_lib.c_int32_p)
            kept.append(b); srcs.append(src)
        return bl, srcs, kept

    def _forward_boxes(self, imgs, boxes_list, on_device, clip, single=False):
        if len(boxes_list) != len(imgs):
            raise ValueError("%d images but %d box lists" % (len(imgs), len(boxes_list)))
        if len(imgs) == 0:
            return []
        caps = [self._capacity(a.shape[1], a.shape[2]) for a in imgs]
        bl, srcs, _kept = self._box_lists(boxes_list, caps)
        res, rows = self._results(caps)
        flags = _lib.DC_BOXES_CLIP if clip else 0
        ptrs, H, W = self._image_list(imgs)
        if single:
            check(self.ctx.h, self.lib.dc_forward_boxes(self.ctx.h, ptrs[0], H[0], W[0], on_device, bl, flags, res),
                  "dc_forward_boxes")
        else:
            check(self.ctx.h, self.lib.dc_forward_boxes_images(self.ctx.h, ptrs, H, W, len(imgs), on_device, bl, flags, res),
                  "dc_forward_boxes_images")
        return [r + (s[:len(r[0])].copy(),) for r, s in zip(rows(), srcs)]

    def forward_boxes(self, img, boxes, clip=False):
        """The model after the RPN on the caller's boxes (dc_forward_boxes): boxes (n,4) xc,yc,w,h in the pixel frame of
        `img` (the frame forward_raw returns), 1 <= n <= num_proposals.  clip: box_utils.clip_boxes first, invalid boxes
        dropped (not for boxes that came out of the library: the reference's clip takes a pixel off w and h every time).
        Returns (boxes (K,4), scores (K,), tokens (K,T), src (K,)): src[r] = the row of `boxes` behind result row r; rows
        are in input order when final_nms_thresh <= 0, else in decreasing objectness after the final NMS."""
        self._push_test_args()
        return self._forward_boxes([self._check_input(img)], [boxes], 0, clip, single=True)[0]

    def forward_boxes_device(self, dev_img, boxes, clip=False):
        """forward_boxes on an image that is already on the device (ops.DeviceArray (3,H,W) float32); boxes stay host memory."""
        self._push_test_args()
        return self._forward_boxes([dev_img], [boxes], 1, clip, single=True)[0]

    def forward_boxes_images(self, imgs, boxes_list, clip=False):
        """forward_boxes over a list of images of any sizes, boxes_list[i] the boxes of imgs[i] (dc_forward_boxes_images:
        pipelined over the lanes, equal-sized runs grouped).  Returns a list of (boxes, scores, tokens, src)."""
        self._push_test_args()
        return self._forward_boxes([self._check_input(im) for im in imgs], list(boxes_list), 0, clip)

    def forward_boxes_images_device(self, dev_imgs, boxes_list, clip=False):
        """forward_boxes_images on device-resident images (ops.preprocess_u8)."""
        self._push_test_args()
        return self._forward_boxes(list(dev_imgs), list(boxes_list), 1, clip)

    def _extract_features_boxes(self, imgs, boxes_list, on_device, clip):
        n = len(imgs)
        if len(boxes_list) != n:
            raise ValueError("%d images but %d box lists" % (n, len(boxes_list)))
        if n == 0:
            return []
        caps = [self._capacity(a.shape[1], a.shape[2]) for a in imgs]
        bl, srcs, _kept = self._box_lists(boxes_list, caps)
        cap = max(b.n for b in bl)                       # rows per image of the output arrays: no image returns more than it passed
        boxes = np.zeros((n, cap, 4), np.float32); feats = np.zeros((n, cap, self.fc_dim), np.float32)
        K = np.zeros((n,), np.int32)
        check(self.ctx.h, self.lib.dc_extract_features_boxes(self.ctx.h, *self._image_list(imgs), n, on_device, bl,
                                                             _lib.DC_BOXES_CLIP if clip else 0, cap, boxes.ctypes.data,
                                                             feats.ctypes.data, K.ctypes.data_as(_lib.c_int32_p)),
              "dc_extract_features_boxes")
        return [(boxes[i, :K[i]].copy(), feats[i, :K[i]].copy(), srcs[i][:K[i]].copy()) for i in range(n)]

    def extractFeatures_boxes(self, imgs, boxes_list, clip=False):
        """fc7 codes of the caller's boxes (dc_extract_features_boxes): list of (boxes after regression (K,4), feats
        (K,fc_dim), src (K,)) per image.  The final NMS runs as in extractFeatures, except that final_nms_thresh <= 0 means
        none: every box, in input order (src = 0..n-1)."""
        self._push_test_args()
        return self._extract_features_boxes([self._check_input(im) for im in imgs], list(boxes_list), 0, clip)

    def extractFeatures_boxes_device(self, dev_imgs, boxes_list, clip=False):
        """extractFeatures_boxes on device-resident images."""
        self._push_test_args()
        return self._extract_features_boxes(list(dev_imgs), list(boxes_list), 1, clip)

    def extractFeatures_images_device(self, dev_imgs):
        """extractFeatures_images on device-resident images (ops.preprocess_u8): list of (boxes, feats)."""
        self._push_test_args()
        return self._extract_features_images(dev_imgs, 1)

    def _extract_features_images(self, imgs, on_device):
        n = len(imgs)
        if n == 0:
            return []
        cap = max(self._capacity(a.shape[1], a.shape[2]) for a in imgs)
        boxes = np.zeros((n, cap, 4), np.float32); feats = np.zeros((n, cap, self.fc_dim), np.float32)
        K = np.zeros((n,), np.int32)
        check(self.ctx.h, self.lib.dc_extract_features_images(self.ctx.h, *self._image_list(imgs), n, on_device, cap,
                                                              boxes.ctypes.data, feats.ctypes.data,
                                                              K.ctypes.data_as(_lib.c_int32_p)),
              "dc_extract_features_images")
        return [(boxes[i, :K[i]].copy(), feats[i, :K[i]].copy()) for i in range(n)]

    def extractFeatures(self, img):
        """DenseCapModel:extractFeatures -> (boxes_xcycwh (K,4), feats (K,fc_dim))."""
        self._push_test_args()
        img = self._check_input(img)
        P = self._capacity(img.shape[1], img.shape[2])
        boxes = np.zeros((P, 4), np.float32); feats = np.zeros((P, self.fc_dim), np.float32)
        K = C.c_int32(0)
        check(self.ctx.h, self.lib.dc_extract_features(self.ctx.h, img.ctypes.data, img.shape[1], img.shape[2], 0, P,
                                                       boxes.ctypes.data, feats.ctypes.data, C.byref(K)),
              "dc_extract_features")
        return boxes[:K.value].copy(), feats[:K.value].copy()

    def extractFeatures_images(self, imgs):
        """extract_features.lua's loop over images (any sizes), pipelined over the lanes: list of (boxes, feats)."""
        self._push_test_args()
        return self._extract_features_images([self._check_input(im) for im in imgs], 0)

    def scoreCaptions(self, img, captions, return_captions=False, max_len=None):
        """Score query phrases against the image's regions (dc_score_captions): the regions forward_test returns, each with
        log p(query | region) under the language model, teacher-forced (LanguageModel.lua:106-127, targets :148-167).
        captions: strings (encoded by encode_captions) or id rows.  Returns (boxes (K,4) xcycwh, scores (K,), loglik (K,Q)),
        plus the regions' own captions when return_captions."""
        self._push_test_args()
        q = self._encode_queries(captions, max_len)
        img = self._check_input(img)
        P = self._capacity(img.shape[1], img.shape[2])
        r, boxes, scores, tokens = self._new_result(P)
        if not return_captions:
            r.tokens = None
        Q, Tq = q.shape
        loglik = np.zeros((P, max(Q, 1)), np.float32)
        check(self.ctx.h, self.lib.dc_score_captions(self.ctx.h, img.ctypes.data, img.shape[1], img.shape[2], 0,
                                                     q.ctypes.data, Q, Tq, C.byref(r), loglik.ctypes.data),
              "dc_score_captions")
        K = r.K
        res = (boxes[:K].copy(), scores[:K].copy(), loglik[:K, :Q].copy())
        if return_captions:
            res = res + (self.decodeSequence(tokens[:K]),)
        return res

    def forward_losses(self, img, gt_boxes, gt_labels, **opts):
        """The validation losses of one image: what DenseCapModel:forward_backward returns (DenseCapModel.lua:401-474) and
        eval_utils.eval_split averages -- mid_objectness_loss, mid_box_reg_loss, end_objectness_loss, end_box_reg_loss,
        captioning_loss, total_loss -- from the forward half alone, Dropout as set_dropout says (none by default; docs/SEMANTICS.md,
        "Validation losses", "Dropout").  gt_boxes (G,4) xcycwh in the frame of the image passed, gt_labels (G,L) word ids padded with zeros.  opts: the
        sampler's settings and the five weights (ops.LOSS_DEFAULTS), forced_pos / forced_neg, dump.  The test arguments
        (setTestArgs) play no part."""
        from . import ops
        return ops.forward_losses(self.ctx, self._check_input(img), gt_boxes, gt_labels, **opts)

    def loss_gradients(self, img, gt_boxes, gt_labels, **opts):
        """forward_losses (same arguments, the same numbers) and the gradient of end_objectness + end_box_reg + captioning with
        respect to every parameter downstream of the RPN (dc_loss_gradients; docs/SEMANTICS.md, "Recognition-net gradients"):
        the six losses and the counts, the eight recognition tensors (fc6_w, fc6_b, fc7_w, fc7_b, obj_w, obj_b, boxreg_w,
        boxreg_b) and the seven language-model tensors in checkpoint layouts, `feat` (512, h, w) -- RoI pooling's share of the
        feature map's gradient, the reference's layout --, `roi_boxes` (num_pos + num_neg, 4) and `codes` (num_pos, fc_dim), the
        language model's gradient of the positive codes.  The CNN backward is not run here (ops.cnn_grad is a call of its own); the loaded weights do not
        change."""
        from . import ops
        return ops.loss_gradients(self.ctx, self._check_input(img), gt_boxes, gt_labels, **opts)

    def forward_backward(self, img, gt_boxes, gt_labels, box_reg_decay=5e-5, cnn=False, **opts):
        """DenseCapModel:forward_backward (DenseCapModel.lua:401-474) with the reference's default -finetune_cnn_after -1
        (dc_forward_backward; docs/SEMANTICS.md, "RPN gradients"): loss_gradients' dict (same arguments, the same numbers) plus
        the gradients of the RPN's six tensors (rpn_conv_w, rpn_conv_b, rpn_box_w, rpn_box_b, rpn_score_w, rpn_score_b) in
        checkpoint layouts -- the two mid criteria and box_reg_decay (train_opts.lua:42) through the sampler's backward, the
        heads and the RPN's convolution.  `feat` (512, h, w) is now the complete grad_cnn_features, `feat_roi` and `feat_rpn`
        its two shares.  Together: the gradient of all five criteria with respect to all 21 tensors outside the CNN.  cnn=True
        (dc_forward_backward_cnn, the reference with model.finetune_cnn; "CNN gradients"): the same dict bit for bit plus
        conv_w4 .. conv_w12 and conv_b4 .. conv_b12, the gradients of conv3_1 .. conv5_3.  The loaded weights do not change
        (train_step is the call that updates them; it does not train the CNN)."""
        from . import ops
        return ops.forward_backward(self.ctx, self._check_input(img), gt_boxes, gt_labels, box_reg_decay=box_reg_decay, cnn=cnn, **opts)

    # ---- training (docs/SEMANTICS.md, "Dropout", "Training step") -----------------------------------------------------------
    def set_dropout(self, p):
        """dc_set_dropout: p of the two Dropout layers of the training forward (after fc6's ReLU and after fc7's; models.lua's
        drop_prob, 0.5 in train_opts.lua).  0, the default: none.  A float in [0, 1).  Read by forward_losses, loss_gradients,
        forward_backward, train_step and ops.recog_grad, whose masks follow their `seed`; inference never drops."""
        check(self.ctx.h, self.lib.dc_set_dropout(self.ctx.h, float(p)), "dc_set_dropout")
        return self

    @property
    def dropout(self):
        """dc_get_dropout: the p in force."""
        p = C.c_float(0.0)
        check(self.ctx.h, self.lib.dc_get_dropout(self.ctx.h, C.byref(p)), "dc_get_dropout")
        return float(p.value)

    def train_begin(self, **opts):
        """dc_train_begin: Adam's moments (zero) and the gradient arena for the 21 tensors outside the CNN; the step count
        starts at 0.  opts: learning_rate 1e-5, beta1 0.9, beta2 0.999, epsilon 1e-8, weight_decay 1e-6 (train_opts.lua)."""
        from . import ops
        ops.train_begin(self.ctx, **opts)

    def train_set_cnn(self, mode):
        """dc_train_set_cnn (train.lua's -finetune_cnn_after): 0 = the CNN is left alone, 1 = decay and Adam on conv3_1 .. conv5_3
        with a zero gradient, 2 = the full CNN backward, decay and Adam; the CNN keeps an Adam step count of its own."""
        from . import ops
        ops.train_set_cnn(self.ctx, mode)

    def train_step(self, img, gt_boxes, gt_labels, box_reg_decay=5e-5, **opts):
        """One iteration of train.lua's loop body (train.lua:163-185) on one image: forward_backward (same arguments; the dict
        returned holds its six losses and the counts, for the weights as they were), grad_params:add(weight_decay, params), adam
        (optim_updates.lua:56-84) on the device, and the refresh of everything derived from a trained weight.  Dropout is
        set_dropout's (none by default); the CNN is trained only after train_set_cnn."""
        from . import ops
        return ops.train_step(self.ctx, self._check_input(img), gt_boxes, gt_labels, box_reg_decay=box_reg_decay, **opts)

    def train_end(self):
        """dc_train_end: frees the moments and the arena; the weights stay as trained."""
        from . import ops
        ops.train_end(self.ctx)

    def train_set_grad_clip(self, max_norm):
        """dc_train_set_grad_clip (docs/SEMANTICS.md, "Gradient clipping"): every later train_step clips its gradient by the
        global L2 norm -- scale = min(1, max_norm / (norm + 1e-6)) on all trained tensors at once -- and its dict gains
        `grad_norm` and `grad_scale`.  0 (the default after train_begin): off; inf: the norm is reported, nothing is scaled."""
        from . import ops
        ops.train_set_grad_clip(self.ctx, max_norm)

    def train_state(self):
        """Adam's state (dc_train_get_state): {"m": {name: array}, "v": {name: array}, "t": int, "cnn_t": int}, numpy arrays in
        the checkpoint's layouts under get_weights' names; the CNN's moments (conv_w4 .. conv_b12) once train_set_cnn made them."""
        from . import ops
        return ops.train_get_state(self.ctx, self._weight_shapes)

    def train_load_state(self, state):
        """dc_train_set_state: continue from train_state()'s dict (after train_begin on the weights saved with it)."""
        from . import ops
        ops.train_set_state(self.ctx, state, self._weight_shapes)

    def save_train_state(self, path):
        """train_state() as an uncompressed .npz with the flat keys m/<name>, v/<name>, t, cnn_t (1.1 GB at the real model)."""
        np.savez(path, **flatten_train_state(self.train_state()))

    def load_train_state(self, path):
        """train_load_state of a file save_train_state wrote; returns (t, cnn_t)."""
        with np.load(path) as z:
            state = unflatten_train_state(z)
        self.train_load_state(state)
        return state["t"], state["cnn_t"]

    def get_weights(self, conv=True):
        """The current weights as a dict in the keys of densecap_amd/weights.py (dc_get_weights), float32 numpy arrays in the
        shapes the model was built from; conv=False leaves the 13 CNN layers out (they are not trained)."""
        from . import ops
        W = ops.get_weights(self.ctx, self._weight_shapes, conv=conv)
        W.update(self._weight_meta)
        W["test_args"] = dict(test_clip_boxes=bool(self.nets.localization_layer.test_clip_boxes),
                              test_nms_thresh=float(self.nets.localization_layer.test_nms_thresh),
                              test_max_proposals=int(self.nets.localization_layer.test_max_proposals),
                              final_nms_thresh=float(self.opt["final_nms_thresh"]))
        return W

    def save_checkpoint(self, path):
        """torch.save(path, {model = ...}) of the current weights (t7.checkpoint_from_weights, t7.save)."""
        from . import t7
        t7.save(path, t7.checkpoint_from_weights(self.get_weights()))

    def lm_gradients(self, codes, labels, weight=1.0):
        """The captioning loss of n (fc7 code, caption) pairs and its gradients with respect to the seven language-model tensors
        (checkpoint layouts) and the codes (dc_op_lm_grad; docs/SEMANTICS.md, "Language-model gradients"): a dict of numpy
        arrays plus `loss` and `rowlik`.  labels (n, L) word ids padded with zeros.  The loaded weights do not change."""
        from . import ops
        return ops.lm_grad(self.ctx, codes, labels, weight)

    def caption_gradients(self, img, boxes, labels):
        """lm_gradients for the caller's boxes on an image: the fc7 codes of the boxes (xcycwh) through the caller-supplied-boxes
        path without a final NMS, so that row i is box i, then lm_gradients(codes, labels)."""
        labels = np.ascontiguousarray(labels, dtype=np.int32)
        saved = self.opt["final_nms_thresh"]
        self.opt["final_nms_thresh"] = 0.0
        try:
            (_b, feats, src), = self.extractFeatures_boxes([img], [boxes])
        finally:
            self.opt["final_nms_thresh"] = saved
            self._push_test_args()
        if len(feats) != len(labels) or not np.array_equal(src, np.arange(len(labels))):
            raise ValueError("caption_gradients: %d boxes came back for %d label rows" % (len(feats), len(labels)))
        return self.lm_gradients(feats, labels)

    def _encode_queries(self, captions, max_len=None):
        """strings (encode_captions, max_len words wide or as wide as the longest) or ready (Q, Tq) id rows -> (Q, Tq) int32"""
        if isinstance(captions, np.ndarray) and captions.ndim == 2:
            return np.ascontiguousarray(captions, dtype=np.int32)
        caps = [captions] if isinstance(captions, str) else list(captions)
        width = max_len or max([1] + [len(words_preprocess(c)) if isinstance(c, str) else np.asarray(c).size for c in caps])
        return encode_captions(caps, self.idx_to_token, max(1, width))

    def localizeCaptions(self, img, captions, nms_thresh=0.3, max_regions=5, min_objectness=None, return_captions=False):
        """Localise query phrases (dc_localize_captions; docs/SEMANTICS.md, "Localising phrases"): for every query a greedy NMS
        ordered by the query's own log-likelihood over ALL proposals of the image, not only the regions the objectness-ordered
        final NMS kept.  captions as in scoreCaptions; nms_thresh in [0, 1]; max_regions in 1..4096 picks per query;
        min_objectness: proposals below it are no candidates (None: all are).  Returns (boxes, scores[, captions]) as forward_test
        gives them and a list with one dict per query, best pick first: {"boxes" (c,4) xcycwh, "loglik" (c,), "objectness" (c,),
        "region" (c,) int32 -- the row of `boxes` that is the same proposal, -1 if the final NMS dropped it}."""
        from .ops import check_localize_args
        opts = check_localize_args(nms_thresh, max_regions, min_objectness)
        q = self._encode_queries(captions)
        self._push_test_args()
        img = self._check_input(img)
        P = self._capacity(img.shape[1], img.shape[2])
        r, boxes, scores, tokens = self._new_result(P)
        if not return_captions:
            r.tokens = None
        Q, Tq = q.shape
        M = opts.max_regions
        cnt = np.zeros((max(Q, 1),), np.int32)
        lb = np.zeros((max(Q, 1), M, 4), np.float32); ll = np.zeros((max(Q, 1), M), np.float32)
        lo = np.zeros((max(Q, 1), M), np.float32); reg = np.full((max(Q, 1), M), -1, np.int32)
        check(self.ctx.h, self.lib.dc_localize_captions(self.ctx.h, img.ctypes.data, img.shape[1], img.shape[2], 0, q.ctypes.data,
                                                        Q, Tq, C.byref(opts), C.byref(r), cnt.ctypes.data, lb.ctypes.data,
                                                        ll.ctypes.data, lo.ctypes.data, reg.ctypes.data),
              "dc_localize_captions")
        K = r.K
        found = [{"boxes": lb[i, :cnt[i]].copy(), "loglik": ll[i, :cnt[i]].copy(), "objectness": lo[i, :cnt[i]].copy(),
                  "region": reg[i, :cnt[i]].copy()} for i in range(Q)]
        res = (boxes[:K].copy(), scores[:K].copy())
        if return_captions:
            res = res + (self.decodeSequence(tokens[:K]),)
        return res + (found,)

    def sampleCaptions(self, img, num_samples, temperature=1.0, seed=0, want_tokens=True, top_k=0, top_p=1.0,
                       want_sample_logprob=False):
        """Sample captions for the image's regions (dc_sample_captions; LM:sample with sample_argmax = false,
        LanguageModel.lua:40-41,328-333): the regions forward_test returns, each with num_samples draws whose words come from
        SoftMax(scores / temperature), and the model's log-probability of every draw.  temperature 0 (num_samples 1) is the
        greedy rule.  Returns (boxes (K,4) xcycwh, scores (K,), tokens (K,T) -- the greedy captions, or None without
        want_tokens --, samples (K,S,T) int32, logprob (K,S)); decodeSequence(samples[:, s]) gives the strings of draw s.
        top_k (0 = off) / top_p (1.0 = off) truncate the distribution of every step (dc_sample_captions_trunc;
        docs/SEMANTICS.md, "Truncation: top-k and nucleus"); want_sample_logprob appends sample_logprob (K,S) -- the
        log-probability of every draw under the distribution it was drawn from -- as a sixth element."""
        from .ops import DeviceArray, check_sample_args, sample_trunc_arg
        opts = check_sample_args(num_samples, temperature, seed, top_k, top_p, want_sample_logprob)
        trunc = sample_trunc_arg(temperature, top_k, top_p, want_sample_logprob, vocab_size=self.vocab_size)
        self._push_test_args()
        on_device = isinstance(img, DeviceArray)       # a (3,H,W) float32 image already on the device (ops.preprocess_u8)
        if on_device:
            if img.dtype != np.float32 or len(img.shape) != 3 or img.shape[0] != 3:
                raise ValueError("sampleCaptions wants a (3,H,W) float32 device image")
            ptr = img.ptr
        else:
            img = self._check_input(img)
            ptr = img.ctypes.data
        P = self._capacity(img.shape[1], img.shape[2])
        r, boxes, scores, tokens = self._new_result(P)
        if not want_tokens:
            r.tokens = None
        S = opts.num_samples
        samples = np.zeros((P, S, self.seq_length), np.int32)
        logprob = np.zeros((P, S), np.float32)
        if trunc is None:
            check(self.ctx.h, self.lib.dc_sample_captions(self.ctx.h, ptr, img.shape[1], img.shape[2], int(on_device),
                                                          C.byref(opts), C.byref(r), samples.ctypes.data, logprob.ctypes.data),
                  "dc_sample_captions")
        else:
            slp = np.zeros((P, S), np.float32) if want_sample_logprob else None
            check(self.ctx.h, self.lib.dc_sample_captions_trunc(self.ctx.h, ptr, img.shape[1], img.shape[2], int(on_device),
                                                                C.byref(opts), C.byref(trunc), C.byref(r), samples.ctypes.data,
                                                                logprob.ctypes.data,
                                                                slp.ctypes.data if slp is not None else None),
                  "dc_sample_captions_trunc")
        K = r.K
        res = (boxes[:K].copy(), scores[:K].copy(), tokens[:K].copy() if want_tokens else None, samples[:K].copy(),
               logprob[:K].copy())
        return res + (slp[:K].copy(),) if want_sample_logprob else res

    def beamCaptions(self, img, beam_size, n_best=None, length_alpha=0.0, want_tokens=True):
        """The n_best best captions of the image's regions by standard beam search (dc_beam_captions; docs/SEMANTICS.md,
        "Standard beam search"): the regions forward_test returns, each with its n_best (None = beam_size) best hypotheses of a
        search of width beam_size -- finished hypotheses set aside, ranked by logprob / len^length_alpha -- and the model's
        unnormalised log-probability of each.  Independent of setBeamSize.  Returns (boxes (K,4) xcycwh, scores (K,), tokens
        (K,T) -- the greedy captions, or None without want_tokens --, captions (K,N,T) int32, logprob (K,N));
        decodeSequence(captions[:, 0]) gives the best strings."""
        from .ops import DeviceArray, check_beam_args
        opts = check_beam_args(beam_size, n_best, length_alpha, vocab_size=self.vocab_size)
        self._push_test_args()
        on_device = isinstance(img, DeviceArray)       # a (3,H,W) float32 image already on the device (ops.preprocess_u8)
        if on_device:
            if img.dtype != np.float32 or len(img.shape) != 3 or img.shape[0] != 3:
                raise ValueError("beamCaptions wants a (3,H,W) float32 device image")
            ptr = img.ptr
        else:
            img = self._check_input(img)
            ptr = img.ctypes.data
        P = self._capacity(img.shape[1], img.shape[2])
        r, boxes, scores, tokens = self._new_result(P)
        if not want_tokens:
            r.tokens = None
        N = opts.n_best
        captions = np.zeros((P, N, self.seq_length), np.int32)
        logprob = np.zeros((P, N), np.float32)
        check(self.ctx.h, self.lib.dc_beam_captions(self.ctx.h, ptr, img.shape[1], img.shape[2], int(on_device), C.byref(opts),
                                                    C.byref(r), captions.ctypes.data, logprob.ctypes.data), "dc_beam_captions")
        K = r.K
        return (boxes[:K].copy(), scores[:K].copy(), tokens[:K].copy() if want_tokens else None, captions[:K].copy(),
                logprob[:K].copy())

    def decodeSequence(self, seq):
        """LanguageModel:decodeSequence (LanguageModel.lua:86-103)."""
        return decode_sequence(seq, self.idx_to_token, self.vocab_size)

    # ---- instrumentation ---------------------------------------------------------------------
    def stage_times(self):
        names = (C.c_char_p * 16)(); ms = (C.c_float * 16)()
        n = self.lib.dc_stage_times(self.ctx.h, names, ms, 16)
        return {names[i].decode(): float(ms[i]) for i in range(max(n, 0))}

    def mfma_profile(self, reset=0):
        l = C.c_int64(0); ms = C.c_double(0); fl = C.c_double(0)
        check(self.ctx.h, self.lib.dc_mfma_profile(self.ctx.h, reset, C.byref(l), C.byref(ms), C.byref(fl)))
        return dict(launches=l.value, ms=ms.value, flops=fl.value)

    def debug_fetch(self, name, shape, dtype=np.float32):
        out = np.empty(shape, dtype)
        n = self.lib.dc_debug_fetch(self.ctx.h, name.encode(), out.ctypes.data, out.nbytes)
        check(self.ctx.h, int(min(n, 0)), "dc_debug_fetch(%s)" % name)
        return out, int(n)
