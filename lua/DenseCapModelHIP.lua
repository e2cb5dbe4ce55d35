--[[
DenseCapModelHIP: drop-in for the TEST-TIME API of nn.DenseCapModel
(densecap/DenseCapModel.lua) backed by libdensecap_hip.so on an AMD MI355X.

Same method names / return values as the reference:
  model:convert(dtype, use_cudnn)            (DenseCapModel.lua:198-208)   no-op, fp32 HIP
  model:setTestArgs{rpn_nms_thresh=, final_nms_thresh=, num_proposals=}   (:185-191)
  model:evaluate()
  boxes, scores, captions = model:forward_test(img)                         (:319-327)
  boxes, feats = model:extractFeatures(img)                                 (:285-304)
and, without a counterpart among the reference's methods:
  boxes, scores, captions, src = model:forward_boxes(img, boxes[, clip])    the test path (:242-275) on the caller's boxes
  model.nets.language_model:decodeSequence(seq)                             (LanguageModel.lua:86-103)

Construction: DenseCapModelHIP.fromCheckpoint(checkpoint.model, gpu) walks the Torch7
module tree of a loaded reference checkpoint (run_model.lua:146-147) and hands the
FloatTensor storages to dc_load_weights.  Written against the header; not executable in
the build container (no LuaJIT / Torch7 there) -- see INTEGRATION.md.
--]]
local ffi = require 'ffi'
local hip = require 'densecap_hip'
local C = hip.C

local Model = {}
Model.__index = Model

-- utils.getopt (densecap/utils.lua:67-75): opt[key], or the default when the key is absent (nil)
local function getopt(opt, key, default_value)
  if default_value == nil and (opt == nil or opt[key] == nil) then
    error('error: required key ' .. key .. ' was not provided in an opt.')
  end
  if opt == nil then return default_value end
  local v = opt[key]
  if v == nil then v = default_value end
  return v
end

local function fptr(t)  -- FloatTensor -> const float*
  assert(t:type() == 'torch.FloatTensor' and t:isContiguous())
  return ffi.cast('const float*', torch.data(t))
end

-- ref: nn.DenseCapModel instance deserialised by torch.load; gpu: 0-based HIP device
function Model.fromCheckpoint(ref, gpu)
  local self = setmetatable({}, Model)
  local pctx = ffi.new('dc_ctx*[1]')
  hip.check(nil, C.dc_create(pctx, gpu or 0), 'dc_create')
  self.ctx = ffi.gc(pctx[0], C.dc_destroy)
  ref:float()
  local w = ffi.new('dc_weights')
  local keep = {}
  local function P(t) t = t:contiguous(); keep[#keep + 1] = t; return fptr(t) end
  -- VGG-16 convs: conv_net1 (layers 1-10) then conv_net2 (11-30), DenseCapModel.lua:61-76
  local convs = {}
  for _, net in ipairs{ref.nets.conv_net1, ref.nets.conv_net2} do
    for i = 1, #net do
      local m = net:get(i)
      if torch.isTypeOf(m, 'nn.SpatialConvolution') then convs[#convs + 1] = m end
    end
  end
  assert(#convs == 13, 'expected the 13 VGG-16 convolutions')
  for i, m in ipairs(convs) do
    w.conv_w[i - 1] = P(m.weight:view(m.nOutputPlane, m.nInputPlane, 3, 3))
    w.conv_b[i - 1] = P(m.bias)
  end
  -- RPN (LocalizationLayer.lua:609-690): rpn = Sequential{conv, ReLU, ConcatTable{box_branch, rpn_branch}, Flatten}
  local rpn = ref.nets.localization_layer.nets.rpn
  local rconv = rpn:get(1)
  local box_conv = rpn:get(3):get(1):get(1)
  local score_conv = rpn:get(3):get(2):get(1)
  w.rpn_conv_w, w.rpn_conv_b = P(rconv.weight), P(rconv.bias)
  w.rpn_box_w, w.rpn_box_b = P(box_conv.weight), P(box_conv.bias)
  w.rpn_score_w, w.rpn_score_b = P(score_conv.weight), P(score_conv.bias)
  local make_anchors = rpn:get(3):get(1):get(3):get(1):get(1)   -- nn.MakeAnchors
  w.anchors = P(make_anchors.anchors)
  w.field_centers[0], w.field_centers[1] = make_anchors.x0, make_anchors.y0
  w.field_centers[2], w.field_centers[3] = make_anchors.sx, make_anchors.sy
  w.num_anchors = make_anchors.anchors:size(2)
  w.rpn_hidden = rconv.nOutputPlane
  -- recog_base = VGG layers 32..38: View, fc6, ReLU, Dropout, fc7, ReLU, Dropout (DenseCapModel.lua:64,90)
  local fcs = {}
  for i = 1, #ref.nets.recog_base do
    local m = ref.nets.recog_base:get(i)
    if torch.isTypeOf(m, 'nn.Linear') then fcs[#fcs + 1] = m end
  end
  w.fc6_w, w.fc6_b, w.fc7_w, w.fc7_b = P(fcs[1].weight), P(fcs[1].bias), P(fcs[2].weight), P(fcs[2].bias)
  w.obj_w, w.obj_b = P(ref.nets.objectness_branch.weight), P(ref.nets.objectness_branch.bias)
  w.boxreg_w, w.boxreg_b = P(ref.nets.box_reg_branch.weight), P(ref.nets.box_reg_branch.bias)
  -- language model (LanguageModel.lua:27-61)
  local lm = ref.nets.language_model
  local enc = lm.image_encoder:get(1)
  w.lm_enc_w, w.lm_enc_b = P(enc.weight), P(enc.bias)
  w.lm_emb = P(lm.lookup_table.weight)
  local lstm, out
  for i = 1, #lm.rnn do
    local m = lm.rnn:get(i)
    if torch.isTypeOf(m, 'nn.LSTM') then lstm = m end
    if torch.isTypeOf(m, 'nn.Linear') then out = m end
  end
  w.lstm_w, w.lstm_b = P(lstm.weight), P(lstm.bias)
  w.lm_out_w, w.lm_out_b = P(out.weight), P(out.bias)
  w.vocab_size, w.seq_length = lm.vocab_size, lm.seq_length
  w.enc_size, w.rnn_size, w.fc_dim = lm.input_encoding_size, lm.rnn_size, fcs[2].weight:size(1)
  hip.check(self.ctx, C.dc_load_weights(self.ctx, w), 'dc_load_weights')
  keep = nil
  -- Test-time state: what the deserialised objects carry (LocalizationLayer.lua:155,233-238 writes the three layer
  -- fields, DenseCapModel.lua:31 opt.final_nms_thresh; train.lua:139-143 sets all four before torch.save) is what the
  -- model runs with until somebody calls setTestArgs.  forward reads these fields at call time, as the reference does.
  local rll = ref.nets.localization_layer
  local ll = {}
  function ll.setTestArgs(layer, args)                     -- LocalizationLayer:setTestArgs, as written: all three re-derived
    layer.test_clip_boxes = getopt(args, 'clip_boxes', true)
    layer.test_nms_thresh = getopt(args, 'nms_thresh', 0.7)
    layer.test_max_proposals = getopt(args, 'max_proposals', 300)
  end
  ll:setTestArgs()
  if rll.test_clip_boxes ~= nil then ll.test_clip_boxes = rll.test_clip_boxes end
  if rll.test_nms_thresh ~= nil then ll.test_nms_thresh = rll.test_nms_thresh end
  if rll.test_max_proposals ~= nil then ll.test_max_proposals = rll.test_max_proposals end
  self.opt = {final_nms_thresh = getopt(ref.opt, 'final_nms_thresh', 0.3)}
  self.vocab_size, self.seq_length, self.fc_dim = lm.vocab_size, lm.seq_length, fcs[2].weight:size(1)
  self.enc_size, self.rnn_size = lm.input_encoding_size, lm.rnn_size
  self.num_anchors = make_anchors.anchors:size(2)
  self.rpn_hidden = rconv.nOutputPlane
  self.idx_to_token = lm.idx_to_token
  -- keep the reference's field layout for callers that reach into it
  -- `model.nets.language_model.beam_size = n` (LanguageModel.lua:129-131) keeps working: the assignment reaches the library
  local lm_state = {}           -- beam_size lives here so that EVERY assignment goes through __newindex
  local lm_proxy = setmetatable({decodeSequence = function(_, seq) return self:decodeSequence(seq) end}, {
    __index = lm_state,
    __newindex = function(t, k, v)
      if k == 'beam_size' then
        self:setBeamSize(v)
        lm_state.beam_size = v
      else
        rawset(t, k, v)
      end
    end})
  self.nets = {language_model = lm_proxy, localization_layer = ll}
  self:_push_test_args()
  return self
end

-- DenseCapModel:setTestArgs (DenseCapModel.lua:185-191), as written: EVERY call re-derives all three values (absent keys
-- -> 0.7 / 1000 / 0.3), unknown keys are ignored (evaluate_model.lua:39-43 passes `max_proposals=`: that caller runs
-- with 1000 proposals), and -- the layer's setTestArgs being called without `clip_boxes` -- box clipping is back on.
function Model:setTestArgs(kwargs)
  local ll = self.nets.localization_layer
  -- a value the library refuses must not stay behind in the object (every later forward would fail in _push_test_args):
  -- the previous state comes back before the error travels on
  local saved = {ll.test_clip_boxes, ll.test_nms_thresh, ll.test_max_proposals, self.opt.final_nms_thresh}
  local ok, err = pcall(function()
    self.nets.localization_layer:setTestArgs{
      nms_thresh = getopt(kwargs, 'rpn_nms_thresh', 0.7),
      max_proposals = getopt(kwargs, 'num_proposals', 1000)
    }
    self.opt.final_nms_thresh = getopt(kwargs, 'final_nms_thresh', 0.3)
    self:_push_test_args()
  end)
  if not ok then
    ll.test_clip_boxes, ll.test_nms_thresh, ll.test_max_proposals, self.opt.final_nms_thresh = unpack(saved)
    error(err, 0)
  end
end
-- the current values travel to the library before every forward (LocalizationLayer.lua:250-256 and DenseCapModel.lua:261
-- read the fields at call time; train.lua:139-143 writes them directly)
function Model:_push_test_args()
  local ll = self.nets.localization_layer
  hip.check(self.ctx, C.dc_set_test_args(self.ctx, ll.test_nms_thresh, self.opt.final_nms_thresh,
                                         ll.test_max_proposals), 'dc_set_test_args')
  if not ll.test_clip_boxes then
    hip.check(self.ctx, C.dc_set_localization_test_args(self.ctx, 0, ll.test_nms_thresh, ll.test_max_proposals),
              'dc_set_localization_test_args')
  end
end
-- rows the result buffers need: num_proposals, or every anchor of the image when it is -1 (uncapped RPN NMS,
-- LocalizationLayer.lua:322-324): k * ceil(H/16) * ceil(W/16) after the four ceil-mode pools
function Model:_capacity(H, W)
  local P = self.nets.localization_layer.test_max_proposals
  if P ~= -1 then return P end
  for _ = 1, 4 do H, W = math.floor((H + 1) / 2), math.floor((W + 1) / 2) end
  return self.num_anchors * H * W
end
-- language_model.beam_size: nil / 0 = greedy LM:sample, n = LM:beamsearch with n beams (1..32)
function Model:setBeamSize(n)
  hip.check(self.ctx, C.dc_set_beam_size(self.ctx, n or 0), 'dc_set_beam_size')
end
-- repeated forwards of one image size relaunched as a captured hipGraph (same results; the webcam daemon's regime)
function Model:setGraphReplay(on)
  hip.check(self.ctx, C.dc_set_graph_replay(self.ctx, on and 1 or 0), 'dc_set_graph_replay')
  return self
end
-- caption order (include/densecap.h: dc_set_caption_order): false = the reference's (LM:sample on all num_proposals rows, then
-- the final NMS, DenseCapModel.lua:127-162,261-275), true = the final NMS first and ONE packed decode of the rows it keeps --
-- the same boxes, scores and tokens bit for bit, about a quarter of the decode work at 1000 proposals
function Model:setCaptionOrder(after_final_nms)
  hip.check(self.ctx, C.dc_set_caption_order(self.ctx, after_final_nms and 1 or 0), 'dc_set_caption_order')
  return self
end
-- arithmetic of the large contractions: 0 = fp32 MFMA (default, the reference's arithmetic), 1 = split-bf16 (opt-in; include/densecap.h)
function Model:setMathMode(mode)
  hip.check(self.ctx, C.dc_set_math_mode(self.ctx, mode or 0), 'dc_set_math_mode')
  return self
end
-- run_model.lua:67-74 on the device: `img` = ByteTensor (H0, W0, 3) RGB as a decoder delivers it -> device pointer of the
-- (3, H, W) float tensor forward_test_device takes, plus H, W.  (image.load + image.scale + BGR, x255, mean; bit-equal to the
-- library's own C loops.)  The caller frees the pointer with C.dc_free(self.ctx, ptr).
function Model:preprocess(img_hwc_bytes, image_size)
  assert(torch.type(img_hwc_bytes) == 'torch.ByteTensor' and img_hwc_bytes:dim() == 3 and img_hwc_bytes:size(3) == 3,
         'preprocess: expected a ByteTensor of shape (H, W, 3)')
  local H0, W0 = img_hwc_bytes:size(1), img_hwc_bytes:size(2)
  local ph, pw = ffi.new('int[1]'), ffi.new('int[1]')
  assert(C.dc_preprocess_size(H0, W0, image_size, ph, pw) == 0, 'image.scale leaves no pixels')
  -- the contiguous copy stays referenced by a local until the call has returned (a temporary could be collected between
  -- the evaluation of the arguments and the C call: ffi.cast allocates)
  local bytes = img_hwc_bytes:contiguous()
  local pp = ffi.new('void*[1]')
  hip.check(self.ctx, C.dc_malloc(self.ctx, pp, 3 * ph[0] * pw[0] * 4), 'dc_malloc')
  local rc = C.dc_preprocess_u8(self.ctx, bytes:data(), H0, W0, 0, image_size, ffi.cast('float*', pp[0]), nil)
  if rc ~= 0 then
    C.dc_free(self.ctx, pp[0])                        -- hip.check raises: give the buffer back first
    hip.check(self.ctx, rc, 'dc_preprocess_u8')
  end
  bytes = nil
  return pp[0], ph[0], pw[0]
end
function Model:convert(dtype, use_cudnn) return self end
function Model:evaluate() return self end
function Model:type() return self end

function Model:decodeSequence(seq)   -- LanguageModel.lua:86-103
  local captions = {}
  local N, T = seq:size(1), seq:size(2)
  for i = 1, N do
    local caption = ''
    for t = 1, T do
      local idx = seq[{i, t}]
      if idx == self.vocab_size + 1 or idx == 0 then break end
      if t > 1 then caption = caption .. ' ' end
      caption = caption .. self.idx_to_token[idx]
    end
    table.insert(captions, caption)
  end
  return captions
end

function Model:forward_test(input)
  self:_push_test_args()
  assert(input:dim() == 4 and input:size(1) == 1 and input:size(2) == 3)  -- DenseCapModel.lua:244
  local img = input:float():contiguous()
  local H, W, T = img:size(3), img:size(4), self.seq_length
  local P = self:_capacity(H, W)
  local boxes, scores = torch.FloatTensor(P, 4), torch.FloatTensor(P, 1)
  local tokens = torch.IntTensor(P, T)
  local r = ffi.new('dc_result')
  r.capacity = P
  r.boxes, r.scores = torch.data(boxes), torch.data(scores)
  r.tokens = torch.data(tokens)
  hip.check(self.ctx, C.dc_forward_test(self.ctx, fptr(img), H, W, 0, r), 'dc_forward_test')
  local K = r.K
  if K == 0 then return torch.FloatTensor(), torch.FloatTensor(), {} end
  local seq = tokens[{{1, K}}]:long()
  return boxes[{{1, K}}]:clone(), scores[{{1, K}}]:clone(), self:decodeSequence(seq)
end

-- The validation losses of one image: what DenseCapModel:forward_backward returns (DenseCapModel.lua:401-474) and
-- eval_utils.eval_split averages, from the forward half alone (docs/SEMANTICS.md, "Validation losses").  model.drop_prob (a number in
-- [0, 1); nil or 0: none) is the Dropout after fc6 and fc7 in this and the other training calls ("Dropout"), masks by loss_seed.
-- data.image (1, 3, H, W), data.gt_boxes (1, G, 4) or (G, 4) xcycwh in the frame of the image, data.gt_labels (1, G, L) or (G, L) word
-- ids padded with zeros.  opts (optional): sampler_batch_size, sampler_high_thresh, sampler_low_thresh,
-- train_remove_outbounds_boxes, the five *_weight keys of train_opts.lua and loss_seed; absent keys take train_opts' defaults.
-- Returns the same table keys as forward_backward.
function Model:forward_losses(data, opts)
  opts = opts or {}
  local input = data.image
  assert(input:dim() == 4 and input:size(1) == 1 and input:size(2) == 3)
  local img = input:float():contiguous()
  local gb, gl = data.gt_boxes, data.gt_labels
  if gb:dim() == 3 then gb = gb[1] end
  if gl:dim() == 3 then gl = gl[1] end
  gb, gl = gb:float():contiguous(), gl:int():contiguous()
  assert(gb:dim() == 2 and gb:size(2) == 4 and gl:dim() == 2 and gl:size(1) == gb:size(1), 'gt_boxes (G,4), gt_labels (G,L)')
  local function get(k, d) if opts[k] == nil then return d end return opts[k] end
  local o = ffi.new('dc_loss_opts')
  o.batch_size = get('sampler_batch_size', 256)
  o.high_thresh, o.low_thresh = get('sampler_high_thresh', 0.7), get('sampler_low_thresh', 0.3)
  o.remove_outbounds = get('train_remove_outbounds_boxes', 1)
  o.mid_box_reg_weight, o.mid_objectness_weight = get('mid_box_reg_weight', 0.05), get('mid_objectness_weight', 0.1)
  o.end_box_reg_weight, o.end_objectness_weight = get('end_box_reg_weight', 0.1), get('end_objectness_weight', 0.1)
  o.captioning_weight = get('captioning_weight', 1.0)
  o.seed = get('loss_seed', 0)
  hip.check(self.ctx, C.dc_set_dropout(self.ctx, self.drop_prob or 0), 'dc_set_dropout')   -- models.lua's drop_prob; nil: none
  local out = ffi.new('dc_losses')
  hip.check(self.ctx, C.dc_forward_losses(self.ctx, fptr(img), img:size(3), img:size(4), 0, torch.data(gb), torch.data(gl),
                                          gb:size(1), gl:size(2), o, nil, out, nil), 'dc_forward_losses')
  return {
    mid_objectness_loss = out.mid_objectness_loss, mid_box_reg_loss = out.mid_box_reg_loss,
    end_objectness_loss = out.end_objectness_loss, end_box_reg_loss = out.end_box_reg_loss,
    captioning_loss = out.captioning_loss, total_loss = out.total_loss,
  }
end

-- forward_losses' losses and the gradient of end_objectness + end_box_reg + captioning with respect to every parameter downstream
-- of the RPN (dc_loss_gradients; docs/SEMANTICS.md, "Recognition-net gradients").  data and opts as forward_losses.  Returns
-- forward_backward's loss keys, num_pos and num_neg, and `grads`: FloatTensors in the checkpoint's layouts for fc6_w, fc6_b, fc7_w,
-- fc7_b, obj_w, obj_b, boxreg_w, boxreg_b and the seven language-model tensors, feat (512, h, w) -- RoI pooling's share of
-- grad_cnn_features --, roi_boxes (num_pos + num_neg, 4) and codes (num_pos, fc_dim).  The CNN backward is not
-- run here (dc_op_cnn_grad is a call of its own).
function Model:loss_gradients(data, opts)
  opts = opts or {}
  local input = data.image
  assert(input:dim() == 4 and input:size(1) == 1 and input:size(2) == 3)
  local img = input:float():contiguous()
  local gb, gl = data.gt_boxes, data.gt_labels
  if gb:dim() == 3 then gb = gb[1] end
  if gl:dim() == 3 then gl = gl[1] end
  gb, gl = gb:float():contiguous(), gl:int():contiguous()
  assert(gb:dim() == 2 and gb:size(2) == 4 and gl:dim() == 2 and gl:size(1) == gb:size(1), 'gt_boxes (G,4), gt_labels (G,L)')
  local function get(k, d) if opts[k] == nil then return d end return opts[k] end
  local o = ffi.new('dc_loss_opts')
  o.batch_size = get('sampler_batch_size', 256)
  o.high_thresh, o.low_thresh = get('sampler_high_thresh', 0.7), get('sampler_low_thresh', 0.3)
  o.remove_outbounds = get('train_remove_outbounds_boxes', 1)
  o.mid_box_reg_weight, o.mid_objectness_weight = get('mid_box_reg_weight', 0.05), get('mid_objectness_weight', 0.1)
  o.end_box_reg_weight, o.end_objectness_weight = get('end_box_reg_weight', 0.1), get('end_objectness_weight', 0.1)
  o.captioning_weight = get('captioning_weight', 1.0)
  o.seed = get('loss_seed', 0)
  hip.check(self.ctx, C.dc_set_dropout(self.ctx, self.drop_prob or 0), 'dc_set_dropout')   -- models.lua's drop_prob; nil: none
  local hw = ffi.new('int[2]')
  hip.check(self.ctx, C.dc_feature_size(img:size(3), img:size(4), hw, hw + 1), 'dc_feature_size')
  local h, w, cap = hw[0], hw[1], o.batch_size
  local E, Hd, D, V = self.enc_size, self.rnn_size, self.fc_dim, self.vocab_size
  local rnames = {'fc6_w', 'fc6_b', 'fc7_w', 'fc7_b', 'obj_w', 'obj_b', 'boxreg_w', 'boxreg_b', 'feat', 'roi_boxes'}
  local lnames = {'lm_enc_w', 'lm_enc_b', 'lm_emb', 'lstm_w', 'lstm_b', 'lm_out_w', 'lm_out_b', 'codes'}
  local shapes = {fc6_w = {D, 512 * 49}, fc6_b = {D}, fc7_w = {D, D}, fc7_b = {D}, obj_w = {1, D}, obj_b = {1}, boxreg_w = {4, D},
                  boxreg_b = {4}, feat = {h, w, 512}, roi_boxes = {cap, 4},
                  lm_enc_w = {E, D}, lm_enc_b = {E}, lm_emb = {V + 2, E}, lstm_w = {E + Hd, 4 * Hd}, lstm_b = {4 * Hd},
                  lm_out_w = {V + 1, Hd}, lm_out_b = {V + 1}, codes = {cap, D}}
  local rg, lg, grads, dev = ffi.new('dc_recog_grads'), ffi.new('dc_lm_grads'), {}, {}
  local function release() for _, p in ipairs(dev) do C.dc_free(self.ctx, p) end end
  local function alloc(bytes)
    local pp = ffi.new('void*[1]')
    local rc = C.dc_malloc(self.ctx, pp, bytes)
    if rc ~= 0 then release(); hip.check(self.ctx, rc, 'dc_malloc') end
    dev[#dev + 1] = pp[0]
    return pp[0]
  end
  for _, k in ipairs(rnames) do
    grads[k] = torch.FloatTensor(unpack(shapes[k]))
    rg[k] = ffi.cast('float*', alloc(grads[k]:nElement() * 4))
  end
  for _, k in ipairs(lnames) do
    grads[k] = torch.FloatTensor(unpack(shapes[k]))
    lg[k] = ffi.cast('float*', alloc(grads[k]:nElement() * 4))
  end
  local out = ffi.new('dc_losses')
  local rc = C.dc_loss_gradients(self.ctx, fptr(img), img:size(3), img:size(4), 0, torch.data(gb), torch.data(gl), gb:size(1),
                                 gl:size(2), o, nil, out, nil, rg, lg)
  for _, k in ipairs(rnames) do
    if rc == 0 then rc = C.dc_memcpy_d2h(self.ctx, torch.data(grads[k]), rg[k], grads[k]:nElement() * 4) end
  end
  for _, k in ipairs(lnames) do
    if rc == 0 then rc = C.dc_memcpy_d2h(self.ctx, torch.data(grads[k]), lg[k], grads[k]:nElement() * 4) end
  end
  release()
  hip.check(self.ctx, rc, 'dc_loss_gradients')
  local n = out.num_pos + out.num_neg
  grads.feat = grads.feat:permute(3, 1, 2):contiguous()                       -- (512, h, w), the reference's layout
  grads.roi_boxes = n > 0 and grads.roi_boxes[{{1, n}}]:clone() or torch.FloatTensor()
  grads.codes = out.num_pos > 0 and grads.codes[{{1, out.num_pos}}]:clone() or torch.FloatTensor()
  return {
    mid_objectness_loss = out.mid_objectness_loss, mid_box_reg_loss = out.mid_box_reg_loss,
    end_objectness_loss = out.end_objectness_loss, end_box_reg_loss = out.end_box_reg_loss,
    captioning_loss = out.captioning_loss, total_loss = out.total_loss,
    num_pos = out.num_pos, num_neg = out.num_neg, grads = grads,
  }
end

-- DenseCapModel:forward_backward (DenseCapModel.lua:401-474) with the reference's default -finetune_cnn_after -1
-- (dc_forward_backward; docs/SEMANTICS.md, "RPN gradients").  data and opts as forward_losses, plus opts.box_reg_decay
-- (train_opts.lua:42: 5e-5).  Returns the reference's loss keys, num_pos and num_neg, and `grads`: loss_gradients' tensors plus
-- rpn_conv_w, rpn_conv_b, rpn_box_w, rpn_box_b, rpn_score_w, rpn_score_b in the checkpoint's layouts -- all 21 tensors outside the
-- CNN --, feat (512, h, w), now the complete grad_cnn_features, and feat_roi, RoI pooling's share of it.  With model.finetune_cnn
-- set (DenseCapModel.lua:338-376) the call is dc_forward_backward_cnn and grads also holds conv_w4 .. conv_w12 (Cout, Cin, 3, 3)
-- and conv_b4 .. conv_b12, the gradients of conv3_1 .. conv5_3.  The loaded weights do not change (train_step updates them).
function Model:forward_backward(data, opts)
  opts = opts or {}
  local input = data.image
  assert(input:dim() == 4 and input:size(1) == 1 and input:size(2) == 3)
  local img = input:float():contiguous()
  local gb, gl = data.gt_boxes, data.gt_labels
  if gb:dim() == 3 then gb = gb[1] end
  if gl:dim() == 3 then gl = gl[1] end
  gb, gl = gb:float():contiguous(), gl:int():contiguous()
  assert(gb:dim() == 2 and gb:size(2) == 4 and gl:dim() == 2 and gl:size(1) == gb:size(1), 'gt_boxes (G,4), gt_labels (G,L)')
  local function get(k, d) if opts[k] == nil then return d end return opts[k] end
  local o = ffi.new('dc_loss_opts')
  o.batch_size = get('sampler_batch_size', 256)
  o.high_thresh, o.low_thresh = get('sampler_high_thresh', 0.7), get('sampler_low_thresh', 0.3)
  o.remove_outbounds = get('train_remove_outbounds_boxes', 1)
  o.mid_box_reg_weight, o.mid_objectness_weight = get('mid_box_reg_weight', 0.05), get('mid_objectness_weight', 0.1)
  o.end_box_reg_weight, o.end_objectness_weight = get('end_box_reg_weight', 0.1), get('end_objectness_weight', 0.1)
  o.captioning_weight = get('captioning_weight', 1.0)
  o.seed = get('loss_seed', 0)
  hip.check(self.ctx, C.dc_set_dropout(self.ctx, self.drop_prob or 0), 'dc_set_dropout')   -- models.lua's drop_prob; nil: none
  local decay = get('box_reg_decay', 5e-5)
  local hw = ffi.new('int[2]')
  hip.check(self.ctx, C.dc_feature_size(img:size(3), img:size(4), hw, hw + 1), 'dc_feature_size')
  local h, w, cap = hw[0], hw[1], o.batch_size
  local E, Hd, D, V = self.enc_size, self.rnn_size, self.fc_dim, self.vocab_size
  local k, R = self.num_anchors, self.rpn_hidden
  local rnames = {'fc6_w', 'fc6_b', 'fc7_w', 'fc7_b', 'obj_w', 'obj_b', 'boxreg_w', 'boxreg_b', 'feat', 'roi_boxes'}
  local lnames = {'lm_enc_w', 'lm_enc_b', 'lm_emb', 'lstm_w', 'lstm_b', 'lm_out_w', 'lm_out_b', 'codes'}
  local pnames = {'rpn_conv_w', 'rpn_conv_b', 'rpn_box_w', 'rpn_box_b', 'rpn_score_w', 'rpn_score_b', 'feat'}
  local shapes = {fc6_w = {D, 512 * 49}, fc6_b = {D}, fc7_w = {D, D}, fc7_b = {D}, obj_w = {1, D}, obj_b = {1}, boxreg_w = {4, D},
                  boxreg_b = {4}, feat = {h, w, 512}, roi_boxes = {cap, 4},
                  lm_enc_w = {E, D}, lm_enc_b = {E}, lm_emb = {V + 2, E}, lstm_w = {E + Hd, 4 * Hd}, lstm_b = {4 * Hd},
                  lm_out_w = {V + 1, Hd}, lm_out_b = {V + 1}, codes = {cap, D},
                  rpn_conv_w = {R, 512, 3, 3}, rpn_conv_b = {R}, rpn_box_w = {4 * k, R, 1, 1}, rpn_box_b = {4 * k},
                  rpn_score_w = {2 * k, R, 1, 1}, rpn_score_b = {2 * k}}
  local rg, lg, pg = ffi.new('dc_recog_grads'), ffi.new('dc_lm_grads'), ffi.new('dc_rpn_grads')
  local grads, dev = {}, {}
  local function release() for _, p in ipairs(dev) do C.dc_free(self.ctx, p) end end
  local function alloc(bytes)
    local pp = ffi.new('void*[1]')
    local rc = C.dc_malloc(self.ctx, pp, bytes)
    if rc ~= 0 then release(); hip.check(self.ctx, rc, 'dc_malloc') end
    dev[#dev + 1] = pp[0]
    return pp[0]
  end
  local host = {}                                   -- {struct, field, tensor}: what comes back
  local function bind(struct, names, rename)
    for _, name in ipairs(names) do
      local t = torch.FloatTensor(unpack(shapes[name]))
      struct[name] = ffi.cast('float*', alloc(t:nElement() * 4))
      local key = rename and rename[name] or name
      grads[key] = t
      host[#host + 1] = {struct, name, t}
    end
  end
  bind(rg, rnames, {feat = 'feat_roi'})
  bind(lg, lnames)
  bind(pg, pnames)
  local cg = nil
  if self.finetune_cnn then                           -- conv3_1 .. conv5_3: entry j of dc_cnn_grads is convolution 4 + j
    local chans = {{128, 256}, {256, 256}, {256, 256}, {256, 512}, {512, 512}, {512, 512}, {512, 512}, {512, 512}, {512, 512}}
    cg = ffi.new('dc_cnn_grads')
    for j, c in ipairs(chans) do
      local tw, tb = torch.FloatTensor(c[2], c[1], 3, 3), torch.FloatTensor(c[2])
      cg.conv_w[j - 1] = ffi.cast('float*', alloc(tw:nElement() * 4))
      cg.conv_b[j - 1] = ffi.cast('float*', alloc(tb:nElement() * 4))
      grads['conv_w' .. (j + 3)], grads['conv_b' .. (j + 3)] = tw, tb
      host[#host + 1] = {cg.conv_w, j - 1, tw}
      host[#host + 1] = {cg.conv_b, j - 1, tb}
    end
  end
  local out = ffi.new('dc_losses')
  local rc
  if cg then
    rc = C.dc_forward_backward_cnn(self.ctx, fptr(img), img:size(3), img:size(4), 0, torch.data(gb), torch.data(gl), gb:size(1),
                                   gl:size(2), o, nil, out, nil, rg, lg, decay, pg, cg)
  else
    rc = C.dc_forward_backward(self.ctx, fptr(img), img:size(3), img:size(4), 0, torch.data(gb), torch.data(gl), gb:size(1),
                               gl:size(2), o, nil, out, nil, rg, lg, decay, pg)
  end
  for _, e in ipairs(host) do
    if rc == 0 then rc = C.dc_memcpy_d2h(self.ctx, torch.data(e[3]), e[1][e[2]], e[3]:nElement() * 4) end
  end
  release()
  hip.check(self.ctx, rc, 'dc_forward_backward')
  local n = out.num_pos + out.num_neg
  grads.feat = grads.feat:permute(3, 1, 2):contiguous()                       -- (512, h, w), the reference's layout
  grads.feat_roi = grads.feat_roi:permute(3, 1, 2):contiguous()
  grads.roi_boxes = n > 0 and grads.roi_boxes[{{1, n}}]:clone() or torch.FloatTensor()
  grads.codes = out.num_pos > 0 and grads.codes[{{1, out.num_pos}}]:clone() or torch.FloatTensor()
  return {
    mid_objectness_loss = out.mid_objectness_loss, mid_box_reg_loss = out.mid_box_reg_loss,
    end_objectness_loss = out.end_objectness_loss, end_box_reg_loss = out.end_box_reg_loss,
    captioning_loss = out.captioning_loss, total_loss = out.total_loss,
    num_pos = out.num_pos, num_neg = out.num_neg, grads = grads,
  }
end

-- The training step (docs/SEMANTICS.md, "Training step"): train.lua's loop body for the default -finetune_cnn_after -1 on the
-- device.  train_begin(opts): opts.learning_rate, optim_beta1, optim_beta2, optim_epsilon, weight_decay (train_opts.lua's names
-- and defaults: 1e-5, 0.9, 0.999, 1e-8, 1e-6); Adam's moments start at zero, the step count at 0.
function Model:train_begin(opts)
  opts = opts or {}
  local function get(k, d) if opts[k] == nil then return d end return opts[k] end
  local o = ffi.new('dc_train_opts')
  o.learning_rate = get('learning_rate', 1e-5)
  o.beta1, o.beta2 = get('optim_beta1', 0.9), get('optim_beta2', 0.999)
  o.epsilon = get('optim_epsilon', 1e-8)
  o.weight_decay = get('weight_decay', 1e-6)
  hip.check(self.ctx, C.dc_train_begin(self.ctx, o), 'dc_train_begin')
end

-- One iteration (dc_train_step): forward_backward on `data` (data and opts as forward_losses, plus opts.box_reg_decay), then
-- grad_params:add(weight_decay, params) and adam(params, grad_params, ...) on the 21 tensors outside the CNN, in place on the
-- device, and the refresh of everything the library derives from them.  Returns forward_backward's loss keys, num_pos and
-- num_neg, for the weights as they were before the step; no gradient leaves the device.  Dropout is model.drop_prob's.  The CNN:
-- opts.cnn_mode (dc_train_set_cnn: 0, 1, 2), by default 2 where model.finetune_cnn is set (train.lua:83-85) and 0 where not;
-- train.lua's step at iter == finetune_cnn_after, decay and Adam on a zero gradient, is cnn_mode = 1.  With model.grad_clip > 0
-- the gradient is clipped by its global norm and the result carries grad_norm and grad_scale.
function Model:train_step(data, opts)
  opts = opts or {}
  local input = data.image
  assert(input:dim() == 4 and input:size(1) == 1 and input:size(2) == 3)
  local img = input:float():contiguous()
  local gb, gl = data.gt_boxes, data.gt_labels
  if gb:dim() == 3 then gb = gb[1] end
  if gl:dim() == 3 then gl = gl[1] end
  gb, gl = gb:float():contiguous(), gl:int():contiguous()
  assert(gb:dim() == 2 and gb:size(2) == 4 and gl:dim() == 2 and gl:size(1) == gb:size(1), 'gt_boxes (G,4), gt_labels (G,L)')
  local function get(k, d) if opts[k] == nil then return d end return opts[k] end
  local o = ffi.new('dc_loss_opts')
  o.batch_size = get('sampler_batch_size', 256)
  o.high_thresh, o.low_thresh = get('sampler_high_thresh', 0.7), get('sampler_low_thresh', 0.3)
  o.remove_outbounds = get('train_remove_outbounds_boxes', 1)
  o.mid_box_reg_weight, o.mid_objectness_weight = get('mid_box_reg_weight', 0.05), get('mid_objectness_weight', 0.1)
  o.end_box_reg_weight, o.end_objectness_weight = get('end_box_reg_weight', 0.1), get('end_objectness_weight', 0.1)
  o.captioning_weight = get('captioning_weight', 1.0)
  o.seed = get('loss_seed', 0)
  hip.check(self.ctx, C.dc_set_dropout(self.ctx, self.drop_prob or 0), 'dc_set_dropout')   -- models.lua's drop_prob; nil: none
  hip.check(self.ctx, C.dc_train_set_cnn(self.ctx, get('cnn_mode', self.finetune_cnn and 2 or 0)), 'dc_train_set_cnn')
  -- gradient clipping (docs/SEMANTICS.md, "Gradient clipping"): model.grad_clip = max_norm of the global L2 norm; nil or 0: off
  local clip = self.grad_clip or 0
  hip.check(self.ctx, C.dc_train_set_grad_clip(self.ctx, clip), 'dc_train_set_grad_clip')
  local out = ffi.new('dc_losses')
  hip.check(self.ctx, C.dc_train_step(self.ctx, fptr(img), img:size(3), img:size(4), 0, torch.data(gb), torch.data(gl),
                                      gb:size(1), gl:size(2), o, nil, out, nil, get('box_reg_decay', 5e-5)), 'dc_train_step')
  local res = {
    mid_objectness_loss = out.mid_objectness_loss, mid_box_reg_loss = out.mid_box_reg_loss,
    end_objectness_loss = out.end_objectness_loss, end_box_reg_loss = out.end_box_reg_loss,
    captioning_loss = out.captioning_loss, total_loss = out.total_loss,
    num_pos = out.num_pos, num_neg = out.num_neg,
  }
  if clip > 0 then
    local norm, scale = ffi.new('double[1]'), ffi.new('float[1]')
    hip.check(self.ctx, C.dc_train_grad_norm(self.ctx, norm, scale), 'dc_train_grad_norm')
    res.grad_norm, res.grad_scale = norm[0], scale[0]
  end
  return res
end

-- dc_train_end: frees the moments and the gradient arenas (the CNN's too); the weights stay as trained.
function Model:train_end()
  hip.check(self.ctx, C.dc_train_end(self.ctx), 'dc_train_end')
end

-- Language-model gradients (dc_op_lm_grad; docs/SEMANTICS.md, "Language-model gradients"): codes FloatTensor (n, fc_dim), labels
-- IntTensor (n, L) word ids padded with zeros, weight (default 1).  Returns a table with the gradients of the seven
-- language-model tensors in the checkpoint's layouts and of the codes (FloatTensors), loss and rowlik (DoubleTensor (n)).
function Model:lm_gradients(codes, labels, weight)
  local x, lab = codes:float():contiguous(), labels:int():contiguous()
  assert(x:dim() == 2 and x:size(2) == self.fc_dim and lab:dim() == 2 and lab:size(1) == x:size(1), 'codes (n,fc_dim), labels (n,L)')
  local n, L = lab:size(1), lab:size(2)
  local E, Hd, D, V = self.enc_size, self.rnn_size, self.fc_dim, self.vocab_size
  local names = {'lm_enc_w', 'lm_enc_b', 'lm_emb', 'lstm_w', 'lstm_b', 'lm_out_w', 'lm_out_b', 'codes'}
  local shapes = {lm_enc_w = {E, D}, lm_enc_b = {E}, lm_emb = {V + 2, E}, lstm_w = {E + Hd, 4 * Hd}, lstm_b = {4 * Hd},
                  lm_out_w = {V + 1, Hd}, lm_out_b = {V + 1}, codes = {n, D}}
  local g, out, dev = ffi.new('dc_lm_grads'), {}, {}
  local function release() for _, p in ipairs(dev) do C.dc_free(self.ctx, p) end end
  local function alloc(bytes)
    local pp = ffi.new('void*[1]')
    local rc = C.dc_malloc(self.ctx, pp, bytes)
    if rc ~= 0 then release(); hip.check(self.ctx, rc, 'dc_malloc') end
    dev[#dev + 1] = pp[0]
    return pp[0]
  end
  local xd = alloc(x:nElement() * 4)
  for _, k in ipairs(names) do
    out[k] = torch.FloatTensor(unpack(shapes[k]))
    g[k] = ffi.cast('float*', alloc(out[k]:nElement() * 4))
  end
  local loss, rowlik = ffi.new('double[1]'), torch.DoubleTensor(n)
  local rc = C.dc_memcpy_h2d(self.ctx, xd, torch.data(x), x:nElement() * 4)
  if rc == 0 then
    rc = C.dc_op_lm_grad(self.ctx, ffi.cast('const float*', xd), n, torch.data(lab), L, weight or 1.0, g, loss, torch.data(rowlik))
  end
  for _, k in ipairs(names) do
    if rc == 0 then rc = C.dc_memcpy_d2h(self.ctx, torch.data(out[k]), g[k], out[k]:nElement() * 4) end
  end
  release()
  hip.check(self.ctx, rc, 'dc_op_lm_grad')
  out.loss, out.rowlik = loss[0], rowlik
  return out
end

-- Rank the regions of one image by log p(query | region) (teacher-forced LanguageModel:updateOutput with a gt_sequence,
-- LanguageModel.lua:106-127, targets of getTarget :148-167).  queries: IntTensor (Q, Tq) of 1-based word ids, zero-padded.
-- Returns the boxes, scores and captions forward_test returns, and loglik (K, Q).
function Model:scoreCaptions(input, queries)
  self:_push_test_args()
  assert(input:dim() == 4 and input:size(1) == 1 and input:size(2) == 3)
  local img = input:float():contiguous()
  local q = queries:int():contiguous()
  local H, W, T = img:size(3), img:size(4), self.seq_length
  local Q, Tq = q:size(1), q:size(2)
  local P = self:_capacity(H, W)
  local boxes, scores = torch.FloatTensor(P, 4), torch.FloatTensor(P, 1)
  local tokens = torch.IntTensor(P, T)
  local loglik = torch.FloatTensor(P, Q)
  local r = ffi.new('dc_result')
  r.capacity = P
  r.boxes, r.scores = torch.data(boxes), torch.data(scores)
  r.tokens = torch.data(tokens)
  hip.check(self.ctx, C.dc_score_captions(self.ctx, fptr(img), H, W, 0, torch.data(q), Q, Tq, r, torch.data(loglik)),
            'dc_score_captions')
  local K = r.K
  if K == 0 then return torch.FloatTensor(), torch.FloatTensor(), {}, torch.FloatTensor() end
  local seq = tokens[{{1, K}}]:long()
  return boxes[{{1, K}}]:clone(), scores[{{1, K}}]:clone(), self:decodeSequence(seq), loglik[{{1, K}}]:clone()
end

-- Localise query phrases (dc_localize_captions; docs/SEMANTICS.md, "Localising phrases"): per query a greedy NMS ordered by the
-- query's own log-likelihood over ALL proposals of the image.  queries as in scoreCaptions; nms_thresh (default 0.3) in [0, 1];
-- max_regions (default 5) in 1..4096; min_objectness (nil = every proposal is a candidate).
-- Returns the boxes, scores and captions forward_test returns, and count: IntTensor (Q); lboxes (Q, M, 4) xcycwh; loglik (Q, M);
-- objectness (Q, M); region: LongTensor (Q, M), the 1-based row of `boxes` that is the same proposal, 0 if the final NMS
-- dropped it.  Entries from count[q] on are zero.
function Model:localizeCaptions(input, queries, nms_thresh, max_regions, min_objectness)
  self:_push_test_args()
  assert(input:dim() == 4 and input:size(1) == 1 and input:size(2) == 3)
  local o = ffi.new('dc_localize_opts')
  o.nms_thresh, o.max_regions, o.min_objectness = nms_thresh or 0.3, max_regions or 5, min_objectness or -math.huge
  local M = o.max_regions
  assert(o.nms_thresh >= 0 and o.nms_thresh <= 1, 'nms_thresh must be in [0, 1]')
  assert(M >= 1 and M <= 4096 and M == (max_regions or 5), 'max_regions must be an integer in 1..4096')
  assert(o.min_objectness == o.min_objectness, 'min_objectness must not be NaN')
  local img = input:float():contiguous()
  local q = queries:int():contiguous()
  local H, W, T = img:size(3), img:size(4), self.seq_length
  local Q, Tq = q:size(1), q:size(2)
  local P = self:_capacity(H, W)
  local boxes, scores = torch.FloatTensor(P, 4), torch.FloatTensor(P, 1)
  local tokens = torch.IntTensor(P, T)
  local count, region = torch.IntTensor(Q):zero(), torch.IntTensor(Q, M):fill(-1)
  local lboxes, loglik, obj = torch.FloatTensor(Q, M, 4):zero(), torch.FloatTensor(Q, M):zero(), torch.FloatTensor(Q, M):zero()
  local r = ffi.new('dc_result')
  r.capacity = P
  r.boxes, r.scores = torch.data(boxes), torch.data(scores)
  r.tokens = torch.data(tokens)
  hip.check(self.ctx, C.dc_localize_captions(self.ctx, fptr(img), H, W, 0, torch.data(q), Q, Tq, o, r, torch.data(count),
                                             torch.data(lboxes), torch.data(loglik), torch.data(obj), torch.data(region)),
            'dc_localize_captions')
  local K = r.K
  local reg1 = region:long():add(1)
  if K == 0 then return torch.FloatTensor(), torch.FloatTensor(), {}, count, lboxes, loglik, obj, reg1 end
  local seq = tokens[{{1, K}}]:long()
  return boxes[{{1, K}}]:clone(), scores[{{1, K}}]:clone(), self:decodeSequence(seq), count, lboxes, loglik, obj, reg1
end

-- Sample captions (LanguageModel:sample with sample_argmax = false, LanguageModel.lua:40-41,328-333): num_samples draws for
-- each region forward_test returns, every word drawn from SoftMax(scores / temperature) (temperature default 1; 0 with
-- num_samples 1 is the greedy rule), noise selected by `seed` (default 0, a non-negative integer below 2^53 from Lua).
-- Returns boxes, scores, the greedy captions, samples: IntTensor (K, S, T) of word ids (up to and including the first END,
-- zeros after it; self:decodeSequence(samples[{{}, s}]:long()) gives the strings of draw s) and logprob (K, S), the model's
-- log-probability of every draw.
-- top_k (nil or 0 = off) / top_p (nil or 1 = off): truncation of every step's distribution (dc_sample_captions_trunc;
-- docs/SEMANTICS.md, "Truncation: top-k and nucleus").  With either, a sixth value is returned: sample_logprob (K, S), the
-- log-probability of every draw under the truncated distribution it was drawn from.
function Model:sampleCaptions(input, num_samples, temperature, seed, top_k, top_p)
  self:_push_test_args()
  assert(input:dim() == 4 and input:size(1) == 1 and input:size(2) == 3)
  local img = input:float():contiguous()
  local H, W, T = img:size(3), img:size(4), self.seq_length
  local S = num_samples
  assert(type(S) == 'number' and S >= 1 and S <= 256 and S == math.floor(S), 'num_samples must be an integer in 1..256')
  local P = self:_capacity(H, W)
  local boxes, scores = torch.FloatTensor(P, 4), torch.FloatTensor(P, 1)
  local tokens = torch.IntTensor(P, T)
  local samples, logprob = torch.IntTensor(P, S, T):zero(), torch.FloatTensor(P, S):zero()
  local o = ffi.new('dc_sample_opts')
  o.num_samples, o.temperature, o.seed = S, temperature or 1, seed or 0
  local r = ffi.new('dc_result')
  r.capacity = P
  r.boxes, r.scores = torch.data(boxes), torch.data(scores)
  r.tokens = torch.data(tokens)
  local truncated = (top_k ~= nil and top_k ~= 0) or (top_p ~= nil and top_p ~= 1)
  local slp
  if truncated then
    local tr = ffi.new('dc_sample_trunc')
    tr.top_k, tr.top_p = top_k or 0, top_p or 1
    slp = torch.FloatTensor(P, S):zero()
    hip.check(self.ctx, C.dc_sample_captions_trunc(self.ctx, fptr(img), H, W, 0, o, tr, r, torch.data(samples),
                                                   torch.data(logprob), torch.data(slp)), 'dc_sample_captions_trunc')
  else
    hip.check(self.ctx, C.dc_sample_captions(self.ctx, fptr(img), H, W, 0, o, r, torch.data(samples), torch.data(logprob)),
              'dc_sample_captions')
  end
  local K = r.K
  if K == 0 then
    return torch.FloatTensor(), torch.FloatTensor(), {}, torch.IntTensor(), torch.FloatTensor(),
           truncated and torch.FloatTensor() or nil
  end
  local seq = tokens[{{1, K}}]:long()
  return boxes[{{1, K}}]:clone(), scores[{{1, K}}]:clone(), self:decodeSequence(seq), samples[{{1, K}}]:clone(),
         logprob[{{1, K}}]:clone(), truncated and slp[{{1, K}}]:clone() or nil
end

-- Standard beam search (dc_beam_captions; docs/SEMANTICS.md, "Standard beam search"): for each region forward_test returns, the
-- n_best (nil = beam_size) best hypotheses of a search of width beam_size (1..32) in which finished hypotheses are set aside,
-- ranked by logprob / len^length_alpha (nil or 0 = by log-probability).  Independent of language_model.beam_size.
-- Returns boxes, scores, the greedy captions, captions: IntTensor (K, N, T) of word ids (up to and including END, zeros after
-- it, best first; self:decodeSequence(captions[{{}, 1}]:long()) gives the best strings) and logprob (K, N), the model's
-- unnormalised log-probability of each.
function Model:beamCaptions(input, beam_size, n_best, length_alpha)
  self:_push_test_args()
  assert(input:dim() == 4 and input:size(1) == 1 and input:size(2) == 3)
  local img = input:float():contiguous()
  local H, W, T = img:size(3), img:size(4), self.seq_length
  local B = beam_size
  assert(type(B) == 'number' and B >= 1 and B <= 32 and B == math.floor(B), 'beam_size must be an integer in 1..32')
  local N = n_best or B
  assert(type(N) == 'number' and N >= 1 and N <= B and N == math.floor(N), 'n_best must be an integer in 1..beam_size')
  local P = self:_capacity(H, W)
  local boxes, scores = torch.FloatTensor(P, 4), torch.FloatTensor(P, 1)
  local tokens = torch.IntTensor(P, T)
  local captions, logprob = torch.IntTensor(P, N, T):zero(), torch.FloatTensor(P, N):zero()
  local o = ffi.new('dc_beam_opts')
  o.beam_size, o.n_best, o.length_alpha = B, N, length_alpha or 0
  local r = ffi.new('dc_result')
  r.capacity = P
  r.boxes, r.scores = torch.data(boxes), torch.data(scores)
  r.tokens = torch.data(tokens)
  hip.check(self.ctx, C.dc_beam_captions(self.ctx, fptr(img), H, W, 0, o, r, torch.data(captions), torch.data(logprob)),
            'dc_beam_captions')
  local K = r.K
  if K == 0 then
    return torch.FloatTensor(), torch.FloatTensor(), {}, torch.IntTensor(), torch.FloatTensor()
  end
  local seq = tokens[{{1, K}}]:long()
  return boxes[{{1, K}}]:clone(), scores[{{1, K}}]:clone(), self:decodeSequence(seq), captions[{{1, K}}]:clone(),
         logprob[{{1, K}}]:clone()
end

-- The model after the RPN on the caller's boxes (dc_forward_boxes; DenseCapModel.lua:242-275 with `boxes` in the place of
-- the localisation layer's roi_boxes).  boxes: FloatTensor (n, 4) xc,yc,w,h in the pixel frame of `input` (the frame
-- forward_test returns), 1 <= n <= num_proposals; clip (optional): box_utils.clip_boxes first, invalid boxes dropped.
-- Returns boxes, scores, captions and src: LongTensor (K), the 1-based row of `boxes` behind each result row.
function Model:forward_boxes(input, boxes, clip)
  self:_push_test_args()
  assert(input:dim() == 4 and input:size(1) == 1 and input:size(2) == 3)
  assert(boxes:dim() == 2 and boxes:size(2) == 4, 'boxes must be (n, 4) xc,yc,w,h')
  local img = input:float():contiguous()
  local inb = boxes:float():contiguous()
  local H, W, T = img:size(3), img:size(4), self.seq_length
  local P = self:_capacity(H, W)
  local out_boxes, scores = torch.FloatTensor(P, 4), torch.FloatTensor(P, 1)
  local tokens, src = torch.IntTensor(P, T), torch.IntTensor(P)
  local r = ffi.new('dc_result')
  r.capacity = P
  r.boxes, r.scores = torch.data(out_boxes), torch.data(scores)
  r.tokens = torch.data(tokens)
  local bl = ffi.new('dc_box_list')
  bl.boxes, bl.n, bl.src = torch.data(inb), inb:size(1), torch.data(src)
  hip.check(self.ctx, C.dc_forward_boxes(self.ctx, fptr(img), H, W, 0, bl, clip and 1 or 0, r), 'dc_forward_boxes')
  local K = r.K
  if K == 0 then return torch.FloatTensor(), torch.FloatTensor(), {}, torch.LongTensor() end
  local seq = tokens[{{1, K}}]:long()
  return out_boxes[{{1, K}}]:clone(), scores[{{1, K}}]:clone(), self:decodeSequence(seq), src[{{1, K}}]:long():add(1)
end

function Model:extractFeatures(input)
  self:_push_test_args()
  local img = input:float():contiguous()
  local H, W = img:size(3), img:size(4)
  local P = self:_capacity(H, W)
  local boxes, feats = torch.FloatTensor(P, 4), torch.FloatTensor(P, self.fc_dim)
  local K = ffi.new('int32_t[1]')
  hip.check(self.ctx, C.dc_extract_features(self.ctx, fptr(img), H, W, 0, P, torch.data(boxes),
                                            torch.data(feats), K), 'dc_extract_features')
  return boxes[{{1, K[0]}}]:clone(), feats[{{1, K[0]}}]:clone()
end

-- Multi-GPU (one LuaJIT process per GPU; the reference is single-device, densecap/utils.lua:22-36): every rank runs
-- forward_raw on its shard of the image list, then ONE gather on rank 0 (RCCL point-to-point over xGMI).
--   id = DenseCapModelHIP.commUniqueId()                       -- rank 0; pass the 128-byte string to the others
--   model:commInit(id, rank, world)
--   all = model:gatherResults(results)                         -- results: array of dc_result filled by forward_raw
function Model.commUniqueId()
  local id = ffi.new('uint8_t[128]')
  hip.check(nil, C.dc_comm_unique_id(id), 'dc_comm_unique_id')
  return ffi.string(id, 128)
end
-- self_transport (world == 1 only): build the RCCL carrier for the single rank too, so that gatherResults travels through
-- ncclSend / ncclRecv to itself (DC_COMM_SELF_TRANSPORT) -- the multi-GPU code path on one GPU
function Model:commInit(id, rank, world, self_transport)
  local pc = ffi.new('dc_comm*[1]')
  hip.check(self.ctx, C.dc_comm_create_ex(pc, self.ctx, id, rank, world, self_transport and 1 or 0), 'dc_comm_create')
  self.comm, self.rank, self.world = ffi.gc(pc[0], C.dc_comm_destroy), rank, world
end
-- forward_test without string decoding: returns a dc_result (and the tensors that own its buffers)
function Model:forward_raw(input)
  self:_push_test_args()
  local img = input:float():contiguous()
  local H, W, T = img:size(3), img:size(4), self.seq_length
  local P = self:_capacity(H, W)
  local keep = {torch.FloatTensor(P, 4), torch.FloatTensor(P), torch.IntTensor(P, T)}
  local r = ffi.new('dc_result')
  r.capacity, r.boxes, r.scores, r.tokens = P, torch.data(keep[1]), torch.data(keep[2]), torch.data(keep[3])
  hip.check(self.ctx, C.dc_forward_test(self.ctx, fptr(img), H, W, 0, r), 'dc_forward_test')
  return r, keep
end
function Model:gatherResults(results)   -- results: Lua array of dc_result with one capacity
  local n = #results
  local loc = ffi.new('dc_result[?]', n)
  for i = 1, n do loc[i - 1] = results[i] end
  local all, keep = nil, {}
  if self.rank == 0 then
    all = ffi.new('dc_result[?]', n * self.world)
    local P, T = loc[0].capacity, self.seq_length
    for i = 0, n * self.world - 1 do
      local k = {torch.FloatTensor(P, 4), torch.FloatTensor(P), torch.IntTensor(P, T)}
      keep[#keep + 1] = k
      all[i].capacity, all[i].boxes, all[i].scores, all[i].tokens = P, torch.data(k[1]), torch.data(k[2]), torch.data(k[3])
    end
  end
  local rc = C.dc_gather_results(self.comm, loc, n, all)
  if rc < 0 then error('dc_gather_results: ' .. ffi.string(C.dc_comm_last_error(self.comm))) end
  return all, keep
end

return Model
