"""Network -- the Faster R-CNN graph of the reference (lib/nets/network.py), re-hosted on
libfrcnn_hip.so.  No TensorFlow: `sess` is a frcnn_hip.runtime.Session (device + stream + weights),
`create_architecture` declares the variables (TF/slim names and layouts), and one call of
`test_image` runs image -> backbone -> RPN -> proposals -> RoI crop -> tail -> cls/bbox entirely
on the GPU -- the py_func host hops of network.py:100-126 and the per-image sess.run (:470-479)
are gone; the chain is captured once per image shape into a hipGraph and replayed.

Public surface kept from the reference (file:line = /root/reference/lib/nets/network.py):
  create_architecture (386), test_image (470), extract_head (464), hooks _image_to_head /
  _head_to_tail (380-384), _anchor_component (210), _region_proposal (323), _crop_pool_layer (141),
  _region_classification (361), self._predictions keys (348-353, 373-376).
"""
import collections

import numpy as np
import torch

from frcnn_hip import ACT_NONE, ACT_RELU, NMS_RULE_CPU, NMS_RULE_GPU, forward, ops, replay
from frcnn_hip.runtime import VarSpec
from model.config import cfg


class Network(object):
    def __init__(self):
        self._predictions = {}
        self._losses = {}
        self._anchor_targets = {}
        self._rpn_anchors = None               # cfg.HIP.RPN_BBOX_LOSS other than 'smooth_l1': the [H W A, 4] anchors the last step's loss decoded on
        self._proposal_targets = {}
        self._layers = {}
        self._act_summaries = []
        self._variables_to_fix = {}
        self._feat_stride = [16, ]
        self._scope = "network"
        self._sess = None
        self._image = None
        self._im_info = None
        self._var_specs = collections.OrderedDict()
        self._tape = []
        self._requires_grad = set()
        self._gt_boxes = None
        self._sample_seed = 0
        self._replayer = replay.StepReplayer()             # train_step_async under cfg.HIP.TRAIN_REPLAY
        self.replay_stats = self._replayer.stats       # dict(eager, recorded, replayed)
        self._train_scope_key = None                   # the step's shape scope (_train_scope)
        self._train_state = None               # the solver handle of the last train_step_with_summary (get_summary's regulariser term)
        self._fuse_tail_entry = False          # TEST-only graph restructuring, see resnetv1._fused_tail_entry
        self._plan, self._forms = None, None   # the last graph build's forward.Plan and forward.Forms (_plan_context)
        self._read_only = False                # inside _ohem_scores: launches as in TRAIN mode, nothing goes on the tape
        self._ohem = {}                        # cfg.HIP.OHEM: keep_inds, roi_loss and the read-only pass's cls_score / bbox_pred of the last step

    # ------------------------------------------------------------------ variable declaration
    def _var(self, name, shape, init, arg=None):
        self._var_specs[name] = VarSpec(shape, init, arg)

    def _declare_conv_bn(self, scope, kh, kw, cin, cout, residual_branch_end=False):
        self._var(scope + "/weights", (kh, kw, cin, cout), "he")
        self._var(scope + "/BatchNorm/gamma", (cout,), "bn_gamma_res" if residual_branch_end else "bn_gamma")
        self._var(scope + "/BatchNorm/beta", (cout,), "bn_beta")
        self._var(scope + "/BatchNorm/moving_mean", (cout,), "bn_mean")
        self._var(scope + "/BatchNorm/moving_variance", (cout,), "bn_var")

    def _declare_conv_bias(self, scope, kh, kw, cin, cout, std):
        self._var(scope + "/weights", (kh, kw, cin, cout), "normal", std)
        self._var(scope + "/biases", (cout,), "zeros")

    def _declare_backbone(self):
        raise NotImplementedError

    def _head_channels(self):
        raise NotImplementedError

    def _tail_channels(self):
        raise NotImplementedError

    def variable_specs(self):
        return self._var_specs

    # ------------------------------------------------------------------ building blocks
    def _conv(self, x, scope, k, stride=1, pad=(0, 0, 0, 0), act=ACT_RELU, bn_eps=None, residual=None,
              res_stride=1, fold_w=False, out_affine=None, real_cin=None, no_bias=False, emit_h2=False, want_f32=True):
        """One convolution on the route forward.conv_route names; emit_h2 / want_f32: what the caller knows about the consumers of the
        result (frcnn_hip/forward.py, "the routes")."""
        N, H, W, Cin = x.shape
        M = N * ops.conv_out_size(H, k, stride, pad[0], pad[1]) * ops.conv_out_size(W, k, stride, pad[2], pad[3])
        route = forward.conv_route(self._plan, scope, k, stride, pad, act, Cin, self._var_specs[scope + "/weights"].shape[-1], M, residual is not None,
                                   res_stride, fold_w, out_affine is not None, no_bias, self._spread(scope), self._forms.has_planes(x) or self._plan.h2_lazy_split)
        out = forward.CONV[route](ops, self._sess, self._plan, self._forms, self._tag, scope, x, k, stride, pad, act, bn_eps, residual,
                                  res_stride, fold_w, out_affine, real_cin, no_bias, emit_h2, want_f32)
        return self._record("conv", out, (x, residual), scope=scope, x=x, k=k, stride=stride, pad=tuple(pad), act=act, residual=residual,
                            res_stride=res_stride)

    def _record(self, kind, y, sources, **fields):
        """TRAIN mode: the tape record of the launches that wrote y; y takes a gradient when one of its sources does, or when the record
        names a filter (`scope`) the solver updates."""
        if self._mode == "TRAIN" and not self._read_only:
            self._tape.append(dict(fields, kind=kind, y=y))
            if ("scope" in fields and self.trainable_scope(fields["scope"])) or any(s is not None and s.data_ptr() in self._requires_grad for s in sources):
                self._requires_grad.add(y.data_ptr())
        return y

    def _spread(self, scope):
        return forward.channel_spread(self._sess, self._plan, scope)

    def _pointwise_route(self, scope, M, Cin, Cout, res_stride=None):
        """The route of the 1x1 / stride 1 convolution `scope` of [M,Cin] -> [M,Cout] (res_stride: of its residual, None = it has none) when
        its input exists as operand planes: what a producer asks about its consumer, answered by the consumer's own rule."""
        return forward.conv_route(self._plan, scope, 1, 1, forward.ZERO_PAD, ACT_RELU, Cin, Cout, M, res_stride is not None, res_stride,
                                  spread=self._spread(scope))

    def _mean_fusable(self, rows, cout, cin, scope, group_rows):
        return forward.mean_fusable(self._plan, rows, cout, cin, group_rows, self._spread(scope))

    def _spatial_mean(self, x):
        """reduce_mean over the positions of every RoI (resnet_v1.py:124) -> fc7 [R, C]"""
        out = self._sess.buf(self._tag + "/fc7", (x.shape[0], x.shape[-1]))
        self._sess.mark("op:spatial_mean", 0, lambda: ops.spatial_mean(x, out=out), nbytes=4 * (x.numel() + out.numel()))
        return self._record("mean", out, (x,), x=x, name=self._scope + "/fc7_mean")

    # ------------------------------------------------------------------ ImageNet-pretrained weights (train_val.py:177-202)
    _rgb_first_conv = None                   # scope tail of the stem conv whose input channels are RGB in the released weights

    def get_variables_to_restore(self, variables, var_keep_dic):
        """Names to restore verbatim from a pretrained checkpoint: everything the checkpoint has, minus the variables
        fix_variables() rewrites (resnet_v1.py:154-167, vgg16.py:62-79, mobilenet_v1.py:253-264)."""
        skip = set(self._variables_to_fix_names())
        self._variables_to_fix = {}
        keep = []
        for name in variables:
            if name in skip:
                self._variables_to_fix[name] = True
                continue
            if name in var_keep_dic:
                keep.append(name)
        return keep

    def _variables_to_fix_names(self):
        return [] if self._rgb_first_conv is None else [self._scope + self._rgb_first_conv + "/weights"]

    def fix_variables(self, sess, pretrained_model):
        """RGB -> BGR on the stem filter (`tf.reverse(conv1_rgb, [2])`, resnet_v1.py:168-178); subclasses add their own."""
        from frcnn_hip.tensor_bundle import open_checkpoint
        reader = open_checkpoint(pretrained_model)
        fixed = {}
        for name in self._variables_to_fix_names():
            fixed[name] = self._fix_one(name, reader.get_tensor(name))
        sess.load_variables(fixed)
        sess.conv_info.clear()
        return sorted(fixed)

    def _fix_one(self, name, value):
        return np.ascontiguousarray(value[:, :, ::-1, :])

    def trainable_scope(self, scope):
        """Which filters the solver updates (reference: `trainable=` flags of the slim layers)."""
        return True

    def _reshape_layer(self, bottom, num_dim, name):
        raise NotImplementedError("folded into frcnn_rpn_softmax (network.py:68-78 only served the pair softmax)")

    def _softmax_layer(self, bottom, name):
        if name.startswith("rpn_cls_prob"):
            A = self._num_anchors
            out = self._sess.buf(self._tag + "/" + name, bottom.shape[:3] + (2 * A,))
            return self._sess.mark("op:rpn_softmax", 0, lambda: ops.rpn_softmax(bottom, A, out=out), nbytes=8 * out.numel())
        out = self._sess.buf(self._tag + "/" + name, bottom.shape)
        return self._sess.mark("op:softmax_rows", 0, lambda: ops.softmax_rows(bottom, out=out), nbytes=8 * out.numel())

    # ------------------------------------------------------------------ graph pieces (same names as the reference)
    def _anchor_component(self):
        # network.py:210-231: feature-map size from im_info; anchors are regenerated in-kernel by the
        # proposal layer, so only the float64 base anchors [A,4] live on the device.
        h = int(np.ceil(self._im_info[0] / np.float32(self._feat_stride[0])))
        w = int(np.ceil(self._im_info[1] / np.float32(self._feat_stride[0])))
        base = ops.generate_anchors(16, self._anchor_ratios, self._anchor_scales)
        if cfg.USE_E2E_TF:
            # generate_anchors_pre_tf (snippets.py:44): tf.constant(anchors, dtype=tf.int32) truncates the base anchors
            base = np.trunc(base)
        key = ("base_anchors", tuple(self._anchor_ratios), tuple(self._anchor_scales), bool(cfg.USE_E2E_TF))
        if key not in self._sess.packed:
            self._sess.packed[key] = self._sess.to_device(base, torch.float64)
        self._base_anchors = self._sess.packed[key]
        self._anchor_length = h * w * self._num_anchors
        self._anchors = None      # materialise on demand with ops.generate_anchors_pre

    @staticmethod
    def _nms_rule():
        """lib/model/nms_wrapper.py:15-23: cfg.USE_GPU_NMS picks the reference's CUDA kernel (`ovr > thresh`,
        nms_kernel.cu:71), otherwise the Cython cpu_nms rule (`ovr >= thresh`, cpu_nms.pyx:65) -- same HIP kernels."""
        return NMS_RULE_GPU if cfg.USE_GPU_NMS else NMS_RULE_CPU

    def _proposal_layer(self, rpn_cls_prob, rpn_bbox_pred, name):
        """network.py:110-131 -> frcnn_proposal_layer_batched: ONE set of launches for the B images of the batch (the
        reference graph is batch-1; a batch here is B independent images whose launches are shared).  rois[:,0] = image index."""
        c = cfg[self._mode]
        post = int(c.RPN_POST_NMS_TOP_N)
        s = self._sess
        B = rpn_cls_prob.shape[0]
        rois = s.buf(self._tag + "/rois", (B * post, 5))
        scores = s.buf(self._tag + "/roi_scores", (B * post, 1))
        num = s.buf(self._tag + "/num_rois", (B,), torch.int32)
        if cfg.USE_E2E_TF:
            # network.py:112-121 -> proposal_layer_tf: tf.image.non_max_suppression over ALL anchors, no pre-NMS top-N
            s.mark("op:proposal_layer_tf", 0, lambda: ops.proposal_layer_tf(
                rpn_cls_prob, rpn_bbox_pred, self._im_info[0], self._im_info[1], self._feat_stride[0],
                self._base_anchors, post, float(c.RPN_NMS_THRESH), rois=rois, scores=scores, num=num))
        else:
            N = rpn_cls_prob.shape[1] * rpn_cls_prob.shape[2] * self._num_anchors
            s.mark("op:proposal_layer", 0, lambda: ops.proposal_layer(
                rpn_cls_prob, rpn_bbox_pred, self._im_info[0], self._im_info[1], self._feat_stride[0],
                self._base_anchors, int(c.RPN_PRE_NMS_TOP_N), post, float(c.RPN_NMS_THRESH), rois=rois, scores=scores, num=num,
                rule=self._nms_rule()), nbytes=B * 36 * N)
        self._num_rois = num
        self._rois_per_image = post
        return rois, scores

    def _proposal_top_layer(self, rpn_cls_prob, rpn_bbox_pred, name):
        # network.py:88-108.  USE_E2E_TF's proposal_top_layer_tf (tf.nn.top_k: descending, equal scores -> lower index first)
        # selects and orders exactly like the kernel's (score desc, index asc) keys, so both settings share it.
        n, s = int(cfg.TEST.RPN_TOP_N), self._sess
        assert rpn_cls_prob.shape[0] == 1, "TEST.MODE 'top' is provided for single images"
        self._rois_per_image = n
        rois, scores = ops.proposal_top_layer(rpn_cls_prob, rpn_bbox_pred, self._im_info[0], self._im_info[1],
                                              self._feat_stride[0], self._base_anchors, n,
                                              rois=s.buf(self._tag + "/top_rois", (n, 5)),
                                              scores=s.buf(self._tag + "/top_scores", (n, 1)))
        self._num_rois = None
        return rois, scores

    def _anchor_target_layer(self, rpn_cls_score, name):
        # network.py:162-183 -> lib/layer_utils/anchor_target_layer.py, on device
        _, H, W, _ = rpn_cls_score.shape
        t = cfg.TRAIN
        labels, tg, iw, ow = ops.anchor_target_layer(self._gt_boxes, self._im_info[0], self._im_info[1], H, W, self._base_anchors,
                                                     self._feat_stride[0], t.RPN_BATCHSIZE, t.RPN_FG_FRACTION, t.RPN_POSITIVE_OVERLAP,
                                                     t.RPN_NEGATIVE_OVERLAP, seed=self._sample_seed,
                                                     opts=ops.rpn_target_opts(t.RPN_CLOBBER_POSITIVES, t.RPN_POSITIVE_WEIGHT,
                                                                              t.RPN_BBOX_INSIDE_WEIGHTS))
        self._anchor_targets = dict(rpn_labels=labels, rpn_bbox_targets=tg, rpn_bbox_inside_weights=iw, rpn_bbox_outside_weights=ow)
        return labels

    def _proposal_target_layer(self, rois, roi_scores, name):
        # network.py:185-208 -> lib/layer_utils/proposal_target_layer.py, on device
        t = cfg.TRAIN
        # the padded proposal buffer goes in whole; the kernel reads the valid row count on the device (no host sync here)
        out = ops.proposal_target_layer(rois, roi_scores.view(-1), self._gt_boxes, self._num_classes,
                                        t.BATCH_SIZE, t.FG_FRACTION, t.FG_THRESH, t.BG_THRESH_HI, t.BG_THRESH_LO,
                                        t.BBOX_NORMALIZE_MEANS, t.BBOX_NORMALIZE_STDS, seed=self._sample_seed + 1, num=self._num_rois,
                                        opts=ops.roi_target_opts(t.USE_GT, t.BBOX_INSIDE_WEIGHTS))
        rois, roi_scores, labels, tg, iw, ow, counts = out
        # the sampled RoIs live at ONE address for the life of the session: the tape's crop record names them, and a captured reverse
        # sweep (cfg.HIP.TRAIN_GRAPH) is only valid for the tensors it was recorded with
        rois = ops.t_copy(self._sess.buf(self._tag + "/" + name + "/rois", tuple(rois.shape)), rois)
        self._proposal_targets = dict(rois=rois, labels=labels, bbox_targets=tg, bbox_inside_weights=iw, bbox_outside_weights=ow,
                                      counts=counts)
        self._num_rois = None
        return rois, roi_scores

    def _ohem_scores(self, net_conv, rois):
        """cfg.HIP.OHEM: cls_score [N,C] / bbox_pred [N,4C] of ALL N rows of the padded proposal buffer under the current weights -- pool5,
        _head_to_tail (without dropout) and _region_classification with the training pass's plan and routes, as a READ-ONLY pass: nothing
        goes on the tape, its activations live under the tag suffix "/ohem" (Session.buf keys by name and shape: with N == BATCH_SIZE the
        training pass would otherwise write the same buffers), and _predictions / _layers are left for the training pass to write.  Batch
        norm is frozen, so this is the arithmetic of the training forward.  Derived filters (operand planes, Winograd U) come from the
        session's caches and PreparedFilters like everybody's, so they follow the solver."""
        tag, preds, layers = self._tag, dict(self._predictions), dict(self._layers)
        self._tag, self._forms.tag, self._read_only = tag + "/ohem", tag + "/ohem", True
        try:
            pool5 = self._crop_pool_layer(net_conv, rois, "pool5")
            fc7 = self._head_to_tail(pool5, False)
            self._region_classification(fc7, False)
            return self._predictions["cls_score"], self._predictions["bbox_pred"]
        finally:
            self._tag, self._forms.tag, self._read_only = tag, tag, False
            self._predictions, self._layers = preds, layers

    def _ohem_target_layer(self, net_conv, rois, roi_scores, name):
        """cfg.HIP.OHEM instead of _proposal_target_layer: the BATCH_SIZE proposals with the largest loss (csrc/ohem_math.h)"""
        t = cfg.TRAIN
        cls_score, bbox_pred = self._ohem_scores(net_conv, rois)
        out = ops.ohem_select(rois, roi_scores.view(-1), self._num_rois, self._gt_boxes, self._num_classes, cls_score, bbox_pred,
                              t.BATCH_SIZE, t.FG_THRESH, t.BG_THRESH_HI, t.BG_THRESH_LO, t.BBOX_NORMALIZE_MEANS, t.BBOX_NORMALIZE_STDS,
                              opts=ops.roi_target_opts(t.USE_GT, t.BBOX_INSIDE_WEIGHTS), nms_thresh=float(cfg.HIP.OHEM_NMS_THRESH),
                              rule=self._nms_rule())
        proposals, proposal_scores, num = rois, roi_scores, self._num_rois
        rois, roi_scores, labels, tg, iw, ow, counts, keep, loss = out
        rois = ops.t_copy(self._sess.buf(self._tag + "/" + name + "/rois", tuple(rois.shape)), rois)      # (as _proposal_target_layer)
        self._proposal_targets = dict(rois=rois, labels=labels, bbox_targets=tg, bbox_inside_weights=iw, bbox_outside_weights=ow,
                                      counts=counts)
        self._ohem = dict(keep_inds=keep, roi_loss=loss, cls_score=cls_score, bbox_pred=bbox_pred, proposals=proposals,
                          proposal_scores=proposal_scores, num_rois=num)
        self._num_rois = None
        return rois, roi_scores

    def _smooth_l1_loss(self, bbox_pred, bbox_targets, bbox_inside_weights, bbox_outside_weights, sigma=1.0, dim=[1]):
        """network.py:264-277 -> (loss [1], d loss / d bbox_pred).  dim=[1]: mean over rows; dim=[1,2,3]: batch of 1."""
        div = float(bbox_pred.shape[0]) if list(dim) == [1] else 1.0
        return ops.smooth_l1_loss(bbox_pred, bbox_targets, bbox_inside_weights, bbox_outside_weights, sigma, div)

    def _add_losses(self, sigma_rpn=3.0):
        """network.py:279-321.  Returns the loss tensors and the seed gradients of the four network outputs."""
        A = self._num_anchors
        p, at, pt = self._predictions, self._anchor_targets, self._proposal_targets
        _, H, W, _ = p["rpn_cls_score"].shape
        rpn_ce, g_rpn_cls = ops.softmax_ce_loss(p["rpn_cls_score"], at["rpn_labels"], rpn_shape=(A, H, W))
        h, t = cfg.HIP, cfg.TRAIN
        if h.RPN_BBOX_LOSS == "smooth_l1":
            rpn_box, g_rpn_box = self._smooth_l1_loss(p["rpn_bbox_pred"], at["rpn_bbox_targets"], at["rpn_bbox_inside_weights"],
                                                      at["rpn_bbox_outside_weights"], sigma=sigma_rpn, dim=[1, 2, 3])
        else:
            # csrc/iouloss_math.h on the anchors the anchor target layer encoded against (it builds them in-kernel from the same base
            # anchors): [1,H,W,4A] read as [H W A, 4], RPN targets are not normalised, batch of 1 like dim=[1, 2, 3] above
            # (kept beside the targets, not among them: _anchor_targets is what the score summaries list)
            self._rpn_anchors = ops.generate_anchors_pre(H, W, self._feat_stride[0], self._base_anchors)
            rpn_box, g_rpn_box = ops.iou_loss(p["rpn_bbox_pred"], at["rpn_bbox_targets"], at["rpn_bbox_inside_weights"],
                                              at["rpn_bbox_outside_weights"], self._rpn_anchors, (0.0, 0.0, 0.0, 0.0), (1.0, 1.0, 1.0, 1.0),
                                              h.RPN_BBOX_LOSS, float(h.RPN_BBOX_LOSS_WEIGHT), 1.0, 1)
        ce, g_cls = ops.softmax_ce_loss(p["cls_score"], pt["labels"].view(-1))
        if h.BBOX_LOSS == "smooth_l1":
            box, g_box = self._smooth_l1_loss(p["bbox_pred"], pt["bbox_targets"], pt["bbox_inside_weights"], pt["bbox_outside_weights"])
        else:
            # on the sampled RoIs, with the means / stds _proposal_target_layer normalised the targets by; the mean over the rows as above
            box, g_box = ops.iou_loss(p["bbox_pred"], pt["bbox_targets"], pt["bbox_inside_weights"], pt["bbox_outside_weights"], pt["rois"],
                                      t.BBOX_NORMALIZE_MEANS, t.BBOX_NORMALIZE_STDS, h.BBOX_LOSS, float(h.BBOX_LOSS_WEIGHT),
                                      float(p["bbox_pred"].shape[0]), self._num_classes)
        self._losses = dict(cross_entropy=ce, loss_box=box, rpn_cross_entropy=rpn_ce, rpn_loss_box=rpn_box)
        self._loss_seeds = [(p["rpn_cls_score"], g_rpn_cls), (p["rpn_bbox_pred"], g_rpn_box), (p["cls_score"], g_cls),
                            (p["bbox_pred"], g_box)]
        return self._losses

    def _crop_images(self, bottom, rois, out, max_pool=False, bias=None, act=ACT_NONE):
        """tf.image.crop_and_resize(bottom, boxes, box_ind = rois[:,0]) (network.py:141-157) for the whole batch in one launch."""
        fs, P = float(self._feat_stride[0]), cfg.POOLING_SIZE
        self._forms.need_f32(bottom)
        nbytes = 4 * (bottom.numel() + out.numel())
        if cfg.POOLING_MODE == "align":              # csrc/roialign_math.h; max_pool does not apply (see _crop_pool)
            S = int(cfg.HIP.ROI_ALIGN_SAMPLES)
            self._sess.mark("op:roi_align", 0, lambda: ops.roi_align_bias_act(bottom, rois, fs, P, S, bias, act, out=out), nbytes=nbytes)
        elif bias is None and act == ACT_NONE:
            self._sess.mark("op:crop_and_resize", 0, lambda: ops.crop_and_resize(bottom, rois, fs, P, max_pool=max_pool, out=out), nbytes=nbytes)
        else:
            self._sess.mark("op:crop_and_resize", 0, lambda: ops.crop_and_resize_bias_act(bottom, rois, fs, P, bias, act, out=out), nbytes=nbytes)
        return self._forms.wrote(out)

    def _crop_pool_layer(self, bottom, rois, name):
        # network.py:141-157: 14x14 crop + 2x2 max pool (TEST: fused in one kernel)
        return self._crop_pool(bottom, rois, name, max_pool=True)

    def _crop_pool(self, bottom, rois, name, max_pool):
        """RoI pooling.  TEST: one kernel (the 2x2 max fused).  TRAIN: crop and max pool are separate tape records so that the
        reverse sweep routes the gradient through the arg-max and then through the bilinear taps."""
        P, C = cfg.POOLING_SIZE, bottom.shape[-1]
        R = rois.shape[0]
        fs = float(self._feat_stride[0])
        if cfg.POOLING_MODE == "align":
            # RoIAlign in its standard form for every backbone: POOLING_SIZE x POOLING_SIZE bins of S x S samples, no 14x14 + 2x2 max detour
            S = int(cfg.HIP.ROI_ALIGN_SAMPLES)
            out = self._crop_images(bottom, rois, self._sess.buf(self._tag + "/" + name, (R, P, P, C)))
            return self._record("roi_align", out, (bottom,), feat=bottom, rois=rois, stride=fs, samples=S)
        if self._mode != "TRAIN":
            return self._crop_images(bottom, rois, self._sess.buf(self._tag + "/" + name, (R, P, P, C)), max_pool=max_pool)
        pre = 2 * P if max_pool else P
        crop = self._sess.buf(self._tag + "/" + name + ("/crop" if max_pool else ""), (R, pre, pre, C))
        self._sess.mark("op:crop_and_resize", 0, lambda: ops.crop_and_resize(bottom, rois, fs, pre, max_pool=False, out=crop),
                        nbytes=4 * (bottom.numel() + crop.numel()))
        self._record("crop", self._forms.wrote(crop), (bottom,), feat=bottom, rois=rois, stride=fs)
        return self._max_pool(crop, 2, 2, name) if max_pool else crop

    def _max_pool(self, x, k, stride, name):
        """slim.max_pool2d(padding='SAME') for k == stride (pads bottom / right only, out = ceil(n / stride)); recorded in TRAIN mode."""
        N, H, W, C = x.shape
        OH, OW = (H + stride - 1) // stride, (W + stride - 1) // stride
        out = self._sess.buf(self._tag + "/" + name, (N, OH, OW, C))
        pad = (0, (OH - 1) * stride + k - H, 0, (OW - 1) * stride + k - W)
        self._sess.mark("op:maxpool", 0, lambda: ops.maxpool(x, k, stride, pad, out=out), nbytes=4 * (x.numel() + out.numel()))
        return self._record("maxpool", self._forms.wrote(out), (x,), x=x, k=k, stride=stride, name=name)

    def weight_decay_for(self, scope):
        """L2 coefficient of one layer's weights; None = cfg.TRAIN.WEIGHT_DECAY (network.py:303-311 arg_scope)."""
        return None

    def _region_proposal(self, net_conv, is_training, initializer=None):
        A = self._num_anchors
        rpn = self._conv(net_conv, self._scope + "/rpn_conv/3x3", 3, 1, (1, 1, 1, 1), ACT_RELU)          # :324-325
        self._act_summaries.append(rpn)
        rpn_cls_score = self._conv(rpn, self._scope + "/rpn_cls_score", 1, act=ACT_NONE)                   # :327-329
        rpn_cls_prob = self._softmax_layer(rpn_cls_score, "rpn_cls_prob")                                   # :331-334
        rpn_bbox_pred = self._conv(rpn, self._scope + "/rpn_bbox_pred", 1, act=ACT_NONE)                   # :335-337
        if is_training:                                                                                    # :338-343
            rois, roi_scores = self._proposal_layer(rpn_cls_prob, rpn_bbox_pred, "rois")
            self._anchor_target_layer(rpn_cls_score, "anchor")
            if cfg.HIP.OHEM:
                rois, _ = self._ohem_target_layer(net_conv, rois, roi_scores, "rpn_rois")
            else:
                rois, _ = self._proposal_target_layer(rois, roi_scores, "rpn_rois")
        elif cfg.TEST.MODE == "nms":
            rois, _ = self._proposal_layer(rpn_cls_prob, rpn_bbox_pred, "rois")
        elif cfg.TEST.MODE == "top":
            rois, _ = self._proposal_top_layer(rpn_cls_prob, rpn_bbox_pred, "rois")
        else:
            raise NotImplementedError
        self._predictions["rpn_cls_score"] = rpn_cls_score
        self._predictions["rpn_cls_prob"] = rpn_cls_prob
        self._predictions["rpn_bbox_pred"] = rpn_bbox_pred
        self._predictions["rois"] = rois
        return rois

    def _region_classification(self, fc7, is_training, initializer=None, initializer_bbox=None):
        R = fc7.shape[0]
        x = fc7.view(1, 1, R, fc7.shape[1])
        cls_score = self._conv(x, self._scope + "/cls_score", 1, act=ACT_NONE).view(R, self._num_classes)   # :362-366
        cls_prob = self._softmax_layer(cls_score, "cls_prob")
        affine = None
        if self._mode == "TEST":      # network.py:428-432: bbox_pred * stds + means, folded into the fc
            affine = (np.tile(np.array(cfg.TRAIN.BBOX_NORMALIZE_STDS), self._num_classes),
                      np.tile(np.array(cfg.TRAIN.BBOX_NORMALIZE_MEANS), self._num_classes))
        bbox_pred = self._conv(x, self._scope + "/bbox_pred", 1, act=ACT_NONE, out_affine=affine).view(R, 4 * self._num_classes)
        self._predictions["cls_score"] = cls_score
        self._predictions["cls_prob"] = cls_prob
        self._predictions["bbox_pred"] = bbox_pred
        return cls_prob, bbox_pred

    def _image_to_head(self, is_training, reuse=None):
        raise NotImplementedError

    def _head_to_tail(self, pool5, is_training, reuse=None):
        raise NotImplementedError

    class _plan_context(object):
        """The batch-invariant launch plan around a graph build: TEST-mode rules (matrix pipe, split-K plan, f32 tile configuration) see the
        PER-IMAGE shape whatever the batch is -- forward.plan_rows here, launch context key 8 inside the library.  Entering it starts a build: the
        network gets the build's Plan (the switches as they are now) and an empty Forms, and keeps both (a sub-graph re-run later continues them)."""

        def __init__(self, net, is_training):
            self.net, self.batch = net, 0 if is_training else int(net._image.shape[0])

        def __enter__(self):
            from frcnn_hip import lib
            net = self.net
            net._plan = forward.make_plan(net._mode, self.batch, cfg.HIP)
            net._forms = forward.Forms(ops, net._sess, net._tag, net._plan.h2_lazy_split)
            lib().frcnn_set_tuning(8, self.batch)        # the same rule inside the library (split-K plan of frcnn_conv2d_nhwc_ws)

        def __exit__(self, *exc):
            from frcnn_hip import lib
            lib().frcnn_set_tuning(8, 0)
            return False

    def _build_network(self, is_training=True):
        with self._plan_context(self, is_training):
            return self._build_network_impl(is_training)

    def _build_network_impl(self, is_training=True):
        self._tape = []
        self._requires_grad = set()
        self._act_summaries = []                        # this build's [head, rpn] (the backbones and _region_proposal append)
        net_conv = self._image_to_head(is_training)
        self._anchor_component()
        fused = self._fuse_tail_entry and not is_training and hasattr(self, "_fused_tail_entry")      # a method of resnetv1 only
        rois = self._region_proposal(net_conv, is_training)
        if fused:
            fc7 = self._fused_tail_entry(net_conv, rois)                # crop commuted past the first 1x1 convs (exact algebra)
        else:
            pool5 = self._crop_pool_layer(net_conv, rois, "pool5")
            self._layers["pool5"] = pool5
            fc7 = self._head_to_tail(pool5, is_training)
        self._layers["fc7"] = fc7
        cls_prob, bbox_pred = self._region_classification(fc7, is_training)
        return rois, cls_prob, bbox_pred

    _trainable_on_device = False          # subclasses whose whole TRAIN graph has a reverse sweep (frcnn_hip/train.py) set True

    @staticmethod
    def _check_supported_cfg(mode):
        """Config keys implemented for ONE value only: refuse the others instead of silently ignoring them.  (TRAIN.USE_GT,
        RPN_CLOBBER_POSITIVES, RPN_POSITIVE_WEIGHT, the two INSIDE_WEIGHTS, TRAIN.TRUNCATED and TEST.BBOX_REG are kernel / initialiser
        arguments since round 3; POOLING_MODE is 'crop' only in the reference, network.py:393-396 -- here also 'align', RoIAlign with
        HIP.ROI_ALIGN_SAMPLES in 1..4 and without RESNET.MAX_POOL; 'pool' and everything else stay refused.)"""
        t = cfg.TRAIN
        bad = []
        if cfg.POOLING_MODE not in ("crop", "align"):
            bad.append("POOLING_MODE = %r (only 'crop' and 'align' are implemented)" % (cfg.POOLING_MODE,))
        if cfg.POOLING_MODE == "align":
            if cfg.HIP.ROI_ALIGN_SAMPLES not in (1, 2, 3, 4):
                bad.append("HIP.ROI_ALIGN_SAMPLES = %r (1..4 samples per bin side)" % (cfg.HIP.ROI_ALIGN_SAMPLES,))
            if cfg.RESNET.MAX_POOL:
                bad.append("RESNET.MAX_POOL = True with POOLING_MODE = 'align' (RoIAlign pools POOLING_SIZE x POOLING_SIZE bins directly)")
        if float(t.RPN_POSITIVE_WEIGHT) >= 0 and not (0.0 < float(t.RPN_POSITIVE_WEIGHT) < 1.0):
            bad.append("TRAIN.RPN_POSITIVE_WEIGHT = %r (the reference asserts 0 < p < 1, anchor_target_layer.py:103-104)" % (t.RPN_POSITIVE_WEIGHT,))
        h = cfg.HIP
        if h.SOFT_NMS not in (0, 1, 2):
            bad.append("HIP.SOFT_NMS = %r (0 = hard NMS, 1 = linear, 2 = Gaussian)" % (h.SOFT_NMS,))
        if not float(h.SOFT_NMS_SIGMA) > 0:
            bad.append("HIP.SOFT_NMS_SIGMA = %r (must be > 0)" % (h.SOFT_NMS_SIGMA,))
        if not float(h.SOFT_NMS_MIN_SCORE) >= 0:
            bad.append("HIP.SOFT_NMS_MIN_SCORE = %r (must be >= 0)" % (h.SOFT_NMS_MIN_SCORE,))
        if not 0.0 < float(h.BBOX_VOTE_THRESH) <= 1.0:
            bad.append("HIP.BBOX_VOTE_THRESH = %r (must be in (0, 1])" % (h.BBOX_VOTE_THRESH,))
        if h.OHEM:
            if not float(h.OHEM_NMS_THRESH) <= 1.0:
                bad.append("HIP.OHEM_NMS_THRESH = %r (at most 1; <= 0 skips the NMS)" % (h.OHEM_NMS_THRESH,))
            if t.USE_GT:
                bad.append("TRAIN.USE_GT = True with HIP.OHEM (the candidates are the proposal rows of the read-only pass)")
            if int(t.RPN_POST_NMS_TOP_N) > Network.OHEM_MAX_ROWS or int(t.BATCH_SIZE) > Network.OHEM_MAX_ROWS:
                bad.append("HIP.OHEM with TRAIN.RPN_POST_NMS_TOP_N = %d, TRAIN.BATCH_SIZE = %d (frcnn_ohem_select holds at most %d rows)"
                           % (int(t.RPN_POST_NMS_TOP_N), int(t.BATCH_SIZE), Network.OHEM_MAX_ROWS))
        for key in ("BBOX_LOSS", "RPN_BBOX_LOSS"):
            if h[key] not in Network.BOX_LOSSES:
                bad.append("HIP.%s = %r (one of %s)" % (key, h[key], ", ".join(repr(v) for v in Network.BOX_LOSSES)))
            elif h[key] != "smooth_l1":
                w = h[key + "_WEIGHT"]
                if isinstance(w, bool) or not isinstance(w, (int, float)) or not (0.0 < float(w) < float("inf")):
                    bad.append("HIP.%s_WEIGHT = %r (must be finite and > 0)" % (key, w))
        if h.OHEM and h.BBOX_LOSS != "smooth_l1":
            bad.append("HIP.OHEM with HIP.BBOX_LOSS = %r (csrc/ohem_math.h ranks the RoIs by the smooth-L1 loss; mining by one loss and "
                       "training on another is refused)" % (h.BBOX_LOSS,))
        if h.TEST_FLIP and mode == "TEST":
            bad += Network._flip_refusals()
        if bad:
            raise NotImplementedError("unsupported configuration for the HIP path: " + "; ".join(bad))

    BOX_LOSSES = ("smooth_l1", "iou", "giou", "diou", "ciou")      # HIP.BBOX_LOSS / HIP.RPN_BBOX_LOSS (model.config.BOX_LOSSES)
    OHEM_MAX_ROWS = 3072                  # OHEM_MAXN of csrc/ohem_math.h: proposal rows, and rows of the batch
    FLIP_MAX_ROWS = 1024                  # rows per image and class the post-processing holds (frcnn_detect_post_*: R <= 1024)

    @staticmethod
    def _flip_refusals():
        """what HIP.TEST_FLIP cannot run with: the merged image has 2 * RPN_POST_NMS_TOP_N rows, refused rather than truncated"""
        bad = []
        if cfg.TEST.MODE != "nms":
            bad.append("HIP.TEST_FLIP with TEST.MODE = %r (the flip ensemble merges the 'nms' proposals of two views)" % (cfg.TEST.MODE,))
        elif 2 * int(cfg.TEST.RPN_POST_NMS_TOP_N) > Network.FLIP_MAX_ROWS:
            bad.append("HIP.TEST_FLIP with TEST.RPN_POST_NMS_TOP_N = %d (two views give %d rows per image, the post-processing holds at most %d)"
                       % (int(cfg.TEST.RPN_POST_NMS_TOP_N), 2 * int(cfg.TEST.RPN_POST_NMS_TOP_N), Network.FLIP_MAX_ROWS))
        return bad

    def create_architecture(self, mode, num_classes, tag=None, anchor_scales=(8, 16, 32), anchor_ratios=(0.5, 1, 2)):
        assert tag is not None
        self._check_supported_cfg(mode)
        if mode == "TRAIN" and not self._trainable_on_device:
            raise NotImplementedError("%s: no reverse sweep for this network's TRAIN graph; TEST mode works" % type(self).__name__)
        self._tag = tag
        self._num_classes = num_classes
        self._mode = mode
        self._anchor_scales = tuple(anchor_scales)
        self._num_scales = len(anchor_scales)
        self._anchor_ratios = tuple(anchor_ratios)
        self._num_ratios = len(anchor_ratios)
        self._num_anchors = self._num_scales * self._num_ratios
        A = self._num_anchors
        self._var_specs.clear()
        self._declare_backbone()
        hc = self._head_channels()
        self._declare_conv_bias(self._scope + "/rpn_conv/3x3", 3, 3, hc, cfg.RPN_CHANNELS, 0.01)           # :239-240,324
        self._declare_conv_bias(self._scope + "/rpn_cls_score", 1, 1, cfg.RPN_CHANNELS, 2 * A, 0.01)
        self._declare_conv_bias(self._scope + "/rpn_bbox_pred", 1, 1, cfg.RPN_CHANNELS, 4 * A, 0.01)
        tc = self._tail_channels()
        self._var(self._scope + "/cls_score/weights", (tc, num_classes), "normal", 0.01)
        self._var(self._scope + "/cls_score/biases", (num_classes,), "zeros")
        self._var(self._scope + "/bbox_pred/weights", (tc, 4 * num_classes), "normal", 0.001)
        self._var(self._scope + "/bbox_pred/biases", (4 * num_classes,), "zeros")
        names = ["rois", "rpn_cls_score", "rpn_cls_prob", "rpn_bbox_pred", "cls_score", "cls_prob", "bbox_pred"]
        return {k: k for k in names}

    # ------------------------------------------------------------------ execution
    def _stage_image(self, sess, image, im_info=None):
        """[1,H,W,3] (BGR - PIXEL_MEANS, like blobs['data']) -> static device buffer [1,H,W,4]; the
        zero 4th channel lets the 7x7/3x3 stem run as a channel-folded MFMA GEMM.  im_info given: the buffer belongs to that image
        shape's scope (freed with the shape's graph); otherwise to the session."""
        if isinstance(image, np.ndarray):
            image = torch.from_numpy(np.ascontiguousarray(image, dtype=np.float32))
        B, H, W, C = image.shape
        if im_info is None:
            buf = sess.buf(self._tag + "/image", (B, H, W, 4), zero=True)
        else:
            with self.shape_scope(sess, (B, H, W, 4), im_info):
                buf = sess.buf(self._tag + "/image", (B, H, W, 4), zero=True)
        buf[..., :C].copy_(image, non_blocking=True)
        return buf

    def graph_key(self, image_shape, im_info):
        """Everything a captured TEST-mode chain depends on: network, image shape, im_info, the configuration outside the plan, and the
        plan the build of this shape would get (forward.Plan.key: every switch a route rule or a route reads)."""
        c = cfg[self._mode]
        return (self._tag, self._scope, self._num_classes, self._anchor_scales, self._anchor_ratios, bool(cfg.RESNET.MAX_POOL),
                bool(cfg.USE_GPU_NMS), tuple(int(v) for v in image_shape), (float(im_info[0]), float(im_info[1])), cfg.TEST.MODE, self._fuse_tail_entry,
                c.RPN_PRE_NMS_TOP_N, c.RPN_POST_NMS_TOP_N, c.RPN_NMS_THRESH, cfg.TEST.RPN_TOP_N, cfg.POOLING_SIZE, bool(cfg.USE_E2E_TF),
                cfg.POOLING_MODE, int(cfg.HIP.ROI_ALIGN_SAMPLES)) + forward.make_plan(self._mode, 0 if self._mode == "TRAIN" else image_shape[0], cfg.HIP).key()

    def shape_scope(self, sess, image_shape, im_info):
        """The buffer scope of one image shape of this network (frcnn_hip/runtime.py Session.shape_scope): at most cfg.HIP.GRAPH_CACHE_SHAPES
        shapes per network tag keep their captured graph and buffers; the least recently used shape goes first.  The reference's graph takes
        [1, None, None, 3] and test_net walks an imdb of hundreds of sizes (lib/nets/network.py:386-390, lib/model/test.py:138-185)."""
        return sess.shape_scope(self.graph_key(image_shape, im_info), group=("graphs", self._tag), cap=int(cfg.HIP.GRAPH_CACHE_SHAPES))

    def forward_device(self, sess, image_d, im_info, use_graph=True):
        """Runs the network on a staged device image; fills self._predictions with DEVICE tensors.
        The whole chain is captured into one hipGraph per (tag, image shape) and replayed; graph and buffers live in the shape's scope."""
        self._sess = sess
        self._image = image_d
        self._im_info = (float(im_info[0]), float(im_info[1]), float(im_info[2]))
        sess.prepared.wait_planes()                    # a solver sharing the session re-derives filter planes on a side stream (a replay reads them)
        ops.ws_scope = self._tag                       # scratch buffers are per network tag (= per stream)
        key = self.graph_key(image_d.shape, self._im_info)
        with self.shape_scope(sess, image_d.shape, self._im_info):
            if not use_graph or sess.profile is not None:
                sess.flops_last_forward = 0
                self._build_network(self._mode == "TRAIN")
                return self._predictions
            replay.launch_captured(sess, key, key, lambda: self._build_network(False), image_d,
                                   lambda out: (self._rois_per_image, (dict(self._predictions), self._num_rois)), self._restore_forward)
        return self._predictions

    def _restore_forward(self, ent):
        """what a replay of a captured forward_device chain leaves on the network and the session (replay.launch_captured)"""
        preds, self._num_rois = ent.state
        self._predictions, self._sess.flops_last_forward, self._rois_per_image = dict(preds), ent.flops, ent.per

    def _restore_proposals(self, ent):
        """... and of a captured propose_device chain (ent.state: the (rois, roi_scores, num_rois) it returns)"""
        self._num_rois, self._sess.flops_last_forward, self._rois_per_image = ent.state[2], ent.flops, ent.per

    def _build_proposals(self):
        """_build_network_impl up to the proposals: head, anchors, _region_proposal -> (rois, roi_scores, num_rois int32 [B])"""
        with self._plan_context(self, False):
            self._tape = []
            self._requires_grad = set()
            self._act_summaries = []
            net_conv = self._image_to_head(False)
            self._anchor_component()
            rois = self._region_proposal(net_conv, False)
        B, per, s = int(self._image.shape[0]), self._rois_per_image, self._sess
        if self._num_rois is None:                                # TEST.MODE 'top': always RPN_TOP_N rows
            return rois, s.buf(self._tag + "/top_scores", (per, 1)), torch.full((B,), per, dtype=torch.int32, device=rois.device)
        return rois, s.buf(self._tag + "/roi_scores", (B * per, 1)), self._num_rois

    def propose_device(self, sess, image_d, im_info, use_graph=True):
        """The RPN alone on a staged device image (TEST mode): head, anchors and _region_proposal under forward_device's plan context and
        shape scope, and nothing after them -- no crop, no tail, no classifier.  -> (rois [B*post,5], roi_scores [B*post,1], num_rois
        int32 [B]) on the device, the very buffers and launches of forward_device, so the same bits for the same image and
        configuration; a later call or forward_device of the same shape overwrites them in stream order.  TEST.MODE 'nms' is captured
        into a hipGraph of its own per shape and replayed, under the key ("propose",) + graph_key -- forward_device's graphs and every
        recorded step keep their keys; the entry names the shape's scope, so it is dropped with the shape's buffers."""
        assert self._mode == "TEST", "propose_device is a test-time path"
        self._sess = sess
        self._image = image_d
        self._im_info = (float(im_info[0]), float(im_info[1]), float(im_info[2]))
        sess.prepared.wait_planes()
        ops.ws_scope = self._tag
        scope_key = self.graph_key(image_d.shape, self._im_info)
        key = ("propose",) + scope_key
        with self.shape_scope(sess, image_d.shape, self._im_info):
            if not use_graph or sess.profile is not None or cfg.TEST.MODE != "nms":
                sess.flops_last_forward = 0
                return self._build_proposals()
            return replay.launch_captured(sess, key, scope_key, self._build_proposals, image_d,
                                          lambda out: (self._rois_per_image, out), self._restore_proposals).state

    # only useful during testing mode
    def extract_head(self, sess, image):
        self._sess = sess
        sess.prepared.wait_planes()
        shape = (int(image.shape[0]), int(image.shape[1]), int(image.shape[2]), 4)
        with sess.shape_scope(("extract_head", self._tag, shape), group=("head", self._tag), cap=int(cfg.HIP.GRAPH_CACHE_SHAPES)):
            self._image = self._stage_image(sess, image)
            ops.ws_scope = self._tag
            with self._plan_context(self, False):          # the same launch plan as forward_device: the same bits for the same image
                feat = self._image_to_head(False)
            return feat.cpu().numpy()

    # only useful during testing mode
    def test_image(self, sess, image, im_info):
        """network.py:470-479: returns cls_score, cls_prob, bbox_pred, rois as numpy arrays (rows of
        the `num_rois` proposals that survived NMS)."""
        img = self._stage_image(sess, image, im_info)
        p = self.forward_device(sess, img, im_info)
        assert img.shape[0] == 1, "test_image keeps the reference's single-image contract (network.py:388); use detect_device for batches"
        n = p["rois"].shape[0] if self._num_rois is None else int(self._num_rois.item())
        return (p["cls_score"][:n].cpu().numpy(), p["cls_prob"][:n].cpu().numpy(), p["bbox_pred"][:n].cpu().numpy(),
                p["rois"][:n].cpu().numpy())

    # ------------------------------------------------------------------ training (network.py:488-516)
    def _stage_train_inputs(self, sess, blobs):
        """blobs -> the step's static input buffers: image [1,H,W,4] (like _stage_image), gt boxes in a [TRAIN_MAX_GT,5] buffer whose
        first G rows are valid (G is a launch argument of the two target layers, the only consumers), im_info as host floats (launch
        arguments; part of a recorded step's key).  A blob without 'data' is RoIDataLayer's raw-image form (roi_data_layer/minibatch.py):
        the uint8 image and the roidb's uint16 boxes / int32 classes go to the device as they are and frcnn_prep_train_image writes both
        static buffers there (mirror, mean, resize; boxes * im_scale)."""
        self._sess = sess
        info = blobs["im_info"]
        self._im_info = (float(info[0]), float(info[1]), float(info[2]))
        if "data" not in blobs:
            im = blobs["image"]
            im_scale, OH, OW = self._train_prep_shape(blobs)
            dev = sess.device
            G = int(blobs["boxes"].shape[0])
            cap = max(self.TRAIN_MAX_GT, (G + 63) // 64 * 64)
            self._image = sess.buf(self._tag + "/image", (1, OH, OW, 4), zero=True)
            buf = sess.buf(self._tag + "/gt_boxes", (cap, 5), zero=True)
            im_d = (im if torch.is_tensor(im) else torch.from_numpy(np.ascontiguousarray(im))).to(dev, non_blocking=True)   # cfg.HIP.JPEG_DEVICE: decoded there
            boxes_d = torch.from_numpy(np.ascontiguousarray(blobs["boxes"], dtype=np.uint16)).to(dev, non_blocking=True) if G else None
            classes_d = torch.from_numpy(np.ascontiguousarray(blobs["gt_classes"], dtype=np.int32)).to(dev, non_blocking=True) if G else None
            ops.prep_train_image(im_d, bool(blobs["flipped"]), cfg.PIXEL_MEANS, im_scale, (OH, OW), out=self._image, out_c=4,
                                 boxes=boxes_d, classes=classes_d, gt_out=buf)
            self._gt_boxes = buf[:G]
            return
        self._image = self._stage_image(sess, blobs["data"])
        gt = blobs["gt_boxes"]
        gt = gt if torch.is_tensor(gt) else torch.from_numpy(np.ascontiguousarray(gt, dtype=np.float32))
        G = int(gt.shape[0])
        cap = max(self.TRAIN_MAX_GT, (G + 63) // 64 * 64)
        buf = sess.buf(self._tag + "/gt_boxes", (cap, 5), zero=True)
        buf[:G].copy_(gt, non_blocking=True)
        self._gt_boxes = buf[:G]

    @staticmethod
    def _train_prep_shape(blobs):
        """(im_scale, OH, OW) of a raw-image blob: blob.py:37-45 for its target size (frcnn_prep_image_shape)."""
        h, w = blobs["image"].shape[:2]
        return ops.prep_image_shape(h, w, int(blobs["target_size"]), int(blobs.get("max_size", cfg.TRAIN.MAX_SIZE)))

    TRAIN_MAX_GT = 128          # rows of the static gt buffer (grows in steps of 64 for an image with more boxes: a new recorded-step key)

    def train_forward(self, sess, blobs):
        """TRAIN-mode forward + losses on the device (eager; the tape for the reverse sweep is recorded)."""
        assert self._mode == "TRAIN"
        self._stage_train_inputs(sess, blobs)
        return self._train_forward_staged(sess)

    def _train_forward_staged(self, sess):
        ops.ws_scope = self._tag
        sess.flops_last_forward = 0
        sess.prepared.enabled = bool(cfg.HIP.PREP_STREAM)
        self._build_network(True)
        return self._add_losses()

    def train_step(self, sess, blobs, train_op):
        """One SGD step.  `train_op` is the solver handle (frcnn_hip.train.TrainState with .lr set), the stand-in
        for the reference's TF train op.  Returns the five losses like network.py:488-498 (one host read-back)."""
        return tuple(float(v) for v in self.train_step_async(sess, blobs, train_op).cpu().tolist())

    def train_step_async(self, sess, blobs, train_op):
        """train_step without the host read-back: returns a DEVICE tensor [5] = (rpn_loss_cls, rpn_loss_box, loss_cls, loss_box,
        total_loss).  Nothing in the step synchronises with the host, so the launch queue stays ahead of the GPU across steps.

        cfg.HIP.TRAIN_REPLAY (default): the reference runs a step as ONE `sess.run` of a graph built once (network.py:488-498); here the
        second step of an image shape is recorded while it runs eagerly (frcnn_hip/replay.py: every C-ABI launch, event record / wait,
        tensor copy and collective of the step, streams as slots) and every later step of that shape replays the list -- the same
        launches, arguments, streams and order, hence the same bits, without the ~14 ms of Python a step costs the host."""
        assert self._mode == "TRAIN"
        with self._train_scope(sess, blobs):
            self._stage_train_inputs(sess, blobs)
            self.configure_train_op(train_op)                # before the recording's key: replay_signature() carries what this sets
            if not cfg.HIP.TRAIN_REPLAY:
                return self._train_step_body(sess, train_op, sess.buf(self._tag + "/train/losses", (5,))).clone()
            return self._replayer.step(sess, torch.cuda.current_stream(sess.device), self._tag + "/train", self._replay_key(train_op),
                                       self._train_scope_key, body=lambda out: self._train_step_body(sess, train_op, out),
                                       ready=lambda: bool(train_op.params) and train_op._sgd_table is not None,
                                       snapshot=self._step_views, restore=self._replayed_step,
                                       now=dict(seed=self._sample_seed, gt=int(self._gt_boxes.shape[0])), hip=cfg.HIP, cap=self.REPLAY_CAP)

    def _train_scope(self, sess, blobs):
        """A roidb's images differ in size from step to step (lib/roi_data_layer/layer.py:80-93); the step's activations, gradients, arena
        results and scratch are static per image SHAPE (a recorded step addresses them), so they live in the shape's buffer scope and at
        most cfg.HIP.TRAIN_CACHE_SHAPES shapes are kept -- the least recently used shape's buffers and recordings are dropped together."""
        if "data" in blobs:
            d = blobs["data"]
            shape = (int(d.shape[0]), int(d.shape[1]), int(d.shape[2]), 4)
        else:                                                # raw-image blob: the staged shape is the prep kernel's output shape
            _, OH, OW = self._train_prep_shape(blobs)
            shape = (1, OH, OW, 4)
        self._train_scope_key = ("train_shape", self._tag, shape)
        return sess.shape_scope(self._train_scope_key, group=("train", self._tag), cap=int(cfg.HIP.TRAIN_CACHE_SHAPES))

    def _train_step_body(self, sess, train_op, out):
        """forward + losses + reverse sweep + solver, enqueued eagerly; the five losses into the static tensor `out`"""
        losses = self._train_forward_staged(sess)
        if not train_op.params:
            with ops.unscoped():                                                  # solver state is per session, not per image shape
                train_op.build()
                if train_op.pending_slots is not None:          # resumed run: momentum before the first update
                    train_op.import_slots(train_op.pending_slots)
                    train_op.pending_slots = None
        train_op.backward(self._loss_seeds, fuse_solver=True)
        reg = train_op.regularization_value()
        parts = [losses[k].view(1) for k in ("rpn_cross_entropy", "rpn_loss_box", "cross_entropy", "loss_box")]

        def assemble():
            torch.cat(parts + [reg + parts[0] + parts[1] + parts[2] + parts[3]], out=out)
        ops.host_op(assemble)
        train_op.apply(train_op.lr, train_op.world_size, train_op.all_reduce)
        self._sample_seed += 2
        return out

    REPLAY_CAP = 16             # recorded steps kept per session (one per image shape; least recently used goes first)

    def _replay_key(self, train_op):
        """Everything a recorded step depends on besides the image's values (formed after configure_train_op)."""
        hip = tuple((k, tuple(v) if isinstance(v, (list, tuple)) else v) for k, v in sorted(cfg.HIP.items()))
        t = cfg.TRAIN
        return ("train_replay", self._tag, tuple(self._image.shape), self._im_info, int(self._gt_boxes.data_ptr()), float(train_op.lr),
                id(train_op), train_op.replay_signature(), hip, self._num_classes, self._anchor_scales, self._anchor_ratios, bool(cfg.RESNET.MAX_POOL),
                bool(cfg.USE_GPU_NMS), bool(cfg.USE_E2E_TF), cfg.POOLING_SIZE, cfg.POOLING_MODE,
                (t.RPN_PRE_NMS_TOP_N, t.RPN_POST_NMS_TOP_N, t.RPN_NMS_THRESH, t.BATCH_SIZE, t.FG_FRACTION, t.FG_THRESH, t.BG_THRESH_HI, t.BG_THRESH_LO,
                 t.RPN_BATCHSIZE, t.RPN_FG_FRACTION, t.RPN_POSITIVE_OVERLAP, t.RPN_NEGATIVE_OVERLAP, bool(t.RPN_CLOBBER_POSITIVES),
                 float(t.RPN_POSITIVE_WEIGHT), tuple(t.RPN_BBOX_INSIDE_WEIGHTS), tuple(t.BBOX_INSIDE_WEIGHTS), bool(t.USE_GT),
                 tuple(float(v) for v in t.BBOX_NORMALIZE_MEANS), tuple(float(v) for v in t.BBOX_NORMALIZE_STDS)))

    def _step_views(self):
        """what a recorded step left on the network for its readers (replay.StepReplayer: snapshot) ..."""
        return (dict(self._predictions), dict(self._losses), dict(self._proposal_targets), dict(self._anchor_targets)), list(self._act_summaries)

    def _replayed_step(self, views, acts):
        """... and what a replayed step owes them: the same views, and the seed advance of _train_step_body"""
        self._predictions, self._losses, self._proposal_targets, self._anchor_targets = views
        self._act_summaries = acts
        self._sample_seed += 2

    @staticmethod
    def configure_train_op(train_op):
        """cfg.HIP -> the solver handle's switches for the reverse sweep (frcnn_hip/train.py)."""
        train_op.winograd = ((int(cfg.HIP.WINOGRAD_M), int(cfg.HIP.WINOGRAD_MIN_CIN), bool(cfg.HIP.WINOGRAD_7X7))
                             if (cfg.HIP.WINOGRAD and cfg.HIP.WINOGRAD_TRAIN and cfg.HIP.WINOGRAD_DGRAD) else None)
        train_op.h2_train = forward.h2_min_tiles("TRAIN", cfg.HIP) if (cfg.HIP.MFMA_H2 and cfg.HIP.H2_TRAIN) else None
        train_op.wgrad_stream = int(cfg.HIP.WGRAD_STREAM)
        train_op.wgrad_tn = bool(cfg.HIP.WGRAD_TN)
        train_op.prep_stream = bool(cfg.HIP.PREP_STREAM)
        train_op.wgrad_h2 = bool(cfg.HIP.MFMA_H2 and cfg.HIP.H2_TRAIN and cfg.HIP.WGRAD_H2)

    def train_step_no_return(self, sess, blobs, train_op):
        self.train_step(sess, blobs, train_op)

    # ------------------------------------------------------------------ TensorBoard summaries (network.py:47-66,437-450,481-511)
    LOSS_TAGS = ("rpn_cross_entropy", "rpn_loss_box", "cross_entropy", "loss_box", "total_loss")     # self._losses keys = the scalar tags (:310-319,440-441)

    def _summary_tensors(self, train_op):
        """[(tag, kind, device tensor)] of one summary step, over the step's RETAINED device tensors: kind 'act' = the activation list
        (histogram + zero_fraction, :57-60), 'score' = every prediction and target (:62-63,181,206,260), 'train' = every trainable
        variable (:65-66; the solver's master copies, i.e. the values AFTER the step's update -- the reference leaves the order of the
        summary and the update inside its one sess.run undefined).  The middle of a tag is the tensor's name here (there are no TF op
        names): ACT/<scope>/<head|rpn_conv/3x3>/activations, SCORE/<key>/scores, TRAIN/<variable name>."""
        out = []
        for name, t in zip(("head", "rpn_conv/3x3"), self._act_summaries):
            out.append(("ACT/%s/%s" % (self._scope, name), "act", t))
        score = collections.OrderedDict()
        for d in (self._anchor_targets, self._proposal_targets, self._predictions):      # (later dicts win a shared key like the reference's update())
            for k, t in d.items():
                if torch.is_tensor(t) and t.dtype == torch.float32:                    # (`counts` of the sampler is bookkeeping, not a target)
                    score[k] = t
        for k, t in score.items():
            out.append(("SCORE/%s/scores" % k, "score", t))
        if train_op is not None:
            for p in train_op.params.values():
                if p.dw:
                    out.append(("TRAIN/%s/depthwise_weights" % p.scope, "train", p.w))
                    continue
                out.append(("TRAIN/%s/weights" % p.scope, "train", p.w))
                if p.bias is not None:
                    out.append(("TRAIN/%s/biases" % p.scope, "train", p.bias))
        return out

    def _gt_image_summary(self):
        """network.py:40-55: the staged image + PIXEL_MEANS, BGR -> RGB, back at its original size, gt boxes drawn (host, PIL)."""
        from frcnn_hip import summary
        from utils.visualization import draw_bounding_boxes, resize_bilinear
        bgr = self._image[0, :, :, :3].cpu().numpy().astype(np.float64) + np.asarray(cfg.PIXEL_MEANS, dtype=np.float64).reshape(1, 1, 3)
        h, w, scale = self._im_info
        rgb = resize_bilinear(bgr[:, :, ::-1], int(h / scale), int(w / scale))
        pic = draw_bounding_boxes(rgb, self._gt_boxes.cpu().numpy(), self._im_info)
        return summary.image("GROUND_TRUTH", pic[0].astype(np.uint8))

    def _build_summary(self, train_op, loss_values, full):
        """The serialised Summary of the step whose tensors this network holds right now: launches on the current stream (after the step),
        one read-back.  full = False: the validation summary (image + losses, :437-441,450)."""
        from frcnn_hip import summary
        parts = [self._gt_image_summary()]
        parts += [summary.scalar(k, v) for k, v in zip(self.LOSS_TAGS, loss_values)]
        if full:
            items = self._summary_tensors(train_op)
            stats = ops.summary_stats([t if t.is_contiguous() else t.contiguous() for _, _, t in items])
            limits = ops.summary_limits()
            for (tag, kind, _), st in zip(items, stats):
                if kind == "act":
                    parts.append(summary.histogram(tag + "/activations", st, limits))
                    parts.append(summary.scalar(tag + "/zero_fraction", summary.zero_fraction(st)))
                else:
                    parts.append(summary.histogram(tag, st, limits))
        return b"".join(parts)

    def train_step_with_summary(self, sess, blobs, train_op):
        """network.py:500-511: train_step plus the serialised Summary (bytes for summary.FileWriter.add_summary).  The step itself is
        train_step_async -- replayed when its shape has a recording, recorded or eager otherwise, exactly as without a summary -- and the
        statistics kernel runs after it on the same stream over the tensors the step left behind; nothing it writes is read by a later
        step."""
        self._train_state = train_op
        losses = self.train_step_async(sess, blobs, train_op)
        vals = tuple(float(v) for v in losses.cpu().tolist())
        return vals + (self._build_summary(train_op, vals, True),)

    def get_summary(self, sess, blobs, train_op=None):
        """network.py:481-486: the validation summary -- TRAIN-mode forward + losses on `blobs`, eagerly, NO update: weights, momentum and
        the gradient buffer are not touched, and the sampling seed is restored, so the training run continues bit for bit as if this had
        not run (the forward pass overwrites only activations and targets, which every step rewrites before reading).  total_loss carries
        the regulariser's value when a solver handle is known (the argument, or the last train_step_with_summary's)."""
        assert self._mode == "TRAIN"
        train_op = self._train_state if train_op is None else train_op
        seed = self._sample_seed
        with self._train_scope(sess, blobs):
            try:
                self._stage_train_inputs(sess, blobs)
                losses = self._train_forward_staged(sess)
            finally:
                self._sample_seed = seed
            parts = [losses[k].view(1) for k in ("rpn_cross_entropy", "rpn_loss_box", "cross_entropy", "loss_box")]
            total = parts[0] + parts[1] + parts[2] + parts[3]
            if train_op is not None and train_op.params:
                reg = torch.zeros((1,), dtype=torch.float32, device=sess.device)
                train_op.regularization_loss(reg)
                total = total + reg
            vals = tuple(float(v) for v in torch.cat(parts + [total]).cpu().tolist())
            return self._build_summary(None, vals, False)

    def detect_device(self, sess, image_d, im_info, im_shape, max_per_image=100, thresh=0.0, out=None, count=None):
        """image(s) already in HBM -> final detections in HBM: forward + the whole of lib/model/test.py:95-102,
        162-180 on device.  One image: returns (dets [max_out,6], count [1]).  A batch [B,H,W,4] of same-size images:
        dets [B,max_out,6], count [B] (the dense layers run once for the batch, the per-image stages once per image)."""
        vote = float(cfg.HIP.BBOX_VOTE_THRESH) if cfg.HIP.BBOX_VOTE else 0.0    # (read per call, like SOFT_NMS: detect_post runs outside the graph)
        if cfg.HIP.TEST_FLIP:
            return self._detect_device_flip(sess, image_d, im_info, im_shape, max_per_image, thresh, out, count, vote)
        p = self.forward_device(sess, image_d, im_info)
        ops.ws_scope = self._tag
        B = image_d.shape[0]
        R, C = self._rois_per_image, self._num_classes
        # rows of the output: test.py:176-180 keeps every detection that TIES the max_per_image-th score, so the list can exceed
        # max_per_image; the default buffer holds 28 extra rows (a 128-row record), `count` reports the true number
        max_out = None if out is None else out.shape[-2]
        with self.shape_scope(sess, image_d.shape, im_info):         # (the post-processing scratch follows the proposal count of the shape's graph)
            if B > 1:
                max_out = (max_per_image + 28) if out is None else max_out
                out = sess.buf(self._tag + "/dets", (B, max_out, 6)) if out is None else out
                count = sess.buf(self._tag + "/det_count", (B,), torch.int32) if count is None else count
            return sess.mark("op:detect_post", 0, lambda: ops.detect_post(
                p["cls_prob"], p["bbox_pred"] if cfg.TEST.BBOX_REG else None, p["rois"], self._num_rois, float(im_info[2]), int(im_shape[0]), int(im_shape[1]),
                float(cfg.TEST.NMS), float(thresh), int(max_per_image), max_out=max_out, out=out, count=count, batch=B,
                rule=self._nms_rule(), soft=int(cfg.HIP.SOFT_NMS), sigma=float(cfg.HIP.SOFT_NMS_SIGMA),
                min_score=float(cfg.HIP.SOFT_NMS_MIN_SCORE), vote=vote), nbytes=B * R * 20 * C)

    def _detect_device_flip(self, sess, image_d, im_info, im_shape, max_per_image, thresh, out, count, vote):
        """detect_device under cfg.HIP.TEST_FLIP: the B staged images and their mirrors as ONE forward pass of 2B views (slot 2b as seen,
        2b+1 mirrored: ops.mirror_views, an exact permutation of the prepared image) -- a shape of its own, hence its own captured graph
        and buffer scope --, the two views' rows merged per image (ops.merge_flip_views: the mirror's rois turned back about im_info[1], its
        dx negated) and the usual post-processing on B images of 2R rows.  The same records for the callers: [B,max_out,6] / [B]."""
        bad = self._flip_refusals()
        if bad:
            raise NotImplementedError("unsupported configuration for the HIP path: " + "; ".join(bad))
        B = int(image_d.shape[0])
        shape2 = (2 * B,) + tuple(int(v) for v in image_d.shape[1:])
        with self.shape_scope(sess, shape2, im_info):
            views = sess.buf(self._tag + "/flip_views", shape2)
        ops.ws_scope = self._tag
        ops.mirror_views(image_d, out=views)
        p = self.forward_device(sess, views, im_info)
        ops.ws_scope = self._tag
        R, C = self._rois_per_image, self._num_classes
        assert self._num_rois is not None and 2 * R <= self.FLIP_MAX_ROWS
        reg = bool(cfg.TEST.BBOX_REG)
        max_out = None if out is None else out.shape[-2]
        with self.shape_scope(sess, shape2, im_info):
            merged = (sess.buf(self._tag + "/flip_cls_prob", (B * 2 * R, C)), sess.buf(self._tag + "/flip_bbox_pred", (B * 2 * R, 4 * C)) if reg else None,
                      sess.buf(self._tag + "/flip_rois", (B * 2 * R, 5)), sess.buf(self._tag + "/flip_num_rois", (B,), torch.int32))
            m_prob, m_pred, m_rois, m_num = sess.mark("op:merge_flip_views", 0, lambda: ops.merge_flip_views(
                p["cls_prob"], p["bbox_pred"] if reg else None, p["rois"], self._num_rois, float(im_info[1]), batch=B, out=merged),
                nbytes=2 * B * R * (5 * C + 5) * 8)
            if B > 1:
                max_out = (max_per_image + 28) if out is None else max_out
                out = sess.buf(self._tag + "/dets", (B, max_out, 6)) if out is None else out
                count = sess.buf(self._tag + "/det_count", (B,), torch.int32) if count is None else count
            return sess.mark("op:detect_post", 0, lambda: ops.detect_post(
                m_prob, m_pred, m_rois, m_num, float(im_info[2]), int(im_shape[0]), int(im_shape[1]),
                float(cfg.TEST.NMS), float(thresh), int(max_per_image), max_out=max_out, out=out, count=count, batch=B,
                rule=self._nms_rule(), soft=int(cfg.HIP.SOFT_NMS), sigma=float(cfg.HIP.SOFT_NMS_SIGMA),
                min_score=float(cfg.HIP.SOFT_NMS_MIN_SCORE), vote=vote), nbytes=B * 2 * R * 20 * C)
