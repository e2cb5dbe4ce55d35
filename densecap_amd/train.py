"""train.lua's loop on the MI355X path (-finetune_cnn_after N trains conv3_1 .. conv5_3 too, from iteration N on; default -1):

    python -m densecap_amd.train -checkpoint_start_from model.t7 -data_h5 VG.h5 -data_json VG.json -image_dir imgs \\
        -max_iters 1000 -checkpoint_path out.t7

Every iteration is one DenseCapModel.train_step on the next image of the train split (walked in index order, again from the
start when it ends): forward_backward, the L2 weight decay and Adam on the device (docs/SEMANTICS.md, "Training step").  The flags
are train.lua's (train_opts.lua) with its defaults, as far as this path reads them; the dataset flags are evaluate_model's.
Prints `iter %d:` lines with the six losses every -losses_log_every iterations; every -save_checkpoint_every iterations and at the
end writes -checkpoint_path (a .t7 that run_model and evaluate_model load) and, beside it, a .json with the loss history.

-drop_prob P is the Dropout of recog_base (after fc6 and after fc7; docs/SEMANTICS.md, "Dropout"), its masks drawn on the device
from the iteration's seed.  The default is 0.0, no Dropout: -drop_prob 0.5 is the reference's training (train_opts.lua:60).

-grad_clip X clips every step's gradient by its global L2 norm (docs/SEMANTICS.md, "Gradient clipping"; inf: log only); the
`iter %d:` lines and the loss history then carry grad_norm.  -save_optim_state 1 writes Adam's moments and step counts beside
every checkpoint (<checkpoint_path stem>.optim.npz); -resume_optim_state FILE loads such a file after train_begin and continues
at its iteration t + 1 with that iteration's image and seed, so that the run is the uninterrupted one -- start it from the
checkpoint written with the file.

Not here: the validation mAP inside the loop (run evaluate_model on the saved checkpoint).  There is no CPU mode: without a
HIP device the tool stops with the library's error.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np


def build_parser():
    p = argparse.ArgumentParser(prefix_chars="-", description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    a = p.add_argument
    # ---- the data: train_opts.lua:46-48 and evaluate_model's -image_dir / -image_size ----
    a("-data_h5", default="data/VG-regions.h5")
    a("-data_json", default="data/VG-regions-dicts.json")
    a("-image_dir", default="", help="where the image files are (the HDF5 file's /images is never read)")
    a("-image_size", type=int, default=720)
    a("-debug_max_train_images", type=int, default=-1, help="use only this many images of the train split; -1 = all")
    # ---- the optimiser: train_opts.lua:41,56-59 ----
    a("-learning_rate", type=float, default=1e-5)
    a("-optim_beta1", type=float, default=0.9)
    a("-optim_beta2", type=float, default=0.999)
    a("-optim_epsilon", type=float, default=1e-8)
    a("-weight_decay", type=float, default=1e-6)
    a("-box_reg_decay", type=float, default=5e-5)
    # ---- the sampler and the loss weights: train_opts.lua:18-40 ----
    a("-sampler_batch_size", type=int, default=256)
    a("-sampler_high_thresh", type=float, default=0.7)
    a("-sampler_low_thresh", type=float, default=0.3)
    a("-train_remove_outbounds_boxes", type=int, default=1, choices=[0, 1])
    a("-mid_box_reg_weight", type=float, default=0.05)
    a("-mid_objectness_weight", type=float, default=0.1)
    a("-end_box_reg_weight", type=float, default=0.1)
    a("-end_objectness_weight", type=float, default=0.1)
    a("-captioning_weight", type=float, default=1.0)
    a("-drop_prob", type=float, default=0.0,
      help="Dropout after fc6 and fc7, a number in [0, 1); 0 (default) = none, 0.5 = the reference's training (train_opts.lua:60)")
    # ---- the loop: train_opts.lua:61-92 ----
    a("-max_iters", type=int, default=-1, help="iterations to run; -1 = until interrupted")
    a("-finetune_cnn_after", type=int, default=-1,
      help="train conv3_1 .. conv5_3 too from this (0-based) iteration on; -1 = never (train_opts.lua:64)")
    a("-checkpoint_start_from", default="", help="the .t7 to start from")
    a("-checkpoint_path", default="checkpoint.t7")
    a("-save_checkpoint_every", type=int, default=10000)
    a("-losses_log_every", type=int, default=10)
    a("-seed", type=int, default=123, help="iteration i samples its boxes with seed + i")
    a("-gpu", type=int, default=0)
    # ---- not reference flags ----
    a("-synthetic_weights", type=int, default=0, help="1: random weights in checkpoint shapes instead of -checkpoint_start_from")
    a("-grad_clip", type=float, default=0.0,
      help="clip the gradient by its global L2 norm to this value; 0 (default) = off, inf = compute and log the norm only")
    a("-save_optim_state", type=int, default=0, choices=[0, 1],
      help="1: write Adam's moments and step counts to <checkpoint_path stem>.optim.npz beside every checkpoint "
           "(about 1.1 GB at the real model)")
    a("-resume_optim_state", default="", help="an .optim.npz to load after train_begin; the loop continues at its iteration t + 1")
    return p


def loss_options(opt, it):
    """evaluate_model.loss_options on train.lua's flags; the sampler's draws of iteration `it` come from -seed + it."""
    from .evaluate_model import loss_options as base
    opt.loss_seed = (int(opt.seed) + int(it)) & (2 ** 64 - 1)
    return base(opt)


def save(model, opt, history, it):
    model.save_checkpoint(opt.checkpoint_path)
    with open(os.path.splitext(opt.checkpoint_path)[0] + ".json", "w") as f:
        json.dump({"iter": it, "loss_history": history, "opt": {k: v for k, v in vars(opt).items()}}, f)
    print("wrote %s after %d iterations" % (opt.checkpoint_path, it))
    if opt.save_optim_state:
        path = optim_state_path(opt.checkpoint_path)
        model.save_train_state(path)
        print("wrote %s" % path)


def optim_state_path(checkpoint_path):
    return os.path.splitext(checkpoint_path)[0] + ".optim.npz"


def main(argv=None):
    opt = build_parser().parse_args(argv)
    from . import DenseCapModel, ops
    from .evaluate_model import read_dataset
    from .run_model import load_image_caffe, load_weights
    if not opt.synthetic_weights and not opt.checkpoint_start_from:
        raise SystemExit("-checkpoint_start_from FILE.t7 (or -synthetic_weights 1) must be given: this path trains "
                         "an existing model")
    opt.checkpoint = opt.checkpoint_start_from
    weights = load_weights(opt)
    model = DenseCapModel(weights, device=opt.gpu)                      # no HIP device: DenseCapError, no CPU fallback
    model.set_dropout(opt.drop_prob)
    data = read_dataset(opt.data_h5, opt.data_json, "train", opt.debug_max_train_images)
    data = [d for d in data if len(d[1]) > 0]
    if not data:
        raise SystemExit("the train split of %s holds no image with ground truth" % opt.data_h5)
    model.train_begin(learning_rate=opt.learning_rate, beta1=opt.optim_beta1, beta2=opt.optim_beta2, epsilon=opt.optim_epsilon,
                      weight_decay=opt.weight_decay)
    model.train_set_grad_clip(opt.grad_clip)
    history, it = {}, 0
    if opt.resume_optim_state:
        it, cnn_t = model.load_train_state(opt.resume_optim_state)      # iteration `it` was the last one of the saved run
        print("resumed Adam's state of %s: t = %d, cnn_t = %d" % (opt.resume_optim_state, it, cnn_t))
    try:
        while opt.max_iters < 0 or it < opt.max_iters:
            name, boxes, labels = data[it % len(data)]
            img = load_image_caffe(os.path.join(opt.image_dir, name), opt.image_size)[0][0]
            it += 1
            model.train_set_cnn(ops.finetune_cnn_mode(opt.finetune_cnn_after, it))
            lo = model.train_step(img, boxes, np.asarray(labels)[:, :model.seq_length], box_reg_decay=opt.box_reg_decay,
                                  **loss_options(opt, it))
            if it % max(1, opt.losses_log_every) == 0 or it == opt.max_iters:
                keys = ops.LOSS_KEYS + (("grad_norm",) if "grad_norm" in lo else ())
                history[str(it)] = {k: lo[k] for k in keys}
                print("iter %d: %s" % (it, ", ".join("%s: %.6f" % (k, lo[k]) for k in keys)))
            if it % max(1, opt.save_checkpoint_every) == 0 and it != opt.max_iters:
                save(model, opt, history, it)
    except KeyboardInterrupt:
        print("interrupted after %d iterations" % it)
    save(model, opt, history, it)
    model.train_end()
    return 0


if __name__ == "__main__":
    sys.exit(main())
