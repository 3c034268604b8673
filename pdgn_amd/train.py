"""`python -m pdgn_amd.train`: the reference's command line (main.py:15-41, same flag names and defaults) in front of
PDGNTrainer.fit (--phase train) and evaluation.generate_and_evaluate (--phase test).

train: ShapeNetCore(choice, 'train', 'shape_unit') -> stack(device) -> data.BatchFeeder -> fit; checkpoints and the log go
where the reference puts them (<checkpoint_dir>/<model_dir>/<network>/<epoch>_<category>_{G,D}.pth,
<checkpoint_dir>/<model_dir>/<log_info>).  test: load --pretrain_model_G/_D from that directory, generate as many clouds as
the test split has, write nonormal_out.npy / out.npy and log.txt under <save_dir>/GEN_Ours_<choice>_<time>/
(models/PDGNet_v2.py:271-326).  --report_every N (train): every N epochs a preview sheet and a row of held-out metrics on the val
split, under <checkpoint_dir>/<model_dir>/report (pdgn_amd/report.py).  --ema_decay D (train): keep an exponential moving average of
the generator's parameters (decay D, e.g. 0.999), write it as <epoch>_<category>_G_ema.pth beside every checkpoint pair and report
on it; --phase test --pretrain_model_G <epoch>_<category>_G_ema.pth evaluates it.  --lr_g / --lr_d (train): base rates of the
generator / the four discriminators instead of --learning_rate; --lr_schedule constant|linear|cosine|step with --lr_warmup_iters,
--lr_final_factor, --lr_step_epochs, --lr_gamma: the rate as a function of Adam's step count over max_epoch x batches-per-epoch
updates, evaluated on the device (pdgn_amd/schedule.py); lr.csv beside the log.  --d_augment P (train): every cloud a discriminator
sees goes through a random similarity transform drawn on the device, each component enabled per sample with probability P
(pdgn_amd/augment.py); --aug_rotate DEG (default 180, about the y axis), --aug_scale S (1.25: log-uniform in [1/S, S]), --aug_flip [0|1]
(1: mirror x), --aug_translate T (0.1), --aug_jitter SIGMA (0) change its ranges and need --d_augment.
--d_augment_target R (train, needs --d_augment): P is only the initial value; the device steers it from the discriminators' scores of the real
batch towards r = R (ADA), with --ada_interval K (4), --ada_span CLOUDS (500000), --ada_p_min / --ada_p_max (0 / 0.8);
aug.csv beside the log, <epoch>_<category>_aug.pth beside every checkpoint pair.  r counts the scores above the objective's decision boundary
against those below it: 1/2 under --gan_loss lsgan, 0 otherwise.  --gan_loss lsgan|hinge|logistic (train): the adversarial objective of all twelve terms
of an iteration -- lsgan (default) is the reference's least squares; hinge and logistic (non-saturating) read the discriminators' outputs as logits
(losses.adversarial); no launch is added, checkpoints are unchanged.  --data_root: the HDF5 file (needs h5py), an .npz whose keys are "<synsetid>/<split>",
or a directory in the layout of ShapeNetCore.v2.PC15k (<synsetid>/<split>/*.npy, each (M,3)).  Clouds stored with M > --num_point points (PC15k: 15 000)
are trained on a fresh draw of --num_point distinct points per cloud and visit, made inside the feed launch (data.BatchFeeder, pdgn_feed_batch_resample),
from the leading --resample_pool P points (default: all M); --phase test and the reports take the LAST --num_point points of every stored cloud as
their reference clouds (disjoint from the pool whenever P <= M - num_point).  --subsample fps (train): the three coarse real resolutions are
nested farthest-point subsets of the finest cloud of the same row instead of three independent with-replacement draws (data.BatchFeeder, csrc/fps.hip;
--num_point at most 8192); --subsample random is the default and the reference's.  --data_root may also hold triangle MESHES -- a directory <synsetid>/<split>/*.obj, or the
.npz that `python -m pdgn_amd.meshes pack DIR OUT.npz` makes of one: the train split then stays on the device as meshes, normalised over
its surface, and every visit of a shape is a fresh i.i.d. sample of its surface (data.MeshFeeder, pdgn_feed_batch_mesh);
--phase test and the reports take draw 0 of --num_point surface points of every raw test / val mesh as their reference clouds;
--resample_pool does not apply.  --mesh_visible on | compute (meshes only): the faces that none of --mesh_views orthographic views can see
get weight zero, for the train split and the reference draws alike (pdgn_mesh_visibility).
--data_root may also hold RAGGED clouds, shapes that store different numbers of points -- the .npz that `python -m pdgn_amd.clouds pack DIR OUT.npz`
makes of a directory <synsetid>/<split>/* of .npy / .pts / .xyz / .txt clouds (it identifies itself), or such a directory under --ragged: the train split
stays on the device as one point array and an offset table, and every visit of a shape is a fresh draw of --num_point of its points, or all of them with
evenly spread duplicates where it stores fewer (data.RaggedFeeder, pdgn_feed_batch_ragged); --min_points K drops shorter shapes at load;
--phase test and the reports take draw 0 of --num_point points of every raw test / val shape; --resample_pool and --mesh_visible do not apply.
--repulsion W (train): the generator's loss gains W times a repulsion term on every generated cloud of --repulsion_levels (default 1,2,3,4), which
is zero when no two points of a cloud are closer than the level's radius (losses.repulsion); --repulsion_radius H is the radius at
--num_point points -- without it the radius is calibrated once before training, --repulsion_radius_factor (1) times the mean nearest-neighbour distance
of up to 64 clouds the feeder itself produces, and printed; repulsion.csv beside the log.  --flatness W (train): the generator's loss gains W times a flatness term on every
generated cloud of --flatness_levels (default 1,2,3,4): the batch mean of the surface variation l0 / (l0 + l1 + l2 + eps) of every point's --flatness_k (16)
nearest neighbours, zero on a flat neighbourhood (losses.flatness); --flatness_eps E is the floor under the trace at --num_point
points -- without it the floor is calibrated once before training, --flatness_eps_factor (1e-2) times the mean trace of the k-neighbourhoods of up to 64
clouds the feeder itself produces, and printed; flatness.csv beside the log.  --report_spacing (needs --report_every): the reports also
append nearest-neighbour spacing statistics of the generated and the val clouds to report/spacing.csv.  --report_lit: the preview sheets are shaded by
surface normals estimated from each cloud's 16 nearest neighbours; --report_surface: the reports also append the surface
variation of the generated and the val clouds to report/surface.csv (both need --report_every).
--report_fidelity (needs --report_every and a mesh --data_root): the reports also append to report/fidelity.csv the distance of the generated
clouds' points to the surface of the nearest val shape, and of the val clouds to their own shapes (meshes.point_to_mesh).
--report_mesh [R] (needs --report_every): the preview sheets get one more column, the surface reconstructed from the finest generated clouds at grid
resolution R (default 64) drawn as flat-lit triangles, and with --report_fidelity another one, the val meshes themselves.
Under torch.distributed.run every rank trains on its own slice of each global batch."""
import argparse
import os
import random
import sys
import time

import numpy as np
import torch


def build_parser():
    p = argparse.ArgumentParser(prog="python -m pdgn_amd.train", description="PDGN training / test phase on an AMD Instinct GPU")
    p.add_argument("--phase", type=str, default="train", help="train or test")
    p.add_argument("--workers", type=int, default=4, help="accepted and ignored: the data set lives on the device")
    p.add_argument("--gpu", type=int, default=0, help="accepted and ignored, as in the reference")
    p.add_argument("--batch_size", type=int, default=50, help="batch size (per rank)")
    p.add_argument("--num_point", type=int, default=2048, help="points of the finest resolution")
    p.add_argument("--num_k", type=int, default=20, help="neighbours of the knn graph")
    p.add_argument("--learning_rate", type=float, default=0.0001)
    p.add_argument("--max_epoch", type=int, default=300)
    p.add_argument("--noise_dim", type=int, default=128)
    p.add_argument("--optimizer", default="adam", help="accepted and ignored, as in the reference")
    p.add_argument("--debug", type=bool, default=True, help="accepted and ignored, as in the reference")
    p.add_argument("--data_root", default="/opt/data/private/shapenet/shapenet.hdf5", help="shapenet.hdf5, an .npz with '<synsetid>/<split>' keys, or a "
                   "directory <synsetid>/<split>/*.npy (ShapeNetCore.v2.PC15k); meshes: a directory <synsetid>/<split>/*.obj or the .npz "
                   "`python -m pdgn_amd.meshes pack` makes of one; ragged clouds: the .npz `python -m pdgn_amd.clouds pack` makes of a directory "
                   "<synsetid>/<split>/* of .npy / .pts / .xyz / .txt clouds, or that directory under --ragged")
    p.add_argument("--log_info", default="log_info.txt")
    p.add_argument("--model_dir", help="model dir (required)")
    p.add_argument("--checkpoint_dir", default="checkpoint")
    p.add_argument("--snapshot", type=int, default=20, help="epochs between checkpoints")
    p.add_argument("--choice", default=None, help="category")
    p.add_argument("--network", default="PDGNet_v2", help="names the checkpoint sub-directory; PDGNet_v2 is the one network")
    p.add_argument("--savename", default=None, help="accepted and ignored, as in the reference")
    p.add_argument("--pretrain_model_G", default=None)
    p.add_argument("--pretrain_model_D", default=None)
    p.add_argument("--softmax", default="True", help="softmax for the bilateral interpolation")
    p.add_argument("--dataset", default="shapenet15k")
    p.add_argument("--normalize", type=lambda s: None if s == "None" else s, default="shape_bbox", choices=[None, "shape_unit", "shape_bbox"])
    p.add_argument("--seed", type=int, default=9999)
    p.add_argument("--save_dir", type=str, default="./results")
    p.add_argument("--device", type=str, default="cuda")
    p.add_argument("--report_every", type=int, default=0, help="epochs between snapshot reports (pdgn_amd.report: a preview sheet and "
                   "a row of held-out metrics on the val split, under <checkpoint_dir>/<model_dir>/report); 0: none")
    p.add_argument("--report_rows", type=int, default=8, help="samples per preview sheet")
    p.add_argument("--report_full", action="store_true", help="reports run the full evaluation (EMD included) instead of the CD-only one")
    p.add_argument("--emd", choices=["approx", "auction"], default=argparse.SUPPRESS, help="the EMD of --phase test and of --report_full: approx, the "
                   "reference's approximate matching (what published numbers use), or auction, the exact assignment of equal-sized clouds "
                   "(about 29 x the approximate EMD's time, 0.56 ms per pair of 2048-point clouds; log.txt / metrics.csv gain emd-capped, the pairs that did not end at an optimum)")
    p.add_argument("--ema_decay", type=float, default=argparse.SUPPRESS, help="decay of the averaged generator (an exponential moving average of the "
                   "generator's parameters, e.g. 0.999: written as <epoch>_<category>_G_ema.pth, shown by the reports); 0: none")
    p.add_argument("--grad_guard", action="store_true", default=argparse.SUPPRESS, help="gradient guard: each network's global gradient "
                   "norm on the device before its Adam launch, an update with a non-finite gradient is skipped, grad_norms.csv beside the log")
    p.add_argument("--clip_grad_norm", type=float, default=argparse.SUPPRESS, help="clip each network's global gradient norm to this "
                   "value (implies --grad_guard)")
    p.add_argument("--guard_max_skips", type=int, default=argparse.SUPPRESS, help="stop, with a checkpoint, after this many consecutive "
                   "skipped updates of a network (default 50)")
    p.add_argument("--lr_g", type=float, default=argparse.SUPPRESS, help="base learning rate of the generator (default: --learning_rate)")
    p.add_argument("--lr_d", type=float, default=argparse.SUPPRESS, help="base learning rate of the four discriminators (default: --learning_rate)")
    p.add_argument("--lr_schedule", choices=["constant", "linear", "cosine", "step"], default=argparse.SUPPRESS,
                   help="learning-rate schedule over max_epoch x batches-per-epoch updates, evaluated on the device from Adam's step count")
    p.add_argument("--lr_warmup_iters", type=int, default=argparse.SUPPRESS, help="updates of linear warm-up from 0 (default 0)")
    p.add_argument("--lr_final_factor", type=float, default=argparse.SUPPRESS, help="linear / cosine: the factor reached at the last update (default 0)")
    p.add_argument("--lr_step_epochs", type=int, default=argparse.SUPPRESS, help="step: epochs between drops")
    p.add_argument("--lr_gamma", type=float, default=argparse.SUPPRESS, help="step: the factor of a drop (default 0.1)")
    p.add_argument("--d_augment", type=float, default=argparse.SUPPRESS, metavar="P", help="discriminator augmentation: a random flip / rotation / "
                   "scale / translation (/ jitter) of every cloud in front of every discriminator call, each enabled per sample with probability P")
    p.add_argument("--aug_rotate", type=float, default=argparse.SUPPRESS, metavar="DEG", help="largest rotation about the up (y) axis, degrees (default 180)")
    p.add_argument("--aug_scale", type=float, default=argparse.SUPPRESS, metavar="S", help="isotropic scale, log-uniform in [1/S, S] (default 1.25)")
    p.add_argument("--aug_flip", type=int, choices=[0, 1], nargs="?", const=1, default=argparse.SUPPRESS, help="mirror the x coordinate (default 1; 0: off)")
    p.add_argument("--aug_translate", type=float, default=argparse.SUPPRESS, metavar="T", help="translation, uniform in [-T, T] per coordinate (default 0.1)")
    p.add_argument("--aug_jitter", type=float, default=argparse.SUPPRESS, metavar="SIGMA", help="per-point Gaussian jitter (default 0: none)")
    p.add_argument("--d_augment_target", type=float, default=argparse.SUPPRESS, metavar="R", help="adaptive discriminator augmentation (ADA, Karras et "
                   "al. 2020): --d_augment becomes the INITIAL p, which the device then steers so that r = (scores above the objective's decision "
                   "boundary - scores below it) / scores, measured on the discriminators' outputs for the real batch, approaches R (the paper: "
                   "0.6); the boundary is 1/2 under --gan_loss lsgan and 0 otherwise; aug.csv beside the log")
    p.add_argument("--ada_interval", type=int, default=argparse.SUPPRESS, metavar="K", help="iterations per adjustment of p (default 4)")
    p.add_argument("--ada_span", type=int, default=argparse.SUPPRESS, metavar="CLOUDS", help="real clouds over which p may travel from 0 to 1 (default "
                   "500000, the paper's: far too long for a category of a few dozen shapes -- give a few hundred epochs' worth of clouds there)")
    p.add_argument("--ada_p_min", type=float, default=argparse.SUPPRESS, help="lower end of p's range (default 0)")
    p.add_argument("--ada_p_max", type=float, default=argparse.SUPPRESS, help="upper end of p's range (default 0.8)")
    p.add_argument("--gan_loss", choices=["lsgan", "hinge", "logistic"], default=argparse.SUPPRESS, help="the adversarial objective: lsgan "
                   "(default: the reference's least squares against 1 / 0), hinge, or logistic (non-saturating); the latter two read the "
                   "discriminators' outputs as logits; no launch is added")
    p.add_argument("--repulsion", type=float, default=argparse.SUPPRESS, metavar="W", help="repulsion regulariser: the generator's loss gains W times the "
                   "sum over the levels of the batch mean of sum_{j != i} max(0, 1 - |x_i - x_j|^2 / h^2)^2 over every generated cloud "
                   "(losses.repulsion, DESIGN.md section 7p); repulsion.csv beside the log")
    p.add_argument("--repulsion_radius", type=float, default=argparse.SUPPRESS, metavar="H", help="--repulsion: the radius h at --num_point points (a coarser "
                   "level of N points gets h sqrt(num_point / N)); default: calibrated once before training, --repulsion_radius_factor times the mean "
                   "nearest-neighbour distance of up to 64 clouds the feeder produces")
    p.add_argument("--repulsion_radius_factor", type=float, default=argparse.SUPPRESS, metavar="K", help="--repulsion without --repulsion_radius: the "
                   "calibrated radius is K times the mean nearest-neighbour distance (default 1)")
    p.add_argument("--repulsion_levels", type=str, default=argparse.SUPPRESS, metavar="L,..", help="--repulsion: the levels that carry the term, 1 (the "
                   "coarsest) .. 4 (--num_point points), comma separated (default 1,2,3,4)")
    p.add_argument("--flatness", type=float, default=argparse.SUPPRESS, metavar="W", help="flatness regulariser: the generator's loss gains W times the "
                   "sum over the levels of the batch mean of the surface variation l0 / (l0 + l1 + l2 + eps) of every generated point's k-neighbourhood "
                   "(losses.flatness, DESIGN.md section 7x); flatness.csv beside the log")
    p.add_argument("--flatness_k", type=int, default=argparse.SUPPRESS, metavar="K", help="--flatness: the number of nearest neighbours, 1 .. 64 and at most "
                   "the coarsest named level's point count (default 16)")
    p.add_argument("--flatness_eps", type=float, default=argparse.SUPPRESS, metavar="E", help="--flatness: the floor under the trace at --num_point points (a "
                   "coarser level of N points gets E num_point / N); default: calibrated once before training, --flatness_eps_factor times the mean "
                   "trace of the k-neighbourhoods of up to 64 clouds the feeder produces")
    p.add_argument("--flatness_eps_factor", type=float, default=argparse.SUPPRESS, metavar="F", help="--flatness without --flatness_eps: the calibrated "
                   "floor is F times the mean neighbourhood trace (default 1e-2)")
    p.add_argument("--flatness_levels", type=str, default=argparse.SUPPRESS, metavar="L,..", help="--flatness: the levels that carry the term, 1 (the "
                   "coarsest) .. 4 (--num_point points), comma separated (default 1,2,3,4)")
    p.add_argument("--report_spacing", action="store_true", default=argparse.SUPPRESS, help="reports also append the nearest-neighbour spacing statistics of "
                   "the generated and of the val clouds to report/spacing.csv (evaluation.spacing_stats); needs --report_every")
    p.add_argument("--report_lit", action="store_true", default=argparse.SUPPRESS, help="preview sheets shaded by surface normals (two-sided headlight "
                   "shading, normals from the 16 nearest neighbours: pointops.estimate_normals) instead of by depth; needs --report_every")
    p.add_argument("--report_fidelity", action="store_true", default=argparse.SUPPRESS, help="reports also append the distance of the generated "
                   "clouds' points to the surface of the nearest val shape, and of the val clouds to their own, to report/fidelity.csv "
                   "(meshes.point_to_mesh); needs --report_every and a mesh --data_root")
    p.add_argument("--report_surface", action="store_true", default=argparse.SUPPRESS, help="reports also append the surface variation "
                   "lambda0 / (lambda0 + lambda1 + lambda2) of the generated and of the val clouds to report/surface.csv (evaluation.surface_stats); "
                   "needs --report_every")
    p.add_argument("--report_mesh", type=int, nargs="?", const=64, default=argparse.SUPPRESS, metavar="R", help="preview sheets get one more column: "
                   "the surface reconstructed from the finest generated clouds at grid resolution R (default 64; reconstruct.reconstruct), drawn "
                   "as flat-lit triangles in those clouds' frames, and with --report_fidelity a column of the val meshes themselves; needs "
                   "--report_every")
    p.add_argument("--resample_pool", type=int, default=argparse.SUPPRESS, metavar="P", help="clouds stored with more than --num_point points: draw "
                   "each visit's points from the leading P points of a cloud (default: all stored points)")
    p.add_argument("--subsample", choices=["random", "fps"], default=argparse.SUPPRESS, help="the three coarse real resolutions: random (default: "
                   "independent draws with replacement, as the reference's loader) or fps (nested farthest-point subsets of the finest cloud, one more "
                   "launch per iteration)")
    p.add_argument("--mesh_visible", choices=["off", "on", "compute"], default=argparse.SUPPRESS, help="meshes: draw from the VISIBLE surface only -- "
                   "the faces that one of a ring of orthographic views can see (pdgn_mesh_visibility, DESIGN.md section 7m), for the train split and "
                   "the reference draws alike; on: the masks `pack --visible` stored where the file has them, computed at start-up otherwise; "
                   "compute: always computed; off (default): every face")
    p.add_argument("--mesh_views", type=int, choices=[6, 14, 26], default=argparse.SUPPRESS, help="--mesh_visible: views of the ring (default 26)")
    p.add_argument("--mesh_visible_res", type=int, default=argparse.SUPPRESS, metavar="R", help="--mesh_visible: pixels per side of a view's "
                   "depth buffer, 16 .. 192 (default 128)")
    p.add_argument("--ragged", action="store_true", default=argparse.SUPPRESS, help="read the directory --data_root as ragged clouds: "
                   "<synsetid>/<split>/* of .npy / .pts / .xyz / .txt files that store different numbers of points (a packed ragged .npz "
                   "identifies itself and needs no flag)")
    p.add_argument("--min_points", type=int, default=argparse.SUPPRESS, metavar="K", help="ragged clouds: drop the shapes that store fewer than K "
                   "points at load (default 1: none)")
    return p


class Args(argparse.Namespace):
    """The parsed command line.  --ema_decay, the gradient guard's, the learning-rate, the augmentation flags (the adaptive ones too), --gan_loss, --resample_pool, --subsample, --emd, the --mesh_visible flags, --ragged and --min_points are listed (vars(), the log's first line) only where
    they were given: a run without them has the namespace, and writes the log line, of the time before the flags existed; reading
    them gives the defaults below then."""
    ema_decay = 0.0
    grad_guard = False
    clip_grad_norm = None
    guard_max_skips = 50
    lr_g = None
    lr_d = None
    lr_schedule = None
    lr_warmup_iters = 0
    lr_final_factor = 0.0
    lr_step_epochs = None
    lr_gamma = 0.1
    emd = "approx"
    d_augment = None                                             # (the ranges' defaults are augment.DEFAULTS: one place)
    aug_rotate = None
    aug_scale = None
    aug_flip = None
    aug_translate = None
    aug_jitter = None
    d_augment_target = None                                      # (the others' defaults are augment.ADA_DEFAULTS: one place)
    ada_interval = None
    ada_span = None
    ada_p_min = None
    ada_p_max = None
    gan_loss = "lsgan"
    resample_pool = None
    subsample = "random"
    mesh_visible = "off"
    mesh_views = 26
    mesh_visible_res = 128
    ragged = False
    min_points = 1
    repulsion = None
    repulsion_radius = None                                      # (None: calibrated from the feeder's clouds)
    repulsion_radius_factor = 1.0
    repulsion_levels = "1,2,3,4"
    flatness = None
    flatness_k = 16
    flatness_eps = None                                          # (None: calibrated from the feeder's clouds)
    flatness_eps_factor = 1e-2
    flatness_levels = "1,2,3,4"
    report_spacing = False
    report_lit = False
    report_surface = False
    report_fidelity = False
    report_mesh = None


def parse_args(argv=None):
    p = build_parser()
    args = p.parse_args(argv, namespace=Args())
    if args.model_dir is None:
        p.error("please create model dir (--model_dir)")                                       # main.py:56-58
    if args.dataset != "shapenet15k":
        p.error("--dataset %s: only shapenet15k is supported (the ModelNet / Part loaders are not part of pdgn_amd)" % args.dataset)
    if args.phase not in ("train", "test"):
        p.error("--phase %s: train or test" % args.phase)
    if args.noise_dim != 128:
        p.error("--noise_dim %d: the generator takes 128" % args.noise_dim)
    if args.num_point < 16 or args.num_point % 16:
        p.error("--num_point %d: a multiple of 16 (the generator doubles base_points four times)" % args.num_point)
    if args.max_epoch < 1 or args.batch_size < 1:
        p.error("--max_epoch and --batch_size must be at least one")
    if args.report_every < 0 or args.report_rows < 1:
        p.error("--report_every must not be negative and --report_rows at least one")
    if not 0.0 <= args.ema_decay < 1.0:
        p.error("--ema_decay %r: at least 0 and below 1" % args.ema_decay)
    if args.clip_grad_norm is not None:
        if not args.clip_grad_norm > 0.0:
            p.error("--clip_grad_norm %r: a positive number" % args.clip_grad_norm)
        args.grad_guard = True
    if args.guard_max_skips < 1:
        p.error("--guard_max_skips must be at least one")
    if args.resample_pool is not None and args.resample_pool < args.num_point:
        p.error("--resample_pool %d: at least --num_point %d" % (args.resample_pool, args.num_point))
    if args.emd == "auction" and args.num_point > 2048:
        p.error("--emd auction: --num_point %d, the auction kernel holds at most 2048 points" % args.num_point)
    if args.subsample == "fps" and args.num_point > 8192:
        p.error("--subsample fps: --num_point %d, the farthest-point kernel holds at most 8192 points" % args.num_point)
    given = vars(args)
    if args.mesh_visible == "off" and ("mesh_views" in given or "mesh_visible_res" in given):
        p.error("--mesh_views and --mesh_visible_res go with --mesh_visible on / compute")
    if args.min_points < 1:
        p.error("--min_points %d: at least one" % args.min_points)
    if not 16 <= args.mesh_visible_res <= 192:
        p.error("--mesh_visible_res %d: 16 .. 192 (the depth buffer of a view lives in one workgroup's LDS)" % args.mesh_visible_res)
    for flag in ("lr_g", "lr_d"):
        rate = getattr(args, flag)
        if rate is not None and not (rate >= 0.0 and rate != float("inf")):
            p.error("--%s %r: a finite rate, not negative" % (flag, rate))
    kind = args.lr_schedule
    if kind is None:
        for flag in ("lr_warmup_iters", "lr_final_factor", "lr_step_epochs", "lr_gamma"):
            if flag in given:
                p.error("--%s needs --lr_schedule" % flag)
    else:
        if args.lr_warmup_iters < 0:
            p.error("--lr_warmup_iters must not be negative")
        if kind not in ("linear", "cosine") and "lr_final_factor" in given:
            p.error("--lr_final_factor goes with --lr_schedule linear or cosine, not %s" % kind)
        if not (args.lr_final_factor >= 0.0 and args.lr_final_factor != float("inf")):
            p.error("--lr_final_factor %r: finite and not negative" % args.lr_final_factor)
        if kind != "step" and ("lr_step_epochs" in given or "lr_gamma" in given):
            p.error("--lr_step_epochs and --lr_gamma go with --lr_schedule step, not %s" % kind)
        if kind == "step":
            if args.lr_step_epochs is None or args.lr_step_epochs < 1:
                p.error("--lr_schedule step needs --lr_step_epochs of at least one")
            if not (args.lr_gamma > 0.0 and args.lr_gamma != float("inf")):
                p.error("--lr_gamma %r: a positive number" % args.lr_gamma)
            drops = (args.max_epoch - 1) // args.lr_step_epochs  # (a drop every lr_step_epochs epochs, none at the end: whatever the batches per epoch)
            if 1 + (args.lr_warmup_iters > 0) + 2 * drops > 16:
                p.error("--lr_schedule step: %d drops in %d epochs do not fit into the schedule's 16 knots" % (drops, args.max_epoch))
    if args.d_augment is None:
        for flag in ("aug_rotate", "aug_scale", "aug_flip", "aug_translate", "aug_jitter"):
            if flag in given:
                p.error("--%s needs --d_augment" % flag)
    else:
        from .augment import validate
        try:
            validate(**augment_kwargs(args))
        except ValueError as e:
            p.error("--d_augment: %s" % e)
    if args.repulsion is None:
        for flag in ("repulsion_radius", "repulsion_radius_factor", "repulsion_levels"):
            if flag in given:
                p.error("--%s needs --repulsion" % flag)
    else:
        if not (args.repulsion >= 0.0 and args.repulsion != float("inf")):
            p.error("--repulsion %r: a finite weight, not negative" % args.repulsion)
        if args.repulsion_radius is not None and not (args.repulsion_radius > 0.0 and args.repulsion_radius != float("inf")):
            p.error("--repulsion_radius %r: a finite positive radius" % args.repulsion_radius)
        if args.repulsion_radius is not None and "repulsion_radius_factor" in given:
            p.error("--repulsion_radius_factor scales the CALIBRATED radius: it does not go with --repulsion_radius")
        if not (args.repulsion_radius_factor > 0.0 and args.repulsion_radius_factor != float("inf")):
            p.error("--repulsion_radius_factor %r: a finite positive factor" % args.repulsion_radius_factor)
        try:
            repulsion_levels(args)
        except ValueError as e:
            p.error("--repulsion_levels: %s" % e)
        if args.num_point > 8192:
            p.error("--repulsion: --num_point %d, the all-pairs kernel holds at most 8192 points" % args.num_point)
    if args.flatness is None:
        for flag in ("flatness_k", "flatness_eps", "flatness_eps_factor", "flatness_levels"):
            if flag in given:
                p.error("--%s needs --flatness" % flag)
    else:
        if not (args.flatness >= 0.0 and args.flatness != float("inf")):
            p.error("--flatness %r: a finite weight, not negative" % args.flatness)
        if args.flatness_eps is not None and not (args.flatness_eps >= 0.0 and args.flatness_eps != float("inf")):
            p.error("--flatness_eps %r: a finite floor, not negative" % args.flatness_eps)
        if args.flatness_eps is not None and "flatness_eps_factor" in given:
            p.error("--flatness_eps_factor scales the CALIBRATED floor: it does not go with --flatness_eps")
        if not (args.flatness_eps_factor >= 0.0 and args.flatness_eps_factor != float("inf")):
            p.error("--flatness_eps_factor %r: a finite factor, not negative" % args.flatness_eps_factor)
        try:
            levels = flatness_levels(args)
        except ValueError as e:
            p.error("--flatness_levels: %s" % e)
        coarsest = args.num_point >> (3 - levels[0])
        if not 1 <= args.flatness_k <= min(64, coarsest):
            p.error("--flatness_k %d: 1 .. 64 and at most the %d points of level %d" % (args.flatness_k, coarsest, levels[0] + 1))
    if args.report_spacing and not args.report_every:
        p.error("--report_spacing needs --report_every")
    for flag in ("report_lit", "report_surface", "report_fidelity"):
        if getattr(args, flag) and not args.report_every:
            p.error("--%s needs --report_every" % flag)
    if args.report_mesh is not None and not args.report_every:
        p.error("--report_mesh needs --report_every")
    if args.report_mesh is not None and args.report_mesh < 2:
        p.error("--report_mesh takes a grid resolution of at least 2")
    if args.d_augment_target is None:
        for flag in ("ada_interval", "ada_span", "ada_p_min", "ada_p_max"):
            if flag in given:
                p.error("--%s needs --d_augment_target" % flag)
    else:
        if args.d_augment is None:
            p.error("--d_augment_target needs --d_augment (the initial p)")
        from .augment import validate_adaptive
        try:
            validate_adaptive(adaptive_kwargs(args), args.d_augment)
        except ValueError as e:
            p.error("--d_augment_target: %s" % e)
    return args


def repulsion_levels(args):
    """--repulsion_levels "1,3,4" (1 the coarsest .. 4 the finest) -> the trainer's (0, 2, 3); raises ValueError on anything else."""
    try:
        levels = [int(w) for w in str(args.repulsion_levels).split(",")]
    except ValueError:
        raise ValueError("%r: comma-separated integers 1 .. 4" % (args.repulsion_levels,)) from None
    if not levels or len(set(levels)) != len(levels) or min(levels) < 1 or max(levels) > 4:
        raise ValueError("%r: distinct levels from 1 (the coarsest) to 4 (the finest)" % (args.repulsion_levels,))
    return tuple(sorted(l - 1 for l in levels))


def flatness_levels(args):
    """--flatness_levels, read as --repulsion_levels is."""
    try:
        levels = [int(w) for w in str(args.flatness_levels).split(",")]
    except ValueError:
        raise ValueError("%r: comma-separated integers 1 .. 4" % (args.flatness_levels,)) from None
    if not levels or len(set(levels)) != len(levels) or min(levels) < 1 or max(levels) > 4:
        raise ValueError("%r: distinct levels from 1 (the coarsest) to 4 (the finest)" % (args.flatness_levels,))
    return tuple(sorted(l - 1 for l in levels))


def calibrate_flatness_eps(feeder, k=16, factor=1e-2, clouds=64):
    """The floor of --flatness without --flatness_eps: `factor` times the mean trace l0 + l1 + l2 of the k-neighbourhoods
    (pointops.estimate_normals' eigenvalues) of up to `clouds` finest-resolution clouds that the feeder itself produces -- the leading
    batches of epoch 1, into buffers of its own.  Under data parallelism rank 0's value goes to every rank."""
    import torch.distributed as dist
    from .pointops import estimate_normals
    reals, z1, z2 = feeder.buffers()
    got = []
    for i in range(min(feeder.batches_per_epoch, -(-int(clouds) // reals[3].shape[0]))):
        feeder.fill(1, i, reals, z1, z2)
        got.append(reals[3].transpose(1, 2).contiguous())
    pcs = torch.cat(got)[:int(clouds)].contiguous()
    _, eig = estimate_normals(pcs, k=int(k), return_eig=True)
    eps = float(factor) * float(eig.double().sum(dim=2).mean().item())
    if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
        t = torch.tensor([eps], dtype=torch.float64, device=pcs.device)
        dist.broadcast(t, 0)
        eps = float(t.item())
    if not (eps >= 0.0 and eps != float("inf")):
        raise SystemExit("--flatness: the calibrated floor is %r (the feeder's clouds have no finite neighbourhood trace); give --flatness_eps" % eps)
    return eps, pcs.shape[0]


def flatness_arg(args, eps=None):
    """PDGNTrainer's `flatness` from the command line (None without --flatness); eps: the calibrated one where --flatness_eps was not given."""
    if args.flatness is None:
        return None
    return {"weight": args.flatness, "k": args.flatness_k, "eps": args.flatness_eps if args.flatness_eps is not None else eps,
            "levels": flatness_levels(args)}


def calibrate_repulsion_radius(feeder, factor=1.0, clouds=64):
    """The radius of --repulsion without --repulsion_radius: `factor` times the mean nearest-neighbour distance (evaluation.spacing_stats)
    of up to `clouds` finest-resolution clouds that the feeder itself produces -- the leading batches of epoch 1, into buffers of its own.
    Under data parallelism rank 0's value goes to every rank."""
    import torch.distributed as dist
    from .evaluation import spacing_stats
    reals, z1, z2 = feeder.buffers()
    got = []
    for i in range(min(feeder.batches_per_epoch, -(-int(clouds) // reals[3].shape[0]))):
        feeder.fill(1, i, reals, z1, z2)
        got.append(reals[3].transpose(1, 2).contiguous())
    pcs = torch.cat(got)[:int(clouds)].contiguous()
    radius = float(factor) * spacing_stats(pcs)["nn_mean"]
    if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
        t = torch.tensor([radius], dtype=torch.float64, device=pcs.device)
        dist.broadcast(t, 0)
        radius = float(t.item())
    if not (radius > 0.0 and radius != float("inf")):
        raise SystemExit("--repulsion: the calibrated radius is %r (the feeder's clouds have no spacing to measure); give --repulsion_radius" % radius)
    return radius, pcs.shape[0]


def repulsion_arg(args, radius=None):
    """PDGNTrainer's `repulsion` from the command line (None without --repulsion); radius: the calibrated one where --repulsion_radius was not given."""
    if args.repulsion is None:
        return None
    return {"weight": args.repulsion, "radius": args.repulsion_radius if args.repulsion_radius is not None else radius, "levels": repulsion_levels(args)}


def adaptive_kwargs(args):
    """augment.Augment's `adaptive` from the command line (None without --d_augment_target): augment.ADA_DEFAULTS where a flag was not given."""
    if args.d_augment_target is None:
        return None
    from .augment import ADA_DEFAULTS
    kw = dict(ADA_DEFAULTS, target=args.d_augment_target)
    for flag, name in (("ada_interval", "interval"), ("ada_span", "span"), ("ada_p_min", "p_min"), ("ada_p_max", "p_max")):
        if getattr(args, flag) is not None:
            kw[name] = getattr(args, flag)
    return kw


def augment_kwargs(args):
    """augment.Augment's parameters from the command line (None without --d_augment): augment.DEFAULTS where a flag was not given."""
    if args.d_augment is None:
        return None
    from .augment import DEFAULTS
    kw = dict(DEFAULTS, p=args.d_augment)
    for flag, name in (("aug_rotate", "rot_max_deg"), ("aug_scale", "scale_max"), ("aug_flip", "flip"), ("aug_translate", "trans_max"),
                       ("aug_jitter", "jitter_sigma")):
        if getattr(args, flag) is not None:
            kw[name] = bool(getattr(args, flag)) if name == "flip" else getattr(args, flag)
    return kw


def schedule_knots(args, batches_per_epoch):
    """The knot list of the command line's schedule over max_epoch x batches_per_epoch updates (None without --lr_schedule);
    --lr_step_epochs is converted by the same factor, --lr_warmup_iters is in updates already."""
    if args.lr_schedule is None:
        return None
    from .schedule import knots
    nb = int(batches_per_epoch)
    return knots(args.lr_schedule, args.max_epoch * nb, args.lr_warmup_iters, args.lr_final_factor,
                 None if args.lr_step_epochs is None else args.lr_step_epochs * nb, args.lr_gamma)


def logged_args(args):
    """What the first line of <log_info> shows: with reports off (--report_every 0) the namespace without the report flags, so
    that the file is what it was before they existed."""
    return argparse.Namespace(**{k: v for k, v in vars(args).items() if args.report_every or not k.startswith("report_")})


def _open_pc15k(root, synsetids=None):
    """A directory <synsetid>/<split>/*.npy, each file one (M,3) cloud (ShapeNetCore.v2.PC15k) -> {synsetid: {split: (S,M,3) fp32}},
    the files of a split in sorted name order; synsetids: load these categories only."""
    out, points = {}, None
    for sid in sorted(os.listdir(root)):
        if not os.path.isdir(os.path.join(root, sid)) or (synsetids is not None and sid not in synsetids):
            continue
        for split in ("train", "val", "test"):
            folder = os.path.join(root, sid, split)
            if not os.path.isdir(folder):
                continue
            clouds = []
            for name in sorted(n for n in os.listdir(folder) if n.endswith(".npy")):
                pc = np.load(os.path.join(folder, name))
                if pc.ndim != 2 or pc.shape[1] != 3:
                    raise ValueError("%s: a cloud is (M,3), got %s" % (os.path.join(folder, name), pc.shape))
                if points is None:
                    points = pc.shape[0]
                if pc.shape[0] != points:
                    raise ValueError("%s has %d points, the clouds read before it %d: every cloud of a data set must store the same "
                                     "number of points" % (os.path.join(folder, name), pc.shape[0], points))
                clouds.append(pc.astype(np.float32, copy=False))
            if clouds:
                out.setdefault(sid, {})[split] = np.stack(clouds, 0)
    if not out:
        raise ValueError("%s: no <synsetid>/<split>/*.npy clouds found" % (root,))
    return out


def open_data_root(path, synsetids=None):
    """What ShapeNetCore takes as `path`: the HDF5 path itself, or -- for an .npz with '<synsetid>/<split>' keys or a directory
    <synsetid>/<split>/*.npy -- the {synsetid: {split: array}} mapping (a directory: of `synsetids` only, where given)."""
    if os.path.isdir(path):
        return _open_pc15k(str(path), synsetids)
    if str(path).endswith(".npz"):
        out = {}
        with np.load(path) as f:
            for key in f.files:
                sid, split = key.split("/")
                out.setdefault(sid, {})[split] = f[key]
        return out
    return path


def load_split(args, split, scale_mode, tail=None):
    """tail = N: the last N points of every stored cloud (ShapeNetCore's `tail`): the reference clouds of the test phase and the reports."""
    from .data import ShapeNetCore, cate_to_synsetid, synsetid_to_cate
    cates = args.choice
    src = open_data_root(args.data_root, None if cates is None or cates not in cate_to_synsetid else {cate_to_synsetid[cates]})
    if cates is None:                                            # the reference's category 'full'
        cates = [synsetid_to_cate[s] for s in sorted(src)] if isinstance(src, dict) else "all"
    return ShapeNetCore(cates, split, scale_mode, src, tail=tail)


def _ragged_root(args):
    """The opened ragged data of --data_root ({synsetid: {split: [clouds]}}, of --choice's category only): a packed ragged .npz, or a
    directory under --ragged; None where --data_root holds anything else.  Decided before open_data_root is reached, and the flags that
    cannot apply are refused here, before anything is built."""
    from . import clouds
    from .data import cate_to_synsetid
    packed = clouds.is_ragged_root(args.data_root)
    if not packed and not args.ragged:
        if "min_points" in vars(args):
            raise SystemExit("--min_points: %s does not hold ragged clouds (a packed ragged .npz, or a directory under --ragged) -- every other "
                             "storage form has one count per data set, there is nothing to drop" % args.data_root)
        return None
    if not packed and not os.path.isdir(args.data_root):
        raise SystemExit("--ragged: %s is neither a directory <synsetid>/<split>/* of clouds nor the .npz `python -m pdgn_amd.clouds pack` "
                         "makes of one" % args.data_root)
    if args.mesh_visible != "off":
        raise SystemExit("--mesh_visible %s: %s holds ragged point clouds -- visibility is decided per face of a mesh, and stored clouds carry "
                         "no faces; give a mesh --data_root or drop the flag" % (args.mesh_visible, args.data_root))
    if args.resample_pool is not None:
        raise SystemExit("--resample_pool: %s holds ragged clouds -- every shape has its own count and every visit draws from all of its "
                         "points, there is no common leading pool to restrict" % args.data_root)
    if args.choice is not None and args.choice not in cate_to_synsetid:
        raise SystemExit("--choice %s: not a ShapeNetCore category" % args.choice)
    try:
        root = clouds.open_ragged_root(args.data_root, None if args.choice is None else {cate_to_synsetid[args.choice]})
    except ValueError as e:
        raise SystemExit("%s: %s" % (args.data_root, e))
    if not root:
        raise SystemExit("--choice %s: %s has no clouds of that category" % (args.choice, args.data_root))
    return root


def _ragged_cloudset(args, ragged_root, split, normalize):
    """split_cloudset under --min_points, with the one line on standard output that says what was dropped and how the counts lie."""
    from .clouds import split_cloudset
    try:
        cs = split_cloudset(ragged_root, split, normalize, min_points=args.min_points)
    except ValueError as e:
        raise SystemExit("%s: %s" % (args.data_root, e))
    st = cs.stats(args.num_point)
    print("ragged clouds, %s split: %d shapes dropped by --min_points %d; %d shapes, %d points, counts min %d / median %g / max %d, "
          "%d shapes store fewer than --num_point %d" % (split, cs.dropped, args.min_points, st["shapes"], st["points"], st["min"],
                                                          st["median"], st["max"], st["shorter"], st["n"]))
    return cs


def _mesh_root(args):
    """The opened mesh data of --data_root ({synsetid: {split: (verts, faces, face_off)}}, of --choice's category only), or None where
    --data_root holds clouds."""
    from . import meshes
    from .data import cate_to_synsetid
    if not meshes.is_mesh_root(args.data_root):
        if args.mesh_visible != "off":
            raise SystemExit("--mesh_visible %s: %s holds point clouds -- visibility is decided per face of a mesh, and stored clouds carry no "
                             "faces; give a mesh --data_root or drop the flag" % (args.mesh_visible, args.data_root))
        return None
    if args.choice is not None and args.choice not in cate_to_synsetid:
        raise SystemExit("--choice %s: not a ShapeNetCore category" % args.choice)
    root = meshes.open_mesh_root(args.data_root, None if args.choice is None else {cate_to_synsetid[args.choice]})
    if not root:
        raise SystemExit("--choice %s: %s has no meshes of that category" % (args.choice, args.data_root))
    return root


def _visible_meshset(args, mesh_root, split, normalize, device):
    """split_meshset under --mesh_visible, with the one line on standard output that says what the masks left out."""
    from .meshes import has_stored_visible, split_meshset
    if args.mesh_visible == "off":
        return split_meshset(mesh_root, split, normalize)
    stored = args.mesh_visible == "on" and has_stored_visible(mesh_root, split)
    ms = split_meshset(mesh_root, split, normalize, visible="stored" if stored else
                       {"views": args.mesh_views, "resolution": args.mesh_visible_res, "device": device})
    st = ms.visible_stats()
    print("--mesh_visible %s, %s split (%s): %d of %d faces hidden, %.2f %% of the area kept" % (
        args.mesh_visible, split, "stored masks" if stored else "%d views at %d" % (args.mesh_views, args.mesh_visible_res),
        st["total_hidden"], st["total_faces"], 100.0 * st["total_kept"]))
    return ms


def reference_clouds(args, split, device, mesh_root=None, ragged_root=None):
    """The (S, num_point, 3) reference clouds of the test phase and the reports, normalised by --normalize: the LAST num_point points of
    every stored cloud, or -- for meshes -- draw 0 of num_point surface points of every raw mesh of the split (MeshSet.sample: streams
    of their own, apart from every training draw), which then go through the same point normalisation; for ragged clouds draw 0 of
    num_point points of every raw shape of the split (CloudSet.sample), normalised the same way -- no held-out tail: the counts differ,
    and the splits are different shapes."""
    if ragged_root is not None:
        from .data import normalize_point_clouds
        return normalize_point_clouds(_ragged_cloudset(args, ragged_root, split, None).to(device).sample(args.num_point, args.seed, draw=0),
                                      args.normalize).contiguous()
    if mesh_root is None:
        return load_split(args, split, args.normalize, tail=args.num_point).stack(device).float().contiguous()
    from .data import normalize_point_clouds
    return normalize_point_clouds(_visible_meshset(args, mesh_root, split, None, device).to(device).sample(args.num_point, args.seed, draw=0), args.normalize).contiguous()


def reference_clouds_and_meshset(args, split, device, mesh_root):
    """`reference_clouds` of a mesh root and the split's MeshSet in those clouds' frame (MeshSet.in_frame with the shift and scale the
    normalisation gave every cloud): what SnapshotReporter(fidelity=...) takes.  The clouds are the same bits."""
    from .data import normalize_clouds
    ms = _visible_meshset(args, mesh_root, split, None, device).to(device)
    raw = ms.sample(args.num_point, args.seed, draw=0)
    if args.normalize is None:
        return raw.contiguous(), ms
    clouds, shift, scale = normalize_clouds(raw, args.normalize)
    return clouds.contiguous(), ms.in_frame(shift.reshape(-1, 3), scale.reshape(-1))


def init_dist(device):
    """(rank, world): from the process group under torch.distributed.run, else (0, 1)."""
    import torch.distributed as dist
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world > 1:
        local = int(os.environ.get("LOCAL_RANK", "0"))
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        torch.cuda.set_device(local)
        dist.init_process_group("nccl", device_id=torch.device("cuda", local))
        return dist.get_rank(), dist.get_world_size(), torch.device("cuda", local)
    return 0, 1, torch.device(device)


def make_trainer(args, device, batches_per_epoch=None, repulsion=None, flatness=None):
    from .generator import PointGenerator
    from .trainer import PDGNTrainer
    base = args.num_point // 16
    gen = PointGenerator(args.num_point, args.num_k, softmax=args.softmax == "True", base_points=base)
    # (--phase test loads whichever file it is given -- G.pth or G_ema.pth -- into the generator itself: no average to keep)
    return PDGNTrainer(device=device, lr=args.learning_rate, num_k=args.num_k, base_points=base, generator=gen,
                       ema_decay=args.ema_decay if args.phase == "train" else 0.0,
                       grad_guard=args.grad_guard and args.phase == "train",
                       clip_grad_norm=args.clip_grad_norm if args.phase == "train" else None,
                       lr_g=args.lr_g if args.phase == "train" else None, lr_d=args.lr_d if args.phase == "train" else None,
                       lr_schedule=schedule_knots(args, batches_per_epoch) if args.phase == "train" and batches_per_epoch else None,
                       augment=_augment_arg(args) if args.phase == "train" else None, gan_loss=args.gan_loss,
                       repulsion=repulsion if args.phase == "train" else None,
                       **({"flatness": flatness} if flatness is not None and args.phase == "train" else {}))


def _augment_arg(args):
    kw = augment_kwargs(args)
    if kw is None:
        return None
    ada = adaptive_kwargs(args)
    return dict(kw, seed=args.seed) if ada is None else dict(kw, seed=args.seed, adaptive=ada)


def _resume(args, trainer, ckpt):
    if args.pretrain_model_G is None and args.pretrain_model_D is None:
        return None                                              # a new training (:334-336)
    if args.pretrain_model_G is None or args.pretrain_model_D is None:
        raise SystemExit("--pretrain_model_G and --pretrain_model_D go together")                 # (:354-356, :377-379)
    return trainer.load(os.path.join(ckpt, args.pretrain_model_G), os.path.join(ckpt, args.pretrain_model_D))


def _cloud_feeder(args, device, rank, world):
    from .data import BatchFeeder
    n = args.num_point
    dset = load_split(args, "train", "shape_unit")
    stored = int(dset.pointclouds[0]["pointcloud"].shape[0])
    if stored < n:
        raise SystemExit("--num_point %d but the clouds of %s have %d points" % (n, args.data_root, stored))
    if args.resample_pool is not None and stored == n:
        raise SystemExit("--resample_pool: the clouds of %s have exactly --num_point %d points, there is nothing to draw" % (args.data_root, n))
    if args.resample_pool is not None and args.resample_pool > stored:
        raise SystemExit("--resample_pool %d but the clouds of %s have %d points" % (args.resample_pool, args.data_root, stored))
    return BatchFeeder.from_dataset(dset, device, args.batch_size, (n // 8, n // 4, n // 2), args.seed, rank=rank, world=world,
                                      num_point=n, pool=args.resample_pool, subsample=args.subsample)


def _mesh_feeder(args, mesh_root, device, rank, world):
    """Meshes: the train split normalised over its surface (the cloud path's 'shape_unit'), resident on the device; every visit is a
    fresh surface sample (data.MeshFeeder)."""
    from .data import MeshFeeder
    if args.resample_pool is not None:
        raise SystemExit("--resample_pool: %s holds meshes -- every visit of a shape already draws fresh points from its whole surface, "
                         "there is no stored pool to restrict" % args.data_root)
    n = args.num_point
    try:
        ms = _visible_meshset(args, mesh_root, "train", "shape_unit", device)
    except ValueError as e:
        raise SystemExit("%s: %s" % (args.data_root, e))
    return MeshFeeder(ms.to(device), args.batch_size, (n // 8, n // 4, n // 2), args.seed, rank=rank, world=world, num_point=n,
                      subsample=args.subsample)


def _ragged_feeder(args, ragged_root, device, rank, world):
    """Ragged clouds: the train split normalised cloud by cloud (the cloud path's 'shape_unit'), resident on the device; every visit is
    a fresh draw of the shape's own points (data.RaggedFeeder)."""
    from .data import RaggedFeeder
    n = args.num_point
    cs = _ragged_cloudset(args, ragged_root, "train", "shape_unit")
    return RaggedFeeder(cs.to(device), args.batch_size, (n // 8, n // 4, n // 2), args.seed, rank=rank, world=world, num_point=n,
                        subsample=args.subsample)


def train(args):
    rank, world, device = init_dist(args.device)
    run_dir = os.path.join(args.checkpoint_dir, args.model_dir)
    ckpt = os.path.join(run_dir, args.network)
    os.makedirs(ckpt, exist_ok=True)
    torch.manual_seed(args.seed)                                 # the networks' initial weights
    n = args.num_point
    ragged_root = _ragged_root(args)
    mesh_root = None if ragged_root is not None else _mesh_root(args)
    if ragged_root is not None:
        feeder = _ragged_feeder(args, ragged_root, device, rank, world)
    elif mesh_root is not None:
        feeder = _mesh_feeder(args, mesh_root, device, rank, world)
    else:
        feeder = _cloud_feeder(args, device, rank, world)
    radius = None
    if args.repulsion is not None and args.repulsion_radius is None:
        radius, used = calibrate_repulsion_radius(feeder, args.repulsion_radius_factor)
        if rank == 0:
            print("# repulsion radius: %.9g (%g x the mean nearest-neighbour distance of %d clouds of %d points)"
                  % (radius, args.repulsion_radius_factor, used, n))
    floor = None
    if args.flatness is not None and args.flatness_eps is None:
        floor, used = calibrate_flatness_eps(feeder, args.flatness_k, args.flatness_eps_factor)
        if rank == 0:
            print("# flatness eps: %.9g (%g x the mean trace of the %d-neighbourhoods of %d clouds of %d points)"
                  % (floor, args.flatness_eps_factor, args.flatness_k, used, n))
    try:
        trainer = make_trainer(args, device, feeder.batches_per_epoch, repulsion_arg(args, radius),
                               **({"flatness": flatness_arg(args, floor)} if args.flatness is not None else {}))
    except ValueError as e:                                      # (a schedule that does not fit this run's number of updates)
        raise SystemExit(str(e))
    trainer.train()
    if rank == 0 and trainer.repulsion is not None:
        print("# repulsion: weight %g, radius %.9g, levels %s" % (trainer.repulsion["weight"], trainer.repulsion["radius"],
                                                                  ",".join(str(l + 1) for l in trainer.repulsion["levels"])))
    if rank == 0 and getattr(trainer, "flatness", None) is not None:
        print("# flatness: weight %g, k %d, eps %.9g, levels %s" % (trainer.flatness["weight"], trainer.flatness["k"], trainer.flatness["eps"],
                                                                    ",".join(str(l + 1) for l in trainer.flatness["levels"])))
    if rank == 0 and trainer.gan_loss != "lsgan":
        print("# adversarial objective: %s (scores are logits; decision boundary 0)" % trainer.gan_loss)
    start = _resume(args, trainer, ckpt) or 1
    log = None
    if rank == 0:
        path = os.path.join(run_dir, args.log_info)
        with open(path, "a") as f:
            f.write(str(logged_args(args)) + "\n")

        def log(line, _f=path):
            print(line)
            with open(_f, "a") as f:
                f.write(line + "\n")
    reporter = None
    if args.report_every > 0 and rank == 0:
        from .report import SnapshotReporter
        val_meshset = None
        if args.report_fidelity:
            if mesh_root is None:
                raise SystemExit("--report_fidelity: %s holds point clouds -- the distance is measured to the faces of the val meshes; give a "
                                 "mesh --data_root or drop the flag" % args.data_root)
            val, val_meshset = reference_clouds_and_meshset(args, "val", device, mesh_root)
        else:
            val = reference_clouds(args, "val", device, mesh_root, ragged_root)
        reporter = SnapshotReporter(trainer, val, os.path.join(run_dir, "report"), args.report_every, args.batch_size, args.normalize,
                                    args.seed, rows=args.report_rows, full=args.report_full, rank=rank, emd=args.emd,
                                    **({"spacing": True} if args.report_spacing else {}), **({"lit": True} if args.report_lit else {}),
                                    **({"surface": True} if args.report_surface else {}),
                                    **({"mesh": args.report_mesh} if args.report_mesh is not None else {}),
                                    **({"fidelity": val_meshset} if val_meshset is not None else {}))
    last = trainer.fit(feeder, args.max_epoch, start_epoch=start, snapshot=args.snapshot, checkpoint_dir=ckpt,
                       category=args.choice or "full", log=log, on_epoch=reporter, guard_max_skips=args.guard_max_skips,
                       grad_norms=os.path.join(run_dir, "grad_norms.csv") if args.grad_guard else None,
                       lr_log=os.path.join(run_dir, "lr.csv"), aug_log=os.path.join(run_dir, "aug.csv"),
                       **({"repulsion_log": os.path.join(run_dir, "repulsion.csv")} if trainer.repulsion is not None else {}),
                       **({"flatness_log": os.path.join(run_dir, "flatness.csv")} if getattr(trainer, "flatness", None) is not None else {}))
    torch.cuda.synchronize(device)
    if world > 1:
        torch.distributed.barrier()
        torch.distributed.destroy_process_group()
    print(" [*] Training finished! (epoch %d)" % last)
    return last


def test(args):
    from . import evaluation
    device = torch.device(args.device)
    ckpt = os.path.join(args.checkpoint_dir, args.model_dir, args.network)
    ragged_root = _ragged_root(args)                             # (first: a flag that does not fit the data is refused before anything is built)
    mesh_root = None if ragged_root is not None else _mesh_root(args)
    trainer = make_trainer(args, device)
    if _resume(args, trainer, ckpt) is None:
        print(" [!] Load failed...")                             # (:275-276: the reference goes on with the initial weights too)
    save_dir = os.path.join(args.save_dir, "GEN_Ours_%s_%d" % (args.choice or "full", int(time.time())))
    os.makedirs(save_dir, exist_ok=True)
    torch.manual_seed(args.seed)                                 # seed_all (:282)
    np.random.seed(args.seed)
    random.seed(args.seed)
    ref = reference_clouds(args, "test", device, mesh_root, ragged_root)
    trainer.G.eval()
    gen, results, raw = evaluation.generate_and_evaluate(trainer.G, ref, args.batch_size, normalize=args.normalize, return_raw=True,
                                                         emd=args.emd)
    np.save(os.path.join(save_dir, "nonormal_out.npy"), raw.cpu().numpy())
    np.save(os.path.join(save_dir, "out.npy"), gen.cpu().numpy())
    with open(os.path.join(save_dir, "log.txt"), "a") as f:
        if args.emd == "auction":                                # (the default's log.txt is the reference's: metric lines only)
            note = "# EMD: auction (exact assignment on quantised costs, pdgn_auction_assign_indexed); pairs not at an optimum: %d" % int(
                results["emd-capped"])
            print(note)
            f.write(note + "\n")
        else:
            print("# EMD: approx (the reference's approxmatch)")
        for k, v in results.items():
            line = "%s: %.12f" % (k, float(v))                   # (:324-325)
            print(line)
            f.write(line + "\n")
    print(" [*] Test finished!")
    return save_dir


def main(argv=None):
    args = parse_args(argv)
    return train(args) if args.phase == "train" else test(args)


if __name__ == "__main__":
    main()
    sys.exit(0)
