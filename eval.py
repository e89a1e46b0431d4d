"""eval.py - the reference's evaluation entry point (eval.py, pocolib/core/trainer.py:298-403) on the MI355X engine.

    python eval.py --cfg configs/demo_poco_cliff.yaml --ckpt data/poco_cliff.pt --smpl data/smpl/SMPL_NEUTRAL.npz \\
                   --j_regressor data/J_regressor_h36m.npy --dataset 3dpw_test.npz [--img_dir DIR]

Prints MPJPE, PA-MPJPE, V2V, the uncertainty / pose-error correlation and N, and writes evaluation_results_<name>.npz (numeric
arrays; the reference joblib-dumps a dict).  The metrics are computed on the GPU (poco_amd/evaluate.py, csrc/eval_metrics.hip):
per crop nothing is copied to the host between the forward and the final reduction.  --likelihood adds the Var-MPJPE and Variance
lines of the reference and the held-out flow NLL - the likelihood of the ground-truth pose under the model's own RealNVP, the
quantity the uncertainty was trained on (csrc/eval_likelihood.hip, DESIGN.md "Likelihood").  --uncert_threshold T evaluates only
the confident rows of a dataset that demo.py --save_dataset wrote (its `var` array, selected as the reference's BaseDataset selects).
--segm (PARE variants; the dataset needs `pose`, `shape` and `part`, as demo.py --save_dataset writes them) scores the part
segmentation head: per batch the ground-truth mesh is rasterised on the GPU into the 24 body parts plus background with the
reference's crop camera and pred_segm_mask is scored against it - cross-entropy, pixel accuracy, mean IoU (poco_amd/segm.py,
csrc/part_labels.hip, csrc/segm_metrics.hip); --part_mapping FILE replaces the default vertex -> part table.
--crop dataset cuts the crops as the reference's dataset code does (crop_cv2 on the float32 image) instead of with the demo's crop,
one launch per batch; --aug_rot / --aug_scale / --aug_flip / --aug_noise perturb every sample, --augment [--aug_seed S] draws per
sample from the config's training-time distribution; the ground truth is transformed with the crop (poco_amd/datacrop.py,
csrc/dataset_crop.hip).  --aug_occlude FILE pastes the reference's synthetic occluders over every crop inside
that launch and reports how the uncertainty follows the covered area.
--cfg2 FILE --ckpt2 FILE [--inf_model2 best] [--select crop|joint] [--select_scale S] evaluates a second model on the same crops and
the selection between the two by their own uncertainty (demo.py's flags): the lines above for model 1, model 2
and the selection, Oracle MPJPE / PA-MPJPE (per crop the better model: the bound no selection beats), the selection accuracy and the
share of crops taken from model 2; the .npz holds the selection under the usual keys and gains the models' mpjpe / pampjpe / v2v as
*_m1 / *_m2, select and select_score.  Not with --segm or --likelihood.
--tta VIEWS [--tta_weight uncert|uniform] (with --crop dataset) regresses K views of every crop - VIEWS is a comma-separated list
of '+'-joined flip, rot:<degrees>, scale:<factor>, e.g. flip,rot:-15,rot:15; the untransformed crop is always the first view - in
one forward, takes every view's rotations back into the crop's frame and fuses them per joint, weighted by the model's own
uncertainty or uniformly (poco_amd/tta.py, csrc/tta_fuse.hip).  Printed: the lines above for the base view and
the fused result, and Corr(view spread, pose distance), the disagreement baseline a learnt uncertainty is compared against; the .npz
holds the fused result under the usual keys and gains *_base, tta_spread [N,24] and tta_views.  Not with --aug_*, --augment, --cfg2,
--segm or --likelihood.
--rank_metrics [--rank_bins K] measures the uncertainty as a ranking, which is how --uncert_threshold, --infill and --select use it:
the records are sorted by uncertainty on the GPU (csrc/rank_curve.hip, poco_amd/ranking.py) and Spearman's
rho is printed beside Pearson's r, then AUSE / AURG (area of the sparsification curve against the oracle ranking / a random one) of
MPJPE, PA-MPJPE, V2V and the pose distance, then per kept fraction the uncertainty threshold and the errors of the crops kept; the
.npz gains rank_spars_*, rank_oracle_*, rank_reliab_*, rank_thresholds and rank_summary.  Not with --cfg2, --tta, --segm or
--likelihood.
--calibrate OUT.npz [--calib_split half|parity|none] [--calib_bins K] fits monotone maps from the uncertainty to the observed error by
isotonic regression on the GPU (csrc/isotonic.hip, poco_amd/calibrate.py): crop_mpjpe, crop_pampjpe, crop_v2v,
joint_all and joint_0 .. joint_23, all in one call from the evaluator's records; printed per map: rows, blocks and the held-out ENCE,
bias and 1 - SSE / SSE_const; OUT.npz is what demo.py --calibration reads, and the .npz gains calib_summary.  Allowed beside
--rank_metrics; not with --segm, --likelihood, --cfg2, --tta, --sequences, --kp_refit, --visibility, --aug_* or --augment.

--sequences treats the dataset's rows as the consecutive frames they are in 3DPW and Human3.6M: the rows are grouped into tracks by
folder, person and frame number (poco_amd/sequences.py) and the records are scored on the GPU for Accel, the prediction's own
jitter, and Accel error, the acceleration error of the video papers, both in mm / frame^2 (csrc/track_accel.hip, DESIGN.md section
29).  --seq_post LIST runs up to four pipelines of video mode's post-processing - infill:<thresh>, smooth_uncert:<lambda> and smooth,
joined with '+' - on the device and prints for each MPJPE, PA-MPJPE, V2V, Accel and Accel error with their differences to the raw
prediction: what --infill and --smooth_uncert do to the error against ground truth.  --seq_max_gap, --seq_uncert_ref, --min_cutoff
and --beta carry the operators' remaining parameters (defaults: demo.py's).  The .npz gains seq_track, seq_frame, seq_accel,
seq_accel_err, seq_track_names, seq_pipelines and seq_summary.  Not with --cfg2, --tta, --segm, --likelihood, --rank_metrics, --aug_*
or --augment.
--visibility [--vis_margin M] [--vis_bins K] states the paper's claim - a joint's uncertainty rises when its body part cannot be seen -
per joint: per batch the ground-truth mesh is placed in the crop as --segm places it and counted on the GPU (csrc/part_visibility.hip,
poco_amd/visibility.py) - per crop and body part the pixels in a window of M pixels around the crop (default
res / 2), inside the crop, in front of the rest of the body, and not touched by the occluders of --aug_occlude.  Printed: the mean
visibility per joint, Pearson's and Spearman's Corr(1 - visibility, uncertainty) pooled, per joint and for each of truncation,
self-occlusion and object occlusion, Corr(1 - visibility, per-joint error), and uncertainty and error over K visibility bins (default
5); the .npz gains vis_counts, vis, vis_summary, vis_joint and vis_bins.  Needs `pose`, `shape` and `part`; works for every model and
with --crop dataset, --aug_*, --augment, --segm and --part_mapping.  Not with --cfg2, --tta, --sequences, --rank_metrics or --likelihood.
--kp_refit LAMBDA [--kp_refit_ref 0.3] [--kp_refit_rho 0.1] [--kp_refit_iters 10] [--kp_vis_thresh 0.3] asks what the keypoint
refit of demo.py's video mode does to the error against ground truth: per batch every row's joint rotations and camera are refitted
on the GPU to the dataset's `openpose` [N,25,3] BODY_25 keypoints (the pseudo-GT files of demo.py --save_dataset carry them), the
network's pose being the prior and each joint held by its precision LAMBDA (ref / var)^2 (poco_amd/refit.py, csrc/kp_refit.hip,
DESIGN.md section 31); camera and norm come from pred_cam, center and scale; the refitted pose is re-posed and the raw prediction
and the refit are scored side by side: the usual lines for each, their difference, the mean shift and r(shift, var).  The .npz
gains mpjpe_raw / pampjpe_raw / v2v_raw / val_*_raw, refit_shift, refit_cost and refit_flag.  Not with --cfg2, --tta, --segm,
--likelihood, --sequences, --rank_metrics, --visibility, --aug_* or --augment.
--bootstrap B [--boot_unit crop|track] [--boot_level 0.95] [--boot_seed 0] puts an interval on every headline number: the crops (or
the tracks sequences.group_tracks finds: the rows of 3DPW are consecutive frames of about 60 clips) are resampled B times with
replacement on the GPU (csrc/bootstrap.hip, poco_amd/bootstrap.py) and MPJPE, PA-MPJPE, V2V, the uncertainty /
pose-error correlation and the per-crop Corr(uncertainty, MPJPE) are printed as `name  point  +- se  [lo, hi]  (valid/B)`: the point
estimate, the bootstrap standard error and the percentile interval.  With --cfg2 (Model 1, Model 2, Selected), --tta (Base view,
Fused) and --kp_refit (Raw, Refit) every label gets its lines and every label after the first its paired difference to the first, from
the same draws.  The .npz gains boot_names, boot_summary [S,5], boot_spec (B, units, level, seed) and with --save_results
boot_replicates [B,S].  Allowed beside --rank_metrics, --calibrate, --uncert_threshold, --crop dataset and --aug_*; not with --segm,
--likelihood, --sequences or --visibility.
--corrupt LEVELS [--corrupt_seed S] (with --crop dataset) asks what happens to the error and to the uncertainty as the picture itself
gets worse: LEVELS is a comma-separated list of levels, each a '+'-joined chain of at most four of gaussian_blur:<sigma>,
motion_blur:<L>:<degrees>, pixelate:<f>, contrast:<c>, gamma:<g>, gaussian_noise:<sigma> and jpeg:<quality>, e.g.
gaussian_blur:1,gaussian_blur:2+jpeg:30; the clean crop is always level 0, at most 8 levels in all.  The raw crops (after --aug_* /
--aug_occlude) are degraded on the GPU (csrc/corrupt.hip, poco_amd/corrupt.py; jpeg goes through the device's
encoder and decoder), the K versions of max(1, batch_size // K) crops go through ONE forward and every level is scored side by
side.  Printed per level: the usual lines, mean and median var and the differences to the clean crop; then Pearson's and Spearman's
Corr(delta var, delta MPJPE) over crops x levels.  The .npz holds level 0 under the usual keys and gains corrupt_levels,
corrupt_summary and the per-crop mpjpe_l<k>, pampjpe_l<k>, v2v_l<k>, var_l<k>.  Allowed beside --bootstrap (every level, and its
paired difference to level 0) and --save_results; not with --tta, --cfg2, --segm, --likelihood, --sequences, --visibility,
--kp_refit, --calibrate or --rank_metrics.  These are not ImageNet-C's definitions (those need cv2 and skimage).
Not computed: gendered SMPL models,
multi-GPU evaluation (DESIGN.md "Evaluation").
"""
import argparse
import os
import sys


def parse_args(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--cfg", type=str, required=True, help="config file that defines model hyperparams")
    p.add_argument("--ckpt", type=str, required=True, help="checkpoint path (.pt/.ckpt/.pth or run dir)")
    p.add_argument("--inf_model", type=str, default="best")
    p.add_argument("--smpl", type=str, default="data/smpl/SMPL_NEUTRAL.npz", help="SMPL body model as .npz (tools/convert_smpl.py)")
    p.add_argument("--j_regressor", type=str, required=True, help="J_regressor_h36m.npy: float [17, 6890]")
    p.add_argument("--dataset", type=str, required=True,
                   help="the reference's dataset .npz: imgname, center, scale and pose + shape (SMPL ground truth) or S (joint "
                        "ground truth); optional img [N,3,224,224] normalised crops, orig_shape, gender, person_id")
    p.add_argument("--img_dir", type=str, default=None, help="folder the imgname entries are relative to (without `img` crops)")
    p.add_argument("--dataset_name", default="3dpw", choices=["3dpw", "h36m-p2", "mpi-inf-3dhp"],
                   help="selects the joint map: 17 joints for mpi-inf-3dhp, 14 otherwise")
    p.add_argument("--batch_size", type=int, default=64)
    p.add_argument("--save_results", action="store_true", help="also store pred_jnts3D / gt_jnts3D per sample")
    p.add_argument("--output_folder", type=str, default="out")
    p.add_argument("--no_kinematic_uncert", action="store_false",
                   help="Do not use SMPL Kinematic for uncert (same store_false semantics as demo.py)")
    p.add_argument("--likelihood", action="store_true",
                   help="also print Var-MPJPE, Variance and the held-out flow NLL (needs `pose` in the dataset and "
                        "flow_head.cond_layer in the checkpoint)")
    p.add_argument("--uncert_threshold", type=float, default=None,
                   help="a dataset inferred from POCO (demo.py --save_dataset) carries `var`: evaluate only its confident rows, "
                        "selected as the reference's BaseDataset selects them (kinematic accumulation, then column 0 < T); "
                        "default: every row")
    p.add_argument("--segm", action="store_true",
                   help="PARE variants: also print Segm CE, Segm pixel acc and Segm mIoU of pred_segm_mask against the body-part map "
                        "of the ground-truth mesh (needs `pose`, `shape` and `part` in the dataset and `faces` in the --smpl file)")
    p.add_argument("--part_mapping", type=str, default=None,
                   help="with --segm: the vertex -> part table as .npy / .npz / the reference's smpl_partSegmentation_mapping.pkl "
                        "(default: each vertex's largest skinning weight)")
    p.add_argument("--crop", choices=["demo", "dataset"], default="demo",
                   help="demo: the demo's crop (unrounded box, cv2's uint8 path); dataset: the reference's dataset crop (crop_cv2 on "
                        "the float32 image: rounded centre and box side, no byte rounding), one launch per batch")
    p.add_argument("--aug_rot", type=float, default=None, metavar="DEG", help="rotate every crop by DEG degrees (implies --crop dataset)")
    p.add_argument("--aug_scale", type=float, default=None, metavar="SC", help="scale every box by SC (implies --crop dataset)")
    p.add_argument("--aug_flip", action="store_true", help="mirror every crop left-right (implies --crop dataset)")
    p.add_argument("--aug_noise", type=str, default=None, metavar="R,G,B",
                   help="multiply the channels of every crop by R,G,B, clamped to [0, 255] (implies --crop dataset)")
    p.add_argument("--augment", action="store_true",
                   help="per sample, draw flip, noise, rotation and scale from the config's DATASET.FLIP / NOISE_FACTOR / ROT_FACTOR / "
                        "SCALE_FACTOR as the reference's training-time augm_params does (implies --crop dataset)")
    p.add_argument("--aug_seed", type=int, default=0, help="seed of --augment and --aug_occlude")
    p.add_argument("--aug_occlude", type=str, default=None, metavar="FILE",
                   help="paste 1..7 synthetic occluders per crop over the ground-truth keypoints as the reference's training dataset "
                        "does (occlude_with_pascal_objects_kp); FILE: its pascal_occluders.pkl or an .npz of uint8 [h,w,4] RGBA cut-outs; "
                        "needs `part` in the dataset; composes with the other --aug_* flags and --augment (implies --crop dataset)")
    p.add_argument("--cfg2", type=str, default=None,
                   help="a second model's config: with --ckpt2, both engines regress every crop and model 1, model 2 and the selection "
                        "by uncertainty are evaluated side by side (poco_amd/select.py, evaluate.run_eval_pair)")
    p.add_argument("--ckpt2", type=str, default=None, help="the second model's checkpoint (needs --cfg2)")
    p.add_argument("--inf_model2", type=str, default="best")
    p.add_argument("--select", default=None, choices=["crop", "joint"],
                   help="with --cfg2 --ckpt2: crop (default) = each crop from the model with the lower global uncertainty; joint = "
                        "each joint rotation from the model with the lower uncertainty of that joint, mixed rows re-posed")
    p.add_argument("--select_scale", type=float, default=None,
                   help="with --cfg2 --ckpt2: multiplies the second model's uncertainty before the comparison (default 1.0)")
    p.add_argument("--tta", type=str, default=None, metavar="VIEWS",
                   help="test-time augmentation: comma-separated views, each a '+'-joined set of flip, rot:<degrees>, scale:<factor> "
                        "(e.g. flip,rot:-15,rot:15,flip+scale:1.1; at most 8 with the untransformed crop, which is always there); all "
                        "views go through one forward and are fused per joint on the GPU (needs --crop dataset); a forward takes the views of "
                        "max(1, batch_size // K) crops, so with --batch_size below the K views the engine is built for a batch of K")
    p.add_argument("--tta_weight", default=None, choices=["uncert", "uniform"],
                   help="with --tta: weigh each view's joint by 1 / its uncertainty (default) or uniformly")
    p.add_argument("--rank_metrics", action="store_true",
                   help="also rank-based measures of the uncertainty, sorted and summed on the GPU (poco_amd/ranking.py): Spearman's rho "
                        "beside Pearson's r, AUSE / AURG of MPJPE, PA-MPJPE, V2V and the pose distance, and the table of what "
                        "--uncert_threshold keeps at what error; the .npz gains rank_spars_*, rank_oracle_*, rank_reliab_*, "
                        "rank_thresholds and rank_summary")
    p.add_argument("--rank_bins", type=int, default=None, metavar="K",
                   help="with --rank_metrics: cuts of the sparsification curves = bins of the tables, 1..1024 (default 20)")
    p.add_argument("--calibrate", type=str, default=None, metavar="OUT.npz",
                   help="also fit monotone maps from the uncertainty to the observed error by isotonic regression on the GPU "
                        "(poco_amd/calibrate.py, csrc/isotonic.hip): per crop for MPJPE, PA-MPJPE and V2V, per joint pooled and for each "
                        "of the 24 joints; writes them to OUT.npz for demo.py --calibration and prints their held-out scores; the .npz "
                        "gains calib_summary; allowed beside --rank_metrics")
    p.add_argument("--calib_split", default=None, choices=["half", "parity", "none"],
                   help="with --calibrate: score held out on first / second half of the rows (default), even / odd rows, or not at all")
    p.add_argument("--calib_bins", type=int, default=None, metavar="K",
                   help="with --calibrate: equal-count bins of the prediction for the calibration error, 1..1024 (default 20)")
    p.add_argument("--sequences", action="store_true",
                   help="the dataset's rows are consecutive frames: group them into tracks by folder, person and frame number and "
                        "also print Accel and Accel error (mm / frame^2), scored on the GPU (poco_amd/sequences.py, "
                        "csrc/track_accel.hip); the .npz gains seq_track, seq_frame, seq_accel, seq_accel_err, seq_track_names, "
                        "seq_pipelines and seq_summary")
    p.add_argument("--seq_post", type=str, default=None, metavar="LIST",
                   help="with --sequences: at most four comma-separated pipelines of video mode's post-processing, each a '+'-joined "
                        "chain of infill:<thresh>, smooth_uncert:<lambda> and smooth (e.g. infill:0.3,smooth_uncert:10,"
                        "infill:0.3+smooth_uncert:10); each is run on the device and scored like the raw prediction")
    p.add_argument("--seq_max_gap", type=int, default=None,
                   help="with --seq_post: the max_gap of infill and smooth_uncert, in frames (default 30, as demo.py)")
    p.add_argument("--seq_uncert_ref", type=float, default=None,
                   help="with --seq_post: the uncertainty at which smooth_uncert weighs a frame 1 (default 0.3, as demo.py)")
    p.add_argument("--visibility", action="store_true",
                   help="also the per-joint visibility of the ground-truth body, counted on the GPU (poco_amd/visibility.py, "
                        "csrc/part_visibility.hip): mean visibility per joint, Corr(1 - visibility, uncertainty) pooled, per joint and "
                        "split into truncation, self-occlusion and object occlusion, and a table over visibility bins (needs `pose`, "
                        "`shape` and `part` in the dataset and `faces` in the --smpl file; with --aug_occlude the occluders count); the "
                        ".npz gains vis_counts, vis, vis_summary, vis_joint and vis_bins")
    p.add_argument("--vis_margin", type=int, default=None, metavar="M",
                   help="with --visibility: pixels around the crop in which the body still counts, 0..res (default res / 2); it bounds "
                        "the truncation that can be measured")
    p.add_argument("--vis_bins", type=int, default=None, metavar="K", help="with --visibility: bins of the table, 2..20 (default 5)")
    p.add_argument("--kp_refit", type=float, default=None, metavar="LAMBDA",
                   help="also refit every row's joint rotations and camera to the dataset's `openpose` BODY_25 keypoints on the GPU "
                        "(poco_amd/refit.py, csrc/kp_refit.hip), the network's pose being the prior, each joint held by its precision "
                        "LAMBDA (ref / var)^2, and score the raw prediction and the refit side by side; the .npz gains *_raw, "
                        "refit_shift, refit_cost and refit_flag")
    p.add_argument("--kp_refit_ref", type=float, default=0.3, help="--kp_refit: the uncertainty at which a joint's prior weight is LAMBDA")
    p.add_argument("--kp_refit_rho", type=float, default=0.1,
                   help="--kp_refit: width of the Geman-McClure robustifier in fractions of the box side (<= 0: plain least squares)")
    p.add_argument("--kp_refit_iters", type=int, default=10, help="--kp_refit: Levenberg-Marquardt steps per row, 1..32")
    p.add_argument("--kp_vis_thresh", type=float, default=0.3, help="--kp_refit: the confidence a keypoint needs to count")
    p.add_argument("--bootstrap", type=int, default=None, metavar="B",
                   help="also a cluster bootstrap of B replicates (1..65536) on the GPU (poco_amd/bootstrap.py, csrc/bootstrap.hip): point "
                        "estimate, standard error and percentile interval of MPJPE, PA-MPJPE, V2V and the correlations, and with --cfg2, "
                        "--tta or --kp_refit of the paired differences; the .npz gains boot_names, boot_summary and boot_spec")
    p.add_argument("--boot_unit", default=None, choices=["crop", "track"],
                   help="with --bootstrap: resample crops (default) or the tracks the image names group into (folder, person, frame number)")
    p.add_argument("--boot_level", type=float, default=None, help="with --bootstrap: level of the percentile interval (default 0.95)")
    p.add_argument("--boot_seed", type=int, default=None, help="with --bootstrap: seed of the draws, 0..2^53-1 (default 0)")
    p.add_argument("--corrupt", type=str, default=None, metavar="LEVELS",
                   help="degrade the raw crops on the GPU and score every level side by side (poco_amd/corrupt.py, csrc/corrupt.hip): "
                        "comma-separated levels, each a '+'-joined chain of at most four of gaussian_blur:<sigma>, motion_blur:<L>:<degrees>, "
                        "pixelate:<f>, contrast:<c>, gamma:<g>, gaussian_noise:<sigma>, jpeg:<quality> (e.g. gaussian_blur:1,gaussian_blur:2+jpeg:30; "
                        "at most 8 with the clean crop, which is always level 0); needs --crop dataset; a forward takes the levels of "
                        "max(1, batch_size // K) crops")
    p.add_argument("--corrupt_seed", type=int, default=None, help="with --corrupt: seed of gaussian_noise, 0..2^64-1 (default 0)")
    p.add_argument("--min_cutoff", type=float, default=None, help="with --seq_post: one-euro filter of `smooth` (default 0.004)")
    p.add_argument("--beta", type=float, default=None, help="with --seq_post: one-euro filter of `smooth` (default 1.5)")
    return p.parse_args(argv)


def augmentation_spec(args):
    """The AugSpec the augmentation flags ask for, or None without any; args.crop becomes 'dataset' when one is given.  Refuses,
    before any GPU work: --augment together with a fixed perturbation, an unreadable --aug_noise, a non-positive --aug_scale, and
    the dataset crop on a file that carries ready-made `img` crops."""
    import math
    import numpy as np
    fixed = [n for n, on in (("--aug_rot", getattr(args, "aug_rot", None) is not None), ("--aug_scale", getattr(args, "aug_scale", None) is not None),
                             ("--aug_flip", bool(getattr(args, "aug_flip", False))), ("--aug_noise", getattr(args, "aug_noise", None) is not None)) if on]
    random = bool(getattr(args, "augment", False))
    occlude = getattr(args, "aug_occlude", None) is not None
    if random and fixed:
        sys.exit(f"--augment draws every parameter per sample: it cannot be combined with {', '.join(fixed)}")
    if getattr(args, "crop", "demo") != "dataset" and not (random or fixed or occlude):
        return None
    flags = (["--augment"] if random else fixed) + (["--aug_occlude"] if occlude else [])
    args.crop = "dataset"
    with np.load(args.dataset, allow_pickle=False) as z:
        if "img" in z.files:
            sys.exit(f"{args.dataset}: {' / '.join(flags) if flags else '--crop dataset'} cuts the crops from the images, but the file "
                     "carries ready-made `img` crops: remove `img` and pass --img_dir")
    if not (args.img_dir and os.path.isdir(args.img_dir)):
        sys.exit("--crop dataset reads the images: --img_dir must name the folder the imgname entries are relative to")
    from poco_amd.datacrop import AugSpec
    if random:
        from poco_amd.config import update_hparams
        return AugSpec(random=True, seed=int(getattr(args, "aug_seed", 0)), cfg=update_hparams(args.cfg).DATASET)
    noise = (1.0, 1.0, 1.0)
    if getattr(args, "aug_noise", None) is not None:
        try:
            noise = tuple(float(x) for x in args.aug_noise.split(","))
        except ValueError:
            noise = ()
        if len(noise) != 3 or not all(math.isfinite(x) and x >= 0 for x in noise):
            sys.exit(f"--aug_noise needs three finite, non-negative factors R,G,B, got {args.aug_noise!r}")
    rot = 0.0 if getattr(args, "aug_rot", None) is None else float(args.aug_rot)
    sc = 1.0 if getattr(args, "aug_scale", None) is None else float(args.aug_scale)
    if not math.isfinite(rot):
        sys.exit(f"--aug_rot must be finite, got {rot}")
    if not (math.isfinite(sc) and sc > 0):
        sys.exit(f"--aug_scale must be finite and positive, got {sc}")
    return AugSpec(rot=rot, scale=sc, flip=bool(getattr(args, "aug_flip", False)), noise=noise)


def occlusion_spec(args):
    """The OcclusionSpec --aug_occlude asks for, or None without the flag.  Refuses, before any GPU work: a dataset file without
    `part` (the occluders are centred on the ground-truth keypoints) and a FILE that is missing or holds anything but uint8 RGBA
    cut-outs.  augmentation_spec, which runs first, has refused ready-made `img` crops and a missing --img_dir."""
    path = getattr(args, "aug_occlude", None)
    if path is None:
        return None
    import numpy as np
    from poco_amd import datacrop
    from poco_amd.evaluate import check_occlusion_keys
    with np.load(args.dataset, allow_pickle=False) as z:
        try:
            check_occlusion_keys(z.files)
        except ValueError as e:
            sys.exit(f"{args.dataset}: --aug_occlude: {e}")
    try:
        return datacrop.OcclusionSpec(datacrop.load_occluders(path), seed=int(getattr(args, "aug_seed", 0)), source=path)
    except ValueError as e:
        sys.exit(f"--aug_occlude: {e}")


def check_dataset_file(path: str) -> str:
    """Refuse a dataset file without ground truth before any GPU work; returns 'smpl' or 'joints'."""
    import numpy as np
    from poco_amd.evaluate import check_dataset_keys
    if not os.path.isfile(path):
        sys.exit(f"dataset file not found: {path}")
    with np.load(path, allow_pickle=False) as z:
        try:
            return check_dataset_keys(z.files)
        except ValueError as e:
            sys.exit(f"{path}: {e}")


def check_likelihood_inputs(args) -> None:
    """--likelihood: refuse a dataset without `pose` and a checkpoint without the flow's context layer before any GPU work."""
    import numpy as np
    from poco_amd.checkpoint import read_checkpoint
    with np.load(args.dataset, allow_pickle=False) as z:
        if "pose" not in z.files:
            sys.exit(f"{args.dataset}: --likelihood needs `pose` (the flow scores the ground-truth pose)")
    keys = {(k[len("model."):] if k.startswith("model.") else k) for k in read_checkpoint(args.ckpt, args.inf_model)}
    missing = [k for k in ("flow_head.cond_layer.weight", "flow_head.cond_layer.bias") if k not in keys]
    if missing:
        sys.exit(f"{args.ckpt}: --likelihood needs {missing} (the checkpoint has no flow context layer)")


def check_uncert_threshold(args) -> None:
    """--uncert_threshold: refuse a dataset without `var` and a threshold that keeps no row before any GPU work."""
    import numpy as np
    from poco_amd.evaluate import select_confident
    with np.load(args.dataset, allow_pickle=False) as z:
        try:
            select_confident(z, args.uncert_threshold, args.dataset)
        except ValueError as e:
            sys.exit(str(e))


def check_segm_inputs(args) -> None:
    """--segm: refuse a head without a segmentation mask, a dataset without pose / shape / part, a body model without triangles and
    an unreadable --part_mapping before any GPU work."""
    import numpy as np
    from poco_amd import segm
    from poco_amd.config import update_hparams
    try:
        with np.load(args.dataset, allow_pickle=False) as z:
            segm.check_eval_inputs(update_hparams(args.cfg).POCO.BACKBONE, z.files)
        if getattr(args, "part_mapping", None):
            segm.load_part_mapping(args.part_mapping)
    except ValueError as e:
        sys.exit(f"{args.dataset}: {e}")
    if not os.path.isfile(args.smpl):
        sys.exit(f"--segm: body-model file not found: {args.smpl}")
    with np.load(args.smpl) as z:
        if "faces" not in z.files:
            sys.exit(f"--segm: {args.smpl} has no `faces` array (convert the SMPL .pkl with tools/convert_smpl.py, which keeps its "
                     "triangles)")


def check_select(args) -> None:
    """--cfg2 / --ckpt2 / --select / --select_scale: refuse what cannot work before an engine is built."""
    from poco_amd.select import flag_error
    msg = flag_error(args, ("segm", "likelihood", "rank_metrics"))
    if msg:
        sys.exit(msg)


def check_rank(args) -> None:
    """--rank_metrics / --rank_bins: refuse what cannot work before an engine is built."""
    from poco_amd.ranking import flag_error
    msg = flag_error(args)
    if msg:
        sys.exit(msg)


def check_calibrate(args) -> None:
    """--calibrate / --calib_split / --calib_bins: refuse what cannot work before an engine is built."""
    from poco_amd.calibrate import flag_error
    msg = flag_error(args)
    if msg:
        sys.exit(msg)


def check_tta(args) -> None:
    """--tta / --tta_weight: refuse what cannot work before an engine is built."""
    from poco_amd.tta import flag_error
    msg = flag_error(args, "eval")
    if msg:
        sys.exit(msg)


def check_kp_refit(args) -> None:
    """--kp_refit and its companions: refuse what cannot work before an engine is built - the flags it excludes, options out of
    range, a dataset file without `openpose`."""
    from poco_amd.refit import flag_error
    msg = flag_error(args, "eval")
    if msg:
        sys.exit(msg)
    if getattr(args, "kp_refit", None) is not None and os.path.isfile(args.dataset):
        import numpy as np
        with np.load(args.dataset, allow_pickle=False) as z:
            if "openpose" not in z.files:
                sys.exit(f"{args.dataset}: --kp_refit fits the rows to their 2-D keypoints, but the file has no `openpose` [N,25,3] "
                         "(demo.py --save_dataset writes it)")
            if z["openpose"].shape[1:] != (25, 3):
                sys.exit(f"{args.dataset}: --kp_refit maps BODY_25 keypoints only, but `openpose` is {tuple(z['openpose'].shape)}, not [N,25,3]")


def check_sequences(args) -> None:
    """--sequences / --seq_*: refuse what cannot work before an engine is built - the flags it excludes, an unreadable --seq_post,
    and a dataset whose image names do not group into tracks."""
    from poco_amd.sequences import flag_error, group_tracks
    msg = flag_error(args)
    if msg:
        sys.exit(msg)
    if getattr(args, "sequences", False) and os.path.isfile(args.dataset):
        import numpy as np
        with np.load(args.dataset, allow_pickle=False) as z:
            if "imgname" in z.files and getattr(args, "uncert_threshold", None) is None:
                try:
                    group_tracks(z["imgname"], z["person_id"] if "person_id" in z.files else None)
                except ValueError as e:
                    sys.exit(f"{args.dataset}: --sequences: {e}")


def check_visibility(args) -> None:
    """--visibility / --vis_margin / --vis_bins: refuse what cannot work before an engine is built - the flags it excludes, a bin
    count or margin out of range, a dataset without pose / shape / part, a body model without triangles, an unreadable
    --part_mapping."""
    from poco_amd import visibility
    msg = visibility.flag_error(args)
    if msg:
        sys.exit(msg)
    if not getattr(args, "visibility", False):
        return
    import numpy as np
    from poco_amd import segm
    if not os.path.isfile(args.dataset):
        sys.exit(f"dataset file not found: {args.dataset}")
    try:
        with np.load(args.dataset, allow_pickle=False) as z:
            visibility.check_dataset_keys(z.files)
        if getattr(args, "part_mapping", None):
            segm.load_part_mapping(args.part_mapping)
    except ValueError as e:
        sys.exit(f"{args.dataset}: {e}")
    if not os.path.isfile(args.smpl):
        sys.exit(f"--visibility: body-model file not found: {args.smpl}")
    with np.load(args.smpl) as z:
        if "faces" not in z.files:
            sys.exit(f"--visibility: {args.smpl} has no `faces` array (convert the SMPL .pkl with tools/convert_smpl.py, which keeps "
                     "its triangles)")


def check_bootstrap(args) -> None:
    """--bootstrap / --boot_*: refuse what cannot work before an engine is built - the flags it excludes, options out of range, and
    with --boot_unit track a dataset whose image names do not group into tracks."""
    from poco_amd.bootstrap import flag_error
    msg = flag_error(args)
    if msg:
        sys.exit(msg)
    if getattr(args, "bootstrap", None) is not None and getattr(args, "boot_unit", None) == "track" and os.path.isfile(args.dataset):
        import numpy as np
        from poco_amd.sequences import group_tracks
        with np.load(args.dataset, allow_pickle=False) as z:
            rows = z
            if getattr(args, "uncert_threshold", None) is not None:
                from poco_amd.evaluate import select_confident
                try:
                    rows = select_confident(z, args.uncert_threshold, args.dataset)     # the tracks of the rows that are evaluated
                except ValueError:
                    return                                                              # check_uncert_threshold names what is wrong
            if "imgname" in rows.files:
                try:
                    group_tracks(rows["imgname"], rows["person_id"] if "person_id" in rows.files else None)
                except ValueError as e:
                    sys.exit(f"{args.dataset}: --boot_unit track: {e}")


def check_corrupt(args) -> None:
    """--corrupt / --corrupt_seed: refuse what cannot work before an engine is built."""
    from poco_amd.corrupt import flag_error
    msg = flag_error(args)
    if msg:
        sys.exit(msg)


def calibrate_spec(args, tester):
    """run_eval's `calibrate` argument from --calibrate / --calib_split / --calib_bins, or None."""
    if not getattr(args, "calibrate", None):
        return None
    from poco_amd.calibrate import make_meta
    return {"split": getattr(args, "calib_split", None) or "half", "bins": getattr(args, "calib_bins", None) or 20,
            "meta": make_meta(args.dataset_name, bool(tester.model_cfg.POCO.KINEMATIC_UNCERT), str(tester.model_cfg.POCO.BACKBONE))}


def main(args):
    check_corrupt(args)
    check_bootstrap(args)
    check_calibrate(args)
    check_visibility(args)
    check_sequences(args)
    check_select(args)
    check_tta(args)
    check_rank(args)
    check_kp_refit(args)
    check_dataset_file(args.dataset)
    aug = augmentation_spec(args)
    occ = occlusion_spec(args)
    if getattr(args, "segm", False):
        check_segm_inputs(args)
    if getattr(args, "uncert_threshold", None) is not None:
        check_uncert_threshold(args)
    if args.likelihood:
        check_likelihood_inputs(args)
    if not os.path.isfile(args.j_regressor):
        sys.exit(f"joint regressor not found: {args.j_regressor}")
    import numpy as np
    from poco_amd import evaluate
    from poco_amd.tester import POCOTester
    try:
        crop_kw = dict(crop="dataset", augment=aug) if getattr(args, "crop", "demo") == "dataset" else {}
        if occ is not None:
            crop_kw["occlude"] = occ
        ds = evaluate.EvalDataset(args.dataset, args.img_dir, args.dataset_name,
                                  uncert_threshold=getattr(args, "uncert_threshold", None), **crop_kw)
    except ValueError as e:
        sys.exit(str(e))
    if ds.crop == "dataset":
        print(f"Dataset crop: {ds.augment.describe()}")
    if occ is not None:
        print(f"Synthetic occluders: {occ.describe()}")
    if getattr(args, "uncert_threshold", None) is not None:
        print(f"Confident rows (uncertainty < {args.uncert_threshold}): {len(ds)} of {ds.total}")
    J = np.load(args.j_regressor).astype(np.float32)
    tester = POCOTester(args)                       # builds the engine from --cfg / --ckpt / --smpl exactly as demo.py does
    boot_kw = {}
    if getattr(args, "bootstrap", None) is not None:
        from poco_amd import bootstrap
        boot_kw["bootstrap"] = bootstrap.spec_from_args(args)
    vis_kw = {}
    if getattr(args, "visibility", False):
        from poco_amd import visibility
        try:
            vis_kw["visibility"] = visibility.prepare(tester.model, ds, args.dataset, args.smpl, part_mapping=args.part_mapping,
                                                      batch_size=max(int(args.batch_size), 1),
                                                      uncert_threshold=getattr(args, "uncert_threshold", None),
                                                      res=tester.model_cfg.DATASET.IMG_RES, margin=getattr(args, "vis_margin", None),
                                                      bins=getattr(args, "vis_bins", None) or 5)
        except ValueError as e:
            sys.exit(str(e))
    if getattr(args, "segm", False):
        from poco_amd import segm
        try:
            res = segm.run_eval(tester.model, ds, args.dataset, J, args.smpl, part_mapping=args.part_mapping,
                                batch_size=max(int(args.batch_size), 1), kinematic=bool(tester.model_cfg.POCO.KINEMATIC_UNCERT),
                                save_results=args.save_results, likelihood=args.likelihood,
                                uncert_threshold=getattr(args, "uncert_threshold", None), res=tester.model_cfg.DATASET.IMG_RES, **vis_kw)
        except ValueError as e:
            sys.exit(str(e))
    elif tester.corrupt is not None:
        from poco_amd import corrupt
        print(f"Corruption levels: {corrupt.levels_text(tester.corrupt.levels)}")
        res = evaluate.run_eval_corrupt(tester.corrupt, ds, J, batch_size=max(int(args.batch_size), 1),
                                        kinematic=bool(tester.model_cfg.POCO.KINEMATIC_UNCERT), save_results=args.save_results, **boot_kw)
    elif tester.tta is not None:
        print(f"Test-time views: {tester.tta_text} ({tester.tta.weight} weights)")
        res = evaluate.run_eval_tta(tester.tta, ds, J, batch_size=max(int(args.batch_size), 1),
                                    kinematic=bool(tester.model_cfg.POCO.KINEMATIC_UNCERT), save_results=args.save_results, **boot_kw)
    elif tester.pair is not None:
        res = evaluate.run_eval_pair(tester.pair, ds, J, batch_size=max(int(args.batch_size), 1),
                                     kinematic=bool(tester.model_cfg.POCO.KINEMATIC_UNCERT), save_results=args.save_results, **boot_kw)
    elif getattr(args, "kp_refit", None) is not None:
        from poco_amd import refit
        res = evaluate.run_eval_refit(tester.model, ds, J, refit.joint_tables(args.smpl), float(args.kp_refit), float(args.kp_refit_ref),
                                      float(args.kp_refit_rho), float(args.kp_vis_thresh), int(args.kp_refit_iters),
                                      batch_size=max(int(args.batch_size), 1), kinematic=bool(tester.model_cfg.POCO.KINEMATIC_UNCERT),
                                      save_results=args.save_results, **boot_kw)
    elif getattr(args, "sequences", False):
        from poco_amd.sequences import parse_pipelines
        opt = lambda name, default: default if getattr(args, name, None) is None else getattr(args, name)   # noqa: E731
        try:
            res = evaluate.run_eval_sequences(tester.model, ds, J, batch_size=max(int(args.batch_size), 1),
                                              kinematic=bool(tester.model_cfg.POCO.KINEMATIC_UNCERT), save_results=args.save_results,
                                              pipelines=parse_pipelines(getattr(args, "seq_post", None)),
                                              max_gap=int(opt("seq_max_gap", 30)), uncert_ref=float(opt("seq_uncert_ref", 0.3)),
                                              min_cutoff=float(opt("min_cutoff", 0.004)), beta=float(opt("beta", 1.5)))
        except ValueError as e:
            sys.exit(f"--sequences: {e}")
    else:
        res = evaluate.run_eval(tester.model, ds, J, batch_size=max(int(args.batch_size), 1),
                                kinematic=bool(tester.model_cfg.POCO.KINEMATIC_UNCERT), save_results=args.save_results,
                                likelihood=args.likelihood,
                                rank_metrics=(args.rank_bins or 20) if getattr(args, "rank_metrics", False) else None,
                                calibrate=calibrate_spec(args, tester), **vis_kw, **boot_kw)
    lines = evaluate.pair_report_lines(res, tester.pair.mode) if tester.pair is not None else evaluate.report_lines(res)
    if tester.tta is not None:
        lines = evaluate.tta_report_lines(res)
    if getattr(args, "kp_refit", None) is not None:
        lines = evaluate.refit_report_lines(res)
    if tester.corrupt is not None:
        lines = evaluate.corrupt_report_lines(res)
    for line in (evaluate.likelihood_lines(res) if args.likelihood else []) + lines:
        print(line)
    if getattr(args, "segm", False):
        for line in segm.report_lines(res):
            print(line)
    if getattr(args, "rank_metrics", False):
        for line in evaluate.rank_lines(res):
            print(line)
    if getattr(args, "calibrate", None):
        from poco_amd import calibrate
        for line in calibrate.summary_lines(res["calibration"]):
            print(line)
        calibrate.save(args.calibrate, res["calibration"])
    if boot_kw:
        for line in bootstrap.report_lines(res):
            print(line)
    if getattr(args, "sequences", False):
        for line in evaluate.sequence_lines(res):
            print(line)
    if getattr(args, "visibility", False):
        for line in visibility.report_lines(res):
            print(line)
    if occ is not None:
        for line in evaluate.occlusion_lines(ds, res):
            print(line)
        res.update(occ_count=ds.occ_count.astype(np.int32), occ_cover=ds.occ_cover.astype(np.float32))
    if ds.crop == "dataset":
        res.update(aug_rot=ds.aug_rot.astype(np.float32), aug_flip=ds.aug_flip.astype(np.int32), aug_scale=ds.aug_scale.astype(np.float32),
                   aug_pn=ds.aug_pn.astype(np.float32))
    out = os.path.join(args.output_folder, f"evaluation_results_{args.dataset_name}.npz")
    evaluate.save_npz(out, res, args.dataset_name)
    return res


if __name__ == "__main__":
    main(parse_args())
