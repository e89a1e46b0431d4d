"""demo.py - the reference's demo CLI (demo.py:219-311) on the MI355X engine.

    python demo.py --cfg configs/demo_poco_cliff.yaml --ckpt data/poco_cliff.pt \\
                   --mode folder --image_folder <dir> --output_folder out --smpl data/smpl/SMPL_NEUTRAL.npz

Same flags as the reference where they concern the regressor (--cfg --ckpt --mode --image_folder
--vid_file --output_folder --batch_size --no_render --no_kinematic_uncert --inf_model --sideview --no_uncert_color --wireframe
--draw_keypoints --render_crop).  Detector /
tracker are third-party and out of scope: person boxes come from
--detections (json {image name: [[cx,cy,w,h],...]}, the format multi_person_tracker produces) or
default to one centred box; results are written as .npz.  --render (opt-in; the reference renders by default) draws the
uncertainty-coloured meshes on the GPU (poco_amd/render.py) into the PNGs the reference writes; --image_format jpg encodes them on
the GPU instead (poco_amd/jpeg.py), --encode gpu compresses the PNGs on the GPU (poco_amd/png.py) and --save_video adds the result video as a Motion-JPEG .avi (the reference's ffmpeg step).
--mode video expects --vid_file to be a folder of extracted frames (the reference shells out to
ffmpeg first, demo.py:71; ffmpeg/cv2 are not part of this image) or a Motion-JPEG .avi, which is read frame by frame
(poco_amd/jpeg.py MjpegReader).  --decode gpu decodes baseline .jpg input on the GPU (poco_amd/jpeg.py JpegDecoder): the file's
bytes cross PCIe instead of its pixels; other files go through PIL as with the default --decode host.  --decode_png gpu does the
same for .png input - what the reference's ffmpeg extraction and this demo's own --render write - with the device inflate and
unfilter of poco_amd/png.py PngDecoder.  --decode_progressive gpu does it for progressive .jpg files (SOF2: what web servers
and export pipelines write) with poco_amd/jpeg.py ProgressiveJpegDecoder; the three flags are independent.
--tracking reads both kinds of tracker output of the reference: box tracks ({'bbox', 'frames'}) and 2-D pose tracks ({'joints2d'
[T,K,3], 'frames'}: the reference's --tracking_method pose), whose boxes are derived from the keypoints on the host
(poco_amd/tracks.py); the file's content decides.  --tracking_method pose insists that every track has keypoints,
--kp_vis_thresh is the confidence a keypoint needs to count (0.3 as in the reference), --smooth_bbox median- and Gaussian-filters
the derived box parameters (off, as in the reference's Inference).  A keypoint track's result carries its keypoints as `joints2d`,
and --draw_keypoints stamps those above the threshold black over the green model joints.
--occlusion_map (folder mode) adds PARE's occlusion analysis per detection (poco_amd/occlusion.py): a --occ_patch square of grey
level --occ_fill slides over the crop in steps of --occ_stride, the engine regresses every occluded copy, and
<out>/occlusion/<image>_<det>.png shows --occ_metric per position as a heat map over the crop, <image>_<det>.npz the records.
--save_dataset FILE.npz closes POCO's self-training loop: the predictions become a pseudo-ground-truth dataset in the format the
reference's BaseDataset (and eval.py --dataset) reads - pose as the reference's rotation_matrix_to_angle_axis of the predicted
rotations, var without the kinematic accumulation (the reader applies it), keypoints, center and scale - made on the GPU behind
each forward (poco_amd/pseudo.py, csrc/pseudo_gt.hip); --uncert_threshold T keeps only the crops get_confident_frames would keep.
The printed JSON line gains dataset_offered, dataset_kept and dataset_threshold.  Video mode exports the raw predictions, not the
--smooth-filtered ones.  Not with --gpus N > 1.
--save_segm (folder mode, PARE variants) writes <out>/segm/<image>_<det>.png per detection: the 224 x 224 crop blended 50/50 with the
coloured argmax of the upsampled pred_segm_mask and, beside it, the same crop blended with the 24 body parts of the predicted mesh
rasterised at pred_cam_t (poco_amd/segm.py, csrc/part_labels.hip, csrc/segm_metrics.hip); --part_mapping FILE replaces the default
vertex -> part table (each vertex's largest skinning weight).
--infill THRESH (video mode) puts the per-joint uncertainty to work: per track and per joint, a rotation whose post-processed
uncertainty exceeds THRESH is replaced by the shortest-arc interpolation between the nearest confident frames on either side, if
those are at most --infill_max_gap frames apart, else by the nearer one if it is at most half of that away, else left alone; betas
and orig_cam follow the root joint, the touched frames are re-posed, --smooth then filters the repaired pose (poco_amd/infill.py,
csrc/track_infill.hip).  The result gains infill [T,24] (0 reliable, 1 interpolated, 2 held, 3 left) and pose_net / betas_net /
orig_cam_net, the values before in-filling.  No default threshold: it is the user's statement of what they trust.  Not with --gpus N > 1.
--smooth_uncert LAMBDA (video mode) is the continuous counterpart of --smooth and --infill: per track and per joint a non-causal
penalised least-squares fit over time, its data term weighted by the precision (--smooth_uncert_ref / var)^2, its penalty LAMBDA
times the squared second difference over the frame indices (none across a hole wider than --smooth_uncert_max_gap frames), each
solved matrix taken back onto SO(3); betas and orig_cam are smoothed with the root joint's weights, every frame is re-posed
(poco_amd/usmooth.py, csrc/track_smooth.hip).  The result gains smooth_shift [T,24] (degrees) and pose_net /
betas_net / orig_cam_net; var stays as regressed.  After --infill it works on the in-filled pose.  Not with --smooth (two
smoothers) and not with --gpus N > 1.
--kp_refit LAMBDA (video mode, keypoint tracks) refits the joints the model doubts to the track's own BODY_25 keypoints on the GPU:
per frame a Levenberg-Marquardt fit of the 24 joint rotations and the weak-perspective camera to the 14 body keypoints above
--kp_vis_thresh, the network's pose being the prior and each joint held by its precision LAMBDA (--kp_refit_ref / var)^2, residuals in
fractions of the box side under a Geman-McClure robustifier of width --kp_refit_rho (<= 0: off), --kp_refit_iters steps; shape is
kept, every fitted frame is re-posed (poco_amd/refit.py, csrc/kp_refit.hip).  It runs first, on the finished
unsmoothed tracks; --infill, then --smooth_uncert or --smooth take what it left.  The result gains refit_shift [T,24] (degrees),
refit_cost [T,2], refit_flag [T] (0 fitted, 1 too few keypoints, 2 non-finite input) and pose_net / betas_net / orig_cam_net; var
stays as regressed.  Not with folder, directory or webcam mode, --cfg2 or --gpus N > 1.
--tracker sort (video mode) builds the tracks itself from the per-frame person boxes of --detections - the file folder mode reads -
where the reference runs multi_person_tracker's SORT behind its detector: a constant-velocity Kalman filter per person and one optimal
IoU assignment per frame, all frames of the clip in one launch (poco_amd/sort.py, csrc/sort_tracks.hip).
--track_iou, --track_max_age and --track_min_hits are SORT's three parameters (0.3, 1, 3); --track_boxes filtered crops with the
filter's boxes instead of the file's; --track_backfill gives a reported person the frames before --track_min_hits was reached.  The
tracks go through the same path as a --tracking file's (and are written as <out>/tracking_results_sort.json, which --tracking reads
back).  Not with --tracking or --kp_refit (box tracks have no keypoints); at most 64 people per frame; no detector, no appearance model.
--track_stitch (video mode) rejoins what an occlusion broke: after the forward, the tracks (SORT's or a --tracking file's; those of at
least --stitch_min_frag frames now reach the forward) are fragments, and one optimal assignment per clip on the GPU decides which
fragment continues which - from the regressed body shape, averaged with the model's own precision, and the motion of the boxes
extrapolated from both sides to the middle of the hole of at most --stitch_max_gap frames (poco_amd/stitch.py, csrc/track_stitch.hip,
DESIGN.md section 36).  The frames of a hole get interpolated boxes and go through the forward (--stitch_no_fill leaves them out), chains
under 25 frames are dropped, and --infill, --smooth_uncert and --smooth see one long track.  The result gains stitch [T] (1 = a row that
fills a hole) and stitch_frag [T]; <out>/tracking_results_stitched.json holds the chains for a later --tracking run.  The defaults of
--stitch_motion_tol and --stitch_shape_tol are guesses, not measured on real video.  Not with keypoint tracks, --kp_refit,
--save_dataset or --gpus N > 1.
--cfg2 FILE --ckpt2 FILE [--inf_model2 best] [--select crop|joint] [--select_scale S] runs a second model on the same crops on the
same GPU and lets the uncertainty choose (poco_amd/select.py, csrc/select_regressor.hip): per crop the model
whose global uncertainty (the reference's get_global_uncert of its own head) is lower, S times the second model's against the
first's, a tie to the first; or with --select joint per joint rotation, shape, camera and 2-D joints following the root joint and
the mixed rows re-posed.  Folder and video mode; the result gains select [n,24] and select_score [n,2].  Not with --gpus N > 1,
--occlusion_map, --save_dataset or --save_segm.
--tta VIEWS [--tta_weight uncert|uniform] (folder mode) regresses K views of every detection - VIEWS is a comma-separated list of
'+'-joined flip, rot:<degrees>, scale:<factor>; the untransformed crop is always the first view - in one forward and fuses them per
joint by the model's own uncertainty (poco_amd/tta.py, csrc/tta_fuse.hip).  With the flag every view, the base
view included, is cut with the DATASET crop from the detection's box (centre (cx, cy), scale max(w, h) / 200: rounded centre and
side, no byte rounding), not with the demo's crop.  Pose, betas, verts, joints3d and var / var_global are the fused ones; camera and
2-D joints stay the base view's; the result gains tta_spread [n,24].  Not with video, directory or webcam mode, --cfg2,
--occlusion_map, --save_dataset, --save_segm or --gpus N > 1.
"""
import argparse
import json
import os
import sys


def parse_args(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--cfg", type=str, required=True, help="config file that defines model hyperparams")
    p.add_argument("--ckpt", type=str, required=True, help="checkpoint path (.pt/.ckpt/.pth or run dir)")
    p.add_argument("--inf_model", type=str, default="best")
    p.add_argument("--mode", default="folder", choices=["video", "folder", "directory", "webcam"])
    p.add_argument("--vid_file", type=str, help="folder of extracted video frames, or a Motion-JPEG .avi file")
    p.add_argument("--decode", default="host", choices=["host", "gpu"],
                   help="where input images are decoded: host = PIL on a thread pool; gpu = baseline .jpg files and Motion-JPEG "
                        "frames on the GPU, same pixels (anything else still goes through PIL)")
    p.add_argument("--decode_png", default="host", choices=["host", "gpu"],
                   help="where .png input is decoded: host = PIL; gpu = 8-bit non-interlaced .png files are inflated and unfiltered "
                        "on the GPU, same pixels (anything else still goes through PIL); independent of --decode")
    p.add_argument("--decode_progressive", default="host", choices=["host", "gpu"],
                   help="where progressive .jpg input is decoded: host = PIL; gpu = progressive Huffman files (8 bit, no restart "
                        "interval) are decoded on the GPU, same pixels (anything else still goes through PIL); independent of "
                        "--decode and --decode_png")
    p.add_argument("--image_folder", type=str, help="input image folder")
    p.add_argument("--output_folder", type=str, default="out", help="output folder to write results")
    p.add_argument("--batch_size", type=int, default=64, help="batch size of POCO")
    p.add_argument("--tracker_batch_size", type=int, default=12)
    p.add_argument("--detector", type=str, default="yolo")
    p.add_argument("--no_render", action="store_true", help="disable rendering (wins over --render)")
    p.add_argument("--render", action="store_true",
                   help="draw the uncertainty-coloured meshes over the input (GPU): folder mode <out>/poco_results/<image>.png, "
                        "video mode <out>/tmp_images_output/%%06d.png + uncertainty.log; needs `faces` in the --smpl file")
    p.add_argument("--sideview", action="store_true", help="with --render: add the Ry(270) view to the right of each picture")
    p.add_argument("--wireframe", action="store_true",
                   help="with --render: draw the meshes (the --sideview canvas too) as wireframes: the edges of the front-facing "
                        "triangles as one-pixel depth-tested lines")
    p.add_argument("--draw_keypoints", action="store_true",
                   help="with --render: stamp the 2-D joints on the main view after each person's mesh: folder mode SMPL joints "
                        "white and OpenPose joints black, video mode all 49 in green and a keypoint track's input keypoints above "
                        "--kp_vis_thresh black")
    p.add_argument("--render_crop", action="store_true",
                   help="with --render, folder mode: draw only the first detection of each image, over its own 224 x 224 crop")
    p.add_argument("--image_format", default="png", choices=["png", "jpg"],
                   help="with --render: format of the per-frame pictures; jpg is encoded on the GPU (baseline JPEG, 4:2:0) and only "
                        "its bytes are copied to the host")
    p.add_argument("--encode", default="host", choices=["host", "gpu"],
                   help="with --render --image_format png: where the pictures are compressed: host = PIL on a thread pool; gpu = "
                        "filtered and deflated on the GPU (poco_amd/png.py: lossless, the same pixels, other bytes), only the "
                        "file's bytes are copied to the host.  --image_format jpg is always encoded on the GPU and does not look "
                        "at this flag; without --render there is nothing to encode")
    p.add_argument("--jpeg_quality", type=int, default=90, help="quality 1..100 of --image_format jpg and --save_video")
    p.add_argument("--save_video", action="store_true",
                   help="video mode with --render: also write <out>/<frame folder>_poco_result.avi (Motion-JPEG, --fps)")
    p.add_argument("--fps", type=float, default=30.0, help="frame rate of --save_video")
    p.add_argument("--no_uncert_color", action="store_true", help="with --render: plain grey meshes instead of the uncertainty colour")
    p.add_argument("--no_kinematic_uncert", action="store_false",
                   help="Do not use SMPL Kinematic for uncert (same store_false semantics as the reference)")
    p.add_argument("--smooth", action="store_true", help="one-euro smoothing of each track (video mode)")
    p.add_argument("--min_cutoff", type=float, default=0.004)
    p.add_argument("--beta", type=float, default=1.5)
    p.add_argument("--tracking", type=str, default=None,
                   help="video mode: json or the reference's tracking_results_<method>.pkl {person_id: {'bbox': [[cx,cy,w,h],...], "
                        "'frames': [idx,...]}} (multi_person_tracker output) or {person_id: {'joints2d': [T,K,3] (x,y,confidence), "
                        "'frames': [idx,...]}} (a 2-D pose tracker's output: boxes are derived from the keypoints); default = one "
                        "centred track over all frames")
    p.add_argument("--tracking_method", default="bbox", choices=["bbox", "pose"],
                   help="video mode: as the reference's flag.  The --tracking file's content decides how each track is read; "
                        "pose = a track without joints2d is an error")
    p.add_argument("--kp_vis_thresh", type=float, default=0.3,
                   help="keypoint tracks: the confidence above which a keypoint counts for the box (and is drawn by --draw_keypoints)")
    p.add_argument("--smooth_bbox", action="store_true",
                   help="keypoint tracks: median (11) + Gaussian (sigma 8) filter of the derived box parameters (cx, cy, scale)")
    p.add_argument("--skip_frame", type=int, default=1)
    p.add_argument("--occlusion_map", action="store_true",
                   help="folder mode: per detection, slide a grey square over the crop, regress every occluded copy on the GPU and "
                        "write <out>/occlusion/<image>_<det>.png (the heat map over the crop, through --image_format / --encode) "
                        "and .npz (records [nh,nw,77], positions, patch, stride, the unoccluded var_pose and pred_cam)")
    p.add_argument("--occ_patch", type=int, default=40, help="--occlusion_map: side of the square, 1..224 pixels of the crop")
    p.add_argument("--occ_stride", type=int, default=10, help="--occlusion_map: step of the square, >= 1")
    p.add_argument("--occ_fill", type=float, default=None,
                   help="--occlusion_map: grey level 0..255 of the square (default: the dataset mean colour, 0 after normalisation)")
    p.add_argument("--occ_metric", type=str, default="v2v",
                   help="--occlusion_map: what the heat map shows: v2v = mean vertex displacement, var = mean change of the "
                        "per-joint uncertainty, joints = mean displacement of the 49 joints, var:<0..23> = one joint's uncertainty")
    p.add_argument("--occ_scale", type=str, default="auto",
                   help="--occlusion_map: the value drawn as the hottest colour: auto = the map's maximum, or a positive float")
    p.add_argument("--save_dataset", type=str, default=None, metavar="FILE.npz",
                   help="also write the predictions as a pseudo-ground-truth dataset in the reference's format (imgname, center, "
                        "scale, pose [N,72] axis-angle, shape, var, has_smpl, part, openpose, S, person_id; every array has N rows), "
                        "made on the GPU from the regressor's RAW outputs: in video mode --smooth does not touch it (smoothing is "
                        "presentation, labels are what the model said).  eval.py --dataset reads it; the reference's BaseDataset "
                        "filters it by its own UNCERT_THRESHOLD.  Folder mode: imgname = file name, person_id = detection index; "
                        "video mode: imgname = frame file name (<video stem>/<frame index> for an .avi), person_id = track id")
    p.add_argument("--uncert_threshold", type=float, default=None,
                   help="with --save_dataset: keep only the confident crops, selected as the reference's get_confident_frames "
                        "selects (kinematic accumulation, then var[:, 0] < T); default: every crop")
    p.add_argument("--save_segm", action="store_true",
                   help="folder mode, PARE variants: per detection write <out>/segm/<image>_<det>.png, two 224 x 224 panels made on the "
                        "GPU: the crop under the coloured argmax of pred_segm_mask, and under the body parts of the predicted mesh "
                        "(needs `faces` in the --smpl file; --encode gpu compresses the pictures on the GPU too)")
    p.add_argument("--part_mapping", type=str, default=None,
                   help="with --save_segm: the vertex -> part table as .npy / .npz / the reference's smpl_partSegmentation_mapping.pkl "
                        "(default: each vertex's largest skinning weight)")
    p.add_argument("--infill", type=float, default=None, metavar="THRESH",
                   help="video mode: replace every joint rotation whose uncertainty (the result's `var`) exceeds THRESH by the "
                        "shortest-arc interpolation between the track's nearest confident frames on either side (made on the GPU, "
                        "before --smooth); the result gains infill, pose_net, betas_net and orig_cam_net")
    p.add_argument("--infill_max_gap", type=int, default=30,
                   help="--infill: the most frames between the two confident frames of an interpolation (one second at the default "
                        "--fps); a single confident frame is held for at most half of it")
    p.add_argument("--cfg2", type=str, default=None,
                   help="a second model's config: with --ckpt2, both engines regress every crop on the one GPU and the per-joint "
                        "uncertainty decides whose result is written (poco_amd/select.py); the result gains select and select_score")
    p.add_argument("--ckpt2", type=str, default=None, help="the second model's checkpoint (needs --cfg2)")
    p.add_argument("--inf_model2", type=str, default="best", help="--inf_model of the second model")
    p.add_argument("--select", default=None, choices=["crop", "joint"],
                   help="with --cfg2 --ckpt2: crop (default) = each crop from the model with the lower global uncertainty; joint = "
                        "each joint rotation from the model with the lower uncertainty of that joint, shape and camera from the "
                        "root's model, mixed rows re-posed")
    p.add_argument("--select_scale", type=float, default=None,
                   help="with --cfg2 --ckpt2: multiplies the second model's uncertainty before the comparison (default 1.0)")
    p.add_argument("--tta", type=str, default=None, metavar="VIEWS",
                   help="folder mode: test-time augmentation: comma-separated views, each a '+'-joined set of flip, rot:<degrees>, "
                        "scale:<factor> (at most 8 with the untransformed crop, which is always there); every view is cut with the "
                        "dataset crop, all go through one forward and are fused per joint on the GPU; the result gains tta_spread; a forward "
                        "takes the views of max(1, batch_size // K) crops, so with --batch_size below the K views the engine is built for "
                        "a batch of K")
    p.add_argument("--tta_weight", default=None, choices=["uncert", "uniform"],
                   help="with --tta: weigh each view's joint by 1 / its uncertainty (default) or uniformly")
    p.add_argument("--smooth_uncert", type=float, default=None, metavar="LAMBDA",
                   help="video mode: smooth every track over time, weighting each frame's joint rotation by the model's own "
                        "precision (made on the GPU, after --infill); LAMBDA in (0, 1e4] is the stiffness; the result gains "
                        "smooth_shift, pose_net, betas_net and orig_cam_net")
    p.add_argument("--smooth_uncert_ref", type=float, default=0.3,
                   help="--smooth_uncert: the uncertainty (`var`) at which a frame's weight is 1")
    p.add_argument("--smooth_uncert_max_gap", type=int, default=30,
                   help="--smooth_uncert: curvature is not penalised across a hole of more than this many frames")
    p.add_argument("--kp_refit", type=float, default=None, metavar="LAMBDA",
                   help="video mode, keypoint tracks: refit every frame's joint rotations and camera to the track's BODY_25 keypoints "
                        "(made on the GPU, before --infill and the smoothers); LAMBDA > 0 weighs the prior, the network's own pose, each "
                        "joint by its precision; the result gains refit_shift, refit_cost, refit_flag, pose_net, betas_net and "
                        "orig_cam_net")
    p.add_argument("--kp_refit_ref", type=float, default=0.3, help="--kp_refit: the uncertainty (`var`) at which a joint's prior weight is LAMBDA")
    p.add_argument("--kp_refit_rho", type=float, default=0.1,
                   help="--kp_refit: width of the Geman-McClure robustifier in fractions of the box side (<= 0: plain least squares)")
    p.add_argument("--kp_refit_iters", type=int, default=10, help="--kp_refit: Levenberg-Marquardt steps per frame, 1..32")
    p.add_argument("--save_obj", action="store_true", help="save results as .obj files (meshes/<image|person>/<idx>.obj)")
    p.add_argument("--detections", type=str, default=None,
                   help="json {image name: [[cx,cy,w,h],...]} or the reference's detection_results.pkl (per-image list)")
    p.add_argument("--calibration", type=str, default=None, metavar="FILE",
                   help="a calibration file written by eval.py --calibrate: the final `var` of every person is mapped to the error "
                        "observed on that dataset (one call on the GPU, after the uncertainty post-processing and every flag that changes "
                        "`var`); the result gains err_pose [n,24] (per joint, the evaluator's pose distance) and err_mpjpe, err_pampjpe, "
                        "err_v2v [n] (metres); the file's kinematic flag and head must be this run's")
    p.add_argument("--tracker", default="none", choices=["none", "sort"],
                   help="video mode: sort = build the tracks from the per-frame person boxes of --detections on the GPU (SORT: a "
                        "Kalman filter per person, one optimal IoU assignment per frame; at most 64 people per frame) instead of "
                        "reading them from --tracking; <out>/tracking_results_sort.json is written for a later --tracking run")
    p.add_argument("--track_iou", type=float, default=0.3, help="--tracker sort: the least IoU of a detection with a predicted box, in (0, 1)")
    p.add_argument("--track_max_age", type=int, default=1, help="--tracker sort: frames a person may go undetected before the track ends")
    p.add_argument("--track_min_hits", type=int, default=3,
                   help="--tracker sort: consecutive detections before a person who enters after the first frames is reported")
    p.add_argument("--track_boxes", default="detection", choices=["detection", "filtered"],
                   help="--tracker sort: crop with the file's own boxes (default: what folder mode cuts) or with the Kalman filter's")
    p.add_argument("--track_backfill", action="store_true",
                   help="--tracker sort: a reported person's track also takes the frames before --track_min_hits was reached")
    p.add_argument("--track_stitch", action="store_true",
                   help="video mode: after the forward, join the tracks an occlusion broke into chains - by the regressed body shape "
                        "(weighted by the model's own uncertainty) and the extrapolated motion of the boxes, one optimal assignment "
                        "on the GPU - run the frames of the holes through the forward with interpolated boxes, and hand the chains to "
                        "--infill / --smooth_uncert / --smooth as single tracks; the result gains stitch and stitch_frag, "
                        "<out>/tracking_results_stitched.json is written for a later --tracking run")
    p.add_argument("--stitch_max_gap", type=int, default=30,
                   help="--track_stitch: the most missing frames between two joined tracks (the default of --infill_max_gap)")
    p.add_argument("--stitch_fit_len", type=int, default=8,
                   help="--track_stitch: the rows at a track's end and start through which its motion is fitted, 1..32")
    p.add_argument("--stitch_motion_tol", type=float, default=0.5,
                   help="--track_stitch: the largest mismatch of the two extrapolated boxes, in body heights per square root of the "
                        "frames apart; the default is a guess that nobody has measured on real video")
    p.add_argument("--stitch_shape_tol", type=float, default=1.0,
                   help="--track_stitch: the largest distance of the two mean shapes in units of their pooled spread (with a floor of "
                        "0.05 per beta); the default and the floor are guesses that nobody has measured on real video")
    p.add_argument("--stitch_shape", type=float, default=1.0,
                   help="--track_stitch: the weight of the shape term against the motion term; 0 switches the shape term off")
    p.add_argument("--stitch_min_frag", type=int, default=5,
                   help="--track_stitch: tracks of at least this many frames reach the forward (instead of 25); the 25-frame rule is "
                        "applied to the chains")
    p.add_argument("--stitch_no_fill", action="store_true", help="--track_stitch: join the ids and leave the holes")
    p.add_argument("--gpus", type=int, default=1,
                   help="video mode: one process per GPU, whole tracks sharded across the ranks, ONE all-gather of the "
                        "packed SMPL records (RCCL over xGMI); `demo.py --gpus N` starts the N ranks itself")
    p.add_argument("--dist_backend", default="nccl", choices=["nccl", "gloo"],
                   help="nccl = RCCL (one GPU per rank); gloo only to exercise the multi-rank path on fewer devices")
    p.add_argument("--smpl", type=str, default="data/smpl/SMPL_NEUTRAL.npz",
                   help="SMPL body model as .npz (tools/convert_smpl.py converts the licensed .pkl)")
    return p.parse_args(argv)


def render_enabled(args) -> bool:
    """--render is opt-in; --no_render keeps its meaning and wins."""
    return bool(getattr(args, "render", False)) and not getattr(args, "no_render", False)


def _check_render_assets(args) -> None:
    """--render draws the body model's triangles: refuse a --smpl file without `faces` before any GPU work."""
    import numpy as np
    if not (isinstance(args.smpl, str) and os.path.isfile(args.smpl)):
        sys.exit(f"--render: body-model file not found: {args.smpl}")
    with np.load(args.smpl) as z:
        if "faces" not in z.files:
            sys.exit(f"--render: {args.smpl} has no `faces` array (convert the SMPL .pkl with tools/convert_smpl.py, which "
                     "keeps its triangles)")


def _check_occlusion(args) -> None:
    """--occlusion_map: refuse video mode and out-of-range options before the engine is built."""
    if not getattr(args, "occlusion_map", False):
        return
    if args.mode not in ("folder", "directory"):
        sys.exit("--occlusion_map sweeps the crops of folder mode: it needs --mode folder")
    if not 1 <= args.occ_patch <= 224:
        sys.exit(f"--occ_patch must be in 1..224, got {args.occ_patch}")
    if args.occ_stride < 1:
        sys.exit(f"--occ_stride must be >= 1, got {args.occ_stride}")
    if args.occ_fill is not None and not 0 <= args.occ_fill <= 255:
        sys.exit(f"--occ_fill must be in 0..255, got {args.occ_fill}")
    m = args.occ_metric
    if not (m in ("v2v", "var", "joints") or (m.startswith("var:") and m[4:].isdigit() and 0 <= int(m[4:]) <= 23)):
        sys.exit(f"--occ_metric must be v2v, var, joints or var:<0..23>, got {m}")
    if args.occ_scale != "auto":
        try:
            v = float(args.occ_scale)
        except ValueError:
            v = float("nan")
        if not 0 < v < float("inf"):
            sys.exit(f"--occ_scale must be auto or a positive number, got {args.occ_scale}")


def _check_dataset(args) -> None:
    """--save_dataset / --uncert_threshold: refuse combinations that cannot work before the engine is built."""
    path = getattr(args, "save_dataset", None)
    thr = getattr(args, "uncert_threshold", None)
    if thr is not None and not path:
        sys.exit("--uncert_threshold selects the crops of --save_dataset: it needs --save_dataset FILE.npz")
    if thr is not None and not thr == thr:
        sys.exit("--uncert_threshold must be a number")
    if path and args.gpus > 1:
        sys.exit("--save_dataset with --gpus N > 1 is not supported: each rank keeps its records on its own device, and gathering "
                 "them across the ranks in source order is a later change; run with --gpus 1")


def _check_infill(args) -> None:
    """--infill / --infill_max_gap: refuse them outside video mode and with --gpus N > 1 before the engine is built."""
    thr = getattr(args, "infill", None)
    gap = getattr(args, "infill_max_gap", 30)
    if thr is None:
        if gap != 30:
            sys.exit("--infill_max_gap bounds the gaps --infill bridges: it needs --infill THRESH")
        return
    if args.mode != "video":
        sys.exit("--infill repairs the tracks of video mode: it needs --mode video")
    if args.gpus > 1:
        sys.exit("--infill with --gpus N > 1 is not supported: the packed record the ranks exchange has no room for the in-fill "
                 "flags; run with --gpus 1")
    if not thr == thr:
        sys.exit("--infill must be a number")
    if gap < 1:
        sys.exit(f"--infill_max_gap must be >= 1, got {gap}")


def _check_select(args) -> None:
    """--cfg2 / --ckpt2 / --select / --select_scale: refuse what cannot work before an engine is built."""
    from poco_amd.select import flag_error
    msg = flag_error(args, ("occlusion_map", "save_dataset", "save_segm"))
    if msg:
        sys.exit(msg)


def _check_tta(args) -> None:
    """--tta / --tta_weight: refuse what cannot work before an engine is built."""
    from poco_amd.tta import flag_error
    msg = flag_error(args, "demo")
    if msg:
        sys.exit(msg)


def _check_smooth_uncert(args) -> None:
    """--smooth_uncert and its two companions: refuse them outside video mode, with --smooth and with --gpus N > 1 before the engine
    is built."""
    lam = getattr(args, "smooth_uncert", None)
    ref, gap = getattr(args, "smooth_uncert_ref", 0.3), getattr(args, "smooth_uncert_max_gap", 30)
    if lam is None:
        if ref != 0.3 or gap != 30:
            sys.exit("--smooth_uncert_ref and --smooth_uncert_max_gap tune --smooth_uncert: they need --smooth_uncert LAMBDA")
        return
    if args.mode != "video":
        sys.exit("--smooth_uncert smooths the tracks of video mode: it needs --mode video")
    if getattr(args, "smooth", False):
        sys.exit("--smooth_uncert with --smooth: two smoothers; choose one")
    if args.gpus > 1:
        sys.exit("--smooth_uncert with --gpus N > 1 is not supported: the packed record the ranks exchange has no room for the "
                 "shifts; run with --gpus 1")
    if not 0.0 < lam <= 1e4:
        sys.exit(f"--smooth_uncert LAMBDA must be in (0, 1e4], got {lam}")
    if not (ref > 0.0 and ref < float("inf")):
        sys.exit(f"--smooth_uncert_ref must be finite and > 0, got {ref}")
    if gap < 1:
        sys.exit(f"--smooth_uncert_max_gap must be >= 1, got {gap}")


def _check_kp_refit(args) -> None:
    """--kp_refit and its three companions: refuse what cannot work before the engine is built."""
    from poco_amd.refit import flag_error
    msg = flag_error(args, "demo")
    if msg:
        sys.exit(msg)


def _check_tracker(args) -> None:
    """--tracker and its --track_* companions: refuse what cannot work before the engine is built."""
    from poco_amd.sort import flag_error
    msg = flag_error(args)
    if msg:
        sys.exit(msg)


def _check_stitch(args) -> None:
    """--track_stitch and its --stitch_* companions: refuse what cannot work before the engine is built."""
    from poco_amd.stitch import flag_error
    msg = flag_error(args)
    if msg:
        sys.exit(msg)


def _check_calibration(args) -> None:
    """--calibration: refuse --cfg2, an unreadable file and a file fitted for another head or kinematic flag before the engine is
    built."""
    from poco_amd import calibrate
    msg = calibrate.demo_flag_error(args)
    if msg:
        sys.exit(msg)
    if not getattr(args, "calibration", None):
        return
    from poco_amd.config import update_hparams
    try:
        calibrate.check_file(args.calibration, bool(getattr(args, "no_kinematic_uncert", True)), str(update_hparams(args.cfg).POCO.BACKBONE))
    except (OSError, ValueError) as e:
        sys.exit(f"--calibration: {e}")


def _build_sort_tracks(args, folder: str, out_dir: str):
    """--tracker sort: the tracks from --detections, and <out>/tracking_results_sort.json (rank 0 writes it)."""
    from poco_amd import sort
    from poco_amd.tester import load_detections
    try:
        names = sort.frame_names(folder)
        min_frames = args.stitch_min_frag if getattr(args, "track_stitch", False) else sort.MIN_NUM_FRAMES
        tracks = sort.build_tracks(load_detections(args.detections), names, iou_thresh=args.track_iou, max_age=args.track_max_age,
                                   min_hits=args.track_min_hits, boxes=args.track_boxes, backfill=args.track_backfill,
                                   min_frames=min_frames)
    except ValueError as e:
        sys.exit(str(e))
    if not tracks:
        sys.exit(f"--tracker sort: no track of at least {min_frames} frames in {args.detections}")
    if int(os.environ.get("RANK", "0")) == 0:
        os.makedirs(out_dir, exist_ok=True)
        sort.write_tracking(os.path.join(out_dir, "tracking_results_sort.json"), tracks)
    return tracks


def _check_segm(args) -> None:
    """--save_segm: refuse video mode, a head without a segmentation mask, a body model without triangles and an unreadable
    --part_mapping before the engine is built."""
    if not getattr(args, "save_segm", False):
        return
    from poco_amd import segm
    from poco_amd.config import update_hparams
    try:
        segm.check_demo_inputs(args, update_hparams(args.cfg).POCO.BACKBONE)
        if getattr(args, "part_mapping", None):
            segm.load_part_mapping(args.part_mapping)
    except ValueError as e:
        sys.exit(str(e))


def _spawn_ranks(args) -> int:
    """`demo.py --gpus N` without a launcher: re-execute under torch.distributed.run, one rank per GPU."""
    import socket
    import subprocess
    import torch
    if args.dist_backend == "nccl" and torch.cuda.device_count() < args.gpus:
        sys.exit(f"demo.py --gpus {args.gpus}: only {torch.cuda.device_count()} GPU(s) visible; RCCL needs one per rank")
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}",
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    return subprocess.call(cmd, env=dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0"))


def main(args):
    if args.mode in ("webcam",):
        sys.exit("webcam mode needs a capture device + renderer: out of scope")
    if render_enabled(args):
        _check_render_assets(args)
    if not 1 <= getattr(args, "jpeg_quality", 90) <= 100:
        sys.exit(f"--jpeg_quality must be in 1..100, got {args.jpeg_quality}")
    if getattr(args, "save_video", False) and not (args.mode == "video" and render_enabled(args)):
        sys.exit("--save_video writes the rendered frames of video mode: it needs --mode video and --render")
    _check_select(args)
    _check_tta(args)
    _check_occlusion(args)
    _check_dataset(args)
    _check_segm(args)
    _check_infill(args)
    _check_smooth_uncert(args)
    _check_tracker(args)
    _check_stitch(args)
    _check_kp_refit(args)
    _check_calibration(args)
    if args.gpus > 1:
        if args.mode != "video":
            sys.exit("--gpus N shards whole tracks: video mode only (folder mode images are independent - run N demos)")
        if "WORLD_SIZE" not in os.environ:
            sys.exit(_spawn_ranks(args))
        import torch
        import torch.distributed as dist
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        if args.dist_backend == "nccl":
            dev = torch.device("cuda", int(os.environ["LOCAL_RANK"]))
            torch.cuda.set_device(dev)
            dist.init_process_group("nccl", device_id=dev)
        else:
            dist.init_process_group("gloo")
    from poco_amd.tester import POCOTester, load_detections, load_tracking, tracking_options
    folder = args.image_folder if args.mode in ("folder", "directory") else args.vid_file
    stem = os.path.basename(os.path.normpath(folder)) if folder else ""
    if args.mode == "video" and folder and os.path.isfile(folder):
        from poco_amd.jpeg import MjpegReader
        try:                                                              # a video file: only Motion-JPEG AVI is read
            MjpegReader(folder).close()
        except ValueError as e:
            sys.exit(f"--vid_file: {e}")
        stem = os.path.splitext(stem)[0]
    elif not folder or not os.path.isdir(folder):
        sys.exit(f"input folder not found: {folder}")
    tracking = args.tracking
    stitching = bool(getattr(args, "track_stitch", False))
    if args.mode == "video" and tracking:                               # read before the engine is built: a bad file ends here
        try:
            tracking = load_tracking(tracking, **tracking_options(args), **({"min_frames": args.stitch_min_frag} if stitching else {}))
        except ValueError as e:
            sys.exit(str(e))
    if stitching:                                                         # gap rows have no keypoints: a keypoint track ends here
        from poco_amd.stitch import tracking_error as stitch_tracking_error
        msg = stitch_tracking_error(tracking)
        if msg:
            sys.exit(msg)
    if getattr(args, "kp_refit", None) is not None:                       # every track needs BODY_25 keypoints: a box track ends here
        from poco_amd.refit import tracking_error
        msg = tracking_error(tracking)
        if msg:
            sys.exit(msg)
    out_dir = os.path.join(args.output_folder, stem + "_")
    if args.mode == "video" and getattr(args, "tracker", "none") == "sort":
        tracking = _build_sort_tracks(args, folder, out_dir)
    tester = POCOTester(args)
    if args.mode == "video":
        stats = tester.run_on_video_folder(folder, tracking, out_dir)
    else:
        dets = load_detections(args.detections)
        stats = tester.run_on_image_folder(folder, dets, out_dir)
        if getattr(args, "save_segm", False):
            from poco_amd import segm
            stats["segm_pictures"] = segm.write_segm_pictures(tester, folder, dets, out_dir)
    if "fps" in stats:                                                    # rank 0 (the reference logs 'poco FPS', demo.py:136-145)
        print(json.dumps({"poco_fps": round(stats["fps"], 2), **stats}))
    if args.gpus > 1:
        import torch.distributed as dist
        dist.destroy_process_group()


if __name__ == "__main__":
    main(parse_args())
