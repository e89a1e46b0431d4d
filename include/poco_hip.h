/* poco_hip.h — C ABI of libpoco_hip.so, the MI355X (gfx950) implementation of POCO's per-crop
 * SMPL regressor hot path.
 *
 * The reference (saidwivedi/POCO) has no FFI/plugin interface: its seam is the Python call
 * `output = self.model(batch)` on an nn.Module (pocolib/core/tester.py:213,408;
 * pocolib/models/poco.py:99-129).  This header is therefore the boundary a binding for that call
 * site uses; every entry point names the reference code it replaces.  Plain C types only: device
 * and host pointers, sizes, a hipStream_t passed as void*.  No torch types.
 *
 * Conventions
 *   - all functions return 0 (POCO_OK) or a positive error code; poco_last_error() returns the
 *     message of the last failure on the calling thread.  Nothing throws across the ABI.
 *   - "d_" pointers are device (HBM) pointers owned by the caller, "h_" pointers are host memory.
 *   - activations handed to the stand-alone conv operators are fp32 in the library's internal layout "L16"
 *     (channel-slice-major NHWC): [B][H][C/16][W][16], i.e. element (b,y,x,c) at
 *     ((b*H + y)*(C/16) + c/16)*W*16 + x*16 + c%16; for H = W = 1 this is plain [B][C].
 *     poco_forward itself takes the reference's NCHW image batch and returns the reference's tensors.
 *   - `stream` is a hipStream_t (NULL = default stream).  Operators enqueue on it; the
 *     poco_op_* test entry points additionally synchronise it before returning.
 */
#ifndef POCO_HIP_H
#define POCO_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Message of the last error on this thread ("" if none). */
const char* poco_last_error(void);

/* Version of this ABI: bumped whenever a struct layout or the meaning / type of an argument of an existing entry point changes
 * (2: poco_crop_normalize takes bbox_scale as double; 3: poco_outputs_t gained `record`, poco_create_ex, poco_crop_normalize_multi,
 * RealNVP scratch planned at finalize; 4: poco_inputs_t / poco_outputs_t start with `struct_size`, see below).  A binding
 * compiled against another header must refuse to run:
 *     if (poco_abi_version() != POCO_ABI_VERSION) fail;                                                                          */
#define POCO_ABI_VERSION 4
int poco_abi_version(void);

/* ---- the engine: POCO(backbone=..., pretrained=ckpt) + model(batch) ---------------------------
 * replaces pocolib/models/poco.py:13-154 (ctor :13-97, forward :99-129, load_pretrained :131-154)
 * as called from pocolib/core/tester.py:75-98 (build) and :213,:408 (output = self.model(batch)). */

typedef struct poco_engine* poco_handle_t;

/* Both I/O structs are SELF-DESCRIBING (ABI 4): the first member is the size in bytes of the struct the CALLER compiled or
 * declared (`x.struct_size = sizeof x;`).  The library reads exactly that many bytes:
 *   - members beyond `struct_size` (added by a later header) read as NULL = "not wanted / not given";
 *   - a `struct_size` that is 0, not a multiple of 8, smaller than the size word plus one pointer, or larger than 4096 is
 *     POCO_ERR_ARG (that is what a struct written from an older header - whose first member is a pointer - or an
 *     uninitialised one looks like), and so is a non-NULL member beyond what THIS library knows;
 * so a binding whose field list is shorter than this header's can no longer make the engine read past its struct. */

/* batch dict of pocolib/core/tester.py:205-212 (device pointers, fp32).  bbox_info/focal_length/
 * scale/center/orig_shape are only read by the *-cliff variants (poco.py:102-111). */
typedef struct {
  uint64_t struct_size;      /* = sizeof(poco_inputs_t) as the caller sees it           */
  const float* img;          /* [B,3,224,224] NCHW, ImageNet-normalised crop            */
  const float* bbox_info;    /* [B,3]   image_utils.py:171-183                           */
  const float* focal_length; /* [B]     image_utils.py:185-187                           */
  const float* scale;        /* [B]     bbox size / 200                                  */
  const float* center;       /* [B,2]   bbox centre (x,y) in full-image pixels           */
  const float* orig_shape;   /* [B,2]   (img_h, img_w)                                   */
} poco_inputs_t;

/* output dict of POCO.forward.  Any pointer may be NULL = not wanted
 * (pred_cam_t / smpl_joints2d / pred_fullimg_cam_t are computed into scratch then). */
typedef struct {
  uint64_t struct_size;      /* = sizeof(poco_outputs_t) as the caller sees it          */
  float* pred_pose;          /* [B,24,3,3] rotation matrices                             */
  float* pred_pose6d;        /* [B,144]    ('pred_pose6d' pare / 'pred_pose_6d' cliff)   */
  float* pred_shape;         /* [B,10]                                                   */
  float* pred_cam;           /* [B,3]  weak-perspective (s,tx,ty)                        */
  float* pred_cam_t;         /* [B,3]  crop camera translation                           */
  float* pred_fullimg_cam_t; /* [B,3]  cliff only                                        */
  float* smpl_vertices;      /* [B,6890,3]                                               */
  float* smpl_joints3d;      /* [B,49,3]                                                 */
  float* smpl_joints2d;      /* [B,49,2]  pare: crop-normalised, cliff: full-image px    */
  float* var_pose;           /* [B,24]  per-joint uncertainty (poco_head.py:144-148)     */
  float* uncert_feat;        /* [B,3072] pare / [B,2048] cliff                           */
  float* pred_segm_mask;     /* [B,25,56,56] NCHW, pare only                             */
  float* body_feat2;         /* [B,1024] cliff only                                      */
  float* backbone_feat;      /* [B,480,56,56] NCHW, hrnet_w32 only: the backbone's output map  */
                             /* (hrnet.py:515-519), for parity checks; NULL in production      */
  float* record;             /* [B,254] packed per-crop record = the payload of the multi-GPU all-gather and of the streaming
                              * D2H copy: [pred_pose 216 | pred_shape 10 | pred_cam 3 | var_pose 24 (raw) | confidence 1], written
                              * by one kernel inside the forward (hipGraph-capturable).  confidence = the reference's
                              * post-processed scalar: kinematic accumulation along the SMPL tree (poco_utils.py:21-25), rows whose
                              * root exceeds the threshold set to 1, cliff: root value / pare: mean over joints (poco_utils.py:50-60),
                              * clipped to [0, 0.99] (tester.py:245).  Options record_kinematic / record_thr of poco_create_ex.  */
} poco_outputs_t;

/* variant = "<backbone>-<head>" exactly as POCO.BACKBONE in the yaml (poco.py:41):
 * "hrnet_w32-pare", "hrnet_w48_cls-cliff", "resnet50-cliff".  num_flow_layers = POCO.NUM_FLOW_LAYERS.
 * Host only (no GPU needed): builds the list of tensors the variant expects. */
int poco_create(const char* variant, int max_batch, int num_flow_layers, poco_handle_t* out);
/* The same with build options: "key=value,key=value" (NULL or "" = defaults = poco_create).  The library reads NO environment
 * variable; every alternative form is chosen here, computes the same model and is compared with the default in tests/:
 *   kcat, kmerge, chain, dual, wg_fuse = 0   the separate-launch form of a fused op group (csrc/engine.hip EngineOpts)
 *   dual_layout = <100 NI + 10 WM + WN>      ResNet-50's two-source shortcut GEMM: load schedule / waves per block (default 41; 0 = one-wave blocks)
 *   stem_mfma = 0                            the stem conv on the packed-FMA kernels instead of the MFMA implicit GEMM (csrc/stem_mfma.hip)
 *   mlp_fuse = 0, mlp_blocks = <1..256>      cliff head: the regressor chain as separate launches instead of the one persistent launch of
 *                                            csrc/mlp_chain.hip / the number of blocks of that launch (default 256)
 *   xdep, tail_lanes, up_lanes = 0           the more conservative lane schedules;  seq_phases = <bit mask>, branch_lanes = "0123"
 *   split_f16 = 1                            EXPERIMENT, only in libraries built with `python -m poco_amd.build --experiments` (an unknown
 *                                            key in the shipped one): plain 1x1 convs in split fp16
 *   w4_min_plane = <7..14>                   smallest plane the whole-position F(4x4) kernel (ALG 13) is prepared for (default 7; 14 = no fragments for the 7x7 planes)
 *   debug_wait_spins = <n>, debug_mlp_timeouts = <n>   TEST HOOKS for poco_status: poll bound of the in-kernel waits (default 2^21 polls,
 *                                            ~3 s) / the first n launches of the fused regressor time out on purpose
 *   flow_ctx_rows = <n>                      context rows poco_realnvp*'s scratch is planned for at finalize (default max_batch)
 *   record_kinematic = 0|1, record_thr = <f> post-processing of poco_outputs_t.record's confidence (defaults 1, 0.40)
 *   mask_params_id = <ids>, exclude_uncert_idx = <ids>   POCO.MASK_PARAMS_ID / POCO.EXCLUDE_UNCERT_IDX as the yaml spells them ("1-4-7";
 *                                            default "" as in the shipped configs): the forward does not read them, poco_flow_nll refuses
 *                                            an engine that has either (a masked flow also tolerates the flow_head.mask_params buffer)
 * Unknown keys are an error. */
int poco_create_ex(const char* variant, int max_batch, int num_flow_layers, const char* options, poco_handle_t* out);
void poco_destroy(poco_handle_t h);

/* Expected tensors: names are the reference state_dict keys after the prefix stripping of
 * pocolib/utils/train_utils.py:69-90 ("backbone.", "head.", "uncert_head.", "flow_head.") plus
 * "smpl." for the body model (smpl_head.py:40).  required=0: tolerated but unused by forward. */
int poco_num_tensors(poco_handle_t h);
int poco_tensor_info(poco_handle_t h, int i, char* name, size_t name_cap, int64_t* shape6, int* rank,
                     int* required);
/* Copy one tensor (host fp32) into the engine.  Strict: unknown names and wrong element counts are
 * errors (the reference's silent strict->non-strict fallback, train_utils.py:118-124, is not kept).
 * The body model's three index tables are range-checked here, because the SMPL kernels index with them unchecked:
 *   smpl.parents           for i >= 1 an integer with 0 <= parents[i] < i (a joint's parent comes before it); entry 0, the root's
 *                          marker (-1, or the 4294967295 of an SMPL pickle's uint32), is neither read nor checked
 *   smpl.joint_map         integers in [0, 54): 24 chain joints | 21 vertex picks | 9 regressed joints
 *   smpl.extra_vertex_ids  integers in [0, 6890)
 * A value that is not finite, not integral or out of its range is POCO_ERR_ARG; the message names the tensor, the index and the
 * value, and nothing is stored (a table loaded earlier under that name stays). */
int poco_load_tensor(poco_handle_t h, const char* name, const float* host_data, const int64_t* shape,
                     int rank);
/* BN folding, MFMA weight packing, upload, workspace planning + allocation.  Needs the GPU. */
int poco_finalize(poco_handle_t h);
/* Enqueue one forward pass for B <= max_batch crops on `stream`.  No allocation, no sync. */
int poco_forward(poco_handle_t h, int B, const poco_inputs_t* in, const poco_outputs_t* out, void* stream);

/* Deferred failures of the forwards enqueued since the last call.  poco_forward only ENQUEUES; two of its kernels contain bounded waits
 * (the grid barrier of the fused CLIFF regressor, csrc/mlp_chain.hip, and the partial hand-off of the stream-K 1x1 GEMM, ALG 14): one
 * that runs out ends its launch early - the queue stays alive, the outputs of that forward are invalid - and raises a word in pinned
 * host memory.  Call this AFTER synchronising the stream (or the event) the forward, or the hipGraph replay of it, was enqueued on and
 * BEFORE trusting its outputs:
 *   POCO_OK       nothing timed out;
 *   POCO_ERR_HIP  a wait timed out (poco_last_error says so).  The word is CLEARED and the device-side state re-armed: the next
 *                 poco_forward / graph replay runs normally.
 * Without this call the failure is still not silent for ever: the next poco_forward refuses to enqueue (POCO_ERR_HIP) until
 * poco_status has been asked - but the forward that failed has already returned POCO_OK, and a hipGraph replay never re-enters
 * poco_forward, so bindings must ask here (poco_amd/model.py POCO.check_status; tester.py and stream.py do before results are
 * written).  Cost on the good path: one read of host memory.  Replaces nothing in the reference (PyTorch raises from the
 * synchronising call); SURVEY.md 8(b): "int status codes, never throw". */
int poco_status(poco_handle_t h);

/* Independent branches of the network (HRNet branches, fuse terms, head branches) are enqueued on up
 * to 4 HIP streams forked from / joined to `stream` (default 4; 1 = everything on `stream`). */
int poco_set_num_lanes(poco_handle_t h, int n);

/* Introspection / tuning. */
int poco_num_ops(poco_handle_t h);
int poco_op_info(poco_handle_t h, int i, char* name, size_t name_cap, double* flops_per_crop, int* type);
/* Schedule of op i (available after poco_create, no GPU needed): sched[0] = phase (parallel region; regions are separated by joins of
 * all lanes), [1] = lane (HIP stream inside the region), [2] = bit mask of the lanes of the region this op additionally waits for
 * through events (everything enqueued on them before it), [3] = number of reads, then (activation id, first channel, end channel)
 * per read, then the number of writes and the same triples.  At most `cap` ints are written (cap >= 40 always suffices).  Lets a
 * test check, without a GPU, that no op reads channels another lane writes in the same region without waiting for it. */
int poco_op_sched(poco_handle_t h, int i, int* sched, int cap);
int poco_profile_ops(poco_handle_t h, int B, const poco_inputs_t* in, const poco_outputs_t* out, int iters,
                     float* ms_per_op, int cap, void* stream);
size_t poco_workspace_bytes(poco_handle_t h);
int poco_uncert_feat_dim(poco_handle_t h);
int poco_set_conv_cfg(poco_handle_t h, int op_index, int B, const int* cfg7);
int poco_get_conv_desc(poco_handle_t h, int op_index, int* desc8);
/* the tile configuration (7 ints, csrc/common.h) conv op `op_index` runs with at batch size B: the value set by
 * poco_set_conv_cfg or, without one, the built-in heuristic's choice. */
int poco_get_conv_cfg(poco_handle_t h, int op_index, int B, int* cfg7);

/* SMPL linear blend skinning with the engine's loaded body model: replaces
 * smplx.SMPL.forward(pose2rot=False) as wrapped by pocolib/models/head/smpl_head.py:22-34.
 * d_betas [B,10], d_rotmat [B,24,3,3] -> d_verts [B,6890,3], d_joints49 [B,49,3].
 * The rotations need not be orthonormal (smoothed and blended matrices are used as they are).  The kernels index with
 * smpl.parents, smpl.joint_map and smpl.extra_vertex_ids without a range check: poco_load_tensor has refused any table that
 * would index outside the 24 joints, the 54 joint sources or the 6890 vertices. */
int poco_smpl_lbs(poco_handle_t h, int B, const float* d_betas, const float* d_rotmat, float* d_verts,
                  float* d_joints49, void* stream);
/* RealNVP with the engine's flow_head.flow.* weights (pocolib/models/layers/real_nvp.py):
 * forward=0: log_prob(x[N,9] | ctx[N,512]) -> out[N]   (:55-65)
 * forward=1: forward_p(z[N,9], ctx)        -> out[N,9] (:25-38)
 * Two launches: one GEMM for the context part of the first Linear of all 2L s/t MLPs, one fp32-MFMA kernel for the coupling
 * recursion (csrc/kernels_flow.hip).  The GEMM's scratch is planned at poco_finalize for `flow_ctx_rows` context rows (option of
 * poco_create_ex; default max_batch = one context per crop): no allocation, no synchronisation here; more context rows than
 * planned is POCO_ERR_ARG. */
int poco_realnvp(poco_handle_t h, int N, const float* d_x, const float* d_ctx, float* d_out, int forward,
                 void* stream);
/* The same with the context as the reference's flow_head actually has it (pocolib/models/head/nf_head.py:93-110): one
 * 512-vector per CROP, used by `rep` consecutive rows (rep = 24 joints) - torch.repeat_interleave(context, rep) is never
 * materialised.  d_ctx [ceil(N/rep), 512]; row r uses d_ctx[r / rep].  rep = 1 is poco_realnvp. */
int poco_realnvp_rep(poco_handle_t h, int N, const float* d_x, const float* d_ctx, int rep, float* d_out, int forward,
                     void* stream);

/* ---- the flow likelihood of the ground truth: held-out NLL of eval.py --likelihood -------------------------------------------------
 * Replaces the training-time branch of flow_head.forward (pocolib/models/head/nf_head.py:78-123) and the loss line
 * pocolib/losses/losses.py:342-347 at evaluation time; csrc/eval_likelihood.hip.  The forward never runs any of this. */
/* context_feats = cond_layer(uncert_feat) (nf_head.py:82): d_uncert_feat [B, poco_uncert_feat_dim] -> d_ctx [B,512], on the engine's
 * small-M GEMM (csrc/linear_mfma.hip; it keeps its partial sums in LDS, so there is no scratch to plan).  flow_head.cond_layer.{weight,
 * bias} stay required=0 and are uploaded at poco_finalize when the checkpoint has them; without them this is POCO_ERR_STATE naming
 * the missing tensor.  A null pointer, B < 1 or B > max_batch is POCO_ERR_ARG.  Enqueued on `stream`: no allocation, no synchronisation. */
int poco_flow_context(poco_handle_t h, int B, const float* d_uncert_feat, float* d_ctx, void* stream);
/* Per crop: bar = |pred_pose - batch_rodrigues(gt_pose)| / (var_pose + 1e-9) (nf_head.py:89-101; sigma repeated over the 3x3; R_gt by
 * the device function of poco_op_rodrigues), log_phi = flow.log_prob(bar.reshape(-1, 9), context repeated over the 24 joints)
 * (nf_head.py:105-112), log sigma = log(var_pose) (losses.py:346).  d_pred_pose [B,24,3,3], d_gt_pose [B,72] axis-angle, d_var_pose
 * [B,24], d_ctx [B,512] (poco_flow_context), d_valid [B] int32 = has_smpl (NULL: every crop), d_out [B, POCO_FLOW_NLL_RECORD_FLOATS]:
 *     [0] valid (1 or 0)  [1] sum over the 24 joints of (log sigma - log phi), in joint order, fp64, stored as fp32  [2..8) 0
 *     [8..32) log phi  [32..56) log sigma  [56..80) mean over the 3x3 of bar
 * The record of an invalid crop is all zero (the reference drops such crops, nf_head.py:88-95).  Three launches on `stream` -
 * residual rows, the two launches of poco_realnvp_rep with rep = 24, epilogue - into scratch planned at poco_finalize for max_batch
 * crops: no allocation, no synchronisation, no host round trip.  POCO_ERR_ARG before any GPU work: a null handle or pointer, B < 1,
 * B > max_batch (or more crops than option flow_ctx_rows planned the flow scratch for), and an engine created with mask_params_id
 * or exclude_uncert_idx (nf_head.py:54-59,90-91,117-118: refused, not approximated). */
#define POCO_FLOW_NLL_RECORD_FLOATS 80
int poco_flow_nll(poco_handle_t h, int B, const float* d_pred_pose, const float* d_gt_pose, const float* d_var_pose,
                  const float* d_ctx, const int32_t* d_valid, float* d_out, void* stream);
/* Reduce N records (device, any number of poco_flow_nll calls laid end to end) in one block, fp64, fixed order, into h_summary4 (host):
 *     [0] valid crops  [1] mean log phi  [2] mean log sigma  [3] loss_nf = mean over valid crops x 24 joints of (log sigma - log phi)
 * = losses.py:346 with nf_loss_weight = 1.  No valid crop: [0] = 0 and NaN means.  Synchronises `stream`.  N < 1 or N > 2^24 is POCO_ERR_ARG. */
int poco_flow_nll_reduce(poco_handle_t h, int64_t N, const float* d_records, double* h_summary4, void* stream);

/* ---- stand-alone operators (parity tests, tuner, micro-benchmarks) -------------------------- */

/* conv(ks x ks, stride, pad=(ks-1)/2, no groups/dilation) * scale[co] + shift[co] (+ residual) (ReLU)
 * == nn.Conv2d -> nn.BatchNorm2d(eval) [-> "+= residual"] [-> ReLU] of
 * pocolib/models/backbone/hrnet.py:42-58,79-99 / hrnet_cls.py / resnet.py:101-121.
 * d_in  [B,H,Cin/16,W,16] (L16), h_weight [Cout,Cin,ks,ks] (host, torch OIHW order),
 * h_scale/h_shift [Cout] (host, nullable), d_res / d_out [B,Ho,Cout/16,Wo,16] (L16; d_res nullable).
 * Cin and Cout must be multiples of 16.  cfg = 7 ints {MT,NT,WM,WN,R,NI,ALG} (csrc/common.h) or NULL for the
 * heuristic. */
int poco_op_conv2d(const float* d_in, int B, int H, int W, int Cin, const float* h_weight,
                   const float* h_scale, const float* h_shift, int Cout, int ks, int stride,
                   const float* d_res, int relu, float* d_out, const int* cfg7, void* stream);

/* The same conv on VIEWS, with every epilogue form - the operand form the engine uses: each activation is the channel slice
 * [co, co + width) of a wider L16 buffer with `cs` channels per pixel (concat buffers, merged-conv outputs read in place).
 * poco_op_conv2d is the dense special case (in_cs = Cin, res_cs = out_cs = Cout, offsets 0, act = relu).
 *   d_in  = base of a buffer [B,H,in_cs/16,W,16], the conv reads channels [in_co, in_co + Cin);
 *   d_res = base of [B,Ho,res_cs/16,Wo,16] (nullable), channels [res_co, res_co + Cout);
 *   d_out = base of [B,Ho,out_cs/16,Wo,16], the conv writes channels [out_co, out_co + Cout) and nothing else.
 *   act: 0 none, 1 ReLU, 2 sigmoid, 3 ReLU on the output channels >= relu_from only (several convs of one input merged along
 *   Cout, the members without a ReLU first: csrc/engine.hip conv_multi); relu_from a multiple of 16 in [0, Cout].
 *   res_after_act: 1 = the residual is added after the activation instead of before it ("out += residual; relu",
 *   hrnet.py:42-58, is the 0 form).
 * The entry adds the channel offsets to the pointers as the engine does (csrc/common.h l16_chan_off) and fills the descriptor
 * with the buffers' strides.  Before any GPU work, POCO_ERR_ARG with a message for: a null d_in / h_weight / d_out; act outside
 * 0..3; a bad relu_from; a stride smaller than offset + width; strides / offsets that are no multiples of 16 (planes: an L16
 * slice) or of 4 (H = W = 1 rows, the regressor's state vector; ALG 11 needs 16 there too).  A form the chosen ALG refuses
 * (the Winograd kernels: act 2 and 3) is POCO_ERR_ARG from the launcher.  Synchronises `stream`. */
int poco_op_conv2d_ex(const float* d_in, int B, int H, int W, int Cin, int in_cs, int in_co, const float* h_weight,
                      const float* h_scale, const float* h_shift, int Cout, int ks, int stride, const float* d_res,
                      int res_cs, int res_co, int act, int relu_from, int res_after_act, float* d_out, int out_cs,
                      int out_co, const int* cfg7, void* stream);

/* ---- backbone side kernels and fused launches on their own (parity tests) ---------------------------------------------------
 * All activations L16; a device pointer is at the FIRST CHANNEL of its slice, `*_cs` = channels per pixel of the buffer it lies
 * in (a multiple of 16, >= the slice width).  Host weights are OIHW with per-channel scale / shift (nullable: 1 / 0), folded and
 * packed exactly as the engine's builder does.  Argument errors are POCO_ERR_ARG before any GPU work; each entry synchronises
 * `stream` before it returns. */
/* Tail of one Bottleneck chained with the head of the next, planes = 64 (hrnet.py:79-99, resnet.py:101-121):
 *   y = ReLU(bn3(conv3(t)) + res)  [.,256],   u = ReLU(bn1(conv1(y)))  [.,64];   t [B,H,W,64], res [B,H,W,256].
 * h_w3 [256,64,1,1], h_w1 [64,256,1,1]. */
int poco_op_bneck_chain(const float* d_t, int t_cs, const float* d_res, int res_cs, float* d_y, int y_cs, float* d_u,
                        int u_cs, const float* h_w3, const float* h_scale3, const float* h_shift3, const float* h_w1,
                        const float* h_scale1, const float* h_shift1, int B, int H, int W, void* stream);
/* 16-pixel sub-tiles the persistent grid of poco_op_bneck_chain holds at once: with more, its waves walk several. */
int poco_op_bneck_chain_resident_tiles(void);
/* Projection-shortcut Bottleneck tail as one GEMM over two sources (resnet.py:101-121, layer2-4 .0):
 *   out = act( bn3(conv3(a)) + bn_d(conv_d(b)) ),  conv_d = 1x1 at stride2 (1|2): b is sampled at (stride2 y, stride2 x).
 * a [B,Ho,Wo,Ca], b [B,H2,W2,Cb], out [B,Ho,Wo,Cout], Cout a multiple of 64; h_wa [Cout,Ca,1,1], h_wb [Cout,Cb,1,1].
 * wave_layout = 100 NI + 10 WM + WN (0 = the default: one wave per block), WM WN <= 8, NI (load schedule) in {0,1,3,4,5,6};
 * any other value is POCO_ERR_ARG.  act 0 | 1. */
int poco_op_conv1x1_dual(const float* d_a, int a_cs, int Ca, const float* d_b, int b_cs, int Cb, int H2, int W2,
                         int stride2, const float* h_wa, const float* h_scale_a, const float* h_shift_a,
                         const float* h_wb, const float* h_scale_b, const float* h_shift_b, float* d_out, int out_cs,
                         int Cout, int B, int Ho, int Wo, int act, int wave_layout, void* stream);
/* HRNet fuse (hrnet.py:257-264): out = [ReLU]( sum_k src_k[b, y >> shift_k, x >> shift_k, :] ), n = 1..4 terms (host arrays of n
 * device pointers, strides, shifts 0..3 = nearest-neighbour upsampling by 2^shift; H, W multiples of 2^shift), C channels. */
int poco_op_fuse_sum(int n, const float* const* d_src, const int* src_cs, const int* shift, float* d_out, int out_cs,
                     int B, int H, int W, int C, int relu, void* stream);
/* F.interpolate(scale_factor=2, mode='bilinear', align_corners=True) (hrnet.py:440): [B,H,W,C] -> [B,2H,2W,C], dense. */
int poco_op_bilinear_up2x(const float* d_in, float* d_out, int B, int H, int W, int C, void* stream);
/* nn.MaxPool2d(kernel_size=3, stride=2, padding=1) (resnet.py:206; padding never wins): [B,H,W,C] dense -> a slice of out_cs. */
int poco_op_maxpool3x3s2(const float* d_in, float* d_out, int B, int H, int W, int C, int out_cs, void* stream);
/* Global average pool (hrnet_cls.py:482, cliff_head.py:96): [B,H,W,C] dense L16 -> d_dst[b * dst_stride + c] (dst_stride a
 * multiple of 4, >= C). */
int poco_op_avgpool(const float* d_in, float* d_dst, int B, int H, int W, int C, int dst_stride, void* stream);
/* Stem conv + BN + ReLU from the image: ks = 3 (hrnet.py:467-469) or 7 (resnet.py:203-205), stride 2, pad (ks-1)/2, 3 -> 64.
 * d_img [B,3,H,W] NCHW, h_weight [64,3,ks,ks], d_out [B,Ho,4,Wo,16] L16 dense.  use_mfma 1 = the implicit-GEMM form where it
 * covers the shape (output width 112), else - and with 0 - the packed-FMA form: the answer is the same. */
int poco_op_stem_conv(const float* d_img, const float* h_weight, const float* h_scale, const float* h_shift, float* d_out,
                      int B, int H, int W, int ks, int use_mfma, void* stream);

/* Time `iters` launches of the same conv (+ReLU) with hipEvents; ms_out = mean ms per launch.
 * cfg_used7 (nullable) receives the tile configuration that ran: SEVEN ints {MT,NT,WM,WN,R,NI,ALG} (csrc/common.h
 * CONV_CFG_INTS) - the caller's array must hold 7. */
int poco_bench_conv2d(const float* d_in, int B, int H, int W, int Cin, const float* h_weight, int Cout,
                      int ks, int stride, float* d_out, const int* cfg7, int iters, float* ms_out,
                      int* cfg_used7, void* stream);

/* Part-attention pooling == pocolib/models/layers/keypoint_attention.py:34-48 (KeypointAttention.forward with
 * use_conv = False, softmax over the pixels) as pare_head.py:794-796 calls it (heat-map channel 0 = background is skipped):
 *   out[b, c, j] = sum_p softmax_p(heat[b, p, 1 + j]) * feat[b, p, c],  j = 0..23.
 * d_heat [B,H,heat_cs/16,W,16] (L16, heat_cs >= 32: channels 1..24 are the parts), d_feat [B,H,C/16,W,16] (L16, C a multiple of
 * 16, <= 128), d_out [B, C, 24]. */
int poco_op_part_attention(const float* d_heat, int heat_cs, const float* d_feat, int C, int B, int H, int W,
                           float* d_out, void* stream);
/* Timing of the same pool: `iters` back-to-back launches between two HIP events on `stream`; ms_out = mean ms per launch
 * (both kernels of the split-pixel softmax pool).  bench.py's `side_kernels` line. */
int poco_bench_part_attention(const float* d_heat, int heat_cs, const float* d_feat, int C, int B, int H, int W,
                              float* d_out, int iters, float* ms_out, void* stream);
/* LocallyConnected2d(128 -> 6, output_size [24,1], kernel 1, no bias) == pocolib/models/layers/locallyconnected2d.py:27-37
 * as pare_head.py builds its pose_mlp: pose6d[b, j, o] = sum_c x[b, c, j] * w[o, c, j].
 * d_x [B,128,24], d_w [6,128,24], d_pose6d [B,24,6]. */
int poco_op_lc2d_pose(const float* d_x, const float* d_w, float* d_pose6d, int B, void* stream);
/* rot6d_to_rotmat == pocolib/utils/geometry.py:247-261: d_in [B,24,3,2] (144 floats per crop) -> d_rotmat [B,24,3,3]. */
int poco_op_rot6d(const float* d_in, float* d_rotmat, int B, void* stream);

/* ---- head kernels on their own, at any stride (parity tests: tests/test_head_kernels_gpu.py) ---------------------------------
 * Row-vector data: a "row" is one crop's floats, `*_stride` the distance between rows in floats.  Argument errors - a null
 * pointer, B < 1, a stride smaller than the row, 2^31 floats or more - are POCO_ERR_ARG before any GPU work; each entry
 * synchronises `stream` before it returns. */
/* poco_op_rot6d with the launcher's operands: d_in rows of in_stride >= 144 floats; the 216 floats of a crop go to d_dst0 and
 * d_dst1 (rows of stride0 / stride1 >= 216; either may be NULL, not both). */
int poco_op_rot6d_ex(const float* d_in, int in_stride, float* d_dst0, int stride0, float* d_dst1, int stride1, int B,
                     void* stream);
/* poco_op_lc2d_pose with d_x rows of x_stride >= 3072 floats. */
int poco_op_lc2d_pose_ex(const float* d_x, int x_stride, const float* d_w, float* d_pose6d, int B, void* stream);
/* d_dst[b * dst_stride + i] = d_src[b * src_stride + i], i < n (1 <= n <= both strides). */
int poco_op_copy_rows(const float* d_src, int src_stride, float* d_dst, int dst_stride, int n, int B, void* stream);
/* d_dst[b * dst_stride + i] = d_src[i], i < n (the regressor's init vectors). */
int poco_op_broadcast_rows(const float* d_src, float* d_dst, int dst_stride, int n, int B, void* stream);
/* The first C channels of an L16 buffer [B,H,cs/16,W,16] -> dense NCHW d_out [B,C,H,W] (1 <= C <= cs, cs a multiple of 16). */
int poco_op_nhwc_to_nchw(const float* d_in, int cs, float* d_out, int B, int H, int W, int C, void* stream);
/* poco_outputs_t.record on its own: d_rec [B,254] = [rotmat 216 | betas 10 | cam 3 | var 24 | confidence 1] from rows of
 * rot_stride >= 216, betas_stride >= 10, cam_stride >= 3, var_stride >= 24 floats.  confidence = poco_utils.py:21-25,50-60 and
 * the clip of tester.py:245: cliff 0 | 1 (root value against 2 thr | mean over the joints against thr), kinematic 0 | 1. */
int poco_op_pack_record(const float* d_rot, int rot_stride, const float* d_betas, int betas_stride, const float* d_cam,
                        int cam_stride, const float* d_var, int var_stride, float* d_rec, int cliff, int kinematic, float thr,
                        int B, void* stream);
/* Camera conversion and projection of the 49 joints (smpl_head.py:63-78; cliff = 1: smplcam_head.py:65-90,123-139):
 * d_cam rows (s, tx, ty) of cam_stride >= 3 floats, d_joints49 [B,49,3] -> d_cam_t [B,3], d_joints2d [B,49,2] and, cliff only,
 * d_fullimg_cam_t [B,3] (nullable: then not written).  cliff = 1 needs d_focal [B], d_scale [B], d_center [B,2] = (x, y) and
 * d_orig_shape [B,2] = (h, w); with cliff = 0 they are not read. */
int poco_op_camera(const float* d_cam, int cam_stride, const float* d_joints49, int cliff, const float* d_focal,
                   const float* d_scale, const float* d_center, const float* d_orig_shape, float* d_cam_t,
                   float* d_fullimg_cam_t, float* d_joints2d, int B, void* stream);
/* The fused regressor's persistent kernel (csrc/mlp_chain.hip) on a caller-described PROGRAM: stages of independent jobs with a
 * grid barrier between consecutive stages.  Every operand is a column slice of one of nbuf caller-owned device buffers
 * (d_bufs[i], 16-byte aligned, buf_floats[i] floats): rows r < B at d_bufs[buf] + off + r * rs.
 *   layers [nlayers][POCO_MLP_LAYER_INTS] = {K, N, act, in_buf, in_off, in_rs, res_buf, res_off, res_rs, out_buf, out_off, out_rs}:
 *     out[r][n] = act(bias[n] + sum_k W[n][k] in[r][k] (+ res[r][n])), act 0 none | 1 ReLU | 2 sigmoid, res_buf = -1: no residual;
 *     K, N multiples of 16, offsets and strides multiples of 4; h_weights[l] = host [N][K] (packed as the engine packs a Linear),
 *     h_bias[l] = host [N].
 *   rows [nrows][POCO_MLP_ROW_INTS] = {kind, src_buf, src_off, src_rs, dst_buf, dst_off, dst_rs, dst2_buf, dst2_off, dst2_rs, n}:
 *     kind 0 copy (dst[r][i] = src[r][i], i < n) | 1 broadcast (dst[r][i] = src[i]) | 2 rot6d (144 -> 216 floats into dst and
 *     dst2; a buffer index of -1 = none, at least one; n is ignored).
 *   stages [nstages][4] = {layer0, nlayers, row0, nrows}: index ranges into the two arrays above.
 * max_blocks >= 1 bounds the grid (the launcher also bounds it by poco_op_mlp_chain_resident_blocks()); results do not depend
 * on it.  The entry owns the kernel's counters and its time-out word for the duration of the call.  POCO_ERR_ARG before any GPU
 * work: null arrays, B < 1, more than 16 layers / 12 row jobs / 14 stages, K or N no multiple of 16, misaligned offsets, an
 * operand that does not fit its buffer, a stage range outside the arrays.  Returns 6 if a grid barrier timed out. */
#define POCO_MLP_LAYER_INTS 12
#define POCO_MLP_ROW_INTS 11
int poco_op_mlp_chain(const int* layers, int nlayers, const float* const* h_weights, const float* const* h_bias,
                      const int* rows, int nrows, const int* stages, int nstages, float* const* d_bufs,
                      const long long* buf_floats, int nbuf, int B, int max_blocks, void* stream);
/* Blocks of that kernel the device holds at once (needs the GPU). */
int poco_op_mlp_chain_resident_blocks(void);
/* batch_rodrigues == pocolib/utils/geometry.py:207-244 (through quat_to_rotmat, with the reference's `theta + 1e-8` inside the
 * norm; not a textbook Rodrigues): d_axis_angle [N,3] -> d_rotmat [N,3,3].  Evaluated in fp64, stored as fp32.  The same device
 * function gives poco_evaluator_step its pose distance; this entry turns a ground-truth axis-angle pose [B,72] (N = 24 B) into
 * the rotation matrices poco_smpl_lbs takes.  Enqueued on `stream`. */
int poco_op_rodrigues(const float* d_axis_angle, float* d_rotmat, int N, void* stream);
/* rotation_matrix_to_angle_axis == pocolib/utils/geometry.py:264-429: d_rotmat [N,3,3] -> d_aa [N,3].  The reference's route, not a
 * textbook logarithm and not batch_rot2aa: rotation_matrix_to_quaternion on the transposed matrix with its four masked candidates
 * (the comparisons R22 < eps, R00 > R11 and R00 < -R11 on the float32 inputs, eps = float32(1e-6)), quaternion_to_angle_axis with
 * its atan2 pair and k = 2 at sin^2 = 0, then aa[isnan] = 0 - so a matrix holding a NaN gives (0, 0, 0) and the zero matrix
 * (0, pi, 0).  Evaluated in fp64, stored as fp32.  The same device function gives poco_pseudo_step its `pose`.  Enqueued on
 * `stream`. */
int poco_op_rotmat_to_aa(const float* d_rotmat, float* d_aa, int N, void* stream);

/* GPU-side crop + normalise: replaces the per-detection CPU loop cv2.getAffineTransform -> cv2.warpAffine(INTER_LINEAR,
 * BORDER_CONSTANT) -> ToTensor -> Normalize + per-crop H2D copy of pocolib/core/tester.py:182-203 and
 * pocolib/utils/vibe_image_utils.py:58-107,233-266,343-351.  The uint8 crop underneath is BYTE-exact with OpenCV 4.5.5's
 * fixed-point algorithm for that call (requirements.txt:4; restated in oracle/crop_np.py): 6x6 LU solve + inversion in
 * double, 10-bit fixed-point coordinates, 1/32-px fractions, int16 weights, rounded 15-bit shift.
 * d_frame uint8 [H,W,3] RGB, d_boxes [N,4] (cx,cy,w,h) px (float32, or float64 for the _f64 entry: the reference's
 * detections / smoothed tracks may be either), bbox_scale = the Python float `scale` of get_single_image_crop_demo,
 * d_out [N,3,res,res] fp32 NCHW. */
int poco_crop_normalize(const unsigned char* d_frame, int H, int W, const float* d_boxes, int N, double bbox_scale,
                        int res, float* d_out, void* stream);
int poco_crop_normalize_f64(const unsigned char* d_frame, int H, int W, const double* d_boxes, int N, double bbox_scale,
                            int res, float* d_out, void* stream);
/* The crops of a whole batch in ONE launch when they come from several frames of the same size (video / streaming mode:
 * tester.py:399-408 crops per frame): d_frames = device array of `nframes` device pointers to uint8 [H,W,3] frames,
 * d_frame_idx [N] int32 = which of them crop n is cut from (device data: cannot be validated on the host; the kernel clamps an
 * index into 0 .. nframes - 1, so a bad one reads the wrong frame, never a wild pointer).  Same arithmetic as poco_crop_normalize
 * (float32 boxes). */
int poco_crop_normalize_multi(const unsigned char* const* d_frames, int nframes, const int* d_frame_idx, int H, int W,
                              const float* d_boxes, int N, double bbox_scale, int res, float* d_out, void* stream);

/* ---- the DATASET crop (eval.py --crop dataset): rotation, flip, scale and per-channel pixel noise -------------------------------
 * Replaces BaseDataset.rgb_processing + normalize_img (pocolib/dataset/base_dataset.py:201-221,309) and the crop_cv2 it calls
 * (pocolib/utils/image_utils.py:189-206: gen_trans_from_patch_cv, pocolib/utils/vibe_image_utils.py:49-91, then cv2.warpAffine of
 * the FLOAT32 image) for a whole batch cut from images of mixed sizes, in one launch; csrc/dataset_crop.hip, DESIGN.md section 24.
 * One record per crop.  The host states gen_trans_from_patch_cv up to its three float32 source points (poco_amd/datacrop.py
 * crop_params: integer centre and box side, float32 rotate_2d with numpy's sin / cos); the device solves getAffineTransform and
 * inverts in double as poco_crop_normalize does, generates warpAffine's 10-bit fixed-point coordinates (1/32-pixel fractions) and
 * blends the four byte-valued taps with cv2's float weights - raw = (sum_i v_i m_i) / 1024, integer m_i summing to 1024, a tap
 * outside the image contributes 0: exact in float32.  Then np.fliplr (output column x shows crop column res - 1 - x), the noise
 * min(255, max(0, raw * pn[c])) in float32, and with normalize != 0 (x / 255 - mean) / std as oracle/crop_np.normalize_np. */
typedef struct {
  int32_t img;      /* which of d_images the crop is cut from; the kernel clamps it into 0 .. n_images - 1              */
  int32_t flip;     /* != 0: mirrored left-right after the warp (base_dataset.py:207-208)                               */
  float src[6];     /* gen_trans_from_patch_cv's `src`: centre, centre + down, centre + right as (x, y) pairs           */
  float pn[3];      /* per-channel noise factors, rounded to float32 (numpy 1.x: float32 array times float64 scalar)    */
  int32_t bb;       /* int(round(sc * scale * 200)): the box side crop_cv2 warps, kept for the host-side validation     */
} poco_dataset_crop_param_t;
/* d_images: device array of n_images device pointers to uint8 [H_i, W_i, 3] RGB images, d_img_hw int32 [n_images, 2] = (H_i, W_i),
 * d_params [N] the records on the device and h_params the host copy they were uploaded from, d_out fp32 [N, 3, res, res] NCHW:
 * the normalised crop, or with normalize = 0 the raw float crop after noise and clamp.  POCO_ERR_ARG before any GPU work (d_out is
 * not touched): a null pointer, N < 1, n_images < 1, res outside 1..4096, and - read from h_params, since device data cannot be
 * validated without a round trip - a non-finite source point or noise factor, or a box side that rounds to less than 1.  That check
 * is advisory in one sense: nothing compares h_params with d_params, so it vouches for the device records only if the caller
 * uploaded them from h_params.  The kernel reads d_params only and is memory-safe for any RECORD: the index is clamped, coordinates
 * saturate to int16 as cv2's maps do and every tap is bounds-checked against d_img_hw.  d_images and d_img_hw themselves are
 * trusted, like any device pointer: a size below 1 reads as an empty image, but a size larger than the allocation behind the
 * pointer lets taps read past it.  Enqueued on `stream`: no allocation, no synchronisation. */
int poco_dataset_crop(const unsigned char* const* d_images, const int* d_img_hw, int n_images, const poco_dataset_crop_param_t* d_params,
                      const poco_dataset_crop_param_t* h_params, int N, int res, int normalize, float* d_out, void* stream);

/* ---- the dataset crop with synthetic occluders (eval.py --aug_occlude) ---------------------------------------------------------
 * rgb_processing's occluder step (base_dataset.py:210-213: occlude_with_pascal_objects_kp, pocolib/dataset/occlusion.py:109-149)
 * inside the launch of poco_dataset_crop, between the flip and the pixel noise, where the reference has it; DESIGN.md section 23,
 * numpy restatement tests/occlude_np.py.  The host makes the reference's draws (poco_amd/datacrop.py occlusion_params): per crop up
 * to 7 objects, each a cut-out, the size resize_by_factor gives it and the centre paste_over receives.  The device computes, per
 * output pixel and object whose paste rectangle [c - size // 2, c - size // 2 + size) holds the pixel, the one texel of
 * cv2.resize(cut-out, (dst_w, dst_h), interpolation=INTER_AREA) on uint8 RGBA that the pixel needs:
 *   both axes with an integer scale src / dst: sums over the sx x sy source block, (s + 2) >> 2 for 2 x 2, otherwise
 *     round-half-to-even of float32(s) * float32(1.f / (sx * sy)); 1 x 1 is the copy;
 *   otherwise cv::computeResizeAreaTab's entries per axis, derived in double, and ResizeArea_'s float32 sequence: per source row
 *     buf += S * alpha in table order, then sum = beta * buf for the first row and sum += beta * buf after it, each multiply and
 *     add rounded on its own; the result round-half-to-even, saturated to a byte.
 * and blends as paste_over does: alpha = float32(a) / 255, out = alpha * colour + (1 - alpha) * dst per channel in float32, two
 * products and one sum, objects in drawn order (later ones cover earlier ones).  Then noise, clamp and Normalize as above.  A record
 * with count = 0 leaves the crop bit for bit what poco_dataset_crop gives. */
#define POCO_OCC_MAX_OBJECTS 7
typedef struct {
  int32_t offset;   /* first texel of the cut-out in the atlas, in texels (4 bytes: R, G, B, A)                        */
  int32_t h, w;     /* its size; rows are packed                                                                       */
} poco_occluder_t;
typedef struct {
  int32_t id;       /* which cut-out; the kernel clamps it into the table                                              */
  int32_t dst_w;    /* resize_by_factor's new_size: np.round([w, h] * factor).astype(int)                              */
  int32_t dst_h;
  int32_t cx, cy;   /* paste_over's centre after np.round(center).astype(np.int32), in crop pixels                     */
} poco_occ_object_t;
typedef struct {
  int32_t count;                                /* objects of this crop, 0 .. POCO_OCC_MAX_OBJECTS                     */
  poco_occ_object_t obj[POCO_OCC_MAX_OBJECTS];  /* in drawn order                                                      */
} poco_occ_record_t;                            /* 144 bytes                                                           */
/* The arguments of poco_dataset_crop, then: d_atlas = all cut-outs as packed uint8 RGBA on the device (4-byte aligned, uploaded
 * once per run), atlas_texels its size in texels, d_occluders [n_occluders] the table on the device and h_occluders its host copy,
 * d_occ [N] the per-crop records on the device and h_occ their host copy, d_cover = null or int32 [N, ceil(res/32)^2]: every block
 * writes, unconditionally, the number of its pixels that a pasted texel with alpha > 0 touched - no memset, no atomics; the caller
 * sums a crop's cells.  POCO_ERR_ARG before any GPU work (d_out and d_cover are not touched): everything poco_dataset_crop refuses,
 * a null or misaligned atlas, table or record pointer, res > 256 (a larger crop could ask for an upscaled cut-out: INTER_LINEAR is
 * not built), an empty atlas, a cut-out side outside 1..4096 or a cut-out that does not lie inside the atlas, a count outside
 * 0..7, an occluder id outside the table, a destination side below 1 or above the source side.  As for the crop records the host
 * copies are what is checked; the kernel is memory-safe for any device record or table: count, id and sizes are clamped, every tap
 * is clamped into its cut-out and checked against atlas_texels.  Enqueued on `stream`: no allocation, no synchronisation. */
int poco_dataset_crop_occ(const unsigned char* const* d_images, const int* d_img_hw, int n_images, const poco_dataset_crop_param_t* d_params,
                          const poco_dataset_crop_param_t* h_params, int N, int res, int normalize, const unsigned char* d_atlas,
                          long long atlas_texels, const poco_occluder_t* d_occluders, const poco_occluder_t* h_occluders, int n_occluders,
                          const poco_occ_record_t* d_occ, const poco_occ_record_t* h_occ, float* d_out, int* d_cover, void* stream);
/* poco_dataset_crop_occ with one more output (eval.py --visibility --aug_occlude): d_mask uint8 [N,res,res] <-
 * 1 where a pasted texel with alpha > 0 touched the pixel - the condition d_cover counts, so a crop's mask sums to its cells - and 0
 * elsewhere; every byte is written, by the same launch, and it may not be null (else POCO_ERR_ARG, as for every argument
 * poco_dataset_crop_occ refuses).  A third instantiation of the one kernel body: d_out and d_cover are bit for bit what
 * poco_dataset_crop_occ gives, and the two older entries keep their own kernels. */
int poco_dataset_crop_occ_mask(const unsigned char* const* d_images, const int* d_img_hw, int n_images,
                               const poco_dataset_crop_param_t* d_params, const poco_dataset_crop_param_t* h_params, int N, int res,
                               int normalize, const unsigned char* d_atlas, long long atlas_texels, const poco_occluder_t* d_occluders,
                               const poco_occluder_t* h_occluders, int n_occluders, const poco_occ_record_t* d_occ,
                               const poco_occ_record_t* h_occ, float* d_out, int* d_cover, unsigned char* d_mask, void* stream);

/* ---- demo renderer: the uncertainty-coloured SMPL overlay of demo.py --render ----------------------------------------------
 * Replaces pyrender's offscreen render (pocolib/utils/vibe_renderer.py:33-57,88-151) as pocolib/core/tester.py:248-345 (folder
 * mode) and :482-580 (video mode) call it; csrc/render.hip.  Draws P posed meshes over an RGB uint8 frame in place.
 *   Geometry (vibe_renderer.py:33-57,88-151): vertex v of person p becomes q = R * Rx(180 deg) * v, R = h_rot3x3 (row-major) or
 *     the identity (the side view passes Ry(270 deg), tester.py:335-348).  The weak-perspective camera (sx, sy, tx, ty) = orig_cam
 *     projects through the matrix of vibe_renderer.py:49-56: col = W/2 (1 + sx (q_x + tx)), row = H/2 (1 - sy (q_y - ty)), rows
 *     from the top; no perspective divide, so screen-space barycentrics are exact.  Pixel (r, c) is one sample at its centre
 *     (c + 0.5, r + 0.5).  Fragments with |q_z| > 1 are discarded (GL clipping, NDC z = -q_z).  Inside one person the larger q_z
 *     (nearer) wins, ties go to the lower triangle index.  Fill rule: a centre on an edge belongs to the triangle it would lie in
 *     after a nudge by (+eps, +eps^2) - an edge shared by two triangles owns each of its centres exactly once.
 *   People: each has its own camera, so there is no common depth (the reference renders them one pass each and pastes): painter's
 *     order, person p + 1 covers person p wherever both cover a pixel.  The caller orders them (folder mode: detection order,
 *     tester.py:276; video mode: ascending orig_cam[1], stable, demo_utils.py:307-313).
 *   Shading: pyrender's metallic-roughness shader for this scene (vibe_renderer.py:74-86: ambient 0.3, three directional lights
 *     of intensity 1 along -z, so l = v = h = +z).  c = clamp(n'_z, 0, 1), n' = the renormalised interpolated vertex normal after
 *     R * Rx; vertex normals = area-weighted sums of the incident faces' normals (gathered, not atomically summed).  material 0
 *     (pyrender's default for a vertex-coloured trimesh): metallic m = 0.2, roughness rho = 0.8; material != 0 (the plain grey of
 *     tester.py:288-290): m = 0, rho = 1.  alpha = rho^2, f0 = F = 0.04 (1 - m) + b m, c_diff = 0.96 b (1 - m),
 *     D = alpha^2 / (pi (c^2 (alpha^2 - 1) + 1)^2), G = (2c / (c + sqrt(alpha^2 + (1 - alpha^2) c^2)))^2,
 *     colour = 3 c ((1 - F) c_diff / pi + F G D / (4 c^2 + 0.001)) + 0.3 b, written as round(255 clamp(colour^(1/2.2), 0, 1)).
 *   Composite (valid_mask, vibe_renderer.py:139-141): pixels no person covers keep their bytes exactly.
 * Limits: P <= 1024, F < 2^22 (the 64-bit visibility key (P - 1 - p) << 54 | bits(1 - q_z) << 22 | triangle), V <= 2^24,
 * H, W <= 16384.  Fidelity to pyrender's pixels is unpinned (single sample, area-weighted normals, view vector +z). */
typedef struct poco_renderer* poco_renderer_t;
/* h_faces int32 [F,3] (host) of meshes with V vertices: validated (indices in [0, V)), a vertex -> face CSR is built, both are
 * uploaded.  Needs the GPU after validation; the handle owns a visibility buffer that grows with the largest frame rendered. */
int poco_renderer_create(const int32_t* h_faces, int F, int V, poco_renderer_t* out);
/* Draw P people over d_frame uint8 [H,W,3] RGB (in place).  d_verts fp32 [P,V,3] (the engine's smpl_vertices as they are),
 * d_params fp32 [P,8] per person (sx, sy, tx, ty, r, g, b, material), r g b = base colour in [0,1].  h_rot3x3: NULL = identity.
 * d_frag_count: NULL, or int32 [H,W] that receives the number of fragments per pixel that pass coverage and clipping (a test hook
 * for the fill rule).  Enqueued on `stream` (a memset + three launches): no allocation unless the frame or P*V is larger than
 * any before, no synchronisation. */
int poco_renderer_render(poco_renderer_t r, unsigned char* d_frame, int H, int W, const float* d_verts, int P,
                         const float* d_params, const float* h_rot3x3, int* d_frag_count, void* stream);
void poco_renderer_destroy(poco_renderer_t r);

/* Wireframe (RenderFlags.ALL_WIREFRAME, pocolib/utils/vibe_renderer.py:133-136, asked for by demo.py:290-303 --wireframe through
 * pocolib/core/tester.py:266-271,485-490): GL polygon mode LINE with the depth test and back-face culling on.  Geometry, clipping,
 * painter's order between people, shading formulas and composite are those of poco_renderer_render; csrc/render.hip.
 *   Edges: the three edges of every FRONT-FACING triangle, ((q1 - q0) x (q2 - q0)).z > 0 in the transformed space q (GL
 *     counter-clockwise, camera looking down -z); a zero-area triangle draws nothing.  An edge between a front- and a back-facing
 *     triangle is drawn, an edge between two back-facing ones is not.
 *   Line rule (one pixel wide, one sample per pixel): an edge is walked from its lower vertex index (A) to its higher one (B), so
 *     both triangles sharing it make bit-identical fragments.  Endpoints in continuous (col, row) float32; the major axis a is the
 *     one with the larger |delta| (a tie: columns), b the other.  Major pixel i is covered when min(a_A, a_B) <= i + 0.5 <
 *     max(a_A, a_B); t = (i + 0.5 - a_A) / (a_B - a_A); minor pixel floor(b_A + t (b_B - b_A)); q_z and the vertex normal are
 *     x_A + t (x_B - x_A).  a_A == a_B draws nothing.  Fragments with |q_z| > 1 or outside the frame are dropped.
 *   Visibility: only line fragments write depth (back edges show through the gaps, as in GL).  Inside one person the nearest
 *     fragment wins, ties go to the lower (triangle << 2 | edge), edge e = the edge opposite vertex e of the triangle.
 *   Shading: the interpolated normal is renormalised and goes through the shader above with the person's colour and material.
 *   Pixels no line covers keep their bytes exactly.
 * Limit: the id (triangle << 2 | edge) takes the key's 22 low bits, so a wireframe call needs F < 2^20 = 1048576 faces
 * (POCO_ERR_ARG beyond; SMPL has 13776).  Fidelity to GL's own line rasterisation (diamond-exit rule) is unpinned. */
#define POCO_RENDER_WIREFRAME 1u   /* bit 0: draw the meshes as wireframes */
#define POCO_RENDER_IDS 2u         /* bit 1: NOT FOR USERS - a test hook like d_frag_count itself, kept only so that the tests can
                                    * compare the winner of each pixel; it may change without an ABI bump.  d_frag_count receives,
                                    * instead of the fragment count, the id that won each pixel - the triangle, or
                                    * (triangle << 2 | edge) of a wireframe call - and -1 where none did */
#define POCO_RENDER_MAX_WIRE_FACES ((1 << 20) - 1)
/* poco_renderer_render with a flags word: flags = 0 is that call exactly (the same launches, the same bytes); any bit other than
 * the two above is POCO_ERR_ARG, and so is POCO_RENDER_IDS without d_frag_count.  A wireframe call enqueues a memset and three
 * launches like the filled one (POCO_RENDER_IDS adds one). */
int poco_renderer_render_ex(poco_renderer_t r, unsigned char* d_frame, int H, int W, const float* d_verts, int P,
                            const float* d_params, const float* h_rot3x3, int* d_frag_count, unsigned flags, void* stream);

/* Keypoint discs: cv2.circle(img, (int(pt[0]), int(pt[1])), 4, colour, -1) of pocolib/core/tester.py:324-328 (folder mode: SMPL
 * joints white, OpenPose joints black) and :552-554 (video mode: green), demo.py:290-303 --draw_keypoints; csrc/render.hip.
 * d_frame uint8 [H,W,3] (in place); d_points fp32 [N,2] (col, row), each truncated toward zero as int() does; d_rgb uint8 [N,3];
 * radius r in 0 .. POCO_DISC_MAX_RADIUS.  Point k paints the pixels (cx + dx, cy + dy), |dy| <= r, |dx| <= half_width[r][|dy|],
 * clipped to the frame: 2r + 1 rows.  Points are painted in index order: where stamps overlap the higher index wins (a per-pixel
 * scan from the last point down; no atomics, deterministic).  A point that is not finite or >= 2^30 in magnitude paints nothing.
 * half_width = the midpoint circle (x = 0, y = r, d = 1 - r; a visited (x, y) gives row y the half-width x and row x the
 * half-width y, the larger one stays), row r[|dy|] of the one table below, which tests/render_overlay_np.py reads from this file.
 * Equality with cv2.circle's own filled circle is unpinned (tools/validate_assets.py --keypoints compares where cv2 exists).
 * Limits: H, W <= 16384, 0 <= N <= 65536 (N = 0 is a no-op).  One launch on `stream`, no allocation, no synchronisation. */
#define POCO_DISC_MAX_RADIUS 8
#define POCO_DISC_HALF_WIDTHS { \
  {0, 0, 0, 0, 0, 0, 0, 0, 0}, \
  {1, 0, 0, 0, 0, 0, 0, 0, 0}, \
  {2, 2, 1, 0, 0, 0, 0, 0, 0}, \
  {3, 3, 2, 1, 0, 0, 0, 0, 0}, \
  {4, 4, 3, 3, 1, 0, 0, 0, 0}, \
  {5, 5, 5, 4, 3, 2, 0, 0, 0}, \
  {6, 6, 6, 5, 4, 3, 2, 0, 0}, \
  {7, 7, 7, 6, 6, 5, 4, 2, 0}, \
  {8, 8, 8, 7, 7, 6, 5, 4, 2} }
int poco_renderer_draw_discs(unsigned char* d_frame, int H, int W, const float* d_points, const unsigned char* d_rgb, int N,
                             int r, void* stream);

/* ---- occlusion sensitivity sweep: demo.py --occlusion_map (csrc/occlusion.hip, poco_amd/occlusion.py) ------------
 * The occlusion analysis of PARE (a grey square slides over the crop, the regressor runs on every occluded copy, the change of
 * the output is drawn per position) around the engine's forwards.  All three calls are one launch on `stream`: no allocation, no
 * synchronisation, arguments validated before the launch.  numpy restatement: tests/occlusion_np.py.
 *
 * poco_op_occlude_batch: d_out fp32 [m,3,res,res] = m copies of d_src fp32 [3,res,res]; copy i holds h_fill3[c] (host, three
 *   normalised values) at rows y0 .. y0 + patch - 1, columns x0 .. x0 + patch - 1, (y0, x0) = d_pos[i] (int32 [m,2] on the device:
 *   it only selects, so a value outside the crop paints less or nothing and never moves an address).  Copy and select only: the
 *   output's bits are the source's or the fill's.  16-byte loads and stores throughout (a patch edge inside a quad is a per-element
 *   select), hence res % 4 == 0 and d_src, d_out 16-byte aligned.  Limits: 4 <= res <= 4096, 1 <= patch <= res, 0 <= m <= 65536. */
int poco_op_occlude_batch(const float* d_src, int res, const int* d_pos, int m, int patch, const float* h_fill3, float* d_out,
                          void* stream);
/* poco_op_occlusion_records: row i of the engine's outputs for the occluded copies (d_verts [m,V,3] = smpl_vertices, d_var [m,24]
 *   = var_pose, d_j3d [m,49,3] = smpl_joints3d) against ONE baseline row (d_base_*), POCO_OCCLUSION_RECORD_FLOATS per row:
 *     [0] mean over the V vertices of |v_occ - v_base| (Euclidean)   [1] the maximum of that
 *     [2] mean of var_occ over its 24 entries                        [3] mean of var_occ - var_base
 *     [4:28] var_occ[j] - var_base[j]                                [28:77] |j3d_occ[k] - j3d_base[k]| of the 49 joints
 *   One workgroup per row; fixed reduction order (lane-strided partial sums, a wave shuffle tree, four LDS partials added in wave
 *   order), no atomics: two calls give the same bits.  V even and d_verts, d_base_verts 8-byte aligned (two vertices are read as
 *   three 8-byte loads; SMPL has 6890).  Limits: 2 <= V <= 2^20, 0 <= m <= 65536. */
#define POCO_OCCLUSION_RECORD_FLOATS 77
int poco_op_occlusion_records(const float* d_verts, const float* d_var, const float* d_j3d, int m, int V,
                              const float* d_base_verts, const float* d_base_var, const float* d_base_j3d, float* d_records,
                              void* stream);
/* poco_op_heat_overlay: d_field fp32 [n] (one value per position: a record column), d_pos int32 [n,2] and patch as above, d_crop
 *   uint8 [res,res,3] (the --render_crop canvas), d_lut uint8 [256,3] (the jet table), d_out uint8 [res,res,3] (may be d_crop).
 *   Per pixel: value = (the float32 sum, in position order, of the field over the patches that cover the pixel) / their count;
 *   t = value / scale clamped to [0, 1] (NaN -> 0); index = (int)(255 t + 0.5); out = (128 lut[index] + 128 crop + 128) >> 8 per
 *   byte.  Every operation is rounded on its own (no contraction), so the bytes equal the float32 restatement.  scale > 0 (finite),
 *   or 0 = "auto": the field's maximum, found on the device (NaN entries skipped); a field whose maximum is not a positive finite
 *   number leaves the crop unchanged, and so does a pixel no patch covers.  Limits: 1 <= res <= 4096, 1 <= patch <= res,
 *   1 <= n <= 65536. */
int poco_op_heat_overlay(const float* d_field, const int* d_pos, int n, int patch, int res, float scale,
                         const unsigned char* d_lut, const unsigned char* d_crop, unsigned char* d_out, void* stream);

/* ---- JPEG encoder: the demo's rendered frames as baseline JPEG, encoded where they are ------------------------------------------
 * Replaces the host-side picture encoding behind pocolib/core/tester.py:338-345 (cv2.imwrite per frame) and, with
 * poco_amd/jpeg.py's Motion-JPEG .avi writer on top, the ffmpeg call of demo.py:148-157 / demo_utils.py:237-245 (images_to_video,
 * -pix_fmt yuv420p); csrc/jpeg_enc.hip.  Takes a uint8 [H,W,3] RGB device frame, leaves the bytes of a JFIF file on the device.
 *   Format: baseline sequential (SOF0), 8 bit, YCbCr 4:2:0 (luma sampling 2x2), JFIF 1.01 with density 1:1.  Stream: SOI, APP0,
 *     DQT x2, SOF0, DHT x4, DRI, SOS, the restart intervals, EOI; the header is 629 bytes.
 *   Arithmetic: integers only, so the bytes are a function of (frame, quality) alone and equal those of the numpy restatement
 *     tests/jpeg_np.py.  RGB -> YCbCr in libjpeg's 16-bit fixed point (jccolor.c, SCALEBITS 16); chroma = the 2x2 box sum with
 *     libjpeg's alternating bias 1, 2, 1, 2 ... along a row, >> 2 (jcsample.c h2v2_downsample); a frame whose sides are no
 *     multiples of 16 is padded by edge replication to whole 16x16 MCUs, SOF0 carries the true H and W; forward DCT = libjpeg's
 *     "islow" integer DCT (jfdctint.c: 13-bit constants, PASS1_BITS 2) on samples minus 128; quantisation by the Annex K tables
 *     scaled by jpeg_quality_scaling (quality 1..100) and clamped to 1..255, rounding to nearest with ties away from zero
 *     (jcdctmgr.c forward_DCT).
 *   Entropy coding: the four Annex K Huffman tables (not optimised), zigzag order, EOB and ZRL.  One restart interval per MCU row
 *     (DRI = MCUs per row): each starts with DC predictors 0, ends padded with 1-bits to a byte boundary, has 0xFF -> 0xFF 0x00
 *     stuffing and is followed by RSTm (m counting modulo 8), the last one by EOI.  The intervals are what is coded in parallel.
 *   Size bound: a block codes into at most 64 x (16 + 11) bits = 216 bytes, at most twice that after stuffing, so
 *     worst case(H, W) = 629 + ceil(H/16) x (ceil(W/16) x 6 x 432 + 2) bytes.  The scratch planned at create and the caller's
 *     out_cap are held to it: overflow cannot happen and is not a status code. */
typedef struct poco_jpeg_encoder* poco_jpeg_encoder_t;
/* Tables, coefficient scratch (768 bytes per MCU) and worst-case interval slots (2592 bytes per MCU) for frames up to max_h x max_w
 * (1 .. 16384 each, else POCO_ERR_ARG without touching the GPU).  Needs the GPU after validation. */
int poco_jpeg_encoder_create(int max_h, int max_w, poco_jpeg_encoder_t* out);
/* d_rgb uint8 [H,W,3] (any alignment) -> d_out[0 .. *d_len): three launches on `stream` - transform, entropy coding, compaction -
 * with no allocation, no synchronisation and no global atomics; nothing outside d_out[0 .. *d_len) and the word d_len is written.
 * POCO_ERR_ARG before any GPU work: a null handle or pointer, H or W < 1 or above the created maximum, quality outside 1..100,
 * out_cap below worst case(H, W).  One encoder is used from one stream at a time (its scratch is reused in stream order). */
int poco_jpeg_encode(poco_jpeg_encoder_t enc, const unsigned char* d_rgb, int H, int W, int quality, unsigned char* d_out,
                     size_t out_cap, unsigned int* d_len, void* stream);
void poco_jpeg_encoder_destroy(poco_jpeg_encoder_t enc);

/* ---- JPEG decoder: baseline JPEG input frames decoded on the device --------------------------------------------------------------
 * Replaces the host-side decode behind pocolib/core/tester.py:171 (cv2.imread + cvtColor per image of the folder) and :507
 * (cv2.imread per frame of the result video), and the frames that demo.py:69-90 / demo_utils.py:183-199 (video_to_images) extract
 * from a video; csrc/jpeg_dec.hip.  Takes the entropy-coded bytes of up to max_batch parsed files (poco_amd/jpeg.py parse_jpeg
 * walks the markers on the host), leaves one uint8 [H,W,3] RGB picture per file on the device: a few hundred KB cross PCIe
 * instead of 6 MB per 1080p frame.
 *   Streams: baseline sequential (SOF0), 8 bit, one interleaved scan; three components YCbCr with luma sampling 1x1, 2x1 or 2x2
 *     and chroma 1x1, or one component (replicated to R = G = B); any 8-bit DQT, any DHT, any DRI or none.
 *   Arithmetic: integers only; the pixels equal libjpeg's with jpeg_decompress defaults (what PIL gives) and those of the numpy
 *     restatement tests/jpegdec_np.py.  Dequantisation, the "islow" inverse DCT (jidctint.c: 13-bit constants, PASS1_BITS 2),
 *     + 128 and a clamp to 0..255; "fancy" chroma upsampling (jdsample.c: h2v1 weights 3/4 1/4 with roundings + 1 / + 2, h2v2
 *     weights 9 3 3 1 / 16 with roundings + 8 / + 7, over the component's own width ceil(W/2) and height ceil(H/2) with the
 *     first / last column and row repeated; plain replication when that width is 2 or less); YCbCr -> RGB in jdcolor.c's 16-bit
 *     fixed point.  Where the inverse DCT leaves 0..255 by more than libjpeg's range-limit table holds the result is clamped.
 *   Entropy decoding: every restart interval is cut into subsequences of 128 bytes; a lane decodes its subsequence from a guessed
 *     state (bit position, block within the MCU, zigzag index) and, round after round, from its predecessor's exit state until
 *     no exit state changes; counts, a prefix sum and a write pass store the coefficients; DC differences become values in a
 *     segmented scan per component.  The Huffman tables (a 9-bit lookahead table + maxcode / valptr) are built on the host.
 *   Safety: every read of the byte stream is clamped to its restart interval, every store is guarded by its own index; a code
 *     that is in no table, a zigzag index past 63 or an interval that ends before its blocks do sets that image's status word. */
typedef struct poco_jpeg_decoder* poco_jpeg_decoder_t;
/* One parsed file (all pointers on the host except d_rgb).  Tables are given per component as the file selects them. */
typedef struct poco_jpeg_image {
  const unsigned char* data;      /* the scan's entropy-coded bytes, RSTm markers included, EOI excluded */
  size_t nbytes;
  const unsigned int* segs;       /* [nseg][3]: offset into data, length, first MCU of every restart interval */
  int nseg;
  int H, W, ncomp;                /* ncomp 1 or 3 */
  int hsamp, vsamp;               /* luma sampling: 1x1, 2x1 or 2x2 (1x1 for one component) */
  unsigned short qt[3][64];       /* quantisation table per component, natural (row-major) order */
  unsigned char dc_bits[3][16], dc_vals[3][16], ac_bits[3][16], ac_vals[3][256];
  unsigned char* d_rgb;           /* device: receives H * W * 3 bytes, any alignment */
} poco_jpeg_image;
/* Device scratch (coefficients, planes, per-subsequence states) and one pinned staging buffer for up to max_batch images of up to
 * max_h x max_w (1 .. 16384 each) whose bytes and tables add up to at most max_bytes per call; POCO_ERR_ARG without touching the
 * GPU for sizes outside that, max_batch outside 1 .. 4096 or max_bytes outside 1 .. 2^30.  Needs the GPU after validation. */
int poco_jpeg_decoder_create(int max_h, int max_w, int max_batch, size_t max_bytes, poco_jpeg_decoder_t* out);
/* Decode imgs[0 .. n) in one call: one host-to-device copy of bytes, tables and interval tables from the pinned staging buffer,
 * two memsets and the launches (synchronisation rounds, counts, write, DC scan, inverse DCT, upsampling + colour) on `stream`; no
 * allocation, no global atomics.  d_status int32 [n] on the device receives 0 for a decoded image and non-zero for one whose
 * stream was damaged (its pixels are then unspecified; the other images are decoded); nothing outside the n pictures and
 * d_status is written.  The only host wait is for the previous call's copy out of the staging buffer.  POCO_ERR_ARG before any
 * GPU work: null handle or pointer, n outside 1 .. max_batch, a size outside the created maximum, sampling or component counts
 * other than those above, a Huffman table that is no prefix code or names more symbols than its array holds (16 for DC, 256 for
 * AC), an interval outside the data, or more bytes / intervals (2048 per image of max_batch) than the decoder was created for.  One decoder is used from one stream at a time. */
int poco_jpeg_decode(poco_jpeg_decoder_t dec, const poco_jpeg_image* imgs, int n, int* d_status, void* stream);
void poco_jpeg_decoder_destroy(poco_jpeg_decoder_t dec);

/* ---- progressive JPEG decoder: SOF2 input frames decoded on the device ------------------------------------------------------------
 * Replaces the same host-side decode as the baseline decoder above (pocolib/core/tester.py:171 and :507, cv2.imread per image)
 * for the files poco_jpeg_decode does not take: progressive DCT (SOF2), what web servers and export pipelines commonly write;
 * csrc/jpeg_prog.hip, DESIGN.md 17.  Takes the bytes of up to max_batch parsed files and their scan tables (poco_amd/jpeg.py
 * parse_progressive_jpeg walks the markers and validates the scan script on the host), leaves one uint8 [H,W,3] RGB picture per
 * file on the device.
 *   Streams: progressive Huffman (SOF2), 8 bit, no restart interval; components and sampling as for poco_jpeg_decode; up to 64
 *     scans: DC first and refinement scans (of one component, or interleaved over all), AC first scans with end-of-band runs and
 *     AC refinement scans with correction bits (one component each), any successive approximation with Al <= 13; DHT between
 *     scans, at most 16 distinct Huffman tables per file.  Every coefficient of every component must end at Al = 0: libjpeg
 *     smooths the blocks of a picture whose script stops above that (jdcoefct.c), this decoder does not, so such a script is
 *     refused (POCO_ERR_ARG) and the pixels of every file that is taken are libjpeg's.  The one exception is a file cut short
 *     (no EOI; its last scan carries POCO_JPEG_PROG_SCAN_CUT): it is taken whatever Al it ends at, and if that is above 0 its
 *     status word is non-zero (2) whatever its last scan decodes to.
 *   Arithmetic: integers only; the pixels equal libjpeg's (what PIL gives) and those of tests/jpegprog_np.py.  The coefficient
 *     stage follows jdphuff.c and writes final values (DC prediction undone by the lane that walks the scan) into the zeroed int16
 *     coefficient buffer in natural order; dequantisation, inverse DCT, upsampling and colour are poco_jpeg_decode's kernels.
 *   Order: a scan runs after every earlier scan of its file that touches one of its (component, coefficient) pairs: the host
 *     gives every scan the length of its longest such chain as its level and launches level after level, one wave per scan;
 *     scans of one level - other components, other bands, other images - run concurrently.
 *   Geometry: a scan of one component covers ceil(w_c / 8) x ceil(h_c / 8) blocks of that component's own size in raster order,
 *     an interleaved scan covers whole MCUs; the coefficient buffer holds whole MCUs.
 *   Safety: every read of the stream is clamped to its scan, every store is guarded by its own index, every loop is bounded by a
 *     constant or a validated count; a window without a code, a run past Se, an end-of-band run past the last block or a scan whose
 *     bytes end before its blocks do sets that image's status word and ends that scan. */
typedef struct poco_jpeg_prog_decoder* poco_jpeg_prog_decoder_t;
typedef struct poco_jpeg_prog_table {
  unsigned char bits[16], vals[256];   /* one DHT table: codes per length 1 .. 16, symbols */
} poco_jpeg_prog_table;
typedef struct poco_jpeg_prog_scan {
  unsigned int offset, length;    /* the scan's entropy-coded bytes in data, up to the next marker */
  unsigned char ncomp, comp[3];   /* components of the scan (indices into the frame's): 1, or all of them for a DC scan */
  unsigned char ss, se, ah, al;   /* spectral selection and successive approximation */
  short tab[3];                   /* tables[]: per component the DC table of a first DC scan; [0] the AC table of an AC scan */
  short flags;                    /* POCO_JPEG_PROG_SCAN_CUT on the last scan of a file that ends without EOI, else 0 */
} poco_jpeg_prog_scan;
#define POCO_JPEG_PROG_SCAN_CUT 1
/* One parsed file (all pointers on the host except d_rgb). */
typedef struct poco_jpeg_prog_image {
  const unsigned char* data;      /* the file's bytes from its first scan to the end of its last */
  size_t nbytes;
  const poco_jpeg_prog_scan* scans;     /* in file order */
  int nscan;                      /* 1 .. 64 */
  const poco_jpeg_prog_table* tables;
  int ntable;                     /* 0 .. 256 */
  int H, W, ncomp;                /* ncomp 1 or 3 */
  int hsamp, vsamp;               /* luma sampling: 1x1, 2x1 or 2x2 (1x1 for one component) */
  unsigned short qt[3][64];       /* quantisation table per component, natural (row-major) order */
  unsigned char* d_rgb;           /* device: receives H * W * 3 bytes, any alignment */
} poco_jpeg_prog_image;
/* Device scratch (coefficients, planes) and one pinned staging buffer for up to max_batch images of up to max_h x max_w (1 .. 16384
 * each) whose bytes add up to at most max_bytes per call; POCO_ERR_ARG without touching the GPU for sizes outside that, max_batch
 * outside 1 .. 4096 or max_bytes outside 1 .. 2^30.  Needs the GPU after validation. */
int poco_jpeg_prog_decoder_create(int max_h, int max_w, int max_batch, size_t max_bytes, poco_jpeg_prog_decoder_t* out);
/* Decode imgs[0 .. n) in one call: one host-to-device copy of bytes, tables and scan tables from the pinned staging buffer, two
 * memsets, one launch per level of the scan order, then inverse DCT and upsampling + colour on `stream`; no allocation, no global
 * atomics.  d_status int32 [n] as for poco_jpeg_decode.  POCO_ERR_ARG before any GPU work: null handle or pointer, n outside
 * 1 .. max_batch, a size outside the created maximum, sampling or component counts other than those above, a scan table that
 * breaks the rules of parse_progressive_jpeg (band, components, successive approximation, a table index outside tables[], a scan
 * outside the data, a coefficient no scan sends, a script that ends above Al = 0 in a file not marked as cut short), a Huffman table
 * that is no prefix code, more than 16 distinct Huffman tables in one file, or more bytes than the decoder was created for.  One
 * decoder is used from one stream at a time. */
int poco_jpeg_prog_decode(poco_jpeg_prog_decoder_t dec, const poco_jpeg_prog_image* imgs, int n, int* d_status, void* stream);
void poco_jpeg_prog_decoder_destroy(poco_jpeg_prog_decoder_t dec);

/* ---- PNG encoder: the demo's rendered frames as PNG, filtered and deflated where they are --------------------------------------
 * Replaces the host-side cv2.imwrite(... '%06d.png') of pocolib/core/tester.py:350 and :572; csrc/png_enc.hip.  Takes a uint8
 * [H,W,3] RGB device frame, leaves the bytes of a .png file on the device: lossless, and byte for byte a function of the frame
 * (tests/png_np.py restates every byte in numpy).
 *   Container: the 8-byte signature, IHDR (W, H, bit depth 8, colour type 2, compression 0, filter 0, interlace 0), one IDAT
 *     chunk per segment, IEND; nothing else.  The first IDAT also carries the zlib header 78 01, the last the big-endian Adler-32
 *     of the filtered stream; every chunk carries the CRC-32 of its type and data.
 *   Row filters: every row gets the one of the five PNG filter types (bpp 3) with the smallest sum of |signed byte| (v < 128 ?
 *     v : 256 - v: libpng's heuristic), ties to the lowest type; the row above the first is zeros.  Filtered stream: H x (1 + 3W).
 *   Segments: the stream is cut every 32 768 bytes regardless of rows; each segment is coded on its own - no match reaches out
 *     of it, it has its own Huffman tables - as one deflate block with BFINAL 0, followed by an empty stored block (000, pad to
 *     the byte, 00 00 FF FF; BFINAL 1 after the last segment), so every segment starts on a byte boundary.  A segment of n bytes
 *     whose dynamic block would be longer than 5 + n bytes is one stored block instead.
 *   LZ77: position p has the candidates p - 3, p - (1 + 3W) where that is inside the segment, and the largest q < p - p % 1024
 *     with hash(q) = hash(p), hash(x) = (le32(s[x .. x+4)) * 2654435761 mod 2^32) >> 19 for x + 4 <= n (a table of positions
 *     filled chunk by chunk of 1024 positions, a chunk seeing the chunks before it).  A candidate's length is the number of equal
 *     bytes, at most min(258, n - p); the longest wins, ties to the smallest distance; below 3 there is no match.  The parse is
 *     greedy from the segment's start.  Every token is a function of the segment's bytes alone.
 *   Huffman: 286 literal/length and 30 distance symbols, at most 15 bits.  Symbols with a non-zero count (end-of-block counts
 *     once; a distance histogram with fewer than two non-zero counts has symbols 0 and 1 raised to 1) are sorted by (count,
 *     symbol) and merged with two queues, the leaf first on equal weight.  Depths above 15 count as 15 and, while the Kraft sum
 *     exceeds 1, count[15] -= 1, the longest shorter length l in use gives count[l] -= 1, count[l+1] += 2.  Lengths are handed
 *     out by rank (the rarest symbols the longest), codes are canonical.  Block header: HLIT 286, HDIST 30, HCLEN 19; the
 *     code-length code is fixed and complete (lengths 0..12 in 4 bits, 13..18 in 5); all 316 lengths are sent literally.
 *   Size bound: a segment of n bytes takes at most n + 10 bytes, its chunk 12 more, so
 *     worst case(H, W) = 51 + S + 22 x ceil(S / 32768) bytes, S = H x (1 + 3W).  The scratch planned at create and the caller's
 *     out_cap are held to it: overflow cannot happen and is not a status code. */
typedef struct poco_png_encoder* poco_png_encoder_t;
/* The filtered stream, worst-case segment slots, lengths and Adler sums for frames up to max_h x max_w (1 .. 16384 each, else
 * POCO_ERR_ARG without touching the GPU).  Needs the GPU after validation. */
int poco_png_encoder_create(int max_h, int max_w, poco_png_encoder_t* out);
/* d_rgb uint8 [H,W,3] (any alignment) -> d_out[0 .. *d_len): three launches on `stream` - row filters, segment coding (the
 * segment staged in LDS), compaction with Adler combine and CRCs - with no allocation, no synchronisation and no global atomics;
 * nothing outside d_out[0 .. *d_len) and the word d_len is written.  POCO_ERR_ARG before any GPU work: a null handle or pointer,
 * H or W < 1 or above the created maximum, out_cap below worst case(H, W).  One encoder is used from one stream at a time. */
int poco_png_encode(poco_png_encoder_t enc, const unsigned char* d_rgb, int H, int W, unsigned char* d_out, size_t out_cap,
                    unsigned int* d_len, void* stream);
void poco_png_encoder_destroy(poco_png_encoder_t enc);

/* ---- PNG decoder: PNG input frames inflated and unfiltered on the device -----------------------------------------------------------
 * Replaces the host-side decode behind pocolib/core/tester.py:171 (cv2.imread + cvtColor per image of the folder) and :507
 * (cv2.imread per frame of the result video) for .png files - what the reference's ffmpeg extraction writes (%06d.png,
 * demo_utils.py:193); csrc/png_dec.hip, DESIGN.md 15.  Takes the IDAT payloads of up to max_batch parsed files (poco_amd/png.py
 * parse_png walks the chunks and checks their CRCs on the host), leaves one uint8 [H,W,3] RGB picture per file on the device: the
 * pixels of PIL's Image.open(f).convert("RGB"), restated in numpy by tests/pngdec_np.py.
 *   Files: bit depth 8; colour type 0 (grey), 2 (RGB), 3 (palette), 4 (grey + alpha), 6 (RGBA); no interlace; sides 1 .. 16384.
 *     Alpha is dropped, grey is replicated, a palette index reads the 256 x 3 table the caller pads with zeros.
 *   Inflate: one workgroup per image.  One lane walks the symbols (the serial part) from an input ring in LDS, stores literals
 *     into a 64 KiB output ring in LDS and queues matches as tokens; a second wave copies the matches of the batch before, in
 *     order, each by 64 lanes (dist < len by the modulo), reading LDS only; two more waves flush finished bytes to the image's
 *     filtered-stream scratch in whole dwords and refill the input ring.  The Huffman tables of a block are built in LDS by the
 *     workgroup.  Stored, fixed and dynamic blocks, any window size.  The Adler-32 is NOT verified (the IDAT CRCs checked by
 *     parse_png cover the same bytes).
 *   Unfilter: one launch per band of 64 rows, one wave per image; lane r undoes row y0 + r one pixel behind lane r - 1 and takes
 *     the pixel above from that lane.  The row above the first and the bpp bytes left of the first pixel are zeros; Average is
 *     (left + up) >> 1 on the 9-bit sum; Paeth breaks ties in the order left, up, up-left.
 *   Status: 0 only for a stream zlib's inflate accepts that yields exactly H x (1 + bpp x W) bytes with filter bytes 0 .. 4.
 *     Non-zero: block type 3, LEN != ~NLEN, HLIT > 286, HDIST > 30, a repeat with nothing to repeat or past HLIT + HDIST, no
 *     end-of-block code, an over-subscribed or incomplete code set (a single code of one bit excepted), literal/length symbols
 *     286 / 287, distance symbols 30 / 31, a distance beyond the bytes produced, input exhausted, another output size, a filter
 *     byte above 4.  The pixels of such an image are unspecified; the other images of the call are decoded.
 *   Safety: every stream read is clamped to the stream, every LDS index masked, every store compared with the image's scratch
 *     or its 3HW output bytes; every loop is bounded by a constant or a count validated on the host. */
typedef struct poco_png_decoder* poco_png_decoder_t;
/* One parsed file (all pointers on the host except d_rgb). */
typedef struct poco_png_image {
  const unsigned char* data;      /* the file's bytes */
  size_t nbytes;
  const unsigned int* idat;       /* [nidat][2]: offset into data and length of every IDAT payload, in file order */
  int nidat;
  int H, W, colour_type;          /* colour_type 0, 2, 3, 4 or 6 */
  unsigned char palette[768];     /* PLTE, padded with zeros (colour type 3) */
  unsigned char* d_rgb;           /* device: receives H * W * 3 bytes, any alignment */
} poco_png_image;
/* Device scratch (the filtered streams at 1 + 4 W bytes per row, two carry rows per image) and one pinned staging buffer for up to
 * max_batch images of up to max_h x max_w (1 .. 16384 each) whose deflate streams add up to at most max_bytes per call;
 * POCO_ERR_ARG without touching the GPU for sizes outside that, max_batch outside 1 .. 4096 or max_bytes outside 1 .. 2^30. */
int poco_png_decoder_create(int max_h, int max_w, int max_batch, size_t max_bytes, poco_png_decoder_t* out);
/* Decode imgs[0 .. n) in one call: the IDAT payloads of each image are copied end to end into the staging buffer, without chunk
 * framing, zlib header or Adler-32, each stream padded by 16 bytes, with the palettes and one descriptor per image; one
 * host-to-device copy, one memset and 1 + ceil(max H / 64) launches on `stream`; no allocation, no global atomics.  d_status int32
 * [n] on the device receives 0 or the non-zero status above; nothing outside the n pictures and d_status is written.  The only
 * host wait is for the previous call's copy out of the staging buffer.  POCO_ERR_ARG before any GPU work: null handle or
 * pointer, n outside 1 .. max_batch, a size outside the created maximum, a colour type outside {0, 2, 3, 4, 6}, an IDAT payload
 * outside the file or fewer than 6 payload bytes, or more stream bytes than max_bytes.  One decoder is used from one stream at a
 * time. */
int poco_png_decode(poco_png_decoder_t dec, const poco_png_image* imgs, int n, int* d_status, void* stream);
void poco_png_decoder_destroy(poco_png_decoder_t dec);

/* ---- evaluator: MPJPE, PA-MPJPE, V2V and the uncertainty / pose-error correlation of eval.py ---------------------------------
 * Replaces the host side of pocolib/core/trainer.py:298-336 (validation_step) and :365-391 (validation_epoch_end):
 * get_jnts_from_mesh, mpjpe_error, pampjpe_error (one np.linalg.svd per crop, in Python), vert_error, calculate_distance_pose,
 * calculate_pearson_coff (pocolib/utils/eval_utils.py:11-118,154-165), POCOUtils.prepare_uncert (poco_utils.py:21-25,62-94) and
 * SaveResults.accumulate_* (save_results.py:45-82); csrc/eval_metrics.hip.  Created once, stepped per batch, finished per run.
 *   Per crop (all sums and the Procrustes solve in fp64, stored as fp32):
 *     joints   = J_regressor @ vertices (eval_utils.py:66-69; base_dataset.py:359-360 for the ground truth), rows h_joint_map
 *                (constants.py:95-96 H36M_TO_J14 / H36M_TO_J17), minus row `pelvis` (eval_utils.py:70-73);
 *     MPJPE    = |pred - gt| per joint and its mean (eval_utils.py:99-102);
 *     PA-MPJPE = the same after the similarity transform s R x + t of the predicted onto the ground-truth joints
 *                (eval_utils.py:11-59,84-97): R = argmax over SO(3) of tr(R K), K = X1 X2^T, found as Horn's quaternion (largest
 *                eigenvector of a symmetric 4x4, cyclic Jacobi, a fixed number of sweeps) - the rotation the reference's SVD and Z
 *                sign fix select; s = tr(R K) / var1.  var1 = 0 gives Inf / NaN in the crop's PA fields, nothing else;
 *     V2V      = mean vertex distance (eval_utils.py:104-118), 0 with joint ground truth;
 *     pose distance [24] = mean squared difference of pred_pose and batch_rodrigues(gt_pose) per SMPL joint (eval_utils.py:154-160);
 *     processed uncertainty [24] = var_pose averaged over its trailing axes (innermost first), then, with `kinematic`,
 *                var[i] += var[parent(i)] for i = 1..23 (poco_utils.py:21-25,67-70,89-90), in fp32 like the host.
 *   Record of crop n = POCO_EVAL_RECORD_FLOATS fp32 (joint slots m >= M are 0):
 *     [0] MPJPE  [1] PA-MPJPE  [2] V2V  [3] 0  [4..36) MPJPE per joint  [36..68) PA-MPJPE per joint  [68..92) pose distance
 *     [92..116) processed uncertainty  [116..212) predicted joints, pelvis-relative [32,3]  [212..308) ground-truth joints [32,3]
 *     [308..404) predicted joints, not pelvis-relative [32,3]  [404..416) 0
 *   Summary = 8 doubles, reduced on the device in fp64 in a fixed order: [0] N  [1] 1000 mean MPJPE  [2] 1000 mean PA-MPJPE
 *     [3] 1000 mean V2V (trainer.py:375-376)  [4] Pearson r of (pose distance, processed uncertainty) over all crops and selected
 *     joints, centred: means first, then the three centred sums, clipped to [-1, 1] (scipy.stats.pearsonr, eval_utils.py:162-165)
 *     [5] number of pairs  [6], [7] 0.
 * One evaluator is used from one stream at a time (its partial-sum scratch is reused in stream order). */
#define POCO_EVAL_MAX_JOINTS 32
#define POCO_EVAL_RECORD_FLOATS 416
typedef struct poco_evaluator* poco_evaluator_t;
/* h_J_regressor fp32 [J,V] (host; dense or sparse - exact zeros are dropped, the rest is kept as CSR by row), 1 <= J <= 32,
 * 1 <= V <= 2^22; h_joint_map int32 [M], 1 <= M <= J, entries and `pelvis` in [0, J); h_sel_uncert int32 [num_sel] = the SMPL
 * joints that enter the correlation (sel_uncert_part, save_results.py:19; entries in [0, 24); num_sel = 0: all 24); kinematic =
 * POCO.KINEMATIC_UNCERT; capacity = records the evaluator can hold (1 .. 2^24).  Host only, like poco_create: everything is
 * validated here; the first step uploads the tables and allocates the records (1664 bytes each) and the scratch. */
int poco_evaluator_create(const float* h_J_regressor, int J, int V, const int32_t* h_joint_map, int M, int pelvis,
                          const int32_t* h_sel_uncert, int num_sel, int kinematic, int64_t capacity, poco_evaluator_t* out);
/* Records of B crops at records[first .. first + B), first += B.  d_pred_vertices [B,V,3] (smpl_vertices), exactly one of
 * d_gt_vertices [B,V,3] (3DPW: joints regressed from it, V2V) and d_gt_joints [B,M,3] (H36M / MPI-INF-3DHP: used as they are),
 * d_pred_pose [B,24,3,3], d_gt_pose [B,72] axis-angle, d_var_pose [B,24,var_t1,var_t2] (the engine's [B,24]: var_t1 = var_t2 = 1).
 * Argument errors - a null handle or pointer, B <= 0, both or neither ground truth, first + B > capacity - return POCO_ERR_ARG
 * before any GPU work and leave the records as they were.  Enqueued on `stream` (two launches per 256 crops), safe right behind
 * poco_forward on the same stream: no synchronisation and, after the first step, no allocation. */
int poco_evaluator_step(poco_evaluator_t e, int B, const float* d_pred_vertices, const float* d_gt_vertices,
                        const float* d_gt_joints, const float* d_pred_pose, const float* d_gt_pose, const float* d_var_pose,
                        int var_t1, int var_t2, void* stream);
/* Reduce the N records written so far into h_summary8 (host, 8 doubles) and, if h_records is not NULL, copy the records to it
 * (host fp32 [records_cap, POCO_EVAL_RECORD_FLOATS], records_cap >= N).  Synchronises `stream`.  N = 0 is POCO_ERR_STATE. */
int poco_evaluator_finish(poco_evaluator_t e, double* h_summary8, float* h_records, int64_t records_cap, void* stream);
/* Var-MPJPE and Variance of pocolib/core/trainer.py:374,377-378,389-390 over the records written so far, which are only read:
 *     u_i = mean over the 24 joints of the processed uncertainty of crop i (POCOUtils.accumulate_uncert('val', ...) returns
 *           prepare_uncert(var_pose).mean(1), poco_utils.py:151-169,265-281)
 *     h_summary2[0] = Var-MPJPE = mean_i(MPJPE_i / (u_i + 1e-9))     [1] = Variance = mean_i(u_i)
 * in fp64 from the stored fp32 fields, in metres (the reference does not scale these two by 1000).  One block, fixed order.
 * Synchronises `stream`.  No step yet is POCO_ERR_STATE. */
int poco_evaluator_uncert_summary(poco_evaluator_t e, double* h_summary2, void* stream);
/* Keys and value planes for poco_op_rank_curve from the N records written so far, which are only read; nothing leaves the device.
 *   mode 0 (per crop):  n = N, E = 3.  d_key[i] = u_i of poco_evaluator_uncert_summary (the 24 stored values added in joint order
 *                       in fp64, divided by 24, rounded once to fp32); d_vals = [MPJPE | PA-MPJPE | V2V] of the crop, [3][n], in
 *                       the records' units (metres).
 *   mode 1 (per joint): n = N * |sel|, E = 1.  d_key = the processed uncertainty and d_vals the pose distance of the selected
 *                       joints, flattened crop-major (entry i * |sel| + k = selected joint k of crop i): the corr_y / corr_x of
 *                       poco_evaluator_finish's records.
 * d_key holds `cap` floats and d_vals E planes of n floats, dense; *h_n and *h_E (host) are written before the call returns.
 * One launch on `stream`, no synchronisation.  POCO_ERR_ARG: a null pointer, a mode outside {0, 1}, cap < n (then *h_n and *h_E
 * are still written, so that the caller learns the size).  No step yet is POCO_ERR_STATE. */
int poco_evaluator_rank_inputs(poco_evaluator_t e, int mode, float* d_key, float* d_vals, int64_t cap, int64_t* h_n, int* h_E,
                               void* stream);
/* Rewind: the next step writes record 0. */
int poco_evaluator_reset(poco_evaluator_t e);
void poco_evaluator_destroy(poco_evaluator_t e);

/* ---- pseudo-labeler: confident predictions as records of the reference's dataset .npz ---------------------------------------
 * The writer of the file pocolib/dataset/base_dataset.py:54-147 reads ("If the dataset is inferred from POCO, select confident
 * frames", :59-70); the released reference declares its accumulators (pocolib/core/tester.py:163) and never fills them;
 * csrc/pseudo_gt.hip.  Created once, stepped per batch behind the forward, finished per run.
 *   Record of a kept crop = POCO_PSEUDO_RECORD_FLOATS fp32 words:
 *     [0]        source_id, the caller's int32 passed through as bits
 *     [1..3)     center = (cx, cy) of the box                     [3] scale = max(w, h) / 200 (tester.py:194-196)
 *     [4..76)    pose [72] = rotation_matrix_to_angle_axis of the 24 predicted matrices (poco_op_rotmat_to_aa's device function)
 *     [76..86)   shape [10] = pred_shape
 *     [86..110)  var [24] = var_pose averaged over its trailing elements in the order numpy's float32 mean adds them (what
 *                postproc.prepare_uncert gives), NOT accumulated along the kinematic tree: the reader does that on load
 *     [110..185) openpose [25,3] = joints2d[:25], confidence 1     [185..257) part [24,3] = joints2d[25:], confidence 1
 *                (tester.py:232-233); with joints_in_crop the points first go through convert_crop_coords_to_orig_img
 *                (pocolib/utils/demo_utils.py:268-281: box side = w), in its float32 operations
 *     [257..353) S [24,4] = joints3d[25:], confidence 1            [353..384) 0
 *   Selection = get_confident_frames (pocolib/utils/train_utils.py:31-45): var accumulated along the kinematic tree
 *     (poco_utils.py:21-25), kept if column 0 < threshold; a NaN compares false and the crop is dropped.
 *   Kept crops are appended in source order - within a step and from step to step - by a prefix sum, not by atomics; the running
 *   count lives on the device.  Record memory that no kept crop has reached holds POCO_PSEUDO_UNWRITTEN in every word.
 * One labeler is used from one stream at a time. */
#define POCO_PSEUDO_RECORD_FLOATS 384
#define POCO_PSEUDO_MAX_TRAILING 128
#define POCO_PSEUDO_UNWRITTEN 0xFFFFFFFFu
typedef struct poco_pseudo* poco_pseudo_t;
/* capacity = crops that may be OFFERED (1 .. 2^24; the kept count is not known on the host); threshold: NaN or <= 0 = keep every
 * crop; joints_in_crop = 1 for the PARE variants (smpl_joints2d in crop coordinates), 0 for the CLIFF variants (image coordinates);
 * crop_res = DATASET.IMG_RES (1 .. 16384).  Host only: everything is validated here; the first step allocates the records
 * (1536 bytes each) and a destination word per crop. */
int poco_pseudo_create(int64_t capacity, float threshold, int joints_in_crop, int crop_res, poco_pseudo_t* out);
/* Offer B crops: d_pred_pose [B,24,3,3], d_pred_shape [B,10], d_var_pose [B,24,var_t] (the engine's [B,24]: var_t = 1; at most
 * POCO_PSEUDO_MAX_TRAILING), d_joints2d [B,49,2], d_joints3d [B,49,3], d_boxes [B,4] = cx, cy, w, h, d_source_id int32 [B].
 * Argument errors - a null handle or pointer, B < 1, var_t outside 1..128, offered + B > capacity - return POCO_ERR_ARG before any
 * GPU work and leave the records and counts as they were.  Enqueued on `stream` (two launches whatever B is), safe right behind
 * poco_forward on the same stream: no synchronisation, nothing read back and, after the first step, no allocation. */
int poco_pseudo_step(poco_pseudo_t p, int B, const float* d_pred_pose, const float* d_pred_shape, const float* d_var_pose, int var_t,
                     const float* d_joints2d, const float* d_joints3d, const float* d_boxes, const int32_t* d_source_id,
                     void* stream);
/* *n_offered, *n_kept and, if h_records is not NULL, the record memory of every offered crop (host fp32 [records_cap,
 * POCO_PSEUDO_RECORD_FLOATS], records_cap >= *n_offered): the first *n_kept records are the kept crops, the rest is unwritten.
 * Two copies on `stream`, then one synchronisation.  Before the first step: both counts 0 and no GPU work. */
int poco_pseudo_finish(poco_pseudo_t p, float* h_records, int64_t records_cap, int64_t* n_kept, int64_t* n_offered, void* stream);
/* Rewind, enqueued on `stream`: both counts 0, the records unwritten again. */
int poco_pseudo_reset(poco_pseudo_t p, void* stream);
void poco_pseudo_destroy(poco_pseudo_t p);

/* ---- body-part segmentation: SMPL part labels in the crop, the crop camera, and the score of PARE's mask ------------------------
 * What the reference trains pred_segm_mask against (pocolib/core/trainer.py:231-262) and scores it with
 * (pocolib/losses/segmentation.py:CrossEntropy); csrc/part_labels.hip, csrc/segm_metrics.hip; DESIGN.md section 21;
 * tests/segm_np.py restates all of it in numpy.
 *
 * poco_op_part_labels: d_labels uint8 [B,res,res] <- the body part seen at every pixel centre of B crops, 0 = background.
 *   d_verts [B,V,3], d_cam_t [B,3], d_faces int32 [F,3], d_face_part uint8 [F] (part 0..23 of each face), d_keys = B * res * res
 *   64-bit words of scratch (set and consumed by the call).
 *   Camera (geometry.py:480-508 perspective_projection, identity rotation, y down): (X, Y, Z) = v + cam_t,
 *     x = focal * X / Z + res / 2, y = focal * Y / Z + res / 2, all in float32 in this order; pixel (r, c) is sampled at (c + 0.5, r + 0.5).
 *   Coverage: the watertight edge rule of the demo renderer (csrc/raster_common.h): a centre on a shared edge or vertex belongs to
 *     exactly one of the triangles around it.  Both windings are filled.  A face with a non-finite vertex, with a vertex at Z < 0.1,
 *     of zero area or with an index outside [0, V) covers nothing.
 *   Visibility: z of a fragment = 1 / ((w0 / z0 + w1 / z1 + w2 / z2) / area) with the edge values w at the centre (1 / z is linear in
 *     screen space); the nearest fragment wins, at equal depth the lower face index: atomicMin of (float bits of z << 32 | face).
 *   Label = d_face_part[winner] + 1: what the reference's bucketize(...) + 1 followed by * mask reduces to.
 *   Two launches (per (crop, face), then per pixel) behind one memset, all on `stream`; no allocation, no synchronisation. */
int poco_op_part_labels(const float* d_verts, int B, int V, const float* d_cam_t, const int32_t* d_faces, int F,
                        const unsigned char* d_face_part, float focal, int res, unsigned long long* d_keys, unsigned char* d_labels,
                        void* stream);
/* poco_op_part_visibility (eval.py --visibility; csrc/part_visibility.hip; tests/visibility_np.py restates it):
 *   d_counts int32 [B,24,4] <- per crop and body part p the pixel counts (total, area, front, seen).
 *   d_verts, d_cam_t, d_faces, d_face_part, focal, res: as for poco_op_part_labels, and so are the camera, the pixel-centre sampling,
 *   the coverage rule (both windings filled), the face exclusions (a non-finite vertex, Z < 0.1, zero area, an index outside
 *   [0, V)) and the depth rule (the nearest fragment wins, at equal depth the lower face index).  A fragment is a covered centre
 *   whose interpolated depth is finite and positive, as poco_op_part_labels draws it.
 *   Window and frame: the frame is the crop, the pixel lattice [0, res)^2; the window is the lattice [-margin, res + margin)^2,
 *   0 <= margin <= res.  A face is walked over its bounding box clipped to the WINDOW: body outside the window is not counted at
 *   all, so `margin` bounds the truncation that can be measured - a part of which more than the margin lies beyond the crop's
 *   border has a `total` that is too small and a vis_frame = area / total that is too large.
 *     total[p]  window pixel centres covered by at least one fragment of part p.  No depth test; a centre covered by several faces
 *               of p (front and back surface, faces that meet in an edge) counts once.
 *     area[p]   the same count restricted to the frame.
 *     front[p]  frame pixels whose nearest fragment belongs to part p = the pixels with label p + 1 in poco_op_part_labels' output
 *               for the same input.
 *     seen[p]   the front pixels at which d_occ_mask (uint8 [B,res,res], e.g. poco_dataset_crop_occ_mask's) is 0; NULL = all zeros.
 *   A part that covers nothing gives four zeros.  seen <= front <= area <= total.
 *   h_face_part: the host copy of d_face_part, or NULL.  Given, a part above 23 is POCO_ERR_ARG; the kernel clamps a part above 23
 *   to 23 either way, so it is memory-safe for any device content (indices, parts, vertices, mask).
 *   d_scratch: poco_op_part_visibility_scratch_bytes(B, res, margin) bytes, 8-byte aligned, set and consumed by the call (the depth
 *   keys of the frame, then one 32-bit word of part bits per window pixel); the helper returns 0 for arguments the operator refuses.
 *   POCO_ERR_ARG before any GPU work, outputs untouched: a null pointer (but h_face_part, d_occ_mask), B outside 1..65535, V or F
 *   outside 1..2^24, res outside 1..4096, margin outside 0..res, a focal that is not finite and > 0, a misaligned scratch.
 *   Three memsets (keys, bits, counts) and two launches (per (crop, face): atomicOr of 1 << part per covered window pixel, atomicMin
 *   of the depth key per covered frame pixel; per window pixel: wave ballots and popcounts, one global integer add per (part,
 *   counter) and block) on `stream`; no allocation, no synchronisation.  Every output word is written; integer sums, so two runs
 *   give equal bits. */
size_t poco_op_part_visibility_scratch_bytes(int B, int res, int margin);
int poco_op_part_visibility(const float* d_verts, int B, int V, const float* d_cam_t, const int32_t* d_faces, int F,
                            const unsigned char* d_face_part, const unsigned char* h_face_part, float focal, int res, int margin,
                            const unsigned char* d_occ_mask, void* d_scratch, int32_t* d_counts, void* stream);
/* geometry.py:511-551 estimate_translation_np per crop: d_cam_t [B,3] <- the translation that brings d_joints3d [B,J,3] closest to
 * d_joints2d [B,J,3] = (x, y, confidence) in crop pixels under the camera above, by the weighted 3x3 normal equations.  The weight
 * sqrt(confidence) is taken in float32 as the reference takes it; products and sums are fp64, added in joint order; the system is
 * solved by Cramer's rule in fp64.  A determinant that is zero (or not finite) gives (1, 1, 1), the reference's `except` branch.
 * One wave per crop, one launch.  J <= POCO_EST_TRANSLATION_MAX_J. */
#define POCO_EST_TRANSLATION_MAX_J 64
int poco_op_estimate_translation(const float* d_joints3d, const float* d_joints2d, int B, int J, float focal, int res,
                                 float* d_cam_t, void* stream);
/* poco_op_segm_score: d_records [B, POCO_SEGM_RECORD_WORDS(C)] 64-bit words <- per crop
 *     [0]          the sum over the H * W label pixels of -log_softmax(upsampled logits)[label], an fp64 value
 *     [1]          pixels whose argmax equals the label (integer, as all that follow)
 *     [2 + 3c ..)  class c: pixels with argmax == label == c, pixels with argmax == c, pixels with label == c
 *   d_logits [B,C,h,w] (pred_segm_mask), d_labels uint8 [B,H,W] with every label < C (a label >= C is counted nowhere).
 *   Upsample: bilinear, align_corners=True: source coordinate s = scale * i with scale = float(n_src - 1) / float(n_dst - 1) (0 when
 *     n_dst = 1), i0 = int(s), i1 = min(i0 + 1, n_src - 1), l = s - i0, h = 1 - l, value = hy * (hx * v00 + lx * v01) + ly * (hx * v10 +
 *     lx * v11), float32, not contracted.  Argmax: the lowest channel wins a tie.  Loss: (max + logf(sum expf(v - max))) - v[label].
 *   The integer words are exact; word 0 is summed in fp64 in a fixed order: the same input gives the same bits on every run.
 *   d_partials: B * poco_op_segm_score_partials(h, H) doubles of scratch.  C <= POCO_SEGM_MAX_C, C * w <= 3750 (four source rows of
 *   every channel are staged in LDS).  No assumption on H / h.  A memset and two launches on `stream`. */
#define POCO_SEGM_MAX_C 32
#define POCO_SEGM_RECORD_WORDS(C) (2 + 3 * (C))
int poco_op_segm_score_partials(int h, int H);
int poco_op_segm_score(const float* d_logits, int B, int C, int h, int w, const unsigned char* d_labels, int H, int W,
                       unsigned long long* d_records, double* d_partials, void* stream);
/* d_out uint8 [B,H,W] <- the argmax poco_op_segm_score takes at every pixel (the same interpolation and tie rule). */
int poco_op_segm_argmax(const float* d_logits, int B, int C, int h, int w, int H, int W, unsigned char* d_out, void* stream);

/* ---- video mode's in-fill: unreliable joint rotations of a track from the confident frames around them -------------------------
 * demo.py --mode video --infill THRESH; csrc/track_infill.hip; tests/infill_np.py restates it in float64
 * numpy.  No counterpart in the reference's code (the paper repairs occluded frames with external motion models).
 *
 * poco_op_track_infill: P tracks concatenated into N rows, track p = rows [d_offsets[p], d_offsets[p + 1]).
 *   d_offsets int32 [P+1] (0 = first, N = last, strictly increasing: the CALLER checks this; the kernel only clamps it to 0..N),
 *   d_frames int32 [N] (the tracks' frame indices, strictly increasing within a track, holes allowed), d_pose [N,24,3,3] (proper
 *   rotations), d_u [N,24] (the post-processed uncertainty), d_lin [N,L] with 0 <= L <= POCO_INFILL_MAX_LIN (NULL iff L = 0;
 *   the demo passes betas | orig_cam, L = 14), thresh, max_gap >= 1, d_scratch = 24 * N int32 words (set and consumed by the call).
 *   Reliable: entry (t, j) is reliable iff u[t][j] <= thresh; a NaN compares false and counts as unreliable.
 *   Per unreliable entry, within its own track only: a = the last reliable row before t in column j, b = the first after (either
 *   may be absent).
 *     1. both exist and frames[b] - frames[a] <= max_gap: R' = R(slerp(q_a, q_b, s)), s = (frames[t] - frames[a]) / (frames[b] -
 *        frames[a]); flag 1.
 *     2. otherwise c = the existing anchor nearer in frames (a tie goes to a); if |frames[t] - frames[c]| <= max_gap / 2 (integer
 *        division): R' = R[c], copied bit for bit; flag 2.
 *     3. otherwise the entry is copied bit for bit from the input; flag 3.
 *   Reliable entries: flag 0, copied bit for bit.
 *   Arithmetic: fp64, rounded once to fp32 on store (as poco_op_rotmat_to_aa).  Matrix -> quaternion by the largest of (trace, m00,
 *   m11, m22), the first of equals, then normalised; q_b is negated when q_a.q_b < 0; |q_a.q_b| > 1 - 1e-12: the normalised linear
 *   blend, else sin((1 - s) th) / sin(th) and sin(s th) / sin(th) with th = acos(q_a.q_b); quaternion -> matrix in the standard form.
 *   Linear block: row t of d_lin follows column 0's decision: flag 1: lin[a] + s (lin[b] - lin[a]) in fp64; flag 2: a copy of
 *   lin[c]; else a copy of the row.
 *   Outputs (every element is written; none may alias an input): d_pose_out [N,24,3,3], d_lin_out [N,L], d_flags uint8 [N,24],
 *   d_touched uint8 [N] = 1 where any flag of the row is 1 or 2, and - both or neither - d_rows int32 [N] whose first *d_count
 *   words are the touched rows in ascending order (the rest is left alone) and d_count int32 [1].
 *   Two launches on `stream` whatever P is (one wave per (track, joint) column, then one block over the rows); no allocation, no
 *   synchronisation, no atomics: the same input gives the same bits on every run and for every split into calls.
 *   POCO_ERR_ARG before any GPU work: a null pointer, P < 1, N < P, 24 * 9 * N >= 2^31, L outside 0..16, max_gap < 1, one of
 *   d_rows / d_count without the other. */
#define POCO_INFILL_MAX_LIN 16
int poco_op_track_infill(const float* d_pose, const float* d_u, const int32_t* d_frames, const int32_t* d_offsets, int P, int N,
                         const float* d_lin, int L, float thresh, int max_gap, int32_t* d_scratch, float* d_pose_out,
                         float* d_lin_out, unsigned char* d_flags, unsigned char* d_touched, int32_t* d_rows, int32_t* d_count,
                         void* stream);

/* ---- choosing between two regressors by their own uncertainty ---------------------------------------------------------------------
 * demo.py / eval.py --cfg2 --ckpt2 --select crop|joint; csrc/select_regressor.hip; tests/select_np.py restates
 * it in float64 numpy with plain loops.  No counterpart in the reference's code (the paper's comparison was offline); the
 * uncertainty post-processing it decides on is pocolib/utils/poco_utils.py:21-25,50-60.
 *
 * poco_op_select_regressor: models m = 0, 1 over B rows.  d_pose_m [B,24,3,3], d_var_m [B,24] (the raw var_pose), kind_m: 0 = the
 *   "mean" rule (pare), 1 = the "root" rule (cliff); kinematic 0 | 1, thr, scale > 0 (multiplies model 1's uncertainty), mode 0 =
 *   crop, 1 = joint; `payloads`: up to POCO_SELECT_MAX_PAYLOADS arrays of `width` floats per row, each with its two sources and
 *   its destination.  All buffers dense and caller-owned; no output may alias an input.
 *   Processed uncertainty: u_m[t][j] = var_m[t][j]; with kinematic u[child] = var[child] + u[parent] in child order 1..23, fp32
 *   additions (poco_utils.py:21-25).
 *   Crop score, fp64 from the fp32 u: kind 1: g = u[0] > 2 thr ? 1 : u[0]; kind 0: g = u[0] > thr ? 1 : (u[0] + ... + u[23], in
 *   joint order) / 24 (poco_utils.py:50-60; the fp64 mean and comparison differ from numpy's fp32 pairwise mean by at most one
 *   rounding: chosen so that kernel and restatement agree bit for bit).  s_0 = g_0, s_1 = scale g_1.
 *   mode 0: row t takes model 1 iff s_1 < s_0 (a tie and a NaN on either side: model 0); all 24 entries of choice[t] are that.
 *   mode 1: entry (t, j) takes model 1 iff scale (double)u_1[t][j] < (double)u_0[t][j], same tie and NaN rule, no 1.0 rule.
 *   Outputs (every element is written): d_pose_out [B,24,3,3] and d_var_out [B,24] = the chosen model's nine floats / one float
 *   per entry, bit for bit; every payload row = a bit-for-bit copy from the model chosen for joint 0; d_choice uint8 [B,24];
 *   d_score fp32 [B,2] = s_0, s_1 rounded once (a NaN is stored as 0x7fc00000), in both modes; d_mixed uint8 [B] = 1 where the
 *   24 choices of the row are not all equal (never in mode 0); and - both or neither - d_rows int32 [B] whose first *d_count
 *   words are the mixed rows in ascending order (the rest is left alone) and d_count int32 [1].
 *   max_blocks: 0 = the default grid, > 0 bounds the first launch's grid; the result does not depend on it.
 *   Two launches on `stream` (one block per row, grid-stride; one block over the rows); no allocation, no synchronisation, no
 *   atomics.  Payload rows are copied with the widest accesses the row's own addresses allow (16, 8 or 4 bytes): no alignment
 *   beyond a float's is assumed.
 *   POCO_ERR_ARG before any GPU work: a null pointer (a payload's included), B outside 1..2^24, mode, kind or kinematic
 *   outside {0, 1}, scale not finite or <= 0, a payload count outside 0..8, a payload width outside 1..2^24, an output equal to
 *   an input, one of d_rows / d_count without the other. */
#define POCO_SELECT_MAX_PAYLOADS 8
typedef struct {
  const float* src0;  /* [B, width] of model 0                                                                           */
  const float* src1;  /* [B, width] of model 1                                                                           */
  float* dst;         /* [B, width]                                                                                      */
  int64_t width;      /* floats per row, 1 .. 2^24                                                                       */
} poco_select_payload_t;
typedef struct {
  int64_t count;                                        /* payloads in use, 0 .. POCO_SELECT_MAX_PAYLOADS               */
  poco_select_payload_t p[POCO_SELECT_MAX_PAYLOADS];
} poco_select_payloads_t;                               /* passed by value                                              */
int poco_op_select_regressor(const float* d_pose0, const float* d_var0, int kind0, const float* d_pose1, const float* d_var1,
                             int kind1, int B, int kinematic, double thr, double scale, int mode, poco_select_payloads_t payloads,
                             float* d_pose_out, float* d_var_out, unsigned char* d_choice, float* d_score, unsigned char* d_mixed,
                             int32_t* d_rows, int32_t* d_count, int max_blocks, void* stream);

/* ---- test-time augmentation: fusing K views of a crop by their uncertainty -----------------------------------------------------------
 * eval.py / demo.py --tta VIEWS [--tta_weight uncert|uniform]; csrc/tta_fuse.hip; poco_amd/tta.py; DESIGN.md section 26;
 * tests/tta_np.py restates it in float64 numpy with plain loops.  No counterpart in the reference's code; the transforms it undoes
 * are flip_pose and rot_aa (pocolib/utils/image_utils.py:236-247,269-278) in the order of pose_processing (base_dataset.py:253-262).
 *
 * poco_op_tta_fuse: K views of B crops, view-major: row k * B + b is view k of crop b.  d_pose [K*B,24,3,3], d_var [K*B,24] (the
 *   raw var_pose), d_betas [K*B,10], all fp32, dense and caller-owned.  `views` (by value): K in 2..8 and per view flip (0 | 1) and
 *   c, s = cos and sin of +rot degrees, formed by the host in float64 (rot = 0: exactly 1 and 0).  View 0 is the identity.
 *   weight: 0 = uniform, 1 = uncertainty.
 *   Per (b, j), in fp64, nothing fused, views in order:
 *     js = flip_k ? SMPL_JOINTS_FLIP_PERM[j] : j;  R_k = pose[k,b,js];  flip: R_k[i][c] *= m_i m_c, m = (1,-1,-1);
 *     j = 0 and (c_k, s_k) != (1, 0): R_k = Rz R_k, Rz = [[c,-s,0],[s,c,0],[0,0,1]] (after the un-flip);
 *     v_k = var[k,b,js];  w_k = 1 (uniform) | 1 / ((double)v_k + 1e-9) (uncertainty);  w_k = 0 where v_k is not finite or is
 *     negative or R_k holds a non-finite value (such a view enters no sum);
 *     M = sum w_k R_k, W = sum w_k;  R' = argmax over SO(3) of tr(R^T M) (Horn's quaternion form, the largest eigenvector of a
 *     symmetric 4x4 by cyclic Jacobi with the 10 fixed sweeps of csrc/eval_metrics.hip);
 *     var' = (sum w_k v_k) / W;  spread = (sum_k w_k mean9((R_k - R')^2)) / W.
 *     W = 0 (every view dropped): pose' and var' are the base view's words, bit for bit, and spread is NaN (0x7fc00000).
 *   Per crop: betas' = (sum g_k betas_k) / sum g_k with g_k the joint-0 weight of view k; sum g_k = 0: the base view's words.
 *   Outputs, fp32, each rounded once, every element written: d_pose_out [B,24,3,3], d_var_out [B,24], d_spread [B,24],
 *   d_betas_out [B,10].
 *   max_blocks: 0 = the default grid, > 0 bounds it; the result does not depend on it.
 *   One launch on `stream` (one lane per (crop, joint), grid-stride); no allocation, no synchronisation, no atomics.
 *   POCO_ERR_ARG before any GPU work: a null pointer, K outside 2..8, B outside 1..2^24, weight outside {0, 1}, a flip outside
 *   {0, 1}, c or s not finite or |c^2 + s^2 - 1| > 1e-12, view 0 not the identity, an output that overlaps an input or another
 *   output. */
#define POCO_TTA_MAX_VIEWS 8
typedef struct {
  int32_t flip;       /* 0 | 1: the view was mirrored left-right                                                          */
  int32_t pad_;
  double c, s;        /* cos and sin of +rot degrees                                                                      */
} poco_tta_view_t;
typedef struct {
  int64_t count;                                        /* views in use, 2 .. POCO_TTA_MAX_VIEWS; view 0 is the identity  */
  poco_tta_view_t v[POCO_TTA_MAX_VIEWS];
} poco_tta_views_t;                                     /* passed by value                                                */
int poco_op_tta_fuse(const float* d_pose, const float* d_var, const float* d_betas, int B, poco_tta_views_t views, int weight,
                     float* d_pose_out, float* d_var_out, float* d_spread, float* d_betas_out, int max_blocks, void* stream);

/* ---- rank-based uncertainty metrics: stable key sort, midranks, fp64 sums at K + 1 cuts ------------------------------------------------
 * eval.py --rank_metrics [--rank_bins K]; csrc/rank_curve.hip; poco_amd/ranking.py; tests/rank_np.py restates
 * it in float64 with plain loops.  No counterpart in the reference's code, which reports Pearson's r only (trainer.py:380).
 *
 * poco_op_rank_curve: n keys (fp32) and E value planes d_vals [E][n] (fp32; NULL if E = 0), dense, caller-owned, on the device.
 *   A key is canonicalised first: -0.0 becomes +0.0 and every NaN becomes 0x7fc00000, so NaN sorts last; its order-preserving
 *   uint32 image is ~bits for a negative key and bits | 0x80000000 otherwise.
 *   d_order [n] int32 = the stable ascending order of the canonical keys: numpy.argsort(key, kind="stable").  Least-significant-
 *     digit radix sort, 4 passes of 8 bits, row index as payload, tiles of POCO_RANK_TILE rows.
 *   d_rank [n] fp64 = the 1-based midrank of row i: rows with equal canonical keys share the mean of their sorted positions
 *     (scipy.stats.rankdata(method="average")).
 *   d_cuts [E + 1][K + 1] fp64: cuts[e][k] = the sum of plane e over the sorted positions [0, c_k), c_k = floor(k n / K) in 64-bit
 *     integers.  Plane 0 = the canonical key widened to fp64, plane e >= 1 = d_vals[e - 1].  prefix(c) = (scan of the totals of the
 *     tiles before tile c / T) + (strided per-lane sums and a halving tree over the first c % T rows of that tile): the summation
 *     tree is a function of c and n alone.  fp64 additions only, no floating-point atomics.
 *   d_cut_keys [K + 1] fp32: the canonical sorted key at position max(c_k, 1) - 1 = the threshold that keeps the first c_k rows.
 *   d_scratch: at least poco_op_rank_curve_scratch_bytes(n, E) bytes (0 = n or E out of range), 8-byte aligned; its contents
 *     before and after the call mean nothing.
 *   max_blocks: 0 = the default grid, > 0 bounds it.  All four outputs are bitwise independent of it and equal from run to run.
 *   16 launches on `stream`; no allocation, no synchronisation, the inputs are only read.
 *   POCO_ERR_ARG before any GPU work: a null pointer, n outside 1..2^24, E outside 0..4, K outside 1..1024, max_blocks < 0, a
 *   scratch buffer that is too small, misaligned buffers, scratch or outputs that overlap an input or each other.
 *
 * poco_op_pearson64: d_r[0] = Pearson's r of the fp64 device arrays d_x and d_y [n], n in 1..2^24: means first, then the three
 *   centred sums and one division, clipped to [-1, 1] as poco_evaluator_finish clips; NaN if every element of either array equals
 *   its first.  One block of 1024 lanes in a fixed order, so the result cannot depend on max_blocks (>= 0, accepted so that the
 *   call reads like its neighbours).  Spearman's rho = poco_op_pearson64 of two d_rank arrays.  One launch on `stream`. */
#define POCO_RANK_TILE 2048
#define POCO_RANK_MAX_N (1 << 24)
#define POCO_RANK_MAX_PLANES 4
#define POCO_RANK_MAX_CUTS 1024
size_t poco_op_rank_curve_scratch_bytes(int64_t n, int E);
int poco_op_rank_curve(const float* d_key, const float* d_vals, int64_t n, int E, int K, void* d_scratch, size_t scratch_bytes,
                       int32_t* d_order, double* d_rank, double* d_cuts, float* d_cut_keys, int max_blocks, void* stream);
int poco_op_pearson64(const double* d_x, const double* d_y, int64_t n, double* d_r, int max_blocks, void* stream);

/* ---- video mode's uncertainty-weighted smoother: each track smoothed over time, the data term weighted by the precision -------
 * demo.py --mode video --smooth_uncert LAMBDA; csrc/track_smooth.hip; tests/usmooth_np.py restates it in
 * float64 numpy with a dense solve.  No counterpart in the reference (its --smooth is the causal one-euro filter on the host).
 *
 * poco_op_track_smooth: P tracks concatenated into N rows as for poco_op_track_infill: d_offsets int32 [P+1] (0 = first, N = last,
 *   strictly increasing: the CALLER checks this; the kernel only clamps it to 0..N), d_frames int32 [N] (strictly increasing within
 *   a track, holes allowed), d_pose [N,24,3,3] (finite), d_u [N,24] (the post-processed uncertainty), d_lin [N,L] with 0 <= L <=
 *   POCO_SMOOTH_MAX_LIN (NULL iff L = 0; the demo passes betas | orig_cam, L = 14), lam in (0, 1e4], u_ref finite and > 0,
 *   max_gap >= 1.
 *   Per track (rows t = 0 .. T-1, frames f_t) and per joint j:
 *     weight     w_t = clamp((u_ref / max(u[t][j], 1e-6))^2, 1e-6, 1e6); a NaN or an infinity of either sign gives 1e-6.
 *     curvature  for 1 <= t <= T-2 with h1 = f_t - f_(t-1) and h2 = f_(t+1) - f_t both in 1..max_gap: row t of D is
 *                (2 / (h1 (h1 + h2)), -2 / (h1 h2), 2 / (h2 (h1 + h2))) at columns t-1, t, t+1, its weight omega_t = (h1 + h2) / 2
 *                (unit spacing: (1, -2, 1), omega 1).  Every other row of D is zero: no penalty across a hole wider than max_gap.
 *     solve      A = diag(w) + lam D^T Omega D (pentadiagonal, symmetric positive definite whatever the data); A X = diag(w) Y for
 *                the nine entries of joint j's matrices; each solved 3x3 M is replaced by the rotation nearest to it: Horn's
 *                quaternion, the largest eigenvector of the symmetric 4x4 by cyclic Jacobi with 10 fixed sweeps, as
 *                poco_op_tta_fuse.  T <= 2 has no penalty row: the output is the projected input.
 *     shift      the angle in degrees between the input matrix A and the output R (before its rounding):
 *                atan2(|skew(A^T R)| / 2, (trace(A^T R) - 1) / 2), skew = (Q21 - Q12, Q02 - Q20, Q10 - Q01).
 *   Linear block: the L columns of d_lin are solved with joint 0's A and are not projected.
 *   Arithmetic: fp64 throughout, rounded once to fp32 on store; banded L D L^T without pivoting (two sub-diagonals), forward and
 *   backward substitution.  lam is capped at 1e4 because the factor's deviation from a dense fp64 solve grows with it (1e-12 for
 *   lam <= 100, 1.2e-10 at 1e4, 1.4e-8 at 1e6 on random tracks).
 *   Outputs (every element is written; none may alias an input): d_pose_out [N,24,3,3], d_lin_out [N,L], d_shift [N,24].
 *   d_scratch: POCO_SMOOTH_SCRATCH_DOUBLES(N, L) doubles, caller-owned, set and consumed by the call (per row the 216 + L substituted
 *   right-hand sides, then the solution in their place, and two sub-diagonal words for each of the 24 joints and the linear block).
 *   One launch on `stream` whatever P is (a block per (track, 7 joints): one wave solves, one lane per column; four waves project);
 *   max_blocks > 0 caps the grid (tests).  No allocation, no synchronisation, no atomics: a track's output bits do not depend on
 *   the other tracks in the buffer or on the grid, and two runs give the same bits.
 *   POCO_ERR_ARG before any GPU work: a null pointer, P < 1, N < P, 24 * 9 * N >= 2^31, L outside 0..16, max_gap < 1, lam not in
 *   (0, 1e4], u_ref not finite and positive, an output that is its own input. */
#define POCO_SMOOTH_MAX_LIN 16
#define POCO_SMOOTH_SCRATCH_DOUBLES(N, L) ((size_t)(N) * (size_t)(266 + (L)))
int poco_op_track_smooth(const float* d_pose, const float* d_u, const int32_t* d_frames, const int32_t* d_offsets, int P, int N,
                         const float* d_lin, int L, double lam, double u_ref, int max_gap, double* d_scratch, float* d_pose_out,
                         float* d_lin_out, float* d_shift, int max_blocks, void* stream);

/* ---- the keypoint refit: uncertain joints follow the row's 2-D keypoints, the network's own pose is the prior --------------------------
 * demo.py --mode video --kp_refit LAMBDA, eval.py --kp_refit LAMBDA; csrc/kp_refit.hip; poco_amd/refit.py; DESIGN.md section 31;
 * tests/refit_np.py restates it in float64 numpy with dense matrices and numpy.linalg.cholesky.  No counterpart in the reference
 * (its demo keeps VIBE's smplify_runner, whose TemporalSMPLify is not in its tree).
 *
 * poco_op_kp_refit: N independent rows (frames of any tracks, crops of any images).  Device inputs: d_pose [N,24,3,3] (the network's
 *   local joint rotations), d_u [N,24] (the post-processed uncertainty), d_jrest [N,24,3] (the rest-pose joints J(beta) of the row's
 *   shape; betas are not optimised), d_kp [N,K,3] (x, y, confidence, any pixel frame), d_cam [N,5] = (a, tx, ty, px, py) with
 *   u = a (X + tx) + px, v = a (Y + ty) + py, d_norm [N] (the box side: residuals are fractions of it).  HOST arrays: kp_joint int32
 *   [K], 1 <= K <= POCO_REFIT_MAX_KP (the kinematic joint a keypoint observes, -1 = none), parents int32 [24] (parents[0] < 0,
 *   0 <= parents[j] < j).  Scalars: lam > 0, u_ref > 0, rho (<= 0: no robustifier), cam_prior > 0, conf_thresh, min_kp >= 2,
 *   iters in 1..POCO_REFIT_MAX_ITERS, all finite.
 *   Unknowns  delta_j in R^3 per joint, applied as R_j <- R_j exp(delta_j) (exp: Rodrigues; |delta| < 1e-8: the series 1 - t^2 / 6,
 *             1 / 2 - t^2 / 24), and (kappa, dtx, dty) applied as a <- a exp(kappa), tx <- tx + dtx, ty <- ty + dty: 75 in all.
 *   Model     G_0 = R_0, p_0 = J_0; G_j = G_parent R_j, p_j = p_parent + G_parent (J_j - J_parent); keypoint k observes p_(kp_joint[k]).
 *             d p_k / d delta_j = -[p_k - p_j]x G_j for j a PROPER ancestor of kp_joint[k] (a joint's own rotation does not move it)
 *             and zero otherwise; d r / d kappa = (u - px, v - py) / norm, d r / d (dtx, dty) = a / norm on the diagonal.
 *   Cost      F = sum_k gm(c_k |r_k|^2) + sum_j w_j |q_j|^2 + cam_prior (kappa^2 + dtx^2 + dty^2), the camera terms being the totals
 *             since the start; r_k = (proj(p_k) - kp_k) / norm; c_k = the confidence if it exceeds conf_thresh and kp_joint[k] >= 0,
 *             else 0; gm(s) = rho^2 s / (rho^2 + s) (Geman-McClure; s itself for rho <= 0); w_j = lam clamp((u_ref / max(u_j,
 *             1e-6))^2, 1e-6, 1e6), a non-finite u_j giving lam 1e-6 (poco_op_track_smooth's rule); q_j = Log(Rnet_j^T R_j): half the
 *             skew part of the matrix times angle / |half skew|, angle = atan2(|half skew|, (trace - 1) / 2), the half skew part
 *             itself below 1e-8.  The sum runs over k, then j, then the camera, in ascending order.
 *   Step      `iters` Levenberg-Marquardt steps from the network's values, every row all of them (no early exit).  A = J^T W J +
 *             diag(w_j, cam_prior) with the IRLS weights W_k = c_k (rho^2 / (rho^2 + s_k))^2 at the current point, g = J^T W r +
 *             (w_j q_j, cam_prior (kappa, dtx, dty)): the prior's Jacobian with respect to delta_j is taken as the identity (first
 *             order in q_j).  (A + mu diag(A)) d = -g by root-free Cholesky (L D L^T) without pivoting: A is positive definite
 *             whatever the data, every w_j and cam_prior being positive.  F at the trial point: lower = accepted, mu <- max(mu / 3,
 *             1e-12); otherwise (a NaN included) the point is kept and mu <- min(3 mu, 1e12); mu starts at 1e-3.
 *   Skipped   a row with a non-finite value in pose, jrest, kp, cam or norm, or norm <= 0: flag 2; else a row with fewer than min_kp
 *             keypoints of non-zero c_k: flag 1.  Its pose and (a, tx, ty) are copied through bit for bit, its shift, cost and
 *             accepted steps are 0.
 *   Outputs (every element is written; none may overlap an input or another output): d_pose_out [N,24,3,3], d_cam_out [N,3] =
 *   (a, tx, ty), d_shift [N,24] (degrees between Rnet_j and R_j, poco_op_track_smooth's formula), d_cost [N,2] (F before, after),
 *   d_info int32 [N,2] (accepted steps, flag: 0 fitted, 1 too few keypoints, 2 non-finite input).
 *   Arithmetic: fp64 throughout, rounded once to fp32 on store.  One launch on `stream` (a block per row at a time, the row in LDS);
 *   max_blocks > 0 caps the grid (tests).  No allocation, no synchronisation, no atomics: a row's bits do not depend on the other
 *   rows, on the grid or on max_blocks, and two runs give the same bits.
 *   POCO_ERR_ARG before any GPU work: a null pointer, N < 1, 216 N >= 2^31, K outside 1..32, a kp_joint entry outside -1..23, a
 *   parents table that is not a tree rooted at 0 with parent < child, a scalar out of range, max_blocks < 0, overlapping buffers. */
#define POCO_REFIT_MAX_KP 32
#define POCO_REFIT_MAX_ITERS 32
int poco_op_kp_refit(const float* d_pose, const float* d_u, const float* d_jrest, const float* d_kp, const float* d_cam,
                     const float* d_norm, int N, int K, const int32_t* kp_joint, const int32_t* parents, double lam, double u_ref,
                     double rho, double cam_prior, double conf_thresh, int min_kp, int iters, float* d_pose_out, float* d_cam_out,
                     float* d_shift, float* d_cost, int32_t* d_info, int max_blocks, void* stream);

/* ---- eval.py --sequences: the acceleration and the acceleration error of every row of a ragged buffer of tracks --------------------
 * eval.py --sequences [--seq_post LIST]; csrc/track_accel.hip; poco_amd/sequences.py; tests/accel_np.py
 * restates it in float64 with plain loops.  The acceleration error is compute_error_accel of the VIBE line of work (not in the
 * reference's code, which reports no temporal metric).
 *
 * poco_op_track_accel: P tracks concatenated into N rows as for poco_op_track_smooth: d_offsets int32 [P+1] (0 = first, N = last,
 *   strictly increasing: the CALLER checks this; the kernels only clamp it to 0..N), d_frames int32 [N].  d_pred and d_gt: fp32
 *   joints [N,M,3], row i at d_x + i * stride floats, 1 <= M <= POCO_ACCEL_MAX_JOINTS, stride >= 3 M; only the first 3 M floats of
 *   a row are read (the evaluator's records in place: d_records + 116 and d_records + 212 at stride POCO_EVAL_RECORD_FLOATS).
 *   d_gt may be NULL: then d_accel_err is not written (it may be NULL too) and the sums of the acceleration error are 0.
 *   Row i is VALID when rows i-1, i, i+1 lie in one track and frames[i-1] + 1 == frames[i] == frames[i+1] - 1.
 *     a_m        = p[i-1][m] - 2 p[i][m] + p[i+1][m] (and g_m the same of the ground truth), formed as (x0 - 2 x1) + x2 in fp64
 *     accel[i]     = (sum_m |a_m|) / M           accel_err[i] = (sum_m |a_m - g_m|) / M      |v| = sqrt((x^2 + y^2) + z^2)
 *   in the units of the joints per frame^2 (metres per frame^2; nothing is divided by a frame rate), all in fp64 and rounded once
 *   to fp32; the sum over the joints is a halving tree over 32 slots.  An invalid row gets the quiet NaN 0x7fc00000 in both.
 *   d_track_sums fp64 [P,3] = per track the sum of accel_err, the sum of accel (the fp64 values before their rounding) and the
 *   number of valid rows; d_total fp64 [3] = the same over all tracks.  A track's sum adds its rows t, t + 256, ... per lane in
 *   ascending order and then a halving tree over the 256 lanes; the total does the same over the tracks' sums: the summation tree
 *   is a function of the track lengths alone.  fp64 additions only, no floating-point atomics: all four outputs are bitwise
 *   independent of max_blocks (0 = the default grid, > 0 bounds it) and equal from run to run.
 *   d_scratch: POCO_ACCEL_SCRATCH_DOUBLES(N) doubles, caller-owned, set and consumed by the call (per row the two fp64 terms and
 *   the valid flag).  Every element of the outputs is written; none may overlap an input.
 *   Three launches on `stream` (a block per 64 rows: the 66 rows it needs are read once, coalesced, into LDS; one half-wave per
 *   row, one lane per joint; then a block per track; then one block); no allocation, no synchronisation.
 *   POCO_ERR_ARG before any GPU work: a null pointer (d_gt and, with it, d_accel_err excepted), M outside 1..32, stride < 3 M or
 *   > 65536, P < 1, N < P, N > 2^24, max_blocks < 0. */
#define POCO_ACCEL_MAX_JOINTS 32
#define POCO_ACCEL_SCRATCH_DOUBLES(N) ((size_t)(N) * 3)
int poco_op_track_accel(const float* d_pred, const float* d_gt, int stride, int M, const int32_t* d_frames, const int32_t* d_offsets,
                        int P, int N, double* d_scratch, float* d_accel, float* d_accel_err, double* d_track_sums, double* d_total,
                        int max_blocks, void* stream);
/* The records of an evaluator, copied on the device: d_out [n, POCO_EVAL_RECORD_FLOATS] fp32 (16-byte aligned) <- record
 * d_order[i] for i in [0, n) (d_order int32 [n] on the device, entries in [0, N written so far), checked by the CALLER: a row whose
 * entry is outside gets zeros); d_order NULL: the first n records in their own order.  One launch on `stream`; the records are
 * only read.  POCO_ERR_ARG: a null handle or d_out, n < 1, n > N without an order, a misaligned d_out; no step yet is
 * POCO_ERR_STATE. */
int poco_evaluator_copy_records(poco_evaluator_t e, const int32_t* d_order, int64_t n, float* d_out, void* stream);

/* ---- SORT: the tracks of video mode from per-frame person boxes (Bewley et al. 2016) ------------------------------------------------
 * demo.py --mode video --detections FILE --tracker sort; csrc/sort_tracks.hip; poco_amd/sort.py; DESIGN.md section 32;
 * tests/sort_np.py restates it in float64 numpy with plain loops and scipy's assignment.  It replaces the association half of the
 * reference's POCOTester.run_tracking (pocolib/core/tester.py), which calls multi_person_tracker: a detector followed by SORT.  The
 * detector is not part of this library: its boxes are the input.
 *
 * poco_op_sort_tracks: C clips concatenated: d_clip_offsets int32 [C+1] over frames (0 = first, F = last), d_frame_offsets int32
 *   [F+1] over detections (0 = first, N = last), both non-decreasing (a frame may hold no detection, a clip no frame); d_dets fp64
 *   [N,4] = (cx, cy, w, h), w, h > 0, at most POCO_SORT_MAX per frame.  The CALLER checks the tables and the boxes (they are device
 *   memory); the kernel clamps what it reads to the buffers and ends a clip with status 2 at a frame whose range is not inside
 *   [0, N], runs backwards or holds more than 64 detections.  iou_thresh in (0, 1), max_age >= 0, min_hits >= 0, max_trackers in
 *   1..POCO_SORT_MAX (SORT's published defaults: 0.3, 1, 3).
 *   A tracker: x = [u, v, s, r, u', v', s'] (s = area, r = w / h), a symmetric 7 x 7 covariance P of which the elements row >= column
 *   are computed and the others are their copies, and the counters time_since_update, hit_streak.  The matrices are those of the
 *   published sort.py (KalmanBoxTracker.__init__): F = I + E(0,4) + E(1,5) + E(2,6); H = [I4 | 0]; R = diag(1, 1, 10, 10);
 *   Q = diag(1, 1, 1, 1, 0.01, 0.01, 0.0001); P0 = diag(10, 10, 10, 10, 1e4, 1e4, 1e4).  Per clip, frame by frame, in fp64 without
 *   contraction (no fused multiply-add):
 *   1 predict  every live tracker: if s + s' <= 0 then s' = 0; x <- F x; P <- F P F^T + Q (each element the sum of at most four
 *              elements of P, as (P[i][j] + P[i+4][j]) + (P[i][j+4] + P[i+4][j+4]), then + Q on the diagonal); hit_streak = 0 if
 *              time_since_update > 0; time_since_update += 1.
 *   2 gate     boxes as corners: a detection is (cx - w/2, cy - h/2, cx + w/2, cy + h/2), a tracker the same of (u, v, w, h) with
 *              w = sqrt(s r), h = s / w.  o = wh / ((area_d + area_t) - wh), wh = max(0, xx2 - xx1) max(0, yy2 - yy1);
 *              g[d][k] = o if o >= iou_thresh, else 0 (a NaN: 0).  A tracker with a non-finite u, v, w or h or with w <= 0 or h <= 0
 *              has g = 0 against everything.
 *   3 assign   a matching that maximises the sum of g; pairs with g = 0 are no matches.  Shortest augmenting paths with potentials
 *              (the Hungarian method) on the max(D, K) square whose missing entries cost 0: a true optimum; where it is not unique
 *              (equal totals) any optimum may come back.  Loops: at most 64 rows, 65 steps per row, 65 steps per path.
 *   4 update   a matched tracker with z = (cx, cy, w h, w / h): y = z - x[:4]; S = P[:4,:4] + R = L D L^T (no pivoting, the sums in
 *              ascending k, v - L[i][k] (L[j][k] D[k])); K = P[:,:4] S^-1 row by row (L w = b, w / D, L^T k = w); x <- x + K y;
 *              AP = P - K P[:4,:]; P <- (AP - AP[:,:4] K^T) + (K R) K^T (the Joseph form); every sum over c = 0..3 starts from the
 *              c = 0 product and adds the others in ascending c.  time_since_update = 0, hit_streak += 1.
 *     birth    every unmatched detection, in detection order, starts a tracker with x = (cx, cy, w h, w / h, 0, 0, 0), P = P0,
 *              both counters 0 and the clip's next id (ids count from 0 in creation order).
 *   5 emit     a tracker is emitted in this frame if time_since_update == 0 and (hit_streak >= min_hits or the 1-based number of
 *              the frame in its clip <= min_hits); then the trackers with time_since_update > max_age are removed, the others
 *              keeping their order.
 *   Outputs (every element is written): d_tracker int32 [N] (the id of the tracker the detection ended up in), d_id int32 [N] (the
 *   same where that tracker was emitted in that frame, else -1), d_box fp64 [N,4] (u, v, sqrt(s r), s / sqrt(s r) of that tracker after
 *   its update or birth), d_count int32 [C] (trackers created), d_status int32 [C]: 0 ok; 1 = at some frame the live trackers plus
 *   the births would have exceeded max_trackers: nothing of that frame is applied and the detections of it and of every later frame
 *   of the clip get d_tracker = d_id = -1 and a NaN box; 2 = the same ending at a frame the kernel could not read (above).
 *   One launch on `stream`: a block of one wave per clip, the frames a sequential loop inside it, the phases of a frame separated by
 *   block barriers; 58 KB of LDS per block (the 64 x 64 fp64 matrix, 64 packed covariances).  No allocation, no synchronisation, no
 *   atomics: a clip's outputs do not depend on the other clips and repeat bit for bit from run to run.
 *   POCO_ERR_ARG before any GPU work: C < 1, F < 0, N < 0, C > 2^24, F > 2^30, N > 2^28 (the int32 plans), a null offset table,
 *   d_count or d_status, a null d_dets, d_tracker, d_id or d_box with N > 0, iou_thresh outside (0, 1) or not finite, max_age < 0,
 *   min_hits < 0, max_trackers outside 1..64. */
#define POCO_SORT_MAX 64
int poco_op_sort_tracks(const double* d_dets, const int32_t* d_frame_offsets, const int32_t* d_clip_offsets, int64_t C, int64_t F,
                        int64_t N, double iou_thresh, int max_age, int min_hits, int max_trackers, int32_t* d_tracker, int32_t* d_id,
                        double* d_box, int32_t* d_count, int32_t* d_status, void* stream);

/* ---- track stitching: the fragments an occlusion left of one person joined into chains, by body shape and box motion ------------------
 * demo.py --mode video --track_stitch; csrc/track_stitch.hip; poco_amd/stitch.py; tests/stitch_np.py restates
 * it in float64 numpy with plain loops and scipy's assignment.  No counterpart in the reference's code: its tracker's ids are final.
 *
 * poco_op_track_stitch: C clips concatenated: d_clip_offsets int32 [C+1] over fragments (0 = first, P = last), d_frag_offsets int32
 *   [P+1] over rows (0 = first, N = last), at most POCO_STITCH_MAX_FRAGS fragments in a clip (a clip may hold none), at least one row
 *   in a fragment; d_frames int32 [N], strictly increasing inside a fragment; d_boxes fp64 [N,4] = (cx, cy, w, h), w, h > 0; d_betas
 *   fp32 [N,10]; d_var fp32 [N,24], >= 0.  The CALLER checks the tables and the rows (they are device memory); the kernels clamp
 *   every index they take from a table, and a clip whose range or one of whose fragments' ranges is not inside the buffers, is empty
 *   or runs backwards, or which holds more than 256 fragments, ends with status 2.
 *   max_gap >= 0, fit_len in 1..POCO_STITCH_MAX_FIT, u_ref, motion_tol, shape_tol, shape_floor > 0, shape_w >= 0 (0: no shape term).
 *   All of it in fp64 without contraction (no fused multiply-add), in this order:
 *   1 describe  fragment p, rows i = 0..T-1, first frame s, last frame e.  u_i = (var[i][0] + ... + var[i][23]) / 24 in ascending
 *               joint order; w_i = r r with r = u_ref / max(u_i, 1e-6).  W = sum w_i, W2 = sum w_i^2, bbar_k = (sum w_i beta_ik) / W,
 *               sig2 = ((sum_i w_i d_i) / W) / 10 with d_i = sum_k (beta_ik - bbar_k)^2 in ascending k.  Every sum over the rows is
 *               the same tree, a function of T alone: slot l of 64 adds its rows l, l + 64, ... in ascending order to 0, then a
 *               halving tree over the slots (slot t += slot t + o for o = 32, 16, .., 1).
 *               tail fit: the last m = min(fit_len, T) rows, t_j = frame_j - e, each of q = (cx, cy, log h): tbar = (sum t_j) / m,
 *               qbar = (sum q_j) / m, Stt = sum (t_j - tbar)^2, Stq = sum (t_j - tbar)(q_j - qbar), all in ascending j from 0;
 *               velocity = Stq / Stt, state = qbar - velocity * tbar; with m = 1 (or Stt = 0) velocity = 0 and state = qbar.
 *               head fit: the same over the first m rows with t_j = frame_j - s.
 *   2 pair      (a -> b), a != b in one clip, D = s_b - e_a in 1..max_gap + 1 (else gain 0): h = D / 2; pa = tail state(a) +
 *               tail velocity(a) * h, pb = head state(b) - head velocity(b) * h;
 *               c_m = sqrt((dx dx + dy dy) / (exp(pa.l) exp(pb.l)) + dl dl) / (motion_tol sqrt(D)) with (dx, dy, dl) = pa - pb;
 *               c_s = sqrt((sum_k (bbar_ak - bbar_bk)^2) / 10) / sqrt((sig2_a + sig2_b) + shape_floor^2) / shape_tol;
 *               gain 0 if c_m > 1, if shape_w > 0 and c_s > 1, or if either is not finite; else
 *               gain = 1 - (c_m c_m + shape_w (c_s c_s)) / (1 + shape_w).
 *   3 assign    per clip a matching of tails to heads that maximises the sum of the gains; pairs of gain 0 are no links.  Shortest
 *               augmenting paths with potentials on the n x n square of costs -gain (poco_op_sort_tracks' step 3 on up to 256
 *               columns): a true optimum; where it is not unique any optimum may come back.  Loops: at most 256 rows, 257 steps
 *               per row, 257 steps per path.  D >= 1 makes every chain run forward in time: no cycle, no overlap inside a chain.
 *   Outputs (every element is written): d_succ, d_pred int32 [P] (fragment index inside the call, -1 = none), d_chain int32 [P]
 *   (chains numbered per clip from 0 in the order of their FIRST fragments' indices), d_gain fp64 [P] (the gain of the link to the
 *   successor, 0 without one), d_desc fp64 [P,POCO_STITCH_DESC] = bbar[10], sig2, W, W2, T, tail state[3], tail velocity[3], head
 *   state[3], head velocity[3], s, e (zeros for a fragment the kernel cannot read), d_status int32 [C]: 0, or 2 (above): then the
 *   clip's fragments get succ = pred = -1, their own chain and gain 0.
 *   d_scratch: POCO_STITCH_SCRATCH_DOUBLES(P) doubles, caller-owned, set and consumed by the call (per fragment its row of the
 *   clip's gain matrix).  Three launches on `stream` (a block of one wave per fragment; a block of 256 per fragment, a lane per
 *   pair; a block of 256 per clip, a lane per column); no allocation, no synchronisation, no atomics, no grid barrier, no spin-wait:
 *   a clip's outputs do not depend on the other clips and repeat bit for bit from run to run.
 *   POCO_ERR_ARG before any GPU work: C < 1, P < 0, N < 0, C > 2^24, P > 2^22, N > 2^24 (the int32 plans), a null offset table or
 *   d_status, a null d_frames, d_boxes, d_betas or d_var with N > 0, a null d_scratch, d_succ, d_pred, d_chain, d_gain or d_desc with
 *   P > 0, max_gap outside 0..2^30, fit_len outside 1..32, u_ref, motion_tol, shape_tol or shape_floor not finite or <= 0, shape_w
 *   not finite or < 0. */
#define POCO_STITCH_MAX_FRAGS 256
#define POCO_STITCH_MAX_FIT 32
#define POCO_STITCH_DESC 28
#define POCO_STITCH_SCRATCH_DOUBLES(P) ((size_t)(P) * 256)
int poco_op_track_stitch(const int32_t* d_clip_offsets, const int32_t* d_frag_offsets, const int32_t* d_frames, const double* d_boxes,
                         const float* d_betas, const float* d_var, int64_t C, int64_t P, int64_t N, int max_gap, int fit_len,
                         double u_ref, double motion_tol, double shape_tol, double shape_floor, double shape_w, double* d_scratch,
                         int32_t* d_succ, int32_t* d_pred, int32_t* d_chain, double* d_gain, double* d_desc, int32_t* d_status,
                         void* stream);

/* ---- calibrating the uncertainty: isotonic regression of the error on the uncertainty, and evaluating the fitted maps ------------------
 * eval.py --calibrate OUT.npz, demo.py --calibration FILE; csrc/isotonic.hip; poco_amd/calibrate.py; DESIGN.md section 33;
 * tests/calib_np.py restates both operators with plain loops and a stack.  No counterpart in the reference's code.
 *
 * poco_op_isotonic: S independent segments in one ragged buffer.  d_key, d_y fp32 [M] in row order; d_order int32 [N], entries in
 *   [0, M); d_seg_offsets int32 [S+1], non-decreasing from 0 to N (the CALLER checks both: they are device memory; the kernels clamp
 *   every index they take from them).  Positions [seg_offsets[s], seg_offsets[s+1]) of d_order list segment s's rows in ascending
 *   order of the canonical key of poco_op_rank_curve (-0.0 = +0.0; no NaN keys): d_order of poco_op_rank_curve plus a base offset.
 *   A row may appear in several segments; a segment may be empty.  1 <= S <= POCO_ISO_MAX_SEGS, 0 <= N <= POCO_ISO_MAX_N,
 *   0 <= M <= POCO_ISO_MAX_N and M >= 1 if N >= 1.  y must be finite (else: unspecified values, nothing out of bounds, every loop
 *   a `for` bounded by the sizes).
 *   The fit is the least-squares non-decreasing fit with ties pooled first:
 *     units   within a segment, maximal runs of positions with equal canonical key; weight = rows, sum = sum of y.
 *     blocks  the unique partition of the segment's units into consecutive blocks whose means (sum of y / rows) increase strictly
 *             from block to block and of which none can be split into a left part whose mean is strictly below the right part's:
 *             two neighbours pool when mean_left >= mean_right, decided as sum_l * rows_r >= sum_r * rows_l in fp64.
 *   d_block int32 [N]: for every position the first position of its block (exact).
 *   d_fit fp64 [N]: the block's mean at every position, summed in a final pass from the block's own rows in fp64 (a segmented scan
 *     over tiles of POCO_ISO_TILE positions; the tree is a function of the block's extent alone) and divided once by the rows:
 *     |value - fsum(block) / rows| <= 2^-52 * sum_block |y|.  No fused multiply-add.
 *   d_seg_blocks int32 [S+1]: block offsets per segment; d_knots fp64 [B_total,4], compacted in order: per block the lowest and
 *     the highest canonical key, the value and the rows.  Capacity N rows; rows past B_total are not written.
 *   d_scratch: poco_op_isotonic_scratch_bytes(N, S) bytes (0 = N or S out of range; 256 when N = 0), 8-byte aligned.
 *   max_blocks: 0 = the default grid, > 0 bounds it; every output is bitwise independent of it and equal from run to run.
 *   12 + max(0, ceil(log2 N) - 11) launches on `stream` (2 when N = 0); the inputs are only read; no allocation, no synchronisation,
 *   no floating-point atomic, no spin-wait, no grid barrier.
 *   POCO_ERR_ARG before any GPU work: a null pointer (the [N] and [M] buffers and d_knots may be NULL only with N = 0), S, N or M
 *   out of range, max_blocks < 0, a scratch buffer that is too small or misaligned, misaligned buffers, outputs or scratch that
 *   overlap an input or each other.
 *
 * poco_op_calib_apply: d_out[r][c] = f_m(d_x[r][c]) with m = d_map_ids[c] (clamped to [0, P)), for d_x fp32 [R,S] row-major.
 *   Map m = rows [d_map_offsets[m], d_map_offsets[m+1]) (clamped to [0, B]) of d_knots fp64 [B,4] as written by poco_op_isotonic:
 *   blocks b = 0 .. n-1 with lo_b <= hi_b < lo_(b+1) and values v_b.  f(NaN) = NaN; an empty map gives NaN; v_0 for x <= lo_0;
 *   v_(n-1) for x >= hi_(n-1); v_b for lo_b <= x <= hi_b; between hi_b and lo_(b+1):
 *   v_b + (v_(b+1) - v_b) * ((x - hi_b) / (lo_(b+1) - hi_b)) in fp64 in exactly that order without contraction, rounded to fp32
 *   once.  One lane per element, a binary search of at most 32 steps.  One launch on `stream`.
 *   POCO_ERR_ARG before any GPU work: a null pointer (d_knots may be NULL only with B = 0), R outside 1..2^26, S outside 1..4096,
 *   R * S > 2^30, P outside 1..4096, B outside 0..2^26, max_blocks < 0, misaligned buffers, d_out overlapping an input. */
#define POCO_ISO_TILE 2048
#define POCO_ISO_MAX_N (1 << 26)
#define POCO_ISO_MAX_SEGS 4096
size_t poco_op_isotonic_scratch_bytes(int64_t N, int S);
int poco_op_isotonic(const float* d_key, const float* d_y, int64_t M, const int32_t* d_order, int64_t N, const int32_t* d_seg_offsets,
                     int S, void* d_scratch, size_t scratch_bytes, int32_t* d_block, double* d_fit, int32_t* d_seg_blocks,
                     double* d_knots, int max_blocks, void* stream);
int poco_op_calib_apply(const float* d_x, int64_t R, int S, const int32_t* d_map_ids, const int32_t* d_map_offsets, int P,
                        const double* d_knots, int64_t B, float* d_out, int max_blocks, void* stream);

/* ---- the cluster bootstrap: fp64 moments per unit and B resamples of the units with replacement, every sum in a fixed order -----------
 * eval.py --bootstrap B; csrc/bootstrap.hip; poco_amd/bootstrap.py; tests/boot_np.py restates it with plain
 * loops and math.fsum.  No counterpart in the reference's code, which reports point estimates only.
 *
 * poco_op_bootstrap: d_planes fp32 [E][n] on the device, 1 <= E <= POCO_BOOT_MAX_PLANES, 1 <= n <= POCO_BOOT_MAX_N.  pairs int32
 *   [P][2] on the HOST (read before the launch; NULL if P = 0), 0 <= P <= POCO_BOOT_MAX_PAIRS, entries in [0, E); a pair may name
 *   one plane twice.  d_unit_offsets int32 [U+1] on the device: unit u = rows [offsets[u], offsets[u+1]), non-decreasing from 0 to n,
 *   empty units allowed, 1 <= U <= n (the CALLER checks the values: they are device memory; the kernel clamps every offset into
 *   [0, n] and never reads outside d_planes).  NULL = every row is its own unit; then U must equal n.  0 <= B <= POCO_BOOT_MAX_B.
 *   M = 1 + E + P.
 *   d_center fp64 [E]: the mean of each plane over all n rows (tiles of 4096 rows: lane-strided sums and a halving tree over 256
 *     lanes per tile, the same over the tiles' sums, one division).
 *   d_unit_mom fp64 [U][M], per unit: column 0 = its rows, columns 1..E = the sums of the raw values, columns E+1..E+P = the sums of
 *     (v_a - center_a) * (v_b - center_b) of each pair, each factor and the product rounded to fp64 before the addition (no fused
 *     multiply-add).  The products are centred so that a correlation formed from them does not cancel; Pearson's r does not change
 *     under a shift.  A wave per unit: lane l adds rows l, l + 64, ... of the unit in order, then a halving tree over the 64 lanes.
 *   d_out fp64 [B+1][M]: row 0 = the sum of unit_mom over the units 0 .. U-1, each once (the full sample, by the arithmetic of the
 *     replicates); row b >= 1 = the sum of unit_mom[idx(b, j)] over the draws j = 0 .. U-1.
 *   The draws: Philox4x32-10 (multipliers 0xD2511F53, 0xCD9E8D57; Weyl constants 0x9E3779B9, 0xBB67AE85; ten rounds), key = (seed
 *     low word, seed high word), counter = (q, 0, b, 0); its four output words, in order, are draws 4q .. 4q+3 of replicate b.
 *     idx = ((uint64_t)word * U) >> 32.  A unit is drawn with a probability that is off from 1 / U by at most 2^-32: relative to
 *     1 / U that is U 2^-32 = 8e-6 at U = 35 515 (3DPW's crops) and 2^-8 at U = 2^24.  Stateless: a draw depends on (seed, b, j, U).
 *   The sum of a replicate: a block of 256 lanes; lane t owns the counters q = t, t + 256, ... and adds the rows of their draws
 *     4q .. 4q+3 (those below U) in that order, column by column; then a halving tree over the 64 lanes of each wave and
 *     ((wave 0 + wave 1) + wave 2) + wave 3.  Which additions form an output word, and their order, is fixed by (n, E, P, the
 *     offsets, seed, b): not by the grid, max_blocks, B or the order in which blocks finish.  No floating-point atomics.
 *   d_draw_counts uint32 [B][U], or NULL to skip: how often replicate b + 1 drew unit u (zeroed by a launch, then integer atomics).
 *   d_scratch: poco_op_bootstrap_scratch_bytes(n, E, P, U) bytes (0 = an argument out of range), 8-byte aligned.
 *   max_blocks: 0 = the default grid, > 0 bounds it; every output is bitwise independent of it and equal from run to run.
 *   4 launches on `stream` (5 with d_draw_counts and B > 0); the inputs are only read; no allocation, no synchronisation.
 *   A NaN or an infinity in a plane reaches center, hence every centred product of that plane; in the raw columns it reaches exactly
 *   the replicates that drew its unit.
 *   POCO_ERR_ARG before any GPU work: a null pointer (pairs may be NULL only with P = 0; d_unit_offsets only with U = n), n, E, P,
 *   U or B out of range, max_blocks < 0, a pair entry outside [0, E), a scratch buffer that is too small, misaligned buffers,
 *   scratch or outputs that overlap an input or each other. */
#define POCO_BOOT_MAX_N (1 << 24)
#define POCO_BOOT_MAX_PLANES 16
#define POCO_BOOT_MAX_PAIRS 16
#define POCO_BOOT_MAX_B 65536
size_t poco_op_bootstrap_scratch_bytes(int64_t n, int E, int P, int64_t U);
int poco_op_bootstrap(const float* d_planes, int64_t n, int E, const int32_t* pairs, int P, const int32_t* d_unit_offsets, int64_t U,
                      int64_t B, uint64_t seed, void* d_scratch, size_t scratch_bytes, double* d_center, double* d_unit_mom,
                      double* d_out, uint32_t* d_draw_counts, int max_blocks, void* stream);

/* ---- image degradation of raw crops: blur, pixelation, contrast, gamma, noise and the rounding before a JPEG round trip -----------------
 * eval.py --corrupt LEVELS; csrc/corrupt.hip; poco_amd/corrupt.py; tests/corrupt_np.py restates it with plain
 * float64 loops.  The reference's only pixel-level augmentation is the per-channel factor of poco_dataset_crop's `pn`; the kinds here
 * are the common ones of corruption benchmarks, defined below and NOT ImageNet-C's (those need cv2 and skimage).
 *
 * poco_op_corrupt: d_in fp32 [N,3,res,res], raw crops in [0, 255] as poco_dataset_crop(..., normalize = 0) writes them; per crop a chain
 *   of chain_len records, d_steps [N][chain_len] on the device and h_steps, the host copy they were uploaded from (the ranges below are
 *   checked on it; nothing compares the two, as for poco_dataset_crop).  A chain ends at its first POCO_CORRUPT_NONE record; crops of
 *   one call may carry different chains.  The steps at positions pos_begin <= p < pos_end are applied, one launch per position over all
 *   crops (none in the range: one launch that copies), ping-pong between d_tmp and d_out, both fp32 [N,3,res,res]; the last launch
 *   writes d_out: raw, or with normalize != 0 mapped by (x / 255 - mean) / std in float32 as oracle/crop_np.normalize_np.  d_tmp's
 *   content afterwards is unspecified.  The caller that composes a JPEG round trip between two positions calls once per position.
 *   Every step reads fp32, evaluates in fp64 without contraction, clamps to [0, 255] and rounds once to fp32 on the store.  A tap
 *   outside the plane is mirrored without repeating the edge (scipy.ndimage mode='mirror'), as often as needed; res = 1 maps every
 *   index to 0.  x = column, y = row, v = the fp32 input of the step as fp64:
 *     GAUSSIAN_BLUR  p0 = sigma in (0, 5].  r = int(3 sigma + 0.5); w_k = exp(-k^2 / (2 sigma^2)), k = -r .. r, divided by their sum taken
 *                    in that order; h(y, x) = sum_k w_k v(y, x + k), then out(y, x) = sum_k w_k h(y + k, x), both in the order k = -r .. r,
 *                    h kept in fp64.  Yardstick: scipy.ndimage.gaussian_filter(float64, sigma, mode='mirror', truncate=3.0).
 *     MOTION_BLUR    ival = L odd in 3..31, (p0, p1) = unit direction (dx, dy), computed on the host.  The mean of the L bilinear samples at
 *                    (x + k p0, y + k p1), k = -(L-1)/2 .. (L-1)/2 in that order; a sample = (1-fy) ((1-fx) v00 + fx v01) + fy ((1-fx) v10 +
 *                    fx v11) with (fx, fy) the fractions above floor.
 *     PIXELATE       ival = f in 2..32.  The mean over each f x f cell anchored at (0, 0), partial at the far edges, written to every pixel
 *                    of the cell: per column the sum over the cell's rows top to bottom, those sums left to right, one division by the count.
 *     CONTRAST       p0 = c in [0, 2].  mean + c (v - mean), mean per crop and channel: 256 lane-strided sums of the row-major plane, the
 *                    halving tree of csrc/block_prims.h, one division.
 *     GAMMA          p0 = g in [0.2, 5].  255 (v / 255)^g.
 *     GAUSSIAN_NOISE p0 = sigma in [0, 255] pixel units.  Philox4x32-10 as poco_op_bootstrap's, key = seed, counter = (e / 4, 0, stream,
 *                    chain position) for element e of the crop's [3,res,res] block; words (w0, w1) and (w2, w3) give two Box-Muller pairs,
 *                    u1 = (w + 1) 2^-32, u2 = w 2^-32, z = sqrt(-2 ln u1) (cos, sin)(2 pi u2): z of elements 4q, 4q+1 | 4q+2, 4q+3.
 *                    out = v + sigma z.  `stream` is the caller's name of the crop (eval.py: the dataset row), so a crop's noise does not
 *                    depend on its place in the batch.
 *     JPEG           ival = quality 1..100.  floor(v + 0.5): the bytes a JPEG encoder is given.  The round trip itself is composed by the
 *                    caller (poco_amd/corrupt.py: poco_jpeg_encode, then poco_jpeg_decode, one picture per crop).
 *   Enqueued on `stream`: no allocation, no synchronisation, any N.  POCO_ERR_ARG before any launch: a null pointer, N < 1, res outside
 *   1..4096, chain_len outside 1..POCO_CORRUPT_MAX_STEPS, a position range outside 0 <= pos_begin <= pos_end <= chain_len, buffers that
 *   are not three different ones, and - read from h_steps - an unknown kind, a step after an empty one, a parameter outside the ranges
 *   above or not finite.  The kernel reads d_steps only and clamps the kind and every index it derives from a record. */
#define POCO_CORRUPT_MAX_STEPS 4
enum { POCO_CORRUPT_NONE = 0, POCO_CORRUPT_GAUSSIAN_BLUR = 1, POCO_CORRUPT_MOTION_BLUR = 2, POCO_CORRUPT_PIXELATE = 3,
       POCO_CORRUPT_CONTRAST = 4, POCO_CORRUPT_GAMMA = 5, POCO_CORRUPT_GAUSSIAN_NOISE = 6, POCO_CORRUPT_JPEG = 7 };
typedef struct {
  int32_t kind;       /* POCO_CORRUPT_*                                                   */
  int32_t ival;       /* motion_blur: L; pixelate: f; jpeg: quality                       */
  float p0, p1;       /* sigma | (dx, dy) | c | g | noise sigma                           */
  uint32_t seed[2];   /* gaussian_noise: the Philox key                                   */
  uint32_t stream;    /* gaussian_noise: counter word 2, the caller's name of the crop    */
} poco_corrupt_step_t;
int poco_op_corrupt(const float* d_in, const poco_corrupt_step_t* d_steps, const poco_corrupt_step_t* h_steps, int N, int chain_len,
                    int pos_begin, int pos_end, int res, int normalize, float* d_tmp, float* d_out, void* stream);

/* Time `ncfg` tile configurations (cfgs7 = ncfg x SEVEN ints {MT,NT,WM,WN,R,NI,ALG} each, csrc/common.h CONV_CFG_INTS;
 * MT<=0 = heuristic) for one conv shape on random data; ms_out[i] < 0 = configuration invalid for this shape.  NULL cfgs7 /
 * ms_out, ncfg < 1 or channel counts that are not multiples of 16 are POCO_ERR_ARG.  iters < 0: |iters| launches of the RESIDUAL form (the
 * input doubles as the residual: conv2 of a BasicBlock; needs Cin == Cout, stride 1).  Used by poco_amd/tune.py. */
int poco_tune_conv(int B, int H, int W, int Cin, int Cout, int ks, int stride, const int* cfgs7, int ncfg,
                   int iters, float* ms_out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* POCO_HIP_H */
