// Launchers of the non-GEMM kernels (all enqueue on `stream`, no allocation, no sync).
#pragma once
// float4 index of (row = b*H + y, x, channel quad c4) in the L16 activation layout (csrc/common.h): a buffer of
// C channels has C/16 slice rows of W*16 floats per image row.  Usable from host and device code.
#define L16_F4(row, x, c4, W, C16) ((((size_t)(row) * (C16)) + ((c4) >> 2)) * (size_t)(W) * 4 + (size_t)(x) * 4 + ((c4) & 3))
#include "common.h"

// ---- backbone side kernels (kernels_misc.hip) ---------------------------------------------------
// Direct small-Cin stem conv (Cin = 3): NCHW image -> NHWC features, + shift, ReLU.
//   ks=3,stride 2,pad 1 : hrnet.py:467-469 ;  ks=7,stride 2,pad 3 : resnet.py:203-205
// w: [ks*ks*3][Cout] (tap-major, scale folded), shift [Cout]; Cout must be 64.
void launch_stem_conv(const float* img_nchw, const float* w, const float* shift, float* out_nhwc, int B,
                      int H, int W, int ks, hipStream_t s, int use_mfma = 1);
// the same as an implicit GEMM on the fp32 MFMA (stem_mfma.hip); false = shape not covered (Wo != 112), nothing launched
bool launch_stem_conv_mfma(const float* img_nchw, const float* w, const float* shift, float* out_nhwc, int B, int H, int W, int ks,
                           hipStream_t s);
// 3x3 stride-2 pad-1 max pool, NHWC (resnet.py:206).
// conv3 + residual + ReLU of one Bottleneck chained with conv1 + ReLU of the next (bneck_chain.hip)
constexpr int BNECK_CHAIN_MAX_BLOCKS = 256, BNECK_CHAIN_WAVES = 8;   // persistent grid: beyond blocks x waves 16-pixel sub-tiles a wave walks several
int launch_bneck_chain(const float* t, int t_cs, const float* res, int res_cs, float* y, int y_cs, float* u, int u_cs,
                       const float* w3, const float* b3, const float* w1, const float* b1, int B, int H, int W,
                       hipStream_t s);
// K-concatenated projection shortcut with a strided second source (gemm1x1.hip)
// wave_layout = 100 NI + 10 WM + WN: WM x WN waves per block (each >= 1, at most 8 in all), NI = load schedule 1 | 3..6 (0 = 1);
// wave_layout 0 = one wave per block, hipcc's load order.  False = not a layout (launch_gemm1x1_dual then returns POCO_ERR_ARG).
bool gemm1x1_dual_layout(int wave_layout, int* WM, int* WN, int* NI);
int launch_gemm1x1_dual(const float* a, int a_cs, int Ca, const float* b, int b_cs, int Cb, int H2, int W2, int stride2,
                        const float* wfrag, const float* bias, float* out, int out_cs, int Cout, int B, int Ho, int Wo, int act,
                        hipStream_t stream, int wave_layout = 0);   // wave_layout = 100 NI + 10 WM + WN (0 = one wave per block, hipcc's load order)
void launch_maxpool3x3s2(const float* in, float* out, int B, int H, int W, int C, int out_cs, hipStream_t s);
// x2 bilinear upsample, align_corners=True, NHWC (hrnet.py:440).
void launch_bilinear_up2x(const float* in, float* out, int B, int H, int W, int C, hipStream_t s);
// out = ReLU( sum_k addend_k[b, y >> shift_k, x >> shift_k, :] )  (HRNet fuse, hrnet.py:257-264).
struct FuseArgs {
  const float* src[4];   // first channel of each term
  int shift[4];          // nearest-neighbour upsampling: the term's plane is (H >> shift) x (W >> shift)
  int src_cs[4];         // channels per pixel of each term's buffer (a term may be a channel slice)
  int n;
};
// `out` points at the first output channel; out_cs = channels per pixel of the destination buffer.
void launch_fuse_sum(const FuseArgs& a, float* out, int B, int H, int W, int C, int out_cs, int relu, hipStream_t s);
// Global average pool NHWC [B,HW,C] -> dst[b*dst_stride + c] (hrnet_cls.py:482, cliff_head.py:96).
void launch_avgpool(const float* in, float* dst, int B, int H, int W, int C, int dst_stride, hipStream_t s);

// ---- head kernels (kernels_head.hip) ---------------------------------------------------------------
// Part attention pooling (KeypointAttention, layers/keypoint_attention.py:34-48):
//   out[b, c, j] = sum_p softmax_p(heat[b,p,1+j]) * feat[b,p,c]      (24 parts; heat channel 0 = bg)
// heat: NHWC [B,HW,heat_cs] ; feat: NHWC [B,HW,C] ; out: dst[b*dst_stride + c*24 + j] (channel-major).
// scratch: part_attention_scratch_floats(B, C) floats.  C <= 128.
size_t part_attention_scratch_floats(int B, int C);
void launch_part_attention_pool_ws(const float* heat, int heat_cs, const float* feat, int C, float* dst,
                                   int dst_stride, int B, int H, int W, float* scratch, hipStream_t s);
// LocallyConnected2d 128->6 per joint (layers/locallyconnected2d.py:27-37):
//   pose6d[b, j, o] = sum_c x[b*x_stride + c*24 + j] * w[o][c][j]
void launch_lc2d_pose(const float* x, int x_stride, const float* w /*[6][128][24]*/, float* pose6d /*[B,144]*/,
                      int B, hipStream_t s);
// rot6d -> rotmat (utils/geometry.py:247-261). in: [B, in_stride] holding 144 floats (24 x (3x2));
// writes rotmat (24*9 per crop) to up to two destinations (stride in floats, nullable).
void launch_rot6d(const float* in, int in_stride, float* dst0, int stride0, float* dst1, int stride1, int B,
                  hipStream_t s);
// Strided row copy: dst[b*dst_stride + i] = src[b*src_stride + i], i < n.
void launch_copy_rows(const float* src, int src_stride, float* dst, int dst_stride, int n, int B,
                      hipStream_t s);
// dst[b*dst_stride + i] = src[i] (broadcast an init vector into every crop's row).
void launch_broadcast_rows(const float* src, float* dst, int dst_stride, int n, int B, hipStream_t s);
// NHWC [B,HW,cs] (first C channels) -> NCHW [B,C,HW]
void launch_nhwc_to_nchw(const float* in, int cs, float* out, int B, int H, int W, int C, hipStream_t s);

// ---- the CLIFF regressor as one persistent launch (mlp_chain.hip) -----------------------------------------
// A program of stages; the jobs of a stage are independent, consecutive stages are separated by a grid barrier.
struct MlpLayer {            // out[r][n] = act(bias[n] + sum_k W[n][k] in[r][k] (+ res[r][n])) for rows r < B (row-major vectors)
  const float* in;           // [B][in_rs], K = 16 nC16 consecutive floats from `in`
  const float* res;          // nullable, [B][res_rs]
  float* out;                // [B][out_rs]
  const float4* wfrag;       // conv_pack_weights(ks = 1): [nC16][nT16][64] float4
  const float* bias;         // [16 nT16]
  int nC16, nT16, in_rs, res_rs, out_rs, act;   // act: 0 none, 1 ReLU, 2 sigmoid
};
enum { MLP_ROW_COPY = 0, MLP_ROW_BCAST = 1, MLP_ROW_ROT6D = 2 };
struct MlpRowJob {           // COPY: dst[r][i] = src[r][i], i < n; BCAST: dst[r][i] = src[i]; ROT6D: 24 x 6 -> 24 x 9 into dst and dst2 (nullable)
  const float* src;
  float* dst;
  float* dst2;
  int kind, src_rs, dst_rs, dst2_rs, n;
};
struct MlpStage { int layer0, nlayers, row0, nrows; };
constexpr int MLP_MAX_LAYERS = 16, MLP_MAX_ROWS = 12, MLP_MAX_STAGES = 14;
struct MlpProgram {
  MlpLayer layer[MLP_MAX_LAYERS];
  MlpRowJob row[MLP_MAX_ROWS];
  MlpStage stage[MLP_MAX_STAGES];
  int nstages, B;
  unsigned* sync;            // device, 1 KiB: arrival counters (mlp_chain.hip); zero before the first launch, re-armed by the kernel
  unsigned* err_host;        // pinned host word (device-visible): set when a grid barrier timed out
  unsigned max_spins;        // bound of a barrier's poll loop (0 = the default, 2^21 polls ~ 3 s); engine option debug_wait_spins
  int debug_skip_arrival;    // test hook (engine option debug_mlp_timeouts): block 0 does not arrive at the first barrier, i.e. every block times out
  long long* trace;          // nullable (tools/probe/mlp_probe.hip): block 0 writes wall_clock64() at the start, after each stage's jobs and after each barrier
};
int mlp_chain_grid(const MlpProgram& p, int max_blocks);
int launch_mlp_chain(const MlpProgram& p, int max_blocks, hipStream_t s);
// blocks of mlp_chain_kernel the device can hold at once (CUs x blocks per CU, queried once): the hand-rolled grid barrier needs
// every block of the grid resident
int mlp_chain_resident_blocks();

// ---- SMPL (kernels_smpl.hip) -------------------------------------------------------------------------
constexpr int SMPL_JOINTS_ITERS = 7;                     // smpl_joints_kernel: 1024 threads x this many hard-unrolled vertex rounds ...
constexpr int SMPL_MAX_V = SMPL_JOINTS_ITERS * 1024;     // ... i.e. body models of up to 7168 vertices (SMPL: 6890); larger ones are refused at load time
constexpr int SMPL_KB = 220;   // K of the blend GEMM: 207 pose + 10 shape + 1 template, padded to a multiple of 4
struct SmplDev {
  int V;                       // 6890
  const float* v_template;     // [V,3]
  const float* shapedirs;      // [10][V*3]   (transposed for coalescing)
  const float* posedirs;       // [207][V*3]
  const float* blend_cm;       // [SMPL_KB][3][VP]: rows 0..206 posedirs, 207..216 shapedirs, 217 v_template, coordinate-major (kernels_smpl.hip)
  int VP;                      // V padded to a multiple of 32
  const float* lbs_weights;    // [V,24]
  const float* J_template;     // [24,3]      J_regressor . v_template
  const float* J_shapedirs;    // [24,3,10]   J_regressor . shapedirs
  const float* J_regressor_extra;  // [9,V]
  const int* parents;          // [24]
  const int* extra_vertex_ids; // [21]
  const int* joint_map;        // [49]
};
struct SmplIO {
  const float* betas;  int betas_stride;    // [B,10]
  const float* rotmat; int rot_stride;      // [B,216]
  float* A;                                 // scratch [B,24,12]
  float* coef;                              // scratch [B,SMPL_KB]: coefficient rows of the blend GEMM (chain kernel -> skin kernel)
  float* joints24;                          // scratch [B,24,3]
  float* verts;                             // [B,V,3] output
  float* joints49;                          // [B,49,3] output
  float* joints49_out;                      // nullable: the same, written a second time (the caller's smpl_joints3d)
};
// smplx.lbs.lbs restated + the 49-joint wrapper of smpl_head.py:22-34.
void launch_smpl_lbs(const SmplDev& m, const SmplIO& io, int B, hipStream_t s);

struct CamArgs {
  const float* cam; int cam_stride;   // [B,3] (s,tx,ty)
  const float* joints49;              // [B,49,3]
  // cliff only (nullable for pare):
  const float* focal; const float* scale; const float* center; const float* orig_shape;
  float* cam_t;          // [B,3]
  float* fullimg_cam_t;  // [B,3] (cliff) nullable
  float* joints2d;       // [B,49,2]
  int cliff;
};
// smpl_head.py:63-78 (pare) / smplcam_head.py:65-90 (cliff) camera conversion + projection.
void launch_camera(const CamArgs& a, int B, hipStream_t s);

// ---- RealNVP (kernels_flow.hip) -----------------------------------------------------------------------
struct FlowDev {
  int L;               // number of coupling layers (rows of mask; even: nf_head.py:20-21 builds mask pairs)
  int ctx;             // context dim (512)
  const float* mask16; // [L][16]: mask rows zero-padded from 9 to 16
  // per (layer, net s|t): 24 x 64 float4 MFMA A-operand fragments = conv_pack_weights(ks = 1) of
  //   W0[:, :9] (K padded to 16) [4 quads] | W1 [16 quads: k slice major] | W2 (rows padded to 16) [4 quads]
  const float4* wpack;
  const float* b1;     // [L][2][64]
  const float* b2;     // [L][2][16] (zero padded)
  // step A (context GEMM): W0[:, 9:] of all 2L MLPs stacked to [L*2*64][512] in conv_pack_weights(ks = 1) order, bias = b0
  const float* wctx_frag;
  const float* bctx;   // [L*2*64]
};
// log_prob (backward_p + N(0,I) prior, layers/real_nvp.py:40-65; forward = 0) or forward_p (:25-38; forward = 1) of N rows.
// ctx: [ceil(N/rep)][512], row r uses context row r / rep (rep = 1: one context per row; rep = 24: nf_head.py:105-110's
// repeat_interleave without materialising it).  scratch: realnvp_scratch_floats(f, ceil(N/rep)) floats.
size_t realnvp_scratch_floats(const FlowDev& f, int ctx_rows);
int launch_realnvp(const FlowDev& f, const float* x, const float* ctx, int rep, float* out, int N, int forward, float* scratch,
                   hipStream_t s);

// ---- flow likelihood and the evaluator's uncertainty summaries (eval_likelihood.hip) -------------------------------------
constexpr int FLOW_NLL_REC = 80;   // include/poco_hip.h POCO_FLOW_NLL_RECORD_FLOATS
// rows [B*24, 9] = |pred_pose - batch_rodrigues(gt_pose)| / (var_pose + 1e-9)   (nf_head.py:89-105)
void launch_flow_residual(const float* pred_pose, const float* gt_pose, const float* var_pose, float* rows, int B, hipStream_t s);
// records [B, 80] from the rows, their log_prob and var_pose; valid [B] int32 (nullable = all): an invalid crop's record is zero
void launch_flow_nll_epilogue(const float* rows, const float* logphi, const float* var_pose, const int* valid, float* out, int B,
                              hipStream_t s);
// {valid crops, mean log phi, mean log sigma, loss_nf} (losses.py:346) of N records, fp64, one block
void launch_flow_nll_reduce(const float* rec, long long N, double* d_summary4, hipStream_t s);
// {Var-MPJPE, Variance} (trainer.py:374-378) of N evaluator records of `stride` floats, fp64, one block
void launch_eval_uncert_summary(const float* rec, int stride, int off_mpjpe, int off_unc, long long N, double* d_summary2, hipStream_t s);

// ---- preprocessing (kernels_misc.hip) --------------------------------------------------------------------
// frame: uint8 [H,W,3] RGB (device); boxes: [N,4] = (cx, cy, w, h) in pixels (float32 or float64); out: [N,3,res,res] fp32
// NCHW = ToTensor + Normalize of the uint8 crop cv2.warpAffine(getAffineTransform(box * scale -> res x res)) makes, byte-exact.
void launch_crop_normalize(const unsigned char* frame, int H, int W, const float* boxes, double bbox_scale, float* out,
                           int N, int res, hipStream_t s);
void launch_crop_normalize_f64(const unsigned char* frame, int H, int W, const double* boxes, double bbox_scale, float* out,
                               int N, int res, hipStream_t s);
// crops of several same-sized frames in one launch: frames = device array of frame pointers, frame_idx[n] = frame of crop n
void launch_crop_normalize_multi(const unsigned char* const* frames, int nframes, const int* frame_idx, int H, int W, const float* boxes,
                                 double bbox_scale, float* out, int N, int res, hipStream_t s);
// poco_outputs_t.record: [rotmat 216 | betas 10 | cam 3 | var 24 | post-processed confidence 1] per crop (254 floats)
void launch_pack_record(const float* rot, int rot_stride, const float* betas, int betas_stride, const float* cam, int cam_stride,
                        const float* var, int var_stride, float* rec, int cliff, int kinematic, float thr, int B, hipStream_t s);

// ---- demo renderer (render.hip) --------------------------------------------------------------------------
// Per person: RENDER_PARAMS floats (sx, sy, tx, ty, r, g, b, material) = include/poco_hip.h poco_renderer_render's d_params.
constexpr int RENDER_PARAMS = 8;
// q = m * v (row-major 3x3): the caller's rotation times Rx(180 deg), applied to vertices and normals.
struct RenderXform {
  float m[9];
};
// verts [P,V,3]; faces [F,3]; csr_off [V+1] / csr_face: the faces incident to each vertex, ascending; pos / nrm [P*V] scratch;
// vis [H*W] must hold all ones (no fragment) on entry; count [H*W] (nullable): +1 per fragment that passes coverage and clipping;
// frame uint8 [H,W,3], overwritten where a person covers a pixel centre.
void launch_render(const float* verts, int P, int V, const int* faces, int F, const int* csr_off, const int* csr_face,
                   const RenderXform& xf, const float* params, int H, int W, float4* pos, float4* nrm, unsigned long long* vis,
                   int* count, unsigned char* frame, hipStream_t s);
// The wireframe call: same arguments (verts is read again for the back-face test); count: +1 per line fragment.  F < 2^20.
void launch_render_wire(const float* verts, int P, int V, const int* faces, int F, const int* csr_off, const int* csr_face,
                        const RenderXform& xf, const float* params, int H, int W, float4* pos, float4* nrm, unsigned long long* vis,
                        int* count, unsigned char* frame, hipStream_t s);
// ids [n] <- the low 22 bits of each visibility key, -1 where the key is empty (POCO_RENDER_IDS).
void launch_render_ids(const unsigned long long* vis, int n, int* ids, hipStream_t s);
// Half-widths of a filled disc stamp per |dy| = 0 .. r (include/poco_hip.h POCO_DISC_HALF_WIDTHS).
constexpr int RENDER_DISC_MAX_RADIUS = 8;
struct DiscRows {
  int hw[RENDER_DISC_MAX_RADIUS + 1];
};
// points fp32 [N,2] (col, row), rgb uint8 [N,3]: stamps painted over frame in index order.
void launch_render_discs(unsigned char* frame, int H, int W, const float* points, const unsigned char* rgb, int N, int r,
                         const DiscRows& rows, hipStream_t s);

// ---- occlusion sensitivity sweep (occlusion.hip) -----------------------------------------------------------
// out [m,3,res,res] = src [3,res,res] with fill3[c] inside the patch x patch square at pos[i] = (y0, x0); res % 4 == 0, src and out
// 16-byte aligned.
void launch_occlude_batch(const float* src, const int* pos, int m, int res, int patch, const float* fill3, float* out,
                          hipStream_t s);
// rec [m,77] of rows verts [m,V,3] / var [m,24] / j3d [m,49,3] against one baseline row; V even, verts and base_verts 8-byte aligned.
void launch_occlusion_records(const float* verts, const float* var, const float* j3d, int m, int V, const float* base_verts,
                              const float* base_var, const float* base_j3d, float* rec, hipStream_t s);
// out uint8 [res,res,3] = crop blended with lut[index of the per-pixel mean of field over the covering patches]; scale 0 = the
// field's maximum.
void launch_heat_overlay(const float* field, const int* pos, int n, int patch, int res, float scale, const unsigned char* lut,
                         const unsigned char* crop, unsigned char* out, hipStream_t s);

// ---- body-part labels and their crop camera (part_labels.hip) -------------------------------------------------
// labels uint8 [B,res,res] <- face_part[nearest face] + 1 at every covered pixel centre, 0 elsewhere; verts [B,V,3], cam_t [B,3],
// faces [F,3], face_part uint8 [F]; keys [B*res*res] must hold all ones (no fragment) on entry.
void launch_part_labels(const float* verts, int B, int V, const float* cam_t, const int* faces, int F, const unsigned char* face_part,
                        float focal, int res, unsigned long long* keys, unsigned char* labels, hipStream_t s);
// cam_t [B,3] <- the weighted least-squares translation of j3d [B,J,3] onto j2d [B,J,3] (x, y, confidence); J <= POCO_EST_MAX_JOINTS.
constexpr int POCO_EST_MAX_JOINTS = 64;
void launch_estimate_translation(const float* j3d, const float* j2d, int B, int J, float focal, int res, float* cam_t, hipStream_t s);

// ---- per-part visibility counts (part_visibility.hip) ---------------------------------------------------------------
// counts int32 [B,24,4] += (total, area, front, seen) of every part: they must be zero on entry, as bits [B, (res + 2 margin)^2];
// keys [B*res*res] must hold all ones; occ_mask uint8 [B,res,res] or null.
void launch_part_visibility(const float* verts, int B, int V, const float* cam_t, const int* faces, int F, const unsigned char* face_part,
                            float focal, int res, int margin, const unsigned char* occ_mask, unsigned long long* keys, unsigned int* bits,
                            int* counts, hipStream_t s);

// ---- segmentation scoring (segm_metrics.hip) ---------------------------------------------------------------------
constexpr int POCO_SEGM_MAX_CLASSES = 32;
// label rows one block owns / blocks per crop = ceil(H / rows); dynamic LDS bytes of a launch
int segm_tile_rows(int h, int H);
size_t segm_score_lds_bytes(int C, int w);
// records [B, 2 + 3C] 64-bit words: word 0 <- the cross-entropy sum (fp64), words 1.. += the counts (they must be zero on entry);
// partials: B * ceil(H / segm_tile_rows(h, H)) doubles of scratch.
void launch_segm_score(const float* logits, const unsigned char* labels, int B, int C, int h, int w, int H, int W,
                       unsigned long long* records, double* partials, hipStream_t s);
// out uint8 [B,H,W] <- the argmax over the C channels of the upsampled logits (the scorer's interpolation and tie rule)
void launch_segm_argmax(const float* logits, int B, int C, int h, int w, int H, int W, unsigned char* out, hipStream_t s);

// ---- video mode's in-fill of unreliable joint rotations (track_infill.hip) -------------------------------------------
// include/poco_hip.h poco_op_track_infill: P tracks = rows [offsets[p], offsets[p + 1]) of N; pose [N,24,3,3], u [N,24], frames [N],
// lin [N,L]; scratch = 24 * N ints; outputs pose_out, lin_out, flags uint8 [N,24], touched uint8 [N]; rows [N] / count [1] nullable.
// Columns are dealt to at most TRACK_INFILL_MAX_BLOCKS one-wave blocks by a grid-stride loop.
constexpr int TRACK_INFILL_MAX_BLOCKS = 4096;
void launch_track_infill(const float* pose, const float* u, const int* frames, const int* offsets, int P, int N, const float* lin, int L,
                         float thresh, int max_gap, int* scratch, float* pose_out, float* lin_out, unsigned char* flags,
                         unsigned char* touched, int* rows, int* count, hipStream_t s);

// ---- choosing between two regressors by their uncertainty (select_regressor.hip) ------------------------------------------
// include/poco_hip.h poco_op_select_regressor: B rows of two models' pose [B,24,3,3] / var [B,24] and up to SELECT_MAX_PAYLOADS
// payload arrays of `width` floats per row (src0, src1 -> dst); outputs pose_out, var_out, choice uint8 [B,24], score [B,2],
// mixed uint8 [B]; rows [B] / count [1] nullable.  Rows are dealt to at most SELECT_MAX_BLOCKS blocks (max_blocks > 0: at most
// that many) by a grid-stride loop.
constexpr int SELECT_MAX_BLOCKS = 1024;
constexpr int SELECT_MAX_PAYLOADS = 8;
struct SelectPayload {
  const float *src0, *src1;
  float* dst;
  int width;
};
struct SelectPayloads {
  int count;
  SelectPayload p[SELECT_MAX_PAYLOADS];
};
void launch_select_regressor(const float* pose0, const float* var0, int kind0, const float* pose1, const float* var1, int kind1, int B,
                             int kinematic, double thr, double scale, int mode, const SelectPayloads& payloads, float* pose_out,
                             float* var_out, unsigned char* choice, float* score, unsigned char* mixed, int* rows, int* count,
                             int max_blocks, hipStream_t s);

// ---- test-time augmentation: fusing K views of a crop by their uncertainty (tta_fuse.hip) -------------------------------------
// include/poco_hip.h poco_op_tta_fuse: K views of B crops, view-major (row k * B + b): pose [K*B,24,3,3], var [K*B,24], betas
// [K*B,10] -> pose_out [B,24,3,3], var_out / spread [B,24], betas_out [B,10].  One lane per (crop, joint), dealt to at most
// TTA_MAX_BLOCKS blocks of TTA_THREADS (max_blocks > 0: at most that many) by a grid-stride loop.
constexpr int TTA_MAX_BLOCKS = 1024;
constexpr int TTA_THREADS = 256;
constexpr int TTA_MAX_VIEWS = 8;
struct TtaViews {
  int count;
  int flip[TTA_MAX_VIEWS];
  double c[TTA_MAX_VIEWS], s[TTA_MAX_VIEWS];
};
void launch_tta_fuse(const float* pose, const float* var, const float* betas, int B, const TtaViews& views, int weight, float* pose_out,
                     float* var_out, float* spread, float* betas_out, int max_blocks, hipStream_t s);

// ---- rank-based uncertainty metrics: stable key sort, midranks, fp64 cut sums (rank_curve.hip) ------------------------------------
// include/poco_hip.h poco_op_rank_curve / poco_op_pearson64: key [n], vals [E][n] -> order int32 [n], rank fp64 [n], cuts fp64
// [E+1][K+1], cut_keys [K+1].  Tiles of RANK_TILE positions are dealt to at most RANK_MAX_BLOCKS blocks of RANK_THREADS (max_blocks
// > 0: at most that many) by a grid-stride loop.  The scratch buffer is the caller's: rank_scratch_layout gives the byte offset of
// every part of it (each a multiple of 256) and the total.
constexpr int RANK_TILE = 2048;
constexpr int RANK_THREADS = 256;
constexpr int RANK_MAX_BLOCKS = 1024;
struct RankScratch {
  int NT;                                                  // tiles
  size_t key_a, key_b, order_a, hist, totals, last_head, first_end, fwd, bwd, tsum, tprefix, bytes;
};
RankScratch rank_scratch_layout(long long n, int E);
void launch_rank_curve(const float* key, const float* vals, long long n, int E, int K, void* scratch, int32_t* order, double* rank,
                       double* cuts, float* cut_keys, int max_blocks, hipStream_t s);
void launch_pearson64(const double* x, const double* y, long long n, double* r, hipStream_t s);

// ---- video mode's uncertainty-weighted smoother (track_smooth.hip) ------------------------------------------------------------
// include/poco_hip.h poco_op_track_smooth: P tracks = rows [offsets[p], offsets[p + 1]) of N; pose [N,24,3,3], u [N,24], frames [N],
// lin [N,L]; scratch = N * (TRACK_SMOOTH_ROW_DOUBLES + L) doubles (a row: 216 + L solution columns, then 25 x 2 factor words);
// outputs pose_out, lin_out, shift [N,24].  (track, group of 7 joints) pairs are dealt to at most TRACK_SMOOTH_MAX_BLOCKS blocks of
// TRACK_SMOOTH_THREADS (max_blocks > 0: at most that many) by a grid-stride loop.
constexpr int TRACK_SMOOTH_MAX_BLOCKS = 4096;
constexpr int TRACK_SMOOTH_THREADS = 256;
constexpr int TRACK_SMOOTH_ROW_DOUBLES = 266;
void launch_track_smooth(const float* pose, const float* u, const int* frames, const int* offsets, int P, int N, const float* lin, int L,
                         double lam, double u_ref, int max_gap, double* scratch, float* pose_out, float* lin_out, float* shift,
                         int max_blocks, hipStream_t s);

// ---- the keypoint refit of demo.py / eval.py --kp_refit (kp_refit.hip) ---------------------------------------------------------------
// include/poco_hip.h poco_op_kp_refit: N independent rows; pose [N,24,3,3], u [N,24], jrest [N,24,3], kp [N,K,3], cam [N,5], norm [N];
// kp_joint [K] and parents [24] are HOST arrays (checked by the caller: -1..23, parents[j] in [0, j) for j >= 1); outputs pose_out,
// cam_out [N,3], shift [N,24], cost [N,2], info int32 [N,2].  Rows are dealt to at most KP_REFIT_MAX_BLOCKS blocks of KP_REFIT_THREADS
// (max_blocks > 0: at most that many) by a grid-stride loop; a block keeps its row in 41 KB of LDS.
constexpr int KP_REFIT_MAX_BLOCKS = 4096;
constexpr int KP_REFIT_THREADS = 128;
constexpr int KP_REFIT_MAX_KP = 32;
constexpr int KP_REFIT_MAX_ITERS = 32;
void launch_kp_refit(const float* pose, const float* u, const float* jrest, const float* kp, const float* cam, const float* norm, int N,
                     int K, const int* kp_joint, const int* parents, double lam, double u_ref, double rho, double cam_prior,
                     double conf_thresh, int min_kp, int iters, float* pose_out, float* cam_out, float* shift, float* cost, int* info,
                     int max_blocks, hipStream_t s);

// ---- the temporal metric of eval.py --sequences: acceleration and acceleration error per row (track_accel.hip) -------------------
// include/poco_hip.h poco_op_track_accel: P tracks = rows [offsets[p], offsets[p + 1]) of N; pred / gt [N,M,3] at a row stride in
// floats (gt nullable); scratch = TRACK_ACCEL_ROW_DOUBLES doubles per row (acceleration error, acceleration, valid: the fp64 terms
// of the sums); outputs accel / accel_err [N], track_sums fp64 [P,3], total fp64 [3].  Tiles of TRACK_ACCEL_TILE rows, then tracks,
// are dealt to at most TRACK_ACCEL_MAX_BLOCKS blocks of TRACK_ACCEL_THREADS (max_blocks > 0: at most that many) by grid-stride loops.
constexpr int TRACK_ACCEL_MAX_BLOCKS = 4096;
constexpr int TRACK_ACCEL_THREADS = 256;
constexpr int TRACK_ACCEL_TILE = 64;
constexpr int TRACK_ACCEL_MAX_JOINTS = 32;
constexpr int TRACK_ACCEL_ROW_DOUBLES = 3;
void launch_track_accel(const float* pred, const float* gt, int stride, int M, const int* frames, const int* offsets, int P, int N,
                        double* scratch, float* accel, float* accel_err, double* track_sums, double* total, int max_blocks, hipStream_t s);

// ---- SORT: tracks from per-frame detections, video mode's --tracker sort (sort_tracks.hip) -------------------------------------------
// include/poco_hip.h poco_op_sort_tracks: C clips = frames [clip_offsets[c], clip_offsets[c + 1]) of F, a frame = detections
// [frame_offsets[f], frame_offsets[f + 1]) of N; dets fp64 [N,4] (cx, cy, w, h); outputs tracker / id int32 [N], box fp64 [N,4],
// count / status int32 [C].  One block of SORT_THREADS (one wave) per clip, the frames a sequential loop inside it; at most
// SORT_MAX people (detections of a frame, live trackers).
constexpr int SORT_THREADS = 64;
constexpr int SORT_MAX = 64;
void launch_sort_tracks(const double* dets, const int* frame_offsets, const int* clip_offsets, int C, int F, int N, double iou_thresh,
                        int max_age, int min_hits, int max_trackers, int* tracker, int* id, double* box, int* count, int* status,
                        hipStream_t s);

// ---- video mode's --track_stitch: fragments of tracks joined into chains by shape and motion (track_stitch.hip) ------------------------
// include/poco_hip.h poco_op_track_stitch: C clips = fragments [clip_offsets[c], clip_offsets[c + 1]) of P, a fragment = rows
// [frag_offsets[p], frag_offsets[p + 1]) of N; frames int32 [N], boxes fp64 [N,4], betas fp32 [N,10], var fp32 [N,24]; scratch =
// STITCH_MAX_FRAGS doubles per fragment (its row of the clip's gain matrix); outputs succ / pred / chain int32 [P], gain fp64 [P],
// desc fp64 [P,STITCH_DESC], status int32 [C].  A block of STITCH_ROW_THREADS per fragment, then blocks of STITCH_THREADS per
// fragment and per clip; at most STITCH_MAX_FRAGS fragments in a clip.
constexpr int STITCH_THREADS = 256;
constexpr int STITCH_ROW_THREADS = 64;
constexpr int STITCH_MAX_FRAGS = 256;
constexpr int STITCH_MAX_FIT = 32;
constexpr int STITCH_DESC = 28;
void launch_track_stitch(const int* clip_offsets, const int* frag_offsets, const int* frames, const double* boxes, const float* betas,
                         const float* var, int C, int P, int N, int max_gap, int fit_len, double u_ref, double motion_tol,
                         double shape_tol, double shape_floor, double shape_w, double* scratch, int* succ, int* pred, int* chain,
                         double* gain, double* desc, int* status, hipStream_t s);

// ---- calibration: isotonic regression over ragged segments, and the fitted maps evaluated (isotonic.hip) --------------------------------
// include/poco_hip.h poco_op_isotonic / poco_op_calib_apply.  Everything works on tiles of ISO_TILE consecutive POSITIONS of the
// ragged buffer (segments are told apart by flags, so many small segments and one large one load the device alike), dealt to at
// most ISO_MAX_BLOCKS blocks of ISO_THREADS (max_blocks > 0: at most that many) by grid-stride loops.  The scratch buffer is the
// caller's: iso_scratch_layout gives the byte offset of every part of it (each a multiple of 256) and the total.
constexpr int ISO_TILE = 2048;
constexpr int ISO_THREADS = 256;
constexpr int ISO_MAX_BLOCKS = 1024;
constexpr int ISO_MAX_SEGS = 4096;
constexpr long long ISO_MAX_N = 1 << 26;
struct IsoScratch {
  int NT;                                                  // tiles
  size_t ys, ukey, flags, sum, lsum, len, head, nh, cp, after, fh, lh, fwd, bwd, nheads, hbase, total, bytes;
};
IsoScratch iso_scratch_layout(long long N);
void launch_isotonic(const float* key, const float* y, int M, const int* order, int N, const int* seg_offsets, int S, void* scratch,
                     int* block, double* fit, int* seg_blocks, double* knots, int max_blocks, hipStream_t s);
void launch_calib_apply(const float* x, long long R, int S, const int* map_ids, const int* map_offsets, int P, const double* knots,
                        int B, float* out, int max_blocks, hipStream_t s);

// ---- the cluster bootstrap of eval.py --bootstrap: unit moments and B resamples of the units (bootstrap.hip) ----------------------------
// include/poco_hip.h poco_op_bootstrap: planes fp32 [E][n], pairs int32 [P][2] on the HOST (checked by the caller), unit_offsets int32
// [U + 1] on the device or null (every row its own unit); outputs center fp64 [E], unit_mom fp64 [U][M], out fp64 [B + 1][M] with
// M = 1 + E + P, draw_counts uint32 [B][U] or null.  Tiles of BOOT_TILE rows, units (a wave each) and replicates (a block each) are dealt
// to at most BOOT_MAX_BLOCKS blocks of BOOT_THREADS (max_blocks > 0: at most that many) by grid-stride loops.  The scratch buffer is the
// caller's: boot_scratch_layout gives its one part (the per-tile partial sums of the planes) and the total.
constexpr int BOOT_TILE = 4096;
constexpr int BOOT_THREADS = 256;
constexpr int BOOT_MAX_BLOCKS = 4096;
constexpr int BOOT_MAX_PLANES = 16;
constexpr int BOOT_MAX_PAIRS = 16;
constexpr int BOOT_MAX_M = 1 + BOOT_MAX_PLANES + BOOT_MAX_PAIRS;
constexpr long long BOOT_MAX_N = 1 << 24;
constexpr long long BOOT_MAX_B = 65536;
struct BootScratch {
  int NT;                                                  // tiles
  size_t partial, bytes;
};
BootScratch boot_scratch_layout(long long n, int E);
void launch_bootstrap(const float* planes, long long n, int E, const int* pairs, int P, const int* unit_offsets, long long U, long long B,
                      unsigned long long seed, void* scratch, double* center, double* unit_mom, double* out, unsigned* draw_counts,
                      int max_blocks, hipStream_t s);
