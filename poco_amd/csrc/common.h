// Shared declarations for the POCO MI355X (gfx950) HIP library.
// Everything here is internal; the public surface is include/poco_hip.h.
#pragma once
#ifndef POCO_PROBES
#define POCO_PROBES 0     // 1: timing-probe builds (tools/build_exp.sh): the POCO_CONV_DBG / POCO_CONV_REPEAT environment switches exist; never in the shipped library
#endif
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

typedef float f32x4 __attribute__((ext_vector_type(4)));

#define POCO_HIP_CHECK(expr)                                                        \
  do {                                                                              \
    hipError_t _e = (expr);                                                         \
    if (_e != hipSuccess) {                                                         \
      poco_set_error(std::string(#expr) + ": " + hipGetErrorString(_e));            \
      return POCO_ERR_HIP;                                                          \
    }                                                                               \
  } while (0)

enum { POCO_OK = 0, POCO_ERR_ARG = 1, POCO_ERR_HIP = 2, POCO_ERR_STATE = 3, POCO_ERR_MISSING = 4,
       POCO_ERR_SHAPE = 5, POCO_ERR_TIMEOUT = 6 /* poco_op_mlp_chain: a grid barrier's bounded wait ran out */ };

void poco_set_error(const std::string& msg);
// Compute units of the current device (hipDeviceAttributeMultiprocessorCount; 256 on MI355X), cached per thread and device.
int poco_num_cus();

// ---------------------------------------------------------------------------------------------
// Convolution (implicit GEMM on v_mfma_f32_16x16x4_f32), NHWC activations.
// ---------------------------------------------------------------------------------------------

// Tile configuration for one conv launch.  MT/NT select the template instantiation (register
// tile of 16x16 MFMA blocks per wave: MT along pixels, NT along output channels); the rest are
// runtime parameters of the block decomposition.
struct ConvCfg {
  int MT;      // 16-pixel sub-tiles per wave            (4, 7 or 13)
  int NT;      // 16-channel sub-tiles per wave          (1..4)
  int WM;      // waves along pixels
  int WN;      // waves along output channels  (block = WM*WN waves)
  int R;       // output rows per slab
  int NI;      // slabs (row bands / whole images) per block
  int ALG;     // the algorithm, 0..14: one row of the table in conv_mfma.hip (conv_alg), which says what each one is and how it reads
               // the fields above
};
constexpr int CONV_CFG_INTS = 7;   // ints per configuration in the C ABI / tuning table
inline ConvCfg conv_cfg_from(const int* c) { return ConvCfg{c[0], c[1], c[2], c[3], c[4], c[5], c[6]}; }

// Activation layout ("L16", channel-slice-major NHWC): element (b, y, x, c) of a buffer with C channels lives at
//   ((b*H + y) * (C/16) + c/16) * (W*16) + x*16 + c%16
// i.e. a 16-channel slice of an image row is one contiguous run of W*64 bytes, so the per-slice halo-patch
// fetches of the conv kernels read whole cache lines.  For vectors (H = W = 1) this is plain [B][C].
// Channel offset `co` of a slice inside a wider buffer -> float offset (co/16)*W*16 + co%16.
inline size_t l16_chan_off(int co, int W) { return (size_t)(co >> 4) * W * 16 + (co & 15); }

// The orders a conv's weights are packed in, one per algorithm family that reads them in an order of its own.  Every conv has the
// plain fragment order (ConvDesc::wfrag, conv_pack_weights); the further ones are nullable: the engine packs a layout only for
// the ops that may run an algorithm that reads it (conv_alg(ALG)->layout).
enum ConvWLayout {
  CONV_W_PLAIN,       // ConvDesc::wfrag; its slot in ConvWeights stays empty
  CONV_W_WINO,        // 3x3 stride-1 only: Winograd F(2x2,3x3)-transformed weights (ALG 3 / 4)
  CONV_W_WINO4,       // 3x3 stride-1 only: F(4x4,3x3) weight fragments, 36 positions (ALG 7)
  CONV_W_WINO4P,      // the same weights in the LDS order of ALG 8 (conv_wino4p.hip)
  CONV_W_WINO4W,      // the same weights in the LDS order of ALG 13 (conv_wino4w.hip)
  CONV_W_WINO4G,      // 3x3 stride-1 convs on small planes: per-position GEMM fragments of ALG 11 (conv_wino4g.hip)
  CONV_W_SPLIT_F16,   // EXPERIMENT (ALG 12, gemm1x1h.hip): hi / lo fp16 halves of the 1x1 weights
  CONV_W_COUNT
};
struct ConvWeights { const float* of[CONV_W_COUNT] = {}; };
// Size (floats) and packer (host: OIHW weights x per-output-channel scale -> the layout's order) of each layout but the plain one,
// whose two take the kernel size as well.  {null, null}: the layout is not part of this build.
struct ConvWLayoutOps {
  size_t (*floats)(int Cin, int Cout16);
  void (*pack)(const float* w_oihw, const float* scale /*nullable*/, int Cout, int Cin, int Cout16, float* dst);
};
const ConvWLayoutOps& conv_w_layout(int layout);

struct ConvDesc {
  // activations: L16 (see above), each buffer may be a channel slice of a wider buffer
  const float* in;  int in_cs,  in_co;    // channel stride (channels per pixel of the buffer), offset
  const float* res; int res_cs, res_co;   // optional residual (same spatial shape as the output)
  float*       out; int out_cs, out_co;
  const float* wfrag;                     // weights in MFMA fragment order (see conv_pack_weights)
  ConvWeights w;                          // ... and in the orders of the algorithms that need their own, each nullable
  float* scratch = nullptr;               // ALG 11: V + M staging (conv_wino4g_scratch_floats), owned by the caller
  size_t scratch_floats = 0;
  float* sk_scratch = nullptr;            // ALG 14 (gemm1x1sk.hip): flags + partial accumulators (gemm1x1sk_scratch_floats), zeroed once by the owner
  size_t sk_scratch_floats = 0;
  unsigned* sk_err_host = nullptr;        // ... and the pinned host word its bounded waits raise
  unsigned sk_max_spins = 0;              // poll bound of those waits (0 = 2^21)
  // ALG 11 chaining (engine only): the previous conv already left this conv's V in scratch half `wg_vsel`; this conv leaves the
  // next conv's V in the other half (wg_mid_kernel) and writes its own output tensor only if somebody else still reads it
  int wg_skip_in = 0, wg_vsel = 0, wg_emit_next = 0, wg_store_y = 1;
  const float* bias;                      // [Cout_padded] folded BN shift / conv bias
  int B, H, W, Cin, Cout;                 // Cout = padded to a multiple of 16
  int ks, stride;                         // ks in {1,3}; pad = (ks-1)/2; stride in {1,2}
  int act;             // 0 none, 1 ReLU, 2 sigmoid, 3 ReLU on output channels >= relu_from only
  int res_after_act;   // residual added after the activation instead of before
  int relu_from;       // act == 3: first output channel (multiple of 16) that gets the ReLU (merged convs)
};

// Size (floats) of the packed weight buffer for a conv.
size_t conv_packed_weight_floats(int Cin, int Cout16, int ks);
// Pack OIHW weights (host) * per-output-channel scale into fragment order (host buffer).
// Cout16 >= Cout is Cout rounded up to a multiple of 16 (extra channels are zero).
void conv_pack_weights(const float* w_oihw, const float* scale /*nullable*/, int Cout, int Cin,
                       int ks, int Cout16, float* dst);
// K concatenation of `nsrc` convs that share their output channels (engine: Builder::concat_k; poco_op_conv1x1_dual):
//   sum_j (scale_j * conv_j(x_j) + shift_j)  =  [s_0 W_0 | s_1 W_1 | ...] . [x_0 ; x_1 ; ...] + sum_j shift_j
// w[j] is OIHW [Cout, C[j], ks, ks], scale[j] / shift[j] are [Cout].  The arithmetic is fixed: a merged weight is
// (float)((double)scale * w), a merged shift is summed in double in source order and rounded once.
inline void conv_concat_k_weights(const float* const* w, const float* const* scale, const float* const* shift, const int* C,
                                  int nsrc, int Cout, int ks, std::vector<float>* wout, std::vector<float>* bout) {
  const int taps = ks * ks;
  int K = 0, koff = 0;
  for (int j = 0; j < nsrc; ++j) K += C[j];
  wout->assign((size_t)Cout * K * taps, 0.f);
  std::vector<double> bsum(Cout, 0.0);
  for (int j = 0; j < nsrc; ++j) {
    for (int o = 0; o < Cout; ++o) {
      for (int k = 0; k < C[j] * taps; ++k)
        (*wout)[((size_t)o * K + koff) * taps + k] = (float)((double)scale[j][o] * w[j][(size_t)o * C[j] * taps + k]);
      bsum[o] += (double)shift[j][o];
    }
    koff += C[j];
  }
  bout->clear();
  for (double v : bsum) bout->push_back((float)v);
}
// Stem conv weights (Cin = 3, Cout = 64): OIHW [64,3,ks,ks] x scale[64] -> tap-major [ks*ks*3][64] (launch_stem_conv).
inline void stem_pack_weights(const float* w_oihw, const float* scale, int ks, std::vector<float>* dst) {
  dst->assign((size_t)ks * ks * 3 * 64, 0.f);
  for (int co = 0; co < 64; ++co)
    for (int c = 0; c < 3; ++c)
      for (int t = 0; t < ks * ks; ++t)
        (*dst)[((size_t)t * 3 + c) * 64 + co] = w_oihw[((size_t)co * 3 + c) * ks * ks + t] * scale[co];
}
// Heuristic tile choice.
ConvCfg conv_default_cfg(const ConvDesc& d);
// What the host has to know about one algorithm: the rows of the table in conv_mfma.hip.
enum ConvScratch { CONV_SCRATCH_NONE, CONV_SCRATCH_WG /* ConvDesc::scratch */, CONV_SCRATCH_SK /* ConvDesc::sk_scratch */, CONV_SCRATCH_KINDS };
struct ConvAlg {
  int alg;               // ConvCfg::ALG
  ConvWLayout layout;    // the weights it reads
  bool wino;             // a Winograd form: 3x3 stride-1 convs with no activation or a plain ReLU only (refuses act 2 / 3)
  int gran;              // channel strides / offsets of the activation slices must be multiples of this
  ConvScratch scratch;   // the caller-owned scratch it needs
  size_t (*lds_bytes)(const ConvDesc& d, const ConvCfg& cfg);      // 0 = the configuration is invalid for the conv
  int (*launch)(const ConvDesc& d, const ConvCfg& cfg, hipStream_t stream);
};
const ConvAlg* conv_alg(int ALG);      // null: no such algorithm
// Validate + launch.  Returns POCO_OK or an error code (message via poco_set_error).
int conv_launch(const ConvDesc& d, const ConvCfg& cfg, hipStream_t stream);
// LDS bytes a configuration needs (0 if invalid, an unknown ALG included).
size_t conv_lds_bytes(const ConvDesc& d, const ConvCfg& cfg);

// ---- small-M linear layers (linear_mfma.hip), ALG 5 -------------------------------------------------
bool linear_cfg_valid(const ConvDesc& d, const ConvCfg& cfg);
int linear_launch(const ConvDesc& d, const ConvCfg& cfg, hipStream_t stream);

// ---- 1x1 convs as a register-direct GEMM (gemm1x1.hip), ALG 6 ---------------------------------------
bool gemm1x1_cfg_valid(const ConvDesc& d, const ConvCfg& cfg);
int gemm1x1_launch(const ConvDesc& d, const ConvCfg& cfg, hipStream_t stream);
// ---- the same with coalesced global traffic and an LDS transposition (gemm1x1t.hip), ALG 9 -----------------
bool gemm1x1t_cfg_valid(const ConvDesc& d, const ConvCfg& cfg);
// ---- stream-K 1x1 GEMM (gemm1x1sk.hip), ALG 14 ---------------------------------------------------------
constexpr int SK_MAX_WAVES = 2048;                 // flags at the head of the scratch buffer
constexpr size_t SK_PART_FLOATS = (size_t)32768 * 256;   // partial accumulators: waves x tiles per wave tile x 256 floats
size_t gemm1x1sk_scratch_floats();
bool gemm1x1sk_cfg_valid(const ConvDesc& d, const ConvCfg& cfg);
int gemm1x1sk_launch(const ConvDesc& d, const ConvCfg& cfg, hipStream_t stream);
size_t gemm1x1t_lds_bytes(const ConvDesc& d, const ConvCfg& cfg);
int gemm1x1t_launch(const ConvDesc& d, const ConvCfg& cfg, hipStream_t stream);

#ifndef POCO_EXPERIMENTS
#define POCO_EXPERIMENTS 0      // 1: also build the labelled experiments (csrc/exp/*.hip, 3-deep rings of ALG 4); not in the shipped library
#endif
#if POCO_EXPERIMENTS
// ---- EXPERIMENT: 1x1 convs in split fp16 (hi + lo, 3 MFMAs of 16x16x32_f16 per product; exp/gemm1x1h.hip), ALG 12 -----------
size_t gemm1x1h_packed_floats(int Cin, int Cout16);
void gemm1x1h_pack_weights(const float* w_oi, const float* scale, int Cout, int Cin, int Cout16, float* dst);
bool gemm1x1h_cfg_valid(const ConvDesc& d, const ConvCfg& cfg);
int gemm1x1h_launch(const ConvDesc& d, const ConvCfg& cfg, hipStream_t stream);
#endif

// ---- Winograd F(4x4,3x3) as a position-batched GEMM for small planes (conv_wino4g.hip), ALG 11 --------------
size_t conv_wino4g_packed_floats(int Cin, int Cout16);
void conv_wino4g_pack_weights(const float* w_oihw, const float* scale, int Cout, int Cin, int Cout16, float* dst);
size_t conv_wino4g_scratch_floats(int B, int H, int W, int Cin, int Cout);
bool conv_wino4g_can_chain(int H, int W, int Cout, int next_Cin);
bool conv_wino4g_cfg_valid(const ConvDesc& d, const ConvCfg& cfg);
int conv_wino4g_launch(const ConvDesc& d, const ConvCfg& cfg, hipStream_t stream);

// ---- 3x3 convs as a register-direct gather GEMM (gemm3x3.hip), ALG 10 -------------------------------------
bool gemm3x3_cfg_valid(const ConvDesc& d, const ConvCfg& cfg);
int gemm3x3_launch(const ConvDesc& d, const ConvCfg& cfg, hipStream_t stream);

#include <vector>
// ---- Winograd F(4x4,3x3) (conv_wino4.hip), ALG 7 -------------------------------------------
size_t conv_wino4_packed_floats(int Cin, int Cout16);
void conv_wino4_pack_weights(const float* w_oihw, const float* scale, int Cout, int Cin, int Cout16, float* dst);
size_t conv_wino4_lds_bytes(const ConvDesc& d, const ConvCfg& cfg);
int conv_wino4_launch(const ConvDesc& d, const ConvCfg& cfg, hipStream_t stream);

// ---- Winograd F(4x4,3x3) with specialised waves (conv_wino4p.hip), ALG 8 ---------------------
size_t conv_wino4p_packed_floats(int Cin, int Cout16);
void conv_wino4p_pack_weights(const float* w_oihw, const float* scale, int Cout, int Cin, int Cout16, float* dst);
size_t conv_wino4p_lds_bytes(const ConvDesc& d, const ConvCfg& cfg);
int conv_wino4p_launch(const ConvDesc& d, const ConvCfg& cfg, hipStream_t stream);

// ---- Winograd F(4x4,3x3) with whole-position MFMA waves (conv_wino4w.hip), ALG 13 ---------------------
size_t conv_wino4w_packed_floats(int Cin, int Cout16);
void conv_wino4w_pack_weights(const float* w_oihw, const float* scale, int Cout, int Cin, int Cout16, float* dst);
size_t conv_wino4w_lds_bytes(const ConvDesc& d, const ConvCfg& cfg);
int conv_wino4w_launch(const ConvDesc& d, const ConvCfg& cfg, hipStream_t stream);

// ---- Winograd F(2x2,3x3) variant (conv_wino.hip) --------------------------------------------------
#include <vector>
// the layout ALG 3 / 4 read: [Cout][Cin][16] transformed filters (G g G^T, float64 on the host) in the order of conv_pack_weights(ks = 4)
size_t conv_wino_packed_floats(int Cin, int Cout16);
void conv_wino_pack_weights(const float* w_oihw, const float* scale, int Cout, int Cin, int Cout16, float* dst);
size_t conv_wino_lds_bytes(const ConvDesc& d, const ConvCfg& cfg);
int conv_wino_launch(const ConvDesc& d, const ConvCfg& cfg, hipStream_t stream);
