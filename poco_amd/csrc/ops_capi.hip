// C-ABI entry points for the stand-alone operators (used by tests, the tuner and bench.py).
// Declarations + reference citations: include/poco_hip.h.
#include "../../include/poco_hip.h"
#include "common.h"

#include <algorithm>
#include <cmath>
#include <mutex>
#include <vector>

static thread_local std::string g_last_error;
void poco_set_error(const std::string& msg) { g_last_error = msg; }

extern "C" const char* poco_last_error(void) { return g_last_error.c_str(); }

namespace {
struct DevBuf {
  float* p = nullptr;
  ~DevBuf() {
    if (p) (void)hipFree(p);
  }
  hipError_t upload(const std::vector<float>& h) {
    hipError_t e = hipMalloc(&p, h.size() * sizeof(float));
    if (e != hipSuccess) return e;
    return hipMemcpy(p, h.data(), h.size() * sizeof(float), hipMemcpyHostToDevice);
  }
};
}  // namespace

// The operand form of a conv: every activation a channel slice [co, co + width) of a buffer with `cs` channels per pixel, and the
// epilogue (ConvDesc::act / relu_from / res_after_act).  poco_op_conv2d is the dense case, poco_op_conv2d_ex exposes all of it.
struct ConvView {
  int in_cs, in_co, res_cs, res_co, out_cs, out_co;
  int act, relu_from, res_after_act;
};

// Host-side validation of a view, before any GPU work.  `alg`: the row of the caller's configuration (null = heuristic / unknown ALG).
static int conv_view_check(const char* who, const void* d_in, const void* h_w, const void* d_out, const void* d_res, int B, int H,
                           int W, int Cin, int Cout, int ks, int stride, const ConvView& v, const ConvAlg* alg) {
  auto bad = [&](const std::string& m) { poco_set_error(std::string(who) + ": " + m); return POCO_ERR_ARG; };
  if (!d_in || !h_w || !d_out) return bad("null pointer");
  if (B < 1 || H < 1 || W < 1 || Cin < 16 || Cout < 16) return bad("B, H, W must be >= 1 and Cin, Cout >= 16");
  if (Cout % 16) return bad("Cout must be a multiple of 16 (the engine pads; the bare op does not)");
  if (!(ks == 1 || ks == 3) || !(stride == 1 || stride == 2)) return bad("ks must be 1|3 and stride 1|2");
  if (v.act < 0 || v.act > 3) return bad("act must be 0 (none), 1 (ReLU), 2 (sigmoid) or 3 (ReLU from relu_from)");
  if (v.relu_from < 0 || (v.relu_from & 15) || v.relu_from > Cout) return bad("relu_from must be a multiple of 16 in [0, Cout]");
  if (v.res_after_act != 0 && v.res_after_act != 1) return bad("res_after_act must be 0 or 1");
  // what conv_launch admits: multiples of 4 (ALG 11 / 12: of 16).  On a plane the L16 layout itself needs whole 16-channel slices
  // (l16_chan_off of any other offset is no channel slice); only vectors (H = W = 1: plain [B][C] rows) can use the multiples of 4.
  const int gran = (H == 1 && W == 1) ? (alg ? alg->gran : 4) : 16;
  const int all = v.in_cs | v.in_co | v.out_cs | v.out_co | (d_res ? (v.res_cs | v.res_co) : 0);
  if (v.in_co < 0 || v.out_co < 0 || (d_res && v.res_co < 0) || (all & (gran - 1)))
    return bad("channel strides / offsets must be non-negative multiples of " + std::to_string(gran) +
               (gran == 4 ? " (rows, H = W = 1)" : " (L16 planes; ALG 11)"));
  if (v.in_cs < v.in_co + Cin) return bad("in_cs is smaller than in_co + Cin");
  if (v.out_cs < v.out_co + Cout) return bad("out_cs is smaller than out_co + Cout");
  if (d_res && v.res_cs < v.res_co + Cout) return bad("res_cs is smaller than res_co + Cout");
  return POCO_OK;
}

static int conv_common(const float* d_in, int B, int H, int W, int Cin, const float* h_w,
                       const float* h_scale, const float* h_shift, int Cout, int ks, int stride,
                       const float* d_res, const ConvView& v, float* d_out, const int* cfg7, int iters,
                       float* ms_out, hipStream_t stream, const char* who = "conv2d") {
  if (int rc = conv_view_check(who, d_in, h_w, d_out, d_res, B, H, W, Cin, Cout, ks, stride, v, (cfg7 && cfg7[0] > 0) ? conv_alg(cfg7[6]) : nullptr)) return rc;
  const int Cout16 = Cout;
  std::vector<float> packed(conv_packed_weight_floats(Cin, Cout16, ks));
  conv_pack_weights(h_w, h_scale, Cout, Cin, ks, Cout16, packed.data());
  std::vector<float> shift(Cout16, 0.f);
  if (h_shift)
    for (int i = 0; i < Cout; ++i) shift[i] = h_shift[i];
  DevBuf dw, db, dwu, dwl, dscr, dsk;
  POCO_HIP_CHECK(dw.upload(packed));
  POCO_HIP_CHECK(db.upload(shift));
  ConvDesc d{};
  auto layout = [&](int l, DevBuf* buf) -> hipError_t {
    std::vector<float> p(conv_w_layout(l).floats(Cin, Cout16));
    conv_w_layout(l).pack(h_w, h_scale, Cout, Cin, Cout16, p.data());
    const hipError_t e = buf->upload(p);
    d.w.of[l] = buf->p;
    return e;
  };
  // the layout and the scratch of the row of the configuration's ALG, where the conv has the shape that layout is packed for ...
  const ConvAlg* row = cfg7 ? conv_alg(cfg7[6]) : nullptr;
  const bool wino_shape = ks == 3 && stride == 1;
  const bool row_fits = row && (row->wino ? wino_shape : row->layout == CONV_W_PLAIN || (ks == 1 && Cin % 32 == 0));
  if (wino_shape) POCO_HIP_CHECK(layout(CONV_W_WINO, &dwu));      // ... and F(2x2) always: the heuristic may pick ALG 3
  if (row_fits && row->layout > CONV_W_WINO && conv_w_layout(row->layout).pack) POCO_HIP_CHECK(layout(row->layout, &dwl));
  if (row_fits && row->scratch == CONV_SCRATCH_WG) {      // V / M staging
    d.scratch_floats = conv_wino4g_scratch_floats(B, H, W, Cin, Cout16);
    POCO_HIP_CHECK(hipMalloc(&dscr.p, d.scratch_floats * sizeof(float)));
    POCO_HIP_CHECK(hipMemsetAsync(dscr.p, 0xFF, d.scratch_floats * sizeof(float), stream));   // NaN: the engine never initialises this staging either
    d.scratch = dscr.p;
  }
  if (row_fits && row->scratch == CONV_SCRATCH_SK) {      // flags (zero) + partial accumulators, the pinned error word
    static unsigned* sk_err = nullptr;
    if (!sk_err) { POCO_HIP_CHECK(hipHostMalloc(reinterpret_cast<void**>(&sk_err), 64, hipHostMallocMapped)); *sk_err = 0; }
    d.sk_scratch_floats = gemm1x1sk_scratch_floats();
    POCO_HIP_CHECK(hipMalloc(&dsk.p, d.sk_scratch_floats * sizeof(float)));
    POCO_HIP_CHECK(hipMemsetAsync(dsk.p, 0xFF, d.sk_scratch_floats * sizeof(float), stream));    // partial accumulators: NaN (never initialised by the engine)
    POCO_HIP_CHECK(hipMemsetAsync(dsk.p, 0, (size_t)SK_MAX_WAVES * sizeof(float), stream));      // flags: zero, as the owner must leave them (both on the kernels' stream)
    d.sk_scratch = dsk.p;
    d.sk_err_host = sk_err;
  }
  // the engine's form (run_op / conv_desc_of): pointers at the first channel of each slice (aptr), offsets 0, strides of the buffers
  const int pad = (ks - 1) / 2;
  const int Wo = (W + 2 * pad - ks) / stride + 1;
  d.in = d_in + l16_chan_off(v.in_co, W); d.in_cs = v.in_cs; d.in_co = 0;
  d.res = d_res ? d_res + l16_chan_off(v.res_co, Wo) : nullptr; d.res_cs = d_res ? v.res_cs : v.out_cs; d.res_co = 0;
  d.out = d_out + l16_chan_off(v.out_co, Wo); d.out_cs = v.out_cs; d.out_co = 0;
  d.wfrag = dw.p; d.bias = db.p;
  d.B = B; d.H = H; d.W = W; d.Cin = Cin; d.Cout = Cout16;
  d.ks = ks; d.stride = stride; d.act = v.act; d.res_after_act = v.res_after_act; d.relu_from = v.relu_from;
  ConvCfg cfg = conv_default_cfg(d);
  if (cfg7 && cfg7[0] > 0) cfg = conv_cfg_from(cfg7);
  int rc = conv_launch(d, cfg, stream);
  if (rc != POCO_OK) return rc;
  if (iters > 0 && ms_out) {
    hipEvent_t e0, e1;
    POCO_HIP_CHECK(hipEventCreate(&e0));
    POCO_HIP_CHECK(hipEventCreate(&e1));
    for (int i = 0; i < 3; ++i) conv_launch(d, cfg, stream);
    POCO_HIP_CHECK(hipEventRecord(e0, stream));
    for (int i = 0; i < iters; ++i) conv_launch(d, cfg, stream);
    POCO_HIP_CHECK(hipEventRecord(e1, stream));
    POCO_HIP_CHECK(hipEventSynchronize(e1));
    float ms = 0.f;
    POCO_HIP_CHECK(hipEventElapsedTime(&ms, e0, e1));
    *ms_out = ms / iters;
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
  }
  POCO_HIP_CHECK(hipStreamSynchronize(stream));
  if (d.sk_err_host && *reinterpret_cast<volatile unsigned*>(d.sk_err_host)) { poco_set_error("conv: a wait of the stream-K GEMM (ALG 14) timed out"); return POCO_ERR_HIP; }
  return POCO_OK;
}

extern "C" int poco_op_conv2d(const float* d_in, int B, int H, int W, int Cin, const float* h_weight,
                              const float* h_scale, const float* h_shift, int Cout, int ks, int stride,
                              const float* d_res, int relu, float* d_out, const int* cfg7,
                              void* stream) {
  const ConvView dense{Cin, 0, Cout, 0, Cout, 0, relu, 0, 0};
  return conv_common(d_in, B, H, W, Cin, h_weight, h_scale, h_shift, Cout, ks, stride, d_res, dense,
                     d_out, cfg7, 0, nullptr, (hipStream_t)stream);
}

extern "C" int poco_op_conv2d_ex(const float* d_in, int B, int H, int W, int Cin, int in_cs, int in_co, const float* h_weight,
                                 const float* h_scale, const float* h_shift, int Cout, int ks, int stride, const float* d_res,
                                 int res_cs, int res_co, int act, int relu_from, int res_after_act, float* d_out, int out_cs,
                                 int out_co, const int* cfg7, void* stream) {
  const ConvView v{in_cs, in_co, res_cs, res_co, out_cs, out_co, act, relu_from, res_after_act};
  return conv_common(d_in, B, H, W, Cin, h_weight, h_scale, h_shift, Cout, ks, stride, d_res, v, d_out, cfg7, 0, nullptr,
                     (hipStream_t)stream, "conv2d_ex");
}

extern "C" int poco_bench_conv2d(const float* d_in, int B, int H, int W, int Cin, const float* h_weight,
                                 int Cout, int ks, int stride, float* d_out, const int* cfg7, int iters,
                                 float* ms_out, int* cfg_used7, void* stream) {
  if (cfg_used7) {
    ConvDesc d{};
    d.B = B; d.H = H; d.W = W; d.Cin = Cin; d.Cout = Cout; d.ks = ks; d.stride = stride;
    ConvCfg c = (cfg7 && cfg7[0] > 0) ? conv_cfg_from(cfg7) : conv_default_cfg(d);
    cfg_used7[0] = c.MT; cfg_used7[1] = c.NT; cfg_used7[2] = c.WM;
    cfg_used7[3] = c.WN; cfg_used7[4] = c.R;  cfg_used7[5] = c.NI; cfg_used7[6] = c.ALG;
  }
  const ConvView dense{Cin, 0, Cout, 0, Cout, 0, 1, 0, 0};
  return conv_common(d_in, B, H, W, Cin, h_weight, nullptr, nullptr, Cout, ks, stride, nullptr, dense, d_out,
                     cfg7, iters, ms_out, (hipStream_t)stream);
}

// Time a list of tile configurations for one conv shape (weights/activations allocated and filled
// here once).  ms_out[i] < 0 marks a configuration that is invalid for the shape.
extern "C" int poco_tune_conv(int B, int H, int W, int Cin, int Cout, int ks, int stride, const int* cfgs7,
                              int ncfg, int iters, float* ms_out, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (!cfgs7 || !ms_out || ncfg < 1 || Cin % 16 || Cout % 16) {
    poco_set_error("poco_tune_conv: bad arguments");
    return POCO_ERR_ARG;
  }
  const bool with_res = iters < 0;                        // iters < 0: |iters| launches of the residual form
  if (with_res) {
    iters = -iters;
    if (Cin != Cout || stride != 1) { poco_set_error("poco_tune_conv: iters < 0 (residual form) needs Cin == Cout and stride 1"); return POCO_ERR_ARG; }
  }
  const int pad = (ks - 1) / 2;
  const int Ho = (H + 2 * pad - ks) / stride + 1, Wo = (W + 2 * pad - ks) / stride + 1;
  const size_t nin = (size_t)B * H * W * Cin, nout = (size_t)B * Ho * Wo * Cout;
  const size_t nw = conv_packed_weight_floats(Cin, Cout, ks);
  uint32_t st = 12345u;
  auto rnd = [&]() { st = st * 1664525u + 1013904223u; return ((st >> 8) & 0xffff) / 32768.0f - 1.0f; };
  std::vector<float> hin(nin), hw(nw), hb(Cout);
  for (auto& v : hin) v = rnd();
  const float ws = 1.0f / sqrtf((float)(Cin * ks * ks));
  for (auto& v : hw) v = rnd() * ws;
  for (auto& v : hb) v = rnd() * 0.1f;
  DevBuf din, dw, db, dout, dwu, dwu4, dwu4g, dscr;
  bool lay[CONV_W_COUNT] = {}, scr[CONV_SCRATCH_KINDS] = {};      // what the rows of the configurations read / need
  for (int i = 0; i < ncfg; ++i)
    if (const ConvAlg* a = conv_alg(cfgs7[CONV_CFG_INTS * i + 6])) lay[a->layout] = scr[a->scratch] = true;
  if (ks == 3 && stride == 1) {
    std::vector<float> hu((size_t)16 * Cin * Cout);
    for (auto& v : hu) v = rnd() * ws;
    POCO_HIP_CHECK(dwu.upload(hu));
    if (lay[CONV_W_WINO4] || lay[CONV_W_WINO4P] || lay[CONV_W_WINO4W]) {
      std::vector<float> hu4((size_t)36 * Cin * Cout + 2 * 9 * 256);          // (+ the slack ALG 13 reads behind the last n-tile)
      for (auto& v : hu4) v = rnd() * ws;
      POCO_HIP_CHECK(dwu4.upload(hu4));
    }
  }
  POCO_HIP_CHECK(din.upload(hin));
  POCO_HIP_CHECK(dw.upload(hw));
  POCO_HIP_CHECK(db.upload(hb));
  POCO_HIP_CHECK(hipMalloc(&dout.p, nout * sizeof(float)));
  ConvDesc d{};
  d.in = din.p; d.in_cs = Cin; d.out = dout.p; d.out_cs = Cout; d.wfrag = dw.p; d.bias = db.p;
  d.w.of[CONV_W_WINO] = dwu.p; d.w.of[CONV_W_WINO4] = d.w.of[CONV_W_WINO4P] = d.w.of[CONV_W_WINO4W] = dwu4.p;     // timing only: random fragments serve all orders
  if (lay[CONV_W_WINO4G] && ks == 3 && stride == 1 && H <= 16 && W <= 16) {
    std::vector<float> hg(conv_wino4g_packed_floats(Cin, Cout));
    for (auto& v : hg) v = rnd() * ws;
    POCO_HIP_CHECK(dwu4g.upload(hg));
    d.w.of[CONV_W_WINO4G] = dwu4g.p;
    d.scratch_floats = conv_wino4g_scratch_floats(B, H, W, Cin, Cout);
    POCO_HIP_CHECK(hipMalloc(&dscr.p, d.scratch_floats * sizeof(float)));
    d.scratch = dscr.p;
  }
  DevBuf dsk;
  if (scr[CONV_SCRATCH_SK]) {                                           // stream-K 1x1 GEMM: flags (zero) + partials, the pinned error word
    static unsigned* sk_err = nullptr;
    if (!sk_err) { POCO_HIP_CHECK(hipHostMalloc(reinterpret_cast<void**>(&sk_err), 64, hipHostMallocMapped)); *sk_err = 0; }
    d.sk_scratch_floats = gemm1x1sk_scratch_floats();
    POCO_HIP_CHECK(hipMalloc(&dsk.p, d.sk_scratch_floats * sizeof(float)));
    POCO_HIP_CHECK(hipMemsetAsync(dsk.p, 0, (size_t)SK_MAX_WAVES * sizeof(float), stream));
    d.sk_scratch = dsk.p;
    d.sk_err_host = sk_err;
  }
#if POCO_EXPERIMENTS
  DevBuf dwh;
  if (lay[CONV_W_SPLIT_F16] && ks == 1 && Cin % 32 == 0) {               // split-fp16 experiment: timing only, hi / lo halves of random weights
    std::vector<float> hw2((size_t)Cout * Cin), ph(gemm1x1h_packed_floats(Cin, Cout));
    for (auto& v : hw2) v = rnd() * ws;
    gemm1x1h_pack_weights(hw2.data(), nullptr, Cout, Cin, Cout, ph.data());
    POCO_HIP_CHECK(dwh.upload(ph));
    d.w.of[CONV_W_SPLIT_F16] = dwh.p;
  }
#endif
  d.B = B; d.H = H; d.W = W; d.Cin = Cin; d.Cout = Cout; d.ks = ks; d.stride = stride; d.act = 1;
  if (with_res) { d.res = din.p; d.res_cs = Cin; d.res_co = 0; }      // the residual form (conv2 of a BasicBlock: `out += x`): the input doubles as the residual
  hipEvent_t e0, e1;
  POCO_HIP_CHECK(hipEventCreate(&e0));
  POCO_HIP_CHECK(hipEventCreate(&e1));
  for (int i = 0; i < ncfg; ++i) {
    const int* c = cfgs7 + CONV_CFG_INTS * i;
    ConvCfg cfg = conv_cfg_from(c);
    if (c[0] <= 0) cfg = conv_default_cfg(d);
    ms_out[i] = -1.f;
    if (conv_launch(d, cfg, stream) != POCO_OK) continue;
    conv_launch(d, cfg, stream);
    POCO_HIP_CHECK(hipEventRecord(e0, stream));
    for (int k = 0; k < iters; ++k) conv_launch(d, cfg, stream);
    POCO_HIP_CHECK(hipEventRecord(e1, stream));
    POCO_HIP_CHECK(hipEventSynchronize(e1));
    float ms = 0.f;
    POCO_HIP_CHECK(hipEventElapsedTime(&ms, e0, e1));
    ms_out[i] = ms / iters;
  }
  (void)hipEventDestroy(e0);
  (void)hipEventDestroy(e1);
  return POCO_OK;
}

#include "kernels.h"
static int crop_common(const unsigned char* d_frame, int H, int W, const void* d_boxes, int f64, int N, double bbox_scale,
                       int res, float* d_out, void* stream) {
  if (!d_frame || !d_boxes || !d_out || N < 0 || H < 1 || W < 1 || res < 1 || H > 32767 || W > 32767) {
    poco_set_error("poco_crop_normalize: bad arguments (frame up to 32767 x 32767: cv2.warpAffine's int16 coordinate maps)");
    return POCO_ERR_ARG;
  }
  if (N == 0) return POCO_OK;
  if (f64) launch_crop_normalize_f64(d_frame, H, W, (const double*)d_boxes, bbox_scale, d_out, N, res, (hipStream_t)stream);
  else launch_crop_normalize(d_frame, H, W, (const float*)d_boxes, bbox_scale, d_out, N, res, (hipStream_t)stream);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) { poco_set_error(std::string("poco_crop_normalize: ") + hipGetErrorString(e)); return POCO_ERR_HIP; }
  return POCO_OK;
}

extern "C" int poco_crop_normalize(const unsigned char* d_frame, int H, int W, const float* d_boxes, int N,
                                   double bbox_scale, int res, float* d_out, void* stream) {
  return crop_common(d_frame, H, W, d_boxes, 0, N, bbox_scale, res, d_out, stream);
}

extern "C" int poco_crop_normalize_multi(const unsigned char* const* d_frames, int nframes, const int* d_frame_idx, int H, int W,
                                         const float* d_boxes, int N, double bbox_scale, int res, float* d_out, void* stream) {
  if (!d_frames || !d_frame_idx || nframes < 1 || !d_boxes || !d_out || N < 0 || H < 1 || W < 1 || res < 1 || H > 32767 || W > 32767) {
    poco_set_error("poco_crop_normalize_multi: bad arguments (frames up to 32767 x 32767)");
    return POCO_ERR_ARG;
  }
  if (N == 0) return POCO_OK;
  launch_crop_normalize_multi(d_frames, nframes, d_frame_idx, H, W, d_boxes, bbox_scale, d_out, N, res, (hipStream_t)stream);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) { poco_set_error(std::string("poco_crop_normalize_multi: ") + hipGetErrorString(e)); return POCO_ERR_HIP; }
  return POCO_OK;
}

extern "C" int poco_crop_normalize_f64(const unsigned char* d_frame, int H, int W, const double* d_boxes, int N,
                                       double bbox_scale, int res, float* d_out, void* stream) {
  return crop_common(d_frame, H, W, d_boxes, 1, N, bbox_scale, res, d_out, stream);
}

// ---- head operators on their own (parity tests against vectors made by the reference's modules) --------------------------
#include "kernels.h"

extern "C" int poco_op_part_attention(const float* d_heat, int heat_cs, const float* d_feat, int C, int B, int H, int W,
                                      float* d_out, void* stream) {
  if (!d_heat || !d_feat || !d_out) { poco_set_error("part_attention: null pointer"); return POCO_ERR_ARG; }
  if (heat_cs < 32 || (heat_cs & 15) || C < 16 || C > 128 || (C & 15) || B < 1 || H < 1 || W < 1) {
    poco_set_error("part_attention: needs heat_cs >= 32 and C <= 128, both multiples of 16 (L16 layout)");
    return POCO_ERR_ARG;
  }
  float* scratch = nullptr;
  POCO_HIP_CHECK(hipMalloc(&scratch, part_attention_scratch_floats(B, C) * sizeof(float)));
  launch_part_attention_pool_ws(d_heat, heat_cs, d_feat, C, d_out, C * 24, B, H, W, scratch, (hipStream_t)stream);
  hipError_t e = hipGetLastError();
  if (e == hipSuccess) e = hipStreamSynchronize((hipStream_t)stream);
  (void)hipFree(scratch);
  POCO_HIP_CHECK(e);
  return POCO_OK;
}

// `iters` back-to-back launches of the pool between two HIP events on `stream` (scratch allocated once, outside the events).
extern "C" int poco_bench_part_attention(const float* d_heat, int heat_cs, const float* d_feat, int C, int B, int H, int W,
                                         float* d_out, int iters, float* ms_out, void* stream) {
  if (!d_heat || !d_feat || !d_out || !ms_out || iters < 1) { poco_set_error("bench_part_attention: bad argument"); return POCO_ERR_ARG; }
  if (heat_cs < 32 || (heat_cs & 15) || C < 16 || C > 128 || (C & 15) || B < 1 || H < 1 || W < 1) {
    poco_set_error("bench_part_attention: needs heat_cs >= 32 and C <= 128, both multiples of 16 (L16 layout)");
    return POCO_ERR_ARG;
  }
  hipStream_t s = (hipStream_t)stream;
  float* scratch = nullptr;
  POCO_HIP_CHECK(hipMalloc(&scratch, part_attention_scratch_floats(B, C) * sizeof(float)));
  hipEvent_t e0, e1;
  (void)hipEventCreate(&e0);
  (void)hipEventCreate(&e1);
  launch_part_attention_pool_ws(d_heat, heat_cs, d_feat, C, d_out, C * 24, B, H, W, scratch, s);
  (void)hipEventRecord(e0, s);
  for (int i = 0; i < iters; ++i) launch_part_attention_pool_ws(d_heat, heat_cs, d_feat, C, d_out, C * 24, B, H, W, scratch, s);
  (void)hipEventRecord(e1, s);
  hipError_t e = hipEventSynchronize(e1);
  float ms = 0.f;
  if (e == hipSuccess) e = hipEventElapsedTime(&ms, e0, e1);
  (void)hipEventDestroy(e0);
  (void)hipEventDestroy(e1);
  (void)hipFree(scratch);
  POCO_HIP_CHECK(e);
  *ms_out = ms / iters;
  return POCO_OK;
}

extern "C" int poco_op_lc2d_pose(const float* d_x, const float* d_w, float* d_pose6d, int B, void* stream) {
  if (!d_x || !d_w || !d_pose6d || B < 1) { poco_set_error("lc2d_pose: bad argument"); return POCO_ERR_ARG; }
  launch_lc2d_pose(d_x, 128 * 24, d_w, d_pose6d, B, (hipStream_t)stream);
  POCO_HIP_CHECK(hipGetLastError());
  return POCO_OK;
}

extern "C" int poco_op_rot6d(const float* d_in, float* d_rotmat, int B, void* stream) {
  if (!d_in || !d_rotmat || B < 1) { poco_set_error("rot6d: bad argument"); return POCO_ERR_ARG; }
  launch_rot6d(d_in, 144, d_rotmat, 216, nullptr, 0, B, (hipStream_t)stream);
  POCO_HIP_CHECK(hipGetLastError());
  return POCO_OK;
}

// ---- backbone side kernels and fused launches on their own (tests/test_engine_kernels_gpu.py) -------------------------------
// Every entry validates on the host before any GPU work, launches on `stream` and synchronises it before it returns (the
// temporary weight buffers live only that long).  Activations are L16; a pointer is at the first channel of its slice (aptr()).
namespace {
int op_bad(const char* who, const std::string& m) { poco_set_error(std::string(who) + ": " + m); return POCO_ERR_ARG; }
// a slice of `width` channels inside a buffer of `cs` channels per pixel
bool slice_ok(int cs, int width) { return cs >= width && (cs & 15) == 0; }
// the kernels move float4: every activation pointer must be 16-byte aligned
bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
int op_finish(const char* who, hipStream_t s) {
  hipError_t e = hipGetLastError();
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  if (e != hipSuccess) { poco_set_error(std::string(who) + ": " + hipGetErrorString(e)); return POCO_ERR_HIP; }
  return POCO_OK;
}
std::vector<float> ones_or(const float* p, int n, float dflt) {
  std::vector<float> v(n, dflt);
  if (p) v.assign(p, p + n);
  return v;
}
}  // namespace

extern "C" int poco_op_bneck_chain_resident_tiles(void) { return BNECK_CHAIN_MAX_BLOCKS * BNECK_CHAIN_WAVES; }

extern "C" int poco_op_bneck_chain(const float* d_t, int t_cs, const float* d_res, int res_cs, float* d_y, int y_cs, float* d_u,
                                   int u_cs, const float* h_w3, const float* h_scale3, const float* h_shift3, const float* h_w1,
                                   const float* h_scale1, const float* h_shift1, int B, int H, int W, void* stream) {
  const char* who = "bneck_chain";
  if (!d_t || !d_res || !d_y || !d_u || !h_w3 || !h_w1) return op_bad(who, "null pointer");
  if (B < 1 || H < 1 || W < 1 || (long)B * H * W >= (1L << 26)) return op_bad(who, "needs B, H, W >= 1 and fewer than 2^26 pixels");
  if (!slice_ok(t_cs, 64) || !slice_ok(u_cs, 64) || !slice_ok(res_cs, 256) || !slice_ok(y_cs, 256))
    return op_bad(who, "channel strides must be multiples of 16, t_cs / u_cs >= 64 and res_cs / y_cs >= 256");
  if ((long)B * H * W * std::max(std::max(t_cs, u_cs), std::max(res_cs, y_cs)) >= (1L << 31)) return op_bad(who, "buffer of 2^31 floats or more");
  // packed the way Builder::chain_op packs them
  std::vector<float> p3(conv_packed_weight_floats(64, 256, 1)), p1(conv_packed_weight_floats(256, 64, 1));
  conv_pack_weights(h_w3, h_scale3, 256, 64, 1, 256, p3.data());
  conv_pack_weights(h_w1, h_scale1, 64, 256, 1, 64, p1.data());
  DevBuf w3, b3, w1, b1;
  POCO_HIP_CHECK(w3.upload(p3));
  POCO_HIP_CHECK(b3.upload(ones_or(h_shift3, 256, 0.f)));
  POCO_HIP_CHECK(w1.upload(p1));
  POCO_HIP_CHECK(b1.upload(ones_or(h_shift1, 64, 0.f)));
  const int rc = launch_bneck_chain(d_t, t_cs, d_res, res_cs, d_y, y_cs, d_u, u_cs, w3.p, b3.p, w1.p, b1.p, B, H, W, (hipStream_t)stream);
  const int rs = op_finish(who, (hipStream_t)stream);
  return rc != POCO_OK ? rc : rs;
}

extern "C" int poco_op_conv1x1_dual(const float* d_a, int a_cs, int Ca, const float* d_b, int b_cs, int Cb, int H2, int W2,
                                    int stride2, const float* h_wa, const float* h_scale_a, const float* h_shift_a,
                                    const float* h_wb, const float* h_scale_b, const float* h_shift_b, float* d_out, int out_cs,
                                    int Cout, int B, int Ho, int Wo, int act, int wave_layout, void* stream) {
  const char* who = "conv1x1_dual";
  if (!d_a || !d_b || !d_out || !h_wa || !h_wb) return op_bad(who, "null pointer");
  if (B < 1 || Ho < 1 || Wo < 1 || H2 < 1 || W2 < 1 || Ca < 16 || Cb < 16 || Cout < 64) return op_bad(who, "empty shape");
  if ((Ca | Cb) % 16 || Cout % 64) return op_bad(who, "Ca, Cb must be multiples of 16 and Cout a multiple of 64");
  if (stride2 != 1 && stride2 != 2) return op_bad(who, "stride2 must be 1 or 2");
  if ((H2 - 1) / stride2 + 1 != Ho || (W2 - 1) / stride2 + 1 != Wo) return op_bad(who, "the second source's plane does not give Ho x Wo at stride2");
  if (!slice_ok(a_cs, Ca) || !slice_ok(b_cs, Cb) || !slice_ok(out_cs, Cout)) return op_bad(who, "channel strides must be multiples of 16 and at least the slice width");
  if (act != 0 && act != 1) return op_bad(who, "act must be 0 or 1");
  {                                // the launcher refuses an unknown layout too; asked here so that it happens before any GPU work
    int WM, WN, NI;
    if (!gemm1x1_dual_layout(wave_layout, &WM, &WN, &NI))
      return op_bad(who, "wave_layout = 100 NI + 10 WM + WN needs WM, WN >= 1, WM * WN <= 8 and NI in {0, 1, 3, 4, 5, 6}");
  }
  if ((long)B * Ho * Wo * std::max(a_cs, out_cs) >= (1L << 31) || (long)B * H2 * W2 * b_cs >= (1L << 31)) return op_bad(who, "buffer of 2^31 floats or more");
  // merged and packed the way Builder::bottleneck packs conv3+downsample
  const std::vector<float> sa = ones_or(h_scale_a, Cout, 1.f), sb = ones_or(h_scale_b, Cout, 1.f);
  const std::vector<float> ba = ones_or(h_shift_a, Cout, 0.f), bb = ones_or(h_shift_b, Cout, 0.f);
  const float* w[2] = {h_wa, h_wb};
  const float* sc[2] = {sa.data(), sb.data()};
  const float* sh[2] = {ba.data(), bb.data()};
  const int C[2] = {Ca, Cb};
  std::vector<float> mw, mb;
  conv_concat_k_weights(w, sc, sh, C, 2, Cout, 1, &mw, &mb);
  std::vector<float> packed(conv_packed_weight_floats(Ca + Cb, Cout, 1));
  conv_pack_weights(mw.data(), nullptr, Cout, Ca + Cb, 1, Cout, packed.data());
  DevBuf dw, db;
  POCO_HIP_CHECK(dw.upload(packed));
  POCO_HIP_CHECK(db.upload(mb));
  const int rc = launch_gemm1x1_dual(d_a, a_cs, Ca, d_b, b_cs, Cb, H2, W2, stride2, dw.p, db.p, d_out, out_cs, Cout, B, Ho, Wo, act,
                                     (hipStream_t)stream, wave_layout);
  const int rs = op_finish(who, (hipStream_t)stream);
  return rc != POCO_OK ? rc : rs;
}

extern "C" int poco_op_fuse_sum(int n, const float* const* d_src, const int* src_cs, const int* shift, float* d_out, int out_cs,
                                int B, int H, int W, int C, int relu, void* stream) {
  const char* who = "fuse_sum";
  if (!d_src || !src_cs || !shift || !d_out) return op_bad(who, "null pointer");
  if (n < 1 || n > 4) return op_bad(who, "1 to 4 terms");
  if (B < 1 || H < 1 || W < 1 || C < 16 || (C & 15)) return op_bad(who, "needs B, H, W >= 1 and C a multiple of 16");
  if (!slice_ok(out_cs, C)) return op_bad(who, "out_cs must be a multiple of 16 and at least C");
  if ((long)B * H * W * out_cs >= (1L << 31)) return op_bad(who, "buffer of 2^31 floats or more");
  FuseArgs fa{};
  fa.n = n;
  for (int k = 0; k < n; ++k) {
    if (!d_src[k]) return op_bad(who, "null term");
    if (shift[k] < 0 || shift[k] > 3 || (H & ((1 << shift[k]) - 1)) || (W & ((1 << shift[k]) - 1)))
      return op_bad(who, "a term's shift must be 0..3 and H, W multiples of 2^shift");
    if (!slice_ok(src_cs[k], C)) return op_bad(who, "a term's channel stride must be a multiple of 16 and at least C");
    fa.src[k] = d_src[k]; fa.shift[k] = shift[k]; fa.src_cs[k] = src_cs[k];
  }
  launch_fuse_sum(fa, d_out, B, H, W, C, out_cs, relu ? 1 : 0, (hipStream_t)stream);
  return op_finish(who, (hipStream_t)stream);
}

extern "C" int poco_op_bilinear_up2x(const float* d_in, float* d_out, int B, int H, int W, int C, void* stream) {
  const char* who = "bilinear_up2x";
  if (!d_in || !d_out) return op_bad(who, "null pointer");
  if (B < 1 || H < 1 || W < 1 || C < 16 || (C & 15)) return op_bad(who, "needs B, H, W >= 1 and C a multiple of 16");
  if ((long)B * 4 * H * W * C >= (1L << 31)) return op_bad(who, "buffer of 2^31 floats or more");
  launch_bilinear_up2x(d_in, d_out, B, H, W, C, (hipStream_t)stream);
  return op_finish(who, (hipStream_t)stream);
}

extern "C" int poco_op_maxpool3x3s2(const float* d_in, float* d_out, int B, int H, int W, int C, int out_cs, void* stream) {
  const char* who = "maxpool3x3s2";
  if (!d_in || !d_out) return op_bad(who, "null pointer");
  if (B < 1 || H < 1 || W < 1 || C < 16 || (C & 15)) return op_bad(who, "needs B, H, W >= 1 and C a multiple of 16");
  if (!slice_ok(out_cs, C)) return op_bad(who, "out_cs must be a multiple of 16 and at least C");
  if ((long)B * H * W * C >= (1L << 31) || (long)B * ((H - 1) / 2 + 1) * ((W - 1) / 2 + 1) * out_cs >= (1L << 31)) return op_bad(who, "buffer of 2^31 floats or more");
  launch_maxpool3x3s2(d_in, d_out, B, H, W, C, out_cs, (hipStream_t)stream);
  return op_finish(who, (hipStream_t)stream);
}

extern "C" int poco_op_avgpool(const float* d_in, float* d_dst, int B, int H, int W, int C, int dst_stride, void* stream) {
  const char* who = "avgpool";
  if (!d_in || !d_dst) return op_bad(who, "null pointer");
  if (B < 1 || H < 1 || W < 1 || C < 16 || (C & 15)) return op_bad(who, "needs B, H, W >= 1 and C a multiple of 16");
  if (dst_stride < C || (dst_stride & 3)) return op_bad(who, "dst_stride must be a multiple of 4 and at least C");
  if (!aligned16(d_in) || !aligned16(d_dst)) return op_bad(who, "d_in and d_dst must be 16-byte aligned (float4 loads / stores)");
  if ((long)B * H * W * C >= (1L << 31) || (long)B * dst_stride >= (1L << 31)) return op_bad(who, "buffer of 2^31 floats or more");
  launch_avgpool(d_in, d_dst, B, H, W, C, dst_stride, (hipStream_t)stream);
  return op_finish(who, (hipStream_t)stream);
}

extern "C" int poco_op_stem_conv(const float* d_img, const float* h_weight, const float* h_scale, const float* h_shift,
                                 float* d_out, int B, int H, int W, int ks, int use_mfma, void* stream) {
  const char* who = "stem_conv";
  if (!d_img || !h_weight || !d_out) return op_bad(who, "null pointer");
  if (ks != 3 && ks != 7) return op_bad(who, "ks must be 3 or 7");
  if (use_mfma != 0 && use_mfma != 1) return op_bad(who, "use_mfma must be 0 or 1");
  if (B < 1 || H < 1 || W < 1 || (long)B * 3 * H * W >= (1L << 31) || (long)B * ((H - 1) / 2 + 1) * ((W - 1) / 2 + 1) * 64 >= (1L << 31))
    return op_bad(who, "needs B, H, W >= 1 and fewer than 2^31 floats per tensor");
  std::vector<float> wt;
  stem_pack_weights(h_weight, ones_or(h_scale, 64, 1.f).data(), ks, &wt);     // as Builder::stem packs them
  DevBuf dw, db;
  POCO_HIP_CHECK(dw.upload(wt));
  POCO_HIP_CHECK(db.upload(ones_or(h_shift, 64, 0.f)));
  launch_stem_conv(d_img, dw.p, db.p, d_out, B, H, W, ks, (hipStream_t)stream, use_mfma);
  return op_finish(who, (hipStream_t)stream);
}

// ---- head kernels on their own, at any stride (tests/test_head_kernels_gpu.py) ----------------------------------------------
namespace {
// B rows of `width` floats, `stride` apart
bool rows_ok(int stride, int width, int B) { return stride >= width && (long)B * stride < (1L << 31); }
}  // namespace

extern "C" int poco_op_rot6d_ex(const float* d_in, int in_stride, float* d_dst0, int stride0, float* d_dst1, int stride1, int B,
                                void* stream) {
  const char* who = "rot6d_ex";
  if (!d_in || (!d_dst0 && !d_dst1)) return op_bad(who, "null pointer (d_in, or both destinations)");
  if (B < 1) return op_bad(who, "needs B >= 1");
  if (!rows_ok(in_stride, 144, B)) return op_bad(who, "in_stride must be at least 144 and B * in_stride below 2^31");
  if ((d_dst0 && !rows_ok(stride0, 216, B)) || (d_dst1 && !rows_ok(stride1, 216, B)))
    return op_bad(who, "a destination's stride must be at least 216 and B * stride below 2^31");
  launch_rot6d(d_in, in_stride, d_dst0, stride0, d_dst1, stride1, B, (hipStream_t)stream);
  return op_finish(who, (hipStream_t)stream);
}

extern "C" int poco_op_lc2d_pose_ex(const float* d_x, int x_stride, const float* d_w, float* d_pose6d, int B, void* stream) {
  const char* who = "lc2d_pose_ex";
  if (!d_x || !d_w || !d_pose6d) return op_bad(who, "null pointer");
  if (B < 1) return op_bad(who, "needs B >= 1");
  if (!rows_ok(x_stride, 128 * 24, B)) return op_bad(who, "x_stride must be at least 3072 and B * x_stride below 2^31");
  launch_lc2d_pose(d_x, x_stride, d_w, d_pose6d, B, (hipStream_t)stream);
  return op_finish(who, (hipStream_t)stream);
}

extern "C" int poco_op_copy_rows(const float* d_src, int src_stride, float* d_dst, int dst_stride, int n, int B, void* stream) {
  const char* who = "copy_rows";
  if (!d_src || !d_dst) return op_bad(who, "null pointer");
  if (B < 1 || n < 1) return op_bad(who, "needs B, n >= 1");
  if (!rows_ok(src_stride, n, B) || !rows_ok(dst_stride, n, B)) return op_bad(who, "strides must be at least n and B * stride below 2^31");
  launch_copy_rows(d_src, src_stride, d_dst, dst_stride, n, B, (hipStream_t)stream);
  return op_finish(who, (hipStream_t)stream);
}

extern "C" int poco_op_broadcast_rows(const float* d_src, float* d_dst, int dst_stride, int n, int B, void* stream) {
  const char* who = "broadcast_rows";
  if (!d_src || !d_dst) return op_bad(who, "null pointer");
  if (B < 1 || n < 1) return op_bad(who, "needs B, n >= 1");
  if (!rows_ok(dst_stride, n, B)) return op_bad(who, "dst_stride must be at least n and B * dst_stride below 2^31");
  launch_broadcast_rows(d_src, d_dst, dst_stride, n, B, (hipStream_t)stream);
  return op_finish(who, (hipStream_t)stream);
}

extern "C" int poco_op_nhwc_to_nchw(const float* d_in, int cs, float* d_out, int B, int H, int W, int C, void* stream) {
  const char* who = "nhwc_to_nchw";
  if (!d_in || !d_out) return op_bad(who, "null pointer");
  if (B < 1 || H < 1 || W < 1 || C < 1) return op_bad(who, "needs B, H, W, C >= 1");
  if (cs < C || (cs & 15)) return op_bad(who, "cs must be a multiple of 16 and at least C");
  if ((double)B * H * W * cs >= 2147483648.0) return op_bad(who, "buffer of 2^31 floats or more");
  launch_nhwc_to_nchw(d_in, cs, d_out, B, H, W, C, (hipStream_t)stream);
  return op_finish(who, (hipStream_t)stream);
}

extern "C" int poco_op_pack_record(const float* d_rot, int rot_stride, const float* d_betas, int betas_stride, const float* d_cam,
                                   int cam_stride, const float* d_var, int var_stride, float* d_rec, int cliff, int kinematic,
                                   float thr, int B, void* stream) {
  const char* who = "pack_record";
  if (!d_rot || !d_betas || !d_cam || !d_var || !d_rec) return op_bad(who, "null pointer");
  if (B < 1 || (long)B * 254 >= (1L << 31)) return op_bad(who, "needs B >= 1 and fewer than 2^31 floats of records");
  if (!rows_ok(rot_stride, 216, B) || !rows_ok(betas_stride, 10, B) || !rows_ok(cam_stride, 3, B) || !rows_ok(var_stride, 24, B))
    return op_bad(who, "strides must be at least 216 (rot), 10 (betas), 3 (cam), 24 (var) and B * stride below 2^31");
  if ((cliff != 0 && cliff != 1) || (kinematic != 0 && kinematic != 1)) return op_bad(who, "cliff and kinematic must be 0 or 1");
  launch_pack_record(d_rot, rot_stride, d_betas, betas_stride, d_cam, cam_stride, d_var, var_stride, d_rec, cliff, kinematic, thr, B,
                     (hipStream_t)stream);
  return op_finish(who, (hipStream_t)stream);
}

extern "C" int poco_op_camera(const float* d_cam, int cam_stride, const float* d_joints49, int cliff, const float* d_focal,
                              const float* d_scale, const float* d_center, const float* d_orig_shape, float* d_cam_t,
                              float* d_fullimg_cam_t, float* d_joints2d, int B, void* stream) {
  const char* who = "camera";
  if (!d_cam || !d_joints49 || !d_cam_t || !d_joints2d) return op_bad(who, "null pointer");
  if (cliff != 0 && cliff != 1) return op_bad(who, "cliff must be 0 or 1");
  if (cliff && (!d_focal || !d_scale || !d_center || !d_orig_shape)) return op_bad(who, "cliff = 1 needs d_focal, d_scale, d_center and d_orig_shape");
  if (B < 1 || (long)B * 147 >= (1L << 31)) return op_bad(who, "needs B >= 1 and fewer than 2^31 floats of joints");
  if (!rows_ok(cam_stride, 3, B)) return op_bad(who, "cam_stride must be at least 3 and B * cam_stride below 2^31");
  CamArgs c{};
  c.cam = d_cam; c.cam_stride = cam_stride; c.joints49 = d_joints49; c.cliff = cliff;
  if (cliff) { c.focal = d_focal; c.scale = d_scale; c.center = d_center; c.orig_shape = d_orig_shape; }
  c.cam_t = d_cam_t; c.fullimg_cam_t = d_fullimg_cam_t; c.joints2d = d_joints2d;
  launch_camera(c, B, (hipStream_t)stream);
  return op_finish(who, (hipStream_t)stream);
}

extern "C" int poco_op_mlp_chain_resident_blocks(void) { return mlp_chain_resident_blocks(); }

static_assert(POCO_MLP_LAYER_INTS == 12 && POCO_MLP_ROW_INTS == 11, "poco_op_mlp_chain reads 12 ints per layer and 11 per row job");

extern "C" int poco_op_mlp_chain(const int* layers, int nlayers, const float* const* h_weights, const float* const* h_bias,
                                 const int* rows, int nrows, const int* stages, int nstages, float* const* d_bufs,
                                 const long long* buf_floats, int nbuf, int B, int max_blocks, void* stream) {
  const char* who = "mlp_chain";
  if (!stages || !d_bufs || !buf_floats || (nlayers > 0 && (!layers || !h_weights || !h_bias)) || (nrows > 0 && !rows))
    return op_bad(who, "null pointer");
  if (B < 1 || max_blocks < 1) return op_bad(who, "needs B >= 1 and max_blocks >= 1");
  if (nlayers < 0 || nlayers > MLP_MAX_LAYERS || nrows < 0 || nrows > MLP_MAX_ROWS || nstages < 1 || nstages > MLP_MAX_STAGES)
    return op_bad(who, "a program holds at most " + std::to_string(MLP_MAX_LAYERS) + " layers, " + std::to_string(MLP_MAX_ROWS) +
                       " row jobs and 1 to " + std::to_string(MLP_MAX_STAGES) + " stages");
  if (nbuf < 1 || nbuf > 64) return op_bad(who, "1 to 64 buffers");
  for (int i = 0; i < nbuf; ++i)
    if (!d_bufs[i] || !aligned16(d_bufs[i]) || buf_floats[i] < 1 || buf_floats[i] >= (1LL << 31))
      return op_bad(who, "buffer " + std::to_string(i) + " is null, not 16-byte aligned, empty or holds 2^31 floats or more");
  // rows [0, nr) of `width` floats at d_bufs[buf] + off + r * rs lie inside the buffer; `quad`: the kernel moves them as float4
  auto slice = [&](int buf, int off, int rs, int width, int nr, bool quad) {
    if (buf < 0 || buf >= nbuf || off < 0 || rs < width) return false;
    if (quad && ((off | rs) & 3)) return false;
    return (long long)off + (long long)(nr - 1) * rs + width <= buf_floats[buf];
  };
  MlpProgram p{};
  p.B = B; p.nstages = nstages;
  for (int l = 0; l < nlayers; ++l) {
    const int* q = layers + (size_t)l * POCO_MLP_LAYER_INTS;
    const std::string nm = "layer " + std::to_string(l);
    const int K = q[0], N = q[1], act = q[2];
    if (K < 16 || N < 16 || (K & 15) || (N & 15)) return op_bad(who, nm + ": K and N must be multiples of 16");
    if (act < 0 || act > 2) return op_bad(who, nm + ": act must be 0, 1 or 2");
    if (!h_weights[l] || !h_bias[l]) return op_bad(who, nm + ": null weights or bias");
    if (!slice(q[3], q[4], q[5], K, B, true)) return op_bad(who, nm + ": the input does not fit its buffer, or its offset / stride is no multiple of 4");
    if (q[6] >= 0 && !slice(q[6], q[7], q[8], N, B, true)) return op_bad(who, nm + ": the residual does not fit its buffer, or its offset / stride is no multiple of 4");
    if (!slice(q[9], q[10], q[11], N, B, true)) return op_bad(who, nm + ": the output does not fit its buffer, or its offset / stride is no multiple of 4");
    MlpLayer& L = p.layer[l];
    L.in = d_bufs[q[3]] + q[4]; L.in_rs = q[5];
    if (q[6] >= 0) { L.res = d_bufs[q[6]] + q[7]; L.res_rs = q[8]; }
    L.out = d_bufs[q[9]] + q[10]; L.out_rs = q[11];
    L.nC16 = K / 16; L.nT16 = N / 16; L.act = act;
  }
  for (int j = 0; j < nrows; ++j) {
    const int* q = rows + (size_t)j * POCO_MLP_ROW_INTS;
    const std::string nm = "row job " + std::to_string(j);
    const int kind = q[0];
    MlpRowJob& J = p.row[j];
    J = MlpRowJob{};
    J.kind = kind;
    if (kind == MLP_ROW_COPY || kind == MLP_ROW_BCAST) {
      const int n = q[10];
      if (n < 1) return op_bad(who, nm + ": n must be at least 1");
      if (!slice(q[1], q[2], kind == MLP_ROW_BCAST ? n : q[3], n, kind == MLP_ROW_BCAST ? 1 : B, false) || !slice(q[4], q[5], q[6], n, B, false))
        return op_bad(who, nm + ": source or destination does not fit its buffer");
      J.src = d_bufs[q[1]] + q[2]; J.src_rs = kind == MLP_ROW_BCAST ? 0 : q[3];
      J.dst = d_bufs[q[4]] + q[5]; J.dst_rs = q[6]; J.n = n;
    } else if (kind == MLP_ROW_ROT6D) {
      if (q[4] < 0 && q[7] < 0) return op_bad(who, nm + ": rot6d needs a destination");
      if (!slice(q[1], q[2], q[3], 144, B, false) || (q[4] >= 0 && !slice(q[4], q[5], q[6], 216, B, false)) ||
          (q[7] >= 0 && !slice(q[7], q[8], q[9], 216, B, false)))
        return op_bad(who, nm + ": source or destination does not fit its buffer");
      J.src = d_bufs[q[1]] + q[2]; J.src_rs = q[3];
      if (q[4] >= 0) { J.dst = d_bufs[q[4]] + q[5]; J.dst_rs = q[6]; }
      if (q[7] >= 0) { J.dst2 = d_bufs[q[7]] + q[8]; J.dst2_rs = q[9]; }
    } else {
      return op_bad(who, nm + ": kind must be 0 (copy), 1 (broadcast) or 2 (rot6d)");
    }
  }
  for (int s = 0; s < nstages; ++s) {
    const int* q = stages + (size_t)s * 4;
    if (q[0] < 0 || q[1] < 0 || q[0] + q[1] > nlayers || q[2] < 0 || q[3] < 0 || q[2] + q[3] > nrows)
      return op_bad(who, "stage " + std::to_string(s) + " names layers or row jobs outside the arrays");
    p.stage[s] = MlpStage{q[0], q[1], q[2], q[3]};
  }
  // weights packed the way the engine's builder packs a Linear (a 1x1 conv on a 1x1 plane)
  DevBuf wdev[MLP_MAX_LAYERS], bdev[MLP_MAX_LAYERS];
  for (int l = 0; l < nlayers; ++l) {
    const int K = p.layer[l].nC16 * 16, N = p.layer[l].nT16 * 16;
    std::vector<float> packed(conv_packed_weight_floats(K, N, 1));
    conv_pack_weights(h_weights[l], nullptr, N, K, 1, N, packed.data());
    POCO_HIP_CHECK(wdev[l].upload(packed));
    POCO_HIP_CHECK(bdev[l].upload(std::vector<float>(h_bias[l], h_bias[l] + N)));
    p.layer[l].wfrag = reinterpret_cast<const float4*>(wdev[l].p);
    p.layer[l].bias = bdev[l].p;
  }
  // the 1 KiB of barrier counters and the pinned time-out word live for this call only
  struct Sync {
    unsigned* dev = nullptr;
    unsigned* host = nullptr;
    ~Sync() {
      if (dev) (void)hipFree(dev);
      if (host) (void)hipHostFree(host);
    }
  } sy;
  POCO_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&sy.dev), 1024));
  POCO_HIP_CHECK(hipMemsetAsync(sy.dev, 0, 1024, (hipStream_t)stream));
  POCO_HIP_CHECK(hipHostMalloc(reinterpret_cast<void**>(&sy.host), 64, hipHostMallocMapped));
  *sy.host = 0;
  p.sync = sy.dev; p.err_host = sy.host;
  const int rc = launch_mlp_chain(p, max_blocks, (hipStream_t)stream);
  const int rs = op_finish(who, (hipStream_t)stream);
  if (rc != POCO_OK || rs != POCO_OK) return rc != POCO_OK ? rc : rs;
  if (*reinterpret_cast<volatile unsigned*>(sy.host)) {
    poco_set_error(std::string(who) + ": a grid barrier timed out");
    return POCO_ERR_TIMEOUT;
  }
  return POCO_OK;
}

// ---- demo renderer (csrc/render.hip) ------------------------------------------------------------------------------------
struct poco_renderer {
  int F = 0, V = 0;
  int* faces = nullptr;                    // [F,3]
  int* csr_off = nullptr;                  // [V+1]
  int* csr_face = nullptr;                 // [3F]
  unsigned long long* vis = nullptr;       // [vis_cap] visibility keys, grown on demand
  size_t vis_cap = 0;
  float4* scratch = nullptr;               // [2 * scratch_cap]: screen position / depth, then unit normals, per (person, vertex)
  size_t scratch_cap = 0;
  ~poco_renderer() {
    for (void* p : {(void*)faces, (void*)csr_off, (void*)csr_face, (void*)vis, (void*)scratch})
      if (p) (void)hipFree(p);
  }
};

static constexpr int RENDER_MAX_PEOPLE = 1024;          // 10 bits of the visibility key
static constexpr int RENDER_MAX_FACES = (1 << 22) - 1;  // 22 bits of the visibility key
static constexpr int RENDER_MAX_VERTS = 1 << 24;
static constexpr int RENDER_MAX_SIDE = 16384;

extern "C" int poco_renderer_create(const int32_t* h_faces, int F, int V, poco_renderer_t* out) {
  if (!out) { poco_set_error("poco_renderer_create: null handle pointer"); return POCO_ERR_ARG; }
  *out = nullptr;
  if (!h_faces || F < 1 || F > RENDER_MAX_FACES || V < 1 || V > RENDER_MAX_VERTS) {
    poco_set_error("poco_renderer_create: bad arguments (need faces, 1 <= F < 2^22, 1 <= V <= 2^24)");
    return POCO_ERR_ARG;
  }
  std::vector<int> off(V + 1, 0);
  for (size_t k = 0; k < (size_t)F * 3; ++k) {
    const int v = h_faces[k];
    if (v < 0 || v >= V) {
      poco_set_error("poco_renderer_create: face " + std::to_string(k / 3) + " has vertex index " + std::to_string(v) +
                     " outside [0, " + std::to_string(V) + ")");
      return POCO_ERR_ARG;
    }
    ++off[v + 1];
  }
  for (int v = 0; v < V; ++v) off[v + 1] += off[v];
  std::vector<int> fill(off.begin(), off.end() - 1), inc((size_t)F * 3);
  for (int f = 0; f < F; ++f)                     // ascending face index per vertex: the normal sum has a fixed order
    for (int j = 0; j < 3; ++j) inc[fill[h_faces[3 * f + j]]++] = f;
  auto* r = new poco_renderer;
  r->F = F;
  r->V = V;
  auto up = [](int** d, const int* h, size_t n) -> hipError_t {
    hipError_t e = hipMalloc(d, n * sizeof(int));
    return e != hipSuccess ? e : hipMemcpy(*d, h, n * sizeof(int), hipMemcpyHostToDevice);
  };
  hipError_t e = up(&r->faces, h_faces, (size_t)F * 3);
  if (e == hipSuccess) e = up(&r->csr_off, off.data(), off.size());
  if (e == hipSuccess) e = up(&r->csr_face, inc.data(), inc.size());
  if (e != hipSuccess) {
    delete r;
    poco_set_error(std::string("poco_renderer_create: ") + hipGetErrorString(e));
    return POCO_ERR_HIP;
  }
  *out = r;
  return POCO_OK;
}

// the one body of poco_renderer_render (flags = 0) and poco_renderer_render_ex
static int renderer_render(const char* who, poco_renderer_t r, unsigned char* d_frame, int H, int W, const float* d_verts, int P,
                           const float* d_params, const float* h_rot3x3, int* d_frag_count, unsigned flags, void* stream) {
  if (flags & ~(POCO_RENDER_WIREFRAME | POCO_RENDER_IDS)) {
    poco_set_error(std::string(who) + ": unknown flag bit (known: bit 0 = wireframe, bit 1 = winning ids)");
    return POCO_ERR_ARG;
  }
  const bool wire = flags & POCO_RENDER_WIREFRAME, ids = flags & POCO_RENDER_IDS;
  if (ids && !d_frag_count) {
    poco_set_error(std::string(who) + ": flag bit 1 (winning ids) needs d_frag_count");
    return POCO_ERR_ARG;
  }
  if (r && wire && r->F > POCO_RENDER_MAX_WIRE_FACES) {
    poco_set_error(std::string(who) + ": a wireframe call needs F < 2^20 faces (the key's 22 low bits hold triangle << 2 | edge)");
    return POCO_ERR_ARG;
  }
  if (!r || !d_frame || H < 1 || W < 1 || H > RENDER_MAX_SIDE || W > RENDER_MAX_SIDE || P < 0 || P > RENDER_MAX_PEOPLE ||
      (P > 0 && (!d_verts || !d_params))) {
    poco_set_error(std::string(who) + ": bad arguments (need a handle, a frame of 1..16384 x 1..16384, 0 <= P <= 1024 and, "
                   "for P > 0, vertices and parameters)");
    return POCO_ERR_ARG;
  }
  const hipStream_t s = (hipStream_t)stream;
  const size_t npix = (size_t)H * W;
  if (d_frag_count) POCO_HIP_CHECK(hipMemsetAsync(d_frag_count, ids ? 0xFF : 0, npix * sizeof(int), s));
  if (P == 0) return POCO_OK;
  const size_t nvert = (size_t)P * r->V;
  // growth frees the old buffer: hipFree waits for the device, so a render still in flight on another stream finishes first
  if (npix > r->vis_cap) {
    if (r->vis) (void)hipFree(r->vis);
    r->vis = nullptr;
    r->vis_cap = 0;
    POCO_HIP_CHECK(hipMalloc(&r->vis, npix * sizeof(unsigned long long)));
    r->vis_cap = npix;
  }
  if (nvert > r->scratch_cap) {
    if (r->scratch) (void)hipFree(r->scratch);
    r->scratch = nullptr;
    r->scratch_cap = 0;
    POCO_HIP_CHECK(hipMalloc(&r->scratch, 2 * nvert * sizeof(float4)));
    r->scratch_cap = nvert;
  }
  // q = R * Rx(180 deg) * v: Rx(180 deg) = diag(1, -1, -1) negates the 2nd and 3rd columns of R (exactly)
  RenderXform xf;
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) {
      const float rij = h_rot3x3 ? h_rot3x3[3 * i + j] : (i == j ? 1.f : 0.f);
      xf.m[3 * i + j] = j == 0 ? rij : -rij;
    }
  POCO_HIP_CHECK(hipMemsetAsync(r->vis, 0xFF, npix * sizeof(unsigned long long), s));
  (wire ? launch_render_wire : launch_render)(d_verts, P, r->V, r->faces, r->F, r->csr_off, r->csr_face, xf, d_params, H, W,
                                              r->scratch, r->scratch + nvert, r->vis, ids ? nullptr : d_frag_count, d_frame, s);
  if (ids) launch_render_ids(r->vis, (int)npix, d_frag_count, s);
  POCO_HIP_CHECK(hipGetLastError());
  return POCO_OK;
}

extern "C" int poco_renderer_render(poco_renderer_t r, unsigned char* d_frame, int H, int W, const float* d_verts, int P,
                                    const float* d_params, const float* h_rot3x3, int* d_frag_count, void* stream) {
  return renderer_render("poco_renderer_render", r, d_frame, H, W, d_verts, P, d_params, h_rot3x3, d_frag_count, 0u, stream);
}

extern "C" int poco_renderer_render_ex(poco_renderer_t r, unsigned char* d_frame, int H, int W, const float* d_verts, int P,
                                       const float* d_params, const float* h_rot3x3, int* d_frag_count, unsigned flags,
                                       void* stream) {
  return renderer_render("poco_renderer_render_ex", r, d_frame, H, W, d_verts, P, d_params, h_rot3x3, d_frag_count, flags, stream);
}

extern "C" int poco_renderer_draw_discs(unsigned char* d_frame, int H, int W, const float* d_points, const unsigned char* d_rgb,
                                        int N, int r, void* stream) {
  static const int table[POCO_DISC_MAX_RADIUS + 1][POCO_DISC_MAX_RADIUS + 1] = POCO_DISC_HALF_WIDTHS;
  static_assert(POCO_DISC_MAX_RADIUS == RENDER_DISC_MAX_RADIUS, "the header's table and the kernel's argument must agree");
  if (!d_frame || H < 1 || W < 1 || H > RENDER_MAX_SIDE || W > RENDER_MAX_SIDE || N < 0 || N > 65536 || r < 0 ||
      r > POCO_DISC_MAX_RADIUS || (N > 0 && (!d_points || !d_rgb))) {
    poco_set_error("poco_renderer_draw_discs: bad arguments (need a frame of 1..16384 x 1..16384, 0 <= N <= 65536, 0 <= r <= 8 and, "
                   "for N > 0, points and colours)");
    return POCO_ERR_ARG;
  }
  if (N == 0) return POCO_OK;
  DiscRows rows;
  for (int k = 0; k <= POCO_DISC_MAX_RADIUS; ++k) rows.hw[k] = table[r][k];
  launch_render_discs(d_frame, H, W, d_points, d_rgb, N, r, rows, (hipStream_t)stream);
  POCO_HIP_CHECK(hipGetLastError());
  return POCO_OK;
}

extern "C" void poco_renderer_destroy(poco_renderer_t r) { delete r; }

// ---- occlusion sensitivity sweep (occlusion.hip) ----------------------------------------------------------------------------
static_assert(POCO_OCCLUSION_RECORD_FLOATS == 77, "occlusion.hip writes 77 floats per record");
static bool aligned_to(const void* p, size_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

extern "C" int poco_op_occlude_batch(const float* d_src, int res, const int* d_pos, int m, int patch, const float* h_fill3,
                                     float* d_out, void* stream) {
  if (!d_src || !d_out || !h_fill3 || res < 4 || res > 4096 || (res & 3) || patch < 1 || patch > res || m < 0 || m > 65536 ||
      (m > 0 && !d_pos) || !aligned_to(d_src, 16) || !aligned_to(d_out, 16)) {
    poco_set_error("poco_op_occlude_batch: bad arguments (need res a multiple of 4 in 4..4096, 1 <= patch <= res, 0 <= m <= 65536, "
                   "16-byte aligned source and output)");
    return POCO_ERR_ARG;
  }
  if (m == 0) return POCO_OK;
  launch_occlude_batch(d_src, d_pos, m, res, patch, h_fill3, d_out, (hipStream_t)stream);
  POCO_HIP_CHECK(hipGetLastError());
  return POCO_OK;
}

extern "C" int poco_op_occlusion_records(const float* d_verts, const float* d_var, const float* d_j3d, int m, int V,
                                         const float* d_base_verts, const float* d_base_var, const float* d_base_j3d,
                                         float* d_records, void* stream) {
  if (!d_verts || !d_var || !d_j3d || !d_base_verts || !d_base_var || !d_base_j3d || !d_records || m < 0 || m > 65536 || V < 2 ||
      V > (1 << 20) || (V & 1) || !aligned_to(d_verts, 8) || !aligned_to(d_base_verts, 8)) {
    poco_set_error("poco_op_occlusion_records: bad arguments (need 0 <= m <= 65536, V even in 2..2^20, 8-byte aligned vertices)");
    return POCO_ERR_ARG;
  }
  if (m == 0) return POCO_OK;
  launch_occlusion_records(d_verts, d_var, d_j3d, m, V, d_base_verts, d_base_var, d_base_j3d, d_records, (hipStream_t)stream);
  POCO_HIP_CHECK(hipGetLastError());
  return POCO_OK;
}

extern "C" int poco_op_heat_overlay(const float* d_field, const int* d_pos, int n, int patch, int res, float scale,
                                    const unsigned char* d_lut, const unsigned char* d_crop, unsigned char* d_out, void* stream) {
  if (!d_field || !d_pos || !d_lut || !d_crop || !d_out || n < 1 || n > 65536 || res < 1 || res > 4096 || patch < 1 || patch > res ||
      !(scale >= 0.f) || std::isinf(scale)) {
    poco_set_error("poco_op_heat_overlay: bad arguments (need 1 <= n <= 65536, 1 <= res <= 4096, 1 <= patch <= res and a finite "
                   "scale > 0, or 0 for the field's maximum)");
    return POCO_ERR_ARG;
  }
  launch_heat_overlay(d_field, d_pos, n, patch, res, scale, d_lut, d_crop, d_out, (hipStream_t)stream);
  POCO_HIP_CHECK(hipGetLastError());
  return POCO_OK;
}

// ---- body-part labels, their crop camera and the segmentation score (part_labels.hip, segm_metrics.hip) ---------------------
static_assert(POCO_SEGM_MAX_C == POCO_SEGM_MAX_CLASSES, "the header's class limit and the kernel's count array must agree");
static_assert(POCO_EST_TRANSLATION_MAX_J == POCO_EST_MAX_JOINTS, "the header's joint limit and the kernel's LDS array must agree");

extern "C" int poco_op_part_labels(const float* d_verts, int B, int V, const float* d_cam_t, const int32_t* d_faces, int F,
                                   const unsigned char* d_face_part, float focal, int res, unsigned long long* d_keys,
                                   unsigned char* d_labels, void* stream) {
  if (!d_verts || !d_cam_t || !d_faces || !d_face_part || !d_keys || !d_labels || B < 1 || B > 65535 || V < 1 || V > (1 << 24) ||
      F < 1 || F > (1 << 24) || res < 1 || res > 4096 || !(focal > 0.f) || std::isinf(focal) || !aligned_to(d_keys, 8)) {
    poco_set_error("poco_op_part_labels: bad arguments (need non-null pointers, 1 <= B <= 65535, 1 <= V, F <= 2^24, 1 <= res <= 4096, "
                   "a finite focal > 0 and 8-byte aligned keys)");
    return POCO_ERR_ARG;
  }
  const hipStream_t s = (hipStream_t)stream;
  POCO_HIP_CHECK(hipMemsetAsync(d_keys, 0xFF, (size_t)B * res * res * sizeof(unsigned long long), s));
  launch_part_labels(d_verts, B, V, d_cam_t, d_faces, F, d_face_part, focal, res, d_keys, d_labels, s);
  POCO_HIP_CHECK(hipGetLastError());
  return POCO_OK;
}

// ---- per-part visibility counts (part_visibility.hip) ----------------------------------------------------------------------
extern "C" size_t poco_op_part_visibility_scratch_bytes(int B, int res, int margin) {
  if (B < 1 || B > 65535 || res < 1 || res > 4096 || margin < 0 || margin > res) return 0;
  const size_t W = (size_t)res + 2 * (size_t)margin;
  return (size_t)B * ((size_t)res * res * sizeof(unsigned long long) + W * W * sizeof(unsigned int));
}

extern "C" int poco_op_part_visibility(const float* d_verts, int B, int V, const float* d_cam_t, const int32_t* d_faces, int F,
                                       const unsigned char* d_face_part, const unsigned char* h_face_part, float focal, int res,
                                       int margin, const unsigned char* d_occ_mask, void* d_scratch, int32_t* d_counts, void* stream) {
  const char* who = "poco_op_part_visibility";
  if (!d_verts || !d_cam_t || !d_faces || !d_face_part || !d_scratch || !d_counts)
    return op_bad(who, "null pointer (only h_face_part and occ_mask may be null)");
  if (B < 1 || B > 65535 || V < 1 || V > (1 << 24) || F < 1 || F > (1 << 24)) return op_bad(who, "needs 1 <= B <= 65535 and 1 <= V, F <= 2^24");
  if (res < 1 || res > 4096) return op_bad(who, "res must be in 1..4096");
  if (margin < 0 || margin > res) return op_bad(who, "margin must be in 0..res");
  if (!(focal > 0.f) || std::isinf(focal)) return op_bad(who, "needs a finite focal > 0");
  if (!aligned_to(d_scratch, 8) || !aligned_to(d_counts, 4)) return op_bad(who, "the scratch must be 8-byte, the counts 4-byte aligned");
  if (h_face_part)
    for (int f = 0; f < F; ++f)
      if (h_face_part[f] > 23) return op_bad(who, "face " + std::to_string(f) + " has part " + std::to_string((int)h_face_part[f]) + " (0..23)");
  const hipStream_t s = (hipStream_t)stream;
  const size_t key_bytes = (size_t)B * res * res * sizeof(unsigned long long);
  const size_t W = (size_t)res + 2 * (size_t)margin;
  unsigned long long* keys = static_cast<unsigned long long*>(d_scratch);
  unsigned int* bits = reinterpret_cast<unsigned int*>(static_cast<unsigned char*>(d_scratch) + key_bytes);
  POCO_HIP_CHECK(hipMemsetAsync(keys, 0xFF, key_bytes, s));
  POCO_HIP_CHECK(hipMemsetAsync(bits, 0, (size_t)B * W * W * sizeof(unsigned int), s));
  POCO_HIP_CHECK(hipMemsetAsync(d_counts, 0, (size_t)B * 24 * 4 * sizeof(int32_t), s));
  launch_part_visibility(d_verts, B, V, d_cam_t, d_faces, F, d_face_part, focal, res, margin, d_occ_mask, keys, bits, d_counts, s);
  POCO_HIP_CHECK(hipGetLastError());
  return POCO_OK;
}

extern "C" int poco_op_estimate_translation(const float* d_joints3d, const float* d_joints2d, int B, int J, float focal, int res,
                                            float* d_cam_t, void* stream) {
  if (!d_joints3d || !d_joints2d || !d_cam_t || B < 1 || J < 1 || J > POCO_EST_TRANSLATION_MAX_J || res < 1 || !(focal > 0.f) ||
      std::isinf(focal)) {
    poco_set_error("poco_op_estimate_translation: bad arguments (need non-null pointers, B >= 1, 1 <= J <= 64, res >= 1 and a finite "
                   "focal > 0)");
    return POCO_ERR_ARG;
  }
  launch_estimate_translation(d_joints3d, d_joints2d, B, J, focal, res, d_cam_t, (hipStream_t)stream);
  POCO_HIP_CHECK(hipGetLastError());
  return POCO_OK;
}

static int segm_shape_check(const char* who, const void* a, const void* b, int B, int C, int h, int w, int H, int W) {
  if (!a || !b || B < 1 || B > 65535 || C < 1 || C > POCO_SEGM_MAX_C || h < 1 || w < 1 || H < 1 || W < 1 || h > 4096 || w > 4096 ||
      H > 4096 || W > 4096) {
    poco_set_error(std::string(who) + ": bad arguments (need non-null pointers, 1 <= B <= 65535, 1 <= C <= 32 and sides in 1..4096)");
    return POCO_ERR_ARG;
  }
  return POCO_OK;
}

extern "C" int poco_op_segm_score_partials(int h, int H) {
  if (h < 1 || H < 1) return 0;
  const int rows = segm_tile_rows(h, H);
  return (H + rows - 1) / rows;
}

extern "C" int poco_op_segm_score(const float* d_logits, int B, int C, int h, int w, const unsigned char* d_labels, int H, int W,
                                  unsigned long long* d_records, double* d_partials, void* stream) {
  if (int rc = segm_shape_check("poco_op_segm_score", d_logits, d_labels, B, C, h, w, H, W)) return rc;
  if (!d_records || !d_partials || !aligned_to(d_records, 8) || !aligned_to(d_partials, 8)) {
    poco_set_error("poco_op_segm_score: records and partials must be non-null and 8-byte aligned");
    return POCO_ERR_ARG;
  }
  if (segm_score_lds_bytes(C, w) > 60000) {
    poco_set_error("poco_op_segm_score: four source rows of every channel must fit the LDS window (C * w <= 3750)");
    return POCO_ERR_ARG;
  }
  const hipStream_t s = (hipStream_t)stream;
  const size_t record_bytes = (size_t)B * POCO_SEGM_RECORD_WORDS(C) * sizeof(unsigned long long);
  POCO_HIP_CHECK(hipMemsetAsync(d_records, 0, record_bytes, s));
  launch_segm_score(d_logits, d_labels, B, C, h, w, H, W, d_records, d_partials, s);
  POCO_HIP_CHECK(hipGetLastError());
  return POCO_OK;
}

extern "C" int poco_op_segm_argmax(const float* d_logits, int B, int C, int h, int w, int H, int W, unsigned char* d_out, void* stream) {
  if (int rc = segm_shape_check("poco_op_segm_argmax", d_logits, d_out, B, C, h, w, H, W)) return rc;
  launch_segm_argmax(d_logits, B, C, h, w, H, W, d_out, (hipStream_t)stream);
  POCO_HIP_CHECK(hipGetLastError());
  return POCO_OK;
}

// ---- video mode's in-fill (track_infill.hip) --------------------------------------------------------------------------------
extern "C" int poco_op_track_infill(const float* d_pose, const float* d_u, const int32_t* d_frames, const int32_t* d_offsets, int P, int N,
                                    const float* d_lin, int L, float thresh, int max_gap, int32_t* d_scratch, float* d_pose_out,
                                    float* d_lin_out, unsigned char* d_flags, unsigned char* d_touched, int32_t* d_rows,
                                    int32_t* d_count, void* stream) {
  const char* who = "poco_op_track_infill";
  if (!d_pose || !d_u || !d_frames || !d_offsets || !d_scratch || !d_pose_out || !d_flags || !d_touched)
    return op_bad(who, "null pointer (pose, u, frames, offsets, scratch, pose_out, flags and touched are needed)");
  if (P < 1 || N < P || (long long)N * 216 >= (1LL << 31))
    return op_bad(who, "needs 1 <= P <= N (no empty track) and fewer than 2^31 floats of pose");
  if (L < 0 || L > POCO_INFILL_MAX_LIN) return op_bad(who, "L must be in 0..16");
  if ((L > 0) != (d_lin != nullptr) || (L > 0) != (d_lin_out != nullptr)) return op_bad(who, "lin and lin_out are needed iff L > 0");
  if (max_gap < 1) return op_bad(who, "max_gap must be >= 1");
  if ((d_rows != nullptr) != (d_count != nullptr)) return op_bad(who, "rows and count come together or not at all");
  if (d_pose_out == d_pose || (L > 0 && d_lin_out == d_lin)) return op_bad(who, "an output may not alias its input");
  launch_track_infill(d_pose, d_u, d_frames, d_offsets, P, N, d_lin, L, thresh, max_gap, d_scratch, d_pose_out, d_lin_out, d_flags,
                      d_touched, d_rows, d_count, (hipStream_t)stream);
  POCO_HIP_CHECK(hipGetLastError());
  return POCO_OK;
}

// ---- choosing between two regressors (select_regressor.hip) ------------------------------------------------------------------
extern "C" int poco_op_select_regressor(const float* d_pose0, const float* d_var0, int kind0, const float* d_pose1, const float* d_var1,
                                        int kind1, int B, int kinematic, double thr, double scale, int mode,
                                        poco_select_payloads_t payloads, float* d_pose_out, float* d_var_out, unsigned char* d_choice,
                                        float* d_score, unsigned char* d_mixed, int32_t* d_rows, int32_t* d_count, int max_blocks,
                                        void* stream) {
  const char* who = "poco_op_select_regressor";
  if (!d_pose0 || !d_var0 || !d_pose1 || !d_var1 || !d_pose_out || !d_var_out || !d_choice || !d_score || !d_mixed)
    return op_bad(who, "null pointer (both models' pose and var, pose_out, var_out, choice, score and mixed are needed)");
  if (B < 1 || B > (1 << 24)) return op_bad(who, "B must be in 1..2^24");
  if ((mode | 1) != 1 || (kind0 | 1) != 1 || (kind1 | 1) != 1 || (kinematic | 1) != 1)
    return op_bad(who, "mode, kind0, kind1 and kinematic must be 0 or 1");
  if (!std::isfinite(scale) || !(scale > 0.0)) return op_bad(who, "scale must be finite and > 0");
  if (payloads.count < 0 || payloads.count > POCO_SELECT_MAX_PAYLOADS) return op_bad(who, "at most 8 payloads");
  if ((d_rows != nullptr) != (d_count != nullptr)) return op_bad(who, "rows and count come together or not at all");
  if (d_pose_out == d_pose0 || d_pose_out == d_pose1 || d_var_out == d_var0 || d_var_out == d_var1)
    return op_bad(who, "an output may not alias an input");
  SelectPayloads pl{};
  pl.count = (int)payloads.count;
  for (int k = 0; k < pl.count; ++k) {
    const poco_select_payload_t& p = payloads.p[k];
    if (!p.src0 || !p.src1 || !p.dst) return op_bad(who, "null pointer in payload " + std::to_string(k));
    if (p.width < 1 || p.width > (1 << 24)) return op_bad(who, "the width of payload " + std::to_string(k) + " must be in 1..2^24");
    if (p.dst == p.src0 || p.dst == p.src1) return op_bad(who, "an output may not alias an input (payload " + std::to_string(k) + ")");
    pl.p[k] = SelectPayload{p.src0, p.src1, p.dst, (int)p.width};
  }
  launch_select_regressor(d_pose0, d_var0, kind0, d_pose1, d_var1, kind1, B, kinematic, thr, scale, mode, pl, d_pose_out, d_var_out,
                          d_choice, d_score, d_mixed, d_rows, d_count, max_blocks, (hipStream_t)stream);
  POCO_HIP_CHECK(hipGetLastError());
  return POCO_OK;
}

// ---- test-time augmentation: fusing K views of a crop (tta_fuse.hip) ------------------------------------------------------------
extern "C" int poco_op_tta_fuse(const float* d_pose, const float* d_var, const float* d_betas, int B, poco_tta_views_t views, int weight,
                                float* d_pose_out, float* d_var_out, float* d_spread, float* d_betas_out, int max_blocks, void* stream) {
  const char* who = "poco_op_tta_fuse";
  if (!d_pose || !d_var || !d_betas || !d_pose_out || !d_var_out || !d_spread || !d_betas_out)
    return op_bad(who, "null pointer (pose, var, betas, pose_out, var_out, spread and betas_out are needed)");
  if (views.count < 2 || views.count > POCO_TTA_MAX_VIEWS) return op_bad(who, "K must be in 2..8");
  if (B < 1 || B > (1 << 24)) return op_bad(who, "B must be in 1..2^24");
  if ((weight | 1) != 1) return op_bad(who, "weight must be 0 (uniform) or 1 (uncertainty)");
  TtaViews tv{};
  tv.count = (int)views.count;
  for (int k = 0; k < tv.count; ++k) {
    const poco_tta_view_t& v = views.v[k];
    if ((v.flip | 1) != 1) return op_bad(who, "the flip of view " + std::to_string(k) + " must be 0 or 1");
    if (!std::isfinite(v.c) || !std::isfinite(v.s) || !(std::fabs(v.c * v.c + v.s * v.s - 1.0) <= 1e-12))
      return op_bad(who, "c and s of view " + std::to_string(k) + " must be the finite cos and sin of one angle (|c^2 + s^2 - 1| <= 1e-12)");
    tv.flip[k] = v.flip; tv.c[k] = v.c; tv.s[k] = v.s;
  }
  if (tv.flip[0] != 0 || tv.c[0] != 1.0 || tv.s[0] != 0.0) return op_bad(who, "view 0 must be the identity (flip 0, c 1, s 0)");
  // [begin, end) in bytes of the three inputs and the four outputs: no output may overlap an input or another output
  const size_t K = (size_t)tv.count, n = (size_t)B;
  const struct { const float* p; size_t floats; } buf[7] = {{d_pose, K * n * 216}, {d_var, K * n * 24}, {d_betas, K * n * 10},
                                                            {d_pose_out, n * 216}, {d_var_out, n * 24}, {d_spread, n * 24}, {d_betas_out, n * 10}};
  for (int o = 3; o < 7; ++o)
    for (int i = 0; i < o; ++i) {
      const uintptr_t a0 = (uintptr_t)buf[o].p, a1 = a0 + 4 * buf[o].floats, b0 = (uintptr_t)buf[i].p, b1 = b0 + 4 * buf[i].floats;
      if (a0 < b1 && b0 < a1) return op_bad(who, "an output may not overlap an input or another output");
    }
  launch_tta_fuse(d_pose, d_var, d_betas, B, tv, weight, d_pose_out, d_var_out, d_spread, d_betas_out, max_blocks, (hipStream_t)stream);
  POCO_HIP_CHECK(hipGetLastError());
  return POCO_OK;
}

// ---- rank-based uncertainty metrics: sort, midranks, cut sums (rank_curve.hip) ---------------------------------------------------
static_assert(POCO_RANK_TILE == RANK_TILE, "include/poco_hip.h and csrc/kernels.h disagree on the sort's tile");
static bool rank_shape_ok(int64_t n, int E) { return n >= 1 && n <= POCO_RANK_MAX_N && E >= 0 && E <= POCO_RANK_MAX_PLANES; }

extern "C" size_t poco_op_rank_curve_scratch_bytes(int64_t n, int E) {
  return rank_shape_ok(n, E) ? rank_scratch_layout(n, E).bytes : 0;
}

extern "C" int poco_op_rank_curve(const float* d_key, const float* d_vals, int64_t n, int E, int K, void* d_scratch, size_t scratch_bytes,
                                  int32_t* d_order, double* d_rank, double* d_cuts, float* d_cut_keys, int max_blocks, void* stream) {
  const char* who = "poco_op_rank_curve";
  if (!rank_shape_ok(n, E)) return op_bad(who, "n must be in 1..2^24 and E in 0..4");
  if (K < 1 || K > POCO_RANK_MAX_CUTS) return op_bad(who, "K must be in 1..1024");
  if (max_blocks < 0) return op_bad(who, "max_blocks must be >= 0");
  if (!d_key || !d_scratch || !d_order || !d_rank || !d_cuts || !d_cut_keys || (E > 0 && !d_vals))
    return op_bad(who, "null pointer (key, scratch, order, rank, cuts and cut_keys are needed, and vals if E > 0)");
  if (!aligned_to(d_scratch, 8) || !aligned_to(d_rank, 8) || !aligned_to(d_cuts, 8) || !aligned_to(d_key, 4) || !aligned_to(d_order, 4) ||
      !aligned_to(d_cut_keys, 4) || (E > 0 && !aligned_to(d_vals, 4)))
    return op_bad(who, "scratch, rank and cuts must be 8-byte aligned, the fp32 and int32 buffers 4-byte aligned");
  const size_t need = rank_scratch_layout(n, E).bytes;
  if (scratch_bytes < need)
    return op_bad(who, "the scratch buffer holds " + std::to_string(scratch_bytes) + " bytes, poco_op_rank_curve_scratch_bytes asks for " +
                           std::to_string(need));
  // [begin, end) in bytes: the two inputs, then the scratch and the four outputs, none of which may overlap anything before it
  const size_t N = (size_t)n, cuts = (size_t)K + 1;
  const struct { const void* p; size_t bytes; } buf[7] = {{d_key, N * 4}, {d_vals, (size_t)E * N * 4}, {d_scratch, need}, {d_order, N * 4},
                                                          {d_rank, N * 8}, {d_cuts, ((size_t)E + 1) * cuts * 8}, {d_cut_keys, cuts * 4}};
  for (int o = 2; o < 7; ++o)
    for (int i = 0; i < o; ++i) {
      if (!buf[i].bytes) continue;
      const uintptr_t a0 = (uintptr_t)buf[o].p, a1 = a0 + buf[o].bytes, b0 = (uintptr_t)buf[i].p, b1 = b0 + buf[i].bytes;
      if (a0 < b1 && b0 < a1) return op_bad(who, "the scratch and the outputs may not overlap an input or each other");
    }
  launch_rank_curve(d_key, d_vals, n, E, K, d_scratch, d_order, d_rank, d_cuts, d_cut_keys, max_blocks, (hipStream_t)stream);
  POCO_HIP_CHECK(hipGetLastError());
  return POCO_OK;
}

extern "C" int poco_op_pearson64(const double* d_x, const double* d_y, int64_t n, double* d_r, int max_blocks, void* stream) {
  const char* who = "poco_op_pearson64";
  if (!d_x || !d_y || !d_r) return op_bad(who, "null pointer (x, y and r are needed)");
  if (n < 1 || n > POCO_RANK_MAX_N) return op_bad(who, "n must be in 1..2^24");
  if (max_blocks < 0) return op_bad(who, "max_blocks must be >= 0");
  if (!aligned_to(d_x, 8) || !aligned_to(d_y, 8) || !aligned_to(d_r, 8)) return op_bad(who, "x, y and r must be 8-byte aligned");
  const uintptr_t r0 = (uintptr_t)d_r, r1 = r0 + 8;
  for (const double* in : {d_x, d_y}) {
    const uintptr_t b0 = (uintptr_t)in, b1 = b0 + (size_t)n * 8;
    if (r0 < b1 && b0 < r1) return op_bad(who, "r may not overlap an input");
  }
  launch_pearson64(d_x, d_y, n, d_r, (hipStream_t)stream);
  POCO_HIP_CHECK(hipGetLastError());
  return POCO_OK;
}

// ---- video mode's uncertainty-weighted smoother (track_smooth.hip) -----------------------------------------------------------
extern "C" int poco_op_track_smooth(const float* d_pose, const float* d_u, const int32_t* d_frames, const int32_t* d_offsets, int P, int N,
                                    const float* d_lin, int L, double lam, double u_ref, int max_gap, double* d_scratch,
                                    float* d_pose_out, float* d_lin_out, float* d_shift, int max_blocks, void* stream) {
  const char* who = "poco_op_track_smooth";
  if (!d_pose || !d_u || !d_frames || !d_offsets || !d_scratch || !d_pose_out || !d_shift)
    return op_bad(who, "null pointer (pose, u, frames, offsets, scratch, pose_out and shift are needed)");
  if (P < 1 || N < P || (long long)N * 216 >= (1LL << 31))
    return op_bad(who, "needs 1 <= P <= N (no empty track) and fewer than 2^31 floats of pose");
  if (L < 0 || L > POCO_SMOOTH_MAX_LIN) return op_bad(who, "L must be in 0..16");
  if ((L > 0) != (d_lin != nullptr) || (L > 0) != (d_lin_out != nullptr)) return op_bad(who, "lin and lin_out are needed iff L > 0");
  if (max_gap < 1) return op_bad(who, "max_gap must be >= 1");
  if (!(lam > 0.0) || !(lam <= 1e4)) return op_bad(who, "lambda must be in (0, 1e4]");
  if (!std::isfinite(u_ref) || !(u_ref > 0.0)) return op_bad(who, "u_ref must be finite and > 0");
  if (d_pose_out == d_pose || (L > 0 && d_lin_out == d_lin)) return op_bad(who, "an output may not alias its input");
  launch_track_smooth(d_pose, d_u, d_frames, d_offsets, P, N, d_lin, L, lam, u_ref, max_gap, d_scratch, d_pose_out, d_lin_out, d_shift,
                      max_blocks, (hipStream_t)stream);
  POCO_HIP_CHECK(hipGetLastError());
  return POCO_OK;
}

// ---- the keypoint refit of demo.py / eval.py --kp_refit (kp_refit.hip) --------------------------------------------------------------
static_assert(POCO_REFIT_MAX_KP == KP_REFIT_MAX_KP && POCO_REFIT_MAX_ITERS == KP_REFIT_MAX_ITERS,
              "include/poco_hip.h and csrc/kernels.h disagree on the keypoint refit");
extern "C" int poco_op_kp_refit(const float* d_pose, const float* d_u, const float* d_jrest, const float* d_kp, const float* d_cam,
                                const float* d_norm, int N, int K, const int32_t* kp_joint, const int32_t* parents, double lam,
                                double u_ref, double rho, double cam_prior, double conf_thresh, int min_kp, int iters, float* d_pose_out,
                                float* d_cam_out, float* d_shift, float* d_cost, int32_t* d_info, int max_blocks, void* stream) {
  const char* who = "poco_op_kp_refit";
  if (!d_pose || !d_u || !d_jrest || !d_kp || !d_cam || !d_norm || !kp_joint || !parents || !d_pose_out || !d_cam_out || !d_shift ||
      !d_cost || !d_info)
    return op_bad(who, "null pointer (every input, both tables and every output are needed)");
  if (N < 1 || (long long)N * 216 >= (1LL << 31)) return op_bad(who, "needs N >= 1 and fewer than 2^31 floats of pose");
  if (K < 1 || K > POCO_REFIT_MAX_KP) return op_bad(who, "K must be in 1..32");
  for (int k = 0; k < K; ++k)
    if (kp_joint[k] < -1 || kp_joint[k] > 23) return op_bad(who, "a kp_joint entry must be in -1..23");
  if (parents[0] >= 0) return op_bad(who, "parents must be a tree rooted at joint 0 (parents[0] < 0)");
  for (int j = 1; j < 24; ++j)
    if (parents[j] < 0 || parents[j] >= j) return op_bad(who, "parents must be a tree rooted at joint 0 with parent < child");
  if (!std::isfinite(lam) || !(lam > 0.0)) return op_bad(who, "lambda must be finite and > 0");
  if (!std::isfinite(u_ref) || !(u_ref > 0.0)) return op_bad(who, "u_ref must be finite and > 0");
  if (!std::isfinite(rho)) return op_bad(who, "rho must be finite (<= 0 turns the robustifier off)");
  if (!std::isfinite(cam_prior) || !(cam_prior > 0.0)) return op_bad(who, "cam_prior must be finite and > 0");
  if (!std::isfinite(conf_thresh)) return op_bad(who, "conf_thresh must be finite");
  if (min_kp < 2) return op_bad(who, "min_kp must be >= 2");
  if (iters < 1 || iters > POCO_REFIT_MAX_ITERS) return op_bad(who, "iters must be in 1..32");
  if (max_blocks < 0) return op_bad(who, "max_blocks must be >= 0");
  // [begin, end) in bytes: six inputs, then five outputs, none of which may overlap anything before it
  const size_t n = (size_t)N;
  const struct { const void* p; size_t bytes; } buf[11] = {
      {d_pose, n * 864}, {d_u, n * 96}, {d_jrest, n * 288}, {d_kp, n * (size_t)K * 12}, {d_cam, n * 20}, {d_norm, n * 4},
      {d_pose_out, n * 864}, {d_cam_out, n * 12}, {d_shift, n * 96}, {d_cost, n * 8}, {d_info, n * 8}};
  for (int o = 6; o < 11; ++o)
    for (int i = 0; i < o; ++i) {
      const uintptr_t a0 = (uintptr_t)buf[o].p, a1 = a0 + buf[o].bytes, b0 = (uintptr_t)buf[i].p, b1 = b0 + buf[i].bytes;
      if (a0 < b1 && b0 < a1) return op_bad(who, "an output may not overlap an input or another output");
    }
  launch_kp_refit(d_pose, d_u, d_jrest, d_kp, d_cam, d_norm, N, K, kp_joint, parents, lam, u_ref, rho, cam_prior, conf_thresh, min_kp,
                  iters, d_pose_out, d_cam_out, d_shift, d_cost, d_info, max_blocks, (hipStream_t)stream);
  POCO_HIP_CHECK(hipGetLastError());
  return POCO_OK;
}

// ---- eval.py --sequences: acceleration and acceleration error per row (track_accel.hip) ----------------------------------------
static_assert(POCO_ACCEL_MAX_JOINTS == TRACK_ACCEL_MAX_JOINTS && POCO_ACCEL_SCRATCH_DOUBLES(1) == TRACK_ACCEL_ROW_DOUBLES,
              "include/poco_hip.h and csrc/kernels.h disagree on the acceleration operator");
extern "C" int poco_op_track_accel(const float* d_pred, const float* d_gt, int stride, int M, const int32_t* d_frames,
                                   const int32_t* d_offsets, int P, int N, double* d_scratch, float* d_accel, float* d_accel_err,
                                   double* d_track_sums, double* d_total, int max_blocks, void* stream) {
  const char* who = "poco_op_track_accel";
  if (!d_pred || !d_frames || !d_offsets || !d_scratch || !d_accel || !d_track_sums || !d_total || (d_gt && !d_accel_err))
    return op_bad(who, "null pointer (pred, frames, offsets, scratch, accel, track_sums and total are needed, and accel_err with gt)");
  if (M < 1 || M > POCO_ACCEL_MAX_JOINTS) return op_bad(who, "M must be in 1..32");
  if (stride < 3 * M || stride > 65536) return op_bad(who, "the row stride must be at least 3 M floats and at most 65536");
  if (P < 1 || N < P || N > (1 << 24)) return op_bad(who, "needs 1 <= P <= N <= 2^24 (no empty track)");
  if (max_blocks < 0) return op_bad(who, "max_blocks must be >= 0");
  launch_track_accel(d_pred, d_gt, stride, M, d_frames, d_offsets, P, N, d_scratch, d_accel, d_accel_err, d_track_sums, d_total,
                     max_blocks, (hipStream_t)stream);
  POCO_HIP_CHECK(hipGetLastError());
  return POCO_OK;
}

// ---- SORT: tracks from per-frame detections, video mode's --tracker sort (sort_tracks.hip) -----------------------------------------
static_assert(POCO_SORT_MAX == SORT_MAX, "include/poco_hip.h and csrc/kernels.h disagree on the tracker");
extern "C" int poco_op_sort_tracks(const double* d_dets, const int32_t* d_frame_offsets, const int32_t* d_clip_offsets, int64_t C,
                                   int64_t F, int64_t N, double iou_thresh, int max_age, int min_hits, int max_trackers,
                                   int32_t* d_tracker, int32_t* d_id, double* d_box, int32_t* d_count, int32_t* d_status, void* stream) {
  const char* who = "poco_op_sort_tracks";
  if (C < 1 || F < 0 || N < 0) return op_bad(who, "needs C >= 1, F >= 0 and N >= 0");
  // the plans are int32: frame and detection indices, and 4 N doubles of boxes addressed from an int
  if (C > (1LL << 24) || F > (1LL << 30) || N > (1LL << 28)) return op_bad(who, "needs C <= 2^24, F <= 2^30 and N <= 2^28 (the int32 plans)");
  if (!d_frame_offsets || !d_clip_offsets || !d_count || !d_status) return op_bad(who, "null pointer (both offset tables, count and status are needed)");
  if (N > 0 && (!d_dets || !d_tracker || !d_id || !d_box)) return op_bad(who, "null pointer (dets, tracker, id and box are needed when N > 0)");
  if (!std::isfinite(iou_thresh) || !(iou_thresh > 0.0) || !(iou_thresh < 1.0)) return op_bad(who, "iou_thresh must be in (0, 1)");
  if (max_age < 0) return op_bad(who, "max_age must be >= 0");
  if (min_hits < 0) return op_bad(who, "min_hits must be >= 0");
  if (max_trackers < 1 || max_trackers > POCO_SORT_MAX) return op_bad(who, "max_trackers must be in 1..64");
  launch_sort_tracks(d_dets, d_frame_offsets, d_clip_offsets, (int)C, (int)F, (int)N, iou_thresh, max_age, min_hits, max_trackers,
                     d_tracker, d_id, d_box, d_count, d_status, (hipStream_t)stream);
  POCO_HIP_CHECK(hipGetLastError());
  return POCO_OK;
}

// ---- video mode's --track_stitch: fragments joined into chains by shape and motion (track_stitch.hip) ---------------------------------
static_assert(POCO_STITCH_MAX_FRAGS == STITCH_MAX_FRAGS && POCO_STITCH_MAX_FIT == STITCH_MAX_FIT && POCO_STITCH_DESC == STITCH_DESC &&
                  POCO_STITCH_SCRATCH_DOUBLES(1) == STITCH_MAX_FRAGS,
              "include/poco_hip.h and csrc/kernels.h disagree on the stitcher");
extern "C" int poco_op_track_stitch(const int32_t* d_clip_offsets, const int32_t* d_frag_offsets, const int32_t* d_frames,
                                    const double* d_boxes, const float* d_betas, const float* d_var, int64_t C, int64_t P, int64_t N,
                                    int max_gap, int fit_len, double u_ref, double motion_tol, double shape_tol, double shape_floor,
                                    double shape_w, double* d_scratch, int32_t* d_succ, int32_t* d_pred, int32_t* d_chain,
                                    double* d_gain, double* d_desc, int32_t* d_status, void* stream) {
  const char* who = "poco_op_track_stitch";
  if (C < 1 || P < 0 || N < 0) return op_bad(who, "needs C >= 1, P >= 0 and N >= 0");
  // the plans are int32: 256 P doubles of scratch and 24 N floats of var addressed from an int
  if (C > (1LL << 24) || P > (1LL << 22) || N > (1LL << 24)) return op_bad(who, "needs C <= 2^24, P <= 2^22 and N <= 2^24 (the int32 plans)");
  if (!d_clip_offsets || !d_frag_offsets || !d_status) return op_bad(who, "null pointer (both offset tables and status are needed)");
  if (N > 0 && (!d_frames || !d_boxes || !d_betas || !d_var)) return op_bad(who, "null pointer (frames, boxes, betas and var are needed when N > 0)");
  if (P > 0 && (!d_scratch || !d_succ || !d_pred || !d_chain || !d_gain || !d_desc))
    return op_bad(who, "null pointer (scratch, succ, pred, chain, gain and desc are needed when P > 0)");
  if (max_gap < 0 || max_gap > (1 << 30)) return op_bad(who, "max_gap must be in 0..2^30");
  if (fit_len < 1 || fit_len > POCO_STITCH_MAX_FIT) return op_bad(who, "fit_len must be in 1..32");
  if (!std::isfinite(u_ref) || !(u_ref > 0.0)) return op_bad(who, "u_ref must be finite and > 0");
  if (!std::isfinite(motion_tol) || !(motion_tol > 0.0)) return op_bad(who, "motion_tol must be finite and > 0");
  if (!std::isfinite(shape_tol) || !(shape_tol > 0.0)) return op_bad(who, "shape_tol must be finite and > 0");
  if (!std::isfinite(shape_floor) || !(shape_floor > 0.0)) return op_bad(who, "shape_floor must be finite and > 0");
  if (!std::isfinite(shape_w) || !(shape_w >= 0.0)) return op_bad(who, "shape_w must be finite and >= 0");
  launch_track_stitch(d_clip_offsets, d_frag_offsets, d_frames, d_boxes, d_betas, d_var, (int)C, (int)P, (int)N, max_gap, fit_len, u_ref,
                      motion_tol, shape_tol, shape_floor, shape_w, d_scratch, d_succ, d_pred, d_chain, d_gain, d_desc, d_status,
                      (hipStream_t)stream);
  POCO_HIP_CHECK(hipGetLastError());
  return POCO_OK;
}

// ---- calibration: isotonic regression over ragged segments, the fitted maps evaluated (isotonic.hip) ---------------------------------
static_assert(POCO_ISO_TILE == ISO_TILE && POCO_ISO_MAX_N == ISO_MAX_N && POCO_ISO_MAX_SEGS == ISO_MAX_SEGS,
              "include/poco_hip.h and csrc/kernels.h disagree on the isotonic fit");
static bool iso_shape_ok(int64_t N, int S) { return N >= 0 && N <= POCO_ISO_MAX_N && S >= 1 && S <= POCO_ISO_MAX_SEGS; }

extern "C" size_t poco_op_isotonic_scratch_bytes(int64_t N, int S) {
  return iso_shape_ok(N, S) ? iso_scratch_layout(N).bytes : 0;
}

extern "C" int poco_op_isotonic(const float* d_key, const float* d_y, int64_t M, const int32_t* d_order, int64_t N,
                                const int32_t* d_seg_offsets, int S, void* d_scratch, size_t scratch_bytes, int32_t* d_block,
                                double* d_fit, int32_t* d_seg_blocks, double* d_knots, int max_blocks, void* stream) {
  const char* who = "poco_op_isotonic";
  if (!iso_shape_ok(N, S)) return op_bad(who, "N must be in 0..2^26 and S in 1..4096");
  if (M < 0 || M > POCO_ISO_MAX_N || (N > 0 && M < 1)) return op_bad(who, "M must be in 0..2^26, and >= 1 when N >= 1");
  if (max_blocks < 0) return op_bad(who, "max_blocks must be >= 0");
  if (!d_seg_offsets || !d_scratch || !d_seg_blocks) return op_bad(who, "null pointer (seg_offsets, scratch and seg_blocks are needed)");
  if (N > 0 && (!d_key || !d_y || !d_order || !d_block || !d_fit || !d_knots))
    return op_bad(who, "null pointer (key, y, order, block, fit and knots are needed when N > 0)");
  if (!aligned_to(d_scratch, 8) || !aligned_to(d_fit, 8) || !aligned_to(d_knots, 8) || !aligned_to(d_key, 4) || !aligned_to(d_y, 4) ||
      !aligned_to(d_order, 4) || !aligned_to(d_seg_offsets, 4) || !aligned_to(d_block, 4) || !aligned_to(d_seg_blocks, 4))
    return op_bad(who, "scratch, fit and knots must be 8-byte aligned, the fp32 and int32 buffers 4-byte aligned");
  const size_t need = iso_scratch_layout(N).bytes;
  if (scratch_bytes < need)
    return op_bad(who, "the scratch buffer holds " + std::to_string(scratch_bytes) + " bytes, poco_op_isotonic_scratch_bytes asks for " +
                           std::to_string(need));
  // [begin, end) in bytes: the four inputs, then the scratch and the four outputs, none of which may overlap anything before it
  const size_t n = (size_t)N, m = (size_t)M, segs = (size_t)S + 1;
  const struct { const void* p; size_t bytes; } buf[9] = {{d_key, m * 4}, {d_y, m * 4}, {d_order, n * 4}, {d_seg_offsets, segs * 4},
                                                          {d_scratch, need}, {d_block, n * 4}, {d_fit, n * 8}, {d_seg_blocks, segs * 4},
                                                          {d_knots, n * 32}};
  for (int o = 4; o < 9; ++o)
    for (int i = 0; i < o; ++i) {
      if (!buf[i].bytes || !buf[o].bytes) continue;
      const uintptr_t a0 = (uintptr_t)buf[o].p, a1 = a0 + buf[o].bytes, b0 = (uintptr_t)buf[i].p, b1 = b0 + buf[i].bytes;
      if (a0 < b1 && b0 < a1) return op_bad(who, "the scratch and the outputs may not overlap an input or each other");
    }
  launch_isotonic(d_key, d_y, (int)M, d_order, (int)N, d_seg_offsets, S, d_scratch, d_block, d_fit, d_seg_blocks, d_knots, max_blocks,
                  (hipStream_t)stream);
  POCO_HIP_CHECK(hipGetLastError());
  return POCO_OK;
}

extern "C" int poco_op_calib_apply(const float* d_x, int64_t R, int S, const int32_t* d_map_ids, const int32_t* d_map_offsets, int P,
                                   const double* d_knots, int64_t B, float* d_out, int max_blocks, void* stream) {
  const char* who = "poco_op_calib_apply";
  if (R < 1 || R > POCO_ISO_MAX_N || S < 1 || S > POCO_ISO_MAX_SEGS || R * S > (1LL << 30))
    return op_bad(who, "R must be in 1..2^26, S in 1..4096 and R * S at most 2^30");
  if (P < 1 || P > POCO_ISO_MAX_SEGS) return op_bad(who, "P must be in 1..4096");
  if (B < 0 || B > POCO_ISO_MAX_N) return op_bad(who, "B must be in 0..2^26");
  if (max_blocks < 0) return op_bad(who, "max_blocks must be >= 0");
  if (!d_x || !d_map_ids || !d_map_offsets || !d_out || (B > 0 && !d_knots))
    return op_bad(who, "null pointer (x, map_ids, map_offsets and out are needed, and knots when B > 0)");
  if (!aligned_to(d_knots, 8) || !aligned_to(d_x, 4) || !aligned_to(d_map_ids, 4) || !aligned_to(d_map_offsets, 4) || !aligned_to(d_out, 4))
    return op_bad(who, "knots must be 8-byte aligned, the fp32 and int32 buffers 4-byte aligned");
  const size_t n = (size_t)R * (size_t)S;
  const struct { const void* p; size_t bytes; } in[4] = {{d_x, n * 4}, {d_map_ids, (size_t)S * 4}, {d_map_offsets, ((size_t)P + 1) * 4},
                                                         {d_knots, (size_t)B * 32}};
  for (int i = 0; i < 4; ++i) {
    if (!in[i].bytes) continue;
    const uintptr_t a0 = (uintptr_t)d_out, a1 = a0 + n * 4, b0 = (uintptr_t)in[i].p, b1 = b0 + in[i].bytes;
    if (a0 < b1 && b0 < a1) return op_bad(who, "out may not overlap an input");
  }
  launch_calib_apply(d_x, R, S, d_map_ids, d_map_offsets, P, d_knots, (int)B, d_out, max_blocks, (hipStream_t)stream);
  POCO_HIP_CHECK(hipGetLastError());
  return POCO_OK;
}

// ---- the cluster bootstrap of eval.py --bootstrap: unit moments and resamples (bootstrap.hip) -----------------------------------------
static_assert(POCO_BOOT_MAX_N == BOOT_MAX_N && POCO_BOOT_MAX_PLANES == BOOT_MAX_PLANES && POCO_BOOT_MAX_PAIRS == BOOT_MAX_PAIRS &&
                  POCO_BOOT_MAX_B == BOOT_MAX_B,
              "include/poco_hip.h and csrc/kernels.h disagree on the bootstrap");
static bool boot_shape_ok(int64_t n, int E, int P, int64_t U) {
  return n >= 1 && n <= POCO_BOOT_MAX_N && E >= 1 && E <= POCO_BOOT_MAX_PLANES && P >= 0 && P <= POCO_BOOT_MAX_PAIRS && U >= 1 && U <= n;
}

extern "C" size_t poco_op_bootstrap_scratch_bytes(int64_t n, int E, int P, int64_t U) {
  return boot_shape_ok(n, E, P, U) ? boot_scratch_layout(n, E).bytes : 0;
}

extern "C" int poco_op_bootstrap(const float* d_planes, int64_t n, int E, const int32_t* pairs, int P, const int32_t* d_unit_offsets,
                                 int64_t U, int64_t B, uint64_t seed, void* d_scratch, size_t scratch_bytes, double* d_center,
                                 double* d_unit_mom, double* d_out, uint32_t* d_draw_counts, int max_blocks, void* stream) {
  const char* who = "poco_op_bootstrap";
  if (!boot_shape_ok(n, E, P, U)) return op_bad(who, "n must be in 1..2^24, E in 1..16, P in 0..16 and U in 1..n");
  if (B < 0 || B > POCO_BOOT_MAX_B) return op_bad(who, "B must be in 0..65536");
  if (max_blocks < 0) return op_bad(who, "max_blocks must be >= 0");
  if (!d_unit_offsets && U != n) return op_bad(who, "without unit_offsets every row is its own unit: U must equal n");
  if (!d_planes || !d_scratch || !d_center || !d_unit_mom || !d_out || (P > 0 && !pairs))
    return op_bad(who, "null pointer (planes, scratch, center, unit_mom and out are needed, and pairs if P > 0)");
  for (int k = 0; k < 2 * P; ++k)
    if (pairs[k] < 0 || pairs[k] >= E) return op_bad(who, "a pair names a plane outside 0..E-1");
  if (!aligned_to(d_scratch, 8) || !aligned_to(d_center, 8) || !aligned_to(d_unit_mom, 8) || !aligned_to(d_out, 8) ||
      !aligned_to(d_planes, 4) || !aligned_to(d_unit_offsets, 4) || !aligned_to(d_draw_counts, 4))
    return op_bad(who, "scratch, center, unit_mom and out must be 8-byte aligned, the fp32, int32 and uint32 buffers 4-byte aligned");
  const size_t need = boot_scratch_layout(n, E).bytes;
  if (scratch_bytes < need)
    return op_bad(who, "the scratch buffer holds " + std::to_string(scratch_bytes) + " bytes, poco_op_bootstrap_scratch_bytes asks for " +
                           std::to_string(need));
  // [begin, end) in bytes: the two inputs, then the scratch and the four outputs, none of which may overlap anything before it
  const size_t N = (size_t)n, Us = (size_t)U, M = (size_t)(1 + E + P);
  const struct { const void* p; size_t bytes; } buf[7] = {{d_planes, (size_t)E * N * 4}, {d_unit_offsets, d_unit_offsets ? (Us + 1) * 4 : 0},
                                                          {d_scratch, need}, {d_center, (size_t)E * 8}, {d_unit_mom, Us * M * 8},
                                                          {d_out, ((size_t)B + 1) * M * 8},
                                                          {d_draw_counts, d_draw_counts ? (size_t)B * Us * 4 : 0}};
  for (int o = 2; o < 7; ++o)
    for (int i = 0; i < o; ++i) {
      if (!buf[i].bytes || !buf[o].bytes) continue;
      const uintptr_t a0 = (uintptr_t)buf[o].p, a1 = a0 + buf[o].bytes, b0 = (uintptr_t)buf[i].p, b1 = b0 + buf[i].bytes;
      if (a0 < b1 && b0 < a1) return op_bad(who, "the scratch and the outputs may not overlap an input or each other");
    }
  launch_bootstrap(d_planes, n, E, pairs, P, d_unit_offsets, U, B, seed, d_scratch, d_center, d_unit_mom, d_out, d_draw_counts, max_blocks,
                   (hipStream_t)stream);
  POCO_HIP_CHECK(hipGetLastError());
  return POCO_OK;
}
