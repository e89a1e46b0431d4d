// Pseudo-ground-truth export on the device: the model's outputs of every confident crop as one record of the reference's dataset
// .npz (pocolib/dataset/base_dataset.py:54-147 reads it; the writer was stripped from the released reference, whose
// pocolib/core/tester.py:163 still declares its accumulators).  Per crop: pose[72] = rotation_matrix_to_angle_axis
// (pocolib/utils/geometry.py:264-429) of the 24 predicted matrices, var[24] = the trailing mean of var_pose WITHOUT the kinematic
// accumulation (the reader applies it on load), openpose / part / S from the 49 joints (tester.py:232-233), center and scale
// (tester.py:194-196), selected as get_confident_frames (pocolib/utils/train_utils.py:31-45) selects.  The contract and the record
// layout are stated in include/poco_hip.h and DESIGN.md section 20; tests/pseudo_np.py restates the step in numpy.
//
// Two launches per step, both on the caller's stream, nothing read back:
//   pseudo_select  ONE block of 256 threads walks the step's crops in chunks of 256: a lane's flag is its crop's selection, the
//                  wave's ranks come from one ballot, the four wave totals go through LDS, the running base is carried in a
//                  register from chunk to chunk.  Writes dest[b] = record index of crop b (or -1) and, last, the new count.
//   pseudo_write   grid B, one wave: a block whose crop was dropped returns; the others write their record, lanes 0..23 one
//                  joint's axis-angle each (fp64 inside, like poco_op_rodrigues), all lanes the keypoints.
// No atomics: a record index is a prefix sum in source order, every record word has one writer, two runs give the same bits.
#include "common.h"
#include "kernels.h"
#include "../../include/poco_hip.h"

#include <cmath>
#include <string>

namespace {

constexpr int PS_REC = POCO_PSEUDO_RECORD_FLOATS;      // 384
// record offsets (include/poco_hip.h)
constexpr int P_SRC = 0, P_CENTER = 1, P_SCALE = 3, P_POSE = 4, P_SHAPE = 76, P_VAR = 86, P_OPENPOSE = 110, P_PART = 185, P_S = 257,
              P_PAD = 353;
static_assert(P_PAD <= PS_REC, "record layout");
constexpr int PS_MAX_T = POCO_PSEUDO_MAX_TRAILING;     // 128: one block of numpy's pairwise sum

// get_smpl_skeleton() of pocolib/utils/kp_utils.py:881-908 as parent per joint
__constant__ int PS_SMPL_PARENT[24] = {-1, 0, 0, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 9, 9, 12, 13, 14, 16, 17, 18, 19, 20, 21};

// rotation_matrix_to_angle_axis (geometry.py:264-293) of one row-major 3x3: rotation_matrix_to_quaternion (:349-429) on the
// transposed matrix with its four masked candidates - the three comparisons on the float32 inputs, eps = float32(1e-6), the masks
// multiplied in and added in the reference's order, so that a NaN or an Inf reaches every component as it does there - then
// quaternion_to_angle_axis (:296-346) with its atan2 pair and k = 2 at sin^2 = 0, then aa[isnan] = 0.  fp64 inside, no contraction
// (the numpy restatement has none either).
__device__ __forceinline__ void rotmat_to_aa_f64(const float* __restrict__ Rf, float* __restrict__ aa) {
  #pragma clang fp contract(off)
  const float f00 = Rf[0], f11 = Rf[4], f22 = Rf[8];
  const bool d2 = f22 < 1e-6f, d0_d1 = f00 > f11, d0_nd1 = f00 < -f11;
  const double m0 = (d2 && d0_d1) ? 1.0 : 0.0, m1 = (d2 && !d0_d1) ? 1.0 : 0.0, m2 = (!d2 && d0_nd1) ? 1.0 : 0.0,
               m3 = (!d2 && !d0_nd1) ? 1.0 : 0.0;
  const double R00 = Rf[0], R01 = Rf[1], R02 = Rf[2], R10 = Rf[3], R11 = Rf[4], R12 = Rf[5], R20 = Rf[6], R21 = Rf[7], R22 = Rf[8];
  // rmat_t[i][j] = R[j][i]
  const double t0 = 1.0 + R00 - R11 - R22, t1 = 1.0 - R00 + R11 - R22, t2 = 1.0 - R00 - R11 + R22, t3 = 1.0 + R00 + R11 + R22;
  const double a0[4] = {R21 - R12, t0, R10 + R01, R02 + R20};
  const double a1[4] = {R02 - R20, R10 + R01, t1, R21 + R12};
  const double a2[4] = {R10 - R01, R02 + R20, R21 + R12, t2};
  const double a3[4] = {t3, R21 - R12, R02 - R20, R10 - R01};
  const double den = sqrt(t0 * m0 + t1 * m1 + t2 * m2 + t3 * m3);
  double q[4];
  #pragma unroll
  for (int k = 0; k < 4; ++k) q[k] = ((a0[k] * m0 + a1[k] * m1 + a2[k] * m2 + a3[k] * m3) / den) * 0.5;
  const double s2 = q[1] * q[1] + q[2] * q[2] + q[3] * q[3];
  const double s = sqrt(s2), c = q[0];
  const double two_theta = 2.0 * (c < 0.0 ? atan2(-s, -c) : atan2(s, c));
  const double k = s2 > 0.0 ? two_theta / s : 2.0;
  #pragma unroll
  for (int i = 0; i < 3; ++i) {
    const double v = q[1 + i] * k;
    aa[i] = v != v ? 0.f : (float)v;
  }
}

__global__ __launch_bounds__(256) void rotmat_to_aa_kernel(const float* __restrict__ rot, float* __restrict__ aa, int N) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= N) return;
  rotmat_to_aa_f64(rot + (size_t)i * 9, aa + (size_t)i * 3);
}

// var_pose[b, j, 0..T).mean() as numpy's float32 add.reduce over a contiguous axis gives it (what postproc.prepare_uncert calls):
// below 8 elements a running sum, from 8 to 128 eight strided partial sums combined as a tree, then the remainder.  T = 1 is the
// value itself.
__device__ __forceinline__ float trailing_mean(const float* __restrict__ v, int T) {
  #pragma clang fp contract(off)
  if (T == 1) return v[0];
  float res;
  if (T < 8) {
    res = 0.f;
    for (int i = 0; i < T; ++i) res += v[i];
  } else {
    float r[8];
    #pragma unroll
    for (int k = 0; k < 8; ++k) r[k] = v[k];
    int i = 8;
    for (; i < T - (T % 8); i += 8)
      #pragma unroll
      for (int k = 0; k < 8; ++k) r[k] += v[i + k];
    res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
    for (; i < T; ++i) res += v[i];
  }
  return res / (float)T;
}

// get_confident_frames (train_utils.py:31-45) of one crop: the kinematic accumulation of poco_utils.py:21-25 in child order, then
// column 0 < threshold.  A NaN compares false: dropped.  keep_all: no threshold.
__device__ __forceinline__ bool crop_selected(const float* __restrict__ var_pose, int T, float threshold, int keep_all) {
  if (keep_all) return true;
  float v[24];
  for (int j = 0; j < 24; ++j) v[j] = trailing_mean(var_pose + (size_t)j * T, T);
  for (int j = 1; j < 24; ++j) v[j] += v[PS_SMPL_PARENT[j]];
  return v[0] < threshold;
}

// One block.  count[0] = records kept so far; dest[b] = record index of crop b of this step, -1 = dropped.
__global__ __launch_bounds__(256) void pseudo_select(int B, const float* __restrict__ var_pose, int T, float threshold, int keep_all,
                                                     int* __restrict__ count, int* __restrict__ dest) {
  __shared__ int wtot[4];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  int base = count[0];                       // read by every thread before the first barrier; written after the last one
  for (int c0 = 0; c0 < B; c0 += 256) {
    const int b = c0 + tid;
    const bool keep = b < B && crop_selected(var_pose + (size_t)b * 24 * T, T, threshold, keep_all);
    const unsigned long long mask = __ballot(keep);
    const int before = __popcll(mask & ((1ull << lane) - 1ull));
    if (lane == 0) wtot[wv] = __popcll(mask);
    __syncthreads();
    int off = 0, total = 0;
    #pragma unroll
    for (int w = 0; w < 4; ++w) {
      if (w < wv) off += wtot[w];
      total += wtot[w];
    }
    if (b < B) dest[b] = keep ? base + off + before : -1;
    base += total;
    __syncthreads();                         // wtot is rewritten by the next chunk
  }
  if (tid == 0) count[0] = base;
}

struct PseudoDev {
  const float *pose, *shape, *var, *j2d, *j3d, *boxes;
  const int* src;
  const int* dest;
  float* rec;
  int T, in_crop;
  float crop_res;
};

__global__ __launch_bounds__(64) void pseudo_write(PseudoDev d) {
  #pragma clang fp contract(off)
  const int b = blockIdx.x, t = threadIdx.x;
  const int slot = d.dest[b];
  if (slot < 0) return;                      // the whole block
  float* rec = d.rec + (size_t)slot * PS_REC;
  const float cx = d.boxes[b * 4], cy = d.boxes[b * 4 + 1], w = d.boxes[b * 4 + 2], h = d.boxes[b * 4 + 3];
  if (t < 24) {
    rotmat_to_aa_f64(d.pose + ((size_t)b * 24 + t) * 9, rec + P_POSE + 3 * t);
    rec[P_VAR + t] = trailing_mean(d.var + ((size_t)b * 24 + t) * d.T, d.T);
  }
  if (t < 10) rec[P_SHAPE + t] = d.shape[(size_t)b * 10 + t];
  if (t == 0) {
    rec[P_SRC] = __int_as_float(d.src[b]);
    rec[P_CENTER] = cx;
    rec[P_CENTER + 1] = cy;
    rec[P_SCALE] = ((w >= h || w != w) ? w : h) / 200.0f;          // np.maximum(w, h) / 200 (tester.py:196)
  }
  if (t < 49) {
    float x = d.j2d[((size_t)b * 49 + t) * 2], y = d.j2d[((size_t)b * 49 + t) * 2 + 1];
    if (d.in_crop) {                         // postproc.convert_crop_coords_to_orig_img, its float32 operations in its order
      const float half = 0.5f * d.crop_res, sc = w / d.crop_res, ox = cx - w / 2.0f, oy = cy - w / 2.0f;
      x = ox + (half * (x + 1.0f)) * sc;
      y = oy + (half * (y + 1.0f)) * sc;
    }
    float* kp = t < 25 ? rec + P_OPENPOSE + 3 * t : rec + P_PART + 3 * (t - 25);
    kp[0] = x; kp[1] = y; kp[2] = 1.0f;
    if (t >= 25) {
      float* S = rec + P_S + 4 * (t - 25);
      const float* j = d.j3d + ((size_t)b * 49 + t) * 3;
      S[0] = j[0]; S[1] = j[1]; S[2] = j[2]; S[3] = 1.0f;
    }
  }
  if (P_PAD + t < PS_REC) rec[P_PAD + t] = 0.f;
}

}  // namespace

extern "C" int poco_op_rotmat_to_aa(const float* d_rotmat, float* d_aa, int N, void* stream) {
  if (!d_rotmat || !d_aa || N < 1) { poco_set_error("rotmat_to_aa: bad argument (need both pointers and N >= 1)"); return POCO_ERR_ARG; }
  rotmat_to_aa_kernel<<<(N + 255) / 256, 256, 0, (hipStream_t)stream>>>(d_rotmat, d_aa, N);
  POCO_HIP_CHECK(hipGetLastError());
  return POCO_OK;
}

// ---- pseudo-labeler -------------------------------------------------------------------------------------------------------
struct poco_pseudo {
  long long capacity = 0, offered = 0;
  float threshold = 0.f, crop_res = 224.f;
  int keep_all = 1, in_crop = 0;
  bool on_device = false;
  float* d_rec = nullptr;
  int *d_dest = nullptr, *d_count = nullptr;
  ~poco_pseudo() {
    for (void* p : {(void*)d_rec, (void*)d_dest, (void*)d_count})
      if (p) (void)hipFree(p);
  }
};

static constexpr long long PSEUDO_MAX_CAPACITY = 1ll << 24;
static_assert(PS_REC - P_PAD <= 64, "pseudo_write zeroes the padding with one wave");

extern "C" int poco_pseudo_create(int64_t capacity, float threshold, int joints_in_crop, int crop_res, poco_pseudo_t* out) {
  if (!out) { poco_set_error("poco_pseudo_create: null handle pointer"); return POCO_ERR_ARG; }
  *out = nullptr;
  if (capacity < 1 || capacity > PSEUDO_MAX_CAPACITY || (joints_in_crop != 0 && joints_in_crop != 1) || crop_res < 1 ||
      crop_res > 16384 || std::isinf(threshold)) {
    poco_set_error("poco_pseudo_create: bad arguments (need 1 <= capacity <= 2^24, joints_in_crop 0 or 1, 1 <= crop_res <= 16384 "
                   "and a finite threshold, or NaN / <= 0 for none)");
    return POCO_ERR_ARG;
  }
  auto* p = new poco_pseudo;
  p->capacity = capacity;
  p->keep_all = (threshold != threshold || threshold <= 0.f) ? 1 : 0;
  p->threshold = p->keep_all ? 0.f : threshold;
  p->in_crop = joints_in_crop;
  p->crop_res = (float)crop_res;
  *out = p;
  return POCO_OK;
}

// The first step: records (filled with POCO_PSEUDO_UNWRITTEN), the step's destination scratch and the count, in stream order.
static int pseudo_upload(poco_pseudo* p, hipStream_t s) {
  if (p->on_device) return POCO_OK;
  const size_t bytes = (size_t)p->capacity * PS_REC * sizeof(float);
  POCO_HIP_CHECK(hipMalloc(&p->d_rec, bytes));
  POCO_HIP_CHECK(hipMalloc(&p->d_dest, (size_t)p->capacity * sizeof(int)));
  POCO_HIP_CHECK(hipMalloc(&p->d_count, 2 * sizeof(int)));
  POCO_HIP_CHECK(hipMemsetAsync(p->d_rec, 0xFF, bytes, s));
  POCO_HIP_CHECK(hipMemsetAsync(p->d_count, 0, 2 * sizeof(int), s));
  p->on_device = true;
  return POCO_OK;
}

extern "C" int poco_pseudo_step(poco_pseudo_t p, int B, const float* d_pred_pose, const float* d_pred_shape, const float* d_var_pose,
                                int var_t, const float* d_joints2d, const float* d_joints3d, const float* d_boxes,
                                const int32_t* d_source_id, void* stream) {
  if (!p || B < 1 || !d_pred_pose || !d_pred_shape || !d_var_pose || !d_joints2d || !d_joints3d || !d_boxes || !d_source_id ||
      var_t < 1 || var_t > PS_MAX_T) {
    poco_set_error("poco_pseudo_step: bad arguments (need a handle, B >= 1, pred_pose, pred_shape, var_pose with 1..128 trailing "
                   "elements, joints2d, joints3d, boxes and source_id)");
    return POCO_ERR_ARG;
  }
  if (p->offered + B > p->capacity) {
    poco_set_error("poco_pseudo_step: " + std::to_string(p->offered) + " + " + std::to_string(B) + " crops exceed the capacity of " +
                   std::to_string(p->capacity));
    return POCO_ERR_ARG;
  }
  const hipStream_t s = (hipStream_t)stream;
  if (int rc = pseudo_upload(p, s)) return rc;
  pseudo_select<<<1, 256, 0, s>>>(B, d_var_pose, var_t, p->threshold, p->keep_all, p->d_count, p->d_dest);
  const PseudoDev d{d_pred_pose, d_pred_shape, d_var_pose, d_joints2d, d_joints3d, d_boxes, d_source_id, p->d_dest, p->d_rec,
                    var_t, p->in_crop, p->crop_res};
  pseudo_write<<<B, 64, 0, s>>>(d);
  POCO_HIP_CHECK(hipGetLastError());
  p->offered += B;
  return POCO_OK;
}

extern "C" int poco_pseudo_finish(poco_pseudo_t p, float* h_records, int64_t records_cap, int64_t* n_kept, int64_t* n_offered,
                                  void* stream) {
  if (!p || !n_kept || !n_offered || (h_records && records_cap < p->offered)) {
    poco_set_error("poco_pseudo_finish: bad arguments (need a handle, both counts and, if records are wanted, room for every offered "
                   "crop: the kept count is not known on the host)");
    return POCO_ERR_ARG;
  }
  *n_offered = p->offered;
  *n_kept = 0;
  if (!p->on_device) return POCO_OK;         // nothing stepped yet: nothing kept, no GPU work
  const hipStream_t s = (hipStream_t)stream;
  int kept = 0;
  POCO_HIP_CHECK(hipMemcpyAsync(&kept, p->d_count, sizeof(int), hipMemcpyDeviceToHost, s));
  if (h_records && p->offered > 0)
    POCO_HIP_CHECK(hipMemcpyAsync(h_records, p->d_rec, (size_t)p->offered * PS_REC * sizeof(float), hipMemcpyDeviceToHost, s));
  POCO_HIP_CHECK(hipStreamSynchronize(s));
  *n_kept = kept;
  return POCO_OK;
}

extern "C" int poco_pseudo_reset(poco_pseudo_t p, void* stream) {
  if (!p) { poco_set_error("poco_pseudo_reset: null handle"); return POCO_ERR_ARG; }
  if (p->on_device) {
    const hipStream_t s = (hipStream_t)stream;
    if (p->offered > 0) POCO_HIP_CHECK(hipMemsetAsync(p->d_rec, 0xFF, (size_t)p->offered * PS_REC * sizeof(float), s));
    POCO_HIP_CHECK(hipMemsetAsync(p->d_count, 0, 2 * sizeof(int), s));
  }
  p->offered = 0;
  return POCO_OK;
}

extern "C" void poco_pseudo_destroy(poco_pseudo_t p) { delete p; }
