// Baseline JPEG decoder for the demo's input frames: the entropy-coded bytes of a batch of parsed files (poco_amd/jpeg.py
// parse_jpeg) -> one uint8 [H,W,3] RGB picture per file on the device.  The contract (libjpeg's pixels with jpeg_decompress
// defaults: "islow" inverse DCT, "fancy" chroma upsampling, jdcolor.c's fixed point) is stated in include/poco_hip.h and DESIGN.md
// 13; tests/jpegdec_np.py restates it in numpy, pinned on PIL, and the GPU tests compare BYTES.  Integer arithmetic only.
//
// One host-to-device copy (bytes, tables, interval tables from the pinned staging buffer), two memsets, then on the caller's stream:
//   jdec_sync     per 256 subsequences of one image: a lane decodes its JD_SUBSEQ bytes from a guessed state, then round after
//                 round from its predecessor's exit state until a block-wide vote finds no exit state changed (<= 256 rounds)
//   jdec_fix      one thread per workgroup of jdec_sync whose first subsequence continues a restart interval: takes the exit
//                 state of the workgroup before it and re-decodes forward until an exit state is the stored one.  Launched
//                 (workgroups the longest interval spans - 1) times; launch k makes the first k + 1 workgroups of every interval right
//   jdec_scan     per image: prefix sum of the finished-block counts, restarting at every interval -> each subsequence's first block
//   jdec_write    the lanes of jdec_sync decode once more from their final entry states and store coefficients (de-zigzagged int16,
//                 DC as differences) into the zeroed coefficient buffer; damage sets the image's status word
//   jdec_dc       per (interval, component): DC differences -> values, a scan in scan order in tiles of 256
//   jdec_idct     per 32 blocks: dequantise, column pass, LDS, row pass, clamp -> the components' planes
//   jdec_colour   per 256 aligned output dwords: fancy upsampling from the chroma planes in memory, YCbCr -> RGB
// A state is (byte, bit) in the STUFFED stream + block within the MCU + zigzag index.  Every loop is bounded by a constant or by a
// count the host validated; every read of the stream is clamped to its interval, every store is guarded by its own index.  No
// global atomics: every word has one writer, except the status words, to which every writer stores a non-zero value.
#include "block_prims.h"
#include "common.h"
#include "jpeg_dec_internal.h"
#include "../../include/poco_hip.h"

#include <algorithm>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

namespace {

using namespace jdec;

constexpr int JD_SUBSEQ = 128;           // bytes per subsequence (poco_amd/jpeg.py SUBSEQ_BYTES): the one place it is set
constexpr int JD_SEGS_PER_IMAGE = 2048;  // restart intervals planned per image of the batch (a call may spread them unevenly)

struct DSeg {
  unsigned off, len;            // in the image's bytes
  unsigned blk0, nblk;          // first block (in the image) and blocks of the interval
  unsigned sub0, nsub;          // first subsequence (in the image) and subsequences
  unsigned img, pad;
};

__device__ const unsigned char JD_ZZ[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                            41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                            30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

__device__ __forceinline__ u64 pack_state(unsigned bp, int bo, int b, int z) {
  return ((u64)bp << 32) | ((u64)bo << 16) | ((u64)b << 8) | (u64)z;
}

// Decode the symbols that START in bytes [.., stop) of an interval that ends at `end`, from `state`; returns the blocks finished.
// WRITE: coefficients go to coef[blk * 64 + natural index] while blk < blk_end, and the first damaged symbol sets *err and ends the
// lane.  Otherwise damage is decoded by a fixed rule (a window without a code counts as a 16-bit code of symbol 0, a run past 63
// ends the block): states only have to be a function of (position, state) for the rounds to converge.
template <bool WRITE>
__device__ __forceinline__ unsigned decode_span(const unsigned char* __restrict__ d, unsigned end, unsigned stop, u64& state,
                                                const HuffTab* tabs, const unsigned char* comp_of, int bpm, short* coef,
                                                unsigned blk, unsigned blk_end, int* err) {
  unsigned bp = (unsigned)(state >> 32);
  int bo = (int)(state >> 16) & 7, b = (int)(state >> 8) & 7, z = (int)state & 127;
  unsigned nblk = 0;
  if (b >= bpm) b = 0;
  for (int it = 0; it < JD_SUBSEQ * 8 && bp < stop && (!WRITE || blk < blk_end); ++it) {
    // 40 bits from (bp, bo): five data bytes, the 0x00 behind an 0xFF skipped, zeros past the interval
    u64 w = 0;
    unsigned q = bp, ffm = 0;
    #pragma unroll
    for (int k = 0; k < 5; ++k) {
      const unsigned byte = q < end ? d[q] : 0u;
      w = (w << 8) | byte;
      const bool ff = byte == 0xFF;
      ffm |= (unsigned)ff << k;
      q += ff ? 2 : 1;
    }
    const unsigned win = (unsigned)((w << bo) >> 8);
    const HuffTab& t = tabs[comp_of[b] * 2 + (z != 0)];
    const unsigned e = t.look[win >> (32 - JD_LOOKAHEAD)];
    int ln = (int)(e >> 8), sym = (int)(e & 255);
    bool bad = false;
    if (e == 0) {
      ln = 0;
      for (int l = JD_LOOKAHEAD + 1; l <= 16; ++l) {
        const int c = (int)(win >> (32 - l));
        if (c <= t.maxcode[l]) {
          const int i = c + t.delta[l];
          if ((unsigned)i < 256u) { ln = l; sym = t.vals[i]; }
          break;
        }
      }
      if (ln == 0) { bad = true; ln = 16; sym = 0; }
    }
    int s = sym & 15, k = -1;
    const int r = sym >> 4;
    if (z == 0) { s = sym & 15; k = 0; z = 1; }
    else if (s == 0) { z = r == 15 ? z + 16 : 64; }
    else {
      z += r;
      if (z > 63) { bad = true; s = 0; } else { k = z; ++z; }
    }
    int val = 0;
    if (s) {
      const unsigned v = (win >> (32 - ln - s)) & ((1u << s) - 1);
      val = v >= (1u << (s - 1)) ? (int)v : (int)v - (1 << s) + 1;
    }
    if (WRITE) {
      if (bad) { *err = 1; break; }
      if (k >= 0 && k < 64 && (val != 0 || k == 0) && blk < blk_end) coef[(size_t)blk * 64 + JD_ZZ[k]] = (short)val;
    }
    const int n = bo + ln + s, steps = n >> 3;                 // steps <= 4
    bp += steps + __popc(ffm & ((1u << steps) - 1));
    bo = n & 7;
    if (z >= 64) {
      z = 0;
      b = b + 1 == bpm ? 0 : b + 1;
      ++blk;
      ++nblk;
    }
  }
  state = pack_state(bp, bo, b, z);
  return nblk;
}

// The restart interval of subsequence j of an image: the last one whose first subsequence is <= j.
__device__ __forceinline__ int find_seg(const DSeg* __restrict__ segs, int nseg, unsigned j) {
  int lo = 0, hi = nseg - 1;
  for (int it = 0; it < 32 && lo < hi; ++it) {
    const int mid = (lo + hi + 1) >> 1;
    if (segs[mid].sub0 <= j) lo = mid; else hi = mid - 1;
  }
  return lo;
}

__device__ __forceinline__ void load_tables(HuffTab* dst, const DImg* im, int tid) {
  const unsigned* src = reinterpret_cast<const unsigned*>(im->tab);
  unsigned* d = reinterpret_cast<unsigned*>(dst);
  const int n = im->ncomp * 2 * (int)(sizeof(HuffTab) / 4);
  for (int i = tid; i < n; i += JD_THREADS) d[i] = src[i];
}

__global__ __launch_bounds__(JD_THREADS) void jdec_sync(const unsigned char* __restrict__ blob, const DImg* __restrict__ imgs,
                                                        const DSeg* __restrict__ segs_g, u64* __restrict__ entry,
                                                        u64* __restrict__ exits, unsigned* __restrict__ count,
                                                        int* __restrict__ seg_of, u64* __restrict__ wg_exit) {
  __shared__ HuffTab tabs[6];
  __shared__ u64 sx[JD_THREADS];
  __shared__ unsigned char comp_of[8];
  const DImg* im = imgs + blockIdx.y;
  if ((int)blockIdx.x >= im->nwg) return;
  const int tid = threadIdx.x;
  load_tables(tabs, im, tid);
  if (tid < 8) comp_of[tid] = im->comp_of[tid];
  const unsigned j = blockIdx.x * JD_THREADS + tid;
  const bool active = j < (unsigned)im->nsub;
  const unsigned char* d = blob + im->data_off;
  const int bpm = im->bpm;
  unsigned end = 0, stop = 0;
  bool first = true;
  int s = 0;
  u64 st_in = 0;
  if (active) {
    const DSeg* segs = segs_g + im->seg_off;
    s = find_seg(segs, im->nseg, j);
    const DSeg sg = segs[s];
    end = sg.off + sg.len;
    unsigned start = sg.off + (j - sg.sub0) * JD_SUBSEQ;
    start = min(start, end);
    stop = min(start + JD_SUBSEQ, end);
    first = j == sg.sub0;
    if (!first && start < end && d[start - 1] == 0xFF && d[start] == 0) ++start;      // a stuffed 0x00 is no place to start
    st_in = pack_state(start, 0, 0, 0);
  }
  __syncthreads();
  u64 st_out = st_in;
  unsigned n = 0;
  if (active) n = decode_span<false>(d, end, stop, st_out, tabs, comp_of, bpm, nullptr, 0, 0, nullptr);
  sx[tid] = st_out;
  for (int round = 1; round < JD_THREADS; ++round) {
    __syncthreads();
    const u64 pred = (active && !first && tid > 0) ? sx[tid - 1] : st_in;
    __syncthreads();
    int changed = 0;
    if (pred != st_in) {
      st_in = pred;
      u64 x = pred;
      n = decode_span<false>(d, end, stop, x, tabs, comp_of, bpm, nullptr, 0, 0, nullptr);
      changed = x != st_out;
      st_out = x;
      sx[tid] = x;
    }
    if (!__syncthreads_or(changed)) break;
  }
  if (active) {
    const size_t g = (size_t)im->sub_off + j;
    entry[g] = st_in;
    exits[g] = st_out;
    count[g] = n;
    seg_of[g] = s;
    if (tid == JD_THREADS - 1 || j == (unsigned)im->nsub - 1) wg_exit[im->wg_off + blockIdx.x] = st_out;
  }
}

__global__ __launch_bounds__(64) void jdec_fix(const unsigned char* __restrict__ blob, const DImg* __restrict__ imgs,
                                               const DSeg* __restrict__ segs_g, u64* __restrict__ entry, u64* __restrict__ exits,
                                               unsigned* __restrict__ count, const int* __restrict__ seg_of,
                                               const u64* __restrict__ wg_in, u64* __restrict__ wg_out) {
  const DImg* im = imgs + blockIdx.y;
  const int w = blockIdx.x * 64 + threadIdx.x;
  if (w >= im->nwg) return;
  const unsigned j0 = (unsigned)w * JD_THREADS;
  const size_t g0 = (size_t)im->sub_off + j0;
  const int s = seg_of[g0];
  const DSeg sg = segs_g[im->seg_off + s];
  const unsigned nsub = (unsigned)im->nsub;
  if (w > 0 && j0 != sg.sub0) {
    const unsigned char* d = blob + im->data_off;
    const unsigned end = sg.off + sg.len;
    u64 e = wg_in[im->wg_off + w - 1];
    for (unsigned i = 0; i < (unsigned)JD_THREADS && j0 + i < nsub && j0 + i < sg.sub0 + sg.nsub; ++i) {
      if (entry[g0 + i] == e) break;
      entry[g0 + i] = e;
      const unsigned start = min(sg.off + (j0 + i - sg.sub0) * JD_SUBSEQ, end);
      u64 x = e;
      count[g0 + i] = decode_span<false>(d, end, min(start + JD_SUBSEQ, end), x, im->tab, im->comp_of, im->bpm, nullptr, 0, 0, nullptr);
      const bool same = exits[g0 + i] == x;
      exits[g0 + i] = x;
      if (same) break;
      e = x;
    }
  }
  wg_out[im->wg_off + w] = exits[(size_t)im->sub_off + min(j0 + JD_THREADS - 1, nsub - 1)];
}

__global__ __launch_bounds__(JD_THREADS) void jdec_scan(const DImg* __restrict__ imgs, const DSeg* __restrict__ segs_g,
                                                        const unsigned* __restrict__ count, const int* __restrict__ seg_of,
                                                        unsigned* __restrict__ prefix, unsigned* __restrict__ base,
                                                        int* __restrict__ status) {
  __shared__ int wsum[JD_THREADS / 64];
  const DImg* im = imgs + blockIdx.x;
  const int tid = threadIdx.x, nsub = im->nsub;
  const size_t g0 = (size_t)im->sub_off;
  int carry = 0;
  for (int j0 = 0; j0 < nsub; j0 += JD_THREADS) {
    const int j = j0 + tid;
    int tot;
    const int ex = block_exscan<JD_THREADS / 64>(j < nsub ? (int)count[g0 + j] : 0, wsum, &tot);
    if (j < nsub) prefix[g0 + j] = (unsigned)(carry + ex);
    carry += tot;
  }
  __threadfence_block();
  __syncthreads();
  const DSeg* segs = segs_g + im->seg_off;
  for (int j = tid; j < nsub; j += JD_THREADS) {
    const DSeg sg = segs[seg_of[g0 + j]];
    const unsigned in_seg = prefix[g0 + j] - prefix[g0 + sg.sub0];
    base[g0 + j] = sg.blk0 + in_seg;
    if ((unsigned)j == sg.sub0 + sg.nsub - 1 && in_seg + count[g0 + j] < sg.nblk) status[blockIdx.x] = JD_ERR_SHORT;
  }
}

__global__ __launch_bounds__(JD_THREADS) void jdec_write(const unsigned char* __restrict__ blob, const DImg* __restrict__ imgs,
                                                         const DSeg* __restrict__ segs_g, const u64* __restrict__ entry,
                                                         const int* __restrict__ seg_of, const unsigned* __restrict__ base,
                                                         short* __restrict__ coef_g, int* __restrict__ status) {
  __shared__ HuffTab tabs[6];
  __shared__ unsigned char comp_of[8];
  const DImg* im = imgs + blockIdx.y;
  if ((int)blockIdx.x >= im->nwg) return;
  const int tid = threadIdx.x;
  load_tables(tabs, im, tid);
  if (tid < 8) comp_of[tid] = im->comp_of[tid];
  __syncthreads();
  const unsigned j = blockIdx.x * JD_THREADS + tid;
  if (j >= (unsigned)im->nsub) return;
  const size_t g = (size_t)im->sub_off + j;
  const DSeg sg = segs_g[im->seg_off + seg_of[g]];
  const unsigned end = sg.off + sg.len;
  const unsigned start = min(sg.off + (j - sg.sub0) * JD_SUBSEQ, end);
  const unsigned blk_end = min(sg.blk0 + sg.nblk, (unsigned)im->nblocks);
  u64 st = entry[g];
  int err = 0;
  decode_span<true>(blob + im->data_off, end, min(start + JD_SUBSEQ, end), st, tabs, comp_of, im->bpm,
                    coef_g + im->coef_off * 64, base[g], blk_end, &err);
  if (err) status[blockIdx.y] = JD_ERR_CODE;
}

// DC differences -> values: component blockIdx.y of interval blockIdx.x, in scan order, from 0 at the start of the interval.
__global__ __launch_bounds__(JD_THREADS) void jdec_dc(const DImg* __restrict__ imgs, const DSeg* __restrict__ segs_g,
                                                      short* __restrict__ coef_g) {
  __shared__ int wsum[JD_THREADS / 64];
  const DSeg sg = segs_g[blockIdx.x];
  const DImg* im = imgs + sg.img;
  const int c = blockIdx.y;
  if (c >= im->ncomp) return;
  const int bpm = im->bpm, nb = c == 0 ? im->hs * im->vs : 1, koff = c == 0 ? 0 : im->hs * im->vs + c - 1;
  const unsigned blk_end = min(sg.blk0 + sg.nblk, (unsigned)im->nblocks);
  const int total = (int)(sg.nblk / (unsigned)bpm) * nb;
  short* coef = coef_g + im->coef_off * 64;
  int carry = 0;
  for (int t0 = 0; t0 < total; t0 += JD_THREADS) {
    const int t = t0 + threadIdx.x;
    const unsigned blk = sg.blk0 + (unsigned)(t / nb) * bpm + koff + t % nb;
    const bool ok = t < total && blk < blk_end;
    const int v = ok ? (int)coef[(size_t)blk * 64] : 0;
    int tot;
    const int ex = block_exscan<JD_THREADS / 64>(v, wsum, &tot);
    if (ok) coef[(size_t)blk * 64] = (short)(carry + ex + v);
    carry += tot;
  }
}

// ---- inverse DCT ----------------------------------------------------------------------------------------------------------------
constexpr int ID_BLOCKS = JD_THREADS / 8;    // blocks per workgroup: 8 threads each (one per column, then one per row)
// int32 per block in LDS: 64 + 8.  In the column pass a group of 32 lanes is 4 blocks x 8 columns storing one dword each; a stride
// of 72 dwords (8 mod 32) puts the 4 blocks on banks 0-7, 8-15, 16-23, 24-31 instead of all on 0-7 (the 4-way conflict of 64).
constexpr int ID_STRIDE = 72;

constexpr int fix13(double x) { return (int)(x * (1 << 13) + 0.5); }

// One pass of libjpeg's jidctint.c jpeg_idct_islow (CONST_BITS 13, PASS1_BITS 2) over 8 values, descaled by N bits.
template <int N>
__device__ __forceinline__ void idct8(int* d) {
  constexpr int R = 1 << (N - 1);
  int z1 = (d[2] + d[6]) * fix13(0.541196100);
  const int t2 = z1 - d[6] * fix13(1.847759065), t3 = z1 + d[2] * fix13(0.765366865);
  const int t0 = (d[0] + d[4]) * (1 << 13), t1 = (d[0] - d[4]) * (1 << 13);
  const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
  int o0 = d[7], o1 = d[5], o2 = d[3], o3 = d[1];
  z1 = o0 + o3;
  int z2 = o1 + o2, z3 = o0 + o2, z4 = o1 + o3;
  const int z5 = (z3 + z4) * fix13(1.175875602);
  o0 *= fix13(0.298631336); o1 *= fix13(2.053119869); o2 *= fix13(3.072711026); o3 *= fix13(1.501321110);
  z1 *= -fix13(0.899976223); z2 *= -fix13(2.562915447);
  z3 = z3 * -fix13(1.961570560) + z5; z4 = z4 * -fix13(0.390180644) + z5;
  o0 += z1 + z3; o1 += z2 + z4; o2 += z2 + z3; o3 += z1 + z4;
  d[0] = (t10 + o3 + R) >> N; d[7] = (t10 - o3 + R) >> N;
  d[1] = (t11 + o2 + R) >> N; d[6] = (t11 - o2 + R) >> N;
  d[2] = (t12 + o1 + R) >> N; d[5] = (t12 - o1 + R) >> N;
  d[3] = (t13 + o0 + R) >> N; d[4] = (t13 - o0 + R) >> N;
}

__global__ __launch_bounds__(JD_THREADS) void jdec_idct(const DImg* __restrict__ imgs, const short* __restrict__ coef_g,
                                                        unsigned char* __restrict__ planes) {
  __shared__ int ws[ID_BLOCKS * ID_STRIDE];
  __shared__ unsigned short q[3 * 64];
  const DImg* im = imgs + blockIdx.y;
  if ((long long)blockIdx.x * ID_BLOCKS >= im->nblocks) return;
  const int tid = threadIdx.x;
  if (tid < 3 * 64) q[tid] = im->qt[tid >> 6][tid & 63];
  __syncthreads();
  const int lb = tid >> 3, i = tid & 7;
  const int blk = blockIdx.x * ID_BLOCKS + lb;
  const bool active = blk < im->nblocks;
  const int k = active ? blk % im->bpm : 0, mcu = active ? blk / im->bpm : 0;
  const int c = im->comp_of[k];
  int d[8];
  if (active) {
    const short* src = coef_g + (im->coef_off + (u64)blk) * 64 + i;
    #pragma unroll
    for (int r = 0; r < 8; ++r) d[r] = (int)src[r * 8] * (int)q[c * 64 + r * 8 + i];
    idct8<11>(d);
    #pragma unroll
    for (int r = 0; r < 8; ++r) ws[lb * ID_STRIDE + r * 8 + i] = d[r];
  }
  __syncthreads();
  if (!active) return;
  #pragma unroll
  for (int x = 0; x < 8; ++x) d[x] = ws[lb * ID_STRIDE + i * 8 + x];
  idct8<18>(d);
  unsigned lo = 0, hi = 0;
  #pragma unroll
  for (int x = 0; x < 4; ++x) {
    lo |= (unsigned)min(max(d[x] + 128, 0), 255) << (8 * x);
    hi |= (unsigned)min(max(d[x + 4] + 128, 0), 255) << (8 * x);
  }
  const int mx = mcu % im->mcux, my = mcu / im->mcux;
  const int bx = c == 0 ? mx * im->hs + k % im->hs : mx, by = c == 0 ? my * im->vs + k / im->hs : my;
  // planes are whole blocks wide and 8-byte aligned: (by * 8 + i, bx * 8 .. + 7) lies inside by construction of pw and nblocks
  unsigned char* dst = planes + im->plane_off[c] + (size_t)(by * 8 + i) * im->pw[c] + bx * 8;
  *reinterpret_cast<uint2*>(dst) = make_uint2(lo, hi);
}

// ---- upsampling and colour ------------------------------------------------------------------------------------------------------
constexpr int fix16(double x) { return (int)(x * 65536.0 + 0.5); }

// jdsample.c: the chroma sample of pixel (y, x) from the component's own cw x ch samples in its plane.
__device__ __forceinline__ int chroma_at(const unsigned char* __restrict__ p, int pw, int cw, int ch, int hs, int vs, int fancy,
                                         int y, int x) {
  if (hs == 1) return p[(size_t)y * pw + x];
  const int i = x >> 1;
  if (!fancy) return p[(size_t)(vs == 2 ? y >> 1 : y) * pw + i];
  if (vs == 1) {                                         // h2v1_fancy_upsample: 3/4 1/4, + 1 on even and + 2 on odd columns
    const unsigned char* row = p + (size_t)y * pw;
    const int v = row[i];
    if (x & 1) return i == cw - 1 ? v : (3 * v + row[i + 1] + 2) >> 2;
    return i == 0 ? v : (3 * v + row[i - 1] + 1) >> 2;
  }
  const int j = y >> 1;                                  // h2v2_fancy_upsample: 9 3 3 1 / 16, + 8 on even and + 7 on odd columns
  const int jf = (y & 1) ? min(j + 1, ch - 1) : max(j - 1, 0);
  const unsigned char* nr = p + (size_t)j * pw;
  const unsigned char* fr = p + (size_t)jf * pw;
  const int s = 3 * nr[i] + fr[i];
  if (x & 1) return i == cw - 1 ? (4 * s + 7) >> 4 : (3 * s + 3 * nr[i + 1] + fr[i + 1] + 7) >> 4;
  return i == 0 ? (4 * s + 8) >> 4 : (3 * s + 3 * nr[i - 1] + fr[i - 1] + 8) >> 4;
}

__global__ __launch_bounds__(JD_THREADS) void jdec_colour(const DImg* __restrict__ imgs, const unsigned char* __restrict__ planes) {
  const DImg* im = imgs + blockIdx.y;
  const int H = im->H, W = im->W;
  const long long total = 3ll * H * W;
  unsigned char* out = im->out;
  const int mis = (int)((uintptr_t)out & 3);
  // thread t owns the aligned dword t of the span that covers out[0, total): bytes f0 .. f0 + 3 of the picture
  const long long t = (long long)blockIdx.x * JD_THREADS + threadIdx.x;
  const long long f0 = t * 4 - mis;
  if (f0 >= total) return;
  const unsigned char* py = planes + im->plane_off[0];
  const unsigned char* pcb = planes + im->plane_off[1];
  const unsigned char* pcr = planes + im->plane_off[2];
  unsigned word = 0;
  long long last = -1;
  int cr_ = 0, cg_ = 0, cb_ = 0;
  #pragma unroll
  for (int b = 0; b < 4; ++b) {
    const long long f = f0 + b;
    if (f < 0 || f >= total) continue;
    const long long px = f / 3;
    if (px != last) {
      last = px;
      const int y = (int)(px / W), x = (int)(px - (long long)y * W);
      const int Y = py[(size_t)y * im->pw[0] + x];
      if (im->ncomp == 1) {
        cr_ = cg_ = cb_ = Y;
      } else {
        const int cb = chroma_at(pcb, im->pw[1], im->cw, im->ch, im->hs, im->vs, im->fancy, y, x) - 128;
        const int cr = chroma_at(pcr, im->pw[2], im->cw, im->ch, im->hs, im->vs, im->fancy, y, x) - 128;
        cr_ = min(max(Y + ((fix16(1.40200) * cr + 32768) >> 16), 0), 255);                 // jdcolor.c, SCALEBITS 16
        cg_ = min(max(Y + ((-fix16(0.34414) * cb + 32768 - fix16(0.71414) * cr) >> 16), 0), 255);
        cb_ = min(max(Y + ((fix16(1.77200) * cb + 32768) >> 16), 0), 255);
      }
    }
    const int chn = (int)(f - px * 3);
    word |= (unsigned)(chn == 0 ? cr_ : chn == 1 ? cg_ : cb_) << (8 * b);
  }
  if (f0 >= 0 && f0 + 4 <= total) {
    *reinterpret_cast<unsigned*>(out + f0) = word;                    // out + f0 = the aligned address
  } else {
    #pragma unroll
    for (int b = 0; b < 4; ++b)
      if (f0 + b >= 0 && f0 + b < total) out[f0 + b] = (unsigned char)(word >> (8 * b));
  }
}

// ---- host ------------------------------------------------------------------------------------------------------------------------
size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

}  // namespace

namespace jdec {

bool build_table(const unsigned char* bits, const unsigned char* vals, bool dc, HuffTab* t) {
  std::memset(t, 0, sizeof(HuffTab));
  int code = 0, k = 0;
  for (int ln = 1; ln <= 16; ++ln) {
    t->delta[ln] = k - code;
    const int nb = bits[ln - 1];
    if (k + nb > (dc ? 16 : 256)) return false;           // vals[] holds 16 (DC) or 256 (AC) symbols
    if (nb && code + nb >= (1 << ln)) return false;       // no prefix code, or the all-ones code word is used: checked before
    for (int i = 0; i < nb; ++i) {                        // the codes index look[], so that code << (LOOKAHEAD - ln) stays inside it
      if (dc && vals[k] > 15) return false;
      t->vals[k] = vals[k];
      if (ln <= JD_LOOKAHEAD) {
        const int lo = code << (JD_LOOKAHEAD - ln);
        for (int j = lo; j < lo + (1 << (JD_LOOKAHEAD - ln)); ++j) t->look[j] = (unsigned short)(ln << 8 | vals[k]);
      }
      ++code;
      ++k;
    }
    t->maxcode[ln] = nb ? code - 1 : -1;
    code <<= 1;
  }
  t->maxcode[0] = -1;
  t->maxcode[17] = 1 << 20;
  return k > 0;
}

size_t max_blocks(int H, int W) {
  const size_t b8h = (H + 7) / 8, b8w = (W + 7) / 8, b16h = (H + 15) / 16, b16w = (W + 15) / 16;
  return std::max({3 * b8h * b8w, 4 * b8h * b16w, 6 * b16h * b16w});
}

void launch_idct_colour(const DImg* d_img, int n, const short* coef, unsigned char* planes, int max_idct, long long max_dwords,
                        hipStream_t s) {
  jdec_idct<<<dim3(max_idct, n), JD_THREADS, 0, s>>>(d_img, coef, planes);
  jdec_colour<<<dim3((unsigned)((max_dwords + JD_THREADS - 1) / JD_THREADS), n), JD_THREADS, 0, s>>>(d_img, planes);
}

}  // namespace jdec

struct poco_jpeg_decoder {
  int max_h = 0, max_w = 0, max_batch = 0;
  size_t max_bytes = 0, blob_cap = 0, max_subs = 0, max_segs = 0, max_wgs = 0, blocks_per_image = 0;
  unsigned char* h_blob = nullptr;         // pinned staging
  unsigned char* d_blob = nullptr;
  short* coef = nullptr;                   // [blocks][64] natural order
  unsigned char* planes = nullptr;         // 64 bytes per block
  u64 *entry = nullptr, *exits = nullptr, *wg_exit = nullptr;      // per subsequence; [2][max_wgs]
  unsigned *count = nullptr, *prefix = nullptr, *base = nullptr;
  int* seg_of = nullptr;
  hipEvent_t copied = nullptr;
  bool in_flight = false;
  ~poco_jpeg_decoder() {
    if (h_blob) (void)hipHostFree(h_blob);
    for (void* p : {(void*)d_blob, (void*)coef, (void*)planes, (void*)entry, (void*)exits, (void*)wg_exit, (void*)count, (void*)prefix,
                    (void*)base, (void*)seg_of})
      if (p) (void)hipFree(p);
    if (copied) (void)hipEventDestroy(copied);
  }
};

extern "C" int poco_jpeg_decoder_create(int max_h, int max_w, int max_batch, size_t max_bytes, poco_jpeg_decoder_t* out) {
  if (!out) { poco_set_error("poco_jpeg_decoder_create: null handle pointer"); return POCO_ERR_ARG; }
  *out = nullptr;
  if (max_h < 1 || max_w < 1 || max_h > JD_MAX_SIDE || max_w > JD_MAX_SIDE || max_batch < 1 || max_batch > JD_MAX_BATCH ||
      max_bytes < 1 || max_bytes > ((size_t)1 << 30)) {
    poco_set_error("poco_jpeg_decoder_create: bad arguments (need 1 <= max_h, max_w <= 16384, 1 <= max_batch <= 4096, "
                   "1 <= max_bytes <= 2^30)");
    return POCO_ERR_ARG;
  }
  auto d = std::make_unique<poco_jpeg_decoder>();
  d->max_h = max_h;
  d->max_w = max_w;
  d->max_batch = max_batch;
  d->max_bytes = max_bytes;
  d->max_segs = (size_t)max_batch * JD_SEGS_PER_IMAGE;
  d->max_subs = max_bytes / JD_SUBSEQ + d->max_segs + max_batch;
  d->max_wgs = d->max_subs / JD_THREADS + max_batch;
  d->blocks_per_image = max_blocks(max_h, max_w);
  d->blob_cap = (size_t)max_batch * sizeof(DImg) + d->max_segs * sizeof(DSeg) + max_bytes + (size_t)max_batch * 16 + 16;
  const size_t blocks = d->blocks_per_image * max_batch;
  POCO_HIP_CHECK(hipHostMalloc((void**)&d->h_blob, d->blob_cap, hipHostMallocDefault));
  POCO_HIP_CHECK(hipMalloc(&d->d_blob, d->blob_cap));
  POCO_HIP_CHECK(hipMalloc(&d->coef, blocks * 64 * sizeof(short)));
  POCO_HIP_CHECK(hipMalloc(&d->planes, blocks * 64));
  POCO_HIP_CHECK(hipMalloc(&d->entry, d->max_subs * sizeof(u64)));
  POCO_HIP_CHECK(hipMalloc(&d->exits, d->max_subs * sizeof(u64)));
  POCO_HIP_CHECK(hipMalloc(&d->wg_exit, 2 * d->max_wgs * sizeof(u64)));
  POCO_HIP_CHECK(hipMalloc(&d->count, d->max_subs * sizeof(unsigned)));
  POCO_HIP_CHECK(hipMalloc(&d->prefix, d->max_subs * sizeof(unsigned)));
  POCO_HIP_CHECK(hipMalloc(&d->base, d->max_subs * sizeof(unsigned)));
  POCO_HIP_CHECK(hipMalloc(&d->seg_of, d->max_subs * sizeof(int)));
  POCO_HIP_CHECK(hipEventCreateWithFlags(&d->copied, hipEventDisableTiming));
  *out = d.release();
  return POCO_OK;
}

extern "C" int poco_jpeg_decode(poco_jpeg_decoder_t dec, const poco_jpeg_image* imgs, int n, int* d_status, void* stream) {
  if (!dec || !imgs || !d_status) { poco_set_error("poco_jpeg_decode: null handle or pointer"); return POCO_ERR_ARG; }
  if (n < 1 || n > dec->max_batch) {
    poco_set_error("poco_jpeg_decode: " + std::to_string(n) + " images, the decoder was created for 1 .. " + std::to_string(dec->max_batch));
    return POCO_ERR_ARG;
  }
  // ---- validate and lay out, before the staging buffer or the GPU is touched
  size_t nsegs = 0, nsubs = 0, nwgs = 0, nbytes = 0, nblocks = 0, plane_bytes = 0;
  int max_wg = 0, max_idct = 0, fix_rounds = 0;
  long long max_dwords = 0;
  std::vector<DImg> dim(n);
  std::vector<DSeg> dseg;
  for (int i = 0; i < n; ++i) {
    const poco_jpeg_image& im = imgs[i];
    const std::string who = "poco_jpeg_decode: image " + std::to_string(i) + ": ";
    if (!im.data || !im.segs || !im.d_rgb) { poco_set_error(who + "null pointer"); return POCO_ERR_ARG; }
    if (im.H < 1 || im.W < 1 || im.H > dec->max_h || im.W > dec->max_w) {
      poco_set_error(who + std::to_string(im.H) + " x " + std::to_string(im.W) + " outside 1 x 1 .. " + std::to_string(dec->max_h) +
                     " x " + std::to_string(dec->max_w) + " (the size the decoder was created for)");
      return POCO_ERR_ARG;
    }
    const bool samp_ok = im.ncomp == 1 ? (im.hsamp == 1 && im.vsamp == 1)
                                       : im.ncomp == 3 && ((im.hsamp == 1 && im.vsamp == 1) || (im.hsamp == 2 && (im.vsamp == 1 || im.vsamp == 2)));
    if (!samp_ok) { poco_set_error(who + "components / sampling must be 1 (1x1) or 3 with luma 1x1, 2x1 or 2x2"); return POCO_ERR_ARG; }
    if (im.nseg < 1 || im.nbytes > ((size_t)1 << 30)) { poco_set_error(who + "no restart interval, or more than 2^30 bytes"); return POCO_ERR_ARG; }
    DImg& d = dim[i];
    std::memset(&d, 0, sizeof(DImg));
    d.H = im.H; d.W = im.W; d.ncomp = im.ncomp; d.hs = im.hsamp; d.vs = im.vsamp;
    d.bpm = im.ncomp == 1 ? 1 : im.hsamp * im.vsamp + 2;
    d.mcux = (im.W + 8 * im.hsamp - 1) / (8 * im.hsamp);
    d.mcuy = (im.H + 8 * im.vsamp - 1) / (8 * im.vsamp);
    const long long nmcu = (long long)d.mcux * d.mcuy;
    d.nblocks = (int)(nmcu * d.bpm);
    d.cw = (im.W + im.hsamp - 1) / im.hsamp;
    d.ch = (im.H + im.vsamp - 1) / im.vsamp;
    d.fancy = im.hsamp == 2 && d.cw > 2;
    for (int k = 0; k < d.bpm; ++k) d.comp_of[k] = (unsigned char)(im.ncomp == 1 ? 0 : (k < im.hsamp * im.vsamp ? 0 : k - im.hsamp * im.vsamp + 1));
    d.out = im.d_rgb;
    d.coef_off = nblocks;
    for (int c = 0; c < im.ncomp; ++c) {
      const int h = c == 0 ? im.hsamp : 1, v = c == 0 ? im.vsamp : 1;
      d.pw[c] = d.mcux * h * 8;
      d.plane_off[c] = plane_bytes;
      plane_bytes += (size_t)d.pw[c] * d.mcuy * v * 8;
      std::memcpy(d.qt[c], im.qt[c], sizeof(d.qt[c]));
      if (!build_table(im.dc_bits[c], im.dc_vals[c], true, &d.tab[2 * c]) || !build_table(im.ac_bits[c], im.ac_vals[c], false, &d.tab[2 * c + 1])) {
        poco_set_error(who + "a Huffman table is no prefix code (or a DC category is above 15)");
        return POCO_ERR_ARG;
      }
    }
    if ((size_t)d.nblocks > dec->blocks_per_image) { poco_set_error(who + "more blocks than planned"); return POCO_ERR_STATE; }
    nblocks += d.nblocks;
    d.data_off = (unsigned)nbytes;          // relative to the bytes region, made absolute below
    d.nbytes = (unsigned)im.nbytes;
    nbytes += align_up(im.nbytes, 16);
    d.nseg = im.nseg;
    d.seg_off = (int)nsegs;
    d.sub_off = (int)nsubs;
    d.wg_off = (int)nwgs;
    unsigned sub = 0;
    for (int s = 0; s < im.nseg; ++s) {
      const unsigned off = im.segs[3 * s], len = im.segs[3 * s + 1], mcu0 = im.segs[3 * s + 2];
      const long long mcu1 = s + 1 < im.nseg ? (long long)im.segs[3 * s + 5] : nmcu;
      if ((size_t)off + len > im.nbytes || (s == 0 && mcu0 != 0) || mcu1 <= (long long)mcu0 || mcu1 > nmcu) {
        poco_set_error(who + "restart interval " + std::to_string(s) + " lies outside the data or the picture");
        return POCO_ERR_ARG;
      }
      DSeg g{};
      g.off = off; g.len = len;
      g.blk0 = mcu0 * d.bpm;
      g.nblk = (unsigned)((mcu1 - mcu0) * d.bpm);
      g.sub0 = sub;
      g.nsub = std::max(1u, (len + JD_SUBSEQ - 1) / JD_SUBSEQ);
      g.img = (unsigned)i;
      fix_rounds = std::max(fix_rounds, (int)((g.sub0 + g.nsub - 1) / JD_THREADS - g.sub0 / JD_THREADS));
      sub += g.nsub;
      dseg.push_back(g);
    }
    d.nsub = (int)sub;
    d.nwg = (int)((sub + JD_THREADS - 1) / JD_THREADS);
    nsegs += im.nseg;
    nsubs += sub;
    nwgs += d.nwg;
    max_wg = std::max(max_wg, d.nwg);
    max_idct = std::max(max_idct, (d.nblocks + ID_BLOCKS - 1) / ID_BLOCKS);
    max_dwords = std::max(max_dwords, (3ll * im.H * im.W + 3 + 3) / 4);
  }
  const size_t img_bytes = (size_t)n * sizeof(DImg), seg_bytes = nsegs * sizeof(DSeg);
  const size_t used = img_bytes + seg_bytes + nbytes + 16;
  if (nbytes > dec->max_bytes + (size_t)n * 16 || nsegs > dec->max_segs || nsubs > dec->max_subs || nwgs > dec->max_wgs || used > dec->blob_cap) {
    poco_set_error("poco_jpeg_decode: " + std::to_string(nbytes) + " bytes in " + std::to_string(nsegs) + " restart intervals exceed "
                   "what the decoder was created for (max_bytes " + std::to_string(dec->max_bytes) + ", " + std::to_string(dec->max_segs) +
                   " intervals)");
    return POCO_ERR_ARG;
  }
  const hipStream_t s = (hipStream_t)stream;
  // the staging buffer is free once the previous call's copy has left it
  if (dec->in_flight) POCO_HIP_CHECK(hipEventSynchronize(dec->copied));
  for (int i = 0; i < n; ++i) {
    dim[i].data_off += (unsigned)(img_bytes + seg_bytes);
    std::memcpy(dec->h_blob + dim[i].data_off, imgs[i].data, imgs[i].nbytes);
    std::memset(dec->h_blob + dim[i].data_off + imgs[i].nbytes, 0, align_up(imgs[i].nbytes, 16) - imgs[i].nbytes);
  }
  std::memcpy(dec->h_blob, dim.data(), img_bytes);
  std::memcpy(dec->h_blob + img_bytes, dseg.data(), seg_bytes);
  std::memset(dec->h_blob + used - 16, 0, 16);
  POCO_HIP_CHECK(hipMemcpyAsync(dec->d_blob, dec->h_blob, used, hipMemcpyHostToDevice, s));
  POCO_HIP_CHECK(hipEventRecord(dec->copied, s));
  dec->in_flight = true;
  POCO_HIP_CHECK(hipMemsetAsync(d_status, 0, (size_t)n * sizeof(int), s));
  POCO_HIP_CHECK(hipMemsetAsync(dec->coef, 0, nblocks * 64 * sizeof(short), s));
  const DImg* d_img = reinterpret_cast<const DImg*>(dec->d_blob);
  const DSeg* d_seg = reinterpret_cast<const DSeg*>(dec->d_blob + img_bytes);
  u64* wg0 = dec->wg_exit;
  u64* wg1 = dec->wg_exit + dec->max_wgs;
  jdec_sync<<<dim3(max_wg, n), JD_THREADS, 0, s>>>(dec->d_blob, d_img, d_seg, dec->entry, dec->exits, dec->count, dec->seg_of, wg0);
  for (int k = 0; k < fix_rounds; ++k) {
    jdec_fix<<<dim3((max_wg + 63) / 64, n), 64, 0, s>>>(dec->d_blob, d_img, d_seg, dec->entry, dec->exits, dec->count, dec->seg_of,
                                                        k & 1 ? wg1 : wg0, k & 1 ? wg0 : wg1);
  }
  jdec_scan<<<n, JD_THREADS, 0, s>>>(d_img, d_seg, dec->count, dec->seg_of, dec->prefix, dec->base, d_status);
  jdec_write<<<dim3(max_wg, n), JD_THREADS, 0, s>>>(dec->d_blob, d_img, d_seg, dec->entry, dec->seg_of, dec->base, dec->coef, d_status);
  jdec_dc<<<dim3((unsigned)nsegs, 3), JD_THREADS, 0, s>>>(d_img, d_seg, dec->coef);
  launch_idct_colour(d_img, n, dec->coef, dec->planes, max_idct, max_dwords, s);
  POCO_HIP_CHECK(hipGetLastError());
  return POCO_OK;
}

extern "C" void poco_jpeg_decoder_destroy(poco_jpeg_decoder_t dec) { delete dec; }
