// Baseline JPEG encoder for the demo's rendered frames: uint8 [H,W,3] RGB on the device -> the bytes of a JFIF file on the device.
// The contract (libjpeg's integer colour conversion, h2v2 downsampling, "islow" DCT and quantisation, Annex K Huffman tables,
// one restart interval per MCU row) is stated in include/poco_hip.h and DESIGN.md "JPEG"; tests/jpeg_np.py restates it in numpy
// and the GPU tests compare BYTES.  Integer arithmetic only.
//
// Three launches per call, all on the caller's stream, into scratch planned at create:
//   jpeg_transform  per tile of 16 MCUs (256 x 16 pixels): RGB staged through LDS, YCbCr + 2x2 chroma box, both DCT passes through
//                   LDS (one thread per 8-point row, then per column), quantisation, zigzag -> int16 coefficients, MCU-interleaved
//   jpeg_entropy    per restart interval (MCU row): lanes take blocks; bit lengths, prefix sum, bits merged in LDS, byte stuffing
//                   behind a second prefix sum -> the interval's slot (sized for the worst case) and its length
//   jpeg_compact    per interval: prefix sum of the lengths (+ 2 marker bytes each), copy behind the header, RSTm / EOI, total length
// The restart interval is what makes the bit stream parallel: DC prediction and bit alignment restart at every MCU row, so rows
// are coded independently and concatenated.  No global atomics: every output word has one writer.
#include "block_prims.h"
#include "common.h"
#include "../../include/poco_hip.h"

#include <algorithm>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

namespace {

constexpr int JPEG_MAX_SIDE = 16384;
constexpr int JPEG_BLOCK_BITS = 64 * 27;                 // per 8x8 block before stuffing: at most a 16-bit code + 11 value bits per coefficient
constexpr int JPEG_BLOCK_BYTES = 2 * JPEG_BLOCK_BITS / 8;  // after stuffing (every byte 0xFF): 432
constexpr int JPEG_HEADER_BYTES = 629;

// ---- tables (ITU-T T.81 Annex K) ------------------------------------------------------------------------------------------------
const unsigned char ZIGZAG[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                  41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                  30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
const unsigned char QUANT[2][64] = {
    {16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
     18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99},
    {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99,
     99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99}};
const unsigned char DC_BITS[2][16] = {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0}, {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0}};
const unsigned char DC_VALS[12] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11};
const unsigned char AC_BITS[2][16] = {{0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7D}, {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77}};
const unsigned char AC_VALS[2][162] = {
    {0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xA1,
     0x08, 0x23, 0x42, 0xB1, 0xC1, 0x15, 0x52, 0xD1, 0xF0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0A, 0x16, 0x17, 0x18, 0x19, 0x1A, 0x25, 0x26,
     0x27, 0x28, 0x29, 0x2A, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3A, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4A, 0x53, 0x54, 0x55, 0x56,
     0x57, 0x58, 0x59, 0x5A, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6A, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7A, 0x83, 0x84, 0x85,
     0x86, 0x87, 0x88, 0x89, 0x8A, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9A, 0xA2, 0xA3, 0xA4, 0xA5, 0xA6, 0xA7, 0xA8, 0xA9, 0xAA,
     0xB2, 0xB3, 0xB4, 0xB5, 0xB6, 0xB7, 0xB8, 0xB9, 0xBA, 0xC2, 0xC3, 0xC4, 0xC5, 0xC6, 0xC7, 0xC8, 0xC9, 0xCA, 0xD2, 0xD3, 0xD4, 0xD5, 0xD6,
     0xD7, 0xD8, 0xD9, 0xDA, 0xE1, 0xE2, 0xE3, 0xE4, 0xE5, 0xE6, 0xE7, 0xE8, 0xE9, 0xEA, 0xF1, 0xF2, 0xF3, 0xF4, 0xF5, 0xF6, 0xF7, 0xF8, 0xF9,
     0xFA},
    {0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42,
     0x91, 0xA1, 0xB1, 0xC1, 0x09, 0x23, 0x33, 0x52, 0xF0, 0x15, 0x62, 0x72, 0xD1, 0x0A, 0x16, 0x24, 0x34, 0xE1, 0x25, 0xF1, 0x17, 0x18, 0x19,
     0x1A, 0x26, 0x27, 0x28, 0x29, 0x2A, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3A, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4A, 0x53, 0x54, 0x55,
     0x56, 0x57, 0x58, 0x59, 0x5A, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6A, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7A, 0x82, 0x83,
     0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8A, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9A, 0xA2, 0xA3, 0xA4, 0xA5, 0xA6, 0xA7, 0xA8,
     0xA9, 0xAA, 0xB2, 0xB3, 0xB4, 0xB5, 0xB6, 0xB7, 0xB8, 0xB9, 0xBA, 0xC2, 0xC3, 0xC4, 0xC5, 0xC6, 0xC7, 0xC8, 0xC9, 0xCA, 0xD2, 0xD3, 0xD4,
     0xD5, 0xD6, 0xD7, 0xD8, 0xD9, 0xDA, 0xE2, 0xE3, 0xE4, 0xE5, 0xE6, 0xE7, 0xE8, 0xE9, 0xEA, 0xF2, 0xF3, 0xF4, 0xF5, 0xF6, 0xF7, 0xF8, 0xF9,
     0xFA}};

// Device tables, built once at create.
constexpr int HUFF_AC = 0, HUFF_DC = 512, HUFF_WORDS = 512 + 24;   // entry = length << 16 | code; AC [2][256] by (run << 4 | size), DC [2][12]
struct JpegTables {
  unsigned short qtab[100][2][64];     // [quality - 1][luma | chroma][zigzag position]: the divisors, which are also the DQT payloads
  unsigned huff[HUFF_WORDS];
  unsigned char izz[64];               // natural index -> zigzag position
  unsigned char header[JPEG_HEADER_BYTES + 3];   // the stream's header with zero tables, size and restart interval (patched per call)
};
// where the per-call values go in the header
struct HeaderPatch {
  int dqt[2], size, dri;
};

// ---- step 1: transform ----------------------------------------------------------------------------------------------------------
constexpr int TR_THREADS = 256;
constexpr int TR_MCUS = 16;                    // MCUs per tile: 256 x 16 pixels, 96 blocks = 768 eight-point rows, three per thread
constexpr int TR_BLOCKS = TR_MCUS * 6;
constexpr int TR_ROW_DWORDS = 194;             // 768 bytes of a tile row + up to 3 bytes in front of it, in whole dwords
constexpr int TR_RAW_STRIDE = TR_ROW_DWORDS * 4;
// int16 per block in LDS: 64 + 8, i.e. 36 dwords.  In the column pass the 8 lanes of a block share 4 banks and the 4 blocks of a
// 32-lane group then sit 4 banks apart (36 mod 32) instead of on the same 4 (the 4-way conflict of a stride of 32 dwords).
constexpr int TR_BLK_STRIDE = 72;

constexpr int fix(double x, int bits) { return (int)(x * (1 << bits) + 0.5); }

// One pass of libjpeg's jfdctint.c (CONST_BITS 13, PASS1_BITS 2) over 8 values; FIRST = the row pass.
template <bool FIRST>
__device__ __forceinline__ void dct8(int* d) {
  constexpr int N = FIRST ? 13 - 2 : 13 + 2;
  constexpr int R = 1 << (N - 1);
  const int t0 = d[0] + d[7], t7 = d[0] - d[7], t1 = d[1] + d[6], t6 = d[1] - d[6];
  const int t2 = d[2] + d[5], t5 = d[2] - d[5], t3 = d[3] + d[4], t4 = d[3] - d[4];
  const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
  d[0] = FIRST ? (t10 + t11) * 4 : (t10 + t11 + 2) >> 2;
  d[4] = FIRST ? (t10 - t11) * 4 : (t10 - t11 + 2) >> 2;
  const int e = (t12 + t13) * fix(0.541196100, 13);
  d[2] = (e + t13 * fix(0.765366865, 13) + R) >> N;
  d[6] = (e - t12 * fix(1.847759065, 13) + R) >> N;
  const int z1 = -(t4 + t7) * fix(0.899976223, 13), z2 = -(t5 + t6) * fix(2.562915447, 13);
  const int z5 = (t4 + t6 + t5 + t7) * fix(1.175875602, 13);
  const int z3 = -(t4 + t6) * fix(1.961570560, 13) + z5, z4 = -(t5 + t7) * fix(0.390180644, 13) + z5;
  d[7] = (t4 * fix(0.298631336, 13) + z1 + z3 + R) >> N;
  d[5] = (t5 * fix(2.053119869, 13) + z2 + z4 + R) >> N;
  d[3] = (t6 * fix(3.072711026, 13) + z2 + z3 + R) >> N;
  d[1] = (t7 * fix(1.501321110, 13) + z1 + z4 + R) >> N;
}

__global__ __launch_bounds__(TR_THREADS) void jpeg_transform(const unsigned char* __restrict__ rgb, int H, int W, int mcux,
                                                             const unsigned short* __restrict__ qtab,
                                                             const unsigned char* __restrict__ izz_g, short* __restrict__ coef) {
  __shared__ __attribute__((aligned(16))) unsigned char raw[16 * TR_RAW_STRIDE];
  __shared__ __attribute__((aligned(16))) short ws[TR_BLOCKS * TR_BLK_STRIDE];
  __shared__ unsigned short q[128];
  __shared__ unsigned char izz[64];
  const int tid = threadIdx.x;
  const int m0 = blockIdx.x * TR_MCUS, my = blockIdx.y;
  const int x0 = m0 * 16, y0 = my * 16;
  const int nblk = min(TR_MCUS, mcux - m0) * 6;
  const int ncol = min(TR_MCUS * 16, W - x0);          // pixel columns of the tile inside the image (>= 1)
  if (tid < 128) q[tid] = qtab[tid];
  if (tid < 64) izz[tid] = izz_g[tid];
  // The tile's 16 rows of RGB, read once, as the aligned dwords that cover each row segment (rows below the image repeat the last
  // one).  A dword that reaches outside the frame - only the first and the last of the buffer can - is assembled from its bytes.
  const unsigned char* const end = rgb + (size_t)H * W * 3;
  for (int i = tid; i < 16 * TR_ROW_DWORDS; i += TR_THREADS) {
    const int r = i / TR_ROW_DWORDS, j = i - r * TR_ROW_DWORDS;
    const unsigned char* src = rgb + ((size_t)min(y0 + r, H - 1) * W + x0) * 3;
    const int mis = (int)((uintptr_t)src & 3);
    if (j * 4 >= mis + ncol * 3) continue;
    const unsigned char* p = src - mis + j * 4;
    unsigned v = 0;
    if (p >= rgb && p + 4 <= end) {
      v = *reinterpret_cast<const unsigned*>(p);
    } else {
      for (int b = 0; b < 4; ++b)
        if (p + b >= rgb && p + b < end) v |= (unsigned)p[b] << (8 * b);
    }
    *reinterpret_cast<unsigned*>(raw + r * TR_RAW_STRIDE + j * 4) = v;
  }
  __syncthreads();
  // Colour conversion (jccolor.c, SCALEBITS 16) and the 2x2 chroma box with its alternating bias (jcsample.c): a thread takes a
  // 2x2 quad; columns right of the image repeat the last one.  Level-shifted samples go to the block layout.
  #pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int qi = tid + TR_THREADS * k;
    const int qy = qi >> 7, qx = qi & 127;
    if ((qx >> 3) * 6 >= nblk) continue;
    int cb = 0, cr = 0;
    #pragma unroll
    for (int dy = 0; dy < 2; ++dy) {
      const int y = 2 * qy + dy;
      const int mis = (int)(((uintptr_t)rgb + ((size_t)min(y0 + y, H - 1) * W + x0) * 3) & 3);
      #pragma unroll
      for (int dx = 0; dx < 2; ++dx) {
        const int x = 2 * qx + dx;
        const unsigned char* px = raw + y * TR_RAW_STRIDE + mis + min(x, ncol - 1) * 3;
        const int R = px[0], G = px[1], B = px[2];
        const int Y = (fix(0.29900, 16) * R + fix(0.58700, 16) * G + fix(0.11400, 16) * B + 32768) >> 16;
        cb += (-fix(0.16874, 16) * R - fix(0.33126, 16) * G + fix(0.50000, 16) * B + (128 << 16) + 32767) >> 16;
        cr += (fix(0.50000, 16) * R - fix(0.41869, 16) * G - fix(0.08131, 16) * B + (128 << 16) + 32767) >> 16;
        ws[((x >> 4) * 6 + (y >> 3) * 2 + ((x >> 3) & 1)) * TR_BLK_STRIDE + (y & 7) * 8 + (x & 7)] = (short)(Y - 128);
      }
    }
    const int bias = 1 + (qx & 1);
    short* c = ws + ((qx >> 3) * 6 + 4) * TR_BLK_STRIDE + qy * 8 + (qx & 7);
    c[0] = (short)(((cb + bias) >> 2) - 128);
    c[TR_BLK_STRIDE] = (short)(((cr + bias) >> 2) - 128);
  }
  __syncthreads();
  // Row pass: one thread per (block, row), 16 contiguous bytes in and out.
  #pragma unroll
  for (int k = 0; k < 3; ++k) {
    const int it = tid + TR_THREADS * k, b = it >> 3, r = it & 7;
    if (b >= nblk) continue;
    short* p = ws + b * TR_BLK_STRIDE + r * 8;
    int d[8];
    #pragma unroll
    for (int i = 0; i < 8; ++i) d[i] = p[i];
    dct8<true>(d);
    #pragma unroll
    for (int i = 0; i < 8; ++i) p[i] = (short)d[i];
  }
  __syncthreads();
  // Column pass: one thread per (block, column); the results stay in registers until every column of the block has been read.
  int v[3][8];
  #pragma unroll
  for (int k = 0; k < 3; ++k) {
    const int it = tid + TR_THREADS * k, b = it >> 3, c = it & 7;
    if (b >= nblk) continue;
    #pragma unroll
    for (int i = 0; i < 8; ++i) v[k][i] = ws[b * TR_BLK_STRIDE + i * 8 + c];
    dct8<false>(v[k]);
  }
  __syncthreads();
  // Quantisation (jcdctmgr.c forward_DCT: divide by 8 q, round to nearest, ties away from zero) into the zigzag position.
  #pragma unroll
  for (int k = 0; k < 3; ++k) {
    const int it = tid + TR_THREADS * k, b = it >> 3, c = it & 7;
    if (b >= nblk) continue;
    const int chroma = (b % 6) >= 4 ? 64 : 0;
    #pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int zz = izz[i * 8 + c];
      const unsigned qv = (unsigned)q[chroma + zz] << 3;
      const int t = v[k][i];
      const int a = (int)(((unsigned)abs(t) + (qv >> 1)) / qv);
      ws[b * TR_BLK_STRIDE + zz] = (short)(t < 0 ? -a : a);
    }
  }
  __syncthreads();
  // The tile's blocks are contiguous in the MCU-interleaved coefficient buffer: 16-byte stores.
  short* dst = coef + ((size_t)my * mcux + m0) * 6 * 64;
  for (int i = tid; i < nblk * 8; i += TR_THREADS) {
    const int b = i >> 3, j = i & 7;
    *reinterpret_cast<int4*>(dst + b * 64 + j * 8) = *reinterpret_cast<const int4*>(ws + b * TR_BLK_STRIDE + j * 8);
  }
}

// ---- step 2: entropy coding -----------------------------------------------------------------------------------------------------
constexpr int EN_THREADS = 256;                               // blocks coded per round (one per lane)
constexpr int EN_CF_STRIDE = 66;                              // int16 per staged block: 33 dwords, so lanes read distinct banks
constexpr int EN_BITS_WORDS = EN_THREADS * (JPEG_BLOCK_BITS / 32) + 2;   // worst case of a round + the carried byte + one spare
constexpr size_t EN_LDS_BYTES = (size_t)EN_BITS_WORDS * 4 + (size_t)EN_THREADS * EN_CF_STRIDE * 2 + HUFF_WORDS * 4 + 8 * 4;

// MSB-first bit writer into the round's LDS buffer from bit position `pos`.  The first and the last word of a lane's string are
// shared with its neighbours (LDS atomic OR into zeroed words); the words in between are its own (plain stores).
struct BitWriter {
  unsigned* buf;
  unsigned word;
  unsigned long long acc;
  int n;
  bool shared;
  __device__ BitWriter(unsigned* b, unsigned pos) : buf(b), word(pos >> 5), acc(0), n((int)(pos & 31)), shared((pos & 31) != 0) {}
  __device__ __forceinline__ void put(unsigned bits, int len) {
    acc = (acc << len) | bits;
    n += len;
    if (n >= 32) {
      const unsigned w = (unsigned)(acc >> (n - 32));
      if (shared) atomicOr(buf + word, w); else buf[word] = w;
      shared = false;
      ++word;
      n -= 32;
    }
  }
  __device__ __forceinline__ void finish() {
    if (n > 0) atomicOr(buf + word, (unsigned)(acc << (32 - n)));
  }
};
struct BitCounter {
  unsigned n = 0;
  __device__ __forceinline__ void put(unsigned, int len) { n += len; }
};

// Huffman-code one block (zigzag-ordered coefficients `c` in LDS, DC difference `diff`) with the tables of its component.
template <class Sink>
__device__ __forceinline__ void code_block(const short* c, int diff, const unsigned* hdc, const unsigned* hac, Sink& out) {
  {
    const int s = diff ? 32 - __clz(abs(diff)) : 0;
    const unsigned e = hdc[s];
    out.put(((e & 0xFFFF) << s) | ((unsigned)(diff > 0 ? diff : diff - 1) & ((1u << s) - 1)), (int)(e >> 16) + s);
  }
  const unsigned zrl = hac[0xF0], eob = hac[0];
  const unsigned* c2 = reinterpret_cast<const unsigned*>(c);
  int run = 0;
  for (int k2 = 0; k2 < 32; ++k2) {
    const unsigned two = c2[k2];
    #pragma unroll
    for (int h = 0; h < 2; ++h) {
      if (k2 == 0 && h == 0) continue;                        // the DC coefficient
      const int v = (short)(h ? two >> 16 : two & 0xFFFF);
      if (v == 0) { ++run; continue; }
      while (run > 15) { out.put(zrl & 0xFFFF, (int)(zrl >> 16)); run -= 16; }
      const int s = 32 - __clz(abs(v));
      const unsigned e = hac[(run << 4) | s];
      out.put(((e & 0xFFFF) << s) | ((unsigned)(v > 0 ? v : v - 1) & ((1u << s) - 1)), (int)(e >> 16) + s);
      run = 0;
    }
  }
  if (run) out.put(eob & 0xFFFF, (int)(eob >> 16));
}

__global__ __launch_bounds__(EN_THREADS) void jpeg_entropy(const short* __restrict__ coef, int mcux, const unsigned* __restrict__ huff_g,
                                                           unsigned char* __restrict__ slots, size_t slot_bytes,
                                                           unsigned* __restrict__ lens) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  unsigned* bits = reinterpret_cast<unsigned*>(smem);
  short* cf = reinterpret_cast<short*>(bits + EN_BITS_WORDS);
  unsigned* huff = reinterpret_cast<unsigned*>(cf + EN_THREADS * EN_CF_STRIDE);
  unsigned* wsum = huff + HUFF_WORDS;
  const int tid = threadIdx.x;
  const int row = blockIdx.x, nblk = mcux * 6;
  const short* src = coef + (size_t)row * nblk * 64;
  unsigned char* out = slots + (size_t)row * slot_bytes;
  for (int i = tid; i < HUFF_WORDS; i += EN_THREADS) huff[i] = huff_g[i];
  unsigned carry_bits = 0, carry_word = 0;      // the unfinished byte of the previous round, in the top bits of a word
  unsigned out_pos = 0;
  for (int c0 = 0; c0 < nblk; c0 += EN_THREADS) {
    const int n = min(EN_THREADS, nblk - c0);
    // the round's coefficients: coalesced 16-byte reads, dword stores to distinct banks
    for (int i = tid; i < n * 8; i += EN_THREADS) {
      const int b = i >> 3, j = i & 7;
      const int4 v = *reinterpret_cast<const int4*>(src + (size_t)(c0 + b) * 64 + j * 8);
      unsigned* d = reinterpret_cast<unsigned*>(cf + b * EN_CF_STRIDE + j * 8);
      d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w;
    }
    __syncthreads();
    // DC difference: the predecessor of the same component is known (Y00 <- the previous MCU's Y11, Y01 <- Y00, ...,
    // Cb / Cr <- the previous MCU's); the first MCU of the interval predicts from 0.
    const bool active = tid < n;
    const int g = c0 + tid, k6 = g % 6;
    const short* mine = cf + tid * EN_CF_STRIDE;
    const unsigned* hdc = huff + HUFF_DC + (k6 >= 4 ? 12 : 0);
    const unsigned* hac = huff + HUFF_AC + (k6 >= 4 ? 256 : 0);
    int diff = 0;
    unsigned len = 0;
    if (active) {
      const int prev = k6 == 0 ? g - 3 : (k6 < 4 ? g - 1 : g - 6);
      diff = mine[0] - (prev < 0 ? 0 : (int)src[(size_t)prev * 64]);
      BitCounter cnt;
      code_block(mine, diff, hdc, hac, cnt);
      len = cnt.n;
    }
    unsigned total;
    const unsigned ex = block_exscan<EN_THREADS / 64>(len, wsum, &total);
    unsigned T = carry_bits + total;
    const bool last = c0 + EN_THREADS >= nblk;
    const unsigned fill = last ? (0u - T) & 7 : 0;            // the interval ends padded with 1-bits to a byte boundary
    for (unsigned i = tid; i < (T + fill + 31) / 32 + 1; i += EN_THREADS) bits[i] = i == 0 ? carry_word : 0;
    __syncthreads();
    if (active) {
      BitWriter w(bits, carry_bits + ex);
      code_block(mine, diff, hdc, hac, w);
      if (tid == n - 1 && fill) w.put((1u << fill) - 1, (int)fill);
      w.finish();
    }
    __syncthreads();
    T += fill;
    // Byte stuffing behind a second prefix sum: a thread takes 4 bytes of the merged string, counts its 0xFF, and writes its
    // bytes (each 0xFF followed by 0x00) at its offset in the interval's slot.
    const unsigned nbytes = T >> 3;
    for (unsigned base = 0; base < nbytes; base += EN_THREADS * 4) {
      const unsigned j = base + tid * 4;
      const unsigned nb = j < nbytes ? min(4u, nbytes - j) : 0;
      const unsigned w = nb ? bits[j >> 2] : 0;
      unsigned ff = 0;
      for (unsigned b = 0; b < nb; ++b) ff += ((w >> (24 - 8 * b)) & 0xFF) == 0xFF;
      unsigned tot;
      unsigned o = out_pos + tid * 4 + block_exscan<EN_THREADS / 64>(ff, wsum, &tot);       // out_pos already counts the rounds before
      for (unsigned b = 0; b < nb; ++b) {
        const unsigned char byte = (unsigned char)(w >> (24 - 8 * b));
        out[o++] = byte;
        if (byte == 0xFF) out[o++] = 0;
      }
      out_pos += min((unsigned)EN_THREADS * 4, nbytes - base) + tot;
    }
    carry_bits = T & 7;
    carry_word = carry_bits ? ((bits[nbytes >> 2] >> (24 - 8 * (nbytes & 3))) & 0xFF & (0xFF00u >> carry_bits)) << 24 : 0;
    __syncthreads();
  }
  if (tid == 0) lens[row] = out_pos;
}

// ---- step 3: compaction ---------------------------------------------------------------------------------------------------------
constexpr int CP_THREADS = 256;

__global__ __launch_bounds__(CP_THREADS) void jpeg_compact(const unsigned char* __restrict__ slots, size_t slot_bytes,
                                                           const unsigned* __restrict__ lens, int mcuy,
                                                           const unsigned char* __restrict__ header, HeaderPatch hp,
                                                           const unsigned short* __restrict__ qtab, int H, int W, int mcux,
                                                           unsigned char* __restrict__ out, unsigned* __restrict__ d_len) {
  __shared__ unsigned long long part[CP_THREADS / 64];
  const int tid = threadIdx.x, row = blockIdx.x;
  // exclusive prefix sum of (length + 2 marker bytes) over the intervals before this one
  unsigned long long s = 0;
  for (int i = tid; i < row; i += CP_THREADS) s += lens[i] + 2;
  #pragma unroll
  for (int d = 32; d >= 1; d >>= 1) s += __shfl_xor(s, d);
  if ((tid & 63) == 0) part[tid >> 6] = s;
  __syncthreads();
  size_t off = 0;
  #pragma unroll
  for (int w = 0; w < CP_THREADS / 64; ++w) off += part[w];
  if (row == 0)
    for (int i = tid; i < JPEG_HEADER_BYTES; i += CP_THREADS) {
      unsigned b = header[i];
      if (i >= hp.dqt[0] && i < hp.dqt[0] + 64) b = qtab[i - hp.dqt[0]];
      else if (i >= hp.dqt[1] && i < hp.dqt[1] + 64) b = qtab[64 + i - hp.dqt[1]];
      else if (i == hp.size) b = H >> 8;
      else if (i == hp.size + 1) b = H & 0xFF;
      else if (i == hp.size + 2) b = W >> 8;
      else if (i == hp.size + 3) b = W & 0xFF;
      else if (i == hp.dri) b = mcux >> 8;
      else if (i == hp.dri + 1) b = mcux & 0xFF;
      out[i] = (unsigned char)b;
    }
  const unsigned n = lens[row];
  const unsigned char* src = slots + (size_t)row * slot_bytes;
  unsigned char* dst = out + JPEG_HEADER_BYTES + off;
  // bytes up to the destination's first dword boundary, whole destination dwords from two aligned source dwords, the rest
  const unsigned head = min(n, (unsigned)((4 - ((uintptr_t)dst & 3)) & 3));
  if ((unsigned)tid < head) dst[tid] = src[tid];
  const unsigned nd = (n - head) / 4;
  const unsigned mis = (unsigned)((uintptr_t)(src + head) & 3);
  const unsigned* s4 = reinterpret_cast<const unsigned*>(src + head - mis);
  unsigned* d4 = reinterpret_cast<unsigned*>(dst + head);
  for (unsigned d = tid; d < nd; d += CP_THREADS) {
    unsigned v = s4[d];
    if (mis) v = (v >> (8 * mis)) | (s4[d + 1] << (32 - 8 * mis));      // (the slots end in a spare dword)
    d4[d] = v;
  }
  for (unsigned i = head + 4 * nd + tid; i < n; i += CP_THREADS) dst[i] = src[i];
  if (tid == 0) {
    dst[n] = 0xFF;
    dst[n + 1] = row == mcuy - 1 ? 0xD9 : (unsigned char)(0xD0 + (row & 7));       // RSTm, m modulo 8; EOI after the last interval
    if (row == mcuy - 1) *d_len = (unsigned)(JPEG_HEADER_BYTES + off + n + 2);
  }
}

// ---- host ------------------------------------------------------------------------------------------------------------------------
void huff_entries(const unsigned char* bits, const unsigned char* vals, unsigned* table) {
  unsigned code = 0;
  int k = 0;
  for (int len = 1; len <= 16; ++len) {
    for (int i = 0; i < bits[len - 1]; ++i) table[vals[k++]] = (unsigned)len << 16 | code++;
    code <<= 1;
  }
}

void segment(std::vector<unsigned char>& h, int marker, const std::vector<unsigned char>& payload) {
  h.push_back(0xFF);
  h.push_back((unsigned char)marker);
  h.push_back((unsigned char)((payload.size() + 2) >> 8));
  h.push_back((unsigned char)((payload.size() + 2) & 0xFF));
  h.insert(h.end(), payload.begin(), payload.end());
}

// SOI, APP0 (JFIF 1.01, density 1:1), DQT x2, SOF0 (4:2:0), DHT x4, DRI, SOS; tables, size and restart interval left zero.
std::vector<unsigned char> header_template(HeaderPatch* hp) {
  std::vector<unsigned char> h = {0xFF, 0xD8};
  segment(h, 0xE0, {'J', 'F', 'I', 'F', 0, 1, 1, 0, 0, 1, 0, 1, 0, 0});
  for (int t = 0; t < 2; ++t) {
    std::vector<unsigned char> p(65, 0);
    p[0] = (unsigned char)t;
    hp->dqt[t] = (int)h.size() + 5;
    segment(h, 0xDB, p);
  }
  hp->size = (int)h.size() + 5;
  segment(h, 0xC0, {8, 0, 0, 0, 0, 3, 1, 0x22, 0, 2, 0x11, 1, 3, 0x11, 1});
  for (int t = 0; t < 2; ++t) {
    std::vector<unsigned char> p = {(unsigned char)t};
    p.insert(p.end(), DC_BITS[t], DC_BITS[t] + 16);
    p.insert(p.end(), DC_VALS, DC_VALS + 12);
    segment(h, 0xC4, p);
    p.assign(1, (unsigned char)(0x10 | t));
    p.insert(p.end(), AC_BITS[t], AC_BITS[t] + 16);
    p.insert(p.end(), AC_VALS[t], AC_VALS[t] + 162);
    segment(h, 0xC4, p);
  }
  hp->dri = (int)h.size() + 4;
  segment(h, 0xDD, {0, 0});
  segment(h, 0xDA, {3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0});
  return h;
}

size_t jpeg_worst_case(int H, int W) {
  const size_t mcux = (W + 15) / 16, mcuy = (H + 15) / 16;
  return JPEG_HEADER_BYTES + mcuy * (mcux * 6 * JPEG_BLOCK_BYTES + 2);
}

}  // namespace

struct poco_jpeg_encoder {
  int max_h = 0, max_w = 0;
  HeaderPatch hp{};
  JpegTables* tables = nullptr;            // device
  short* coef = nullptr;                   // [mcuy][mcux][6][64] quantised, zigzag order
  unsigned char* slots = nullptr;          // [mcuy] worst-case slots of entropy-coded bytes (+ one spare dword)
  unsigned* lens = nullptr;                // [mcuy]
  ~poco_jpeg_encoder() {
    for (void* p : {(void*)tables, (void*)coef, (void*)slots, (void*)lens})
      if (p) (void)hipFree(p);
  }
};

extern "C" int poco_jpeg_encoder_create(int max_h, int max_w, poco_jpeg_encoder_t* out) {
  if (!out) { poco_set_error("poco_jpeg_encoder_create: null handle pointer"); return POCO_ERR_ARG; }
  *out = nullptr;
  if (max_h < 1 || max_w < 1 || max_h > JPEG_MAX_SIDE || max_w > JPEG_MAX_SIDE) {
    poco_set_error("poco_jpeg_encoder_create: bad arguments (need 1 <= max_h, max_w <= 16384)");
    return POCO_ERR_ARG;
  }
  std::vector<unsigned char> hdr;
  HeaderPatch hp;
  hdr = header_template(&hp);
  if (hdr.size() != JPEG_HEADER_BYTES) { poco_set_error("poco_jpeg_encoder_create: header size"); return POCO_ERR_STATE; }
  auto t = std::make_unique<JpegTables>();
  std::memset(t.get(), 0, sizeof(JpegTables));
  for (int q = 1; q <= 100; ++q) {                           // jpeg_quality_scaling + the baseline clamp of jpeg_add_quant_table
    const int scale = q < 50 ? 5000 / q : 200 - 2 * q;
    for (int c = 0; c < 2; ++c)
      for (int z = 0; z < 64; ++z)
        t->qtab[q - 1][c][z] = (unsigned short)std::min(std::max((QUANT[c][ZIGZAG[z]] * scale + 50) / 100, 1), 255);
  }
  for (int c = 0; c < 2; ++c) {
    huff_entries(AC_BITS[c], AC_VALS[c], t->huff + HUFF_AC + 256 * c);
    huff_entries(DC_BITS[c], DC_VALS, t->huff + HUFF_DC + 12 * c);
  }
  for (int z = 0; z < 64; ++z) t->izz[ZIGZAG[z]] = (unsigned char)z;
  std::memcpy(t->header, hdr.data(), hdr.size());
  auto e = std::make_unique<poco_jpeg_encoder>();
  e->max_h = max_h;
  e->max_w = max_w;
  e->hp = hp;
  const size_t mcux = (max_w + 15) / 16, mcuy = (max_h + 15) / 16;
  POCO_HIP_CHECK(hipMalloc(&e->tables, sizeof(JpegTables)));
  POCO_HIP_CHECK(hipMemcpy(e->tables, t.get(), sizeof(JpegTables), hipMemcpyHostToDevice));
  POCO_HIP_CHECK(hipMalloc(&e->coef, mcuy * mcux * 6 * 64 * sizeof(short)));
  POCO_HIP_CHECK(hipMalloc(&e->slots, mcuy * mcux * 6 * JPEG_BLOCK_BYTES + 8));
  POCO_HIP_CHECK(hipMalloc(&e->lens, mcuy * sizeof(unsigned)));
  POCO_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(jpeg_entropy), hipFuncAttributeMaxDynamicSharedMemorySize,
                                     (int)EN_LDS_BYTES));
  *out = e.release();
  return POCO_OK;
}

extern "C" int poco_jpeg_encode(poco_jpeg_encoder_t e, const unsigned char* d_rgb, int H, int W, int quality, unsigned char* d_out,
                                size_t out_cap, unsigned int* d_len, void* stream) {
  if (!e || !d_rgb || !d_out || !d_len) { poco_set_error("poco_jpeg_encode: null handle or pointer"); return POCO_ERR_ARG; }
  if (H < 1 || W < 1 || H > e->max_h || W > e->max_w) {
    poco_set_error("poco_jpeg_encode: frame of " + std::to_string(H) + " x " + std::to_string(W) + " outside 1 x 1 .. " +
                   std::to_string(e->max_h) + " x " + std::to_string(e->max_w) + " (the size the encoder was created for)");
    return POCO_ERR_ARG;
  }
  if (quality < 1 || quality > 100) { poco_set_error("poco_jpeg_encode: quality must be in 1..100"); return POCO_ERR_ARG; }
  if (out_cap < jpeg_worst_case(H, W)) {
    poco_set_error("poco_jpeg_encode: out_cap " + std::to_string(out_cap) + " is below the worst case of " +
                   std::to_string(jpeg_worst_case(H, W)) + " bytes for this frame size");
    return POCO_ERR_ARG;
  }
  const hipStream_t s = (hipStream_t)stream;
  const int mcux = (W + 15) / 16, mcuy = (H + 15) / 16;
  const size_t slot = (size_t)mcux * 6 * JPEG_BLOCK_BYTES;
  const unsigned short* qtab = &e->tables->qtab[quality - 1][0][0];
  jpeg_transform<<<dim3((mcux + TR_MCUS - 1) / TR_MCUS, mcuy), TR_THREADS, 0, s>>>(d_rgb, H, W, mcux, qtab, e->tables->izz, e->coef);
  jpeg_entropy<<<mcuy, EN_THREADS, EN_LDS_BYTES, s>>>(e->coef, mcux, e->tables->huff, e->slots, slot, e->lens);
  jpeg_compact<<<mcuy, CP_THREADS, 0, s>>>(e->slots, slot, e->lens, mcuy, e->tables->header, e->hp, qtab, H, W, mcux, d_out, d_len);
  POCO_HIP_CHECK(hipGetLastError());
  return POCO_OK;
}

extern "C" void poco_jpeg_encoder_destroy(poco_jpeg_encoder_t e) { delete e; }
