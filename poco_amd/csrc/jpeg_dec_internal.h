// What csrc/jpeg_prog.hip shares with csrc/jpeg_dec.hip: the per-image record the inverse DCT and the colour kernel read, the
// Huffman table both decoders look codes up in, and the launch of those two kernels (defined in jpeg_dec.hip, unchanged).
#pragma once
#include "common.h"

#include <cstddef>

namespace jdec {

constexpr int JD_MAX_SIDE = 16384;
constexpr int JD_LOOKAHEAD = 9;          // bits of the lookahead table
constexpr int JD_THREADS = 256;          // subsequences per workgroup
constexpr int JD_MAX_BATCH = 4096;
constexpr int JD_ERR_CODE = 1, JD_ERR_SHORT = 2;

typedef unsigned long long u64;

struct HuffTab {
  unsigned short look[1 << JD_LOOKAHEAD];   // length << 8 | symbol of the code at the top of the window, 0 = none this short
  int maxcode[18];                          // [l]: largest code of length l, -1 = none
  int delta[17];                            // valptr[l] - mincode[l]
  unsigned char vals[256];
};
static_assert(sizeof(HuffTab) % 4 == 0, "copied as dwords");

struct DImg {
  u64 coef_off;                 // first block of the image in the coefficient scratch
  u64 plane_off[3];             // bytes into the plane scratch
  unsigned char* out;
  unsigned data_off, nbytes;    // the image's bytes in the blob
  int H, W, ncomp, hs, vs, bpm, mcux, mcuy, nblocks;
  int cw, ch, fancy;            // chroma planes' own size; the fancy filters apply (cw > 2)
  int pw[3];                    // plane widths (whole blocks)
  int nseg, seg_off, nsub, sub_off, nwg, wg_off;
  unsigned char comp_of[8];     // component of each block of an MCU
  unsigned short qt[3][64];
  HuffTab tab[6];               // [component * 2 + (AC)]
};
static_assert(sizeof(DImg) % 8 == 0, "array of 8-byte aligned records");

bool build_table(const unsigned char* bits, const unsigned char* vals, bool dc, HuffTab* t);
size_t max_blocks(int H, int W);
// jdec_idct then jdec_colour over d_img[0 .. n): max_idct = the most workgroups of 32 blocks an image needs, max_dwords = the most
// aligned dwords a picture spans.
void launch_idct_colour(const DImg* d_img, int n, const short* coef, unsigned char* planes, int max_idct, long long max_dwords,
                        hipStream_t s);

}  // namespace jdec
