// Progressive JPEG decoder for the demo's input frames: the scans of a batch of parsed SOF2 files (poco_amd/jpeg.py
// parse_progressive_jpeg) -> the int16 coefficient buffer jpeg_dec.hip's inverse DCT reads -> one uint8 [H,W,3] RGB picture per
// file.  The contract is stated in include/poco_hip.h and DESIGN.md 17; tests/jpegprog_np.py restates the coefficient stage in
// numpy (jdphuff.c's decoders), pinned on PIL, and the GPU tests compare BYTES.  Integer arithmetic only.
//
// One host-to-device copy (image records, scan table, Huffman tables, bytes), two memsets, then on the caller's stream:
//   jprog_scan    one launch per LEVEL of the scan order, one wave per scan of that level.  The level of a scan is the length of
//                 the longest chain of earlier scans of its file that touch one of its (component, coefficient) pairs, so a launch
//                 holds only scans that are independent of each other (other components, other bands, other images) and every scan
//                 finds the coefficients its predecessors left.  The wave walks the scan's symbols with ONE bit reader whose
//                 state is uniform across the lanes; the lanes are the 64 zigzag positions of the block in hand: a refinement scan
//                 loads the block with one coalesced read (the next block's is in flight meanwhile), votes the non-zero history
//                 into a 64-bit mask, takes runs and correction bits by mask arithmetic and stores the changed coefficients.
//                 DC values are final (the prediction is a register of the walk): there is no jdec_dc pass.
//   jdec_idct, jdec_colour   jpeg_dec.hip's, through jdec::launch_idct_colour.
// Every loop is bounded by a constant or by a count the host validated; every read of the stream is clamped to its scan (bytes
// behind it read as zero bits, and a scan that consumes one is damaged); every store is guarded by its own index.  No global
// atomics: every coefficient has one writer per launch; every writer of a status word stores a non-zero value.
#include "common.h"
#include "jpeg_dec_internal.h"
#include "../../include/poco_hip.h"

#include <algorithm>
#include <cstddef>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

using namespace jdec;

namespace {

constexpr int JP_MAX_SCANS = 64;          // per file (poco_amd/jpeg.py MAX_SCANS)
constexpr int JP_TABS_PER_IMAGE = 16;     // Huffman tables planned per image of the batch (poco_amd/jpeg.py TABLES_PER_IMAGE)
constexpr int JP_WAVE = 64;

struct PScan {
  unsigned off, len;            // the scan's bytes in the image's
  int img;
  int tab[3];                   // tables in the call's table array
  unsigned char ncomp, comp, ss, se, ah, al, pad[2];
};
static_assert(sizeof(PScan) == 32, "array of 16-byte aligned records");

__device__ const unsigned char JP_ZZ[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                            41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                            30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

// Bits MSB first from bytes [pos, end) of the image's data, the byte behind an 0xFF skipped, zero bits behind `end`.
struct BitReader {
  const unsigned* w;            // the image's bytes as aligned dwords (the staging layout pads every image to 16 bytes)
  unsigned pos, end, ci, cur;   // ci: index of the cached dword `cur`
  u64 acc;                      // the next n bits, left-aligned
  int n, fake;                  // fake: how many of the n are zeros from behind `end` (they are the last ones)
};

__device__ __forceinline__ void br_init(BitReader& b, const unsigned char* d, unsigned off, unsigned len) {
  b.w = reinterpret_cast<const unsigned*>(d);
  b.pos = off; b.end = off + len; b.ci = 0xFFFFFFFFu; b.cur = 0; b.acc = 0; b.n = 0; b.fake = 0;
}

// At least 57 bits afterwards.
__device__ __forceinline__ void br_fill(BitReader& b) {
  #pragma unroll 1
  for (int it = 0; it < 8 && b.n <= 56; ++it) {
    unsigned byte = 0;
    if (b.pos < b.end) {
      const unsigned i = b.pos >> 2;
      if (i != b.ci) { b.cur = b.w[i]; b.ci = i; }
      byte = (b.cur >> ((b.pos & 3) * 8)) & 255u;
      b.pos += (byte == 0xFF && b.pos + 1 < b.end) ? 2 : 1;
    } else {
      b.fake += 8;
    }
    b.acc |= (u64)byte << (56 - b.n);
    b.n += 8;
  }
}

__device__ __forceinline__ unsigned br_get(BitReader& b, int k) {       // k in 0 .. 32, after br_fill
  if (k == 0) return 0;
  const unsigned v = (unsigned)(b.acc >> (64 - k));
  b.acc <<= k;
  b.n -= k;
  return v;
}

__device__ __forceinline__ bool br_short(const BitReader& b) { return b.n < b.fake; }

// One Huffman symbol (after br_fill); -1 when the window holds no code.
__device__ __forceinline__ int huff_symbol(BitReader& b, const HuffTab& t) {
  const unsigned w16 = (unsigned)(b.acc >> 48);
  const unsigned e = t.look[w16 >> (16 - JD_LOOKAHEAD)];
  int ln = (int)(e >> 8), sym = (int)(e & 255);
  if (e == 0) {
    ln = 0;
    for (int l = JD_LOOKAHEAD + 1; l <= 16; ++l) {
      const int c = (int)(w16 >> (16 - l));
      if (c <= t.maxcode[l]) {
        const int i = c + t.delta[l];
        if ((unsigned)i < 256u) { ln = l; sym = t.vals[i]; }
        break;
      }
    }
    if (ln == 0) return -1;
  }
  b.acc <<= ln;
  b.n -= ln;
  return sym;
}

__device__ __forceinline__ int extend(unsigned v, int s) { return s == 0 ? 0 : (v >= (1u << (s - 1)) ? (int)v : (int)v - (1 << s) + 1); }

// bits a .. b of a 64-bit mask (0 <= a, b <= 63), none when a > b
__device__ __forceinline__ u64 bit_range(int a, int b) { return a > b ? 0ull : ((~0ull >> (63 - b)) & (~0ull << a)); }

// The block of component c at (bx, by) of the component's own raster, in the MCU-ordered coefficient buffer.
__device__ __forceinline__ unsigned block_of(const DImg* im, int c, int bx, int by) {
  if (c == 0) return (unsigned)(((by / im->vs) * im->mcux + bx / im->hs) * im->bpm + (by % im->vs) * im->hs + bx % im->hs);
  return (unsigned)((by * im->mcux + bx) * im->bpm + im->hs * im->vs + c - 1);
}

// `cnt` (<= 64) correction bits for the lanes whose bit is set in `seg`, in zigzag order: true for a lane whose bit is 1.
__device__ __forceinline__ bool take_corrections(BitReader& b, u64 seg, int lane) {
  const int cnt = __popcll(seg);
  const int rank = __popcll(seg & ((1ull << lane) - 1ull));
  const bool mine = (seg >> lane) & 1ull;
  bool bit = false;
  int done = 0;
  #pragma unroll 1
  for (int it = 0; it < 2 && done < cnt; ++it) {
    const int c = min(cnt - done, 32);
    br_fill(b);
    const unsigned v = br_get(b, c);
    const int r = rank - done;
    if (mine && r >= 0 && r < c) bit = (v >> (c - 1 - r)) & 1u;
    done += c;
  }
  return bit;
}

__global__ __launch_bounds__(JP_WAVE) void jprog_scan(const unsigned char* __restrict__ blob, const DImg* __restrict__ imgs,
                                                      const PScan* __restrict__ scans, const HuffTab* __restrict__ tabs_g,
                                                      short* __restrict__ coef_g, int* __restrict__ status) {
  __shared__ HuffTab tabs[3];
  const PScan sc = scans[blockIdx.x];
  const DImg* im = imgs + sc.img;
  const int lane = threadIdx.x;
  const bool dc = sc.ss == 0, first = sc.ah == 0;
  const int ntab = dc ? (first ? sc.ncomp : 0) : 1;
  for (int t = 0; t < ntab; ++t) {
    const unsigned* src = reinterpret_cast<const unsigned*>(tabs_g + sc.tab[t]);
    unsigned* dst = reinterpret_cast<unsigned*>(tabs + t);
    for (int i = lane; i < (int)(sizeof(HuffTab) / 4); i += JP_WAVE) dst[i] = src[i];
  }
  __syncthreads();
  BitReader b;
  br_init(b, blob + im->data_off, sc.off, sc.len);
  short* coef = coef_g + im->coef_off * 64;
  const unsigned nblocks = (unsigned)im->nblocks;
  const int al = sc.al, ss = sc.ss, se = sc.se, c0 = sc.comp;
  // what the scan covers: whole MCUs when interleaved, else the component's own blocks in raster order
  const bool inter = sc.ncomp > 1;
  const int bw = inter ? 0 : (c0 == 0 ? (im->W + 7) / 8 : (im->cw + 7) / 8);
  const int bh = inter ? 0 : (c0 == 0 ? (im->H + 7) / 8 : (im->ch + 7) / 8);
  const unsigned total = inter ? nblocks : (unsigned)(bw * bh);
  int err = 0;

  if (dc && first) {
    int p0 = 0, p1 = 0, p2 = 0;
    int bx = 0, by = 0, k = 0;
    #pragma unroll 1
    for (unsigned i = 0; i < total; ++i) {
      const int t = inter ? (int)im->comp_of[k] : 0;
      const unsigned blk = inter ? i : block_of(im, c0, bx, by);
      br_fill(b);
      const int s = huff_symbol(b, tabs[t]);
      if (s < 0 || s > 15) { err = JD_ERR_CODE; break; }
      const int v = extend(br_get(b, s), s);
      if (br_short(b)) { err = JD_ERR_SHORT; break; }
      int pred;
      if (t == 0) pred = (p0 += v); else if (t == 1) pred = (p1 += v); else pred = (p2 += v);
      if (lane == 0 && blk < nblocks) coef[(size_t)blk * 64] = (short)(pred * (1 << al));
      if (inter) { if (++k == im->bpm) k = 0; } else if (++bx == bw) { bx = 0; ++by; }
    }
  } else if (dc) {
    // one bit per block: 64 blocks a round, lane j takes the j-th
    #pragma unroll 1
    for (unsigned i0 = 0; i0 < total; i0 += 64) {
      const int cnt = (int)min(64u, total - i0);
      br_fill(b);
      const unsigned hi = br_get(b, min(cnt, 32));
      br_fill(b);
      const unsigned lo = br_get(b, max(cnt - 32, 0));
      if (br_short(b)) { err = JD_ERR_SHORT; break; }
      const unsigned i = i0 + lane;
      if (lane < cnt) {
        const bool bit = lane < 32 ? (hi >> (min(cnt, 32) - 1 - lane)) & 1u : (lo >> (cnt - 1 - lane)) & 1u;
        const unsigned blk = inter ? i : block_of(im, c0, (int)(i % (unsigned)bw), (int)(i / (unsigned)bw));
        if (bit && blk < nblocks) coef[(size_t)blk * 64] |= (short)(1 << al);
      }
    }
  } else if (first) {
    const HuffTab& t = tabs[0];
    const int zz = JP_ZZ[lane];
    #pragma unroll 1
    for (unsigned i = 0; i < total; ++i) {
      const unsigned blk = block_of(im, c0, (int)(i % (unsigned)bw), (int)(i / (unsigned)bw));
      u64 mask = 0;
      int mine = 0;
      #pragma unroll 1
      for (int k = ss; k <= se; ++k) {
        br_fill(b);
        const int sym = huff_symbol(b, t);
        if (sym < 0) { err = JD_ERR_CODE; break; }
        const int r = sym >> 4, s = sym & 15;
        if (s) {
          k += r;
          if (k > se) { err = JD_ERR_CODE; break; }
          const int v = extend(br_get(b, s), s) * (1 << al);
          if (lane == k) mine = v;
          mask |= 1ull << k;
        } else if (r == 15) {
          k += 15;
        } else {
          const unsigned run = (1u << r) + br_get(b, r) - 1u;      // blocks behind this one that are at their end of band too
          if (run > total - 1u - i) { err = JD_ERR_CODE; break; }
          i += run;
          break;
        }
        if (br_short(b)) break;
      }
      if (!err && br_short(b)) err = JD_ERR_SHORT;
      if (((mask >> lane) & 1ull) && blk < nblocks) coef[(size_t)blk * 64 + zz] = (short)mine;
      if (err) break;
    }
  } else {
    const HuffTab& t = tabs[0];
    const int zz = JP_ZZ[lane];
    const int p1 = 1 << al;
    const u64 band = bit_range(ss, se);
    unsigned eobrun = 0;
    unsigned blk = total ? block_of(im, c0, 0, 0) : 0;
    short cv = blk < nblocks && total ? coef[(size_t)blk * 64 + zz] : (short)0;
    int bx = 0, by = 0;
    #pragma unroll 1
    for (unsigned i = 0; i < total; ++i) {
      // the next block's coefficients are on their way while this one is decoded
      if (++bx == bw) { bx = 0; ++by; }
      const unsigned nblk = i + 1 < total ? block_of(im, c0, bx, by) : 0xFFFFFFFFu;
      const short nv = nblk < nblocks ? coef[(size_t)nblk * 64 + zz] : (short)0;
      int c = cv;
      const u64 nz = __ballot(c != 0) & band;
      bool corr = false;
      u64 newmask = 0, newneg = 0;
      int k = ss;
      if (eobrun == 0) {
        #pragma unroll 1
        for (int it = 0; it < 64 && k <= se; ++it) {
          br_fill(b);
          const int sym = huff_symbol(b, t);
          if (sym < 0) { err = JD_ERR_CODE; break; }
          int r = sym >> 4;
          const int s = sym & 15;
          bool neg = false;
          if (s) {
            if (s != 1) { err = JD_ERR_CODE; break; }
            neg = br_get(b, 1) == 0;
          } else if (r != 15) {
            eobrun = (1u << r) + br_get(b, r);
            if (eobrun - 1u > total - 1u - i) { err = JD_ERR_CODE; eobrun = 0; }
            break;
          }
          // r zeros are skipped and the run ends at the next one; every non-zero coefficient on the way takes a correction bit
          u64 zeros = ~nz & bit_range(k, se);
          for (int j = 0; j < 15 && j < r && zeros; ++j) zeros &= zeros - 1ull;
          const int pos = zeros ? __ffsll((long long)zeros) - 1 : se + 1;
          corr |= take_corrections(b, nz & bit_range(k, pos - 1), lane);
          if (s) {
            if (pos > se) { err = JD_ERR_CODE; break; }
            newmask |= 1ull << pos;
            if (neg) newneg |= 1ull << pos;
          }
          k = pos + 1;
          if (br_short(b)) break;
        }
      }
      if (!err && eobrun > 0) {
        corr |= take_corrections(b, nz & bit_range(k, se), lane);
        --eobrun;
      }
      if (!err && br_short(b)) err = JD_ERR_SHORT;
      bool changed = false;
      if (corr && (c & p1) == 0) { c += c >= 0 ? p1 : -p1; changed = true; }
      if ((newmask >> lane) & 1ull) { c = ((newneg >> lane) & 1ull) ? -p1 : p1; changed = true; }
      if (changed && blk < nblocks) coef[(size_t)blk * 64 + zz] = (short)c;
      if (err) break;
      blk = nblk;
      cv = nv;
    }
  }
  if (err && lane == 0) status[sc.img] = err;
}

size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

}  // namespace

struct poco_jpeg_prog_decoder {
  int max_h = 0, max_w = 0, max_batch = 0;
  size_t max_bytes = 0, blob_cap = 0, blocks_per_image = 0;
  unsigned char* h_blob = nullptr;         // pinned staging
  unsigned char* d_blob = nullptr;
  short* coef = nullptr;                   // [blocks][64] natural order
  unsigned char* planes = nullptr;         // 64 bytes per block
  hipEvent_t copied = nullptr;
  bool in_flight = false;
  ~poco_jpeg_prog_decoder() {
    if (h_blob) (void)hipHostFree(h_blob);
    for (void* p : {(void*)d_blob, (void*)coef, (void*)planes})
      if (p) (void)hipFree(p);
    if (copied) (void)hipEventDestroy(copied);
  }
};

extern "C" int poco_jpeg_prog_decoder_create(int max_h, int max_w, int max_batch, size_t max_bytes, poco_jpeg_prog_decoder_t* out) {
  if (!out) { poco_set_error("poco_jpeg_prog_decoder_create: null handle pointer"); return POCO_ERR_ARG; }
  *out = nullptr;
  if (max_h < 1 || max_w < 1 || max_h > JD_MAX_SIDE || max_w > JD_MAX_SIDE || max_batch < 1 || max_batch > JD_MAX_BATCH ||
      max_bytes < 1 || max_bytes > ((size_t)1 << 30)) {
    poco_set_error("poco_jpeg_prog_decoder_create: bad arguments (need 1 <= max_h, max_w <= 16384, 1 <= max_batch <= 4096, "
                   "1 <= max_bytes <= 2^30)");
    return POCO_ERR_ARG;
  }
  auto d = std::make_unique<poco_jpeg_prog_decoder>();
  d->max_h = max_h;
  d->max_w = max_w;
  d->max_batch = max_batch;
  d->max_bytes = max_bytes;
  d->blocks_per_image = max_blocks(max_h, max_w);
  d->blob_cap = (size_t)max_batch * (sizeof(DImg) + JP_MAX_SCANS * sizeof(PScan) + JP_TABS_PER_IMAGE * sizeof(HuffTab) + 16) + max_bytes + 64;
  const size_t blocks = d->blocks_per_image * max_batch;
  POCO_HIP_CHECK(hipHostMalloc((void**)&d->h_blob, d->blob_cap, hipHostMallocDefault));
  POCO_HIP_CHECK(hipMalloc(&d->d_blob, d->blob_cap));
  POCO_HIP_CHECK(hipMalloc(&d->coef, blocks * 64 * sizeof(short)));
  POCO_HIP_CHECK(hipMalloc(&d->planes, blocks * 64));
  POCO_HIP_CHECK(hipEventCreateWithFlags(&d->copied, hipEventDisableTiming));
  *out = d.release();
  return POCO_OK;
}

extern "C" int poco_jpeg_prog_decode(poco_jpeg_prog_decoder_t dec, const poco_jpeg_prog_image* imgs, int n, int* d_status, void* stream) {
  if (!dec || !imgs || !d_status) { poco_set_error("poco_jpeg_prog_decode: null handle or pointer"); return POCO_ERR_ARG; }
  if (n < 1 || n > dec->max_batch) {
    poco_set_error("poco_jpeg_prog_decode: " + std::to_string(n) + " images, the decoder was created for 1 .. " + std::to_string(dec->max_batch));
    return POCO_ERR_ARG;
  }
  // ---- validate and lay out, before the staging buffer or the GPU is touched
  size_t nbytes = 0, nblocks = 0, plane_bytes = 0;
  int max_idct = 0, nlevels = 0;
  long long max_dwords = 0;
  std::vector<DImg> dim(n);
  std::vector<PScan> scans;                 // in call order; sorted by level below
  std::vector<int> level;
  std::vector<HuffTab> tabs;
  std::vector<int> cut_short;               // images cut short above Al = 0: their status word starts non-zero
  for (int i = 0; i < n; ++i) {
    const poco_jpeg_prog_image& im = imgs[i];
    const std::string who = "poco_jpeg_prog_decode: image " + std::to_string(i) + ": ";
    if (!im.data || !im.scans || !im.d_rgb || (im.ntable > 0 && !im.tables)) { poco_set_error(who + "null pointer"); return POCO_ERR_ARG; }
    if (im.H < 1 || im.W < 1 || im.H > dec->max_h || im.W > dec->max_w) {
      poco_set_error(who + std::to_string(im.H) + " x " + std::to_string(im.W) + " outside 1 x 1 .. " + std::to_string(dec->max_h) +
                     " x " + std::to_string(dec->max_w) + " (the size the decoder was created for)");
      return POCO_ERR_ARG;
    }
    const bool samp_ok = im.ncomp == 1 ? (im.hsamp == 1 && im.vsamp == 1)
                                       : im.ncomp == 3 && ((im.hsamp == 1 && im.vsamp == 1) || (im.hsamp == 2 && (im.vsamp == 1 || im.vsamp == 2)));
    if (!samp_ok) { poco_set_error(who + "components / sampling must be 1 (1x1) or 3 with luma 1x1, 2x1 or 2x2"); return POCO_ERR_ARG; }
    if (im.nscan < 1 || im.nscan > JP_MAX_SCANS || im.ntable < 0 || im.ntable > 256 || im.nbytes > ((size_t)1 << 30)) {
      poco_set_error(who + "scans outside 1 .. 64, tables outside 0 .. 256 or more than 2^30 bytes");
      return POCO_ERR_ARG;
    }
    DImg& d = dim[i];
    std::memset(&d, 0, offsetof(DImg, tab));          // (tab is not read by the kernels this decoder launches, and not copied)
    d.H = im.H; d.W = im.W; d.ncomp = im.ncomp; d.hs = im.hsamp; d.vs = im.vsamp;
    d.bpm = im.ncomp == 1 ? 1 : im.hsamp * im.vsamp + 2;
    d.mcux = (im.W + 8 * im.hsamp - 1) / (8 * im.hsamp);
    d.mcuy = (im.H + 8 * im.vsamp - 1) / (8 * im.vsamp);
    d.nblocks = (int)((long long)d.mcux * d.mcuy * d.bpm);
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
    }
    if ((size_t)d.nblocks > dec->blocks_per_image) { poco_set_error(who + "more blocks than planned"); return POCO_ERR_STATE; }
    nblocks += d.nblocks;
    d.data_off = (unsigned)nbytes;          // relative to the bytes region, made absolute below
    d.nbytes = (unsigned)im.nbytes;
    nbytes += align_up(im.nbytes, 16);
    // the scan script: jdphuff.c's rules, and every scan's level
    int bits[3][64], lvl[3][64], built[2][256];
    for (int c = 0; c < 3; ++c) for (int k = 0; k < 64; ++k) { bits[c][k] = -1; lvl[c][k] = -1; }
    for (int k = 0; k < 256; ++k) built[0][k] = built[1][k] = -1;
    const size_t tabs0 = tabs.size();
    for (int s = 0; s < im.nscan; ++s) {
      const poco_jpeg_prog_scan& sc = im.scans[s];
      const std::string ws = who + "scan " + std::to_string(s) + ": ";
      const bool dc = sc.ss == 0;
      bool ok = (sc.ncomp == 1 || (sc.ncomp == im.ncomp && dc)) && (dc ? sc.se == 0 : (sc.se >= sc.ss && sc.se <= 63)) && sc.al <= 13 &&
                (sc.ah == 0 || sc.ah == sc.al + 1) && (size_t)sc.offset + sc.length <= im.nbytes;
      for (int k = 0; ok && k < sc.ncomp; ++k) ok = sc.ncomp == 1 ? sc.comp[k] < im.ncomp : sc.comp[k] == k;
      if (!ok) { poco_set_error(ws + "components, band, successive approximation or bytes outside what a progressive scan may have"); return POCO_ERR_ARG; }
      PScan p{};
      p.off = sc.offset; p.len = sc.length; p.img = i;
      p.ncomp = sc.ncomp; p.comp = sc.comp[0]; p.ss = sc.ss; p.se = sc.se; p.ah = sc.ah; p.al = sc.al;
      int lv = 0;
      for (int k = 0; k < sc.ncomp; ++k) {
        const int c = sc.comp[k];
        for (int z = sc.ss; z <= sc.se; ++z) {
          if (bits[c][z] != (sc.ah ? (int)sc.ah : -1) || (!dc && bits[c][0] < 0)) {
            poco_set_error(ws + "a first scan of coefficients sent before, a refinement that does not follow Al = Ah, or AC before DC");
            return POCO_ERR_ARG;
          }
          bits[c][z] = sc.al;
          lv = std::max(lv, lvl[c][z] + 1);
        }
      }
      for (int k = 0; k < sc.ncomp; ++k)
        for (int z = sc.ss; z <= sc.se; ++z) lvl[sc.comp[k]][z] = lv;
      const int ntab = dc ? (sc.ah == 0 ? sc.ncomp : 0) : 1;
      for (int k = 0; k < ntab; ++k) {
        const int t = sc.tab[k];
        if (t < 0 || t >= im.ntable) { poco_set_error(ws + "a table index outside tables[]"); return POCO_ERR_ARG; }
        int& g = built[dc ? 0 : 1][t];
        if (g < 0) {
          HuffTab ht;
          if (!build_table(im.tables[t].bits, im.tables[t].vals, dc, &ht)) {
            poco_set_error(ws + "a Huffman table is no prefix code (or a DC category is above 15)");
            return POCO_ERR_ARG;
          }
          g = (int)tabs.size();
          tabs.push_back(ht);
        }
        p.tab[k] = g;
      }
      scans.push_back(p);
      level.push_back(lv);
      nlevels = std::max(nlevels, lv + 1);
    }
    for (int c = 0; c < im.ncomp; ++c)
      for (int z = 0; z < 64; ++z)
        if (bits[c][z] < 0) { poco_set_error(who + "a coefficient no scan sends"); return POCO_ERR_ARG; }
    // libjpeg smooths the blocks of a picture whose low AC coefficients have not reached Al = 0 (jdcoefct.c); this decoder does not, so
    // such a script is not taken.  A file CUT SHORT inside such a script is taken, and is damaged whatever its last scan decodes to.
    bool above = false;
    for (int c = 0; c < im.ncomp; ++c)
      for (int z = 0; z < 64; ++z) above = above || bits[c][z] > 0;
    if (above) {
      if (!(im.scans[im.nscan - 1].flags & POCO_JPEG_PROG_SCAN_CUT)) {
        poco_set_error(who + "the scan script ends with a coefficient above Al = 0 (libjpeg smooths such pictures; decode them with it)");
        return POCO_ERR_ARG;
      }
      cut_short.push_back(i);
    }
    if (tabs.size() - tabs0 > (size_t)JP_TABS_PER_IMAGE) {
      poco_set_error(who + "more than " + std::to_string(JP_TABS_PER_IMAGE) + " Huffman tables");
      return POCO_ERR_ARG;
    }
    max_idct = std::max(max_idct, (d.nblocks + 31) / 32);
    max_dwords = std::max(max_dwords, (3ll * im.H * im.W + 3 + 3) / 4);
  }
  // scans by level: launch l takes level_off[l] .. level_off[l + 1]
  std::vector<int> level_off(nlevels + 1, 0);
  for (int lv : level) ++level_off[lv + 1];
  for (int l = 0; l < nlevels; ++l) level_off[l + 1] += level_off[l];
  std::vector<PScan> sorted(scans.size());
  {
    std::vector<int> at(level_off.begin(), level_off.end() - 1);
    for (size_t k = 0; k < scans.size(); ++k) sorted[at[level[k]]++] = scans[k];
  }
  const size_t img_bytes = align_up((size_t)n * sizeof(DImg), 16), scan_bytes = sorted.size() * sizeof(PScan),
               tab_bytes = align_up(tabs.size() * sizeof(HuffTab), 16);
  const size_t used = img_bytes + scan_bytes + tab_bytes + nbytes + 16;
  if (nbytes > dec->max_bytes + (size_t)n * 16 || used > dec->blob_cap) {
    poco_set_error("poco_jpeg_prog_decode: " + std::to_string(nbytes) + " bytes exceed what the decoder was created for (max_bytes " +
                   std::to_string(dec->max_bytes) + ")");
    return POCO_ERR_ARG;
  }
  const hipStream_t s = (hipStream_t)stream;
  // the staging buffer is free once the previous call's copy has left it
  if (dec->in_flight) POCO_HIP_CHECK(hipEventSynchronize(dec->copied));
  const size_t data0 = img_bytes + scan_bytes + tab_bytes;
  for (int i = 0; i < n; ++i) {
    dim[i].data_off += (unsigned)data0;
    std::memcpy(dec->h_blob + dim[i].data_off, imgs[i].data, imgs[i].nbytes);
    std::memset(dec->h_blob + dim[i].data_off + imgs[i].nbytes, 0, align_up(imgs[i].nbytes, 16) - imgs[i].nbytes);
    std::memcpy(dec->h_blob + (size_t)i * sizeof(DImg), &dim[i], sizeof(DImg));
  }
  std::memcpy(dec->h_blob + img_bytes, sorted.data(), scan_bytes);
  std::memcpy(dec->h_blob + img_bytes + scan_bytes, tabs.data(), tabs.size() * sizeof(HuffTab));
  std::memset(dec->h_blob + used - 16, 0, 16);
  POCO_HIP_CHECK(hipMemcpyAsync(dec->d_blob, dec->h_blob, used, hipMemcpyHostToDevice, s));
  POCO_HIP_CHECK(hipEventRecord(dec->copied, s));
  dec->in_flight = true;
  POCO_HIP_CHECK(hipMemsetAsync(d_status, 0, (size_t)n * sizeof(int), s));
  for (int i : cut_short) POCO_HIP_CHECK(hipMemsetD32Async((hipDeviceptr_t)(d_status + i), JD_ERR_SHORT, 1, s));
  POCO_HIP_CHECK(hipMemsetAsync(dec->coef, 0, nblocks * 64 * sizeof(short), s));
  const DImg* d_img = reinterpret_cast<const DImg*>(dec->d_blob);
  const PScan* d_scan = reinterpret_cast<const PScan*>(dec->d_blob + img_bytes);
  const HuffTab* d_tab = reinterpret_cast<const HuffTab*>(dec->d_blob + img_bytes + scan_bytes);
  for (int l = 0; l < nlevels; ++l) {
    const int cnt = level_off[l + 1] - level_off[l];
    if (cnt > 0) jprog_scan<<<cnt, JP_WAVE, 0, s>>>(dec->d_blob, d_img, d_scan + level_off[l], d_tab, dec->coef, d_status);
  }
  launch_idct_colour(d_img, n, dec->coef, dec->planes, max_idct, max_dwords, s);
  POCO_HIP_CHECK(hipGetLastError());
  return POCO_OK;
}

extern "C" void poco_jpeg_prog_decoder_destroy(poco_jpeg_prog_decoder_t dec) { delete dec; }
