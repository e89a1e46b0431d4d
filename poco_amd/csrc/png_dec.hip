// PNG decoder for the demo's input frames: the IDAT payloads of a batch of parsed files (poco_amd/png.py parse_png) -> one uint8
// [H,W,3] RGB picture per file on the device, the pixels of PIL's Image.open(f).convert("RGB").  The contract is stated in
// include/poco_hip.h and DESIGN.md 15; tests/pngdec_np.py restates it in numpy, pinned on zlib and PIL, and the GPU tests compare
// BYTES.  Integer arithmetic only.
//
// One host-to-device copy (descriptors, palettes, deflate streams from the pinned staging buffer), one memset, then on the stream:
//   pngd_inflate   one workgroup of four waves per image.  Lane 0 of wave 0 WALKS the symbols (the serial part): it reads the
//                  stream from a 32 KiB input ring in LDS, stores literals straight into the 64 KiB output ring in LDS and queues
//                  matches and stored pieces as tokens (output position, length, distance) in batches.  Wave 1 RESOLVES the
//                  batch before: the matches in order, each copied by the 64 lanes, dist < len by the modulo; the sources are
//                  LDS only.  Waves 2 and 3 FLUSH the batch before that to the image's filtered-stream scratch in whole dwords
//                  and refill the input ring.  One barrier per batch; at a block boundary the whole workgroup builds the two
//                  Huffman tables in LDS (counts by LDS atomics, canonical codes, a 10-bit lookup table + a sorted list for the
//                  longer codes); the code-length code and the run-length expansion are read by the walker.
//   pngd_unfilter  launched once per band of 64 rows, one wave per image: lane r undoes row y0 + r one pixel behind lane r - 1,
//                  the pixel above comes from the neighbouring lane, the row above the band from a carry row the launch before
//                  wrote (two buffers by band parity).  The same lane maps the pixel to RGB and stores it.
// Every loop is bounded by a constant or by a count the host validated; every LDS index is masked, every global index compared
// before use.  No global atomics: every word has one writer, except the status words, to which every writer stores a non-zero
// value.  No lane reads global memory that the same launch wrote.
#include "common.h"
#include "../../include/poco_hip.h"

#include <algorithm>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

namespace {

constexpr int PD_MAX_SIDE = 16384;
constexpr int PD_MAX_BATCH = 4096;
constexpr int PD_THREADS = 256;
constexpr unsigned PD_RING = 65536;        // output ring, bytes: a 32 KiB window + three batches in flight
constexpr unsigned PD_IN_DW = 8192;        // input ring, dwords
constexpr unsigned PD_NTOK = 1024;         // tokens per batch
constexpr unsigned PD_BATCH_OUT = 8192;    // a batch ends once it has produced this many bytes (+ at most one token more)
constexpr unsigned PD_PIECE = 1024;        // bytes of a stored block per token
constexpr unsigned PD_HEADER_DW = 200;     // dwords a block header may read: 17 + 57 + 316 x 14 bits = 562 bytes
constexpr int PD_TB = 10;                  // bits of the lookup tables
constexpr int PD_BAND = 64;                // rows per unfilter launch
enum { PD_ERR_CODE = 1, PD_ERR_SHORT = 2, PD_ERR_SIZE = 3, PD_ERR_FILTER = 4 };
enum { M_HEADER = 0, M_SYMS = 1, M_STORED = 2, M_REPOS = 3, M_DONE = 4 };

typedef unsigned long long u64;

struct PImg {
  unsigned char* out;           // H * W * 3 bytes
  u64 scr_off;                  // the image's filtered stream in the scratch, a multiple of 16
  unsigned data_off, nbytes;    // the deflate stream in the blob (data_off a multiple of 16) and its length
  unsigned padded;              // bytes of the blob that belong to the stream's slot (a multiple of 16, zeros behind nbytes)
  unsigned pal_off;             // 768 bytes of palette in the blob
  unsigned expect;              // H * (1 + bpp * W)
  unsigned max_iter;            // bound of the batch loop
  int H, W, ctype, bpp;
  unsigned pad[2];
};
static_assert(sizeof(PImg) == 64, "array of 16-byte aligned records");

__device__ __forceinline__ unsigned cl_order(int i) {      // RFC 1951 3.2.7: the order of the code-length code's lengths
  // 16 17 18 0 8 7 9 6 10 5 11 4 | 12 3 13 2 14 1 15, five bits each
  const u64 lo = 16ull | 17ull << 5 | 18ull << 10 | 0ull << 15 | 8ull << 20 | 7ull << 25 | 9ull << 30 | 6ull << 35 | 10ull << 40 |
                 5ull << 45 | 11ull << 50 | 4ull << 55;
  const u64 hi = 12ull | 3ull << 5 | 13ull << 10 | 2ull << 15 | 14ull << 20 | 1ull << 25 | 15ull << 30;
  return (unsigned)((i < 12 ? lo >> (5 * i) : hi >> (5 * (i - 12))) & 31);
}

__global__ __launch_bounds__(PD_THREADS) void pngd_inflate(const unsigned char* __restrict__ blob, const PImg* __restrict__ imgs,
                                                           unsigned char* __restrict__ scratch, int* __restrict__ status) {
  __shared__ unsigned s_out[PD_RING / 4];
  __shared__ unsigned s_in[PD_IN_DW];
  __shared__ unsigned s_tpos[2][PD_NTOK], s_tinfo[2][PD_NTOK], s_tsrc[2][PD_NTOK];
  __shared__ unsigned short s_tab[2][1 << PD_TB];      // (symbol << 4 | length) by the next PD_TB bits, 0 = no code this short
  __shared__ unsigned short s_sorted[2][320];          // symbols by (length, symbol): the codes longer than PD_TB bits
  __shared__ unsigned char s_lens[352];                // [0, nlit) literal/length, [nlit, nlit + ndist) distance code lengths
  __shared__ unsigned char s_cl[128];                  // the code-length code: symbol << 3 | length by the next 7 bits
  __shared__ int s_cnt[2][16], s_first[2][16], s_offs[2][16];
  __shared__ unsigned s_lentab[32], s_disttab[32];     // base | extra bits << 16
  __shared__ unsigned s_ntok[4], s_bend[4], s_inpos[4], s_build[4];
  __shared__ unsigned s_nlit, s_ndist, s_done, s_stat, s_builderr;

  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const PImg im = imgs[blockIdx.x];
  const unsigned nbytes = im.nbytes, expect = im.expect;
  const unsigned* in32 = reinterpret_cast<const unsigned*>(blob + im.data_off);
  const unsigned in_dw = im.padded >> 2;
  unsigned char* scr = scratch + im.scr_off;
  unsigned char* ring8 = reinterpret_cast<unsigned char*>(s_out);

  for (unsigned d = tid; d < PD_IN_DW; d += PD_THREADS) s_in[d] = d < in_dw ? in32[d] : 0u;
  if (tid < 32) {
    const int i = tid;
    unsigned eb = i < 8 ? 0 : (i >> 2) - 1, base = i < 8 ? 3 + i : 3 + ((4 + (i & 3)) << eb);
    if (i == 28) { eb = 0; base = 258; }
    s_lentab[i] = base | eb << 16;
    const unsigned de = i < 4 ? 0 : (i >> 1) - 1, db = i < 4 ? i + 1 : 1 + ((2 + (i & 1)) << de);
    s_disttab[i] = db | de << 16;
  }
  if (tid < 4) { s_ntok[tid] = 0; s_bend[tid] = 0; s_inpos[tid] = 0; s_build[tid] = 0; }
  if (tid == 0) { s_nlit = 0; s_ndist = 0; s_done = 0; s_stat = 0; s_builderr = 0; }
  __syncthreads();

  // the walker's registers (thread 0)
  u64 bb = 0;
  int nb = 0, mode = M_HEADER, bfinal = 0;
  unsigned qd = 0, out = 0, st_src = 0, st_left = 0, pub = 0;
  // every thread
  unsigned staged = PD_IN_DW, flushed = 0;

  for (unsigned it = 0; it < im.max_iter; ++it) {
    const unsigned inpos = s_inpos[it & 3];
    const unsigned load_hi = inpos + PD_IN_DW;
    if (wave == 0) {
      if (tid == 0) {
        unsigned ntok = 0, build = 0;
        const unsigned bstart = out;
        const int buf = it & 1;
        int fail = 0;
        if (mode != M_DONE && s_builderr) fail = PD_ERR_CODE;
#define PD_REFILL() do { if (nb <= 32) { bb |= (u64)s_in[qd & (PD_IN_DW - 1)] << nb; nb += 32; ++qd; } } while (0)
#define PD_DROP(n) do { bb >>= (n); nb -= (n); } while (0)
        bool stop = mode == M_DONE || fail;
        for (unsigned guard = 0; guard < 4 * PD_BATCH_OUT && !stop; ++guard) {
          if (qd > (nbytes >> 2) + 4) { fail = PD_ERR_SHORT; break; }
          if (mode == M_REPOS) {
            const unsigned rq = st_src >> 2;
            if (rq + 1 > staged) break;
            const int sh = (int)(st_src & 3) * 8;
            bb = (u64)(s_in[rq & (PD_IN_DW - 1)] >> sh);
            nb = 32 - sh;
            qd = rq + 1;
            mode = M_HEADER;
          } else if (mode == M_HEADER) {
            if (qd + PD_HEADER_DW > staged) break;
            PD_REFILL();
            bfinal = (int)(bb & 1);
            const int btype = (int)(bb >> 1) & 3;
            PD_DROP(3);
            if (btype == 3) { fail = PD_ERR_CODE; break; }
            if (btype == 0) {
              PD_DROP(nb & 7);
              PD_REFILL();
              const unsigned len = (unsigned)bb & 0xFFFFu, nlen = (unsigned)(bb >> 16) & 0xFFFFu;
              PD_DROP(32);
              if ((len ^ 0xFFFFu) != nlen) { fail = PD_ERR_CODE; break; }
              st_src = qd * 4 - (unsigned)(nb >> 3);
              if (st_src > nbytes) { fail = PD_ERR_SHORT; break; }
              st_left = len;
              mode = M_STORED;
            } else if (btype == 1) {
              build = 1;
              mode = M_SYMS;
              stop = true;
            } else {
              PD_REFILL();
              const unsigned hlit = ((unsigned)bb & 31) + 257, hdist = ((unsigned)(bb >> 5) & 31) + 1, hclen = ((unsigned)(bb >> 10) & 15) + 4;
              PD_DROP(14);
              if (hlit > 286 || hdist > 30) { fail = PD_ERR_CODE; break; }
              u64 cll = 0;                                   // the 19 lengths of the code-length code, three bits each
              for (unsigned i = 0; i < hclen; ++i) {
                PD_REFILL();
                cll |= (bb & 7) << (3 * cl_order((int)i));
                PD_DROP(3);
              }
              for (int j = 0; j < 32; ++j) reinterpret_cast<unsigned*>(s_cl)[j] = 0;
              unsigned code = 0, kraft = 0;
              for (int l = 1; l <= 7; ++l) {
                for (int sym = 0; sym < 19; ++sym) {
                  if ((int)((cll >> (3 * sym)) & 7) != l) continue;
                  kraft += 128u >> l;
                  for (unsigned j = __brev(code) >> (32 - l); j < 128; j += 1u << l) s_cl[j] = (unsigned char)(sym << 3 | l);
                  ++code;
                }
                code <<= 1;
              }
              if (kraft != 128) { fail = PD_ERR_CODE; break; }         // the code-length code must be complete
              const unsigned n = hlit + hdist;
              unsigned i = 0, prev = 0;
              for (unsigned g2 = 0; g2 < 320 && i < n; ++g2) {
                PD_REFILL();
                const unsigned e = s_cl[(unsigned)bb & 127];
                if (e == 0) { fail = PD_ERR_CODE; break; }
                PD_DROP((int)(e & 7));
                const unsigned sym = e >> 3;
                unsigned rep = 1, v = sym;
                if (sym == 16) {
                  if (i == 0) { fail = PD_ERR_CODE; break; }
                  rep = 3 + ((unsigned)bb & 3); PD_DROP(2); v = prev;
                } else if (sym == 17) {
                  rep = 3 + ((unsigned)bb & 7); PD_DROP(3); v = 0;
                } else if (sym == 18) {
                  rep = 11 + ((unsigned)bb & 127); PD_DROP(7); v = 0;
                }
                if (i + rep > n) { fail = PD_ERR_CODE; break; }
                for (unsigned r = 0; r < rep; ++r) s_lens[i++] = (unsigned char)v;
                prev = v;
              }
              if (fail) break;
              if (i != n || s_lens[256] == 0) { fail = PD_ERR_CODE; break; }       // no end-of-block code
              s_nlit = hlit;
              s_ndist = hdist;
              build = 2;
              mode = M_SYMS;
              stop = true;
            }
          } else if (mode == M_STORED) {
            if (st_left == 0) {
              if (bfinal) { mode = M_DONE; break; }
              mode = M_REPOS;
              continue;
            }
            if (ntok >= PD_NTOK || out - bstart >= PD_BATCH_OUT) break;
            const unsigned piece = st_left < PD_PIECE ? st_left : PD_PIECE;
            if (st_src + piece > nbytes) { fail = PD_ERR_SHORT; break; }
            if (piece > expect - out) { fail = PD_ERR_SIZE; break; }
            s_tpos[buf][ntok] = out;
            s_tinfo[buf][ntok] = 0x80000000u | piece;
            s_tsrc[buf][ntok] = st_src;
            ++ntok;
            out += piece;
            st_src += piece;
            st_left -= piece;
          } else {                                            // M_SYMS
            if (ntok >= PD_NTOK || out - bstart >= PD_BATCH_OUT || qd + 2 > staged) break;
            PD_REFILL();
            unsigned e = s_tab[0][(unsigned)bb & ((1u << PD_TB) - 1)];
            if (e == 0) {                                     // a code longer than PD_TB bits, or none
              const unsigned rev = __brev((unsigned)bb) >> 17;
              for (int l = PD_TB + 1; l <= 15; ++l) {
                const unsigned idx = (rev >> (15 - l)) - (unsigned)s_first[0][l];
                if (idx < (unsigned)s_cnt[0][l]) { e = (unsigned)s_sorted[0][(s_offs[0][l] + idx) % 320u] << 4 | l; break; }
              }
              if (e == 0) { fail = PD_ERR_CODE; break; }
            }
            PD_DROP((int)(e & 15));
            const unsigned sym = e >> 4;
            if (sym < 256) {
              if (out >= expect) { fail = PD_ERR_SIZE; break; }
              ring8[out & (PD_RING - 1)] = (unsigned char)sym;
              ++out;
            } else if (sym == 256) {
              if (bfinal) {
                if ((u64)qd * 32 - (u64)nb > (u64)nbytes * 8) fail = PD_ERR_SHORT;      // the block ended in the padding
                mode = M_DONE;
                break;
              }
              mode = M_HEADER;
            } else {
              if (sym >= 286) { fail = PD_ERR_CODE; break; }
              const unsigned lt = s_lentab[sym - 257];
              const unsigned len = (lt & 0xFFFF) + ((unsigned)bb & ((1u << (lt >> 16)) - 1));
              PD_DROP((int)(lt >> 16));
              PD_REFILL();
              unsigned f = s_tab[1][(unsigned)bb & ((1u << PD_TB) - 1)];
              if (f == 0) {
                const unsigned rev = __brev((unsigned)bb) >> 17;
                for (int l = PD_TB + 1; l <= 15; ++l) {
                  const unsigned idx = (rev >> (15 - l)) - (unsigned)s_first[1][l];
                  if (idx < (unsigned)s_cnt[1][l]) { f = (unsigned)s_sorted[1][(s_offs[1][l] + idx) % 320u] << 4 | l; break; }
                }
                if (f == 0) { fail = PD_ERR_CODE; break; }
              }
              PD_DROP((int)(f & 15));
              const unsigned dsym = f >> 4;
              if (dsym >= 30) { fail = PD_ERR_CODE; break; }
              const unsigned dt = s_disttab[dsym];
              const unsigned dist = (dt & 0xFFFF) + ((unsigned)bb & ((1u << (dt >> 16)) - 1));
              PD_DROP((int)(dt >> 16));
              if (dist > out) { fail = PD_ERR_CODE; break; }            // a distance beyond the bytes produced so far
              if (len > expect - out) { fail = PD_ERR_SIZE; break; }
              s_tpos[buf][ntok] = out;
              s_tinfo[buf][ntok] = len << 16 | dist;
              ++ntok;
              out += len;
            }
          }
        }
#undef PD_REFILL
#undef PD_DROP
        if (fail) { s_stat = (unsigned)fail; mode = M_DONE; }
        s_ntok[it & 3] = ntok;
        s_bend[it & 3] = out;
        s_build[it & 3] = fail ? 0u : build;
        // the oldest dword the walker may still read: the bit buffer holds at most two, a stored block is re-entered at st_src
        const unsigned oldest = (mode == M_REPOS || mode == M_STORED) ? st_src >> 2 : (qd > 2 ? qd - 2 : 0u);
        pub = oldest > pub ? oldest : pub;
        s_inpos[(it + 1) & 3] = pub;
        if (mode == M_DONE && s_done == 0) s_done = it + 1;
      }
    } else if (wave == 1) {
      if (it >= 1) {                                          // the tokens of the batch before, in order
        const int buf = (it - 1) & 1;
        const unsigned nt = min(s_ntok[(it - 1) & 3], PD_NTOK);
        volatile unsigned char* r8 = ring8;
        for (unsigned t = 0; t < nt; ++t) {
          const unsigned pos = s_tpos[buf][t], info = s_tinfo[buf][t];
          if (info & 0x80000000u) {
            const unsigned piece = min(info & 0xFFFFu, PD_PIECE), src = s_tsrc[buf][t];
            for (unsigned o = lane; o < piece; o += 64) {
              const unsigned q = src + o;
              r8[(pos + o) & (PD_RING - 1)] = q < nbytes ? blob[im.data_off + q] : (unsigned char)0;
            }
          } else {
            const unsigned len = min(info >> 16, 258u), dist = max(info & 0xFFFFu, 1u);
            for (unsigned o = lane; o < len; o += 64) {
              const unsigned k = o < dist ? o : o % dist;
              r8[(pos + o) & (PD_RING - 1)] = r8[(pos - dist + k) & (PD_RING - 1)];
            }
          }
          __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
          __builtin_amdgcn_wave_barrier();
        }
      }
    } else {
      const int ft = tid - 128;
      if (it >= 2) {                                          // the bytes the batch before the last finished, in whole dwords
        const unsigned hi = min(s_bend[(it - 2) & 3], expect) & ~3u;
        for (unsigned p = flushed + 4 * ft; p < hi; p += 4 * 128)
          *reinterpret_cast<unsigned*>(scr + p) = s_out[(p & (PD_RING - 1)) >> 2];
      }
      for (unsigned d = max(staged, inpos) + ft; d < load_hi; d += 128) s_in[d & (PD_IN_DW - 1)] = d < in_dw ? in32[d] : 0u;
    }
    if (it >= 2) flushed = max(flushed, min(s_bend[(it - 2) & 3], expect) & ~3u);
    staged = load_hi;
    __syncthreads();

    const unsigned build = s_build[it & 3];
    if (build) {                                              // uniform: the whole workgroup builds the block's tables
      unsigned nlit = s_nlit, ndist = s_ndist;
      if (build == 1) {
        nlit = 288;
        ndist = 32;
        for (int t = tid; t < 320; t += PD_THREADS) s_lens[t] = (unsigned char)(t < 144 ? 8 : t < 256 ? 9 : t < 280 ? 7 : t < 288 ? 8 : 5);
      }
      nlit = min(nlit, 288u);
      ndist = min(ndist, 32u);
      for (int t = tid; t < (2 << PD_TB) / 2; t += PD_THREADS) reinterpret_cast<unsigned*>(&s_tab[0][0])[t] = 0;
      if (tid < 32) (&s_cnt[0][0])[tid] = 0;
      __syncthreads();
      for (unsigned t = tid; t < nlit + ndist; t += PD_THREADS) {
        const int l = s_lens[t] & 15;
        if (l) atomicAdd(&s_cnt[t >= nlit][l], 1);
      }
      __syncthreads();
      if (tid < 2) {
        int code = 0, off = 0, kraft = 0;
        s_first[tid][0] = 0;
        s_offs[tid][0] = 0;
        for (int l = 1; l <= 15; ++l) {
          s_first[tid][l] = code;
          s_offs[tid][l] = off;
          const int c = s_cnt[tid][l];
          code = (code + c) << 1;
          off += c;
          kraft += c << (15 - l);
        }
        // complete, or a single code of one bit, or (distances only) no code at all
        const bool ok = kraft == 32768 || (off == 1 && s_cnt[tid][1] == 1) || (tid == 1 && off == 0);
        if (!ok) s_builderr = 1;
      }
      __syncthreads();
      for (unsigned t = tid; t < nlit + ndist; t += PD_THREADS) {
        const int which = t >= nlit, l = s_lens[t] & 15;
        if (!l) continue;
        const unsigned lo = which ? nlit : 0u, sym = t - lo;
        int rank = 0;
        for (unsigned s = lo; s < t; ++s) rank += (s_lens[s] & 15) == l;
        s_sorted[which][(unsigned)(s_offs[which][l] + rank) % 320u] = (unsigned short)sym;
        if (l <= PD_TB) {
          const unsigned code = (unsigned)(s_first[which][l] + rank);
          for (unsigned j = __brev(code) >> (32 - l); j < (1u << PD_TB); j += 1u << l) s_tab[which][j] = (unsigned short)(sym << 4 | l);
        }
      }
      __syncthreads();
    }
    const unsigned done = s_done;
    if (done != 0 && it >= done - 1 + 2) break;
  }
  __syncthreads();
  const unsigned end = min(s_bend[0] > s_bend[1] ? s_bend[0] : s_bend[1], expect);      // positions only grow: the largest is the last
  const unsigned end2 = min(s_bend[2] > s_bend[3] ? s_bend[2] : s_bend[3], expect);
  const unsigned fin = end > end2 ? end : end2;
  for (unsigned p = flushed + tid; p < fin; p += PD_THREADS) scr[p] = ring8[p & (PD_RING - 1)];
  if (tid == 0) {
    unsigned st = s_stat;
    if (st == 0 && s_done == 0) st = PD_ERR_SHORT;           // the batch loop ran out
    if (st == 0 && fin != expect) st = PD_ERR_SIZE;
    if (st) status[blockIdx.x] = (int)st;
  }
}

__device__ __forceinline__ unsigned unfilter_px(unsigned raw, unsigned a, unsigned b, unsigned c, int ft) {
  unsigned res = 0;
  #pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int x = (int)(raw >> (8 * k)) & 255, ak = (int)(a >> (8 * k)) & 255, bk = (int)(b >> (8 * k)) & 255, ck = (int)(c >> (8 * k)) & 255;
    int p = 0;
    if (ft == 1) p = ak;
    else if (ft == 2) p = bk;
    else if (ft == 3) p = (ak + bk) >> 1;
    else if (ft == 4) {
      const int pa = abs(bk - ck), pb = abs(ak - ck), pc = abs(ak + bk - 2 * ck);
      p = (pa <= pb && pa <= pc) ? ak : (pb <= pc ? bk : ck);
    }
    res |= (unsigned)((x + p) & 255) << (8 * k);
  }
  return res;
}

__global__ __launch_bounds__(64) void pngd_unfilter(const unsigned char* __restrict__ blob, const PImg* __restrict__ imgs,
                                                    const unsigned char* __restrict__ scratch, unsigned* __restrict__ carry,
                                                    unsigned carry_stride, int band, int* __restrict__ status) {
  const PImg im = imgs[blockIdx.x];
  const int H = im.H, W = im.W, bpp = im.bpp, ctype = im.ctype;
  const int y0 = band * PD_BAND;
  if (y0 >= H) return;
  const int r = threadIdx.x, y = y0 + r;
  const bool rowok = y < H;
  const size_t stride = 1 + (size_t)bpp * W;
  const unsigned char* row = scratch + im.scr_off + (size_t)(rowok ? y : y0) * stride;
  int ft = row[0];
  if (rowok && ft > 4) status[blockIdx.x] = PD_ERR_FILTER;
  if (!rowok || ft > 4) ft = 0;
  unsigned* cbase = carry + (size_t)blockIdx.x * 2 * carry_stride;
  const unsigned* cin = cbase + (size_t)((band + 1) & 1) * carry_stride;      // written by the launch of the band above
  unsigned* cout = cbase + (size_t)(band & 1) * carry_stride;
  const unsigned char* pal = blob + im.pal_off;
  unsigned char* dst = im.out + (size_t)(rowok ? y : y0) * W * 3;
  const bool from_carry = r == 0 && band > 0;

  auto fetch = [&](int s) -> unsigned {
    const int px = s - r;
    if (!rowok || px < 0 || px >= W) return 0u;
    const unsigned char* p = row + 1 + (size_t)px * bpp;
    unsigned v = p[0];
    if (bpp > 1) v |= (unsigned)p[1] << 8;
    if (bpp > 2) v |= (unsigned)p[2] << 16;
    if (bpp > 3) v |= (unsigned)p[3] << 24;
    return v;
  };
  auto fetch_up = [&](int s) -> unsigned { return from_carry && s < W && s < (int)carry_stride ? cin[s] : 0u; };

  constexpr int G = 8;
  unsigned raw[G], cu[G];
  #pragma unroll
  for (int j = 0; j < G; ++j) { raw[j] = fetch(j); cu[j] = fetch_up(j); }
  unsigned left = 0, upprev = 0;
  const int nsteps = W + PD_BAND - 1;
  for (int s0 = 0; s0 < nsteps; s0 += G) {
    unsigned nraw[G], ncu[G];
    #pragma unroll
    for (int j = 0; j < G; ++j) { nraw[j] = fetch(s0 + G + j); ncu[j] = fetch_up(s0 + G + j); }
    #pragma unroll
    for (int j = 0; j < G; ++j) {
      const int px = s0 + j - r;
      unsigned up = __shfl_up(left, 1);                      // the lane above finished this column one step ago
      if (r == 0) up = cu[j];
      if (rowok && px >= 0 && px < W) {
        const unsigned cur = unfilter_px(raw[j], px > 0 ? left : 0u, up, px > 0 ? upprev : 0u, ft);
        unsigned R = cur & 255, Gc = (cur >> 8) & 255, B = (cur >> 16) & 255;
        if (ctype == 0 || ctype == 4) {
          Gc = B = R;
        } else if (ctype == 3) {
          const unsigned char* e = pal + 3 * R;              // R <= 255: inside the 768 zero-padded bytes
          R = e[0]; Gc = e[1]; B = e[2];
        }
        unsigned char* o = dst + (size_t)px * 3;
        o[0] = (unsigned char)R; o[1] = (unsigned char)Gc; o[2] = (unsigned char)B;
        if (r == PD_BAND - 1 && px < (int)carry_stride) cout[px] = cur;
        left = cur;
      }
      upprev = up;
    }
    #pragma unroll
    for (int j = 0; j < G; ++j) { raw[j] = nraw[j]; cu[j] = ncu[j]; }
  }
}

size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

int bpp_of(int ctype) { return ctype == 0 ? 1 : ctype == 2 ? 3 : ctype == 3 ? 1 : ctype == 4 ? 2 : ctype == 6 ? 4 : 0; }

}  // namespace

struct poco_png_decoder {
  int max_h = 0, max_w = 0, max_batch = 0;
  size_t max_bytes = 0, blob_cap = 0, scr_per_image = 0;
  unsigned char* h_blob = nullptr;         // pinned staging
  unsigned char* d_blob = nullptr;
  unsigned char* scratch = nullptr;        // the filtered streams
  unsigned* carry = nullptr;               // [max_batch][2][max_w]
  hipEvent_t copied = nullptr;
  bool in_flight = false;
  ~poco_png_decoder() {
    if (h_blob) (void)hipHostFree(h_blob);
    for (void* p : {(void*)d_blob, (void*)scratch, (void*)carry})
      if (p) (void)hipFree(p);
    if (copied) (void)hipEventDestroy(copied);
  }
};

extern "C" int poco_png_decoder_create(int max_h, int max_w, int max_batch, size_t max_bytes, poco_png_decoder_t* out) {
  if (!out) { poco_set_error("poco_png_decoder_create: null handle pointer"); return POCO_ERR_ARG; }
  *out = nullptr;
  if (max_h < 1 || max_w < 1 || max_h > PD_MAX_SIDE || max_w > PD_MAX_SIDE || max_batch < 1 || max_batch > PD_MAX_BATCH ||
      max_bytes < 1 || max_bytes > ((size_t)1 << 30)) {
    poco_set_error("poco_png_decoder_create: bad arguments (need 1 <= max_h, max_w <= 16384, 1 <= max_batch <= 4096, "
                   "1 <= max_bytes <= 2^30)");
    return POCO_ERR_ARG;
  }
  auto d = std::make_unique<poco_png_decoder>();
  d->max_h = max_h;
  d->max_w = max_w;
  d->max_batch = max_batch;
  d->max_bytes = max_bytes;
  d->scr_per_image = align_up((size_t)max_h * (1 + 4 * (size_t)max_w), 16);
  d->blob_cap = (size_t)max_batch * (sizeof(PImg) + 768 + 32) + align_up(max_bytes, 16) + 16;
  POCO_HIP_CHECK(hipHostMalloc((void**)&d->h_blob, d->blob_cap, hipHostMallocDefault));
  POCO_HIP_CHECK(hipMalloc(&d->d_blob, d->blob_cap));
  POCO_HIP_CHECK(hipMalloc(&d->scratch, d->scr_per_image * max_batch));
  POCO_HIP_CHECK(hipMalloc(&d->carry, (size_t)max_batch * 2 * max_w * sizeof(unsigned)));
  POCO_HIP_CHECK(hipEventCreateWithFlags(&d->copied, hipEventDisableTiming));
  *out = d.release();
  return POCO_OK;
}

extern "C" int poco_png_decode(poco_png_decoder_t dec, const poco_png_image* imgs, int n, int* d_status, void* stream) {
  if (!dec || !imgs || !d_status) { poco_set_error("poco_png_decode: null handle or pointer"); return POCO_ERR_ARG; }
  if (n < 1 || n > dec->max_batch) {
    poco_set_error("poco_png_decode: " + std::to_string(n) + " images, the decoder was created for 1 .. " + std::to_string(dec->max_batch));
    return POCO_ERR_ARG;
  }
  // ---- validate and lay out, before the staging buffer or the GPU is touched
  std::vector<PImg> dim(n);
  std::vector<size_t> total(n);
  size_t nbytes = 0, scr = 0;
  int max_h = 0;
  for (int i = 0; i < n; ++i) {
    const poco_png_image& im = imgs[i];
    const std::string who = "poco_png_decode: image " + std::to_string(i) + ": ";
    if (!im.data || !im.idat || !im.d_rgb) { poco_set_error(who + "null pointer"); return POCO_ERR_ARG; }
    if (im.H < 1 || im.W < 1 || im.H > dec->max_h || im.W > dec->max_w) {
      poco_set_error(who + std::to_string(im.H) + " x " + std::to_string(im.W) + " outside 1 x 1 .. " + std::to_string(dec->max_h) +
                     " x " + std::to_string(dec->max_w) + " (the size the decoder was created for)");
      return POCO_ERR_ARG;
    }
    const int bpp = bpp_of(im.colour_type);
    if (!bpp) { poco_set_error(who + "colour type " + std::to_string(im.colour_type) + " is none of 0, 2, 3, 4, 6"); return POCO_ERR_ARG; }
    if (im.nidat < 1) { poco_set_error(who + "no IDAT payload"); return POCO_ERR_ARG; }
    size_t sum = 0;
    for (int k = 0; k < im.nidat; ++k) {
      const size_t off = im.idat[2 * k], len = im.idat[2 * k + 1];
      if (off + len > im.nbytes) { poco_set_error(who + "IDAT payload " + std::to_string(k) + " lies outside the file"); return POCO_ERR_ARG; }
      sum += len;
    }
    if (sum < 6 || sum > ((size_t)1 << 30)) { poco_set_error(who + "the IDAT payloads hold fewer than 6 bytes or more than 2^30"); return POCO_ERR_ARG; }
    total[i] = sum;
    PImg& d = dim[i];
    std::memset(&d, 0, sizeof(PImg));
    d.out = im.d_rgb;
    d.H = im.H; d.W = im.W; d.ctype = im.colour_type; d.bpp = bpp;
    d.nbytes = (unsigned)(sum - 6);
    d.padded = (unsigned)(align_up(d.nbytes, 16) + 16);
    d.expect = (unsigned)((size_t)im.H * (1 + (size_t)bpp * im.W));
    // batches: each makes 3 bytes per token, reads input or ends a block; blocks and idle turns are counted by the stream's bytes
    d.max_iter = d.expect / 2048 + 2 * d.nbytes + 64;
    d.scr_off = scr;
    d.data_off = (unsigned)nbytes;
    scr += align_up(d.expect, 16);
    nbytes += d.padded;
    max_h = std::max(max_h, im.H);
  }
  const size_t img_bytes = (size_t)n * sizeof(PImg), pal_bytes = (size_t)n * 768;
  const size_t used = img_bytes + pal_bytes + nbytes;
  if (nbytes > dec->max_bytes + (size_t)n * 32 || used > dec->blob_cap || scr > dec->scr_per_image * dec->max_batch) {
    poco_set_error("poco_png_decode: " + std::to_string(nbytes) + " bytes of deflate streams exceed what the decoder was created for "
                   "(max_bytes " + std::to_string(dec->max_bytes) + ")");
    return POCO_ERR_ARG;
  }
  const hipStream_t s = (hipStream_t)stream;
  // the staging buffer is free once the previous call's copy has left it
  if (dec->in_flight) POCO_HIP_CHECK(hipEventSynchronize(dec->copied));
  for (int i = 0; i < n; ++i) {
    PImg& d = dim[i];
    d.pal_off = (unsigned)(img_bytes + (size_t)i * 768);
    d.data_off += (unsigned)(img_bytes + pal_bytes);
    std::memcpy(dec->h_blob + d.pal_off, imgs[i].palette, 768);
    // the payloads end to end, without the 2-byte zlib header and the 4-byte Adler-32
    unsigned char* dst = dec->h_blob + d.data_off;
    size_t skip = 2, left = total[i] - 6;
    for (int k = 0; k < imgs[i].nidat && left; ++k) {
      size_t off = imgs[i].idat[2 * k], len = imgs[i].idat[2 * k + 1];
      const size_t sk = std::min(skip, len);
      off += sk; len -= sk; skip -= sk;
      const size_t take = std::min(len, left);
      std::memcpy(dst, imgs[i].data + off, take);
      dst += take;
      left -= take;
    }
    std::memset(dst, 0, d.padded - d.nbytes);
  }
  std::memcpy(dec->h_blob, dim.data(), img_bytes);
  POCO_HIP_CHECK(hipMemcpyAsync(dec->d_blob, dec->h_blob, used, hipMemcpyHostToDevice, s));
  POCO_HIP_CHECK(hipEventRecord(dec->copied, s));
  dec->in_flight = true;
  POCO_HIP_CHECK(hipMemsetAsync(d_status, 0, (size_t)n * sizeof(int), s));
  const PImg* d_img = reinterpret_cast<const PImg*>(dec->d_blob);
  pngd_inflate<<<n, PD_THREADS, 0, s>>>(dec->d_blob, d_img, dec->scratch, d_status);
  for (int band = 0; band * PD_BAND < max_h; ++band)
    pngd_unfilter<<<n, 64, 0, s>>>(dec->d_blob, d_img, dec->scratch, dec->carry, (unsigned)dec->max_w, band, d_status);
  POCO_HIP_CHECK(hipGetLastError());
  return POCO_OK;
}

extern "C" void poco_png_decoder_destroy(poco_png_decoder_t dec) { delete dec; }
