// PNG encoder for the demo's rendered frames: uint8 [H,W,3] RGB on the device -> the bytes of a .png file on the device.
// The contract is stated in include/poco_hip.h and DESIGN.md 14; tests/png_np.py restates it in numpy and the GPU tests compare
// BYTES.  In short:
//   container  signature, IHDR (8 bit, colour type 2, no interlace), one IDAT per segment, IEND, nothing else
//   filters    per row the one of the five PNG filters (bpp 3) with the smallest sum of |signed byte| (libpng's heuristic), ties
//              to the lowest type; the row above the first is zeros
//   segments   the filtered stream H x (1 + 3W) is cut every 32 768 bytes; a segment is coded on its own (no match leaves it, own
//              Huffman tables) as one deflate block, BFINAL 0: dynamic, or stored when the dynamic block would be longer than
//              5 + n bytes.  Behind every block an empty stored block (000, pad, 00 00 FF FF; BFINAL 1 after the last segment)
//              puts the next segment on a byte boundary
//   matches    candidates of position p: p - 3, p - (1 + 3W) and the largest q < p - p % 1024 with the same 13-bit hash of 4 bytes
//              (hash table of positions filled chunk by chunk with an LDS atomicMax: order-independent); longest wins, ties to
//              the smallest distance, at most min(258, n - p), none below 3; greedy parse from the segment start
//   codes      symbols sorted by (count, symbol), two-queue merge (leaf first on equal weight), lengths above 15 repaired on the
//              counts per length (count[15] -= 1, the longest shorter length in use gives one code that becomes two, until Kraft
//              holds), lengths handed out by rank, canonical codes; HLIT 286, HDIST 30, HCLEN 19, the fixed complete code-length
//              code (0..12 in 4 bits, 13..18 in 5), all 316 lengths sent literally
//   framing    78 01 in front, Adler-32 (per-segment partial sums, combined) behind, CRC-32 per chunk (lanes over slices,
//              combined by multiplication by x^(8n) mod P)
//
// Three launches per call, all on the caller's stream, into scratch planned at create:
//   png_filter   per row: the five sums, the choice, the filtered row
//   png_segment  per segment (1024 lanes, the segment staged in LDS): matches per chunk, the greedy walk, histogram, the two codes,
//                bits behind prefix sums assembled in LDS -> the segment's slot (n + 10 bytes at most), its length, its Adler sums
//   png_compact  per segment: prefix sum of the lengths, IDAT header, copy, CRC; the first writes signature + IHDR, the last the
//                Adler-32, IEND and the total length
// No global atomics: every output byte has one writer.
#include "block_prims.h"
#include "common.h"
#include "../../include/poco_hip.h"

#include <cstring>
#include <memory>
#include <string>

namespace {

constexpr int PNG_MAX_SIDE = 16384;
constexpr int SEG = 32768;                      // bytes of the filtered stream per segment
constexpr int CHUNK = 1024;                     // positions per round: of the match finder and of the bit emission
constexpr int HASH_BITS = 13;
constexpr int MAX_MATCH = 258;
constexpr int SLOT = SEG + 32;                  // a segment's blocks take n + 10 bytes at most; + a spare dword for the copy
constexpr unsigned ADLER_MOD = 65521;
constexpr unsigned CRC_POLY = 0xEDB88320u;
constexpr int NLIT = 286, NDIST = 30, DOFF = 288, NSYM = DOFF + 32;      // litlen symbols at [0, 286), distance symbols at [288, 318)

size_t png_stream_bytes(int H, int W) { return (size_t)H * (1 + 3 * (size_t)W); }
size_t png_segments(int H, int W) { return (png_stream_bytes(H, W) + SEG - 1) / SEG; }
// signature 8 + IHDR 25 + IEND 12 + zlib header 2 + Adler 4 + the stream + per segment (5 + 5 of its blocks, 12 of its chunk)
size_t png_worst_case(int H, int W) { return 51 + png_stream_bytes(H, W) + 22 * png_segments(H, W); }

// ---- step 1: row filters ----------------------------------------------------------------------------------------------------------
constexpr int FL_THREADS = 256;

__device__ __forceinline__ int paeth(int a, int b, int c) {
  const int p = a + b - c, pa = abs(p - a), pb = abs(p - b), pc = abs(p - c);
  return (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
}

__device__ __forceinline__ int predictor(int t, int a, int b, int c) {
  return t == 0 ? 0 : t == 1 ? a : t == 2 ? b : t == 3 ? (a + b) >> 1 : paeth(a, b, c);
}

__global__ __launch_bounds__(FL_THREADS) void png_filter(const unsigned char* __restrict__ rgb, int H, int W,
                                                         unsigned char* __restrict__ filt) {
  __shared__ unsigned part[FL_THREADS / 64][5];
  const int tid = threadIdx.x, y = blockIdx.x, n = 3 * W;
  const unsigned char* cur = rgb + (size_t)y * n;
  const unsigned char* up = rgb + (size_t)(y > 0 ? y - 1 : 0) * n;         // (not read for the first row)
  unsigned s[5] = {0, 0, 0, 0, 0};
  for (int i = tid; i < n; i += FL_THREADS) {
    const int x = cur[i], a = i >= 3 ? cur[i - 3] : 0, b = y ? up[i] : 0, c = (y && i >= 3) ? up[i - 3] : 0;
    #pragma unroll
    for (int t = 0; t < 5; ++t) {
      const int v = (x - predictor(t, a, b, c)) & 255;
      s[t] += v < 128 ? v : 256 - v;
    }
  }
  #pragma unroll
  for (int t = 0; t < 5; ++t) {
    #pragma unroll
    for (int d = 32; d >= 1; d >>= 1) s[t] += __shfl_xor(s[t], d);
    if ((tid & 63) == 0) part[tid >> 6][t] = s[t];
  }
  __syncthreads();
  int best = 0;
  unsigned best_sum = 0;
  #pragma unroll
  for (int t = 0; t < 5; ++t) {
    unsigned tot = 0;
    #pragma unroll
    for (int w = 0; w < FL_THREADS / 64; ++w) tot += part[w][t];
    if (t == 0 || tot < best_sum) { best = t; best_sum = tot; }          // ties stay with the lowest type
  }
  unsigned char* out = filt + (size_t)y * (n + 1);
  if (tid == 0) out[0] = (unsigned char)best;
  for (int i = tid; i < n; i += FL_THREADS) {
    const int x = cur[i], a = i >= 3 ? cur[i - 3] : 0, b = y ? up[i] : 0, c = (y && i >= 3) ? up[i - 3] : 0;
    out[1 + i] = (unsigned char)(x - predictor(best, a, b, c));
  }
}

// ---- step 2: segment coding -------------------------------------------------------------------------------------------------------
constexpr int SG_THREADS = 1024;
constexpr int SG_WAVES = SG_THREADS / 64;
constexpr int BITS_WORDS = CHUNK * 48 / 32 + 4;          // a round: 1024 tokens of at most 48 bits, the carried byte, the trailer
// LDS carve-up (bytes).  The bit buffer of the emission rounds lies over the hash table, which is dead by then.
constexpr int L_SEG = 0;                                  // the segment + 16 zero bytes
constexpr int L_TOK = L_SEG + SEG + 16;                   // uint16 per position: 0 not a token start, 1 literal, 3..258 match length
constexpr int L_HASH = L_TOK + 2 * SEG + 16;              //   (the distance | 0x8000 in the next entry)
constexpr int L_CL = L_HASH + (4 << HASH_BITS);           // best length / distance of the chunk's positions
constexpr int L_CD = L_CL + 2 * CHUNK;
constexpr int L_HIST = L_CD + 2 * CHUNK;                  // uint32 [NSYM] counts, code lengths, codes
constexpr int L_LEN = L_HIST + 4 * NSYM;
constexpr int L_CODE = L_LEN + 4 * NSYM;
constexpr int L_WORK = L_CODE + 4 * NSYM;                 // the Huffman construction's arrays
constexpr int L_END = L_WORK + 4 * 6 * 288 + 4 * 64;
static_assert((4 << HASH_BITS) >= 4 * BITS_WORDS, "the bit buffer lies over the hash table");
static_assert(L_END <= 160 * 1024, "LDS of a gfx950 CU");

struct HuffWork {
  unsigned* ord;      // [288] symbol by rank
  unsigned* wt;       // [288] its count
  unsigned* iw;       // [288] weights of the internal nodes in the order made
  unsigned* ipar;     // [288] parent of an internal node
  unsigned* lpar;     // [288] parent of a leaf
  unsigned* lenr;     // [288] depth of an internal node, then length by rank
  unsigned* misc;     // [64]  counts per length [0..15], first code per length [16..31], wave sums [32..47], scalars [48..]
};

__device__ __forceinline__ unsigned block_sum(unsigned v, unsigned* wsum) {
  unsigned total;
  (void)block_exscan<SG_WAVES>(v, wsum, &total);
  return total;
}

// Four bytes of the staged segment from any byte offset: two aligned LDS dwords, byte-aligned.
__device__ __forceinline__ unsigned load4(const unsigned* seg, unsigned at) {
  const unsigned lo = seg[at >> 2], hi = seg[(at >> 2) + 1];
  return (unsigned)((((unsigned long long)hi << 32) | lo) >> (8 * (at & 3)));
}

// Equal bytes from (q, p) on, at most room.
__device__ __forceinline__ int match_length(const unsigned* seg, int q, int p, int room) {
  int l = 0;
  while (l < room) {
    const unsigned x = load4(seg, q + l) ^ load4(seg, p + l);
    if (x) { l += (__ffs(x) - 1) >> 3; break; }
    l += 4;
  }
  return min(l, room);
}

// (symbol, number of extra bits, their value) of a match length 3..258 and of a distance 1..32767
__device__ __forceinline__ void length_symbol(int len, int* sym, int* eb, int* ev) {
  const int x = len - 3;
  if (x < 8) { *sym = 257 + x; *eb = 0; *ev = 0; return; }
  if (len == MAX_MATCH) { *sym = 285; *eb = 0; *ev = 0; return; }
  const int e = 29 - __clz(x);                             // bit length - 3
  *sym = 261 + 4 * e + ((x >> e) & 3); *eb = e; *ev = x & ((1 << e) - 1);
}
__device__ __forceinline__ void distance_symbol(int d, int* sym, int* eb, int* ev) {
  const int x = d - 1;
  if (x < 4) { *sym = x; *eb = 0; *ev = 0; return; }
  const int e = 30 - __clz(x);                             // bit length - 2
  *sym = 2 * (e + 1) + ((x >> e) & 1); *eb = e; *ev = x & ((1 << e) - 1);
}
__device__ __forceinline__ int symbol_extra_bits(int s) {  // s: index into the joint table
  if (s < DOFF) return (s >= 265 && s < 285) ? (s - 261) >> 2 : 0;
  return s - DOFF >= 4 ? ((s - DOFF) >> 1) - 1 : 0;
}

__device__ __forceinline__ unsigned reverse_bits(unsigned code, int len) { return len ? __brev(code) >> (32 - len) : 0; }

// The length-limited Huffman code of cnt[0 .. nsym): lengths and bit-reversed canonical codes.  Every thread of the block calls it.
__device__ void build_code(const unsigned* cnt, int nsym, unsigned* len_out, unsigned* code_out, const HuffWork& w) {
  const int tid = threadIdx.x;
  unsigned c = 0, rank = 0;
  if (tid < nsym) {
    c = cnt[tid];
    if (c)
      for (int t = 0; t < nsym; ++t) {
        const unsigned ct = cnt[t];
        rank += ct && (ct < c || (ct == c && t < tid));
      }
  }
  const int n = __syncthreads_count(c != 0);
  if (c) { w.ord[rank] = tid; w.wt[rank] = c; }
  if (tid < 16) w.misc[tid] = 0;
  __syncthreads();
  if (tid == 0) {
    unsigned* cl = w.misc;                                   // codes per length
    if (n == 1) {
      cl[1] = 1;
    } else if (n >= 2) {
      int i = 0, j = 0;
      for (int k = 0; k < n - 1; ++k) {
        unsigned tot = 0;
        for (int h = 0; h < 2; ++h) {
          if (i < n && (j >= k || w.wt[i] <= w.iw[j])) { tot += w.wt[i]; w.lpar[i++] = k; }
          else { tot += w.iw[j]; w.ipar[j++] = k; }
        }
        w.iw[k] = tot;
      }
      w.lenr[n - 2] = 0;
      for (int k = n - 3; k >= 0; --k) w.lenr[k] = w.lenr[w.ipar[k]] + 1;
      for (int l = 0; l < n; ++l) cl[min(w.lenr[w.lpar[l]] + 1, 15u)] += 1;
      unsigned total = 0;
      for (int l = 1; l <= 15; ++l) total += cl[l] << (15 - l);
      while (total > (1u << 15)) {
        cl[15] -= 1;
        for (int l = 14; l >= 1; --l)
          if (cl[l]) { cl[l] -= 1; cl[l + 1] += 2; break; }
        total -= 1;
      }
    }
    int r = n;                                               // by rank: the most frequent symbols get the shortest lengths
    unsigned code = 0;
    for (int l = 1; l <= 15; ++l) {
      code = (code + (l > 1 ? cl[l - 1] : 0)) << 1;
      w.misc[16 + l] = code;
      for (unsigned k = 0; k < cl[l]; ++k) w.lenr[--r] = l;
    }
  }
  __syncthreads();
  const unsigned len = c ? w.lenr[rank] : 0;
  if (tid < nsym) len_out[tid] = len;
  __syncthreads();
  if (tid < nsym) {
    unsigned before = 0;
    if (len)
      for (int t = 0; t < tid; ++t) before += len_out[t] == len;
    code_out[tid] = len ? reverse_bits(w.misc[16 + len] + before, (int)len) : 0;
  }
  __syncthreads();
}

// LSB-first bit writer into the round's LDS buffer from bit position `pos`.  The first and the last word of a lane's string are
// shared with its neighbours (LDS atomic OR into zeroed words); the words in between are its own (plain stores).
struct BitWriter {
  unsigned* buf;
  unsigned word;
  unsigned long long acc;
  int n;
  bool shared;
  __device__ BitWriter(unsigned* b, unsigned pos) : buf(b), word(pos >> 5), acc(0), n((int)(pos & 31)), shared((pos & 31) != 0) {}
  __device__ __forceinline__ void put(unsigned bits, int len) {          // len <= 32, bits < 2^len
    acc |= (unsigned long long)bits << n;
    n += len;
    if (n >= 32) {
      if (shared) atomicOr(buf + word, (unsigned)acc); else buf[word] = (unsigned)acc;
      shared = false;
      ++word;
      acc >>= 32;
      n -= 32;
    }
  }
  __device__ __forceinline__ void finish() {
    if (n > 0) atomicOr(buf + word, (unsigned)acc);
  }
};
struct BitCounter {
  unsigned n = 0;
  __device__ __forceinline__ void put(unsigned, int len) { n += len; }
};

// the block header in front of the code lengths: BFINAL 0, BTYPE 2, HLIT 29, HDIST 29, HCLEN 15, then the 19 lengths of the fixed
// code-length code in the order 16 17 18 0 8 7 9 6 10 5 11 4 12 3 13 2 14 1 15 (3 bits each: 5 for symbols 13..18, 4 otherwise)
constexpr unsigned HEAD17 = 4u | 29u << 3 | 29u << 8 | 15u << 13;
constexpr unsigned long long cl_lengths_word() {
  const int order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
  unsigned long long v = 0;
  for (int i = 0; i < 19; ++i) v |= (unsigned long long)(order[i] <= 12 ? 4 : 5) << (3 * i);
  return v;
}
constexpr unsigned long long CL57 = cl_lengths_word();
constexpr int HEAD_BITS = 17 + 57;

// One emission round: lanes put their items (emit(sink) with a BitCounter, then a BitWriter at the prefix sum), whole bytes go to
// the slot, the unfinished byte is carried.  `closing`: the round ends the segment - the last item's lane (tid == closer) appends
// the empty stored block behind its item.
template <class Emit>
__device__ __forceinline__ void emit_round(Emit emit, unsigned* bits, unsigned* wsum, unsigned char* out, unsigned* out_pos,
                                           unsigned* carry_bits, unsigned* carry_word, bool closing, int closer, unsigned bfinal) {
  const int tid = threadIdx.x;
  BitCounter cnt;
  emit(cnt);
  if (closing && tid == closer) cnt.put(0, 3);
  unsigned total;
  const unsigned ex = block_exscan<SG_WAVES>(cnt.n, wsum, &total);
  unsigned T = *carry_bits + total;
  const unsigned pad = closing ? (0u - T) & 7 : 0;
  const unsigned T_end = T + (closing ? pad + 32 : 0);
  for (unsigned i = tid; i < (T_end + 31) / 32 + 1; i += SG_THREADS) bits[i] = i == 0 ? *carry_word : 0;
  __syncthreads();
  {
    BitWriter w(bits, *carry_bits + ex);
    emit(w);
    if (closing && tid == closer) {
      w.put(bfinal, 3);                                      // BFINAL, BTYPE 00
      w.put(0, (int)pad);
      w.put(0xFFFF0000u, 32);                                // LEN 0, NLEN FFFF
    }
    if (cnt.n) w.finish();
  }
  __syncthreads();
  const unsigned nbytes = T_end >> 3;
  const unsigned char* b8 = reinterpret_cast<const unsigned char*>(bits);
  for (unsigned j = tid; j < nbytes; j += SG_THREADS)
    if (*out_pos + j < (unsigned)SLOT) out[*out_pos + j] = b8[j];                  // (n + 10 at most: the stored fallback holds it)
  const unsigned cb = T_end & 7;
  const unsigned cw = cb ? (unsigned)b8[nbytes] & ((1u << cb) - 1) : 0;
  __syncthreads();
  *out_pos += nbytes;
  *carry_bits = cb;
  *carry_word = cw;
}

__global__ __launch_bounds__(SG_THREADS) void png_segment(const unsigned char* __restrict__ filt, size_t S, int W, int nseg,
                                                          unsigned char* __restrict__ slots, unsigned* __restrict__ lens,
                                                          unsigned* __restrict__ adler) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  unsigned* seg = reinterpret_cast<unsigned*>(smem + L_SEG);
  const unsigned char* seg8 = smem + L_SEG;
  unsigned short* tok = reinterpret_cast<unsigned short*>(smem + L_TOK);
  unsigned* table = reinterpret_cast<unsigned*>(smem + L_HASH);
  unsigned* bits = table;
  unsigned short* cl = reinterpret_cast<unsigned short*>(smem + L_CL);
  unsigned short* cd = reinterpret_cast<unsigned short*>(smem + L_CD);
  unsigned* hist = reinterpret_cast<unsigned*>(smem + L_HIST);
  unsigned* hlen = reinterpret_cast<unsigned*>(smem + L_LEN);
  unsigned* hcode = reinterpret_cast<unsigned*>(smem + L_CODE);
  unsigned* work = reinterpret_cast<unsigned*>(smem + L_WORK);
  const HuffWork hw = {work, work + 288, work + 2 * 288, work + 3 * 288, work + 4 * 288, work + 5 * 288, work + 6 * 288};
  unsigned* wsum = hw.misc + 32;
  const int tid = threadIdx.x, sg = blockIdx.x;
  const size_t base = (size_t)sg * SEG;
  const int n = (int)min((size_t)SEG, S - base);
  const unsigned char* src = filt + base;
  unsigned char* out = slots + (size_t)sg * SLOT;

  // stage the segment (16-byte reads where whole, bytes at the end), zero what lies behind it, the tokens, the table, the counts
  for (int i = tid * 16; i < SEG + 16; i += SG_THREADS * 16) {
    int4 v = make_int4(0, 0, 0, 0);
    if (i + 16 <= n) {
      v = *reinterpret_cast<const int4*>(src + i);
    } else if (i < n) {
      unsigned w[4] = {0, 0, 0, 0};
      #pragma unroll
      for (int k = 0; k < 16; ++k)
        if (i + k < n) w[k >> 2] |= (unsigned)src[i + k] << (8 * (k & 3));
      v = make_int4((int)w[0], (int)w[1], (int)w[2], (int)w[3]);
    }
    *reinterpret_cast<int4*>(smem + L_SEG + i) = v;
  }
  for (int i = tid; i < (2 * SEG + 16) / 4; i += SG_THREADS) reinterpret_cast<unsigned*>(tok)[i] = 0;
  for (int i = tid; i < (1 << HASH_BITS); i += SG_THREADS) table[i] = 0;
  for (int i = tid; i < NSYM; i += SG_THREADS) hist[i] = i == 256 ? 1 : 0;
  __syncthreads();

  // Adler-32 partial sums of the segment: A = sum d, B = sum (n - i) d, both mod 65521
  {
    unsigned a = 0, b = 0;
    for (int i = tid; i < n; i += SG_THREADS) {
      const unsigned d = seg8[i];
      a += d;
      b += (unsigned)(n - i) * d;
    }
    const unsigned A = block_sum(a, wsum), B = block_sum(b % ADLER_MOD, wsum);
    if (tid == 0) {
      adler[2 * sg] = A % ADLER_MOD;
      adler[2 * sg + 1] = B % ADLER_MOD;
    }
  }

  // matches chunk by chunk, the greedy walk behind them
  const int rowd = 1 + 3 * W;
  int entry = 0;                                             // (thread 0) where the parse enters the next chunk
  for (int lo = 0; lo < n; lo += CHUNK) {
    const int p = lo + tid;
    unsigned h = 0;
    const bool hashed = p + 4 <= n;
    if (p < n) {
      const int room = min(MAX_MATCH, n - p);
      int bl = 0, bd = 0;
      auto candidate = [&](int d) {
        if (d > p) return;
        const int l = match_length(seg, p - d, p, room);
        if (l >= 3 && (l > bl || (l == bl && d < bd))) { bl = l; bd = d; }
      };
      candidate(3);
      candidate(rowd);
      if (hashed) {
        h = (load4(seg, p) * 2654435761u) >> (32 - HASH_BITS);
        const unsigned q1 = table[h];
        if (q1) candidate(p - (int)(q1 - 1));
      }
      cl[tid] = (unsigned short)bl;
      cd[tid] = (unsigned short)bd;
    }
    __syncthreads();
    if (hashed) atomicMax(table + h, (unsigned)p + 1);
    if (tid == 0) {
      const int hi = min(lo + CHUNK, n);
      int q = entry;
      while (q < hi) {
        const int l = cl[q - lo];
        if (l >= 3) {
          tok[q] = (unsigned short)l;
          tok[q + 1] = (unsigned short)(0x8000u | cd[q - lo]);
          q += l;
        } else {
          tok[q] = 1;
          q += 1;
        }
      }
      entry = q;
    }
    __syncthreads();
  }

  // histogram of the tokens (LDS atomic adds: counts do not depend on the order)
  for (int p = tid; p < n; p += SG_THREADS) {
    const unsigned t = tok[p];
    if (t == 1) {
      atomicAdd(hist + seg8[p], 1u);
    } else if (t >= 3 && t < 0x8000u) {
      int s, eb, ev;
      length_symbol((int)t, &s, &eb, &ev);
      atomicAdd(hist + s, 1u);
      distance_symbol(tok[p + 1] & 0x7FFF, &s, &eb, &ev);
      atomicAdd(hist + DOFF + s, 1u);
    }
  }
  __syncthreads();
  if (tid == 0) {                                            // every tree gets two symbols
    int used = 0;
    for (int s = 0; s < NDIST; ++s) used += hist[DOFF + s] != 0;
    hw.misc[48] = used < 2 && hist[DOFF] == 0;               // a count raised here stands for no token
    hw.misc[49] = used < 2 && hist[DOFF + 1] == 0;
    if (used < 2) {
      hist[DOFF] = max(hist[DOFF], 1u);
      hist[DOFF + 1] = max(hist[DOFF + 1], 1u);
    }
  }
  if (tid >= NLIT && tid < DOFF) { hlen[tid] = 0; hcode[tid] = 0; }
  __syncthreads();
  build_code(hist, NLIT, hlen, hcode, hw);
  build_code(hist + DOFF, NDIST, hlen + DOFF, hcode + DOFF, hw);

  // the dynamic block's size; longer than 5 + n bytes -> a stored block
  unsigned mine = 0;
  if (tid < NLIT || (tid >= DOFF && tid < DOFF + NDIST)) {
    const unsigned l = hlen[tid];
    const bool raised = (tid == DOFF && hw.misc[48]) || (tid == DOFF + 1 && hw.misc[49]);
    mine = (raised ? 0 : hist[tid]) * (l + symbol_extra_bits(tid)) + (l <= 12 ? 4 : 5);
  }
  const unsigned dyn_bits = HEAD_BITS + block_sum(mine, wsum);
  const unsigned bfinal = sg == nseg - 1 ? 1u : 0u;
  if ((dyn_bits + 7) / 8 > 5u + (unsigned)n) {
    if (tid == 0) {
      out[0] = 0;
      out[1] = (unsigned char)(n & 0xFF);
      out[2] = (unsigned char)((n >> 8) & 0xFF);
      out[3] = (unsigned char)(~n & 0xFF);
      out[4] = (unsigned char)((~n >> 8) & 0xFF);
      out[5 + n] = (unsigned char)bfinal;
      out[6 + n] = 0;
      out[7 + n] = 0;
      out[8 + n] = 0xFF;
      out[9 + n] = 0xFF;
      lens[sg] = (unsigned)n + 10;
    }
    for (int i = tid; i < n; i += SG_THREADS) out[5 + i] = seg8[i];
    return;
  }

  unsigned out_pos = 0, carry_bits = 0, carry_word = 0;
  // the header: lane 0 the fixed part, lanes 1 .. 316 one code length each in the fixed code-length code
  emit_round([&](auto& sink) {
    if (tid == 0) {
      sink.put(HEAD17, 17);
      sink.put((unsigned)(CL57 & 0x3FFFFFFFu), 30);
      sink.put((unsigned)(CL57 >> 30), 27);
    } else if (tid <= NLIT + NDIST) {
      const unsigned v = hlen[tid <= NLIT ? tid - 1 : DOFF + tid - 1 - NLIT];
      if (v <= 12) sink.put(reverse_bits(v, 4), 4); else sink.put(reverse_bits(26 + v - 13, 5), 5);
    }
  }, bits, wsum, out, &out_pos, &carry_bits, &carry_word, false, 0, bfinal);
  // the tokens: a lane per position, the end-of-block symbol at position n
  for (int lo = 0; lo <= n; lo += CHUNK) {
    const int p = lo + tid;
    const unsigned t = p < n ? tok[p] : 0;
    const bool closing = lo + CHUNK > n;
    emit_round([&](auto& sink) {
      if (p == n) {
        sink.put(hcode[256], (int)hlen[256]);
      } else if (t == 1) {
        const unsigned s = seg8[p];
        sink.put(hcode[s], (int)hlen[s]);
      } else if (t >= 3 && t < 0x8000u) {
        int s, eb, ev;
        length_symbol((int)t, &s, &eb, &ev);
        sink.put(hcode[s] | (unsigned)ev << hlen[s], (int)hlen[s] + eb);
        distance_symbol(tok[p + 1] & 0x7FFF, &s, &eb, &ev);
        sink.put(hcode[DOFF + s] | (unsigned)ev << hlen[DOFF + s], (int)hlen[DOFF + s] + eb);
      }
    }, bits, wsum, out, &out_pos, &carry_bits, &carry_word, closing, n - lo, bfinal);
  }
  if (tid == 0) lens[sg] = out_pos;
}

// ---- step 3: compaction -----------------------------------------------------------------------------------------------------------
constexpr int CP_THREADS = 256;

struct PngHead {
  unsigned char b[36];                                       // signature + IHDR chunk: 33 bytes
};

// a(x) b(x) mod P in the reflected representation of CRC-32 (x^0 = 0x80000000)
__device__ __forceinline__ unsigned gf2_mul(unsigned a, unsigned b) {
  unsigned p = 0;
  for (int i = 0; i < 32; ++i) {
    if (a & (0x80000000u >> i)) p ^= b;
    b = (b & 1) ? (b >> 1) ^ CRC_POLY : b >> 1;
  }
  return p;
}
// x^(8 n) mod P
__device__ __forceinline__ unsigned gf2_x8n(unsigned n) {
  unsigned r = 0x80000000u, p = 0x00800000u;                 // 1, x^8
  for (; n; n >>= 1) {
    if (n & 1) r = gf2_mul(r, p);
    p = gf2_mul(p, p);
  }
  return r;
}

__device__ __forceinline__ unsigned crc_step(const unsigned* tab, unsigned c, unsigned byte) { return tab[(c ^ byte) & 0xFF] ^ (c >> 8); }
__device__ __forceinline__ unsigned crc_bytes(const unsigned* tab, const unsigned char* p, unsigned n) {
  unsigned c = 0xFFFFFFFFu;
  for (unsigned i = 0; i < n; ++i) c = crc_step(tab, c, p[i]);
  return ~c;
}
__device__ __forceinline__ unsigned crc_be32(const unsigned* tab, unsigned c, unsigned v) {
  #pragma unroll
  for (int k = 24; k >= 0; k -= 8) c = crc_step(tab, c, (v >> k) & 0xFF);
  return c;
}

__device__ __forceinline__ void store_be32(unsigned char* p, unsigned v) {
  p[0] = (unsigned char)(v >> 24); p[1] = (unsigned char)(v >> 16); p[2] = (unsigned char)(v >> 8); p[3] = (unsigned char)v;
}

__global__ __launch_bounds__(CP_THREADS) void png_compact(const unsigned char* __restrict__ slots, const unsigned* __restrict__ lens,
                                                          const unsigned* __restrict__ adler, int nseg, size_t S, PngHead head,
                                                          unsigned char* __restrict__ out, unsigned* __restrict__ d_len) {
  __shared__ unsigned long long part[CP_THREADS / 64];
  __shared__ unsigned xpart[CP_THREADS / 64];
  __shared__ unsigned crc_tab[256];
  __shared__ unsigned adler_value;
  const int tid = threadIdx.x, sg = blockIdx.x;
  const bool first = sg == 0, last = sg == nseg - 1;
  {
    unsigned c = tid;
    for (int k = 0; k < 8; ++k) c = (c & 1) ? (c >> 1) ^ CRC_POLY : c >> 1;
    crc_tab[tid] = c;
  }
  // exclusive prefix sum of (length + 12 bytes of chunk framing) over the segments before this one
  unsigned long long s = 0;
  for (int i = tid; i < sg; i += CP_THREADS) s += lens[i] + 12;
  #pragma unroll
  for (int d = 32; d >= 1; d >>= 1) s += __shfl_xor(s, d);
  if ((tid & 63) == 0) part[tid >> 6] = s;
  __syncthreads();
  size_t off = 33 + (first ? 0 : 2);                         // signature + IHDR, the zlib header in the first chunk
  #pragma unroll
  for (int w = 0; w < CP_THREADS / 64; ++w) off += part[w];
  __syncthreads();
  if (last) {
    // Adler-32 of the stream from the segments' partial sums: A = 1 + sum A_i, B = S + sum (A_i (S - end_i) + B_i), mod 65521
    unsigned long long a = 0, b = 0;
    for (int i = tid; i < nseg; i += CP_THREADS) {
      const size_t end = min((size_t)(i + 1) * SEG, S);
      a += adler[2 * i];
      b += (unsigned long long)adler[2 * i] * (unsigned)((S - end) % ADLER_MOD) % ADLER_MOD + adler[2 * i + 1];
    }
    #pragma unroll
    for (int d = 32; d >= 1; d >>= 1) { a += __shfl_xor(a, d); b += __shfl_xor(b, d); }
    if ((tid & 63) == 0) part[tid >> 6] = a;
    __syncthreads();
    unsigned long long A = 1;
    for (int w = 0; w < CP_THREADS / 64; ++w) A += part[w];
    __syncthreads();
    if ((tid & 63) == 0) part[tid >> 6] = b;
    __syncthreads();
    unsigned long long B = S % ADLER_MOD;
    for (int w = 0; w < CP_THREADS / 64; ++w) B += part[w];
    if (tid == 0) adler_value = (unsigned)(B % ADLER_MOD) << 16 | (unsigned)(A % ADLER_MOD);
    __syncthreads();
  }
  if (first)
    for (int i = tid; i < 33; i += CP_THREADS) out[i] = head.b[i];
  const unsigned n = lens[sg];
  const unsigned hb = first ? 2 : 0, tb = last ? 4 : 0;      // bytes of the chunk's data in front of and behind the segment's
  const unsigned char* src = slots + (size_t)sg * SLOT;
  unsigned char* chunk = out + off;
  unsigned char* dst = chunk + 8 + hb;
  // CRC-32 of type + data: a lane takes a slice of the segment's bytes, its CRC is moved to the slice's place by x^(8 (bytes
  // behind it)), the pieces are XORed; lane 0 adds the bytes in front, lane 1 the Adler-32 behind.
  const unsigned per = (n + CP_THREADS - 1) / CP_THREADS;
  const unsigned lo = min(n, tid * per), hi = min(n, lo + per);
  unsigned piece = gf2_mul(gf2_x8n(n - hi + tb), crc_bytes(crc_tab, src + lo, hi - lo));
  if (tid == 0) {
    unsigned c = crc_be32(crc_tab, 0xFFFFFFFFu, 0x49444154u);                 // "IDAT"
    if (first) c = crc_step(crc_tab, crc_step(crc_tab, c, 0x78), 0x01);
    piece ^= gf2_mul(gf2_x8n(n + tb), ~c);
  }
  if (tid == 1 && last) {
    piece ^= ~crc_be32(crc_tab, 0xFFFFFFFFu, adler_value);
  }
  #pragma unroll
  for (int d = 32; d >= 1; d >>= 1) piece ^= __shfl_xor(piece, d);
  if ((tid & 63) == 0) xpart[tid >> 6] = piece;
  __syncthreads();
  if (tid == 0) {
    unsigned crc = 0;
    for (int w = 0; w < CP_THREADS / 64; ++w) crc ^= xpart[w];
    store_be32(chunk, n + hb + tb);
    chunk[4] = 'I'; chunk[5] = 'D'; chunk[6] = 'A'; chunk[7] = 'T';
    if (first) { chunk[8] = 0x78; chunk[9] = 0x01; }
    if (last) store_be32(dst + n, adler_value);
    store_be32(dst + n + tb, crc);
    if (last) {
      store_be32(dst + n + tb + 4, 0);                       // IEND: length 0, type, its CRC
      store_be32(dst + n + tb + 8, 0x49454E44u);
      store_be32(dst + n + tb + 12, 0xAE426082u);
      *d_len = (unsigned)(off + 8 + hb + n + tb + 4 + 12);
    }
  }
  // the segment's bytes: up to the destination's first dword boundary, whole destination dwords from two aligned source dwords,
  // the rest
  const unsigned headb = min(n, (unsigned)((4 - ((uintptr_t)dst & 3)) & 3));
  if ((unsigned)tid < headb) dst[tid] = src[tid];
  const unsigned nd = (n - headb) / 4;
  const unsigned mis = (unsigned)((uintptr_t)(src + headb) & 3);
  const unsigned* s4 = reinterpret_cast<const unsigned*>(src + headb - mis);
  unsigned* d4 = reinterpret_cast<unsigned*>(dst + headb);
  for (unsigned d = tid; d < nd; d += CP_THREADS) {
    unsigned v = s4[d];
    if (mis) v = (v >> (8 * mis)) | (s4[d + 1] << (32 - 8 * mis));      // (the slots end in spare dwords)
    d4[d] = v;
  }
  for (unsigned i = headb + 4 * nd + tid; i < n; i += CP_THREADS) dst[i] = src[i];
}

// ---- host ------------------------------------------------------------------------------------------------------------------------
unsigned host_crc32(const unsigned char* p, size_t n) {
  unsigned c = 0xFFFFFFFFu;
  for (size_t i = 0; i < n; ++i) {
    c ^= p[i];
    for (int k = 0; k < 8; ++k) c = (c & 1) ? (c >> 1) ^ CRC_POLY : c >> 1;
  }
  return ~c;
}

void put_be32(unsigned char* p, unsigned v) {
  p[0] = (unsigned char)(v >> 24); p[1] = (unsigned char)(v >> 16); p[2] = (unsigned char)(v >> 8); p[3] = (unsigned char)v;
}

PngHead png_head(int H, int W) {
  PngHead h{};
  const unsigned char sig[8] = {0x89, 'P', 'N', 'G', '\r', '\n', 0x1A, '\n'};
  std::memcpy(h.b, sig, 8);
  put_be32(h.b + 8, 13);
  std::memcpy(h.b + 12, "IHDR", 4);
  put_be32(h.b + 16, (unsigned)W);
  put_be32(h.b + 20, (unsigned)H);
  h.b[24] = 8; h.b[25] = 2; h.b[26] = 0; h.b[27] = 0; h.b[28] = 0;       // bit depth, colour type, compression, filter, interlace
  put_be32(h.b + 29, host_crc32(h.b + 12, 17));
  return h;
}

}  // namespace

struct poco_png_encoder {
  int max_h = 0, max_w = 0;
  unsigned char* filt = nullptr;           // the filtered stream, H x (1 + 3W)
  unsigned char* slots = nullptr;          // [segments] worst-case slots of deflate bytes
  unsigned* lens = nullptr;                // [segments]
  unsigned* adler = nullptr;               // [segments][2]
  ~poco_png_encoder() {
    for (void* p : {(void*)filt, (void*)slots, (void*)lens, (void*)adler})
      if (p) (void)hipFree(p);
  }
};

extern "C" int poco_png_encoder_create(int max_h, int max_w, poco_png_encoder_t* out) {
  if (!out) { poco_set_error("poco_png_encoder_create: null handle pointer"); return POCO_ERR_ARG; }
  *out = nullptr;
  if (max_h < 1 || max_w < 1 || max_h > PNG_MAX_SIDE || max_w > PNG_MAX_SIDE) {
    poco_set_error("poco_png_encoder_create: bad arguments (need 1 <= max_h, max_w <= 16384)");
    return POCO_ERR_ARG;
  }
  auto e = std::make_unique<poco_png_encoder>();
  e->max_h = max_h;
  e->max_w = max_w;
  const size_t nseg = png_segments(max_h, max_w);
  POCO_HIP_CHECK(hipMalloc(&e->filt, png_stream_bytes(max_h, max_w) + 16));
  POCO_HIP_CHECK(hipMalloc(&e->slots, nseg * SLOT));
  POCO_HIP_CHECK(hipMalloc(&e->lens, nseg * sizeof(unsigned)));
  POCO_HIP_CHECK(hipMalloc(&e->adler, nseg * 2 * sizeof(unsigned)));
  POCO_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(png_segment), hipFuncAttributeMaxDynamicSharedMemorySize, L_END));
  *out = e.release();
  return POCO_OK;
}

extern "C" int poco_png_encode(poco_png_encoder_t e, const unsigned char* d_rgb, int H, int W, unsigned char* d_out, size_t out_cap,
                               unsigned int* d_len, void* stream) {
  if (!e || !d_rgb || !d_out || !d_len) { poco_set_error("poco_png_encode: null handle or pointer"); return POCO_ERR_ARG; }
  if (H < 1 || W < 1 || H > e->max_h || W > e->max_w) {
    poco_set_error("poco_png_encode: frame of " + std::to_string(H) + " x " + std::to_string(W) + " outside 1 x 1 .. " +
                   std::to_string(e->max_h) + " x " + std::to_string(e->max_w) + " (the size the encoder was created for)");
    return POCO_ERR_ARG;
  }
  if (out_cap < png_worst_case(H, W)) {
    poco_set_error("poco_png_encode: out_cap " + std::to_string(out_cap) + " is below the worst case of " +
                   std::to_string(png_worst_case(H, W)) + " bytes for this frame size");
    return POCO_ERR_ARG;
  }
  const hipStream_t s = (hipStream_t)stream;
  const size_t S = png_stream_bytes(H, W);
  const int nseg = (int)png_segments(H, W);
  png_filter<<<H, FL_THREADS, 0, s>>>(d_rgb, H, W, e->filt);
  png_segment<<<nseg, SG_THREADS, L_END, s>>>(e->filt, S, W, nseg, e->slots, e->lens, e->adler);
  png_compact<<<nseg, CP_THREADS, 0, s>>>(e->slots, e->lens, e->adler, nseg, S, png_head(H, W), d_out, d_len);
  POCO_HIP_CHECK(hipGetLastError());
  return POCO_OK;
}

extern "C" void poco_png_encoder_destroy(poco_png_encoder_t e) { delete e; }
