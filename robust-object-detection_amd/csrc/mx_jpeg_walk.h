// mx_jpeg_walk.h — the Huffman walk of the parallel JPEG entropy decoder, shared by the kernels
// (mx_jpeg.hip: mx_jpeg_entropy_decode) and their serial host restatement (mx_jpeg.cpp:
// mx_jpeg_decode_coefs_chunked). One step = one Huffman symbol with its extra bits (T.81 F.2.2), read
// from the unstuffed ("clean") stream; the state it advances is (bit position, block slot inside the
// MCU, zig-zag index). A prefix code is decoded from the bits it consumes alone, so whatever lies past
// a segment's last bit never influences a step that ends inside the segment.
#pragma once
#include <stdint.h>

#include "../../include/mx_det.h"

#ifdef __HIP__
#define MX_HD __host__ __device__ __forceinline__
#else
#define MX_HD inline
#endif

namespace mx {

// Canonical decoding tables of one DHT table (T.81 F.2.2.3 MAXCODE / VALPTR) + the 9-bit lookahead,
// as build_huff (mx_jpeg.cpp) derives them. look: length << 8 | value, 0 for a code over 9 bits.
struct JdHuff {
  int32_t maxcode[18];
  int32_t valoff[17];
  uint8_t val[256];
  uint16_t look[512];
};
constexpr int kJdTables = 6;  // dc, ac of component 0, 1, 2
constexpr int kJdHuffWords = (int)(kJdTables * sizeof(JdHuff) / 4);

struct JdGeom {
  int32_t ncomp, mcux, bpm;             // bpm: blocks per MCU
  int32_t h[3], v[3], bw[3], first[3];  // first: slot of the component's first block inside an MCU
  int64_t coef_off[3];
  int64_t nblk;    // blocks of the scan
  int64_t segblk;  // blocks of a full restart segment (nblk without restarts)
  int32_t nseg;    // restart segments the geometry calls for
  int32_t subseq;  // bits per subsequence
};

// subsequence size: bits one lane decodes. A step consumes at most 31 bits, so a lane overshoots its
// subsequence by less than 64 bits (the 6 bits of `over` below) and never skips one.
constexpr int kJdSubseqMin = 64, kJdSubseqDefault = 512, kJdSubseqMax = 65536;
constexpr int kJdLanes = 256;      // subsequences per workgroup
constexpr int kJdChunk = 4096;     // bytes per workgroup of the unstuffing passes (16 per lane)
constexpr uint32_t kJdEnd = 0xffffffffu;  // exit state: the segment's data ended inside the lane

struct JdState {
  int64_t pos;  // bit of the clean stream
  int32_t slot, k;  // block slot inside the MCU; zig-zag index of the next coefficient (0: the DC is next)
};

// exit state of a lane relative to `boundary`, the first bit of the next subsequence
MX_HD uint32_t jd_pack(const JdState& s, int64_t boundary) {
  return ((uint32_t)(s.pos - boundary) << 10) | ((uint32_t)s.slot << 6) | (uint32_t)s.k;
}
MX_HD JdState jd_unpack(uint32_t e, int64_t boundary) {
  JdState s;
  s.pos = boundary + (int64_t)(e >> 10);
  s.slot = (int32_t)((e >> 6) & 15);
  s.k = (int32_t)(e & 63);
  return s;
}

// byte classes of the stuffed scan. prev / next: the neighbouring bytes, -1 beyond the buffer.
//   marker: 0xFF followed by a non-zero byte (RSTn, EOI, fill bytes, anything else); a last 0xFF
//           counts as data, as the sequential reader takes it;
//   rst:    marker RST0..RST7;
//   drop:   the byte after a 0xFF: a stuffed zero or a marker's second byte, never data.
constexpr int kJdMarker = 1, kJdRst = 2, kJdDrop = 4;
MX_HD int jd_classify(int prev, int cur, int next) {
  int f = prev == 0xFF ? kJdDrop : 0;
  if (cur == 0xFF && next > 0) f |= kJdMarker | ((next >= 0xD0 && next <= 0xD7) ? kJdRst : 0);
  return f;
}

MX_HD int jd_natural(int k) {  // zig-zag index -> natural index (T.81 Figure A.6)
  const uint8_t t[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                         41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                         30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
  return t[k];
}

// Reader of the clean stream: 32 bits from the state's bit on at every step, MSB first, out of a 64-bit
// window refilled one 4-byte aligned word at a time (one load per 32 bits consumed). words: the stream
// in memory order; a peek at bit b reads no further than the word after b's.
struct JdReader {
  const uint32_t* words;
  int64_t next;  // word the next refill loads
  uint64_t buf;
  int cnt;  // valid bits of buf; buf ends on a word boundary
};
MX_HD void jd_open(JdReader& r, const uint32_t* words, int64_t bit) {
  const int64_t w = bit >> 5;
  const int sh = (int)(bit & 31);
  r.words = words;
  r.buf = (((uint64_t)__builtin_bswap32(words[w]) << 32) | __builtin_bswap32(words[w + 1])) << sh;
  r.cnt = 64 - sh;
  r.next = w + 2;
}
MX_HD uint32_t jd_peek32(JdReader& r) {
  if (r.cnt < 32) {
    r.buf |= (uint64_t)__builtin_bswap32(r.words[r.next++]) << (32 - r.cnt);
    r.cnt += 32;
  }
  return (uint32_t)(r.buf >> 32);
}
MX_HD void jd_skip(JdReader& r, int n) {
  r.buf <<= n;
  r.cnt -= n;
}

MX_HD int jd_comp(const JdGeom& g, int slot) {
  return (g.ncomp == 3 && slot >= g.first[1]) ? (slot >= g.first[2] ? 2 : 1) : 0;
}

// coefficient offset of scan-order block s (MCU-interleaved order -> planar [comp][by][bx][64], the
// mapping of mx_jpeg_decode_coefs)
MX_HD int64_t jd_block_off(const JdGeom& g, int64_t s) {
  const int64_t m = s / g.bpm;
  const int slot = (int)(s - m * g.bpm);
  const int c = jd_comp(g, slot);
  const int kk = slot - g.first[c];
  return g.coef_off[c] + (((m / g.mcux) * g.v[c] + kk / g.h[c]) * g.bw[c] + (m % g.mcux) * g.h[c] + kk % g.h[c]) * 64;
}

// One step. Returns -1 (s untouched) when the symbol would pass `end`, the segment's last bit; else
// the MX_JPEG_ST_* bits of what is wrong with the symbol (0: nothing). A wrong symbol still advances
// the state deterministically (speculating lanes meet them all the time): an invalid code consumes
// 16 bits as symbol 0, a DC size takes its low 4 bits, an AC run past 63 ends the block.
// *idx / *val: the coefficient the step produced (zig-zag -> natural index; the DC difference at 0),
// idx -1 for none. *done: 1 when the step completed a block.
MX_HD int jd_step(JdReader& rd, int64_t end, const JdHuff* tabs, const JdGeom& g, JdState& s, int* idx, int* val,
                  int* done) {
  const uint32_t w = jd_peek32(rd);
  const JdHuff& t = tabs[2 * jd_comp(g, s.slot) + (s.k != 0)];
  int err = 0, len, sym;
  const uint32_t lk = t.look[w >> 23];
  if (lk) {
    len = (int)(lk >> 8);
    sym = (int)(lk & 255);
  } else {
    // the first length 9..16 whose prefix is at most MAXCODE (T.81 F.2.2.3 DECODE), all eight compared
    // at once: the loads do not wait on one another, as they would in the loop over lengths
    const uint32_t top = w >> 16;
    uint32_t fits = 0;
#pragma unroll
    for (int l = 9; l <= 16; ++l) fits |= (uint32_t)((int32_t)(top >> (16 - l)) <= t.maxcode[l]) << (l - 9);
    if (fits == 0) {
      err = MX_JPEG_ST_CODE;
      len = 16;
      sym = 0;
    } else {
      len = 9 + __builtin_ctz(fits);
      sym = t.val[((int32_t)(top >> (16 - len)) + t.valoff[len]) & 255];
    }
  }
  const int sz = sym & 15;
  if (s.pos + len + sz > end) return -1;
  int v = 0;
  if (sz) {
    v = (int)((w << len) >> (32 - sz));
    if (v < (1 << (sz - 1))) v = v - (1 << sz) + 1;  // EXTEND (T.81 F.2.2.1)
  }
  s.pos += len + sz;
  jd_skip(rd, len + sz);
  *idx = -1;
  *done = 0;
  if (s.k == 0) {
    if (sym > 11) err |= MX_JPEG_ST_DC;
    *idx = 0;
    *val = v;
    s.k = 1;
  } else {
    const int r = sym >> 4;
    if (sz) {
      s.k += r;
      if (s.k > 63) {
        err |= MX_JPEG_ST_RUN;
        s.k = 64;
      } else {
        *idx = jd_natural(s.k);
        *val = v;
        ++s.k;
      }
    } else {
      s.k = r == 15 ? s.k + 16 : 64;  // ZRL / EOB
    }
  }
  if (s.k >= 64) {
    s.k = 0;
    s.slot = s.slot + 1 == g.bpm ? 0 : s.slot + 1;
    *done = 1;
  }
  return err;
}

// The walk of one lane without stores: from s to the first state at or past `limit` (the next
// subsequence's first bit, or the segment's end). Returns the packed exit state; *nblk = blocks completed.
MX_HD uint32_t jd_walk(const uint32_t* words, const JdHuff* tabs, const JdGeom& g, JdState s, int64_t limit, int64_t end,
                       uint32_t* nblk) {
  uint32_t n = 0;
  int idx, val, done;
  JdReader rd;
  if (s.pos < limit) jd_open(rd, words, s.pos);
  while (s.pos < limit) {
    if (jd_step(rd, end, tabs, g, s, &idx, &val, &done) < 0) {
      *nblk = n;
      return kJdEnd;
    }
    n += done;
  }
  *nblk = n;
  return jd_pack(s, limit);
}

// The same walk from the lane's true start state, storing. blk: blocks of the segment completed before
// the lane; quota: blocks the segment holds; seg_first: scan-order index of its first block. Blocks past
// the quota (padding bits, trailing data) are neither stored nor judged. last: the lane is the
// segment's last, and reports a segment that ends short of its quota. Returns MX_JPEG_ST_* bits.
MX_HD int jd_walk_store(const uint32_t* words, const JdHuff* tabs, const JdGeom& g, JdState s, bool ended, int64_t limit,
                        int64_t end, int64_t blk, int64_t quota, int64_t seg_first, bool last, int16_t* coefs) {
  int err = 0;
  int idx, val, done;
  int64_t off = blk < quota ? jd_block_off(g, seg_first + blk) : 0;
  JdReader rd;
  if (!ended && s.pos < limit) jd_open(rd, words, s.pos);
  while (!ended && s.pos < limit) {
    const int r = jd_step(rd, end, tabs, g, s, &idx, &val, &done);
    if (r < 0) break;
    if (blk < quota) {
      err |= r;
      if (idx >= 0) coefs[off + idx] = (int16_t)val;
    }
    if (done) {
      ++blk;
      if (blk < quota) off = jd_block_off(g, seg_first + blk);
    }
  }
  if (last && blk < quota) err |= MX_JPEG_ST_SHORT;
  return err;
}

// lane i of all subsequences -> its restart segment: the j with sub_base[j] <= i < sub_base[j + 1]
MX_HD int jd_find_seg(const int64_t* sub_base, int nseg, int64_t i) {
  int lo = 0, hi = nseg - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (sub_base[mid] <= i) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}

// placement of lane i: everything a walk needs besides its input state
struct JdLane {
  int seg;
  int64_t q;         // index inside the segment
  int64_t boundary;  // first bit of the lane's subsequence
  int64_t limit;     // first bit of the next one, clipped to the segment's end
  int64_t end;       // the segment's last bit + 1
  int64_t quota, seg_first;
  bool last;
};
MX_HD JdLane jd_lane(const JdGeom& g, const int64_t* seg_start, const int64_t* sub_base, int64_t i) {
  JdLane l;
  l.seg = jd_find_seg(sub_base, g.nseg, i);
  l.q = i - sub_base[l.seg];
  const int64_t seg0 = seg_start[l.seg] * 8;
  l.end = seg_start[l.seg + 1] * 8;
  l.boundary = seg0 + l.q * g.subseq;
  l.limit = l.boundary + g.subseq < l.end ? l.boundary + g.subseq : l.end;
  l.seg_first = (int64_t)l.seg * g.segblk;
  l.quota = g.nblk - l.seg_first < g.segblk ? g.nblk - l.seg_first : g.segblk;
  l.last = i + 1 == sub_base[l.seg + 1];
  return l;
}

// segmented running sum (DC prediction: reset at every restart segment): (flag, value) pairs, a then b
struct JdSeg {
  int32_t f, v;
};
MX_HD JdSeg jd_seg_combine(const JdSeg& a, const JdSeg& b) {
  JdSeg r;
  r.f = a.f | b.f;
  r.v = b.f ? b.v : (int32_t)((uint32_t)a.v + (uint32_t)b.v);
  return r;
}

// scan-order element e of component c (its e-th block in the order the scan codes them) -> offset of
// the block; *reset: the element starts a restart segment
MX_HD int64_t jd_dc_off(const JdGeom& g, int c, int64_t e, int* reset) {
  const int hv = g.h[c] * g.v[c];
  const int64_t m = e / hv;
  const int kk = (int)(e - m * hv);
  const int64_t seg_mcus = g.segblk / g.bpm;
  *reset = kk == 0 && m % seg_mcus == 0;
  return g.coef_off[c] + (((m / g.mcux) * g.v[c] + kk / g.h[c]) * g.bw[c] + (m % g.mcux) * g.h[c] + kk % g.h[c]) * 64;
}

// host helpers (mx_jpeg.cpp)
bool jpeg_dec_tables(const mx_jpeg_info* info, JdHuff* tabs);  // false: a table build_huff rejects
const char* jpeg_dec_geom(const mx_jpeg_info* info, int subseq, JdGeom* g);  // nullptr, or what is wrong

}  // namespace mx
