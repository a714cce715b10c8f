// mx_jpeg.cpp — host half of the hybrid baseline-JPEG decoder: marker parsing and Huffman entropy
// decoding into quantised DCT coefficients (the bitstream of a JPEG without restart markers is one
// sequential prefix-code stream). The device half (mx_jpeg.hip) dequantises, runs the islow IDCT,
// upsamples and converts colour. The encoder's host half (tables, header, reference Huffman coder) is at
// the end of the file.
//
// Replaces the libjpeg(-turbo) decode behind PIL Image.open(...).convert("RGB")
// (coco_detection_dataset.py:23) and cv2.imread (restore_testsets.py:99, build_corrupted_testsets.py:139).
// Follows ITU-T T.81 (baseline sequential, Huffman): Annex B (markers), F.2.2 (DC/AC decoding,
// EXTEND), C (canonical Huffman tables), and libjpeg's MCU geometry (jdinput.c initial_setup,
// per_scan_setup) for the coefficient layout.
#include <string.h>

#include <vector>

#include "../../include/mx_det.h"
#include "mx_jpeg_walk.h"

namespace mx {
void set_error(const char* fmt, ...);
}

namespace {

// zig-zag index -> natural (row-major) index (T.81 Figure A.6 / libjpeg jpeg_natural_order)
const int kNatural[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                          41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                          30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

int fail(int code, const char* msg) {
  mx::set_error("%s", msg);
  return code;
}

int cdiv(int a, int b) { return (a + b - 1) / b; }

// Canonical decoding tables (T.81 F.2.2.3: MAXCODE / VALPTR / MINCODE) + a 9-bit lookahead
struct Huff {
  int32_t maxcode[18];
  int32_t valoff[17];
  uint8_t val[256];
  uint8_t look_len[512], look_val[512];  // 0 length: code longer than 9 bits
};

bool huff_counts_ok(const uint8_t* bits);
const char* enc_check(const mx_jpeg_info* info);  // below: geometry the coders rely on

bool build_huff(const uint8_t* bits, const uint8_t* vals, Huff* h) {
  if (!huff_counts_ok(bits)) return false;
  int code = 0, k = 0;
  int total = 0;
  for (int l = 1; l <= 16; ++l) total += bits[l];
  if (total > 256) return false;
  memcpy(h->val, vals, total);
  memset(h->look_len, 0, sizeof(h->look_len));
  for (int l = 1; l <= 16; ++l) {
    // over-subscription check BEFORE any table write: every code of this length must fit in l bits
    if (code + bits[l] > (1 << l)) return false;
    h->valoff[l] = k - code;  // value index = code + valoff[l]
    for (int i = 0; i < bits[l]; ++i, ++k, ++code) {
      if (l <= 9) {
        const int shift = 9 - l;
        for (int e = 0; e < (1 << shift); ++e) {
          h->look_len[(code << shift) | e] = (uint8_t)l;
          h->look_val[(code << shift) | e] = vals[k];
        }
      }
    }
    h->maxcode[l] = bits[l] ? code - 1 : -1;
    code <<= 1;
  }
  h->maxcode[17] = 0x7fffffff;
  return true;
}

// T.81 C.2 code assignment, checked as libjpeg's jpeg_make_d_derived_tbl does when a scan USES the
// table: after the codes of length l (l up to the longest length in use) the next code must still fit
// in l bits -- no code may be all ones, so a complete table (e.g. two 1-bit codes) is rejected too
// (JERR_BAD_HUFF_TABLE). Tables a scan never uses are not checked (libjpeg derives only used ones).
bool huff_counts_ok(const uint8_t* bits) {
  int last = 0;
  for (int l = 1; l <= 16; ++l)
    if (bits[l]) last = l;
  int code = 0;
  for (int l = 1; l <= last; ++l) {
    code += bits[l];
    if (code >= (1 << l)) return false;
    code <<= 1;
  }
  return true;
}

// JPEG_MAX pixel count accepted on the hybrid path (larger frames decode on the host)
constexpr int64_t kMaxPixels = (int64_t)1 << 28;

struct Bits {
  const uint8_t* p;
  const uint8_t* end;
  uint64_t buf = 0;
  int cnt = 0;        // valid bits in buf (MSB aligned at bit 63)
  bool marker = false;  // hit a marker: feed zeros (libjpeg does the same)
  void fill() {
    while (cnt <= 56) {
      uint32_t b = 0;
      if (!marker && p < end) {
        b = *p;
        if (b == 0xFF) {
          uint8_t nx = (p + 1 < end) ? p[1] : 0;
          if (nx == 0x00) {
            p += 2;
          } else {  // RSTn / EOI / other marker: stop consuming
            marker = true;
            b = 0;
          }
        } else {
          ++p;
        }
      }
      buf |= (uint64_t)b << (56 - cnt);
      cnt += 8;
    }
  }
  int peek(int n) {
    if (cnt < n) fill();
    return (int)(buf >> (64 - n));
  }
  void skip(int n) {
    buf <<= n;
    cnt -= n;
  }
  int get(int n) {
    if (n == 0) return 0;
    int v = peek(n);
    skip(n);
    return v;
  }
};

inline int extend(int v, int s) { return v < (1 << (s - 1)) ? v - (1 << s) + 1 : v; }

inline int decode(Bits& b, const Huff& h) {
  const int look = b.peek(9);
  const int l = h.look_len[look];
  if (l) {
    b.skip(l);
    return h.look_val[look];
  }
  int code = b.get(9);
  int len = 9;
  while (len < 17 && code > h.maxcode[len]) {
    code = (code << 1) | b.get(1);
    ++len;
  }
  if (len > 16) return -1;
  return h.val[code + h.valoff[len]];
}

}  // namespace

extern "C" int mx_jpeg_parse(const uint8_t* d, int64_t n, mx_jpeg_info* info) {
  if (!d || !info || n < 4) return fail(MX_EINVAL, "jpeg: null or short buffer");
  memset(info, 0, sizeof(*info));
  if (d[0] != 0xFF || d[1] != 0xD8) return fail(MX_EINVAL, "jpeg: no SOI marker");
  int64_t i = 2;
  bool sof = false, jfif = false, adobe = false;
  int adobe_transform = -1;
  bool qdef[4] = {false, false, false, false};
  while (i + 4 <= n) {
    if (d[i] != 0xFF) {  // extraneous bytes before a marker: skipped, as libjpeg's next_marker does
      ++i;
      continue;
    }
    int m = d[i + 1];
    if (m == 0xFF) { ++i; continue; }  // fill byte
    i += 2;
    if (m == 0xD8 || (m >= 0xD0 && m <= 0xD7) || m == 0x01) continue;
    if (m == 0xD9) break;
    const int len = (d[i] << 8) | d[i + 1];
    if (len < 2 || i + len > n) return fail(MX_EINVAL, "jpeg: truncated segment");
    const uint8_t* s = d + i + 2;
    const int sl = len - 2;
    if (m == 0xC0 || m == 0xC1) {  // baseline / extended sequential, Huffman
      if (sl < 6 || s[0] != 8) return fail(MX_EUNSUPPORTED, "jpeg: only 8-bit sequential frames are supported");
      info->height = (s[1] << 8) | s[2];
      info->width = (s[3] << 8) | s[4];
      info->ncomp = s[5];
      if (info->height == 0 || info->width == 0) return fail(MX_EUNSUPPORTED, "jpeg: DNL-defined height");
      if (info->ncomp != 1 && info->ncomp != 3) return fail(MX_EUNSUPPORTED, "jpeg: 1 or 3 components only");
      if ((int64_t)info->height * info->width > kMaxPixels)
        return fail(MX_EUNSUPPORTED, "jpeg: frame larger than 2^28 pixels (decoded on the host)");
      if (sl < 6 + 3 * info->ncomp) return fail(MX_EINVAL, "jpeg: short SOF");
      for (int c = 0; c < info->ncomp; ++c) {
        info->cid[c] = s[6 + 3 * c];
        info->h[c] = s[7 + 3 * c] >> 4;
        info->v[c] = s[7 + 3 * c] & 15;
        info->tq[c] = s[8 + 3 * c];
        if (info->h[c] < 1 || info->h[c] > 2 || info->v[c] < 1 || info->v[c] > 2 || info->tq[c] > 3)
          return fail(MX_EUNSUPPORTED, "jpeg: sampling factors 1..2 and quant tables 0..3 only");
      }
      sof = true;
    } else if ((m >= 0xC2 && m <= 0xC3) || (m >= 0xC5 && m <= 0xC7) || (m >= 0xC9 && m <= 0xCB) ||
               (m >= 0xCD && m <= 0xCF)) {
      return fail(MX_EUNSUPPORTED, "jpeg: progressive / lossless / arithmetic-coded frames are not supported");
    } else if (m == 0xC4) {  // DHT
      int o = 0;
      while (o < sl) {
        const int tc = s[o] >> 4, th = s[o] & 15;
        if (tc > 1 || th > 3 || o + 17 > sl) return fail(MX_EINVAL, "jpeg: bad DHT");
        const int t = tc * 4 + th;
        int tot = 0;
        info->hbits[t][0] = 0;
        for (int l = 1; l <= 16; ++l) {
          info->hbits[t][l] = s[o + l];
          tot += s[o + l];
        }
        if (tot > 256 || o + 17 + tot > sl)
          return fail(MX_EINVAL, "jpeg: bad DHT counts");
        memcpy(info->hval[t], s + o + 17, tot);
        info->hdef[t] = 1;
        o += 17 + tot;
      }
    } else if (m == 0xDB) {  // DQT
      int o = 0;
      while (o < sl) {
        const int pq = s[o] >> 4, tq = s[o] & 15;
        if (tq > 3 || pq > 1 || o + 1 + 64 * (pq + 1) > sl) return fail(MX_EINVAL, "jpeg: bad DQT");
        for (int k = 0; k < 64; ++k)
          info->qt[tq][kNatural[k]] = pq ? (uint16_t)((s[o + 1 + 2 * k] << 8) | s[o + 2 + 2 * k]) : s[o + 1 + k];
        qdef[tq] = true;
        o += 1 + 64 * (pq + 1);
      }
    } else if (m == 0xE0) {  // APP0: a JFIF marker implies YCbCr (jdmarker.c examine_app0)
      if (sl >= 5 && memcmp(s, "JFIF\0", 5) == 0) jfif = true;
    } else if (m == 0xEE) {  // APP14: Adobe colour transform flag (jdmarker.c examine_app14)
      if (sl >= 12 && memcmp(s, "Adobe", 5) == 0) {
        adobe = true;
        adobe_transform = s[11];
      }
    } else if (m == 0xDD) {  // DRI
      if (sl < 2) return fail(MX_EINVAL, "jpeg: bad DRI");
      info->restart_interval = (s[0] << 8) | s[1];
    } else if (m == 0xDA) {  // SOS: the (single, interleaved) scan starts after this header
      if (!sof) return fail(MX_EINVAL, "jpeg: SOS before SOF");
      if (sl < 1) return fail(MX_EINVAL, "jpeg: short SOS");
      const int ns = s[0];
      if (ns != info->ncomp || sl < 1 + 2 * ns + 3)
        return fail(MX_EUNSUPPORTED, "jpeg: only single-scan (all components interleaved) images are supported");
      for (int k = 0; k < ns; ++k) {
        int c = 0;
        while (c < info->ncomp && info->cid[c] != s[1 + 2 * k]) ++c;
        if (c == info->ncomp || c != k) return fail(MX_EUNSUPPORTED, "jpeg: scan component order");
        info->td[c] = s[2 + 2 * k] >> 4;
        info->ta[c] = s[2 + 2 * k] & 15;
        if (info->td[c] > 3 || info->ta[c] > 3 || !info->hdef[info->td[c]] || !info->hdef[4 + info->ta[c]])
          return fail(MX_EINVAL, "jpeg: scan references an undefined Huffman table");
      }
      for (int c = 0; c < info->ncomp; ++c)
        if (!qdef[info->tq[c]]) return fail(MX_EINVAL, "jpeg: component references an undefined quantisation table");
      if (info->ncomp == 3) {
        // libjpeg default_decompress_parms: the colour space of a 3-component frame is YCbCr unless an
        // Adobe marker says transform 0 or (no JFIF / Adobe marker) the component IDs are 'R','G','B';
        // RGB-coded frames have no colour transform and are decoded on the host
        bool rgb = false;
        if (!jfif && adobe) {
          rgb = adobe_transform == 0;
        } else if (!jfif && !adobe) {
          rgb = info->cid[0] == 82 && info->cid[1] == 71 && info->cid[2] == 66;
        }
        if (rgb) return fail(MX_EUNSUPPORTED, "jpeg: RGB-coded frame (no YCbCr transform)");
      }
      const int ss = s[1 + 2 * ns], se = s[2 + 2 * ns], ahl = s[3 + 2 * ns];
      if (ss != 0 || se != 63 || ahl != 0) return fail(MX_EUNSUPPORTED, "jpeg: not a sequential scan");
      info->scan_off = (int32_t)(i + len);
      // geometry (jdinput.c initial_setup / per_scan_setup)
      int hm = 1, vm = 1;
      for (int c = 0; c < info->ncomp; ++c) {
        hm = info->h[c] > hm ? info->h[c] : hm;
        vm = info->v[c] > vm ? info->v[c] : vm;
      }
      if (info->ncomp == 1) {
        info->h[0] = info->v[0] = 1;
        hm = vm = 1;
      }
      info->hmax = hm;
      info->vmax = vm;
      info->mcux = cdiv(info->width, 8 * hm);
      info->mcuy = cdiv(info->height, 8 * vm);
      int64_t off = 0;
      for (int c = 0; c < info->ncomp; ++c) {
        info->bw[c] = info->mcux * info->h[c];
        info->bh[c] = info->mcuy * info->v[c];
        info->dw[c] = cdiv(info->width * info->h[c], hm);
        info->dh[c] = cdiv(info->height * info->v[c], vm);
        info->coef_off[c] = off;
        off += (int64_t)info->bw[c] * info->bh[c] * 64;
      }
      info->coef_total = off;
      if (info->ncomp == 3) {
        const bool ok = info->h[1] == 1 && info->v[1] == 1 && info->h[2] == 1 && info->v[2] == 1 &&
                        !(info->h[0] == 1 && info->v[0] == 2);
        if (!ok) return fail(MX_EUNSUPPORTED, "jpeg: chroma subsampling 4:4:4, 4:2:2 or 4:2:0 only");
      }
      return MX_OK;
    }
    i += len;
  }
  return fail(MX_EINVAL, "jpeg: no scan found");
}

extern "C" int mx_jpeg_decode_coefs(const uint8_t* d, int64_t n, const mx_jpeg_info* info, int16_t* coefs) {
  if (!d || !info || !coefs || info->scan_off <= 0 || info->scan_off > n) return fail(MX_EINVAL, "jpeg: bad arguments");
  Huff dc[4], ac[4];
  for (int c = 0; c < info->ncomp; ++c) {
    if (!build_huff(info->hbits[info->td[c]], info->hval[info->td[c]], &dc[info->td[c]]) ||
        !build_huff(info->hbits[4 + info->ta[c]], info->hval[4 + info->ta[c]], &ac[info->ta[c]]))
      return fail(MX_EINVAL, "jpeg: bad Huffman table");
  }
  memset(coefs, 0, sizeof(int16_t) * (size_t)info->coef_total);
  Bits b;
  b.p = d + info->scan_off;
  b.end = d + n;
  int pred[3] = {0, 0, 0};
  const int64_t nmcu = (int64_t)info->mcux * info->mcuy;
  const int ri = info->restart_interval;
  int64_t left = ri;
  for (int64_t mcu = 0; mcu < nmcu; ++mcu) {
    if (ri && left == 0) {  // restart: byte-align, consume RSTn, reset the DC predictors
      b.buf = 0;
      b.cnt = 0;
      b.marker = false;
      while (b.p + 1 < b.end && !(b.p[0] == 0xFF && b.p[1] >= 0xD0 && b.p[1] <= 0xD7)) ++b.p;
      if (b.p + 1 < b.end) b.p += 2;
      pred[0] = pred[1] = pred[2] = 0;
      left = ri;
    }
    const int64_t my = mcu / info->mcux, mx_ = mcu % info->mcux;
    for (int c = 0; c < info->ncomp; ++c) {
      const Huff& hd = dc[info->td[c]];
      const Huff& ha = ac[info->ta[c]];
      for (int vv = 0; vv < info->v[c]; ++vv)
        for (int hh = 0; hh < info->h[c]; ++hh) {
          const int64_t by = my * info->v[c] + vv, bx = mx_ * info->h[c] + hh;
          int16_t* blk = coefs + info->coef_off[c] + (by * info->bw[c] + bx) * 64;
          int s = decode(b, hd);
          if (s < 0 || s > 11) return fail(MX_EINVAL, "jpeg: corrupt DC code");
          if (s) pred[c] += extend(b.get(s), s);
          blk[0] = (int16_t)pred[c];
          for (int k = 1; k < 64;) {
            const int rs = decode(b, ha);
            if (rs < 0) return fail(MX_EINVAL, "jpeg: corrupt AC code");
            const int r = rs >> 4, sz = rs & 15;
            if (sz) {
              k += r;
              if (k > 63) return fail(MX_EINVAL, "jpeg: AC run past the block");
              blk[kNatural[k]] = (int16_t)extend(b.get(sz), sz);
              ++k;
            } else {
              if (r != 15) break;  // EOB
              k += 16;
            }
          }
        }
    }
    if (ri) --left;
  }
  return MX_OK;
}

// ------------------------------------------------------------------------------------------------
// Parallel entropy decode, host half: the tables and geometry mx_jpeg_entropy_decode (mx_jpeg.hip)
// uploads, and mx_jpeg_decode_coefs_chunked, the serial restatement of its passes (unstuff,
// speculative walks, synchronisation to a fixed point, scan, write, DC sums) over the walk both
// share (mx_jpeg_walk.h).
// ------------------------------------------------------------------------------------------------
namespace {
int g_jd_subseq = mx::kJdSubseqDefault;
}

namespace mx {

int jpeg_dec_subseq() { return g_jd_subseq; }

bool jpeg_dec_tables(const mx_jpeg_info* info, JdHuff* tabs) {
  memset(tabs, 0, sizeof(JdHuff) * kJdTables);
  for (int c = 0; c < info->ncomp; ++c)
    for (int ac = 0; ac < 2; ++ac) {
      const int t = ac ? 4 + info->ta[c] : info->td[c];
      Huff h;
      if (info->td[c] > 3 || info->ta[c] > 3 || !build_huff(info->hbits[t], info->hval[t], &h)) return false;
      JdHuff& o = tabs[2 * c + ac];
      memcpy(o.maxcode, h.maxcode, sizeof(o.maxcode));
      o.valoff[0] = 0;
      for (int l = 1; l <= 16; ++l) o.valoff[l] = h.valoff[l];
      memcpy(o.val, h.val, sizeof(o.val));
      for (int i = 0; i < 512; ++i) o.look[i] = (uint16_t)(h.look_len[i] ? (h.look_len[i] << 8) | h.look_val[i] : 0);
    }
  return true;
}

const char* jpeg_dec_geom(const mx_jpeg_info* info, int subseq, JdGeom* g) {
  if (const char* e = enc_check(info)) return e;
  if (info->restart_interval < 0) return "negative restart interval";
  memset(g, 0, sizeof(*g));
  g->ncomp = info->ncomp;
  g->mcux = info->mcux;
  for (int c = 0; c < 3; ++c) {
    const bool on = c < info->ncomp;
    g->h[c] = on ? info->h[c] : 1;
    g->v[c] = on ? info->v[c] : 1;
    g->bw[c] = on ? info->bw[c] : 0;
    g->coef_off[c] = on ? info->coef_off[c] : 0;
    g->first[c] = g->bpm;
    if (on) g->bpm += info->h[c] * info->v[c];
  }
  const int64_t nmcu = (int64_t)info->mcux * info->mcuy;
  g->nblk = nmcu * g->bpm;
  if (g->nblk * 64 != info->coef_total) return "inconsistent coefficient total";
  const int64_t ri = info->restart_interval;
  g->segblk = ri ? ri * g->bpm : g->nblk;
  g->nseg = ri ? (int32_t)((nmcu + ri - 1) / ri) : 1;
  g->subseq = subseq;
  return nullptr;
}

}  // namespace mx

extern "C" int mx_jpeg_entropy_decode_set_subseq(int bits) {
  if (bits < mx::kJdSubseqMin || bits > mx::kJdSubseqMax) {
    mx::set_error("mx_jpeg_entropy_decode_set_subseq: %d .. %d bits", mx::kJdSubseqMin, mx::kJdSubseqMax);
    return MX_EINVAL;
  }
  g_jd_subseq = bits;
  return MX_OK;
}

extern "C" int mx_jpeg_decode_coefs_chunked(const uint8_t* d, int64_t n, const mx_jpeg_info* info, int subseq_bits,
                                            int16_t* coefs, int32_t* status) {
  using namespace mx;
  if (!d || !info || !coefs || !status || info->scan_off <= 0 || info->scan_off >= n)
    return fail(MX_EINVAL, "jpeg_decode_coefs_chunked: bad arguments");
  const int S = subseq_bits ? subseq_bits : g_jd_subseq;
  if (S < kJdSubseqMin || S > kJdSubseqMax) return fail(MX_EINVAL, "jpeg_decode_coefs_chunked: subsequence size out of range");
  JdGeom g;
  if (const char* e = jpeg_dec_geom(info, S, &g)) return fail(MX_EINVAL, e);
  std::vector<JdHuff> tabs(kJdTables);
  if (!jpeg_dec_tables(info, tabs.data())) return fail(MX_EINVAL, "jpeg: bad Huffman table");
  int st = 0;
  // ---- 1. find and unstuff: the data of every restart segment up to its first marker
  const uint8_t* s = d + info->scan_off;
  const int64_t ns = n - info->scan_off;
  std::vector<uint32_t> words((size_t)(ns + 16) / 4 + 1, 0);  // the clean stream, zero padded
  uint8_t* clean = (uint8_t*)words.data();
  std::vector<int64_t> seg_start((size_t)g.nseg + 1, 0);
  int64_t nclean = 0, rst = 0;
  bool live = true;
  for (int64_t i = 0; i < ns; ++i) {
    const int f = jd_classify(i > 0 ? s[i - 1] : -1, s[i], i + 1 < ns ? s[i + 1] : -1);
    if (f & kJdMarker) {
      live = (f & kJdRst) != 0;
      if (live && ++rst < g.nseg) seg_start[rst] = nclean;
    } else if (live && !(f & kJdDrop)) {
      clean[nclean++] = s[i];
    }
  }
  for (int64_t j = (rst < g.nseg - 1 ? rst : g.nseg - 1) + 1; j <= g.nseg; ++j) seg_start[j] = nclean;
  if (rst != g.nseg - 1) st |= MX_JPEG_ST_RESTART;
  // ---- subsequences of every segment
  std::vector<int64_t> sub_base((size_t)g.nseg + 1, 0);
  for (int j = 0; j < g.nseg; ++j) {
    const int64_t bits = (seg_start[j + 1] - seg_start[j]) * 8;
    if (bits == 0) st |= MX_JPEG_ST_SHORT;
    sub_base[j + 1] = sub_base[j] + (bits + S - 1) / S;
  }
  const int64_t total = sub_base[g.nseg];
  std::vector<uint32_t> ex((size_t)total), lastin((size_t)total, 0), cnt((size_t)total);
  std::vector<JdLane> lane((size_t)total);
  // ---- 2. speculative walk: every lane from the assumed state (block start, DC next) at its first bit
  for (int64_t i = 0; i < total; ++i) {
    lane[i] = jd_lane(g, seg_start.data(), sub_base.data(), i);
    ex[i] = jd_walk(words.data(), tabs.data(), g, jd_unpack(0, lane[i].boundary), lane[i].limit, lane[i].end, &cnt[i]);
  }
  // ---- 3. synchronise: rounds inside a workgroup to its fixed point, passes across workgroups
  const int64_t nwg = (total + kJdLanes - 1) / kJdLanes;
  std::vector<uint32_t> next(kJdLanes);
  for (int64_t pass = 0; pass < (nwg > 0 ? nwg : 1); ++pass) {
    bool boundary_changed = false;
    for (int64_t w = pass; w < nwg; ++w) {
      const int64_t i0 = w * kJdLanes, cntw = total - i0 < kJdLanes ? total - i0 : kJdLanes;
      const uint32_t ex_last = ex[i0 + cntw - 1];
      const uint32_t head = pass == 0 || w == 0 ? lastin[i0] : ex[i0 - 1];
      for (int round = 0; round <= kJdLanes; ++round) {
        bool any = false;
        for (int64_t t = 0; t < cntw; ++t) {  // all lanes read ...
          const int64_t i = i0 + t;
          next[t] = lane[i].q == 0 ? 0 : (t == 0 ? head : ex[i - 1]);
        }
        for (int64_t t = 0; t < cntw; ++t) {  // ... then the changed ones walk
          const int64_t i = i0 + t;
          if (next[t] == lastin[i]) continue;
          any = true;
          lastin[i] = next[t];
          if (next[t] == kJdEnd) {
            ex[i] = kJdEnd;
            cnt[i] = 0;
          } else {
            ex[i] = jd_walk(words.data(), tabs.data(), g, jd_unpack(next[t], lane[i].boundary), lane[i].limit, lane[i].end,
                            &cnt[i]);
          }
        }
        if (!any) break;
      }
      if (cntw == kJdLanes && ex[i0 + cntw - 1] != ex_last) boundary_changed = true;
    }
    if (pass > 0 && !boundary_changed) break;
  }
  // ---- 4. count and place
  std::vector<int64_t> P((size_t)total + 1, 0);
  for (int64_t i = 0; i < total; ++i) P[i + 1] = P[i] + cnt[i];
  // ---- 5. write: AC values and DC differences
  memset(coefs, 0, sizeof(int16_t) * (size_t)info->coef_total);
  for (int64_t i = 0; i < total; ++i) {
    const JdLane& l = lane[i];
    const uint32_t in = l.q == 0 ? 0 : ex[i - 1];
    st |= jd_walk_store(words.data(), tabs.data(), g, jd_unpack(in, l.boundary), in == kJdEnd, l.limit, l.end,
                        P[i] - P[sub_base[l.seg]], l.quota, l.seg_first, l.last, coefs);
  }
  // ---- 6. DC prediction: running sums per component in scan order, reset at restart segments
  for (int c = 0; c < g.ncomp; ++c) {
    const int64_t ne = (int64_t)g.bw[c] * info->bh[c];
    JdSeg run{0, 0};
    for (int64_t e = 0; e < ne; ++e) {
      int reset;
      int16_t* p = coefs + jd_dc_off(g, c, e, &reset);
      run = jd_seg_combine(run, JdSeg{reset, (int32_t)*p});
      *p = (int16_t)run.v;
    }
  }
  *status = st;
  return MX_OK;
}

// ------------------------------------------------------------------------------------------------
// Encoder, host half: the tables and header libjpeg writes for jpeg_set_defaults + jpeg_set_quality
// (what PIL's Image.save(format="JPEG", quality, subsampling) produces), and the sequential Huffman
// coder of jchuff.c over coefficients in the decoder's layout. The pixel stage (colour, downsampling,
// forward DCT, quantisation) and the parallel entropy coder are in mx_jpeg.hip.
// ------------------------------------------------------------------------------------------------
namespace {

// T.81 Annex K.1 / K.2 base quantisation tables, natural order (jcparam.c std_luminance_quant_tbl)
const uint8_t kBaseQ[2][64] = {
    {16, 11, 10, 16, 24,  40,  51,  61,  12, 12, 14, 19, 26,  58,  60,  55,  14, 13, 16, 24, 40,  57,
     69, 56, 14, 17, 22,  29,  51,  87,  80, 62, 18, 22, 37,  56,  68,  109, 103, 77, 24, 35, 55,  64,
     81, 104, 113, 92, 49, 64,  78,  87,  103, 121, 120, 101, 72, 92, 95,  98,  112, 100, 103, 99},
    {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99,
     99, 99, 47, 66, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99,
     99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99}};

// T.81 Annex K.3 - K.6 Huffman tables (jcparam.c std_huff_tables): BITS[1..16], HUFFVAL
const uint8_t kStdDcBits[2][16] = {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0},
                                   {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0}};
const uint8_t kStdAcBits[2][16] = {{0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125},
                                   {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119}};
const uint8_t kStdAcVal[2][162] = {
    {1,   2,   3,   0,   4,   17,  5,   18,  33,  49,  65,  6,   19,  81,  97,  7,   34,  113, 20,  50,  129,
     145, 161, 8,   35,  66,  177, 193, 21,  82,  209, 240, 36,  51,  98,  114, 130, 9,   10,  22,  23,  24,
     25,  26,  37,  38,  39,  40,  41,  42,  52,  53,  54,  55,  56,  57,  58,  67,  68,  69,  70,  71,  72,
     73,  74,  83,  84,  85,  86,  87,  88,  89,  90,  99,  100, 101, 102, 103, 104, 105, 106, 115, 116, 117,
     118, 119, 120, 121, 122, 131, 132, 133, 134, 135, 136, 137, 138, 146, 147, 148, 149, 150, 151, 152, 153,
     154, 162, 163, 164, 165, 166, 167, 168, 169, 170, 178, 179, 180, 181, 182, 183, 184, 185, 186, 194, 195,
     196, 197, 198, 199, 200, 201, 202, 210, 211, 212, 213, 214, 215, 216, 217, 218, 225, 226, 227, 228, 229,
     230, 231, 232, 233, 234, 241, 242, 243, 244, 245, 246, 247, 248, 249, 250},
    {0,   1,   2,   3,   17,  4,   5,   33,  49,  6,   18,  65,  81,  7,   97,  113, 19,  34,  50,  129, 8,
     20,  66,  145, 161, 177, 193, 9,   35,  51,  82,  240, 21,  98,  114, 209, 10,  22,  36,  52,  225, 37,
     241, 23,  24,  25,  26,  38,  39,  40,  41,  42,  53,  54,  55,  56,  57,  58,  67,  68,  69,  70,  71,
     72,  73,  74,  83,  84,  85,  86,  87,  88,  89,  90,  99,  100, 101, 102, 103, 104, 105, 106, 115, 116,
     117, 118, 119, 120, 121, 122, 130, 131, 132, 133, 134, 135, 136, 137, 138, 146, 147, 148, 149, 150, 151,
     152, 153, 154, 162, 163, 164, 165, 166, 167, 168, 169, 170, 178, 179, 180, 181, 182, 183, 184, 185, 186,
     194, 195, 196, 197, 198, 199, 200, 201, 202, 210, 211, 212, 213, 214, 215, 216, 217, 218, 226, 227, 228,
     229, 230, 231, 232, 233, 234, 242, 243, 244, 245, 246, 247, 248, 249, 250}};

// bounded byte sink: never writes at or past cap; `n` keeps counting so the caller learns the need
struct Sink {
  uint8_t* p;
  int64_t cap, n = 0;
  void put(int b) {
    if (n < cap) p[n] = (uint8_t)b;
    ++n;
  }
  void put2(int v) {
    put(v >> 8);
    put(v & 255);
  }
};

int huff_total(const uint8_t* bits) {
  int t = 0;
  for (int l = 1; l <= 16; ++l) t += bits[l];
  return t;
}

void write_header(const mx_jpeg_info* info, Sink& s) {
  s.put2(0xFFD8);
  s.put2(0xFFE0);  // APP0: JFIF 1.01, no units, 1:1 aspect, no thumbnail (jcmarker.c emit_jfif_app0)
  s.put2(16);
  const uint8_t jfif[14] = {'J', 'F', 'I', 'F', 0, 1, 1, 0, 0, 1, 0, 1, 0, 0};
  for (int k = 0; k < 14; ++k) s.put(jfif[k]);
  bool qdone[4] = {false, false, false, false};
  for (int c = 0; c < info->ncomp; ++c) {  // one DQT segment per table, in order of first use, zig-zag
    const int t = info->tq[c];
    if (qdone[t]) continue;
    qdone[t] = true;
    s.put2(0xFFDB);
    s.put2(67);
    s.put(t);
    for (int k = 0; k < 64; ++k) s.put(info->qt[t][kNatural[k]]);
  }
  s.put2(0xFFC0);
  s.put2(8 + 3 * info->ncomp);
  s.put(8);
  s.put2(info->height);
  s.put2(info->width);
  s.put(info->ncomp);
  for (int c = 0; c < info->ncomp; ++c) {
    s.put(info->cid[c]);
    s.put((info->h[c] << 4) | info->v[c]);
    s.put(info->tq[c]);
  }
  bool hdone[8] = {false, false, false, false, false, false, false, false};
  for (int c = 0; c < info->ncomp; ++c)  // DC then AC table of each component, once each (emit_dht)
    for (int ac = 0; ac < 2; ++ac) {
      const int t = ac ? 4 + info->ta[c] : info->td[c];
      if (hdone[t]) continue;
      hdone[t] = true;
      const int tot = huff_total(info->hbits[t]);
      s.put2(0xFFC4);
      s.put2(19 + tot);
      s.put(ac ? 0x10 | info->ta[c] : info->td[c]);
      for (int l = 1; l <= 16; ++l) s.put(info->hbits[t][l]);
      for (int k = 0; k < tot; ++k) s.put(info->hval[t][k]);
    }
  s.put2(0xFFDA);
  s.put2(6 + 2 * info->ncomp);
  s.put(info->ncomp);
  for (int c = 0; c < info->ncomp; ++c) {
    s.put(info->cid[c]);
    s.put((info->td[c] << 4) | info->ta[c]);
  }
  s.put(0);
  s.put(63);
  s.put(0);
}

// what both coders need of an info, whoever filled it
const char* enc_check(const mx_jpeg_info* info) {
  if (!info) return "jpeg encode: null info";
  if (info->ncomp != 1 && info->ncomp != 3) return "jpeg encode: 1 or 3 components";
  if (info->width < 1 || info->height < 1 || info->mcux < 1 || info->mcuy < 1 || info->coef_total < 1)
    return "jpeg encode: empty geometry (mx_jpeg_parse or mx_jpeg_encode_info first)";
  int64_t off = 0;
  for (int c = 0; c < info->ncomp; ++c) {
    if (info->h[c] < 1 || info->h[c] > 2 || info->v[c] < 1 || info->v[c] > 2 || info->tq[c] < 0 || info->tq[c] > 3 ||
        info->td[c] > 3 || info->ta[c] > 3)
      return "jpeg encode: bad sampling factors or table numbers";
    if (info->bw[c] != info->mcux * info->h[c] || info->bh[c] != info->mcuy * info->v[c] || info->coef_off[c] != off)
      return "jpeg encode: inconsistent block geometry";
    off += (int64_t)info->bw[c] * info->bh[c] * 64;
  }
  if (off != info->coef_total) return "jpeg encode: inconsistent coefficient total";
  return nullptr;
}

struct BitSink {
  Sink s;
  uint64_t acc = 0;
  int cnt = 0;
  void put(uint32_t v, int n) {  // n <= 32 bits, MSB first; a 0x00 is stuffed after every 0xFF byte
    acc = (acc << n) | v;
    cnt += n;
    while (cnt >= 8) {
      const int b = (int)((acc >> (cnt - 8)) & 255);
      s.put(b);
      if (b == 255) s.put(0);
      cnt -= 8;
    }
    acc &= ((uint64_t)1 << cnt) - 1;
  }
};

inline int nbits_of(int a) { return a ? 32 - __builtin_clz((unsigned)a) : 0; }

}  // namespace

namespace mx {
const char* jpeg_enc_check(const mx_jpeg_info* info) { return enc_check(info); }

// the Annex K base table t (0 luma, 1 chroma) mx_jpeg_encode_info scales: the round-trip kernel
// (mx_jpeg.hip) scales the same 64 bytes on the device
const uint8_t* jpeg_base_quant(int t) { return kBaseQ[t]; }

// Encoding table of one DHT table (T.81 C.2, jchuff.c jpeg_make_c_derived_tbl): tab[symbol] =
// code << 8 | length, 0 for a symbol without a code. Shared with the device coder (mx_jpeg.hip).
bool jpeg_enc_table(const uint8_t* bits, const uint8_t* vals, uint32_t* tab) {
  if (!huff_counts_ok(bits) || huff_total(bits) > 256) return false;
  memset(tab, 0, 256 * sizeof(uint32_t));
  uint32_t code = 0;
  int k = 0;
  for (int l = 1; l <= 16; ++l) {
    for (int i = 0; i < bits[l]; ++i, ++k, ++code) {
      if (tab[vals[k]]) return false;  // duplicate symbol
      tab[vals[k]] = (code << 8) | (uint32_t)l;
    }
    code <<= 1;
  }
  return true;
}
}  // namespace mx

extern "C" int mx_jpeg_encode_info(int width, int height, int quality, int subsampling, mx_jpeg_info* out) {
  if (!out) return fail(MX_EINVAL, "jpeg_encode_info: null info");
  if (width < 1 || height < 1) return fail(MX_EINVAL, "jpeg_encode_info: empty image");
  if (quality < 1 || quality > 100) return fail(MX_EINVAL, "jpeg_encode_info: quality must be 1..100");
  if (subsampling != 0 && subsampling != 2)
    return fail(MX_EINVAL, "jpeg_encode_info: subsampling 0 (4:4:4) or 2 (4:2:0) only");
  if (width > 65535 || height > 65535 || (int64_t)width * height > kMaxPixels)
    return fail(MX_EUNSUPPORTED, "jpeg_encode_info: frame larger than 65535 a side or 2^28 pixels");
  memset(out, 0, sizeof(*out));
  out->width = width;
  out->height = height;
  out->ncomp = 3;
  const int hm = subsampling == 2 ? 2 : 1;
  out->hmax = out->vmax = hm;
  out->mcux = cdiv(width, 8 * hm);
  out->mcuy = cdiv(height, 8 * hm);
  int64_t off = 0;
  for (int c = 0; c < 3; ++c) {
    out->cid[c] = (uint8_t)(c + 1);
    out->h[c] = out->v[c] = c == 0 ? hm : 1;
    out->tq[c] = out->td[c] = out->ta[c] = c == 0 ? 0 : 1;
    out->bw[c] = out->mcux * out->h[c];
    out->bh[c] = out->mcuy * out->v[c];
    out->dw[c] = cdiv(width * out->h[c], hm);
    out->dh[c] = cdiv(height * out->v[c], hm);
    out->coef_off[c] = off;
    off += (int64_t)out->bw[c] * out->bh[c] * 64;
  }
  out->coef_total = off;
  // jcparam.c jpeg_quality_scaling + jpeg_add_quant_table (force_baseline)
  const int scale = quality < 50 ? 5000 / quality : 200 - 2 * quality;
  for (int t = 0; t < 2; ++t)
    for (int k = 0; k < 64; ++k) {
      int q = (kBaseQ[t][k] * scale + 50) / 100;
      out->qt[t][k] = (uint16_t)(q < 1 ? 1 : (q > 255 ? 255 : q));
    }
  for (int t = 0; t < 2; ++t) {
    memcpy(&out->hbits[t][1], kStdDcBits[t], 16);
    for (int k = 0; k < 12; ++k) out->hval[t][k] = (uint8_t)k;
    memcpy(&out->hbits[4 + t][1], kStdAcBits[t], 16);
    memcpy(out->hval[4 + t], kStdAcVal[t], 162);
    out->hdef[t] = out->hdef[4 + t] = 1;
  }
  Sink s{nullptr, 0};
  write_header(out, s);
  out->scan_off = (int32_t)s.n;
  return MX_OK;
}

extern "C" int mx_jpeg_write_header(const mx_jpeg_info* info, uint8_t* out, int64_t cap, int64_t* n) {
  if (const char* e = enc_check(info)) return fail(MX_EINVAL, e);
  if (!out || !n || cap < 0) return fail(MX_EINVAL, "jpeg_write_header: null argument");
  for (int c = 0; c < info->ncomp; ++c)
    for (int k = 0; k < 64; ++k)
      if (info->qt[info->tq[c]][k] < 1 || info->qt[info->tq[c]][k] > 255)
        return fail(MX_EUNSUPPORTED, "jpeg_write_header: 8-bit quantisation tables only");
  Sink s{out, cap};
  write_header(info, s);
  *n = s.n;
  if (s.n > cap) {
    mx::set_error("jpeg_write_header: %lld bytes required, %lld given", (long long)s.n, (long long)cap);
    return MX_EINVAL;
  }
  return MX_OK;
}

// Worst-case bytes of the entropy-coded segment: a block is at most 64 * 26 + 27 bits, every byte may
// need a stuffed zero. Sizes the output of mx_jpeg_encode_coefs and of mx_jpeg_entropy.
extern "C" int64_t mx_jpeg_scan_bound(const mx_jpeg_info* info) {
  if (enc_check(info)) return 0;
  const int64_t bits = (info->coef_total / 64) * (64 * 26 + 27);
  return 2 * ((bits + 7) / 8 + 1);
}

extern "C" int mx_jpeg_encode_coefs(const mx_jpeg_info* info, const int16_t* coefs, uint8_t* out, int64_t cap,
                                    int64_t* n) {
  if (const char* e = enc_check(info)) return fail(MX_EINVAL, e);
  if (!coefs || !out || !n || cap < 0) return fail(MX_EINVAL, "jpeg_encode_coefs: null argument");
  if (info->restart_interval != 0) return fail(MX_EUNSUPPORTED, "jpeg_encode_coefs: restart intervals are not supported");
  uint32_t dc[3][256], ac[3][256];
  for (int c = 0; c < info->ncomp; ++c)
    if (!mx::jpeg_enc_table(info->hbits[info->td[c]], info->hval[info->td[c]], dc[c]) ||
        !mx::jpeg_enc_table(info->hbits[4 + info->ta[c]], info->hval[4 + info->ta[c]], ac[c]))
      return fail(MX_EINVAL, "jpeg_encode_coefs: bad Huffman table");
  BitSink b;
  b.s = Sink{out, cap};
  int pred[3] = {0, 0, 0};
  const int64_t nmcu = (int64_t)info->mcux * info->mcuy;
  for (int64_t mcu = 0; mcu < nmcu; ++mcu) {
    const int64_t my = mcu / info->mcux, mx_ = mcu % info->mcux;
    for (int c = 0; c < info->ncomp; ++c)
      for (int vv = 0; vv < info->v[c]; ++vv)
        for (int hh = 0; hh < info->h[c]; ++hh) {
          const int64_t by = my * info->v[c] + vv, bx = mx_ * info->h[c] + hh;
          const int16_t* blk = coefs + info->coef_off[c] + (by * info->bw[c] + bx) * 64;
          // jchuff.c encode_one_block: DC difference, then (run, size) pairs over the zig-zag sequence
          int d = blk[0] - pred[c];
          pred[c] = blk[0];
          int nb = nbits_of(d < 0 ? -d : d);
          if (nb > 11 || !dc[c][nb]) return fail(MX_EINVAL, "jpeg_encode_coefs: DC difference without a code");
          b.put(dc[c][nb] >> 8, (int)(dc[c][nb] & 255));
          if (nb) b.put((uint32_t)(d < 0 ? d - 1 : d) & ((1u << nb) - 1), nb);
          int r = 0;
          for (int k = 1; k < 64; ++k) {
            const int v = blk[kNatural[k]];
            if (v == 0) {
              ++r;
              continue;
            }
            for (; r > 15; r -= 16) {
              if (!ac[c][0xF0]) return fail(MX_EINVAL, "jpeg_encode_coefs: ZRL without a code");
              b.put(ac[c][0xF0] >> 8, (int)(ac[c][0xF0] & 255));
            }
            nb = nbits_of(v < 0 ? -v : v);
            const uint32_t e = nb > 10 ? 0 : ac[c][(r << 4) | nb];
            if (!e) return fail(MX_EINVAL, "jpeg_encode_coefs: AC coefficient without a code");
            b.put(e >> 8, (int)(e & 255));
            b.put((uint32_t)(v < 0 ? v - 1 : v) & ((1u << nb) - 1), nb);
            r = 0;
          }
          if (r > 0) {
            if (!ac[c][0]) return fail(MX_EINVAL, "jpeg_encode_coefs: EOB without a code");
            b.put(ac[c][0] >> 8, (int)(ac[c][0] & 255));
          }
        }
  }
  if (b.cnt) b.put((1u << (8 - b.cnt)) - 1, 8 - b.cnt);  // flush_bits: pad the last byte with ones
  *n = b.s.n;
  if (b.s.n > cap) {
    mx::set_error("jpeg_encode_coefs: %lld bytes required, %lld given (mx_jpeg_scan_bound is the worst case)",
                  (long long)b.s.n, (long long)cap);
    return MX_EINVAL;
  }
  return MX_OK;
}
