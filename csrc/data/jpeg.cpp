// Baseline / extended-sequential Huffman JPEG entropy decoder (see jpeg.h). Plain C++, no
// dependency; every read of the input goes through a bounds check and every coefficient store
// lands inside a window whose size was checked against the capacity before the scan is decoded.
#include "jpeg.h"

#include <cstring>

namespace hcbjpeg {

namespace {

const uint8_t ZIGZAG[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                            41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                            30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

struct Huff {
  bool defined = false;
  int nvals = 0;
  uint8_t vals[256];
  int32_t maxcode[18];    // largest code of each length, -1 when the length has none
  int32_t valoffset[17];  // index of the first value of a length minus its first code
  uint16_t fast[512];     // 9-bit lookahead: (length << 8) | value, 0 when the code is longer
};

// false: the table's counts do not form a prefix code
bool build_huff(Huff& h, const uint8_t* counts, const uint8_t* vals, int nvals) {
  h.nvals = nvals;
  std::memcpy(h.vals, vals, nvals);
  std::memset(h.fast, 0, sizeof(h.fast));
  int code = 0, k = 0;
  for (int l = 1; l <= 16; ++l) {
    const int c = counts[l - 1];
    if (c == 0) {
      h.maxcode[l] = -1;
      h.valoffset[l] = 0;
    } else {
      if (code + c > (1 << l)) return false;
      h.valoffset[l] = k - code;
      if (l <= 9)
        for (int i = 0; i < c; ++i) {
          const int first = (code + i) << (9 - l);
          for (int j = 0; j < (1 << (9 - l)); ++j) h.fast[first + j] = (uint16_t)((l << 8) | vals[k + i]);
        }
      code += c;
      k += c;
      h.maxcode[l] = code - 1;
    }
    code <<= 1;
  }
  h.maxcode[17] = 0x7fffffff;
  h.defined = true;
  return true;
}

// Bit reader over the entropy-coded segment: removes 0xFF00 stuffing, stops at a marker or the end
// of the buffer and from there on supplies zero bits that may be looked at but not consumed.
struct Bits {
  const uint8_t* p;
  size_t n, pos;
  uint64_t buf = 0;
  int cnt = 0;  // bits in buf
  int pad = 0;  // of which padding (at the low end)
  bool stopped = false;

  void fill() {
    while (cnt <= 56) {
      if (!stopped && pos < n) {
        const uint8_t b = p[pos];
        if (b == 0xFF) {
          if (pos + 1 < n && p[pos + 1] == 0x00) {
            pos += 2;
          } else {
            stopped = true;
            continue;
          }
        } else {
          pos += 1;
        }
        buf = (buf << 8) | b;
        cnt += 8;
      } else {
        stopped = true;
        buf <<= 8;
        cnt += 8;
        pad += 8;
      }
    }
  }
  // k in [1, 16]
  inline uint32_t peek(int k) {
    if (cnt < k) fill();
    return (uint32_t)(buf >> (cnt - k)) & ((1u << k) - 1u);
  }
  inline bool skip(int k) {
    cnt -= k;
    return cnt >= pad;
  }
  void reset() {
    buf = 0;
    cnt = pad = 0;
    stopped = false;
  }
};

inline int decode_symbol(Bits& b, const Huff& h) {
  const uint32_t look = b.peek(16);
  const uint16_t f = h.fast[look >> 7];
  if (f) {
    if (!b.skip(f >> 8)) return -1;
    return f & 0xff;
  }
  int l = 10;
  while (l <= 16 && (int32_t)(look >> (16 - l)) > h.maxcode[l]) ++l;
  if (l > 16) return -1;
  const int idx = (int)(look >> (16 - l)) + h.valoffset[l];
  if (idx < 0 || idx >= h.nvals) return -1;
  if (!b.skip(l)) return -1;
  return h.vals[idx];
}

// s in [1, 15]: s raw bits, sign-extended the JPEG way; false when the stream ended
inline bool receive_extend(Bits& b, int s, int& v) {
  const int raw = (int)b.peek(s);
  if (!b.skip(s)) return false;
  v = raw < (1 << (s - 1)) ? raw - (1 << s) + 1 : raw;
  return true;
}

// One block: DC difference onto pred, AC run lengths; out == nullptr decodes without storing.
// Returns nullptr or the reason the stream is unusable.
inline const char* decode_block(Bits& b, const Huff& dc, const Huff& ac, int& pred, int16_t* out) {
  int s = decode_symbol(b, dc);
  if (s < 0) return "truncated or invalid Huffman code";
  if (s > 15) return "DC size out of range";
  if (s) {
    int d;
    if (!receive_extend(b, s, d)) return "truncated entropy data";
    pred += d;
  }
  if (pred < -32768 || pred > 32767) return "DC coefficient out of range";
  if (out) out[0] = (int16_t)pred;
  int k = 1;
  while (k < 64) {
    const int rs = decode_symbol(b, ac);
    if (rs < 0) return "truncated or invalid Huffman code";
    const int r = rs >> 4, sz = rs & 15;
    if (sz == 0) {
      if (r != 15) break;  // end of block
      k += 16;
      continue;
    }
    k += r;
    if (k > 63) return "AC run past the end of the block";
    int v;
    if (!receive_extend(b, sz, v)) return "truncated entropy data";
    if (out) out[ZIGZAG[k]] = (int16_t)v;
    ++k;
  }
  if (k > 64) return "AC run past the end of the block";
  return nullptr;
}

struct Comp {
  int id = 0, h = 1, v = 1, tq = 0, td = 0, ta = 0;
};

inline int u16(const uint8_t* p) { return (p[0] << 8) | p[1]; }

}  // namespace

long jpeg_entropy_decode(const uint8_t* data, size_t n, int wy, int wx, int wh, int ww, uint8_t* dst, size_t cap,
                         const char** reason) {
#define DECLINE(why)   \
  do {                 \
    *reason = (why);   \
    return -1;         \
  } while (0)
  if ((reinterpret_cast<uintptr_t>(dst) & 15) != 0) DECLINE("destination not 16-byte aligned");
  if (n < 4 || data[0] != 0xFF || data[1] != 0xD8) DECLINE("not a JPEG");
  uint16_t qt[4][64];
  bool qt_def[4] = {false, false, false, false};
  std::memset(qt, 0, sizeof(qt));
  // heap-free: 8 tables of about 1.9 KB on the stack
  Huff huff[2][4];
  Comp comp[3];
  int ncomp = 0, H = 0, W = 0, restart = 0;
  bool have_sof = false;
  size_t pos = 2;
  for (;;) {
    // next marker: 0xFF, any number of 0xFF fill bytes, the code
    if (pos >= n) DECLINE("truncated before the scan");
    if (data[pos] != 0xFF) DECLINE("marker expected");
    while (pos < n && data[pos] == 0xFF) ++pos;
    if (pos >= n) DECLINE("truncated before the scan");
    const int m = data[pos++];
    if (m == 0xD8 || (m >= 0xD0 && m <= 0xD7) || m == 0x01 || m == 0x00) DECLINE("unexpected marker");
    if (m == 0xD9) DECLINE("no scan before the end of the image");
    if (pos + 2 > n) DECLINE("truncated segment");
    const int len = u16(data + pos);
    if (len < 2 || pos + (size_t)len > n) DECLINE("truncated segment");
    const uint8_t* s = data + pos + 2;
    const int sl = len - 2;
    pos += len;
    if (m == 0xC0 || m == 0xC1) {
      if (have_sof) DECLINE("more than one frame header");
      if (sl < 6) DECLINE("short frame header");
      if (s[0] != 8) DECLINE("sample precision is not 8 bits");
      H = u16(s + 1);
      W = u16(s + 3);
      ncomp = s[5];
      if (H == 0 || W == 0) DECLINE("zero image size");
      if (ncomp == 4) DECLINE("4 components (CMYK)");
      if (ncomp != 1 && ncomp != 3) DECLINE("component count is not 1 or 3");
      if (sl != 6 + 3 * ncomp) DECLINE("inconsistent frame header");
      for (int c = 0; c < ncomp; ++c) {
        comp[c].id = s[6 + 3 * c];
        comp[c].h = s[7 + 3 * c] >> 4;
        comp[c].v = s[7 + 3 * c] & 15;
        comp[c].tq = s[8 + 3 * c];
        if (comp[c].tq > 3) DECLINE("quantisation table index out of range");
        if (comp[c].h < 1 || comp[c].h > 4 || comp[c].v < 1 || comp[c].v > 4) DECLINE("invalid sampling factors");
      }
      if (ncomp == 1) {
        comp[0].h = comp[0].v = 1;  // a single-component scan is not interleaved: the factors do not matter
      } else {
        if (comp[0].h > 2 || comp[0].v > 2 || comp[1].h != 1 || comp[1].v != 1 || comp[2].h != 1 || comp[2].v != 1)
          DECLINE("unusual sampling factors");
      }
      have_sof = true;
    } else if (m == 0xC2) {
      DECLINE("progressive");
    } else if (m == 0xC9 || m == 0xCA || m == 0xCB || m == 0xCD || m == 0xCE || m == 0xCF || m == 0xCC) {
      DECLINE("arithmetic coded");
    } else if (m == 0xC3 || m == 0xC5 || m == 0xC6 || m == 0xC7) {
      DECLINE("lossless or hierarchical");
    } else if (m == 0xDB) {
      int o = 0;
      while (o < sl) {
        const int pq = s[o] >> 4, tq = s[o] & 15;
        if (pq > 1 || tq > 3) DECLINE("invalid quantisation table");
        const int need = 1 + 64 * (pq + 1);
        if (o + need > sl) DECLINE("truncated quantisation table");
        for (int i = 0; i < 64; ++i)
          qt[tq][ZIGZAG[i]] = pq ? (uint16_t)u16(s + o + 1 + 2 * i) : (uint16_t)s[o + 1 + i];
        qt_def[tq] = true;
        o += need;
      }
    } else if (m == 0xC4) {
      int o = 0;
      while (o < sl) {
        if (o + 17 > sl) DECLINE("truncated Huffman table");
        const int tc = s[o] >> 4, th = s[o] & 15;
        if (tc > 1 || th > 3) DECLINE("invalid Huffman table");
        int total = 0;
        for (int i = 0; i < 16; ++i) total += s[o + 1 + i];
        if (total > 256 || o + 17 + total > sl) DECLINE("truncated Huffman table");
        if (!build_huff(huff[tc][th], s + o + 1, s + o + 17, total)) DECLINE("invalid Huffman table");
        o += 17 + total;
      }
    } else if (m == 0xDD) {
      if (sl != 2) DECLINE("invalid restart interval");
      restart = u16(s);
    } else if (m == 0xDA) {
      if (!have_sof) DECLINE("scan before the frame header");
      if (sl < 1) DECLINE("short scan header");
      const int ns = s[0];
      if (ns != ncomp) DECLINE("multi-scan (not one interleaved scan)");
      if (sl != 4 + 2 * ns) DECLINE("inconsistent scan header");
      for (int c = 0; c < ns; ++c) {
        if (s[1 + 2 * c] != comp[c].id) DECLINE("scan components out of frame order");
        comp[c].td = s[2 + 2 * c] >> 4;
        comp[c].ta = s[2 + 2 * c] & 15;
        if (comp[c].td > 3 || comp[c].ta > 3) DECLINE("Huffman table index out of range");
        if (!huff[0][comp[c].td].defined || !huff[1][comp[c].ta].defined) DECLINE("missing Huffman table");
        if (!qt_def[comp[c].tq]) DECLINE("missing quantisation table");
      }
      if (s[1 + 2 * ns] != 0 || s[2 + 2 * ns] != 63 || s[3 + 2 * ns] != 0) DECLINE("not a sequential scan");
      break;
    }
    // APPn, COM and anything else: skipped by its length
  }

  // ---- the window
  if (wh <= 0 || ww <= 0) {
    wy = wx = 0;
    wh = H;
    ww = W;
  }
  if (wy < 0 || wx < 0 || wy > H - wh || wx > W - ww) DECLINE("crop window outside the image");
  const int hs = comp[0].h, vs = comp[0].v;
  const int mcux = (W + 8 * hs - 1) / (8 * hs), mcuy = (H + 8 * vs - 1) / (8 * vs);
  // rows / columns of the least-resolved plane the crop touches, with the filter's margin where
  // that plane is subsampled, clipped to the plane; then MCU units
  auto span = [](int lo, int len, int f, int full, int& m0, int& m1) {
    int c0 = lo, c1 = lo + len - 1;
    if (f == 2) {
      const int cn = (full + 1) / 2;
      c0 = (lo >> 1) - 1;
      c1 = ((lo + len - 1) >> 1) + 1;
      if (c0 < 0) c0 = 0;
      if (c1 > cn - 1) c1 = cn - 1;
      m0 = c0 / 8;
      m1 = c1 / 8;
    } else {
      m0 = c0 / 8;
      m1 = c1 / 8;
    }
  };
  int mx0, mx1, my0, my1;
  span(wx, ww, hs, W, mx0, mx1);
  span(wy, wh, vs, H, my0, my1);
  if (mx1 > mcux - 1 || my1 > mcuy - 1) DECLINE("inconsistent window");
  const int mw = mx1 - mx0 + 1, mh = my1 - my0 + 1;

  int32_t hdr[HDR_INTS];
  std::memset(hdr, 0, sizeof(hdr));
  hdr[HDR_MAGIC_AT] = HDR_MAGIC;
  hdr[HDR_NCOMP] = ncomp;
  hdr[HDR_HS] = hs;
  hdr[HDR_VS] = vs;
  hdr[HDR_H] = H;
  hdr[HDR_W] = W;
  hdr[HDR_CY] = wy;
  hdr[HDR_CX] = wx;
  hdr[HDR_CH] = wh;
  hdr[HDR_CW] = ww;
  int64_t nblocks = 0;
  int64_t first[3] = {0, 0, 0};
  int cbw[3] = {0, 0, 0};
  for (int c = 0; c < ncomp; ++c) {
    const int ch = comp[c].h, cv = comp[c].v;
    int32_t* f = hdr + HDR_COMP + 6 * c;
    f[0] = mx0 * ch;
    f[1] = my0 * cv;
    f[2] = mw * ch;
    f[3] = mh * cv;
    f[4] = comp[c].tq;
    if (nblocks > 0x7fffffff) DECLINE("window does not fit the capacity");
    f[5] = (int32_t)nblocks;
    first[c] = nblocks;
    cbw[c] = mw * ch;
    nblocks += (int64_t)f[2] * f[3];
  }
  hdr[HDR_OY] = wy - 8 * hdr[HDR_COMP + 1];
  hdr[HDR_OX] = wx - 8 * hdr[HDR_COMP + 0];
  const int64_t total = (int64_t)COEF_OFFSET + nblocks * 128;
  if (nblocks > 0x7fffffff || total > 0x7fffffff || (uint64_t)total > (uint64_t)cap)
    DECLINE("window does not fit the capacity");
  hdr[HDR_NBLOCKS] = (int32_t)nblocks;
  hdr[HDR_BYTES] = (int32_t)total;
  int16_t* coef = reinterpret_cast<int16_t*>(dst + COEF_OFFSET);
  std::memset(coef, 0, (size_t)nblocks * 128);

  // ---- the scan: every MCU up to the last row the window needs
  Bits b;
  b.p = data;
  b.n = n;
  b.pos = pos;
  int pred[3] = {0, 0, 0};
  int64_t mcu = 0;
  const int last_row = my1;
  for (int my = 0; my <= last_row; ++my) {
    const bool row_in = my >= my0;
    for (int mx = 0; mx < mcux; ++mx, ++mcu) {
      if (restart && mcu && mcu % restart == 0) {
        b.fill();
        if (b.cnt - b.pad >= 8) DECLINE("entropy data left before a restart marker");
        b.reset();
        size_t q = b.pos;
        if (q >= n || data[q] != 0xFF) DECLINE("restart marker expected");
        while (q < n && data[q] == 0xFF) ++q;
        if (q >= n) DECLINE("truncated at a restart marker");
        if (data[q] != 0xD0 + (int)((mcu / restart - 1) & 7)) DECLINE("wrong restart marker");
        b.pos = q + 1;
        pred[0] = pred[1] = pred[2] = 0;
      }
      const bool in = row_in && mx >= mx0 && mx <= mx1;
      for (int c = 0; c < ncomp; ++c) {
        const Huff& dc = huff[0][comp[c].td];
        const Huff& ac = huff[1][comp[c].ta];
        for (int v = 0; v < comp[c].v; ++v)
          for (int h = 0; h < comp[c].h; ++h) {
            int16_t* out = nullptr;
            if (in) {
              const int64_t by = (int64_t)(my - my0) * comp[c].v + v, bx = (int64_t)(mx - mx0) * comp[c].h + h;
              out = coef + (first[c] + by * cbw[c] + bx) * 64;
            }
            const char* why = decode_block(b, dc, ac, pred[c], out);
            if (why) DECLINE(why);
          }
      }
    }
  }
  if (last_row == mcuy - 1) {
    // the scan was decoded to its end: the end-of-image marker has to follow
    b.fill();
    if (b.cnt - b.pad >= 8) DECLINE("entropy data left after the last MCU");
    size_t q = b.pos;
    if (q >= n || data[q] != 0xFF) DECLINE("truncated: no end-of-image marker");
    while (q < n && data[q] == 0xFF) ++q;
    if (q >= n || data[q] != 0xD9) DECLINE("truncated: no end-of-image marker");
  }
  std::memcpy(dst, hdr, sizeof(hdr));
  std::memcpy(dst + QT_OFFSET, qt, sizeof(qt));
  return (long)total;
#undef DECLINE
}

}  // namespace hcbjpeg
