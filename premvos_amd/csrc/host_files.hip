// Host-only translation unit (no kernels): the files of ONE frame -- <frame>.flo, general / specific / combined / refined proposal
// JSON -- written from the arrays a rank's results consist of, in one call that never touches the Python interpreter.
//
// Why it exists: the merge rank of a gathered 8-GPU job turns ~430 frames/s of gathered buffers into files
// (premvos_amd/stream.py: DeviceGather) while its own stage threads drive ~1500 kernel launches per chunk from Python.  Per frame
// the host work is small (3 ms) but two thirds of it held the interpreter lock (numpy scalar arithmetic of the box conversion, the
// JSON encoder, string slicing): four writer threads scaled NEGATIVELY (tools/dev/ingest_host_bench.py: 3.3 ms of writer time per
// frame with one thread, 15.9 ms with four) and slowed the rank's own launches by 15 %.  ctypes releases the lock for the duration
// of a foreign call, so this function runs on N threads at once.
//
// The bytes are the ones the Python writers produce -- and those are the reference's:
//   .flo           script_pwc_multi.py:16-31                      (tag 202021.25f, int32 W, int32 H, H*W*2 float32)
//   proposal JSON  proposal_net/eval.py:93-94 + train.py:388-428  boxes / scale and clip in float32, xywh, round(x, 1) / round(s, 2)
//                  on numpy float32 scalars (= multiply, rint, divide in float32), float(...), json.dump: repr of the double
//   combined       combine_general_and_specific.py:33             (general + specific)
//   refined        FewShotSegmentationForwarder.py:137-155        + "segmentation": {"size": [h, w], "counts": str}, "conf_score": str(float32)
// Number formatting: Python's float repr = the shortest decimal string that reads back as the same double (exponent form below 1e-4
// and from 1e16); numpy's str(float32) = the shortest that reads back as the same float (same thresholds, "1.0" / "1e-05" shapes).
// Both are produced here by searching the digit count with the C library's correctly rounded printf / strtod; tests/test_cpu_host_files.py
// compares a few hundred thousand values and whole frames against the interpreter.
#include <errno.h>
#include <fcntl.h>
#include <math.h>
#include <stdlib.h>
#include <string.h>
#include <sys/uio.h>
#include <unistd.h>

#include <string>

#include "common.h"

namespace {

// Shortest digits d1 d2 ... dn (no trailing zeros) and decimal point position `decpt` (value = 0.d1d2...dn x 10^decpt) of a finite,
// non-zero |x|; SINGLE: shortest that identifies the float, else the double.
template <bool SINGLE>
int shortest_digits(double x, char* digits, int* decpt) {
  const int maxp = SINGLE ? 9 : 17;
  char buf[40];
  auto ok = [&](int p) {
    snprintf(buf, sizeof(buf), "%.*e", p - 1, x);
    return SINGLE ? strtof(buf, nullptr) == (float)x : strtod(buf, nullptr) == x;
  };
  int lo = 1, hi = maxp;                     // smallest p that round-trips (round-tripping is monotone in p)
  // (the doubles of this file are float32 values widened: nearly all need 16 or 17 digits -- probe the top first)
  if (!SINGLE) {
    if (!ok(15)) lo = 16; else hi = 15;
  }
  while (lo < hi) {
    const int mid = (lo + hi) / 2;
    if (ok(mid)) hi = mid; else lo = mid + 1;
  }
  snprintf(buf, sizeof(buf), "%.*e", lo - 1, x);        // d.ddddde[+-]XX
  int n = 0;
  const char* p = buf;
  if (*p == '-') ++p;
  for (; *p && *p != 'e'; ++p)
    if (*p >= '0' && *p <= '9') digits[n++] = *p;
  const int e10 = atoi(p + 1);
  while (n > 1 && digits[n - 1] == '0') --n;
  digits[n] = 0;
  *decpt = e10 + 1;
  return n;
}

// Python: repr(float) -- what json.dumps writes for a float
void py_repr_double(double x, std::string& out) {
  if (isnan(x)) { out += "NaN"; return; }
  if (isinf(x)) { out += x < 0 ? "-Infinity" : "Infinity"; return; }
  if (x == 0.0) { out += signbit(x) ? "-0.0" : "0.0"; return; }
  if (x < 0) { out += '-'; x = -x; }
  char d[24];
  int decpt;
  const int n = shortest_digits<false>(x, d, &decpt);
  if (decpt <= -4 || decpt > 16) {             // exponent form: d[.ddd]e[+-]XX (at least two exponent digits)
    out += d[0];
    if (n > 1) { out += '.'; out.append(d + 1, n - 1); }
    char e[8];
    snprintf(e, sizeof(e), "e%c%02d", decpt - 1 < 0 ? '-' : '+', abs(decpt - 1));
    out += e;
  } else if (decpt <= 0) {
    out += "0.";
    out.append(-decpt, '0');
    out.append(d, n);
  } else if (decpt >= n) {
    out.append(d, n);
    out.append(decpt - n, '0');
    out += ".0";
  } else {
    out.append(d, decpt);
    out += '.';
    out.append(d + decpt, n - decpt);
  }
}

// numpy: str(np.float32(x)) (Dragon4, unique digits; positional for 1e-4 <= |x| < 1e16 with at least one fractional digit, else
// scientific with the mantissa's trailing zeros and point trimmed and at least two exponent digits)
void np_str_float32(float xf, std::string& out) {
  double x = xf;
  if (isnan(x)) { out += "nan"; return; }
  if (isinf(x)) { out += x < 0 ? "-inf" : "inf"; return; }
  if (x == 0.0) { out += signbit(x) ? "-0.0" : "0.0"; return; }
  if (x < 0) { out += '-'; x = -x; }
  char d[16];
  int decpt;
  const int n = shortest_digits<true>(x, d, &decpt);
  if (x >= 1e16 || x < 1e-4) {
    out += d[0];
    if (n > 1) { out += '.'; out.append(d + 1, n - 1); }
    char e[8];
    snprintf(e, sizeof(e), "e%c%02d", decpt - 1 < 0 ? '-' : '+', abs(decpt - 1));
    out += e;
  } else if (decpt <= 0) {
    out += "0.";
    out.append(-decpt, '0');
    out.append(d, n);
  } else if (decpt >= n) {
    out.append(d, n);
    out.append(decpt - n, '0');
    out += ".0";
  } else {
    out.append(d, decpt);
    out += '.';
    out.append(d + decpt, n - decpt);
  }
}

// one detection -> `"bbox": [x, y, w, h], "score": s` (without the braces: the refined file appends to it)
void item_text(const float* box_resized, float prob, float scale, int h, int w, std::string& out) {
  // eval.py:93-94: boxes / scale, clip (float32 array arithmetic); train.py:404-406: xywh; round(., 1), round(., 2) on float32 scalars
  volatile float x0 = box_resized[0] / scale, y0 = box_resized[1] / scale, x1 = box_resized[2] / scale, y1 = box_resized[3] / scale;
  float b[4];
  b[0] = x0 <= 0.f ? 0.f : x0;                 // proposal/driver.py clip_boxes: values <= 0 (a negative zero included) -> +0; NaN stays
  b[1] = y0 <= 0.f ? 0.f : y0;
  b[2] = x1 > (float)w ? (float)w : x1;
  b[3] = y1 > (float)h ? (float)h : y1;
  volatile float bw = b[2] - b[0], bh = b[3] - b[1];
  b[2] = bw;
  b[3] = bh;
  out += "\"bbox\": [";
  for (int k = 0; k < 4; ++k) {
    volatile float t = b[k] * 10.0f;           // (volatile: one rounding per operation, no contraction into an fma)
    volatile float r = rintf(t);
    volatile float q = r / 10.0f;
    if (k) out += ", ";
    py_repr_double((double)q, out);
  }
  out += "], \"score\": ";
  volatile float t = prob * 100.0f;
  volatile float r = rintf(t);
  volatile float q = r / 100.0f;
  py_repr_double((double)q, out);
}

int write_file(const char* path, const void* head, size_t head_n, const void* body, size_t body_n) {
  const int fd = open(path, O_WRONLY | O_CREAT | O_TRUNC, 0666);
  if (fd < 0) return errno == ENOENT ? 1 : premvos::fail(PREMVOS_EINVAL, "write_frame_files: open %s: %s", path, strerror(errno));
  struct iovec iov[2] = {{const_cast<void*>(head), head_n}, {const_cast<void*>(body), body_n}};
  int first = head_n ? 0 : 1;
  size_t left = head_n + body_n;
  while (left > 0) {
    const ssize_t n = writev(fd, iov + first, 2 - first);
    if (n < 0) {
      if (errno == EINTR) continue;
      const int e = errno;
      close(fd);
      return premvos::fail(PREMVOS_EINVAL, "write_frame_files: write %s: %s", path, strerror(e));
    }
    left -= (size_t)n;
    size_t adv = (size_t)n;
    for (int k = first; k < 2 && adv > 0; ++k) {
      const size_t take = adv < iov[k].iov_len ? adv : iov[k].iov_len;
      iov[k].iov_base = static_cast<char*>(iov[k].iov_base) + take;
      iov[k].iov_len -= take;
      adv -= take;
      if (iov[k].iov_len == 0 && k == first) first = k + 1;
    }
  }
  if (close(fd) != 0) return premvos::fail(PREMVOS_EINVAL, "write_frame_files: close %s: %s", path, strerror(errno));
  return 0;
}

}  // namespace

extern "C" int premvos_format_floats_host(const double* values, int64_t n, int32_t as_float32_str, char* out, int64_t cap) {
  std::string s;
  for (int64_t i = 0; i < n; ++i) {
    if (as_float32_str) np_str_float32((float)values[i], s); else py_repr_double(values[i], s);
    s += '\n';
  }
  if ((int64_t)s.size() > cap) return premvos::fail(PREMVOS_EINVAL, "format_floats: output needs %ld bytes", (long)s.size());
  memcpy(out, s.data(), s.size());
  return (int)s.size();
}

extern "C" int premvos_write_frame_files_host(const premvos_frame_files* f) {
  PV_REQUIRE(f != nullptr && f->h > 0 && f->w > 0, "write_frame_files: bad arguments");
  PV_REQUIRE(f->count[0] >= 0 && f->count[1] >= 0 && f->count[0] <= 4096 && f->count[1] <= 4096, "write_frame_files: bad detection counts");
  int missing_dir = 0;
  // ---- <frame>.flo
  if (f->flo_path != nullptr) {
    PV_REQUIRE(f->flow != nullptr && f->flow_row_stride >= 2 * (int64_t)f->w, "write_frame_files: flow");
    struct { float tag; int32_t w, h; } head = {202021.25f, f->w, f->h};
    int rc;
    if (f->flow_row_stride == 2 * (int64_t)f->w) {
      rc = write_file(f->flo_path, &head, 12, f->flow, (size_t)f->h * f->w * 8);
    } else {                                 // a window of a wider block: gather the rows first
      std::string rows;
      rows.resize((size_t)f->h * f->w * 8);
      for (int y = 0; y < f->h; ++y) memcpy(&rows[(size_t)y * f->w * 8], f->flow + (int64_t)y * f->flow_row_stride, (size_t)f->w * 8);
      rc = write_file(f->flo_path, &head, 12, rows.data(), rows.size());
    }
    if (rc < 0) return rc;
    missing_dir |= rc;
  }
  // ---- the detections' texts, once
  const int n_all = f->count[0] + f->count[1];
  std::string items[2], one;
  std::string refined = "[";
  for (int which = 0; which < 2; ++which) {
    PV_REQUIRE(f->count[which] == 0 || (f->boxes[which] != nullptr && f->probs[which] != nullptr), "write_frame_files: detections");
    for (int i = 0; i < f->count[which]; ++i) {
      one.clear();
      item_text(f->boxes[which] + 4 * i, f->probs[which][i], f->scale, f->h, f->w, one);
      if (i) items[which] += ", ";
      items[which] += '{';
      items[which] += one;
      items[which] += '}';
      if (f->json_path[3] != nullptr) {
        const int slot = (which ? f->count[0] : 0) + i;
        if (slot) refined += ", ";
        refined += '{';
        refined += one;
        // "segmentation": {"size": [h, w], "counts": "<COCO string>"}, "conf_score": "<str(float32)>"
        PV_REQUIRE(f->rle_pool != nullptr && f->rle_offsets != nullptr && f->conf != nullptr, "write_frame_files: refined file without masks / conf");
        char sz[64];
        snprintf(sz, sizeof(sz), ", \"segmentation\": {\"size\": [%d, %d], \"counts\": \"", f->h, f->w);
        refined += sz;
        const int32_t* e = f->rle_pool + f->rle_offsets[slot];
        const int64_t m = (int64_t)f->rle_offsets[slot + 1] - f->rle_offsets[slot];
        const long long hw = (long long)f->h * f->w;
        long long prev_edge = 0, c1 = 0, c2 = 0;
        for (int64_t k = 0; k <= m; ++k) {           // maskApi.c rleToString on the successive differences of [0, edges..., hw]
          const long long edge = k < m ? (long long)e[k] : hw;
          const long long cnt = edge - prev_edge;
          prev_edge = edge;
          long long x = k > 2 ? cnt - c2 : cnt;
          c2 = c1;
          c1 = cnt;
          bool more = true;
          while (more) {
            char c = (char)(x & 0x1f);
            x >>= 5;
            more = (c & 0x10) ? x != -1 : x != 0;
            if (more) c |= 0x20;
            c = (char)(c + 48);
            if (c == '\\') refined += '\\';          // the one character of the alphabet (48 .. 111) JSON escapes
            refined += c;
          }
        }
        refined += "\"}, \"conf_score\": \"";
        np_str_float32(f->conf[slot], refined);
        refined += "\"}";
      }
    }
  }
  refined += ']';
  for (int which = 0; which < 2; ++which)
    if (f->json_path[which] != nullptr) {
      const std::string text = "[" + items[which] + "]";
      const int rc = write_file(f->json_path[which], nullptr, 0, text.data(), text.size());
      if (rc < 0) return rc;
      missing_dir |= rc;
    }
  if (f->json_path[2] != nullptr) {
    std::string text = "[" + items[0];
    if (f->count[0] && f->count[1]) text += ", ";
    text += items[1];
    text += ']';
    const int rc = write_file(f->json_path[2], nullptr, 0, text.data(), text.size());
    if (rc < 0) return rc;
    missing_dir |= rc;
  }
  if (f->json_path[3] != nullptr) {
    (void)n_all;
    const int rc = write_file(f->json_path[3], nullptr, 0, refined.data(), refined.size());
    if (rc < 0) return rc;
    missing_dir |= rc;
  }
  return missing_dir;       // 1: a directory does not exist (nothing else failed): the caller creates it and calls again
}

// ---------------------------------------------------------------------------------------------------------------------------
// <frame>.jpg: the host half of the baseline JPEG encoder (the device half is csrc/jpeg_enc_ops.hip).  Quantised coefficients
// in the layout premvos_jpeg_entropy_decode_host produces -> a complete JFIF file with the bytes libjpeg writes for
// jpeg_set_quality(q, TRUE) and default settings (jcmarker.c write_file_header / write_frame_header / write_scan_header,
// jchuff.c encode_one_block): no optimised tables, no restart markers, one interleaved scan.  tests/test_cpu_jpeg_encode.py
// compares whole files with PIL's.
// ---------------------------------------------------------------------------------------------------------------------------
namespace {

const uint8_t kEncZigzag[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

// T.81 annex K.3: the typical Huffman tables, {code-length counts[16], symbols}
const uint8_t kDcBits[2][16] = {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0}, {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0}};
const uint8_t kDcVals[12] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11};
const uint8_t kAcBits[2][16] = {{0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d}, {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77}};
const uint8_t kAcVals[2][162] = {
    {0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81,
     0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18,
     0x19, 0x1a, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48,
     0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75,
     0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99,
     0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3,
     0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5,
     0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa},
    {0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08,
     0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25,
     0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47,
     0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74,
     0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97,
     0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba,
     0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4,
     0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa}};

struct EncHuff {
  uint16_t code[256];
  uint8_t size[256];       // 0: the symbol has no code
};

struct EncTables {
  EncHuff dc[2], ac[2];
  static void derive(EncHuff& h, const uint8_t* bits, const uint8_t* vals) {      // T.81 annex C: canonical codes by length
    memset(&h, 0, sizeof(h));
    int code = 0, k = 0;
    for (int len = 1; len <= 16; ++len) {
      for (int i = 0; i < bits[len - 1]; ++i, ++k, ++code) {
        h.code[vals[k]] = (uint16_t)code;
        h.size[vals[k]] = (uint8_t)len;
      }
      code <<= 1;
    }
  }
  EncTables() {
    for (int t = 0; t < 2; ++t) {
      derive(dc[t], kDcBits[t], kDcVals);
      derive(ac[t], kAcBits[t], kAcVals[t]);
    }
  }
};

// Bytes go out through put(): behind the end of the caller's buffer they are counted, never stored.
struct ByteSink {
  uint8_t* p;
  uint8_t* end;
  int64_t dropped = 0;
  uint64_t acc = 0;          // pending bits, right-aligned
  int n = 0;
  void put(int b) {
    if (p < end) *p++ = (uint8_t)b;
    else ++dropped;
  }
  void put16(int v) {
    put(v >> 8);
    put(v & 0xFF);
  }
  void bits(uint32_t v, int k) {                    // k <= 32, n <= 7 on entry
    acc = (acc << k) | (v & ((1ull << k) - 1));
    n += k;
    while (n >= 8) {
      const int b = (int)((acc >> (n - 8)) & 0xFF);
      put(b);
      if (b == 0xFF) put(0);                        // T.81 B.1.1.5 byte stuffing
      n -= 8;
    }
  }
  void flush() {                                    // pad the last byte with 1-bits
    if (n) bits(0x7F, 8 - n);
    acc = 0;
    n = 0;
  }
};

inline int bit_length(unsigned v) { return v ? 32 - __builtin_clz(v) : 0; }

// jchuff.c encode_one_block (T.81 F.1.2): false = a coefficient outside the baseline range
inline bool encode_block(ByteSink& o, const EncHuff& dc, const EncHuff& ac, const int16_t* blk, int& last_dc) {
  int diff = blk[0] - last_dc;
  last_dc = blk[0];
  int nb = bit_length((unsigned)(diff < 0 ? -diff : diff));
  if (nb > 11) return false;
  o.bits(dc.code[nb], dc.size[nb]);
  if (nb) o.bits((uint32_t)(diff < 0 ? diff - 1 : diff), nb);
  int run = 0;
  for (int k = 1; k < 64; ++k) {
    const int v = blk[kEncZigzag[k]];
    if (v == 0) {
      ++run;
      continue;
    }
    for (; run > 15; run -= 16) o.bits(ac.code[0xF0], ac.size[0xF0]);           // ZRL
    nb = bit_length((unsigned)(v < 0 ? -v : v));
    if (nb > 10) return false;
    const int sym = (run << 4) | nb;
    o.bits(ac.code[sym], ac.size[sym]);
    o.bits((uint32_t)(v < 0 ? v - 1 : v), nb);
    run = 0;
  }
  if (run) o.bits(ac.code[0], ac.size[0]);                                        // EOB
  return true;
}

void put_dht(ByteSink& o, int tc_th, const uint8_t* bits, const uint8_t* vals) {
  int n = 0;
  for (int i = 0; i < 16; ++i) n += bits[i];
  o.put16(0xFFC4);
  o.put16(2 + 1 + 16 + n);
  o.put(tc_th);
  for (int i = 0; i < 16; ++i) o.put(bits[i]);
  for (int i = 0; i < n; ++i) o.put(vals[i]);
}

}  // namespace

extern "C" int premvos_jpeg_entropy_encode_host(const int16_t* coef, const premvos_jpeg_info* info, uint8_t* out, int64_t capacity,
                                                int64_t* written) {
  PV_REQUIRE(coef && info && out && written && capacity >= 0, "jpeg encode: null argument");
  const premvos_jpeg_info& I = *info;
  PV_REQUIRE(I.ncomp == 3 && I.width > 0 && I.height > 0 && I.width <= 65535 && I.height <= 65535, "jpeg encode: bad info block");
  PV_REQUIRE((I.hs == 1 || I.hs == 2) && (I.vs == 1 || I.vs == 2) && !(I.hs == 1 && I.vs == 2), "jpeg encode: bad sampling factors");
  PV_REQUIRE(I.mcux == premvos::cdiv(I.width, 8 * I.hs) && I.mcuy == premvos::cdiv(I.height, 8 * I.vs),
             "jpeg encode: info block geometry is inconsistent");
  int64_t off = 0;
  for (int c = 0; c < 3; ++c) {
    PV_REQUIRE(I.blocks_w[c] == I.mcux * (c == 0 ? I.hs : 1) && I.blocks_h[c] == I.mcuy * (c == 0 ? I.vs : 1) && I.coef_offset[c] == off,
               "jpeg encode: info block geometry is inconsistent");
    off += (int64_t)I.blocks_w[c] * I.blocks_h[c] * 64;
    for (int k = 0; k < 64; ++k)
      PV_REQUIRE(I.quant[c][k] >= 1 && I.quant[c][k] <= 255, "jpeg encode: quantisation values must be 1 ... 255 (baseline)");
  }
  PV_REQUIRE(I.coef_count == off, "jpeg encode: info block geometry is inconsistent");
  PV_REQUIRE(memcmp(I.quant[1], I.quant[2], sizeof(I.quant[1])) == 0, "jpeg encode: the two chroma components share one table");
  static const EncTables T;
  ByteSink o{out, out + capacity};
  *written = 0;
  o.put16(0xFFD8);                                                              // SOI
  o.put16(0xFFE0);                                                              // JFIF APP0: version 1.01, no units, 1 x 1
  o.put16(16);
  for (const char* s = "JFIF"; ; ++s) {
    o.put(*s);
    if (!*s) break;
  }
  o.put16(0x0101);
  o.put(0);
  o.put16(1);
  o.put16(1);
  o.put16(0);
  for (int t = 0; t < 2; ++t) {                                                 // DQT, one segment per table, zig-zag order
    o.put16(0xFFDB);
    o.put16(67);
    o.put(t);
    for (int k = 0; k < 64; ++k) o.put(I.quant[t][kEncZigzag[k]]);
  }
  o.put16(0xFFC0);                                                              // SOF0
  o.put16(17);
  o.put(8);
  o.put16(I.height);
  o.put16(I.width);
  o.put(3);
  for (int c = 0; c < 3; ++c) {
    o.put(c + 1);
    o.put(c == 0 ? (I.hs << 4) | I.vs : 0x11);
    o.put(c == 0 ? 0 : 1);
  }
  for (int t = 0; t < 2; ++t) {                                                 // DHT: DC0, AC0, DC1, AC1
    put_dht(o, t, kDcBits[t], kDcVals);
    put_dht(o, 0x10 | t, kAcBits[t], kAcVals[t]);
  }
  o.put16(0xFFDA);                                                              // SOS
  o.put16(12);
  o.put(3);
  for (int c = 0; c < 3; ++c) {
    o.put(c + 1);
    o.put(c == 0 ? 0x00 : 0x11);
  }
  o.put(0);
  o.put(63);
  o.put(0);
  int last_dc[3] = {0, 0, 0};
  for (int my = 0; my < I.mcuy && !o.dropped; ++my)
    for (int mx = 0; mx < I.mcux; ++mx)
      for (int c = 0; c < 3; ++c) {
        const int ch = c == 0 ? I.hs : 1, cv = c == 0 ? I.vs : 1, t = c == 0 ? 0 : 1;
        for (int by = 0; by < cv; ++by)
          for (int bx = 0; bx < ch; ++bx) {
            const int16_t* blk = coef + I.coef_offset[c] + ((int64_t)(my * cv + by) * I.blocks_w[c] + mx * ch + bx) * 64;
            PV_REQUIRE(encode_block(o, T.dc[t], T.ac[t], blk, last_dc[c]),
                       "jpeg encode: a coefficient of MCU (%d, %d) is outside the baseline range", my, mx);
          }
      }
  o.flush();
  o.put16(0xFFD9);                                                              // EOI
  if (o.dropped) return premvos::fail(PREMVOS_ENOSPACE, "jpeg encode: the output buffer holds %lld bytes, the file needs more",
                                      (long long)capacity);
  *written = o.p - out;
  return PREMVOS_OK;
}
