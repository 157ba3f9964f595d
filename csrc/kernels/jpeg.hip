// GPU half of the JPEG decode (--gpu_jpeg_decode). The host's entropy decoder (csrc/data/jpeg.cpp)
// leaves, per image, quantised DCT coefficients of the block window its crop needs plus the
// quantisation tables; the two kernels here do everything after the Huffman stage. Both are pure
// 32-bit integer arithmetic and equal data/jpeg.py jpeg_decode_reference bitwise.
//
//   jpeg_idct      one launch over all blocks of all images and components. The segment table
//                  (int64 [nseg][8], one row per image component: group0, nblocks, coefficient byte
//                  offset, record byte offset, quantisation table, plane byte offset, 0, 0) carries
//                  the exclusive prefix of ceil(nblocks / 32): a workgroup of 256 threads takes 32
//                  blocks of ONE segment, found by binary search over that prefix (wave-uniform, as
//                  fusion_pack does). 8 lanes per block: lane k loads row k of the coefficients and of
//                  the table (16 bytes each), dequantises into LDS, runs the column pass on column k,
//                  then the row pass on row k, and stores 8 samples. Planes are block-major
//                  ([block][8][8] uint8), so a wave's stores are one contiguous 512-byte run.
//                  LDS: 72 dwords per block (64 + 8 of padding, so the four blocks of a 32-lane
//                  group fall on distinct banks in the column pass).
//   jpeg_crop_rgb  one thread per pixel of the packed crop: luma fetch, triangle chroma upsampling
//                  (replication at the image's true border only), YCbCr -> RGB, r x r box mean, 3 bytes
//                  out at the (offset, h, w, flip) descriptor row preprocess_images reads afterwards.
//                  The image table (int64 [B][24]): ncomp (0: the row is not a GPU image and nothing is
//                  written), r, hs, vs, H, W, y0, x0, then per component plane byte offset, bx0, by0,
//                  bw, bh.
// Nothing relies on zeroed memory, there are no atomics; every offset and window is range-checked
// on the host copy of the tables before the launch (bindings.cpp).
#include "common.h"
#include "kernels.h"

namespace hcb {

namespace {

constexpr int IDCT_THREADS = 256;
constexpr int IDCT_LDS_STRIDE = 72;
constexpr int JPEG_QT_OFFSET = 128;  // quantisation tables inside a record (csrc/data/jpeg.h)

// One pass of the slow-integer IDCT (Loeffler-Ligtenberg-Moschytz, 13-bit constants) over 8 values,
// descaled by `shift` with rounding. Unsigned arithmetic: the definition wraps at 32 bits.
__device__ __forceinline__ void idct_pass(int (&v)[8], int shift) {
  typedef uint32_t u;
  u z2 = (u)v[2], z3 = (u)v[6];
  u z1 = (z2 + z3) * 4433u;
  u t2 = z1 - z3 * 15137u;
  u t3 = z1 + z2 * 6270u;
  u t0 = ((u)v[0] + (u)v[4]) << 13;
  u t1 = ((u)v[0] - (u)v[4]) << 13;
  const u t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
  t0 = (u)v[7];
  t1 = (u)v[5];
  t2 = (u)v[3];
  t3 = (u)v[1];
  z1 = t0 + t3;
  z2 = t1 + t2;
  z3 = t0 + t2;
  u z4 = t1 + t3;
  const u z5 = (z3 + z4) * 9633u;
  t0 *= 2446u;
  t1 *= 16819u;
  t2 *= 25172u;
  t3 *= 12299u;
  z1 = 0u - z1 * 7373u;
  z2 = 0u - z2 * 20995u;
  z3 = z5 - z3 * 16069u;
  z4 = z5 - z4 * 3196u;
  t0 += z1 + z3;
  t1 += z2 + z4;
  t2 += z2 + z3;
  t3 += z1 + z4;
  const u rnd = 1u << (shift - 1);
  v[0] = (int)(t10 + t3 + rnd) >> shift;
  v[7] = (int)(t10 - t3 + rnd) >> shift;
  v[1] = (int)(t11 + t2 + rnd) >> shift;
  v[6] = (int)(t11 - t2 + rnd) >> shift;
  v[2] = (int)(t12 + t1 + rnd) >> shift;
  v[5] = (int)(t12 - t1 + rnd) >> shift;
  v[3] = (int)(t13 + t0 + rnd) >> shift;
  v[4] = (int)(t13 - t0 + rnd) >> shift;
}

__global__ __launch_bounds__(IDCT_THREADS) void jpeg_idct_kernel(const int64_t* __restrict__ segs, int nseg,
                                                                 const uint8_t* __restrict__ coef,
                                                                 uint8_t* __restrict__ planes) {
  __shared__ __attribute__((aligned(16))) int ws[(IDCT_THREADS / 8) * IDCT_LDS_STRIDE];
  const int64_t g = blockIdx.x;
  int lo = 0, hi = nseg - 1;  // the last row whose prefix is <= g: the segment that owns group g
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (segs[mid * 8] <= g)
      lo = mid;
    else
      hi = mid - 1;
  }
  const int64_t* s = segs + lo * 8;
  const int64_t blk = (g - s[0]) * (IDCT_THREADS / 8) + (threadIdx.x >> 3);
  const int k = threadIdx.x & 7;
  const bool live = blk >= 0 && blk < s[1];
  int* w = ws + (threadIdx.x >> 3) * IDCT_LDS_STRIDE;
  int v[8];
  if (live) {
    const u32x4 c = *reinterpret_cast<const u32x4*>(coef + s[2] + blk * 128 + k * 16);
    const u32x4 q = *reinterpret_cast<const u32x4*>(coef + s[3] + JPEG_QT_OFFSET + s[4] * 128 + k * 16);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      v[2 * j] = (int)(int16_t)(c[j] & 0xffffu) * (int)(q[j] & 0xffffu);
      v[2 * j + 1] = ((int)c[j] >> 16) * (int)(q[j] >> 16);
    }
    *reinterpret_cast<u32x4*>(w + k * 8) = u32x4{(unsigned)v[0], (unsigned)v[1], (unsigned)v[2], (unsigned)v[3]};
    *reinterpret_cast<u32x4*>(w + k * 8 + 4) = u32x4{(unsigned)v[4], (unsigned)v[5], (unsigned)v[6], (unsigned)v[7]};
  }
  __syncthreads();
  if (live) {  // columns: lane k owns column k, nobody else reads or writes it in this pass
#pragma unroll
    for (int r = 0; r < 8; ++r) v[r] = w[r * 8 + k];
    idct_pass(v, 11);
#pragma unroll
    for (int r = 0; r < 8; ++r) w[r * 8 + k] = v[r];
  }
  __syncthreads();
  if (live) {  // rows
    const u32x4 a = *reinterpret_cast<const u32x4*>(w + k * 8), b = *reinterpret_cast<const u32x4*>(w + k * 8 + 4);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      v[j] = (int)a[j];
      v[4 + j] = (int)b[j];
    }
    idct_pass(v, 18);
    unsigned o[2] = {0u, 0u};
#pragma unroll
    for (int j = 0; j < 8; ++j) o[j >> 2] |= (unsigned)min(max(v[j] + 128, 0), 255) << (8 * (j & 3));
    *reinterpret_cast<u32x2*>(planes + s[5] + blk * 64 + k * 8) = u32x2{o[0], o[1]};
  }
}

struct Plane {
  const uint8_t* p;
  int x0, y0, bw;  // window origin in the component's samples, blocks per row
  __device__ __forceinline__ int at(int y, int x) const {
    const int yy = y - y0, xx = x - x0;
    return p[(((int64_t)(yy >> 3) * bw + (xx >> 3)) << 6) + ((yy & 7) << 3) + (xx & 7)];
  }
};

__device__ __forceinline__ Plane plane_of(const int64_t* t, int c, const uint8_t* planes) {
  const int64_t* f = t + 8 + 5 * c;
  return Plane{planes + f[0], (int)f[1] * 8, (int)f[2] * 8, (int)f[3]};
}

// nearer (a) and farther (b) sample of a subsampled axis for the full-resolution coordinate p;
// n: that axis of the image, so the farther tap is replicated at the true border only
__device__ __forceinline__ void taps(int p, int f, int n, int& a, int& b) {
  if (f == 1) {
    a = b = p;
    return;
  }
  a = p >> 1;
  b = min(max((p & 1) ? a + 1 : a - 1, 0), ((n + 1) >> 1) - 1);
}

__device__ __forceinline__ int chroma(const Plane& P, int hs, int vs, int ya, int yb, int xa, int xb, int Y, int X) {
  if (hs == 1 && vs == 1) return P.at(ya, xa);
  if (vs == 1) return (3 * P.at(ya, xa) + P.at(ya, xb) + ((X & 1) ? 2 : 1)) >> 2;
  if (hs == 1) return (3 * P.at(ya, xa) + P.at(yb, xa) + ((Y & 1) ? 2 : 1)) >> 2;
  const int near = 3 * P.at(ya, xa) + P.at(yb, xa), far = 3 * P.at(ya, xb) + P.at(yb, xb);
  return (3 * near + far + ((X & 1) ? 7 : 8)) >> 4;
}

__global__ __launch_bounds__(256) void jpeg_crop_rgb_kernel(const int64_t* __restrict__ imgs,
                                                            const int64_t* __restrict__ desc,
                                                            const uint8_t* __restrict__ planes,
                                                            uint8_t* __restrict__ stage) {
  const int img = blockIdx.y;
  const int64_t* t = imgs + (int64_t)img * 24;
  const int ncomp = (int)t[0];
  if (ncomp == 0) return;
  const int oh = (int)desc[img * 4 + 1], ow = (int)desc[img * 4 + 2];
  const int pix = blockIdx.x * 256 + threadIdx.x;
  if (pix >= oh * ow) return;
  const int r = (int)t[1], hs = (int)t[2], vs = (int)t[3], H = (int)t[4], W = (int)t[5];
  const int i = pix / ow, j = pix - i * ow;
  const int ybase = (int)t[6] + i * r, xbase = (int)t[7] + j * r;
  const Plane P0 = plane_of(t, 0, planes);
  const Plane P1 = plane_of(t, ncomp == 3 ? 1 : 0, planes), P2 = plane_of(t, ncomp == 3 ? 2 : 0, planes);
  int sr = 0, sg = 0, sb = 0;
  for (int dy = 0; dy < r; ++dy) {
    const int Y = ybase + dy;
    int ya, yb;
    taps(Y, vs, H, ya, yb);
    for (int dx = 0; dx < r; ++dx) {
      const int X = xbase + dx;
      const int lum = P0.at(Y, X);
      if (ncomp == 1) {
        sr += lum;
        sg += lum;
        sb += lum;
      } else {
        int xa, xb;
        taps(X, hs, W, xa, xb);
        const int cb = chroma(P1, hs, vs, ya, yb, xa, xb, Y, X) - 128;
        const int cr = chroma(P2, hs, vs, ya, yb, xa, xb, Y, X) - 128;
        sr += min(max(lum + ((91881 * cr + 32768) >> 16), 0), 255);
        sg += min(max(lum + ((-22554 * cb - 46802 * cr + 32768) >> 16), 0), 255);
        sb += min(max(lum + ((116130 * cb + 32768) >> 16), 0), 255);
      }
    }
  }
  const int half = (r * r) >> 1, sh = r == 1 ? 0 : (r == 2 ? 2 : (r == 4 ? 4 : 6));
  uint8_t* o = stage + desc[img * 4] + (int64_t)pix * 3;
  o[0] = (uint8_t)((sr + half) >> sh);
  o[1] = (uint8_t)((sg + half) >> sh);
  o[2] = (uint8_t)((sb + half) >> sh);
}

}  // namespace

int jpeg_idct_group_blocks() { return IDCT_THREADS / 8; }

void launch_jpeg_idct(const int64_t* segs_dev, int nseg, int64_t groups, const uint8_t* coef, uint8_t* planes,
                      hipStream_t st) {
  if (nseg <= 0 || groups <= 0) return;
  hipLaunchKernelGGL(jpeg_idct_kernel, dim3((unsigned)groups), dim3(IDCT_THREADS), 0, st, segs_dev, nseg, coef, planes);
}

void launch_jpeg_crop_rgb(const int64_t* imgs_dev, const int64_t* desc_dev, int B, int64_t max_pixels,
                          const uint8_t* planes, uint8_t* stage, hipStream_t st) {
  if (B <= 0 || max_pixels <= 0) return;
  hipLaunchKernelGGL(jpeg_crop_rgb_kernel, dim3((unsigned)((max_pixels + 255) / 256), B), dim3(256), 0, st, imgs_dev,
                     desc_dev, planes, stage);
}

}  // namespace hcb
