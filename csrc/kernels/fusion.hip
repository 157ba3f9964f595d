// Tensor fusion for the hvd API: one launch moves ANY number of scattered tensors into (pack) or
// out of (unpack) one flat fp32 fusion buffer.
//
//   pack:    flat[off_i + j] = float(src_i[j]) * scale
//   unpack:  dst_i[j]        = T_i(flat[off_i + j] * scale)
//
// The tensor set is a device table of FusionEntry rows (kernels.h; a plain int64 tensor [n][5]).
// Every tensor is cut into chunks of FUSION_CHUNK elements; chunk0 is the exclusive prefix of the
// per-entry chunk counts, so a block maps its chunk number to (entry, chunk of that entry) with a
// binary search over the rows (wave-uniform: the rows come in through the scalar cache). A launch
// over a sub-run of rows (one bucket) passes the pointer to its first row; the prefix of that row
// is the base. A zero-length entry owns no chunk and is never selected.
//
// Per entry, 4 elements per lane: 16-byte fp32 accesses on the flat side (every slot starts at a
// multiple of 4 floats of a 16-byte aligned buffer, chunks are multiples of 4) against 16-byte
// (fp32) or 8-byte (bf16 / fp16) accesses on the tensor side, when the tensor's pointer is aligned
// to that width; otherwise (a view at an odd storage offset) the entry is copied element-wise.
// The tail (n % 4) is element-wise, as in bucket_pack_kernel (misc.hip). Slot padding is never
// touched. All bounds come from the entry's own n: an inconsistent prefix could skip or repeat
// elements but never leaves [ptr, ptr + n) / [off, off + n) -- those are validated on the host
// when the layout is built (parallel/fusion.py).
//
// Arithmetic: one fp32 multiply per element; to bf16 with f2bf (round to nearest even), to fp16
// with the _Float16 cast. Both are always the WIRE types (tags), whatever the 16-bit activation
// type of the library build.
#include "common.h"
#include "kernels.h"

namespace hcb {

namespace {

typedef _Float16 h16x4 __attribute__((ext_vector_type(4)));
constexpr int FUSION_THREADS = 256;

template <int TAG>
struct FusionT;
template <>
struct FusionT<0> {
  typedef float T;
  __device__ static __forceinline__ float to_f(float v) { return v; }
  __device__ static __forceinline__ float from_f(float v) { return v; }
  __device__ static __forceinline__ f32x4 load4(const float* p) { return *reinterpret_cast<const f32x4*>(p); }
  __device__ static __forceinline__ void store4(float* p, const f32x4& v) { *reinterpret_cast<f32x4*>(p) = v; }
};
template <>
struct FusionT<1> {  // bf16
  typedef uint16_t T;
  __device__ static __forceinline__ float to_f(uint16_t v) { return bf2f(v); }
  __device__ static __forceinline__ uint16_t from_f(float v) { return f2bf(v); }
  __device__ static __forceinline__ f32x4 load4(const uint16_t* p) {
    const u32x2 u = *reinterpret_cast<const u32x2*>(p);
    return f32x4{__uint_as_float(u[0] << 16), __uint_as_float(u[0] & 0xffff0000u), __uint_as_float(u[1] << 16),
                 __uint_as_float(u[1] & 0xffff0000u)};
  }
  __device__ static __forceinline__ void store4(uint16_t* p, const f32x4& v) {
    *reinterpret_cast<u32x2*>(p) = u32x2{(uint32_t)f2bf(v[0]) | ((uint32_t)f2bf(v[1]) << 16),
                                         (uint32_t)f2bf(v[2]) | ((uint32_t)f2bf(v[3]) << 16)};
  }
};
template <>
struct FusionT<2> {  // IEEE fp16
  typedef _Float16 T;
  __device__ static __forceinline__ float to_f(_Float16 v) { return (float)v; }
  __device__ static __forceinline__ _Float16 from_f(float v) { return (_Float16)v; }
  __device__ static __forceinline__ f32x4 load4(const _Float16* p) {
    const h16x4 h = *reinterpret_cast<const h16x4*>(p);
    return f32x4{(float)h[0], (float)h[1], (float)h[2], (float)h[3]};
  }
  __device__ static __forceinline__ void store4(_Float16* p, const f32x4& v) {
    *reinterpret_cast<h16x4*>(p) = h16x4{(_Float16)v[0], (_Float16)v[1], (_Float16)v[2], (_Float16)v[3]};
  }
};

// one chunk: len elements of tensor t <-> flat f; vec = t is aligned to 4 of its elements
template <bool PACK, int TAG>
__device__ __forceinline__ void fusion_chunk(typename FusionT<TAG>::T* __restrict__ t, float* __restrict__ f, int len,
                                             bool vec, float scale) {
  typedef FusionT<TAG> F;
  const int tid = threadIdx.x;
  const int n4 = vec ? len >> 2 : 0;
  for (int i = tid; i < n4; i += FUSION_THREADS) {
    if constexpr (PACK)
      *reinterpret_cast<f32x4*>(f + 4 * i) = F::load4(t + 4 * i) * scale;
    else
      F::store4(t + 4 * i, *reinterpret_cast<const f32x4*>(f + 4 * i) * scale);
  }
  for (int i = 4 * n4 + tid; i < len; i += FUSION_THREADS) {
    if constexpr (PACK)
      f[i] = F::to_f(t[i]) * scale;
    else
      t[i] = F::from_f(f[i] * scale);
  }
}

// no-fma-mix-insts: without it the element-wise fp16 store compiles (float * scale -> _Float16) to
// one v_fma_mixlo_f16, whose results differ from the fp32 multiply followed by the conversion in
// a few elements per 10^5 (measured against the vector path and the PyTorch reference); the
// contract here is the fp32 product, rounded once more by the cast
template <bool PACK>
__attribute__((target("no-fma-mix-insts"))) __global__ __launch_bounds__(FUSION_THREADS) void fusion_kernel(const FusionEntry* __restrict__ ents, int n_ent,
                                                                float* __restrict__ flat, float scale) {
  const int64_t base = ents[0].chunk0;
  const int64_t total =
      ents[n_ent - 1].chunk0 + (ents[n_ent - 1].n + FUSION_CHUNK - 1) / FUSION_CHUNK - base;
  for (int64_t c = blockIdx.x; c < total; c += gridDim.x) {
    int lo = 0, hi = n_ent - 1;  // the last row whose prefix is <= c: the entry that owns chunk c
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (ents[mid].chunk0 - base <= c)
        lo = mid;
      else
        hi = mid - 1;
    }
    const FusionEntry e = ents[lo];
    const int64_t s = (c - (e.chunk0 - base)) * FUSION_CHUNK;
    if (s < 0 || s >= e.n) continue;  // only with an inconsistent prefix
    const int len = (int)(e.n - s < FUSION_CHUNK ? e.n - s : FUSION_CHUNK);
    float* f = flat + e.off + s;
    if (e.tag == 0) {
      fusion_chunk<PACK, 0>(reinterpret_cast<float*>(e.ptr) + s, f, len, (e.ptr & 15) == 0, scale);
    } else if (e.tag == 1) {
      fusion_chunk<PACK, 1>(reinterpret_cast<uint16_t*>(e.ptr) + s, f, len, (e.ptr & 7) == 0, scale);
    } else if (e.tag == 2) {
      fusion_chunk<PACK, 2>(reinterpret_cast<_Float16*>(e.ptr) + s, f, len, (e.ptr & 7) == 0, scale);
    }
  }
}

int fusion_grid(int64_t max_chunks) {
  const int64_t cap = 2048;  // 8 blocks per CU; the blocks stride over the chunks
  return (int)(max_chunks < 1 ? 1 : (max_chunks > cap ? cap : max_chunks));
}

}  // namespace

int fusion_chunk_elems() { return FUSION_CHUNK; }

void launch_fusion_pack(const FusionEntry* entries_dev, int n_entries, float* flat, int64_t max_chunks, float scale,
                        hipStream_t st) {
  if (n_entries <= 0) return;
  hipLaunchKernelGGL(fusion_kernel<true>, dim3(fusion_grid(max_chunks)), dim3(FUSION_THREADS), 0, st, entries_dev,
                     n_entries, flat, scale);
}
void launch_fusion_unpack(const FusionEntry* entries_dev, int n_entries, const float* flat, int64_t max_chunks,
                          float scale, hipStream_t st) {
  if (n_entries <= 0) return;
  hipLaunchKernelGGL(fusion_kernel<false>, dim3(fusion_grid(max_chunks)), dim3(FUSION_THREADS), 0, st, entries_dev,
                     n_entries, const_cast<float*>(flat), scale);
}

}  // namespace hcb
