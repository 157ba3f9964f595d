// Evaluation metrics (gfx950): top-1 / top-5 hit counts of a batch of logits, accumulated on the
// device (tf_cnn_benchmarks --eval: tf.nn.in_top_k over the validation split).
//
//   * eval_metrics: for each row, t = logits[row][label]; the row is a top-k hit iff t is finite
//     and fewer than k of the row's ncls classes are STRICTLY greater than t (ties that straddle
//     the boundary all count as inside; a NaN never counts as greater; a NaN / Inf target is a
//     miss). label < 0: a padding row of a partial last batch, skipped and not an example.
//     label >= ncls: an example and a miss, and the row is not read.
//     counters (int64 [3]) = {examples, top1_hits, top5_hits} are ADDED INTO, so one launch per
//     batch accumulates over a whole pass: no zeroing launch, no memset node (misc.hip, colsum),
//     no host read -- legal inside a captured graph, and a replay keeps counting. Integer sums are
//     exact in any order, so deterministic mode needs no variant.
//
// One wave per row, EVAL_ROWS rows per 256-thread block (B = 64 rows of 1001 logits are 16 full
// blocks, not 64 nearly empty ones). The wave loads t first, then streams the row once: dword
// loads up to the first 16-byte boundary, 16-byte loads over the body, dword loads over the tail
// (rows of ld = 1001 floats are not 16-byte aligned), never outside [row, row + ncls). Row counts
// meet in wave_sum (<= ncls < 2^24: exact in fp32), the block's rows in LDS, and thread 0 ends with
// at most three 64-bit integer atomics.
#include "common.h"
#include "kernels.h"

namespace hcb {

constexpr int EVAL_ROWS = 4;  // waves (= rows) per block

__global__ __launch_bounds__(64 * EVAL_ROWS) void eval_metrics_kernel(const float* __restrict__ logits, int ld,
                                                                      const int64_t* __restrict__ labels, int B,
                                                                      int ncls, unsigned long long* counters) {
  __shared__ int hit[EVAL_ROWS][3];
  const int lane = threadIdx.x & 63, wid = wave_id_uniform();
  const int row = blockIdx.x * EVAL_ROWS + wid;
  int ex = 0, h1 = 0, h5 = 0;
  if (row < B) {
    const int64_t lab = labels[row];
    ex = lab >= 0;
    if (lab >= 0 && lab < ncls) {
      const float* lr = logits + (size_t)row * ld;
      const float t = lr[lab];
      if ((__float_as_uint(t) & 0x7f800000u) != 0x7f800000u) {  // finite target
        int head = (int)(((16u - (unsigned)((uintptr_t)lr & 15u)) & 15u) >> 2);
        head = head < ncls ? head : ncls;
        const int n4 = (ncls - head) >> 2;
        int cnt = 0;
        if (lane < head) cnt += lr[lane] > t;
        const f32x4* p4 = reinterpret_cast<const f32x4*>(lr + head);
        for (int i = lane; i < n4; i += 64) {
          const f32x4 v = p4[i];
          cnt += (v[0] > t) + (v[1] > t) + (v[2] > t) + (v[3] > t);
        }
        const int c = head + 4 * n4 + lane;  // tail: fewer than 4 elements
        if (c < ncls) cnt += lr[c] > t;
        const int above = (int)wave_sum((float)cnt);
        h1 = above < 1;
        h5 = above < 5;
      }
    }
  }
  if (lane == 0) {
    hit[wid][0] = ex;
    hit[wid][1] = h1;
    hit[wid][2] = h5;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    int s[3] = {0, 0, 0};
#pragma unroll
    for (int w = 0; w < EVAL_ROWS; ++w) {
      s[0] += hit[w][0];
      s[1] += hit[w][1];
      s[2] += hit[w][2];
    }
#pragma unroll
    for (int k = 0; k < 3; ++k)
      if (s[k] != 0) atomicAdd(counters + k, (unsigned long long)s[k]);
  }
}

void launch_eval_metrics(const float* logits, int ld, const int64_t* labels, int B, int ncls, int64_t* counters,
                         hipStream_t st) {
  if (B <= 0) return;
  hipLaunchKernelGGL(eval_metrics_kernel, dim3((unsigned)((B + EVAL_ROWS - 1) / EVAL_ROWS)), dim3(64 * EVAL_ROWS), 0,
                     st, logits, ld, labels, B, ncls, reinterpret_cast<unsigned long long*>(counters));
}

}  // namespace hcb
