// qnet_kernel.hpp - diral_qnet_forward: the reference's dense Q-network chain (DRQN._create_network,
// algorithms/drl_drqn.py:109-155) as ONE launch: [matmul + bias -> relu -> layer_norm] x L, then matmul + bias, for
// D -> h_1 .. h_L -> A with 0 <= L <= 3, D <= 1024, h_i <= 256, A <= 256.  With use_lstm_input false this is the whole
// Q-network (the DQN branch), with it true everything behind lstm_out[:, -1, :].  Float32 throughout: x (float32, float16
// or bfloat16) is converted exactly, the parameters and q are float32.  A row is worked in this order:
//   1. z[j] = (sum over k = 0, 1, .. in - 1, in that order, of x[k] * W[k][j]) + b[j]: the sum is the f32-input MFMA's
//      accumulation from zero - acc = fmaf(x[k], W[k][j], acc), one rounding per term -, the bias one float32 addition
//      after it.  W is [in][out] row-major, the reference's orientation;
//   2. r[j] = z[j] > 0 ? z[j] : 0 (a NaN stays a NaN);
//   3. mean = (sum of r) / h, var = (sum of (r - mean)^2) / h - two passes, biased, as tf.nn.moments -, over the h true
//      columns only.  Each sum is four partial sums, partial s over the columns s, s + 4, s + 8, .. in turn, added as
//      ((p0 + p1) + p2) + p3.  The mean is summed twice: m0 = (sum of r) / h, mean = m0 + (sum of (r - m0)) / h.  The second
//      sum takes the first one's rounding out: a row of h equal values c (every row behind a dead relu row: b everywhere)
//      has mean == c, var == 0 and y == beta exactly, where m0 alone is an ulp off and 1 / sqrt(0 + 1e-12) = 1e6 turns
//      that ulp into 0.06 in every column;
//   4. y[j] = (r[j] - mean) * (1.0f / sqrtf(var + (float)eps)) * gamma[j] + beta[j], left to right, never fused (the
//      build has -ffp-contract=off), the division and the square root correctly rounded;
//   5. the output layer is step 1 alone.
// norm == 0 leaves out steps 3 and 4.  eps is the caller's; the Python layer's default 1e-12 is the variance_epsilon of
// TF 1.14's tf.contrib.layers.layer_norm (its call of tf.nn.batch_normalization) AS FAR AS ITS SOURCE IS REMEMBERED:
// TensorFlow was not installed where this was written, so the value has not been read off a TensorFlow tree.
//
// Layout.  A workgroup of four waves owns 64 rows.  The activations of the tile live in LDS as float32 [64][257] - the
// odd pitch puts the 32 rows an A fragment reads, and the 64 rows the layer-norm passes walk, on distinct banks - and stay
// there from layer to layer: only x is read from HBM and only q is written.  A layer is C[64][out] = act[64][in] * W on
// __builtin_amdgcn_mfma_f32_32x32x2f32: lane l holds A[row l & 31][k = l >> 5] (one LDS read) and B[k = l >> 5][col l & 31]
// (one global load straight from the blob: a 256 x 256 layer is 256 KB and stays in L2); register i of the result is
// C[row (i & 3) + 8 (i >> 2) + 4 (l >> 5)][col l & 31].  With more than two 32-column tiles wave w owns the column tiles
// w and w + 4 for both 32-row tiles (each B load feeds two MFMAs, each A read two); with one or two, wave w owns column
// tile w >> 1 of row tile w & 1.  Columns past `out` and k past `in` are zeros (B is loaded under a guard, the pad columns
// of act are written as zeros), so the padding adds exact zeros at the end of a chain and nothing to the statistics.  A
// first layer wider than 256 streams x through the LDS tile in chunks of 256 columns, the accumulators carrying over, so
// the k order is unchanged.  A row's values depend on that row and the parameters only: row i of A meets row i of C and
// nothing else, and the statistics of a row are summed by column index.  Rows past `rows` are zeros in LDS, never read
// from x and never written to q.
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>

#include "qnet_params.hpp"
#include "select_kernel.hpp"   // bf16_bits

namespace diral {

constexpr int kQnetPitch = kQnetMaxWidth + 1;
constexpr int kQnetChunk = kQnetMaxWidth;      // columns of x in LDS at a time

using qnet_f32x16 = __attribute__((ext_vector_type(16))) float;

// element i of x as float32, exactly
__device__ __forceinline__ float qnet_x(const void* x, int dtype, long long i) {
  if (dtype == DIRAL_F32) return static_cast<const float*>(x)[i];
  if (dtype == DIRAL_F16) return (float)static_cast<const _Float16*>(x)[i];
  return __uint_as_float((uint32_t)static_cast<const bf16_bits*>(x)[i].b << 16);
}

__device__ __forceinline__ float qnet_sum4(const float (*part)[kQnetRows], int r) {
  return ((part[0][r] + part[1][r]) + part[2][r]) + part[3][r];
}

__global__ __launch_bounds__(kQnetThreads) void qnet_forward_kernel(const QnetParams p) {
  __shared__ float act[kQnetRows * kQnetPitch];
  __shared__ float part[2][4][kQnetRows];
  const int tid = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63, l31 = lane & 31, half = lane >> 5;
  const long long row0 = (long long)blockIdx.x * kQnetRows;
  const int live = (int)((long long)p.rows - row0 < kQnetRows ? (long long)p.rows - row0 : kQnetRows);

  for (int l = 0; l <= p.L; ++l) {
    const int in = p.width[l], out = p.width[l + 1];
    const float* __restrict__ W = p.params + p.off[l];
    const float* __restrict__ bias = W + (size_t)in * out;
    const int ntiles = (out + 31) >> 5;
    // the wave's 32 x 32 tiles of C: (ct[c], rt[r]) where on[c][r]
    int ct[2], rt[2];
    bool on[2][2];
    if (ntiles > 2) {
      ct[0] = wave; ct[1] = wave + 4; rt[0] = 0; rt[1] = 1;
      on[0][0] = on[0][1] = ct[0] < ntiles;
      on[1][0] = on[1][1] = ct[1] < ntiles;
    } else {
      ct[0] = ct[1] = wave >> 1; rt[0] = rt[1] = wave & 1;
      on[0][0] = ct[0] < ntiles;
      on[0][1] = on[1][0] = on[1][1] = false;
    }
    const int col0 = ct[0] * 32 + l31, col1 = ct[1] * 32 + l31;
    const bool c0 = col0 < out, c1 = col1 < out;
    qnet_f32x16 acc[2][2];
#pragma unroll
    for (int c = 0; c < 2; ++c)
#pragma unroll
      for (int r = 0; r < 2; ++r)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[c][r][i] = 0.0f;

    const int nchunk = l == 0 ? (in + kQnetChunk - 1) / kQnetChunk : 1;
    for (int ch = 0; ch < nchunk; ++ch) {
      const int k0 = ch * kQnetChunk;
      const int kw = in - k0 < kQnetChunk ? in - k0 : kQnetChunk, kp = (kw + 1) & ~1;
      if (l == 0) {
        if (ch) __syncthreads();                       // the previous chunk has been read
        for (int r = wave; r < kQnetRows; r += 4) {
          const long long base = (row0 + r) * p.x_stride + k0;
          for (int c = lane; c < kp; c += 64)
            act[r * kQnetPitch + c] = (r < live && c < kw) ? qnet_x(p.x, p.x_dtype, base + c) : 0.0f;
        }
        __syncthreads();
      }
      const float* a0p = act + (rt[0] * 32 + l31) * kQnetPitch + half;
      const float* a1p = act + (rt[1] * 32 + l31) * kQnetPitch + half;
      const float* w0p = W + (size_t)(k0 + half) * out + (c0 ? col0 : 0);
      const float* w1p = W + (size_t)(k0 + half) * out + (c1 ? col1 : 0);
      // the wave's B values of the k pair at k (this lane's k is k + half); a pad column reads column 0 - a valid address -
      // and is zeroed in mma: NC column tiles x NR row tiles, one k pair.
      auto load_b = [&](auto nc, int k, float& b0, float& b1) {
        b0 = w0p[(size_t)k * out];
        b1 = 0.0f;
        if constexpr (decltype(nc)::value == 2) b1 = w1p[(size_t)k * out];
      };
      auto mma = [&](auto nc, auto nr, int k, float b0, float b1) {
        b0 = c0 ? b0 : 0.0f;
        b1 = c1 ? b1 : 0.0f;
        const float a0 = a0p[k];
        acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc[0][0], 0, 0, 0);
        if constexpr (decltype(nr)::value == 2) {
          const float a1 = a1p[k];
          acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, acc[0][1], 0, 0, 0);
          if constexpr (decltype(nc)::value == 2) {
            acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc[1][1], 0, 0, 0);
          }
        }
      };
      auto chain = [&](auto nc, auto nr) {
        const int kf = kw & ~1, k8 = kw & ~7;
        float b0[4], b1[4], n0[4], n1[4];
        if (k8) {
#pragma unroll
          for (int j = 0; j < 4; ++j) load_b(nc, 2 * j, b0[j], b1[j]);
        }
        for (int k = 0; k < k8; k += 8) {              // the next four pairs' B values are in flight under these MFMAs
          const int kn = k + 8 < k8 ? k + 8 : k;       // (the last block loads itself again)
#pragma unroll
          for (int j = 0; j < 4; ++j) load_b(nc, kn + 2 * j, n0[j], n1[j]);
          __builtin_amdgcn_sched_barrier(0);           // (hipcc otherwise sinks the loads behind the MFMAs)
#pragma unroll
          for (int j = 0; j < 4; ++j) mma(nc, nr, k + 2 * j, b0[j], b1[j]);
#pragma unroll
          for (int j = 0; j < 4; ++j) { b0[j] = n0[j]; b1[j] = n1[j]; }
        }
        for (int k = k8; k < kf; k += 2) {
          load_b(nc, k, b0[0], b1[0]);
          mma(nc, nr, k, b0[0], b1[0]);
        }
        if (kw & 1) {                                  // the odd tail of `in`: a zero row of B at k = in
          b0[0] = b1[0] = 0.0f;
          if (half == 0) load_b(nc, kf, b0[0], b1[0]);
          mma(nc, nr, kf, b0[0], b1[0]);
        }
      };
      using one = std::integral_constant<int, 1>;
      using two = std::integral_constant<int, 2>;
      if (on[1][1]) chain(two{}, two{});
      else if (on[0][1]) chain(one{}, two{});
      else if (on[0][0]) chain(one{}, one{});
    }

    if (l == p.L) {                                    // the output layer: z to q, nothing else
#pragma unroll
      for (int c = 0; c < 2; ++c) {
        const int col = c ? col1 : col0;
        if (col >= out) continue;
        const float b = bias[col];
#pragma unroll
        for (int r = 0; r < 2; ++r) {
          if (!on[c][r]) continue;
#pragma unroll
          for (int i = 0; i < 16; ++i) {
            const int row = rt[r] * 32 + (i & 3) + 8 * (i >> 2) + 4 * half;
            if (row < live) p.q[(size_t)(row0 + row) * out + col] = acc[c][r][i] + b;
          }
        }
      }
      break;
    }

    __syncthreads();                                   // every wave has read the layer's input
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      const int col = c ? col1 : col0;
      const bool cin = col < out;
      const float b = cin ? bias[col] : 0.0f;
#pragma unroll
      for (int r = 0; r < 2; ++r) {
        if (!on[c][r]) continue;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          const int row = rt[r] * 32 + (i & 3) + 8 * (i >> 2) + 4 * half;
          const float z = acc[c][r][i] + b;
          act[row * kQnetPitch + col] = cin ? (z > 0.0f ? z : (z != z ? z : 0.0f)) : 0.0f;   // pad columns: zeros
        }
      }
    }
    __syncthreads();
    if (!p.norm) continue;

    // layer norm: thread (wave s, lane r) walks the columns s, s + 4, .. of row r
    const float* __restrict__ gamma = bias + out;
    const float* __restrict__ beta = gamma + out;
    float* arow = act + lane * kQnetPitch;
    const float h = (float)out;
    float s = 0.0f;
    for (int c = wave; c < out; c += 4) s += arow[c];
    part[0][wave][lane] = s;
    __syncthreads();
    const float m0 = qnet_sum4(part[0], lane) / h;
    float e = 0.0f;                                    // the sum again, of what the first one's rounding left
    for (int c = wave; c < out; c += 4) e += arow[c] - m0;
    part[1][wave][lane] = e;
    __syncthreads();
    const float mean = m0 + qnet_sum4(part[1], lane) / h;
    float v = 0.0f;
    for (int c = wave; c < out; c += 4) {
      const float d = arow[c] - mean;
      v += d * d;
    }
    part[0][wave][lane] = v;                           // (every thread has read part[0] in front of the barrier above)
    __syncthreads();
    const float rstd = 1.0f / sqrtf(qnet_sum4(part[0], lane) / h + p.eps);
    for (int c = wave; c < out; c += 4) arow[c] = (arow[c] - mean) * rstd * gamma[c] + beta[c];
    __syncthreads();
  }
}

}  // namespace diral
