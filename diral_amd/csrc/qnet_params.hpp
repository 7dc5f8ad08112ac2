// qnet_params.hpp - what diral_qnet_forward (diral_agent.hip) hands to the launcher of qnet_forward_kernel (k_qnet.hip,
// qnet_kernel.hpp): the limits of the dense chain, the parameter struct and the launcher's declaration.
#pragma once
#include <hip/hip_runtime.h>

namespace diral {

constexpr int kQnetMaxHidden = 3;      // L: D -> h_1 .. h_L -> A
constexpr int kQnetMaxIn = 1024;       // D
constexpr int kQnetMaxWidth = 256;     // h_i and A: one activation row of the tile in LDS
constexpr int kQnetThreads = 256;      // four waves
constexpr int kQnetRows = 64;          // rows of x per workgroup: two 32-row MFMA tiles

struct QnetParams {
  const void* x;                       // [rows] rows of width[0] elements of x_dtype, x_stride elements apart
  long long x_stride;
  int x_dtype;                         // DIRAL_F32 / DIRAL_F16 / DIRAL_BF16
  const float* params;                 // the blob (include/diral_env.h)
  float* q;                            // [rows][width[L + 1]]
  int rows, L, norm;
  float eps;                           // (float)ln_eps
  int width[kQnetMaxHidden + 2];       // D, h_1 .. h_L, A
  int off[kQnetMaxHidden + 1];         // layer l's W in the blob; b, gamma and beta follow it
};

// one walk over the blob of a chain - per hidden layer W, b, gamma, beta; then W, b -: where each layer's W starts
// (QnetParams::off), and the number of floats in all
inline long long qnet_params_walk(const int* width, int L, int* off) {
  long long n = 0;
  for (int l = 0; l <= L; ++l) {
    off[l] = (int)n;
    n += (long long)width[l] * width[l + 1] + (l < L ? 3 : 1) * (long long)width[l + 1];
  }
  return n;
}

hipError_t launch_qnet(const QnetParams& p, hipStream_t s);

}  // namespace diral
