// aux_kernels.hpp - the env's small kernels around the step (diral_env.hip): topology reset, action
// sampling, velocity update, state export/import, the xpos ring, pack / unpack, information-age histogram,
// metric read-out.  All are elementwise / tiny; none is on the hot path.  (The agent side's: agent_kernels.hpp.)
#pragma once
#include "common.hpp"
#include "policy_device.hpp"

namespace diral {

// Network.initialize_mobility_topology (network.py:92-119): x = randint(0, L)
// (integer valued), y = randint(0, H/2) = 0, v = 1.7 if mobility_vary else
// uniform(1.1, 2.7); any of x0/y0/v0 given => copied instead.
// Device draws are indexed by the GLOBAL vehicle index idx0 + i (idx0 = env offset of this
// handle x N, DIRAL_OPT_ENV_OFFSET): a batch sharded over several handles / GPUs draws
// exactly what one handle holding the whole batch draws.
// One vehicle: `g` its global index (the draws), `i` its place in this handle's [B][N] arrays (the given values).
// reset_kernel and reset_envs_kernel (reset_envs_kernel.hpp) both state a fresh vehicle through here.
template <typename Index>
__device__ __forceinline__ void reset_draw(double L, int vary, uint64_t seed, uint64_t g, Index i, const double* x0,
                                           const double* y0, const double* v0, double& x, double& y, double& v) {
  if (x0) x = x0[i];
  else {
    const double Lf = floor(L);
    x = floor(rng_unit(rng_u64(seed, 1, g)) * Lf);
    if (x >= Lf) x = Lf - 1.0;
  }
  y = y0 ? y0[i] : 0.0;
  if (v0) v = v0[i];
  else v = vary ? 1.7 : 1.1 + rng_unit(rng_u64(seed, 2, g)) * (2.7 - 1.1);
}

__global__ void reset_kernel(int total, double L, int vary, uint64_t seed, uint64_t idx0, const double* x0,
                             const double* y0, const double* v0, double* pos_x, double* pos_y,
                             double* vel) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  double x, y, v;
  reset_draw(L, vary, seed, idx0 + (uint64_t)i, i, x0, y0, v0, x, y, v);
  pos_x[i] = x; pos_y[i] = y; vel[i] = v;
}

// TestEnv.sample (test_env.py:116-122)
__global__ void sample_kernel(int total, int A, uint64_t seed, uint64_t idx0, int32_t* out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  out[i] = (int32_t)(rng_u64(seed, 3, idx0 + (uint64_t)i) % (uint64_t)A);
}

// Network.update_velocity (network.py:208-223)
__global__ void velocity_kernel(int total, const uint8_t* draws, uint64_t seed, uint64_t idx0, double* vel) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  vel[i] = draws ? velocity_step(vel[i], (int)draws[i]) : velocity_draw(vel[i], seed, idx0 + (uint64_t)i);
}

// subject-major packed table -> reference-shaped [env][viewer][subject] planes
__global__ void export_tables_kernel(int B, int N, int NV, int NR, const uint32_t* tkey, const double* tx,
                                     const double* pos_y, int32_t* seq, int32_t* age, double* x,
                                     double* y) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t total = (size_t)B * N * N;
  if (i >= total) return;
  const int k = (int)(i % N);
  const int u = (int)((i / N) % N);
  const int b = (int)(i / ((size_t)N * N));
  const size_t src = ((size_t)b * NR + k) * NV + u;
  const uint32_t w = tkey[src];
  if (seq) seq[i] = (int32_t)(w >> 8);
  if (age) age[i] = (int32_t)(w & 255u);
  if (x) x[i] = tx[src];
  if (y) y[i] = (w >> 8) ? pos_y[(size_t)b * N + k] : 0.0;
}

// The xpos ring of the N <= 64 kernel (step_fast64.hpp): ring[env][subject][seq & 7]
// is the subject's stamp at sequence number `seq`, for its 8 most recent numbers.  An entry that
// lags its subject by at most 7 finds its xpos there; only older entries need the per-entry plane.
// rebuild: plane -> ring (after an import or a step of another kernel family); materialise: ring ->
// plane (before anything else reads the plane).  Entries of one subject with equal sequence numbers
// hold equal xpos in every reachable state, so concurrent writers of a slot agree.
__global__ void ring_rebuild_kernel(int B, int N, int NV, int NR, const uint32_t* tkey, const double* tx, double* ring) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (size_t)B * N * N) return;
  const int u = (int)(i % N);
  const int k = (int)((i / N) % N);
  const int b = (int)(i / ((size_t)N * N));
  const size_t row = (size_t)b * NR + k;
  const uint32_t seq = tkey[row * NV + u] >> 8, tk = tkey[row * NV + k] >> 8;
  if (tk - seq <= 7u) ring[row * 8 + (seq & 7u)] = tx[row * NV + u];
}
// After an import: every entry the ring answers for must find ITS xpos there.  Tables no run of the reference
// produces (two entries about one subject with the same sequence number and different xpos) make the writers of
// ring_rebuild_kernel race; the loser is found here and reported through the sticky error word
// (diral_env_check: DIRAL_ERR_TABLE_CONFLICT).  Bitwise comparison: -0.0 / NaN payloads count as written.
__global__ void ring_verify_kernel(int B, int N, int NV, int NR, const uint32_t* tkey, const double* tx, const double* ring,
                                   uint32_t* err) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (size_t)B * N * N) return;
  const int u = (int)(i % N);
  const int k = (int)((i / N) % N);
  const int b = (int)(i / ((size_t)N * N));
  const size_t row = (size_t)b * NR + k;
  const uint32_t seq = tkey[row * NV + u] >> 8, tk = tkey[row * NV + k] >> 8;
  if (tk - seq <= 7u &&
      __double_as_longlong(ring[row * 8 + (seq & 7u)]) != __double_as_longlong(tx[row * NV + u]))
    atomicOr(err, kErrTable);
}
__global__ void ring_materialize_kernel(int B, int N, int NV, int NR, const uint32_t* tkey, const double* ring, double* tx) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (size_t)B * N * N) return;
  const int u = (int)(i % N);
  const int k = (int)((i / N) % N);
  const int b = (int)(i / ((size_t)N * N));
  const size_t row = (size_t)b * NR + k;
  const uint32_t seq = tkey[row * NV + u] >> 8, tk = tkey[row * NV + k] >> 8;
  if (tk - seq <= 7u) tx[row * NV + u] = ring[row * 8 + (seq & 7u)];
}

// The PACKED table of step_fast64 (step_fast64.hpp: codes, ages, own sequence numbers, old-quad flags) from the
// planes and back.  One thread per (env, row-quad, viewer): four table entries.
//   pack: after an import or a step of another kernel family (`told` zeroed by the caller beforehand).  An entry
//   is coded if it was heard (seq != 0) and lags its subject by at most 7; one that lags 7 or more flags its
//   quad - from the next slot on it is beyond the codes, and the planes hold it (they are complete right now).
//   unpack: before anything reads the planes.  A coded entry's sequence number is the subject's own minus its lag,
//   its xpos the subject's stamp of that number in the ring; a code-0 entry keeps the plane's sequence number
//   (0: never heard) and xpos; every entry's age comes from the age words.
__global__ void pack_codes_kernel(int B, int N, int NV, int NR, const uint32_t* tkey, uint32_t* tcode, uint32_t* tage,
                                  uint32_t* tseq, uint32_t* told) {
  const int NQ = NR >> 2;
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (size_t)B * NQ * NV) return;
  const int u = (int)(i % NV);
  const int q = (int)((i / NV) % NQ);
  const int b = (int)(i / ((size_t)NV * NQ));
  uint32_t code = 0u, age = 0u;
  bool flag = false;
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const int k = 4 * q + c;
    const size_t row = (size_t)b * NR + k;
    const bool ex = k < N && u < N;
    const uint32_t w = ex ? tkey[row * NV + u] : 0u;
    const uint32_t tk = k < N ? tkey[row * NV + k] >> 8 : 0u;
    const uint32_t seq = w >> 8, lag = tk - seq;
    const bool coded = seq != 0u && lag <= 7u;
    code |= (coded ? ((0xffu << lag) & 0xffu) : 0u) << (8 * c);
    age |= (w & 255u) << (8 * c);
    flag = flag || (seq != 0u && lag >= 7u);
    if (u == k || (k >= N && u == 0)) tseq[row] = tk;
  }
  tcode[i] = code;
  tage[i] = age;
  if (flag) atomicOr(&told[(size_t)b * NQ + q], 1u);
}
__global__ void unpack_codes_kernel(int B, int N, int NV, int NR, const uint32_t* tcode, const uint32_t* tage,
                                    const uint32_t* tseq, const double* ring, uint32_t* tkey, double* tx) {
  const int NQ = NR >> 2;
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (size_t)B * NQ * NV) return;
  const int u = (int)(i % NV);
  const int q = (int)((i / NV) % NQ);
  const int b = (int)(i / ((size_t)NV * NQ));
  if (u >= N) return;
  const uint32_t code = tcode[i], age = tage[i];
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const int k = 4 * q + c;
    if (k >= N) break;
    const size_t row = (size_t)b * NR + k;
    const uint32_t r = (code >> (8 * c)) & 255u, a = (age >> (8 * c)) & 255u;
    if (r) {
      const uint32_t seq = tseq[row] - 8u + (uint32_t)__popc(r);
      tkey[row * NV + u] = (seq << 8) | a;
      tx[row * NV + u] = ring[row * 8 + (seq & 7u)];
    } else {
      tkey[row * NV + u] = (tkey[row * NV + u] & ~255u) | a;
    }
  }
}

// A sequence number the 24-bit field of the table word cannot hold, or the one past the last a step accepts
// (outside [0, kSeqMax]), is not truncated into a legal-looking one: it raises kErrSeq in the sticky error
// word (diral_env_check: DIRAL_ERR_SEQ_OVERFLOW) and the entry is stored as never heard.
constexpr uint32_t kSeqMax = (1u << 24) - 2u;   // DIRAL_MAX_SLOTS
__global__ void import_tables_kernel(int B, int N, int NV, int NR, const int32_t* seq, const int32_t* age,
                                     const double* x, uint32_t* tkey, double* tx, uint32_t* err) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t total = (size_t)B * N * N;
  if (i >= total) return;
  const int k = (int)(i % N);
  const int u = (int)((i / N) % N);
  const int b = (int)(i / ((size_t)N * N));
  const size_t dst = ((size_t)b * NR + k) * NV + u;
  if (seq || age) {
    uint32_t w = tkey[dst];
    uint32_t s = seq ? (uint32_t)seq[i] : (w >> 8);
    if (s > kSeqMax) { atomicOr(err, kErrSeq); s = 0u; }      // (a negative number lands here too)
    int a = age ? age[i] : (int)(w & 255u);
    if (a > 255) a = 255;
    if (a < 0) a = 0;
    tkey[dst] = (s << 8) | (uint32_t)a;
  }
  if (x) tx[dst] = x[i];
}

// The tables as RealNeS MA_NeighborTableEntry records (diral_env.h: DiralNeighborEntry), one 16-byte
// record per thread: a coalesced dwordx4 on the record side, a stride-NV gather on the plane side.
__global__ void export_entries_kernel(int B, int N, int NV, int NR, const uint32_t* tkey, const double* tx,
                                      const double* pos_y, DiralNeighborEntry* out) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (size_t)B * N * N) return;
  const int k = (int)(i % N);
  const int u = (int)((i / N) % N);
  const int b = (int)(i / ((size_t)N * N));
  const size_t src = ((size_t)b * NR + k) * NV + u;
  const uint32_t w = tkey[src];
  DiralNeighborEntry r;
  r.pos_x = (float)tx[src];
  r.pos_y = (w >> 8) ? (float)pos_y[(size_t)b * N + k] : 0.0f;
  r.seq_num = (int32_t)(w >> 8);
  r.last_update = (int32_t)(w & 255u);
  out[i] = r;
}

__global__ void import_entries_kernel(int B, int N, int NV, int NR, const DiralNeighborEntry* in, uint32_t* tkey,
                                      double* tx, uint32_t* err) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (size_t)B * N * N) return;
  const int k = (int)(i % N);
  const int u = (int)((i / N) % N);
  const int b = (int)(i / ((size_t)N * N));
  const size_t dst = ((size_t)b * NR + k) * NV + u;
  const DiralNeighborEntry r = in[i];
  const int a = r.last_update > 255 ? 255 : (r.last_update < 0 ? 0 : r.last_update);
  uint32_t s = (uint32_t)r.seq_num;
  if (s > kSeqMax) { atomicOr(err, kErrSeq); s = 0u; }        // as in import_tables_kernel
  tkey[dst] = (s << 8) | (uint32_t)a;
  tx[dst] = (double)r.pos_x;
}

// Network.get_information_age (network.py:560-574); one workgroup per env.
// Python's negative list indexing (ia in [-100,-1]) is reproduced.
__global__ void info_age_kernel(int N, long long t, const int32_t* la, int32_t* out) {
  __shared__ int bins[100];
  const int b = blockIdx.x;
  for (int j = threadIdx.x; j < 100; j += blockDim.x) bins[j] = 0;
  __syncthreads();
  const int32_t* l = la + (size_t)b * N * N;
  for (int i = threadIdx.x; i < N * N; i += blockDim.x) {
    const int tx = i / N, rx = i - tx * N;
    if (tx == rx) continue;
    const int32_t v = l[i];
    if (v != -1) {
      long long ia = t - (long long)v;
      if (ia < 100) { if (ia < 0) ia += 100; if (ia >= 0) atomicAdd(&bins[(int)ia], 1); }
    }
  }
  __syncthreads();
  for (int j = threadIdx.x; j < 100; j += blockDim.x) out[(size_t)b * 100 + j] = bins[j];
}

__global__ void any_nonzero_kernel(int total, const double* v, uint32_t* flag) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < total && v[i] != 0.0) atomicOr(flag, 1u);
}

__global__ void metrics_kernel(int total, double* metrics, double* out, int clear) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  if (out) out[i] = metrics[i];
  if (clear) metrics[i] = 0.0;
}

}  // namespace diral
