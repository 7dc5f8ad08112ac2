// step_wide.hpp - the fused env-step kernel specialised for 64 < N <= 256
// vehicles (BASELINE.json configs[2] and [4]: 256-UE/64-res congested,
// 128-UE/64-res dynamic density), the toy YAML's State flags (one-hot action +
// type-2 piggybacked positional histogram), my_step + obtain_state, all y == 0.
//
// Same semantics as step_kernel.hpp (the general path; tests compare the two
// and the oracle bit for bit).  What the profile of the general kernel showed at
// N = 256 (profiles/r01/general_c3_before_wide_summary.txt): one 1024-thread workgroup per CU (115 KB LDS,
// 128 VGPRs + 40 spilled), the gossip merge moving 16-bit (rank, source) keys
// through LDS (4.3 KB per resource step per wave), and a finalize phase of
// ~160 VALU instructions per table entry full of exec-mask control flow.  Here:
//   * 8-bit merge keys.  For a fixed subject k an entry is determined by its
//     sequence number, so the merge only has to carry rank = 255 - lag
//     (lag = t_k - seq against the subject's own fresh sequence number): FOUR
//     columns per 32-bit LDS word, byte-wise max with SDWA.  Exact while every
//     entry of the pass has lag < 255 or seq == 0; otherwise the pass takes a
//     32-bit (seq, source) path, column by column.
//   * no source tracking: after the merge an updated entry needs the xpos that
//     belongs to its final sequence number.  Entries with equal (k, seq) hold
//     equal xpos, so every viewer drops its old xpos into a
//     256-entry LDS table indexed by its OLD rank and updated entries pick
//     theirs up by their NEW rank - one LDS write + one LDS read per entry.
//   * the per-entry state kept across the merge is 16 bits (old rank, age);
//     8 waves per workgroup (16 columns each at N <= 128, 32 at N <= 256), at most
//     84 VGPRs, three workgroups per CU (52 KB LDS each at N = 256).
//   * branch-free finalize (signed distance x1 - x2 is the histogram value when
//     all y are 0; bin = estimate + edge correction).
//   * xpos ring (see step_fast64.hpp / aux_kernels.hpp): an entry's xpos is a function of (subject, sequence number), the
//     ring keeps every subject's 8 latest stamps, so the finalize phase fills the rank -> xpos table of a column from the
//     subject's ring row (8 lanes) instead of having all viewers scatter their old xpos into it, and EVERY entry that lags
//     at most 7 reads its xpos there.  The per-entry xpos plane - two thirds of the table bytes - is only read for older
//     entries and only written when an entry reaches lag 7 (or copies an older one).
// (No kernel in this header: the body, step_wide_body.inc, is compiled by k_wide2.hip, k_wide4.hip and k_wide_slots.hip.)
#pragma once
#include <type_traits>

#include "common.hpp"
#include "policy_device.hpp"
#include "ref_math.hpp"
#include "rich_out.hpp"
#include "step_params.hpp"
#include "wave_ops.hpp"

namespace diral {

struct WideLds {
  uint32_t px, npx, rv, edges, red, mask, act, cnt, hist, mtab, scratch, pbytes, lut, slow, total;
};
#ifndef DIRAL_WIDE_WAVES4
#define DIRAL_WIDE_WAVES4 8              // waves per workgroup at N <= 256 (each owns 256 / waves subject columns)
#endif
// waves per workgroup: 8 x 16 columns (N <= 128), 8 x 32 columns (N <= 256)
__host__ __device__ constexpr int wide_waves(int vpl) { return vpl == 2 ? 8 : DIRAL_WIDE_WAVES4; }
#ifndef DIRAL_WIDE_PC2
#define DIRAL_WIDE_PC2 8                 // subject columns per merge pass, N <= 128
#endif
#ifndef DIRAL_WIDE_PC4
#define DIRAL_WIDE_PC4 8                 // subject columns per merge pass, N <= 256 (4 until the xpos ring freed the registers: C3 -3.5 %)
#endif
// merge scratch per wave: a pass's rank words (one byte per column and viewer), then the
// rank -> xpos table (256 doubles)
// (N <= 256: + 64 bytes in front of the lag -> xpos table of the packed form's finalize phase, whose lookup of a
// never-heard entry - lag "-1" - lands 8 bytes below its column's row: csrc/step_wide_closure.inc)
__host__ __device__ constexpr uint32_t wide_scratch(int vpl) {
  const uint32_t words = 64u * vpl * (vpl == 2 ? DIRAL_WIDE_PC2 : DIRAL_WIDE_PC4);
  return (words > 2048u ? words : 2048u) + (vpl == 4 ? 64u : 0u);
}
// histogram row stride in 32-bit words: two 16-bit bins per word (counts <= 255), odd stride
__host__ __device__ constexpr int wide_hist_stride(int K) { return ((K + 1) / 2) | 1; }
// row stride of the gather-source table in elements (u32 of 4 source bytes at N <= 256, u16 of
// 2 at N <= 128): 64 lanes + one 32-bit word of padding, so that the RICH output phase
// (lane -> (viewer, resource quad)) spreads over the banks; the merge (lane-contiguous) is
// conflict-free at any stride
__host__ __device__ constexpr int wide_mtab_stride(int vpl) { return vpl == 4 ? 65 : 66; }

__host__ __device__ inline WideLds wide_lds_layout(int vpl, int A, int K, bool packed = false) {
  const uint32_t npad = 64u * vpl;
  WideLds l;
  // The per-wave merge scratch sits at LDS offset 0: wave W's words start at the COMPILE-TIME
  // address 2048 W, which the merge loop (one copy per wave index) folds into the immediate
  // offset of its gathers instead of adding a base register to every gather address.
  l.scratch = 0;
  uint32_t o = wide_scratch(vpl) * wide_waves(vpl);        // 2 KB per wave (4 KB at 16 columns per pass)
  // the packed form's merge (step_wide_closure.inc), at compile-time addresses as well (DS immediate offsets): the
  // reachability matrix P of the slot as bytes [viewer][lane group][K step] (8 KB at N = 256, 2 KB at N = 128) and the
  // 256-entry bits -> 8 x bf16 table of the product's B operand
  // (one 16-byte read per K step; a 16-entry form of 4 x bf16 - 128 bytes, conflict-free - was bit-exact and slower: C3 1.33 -> 1.36 ms)
  l.pbytes = l.lut = o;
  // (+ the closure's own rows of P - npad / 16 bytes x 2 waves per viewer - and one row-ready flag per resource: it runs beside P1)
  if (packed) { l.pbytes = o; o += 8u * vpl * npad; l.lut = o; o += 4096u; o += 8u * vpl * npad; o += 4u * (uint32_t)kWideMaxA; }
  l.px = o;    o += 8u * npad;
  l.npx = o;   o += 8u * npad;
  l.rv = o;    o += 8u * A;
  l.edges = o; o += 8u * (K + 2);
  l.red = o;   o += 8u * 4 * vpl;
  l.slow = o;  o += 8u;                                  // the env holds a pass beyond the codes: a place among the first blocks of the next launch
  l.mask = o;  o += 8u * A * vpl;
  l.act = o;   o += 4u * npad;
  l.cnt = o;   o += 4u * npad;
  l.hist = o;  o += 4u * wide_hist_stride(K) * npad;   // [viewer][stride]: two bins per word
  l.mtab = o;  o += (uint32_t)A * wide_mtab_stride(vpl) * vpl;   // [resource][lane][slot]: gather source viewer (bytes)
  l.total = align_up(o, 16);
  return l;
}

// byte-wise unsigned max of four packed words (16 ranks) with SDWA.  The four
// words are interleaved so that no instruction consumes the partial result of
// the one right before it; the trailing s_nop covers the first consumer the
// compiler places after the block (it cannot see inside).
__device__ inline void max_u8x16(unsigned int (&a)[4], const unsigned int (&b)[4]) {
#define DIRAL_SDWA_MAX(B)                                                                                          \
  "v_max_u32_sdwa %0, %0, %4 dst_sel:BYTE_" #B " dst_unused:UNUSED_PRESERVE src0_sel:BYTE_" #B " src1_sel:BYTE_" #B "\n\t" \
  "v_max_u32_sdwa %1, %1, %5 dst_sel:BYTE_" #B " dst_unused:UNUSED_PRESERVE src0_sel:BYTE_" #B " src1_sel:BYTE_" #B "\n\t" \
  "v_max_u32_sdwa %2, %2, %6 dst_sel:BYTE_" #B " dst_unused:UNUSED_PRESERVE src0_sel:BYTE_" #B " src1_sel:BYTE_" #B "\n\t" \
  "v_max_u32_sdwa %3, %3, %7 dst_sel:BYTE_" #B " dst_unused:UNUSED_PRESERVE src0_sel:BYTE_" #B " src1_sel:BYTE_" #B "\n\t"
  asm(DIRAL_SDWA_MAX(0) DIRAL_SDWA_MAX(1) DIRAL_SDWA_MAX(2) DIRAL_SDWA_MAX(3) "s_nop 0"
      : "+v"(a[0]), "+v"(a[1]), "+v"(a[2]), "+v"(a[3])
      : "v"(b[0]), "v"(b[1]), "v"(b[2]), "v"(b[3]));
#undef DIRAL_SDWA_MAX
}

// ... and of eight packed words (32 ranks)
__device__ inline void max_u8x32(unsigned int (&a)[8], const unsigned int (&b)[8]) {
#define DIRAL_SDWA_MAX8(B)                                                                                          \
  "v_max_u32_sdwa %0, %0, %8 dst_sel:BYTE_" #B " dst_unused:UNUSED_PRESERVE src0_sel:BYTE_" #B " src1_sel:BYTE_" #B "\n\t" \
  "v_max_u32_sdwa %1, %1, %9 dst_sel:BYTE_" #B " dst_unused:UNUSED_PRESERVE src0_sel:BYTE_" #B " src1_sel:BYTE_" #B "\n\t" \
  "v_max_u32_sdwa %2, %2, %10 dst_sel:BYTE_" #B " dst_unused:UNUSED_PRESERVE src0_sel:BYTE_" #B " src1_sel:BYTE_" #B "\n\t" \
  "v_max_u32_sdwa %3, %3, %11 dst_sel:BYTE_" #B " dst_unused:UNUSED_PRESERVE src0_sel:BYTE_" #B " src1_sel:BYTE_" #B "\n\t" \
  "v_max_u32_sdwa %4, %4, %12 dst_sel:BYTE_" #B " dst_unused:UNUSED_PRESERVE src0_sel:BYTE_" #B " src1_sel:BYTE_" #B "\n\t" \
  "v_max_u32_sdwa %5, %5, %13 dst_sel:BYTE_" #B " dst_unused:UNUSED_PRESERVE src0_sel:BYTE_" #B " src1_sel:BYTE_" #B "\n\t" \
  "v_max_u32_sdwa %6, %6, %14 dst_sel:BYTE_" #B " dst_unused:UNUSED_PRESERVE src0_sel:BYTE_" #B " src1_sel:BYTE_" #B "\n\t" \
  "v_max_u32_sdwa %7, %7, %15 dst_sel:BYTE_" #B " dst_unused:UNUSED_PRESERVE src0_sel:BYTE_" #B " src1_sel:BYTE_" #B "\n\t"
  asm(DIRAL_SDWA_MAX8(0) DIRAL_SDWA_MAX8(1) DIRAL_SDWA_MAX8(2) DIRAL_SDWA_MAX8(3) "s_nop 0"
      : "+v"(a[0]), "+v"(a[1]), "+v"(a[2]), "+v"(a[3]), "+v"(a[4]), "+v"(a[5]), "+v"(a[6]), "+v"(a[7])
      : "v"(b[0]), "v"(b[1]), "v"(b[2]), "v"(b[3]), "v"(b[4]), "v"(b[5]), "v"(b[6]), "v"(b[7]));
#undef DIRAL_SDWA_MAX8
}
template <int NK>
__device__ inline void max_u8_words(unsigned int (&a)[NK], const unsigned int (&b)[NK]) {
  if constexpr (NK == 4) max_u8x16(a, b);
  else if constexpr (NK == 8) max_u8x32(a, b);
  else {
    static_assert(NK % 8 == 0, "4, 8 or a multiple of 8 words");
#pragma unroll
    for (int q = 0; q < NK; q += 8)
      max_u8x32(*reinterpret_cast<unsigned int (*)[8]>(&a[q]), *reinterpret_cast<const unsigned int (*)[8]>(&b[q]));
  }
}

#ifndef DIRAL_WIDE_INFLIGHT
#define DIRAL_WIDE_INFLIGHT 16          // table words a lane has in flight while a pass loads its columns
#endif

// run f(std::integral_constant<int, wave>) - a copy of f per wave index (wave-uniform switch): the wave's
// scratch base becomes an immediate offset of the LDS instructions; f(-1): base in a register
#define DIRAL_WIDE_DISPATCH_WAVE(f)                                      \
  do {                                                                   \
    if (!lds_base_is_zero) { f(std::integral_constant<int, -1>{}); break; } \
    switch (wave) {                                                      \
      case 0: f(std::integral_constant<int, 0>{}); break;                \
      case 1: f(std::integral_constant<int, 1>{}); break;                \
      case 2: f(std::integral_constant<int, 2>{}); break;                \
      case 3: f(std::integral_constant<int, 3>{}); break;                \
      case 4: f(std::integral_constant<int, 4>{}); break;                \
      case 5: f(std::integral_constant<int, 5>{}); break;                \
      case 6: f(std::integral_constant<int, 6>{}); break;                \
      default: f(std::integral_constant<int, 7>{}); break;               \
    }                                                                    \
  } while (0)

// byte j of the packed gather-source word, shifted left by SH (the LDS byte offset of that
// viewer's rank words), one SDWA shift each instead of extract + shift
template <int VPL, unsigned int SH>
__device__ inline void unpack_src(unsigned int mw, unsigned int (&a)[VPL]) {
  if constexpr (VPL == 4) {
    asm("v_lshlrev_b32_sdwa %0, %4, %5 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:BYTE_0\n\t"
        "v_lshlrev_b32_sdwa %1, %4, %5 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:BYTE_1\n\t"
        "v_lshlrev_b32_sdwa %2, %4, %5 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:BYTE_2\n\t"
        "v_lshlrev_b32_sdwa %3, %4, %5 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:BYTE_3"
        : "=&v"(a[0]), "=&v"(a[1]), "=&v"(a[2]), "=&v"(a[3]) : "s"(SH), "v"(mw));
  } else {
    asm("v_lshlrev_b32_sdwa %0, %2, %3 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:BYTE_0\n\t"
        "v_lshlrev_b32_sdwa %1, %2, %3 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:BYTE_1"
        : "=&v"(a[0]), "=&v"(a[1]) : "s"(SH), "v"(mw));
  }
}

// byte BYTE of a word of table indices, times 16: the LDS byte offset of that row of the bits -> bf16 table
// (step_wide_closure.inc), shift and byte extraction in one SDWA instruction
template <int BYTE>
__device__ inline unsigned int lut_row(unsigned int w) {
  unsigned int r;
  static_assert(BYTE >= 0 && BYTE < 4, "byte select");
  if constexpr (BYTE == 0) asm("v_lshlrev_b32_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:BYTE_0" : "=v"(r) : "s"(4u), "v"(w));
  if constexpr (BYTE == 1) asm("v_lshlrev_b32_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:BYTE_1" : "=v"(r) : "s"(4u), "v"(w));
  if constexpr (BYTE == 2) asm("v_lshlrev_b32_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:BYTE_2" : "=v"(r) : "s"(4u), "v"(w));
  if constexpr (BYTE == 3) asm("v_lshlrev_b32_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:BYTE_3" : "=v"(r) : "s"(4u), "v"(w));
  return r;
}

// Reward of a colliding resource (test_env.py:163-199) for N > 64, positions in
// LDS, all y == 0.  Out of line: runs ~once per colliding resource.
template <int VPL>
__device__ DIRAL_OUTLINE double wide_collision_reward(int rd, uint32_t flags, double L, double Rc, int N,
                                                                  const unsigned long long* mkp, int c,
                                                                  const double* s_px) {
  int wgt = 0;
  if (rd == 1 || ((rd == 2 || rd == 5) && c == 2)) {
    double s = 0.0;                    // calculate_avg_distance (network.py:307-316): combinations order
    int cnt = 0;
    for (int ja = 0; ja < VPL; ++ja) {
      unsigned long long ma = mkp[ja];
      while (ma) {
        const int a = ja * 64 + __builtin_ctzll(ma);
        ma &= ma - 1;
        for (int jb = ja; jb < VPL; ++jb) {
          unsigned long long mb = (jb == ja) ? ma : mkp[jb];
          while (mb) {
            const int b = jb * 64 + __builtin_ctzll(mb);
            mb &= mb - 1;
            s = s + dist2d_leaf(s_px[a], 0.0, s_px[b], 0.0);
            ++cnt;
          }
        }
      }
    }
    const double m = s / (double)cnt;
    if (flags & DIRAL_F_TOY_WEIGHTS) {
      double x_min = L + 1, x_max = -L - 1;      // calculate_norm (network.py:225-246)
      int umin = 0, umax = 0;
      for (int u = 0; u < N; ++u) {
        const double x = s_px[u];
        if (x < x_min) { x_min = x; umin = u; }
        if (x > x_max) { x_max = x; umax = u; }
      }
      wgt = (m == dist2d_leaf(s_px[umin], 0.0, s_px[umax], 0.0));
    } else {
      wgt = (m > Rc);
    }
  }
  // (collision_value, spelled out: see ref_math.hpp)
  if (rd == 1) { const double R = (double)wgt / (double)c; return -1.0 * (1.0 - R); }
  if (rd == 2) return (c == 2) ? 2.0 * (double)wgt - (double)c : 0.0 - (double)c;
  if (rd == 3) { const double R = 1.0 / (double)c; return -1.0 * exp(1.0 - R); }
  if (rd == 4) return 1.0 / (double)c;
  return (c == 2 && wgt == 1) ? 0.0 : -1.0;
}

// The far-entry guard of a flagged pass of the packed form at N <= 128 (step_wide_kernel, `cl_far_guard`: what it decides and
// why that is exact).  `rows`: the closure walk's rows of P in LDS, [half][viewer] 8 bytes - sources 0 .. 63 / 64 .. 127 of
// each viewer; `tcq`: the code words of the wave's four quads [quad][NV]; `tkw`: the env's `tkey` rows [subject][NV];
// `flagged`: bit pch = pass pch (8 columns) is flagged.  Returns the passes whose far entries cannot move this slot.
template <bool FULL>
__device__ __attribute__((noinline)) unsigned int wide_far_guard(const unsigned char* rows, int npad, const unsigned int* tcq,
                                                                 const unsigned int* tkw, int kbase, int N, int NV,
                                                                 unsigned int flagged, int lane) {
  constexpr int VPL = 2, PC = 8;
  typedef __attribute__((ext_vector_type(2))) unsigned int g_u32x2;
  const unsigned int ul = (unsigned int)lane;
  g_u32x2 plo[VPL], phi[VPL];
#pragma unroll
  for (int j = 0; j < VPL; ++j) {
    plo[j] = *reinterpret_cast<const g_u32x2*>(rows + 8u * (ul + 64u * j));
    phi[j] = *reinterpret_cast<const g_u32x2*>(rows + 8u * (unsigned int)npad + 8u * (ul + 64u * j));
  }
  unsigned int stable = 0u;
#pragma unroll 1
  for (int pch = 0; pch < 2; ++pch) {
    if (((flagged >> pch) & 1u) == 0u) continue;
    bool viol = false;
    unsigned int qfar = 0u;                     // bit w: quad w of the pass holds an entry beyond the codes (a sequence number in `tkey`)
    unsigned int cw[2][VPL];                   // the pass's raw code words (two quads x VPL slots)
#pragma unroll
    for (int w = 0; w < 2; ++w)
#pragma unroll
      for (int j = 0; j < VPL; ++j) cw[w][j] = tcq[(unsigned int)((2 * pch + w) * NV) + ul + 64u * j];
    // the sequence numbers of the pass's far entries, all 16 loads in flight together (a column at a time the guard paid a
    // round trip to HBM per column: 110 k cycles for a workgroup with two flagged passes)
    unsigned int seqa[PC][VPL];
    bool isfa[PC][VPL];
#pragma unroll
    for (int c = 0; c < PC; ++c) {
      const int k = kbase + pch * PC + c;
      const unsigned int* const tkrow = tkw + (size_t)(FULL || k < N ? k : kbase) * NV;
#pragma unroll
      for (int j = 0; j < VPL; ++j) {
        const unsigned int u = ul + 64u * j;
        const unsigned int rc = (cw[c >> 2][j] >> (8 * (c & 3))) & 255u;
        // beyond the codes once this slot's stamp is taken: raw code 0 (8 or more behind, or never heard) or 0x80 (7 behind:
        // handed over to `tkey` when it got there, vehicle.py:56-70 makes it 8 now)
        isfa[c][j] = (rc & 0x7fu) == 0u && (FULL || (u < (unsigned int)N && k < N));
        seqa[c][j] = tkrow[u] >> 8;              // (unconditional: a padded viewer reads inside the allocation, its value is masked)
      }
    }
#pragma unroll
    for (int c = 0; c < PC; ++c)
#pragma unroll
      for (int j = 0; j < VPL; ++j) seqa[c][j] = isfa[c][j] ? seqa[c][j] : 0u;
#pragma unroll
    for (int c = 0; c < PC; ++c) {
      unsigned int seqv[VPL];
      unsigned long long farm[VPL];
      bool isf[VPL];
#pragma unroll
      for (int j = 0; j < VPL; ++j) { isf[j] = isfa[c][j]; seqv[j] = seqa[c][j]; farm[j] = __ballot(isf[j]); }
      if ((farm[0] | farm[1]) == 0ull) continue;
      if ((__ballot(isf[0] && seqv[0] != 0u) | __ballot(isf[1] && seqv[1] != 0u)) != 0ull) qfar |= 1u << (c >> 2);
      unsigned long long rem[VPL];
#pragma unroll
      for (int j = 0; j < VPL; ++j) rem[j] = farm[j];
      while ((rem[0] | rem[1]) != 0ull) {          // over the distinct far numbers of the column (one, as a rule: nothing to propagate)
        const int js = rem[0] != 0ull ? 0 : 1;
        const unsigned int d = (unsigned int)__builtin_amdgcn_readlane((int)(js == 0 ? seqv[0] : seqv[1]), __builtin_ctzll(rem[js]));
        unsigned long long g[VPL];
        bool lower[VPL];
        bool anylower = false;
#pragma unroll
        for (int j = 0; j < VPL; ++j) {
          g[j] = __ballot(isf[j] && seqv[j] == d);
          rem[j] &= ~g[j];
          lower[j] = isf[j] && seqv[j] < d;
          anylower = anylower || lower[j];
        }
        if (__ballot(anylower) == 0ull) continue;  // (uniform) nobody holds an older number than d
#pragma unroll
        for (int j = 0; j < VPL; ++j) {
          const unsigned int hit = (plo[j][0] & (unsigned int)g[0]) | (plo[j][1] & (unsigned int)(g[0] >> 32)) |
                                   (phi[j][0] & (unsigned int)g[1]) | (phi[j][1] & (unsigned int)(g[1] >> 32));
          viol = viol || (lower[j] && hit != 0u);
        }
      }
    }
    // a stable pass: bit pch; its quads without a far entry any more (refreshed since they were flagged): bits 8 + quad -
    // the caller takes their flags down (the coded path only ever raises them: at a hand-over)
    if (__ballot(viol) == 0ull) stable |= (1u << pch) | ((~qfar & 3u) << (8 + 2 * pch));
  }
  return stable;
}

#ifdef DIRAL_TIMING
#define DIRAL_WSTAMP(i) do { if (lane == 0 && p.dbg) p.dbg[((size_t)b * WAVES + wave) * 8 + (i)] = __builtin_amdgcn_s_memtime(); } while (0)
#define DIRAL_WCLOCK(v) v = __builtin_amdgcn_s_memtime()
#else
#define DIRAL_WSTAMP(i) do {} while (0)
#define DIRAL_WCLOCK(v) do {} while (0)
#endif
#ifndef DIRAL_WIDE_MINWAVES2
#define DIRAL_WIDE_MINWAVES2 8           // N <= 128: 64 VGPRs, four 512-thread workgroups per CU (35 KB of LDS each).  Before the xpos ring
                                         // freed the xpos prefetch registers: 1.61 / 1.68 / 1.76 ms for 6 / 7 / 8; with it 1.375 / 1.386 / 1.349 ms
                                         // (with the channel observation 1.46 / 1.47 / 1.33)
#endif
#ifndef DIRAL_WIDE_MINWAVES4
#define DIRAL_WIDE_MINWAVES4 6           // N <= 256: 84 VGPRs, three 512-thread workgroups per CU
#endif
#ifndef DIRAL_WIDE_MINWAVES4P
#define DIRAL_WIDE_MINWAVES4P 4          // ... the packed form: 128 VGPRs (the product's A operand alone takes 64), two workgroups per CU
#endif
#ifndef DIRAL_WIDE_FLAG_UNROLL
#define DIRAL_WIDE_FLAG_UNROLL 1         // column loops of a flagged pass's unpack / repack stages (4 - the four loads of a word in flight together - measured C5 + 4 %: registers)
#endif
#ifndef DIRAL_WIDE_MINWAVES2P
#define DIRAL_WIDE_MINWAVES2P 6          // N <= 128, packed form: 84 VGPRs, three workgroups per CU (43 KB of LDS each)
#endif

// The template parameters of the kernels in step_wide_body.inc:
// FULL: N == 64 * VPL (every viewer slot and subject row exists): the u < N / k < N predicates
// are compiled out (BASELINE.json's 128- and 256-vehicle configurations)
// CH: my_step_ch (PRR reward, test_env.py:351-443) instead of my_step, as in step_fast64.hpp
// EXTRA: run-time switches for my_step_design and the arrival stamps, as in step_fast64.hpp
// RICH: the output tail of rich_out.hpp (channel observation output, cheap State flags)
// PACKED: the table form (the host decides per handle, csrc/diral_env.hip `use_packed_table`): codes + ages + own sequence
// numbers, or the round-2 (seq, age) plane `tkey` whose passes re-derive the lags every slot and fall back to byte
// ranks in place.  Dense topologies (BASELINE configs[2] and [4]) run packed - the coded passes merge as reachability
// closure + one bf16 product, step_wide_closure.inc -; where most entries lag their subject by more than 7 stamps (sparse
// topologies) every pass of the packed form would detour through the planes - those handles keep the plane form.

// The SPS agents of one wave decide for the next slot (step_wide_slots_kernel, k_wide_slots.hip): what
// sps_step_wave_kernel<1, T, true> does with the rows of the channel observation it loads, for the 64 vehicles
// 64 wave + lane.  Which agents re-select is fixed by sps_advance before any row is needed (counter and a draw), and the
// row of a re-selecting agent is rebuilt from what P1 left in LDS - gather sources, positions, actions, the resources with
// a transmitter - as the output tail writes `obs[user][i]`, rounded to the output dtype T: any number of re-selecting
// agents, nothing staged.  `ks`: slot ks of the launch draws with seed + ks, what K one-slot calls are given.
template <typename T, int VPL, int MT>
__device__ DIRAL_OUTLINE void wide_sps_decide(const PolParams* q, const int* s_act, const double* s_px,
                                              const typename std::conditional<VPL == 4, uint32_t, uint16_t>::type* s_mtab,
                                              unsigned long long actw, bool dist_obs, int N, int A, size_t bN, int wave,
                                              int lane, int ks) {
  const uint64_t seed = q->seed + (uint64_t)ks + (q->clock ? (uint64_t)*q->clock : 0ull);
  const int u = 64 * wave + lane;
  const int i = (int)bN + u;
  const bool live = u < N;
  int action = live ? q->sps_prev[i] : 0;
  int cnt = live ? q->sps_counter[i] : 1;
  const bool resel = live && sps_advance(i, cnt, q->keep_prob, q->draw_counter, q->draw_keep, seed);
  unsigned int r = 0;
  if (resel) r = q->draw_choice ? (unsigned int)q->draw_choice[i] : (unsigned int)(rng_u64(seed, 9, (uint64_t)i) >> 33);
  unsigned long long todo = __ballot(resel);
  while (todo) {
    const int j = __builtin_ctzll(todo);
    todo &= todo - 1;
    const int uj = 64 * wave + j;
    const int prev_j = __builtin_amdgcn_readlane(action, j);
    const int own_j = s_act[uj];
    const unsigned int r_j = (unsigned int)__builtin_amdgcn_readlane((int)r, j);
    double d[1];
    d[0] = 0.0;
    if (lane < A) {                                          // obs[uj][lane], as the output tail writes it
      double v;
      if (own_j == lane || ((actw >> lane) & 1ull) == 0ull) v = 0.0;
      else if (!dist_obs) v = 1.0;
      else {
        const int src = (int)(((unsigned int)s_mtab[lane * MT + (uj & 63)] >> (8 * (uj >> 6))) & 255u);
        v = src == uj ? 100000.0 : fast_dist<true>(s_px[src], 0.0, s_px[uj], 0.0);   // network.py:385
      }
      d[0] = (double)(T)v;
    }
    const int ch = sps_choose_chobs_wave<1>(d, lane, A, prev_j, own_j, q->threshold, q->inc_db, r_j);
    if (lane == j) action = ch;
  }
  if (live) {
    q->sps_prev[i] = action;                                 // (unchanged unless re-selected: v2x_sps.py:98)
    q->sps_counter[i] = cnt;
    q->actions_out[i] = action;
  }
}

}  // namespace diral
