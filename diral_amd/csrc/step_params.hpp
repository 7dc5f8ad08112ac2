// step_params.hpp - what the host (diral_env.hip) and the step_fast64 / step_wide kernels share without sharing a kernel:
// the parameter block FastParams, the limits launches are planned with, the late-bound kernel arguments.  No __global__ here.
#pragma once
#include "common.hpp"
#include "policy_device.hpp"
#include "rich_out.hpp"

namespace diral {

constexpr int kFastMaxA = 64;           // LDS is sized by the actual A (rounded up to 32): A <= 32 keeps 8 workgroups per CU
constexpr int kWideMaxA = 64;

// Index arithmetic of the write-out loops of step_fast64 in 16-byte pieces (CV = 4 floats or 2 doubles): the channel
// observation, qa = A / CV pieces per row, and the state rows of P4, qs = (A + K) / CV.  Every operand is uniform and known
// to the host, so the divisions are done there, once per launch.  i / q is (i * mul) >> shift with mul = ceil(2^shift / q),
// shift = 16 + ceil(log2 q): with e = mul * q - 2^shift < q <= 2^(shift - 16) the quotient is exact while i * e < 2^shift,
// that is for every i < 2^16; both factors stay below 2^24 and the product below 2^32 for i < 2^15 (q <= 2^12): a full-rate
// v_mul_u32_u24.  The kernel divides a thread index < 256.
struct WriteoutParams {
  int qa_mul, qa_shift;          // i / qa
  int co_du, co_dq;              // 256 / qa and 256 % qa: what a thread of the channel-observation loop advances by
  int qs_mul, qs_shift;          // i / qs
  int p4_du3, p4_dq3;            // 192 / qs and 192 % qs: P4 by waves 1-3 (`late_p2`)
  int p4_du4, p4_dq4;            // 256 / qs and 256 % qs: P4 by all four waves
};
__host__ __device__ inline void writeout_reciprocal(int q, int& mul, int& shift) {
  mul = 0; shift = 16;
  if (q <= 0) return;
  while ((1 << (shift - 16)) < q) ++shift;
  mul = (int)(((1ll << shift) + q - 1) / q);
}
// (A, or A and K, that are no multiples of CV: that loop writes element by element and reads none of these)
__host__ __device__ inline WriteoutParams writeout_params(int A, int K, bool out_f64) {
  const int cv = out_f64 ? 2 : 4;
  const int qa = (A % cv) == 0 ? A / cv : 0;
  const int qs = (A % cv) == 0 && (K % cv) == 0 ? (A + K) / cv : 0;
  WriteoutParams w;
  writeout_reciprocal(qa, w.qa_mul, w.qa_shift);
  w.co_du = qa ? 256 / qa : 0; w.co_dq = qa ? 256 % qa : 0;
  writeout_reciprocal(qs, w.qs_mul, w.qs_shift);
  w.p4_du3 = qs ? 192 / qs : 0; w.p4_dq3 = qs ? 192 % qs : 0;
  w.p4_du4 = qs ? 256 / qs : 0; w.p4_dq4 = qs ? 256 % qs : 0;
  return w;
}

struct FastParams {
  int N, A, K, NR;               // NR: padded subject rows (multiple of 16); viewer stride is 64
  int NV;                        // viewer stride (step_wide.hpp; 64 for step_fast64)
  uint32_t flags;
  int reward_design, age_limit, episode_interval;
  int design;                    // 1: my_step_design (test_env.py:269-349) - runtime switch of the non-CH instantiation
  int done_now;                  // t % episode_interval == episode_interval - 1 (main_test.py:226), evaluated on the host
  int notab;                     // 1: State.add_positional_dist_piggy is off - the reference keeps no neighbour tables at all
                                 // (test_env.py:138-139, 231-238: no periodic_update, no received_update): stamp, merge and
                                 // histogram are skipped - EXTRA + RICH instantiations
  int nomove;                    // 1: static topology (`mobility: False` with the design topology, network.py:54-60, 302-305):
                                 // update_mobility does nothing - EXTRA instantiations
  int prr;                       // 1: my_step also accumulates the PRR metric columns (DIRAL_F_TRACK_PRR, a build extension:
                                 // the reception ratio of test_env.py:384-405 per colliding transmitter) - EXTRA instantiations
  int chobs_mode;                // RICH: bit 0 = chobs_out is set; bit 1 = the channel observation is the distance to the
                                 // closest in-range transmitter (my_step with State.type 2) instead of the constant 1
                                 // (my_step_ch, my_step_design, State.type 1).  Host-folded: P1 touches no RichParams field
  double L, Rc, Rb, inv_w;
  long long t;
  const long long* t_dev;        // slot clock (diral_env_set_clock) or null: the slot number is t + *t_dev, read on the device -
                                 // a captured hipGraph of K steps replays with a clock that moves on
  const int32_t* actions;
  double* pos_x;
  const double* pos_y;
  const double* vel;
  uint32_t* tkey;
  double* tx;
  double* ring;                  // [B][NR][8] xpos ring (always set for step_fast64; step_wide: null = every xpos from the plane)
  // the PACKED table of step_fast64: what the merge works on is what is stored.  Row-quad q = k / 4:
  uint32_t* tcode;               // [B][NR/4][64]: byte c = thermometer code of the lag of viewer u's entry about subject 4q + c
                                 // (0xff << lag for lag 0..7; 0 = never heard, or older than 7: then `tkey` holds its sequence number)
  uint32_t* tage;                // [B][NR/4][64]: byte c = last_updated (saturating at 255) of the same entry - EVERY entry
  uint32_t* tseq;                // [B][NR]: the subjects' own sequence numbers
  uint32_t* told;                // [B][NR/4]: != 0: the quad holds an entry older than the codes reach -> keyed path
  int32_t* la;                   // last_arrival_time[tx][rx] (network.py:39-42) or null: not tracked
  const double* trace;           // replayed x positions (network.py:171-178, 194-199) or null
  int trace_len, trace_per_env;
  double* metrics;
  uint32_t* err;
  const double* edges;
  const double* inv_tab;          // [256] 1.0 / n (0 for n = 0): the f32 histogram output multiplies instead of dividing
  void* state_out;                // float* or double* (OUT64)
  void* rew_out;
  uint8_t* done_out;
  unsigned long long* dbg;
  int B;                          // envs of the handle (the grid may be larger: slow-first blocks below)
  // float32 screening of the histogram bin in the fast quads (P3b): the bin of v = xpos - own position computed from
  // float32 copies, exact whenever its fraction is further than `f32_m16` / 65536 bin widths from an integer (the
  // host's bound on everything float32 can lose for positions up to `f32_xmax`); lanes inside the band take the
  // float64 statement.  f32_m16 = 0: off (a highway too long for float32 to be worth it).
  int f32_m16;
  float f32_xmax;
  // Slow envs first (step_fast64 only).  An env whose tables hold entries beyond the codes runs its
  // quads on the keyed path and takes two to three times as long as the others; a launch ends when its last workgroup
  // does, so such a workgroup must not be among the last to START.  Every launch leaves, for the next one, the list of
  // the envs it found slow (`told` flags set for the next slot) and a flag per env; the next launch runs the listed envs
  // in its first fast_slow_max(B) blocks - dispatched first - and the block that would have taken such an env in dispatch
  // order exits at once.  Three rotating sets (the host counts launches): read set r, build set r + 1, EMPTY set r + 2
  // (its count and every env's flag: at every launch boundary each set is either a complete list or empty, so a launch
  // that reads any of them - a captured launch replays against the set it was baked with, whatever the eager launches in
  // between did to it - steps every env exactly once).  A captured launch gets the read set only (slow_*_w / _z null: a
  // replayed graph cannot rotate), unless the graph rotates as a whole (diral_env_set_capture_rotation).
  // slow_cnt_r null: blocks = envs in order (DIRAL_NO_SLOW_FIRST).
  const uint32_t* slow_cnt_r;     // [1] number of listed envs
  const uint32_t* slow_list_r;    // [fast_slow_max(B)]
  const uint32_t* slow_flag_r;    // [B] != 0: listed
  uint32_t* slow_cnt_w;
  uint32_t* slow_list_w;
  uint32_t* slow_flag_w;
  uint32_t* slow_cnt_z;           // the set [count | list | flags] the launch after the next will build: emptied here
  WriteoutParams wo;              // step_fast64 only, read late (LateFastArgs) where the write-out loops start
};
// listed envs per launch (an env beyond that keeps its place in dispatch order): a quarter of the batch, 16 ... 4096
#ifndef DIRAL_SLOW_SHIFT
#define DIRAL_SLOW_SHIFT 2             // a quarter of the batch (an eighth: sticky policies overflow the list, c2_sticky_0.9 58 -> 52 us; half: no better)
#endif
__host__ __device__ inline int fast_slow_max(int B) { const int m = B >> DIRAL_SLOW_SHIFT; return m < 16 ? 16 : (m > 4096 ? 4096 : m); }

// Late-bound kernel arguments.  The compiler hoists the scalar loads of EVERY by-value kernel
// argument to the kernel entry and then keeps (or spills, through v_writelane / v_readlane - VALU
// instructions inside the hot loops) the SGPRs of values only the last phases use: output
// pointers, section offsets.  Reading such fields through the kernarg segment pointer behind an
// opaque asm pins their s_load to the point of use instead (SGPR spills of every instantiation:
// profiles/r02/resource_usage.txt).
typedef const __attribute__((address_space(4))) FastParams* LateFastArgs;
__device__ inline unsigned long long late_kernarg_base() {
  unsigned long long a = (unsigned long long)__builtin_amdgcn_kernarg_segment_ptr();
  asm volatile("" : "+s"(a));
  return a;
}
__device__ inline WriteoutParams load_writeout_args(unsigned long long kernarg_base) {
  const LateFastArgs a = (LateFastArgs)kernarg_base;
  WriteoutParams w;
  w.qa_mul = a->wo.qa_mul; w.qa_shift = a->wo.qa_shift; w.co_du = a->wo.co_du; w.co_dq = a->wo.co_dq;
  w.qs_mul = a->wo.qs_mul; w.qs_shift = a->wo.qs_shift; w.p4_du3 = a->wo.p4_du3; w.p4_dq3 = a->wo.p4_dq3;
  w.p4_du4 = a->wo.p4_du4; w.p4_dq4 = a->wo.p4_dq4;
  return w;
}
// byte offset of the second kernel argument (RichParams) in the kernarg segment
constexpr unsigned long long kRichArgOffset = (sizeof(FastParams) + alignof(RichParams) - 1) / alignof(RichParams) * alignof(RichParams);
typedef const __attribute__((address_space(4))) RichParams* LateRichArgs;
// ... and of the third (PolParams)
constexpr unsigned long long kPolArgOffset = (kRichArgOffset + sizeof(RichParams) + alignof(PolParams) - 1) / alignof(PolParams) * alignof(PolParams);
typedef const __attribute__((address_space(4))) PolParams* LatePolArgs;
__device__ inline RichParams load_rich_args(unsigned long long kernarg_base) {
  const LateRichArgs a = (LateRichArgs)(kernarg_base + kRichArgOffset);
  RichParams r;
  r.chobs_out = a->chobs_out; r.S = a->S; r.state_type = a->state_type; r.plain_state = a->plain_state;
  r.off_act = a->off_act; r.off_chobs = a->off_chobs; r.off_hist = a->off_hist; r.off_rew = a->off_rew;
  r.off_idx = a->off_idx; r.off_pos = a->off_pos; r.off_vel = a->off_vel; r.off_fp = a->off_fp;
  r.off_skip = a->off_skip; r.len_skip = a->len_skip;
  r.H = a->H; r.episode = a->episode; r.eps = a->eps; r.vel = a->vel; r.pos_y = a->pos_y;
  r.pf = a->pf; r.pf_threshold = a->pf_threshold; r.pf_penalty = a->pf_penalty;
  return r;
}

}  // namespace diral
