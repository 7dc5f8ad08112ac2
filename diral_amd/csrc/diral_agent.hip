// diral_agent.hip - the agent side of include/diral_env.h: the entry points that take device pointers and no handle (the SPS
// baseline policy, the slot clock, the driver's reward shaping, action selection, the replay memory, the TD head, the dense
// Q-network).  Argument checks, then launches; the env handle and everything it owns is diral_env.hip's.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <initializer_list>

#include "agent_host.hpp"
#include "agent_kernels.hpp"
#include "host_util.hpp"
#include "memory_kernel.hpp"
#include "qnet_params.hpp"
#include "select_kernel.hpp"
#include "td_kernel.hpp"

using namespace diral;

namespace {

// the dtype codes an argument takes
bool f32_or_f64(int dtype) { return dtype == DIRAL_F32 || dtype == DIRAL_F64; }
bool f32_f16_or_bf16(int dtype) { return dtype == DIRAL_F32 || dtype == DIRAL_F16 || dtype == DIRAL_BF16; }

// sps_step_wave_kernel, one wave lane per 1 / 2 / 4 resources (num_channels <= kSpsWaveMaxA).  `src` holds T: the float64
// selection window, or (CHOBS) the env's channel observation in its own dtype; `rest`: the kernel's other arguments
template <typename T, bool CHOBS, typename... Rest>
hipError_t launch_sps_wave(int agents, int num_channels, const void* src, hipStream_t s, Rest... rest) {
  const T* in = static_cast<const T*>(src);
  if (num_channels <= 64) return launch_1d<sps_step_wave_kernel<1, T, CHOBS>>((size_t)agents, s, agents, num_channels, in, rest...);
  if (num_channels <= 128) return launch_1d<sps_step_wave_kernel<2, T, CHOBS>>((size_t)agents, s, agents, num_channels, in, rest...);
  return launch_1d<sps_step_wave_kernel<4, T, CHOBS>>((size_t)agents, s, agents, num_channels, in, rest...);
}

// The launch of the kernels that give a row of A values to 2^gshift lanes (select_actions_kernel, td_head_kernel) or, past
// 64 values, to a wave of its own (their _wide_ forms).  gshift: the power of two >= A, at least 4 lanes
struct RowLaunch { int gshift; dim3 grid, block; };
RowLaunch row_launch(int rows, int A, int narrow_block) {
  int gshift = 0;
  while ((1 << gshift) < A || gshift < 2) ++gshift;
  if (A > 64) return {gshift, dim3((uint32_t)rows), dim3(64)};
  const size_t waves = ((size_t)rows + (64u >> gshift) - 1) >> (6 - gshift);
  return {gshift, dim3(blocks(waves * 64, narrow_block)), dim3(narrow_block)};
}

// VEC of the memory kernels: the widest of 4 / 2 / 1 elements per lane that `values` per block and the addresses allow
int mem_vec(long long values, size_t elem, std::initializer_list<const void*> ptrs) {
  for (int v = 4; v > 1; v >>= 1) {
    bool ok = values % v == 0;
    for (const void* q : ptrs) ok = ok && (q == nullptr || (uintptr_t)q % (elem * v) == 0);
    if (ok) return v;
  }
  return 1;
}

// memory_sample_kernel and memory_history_kernel move items of NS = num_users * state_space ring values to rows of
// `out_dtype`: what the ring converts to ...
bool mem_out_ok(const DiralMemory* m, int out_dtype) { return m->dtype == DIRAL_F64 ? f32_or_f64(out_dtype) : f32_f16_or_bf16(out_dtype); }
// ... the shape of such a launch: VEC, VEC-wide stores where every one of `outs` allows them, the threads per item, and per
// XCD `per_xcd` items, kMemBlock >> ushift of them to a workgroup (memory_kernel.hpp) ...
struct MemItems { int vec, vst, ushift; dim3 grid; };
MemItems mem_items(const DiralMemory* m, int out_dtype, size_t per_xcd, std::initializer_list<const void*> outs) {
  const long long NS = (long long)m->num_users * m->state_space;
  const size_t er = m->dtype == DIRAL_F64 ? 8 : 4, eo = out_dtype == DIRAL_F64 ? 8 : out_dtype == DIRAL_F32 ? 4 : 2;
  MemItems t{};
  t.vec = mem_vec(NS, er, {m->states});
  t.vst = t.vec > 1 && mem_vec(m->state_space, eo, outs) >= t.vec;
  t.ushift = NS / t.vec <= 256 ? 6 : 8;                             // a wave per item up to four loads per lane
  const size_t ipb = (size_t)(kMemBlock >> t.ushift);
  t.grid = dim3((uint32_t)(8 * ((per_xcd + ipb - 1) / ipb)));
  return t;
}
// ... and its instantiation: `f` is handed the ring type, the out type and VEC
template <typename F>
hipError_t by_ring_out_vec(const DiralMemory* m, int out_dtype, int vec, F&& f) {
  return by_vec(vec, [&](auto v) {
    if (m->dtype == DIRAL_F64) return out_dtype == DIRAL_F64 ? f(double{}, double{}, v) : f(double{}, float{}, v);
    return out_dtype == DIRAL_F32 ? f(float{}, float{}, v) : out_dtype == DIRAL_F16 ? f(float{}, _Float16{}, v) : f(float{}, bf16_bits{}, v);
  });
}

}  // namespace

namespace diral {

bool memory_ok(const DiralMemory* m) {
  return m && m->struct_bytes == sizeof(DiralMemory) && m->states && m->actions && m->rewards && m->capacity >= 1 && m->batch >= 1 &&
         m->num_users >= 1 && m->state_space >= 1 && f32_or_f64(m->dtype) && (m->count_dev || m->count >= 0);
}

int sps_step_chobs_with_clock(int agents, int num_channels, const void* chobs, int chobs_dtype, const int32_t* actions,
                              int32_t* prev_action, int32_t* counter, double rssi_threshold, double inc_db,
                              double keep_prob, const int32_t* draw_counter, const double* draw_keep,
                              const int32_t* draw_choice, uint64_t seed, const long long* clock, int32_t* actions_out,
                              void* stream) {
  if (agents < 1 || num_channels < 1 || !chobs || !actions || !prev_action || !counter || !actions_out)
    return DIRAL_ERR_BAD_ARG;
  if (!f32_or_f64(chobs_dtype)) return DIRAL_ERR_BAD_ARG;
  if (num_channels > kSpsWaveMaxA) return DIRAL_ERR_UNSUPPORTED;   // use window_from_chobs + sps_step
  DEVICE_ENTER(prev_action);
  return hip_status(by_dtype(chobs_dtype, [&](auto tag) {
    return launch_sps_wave<decltype(tag), true>(agents, num_channels, chobs, (hipStream_t)stream, actions, prev_action, counter,
                                                rssi_threshold, inc_db, keep_prob, draw_counter, draw_keep, draw_choice, seed,
                                                clock, actions_out);
  }));
}

}  // namespace diral

extern "C" {

int diral_sps_init(int agents, int selection_window, int32_t* prev_action, int32_t* counter, uint64_t seed,
                   void* stream) {
  if (agents < 1 || selection_window < 0 || !prev_action || !counter) return DIRAL_ERR_BAD_ARG;
  DEVICE_ENTER(prev_action);
  return hip_status(launch_1d<sps_init_kernel>((size_t)agents, (hipStream_t)stream, agents, selection_window, seed, prev_action, counter));
}

int diral_sps_step(int agents, int num_channels, const double* selection_window, int32_t* prev_action,
                   int32_t* counter, double rssi_threshold, double inc_db, double keep_prob,
                   const int32_t* draw_counter, const double* draw_keep, const int32_t* draw_choice, uint64_t seed,
                   int32_t* actions_out, void* stream) {
  if (agents < 1 || num_channels < 1 || !selection_window || !prev_action || !counter || !actions_out)
    return DIRAL_ERR_BAD_ARG;
  DEVICE_ENTER(prev_action);
  const hipStream_t s = (hipStream_t)stream;
  if (num_channels <= kSpsWaveMaxA)
    return hip_status(launch_sps_wave<double, false>(agents, num_channels, selection_window, s, (const int32_t*)nullptr, prev_action,
                                                     counter, rssi_threshold, inc_db, keep_prob, draw_counter, draw_keep,
                                                     draw_choice, seed, (const long long*)nullptr, actions_out));
  // one thread per agent
  return hip_status(launch_k<sps_step_kernel>(dim3(blocks((size_t)agents, 128)), dim3(128), 0, s, agents, num_channels,
                                              selection_window, prev_action, counter, rssi_threshold, inc_db, keep_prob,
                                              draw_counter, draw_keep, draw_choice, seed, actions_out));
}

int diral_sps_window_from_chobs(int agents, int num_channels, const void* chobs, int chobs_dtype,
                                const int32_t* actions, double* window_out, void* stream) {
  if (agents < 1 || num_channels < 1 || !chobs || !actions || !window_out) return DIRAL_ERR_BAD_ARG;
  if (!f32_or_f64(chobs_dtype)) return DIRAL_ERR_BAD_ARG;
  DEVICE_ENTER(chobs);
  const size_t total = (size_t)agents * num_channels;
  return hip_status(by_dtype(chobs_dtype, [&](auto tag) {
    using T = decltype(tag);
    return launch_1d<sps_window_kernel<T>>(total, (hipStream_t)stream, total, num_channels, static_cast<const T*>(chobs), actions, window_out);
  }));
}

int diral_sps_step_chobs(int agents, int num_channels, const void* chobs, int chobs_dtype, const int32_t* actions,
                         int32_t* prev_action, int32_t* counter, double rssi_threshold, double inc_db,
                         double keep_prob, const int32_t* draw_counter, const double* draw_keep,
                         const int32_t* draw_choice, uint64_t seed, int32_t* actions_out, void* stream) {
  return sps_step_chobs_with_clock(agents, num_channels, chobs, chobs_dtype, actions, prev_action, counter, rssi_threshold,
                                   inc_db, keep_prob, draw_counter, draw_keep, draw_choice, seed, nullptr, actions_out, stream);
}

int diral_sps_step_chobs_clocked(int agents, int num_channels, const void* chobs, int chobs_dtype, const int32_t* actions,
                                 int32_t* prev_action, int32_t* counter, double rssi_threshold, double inc_db,
                                 double keep_prob, uint64_t seed, const int64_t* clock, int32_t* actions_out, void* stream) {
  if (!clock) return DIRAL_ERR_BAD_ARG;
  return sps_step_chobs_with_clock(agents, num_channels, chobs, chobs_dtype, actions, prev_action, counter, rssi_threshold,
                                   inc_db, keep_prob, nullptr, nullptr, nullptr, seed, (const long long*)clock, actions_out, stream);
}

int diral_clock_add(int64_t* clock, int64_t inc, void* stream) {
  if (!clock) return DIRAL_ERR_BAD_ARG;
  DEVICE_ENTER(clock);
  return hip_status(launch_k<clock_add_kernel>(dim3(1), dim3(1), 0, (hipStream_t)stream, (long long*)clock, (long long)inc));
}

int diral_driver_shape(int envs, int num_users, int num_channels, const void* reward_in, int dtype,
                       const int32_t* actions, const int32_t* ia, int64_t* sum_ia_prev, int32_t* pen_counter,
                       int32_t* prev_actions, int flags, int ia_penalty_threshold, double ia_penalty_value,
                       void* reward_out, void* sum_r_out, void* collision_out, int64_t* ia_sum_out,
                       int32_t* ia_penalty_out, void* stream) {
  if (envs < 1 || num_users < 1 || !reward_in || !reward_out) return DIRAL_ERR_BAD_ARG;
  if (!f32_or_f64(dtype)) return DIRAL_ERR_BAD_ARG;
  if ((flags & 4) && (!actions || !pen_counter || !prev_actions)) return DIRAL_ERR_BAD_ARG;
  if ((flags & 2) && (!ia || !sum_ia_prev)) return DIRAL_ERR_BAD_ARG;
  DEVICE_ENTER(reward_in);
  return hip_status(by_dtype(dtype, [&](auto tag) {
    using T = decltype(tag);
    const T* in = static_cast<const T*>(reward_in);
    T *out = static_cast<T*>(reward_out), *sum = static_cast<T*>(sum_r_out), *coll = static_cast<T*>(collision_out);
    if (!ia && !(flags & 2) && num_users >= 8 && num_users <= 64)   // no information-age terms, one wave per env (agent_kernels.hpp)
      return launch_k<driver_shape_wave_kernel<T>>(dim3(blocks((size_t)envs, kShapeWaveBlock / 64)), dim3(kShapeWaveBlock), 0,
                                                   (hipStream_t)stream, envs, num_users, num_channels, in, actions, pen_counter,
                                                   prev_actions, flags, ia_penalty_threshold, ia_penalty_value, out, sum, coll);
    return launch_k<driver_shape_kernel<T>>(dim3(blocks((size_t)envs, kShapeEnvsPerBlock)), dim3(256), 0, (hipStream_t)stream, envs,
                                            num_users, num_channels, in, actions, ia, (long long*)sum_ia_prev, pen_counter,
                                            prev_actions, flags, ia_penalty_threshold, ia_penalty_value, out, sum, coll,
                                            (long long*)ia_sum_out, ia_penalty_out);
  }));
}

int diral_policy_select(const DiralSelect* s, void* stream) {
  if (!s || s->struct_bytes != sizeof(DiralSelect) || !s->q || !s->actions_out) return DIRAL_ERR_BAD_ARG;
  if (s->agents < 1 || s->num_channels < 1 || s->num_users < 1 || s->agents % s->num_users != 0) return DIRAL_ERR_BAD_ARG;
  if (s->kind < DIRAL_SELECT_GREEDY || s->kind > DIRAL_SELECT_BOLTZMANN) return DIRAL_ERR_BAD_ARG;
  if (s->q_dtype < DIRAL_F32 || s->q_dtype > DIRAL_BF16) return DIRAL_ERR_BAD_ARG;
  if (s->kind == DIRAL_SELECT_SOFTMAX && !s->param_dev && !(s->tmp > 0.0 && std::isfinite(s->tmp))) return DIRAL_ERR_BAD_ARG;
  if (s->param_per_env && !s->param_dev) return DIRAL_ERR_BAD_ARG;
  if (s->num_channels > kSelMaxA) return DIRAL_ERR_UNSUPPORTED;
  DEVICE_ENTER(s->q);
  const int A = s->num_channels;
  const RowLaunch rl = row_launch(s->agents, A, kSelBlock);
  SelParams p{};
  p.q = s->q; p.agents = s->agents; p.N = s->num_users; p.A = A; p.gshift = rl.gshift;
  p.param = s->kind == DIRAL_SELECT_EPS_GREEDY ? s->eps : s->kind == DIRAL_SELECT_SOFTMAX ? s->tmp : s->explore_p;
  p.beta = s->beta; p.alpha = s->alpha;
  p.param_dev = s->kind == DIRAL_SELECT_GREEDY ? nullptr : s->param_dev; p.param_per_env = s->param_per_env;
  p.draw_u = s->draw_u; p.draw_a = s->draw_a; p.seed = s->seed; p.idx0 = s->idx0;
  p.clock = (const long long*)s->clock; p.clock_offset = (long long)s->clock_offset;
  p.actions_out = s->actions_out; p.explored_out = s->explored_out; p.bad_rows = s->bad_rows;
  const hipStream_t st = (hipStream_t)stream;
  auto launch = [&](auto tag, auto kind) {
    using QT = decltype(tag);
    constexpr int KIND = decltype(kind)::value;
    if (A > 64) {
      const uint32_t lds = (KIND == kSelSoftmax || KIND == kSelBoltzmann) ? (uint32_t)A * 8u : 0u;
      return launch_k<select_actions_wide_kernel<QT, KIND>>(rl.grid, rl.block, lds, st, p);
    }
    return launch_k<select_actions_kernel<QT, KIND>>(rl.grid, rl.block, 0, st, p);
  };
  auto by_q = [&](auto kind) {
    switch (s->q_dtype) {
      case DIRAL_F64: return launch(double{}, kind);
      case DIRAL_F32: return launch(float{}, kind);
      case DIRAL_F16: return launch(_Float16{}, kind);
      default: return launch(bf16_bits{}, kind);
    }
  };
  switch (s->kind) {
    case DIRAL_SELECT_GREEDY: return hip_status(by_q(std::integral_constant<int, kSelGreedy>{}));
    case DIRAL_SELECT_EPS_GREEDY: return hip_status(by_q(std::integral_constant<int, kSelEpsGreedy>{}));
    case DIRAL_SELECT_SOFTMAX: return hip_status(by_q(std::integral_constant<int, kSelSoftmax>{}));
    default: return hip_status(by_q(std::integral_constant<int, kSelBoltzmann>{}));
  }
}

int diral_memory_add(const DiralMemory* m, const DiralMemoryAdd* a, void* stream) {
  if (!memory_ok(m) || !a || a->struct_bytes != sizeof(DiralMemoryAdd)) return DIRAL_ERR_BAD_ARG;
  if (a->slots < 1 || a->slots > m->capacity || !a->next_states || !a->actions || !a->rewards) return DIRAL_ERR_BAD_ARG;
  if (!f32_or_f64(a->src_dtype) || !f32_or_f64(a->rewards_dtype)) return DIRAL_ERR_BAD_ARG;
  DEVICE_ENTER(m->states);
  MemAddParams p{};
  p.states = m->states; p.actions = m->actions; p.rewards = m->rewards;
  p.C = m->capacity; p.K = a->slots;
  p.BN = (long long)m->batch * m->num_users; p.BNS = p.BN * m->state_space;
  p.count = (long long)m->count; p.count_dev = (const long long*)m->count_dev;
  p.next_states = a->next_states; p.state0 = a->state0; p.a_in = a->actions; p.r_in = a->rewards;
  p.r_f64 = a->rewards_dtype == DIRAL_F64; p.r_bcast = a->rewards_broadcast != 0;
  const size_t es = a->src_dtype == DIRAL_F64 ? 8 : 4, er = m->dtype == DIRAL_F64 ? 8 : 4;
  const int vec = std::min(mem_vec(p.BNS, es, {a->next_states, a->state0}), mem_vec(p.BNS, er, {m->states}));
  const int ny = p.K + (p.state0 ? 1 : 0);
  const dim3 grid((uint32_t)std::min<size_t>(blocks((size_t)p.BNS / vec, kMemBlock), 4096), (uint32_t)std::min(ny, 65535));
  const hipStream_t st = (hipStream_t)stream;
  return hip_status(by_dtype(a->src_dtype, [&](auto src) {
    return by_dtype(m->dtype, [&](auto ring) {
      return by_vec(vec, [&](auto v) {
        return launch_k<memory_add_kernel<decltype(src), decltype(ring), decltype(v)::value>>(grid, dim3(kMemBlock), 0, st, p);
      });
    });
  }));
}

int diral_memory_sample(const DiralMemory* m, const DiralMemorySample* s, void* stream) {
  if (!memory_ok(m) || !s || s->struct_bytes != sizeof(DiralMemorySample)) return DIRAL_ERR_BAD_ARG;
  if (s->step < 1 || s->windows < 1 || (s->idx == nullptr) != (s->env == nullptr)) return DIRAL_ERR_BAD_ARG;
  if (!m->count_dev) {
    const long long len = std::min<long long>(m->count, m->capacity);
    if (len <= s->step) return DIRAL_ERR_BAD_ARG;
    if (!s->idx && (long long)s->windows > (len - s->step) * m->batch) return DIRAL_ERR_BAD_ARG;
  }
  if (!mem_out_ok(m, s->out_dtype)) return DIRAL_ERR_UNSUPPORTED;
  if ((long long)m->num_users * m->state_space > 0x7fffffffLL || ((long long)s->windows + 8) * (s->step + 1LL) > 0x7fffffffLL)
    return DIRAL_ERR_UNSUPPORTED;
  DEVICE_ENTER(m->states);
  // an item: one state of a window; per XCD those of ceil(M / 8) windows
  const MemItems t = mem_items(m, s->out_dtype, ((size_t)s->windows + 7) / 8 * ((size_t)s->step + 1), {s->states_out, s->next_states_out});
  MemSampleParams p{};
  p.states = m->states; p.actions = m->actions; p.rewards = m->rewards;
  p.C = m->capacity; p.B = m->batch; p.N = m->num_users; p.S = m->state_space;
  p.count = (long long)m->count; p.count_dev = (const long long*)m->count_dev;
  p.M = s->windows; p.step = s->step; p.last_only = s->last_only != 0;
  p.idx = s->idx; p.env = s->env; p.seed = s->seed; p.clock = (const long long*)s->clock; p.clock_offset = (long long)s->clock_offset;
  p.states_out = s->states_out; p.next_out = s->next_states_out; p.actions_out = s->actions_out; p.rewards_out = s->rewards_out;
  p.idx_out = s->idx_out; p.env_out = s->env_out; p.bad = s->bad_samples;
  p.vst = t.vst; p.ushift = t.ushift;
  return hip_status(by_ring_out_vec(m, s->out_dtype, t.vec, [&](auto ring, auto out, auto v) {
    return launch_k<memory_sample_kernel<decltype(ring), decltype(out), decltype(v)::value>>(t.grid, dim3(kMemBlock), 0, (hipStream_t)stream, p);
  }));
}

int diral_memory_history(const DiralMemory* m, int32_t step, int32_t out_dtype, void* out, int32_t* bad, void* stream) {
  if (!memory_ok(m) || step < 1 || !out) return DIRAL_ERR_BAD_ARG;
  if (!m->count_dev && (long long)step > std::min<long long>(m->count, m->capacity) + 1) return DIRAL_ERR_BAD_ARG;
  if (!mem_out_ok(m, out_dtype)) return DIRAL_ERR_UNSUPPORTED;
  if ((long long)m->num_users * m->state_space > 0x7fffffffLL || ((long long)m->batch + 8) * step > 0x7fffffffLL)
    return DIRAL_ERR_UNSUPPORTED;
  DEVICE_ENTER(m->states);
  // an item: one state of an env's window; per XCD those of ceil(B / 8) envs
  const MemItems t = mem_items(m, out_dtype, ((size_t)m->batch + 7) / 8 * (size_t)step, {out});
  MemHistoryParams p{};
  p.states = m->states; p.C = m->capacity; p.B = m->batch; p.N = m->num_users; p.S = m->state_space;
  p.count = (long long)m->count; p.count_dev = (const long long*)m->count_dev;
  p.step = step; p.out = out; p.bad = bad;
  p.vst = t.vst; p.ushift = t.ushift;
  return hip_status(by_ring_out_vec(m, out_dtype, t.vec, [&](auto ring, auto o, auto v) {
    return launch_k<memory_history_kernel<decltype(ring), decltype(o), decltype(v)::value>>(t.grid, dim3(kMemBlock), 0, (hipStream_t)stream, p);
  }));
}

int diral_td_head(int32_t rows, int32_t num_actions, const void* q, const void* q_next_target, const void* q_next_eval,
                  int32_t q_dtype, const int32_t* actions, const void* rewards, int32_t rewards_dtype, double gamma,
                  int32_t hysteretic, float* targets_out, float* td_out, int32_t* next_action_out, void* grad_q_out,
                  float* loss_out, int32_t* bad_rows, void* stream) {
  if (!q_next_target || !actions || !rewards || rows < 1 || num_actions < 1) return DIRAL_ERR_BAD_ARG;
  if (q_dtype < DIRAL_F32 || q_dtype > DIRAL_BF16 || !f32_or_f64(rewards_dtype)) return DIRAL_ERR_BAD_ARG;
  if (!std::isfinite(gamma)) return DIRAL_ERR_BAD_ARG;
  if (!q && (td_out || grad_q_out || loss_out)) return DIRAL_ERR_BAD_ARG;
  if (loss_out && !td_out) return DIRAL_ERR_BAD_ARG;
  if (num_actions > kTdMaxA || rows > kTdMaxRows || !f32_f16_or_bf16(q_dtype)) return DIRAL_ERR_UNSUPPORTED;
  DEVICE_ENTER(q_next_target);
  const int A = num_actions;
  const RowLaunch rl = row_launch(rows, A, kTdBlock);
  TdParams p{};
  p.q = q; p.qn_target = q_next_target; p.qn_eval = q_next_eval; p.actions = actions; p.rewards = rewards;
  p.rows = rows; p.A = A; p.gshift = rl.gshift;
  p.gamma = (float)gamma; p.rows_f = (float)rows; p.hysteretic = hysteretic != 0;
  p.targets_out = targets_out; p.td_out = td_out; p.next_action_out = next_action_out; p.grad_q_out = grad_q_out;
  p.bad_rows = bad_rows;
  const hipStream_t st = (hipStream_t)stream;
  auto launch = [&](auto qt, auto rt) {
    using QT = decltype(qt);
    using RT = decltype(rt);
    if (A > 64) return launch_k<td_head_wide_kernel<QT, RT>>(rl.grid, rl.block, 0, st, p);
    return launch_k<td_head_kernel<QT, RT>>(rl.grid, rl.block, 0, st, p);
  };
  const hipError_t head = by_dtype(rewards_dtype, [&](auto rt) {
    return q_dtype == DIRAL_F32 ? launch(float{}, rt) : q_dtype == DIRAL_F16 ? launch(_Float16{}, rt) : launch(bf16_bits{}, rt);
  });
  if (head != hipSuccess || !loss_out) return hip_status(head);
  return hip_status(launch_k<td_loss_kernel>(dim3(1), dim3(kTdBlock), 0, st, (const float*)td_out, (int)rows, loss_out));
}

int diral_qnet_forward(int32_t rows, int32_t num_hidden, const int32_t* widths, const void* x, int32_t x_dtype,
                       int64_t x_row_stride, const float* params, int64_t params_len, int32_t norm, double ln_eps,
                       float* q_out, void* stream) {
  if (!widths || !x || !params || !q_out || rows < 1 || num_hidden < 0) return DIRAL_ERR_BAD_ARG;
  if (x_dtype < DIRAL_F32 || x_dtype > DIRAL_BF16 || !std::isfinite(ln_eps) || ln_eps < 0.0) return DIRAL_ERR_BAD_ARG;
  if (num_hidden > kQnetMaxHidden || !f32_f16_or_bf16(x_dtype)) return DIRAL_ERR_UNSUPPORTED;
  for (int i = 0; i < num_hidden + 2; ++i)
    if (widths[i] < 1) return DIRAL_ERR_BAD_ARG;
  for (int i = 0; i < num_hidden + 2; ++i)
    if (widths[i] > (i ? kQnetMaxWidth : kQnetMaxIn)) return DIRAL_ERR_UNSUPPORTED;
  QnetParams p{};
  p.x = x; p.x_stride = x_row_stride; p.x_dtype = x_dtype; p.params = params; p.q = q_out;
  p.rows = rows; p.L = num_hidden; p.norm = norm != 0; p.eps = (float)ln_eps;
  for (int i = 0; i < num_hidden + 2; ++i) p.width[i] = widths[i];
  if (x_row_stride < widths[0] || params_len != qnet_params_walk(p.width, num_hidden, p.off)) return DIRAL_ERR_BAD_ARG;
  DEVICE_ENTER(x);
  return hip_status(launch_qnet(p, (hipStream_t)stream));
}

}  // extern "C"
