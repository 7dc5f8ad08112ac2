// agent_host.hpp - the two host functions of diral_agent.hip that diral_env.hip calls besides the C symbol
// diral_driver_shape: neither is part of the library's surface.
#pragma once
#include "common.hpp"

namespace diral {

// a DiralMemory every memory entry point takes (diral_memory_*; the memory block of a rollout / prefill)
bool memory_ok(const DiralMemory* m);

// diral_sps_step_chobs with the seed clock of diral_sps_step_chobs_clocked as one more argument (null: none): the body of
// both, argument checks included, and the last of the three launches of an unfused closed-loop slot (diral_env_step_policy)
int sps_step_chobs_with_clock(int agents, int num_channels, const void* chobs, int chobs_dtype, const int32_t* actions,
                              int32_t* prev_action, int32_t* counter, double rssi_threshold, double inc_db,
                              double keep_prob, const int32_t* draw_counter, const double* draw_keep,
                              const int32_t* draw_choice, uint64_t seed, const long long* clock, int32_t* actions_out,
                              void* stream);

}  // namespace diral
