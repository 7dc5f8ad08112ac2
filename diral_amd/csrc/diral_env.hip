// diral_env.hip - C-ABI implementation of include/diral_env.h for gfx950: the env handle and every diral_env_* call.
// (The entry points that take no handle - diral_sps_*, diral_policy_select, diral_memory_*, ... - are diral_agent.hip's.)
// Host side: config validation, HBM allocation, kernel launches.  No torch
// types anywhere; every data pointer in the ABI is a device pointer.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

#include "agent_host.hpp"
#include "aux_kernels.hpp"
#include "common.hpp"
#include "copy_envs_kernel.hpp"
#include "host_util.hpp"
#include "launch.hpp"
#include "observe_kernel.hpp"
#include "piggyback_kernel.hpp"
#include "posdist_kernel.hpp"
#include "reset_envs_kernel.hpp"
#include "step_params.hpp"

using namespace diral;

// One device allocation of a handle (`own`, below): what diral_env_destroy frees, diral_env_hbm_bytes sums and
// diral_env_reset fills again.
struct DevBuf {
  void* p;
  size_t bytes;         // allocated and filled at create, slack included
  size_t reset_bytes;   // what diral_env_reset fills again (never the slack); 0 = reset leaves the buffer alone
  int fill;             // the fill byte; kNoFill = left as allocated (written before its first read)
};
constexpr int kNoFill = -1;
constexpr bool kOnReset = true;

// The test hooks of diral_env_create (include/diral_env.h lists them): read from the process environment ONCE per
// handle (read_hooks), never on the step path.
struct Hooks {
  int table_form = 0;            // DIRAL_TABLE_FORM=packed (+1) | plane (-1): the table form for N > 64 (use_packed_table)
  bool no_fast64 = false;        // DIRAL_NO_FAST64: the general kernel also for N <= 64
  bool no_wide = false;          // DIRAL_NO_WIDE: ... and for N > 64
  bool slow_first = true;        // DIRAL_NO_SLOW_FIRST=1 clears it: blocks = envs in order (A/B timing, tests)
  bool wide_slow_first = false;  // DIRAL_WIDE_SLOW_FIRST=1: step_wide's packed form at N <= 128 dispatches its slow envs first (round 5's default)
  int f32_margin = -1;           // DIRAL_F32_MARGIN=<n> (N <= 64): 0 = no float32 screening of the bin, n > 0 = a band of at
                                 //   least n / 65536 bin widths (tests: a wide band sends many entries to float64); -1 = the bound
};

struct DiralEnv {
  DiralCfg cfg;
  Hooks hooks;
  std::vector<DevBuf> bufs;   // every device buffer of the handle but `trace` and `dbg`
  int B = 0, N = 0, A = 0, K = 0, S = 0, NV = 0, NR = 0, vpl = 1;
  int device = 0;
  StepParams base;       // everything that does not change per call
  RichParams rich;       // section offsets etc. of the RICH output tail (rich_out.hpp)
  uint32_t lds_bytes = 0;
  int64_t env_offset = 0;  // global index of env 0 (DIRAL_OPT_ENV_OFFSET): device RNG draws are indexed globally
  int kernel_path = DIRAL_PATH_AUTO;   // DIRAL_OPT_KERNEL_PATH
  bool subwave_slots = false;          // DIRAL_OPT_SUBWAVE_SLOTS (only while kernel_path == DIRAL_PATH_SUBWAVE)
  int last_kernel = -1;    // DIRAL_KERNEL_* of the last step / observe launch
  double* pos_x = nullptr;
  double* pos_y = nullptr;
  double* vel = nullptr;
  uint32_t* tkey = nullptr;
  double* tx = nullptr;
  // the xpos ring of the N <= 64 kernel (aux_kernels.hpp): while it is in use the per-entry plane `tx` is only
  // kept for entries older than the ring reaches; `plane_valid` / `ring_valid` say which of the two is complete
  double* ring = nullptr;
  bool plane_valid = true, ring_valid = false;
  // the packed table of step_fast64 (N <= 64; step_fast64.hpp): thermometer codes of the entries' lags and their ages,
  // four per word, the subjects' own sequence numbers, the old-quad flags.  It travels with the ring: `ring_valid`
  // = ring AND packed words are current; `plane_valid` = the planes tkey / tx are complete and current
  uint32_t* tcode = nullptr;
  uint32_t* tage = nullptr;
  uint32_t* tseq = nullptr;
  uint32_t* told = nullptr;
  // slow envs first (step_params.hpp FastParams::slow_*): three rotating sets of [count (16 words) | list | flag per env]
  uint32_t* slow = nullptr;
  uint64_t slow_launches = 0;   // launches that rotated the sets
  bool capture_rotates = false; // diral_env_set_capture_rotation: captured launches rotate the sets too (graphs of 3 k launches)
  int32_t* la = nullptr;
  int32_t* pf = nullptr;
  double* metrics = nullptr;
  uint32_t* err = nullptr;
  double* edges = nullptr;
  double* edges1 = nullptr;    // np.linspace(-1, 1, K+1) for the type-1 histogram
  double* inv_tab = nullptr;   // [256] 1.0 / n (n = 0: 0): f32 histogram output, csrc/step_fast64.hpp
  double* trace = nullptr;    // handle-owned copy of the replay trace
  int trace_len = 0, trace_per_env = 0;
  bool flat_y = true;      // every pos_y == 0 (random topologies, network.py:104): |dx| distance path
  uint32_t* yflag = nullptr;
  // State.piggybacking (piggyback_kernel.hpp): TestEnv.prev_obs, and this slot's plain observation / closest transmitters
  int off_chobs_pb = -1;       // column of the A * A section in a state row (the kernels are handed off_chobs = -1)
  double* prev_obs = nullptr;
  double* obs_new = nullptr;
  int32_t* txid = nullptr;
  // num_users > 256 / num_channels > 256 / num_bins > 64 (step_large.hpp): no one-workgroup kernel holds such an env
  bool large = false;
  LargeScratch lg = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  unsigned long long* dbg = nullptr;   // DIRAL_TIMING builds: [B][waves][8] timestamps
  bool capture_violation = false;   // a ring <-> plane switch was asked for inside a stream capture
  std::string last_hip_error;
};

namespace {

bool has(const DiralCfg* c, uint32_t f) { return (c->flags & f) != 0; }

int note_hip(DiralEnv* e, hipError_t st, const char* what) {
  if (st == hipSuccess) return DIRAL_OK;
  if (e && e->capture_violation) {
    e->capture_violation = false;
    e->last_hip_error = std::string(what) + ": the call needs a ring <-> plane conversion launch, which cannot be part of a stream capture";
    return DIRAL_ERR_CAPTURE;
  }
  if (e) e->last_hip_error = std::string(what) + ": " + hipGetErrorString(st);
  return DIRAL_ERR_HIP;
}

#define HIP_TRY(env, call)                                   \
  do {                                                       \
    hipError_t st__ = (call);                                \
    if (st__ != hipSuccess) return note_hip(env, st__, #call); \
  } while (0)

// np.linspace(start, stop, num), endpoint=True (numpy/_core/function_base.py):
// y[i] = i*step + start with both roundings, last = stop.
void np_linspace(double start, double stop, int num, std::vector<double>& out) {
  out.assign(num, 0.0);
  const int div = num - 1;
  const double delta = stop - start;
  if (div > 0) {
    const double step = delta / (double)div;
    for (int i = 0; i < num; ++i) {
      volatile double y = (double)i;
      if (step == 0.0) { y = y / (double)div; y = y * delta; }
      else y = y * step;
      volatile double r = y + start;
      out[i] = r;
    }
    out[num - 1] = stop;
  } else if (num == 1) {
    out[0] = start;
  }
}

struct Offsets { int act, chobs, posdist, hist, rew, idx, pos, vel, fp, S; };

// section order of TestEnv.obtain_state (test_env.py:527-583)
Offsets state_offsets(const DiralCfg* c) {
  Offsets o{-1, -1, -1, -1, -1, -1, -1, -1, -1, 0};
  int p = 0;
  if (has(c, DIRAL_F_ADD_ACTION)) { o.act = p; p += has(c, DIRAL_F_ACTION_REAL) ? 1 : c->num_channels; }
  // (State.piggybacking: `obs[user_i]` is piggy_obs, A * A values - test_env.py:71-72, 263-264, 539-541)
  if (has(c, DIRAL_F_ADD_CHANNEL_OBS)) { o.chobs = p; p += has(c, DIRAL_F_PIGGYBACKING) ? c->num_channels * c->num_channels : c->num_channels; }
  if (has(c, DIRAL_F_ADD_POSDIST)) { o.posdist = p; p += c->num_users - 1; }
  if (has(c, DIRAL_F_ADD_POSDIST_PIGGY)) { o.hist = p; p += c->num_bins; }
  if (has(c, DIRAL_F_ADD_REWARD)) { o.rew = p; p += 1; }
  if (has(c, DIRAL_F_ADD_INDEX)) { o.idx = p; p += 1; }
  if (has(c, DIRAL_F_ADD_POSITION)) { o.pos = p; p += 2; }
  if (has(c, DIRAL_F_ADD_VELOCITY)) { o.vel = p; p += 1; }
  if (has(c, DIRAL_F_FINGERPRINT)) { o.fp = p; p += 2; }
  o.S = p;
  return o;
}

int vpl_for(int N) { return N <= 64 ? 1 : (N <= 128 ? 2 : 4); }

// sizes no one-workgroup kernel holds: the three launches of step_large.hpp
bool is_large_cfg(const DiralCfg* c) {
  if (c->num_users > DIRAL_SMALL_MAX_USERS || c->num_channels > DIRAL_SMALL_MAX_CHANNELS ||
      (has(c, DIRAL_F_ADD_POSDIST_PIGGY) && c->num_bins > DIRAL_SMALL_MAX_BINS))
    return true;
  // ... and the combinations below those sizes whose env does not fit the general kernel's workgroup (e.g. 200 vehicles,
  // 200 resources, 64 bins): every handle can fall back on that kernel, so they run here as well
  const int vpl = vpl_for(c->num_users);
  return lds_layout(64 * vpl, c->num_channels, c->num_bins > 0 ? c->num_bins : 1, vpl, 4 * vpl).total > 160u * 1024u;
}
bool runs_large(const DiralEnv* e) { return e->large || e->kernel_path == DIRAL_PATH_LARGE; }

// The sizes the specialised kernels take, step_fast64 and step_wide: such a handle keeps an xpos ring (diral_env_create),
// and only such a handle is ever planned onto them (plan_step).
bool fits_fast64(const DiralEnv* e) { return !e->large && e->vpl == 1 && e->NV == 64 && e->A <= kFastMaxA; }
bool fits_wide(const DiralEnv* e) { return !e->large && e->vpl > 1 && e->A <= kWideMaxA; }

Hooks read_hooks() {
  Hooks h;
  if (const char* f = std::getenv("DIRAL_TABLE_FORM")) h.table_form = std::strcmp(f, "packed") == 0 ? 1 : (std::strcmp(f, "plane") == 0 ? -1 : 0);
  h.no_fast64 = std::getenv("DIRAL_NO_FAST64") != nullptr;
  h.no_wide = std::getenv("DIRAL_NO_WIDE") != nullptr;
  if (const char* off = std::getenv("DIRAL_NO_SLOW_FIRST")) h.slow_first = off[0] != '1';
  if (const char* ws = std::getenv("DIRAL_WIDE_SLOW_FIRST")) h.wide_slow_first = ws[0] == '1';
  if (const char* fm = std::getenv("DIRAL_F32_MARGIN")) h.f32_margin = std::max(0, std::atoi(fm));
  return h;
}

// The table form of a handle (fixed at create): packed thermometer codes + ages + own sequence numbers, or the (seq, age)
// plane `tkey` of round 2.  N <= 64: always packed (step_fast64 has no other form).  64 < N <= 256 (step_wide): packed
// where the vehicles are dense enough for tables to stay fresh - on average at least kPackedMinNeighbours vehicles within
// communication range (N * 2 Rc / L; BASELINE configs[2]: 32, configs[4]: 16) -, else the plane: on a sparse highway most
// entries lag their subject by more than the 7 stamps the codes carry, and every pass of the packed form would detour
// through the planes (N > 128: measured + 60 % at 2.4 neighbours, + 58 % at 10.7).  At configs[4]'s density one env in
// ten has broken into clusters and runs nearly all its passes through the planes at three times the price of a plane-form
// pass, the other nine run coded passes at a third of it: 1.11 -> 1.02-1.04 ms with those envs dispatched first (step_wide.hpp).
// DIRAL_TABLE_FORM = packed | plane in the environment overrides the choice for N > 64 (tests run both forms on both
// kinds of topology).
constexpr double kPackedMinNeighbours = 20.0;
constexpr double kPackedMinNeighbours2 = 15.0;           // 64 < N <= 128
bool use_packed_table(const DiralEnv* e) {
  if (e->vpl == 1) return true;
  if (e->hooks.table_form != 0) return e->hooks.table_form > 0;
  const double neigh = e->N * 2.0 * e->cfg.communication_range / e->cfg.highway_length;
  return neigh >= (e->vpl == 2 ? kPackedMinNeighbours2 : kPackedMinNeighbours);
}

// State flags that only add OUTPUT columns to the state vector (test_env.py:527-583): served
// by the RICH instantiations of the specialised kernels (rich_out.hpp)
constexpr uint32_t kRichFlags = DIRAL_F_ACTION_REAL | DIRAL_F_ADD_CHANNEL_OBS | DIRAL_F_ADD_REWARD | DIRAL_F_ADD_INDEX |
                                DIRAL_F_ADD_VELOCITY | DIRAL_F_ADD_POSITION | DIRAL_F_FINGERPRINT | DIRAL_F_PIGGYBACKING;

// Configurations the specialised kernels (step_fast64 / step_wide) serve: every step kind on a mobile
// topology with piggybacked neighbour tables, any combination of outputs and State flags, proportional
// fairness.  The type-2 piggybacked histogram is part of the kernels; the secondary observation modes
// (a15/a16: sorted true distances, type-1 weighted histogram) are columns posdist_kernel fills right
// after the step, so the step itself runs here all the same (RICH instantiation, histogram columns off
// unless type 2).  A State block without piggybacked tables (test_env.py:138, 231-238: no gossip at all), PRR
// tracking in my_step and static topologies are run-time switches of the EXTRA instantiations.  What is left
// for the general kernel: A > 64, and vehicles off the common lane at N > 64 (nothing the reference draws).
bool is_specialised_cfg(const StepParams& p) {
  const uint32_t want = 0u;
  const uint32_t ignore = DIRAL_F_MOBILITY | DIRAL_F_ADD_POSDIST_PIGGY | DIRAL_F_TOY_WEIGHTS | DIRAL_F_MOBILITY_VARY | DIRAL_F_DESIGN_TOPOLOGY | DIRAL_F_TRACK_ARRIVAL |
                          DIRAL_F_TRACK_PRR | DIRAL_F_ADD_ACTION | DIRAL_F_PROPORTIONAL_FAIR | DIRAL_F_ADD_POSDIST | kRichFlags;
  return (p.flags & ~ignore) == want &&
         (p.mode == DIRAL_STEP_MY_STEP || p.mode == DIRAL_STEP_MY_STEP_CH || p.mode == DIRAL_STEP_DESIGN);
}
// the state vector carries the type-2 piggybacked histogram
bool has_hist2(const StepParams& p) { return (p.flags & DIRAL_F_ADD_POSDIST_PIGGY) && p.posdist_type == 2; }
// the toy YAML's State flags: a state row is [action one-hot | type-2 histogram] (RichParams::plain_state)
bool is_plain_state(const StepParams& p) {
  return (p.flags & (kRichFlags | DIRAL_F_ADD_POSDIST)) == 0 && has_hist2(p) && (p.flags & DIRAL_F_ADD_ACTION);
}
// ... of which the PLAIN instantiations serve that state vector as the only observation output, without
// proportional fairness (the metric's configuration)
bool is_plain_cfg(const StepParams& p) {
  return is_plain_state(p) && !(p.flags & DIRAL_F_PROPORTIONAL_FAIR) && p.state_out != nullptr && p.chobs_out == nullptr;
}

// A switch between the xpos ring and the per-entry plane (ring_rebuild / ring_materialize) is a launch that
// depends on HOST-side validity flags: recorded into a hipGraph it would replay against tables it no longer
// describes.  Such a call fails with DIRAL_ERR_CAPTURE instead (do the first step of a new kernel path, or the
// export / observe, outside the capture).
bool stream_is_capturing(hipStream_t s) {
  hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing(s, &st) != hipSuccess) { (void)hipGetLastError(); return false; }
  return st != hipStreamCaptureStatusNone;
}

// Every hipMalloc of a handle: `bytes` + `slack` are allocated, recorded (DevBuf) and filled with `fill`; with `on_reset`
// diral_env_reset fills the `bytes` again, on the caller's stream.  The slack is what a kernel reads past the end
// UNMASKED: it is filled here once and nobody writes it, so each size is stated at its one call of `own` and nowhere else.
template <typename T>
hipError_t own(DiralEnv* e, T*& p, size_t bytes, size_t slack = 0, bool on_reset = false, int fill = 0) {
  const hipError_t st = hipMalloc((void**)&p, bytes + slack);
  if (st != hipSuccess) return st;
  e->bufs.push_back({p, bytes + slack, on_reset ? bytes : 0, fill});
  return fill == kNoFill ? hipSuccess : hipMemset(p, fill, bytes + slack);
}
const DevBuf& buf_of(const DiralEnv* e, const void* p) {
  for (const DevBuf& b : e->bufs) if (b.p == p) return b;
  std::abort();   // (not a buffer of `own`: a bug in this file)
}

// every consumer of the per-entry xpos plane other than step_fast64 goes through here first
hipError_t ensure_plane(DiralEnv* e, hipStream_t s) {
  if (e->plane_valid || !e->ring) { e->plane_valid = true; return hipSuccess; }
  if (stream_is_capturing(s)) { e->capture_violation = true; return hipErrorStreamCaptureUnsupported; }
  e->plane_valid = true;
  if (e->tcode)
    return launch_1d<unpack_codes_kernel>((size_t)e->B * (e->NR / 4) * e->NV, s, e->B, e->N, e->NV, e->NR, e->tcode, e->tage,
                                          e->tseq, e->ring, e->tkey, e->tx);
  return launch_1d<ring_materialize_kernel>((size_t)e->B * e->N * e->N, s, e->B, e->N, e->NV, e->NR, e->tkey, e->ring, e->tx);
}
hipError_t ensure_ring(DiralEnv* e, hipStream_t s) {
  if (e->ring_valid) return hipSuccess;
  if (stream_is_capturing(s)) { e->capture_violation = true; return hipErrorStreamCaptureUnsupported; }
  hipError_t st = launch_1d<ring_rebuild_kernel>((size_t)e->B * e->N * e->N, s, e->B, e->N, e->NV, e->NR, e->tkey, e->tx, e->ring);
  if (st == hipSuccess && e->tcode) {
    st = hipMemsetAsync(e->told, 0, buf_of(e, e->told).reset_bytes, s);
    if (st == hipSuccess)
      st = launch_1d<pack_codes_kernel>((size_t)e->B * (e->NR / 4) * e->NV, s, e->B, e->N, e->NV, e->NR, e->tkey, e->tcode, e->tage,
                                        e->tseq, e->told);
  }
  e->ring_valid = st == hipSuccess;
  return st;
}

// What diral_env_copy_envs moves: the per-env slabs of every buffer that is STATE - the positions and velocities, and
// whatever diral_env_reset refills (tables in every stored form, arrival stamps, pf counters, metric sums, prev_obs) except
// the slow-first sets, a scheduling hint with a list / flag consistency of its own that no result depends on
// (step_params.hpp).  Taken from the records of `own`, in the order of its calls: two handles of one config and one table
// form give the same list.  false: more than kCopyMaxSlabs such buffers (a bug in this file).
bool copy_slabs(const DiralEnv* e, std::vector<std::pair<char*, uint32_t>>& out) {
  out.clear();
  for (const DevBuf& b : e->bufs) {
    const bool pos = b.p == e->pos_x || b.p == e->pos_y || b.p == e->vel;
    if (!pos && (!b.reset_bytes || b.p == e->slow)) continue;
    out.push_back({(char*)b.p, (uint32_t)((pos ? b.bytes : b.reset_bytes) / (size_t)e->B)});
  }
  return out.size() <= (size_t)kCopyMaxSlabs;
}

// The RICH output-tail description of one call: section layout of the state vector, and which of its columns
// belong to the observation launch that follows (posdist_kernel.hpp) and are left alone here.
RichParams rich_for(const DiralEnv* e, const StepParams& p) {
  RichParams r = e->rich;
  r.chobs_out = nullptr; r.episode = p.episode; r.eps = p.eps;
  // (the row's layout, whatever else the call writes: is_plain_cfg without its conditions on outputs and fairness)
  r.plain_state = is_plain_state(p) ? 1 : 0;
  if (!has_hist2(p)) r.off_hist = -1;                         // (type 1: posdist_kernel writes those columns)
  // the sorted-distance columns and the type-1 histogram are posdist_kernel.hpp's, every one of them (and
  // neighbours in the state vector, state_offsets): not written here at all
  const bool skip_full = (p.flags & DIRAL_F_ADD_POSDIST) && p.state_out && p.off_posdist >= 0 && p.N > 1;
  const bool skip_t1 = (p.flags & DIRAL_F_ADD_POSDIST_PIGGY) && p.posdist_type == 1 && p.state_out && p.off_hist >= 0;
  // State.piggybacking: the A * A channel-observation section is piggy_emit_kernel's (piggyback_kernel.hpp); it sits
  // right in front of the other two (state_offsets), so the skipped columns stay one range
  const bool skip_pb = (e->cfg.flags & DIRAL_F_PIGGYBACKING) && p.state_out && e->off_chobs_pb >= 0;
  r.off_skip = skip_pb ? e->off_chobs_pb : (skip_full ? p.off_posdist : (skip_t1 ? p.off_hist : 0));
  r.len_skip = (skip_pb ? p.A * p.A : 0) + (skip_full ? p.N - 1 : 0) + (skip_t1 ? p.K : 0);
  r.pf = nullptr;
  return r;
}

// TestEnv.obtain_state as its own launch (observe_kernel.hpp): reads the tables as they are - young entries'
// xpos from the ring when it is valid, so no plane materialisation is needed - and changes nothing
hipError_t launch_observe_any(DiralEnv* e, const StepParams& p, hipStream_t s) {
  const bool use_ring = e->ring != nullptr && e->ring_valid;
  if (!use_ring) {
    const hipError_t st = ensure_plane(e, s);
    if (st != hipSuccess) return st;
  }
  ObserveParams o;
  o.N = p.N; o.A = p.A; o.K = p.K; o.NV = p.NV; o.NR = p.NR; o.flags = p.flags; o.age_limit = p.age_limit;
  o.want_hist = (has_hist2(p) && p.off_hist >= 0) ? 1 : 0;
  o.L = p.L; o.Rb = p.Rb; o.inv_w = p.hist_inv_width;
  o.actions = p.actions; o.chobs_in = p.chobs_in; o.rew_in = p.rew_in;
  o.pos_x = p.pos_x; o.pos_y = p.pos_y; o.vel = p.vel; o.tkey = p.tkey; o.tx = p.tx;
  o.ring = use_ring ? e->ring : nullptr;
  const bool packed = use_ring && e->tcode != nullptr;           // codes, ages, own sequence numbers
  o.tcode = packed ? e->tcode : nullptr; o.tage = packed ? e->tage : nullptr; o.tseq = packed ? e->tseq : nullptr;
  o.edges = p.edges; o.inv_tab = e->inv_tab; o.err = p.err; o.state_out = p.state_out;
  const RichParams r = rich_for(e, p);
  e->last_kernel = DIRAL_KERNEL_OBSERVE | (use_ring ? DIRAL_KERNEL_RING : 0);
  return launch_observe(o, r, e->flat_y, p.out_f64 != 0, p.B, s);
}

// after an import: the ring must answer every young entry with that entry's own xpos (aux_kernels.hpp)
hipError_t verify_ring(DiralEnv* e, hipStream_t s) {
  return launch_1d<ring_verify_kernel>((size_t)e->B * e->N * e->N, s, e->B, e->N, e->NV, e->NR, e->tkey, e->tx, e->ring, e->err);
}

// scratch of the three-launch form (step_large.hpp), and its kernels' LDS attributes: at create for a large handle,
// at diral_env_set_option(DIRAL_OPT_KERNEL_PATH, DIRAL_PATH_LARGE) for any other
hipError_t alloc_large_scratch(DiralEnv* e) {
  if (e->lg.src) return hipSuccess;
  const size_t bn = (size_t)e->B * e->N, ba = (size_t)e->B * e->A;
  hipError_t st = own(e, e->lg.src, ba * e->N * 2);
  if (st == hipSuccess) st = own(e, e->lg.cnt, ba * 4);
  if (st == hipSuccess) st = own(e, e->lg.alist, ba * 2);
  if (st == hipSuccess) st = own(e, e->lg.nact, (size_t)e->B * 4);
  if (st == hipSuccess) st = own(e, e->lg.qflag, (size_t)e->B * ((e->N + 1) / 2) + 16);
  if (st == hipSuccess) st = own(e, e->lg.px0, bn * 8);
  if (st == hipSuccess) st = own(e, e->lg.rew, bn * 8);
  if (st == hipSuccess) st = own(e, e->lg.rtx, bn * 8);
  return st == hipSuccess ? set_attr_large(e->N, e->A, e->K) : st;
}

size_t slow_set_words(const DiralEnv* e) { return 16 + (size_t)fast_slow_max(e->B) + (size_t)e->B; }

// A slot call (diral_env_step_policy - the closed loop -, diral_env_prefill, diral_env_rollout), described once: what the
// slot loops are handed, zero until the call or a block sets it (`prefill` / `rollout`: which call; ia_on / rp_on / mem_on:
// which blocks), and whether the closed loop got a channel-observation buffer (it can run a slot as three launches then)
struct SlotRequest { PolParams q{}; bool chobs = false; };
// a state vector with a secondary observation mode (a15 / a16): launches of their own behind ONE vector (posdist_kernel.hpp)
bool secondary_obs(const StepParams& p) {
  return p.state_out && ((p.flags & DIRAL_F_ADD_POSDIST) || ((p.flags & DIRAL_F_ADD_POSDIST_PIGGY) && p.posdist_type == 1));
}

// What one step call launches, or the status that refuses it: decided by plan_step - which refuses, and has choose_launch
// pick the kernel - without side effects or HIP calls, from the handle, the call's parameters and its slot request (null: diral_env_step / diral_env_observe) -
// for the launch itself (launch_step_any) and for everyone who must know the outcome before anything is launched.
enum class StepLaunch { Large, General, Subwave, SubwaveSlots, Fast64, Wide, Fast64Policy, Fast64Slots, WideSlots };
struct StepPlan {
  int status;                  // DIRAL_OK, or why the slot call is refused: nothing is launched then
  StepLaunch launch;
  bool use_fast64, use_wide;   // the kernel family of the five specialised launches
  bool use_ring;               // xpos ring (step_fast64.hpp): the kernel keeps the plane only for entries older than the ring reaches
  bool slow_sets;              // the launch reads the slow-env sets (and rotates them: rotate_slow_sets); its grid has their blocks
  bool fused;                  // the policy request is part of the launch (Fast64Policy, Fast64Slots, WideSlots, SubwaveSlots)
  // the run-time switches of the EXTRA instantiations, host-folded (FastParams::design ... nomove)
  bool design, prr, notab, nomove;
  int32_t* la;
  const double* trace;
  bool general_fast;           // StepLaunch::General: the FAST instantiation of the general kernel
  KernelSel k;
  int last_kernel;             // DIRAL_KERNEL_*
};
// the kernel family and instantiation of a call that plan_step has not refused by then
StepPlan choose_launch(const DiralEnv* e, const StepParams& p, const PolParams* pol) {
  StepPlan d = {};
  if (runs_large(e)) {
    // (and diral_env_observe: the search kernel's observe mode + the histogram launch)
    d.launch = StepLaunch::Large; d.last_kernel = DIRAL_KERNEL_LARGE;
    return d;
  }
  if (e->kernel_path == DIRAL_PATH_SUBWAVE && p.mode != kModeObserve) {
    // toy-size envs, 4 or 8 lanes each (step_subwave.hpp): every step call of a pinned handle, on the planes; never `fused`
    d.launch = StepLaunch::Subwave; d.last_kernel = DIRAL_KERNEL_SUBWAVE;
    // ... unless the handle opted in to the slot loop (DIRAL_OPT_SUBWAVE_SLOTS, step_subwave_slots.hpp): an open-loop rollout of
    // any K >= 1 and the random prefill, without the information-age and replay / position-log blocks; the prefill refuses a
    // handle with a trace or arrival stamps, as the fast64 prefill does.  diral_env_step_policy stays where it was: the SPS
    // agents are wave-cooperative code.
    const bool tracking = ((p.flags & DIRAL_F_TRACK_ARRIVAL) && p.la != nullptr) || p.trace != nullptr;
    if (e->subwave_slots && pol && (pol->prefill || pol->rollout) && !pol->ia_on && !pol->rp_on && !(pol->prefill && tracking)) {
      d.launch = StepLaunch::SubwaveSlots; d.fused = true; d.last_kernel = DIRAL_KERNEL_SUBWAVE | DIRAL_KERNEL_POLICY;
    }
    return d;
  }
  // (DIRAL_PATH_GENERAL keeps the general kernel's FAST instantiation: plain_cfg does not ask for the path)
  const bool plain_cfg = is_specialised_cfg(p) && is_plain_cfg(p);
  const bool spec = is_specialised_cfg(p) && e->kernel_path == DIRAL_PATH_AUTO;
  const bool plain = spec && plain_cfg;
  const bool ch = p.mode == DIRAL_STEP_MY_STEP_CH;
  // the wide kernels read the reward column of a RICH state back from rew_out
  const bool wide_rich_ok = plain || !(p.flags & DIRAL_F_ADD_REWARD) || p.state_out == nullptr || p.rew_out != nullptr;
  d.use_fast64 = spec && fits_fast64(e);
  d.use_wide = spec && fits_wide(e) && e->flat_y && wide_rich_ok;
  if (!d.use_fast64 && !d.use_wide) {
    // the generic FAST instantiation of the general kernel: the plain configuration on sizes the
    // specialised kernels do not take (A > 64, vehicles off the y = 0 lane at N > 64): my_step,
    // f32 outputs, no arrival stamps, no trace replay
    d.general_fast = plain_cfg && !p.out_f64 && p.mode == DIRAL_STEP_MY_STEP && !(p.flags & DIRAL_F_TRACK_ARRIVAL) && p.trace == nullptr;
    d.launch = StepLaunch::General; d.last_kernel = DIRAL_KERNEL_GENERAL;
    return d;
  }
  d.use_ring = e->ring != nullptr;
  d.design = p.mode == DIRAL_STEP_DESIGN;
  d.prr = (p.flags & DIRAL_F_TRACK_PRR) && p.mode == DIRAL_STEP_MY_STEP;
  d.notab = !(p.flags & DIRAL_F_ADD_POSDIST_PIGGY);          // no piggybacked tables: test_env.py:138-139, 231-238
  d.nomove = !(p.flags & DIRAL_F_MOBILITY);                  // static (design) topology: network.py:302-305
  d.la = (p.flags & DIRAL_F_TRACK_ARRIVAL) ? p.la : nullptr;
  d.trace = d.nomove ? nullptr : p.trace;
  // (a my_step_ch call that carries the information-age block - diral_env_rollout_ia / diral_env_step_policy_ia - runs its
  // stamps in the slot loop of step_fast64: they do not ask for an EXTRA instantiation there)
  const bool la_in_slots = pol && pol->ia_on && ch;
  const bool switches = (d.la != nullptr && !la_in_slots) || d.trace != nullptr || d.prr || d.notab || d.nomove;
  const bool extra = d.design || switches;
  // the POL instantiation of step_fast64 (policy epilogue inside the launch) takes this call
  const bool pol_ok = d.use_fast64 && e->flat_y && !ch && !extra && p.N >= 8;
  // ... and the K-slot form of it runs this configuration's random prefill (diral_env_prefill: my_step_design's
  // reward is computed in P2 there, so the design switch does not count against it)
  const bool prefill_ok = d.use_fast64 && e->flat_y && d.design && !switches && p.N >= 8;
  // my_step_ch: the K-slot form only (slots > 1 of diral_env_step_policy, and the enable_channel prefill of
  // diral_env_prefill_mode); a one-slot policy call in this mode keeps its three launches
  const bool pol_ch_ok = d.use_fast64 && e->flat_y && ch && !extra && p.N >= 8;
  // step_wide_slots_kernel (k_wide_slots.hip) takes K > 1 slots of diral_env_step_policy at 64 < N <= 256; a one-slot
  // call there keeps its three launches
  const bool wide_kslots_ok = d.use_wide && !ch && !extra;
  d.launch = d.use_wide ? StepLaunch::Wide : StepLaunch::Fast64;
  if (pol && pol->prefill) { if (prefill_ok || pol_ch_ok) d.launch = StepLaunch::Fast64Slots; }
  else if (pol && pol->rollout) {
    // an open-loop rollout (diral_env_rollout): any K >= 1 on the two slot loops - every slot's state vector only where
    // the env stays on the chip (N <= 64)
    if (pol_ok || pol_ch_ok) d.launch = StepLaunch::Fast64Slots;
    else if (wide_kslots_ok && !(pol->rollout & 2)) d.launch = StepLaunch::WideSlots;
  }
  else if (pol && pol->K > 1) { if (pol_ok || pol_ch_ok) d.launch = StepLaunch::Fast64Slots; else if (wide_kslots_ok) d.launch = StepLaunch::WideSlots; }
  else if (pol && pol_ok) d.launch = StepLaunch::Fast64Policy;
  // K slots per launch (DiralSlotPolicy::slots > 1, prefill): blocks = envs in order - over K slots a straggler averages
  // out; the slow-env sets stay as the last one-slot launch left them (complete or empty), unread
  const bool kslots = d.launch == StepLaunch::Fast64Slots || d.launch == StepLaunch::WideSlots;
  d.fused = kslots || d.launch == StepLaunch::Fast64Policy;
  // (step_wide: the packed form at N <= 128 only - its slow envs are 4 x the others; the plane form's are 1.6 x and measured
  // 4 % SLOWER dispatched first, N > 128 packed runs on dense topologies without any: - 0.7 % for the bookkeeping)
  // Round 6: with the far-entry guard (step_wide.hpp `wide_far_guard`) the flagged passes of a highway that broke apart run
  // on the coded path - those envs are no longer 3 x the others, and the slow-first grid (B / 4 more blocks, a flag load per
  // block) now costs more than it orders: C5 0.930 ms with it, 0.875 in batch order (one box, interleaved, profiles/r06).
  // DIRAL_WIDE_SLOW_FIRST=1 at create brings it back (A/B).
  const bool wide_slow = d.use_wide && e->vpl == 2 && e->tcode != nullptr && e->hooks.wide_slow_first;
  d.slow_sets = (d.use_fast64 || wide_slow) && e->slow && e->hooks.slow_first && !kslots;
  KernelSel& k = d.k;
  k.flat = e->flat_y; k.out64 = p.out_f64 != 0; k.full = p.N == 64 * e->vpl; k.ch = ch;
  k.extra = extra;                                            // EXTRA instantiation: the run-time switches compiled in
  k.rich = !plain;
  k.packed = d.use_wide && e->tcode != nullptr;
  // (a fused launch is a RICH instantiation: the channel observation is staged in LDS whether or not it is written out)
  d.last_kernel = (d.use_wide ? DIRAL_KERNEL_WIDE : DIRAL_KERNEL_FAST64) | ((k.rich || d.fused) ? DIRAL_KERNEL_RICH : 0) |
                  ((k.packed || d.use_fast64) ? DIRAL_KERNEL_PACKED : 0) | (k.extra ? DIRAL_KERNEL_EXTRA : 0) |
                  (k.ch ? DIRAL_KERNEL_CH : 0) | (d.use_ring ? DIRAL_KERNEL_RING : 0) | (d.fused ? DIRAL_KERNEL_POLICY : 0);
  return d;
}

// The verdict of a call (DESIGN.md section 6 tabulates it): a slot call is refused here by what the handle is, or by which
// launch choose_launch picks for it.  The first reason below wins - the order is behaviour (tests/test_gpu_slot_refusals.py).
StepPlan plan_step(const DiralEnv* e, const StepParams& p, const SlotRequest* req) {
  if (!req) return choose_launch(e, p, nullptr);
  const PolParams& q = req->q;
  const bool closed = !q.prefill && !q.rollout, ch = p.mode == DIRAL_STEP_MY_STEP_CH, ia = q.ia_on != 0;
  const bool bad_draws = closed && q.K > 1 && (q.draw_counter || q.draw_keep || q.draw_choice);   // (they draw on the device)
  auto refuse = [](int status) { StepPlan d = {}; d.status = status; return d; };
  if (ia && bad_draws) return refuse(DIRAL_ERR_BAD_ARG);
  if (ia && !e->la) return refuse(DIRAL_ERR_BAD_CONFIG);        // (as diral_env_info_age)
  // my_step's only stamp effect is the -1 of network.py:394; there is no fused one-slot my_step_ch launch
  if (ia && (!ch || (closed && q.K <= 1))) return refuse(DIRAL_ERR_UNSUPPORTED);
  if (closed && e->A > kSpsWaveMaxA) return refuse(DIRAL_ERR_UNSUPPORTED);
  // State.piggybacking: the SPS agents sense A values, not A * A, the A * A observation is piggy_emit_kernel's, and the steps
  // are my_step only (diral_env_step): the loop a my_step_design prefill stands for fails there too
  if (e->prev_obs) return refuse(q.prefill && !ch ? DIRAL_ERR_BAD_CONFIG : DIRAL_ERR_UNSUPPORTED);
  if (bad_draws) return refuse(DIRAL_ERR_BAD_ARG);
  if (!closed && secondary_obs(p)) return refuse(DIRAL_ERR_UNSUPPORTED);   // (the closed loop's last state vector gets its launches)
  StepPlan d = choose_launch(e, p, &q);
  const bool fast_slots = d.launch == StepLaunch::Fast64Slots;
  // not fused: one slot of the closed loop runs as three launches around the caller's channel observation (a caller without
  // the buffer can retry with one); a prefill or rollout launches nothing, the caller loops
  if (!d.fused && (!closed || !req->chobs || q.K > 1)) d.status = DIRAL_ERR_UNSUPPORTED;
  // only step_fast64's slot loop keeps the stamps and takes recorded positions (one closed-loop slot: diral_env_set_trace)
  if ((ia && !fast_slots) || (q.rp_on && (!fast_slots || (closed && q.K <= 1)))) d.status = DIRAL_ERR_UNSUPPORTED;
  // the memory block: the two slot loops that keep the env on the chip - the wide one has no states_all
  if (q.mem_on && !fast_slots && d.launch != StepLaunch::SubwaveSlots) d.status = DIRAL_ERR_UNSUPPORTED;
  return d;
}

// float32 screening of the histogram bin (step_fast64.hpp, fast quads), FastParams::f32_m16: everything float32 can lose,
// in bin widths, for positions in [0, L] - the three conversions and the fma at t <= K below - with a factor of two on
// top; as 1 / 65536ths, rounded up, + 1.  0 = no screening: the band would be too wide, or `hook` (DIRAL_F32_MARGIN) is 0;
// a hook > 0 widens the band to at least that.
int f32_margin16(double L, double Rb, int K, int hook) {
  const double w = (Rb - (-Rb)) / (double)K;
  const double xmax = L;
  // (the kernel computes t = fma(float(xpos), float(inv_w 2^16), float((Rb - npx) inv_w 2^16)): the conversion of the
  // stamp and of the factor lose 2 |xpos| 2^-24 / w bin widths, the addend's |Rb - npx| 2^-24 / w <= (xmax + Rb) 2^-24 / w,
  // the fma's own rounding K 2^-24)
  // The margin itself rides in the addend: the kernel forms float((Rb - npx) inv_w 2^16 + m) and
  // the fma yields t + m.  m / 65536 is at most 1 / 4 bin width (the hook stops at 16384), so the addend's conversion loses
  // at most 2^-26 bin widths more and the fma rounds a sum of at most K + 1 / 4: (K + 1 / 2) 2^-24 in all where the term
  // below allows 4 K 2^-24 before its factor of two - for every K >= 1 the larger addend is covered with the bound as it
  // was, and the bands (and the lists derived from them in tests/hist_edge_cases.py) stay what they are.  Truncation: for
  // t >= 0 trunc(t + m) == trunc(t) + m; for t in (-m - 1, 0) the two differ by at most one and both lie in [0, m] - in
  // range and inside the band, left to float64 either way.
  const double lost = 2.0 * (((3.0 * xmax + Rb) * 0x1p-24) / w + 2.0 * (double)K * 0x1p-23);
  const double m = std::ceil(lost * 65536.0) + 1.0;
  const bool on = m <= 64.0 && xmax < 1e6 && hook != 0;
  return on ? std::max((int)m, std::min(hook, 16384)) : 0;
}

// the arguments of a specialised launch, but for the slow-env sets (rotate_slow_sets)
FastParams fast_params(const DiralEnv* e, const StepParams& p, const StepPlan& d) {
  FastParams f;
  f.N = p.N; f.A = p.A; f.K = p.K; f.NR = p.NR; f.NV = p.NV; f.flags = p.flags;
  f.reward_design = p.reward_design; f.age_limit = p.age_limit; f.episode_interval = p.episode_interval;
  f.design = d.design ? 1 : 0;
  f.done_now = (!p.t_dev && (p.t % p.episode_interval) == p.episode_interval - 1) ? 1 : 0;   // main_test.py:226 (with a slot clock: on the device)
  f.prr = d.prr ? 1 : 0;
  f.notab = d.notab ? 1 : 0;
  f.nomove = d.nomove ? 1 : 0;
  f.trace = d.trace;
  f.chobs_mode = (p.chobs_out ? 1 : 0) | ((p.mode == DIRAL_STEP_MY_STEP && p.state_type == 2) ? 2 : 0);
  f.L = p.L; f.Rc = p.Rc; f.Rb = p.Rb; f.inv_w = p.hist_inv_width; f.t = p.t; f.t_dev = p.t_dev;
  f.actions = p.actions; f.pos_x = p.pos_x; f.pos_y = p.pos_y; f.vel = p.vel; f.tkey = p.tkey; f.tx = p.tx;
  f.metrics = p.metrics; f.err = p.err; f.edges = p.edges; f.inv_tab = e->inv_tab;
  f.ring = d.use_ring ? e->ring : nullptr;
  f.tcode = e->tcode; f.tage = e->tage; f.tseq = e->tseq; f.told = e->told;
  f.la = d.la;
  f.trace_len = p.trace_len; f.trace_per_env = p.trace_per_env;
  f.state_out = p.state_out; f.rew_out = p.rew_out;
  f.done_out = p.done_out; f.dbg = p.dbg;
  f.B = p.B;
  f.f32_m16 = d.use_fast64 ? f32_margin16(p.L, p.Rb, p.K, e->hooks.f32_margin) : 0;
  f.f32_xmax = (float)p.L;
  f.wo = writeout_params(p.A, p.K, p.out_f64 != 0);
  f.slow_cnt_r = nullptr; f.slow_list_r = nullptr; f.slow_flag_r = nullptr;
  f.slow_cnt_w = nullptr; f.slow_list_w = nullptr; f.slow_flag_w = nullptr; f.slow_cnt_z = nullptr;
  return f;
}

// Slow envs first: this launch reads set (launches % 3), builds the next one and clears the one after, and moves on.
void rotate_slow_sets(DiralEnv* e, FastParams& f, hipStream_t s) {
  const size_t w = slow_set_words(e);
  uint32_t* const set_r = e->slow + (e->slow_launches % 3) * w;
  uint32_t* const set_w = e->slow + ((e->slow_launches + 1) % 3) * w;
  uint32_t* const set_z = e->slow + ((e->slow_launches + 2) % 3) * w;
  f.slow_cnt_r = set_r; f.slow_list_r = set_r + 16; f.slow_flag_r = set_r + 16 + fast_slow_max(e->B);
  if (e->capture_rotates || !stream_is_capturing(s)) {
    f.slow_cnt_w = set_w; f.slow_list_w = set_w + 16; f.slow_flag_w = set_w + 16 + fast_slow_max(e->B);
    f.slow_cnt_z = set_z;
    ++e->slow_launches;
  }
  // (a CAPTURED launch reads the set it was baked with and builds none: a replayed graph could not rotate the sets -
  // unless the caller keeps every graph at a multiple of three launches and its phase aligned:
  // diral_env_set_capture_rotation.  Eager launches between two replays keep rotating through that set: they leave it
  // either rebuilt or EMPTY - count and flags, step_params.hpp - never half cleared, so the replay runs every env
  // exactly once whatever happened in between; the list it reads ages - slow envs stay slow for hundreds of slots,
  // profiles/launch_timeline.py - or is empty, which costs time, not correctness.)
}

// Executes a plan.  `pol`: the policy request the plan was made for; where the plan is `fused` the policy epilogue is
// part of this launch, otherwise the plain step is launched and diral_env_step_policy adds the two policy launches.
hipError_t launch_step_any(DiralEnv* e, const StepParams& p, const StepPlan& d, hipStream_t s, const PolParams* pol = nullptr) {
  const hipError_t st = d.use_ring ? ensure_ring(e, s) : ensure_plane(e, s);
  if (st != hipSuccess) return st;
  if (d.use_ring) e->plane_valid = false;
  else if (p.mode != kModeObserve) e->ring_valid = false;      // this step moves the tables without the ring
  e->last_kernel = d.last_kernel;
  if (d.launch == StepLaunch::Large) return launch_large(p, e->lg, s);
  if (d.launch == StepLaunch::General) return launch_general(e->vpl, d.general_fast, p, e->lds_bytes, s);
  if (d.launch == StepLaunch::Subwave) return launch_subwave(p, s);
  if (d.launch == StepLaunch::SubwaveSlots) return launch_subwave_slots(p, *pol, s);
  FastParams f = fast_params(e, p, d);
  if (d.slow_sets) rotate_slow_sets(e, f, s);
  RichParams r = rich_for(e, p);
  r.chobs_out = p.chobs_out;
  r.pf = ((p.flags & DIRAL_F_PROPORTIONAL_FAIR) && p.mode == DIRAL_STEP_MY_STEP) ? p.pf : nullptr;
  r.pf_threshold = p.pf_threshold; r.pf_penalty = p.pf_penalty;
  const int grid = p.B + (d.slow_sets ? fast_slow_max(p.B) : 0);
  switch (d.launch) {
    // K slots per launch with the policy epilogue at 64 < N <= 256: step_wide_slots_kernel, blocks = envs in batch order
    case StepLaunch::WideSlots: return launch_wide_slots(f, r, *pol, d.k, e->vpl, p.B, s);
    case StepLaunch::Wide: return e->vpl == 2 ? launch_wide2(f, r, d.k, grid, s) : launch_wide4(f, r, d.k, grid, s);
    // the env stays on the chip from slot to slot: step_fast64_slots_kernel
    case StepLaunch::Fast64Slots: return launch_fast64_slots(f, r, *pol, d.k.ch, d.k.out64, p.B, s);
    case StepLaunch::Fast64Policy: return launch_fast64_policy(f, r, *pol, d.k.out64, grid, s);
    default: return launch_fast64(f, r, d.k, grid, s);
  }
}

// Secondary observation modes (a15/a16) run as their own launch after the step (posdist_kernel.hpp).
hipError_t launch_posdist_if_needed(DiralEnv* e, const StepParams& p, hipStream_t s) {
  const bool full = (p.flags & DIRAL_F_ADD_POSDIST) != 0;
  const bool type1 = (p.flags & DIRAL_F_ADD_POSDIST_PIGGY) && p.posdist_type == 1;
  if (!secondary_obs(p)) return hipSuccess;
  PosdistParams q;
  q.N = p.N; q.A = p.A; q.K = p.K; q.S = p.S; q.NV = p.NV; q.NR = p.NR; q.flags = p.flags;
  q.posdist_type = p.posdist_type; q.age_limit = p.age_limit; q.out_f64 = p.out_f64;
  q.off_posdist = p.off_posdist; q.off_hist = p.off_hist;
  q.pos_x = p.pos_x; q.pos_y = p.pos_y; q.tkey = p.tkey; q.tx = p.tx; q.edges1 = e->edges1; q.state_out = p.state_out;
  q.do_full = 0; q.do_type1 = 0; q.ring = nullptr; q.tcode = nullptr; q.tage = nullptr; q.tseq = nullptr;
  q.flat_y = e->flat_y ? 1 : 0;
  const bool full_flat = full && e->flat_y;                     // one ranking of the env's x serves every viewer
  const bool type1_n64 = type1 && p.NV == 64 && p.K <= DIRAL_SMALL_MAX_BINS;   // lane = viewer, sort in registers
  const bool type1_lanes = type1 && !type1_n64 && p.N <= DIRAL_SMALL_MAX_USERS && p.K <= DIRAL_SMALL_MAX_BINS;   // 4 / 8 lanes per viewer (N <= 128 / 256)
  const bool type1_generic = type1 && !type1_n64 && !type1_lanes;   // beyond: posdist_kernel's literal statement
  if (full_flat) {
    q.do_full = 1;
    hipLaunchKernelGGL(posdist_sorted_flat_kernel, dim3(p.B), dim3(256), posdist_flat_lds_bytes(p.N), s, q);
    q.do_full = 0;
  }
  if (type1_n64) {
    q.do_type1 = 1;
    q.ring = (e->ring && !e->plane_valid) ? e->ring : nullptr;  // young entries straight from the ring: no materialise pass
    if (q.ring && e->tcode) { q.tcode = e->tcode; q.tage = e->tage; q.tseq = e->tseq; }   // ... and the words from the packed table
    hipLaunchKernelGGL(posdist_type1_n64_kernel, dim3(p.B), dim3(64), posdist_type1_lds_bytes(p.K), s, q);
    q.do_type1 = 0; q.ring = nullptr; q.tcode = nullptr; q.tage = nullptr; q.tseq = nullptr;
  }
  if (type1_lanes) {
    const int npad = p.N <= 128 ? 128 : 256;
    const int lpv = npad / 32, vw = 64 / lpv, nvb = (p.N + vw - 1) / vw;
    q.do_type1 = 1;
    q.ring = (e->ring && !e->plane_valid) ? e->ring : nullptr;
    if (q.ring && e->tcode) { q.tcode = e->tcode; q.tage = e->tage; q.tseq = e->tseq; }
    const uint32_t lds = posdist_type1_lanes_lds_bytes(p.K, npad, lpv);
    const dim3 grid((unsigned)p.B * nvb);
    if (lpv == 4) hipLaunchKernelGGL((posdist_type1_lanes_kernel<4, 32>), grid, dim3(64), lds, s, q);
    else hipLaunchKernelGGL((posdist_type1_lanes_kernel<8, 32>), grid, dim3(64), lds, s, q);
    q.do_type1 = 0; q.ring = nullptr; q.tcode = nullptr; q.tage = nullptr; q.tseq = nullptr;
  }
  q.do_full = (full && !full_flat) ? 1 : 0;
  q.do_type1 = type1_generic ? 1 : 0;
  if (q.do_full || q.do_type1) {
    if (q.do_type1) {                                           // (the sorted true distances read no table)
      const hipError_t st = ensure_plane(e, s);
      if (st != hipSuccess) return st;
    }
    if (posdist_lds_bytes(p.N, p.K) > 160u * 1024u) return hipErrorInvalidValue;   // (off-lane vehicles at N >~ 1400: one env's values do not fit)
    hipLaunchKernelGGL(posdist_kernel, dim3(p.B), dim3(64 * kPdWaves), posdist_lds_bytes(p.N, p.K), s, q);
  }
  return hipGetLastError();
}

PiggyParams piggy_params(const DiralEnv* e, const StepParams& p) {
  PiggyParams q;
  q.N = e->N; q.A = e->A; q.S = e->S; q.off_chobs = e->off_chobs_pb; q.out_f64 = p.out_f64; q.Rc = p.Rc;
  q.actions = p.actions; q.pos_x = e->pos_x; q.pos_y = e->pos_y;
  q.obs_new = e->obs_new; q.txid = e->txid; q.prev_obs = e->prev_obs;
  q.chobs_out = p.chobs_out; q.state_out = p.state_out; q.chobs_in = p.chobs_in; q.err = e->err;
  return q;
}

// The parameters of one call: the handle's `base` plus what every step / observe entry point is handed.  The output
// and input buffers other than the state vector stay null (as in `base`) for the caller to set.
StepParams call_params(const DiralEnv* e, int mode, int64_t t, const int32_t* actions, void* state_out, int out_dtype,
                       double episode, double epsilon) {
  StepParams p = e->base;
  p.mode = mode; p.t = t; p.episode = episode; p.eps = epsilon; p.out_f64 = (out_dtype == DIRAL_F64);
  p.actions = actions;
  p.state_out = e->S > 0 ? state_out : nullptr;
  return p;
}

// Recompute DiralEnv::flat_y (all pos_y == 0) after pos_y was written by the
// caller.  Synchronises the stream; only reset/import call it, never step.
int refresh_flat_y(DiralEnv* e, hipStream_t s) {
  const size_t bn = (size_t)e->B * e->N;
  if (hipMemsetAsync(e->yflag, 0, 4, s) != hipSuccess) return DIRAL_ERR_HIP;
  if (launch_1d<any_nonzero_kernel>(bn, s, (int)bn, e->pos_y, e->yflag) != hipSuccess) return DIRAL_ERR_HIP;
  uint32_t f = 1;
  if (hipMemcpyAsync(&f, e->yflag, 4, hipMemcpyDeviceToHost, s) != hipSuccess) return DIRAL_ERR_HIP;
  if (hipStreamSynchronize(s) != hipSuccess) return DIRAL_ERR_HIP;
  e->flat_y = (f == 0);
  return DIRAL_OK;
}

// The argument checks every step entry point shares: the step mode (`not_taken`: the one DIRAL_STEP_* the entry does not
// take, -1: it takes all three), the out dtype, my_step_ch's reward_design - rewards only for 2, 3, 4 (test_env.py:413-429)
int call_check(const DiralEnv* e, int mode, int not_taken, int out_dtype) {
  if ((mode != DIRAL_STEP_MY_STEP && mode != DIRAL_STEP_MY_STEP_CH && mode != DIRAL_STEP_DESIGN) || mode == not_taken) return DIRAL_ERR_BAD_ARG;
  if (out_dtype != DIRAL_F32 && out_dtype != DIRAL_F64) return DIRAL_ERR_BAD_ARG;
  if (mode == DIRAL_STEP_MY_STEP_CH && (e->cfg.reward_design < 2 || e->cfg.reward_design > 4)) return DIRAL_ERR_BAD_CONFIG;
  return DIRAL_OK;
}
// The shaping fields DiralSlotPolicy and DiralRollout share by name (`S`: either), checked and handed to the slot loops;
// `shaped_out`: the struct's own buffer or a memory block's reward ring
template <typename S>
int shaping_params(const S& s, void* shaped_out, const void* rew_out, PolParams& q) {
  if ((s.shape_flags & ~5) != 0) return DIRAL_ERR_BAD_ARG;       // global_reward_avg | stuck-action penalty
  if (s.shaped_out && !rew_out) return DIRAL_ERR_BAD_ARG;        // (the three-launch form and the wide slot loop shape rew_out)
  if (shaped_out && (s.shape_flags & 4) && (!s.pen_counter || !s.pen_prev_actions)) return DIRAL_ERR_BAD_ARG;
  q.shape_flags = s.shape_flags; q.pen_threshold = s.pen_threshold; q.pen_value = s.pen_value;
  q.shaped_out = shaped_out; q.sum_r_out = s.sum_r_out; q.coll_out = s.collision_out;
  q.pen_counter = s.pen_counter; q.pen_prev = s.pen_prev_actions;
  return DIRAL_OK;
}
// The launch-wide fields; `vel_updates`: mobility_vary's draws behind episode ends (the prefill's slots all run at t = 0)
void launch_params(const DiralEnv* e, int slots, bool vel_updates, uint64_t vel_seed, PolParams& q) {
  q.K = slots; q.vel_vary = (vel_updates && has(&e->cfg, DIRAL_F_MOBILITY_VARY)) ? 1 : 0; q.vel_seed = vel_seed;
  q.idx0 = (uint64_t)e->env_offset * (uint64_t)e->N; q.vel_w = e->vel;
}

}  // namespace

extern "C" {

int diral_env_abi_version(void) { return DIRAL_ABI_VERSION; }

const char* diral_env_strerror(int status) {
  switch (status) {
    case DIRAL_OK: return "ok";
    case DIRAL_ERR_BAD_ARG: return "bad argument";
    case DIRAL_ERR_BAD_CONFIG: return "config rejected (the reference cannot run it either, or undefined behaviour there)";
    case DIRAL_ERR_UNSUPPORTED: return "valid reference config outside this build's limits";
    case DIRAL_ERR_HIP: return "HIP runtime error (see diral_env_last_hip_error)";
    case DIRAL_ERR_NO_DEVICE: return "no usable HIP device";
    case DIRAL_ERR_ACTION_RANGE: return "action outside [0, num_channels)";
    case DIRAL_ERR_SEQ_OVERFLOW: return "more than DIRAL_MAX_SLOTS steps since reset";
    case DIRAL_ERR_CAPTURE: return "call needs a ring <-> plane conversion and the stream is being captured into a hipGraph";
    case DIRAL_ERR_TABLE_CONFLICT: return "imported tables hold entries about one subject with equal sequence numbers but different xpos";
    case DIRAL_ERR_PIGGY_NO_TX: return "State.piggybacking: a receiver heard no transmitter on a used resource (the reference's prev_obs[None] KeyError)";
    case DIRAL_ERR_ENV_INDEX: return "diral_env_copy_envs / diral_env_reset_envs: an env index outside its handle (that entry was skipped)";
    default: return "unknown status";
  }
}

void diral_cfg_defaults(DiralCfg* c) {
  if (!c) return;
  std::memset(c, 0, sizeof(*c));
  c->struct_bytes = sizeof(DiralCfg);
  c->flags = 0;
  c->num_users = 3;            // test_env.py:12
  c->num_channels = 3;         // test_env.py:13
  c->num_bins = 20;
  c->reward_design = 1;        // test_env.py:20
  c->state_type = 2;
  c->posdist_type = 2;
  c->episode_interval = 25;    // main_test.py:22
  c->info_age_limit = 20;      // network.py:547
  c->pf_threshold = 10;        // test_env.py:89
  c->pf_penalty = -10.0;       // test_env.py:90
  c->highway_length = 200;     // test_env.py:18
  c->highway_height = 2;       // network.py:31
  c->communication_range = 1;  // test_env.py:21
  c->bin_range = 500;          // test_env.py:24
}

int diral_env_validate(const DiralCfg* c) {
  if (!c || c->struct_bytes != sizeof(DiralCfg)) return DIRAL_ERR_BAD_ARG;
  if (c->num_users < 1 || c->num_channels < 1) return DIRAL_ERR_BAD_CONFIG;
  if (c->reward_design < 1 || c->reward_design > 5) return DIRAL_ERR_BAD_CONFIG;   // test_env.py:198-199
  if (c->state_type != 1 && c->state_type != 2) return DIRAL_ERR_BAD_CONFIG;
  if (!has(c, DIRAL_F_MOBILITY) && !has(c, DIRAL_F_DESIGN_TOPOLOGY)) return DIRAL_ERR_BAD_CONFIG;  // network.py:54-60
  if (c->episode_interval < 1 || c->info_age_limit < 0 || c->info_age_limit > 255) return DIRAL_ERR_BAD_CONFIG;
  if (!(c->highway_length > 0) || !(c->highway_height > 0)) return DIRAL_ERR_BAD_CONFIG;
  if (has(c, DIRAL_F_ADD_POSDIST_PIGGY)) {
    if (c->posdist_type != 1 && c->posdist_type != 2) return DIRAL_ERR_BAD_CONFIG;  // test_env.py:555-560
    if (c->num_bins < 1 || !(c->bin_range > 0)) return DIRAL_ERR_BAD_CONFIG;
    if (c->num_bins > DIRAL_MAX_BINS) return DIRAL_ERR_UNSUPPORTED;
  }
  if (has(c, DIRAL_F_PIGGYBACKING)) {
    // type 1 inserts on idle resources only (test_env.py:226-232, 250-254): ragged observations; without the
    // channel-observation section obtain_state never reads what get_state_space() counts (test_env.py:71-72, 539-541)
    if (c->state_type != 2 || !has(c, DIRAL_F_ADD_CHANNEL_OBS)) return DIRAL_ERR_BAD_CONFIG;
  }
  if (c->num_users > DIRAL_MAX_USERS || c->num_channels > DIRAL_MAX_CHANNELS) return DIRAL_ERR_UNSUPPORTED;
  const int kbins = c->num_bins > 0 ? c->num_bins : 1;
  if (is_large_cfg(c)) {
    // step_large.hpp: the env's vehicles and resource lists in one workgroup's LDS, a table column in a wave's
    if (large_lds_bytes(c->num_users, c->num_channels, kbins) > 160u * 1024u) return DIRAL_ERR_UNSUPPORTED;
    // State.piggybacking: A * A values per agent, indexed with 32 bits in piggyback_kernel.hpp
    if (has(c, DIRAL_F_PIGGYBACKING) && c->num_channels > DIRAL_SMALL_MAX_CHANNELS) return DIRAL_ERR_UNSUPPORTED;
    // the type-1 histogram at these sizes is posdist_kernel's literal statement: one env's values in LDS (N <~ 1400)
    if (has(c, DIRAL_F_ADD_POSDIST_PIGGY) && c->posdist_type == 1 && posdist_lds_bytes(c->num_users, kbins) > 160u * 1024u)
      return DIRAL_ERR_UNSUPPORTED;
    if (has(c, DIRAL_F_ADD_POSDIST) && posdist_flat_lds_bytes(c->num_users) > 160u * 1024u) return DIRAL_ERR_UNSUPPORTED;
    return DIRAL_OK;
  }
  const int vpl = vpl_for(c->num_users);
  const LdsLayout l = lds_layout(64 * vpl, c->num_channels, kbins, vpl, 4 * vpl);
  if (l.total > 160u * 1024u) return DIRAL_ERR_UNSUPPORTED;
  return DIRAL_OK;
}

// the sizes step_subwave.hpp holds: a viewer's N table entries in its lane's registers, one 4-bit gather source per
// resource in a 64-bit word, a 4-bit count per bin in four
int diral_env_subwave_ok(const DiralCfg* c) {
  const int st = diral_env_validate(c);
  if (st != DIRAL_OK) return st;
  if (c->num_users > DIRAL_SUBWAVE_MAX_USERS || c->num_channels > DIRAL_SUBWAVE_MAX_CHANNELS ||
      c->num_bins > DIRAL_SMALL_MAX_BINS)
    return DIRAL_ERR_UNSUPPORTED;
  if (has(c, DIRAL_F_PIGGYBACKING)) return DIRAL_ERR_UNSUPPORTED;   // (the A * A observation: piggyback_kernel.hpp's paths only)
  return DIRAL_OK;
}

int diral_env_state_space(const DiralCfg* c) {
  if (!c || c->struct_bytes != sizeof(DiralCfg)) return DIRAL_ERR_BAD_ARG;
  return state_offsets(c).S;
}

int diral_env_create(const DiralCfg* cfg, int batch, int device, DiralEnv** out) {
  if (!out) return DIRAL_ERR_BAD_ARG;
  *out = nullptr;
  int st = diral_env_validate(cfg);
  if (st != DIRAL_OK) return st;
  if (batch < 1) return DIRAL_ERR_BAD_ARG;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) return DIRAL_ERR_NO_DEVICE;
  if (device < 0 || device >= ndev) return DIRAL_ERR_NO_DEVICE;

  DiralEnv* e = new DiralEnv();
  e->cfg = *cfg;
  e->hooks = read_hooks();
  e->B = batch; e->N = cfg->num_users; e->A = cfg->num_channels;
  e->K = cfg->num_bins > 0 ? cfg->num_bins : 1;
  e->NV = e->N <= 64 ? 64 : (int)align_up((uint32_t)e->N, 16);   // one wave lane per viewer, no lane predicate
  e->NR = (int)align_up((uint32_t)e->N, 16);   // every wave owns 16 existing subject rows
  e->vpl = vpl_for(e->N);
  e->large = is_large_cfg(cfg);
  e->device = device;
  const Offsets off = state_offsets(cfg);
  e->S = off.S;

  auto fail = [&](int code) { diral_env_destroy(e); return code; };
  DeviceGuard guard(device);
  if (!guard.ok) return fail(DIRAL_ERR_NO_DEVICE);

  const size_t bn = (size_t)e->B * e->N;
  const size_t tab = (size_t)e->B * e->NR * e->NV;
#define CREATE_TRY(call) do { hipError_t r__ = (call); if (r__ != hipSuccess) { note_hip(e, r__, #call); \
      std::fprintf(stderr, "diral_env_create: %s\n", e->last_hip_error.c_str()); return fail(DIRAL_ERR_HIP); } } while (0)
  // (diral_env_reset fills the buffers marked kOnReset in THIS order; reset_kernel writes the first three)
  CREATE_TRY(own(e, e->pos_x, bn * 8));
  CREATE_TRY(own(e, e->pos_y, bn * 8));
  CREATE_TRY(own(e, e->vel, bn * 8));
  // + 512 elements of slack: step_wide.hpp loads a padded viewer slot (lane + 64 j) past the
  // end of a row without clamping (the values are masked, never stored)
  // + 64 rows: the type-1 kernels (posdist_kernel.hpp) read the rows up to the next multiple of 64 of their env
  // unmasked as well
  const size_t tab_slack = 512 + 64 * 256;
  CREATE_TRY(own(e, e->tkey, tab * 4, tab_slack * 4, kOnReset));
  CREATE_TRY(own(e, e->tx, tab * 8, tab_slack * 8, kOnReset));
  if (fits_fast64(e) || fits_wide(e)) {                         // the xpos ring of the specialised kernels
    CREATE_TRY(own(e, e->ring, (size_t)e->B * e->NR * 8 * 8, 0, kOnReset));
    if (use_packed_table(e)) {                                  // the packed table of step_fast64 and of step_wide at N > 128
      // (+ 512 words of slack: step_wide.hpp loads a padded viewer slot past the end of a row without clamping)
      const size_t nq = (size_t)e->B * (e->NR / 4);
      CREATE_TRY(own(e, e->tcode, nq * e->NV * 4, 512 * 4, kOnReset));
      CREATE_TRY(own(e, e->tage, nq * e->NV * 4, 512 * 4, kOnReset));
      CREATE_TRY(own(e, e->tseq, (size_t)e->B * e->NR * 4, 64 * 4, kOnReset));
      CREATE_TRY(own(e, e->told, nq * 4, 16 * 4, kOnReset));
    }
    CREATE_TRY(own(e, e->slow, 3 * slow_set_words(e) * 4, 0, kOnReset));
    e->ring_valid = true;                                       // all tables zero: never heard, age 0, xpos 0
  }
  CREATE_TRY(own(e, e->metrics, (size_t)e->B * DIRAL_M_COLUMNS * 8, 0, kOnReset));
  CREATE_TRY(own(e, e->err, 4));
  CREATE_TRY(own(e, e->yflag, 4, 0, false, kNoFill));
  CREATE_TRY(own(e, e->edges, (size_t)(e->K + 1) * 8, 0, false, kNoFill));
  CREATE_TRY(own(e, e->edges1, (size_t)(e->K + 1) * 8, 0, false, kNoFill));
  CREATE_TRY(own(e, e->inv_tab, 256 * 8, 0, false, kNoFill));
  if (has(cfg, DIRAL_F_TRACK_ARRIVAL)) CREATE_TRY(own(e, e->la, bn * e->N * 4, 0, kOnReset, 0xFF));
  if (has(cfg, DIRAL_F_PROPORTIONAL_FAIR)) CREATE_TRY(own(e, e->pf, bn * 4, 0, kOnReset));
  if (has(cfg, DIRAL_F_PIGGYBACKING)) {
    if (piggy_search_lds_bytes(e->N) > 48u * 1024u)
      CREATE_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(piggy_search_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                     (int)piggy_search_lds_bytes(e->N)));
    CREATE_TRY(own(e, e->prev_obs, bn * e->A * 8, 0, kOnReset));   // test_env.py:76-79
    CREATE_TRY(own(e, e->obs_new, bn * e->A * 8, 0, false, kNoFill));
    CREATE_TRY(own(e, e->txid, bn * e->A * 4, 0, false, kNoFill));
  }

  std::vector<double> edges;
  np_linspace(-cfg->bin_range, cfg->bin_range, e->K + 1, edges);
  for (int i = 0; i < e->K; ++i)   // np.histogram: "Too many bins for data range"
    if (!(edges[i] < edges[i + 1])) return fail(DIRAL_ERR_BAD_CONFIG);
  CREATE_TRY(hipMemcpy(e->edges, edges.data(), edges.size() * 8, hipMemcpyHostToDevice));
  np_linspace(-1.0, 1.0, e->K + 1, edges);
  CREATE_TRY(hipMemcpy(e->edges1, edges.data(), edges.size() * 8, hipMemcpyHostToDevice));
  {
    std::vector<double> inv(256, 0.0);
    for (int n = 1; n < 256; ++n) { volatile double d = (double)n; inv[n] = 1.0 / d; }
    CREATE_TRY(hipMemcpy(e->inv_tab, inv.data(), 256 * 8, hipMemcpyHostToDevice));
  }
  if (posdist_lds_bytes(e->N, e->K) <= 160u * 1024u)
    CREATE_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(posdist_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                   (int)posdist_lds_bytes(e->N, e->K)));
  if (posdist_flat_lds_bytes(e->N) > 48u * 1024u && posdist_flat_lds_bytes(e->N) <= 160u * 1024u)
    CREATE_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(posdist_sorted_flat_kernel),
                                   hipFuncAttributeMaxDynamicSharedMemorySize, (int)posdist_flat_lds_bytes(e->N)));
  if (!e->large)
    CREATE_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(posdist_type1_n64_kernel),
                                   hipFuncAttributeMaxDynamicSharedMemorySize, (int)posdist_type1_lds_bytes(e->K)));

  if (e->large) {
    CREATE_TRY(alloc_large_scratch(e));
  } else {
    const LdsLayout l = lds_layout(64 * e->vpl, e->A, e->K, e->vpl, 4 * e->vpl);
    e->lds_bytes = l.total;
    CREATE_TRY(set_attr_general(e->vpl, l.total));
    if (fits_wide(e)) {
      CREATE_TRY(e->vpl == 2 ? set_attr_wide2(e->A, e->K) : set_attr_wide4(e->A, e->K));
      CREATE_TRY(set_attr_wide_slots(e->vpl, e->A, e->K));
    }
    CREATE_TRY(set_attr_observe(e->N, e->K));
  }
#undef CREATE_TRY

  StepParams& p = e->base;
  std::memset(&p, 0, sizeof(p));
  p.B = e->B; p.N = e->N; p.A = e->A; p.K = e->K; p.S = e->S; p.NV = e->NV; p.NR = e->NR;
  p.flags = cfg->flags;
  p.reward_design = cfg->reward_design; p.state_type = cfg->state_type; p.posdist_type = cfg->posdist_type;
  p.age_limit = cfg->info_age_limit; p.pf_threshold = cfg->pf_threshold; p.pf_penalty = cfg->pf_penalty;
  p.L = cfg->highway_length; p.H = cfg->highway_height; p.Rc = cfg->communication_range;
  p.Rb = cfg->bin_range;
  p.hist_inv_width = (double)e->K / (cfg->bin_range - (-cfg->bin_range));
  p.episode_interval = cfg->episode_interval;
  p.off_act = off.act; p.off_chobs = off.chobs; p.off_posdist = off.posdist; p.off_hist = off.hist;
  if (has(cfg, DIRAL_F_PIGGYBACKING)) {
    // the step / observe kernels build a state vector WITHOUT the channel-observation section and leave its A * A
    // columns alone (rich_for); piggyback_kernel.hpp fills them
    e->off_chobs_pb = off.chobs;
    p.off_chobs = -1;
    p.flags &= ~(uint32_t)DIRAL_F_ADD_CHANNEL_OBS;
  }
  p.off_rew = off.rew; p.off_idx = off.idx; p.off_pos = off.pos; p.off_vel = off.vel; p.off_fp = off.fp;
  p.pos_x = e->pos_x; p.pos_y = e->pos_y; p.vel = e->vel; p.tkey = e->tkey; p.tx = e->tx;
#if defined(DIRAL_TIMING) || defined(DIRAL_DEBUG_XG)
  if (hipMalloc((void**)&e->dbg, (size_t)e->B * 4096 * 8) == hipSuccess) (void)hipMemset(e->dbg, 0, (size_t)e->B * 4096 * 8);
#endif
  p.dbg = e->dbg;
  p.la = e->la; p.pf = e->pf; p.metrics = e->metrics; p.err = e->err; p.edges = e->edges;
  RichParams& r = e->rich;
  std::memset(&r, 0, sizeof(r));
  r.S = e->S; r.state_type = cfg->state_type;
  r.off_act = off.act; r.off_chobs = has(cfg, DIRAL_F_PIGGYBACKING) ? -1 : off.chobs; r.off_hist = off.hist; r.off_rew = off.rew; r.off_idx = off.idx;
  r.off_skip = 0; r.len_skip = 0;
  r.off_pos = off.pos; r.off_vel = off.vel; r.off_fp = off.fp;
  r.H = cfg->highway_height; r.vel = e->vel; r.pos_y = e->pos_y;
  // test hooks: force the general kernel
  if (e->hooks.no_fast64 && e->vpl == 1) e->kernel_path = DIRAL_PATH_GENERAL;
  if (e->hooks.no_wide && e->vpl > 1 && !e->large) e->kernel_path = DIRAL_PATH_GENERAL;
  *out = e;
  return DIRAL_OK;
}

int diral_env_destroy(DiralEnv* e) {
  if (!e) return DIRAL_OK;
  DeviceGuard guard(e->device);
  for (const DevBuf& b : e->bufs) (void)hipFree(b.p);
  if (e->trace) (void)hipFree(e->trace);
  if (e->dbg) (void)hipFree(e->dbg);
  delete e;
  return DIRAL_OK;
}

int64_t diral_env_hbm_bytes(const DiralEnv* e) {
  int64_t sum = 0;
  if (e) for (const DevBuf& b : e->bufs) sum += (int64_t)b.bytes;
  return sum;
}

int diral_env_set_option(DiralEnv* e, int option, int64_t value) {
  if (!e) return DIRAL_ERR_BAD_ARG;
  switch (option) {
    case DIRAL_OPT_ENV_OFFSET:
      if (value < 0) return DIRAL_ERR_BAD_ARG;
      e->env_offset = value;
      return DIRAL_OK;
    case DIRAL_OPT_KERNEL_PATH:
      if (value != DIRAL_PATH_AUTO && value != DIRAL_PATH_GENERAL && value != DIRAL_PATH_LARGE && value != DIRAL_PATH_SUBWAVE)
        return DIRAL_ERR_BAD_ARG;
      if (value == DIRAL_PATH_SUBWAVE) {                          // (opt-in; a refusal leaves the path as it was)
        const int ok = e->large ? DIRAL_ERR_UNSUPPORTED : diral_env_subwave_ok(&e->cfg);
        if (ok != DIRAL_OK) return ok;
        e->kernel_path = DIRAL_PATH_SUBWAVE;
        return DIRAL_OK;
      }
      if (e->large) return value == DIRAL_PATH_GENERAL ? DIRAL_ERR_UNSUPPORTED : DIRAL_OK;   // (there is one path for such a handle)
      if (value == DIRAL_PATH_LARGE) {
        if (large_lds_bytes(e->N, e->A, e->K) > 160u * 1024u) return DIRAL_ERR_UNSUPPORTED;
        DEVICE_ENTER(e->device);
        HIP_TRY(e, alloc_large_scratch(e));
      }
      e->kernel_path = (int)value;
      e->subwave_slots = false;                                    // (leaving DIRAL_PATH_SUBWAVE clears DIRAL_OPT_SUBWAVE_SLOTS)
      return DIRAL_OK;
    case DIRAL_OPT_SUBWAVE_SLOTS:
      if (value != 0 && value != 1) return DIRAL_ERR_BAD_ARG;
      if (value == 1 && e->kernel_path != DIRAL_PATH_SUBWAVE) return DIRAL_ERR_UNSUPPORTED;
      e->subwave_slots = value == 1;
      return DIRAL_OK;
    default:
      return DIRAL_ERR_BAD_ARG;
  }
}

int diral_env_last_kernel(const DiralEnv* e) { return e ? e->last_kernel : DIRAL_ERR_BAD_ARG; }

const char* diral_env_last_hip_error(const DiralEnv* e) { return e ? e->last_hip_error.c_str() : ""; }

int diral_env_reset(DiralEnv* e, const double* x0, const double* y0, const double* v0, uint64_t seed,
                    void* stream) {
  if (!e) return DIRAL_ERR_BAD_ARG;
  DEVICE_ENTER(e->device);
  hipStream_t s = (hipStream_t)stream;
  const size_t bn = (size_t)e->B * e->N;
  // tables, ring, packed table, slow-env sets, metrics, la (0xFF), pf, prev_obs - as a fresh handle has them
  for (const DevBuf& b : e->bufs)
    if (b.reset_bytes) HIP_TRY(e, hipMemsetAsync(b.p, b.fill, b.reset_bytes, s));
  e->slow_launches = 0;
  e->plane_valid = true; e->ring_valid = e->ring != nullptr;
  HIP_TRY(e, launch_1d<reset_kernel>(bn, s, (int)bn, e->cfg.highway_length, has(&e->cfg, DIRAL_F_MOBILITY_VARY) ? 1 : 0, seed,
                                     (uint64_t)e->env_offset * (uint64_t)e->N, x0, y0, v0, e->pos_x, e->pos_y, e->vel));
  if (y0) { if (refresh_flat_y(e, s) != DIRAL_OK) return DIRAL_ERR_HIP; }
  else e->flat_y = true;
  return DIRAL_OK;
}

int diral_env_step(DiralEnv* e, int mode, const int32_t* actions, int64_t t, void* state_out, void* rew_out,
                   uint8_t* done_out, void* chobs_out, int out_dtype, double episode, double epsilon,
                   void* stream) {
  if (!e || !actions) return DIRAL_ERR_BAD_ARG;
  if (const int bad = call_check(e, mode, -1, out_dtype)) return bad;
  DEVICE_ENTER(e->device);
  hipStream_t s = (hipStream_t)stream;
  StepParams p = call_params(e, mode, t, actions, state_out, out_dtype, episode, epsilon);
  p.rew_out = rew_out; p.done_out = done_out; p.chobs_out = chobs_out;
  if (e->prev_obs) {
    // State.piggybacking: my_step_ch / my_step_design hand obtain_state the plain A-wide observation (test_env.py:316,
    // 443) - a state vector shorter than get_state_space()
    if (mode != DIRAL_STEP_MY_STEP) return DIRAL_ERR_BAD_CONFIG;
    const PiggyParams q = piggy_params(e, p);
    p.chobs_out = nullptr;                                       // (the A * A observation is piggy_emit_kernel's)
    HIP_TRY(e, launch_k<piggy_search_kernel>(dim3(e->B), dim3(256), piggy_search_lds_bytes(e->N), s, q));
    HIP_TRY(e, launch_step_any(e, p, plan_step(e, p, nullptr), s));
    HIP_TRY(e, launch_posdist_if_needed(e, p, s));
    HIP_TRY(e, launch_k<piggy_emit_kernel>(dim3(e->B), dim3(256), 0, s, q));
    return DIRAL_OK;
  }
  HIP_TRY(e, launch_step_any(e, p, plan_step(e, p, nullptr), s));
  HIP_TRY(e, launch_posdist_if_needed(e, p, s));
  return DIRAL_OK;
}

// The information-age block of a K-slot my_step_ch call (DiralSlotInfoAge): its own argument checks ...
static int ia_block_check(const DiralSlotInfoAge* ia, const void* shaped_out) {
  if (ia->struct_bytes != sizeof(DiralSlotInfoAge) || (ia->flags & ~1) != 0) return DIRAL_ERR_BAD_ARG;
  if ((ia->flags & 1) && (!ia->sum_ia_prev || !shaped_out)) return DIRAL_ERR_BAD_ARG;
  return DIRAL_OK;
}
// ... and what the slot loop is handed (PolParams::ia_on: bit 0 the block, bit 1 a histogram pass every slot)
static void ia_block_params(const DiralSlotInfoAge* ia, PolParams& q) {
  if (!ia) return;
  const bool hist = ia->ia_out || ia->ia_sum_out || (ia->flags & 1);
  q.ia_on = 1 | (hist ? 2 : 0); q.ia_flags = ia->flags;
  q.ia_out = ia->ia_out; q.ia_sum_out = (long long*)ia->ia_sum_out; q.ia_pen_out = ia->ia_pen_out;
  q.sum_ia_prev = (long long*)ia->sum_ia_prev;
}

// The recorded-mobility block of a K-slot call (DiralSlotReplay): its own argument checks ...
static int replay_block_check(const DiralSlotReplay* rp) {
  if (rp->struct_bytes != sizeof(DiralSlotReplay) || rp->flags != 0) return DIRAL_ERR_BAD_ARG;
  if (rp->x_positions ? rp->T < 1 : rp->T != 0) return DIRAL_ERR_BAD_ARG;
  return DIRAL_OK;
}
// ... and what the slot loop is handed (nothing where the block is absent or empty: the call is its _ia entry point's)
static void replay_block_params(const DiralSlotReplay* rp, PolParams& q) {
  if (!rp || (!rp->x_positions && !rp->xpos_out)) return;
  q.rp_on = 1; q.rp_T = rp->T; q.rp_per_env = rp->per_env ? 1 : 0; q.rp_x = rp->x_positions; q.rp_xout = rp->xpos_out;
}

// The memory block of a rollout / prefill (DiralMemory: diral_env_rollout_memory / diral_env_prefill_memory): its own
// argument checks - no device is needed for any of them ...
static int memory_block_check(const DiralEnv* e, const DiralMemory* m, int32_t slots, int out_dtype) {
  if (!memory_ok(m) || slots > m->capacity) return DIRAL_ERR_BAD_ARG;
  if (m->batch != e->B || m->num_users != e->N || m->state_space != e->S) return DIRAL_ERR_BAD_ARG;
  if (m->dtype != out_dtype) return DIRAL_ERR_BAD_ARG;           // (the stored bits are the scratch path's: no conversion)
  return DIRAL_OK;
}
// ... and what the slot loops are handed (a host count: its row; a device count is read by the kernel)
static void memory_block_params(const DiralMemory* m, PolParams& q) {
  if (!m) return;
  q.mem_on = 1; q.mem_rows = m->capacity + 1;
  q.mem_head = m->count_dev ? 0 : (int)(m->count % (int64_t)q.mem_rows);
  q.mem_count_dev = (const long long*)m->count_dev;
  q.mem_states = m->states; q.mem_actions = m->actions; q.mem_rewards = m->rewards;
}

static int step_policy_impl(DiralEnv* e, int mode, const int32_t* actions, int64_t t, void* state_out, void* rew_out,
                            uint8_t* done_out, void* chobs_out, int out_dtype, const DiralSlotPolicy* pol,
                            const DiralSlotInfoAge* ia, const DiralSlotReplay* rp, void* stream) {
  if (!e || !actions || !pol || pol->struct_bytes != sizeof(DiralSlotPolicy)) return DIRAL_ERR_BAD_ARG;
  if (rp && replay_block_check(rp) != DIRAL_OK) return DIRAL_ERR_BAD_ARG;
  if (ia && ia_block_check(ia, pol->shaped_out) != DIRAL_OK) return DIRAL_ERR_BAD_ARG;
  if (!pol->sps_prev_action || !pol->sps_counter || !pol->actions_out) return DIRAL_ERR_BAD_ARG;
  if (const int bad = call_check(e, mode, DIRAL_STEP_DESIGN, out_dtype)) return bad;
  SlotRequest req{{}, chobs_out != nullptr};
  PolParams& q = req.q;                                          // (no memory block: the closed loop writes the last state only)
  if (const int bad = shaping_params(*pol, pol->shaped_out, rew_out, q)) return bad;
  StepParams p = call_params(e, mode, t, actions, state_out, out_dtype, 0.0, 1.0);
  p.rew_out = rew_out; p.done_out = done_out; p.chobs_out = chobs_out;
  q.sps_prev = pol->sps_prev_action; q.sps_counter = pol->sps_counter;
  q.threshold = pol->rssi_threshold; q.inc_db = pol->inc_db; q.keep_prob = pol->keep_prob;
  q.draw_counter = pol->draw_counter; q.draw_keep = pol->draw_keep; q.draw_choice = pol->draw_choice;
  q.seed = pol->seed; q.clock = (const long long*)pol->seed_clock; q.actions_out = pol->actions_out;
  launch_params(e, pol->slots > 1 ? pol->slots : 1, true, pol->vel_seed, q);
  ia_block_params(ia, q); replay_block_params(rp, q);
  const StepPlan d = plan_step(e, p, &req);
  if (d.status != DIRAL_OK) return d.status;                     // (nothing launched, no device entered)
  DEVICE_ENTER(e->device);
  HIP_TRY(e, launch_step_any(e, p, d, (hipStream_t)stream, &q));
  HIP_TRY(e, launch_posdist_if_needed(e, p, (hipStream_t)stream));
  if (d.fused) return DIRAL_OK;
  // the same slot as three launches (configurations the POL instantiation does not take)
  if (pol->shaped_out) {
    const int st = diral_driver_shape(e->B, e->N, e->A, rew_out, out_dtype, actions, nullptr, nullptr, pol->pen_counter,
                                      pol->pen_prev_actions, pol->shape_flags, pol->pen_threshold, pol->pen_value,
                                      pol->shaped_out, pol->sum_r_out, pol->collision_out, nullptr, nullptr, stream);
    if (st != DIRAL_OK) return st;
  }
  return sps_step_chobs_with_clock(e->B * e->N, e->A, chobs_out, out_dtype, actions, pol->sps_prev_action, pol->sps_counter,
                                   pol->rssi_threshold, pol->inc_db, pol->keep_prob, pol->draw_counter, pol->draw_keep,
                                   pol->draw_choice, pol->seed, (const long long*)pol->seed_clock, pol->actions_out, stream);
}

int diral_env_step_policy(DiralEnv* e, int mode, const int32_t* actions, int64_t t, void* state_out, void* rew_out,
                          uint8_t* done_out, void* chobs_out, int out_dtype, const DiralSlotPolicy* pol, void* stream) {
  return step_policy_impl(e, mode, actions, t, state_out, rew_out, done_out, chobs_out, out_dtype, pol, nullptr, nullptr, stream);
}

int diral_env_step_policy_ia(DiralEnv* e, int mode, const int32_t* actions, int64_t t, void* state_out, void* rew_out,
                             uint8_t* done_out, void* chobs_out, int out_dtype, const DiralSlotPolicy* pol,
                             const DiralSlotInfoAge* ia, void* stream) {
  return step_policy_impl(e, mode, actions, t, state_out, rew_out, done_out, chobs_out, out_dtype, pol, ia, nullptr, stream);
}

int diral_env_step_policy_replay(DiralEnv* e, int mode, const int32_t* actions, int64_t t, void* state_out, void* rew_out,
                                 uint8_t* done_out, void* chobs_out, int out_dtype, const DiralSlotPolicy* pol,
                                 const DiralSlotInfoAge* ia, const DiralSlotReplay* rp, void* stream) {
  return step_policy_impl(e, mode, actions, t, state_out, rew_out, done_out, chobs_out, out_dtype, pol, ia, rp, stream);
}

static int prefill_impl(DiralEnv* e, int mode, const int32_t* actions, int32_t slots, uint64_t seed, void* states_out,
                        int out_dtype, int32_t* actions_all_out, int32_t* actions_next_out, const double* rew_in,
                        double episode, double epsilon, const DiralMemory* mem, void* stream) {
  if (!e || !actions || !actions_next_out || slots < 1) return DIRAL_ERR_BAD_ARG;
  if (mem) {
    // the rings take the place of the scratch outputs; the reward they store is the stale bootstrap one
    if (memory_block_check(e, mem, slots, out_dtype) != DIRAL_OK || states_out || actions_all_out || !rew_in) return DIRAL_ERR_BAD_ARG;
    states_out = mem->states;
  }
  if (const int bad = call_check(e, mode, DIRAL_STEP_MY_STEP, out_dtype)) return bad;
  const StepParams p = call_params(e, mode, 0, actions, states_out, out_dtype, episode, epsilon);
  SlotRequest req; PolParams& q = req.q;
  launch_params(e, slots, false, 0, q);
  q.prefill = 1; q.seed = seed;
  q.actions_out = actions_next_out; q.actions_all = actions_all_out; q.rew_in = rew_in;
  memory_block_params(mem, q);
  const StepPlan d = plan_step(e, p, &req);
  if (d.status != DIRAL_OK) return d.status;                     // (nothing launched, no device entered: the caller loops sample + step + observe)
  DEVICE_ENTER(e->device);
  HIP_TRY(e, launch_step_any(e, p, d, (hipStream_t)stream, &q));
  return DIRAL_OK;
}

int diral_env_prefill_mode(DiralEnv* e, int mode, const int32_t* actions, int32_t slots, uint64_t seed, void* states_out,
                           int out_dtype, int32_t* actions_all_out, int32_t* actions_next_out, const double* rew_in,
                           double episode, double epsilon, void* stream) {
  return prefill_impl(e, mode, actions, slots, seed, states_out, out_dtype, actions_all_out, actions_next_out, rew_in, episode,
                      epsilon, nullptr, stream);
}

int diral_env_prefill_memory(DiralEnv* e, int mode, const int32_t* actions, int32_t slots, uint64_t seed, void* states_out,
                             int out_dtype, int32_t* actions_all_out, int32_t* actions_next_out, const double* rew_in,
                             double episode, double epsilon, const DiralMemory* memory, void* stream) {
  return prefill_impl(e, mode, actions, slots, seed, states_out, out_dtype, actions_all_out, actions_next_out, rew_in, episode,
                      epsilon, memory, stream);
}

static int rollout_impl(DiralEnv* e, int mode, const int32_t* actions_seq, int32_t slots, int64_t t, void* states_out,
                        int states_all, void* rew_out, uint8_t* done_out, int out_dtype, const DiralRollout* ro,
                        const DiralSlotInfoAge* ia, const DiralSlotReplay* rp, const DiralMemory* mem, void* stream) {
  if (!e || !actions_seq || !ro || ro->struct_bytes != sizeof(DiralRollout) || slots < 1) return DIRAL_ERR_BAD_ARG;
  if (rp && replay_block_check(rp) != DIRAL_OK) return DIRAL_ERR_BAD_ARG;
  void* shaped_out = ro->shaped_out;
  if (mem) {
    // the rings take the place of the scratch outputs: every slot's state vector and shaped reward leave, into ring rows
    if (memory_block_check(e, mem, slots, out_dtype) != DIRAL_OK || states_out || ro->shaped_out) return DIRAL_ERR_BAD_ARG;
    states_out = mem->states; states_all = 1; shaped_out = mem->rewards;
  }
  if (ia && ia_block_check(ia, shaped_out) != DIRAL_OK) return DIRAL_ERR_BAD_ARG;
  SlotRequest req; PolParams& q = req.q;
  if (const int bad = shaping_params(*ro, shaped_out, rew_out, q)) return bad;
  if (const int bad = call_check(e, mode, DIRAL_STEP_DESIGN, out_dtype)) return bad;
  StepParams p = call_params(e, mode, t, actions_seq, states_out, out_dtype, 0.0, 1.0);
  p.rew_out = rew_out; p.done_out = done_out;
  launch_params(e, slots, true, ro->vel_seed, q);
  q.rollout = 1 | ((states_all && p.state_out) ? 2 : 0); q.actions_seq = actions_seq;
  ia_block_params(ia, q); replay_block_params(rp, q); memory_block_params(mem, q);
  const StepPlan d = plan_step(e, p, &req);
  if (d.status != DIRAL_OK) return d.status;                     // (nothing launched, no device entered: the caller loops step + shape)
  DEVICE_ENTER(e->device);
  HIP_TRY(e, launch_step_any(e, p, d, (hipStream_t)stream, &q));
  return DIRAL_OK;
}

int diral_env_rollout(DiralEnv* e, int mode, const int32_t* actions_seq, int32_t slots, int64_t t, void* states_out,
                      int states_all, void* rew_out, uint8_t* done_out, int out_dtype, const DiralRollout* ro, void* stream) {
  return rollout_impl(e, mode, actions_seq, slots, t, states_out, states_all, rew_out, done_out, out_dtype, ro, nullptr, nullptr, nullptr, stream);
}

int diral_env_rollout_ia(DiralEnv* e, int mode, const int32_t* actions_seq, int32_t slots, int64_t t, void* states_out,
                         int states_all, void* rew_out, uint8_t* done_out, int out_dtype, const DiralRollout* ro,
                         const DiralSlotInfoAge* ia, void* stream) {
  return rollout_impl(e, mode, actions_seq, slots, t, states_out, states_all, rew_out, done_out, out_dtype, ro, ia, nullptr, nullptr, stream);
}

int diral_env_rollout_replay(DiralEnv* e, int mode, const int32_t* actions_seq, int32_t slots, int64_t t, void* states_out,
                             int states_all, void* rew_out, uint8_t* done_out, int out_dtype, const DiralRollout* ro,
                             const DiralSlotInfoAge* ia, const DiralSlotReplay* rp, void* stream) {
  return rollout_impl(e, mode, actions_seq, slots, t, states_out, states_all, rew_out, done_out, out_dtype, ro, ia, rp, nullptr, stream);
}

int diral_env_rollout_memory(DiralEnv* e, int mode, const int32_t* actions_seq, int32_t slots, int64_t t, void* states_out,
                             int states_all, void* rew_out, uint8_t* done_out, int out_dtype, const DiralRollout* ro,
                             const DiralSlotInfoAge* ia, const DiralSlotReplay* rp, const DiralMemory* memory, void* stream) {
  return rollout_impl(e, mode, actions_seq, slots, t, states_out, states_all, rew_out, done_out, out_dtype, ro, ia, rp, memory, stream);
}

int diral_env_prefill(DiralEnv* e, const int32_t* actions, int32_t slots, uint64_t seed, void* states_out, int out_dtype,
                      int32_t* actions_all_out, int32_t* actions_next_out, const double* rew_in, double episode, double epsilon,
                      void* stream) {
  return diral_env_prefill_mode(e, DIRAL_STEP_DESIGN, actions, slots, seed, states_out, out_dtype, actions_all_out,
                                actions_next_out, rew_in, episode, epsilon, stream);
}

int diral_env_observe(DiralEnv* e, const int32_t* actions, const double* chobs_in, const double* rew_in,
                      void* state_out, int out_dtype, double episode, double epsilon, void* stream) {
  if (!e || !actions || !state_out) return DIRAL_ERR_BAD_ARG;
  if (out_dtype != DIRAL_F32 && out_dtype != DIRAL_F64) return DIRAL_ERR_BAD_ARG;
  if (e->S == 0) return DIRAL_OK;
  DEVICE_ENTER(e->device);
  hipStream_t s = (hipStream_t)stream;
  StepParams p = call_params(e, kModeObserve, 0, actions, state_out, out_dtype, episode, epsilon);
  p.chobs_in = chobs_in; p.rew_in = rew_in;
  if (e->kernel_path == DIRAL_PATH_GENERAL || runs_large(e)) HIP_TRY(e, launch_step_any(e, p, plan_step(e, p, nullptr), s));   // (tests: the general kernel's observe mode; step_large.hpp's)
  else HIP_TRY(e, launch_observe_any(e, p, s));
  HIP_TRY(e, launch_posdist_if_needed(e, p, s));
  if (e->prev_obs && e->off_chobs_pb >= 0) {                    // `obs` = piggy_obs, A * A values per agent
    const size_t total = (size_t)e->B * e->N * e->A * e->A;
    HIP_TRY(e, launch_1d<piggy_fill_kernel>(total, s, piggy_params(e, p), total));
  }
  return DIRAL_OK;
}

int diral_env_update_velocity(DiralEnv* e, const uint8_t* draws, uint64_t seed, void* stream) {
  if (!e) return DIRAL_ERR_BAD_ARG;
  if (!has(&e->cfg, DIRAL_F_MOBILITY_VARY)) return DIRAL_OK;   // test_env.py:503
  DEVICE_ENTER(e->device);
  const size_t bn = (size_t)e->B * e->N;
  HIP_TRY(e, launch_1d<velocity_kernel>(bn, (hipStream_t)stream, (int)bn, draws, seed, (uint64_t)e->env_offset * (uint64_t)e->N, e->vel));
  return DIRAL_OK;
}

int diral_env_sample(DiralEnv* e, int32_t* actions_out, uint64_t seed, void* stream) {
  if (!e || !actions_out) return DIRAL_ERR_BAD_ARG;
  DEVICE_ENTER(e->device);
  const size_t bn = (size_t)e->B * e->N;
  HIP_TRY(e, launch_1d<sample_kernel>(bn, (hipStream_t)stream, (int)bn, e->A, seed, (uint64_t)e->env_offset * (uint64_t)e->N, actions_out));
  return DIRAL_OK;
}

int diral_env_info_age(DiralEnv* e, int64_t t, int32_t* out, void* stream) {
  if (!e || !out) return DIRAL_ERR_BAD_ARG;
  if (!e->la) return DIRAL_ERR_BAD_CONFIG;
  DEVICE_ENTER(e->device);
  HIP_TRY(e, launch_k<info_age_kernel>(dim3(e->B), dim3(256), 0, (hipStream_t)stream, e->N, (long long)t, e->la, out));
  return DIRAL_OK;
}

int diral_env_export_state(DiralEnv* e, double* pos_x, double* pos_y, double* vel, int32_t* tab_seq,
                           int32_t* tab_age, double* tab_x, double* tab_y, int32_t* last_arrival, void* stream) {
  if (!e) return DIRAL_ERR_BAD_ARG;
  DEVICE_ENTER(e->device);
  hipStream_t s = (hipStream_t)stream;
  const size_t bn = (size_t)e->B * e->N;
  if (pos_x) HIP_TRY(e, hipMemcpyAsync(pos_x, e->pos_x, bn * 8, hipMemcpyDeviceToDevice, s));
  if (pos_y) HIP_TRY(e, hipMemcpyAsync(pos_y, e->pos_y, bn * 8, hipMemcpyDeviceToDevice, s));
  if (vel) HIP_TRY(e, hipMemcpyAsync(vel, e->vel, bn * 8, hipMemcpyDeviceToDevice, s));
  if (tab_seq || tab_age || tab_x || tab_y) {
    HIP_TRY(e, ensure_plane(e, s));                               // (sequence numbers and ages too: the packed table of N <= 64)
    HIP_TRY(e, launch_1d<export_tables_kernel>(bn * e->N, s, e->B, e->N, e->NV, e->NR, e->tkey, e->tx, e->pos_y, tab_seq, tab_age,
                                               tab_x, tab_y));
  }
  if (last_arrival) {
    if (!e->la) return DIRAL_ERR_BAD_CONFIG;
    HIP_TRY(e, hipMemcpyAsync(last_arrival, e->la, bn * e->N * 4, hipMemcpyDeviceToDevice, s));
  }
  return DIRAL_OK;
}

int diral_env_import_state(DiralEnv* e, const double* pos_x, const double* pos_y, const double* vel,
                           const int32_t* tab_seq, const int32_t* tab_age, const double* tab_x,
                           const int32_t* last_arrival, void* stream) {
  if (!e) return DIRAL_ERR_BAD_ARG;
  DEVICE_ENTER(e->device);
  hipStream_t s = (hipStream_t)stream;
  const size_t bn = (size_t)e->B * e->N;
  if (pos_x) HIP_TRY(e, hipMemcpyAsync(e->pos_x, pos_x, bn * 8, hipMemcpyDeviceToDevice, s));
  if (pos_y) {
    HIP_TRY(e, hipMemcpyAsync(e->pos_y, pos_y, bn * 8, hipMemcpyDeviceToDevice, s));
    if (refresh_flat_y(e, s) != DIRAL_OK) return DIRAL_ERR_HIP;
  }
  if (vel) HIP_TRY(e, hipMemcpyAsync(e->vel, vel, bn * 8, hipMemcpyDeviceToDevice, s));
  if (tab_seq || tab_age || tab_x) {
    HIP_TRY(e, ensure_plane(e, s));                             // (a partial import keeps the other planes)
    e->ring_valid = false;
    HIP_TRY(e, launch_1d<import_tables_kernel>(bn * e->N, s, e->B, e->N, e->NV, e->NR, tab_seq, tab_age, tab_x, e->tkey, e->tx, e->err));
    // the ring again, right away (not at the next step: a step sequence captured into a hipGraph must not
    // contain a rebuild from a plane that later replays find stale)
    if (e->ring) { HIP_TRY(e, ensure_ring(e, s)); HIP_TRY(e, verify_ring(e, s)); }
  }
  if (last_arrival) {
    if (!e->la) return DIRAL_ERR_BAD_CONFIG;
    HIP_TRY(e, hipMemcpyAsync(e->la, last_arrival, bn * e->N * 4, hipMemcpyDeviceToDevice, s));
  }
  return DIRAL_OK;
}

int diral_env_copy_envs(DiralEnv* dst, const int32_t* dst_index, DiralEnv* src, const int32_t* src_index, int32_t count,
                        void* stream) {
  if (!dst || !src || count < 1) return DIRAL_ERR_BAD_ARG;
  if ((!dst_index && count > dst->B) || (!src_index && count > src->B)) return DIRAL_ERR_BAD_ARG;
  if (dst->device != src->device) return DIRAL_ERR_UNSUPPORTED;
  if (std::memcmp(&dst->cfg, &src->cfg, sizeof(DiralCfg)) != 0) return DIRAL_ERR_BAD_CONFIG;
  std::vector<std::pair<char*, uint32_t>> from, to;
  if (!copy_slabs(src, from) || !copy_slabs(dst, to)) return DIRAL_ERR_UNSUPPORTED;
  if (from.size() != to.size()) return DIRAL_ERR_BAD_CONFIG;      // (a wide handle made under another DIRAL_TABLE_FORM)
  CopyPlan plan;
  std::memset(&plan, 0, sizeof(plan));
  for (size_t i = 0; i < from.size(); ++i) {
    if (from[i].second != to[i].second) return DIRAL_ERR_BAD_CONFIG;
    plan.slab[i] = {from[i].first, to[i].first, from[i].second, plan.units};
    plan.units += copy_units(from[i].second);
  }
  plan.slabs = (int32_t)from.size();
  DEVICE_ENTER(dst->device);
  hipStream_t s = (hipStream_t)stream;
  // Host flags only: behind the copy `dst` is valid in a form only if both handles were.  Where that would leave neither
  // form, both handles complete their planes first - the one launch this call ever adds (refused inside a capture).
  if (!(dst->plane_valid && src->plane_valid) && !(dst->ring_valid && src->ring_valid)) {
    for (DiralEnv* h : {dst, src}) {
      const hipError_t st = ensure_plane(h, s);
      if (st == hipSuccess) continue;
      if (h->capture_violation) { h->capture_violation = false; dst->capture_violation = true; }
      return note_hip(dst, st, "diral_env_copy_envs: ensure_plane");
    }
  }
  const uint32_t chunks = (plan.units + kCopyChunk - 1) / kCopyChunk;
  HIP_TRY(dst, launch_k<copy_envs_kernel>(dim3(chunks, (uint32_t)std::min(count, 65535)), dim3(kCopyThreads), 0, s, plan, src_index,
                                          dst_index, (int)count, src->B, dst->B, dst == src ? 1 : 0, dst->err));
  dst->plane_valid = dst->plane_valid && src->plane_valid;
  dst->ring_valid = dst->ring_valid && src->ring_valid;
  dst->flat_y = dst->flat_y && src->flat_y;                       // (the non-flat instantiations are correct for flat data)
  return DIRAL_OK;
}

int diral_env_reset_envs(DiralEnv* e, const int32_t* index, int32_t count, const uint8_t* mask, const double* x0,
                         const double* y0, const double* v0, uint64_t seed, void* stream) {
  if (!e || (index && mask)) return DIRAL_ERR_BAD_ARG;
  if (!mask && count < 1) return DIRAL_ERR_BAD_ARG;
  if (!mask && !index && count > e->B) return DIRAL_ERR_BAD_ARG;
  // the slabs of copy_slabs other than the positions, each with the fill byte of its `own`
  ResetPlan plan;
  std::memset(&plan, 0, sizeof(plan));
  for (const DevBuf& b : e->bufs) {
    if (!b.reset_bytes || b.p == e->slow) continue;
    if (plan.slabs == kCopyMaxSlabs) return DIRAL_ERR_UNSUPPORTED;   // (a bug in this file, as in copy_slabs)
    const uint32_t bytes = (uint32_t)(b.reset_bytes / (size_t)e->B);
    plan.slab[plan.slabs++] = {(char*)b.p, bytes, plan.units, 0x01010101u * (uint32_t)(b.fill & 0xFF)};
    plan.units += copy_units(bytes);
  }
  DEVICE_ENTER(e->device);
  hipStream_t s = (hipStream_t)stream;
  // y0: `flat_y` is recomputed on the host behind the launch, which a capture cannot hold - refused with nothing enqueued
  if (y0 && stream_is_capturing(s)) {
    e->last_hip_error = "diral_env_reset_envs: y0 needs a host read-back of the lanes, which cannot be part of a stream capture";
    return DIRAL_ERR_CAPTURE;
  }
  // Host flags stay as they are: an all-fill env is valid in the ring form and in the plane form alike (a fresh handle
  // has both), so whichever form is current for the other envs is current for the listed ones too.
  const int n = mask ? e->B : (int)count;
  const uint32_t chunks = std::max(1u, (plan.units + kCopyChunk - 1) / kCopyChunk);
  HIP_TRY(e, launch_k<reset_envs_kernel>(dim3(chunks, (uint32_t)std::min(n, 65535)), dim3(kCopyThreads), 0, s, plan, index, mask, n,
                                         e->B, e->N, e->cfg.highway_length, has(&e->cfg, DIRAL_F_MOBILITY_VARY) ? 1 : 0, seed,
                                         (uint64_t)e->env_offset * (uint64_t)e->N, x0, y0, v0, e->pos_x, e->pos_y, e->vel, e->err));
  // without y0 the listed envs are on the lane: the flag stays true where it was, and where it was false the non-flat
  // instantiations are correct for flat data (as in diral_env_copy_envs)
  if (y0 && refresh_flat_y(e, s) != DIRAL_OK) return DIRAL_ERR_HIP;
  return DIRAL_OK;
}

int diral_env_export_prev_obs(DiralEnv* e, double* prev_obs, void* stream) {
  if (!e || !prev_obs) return DIRAL_ERR_BAD_ARG;
  if (!e->prev_obs) return DIRAL_ERR_BAD_CONFIG;
  DEVICE_ENTER(e->device);
  HIP_TRY(e, hipMemcpyAsync(prev_obs, e->prev_obs, (size_t)e->B * e->N * e->A * 8, hipMemcpyDeviceToDevice, (hipStream_t)stream));
  return DIRAL_OK;
}

int diral_env_import_prev_obs(DiralEnv* e, const double* prev_obs, void* stream) {
  if (!e || !prev_obs) return DIRAL_ERR_BAD_ARG;
  if (!e->prev_obs) return DIRAL_ERR_BAD_CONFIG;
  DEVICE_ENTER(e->device);
  HIP_TRY(e, hipMemcpyAsync(e->prev_obs, prev_obs, (size_t)e->B * e->N * e->A * 8, hipMemcpyDeviceToDevice, (hipStream_t)stream));
  return DIRAL_OK;
}

int diral_env_export_entries(DiralEnv* e, DiralNeighborEntry* entries, void* stream) {
  if (!e || !entries) return DIRAL_ERR_BAD_ARG;
  DEVICE_ENTER(e->device);
  hipStream_t s = (hipStream_t)stream;
  HIP_TRY(e, ensure_plane(e, s));
  HIP_TRY(e, launch_1d<export_entries_kernel>((size_t)e->B * e->N * e->N, s, e->B, e->N, e->NV, e->NR, e->tkey, e->tx, e->pos_y, entries));
  return DIRAL_OK;
}

int diral_env_import_entries(DiralEnv* e, const DiralNeighborEntry* entries, void* stream) {
  if (!e || !entries) return DIRAL_ERR_BAD_ARG;
  DEVICE_ENTER(e->device);
  hipStream_t s = (hipStream_t)stream;
  e->plane_valid = true;                                        // every entry of the plane is rewritten
  e->ring_valid = false;
  HIP_TRY(e, launch_1d<import_entries_kernel>((size_t)e->B * e->N * e->N, s, e->B, e->N, e->NV, e->NR, entries, e->tkey, e->tx, e->err));
  if (e->ring) { HIP_TRY(e, ensure_ring(e, s)); HIP_TRY(e, verify_ring(e, s)); }   // as in diral_env_import_state
  return DIRAL_OK;
}

int diral_env_set_trace(DiralEnv* e, const double* x_positions, int T, int per_env, void* stream) {
  if (!e || T < 0) return DIRAL_ERR_BAD_ARG;
  DEVICE_ENTER(e->device);
  hipStream_t s = (hipStream_t)stream;
  HIP_TRY(e, hipStreamSynchronize(s));               // no launch may still read the old copy
  if (e->trace) { (void)hipFree(e->trace); e->trace = nullptr; }
  e->trace_len = 0; e->trace_per_env = 0;
  // the step parameters stop pointing at the freed copy BEFORE anything below can fail
  e->base.trace = nullptr; e->base.trace_len = 0; e->base.trace_per_env = 0;
  if (x_positions && T > 0) {
    const size_t n = (size_t)(per_env ? e->B : 1) * T * e->N;
    double* fresh = nullptr;
    HIP_TRY(e, hipMalloc((void**)&fresh, n * 8));
    hipError_t st = hipMemcpyAsync(fresh, x_positions, n * 8, hipMemcpyDeviceToDevice, s);
    if (st == hipSuccess) st = hipStreamSynchronize(s);
    if (st != hipSuccess) { (void)hipFree(fresh); return note_hip(e, st, "diral_env_set_trace copy"); }
    e->trace = fresh;
    e->trace_len = T; e->trace_per_env = per_env ? 1 : 0;
  }
  e->base.trace = e->trace; e->base.trace_len = e->trace_len; e->base.trace_per_env = e->trace_per_env;
  return DIRAL_OK;
}

int diral_env_metrics(DiralEnv* e, double* out, int clear, void* stream) {
  if (!e) return DIRAL_ERR_BAD_ARG;
  DEVICE_ENTER(e->device);
  const int total = e->B * DIRAL_M_COLUMNS;
  HIP_TRY(e, launch_1d<metrics_kernel>((size_t)total, (hipStream_t)stream, total, e->metrics, out, clear));
  return DIRAL_OK;
}

#if defined(DIRAL_TIMING) || defined(DIRAL_DEBUG_XG)
// -DDIRAL_TIMING tuning builds only (profiles/phase_timing.py binds it by name); compiled out of the
// release library, so the release symbol table is exactly include/diral_env.h: copy the phase
// timestamps [B][waves][8] to a host buffer.
int diral_env_debug_timing(DiralEnv* e, unsigned long long* host_out, int waves) {
  if (!e || !e->dbg || !host_out) return DIRAL_ERR_BAD_ARG;
  DEVICE_ENTER(e->device);
  if (hipDeviceSynchronize() != hipSuccess) return DIRAL_ERR_HIP;
  if (hipMemcpy(host_out, e->dbg, (size_t)e->B * waves * 8 * 8, hipMemcpyDeviceToHost) != hipSuccess) return DIRAL_ERR_HIP;
  return DIRAL_OK;
}
#endif

int diral_env_set_clock(DiralEnv* e, const int64_t* t_dev) {
  if (!e) return DIRAL_ERR_BAD_ARG;
  e->base.t_dev = (const long long*)t_dev;
  return DIRAL_OK;
}

int diral_env_set_capture_rotation(DiralEnv* e, int on, int* phase) {
  if (!e) return DIRAL_ERR_BAD_ARG;
  e->capture_rotates = on != 0;
  if (phase) *phase = (int)(e->slow_launches % 3);
  return DIRAL_OK;
}

int diral_env_align_phase(DiralEnv* e, int phase, void* stream) {
  if (!e || phase < 0 || phase > 2) return DIRAL_ERR_BAD_ARG;
  if (!e->slow || (int)(e->slow_launches % 3) == phase) return DIRAL_OK;
  DEVICE_ENTER(e->device);
  hipStream_t s = (hipStream_t)stream;
  if (stream_is_capturing(s)) { e->capture_violation = true; return DIRAL_ERR_CAPTURE; }
  // the sets a launch of the new phase reads, builds and clears must not hold what launches of another phase left half
  // done (a cleared count under flags that still stand): all three empty = every env runs in dispatch order once
  if (hipMemsetAsync(e->slow, 0, buf_of(e, e->slow).bytes, s) != hipSuccess) return DIRAL_ERR_HIP;
  while ((int)(e->slow_launches % 3) != phase) ++e->slow_launches;
  return DIRAL_OK;
}

int diral_env_check(DiralEnv* e, void* stream) {
  if (!e) return DIRAL_ERR_BAD_ARG;
  DEVICE_ENTER(e->device);
  uint32_t flags = 0;
  HIP_TRY(e, hipMemcpyAsync(&flags, e->err, 4, hipMemcpyDeviceToHost, (hipStream_t)stream));
  HIP_TRY(e, hipStreamSynchronize((hipStream_t)stream));
  if (flags) HIP_TRY(e, hipMemsetAsync(e->err, 0, 4, (hipStream_t)stream));
  if (flags & kErrAction) return DIRAL_ERR_ACTION_RANGE;
  if (flags & kErrSeq) return DIRAL_ERR_SEQ_OVERFLOW;
  if (flags & kErrTable) return DIRAL_ERR_TABLE_CONFLICT;
  if (flags & kErrPiggy) return DIRAL_ERR_PIGGY_NO_TX;
  if (flags & kErrEnvIndex) return DIRAL_ERR_ENV_INDEX;
  return DIRAL_OK;
}

}  // extern "C"
