/*
 * diral_env.h - C-ABI of libdiral_env.so: the MI355X-native, batched V2V
 * resource-allocation environment step.
 *
 * The reference (gundoganalperen/DIRAL) has NO FFI/plugin layer: the env is a
 * duck-typed Python object (`TestEnv`, envs/test_env.py:6) that agents and the
 * driver call directly.  This header is the boundary a maintainer would bind
 * with ctypes to replace that object's hot path; every entry point names the
 * reference method(s) it replaces.  INTEGRATION.md shows the binding.
 *
 * Conventions
 *  - plain C: pointers + sizes, no C++/torch types.  Every data pointer is a
 *    DEVICE pointer (HBM) unless its name ends in `_host`.
 *  - `stream` is a hipStream_t passed as void* (NULL = default stream).  All
 *    entry points that take a stream only ENQUEUE work on it (no host sync, no
 *    allocation) - safe inside hipGraph capture.  Exceptions, which SYNCHRONISE
 *    the stream: diral_env_check, diral_env_set_trace, and diral_env_reset /
 *    diral_env_import_state when they are given y positions (the host keeps an
 *    "every y == 0" flag that selects the kernel instantiation).
 *  - every entry point runs with the handle's device current and restores the
 *    caller's current device before it returns.
 *  - B = parallel envs (independent episodes), N = num_users, A = num_channels,
 *    S = state_space.  Batched arrays are row-major [B][N], [B][N][A], [B][N][S].
 *  - return value: 0 = DIRAL_OK, <0 = DiralStatus error; diral_env_strerror().
 *  - a handle is bound to one device and is NOT thread-safe.
 */
#ifndef DIRAL_ENV_H
#define DIRAL_ENV_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DIRAL_ABI_VERSION 8

/* ---- status codes --------------------------------------------------------- */
typedef enum DiralStatus {
  DIRAL_OK = 0,
  DIRAL_ERR_BAD_ARG = -1,      /* null pointer, bad size, bad enum            */
  DIRAL_ERR_BAD_CONFIG = -2,   /* config the reference itself cannot run, or a
                                  combination this build rejects */
  DIRAL_ERR_UNSUPPORTED = -3,  /* valid reference config outside this build's
                                  limits (e.g. N > 256)                        */
  DIRAL_ERR_HIP = -4,          /* a HIP runtime call failed; see strerror      */
  DIRAL_ERR_NO_DEVICE = -5,    /* no gfx950 device / device index out of range */
  DIRAL_ERR_ACTION_RANGE = -6, /* an action outside [0, A) was seen (sticky flag
                                  raised by the step kernel; test_env.py:592)   */
  DIRAL_ERR_SEQ_OVERFLOW = -7, /* more than DIRAL_MAX_SLOTS steps since reset, or an
                                  imported sequence number outside [0, DIRAL_MAX_SLOTS]
                                  (sticky flag, reported once by diral_env_check; what
                                  the handle computes after it was raised is undefined
                                  until diral_env_reset)                         */
  DIRAL_ERR_CAPTURE = -8,      /* the call would launch a ring <-> plane conversion
                                  (first step after a kernel-path switch, export /
                                  observe after ring steps) while `stream` is being
                                  captured into a hipGraph: do it outside the capture */
  DIRAL_ERR_TABLE_CONFLICT = -9, /* imported tables: two entries about one subject carry
                                  the same sequence number but different xpos - no
                                  run of the reference produces that (an entry IS the
                                  subject's stamp at that number, vehicle.py:35-63);
                                  raised by diral_env_check after an import      */
  DIRAL_ERR_PIGGY_NO_TX = -10, /* State.piggybacking: a receiver found no transmitter in range
                                  on a used resource - the reference's `self.prev_obs[tx_id]`
                                  with tx_id None, a KeyError (test_env.py:243; sticky flag
                                  raised by the step, reported by diral_env_check)      */
  DIRAL_ERR_ENV_INDEX = -11    /* diral_env_copy_envs met an env index outside its handle (sticky flag on dst,
                                  reported by diral_env_check; that pair was skipped) */
} DiralStatus;

/* ---- config flags: the booleans of the `EnvironmentTest` YAML block -------- */
enum {
  DIRAL_F_MOBILITY          = 1u << 0,  /* mobility            test_env.py:14  */
  DIRAL_F_MOBILITY_VARY     = 1u << 1,  /* mobility_vary       test_env.py:15  */
  DIRAL_F_TOY_WEIGHTS       = 1u << 2,  /* congestion_test     test_env.py:48, network.py:284-290 */
  DIRAL_F_ADD_ACTION        = 1u << 3,  /* State.add_action    test_env.py:29  */
  DIRAL_F_ACTION_REAL       = 1u << 4,  /* State.action_index == "real" (else "binary") test_env.py:32 */
  DIRAL_F_ADD_CHANNEL_OBS   = 1u << 5,  /* State.add_channel_obs test_env.py:41 */
  DIRAL_F_ADD_REWARD        = 1u << 6,  /* State.add_reward    test_env.py:28  */
  DIRAL_F_ADD_INDEX         = 1u << 7,  /* State.add_index     test_env.py:30  */
  DIRAL_F_ADD_VELOCITY      = 1u << 8,  /* State.add_velocity  test_env.py:31  */
  DIRAL_F_ADD_POSITION      = 1u << 9,  /* State.add_position  test_env.py:34  */
  DIRAL_F_ADD_POSDIST       = 1u << 10, /* State.add_positional_dist test_env.py:35 */
  DIRAL_F_ADD_POSDIST_PIGGY = 1u << 11, /* State.add_positional_dist_piggy test_env.py:36 */
  DIRAL_F_FINGERPRINT       = 1u << 12, /* enable_fingerprint  test_env.py:19  */
  DIRAL_F_PROPORTIONAL_FAIR = 1u << 13, /* proportional_fair   test_env.py:22  */
  DIRAL_F_DESIGN_TOPOLOGY   = 1u << 14, /* enable_design_topology test_env.py:16 */
  DIRAL_F_PIGGYBACKING      = 1u << 15, /* State.piggybacking  test_env.py:33, 71-79, 241-254, 260-264: my_step returns,
                                           per agent, its observation with the previous observation of each resource's
                                           closest transmitter inserted (np.insert at the resource's index): A * A values.
                                           Needs State.type 2 and State.add_channel_obs (DIRAL_ERR_BAD_CONFIG otherwise:
                                           type 1 makes the vector's length depend on the slot's traffic, and without the
                                           channel-observation section obtain_state never reads what get_state_space()
                                           counts); my_step_ch / my_step_design return DIRAL_ERR_BAD_CONFIG on such a handle
                                           (they hand obtain_state the plain A-wide observation, test_env.py:316, 443) */
  /* build extensions (no reference counterpart) */
  DIRAL_F_TRACK_ARRIVAL     = 1u << 16, /* keep last_arrival_time[N][N] (network.py:39-42)
                                           so diral_env_info_age() works        */
  DIRAL_F_TRACK_PRR         = 1u << 17  /* accumulate PRR metrics in my_step too */
};

/* One env configuration = the `EnvironmentTest` block (test_env.py:12-48) plus
 * its nested `State` block (test_env.py:26-41) and the driver's
 * `episode_interval` (main_test.py:226). */
typedef struct DiralCfg {
  uint32_t struct_bytes;        /* = sizeof(DiralCfg); ABI guard               */
  uint32_t flags;               /* DIRAL_F_*                                   */
  int32_t  num_users;           /* N  test_env.py:12                           */
  int32_t  num_channels;        /* A  test_env.py:13 (= action space, :44)     */
  int32_t  num_bins;            /* K  State.num_bins test_env.py:40            */
  int32_t  reward_design;       /* 1..5  test_env.py:20                        */
  int32_t  state_type;          /* State.type 1|2  test_env.py:27              */
  int32_t  posdist_type;        /* State.add_positional_dist_type 1|2  :37     */
  int32_t  episode_interval;    /* main_test.py:226 (25); done = t%EI == EI-1  */
  int32_t  info_age_limit;      /* 20: table entry valid iff last_updated < 20 (network.py:547) */
  int32_t  pf_threshold;        /* 10  test_env.py:89                          */
  int32_t  reserved0;
  double   pf_penalty;          /* -10 test_env.py:90                          */
  double   highway_length;      /* L   test_env.py:18                          */
  double   highway_height;      /* 2   network.py:31                           */
  double   communication_range; /* Rc  test_env.py:21                          */
  double   bin_range;           /* Rb  test_env.py:24                          */
} DiralCfg;

/* which reference step function a diral_env_step() call replaces */
typedef enum DiralStepMode {
  DIRAL_STEP_MY_STEP = 0,   /* TestEnv.my_step         test_env.py:124-266 */
  DIRAL_STEP_MY_STEP_CH = 1,/* TestEnv.my_step_ch      test_env.py:351-443 */
  DIRAL_STEP_DESIGN = 2     /* TestEnv.my_step_design  test_env.py:269-349 */
} DiralStepMode;

/* element type of the floating-point OUTPUT buffers (state, reward, chobs).
 * The arithmetic is always float64, like the reference; F32 is a final cast. */
typedef enum DiralDType { DIRAL_F32 = 0, DIRAL_F64 = 1, DIRAL_F16 = 2, DIRAL_BF16 = 3 } DiralDType;   /* the 16-bit kinds: Q-values (DiralSelect::q_dtype, diral_td_head) and the memory's state outputs only */

/* limits of this build (the reference has none: TestEnv takes any N, A and State.num_bins, test_env.py:12-13, 40).
 * The specialised kernels (csrc/step_fast64.hpp, step_wide.hpp: every number bench.py reports) serve num_users <= 256
 * with num_channels <= 64; 64 < num_channels <= 256 at num_users <= 256 is stepped by the general kernel
 * (csrc/step_kernel.hpp: same results, bit for bit, 2.5-4 x the time).  Beyond num_users 256, num_channels 256 or
 * num_bins 64 the step runs as three launches with the tables' columns spread over the chip (csrc/step_large.hpp,
 * DIRAL_KERNEL_LARGE: same results, bit for bit) up to the sizes below - as long as the per-env working set fits a
 * workgroup's 160 KB of LDS (28 bytes per vehicle + 8 per resource: 4096 vehicles with 4096 resources do), else
 * DIRAL_ERR_UNSUPPORTED.  diral_env_last_kernel() says which kernel ran.  Not served: State.piggybacking beyond 256
 * resources (A * A values per agent), the type-1 histogram beyond ~1400 vehicles (DIRAL_ERR_UNSUPPORTED at create). */
#define DIRAL_MAX_USERS    4096
#define DIRAL_MAX_CHANNELS 4096
#define DIRAL_MAX_BINS     1024
#define DIRAL_SMALL_MAX_USERS    256   /* the one-workgroup kernels */
#define DIRAL_SMALL_MAX_CHANNELS 256
#define DIRAL_SMALL_MAX_BINS     64
#define DIRAL_SUBWAVE_MAX_USERS    8    /* the sub-wave step kernel (csrc/step_subwave.hpp, DIRAL_PATH_SUBWAVE): 4 or 8 */
#define DIRAL_SUBWAVE_MAX_CHANNELS 16   /* lanes per env; num_bins <= DIRAL_SMALL_MAX_BINS                              */
#define DIRAL_MAX_SLOTS    16777214   /* steps between resets (24-bit sequence numbers) */

/* per-env episode metric columns written by diral_env_metrics() */
enum {
  DIRAL_M_SLOTS = 0,        /* steps taken since reset/clear                    */
  DIRAL_M_SUM_REWARD,       /* sum over slots and agents of reward              */
  DIRAL_M_TX_SOLE,          /* #transmissions alone on their resource           */
  DIRAL_M_TX_COLLIDED,      /* #transmissions sharing their resource            */
  DIRAL_M_PRR_SUM,          /* sum over transmissions of R (test_env.py:402-405; 1 for a sole tx) */
  DIRAL_M_PRR_CNT,          /* #transmissions that R was summed over            */
  DIRAL_M_COLUMNS
};

typedef struct DiralEnv DiralEnv;   /* opaque handle */

/* ---- pure host helpers ----------------------------------------------------- */

/* Fill *cfg with the reference's defaults (test_env.py:12-48 kwargs.setdefault
 * values; State flags all off; episode_interval 25). */
void diral_cfg_defaults(DiralCfg* cfg);

/* Replaces TestEnv.get_state_space() (test_env.py:492; sizing :49-85).
 * Returns S >= 0, or a negative DiralStatus for an invalid config. */
int diral_env_state_space(const DiralCfg* cfg);

/* 0 if `cfg` can be run by this build, else the DiralStatus explaining why. */
int diral_env_validate(const DiralCfg* cfg);

/* Whether a handle of `cfg` can be pinned to the sub-wave step kernel (DIRAL_PATH_SUBWAVE below); needs no device.
 * DIRAL_OK; DIRAL_ERR_BAD_ARG for a NULL cfg; what diral_env_validate says for a config this build cannot run at all;
 * DIRAL_ERR_UNSUPPORTED for num_users > DIRAL_SUBWAVE_MAX_USERS, num_channels > DIRAL_SUBWAVE_MAX_CHANNELS,
 * num_bins > DIRAL_SMALL_MAX_BINS and State.piggybacking (DIRAL_F_PIGGYBACKING). */
int diral_env_subwave_ok(const DiralCfg* cfg);

const char* diral_env_strerror(int status);
int diral_env_abi_version(void);

/* ---- lifetime ---------------------------------------------------------------- */

/* Replaces TestEnv.__init__ -> Network.__init__ (test_env.py:7-107,
 * network.py:15-67) for B independent envs on HIP device `device`.
 * Allocates all persistent state in HBM; tables zeroed (vehicle.py:24-33).
 * Test hooks, read from the process environment ONCE here: DIRAL_NO_FAST64 /
 * DIRAL_NO_WIDE (the general kernel also for N <= 64 / N > 64),
 * DIRAL_TABLE_FORM=packed|plane (the table form for N > 64),
 * DIRAL_NO_SLOW_FIRST=1 (blocks = envs in order, no slow envs first),
 * DIRAL_WIDE_SLOW_FIRST=1 (step_wide's packed form at N <= 128 dispatches its
 * slow envs first), DIRAL_F32_MARGIN=<n> (N <= 64: 0 = no float32 screening of
 * the histogram bin, n > 0 = a band of at least n / 65536 bin widths). */
int diral_env_create(const DiralCfg* cfg, int batch, int device, DiralEnv** out);
int diral_env_destroy(DiralEnv* env);

/* bytes of HBM the handle owns (for sizing batches against 288 GB) */
int64_t diral_env_hbm_bytes(const DiralEnv* env);

/* ---- handle options ---------------------------------------------------------- */
typedef enum DiralOption {
  /* global index of this handle's env 0.  The reference draws topology, actions and
   * velocity changes from unseeded global RNGs (network.py:103-110, 214;
   * test_env.py:121); here every device draw is a pure function of (seed, global
   * env index, vehicle), so a batch sharded over several handles / GPUs (shard g
   * owning envs [offset_g, offset_g + B_g)) draws exactly what one handle holding
   * the whole batch draws with the same seed. */
  DIRAL_OPT_ENV_OFFSET = 1,
  /* DIRAL_PATH_AUTO (default): configurations the specialised kernels serve run on
   * them; DIRAL_PATH_GENERAL: always the general kernel (tests compare the two);
   * DIRAL_PATH_LARGE: always the three-launch form of csrc/step_large.hpp (tests run the
   * reference's fixtures through it; not with State.piggybacking's A * A section);
   * DIRAL_PATH_SUBWAVE: opt-in, toy-size envs only - every diral_env_step call runs csrc/step_subwave.hpp, 4 or 8 lanes
   * per env and 16 or 8 envs per wavefront, same results bit for bit.  Returns what diral_env_subwave_ok says for the
   * handle's config (DIRAL_ERR_UNSUPPORTED on a handle of the three-launch form too) and leaves the path as it was on
   * refusal.  On such a handle diral_env_observe stays the stand-alone observe kernel, a one-slot diral_env_step_policy
   * runs its three launches, and diral_env_rollout, diral_env_prefill and slots > 1 return DIRAL_ERR_UNSUPPORTED with
   * nothing launched (as on a handle pinned to the general kernel) - unless DIRAL_OPT_SUBWAVE_SLOTS is set, below.
   * Any other value: DIRAL_ERR_BAD_ARG. */
  DIRAL_OPT_KERNEL_PATH = 2,
  /* 0 (default) / 1; 1 only on a handle pinned to DIRAL_PATH_SUBWAVE (else DIRAL_ERR_UNSUPPORTED), cleared by setting
   * any other kernel path; any other value: DIRAL_ERR_BAD_ARG.  While it is set, diral_env_rollout (any slots >= 1,
   * my_step and my_step_ch, states last / all / none) and diral_env_prefill / diral_env_prefill_mode (my_step_design and
   * my_step_ch) run as ONE launch of csrc/step_subwave_slots.hpp: the env's tables, positions, velocities and counters
   * stay in registers from slot to slot; same results as the loop of one-slot calls, bit for bit;
   * diral_env_last_kernel says DIRAL_KERNEL_SUBWAVE | DIRAL_KERNEL_POLICY.  The rollout takes every run-time switch of
   * the one-slot kernel (reward_design 1-5, proportional fairness, PRR metrics, static topology, no tables, off-lane
   * vehicles, the handle's trace, arrival stamps, the slot clock).  Still DIRAL_ERR_UNSUPPORTED, with nothing launched
   * and the env untouched: diral_env_step_policy with slots > 1 (a one-slot call keeps its three launches), the
   * information-age block (diral_env_rollout_ia), the replay / position-log block (diral_env_rollout_replay with a
   * non-empty block), a state vector with a secondary observation mode (sorted distances, type-1 histogram), and the
   * prefill on a handle with a trace or arrival stamps. */
  DIRAL_OPT_SUBWAVE_SLOTS = 3
} DiralOption;
enum { DIRAL_PATH_AUTO = 0, DIRAL_PATH_GENERAL = 1, DIRAL_PATH_LARGE = 2, DIRAL_PATH_SUBWAVE = 3 };
int diral_env_set_option(DiralEnv* env, int option, int64_t value);

/* which kernel the last diral_env_step / diral_env_observe call launched:
 * DIRAL_KERNEL_GENERAL, or DIRAL_KERNEL_FAST64 / DIRAL_KERNEL_WIDE or'ed with the
 * instantiation bits; negative before the first call. */
enum {
  DIRAL_KERNEL_GENERAL = 0,   /* csrc/step_kernel.hpp  */
  DIRAL_KERNEL_FAST64  = 1,   /* csrc/step_fast64.hpp, N <= 64       */
  DIRAL_KERNEL_WIDE    = 2,   /* csrc/step_wide.hpp,  64 < N <= 256  */
  DIRAL_KERNEL_OBSERVE = 3,   /* csrc/observe_kernel.hpp: diral_env_observe (stand-alone obtain_state) */
  DIRAL_KERNEL_LARGE   = 4,   /* csrc/step_large.hpp: N > 256, A > 256 or K > 64 (step and observe) */
  DIRAL_KERNEL_SUBWAVE = 5,   /* csrc/step_subwave.hpp: N <= 8 on a handle pinned to DIRAL_PATH_SUBWAVE (no instantiation bits) */
  DIRAL_KERNEL_RICH    = 16,  /* channel-obs output / cheap State flags (csrc/rich_out.hpp) */
  DIRAL_KERNEL_EXTRA   = 32,  /* my_step_design / arrival stamps / trace replay */
  DIRAL_KERNEL_CH      = 64,  /* my_step_ch */
  DIRAL_KERNEL_RING    = 128, /* the xpos ring (the per-entry xpos plane only for old entries) */
  DIRAL_KERNEL_PACKED  = 256, /* the packed table form: thermometer codes + ages + own sequence numbers (N <= 64 always;
                                 128 < N <= 256 on dense topologies), else the (seq, age) plane */
  DIRAL_KERNEL_POLICY  = 512  /* diral_env_step_policy ran as ONE launch (reward shaping + SPS decision in the step);
                                 DIRAL_KERNEL_SUBWAVE | DIRAL_KERNEL_POLICY: csrc/step_subwave_slots.hpp (DIRAL_OPT_SUBWAVE_SLOTS) */
};
int diral_env_last_kernel(const DiralEnv* env);

/* ---- topology / reset ------------------------------------------------------- */

/* Replaces Network.initialize_mobility_topology (network.py:92-119) /
 * reset_positions (network.py:181-187).  x0,y0,v0: [B][N] float64 device
 * arrays; any may be NULL => drawn on device from `seed`
 * (x0 integer-uniform in [0,L), y0 = 0, v0 ~ U(1.1,2.7) or 1.7 if
 * mobility_vary).  Zeroes tables, arrival stamps, pf counters and metrics. */
int diral_env_reset(DiralEnv* env, const double* x0, const double* y0,
                    const double* v0, uint64_t seed, void* stream);

/* ---- the hot path ----------------------------------------------------------- */

/* One time-slot for all B envs in ONE fused launch.  Replaces, per env,
 *   my_step / my_step_ch / my_step_design (per `mode`) followed by
 *   obtain_state(obs, actions, rewards, episode, epsilon) (test_env.py:527-583).
 * actions   [B][N] int32 in [0,A)
 * t         the driver's time_step (used for `done`, arrival stamps)
 * state_out [B][N][S] (dtype `out_dtype`), NULL => observation not built
 * rew_out   [B][N]    (dtype `out_dtype`), NULL allowed
 * done_out  [B] uint8, NULL allowed: t % episode_interval == episode_interval-1
 * chobs_out [B][N][A] (dtype `out_dtype`), NULL allowed: the `obs` dict of the
 *           reference step (test_env.py:143, 206, 228, 240).  With DIRAL_F_PIGGYBACKING
 *           [B][N][A * A]: the `piggy_obs` dict my_step returns instead (test_env.py:263-264),
 *           and the env keeps this slot's plain observation as the next slot's `prev_obs`
 *           (test_env.py:260-261)
 * episode, epsilon: only used with DIRAL_F_FINGERPRINT (test_env.py:577-579) */
int diral_env_step(DiralEnv* env, int mode, const int32_t* actions, int64_t t,
                   void* state_out, void* rew_out, uint8_t* done_out,
                   void* chobs_out, int out_dtype, double episode,
                   double epsilon, void* stream);

/* Observation only, no state change: replaces a stand-alone
 * TestEnv.obtain_state(obs, acts, rewards, episode, eps) (test_env.py:527-583)
 * on the CURRENT tables/positions.  chobs_in [B][N][A] ([B][N][A * A] with
 * DIRAL_F_PIGGYBACKING) and rew_in [B][N] are float64 device arrays (NULL allowed
 * when the State flags do not use them). */
int diral_env_observe(DiralEnv* env, const int32_t* actions,
                      const double* chobs_in, const double* rew_in,
                      void* state_out, int out_dtype, double episode,
                      double epsilon, void* stream);

/* Replaces TestEnv.update_velocity -> Network.update_velocity
 * (test_env.py:498-504, network.py:208-223).  draws [B][N] uint8 in {1,2,3}
 * (random.randrange(1,4)); NULL => drawn on device from `seed`.
 * No-op unless DIRAL_F_MOBILITY_VARY. */
int diral_env_update_velocity(DiralEnv* env, const uint8_t* draws,
                              uint64_t seed, void* stream);

/* Replaces TestEnv.sample (test_env.py:116-122): uniform actions [B][N]. */
int diral_env_sample(DiralEnv* env, int32_t* actions_out, uint64_t seed,
                     void* stream);

/* Replaces Network.get_information_age(t) (network.py:560-574):
 * out [B][100] int32.  Needs DIRAL_F_TRACK_ARRIVAL. */
int diral_env_info_age(DiralEnv* env, int64_t t, int32_t* out, void* stream);

/* Replaces Network.load_x_positions + the replay branch of update_positions
 * (network.py:171-178, 194-199; TestEnv.load_saved_positions, test_env.py:109-114):
 * after each step pos_x[u] = x_positions[t % T][u] instead of the velocity move.
 * x_positions: float64 device array [T][N] (per_env == 0, shared by all envs, the
 * reference's shape) or [B][T][N] (per_env != 0).  The trace is COPIED into
 * handle-owned HBM (synchronises `stream`); T == 0 or NULL removes it. */
int diral_env_set_trace(DiralEnv* env, const double* x_positions, int T, int per_env, void* stream);

/* ---- state export / import (checkpoint, golden replay, debugging) --------- */

/* Reference-shaped copies of the env state, all device pointers, any NULL
 * skipped.  pos_x,pos_y,vel [B][N] f64; tab_seq, tab_age [B][N][N] int32 and
 * tab_x, tab_y [B][N][N] f64 indexed [env][viewer][subject]
 * (Vehicle.pos_of_neighbors, vehicle.py:20-33; age saturates at 255);
 * last_arrival [B][N][N] int32 indexed [env][tx][rx] (network.py:39-42).
 * Imported tables must be states the reference can reach in this one respect:
 * entries about one subject that carry equal sequence numbers carry equal xpos
 * (an entry IS the subject's stamp at that number, vehicle.py:56-63; every
 * exported state qualifies).  The kernels build on it: N <= 64 keeps the xpos of
 * entries at most 7 stamps old in a per-subject ring instead of the per-entry
 * plane, N > 64 routes xpos through a rank-indexed table; export / observe /
 * other consumers see the plane completed first (no caller-visible difference).
 * An import that violates the requirement is detected: the next
 * diral_env_check() returns DIRAL_ERR_TABLE_CONFLICT.  So is a sequence number
 * the 24-bit table words cannot carry: tab_seq outside [0, DIRAL_MAX_SLOTS]
 * (negative ones included) is never truncated into a legal-looking number; the
 * next diral_env_check() returns DIRAL_ERR_SEQ_OVERFLOW, and the handle's outputs
 * are undefined until diral_env_reset.  A call that needs the
 * plane <-> ring conversion launch (the first step after a kernel-path switch,
 * export / observe after ring steps) while `stream` is being captured into a
 * hipGraph returns DIRAL_ERR_CAPTURE and launches nothing: a captured
 * conversion would replay against tables it no longer describes. */
int diral_env_export_state(DiralEnv* env, double* pos_x, double* pos_y,
                           double* vel, int32_t* tab_seq, int32_t* tab_age,
                           double* tab_x, double* tab_y, int32_t* last_arrival,
                           void* stream);
int diral_env_import_state(DiralEnv* env, const double* pos_x,
                           const double* pos_y, const double* vel,
                           const int32_t* tab_seq, const int32_t* tab_age,
                           const double* tab_x, const int32_t* last_arrival,
                           void* stream);

/* DIRAL_F_PIGGYBACKING: TestEnv.prev_obs (test_env.py:76-79, 260-261), the plain channel
 * observation of the last my_step, [B][N][A] float64 device arrays; zeros after a reset.
 * Handles without the flag return DIRAL_ERR_BAD_CONFIG. */
int diral_env_export_prev_obs(DiralEnv* env, double* prev_obs, void* stream);
int diral_env_import_prev_obs(DiralEnv* env, const double* prev_obs, void* stream);

/* The same tables as 16-byte records in the field order of the RealNeS bridge's
 * MA_NeighborTableEntry message (envs/ma_messages_pb2.py:195-230: float pos_x,
 * float pos_y, int32 seq_num, int32 last_update - what
 * realness_bridge.py:168-191 unpacks into the pos_of_neighbors dict the
 * observation code reads).  entries [B][N][N] device records indexed
 * [env][viewer][subject].  export narrows the f64 positions to f32 (round to
 * nearest); import widens pos_x exactly, ignores pos_y (an entry's ypos is the
 * subject's lane) and saturates last_update at 255 like
 * diral_env_import_state, whose reachability note and range of seq_num
 * ([0, DIRAL_MAX_SLOTS], else DIRAL_ERR_SEQ_OVERFLOW at the next check) apply. */
typedef struct DiralNeighborEntry {
  float pos_x, pos_y;
  int32_t seq_num, last_update;
} DiralNeighborEntry;
int diral_env_export_entries(DiralEnv* env, DiralNeighborEntry* entries, void* stream);
int diral_env_import_entries(DiralEnv* env, const DiralNeighborEntry* entries, void* stream);

/* ---- env copies between handles: fork, snapshot / restore, the candidates of a search --------------
 * (additive within ABI 8; csrc/copy_envs_kernel.hpp)
 *   for i in [0, count):  env dst_index[i] of `dst`  :=  env src_index[i] of `src`     (a NULL index array = i)
 * as ONE gather launch over the handles' own storage - no conversion to the reference-shaped planes of
 * diral_env_export_state / diral_env_import_state, no launch per buffer.  dst_index / src_index: [count] int32 device
 * arrays.  Only ENQUEUES: no host synchronisation, no allocation.
 *   What "an env" is: everything a later call can observe of it - positions and velocities; the tables in every stored
 *     form the handle has (the (seq, age) plane and the xpos plane, the xpos ring, the packed codes / ages / own sequence
 *     numbers / old-quad flags), whole slabs whichever form is current; arrival stamps (DIRAL_F_TRACK_ARRIVAL), the
 *     proportional-fair counters, the metric sums, prev_obs (DIRAL_F_PIGGYBACKING).  i.e. the positions plus whatever
 *     diral_env_reset refills, except the slow-first sets (a dispatch-order hint; no result depends on them).
 *   What does NOT travel, being the handle's and not the env's: the slot number `t` of the caller, the replay trace, the
 *     env offset, the device clock, the options.  Device random draws are a function of the GLOBAL env index, so a copied
 *     env draws what its new position draws; arrival stamps stay in the source's slot numbering.
 *   The two handles must be on one device (else DIRAL_ERR_UNSUPPORTED), have byte-equal DiralCfg and own the same set of
 *     state buffers (else DIRAL_ERR_BAD_CONFIG: e.g. a wide handle created under another DIRAL_TABLE_FORM).  Batch sizes
 *     and kernel paths may differ.
 *   DIRAL_ERR_BAD_ARG, checked first and without touching a device: a NULL handle; count < 1; a NULL index array with
 *     count larger than THAT handle's B.
 *   dst == src is allowed: the caller promises that no env is both read and written by different pairs; a pair with
 *     equal indices is skipped.  Broadcasting env b over a handle: src_index = [b] * B, dst_index = NULL.
 *   Duplicate entries in dst_index: which pair wins is unspecified.
 *   An index outside [0, B) of its handle: that pair is skipped, the others are copied, and the sticky flag behind
 *     DIRAL_ERR_ENV_INDEX is raised on `dst` (diral_env_check).
 *   Table forms: the validity of ring and plane is a pair of HOST flags per handle; behind the copy `dst` is valid in a
 *     form only if both handles were.  Where that would leave neither form (one handle last stepped on the ring, the
 *     other on another kernel path), both handles complete their planes first: the only launch the call ever adds,
 *     and - like every such conversion - refused inside a stream capture with DIRAL_ERR_CAPTURE and nothing copied.
 *     Likewise `dst` keeps its "every y == 0" flag only if `src` has it.
 *   A CAPTURED copy bakes the host flags of capture time into the graph: replay it only while both handles are in the
 *     forms (ring / plane validity, flat y) they had when it was captured. */
int diral_env_copy_envs(DiralEnv* dst, const int32_t* dst_index, DiralEnv* src, const int32_t* src_index,
                        int32_t count, void* stream);

/* ---- reset of a chosen subset of envs: index list or device mask --------------------------------------
 * (additive within ABI 8; csrc/reset_envs_kernel.hpp)
 * Every listed env b ends with exactly what diral_env_reset(env, x0, y0, v0, seed) leaves in env b of this handle; every
 * other env is untouched.  ONE fill-and-draw launch over the listed envs' slabs in their stored form.
 *   Which envs: `index` - a device array of `count` >= 1 env indices; or `mask` - a device array [B] of bytes, non-zero =
 *     reset this env (`count` is ignored); or neither: envs 0 ... count - 1 (count <= B), as diral_env_copy_envs reads a
 *     NULL index.
 *   What a listed env gets: every slab diral_env_copy_envs moves, other than the positions, filled as at create (zero; the
 *     arrival stamps -1) - tables in every stored form, arrival stamps, proportional-fair counters, metric sums, prev_obs;
 *     pos_x / pos_y / vel from ROW b of x0 / y0 / v0 ([B][N] float64 device arrays indexed by env as in diral_env_reset;
 *     only the listed rows are read), a NULL one from the device draws of diral_env_reset at the env's global index.
 *   What it leaves alone: the slow-first sets (a dispatch-order hint), the validity of ring and plane (an all-fill env is
 *     valid in both forms), the error flags, trace, clock, env offset, options.  The "every y == 0" flag is recomputed as
 *     in diral_env_reset when y0 is given - that reads back to the host, so inside a stream capture the call returns
 *     DIRAL_ERR_CAPTURE with nothing enqueued; without y0 the listed envs get y = 0, the flag stays as it was, and the
 *     call only ENQUEUES: no host synchronisation, no allocation, capturable (a replay reads index / mask again).
 *   DIRAL_ERR_BAD_ARG, checked first and without touching a device: a NULL handle; `index` and `mask` both given;
 *     count < 1 without a mask; a NULL index with count larger than B.
 *   An index outside [0, B): that env is skipped, the others are reset, and the sticky flag behind DIRAL_ERR_ENV_INDEX
 *     is raised (diral_env_check).  Duplicate indices are allowed: every writer stores the same values. */
int diral_env_reset_envs(DiralEnv* env, const int32_t* index, int32_t count, const uint8_t* mask,
                         const double* x0, const double* y0, const double* v0, uint64_t seed, void* stream);

/* ---- metrics ------------------------------------------------------------------ */

/* out [B][DIRAL_M_COLUMNS] float64 device array; clear != 0 zeroes the
 * accumulators afterwards. */
int diral_env_metrics(DiralEnv* env, double* out, int clear, void* stream);

/* Sticky device-side error flags (action range, sequence overflow, piggybacking without a transmitter, an env index
 * outside its handle in diral_env_copy_envs / diral_env_reset_envs) raised by
 * kernels since the last call.  SYNCHRONISES `stream`.  Returns DIRAL_OK or the
 * first error. */
int diral_env_check(DiralEnv* env, void* stream);

/* ---- the driver's reward post-processing (main_test.py:150-206) ----------------- */

/* What `marl_test` does to the rewards of one slot between `env.my_step*` and
 * `memory.add`, for `envs` envs in ONE launch (stateless: the caller owns the counters):
 *   sum_r      = np.sum(reward) in NumPy's pairwise order (:171), collision = A - sum_r (:178)
 *   ia_sum     = utils/misc.calculate_ia_penalty(ia) = sum (i+1)*ia[i]      (:151; ia [envs][100] or NULL)
 *   ia_penalty = -1 / +1 / 0 as ia_sum rose / fell / stayed vs *sum_ia_prev  (:153-160; flags bit 1)
 *   reward'    = reward + ia_penalty (:190-192); counter penalty: an agent that repeats an
 *                unsuccessful action (reward' < 1) more than `ia_penalty_threshold` times gets
 *                `ia_penalty_value` (:194-203; flags bit 2; pen_counter, prev_actions [envs][N] in/out);
 *                + sum_r / N (global_reward_avg, :205-206; flags bit 0)
 * reward_in / reward_out / sum_r_out / collision_out: `dtype` (arithmetic in that type, like the
 * torch statement diral_amd/driver.py keeps for the CPU-backed tests; float64 = the reference's).
 * Any output pointer may be NULL except reward_out. */
int diral_driver_shape(int envs, int num_users, int num_channels, const void* reward_in, int dtype,
                       const int32_t* actions, const int32_t* ia, int64_t* sum_ia_prev, int32_t* pen_counter,
                       int32_t* prev_actions, int flags, int ia_penalty_threshold, double ia_penalty_value,
                       void* reward_out, void* sum_r_out, void* collision_out, int64_t* ia_sum_out,
                       int32_t* ia_penalty_out, void* stream);

/* ---- SPS baseline policy (agent side, stateless entry points) ----------------- */

/* Replaces SemiPersistentScheduling.step + choose_new_resource
 * (algorithms/v2x_sps.py:76-104, 24-74) for `agents` independent agents in one
 * launch.  selection_window [agents][A] float64: the averaged-RSSI vector each
 * agent senses (lower = better); prev_action, counter [agents] int32: the
 * per-agent state (self.prev_action, self.reselection_counter), updated in place;
 * actions_out [agents] int32.  The reference draws from Python's global RNG; here
 * every draw is injectable (NULL => counter-based device RNG from `seed`):
 *   draw_counter [agents] int32 in [5,16]   random.randint(5, 16)      (v2x_sps.py:91)
 *   draw_keep    [agents] float64 in [0,1)  random.random()           (v2x_sps.py:93)
 *   draw_choice  [agents] int32 >= 0        random.choice(sB) = sB[draw % len(sB)] (v2x_sps.py:57)
 * rssi_threshold, inc_db (3), keep_prob (0.8): v2x_sps.py:12,18,22. */
int diral_sps_step(int agents, int num_channels, const double* selection_window, int32_t* prev_action,
                   int32_t* counter, double rssi_threshold, double inc_db, double keep_prob,
                   const int32_t* draw_counter, const double* draw_keep, const int32_t* draw_choice,
                   uint64_t seed, int32_t* actions_out, void* stream);

/* Build extension - the reference never wires its SPS agent to the toy env, so the map from
 * the env's channel observation to the "averaged RSSI" window SPS consumes is this build's:
 * window[a][i] = -60 on the agent's own resource (actions[a] == i); else from
 * d = chobs[a][i] (test_env.py:206, 240; network.py:385): d >= 100000 (busy, nobody in
 * range) -> -160; d > 0 -> -40 - 30 log10(max(d, 1)) (log-distance path loss, dB);
 * d == 0 (idle) -> -200.  chobs [agents][A] of `chobs_dtype`, window_out [agents][A] f64. */
int diral_sps_window_from_chobs(int agents, int num_channels, const void* chobs, int chobs_dtype,
                                const int32_t* actions, double* window_out, void* stream);

/* diral_sps_window_from_chobs + diral_sps_step in ONE launch (same decisions, bit for bit):
 * only the agents that re-select this slot build their window, in private memory.
 * num_channels <= 64, else DIRAL_ERR_UNSUPPORTED (use the two calls). */
int diral_sps_step_chobs(int agents, int num_channels, const void* chobs, int chobs_dtype,
                         const int32_t* actions, int32_t* prev_action, int32_t* counter,
                         double rssi_threshold, double inc_db, double keep_prob,
                         const int32_t* draw_counter, const double* draw_keep,
                         const int32_t* draw_choice, uint64_t seed, int32_t* actions_out, void* stream);

/* ---- the closed loop of a policy-only rollout as ONE launch per slot -----------------------------
 * The reference's slot is env step -> reward shaping -> policy (main_test.py:127-206 with algorithms/v2x_sps.py as the
 * policy); diral_env_step + diral_driver_shape + diral_sps_step_chobs are three dependent launches and the channel
 * observation travels through HBM between the first and the third.  diral_env_step_policy runs the same slot as one
 * launch where the configuration allows (N <= 64 on the one-lane highway, my_step, none of the run-time extras: the
 * channel observation is staged in LDS by the step and the agents decide from there), and as the three launches
 * otherwise (then `chobs_out` must be given) - same results either way, bit for bit:
 *   shaped_out / sum_r_out / collision_out, pen_*: diral_driver_shape without the information-age terms
 *     (shape_flags: bit 0 global_reward_avg, bit 2 stuck-action penalty); shaped_out NULL = no shaping;
 *   sps_*, draws, seed: diral_sps_step_chobs (seed_clock != NULL: diral_sps_step_chobs_clocked, injected draws ignored
 *     there too); actions_out [B][N]: the actions of the NEXT slot.
 * `chobs_out` may be NULL when the slot runs fused: the observation then never leaves the chip. */
typedef struct DiralSlotPolicy {
  uint32_t struct_bytes;          /* = sizeof(DiralSlotPolicy) */
  int32_t  shape_flags;
  int32_t  pen_threshold;
  int32_t  reserved0;
  double   pen_value;
  void*    shaped_out;            /* [B][N] out dtype or NULL */
  void*    sum_r_out;             /* [B] or NULL */
  void*    collision_out;         /* [B] or NULL */
  int32_t* pen_counter;           /* [B][N] (shape_flags bit 2) */
  int32_t* pen_prev_actions;      /* [B][N] */
  int32_t* sps_prev_action;       /* [B][N] */
  int32_t* sps_counter;           /* [B][N] */
  double   rssi_threshold, inc_db, keep_prob;
  const int32_t* draw_counter;    /* [B][N] or NULL */
  const double*  draw_keep;
  const int32_t* draw_choice;
  uint64_t seed;
  const int64_t* seed_clock;      /* NULL, or a device counter added to the seed */
  int32_t* actions_out;           /* [B][N] */
  /* K slots in ONE launch (ABI 6).  slots <= 1: one slot, as above.  slots = K > 1 (configurations the fused kernels take -
   * N <= 256 vehicles, my_step, the flat highway, A <= 64, none of the run-time extras (arrival stamps - but see
   * diral_env_step_policy_ia -, trace replay, PRR
   * tracking, static topologies, handles without piggybacked tables), no State.piggybacking; at 8 <= N <= 64 also
   * my_step_ch (DIRAL_STEP_MY_STEP_CH with reward_design 2, 3 or 4: the PRR reward and the PRR metric columns every slot;
   * a ONE-slot call in that mode stays three launches, and 64 < N <= 256 refuses it); otherwise
   * DIRAL_ERR_UNSUPPORTED with nothing launched): the workgroup of an env runs K slots of [env step -> shaping -> SPS
   * decision] back to back (N <= 64 keeps the env on the chip; 64 < N <= 256 leaves its tables in HBM / L2 between
   * slots, as a one-slot launch does), `actions` being slot 0's and the policy's
   * decisions the later ones'.  Equal, bit for bit, to K one-slot calls with t, t + 1, ... and seed, seed + 1, ... (plus
   * diral_env_update_velocity(env, NULL, vel_seed + slot / episode_interval) behind every slot that ends an episode, when
   * the config has mobility_vary) - tables, positions, velocities, metrics, policy state, actions_out (the actions of
   * slot t + K).  state_out / rew_out / done_out / chobs_out: of the LAST slot (each may be NULL; without state_out no
   * slot computes the positional histogram); shaped_out / sum_r_out / collision_out: [K][...] arrays, slot-major.
   * Injected draws (draw_*) must be NULL. */
  int32_t  slots;
  int32_t  reserved1;
  uint64_t vel_seed;
} DiralSlotPolicy;
int diral_env_step_policy(DiralEnv* env, int mode, const int32_t* actions, int64_t t, void* state_out, void* rew_out,
                          uint8_t* done_out, void* chobs_out, int out_dtype, const DiralSlotPolicy* policy,
                          void* stream);

/* The driver's random prefill (main_test.py:99-114) as ONE launch of K slots (ABI 8; step_fast64_slots_kernel):
 *   for k = 0 .. K - 1:   a_k = (k == 0) ? actions : TestEnv.sample()          [diral_env_sample(env, ., seed + k, .)]
 *                         obs, _ = my_step_design(a_k, 0)                        [test_env.py:269-349]
 *                         states_out[k] = obtain_state(obs, a_k, rews)           [rews = rew_in: the bootstrap step's, :110]
 * with the env kept on the chip from slot to slot.  Equal, bit for bit, to that loop of diral_env_sample +
 * diral_env_step(DIRAL_STEP_DESIGN) + diral_env_observe calls: states, tables, positions, metrics.
 *   actions [B][N]            slot 0's actions (e.g. diral_env_sample(env, actions, seed, stream))
 *   states_out [K][B][N][S]   out dtype, or NULL (no state is built)
 *   actions_all_out [K][B][N] a_k, or NULL          actions_next_out [B][N]  the draw of seed + K (mandatory: what the
 *                                                    next call passes as `actions`, with seed + K)
 *   rew_in [B][N] float64     the reward column of the state vectors (State.add_reward), or NULL: each slot's own reward
 * Configurations the fused kernel takes - N <= 64 (>= 8), A <= 64, the one-lane highway, piggybacked tables, no arrival /
 * PRR tracking, no trace replay, no secondary observation mode; otherwise DIRAL_ERR_UNSUPPORTED with nothing launched
 * (loop over the three calls instead: diral_amd.driver.DriverLoop.prefill does).  Toy-size envs (N <= 8): on a handle pinned
 * to DIRAL_PATH_SUBWAVE with DIRAL_OPT_SUBWAVE_SLOTS, in both modes below; not on a handle with a trace or arrival stamps. */
int diral_env_prefill(DiralEnv* env, const int32_t* actions, int32_t slots, uint64_t seed, void* states_out, int out_dtype,
                      int32_t* actions_all_out, int32_t* actions_next_out, const double* rew_in, double episode,
                      double epsilon, void* stream);
/* ... with the step the driver's branch calls (additive within ABI 8): `mode` = DIRAL_STEP_DESIGN is diral_env_prefill;
 * `mode` = DIRAL_STEP_MY_STEP_CH runs the `enable_channel` prefill of main_test.py:101-103 -
 *                         obs, _ = my_step_ch(a_k, 0)                            [test_env.py:351-443]
 * in place of my_step_design: every slot pays the PRR reward and adds to the PRR metric columns, the state rows take
 * `obs` (0 on the own or an idle resource, else 1) and `rew_in` as above.  Equal, bit for bit, to the loop of
 * diral_env_sample + diral_env_step(DIRAL_STEP_MY_STEP_CH) + diral_env_observe.  Any other mode: DIRAL_ERR_BAD_ARG;
 * my_step_ch with reward_design outside 2 ... 4: DIRAL_ERR_BAD_CONFIG (as diral_env_step); the configurations listed
 * above, vehicles off the lane, static topologies and State.piggybacking: DIRAL_ERR_UNSUPPORTED with nothing launched. */
int diral_env_prefill_mode(DiralEnv* env, int mode, const int32_t* actions, int32_t slots, uint64_t seed, void* states_out,
                           int out_dtype, int32_t* actions_all_out, int32_t* actions_next_out, const double* rew_in,
                           double episode, double epsilon, void* stream);

/* An open-loop rollout: K slots of a GIVEN action sequence as ONE launch (additive within ABI 8; the slot loops of
 * step_fast64_slots_kernel / step_wide_slots_kernel with the actions read from `actions_seq` instead of decided on the chip):
 *   for k = 0 .. K - 1:   obs, rews = my_step(actions_seq[k], t + k)            [mode DIRAL_STEP_MY_STEP_CH: my_step_ch]
 *                         shaped_out[k], sum_r_out[k], collision_out[k] = diral_driver_shape(rews, actions_seq[k], ...)
 *                         diral_env_update_velocity(env, NULL, vel_seed + (t + k) / episode_interval)   [at an episode end]
 * Equal, bit for bit, to that loop of diral_env_step + diral_driver_shape (+ diral_env_update_velocity) calls: states,
 * rewards, shaped rewards, sums, collisions, done, tables, ring, positions, velocities, metrics, penalty state.  A replayed
 * action log, a fixed schedule (TDMA), action repeat, B candidate sequences of a search.
 *   actions_seq [K][B][N]     slots >= 1
 *   states_out                NULL: no slot computes the positional histogram; states_all = 0: [B][N][S] of the LAST slot;
 *                             states_all = 1: [K][B][N][S], row k = obtain_state(obs_k, actions_seq[k], rews_k)
 *   rew_out [B][N], done_out [B]   of the LAST slot (each may be NULL; shaped_out needs rew_out)
 *   shaped_out [K][B][N], sum_r_out [K][B], collision_out [K][B]   out dtype, slot-major; shaped_out NULL = no shaping;
 *     shape_flags: bit 0 global_reward_avg, bit 2 stuck-action penalty (then pen_counter / pen_prev_actions are mandatory);
 *     shape_flags = 0: shaped_out[k] is the reward as the step returns it
 * Configurations the slot loops take: 8 <= N <= 256, A <= 64, the one-lane highway, piggybacked tables, no arrival (but
 * see diral_env_rollout_ia) / PRR tracking, no trace replay, no static topology, no State.piggybacking, no secondary observation mode behind a state
 * vector; my_step_ch and states_all = 1 at N <= 64 only.  Otherwise DIRAL_ERR_UNSUPPORTED with nothing launched and the env
 * untouched (loop over the calls instead: diral_amd.driver.DriverLoop.rollout does).  my_step_ch with reward_design
 * outside 2 ... 4: DIRAL_ERR_BAD_CONFIG (as diral_env_step).  Toy-size envs (N <= 8, A <= 16): on a handle pinned to
 * DIRAL_PATH_SUBWAVE with DIRAL_OPT_SUBWAVE_SLOTS (csrc/step_subwave_slots.hpp), with every run-time switch of the one-slot
 * kernel - arrival and PRR tracking, the handle's trace, static topologies, off-lane vehicles, no tables -, both modes and
 * states_all = 1; diral_env_rollout_ia and a non-empty diral_env_rollout_replay block stay DIRAL_ERR_UNSUPPORTED there. */
typedef struct DiralRollout {
  uint32_t struct_bytes;          /* = sizeof(DiralRollout) */
  int32_t  shape_flags;
  int32_t  pen_threshold;
  int32_t  reserved0;
  double   pen_value;
  void*    shaped_out;            /* [K][B][N] out dtype or NULL */
  void*    sum_r_out;             /* [K][B] or NULL */
  void*    collision_out;         /* [K][B] or NULL */
  int32_t* pen_counter;           /* [B][N] (shape_flags bit 2) */
  int32_t* pen_prev_actions;      /* [B][N] */
  uint64_t vel_seed;              /* as DiralSlotPolicy::vel_seed */
} DiralRollout;
int diral_env_rollout(DiralEnv* env, int mode, const int32_t* actions_seq, int32_t slots, int64_t t, void* states_out,
                      int states_all, void* rew_out, uint8_t* done_out, int out_dtype, const DiralRollout* rollout,
                      void* stream);

/* Information age inside the K-slot my_step_ch launches (additive within ABI 8; step_fast64_slots_kernel, 8 <= N <= 64).
 * The reference's driver reads Network.get_information_age(time_step) behind EVERY slot (main_test.py:150) and, with
 * `ia_averaging`, turns the movement of utils/misc.calculate_ia_penalty of it into a -1 / 0 / +1 reward term
 * (main_test.py:151-160, 190-192).  The arrival stamps are my_step_ch's (test_env.py:436, network.py:394): the two entry
 * points below are diral_env_rollout / diral_env_step_policy with one more argument, the block, and on a handle created
 * with DIRAL_F_TRACK_ARRIVAL the slot loop then
 *   - keeps the arrival stamps from slot to slot (slot k stamps t + k, plus the slot clock when one is set),
 *   - writes behind slot k   ia_out[k] = diral_env_info_age(env, t + k),  ia_sum_out[k] = sum (i + 1) ia[i] over ia[i] > 0,
 *   - with flags bit 0 adds  term = -1 / +1 / 0 (ia_sum rose above / fell below / equals sum_ia_prev) to slot k's rewards
 *     in front of the stuck-action test and the global average (diral_driver_shape's order with `ia` and flag bit 1),
 *     writes it to ia_pen_out[k] and leaves ia_sum in sum_ia_prev; the state vector's reward column stays the raw reward.
 * Equal, bit for bit, to the loop of diral_env_step(DIRAL_STEP_MY_STEP_CH) + diral_env_info_age + diral_driver_shape
 * (+ diral_env_update_velocity) calls.  All three outputs NULL and flags 0: the stamps are kept, no histogram is built.
 *   `ia` NULL: exactly diral_env_rollout / diral_env_step_policy, refusals included (a tracking handle stays refused).
 *   DIRAL_ERR_BAD_ARG (checked first, no device needed): struct_bytes, flags & ~1, bit 0 without sum_ia_prev or without
 *     shaped_out, and everything the base entry point rejects;
 *   DIRAL_ERR_BAD_CONFIG: a handle without DIRAL_F_TRACK_ARRIVAL (as diral_env_info_age); reward_design outside 2 ... 4;
 *   DIRAL_ERR_UNSUPPORTED, nothing launched, env untouched: mode != DIRAL_STEP_MY_STEP_CH, N < 8 or N > 64, a one-slot
 *     diral_env_step_policy_ia call (slots <= 1), and every configuration the my_step_ch slot loop refuses (PRR tracking,
 *     trace replay, static topology, no piggybacked tables, vehicles off the lane, State.piggybacking, secondary observation
 *     modes behind a state vector).
 * Enqueue-only, like the other slot launches. */
typedef struct DiralSlotInfoAge {
  uint32_t struct_bytes;          /* = sizeof(DiralSlotInfoAge) */
  int32_t  flags;                 /* bit 0: ia_averaging - add the -1 / 0 / +1 term to every slot's shaped rewards */
  int32_t* ia_out;                /* [K][B][100] Network.get_information_age(t + k) behind slot k, or NULL */
  int64_t* ia_sum_out;            /* [K][B] utils/misc.calculate_ia_penalty of it, or NULL */
  int32_t* ia_pen_out;            /* [K][B] the term (written with bit 0), or NULL */
  int64_t* sum_ia_prev;           /* [B] in/out, the caller's (as pen_counter is); mandatory with bit 0 */
} DiralSlotInfoAge;
int diral_env_rollout_ia(DiralEnv* env, int mode, const int32_t* actions_seq, int32_t slots, int64_t t, void* states_out,
                         int states_all, void* rew_out, uint8_t* done_out, int out_dtype, const DiralRollout* rollout,
                         const DiralSlotInfoAge* ia, void* stream);
int diral_env_step_policy_ia(DiralEnv* env, int mode, const int32_t* actions, int64_t t, void* state_out, void* rew_out,
                             uint8_t* done_out, void* chobs_out, int out_dtype, const DiralSlotPolicy* policy,
                             const DiralSlotInfoAge* ia, void* stream);

/* Recorded mobility inside the K-slot launches (additive within ABI 8; step_fast64_slots_kernel, 8 <= N <= 64).
 * The reference's driver replaces the velocity model with a recorded run before its main loop (main_test.py:118,
 * Network.load_x_positions and the replay branch of update_positions, network.py:171-178, 194-199) and logs the positions of
 * every slot (main_test.py:140-142, 254-255).  The two entry points below are diral_env_rollout_ia /
 * diral_env_step_policy_ia with one more argument, the block; slot k of the launch then
 *   - with x_positions: leaves  pos_x[b][u] = x_positions[(per_env ? b * T : 0) + tt][u],  tt = (t + k + clock) mod T with
 *     Python's sign (clock: the slot clock, when one is set) - what the one-slot calls do on a handle that had
 *     diral_env_set_trace(x_positions, T, per_env); `per_env` indexes by the env's index in THIS handle; the positions slot
 *     0 starts from are the handle's own; velocities are still drawn at episode ends (mobility_vary) and still feed the
 *     state vector's velocity column, as in the reference;
 *   - with xpos_out: writes pos_x behind slot k to xpos_out[k] (= get_x_pos() in front of slot k + 1), with or without
 *     x_positions: the log of a velocity-model launch, handed back as x_positions with T = K, reproduces that launch.
 * The sequence is the caller's device memory: it is not copied, the call is enqueue-only (capturable), and it may differ
 * from call to call.  Equal, bit for bit, to the loop of one-slot calls on a handle that carries the trace.
 *   `replay` NULL, or both pointers NULL: exactly diral_env_rollout_ia / diral_env_step_policy_ia, refusals included.
 *   DIRAL_ERR_BAD_ARG (checked first, no device needed): struct_bytes, flags != 0, x_positions with T < 1, T != 0 without
 *     x_positions, and everything the _ia entry point rejects;
 *   DIRAL_ERR_UNSUPPORTED, nothing launched, env untouched: everything the _ia entry point refuses - a handle with a trace
 *     of its own among it (one source of positions per call) -, N > 64 (step_wide_slots_kernel does not take the block), and
 *     a one-slot diral_env_step_policy_replay call (slots <= 1).
 * The prefill does not take the block: the driver loads the positions behind it (main_test.py:99-118). */
typedef struct DiralSlotReplay {
  uint32_t struct_bytes;          /* = sizeof(DiralSlotReplay) */
  int32_t  flags;                 /* 0 */
  const double* x_positions;      /* [T][N] (per_env == 0) or [B][T][N] (per_env != 0) float64, device; or NULL: the velocity model */
  int32_t  T, per_env;
  double*  xpos_out;              /* [K][B][N] float64: pos_x BEHIND slot k, or NULL */
} DiralSlotReplay;
int diral_env_rollout_replay(DiralEnv* env, int mode, const int32_t* actions_seq, int32_t slots, int64_t t, void* states_out,
                             int states_all, void* rew_out, uint8_t* done_out, int out_dtype, const DiralRollout* rollout,
                             const DiralSlotInfoAge* ia, const DiralSlotReplay* replay, void* stream);
int diral_env_step_policy_replay(DiralEnv* env, int mode, const int32_t* actions, int64_t t, void* state_out, void* rew_out,
                                 uint8_t* done_out, void* chobs_out, int out_dtype, const DiralSlotPolicy* policy,
                                 const DiralSlotInfoAge* ia, const DiralSlotReplay* replay, void* stream);

/* ---- slot clock: rollouts captured into a hipGraph ---------------------------------------------
 * A captured sequence of K slots (env step, reward shaping, policy) bakes every by-value argument into its
 * kernel nodes; what has to move on from replay to replay - the slot number behind `done`, arrival stamps and
 * trace replay; the seed of the policy's draws - is read from a DEVICE counter instead.
 *   diral_env_set_clock(env, t_dev): from now on diral_env_step's `t` is an OFFSET: the slot number is
 *     *t_dev + t, read by the kernel (t_dev NULL: back to the by-value slot number).  int64 in HBM, owned by
 *     the caller, alive as long as it is set.
 *   diral_clock_add(clock, inc, stream): *clock += inc as a one-thread launch (the last node of the graph).
 *   diral_sps_step_chobs_clocked: diral_sps_step_chobs with device draws seeded by seed + *clock. */
int diral_env_set_clock(DiralEnv* env, const int64_t* t_dev);
/* Slow-first dispatch inside captured graphs (N <= 64).  A step launch leaves the list of the envs
 * it found slow for the NEXT launch in one of three rotating sets; the host counts launches to know which set a launch
 * reads, builds and clears.  A captured launch is baked with its sets, so by default it only READS the set of the last
 * eager launch and builds none - correct, but the list ages with the replays.
 *   diral_env_set_capture_rotation(env, 1, &phase): from now on captured step launches rotate the sets like eager ones.
 *     The caller promises: every graph captured while this is on holds a MULTIPLE OF 3 step launches of this env, is
 *     replayed whole, and diral_env_align_phase(env, phase, stream) is called (on the replay's stream) before a replay
 *     that follows anything but another replay of the same graph.  *phase (may be NULL) = the env's phase (launch count
 *     mod 3) at the call: the phase of the first launch captured next.  (…, 0, …): back to the default.
 *   diral_env_align_phase(env, phase, stream): make the env's phase `phase`; if it has to move, the three sets are
 *     emptied first (an empty list is always a valid one: the next launch runs every env in dispatch order). */
int diral_env_set_capture_rotation(DiralEnv* env, int on, int* phase);
int diral_env_align_phase(DiralEnv* env, int phase, void* stream);
int diral_clock_add(int64_t* clock, int64_t inc, void* stream);
int diral_sps_step_chobs_clocked(int agents, int num_channels, const void* chobs, int chobs_dtype,
                                 const int32_t* actions, int32_t* prev_action, int32_t* counter,
                                 double rssi_threshold, double inc_db, double keep_prob, uint64_t seed,
                                 const int64_t* clock, int32_t* actions_out, void* stream);

/* ---- actions from Q-values: the exploration policies of algorithms/policies.py ---------------------
 * diral_policy_select: actions_out[i] for agents = B * N rows of num_channels Q-values, ONE launch, handle-free like
 * diral_sps_*.  Every Q-value (q_dtype: DIRAL_F64 / F32 / F16 / BF16) is converted exactly to float64; all arithmetic
 * is float64 in NumPy's order.
 *   DIRAL_SELECT_GREEDY (policies.py:24-35): np.argmax - the first index of the maximum (-0.0 == +0.0), the first NaN
 *     of a row that holds one, 0 for a row of -inf.
 *   DIRAL_SELECT_EPS_GREEDY (:45-54): draw_u > eps -> greedy, else draw_a % A.
 *   DIRAL_SELECT_SOFTMAX (:92-112, np.random.choice(p=)): x = q / tmp; x -= max(x); y = exp(x); p = y / np.sum(y);
 *     cdf = cumsum(p) sequentially; cdf /= cdf[A - 1]; the action is the number of cdf[j] <= draw_u, at most A - 1.  A row
 *     the reference raises on (a NaN, a +inf, nothing but -inf) is answered by the GREEDY rule and counted in *bad_rows.
 *   DIRAL_SELECT_BOLTZMANN (:144-178): explore_p > draw_u -> draw_a % A, else
 *     argmax((1 - alpha) * exp(beta * q) / np.sum(exp(beta * q)) + alpha / A) as written (inf / inf is NaN: the first one).
 * draw_u [agents] float64 in [0, 1) / draw_a [agents] int32 >= 0: injected draws; NULL: the device generator at
 * (seed, stream 10 / 11, idx0 + i), idx0 = the caller's DIRAL_OPT_ENV_OFFSET * num_users - shards of a batch draw what
 * the whole batch draws.  clock != NULL: the launch draws with seed + clock_offset + *clock (a device counter, see
 * diral_clock_add), so a replayed graph draws afresh.  param_dev != NULL: the kind's parameter (eps / tmp / explore_p)
 * is read from device memory instead - one float64, or one per env ([agents / num_users], param_per_env != 0); a tmp
 * read there is not checked.  explored_out (uint8 [agents], 1 where the exploring branch chose) and bad_rows (int32,
 * added to) may be NULL.
 * DIRAL_ERR_BAD_ARG, before any device is touched: a NULL struct / q / actions_out, a wrong struct_bytes, agents < 1,
 * num_channels < 1, agents no multiple of num_users, an unknown kind or dtype, a by-value tmp that is not finite and
 * > 0 (SOFTMAX), param_per_env without param_dev.  DIRAL_ERR_UNSUPPORTED: num_channels > 4096. */
typedef enum DiralSelectKind {
  DIRAL_SELECT_GREEDY = 0, DIRAL_SELECT_EPS_GREEDY = 1, DIRAL_SELECT_SOFTMAX = 2, DIRAL_SELECT_BOLTZMANN = 3
} DiralSelectKind;
typedef struct DiralSelect {
  uint32_t struct_bytes;       /* sizeof(DiralSelect) */
  int32_t kind;                /* DiralSelectKind */
  int32_t agents;              /* B * N */
  int32_t num_users;
  int32_t num_channels;
  const void* q;               /* [agents][num_channels], contiguous */
  int32_t q_dtype;             /* DiralDType */
  double eps, tmp, beta, alpha, explore_p;
  const double* param_dev;
  int32_t param_per_env;
  const double* draw_u;
  const int32_t* draw_a;
  uint64_t seed;
  uint64_t idx0;
  const int64_t* clock;
  int64_t clock_offset;
  int32_t* actions_out;
  uint8_t* explored_out;
  int32_t* bad_rows;
} DiralSelect;
int diral_policy_select(const DiralSelect* s, void* stream);

/* ---- replay memory: Memory of utils/memory.py:162-194 for B envs, and the regrouping of drl_drqn.py:294-377 --------
 * Handle-free like diral_policy_select: the caller owns three rings of capacity + 1 rows and describes them here.
 *   states  [capacity + 1][batch][num_users][state_space]   dtype (DIRAL_F32 / DIRAL_F64)
 *   actions [capacity + 1][batch][num_users]                int32
 *   rewards [capacity + 1][batch][num_users]                dtype
 * The driver always has state = next_state (main_test.py:113, 217), so a state is stored once: logical state j lives in
 * row j mod (capacity + 1), transition j (state j -> j + 1) keeps its action and reward in row j mod (capacity + 1).
 * With `count` transitions added so far the live ones are j in [count - len, count), len = min(count, capacity) - the
 * deque's maxlen.  count is the host value below, or *count_dev (device memory, read by the kernels) when that is given;
 * the caller moves it on behind an add (diral_clock_add(count_dev, slots)). */
typedef struct DiralMemory {
  uint32_t struct_bytes;       /* sizeof(DiralMemory) */
  int32_t capacity;            /* C >= 1 */
  int32_t batch, num_users, state_space;
  int32_t dtype;               /* DiralDType of states and rewards: DIRAL_F32 / DIRAL_F64 */
  void* states;
  int32_t* actions;
  void* rewards;
  int64_t count;               /* transitions added so far (>= 0); not read when count_dev != NULL */
  const int64_t* count_dev;
} DiralMemory;

/* diral_memory_add: ONE launch writes `slots` = K transitions: next_states[k] into state row (count + 1 + k), actions[k]
 * and rewards[k] into row (count + k), all mod (capacity + 1) - across the wrap.  state0 != NULL (the first call after a
 * begin): written to state row count.  src_dtype / rewards_dtype: DIRAL_F32 / DIRAL_F64 of next_states + state0 / of
 * rewards; float64 into a float32 ring is rounded to nearest, float32 into a float64 ring is exact.  rewards_broadcast
 * != 0: rewards is ONE [batch][num_users] row stored for every slot (the prefill's stale bootstrap rewards,
 * main_test.py:110-112).  The count itself is the caller's to move on.
 * DIRAL_ERR_BAD_ARG, before any device is touched: a NULL struct / ring / source, a wrong struct_bytes, capacity, batch,
 * num_users or state_space < 1, count < 0, slots < 1, slots > capacity, an unknown dtype. */
typedef struct DiralMemoryAdd {
  uint32_t struct_bytes;       /* sizeof(DiralMemoryAdd) */
  int32_t slots;               /* K */
  const void* next_states;     /* [K][batch][num_users][state_space] */
  const void* state0;          /* [batch][num_users][state_space] or NULL */
  int32_t src_dtype;
  int32_t rewards_dtype;
  const int32_t* actions;      /* [K][batch][num_users] */
  const void* rewards;         /* [K][batch][num_users], or [batch][num_users] (rewards_broadcast) */
  int32_t rewards_broadcast;
} DiralMemoryAdd;
int diral_memory_add(const DiralMemory* m, const DiralMemoryAdd* a, void* stream);

/* diral_memory_sample: `windows` = M windows of `step` consecutive transitions as ONE launch, regrouped user-major as
 * DRQN.get_states_user and the three like it leave them (row n * M + m):
 *   states_out, next_states_out [num_users * M][step][state_space]  out_dtype
 *   actions_out [num_users * M][step] int32, rewards_out [num_users * M][step] ring dtype
 *   last_only != 0: actions_out / rewards_out [num_users * M], the last step only (drl_drqn.py:255, 288)
 * Any output may be NULL.  out_dtype: F32 ring -> DIRAL_F32 / F16 / BF16 (one round-to-nearest-even from float32), F64
 * ring -> DIRAL_F64 / F32; any other pair is DIRAL_ERR_UNSUPPORTED.  Each of a window's step + 1 state rows is read once.
 * Window m is (env b, start i), i in [0, L), L = len - step (np.arange(len(buffer) - step_size): the last start is
 * excluded as there); it covers the logical transitions count - len + i + s, s < step.
 *   Injected: idx [M] and env [M] (int32, device).  A start outside [0, L) or an env outside [0, batch) makes that
 *   window's outputs zeros and adds one to *bad_samples; nothing out of bounds is read.
 *   Drawn (idx == env == NULL): distinct by construction over the R = batch * L pairs: v = P(m), b = v mod batch,
 *   i = v div batch, P a cycle-walking 4-round Feistel permutation of [0, R) on 2 w bits, w = max(1, ceil(ceil_log2(R)
 *   / 2)): (l, r) -> (r, l ^ (rng(seed', round, r) & (2^w - 1))), applied again while the value is >= R; rng is the
 *   generator of diral_env_sample, seed' = seed (+ clock_offset + *clock when clock != NULL: a replayed graph draws
 *   afresh).  idx_out / env_out [M] (may be NULL) receive the windows, so that a run can be replayed by injection.
 * DIRAL_ERR_BAD_ARG, before any device is touched: a NULL struct, a wrong struct_bytes, step < 1, windows < 1, a host
 * count with len <= step, drawn windows > R, idx without env or env without idx.  With count_dev the kernel applies the
 * last two itself: every window is zeros and counted in *bad_samples. */
typedef struct DiralMemorySample {
  uint32_t struct_bytes;       /* sizeof(DiralMemorySample) */
  int32_t windows;             /* M */
  int32_t step;
  int32_t out_dtype;           /* DiralDType of states_out / next_states_out */
  int32_t last_only;
  const int32_t* idx;
  const int32_t* env;
  uint64_t seed;
  const int64_t* clock;
  int64_t clock_offset;
  void* states_out;
  void* next_states_out;
  int32_t* actions_out;
  void* rewards_out;
  int32_t* idx_out;
  int32_t* env_out;
  int32_t* bad_samples;
} DiralMemorySample;
int diral_memory_sample(const DiralMemory* m, const DiralMemorySample* s, void* stream);

/* diral_memory_history (additive within ABI 8): the acting window, ONE launch - history_input = deque(maxlen=step_size),
 * np.array(history_input) and state_vector[:, user] (main_test.py:86, 114, 125, 219; drl_drqn.py:171-172) of every agent:
 *   out [batch * num_users][step][state_space]  out_dtype, row b * num_users + n - ENV-major, so that a network's output
 *   on it viewed as [batch][num_users][A] is what diral_policy_select takes.
 * Step s holds logical state count - step + 1 + s (ring row mod capacity + 1): the window ENDS at the newest state, which
 * no window of diral_memory_sample contains.  The live states are [count - len, count], so step <= len + 1; with a host
 * count anything else is DIRAL_ERR_BAD_ARG, with count_dev the kernel writes zeros to all of `out` and adds one to *bad
 * (may be NULL).  State row `count` must be valid: after a begin the caller has written state0 there.  The dtype pairs are
 * diral_memory_sample's (any other: DIRAL_ERR_UNSUPPORTED).  Enqueue-only.
 * DIRAL_ERR_BAD_ARG, before any device is touched: what DiralMemory is refused for (above), step < 1, a NULL out. */
int diral_memory_history(const DiralMemory* m, int32_t step, int32_t out_dtype, void* out, int32_t* bad, void* stream);

/* diral_td_head (additive within ABI 8): the TD targets of DRQN._calc_target (drl_drqn.py:267-292), the loss head
 * (:76-80) and its gradient dL/dQ for rows = num_users * batch rows of num_actions Q-values.  Handle-free, flat arguments,
 * ONE launch and a second, single-workgroup one for the loss (skipped when loss_out is NULL).
 *   q             [rows][num_actions]  the eval net on `states`; NULL: targets only (_calc_target by itself; actions must
 *                                      still be given and is not read)
 *   q_next_target [rows][num_actions]  the target net on `next_states`
 *   q_next_eval   [rows][num_actions]  the eval net on `next_states`, or NULL for use_double = False
 *   q_dtype       of all three: DIRAL_F32 / F16 / BF16, converted exactly to float32
 *   actions [rows] int32, rewards [rows] DIRAL_F32 / F64 (rewards_dtype): diral_memory_sample's last_only outputs
 * Per row, float32 arithmetic unless said otherwise:
 *   1. j = np.argmax(q_next_eval row, or q_next_target row when that is NULL): the first index between equals (-0.0 ==
 *      +0.0) and between NaNs, a NaN above any number
 *   2. nv = q_next_target[row][j] - np.max in the plain case (a NaN row gives NaN; the sign of a zero maximum is the first
 *      zero's, numerically equal to np.max)
 *   3. target = (float)((double)r + (double)((float)gamma * nv)), never fused
 *   4. Q = q[row][a], h = Q - target.  a outside [0, num_actions): Q = 0, a zero gradient row (tf.one_hot's), one more in
 *      *bad_rows, nothing read out of bounds.  Q is gathered where the reference has reduce_sum(q * one_hot): a non-finite
 *      value in a column that was not chosen does not poison the row, and a chosen -0.0 stays -0.0
 *   5. hl = (hysteretic != 0 && h < 0) ? h / 10.0f : h
 *   6. g = (2.0f * hl) / (float)rows, and g / 10.0f on the rows of the hysteretic branch
 * Outputs, each may be NULL: targets_out [rows] float32; td_out [rows] float32 (hl); next_action_out [rows] int32 (j);
 * grad_q_out [rows][num_actions] q_dtype - g rounded to nearest even once in column a, zeros elsewhere, all of it written
 * by the launch; loss_out, one float32: mean(hl^2) = (float)(sum / rows), the sum in double over td_out - thread t of 256
 * adds (double)hl * (double)hl of the rows t, t + 256, ... in turn, the 256 partial sums are added in index order -, so the
 * same input gives the same bits; bad_rows, an int32 counter that is added to.  grad_q_out does not depend on the loss.
 * DIRAL_ERR_BAD_ARG, before any device is touched: a NULL q_next_target, actions or rewards, rows < 1, num_actions < 1,
 *   an unknown dtype, a non-finite gamma, q == NULL with td_out, grad_q_out or loss_out, loss_out without td_out;
 * DIRAL_ERR_UNSUPPORTED: num_actions > 4096, rows > 2^24 ((float)rows must be exact), q_dtype == DIRAL_F64. */
int diral_td_head(int32_t rows, int32_t num_actions, const void* q, const void* q_next_target, const void* q_next_eval,
                  int32_t q_dtype, const int32_t* actions, const void* rewards, int32_t rewards_dtype, double gamma,
                  int32_t hysteretic, float* targets_out, float* td_out, int32_t* next_action_out, void* grad_q_out,
                  float* loss_out, int32_t* bad_rows, void* stream);

/* diral_qnet_forward (additive within ABI 8): the dense chain of DRQN._create_network (drl_drqn.py:109-155) as ONE
 * launch - [matmul + bias -> relu -> layer_norm] x num_hidden, then matmul + bias - for q [rows][A] from x [rows][D].  With
 * use_lstm_input false it is the whole Q-network (the DQN branch, state_vector[-1:, user]), with it true everything behind
 * lstm_out[:, -1, :].  Handle-free, flat arguments, no gradient.
 *   widths   HOST array [D, h_1 .. h_num_hidden, A]: 0 <= num_hidden <= 3, 1 <= D <= 1024, 1 <= h_i <= 256, 1 <= A <= 256
 *   x        rows of D elements of x_dtype (DIRAL_F32 / F16 / BF16, converted exactly to float32), unit stride along D,
 *            x_row_stride >= D ELEMENTS from row to row, 64-bit addressing: window[:, -1] of a [rows][step][S] window
 *            goes in as x = &window[0][step - 1][0], x_row_stride = step * S
 *   params   ONE device blob of float32, params_len values: per hidden layer W [in][out] row-major (the reference's
 *            orientation), b [out], gamma [out], beta [out] - gamma and beta are there with norm == 0 too -, then the
 *            output layer's W [h_L][A], b [A].  Read at every launch (and at every replay of a captured one).
 *   q_out    [rows][A] float32, contiguous
 * Per row, float32 arithmetic, never fused:
 *   1. z[j] = (sum over k = 0 .. in - 1, in that order, of x[k] * W[k][j]) + b[j]: the sum starts at zero and is the
 *      f32-input MFMA's, acc = fmaf(x[k], W[k][j], acc) with one rounding per term; the bias is added to the finished sum
 *   2. r[j] = z[j] > 0 ? z[j] : 0; a NaN stays a NaN
 *   3. mean = (sum r) / h, var = (sum (r - mean)^2) / h over the h columns of the layer: two passes, biased, tf.nn.moments'.
 *      Each sum is four partial sums - partial s adds the columns s, s + 4, s + 8, .. in turn - added as ((p0 + p1) + p2) + p3.
 *      The mean is summed twice, m0 = (sum r) / h and mean = m0 + (sum (r - m0)) / h, which takes the first sum's rounding
 *      out: a row of equal values c has mean == c, var == 0 and y == beta exactly (with ln_eps = 1e-12 an ulp in the mean
 *      would come out as 0.06 in every column)
 *   4. y[j] = (r[j] - mean) * (1.0f / sqrtf(var + (float)ln_eps)) * gamma[j] + beta[j], left to right
 *   5. the output layer is step 1 alone
 * norm == 0 leaves out 3 and 4 (relu only).  ln_eps is the caller's; tf.contrib.layers.layer_norm of TF 1.14 uses
 * variance_epsilon = 1e-12 as far as its source is remembered - TensorFlow was not at hand to read it off.
 * The order of every sum is fixed, and a row's Q-values depend on that row and the blob only: not on `rows`, not on the
 * row's place in the call, not on what other rows hold.  Nothing past row `rows` is read or written.  Enqueue-only on
 * `stream`, one kernel node, no allocation, no synchronisation.
 * DIRAL_ERR_BAD_ARG, before any device is touched: a NULL widths, x, params or q_out, rows < 1, num_hidden < 0, a width
 *   < 1, an unknown x_dtype, x_row_stride < D, params_len other than what widths implies, ln_eps negative or not finite;
 * DIRAL_ERR_UNSUPPORTED, likewise: num_hidden > 3, D > 1024, h_i > 256, A > 256, x_dtype == DIRAL_F64. */
int diral_qnet_forward(int32_t rows, int32_t num_hidden, const int32_t* widths, const void* x, int32_t x_dtype,
                       int64_t x_row_stride, const float* params, int64_t params_len, int32_t norm, double ln_eps,
                       float* q_out, void* stream);

/* The K-slot rollout and prefill write the ring rows themselves (additive within ABI 8; step_fast64_slots_kernel at
 * 8 <= N <= 64 and step_subwave_slots_kernel at N <= 8).  diral_env_rollout_memory is diral_env_rollout_replay with one
 * more argument, the caller's DiralMemory; diral_env_prefill_memory is diral_env_prefill_mode with the same.  A ring row is
 * a [batch][num_users][state_space] block like a row of states_out, so with the block slot k of the launch writes
 *   its state vector (what states_out[k] would get)                       to state row  (count + 1 + k)
 *   the actions it ran with (actions_seq[k]; prefill: actions_all_out[k]) to action row (count + k)
 *   rollout: its shaped reward (what shaped_out[k] would get)             to reward row (count + k)
 *   prefill: rew_in[b][n] cast to the ring dtype, for every slot          to reward row (count + k)
 * all mod (capacity + 1), across the wrap: the rows and values diral_memory_add writes from the launch's scratch outputs
 * (above; rewards_broadcast for the prefill), without that launch and without the scratch.  count is the host value, or
 * *count_dev read once per workgroup.  State row `count` must already be valid - the last state of the previous add, or
 * state0 written there by the caller after a begin -: the launch does not write it.  The count is the caller's to move on
 * (diral_clock_add(count_dev, slots)), as for diral_memory_add.  sum_r_out and collision_out stay [K][B] caller outputs,
 * rew_out and done_out the last slot's; ia and replay blocks are taken as by diral_env_rollout_replay.  Enqueue-only.
 *   `memory` NULL: exactly diral_env_rollout_replay / diral_env_prefill_mode, refusals included.
 *   DIRAL_ERR_BAD_ARG (checked first, no device needed): a wrong struct_bytes, a NULL ring, capacity < 1, slots > capacity,
 *     count < 0 (host count), batch / num_users / state_space that differ from the handle's B, N and state size, the ring
 *     dtype != out_dtype (no conversion is added: the stored bits are the scratch path's), states_out or shaped_out
 *     (rollout) / states_out or actions_all_out (prefill) given together with the block - the rings take their place -,
 *     a prefill without rew_in, and everything the base entry point rejects;
 *   DIRAL_ERR_UNSUPPORTED, nothing launched, env and rings untouched: N > 64 (step_wide_slots_kernel has no states_all),
 *     a handle pinned to DIRAL_PATH_SUBWAVE without DIRAL_OPT_SUBWAVE_SLOTS, and everything the base entry point refuses
 *     (loop and diral_memory_add instead: diral_amd.driver.DriverLoop.rollout / prefill with memory= do). */
int diral_env_rollout_memory(DiralEnv* env, int mode, const int32_t* actions_seq, int32_t slots, int64_t t, void* states_out,
                             int states_all, void* rew_out, uint8_t* done_out, int out_dtype, const DiralRollout* rollout,
                             const DiralSlotInfoAge* ia, const DiralSlotReplay* replay, const DiralMemory* memory,
                             void* stream);
int diral_env_prefill_memory(DiralEnv* env, int mode, const int32_t* actions, int32_t slots, uint64_t seed, void* states_out,
                             int out_dtype, int32_t* actions_all_out, int32_t* actions_next_out, const double* rew_in,
                             double episode, double epsilon, const DiralMemory* memory, void* stream);

/* Replaces SemiPersistentScheduling.__init__ (v2x_sps.py:8-22): prev_action =
 * randint(0, selection_window) (inclusive, as in the reference), counter =
 * randint(5, 15); device RNG from `seed`. */
int diral_sps_init(int agents, int selection_window, int32_t* prev_action, int32_t* counter, uint64_t seed,
                   void* stream);

/* last HIP error string seen by this handle (host-side, for DIRAL_ERR_HIP) */
const char* diral_env_last_hip_error(const DiralEnv* env);

#ifdef __cplusplus
}
#endif
#endif /* DIRAL_ENV_H */
