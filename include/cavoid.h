/* cavoid.h -- C ABI of the MI355X-native batched collision-avoidance env.step hot path.
 *
 * Drop-in boundary.  The reference has NO FFI for this path: the seam is a duck-typed Python
 * object.  Each entry point below names the reference interface it
 * stands in for (paths relative to /root/reference):
 *
 *   cavoid_create / cavoid_destroy ... `env, one_env = create_env()`            ga3c/GA3C/Environment.py:54-56
 *   cavoid_reset ..................... `observations = self.game.reset()`        ga3c/GA3C/Environment.py:106
 *   cavoid_step ...................... `self.game.step(action)` -> 4-tuple        ga3c/GA3C/Environment.py:112
 *                                      (obs, rewards, game_over, which_agents_done) ga3c/GA3C/ProcessAgent.py:149-157
 *   cavoid_step_autoreset ............ the per-episode `env.reset()` + step loop  ga3c/GA3C/ProcessAgent.py:105-116
 *   cavoid_*_packed .................. the same calls, returning ONE record per agent (obs | reward | done): what
 *                                      an actor hands back per step                  ga3c/GA3C/ProcessAgent.py:149-157
 *   cavoid_comm_* / cavoid_gather_* .. (new) the actors -> trainer hand-over across GPUs; the reference moves it
 *                                      through mp.Queue between processes            ga3c/GA3C/ProcessAgent.py:221,238
 *   cavoid_step_continuous ........... the env-level continuous action space      run-ws/config.yaml:3-5 (ACTION_SPACE_TYPE)
 *   cavoid_observe ................... the obs half of reset()/step()             ga3c/GA3C/Environment.py:81-91
 *   cavoid_set_state/get_state ....... (new) explicit initial states for parity runs; env checkpointing
 *   cavoid_default_cfg ............... the env's Config scalars                   ga3c/GA3C/Config.py:29,34-52 +
 *                                      checkpoints/regression/wandb/run-ws/config.yaml
 *   cavoid_default_actions ........... `Actions().actions[11,2]`                  ga3c/GA3C/Server.py:36,51-52
 *
 * Conventions: plain pointers and sizes, no torch types.  Every data pointer is a DEVICE pointer
 * on the env's device and is owned by the caller; the library owns only its internal world
 * buffer.  All work is enqueued asynchronously on the `hipStream_t` passed as `void *stream`
 * (NULL = the default stream).  Return 0 on success, a negative CAVOID_E* code on failure; the
 * library never throws, aborts or falls back to a CPU path.  A handle is not thread-safe; use
 * one per device/stream.
 *
 * Layouts (W worlds, N = max_agents, M = max_other, flat agent index a = w*N + i):
 *   obs        float  [W, N, 2+4+7M]  col0 is_learning, col1 num_other_agents, col2 dist_to_goal,
 *                                     col3 heading_ego_frame, col4 pref_speed, col5 radius, then M x
 *                                     [p_par, p_orth, v_par, v_orth, r_other, r_host+r_other, gap]
 *                                     (ga3c/GA3C/Config.py:40,72-76; NetworkVP_rnn.py:58-61)
 *   rewards    float  [W, N]
 *   done       u8     [W, N]          which_agents_done; 1 for absent agents
 *   game_over  u8     [W]             every *learning* agent of the world is done (TRAIN_MODE)
 *   actions    int32  [W, N]          index into the action table; ignored for done / scripted agents
 *   packed     float  [W, N, 2+4+7M+2] the obs row followed by the step's reward and done (0.0f / 1.0f): the
 *                                     per-agent record of the multi-GPU gather
 *   state_f64  double [4, W*N]        px, py, heading, t_remaining           (SoA, field-major)
 *   state_f32  float  [5, W*N]        gx, gy, radius, pref_speed, speed
 *   flags      u32    [W*N]           CAVOID_F_* bits
 */
#ifndef CAVOID_H
#define CAVOID_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CAVOID_ABI_VERSION 3
#define CAVOID_MAX_ACTIONS 32
/* Agents per world: 1..64.  Worlds of up to 16 agents run the tile forms below; 17..64 agents run ONE form,
 * CAVOID_FORM_CROWD (the lanes of a world are its agents; a wavefront owns floor(64/N) whole worlds: three of 17..21 agents,
 * two of 22..32, one of 33..64).
 * What stops at 16 agents (CAVOID_EUNSUPPORTED for max_agents > 16): gen_lookahead > 0 and rvo_enabled = 1 (checked by
 * cavoid_create), cavoid_actor_run and cavoid_actor_run_mix (use cavoid_step_push, or the env step + cavoid_rollout_push).
 * ORCA agents in worlds of 17..64 agents: rvo_enabled = CAVOID_RVO_WAVE (the wavefront solves one agent's programme at a time, one
 * lane per constraint line; stepping launches then report CAVOID_FORM_CROWD_RVO).  ORCA at EXACTLY 16 agents is not available in
 * either form (the tile forms' line scratch ends at 15, the crowd form starts at 17): take max_agents = 17, gen_max_agents = 16. */
#define CAVOID_MAX_AGENTS 64

/* agent flag bits */
#define CAVOID_F_AT_GOAL 0x01u
#define CAVOID_F_RAN_OUT 0x02u
#define CAVOID_F_IN_COLL 0x04u
#define CAVOID_F_WAS_AT_GOAL 0x08u
#define CAVOID_F_WAS_IN_COLL 0x10u
#define CAVOID_F_PRESENT 0x20u
#define CAVOID_F_LEARNING 0x40u
#define CAVOID_F_POLICY_SHIFT 8 /* bits 8..10: 0 external (learning), 1 static, 2 non-cooperative, 3 RVO (ORCA),
                                   4 frozen network: a NON-learning agent whose action index the caller supplies like a learner's
                                   (from a second, frozen NetworkVP_rnn -- the GA3C-CADRL agent, ga3c/GA3C/Server.py:36) */
#define CAVOID_F_POLICY_MASK 7u
enum { CAVOID_POLICY_EXTERNAL = 0, CAVOID_POLICY_STATIC = 1, CAVOID_POLICY_NONCOOP = 2, CAVOID_POLICY_RVO = 3, CAVOID_POLICY_FROZEN_NET = 4 };
#define CAVOID_F_DONE_MASK 0x07u

enum { CAVOID_SORT_CLOSEST_LAST = 0, CAVOID_SORT_CLOSEST_FIRST = 1, CAVOID_SORT_TIME_TO_IMPACT = 2 };
enum { CAVOID_DYN_UNICYCLE = 0, CAVOID_DYN_UNICYCLE_MAX_TURN = 1, CAVOID_DYN_HOLONOMIC = 2 };

enum {
    CAVOID_OK = 0,
    CAVOID_EINVAL = -1,    /* bad argument / config */
    CAVOID_ENOMEM = -2,    /* device allocation failed */
    CAVOID_EHIP = -3,      /* a HIP runtime call failed (see cavoid_last_hip_error) */
    CAVOID_EUNSUPPORTED = -4, /* max_agents outside [1, CAVOID_MAX_AGENTS], or a feature that stops at 16 agents (see CAVOID_MAX_AGENTS) */
    CAVOID_ENODEVICE = -5, /* no usable gfx950 device */
    CAVOID_ECOMM = -6      /* an RCCL call failed (see cavoid_last_comm_error) */
};

typedef struct cavoid_cfg {
    uint32_t struct_size;      /* = sizeof(cavoid_cfg); checked by cavoid_create */
    uint32_t abi_version;      /* = CAVOID_ABI_VERSION */
    int32_t max_agents;        /* N: MAX_NUM_AGENTS_IN_ENVIRONMENT   (Config.py:34-37) */
    int32_t max_other;         /* M: MAX_NUM_OTHER_AGENTS_OBSERVED   (Config.py:46-49) */
    int32_t sort_method;       /* AGENT_SORTING_METHOD               (run-ws/config.yaml:9-11) */
    int32_t dynamics;          /* CAVOID_DYN_* */
    int32_t actions_fp32;      /* joint action array is float32 (default 1) */
    int32_t timeout_enabled;   /* default 1 */
    int32_t num_actions;       /* NUM_ACTIONS (Config.py:79) */
    int32_t evaluate_mode;     /* 0 (TRAIN_MODE): game over when every LEARNING agent is done; 1 (EVALUATE_MODE): every agent */
    int32_t time_budget_from_goal_edge; /* U11: 1 (default): an agent's time budget is MAX_TIME_RATIO * (dist_to_goal -
                                   NEAR_GOAL_THRESHOLD) / pref_speed (upstream agent.py as recalled); 0: SURVEY App. A's
                                   MAX_TIME_RATIO * dist_to_goal / pref_speed.  Either way at least one DT. */
    int32_t wrap_closed_end;   /* U2: 0 (default) angles wrap to [-pi, pi); 1: to (-pi, pi] */
    int32_t done_agents_collide; /* U4: 1 (default) an agent that is already done (frozen) still takes part in the others' collision
                                   test and nearest gap; 0: a pair with an agent that was done before the step is skipped */
    int32_t sort_round_gap;    /* U7a: 1 (default) neighbours are ordered by the gap rounded to centimetres; 0: by the exact gap */
    int32_t sort_tie_lateral;  /* U7b: 1 (default) equal (rounded) gaps are ordered by the lateral offset p_orth, then agent index;
                                   0: by agent index alone (a stable sort on the gap) */
    int32_t gen_lookahead;     /* R (power of two, 0 = off; needs gen_pool_size == 0): a FRESH scenario per episode without the generator on the step's
                                * critical path -- see "scenario look-ahead" below.  (this word was padding up to ABI 3: zero = off) */
    double dt;                 /* DT 0.2 */
    double near_goal_threshold;/* 0.2 */
    double max_time_ratio;     /* 2.0 */
    double collision_dist;     /* 0.0 */
    double getting_close_range;/* 0.2 */
    double reward_at_goal;     /* 1.0 */
    double reward_collision;   /* -0.25 */
    double reward_getting_close;/* -0.1 */
    double reward_time_step;   /* 0.0 */
    double close_penalty_slope;/* +0.5 (the published reward, arXiv:1805.01956; -0.5 = upstream code as the survey recalls it): r = reward_getting_close + slope*gap */
    double reward_clip_lo, reward_clip_hi; /* [-0.25, 1.0] */
    double sensing_horizon;    /* +inf */
    double max_turn_rate;      /* 3.0 rad/s (CAVOID_DYN_UNICYCLE_MAX_TURN only) */
    double actions[CAVOID_MAX_ACTIONS][2]; /* [speed fraction, delta heading] */
    /* scenario generator "GEN v1" used by cavoid_reset / autoreset */
    int32_t gen_min_agents, gen_max_agents;
    double gen_nonlearning_fraction, gen_static_fraction, gen_goal_jitter, gen_angle_jitter;
    /* scenario pool: > 0 pre-generates that many GEN v1 scenarios at cavoid_seed() time (pool entry k
     * = generator world k, episode 0); the episode `ep` of global world `gw` then uses entry
     * hash(seed, gw, ep) -> [0, pool_size) -- a gather instead of the generator on the step's critical
     * path (cf. the reference env's fixed test-case sets, NUM_TEST_CASES run-ws/config.yaml:136-138).
     * 0 = every episode runs the generator in-kernel with counter (gw, ep).  Default 65536. */
    int32_t gen_pool_size;
    /* scenario look-ahead (gen_pool_size == 0 and gen_lookahead = R > 0): every world owns a ring of R pre-generated scenarios of ITS OWN next
     * episodes -- slot e % R holds the generator's scenario of (global world, episode e), the very one the in-kernel generator would make --
     * refilled by a small kernel in front of the stepping launches (only the slots consumed since the last refill are generated), so a
     * restart is a gather, as with the pool, but every episode is the fresh, exact scenario of gen_pool_size = 0 (bitwise: tests).  A launch
     * may hold at most R - 1 steps (a world can restart at most once per step): more is CAVOID_EUNSUPPORTED.  Memory: W * R * N * 64 bytes. */
    /* GEN v2 (gen_mode = 1): starts and goals uniform in a box (half side ~ U(gen_box_small) for worlds of fewer than
     * gen_box_large_from agents, ~ U(gen_box_large) otherwise), agents placed one after the other by rejection sampling
     * against those already placed (starts and goals at least r_i + r_j + getting_close_range apart, trips of at least
     * gen_min_trip) -- the shape of upstream's get_testcase_random as recalled (TEST_CASE_FN, run-ws/config.yaml:281-283).
     * cavoid_reset and the auto-reset steps generate in-kernel (the placement is sequential over a world's agents: the wavefront
     * that owns the world generates it cooperatively) or, with gen_pool_size > 0, take GEN v2 scenarios from the pool. */
    int32_t gen_mode;
    int32_t gen_box_large_from;   /* 5 */
    uint32_t gen_pool_epoch;      /* the pool holds generator worlds 0..P-1 of THIS episode index (cavoid_pool_refresh) */
    int32_t rvo_enabled;          /* agents with policy 3 may exist.  Up to 15 agents per world any non-zero value selects the tile forms'
                                     ORCA (a lane solves its own agent; 4 KiB of LDS per wavefront and neighbour for the lines, which is
                                     why it ends at 15).  17..64 agents: CAVOID_RVO_WAVE only (the crowd form's wave-cooperative solve; no
                                     LDS beyond the crowd form's own); 1 is refused there, and both at exactly 16: CAVOID_EUNSUPPORTED */
    double gen_rvo_fraction;      /* of the scripted agents: P(static) = gen_static_fraction, P(RVO) = this, P(frozen network) =
                                     gen_frozen_fraction, the rest non-cooperative */
    double gen_frozen_fraction;   /* policy 4 agents (their actions come from the caller: cavoid_policy_rows lists them) */
    double gen_box_small[2], gen_box_large[2];   /* (4,5), (6,8) */
    double gen_min_trip;          /* 1.0 */
    /* RVO scripted policy: ORCA over the other agents' positions and last velocities */
    double rvo_time_horizon;      /* RVO_TIME_HORIZON 5.0   (run-ws/config.yaml:237-239) */
    double rvo_collab_coeff;      /* RVO_COLLAB_COEFF 0.5   (run-ws/config.yaml:234-236) */
    double rvo_radius_scale;      /* 1.05: the policy inflates every radius by 5 % */
    double rvo_max_delta_heading; /* pi/6: larger turns are clipped and taken standing still */
} cavoid_cfg;

/* values of cavoid_cfg.rvo_enabled */
enum { CAVOID_RVO_OFF = 0, CAVOID_RVO_LANE = 1, CAVOID_RVO_WAVE = 2 };

typedef struct cavoid_env cavoid_env;
typedef struct cavoid_rollout cavoid_rollout;   /* (section 'rollout' below) */
typedef struct cavoid_policy cavoid_policy;     /* (section 'fused policy inference' below) */

int cavoid_abi_version(void);
const char *cavoid_strerror(int code);
int cavoid_last_hip_error(void);                /* raw hipError_t of the last CAVOID_EHIP */
int cavoid_default_cfg(cavoid_cfg *cfg, int32_t max_agents, int32_t max_other);
int cavoid_default_actions(double (*table)[2], int32_t *num_actions);

/* world_offset: global id of this handle's first world (RNG streams are keyed on global world
 * ids so that results do not depend on how worlds are sharded over GPUs). */
int cavoid_create(const cavoid_cfg *cfg, int64_t num_worlds, int64_t world_offset, int device, cavoid_env **out);
void cavoid_destroy(cavoid_env *env);
int64_t cavoid_num_worlds(const cavoid_env *env);
int32_t cavoid_obs_width(const cavoid_env *env);

/* seed the generator; episode (device u32 [W]) may be NULL = "before episode 0" for every world */
int cavoid_seed(cavoid_env *env, uint64_t seed, const uint32_t *episode, void *stream);
int cavoid_get_episode(cavoid_env *env, uint32_t *episode_out, void *stream);
/* re-fill the scenario pool with generator worlds 0..P-1 of episode index `epoch` (cavoid_seed fills epoch
 * cfg.gen_pool_epoch): a long run that wants fresh scenarios without the generator on the step's critical path
 * refreshes the pool every so often.  No-op without a pool. */
int cavoid_pool_refresh(cavoid_env *env, uint32_t epoch, void *stream);

/* the agents of a world must be packed: CAVOID_F_PRESENT rows first (indices 0..n-1), absent rows after */
int cavoid_set_state(cavoid_env *env, const double *state_f64, const float *state_f32, const uint32_t *flags, void *stream);
int cavoid_get_state(cavoid_env *env, double *state_f64, float *state_f32, uint32_t *flags, void *stream);

/* start the next episode in every world whose mask byte is non-zero (mask NULL = all worlds) and
 * write the observation of ALL worlds (obs may be NULL to skip) */
int cavoid_reset(cavoid_env *env, const uint8_t *world_mask, float *obs, void *stream);
int cavoid_observe(cavoid_env *env, float *obs, void *stream);

int cavoid_step(cavoid_env *env, const int32_t *actions, float *obs, float *rewards, uint8_t *done,
                uint8_t *game_over, void *stream);
int cavoid_step_continuous(cavoid_env *env, const float *actions /* [W,N,2] */, float *obs, float *rewards,
                           uint8_t *done, uint8_t *game_over, void *stream);
/* step; worlds that end are restarted in the same launch and their obs rows hold the first
 * observation of the new episode (rewards/done/game_over still describe the finished step) */
int cavoid_step_autoreset(cavoid_env *env, const int32_t *actions, float *obs, float *rewards, uint8_t *done,
                          uint8_t *game_over, void *stream);
/* n_steps back-to-back autoreset steps in ONE launch; step t reads actions + t*action_stride (int32 elements) and
 * writes its outputs into SLOT t: with S = out_step_stride (in WORLDS, >= num_worlds) the outputs are arrays
 *   obs [n_steps, S, N, width], rewards / done [n_steps, S, N], game_over [n_steps, S]
 * -- what ProcessAgent.run_episode consumes of EVERY step (rewards, which_agents_done, the next observation:
 * ga3c/GA3C/ProcessAgent.py:149-157).  out_step_stride = 0: every step overwrites slot 0 (after the call the outputs hold
 * the LAST step's).  Worlds are independent and a wavefront owns whole worlds, so the world state stays in registers
 * between the steps: per step only the action slice is read and the outputs are written; the world buffer is updated
 * once.  The actions are pre-staged (scripted / open-loop runs; a policy in the loop: cavoid_step_autoreset or
 * cavoid_actor_run). */
int cavoid_step_autoreset_n(cavoid_env *env, const int32_t *actions, int64_t action_stride, int32_t n_steps, int64_t out_step_stride,
                            float *obs, float *rewards, uint8_t *done, uint8_t *game_over, void *stream);
/* Table actions outside [0, num_actions) are CLAMPED to that range by every stepping form (a negative index acts as 0, one at or
 * past num_actions as num_actions - 1); the action of a done or scripted agent is ignored.  This header is the definition: the
 * C oracle indexes the table without a clamp. */

/* which kernel form the last stepping launch of this handle ran (cavoid_step, _packed, _continuous and every
 * cavoid_step*_autoreset* entry point; reset and observe leave it alone, the actor does not report here and cavoid_step_push only
 * on an env of more than 16 agents per world: CAVOID_FORM_CROWD, or CAVOID_FORM_CROWD_RVO where ORCA agents may exist).
 * Several forms carry the same call and a form that does not carry a configuration hands it to the next one; all of them are
 * bit-identical to CAVOID_FORM_STEP.  relay_consumers (may be NULL) receives the
 * observation wavefronts per tile the relay launch really used (the launcher lowers CAVOID_RELAY_CONSUMERS until the LDS fits),
 * 0 for the other forms.  Returns CAVOID_FORM_NONE before the first stepping launch, when the last one failed, and for a NULL env. */
enum {
    CAVOID_FORM_NONE = 0,
    CAVOID_FORM_STEP = 1,      /* env_kernel, one step per launch, one wavefront per tile */
    CAVOID_FORM_QUAD = 2,      /* env_quad_kernel: one auto-reset step, four wavefronts per tile */
    CAVOID_FORM_RVO = 3,       /* the ORCA-carrying instantiations of cavoid_rvo.hip (any step mode) */
    CAVOID_FORM_LOOP_PF = 4,   /* env_kernel's in-launch step loop, next pool record in registers (MODE_STEP_AUTORESET_PF) */
    CAVOID_FORM_LOOP = 5,      /* env_kernel's in-launch step loop, restarts gathered on demand (MODE_STEP_AUTORESET_N) */
    CAVOID_FORM_PIPE = 6,      /* env_pipe_kernel: the step loop on two wavefronts per tile */
    CAVOID_FORM_RELAY = 7,     /* env_relay_kernel: the step loop cut into roles on 3 + relay_consumers wavefronts per tile */
    CAVOID_FORM_CROWD = 8,     /* crowd_kernel: every stepping mode of a world of 17..64 agents (one lane per agent, keys and ranks in LDS) */
    CAVOID_FORM_CROWD_RVO = 9  /* crowd_rvo_kernel: the same with ORCA agents solved by the whole wavefront (rvo_enabled = CAVOID_RVO_WAVE) */
};
int32_t cavoid_last_step_form(const cavoid_env *env, int32_t *relay_consumers);

/* Scenario look-ahead bookkeeping (gen_lookahead > 0), host side only, no synchronisation: refill_launches (may be NULL) receives how many
 * ahead_fill_kernel launches this handle has made so far (the first fill after create / seed / pool refresh, and every refill in front of
 * a launch whose form does not regenerate the consumed ring slots itself); budget (may be NULL) the restarts per world the rings are still
 * guaranteed to cover (0 before the first fill).  A relay launch (CAVOID_FORM_RELAY) of GEN v1 scenarios tops the rings up inside the
 * launch and needs no refill launch as long as n_steps <= gen_lookahead / 2.  Without look-ahead both stay 0. */
int cavoid_ahead_info(const cavoid_env *env, int64_t *refill_launches, int32_t *budget);

/* The env-level CONTINUOUS action space (run-ws/config.yaml:3-5, ACTION_SPACE_TYPE = 0: "continuous" at the gym level; SURVEY App. A:
 * the discretisation lives in the policy) in the auto-reset and K-step launch forms: float actions [n_steps][W,N,2] -- (speed,
 * heading change) for the unicycle dynamics, a velocity (vx, vy) for CAVOID_DYN_HOLONOMIC (which ONLY these entry points and
 * cavoid_step_continuous can step: it has no table actions) -- slice t at actions + t*action_stride FLOATS (>= 2*W*N, or 0 with
 * n_steps == 1); everything else as cavoid_step_autoreset / _n / _packed: in-kernel restarts from the pool, the look-ahead rings or the
 * in-step generator, every step's outputs in its own slot, scripted agents acting by their own rule.  (A continuous K-step launch
 * runs the single-wavefront step loop: the role-split and pipelined forms decode table actions.) */
int cavoid_step_continuous_autoreset(cavoid_env *env, const float *actions /* [W,N,2] */, float *obs, float *rewards, uint8_t *done,
                                     uint8_t *game_over, void *stream);
int cavoid_step_continuous_autoreset_n(cavoid_env *env, const float *actions, int64_t action_stride, int32_t n_steps, int64_t out_step_stride,
                                       float *obs, float *rewards, uint8_t *done, uint8_t *game_over, void *stream);

/* ---- packed outputs: one record per agent, [W, N, cavoid_packed_width()] floats = (obs row | reward | done) ----
 * The kernel assembles the record in its LDS tile and writes it with the same coalesced stores as the plain
 * observation: no separate reward / done arrays, no pack pass before the multi-GPU gather.  reset / observe write
 * reward 0 and the agents' current done state. */
int32_t cavoid_packed_width(const cavoid_env *env);
int cavoid_reset_packed(cavoid_env *env, const uint8_t *world_mask, float *packed, void *stream);
int cavoid_observe_packed(cavoid_env *env, float *packed, void *stream);
int cavoid_step_packed(cavoid_env *env, const int32_t *actions, float *packed, uint8_t *game_over, void *stream);
/* packed [n_steps, S, N, width + 2] and game_over [n_steps, S] with S = out_step_stride worlds, or one slot when it is 0 */
int cavoid_step_autoreset_packed(cavoid_env *env, const int32_t *actions, int64_t action_stride, int32_t n_steps, int64_t out_step_stride,
                                 float *packed, uint8_t *game_over, void *stream);
int cavoid_step_continuous_autoreset_packed(cavoid_env *env, const float *actions, int64_t action_stride, int32_t n_steps,
                                            int64_t out_step_stride, float *packed, uint8_t *game_over, void *stream);

/* ---- multi-GPU hand-over: ONE all-gather of every rank's packed shard (RCCL over xGMI) ------------------------------
 * One process per GPU, contiguous world ranges (rank r owns worlds [r*W, (r+1)*W)).  The communicator is created from
 * a 128-byte id made on rank 0 by cavoid_comm_unique_id and handed to the other ranks out of band (the host side uses
 * its process-group store).  cavoid_gather_begin(slot) enqueues, on the communicator's OWN stream, an ncclAllGather of
 * `floats_per_rank` floats from `send` into `recv` [nranks * floats_per_rank] after everything enqueued so far on
 * `producer_stream` (the step that wrote `send`); it returns at once.  cavoid_gather_wait(slot) makes a stream wait
 * for the last gather begun in that slot (no host synchronisation).  Two slots: with send / recv double-buffered and
 * slot = t % 2, step t+1 (writing the other buffer) overlaps gather t; before step t+2 re-uses the buffers the
 * producer stream waits on the slot.  With nranks == 1 the gather is a device copy (unless CAVOID_COMM_FORCE_RCCL, below).
 * Errors: CAVOID_ECOMM (see cavoid_last_comm_error). */
typedef struct cavoid_comm cavoid_comm;
#define CAVOID_COMM_ID_BYTES 128
#define CAVOID_COMM_SLOTS 2
int cavoid_comm_unique_id(void *id_out);
int cavoid_comm_create(const void *unique_id, int32_t nranks, int32_t rank, int device, cavoid_comm **out);
/* flags: CAVOID_COMM_FORCE_RCCL = a ONE-rank communicator is a real RCCL communicator too (ncclCommInitRank with nranks = 1;
 * cavoid_gather_begin issues ncclAllGather, cavoid_gatherv_begin a grouped ncclSend / ncclRecv to itself) instead of the device
 * copy -- a development switch that lets a 1-GPU box execute the very calls a multi-rank communicator makes.  unique_id may be
 * NULL for one rank (an id is made internally).  cavoid_comm_create = this with flags 0, or CAVOID_COMM_FORCE_RCCL when the
 * environment variable CAVOID_COMM_FORCE_RCCL is set to anything but "" / "0".  Unknown flag bits: CAVOID_EINVAL. */
#define CAVOID_COMM_FORCE_RCCL 1u
int cavoid_comm_create_ex(const void *unique_id, int32_t nranks, int32_t rank, int device, uint32_t flags, cavoid_comm **out);
/* what the handle is: any of the out pointers may be NULL.  uses_rccl = 1 when the gathers go through RCCL (0 = one rank, device
 * copy); rccl_version = ncclGetVersion() of the library bound (0 when uses_rccl is 0). */
int cavoid_comm_info(const cavoid_comm *comm, int32_t *nranks, int32_t *rank, int32_t *uses_rccl, int32_t *rccl_version);
void cavoid_comm_destroy(cavoid_comm *comm);
int cavoid_gather_begin(cavoid_comm *comm, int32_t slot, const float *send, float *recv, int64_t floats_per_rank,
                        void *producer_stream);
/* the same hand-over for RAGGED shards and / or to ONE rank: counts[r] (host array [nranks], identical on every rank) = floats of
 * rank r's shard; recv [sum(counts)] holds the shards in rank order.  root < 0: every rank receives every shard; root >= 0:
 * only that rank does (the trainer rank of the full GA3C loop; recv may be NULL on the others).  Point-to-point sends inside
 * one RCCL group: on the fully connected xGMI mesh every shard travels over its own link (a direct gather, no padding). */
int cavoid_gatherv_begin(cavoid_comm *comm, int32_t slot, const float *send, float *recv, const int64_t *counts, int32_t root,
                         void *producer_stream);
int cavoid_gather_wait(cavoid_comm *comm, int32_t slot, void *consumer_stream);
int cavoid_last_comm_error(void);               /* raw ncclResult_t of the last CAVOID_ECOMM */

/* as cavoid_step_autoreset_n in launches of `steps_per_launch` steps, every launch carrying its own HIP start/stop
 * event pair (recorded with the dispatch, so launch gaps are excluded); synchronises and returns the MEAN duration
 * of a launch in milliseconds.  Measurement aid for bench.py's roofline figure. */
int cavoid_step_autoreset_n_timed(cavoid_env *env, const int32_t *actions, int64_t action_stride, int32_t n_steps,
                                  int32_t steps_per_launch, int64_t out_step_stride, float *obs, float *rewards, uint8_t *done,
                                  uint8_t *game_over, void *stream, float *mean_launch_ms);

/* the (world, agent) slots whose agent runs scripted policy `policy_id` (CAVOID_POLICY_*) and is present and, with
 * only_running != 0, not done: row_index int32 [W*N] (unspecified order), row_count int32 [1], both on the device (feed them
 * to cavoid_policy_forward_rows of the frozen network that drives CAVOID_POLICY_FROZEN_NET agents). */
int cavoid_policy_rows(cavoid_env *env, int32_t policy_id, int32_t only_running, int32_t *row_index, int32_t *row_count, void *stream);

/* ---- batched GA3C actor bookkeeping (rollout) -------------------------------------------------------
 * Stands in for one ProcessAgent per world: ProcessAgent.run_episode / _accumulate_rewards /
 * convert_to_nparray (ga3c/GA3C/ProcessAgent.py:54-87,105-211) and the training_q / episode_log_q
 * puts (:238,243).  cavoid_rollout_push records one env step for every learning (world, agent) slot
 * in a caller-owned TIME-MAJOR experience store of `ring_len` step blocks (block = step % ring_len):
 *   x float [ring_len,W*N,D] (state the policy acted on), val double [ring_len,W*N] (the step's reward),
 *   ret float [ring_len,W*N] (n-step return y_r the row was emitted with), act u8, emit_t int32 (-1 = pending
 *   or nothing recorded, >= 0 = a training row, emitted at that step).  A block is final once it is older than
 *   time_max + 1 steps; the caller compacts the emit_t >= 0 rows of final blocks into (x, y_r, action) batches
 *   (the trainer's one-hot is eye(num_actions)[act]).
 *   prev_obs float [W,N,1+D] = the observation the policy acted on (Environment.previous_state plus col 0),
 *   actions int32 [W,N], values float [W,N] (V(s_t)), rewards/done/game_over = what the step returned.
 *   dup_* : append buffer for the rows only the reference's post-done re-flush quirk produces
 *   (reflush_done = 1: a done agent that is still reported learning re-emits its kept experience with
 *   every later step); dup_count int32 [2] = (rows OFFERED: stored plus dropped, rows dropped for lack
 *   of capacity), reset by the caller.  The rows stored are the first min(dup_count[0], dup_capacity) of dup_*: read no further.
 *   ep_out float [ep_capacity,3] (world, total_reward, total_length), ep_count int32 [2] = (records offered, records dropped) in
 *   the same sense: min(ep_count[0], ep_capacity) records are stored.  Nothing is written behind either capacity.
 *   step < 0: use (and advance) the handle's device-side step counter (hipGraph replays). */
int cavoid_rollout_create(int64_t num_worlds, int32_t max_agents, int32_t obs_width, int32_t time_max, double discount,
                          int32_t reflush_done, int32_t ring_len, int device, cavoid_rollout **out);
void cavoid_rollout_destroy(cavoid_rollout *r);
int cavoid_rollout_reset(cavoid_rollout *r, void *stream);
int cavoid_rollout_push(cavoid_rollout *r, const float *prev_obs, const int32_t *actions, const float *values,
                        const float *rewards, const uint8_t *done, const uint8_t *game_over, int32_t step,
                        float *x, double *val, float *ret, uint8_t *act, int32_t *emit_t,
                        float *dup_x, float *dup_r, int32_t *dup_a, int32_t *dup_src, int32_t *dup_count, int64_t dup_capacity,
                        float *ep_out, int32_t *ep_count, int64_t ep_capacity, void *stream);

/* ---- the fused actor: K closed-loop steps of EVERY world in ONE launch ------------------------------------------------
 * observe -> predict_p_and_v -> select_action -> env.step -> Experience bookkeeping, K times (ProcessAgent.run_episode's loop body,
 * ga3c/GA3C/ProcessAgent.py:116-211, with the ThreadPredictor round trip of :89-96 and ThreadPredictor.py:61-75 inside it): per
 * tile of floor(64/N) worlds a workgroup runs cavoid_policy_forward's arithmetic on the tile's rows, draws the actions, steps
 * the tile's worlds (cavoid_step_autoreset's arithmetic) and records the step (cavoid_rollout_push's arithmetic) -- no kernel
 * boundary, no host, nothing between workgroups.  Results are bit-identical to calling those three entry points K times.
 *   obs_cur [W,N,1+D]: the observation to act on first; obs_next: a second buffer of the same shape -- step t reads one and
 *   writes the other, so after the call the current observation is in obs_cur when n_steps is even, in obs_next when odd.
 *   rewards / done / game_over / actions int32 [W,N] / values float [W,N]: per-step OUTPUTS, holding the LAST step's afterwards; they are
 *   never read (which rows need an action at a launch's first step is derived from the world state's own flags, so a cavoid_reset -- masked
 *   or not --, a cavoid_set_state or fresh buffers between two launches are all fine).
 *   The network runs only for the rows that still need an action -- what cavoid_rollout_active_rows lists: a learning agent (obs
 *   column 0) that was not done in the step that produced the observation, or whose world has just restarted; a finished agent
 *   waits for its world's last learning agent, a scripted agent acts by its own rule, the env ignores what either is given -- and
 *   the other rows are handed action 0 / value 0, like cavoid_policy_forward_rows' pass over that list (nothing reads them; the
 *   experience store's action entry of such a row is 0).  With reflush_done (the reference's re-flush quirk reads a done agent's
 *   value) and in cavoid_actor_run_mix every row runs.
 *   buffers: the experience store of cavoid_rollout_push.  The policy's launch counter and the rollout's step counter advance
 *   by n_steps on the device (the call can sit in a hipGraph).
 * Worlds with ORCA agents (rvo_enabled) and GEN v2 scenarios generated inside the step run over the env step's ORCA instantiation,
 * as in cavoid_step_autoreset.
 * CAVOID_EUNSUPPORTED (use the step-by-step entry points): holonomic dynamics, CAVOID_POLICY_F32 / a non-default
 * CAVOID_POLICY_PRODUCTS, a policy (or frozen) handle of more than 19 observed agents (a crowd handle: an env of <= 16 agents padded
 * wider), rvo_enabled with so many agents per world (> 12) that the ORCA lines do not fit into the LDS the policy lends the env step.  Frozen-network agents (CAVOID_POLICY_FROZEN_NET) act by a SECOND network: cavoid_actor_run_mix carries it;
 * this entry point refuses an env whose generator makes such agents (gen_frozen_fraction > 0 with gen_nonlearning_fraction > 0).  The
 * refusal looks at the GENERATOR's fractions only: frozen-network agents put into the worlds some other way -- cavoid_set_state, or a
 * scenario pool filled under another configuration -- are NOT detected here and would be handed the learner's sampled action; callers
 * that inject such agents must use cavoid_actor_run_mix.
 * Side effect: like every entry point that launches, the call leaves the CALLER's current HIP device set to the env's device. */
typedef struct cavoid_rollout_buffers {
    int32_t struct_size;             /* sizeof(cavoid_rollout_buffers) */
    int32_t reserved;
    float *x; double *val; float *ret; uint8_t *act; int32_t *emit_t;               /* the rings of cavoid_rollout_push */
    float *dup_x; float *dup_r; int32_t *dup_a; int32_t *dup_src; int32_t *dup_count; int64_t dup_capacity;
    float *ep_out; int32_t *ep_count; int64_t ep_capacity;
} cavoid_rollout_buffers;
int cavoid_actor_run(cavoid_env *env, cavoid_policy *policy, cavoid_rollout *rollout, const cavoid_rollout_buffers *buffers,
                     float *obs_cur, float *obs_next, float *rewards, uint8_t *done, uint8_t *game_over, int32_t *actions, float *values,
                     int32_t n_steps, int32_t greedy, void *stream);

/* cavoid_actor_run for the reference's TRAINING MIX (static / non-cooperative / RVO / CADRL agents around the learners,
 * ga3c/GA3C/checkpoints/RL/wandb/run-2018-backup/checkpoints/index.txt:1-3; the CADRL agent is a frozen network, ga3c/GA3C/Server.py:36):
 * `frozen` = a second cavoid_policy handle (same shapes, its own weights) that drives the CAVOID_POLICY_FROZEN_NET agents.  A tile that holds a
 * running frozen-network agent runs the forward pass once more on `frozen`'s weights and takes its ARGMAX for exactly those rows -- what the
 * step-by-step form does with cavoid_policy_rows + cavoid_policy_forward_rows(greedy) -- inside the same launch; other tiles skip it.
 * Runs over the env step's ORCA instantiation (ORCA agents and in-step box scenarios included).  Bit-identical to the step-by-step
 * form.  CAVOID_EUNSUPPORTED as cavoid_actor_run, and for a `frozen` handle of another inference form (CAVOID_POLICY_PRODUCTS / _F32). */
int cavoid_actor_run_mix(cavoid_env *env, cavoid_policy *policy, cavoid_policy *frozen, cavoid_rollout *rollout,
                         const cavoid_rollout_buffers *buffers, float *obs_cur, float *obs_next, float *rewards, uint8_t *done, uint8_t *game_over,
                         int32_t *actions, float *values, int32_t n_steps, int32_t greedy, void *stream);

/* cavoid_actor_run for CROWD worlds (17..64 agents per world; cavoid_actor_run and _run_mix refuse them): the same closed loop, K steps in one
 * launch, over the crowd step form -- per tile of floor(64/N) worlds (at most 64 rows: one policy tile) a workgroup runs cavoid_policy_forward's
 * arithmetic on the tile's rows with the input slots used as a ring (rows of up to 63 observed agents), draws the actions, steps the tile's worlds
 * (cavoid_step_push's crowd launch: env step + Experience bookkeeping + episode log) and copies the step's state rows into the experience store.
 * Arguments, buffers, counters and the rule for the rows that need an action exactly as cavoid_actor_run; results are bit-identical to the
 * step-by-step entry points (cavoid_rollout_active_rows, cavoid_policy_forward[_rows], cavoid_step_push).  With rvo_enabled = CAVOID_RVO_WAVE
 * the launch runs over the ORCA-carrying env step; afterwards cavoid_last_step_form reports CAVOID_FORM_CROWD / CAVOID_FORM_CROWD_RVO as after
 * cavoid_step_push.  `policy`: an LSTM handle (cavoid_policy_create) of the default inference form whose max_other is the env's, 1..63.
 * CAVOID_EINVAL: null or mismatching handles and buffers (cavoid_actor_run's checks).  CAVOID_EUNSUPPORTED (use the step-by-step entry
 * points): an env of <= 16 agents per world (cavoid_actor_run carries those), a weight-sharing handle (cavoid_crowd_actor_run_ws carries it), holonomic dynamics,
 * CAVOID_POLICY_F32 / a non-default CAVOID_POLICY_PRODUCTS (the bf16 product form included), and an env whose generator makes frozen-network
 * agents (gen_frozen_fraction > 0 with gen_nonlearning_fraction > 0: this launch carries one network, cavoid_crowd_actor_run_mix carries the
 * second; the refusal looks at the generator's fractions only, as cavoid_actor_run's).  n_steps == 0: CAVOID_OK, nothing is launched. */
int cavoid_crowd_actor_run(cavoid_env *env, cavoid_policy *policy, cavoid_rollout *rollout, const cavoid_rollout_buffers *buffers,
                           float *obs_cur, float *obs_next, float *rewards, uint8_t *done, uint8_t *game_over, int32_t *actions, float *values,
                           int32_t n_steps, int32_t greedy, void *stream);

/* cavoid_actor_run_mix for CROWD worlds (17..64 agents per world; cavoid_actor_run_mix refuses them, cavoid_crowd_actor_run refuses an env whose
 * generator makes frozen-network agents): cavoid_crowd_actor_run's closed loop, K steps in one launch, with `frozen` = a second LSTM handle
 * (same shapes, its own weights) that drives the CAVOID_POLICY_FROZEN_NET agents.  Per step, after the learner's pass, a tile that holds a
 * RUNNING frozen-network agent (present, policy 4, no terminal flag in the state before this step -- what cavoid_policy_rows lists) runs the
 * same ring pass once more on `frozen`'s weights and takes its ARGMAX for exactly those rows; values[] of those rows stays what the learner's
 * pass left (0 for a row that needs no action).  Other tiles skip the second pass, and a tile without a row that needs the learner's action
 * skips the first.  The argument list is cavoid_actor_run_mix's; buffers, counters, the rule for the rows that need an action, the ORCA
 * routing and cavoid_last_step_form exactly as cavoid_crowd_actor_run.  Bit-identical to the step-by-step entry points
 * (cavoid_rollout_active_rows, cavoid_policy_forward[_rows], cavoid_policy_rows + cavoid_policy_forward_rows on `frozen`, cavoid_step_push).
 * An env whose generator makes no frozen-network agents is accepted: the second pass then never runs.
 * CAVOID_EINVAL: null handles (`frozen` included), buffers or pointers, a wrong struct_size, n_steps < 0 -- looked at before n_steps == 0 --, a
 * handle that is not loaded, handles that do not describe the same batch.  CAVOID_EUNSUPPORTED (use the step-by-step entry points): an env of
 * <= 16 agents per world (cavoid_actor_run_mix carries those), a weight-sharing handle as `policy` or as `frozen`, CAVOID_POLICY_F32 / a
 * non-default CAVOID_POLICY_PRODUCTS on either handle (the bf16 product form included), a `frozen` handle whose max_other, input size or action
 * count differ from the policy's, a policy whose max_other is not the env's, holonomic dynamics, an env with scenario look-ahead rings, and a
 * crowd env step whose LDS exceeds what cavoid_crowd_actor_run's launch allows.  n_steps == 0: CAVOID_OK, nothing is launched. */
int cavoid_crowd_actor_run_mix(cavoid_env *env, cavoid_policy *policy, cavoid_policy *frozen, cavoid_rollout *rollout,
                               const cavoid_rollout_buffers *buffers, float *obs_cur, float *obs_next, float *rewards, uint8_t *done,
                               uint8_t *game_over, int32_t *actions, float *values, int32_t n_steps, int32_t greedy, void *stream);

/* cavoid_actor_run for the WEIGHT-SHARING network (cavoid_policy_create_ws; cavoid_actor_run, _run_mix and cavoid_crowd_actor_run refuse such a
 * handle): the same closed loop, K steps in one launch -- per tile of floor(64/N) worlds a workgroup runs the weight-sharing pass
 * (cavoid_policy_forward's arithmetic on a weight-sharing handle: float32 MFMA) on the tile's rows, draws the actions, steps the tile's worlds and
 * records the step.  Arguments, buffers, counters, the ORCA / in-step box routing and the rule for the rows that need an action exactly as
 * cavoid_actor_run; results are bit-identical to the step-by-step entry points (cavoid_rollout_active_rows, cavoid_policy_forward[_rows],
 * cavoid_step_push).  `policy`: a loaded cavoid_policy_create_ws handle whose max_other (1..19) is the env's.
 * CAVOID_EINVAL: null or mismatching handles and buffers (cavoid_actor_run's checks).  CAVOID_EUNSUPPORTED (use the step-by-step entry
 * points): an LSTM handle (cavoid_actor_run carries it), a cavoid_policy_create_ws_crowd handle (the ring form, 20..64 observed agents), an env of
 * more than 16 agents per world (cavoid_crowd_actor_run_ws carries crowd worlds, with either weight-sharing handle), holonomic dynamics, an env whose generator makes frozen-network agents (gen_frozen_fraction > 0 with
 * gen_nonlearning_fraction > 0: one network per launch, no _mix form; the refusal looks at the generator's fractions only, as
 * cavoid_actor_run's), and an env step whose LDS (with rvo_enabled: the ORCA lines) does not fit the 66 560 bytes of activation rows the pass
 * lends it.  n_steps == 0: CAVOID_OK, nothing is launched. */
int cavoid_actor_run_ws(cavoid_env *env, cavoid_policy *policy, cavoid_rollout *rollout, const cavoid_rollout_buffers *buffers,
                        float *obs_cur, float *obs_next, float *rewards, uint8_t *done, uint8_t *game_over, int32_t *actions, float *values,
                        int32_t n_steps, int32_t greedy, void *stream);

/* cavoid_actor_run_ws for CROWD worlds (17..64 agents per world): the same closed loop, K steps in one launch, over the crowd step form -- per
 * tile of floor(64/N) worlds (at most 64 rows: one policy tile) a workgroup runs the weight-sharing pass on the tile's rows that need an action
 * with the input slots used as a ring (rows of up to 63 observed agents; with 19 or fewer no slot is refilled), draws the actions, steps the
 * tile's worlds (cavoid_step_push's crowd launch: env step + Experience bookkeeping + episode log) and copies the step's state rows into the
 * experience store.  Arguments, buffers, counters and the rule for the rows that need an action exactly as cavoid_actor_run; results are
 * bit-identical to the step-by-step entry points (cavoid_rollout_active_rows, cavoid_policy_forward[_rows], cavoid_step_push).  With rvo_enabled =
 * CAVOID_RVO_WAVE the launch runs over the ORCA-carrying env step; afterwards cavoid_last_step_form reports CAVOID_FORM_CROWD /
 * CAVOID_FORM_CROWD_RVO as after cavoid_step_push.  `policy`: a loaded weight-sharing handle whose max_other is the env's -- cavoid_policy_create_ws
 * (1..19) or cavoid_policy_create_ws_crowd (20..64): one kernel serves both.
 * CAVOID_EINVAL: null or mismatching handles and buffers (cavoid_crowd_actor_run's checks).  CAVOID_EUNSUPPORTED (use the step-by-step entry
 * points): an env of <= 16 agents per world (cavoid_actor_run_ws carries those), an LSTM handle (cavoid_crowd_actor_run carries it), holonomic
 * dynamics (velocity actions), an env whose generator makes frozen-network agents (gen_frozen_fraction > 0 with gen_nonlearning_fraction > 0:
 * one network per launch, no _mix form; the refusal looks at the generator's fractions only, as cavoid_actor_run's), an env with scenario
 * look-ahead rings, and a crowd env step whose LDS exceeds 64 KiB or the 66 560 bytes of activation rows the pass lends it.
 * n_steps == 0: CAVOID_OK, nothing is launched. */
int cavoid_crowd_actor_run_ws(cavoid_env *env, cavoid_policy *policy, cavoid_rollout *rollout, const cavoid_rollout_buffers *buffers,
                              float *obs_cur, float *obs_next, float *rewards, uint8_t *done, uint8_t *game_over, int32_t *actions, float *values,
                              int32_t n_steps, int32_t greedy, void *stream);

/* ---- evaluation: K greedy (or sampled) steps of every world in ONE launch, with outcome records ------------------------------------
 * The EVALUATE_MODE loop (argmax actions, ga3c/GA3C/ProcessAgent.py:98-103; every agent of a world must finish) without the host in it:
 * per tile of floor(64/N) worlds a workgroup runs cavoid_policy_forward's arithmetic on the tile's rows that still need an action (a
 * learning agent whose state carries no terminal flag; the other rows are handed action 0 / value 0), steps the tile's worlds WITHOUT
 * auto-reset (cavoid_step's arithmetic: a world that is over stays as it is) and records the outcome -- up to n_steps times, and a tile
 * whose worlds are all over leaves the loop at once.  "Over" is cavoid_step's game_over: no learning agent -- with evaluate_mode no agent
 * at all -- of the world is still running; at the first step of a launch it is read from the world state's flags, so a launch on
 * finished worlds does nothing, and a chain of launches continues where the last one stopped.  Trajectories are bit-identical to calling
 * cavoid_policy_forward (+ cavoid_policy_forward_rows on `frozen` for the CAVOID_POLICY_FROZEN_NET rows) and cavoid_step per step.
 *   obs [W,N,1+D]: the current observation on entry (cavoid_reset's, or the last launch's); every step writes the next one into the SAME
 *   buffer, so on return it holds, per tile, the observation after that tile's last step.
 *   rewards / done / game_over / actions int32 [W,N] / values float [W,N]: per-step outputs, per tile its last step's; never read.
 *   buffers: the records, caller-owned device memory that the caller zeroes before an episode's first launch; read at a tile's first
 *   step of the launch and written back when it leaves.
 *     ret double [W*N]         An agent's return sums the rewards up to and including the step at which its world is over.
 *                              (float64, added in step order.  Rewards cavoid_step would go on paying a finished world -- with a
 *                              reward_time_step every step -- are NOT in it: the kernel never takes those steps.)
 *     goal_step int32 [W*N]    the world's step count at the step that first left the agent with CAVOID_F_AT_GOAL (time to goal =
 *                              goal_step * dt); 0: not reached
 *     world_steps int32 [W]    steps the world has taken = the step at which it was over, once it is
 *     worlds_running int32 [1] OUTPUT: worlds not over when their tile left this launch.  Zeroed by the call on the stream, then one
 *                              atomic add per tile; read it after the launch to decide whether another one is needed.
 *   greedy != 0: argmax; 0: the Philox draw of cavoid_policy_forward for (seed, row, step counter + t).  The policy's step counter
 *   advances by n_steps on the device, whatever the tiles did.
 * Routing as cavoid_actor_run / _run_mix: rvo_enabled (and in-step box scenarios) run over the env step's ORCA instantiation, a `frozen`
 * handle (may be NULL) drives the frozen-network agents by its argmax; CAVOID_ACTOR_QUAD applies.  The scenario look-ahead is not
 * touched: nothing restarts.
 * CAVOID_EINVAL: null handles, buffers or record pointers, a wrong struct_size, handles that do not describe the same batch
 * (cavoid_actor_run's checks).  CAVOID_EUNSUPPORTED (evaluate step by step): exactly what cavoid_actor_run / _run_mix refuse -- a
 * weight-sharing handle, more than 16 agents per world, a policy (or frozen) handle of more than 19 observed agents, holonomic dynamics,
 * CAVOID_POLICY_F32 / a non-default CAVOID_POLICY_PRODUCTS, an env step whose LDS does not fit what the policy lends it, and an env whose
 * generator makes frozen-network agents when `frozen` is NULL.  n_steps == 0: CAVOID_OK, nothing is launched or written. */
typedef struct cavoid_eval_buffers {
    int32_t struct_size;             /* sizeof(cavoid_eval_buffers) */
    double *ret;                     /* [W*N] */
    int32_t *goal_step;              /* [W*N] */
    int32_t *world_steps;            /* [W] */
    int32_t *worlds_running;         /* [1] */
} cavoid_eval_buffers;
int cavoid_eval_run(cavoid_env *env, cavoid_policy *policy, cavoid_policy *frozen /* or NULL */, const cavoid_eval_buffers *buffers,
                    float *obs, float *rewards, uint8_t *done, uint8_t *game_over, int32_t *actions, float *values, int32_t n_steps,
                    int32_t greedy, void *stream);

/* cavoid_eval_run for the WEIGHT-SHARING network (cavoid_policy_create_ws; cavoid_eval_run refuses such a handle): the same evaluation loop,
 * up to n_steps steps in one launch that finished tiles leave early -- per tile of floor(64/N) worlds a workgroup runs the weight-sharing
 * pass (cavoid_policy_forward's arithmetic on a weight-sharing handle: float32 MFMA) on the tile's rows that still need an action, takes
 * the argmax (or the Philox draw), steps the tile's worlds without auto-reset and records the outcome.  Arguments, buffers, records, the
 * definition of "over", the step counter, the ORCA / in-step box routing and CAVOID_ACTOR_QUAD exactly as cavoid_eval_run; in particular
 * the same definition of the return: An agent's return sums the rewards up to and including the step at which its world is over.
 * Trajectories are bit-identical to calling cavoid_policy_forward (+ cavoid_policy_forward_rows on `frozen` for the
 * CAVOID_POLICY_FROZEN_NET rows) and cavoid_step per step.
 *   policy: a loaded cavoid_policy_create_ws handle whose max_other (1..19) is the env's.
 *   frozen (may be NULL): a loaded cavoid_policy_create_ws handle of the same max_other, input size and action count; it drives the
 *   frozen-network agents by its argmax.  values[] of those rows then holds the frozen network's value (nothing reads it).
 * CAVOID_EINVAL: cavoid_eval_run's cases -- null handles, buffers or record pointers, a wrong struct_size, n_steps < 0, handles that do not
 * describe the same batch, a handle that is not loaded.  CAVOID_EUNSUPPORTED (evaluate step by step): an LSTM handle (cavoid_eval_run carries
 * it), a cavoid_policy_create_ws_crowd handle (the ring form, 20..64 observed agents), an env of more than 16 agents per world, holonomic
 * dynamics, a `frozen` handle that is not a matching whole-row weight-sharing handle, an env whose generator makes frozen-network agents
 * when `frozen` is NULL (gen_frozen_fraction > 0 with gen_nonlearning_fraction > 0), and an env step whose LDS (with rvo_enabled: the ORCA
 * lines) does not fit the 66 560 bytes of activation rows the pass lends it.  n_steps == 0: CAVOID_OK, nothing is launched or written. */
int cavoid_eval_run_ws(cavoid_env *env, cavoid_policy *policy, cavoid_policy *frozen /* or NULL */, const cavoid_eval_buffers *buffers,
                       float *obs, float *rewards, uint8_t *done, uint8_t *game_over, int32_t *actions, float *values, int32_t n_steps,
                       int32_t greedy, void *stream);

/* cavoid_eval_run for CROWD worlds (17..64 agents per world; cavoid_eval_run refuses them): the same evaluation loop, up to n_steps steps in
 * one launch that finished tiles leave early, over the crowd step form -- per tile of floor(64/N) worlds (at most 64 rows: one policy tile) a
 * workgroup runs cavoid_policy_forward's arithmetic on the tile's rows with the input slots used as a ring (rows of up to 63 observed agents;
 * the pass runs while one row of the tile still needs an action, and only those rows take its result: the others are handed action 0 /
 * value 0), takes the argmax (or the Philox draw), steps the tile's worlds without auto-reset (cavoid_step's crowd launch) and records the
 * outcome.  There is no `frozen` argument; `buffers` is cavoid_eval_run's struct, unchanged.  The records, the definition of "over", the
 * return, the worlds_running protocol (zeroed on the stream by the call) and the step counter are exactly cavoid_eval_run's.  The return,
 * once more, as the two blocks above define it: An agent's return sums the rewards up to and including the step
 * at which its world is over.
 * Trajectories are bit-identical to calling cavoid_policy_forward and cavoid_step per step.  With rvo_enabled = CAVOID_RVO_WAVE the launch
 * runs over the ORCA-carrying env step; afterwards cavoid_last_step_form reports CAVOID_FORM_CROWD / CAVOID_FORM_CROWD_RVO, as after
 * cavoid_step on such an env.  `policy`: a loaded LSTM handle (cavoid_policy_create) of the default inference form whose max_other is the
 * env's, 1..63.
 * CAVOID_EINVAL: cavoid_eval_run's cases -- null handles, buffers or record pointers, a wrong struct_size, n_steps < 0, a handle that is not
 * loaded, handles that do not describe the same batch.  CAVOID_EUNSUPPORTED (evaluate step by step): what cavoid_crowd_actor_run refuses -- an
 * env of <= 16 agents per world (cavoid_eval_run carries those), a weight-sharing handle, holonomic dynamics, CAVOID_POLICY_F32 / a
 * non-default CAVOID_POLICY_PRODUCTS (the bf16 product form included), an env whose generator makes frozen-network agents
 * (gen_frozen_fraction > 0 with gen_nonlearning_fraction > 0: one network per launch; cavoid_crowd_eval_run_mix carries the second), and an env
 * step whose LDS exceeds what cavoid_crowd_actor_run's launch allows.  n_steps == 0: CAVOID_OK, nothing is launched or written. */
int cavoid_crowd_eval_run(cavoid_env *env, cavoid_policy *policy, const cavoid_eval_buffers *buffers, float *obs, float *rewards,
                          uint8_t *done, uint8_t *game_over, int32_t *actions, float *values, int32_t n_steps, int32_t greedy, void *stream);

/* cavoid_crowd_eval_run with a FROZEN network: cavoid_eval_run's `frozen` argument for CROWD worlds (17..64 agents per world) -- the same
 * evaluation loop, up to n_steps steps in one launch that finished tiles leave early, and per step, after the learner's pass, a tile that
 * holds a RUNNING frozen-network agent (CAVOID_POLICY_FROZEN_NET, present, no terminal flag in the state before this step -- what
 * cavoid_policy_rows lists) runs the same ring pass once more on `frozen`'s weights and takes its ARGMAX for exactly those rows.  The learner's
 * pass is skipped while no row of the tile needs its action; the frozen pass runs all the same (with evaluate_mode a frozen-network agent can
 * outlive every learner of its tile).  values[] is not written by the frozen pass.  The argument list is cavoid_eval_run's with `frozen`
 * REQUIRED; `buffers` is cavoid_eval_run's struct, unchanged.  The records, the definition of "over", the return, the worlds_running protocol
 * (zeroed on the stream by the call) and the step counter are exactly cavoid_eval_run's.  The return, as the blocks above define it: An
 * agent's return sums the rewards up to and including the step
 * at which its world is over.
 * Trajectories are bit-identical to calling cavoid_policy_forward, cavoid_policy_rows + cavoid_policy_forward_rows on `frozen`, and
 * cavoid_step per step.  ORCA routing and cavoid_last_step_form as cavoid_crowd_eval_run.  An env whose generator makes no frozen-network
 * agents is accepted: the second pass then never runs.
 * CAVOID_EINVAL: null handles (`frozen` included), buffers or record pointers, a wrong struct_size, n_steps < 0 -- looked at before
 * n_steps == 0 --, a handle that is not loaded, handles that do not describe the same batch.  CAVOID_EUNSUPPORTED (evaluate step by step): an
 * env of <= 16 agents per world (cavoid_eval_run carries those), a weight-sharing handle as `policy` or as `frozen` (cavoid_crowd_eval_run_ws
 * carries those), CAVOID_POLICY_F32 / a non-default CAVOID_POLICY_PRODUCTS on either handle (the bf16 product form included), a `frozen`
 * handle whose max_other, input size or action count differ from the policy's, a policy whose max_other is not the env's, holonomic
 * dynamics, an env with scenario look-ahead rings, and an env step whose LDS exceeds what cavoid_crowd_actor_run's launch allows.
 * n_steps == 0: CAVOID_OK, nothing is launched or written. */
int cavoid_crowd_eval_run_mix(cavoid_env *env, cavoid_policy *policy, cavoid_policy *frozen, const cavoid_eval_buffers *buffers, float *obs,
                              float *rewards, uint8_t *done, uint8_t *game_over, int32_t *actions, float *values, int32_t n_steps,
                              int32_t greedy, void *stream);

/* cavoid_eval_run_ws for CROWD worlds (17..64 agents per world; cavoid_eval_run_ws refuses them): the evaluation loop of the WEIGHT-SHARING
 * network over the crowd step form, up to n_steps steps in one launch that finished tiles leave early -- per tile of floor(64/N) worlds (at
 * most 64 rows: one policy tile) a workgroup lists the tile's rows that still need an action, runs the weight-sharing pass on them
 * (cavoid_policy_forward's arithmetic on a weight-sharing handle: float32 MFMA, the input slots used as a ring: rows of up to 63 observed
 * agents), takes the argmax (or the Philox draw), steps the tile's worlds without auto-reset (cavoid_step's crowd launch) and records the
 * outcome.  Rows that need no action (a finished agent, a scripted agent, an absent slot) are handed action 0 / value 0.  The argument list
 * is cavoid_eval_run_ws's; `buffers` is cavoid_eval_run's struct, unchanged.  The records, the definition of "over", the return, the
 * worlds_running protocol (zeroed on the stream by the call) and the step counter are exactly cavoid_eval_run's.  The return, as the
 * blocks above define it: An agent's return sums the rewards up to and including the step
 * at which its world is over.
 * Trajectories are bit-identical to calling cavoid_policy_forward (+ cavoid_policy_forward_rows on `frozen` for the
 * CAVOID_POLICY_FROZEN_NET rows) and cavoid_step per step.  With rvo_enabled = CAVOID_RVO_WAVE the launch runs over the ORCA-carrying env
 * step; afterwards cavoid_last_step_form reports CAVOID_FORM_CROWD / CAVOID_FORM_CROWD_RVO, as after cavoid_step on such an env.  The
 * scenario look-ahead is not touched: nothing restarts.
 *   policy: a loaded weight-sharing handle whose max_other is the env's -- cavoid_policy_create_ws (1..19 observed agents) or
 *   cavoid_policy_create_ws_crowd (20..64): one kernel serves both.
 *   frozen (may be NULL): a loaded weight-sharing handle of either kind with the same max_other, input size and action count; it drives
 *   the frozen-network agents by its argmax in a second pass on their rows (the first crowd launch that carries them).  values[] of those
 *   rows then holds the frozen network's value (nothing reads it).
 * CAVOID_EINVAL: cavoid_eval_run's cases -- null handles, buffers or record pointers, a wrong struct_size, n_steps < 0, a handle that is not
 * loaded, handles that do not describe the same batch.  CAVOID_EUNSUPPORTED (evaluate step by step): an LSTM handle (cavoid_crowd_eval_run
 * carries it), a handle of more than 64 observed agents, an env of <= 16 agents per world (cavoid_eval_run_ws carries those), holonomic
 * dynamics, a `frozen` handle that is not a matching weight-sharing handle, an env whose generator makes frozen-network agents when `frozen`
 * is NULL (gen_frozen_fraction > 0 with gen_nonlearning_fraction > 0), and a crowd env step whose LDS exceeds 65 536 bytes or the 66 560
 * bytes of activation rows the pass lends it.  n_steps == 0: CAVOID_OK, nothing is launched or written. */
int cavoid_crowd_eval_run_ws(cavoid_env *env, cavoid_policy *policy, cavoid_policy *frozen /* or NULL */, const cavoid_eval_buffers *buffers,
                             float *obs, float *rewards, uint8_t *done, uint8_t *game_over, int32_t *actions, float *values, int32_t n_steps,
                             int32_t greedy, void *stream);

/* cavoid_step_autoreset + cavoid_rollout_push as ONE launch: the env step of every world and the Experience bookkeeping of its slots
 * (ProcessAgent.py:149-211) -- the fused actor's env phase for actors whose policy is a launch of its own (frozen-network agents,
 * a caller-supplied policy).  obs_cur [W,N,1+D]: the observation `actions` / `values` (V(s_t)) were computed on; the step writes the
 * next one into obs_next (a different buffer) and rewards / done / game_over; buffers: the experience store of cavoid_rollout_push;
 * step as there (< 0: the handle's device-side counter, advanced by the call).  Bit-identical to the two calls it replaces.
 * Worlds of 17..64 agents run the crowd form's kernel of the same kind (one workgroup of two wavefronts per tile: the env step and the
 * bookkeeping on one, the copy of the step's state rows on the other) and report CAVOID_FORM_CROWD to cavoid_last_step_form
 * (CAVOID_FORM_CROWD_RVO with rvo_enabled = CAVOID_RVO_WAVE: the same launch over the ORCA-carrying env step).
 * CAVOID_EUNSUPPORTED: holonomic dynamics. */
int cavoid_step_push(cavoid_env *env, cavoid_rollout *rollout, const cavoid_rollout_buffers *buffers, const float *obs_cur, float *obs_next,
                     const int32_t *actions, const float *values, float *rewards, uint8_t *done, uint8_t *game_over, int32_t step, void *stream);

/* hand-over to the trainer (`training_q.put((x_, r_, a_))`, ProcessAgent.py:238): append the training rows (emit_t >= 0) of
 * the step blocks [step_lo, step_hi) to one batch -- out_x float [capacity, D], out_r float [capacity] (n-step returns),
 * out_a int32 [capacity], out_src int32 [capacity, 4] (world, agent, recorded-at, emitted-at; may be NULL),
 * out_count int32 [2] = (rows OFFERED: stored plus dropped, rows dropped for lack of capacity), zeroed by the call: the batch holds
 * min(out_count[0], capacity) rows and nothing is written behind `capacity` (0 is allowed).  Row order is unspecified.
 * mark_taken != 0 stamps the STORED rows emit_t = -2 (they are not handed out again; a dropped row stays for a later call).  Rows of every width the env makes are carried
 * (D up to 453 = 5 + 7 * 64); CAVOID_EUNSUPPORTED only from D = 4096 up, where the copy loop's multiply-shift e / D is no longer exact. */
int cavoid_rollout_compact(cavoid_rollout *r, int32_t step_lo, int32_t step_hi, int32_t mark_taken, const float *x, const float *ret,
                           const uint8_t *act, int32_t *emit_t, float *out_x, float *out_r, int32_t *out_a, int32_t *out_src,
                           int32_t *out_count, int64_t capacity, void *stream);

/* the (world, agent) slots that still need a policy output: learning agents that have not finished (an agent that is done
 * waits for its world's last learning agent; the env ignores its action -- ProcessAgent.py:149-211).  obs = the observation
 * the policy is about to act on [W,N,1+D]; done / game_over = the outputs of the step that produced it (after a reset:
 * game_over = 1 everywhere).  row_index int32 [W*N] receives the slot ids in unspecified order, row_count int32 [1] their
 * number; both stay on the device (cavoid_policy_forward_rows reads them there). */
int cavoid_rollout_active_rows(cavoid_rollout *r, const float *obs, const uint8_t *done, const uint8_t *game_over,
                               int32_t *row_index, int32_t *row_count, void *stream);

/* ---- fused policy inference (the actors' predict + select_action) ------------------------------------
 * Stands in for `NetworkVPCore.predict_p_and_v(x)` (ga3c/GA3C/NetworkVPCore.py:175-176) on the graph
 * `NetworkVP_rnn._create_graph` builds for MULTI_AGENT_ARCH 'RNN' (ga3c/GA3C/NetworkVP_rnn.py:50-67,103-105;
 * NetworkVPCore.py:66-75) and, optionally, `ProcessAgent.select_action` (ga3c/GA3C/ProcessAgent.py:89-103),
 * for every agent row of the batched env in ONE kernel on the matrix cores (float32 in, float32 accumulate).
 *   cavoid_policy_load   : hand over the variables in the reference checkpoint's layout (device pointers; dense
 *                          kernels [in,out], LSTM kernel [7+64, 4*64] in gate order i,j,f,o); they are re-packed
 *                          into MFMA fragment order inside the handle.  Call again whenever the trainer has
 *                          updated the weights.  avg/std = NN_INPUT_AVG_VECTOR / NN_INPUT_STD_VECTOR
 *                          (Config.py:64-71), both NULL = NORMALIZE_INPUT off.
 *   cavoid_policy_forward: x = first policy input (num_other_agents) of row 0, `row_stride` floats between
 *                          rows -- pass `obs + 1, 1 + D` to run straight on the env's observation tensor.
 *                          p_out float [rows, num_actions] (softmax_p incl. MIN_POLICY), v_out float [rows].
 *                          actions_out (nullable) int32 [rows]: greedy != 0 -> argmax p (PLAY_MODE /
 *                          EVALUATE_MODE), else one inverse-CDF sample per row from Philox4x32-10 keyed on
 *                          (seed, row, launch counter); the counter lives on the device (hipGraph replays).
 * Observed agents: cavoid_policy_create takes max_other 1..64 (the env's own limit); 65 and up is CAVOID_EINVAL.
 *   max_other <= 19: every kernel below -- the inference forms (CAVOID_POLICY_F32 / _PRODUCTS / _FORM), the trainer pass, the fused actor.
 *   20..64, a CROWD handle: inference on one kernel that streams the observed agents through a ring of input slots; a row of
 *     <= 19 observed agents gets bit for bit what a handle of max_other <= 19 gives it.  Two product forms: the default (float16 pieces) and
 *     CAVOID_POLICY_PRODUCTS=3 (bf16 pieces, float32's range); CAVOID_POLICY_F32=1 or _PRODUCTS=4 / 5 make cavoid_policy_create return
 *     CAVOID_EUNSUPPORTED, CAVOID_POLICY_FORM is ignored.  cavoid_policy_forward / _rows take a row_stride up to 455 floats (1 + 6 + 7 * 64:
 *     the widest env observation row; 256 for max_other <= 19).  cavoid_policy_train / _train_regression run their forward launch on
 *     ring kernels of the same kind (float32 MFMA, whatever the inference form) and the unchanged backward launch behind it: same
 *     buffers and contract, bit for bit a max_other <= 19 handle's results on rows of <= 19 observed agents.  cavoid_actor_run /
 *     _run_mix return CAVOID_EUNSUPPORTED: the actor kernel parks the whole input row and stops at 19. */
typedef struct cavoid_policy_weights {
    int32_t struct_size;             /* sizeof(cavoid_policy_weights) */
    float min_policy;                /* Config.MIN_POLICY */
    float forget_bias;               /* tf.contrib.rnn.LSTMCell default: 1.0 */
    int32_t with_backward;           /* != 0: also pack the transposed copies cavoid_policy_train_* needs */
    const float *avg, *std;          /* [5 + 7*max_other] or both NULL */
    const float *lstm_kernel, *lstm_bias;       /* rnn/lstm_cell/kernel [71,256], bias [256] */
    const float *layer1_kernel, *layer1_bias;   /* layer1 [68,256], [256] */
    const float *layer2_kernel, *layer2_bias;   /* layer2 [256,256], [256] */
    const float *fc1_kernel, *fc1_bias;         /* fullyconnected1 [256,256], [256] */
    const float *p_kernel, *p_bias;             /* logits_p [256,A], [A] */
    const float *v_kernel, *v_bias;             /* logits_v [256,1], [1] */
} cavoid_policy_weights;
int cavoid_policy_create(int32_t max_other, int32_t num_actions, int device, cavoid_policy **out);
void cavoid_policy_destroy(cavoid_policy *p);
int cavoid_policy_load(cavoid_policy *p, const cavoid_policy_weights *w, void *stream);
int cavoid_policy_seed(cavoid_policy *p, uint64_t seed, void *stream);
/* what the handle is (fixed at cavoid_policy_create: the environment switches CAVOID_POLICY_F32 / CAVOID_POLICY_PRODUCTS are read there,
 * never again): use_split = 1 when inference runs on the operand-split kernel (0: the float32-MFMA kernel); split_products = 16 for the
 * default float16 two-piece form, 3 / 4 / 5 for bf16 pieces.  RANGE LIMIT of the default form: a float16 piece saturates at +-65504, so a
 * weight beyond that (after the LSTM gate columns' scale of log2 e / 2 log2 e) is CLAMPED at load and the network then differs from the
 * reference's float32 predictor; clamped_weights = how many weights of the last cavoid_policy_load were (0 for every sane checkpoint;
 * reading it synchronises `stream`).  A caller that finds it non-zero should re-create the handle with CAVOID_POLICY_PRODUCTS=3 (bf16
 * pieces: float32's range) or, for max_other <= 19 only, CAVOID_POLICY_F32=1.  Inputs and hidden activations beyond +-65504 saturate in the kernel the same way.
 * Any out pointer may be NULL. */
int cavoid_policy_info(cavoid_policy *p, void *stream, int32_t *use_split, int32_t *split_products, int32_t *clamped_weights);
int cavoid_policy_forward(cavoid_policy *p, const float *x, int64_t rows, int64_t row_stride, float *p_out, float *v_out,
                          int32_t *actions_out, int32_t greedy, void *stream);
/* as cavoid_policy_forward, for the rows row_index[0 .. *row_count) only (device-side list and count: the launch geometry
 * does not depend on them, so the call can sit in a hipGraph); outputs of the other rows are left untouched */
int cavoid_policy_forward_rows(cavoid_policy *p, const float *x, int64_t rows, int64_t row_stride, const int32_t *row_index,
                               const int32_t *row_count, float *p_out, float *v_out, int32_t *actions_out, int32_t greedy,
                               void *stream);

/* ---- fused trainer pass (Server.train_model -> NetworkVPCore.train, ga3c/GA3C/Server.py:114-124, NetworkVPCore.py:71-100,178-187)
 * Forward + loss + the row-local part of the backward pass of the same network, for a batch of training rows
 * (x [rows, row_stride], y_r [rows] n-step returns, a_idx int32 [rows] actions taken), in two launches on the matrix
 * cores.  Needs cavoid_policy_load(with_backward = 1).  It leaves, in caller-owned buffers, the operand pair of every
 * weight-gradient GEMM (the layer's input rows and the gradient at its output rows).  A caller either finishes the step inside the
 * library -- cavoid_policy_weight_grads + cavoid_policy_apply, section 'the rest of the trainer step' below -- or forms X^T G with its
 * own GEMM library, sums the bias gradients and takes the optimiser step itself:
 *   d fullyconnected1 = z2^T g3,  d layer2 = z1^T g2,  d layer1 (rows in packed order: 64 hidden, 4 host) = l1_in^T g1,
 *   d [logits_p | logits_v] = z3^T gh,  d lstm (rows: 64 hidden then 7 inputs; gate columns in packed order
 *   64w + 16 gate + u for unit 16w + u) = sum_t h_in[t]^T gl[t];   bias gradients (column sums of g3, g2, g1, gh, gl) come back in `db`.
 * All per-row buffers have `capacity_rows` rows (a multiple of 64, >= rows rounded up to 64); every one of them is
 * written by each call, rows past `rows` with zero gradients -- the GEMMs may run over all capacity_rows.  loss[0] = cost_p, loss[1] = cost_v (sums over rows, NetworkVPCore.py:71-100).
 * max_other 1..64: a crowd handle (20..64) takes the same call and buffers.  Mind their size there: 6 496 + 3 360 max_other bytes per
 * buffer row, 218 KB at max_other = 63. */
typedef struct cavoid_policy_train_buffers {
    int32_t struct_size;             /* sizeof(cavoid_policy_train_buffers) */
    int32_t reserved;
    int64_t capacity_rows;
    float *z1, *z2, *z3;             /* [capacity_rows, 256] */
    float *l1_in;                    /* [capacity_rows, 72] */
    float *h_in;                     /* [max_other, capacity_rows, 72] */
    float *save;                     /* [capacity_rows / 64, max_other, 16, 256, 8] */
    float *gh;                       /* [capacity_rows, 16] */
    float *loss;                     /* [2] */
    float *g1, *g2, *g3;             /* [capacity_rows, 256] */
    float *gl;                       /* [max_other, capacity_rows, 256] */
    float *db;                       /* [1040] bias gradients: lstm 256 (packed gate order), layer1, layer2, fullyconnected1 256 each,
                                        heads 16 (A logits, value, padding) */
} cavoid_policy_train_buffers;
int cavoid_policy_train(cavoid_policy *p, const float *x, int64_t rows, int64_t row_stride, const float *y_r, const int32_t *a_idx,
                        float beta, float log_epsilon, const cavoid_policy_train_buffers *buffers, void *stream);

/* ---- the weight-sharing network (MULTI_AGENT_ARCH 'weight_sharing', ga3c/GA3C/NetworkVP_rnn.py:69-92) ----------------------
 * Every observed-agent slot i < max_other goes through ONE shared dense filter, also past the row's own count:
 *   f_i = relu([xn_i (7) | is_on_i] . other_kernel[8, 64] + other_bias[64]),  is_on_i = (x[:,0] >= i + 1) on the RAW count,
 *   layer1 = relu([host(4) | f_0 .. f_{max_other-1}] . layer1_kernel[4 + 64 max_other, 256] + layer1_bias), then layer2,
 *   fullyconnected1 and the heads as for the LSTM network.  Float32 MFMA (no split form; the products are exact float32).
 *   cavoid_policy_create_ws: max_other 1..19 (the kernel parks the whole input row); 20..64 is CAVOID_EUNSUPPORTED (_create_ws_crowd
 *       takes those), outside 1..64
 *       CAVOID_EINVAL (the range is checked before the device).
 *   cavoid_policy_create_ws_crowd: max_other 20..64, the handle for the rows the crowd step form's worlds observe.  1..19 is
 *       CAVOID_EUNSUPPORTED (use cavoid_policy_create_ws), outside 1..64 CAVOID_EINVAL (the range is checked before the device).  Every
 *       call below takes such a handle as it takes a cavoid_policy_create_ws one -- same arguments, buffers, contract and error codes;
 *       cavoid_policy_forward / _rows then take a row_stride up to 455 floats, and the forward launches (inference, _train_ws,
 *       _train_regression_ws) run on kernels that park 19 slots of the row at a time and stream the rest through them as a ring; the
 *       backward launch is the same kernel.  On rows whose slots past 19 carry zero layer1 weights they give bit for bit what a
 *       max_other = 19 handle gives.  Mind the trainer buffers' size: 6 224 + 544 max_other bytes per buffer row.
 *   cavoid_policy_load_ws  : w as for cavoid_policy_load, except that w->layer1_kernel is [4 + 64 max_other, 256] (rows: host, then
 *       slot-major) and the lstm fields and forget_bias are ignored; other_kernel [8, 64], other_bias [64].
 *   cavoid_policy_forward / _forward_rows / _seed / _info / _destroy take either kind of handle (same arguments, same action draw;
 *       _info reports use_split = 0, split_products = 0).  cavoid_policy_load / _train on a weight-sharing handle, and _load_ws /
 *       _train_ws on an LSTM handle, are CAVOID_EINVAL; cavoid_actor_run / _run_mix with one (as policy or frozen) are
 *       CAVOID_EUNSUPPORTED (cavoid_actor_run_ws is this network's closed actor loop, cavoid_crowd_actor_run_ws the one of crowd worlds).  CAVOID_POLICY_F32 / _PRODUCTS / _FORM do not apply.
 *   cavoid_policy_train_ws : the trainer pass of cavoid_policy_train for this network (load with with_backward = 1).  The contractions it
 *       leaves the operands of (cavoid_policy_weight_grads_ws forms them, or the caller's own GEMM library):
 *       d fullyconnected1 = z2^T g3,  d layer2 = z1^T g2,  d [logits_p | logits_v] = z3^T gh,
 *       d layer1 = l1_in^T g1 (rows in the checkpoint's order),  d other_kernel = f_in^T gf over all max_other * capacity_rows rows;
 *       bias gradients in db: other_bias at 0..63, then layer1 / layer2 / fullyconnected1 / heads at 256 / 512 / 768 / 1024. */
typedef struct cavoid_policy_train_ws_buffers {
    int32_t struct_size;             /* sizeof(cavoid_policy_train_ws_buffers) */
    int32_t reserved;
    int64_t capacity_rows;           /* a multiple of 64, >= rows rounded up to 64; every row is written (past `rows`: zero gradients) */
    float *z1, *z2, *z3;             /* [capacity_rows, 256] */
    float *l1_in;                    /* [capacity_rows, 4 + 64 max_other]: [host | f_0 .. f_{max_other-1}] */
    float *f_in;                     /* [max_other, capacity_rows, 8]: [xn_i | is_on_i] */
    float *gh;                       /* [capacity_rows, 16] */
    float *loss;                     /* [2] cost_p, cost_v */
    float *g1, *g2, *g3;             /* [capacity_rows, 256] */
    float *gf;                       /* [max_other, capacity_rows, 64]: d cost / d f_i, masked by the filter's relu */
    float *db;                       /* [1040] */
} cavoid_policy_train_ws_buffers;
int cavoid_policy_create_ws(int32_t max_other, int32_t num_actions, int device, cavoid_policy **out);
int cavoid_policy_create_ws_crowd(int32_t max_other, int32_t num_actions, int device, cavoid_policy **out);
int cavoid_policy_load_ws(cavoid_policy *p, const cavoid_policy_weights *w, const float *other_kernel, const float *other_bias, void *stream);
int cavoid_policy_train_ws(cavoid_policy *p, const float *x, int64_t rows, int64_t row_stride, const float *y_r, const int32_t *a_idx,
                           float beta, float log_epsilon, const cavoid_policy_train_ws_buffers *buffers, void *stream);

/* ---- the supervised start's trainer pass (train_regression_op on cost_regression, ga3c/GA3C/NetworkVPCore.py:90-100,123; the
 * phase Regression.py runs for TRAIN_ONLY_REGRESSION and LOAD_REGRESSION_THEN_TRAIN_RL) ------------------------------------------
 * cavoid_policy_train / cavoid_policy_train_ws with the other loss head, everything else the same: the same two launches, buffer
 * structs, preconditions (with_backward = 1, max_other <= 64 / for _ws <= 19, or <= 64 on a cavoid_policy_create_ws_crowd handle; capacity_rows), caller's GEMMs, db layout and error codes -- the LSTM
 * call on a weight-sharing handle and the _ws call on an LSTM handle are CAVOID_EINVAL.  Per row, with z the A policy logits, v the
 * value logit, a_idx the TEACHER's action and y_r the value target:
 *   cost_p_regression = log sum_k exp(z_k) - z_a   (softmax cross-entropy on the logits, evaluated as log-sum-exp: finite and exact
 *                                                   where float32 softmax entries are 0),   cost_v = 0.5 (y_r - v)^2,
 *   gh[:, k] = softmax(z)_k - [k == a] for k < A,  gh[:, A] = v - y_r,  0 in the padding columns and in rows past `rows`.
 * MIN_POLICY, beta and LOG_EPSILON play no part (the reference takes logits_p, not softmax_p).  loss[0] = cost_p_regression,
 * loss[1] = cost_v, sums over rows.  Precondition, as for cavoid_policy_train / _train_ws: 0 <= a_idx[i] < num_actions for every
 * row; the kernels do not check it (an index outside the range selects another head column of the row). */
int cavoid_policy_train_regression(cavoid_policy *p, const float *x, int64_t rows, int64_t row_stride, const float *y_r,
                                   const int32_t *a_idx, const cavoid_policy_train_buffers *buffers, void *stream);
int cavoid_policy_train_regression_ws(cavoid_policy *p, const float *x, int64_t rows, int64_t row_stride, const float *y_r,
                                      const int32_t *a_idx, const cavoid_policy_train_ws_buffers *buffers, void *stream);

/* ---- the rest of the trainer step (Server.train_model's tail: the weight gradients, NetworkVPCore.py:104-122's optimiser with
 * USE_GRAD_CLIP, and the weight hand-over to the predictors) for the LSTM network, so that a caller without a GEMM library or an
 * optimiser of its own trains through this header alone:
 *     cavoid_policy_train (or _train_regression)  ->  cavoid_policy_weight_grads  ->  [the caller's all-reduce of grads_flat]  ->  cavoid_policy_apply
 *
 * ONE flat parameter vector.  cavoid_policy_param_layout (host code only: no handle, no device) defines it: the CAVOID_POLICY_PARAMS = 12
 *   variables in the order of cavoid_policy_weights' pointers -- lstm_kernel, lstm_bias, layer1_kernel, layer1_bias, layer2_kernel,
 *   layer2_bias, fc1_kernel, fc1_bias, p_kernel, p_bias, v_kernel, v_bias -- each in the checkpoint's shape (row-major), each starting
 *   on a multiple of 64 floats: variable i occupies [offsets[i], offsets[i] + sizes[i]), *total = the end of the last one.  The
 *   floats between two variables are padding: the calls below write zeros there (gradients) or leave them alone (optimiser state).
 *   Gradients, both optimiser state vectors and a multi-GPU all-reduce use this layout.  max_other 1..64, num_actions 1..15, else CAVOID_EINVAL.
 *
 * cavoid_policy_weight_grads: every weight and bias gradient of the pass that just filled `buffers`, into grads_flat [total] in that layout --
 *   the five contractions listed above on the float32 matrix instructions (exact float32 products, float32 accumulation) with the
 *   un-permutations in the epilogue (packed gate columns and the "64 hidden, inputs, pad" row order of the LSTM and layer1 back to the
 *   checkpoint's [7 + 64] / [4 + 64], the [256, 16] head block split into logits_p [256, A] and logits_v [256, 1], db into the six biases).
 *   Two launches, whatever max_other and the row count: the rows are cut into slices of 1 024 (the LSTM's max_other * capacity_rows rows:
 *   of 1 024, or 4 096 once there are more than 4 194 304 of them), one wavefront forms one 64 x 64 (or edge) tile of one slice's partial
 *   product in `scratch`, and a second launch sums the partials of every entry in slice order and writes it where it belongs.  The
 *   partition depends on capacity_rows and max_other only and there are no floating-point atomics: two calls on the same buffers give
 *   the same bits.  The longest accumulation chain is the slice length plus the number of slices.
 *   scratch: device memory of at least the floats cavoid_policy_weight_grads_scratch reports for this handle and capacity_rows, 16-byte
 *   aligned like every per-row buffer (CAVOID_EINVAL otherwise, as for a NULL pointer, a wrong struct_size or a capacity_rows that is
 *   not a positive multiple of 64).  ALL capacity_rows rows are read: call it after a pass that wrote them (a pass over rows = 0 rows
 *   launches nothing and writes none).  Both LSTM handle kinds (max_other 1..19 and crowd handles, 20..64); CAVOID_EUNSUPPORTED on a
 *   weight-sharing handle (cavoid_policy_weight_grads_ws below).
 *
 * cavoid_policy_apply: one optimiser step on the float32 MASTER weights and the re-pack.  `weights`: the struct of cavoid_policy_load whose
 *   twelve variable pointers are the masters (device memory the caller owns; updated IN PLACE although the struct says const), with
 *   min_policy / forget_bias / with_backward / avg / std as the caller would load them.  opt->kind:
 *     CAVOID_OPT_ADAM     m = b1 m + (1 - b1) g,  v = b2 v + (1 - b2) g^2,  w -= lr / (1 - b1^t) * m / (sqrt(v) / sqrt(1 - b2^t) + eps)
 *                         (decay1 = b1, decay2 = b2, state1 = m, state2 = v, t = *step + 1: torch.optim.Adam without amsgrad / weight decay)
 *     CAVOID_OPT_RMSPROP  ms = rho ms + (1 - rho) g^2,  mom = mu mom + lr g / sqrt(ms + eps),  w -= mom
 *                         (decay1 = rho, decay2 = mu, state1 = ms, state2 = mom: tf.train.RMSPropOptimizer, not centred, eps INSIDE the
 *                         root; the caller initialises ms to ones as TensorFlow does)
 *   clip_average_norm = c > 0 (tf.clip_by_average_norm, GRAD_CLIP_NORM): per variable g <- g * c / max(||g||_2 / n, c), n its element
 *   count, applied to what the update reads; grads_flat itself is not modified.  c = 0: off.  lr is passed by value (the reference
 *   anneals it per step); the coefficients are formed in double and rounded to float32 once, the element arithmetic is float32.
 *   state1 / state2: device float [total]; step: device int64, read as t - 1 and written back as t by one thread.  Launches: one for the
 *   update, one more in front of it for the twelve norms when clipping (a fixed-order reduction per variable); then exactly
 *   cavoid_policy_load on the updated masters on the same stream -- the handle afterwards is, bit for bit, what a fresh load gives.
 *   CAVOID_EINVAL: NULL pointers, wrong struct sizes, an unknown kind, a negative clip; CAVOID_EUNSUPPORTED: a weight-sharing handle (cavoid_policy_apply_ws below). */
#define CAVOID_POLICY_PARAMS 12
enum { CAVOID_OPT_ADAM = 0, CAVOID_OPT_RMSPROP = 1 };
typedef struct cavoid_policy_optimizer {
    int32_t struct_size;             /* sizeof(cavoid_policy_optimizer) */
    int32_t kind;                    /* CAVOID_OPT_* */
    double lr;
    double decay1, decay2;           /* Adam: beta1, beta2; RMSProp: decay rho, momentum mu */
    double eps;
    double clip_average_norm;        /* 0 = off */
    float *state1, *state2;          /* [total] each */
    int64_t *step;                   /* [1] optimiser steps taken so far */
} cavoid_policy_optimizer;
int cavoid_policy_param_layout(int32_t max_other, int32_t num_actions, int64_t *offsets, int64_t *sizes, int64_t *total);
int cavoid_policy_weight_grads_scratch(const cavoid_policy *p, int64_t capacity_rows, int64_t *floats);
int cavoid_policy_weight_grads(cavoid_policy *p, const cavoid_policy_train_buffers *buffers, float *scratch, int64_t scratch_floats,
                               float *grads_flat, void *stream);
int cavoid_policy_apply(cavoid_policy *p, const cavoid_policy_weights *weights, const cavoid_policy_optimizer *opt, const float *grads_flat,
                        void *stream);

/* ---- the rest of the trainer step for the WEIGHT-SHARING network: the same sequence on a cavoid_policy_create_ws / _create_ws_crowd handle
 *     cavoid_policy_train_ws (or _train_regression_ws)  ->  cavoid_policy_weight_grads_ws  ->  [the caller's all-reduce of grads_flat]  ->  cavoid_policy_apply_ws
 * with cavoid_policy_optimizer and cavoid_policy_train_ws_buffers as they are.  The three LSTM calls above stay CAVOID_EUNSUPPORTED on such
 * a handle, and these are CAVOID_EUNSUPPORTED on an LSTM handle.
 *
 * cavoid_policy_param_layout_ws (host code only): the flat vector of this network -- CAVOID_POLICY_PARAMS = 12 variables in the order
 *   other_kernel [8, 64], other_bias [64], layer1_kernel [4 + 64 max_other, 256], layer1_bias, layer2_kernel, layer2_bias, fc1_kernel,
 *   fc1_bias, p_kernel [256, A], p_bias, v_kernel, v_bias -- each in the checkpoint's shape, each starting on a multiple of 64 floats, the
 *   padding as above.  Unlike the LSTM layout it depends on max_other.  max_other 1..64, num_actions 1..15, no NULL, else CAVOID_EINVAL.
 *
 * cavoid_policy_weight_grads_ws: every weight and bias gradient of the pass that just filled `buffers`, into grads_flat [total]: the five
 *   contractions of cavoid_policy_train_ws's comment on the float32 matrix instructions (exact float32 products, float32 accumulation).
 *   Nothing is permuted -- l1_in's columns and f_in's [xn | is_on] are in the checkpoint's order: layer1 is max_other 64-row blocks plus a
 *   4-row host edge, other_kernel an 8-row edge over the flat max_other * capacity_rows rows; absent columns of an edge tile are zeros that
 *   are never loaded.  db is moved into the six biases.  Two launches, whatever max_other and the row count.  The row slices, by
 *   capacity_rows (R) and max_other (M) only:
 *     fullyconnected1, layer2, heads   1 024 rows;                                     D = ceil(R / 1 024) slices
 *     layer1                           1 024 rows;                                     L = D
 *     other_kernel                     1 024 flat rows, 4 096 once M R > 4 194 304;    F = ceil(M R / that)
 *   (a layer1 partial is 4 MB at M = 63, so 16 384 rows there take 66 MB of partials, a tenth of the pass's own buffers: longer slices
 *   measured slower by the time of one long tile).  One wavefront forms one
 *   64 x 64 (or edge) tile of one slice's partial in `scratch`, the second launch sums every entry's partials in slice order: no
 *   floating-point atomics, the same bits for the same buffers; the longest accumulation chain is the slice length plus the number of
 *   slices.  Every float of grads_flat is written (zeros in the padding); ALL capacity_rows rows are read.
 *   scratch: at least the floats cavoid_policy_weight_grads_scratch_ws reports,
 *       L * (4 + 64 M) * 256  +  D * 135 168  +  F * 512,
 *   16-byte aligned like every per-row buffer.  CAVOID_EINVAL: a NULL or misaligned pointer, a wrong struct_size, a capacity_rows that is
 *   not a positive multiple of 64, too small a scratch.
 *
 * cavoid_policy_apply_ws: cavoid_policy_apply's launches (the same kernels, the same optimiser rules and clip) over this layout.  The
 *   twelve masters are other_kernel, other_bias and the ten non-LSTM pointers of `weights` (its lstm fields are ignored, as in
 *   cavoid_policy_load_ws); then exactly cavoid_policy_load_ws on the updated masters on the same stream -- the handle afterwards is, bit
 *   for bit, what a fresh load gives.  Error codes as for cavoid_policy_apply; a refused call does not step. */
int cavoid_policy_param_layout_ws(int32_t max_other, int32_t num_actions, int64_t *offsets, int64_t *sizes, int64_t *total);
int cavoid_policy_weight_grads_scratch_ws(const cavoid_policy *p, int64_t capacity_rows, int64_t *floats);
int cavoid_policy_weight_grads_ws(cavoid_policy *p, const cavoid_policy_train_ws_buffers *buffers, float *scratch, int64_t scratch_floats,
                                  float *grads_flat, void *stream);
int cavoid_policy_apply_ws(cavoid_policy *p, const cavoid_policy_weights *weights, const float *other_kernel, const float *other_bias,
                           const cavoid_policy_optimizer *opt, const float *grads_flat, void *stream);

/* kernel timing helper: HIP events recorded on `stream` around the launches of the calls made
 * between begin and end; end synchronises and returns elapsed milliseconds */
int cavoid_timer_begin(cavoid_env *env, void *stream);
int cavoid_timer_end(cavoid_env *env, void *stream, float *elapsed_ms);

#ifdef __cplusplus
}
#endif
#endif /* CAVOID_H */
