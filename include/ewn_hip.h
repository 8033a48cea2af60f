/*
 * include/ewn_hip.h -- C ABI of libewn_hip.so: the MI355X (gfx950) vectorised
 * EinStein-wuerfelt-nicht environment step and opponent-search engine.
 *
 * The reference (jchen8tw/ewn-gym) is pure Python and has no FFI: its boundary
 * for this path is the Python class surface of envs/ewn.py, envs/minimax_ewn.py,
 * envs/training_ewn.py and classical_policies/{random_policy,minimax,mcts}.py.
 * Each entry point below names the reference method(s) it replaces, batched over
 * N independent games ("lanes").  The Python mirror of those classes (packages
 * envs/, classical_policies/, constants/ at the repo root) binds this ABI with
 * ctypes; INTEGRATION.md shows the stub a reference maintainer would add.
 *
 * Conventions
 *  - Plain C: pointers + sizes only.  Every buffer pointer is a DEVICE pointer
 *    owned by the caller (e.g. torch.Tensor.data_ptr()); nothing is allocated,
 *    freed or synchronised inside a call, so calls are hipGraph-capturable.
 *  - `stream` is a hipStream_t passed as void* (NULL = the null stream).
 *  - Return value: 0 on success, a negative EWN_E* code otherwise (never throws,
 *    never aborts).  ewn_strerror() maps a code to text.
 *  - No hidden global state beyond six tuning overrides read from the
 *    environment, each selecting only a launch shape or a kernel instance.  Five
 *    are latched -- read once per process, by the first call that needs them:
 *    EWN_D3_T, EWN_ROLLOUT_T, EWN_ROLLOUT_SLOTS, EWN_MCTS_GPB and EWN_EVAL_NT.
 *    The sixth, EWN_PUCT_TILE, is read at every call (see ewn_puct_search).  A
 *    call is thread-safe w.r.t. other calls that do not share buffers.
 *  - Boards are int8, row-major [lane][row][col], value k>0 = TOP_LEFT cube k,
 *    k<0 = BOTTOM_RIGHT cube |k|, 0 = empty (envs/ewn.py:49-58, 94-107).
 *  - Actions are int8 [lane][2] = {chose_larger in {0,1}, direction in {0,1,2}}
 *    (envs/ewn.py:61-62, 436-442); action buffers are 2-byte aligned, board / rng
 *    / table buffers 16-byte aligned (any torch allocation is).
 */
#ifndef EWN_HIP_H
#define EWN_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define EWN_ABI_VERSION 4 /* 2: ewn_step_k, ewn_predict_minimax_sim, ewn_lanes_per_game; six table images; boards up to 11x11.  3: EWN_AGENT_SAMPLE; 32 KB table images.
                             4: ewn_rollout_out.record, ewn_roll_dice, EWN_AGENT_MLP / ewn_policy, shaped env and MCTS opponent in ewn_step_k, ewn_a2c_*;
                                later ewn_ppo_hyper / ewn_ppo_* (purely additive: the version stays 4) */

/* error codes */
#define EWN_OK 0
#define EWN_EINVAL (-1)      /* bad argument / unsupported configuration (the reference asserts, envs/ewn.py:47) */
#define EWN_ENULL (-2)       /* required pointer is NULL */
#define EWN_ELAUNCH (-3)     /* kernel launch failed (hipGetLastError != hipSuccess) */
#define EWN_EUNSUPPORTED (-4)/* valid in the reference, not built here (e.g. board_size > 11, max_depth > 6) */

/* opponent_kind: constants/policy.py:4-10 (uct / alpha_zero are out of scope) */
#define EWN_OPP_RANDOM 0
#define EWN_OPP_MINIMAX 1
#define EWN_OPP_MCTS 2

/* rng_kind */
#define EWN_RNG_MT19937 0 /* bit-exact numpy legacy global stream, one per lane (envs/ewn.py:91,490) */
#define EWN_RNG_PHILOX 1  /* Philox4x32-10 counter RNG, same masked-rejection randint */

/* heuristic: envs/minimax_ewn.py:29-38 */
#define EWN_H_HYBRID 0
#define EWN_H_MIN_DIST 1
#define EWN_H_TWO_MIN_DIST 2
#define EWN_H_ATTK 3
#define EWN_H_SIM_WINRATE 4 /* MinimaxEnv.simulate as the search leaf (envs/minimax_ewn.py:36-37, 215-238): 100 random playouts per
                               leaf; searches only (ewn_evaluate answers it through ewn_playout_wins); max_depth 5 / 6 run for seconds */
#define EWN_SIM_WINRATE_PLAYOUTS 100 /* MinimaxEnv.num_simulations, envs/minimax_ewn.py:20 */
#define EWN_SIM_WINRATE_MAX_DEPTH 6

/* info codes of ewn_step: the messages of envs/ewn.py:448,454,473,478 and envs/training_ewn.py:56 */
#define EWN_INFO_NONE 0
#define EWN_INFO_INVALID_PLAYER 1 /* "Invalid move for player! End the game." */
#define EWN_INFO_WON 2            /* "You won!" */
#define EWN_INFO_INVALID_OPP 3    /* "Invalid move for opponent! End the game." */
#define EWN_INFO_LOST 4           /* "You lost!" */
#define EWN_INFO_TOLERANCE 5      /* "Invalid move for player! Tolerance left {n}." */

#define EWN_MAX_BOARD 11  /* up to 8x8: 64-bit occupancy masks and the table-driven kernels; 9x9 .. 11x11: the generic kernels on a
                             mask-free state (7-bit positions) */
#define EWN_MAX_CUBES 15  /* cube_layer <= 5 */
#define EWN_MAX_DEPTH 6
#define EWN_MT_WINDOW_MAX 227 /* MT19937 outputs computable from the seeded state alone */
#define EWN_RNG_HEADER_WORDS 4

/* Replaces the constructor arguments of EinsteinWuerfeltNichtEnv (envs/ewn.py:35-42),
 * MiniMaxHeuristicEnv (envs/training_ewn.py:19-29) and the opponent policy ctor
 * kwargs (classical_policies/minimax.py:10-11, mcts.py:11-13). */
typedef struct ewn_config {
    int32_t board_size;             /* S, 3..EWN_MAX_BOARD */
    int32_t cube_layer;             /* L, cube_num = L(L+1)/2, L < S-1 */
    int32_t n_lanes;                /* N parallel games handled by this call */
    int32_t opponent_kind;          /* EWN_OPP_* */
    int32_t max_depth;              /* ExpectiMinimaxAgent.max_depth, 1..EWN_MAX_DEPTH */
    int32_t heuristic;              /* EWN_H_* */
    int32_t num_simulations;        /* MctsAgent.num_simulations */
    int32_t num_env_copies;         /* MctsAgent.num_env_copies */
    int32_t rng_kind;               /* EWN_RNG_* */
    int32_t shaped;                 /* 0: EinsteinWuerfeltNichtEnv.step, 1: MiniMaxHeuristicEnv.step */
    int32_t illegal_move_tolerance; /* initial tolerance (training_ewn.py:38); used by ewn_init_aux */
    int32_t autoreset;              /* 1: a terminated lane is reset (next seed) inside ewn_step */
    int32_t shaped_refresh_on_reset;/* 0 = reference behaviour: prev_score is set in the ctor only */
    int32_t lane_offset;            /* global id of lane 0 (multi-GPU sharding); enters the Philox agent/MCTS streams */
    uint32_t seed_stride;           /* auto-reset: seed += seed_stride per episode */
    uint32_t mt_window;             /* MT19937 outputs precomputed per episode, 16..EWN_MT_WINDOW_MAX (0 = 128) */
    double reward;                  /* envs/ewn.py:38 (goal_reward of the shaped env) */
    double illegal_move_reward;     /* training_ewn.py:28 */
    uint64_t philox_key;
} ewn_config;

/* Per-lane state, structure-of-arrays, all device pointers, caller-owned. */
typedef struct ewn_state {
    int8_t *board;       /* [N][S*S]  the observation "board" (agent = TOP_LEFT to move) */
    int8_t *dice;        /* [N]       the observation "dice_roll" */
    uint8_t *done;       /* [N]       1 = terminated and not yet reset (lane frozen) */
    uint32_t *rng;       /* N*ewn_rng_words() words: [N][4] headers {seed, draw index, next_seed, flags}, then (MT kind)
                            [N][3][W] windows of precomputed MT19937 outputs (this episode's and the next two) and
                            [N] reset epochs.  Opaque to the caller; zero-initialise, then ewn_init_aux. */
    double *prev_score;  /* [N]  shaped env only (training_ewn.py:35), may be NULL otherwise */
    int32_t *tolerance;  /* [N]  shaped env only (training_ewn.py:38), may be NULL otherwise */
    const void *tables;  /* device copy of ewn_build_tables() output, or NULL.  When present and the config is
                            (cube_layer 3, boards 5..8, plain or shaped; RandomAgent opponent, or minimax with max_depth
                            1..6 and 'hybrid', 'min_dist', 'attk' or 'two_min_dist') ewn_step runs the specialised
                            table-driven kernel; results are identical either way. */
} ewn_state;

/* Outputs of one step, device pointers, caller-owned.  The post-step observation is
 * written in place to ewn_state.board / .dice. */
typedef struct ewn_step_out {
    double *reward;        /* [N] */
    uint8_t *terminated;   /* [N] */
    uint8_t *truncated;    /* [N] */
    uint8_t *info;         /* [N] EWN_INFO_* */
    int8_t *terminal_board;/* [N][S*S] observation before auto-reset (SB3 "terminal_observation"); NULL to skip */
    int8_t *terminal_dice; /* [N] ; NULL to skip */
    int8_t *random_action; /* [N][2] ; NULL to skip.  RandomAgent.predict (classical_policies/random_policy.py:11-15) on the
                              POST-step observation, fused into the step: a uniformly random legal action of the agent,
                              drawn from a hash of (episode seed, draws so far, global lane id, philox_key).  May alias
                              `actions` (each lane reads its action before it writes the next one). */
} ewn_step_out;

int ewn_abi_version(void);
const char *ewn_strerror(int code);

/* number of uint32 words per lane in ewn_state.rng for this config (<0 on error) */
int ewn_rng_words(const ewn_config *cfg);
/* bytes of device scratch ewn_step needs for this config (0 if none; <0 on error): the MCTS split-phase buffers, or
 * (MT kind with auto-reset) the queue through which one step launch hands window refills to the next.  The scratch
 * must be zero-initialised once and then left alone between calls. */
int64_t ewn_step_scratch_bytes(const ewn_config *cfg);

/* Search and move-selection tables of the specialised kernel (leaf-value ranks, ring-order geometry, dice -> cube
 * selectors; two images: max_depth 1-3 and 5, and max_depth 4 and 6, whose leaves are six-dice averages of evaluate();
 * ewn_gym_amd/csrc/ewn_fast.hpp).  Pure host computation: ewn_tables_bytes() gives the size
 * (0 = no specialised kernel for this geometry), ewn_build_tables() fills a HOST buffer the
 * caller then copies to the device and passes as ewn_state.tables / the `tables` argument. */
int64_t ewn_tables_bytes(int board_size, int cube_layer);
int ewn_build_tables(int board_size, int cube_layer, void *host_out);
/* Byte offset, inside ONE image of ewn_build_tables()'s output, of the 16-bit leaf-rank entry of the pair (ix, iy), 0 <= ix, iy < 64
 * (a side's index: level * 8 + count): the address every search kernel reads it at.  The layout of the rank table is otherwise
 * private to ewn_fast.hpp; this query lets a test or a tool read an image without knowing it.  < 0: no tables for this board
 * size, or an index out of range. */
int ewn_tables_rank_offset(int board_size, int ix, int iy);

/* Constructor-time state that reset() does not touch in the reference:
 * prev_score = evaluate(initial board) (training_ewn.py:35) and the tolerance
 * counter (:38); also clears `done` and zeroes the rng header. */
int ewn_init_aux(const ewn_config *cfg, const ewn_state *st, void *stream);

/* EinsteinWuerfeltNichtEnv.reset(seed) (envs/ewn.py:488-494) + setup_game (:94-108)
 * for every lane with lane_mask[i] != 0 (NULL = all lanes).  seeds[i] (NULL = the
 * lane's stored next_seed) is the argument of np.random.seed. */
int ewn_reset(const ewn_config *cfg, const ewn_state *st, const uint32_t *seeds, const uint8_t *lane_mask, void *stream);

/* EinsteinWuerfeltNichtEnv.roll_dice (envs/ewn.py:90-92): dice_roll = np.random.randint(1, cube_num + 1), one draw from the
 * lane's own dice stream, for every lane with lane_mask[i] != 0 (NULL = all lanes) whose game is not finished.  The step
 * and reset entry points roll their dice themselves; this is the public method on its own. */
int ewn_roll_dice(const ewn_config *cfg, const ewn_state *st, const uint8_t *lane_mask, void *stream);

/* EinsteinWuerfeltNichtEnv.step (envs/ewn.py:436-486) or, with cfg->shaped,
 * MiniMaxHeuristicEnv.step (envs/training_ewn.py:43-99): agent move, win test,
 * opponent dice + reply (opponent_action, ewn.py:289-296, by cfg->opponent_kind),
 * win test, next dice; optional auto-reset.  `scratch` = ewn_step_scratch_bytes() bytes. */
int ewn_step(const ewn_config *cfg, const ewn_state *st, const int8_t *actions, const ewn_step_out *out,
             void *scratch, void *stream);

/* ---- K env steps per launch, the agent played by the engine too --------------------------------------------------
 * Replaces the evaluation loop of eval_minimax.py:16-50 / eval_pairs.py:10-35
 *     while not done: action, _ = agent.predict(obs); obs, reward, done, trunc, info = env.step(action)
 * (and a rollout collector's inner loop) when `agent` is one of the classical policies: the state is read once, stays in
 * registers for K steps and is written once; results are identical, step for step, to K ewn_step calls with the agent's
 * action fed back.  Always un-shaped, and MT19937-compat dice only without auto-reset.  Served for (ewn_step_k_supported() says which):
 * the table-driven configurations (cube_layer 3, board sizes 5..8, ewn_state.tables set; opponent RandomAgent or minimax with
 * 'hybrid', 'min_dist', 'attk' -- every agent -- or 'two_min_dist' -- RandomAgent / sample agents); the MCTS opponent (cube_layer <= 3,
 * boards <= 8x8, RandomAgent / sample agents); and the geometries without a table image (the generic kernel, see
 * ewn_step_k_supported).  The MCTS agent, and the minimax agent against the MCTS opponent, are ewn_step_k_agent's (below). */
#define EWN_AGENT_RANDOM 0  /* RandomAgent.predict (classical_policies/random_policy.py:11-15): the hash-driven uniform legal pick
                               of ewn_step_out.random_action, same stream */
#define EWN_AGENT_MINIMAX 1 /* ExpectiMinimaxAgent(agent_max_depth, 'hybrid').predict (classical_policies/minimax.py:89-93) */
#define EWN_AGENT_SAMPLE 2  /* env.action_space.sample() on MultiDiscrete([2, 3]) (envs/ewn.py:59): uniform over all six actions, illegal ones
                             * included -- what an untrained policy plays; hash-driven like EWN_AGENT_RANDOM, agent_max_depth ignored */

typedef struct ewn_rollout_out {
    /* trajectory, row k = step k of this call; every pointer may be NULL (that column is not written) */
    int8_t *board;       /* [K][N][S*S] observation after step k (after the auto-reset, like ewn_state.board after ewn_step) */
    int8_t *dice;        /* [K][N] */
    int8_t *action;      /* [K][N][2] the action the agent played at step k */
    double *reward;      /* [K][N] */
    uint8_t *terminated; /* [K][N] */
    uint8_t *truncated;  /* [K][N] */
    uint8_t *info;       /* [K][N] EWN_INFO_* */
    /* per-lane totals over the K steps, ADDED to what the buffers hold; every pointer may be NULL */
    double *return_sum;  /* [N] sum of rewards */
    int32_t *n_steps;    /* [N] steps played (a finished, un-reset lane plays none) */
    int32_t *n_episodes; /* [N] episodes finished */
    int32_t *n_wins;     /* [N] of which won ("You won!", envs/ewn.py:454) */
    /* The same trajectory as ONE record per lane-step, [K][N][EWN_TRAJ_RECORD_STRIDE(S)] bytes, 16-byte aligned; may be NULL.
     * Record = board int8 [S*S] | dice | action[2] | terminated | truncated | info | zero padding: a lane-step is one or two whole
     * 32-byte sectors written with 16-byte stores (32 bytes for 5x5, 64 for 7x7) instead of a 25-byte row at an odd offset plus
     * five 1-2 byte columns.  The reward stays in its own f64 column.  Independent of the columns above (any subset may be asked for). */
    uint8_t *record;
} ewn_rollout_out;
#define EWN_TRAJ_RECORD_STRIDE(S) ((((S) * (S)) + 6 + 15) & ~15)
#define EWN_TRAJ_REC_DICE(S) ((S) * (S))          /* byte offsets inside a record */
#define EWN_TRAJ_REC_ACTION(S) ((S) * (S) + 1)
#define EWN_TRAJ_REC_TERMINATED(S) ((S) * (S) + 3)
#define EWN_TRAJ_REC_TRUNCATED(S) ((S) * (S) + 4)
#define EWN_TRAJ_REC_INFO(S) ((S) * (S) + 5)

/* Introspection: how many lanes of a wavefront share one game in the table-driven kernel this configuration runs -- entry 0:
 * ewn_step (given ewn_state.tables), entry 1: ewn_step_k with the RandomAgent agent; 0 = a generic kernel (one thread per game).
 * The choice depends on n_lanes only (measured thresholds) unless the tuning variables EWN_D3_T /
 * EWN_ROLLOUT_T are set in the environment; tests pin the defaults. */
int ewn_lanes_per_game(const ewn_config *cfg, int entry);

/* 1 if ewn_step_k serves this configuration and agent, 0 if not, < 0 on an invalid configuration.  Geometries without a table
 * image (cube_layer 4 / 5, boards of 9x9 .. 11x11) are served by the generic one-thread-per-game K-step kernel for the RandomAgent /
 * sample agents against RandomAgent or minimax opponents of the four evaluate() heuristics (no ewn_state.tables needed). */
int ewn_step_k_supported(const ewn_config *cfg, int agent_kind, int agent_max_depth);
/* K >= 1 steps of every lane; out may be NULL (only the state advances).  No scratch; one kernel launch. */
int ewn_step_k(const ewn_config *cfg, const ewn_state *st, int K, int agent_kind, int agent_max_depth,
               const ewn_rollout_out *out, void *stream);

/* ---- K env steps per launch with an MCTS agent, or a minimax agent against the MCTS opponent: the cells of eval_pairs.py:10-35's
 * matrix that ewn_step_k does not serve -- MctsAgent against RandomAgent, minimax (the four evaluate() heuristics, max_depth 1..6) or
 * MCTS, and ExpectiMinimaxAgent(max_depth 1..6; 'hybrid', 'min_dist', 'attk', 'two_min_dist') against MCTS.  cube_layer 3, boards 5..8,
 * un-shaped; Philox dice with or without auto-reset, MT19937-compat dice without.  Results are identical, step for step, to the
 * agent's predict_minimax / predict_mcts fed to ewn_step: the MCTS agent's observation is the board as it stands (TOP_LEFT to move),
 * and at evaluation step t = step_base + k its playouts of lane n use the stream of ewn_predict_mcts with obs_id = lane_offset + n and
 * key_t = key + 0x9E3779B97F4A7C15 * (t + 1) (mod 2^64).  The MCTS opponent's stream is ewn_step_k's.  The minimax side (the agent, or
 * the opponent of the MCTS agent) runs the table-driven search of ewn_predict_minimax / ewn_step and needs ewn_state.tables. */
#define EWN_AGENT_MCTS 4    /* MctsAgent(num_simulations, num_env_copies).predict (classical_policies/mcts.py:47-69), ewn_step_k_agent only */
typedef struct ewn_agent {
    int32_t kind;             /* EWN_AGENT_MCTS, or EWN_AGENT_MINIMAX (against the MCTS opponent) */
    int32_t max_depth;        /* minimax: 1..EWN_MAX_DEPTH */
    int32_t heuristic;        /* minimax: EWN_H_*, not EWN_H_SIM_WINRATE */
    int32_t num_simulations;  /* mcts: MctsAgent.num_simulations */
    int32_t num_env_copies;   /* mcts: MctsAgent.num_env_copies */
    uint32_t step_base;       /* mcts: evaluation step index of this launch's first step */
    uint64_t key;             /* mcts: playout key (see above) */
} ewn_agent;
/* 1 if ewn_step_k_agent serves (cfg, agent), 0 if not, < 0 for an invalid cfg or agent; decided on the host */
int ewn_step_k_agent_supported(const ewn_config *cfg, const ewn_agent *agent);
/* K >= 1 steps of every lane; out may be NULL, and takes what ewn_step_k's does (columns and/or records, totals ADDED to).  One kernel
 * launch, no scratch.  Anything ewn_step_k_agent_supported does not answer 1 for returns EWN_EUNSUPPORTED / EWN_EINVAL unlaunched. */
int ewn_step_k_agent(const ewn_config *cfg, const ewn_state *st, int K, const ewn_agent *agent, const ewn_rollout_out *out, void *stream);

/* ---- K env steps per launch with the TRAINED policy as the agent: the rollout collector of train.py:35-63, 134, 148 -----------
 * (SB3 A2C("MultiInputPolicy", env, policy_kwargs=dict(activation_fn=Tanh)).learn -> collect_rollouts over SubprocVecEnv workers)
 * as one kernel: observation -> features (S*S board cells as floats ++ one_hot(dice_roll - 1), width cube_num + 1 = 7,
 * envs/ewn.py:66-68) -> policy network (SB3's default net_arch: two separate hidden-64-64 tanh bodies, 5 logits for
 * MultiDiscrete([2, 3]) and a scalar value) on the bf16 matrix pipe with every operand split into three bf16 parts (fp32 accuracy)
 * -> Gumbel-max sample -> env step (plain or
 * cfg->shaped: envs/training_ewn.py:43-99) -> opponent reply -> auto-reset.  Served for cube_layer 3, board sizes 5 and 7,
 * opponent RandomAgent or minimax max_depth 1..4 with a (level, count) heuristic image, Philox dice. */
#define EWN_AGENT_MLP 3     /* agent_kind of ewn_step_k_supported for this path (ewn_step_k itself takes no parameters: use ewn_step_k_policy) */
#define EWN_POLICY_HIDDEN 64
#define EWN_POLICY_LOGITS 5

typedef struct ewn_policy {
    const float *params;        /* [ewn_policy_param_count()] fp32, device: body pi {W1 [64][F], b1 [64], W2 [64][64], b2 [64]}, body vf
                                   {same}, action head {W [5][64], b [5]}, value head {W [1][64], b [1]}; F = S*S + 7; row-major
                                   [out][in] like torch.nn.Linear.weight -- the order of a2c.ActorCritic.parameters() */
    int32_t deterministic;      /* 1: argmax of the logits (model.predict(deterministic=True), train.py:93) instead of sampling */
    int32_t record_initial_obs; /* 1: ewn_rollout_out.record has K + 1 rows, row 0 = the observation before step 0 (meta bytes:
                                   its dice, zeros) and row k + 1 = step k; what an n-step update needs (s_0 .. s_K) */
    uint64_t noise_key;         /* keys the sampling noise together with cfg->philox_key, the global lane id, the episode seed
                                   and the episode's draw count (the hash stream of ewn_step_out.random_action) */
    /* per-step outputs of the policy, [K][N]...; each may be NULL */
    float *logits;              /* [K][N][5] */
    float *value;               /* [K][N]; non-NULL makes the kernel evaluate the value body too */
    float *noise;               /* [K][N][5] the uniforms u in (0, 1) behind the Gumbel noise -log(-log u) of that step */
} ewn_policy;

/* number of fp32 parameters of the actor-critic for this geometry (< 0: not served) */
int64_t ewn_policy_param_count(int board_size, int cube_layer);
/* K >= 1 steps of every lane, the agent's action sampled from the policy; out may be NULL.  One kernel launch, no scratch. */
int ewn_step_k_policy(const ewn_config *cfg, const ewn_state *st, int K, const ewn_policy *pol, const ewn_rollout_out *out, void *stream);

/* ---- evaluating a trained policy: train.py:66-117's per-epoch evaluation (and eval_A2C.py's loop) as K steps per launch ----------
 * The agent plays the argmax of the actor-critic's logits (model.predict(deterministic=True)) on the UN-shaped env without auto-reset,
 * one episode per lane, against RandomAgent or minimax max_depth 1..6 ('hybrid', 'min_dist', 'attk'; max_depth 5 / 6 through the
 * closed-form search), on MT19937-compat or Philox dice; cube_layer 3, board sizes 5 and 7.  The same transitions as the agent's
 * argmax fed to ewn_step step by step.  Not served ('two_min_dist', 'sim_winrate', MCTS opponents, shaped or auto-resetting envs,
 * other geometries): ewn_policy_eval returns EWN_EUNSUPPORTED.  ewn_step_k_policy / EWN_AGENT_MLP stay as documented above.
 * The MCTS opponent has a call of its own: ewn_policy_eval_mcts (below). */
/* 1 if ewn_policy_eval serves cfg, 0 if not, < 0 for an invalid cfg; decided on the host */
int ewn_policy_eval_supported(const ewn_config *cfg);
/* K >= 1 steps of every lane, the agent = argmax of the actor-critic `params` (ewn_policy.params layout); un-shaped, no auto-reset.
 * out: the four per-lane totals are required (ADDED to; return_sum is the episode's score: the un-shaped env rewards only its last
 * step); out->action is optional: row k of lane n is written only if the lane played step k of this call (a finished lane is left
 * alone); every other pointer of out must be NULL (EWN_EINVAL).  One kernel launch, no scratch; a lane whose episode is over is not
 * stepped, so a caller loops launches until ewn_state.done is set everywhere.  The MT19937-compat overflow flag is kept in the lane's
 * RNG header as ewn_step keeps it. */
int ewn_policy_eval(const ewn_config *cfg, const ewn_state *st, int K, const float *params, const ewn_rollout_out *out, void *stream);

/* ---- ... against the flat Monte-Carlo opponent (eval_A2C.py --opponent_policy mcts): opponent_kind EWN_OPP_MCTS, cube_layer 3, board
 * sizes 5 and 7, MT19937-compat or Philox dice, un-shaped, no auto-reset; everything else well-formed: EWN_EUNSUPPORTED, unlaunched.
 * The same transitions as the agent's argmax fed to ewn_step step by step: the opponent's playout stream is the one ewn_step and
 * ewn_step_k use (keyed by the lane's RNG header, not by a step index, so where a caller cuts its launches changes nothing). */
/* 1 if ewn_policy_eval_mcts serves cfg, 0 if not, < 0 for an invalid cfg; decided on the host */
int ewn_policy_eval_mcts_supported(const ewn_config *cfg);
/* ewn_policy_eval's contract with the flat Monte-Carlo opponent of cfg (num_simulations x num_env_copies playouts per
 * root move): K >= 1 steps of every lane, agent = argmax of the actor-critic `params`, un-shaped, no auto-reset, one
 * launch, no scratch, ewn_state.tables not needed.  out: the four totals required (ADDED to), out->action optional
 * (row k of lane n written only if the lane played step k), every other pointer NULL (EWN_EINVAL). */
int ewn_policy_eval_mcts(const ewn_config *cfg, const ewn_state *st, int K, const float *params,
                         const ewn_rollout_out *out, void *stream);

/* ---- a trained policy as the OPPONENT (the reference's `A2C.load(opponent_policy)`, envs/ewn.py:265-296): self-play ----
 * After the agent's move the opponent's actor-critic sees the canonical view np.rot90(-board, 2) with the opponent's dice
 * (opponent_action, envs/ewn.py:289-296) and its [flag, dir] is played as it is.  A move that leaves the board, or that asks for
 * a cube that is gone, ends the game as envs/ewn.py:469-473 does: reward 0, terminated, truncated, EWN_INFO_INVALID_OPP, board
 * and dice left as they were after the agent's move.  The policy opponent draws NOTHING from the lane's dice stream (like the
 * minimax opponent): per step the stream gives the opponent's dice and then the next dice.
 * deterministic: 1 the argmax of each head (ewn_step_k_policy's comparisons, so ties break as the agent's do), 0 a Gumbel-max
 * sample whose five uniforms are pol_uniform(w, i) of ewn_step_k_policy's noise with
 *   w = fmix32(agent_hash(the step's agent-hash arguments, philox_key ^ noise_key) ^ 0x4F505031):
 * the agent-hash stream at the START of the step under the opponent's own key, never the dice stream.  The reference's
 * `predict` arithmetic (stable_baselines3) is not vendored: parity unpinned, as for the agent; both modes are offered.
 * These calls do NOT read the opponent fields of cfg (opponent_kind, max_depth, heuristic, num_simulations, num_env_copies):
 * any values there are accepted.  cube_layer 3, board sizes 5 and 7; anything else well-formed: EWN_EUNSUPPORTED, unlaunched. */
typedef struct ewn_opponent_policy {
    const float *params;     /* ewn_policy.params layout, device; may equal the agent's pointer; frozen for the launch */
    int32_t deterministic;   /* 1: argmax, 0: Gumbel-max sample */
    uint64_t noise_key;      /* sampling only */
    int8_t *action;          /* [K][N][3] {dice, flag, dir} of the opponent's move in step k, {0, 0, 0} when it did not move; may be NULL */
} ewn_opponent_policy;
/* 1 if ewn_step_k_selfplay serves cfg with this pol (only pol->value is looked at; pol may be NULL), 0 if not, < 0 for an
 * invalid cfg.  Philox dice only; 7x7 with pol->value set is not served (three weight images do not fit the CU's LDS). */
int ewn_step_k_selfplay_supported(const ewn_config *cfg, const ewn_policy *pol);
/* ewn_step_k_policy's contract with the opponent = opp.  opp->action row k of lane n is written for every lane (a frozen
 * lane: {0, 0, 0}). */
int ewn_step_k_selfplay(const ewn_config *cfg, const ewn_state *st, int K, const ewn_policy *pol, const ewn_opponent_policy *opp,
                        const ewn_rollout_out *out, void *stream);
/* 1 if ewn_policy_eval_vs serves cfg, 0 if not, < 0 for an invalid cfg: un-shaped, no auto-reset, either dice kind */
int ewn_policy_eval_vs_supported(const ewn_config *cfg);
/* ewn_policy_eval's contract with the opponent = opp (ewn_state.tables is needed, as there).  opp->action row k of lane n is
 * written only if the lane played step k of this call, like out->action. */
int ewn_policy_eval_vs(const ewn_config *cfg, const ewn_state *st, int K, const float *params, const ewn_opponent_policy *opp,
                       const ewn_rollout_out *out, void *stream);

/* ---- ... for ANY agent: the env `EinsteinWuerfeltNichtEnv(opponent_policy=<path>)` as eval_random.py, eval_minimax.py, play_gym.py and
 * an SB3 wrapper step it.  The same opponent (view, argmax / Gumbel-max, noise word, illegal-move rule, nothing drawn from the dice
 * stream) as above; a step here is, bit for bit, the step ewn_step_k_selfplay / ewn_policy_eval_vs make for the same agent action.
 * cube_layer 3, board sizes 5 and 7, plain or cfg->shaped; Philox dice, or MT19937-compat dice without auto-reset (with it:
 * EWN_EUNSUPPORTED).  The opponent fields of cfg are not read; ewn_state.tables is needed.  One kernel launch, no scratch. */
/* 1 if ewn_step_vs serves cfg, 0 if not, < 0 for an invalid cfg; decided on the host */
int ewn_step_vs_supported(const ewn_config *cfg);
/* ewn_step's contract (actions, frozen lanes, auto-reset, terminal observation) with the opponent = opp; out->random_action must be
 * NULL (EWN_EINVAL).  opp->action, if given, is [N][3]: written for every lane ({0, 0, 0}: the opponent did not move). */
int ewn_step_vs(const ewn_config *cfg, const ewn_state *st, const int8_t *actions, const ewn_opponent_policy *opp, const ewn_step_out *out,
                void *stream);
/* 1 if ewn_step_k_vs serves (cfg, agent), 0 if not (EWN_AGENT_MLP: that is ewn_step_k_selfplay; EWN_AGENT_MCTS: not built), < 0 for
 * an invalid cfg or agent.  EWN_AGENT_RANDOM / EWN_AGENT_SAMPLE, or EWN_AGENT_MINIMAX ('hybrid') of agent_max_depth 1..6. */
int ewn_step_k_vs_supported(const ewn_config *cfg, int agent_kind, int agent_max_depth);
/* ewn_step_k's contract (columns and / or records, totals ADDED to, out may be NULL) with the opponent = opp, plain or shaped: the same
 * as K ewn_step_vs calls with the agent's action fed back.  The stand-in agents draw from ewn_step_k's hash stream; the minimax agent
 * plays ewn_predict_minimax on the observation.  opp->action, if given, is [K][N][3], written for every lane. */
int ewn_step_k_vs(const ewn_config *cfg, const ewn_state *st, int K, int agent_kind, int agent_max_depth,
                  const ewn_opponent_policy *opp, const ewn_rollout_out *out, void *stream);

/* ---- the A2C update on the records of ewn_step_k_policy: stable_baselines3 A2C.train as train.py:35-63, 148 configures it ----
 * (n-step returns = GAE with lambda 1, no advantage normalisation; loss = policy gradient + vf_coef * MSE(returns, values) +
 * ent_coef * (-entropy), a mean over the n_steps x lanes batch; clip_grad_norm_(max_grad_norm); RMSprop(alpha, eps)).  SB3 is not
 * vendored: parity with it is unpinned, the arithmetic is checked against torch autograd of the same loss.  Forward (recomputed from
 * the records: the parameters have not changed since the rollout) and backward run on the bf16 matrix pipe with every operand split
 * into three bf16 parts (six products per multiply: fp32 accuracy, measured against float64 -- tools/a2c_accuracy.py). */
typedef struct ewn_a2c_hyper {
    float gamma;            /* 0.99 */
    float vf_coef;          /* 0.5 */
    float ent_coef;         /* 0.0 */
    float max_grad_norm;    /* 0.5; <= 0: no clipping */
    float learning_rate;    /* SB3 A2C default 7e-4; train.py passes its own (3e-4) */
    float rms_alpha;        /* 0.99 */
    float rms_eps;          /* 1e-5 */
    int32_t world_size;     /* ewn_a2c_apply divides the (all-reduced, summed) gradient by it */
} ewn_a2c_hyper;

/* bytes of device scratch ewn_a2c_grad needs (advantages [K][N], per-block partial gradients and loss sums, then 64 floats that only
 * a timing build writes); < 0: configuration not served */
int64_t ewn_a2c_scratch_bytes(const ewn_config *cfg, int K);
/* record: [K + 1][N][EWN_TRAJ_RECORD_STRIDE(S)] written by ewn_step_k_policy with record_initial_obs = 1; reward [K][N].
 * grad [ewn_policy_param_count() + 8]: the gradient of THIS rank's mean loss in the layout of ewn_policy.params, then eight loss sums
 * over the K * N samples (divide by K * N for means), {policy, value, entropy, 0} of the policy pass and then of the value pass.  Each
 * pass counts only its own: [P + 0] policy loss -(adv log pi(a)), [P + 2] entropy, [P + 5] squared error (R - V)^2; [P + 1], [P + 3],
 * [P + 4], [P + 6] and [P + 7] are exactly 0.  Three launches. */
int ewn_a2c_grad(const ewn_config *cfg, int K, const uint8_t *record, const double *reward, const float *params, const ewn_a2c_hyper *hp,
                 float *grad, void *scratch, void *stream);
/* clip by the global norm, then one RMSprop step on params / sq_avg (both [param count], in place); grad_norm_out (may be NULL)
 * receives the norm before clipping.  A multi-GPU job all-reduces (sums) grad between the two calls -- the one collective. */
int ewn_a2c_apply(const ewn_config *cfg, float *params, float *sq_avg, const float *grad, const ewn_a2c_hyper *hp, float *grad_norm_out,
                  void *stream);

/* ---- the PPO update on the records of ewn_step_k_policy: stable_baselines3 PPO.train as train.py:39-49, 178-183 configures it, in the
 * arithmetic of ewn_gym_amd/ppo.py's PPOTrainer (parity with SB3 unpinned, as for A2C).  Per update: ewn_ppo_prepare once (behaviour-
 * policy log-probabilities, values, GAE(lambda) advantages and returns), ewn_ppo_shuffle once (every epoch's minibatch order), then per
 * minibatch ewn_ppo_grad, the all-reduce of a multi-GPU job, ewn_ppo_apply.  Sample s = t * N + lane.  Served where ewn_a2c_* is
 * (cube_layer 3, 5x5 and 7x7; anything else EWN_EUNSUPPORTED); K < 1 or batch_size outside [1, K * N]: EWN_EINVAL. */
typedef struct ewn_ppo_hyper {
    float gamma;               /* 0.99 */
    float gae_lambda;          /* 0.95 */
    float clip_range;          /* 0.2: the ratio is clamped to [1 - clip_range, 1 + clip_range] */
    float vf_coef;             /* 0.5 */
    float ent_coef;            /* 0.0 */
    float max_grad_norm;       /* 0.5; <= 0: no clipping */
    float learning_rate;       /* 3e-4 */
    float adam_beta1;          /* 0.9 */
    float adam_beta2;          /* 0.999 */
    float adam_eps;            /* 1e-5 */
    int32_t normalize_advantage; /* 1: (A - mean) / (std + 1e-8) over the minibatch (unbiased std, sums in double; minibatches of 2 or more) */
    int32_t world_size;        /* ewn_ppo_apply divides the (all-reduced, summed) gradient by it */
} ewn_ppo_hyper;

/* bytes of device scratch ewn_ppo_grad needs (per-block partial gradients, loss sums and advantage sums; 8-byte aligned) */
int64_t ewn_ppo_scratch_bytes(const ewn_config *cfg, int K, int batch_size);
/* record [K + 1][N][EWN_TRAJ_RECORD_STRIDE(S)] from ewn_step_k_policy with record_initial_obs = 1, reward [K][N]; params: the parameters
 * the rollout ran with.  samples [K * N][4] fp32 (16-byte aligned): {log pi(a_t | s_t), advantage, return = advantage + value, value}.
 * One launch. */
int ewn_ppo_prepare(const ewn_config *cfg, int K, const uint8_t *record, const double *reward, const float *params, const ewn_ppo_hyper *hp, float *samples, void *stream);
/* perm [n_epochs][n] int32: row e a permutation of 0 .. n - 1 keyed by (key, *counter, e) (counter: a device int32, NULL = 0; FusedPPOTrainer
 * passes its Adam step count, so a replayed graph shuffles differently every update).  A four-round Feistel network on the next even
 * power of two with cycle walking; tests/test_ppo_fused_cpu.py holds a numpy mirror.  One launch. */
int ewn_ppo_shuffle(int64_t n, int n_epochs, uint64_t key, const int32_t *counter, int32_t *perm, void *stream);
/* One minibatch: idx [batch_size] sample indices (any, e.g. a slice of perm; an index outside [0, K * N) reads sample 0).
 * grad [ewn_policy_param_count() + 8]: the gradient of the minibatch's mean loss in the layout of ewn_policy.params, then eight sums over
 * the minibatch: [P + 0] -min(A r, A clamp(r)), [P + 1] entropy, [P + 2] samples with |r - 1| > clip_range, [P + 3] (r - 1) - log r,
 * [P + 4] (R - V)^2; [P + 5 .. P + 7] are 0.  Deterministic (no atomics).  Three launches. */
int ewn_ppo_grad(const ewn_config *cfg, int K, const uint8_t *record, const float *samples, const float *params, const ewn_ppo_hyper *hp, const int32_t *idx, int batch_size, float *grad, void *scratch, void *stream);
/* clip by the global norm, then one Adam step (bias-corrected, torch's formula) on params / exp_avg / exp_avg_sq ([param count], in
 * place); *step (device int32) is the number of steps taken so far and is incremented.  grad_norm_out (may be NULL): the norm before
 * clipping.  One launch. */
int ewn_ppo_apply(const ewn_config *cfg, float *params, float *exp_avg, float *exp_avg_sq, int32_t *step, const float *grad, const ewn_ppo_hyper *hp, float *grad_norm_out, void *stream);

/* ---- stateless policy / rule queries on M given observations (canonical: TOP_LEFT to move) ---- */

/* get_legal_actions (envs/ewn.py:338-375), find_cube_to_move (:178-215), check_win (:131-142).
 * player: 1 TOP_LEFT, 2 BOTTOM_RIGHT (constants/player.py).  Outputs (each may be NULL):
 * acts [M][6][2] (-1 padded, reference order), n_acts [M], cube_small/cube_large [M]
 * (cube NUMBER moved with flag 0 / 1), win [M]. */
int ewn_legal_actions(int board_size, int cube_layer, int M, const int8_t *boards, const int8_t *dice, int player,
                      int8_t *acts, int8_t *n_acts, int8_t *cube_small, int8_t *cube_large, uint8_t *win, void *stream);

/* make_simulated_action (envs/ewn.py:377-412) on M positions: player (1 TOP_LEFT / 2 BOTTOM_RIGHT) moves the cube its
 * dice selects ([flag, dir] as in step).  new_boards [M][S*S] receives the position after the move (unchanged when the
 * move leaves the board); valid [M] (may be NULL) is 1 for a legal move.  The host keeps the undo history. */
int ewn_apply_action(int board_size, int cube_layer, int M, const int8_t *boards, const int8_t *dice, int player,
                     const int8_t *actions, int8_t *new_boards, uint8_t *valid, void *stream);

/* MinimaxEnv.simulate (envs/minimax_ewn.py:215-238), the 'sim_winrate' heuristic: n_sims uniformly random playouts
 * from each position, `first_player` (1/2) moving first; wins [M] = playouts TOP_LEFT won.  Statistical parity only
 * (the reference draws from an unseeded Python `random`); randomness as in ewn_predict_mcts with block {0, m, 0, 'SIMU'}
 * and playout number r. */
int ewn_playout_wins(int board_size, int cube_layer, int M, const int8_t *boards, int first_player, int n_sims,
                     uint64_t key, int32_t *wins, void *stream);

/* MinimaxEnv.evaluate(heuristic) (envs/minimax_ewn.py:29-213) */
int ewn_evaluate(int board_size, int cube_layer, int M, const int8_t *boards, int heuristic, double *out, void *stream);

/* ExpectiMinimaxAgent.predict (classical_policies/minimax.py:89-93): actions [M][2];
 * values [M] = root value (may be NULL); tables: see ewn_build_tables (may be NULL).
 * A position that is already won/lost returns action {-1,-1} and value = evaluate(). */
int ewn_predict_minimax(int board_size, int cube_layer, int M, const int8_t *boards, const int8_t *dice, int max_depth,
                        int heuristic, int8_t *actions, double *values, const void *tables, void *stream);

/* The same with heuristic = 'sim_winrate' and an explicit key / per-observation stream id for the playouts' randomness (one
 * Philox block {0, obs_id (NULL = index), 0, 'SIMW'} per observation seeds one generator, drawn from in the order of the
 * depth-first search).  values [M] = root value (may be NULL).  Statistical parity with the reference (unseeded Python
 * `random`, envs/minimax_ewn.py:222-225); bit-exact with oracle/ewn_oracle.c, which mirrors it. */
int ewn_predict_minimax_sim(int board_size, int cube_layer, int M, const int8_t *boards, const int8_t *dice, int max_depth, uint64_t key,
                            const uint32_t *obs_id, int8_t *actions, double *values, void *stream);

/* RandomAgent.predict (classical_policies/random_policy.py:11-15) as a stateless policy:
 * uniform legal action from Philox ctr={step + (step_dev ? *step_dev : 0), lane_offset+i, 'AGNT', 0}, key.
 * step_dev (device pointer, may be NULL) lets a captured hipGraph advance the stream between replays. */
int ewn_predict_random(int board_size, int cube_layer, int M, const int8_t *boards, const int8_t *dice, uint64_t key,
                       uint32_t step, const uint32_t *step_dev, int32_t lane_offset, int8_t *actions, void *stream);

/* MctsAgent.predict (classical_policies/mcts.py:102-106, flat Monte-Carlo :47-69, rollouts :21-45).
 * wins [M][6] int32 is REQUIRED scratch/output (win count per root move, -1 = no such move).
 * obs_id [M] (NULL = 0..M-1) and key select the rollout randomness: one Philox block {0, obs_id, 0, 'MCTS'} per observation
 * gives a word; rollout r of root move i runs a 32-bit LCG started at fmix32(word + (i * total + r) * 0x9E3779B9), one draw
 * per ply (dice and move index).  The result does not depend on how rollouts are distributed over lanes.  Statistical parity
 * with the reference (never-seeded Python `random`, mcts.py:29-32); bit-exact with oracle/ewn_oracle.c, which mirrors it. */
int ewn_predict_mcts(int board_size, int cube_layer, int M, const int8_t *boards, const int8_t *dice,
                     int num_simulations, int num_env_copies, uint64_t key, const uint32_t *obs_id, int8_t *actions,
                     int32_t *wins, void *stream);

/* The trained actor-critic as a stateless policy: model.predict(obs, deterministic=True) of the reference (train.py:89, eval_A2C.py)
 * on M observations, no env behind it.  params: the ewn_policy.params layout, [ewn_policy_param_count()] fp32; served where that
 * count is (cube_layer 3, board sizes 5 and 7), EWN_EUNSUPPORTED elsewhere.  actions [M][2] is required; logits [M][5] and value [M]
 * may be NULL (the value body runs only when value is given).  The network is ewn_step_k_policy's, operand for operand: a recorded
 * step of a rollout, replayed here on its observation with its ewn_policy.noise row as `uniforms`, returns the recorded logits, value
 * and action bit for bit.  deterministic != 0: a[0] = l1 > l0, a[1] = first argmax of (l2, l3, l4).  Otherwise the Gumbel-max of
 * l[i] - ln(-ln u[i]): u = uniforms[m][0..4] (fp32 in (0, 1)) if given, else u[i] = ((fmix32(w + (i + 1) * 0x9E3779B9) >> 9) + 0.5) / 2^23
 * with w = fmix32(fmix32(fmix32(id) ^ fmix32((uint32_t)key ^ 'AGNT') ^ (uint32_t)(key >> 32) * 0x85ebca6b) ^ 'PRED'), id = obs_id[m]
 * (NULL = m), fmix32 the MurmurHash3 finaliser: a function of (key, id) alone, not of M or of the order of the observations.
 * dice outside 1..6 is the caller's error (it selects no memory: the one-hot is arithmetic).  One kernel launch on `stream`, no
 * allocation, no synchronisation, no scratch; M == 0 is EWN_OK without a launch.  Reads exactly boards[0 .. M*S*S), dice[0 .. M),
 * obs_id[0 .. M), uniforms[0 .. 5 M); writes exactly the M rows of the outputs given. */
int ewn_predict_policy(int board_size, int cube_layer, int M, const int8_t *boards, const int8_t *dice, const float *params,
                       int deterministic, uint64_t key, const uint32_t *obs_id, const float *uniforms, int8_t *actions, float *logits,
                       float *value, void *stream);

/* One-ply lookahead on the trained critic: what the actor-critic plays when it searches one agent move and one reply ahead and asks
 * its own value net V (ewn_predict_policy's `value`) at the next agent-to-move state.  Per observation (agent = TOP_LEFT; dice outside
 * 1..6 are clamped), for the six env actions (f, r):  Q[f][r] = -inf if the move of find_cube_to_move(f) in direction r leaves the
 * board; +terminal_value if the board after it, b1, has the agent on the far corner or no opposing cube; otherwise
 * 1/6 sum_{d1 = 1..6} min over BOTTOM_RIGHT's legal replies under d1 of W, W = -terminal_value if the board after the reply, b2, has
 * the opponent on (0, 0) or no agent cube, else 1/6 sum_{d2 = 1..6} V(b2, d2).  Plain expectiminimax, no alpha-beta window: Q is a
 * continuous function of the leaf values.  actions [M][2] (required): the first maximum of Q in (f, r) order (strict >); q [M][6] may
 * be NULL.  A row that is already over (check_win) or has no agent cube gets action (0, 0) and six -inf.  params: the
 * ewn_policy.params layout; served where ewn_policy_param_count() is (EWN_EUNSUPPORTED elsewhere); a non-finite terminal_value is
 * EWN_EINVAL.  One kernel launch on `stream`, no allocation, no synchronisation, no scratch; M == 0 is EWN_OK without a launch.  Reads
 * exactly boards[0 .. M*S*S), dice[0 .. M); writes exactly the M rows of the outputs given. */
int ewn_predict_lookahead(int board_size, int cube_layer, int M, const int8_t *boards, const int8_t *dice,
                          const float *params, float terminal_value, int8_t *actions /* [M][2] */,
                          float *q /* [M][6], optional */, void *stream);

/* The two ends of ewn_predict_lookahead's tree as calls of their own, so that the leaves can be valued by something else than the plain
 * critic -- by ewn_predict_lookahead itself: a two-move lookahead (agent, reply, agent, reply, critic).  Tuple t = 18 root + 3 (cube - 1)
 * + direction, root = 3 f + r: the agent's move (f, r), then the reply of BOTTOM_RIGHT's cube `cube` in direction 0 left / 1 up /
 * 2 up-left.  Leaf row of (m, t, d2) = (m * 108 + t) * 6 + d2 - 1: 648 rows per observation.
 *
 * ewn_lookahead_expand: kind [M][108] int8: 0 no such reply (the cube is not on b1, the reply leaves the board, the root leaves the
 * board or wins, or roots 3..5 when both flags name one cube), 1 the reply wins for the opponent, 2 a leaf.  leaf_boards [648 M][S*S] and
 * leaf_dice [648 M]: b2 (the observation after both moves) and d2 where kind == 2, an all-zero board and d2 elsewhere.  Every row is
 * written on every call (a degenerate observation: 108 zeros, zero boards); nothing has to be cleared.
 *
 * ewn_lookahead_reduce: leaf [648 M][leaf_width] float, leaf_width 1 (a value) or 6 (a q row); a row's value is the maximum of its
 * entries.  W = the six values of a kind-2 tuple summed in d2 order times 1/6f, -terminal_value for kind 1, +inf for kind 0; then R, Q
 * and the action exactly as ewn_predict_lookahead takes them (the roots are read off boards and dice again; kind only selects, it never
 * indexes; rows of leaf whose kind is not 2 are not read).  actions [M][2] is required, q [M][6] may be NULL.  With leaf = the `value`
 * of ewn_predict_policy on expand's rows the result is ewn_predict_lookahead's, bit for bit.
 *
 * Both: EWN_EINVAL for M < 0 or 648 M > INT_MAX, EWN_EUNSUPPORTED where ewn_policy_param_count() is, EWN_OK without a launch for
 * M == 0, EWN_ENULL for a missing required pointer, then (reduce) EWN_EINVAL for a non-finite terminal_value or a leaf_width other
 * than 1 or 6.  One kernel launch on `stream`, no allocation, no synchronisation, no scratch. */
int ewn_lookahead_expand(int board_size, int cube_layer, int M, const int8_t *boards, const int8_t *dice,
                         int8_t *leaf_boards /* [648 M][S*S] */, int8_t *leaf_dice /* [648 M] */, int8_t *kind /* [M][108] */,
                         void *stream);
int ewn_lookahead_reduce(int board_size, int cube_layer, int M, const int8_t *boards, const int8_t *dice, const int8_t *kind,
                         const float *leaf /* [648 M][leaf_width] */, int leaf_width, float terminal_value,
                         int8_t *actions /* [M][2] */, float *q /* [M][6], optional */, void *stream);

/* ---- a PUCT search on the trained actor-critic, staged like the above: tree kernels at the two ends, ewn_predict_policy in the
 * middle (which holds the definition: nodes, edges, chance by the least visited dice, selection, backup, result).
 * A tree is ewn_puct_tree_bytes() bytes, 4-byte aligned, trees back to back; its layout is documented in DESIGN.md 4o and in
 * csrc/ewn_puct.hip and carries a version in its header.  sims: 0 .. 4096 simulations, a tree holds at most sims + 1 nodes.
 *
 * ewn_puct_tree_bytes: bytes of one tree; EWN_EUNSUPPORTED where ewn_policy_param_count() is, else EWN_EINVAL for sims outside 0 .. 4096.
 * ewn_puct_begin: writes every byte of the M trees (nothing has to be cleared), makes the root the pending leaf -- or marks the tree
 * degenerate where the observation is already over or a side has no cube -- and writes the M leaf rows: leaf_boards [M][S*S],
 * leaf_dice [M] (dice outside 1..6 are clamped; a degenerate tree: a zero board with dice 1).
 * ewn_puct_advance: per tree, if a leaf is pending, evaluates it from row m of logits [M][5] / value [M] (ewn_predict_policy's
 * outputs on the leaf rows) and backs up; then, if fewer than `sims` simulations have begun, runs one down to its pending leaf or
 * its immediate end at a winning move.  Writes row m of leaf_boards / leaf_dice on every call: the pending observation, or a zero
 * board with dice 1.  The tree is updated in place; `sims` is the one begin was given (a tree of another budget is left alone).
 * sims + 1 calls after begin complete the search.
 * ewn_puct_result: actions [M][2] (required): the first root move that wins if there is one, else the first maximum (strict >) of
 * the root's visits over the searched moves; visits [M][6] int32, q [M][6] (-inf not an action, +1 wins, W / N or 0 searched, in
 * units of the terminal value) and value [M] (sum W / sum N or 0) may be NULL.  A degenerate row: (0, 0), zero visits, six -inf, 0.
 *
 * Refusals in this order: EWN_EINVAL for M < 0 or M > INT_MAX / 64, EWN_EUNSUPPORTED where ewn_policy_param_count() is, EWN_OK
 * without a launch for M == 0, EWN_ENULL for a missing required pointer, then EWN_EINVAL for sims outside 0 .. 4096, a tree that is
 * not 4-byte aligned, a terminal_value that is not finite and positive, or a c_puct that is not finite and >= 0.  Each is one kernel
 * launch on `stream`, no allocation, no synchronisation, no atomics, no random numbers: the same inputs give the same bits. */
int64_t ewn_puct_tree_bytes(int board_size, int cube_layer, int sims);
int ewn_puct_begin(int board_size, int cube_layer, int M, int sims, const int8_t *boards, const int8_t *dice, void *tree,
                   int8_t *leaf_boards /* [M][S*S] */, int8_t *leaf_dice /* [M] */, void *stream);
int ewn_puct_advance(int board_size, int cube_layer, int M, int sims, float c_puct, float terminal_value, void *tree,
                     const float *logits /* [M][5] */, const float *value /* [M] */, int8_t *leaf_boards, int8_t *leaf_dice,
                     void *stream);
int ewn_puct_result(int board_size, int cube_layer, int M, const void *tree, int8_t *actions /* [M][2] */,
                    int32_t *visits /* [M][6], optional */, float *q /* [M][6], optional */, float *value /* [M], optional */,
                    void *stream);

/* ---- PUCT self-play: exploration at the root and the move of a game, on the trees above ----
 * ewn_puct_advance_noise is ewn_puct_advance in every respect but one: when the node it evaluates is node 0, the root's priors are
 * mixed with the caller's weights before the backup and before the first simulation selects on them (that simulation begins in
 * the same launch, so the mixing cannot be a later kernel).  With eta[a] = root_noise[m][a] where edge a has kind 1 or 2 and the
 * number is finite and positive, 0 otherwise, and es the fp32 sum of eta in ascending a:
 *   es > 0:  P[a] = fl(fl(keep * P[a]) + fl(noise_eps * fl(eta[a] / es)))  on the edges of kind 1 or 2,  keep = fl(1 - noise_eps),
 *   es == 0: the priors stay as they are.
 * The weights are un-normalised (Gamma(alpha) variates give Dirichlet(alpha) noise over the legal edges); their sum must not overflow.
 * Refusals in ewn_puct_advance's order, with root_noise == NULL among the pointers (EWN_ENULL) and, last, a noise_eps that is not
 * finite or outside [0, 1] (EWN_EINVAL).  With noise_eps == 0 every written byte equals ewn_puct_advance's.
 *
 * ewn_puct_play plays one ply of M games off their searched trees.  game [M][4] int32, 4-byte aligned: {ply, over (0 / 1), winner, 0};
 * winner 0 none, +1 the side that moves at even plies, -1 the other.  The position played is the tree's root board and dice (the
 * budget is read from the first tree's header).  rec_* address this ply's row of the caller's record; each may be NULL.  Per game:
 *  1. not live -- over != 0, or the tree is degenerate, or the root has no edge of kind 1 or 2, or the buffer is no tree of this
 *     layout (ewn_puct_advance's checks): rec_live 0 and the other record rows zero; boards, dice and ply are not touched; a tree
 *     (degenerate or without a move) whose game was not over sets over = 1 and leaves winner 0.
 *  2. o = philox4x32_10(ctr = {ply, lo32(g), hi32(g), 0x50555350}, key = {lo32(key), hi32(key)}), g = game_offset + m.
 *  3. the edge: the first root edge of kind 1; else, with tn the sum of N over the edges of kind 2: if ply < temp_plies and tn > 0,
 *     r = (uint64(o[0]) * tn) >> 32 and the edge is the first of kind 2 in ascending a whose running sum of N exceeds r (integers
 *     only, proportional to the visits, an edge with N == 0 is never drawn); else ewn_puct_result's first maximum of N (strict >).
 *  4. the record: rec_board [M][S*S] and rec_dice [M] the root's, rec_visits [M][6] = N, rec_value [M] = sum W / sum N or 0 (as
 *     ewn_puct_result's value), rec_action [M][2] = (a / 3, a % 3), rec_live [M] = 1.
 *  5. the move: boards[m] = flip(b1), b1 the board after the edge's move (captures as in the search); dice[m] = 1 +
 *     ((uint64(o[1]) * 6) >> 32), whose bias is below 2^-30 (6 does not divide 2^32: no face's probability is off by more than
 *     2^-32); ply += 1; an edge of kind 1 also sets over = 1 and winner = +1 if the ply just played was even, -1 otherwise.
 * Refusals in this order: ewn_puct_result's for M and the geometry, EWN_OK without a launch for M == 0, EWN_ENULL for a missing
 * tree, boards, dice or game, then EWN_EINVAL for temp_plies < 0 or a tree or game that is not 4-byte aligned.  One kernel launch
 * each on `stream`, vector stores only, no atomics, no allocation, no synchronisation: the same inputs give the same bits. */
int ewn_puct_advance_noise(int board_size, int cube_layer, int M, int sims, float c_puct, float terminal_value, void *tree,
                           const float *logits /* [M][5] */, const float *value /* [M] */, const float *root_noise /* [M][6] */,
                           float noise_eps, int8_t *leaf_boards, int8_t *leaf_dice, void *stream);
int ewn_puct_play(int board_size, int cube_layer, int M, const void *tree, int8_t *boards, int8_t *dice, int32_t *game /* [M][4] */,
                  int temp_plies, uint64_t key, int64_t game_offset,
                  int8_t *rec_board, int8_t *rec_dice, int32_t *rec_visits, float *rec_value, int8_t *rec_action, int8_t *rec_live,
                  void *stream);

/* ---- the PUCT search in one launch: the network inside the tree kernel ----
 * When ewn_puct_search finishes, every byte of `tree` (M trees of ewn_puct_tree_bytes(S, L, sims) bytes, the layout above) equals
 * what this sequence leaves there: ewn_puct_begin; then R rounds of ewn_predict_policy(deterministic = 1, logits, value) on the
 * leaf rows, each followed by ewn_puct_advance -- round 0 by ewn_puct_advance_noise with these root_noise and noise_eps when
 * root_noise != NULL.  R = sims + 1 when rounds < 0, min(rounds, sims + 1) otherwise; rounds == 0 is ewn_puct_begin alone.  No
 * leaf row leaves the kernel; ewn_puct_result and ewn_puct_play read the finished tree as they read a staged one.  What `tree`
 * held before the call does not matter.
 * Refusals in ewn_puct_advance_noise's order, all before the launch: EWN_EINVAL for M < 0 or M > INT_MAX / 64; EWN_EUNSUPPORTED by
 * geometry; EWN_OK without a launch for M == 0; EWN_ENULL for a missing boards, dice, params or tree; then EWN_EINVAL for sims
 * outside 0 .. 4096, a tree that is not 4-byte aligned, a terminal_value that is not finite and positive, a c_puct that is not
 * finite and non-negative and, only when root_noise is given, a noise_eps that is not finite or outside [0, 1].
 * One kernel launch on `stream`, vector stores only, no atomics, no allocation, no synchronisation; byte offsets into `tree` are
 * 64-bit.  How many trees share a block (EWN_PUCT_TILE = 1 .. 32 overrides the choice) changes no byte of the result. */
int ewn_puct_search(int board_size, int cube_layer, int M, int sims, int rounds, float c_puct, float terminal_value,
                    const int8_t *boards, const int8_t *dice, const float *params,
                    const float *root_noise /* [M][6] or NULL */, float noise_eps, void *tree, void *stream);

/* ---- whole self-play games of the PUCT search in one launch, finished columns refilled ----
 * ewn_puct_selfplay plays M games from boards [M][S*S], dice [M], game [M][4] (ewn_puct_play's {ply, over, winner, 0}) to their end
 * or to ply max_plies.  Per ply of a game: ewn_puct_search on its position (round 0 with row (ply * M + m) of `noise` when noise
 * != NULL), then ewn_puct_play with key and game_offset + m into row `ply` of the record buffers -- rows of [max_plies][M]... with
 * row stride M, each pointer may be NULL as in ewn_puct_play.  boards, dice and game are updated in place.  Every record row
 * 0 .. max_plies - 1 of every game is written: rows a game does not play (below the ply it enters with, after its end, all rows of
 * a game that enters over or with ply outside 0 .. max_plies - 1) are zeros.  The records, boards, dice and game equal what
 * the ply-by-ply sequence leaves, byte for byte; what scratch or the record buffers held before the call does not matter.
 * A block has `tile` columns (1 .. 32; 0: the library's choice) and there are `blocks` blocks (1 .. 256; 0: the library's choice),
 * never more than ceil(M / tile); block b of nb owns games b M / nb .. (b + 1) M / nb - 1, and a column whose game has ended takes
 * the block's next one.  tile and blocks change no byte of the result.  scratch: blocks x tile trees of ewn_puct_tree_bytes(),
 * 4-byte aligned; ewn_puct_selfplay_scratch_bytes returns that product for the effective values (0 for M == 0; negative: the
 * refusal for M, the geometry, sims, tile or blocks).
 * Refusals in ewn_puct_search's order, all before the launch: EWN_EINVAL for M < 0 or M > INT_MAX / 64; EWN_EUNSUPPORTED by
 * geometry; EWN_OK without a launch for M == 0; EWN_ENULL for a missing params, boards, dice, game or scratch; then EWN_EINVAL for
 * sims outside 0 .. 4096, a scratch or game that is not 4-byte aligned, a terminal_value that is not finite and positive, a c_puct
 * that is not finite and non-negative; for max_plies < 1, temp_plies < 0, tile outside 0 .. 32, blocks outside 0 .. 256; and, only
 * when noise is given, a noise_eps that is not finite or outside [0, 1].
 * One kernel launch on `stream`, vector stores only, no atomics, no allocation, no synchronisation; all row offsets are 64-bit. */
int64_t ewn_puct_selfplay_scratch_bytes(int board_size, int cube_layer, int M, int sims, int tile, int blocks);
int ewn_puct_selfplay(int board_size, int cube_layer, int M, int sims, int max_plies, float c_puct, float terminal_value,
                      const float *params, const float *noise /* [max_plies][M][6] or NULL */, float noise_eps,
                      int temp_plies, uint64_t key, int64_t game_offset, int tile, int blocks,
                      int8_t *boards, int8_t *dice, int32_t *game,
                      int8_t *rec_board, int8_t *rec_dice, int32_t *rec_visits, float *rec_value, int8_t *rec_action, int8_t *rec_live,
                      void *scratch, void *stream);

/* ---- the supervised update on M given observations: targets from outside (a search: expert iteration) ----
 * loss = (1/M) sum_m w_m (pi_coef CE_m + vf_coef (V_m - v*_m)^2),  CE_m = -sum_i p_i logsoftmax_head(i)(logits_m)_i, with
 * p = target_pi[m][0..4] (entries 0-1 the flag head, 2-4 the direction head; the caller makes each head's mass 1, or 0 to mask the
 * head), v* = target_value[m], w = weight[m] (weight NULL: all ones).  A sample whose w is not > 0 contributes nothing, by selection
 * and not by multiplication, to the gradient and to every statistic: its targets may be NaN or infinite (ewn_predict_lookahead returns
 * six -inf on a finished row).  The network, the bf16 x 3 arithmetic and the backward pass are ewn_a2c_grad's.
 * grad [ewn_policy_param_count() + 8]: the gradient in the layout of ewn_policy.params (the policy pass writes the pi body and the
 * action head, the value pass the vf body and the value head: with vf_coef == 0 the value entries are exactly 0, with pi_coef == 0
 * the policy entries), then sums over the samples with w > 0: [P + 0] w CE, [P + 1] w (entropy of both heads), [P + 2] the number of
 * samples whose pick (ewn_predict_policy's deterministic comparisons) is the target's first maximum on every head with target mass,
 * [P + 3] w, [P + 4] w (V - v*)^2; [P + 5 .. P + 7] are exactly 0.  The optimiser step is ewn_a2c_apply (or ewn_ppo_apply): the same
 * grad layout.  Refusals in this order: M < 1, or M above INT32_MAX - 32 896 (the tiles are counted in an int), EWN_EINVAL;
 * EWN_EUNSUPPORTED where ewn_policy_param_count() is; EWN_ENULL for a missing pointer other than weight; EWN_EINVAL for a negative or
 * non-finite coefficient, then for a scratch that is not 4-byte aligned.  scratch: ewn_sup_scratch_bytes() bytes, 4-byte aligned (8:
 * the faster reduce kernel serves).  Reads
 * exactly boards[0 .. M*S*S), dice[0 .. M) (dice outside 1..6: the caller's error, as in ewn_predict_policy) and the M rows of the
 * targets.  Four launches on `stream`, no allocation, no synchronisation, no atomics: the same inputs give the same bits. */
int64_t ewn_sup_scratch_bytes(int board_size, int cube_layer, int M);
int ewn_sup_grad(int board_size, int cube_layer, int M, const int8_t *boards, const int8_t *dice,
                 const float *target_pi /* [M][5] */, const float *target_value /* [M] */,
                 const float *weight /* [M], may be NULL */, const float *params,
                 float pi_coef, float vf_coef, float *grad /* [P + 8] */, void *scratch, void *stream);

/* q rows of ewn_predict_lookahead -> the targets of ewn_sup_grad.  Per row the finite set is the entries above -inf.  Empty (a
 * finished observation): five zeros, value 0, weight 0.  Otherwise weight 1 and value the maximum.  temperature == 0: the first
 * maximum in (f, r) order under strict > (ewn_predict_lookahead's action) one-hot on both heads, except that the flag head gets
 * (0.5, 0.5) when q[0][r*] and q[1][r*] have equal bit patterns (both flags name one cube).  temperature > 0:
 * P(f, r) = exp((q - max) / temperature) / Z over the finite set; the flag head gets the sums over r, the direction head the sums
 * over f, in index order.  M < 0: EWN_EINVAL; M == 0: EWN_OK without a launch; a missing pointer: EWN_ENULL; then a negative or
 * non-finite temperature: EWN_EINVAL.  One launch. */
int ewn_lookahead_targets(int M, const float *q /* [M][6] */, float temperature,
                          float *target_pi /* [M][5] */, float *target_value /* [M] */,
                          float *weight /* [M] */, void *stream);

/* ---- exact endgame values: a retrograde table over every position with few cubes left ----
 * A position is seen from the side to move, before its dice; the mover is TOP_LEFT (the view ewn_predict_lookahead takes, and the one
 * the opponent gets through flip(b) = the board turned by 180 degrees with the sides swapped).  With C = S * S:
 *   E(b) = fl((m_1 + ... + m_6) * fl(1/6))      fp32, summed in dice order, one multiply
 *   m_d  = max over f in {0, 1}, r in {0, 1, 2} whose move stays on the board of G(b, d, f, r)
 *   G    = +1 if the move wins (it reaches cell C - 1, or the other side has no cube left after it), else -E(flip(b1)), b1 the board
 *          after the move; the cube is find_cube_to_move(f) under d, and the move captures whatever stands on its target.
 * (1 + E) / 2 is the mover's win probability under optimal play by both sides.  The table covers the positions with 1 .. max_cubes
 * (1..3) cubes a side and at most max_total (2 .. 2 max_cubes) in all that are live: no agent cube on C - 1, no opposing cube on
 * cell 0, cells in -6..6, no cube number twice on a side.  Boards 3x3 .. 11x11.  It holds sum over the covered (ka, ko) of n_ka n_ko
 * floats, n_k = binom(6, k) C^k; the layout is the library's own (csrc/ewn_endgame.hip) and may change with the library.
 *
 * ewn_endgame_table_bytes: the table's size, or EWN_EINVAL for parameters outside the ranges above.
 * ewn_endgame_build: fills the table on `stream`: one clear, then one launch per level of Phi = the sum of all cubes' Manhattan
 * distances to their own corners (every ply lowers it), each reading only lower levels.  No atomics: the same bits on every build,
 * whatever the buffer held; every slot is written (0 where the slot is not a live position).  Refusals in this order: EWN_EINVAL for
 * the parameters, EWN_ENULL, EWN_EINVAL for a table_bytes other than ewn_endgame_table_bytes() or a table not 4-byte aligned, then
 * EWN_EUNSUPPORTED for a table so large that a level does not fit one grid (2^31 - 1 workgroups of 256 entries).
 * ewn_endgame_lookup: per observation (board, dice; dice outside 1..6 are clamped) q [M][6] = G under that dice in (f, r) order, -inf
 * where the move leaves the board; actions [M][2] the first maximum of q (strict >); value [M] = E(b); covered [M] = 1.  A row that
 * is not covered gets (0, 0), six -inf, value 0 and covered 0, and reads nothing from the table.  q, value and covered may be NULL.
 * Refusals in this order: EWN_EINVAL for M < 0 or the parameters, EWN_OK without a launch for M == 0, EWN_ENULL, EWN_EINVAL for a
 * table not 4-byte aligned.  One launch.  Reads exactly boards[0 .. M*C), dice[0 .. M); writes exactly the M rows of the outputs given.
 * None of the three allocates or synchronises. */
int64_t ewn_endgame_table_bytes(int board_size, int max_cubes, int max_total);
int ewn_endgame_build(int board_size, int max_cubes, int max_total, float *table, int64_t table_bytes, void *stream);
int ewn_endgame_lookup(int board_size, int max_cubes, int max_total, const float *table, int M, const int8_t *boards,
                       const int8_t *dice, int8_t *actions /* [M][2] */, float *q /* [M][6], optional */,
                       float *value /* [M], optional */, uint8_t *covered /* [M], optional */, void *stream);

/* ewn_predict_lookahead with exact leaves: everything as there, except that W of a reply whose b2 the table (of
 * ewn_endgame_build for board_size, max_cubes, max_total) covers is fl(terminal_value * E(b2)), E(b2) the table's entry for b2 with
 * the agent to move, instead of the mean of the six critic values.  b2 is covered exactly where ewn_endgame_lookup would cover it.
 * An observation with a cube number twice on a side, or a cell outside -6..6, is no position of the table's: all its leaves go to
 * the critic and its row is ewn_predict_lookahead's, bit for bit.  q [M][6] may be NULL; leaf_counts [M][2] (int16) may be NULL:
 * the number of leaf tuples valued by the table, then by the critic ((0, 0) on a row that is not searched).  Refusals in this order:
 * EWN_EINVAL for M < 0, EWN_EUNSUPPORTED where ewn_policy_param_count() is negative, EWN_EINVAL for table parameters that
 * ewn_endgame_table_bytes refuses, EWN_OK without a launch for M == 0, EWN_ENULL for a missing boards, dice, params, table or
 * actions, EWN_EINVAL for a non-finite terminal_value.  One kernel launch on `stream`, no allocation, no synchronisation.  Reads
 * exactly boards[0 .. M*S*S), dice[0 .. M) and the table entries of covered leaves; writes exactly the M rows of the outputs given. */
int ewn_predict_lookahead_eg(int board_size, int cube_layer, int M, const int8_t *boards, const int8_t *dice,
                             const float *params, float terminal_value, int max_cubes, int max_total, const float *table,
                             int8_t *actions /* [M][2] */, float *q /* [M][6], optional */,
                             int16_t *leaf_counts /* [M][2], optional */, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* EWN_HIP_H */
