/*
 * mapfx_partial.h -- C ABI of the batched MARL_PARTIAL_ENV step.
 *
 * MARL_PARTIAL_ENV is the env the reference actually registers
 * (MARL-curve-main/src/envs/__init__.py:60).  Paths below are relative to
 * MARL-curve-main/src/envs/marl_partial.py:
 *
 *   reference (one env per object)              this ABI (E envs per call)
 *   ------------------------------------------  ------------------------------
 *   MARL_PARTIAL_ENV.__init__  :25-123          mapfx_partial_create
 *   __setup_agent_goal_dist    :906-928         mapfx_partial_goal_dist (BFS)
 *   reset                      :125-163         mapfx_partial_reset
 *   step                       :165-310         mapfx_partial_step
 *   get_obs / get_state / get_avail_actions
 *                              :312-391         mapfx_partial_observe
 *
 * Same conventions as mapfx.h: caller-owned DEVICE pointers, (row, col) int32
 * positions, LSB-first obstacle bitmaps of mapfx_map_stride(H, W) bytes per env,
 * asynchronous on `stream`, 0 / negative MAPFX_E* return codes, messages from
 * mapfx_last_error().  Not part of this ABI: the visualisation hooks.  The `output` mode's
 * collision repair (:262-275) is mapfx_partial_repair below; the drop-in env
 * (mapfx/envs/marl_partial.py) still runs the reference's own host form by default.
 *
 * Limits: N <= 1024, H <= 1024, W <= 1536, and for a side above 256 the BFS
 * frontier rows must fit LDS: H * ceil(W / 64) * 8 bytes plus the BFS kernel's few
 * bytes of static LDS <= 160 KB, i.e. H * ceil(W / 64) just under 20480 (every map the
 * reference ships fits: orz900d's 656 x 1491 needs 126 KB; a full 1024 x 1536 map
 * would need 196 KB and is refused by mapfx_partial_create).  N <= 64 with H, W <= 256 keeps each env in one wavefront
 * with its cell maps in LDS; otherwise one workgroup steps an env with the agents'
 * cells in an LDS hash table and the obstacle bitmap read from HBM.
 */
#ifndef MAPFX_PARTIAL_H
#define MAPFX_PARTIAL_H

#include <stdint.h>

#include "mapfx.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct mapfx_partial_cfg {
  int32_t H, W;             /* grid rows, cols                                      */
  int32_t n_agents;         /* N <= 1024                                            */
  int32_t n_envs;           /* E (this rank's shard)                                */
  int64_t env_offset;       /* global id of env 0                                   */
  int32_t episode_limit;    /* :33                                                  */
  int32_t obs_window;       /* W of the window part (:31)                           */
  int32_t obs_knn_agents;   /* K (:32)                                              */
  int32_t map_shared;       /* 1: one obstacle map for all envs                     */
  double move_reward;       /* :35 */
  double stay_reward;       /* :36 */
  double stay_goal_reward;  /* :37 */
  double node_collide_reward, edge_collide_reward, env_collide_reward; /* :38-40 */
  double complete_reward;   /* :41 */
  double complete_fac;      /* :42 */
  double gamma;             /* :45 */
} mapfx_partial_cfg;

/* Caller-owned device state of E envs. */
typedef struct mapfx_partial_state {
  int32_t* pos;             /* [E][N][2] current (row, col)                         */
  const int32_t* goal;      /* [E][N][2]                                            */
  const int32_t* init_pos;  /* [E][N][2]                                            */
  int32_t* steps;           /* [E][N] _agent_step_count                             */
  uint8_t* at_goal;         /* [E][N] _agent_at_goals                               */
  uint8_t* done;            /* [E][N] _agent_dones                                  */
  int32_t* goal_cost;       /* [E][N] _each_goal_cost                               */
  uint8_t* node;            /* [E][N] _node_collision_agents of the last step       */
  int32_t* edge;            /* [E][N] _edge_collision_agents of the last step       */
  int32_t* t;               /* [E] _step_count                                      */
  uint8_t* terminated;      /* [E] _terminated                                      */
  int32_t* total_coll;      /* [E] _total_number_collisions                         */
  const uint8_t* map_bits;  /* [E or 1][mapfx_map_stride(H, W)]                     */
  void* goal_dist;          /* [E][N][H*W] shortest-path lengths to each goal (-1:
                               obstacle / unreachable), filled by
                               mapfx_partial_goal_dist; u8 when H*W <= 255 (255
                               stands for -1; ABI 5), int16 up to 32767 cells, else
                               int32 (mapfx_partial_goal_dist_elem_size)            */
  int32_t* pdist;           /* [E][N] goal_dist of each agent's current cell, carried
                               from step to step (the reference's _new_pdist / next
                               _old_pdist, :227-233): a step reads it as opd and looks
                               up only a moving agent's npd; reset / observe refresh
                               it from the table.  INT32_MIN (never reset) or a NULL
                               pointer: looked up.  Appended in ABI 4.            */
  int16_t* pnbr;            /* [E][N][4] goal_dist of the 4 neighbours (up, down,
                               left, right; an off-grid entry is unused) of each
                               agent's current cell, written with pdist by every
                               launch of the wave kernel: a step
                               takes a moving agent's npd from it instead of a
                               dependent table lookup.  Used only with pdist and
                               u8 / int16 tables (H*W <= 32767); NULL: looked up.
                               The workgroup kernel (N > 64 or a side > 256)
                               neither reads nor writes it.
                               Appended in ABI 4.                                  */
} mapfx_partial_state;

/* Per-call outputs (device, caller-owned; NULL = not produced). */
typedef struct mapfx_partial_out {
  double* reward;           /* [E] sum(rewards) (:310), fp64 in reference op order  */
  float* obs;               /* [E][N][2*W*W + 13*K] get_obs as float32 (PyMARL)     */
  float* state;             /* [E][3] get_state (:377-387)                          */
  uint8_t* avail;           /* [E][N] 5-bit get_avail_actions mask                  */
  int32_t* err;             /* [1] 0, or 1 + env index given an action outside 0..4 */
} mapfx_partial_out;

typedef struct mapfx_partial_t mapfx_partial_t;

int mapfx_partial_create(const mapfx_partial_cfg* cfg, mapfx_partial_t** out_handle);
void mapfx_partial_destroy(mapfx_partial_t* h);
/* 2*W*W + 13*K (:377 get_obs_size) */
int32_t mapfx_partial_obs_dim(const mapfx_partial_t* h);
/* 1, 2 or 4: bytes per goal_dist entry (a path on H*W cells is shorter than H*W; the
 * u8 form (ABI 5) holds -1 as 255). */
int32_t mapfx_partial_goal_dist_elem_size(int32_t H, int32_t W);

/* BFS distance tables of every (masked) env's goals (:906-928: A* lengths on
 * the 4-connected free-cell graph == BFS levels).  The carried distances of the
 * recomputed envs become stale with their tables, so st->pdist (when non-NULL) is
 * set to INT32_MIN for them: their next step looks the distances up again, as the
 * reference reads _goal_dist afresh every step (:228-229). */
int mapfx_partial_goal_dist(mapfx_partial_t* h, const mapfx_partial_state* st,
                            const uint8_t* env_mask, void* stream);

/* reset (:125-163) of the masked envs (all when env_mask is NULL) to init_pos,
 * then get_obs / get_state / get_avail_actions of every env into `out`. */
int mapfx_partial_reset(mapfx_partial_t* h, const mapfx_partial_state* st,
                        const uint8_t* env_mask, const mapfx_partial_out* out, void* stream);

/* step (:165-310) of all E envs, then the post-step observations. */
int mapfx_partial_step(mapfx_partial_t* h, const mapfx_partial_state* st, const void* actions,
                       int action_dtype, const mapfx_partial_out* out, void* stream);

/* get_obs / get_state / get_avail_actions of the current state. */
int mapfx_partial_observe(mapfx_partial_t* h, const mapfx_partial_state* st,
                          const mapfx_partial_out* out, void* stream);

/* Device-side scenario draw: new starts and goals of the (masked) envs, the reference's
 * per-reset re-sampling (:130, __setup_agent :902-929: one of the scen files by
 * random.randint, then random.sample(lines, N)) with the library's counter-based
 * streams instead of Python's generator.  Same distribution -- a uniform file, then a
 * uniform ordered sample of N distinct lines -- but not the same numbers.
 *
 * `lines` row j of file k is (start_row, start_col, goal_row, goal_col) of that file's
 * line j (mapfx.maps.load_scen_table); the kernel trusts the table.  With u64 wrapping
 * arithmetic, splitmix64 and K_* as in mapfx_action (mapfx.h) / mapfx/rng.py,
 * gid = cfg.env_offset + e and ep = episode[e]:
 *
 *   key(stream, idx) = splitmix64(seed ^ gid*K_ENV ^ ep*K_T ^ idx*K_CELL ^ stream*K_STREAM)
 *   1. f = ((key(0x500, 0) >> 32) * n_files) >> 32
 *   2. L = n_lines[f]; L <= N: the env is bad (the reference asserts len(lines) > N)
 *   3. s_j = (key(0x600, j) & ~0xFFFF) | j for j < L   (distinct: no tie rule)
 *   4. agent a gets line sorted(s)[a] & 0xFFFF
 *   5. init_pos[e][a], goal[e][a] from that line; episode[e] = ep + 1
 *
 * so an env's instances depend on (seed, gid, ep) only, not on the sharding.
 * mapfx.rng.scen_draw restates it bit for bit. */
typedef struct mapfx_partial_scen {
  uint64_t seed;
  const int16_t* lines;    /* [F][l_max][4] device */
  const int32_t* n_lines;  /* [F] device */
  int32_t n_files, l_max;  /* F >= 1, 1 <= l_max <= 4096 */
  int32_t* init_pos;       /* [E][N][2] written */
  int32_t* goal;           /* [E][N][2] written */
  int32_t* episode;        /* [E] read, incremented for drawn envs */
  const uint8_t* mask;     /* [E] or NULL */
  int32_t* err;            /* [1] 0, or 1 + a bad env (first report wins) */
} mapfx_partial_scen;

/* One launch.  E, N and env_offset are the handle's cfg.  An env with mask[e] == 0 is
 * neither read nor written; a bad env sets *err and has none of its bytes written,
 * every other env is drawn.  MAPFX_EINVAL before any launch: a NULL handle, struct,
 * lines, n_lines, init_pos, goal, episode or err; n_files < 1; l_max outside 1..4096.
 * Goal-distance tables and pdist are not touched: follow the call with
 * mapfx_partial_goal_dist on the same mask. */
int mapfx_partial_draw(mapfx_partial_t* h, const mapfx_partial_scen* sc, void* stream);

/* Fused multi-step rollout: T successive steps of all E envs in one call, with the
 * actions given ([T][E][N]) or drawn by the on-device policy below.  Additive exports
 * (the ABI version is unchanged).
 *
 * Trajectory arrays (device, caller-owned; NULL = not produced).  Slot k of each holds
 * exactly what the k-th of T successive mapfx_partial_step calls writes to
 * mapfx_partial_out; pos and terminated hold the state after that step.  After the call
 * every array of `st` equals what those T calls leave, bit for bit (pdist, pnbr, node,
 * edge and total_coll included). */
typedef struct mapfx_partial_traj {
  double*  reward;      /* [T][E]                     as mapfx_partial_out.reward   */
  float*   obs;         /* [T][E][N][D]               NULL: rows are not even built */
  float*   state;       /* [T][E][3]                                                */
  uint8_t* avail;       /* [T][E][N]   5-bit mask of the post-step state            */
  int32_t* pos;         /* [T][E][N][2] post-step (row, col)                        */
  uint8_t* terminated;  /* [T][E]                                                   */
  int8_t*  actions;     /* [T][E][N]   policy mode only: the action each agent took */
  int32_t* err;         /* [1] as mapfx_partial_out.err, first report wins          */
} mapfx_partial_traj;

/* The on-device policy, used when `actions` is NULL: each agent walks down its own
 * shortest path, with eps-random moves.  With gid = cfg.env_offset + e, step k of the
 * call and agent a (splitmix64 and K_* as in mapfx_action, mapfx.h / mapfx/rng.py):
 *
 *   u = splitmix64(seed ^ gid*K_ENV ^ (t0 + k)*K_T ^ a*K_AGENT)     mapfx_action's word
 *   (u >> 32) < eps_q :  act = u % 5                    == mapfx_action(seed, gid, t0+k, a)
 *   otherwise         :  pd   = goal distance of the agent's cell in the pre-step state
 *                        d_m  = goal distance of neighbour m (0 up, 1 down, 2 left, 3 right)
 *                        ok_m = bit m of the PRE-step get_avail_actions mask and d_m >= 0
 *                        pd < 0 or no ok_m with d_m < pd : act = 4 (stay)
 *                        else act = the lowest m among the ok_m of minimal d_m
 *
 * eps_q runs over 0 .. 2^32: 0 is pure descent, 2^32 reproduces mapfx_action exactly.
 * The action depends on (seed, gid, t0 + k, a) and the env's state only (shard-invariant);
 * done agents get one by the same rule (the step ignores it).  The distances are the
 * carried pdist / pnbr where they apply and looked up in goal_dist where they do not
 * (pdist == INT32_MIN, pnbr == NULL).  mapfx.rng.partial_policy_actions restates the rule.
 * Policy mode is offered where the wave kernel runs (N <= 64, sides <= 256) and the goal
 * tables are u8 or int16 (H*W <= 32767); with int32 tables or on the workgroup path the
 * call returns MAPFX_EINVAL. */
typedef struct mapfx_partial_policy { uint64_t seed; uint64_t eps_q; int32_t t0; } mapfx_partial_policy;

/* The policy's rule: a setting of the handle (like mapfx_partial_bind_err), read when a
 * policy-mode call is enqueued -- under graph capture it is captured with the launch -- by
 * mapfx_partial_rollout (rows built or not) and mapfx_runner_rollout alike.  Additive.
 *
 * MAPFX_POLICY_DESCENT (the default): the rule above; every agent ignores the others.
 *
 * MAPFX_POLICY_PIBT: one-step priority inheritance with backtracking; no step it drives
 * creates an edge collision, nor a node collision except among agents that already shared
 * a cell.  u, pd, d_m and ok_m as above, p_a the agent's cell, v_{a,m} its neighbour m,
 * explore_a = (u_a >> 32) < eps_q.  The candidates of agent a, in order:
 *   pd_a < 0                            stay alone
 *   called at top level and explore_a   [u_a % 5, if that is a move m < 4 with ok_m], stay
 *   otherwise (a pushed agent always)   the ok_m moves and stay as (pd_a, 4), ascending (d, m)
 * Agents are planned in ascending (pd_a == 0, (a - t) mod N) -- t = t0 + k as an unsigned
 * 32-bit value, the non-negative modulus -- so agents off their goals come first and the
 * index priority rotates every step; one still undecided at its turn runs PLAN(a, none).
 * PLAN(a, parent), for each candidate (m, v):
 *   1. v is claimed: skip.     2. v == p_parent: skip (no swap).
 *   3. m != 4: U = the undecided agents b != a with p_b == v; |U| >= 2: skip.
 *   4. claim v; a is decided with action m.
 *   5. |U| == 1: PLAN(b, a); false (b has taken stay on v, v stays claimed): a goes on
 *      with its next candidate.     6. otherwise return true.
 *   list exhausted: action 4, claim p_a, return false.
 * Properties:
 *   - every agent is planned exactly once per step: N calls, at most 2N calls and returns;
 *   - no edge collision arises, from any state.  A claim that stands is a move only if its
 *     PLAN returned true, and true goes all the way up: nobody decided at that moment acts
 *     otherwise later.  Of a swapping pair (a: p_a -> p_b, b: p_b -> p_a) let a's standing
 *     claim be the earlier; b was then undecided, so it was the only undecided occupant
 *     of p_b (two: rule 3), a pushed it, rule 2 barred p_a, and b is planned once;
 *   - a node collision arises only among agents that shared a cell before the step.  Rule 1
 *     gives a cell to one agent, except that an exhausted agent a claims p_a whoever holds
 *     it.  A mover b into p_a claimed it while a was undecided -- then it pushed a (rule 3),
 *     a returned false and b went on to another cell -- or while a, higher in the chain,
 *     held another cell -- then a exhausts only after b returned false, i.e. b stays;
 *   - the action depends on (seed, gid, t, a) and the env's state only: shard-invariant,
 *     and two calls of T / 2 equal one of T.
 * At eps_q = 2^32 this rule does NOT reproduce mapfx_action (descent does): a draw is
 * dropped where ok_m fails or the cell is claimed, and a pushed agent does not draw.
 * mapfx.rng.partial_policy_pibt_actions restates it and is its definition.
 * Offered exactly where policy mode is (the wave kernel, u8 / int16 tables). */
#define MAPFX_POLICY_DESCENT 0
#define MAPFX_POLICY_PIBT 1
/* MAPFX_EINVAL: a NULL handle, an unknown rule, or one not offered on this handle (the
 * handle's rule is then unchanged). */
int mapfx_partial_policy_rule(mapfx_partial_t* h, int32_t rule);
/* 1: mapfx_partial_policy_rule(h, rule) succeeds; 0 otherwise. */
int mapfx_partial_policy_rule_offered(const mapfx_partial_t* h, int32_t rule);

/* T steps.  `actions` [T][E][N] of action_dtype, or NULL to use `pol`.  An action
 * outside 0..4 skips that env for that step only (env unchanged, reward 0.0, err set).
 * autoreset != 0: at the start of every step k (k = 0 included) an env whose terminated
 * flag is set is first reset exactly as mapfx_partial_reset resets a masked env, then
 * stepped; starts and goals are not redrawn, so two calls of T/2 equal one of T.
 * Asynchronous on `stream`, no allocation, no host sync (graph-capturable).
 * MAPFX_EINVAL before any launch: T outside 1..65536, a bad action_dtype, actions and pol
 * both NULL, policy mode where it is not offered.
 * N <= 64 and sides <= 256: one launch of partial_rollout_kernel (state in registers,
 * maps in LDS across the steps).  Otherwise (given actions only) the call enqueues T
 * launches of the workgroup step kernel -- and the masked reset before each with
 * autoreset -- with the same result; mapfx_partial_rollout_fused tells which. */
int mapfx_partial_rollout(mapfx_partial_t* h, const mapfx_partial_state* st, int32_t T,
                          const void* actions, int action_dtype,
                          const mapfx_partial_policy* pol,
                          int32_t autoreset, const mapfx_partial_traj* traj, void* stream);
/* 1: one launch; 0: a loop of step launches */
int mapfx_partial_rollout_fused(const mapfx_partial_t* h);

/* The device word ([1], as mapfx_partial_out.err: 0, or 1 + an env given an action outside
 * 0..4, first report wins) for the calls that take no mapfx_partial_out
 * (mapfx_runner_rollout, mapfx_runner.h).  NULL (the default): not reported.  Additive. */
int mapfx_partial_bind_err(mapfx_partial_t* h, int32_t* err);

/* Output mode (`output=True`, :262-275): after the raw step, colliding agents are moved until
 * no node or edge collision is left (solvers :645-711 and :739-820).  Call it right after
 * mapfx_partial_step, with the positions the step started from and the actions it read.
 * Additive exports (the ABI version is unchanged).
 *
 * The rule is mapfx.rng.partial_repair (mapfx/rng.py), which this call equals bit for bit.
 * The reference's: the free-cell test on the PRE-step occupancy, the raw node / edge checks,
 * the node rounds, then the edge rounds over the RAW pair set, with every quirk of the
 * solvers' count bookkeeping.  This library's own: each `while` loop is cut at max_rounds
 * rounds (the reference's can spin for ever: a swap the node repair created is in no raw
 * pair), and each random.shuffle is a counter-based order.  With splitmix64 and K_* as in
 * mapfx_action (mapfx.h / mapfx/rng.py), gid = cfg.env_offset + e, t = st->t[e] (the step
 * count after the step), r the round within its phase from 0:
 *
 *   word(site, r, owner, j) = splitmix64(seed ^ gid*K_ENV ^ (uint32)t*K_T ^ owner*K_AGENT
 *                                        ^ (r*4096 + j)*K_CELL ^ (0x800 + site)*K_STREAM)
 *
 * The items in canonical ascending order (agent index; (i, j), i < j, lexicographic; 0..3),
 * item j keyed (word & ~0xFFFF) | j, processed in ascending key order:
 *   site 0  the colliding agents of a node round        owner 0
 *   site 1  these_agents of agent a                      owner a
 *   site 2  acts_try of agent a                          owner a
 *   site 3  the pairs of an edge round                   owner 0
 *   site 4  the members of pair (i, j): (j, i) iff bit 63 of word(4, r, i, j), else (i, j)
 *
 * st->pos, st->node (the vector of the last node check) and st->edge (of the last edge check)
 * are updated in place; rewards, at_goal, goal_cost, total_coll, terminated, done, steps and t
 * stay those of the raw step, as in the reference (:216-234, 250-258, 291-299).  An env whose
 * round cap was hit keeps the positions of its last round.  An env with an action outside
 * 0..4 (the step skipped it) is not repaired: flags 0, nothing else of it written.
 * With out != NULL the observations of every env (obs, state, avail) are then produced as
 * mapfx_partial_observe produces them -- which also refreshes pdist / pnbr, stale after a
 * repair; out->reward is never written.  Asynchronous on `stream`, no allocation, no host
 * sync (graph-capturable): one launch of partial_repair_kernel (mapfx_last_kernel names it),
 * one wavefront per env, then the observe launch.
 * Offered where the wave kernel runs (N <= 64, sides <= 256).  MAPFX_EINVAL before any
 * launch: a NULL handle, state, args, old_pos, actions or flags; a bad action_dtype;
 * max_rounds outside 1..16; a handle on which the call is not offered.  E == 0: OK. */
#define MAPFX_REPAIR_NODE_RAN 1  /* flags: the node phase ran            */
#define MAPFX_REPAIR_EDGE_RAN 2  /*        the edge phase ran            */
#define MAPFX_REPAIR_NODE_CAP 4  /*        the node phase hit max_rounds */
#define MAPFX_REPAIR_EDGE_CAP 8  /*        the edge phase hit max_rounds */
/* the edge check of the FINAL positions reads above 0.  With bit 3 clear this is a swap the
 * node phase created on a step whose raw edge count was 0: the reference starts no edge phase
 * then (:269), so the swap stays, there as here.  st->edge still holds the last check the
 * rule made. */
#define MAPFX_REPAIR_SWAP_LEFT 16
typedef struct mapfx_partial_repair_args {
  uint64_t seed;
  const int32_t* old_pos;      /* [E][N][2] positions before the step            */
  const void* actions;         /* the step's [E][N]                              */
  int32_t action_dtype;
  int32_t max_rounds;          /* 1..16 per phase                                */
  uint8_t* flags;              /* [E] written for every env                      */
  int32_t* rounds;             /* [E][2] rounds used (node, edge), or NULL       */
} mapfx_partial_repair_args;
int mapfx_partial_repair(mapfx_partial_t* h, const mapfx_partial_state* st, const mapfx_partial_repair_args* ra,
                         const mapfx_partial_out* out, void* stream);
/* 1: mapfx_partial_repair runs on this handle; 0 otherwise. */
int mapfx_partial_repair_offered(const mapfx_partial_t* h);

#ifdef __cplusplus
}
#endif
#endif /* MAPFX_PARTIAL_H */
