/*
 * mapfx_primal.h -- C ABI of PRIMAL's sequential dynamics, batched.
 *
 * Paths relative to MARL-curve-main/src/envs/mapf_primal.py:
 *
 *   reference (one world per object, one agent per call)   this ABI (E worlds per call)
 *   ---------------------------------------------------    --------------------------
 *   MAPFEnv(world0, goals0, observation_size) :175-203      mapfx_primal_create + state
 *   MAPFEnv._step((agent_id, action))         :549-637      mapfx_primal_act (K calls
 *                                                           per world, in order)
 *     State.moveAgent :103-135, reward table :579-596, _observe :343-386,
 *     State.done :159-166, _listNextValidActions :639-667
 *   MAPFEnv._observe(agent_id)                :343-386      mapfx_primal_observe (Q queries
 *   MAPFEnv._listNextValidActions(agent_id,   :639-667      per world, any agents, the
 *                                 prev_action)              worlds are not changed)
 *   MAPFEnv._complete()                       :404-405
 *
 * Actions: 0 stay, 1 (0,+1), 2 (+1,0), 3 (0,-1), 4 (-1,0) (dirDict, :28); with
 * cfg.diagonal (DIAGONAL_MOVEMENT, :175) also 5 (1,1), 6 (1,-1), 7 (-1,-1), 8 (-1,1):
 * then every move is also refused (-3) when it crosses another agent's last move
 * (State.diagonalCollision :77-99: equal midpoints of (past, present) and (old, new);
 * with integer coordinates np.isclose of the halves is exact equality of the sums),
 * each agent's past position (agents_past) is part of the state, updated by a stay
 * and by a successful move (:110-112, :129-131), and next_mask has 9 bits (u16).
 * JOINT = False (the reference default, :27).
 * The stay-on-goal blocking term (:583, get_blocking_reward :513-546) is 0 unless the
 * blocking pass (mapfx_primal_blocking, after mapfx_primal_act) is run: then a stay on
 * the goal gets GOAL_REWARD + num_blocking * BLOCKING_COST and `blocking` is produced.
 * The reference asks the od_mstar3 planner for one robot's path at inflation 1 and uses
 * only its length and "no solution"; the pass assumes that planner returns optimal
 * 4-connected paths (also with DIAGONAL_MOVEMENT: the planner is called the same way),
 * so the lengths are BFS distances + 1 -- parity is pinned up to the planner.  Not
 * modelled: the planner's 5 s time limit / OutOfTimeError; JOINT stays False.  As in the
 * reference (`range(1, num_agents)`, :523) the last agent is never examined.
 * Agents start on free cells (PRIMAL keeps agents and obstacles in one array).
 *
 * Same conventions as mapfx.h: caller-owned DEVICE pointers, asynchronous on
 * `stream`, 0 / negative MAPFX_E* return codes, messages from mapfx_last_error().
 * Limits: N <= 255, H * W <= 16384, observation size 1..32.
 */
#ifndef MAPFX_PRIMAL_H
#define MAPFX_PRIMAL_H

#include <stdint.h>

#include "mapfx.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct mapfx_primal_cfg {
  int32_t H, W;          /* grid rows, cols                                      */
  int32_t n_agents;      /* N                                                    */
  int32_t n_envs;        /* E worlds                                             */
  int32_t obs_size;      /* observation_size s (:175)                            */
  int32_t map_shared;    /* 1: one obstacle map for all worlds                   */
  int32_t diagonal;      /* DIAGONAL_MOVEMENT (:175): 9 actions, agents_past     */
} mapfx_primal_cfg;

typedef struct mapfx_primal_state {
  int32_t* pos;             /* [E][N][2] (row, col), updated in place             */
  const int32_t* goal;      /* [E][N][2]                                          */
  const uint8_t* map_bits;  /* [E or 1][mapfx_map_stride(H, W)] obstacle bitmaps  */
  int32_t* past;            /* [E][N][2] agents_past (cfg.diagonal only; updated in
                               place; set it equal to pos for a fresh world, :55-66) */
} mapfx_primal_state;

/* Outputs of the k-th call of world e at index [e][k] (NULL = not produced). */
typedef struct mapfx_primal_out {
  double* reward;        /* [E][K]                                               */
  uint8_t* done;         /* [E][K] world.done() after the call                   */
  uint8_t* next_mask;    /* [E][K] bit a = action a in _listNextValidActions; u8,
                            or u16 ([E][K] uint16_t) with cfg.diagonal (9 bits)   */
  uint8_t* on_goal;      /* [E][K]                                               */
  uint8_t* valid;        /* [E][K] action_status >= 0                            */
  uint8_t* obs;          /* [E][K][4][s][s] _observe maps (poss, goal, goals, obs) */
  double* vec;           /* [E][K][3] _observe goal vector (dx, dy, mag)         */
  int32_t* err;          /* [1] 0, or 1 + index of a world given a bad agent/action */
} mapfx_primal_out;

typedef struct mapfx_primal_t mapfx_primal_t;

int mapfx_primal_create(const mapfx_primal_cfg* cfg, mapfx_primal_t** out_handle);
void mapfx_primal_destroy(mapfx_primal_t* h);

/* K calls of MAPFEnv._step per world, in order: call k of world e is
 * (agent_ids[e][k] (1-based, as the reference), actions[e][k]).
 * `out` and every member of it may be NULL (not produced); st->pos (and st->past) are
 * updated all the same.  Only elements [e][0 .. K-1] of the outputs are written.
 * A bad call -- an id outside 1..N, an action outside 0..4 (0..8 with cfg.diagonal); the
 * reference asserts, :552-557 -- stops ITS world: *out->err is set to 1 + e (the first
 * report wins), the calls of that world before it are complete, no output element of
 * that world from the bad call on is written (the caller's bytes stay as they were), and
 * st->pos / st->past of that world are the state after its last good call.  Every other
 * world runs all its K calls.
 * out->obs must be 4-byte aligned (MAPFX_EINVAL before any launch otherwise: the
 * records leave as dwords).  The one-world-per-wave kernel (primal_seq_kernel: even
 * obs_size 4..10, N <= 64, H and W + obs_size <= 64) writes 16-byte runs and is only
 * taken when out->obs is 16-byte aligned or NULL; any other 4-byte aligned pointer gets
 * the lane-group kernel (primal_act_kernel), with the same results. */
int mapfx_primal_act(mapfx_primal_t* h, const mapfx_primal_state* st, const int32_t* agent_ids,
                     const int32_t* actions, int32_t K, const mapfx_primal_out* out, void* stream);

/* mapfx_primal_act with the launch's own start / stop timestamps recorded into
 * `start_event` / `stop_event` (hipEvent_t, created by the caller) at the kernel's
 * begin and end (hipExtLaunchKernel): the kernel duration, without the host's
 * launch gaps.  NULL events: plain mapfx_primal_act. */
int mapfx_primal_act_timed(mapfx_primal_t* h, const mapfx_primal_state* st, const int32_t* agent_ids,
                           const int32_t* actions, int32_t K, const mapfx_primal_out* out,
                           void* start_event, void* stop_event, void* stream);

/* _observe (:343-386), _listNextValidActions (:639-667), on_goal (:633) and State.done
 * (:159-166) of the worlds AS THEY STAND.  Nothing in `st` is written (pos, past).
 * Query q of world e asks about agent agent_ids[e][q] (1-based) with previous action
 * prev_actions[e][q].  agent_ids NULL: Q must equal N and query q is agent q + 1.
 * prev_actions NULL: 0 for every query (opposite_actions[0] removes nothing).
 * Outputs at [e][q] of out->obs, vec, next_mask (u8, or u16 with cfg.diagonal), on_goal,
 * done (the same value for every q of a world); out->reward and out->valid are ignored
 * and never written; any output pointer may be NULL.  out->obs must be 4-byte aligned.
 * MAPFX_EINVAL before any launch: NULL handle or state, Q < 0, agent_ids NULL with
 * Q != N, a diagonal handle without st->past.  Q == 0 or E == 0: OK, no launch.
 * A bad query (an id outside 1..N, a prev_action outside 0..nact-1) sets *out->err to
 * 1 + its world (the first report wins, as in mapfx_primal_act) and writes none of its
 * own output elements.  Unlike mapfx_primal_act, where a bad call stops its world
 * (later calls depend on it), queries do not depend on each other: every other query,
 * those of the same world included, still produces its result. */
int mapfx_primal_observe(mapfx_primal_t* h, const mapfx_primal_state* st,
                         const int32_t* agent_ids, const int32_t* prev_actions,
                         int32_t Q, const mapfx_primal_out* out, void* stream);

/* get_blocking_reward(agent_ids[e]) (:513-546) of every world at st->pos as it stands
 * (the agent need not be on its goal, as in the reference): counts[e] = num_blocking
 * (0 for an id outside 1..N). */
int mapfx_primal_blocking_count(mapfx_primal_t* h, const mapfx_primal_state* st,
                                const int32_t* agent_ids /* [E], 1-based */,
                                int32_t* counts /* [E] */, void* stream);

/* The blocking term of the K calls a mapfx_primal_act launch has just made: same h,
 * agent_ids, actions and K, same stream, st->pos as that launch left it, valid /
 * on_goal as it wrote them.  For every executed call with action 0 and on_goal 1:
 * reward[e][k] = 0.0 + n * -1.0, blocking[e][k] = n > 0, counts[e][k] = n; every
 * other element of the three arrays: reward untouched, blocking = 0, counts = 0.
 * reward, blocking, counts may each be NULL (not produced); valid and on_goal not.
 * The world call k saw is st->pos with the valid moves of the later calls undone; a
 * world that mapfx_primal_act stopped at a bad (agent, action) stops here too. */
int mapfx_primal_blocking(mapfx_primal_t* h, const mapfx_primal_state* st,
                          const int32_t* agent_ids, const int32_t* actions, int32_t K,
                          const uint8_t* valid, const uint8_t* on_goal,
                          double* reward, uint8_t* blocking, int32_t* counts, void* stream);

/* MAPFEnv._setWorld (:248-341) on the device: a new episode for every world, or for the
 * worlds with mask[e] != 0, in one launch and in place -- a random square world, the
 * agents on random free cells, each agent's goal on a random cell of the connected
 * region it stands in (so every episode is solvable).  The distribution is the
 * reference's; the draws are this library's own counter-based splitmix64 streams
 * (mapfx/rng.py), not numpy's, keyed by the world's GLOBAL id gid = env_offset + e and
 * its episode counter ep = episode[e], so a world does not depend on how worlds are
 * sharded over handles:
 *   key(stream, idx) = splitmix64(seed ^ gid*K_ENV ^ ep*K_T ^ idx*K_CELL ^ stream*K_STREAM)
 *   draw32 = key >> 32;  pick(d, n) = (d * n) >> 32;  ties between cells: row-major.
 *   1. k = key(WORLD, 0): side = side_lut[k & (n_side-1)], thresh = prob_lut[(k >> 32) &
 *      (n_prob-1)] (mapfx.maps.primal_gen_luts builds the reference's tables, :313-314).
 *      The world is the top-left side x side corner of the H x W grid; every other cell is
 *      an obstacle, which no output of act / observe can tell from the reference's
 *      side x side world (out of bounds and wall are priced and masked alike).
 *   2. cell (r, c), r, c < side, is an obstacle iff draw32(OBST + t, r*64 + c) < (thresh >> t)
 *      (:315); t = 0, and t + 1 while fewer than N cells are free (t = 32: empty world).
 *   3. agent a = 0..N-1 in order starts on cell pick(draw32(START, a), |F|) of F, the free
 *      cells no earlier agent took (:320-325).
 *   4. agent a's goal is cell pick(draw32(GOAL, a), |R|) of R, the free cells 4-connected
 *      to its start (agents do not block, :265) without the earlier agents' goals (:327-336).
 *   5. written: pos, goal, past = pos (diagonal handles), the bitmap, episode[e] = ep + 1.
 * keep_map (blank_world, :281-305): steps 1-2 are skipped, the world's bitmap (shared or
 * not) is read as it stands and only agents and goals are placed.
 * A world with mask[e] == 0 is neither read nor written.  A bad world -- side outside
 * 1..min(H, W), side * side < N, fewer than N free cells under keep_map -- sets *err to
 * 1 + e (the first report wins) and none of its state is written; all others are generated.
 * MAPFX_EINVAL before any launch: NULL handle / state / gen (or pos, goal, episode,
 * map_bits), a map_shared handle without keep_map, a diagonal handle without st->past,
 * table lengths that are not powers of two, H or W above 64 (the kernel holds a row in
 * one 64-bit lane mask; PRIMAL's own range is SIZE = (10, 40); larger grids are out of
 * scope of the generator).  E == 0: OK, no launch. */
typedef struct mapfx_primal_gen {
  uint64_t seed;
  int64_t env_offset;          /* global id of world 0 */
  const int32_t* side_lut;  int32_t n_side;   /* device, power-of-two length; unused with keep_map */
  const uint32_t* prob_lut; int32_t n_prob;   /* device, power-of-two length; unused with keep_map */
  int32_t* episode;            /* [E] device, read and incremented for generated worlds */
  const uint8_t* mask;         /* [E] device or NULL */
  uint8_t* map_bits;           /* [E][mapfx_map_stride(H, W)] written; with keep_map: [E or 1], read only */
  int32_t keep_map;
  int32_t* err;                /* [1] */
} mapfx_primal_gen;
int mapfx_primal_generate(mapfx_primal_t* h, const mapfx_primal_state* st /* pos, goal, past written */,
                          const mapfx_primal_gen* gen, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MAPFX_PRIMAL_H */
