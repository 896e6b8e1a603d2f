/*
 * mapfx_runner.h -- C ABI of the batched ParallelRunner's episode writes
 * (SURVEY.md §8(f) F2).
 *
 * The reference collects one transition per env and step through a Pipe and
 * writes it into PyMARL's EpisodeBatch with EpisodeBatch.update
 * (MARL-curve-main/src/runners/parallel_runner.py:62-76 reset, :91-173 run;
 * components/episode_buffer.py:100-134 update).  Here the E = B envs of one
 * MarlPartialBatch are stepped by mapfx_partial_step and these kernels write the
 * step's rows straight into the EpisodeBatch's device tensors, with the runner's
 * bookkeeping (which envs are still running, the MAC's `bs` list, returns,
 * lengths, env-step count) kept on the device -- no per-step host round trip:
 *
 *   reference                                   this ABI
 *   -----------------------------------------   ---------------------------------
 *   reset(): batch.update(pre_transition, ts=0) mapfx_runner_begin
 *   run(): batch.update({"actions"}, bs, ts)    mapfx_runner_actions
 *          (+ the OneHot preprocess of actions)
 *   run(): receive loop, update(post, bs, ts),  mapfx_runner_post (after
 *          update(pre, bs, ts + 1), returns,     mapfx_partial_step)
 *          lengths, envs_not_terminated (:123)
 *
 * Row semantics are the reference's, including its stale list: the MAC and the
 * actions row at step t cover the envs that were running before step t - 1
 * (`bs`), the env step and every other row the envs still running now (`alive`).
 * Tensors are caller-owned DEVICE memory; element strides of the batch (sb) and
 * time (st) dimensions; NULL = field absent.  0 / negative MAPFX_E* return codes.
 */
#ifndef MAPFX_RUNNER_H
#define MAPFX_RUNNER_H

#include <stdint.h>

#include "mapfx_partial.h"

#ifdef __cplusplus
extern "C" {
#endif

/* EpisodeBatch.data.transition_data tensors, [B][max_t][...] (PyMARL's scheme,
 * episode_buffer.py:46-86: obs / state float32, avail_actions int32, actions int64,
 * actions_onehot float32, reward float32, terminated uint8, filled int64). */
typedef struct mapfx_episode_rows {
  int32_t max_t;                                   /* episode_limit + 1          */
  float* obs;          int64_t obs_sb, obs_st;      /* [B][T][N][D]               */
  float* state;        int64_t state_sb, state_st;  /* [B][T][3]                  */
  int32_t* avail;      int64_t avail_sb, avail_st;  /* [B][T][N][5]               */
  int64_t* actions;    int64_t actions_sb, actions_st;       /* [B][T][N][1]      */
  float* onehot;       int64_t onehot_sb, onehot_st;         /* [B][T][N][5]      */
  float* reward;       int64_t reward_sb, reward_st;         /* [B][T][1]         */
  uint8_t* terminated; int64_t terminated_sb, terminated_st; /* [B][T][1]         */
  int64_t* filled;     int64_t filled_sb, filled_st;         /* [B][T][1]         */
} mapfx_episode_rows;

/* The runner's device bookkeeping for B envs of N agents and obs size D. */
typedef struct mapfx_runner_state {
  int32_t B, N, D;
  uint8_t* alive;        /* [B] env not terminated (after the last step)            */
  uint8_t* alive_prev;   /* [B] running before the last step: the stale list        */
                         /* (mapfx_runner_step with the post pass fused -- every map
                            the one-wave-per-env-group kernel takes, N <= 64 and sides
                            <= 256 -- uses the two as A[0] / A[1], A[ts & 1] = running
                            before step ts; ABI 6)                                   */
  int64_t* bs;           /* [B] ascending indices of alive_prev, padded with bs[0]: the
                            MAC's `bs` (parallel_runner.py:91, :123)                 */
  int32_t* counts;       /* [2] len(bs), number alive                               */
  double* ep_return;     /* [B] episode_returns (:139, fp64 like the Python floats)  */
  int64_t* ep_length;    /* [B] episode_lengths (:140)                              */
  int64_t* env_steps;    /* [1] env_steps_this_run (:142)                           */
  int8_t* env_actions;   /* [B][N] the actions the env step reads (mapfx_runner_actions) */
  int32_t* bs_inv;       /* [2][B] row of env b in bs, -1 when b is not in it: the fused
                            step (mapfx_runner_step) reads env b's actions from row
                            bs_inv[ts & 1][b] of the MAC's output and writes its actions
                            rows there, so no separate actions pass runs (appended in
                            ABI 4; two parity halves since ABI 6, the first one used by
                            the unfused forms) */
} mapfx_runner_state;

/* reset(): every env's observations (from `out` of mapfx_partial_reset) into row
 * ts = 0, filled = 1; every env alive, bs = 0..B-1, returns / lengths / steps 0. */
int mapfx_runner_begin(const mapfx_runner_state* rs, const mapfx_partial_out* out,
                       const mapfx_episode_rows* rows, void* stream);

/* The MAC's actions ([counts[0]] rows of N, row j for env bs[j], `row_stride`
 * elements apart, dtype MAPFX_I8 / I32 / I64) into the actions / actions_onehot rows
 * at ts and into env_actions. */
int mapfx_runner_actions(const mapfx_runner_state* rs, const void* actions, int32_t action_dtype,
                         int64_t row_stride, int32_t ts, const mapfx_episode_rows* rows,
                         void* stream);

/* After mapfx_partial_step(env_actions): for every alive env the reward /
 * terminated rows at ts and obs / state / avail_actions / filled at ts + 1 (when
 * ts + 1 < max_t), returns and lengths; then alive_prev = alive, alive &= !terminated,
 * and bs / counts recomputed from alive_prev.  The new counts are also written to
 * `counts_out` (may be pinned host memory: the host polls it behind an event
 * instead of copying; mapfx_host_ring_alloc's dev_ptr), when not NULL. */
int mapfx_runner_post(const mapfx_runner_state* rs, const uint8_t* terminated,
                      const mapfx_partial_out* out, int32_t ts, int32_t* counts_out,
                      const mapfx_episode_rows* rows, void* stream);

/* One runner step in one call: the env step of mapfx_partial_step with every env's
 * actions read from row bs_inv[b] of `actions` (stay for an env not in bs: it is no
 * longer running and nothing of it is recorded), which also writes the actions /
 * actions_onehot rows at ts of the envs in bs -- what mapfx_runner_actions does, in the
 * same launch -- then mapfx_runner_post(rs, st->terminated, out, ...).  When rows->obs
 * is set, the env step writes the observation rows of the envs running before it
 * straight into rows->obs at ts + 1 (out->obs is then not written) and the post kernel
 * copies no observation bytes.
 * One launch (ABI 6) where the env kernel fuses the post pass (mapfx_runner_state
 * alive): the compaction for the next MAC call is its first workgroup, over A[ts & 1]
 * (running before step ts), so counts / counts_out = {len(bs), envs running after step
 * ts - 1}: the running count lags one step more than mapfx_runner_post's. */
int mapfx_runner_step(mapfx_partial_t* h, const mapfx_partial_state* st, const mapfx_partial_out* out,
                      const mapfx_runner_state* rs, const void* actions, int32_t action_dtype,
                      int64_t row_stride, int32_t ts, int32_t* counts_out,
                      const mapfx_episode_rows* rows, void* stream);

/* Output mode (mapfx_partial_repair, mapfx_partial.h): after mapfx_runner_step at ts and the
 * repair of that step -- whose `out` now holds the observations of the repaired state -- the
 * obs / state / avail_actions rows at ts + 1 are written again from `out`, with
 * EpisodeBatch's dtypes, for every env b with rows->filled[b][ts + 1] != 0 (the step has
 * just written that row from the raw positions); other envs are not touched.  One small
 * launch; none when ts + 1 == max_t.  MAPFX_EINVAL: a NULL argument, out->obs / state /
 * avail or rows->filled NULL, ts outside the batch.  Additive export. */
int mapfx_runner_reobserve(const mapfx_runner_state* rs, const mapfx_partial_out* out, int32_t ts,
                           const mapfx_episode_rows* rows, void* stream);

/* T runner steps, ts = ts0 .. ts0 + T - 1, of all B envs in one call: the episode loop with
 * no MAC between the steps.  Additive exports (the ABI version is unchanged).
 *
 * The contract is an equivalence.  After the call every byte of every tensor in `rows`,
 * every array of `rs` (alive / alive_prev as the parity pair, bs, both halves of bs_inv,
 * counts, ep_return, ep_length, env_steps, env_actions) and every array of `st` equals what
 * T successive mapfx_runner_step calls at ts = ts0 .. ts0 + T - 1 leave, and `counts_out`
 * holds what the last of them writes, where row j of call ts's `actions` argument holds the
 * actions of env bs[j]:
 *   given actions: actions[ts - ts0][bs[j]] ([T][B][N] of action_dtype).  An action outside
 *     0..4 skips that env for that step and sets err, as mapfx_runner_step does.
 *   policy (actions NULL): mapfx_partial_policy's rule (mapfx_partial.h,
 *     mapfx.rng.partial_policy_actions) on env bs[j] as it stands before call ts, with the
 *     counter pol->t0 + ts -- the absolute row, so two calls of T / 2 equal one of T.
 * An env that terminated in step ts - 1 is on the stale list once more: its actions and
 * one-hot rows at ts are recorded from its resting state, and no other row of it is written.
 * Like the step form the call keeps stepping the state `st` of an env that is no longer
 * running (with its stale action, then with stay): only the runner's rows stop.  An
 * iteration that finds no env running and none stale writes no row.  The mapfx_partial_out
 * scratch of the step form is not an argument; err goes to the word given to
 * mapfx_partial_bind_err (none bound: not reported).  A NULL field of `rows` is not
 * produced; with rows->obs NULL the observation rows are not even built.
 *
 * Offered (mapfx_runner_rollout_offered) where mapfx_runner_step is one launch: the wave
 * kernel with the fused post pass, N <= 64 and sides <= 256; policy mode also needs u8 /
 * int16 goal tables (H * W <= 32767).  MAPFX_EINVAL before any launch: not offered, T < 1,
 * ts0 < 0, ts0 + T > rows->max_t, actions and pol both NULL, a bad dtype, a NULL handle,
 * state, rs (or an rs without bs_inv) or rows.
 * Asynchronous on `stream`, no allocation, no host synchronisation, graph-capturable in a
 * single-stream capture: one launch of partial_runner_rollout_kernel, then one of
 * runner_compact_kernel, which leaves bs / bs_inv / counts as the equivalence demands -- a
 * run can go on with MAC-driven mapfx_runner_step calls after a scripted prefix. */
int mapfx_runner_rollout(mapfx_partial_t* h, const mapfx_partial_state* st,
                         const mapfx_runner_state* rs, int32_t ts0, int32_t T,
                         const void* actions /* [T][B][N] of action_dtype, or NULL */,
                         int action_dtype, const mapfx_partial_policy* pol,
                         int32_t* counts_out, const mapfx_episode_rows* rows, void* stream);
/* 1 where the call is offered (policy != 0: in policy mode), else 0 */
int mapfx_runner_rollout_offered(const mapfx_partial_t* h, int policy);

/* Action selection on the device: PyMARL's EpsilonGreedyActionSelector and
 * MultinomialActionSelector (components/action_selectors.py:54-71, :23-37) as one launch,
 * its random words counter-based and keyed by the GLOBAL env id like every other stream of
 * the library -- so the actions of an env do not depend on which other rows the call holds
 * (the runner's padded or exact `bs`, a sharded or an unsharded run).  Additive exports (the
 * ABI version is unchanged).  The rule is defined by mapfx.rng.select_actions; restated:
 *
 * Row j belongs to global env gid = env_offset + (env_ids ? env_ids[j] : j); agent a of it
 * draws the word
 *   u = splitmix64(seed ^ gid*K_ENV ^ (uint32)t*K_T ^ a*K_AGENT ^ 0x700*K_STREAM)
 * (mapfx_select_word; the K_* of mapfx/rng.py, 0x700 = STREAM_SELECT).  m_i = action i is
 * available (avail NULL: every action).  greedy(v) = the first index of the maximum, a NaN
 * greater than every number (the first NaN wins), 0 when every entry is -inf: what
 * torch.max(dim)[1] returns on the CPU.
 *   MAPFX_SELECT_EPS_GREEDY: v_i = m_i ? q_i : -inf, g = greedy(v).  explore = !greedy_only
 *     && (u >> 32) < eps_q (eps_q = round(eps * 2^32): 0 never, 2^32 always, as in
 *     mapfx_partial_policy).  n = popcount(m).  explore && n > 0: the k-th available index
 *     in ascending order, k = ((u & 0xFFFFFFFF) * n) >> 32; else g (0 when nothing is
 *     available, where torch's Categorical raises).
 *   MAPFX_SELECT_MULTINOMIAL: p_i = m_i ? q_i : 0.0f.  greedy_only: greedy(p) (the masked
 *     zeros take part, as in the reference).  Else the float32 prefix sums c_0 = p_0, c_i =
 *     c_{i-1} + p_i in this order and s = c_{A-1}; s not a finite number above 0: greedy(p);
 *     else r = float((u & 0xFFFFFFFF) >> 8) * 2^-24 (exact), x = r * s (one float32
 *     rounding), and the action is the first i with c_i > x, or, if there is none, the last
 *     i with p_i > 0.
 * The distribution is the reference's (a uniform available action with probability eps,
 * else the greedy one; a draw from p / s); the numbers are this library's, not torch's.
 *
 * One launch of select_kernel<5> (A == 5) or select_kernel<0> (any other A), reported by
 * mapfx_last_kernel(); asynchronous on `stream`, no allocation, no host synchronisation,
 * graph-capturable.  rows == 0: MAPFX_OK, no launch.  MAPFX_EINVAL before any launch: NULL
 * a, q or actions; rows < 0, N < 1, A outside 1..9, rows * N >= 2^31; an unknown mode or
 * avail_form; eps_q > 2^32; a row stride smaller than the row.  An env_ids entry is used as
 * given: a padded duplicate computes the same actions as the row it duplicates. */
#define MAPFX_SELECT_EPS_GREEDY 0
#define MAPFX_SELECT_MULTINOMIAL 1
#define MAPFX_AVAIL_I32 0
#define MAPFX_AVAIL_BITS 1
typedef struct mapfx_select_args {
  int32_t rows, N, A;            /* A in 1..9 */
  const float* q;     int64_t q_sr;       /* [rows][N][A], row stride in elements */
  const void* avail;  int64_t avail_sr;   /* NULL: every action available */
  int32_t avail_form; /* MAPFX_AVAIL_I32: int32 [rows][N][A], != 0 = available (EpisodeBatch rows);
                         MAPFX_AVAIL_BITS: [rows][N] bit i = action i, u8 for A <= 8, u16 for A == 9
                         (the avail / next_mask outputs of the env calls) */
  const int64_t* env_ids;        /* [rows] or NULL: the runner's bs */
  int64_t env_offset;
  uint64_t seed, eps_q;          /* eps_q in 0 .. 2^32 */
  int32_t t, mode, greedy_only;
  int64_t* actions;   int64_t actions_sr; /* [rows][N] out, int64: PyMARL's dtype */
} mapfx_select_args;
int mapfx_select_actions(const mapfx_select_args* a, void* stream);
/* the word u above, on the host (as mapfx_action is for the action generator) */
uint64_t mapfx_select_word(uint64_t seed, int64_t gid, int32_t t, int32_t agent);

/* n int32 of host memory the device writes directly (hipHostMalloc mapped +
 * coherent): *host_ptr for the host, *dev_ptr for kernels (mapfx_runner_post's
 * counts_out).  Free with mapfx_host_ring_free(host_ptr). */
int mapfx_host_ring_alloc(int32_t n, int32_t** host_ptr, int32_t** dev_ptr);
void mapfx_host_ring_free(int32_t* host_ptr);

#ifdef __cplusplus
}
#endif
#endif /* MAPFX_RUNNER_H */
