// internal.h -- shared between the translation units of libmapfx.so (not installed).
#ifndef MAPFX_INTERNAL_H
#define MAPFX_INTERNAL_H

#include "mapfx_partial.h"

#ifdef __cplusplus
extern "C" {
#endif
// sets the message returned by mapfx_last_error(); returns `code`
int mapfx_internal_error(int code, const char* msg);
// records the host stub of the kernel the calling thread just launched (mapfx_last_kernel)
void mapfx_note_kernel(const void* fn);
// partial.hip: mapfx_partial_step with the observation rows written to an EpisodeBatch
// time row (obs_rows + e * obs_env_stride floats, only envs with obs_mask[e] != 0)
int mapfx_partial_step_rows(mapfx_partial_t* h, const mapfx_partial_state* st, const void* actions,
                            int action_dtype, const mapfx_partial_out* out, float* obs_rows,
                            long long obs_env_stride, const uint8_t* obs_mask, void* stream);
// The runner's fused step: env e's actions are row act_row[e] (act_row_stride elements
// apart) of `actions`, stay when act_row[e] < 0; the env's actions / one-hot EpisodeBatch
// rows at ts are written where act_row[e] >= 0 (ep_actions / ep_onehot may be NULL).
// obs_rows NULL: observations go to out->obs.
typedef struct mapfx_runner_acts {
  const int32_t* act_row;
  long long act_row_stride;
  int64_t* ep_actions;
  long long ep_actions_sb, ep_actions_st;
  float* ep_onehot;
  long long ep_onehot_sb, ep_onehot_st;
  int ts;
  // runner_post_kernel's work for the envs running before the step (alive[e] != 0),
  // fused into the env step's write-back (alive NULL: not fused): the reward /
  // terminated rows at ts, returns, lengths, alive / alive_prev, and the state /
  // avail_actions / filled rows at ts + 1 (ep_state / ep_avail / ep_filled point at
  // that time row; NULL when ts + 1 == max_t or the field is absent)
  uint8_t* alive;
  uint8_t* alive_prev;
  double* ep_return;
  int64_t* ep_length;
  float* ep_reward;
  long long ep_reward_sb, ep_reward_st;
  uint8_t* ep_term;
  long long ep_term_sb, ep_term_st;
  float* ep_state;
  long long ep_state_sb;
  int32_t* ep_avail;
  long long ep_avail_sb;
  int64_t* ep_filled;
  long long ep_filled_sb;
  // The `bs` compaction for the NEXT MAC call fused into the same launch (cmp_bs NULL:
  // not fused; runner.hip runner_compact_kernel then runs after the step).  The alive
  // flags are double-buffered by step parity: `alive` is A[ts & 1] (running before this
  // step: read, never written) and `alive_prev` is A[(ts + 1) & 1] (written for every env:
  // running after this step), so the launch's first workgroup compacts A[ts & 1] -- the
  // stale list bs(ts + 1) -- while the env workgroups step.  It writes bs, the row map
  // cmp_bs_inv (bs_inv of the next step's parity), counts {len(bs), len(bs)}, env_steps
  // += len(bs) and, when not NULL, counts_out.
  const uint8_t* cmp_alive;
  int64_t* cmp_bs;
  int32_t* cmp_bs_inv;
  int32_t* cmp_counts;
  int64_t* cmp_env_steps;
  int32_t* cmp_counts_out;
  int cmp_B;
} mapfx_runner_acts;
// 1 when mapfx_partial_step_runner can take the post pass (mapfx_runner_acts.alive):
// the one-wave-per-env-group kernel; the workgroup path (N > 64, a side > 256) cannot
int mapfx_partial_fuses_post(const mapfx_partial_t* h);
int mapfx_partial_step_runner(mapfx_partial_t* h, const mapfx_partial_state* st, const void* actions,
                              int action_dtype, const mapfx_runner_acts* ra, const mapfx_partial_out* out,
                              float* obs_rows, long long obs_env_stride, const uint8_t* obs_mask,
                              void* stream);
// The fused launch of mapfx_runner_rollout: T runner steps ts = ra->ts .. ra->ts + T - 1 of
// every env.  Of `ra`: the actions / one-hot / reward / terminated rows with their strides,
// ep_state / ep_avail / ep_filled as ROW 0 pointers (the kernel adds (ts + 1) times the time
// strides below), alive = A[ts0 & 1] and alive_prev = A[(ts0 + 1) & 1] (both rewritten),
// ep_return, ep_length and cmp_env_steps (+= the envs running before each step but the
// last: the compaction after the launch adds those).  act_row and the other cmp_* are
// unused: actions are indexed by env.
typedef struct mapfx_runner_roll {
  int max_t;
  float* obs_rows;     // the observation rows' time row ts0 + 1, NULL: rows are not built
  long long obs_sb, obs_st;
  long long state_st, avail_st, filled_st;
  int32_t* stale_out;  // [E] 0 / -1: env on the last step's stale list; NULL when T == 1
} mapfx_runner_roll;
int mapfx_partial_rollout_runner(mapfx_partial_t* h, const mapfx_partial_state* st, int32_t T, const void* actions,
                                 int action_dtype, const mapfx_partial_policy* pol, const mapfx_runner_acts* ra,
                                 const mapfx_runner_roll* rr, void* stream);
int mapfx_partial_runner_rollout_offered(const mapfx_partial_t* h, int policy);
#ifdef __cplusplus
}

// ---- helpers shared by the four translation units: one definition each ----
#include <hip/hip_ext.h>
#include <hip/hip_runtime.h>
#include <stdio.h>

inline int round_up(int x, int m) { return (x + m - 1) / m * m; }

// x / d for 0 <= x < 2^32, 1 <= d < 2^16, with m = magic48(d) = ceil(2^48 / d).
inline uint64_t magic48(int d) { return ((1ull << 48) + (uint64_t)d - 1) / (uint64_t)d; }
__device__ inline int fastdiv(int x, uint64_t m) { return (int)(((uint64_t)(uint32_t)x * m) >> 48); }

// the finaliser of every counter-based draw (mapfx/rng.py splitmix64)
__host__ __device__ inline uint64_t splitmix64(uint64_t x) {
  x += 0x9E3779B97F4A7C15ull;
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}

// the wave's LDS writes before it are visible to its reads after it
__device__ inline void wave_fence() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// element idx of an int8 / int32 / int64 action buffer; any out-of-range int64 is -1 (invalid)
__device__ inline int load_action(const void* p, int dtype, long long idx) {
  if (dtype == MAPFX_I8) return (int)((const int8_t*)p)[idx];
  if (dtype == MAPFX_I32) return ((const int32_t*)p)[idx];
  const long long v = ((const int64_t*)p)[idx];
  return (v < -1 || v > 5) ? -1 : (int)v;
}

inline int perr(int code, const char* msg) { return mapfx_internal_error(code, msg); }

inline int check_hip(hipError_t e, const char* what) {
  if (e == hipSuccess) return MAPFX_OK;
  char buf[512];
  snprintf(buf, sizeof(buf), "%s: %s", what, hipGetErrorString(e));
  return perr(MAPFX_EHIP, buf);
}

// The one launch path.  The Ext form exactly when an event is given (the two are different
// runtime entry points, and a captured graph records which); NOTED records the kernel for
// mapfx_last_kernel (and resets mapfx_last_action_path to 0); returns the checked status.
enum LaunchNote { QUIET, NOTED };
template <typename... P, typename... A>
int launch_kernel(void (*fn)(P...), dim3 grid, dim3 block, unsigned lds, hipStream_t stream, hipEvent_t ev0,
                  hipEvent_t ev1, const char* what, LaunchNote note, const A&... args) {
  if (ev0 || ev1)
    hipExtLaunchKernelGGL(fn, grid, block, lds, stream, ev0, ev1, 0, args...);
  else
    hipLaunchKernelGGL(fn, grid, block, lds, stream, args...);
  if (note == NOTED) mapfx_note_kernel((const void*)fn);
  return check_hip(hipGetLastError(), what);
}
#endif
#endif
