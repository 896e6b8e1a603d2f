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
// The runner's fused step (partial.hip): env e's actions are row act_row[e] (act_row_stride
// elements apart) of `actions`, stay when act_row[e] < 0; the env's actions / one-hot
// EpisodeBatch rows at ts are written where act_row[e] >= 0 (ep_actions / ep_onehot may be
// NULL).  The observation rows go to an EpisodeBatch time row (obs_rows + e * obs_env_stride
// floats, only envs with obs_mask[e] != 0); obs_rows NULL: to out->obs.
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
// partial.hip, for repair.hip: the handle's shape (big: the workgroup path, N > 64 or a side
// > 256) and the state check every mapfx_partial_* entry point makes
typedef struct mapfx_partial_shape {
  int32_t H, W, N, E, map_shared, big;
  long long map_stride, env_offset;
} mapfx_partial_shape;
int mapfx_partial_shape_of(const mapfx_partial_t* h, mapfx_partial_shape* s);
int mapfx_partial_check_state(const mapfx_partial_t* h, const mapfx_partial_state* st);

#ifdef MAPFX_SPLIT_PROBE
// ---- split protocol probe: libmapfx_probe.so only (mapfx.hip compiled with
// -DMAPFX_SPLIT_PROBE); no product path loads that library.  tests/split_protocol.py
// mirrors these numbers. ----
// the LDS resources the split rollout's three waves share
enum { MAPFX_PR_MAP, MAPFX_PR_INFO, MAPFX_PR_EDGE, MAPFX_PR_IMG, MAPFX_PR_CODE, MAPFX_PR_RTAB, MAPFX_PR_STAGE };
// access kinds; SHARE: a write to the wave's own part of a slot the waves fill together
enum { MAPFX_PK_R, MAPFX_PK_W, MAPFX_PK_RMW, MAPFX_PK_SHARE };
// annotated sites: the step wave's (role 0) and the store waves' (roles 1 and 2, parity role - 1)
enum {
  MAPFX_PS_MAP_BUILD,    // every role: its rows of both padded maps (prologue)
  MAPFX_PS_STAGE_COMMIT, // every role: its staged action rows and flag byte (prologue)
  MAPFX_PS_MAP_INIT,     // step: the agents counted into both maps
  MAPFX_PS_STAGE_FIRST,  // step: the three flags and row 0
  MAPFX_PS_MAP_RESET,    // step: autoreset re-count in map s & 1
  MAPFX_PS_MAP_MOVE,     // step: step s's move in map s & 1
  MAPFX_PS_STAGE_NEXT,   // step: the next step's action row
  MAPFX_PS_EDGE_PREV,    // step: edge counts of step s - 1
  MAPFX_PS_INFO_W,       // step: info words of step s
  MAPFX_PS_EDGE_LAST,    // step: edge counts of the launch's last step (slot 2)
  MAPFX_PS_RTAB_W,       // store: its half of the reward table
  MAPFX_PS_INFO_R,       // store a(q)
  MAPFX_PS_MAP_R,        // store a(q): window rows of map q & 1
  MAPFX_PS_IMG_W,        // store a(q): the staged records
  MAPFX_PS_IMG_R,        // store b(q)
  MAPFX_PS_EDGE_R,       // store b(q)
  MAPFX_PS_CODE_W,       // store b(q): reward codes, ring row q & 31
  MAPFX_PS_FOLD,         // store: a batch's ring rows and the reward table
  MAPFX_PS_COUNT
};
#define MAPFX_SPLIT_PROBE_CAP 1024        // records per wave: enough for T <= 130
#define MAPFX_SPLIT_PROBE_STAGE_FLAGS 64  // STAGE slot of the flag bytes (rows are slots 0 .. 63)
typedef struct mapfx_split_probe_cfg {
  int32_t block;            // the traced workgroup (blockIdx.x), -1: none
  int32_t delay_role;       // the wave that sleeps before its accesses at delay_site, -1: none
  int32_t delay_site;
  int32_t delay_len;        // sleeps of about 2000 cycles each, at most 64
  int32_t early_last_fold;  // != 0: the launch's last fold in interval T (negative control)
} mapfx_split_probe_cfg;
// rec[role][i]: word 0 = i | barriers passed << 16, word 1 = site | resource << 8 |
// kind << 12 | slot << 16 | (tag + 1) << 24 (tag: the step the data belongs to, -1 none)
typedef struct mapfx_split_probe_trace {
  uint32_t n[3];
  uint32_t barriers[3];
  uint32_t overflow;  // a wave had more than MAPFX_SPLIT_PROBE_CAP records
  uint32_t pad;
  uint32_t rec[3][MAPFX_SPLIT_PROBE_CAP][2];
} mapfx_split_probe_trace;
int mapfx_split_probe_config(const mapfx_split_probe_cfg* cfg);
int mapfx_split_probe_read(mapfx_split_probe_trace* out);
#endif
#ifdef __cplusplus
}

// ---- helpers shared by the five translation units: one definition each ----
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
