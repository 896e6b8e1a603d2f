// partial.hip -- MI355X (gfx950) batched MARL_PARTIAL_ENV step.
//
// The env the reference registers (MARL-curve-main/src/envs/__init__.py:60),
// envs/marl_partial.py (paths below relative to it):
//   step :165-310 -- moves against the PRE-step occupancy (obstacle passable while
//     occupied, :508-512), move / stay / stay-at-goal / env-collision rewards, goal
//     flags, episode limit, BFS-distance "closer" reward (:213-220), node / edge
//     collisions, completion bonus gamma^-(limit - t) (:289-299), fp64 sum in agent
//     order;
//   get_obs :312-375 -- w x w obstacle / agents planes + K nearest agents x 13
//     features (stable sort by L2 distance, self first, -1 padding), float32;
//   get_state :377-387, avail :399-433;
//   goal distances :906-928 -- A* path lengths == BFS levels (bit-parallel BFS).
//
// Layout: one wavefront holds EPW envs (L = pow2ceil(N) lanes per env, lane =
// agent); an env's padded cell map (c = count + 1 - obstacle, c == 0 blocked /
// border) and its dep map (bit 7: obstacle, bits 0-6: the occupant's move) live in
// LDS for the launch; state round-trips HBM between calls (partial_rollout_kernel: T steps
// of one launch, the state in registers and the maps in LDS in between).  N > 64 or a side > 256
// (the reference's larger maps and agent counts) take partial_wg_kernel: one
// workgroup per env, the agents' cells in an LDS hash table, the map in HBM.  Every fp64 value is
// computed in the reference's operation order; the completion bonus comes from a host-libm
// LUT (float ** int), sqrt(int) from the device's correctly rounded fp64 sqrt once
// mapfx_partial_create has checked it against host libm on every argument the launch can
// use (else from a host-libm LUT too).
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <memory>
#include <new>
#include <type_traits>

#include "internal.h"
#include "mapfx.h"
#include "mapfx_partial.h"


#ifdef PARTIAL_STAMPS
// Diagnostic build only (never the shipped library): s_memtime stamps of partial_kernel's
// phases, block 0 / lane 0, read back with mapfx_partial_debug_stamps().  The stamps stay
// in registers until the end (PST_FLUSH): a store per stamp would make the kernel's
// waits on the vector-memory counter wait for it too.
__device__ unsigned long long g_pstamps[16];
// every wave's s_memrealtime (100 MHz, one clock for the whole device) at stamps 0, 1,
// 8, 10, 11, 13: where the launch's tail comes from
constexpr int PBLK_MAX = 8192, PBLK_N = 6;
__device__ unsigned int g_pblk[PBLK_MAX * PBLK_N];
__device__ __forceinline__ int pblk_slot(int k) {
  return k == 0 ? 0 : k == 1 ? 1 : k == 8 ? 2 : k == 10 ? 3 : k == 11 ? 4 : k == 13 ? 5 : -1;
}
#define PST_DECL uint32_t pst_[14], pbt_[PBLK_N];
#define PST(k)                                                                       \
  do {                                                                               \
    __builtin_amdgcn_sched_barrier(0);                                               \
    unsigned long long t_;                                                           \
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_)::"memory");     \
    uint32_t v_;                                                                     \
    asm volatile("v_mov_b32 %0, %1" : "=v"(v_) : "s"((uint32_t)t_));                 \
    if (pblk_slot(k) >= 0) {                                                         \
      unsigned long long r_;                                                         \
      asm volatile("s_memrealtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(r_)::"memory"); \
      uint32_t w_;                                                                   \
      asm volatile("v_mov_b32 %0, %1" : "=v"(w_) : "s"((uint32_t)r_));               \
      pbt_[pblk_slot(k) < 0 ? 0 : pblk_slot(k)] = w_;                                \
    }                                                                                \
    __builtin_amdgcn_sched_barrier(0);                                               \
    pst_[(k)] = v_;                                                                  \
  } while (0)
#define PST_FLUSH()                                                                  \
  do {                                                                               \
    if (blockIdx.x == 0 && threadIdx.x == 0)                                         \
      for (int k_ = 0; k_ < 14; ++k_) g_pstamps[k_] = pst_[k_];                      \
    if (lane64 == 0 && gw < PBLK_MAX)                                                \
      for (int k_ = 0; k_ < PBLK_N; ++k_) g_pblk[gw * PBLK_N + k_] = pbt_[k_];         \
  } while (0)
extern "C" int mapfx_partial_debug_stamps(unsigned long long* host_out) {
  return hipMemcpyFromSymbol(host_out, HIP_SYMBOL(g_pstamps), sizeof(unsigned long long) * 16) ==
                 hipSuccess ? 0 : -1;
}
// n_blocks x 6 realtime stamps (diagnostic build)
extern "C" int mapfx_partial_debug_blocks(unsigned int* host_out, int n_blocks) {
  if (n_blocks < 0 || n_blocks > PBLK_MAX) return -1;
  return hipMemcpyFromSymbol(host_out, HIP_SYMBOL(g_pblk), sizeof(unsigned int) * PBLK_N * n_blocks) ==
                 hipSuccess ? 0 : -1;
}
#else
#define PST_DECL
#define PST(k) \
  do {         \
  } while (0)
#define PST_FLUSH() \
  do {              \
  } while (0)
#endif

namespace {

constexpr int NF = 13;   // KNN features per agent (:81)
constexpr int FR = 12;   // per-agent feature row in LDS (all but the pairwise distance)
constexpr int BONUS_EXTRA = 65536;  // completion-bonus LUT entries past the episode limit
constexpr int PARTIAL_MAX_WPB = 4;  // partial_kernel: waves per block (g.wpb <= this)

struct PGeo {
  int H, W, N, E;
  int L, lshift, EPW;
  int P, pl, pitch, rows, wpr;       // padded LDS map
  int bits_words, map_shared;
  long long map_stride;
  int map_env_bytes, bits_env_bytes, feat_env_bytes, pos_env_bytes, rew_env_bytes, stage_env_bytes, stage_lanes;
  int off_map, off_dep, off_bits, off_feat, off_pos, off_rew, off_stage, lds;  // off_stage < 0: none
  int off_sqrt;                      // float32 sqrt(0 .. sq_max) per wave (fast path), < 0: none
  int win, K, D, limit, hw;          // window, knn, obs dim, episode limit, H*W
  double move_rew, stay_rew, stay_goal_rew, nc_rew, ec_rew, env_rew;
  int sq_max, bonus_len;             // LUT sizes
  int gd32;                          // goal-distance tables are int32 (H * W > 32767)
  int gd8;                           // ... u8 (H * W <= 255: 255 = -1), else int16
  int big;                           // workgroup-per-env path (N > 64 or H, W > 256), map in HBM
  int hs_log, wg_lds, huge_lds;      // its LDS hash size (log2), block LDS; huge-map BFS LDS
  uint32_t m_wpr;                    // ceil(2^32 / wpr): wi / wpr = umulhi(wi, m_wpr) below rows * wpr
  int wpb;                           // partial_kernel: waves per block (each with g.lds of LDS)
};

struct PArgs {
  int32_t* pos;
  const int32_t* goal;
  const int32_t* init_pos;
  int32_t* steps;
  uint8_t* at_goal;
  uint8_t* done;
  int32_t* goal_cost;
  uint8_t* node;
  int32_t* edge;
  int32_t* t;
  uint8_t* terminated;
  int32_t* total_coll;
  const uint8_t* bits;
  const void* gd;  // u8, int16 or int32 (g.gd8, g.gd32)
  int32_t* pdist;  // [E][N] goal distance of the current cell (carried), or NULL
  int16_t* pnbr;   // [E][N][4] goal distances of its 4 neighbours (carried with pdist), or NULL
  const void* actions;
  int act_dtype;
  int do_step;       // 0: observe only
  const uint8_t* reset_mask;  // reset pass: envs to reset (NULL = all); nullptr when not resetting
  int do_reset;
  double* reward;
  float* obs;
  float* state;
  uint8_t* avail;
  int32_t* err;
  const double* bonus_lut;  // (complete / gamma ** (limit - t)) * fac, t = 0 .. bonus_len-1
  // runner fusion (mapfx_partial_step_runner): observation rows go to obs_rows + e *
  // obs_env_stride (an EpisodeBatch time row) for the envs with obs_mask[e] != 0,
  // instead of the contiguous `obs`
  float* obs_rows;
  long long obs_env_stride;
  const uint8_t* obs_mask;
  // the runner's fused actions (mapfx_partial_step_runner; act_row NULL otherwise)
  mapfx_runner_acts ra;
};

// partial_rollout_kernel (mapfx_partial_rollout): T steps of one launch.  PArgs' reward /
// obs / state / avail point at slot 0 of the trajectory arrays; the kernel advances them.
struct RArgs {
  int T;
  int autoreset;
  int policy;           // actions from the on-device policy (PArgs.actions is then a dummy)
  int t0;
  uint64_t seed, eps_q;
  long long env_offset;
  int32_t* pos;         // [T][E][N][2], or NULL
  uint8_t* terminated;  // [T][E], or NULL
  int8_t* actions;      // [T][E][N] (policy mode), or NULL
};

// partial_runner_rollout_kernel (mapfx_runner_rollout) on top of RArgs: step k is runner
// step ts0 + k; the rows the post pass writes at ts + 1 move by these time strides (PArgs.ra
// holds their row-0 pointers, PArgs.obs_rows row ts0 + 1), none past max_t - 1
struct RRun {
  int ts0, max_t;
  long long obs_st, state_st, avail_st, filled_st;
  int32_t* stale_out;   // [E] 0 / -1: env on the last step's stale list (T >= 2), or NULL
};

// where env e's observation rows go ([N][D] floats), or nullptr when not written
// (partial_kernel: the caller has read obs_mask[e] with the launch's other loads)
template <bool ROWS = true>
__device__ __forceinline__ float* obs_env_nomask(const PArgs& a, int e, int D, int N) {
  if (ROWS && a.obs_rows) return a.obs_rows + (long long)e * a.obs_env_stride;
  return a.obs ? a.obs + (long long)e * N * D : nullptr;
}
__device__ __forceinline__ float* obs_env(const PArgs& a, int e, int D, int N) {
  if (a.obs_rows) return (a.obs_mask && !a.obs_mask[e]) ? nullptr : a.obs_rows + (long long)e * a.obs_env_stride;
  return a.obs ? a.obs + (long long)e * N * D : nullptr;
}

// The step's action of agent `ag` of env `env` (oa = env * N + ag).  The runner's fused
// form (a.ra.act_row): row act_row[env] of the MAC's output, recorded into the
// EpisodeBatch's actions / actions_onehot rows at ts (parallel_runner.py:104-110 and the
// OneHot preprocess); an env outside bs stays (it has terminated: nothing of it is
// recorded again).  Values outside 0..4 come back as -1 (the env is then skipped, :174).
__device__ inline int step_action(const PArgs& a, int env, int ag, long long oa) {
  if (!a.ra.act_row) return load_action(a.actions, a.act_dtype, oa);
  const int row = a.ra.act_row[env];
  if (row < 0) return 4;
  const long long i = (long long)row * a.ra.act_row_stride + ag;
  const long long v = a.act_dtype == MAPFX_I8 ? (long long)((const int8_t*)a.actions)[i]
                      : a.act_dtype == MAPFX_I32 ? (long long)((const int32_t*)a.actions)[i]
                                                 : ((const int64_t*)a.actions)[i];
  if (a.ra.ep_actions)
    a.ra.ep_actions[(long long)env * a.ra.ep_actions_sb + (long long)a.ra.ts * a.ra.ep_actions_st + ag] = v;
  if (a.ra.ep_onehot) {
    float* oh = a.ra.ep_onehot + (long long)env * a.ra.ep_onehot_sb + (long long)a.ra.ts * a.ra.ep_onehot_st +
                (long long)ag * 5;
#pragma unroll
    for (int k = 0; k < 5; ++k) oh[k] = v == k ? 1.0f : 0.0f;
  }
  return (v < 0 || v > 4) ? -1 : (int)v;
}

// sqrt(n) of a non-negative integer n <= sq_max in fp64 (math.sqrt of the reference's
// squared distances): the device's correctly rounded sqrt, which mapfx_partial_create
// checks bit for bit against host libm on all of 0 .. sq_max (it refuses the
// configuration otherwise).  Computed, not loaded: a table load here would make every
// later wait on the vector-memory counter also wait for the loads issued before it.
__device__ __forceinline__ double isqrt_f64(int n) { return sqrt((double)n); }

// the action (int64 as (lo, hi), int8 / int32 sign-extended into hi): 0..4, or -1 for
// any value outside 0..4 (the env is then skipped, :174)
__device__ __forceinline__ int act_decode(int lo, int hi) { return ((uint32_t)lo <= 4u && hi == 0) ? lo : -1; }
// the action as the int64 the EpisodeBatch records
__device__ __forceinline__ long long act_value(int lo, int hi) {
  return (long long)(((uint64_t)(uint32_t)hi << 32) | (uint32_t)lo);
}

// Cross-lane sums inside an env's L-lane group without the LDS pipeline: DPP moves
// within 16-lane rows (L <= 16: an env's lanes never leave their row), else shuffles.
template <int CTRL>
__device__ __forceinline__ int dpp_mov(int x) {
  return __builtin_amdgcn_update_dpp(0, x, CTRL, 0xF, 0xF, false);
}
__device__ __forceinline__ int group_sum(int x, int L) {
  if (L == 16) {  // row_ror 8, 4, 2, 1
    x += dpp_mov<0x128>(x);
    x += dpp_mov<0x124>(x);
    x += dpp_mov<0x122>(x);
    return x + dpp_mov<0x121>(x);
  }
  if (L == 8) {  // quad_perm [1,0,3,2], [2,3,0,1], row_half_mirror
    x += dpp_mov<0xB1>(x);
    x += dpp_mov<0x4E>(x);
    return x + dpp_mov<0x141>(x);
  }
  if (L == 4) {
    x += dpp_mov<0xB1>(x);
    return x + dpp_mov<0x4E>(x);
  }
  if (L == 2) return x + dpp_mov<0xB1>(x);
  if (L == 1) return x;
  for (int o = 1; o < L; o <<= 1) x += __shfl_xor(x, o);
  return x;
}
// `sum(rewards)` (:310): the naive left fold 0.0 + r[0] + r[1] + ... + r[N-1] in agent
// order, valid in each env's agent-0 lane; r[k] arrives by a DPP row shift (lane i reads
// lane i + k of its row), so L <= 16 (callers fold through LDS otherwise)
template <int K>
__device__ __forceinline__ double row_shl_f64(double v) {
  const unsigned long long b = (unsigned long long)__double_as_longlong(v);
  const int lo = dpp_mov<0x100 + K>((int)(uint32_t)b);
  const int hi = dpp_mov<0x100 + K>((int)(uint32_t)(b >> 32));
  return __longlong_as_double((long long)(((unsigned long long)(uint32_t)hi << 32) | (uint32_t)lo));
}
template <int K>
__device__ __forceinline__ void fold_from(double& R, double x, int N) {
  if constexpr (K < 16) {
    if (K < N) R = R + row_shl_f64<K>(x);
    fold_from<K + 1>(R, x, N);
  }
}
// The same fold over a lane group of LG lanes known at compile time: every lane of the
// group past the env's N agents holds 0.0, and R is never -0.0 (it starts as 0.0 + r[0],
// and in round-to-nearest a sum is -0.0 only when both terms are), so R + 0.0 == R
// exactly and all LG - 1 shifts are folded with no per-term test of N (which cost a
// branch per term)
template <int K, int LG>
__device__ __forceinline__ void fold_all(double& R, double x) {
  if constexpr (K < LG) {
    R = R + row_shl_f64<K>(x);
    fold_all<K + 1, LG>(R, x);
  }
}
// edge collisions against every other lane of a 16-lane row (lane i sees lane (i + k) % 16
// for k = 1..15; lanes past N hold an unmoved cell and never match a moving agent)
template <int K>
__device__ __forceinline__ void dpp_edge_scan(int cur, int nc, int& e) {
  if constexpr (K < 16) {
    const int oj = dpp_mov<0x120 + K>(cur), nj = dpp_mov<0x120 + K>(nc);
    e += (oj == nc) & (nj == cur);
    dpp_edge_scan<K + 1>(cur, nc, e);
  }
}
// LG: the lane group when known at compile time (lanes past N must then hold 0.0), else 0
template <int LG>
__device__ __forceinline__ double row_fold(double x, int N) {
  double R = 0.0 + x;
  if constexpr (LG > 0 && LG <= 16) fold_all<1, LG>(R, x);
  else fold_from<1>(R, x, N);
  return R;
}

// goal distance of neighbour `act` (0 up, 1 down, 2 left, 3 right) from the carried
// pnbr entry (4 x int16 as two words)
__device__ __forceinline__ int nbr_dist(uint2 nb, int act) {
  const uint32_t w = act < 2 ? nb.x : nb.y;
  return (int)(int16_t)(uint16_t)((act & 1) ? (w >> 16) : (w & 0xFFFFu));
}

// entry i of a goal table: u8 while H * W <= 255 (a path is shorter than H * W cells;
// 255 stands for -1, obstacle / unreachable), int16 up to 32767 cells, else int32
__device__ __forceinline__ int gd_entry(const PGeo& g, const void* gd, long long i) {
  if (g.gd8) {
    const int v = ((const uint8_t*)gd)[i];
    return v == 255 ? -1 : v;
  }
  return g.gd32 ? ((const int32_t*)gd)[i] : (int)((const int16_t*)gd)[i];
}
// goal distance of cell `cell` in agent `oa`'s table
__device__ __forceinline__ int goal_dist_at(const PGeo& g, const void* gd, long long oa, int cell) {
  return gd_entry(g, gd, oa * g.hw + cell);
}
// the same with the table width known at compile time (GDE bytes: 1 u8, 2 int16; 0: run
// time): a single load with no branch around it
template <int GDE>
__device__ __forceinline__ int gd_entry_t(const PGeo& g, const void* gd, long long i) {
  if constexpr (GDE == 1) {
    const int v = ((const uint8_t*)gd)[i];
    return v == 255 ? -1 : v;
  } else if constexpr (GDE == 2) {
    return ((const int16_t*)gd)[i];
  } else {
    return gd_entry(g, gd, i);
  }
}

// The step's goal-path distances (:227-233) with the current cell's distance carried in
// the state (mapfx_partial_state.pdist, the reference's _new_pdist of the last step):
// opd is that value, npd = opd unless the agent moved, when it is the table entry of the
// target cell -- looked up speculatively as soon as the position and action are loaded
// (the lookup's latency then overlaps the map build).  Every non-step pass (reset,
// observe: positions may have been rewritten, e.g. by output mode's repair) refreshes
// the carried value from the table; PD_NONE (a state never reset) falls back to it too.
constexpr int PD_NONE = (int)0x80000000;

// The move target of action `act` from (r, c) when it lies on the grid (-1 otherwise):
// the cell whose distance a moving agent's npd is.
__device__ __forceinline__ int move_target(const PGeo& g, int r, int c, int act) {
  if (act < 0 || act > 3) return -1;
  const int tr = r + (act == 0 ? -1 : act == 1 ? 1 : 0);
  const int tc = c + (act == 2 ? -1 : act == 3 ? 1 : 0);
  return (tr < 0 || tr >= g.H || tc < 0 || tc >= g.W) ? -1 : tr * g.W + tc;
}

// ---------------------------------------------------------------------------
// BFS distance tables: one wave per (env, agent), lane r holds row r of the grid
// as a 64-bit mask; each level expands the frontier by shifts (same row) and
// shuffles (rows r-1, r+1).  Distances go to LDS then out, row-major int16.
// ---------------------------------------------------------------------------
template <typename DT>
__global__ void __launch_bounds__(64) partial_bfs_kernel(PGeo g, const uint8_t* bits,
                                                         const int32_t* goal, const uint8_t* mask,
                                                         DT* gd) {
  __shared__ int16_t dist[64 * 64];
  const int pair = blockIdx.x;  // env * N + agent
  const int env = pair / g.N;
  if (mask && !mask[env]) return;  // uniform per block
  const int r = threadIdx.x;
  const int H = g.H, W = g.W;
  const uint64_t wmask = W == 64 ? ~0ull : ((1ull << W) - 1ull);
  // free cells of row r
  uint64_t freem = 0;
  if (r < H) {
    const uint8_t* b = bits + (g.map_shared ? 0 : (long long)env * g.map_stride);
    for (int c = 0; c < W; ++c) {
      const int idx = r * W + c;
      if (!((b[idx >> 3] >> (idx & 7)) & 1)) freem |= 1ull << c;
    }
  }
  for (int i = r; i < H * W; i += 64) dist[i] = -1;
  wave_fence();
  const int gr = goal[2 * pair], gc = goal[2 * pair + 1];
  uint64_t front = (r == gr && ((freem >> gc) & 1)) ? (1ull << gc) : 0ull;
  uint64_t seen = front;
  if (front) dist[r * W + gc] = 0;
  int level = 0;
  while (__ballot(front != 0)) {
    ++level;
    const uint64_t up = __shfl_up(front, 1);    // row r-1
    const uint64_t dn = __shfl_down(front, 1);  // row r+1
    uint64_t nxt = (front << 1) | (front >> 1);
    if (r > 0) nxt |= up;
    if (r < 63) nxt |= dn;
    nxt &= freem & wmask & ~seen;
    if (r >= H) nxt = 0;
    seen |= nxt;
    for (uint64_t m = nxt; m; m &= m - 1) dist[r * W + __builtin_ctzll(m)] = (int16_t)level;
    front = nxt;
  }
  wave_fence();
  DT* out = gd + (long long)pair * g.hw;
  for (int i = r; i < g.hw; i += 64) out[i] = (DT)dist[i];
}

// Maps wider or taller than 64 (up to 256 x 256): one 256-thread workgroup per
// (env, agent); thread r holds row r as four 64-bit masks, the frontier rows are
// exchanged through LDS (double-buffered, one barrier per level), distances go
// straight to the table in global memory (its cells were set to -1 first).
constexpr int BIGW = 4;  // 64-bit words per row: W <= 256
template <typename DT>
__global__ void __launch_bounds__(256) partial_bfs_big_kernel(PGeo g, const uint8_t* bits,
                                                              const int32_t* goal, const uint8_t* mask,
                                                              DT* gd) {
  __shared__ uint64_t front[2][256][BIGW];
  const int pair = blockIdx.x;  // env * N + agent
  const int env = pair / g.N;
  if (mask && !mask[env]) return;  // uniform per block
  const int r = threadIdx.x;
  const int H = g.H, W = g.W;
  DT* out = gd + (long long)pair * g.hw;
  uint64_t freem[BIGW], seen[BIGW], cur[BIGW];
#pragma unroll
  for (int k = 0; k < BIGW; ++k) freem[k] = seen[k] = cur[k] = 0;
  if (r < H) {
    const uint8_t* b = bits + (g.map_shared ? 0 : (long long)env * g.map_stride);
    for (int c = 0; c < W; ++c) {
      const int idx = r * W + c;
      if (!((b[idx >> 3] >> (idx & 7)) & 1)) freem[c >> 6] |= 1ull << (c & 63);
    }
    for (int c = 0; c < W; ++c) out[r * W + c] = -1;
  }
  const int gr = goal[2 * pair], gc = goal[2 * pair + 1];
  if (r == gr && ((freem[gc >> 6] >> (gc & 63)) & 1)) {
    cur[gc >> 6] = 1ull << (gc & 63);
    seen[gc >> 6] = cur[gc >> 6];
    out[r * W + gc] = 0;
  }
#pragma unroll
  for (int k = 0; k < BIGW; ++k) front[0][r][k] = cur[k];
  __syncthreads();
  int level = 0, buf = 0;
  bool any = true;
  while (any) {
    ++level;
    uint64_t nxt[BIGW];
#pragma unroll
    for (int k = 0; k < BIGW; ++k) {
      // same row: cells c-1 / c+1 (carries across the 64-bit words)
      const uint64_t lft = (cur[k] << 1) | (k > 0 ? cur[k - 1] >> 63 : 0ull);
      const uint64_t rgt = (cur[k] >> 1) | (k + 1 < BIGW ? cur[k + 1] << 63 : 0ull);
      const uint64_t up = r > 0 ? front[buf][r - 1][k] : 0ull;
      const uint64_t dn = r + 1 < 256 ? front[buf][r + 1][k] : 0ull;
      nxt[k] = (lft | rgt | up | dn) & freem[k] & ~seen[k];
    }
    if (r >= H) {
#pragma unroll
      for (int k = 0; k < BIGW; ++k) nxt[k] = 0;
    }
    bool mine = false;
#pragma unroll
    for (int k = 0; k < BIGW; ++k) {
      seen[k] |= nxt[k];
      cur[k] = nxt[k];
      front[buf ^ 1][r][k] = nxt[k];
      mine |= nxt[k] != 0;
      for (uint64_t m = nxt[k]; m; m &= m - 1) out[r * W + 64 * k + __builtin_ctzll(m)] = (DT)level;
    }
    buf ^= 1;
    any = __syncthreads_or(mine ? 1 : 0) != 0;
  }
}

// Maps larger than 256 on a side (the reference ships brc202d 481 x 530, orz900d
// 656 x 1491, w_woundedcoast 578 x 642, ...): one 512-thread workgroup per (env,
// agent), thread t owns rows t and t + 512 (H <= 1024), each row as up to 24 64-bit
// words (W <= 1536).  The frontier rows live in LDS (H x words x 8 bytes: 126 KB for
// orz900d); every thread keeps its rows' "free and not yet reached" masks and the
// next frontier in registers, so a level is one LDS read phase, a barrier, one
// write phase and the termination test.  Grid graphs are bipartite and unweighted:
// level-synchronous expansion gives exactly the A* / BFS path lengths (:906-928).
constexpr int HUGE_WORDS = 24;
constexpr int HUGE_THREADS = 512;
template <typename DT>
__global__ void __launch_bounds__(HUGE_THREADS) partial_bfs_huge_kernel(PGeo g, const uint8_t* bits,
                                                                        const int32_t* goal,
                                                                        const uint8_t* mask, DT* gd) {
  extern __shared__ __align__(16) unsigned char lds[];
  uint64_t* front = (uint64_t*)lds;  // [H][WW]
  const int pair = blockIdx.x;       // env * N + agent
  const int env = pair / g.N;
  if (mask && !mask[env]) return;    // uniform per block
  const int tid = threadIdx.x;
  const int H = g.H, W = g.W, WW = (W + 63) >> 6;
  DT* out = gd + (long long)pair * g.hw;
  const uint64_t* b64 = (const uint64_t*)(bits + (g.map_shared ? 0 : (long long)env * g.map_stride));
  const long long nb64 = (g.map_stride + 7) / 8;  // whole u64 words of one env's bitmap
  for (int i = tid; i < g.hw; i += HUGE_THREADS) out[i] = (DT)-1;
  for (int i = tid; i < H * WW; i += HUGE_THREADS) front[i] = 0ull;
  uint64_t allow[2][HUGE_WORDS];
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int r = tid + j * HUGE_THREADS;
#pragma unroll
    for (int k = 0; k < HUGE_WORDS; ++k) {
      allow[j][k] = 0ull;
      if (r < H && k < WW) {  // bits r*W + 64k .. of the bitmap, 1 = obstacle
        const long long p = (long long)r * W + 64 * k;
        const long long wi = p >> 6;
        const int sh = (int)(p & 63);
        const uint64_t lo = b64[wi];
        const uint64_t hi = (sh && wi + 1 < nb64) ? b64[wi + 1] : 0ull;
        const uint64_t word = sh ? (lo >> sh) | (hi << (64 - sh)) : lo;
        const int nc = min(64, W - 64 * k);
        const uint64_t cols = nc == 64 ? ~0ull : ((1ull << nc) - 1ull);
        allow[j][k] = ~word & cols;
      }
    }
  }
  __syncthreads();  // the -1 fill and the zeroed frontier come first
  const int gr = goal[2 * pair], gc = goal[2 * pair + 1];
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    if (tid + j * HUGE_THREADS == gr) {
#pragma unroll
      for (int k = 0; k < HUGE_WORDS; ++k) {
        if (k == (gc >> 6) && ((allow[j][k] >> (gc & 63)) & 1ull)) {
          allow[j][k] &= ~(1ull << (gc & 63));
          front[gr * WW + k] = 1ull << (gc & 63);
          out[gr * W + gc] = (DT)0;
        }
      }
    }
  }
  __syncthreads();
  int level = 0;
  bool any = true;
  while (any) {
    ++level;
    uint64_t nxt[2][HUGE_WORDS];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int r = tid + j * HUGE_THREADS;
#pragma unroll
      for (int k = 0; k < HUGE_WORDS; ++k) {
        nxt[j][k] = 0ull;
        if (r < H && k < WW) {
          const uint64_t* fr = front + r * WW;
          const uint64_t cur = fr[k];
          const uint64_t lft = (cur << 1) | (k > 0 ? fr[k - 1] >> 63 : 0ull);
          const uint64_t rgt = (cur >> 1) | (k + 1 < WW ? fr[k + 1] << 63 : 0ull);
          const uint64_t up = r > 0 ? fr[k - WW] : 0ull;
          const uint64_t dn = r + 1 < H ? fr[k + WW] : 0ull;
          nxt[j][k] = (lft | rgt | up | dn) & allow[j][k];
        }
      }
    }
    __syncthreads();  // every read of this level's frontier is done
    bool mine = false;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int r = tid + j * HUGE_THREADS;
#pragma unroll
      for (int k = 0; k < HUGE_WORDS; ++k) {
        if (r < H && k < WW) {
          front[r * WW + k] = nxt[j][k];
          allow[j][k] &= ~nxt[j][k];
          mine |= nxt[j][k] != 0ull;
          for (uint64_t m = nxt[j][k]; m; m &= m - 1) out[r * W + 64 * k + __builtin_ctzll(m)] = (DT)level;
        }
      }
    }
    any = __syncthreads_or(mine ? 1 : 0) != 0;
  }
}

// ---------------------------------------------------------------------------
// Workgroup-per-env step for what the wave kernel cannot hold: N > 64 agents or a
// side > 256 cells (SURVEY.md §8(f) F1 at the reference's full range).  One
// 256-thread workgroup per env, thread t owns agents t, t + 256, ... (APL <= 4:
// N <= 1024).  No dense map in LDS: the obstacle bitmap is read from HBM and the
// agents' cells live in an LDS hash table (open addressing, keys = row * W + col,
// >= 4 slots per agent) carrying per cell the PRE-step count, the POST-step count
// and the move of a single pre-step occupant (the edge test's fast case), rebuilt
// every launch.  Same operation order as partial_kernel for every fp64 value.
// ---------------------------------------------------------------------------
constexpr int WG_THREADS = 256;
constexpr uint32_t HEMPTY = 0xFFFFFFFFu;
constexpr uint32_t HPRE = 1u, HPOST = 1u << 11, HDEP_SH = 22;  // val = pre | post << 11 | dep << 22

__device__ __forceinline__ uint32_t hslot0(uint32_t key, int hs_log) {
  return (key * 0x9E3779B1u) >> (32 - hs_log);
}
// the slot of `key`, inserted if absent
__device__ __forceinline__ int hinsert(uint32_t* keys, int hs_log, uint32_t key) {
  const uint32_t msk = (1u << hs_log) - 1u;
  uint32_t s = hslot0(key, hs_log);
  while (true) {
    const uint32_t k = keys[s];
    if (k == key) return (int)s;
    if (k == HEMPTY) {
      const uint32_t old = atomicCAS(&keys[s], HEMPTY, key);
      if (old == HEMPTY || old == key) return (int)s;
    }
    s = (s + 1) & msk;
  }
}
// the value of `key` (0 when absent); all insertions done
__device__ __forceinline__ uint32_t hlookup(const uint32_t* keys, const uint32_t* vals, int hs_log, uint32_t key) {
  const uint32_t msk = (1u << hs_log) - 1u;
  uint32_t s = hslot0(key, hs_log);
  while (true) {
    const uint32_t k = keys[s];
    if (k == key) return vals[s];
    if (k == HEMPTY) return 0u;
    s = (s + 1) & msk;
  }
}

template <int WIN, int APL>
__global__ void __launch_bounds__(WG_THREADS) partial_wg_kernel(PGeo g, PArgs a) {
  extern __shared__ __align__(16) unsigned char lds[];
  constexpr int H2 = WIN / 2, WW = WIN * WIN;
  const int tid = threadIdx.x, env = blockIdx.x, N = g.N, H = g.H, W = g.W;
  const int hs = 1 << g.hs_log;
  uint32_t* keys = (uint32_t*)lds;                    // [hs]
  uint32_t* vals = keys + hs;                         // [hs]
  int* oldL = (int*)(vals + hs);                      // [N] pre-step cell (edge scan)
  int* newL = oldL + N;                               // [N] post-step cell
  int2* posL = (int2*)(newL + N);                     // [N] post-step (row, col) (KNN)
  float* feat = (float*)(posL + N);                   // [N][FR]
  double* rewL = (double*)(((uintptr_t)(feat + N * FR) + 15) & ~(uintptr_t)15);  // [N]
  int* red = (int*)(rewL + N);                        // [8] block reductions
  const uint8_t* bm = a.bits + (g.map_shared ? 0 : (long long)env * g.map_stride);
  const auto obstacle = [&](int rr, int cc) {  // 1 outside the grid or on a static obstacle
    if (rr < 0 || rr >= H || cc < 0 || cc >= W) return 1u;
    const int idx = rr * W + cc;
    return (uint32_t)((bm[idx >> 3] >> (idx & 7)) & 1u);
  };

  int r[APL], c[APL], gr[APL], gc[APL], ir[APL], ic[APL], steps[APL], gcost[APL], edge[APL];
  int pd[APL];  // goal distance of the current cell (carried, see PD_NONE)
  bool has[APL], at_goal[APL], dn[APL];
  uint32_t node[APL];
  const bool reset_me = a.do_reset && (!a.reset_mask || a.reset_mask[env]);
  int tcur = a.t[env], total = a.total_coll[env];
  bool term = a.terminated[env] != 0;
  if (reset_me) {
    tcur = 0;
    term = false;
    total = 0;
  }
#pragma unroll
  for (int k = 0; k < APL; ++k) {
    const int ag = tid + k * WG_THREADS;
    has[k] = ag < N;
    r[k] = c[k] = gr[k] = gc[k] = ir[k] = ic[k] = steps[k] = edge[k] = 0;
    gcost[k] = -1;
    pd[k] = PD_NONE;
    at_goal[k] = dn[k] = false;
    node[k] = 0;
    if (has[k]) {
      const long long oa = (long long)env * N + ag;
      const int2 q = ((const int2*)a.goal)[oa], ip = ((const int2*)a.init_pos)[oa];
      gr[k] = q.x, gc[k] = q.y, ir[k] = ip.x, ic[k] = ip.y;
      if (reset_me) {  // :125-163
        r[k] = ir[k], c[k] = ic[k];
      } else {
        const int2 p = ((const int2*)a.pos)[oa];
        r[k] = p.x, c[k] = p.y;
        steps[k] = a.steps[oa];
        at_goal[k] = a.at_goal[oa] != 0;
        dn[k] = a.done[oa] != 0;
        gcost[k] = a.goal_cost[oa];
        node[k] = a.node[oa];
        edge[k] = a.edge[oa];
        if (a.pdist && a.do_step) pd[k] = a.pdist[oa];
      }
      if (pd[k] == PD_NONE) pd[k] = goal_dist_at(g, a.gd, oa, r[k] * W + c[k]);
    }
  }
  for (int i = tid; i < hs; i += WG_THREADS) {
    keys[i] = HEMPTY;
    vals[i] = 0u;
  }
  if (tid < 8) red[tid] = 0;
  __syncthreads();
  // pre-step counts (the move test reads the PRE-step occupancy, :508-512)
  int oslot[APL];
#pragma unroll
  for (int k = 0; k < APL; ++k) {
    oslot[k] = 0;
    if (has[k]) {
      oslot[k] = hinsert(keys, g.hs_log, (uint32_t)(r[k] * W + c[k]));
      atomicAdd(&vals[oslot[k]], HPRE);
    }
  }
  __syncthreads();

  // ---- step (:165-310) ----
  int act[APL];
  bool bad = false;
#pragma unroll
  for (int k = 0; k < APL; ++k) {
    act[k] = 4;
    if (a.do_step && has[k]) {
      act[k] = step_action(a, env, tid + k * WG_THREADS, (long long)env * N + tid + k * WG_THREADS);
      if (act[k] < 0 || act[k] > 4) bad = true;
    }
  }
  const bool skip = a.do_step && __syncthreads_or(bad ? 1 : 0) != 0;  // the reference asserts (:174)
  if (a.do_step && !skip) {
    ++tcur;  // :178
    double rew[APL];
    bool moved[APL];
    int pre[APL], nr[APL], ncol[APL];
    uint32_t dnew[APL];
#pragma unroll
    for (int k = 0; k < APL; ++k) {
      rew[k] = 0.0;  // rewards[i] = 0 (:183)
      moved[k] = false;
      pre[k] = 0;
      nr[k] = r[k], ncol[k] = c[k];
      if (has[k] && !dn[k]) {  // :193-211
        ++steps[k];
        bool envc = false;
        if (act[k] != 4) {
          const int tr = r[k] + (act[k] == 0 ? -1 : act[k] == 1 ? 1 : 0);
          const int tc = c[k] + (act[k] == 2 ? -1 : act[k] == 3 ? 1 : 0);
          const bool out = tr < 0 || tr >= H || tc < 0 || tc >= W;
          const int cnt = out ? 0 : (int)(hlookup(keys, vals, g.hs_log, (uint32_t)(tr * W + tc)) & 0x7FFu);
          if (out || (obstacle(tr, tc) && cnt == 0)) envc = true;  // obstacle nobody stands on
          else {
            nr[k] = tr, ncol[k] = tc;
            moved[k] = true;
            pre[k] = cnt;
          }
        }
        if (envc) rew[k] = rew[k] + g.env_rew;                          // :203
        if (act[k] != 4) rew[k] = rew[k] + g.move_rew;                  // :207
        else rew[k] = rew[k] + (at_goal[k] ? g.stay_goal_rew : g.stay_rew);  // :209-212
      }
    }
#pragma unroll
    for (int k = 0; k < APL; ++k) {
      if (!has[k]) continue;
      const int ag = tid + k * WG_THREADS;
      at_goal[k] = nr[k] == gr[k] && ncol[k] == gc[k];  // :214-219
      if (at_goal[k]) gcost[k] = tcur;
      if (tcur >= g.limit) {  // :221-225
        term = true;
        dn[k] = true;
      }
      const long long oa = (long long)env * N + ag;
      const int opd = pd[k];  // :227-233
      const int npd = moved[k] ? goal_dist_at(g, a.gd, oa, nr[k] * W + ncol[k]) : opd;
      rew[k] = rew[k] + (double)(opd - npd) / (double)g.limit;
      pd[k] = npd;
      // the single pre-step occupant's move (0..3, 7: stayed) and the post-step count
      atomicOr(&vals[oslot[k]], (moved[k] ? (uint32_t)act[k] : 7u) << HDEP_SH);
      const int ns = hinsert(keys, g.hs_log, (uint32_t)(nr[k] * W + ncol[k]));
      atomicAdd(&vals[ns], HPOST);
      oldL[ag] = r[k] * W + c[k];
      newL[ag] = nr[k] * W + ncol[k];
    }
    __syncthreads();
    // node / edge collisions (:708-727, :822-857); total += (sum(node) + sum(edge)) // 2 (:239)
    int esum = 0;
#pragma unroll
    for (int k = 0; k < APL; ++k) {
      dnew[k] = 0u;
      if (!has[k]) continue;
      const uint32_t v = hlookup(keys, vals, g.hs_log, (uint32_t)(nr[k] * W + ncol[k]));
      node[k] = ((v >> 11) & 0x7FFu) >= 2u ? 1u : 0u;
      edge[k] = 0;
      if (moved[k] && pre[k] > 0) {
        if (pre[k] == 1) {
          edge[k] = (int)((v >> HDEP_SH) & 7u) == (act[k] ^ 1) ? 1 : 0;
        } else {
          const int oc = r[k] * W + c[k], nc = nr[k] * W + ncol[k];
          for (int j = 0; j < N; ++j) edge[k] += (oldL[j] == nc) & (newL[j] == oc);
        }
      }
      esum += (int)node[k] + edge[k];
    }
    if (esum) atomicAdd(&red[0], esum);
    int nat = 0;
#pragma unroll
    for (int k = 0; k < APL; ++k) nat += (has[k] && at_goal[k]) ? 1 : 0;
    if (nat) atomicAdd(&red[1], nat);
    __syncthreads();
    total += red[0] / 2;
    const bool all_at = red[1] == N;  // :283-299
#pragma unroll
    for (int k = 0; k < APL; ++k) {
      if (!has[k]) continue;
      rew[k] = rew[k] + g.nc_rew * (double)node[k];  // :247
      rew[k] = rew[k] + g.ec_rew * (double)edge[k];  // :249
      if (all_at) {
        dn[k] = true;
        rew[k] = rew[k] + a.bonus_lut[min(tcur, g.bonus_len - 1)];
      }
      rewL[tid + k * WG_THREADS] = rew[k];
      r[k] = nr[k], c[k] = ncol[k];
    }
    if (all_at) term = true;
    __syncthreads();
    if (tid == 0) {  // sum(rewards): naive left fold in agent order (:310)
      double R = 0.0;
      for (int j = 0; j < N; ++j) R = R + rewL[j];
      if (a.reward) a.reward[env] = R;
    }
  } else if (a.do_step && tid == 0) {
    if (a.err) atomicCAS(a.err, 0, env + 1);
    if (a.reward) a.reward[env] = 0.0;
  }
  __syncthreads();
  // post-step occupancy: rebuild the table from the current cells (the step's post
  // counts hold it already; a reset / observe pass counts the positions here)
  if (!(a.do_step && !skip)) {
    for (int i = tid; i < hs; i += WG_THREADS) {
      keys[i] = HEMPTY;
      vals[i] = 0u;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < APL; ++k)
      if (has[k]) atomicAdd(&vals[hinsert(keys, g.hs_log, (uint32_t)(r[k] * W + c[k]))], HPOST);
  }
  // ---- observations of the current state (:312-391) ----
#pragma unroll
  for (int k = 0; k < APL; ++k) {
    if (!has[k]) continue;
    const int ag = tid + k * WG_THREADS;
    const int d0 = gr[k] - r[k], d1 = gc[k] - c[k];
    const double nrm = isqrt_f64(d0 * d0 + d1 * d1);   // :937
    const double ux = nrm == 0.0 ? 0.0 : (double)d0 / nrm;   // :938-941
    const double uy = nrm == 0.0 ? 0.0 : (double)d1 / nrm;
    float* fr = feat + ag * FR;
    fr[0] = (float)r[k]; fr[1] = (float)c[k]; fr[2] = (float)ir[k]; fr[3] = (float)ic[k];
    fr[4] = (float)gr[k]; fr[5] = (float)gc[k]; fr[6] = (float)ux; fr[7] = (float)uy;
    fr[8] = (float)nrm; fr[9] = (float)node[k]; fr[10] = (float)edge[k]; fr[11] = (float)steps[k];
    posL[ag] = make_int2(r[k], c[k]);
  }
  int gsum = 0;
#pragma unroll
  for (int k = 0; k < APL; ++k) gsum += has[k] ? gcost[k] : 0;
  if (tid == 0) red[2] = 0;
  __syncthreads();
  if (gsum) atomicAdd(&red[2], gsum);
  float* const env_obs = obs_env(a, env, g.D, N);
  // the c value of a cell: count + 1 - obstacle, 0 = outside / an obstacle nobody stands on
  const auto cval = [&](int rr, int cc) -> uint32_t {
    if (rr < 0 || rr >= H || cc < 0 || cc >= W) return 0u;
    const uint32_t cnt = (hlookup(keys, vals, g.hs_log, (uint32_t)(rr * W + cc)) >> 11) & 0x7FFu;
    return cnt + 1u - obstacle(rr, cc);
  };
#pragma unroll
  for (int k = 0; k < APL; ++k) {
    if (!has[k]) continue;
    const int ag = tid + k * WG_THREADS;
    if (env_obs) {
      float* o = env_obs + (long long)ag * g.D;
      if constexpr (WIN > 0) {  // window planes (:327-342): OOB / obstacle -> 1; agents -> count
        for (int y = 0; y < WIN; ++y)
          for (int x = 0; x < WIN; ++x) {
            const uint32_t cv = cval(r[k] + y - H2, c[k] + x - H2);
            o[y * WIN + x] = cv == 0 ? 1.0f : 0.0f;
            o[WW + y * WIN + x] = cv == 0 ? 0.0f : (float)(cv - 1u);
          }
      }
      // K nearest agents (:346-372): self first, then the k-1 nearest others by L2
      // distance (sorted() is stable: ties by agent index); rows past min(N, K) = -1
      float* kn = o + 2 * WW;
      const int K = g.K, km1 = min(N, K) - 1;
      for (int q = 0; q < 11; ++q) kn[q] = feat[ag * FR + q];
      kn[11] = (float)(H * W);  // distance to itself (:543-545)
      kn[12] = feat[ag * FR + 11];
      long long prev = -1;
      for (int sI = 1; sI <= km1; ++sI) {
        long long best = 0x7FFFFFFFFFFFFFFFll;
        for (int j = 0; j < N; ++j) {
          if (j == ag) continue;
          const int2 pj = posL[j];
          const int dr = r[k] - pj.x, dc = c[k] - pj.y;
          const long long key = (long long)(dr * dr + dc * dc) * 1024 + j;
          if (key > prev && key < best) best = key;
        }
        prev = best;
        const int j = (int)(best & 1023);
        const int sq = (int)(best >> 10);
        float* row = kn + sI * NF;
        for (int q = 0; q < 11; ++q) row[q] = feat[j * FR + q];
        row[11] = (float)isqrt_f64(sq);
        row[12] = feat[j * FR + 11];
      }
      for (int sI = km1 + 1; sI < K; ++sI)
        for (int q = 0; q < NF; ++q) kn[sI * NF + q] = -1.0f;
    }
    if (a.avail) {  // avail (:399-433): neighbour in bounds and not a free-standing obstacle
      uint32_t m = 16u;
      if (cval(r[k] - 1, c[k])) m |= 1u;
      if (cval(r[k] + 1, c[k])) m |= 2u;
      if (cval(r[k], c[k] - 1)) m |= 4u;
      if (cval(r[k], c[k] + 1)) m |= 8u;
      a.avail[(long long)env * N + ag] = (uint8_t)m;
    }
  }
  __syncthreads();
  if (tid == 0 && a.state) {  // state (:377-387): [total collisions, step count, sum(each goal cost)]
    a.state[3 * env + 0] = (float)total;
    a.state[3 * env + 1] = (float)tcur;
    a.state[3 * env + 2] = (float)red[2];
  }
  // ---- state write-back ----
#pragma unroll
  for (int k = 0; k < APL; ++k) {
    if (!has[k]) continue;
    const long long oa = (long long)env * N + tid + k * WG_THREADS;
    ((int2*)a.pos)[oa] = make_int2(r[k], c[k]);
    a.steps[oa] = steps[k];
    a.at_goal[oa] = at_goal[k] ? 1 : 0;
    a.done[oa] = dn[k] ? 1 : 0;
    a.goal_cost[oa] = gcost[k];
    a.node[oa] = (uint8_t)node[k];
    a.edge[oa] = edge[k];
    if (a.pdist) a.pdist[oa] = pd[k];
  }
  if (tid == 0) {
    a.t[env] = tcur;
    a.terminated[env] = term ? 1 : 0;
    a.total_coll[env] = total;
  }
}

// ---------------------------------------------------------------------------
// Step / observe / reset kernel (one launch = one env step or observation pass).
// ---------------------------------------------------------------------------
// KF / LF: K and lanes-per-env fixed at compile time (0: run-time generic path)
// A block is g.wpb independent waves (no barrier between them): bigger blocks let the
// dispatcher start the launch's waves sooner (one wave per block took ~1.4 us to have
// all 1024 waves of the bench shape running).
// GDE: goal-table entry bytes fixed at compile time (1 u8, 2 int16; 0: run time)
// RUN: the runner's fused actions / post pass and EpisodeBatch observation rows compiled
// in (false: the plain step, whose code then holds none of the runner's pointers: 2043
// -> 1747 VALU instructions)
// The runner's `bs` compaction for the next MAC call (runner.hip runner_compact_kernel's
// work) as the extra FIRST workgroup of the runner step's launch (mapfx_runner_acts
// cmp_*): A = cmp_alive (running before this step) is not written by this launch, so the
// compaction runs beside the env workgroups -- dispatched first, it is done long before
// them -- instead of as a launch after them.  Ascending indices of A, padded with the
// first; per-thread chunks (up to 32 flags held as a bit set between the count and the
// write pass, a 16-flag chunk read as one 16-byte load), a shuffle scan per wave and one
// barrier for the wave totals (blockDim = 64 * wpb, 64 .. 256 threads).
__device__ __forceinline__ void runner_compact_block(const mapfx_runner_acts& ra, unsigned char* lds) {
  const int nt = (int)blockDim.x, tid = (int)threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int nw = nt >> 6, B = ra.cmp_B;
  const int chunk = (B + nt - 1) / nt;
  const int lo = min(B, tid * chunk), hi = min(B, lo + chunk);
  const bool held = chunk <= 32;
  uint32_t bits = 0;  // flag b - lo (held chunks)
  int c = 0;
  if (held) {
    if (chunk == 16 && hi - lo == 16 && ((uintptr_t)(ra.cmp_alive + lo) & 15) == 0) {
      const uint4 w = *(const uint4*)(ra.cmp_alive + lo);
      const uint32_t ws4[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
      for (int i = 0; i < 4; ++i) {  // bit 7 of each byte: byte != 0
        const uint32_t nz = (((ws4[i] & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | ws4[i]) & 0x80808080u;
        const uint32_t m = nz >> 7;
        bits |= ((m | (m >> 7) | (m >> 14) | (m >> 21)) & 0xFu) << (4 * i);
      }
    } else {
      for (int b = lo; b < hi; ++b) bits |= (ra.cmp_alive[b] ? 1u : 0u) << (b - lo);
    }
    c = __popc(bits);
  } else {
    for (int b = lo; b < hi; ++b) c += ra.cmp_alive[b] ? 1 : 0;
  }
  int x = c;  // inclusive scan over the wave's lanes
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int y = __shfl_up(x, o);
    if (lane >= o) x += y;
  }
  int* ws = (int*)lds;
  if (lane == 63) ws[wv] = x;
  __syncthreads();
  int off = 0, total = 0;
  for (int i = 0; i < nw; ++i) {
    const int v = ws[i];
    off += i < wv ? v : 0;
    total += v;
  }
  int o = off + x - c;  // exclusive prefix of this thread's chunk
  for (int b = lo; b < hi; ++b) {
    const bool in = held ? ((bits >> (b - lo)) & 1u) != 0 : ra.cmp_alive[b] != 0;
    ra.cmp_bs_inv[b] = in ? o : -1;  // where the next MAC call puts env b's row
    if (in) ra.cmp_bs[o++] = b;
  }
  __syncthreads();  // bs[0] written
  const int64_t first = total > 0 ? ra.cmp_bs[0] : 0;
  for (int j = total + tid; j < B; j += nt) ra.cmp_bs[j] = first;
  if (tid == 0) {
    ra.cmp_counts[0] = total;  // len(bs) = the envs running before this step
    ra.cmp_counts[1] = total;  // = the envs running after the previous one
    ra.cmp_env_steps[0] += total;  // the envs this step steps (env_steps_this_run, :142)
    if (ra.cmp_counts_out) {  // possibly pinned host memory
      ra.cmp_counts_out[0] = total;
      ra.cmp_counts_out[1] = total;
    }
  }
}

// The on-device policy of mapfx_partial_rollout (mapfx_partial.h; mapfx/rng.py
// partial_policy_actions restates it): mapfx_action's own word u decides between its
// uniform draw ((u >> 32) < eps_q) and the descent of the agent's goal distances -- the
// lowest-numbered available neighbour of minimal distance when that is below the cell's
// own (pd), else stay.  avail: the PRE-step get_avail_actions mask; d0..d3: the goal
// distances of the neighbours up, down, left, right (any value where the bit is clear).
constexpr uint64_t PK_ENV = 0xD1B54A32D192ED03ull, PK_T = 0xABC98388FB8FAC03ull,
                   PK_AGENT = 0x8CB92BA72F3D8DD7ull;  // mapfx/rng.py K_ENV, K_T, K_AGENT
__device__ __forceinline__ int policy_action(const RArgs& ro, int env, int k, int ag, uint32_t avail, int pd,
                                             int d0, int d1, int d2, int d3) {
  const uint64_t u = splitmix64(ro.seed ^ ((uint64_t)(ro.env_offset + env) * PK_ENV) ^
                                ((uint64_t)(uint32_t)(ro.t0 + k) * PK_T) ^ ((uint64_t)(uint32_t)ag * PK_AGENT));
  if ((u >> 32) < ro.eps_q) return (int)(u % 5ull);
  int best = 0x7FFFFFFF, bm = 4;
  if ((avail & 1u) && d0 >= 0 && d0 < best) best = d0, bm = 0;
  if ((avail & 2u) && d1 >= 0 && d1 < best) best = d1, bm = 1;
  if ((avail & 4u) && d2 >= 0 && d2 < best) best = d2, bm = 2;
  if ((avail & 8u) && d3 >= 0 && d3 < best) best = d3, bm = 3;
  return (pd >= 0 && best < pd) ? bm : 4;
}

// MAPFX_POLICY_PIBT (mapfx_partial.h; mapfx/rng.py partial_policy_pibt_actions is the rule's
// definition): the env's agents are planned one at a time by its lane group, every lane of
// the wave in the loop until the wave's last group is through -- no LDS, no barrier.
//   per lane   dec / tgt / pact  decided, the cell it claims, its action: the claimed cells
//                                are exactly the decided agents' tgt (a failed push leaves
//                                the cell to the pushed agent, which stays on it)
//              lst               the candidates it has not tried: 3 bits each, move + 1, 0 ends
//              par / pcell       who pushed it and from where (the stack of the recursion:
//                                an agent is planned once, so one entry per lane holds it)
//   per group  ca                the agent being planned (the same value in the group's lanes)
// One pass looks at one candidate of `ca`: the lane broadcasts (move, cell, parent) in one
// word; two ballots masked to the group answer "claimed?" (decided lanes whose tgt is the
// cell) and give U (undecided lanes standing on it) -- the agents' cells are the `cur`
// registers.  A call (push) or a return changes ca; a return of true ends the whole chain.
// At most 6 passes per agent (5 candidates and the exhausted list), 2 N calls and returns.
// cur: the agent's index into the padded LDS map (one per cell), pitch: its row stride.
// the cell offset of list entry m1 (move + 1): -pitch, +pitch, -1, +1, and 0 for stay (5)
__device__ __forceinline__ int move_delta(int m1, int pitch) {
  const int mag = m1 <= 2 ? pitch : 1;
  return m1 == 5 ? 0 : (m1 & 1) ? -mag : mag;
}
__device__ __forceinline__ int pibt_action(const RArgs& ro, int N, int env, int k, int ag, bool has, int base,
                                           uint64_t envmask, uint32_t avail, int pd, int d0, int d1, int d2,
                                           int d3, int cur, int pitch) {
  const uint32_t t = (uint32_t)(ro.t0 + k);
  const uint64_t u = splitmix64(ro.seed ^ ((uint64_t)(ro.env_offset + env) * PK_ENV) ^ ((uint64_t)t * PK_T) ^
                                ((uint64_t)(uint32_t)ag * PK_AGENT));
  const bool explore = (u >> 32) < ro.eps_q;
  // both candidate lists up front (every lane at once): the sorted one by ranks -- key
  // d * 8 + m, stay as pd * 8 + 4, keys of moves that are not ok left out
  constexpr int NOKEY = 0x7FFFFFFF;
  uint32_t sorted = 5u, expl = 5u;  // pd < 0: stay alone
  if (pd >= 0) {
    const int key[5] = {(avail & 1u) && d0 >= 0 ? d0 * 8 : NOKEY, (avail & 2u) && d1 >= 0 ? d1 * 8 + 1 : NOKEY,
                        (avail & 4u) && d2 >= 0 ? d2 * 8 + 2 : NOKEY, (avail & 8u) && d3 >= 0 ? d3 * 8 + 3 : NOKEY,
                        pd * 8 + 4};
    sorted = 0u;
#pragma unroll
    for (int i = 0; i < 5; ++i) {
      int rank = 0;
#pragma unroll
      for (int j = 0; j < 5; ++j) rank += key[j] < key[i] ? 1 : 0;
      if (key[i] != NOKEY) sorted |= (uint32_t)(i + 1) << (3 * rank);
    }
    const int m = (int)(u % 5ull);
    const uint32_t okm = (key[0] != NOKEY ? 1u : 0u) | (key[1] != NOKEY ? 2u : 0u) | (key[2] != NOKEY ? 4u : 0u) |
                         (key[3] != NOKEY ? 8u : 0u);
    if ((okm >> m) & 1u) expl = (uint32_t)(m + 1) | (5u << 3);  // (m == 4: bit 4 is clear)
  }
  const uint32_t tm = t % (uint32_t)N;  // (a - t) mod N ascending: a = tm, tm + 1, .., N - 1, 0, .., tm - 1
  bool dec = !has;
  int tgt = -1, pact = 4, par = -1, pcell = -2;
  uint32_t lst = 0u;
  // the next agent planned at top level: undecided, off its goal first, then in rotated order
  const auto select = [&]() {
    const uint64_t und = (__ballot(has && !dec) & envmask) >> base;
    const uint64_t off = (__ballot(has && !dec && pd != 0) & envmask) >> base;
    const uint64_t c = off ? off : und;
    const uint64_t hi = (c >> tm) << tm;
    return c ? __ffsll((unsigned long long)(hi ? hi : c)) - 1 : -1;
  };
  int ca = select();
  if (ag == ca) lst = explore ? expl : sorted;
  while (__ballot(ca >= 0)) {
    const bool on = ca >= 0, me = on && ag == ca;
    const int m1 = (int)(lst & 7u);
    const int v = m1 == 0 ? -1 : cur + move_delta(m1, pitch);
    const uint32_t word = ((uint32_t)(v + 1) << 11) | (m1 != 0 && v == pcell ? 1024u : 0u) |
                          ((uint32_t)(par + 1) << 3) | (uint32_t)m1;
    const uint32_t wb = (uint32_t)__shfl((int)word, base + (on ? ca : 0));
    const int mb = (int)(wb & 7u), parb = (int)((wb >> 3) & 127u) - 1, vb = (int)(wb >> 11) - 1;
    const uint64_t cm = __ballot(on && has && dec && tgt == vb) & envmask;
    const uint64_t um = __ballot(on && has && !dec && !me && mb != 5 && cur == vb) & envmask;
    // (selects, no branches: the groups of a wave are at different places of their plans)
    const bool exh = mb == 0;  // the list is exhausted: stay, false to the parent (or the chain ends)
    const bool skip = !exh && ((cm != 0) | ((wb & 1024u) != 0) | (__popcll(um) >= 2));
    const bool push = !exh && !skip && um != 0;  // the cell's occupant is planned next
    const int child = __ffsll((unsigned long long)um) - 1 - base;  // (meaningful with push)
    if (me && !skip) dec = true, pact = exh ? 4 : mb - 1, tgt = exh ? cur : vb;
    if (me && !exh) lst >>= 3;  // (after a claim too: the next one, should the push fail)
    if (push && ag == child) par = ca, pcell = cur - move_delta(mb, pitch), lst = sorted;
    int nca = exh ? parb : skip ? ca : push ? child : -1;  // (-1: true, all the way up)
    const int top = select();
    if (on && nca < 0) {
      nca = top;
      if (ag == top) lst = explore ? expl : sorted;
    }
    ca = on ? nca : -1;
  }
  return pact;
}

// The body of partial_kernel (ROLL 0: one pass, exactly the step / observe / reset kernel)
// and of partial_rollout_kernel (ROLL 1: T steps with the observation rows, ROLL 2: T steps
// without them -- no feature rows, no K-nearest rows, no window planes, no staging).  The
// rollout keeps the agent state in registers and both maps in LDS between its steps, takes
// a moving agent's npd (and the policy its four distances) from the neighbour lookups the
// step issues anyway, and writes the state back once after the last step.  Its layout
// (layout_rollout) keeps the staging images clear of live data, so nothing is rebuilt
// between steps; stale low bits of dep are harmless: every occupant of a cell writes its
// move before anyone reads it.
template <int WIN, int KF, int LF, int GDE, bool RUN, int ROLL, int RULE = MAPFX_POLICY_DESCENT>
__device__ __forceinline__ void partial_body(const PGeo& g_, const PArgs& a_, const RArgs& ro, const RRun& rn,
                                             const int blk) {
  std::conditional_t<ROLL != 0, PArgs, const PArgs&> a = a_;  // (the rollout advances the outputs)
  PGeo g = g_;
  if constexpr (LF > 0) {  // the fast instances' lane group and K as constants (launch() picks
    g.L = LF;              // them only for g.L == LF, g.K == KF)
    g.lshift = __builtin_ctz(LF);
    g.K = KF;
  }
  extern __shared__ __align__(16) unsigned char lds_blk[];
  constexpr int H2 = WIN / 2;
  const int lane64 = threadIdx.x & 63;
  const int gw = blk * g.wpb + (int)(threadIdx.x >> 6);  // this wave's index
  unsigned char* const lds = lds_blk + (threadIdx.x >> 6) * g.lds;
  const int slot = lane64 >> g.lshift;
  const int ag = lane64 & (g.L - 1);
  const int base = slot << g.lshift;
  const int env = gw * g.EPW + slot;
  const int N = g.N;
  const bool env_ok = slot < g.EPW && env < g.E;
  const bool has = env_ok && ag < N;
  const uint64_t envmask = (g.L == 64 ? ~0ull : ((1ull << g.L) - 1ull)) << base;
  const int pitch = g.pitch;
  const int cs = env_ok ? slot : 0;  // LDS slot (idle lanes alias slot 0, write nothing)

  unsigned char* map = lds + g.off_map + cs * g.map_env_bytes;
  uint32_t* map32 = (uint32_t*)map;
  unsigned char* dep = lds + g.off_dep + cs * g.map_env_bytes;
  uint32_t* dep32 = (uint32_t*)dep;
  uint32_t* bitsL = (uint32_t*)(lds + g.off_bits + cs * g.bits_env_bytes);
  float* feat = (float*)(lds + g.off_feat + cs * g.feat_env_bytes);
  int2* posL = (int2*)(lds + g.off_pos + cs * g.pos_env_bytes);
  double* rewL = (double*)(lds + g.off_rew + cs * g.rew_env_bytes);

  PST_DECL
  PST(0);
  const long long oa = (long long)env * N + ag;
  // ---- every global read of the launch issued up front (idle lanes read entry 0),
  // the bitmap's first words first; optional arrays behind uniform branches, and no
  // loaded value used before the map build: a value tested right after its load would
  // put a wait on the vector-memory counter (in-order: on every load before it) into
  // the prologue ----
  const long long oc_ = has ? oa : 0;
  const int ec_ = env_ok ? env : 0;
  // RR: the runner's rollout (mapfx_runner_rollout) -- T runner steps of one launch.  Actions
  // are indexed by env (no act_row map, no compaction workgroup); an env's running / stale
  // flags and its return stay in registers across the loop
  constexpr bool RR = RUN && ROLL != 0;
  const bool runner = RUN && !RR && a.do_step && a.ra.act_row != nullptr;
  const bool post = RUN && a.ra.alive != nullptr;  // the runner's post pass, fused
  const bool nb_carry = a.pnbr && a.pdist && !g.gd32;  // neighbour distances carried
  const uint32_t* bsrc = (const uint32_t*)(a.bits + (g.map_shared ? 0 : (long long)ec_ * g.map_stride));
  const uint32_t bw0 = bsrc[ag < g.bits_words ? ag : 0];  // this lane's first bitmap word
  // the step's action: one 8-byte load of the aligned block that holds it (whatever the
  // dtype: the block lies in the element's page), decoded after the map build; the
  // runner's address needs the env's row of the MAC output first
  const int esh = a.act_dtype == MAPFX_I64 ? 3 : a.act_dtype == MAPFX_I32 ? 2 : 0;
  int arow = 0;
  long long ai = oc_;
  if (runner) {
    arow = a.ra.act_row[ec_];
    ai = (has && arow >= 0) ? (long long)arow * a.ra.act_row_stride + ag : 0;
  }
  const uintptr_t abyte = (uintptr_t)(a.do_step ? a.actions : (const void*)a.pos) + ((uintptr_t)ai << esh);
  const uint2 araw = *(const uint2*)(abyte & ~(uintptr_t)7);
  const int2 q = ((const int2*)a.goal)[oc_];
  const int2 ip = ((const int2*)a.init_pos)[oc_];
  const int2 p0 = ((const int2*)a.pos)[oc_];
  int pd_raw = 0;
  if (a.pdist) pd_raw = a.pdist[oc_];
  uint2 nb0 = make_uint2(0u, 0u);
  if (nb_carry && a.do_step) nb0 = ((const uint2*)a.pnbr)[oc_];
  const int steps0 = a.steps[oc_];
  const uint8_t at_goal0 = a.at_goal[oc_], dn0 = a.done[oc_], node0 = a.node[oc_];
  const int gcost0 = a.goal_cost[oc_], edge0 = a.edge[oc_];
  const int t0 = a.t[ec_], total0 = a.total_coll[ec_];
  const uint8_t term0 = a.terminated[ec_];
  uint32_t om_raw = 1, rm_raw = 1, live_raw = 0;
  if (RUN && a.obs_rows && a.obs_mask) om_raw = a.obs_mask[ec_];
  if (a.do_reset && a.reset_mask) rm_raw = a.reset_mask[ec_];
  double epr_raw = 0.0;
  int64_t epl_raw = 0;
  uint32_t stale_raw = 0;
  if (post) {
    live_raw = a.ra.alive[ec_];
    epr_raw = a.ra.ep_return[ec_];
    epl_raw = a.ra.ep_length[ec_];
    if constexpr (RR) stale_raw = a.ra.alive_prev[ec_];
  }
  if constexpr (KF > 0 && LF > 0 && ROLL != 2) {  // float32 sqrt(0 .. sq_max) for the K-nearest rows
    if (g.off_sqrt >= 0) {            // (:352 math.sqrt), while the loads are in flight
      float* sqt = (float*)(lds + g.off_sqrt);
#pragma unroll 1
      for (int i = lane64; i <= g.sq_max; i += 64) sqt[i] = (float)isqrt_f64(i);
    }
  }
  // ---- LDS map (c format) + dep map (obstacle flag in bit 7) ----
  // (staging the bitmap before the state loads are issued measured slower: 15.73 vs
  // 15.42 us per step)
  if (env_ok) {
    if (ag < g.bits_words) bitsL[ag] = bw0;
    for (int w = ag + g.L; w < g.bits_words; w += g.L) bitsL[w] = bsrc[w];  // maps past 16 x 32 words
  }
  PST(1);
  wave_fence();
  if (env_ok) {
    // word wi of the padded map = row pr, cells 4 pw .. 4 pw + 3 (pr = wi / wpr by a
    // multiply-high, exact below rows * wpr: checked at create); each word's 4 obstacle
    // bits from the two bitmap words around its first cell, every read of a group of
    // 4 words issued before any is used (no branch: off-grid cells are masked)
    const int nw = g.rows * g.wpr;
    for (int w0 = ag; w0 < nw; w0 += 4 * g.L) {
      uint32_t blo[4], bhi[4], vm[4];
      int sh[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int wi = w0 + u * g.L;
        const int pr = (int)__umulhi((uint32_t)wi, g.m_wpr), pw = wi - pr * g.wpr;
        const int rr = pr - g.P, cc = pw * 4 - g.pl;  // the word's grid row, first column
        const bool rin = (unsigned)rr < (unsigned)g.H;
        const int idx = (rin ? rr : 0) * g.W + cc;    // bit of the first cell (>= -8)
        const int iw = idx >> 5;
        blo[u] = bitsL[min(max(iw, 0), g.bits_words)];  // (bitsL has a slack word)
        bhi[u] = bitsL[min(max(iw + 1, 0), g.bits_words)];
        sh[u] = idx & 31;
        const int lv = max(0, -cc), hv = min(4, max(0, g.W - cc));  // on-grid cells lv .. hv - 1
        vm[u] = (rin && lv < hv) ? ((1u << hv) - 1u) & ~((1u << lv) - 1u) : 0u;
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int wi = w0 + u * g.L;
        if (wi < nw) {
          const uint32_t b4 = (uint32_t)((((uint64_t)bhi[u] << 32) | blo[u]) >> sh[u]) & 0xFu;
          const uint32_t ob4 = (b4 & vm[u]) | (~vm[u] & 0xFu);  // obstacle flags (off the grid: 1)
          const uint32_t f = (ob4 * 0x00204081u) & 0x01010101u;  // bit j -> byte j
          map32[wi] = f ^ 0x01010101u;  // c = 1 - obstacle before agents are added
          dep32[wi] = (f << 7) | 0x7F7F7F7Fu;
        }
      }
    }
  }
  wave_fence();
  PST(2);
  // ---- state (:125-163 for a reset env) ----
  const bool reset_me = env_ok && a.do_reset && rm_raw != 0;
  const bool omask = om_raw != 0;
  const uint8_t live0 = live_raw != 0 ? 1 : 0;
  const double epr0 = epr_raw;
  const int64_t epl0 = epl_raw;
  // RR: the env is running before the step (A[ts & 1]) / on the step's stale list (running
  // before step ts - 1: at entry the other parity half); the return so far, the steps it
  // ran in this launch, the wave's env steps (all but the last step's: the compaction adds
  // those)
  bool live = live0 != 0, stale = stale_raw != 0, stale_last = stale;
  double epr = epr0;
  int nlive = 0, wave_steps = 0;
  (void)live, (void)stale, (void)stale_last, (void)epr, (void)nlive, (void)wave_steps;
  const int gr = q.x, gc = q.y, ir = ip.x, ic = ip.y;
  int r = 0, c = 0, steps = 0, gcost = -1, edge = 0;
  int pd = PD_NONE;  // goal distance of the current cell (carried)
  bool at_goal = false, dn = false;
  uint32_t node = 0;
  if (has) {
    r = reset_me ? ir : p0.x;
    c = reset_me ? ic : p0.y;
    if (!reset_me) {
      steps = steps0;
      at_goal = at_goal0 != 0;
      dn = dn0 != 0;
      gcost = gcost0;
      node = node0;
      edge = edge0;
      pd = a.pdist ? pd_raw : PD_NONE;  // (pd_raw is 0 without pdist)
    }
  }
  int tcur = (env_ok && !reset_me) ? t0 : 0, total = (env_ok && !reset_me) ? total0 : 0;
  bool term = env_ok && !reset_me && term0 != 0;
  // the action (raw int64 as (alo, ahi); int8 / int32 sign-extended); an env outside
  // the runner's bs stays
  const uint32_t aw = (abyte & 4) ? araw.y : araw.x;
  int alo, ahi;
  if (a.act_dtype == MAPFX_I64) {
    alo = (int)araw.x;
    ahi = (int)araw.y;
  } else if (a.act_dtype == MAPFX_I32) {
    alo = (int)aw;
    ahi = alo >> 31;
  } else {
    alo = (int)(int8_t)(uint8_t)(aw >> ((abyte & 3) * 8));
    ahi = alo >> 31;
  }
  int act = 4;
  if (a.do_step && has && !(runner && arow < 0)) act = act_decode(alo, ahi);
  // goal-path distances (:227-233): a moving agent's npd is its target's entry of the
  // carried neighbour distances; without them (no pnbr, int32 tables, a state never reset)
  // the target's table entry is looked up here, and the current cell's when no carried
  // value applies (every non-step pass refreshes it)
  const bool nb_ok = nb_carry && a.do_step && pd != PD_NONE;
  const bool need_cur = has && (!a.do_step || !a.pdist || pd == PD_NONE);
  int npd_t = 0;
  // the goal distances of the current cell's neighbours (up, down, left, right): the
  // step's lookups for the next step; the rollout carries them from step to step
  int nbd0 = 0, nbd1 = 0, nbd2 = 0, nbd3 = 0;
  // the four neighbours of (r, c) from the table (an off-grid one: the cell itself)
  const auto nbr_lookup = [&]() {
    const long long gi = oc_ * g.hw + r * g.W + c;
    nbd0 = gd_entry_t<GDE>(g, a.gd, gi + (r > 0 ? -g.W : 0));
    nbd1 = gd_entry_t<GDE>(g, a.gd, gi + (r + 1 < g.H ? g.W : 0));
    nbd2 = gd_entry_t<GDE>(g, a.gd, gi + (c > 0 ? -1 : 0));
    nbd3 = gd_entry_t<GDE>(g, a.gd, gi + (c + 1 < g.W ? 1 : 0));
  };
  if constexpr (ROLL == 0) {
    if (has && !nb_ok) {
      const int tgt = (a.do_step && !dn) ? move_target(g, r, c, act) : -1;
      if (tgt >= 0) npd_t = gd_entry_t<GDE>(g, a.gd, oa * g.hw + tgt);
      if (need_cur) pd = gd_entry_t<GDE>(g, a.gd, oa * g.hw + r * g.W + c);
    }
  } else {  // once per launch: the carried distances, or the table where none apply
    if (has && nb_ok) {
      nbd0 = nbr_dist(nb0, 0), nbd1 = nbr_dist(nb0, 1), nbd2 = nbr_dist(nb0, 2), nbd3 = nbr_dist(nb0, 3);
    } else if (has) {
      if (need_cur) pd = gd_entry_t<GDE>(g, a.gd, oa * g.hw + r * g.W + c);
      nbr_lookup();
    }
  }
  PST(3);
  int cur = (r + g.P) * pitch + c + g.pl;
  if (has) atomicAdd(&map32[cur >> 2], 1u << ((cur & 3) * 8));
  wave_fence();
  PST(4);

  // the rollout's given actions: row k + 1's block is fetched while step k runs -- an
  // unconditional load (a conditional one compiles to a synchronous fetch), its row
  // clamped below T
  const long long act_row_bytes = (ROLL != 0 && ro.policy) ? 0 : ((long long)g.E * N) << esh;
  uint2 araw_n = araw;
  uintptr_t abyte_n = abyte;
  const auto decode_raw = [&](uint2 raw, uintptr_t ab) {
    const uint32_t w = (ab & 4) ? raw.y : raw.x;
    if (a.act_dtype == MAPFX_I64) return act_decode((int)raw.x, (int)raw.y);
    if (a.act_dtype == MAPFX_I32) return act_decode((int)w, (int)w >> 31);
    const int v = (int)(int8_t)(uint8_t)(w >> ((ab & 3) * 8));
    return act_decode(v, v >> 31);
  };
  // ---- state write-back (the step kernel: with its results; the rollout: after its loop) ----
  const auto write_back = [&]() {
    if (has) {
      ((int2*)a.pos)[oa] = make_int2(r, c);
      a.steps[oa] = steps;
      a.at_goal[oa] = at_goal ? 1 : 0;
      a.done[oa] = dn ? 1 : 0;
      a.goal_cost[oa] = gcost;
      a.node[oa] = (uint8_t)node;
      a.edge[oa] = edge;
      if (a.pdist) a.pdist[oa] = pd;
      if (runner && arow >= 0) {  // the EpisodeBatch's actions / actions_onehot rows at ts
        const long long v = act_value(alo, ahi);
        if (a.ra.ep_actions)
          a.ra.ep_actions[(long long)env * a.ra.ep_actions_sb + (long long)a.ra.ts * a.ra.ep_actions_st + ag] = v;
        if (a.ra.ep_onehot) {
          float* oh = a.ra.ep_onehot + (long long)env * a.ra.ep_onehot_sb +
                      (long long)a.ra.ts * a.ra.ep_onehot_st + (long long)ag * 5;
#pragma unroll
          for (int q = 0; q < 5; ++q) oh[q] = v == q ? 1.0f : 0.0f;
        }
      }
    }
    if (env_ok && ag == 0) {
      a.t[env] = tcur;
      a.terminated[env] = term ? 1 : 0;
      a.total_coll[env] = total;
    }
  };
  const int T = ROLL ? ro.T : 1;
  // RR: the env's last step in this launch was a full step of an env already terminated --
  // nobody moved (every agent of a terminated env is done), so its node / edge flags stand
  bool quiet = !env_ok;
  (void)quiet;
  for (int k = 0; k < T; ++k) {  // (the step kernel: one pass, no loop is left in its code)
  const bool term_in = term;
  (void)term_in;
  if constexpr (RR) {
    // A wave none of whose envs is running or stale leaves the loop.  The steps it skips
    // write no row, and what they do to the env state (the step form steps a terminated env
    // too, with stay) is known once every env is quiet: each counts the standing collisions
    // again, advances the step count and stamps it on the agents at their goals.
    if (!__ballot((env_ok && (live || stale)) || !quiet)) {
      const int R = T - k;
      const int esum = group_sum(has ? (int)node + edge : 0, LF > 0 ? LF : g.L);
      tcur += R;
      total += R * (esum / 2);
      if (at_goal) gcost = tcur;
      stale_last = false;
      break;
    }
  }
  if constexpr (ROLL != 0) {
    // autoreset: a terminated env restarts from init_pos (:125-163) before it is stepped
    const bool rs = ro.autoreset && term;
    if (__ballot(rs)) {
      if (rs && has) atomicSub(&map32[cur >> 2], 1u << ((cur & 3) * 8));
      if (rs) {
        r = has ? ir : 0;
        c = has ? ic : 0;
        steps = 0, gcost = -1, edge = 0, node = 0;
        at_goal = dn = term = false;
        tcur = total = 0;
        cur = (r + g.P) * pitch + c + g.pl;
        if (has) {
          atomicAdd(&map32[cur >> 2], 1u << ((cur & 3) * 8));
          pd = gd_entry_t<GDE>(g, a.gd, oa * g.hw + r * g.W + c);
          nbr_lookup();
        }
      }
      wave_fence();
    }
    if (ro.policy) {
      uint32_t pm = 16u;  // the pre-step avail mask, from the resident map
      if (map[cur - pitch]) pm |= 1u;
      if (map[cur + pitch]) pm |= 2u;
      if (map[cur - 1]) pm |= 4u;
      if (map[cur + 1]) pm |= 8u;
      if constexpr (RULE == MAPFX_POLICY_PIBT)  // (every lane of the wave: the plan runs on ballots)
        act = pibt_action(ro, N, env, k, ag, has, base, envmask, pm, pd, nbd0, nbd1, nbd2, nbd3, cur, pitch);
      else
        act = has ? policy_action(ro, env, k, ag, pm, pd, nbd0, nbd1, nbd2, nbd3) : 4;
      if (has && ro.actions) ro.actions[(long long)k * g.E * N + oa] = (int8_t)act;
    } else if (k > 0) {
      act = has ? decode_raw(araw_n, abyte_n) : 4;
    }
    if constexpr (RR) {
      // the actions / actions_onehot rows at ts of an env on the stale list (a terminated
      // one is there once more, with the action its resting state gives); an env off it stays
      if (!stale) {
        act = 4;
      } else if (has) {
        long long v = act;  // the raw value, as the step form records it
        if (!ro.policy) {
          const uint32_t w = (abyte_n & 4) ? araw_n.y : araw_n.x;
          const int b8 = (int)(int8_t)(uint8_t)(w >> ((abyte_n & 3) * 8));
          v = a.act_dtype == MAPFX_I64   ? act_value((int)araw_n.x, (int)araw_n.y)
              : a.act_dtype == MAPFX_I32 ? (long long)(int)w
                                         : (long long)b8;
        }
        const long long ts = rn.ts0 + k;
        if (a.ra.ep_actions) a.ra.ep_actions[(long long)env * a.ra.ep_actions_sb + ts * a.ra.ep_actions_st + ag] = v;
        if (a.ra.ep_onehot) {
          float* oh = a.ra.ep_onehot + (long long)env * a.ra.ep_onehot_sb + ts * a.ra.ep_onehot_st + (long long)ag * 5;
#pragma unroll
          for (int q = 0; q < 5; ++q) oh[q] = v == q ? 1.0f : 0.0f;
        }
      }
    }
    // (policy mode: row stride 0 -- the dummy block again, outside every branch)
    // a GLOBAL load: a flat one also counts on the LDS counter, and the step's next LDS
    // read would wait for it
    abyte_n = abyte + (uintptr_t)(act_row_bytes * min(k + 1, T - 1));
    typedef const unsigned long long __attribute__((address_space(1))) * GlobalU64;
    const unsigned long long blk8 = *(GlobalU64)(abyte_n & ~(uintptr_t)7);
    araw_n = make_uint2((uint32_t)blk8, (uint32_t)(blk8 >> 32));
  }
  // ---- step (:165-310) ----
  double Rsum = 0.0;  // sum(rewards) of the env (agent-0 lane)
  if (a.do_step && env_ok) {
    const bool skip = (__ballot(act < 0) & envmask) != 0;  // the reference asserts (:174)
    if (!skip) {
      ++tcur;  // :178
      double rew = 0.0;  // rewards[i] = 0 (:183)
      bool moved = false;
      int nc = cur;
      uint32_t v = 0;
      if (has && !dn) {  // :193-211
        ++steps;
        bool envc = false;
        if (act != 4) {
          const int d = act == 0 ? -pitch : act == 1 ? pitch : act == 2 ? -1 : 1;
          v = map[cur + d];   // PRE-step occupancy: 0 = out of bounds / free-standing obstacle
          if (v == 0) envc = true;
          else {
            nc = cur + d;
            moved = true;
          }
        }
        if (envc) rew = rew + g.env_rew;                    // :203
        if (act != 4) rew = rew + g.move_rew;               // :207
        else rew = rew + (at_goal ? g.stay_goal_rew : g.stay_rew);  // :209-212
      }
      const int nr = r + (moved ? (act == 0 ? -1 : act == 1 ? 1 : 0) : 0);
      const int ncol = c + (moved ? (act == 2 ? -1 : act == 3 ? 1 : 0) : 0);
      at_goal = has && nr == gr && ncol == gc;              // :214-219
      if (at_goal) gcost = tcur;
      if (tcur >= g.limit) {                                // :221-225
        term = true;
        dn = true;
      }
      if (has) {                                            // :227-233
        const int opd = pd;
        int npd;
        if constexpr (ROLL != 0) npd = moved ? (act == 0 ? nbd0 : act == 1 ? nbd1 : act == 2 ? nbd2 : nbd3) : opd;
        else npd = moved ? (nb_ok ? nbr_dist(nb0, act) : npd_t) : opd;
        rew = rew + (double)(opd - npd) / (double)g.limit;
        pd = npd;
      }
      // counts move; node / edge collisions (:708-727, :822-857)
      if (has) dep[cur] = (unsigned char)((dep[cur] & 0x80u) | (moved ? (uint32_t)act : 0x7Fu));
      wave_fence();
      if (moved) {
        atomicSub(&map32[cur >> 2], 1u << ((cur & 3) * 8));
        atomicAdd(&map32[nc >> 2], 1u << ((nc & 3) * 8));
      }
      wave_fence();
      PST(5);
      const uint32_t dj = has ? dep[nc] : 0x7Fu;
      const uint32_t cn = has ? map[nc] : 0u;
      node = (has && cn + (dj >> 7) >= 3u) ? 1u : 0u;
      const int pre = (int)v - 1 + (int)(dj >> 7);
      edge = 0;
      const bool suspect = moved && pre > 0;
      if (__ballot(suspect)) {
        if (suspect && pre == 1) edge = (dj & 0x7Fu) == (uint32_t)(act ^ 1) ? 1 : 0;
        if (__ballot(suspect && pre > 1)) {  // stacked pre-occupants: scan the env's agents
          if (g.L == 16) {  // the env is one DPP row: rotate its (old, new) cells past each lane
            int e2 = 0;
            dpp_edge_scan<1>(cur, nc, e2);
            if (suspect && pre > 1) edge += e2;
          } else {
            for (int j = 0; j < N; ++j) {
              const int oj = __shfl(cur, base + j);
              const int nj = __shfl(nc, base + j);
              if (suspect && pre > 1) edge += (oj == nc) & (nj == cur);
            }
          }
        }
      }
      // env sums: total collisions += (sum(node) + sum(edge)) // 2  (:239)
      const int esum = group_sum(has ? (int)node + edge : 0, LF > 0 ? LF : g.L);
      total += esum / 2;
      rew = rew + g.nc_rew * (double)node;  // :247
      rew = rew + g.ec_rew * (double)edge;  // :249
      r = nr;
      c = ncol;
      cur = nc;
      // all at goals: dones, terminated, completion bonus (:283-299)
      const bool all_at = (__ballot(has && !at_goal) & envmask) == 0;
      if (all_at) {
        dn = true;
        term = true;
        const int bi = min(tcur, g.bonus_len - 1);
        rew = rew + a.bonus_lut[bi];
      }
      PST(6);
      // sum(rewards): naive left fold in agent order (:310)
      if (g.L <= 16) {
        const double R = row_fold<LF>(has ? rew : 0.0, N);
        if (ag == 0) {
          if (a.reward) a.reward[env] = R;
          Rsum = R;
        }
      } else {
        if (has) rewL[ag] = rew;
        wave_fence();
        if (ag == 0) {
          double R = 0.0;
          for (int j = 0; j < N; ++j) R = R + rewL[j];
          if (a.reward) a.reward[env] = R;
          Rsum = R;
        }
      }
      PST(7);
      if constexpr (RR) quiet = term_in;
    } else {
      if constexpr (RR) quiet = false;
      if (ag == 0 && a.err) atomicCAS(a.err, 0, env + 1);
      if (ag == 0 && a.reward) a.reward[env] = 0.0;
    }
  }
  wave_fence();
  // the goal distances of the (new) cell's neighbours, carried to the next step: issued
  // here, consumed before the staged copy-out (the observation rows hide their latency)
  // -- unconditional loads (idle lanes read agent 0's table at (0, 0), an off-grid
  // neighbour the cell itself; no branch, so no use of a value can move up to its load)
  // (u8 tables, H * W <= 255: the 4 lookups of an agent fall in one 64-byte table, so one
  // memory request; int16 tables span two)
  nbr_lookup();

  PST(8);
  // ---- the step's results leave before the observation rows are built: their stores
  // then queue ahead of the rows' copy-out instead of behind it ----
  // avail (:399-433): neighbour in bounds and not a free-standing obstacle
  uint32_t am = 16u;
  if (has && (a.avail || (RUN && a.ra.ep_avail))) {
    if (map[cur - pitch]) am |= 1u;
    if (map[cur + pitch]) am |= 2u;
    if (map[cur - 1]) am |= 4u;
    if (map[cur + 1]) am |= 8u;
    if (a.avail) a.avail[oa] = (uint8_t)am;
  }
  // state (:377-387): [total collisions, step count, sum(each goal cost)]
  const int gsum = group_sum(has ? gcost : 0, LF > 0 ? LF : g.L);
  if (env_ok && ag == 0 && a.state) {
    a.state[3 * env + 0] = (float)total;
    a.state[3 * env + 1] = (float)tcur;
    a.state[3 * env + 2] = (float)gsum;
  }
  if constexpr (ROLL == 0) {
    write_back();
  } else {  // the rollout's state stays in registers: its trajectory slots instead
    if (has && ro.pos) ((int2*)ro.pos)[(long long)k * g.E * N + oa] = make_int2(r, c);
    if (env_ok && ag == 0 && ro.terminated) ro.terminated[(long long)k * g.E + env] = term ? 1 : 0;
  }
  if (post && env_ok) {  // runner_post_kernel (runner.hip) for a running env, fused
    const mapfx_runner_acts& ra = a.ra;
    // the step's time row and the rows at ts + 1 (the step form: as the call gave them)
    int ts = ra.ts;
    float* ep_state = ra.ep_state;
    int32_t* ep_avail = ra.ep_avail;
    int64_t* ep_filled = ra.ep_filled;
    if constexpr (RR) {
      ts = rn.ts0 + k;
      const bool nxt = ts + 1 < rn.max_t;
      ep_state = nxt && ra.ep_state ? ra.ep_state + (long long)(ts + 1) * rn.state_st : nullptr;
      ep_avail = nxt && ra.ep_avail ? ra.ep_avail + (long long)(ts + 1) * rn.avail_st : nullptr;
      ep_filled = nxt && ra.ep_filled ? ra.ep_filled + (long long)(ts + 1) * rn.filled_st : nullptr;
    }
    if (RR ? live : live0 != 0) {
      if (ag == 0) {
        if (ra.ep_reward) ra.ep_reward[(long long)env * ra.ep_reward_sb + (long long)ts * ra.ep_reward_st] = (float)Rsum;
        // env_terminated = terminated and not info.get("episode_limit") (parallel_runner.py:146-150):
        // MARL_PARTIAL's info has no "episode_limit" key
        if (ra.ep_term) ra.ep_term[(long long)env * ra.ep_term_sb + (long long)ts * ra.ep_term_st] = term ? 1 : 0;
        if constexpr (RR) {  // (stored once, after the loop)
          epr = epr + Rsum;
          ++nlive;
        } else {
          ra.ep_return[env] = epr0 + Rsum;
          ra.ep_length[env] = epl0 + 1;
          if (!ra.cmp_bs) ra.alive[env] = term ? 0 : 1;  // (fused compaction: A_out below)
        }
        if (ep_state) {  // update(pre_transition_data, bs, ts + 1): state, avail, filled
          float* d = ep_state + (long long)env * ra.ep_state_sb;
          d[0] = (float)total;
          d[1] = (float)tcur;
          d[2] = (float)gsum;
        }
        if (ep_filled) ep_filled[(long long)env * ra.ep_filled_sb] = 1;
      }
      if (has && ep_avail) {
        int32_t* d = ep_avail + (long long)env * ra.ep_avail_sb + ag * 5;
#pragma unroll
        for (int k = 0; k < 5; ++k) d[k] = (int32_t)((am >> k) & 1u);
      }
    }
    // alive_prev: the stale list for the separate compaction, or, with the compaction
    // fused (cmp_bs), A[(ts + 1) & 1] = running after this step, written for every env
    // (the rollout: both parity halves once, after the loop)
    if constexpr (!RR)
      if (ag == 0) ra.alive_prev[env] = ra.cmp_bs ? (uint8_t)(live0 && !term ? 1 : 0) : live0;
  }
  uint2 nb1 = make_uint2(0u, 0u);
  if constexpr (ROLL != 2) {  // (a rollout without the rows builds and stages none of this)
  // ---- observations of the current state (:312-391) ----
  // per-agent feature rows: curr, start, goal, unit vec, norm, node, edge, steps
  if (has) {
    const int d0 = gr - r, d1 = gc - c;
    const double nrm = isqrt_f64(d0 * d0 + d1 * d1);   // :937
    const double ux = nrm == 0.0 ? 0.0 : (double)d0 / nrm;   // :938-941
    const double uy = nrm == 0.0 ? 0.0 : (double)d1 / nrm;
    float* fr = feat + ag * FR;
    fr[0] = (float)r; fr[1] = (float)c; fr[2] = (float)ir; fr[3] = (float)ic;
    fr[4] = (float)gr; fr[5] = (float)gc; fr[6] = (float)ux; fr[7] = (float)uy;
    fr[8] = (float)nrm; fr[9] = (float)node; fr[10] = (float)edge; fr[11] = (float)steps;
    posL[ag] = make_int2(r, c);
  }
  wave_fence();
  PST(9);
  constexpr int WW = WIN * WIN;
  constexpr int DF = (KF > 0 && LF > 0) ? 2 * WW + NF * KF : 1;  // fast-path row length
  float o[DF];
  // (the runner's rollout: the rows at ts + 1 of the envs running before this step)
  const bool om = RR ? (live && rn.ts0 + k + 1 < rn.max_t) : omask;
  float* const my_obs = (env_ok && om) ? obs_env_nomask<RUN>(a, env, (KF > 0 && LF > 0) ? DF : g.D, N) : nullptr;
  // Staged copy-out (fast path): the rows of the envs of a staging group (the whole wave,
  // or each half of it) are one contiguous run of the destination (a.obs), or one run
  // per env (EpisodeBatch rows): each run is staged in LDS as its byte image, at the
  // run's own 16-byte misalignment, and copied with lane-contiguous 16-byte stores --
  // per-lane dword stores of 460-byte rows touch 64 lines each.  The images alias the LDS
  // regions the step is done with (dep onwards).  (Sending the window planes first, while
  // the K-nearest rows are built, measured 19.0 vs 15.2 us: chunks of partial lines.)
  constexpr bool FAST = KF > 0 && LF > 0;
  const bool one_run = !RUN || a.obs_rows == nullptr;
  const bool staged = FAST && (a.obs || (RUN && a.obs_rows)) && g.off_stage >= 0;
  // this lane's row of group gi's image (G lanes per group)
  auto stage_row = [&](int gi, int G, int i0, int i1) {
    const int s0 = (G * gi) >> g.lshift;
    if (has && my_obs && lane64 / G == gi) {
      const int kme = slot - s0;  // this lane's env within the group
      const float* rb = one_run ? a.obs + (long long)(gw * g.EPW + s0) * N * DF : my_obs;
      const uint32_t mis = (uint32_t)(uintptr_t)rb & 15u;
      const int k = one_run ? 0 : kme;
      const int ri = (one_run ? kme * N : 0) + ag;  // row within the run
      uint32_t* row = (uint32_t*)(lds + g.off_stage + k * g.stage_env_bytes + mis + ri * (DF * 4));
#pragma unroll
      for (int i = 0; i < DF; ++i)
        if (i >= i0 && i < i1) row[i] = __float_as_uint(o[i]);
    }
  };
  // copy group gi's runs
  auto copy_runs = [&](int gi, int G) {
    const int s0 = (G * gi) >> g.lshift;
    const int ne = max(0, min(min(G >> g.lshift, g.EPW - s0), g.E - (gw * g.EPW + s0)));  // signed
    const int nrun = one_run ? (ne > 0 ? 1 : 0) : ne;
    const int rowB = DF * 4;
    for (int k = 0; k < nrun; ++k) {
      unsigned char* gdst;
      if (one_run) {
        gdst = (unsigned char*)(a.obs + (long long)(gw * g.EPW + s0) * N * DF);
      } else {  // env s0 + k's destination, from its agent-0 lane (NULL: masked)
        const uint64_t pe = (uint64_t)(uintptr_t)my_obs;
        const int src = (s0 + k) << g.lshift;
        const uint32_t lo = __builtin_amdgcn_readlane((uint32_t)pe, src);
        const uint32_t hi = __builtin_amdgcn_readlane((uint32_t)(pe >> 32), src);
        gdst = (unsigned char*)(uintptr_t)(((uint64_t)hi << 32) | lo);
        if (!gdst) continue;
      }
      const uint32_t mis = (uint32_t)(uintptr_t)gdst & 15u;
      const unsigned char* img = lds + g.off_stage + k * g.stage_env_bytes + mis;
      const int nbytes = (one_run ? ne : 1) * N * rowB;
      const int head = mis ? min(16 - (int)mis, nbytes) : 0;  // a multiple of 4
      const int body = (nbytes - head) & ~15;
      if (lane64 < head / 4) ((uint32_t*)gdst)[lane64] = ((const uint32_t*)img)[lane64];
      const uint4* s4 = (const uint4*)(img + head);  // 16-byte aligned: mis + head
      uint4* g4 = (uint4*)(gdst + head);
      const int n16 = body / 16;
      // four LDS reads in flight per lane before their stores
      for (int i = lane64; i < n16; i += 256) {
        const bool b1 = i + 64 < n16, b2 = i + 128 < n16, b3 = i + 192 < n16;
        const uint4 v0 = s4[i];
        uint4 v1, v2, v3;
        if (b1) v1 = s4[i + 64];
        if (b2) v2 = s4[i + 128];
        if (b3) v3 = s4[i + 192];
        g4[i] = v0;
        if (b1) g4[i + 64] = v1;
        if (b2) g4[i + 128] = v2;
        if (b3) g4[i + 192] = v3;
      }
      const int tail = nbytes - head - body;
      if (lane64 < tail / 4)
        ((uint32_t*)(gdst + head + body))[lane64] = ((const uint32_t*)(img + head + body))[lane64];
    }
  };
  if (has && my_obs) {
    if constexpr (FAST) {
      // -------- fast path: the whole row in registers --------
      if constexpr (WIN > 0) {  // window planes (:327-342) from whole map words
        const int wb = (cur - H2 * pitch - H2);
        const int sh = (wb & 3) * 8;
#pragma unroll
        for (int y = 0; y < WIN; ++y) {
          const uint32_t* rowp = map32 + ((wb + y * pitch) >> 2);
          const uint64_t lo = ((uint64_t)rowp[1] << 32) | rowp[0];
          const uint32_t x03 = (uint32_t)(lo >> sh);
          uint32_t x47 = 0u;  // cells 4-7 (WIN > 4)
          if constexpr (WIN > 4) {
            const uint64_t hi = ((uint64_t)rowp[2] << 32) | rowp[1];
            x47 = (uint32_t)(hi >> sh);
          }
#pragma unroll
          for (int x = 0; x < WIN; ++x) {
            const uint32_t cv = ((x < 4 ? x03 : x47) >> (8 * (x & 3))) & 0xFFu;
            o[y * WIN + x] = cv == 0 ? 1.0f : 0.0f;
            o[WW + y * WIN + x] = cv == 0 ? 0.0f : (float)(cv - 1u);  // max(count - obst, 0)
          }
        }
      }
      // K nearest (:346-372): keys = sq distance * 64 + index, selected by repeated min
      uint32_t key[LF];
#pragma unroll
      for (int j = 0; j < LF; ++j) {
        const int2 pj = posL[j];
        const int dr = r - pj.x, dc = c - pj.y;
        key[j] = (j < N && j != ag) ? (uint32_t)(dr * dr + dc * dc) * 64u + (uint32_t)j : 0xFFFFFFFFu;
      }
      const int km1 = min(N, KF) - 1;
      float* k0 = o + 2 * WW;
      const float* me = feat + ag * FR;
#pragma unroll
      for (int q = 0; q < 11; ++q) k0[q] = me[q];
      k0[11] = (float)(g.H * g.W);  // distance to itself (:543-545)
      k0[12] = me[11];
      // round sI takes the smallest key above the last one: keys are distinct, so with
      // prev1 = last + 1 every key <= last wraps to ~2^32 in key - prev1 (an unused
      // slot's 0xFFFFFFFF stays above every real key) and one min over key - prev1 finds
      // it -- a subtract and a third of a min3 per key (was compare, compare, select)
      uint32_t prev1 = 0u;
      const float* sqt = (const float*)(lds + (g.off_sqrt >= 0 ? g.off_sqrt : 0));
      // (a branch per round measured faster than computing every round and selecting -1:
      // 15.2 vs 16.2 us)
      const auto rounds = [&](auto lut) {  // lut: the distances from the wave's table
#pragma unroll
        for (int sI = 1; sI < KF; ++sI) {
          float* row = o + 2 * WW + sI * NF;
          if (sI <= km1) {
            uint32_t m = 0xFFFFFFFFu;
#pragma unroll
            for (int j = 0; j < LF; ++j) m = min(m, key[j] - prev1);
            const uint32_t best = m + prev1;
            prev1 = best + 1u;
            const int j = (int)(best & 63u);
            const float* fj = feat + j * FR;
#pragma unroll
            for (int q = 0; q < 11; ++q) row[q] = fj[q];
            if constexpr (decltype(lut)::value) row[11] = sqt[best >> 6];
            else row[11] = (float)isqrt_f64((int)(best >> 6));
            row[12] = fj[11];
          } else {
#pragma unroll
            for (int q = 0; q < NF; ++q) row[q] = -1.0f;
          }
        }
      };
      if (g.off_sqrt >= 0) rounds(std::true_type{});
      else rounds(std::false_type{});
    } else {
      // -------- generic path --------
      float* o = my_obs + ag * g.D;
      if constexpr (WIN > 0) {  // window planes (:327-342): OOB / obstacle -> 1; agents -> count
        for (int y = 0; y < WIN; ++y) {
          for (int x = 0; x < WIN; ++x) {
            const uint32_t cv = map[cur + (y - H2) * pitch + (x - H2)];
            o[y * WIN + x] = cv == 0 ? 1.0f : 0.0f;
            o[WW + y * WIN + x] = cv == 0 ? 0.0f : (float)(cv - 1u);
          }
        }
      }
      // K nearest agents (:346-372): self first, then the k-1 nearest others by L2
      // distance (sorted() is stable: ties by agent index); rows past min(N, K) = -1
      float* kn = o + 2 * WW;
      const int K = g.K;
      const int km1 = min(N, K) - 1;
      for (int q = 0; q < 11; ++q) kn[q] = feat[ag * FR + q];
      kn[11] = (float)(g.H * g.W);  // distance to itself (:543-545)
      kn[12] = feat[ag * FR + 11];
      long long prev = -1;
      for (int sI = 1; sI <= km1; ++sI) {
        long long best = 0x7FFFFFFFFFFFFFFFll;
        for (int j = 0; j < N; ++j) {
          if (j == ag) continue;
          const int2 pj = posL[j];
          const int dr = r - pj.x, dc = c - pj.y;
          const long long key = (long long)(dr * dr + dc * dc) * 64 + j;
          if (key > prev && key < best) best = key;
        }
        prev = best;
        const int j = (int)(best & 63);
        const int sq = (int)(best >> 6);
        float* row = kn + sI * NF;
        for (int q = 0; q < 11; ++q) row[q] = feat[j * FR + q];
        row[11] = (float)isqrt_f64(sq);
        row[12] = feat[j * FR + 11];
      }
      for (int sI = km1 + 1; sI < K; ++sI)
        for (int q = 0; q < NF; ++q) kn[sI * NF + q] = -1.0f;
    }
  }
  PST(10);
  // the carried neighbour distances (their loads have landed by now)
  if constexpr (ROLL == 0) {
    nb1 = make_uint2(((uint32_t)nbd0 & 0xFFFFu) | ((uint32_t)nbd1 << 16),
                     ((uint32_t)nbd2 & 0xFFFFu) | ((uint32_t)nbd3 << 16));
    asm volatile("" : "+v"(nb1.x), "+v"(nb1.y));
  }
  if constexpr (FAST) {
    if (g.off_stage < 0 && has && my_obs) {  // rows straight to HBM (per-lane stores)
      uint32_t* d = (uint32_t*)(my_obs + ag * DF);
#pragma unroll
      for (int i = 0; i < DF; ++i) d[i] = __float_as_uint(o[i]);
    }
    if (staged) {
      const int G = g.stage_lanes;  // 64 or 32
      wave_fence();
      for (int gi = 0; gi < 64 / G; ++gi) {
        if (max(0, min(min(G >> g.lshift, g.EPW - ((G * gi) >> g.lshift)),
                       g.E - (gw * g.EPW + ((G * gi) >> g.lshift)))) == 0)
          break;
        stage_row(gi, G, 0, DF);
        wave_fence();
        copy_runs(gi, G);
        wave_fence();  // the next group's rows reuse the images
      }
    }
  }
  PST(11);
  (void)o;
  }
  if constexpr (ROLL == 0) {
    // the carried neighbour distances are stored last (their loads land during the rows)
    if (has && nb_carry) ((uint2*)a.pnbr)[oa] = nb1;
  } else {  // the next step's slots
    if (a.reward) a.reward += g.E;
    if (a.obs) a.obs += (long long)g.E * N * g.D;
    if (a.state) a.state += 3ll * g.E;
    if (a.avail) a.avail += (long long)g.E * N;
    if constexpr (RR) {  // the next step's time row and flags
      if (a.obs_rows) a.obs_rows += rn.obs_st;
      if (k + 1 < T) wave_steps += __popcll(__ballot(env_ok && ag == 0 && live));
      stale_last = stale;
      stale = live;
      live = live && !term;
    }
  }
  }  // for k
  if constexpr (ROLL != 0) {  // the state leaves once, after the last step
    write_back();
    if (has && nb_carry)
      ((uint2*)a.pnbr)[oa] = make_uint2(((uint32_t)nbd0 & 0xFFFFu) | ((uint32_t)nbd1 << 16),
                                        ((uint32_t)nbd2 & 0xFFFFu) | ((uint32_t)nbd3 << 16));
  }
  if constexpr (RR) {
    // The runner's bookkeeping as T runner steps leave it: A[(ts + 1) & 1] = running after
    // the last step ts, A[ts & 1] = running before it (`alive` is the half of ts0's parity);
    // returns / lengths of the envs that ran; the stale list of the last step as flags
    // where its row map goes (the compaction that follows turns them into rows)
    if (post && env_ok && ag == 0) {
      const mapfx_runner_acts& ra = a.ra;
      const bool odd = (T & 1) != 0;
      ra.alive[env] = (odd ? stale : live) ? 1 : 0;
      ra.alive_prev[env] = (odd ? live : stale) ? 1 : 0;
      if (nlive) {
        ra.ep_return[env] = epr;
        ra.ep_length[env] = epl0 + nlive;
      }
      if (rn.stale_out) rn.stale_out[env] = stale_last ? 0 : -1;
    }
    if (post && lane64 == 0 && wave_steps)
      atomicAdd((unsigned long long*)a.ra.cmp_env_steps, (unsigned long long)wave_steps);
  }
  PST(12);
#ifdef PARTIAL_STAMPS
  __builtin_amdgcn_s_waitcnt(0);
  PST(13);
  PST_FLUSH();
#endif
}

template <int WIN, int KF, int LF, int GDE = 0, bool RUN = true>
__global__ void __launch_bounds__(64 * PARTIAL_MAX_WPB) partial_kernel(PGeo g_, PArgs a) {
  int blk = (int)blockIdx.x;
  if constexpr (RUN) {  // the runner's fused compaction: the launch's extra first workgroup
    if (a.ra.cmp_bs && blk-- == 0) {
      extern __shared__ __align__(16) unsigned char lds_cmp[];
      runner_compact_block(a.ra, lds_cmp);
      return;
    }
  }
  partial_body<WIN, KF, LF, GDE, RUN, 0>(g_, a, RArgs{}, RRun{}, blk);
}

// T steps of every env in one launch (mapfx_partial_rollout).  OBS false: the trajectory
// has no observation rows, and WIN / KF play no part.
template <int WIN, int KF, int LF, int GDE, bool OBS>
__global__ void __launch_bounds__(64 * PARTIAL_MAX_WPB) partial_rollout_kernel(PGeo g_, PArgs a, RArgs ro) {
  partial_body<WIN, KF, LF, GDE, false, OBS ? 1 : 2>(g_, a, ro, RRun{}, (int)blockIdx.x);
}

// T runner steps of every env in one launch (mapfx_runner_rollout): the rollout's loop with
// the runner's actions rows, post pass and flags (RUN) per step.  OBS false: rows->obs NULL.
template <int WIN, int KF, int LF, int GDE, bool OBS>
__global__ void __launch_bounds__(64 * PARTIAL_MAX_WPB) partial_runner_rollout_kernel(PGeo g_, PArgs a, RArgs ro,
                                                                                      RRun rn) {
  partial_body<WIN, KF, LF, GDE, true, OBS ? 1 : 2>(g_, a, ro, rn, (int)blockIdx.x);
}

// The two rollout kernels with the policy rule MAPFX_POLICY_PIBT (policy mode only): instances
// of their own, so the descent instances keep their code and their registers.
template <int WIN, int KF, int LF, int GDE, bool OBS>
__global__ void __launch_bounds__(64 * PARTIAL_MAX_WPB) partial_pibt_rollout_kernel(PGeo g_, PArgs a, RArgs ro) {
  partial_body<WIN, KF, LF, GDE, false, OBS ? 1 : 2, MAPFX_POLICY_PIBT>(g_, a, ro, RRun{}, (int)blockIdx.x);
}
template <int WIN, int KF, int LF, int GDE, bool OBS>
__global__ void __launch_bounds__(64 * PARTIAL_MAX_WPB) partial_pibt_runner_rollout_kernel(PGeo g_, PArgs a,
                                                                                           RArgs ro, RRun rn) {
  partial_body<WIN, KF, LF, GDE, true, OBS ? 1 : 2, MAPFX_POLICY_PIBT>(g_, a, ro, rn, (int)blockIdx.x);
}

// A goal-table rebuild makes the carried distances stale: pdist of every (masked) env
// becomes PD_NONE, so its next step looks the current and target cells up in the new
// table (marl_partial.py:228-229 reads _goal_dist afresh every step); pnbr is only read
// while pdist is valid
__global__ void __launch_bounds__(256) pdist_invalidate_kernel(long long total, int N, const uint8_t* env_mask,
                                                               int32_t* pdist) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  if (env_mask && !env_mask[i / N]) return;
  pdist[i] = PD_NONE;
}

// ---- device scenario draw (mapfx_partial_draw; definition in mapfx_partial.h, restated
//      by mapfx/rng.py scen_draw) ----
// mapfx/rng.py: K_ENV, K_T, K_CELL, K_STREAM and the draw's stream ids
constexpr uint64_t SK_ENV = 0xD1B54A32D192ED03ull, SK_T = 0xABC98388FB8FAC03ull,
                   SK_CELL = 0x9E6C63D0676A9A99ull, SK_STREAM = 0xF1357AEA2E62A9C5ull;
constexpr uint32_t SS_FILE = 0x500u, SS_LINE = 0x600u;
constexpr int SCEN_LMAX = 4096;       // keys of one env: 32 KB of LDS at most
constexpr int SCEN_WAVE_LMAX = 1024;  // up to here one wavefront sorts an env's keys

struct SArgs {
  uint64_t seed;
  long long env_offset;
  const int16_t* lines;
  const int32_t* n_lines;
  int n_files, l_max;
  int32_t* init_pos;
  int32_t* goal;
  int32_t* episode;
  const uint8_t* mask;
  int32_t* err;
  int N;
};

__device__ inline uint64_t scen_key(uint64_t base, uint32_t stream, uint32_t idx) {
  return splitmix64(base ^ ((uint64_t)idx * SK_CELL) ^ ((uint64_t)stream * SK_STREAM));
}

// compare-exchange of keys[lo] / keys[hi] (lo < hi): the smaller one to lo when `up`
__device__ __forceinline__ void scen_cmpx(uint64_t* keys, int lo, int hi, bool up) {
  const uint64_t x = keys[lo], y = keys[hi];
  if ((x > y) == up) {
    keys[lo] = y;
    keys[hi] = x;
  }
}

// One workgroup of T threads per env (T = 64 while l_max <= SCEN_WAVE_LMAX, else 256): the L
// line keys (key & ~0xFFFF) | j of the env's file sit in LDS, padded with ~0 to P = the next
// power of two (8 P <= 32 KB, the only LDS of the kernel); their N smallest, ascending, end
// up in keys[0 .. N) and agent a takes the line in the low 16 bits of key a.  The keys are
// distinct and a pad (low bits 0xFFFF > any j) is above every key, so the order has no ties.
// Selection, with M = the next power of two of N (2 <= M <= P):
//   A. a bitonic sort of every chunk of M keys, even chunks ascending, odd ones descending;
//   B. while more than one chunk is left: of each pair of chunks (ascending, descending;
//      S keys apart) min(a[i], b[i]) is kept in a -- the M smallest of the 2 M, a bitonic
//      sequence -- and merged ascending / descending for the next round.  The work halves
//      with every round; no key above the M smallest of its pair is sorted again.
// M == P (N > L / 2) is the plain bitonic sort.  Every exit is uniform over the workgroup.
template <int T>
__global__ void __launch_bounds__(T) partial_draw_kernel(SArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char scen_lds[];
  uint64_t* keys = reinterpret_cast<uint64_t*>(scen_lds);
  const int e = (int)blockIdx.x, tid = (int)threadIdx.x, N = a.N;
  if (a.mask && !a.mask[e]) return;  // masked out: nothing of the env is read or written
  const int ep = a.episode[e];
  const uint64_t base = a.seed ^ ((uint64_t)(a.env_offset + e) * SK_ENV) ^ ((uint64_t)(uint32_t)ep * SK_T);
  const uint32_t f = (uint32_t)(((scen_key(base, SS_FILE, 0) >> 32) * (uint64_t)(uint32_t)a.n_files) >> 32);
  const int L = a.n_lines[f];
  if (L <= N || L > a.l_max) {  // the reference asserts len(lines) > N; (a count past the table's rows: refused too)
    if (tid == 0) atomicCAS(a.err, 0, e + 1);
    return;
  }
  int P = 2;
  while (P < L) P <<= 1;  // <= the launch's LDS: P <= next_pow2(l_max)
  for (int j = tid; j < P; j += T)
    keys[j] = j < L ? ((scen_key(base, SS_LINE, (uint32_t)j) & ~0xFFFFull) | (uint64_t)j) : ~0ull;
  __syncthreads();
  int M = 2, lm = 1;  // lm = log2 M
  while (M < N) M <<= 1, ++lm;
  for (int k = 2; k <= M; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int i = tid; i < (P >> 1); i += T) {
        const int lo = ((i & ~(j - 1)) << 1) | (i & (j - 1));  // i with a 0 inserted at bit log2 j
        scen_cmpx(keys, lo, lo | j, (lo & k) == 0);
      }
      __syncthreads();
    }
  }
  for (int S = M; S < P; S <<= 1) {  // pair p: the chunks at 2 p S (kept) and 2 p S + S
    const int pairs = P / (2 * S);
    for (int i = tid; i < pairs * M; i += T) {
      const int lo = (i >> lm) * 2 * S + (i & (M - 1));
      scen_cmpx(keys, lo, lo + S, true);
    }
    __syncthreads();
    for (int j = M >> 1; j > 0; j >>= 1) {
      for (int i = tid; i < pairs * (M >> 1); i += T) {
        const int p = i >> (lm - 1), o = i & ((M >> 1) - 1);
        const int lo = p * 2 * S + (((o & ~(j - 1)) << 1) | (o & (j - 1)));
        scen_cmpx(keys, lo, lo | j, (p & 1) == 0);
      }
      __syncthreads();
    }
  }
  const int16_t* tab = a.lines + (long long)f * a.l_max * 4;
  int32_t* ip = a.init_pos + (long long)e * N * 2;
  int32_t* gl = a.goal + (long long)e * N * 2;
  for (int ag = tid; ag < N; ag += T) {
    const int16_t* row = tab + (int)(keys[ag] & 0xFFFFull) * 4;
    ip[2 * ag] = row[0];
    ip[2 * ag + 1] = row[1];
    gl[2 * ag] = row[2];
    gl[2 * ag + 1] = row[3];
  }
  if (tid == 0) a.episode[e] = ep + 1;  // (every thread read it before the first barrier)
}

// sqrt(i), i = 0 .. n, with the same device sqrt isqrt_f64 uses (mapfx_partial_create
// compares it bit for bit with host libm before the kernels may use it)
__global__ void __launch_bounds__(256) sqrt_probe_kernel(double* out, int n) {
  const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (i <= n) out[i] = sqrt((double)i);
}

}  // namespace

struct mapfx_partial_t {
  mapfx_partial_cfg cfg;
  PGeo geo;
  PGeo geo_roll[2];  // partial_rollout_kernel's: [0] without the observation rows, [1] with (layout_rollout)
  double* bonus_lut;
  int device;
  int no_nbcarry;  // diagnostic builds (MAPFX_PARTIAL_DIAG_ENV) only: ignore the state's pnbr
  int32_t* err;    // mapfx_partial_bind_err: where the calls without a mapfx_partial_out report
  int32_t rule;    // mapfx_partial_policy_rule: MAPFX_POLICY_* of the next policy-mode launch
};

namespace {

int check_state(const mapfx_partial_t* h, const mapfx_partial_state* st) {
  if (!st) return perr(MAPFX_EINVAL, "NULL state");
  if (!st->pos || !st->goal || !st->init_pos || !st->steps || !st->at_goal || !st->done ||
      !st->goal_cost || !st->node || !st->edge || !st->t || !st->terminated || !st->total_coll ||
      !st->map_bits || !st->goal_dist)
    return perr(MAPFX_EINVAL, "mapfx_partial_state: every pointer is required");
  (void)h;
  return MAPFX_OK;
}

template <int WIN>
void (*pick_wg_apl(int apl))(PGeo, PArgs) {
  if (apl <= 1) return partial_wg_kernel<WIN, 1>;
  if (apl <= 2) return partial_wg_kernel<WIN, 2>;
  return partial_wg_kernel<WIN, 4>;
}

void (*pick_wg(int win, int apl))(PGeo, PArgs) {
  switch (win) {
    case 0: return pick_wg_apl<0>(apl);
    case 1: return pick_wg_apl<1>(apl);
    case 3: return pick_wg_apl<3>(apl);
    case 5: return pick_wg_apl<5>(apl);
    case 7: return pick_wg_apl<7>(apl);
    case 9: return pick_wg_apl<9>(apl);
  }
  return nullptr;
}

int wg_apl(const PGeo& g) { return (g.N + WG_THREADS - 1) / WG_THREADS; }

// ---- The wave kernels' instance table: the one place that names their instances. ----
// Five families share the shapes: partial_kernel (STEP, flag RUN: the runner's fused step)
// and the four rollouts (flag OBS: the observation rows are built).  A shape is a fast one,
// <WIN, 5, LF, GDE, flag> with the table width GDE (1 u8 / 2 int16 / 0 read at run time), or
// the window's generic <WIN, 0, 0, 0, true>.  Without the rows a rollout's window and K play
// no part: <0, 5, LF, GDE, false> per fast lane group, and the generic <0, 0, 0, 0, false>.
enum Family { STEP, ROLL, PIBT_ROLL, RUN_ROLL, PIBT_RUN_ROLL };

#define FAST_SHAPES(X) X(5, 16) X(5, 8) X(5, 32) X(3, 16) X(7, 16)  // (WIN, LF), at K = 5
#define GENERIC_WINDOWS(X) X(0) X(1) X(3) X(5) X(7) X(9)

// What differs per family.  gde[flag][table width] is the GDE of a fast shape's instance:
// the pibt rule has none for int32 tables (it is not offered there); the runner's rollouts
// take the generic window instance for them with the rows, and read the width at run time
// without.
constexpr int GENERIC = -1, NONE = -2;  // (NONE: nullptr)
struct FamilyTraits {
  bool flag_is_obs;  // the flag is OBS (a rollout), not RUN
  int gde[2][3];
};
constexpr FamilyTraits FAMILY[] = {  // (indexed by Family)
    /* STEP          */ {false, {{0, 1, 2}, {0, 1, 2}}},
    /* ROLL          */ {true, {{0, 1, 2}, {0, 1, 2}}},
    /* PIBT_ROLL     */ {true, {{NONE, 1, 2}, {NONE, 1, 2}}},
    /* RUN_ROLL      */ {true, {{0, 0, 0}, {GENERIC, 1, 2}}},
    /* PIBT_RUN_ROLL */ {true, {{0, 0, 0}, {GENERIC, 1, 2}}},
};
constexpr bool offers(Family f, bool flag, int gde) {
  for (int v : FAMILY[f].gde[flag])
    if (v == gde) return true;
  return false;
}

using PartialFn = void (*)(PGeo, PArgs);
using RolloutFn = void (*)(PGeo, PArgs, RArgs);
using RunRollFn = void (*)(PGeo, PArgs, RArgs, RRun);
template <Family F>
using FnOf = std::conditional_t<F == STEP, PartialFn,
                                std::conditional_t<F == ROLL || F == PIBT_ROLL, RolloutFn, RunRollFn>>;

template <Family F, int WIN, int KF, int LF, int GDE, bool FLAG>
FnOf<F> inst() {
  if constexpr (F == STEP) return partial_kernel<WIN, KF, LF, GDE, FLAG>;
  else if constexpr (F == ROLL) return partial_rollout_kernel<WIN, KF, LF, GDE, FLAG>;
  else if constexpr (F == PIBT_ROLL) return partial_pibt_rollout_kernel<WIN, KF, LF, GDE, FLAG>;
  else if constexpr (F == RUN_ROLL) return partial_runner_rollout_kernel<WIN, KF, LF, GDE, FLAG>;
  else return partial_pibt_runner_rollout_kernel<WIN, KF, LF, GDE, FLAG>;
}

// the fast shape's instance at table width tw (only the GDEs the family offers exist)
template <Family F, int WIN, int LF, bool FLAG>
FnOf<F> fast_inst(int tw) {
  const int gde = FAMILY[F].gde[FLAG][tw];
  if constexpr (offers(F, FLAG, 0))
    if (gde == 0) return inst<F, WIN, 5, LF, 0, FLAG>();
  if constexpr (offers(F, FLAG, 1))
    if (gde == 1) return inst<F, WIN, 5, LF, 1, FLAG>();
  if constexpr (offers(F, FLAG, 2))
    if (gde == 2) return inst<F, WIN, 5, LF, 2, FLAG>();
  return nullptr;
}

template <Family F, bool FLAG>
FnOf<F> pick_flag(int win, int K, int L, int tw) {
  // (a rollout without the rows: any window and K, and a lane group that several pairs name
  // is the same instance each time)
  constexpr bool windowed = FLAG || !FAMILY[F].flag_is_obs;
  if (FAMILY[F].gde[FLAG][tw] != GENERIC) {
#define X(WIN, LF) \
  if (L == LF && (!windowed || (K == 5 && win == WIN))) return fast_inst<F, windowed ? WIN : 0, LF, FLAG>(tw);
    FAST_SHAPES(X)
#undef X
  }
  if constexpr (!windowed) {
    return inst<F, 0, 0, 0, 0, false>();
  } else {
    switch (win) {
#define X(WIN) \
  case WIN: return inst<F, WIN, 0, 0, 0, true>();
      GENERIC_WINDOWS(X)
#undef X
    }
    return nullptr;  // no instance has this window
  }
}

// The instance of family F for a configuration's window, K, lane group and table width.
template <Family F>
FnOf<F> pick(int win, int K, int L, int tw, bool flag) {
  return flag ? pick_flag<F, true>(win, K, L, tw) : pick_flag<F, false>(win, K, L, tw);
}

// every partial_kernel instance: the table walked (mapfx_partial_create raises their
// dynamic-LDS limit)
template <typename Fn>
void each_step_inst(Fn f) {
#define X(WIN, LF)               \
  for (int tw = 0; tw < 3; ++tw) \
    for (int run = 0; run < 2; ++run) f(pick<STEP>(WIN, 5, LF, tw, run != 0));
  FAST_SHAPES(X)
#undef X
#define X(WIN) f(pick<STEP>(WIN, 0, 0, 0, true));
  GENERIC_WINDOWS(X)
#undef X
}

int table_width(const PGeo& g) { return g.gd8 ? 1 : g.gd32 ? 0 : 2; }
// a handle's rollout instance under policy rule `rule` (MAPFX_POLICY_PIBT has kernels of its own)
RolloutFn pick_roll(const PGeo& g, int rule, bool obs) {
  return rule == MAPFX_POLICY_PIBT ? pick<PIBT_ROLL>(g.win, g.K, g.L, table_width(g), obs)
                                   : pick<ROLL>(g.win, g.K, g.L, table_width(g), obs);
}
RunRollFn pick_run_roll(const PGeo& g, int rule, bool obs) {
  return rule == MAPFX_POLICY_PIBT ? pick<PIBT_RUN_ROLL>(g.win, g.K, g.L, table_width(g), obs)
                                   : pick<RUN_ROLL>(g.win, g.K, g.L, table_width(g), obs);
}

// the wave kernels (one wave per env group: N <= 64, sides <= 256), and those with u8 / int16
// goal tables, which is where the on-device policy and its pibt rule are offered
bool wave_path(const PGeo& g) { return !g.big; }
bool wave_path_small_tables(const PGeo& g) { return !g.big && !g.gd32; }
// the refusal outside wave_path_small_tables(): "<who> needs ..."
int refuse_small_tables(const char* who) {
  char msg[256];
  snprintf(msg, sizeof msg,
           "%s needs the wave kernel (N <= 64, sides <= 256) and u8 / int16 goal tables (H * W <= 32767)", who);
  return perr(MAPFX_EINVAL, msg);
}

// The fast observation path's staging images (one env's rows + 16 bytes of alignment slack
// each) for a group of 64 lanes (the whole wave) or 32 (each half in turn); the whole wave
// while the block stays within 40 KB (4 blocks per CU).  `off` is the first free offset; the
// images alias dep onwards (`alias`) or start at `off`.  Sets off_stage and stage_lanes and
// returns the new first free offset (`off` when there are no images).
int place_stage(PGeo& g, int off, bool alias) {
  g.off_stage = -1;
  g.stage_lanes = 0;
  if (g.K == 5 && (g.win == 3 || g.win == 5 || g.win == 7) && g.L >= 8 && g.L <= 32) {
    for (int G : {64, 32}) {
      const int st = std::min(g.EPW, G / g.L) * g.stage_env_bytes;
      const int need = alias ? std::max(off, g.off_dep + st) : off + st;
      if (need <= (G == 64 ? 40 * 1024 : 64 * 1024)) {
        g.off_stage = alias ? g.off_dep : off;
        g.stage_lanes = G;
        return need;
      }
    }
  }
  return off;
}

// The rollout's layout of a wave-kernel configuration: layout()'s regions, with the staging
// images BEHIND them instead of over the dep map onwards -- a loop of steps reads bit 7 of
// every dep byte (the obstacle flag) and the sqrt table again after the rows have left.
// Without the rows (obs false) there is no staging and no sqrt table.
void layout_rollout(const PGeo& base, bool obs, PGeo& g) {
  g = base;
  int off = g.off_rew + g.EPW * g.rew_env_bytes;
  if (obs && g.off_sqrt >= 0) off = g.off_sqrt + round_up((g.sq_max + 1) * 4, 16);
  if (obs) {
    off = place_stage(g, off, false);
  } else {
    g.off_sqrt = g.off_stage = -1;
    g.stage_lanes = 0;
  }
  g.lds = round_up(off, 16);
  g.wpb = PARTIAL_MAX_WPB;
  while (g.wpb > 1 && g.wpb * g.lds > 160 * 1024) --g.wpb;
}

int launch(mapfx_partial_t* h, PArgs& a, void* stream) {
  const PGeo& g = h->geo;
  if (g.E == 0) return MAPFX_OK;
  a.bonus_lut = h->bonus_lut;
  if (h->no_nbcarry) a.pnbr = nullptr;
  // the runner's fused step, or observation rows to an EpisodeBatch time row
  const bool run = a.ra.act_row != nullptr || a.ra.alive != nullptr || a.obs_rows != nullptr;
  // N > 64 or a side > 256: one workgroup per env, map in HBM
  const PartialFn fn = g.big ? pick_wg(g.win, wg_apl(g)) : pick<STEP>(g.win, g.K, g.L, table_width(g), run);
  if (!fn) return perr(MAPFX_EINVAL, "obs_window must be one of 0, 1, 3, 5, 7, 9");
  if (g.big)
    return launch_kernel(fn, dim3(g.E), dim3(WG_THREADS), g.wg_lds, (hipStream_t)stream, nullptr, nullptr,
                         "partial_wg_kernel launch", NOTED, g, a);
  const int blocks = (g.E + g.EPW - 1) / g.EPW;
  // (+ one workgroup for the runner's fused compaction, partial_kernel's first block)
  const int nblk = (blocks + g.wpb - 1) / g.wpb + (run && a.ra.cmp_bs ? 1 : 0);
  return launch_kernel(fn, dim3(nblk), dim3(64 * g.wpb), g.lds * g.wpb, (hipStream_t)stream, nullptr, nullptr,
                       "partial_kernel launch", NOTED, g, a);
}

void fill_state(PArgs& a, const mapfx_partial_state* st) {
  a.pos = st->pos;
  a.goal = st->goal;
  a.init_pos = st->init_pos;
  a.steps = st->steps;
  a.at_goal = st->at_goal;
  a.done = st->done;
  a.goal_cost = st->goal_cost;
  a.node = st->node;
  a.edge = st->edge;
  a.t = st->t;
  a.terminated = st->terminated;
  a.total_coll = st->total_coll;
  a.bits = st->map_bits;
  a.gd = st->goal_dist;
  a.pdist = st->pdist;
  a.pnbr = st->pnbr;
}

void fill_out(PArgs& a, const mapfx_partial_out* o) {
  if (!o) return;
  a.reward = o->reward;
  a.obs = o->obs;
  a.state = o->state;
  a.avail = o->avail;
  a.err = o->err;
}

// Where every entry point that launches the env kernels starts: the handle and the state
// checked, `a` cleared and filled from the state and the outputs (out may be NULL).
int begin(const mapfx_partial_t* h, const mapfx_partial_state* st, const mapfx_partial_out* out, PArgs& a) {
  if (!h) return perr(MAPFX_EINVAL, "NULL handle");
  if (int rc = check_state(h, st)) return rc;
  memset(&a, 0, sizeof(a));
  fill_state(a, st);
  fill_out(a, out);
  return MAPFX_OK;
}

// The one step: mapfx_partial_step, and with `ra` the runner's fused step.  obs_rows not
// NULL: the observation rows go to an EpisodeBatch time row (obs_rows + e * obs_env_stride
// floats, envs with obs_mask[e] != 0) instead of out->obs.
int step(mapfx_partial_t* h, const mapfx_partial_state* st, const void* actions, int action_dtype,
         const mapfx_runner_acts* ra, const mapfx_partial_out* out, float* obs_rows, long long obs_env_stride,
         const uint8_t* obs_mask, void* stream) {
  PArgs a;
  if (int rc = begin(h, st, out, a)) return rc;
  if (!actions || (ra && !ra->act_row))
    return perr(MAPFX_EINVAL, ra ? "NULL actions / rows map" : "NULL actions");
  if (action_dtype < MAPFX_I8 || action_dtype > MAPFX_I64) return perr(MAPFX_EINVAL, "bad action_dtype");
  if (obs_rows) {
    a.obs = nullptr;
    a.obs_rows = obs_rows;
    a.obs_env_stride = obs_env_stride;
    a.obs_mask = obs_mask;
  }
  a.actions = actions;
  a.act_dtype = action_dtype;
  if (ra) a.ra = *ra;
  a.do_step = 1;
  return launch(h, a, stream);
}

// ---- what the two fused rollouts (mapfx_partial_rollout's wave path, mapfx_partial_rollout_runner)
// share; `who` is the public call their messages name ----
// actions or a policy, and the policy only where it is offered
int check_policy(const mapfx_partial_t* h, const char* who, const void* actions, const mapfx_partial_policy* pol) {
  char msg[96];
  if (!actions && !pol) {
    snprintf(msg, sizeof msg, "%s: actions or a policy is required", who);
    return perr(MAPFX_EINVAL, msg);
  }
  if (actions || wave_path_small_tables(h->geo)) return MAPFX_OK;
  snprintf(msg, sizeof msg, "%s: the on-device policy", who);
  return refuse_small_tables(msg);
}

// the wave launch's arguments on top of begin()'s `a`; without actions the policy `pol` acts
void fused_args(const mapfx_partial_t* h, const mapfx_partial_state* st, int32_t T, const void* actions,
                int action_dtype, const mapfx_partial_policy* pol, PArgs& a, RArgs& ro) {
  const bool policy = actions == nullptr;
  a.bonus_lut = h->bonus_lut;
  if (h->no_nbcarry) a.pnbr = nullptr;
  // policy mode: the prologue's unconditional action load reads the positions instead
  a.actions = policy ? (const void*)st->pos : actions;
  a.act_dtype = policy ? MAPFX_I8 : action_dtype;
  a.do_step = 1;
  memset(&ro, 0, sizeof(ro));
  ro.T = T;
  ro.policy = policy ? 1 : 0;
  if (policy) {
    ro.t0 = pol->t0;
    ro.seed = pol->seed;
    ro.eps_q = pol->eps_q;
  }
  ro.env_offset = (long long)h->cfg.env_offset;
}

// the launch of instance `fn` over the rollout's layout with or without the rows (`more`:
// the family's arguments after PGeo and PArgs)
template <typename... P, typename... A>
int launch_fused(const mapfx_partial_t* h, void (*fn)(P...), bool obs, void* stream, const char* what,
                 const PArgs& a, const A&... more) {
  if (!fn) return perr(MAPFX_EINVAL, "obs_window must be one of 0, 1, 3, 5, 7, 9");
  const PGeo& gr = h->geo_roll[obs ? 1 : 0];
  const int waves = (h->geo.E + gr.EPW - 1) / gr.EPW;
  return launch_kernel(fn, dim3((waves + gr.wpb - 1) / gr.wpb), dim3(64 * gr.wpb), gr.lds * gr.wpb,
                       (hipStream_t)stream, nullptr, nullptr, what, NOTED, gr, a, more...);
}

int raise_lds(const void* fn, int bytes, const char* what) {
  return check_hip(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, bytes), what);
}

// the goal-distance BFS instance `fn` (tables of DT), recorded for mapfx_last_kernel
template <typename DT>
int launch_bfs(void (*fn)(PGeo, const uint8_t*, const int32_t*, const uint8_t*, DT*), int threads, int lds,
               const PGeo& g, const mapfx_partial_state* st, const uint8_t* env_mask, hipStream_t sm) {
  return launch_kernel(fn, dim3((unsigned)(g.E * g.N)), dim3(threads), lds, sm, nullptr, nullptr,
                       "partial_bfs_kernel launch", NOTED, g, st->map_bits, st->goal, env_mask, (DT*)st->goal_dist);
}

// The launch geometry and LDS layout of a validated configuration: a plain function of the
// configuration (no HIP call).  Returns the refusal's message, nullptr when there is none.
const char* layout(const mapfx_partial_cfg& c, PGeo& g) {
  memset(&g, 0, sizeof(g));
  g.H = c.H;
  g.W = c.W;
  g.N = c.n_agents;
  g.E = c.n_envs;
  int L = 1;
  while (L < g.N) L <<= 1;
  g.L = L;
  while ((1 << g.lshift) < L) ++g.lshift;
  g.win = c.obs_window;
  g.K = c.obs_knn_agents;
  g.D = 2 * c.obs_window * c.obs_window + NF * c.obs_knn_agents;
  g.limit = c.episode_limit;
  g.hw = c.H * c.W;
  g.P = std::max(1, c.obs_window / 2);
  g.pl = round_up(g.P, 4);
  g.pitch = round_up(g.pl + c.W + g.P, 4);
  g.rows = c.H + 2 * g.P;
  g.wpr = g.pitch / 4;
  g.m_wpr = (uint32_t)((0x100000000ull + (unsigned long long)g.wpr - 1ull) / (unsigned long long)g.wpr);
  g.bits_words = (c.H * c.W + 31) / 32;
  g.map_shared = c.map_shared ? 1 : 0;
  g.map_stride = mapfx_map_stride(c.H, c.W);
  g.map_env_bytes = round_up(g.rows * g.pitch, 16);
  g.bits_env_bytes = round_up(g.bits_words * 4 + 4, 16);
  g.feat_env_bytes = round_up(L * FR * 4, 16);  // (L lanes per env)
  g.pos_env_bytes = round_up(L * 8, 16);
  g.rew_env_bytes = round_up(L * 8, 16);
  g.gd32 = (long long)c.H * c.W > 32767 ? 1 : 0;  // a path is shorter than H * W cells
  g.gd8 = (long long)c.H * c.W <= 255 ? 1 : 0;
  g.big = (g.N > 64 || c.H > 256 || c.W > 256) ? 1 : 0;
  g.hs_log = 8;
  while ((1 << g.hs_log) < 4 * g.N) ++g.hs_log;
  g.wg_lds = (1 << g.hs_log) * 8 + g.N * (4 + 4 + 8 + FR * 4) + 16 + g.N * 8 + 8 * 4;
  g.huge_lds = (c.H > 256 || c.W > 256) ? c.H * ((c.W + 63) / 64) * 8 : 0;
  g.move_rew = c.move_reward;
  g.stay_rew = c.stay_reward;
  g.stay_goal_rew = c.stay_goal_reward;
  g.nc_rew = c.node_collide_reward;
  g.ec_rew = c.edge_collide_reward;
  g.env_rew = c.env_collide_reward;
  // the LUT sizes: sqrt(0 .. sq_max), the completion bonus at t = 0 .. bonus_len - 1
  const int S = std::max(c.H, c.W);
  g.sq_max = 2 * (S - 1) * (S - 1);
  g.bonus_len = c.episode_limit + BONUS_EXTRA;
  const int per_env = 2 * g.map_env_bytes + g.bits_env_bytes + g.feat_env_bytes + g.pos_env_bytes +
                      g.rew_env_bytes;
  // envs per wave: as many as fit 64 KB of LDS; one env may take up to the CU's
  // 160 KB (maps up to 256 x 256), with the dynamic-LDS limit raised by mapfx_partial_create
  // (the workgroup path keeps no map in LDS)
  int EPW = g.big ? 1 : 64 / L;
  while (EPW > 1 && EPW * per_env > 64 * 1024) --EPW;
#ifdef MAPFX_PARTIAL_DIAG_ENV
  if (const char* ev = getenv("MAPFX_PARTIAL_EPW")) {  // diagnostic / A-B: fewer envs per wave
    const int v = atoi(ev);
    if (v >= 1 && v < EPW) EPW = v;
  }
#endif
  if (!g.big && EPW * per_env > 160 * 1024) return "one env needs more than 160 KB of LDS (map too large)";
  g.EPW = EPW;
  int off = 0;
  g.off_map = off; off += EPW * g.map_env_bytes;
  g.off_dep = off; off += EPW * g.map_env_bytes;
  g.off_bits = off; off += EPW * g.bits_env_bytes;
  g.off_feat = off; off += EPW * g.feat_env_bytes;
  g.off_pos = off; off += EPW * g.pos_env_bytes;
  g.off_rew = off; off += EPW * g.rew_env_bytes;
  // the K-nearest rows' distances sqrt(0 .. sq_max) as float32, one table per wave filled
  // while the state loads are in flight (small maps: sq_max < 512, i.e. sides up to 16)
  g.off_sqrt = -1;
  if (g.sq_max < 512) {
    g.off_sqrt = off;
    off += round_up((g.sq_max + 1) * 4, 16);
  }
  g.stage_env_bytes = round_up(L * g.D * 4 + 16, 16);
  off = place_stage(g, off, true);  // (the step's images alias dep onwards)
  g.lds = round_up(off, 16);
  // waves per block: up to PARTIAL_MAX_WPB while the block's LDS fits the CU
  g.wpb = 1;
  if (!g.big) {
    g.wpb = PARTIAL_MAX_WPB;
#ifdef MAPFX_PARTIAL_DIAG_ENV
    if (const char* ev = getenv("MAPFX_PARTIAL_WPB")) {  // diagnostic / A-B
      const int v = atoi(ev);
      if (v >= 1 && v <= PARTIAL_MAX_WPB) g.wpb = v;
    }
#endif
    while (g.wpb > 1 && g.wpb * g.lds > 160 * 1024) --g.wpb;
  }
  return nullptr;
}

}  // namespace

extern "C" {

int mapfx_partial_create(const mapfx_partial_cfg* cfg, mapfx_partial_t** out) {
  if (!cfg || !out) return perr(MAPFX_EINVAL, "NULL argument");
  *out = nullptr;
  const mapfx_partial_cfg& c = *cfg;
  if (c.H < 1 || c.W < 1 || c.H > HUGE_THREADS * 2 || c.W > 64 * HUGE_WORDS)
    return perr(MAPFX_EINVAL, "MARL_PARTIAL path supports 1 <= H <= 1024, 1 <= W <= 1536");
  if (c.n_agents < 1 || c.n_agents > 4 * WG_THREADS) return perr(MAPFX_EINVAL, "n_agents must be in 1..1024");
  if (c.n_envs < 0) return perr(MAPFX_EINVAL, "n_envs < 0");
  if (c.episode_limit < 1) return perr(MAPFX_EINVAL, "episode_limit must be >= 1");
  if (c.obs_knn_agents < 1) return perr(MAPFX_EINVAL, "obs_knn_agents must be >= 1");
  if (c.obs_window < 0 || c.obs_window > 9 || (c.obs_window > 0 && !(c.obs_window & 1)))
    return perr(MAPFX_EINVAL, "obs_window must be 0 or odd <= 9");
  std::unique_ptr<mapfx_partial_t, void (*)(mapfx_partial_t*)> h(new (std::nothrow) mapfx_partial_t(),
                                                                 mapfx_partial_destroy);
  if (!h) return perr(MAPFX_ENOMEM, "host allocation failed");
  h->cfg = c;
#ifdef MAPFX_PARTIAL_DIAG_ENV  // A/B knobs read from the environment: diagnostic builds only
  if (const char* ev = getenv("MAPFX_PARTIAL_NBCARRY")) h->no_nbcarry = atoi(ev) == 0;
#endif
  if (hipGetDevice(&h->device) != hipSuccess) h->device = 0;
  PGeo& g = h->geo;
  if (const char* msg = layout(c, g)) return perr(MAPFX_EINVAL, msg);
  const void* huge_bfs = g.gd32 ? (const void*)partial_bfs_huge_kernel<int32_t>
                                : (const void*)partial_bfs_huge_kernel<int16_t>;
  if (g.big && g.huge_lds > 0) {
    // the frontier rows plus the kernel's own static LDS (__syncthreads_or's scratch)
    hipFuncAttributes fa;
    memset(&fa, 0, sizeof fa);
    (void)hipFuncGetAttributes(&fa, huge_bfs);
    if (g.huge_lds + (int)fa.sharedSizeBytes > 160 * 1024) {
      char msg[240];
      snprintf(msg, sizeof msg,
               "MARL_PARTIAL: the %d x %d map's BFS frontier needs H * ceil(W / 64) * 8 = %d B of "
               "LDS (+ %d B static; the CU has 160 KB: H * ceil(W / 64) must stay below ~20470)",
               c.H, c.W, g.huge_lds, (int)fa.sharedSizeBytes);
      return perr(MAPFX_EINVAL, msg);
    }
  }
  if (g.big && g.wg_lds > 160 * 1024)
    return perr(MAPFX_EINVAL, "MARL_PARTIAL: the workgroup path needs more than 160 KB of LDS");
  // device resources: dynamic-LDS limits above 64 KB, then the LUT and the sqrt check
  int rc = MAPFX_OK;
  if (g.big) {
    if (g.wg_lds > 64 * 1024)
      rc = raise_lds((const void*)pick_wg(g.win, wg_apl(g)), g.wg_lds, "hipFuncSetAttribute(partial_wg_kernel LDS)");
    if (!rc && g.huge_lds > 64 * 1024 &&
        hipFuncSetAttribute(huge_bfs, hipFuncAttributeMaxDynamicSharedMemorySize, g.huge_lds) != hipSuccess) {
      (void)hipGetLastError();
      char msg[200];
      snprintf(msg, sizeof msg,
               "MARL_PARTIAL: the %d x %d map's BFS frontier (H * ceil(W / 64) * 8 = %d B) exceeds "
               "the LDS a workgroup may allocate", c.H, c.W, g.huge_lds);
      rc = perr(MAPFX_EINVAL, msg);
    }
  } else if (g.lds * g.wpb > 64 * 1024) {
    each_step_inst([&](PartialFn fn) {
      if (!rc) rc = raise_lds((const void*)fn, g.lds * g.wpb, "hipFuncSetAttribute(partial_kernel LDS)");
    });
  }
  if (!g.big) {  // the rollout's two layouts and this configuration's two instances
    for (int i = 0; i < 4 && !rc; ++i) {  // (i >> 1: the policy rule, pibt where it is offered)
      const int obs = i & 1, rule = i >> 1;
      if (rule != MAPFX_POLICY_DESCENT && g.gd32) break;
      PGeo& gr = h->geo_roll[obs];
      if (rule == MAPFX_POLICY_DESCENT) layout_rollout(g, obs != 0, gr);
      if (gr.lds * gr.wpb <= 64 * 1024) continue;
      const RolloutFn fn = pick_roll(g, rule, obs != 0);
      if (fn) rc = raise_lds((const void*)fn, gr.lds * gr.wpb, "hipFuncSetAttribute(partial_rollout_kernel LDS)");
      const RunRollFn rfn = pick_run_roll(g, rule, obs != 0);
      if (!rc && rfn)
        rc = raise_lds((const void*)rfn, gr.lds * gr.wpb, "hipFuncSetAttribute(partial_runner_rollout_kernel LDS)");
    }
  }
  if (rc) return rc;
  {  // the map build's multiply-high division (partial_kernel) must be exact on its range
    const unsigned long long nw = (unsigned long long)g.rows * g.wpr;
    for (unsigned long long wi = 0; wi < nw; ++wi)
      if (((wi * g.m_wpr) >> 32) != wi / (unsigned long long)g.wpr)
        return perr(MAPFX_EINVAL, "MARL_PARTIAL: map too large for the padded-map word index");
  }
  // the completion-bonus LUT from host libm (float ** int is correctly rounded there) and
  // the sqrt reference values the device sqrt is checked against
  const size_t nsq = (size_t)g.sq_max + 1;
  const std::unique_ptr<double[]> sq(new (std::nothrow) double[nsq]), bo(new (std::nothrow) double[g.bonus_len]),
      back(new (std::nothrow) double[nsq]);
  if (!sq || !bo || !back) return perr(MAPFX_ENOMEM, "host allocation failed");
  double (*volatile libm_sqrt)(double) = sqrt;
  double (*volatile libm_pow)(double, double) = pow;
  for (int i = 0; i <= g.sq_max; ++i) sq[i] = libm_sqrt((double)i);
  for (int t = 0; t < g.bonus_len; ++t)  // (complete / (gamma ** (limit - t))) * fac  (:292)
    bo[t] = (c.complete_reward / libm_pow(c.gamma, (double)(c.episode_limit - t))) * c.complete_fac;
  rc = check_hip(hipMalloc(&h->bonus_lut, sizeof(double) * g.bonus_len), "hipMalloc");
  if (!rc) rc = check_hip(hipMemcpy(h->bonus_lut, bo.get(), sizeof(double) * g.bonus_len, hipMemcpyHostToDevice), "hipMemcpy");
  // the kernels' sqrt (isqrt_f64) must equal host libm on every argument they can use
  double* probe = nullptr;
  if (!rc) rc = check_hip(hipMalloc(&probe, sizeof(double) * nsq), "hipMalloc");
  if (!rc)
    rc = launch_kernel(sqrt_probe_kernel, dim3((unsigned)(g.sq_max / 256 + 1)), dim3(256), 0, nullptr, nullptr,
                       nullptr, "sqrt_probe_kernel launch", QUIET, probe, g.sq_max);
  if (!rc) rc = check_hip(hipMemcpy(back.get(), probe, sizeof(double) * nsq, hipMemcpyDeviceToHost), "hipMemcpy");
  if (!rc && memcmp(back.get(), sq.get(), sizeof(double) * nsq) != 0)
    rc = perr(MAPFX_EINVAL, "MARL_PARTIAL: the device fp64 sqrt differs from host libm (observations would not match)");
  if (probe) (void)hipFree(probe);
  if (rc) return rc;
  *out = h.release();
  return MAPFX_OK;
}

void mapfx_partial_destroy(mapfx_partial_t* h) {
  if (!h) return;
  if (h->bonus_lut) (void)hipFree(h->bonus_lut);
  delete h;
}

int32_t mapfx_partial_obs_dim(const mapfx_partial_t* h) { return h ? h->geo.D : -1; }

int32_t mapfx_partial_goal_dist_elem_size(int32_t H, int32_t W) {
  const long long hw = (long long)H * W;
  return hw <= 255 ? 1 : hw > 32767 ? 4 : 2;
}

int mapfx_partial_goal_dist(mapfx_partial_t* h, const mapfx_partial_state* st,
                            const uint8_t* env_mask, void* stream) {
  if (!h) return perr(MAPFX_EINVAL, "NULL handle");
  int rc = check_state(h, st);
  if (rc) return rc;
  const PGeo& g = h->geo;
  if ((long long)g.E * g.N == 0) return MAPFX_OK;
  const hipStream_t sm = (hipStream_t)stream;
  if (g.huge_lds)
    rc = g.gd32 ? launch_bfs(partial_bfs_huge_kernel<int32_t>, HUGE_THREADS, g.huge_lds, g, st, env_mask, sm)
                : launch_bfs(partial_bfs_huge_kernel<int16_t>, HUGE_THREADS, g.huge_lds, g, st, env_mask, sm);
  else if (g.H <= 64 && g.W <= 64)
    rc = g.gd8 ? launch_bfs(partial_bfs_kernel<uint8_t>, 64, 0, g, st, env_mask, sm)
               : launch_bfs(partial_bfs_kernel<int16_t>, 64, 0, g, st, env_mask, sm);
  else
    rc = g.gd32  ? launch_bfs(partial_bfs_big_kernel<int32_t>, 256, 0, g, st, env_mask, sm)
         : g.gd8 ? launch_bfs(partial_bfs_big_kernel<uint8_t>, 256, 0, g, st, env_mask, sm)
                 : launch_bfs(partial_bfs_big_kernel<int16_t>, 256, 0, g, st, env_mask, sm);
  if (rc || !st->pdist) return rc;
  const long long total = (long long)g.E * g.N;  // (QUIET: the recorded kernel stays the BFS instance)
  return launch_kernel(pdist_invalidate_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, sm, nullptr,
                       nullptr, "pdist_invalidate_kernel launch", QUIET, total, g.N, env_mask, st->pdist);
}

int mapfx_partial_draw(mapfx_partial_t* h, const mapfx_partial_scen* sc, void* stream) {
  if (!h) return perr(MAPFX_EINVAL, "NULL handle");
  if (!sc) return perr(MAPFX_EINVAL, "NULL mapfx_partial_scen");
  if (!sc->lines || !sc->n_lines || !sc->init_pos || !sc->goal || !sc->episode || !sc->err)
    return perr(MAPFX_EINVAL, "mapfx_partial_scen: lines, n_lines, init_pos, goal, episode and err are required");
  if (sc->n_files < 1) return perr(MAPFX_EINVAL, "mapfx_partial_scen: n_files must be >= 1");
  if (sc->l_max < 1 || sc->l_max > SCEN_LMAX)
    return perr(MAPFX_EINVAL, "mapfx_partial_scen: l_max must be in 1..4096");
  const PGeo& g = h->geo;
  if (g.E == 0) return MAPFX_OK;
  SArgs a;
  memset(&a, 0, sizeof(a));
  a.seed = sc->seed;
  a.env_offset = (long long)h->cfg.env_offset;
  a.lines = sc->lines;
  a.n_lines = sc->n_lines;
  a.n_files = sc->n_files;
  a.l_max = sc->l_max;
  a.init_pos = sc->init_pos;
  a.goal = sc->goal;
  a.episode = sc->episode;
  a.mask = sc->mask;
  a.err = sc->err;
  a.N = g.N;
  unsigned P = 2;
  while (P < (unsigned)sc->l_max) P <<= 1;
  const hipStream_t sm = (hipStream_t)stream;
  const bool wave = sc->l_max <= SCEN_WAVE_LMAX;
  return launch_kernel(wave ? partial_draw_kernel<64> : partial_draw_kernel<256>, dim3((unsigned)g.E),
                       dim3(wave ? 64 : 256), P * 8u, sm, nullptr, nullptr, "partial_draw_kernel launch", NOTED, a);
}

int mapfx_partial_reset(mapfx_partial_t* h, const mapfx_partial_state* st, const uint8_t* env_mask,
                        const mapfx_partial_out* out, void* stream) {
  PArgs a;
  if (int rc = begin(h, st, out, a)) return rc;
  a.reward = nullptr;
  a.do_reset = 1;
  a.reset_mask = env_mask;
  return launch(h, a, stream);
}

int mapfx_partial_step(mapfx_partial_t* h, const mapfx_partial_state* st, const void* actions,
                       int action_dtype, const mapfx_partial_out* out, void* stream) {
  return step(h, st, actions, action_dtype, nullptr, out, nullptr, 0, nullptr, stream);
}

int mapfx_partial_fuses_post(const mapfx_partial_t* h) { return h && wave_path(h->geo) ? 1 : 0; }

// the runner's fused step (runner.hip), internal.h
int mapfx_partial_step_runner(mapfx_partial_t* h, const mapfx_partial_state* st, const void* actions,
                              int action_dtype, const mapfx_runner_acts* ra, const mapfx_partial_out* out,
                              float* obs_rows, long long obs_env_stride, const uint8_t* obs_mask,
                              void* stream) {
  static const mapfx_runner_acts no_rows_map = {};  // (ra NULL is refused like its act_row NULL)
  return step(h, st, actions, action_dtype, ra ? ra : &no_rows_map, out, obs_rows, obs_env_stride, obs_mask, stream);
}

int mapfx_partial_observe(mapfx_partial_t* h, const mapfx_partial_state* st,
                          const mapfx_partial_out* out, void* stream) {
  PArgs a;
  if (int rc = begin(h, st, out, a)) return rc;
  a.reward = nullptr;
  return launch(h, a, stream);
}

int mapfx_partial_rollout_fused(const mapfx_partial_t* h) { return h && wave_path(h->geo) ? 1 : 0; }

// internal.h: what repair.hip needs of a handle
int mapfx_partial_shape_of(const mapfx_partial_t* h, mapfx_partial_shape* s) {
  if (!h || !s) return perr(MAPFX_EINVAL, "NULL handle");
  const PGeo& g = h->geo;
  *s = mapfx_partial_shape{g.H, g.W, g.N, g.E, g.map_shared, g.big, g.map_stride, (long long)h->cfg.env_offset};
  return MAPFX_OK;
}
int mapfx_partial_check_state(const mapfx_partial_t* h, const mapfx_partial_state* st) { return check_state(h, st); }

int mapfx_partial_rollout(mapfx_partial_t* h, const mapfx_partial_state* st, int32_t T, const void* actions,
                          int action_dtype, const mapfx_partial_policy* pol, int32_t autoreset,
                          const mapfx_partial_traj* traj, void* stream) {
  PArgs a;
  int rc = begin(h, st, nullptr, a);
  if (rc) return rc;
  if (T < 1 || T > 65536) return perr(MAPFX_EINVAL, "mapfx_partial_rollout: T must be in 1..65536");
  if (action_dtype < MAPFX_I8 || action_dtype > MAPFX_I64) return perr(MAPFX_EINVAL, "bad action_dtype");
  if ((rc = check_policy(h, "mapfx_partial_rollout", actions, pol))) return rc;
  const PGeo& g = h->geo;
  if (g.E == 0) return MAPFX_OK;
  const mapfx_partial_traj none = {};
  const mapfx_partial_traj& tj = traj ? *traj : none;
  const long long EN = (long long)g.E * g.N;
  a.act_dtype = action_dtype;
  a.do_step = 1;
  a.err = tj.err;
  if (g.big) {
    // the workgroup path: T step launches with the slot pointers advanced (and the masked
    // reset before each when autoreset), the post-step positions and flags copied to
    // their slots -- the same result, one launch floor per step
    const hipStream_t sm = (hipStream_t)stream;
    const size_t esz = action_dtype == MAPFX_I64 ? 8 : action_dtype == MAPFX_I32 ? 4 : 1;
    for (int k = 0; k < T && !rc; ++k) {
      if (autoreset) {
        PArgs r = a;
        r.do_step = 0;
        r.do_reset = 1;
        r.reset_mask = st->terminated;
        r.err = nullptr;
        rc = launch(h, r, stream);
        if (rc) break;
      }
      PArgs s = a;
      s.actions = (const char*)actions + (size_t)k * EN * esz;
      s.reward = tj.reward ? tj.reward + (long long)k * g.E : nullptr;
      s.obs = tj.obs ? tj.obs + k * EN * g.D : nullptr;
      s.state = tj.state ? tj.state + 3ll * k * g.E : nullptr;
      s.avail = tj.avail ? tj.avail + k * EN : nullptr;
      rc = launch(h, s, stream);
      if (!rc && tj.pos)
        rc = check_hip(hipMemcpyAsync(tj.pos + k * EN * 2, st->pos, sizeof(int32_t) * 2 * EN,
                                      hipMemcpyDeviceToDevice, sm), "hipMemcpyAsync(traj pos)");
      if (!rc && tj.terminated)
        rc = check_hip(hipMemcpyAsync(tj.terminated + (long long)k * g.E, st->terminated, (size_t)g.E,
                                      hipMemcpyDeviceToDevice, sm), "hipMemcpyAsync(traj terminated)");
    }
    return rc;
  }
  RArgs ro;
  fused_args(h, st, T, actions, action_dtype, pol, a, ro);
  a.reward = tj.reward;
  a.obs = tj.obs;
  a.state = tj.state;
  a.avail = tj.avail;
  ro.autoreset = autoreset ? 1 : 0;
  if (ro.policy) ro.actions = tj.actions;
  ro.pos = tj.pos;
  ro.terminated = tj.terminated;
  const bool obs = tj.obs != nullptr;
  return launch_fused(h, pick_roll(g, ro.policy ? h->rule : MAPFX_POLICY_DESCENT, obs), obs, stream,
                      "partial_rollout_kernel launch", a, ro);
}

int mapfx_partial_bind_err(mapfx_partial_t* h, int32_t* err) {
  if (!h) return perr(MAPFX_EINVAL, "NULL handle");
  h->err = err;
  return MAPFX_OK;
}

int mapfx_partial_policy_rule_offered(const mapfx_partial_t* h, int32_t rule) {
  if (!h) return 0;
  if (rule == MAPFX_POLICY_DESCENT) return 1;
  return rule == MAPFX_POLICY_PIBT && wave_path_small_tables(h->geo) ? 1 : 0;
}

int mapfx_partial_policy_rule(mapfx_partial_t* h, int32_t rule) {
  if (!h) return perr(MAPFX_EINVAL, "NULL handle");
  if (rule != MAPFX_POLICY_DESCENT && rule != MAPFX_POLICY_PIBT)
    return perr(MAPFX_EINVAL, "mapfx_partial_policy_rule: unknown rule");
  if (!mapfx_partial_policy_rule_offered(h, rule))
    return refuse_small_tables("mapfx_partial_policy_rule: MAPFX_POLICY_PIBT");
  h->rule = rule;
  return MAPFX_OK;
}

int mapfx_partial_runner_rollout_offered(const mapfx_partial_t* h, int policy) {
  return h && (policy ? wave_path_small_tables(h->geo) : wave_path(h->geo)) ? 1 : 0;
}

// The fused launch of mapfx_runner_rollout (runner.hip, which checks the runner's half of
// the arguments and runs the compaction after it); internal.h
int mapfx_partial_rollout_runner(mapfx_partial_t* h, const mapfx_partial_state* st, int32_t T, const void* actions,
                                 int action_dtype, const mapfx_partial_policy* pol, const mapfx_runner_acts* ra,
                                 const mapfx_runner_roll* rr, void* stream) {
  PArgs a;
  int rc = begin(h, st, nullptr, a);
  if (rc) return rc;
  if (!ra || !rr || !ra->alive || !ra->alive_prev) return perr(MAPFX_EINVAL, "mapfx_runner_rollout: NULL runner rows");
  if (T < 1) return perr(MAPFX_EINVAL, "mapfx_runner_rollout: T must be >= 1");
  // (check_policy refuses only without actions, the two checks after it only with them)
  if ((rc = check_policy(h, "mapfx_runner_rollout", actions, pol))) return rc;
  if (actions && (action_dtype < MAPFX_I8 || action_dtype > MAPFX_I64)) return perr(MAPFX_EINVAL, "bad action_dtype");
  const PGeo& g = h->geo;
  if (!wave_path(g))
    return perr(MAPFX_EINVAL, "mapfx_runner_rollout: offered on the wave kernel only (N <= 64, sides <= 256)");
  if (g.E == 0) return MAPFX_OK;
  RArgs ro;
  fused_args(h, st, T, actions, action_dtype, pol, a, ro);
  a.err = h->err;
  a.obs_rows = rr->obs_rows;
  a.obs_env_stride = rr->obs_sb;
  a.ra = *ra;
  a.ra.act_row = nullptr;
  a.ra.cmp_bs = nullptr;
  if (ro.policy) ro.t0 += ra->ts;  // the counter is the absolute row pol->t0 + ts
  RRun rn;
  memset(&rn, 0, sizeof(rn));
  rn.ts0 = ra->ts;
  rn.max_t = rr->max_t;
  rn.obs_st = rr->obs_st;
  rn.state_st = rr->state_st;
  rn.avail_st = rr->avail_st;
  rn.filled_st = rr->filled_st;
  rn.stale_out = rr->stale_out;
  const bool obs = rr->obs_rows != nullptr;
  return launch_fused(h, pick_run_roll(g, ro.policy ? h->rule : MAPFX_POLICY_DESCENT, obs), obs, stream,
                      "partial_runner_rollout_kernel launch", a, ro, rn);
}

}  // extern "C"
