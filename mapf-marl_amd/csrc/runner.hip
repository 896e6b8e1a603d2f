// runner.hip — MI355X (gfx950) episode writes of the batched ParallelRunner
// (include/mapfx_runner.h).
//
// The reference's runner loop (MARL-curve-main/src/runners/parallel_runner.py:91-173)
// moves every env's transition through a Pipe and a Python list into PyMARL's
// EpisodeBatch (components/episode_buffer.py:100-134).  These kernels write the
// same rows from the batched env's device outputs into the EpisodeBatch tensors
// and keep the runner's bookkeeping (running envs, the MAC's `bs` list, returns,
// lengths, env-step count) on the device, so a runner step needs no host sync.
//
// Byte-moving work only (HBM-bound): one workgroup per env copies the env's
// N x D float observation row with coalesced dword stores; the `bs` compaction is
// one workgroup's prefix scan.
#include <hip/hip_runtime.h>

#include <stdint.h>
#include <string.h>

#include "internal.h"
#include "mapfx.h"
#include "mapfx_runner.h"

namespace {

constexpr int RB = 256;  // threads of a row-copy workgroup

// obs / state / avail_actions (+ filled = 1) of env b into time row t
__device__ inline void write_pre(const mapfx_runner_state& rs, const mapfx_partial_out& o,
                                 const mapfx_episode_rows& r, int b, int t) {
  const int ND = rs.N * rs.D;
  if (r.obs) {  // U loads in flight per thread before the stores (restrict: no alias stalls)
    const float* __restrict__ src = o.obs + (int64_t)b * ND;
    float* __restrict__ dst = r.obs + (int64_t)b * r.obs_sb + (int64_t)t * r.obs_st;
    constexpr int U = 8;
    for (int base = 0; base < ND; base += RB * U) {
      float v[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int i = base + u * RB + (int)threadIdx.x;
        v[u] = i < ND ? src[i] : 0.0f;
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int i = base + u * RB + (int)threadIdx.x;
        if (i < ND) dst[i] = v[u];
      }
    }
  }
  if (r.state && threadIdx.x < 3)
    r.state[(int64_t)b * r.state_sb + (int64_t)t * r.state_st + threadIdx.x] = o.state[(int64_t)b * 3 + threadIdx.x];
  if (r.avail) {  // 5-bit mask -> [N][5] int32 (get_avail_actions, marl_partial.py:389-433)
    int32_t* dst = r.avail + (int64_t)b * r.avail_sb + (int64_t)t * r.avail_st;
    for (int i = threadIdx.x; i < rs.N * 5; i += blockDim.x) {
      const int n = i / 5, k = i - 5 * n;
      dst[i] = (o.avail[(int64_t)b * rs.N + n] >> k) & 1;
    }
  }
  if (r.filled && threadIdx.x == 0) r.filled[(int64_t)b * r.filled_sb + (int64_t)t * r.filled_st] = 1;
}

__global__ void __launch_bounds__(RB) runner_begin_kernel(mapfx_runner_state rs, mapfx_partial_out o,
                                                          mapfx_episode_rows r) {
  const int b = blockIdx.x;
  write_pre(rs, o, r, b, 0);  // reset(): update(pre_transition_data, ts=0) (:62-76), all envs
  if (threadIdx.x == 0) {
    rs.alive[b] = 1;
    rs.alive_prev[b] = 1;
    rs.bs[b] = b;
    if (rs.bs_inv) rs.bs_inv[b] = b;
    rs.ep_return[b] = 0.0;
    rs.ep_length[b] = 0;
    if (b == 0) {
      rs.counts[0] = rs.B;
      rs.counts[1] = rs.B;
      rs.env_steps[0] = 0;
    }
  }
  for (int n = threadIdx.x; n < rs.N; n += blockDim.x) rs.env_actions[(int64_t)b * rs.N + n] = 4;
}

__device__ inline int64_t load_act(const void* p, int dtype, int64_t i) {
  if (dtype == MAPFX_I8) return ((const int8_t*)p)[i];
  if (dtype == MAPFX_I32) return ((const int32_t*)p)[i];
  return ((const int64_t*)p)[i];
}

// update({"actions": actions.unsqueeze(1)}, bs=envs_not_terminated, ts) (:104-110) and
// the OneHot preprocess (components/transforms.py) of the same rows
__global__ void runner_actions_kernel(mapfx_runner_state rs, const void* acts, int dtype,
                                      int64_t row_stride, int ts, mapfx_episode_rows r) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int j = (int)(i / rs.N), n = (int)(i - (int64_t)j * rs.N);
  if (j >= rs.counts[0]) return;
  const int64_t b = rs.bs[j];
  const int64_t a = load_act(acts, dtype, (int64_t)j * row_stride + n);
  if (r.actions) r.actions[b * r.actions_sb + (int64_t)ts * r.actions_st + n] = a;
  if (r.onehot) {
    float* oh = r.onehot + b * r.onehot_sb + (int64_t)ts * r.onehot_st + (int64_t)n * 5;
#pragma unroll
    for (int k = 0; k < 5; ++k) oh[k] = (a == k) ? 1.0f : 0.0f;
  }
  // the env receives only the envs that have not terminated (:116-121); the others
  // are never stepped again, whatever env_actions holds for them
  rs.env_actions[b * rs.N + n] = (int8_t)((a < -128 || a > 127) ? -1 : a);
}

// output mode: the rows at ts + 1 of every env the step just wrote them for (filled != 0),
// again, from the observations of the repaired state (mapfx_runner_reobserve)
__global__ void __launch_bounds__(RB) runner_reobserve_kernel(mapfx_runner_state rs, mapfx_partial_out o, int ts,
                                                              mapfx_episode_rows r) {
  const int b = blockIdx.x;
  if (r.filled[(int64_t)b * r.filled_sb + (int64_t)(ts + 1) * r.filled_st] == 0) return;  // uniform per block
  write_pre(rs, o, r, b, ts + 1);
}

// receive loop of one step (:125-173) for every env still running
__global__ void __launch_bounds__(RB) runner_post_kernel(mapfx_runner_state rs, const uint8_t* term,
                                                         mapfx_partial_out o, int ts,
                                                         mapfx_episode_rows r) {
  const int b = blockIdx.x;
  const uint8_t live = rs.alive[b];
  __syncthreads();  // every thread read alive[b] before thread 0 rewrites it
  if (live) {
    const double R = o.reward[b];
    const uint8_t tn = term[b] ? 1 : 0;
    if (threadIdx.x == 0) {
      if (r.reward) r.reward[(int64_t)b * r.reward_sb + (int64_t)ts * r.reward_st] = (float)R;
      // env_terminated = terminated and not info.get("episode_limit") (:146-150): MARL_PARTIAL's
      // info has no "episode_limit" key
      if (r.terminated) r.terminated[(int64_t)b * r.terminated_sb + (int64_t)ts * r.terminated_st] = tn;
      rs.ep_return[b] = rs.ep_return[b] + R;
      rs.ep_length[b] += 1;
      rs.alive[b] = tn ? 0 : 1;   // (env_steps: counted by the compaction, no atomics here)
    }
    if (ts + 1 < r.max_t) write_pre(rs, o, r, b, ts + 1);
  }
  if (threadIdx.x == 0) rs.alive_prev[b] = live;
}

// envs_not_terminated (:123) for the next MAC call: ascending indices of alive_prev,
// padded with the first one (so a MAC indexing rows by `bs` only sees running envs);
// counts = {len(bs), number alive}.  One workgroup: per-thread chunk counts, a
// shuffle scan inside each wave and one barrier for the 16 wave totals.
constexpr int CT = 1024;
// A second workgroup (mapfx_runner_rollout only, stale_map not NULL): the row map of a stale
// list given as flags in stale_map (>= 0: on it), turned into rows in place -- the same scan,
// nothing else written.
__global__ void __launch_bounds__(CT) runner_compact_kernel(mapfx_runner_state rs, int32_t* counts_out,
                                                            int32_t* stale_map) {
  const bool second = blockIdx.x == 1;
  const auto listed = [&](int b) { return second ? stale_map[b] >= 0 : rs.alive_prev[b] != 0; };
  __shared__ int wsum[CT / 64];
  __shared__ int wsum_a[CT / 64];
  const int chunk = (rs.B + CT - 1) / CT;
  const int lo = threadIdx.x * chunk, hi = min(rs.B, lo + chunk);
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  int c = 0, ca = 0;
  for (int b = lo; b < hi; ++b) {
    c += listed(b) ? 1 : 0;
    ca += rs.alive[b] ? 1 : 0;
  }
  int x = c;  // inclusive scan over the wave's lanes
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int y = __shfl_up(x, o);
    if (lane >= o) x += y;
  }
  int xa = ca;  // the wave's alive count
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) xa += __shfl_xor(xa, o);
  if (lane == 63) wsum[wv] = x;
  if (lane == 0) wsum_a[wv] = xa;
  __syncthreads();
  int off = 0, total = 0, total_a = 0;
#pragma unroll
  for (int i = 0; i < CT / 64; ++i) {
    const int v = wsum[i];
    off += i < wv ? v : 0;
    total += v;
    total_a += wsum_a[i];
  }
  int o = off + x - c;  // exclusive prefix of this thread's chunk
  if (second) {
    for (int b = lo; b < hi; ++b) stale_map[b] = listed(b) ? o++ : -1;
    return;  // (uniform over the workgroup)
  }
  for (int b = lo; b < hi; ++b) {
    const bool in = rs.alive_prev[b] != 0;
    if (rs.bs_inv) rs.bs_inv[b] = in ? o : -1;  // where the next MAC call puts env b's row
    if (in) rs.bs[o++] = b;
  }
  __syncthreads();  // bs[0] written
  const int64_t first = total > 0 ? rs.bs[0] : 0;
  for (int j = total + threadIdx.x; j < rs.B; j += CT) rs.bs[j] = first;
  if (threadIdx.x == 0) {
    rs.counts[0] = total;
    rs.counts[1] = total_a;
    rs.env_steps[0] += total;  // the envs stepped this step: env_steps_this_run (:142)
    if (counts_out) {  // possibly pinned host memory
      counts_out[0] = total;
      counts_out[1] = total_a;
    }
  }
}

// ---- action selection (mapfx_select_actions; the rule: mapfx_runner.h, mapfx/rng.py
// select_actions) ----
// mapfx/rng.py: K_ENV, K_T, K_AGENT, K_STREAM and the selection's stream id
constexpr uint64_t RK_ENV = 0xD1B54A32D192ED03ull, RK_T = 0xABC98388FB8FAC03ull,
                   RK_AGENT = 0x8CB92BA72F3D8DD7ull, RK_STREAM = 0xF1357AEA2E62A9C5ull;
constexpr uint64_t STREAM_SELECT = 0x700;

__host__ __device__ inline uint64_t select_word(uint64_t seed, int64_t gid, int32_t t, int32_t agent) {
  return splitmix64(seed ^ ((uint64_t)gid * RK_ENV) ^ ((uint64_t)(uint32_t)t * RK_T) ^
                    ((uint64_t)(uint32_t)agent * RK_AGENT) ^ (STREAM_SELECT * RK_STREAM));
}

// x replaces the running maximum b: torch's order, a NaN above every number and kept once met
__device__ inline bool beats(float x, float b) { return !(b != b) && ((x != x) || x > b); }

constexpr int SB = 256;  // threads of a selection workgroup: four independent waves

// The wave's 64 * A dwords of a dense [rows][N][A] array (row stride N * A: one contiguous
// run starting at the wave's first lane) into its LDS slice with A coalesced loads per lane;
// lane l then reads dwords l * A .. l * A + A - 1 (a lane stride of A dwords: at A = 5 coprime
// to the banks, no conflict).  The lanes past the array's end load nothing.
template <int AM, typename T>
__device__ inline void stage_dense(T* __restrict__ lds, const T* __restrict__ src, int A, int64_t base,
                                   int64_t end, int lane) {
#pragma unroll
  for (int i = 0; i < AM; ++i) {
    const int idx = i * 64 + lane;
    if (i < A && base + idx < end) lds[idx] = src[base + idx];
  }
}

// One lane per (row, agent).  AC: the compile-time number of actions, 0 = a.A at run time.
template <int AC>
__global__ void __launch_bounds__(SB) select_kernel(mapfx_select_args a, int dense_q, int dense_av) {
  constexpr int AM = AC ? AC : 9;
  const int A = AC ? AC : a.A;
  __shared__ float s_q[SB / 64][64 * AM];
  __shared__ int32_t s_av[SB / 64][64 * AM];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const uint32_t total = (uint32_t)a.rows * (uint32_t)a.N;  // < 2^31 (checked by the host)
  const uint32_t wave0 = blockIdx.x * SB + wv * 64;
  if (wave0 >= total) return;  // (wave-uniform)
  if (dense_q) stage_dense<AM>(s_q[wv], a.q, A, (int64_t)wave0 * A, (int64_t)total * A, lane);
  if (dense_av)
    stage_dense<AM>(s_av[wv], (const int32_t*)a.avail, A, (int64_t)wave0 * A, (int64_t)total * A, lane);
  wave_fence();
  const uint32_t gl = wave0 + lane;
  if (gl >= total) return;  // the tail lanes are off from here on: no address of theirs is formed
  const uint32_t row = gl / (uint32_t)a.N, ag = gl - row * (uint32_t)a.N;

  float v[AM];
  unsigned m = 0;
  const unsigned all = (1u << A) - 1u;
  // (two loops, not one select per element: a select of the two pointers becomes a flat load)
  if (dense_q) {
#pragma unroll
    for (int i = 0; i < AM; ++i)
      if (i < A) v[i] = s_q[wv][lane * A + i];
  } else {
    const float* qrow = a.q + (int64_t)row * a.q_sr + (int64_t)ag * A;
#pragma unroll
    for (int i = 0; i < AM; ++i)
      if (i < A) v[i] = qrow[i];
  }
  if (!a.avail) {
    m = all;
  } else if (a.avail_form == MAPFX_AVAIL_BITS) {
    const int64_t i = (int64_t)row * a.avail_sr + ag;
    m = (A == 9 ? (unsigned)((const uint16_t*)a.avail)[i] : (unsigned)((const uint8_t*)a.avail)[i]) & all;
  } else if (dense_av) {
#pragma unroll
    for (int i = 0; i < AM; ++i)
      if (i < A) m |= (s_av[wv][lane * A + i] != 0 ? 1u : 0u) << i;
  } else {
    const int32_t* arow = (const int32_t*)a.avail + (int64_t)row * a.avail_sr + (int64_t)ag * A;
#pragma unroll
    for (int i = 0; i < AM; ++i)
      if (i < A) m |= (arow[i] != 0 ? 1u : 0u) << i;
  }
  const int64_t gid = a.env_offset + (a.env_ids ? a.env_ids[row] : (int64_t)row);
  const uint64_t u = select_word(a.seed, gid, a.t, (int32_t)ag);
  const uint64_t lo = u & 0xFFFFFFFFull;

  // greedy(v masked with `fill`): the first maximum, NaN above all
  const float fill = a.mode == MAPFX_SELECT_EPS_GREEDY ? -__builtin_inff() : 0.0f;
#pragma unroll
  for (int i = 0; i < AM; ++i)
    if (i < A && !((m >> i) & 1u)) v[i] = fill;
  int g = 0;
  float best = v[0];
#pragma unroll
  for (int i = 1; i < AM; ++i)
    if (i < A && beats(v[i], best)) {
      best = v[i];
      g = i;
    }
  int act = g;
  if (a.mode == MAPFX_SELECT_EPS_GREEDY) {
    const int n = __popc(m);
    if (!a.greedy_only && (u >> 32) < a.eps_q && n > 0) {
      const int k = (int)((lo * (uint64_t)n) >> 32);  // the k-th available index, ascending
      int cnt = 0;
#pragma unroll
      for (int i = 0; i < AM; ++i)
        if (i < A && ((m >> i) & 1u)) {
          if (cnt == k) act = i;
          ++cnt;
        }
    }
  } else if (!a.greedy_only) {
    float c[AM];
    float s = 0.0f;
#pragma unroll
    for (int i = 0; i < AM; ++i)
      if (i < A) {
        s = i == 0 ? v[0] : __fadd_rn(s, v[i]);  // c_i = c_{i-1} + p_i, float32, in this order
        c[i] = s;
      }
    if (s > 0.0f && s < __builtin_inff()) {  // a finite number above 0 (a NaN fails s > 0)
      // r is exact (24 bits), x one float32 rounding; neither product feeds an add
      const float r = __fmul_rn((float)(uint32_t)(lo >> 8), 0x1p-24f);
      const float x = __fmul_rn(r, s);
      int first = -1, last = 0;
#pragma unroll
      for (int i = 0; i < AM; ++i)
        if (i < A) {
          if (first < 0 && c[i] > x) first = i;
          if (v[i] > 0.0f) last = i;
        }
      act = first >= 0 ? first : last;
    }
  }
  a.actions[(int64_t)row * a.actions_sr + ag] = (int64_t)act;
}

int check_select(const mapfx_select_args* a) {
  if (!a) return perr(MAPFX_EINVAL, "select_actions: NULL args");
  if (a->rows < 0 || a->N < 1) return perr(MAPFX_EINVAL, "select_actions: rows < 0 or N < 1");
  if (a->A < 1 || a->A > 9) return perr(MAPFX_EINVAL, "select_actions: A not in 1..9");
  if ((int64_t)a->rows * a->N >= (1ll << 31)) return perr(MAPFX_EINVAL, "select_actions: rows * N must be below 2^31");
  if (a->mode != MAPFX_SELECT_EPS_GREEDY && a->mode != MAPFX_SELECT_MULTINOMIAL)
    return perr(MAPFX_EINVAL, "select_actions: unknown mode");
  if (a->avail_form != MAPFX_AVAIL_I32 && a->avail_form != MAPFX_AVAIL_BITS)
    return perr(MAPFX_EINVAL, "select_actions: unknown avail_form");
  if (a->eps_q > (1ull << 32)) return perr(MAPFX_EINVAL, "select_actions: eps_q above 2^32");
  if (a->rows == 0) return MAPFX_OK;
  if (!a->q || !a->actions) return perr(MAPFX_EINVAL, "select_actions: NULL q / actions");
  const int64_t na = (int64_t)a->N * a->A;
  if (a->q_sr < na) return perr(MAPFX_EINVAL, "select_actions: q row stride smaller than N * A");
  if (a->avail && a->avail_sr < (a->avail_form == MAPFX_AVAIL_BITS ? (int64_t)a->N : na))
    return perr(MAPFX_EINVAL, "select_actions: avail row stride smaller than the row");
  if (a->actions_sr < a->N) return perr(MAPFX_EINVAL, "select_actions: actions row stride smaller than N");
  return MAPFX_OK;
}

int check_rs(const mapfx_runner_state* rs) {
  if (!rs || rs->B < 0 || rs->N < 1 || rs->D < 0 || !rs->alive || !rs->alive_prev || !rs->bs ||
      !rs->counts || !rs->ep_return || !rs->ep_length || !rs->env_steps || !rs->env_actions)
    return perr(MAPFX_EINVAL, "runner state: NULL field or bad B/N/D");
  return MAPFX_OK;
}

}  // namespace

extern "C" {

int mapfx_runner_begin(const mapfx_runner_state* rs, const mapfx_partial_out* out,
                       const mapfx_episode_rows* rows, void* stream) {
  int rc = check_rs(rs);
  if (rc) return rc;
  if (!out || !rows || !out->obs || !out->state || !out->avail)
    return perr(MAPFX_EINVAL, "runner_begin: NULL out / rows");
  if (rs->B == 0) return MAPFX_OK;
  return launch_kernel(runner_begin_kernel, dim3(rs->B), dim3(RB), 0, (hipStream_t)stream, nullptr, nullptr,
                       "runner_begin_kernel launch", QUIET, *rs, *out, *rows);
}

int mapfx_runner_actions(const mapfx_runner_state* rs, const void* actions, int32_t action_dtype,
                         int64_t row_stride, int32_t ts, const mapfx_episode_rows* rows,
                         void* stream) {
  int rc = check_rs(rs);
  if (rc) return rc;
  if (!actions || !rows) return perr(MAPFX_EINVAL, "runner_actions: NULL actions / rows");
  if (action_dtype < MAPFX_I8 || action_dtype > MAPFX_I64) return perr(MAPFX_EINVAL, "runner_actions: bad dtype");
  if (ts < 0 || ts >= rows->max_t) return perr(MAPFX_EINVAL, "runner_actions: ts outside the batch");
  const int64_t total = (int64_t)rs->B * rs->N;
  if (total == 0) return MAPFX_OK;
  return launch_kernel(runner_actions_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0,
                       (hipStream_t)stream, nullptr, nullptr, "runner_actions_kernel launch", QUIET, *rs, actions,
                       (int)action_dtype, row_stride, (int)ts, *rows);
}

int mapfx_runner_post(const mapfx_runner_state* rs, const uint8_t* terminated,
                      const mapfx_partial_out* out, int32_t ts, int32_t* counts_out,
                      const mapfx_episode_rows* rows, void* stream) {
  int rc = check_rs(rs);
  if (rc) return rc;
  if (!terminated || !out || !rows || !out->reward || !out->obs || !out->state || !out->avail)
    return perr(MAPFX_EINVAL, "runner_post: NULL terminated / out / rows");
  if (ts < 0 || ts >= rows->max_t) return perr(MAPFX_EINVAL, "runner_post: ts outside the batch");
  if (rs->B == 0) return MAPFX_OK;
  rc = launch_kernel(runner_post_kernel, dim3(rs->B), dim3(RB), 0, (hipStream_t)stream, nullptr, nullptr,
                     "runner_post_kernel launch", QUIET, *rs, terminated, *out, (int)ts, *rows);
  if (rc) return rc;
  return launch_kernel(runner_compact_kernel, dim3(1), dim3(CT), 0, (hipStream_t)stream, nullptr, nullptr,
                       "runner_compact_kernel launch", QUIET, *rs, counts_out, (int32_t*)nullptr);
}

int mapfx_runner_reobserve(const mapfx_runner_state* rs, const mapfx_partial_out* out, int32_t ts,
                           const mapfx_episode_rows* rows, void* stream) {
  int rc = check_rs(rs);
  if (rc) return rc;
  if (!out || !rows || !out->obs || !out->state || !out->avail || !rows->filled)
    return perr(MAPFX_EINVAL, "runner_reobserve: NULL out / rows / filled rows");
  if (ts < 0 || ts >= rows->max_t) return perr(MAPFX_EINVAL, "runner_reobserve: ts outside the batch");
  if (rs->B == 0 || ts + 1 == rows->max_t) return MAPFX_OK;  // no row ts + 1: nothing to launch
  return launch_kernel(runner_reobserve_kernel, dim3(rs->B), dim3(RB), 0, (hipStream_t)stream, nullptr, nullptr,
                       "runner_reobserve_kernel launch", QUIET, *rs, *out, (int)ts, *rows);
}

int mapfx_runner_step(mapfx_partial_t* h, const mapfx_partial_state* st, const mapfx_partial_out* out,
                      const mapfx_runner_state* rs, const void* actions, int32_t action_dtype,
                      int64_t row_stride, int32_t ts, int32_t* counts_out,
                      const mapfx_episode_rows* rows, void* stream) {
  int rc = check_rs(rs);
  if (rc) return rc;
  if (!rows) return perr(MAPFX_EINVAL, "runner_step: NULL rows");
  if (ts < 0 || ts >= rows->max_t) return perr(MAPFX_EINVAL, "runner_step: ts outside the batch");
  if (!rs->bs_inv)  // the unfused form: a separate actions pass into env_actions
    return (rc = mapfx_runner_actions(rs, actions, action_dtype, row_stride, ts, rows, stream)) ? rc
           : (rc = mapfx_partial_step(h, st, rs->env_actions, MAPFX_I8, out, stream))
               ? rc : mapfx_runner_post(rs, st->terminated, out, ts, counts_out, rows, stream);
  // the env step reads each env's actions from the MAC's output (row bs_inv[b]) and
  // writes the actions / one-hot rows at ts itself; when the batch has observation rows
  // it also writes those of the envs running before it (rs->alive, updated only by the
  // post kernel) straight into time row ts + 1, so the post kernel moves no observation
  // bytes
  mapfx_runner_acts ra;
  memset(&ra, 0, sizeof ra);
  // the post pass in the env step's write-back too (the one-wave-per-env-group kernel),
  // and with it the compaction for the next MAC call as the launch's first workgroup:
  // alive flags and the row map double-buffered by step parity (alive / alive_prev =
  // A[0] / A[1], bs_inv = [2][B]; A[ts & 1] = running before step ts)
  const bool fpost = mapfx_partial_fuses_post(h) != 0;
  const int par = ts & 1;
  ra.act_row = rs->bs_inv + (fpost ? (int64_t)par * rs->B : 0);
  ra.act_row_stride = row_stride;
  ra.ep_actions = rows->actions;
  ra.ep_actions_sb = rows->actions_sb;
  ra.ep_actions_st = rows->actions_st;
  ra.ep_onehot = rows->onehot;
  ra.ep_onehot_sb = rows->onehot_sb;
  ra.ep_onehot_st = rows->onehot_st;
  ra.ts = ts;
  const bool nxt = ts + 1 < rows->max_t;
  uint8_t* const a_in = par ? rs->alive_prev : rs->alive;   // A[ts & 1]
  uint8_t* const a_out = par ? rs->alive : rs->alive_prev;  // A[(ts + 1) & 1]
  if (fpost) {
    ra.alive = a_in;
    ra.alive_prev = a_out;
    ra.cmp_alive = a_in;
    ra.cmp_bs = rs->bs;
    ra.cmp_bs_inv = rs->bs_inv + (int64_t)(par ^ 1) * rs->B;
    ra.cmp_counts = rs->counts;
    ra.cmp_env_steps = rs->env_steps;
    ra.cmp_counts_out = counts_out;
    ra.cmp_B = rs->B;
    ra.ep_return = rs->ep_return;
    ra.ep_length = rs->ep_length;
    ra.ep_reward = rows->reward;
    ra.ep_reward_sb = rows->reward_sb;
    ra.ep_reward_st = rows->reward_st;
    ra.ep_term = rows->terminated;
    ra.ep_term_sb = rows->terminated_sb;
    ra.ep_term_st = rows->terminated_st;
    ra.ep_state = nxt && rows->state ? rows->state + (int64_t)(ts + 1) * rows->state_st : nullptr;
    ra.ep_state_sb = rows->state_sb;
    ra.ep_avail = nxt && rows->avail ? rows->avail + (int64_t)(ts + 1) * rows->avail_st : nullptr;
    ra.ep_avail_sb = rows->avail_sb;
    ra.ep_filled = nxt && rows->filled ? rows->filled + (int64_t)(ts + 1) * rows->filled_st : nullptr;
    ra.ep_filled_sb = rows->filled_sb;
  }
  float* obs_row = rows->obs && nxt ? rows->obs + (int64_t)(ts + 1) * rows->obs_st : nullptr;
  if ((rc = mapfx_partial_step_runner(h, st, actions, action_dtype, &ra, out, obs_row, rows->obs_sb,
                                      fpost ? a_in : rs->alive, stream)))
    return rc;
  if (fpost) return MAPFX_OK;  // (the compaction ran as the launch's first workgroup)
  if (!rows->obs) return mapfx_runner_post(rs, st->terminated, out, ts, counts_out, rows, stream);
  mapfx_episode_rows r2 = *rows;
  r2.obs = nullptr;
  return mapfx_runner_post(rs, st->terminated, out, ts, counts_out, &r2, stream);
}

int mapfx_runner_rollout_offered(const mapfx_partial_t* h, int policy) {
  return mapfx_partial_runner_rollout_offered(h, policy);
}

int mapfx_runner_rollout(mapfx_partial_t* h, const mapfx_partial_state* st, const mapfx_runner_state* rs,
                         int32_t ts0, int32_t T, const void* actions, int action_dtype,
                         const mapfx_partial_policy* pol, int32_t* counts_out, const mapfx_episode_rows* rows,
                         void* stream) {
  if (!h) return perr(MAPFX_EINVAL, "runner_rollout: NULL handle");
  int rc = check_rs(rs);
  if (rc) return rc;
  if (!rs->bs_inv) return perr(MAPFX_EINVAL, "runner_rollout: the runner state needs bs_inv");
  if (!st || !rows) return perr(MAPFX_EINVAL, "runner_rollout: NULL state / rows");
  if (T < 1 || ts0 < 0 || (int64_t)ts0 + T > rows->max_t)
    return perr(MAPFX_EINVAL, "runner_rollout: steps ts0 .. ts0 + T - 1 must lie inside the batch, T >= 1");
  if (!actions && !pol) return perr(MAPFX_EINVAL, "runner_rollout: actions or a policy is required");
  if (actions && (action_dtype < MAPFX_I8 || action_dtype > MAPFX_I64))
    return perr(MAPFX_EINVAL, "runner_rollout: bad dtype");
  // the parity pair as mapfx_runner_step uses it: A[ts & 1] = running before step ts
  const int par0 = ts0 & 1, ts_end = ts0 + T - 1, par_end = ts_end & 1;
  mapfx_runner_acts ra;
  memset(&ra, 0, sizeof ra);
  ra.ts = ts0;
  ra.ep_actions = rows->actions;
  ra.ep_actions_sb = rows->actions_sb;
  ra.ep_actions_st = rows->actions_st;
  ra.ep_onehot = rows->onehot;
  ra.ep_onehot_sb = rows->onehot_sb;
  ra.ep_onehot_st = rows->onehot_st;
  ra.alive = par0 ? rs->alive_prev : rs->alive;
  ra.alive_prev = par0 ? rs->alive : rs->alive_prev;
  ra.ep_return = rs->ep_return;
  ra.ep_length = rs->ep_length;
  ra.cmp_env_steps = rs->env_steps;
  ra.ep_reward = rows->reward;
  ra.ep_reward_sb = rows->reward_sb;
  ra.ep_reward_st = rows->reward_st;
  ra.ep_term = rows->terminated;
  ra.ep_term_sb = rows->terminated_sb;
  ra.ep_term_st = rows->terminated_st;
  ra.ep_state = rows->state;
  ra.ep_state_sb = rows->state_sb;
  ra.ep_avail = rows->avail;
  ra.ep_avail_sb = rows->avail_sb;
  ra.ep_filled = rows->filled;
  ra.ep_filled_sb = rows->filled_sb;
  mapfx_runner_roll rr;
  memset(&rr, 0, sizeof rr);
  rr.max_t = rows->max_t;
  rr.obs_rows = rows->obs ? rows->obs + (int64_t)(ts0 + 1) * rows->obs_st : nullptr;
  rr.obs_sb = rows->obs_sb;
  rr.obs_st = rows->obs_st;
  rr.state_st = rows->state_st;
  rr.avail_st = rows->avail_st;
  rr.filled_st = rows->filled_st;
  // T >= 2: the row map of the last step's stale list (what step ts_end - 1's compaction
  // leaves in bs_inv[ts_end & 1]) -- the kernel writes the list as flags, the compaction's
  // second workgroup turns them into rows
  int32_t* const stale_map = T >= 2 ? rs->bs_inv + (int64_t)par_end * rs->B : nullptr;
  rr.stale_out = stale_map;
  if ((rc = mapfx_partial_rollout_runner(h, st, T, actions, action_dtype, pol, &ra, &rr, stream))) return rc;
  if (rs->B == 0) return MAPFX_OK;
  // what step ts_end's compaction leaves: bs / counts of A[ts_end & 1] (running before the
  // last step), its row map in the other half of bs_inv, env_steps += its length
  mapfx_runner_state r2 = *rs;
  r2.alive_prev = par_end ? rs->alive_prev : rs->alive;
  r2.alive = r2.alive_prev;  // counts[1] = len(bs), as the fused step reports it
  r2.bs_inv = rs->bs_inv + (int64_t)(par_end ^ 1) * rs->B;
  return launch_kernel(runner_compact_kernel, dim3(stale_map ? 2 : 1), dim3(CT), 0, (hipStream_t)stream, nullptr,
                       nullptr, "runner_compact_kernel launch", QUIET, r2, counts_out, stale_map);
}

uint64_t mapfx_select_word(uint64_t seed, int64_t gid, int32_t t, int32_t agent) {
  return select_word(seed, gid, t, agent);
}

int mapfx_select_actions(const mapfx_select_args* a, void* stream) {
  const int rc = check_select(a);
  if (rc || a->rows == 0) return rc;
  const int64_t na = (int64_t)a->N * a->A;
  const int dense_q = a->q_sr == na;
  const int dense_av = a->avail && a->avail_form == MAPFX_AVAIL_I32 && a->avail_sr == na;
  const dim3 grid((unsigned)(((int64_t)a->rows * a->N + SB - 1) / SB));
  return launch_kernel(a->A == 5 ? select_kernel<5> : select_kernel<0>, grid, dim3(SB), 0, (hipStream_t)stream,
                       nullptr, nullptr, "select_kernel launch", NOTED, *a, dense_q, dense_av);
}

int mapfx_host_ring_alloc(int32_t n, int32_t** host_ptr, int32_t** dev_ptr) {
  if (n < 1 || !host_ptr || !dev_ptr) return perr(MAPFX_EINVAL, "host_ring_alloc: bad arguments");
  *host_ptr = nullptr;
  *dev_ptr = nullptr;
  void* p = nullptr;
  if (hipHostMalloc(&p, sizeof(int32_t) * (size_t)n, hipHostMallocMapped | hipHostMallocCoherent) != hipSuccess)
    return perr(MAPFX_ENOMEM, "hipHostMalloc (mapped, coherent) failed");
  void* d = nullptr;
  if (hipHostGetDevicePointer(&d, p, 0) != hipSuccess) {
    (void)hipHostFree(p);
    return perr(MAPFX_EHIP, "hipHostGetDevicePointer failed");
  }
  memset(p, 0, sizeof(int32_t) * (size_t)n);
  *host_ptr = (int32_t*)p;
  *dev_ptr = (int32_t*)d;
  return MAPFX_OK;
}

void mapfx_host_ring_free(int32_t* host_ptr) {
  if (host_ptr) (void)hipHostFree(host_ptr);
}

}  // extern "C"
