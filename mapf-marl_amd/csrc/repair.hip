// repair.hip -- MARL_PARTIAL_ENV output mode: the collision repair after a step
// (MARL-curve-main/src/envs/marl_partial.py:262-275, solvers :645-711 and :739-820) on the
// device.  The rule -- the reference's control flow with its two `while` loops cut at
// max_rounds and every random.shuffle a counter-based order -- is defined by
// mapfx.rng.partial_repair (mapfx/rng.py); this kernel equals it bit for bit.
//
// One wavefront (one 64-thread workgroup) per env, lane = agent, offered where the wave step
// kernel runs (N <= 64, sides <= 256).  The positions live in registers; everything the
// reference does to ONE agent or pair at a time is a wave-uniform walk: the operands come
// from the owning lanes by shuffle, every lane computes the same decision, and the owning
// lane alone takes the new cell.  `these_agents`, the node groups and the swap pairs are
// ballots / shuffle loops over the lane-held cells.
//
// LDS (4 KB static, up to 20 KB dynamic per workgroup):
//   tab_key / tab_cnt  2 x 512 x 4 B  the round's signed per-cell counts, open addressing on
//                                     the cell index.  Every cell a repair touches is an
//                                     agent's pre-step cell or one of its 4 neighbours: at
//                                     most 5 N = 320 keys, so a probe always ends on a hit or
//                                     a free slot.  Rebuilt from the positions every round.
//   keys               P x 8 B        the order keys of an edge round's pairs, sorted by a
//                                     bitonic network; P = the next power of two of
//                                     N (N - 1) / 2 (dynamic: 2048 at N = 64, 128 at N = 15)
//   pair_id            P x 2 B        item number -> (i << 8 | j) of the raw pair set
// The table is read and written by all lanes with the same (uniform) operands -- each lane
// reads back what it wrote itself -- except for the parallel build at the start of a round,
// which is fenced by workgroup barriers.
//
// Every loop is bounded at launch: max_rounds rounds of at most N agents (x at most N
// `these_agents` x 4 directions) or at most N (N - 1) / 2 pairs; a probe by the table size.
#include <string.h>

#include "internal.h"

namespace {

constexpr uint64_t RK_ENV = 0xD1B54A32D192ED03ull, RK_T = 0xABC98388FB8FAC03ull, RK_AGENT = 0x8CB92BA72F3D8DD7ull,
                   RK_CELL = 0x9E6C63D0676A9A99ull, RK_STREAM = 0xF1357AEA2E62A9C5ull;  // mapfx/rng.py K_*
constexpr uint32_t RS_REPAIR = 0x800u;  // rng.STREAM_REPAIR
constexpr int TAB = 512, TAB_LOG = 9, PAIR_MAX = 2048;
constexpr uint32_t TAB_EMPTY = 0xFFFFFFFFu;
enum { F_NODE_RAN = 1, F_EDGE_RAN = 2, F_NODE_CAP = 4, F_EDGE_CAP = 8, F_SWAP_LEFT = 16 };

struct RepArgs {
  int H, W, N, map_shared;
  long long map_stride, env_offset;
  uint64_t seed;
  int max_rounds;
  int pair_cap;  // next power of two of max(2, N (N - 1) / 2): entries of the pair arrays
  int32_t* pos;
  const int32_t* old_pos;
  uint8_t* node;
  int32_t* edge;
  const int32_t* t;
  const uint8_t* bits;
  const void* actions;
  int act_dtype;
  uint8_t* flags;
  int32_t* rounds;
};

struct Tab {
  uint32_t* key;
  int32_t* cnt;
  __device__ __forceinline__ uint32_t slot0(uint32_t cell) const { return (cell * 2654435761u) >> (32 - TAB_LOG); }
  // the slot of `cell`, or of the free slot its probe ends on (-1: table full, which 5 N <= 320
  // keys cannot make it)
  __device__ int find(uint32_t cell) const {
    uint32_t s = slot0(cell);
    for (int k = 0; k < TAB; ++k) {
      const uint32_t v = key[s];
      if (v == cell || v == TAB_EMPTY) return (int)s;
      s = (s + 1) & (TAB - 1);
    }
    return -1;
  }
  __device__ int get(uint32_t cell) const {
    const int s = find(cell);
    return (s >= 0 && key[s] == cell) ? cnt[s] : 0;
  }
  // All 64 lanes run this with the same operands and store the same values to the same
  // words: plain (non-atomic) accesses on purpose -- each lane reads back what it wrote
  // itself, so one lane's program order is all the ordering needed.  It holds only while
  // every call site is wave-uniform and `cnt[s] += d` stays a plain load / add / store (an
  // LDS atomic would apply d once per lane).
  __device__ void add(uint32_t cell, int d) const {
    const int s = find(cell);
    if (s < 0) return;
    if (key[s] != cell) {
      key[s] = cell;
      cnt[s] = d;
    } else {
      cnt[s] += d;
    }
  }
  // the parallel build: every lane with an agent counts its cell
  __device__ void count(uint32_t cell) const {
    uint32_t s = slot0(cell);
    for (int k = 0; k < TAB; ++k) {
      const uint32_t v = atomicCAS(&key[s], TAB_EMPTY, cell);
      if (v == TAB_EMPTY || v == cell) {
        atomicAdd(&cnt[s], 1);
        return;
      }
      s = (s + 1) & (TAB - 1);
    }
  }
};

__device__ __forceinline__ uint64_t rep_word(uint64_t base, uint32_t site, uint32_t r, uint32_t owner, uint32_t j) {
  return splitmix64(base ^ ((uint64_t)owner * RK_AGENT) ^ ((uint64_t)(r * 4096u + j) * RK_CELL) ^
                    ((uint64_t)(RS_REPAIR + site) * RK_STREAM));
}
__device__ __forceinline__ uint64_t rep_key(uint64_t base, uint32_t site, uint32_t r, uint32_t owner, uint32_t j) {
  return (rep_word(base, site, r, owner, j) & ~0xFFFFull) | (uint64_t)j;
}

__device__ __forceinline__ uint64_t shfl64(uint64_t v, int src) {
  const uint32_t lo = (uint32_t)__shfl((int)(uint32_t)v, src);
  const uint32_t hi = (uint32_t)__shfl((int)(uint32_t)(v >> 32), src);
  return ((uint64_t)hi << 32) | lo;
}

// lane `lane`'s place among the lanes with `item` set, in ascending key order (the keys are
// distinct: their low 16 bits are the item numbers)
__device__ __forceinline__ int key_rank(uint64_t key, bool item, int N) {
  int rank = 0;
  for (int k = 0; k < N; ++k) {
    const uint64_t o = shfl64(key, k);
    const int it = __shfl((int)item, k);
    rank += (it && o < key) ? 1 : 0;
  }
  return rank;
}

struct Env {
  const RepArgs& a;
  const uint8_t* bits;
  int lane;
  bool has;
  int orow, ocol, crow, ccol, act;  // this lane's agent: cell before the step, current cell, action

  __device__ __forceinline__ uint32_t cell(int r, int c) const { return (uint32_t)(r * a.W + c); }
  // __is_valid and not __is_cell_obstacle on the PRE-step occupancy (:504-522): (r, c) uniform
  __device__ bool is_free(int r, int c) const {
    if (r < 0 || r >= a.H || c < 0 || c >= a.W) return false;
    const uint32_t i = cell(r, c);
    if (!((bits[i >> 3] >> (i & 7)) & 1)) return true;
    return __ballot(has && orow == r && ocol == c) != 0;
  }
  __device__ __forceinline__ void put(int ag, int r, int c) {
    if (lane == ag) {
      crow = r;
      ccol = c;
    }
  }
};

__device__ __forceinline__ int d_row(int act) { return act == 0 ? -1 : act == 1 ? 1 : 0; }  // :617-643
__device__ __forceinline__ int d_col(int act) { return act == 2 ? -1 : act == 3 ? 1 : 0; }

// __check_node_collisions (:713-737): this lane's 0 / 1
__device__ int check_node(const Env& v, int N) {
  int n = 0;
  for (int k = 0; k < N; ++k) {  // (no shuffle behind a lane-dependent &&: all lanes take part in each)
    const int kr = __shfl(v.crow, k), kc = __shfl(v.ccol, k);
    n += (kr == v.crow && kc == v.ccol) ? 1 : 0;
  }
  return (v.has && n > 1) ? 1 : 0;
}

// __check_edge_collisions (:822-857): this lane's count, and its partners as a lane mask
__device__ int check_edge(const Env& v, int N, uint64_t& partners) {
  int n = 0;
  partners = 0;
  const bool moved = v.has && (v.orow != v.crow || v.ocol != v.ccol);
  for (int k = 0; k < N; ++k) {
    const int k_or = __shfl(v.orow, k), k_oc = __shfl(v.ocol, k), k_cr = __shfl(v.crow, k), k_cc = __shfl(v.ccol, k);
    const bool hit = k_or == v.crow && k_oc == v.ccol && k_cr == v.orow && k_cc == v.ocol;
    if (moved && hit && k != v.lane) {
      ++n;
      partners |= 1ull << k;
    }
  }
  return n;
}

__device__ void rebuild(const Tab& tb, const Env& v) {
  __syncthreads();
  for (int i = v.lane; i < TAB; i += 64) {
    tb.key[i] = TAB_EMPTY;
    tb.cnt[i] = 0;
  }
  __syncthreads();
  if (v.has) tb.count(v.cell(v.crow, v.ccol));
  __syncthreads();
}

// __solve_node_collisions (:645-711), round r
__device__ void solve_node(const Tab& tb, Env& v, int N, uint64_t base, uint32_t r, int nvec) {
  rebuild(tb, v);
  const uint64_t lt = (1ull << v.lane) - 1ull;
  const bool item = v.has && nvec > 0;
  const uint64_t m = __ballot(item);
  const uint64_t key = item ? rep_key(base, 0, r, 0, (uint32_t)__popcll(m & lt)) : ~0ull;
  const int rank = key_rank(key, item, N);
  const int n_col = __popcll(m);
  for (int s = 0; s < n_col; ++s) {
    const int ag = __builtin_ctzll(__ballot(item && rank == s));
    const int ar = __shfl(v.crow, ag), ac = __shfl(v.ccol, ag);
    const uint32_t a_cell = v.cell(ar, ac);
    if (tb.get(a_cell) <= 1) continue;
    const int o_r = __shfl(v.orow, ag), o_c = __shfl(v.ocol, ag);
    const uint32_t o_cell = v.cell(o_r, o_c);
    if (tb.get(o_cell) <= 0) {  // back to its old cell
      tb.add(a_cell, -1);
      v.put(ag, o_r, o_c);
      tb.add(o_cell, 1);
      continue;
    }
    const int a_act = __shfl(v.act, ag);
    // these_agents: whoever stands on the old cell now, their actions tried in shuffled order
    const bool th = v.has && v.crow == o_r && v.ccol == o_c;
    const uint64_t mt = __ballot(th);
    const uint64_t tkey = th ? rep_key(base, 1, r, (uint32_t)ag, (uint32_t)__popcll(mt & lt)) : ~0ull;
    const int trank = key_rank(tkey, th, N);
    const int n_th = __popcll(mt);
    bool solved = false;
    for (int s2 = 0; s2 < n_th && !solved; ++s2) {
      const int other = __builtin_ctzll(__ballot(th && trank == s2));
      const int oa = __shfl(v.act, other);
      if (oa == a_act) continue;
      int pr = o_r, pc = o_c;
      if (oa != 4) {
        pr += d_row(oa);
        pc += d_col(oa);
        if (!v.is_free(pr, pc)) continue;
      }
      const uint32_t p = v.cell(pr, pc);
      if (tb.get(p) <= 0) {
        tb.add(a_cell, -1);
        v.put(ag, pr, pc);
        tb.add(p, 1);
        solved = true;
      }
    }
    if (solved) continue;
    // acts_try: the four moves in shuffled order
    uint64_t k4[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) k4[j] = rep_key(base, 2, r, (uint32_t)ag, (uint32_t)j);
#pragma unroll
    for (int i = 1; i < 4; ++i)
#pragma unroll
      for (int j = i; j > 0; --j)
        if (k4[j] < k4[j - 1]) {
          const uint64_t x = k4[j];
          k4[j] = k4[j - 1];
          k4[j - 1] = x;
        }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (solved) break;
      const int mv = (int)(k4[j] & 3ull);
      const int pr = o_r + d_row(mv), pc = o_c + d_col(mv);
      if (mv == a_act || !v.is_free(pr, pc)) continue;
      const uint32_t p = v.cell(pr, pc);
      if (tb.get(p) <= 0) {
        tb.add(o_cell, -1);  // the OLD cell, as the reference does (:706)
        v.put(ag, pr, pc);
        tb.add(p, 1);
        solved = true;
      }
    }
  }
}

__device__ __forceinline__ void cmpx(uint64_t* keys, int lo, int hi, bool up) {
  const uint64_t x = keys[lo], y = keys[hi];
  if ((x > y) == up) {
    keys[lo] = y;
    keys[hi] = x;
  }
}

// one agent's try at cell (pr, pc), leaving `from`: the move all three edge branches make
__device__ __forceinline__ bool try_cell(const Tab& tb, Env& v, int ag, int pr, int pc, uint32_t from) {
  if (!v.is_free(pr, pc)) return false;
  const uint32_t p = v.cell(pr, pc);
  if (tb.get(p) > 0) return false;
  tb.add(from, -1);
  v.put(ag, pr, pc);
  tb.add(p, 1);
  return true;
}

// __solve_edge_collisions (:739-820), round r, over the n_pairs RAW pairs in pair_id
__device__ void solve_edge(const Tab& tb, Env& v, uint64_t base, uint32_t r, uint64_t* keys, const uint16_t* pair_id,
                           int n_pairs) {
  rebuild(tb, v);
  int P = 2;
  while (P < n_pairs) P <<= 1;  // <= a.pair_cap: n_pairs <= N (N - 1) / 2
  for (int j = v.lane; j < P; j += 64) keys[j] = j < n_pairs ? rep_key(base, 3, r, 0, (uint32_t)j) : ~0ull;
  __syncthreads();
  for (int k = 2; k <= P; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int i = v.lane; i < (P >> 1); i += 64) {
        const int lo = ((i & ~(j - 1)) << 1) | (i & (j - 1));
        cmpx(keys, lo, lo | j, (lo & k) == 0);
      }
      __syncthreads();
    }
  for (int idx = 0; idx < n_pairs; ++idx) {
    const int id = pair_id[(int)(keys[idx] & 0xFFFFull)];
    const int pi = id >> 8, pj = id & 255;
    const bool flip = (rep_word(base, 4, r, (uint32_t)pi, (uint32_t)pj) >> 63) != 0;
    const int pair[2] = {flip ? pj : pi, flip ? pi : pj};
    bool solved = false;
    uint32_t a_cell = 0;
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      if (solved) break;
      const int ag = pair[q];
      a_cell = v.cell(__shfl(v.crow, ag), __shfl(v.ccol, ag));
      const int o_r = __shfl(v.orow, ag), o_c = __shfl(v.ocol, ag), aa = __shfl(v.act, ag);
      if (aa > 3) continue;  // (a swapping agent moved: never a stay)
      // try_map (:775): the two moves across the one taken, in the reference's order
      const int first = aa == 0 ? 2 : aa == 1 ? 3 : aa == 2 ? 0 : 1;
      if (try_cell(tb, v, ag, o_r + d_row(first), o_c + d_col(first), a_cell) ||
          try_cell(tb, v, ag, o_r + d_row(first ^ 1), o_c + d_col(first ^ 1), a_cell))
        solved = true;
    }
    if (solved) continue;
#pragma unroll
    for (int q = 0; q < 2; ++q) {  // back up; a_cell is the one the loop above left (:807)
      const int ag = pair[q];
      const int o_r = __shfl(v.orow, ag), o_c = __shfl(v.ocol, ag), aa = __shfl(v.act, ag);
      if (aa > 3) continue;
      const int bk = aa ^ 1;
      if (try_cell(tb, v, ag, o_r + d_row(bk), o_c + d_col(bk), a_cell)) solved = true;
    }
    if (solved) continue;
#pragma unroll
    for (int q = 0; q < 2; ++q) v.put(pair[q], __shfl(v.orow, pair[q]), __shfl(v.ocol, pair[q]));
  }
}

__global__ void __launch_bounds__(64) partial_repair_kernel(RepArgs a) {
  __shared__ uint32_t s_key[TAB];
  __shared__ int32_t s_cnt[TAB];
  // the pair keys and the item -> pair map: a.pair_cap entries each (dynamic LDS)
  extern __shared__ __attribute__((aligned(16))) unsigned char s_dyn[];
  uint64_t* const s_keys = reinterpret_cast<uint64_t*>(s_dyn);
  uint16_t* const s_pair = reinterpret_cast<uint16_t*>(s_dyn + (size_t)a.pair_cap * 8);
  const int e = (int)blockIdx.x, lane = (int)threadIdx.x, N = a.N;
  const bool has = lane < N;
  const long long oa = (long long)e * N + (has ? lane : 0);
  const int act = has ? load_action(a.actions, a.act_dtype, oa) : 4;
  if (__ballot(has && (act < 0 || act > 4))) {  // the step skipped this env: nothing of it is repaired
    if (lane == 0) a.flags[e] = 0;
    return;
  }
  Env v{a, a.bits + (a.map_shared ? 0 : (long long)e * a.map_stride), lane, has, 0, 0, 0, 0, act};
  v.orow = has ? a.old_pos[2 * oa] : -1 - lane;  // (an idle lane's cell equals no other)
  v.ocol = has ? a.old_pos[2 * oa + 1] : -1;
  v.crow = has ? a.pos[2 * oa] : -1 - lane;
  v.ccol = has ? a.pos[2 * oa + 1] : -1;
  int nvec = check_node(v, N);
  uint64_t partners;
  int evec = check_edge(v, N, partners);
  const bool any_node = __ballot(nvec > 0) != 0, any_edge = __ballot(evec > 0) != 0;
  if (!any_node && !any_edge) {
    if (lane == 0) {
      a.flags[e] = 0;
      if (a.rounds) a.rounds[2 * e] = a.rounds[2 * e + 1] = 0;
    }
    return;
  }
  const Tab tb{s_key, s_cnt};
  const uint64_t base = a.seed ^ ((uint64_t)(a.env_offset + e) * RK_ENV) ^ ((uint64_t)(uint32_t)a.t[e] * RK_T);
  // the raw pair set (:246), numbered in ascending (i, j), i < j: lane i owns its pairs
  int n_pairs = 0;
  if (any_edge) {
    const uint64_t upper = partners & ~((2ull << lane) - 1ull);
    const int mine = __popcll(upper);
    int before = 0;
    for (int k = 0; k < N; ++k) {
      const int c = __shfl(mine, k);
      before += k < lane ? c : 0;
      n_pairs += c;
    }
    int item = before;
    for (uint64_t m = upper; m; m &= m - 1) s_pair[item++] = (uint16_t)((lane << 8) | __builtin_ctzll(m));
  }
  int flags = 0, r_node = 0, r_edge = 0;
  if (any_node) {
    flags |= F_NODE_RAN;
    bool left = true;
    while (left && r_node < a.max_rounds) {
      solve_node(tb, v, N, base, (uint32_t)r_node, nvec);
      nvec = check_node(v, N);
      left = __ballot(nvec > 0) != 0;
      ++r_node;
    }
    if (left) flags |= F_NODE_CAP;
  }
  if (any_edge && !(flags & F_NODE_CAP)) {
    flags |= F_EDGE_RAN;
    bool left = true;
    while (left && r_edge < a.max_rounds) {
      solve_edge(tb, v, base, (uint32_t)r_edge, s_keys, s_pair, n_pairs);
      evec = check_edge(v, N, partners);
      left = __ballot(evec > 0) != 0;
      ++r_edge;
    }
    if (left) flags |= F_EDGE_CAP;
  }
  // a swap on the final positions: the last edge check where the edge phase ran, else one
  // more (the node phase may have created a swap that no phase then looks at); its vector is
  // not stored
  if (flags & F_EDGE_RAN) {
    if (flags & F_EDGE_CAP) flags |= F_SWAP_LEFT;
  } else {
    uint64_t unused;
    const int fin = check_edge(v, N, unused);
    if (__ballot(fin > 0)) flags |= F_SWAP_LEFT;
  }
  if (has) {
    a.pos[2 * oa] = v.crow;
    a.pos[2 * oa + 1] = v.ccol;
    a.node[oa] = (uint8_t)nvec;
    a.edge[oa] = evec;
  }
  if (lane == 0) {
    a.flags[e] = (uint8_t)flags;
    if (a.rounds) {
      a.rounds[2 * e] = r_node;
      a.rounds[2 * e + 1] = r_edge;
    }
  }
}

}  // namespace

extern "C" {

int mapfx_partial_repair_offered(const mapfx_partial_t* h) {
  mapfx_partial_shape s;
  return (h && mapfx_partial_shape_of(h, &s) == MAPFX_OK && !s.big) ? 1 : 0;
}

int mapfx_partial_repair(mapfx_partial_t* h, const mapfx_partial_state* st, const mapfx_partial_repair_args* ra,
                         const mapfx_partial_out* out, void* stream) {
  if (!h) return perr(MAPFX_EINVAL, "NULL handle");
  int rc = mapfx_partial_check_state(h, st);
  if (rc) return rc;
  if (!ra) return perr(MAPFX_EINVAL, "NULL mapfx_partial_repair_args");
  if (!ra->old_pos || !ra->actions || !ra->flags)
    return perr(MAPFX_EINVAL, "mapfx_partial_repair_args: old_pos, actions and flags are required");
  if (ra->action_dtype < MAPFX_I8 || ra->action_dtype > MAPFX_I64) return perr(MAPFX_EINVAL, "bad action_dtype");
  if (ra->max_rounds < 1 || ra->max_rounds > 16)
    return perr(MAPFX_EINVAL, "mapfx_partial_repair_args: max_rounds must be in 1..16");
  mapfx_partial_shape s;
  rc = mapfx_partial_shape_of(h, &s);
  if (rc) return rc;
  if (s.big)
    return perr(MAPFX_EINVAL, "mapfx_partial_repair is offered for n_agents <= 64 and sides <= 256 only");
  if (s.E == 0) return MAPFX_OK;
  RepArgs a;
  memset(&a, 0, sizeof(a));
  a.H = s.H;
  a.W = s.W;
  a.N = s.N;
  a.map_shared = s.map_shared;
  a.map_stride = s.map_stride;
  a.env_offset = s.env_offset;
  a.seed = ra->seed;
  a.max_rounds = ra->max_rounds;
  a.pair_cap = 2;
  while (a.pair_cap < s.N * (s.N - 1) / 2) a.pair_cap <<= 1;  // <= PAIR_MAX at N <= 64
  a.pos = st->pos;
  a.old_pos = ra->old_pos;
  a.node = st->node;
  a.edge = st->edge;
  a.t = st->t;
  a.bits = st->map_bits;
  a.actions = ra->actions;
  a.act_dtype = ra->action_dtype;
  a.flags = ra->flags;
  a.rounds = ra->rounds;
  rc = launch_kernel(partial_repair_kernel, dim3((unsigned)s.E), dim3(64), (unsigned)a.pair_cap * 10u, (hipStream_t)stream, nullptr, nullptr,
                     "partial_repair_kernel launch", NOTED, a);
  if (rc || !out) return rc;
  // the observations of the repaired state; the pass also refreshes the carried goal
  // distances (pdist / pnbr), stale where an agent was moved
  mapfx_partial_out o = *out;
  o.reward = nullptr;
  rc = mapfx_partial_observe(h, st, &o, stream);
  mapfx_note_kernel((const void*)partial_repair_kernel);
  return rc;
}

}  // extern "C"
