// primal.hip -- MI355X (gfx950) batched PRIMAL sequential dynamics.
//
// MARL-curve-main/src/envs/mapf_primal.py (paths below relative to it):
// MAPFEnv._step((agent_id, action)) :549-637 moves ONE agent against the current
// world (State.moveAgent :103-135: out of bounds -1, wall -2, robot -3, else move;
// status 1 on / reached goal, 2 left goal, 0 otherwise), prices it with the
// reward table :579-596, and returns _observe (:343-386), world.done (:159-166),
// _listNextValidActions (:639-667), on_goal and valid.  Calls are sequential: a
// later call sees the moves of the earlier ones.
//
// One lane group of 16, 32 or 64 lanes per world, 64 / lw worlds per wave.  The
// world lives in LDS as a PADDED byte map (bit 0 agent, bit 1 wall or outside the
// grid: PRIMAL's state array, :38-45, with the out-of-bounds test of :356-359 as a
// border of walls) and the agents' (position, goal) records; each lane also holds
// its own agents (and, for DIAGONAL_MOVEMENT, their past positions) in registers.
// Per call every lane of the world resolves State.moveAgent itself from broadcast
// LDS reads (no status hand-off), then produces 4 bytes of each observation plane
// with SWAR on one realigned map dword (s even: a plane row of s cells is s / 4
// dwords, so lane m writes cells 4m .. 4m + 3 of each plane with ONE dword store),
// stamps the visible agents' clamped goals into a per-world window image, and the
// world's scalar outputs (reward, done, next-action mask, on_goal, valid, goal
// vector) are staged in LDS and leave once per 64-call block as coalesced runs.
// The goal-vector magnitude comes from a host libm pow LUT, as the reference
// computes `(dx**2 + dy**2) ** .5` (quirk 8).
#include <hip/hip_ext.h>
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <memory>
#include <new>

#include "internal.h"
#include "mapfx.h"
#include "mapfx_primal.h"

namespace {

constexpr double ACTION_COST = -0.3, IDLE_COST = -.5, GOAL_REWARD = 0.0, COLLISION_REWARD = -2.;  // :25

struct QGeo {
  int H, W, N, E, s, map_shared;
  long long map_stride;
  int hw, bits_words, lut_n;
  int lw, lw_shift, wreg;  // lanes per world (16 / 32 / 64), log2, LDS bytes per world
  int P, PW, rows;         // padded byte map: rows x PW, interior at (P, P); P >= max(1, s / 2)
  int off_bm, off_goals, off_ag, off_pair, off_pend, off_rst, off_fst;  // regions of a world
  int diag, nact, apl;     // DIAGONAL_MOVEMENT, actions (5 / 9), agents per lane
  uint64_t m_s, m_ss;      // fastdiv magics (odd s path)
  // primal_seq_kernel (world per wave): LDS regions and size; seq = 0 when not eligible
  int seq, off_gl, off_snap, off_psnap, off_bstr, lds_seq;
};

struct QArgs {
  int32_t* pos;
  const int32_t* goal;
  const uint8_t* bits;
  int32_t* past;
  const int32_t* ids;
  const int32_t* acts;
  int K;
  double* reward;
  uint8_t* done;
  uint8_t* next_mask;
  uint8_t* on_goal;
  uint8_t* valid;
  uint8_t* obs;
  double* vec;
  int32_t* err;
  const double* pow_lut;  // (double)n ** .5 by host libm pow, n = 0 .. lut_n-1
};

// dirDict (:28) as 2-bit fields of (d + 1), action a at bits 2a:
// a:      0  1  2  3  4  5  6  7  8
// row+1:  1  1  2  1  0  2  2  0  0      col+1:  1  2  1  0  1  2  0  0  2
constexpr uint32_t DR1 = 1u | 1u << 2 | 2u << 4 | 1u << 6 | 0u << 8 | 2u << 10 | 2u << 12 | 0u << 14 | 0u << 16;
constexpr uint32_t DC1 = 1u | 2u << 2 | 1u << 4 | 0u << 6 | 1u << 8 | 2u << 10 | 0u << 12 | 0u << 14 | 2u << 16;
__device__ inline int dir_r(int a) { return (int)((DR1 >> (2 * a)) & 3u) - 1; }
__device__ inline int dir_c(int a) { return (int)((DC1 >> (2 * a)) & 3u) - 1; }
// opposite_actions (:26): 1<->3, 2<->4, 5<->7, 6<->8; 0 has none
__device__ inline int opposite(int a) { return a == 0 ? -1 : (a <= 4 ? ((a + 1) & 3) + 1 : ((a - 3) & 3) + 5); }
// the action whose direction is (dr, dc), |dr|, |dc| <= 1 (index (dr + 1) * 3 + dc + 1), 0 for (0, 0)
constexpr uint64_t ACT_OF = 7ull | 4ull << 4 | 8ull << 8 | 3ull << 12 | 0ull << 16 | 1ull << 20 |
                            6ull << 24 | 2ull << 28 | 5ull << 32;

// S: observation size fixed at compile time (0: g.s); LS: log2(lanes per world);
// DIAG: DIAGONAL_MOVEMENT; MA: agents per lane held in registers (>= g.apl).
template <int S_, int LS, bool DIAG, int MA>
__global__ void __launch_bounds__(64) primal_act_kernel(QGeo g, QArgs a) {
  extern __shared__ __align__(16) unsigned char lds[];
  constexpr int lw = 1 << LS;
  constexpr int NDIR = DIAG ? 8 : 4;
  const int lane = threadIdx.x, wl = lane >> LS, ag = lane & (lw - 1), lead = wl << LS;
  const int e = blockIdx.x * (64 >> LS) + wl;
  const bool live = e < g.E;
  const uint64_t wmask = (lw == 64 ? ~0ull : ((1ull << lw) - 1ull)) << lead;
  const int N = g.N, H = g.H, W = g.W, P = g.P, PW = g.PW;
  const int s = S_ ? S_ : g.s, ss = s * s, h2 = s / 2;
  const int apl = MA == 1 ? 1 : g.apl;
  unsigned char* wr = lds + wl * g.wreg;
  uint8_t* cm = wr;                                   // [rows][PW] agent | wall << 1
  const uint32_t* cm32 = (const uint32_t*)wr;
  uint32_t* bm = (uint32_t*)(wr + g.off_bm);          // obstacle bitmap (set-up only)
  uint8_t* gim = wr + g.off_goals;                    // [s*s] visible goals of the call
  int4* agL = (int4*)(wr + g.off_ag);                 // [N] {row, col, goal row, goal col}
  int2* pairL = (int2*)(wr + g.off_pair);             // [64] a block's (agent id, action)
  int2* pend = (int2*)(wr + g.off_pend);              // [64] goal vector (dx, dy) of a block's calls
  double* rst = (double*)(wr + g.off_rst);            // [64] rewards of a block's calls
  uint8_t* fst = wr + g.off_fst;                      // [5][64] done, on_goal, valid, mask lo / hi

  // ---- agents: lane ag owns agents ag + r * lw (registers) and their LDS records ----
  int px[MA], py[MA], gx[MA], gy[MA], qx[MA], qy[MA];
  bool has[MA];
#pragma unroll
  for (int r = 0; r < MA; ++r) {
    const int b = ag + r * lw;
    has[r] = live && r < apl && b < N;
    px[r] = py[r] = gx[r] = gy[r] = qx[r] = qy[r] = -(1 << 20);  // far outside every window
    if (has[r]) {
      const long long i = (long long)e * N + b;
      const int2 p = ((const int2*)a.pos)[i], q = ((const int2*)a.goal)[i];
      px[r] = p.x, py[r] = p.y, gx[r] = q.x, gy[r] = q.y;
      if constexpr (DIAG) {
        const int2 pp = ((const int2*)a.past)[i];
        qx[r] = pp.x, qy[r] = pp.y;
      }
      agL[b] = make_int4(p.x, p.y, q.x, q.y);
    }
  }
  if (live) {
    const uint32_t* src = (const uint32_t*)(a.bits + (g.map_shared ? 0 : (long long)e * g.map_stride));
    for (int w = ag; w < g.bits_words; w += lw) bm[w] = src[w];
    for (int i = ag; i < (ss + 3) >> 2; i += lw) ((uint32_t*)gim)[i] = 0u;
  }
  wave_fence();
  // ---- the padded map: 4 cells per dword, walls from the bitmap, border = wall ----
  if (live) {
    const int wpr = PW >> 2, nwd = g.rows * wpr;
    for (int wi = ag; wi < nwd; wi += lw) {
      const int pr = wi / wpr;
      const int r = pr - P, c0 = (wi - pr * wpr) * 4 - P;
      uint32_t v = 0;
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const int c = c0 + t;
        const bool in = r >= 0 && r < H && c >= 0 && c < W;
        const int idx = in ? r * W + c : 0;
        const bool wall = !in || ((bm[idx >> 5] >> (idx & 31)) & 1u);
        v |= (wall ? 2u : 0u) << (8 * t);
      }
      ((uint32_t*)cm)[wi] = v;
    }
  }
  wave_fence();
  int ngoal = 0;  // agents on their goal (State.done :159-166 is ngoal == N)
#pragma unroll
  for (int r = 0; r < MA; ++r) {
    if (has[r]) cm[(px[r] + P) * PW + py[r] + P] = 1;  // agents start on free cells
    ngoal += __popcll(__ballot(has[r] && px[r] == gx[r] && py[r] == gy[r]) & wmask);
  }
  wave_fence();

  // ---- per-lane constants of the observation planes (s even) ----
  // lane m < s*s/4 writes cells 4m .. 4m+3 of each plane: nlow of them in window row
  // y0 from column x0, the rest at the start of row y0 + 1 (o2; = o1 when none)
  const bool even = (s & 1) == 0;
  const int D = even ? ss >> 2 : ss;  // dwords a call writes per plane (even) / per record (odd)
  constexpr int RW = 4;               // rounds held in registers (host: D <= 4 lw for even s)
  int o1[RW], o2[RW];
  uint32_t lom[RW];
#pragma unroll
  for (int rr = 0; rr < RW; ++rr) {
    const int m = ag + rr * lw;
    const int c4 = 4 * m, y0 = c4 / s, x0 = c4 - y0 * s, nlow = min(4, s - x0);
    o1[rr] = y0 * PW + x0;
    o2[rr] = nlow < 4 ? (y0 + 1) * PW + x0 - s : o1[rr];
    lom[rr] = nlow >= 4 ? ~0u : (1u << (8 * nlow)) - 1u;
  }
  const bool probe = ag >= 1 && ag <= NDIR;
  const int pofs = probe ? dir_r(ag) * PW + dir_c(ag) : 0;

  const long long e0k = (long long)e * a.K;
  int kstop = live ? a.K : 0;  // calls of this world from kstop on are not run (bad call)
  for (int kb = 0; kb < a.K; kb += 64) {
    const int kend = min(a.K, kb + 64);
    // the block's (id, action) pairs -> LDS: one load wait per 64 calls (on gfx9
    // vmcnt also counts stores, so a wait drains the earlier calls' outputs)
    if (kb < kstop)
      for (int j = ag; j < kend - kb; j += lw) pairL[j] = make_int2(a.ids[e0k + kb + j], a.acts[e0k + kb + j]);
    wave_fence();
    int2 pa = pairL[0];
    for (int k = kb; k < kend; ++k) {
      const int2 nxt = pairL[min(k + 1 - kb, 63)];  // the next call's pair, read ahead
      const int aid = pa.x - 1, act = pa.y;
      pa = nxt;
      if (k >= kstop) continue;  // (uniform within a world)
      if (aid < 0 || aid >= N || act < 0 || act >= g.nact) {  // the reference asserts (:556-558)
        if (ag == 0 && a.err) atomicCAS(a.err, 0, e + 1);
        kstop = k;
        continue;
      }
      // ---- State.moveAgent (:103-135), resolved by every lane of the world ----
      const int4 A = agL[aid];  // broadcast read: aid's (row, col, goal row, goal col)
      const int nx = A.x + dir_r(act), ny = A.y + dir_c(act);
      const bool inb = nx < H && nx >= 0 && ny < W && ny >= 0;
      const uint32_t tv = cm[(nx + P) * PW + ny + P];  // |d| <= 1 <= P: inside the padded map
      bool dcol = false;
      if constexpr (DIAG) {  // diagonalCollision (:77-99) against the PRE-move positions
        const int sx = A.x + nx, sy = A.y + ny;
        bool hit = false;
#pragma unroll
        for (int r = 0; r < MA; ++r)
          hit |= has[r] && ag + r * lw != aid && qx[r] + px[r] == sx && qy[r] + py[r] == sy;
        dcol = (__ballot(hit) & wmask) != 0;
      }
      const bool wall = (tv & 2u) != 0, robot = (tv & 1u) != 0;
      const bool moved = act != 0 && inb && !wall && !robot && !dcol;
      const bool on_old = A.z == A.x && A.w == A.y, on_new = A.z == nx && A.w == ny;
      const int st_blocked = !inb ? -1 : (wall ? -2 : -3);  // out of bounds, wall, robot / diagonal
      const int status = act == 0 ? (on_old ? 1 : 0) : (moved ? (on_new ? 1 : (on_old ? 2 : 0)) : st_blocked);
      const int cx = moved ? nx : A.x, cy = moved ? ny : A.y;
      ngoal += (moved && on_new ? 1 : 0) - (moved && on_old ? 1 : 0);
      if (moved && ag == 0) {
        cm[(A.x + P) * PW + A.y + P] = 0;
        cm[(nx + P) * PW + ny + P] = 1;
        *(int2*)&agL[aid] = make_int2(nx, ny);
      }
#pragma unroll
      for (int r = 0; r < MA; ++r) {
        if (ag + r * lw == aid) {
          if constexpr (DIAG) {
            if (act == 0 || moved) qx[r] = A.x, qy[r] = A.y;  // agents_past (:110-112, :129-131)
          }
          px[r] = cx, py[r] = cy;
        }
      }
      wave_fence();
      // ---- _observe (:343-386) on the post-move world, next valid actions ----
      const int tr = cx - h2, tc = cy - h2;
      const int base = (tr + P) * PW + tc + P;  // first window cell in the padded map
      const int gq = (A.z >= tr && A.z < tr + s && A.w >= tc && A.w < tc + s)
                         ? (A.z - tr) * s + (A.w - tc) : -(1 << 20);  // own goal's window cell
      uint32_t V[RW];
      if (a.obs && even) {
#pragma unroll
        for (int rr = 0; rr < RW; ++rr) {
          V[rr] = 0;
          if (rr * lw < D && ag + rr * lw < D) {
            const int A1 = base + o1[rr], A2 = base + o2[rr];
            const uint32_t v1 = __builtin_amdgcn_alignbyte(cm32[(A1 >> 2) + 1], cm32[A1 >> 2], A1 & 3);
            const uint32_t v2 = __builtin_amdgcn_alignbyte(cm32[(A2 >> 2) + 1], cm32[A2 >> 2], A2 & 3);
            V[rr] = (v1 & lom[rr]) | (v2 & ~lom[rr]);
          }
        }
      }
      bool ok = false;  // _listNextValidActions (:639-667): lane d probes action d
      if (probe) ok = cm[(cx + P) * PW + cy + P + pofs] == 0;  // in bounds, no wall, no robot
      uint32_t dmask = 0;  // DIAG: directions refused by diagonalCollision from (cx, cy)
#pragma unroll
      for (int r = 0; r < MA; ++r) {
        const int b = ag + r * lw;
        if (a.obs && has[r] && b != aid && px[r] >= tr && px[r] < tr + s && py[r] >= tc && py[r] < tc + s) {
          const int mr = max(tr, min(tr + s - 1, gx[r])), mc = max(tc, min(tc + s - 1, gy[r]));
          gim[(mr - tr) * s + (mc - tc)] = 1;  // a visible agent's goal, clamped into view (:374-378)
        }
        if constexpr (DIAG) {
          const int sx = qx[r] + px[r] - 2 * cx, sy = qy[r] + py[r] - 2 * cy;
          if (has[r] && b != aid && sx >= -1 && sx <= 1 && sy >= -1 && sy <= 1)
            dmask |= 1u << (uint32_t)((ACT_OF >> (4 * ((sx + 1) * 3 + sy + 1))) & 0xFu);
        }
      }
      uint32_t mask = 1u | ((uint32_t)(__ballot(ok) >> lead) & (NDIR == 8 ? 0x1FEu : 0x1Eu));
      if constexpr (DIAG) {
#pragma unroll
        for (int d = 1; d <= 8; ++d)
          if (__ballot((dmask >> d) & 1u) & wmask) mask &= ~(1u << d);
      }
      const int opp = opposite(act);
      if (opp > 0) mask &= ~(1u << opp);
      wave_fence();
      if (a.obs) {
        uint8_t* o = a.obs + (e0k + k) * 4 * ss;
        if (even) {
#pragma unroll
          for (int rr = 0; rr < RW; ++rr) {
            const int m = ag + rr * lw;
            if (rr * lw < D && m < D) {
              uint32_t* g32 = (uint32_t*)gim + m;
              const uint32_t gw = *g32;
              *g32 = 0u;  // clear for the next call (in order before its stamps)
              const int d = gq - 4 * m;
              const uint32_t g4 = (uint32_t)d < 4u ? 1u << (8 * d) : 0u;
              uint32_t* o32 = (uint32_t*)(o + 4 * m);
              o32[0] = V[rr] & 0x01010101u;              // poss: own and other agents (:363-372)
              o32[ss >> 2] = g4;                         // goal (:366-368)
              o32[ss >> 1] = gw;                         // goals of visible agents (:374-378)
              o32[3 * (ss >> 2)] = (V[rr] >> 1) & 0x01010101u;  // obstacles, outside = 1 (:356-362)
            }
          }
        } else {  // odd s: record dword m, byte by byte (plane = byte / s^2)
          for (int m = ag; m < ss; m += lw) {
            uint32_t w = 0;
#pragma unroll
            for (int t = 0; t < 4; ++t) {
              const int b = 4 * m + t;
              const int pl = fastdiv(b, g.m_ss), i = b - pl * ss;
              const int y = fastdiv(i, g.m_s), x = i - y * s;
              const uint32_t v = cm[base + y * PW + x];
              uint32_t bv;
              if (pl == 0) bv = v & 1u;
              else if (pl == 1) bv = i == gq ? 1u : 0u;
              else if (pl == 2) {
                bv = gim[i];
                gim[i] = 0;
              } else bv = (v >> 1) & 1u;
              w |= bv << (8 * t);
            }
            ((uint32_t*)o)[m] = w;
          }
        }
      }
      if (ag == 0) {
        // ---- reward (:579-596), JOINT = False; the stay-on-goal blocking term is added
        //      afterwards by mapfx_primal_blocking (0 when that pass is not run) ----
        const double rew = act == 0 ? (status == 1 ? GOAL_REWARD + 0 : IDLE_COST)
                                    : status == 1 ? GOAL_REWARD : status < 0 ? COLLISION_REWARD : ACTION_COST;
        const int j = k - kb;
        rst[j] = rew;
        fst[j] = ngoal == N ? 1 : 0;                          // world.done() (:626)
        fst[64 + j] = (cx == A.z && cy == A.w) ? 1 : 0;       // on_goal (:633)
        fst[128 + j] = status >= 0 ? 1 : 0;                   // valid_action (:566)
        fst[192 + j] = (uint8_t)mask;
        if constexpr (DIAG) fst[256 + j] = (uint8_t)(mask >> 8);
        pend[j] = make_int2(A.z - cx, A.w - cy);              // goal vector (:379-384), LUT later
      }
    }
    wave_fence();
    // ---- the block's staged outputs, calls kb .. min(kend, kstop) - 1, as runs ----
    const int n = min(kend, kstop) - kb;
    const long long o0 = e0k + kb;
    for (int j = ag; j < n; j += lw) {
      if (a.reward) a.reward[o0 + j] = rst[j];
      if (a.done) a.done[o0 + j] = fst[j];
      if (a.on_goal) a.on_goal[o0 + j] = fst[64 + j];
      if (a.valid) a.valid[o0 + j] = fst[128 + j];
      if (a.next_mask) {
        if constexpr (DIAG) ((uint16_t*)a.next_mask)[o0 + j] = (uint16_t)(fst[192 + j] | (fst[256 + j] << 8));
        else a.next_mask[o0 + j] = fst[192 + j];
      }
      if (a.vec) {
        const int2 d = pend[j];
        const double mag = a.pow_lut[d.x * d.x + d.y * d.y];
        double vx = (double)d.x, vy = (double)d.y;
        if (mag != 0.0) {
          vx = vx / mag;
          vy = vy / mag;
        }
        double* v = a.vec + (o0 + j) * 3;
        v[0] = vx;
        v[1] = vy;
        v[2] = mag;
      }
    }
    wave_fence();
  }
#pragma unroll
  for (int r = 0; r < MA; ++r) {
    if (!has[r]) continue;
    const long long i = (long long)e * N + ag + r * lw;
    ((int2*)a.pos)[i] = make_int2(px[r], py[r]);
    if constexpr (DIAG) ((int2*)a.past)[i] = make_int2(qx[r], qy[r]);
  }
}

// ---------------------------------------------------------------------------
// primal_seq_kernel<S, DIAG>: one world per wave, the calls of a 64-call block in two
// phases (even s in 4..10, N <= 64, H + 2P <= 64, W + 2P <= 64).
//
// The only truly sequential part of _step is State.moveAgent (:103-135): whether call
// k's move happens depends on the positions the earlier calls left.  Everything else a
// call returns (_observe :343-386, done :159-166, _listNextValidActions :639-667, the
// reward :579-596) is a function of the positions right after the call.  So:
//
//   phase A (the chain, wave-uniform, no LDS on it): lane j holds agent j's position;
//     per call the moved agent's position and the target row's wall mask are
//     v_readlane'd, the robot test is a ballot of lane compares (DIAG: the midpoint
//     test of diagonalCollision :77-99 is a second ballot), the move is a v_cndmask
//     on lane aid.  The call leaves its (old position, moved) in lane k of a log
//     register and every agent's post-call position in a [64][N] u16 LDS snapshot;
//   phase B (parallel, lane k = call k): each lane rebuilds its call's status, reward,
//     done, next-action mask and goal vector from the log and the snapshot, and its
//     call's four observation planes as four S*S-bit masks (walls from padded row
//     masks, agents and clamped goals set bit by bit from the snapshot); the 4*S*S-bit
//     string of call k goes to LDS, and the wave expands strings to bytes (one bit ->
//     one byte, 16 bits per lane-chunk) and writes the block's records as one
//     contiguous run of 16-byte stores.
// ---------------------------------------------------------------------------
__device__ __forceinline__ uint32_t readlane_u32(uint32_t v, int l) {
  return (uint32_t)__builtin_amdgcn_readlane((int)v, l);
}

// acc |= bit idx (idx < 128; 127 is the "nothing" sentinel, masked off later)
__device__ __forceinline__ void set_bit128(uint32_t (&acc)[4], uint32_t idx) {
  const uint32_t b = 1u << (idx & 31u), w = idx >> 5;
#pragma unroll
  for (int i = 0; i < 4; ++i) acc[i] |= (w == (uint32_t)i) ? b : 0u;
}

// str |= v at compile-time bit offset B (v has no bits at or above `bits`)
template <int B, int NSW>
__device__ __forceinline__ void put_at(uint32_t (&str)[NSW], uint32_t v) {
  constexpr int w = B >> 5, sh = B & 31;
  if constexpr (w < NSW) str[w] |= v << sh;
  if constexpr (sh != 0 && w + 1 < NSW) str[w + 1] |= v >> (32 - sh);
}

template <int P0, int SS, int NSW>
__device__ __forceinline__ void put_plane(uint32_t (&str)[NSW], const uint32_t (&pl)[4]) {
  put_at<P0, NSW>(str, SS >= 32 ? pl[0] : (pl[0] & ((1u << (SS & 31)) - 1u)));
  if constexpr (SS > 32) put_at<P0 + 32, NSW>(str, SS >= 64 ? pl[1] : (pl[1] & ((1u << (SS & 31)) - 1u)));
  if constexpr (SS > 64) put_at<P0 + 64, NSW>(str, SS >= 96 ? pl[2] : (pl[2] & ((1u << (SS & 31)) - 1u)));
  if constexpr (SS > 96) put_at<P0 + 96, NSW>(str, pl[3] & ((1u << (SS & 31)) - 1u));
}

#ifndef MAPFX_QABL
#define MAPFX_QABL 0  // diagnostic builds only: 1 no record stores, 2 no phase B, 4 no move chain
#endif
template <int S, bool DIAG>
__global__ void __launch_bounds__(64) primal_seq_kernel(QGeo g, QArgs a) {
  extern __shared__ __align__(16) unsigned char lds[];
  constexpr int SS = S * S, H2 = S / 2;
  constexpr int CPC = SS / 4;              // 16-byte chunks (= 16-bit string pieces) of one call
  constexpr int NSW = (4 * SS + 31) / 32;  // dwords of a call's bit string
  constexpr int NDIR = DIAG ? 8 : 4;
  static_assert(S % 2 == 0 && S >= 4 && SS <= 100, "even S in 4..10");
  const int lane = threadIdx.x, e = blockIdx.x;
  const int N = g.N, H = g.H, W = g.W, P = g.P;
  uint64_t* rowm = (uint64_t*)lds;                   // [H + 2P] padded wall rows
  uint32_t* gl = (uint32_t*)(lds + g.off_gl);        // [N] biased goal cell
  uint16_t* snap = (uint16_t*)(lds + g.off_snap);    // [65][N] cells before call 0, after calls 0..63
  uint16_t* psnap = (uint16_t*)(lds + g.off_psnap);  // DIAG: agents_past, same rows
  uint16_t* bstr = (uint16_t*)(lds + g.off_bstr);    // the block's bit strings, call k at CPC * k
  const int2* goal2 = (const int2*)a.goal + (long long)e * N;  // wave-uniform reads: SGPRs

  // ---- state: lane j = agent j at its BIASED cell (row + P) | (col + P) << 8 (rows and
  //      columns of the padded map, < 64: the cell is its own u16 snapshot value and a
  //      move is one packed add); other lanes hold a value no cell has ----
  const bool agent = lane < N;
  const uint32_t bias = (uint32_t)P | ((uint32_t)P << 8);
  // block 0's calls are loaded first: their latency overlaps the set-up loads
  int id0 = 0, ac0 = 0;
  if (lane < min(64, a.K)) {
    id0 = a.ids[(long long)e * a.K + lane];
    ac0 = a.acts[(long long)e * a.K + lane];
  }
  uint32_t vpos = 0xFFFFFFFFu, vpast = 0u;
  if (agent) {
    const long long i = (long long)e * N + lane;
    const int2 p = ((const int2*)a.pos)[i], q = goal2[lane];
    vpos = ((uint32_t)p.x | ((uint32_t)p.y << 8)) + bias;
    gl[lane] = ((uint32_t)q.x | ((uint32_t)q.y << 8)) + bias;
    if constexpr (DIAG) {
      const int2 pp = ((const int2*)a.past)[i];
      vpast = ((uint32_t)pp.x | ((uint32_t)pp.y << 8)) + bias;
    }
  }
  uint32_t vsum = vpos + vpast;  // DIAG: past + present, the midpoint test's sum (sentinel off-agent)
  // ---- padded wall rows: lane r = padded row r, bit c + P = wall at column c; outside = 1 ----
  uint64_t vrow = ~0ull;
  {
    const int r = lane - P;
    if (r >= 0 && r < H) {
      const uint32_t* w32 = (const uint32_t*)(a.bits + (g.map_shared ? 0 : (long long)e * g.map_stride));
      const int b0 = r * W, wi = b0 >> 5, sh = b0 & 31, last = (b0 + W - 1) >> 5;
      const uint64_t d0 = w32[wi], d1 = wi + 1 <= last ? w32[wi + 1] : 0u, d2 = wi + 2 <= last ? w32[wi + 2] : 0u;
      uint64_t v = (d0 | (d1 << 32)) >> sh;
      if (sh) v |= d2 << (64 - sh);
      const uint64_t fm = ((1ull << W) - 1ull) << P;
      vrow = (~fm) | ((v << P) & fm);
    }
    if (lane < H + 2 * P) rowm[lane] = vrow;
  }
  const uint32_t vrow_lo = (uint32_t)vrow, vrow_hi = (uint32_t)(vrow >> 32);
  wave_fence();

  const long long e0k = (long long)e * a.K;
  int kstop = a.K;
  for (int kb = 0; kb < kstop; kb += 64) {
    const int nb = min(64, a.K - kb);
    // call kb + lane: agent index, action, and the move as one packed add (cells biased,
    // so a row step never borrows from the column byte); the first bad call ends the
    // world's calls (the reference asserts, :556-558)
    int id = id0, ac = ac0;
    if (kb > 0 && lane < nb) {
      id = a.ids[e0k + kb + lane];
      ac = a.acts[e0k + kb + lane];
    }
    const bool okc = lane < nb && (unsigned)(id - 1) < (unsigned)N && (unsigned)ac < (unsigned)g.nact;
    const uint64_t badm = __ballot(lane < nb && !okc);
    const int nv = badm ? (int)__ffsll((unsigned long long)badm) - 1 : nb;
    const int vaid = okc ? id - 1 : 0, vact = okc ? ac : 0;
    const uint32_t vdel = okc ? (uint32_t)(dir_r(ac) + dir_c(ac) * 256) : 0u;
    // ================= phase A: State.moveAgent, call after call =================
    // snapshot rows: row 0 = the cells before call kb, row kk + 1 = after call kb + kk;
    // agent lanes write slot [row][lane], the others one spare slot past the rows
    uint32_t saddr = agent ? 2u * (uint32_t)lane : 2u * 65u * (uint32_t)N;
    const uint32_t sinc = agent ? 2u * (uint32_t)N : 0u;
    *(uint16_t*)((unsigned char*)snap + saddr) = (uint16_t)vpos;
    if constexpr (DIAG) *(uint16_t*)((unsigned char*)psnap + saddr) = (uint16_t)vpast;
    saddr += sinc;
    for (int kk = 0; kk < nv; ++kk) {
      if (MAPFX_QABL & 4) {
        *(uint16_t*)((unsigned char*)snap + saddr) = (uint16_t)vpos;
        saddr += sinc;
        continue;
      }
      const int aid = __builtin_amdgcn_readlane(vaid, kk);
      const uint32_t d = readlane_u32(vdel, kk);
      const uint32_t o = readlane_u32(vpos, aid), t = o + d;
      const int rs = (int)(t & 0xFFu);  // padded row of the target (outside = wall)
      const uint64_t wr = ((uint64_t)readlane_u32(vrow_hi, rs) << 32) | readlane_u32(vrow_lo, rs);
      // wall / outside, or an agent on the target (a stay hits itself)
      uint64_t blk = ((wr >> (t >> 8)) & 1ull) | __ballot(vpos == t);
      if constexpr (DIAG) blk |= __ballot(vsum == o + t && vpos != o);  // (vpos == o: agent aid)
      uint32_t tm = blk == 0 ? t : o;  // agent aid's cell after the call
      asm volatile("" : "+s"(tm));      // (uniform, computed before the select: no exec branch)
      const bool me = vpos == o;        // (cells are distinct: only lane aid)
      if constexpr (DIAG) vpast = (me && (d == 0u || tm != o)) ? o : vpast;  // agents_past (:110-112, :129-131)
      vpos = me ? tm : vpos;
      if constexpr (DIAG) vsum = vpos + vpast;
      *(uint16_t*)((unsigned char*)snap + saddr) = (uint16_t)vpos;
      if constexpr (DIAG) *(uint16_t*)((unsigned char*)psnap + saddr) = (uint16_t)vpast;
      saddr += sinc;
    }
    if (nv < nb) {
      if (lane == 0 && a.err) atomicCAS(a.err, 0, e + 1);
      kstop = kb + nv;
    }
    wave_fence();
    // ================= phase B: lane k = call kb + k =================
    if (MAPFX_QABL & 2) continue;
    const bool cv = lane < nv;
    const int aid = vaid, act = vact;
    // call k's cell before / after it: snapshot rows k and k + 1 (lanes without a call: the
    // biased (0, 0), so the reads below stay inside the padded map)
    const uint32_t ob = cv ? (uint32_t)snap[lane * N + aid] : bias;
    const uint32_t cb = cv ? (uint32_t)snap[(lane + 1) * N + aid] : bias;
    const uint32_t tb = ob + vdel;
    const bool moved = cb != ob;
    const int cxb = (int)(cb & 0xFFu), cyb = (int)(cb >> 8);
    const bool inb = (unsigned)((int)(tb & 0xFFu) - P) < (unsigned)H && (unsigned)((int)(tb >> 8) - P) < (unsigned)W;
    const uint32_t gA = gl[aid];
    const int gxb = (int)(gA & 0xFFu), gyb = (int)(gA >> 8);
    const int trb = cxb - H2, tcb = cyb - H2;  // window origin in padded coordinates
    // obstacle plane (:356-362, outside = 1) and the walls of the 3 x 3 around the agent
    uint32_t obsp[4] = {0u, 0u, 0u, 0u};
    uint32_t w9 = 0;
#pragma unroll
    for (int y = 0; y < S; ++y) {
      const uint64_t m = rowm[trb + y];
      const uint32_t bits = (uint32_t)(m >> tcb) & ((1u << S) - 1u);
      const int B = S * y;
      obsp[B >> 5] |= bits << (B & 31);
      if ((B & 31) + S > 32) obsp[(B >> 5) + 1] |= bits >> (32 - (B & 31));
      if (y >= H2 - 1 && y <= H2 + 1) w9 |= ((bits >> (H2 - 1)) & 7u) << (3 * (y - H2 + 1));
    }
    // agents at this call: poss plane (:363-372), visible agents' clamped goals
    // (:374-378), agents on their goal (done), DIAG crossing directions
    uint32_t possp[4] = {0u, 0u, 0u, 0u}, goalsp[4] = {0u, 0u, 0u, 0u};
    uint32_t dmask = 0;
    int ngoal = 0;
    const uint16_t* sk = snap + (lane + 1) * N;
    const uint16_t* pk = psnap + (lane + 1) * N;
    for (int j = 0; j < N; ++j) {
      const int2 gj = goal2[j];
      const int gjxb = gj.x + P, gjyb = gj.y + P;
      const uint32_t pj = sk[j];
      ngoal += pj == (uint32_t)(gjxb | (gjyb << 8)) ? 1 : 0;
      const int dx = (int)(pj & 0xFFu) - trb, dy = (int)(pj >> 8) - tcb;
      const bool vis = (unsigned)dx < (unsigned)S && (unsigned)dy < (unsigned)S;
      set_bit128(possp, vis ? (uint32_t)(dx * S + dy) : 127u);
      const int mx = min(max(gjxb - trb, 0), S - 1), my = min(max(gjyb - tcb, 0), S - 1);
      set_bit128(goalsp, (vis && j != aid) ? (uint32_t)(mx * S + my) : 127u);
      if constexpr (DIAG) {
        const uint32_t qj = pk[j];
        const int sx = (int)(qj & 0xFFu) + (int)(pj & 0xFFu) - 2 * cxb;
        const int sy = (int)(qj >> 8) + (int)(pj >> 8) - 2 * cyb;
        if (j != aid && sx >= -1 && sx <= 1 && sy >= -1 && sy <= 1)
          dmask |= 1u << (uint32_t)((ACT_OF >> (4 * ((sx + 1) * 3 + sy + 1))) & 0xFu);
      }
    }
    // the 3 x 3 around the agent is inside the window (S >= 4): its occupied cells are
    // poss-plane bits (the centre is the agent itself, never a probe)
    uint32_t nb9 = 0;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      const int B = (H2 - 1 + r) * S + H2 - 1;
      uint32_t v = possp[B >> 5] >> (B & 31);
      if ((B & 31) > 29) v |= possp[(B >> 5) + 1] << (32 - (B & 31));
      nb9 |= (v & 7u) << (3 * r);
    }
    uint32_t goalp[4] = {0u, 0u, 0u, 0u};
    {
      const int dx = gxb - trb, dy = gyb - tcb;
      set_bit128(goalp, ((unsigned)dx < (unsigned)S && (unsigned)dy < (unsigned)S) ? (uint32_t)(dx * S + dy) : 127u);
    }
    // status (State.moveAgent), reward (:579-596), next valid actions (:639-667)
    const bool on_old = gA == ob, on_new = gA == tb;
    const int i9 = (dir_r(act) + 1) * 3 + dir_c(act) + 1;  // target in the 3 x 3 (not moved: c = o)
    const bool wallT = ((w9 >> i9) & 1u) != 0;
    const int st_blocked = !inb ? -1 : (wallT ? -2 : -3);
    const int status = act == 0 ? (on_old ? 1 : 0) : (moved ? (on_new ? 1 : (on_old ? 2 : 0)) : st_blocked);
    const uint32_t blocked9 = w9 | nb9;
    uint32_t mask = 1u;
#pragma unroll
    for (int d = 1; d <= NDIR; ++d) {
      const int id9 = (dir_r(d) + 1) * 3 + dir_c(d) + 1;
      mask |= ((~blocked9 >> id9) & 1u) << d;
    }
    const int opp = opposite(act);
    if (opp > 0) mask &= ~(1u << opp);
    if constexpr (DIAG) mask &= ~(dmask & 0x1FEu);
    if (cv) {
      const long long oi = e0k + kb + lane;
      const double rew = act == 0 ? (status == 1 ? GOAL_REWARD + 0 : IDLE_COST)
                                  : status == 1 ? GOAL_REWARD : status < 0 ? COLLISION_REWARD : ACTION_COST;
      if (a.reward) a.reward[oi] = rew;
      if (a.done) a.done[oi] = ngoal == N ? 1 : 0;
      if (a.on_goal) a.on_goal[oi] = gA == cb ? 1 : 0;
      if (a.valid) a.valid[oi] = status >= 0 ? 1 : 0;
      if (a.next_mask) {
        if constexpr (DIAG) ((uint16_t*)a.next_mask)[oi] = (uint16_t)mask;
        else a.next_mask[oi] = (uint8_t)mask;
      }
      if (a.vec) {  // :379-386, magnitude from the host libm pow LUT
        const int dX = gxb - cxb, dY = gyb - cyb;
        const double mag = a.pow_lut[dX * dX + dY * dY];
        double vx = (double)dX, vy = (double)dY;
        if (mag != 0.0) {
          vx = vx / mag;
          vy = vy / mag;
        }
        double* v = a.vec + oi * 3;
        v[0] = vx;
        v[1] = vy;
        v[2] = mag;
      }
    }
    if (a.obs) {
      uint32_t str[NSW];
#pragma unroll
      for (int i = 0; i < NSW; ++i) str[i] = 0u;
      put_plane<0, SS, NSW>(str, possp);
      put_plane<SS, SS, NSW>(str, goalp);
      put_plane<2 * SS, SS, NSW>(str, goalsp);
      put_plane<3 * SS, SS, NSW>(str, obsp);
      // call k's 4 S^2 bits = 16-bit pieces CPC k .. CPC k + CPC - 1 of one contiguous
      // string: the block's records are one run of bytes, piece c -> record bytes 16c ..
      uint16_t* dst = bstr + CPC * lane;
#pragma unroll
      for (int i = 0; i < CPC; ++i) dst[i] = (uint16_t)(str[i >> 1] >> (16 * (i & 1)));
      wave_fence();
      const uint32_t* b32 = (const uint32_t*)bstr;
      uint4* obase = (uint4*)(a.obs + (e0k + kb) * (4 * SS));
      const int nch = nv * CPC;
      for (int i = lane; 2 * i < nch; i += 64) {
        const uint32_t b = b32[i];
        uint4 v0, v1;
        v0.x = ((b & 15u) * 0x00204081u) & 0x01010101u;
        v0.y = (((b >> 4) & 15u) * 0x00204081u) & 0x01010101u;
        v0.z = (((b >> 8) & 15u) * 0x00204081u) & 0x01010101u;
        v0.w = (((b >> 12) & 15u) * 0x00204081u) & 0x01010101u;
        v1.x = (((b >> 16) & 15u) * 0x00204081u) & 0x01010101u;
        v1.y = (((b >> 20) & 15u) * 0x00204081u) & 0x01010101u;
        v1.z = (((b >> 24) & 15u) * 0x00204081u) & 0x01010101u;
        v1.w = ((b >> 28) * 0x00204081u) & 0x01010101u;
        if (MAPFX_QABL & 1) continue;
        obase[2 * i] = v0;
        if (2 * i + 1 < nch) obase[2 * i + 1] = v1;
      }
    }
    wave_fence();
  }
  if (agent) {
    const long long i = (long long)e * N + lane;
    const uint32_t p = vpos - bias;
    ((int2*)a.pos)[i] = make_int2((int)(p & 0xFFu), (int)(p >> 8));
    if constexpr (DIAG) {
      const uint32_t q = vpast - bias;
      ((int2*)a.past)[i] = make_int2((int)(q & 0xFFu), (int)(q >> 8));
    }
  }
}

}  // namespace

struct mapfx_primal_t {
  QGeo geo;  // (seq layout included)
  double* pow_lut;
  int lds;
  int blocking_flat;  // MAPFX_PRIMAL_BLOCKING=flat: the flat-set blocking kernel at every shape
  int observe_pin;    // MAPFX_PRIMAL_OBSERVE=waves / lanes: 1 the wave-per-query observe kernel at
                      // every shape, 2 the lane-per-query kernel wherever its LDS fits
};

namespace {

using PrimalFn = void (*)(QGeo, QArgs);
struct BArgs;
using PrimalBFn = void (*)(QGeo, BArgs);

template <int S, int LS, bool DIAG>
PrimalFn pick_ma(int apl) {
  if (apl <= 1) return primal_act_kernel<S, LS, DIAG, 1>;
  return primal_act_kernel<S, LS, DIAG, 4>;
}
template <int S, bool DIAG>
PrimalFn pick_ls(int ls, int apl) {
  if (ls == 4) return pick_ma<S, 4, DIAG>(apl);
  if (ls == 5) return pick_ma<S, 5, DIAG>(apl);
  return pick_ma<S, 6, DIAG>(apl);
}
PrimalFn pick_primal(const QGeo& g) {
  if (g.s == 10) return g.diag ? pick_ls<10, true>(g.lw_shift, g.apl) : pick_ls<10, false>(g.lw_shift, g.apl);
  return g.diag ? pick_ls<0, true>(g.lw_shift, g.apl) : pick_ls<0, false>(g.lw_shift, g.apl);
}

template <bool DIAG>
PrimalFn pick_seq_s(int s) {
  if (s == 4) return primal_seq_kernel<4, DIAG>;
  if (s == 6) return primal_seq_kernel<6, DIAG>;
  if (s == 8) return primal_seq_kernel<8, DIAG>;
  return primal_seq_kernel<10, DIAG>;
}
PrimalFn pick_seq(const QGeo& g) { return g.diag ? pick_seq_s<true>(g.s) : pick_seq_s<false>(g.s); }

// primal_seq_kernel eligibility and LDS layout of its one world per block: padded wall
// rows (u64), goals (u32), the [64][N] u16 position (and DIAG past) snapshots, the
// [64][16] u32 bit strings.  Returns the size, 0 when the world does not qualify.
int layout_seq(QGeo& g) {
  const bool ok = g.s % 2 == 0 && g.s >= 4 && g.s <= 10 && g.N <= 64 && g.H + 2 * g.P <= 64 &&
                  g.W + 2 * g.P <= 64;
  if (!ok) return 0;
  int o = round_up((g.H + 2 * g.P) * 8, 16);
  g.off_gl = o;
  o += round_up(4 * g.N, 16);
  g.off_snap = o;
  o += round_up(65 * 2 * g.N + 2, 16);  // 65 rows + the spare slot of the non-agent lanes
  g.off_psnap = o;
  if (g.diag) o += round_up(65 * 2 * g.N + 2, 16);
  g.off_bstr = o;
  o += 64 * 64;
  return o;
}

// LDS layout of one world for lanes-per-world 1 << ls; returns its size.
int layout(QGeo& g) {
  int o = round_up(g.rows * g.PW + 4, 16);  // + the realigning read's overrun
  g.off_bm = o;
  o += round_up(g.bits_words * 4, 16);
  g.off_goals = o;
  o += round_up(g.s * g.s + 4, 16);
  g.off_ag = o;
  o += 16 * g.N;
  g.off_pair = o;
  o += 64 * 8;
  g.off_pend = o;
  o += 64 * 8;
  g.off_rst = o;
  o += 64 * 8;
  g.off_fst = o;
  o += 5 * 64;
  return round_up(o, 16);
}

// ---------------------------------------------------------------------------
// primal_blocking_kernel<ROWS>: get_blocking_reward (:513-546), one 64-lane workgroup
// per (world, call).
//
// The reference asks its planner for ONE robot's optimal 4-connected path twice per
// examined agent j (astar :501-511): with the sitter's cell as an obstacle ("before")
// and without it ("after"), and uses only the two lengths and "no solution".  On an
// unweighted grid that is a pair of BFS distances, so both searches run here as
// bit-parallel floods that share one level loop: "after" stops at its goal level d,
// "before" is cut at level d + 10 (inflation, :519), no distance table is written and
// nothing per level leaves the workgroup.  The level counter is a plain int (a
// serpentine 128 x 128 has paths of thousands of levels).
//
//   ROWS (H <= 64 and W <= 64): lane r holds row r as a 64-bit mask, as
//     partial_bfs_kernel does: left / right are shifts, up / down come from lanes
//     r - 1 / r + 1; the visible robots' row masks are built once per call in LDS.
//   otherwise: one flat H * W-bit set (cell r * W + c = bit, the layout of the obstacle
//     bitmap), up to 256 64-bit words, word lane + 64 t in lane's registers, published
//     to LDS once per level for the neighbours' reads; left / right are shifts by 1
//     under row-edge masks, up / down shifts by W across words.
//
// With a.undo the world call k saw is rebuilt from st->pos after the launch: the valid
// moves of calls k + 1 .. kstop - 1 are subtracted (kstop: the world's first bad call,
// the range test of primal_act_kernel), which needs no order -- the sum of an agent's
// undone moves is the same in any.
// ---------------------------------------------------------------------------
constexpr int BLOCK_INFLATION = 10;   // :519
constexpr double BLOCKING_COST = -1.;  // :25

struct BArgs {
  const int32_t* pos;
  const int32_t* goal;
  const uint8_t* bits;
  const int32_t* ids;
  const int32_t* acts;
  int K;
  const uint8_t* valid;
  const uint8_t* on_goal;
  double* reward;
  uint8_t* blocking;
  int32_t* counts;
  int undo;  // 1: the K calls of an act launch; 0: agent ids[e] at st->pos as it stands (K = 1)
};

// x[i], 0 outside 0 .. nw - 1 (a clamped read and a select: no branch around the load)
__device__ inline uint64_t bw_get(const uint64_t* x, int i, int nw) {
  const uint64_t v = x[min(max(i, 0), nw - 1)];
  return (unsigned)i < (unsigned)nw ? v : 0ull;
}
// word w of the set x moved by +(64 q + r) / -(64 q + r) cells (0 <= r < 64)
__device__ inline uint64_t bw_up(const uint64_t* x, int w, int q, int r, int nw) {
  const uint64_t lo = bw_get(x, w - q - 1, nw) >> ((64 - r) & 63);
  return (bw_get(x, w - q, nw) << r) | (r ? lo : 0ull);
}
__device__ inline uint64_t bw_down(const uint64_t* x, int w, int q, int r, int nw) {
  const uint64_t hi = bw_get(x, w + q + 1, nw) << ((64 - r) & 63);
  return (bw_get(x, w + q, nw) >> r) | (r ? hi : 0ull);
}
// the 4-connected neighbours of the set x, word w (not yet masked by the free cells)
__device__ inline uint64_t bw_nbr(const uint64_t* x, int w, int nw, int q, int r, uint64_t nc0, uint64_t ncl) {
  return (bw_up(x, w, 0, 1, nw) & nc0) | (bw_down(x, w, 0, 1, nw) & ncl) | bw_up(x, w, q, r, nw) |
         bw_down(x, w, q, r, nw);
}
// the neighbours of the rows x (lane = row): same row by shifts, rows r - 1 / r + 1 by shuffles
__device__ inline uint64_t row_nbr(uint64_t x, int lane) {
  const uint64_t up = __shfl_up(x, 1), dn = __shfl_down(x, 1);
  return (x << 1) | (x >> 1) | (lane > 0 ? up : 0ull) | (lane < 63 ? dn : 0ull);
}

// After level L of the two floods (gA / gB: the goal is in the flood, chA / chB: the
// flood grew; "after" is no longer advanced once found): 0 go on, 1 not blocked, 2 blocked.
__device__ inline int bw_verdict(bool& foundA, int& dA, int L, bool gA, bool chA, bool gB, bool chB) {
  if (!foundA) {
    if (__ballot(gA)) foundA = true, dA = L;
    else if (!__ballot(chA)) return 1;  // "after" died out: no path either way (:541-542)
  }
  if (__ballot(gB)) return 1;           // "before" arrives by level d_after + 10
  if (foundA && (L >= dA + BLOCK_INFLATION || !__ballot(chB))) return 2;  // (:543-545)
  return 0;
}

template <bool ROWS>
__global__ void __launch_bounds__(64) primal_blocking_kernel(QGeo g, BArgs a) {
  extern __shared__ __align__(16) unsigned char lds[];
  constexpr int WPL = 4;  // flat words per lane: H * W <= 16384 = 4 * 64 * 64
  const int lane = threadIdx.x, K = a.K, N = g.N, H = g.H, W = g.W;
  const int e = (int)(blockIdx.x / (unsigned)K), k = (int)(blockIdx.x - (unsigned)e * (unsigned)K);
  const long long e0k = (long long)e * K, oi = e0k + k;
  const int nw = ROWS ? 64 : (g.hw + 63) >> 6;
  uint64_t* fre = (uint64_t*)lds;  // ROWS: [64] the visible robots' rows; flat: the free cells
  uint64_t* nc0 = fre + nw;        // flat only: cells not in column 0
  uint64_t* ncl = nc0 + nw;        //            cells not in column W - 1
  uint64_t* curA = ncl + nw;       //            the "after" / "before" floods of the level
  uint64_t* curB = curA + nw;
  int* posr = (int*)(ROWS ? fre + nw : curB + nw);  // [N] rows, [N] columns of the world at this call
  int* posc = posr + N;
  int2* goalL = (int2*)(posc + N);                  // [N] goals

  int n = 0, aid = 0;
  bool run = true;
  if (a.undo)  // a stay (action 0) on the goal, two loads; everything else leaves at once
    run = a.acts[oi] == 0 && a.on_goal[oi] != 0;
  uint64_t frow = 0;  // ROWS: the cells of row `lane` without a wall
  if (run) {
    // ---- set-up.  Everything the call needs from global memory is loaded before the
    //      first use (one round trip): the sitter, the first 64 calls of the world,
    //      positions, goals, the map ----
    aid = a.ids[oi] - 1;
    int id0 = 0, ac0 = 0, va0 = 0;
    if (a.undo && lane < K) {
      id0 = a.ids[e0k + lane];
      ac0 = a.acts[e0k + lane];
      va0 = a.valid[e0k + lane];
    }
    int2 pp[WPL], gg[WPL];  // N <= 255: at most 4 agents per lane
#pragma unroll
    for (int t = 0; t < WPL; ++t) {
      const int i = lane + 64 * t;
      if (i < N) {
        pp[t] = ((const int2*)a.pos)[(long long)e * N + i];
        gg[t] = ((const int2*)a.goal)[(long long)e * N + i];
      }
    }
    const uint32_t* src = (const uint32_t*)(a.bits + (g.map_shared ? 0 : (long long)e * g.map_stride));
    if constexpr (ROWS) {
      if (lane < H) {
        const int b0 = lane * W, wi = b0 >> 5, sh = b0 & 31, last = (b0 + W - 1) >> 5;
        const uint64_t d0 = src[wi], d1 = wi + 1 <= last ? src[wi + 1] : 0u, d2 = wi + 2 <= last ? src[wi + 2] : 0u;
        uint64_t v = (d0 | (d1 << 32)) >> sh;
        if (sh) v |= d2 << (64 - sh);
        frow = ~v & (W == 64 ? ~0ull : (1ull << W) - 1ull);
      }
      fre[lane] = 0ull;
    } else {
      uint64_t wl[WPL];
#pragma unroll
      for (int t = 0; t < WPL; ++t) {
        const int w = lane + 64 * t;
        if (w < nw) wl[t] = (uint64_t)src[2 * w] | ((uint64_t)(2 * w + 1 < g.bits_words ? src[2 * w + 1] : 0u) << 32);
      }
#pragma unroll
      for (int t = 0; t < WPL; ++t) {
        const int w = lane + 64 * t;
        if (w < nw) {
          const int rem = g.hw - 64 * w;
          fre[w] = ~wl[t] & (rem >= 64 ? ~0ull : (1ull << rem) - 1ull);
          nc0[w] = ~0ull;
          ncl[w] = ~0ull;
        }
      }
    }
#pragma unroll
    for (int t = 0; t < WPL; ++t) {
      const int i = lane + 64 * t;
      if (i < N) {
        posr[i] = pp[t].x;
        posc[i] = pp[t].y;
        goalL[i] = gg[t];
      }
    }
    wave_fence();
    if constexpr (!ROWS)
      for (int r = lane; r < H; r += 64) {
        const int i0 = r * W, i1 = i0 + W - 1;
        atomicAnd((unsigned int*)nc0 + (i0 >> 5), ~(1u << (i0 & 31)));
        atomicAnd((unsigned int*)ncl + (i1 >> 5), ~(1u << (i1 & 31)));
      }
    if (a.undo) {
      // the world's first bad call kstop (:556-558; later calls were not executed, their
      // valid / on_goal are stale), and the valid moves of calls k + 1 .. kstop - 1 undone
      // (moved by the action's direction; a stay moves nothing)
      int kstop = K;
      for (int kb = 0; kb < K && kstop == K; kb += 64) {
        const int j = kb + lane;
        int id = id0, ac = ac0, va = va0;
        if (kb > 0 && j < K) {
          id = a.ids[e0k + j];
          ac = a.acts[e0k + j];
          va = a.valid[e0k + j];
        }
        const bool bad = j < K && !((unsigned)(id - 1) < (unsigned)N && (unsigned)ac < (unsigned)g.nact);
        const uint64_t m = __ballot(bad);
        if (m) kstop = kb + (int)__ffsll((unsigned long long)m) - 1;
        if (j > k && j < kstop && va) {
          atomicSub(&posr[id - 1], dir_r(ac));
          atomicSub(&posc[id - 1], dir_c(ac));
        }
      }
      run = k < kstop;
    }
    run = run && (unsigned)aid < (unsigned)N;
    wave_fence();
  }
  if (run) {
    // ---- the window of the sitter (:520-522) and the visible robots 1 .. N - 1 (:523-529:
    //      the loop is range(1, num_agents), so the last agent is neither examined nor an
    //      obstacle) ----
    const int sr = posr[aid], sc = posc[aid];
    const int tr = sr - g.s / 2, tc = sc - g.s / 2;
    auto seen = [&](int r, int c) {
      return r >= tr && r < tr + g.s && c >= tc && c < tc + g.s && (unsigned)r < (unsigned)H &&
             (unsigned)c < (unsigned)W;
    };
    for (int i = lane; i < N - 1; i += 64)
      if (i != aid && seen(posr[i], posc[i])) {
        if constexpr (ROWS) {
          atomicOr((unsigned int*)(fre + posr[i]) + (posc[i] >> 5), 1u << (posc[i] & 31));
        } else {
          const int idx = posr[i] * W + posc[i];
          atomicAnd((unsigned int*)fre + (idx >> 5), ~(1u << (idx & 31)));
        }
      }
    wave_fence();
    const bool sin = (unsigned)sr < (unsigned)H && (unsigned)sc < (unsigned)W;
    if constexpr (ROWS) frow &= ~fre[lane];
    const int q = W >> 6, r = W & 63;
    for (int j = 0; j < N - 1; ++j) {  // (everything below is uniform over the wave)
      if (j == aid) continue;
      const int pr = posr[j], pc = posc[j];
      if (!seen(pr, pc)) continue;
      const int2 gj = goalL[j];
      if ((unsigned)gj.x >= (unsigned)H || (unsigned)gj.y >= (unsigned)W) continue;
      if (pr == gj.x && pc == gj.y) continue;  // both lengths 1
      // "after": walls + the other visible robots; "before": the same + the sitter's cell
      int verdict = 0;
      if constexpr (ROWS) {
        const uint64_t pb = lane == pr ? 1ull << pc : 0ull, gb = lane == gj.x ? 1ull << gj.y : 0ull;
        const uint64_t fA = frow | pb, fB = fA & ~(sin && lane == sr ? 1ull << sc : 0ull);
        if (!__ballot((fA & gb) != 0)) continue;  // the goal cell is an obstacle: no path after
        uint64_t RA = pb, RB = pb;
        bool foundA = false;
        int dA = 0;
        for (int L = 1; !verdict; ++L) {
          bool chA = false, gA = false;
          if (!foundA) {
            const uint64_t nr = RA | (row_nbr(RA, lane) & fA);
            chA = nr != RA;
            RA = nr;
            gA = (nr & gb) != 0;
          }
          const uint64_t nr = RB | (row_nbr(RB, lane) & fB);
          const bool chB = nr != RB;
          RB = nr;
          verdict = bw_verdict(foundA, dA, L, gA, chA, (nr & gb) != 0, chB);
        }
      } else {
        const int pidx = pr * W + pc, gidx = gj.x * W + gj.y, sidx = sin ? sr * W + sc : -1;
        uint64_t fA[WPL], fB[WPL], RA[WPL], RB[WPL], m0[WPL], ml[WPL], gb[WPL];
        bool gfree = false;
#pragma unroll
        for (int t = 0; t < WPL; ++t) {
          const int w = lane + 64 * t;
          const bool in = w < nw;
          const uint64_t pb = (pidx >> 6) == w ? 1ull << (pidx & 63) : 0ull;
          const uint64_t sb = (sidx >> 6) == w && sidx >= 0 ? 1ull << (sidx & 63) : 0ull;
          gb[t] = (gidx >> 6) == w ? 1ull << (gidx & 63) : 0ull;
          fA[t] = (in ? fre[w] : 0ull) | pb;
          fB[t] = fA[t] & ~sb;
          RA[t] = RB[t] = pb;
          m0[t] = in ? nc0[w] : 0ull;
          ml[t] = in ? ncl[w] : 0ull;
          gfree |= (fA[t] & gb[t]) != 0;
        }
        if (!__ballot(gfree)) continue;  // the goal cell is an obstacle: no path after
        bool foundA = false;
        int dA = 0;
        for (int L = 1; !verdict; ++L) {
          bool chA = false, chB = false, gA = false, gB = false;
#pragma unroll
          for (int t = 0; t < WPL; ++t) {
            const int w = lane + 64 * t;
            if (w < nw) {
              curA[w] = RA[t];
              curB[w] = RB[t];
            }
          }
          wave_fence();
#pragma unroll
          for (int t = 0; t < WPL; ++t) {
            const int w = lane + 64 * t;
            if (w < nw) {
              if (!foundA) {
                const uint64_t nr = RA[t] | (bw_nbr(curA, w, nw, q, r, m0[t], ml[t]) & fA[t]);
                chA |= nr != RA[t];
                RA[t] = nr;
                gA |= (nr & gb[t]) != 0;
              }
              const uint64_t nr = RB[t] | (bw_nbr(curB, w, nw, q, r, m0[t], ml[t]) & fB[t]);
              chB |= nr != RB[t];
              RB[t] = nr;
              gB |= (nr & gb[t]) != 0;
            }
          }
          wave_fence();
          verdict = bw_verdict(foundA, dA, L, gA, chA, gB, chB);
        }
      }
      n += verdict == 2 ? 1 : 0;
    }
  }
  if (lane == 0) {
    if (run && a.reward) a.reward[oi] = GOAL_REWARD + n * BLOCKING_COST;  // (:581-583)
    if (a.blocking) a.blocking[oi] = n > 0 ? 1 : 0;
    if (a.counts) a.counts[oi] = n;
  }
}

int launch_blocking(mapfx_primal_t* h, const BArgs& a, void* stream) {
  const QGeo& g = h->geo;
  if ((long long)g.E * a.K > 0x7FFFFFFFll) return perr(MAPFX_EINVAL, "n_envs * K too large");
  // lane-per-row masks wherever the grid fits 64 x 64, unless a test pins the flat-set
  // kernel (MAPFX_PRIMAL_BLOCKING=flat at mapfx_primal_create)
  const bool rows = g.H <= 64 && g.W <= 64 && !h->blocking_flat;
  const int lds = (rows ? 64 * 8 : (g.hw + 63) / 64 * 8 * 5) + g.N * 16;  // + positions, goals
  const PrimalBFn fn = rows ? primal_blocking_kernel<true> : primal_blocking_kernel<false>;
  return launch_kernel(fn, dim3((unsigned)(g.E * a.K)), dim3(64), lds, (hipStream_t)stream, nullptr, nullptr,
                       "primal_blocking_kernel launch", NOTED, g, a);
}

// ---------------------------------------------------------------------------
// primal_observe_kernel<S, DIAG>: _observe (:343-386), _listNextValidActions (:639-667),
// on_goal (:633) and State.done (:159-166) of the worlds as they stand; nothing of the
// state is written.  Queries do not depend on each other: one wave per (world, query),
// a.nw waves per workgroup, a.chunks workgroups per world.
//
// A workgroup stages its world once -- the obstacle bitmap as it lies in memory (H * W
// bits, at most 2 KB: no padded byte map, the queries touch only Q * s * s cells) and the
// agents' {row, col, goal row, goal col} (DIAG: past) records -- and each wave builds its
// query's [4][s][s] record in its own LDS slab:
//   cells over lanes: obstacle plane from the bitmap (outside the grid = 1, :356-359),
//     own goal plane, the other two planes cleared;
//   agents over lanes: an agent inside the window stamps poss_map, and (unless it is the
//     queried agent) its goal, clamped into the window, into goals_map (:369-378); the
//     same pass finds the neighbours that refuse a move (a robot on the target, DIAG: a
//     crossing of (past, present), :77-99) and counts the agents on their goals;
//   the record is 4 s^2 bytes at offset (e Q + q) 4 s^2, a whole number of dwords for
//     every s: it leaves the slab as s^2 coalesced dword stores, odd s included.
// A bad query (id outside 1..N, prev_action outside 0..nact-1) reports 1 + world in err
// (first report wins, as in primal_act_kernel) and writes nothing; its wave ends, the
// other queries of the world are other waves.
// ---------------------------------------------------------------------------
struct OArgs {
  const int32_t* pos;
  const int32_t* goal;
  const uint8_t* bits;
  const int32_t* past;
  const int32_t* ids;    // NULL: query q is agent q + 1
  const int32_t* prev;   // NULL: previous action 0
  int Q, chunks, nw;     // queries per world, workgroups per world, waves per workgroup
  int wmax, w_ag, w_past;  // packed kernel: worlds a wave can span, offsets inside a staged world
  int off_ag, off_past, off_rec, rec_bytes;  // LDS regions; a wave's slab is rec_bytes
  uint8_t* obs;
  double* vec;
  uint8_t* next_mask;
  uint8_t* on_goal;
  uint8_t* done;
  int32_t* err;
  const double* pow_lut;
};

template <int S_, bool DIAG>
__global__ void __launch_bounds__(1024) primal_observe_kernel(QGeo g, OArgs a) {
  extern __shared__ __align__(16) unsigned char lds[];
  constexpr int NDIR = DIAG ? 8 : 4;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, nthr = a.nw * 64;
  const int e = (int)(blockIdx.x / (unsigned)a.chunks), ch = (int)(blockIdx.x - (unsigned)e * (unsigned)a.chunks);
  const int N = g.N, H = g.H, W = g.W;
  const int s = S_ ? S_ : g.s, ss = s * s, h2 = s / 2;
  const uint32_t* bm = (const uint32_t*)lds;             // the world's obstacle bitmap
  const int4* agL = (const int4*)(lds + a.off_ag);       // [N] {row, col, goal row, goal col}
  const int2* pastL = (const int2*)(lds + a.off_past);   // [N] agents_past (DIAG)
  uint8_t* rec = lds + a.off_rec + wv * a.rec_bytes;     // this wave's [4][s][s] record

  // ---- the world, once per workgroup ----
  {
    const uint32_t* src = (const uint32_t*)(a.bits + (g.map_shared ? 0 : (long long)e * g.map_stride));
    for (int w = tid; w < g.bits_words; w += nthr) ((uint32_t*)lds)[w] = src[w];
    for (int b = tid; b < N; b += nthr) {
      const long long i = (long long)e * N + b;
      const int2 p = ((const int2*)a.pos)[i], q = ((const int2*)a.goal)[i];
      ((int4*)(lds + a.off_ag))[b] = make_int4(p.x, p.y, q.x, q.y);
      if constexpr (DIAG) ((int2*)(lds + a.off_past))[b] = ((const int2*)a.past)[i];
    }
  }
  __syncthreads();

  const int q = ch * a.nw + wv;
  if (q >= a.Q) return;  // (no workgroup barrier below)
  const long long oi = (long long)e * a.Q + q;
  const int aid = (a.ids ? a.ids[oi] : q + 1) - 1, prev = a.prev ? a.prev[oi] : 0;
  if ((unsigned)aid >= (unsigned)N || (unsigned)prev >= (unsigned)g.nact) {  // the reference asserts / KeyErrors
    if (lane == 0 && a.err) atomicCAS(a.err, 0, e + 1);
    return;
  }
  const int4 A = agL[aid];
  const int tr = A.x - h2, tc = A.y - h2;  // top_left (:345-346)

  // ---- cells over lanes: obstacle and own-goal planes, poss_map / goals_map cleared ----
  if (a.obs) {
    for (int i = lane; i < ss; i += 64) {
      const int y = S_ ? i / s : fastdiv(i, g.m_s), x = i - y * s;
      const int r = tr + y, c = tc + x;
      const bool in = r >= 0 && r < H && c >= 0 && c < W;
      const int idx = in ? r * W + c : 0;
      const bool wall = !in || ((bm[idx >> 5] >> (idx & 31)) & 1u);
      rec[i] = 0;
      rec[ss + i] = (r == A.z && c == A.w) ? 1 : 0;  // (:366-368; the goal is inside the grid)
      rec[2 * ss + i] = 0;
      rec[3 * ss + i] = wall ? 1 : 0;                // (:356-362)
    }
  }
  // ---- _listNextValidActions (:639-667): lane d probes action d for bounds and wall ----
  bool ok = false;
  if (lane >= 1 && lane <= NDIR) {
    const int nx = A.x + dir_r(lane), ny = A.y + dir_c(lane);
    const bool in = nx >= 0 && nx < H && ny >= 0 && ny < W;
    const int idx = in ? nx * W + ny : 0;
    ok = in && !((bm[idx >> 5] >> (idx & 31)) & 1u);
  }
  uint32_t mask = 1u | ((uint32_t)__ballot(ok) & (NDIR == 8 ? 0x1FEu : 0x1Eu));
  wave_fence();
  // ---- agents over lanes ----
  uint32_t refuse = 0;  // directions with a robot on the target or (DIAG) a diagonal crossing
  int ngoal = 0;
  for (int b0 = 0; b0 < N; b0 += 64) {
    const int b = b0 + lane;
    bool og = false;
    if (b < N) {
      const int4 B = agL[b];
      og = B.x == B.z && B.y == B.w;
      const int wy = B.x - tr, wx = B.y - tc;
      if (a.obs && wy >= 0 && wy < s && wx >= 0 && wx < s) {
        rec[wy * s + wx] = 1;  // poss_map: the agent itself and the others (:363-372)
        if (b != aid) {        // a visible agent's goal, clamped into view (:374-378)
          const int mr = max(tr, min(tr + s - 1, B.z)), mc = max(tc, min(tc + s - 1, B.w));
          rec[2 * ss + (mr - tr) * s + (mc - tc)] = 1;
        }
      }
      if (b != aid) {
        const int rx = B.x - A.x, ry = B.y - A.y;  // a robot on a neighbouring cell
        if (rx >= -1 && rx <= 1 && ry >= -1 && ry <= 1)
          refuse |= 1u << (uint32_t)((ACT_OF >> (4 * ((rx + 1) * 3 + ry + 1))) & 0xFu);
        if constexpr (DIAG) {  // equal midpoints of (past, present) and (position, target)
          const int2 pp = pastL[b];
          const int sx = pp.x + B.x - 2 * A.x, sy = pp.y + B.y - 2 * A.y;
          if (sx >= -1 && sx <= 1 && sy >= -1 && sy <= 1)
            refuse |= 1u << (uint32_t)((ACT_OF >> (4 * ((sx + 1) * 3 + sy + 1))) & 0xFu);
        }
      }
    }
    ngoal += __popcll(__ballot(og));
  }
#pragma unroll
  for (int d = 1; d <= NDIR; ++d)
    if (__ballot((refuse >> d) & 1u)) mask &= ~(1u << d);
  const int opp = opposite(prev);
  if (opp > 0) mask &= ~(1u << opp);
  wave_fence();
  // ---- the record: s^2 dwords, coalesced ----
  if (a.obs) {
    uint32_t* o32 = (uint32_t*)(a.obs + oi * 4 * ss);
    const uint32_t* r32 = (const uint32_t*)rec;
    for (int m = lane; m < ss; m += 64) o32[m] = r32[m];
  }
  if (lane == 0) {
    if (a.done) a.done[oi] = ngoal == N ? 1 : 0;                        // world.done() (:159-166)
    if (a.on_goal) a.on_goal[oi] = (A.x == A.z && A.y == A.w) ? 1 : 0;  // (:633)
    if (a.next_mask) {
      if constexpr (DIAG) ((uint16_t*)a.next_mask)[oi] = (uint16_t)mask;
      else a.next_mask[oi] = (uint8_t)mask;
    }
    if (a.vec) {  // :380-386, magnitude from the host libm pow LUT
      const int dX = A.z - A.x, dY = A.w - A.y;
      const double mag = a.pow_lut[dX * dX + dY * dY];
      double vx = (double)dX, vy = (double)dY;
      if (mag != 0.0) {
        vx = vx / mag;
        vy = vy / mag;
      }
      double* v = a.vec + oi * 3;
      v[0] = vx;
      v[1] = vy;
      v[2] = mag;
    }
  }
}

// ---------------------------------------------------------------------------
// primal_observe_packed_kernel<DIAG>: the same answers with one LANE per query, the
// second half of primal_seq_kernel's idea (its phase B) without a move chain in front.
//
// A wave-per-query costs a few hundred wave instructions per query whatever the lanes
// do, and 65,536 queries of the bench shape then are VALU-issue bound far above what
// the record bytes cost.  Here wave w answers the 64 consecutive queries 64 w .. 64 w +
// 63 of the flat [E][Q] order: it stages the (at most a.wmax) worlds those queries belong
// to -- bitmap and agent records, as above -- and every lane builds its query's four
// planes as ONE 4 s^2-bit string (plane p at bits p s^2; the obstacle rows are s-bit
// extracts of the bitmap, agents and clamped goals single bits).  The 64 strings are
// packed back to back in LDS, so bit i of the packed string is byte i of the wave's
// contiguous run of records: the wave expands 32 bits to two 16-byte stores per lane.
// Strings of neighbouring lanes share a dword when 4 s^2 is no multiple of 32, so bits are
// set with LDS atomic ORs.  A wave with a bad query expands dword by dword and leaves the
// bad query's bytes alone.
// ---------------------------------------------------------------------------
__device__ inline uint32_t lowmask(int n) { return n >= 32 ? ~0u : (1u << n) - 1u; }
__device__ inline uint32_t nibble_bytes(uint32_t v) { return ((v & 15u) * 0x00204081u) & 0x01010101u; }

template <bool DIAG>
__global__ void __launch_bounds__(64) primal_observe_packed_kernel(QGeo g, OArgs a) {
  extern __shared__ __align__(16) unsigned char lds[];
  constexpr int NDIR = DIAG ? 8 : 4;
  const int lane = threadIdx.x;
  const int N = g.N, H = g.H, W = g.W, s = g.s, ss = s * s, h2 = s / 2, Q = a.Q;
  const long long total = (long long)g.E * Q, f0 = (long long)blockIdx.x * 64, f = f0 + lane;
  const int nq = (int)min(64ll, total - f0);             // queries of this wave
  const int e_lo = (int)(f0 / Q), e_hi = (int)((f0 + nq - 1) / Q);  // its worlds (at most a.wmax)
  uint32_t* str = (uint32_t*)lds;                          // [8 s^2 + 1] the packed strings
  unsigned char* wbase = lds + a.off_ag;                   // staged worlds, a.rec_bytes each:
  const int o_ag = a.w_ag, o_past = a.w_past;            // ... bitmap, agent records, past

  for (int i = lane; i < 8 * ss + 1; i += 64) str[i] = 0u;
  // staging, flat over (world, item) with the loads of four rounds in flight together
  // (a loop over the worlds would pay one global round trip per world)
  {
    const int per = g.bits_words + N, T = (e_hi - e_lo + 1) * per;
    for (int i0 = 0; i0 < T; i0 += 256) {
      uint32_t bw[4];
      int2 P[4], G[4], PP[4];
      int wo[4], item[4];  // the item's world (LDS byte offset) and index; item < 0: none
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const int idx = i0 + lane + 64 * t;
        item[t] = -1, wo[t] = 0;
        if (idx < T) {
          const int wl = (int)((unsigned)idx / (unsigned)per), it = idx - wl * per;
          const long long ew = e_lo + wl;
          item[t] = it, wo[t] = wl * a.rec_bytes;
          if (it < g.bits_words) {
            bw[t] = ((const uint32_t*)(a.bits + (g.map_shared ? 0 : ew * g.map_stride)))[it];
          } else {
            const long long i = ew * N + (it - g.bits_words);
            P[t] = ((const int2*)a.pos)[i];
            G[t] = ((const int2*)a.goal)[i];
            if constexpr (DIAG) PP[t] = ((const int2*)a.past)[i];
          }
        }
      }
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        if (item[t] < 0) continue;
        if (item[t] < g.bits_words) {
          *(uint32_t*)(wbase + wo[t] + 4 * item[t]) = bw[t];
        } else {
          const int b = item[t] - g.bits_words;
          *(int4*)(wbase + wo[t] + a.w_ag + 16 * b) = make_int4(P[t].x, P[t].y, G[t].x, G[t].y);
          if constexpr (DIAG) *(int2*)(wbase + wo[t] + a.w_past + 8 * b) = PP[t];
        }
      }
    }
  }
  const bool live = lane < nq;
  int aid = 0, prev = 0, e = e_lo;
  if (live) {
    e = (int)(f / Q);
    aid = (a.ids ? a.ids[f] : (int)(f - (long long)e * Q) + 1) - 1;
    prev = a.prev ? a.prev[f] : 0;
  }
  const bool okq = live && (unsigned)aid < (unsigned)N && (unsigned)prev < (unsigned)g.nact;
  if (live && !okq && a.err) atomicCAS(a.err, 0, e + 1);  // the reference asserts / KeyErrors
  const uint64_t okm = __ballot(okq);
  wave_fence();
  if (okq) {
    const unsigned char* wr = wbase + (e - e_lo) * a.rec_bytes;
    const uint32_t* bm = (const uint32_t*)wr;
    const int4* agL = (const int4*)(wr + o_ag);
    const int2* pastL = (const int2*)(wr + o_past);
    const int4 A = agL[aid];
    const int tr = A.x - h2, tc = A.y - h2;  // top_left (:345-346)
    const uint32_t sb = (uint32_t)lane * 4u * (uint32_t)ss;  // first bit of this lane's string
    if (a.obs) {
      // obstacle plane (:356-362): row y is the bitmap's bits of columns c0 .. c0 + n - 1
      // at window columns sh .. sh + n - 1, ones outside the grid
      const int c0 = max(tc, 0), n = min(tc + s, W) - c0, sh = c0 - tc;  // (n >= 1: the agent's column)
      const uint32_t full = lowmask(s), inside = lowmask(n) << sh;
      for (int y = 0; y < s; ++y) {
        const int r = tr + y;
        uint32_t row = full;
        if (r >= 0 && r < H) {
          const int i0 = r * W + c0, w0 = i0 >> 5;
          const uint64_t two = (uint64_t)bm[w0] | ((uint64_t)bm[min(w0 + 1, g.bits_words - 1)] << 32);
          row = (full & ~inside) | (((uint32_t)(two >> (i0 & 31)) << sh) & inside);
        }
        const uint32_t B = sb + 3u * ss + (uint32_t)(y * s), o = B & 31u;
        atomicOr(&str[B >> 5], row << o);
        if (o + (uint32_t)s > 32u) atomicOr(&str[(B >> 5) + 1], row >> (32u - o));
      }
      const int gy = A.z - tr, gx = A.w - tc;  // own goal (:366-368)
      if (gy >= 0 && gy < s && gx >= 0 && gx < s) {
        const uint32_t B = sb + ss + (uint32_t)(gy * s + gx);
        atomicOr(&str[B >> 5], 1u << (B & 31u));
      }
    }
    // _listNextValidActions (:639-667): bounds and walls, then robots and crossings
    uint32_t mask = 1u, refuse = 0u;
#pragma unroll
    for (int d = 1; d <= NDIR; ++d) {
      const int nx = A.x + dir_r(d), ny = A.y + dir_c(d);
      const bool in = nx >= 0 && nx < H && ny >= 0 && ny < W;
      const int idx = in ? nx * W + ny : 0;
      if (in && !((bm[idx >> 5] >> (idx & 31)) & 1u)) mask |= 1u << d;
    }
    int ngoal = 0;
    for (int b = 0; b < N; ++b) {
      const int4 B4 = agL[b];
      ngoal += (B4.x == B4.z && B4.y == B4.w) ? 1 : 0;
      const int wy = B4.x - tr, wx = B4.y - tc;
      if (a.obs && wy >= 0 && wy < s && wx >= 0 && wx < s) {
        const uint32_t B = sb + (uint32_t)(wy * s + wx);  // poss_map (:363-372)
        atomicOr(&str[B >> 5], 1u << (B & 31u));
        if (b != aid) {  // a visible agent's goal, clamped into view (:374-378)
          const int mr = max(tr, min(tr + s - 1, B4.z)), mc = max(tc, min(tc + s - 1, B4.w));
          const uint32_t G = sb + 2u * ss + (uint32_t)((mr - tr) * s + (mc - tc));
          atomicOr(&str[G >> 5], 1u << (G & 31u));
        }
      }
      if (b != aid) {
        const int rx = B4.x - A.x, ry = B4.y - A.y;  // a robot on a neighbouring cell
        if (rx >= -1 && rx <= 1 && ry >= -1 && ry <= 1)
          refuse |= 1u << (uint32_t)((ACT_OF >> (4 * ((rx + 1) * 3 + ry + 1))) & 0xFu);
        if constexpr (DIAG) {  // equal midpoints of (past, present) and (position, target)
          const int2 pp = pastL[b];
          const int sx = pp.x + B4.x - 2 * A.x, sy = pp.y + B4.y - 2 * A.y;
          if (sx >= -1 && sx <= 1 && sy >= -1 && sy <= 1)
            refuse |= 1u << (uint32_t)((ACT_OF >> (4 * ((sx + 1) * 3 + sy + 1))) & 0xFu);
        }
      }
    }
    mask &= ~(refuse & 0x1FEu);
    const int opp = opposite(prev);
    if (opp > 0) mask &= ~(1u << opp);
    if (a.done) a.done[f] = ngoal == N ? 1 : 0;                        // world.done() (:159-166)
    if (a.on_goal) a.on_goal[f] = (A.x == A.z && A.y == A.w) ? 1 : 0;  // (:633)
    if (a.next_mask) {
      if constexpr (DIAG) ((uint16_t*)a.next_mask)[f] = (uint16_t)mask;
      else a.next_mask[f] = (uint8_t)mask;
    }
    if (a.vec) {  // :380-386, magnitude from the host libm pow LUT
      const int dX = A.z - A.x, dY = A.w - A.y;
      const double mag = a.pow_lut[dX * dX + dY * dY];
      double vx = (double)dX, vy = (double)dY;
      if (mag != 0.0) {
        vx = vx / mag;
        vy = vy / mag;
      }
      double* v = a.vec + f * 3;
      v[0] = vx;
      v[1] = vy;
      v[2] = mag;
    }
  }
  if (!a.obs) return;
  wave_fence();
  // ---- the wave's records: nq * s^2 dwords, dword d = bits 4 d .. 4 d + 3 ----
  const int nd = nq * ss;
  int d0 = 0;  // dwords below d0 leave as 16-byte stores
  if (okm == (nq == 64 ? ~0ull : (1ull << nq) - 1ull)) {
    const int nch = nd >> 2;
    uint4* obase = (uint4*)(a.obs + f0 * 4 * ss);  // (16-byte aligned: the host checks a.obs)
    for (int i = lane; 2 * i < nch; i += 64) {
      const uint32_t b = str[i];
      uint4 v0, v1;
      v0.x = nibble_bytes(b), v0.y = nibble_bytes(b >> 4), v0.z = nibble_bytes(b >> 8), v0.w = nibble_bytes(b >> 12);
      v1.x = nibble_bytes(b >> 16), v1.y = nibble_bytes(b >> 20), v1.z = nibble_bytes(b >> 24), v1.w = nibble_bytes(b >> 28);
      obase[2 * i] = v0;
      if (2 * i + 1 < nch) obase[2 * i + 1] = v1;
    }
    d0 = nch << 2;
  }
  uint32_t* o32 = (uint32_t*)(a.obs + f0 * 4 * ss);
  for (int d = d0 + lane; d < nd; d += 64) {
    const int owner = fastdiv(d, g.m_ss);
    if ((okm >> owner) & 1ull) o32[d] = nibble_bytes(str[d >> 3] >> (4 * (d & 7)));
  }
}

using PrimalOFn = void (*)(QGeo, OArgs);
PrimalOFn pick_observe(const QGeo& g) {
  if (g.s == 10) return g.diag ? primal_observe_kernel<10, true> : primal_observe_kernel<10, false>;
  return g.diag ? primal_observe_kernel<0, true> : primal_observe_kernel<0, false>;
}

// ---------------------------------------------------------------------------
// primal_generate_kernel: MAPFEnv._setWorld (:248-341) for every (masked-in) world of the
// batch -- a random square world, agents on random free cells, every agent's goal on a
// random cell of the connected region it stands in -- by the rules of mapfx_primal.h.
//
// One 64-lane wave per world, GEN_WAVES worlds per workgroup; the waves never meet (no
// workgroup barrier: a wave leaves as soon as its world is masked out or bad).  Lane r
// holds row r as a 64-bit mask, as primal_blocking_kernel<true> does:
//   obstacles: lane r draws its own row, one counter-based draw per cell;
//   the k-th cell of a set: a wave prefix sum of the rows' popcounts names the row, and
//     lane c of the wave tests "bit c is set and has k' set bits below it" of that row;
//     the sets only shrink by the cell just picked, so the prefix sum is scanned once
//     per run of picks (the starts; the goals of one region) and then kept by decrement;
//   regions: the flood m |= row_nbr(m) & free runs until a ballot says nothing grew, ONCE
//     per region: a flood started at the lowest agent without a goal is the region of
//     every agent standing in it (regions are disjoint, so those agents, served in
//     ascending id, see exactly the goals the plain per-agent order would have placed);
//   lane l keeps agents l, l + 64, .. (N <= 255) in registers; positions and goals leave
//     as coalesced int2 stores, the bitmap as whole dwords built from the rows in LDS.
// Everything is integer arithmetic; a bad world writes nothing but *err.
// ---------------------------------------------------------------------------
struct GArgs {
  uint64_t seed;
  long long env_offset;
  const int32_t* side_lut;
  const uint32_t* prob_lut;
  int n_side, n_prob;
  int32_t* episode;
  const uint8_t* mask;
  uint8_t* bits;
  int keep_map;
  int32_t* err;
  int32_t* pos;
  int32_t* goal;
  int32_t* past;
};

constexpr int GEN_WAVES = 4;
// mapfx/rng.py: K_ENV, K_T, K_CELL, K_STREAM and the generator's stream ids
constexpr uint64_t GK_ENV = 0xD1B54A32D192ED03ull, GK_T = 0xABC98388FB8FAC03ull,
                   GK_CELL = 0x9E6C63D0676A9A99ull, GK_STREAM = 0xF1357AEA2E62A9C5ull;
constexpr uint32_t GS_WORLD = 0x100u, GS_OBST = 0x200u, GS_START = 0x300u, GS_GOAL = 0x400u;

__device__ inline uint64_t gen_key(uint64_t base, uint32_t stream, uint32_t idx) {
  return splitmix64(base ^ ((uint64_t)idx * GK_CELL) ^ ((uint64_t)stream * GK_STREAM));
}
__device__ inline uint32_t gen_draw32(uint64_t base, uint32_t stream, uint32_t idx) {
  return (uint32_t)(gen_key(base, stream, idx) >> 32);
}

// inclusive prefix sum over the wave
__device__ inline int wave_scan(int v, int lane) {
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int u = __shfl_up(v, d);
    if (lane >= d) v += u;
  }
  return v;
}
__device__ inline uint64_t readlane_u64(uint64_t v, int l) {
  return ((uint64_t)readlane_u32((uint32_t)(v >> 32), l) << 32) | readlane_u32((uint32_t)v, l);
}

// Cell number pick(draw, |x|) of the set x (lane = row, row-major order): its (row, col),
// the same in every lane.  inc is the inclusive prefix sum over the lanes of the rows'
// popcounts, kept by the caller: taking one cell out of row r is `inc -= lane >= r`, so
// a run of picks from a shrinking set costs one wave_scan, not one per pick.  x must
// not be empty.
__device__ inline void gen_pick_cell(uint64_t x, int inc, uint32_t draw, int lane, int& row, int& col) {
  const int exc = inc - __popcll(x);
  const uint32_t total = (uint32_t)__builtin_amdgcn_readlane(inc, 63);
  const uint32_t k = (uint32_t)(((uint64_t)draw * total) >> 32);
  const uint64_t hit = __ballot((uint32_t)exc <= k && k < (uint32_t)inc);
  row = __builtin_amdgcn_readfirstlane((int)__ffsll((unsigned long long)hit) - 1) & 63;
  const uint32_t kk = k - (uint32_t)__builtin_amdgcn_readlane(exc, row);
  const uint64_t bits = readlane_u64(x, row);
  const bool me = ((bits >> lane) & 1ull) != 0 && (uint32_t)__popcll(bits & ((1ull << lane) - 1ull)) == kk;
  col = __builtin_amdgcn_readfirstlane((int)__ffsll((unsigned long long)__ballot(me)) - 1) & 63;
}

__global__ void __launch_bounds__(64 * GEN_WAVES) primal_generate_kernel(QGeo g, GArgs a) {
  __shared__ uint64_t rowsL[GEN_WAVES][64];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int e = blockIdx.x * GEN_WAVES + wv;
  if (e >= g.E) return;               // (wave-uniform, like every exit below)
  if (a.mask && !a.mask[e]) return;   // masked out: nothing of the world is read or written
  const int N = g.N, H = g.H, W = g.W;
  const int ep = a.episode[e];
  const uint64_t base = a.seed ^ ((uint64_t)(a.env_offset + e) * GK_ENV) ^ ((uint64_t)(uint32_t)ep * GK_T);
  const long long moff = g.map_shared ? 0 : (long long)e * g.map_stride;
  uint64_t fre = 0;  // the free cells of row `lane`
  bool bad;
  if (!a.keep_map) {
    // ---- world draw (:313-314 by table) and obstacles (:315), redrawn at half the
    //      density while fewer than N cells are free: attempt 32 is the empty world ----
    const uint64_t k = gen_key(base, GS_WORLD, 0);
    const int side = a.side_lut[(uint32_t)k & (uint32_t)(a.n_side - 1)];
    const uint32_t thresh = a.prob_lut[(uint32_t)(k >> 32) & (uint32_t)(a.n_prob - 1)];
    bad = side < 1 || side > min(H, W) || side * side < N;
    if (!bad) {
      const uint64_t sm = side >= 64 ? ~0ull : (1ull << side) - 1ull;
      for (uint32_t t = 0; t <= 32u; ++t) {
        const uint32_t th = (uint32_t)((uint64_t)thresh >> t);
        uint64_t ob = 0;
        if (th != 0u && lane < side)
          for (int c = 0; c < side; ++c)
            ob |= (uint64_t)(gen_draw32(base, GS_OBST + t, (uint32_t)(lane * 64 + c)) < th ? 1u : 0u) << c;
        fre = lane < side ? ~ob & sm : 0ull;
        const int nfree = __builtin_amdgcn_readlane(wave_scan(__popcll(fre), lane), 63);
        if (nfree >= N) break;
      }
    }
  } else {
    // ---- blank_world (:281-305): the world's bitmap as it stands ----
    if (lane < H) {
      const uint32_t* src = (const uint32_t*)(a.bits + moff);
      const int b0 = lane * W, wi = b0 >> 5, sh = b0 & 31, last = (b0 + W - 1) >> 5;
      const uint64_t d0 = src[wi], d1 = wi + 1 <= last ? src[wi + 1] : 0u, d2 = wi + 2 <= last ? src[wi + 2] : 0u;
      uint64_t v = (d0 | (d1 << 32)) >> sh;
      if (sh) v |= d2 << (64 - sh);
      fre = ~v & (W >= 64 ? ~0ull : (1ull << W) - 1ull);
    }
    bad = __builtin_amdgcn_readlane(wave_scan(__popcll(fre), lane), 63) < N;
  }
  if (bad) {
    if (lane == 0 && a.err) atomicCAS(a.err, 0, e + 1);
    return;
  }
  // ---- starts (:320-325): agent a on a uniform cell of the free cells still empty ----
  int srow[4], scol[4], grow[4], gcol[4];
  {
    uint64_t avail = fre;
    int inc = wave_scan(__popcll(avail), lane);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      srow[j] = scol[j] = grow[j] = gcol[j] = 0;
      for (int i = 0; i < 64 && 64 * j + i < N; ++i) {
        int r, c;
        gen_pick_cell(avail, inc, gen_draw32(base, GS_START, (uint32_t)(64 * j + i)), lane, r, c);
        if (lane == r) avail &= ~(1ull << c);
        inc -= lane >= r ? 1 : 0;
        if (lane == i) srow[j] = r, scol[j] = c;
      }
    }
  }
  // ---- goals (:327-336): one flood per region, its agents served in ascending id ----
  {
    uint64_t gtaken = 0;                  // row `lane` of the cells that hold a goal
    uint64_t served[4] = {0ull, 0ull, 0ull, 0ull};  // agents 64 j + bit with a goal (uniform)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (64 * j >= N) break;
      const int nj = min(64, N - 64 * j);
      const uint64_t all = nj >= 64 ? ~0ull : (1ull << nj) - 1ull;
      while (all & ~served[j]) {
        const int i0 = __builtin_amdgcn_readfirstlane((int)__ffsll((unsigned long long)(all & ~served[j])) - 1);
        const int r0 = __builtin_amdgcn_readlane(srow[j], i0), c0 = __builtin_amdgcn_readlane(scol[j], i0);
        uint64_t m = lane == r0 ? 1ull << c0 : 0ull;
        for (;;) {
          const uint64_t nm = m | (row_nbr(m, lane) & fre);
          const bool grew = nm != m;
          m = nm;
          if (!__ballot(grew)) break;
        }
        int inc = wave_scan(__popcll(m & ~gtaken), lane);  // the region's cells still without a goal
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) {
          if (jj < j || 64 * jj >= N) continue;
          // agent 64 jj + lane stands in the region (an earlier agent cannot: its own
          // flood would have served the agent this flood started from)
          const uint64_t mr = __shfl(m, srow[jj]);
          const bool in = 64 * jj + lane < N && ((mr >> scol[jj]) & 1ull) != 0;
          uint64_t todo = __ballot(in) & ~served[jj];
          served[jj] |= todo;
          while (todo) {
            const int i = __builtin_amdgcn_readfirstlane((int)__ffsll((unsigned long long)todo) - 1);
            todo &= todo - 1ull;
            int r, c;
            gen_pick_cell(m & ~gtaken, inc, gen_draw32(base, GS_GOAL, (uint32_t)(64 * jj + i)), lane, r, c);
            if (lane == r) gtaken |= 1ull << c;
            inc -= lane >= r ? 1 : 0;
            if (lane == i) grow[jj] = r, gcol[jj] = c;
          }
        }
      }
    }
  }
  // ---- writes: pos, goal, past = pos (:55-66), the bitmap, the episode counter ----
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int b = 64 * j + lane;
    if (b < N) {
      const long long i = (long long)e * N + b;
      ((int2*)a.pos)[i] = make_int2(srow[j], scol[j]);
      ((int2*)a.goal)[i] = make_int2(grow[j], gcol[j]);
      if (a.past) ((int2*)a.past)[i] = make_int2(srow[j], scol[j]);
    }
  }
  if (!a.keep_map) {
    // obstacle rows -> LDS; dword w of the bitmap is bits 32 w .. 32 w + 31 of the row-major
    // H * W bit string (rows of a W that does not divide 32 straddle dwords), 0 past its end
    rowsL[wv][lane] = lane < H ? ~fre & (W >= 64 ? ~0ull : (1ull << W) - 1ull) : 0ull;
    wave_fence();
    uint32_t* dst = (uint32_t*)(a.bits + moff);
    const int nd = (int)(g.map_stride >> 2);
    for (int w = lane; w < nd; w += 64) {
      uint32_t v = 0;
      const int b0 = 32 * w;
      if (b0 < g.hw) {
        int r = b0 / W, c = b0 - r * W, p = 0;
        while (p < 32 && r < H) {
          const int take = min(W - c, 32 - p);
          const uint32_t piece = (uint32_t)(rowsL[wv][r] >> c) & (take >= 32 ? ~0u : (1u << take) - 1u);
          v |= piece << p;
          p += take;
          ++r;
          c = 0;
        }
      }
      dst[w] = v;
    }
  }
  if (lane == 0) a.episode[e] = ep + 1;
}

// the checks every entry point that reads the worlds starts with
int check_state(const mapfx_primal_t* h, const mapfx_primal_state* st) {
  if (!h) return perr(MAPFX_EINVAL, "NULL handle");
  if (!st || !st->pos || !st->goal || !st->map_bits) return perr(MAPFX_EINVAL, "bad state");
  return MAPFX_OK;
}

// a zeroed QArgs / OArgs / BArgs with the worlds' pos / goal / bits
template <typename A>
void fill_state(A& a, const mapfx_primal_state* st) {
  memset(&a, 0, sizeof(a));
  a.pos = st->pos;
  a.goal = st->goal;
  a.bits = st->map_bits;
}

}  // namespace

extern "C" {

int mapfx_primal_create(const mapfx_primal_cfg* cfg, mapfx_primal_t** out) {
  if (!cfg || !out) return perr(MAPFX_EINVAL, "NULL argument");
  *out = nullptr;
  const mapfx_primal_cfg& c = *cfg;
  if (c.H < 1 || c.W < 1 || (long long)c.H * c.W > 16384)
    return perr(MAPFX_EINVAL, "PRIMAL path supports H * W <= 16384");
  if (c.n_agents < 1 || c.n_agents > 255) return perr(MAPFX_EINVAL, "n_agents must be in 1..255");
  if (c.n_envs < 0) return perr(MAPFX_EINVAL, "n_envs < 0");
  if (c.obs_size < 1 || c.obs_size > 32) return perr(MAPFX_EINVAL, "obs_size must be in 1..32");
  std::unique_ptr<mapfx_primal_t, void (*)(mapfx_primal_t*)> h(new (std::nothrow) mapfx_primal_t(),
                                                               mapfx_primal_destroy);
  if (!h) return perr(MAPFX_ENOMEM, "host allocation failed");
  QGeo& g = h->geo;
  memset(&g, 0, sizeof(g));
  g.H = c.H;
  g.W = c.W;
  g.N = c.n_agents;
  g.E = c.n_envs;
  g.s = c.obs_size;
  g.map_shared = c.map_shared ? 1 : 0;
  g.map_stride = mapfx_map_stride(c.H, c.W);
  g.hw = c.H * c.W;
  g.bits_words = (g.hw + 31) / 32;
  g.lut_n = (c.H - 1) * (c.H - 1) + (c.W - 1) * (c.W - 1) + 1;
  g.diag = c.diagonal ? 1 : 0;
  g.nact = g.diag ? 9 : 5;
  g.P = std::max(1, g.s / 2);
  g.PW = (c.W + 2 * g.P + 3) & ~3;
  g.rows = c.H + 2 * g.P;
  g.m_s = magic48(g.s);
  g.m_ss = magic48(g.s * g.s);
  // One world per wave, phase A / phase B (primal_seq_kernel) wherever it applies, unless
  // a test pins the lane-group kernel (MAPFX_PRIMAL_LANES, or MAPFX_PRIMAL_PATH=groups).
  {
    const char* lanes = getenv("MAPFX_PRIMAL_LANES");
    const char* path = getenv("MAPFX_PRIMAL_PATH");
    const bool pinned = (lanes && *lanes) || (path && strcmp(path, "groups") == 0);
    g.lds_seq = pinned ? 0 : layout_seq(g);
    g.seq = g.lds_seq > 0 ? 1 : 0;
  }
  const int wreg = layout(g);
  // Lanes per world: the smallest of 16 / 32 / 64 that writes an even-s call's planes
  // in at most 4 rounds (s * s / 4 dwords per plane) and holds the agents in at most
  // 4 registers each, widened while the grid has fewer than 2 waves per SIMD (2048
  // waves: more waves hide the call's LDS round trips) or a wave's worlds would pass
  // 64 KB of LDS.  At 4096 worlds, s = 10 (the bench) this is 32 lanes, 2 worlds a
  // wave.  MAPFX_PRIMAL_LANES (16 / 32 / 64) overrides the wave-count rule (tests).
  const int D = (g.s % 2 == 0) ? g.s * g.s / 4 : 1;
  int ls = 4;
  while (ls < 6 && (D > 4 * (1 << ls) || g.N > 4 * (1 << ls))) ++ls;
  const char* force = getenv("MAPFX_PRIMAL_LANES");
  const int fl = force ? atoi(force) : 0;
  if (fl == 16 || fl == 32 || fl == 64) ls = std::max(ls, fl == 16 ? 4 : fl == 32 ? 5 : 6);
  else
    while (ls < 6 && (long long)(g.E + (64 >> ls) - 1) / (64 >> ls) < 2048) ++ls;
  while (ls < 6 && (64 >> ls) * wreg > 65536) ++ls;
  if ((64 >> ls) * wreg > 160 * 1024) return perr(MAPFX_EINVAL, "PRIMAL world needs too much LDS");
  g.lw_shift = ls;
  g.lw = 1 << ls;
  g.apl = (g.N + g.lw - 1) / g.lw;
  g.wreg = wreg;
  h->lds = (64 >> ls) * wreg;
  {
    const char* bp = getenv("MAPFX_PRIMAL_BLOCKING");
    h->blocking_flat = bp && strcmp(bp, "flat") == 0;
    const char* op = getenv("MAPFX_PRIMAL_OBSERVE");
    h->observe_pin = op && strcmp(op, "waves") == 0 ? 1 : op && strcmp(op, "lanes") == 0 ? 2 : 0;
  }
  if (h->lds > 64 * 1024) {
    const hipError_t e = hipFuncSetAttribute((const void*)pick_primal(g),
                                             hipFuncAttributeMaxDynamicSharedMemorySize, h->lds);
    if (e != hipSuccess) return check_hip(e, "hipFuncSetAttribute");
  }
  double* lut = (double*)malloc(sizeof(double) * g.lut_n);
  if (!lut) return perr(MAPFX_ENOMEM, "host allocation failed");
  double (*volatile libm_pow)(double, double) = pow;  // `n ** .5` in Python = libm pow
  for (int i = 0; i < g.lut_n; ++i) lut[i] = libm_pow((double)i, 0.5);
  int rc = check_hip(hipMalloc(&h->pow_lut, sizeof(double) * g.lut_n), "hipMalloc");
  if (!rc) rc = check_hip(hipMemcpy(h->pow_lut, lut, sizeof(double) * g.lut_n, hipMemcpyHostToDevice), "hipMemcpy");
  free(lut);
  if (rc) return rc;
  *out = h.release();
  return MAPFX_OK;
}

void mapfx_primal_destroy(mapfx_primal_t* h) {
  if (!h) return;
  if (h->pow_lut) (void)hipFree(h->pow_lut);
  delete h;
}

int mapfx_primal_act_timed(mapfx_primal_t* h, const mapfx_primal_state* st, const int32_t* agent_ids,
                           const int32_t* actions, int32_t K, const mapfx_primal_out* out,
                           void* start_event, void* stop_event, void* stream) {
  if (const int rc = check_state(h, st)) return rc;
  if (h->geo.diag && !st->past) return perr(MAPFX_EINVAL, "diagonal movement needs state.past");
  if (K < 0) return perr(MAPFX_EINVAL, "K < 0");
  // (both kernels write the observation records as dwords)
  if (out && ((uintptr_t)out->obs & 3u)) return perr(MAPFX_EINVAL, "out->obs must be 4-byte aligned");
  if (K == 0 || h->geo.E == 0) return MAPFX_OK;
  if (!agent_ids || !actions) return perr(MAPFX_EINVAL, "NULL agent_ids / actions");
  QArgs a;
  fill_state(a, st);
  a.past = st->past;
  a.ids = agent_ids;
  a.acts = actions;
  a.K = K;
  a.pow_lut = h->pow_lut;
  if (out) {
    a.reward = out->reward;
    a.done = out->done;
    a.next_mask = out->next_mask;
    a.on_goal = out->on_goal;
    a.valid = out->valid;
    a.obs = out->obs;
    a.vec = out->vec;
    a.err = out->err;
  }
  const QGeo& g = h->geo;
  if (g.seq && ((uintptr_t)a.obs & 15u) == 0)  // (16-byte record runs)
    return launch_kernel(pick_seq(g), dim3(g.E), dim3(64), g.lds_seq, (hipStream_t)stream, (hipEvent_t)start_event,
                         (hipEvent_t)stop_event, "primal_seq_kernel launch", NOTED, g, a);
  const int wpw = 64 >> g.lw_shift;
  return launch_kernel(pick_primal(g), dim3((g.E + wpw - 1) / wpw), dim3(64), h->lds, (hipStream_t)stream,
                       (hipEvent_t)start_event, (hipEvent_t)stop_event, "primal_act_kernel launch", NOTED, g, a);
}

int mapfx_primal_act(mapfx_primal_t* h, const mapfx_primal_state* st, const int32_t* agent_ids,
                     const int32_t* actions, int32_t K, const mapfx_primal_out* out, void* stream) {
  return mapfx_primal_act_timed(h, st, agent_ids, actions, K, out, nullptr, nullptr, stream);
}

int mapfx_primal_observe(mapfx_primal_t* h, const mapfx_primal_state* st, const int32_t* agent_ids,
                         const int32_t* prev_actions, int32_t Q, const mapfx_primal_out* out, void* stream) {
  if (const int rc = check_state(h, st)) return rc;
  const QGeo& g = h->geo;
  if (g.diag && !st->past) return perr(MAPFX_EINVAL, "diagonal movement needs state.past");
  if (Q < 0) return perr(MAPFX_EINVAL, "Q < 0");
  if (!agent_ids && Q != g.N) return perr(MAPFX_EINVAL, "agent_ids NULL asks for every agent: Q must equal n_agents");
  if (out && ((uintptr_t)out->obs & 3u)) return perr(MAPFX_EINVAL, "out->obs must be 4-byte aligned");
  if (Q == 0 || g.E == 0) return MAPFX_OK;
  OArgs a;
  fill_state(a, st);
  a.past = st->past;
  a.ids = agent_ids;
  a.prev = prev_actions;
  a.Q = Q;
  a.pow_lut = h->pow_lut;
  if (out) {
    a.obs = out->obs;
    a.vec = out->vec;
    a.next_mask = out->next_mask;
    a.on_goal = out->on_goal;
    a.done = out->done;
    a.err = out->err;
  }
  // One lane per query (primal_observe_packed_kernel) where a world's staging is shared
  // by enough of its queries -- at most 12 staged items (bitmap words + agents) per query;
  // measured at the bench shape: 3 items per query (Q = 16) it is 2 x faster than a wave
  // per query, 48 (Q = 1, a wave stages 64 worlds) 2 x slower -- and the worlds 64
  // consecutive queries can belong to fit a wave's LDS next to the packed strings and
  // the records leave as 16-byte stores; else one wave per query.  MAPFX_PRIMAL_OBSERVE
  // = waves / lanes pins either (tests; lanes still needs the LDS to fit).
  {
    const int strs = round_up((8 * g.s * g.s + 1) * 4, 16);
    a.w_ag = round_up(g.bits_words * 4, 16);
    a.w_past = a.w_ag + 16 * g.N;
    const int per_world = a.w_past + (g.diag ? round_up(8 * g.N, 16) : 0);
    const long long total = (long long)g.E * Q;
    const int wmax = (int)std::min<long long>(g.E, 63 / Q + 2);
    const long long lds = strs + (long long)wmax * per_world;
    const bool shared_enough = g.bits_words + g.N <= 12 * Q;
    if (h->observe_pin != 1 && (shared_enough || h->observe_pin == 2) && lds <= 64 * 1024 &&
        ((uintptr_t)a.obs & 15u) == 0) {
      if ((total + 63) / 64 > 0x7FFFFFFFll) return perr(MAPFX_EINVAL, "n_envs * Q too large");
      a.wmax = wmax;
      a.off_ag = strs;
      a.rec_bytes = per_world;
      const PrimalOFn fn = g.diag ? primal_observe_packed_kernel<true> : primal_observe_packed_kernel<false>;
      return launch_kernel(fn, dim3((unsigned)((total + 63) / 64)), dim3(64), (int)lds, (hipStream_t)stream, nullptr,
                           nullptr, "primal_observe_packed_kernel launch", NOTED, g, a);
    }
  }
  // LDS of a workgroup: bitmap (<= 2 KB), agent records (<= 4 KB, DIAG + 2 KB), one
  // 4 s^2-byte slab per wave (<= 4 KB): with up to 16 waves at most 72 KB, so the waves
  // are capped to stay inside the 64 KB every kernel gets without an attribute.
  a.off_ag = round_up(g.bits_words * 4, 16);
  a.off_past = a.off_ag + 16 * g.N;
  a.off_rec = a.off_past + (g.diag ? round_up(8 * g.N, 16) : 0);
  a.rec_bytes = round_up(4 * g.s * g.s, 16);
  const int maxw = std::min(16, (64 * 1024 - a.off_rec) / a.rec_bytes);
  a.chunks = (Q + maxw - 1) / maxw;
  a.nw = (Q + a.chunks - 1) / a.chunks;  // the world's queries spread evenly over its workgroups
  if ((long long)g.E * a.chunks > 0x7FFFFFFFll) return perr(MAPFX_EINVAL, "n_envs * Q too large");
  const int lds = a.off_rec + a.nw * a.rec_bytes;
  const PrimalOFn fn = pick_observe(g);
  return launch_kernel(fn, dim3((unsigned)(g.E * a.chunks)), dim3(64 * a.nw), lds, (hipStream_t)stream, nullptr,
                       nullptr, "primal_observe_kernel launch", NOTED, g, a);
}

int mapfx_primal_blocking_count(mapfx_primal_t* h, const mapfx_primal_state* st, const int32_t* agent_ids,
                                int32_t* counts, void* stream) {
  if (const int rc = check_state(h, st)) return rc;
  if (!agent_ids || !counts) return perr(MAPFX_EINVAL, "NULL agent_ids / counts");
  if (h->geo.E == 0) return MAPFX_OK;
  BArgs a;
  fill_state(a, st);
  a.ids = agent_ids;
  a.K = 1;
  a.counts = counts;
  return launch_blocking(h, a, stream);
}

int mapfx_primal_blocking(mapfx_primal_t* h, const mapfx_primal_state* st, const int32_t* agent_ids,
                          const int32_t* actions, int32_t K, const uint8_t* valid, const uint8_t* on_goal,
                          double* reward, uint8_t* blocking, int32_t* counts, void* stream) {
  if (const int rc = check_state(h, st)) return rc;
  if (K < 0) return perr(MAPFX_EINVAL, "K < 0");
  if (!valid || !on_goal) return perr(MAPFX_EINVAL, "the blocking pass needs the launch's valid and on_goal");
  if (K == 0 || h->geo.E == 0) return MAPFX_OK;
  if (!agent_ids || !actions) return perr(MAPFX_EINVAL, "NULL agent_ids / actions");
  BArgs a;
  fill_state(a, st);
  a.ids = agent_ids;
  a.acts = actions;
  a.K = K;
  a.valid = valid;
  a.on_goal = on_goal;
  a.reward = reward;
  a.blocking = blocking;
  a.counts = counts;
  a.undo = 1;
  return launch_blocking(h, a, stream);
}

int mapfx_primal_generate(mapfx_primal_t* h, const mapfx_primal_state* st, const mapfx_primal_gen* gen,
                          void* stream) {
  if (!h) return perr(MAPFX_EINVAL, "NULL handle");
  if (!st || !st->pos || !st->goal) return perr(MAPFX_EINVAL, "bad state: the generator writes pos and goal");
  if (!gen || !gen->episode || !gen->map_bits) return perr(MAPFX_EINVAL, "NULL gen, gen->episode or gen->map_bits");
  const QGeo& g = h->geo;
  if (g.map_shared && !gen->keep_map)
    return perr(MAPFX_EINVAL, "a map_shared handle generates with keep_map only (one map cannot hold E worlds)");
  if (g.diag && !st->past) return perr(MAPFX_EINVAL, "diagonal movement needs state.past");
  if (g.H > 64 || g.W > 64) return perr(MAPFX_EINVAL, "the generator supports H <= 64 and W <= 64");
  if (!gen->keep_map) {
    if (!gen->side_lut || !gen->prob_lut) return perr(MAPFX_EINVAL, "NULL side_lut / prob_lut without keep_map");
    const auto pow2 = [](int n) { return n >= 1 && (n & (n - 1)) == 0; };
    if (!pow2(gen->n_side) || !pow2(gen->n_prob))
      return perr(MAPFX_EINVAL, "n_side and n_prob must be powers of two");
  }
  if (g.E == 0) return MAPFX_OK;
  GArgs a;
  memset(&a, 0, sizeof(a));
  a.seed = gen->seed;
  a.env_offset = gen->env_offset;
  a.side_lut = gen->side_lut;
  a.prob_lut = gen->prob_lut;
  a.n_side = gen->n_side;
  a.n_prob = gen->n_prob;
  a.episode = gen->episode;
  a.mask = gen->mask;
  a.bits = gen->map_bits;
  a.keep_map = gen->keep_map ? 1 : 0;
  a.err = gen->err;
  a.pos = st->pos;
  a.goal = const_cast<int32_t*>(st->goal);
  a.past = g.diag ? st->past : nullptr;
  return launch_kernel(primal_generate_kernel, dim3((unsigned)((g.E + GEN_WAVES - 1) / GEN_WAVES)),
                       dim3(64 * GEN_WAVES), 0, (hipStream_t)stream, nullptr, nullptr,
                       "primal_generate_kernel launch", NOTED, g, a);
}

}  // extern "C"
