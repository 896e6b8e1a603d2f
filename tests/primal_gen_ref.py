"""Plain Python / numpy restatement of the device PRIMAL world generator
(mapfx_primal_generate, include/mapfx_primal.h; PrimalBatch.random / regenerate) -- TEST
INFRASTRUCTURE ONLY.  It restates the rules of the header from scratch: its own
splitmix64, its own constants, its own breadth-first search; nothing is imported from the
package.

    key(gid, ep, stream, idx) = splitmix64(seed ^ gid*K_ENV ^ ep*K_T ^ idx*K_CELL ^ stream*K_STREAM)
    draw32 = key >> 32;  pick(d, n) = (d * n) >> 32;  cells in row-major order
"""
from collections import deque

import numpy as np

M64 = (1 << 64) - 1
K_ENV, K_T = 0xD1B54A32D192ED03, 0xABC98388FB8FAC03
K_CELL, K_STREAM = 0x9E6C63D0676A9A99, 0xF1357AEA2E62A9C5
WORLD, OBST, START, GOAL = 0x100, 0x200, 0x300, 0x400


def mix(x):
    x = (x + 0x9E3779B97F4A7C15) & M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M64
    return x ^ (x >> 31)


def base_key(seed, gid, ep):
    return (seed & M64) ^ ((gid * K_ENV) & M64) ^ (((ep & 0xFFFFFFFF) * K_T) & M64)


def key(base, stream, idx):
    return mix(base ^ ((idx * K_CELL) & M64) ^ ((stream * K_STREAM) & M64))


def draw32(base, stream, idx):
    return key(base, stream, idx) >> 32


def pick(d, n):
    return (d * n) >> 32


def _draw32_cells(base, stream, idx):
    """draw32 for an integer array of cell indices (the same arithmetic on uint64 arrays)."""
    u = np.uint64
    with np.errstate(over="ignore"):
        x = u(base) ^ (idx.astype(np.uint64) * u(K_CELL)) ^ u((stream * K_STREAM) & M64)
        x = x + u(0x9E3779B97F4A7C15)
        x = (x ^ (x >> u(30))) * u(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> u(27))) * u(0x94D049BB133111EB)
        x = x ^ (x >> u(31))
    return x >> u(32)


def region(free, r0, c0):
    """Free cells 4-connected to (r0, c0), as a boolean array (breadth-first)."""
    H, W = free.shape
    seen = np.zeros((H, W), dtype=bool)
    seen[r0, c0] = True
    q = deque([(r0, c0)])
    while q:
        r, c = q.popleft()
        for dr, dc in ((1, 0), (-1, 0), (0, 1), (0, -1)):
            rr, cc = r + dr, c + dc
            if 0 <= rr < H and 0 <= cc < W and free[rr, cc] and not seen[rr, cc]:
                seen[rr, cc] = True
                q.append((rr, cc))
    return seen


def _nth(cells_mask, n):
    """(row, col) of cell number n of a boolean array, row-major."""
    W = cells_mask.shape[1]
    i = int(np.flatnonzero(cells_mask.reshape(-1))[n])
    return i // W, i % W


def world(seed, gid, ep, N, H, W, side_lut=None, prob_lut=None, obstacles=None):
    """One world.  obstacles None: steps 1-5 of the header; else keep_map on the given
    boolean [H, W] obstacle array.  Returns None for a bad world, else a dict with
    obst (bool [H, W]), pos, goal (int32 [N, 2]), side, attempts."""
    base = base_key(seed, gid, ep)
    side, t = None, 0
    if obstacles is None:
        k = key(base, WORLD, 0)
        side = int(side_lut[k & (len(side_lut) - 1)])
        thresh = int(prob_lut[(k >> 32) & (len(prob_lut) - 1)])
        if side < 1 or side > min(H, W) or side * side < N:
            return None
        rr, cc = np.meshgrid(np.arange(side), np.arange(side), indexing="ij")
        while True:
            ob = _draw32_cells(base, OBST + t, rr * 64 + cc) < np.uint64(thresh >> t)
            if side * side - int(ob.sum()) >= N:
                break
            t += 1
        obst = np.ones((H, W), dtype=bool)
        obst[:side, :side] = ob
    else:
        obst = np.asarray(obstacles, dtype=bool)
        if int((~obst).sum()) < N:
            return None
    free = ~obst
    avail = free.copy()
    pos = np.zeros((N, 2), dtype=np.int32)
    for a in range(N):
        r, c = _nth(avail, pick(draw32(base, START, a), int(avail.sum())))
        avail[r, c] = False
        pos[a] = (r, c)
    goal = np.zeros((N, 2), dtype=np.int32)
    taken = np.zeros((H, W), dtype=bool)
    for a in range(N):
        R = region(free, int(pos[a, 0]), int(pos[a, 1])) & ~taken
        r, c = _nth(R, pick(draw32(base, GOAL, a), int(R.sum())))
        taken[r, c] = True
        goal[a] = (r, c)
    return {"obst": obst, "pos": pos, "goal": goal, "side": side, "attempts": t}


def stride(H, W):
    return ((H * W + 7) // 8 + 15) // 16 * 16


def pack(obst):
    """bool [H, W] -> uint8 [stride]: cell r * W + c is bit (r * W + c) % 8 of byte (r * W + c) // 8."""
    H, W = obst.shape
    out = np.zeros(stride(H, W), dtype=np.uint8)
    p = np.packbits(obst.reshape(-1), bitorder="little")
    out[:len(p)] = p
    return out


def unpack(bits, H, W):
    return np.unpackbits(np.asarray(bits, dtype=np.uint8), count=H * W, bitorder="little").reshape(H, W).astype(bool)


def generate(state, seed, env_offset, N, H, W, luts=None, mask=None, keep_map=False):
    """mapfx_primal_generate on host arrays, in place.  state: dict of numpy arrays bits
    [E or 1, stride], pos, goal [E, N, 2], past ([E, N, 2] or None), episode [E].
    Returns the list of bad worlds (the device reports 1 + one of them in *err)."""
    E = state["pos"].shape[0]
    bad = []
    for e in range(E):
        if mask is not None and not mask[e]:
            continue
        ep = int(state["episode"][e])
        if keep_map:
            b = state["bits"][e if state["bits"].shape[0] == E else 0]
            w = world(seed, env_offset + e, ep, N, H, W, obstacles=unpack(b, H, W))
        else:
            w = world(seed, env_offset + e, ep, N, H, W, luts[0], luts[1])
        if w is None:
            bad.append(e)
            continue
        state["pos"][e] = w["pos"]
        state["goal"][e] = w["goal"]
        if state.get("past") is not None:
            state["past"][e] = w["pos"]
        if not keep_map:
            state["bits"][e] = pack(w["obst"])
        state["episode"][e] = ep + 1
    return bad
