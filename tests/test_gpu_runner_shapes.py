"""The batched ParallelRunner (mapfx/runners.py, csrc/runner.hip, the RUN half of
csrc/partial.hip) over the matrix of kernel instances its step can reach, each against
tests/runner_ref.py -- the restatement of the reference runner loop that
tests/test_runner_ref.py pins to the reference's own output -- byte for byte.

Every case: one map, per-env random starts / goals (a seeded numpy rng, new ones for the
second run), 2 runs (the second meets a recycled env state), a MAC that reads a seeded
action table [T, B, N] on the device through the `bs` it is given and replaces an action
by 4 (stay) where batch["avail_actions"][bs, t_ep] forbids it (so the avail rows of
t_ep must be in place before the call).  The batch handed to the runner is filled with
the byte 0xA5 instead of zeros and the restatement starts from the same fill: a store
into any element the reference loop never writes (rows of an env after its termination,
rows past the last step, the padding of the padded case) fails the comparison.

Early terminations are built in: every agent of an early env b has its goal one free
move from its start; env b's table says stay before step t_b, that move at t_b.  The
starts and goals are the two ends of N disjoint dominoes of free cells (all 2N cells
distinct); where the map has fewer than N such dominoes (N = 64 on 10 x 10, N = 300 on
24 x 24: 2N exceeds the cells) the goals are the starts shifted one column right, and the
agents move as one block.  test_matrix_reference_has_early_terminations checks on the
restatement alone (no GPU) that every case has >= 3 distinct termination steps before
the limit, an env that runs to the limit and an env that ends at step 0.

Cases with a large B (the compaction's long chunks) tile P archetype envs: env b has
the instance and the action table of archetype b % P, so (envs never interact) its
rows, return and length are those of env b % P of the restatement run on the P
archetypes, and the MAC's bs is every b whose b % P is in the restatement's bs.

Which kernel a case reaches is asserted from mapfx_last_kernel after the run; the LDS
geometry behind the staging classes (csrc/partial.hip layout()'s sums) is derived in
CASES' comments.
"""
import re
import types

import numpy as np
import pytest

import runner_ref

REWARDS = dict(move_reward=0, stay_reward=-0.1, stay_goal_reward=1, node_collide_reward=-2000,
               edge_collide_reward=-2000, env_collide_reward=-2000, complete_reward=1000,
               complete_fac=1.5, gamma=0.99)
FILL = 0xA5
RUNS = 2
MOVES = {(-1, 0): 0, (1, 0): 1, (0, -1): 2, (0, 1): 3}


def _open(h, w, obstacles=()):
    rows = [["."] * w for _ in range(h)]
    for r, c in obstacles:
        rows[r][c] = "@"
    return ["".join(r) for r in rows]


def _block200():
    """200 x 200, all obstacle but a 20 x 20 block (with three obstacles inside)."""
    rows = [["@"] * 200 for _ in range(200)]
    for r in range(90, 110):
        for c in range(95, 115):
            rows[r][c] = "."
    for r, c in ((93, 100), (99, 108), (104, 97)):
        rows[r][c] = "@"
    return ["".join(r) for r in rows]


_OBS12 = ((2, 3), (5, 8), (9, 4), (7, 7))
_OBS10 = ((3, 3), (6, 7))

# name: grid, N, window, K, B, limit (T = limit + 1 <= 6), kernel = (name, template args)
# pick() must return; `tile`: B tiles that many archetype envs.
#
# LDS per env (mapfx_partial_create): 2 map images of rows * pitch bytes (rows = H + 2P,
# pitch = round4(round4(P) + W + P), P = max(1, win / 2)) + the bitmap + L * 48 (features)
# + 2 * L * 8, each rounded to 16; EPW = 64 / L envs per wave while EPW * per_env <= 64 KB;
# the stage image of one env is L * D * 4 + 16 bytes and min(EPW, G / L) of them alias the
# second map image onwards: G = 64 lanes if the wave's total stays <= 40 KB, else G = 32 if
# <= 64 KB, else no stage; waves per block: 4 while wpb * lds <= 160 KB.
#   12 x 12, L = 8: per_env 1184, EPW 8, stage 8 * 3696 -> 32128 <= 40 KB: G = 64, wpb 4
#   32 x 32, L = 16: per_env 4048, EPW 4, stage 4 * 7376 -> 35264 <= 40 KB: G = 64, wpb 4
#   64 x 64, L = 16: per_env 11344, EPW 4: 45376 > 40 KB already, with G = 32 two images
#     (14752) fit under the 45376 the maps take: G = 32 (half-wave staging), wpb 3
#   200 x 200: one map image is 204 * 208 = 42432 bytes, per_env ~ 90 KB > 64 KB: EPW 1,
#     no stage (off_stage < 0), 2 * lds > 160 KB: wpb 1; H * W > 32767: int32 tables
CASES = {
    # fast L = 8, u8 tables; N * D * 4 mod 16 = 12, 8, 4, 0 (D = 115): with ts every
    # destination misalignment; B = 21 = 2 full waves of 8 envs + 5
    "fast8_n5": dict(grid=_open(12, 12, _OBS12), N=5, win=5, K=5, B=21, limit=5,
                     kernel=("partial_kernel", "5,5,8,1,true")),
    "fast8_n6": dict(grid=_open(12, 12, _OBS12), N=6, win=5, K=5, B=21, limit=5,
                     kernel=("partial_kernel", "5,5,8,1,true")),
    "fast8_n7": dict(grid=_open(12, 12, _OBS12), N=7, win=5, K=5, B=21, limit=5,
                     kernel=("partial_kernel", "5,5,8,1,true")),
    "fast8_n8": dict(grid=_open(12, 12, _OBS12), N=8, win=5, K=5, B=21, limit=5,
                     kernel=("partial_kernel", "5,5,8,1,true")),
    # the bench's instance (32 x 32, N = 16, int16 tables, per-env instances); 4 envs per
    # wave, 4 waves per block: B = 70 = 4 blocks + 1 wave + 2 envs
    "fast16_n16": dict(grid=_open(32, 32, ((4, 9), (17, 20), (25, 3), (11, 30))), N=16, win=5, K=5,
                       B=70, limit=5, kernel=("partial_kernel", "5,5,16,2,true")),
    "fast16_n9": dict(grid=_open(32, 32, ((4, 9), (17, 20), (25, 3), (11, 30))), N=9, win=5, K=5,
                      B=70, limit=5, kernel=("partial_kernel", "5,5,16,2,true")),
    # the other two fast windows (16 x 16 = 256 cells: int16)
    "fast16_w3": dict(grid=_open(16, 16, ((3, 4), (10, 9))), N=12, win=3, K=5, B=10, limit=5,
                      kernel=("partial_kernel", "3,5,16,2,true")),
    "fast16_w7": dict(grid=_open(16, 16, ((3, 4), (10, 9))), N=12, win=7, K=5, B=10, limit=5,
                      kernel=("partial_kernel", "7,5,16,2,true")),
    # L = 32: 2 envs per wave
    "fast32_n17": dict(grid=_open(20, 20, ((5, 5), (12, 14))), N=17, win=5, K=5, B=7, limit=5,
                       kernel=("partial_kernel", "5,5,32,2,true")),
    "fast32_n32": dict(grid=_open(20, 20, ((5, 5), (12, 14))), N=32, win=5, K=5, B=7, limit=5,
                       kernel=("partial_kernel", "5,5,32,2,true")),
    # half-wave staging (stage_lanes = 32, derived above); 3 waves, the last with 2 envs
    "half64_n16": dict(grid=_open(64, 64, ((9, 9), (30, 41), (50, 17))), N=16, win=5, K=5, B=10,
                       limit=5, kernel=("partial_kernel", "5,5,16,2,true")),
    # unstaged fast path, int32 tables, one env per wave, one wave per block
    "block200_n9": dict(grid=_block200(), N=9, win=5, K=5, B=5, limit=5,
                        kernel=("partial_kernel", "5,5,16,0,true")),
    # the generic fused kernel: L = 4 (16 envs per wave), L = 64, K != 5, windows 9 / 0 / 1
    "gen_n3": dict(grid=_open(10, 10, _OBS10), N=3, win=5, K=5, B=21, limit=5,
                   kernel=("partial_kernel", "5,0,0,0,true")),
    "gen_n40": dict(grid=_open(10, 10, _OBS10), N=40, win=5, K=5, B=5, limit=5,
                    kernel=("partial_kernel", "5,0,0,0,true")),
    "gen_n64": dict(grid=_open(10, 10, _OBS10), N=64, win=5, K=5, B=5, limit=5,
                    kernel=("partial_kernel", "5,0,0,0,true")),
    "gen_w9_k3": dict(grid=_open(10, 10, _OBS10), N=12, win=9, K=3, B=6, limit=5,
                      kernel=("partial_kernel", "9,0,0,0,true")),
    "gen_w0": dict(grid=_open(10, 10, _OBS10), N=6, win=0, K=5, B=9, limit=5,
                   kernel=("partial_kernel", "0,0,0,0,true")),
    "gen_w1": dict(grid=_open(10, 10, _OBS10), N=6, win=1, K=5, B=9, limit=5,
                   kernel=("partial_kernel", "1,0,0,0,true")),
    # the workgroup path (N > 64 or a side > 256; mapfx_partial_fuses_post = 0): act_row /
    # obs_rows in partial_wg_kernel<WIN, agents per thread>, then runner_post_kernel and
    # runner_compact_kernel
    "wg_n70": dict(grid=_open(20, 20, ((5, 5), (12, 14))), N=70, win=5, K=5, B=5, limit=5,
                   kernel=("partial_wg_kernel", "5,1")),
    "wg_n300": dict(grid=_open(24, 24), N=300, win=5, K=5, B=5, limit=4,
                    kernel=("partial_wg_kernel", "5,2")),
    "wg_tall260": dict(grid=_open(260, 6, ((100, 2), (200, 4))), N=4, win=5, K=5, B=5, limit=5,
                       kernel=("partial_wg_kernel", "5,1")),
    # runner_compact_block's chunks above 32 flags (not held as a bit set): the fused
    # compaction workgroup has 64 * wpb threads and wpb = 1 on the 200 x 200 map (above),
    # so ceil(B / 64) > 32 from B = 32 * 64 + 1 = 2049
    "cmp_fused_2049": dict(grid=_block200(), N=1, win=5, K=5, B=2049, limit=5, tile=41,
                           kernel=("partial_kernel", "5,0,0,0,true")),
    # runner_compact_kernel (the unfused form, 1024 threads): chunks of 2 and of 34 envs
    "cmp_unfused_1025": dict(grid=_open(4, 4, ((2, 1),)), N=1, win=3, K=2, B=1025, limit=5, tile=41,
                             unfused=True, kernel=("partial_kernel", "3,0,0,0,true")),
    "cmp_unfused_33795": dict(grid=_open(4, 4, ((2, 1),)), N=1, win=3, K=2, B=33 * 1024 + 3, limit=5,
                              tile=41, unfused=True, kernel=("partial_kernel", "3,0,0,0,true")),
}


# ------------------------------------------------------------------ instances
def _dominoes(grid, vertical):
    """Disjoint pairs of adjacent free cells, scanning rows (columns if vertical)."""
    h, w = grid.shape
    used = np.zeros((h, w), bool)
    out = []
    dr, dc = (1, 0) if vertical else (0, 1)
    order = [(r, c) for c in range(w) for r in range(h)] if vertical else \
        [(r, c) for r in range(h) for c in range(w)]
    for r, c in order:
        rr, cc = r + dr, c + dc
        if rr < h and cc < w and grid[r, c] == 0 and grid[rr, cc] == 0 and not used[r, c] \
                and not used[rr, cc]:
            used[r, c] = used[rr, cc] = True
            out.append(((r, c), (rr, cc)))
    return out


def _instances(case, seed):
    """(starts, goals) [P, N, 2] (row, col) and the action table [T, P, N] of one run;
    P = the case's tile or B.  Early envs: 0 (t_b = 2), 1 (0), P - 1 (1), P // 2 (3)."""
    rng = np.random.RandomState(seed)
    grid = runner_ref.parse_map(case["grid"])
    N, P, T = case["N"], case.get("tile", case["B"]), case["limit"] + 1
    free = np.argwhere(grid == 0)
    starts = np.zeros((P, N, 2), np.int32)
    goals = np.zeros((P, N, 2), np.int32)
    table = rng.randint(0, 5, size=(T, P, N))
    early = {0: 2, 1: 0, P - 1: 1, P // 2: 3}
    for b in range(P):
        if b not in early:
            starts[b] = free[rng.choice(len(free), N, replace=False)]
            goals[b] = free[rng.choice(len(free), N, replace=False)]
            continue
        dom = _dominoes(grid, vertical=bool(b & 1))
        if len(dom) >= N:
            for n, i in enumerate(rng.choice(len(dom), N, replace=False)):
                a, z = dom[i] if rng.randint(2) else dom[i][::-1]
                starts[b, n], goals[b, n] = a, z
        else:   # fewer than N dominoes: one block, shifted one column right
            ok = np.array([(r, c) for r, c in free if c + 1 < grid.shape[1] and grid[r, c + 1] == 0])
            starts[b] = ok[rng.choice(len(ok), N, replace=False)]
            goals[b] = starts[b] + np.array([0, 1], np.int32)
        table[:, b, :] = 4
        for n in range(N):
            table[early[b], b, n] = MOVES[tuple((goals[b, n] - starts[b, n]).tolist())]
    return starts, goals, table


_REF = {}


def reference(name):
    """The restatement's result for a case, computed once per session and never modified:
    per run the instances, the action table, the final batch, the MAC calls, returns and
    lengths (of the P archetypes when the case tiles); and the log / t_env of the full B."""
    if name in _REF:
        return _REF[name]
    case = CASES[name]
    N, W, K, limit, B = case["N"], case["win"], case["K"], case["limit"], case["B"]
    P = case.get("tile", B)
    grid = runner_ref.parse_map(case["grid"])
    ref = runner_ref.RefRunner(runner_log_interval=1)
    full = ref if P == B else runner_ref.RefRunner(runner_log_interval=1)
    src = np.arange(B) % P
    runs = []
    for r in range(RUNS):
        starts, goals, table = _instances(case, 1000 * r + 17 + N + W)
        envs = runner_ref.make_envs(grid, starts, goals, obs_window=W, obs_knn_agents=K,
                                    episode_limit=limit, **REWARDS)

        def mac(batch, t_ep, bs, table=table):
            a = table[t_ep][bs]
            ok = np.take_along_axis(batch["avail_actions"][bs, t_ep], a[..., None], 2)[..., 0] != 0
            return np.where(ok, a, 4)

        batch = runner_ref.new_batch(P, limit + 1, N, 2 * W * W + 13 * K, fill=FILL)
        batch, calls, returns, lengths = ref.run(envs, batch, mac)
        if full is not ref:
            full.finish([returns[s] for s in src], [lengths[s] for s in src],
                        int(sum(lengths[s] for s in src)), [{"_step_count": lengths[s]} for s in src])
        runs.append(dict(starts=starts, goals=goals, table=table, batch=batch, calls=calls,
                         returns=np.array(returns, np.float64), lengths=np.array(lengths, np.int64),
                         t_env=full.t_env))
    _REF[name] = dict(runs=runs, log=list(full.log), src=src)
    return _REF[name]


@pytest.mark.parametrize("name", list(CASES))
def test_matrix_reference_has_early_terminations(name):
    _assert_terminations(name)


def _assert_terminations(name):
    """Before anything runs on the GPU: each run of each case has, by the restatement,
    >= 3 distinct termination steps before the limit, an env that runs to the limit and
    an env that ends at step 0 (length 1)."""
    case = CASES[name]
    unwritten = int(np.full(8, FILL, np.uint8).view(np.int64)[0])
    for run in reference(name)["runs"]:
        lengths = run["lengths"]
        term = run["batch"]["terminated"][..., 0]
        assert len(set(lengths[lengths < case["limit"]].tolist())) >= 3, lengths
        assert (lengths == case["limit"]).any() and (lengths == 1).any(), lengths
        for b, n in enumerate(lengths):                  # the rows say the same
            assert term[b, n - 1] == 1 and run["batch"]["filled"][b, :, 0].tolist() == \
                [1] * (n + 1) + [unwritten] * (case["limit"] - n)
        # the stale list: the MAC call after an env's last step still has it in bs
        assert len(run["calls"]) == lengths.max() + 1
        for b, n in enumerate(lengths):
            assert [b in bs for _, bs in run["calls"]] == [t <= n for t in range(len(run["calls"]))]


# ------------------------------------------------------------------ GPU side
class Logger:
    def __init__(self):
        self.stats = []

    def log_stat(self, k, v, t):
        self.stats.append((k, float(v), int(t)))


class TableMAC:
    """Reads the run's action table through `bs` on the device (no host reads), applies
    the avail rule, records every (t_ep, bs) and -- from the first call past the
    reference's last one -- a copy of the batch."""

    action_selector = types.SimpleNamespace()

    def __init__(self, dtype, src):
        self.dtype, self.src = dtype, src
        self.calls, self.table, self.n_ref, self.snap = [], None, 0, None

    def start_run(self, table, n_ref, device):
        import torch
        self.table = torch.as_tensor(table[:, self.src.cpu().numpy()], device=device)
        self.calls, self.n_ref, self.snap = [], n_ref, None

    def init_hidden(self, batch_size):
        pass

    def select_actions(self, batch, t_ep, t_env, bs, test_mode=False):
        import torch
        if len(self.calls) == self.n_ref:
            self.snap = {k: v.clone() for k, v in batch.data.transition_data.items()}
        self.calls.append((t_ep, bs.clone()))
        a = self.table[t_ep][bs]
        ok = torch.gather(batch["avail_actions"][bs, t_ep], 2, a[..., None]).squeeze(-1) != 0
        return torch.where(ok, a, torch.full_like(a, 4)).to(self.dtype)


def _batch_classes():
    import torch
    from mapfx.episode import DeviceEpisodeBatch

    class SentinelBatch(DeviceEpisodeBatch):
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            for t in self.data.transition_data.values():
                t.view(torch.uint8).fill_(FILL)

    class PaddedBatch(DeviceEpisodeBatch):
        """Every tensor a view of wider storage: the time stride is the row + 1 element
        for obs, + 3 for the other fields."""

        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            self.storage = {}
            td = self.data.transition_data
            for key, t in list(td.items()):
                inner = int(np.prod(t.shape[2:]))
                wide = torch.empty(t.shape[:2] + (inner + (1 if key == "obs" else 3),),
                                   dtype=t.dtype, device=t.device)
                wide.view(torch.uint8).fill_(FILL)
                self.storage[key] = wide
                td[key] = wide[:, :, :inner].unflatten(2, t.shape[2:])
                assert td[key].shape == t.shape and td[key].data_ptr() == wide.data_ptr()

    return SentinelBatch, PaddedBatch


def _make_runner(tmp_path, name, mac, padded=False, **extra):
    import torch
    from mapfx.episode import OneHot
    from mapfx.runners import ParallelRunner
    case = CASES[name]
    ref = reference(name)
    rows = case["grid"]
    mp = tmp_path / "m.map"
    mp.write_text("type octile\nheight %d\nwidth %d\nmap\n%s\n" % (len(rows), len(rows[0]), "\n".join(rows)))
    N, B, src = case["N"], case["B"], ref["src"]

    def instance_fn(ep):
        run = ref["runs"][ep % RUNS]
        return run["starts"][src], run["goals"][src]

    sentinel, padded_cls = _batch_classes()
    args = types.SimpleNamespace(
        env="marl_partial", batch_size_run=B, device="cuda",
        env_args=dict(REWARDS, grid_file_path=str(mp), agents_path=str(tmp_path / "x-"),
                      n_agents=N, obs_window=case["win"], obs_knn_agents=case["K"],
                      episode_limit=case["limit"]),
        episode_batch_cls=padded_cls if padded else sentinel, test_nepisode=B,
        runner_log_interval=1, **extra)
    logger = Logger()
    runner = ParallelRunner(args, logger, instance_fn=instance_fn)
    info = runner.get_env_info()
    scheme = {"state": {"vshape": info["state_shape"]},
              "obs": {"vshape": info["obs_shape"], "group": "agents"},
              "actions": {"vshape": (1,), "group": "agents", "dtype": torch.long},
              "avail_actions": {"vshape": (info["n_actions"],), "group": "agents", "dtype": torch.int},
              "reward": {"vshape": (1,)}, "terminated": {"vshape": (1,), "dtype": torch.uint8}}
    runner.setup(scheme, {"agents": N}, {"actions": ("actions_onehot", [OneHot(out_dim=5)])}, mac)
    return runner, logger


def _kernel_args(name):
    m = re.search(r"(partial_(?:wg_)?kernel)<([^>]*)>", name)
    return (m.group(1), m.group(2).replace(" ", "")) if m else None


def _check(tmp_path, name, mode="padded", dtype="int64", padded=False):
    """The pattern of every case (module docstring).  mode: "padded" (the default `bs`
    of length B), "exact" (args.runner_exact_bs) or "unfused" (no bs_inv in the runner
    state: the separate actions / env step / post / compaction launches)."""
    import torch
    from mapfx import _abi
    _assert_terminations(name)
    case, ref = CASES[name], reference(name)
    B, src = case["B"], ref["src"]
    P = case.get("tile", B)
    if case.get("unfused"):
        mode = "unfused"
    src_t = torch.as_tensor(src, device="cuda")
    mac = TableMAC(getattr(torch, dtype), src_t)
    extra = {"runner_exact_bs": True} if mode == "exact" else {}
    runner, logger = _make_runner(tmp_path, name, mac, padded=padded, **extra)
    if mode == "unfused":
        runner._rs.bs_inv = None
    member = np.zeros(P, bool)
    for r, run in enumerate(ref["runs"]):
        mac.start_run(run["table"], len(run["calls"]), runner.device)
        batch = runner.run(test_mode=False)
        kernel = _abi.last_kernel()
        td = batch.data.transition_data
        assert list(td) == list(run["batch"])
        for k, v in td.items():
            want = run["batch"][k][src]
            got = v.cpu().numpy()
            assert got.shape == want.shape and got.dtype == want.dtype, (r, k)
            same = got.view(np.uint8) == want.view(np.uint8)
            assert same.all(), (r, k, "first differing (env, t): %s" % np.argwhere(
                ~same.reshape(B, want.shape[1], -1).all(-1))[:8].tolist())
        if padded:
            for k, wide in batch.storage.items():
                inner = int(np.prod(td[k].shape[2:]))
                pad = wide[:, :, inner:].contiguous().view(torch.uint8)
                assert bool((pad == FILL).all()), (r, k)
        assert np.array_equal(runner._ep_return.cpu().numpy().view(np.uint64),
                              run["returns"][src].view(np.uint64)), r
        assert np.array_equal(runner._ep_length.cpu().numpy(), run["lengths"][src]), r
        assert runner.t_env == run["t_env"], r
        # the MAC's calls
        n_ref = len(run["calls"])
        assert [t for t, _ in mac.calls] == list(range(len(mac.calls)))
        if mode == "exact":
            assert len(mac.calls) == n_ref, (r, len(mac.calls), n_ref)
        assert len(mac.calls) >= n_ref
        for (t_ep, bs_ref), (_, bs) in zip(run["calls"], mac.calls):
            member[:] = False
            member[list(bs_ref)] = True
            want = np.nonzero(member[src])[0]
            got = bs.cpu().numpy()
            if mode == "exact":
                assert np.array_equal(got, want), (r, t_ep)
            else:
                assert got.shape == (B,) and np.array_equal(got[:len(want)], want), (r, t_ep)
                assert (got[len(want):] == want[0]).all(), (r, t_ep)
        if len(mac.calls) > n_ref:      # the calls past the reference's last wrote nothing
            for k, v in td.items():
                assert torch.equal(v, mac.snap[k]), (r, k)
        want_kernel = case["kernel"]
        if mode == "unfused" and want_kernel[1].split(",")[2:3] not in ([], ["0"]):
            # the plain step of a fast instance is compiled without the runner's half
            # (the generic partial_kernel<WIN, 0, 0> has one form)
            want_kernel = (want_kernel[0], want_kernel[1].replace("true", "false"))
        assert _kernel_args(kernel) == want_kernel, kernel
    assert logger.stats == ref["log"]


MATRIX = [n for n in CASES]


@pytest.mark.gpu
@pytest.mark.parametrize("name", MATRIX)
def test_runner_kernel_instance_matches_reference_loop(tmp_path, name):
    _check(tmp_path, name)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["int8", "int32"])
def test_runner_action_dtypes(tmp_path, dtype):
    """The fused step's 8-byte action-block decode at odd element offsets (N = 5): the
    MAC returns int8 / int32 (int64 is the matrix's)."""
    _check(tmp_path, "fast8_n5", dtype=dtype)


@pytest.mark.gpu
def test_runner_padded_batch(tmp_path):
    """EpisodeBatch tensors that are views of wider storage (time stride = row + 1
    element for obs, + 3 for the small fields): the stride arithmetic and the staged
    copy-out at destinations of every 16-byte misalignment; the padding keeps its fill."""
    _check(tmp_path, "fast8_n7", padded=True)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["fast16_n16", "fast8_n5", "wg_n70", "cmp_fused_2049"])
@pytest.mark.parametrize("mode", ["exact", "unfused"])
def test_runner_modes_write_the_same_bytes(tmp_path, name, mode):
    """runner_exact_bs (the MAC's calls are then exactly the reference loop's: as many,
    with the same bs) and the unfused launches fill the batch like the default form."""
    _check(tmp_path, name, mode=mode)
