"""GPU tests of the device action selection (include/mapfx_runner.h mapfx_select_actions,
mapfx/selectors.py): the kernel against the rule's numpy restatement
(mapfx.rng.select_actions) bit for bit, the selectors through the batched ParallelRunner
(the same actions from the padded and from the exact `bs`), shard invariance and graph
replay."""
import ctypes
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GUARD = 64        # bytes of 0xA5 on each side of the actions buffer
SEED = 0x5EED0123456789AB
MODES = ("epsilon_greedy", "multinomial")


def _q(rs, rows, N, A, mode):
    """[rows, N, A] float32: Q-values on a coarse lattice (ties) or policies with rounding
    prefix sums, and per (row, agent) specials: all equal, a -inf, NaNs, all zero, all -inf."""
    flat = rows * N
    if mode == "epsilon_greedy":
        q = (rs.randint(-3, 4, size=(flat, A)) * 0.5).astype(np.float32)
    else:
        q = rs.random_sample((flat, A)).astype(np.float32)
        q[::2] = (rs.randint(0, 4, size=(flat, A)) * 0.125).astype(np.float32)[::2]
    k = np.arange(flat) % 11
    q[k == 1] = 0.25
    q[k == 2, A // 2] = -np.inf
    q[k == 3, A - 1] = np.nan
    q[k == 3, A // 3] = np.nan
    q[k == 4] = 0.0
    q[k == 5] = -np.inf
    return q.reshape(rows, N, A)


def _avail(rs, rows, N, A):
    m = (rs.random_sample((rows * N, A)) < 0.6).astype(np.int32)
    m[np.arange(rows * N) % 13 == 6] = 0          # nothing available
    m[m != 0] = rs.randint(1, 1000, size=int((m != 0).sum()))   # any nonzero value counts
    return m.reshape(rows, N, A)


def _env_id_forms(rs, rows):
    perm = rs.permutation(rows).astype(np.int64)
    live = np.sort(rs.choice(rows, size=(rows + 1) // 2, replace=False)).astype(np.int64)
    padded = np.concatenate([live, np.full(rows - live.shape[0], live[0], np.int64)])
    return {"none": None, "perm": perm, "padded": padded}


def _strided(arr, pad, fill):
    """`arr` [rows, inner...] as a device tensor whose rows are `pad` elements further apart."""
    rows = arr.shape[0]
    inner = int(np.prod(arr.shape[1:]))
    buf = torch.full((rows, inner + pad), fill, dtype=torch.from_numpy(arr[:0]).dtype, device="cuda")
    buf[:, :inner] = torch.from_numpy(arr.reshape(rows, inner)).cuda()
    return buf, inner + pad


@pytest.mark.parametrize("shape", [(1, 1, 5), (3, 5, 5), (7, 64, 5), (65, 16, 5), (5, 3, 9), (4, 2, 1)],
                         ids=lambda s: "%dx%dx%d" % s)
def test_kernel_matches_restatement(shape):
    from mapfx import _abi, rng
    from mapfx._abi import SelArgs, lib
    rows, N, A = shape
    rs = np.random.RandomState(1000 * rows + 10 * N + A)
    av_np = _avail(rs, rows, N, A)
    bits_np = (av_np != 0).astype(np.int64) @ (1 << np.arange(A))
    bits_np = bits_np.astype(np.uint8) if A <= 8 else bits_np.astype(np.uint16).view(np.int16)
    ids = _env_id_forms(rs, rows)
    ids_dev = {k: None if v is None else torch.from_numpy(v).cuda() for k, v in ids.items()}
    env_offset, t = 1 << 33, 2 ** 31 - 5
    stream = torch.cuda.current_stream().cuda_stream
    launches = 0
    for mode in MODES:
        q_np = _q(rs, rows, N, A, mode)
        for dense in (True, False):
            pad = 0 if dense else 7
            q_dev, q_sr = _strided(q_np, pad, 123.0)
            av_dev, av_sr = _strided(av_np, pad and 3, 1)
            bits_dev, bits_sr = _strided(bits_np, pad and 5, 0x7F)
            act_sr = N + (pad and 2)
            for eps_q in ((0, 2 ** 31, 2 ** 32) if dense else (2 ** 31,)):
                for greedy in (False, True):
                    for form in ("i32", "bits", "null"):
                        for idk, idv in ids.items():
                            n8 = rows * act_sr * 8
                            buf = torch.full((2 * GUARD + n8,), 0xA5, dtype=torch.uint8, device="cuda")
                            avp, avs, avf = {"i32": (av_dev, av_sr, _abi.MAPFX_AVAIL_I32),
                                             "bits": (bits_dev, bits_sr, _abi.MAPFX_AVAIL_BITS),
                                             "null": (None, 0, 0)}[form]
                            a = SelArgs(rows=rows, N=N, A=A, q=q_dev.data_ptr(), q_sr=q_sr,
                                        avail=_abi.ptr(avp), avail_sr=avs, avail_form=avf,
                                        env_ids=_abi.ptr(ids_dev[idk]), env_offset=env_offset, seed=SEED,
                                        eps_q=eps_q, t=t, mode=rng.SELECT_MODES[mode],
                                        greedy_only=int(greedy), actions=buf.data_ptr() + GUARD,
                                        actions_sr=act_sr)
                            assert lib.mapfx_select_actions(ctypes.byref(a), stream) == 0, lib.mapfx_last_error()
                            assert ("select_kernel<%d>" % (5 if A == 5 else 0)) in _abi.last_kernel()
                            launches += 1
                            got = buf.cpu().numpy()
                            what = (mode, dense, eps_q, greedy, form, idk)
                            assert (got[:GUARD] == 0xA5).all() and (got[GUARD + n8:] == 0xA5).all(), what
                            body = got[GUARD:GUARD + n8].view(np.int64).reshape(rows, act_sr)
                            assert (body[:, N:] == np.frombuffer(b"\xa5" * 8, np.int64)[0]).all(), what
                            gids = env_offset + (np.arange(rows) if idv is None else idv)
                            ref = rng.select_actions(SEED, gids, t, q_np, None if form == "null" else av_np,
                                                     eps_q=eps_q, mode=mode, greedy_only=greedy)
                            assert np.array_equal(body[:, :N], ref), what
    assert launches == 2 * (3 + 1) * 2 * 3 * 3


def _inputs(rows, N, A, seed):
    rs = np.random.RandomState(seed)
    q = rs.random_sample((rows, N, A)).astype(np.float32)
    av = (rs.random_sample((rows, N, A)) < 0.6).astype(np.int32)
    return q, av


@pytest.mark.parametrize("mode", MODES)
def test_shard_invariance(mode):
    """Rows of envs 0..7 in one call = two calls of 4 rows with env_offset 0 and 4."""
    from mapfx import rng
    from mapfx.selectors import select_actions
    q, av = _inputs(8, 6, 5, 3)
    qd, ad = torch.from_numpy(q).cuda(), torch.from_numpy(av).cuda()
    kw = dict(eps=0.5, seed=77, t=12, mode=mode)
    full = select_actions(qd, ad, **kw)
    parts = [select_actions(qd[o:o + 4], ad[o:o + 4], env_offset=o, **kw) for o in (0, 4)]
    assert full.dtype == torch.int64 and torch.equal(full, torch.cat(parts))
    ref = rng.select_actions(77, np.arange(8), 12, q, av, eps_q=2 ** 31, mode=mode)
    assert np.array_equal(full.cpu().numpy(), ref)
    # the same envs given by id, in another order
    order = torch.tensor([5, 0, 7, 2], device="cuda")
    picked = select_actions(qd[order], ad[order], env_ids=order, **kw)
    assert torch.equal(picked, full[order])


def test_wrapper_converts_what_the_kernel_does_not_take():
    from mapfx import rng
    from mapfx.selectors import select_actions
    rows, N, A = 5, 4, 5
    q, av = _inputs(rows, N, A, 8)
    ref = rng.select_actions(9, np.arange(rows), 2, q, av, eps_q=2 ** 30)
    kw = dict(eps=0.25, seed=9, t=2)
    qd, ad = torch.from_numpy(q).cuda(), torch.from_numpy(av).cuda()
    q64_t = qd.double().permute(2, 0, 1).contiguous().permute(1, 2, 0)     # float64, not contiguous
    bits = torch.from_numpy(((av != 0) @ (1 << np.arange(A))).astype(np.uint8)).cuda()
    out = torch.full((rows, N), -1, dtype=torch.int64, device="cuda")
    for qq, aa in ((qd, ad), (q64_t, ad), (qd, ad.bool()), (qd, ad.float() * 0.5), (qd, bits)):
        got = select_actions(qq, aa, out=out.fill_(-1), **kw)
        assert got is out and np.array_equal(got.cpu().numpy(), ref)
    ref_all = rng.select_actions(9, np.arange(rows), 2, q, None, eps_q=2 ** 30)
    assert np.array_equal(select_actions(qd, None, **kw).cpu().numpy(), ref_all)
    assert select_actions(qd[:0], ad[:0], **kw).shape == (0, N)
    with pytest.raises(ValueError):
        select_actions(qd, ad, eps=1.5, seed=9, t=2)


def _sel_args(**kw):
    return types.SimpleNamespace(epsilon_start=1.0, epsilon_finish=0.05, epsilon_anneal_time=1000, seed=31, **kw)


def test_selector_classes_bound_and_unbound():
    from mapfx import rng
    from mapfx.selectors import REGISTRY
    rows, N, A = 6, 3, 5
    q, av = _inputs(rows, N, A, 4)
    qd, ad = torch.from_numpy(q).cuda(), torch.from_numpy(av).cuda()
    sel = REGISTRY["mapfx_epsilon_greedy"](_sel_args())
    for call in range(2):      # unbound: envs 0 .. rows - 1, the call counter, run 0
        got = sel.select_action(qd, ad, t_env=500)
        assert sel.epsilon == 1.0 - (1.0 - 0.05) / 1000 * 500
        ref = rng.select_actions(rng.runner_policy_seed(31, 0), np.arange(rows), call, q, av,
                                 eps_q=int(round(sel.epsilon * 2 ** 32)))
        assert np.array_equal(got.cpu().numpy(), ref)
    ids = np.array([4, 9, 9, 0, 2, 4])
    sel.bind(torch.from_numpy(ids).cuda(), t_ep=17, run=3, env_offset=100)
    got = sel.select_action(qd, ad, t_env=10 ** 6)
    assert sel.epsilon == 0.05
    ref = rng.select_actions(rng.runner_policy_seed(31, 3), 100 + ids, 17, q, av,
                             eps_q=int(round(0.05 * 2 ** 32)))
    assert np.array_equal(got.cpu().numpy(), ref)
    got = sel.select_action(qd, ad, t_env=0, test_mode=True)    # the binding held for one call
    assert sel.epsilon == 0.0
    assert np.array_equal(got.cpu().numpy(), rng.select_actions(0, np.arange(rows), 0, q, av, greedy_only=True))
    mul = REGISTRY["mapfx_multinomial"](_sel_args())
    assert mul.test_greedy is True
    got = mul.select_action(qd, ad, t_env=0)
    ref = rng.select_actions(rng.runner_policy_seed(31, 0), np.arange(rows), 0, q, av, mode="multinomial")
    assert np.array_equal(got.cpu().numpy(), ref)
    got = mul.select_action(qd, ad, t_env=0, test_mode=True)
    assert np.array_equal(got.cpu().numpy(),
                          rng.select_actions(0, np.arange(rows), 0, q, av, mode="multinomial", greedy_only=True))


def test_graph_replay_matches_eager():
    from mapfx.selectors import select_actions
    rows, N, A = 9, 16, 5
    q, av = _inputs(rows, N, A, 6)
    qd, ad = torch.from_numpy(q).cuda(), torch.from_numpy(av).cuda()
    ids = torch.arange(rows, device="cuda").flip(0)
    kw = dict(eps=0.5, seed=21, t=4, env_ids=ids, env_offset=7)
    eager = select_actions(qd, ad, **kw).cpu()
    out = torch.full((rows, N), -1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        select_actions(qd, ad, out=out, **kw)
    torch.cuda.synchronize()
    assert bool((out == -1).all()), "ran at capture time"
    for r in range(2):
        out.fill_(-1)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out.cpu(), eager), "replay %d" % r
    del graph, side


# ---- bs-invariance through the runner ----
RUN_SEED, RUN_EPS, RUN_LIMIT, RUN_N, RUN_B = 5, 0.25, 10, 2, 8
def run_instances(ep):
    """Envs 0..3 start on their goals (greedy = stay ends them after one step unless an agent
    explores away), envs 4..7 two cells from them (staying never ends them)."""
    starts = np.array([[[0, 0], [4, 4]], [[1, 3], [3, 1]], [[2, 2], [0, 4]], [[4, 0], [2, 3]]] * 2, np.int32)
    goals = starts.copy()
    goals[4:, :, 0] = (goals[4:, :, 0] + 2) % 5
    if ep % 2:
        starts, goals = starts[::-1].copy(), goals[::-1].copy()
    return starts, goals


# what _make_runner reads of a fixture (its own instance_fn, one instance for every env, is
# replaced by run_instances)
RUN_FX = {"map": np.array(["." * 5] * 5), "n_agents": RUN_N, "limit": RUN_LIMIT, "obs_window": 3,
          "obs_knn_agents": 1, "inst_starts": run_instances(0)[0][:1], "inst_goals": run_instances(0)[1][:1]}


def simulate_run(run):
    """The run on the CPU: oracle/partial_oracle.py envs, actions from the rule's restatement
    with the stay-preferring Q.  (actions [B, limit, N] with -1 past the end, lengths [B])"""
    from mapfx import rng
    from oracle.partial_oracle import PartialEnvState
    from test_gpu_runner import REWARDS
    starts, goals = run_instances(run)
    seed = rng.runner_policy_seed(RUN_SEED, run)
    q = np.zeros((1, RUN_N, 5), np.float32)
    q[..., 4] = 1.0
    acts = np.full((RUN_B, RUN_LIMIT, RUN_N), -1, np.int64)
    lengths = np.zeros(RUN_B, np.int64)
    for b in range(RUN_B):
        env = PartialEnvState(np.zeros((5, 5), np.int8), starts[b], goals[b], obs_window=3, obs_knn_agents=1,
                              episode_limit=RUN_LIMIT, **REWARDS)
        for t in range(RUN_LIMIT):
            a = rng.select_actions(seed, [b], t, q, env.avail()[None], eps_q=int(round(RUN_EPS * 2 ** 32)))[0]
            acts[b, t] = a
            lengths[b] = t + 1
            if env.step(a)[1]:
                break
    return acts, lengths


class StubMAC:
    """Q = an elementwise function of the env's own obs row that prefers stay."""

    def __init__(self, selector):
        self.action_selector = selector

    def init_hidden(self, batch_size):
        pass

    def select_actions(self, batch, t_ep, t_env, bs, test_mode=False):
        q = torch.tanh(batch["obs"][bs, t_ep][..., :5]) * 0.1
        q[..., 4] += 1.0
        return self.action_selector.select_action(q, batch["avail_actions"][bs, t_ep], t_env, test_mode)


def test_runner_same_actions_from_padded_and_exact_bs(tmp_path):
    from mapfx.selectors import DeviceEpsilonGreedySelector
    from test_gpu_runner import _make_runner
    results = {}
    for exact in (False, True):
        d = tmp_path / ("exact" if exact else "padded")
        d.mkdir()
        sargs = types.SimpleNamespace(epsilon_start=RUN_EPS, epsilon_finish=RUN_EPS, epsilon_anneal_time=1,
                                      seed=RUN_SEED)
        runner, logger = _make_runner(d, RUN_FX, RUN_B, StubMAC(DeviceEpsilonGreedySelector(sargs)),
                                      seed=RUN_SEED, runner_exact_bs=exact)
        runner._instance_fn = run_instances
        runs = []
        for r in range(2):
            batch = runner.run(test_mode=False)
            runs.append(({k: v.cpu().numpy() for k, v in batch.data.transition_data.items()},
                         runner.t_env, runner._ep_return.cpu().numpy(), runner._ep_length.cpu().numpy()))
        results[exact] = (runs, logger.stats)
    for r in range(2):
        (td_p, t_env_p, ret_p, len_p), (td_e, t_env_e, ret_e, len_e) = results[False][0][r], results[True][0][r]
        assert sorted(td_p) == sorted(td_e)
        for k in td_p:
            assert td_p[k].dtype == td_e[k].dtype and td_p[k].shape == td_e[k].shape, (r, k)
            assert np.array_equal(td_p[k].view(np.uint8), td_e[k].view(np.uint8)), (r, k)
        assert t_env_p == t_env_e
        assert np.array_equal(ret_p.view(np.uint64), ret_e.view(np.uint64))
        assert np.array_equal(len_p, len_e)
        # not vacuous: an env ended early, one did not, and an agent explored
        assert (len_p < RUN_LIMIT).any() and (len_p == RUN_LIMIT).any(), len_p
        acts = td_p["actions"][:, :RUN_LIMIT, :, 0]
        filled = np.arange(RUN_LIMIT)[None, :] < len_p[:, None]
        assert (acts[filled] != 4).any()
        # and they are the actions of the rule, on the oracle's envs
        sim_acts, sim_len = simulate_run(r)
        assert np.array_equal(len_p, sim_len)
        assert np.array_equal(acts[filled], sim_acts[filled])
    assert results[False][1] == results[True][1]
    assert any(k == "epsilon" and v == RUN_EPS for k, v, _ in results[True][1])
