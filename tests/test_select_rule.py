"""CPU checks of the device action selection (include/mapfx_runner.h mapfx_select_actions):
the key of its random words, the numpy restatement that defines the rule
(mapfx.rng.select_actions) against torch on the CPU and against the distributions of
PyMARL's selectors, and the C ABI's refusals (no GPU: a launch would fail differently)."""
import ctypes

import numpy as np
import torch

M64 = (1 << 64) - 1
K_ENV, K_T, K_AGENT, K_STREAM = (0xD1B54A32D192ED03, 0xABC98388FB8FAC03, 0x8CB92BA72F3D8DD7,
                                 0xF1357AEA2E62A9C5)


def _splitmix64(x):
    x = (x + 0x9E3779B97F4A7C15) & M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M64
    return x ^ (x >> 31)


def _word(seed, gid, t, a):
    """u of the issue, in Python integers."""
    return _splitmix64(seed ^ (gid * K_ENV & M64) ^ ((t & 0xFFFFFFFF) * K_T & M64)
                       ^ (a * K_AGENT & M64) ^ (0x700 * K_STREAM & M64))


def test_select_word_key_pin():
    from mapfx import lib, rng
    assert rng.STREAM_SELECT == 0x700
    envs, ts, agents = [0, 1, 4095, 123456789], [0, 1, 2 ** 31 - 1], [0, 15, 63]
    for seed in (0, 12345, 0xFEDCBA9876543210):
        for t in ts:
            words = rng.select_words(seed, envs, t, 64)
            for ei, e in enumerate(envs):
                for a in agents:
                    w = _word(seed, e, t, a)
                    assert lib.mapfx_select_word(seed, e, t, a) == w, (seed, e, t, a)
                    assert int(words[ei, a]) == w, (seed, e, t, a)
    # a stream of its own: not the action generator's word (no stream term)
    assert _word(7, 3, 2, 1) != _splitmix64(7 ^ (3 * K_ENV & M64) ^ (2 * K_T & M64) ^ (1 * K_AGENT & M64))


def _special_q(rs, rows, N, A):
    """Random Q on a coarse lattice (ties), with rows of -inf, NaN and all-equal values."""
    q = (rs.randint(-3, 4, size=(rows, N, A)) * 0.5).astype(np.float32)
    q[1] = 0.25                                   # every action ties
    q[2, :, 1] = -np.inf
    q[3] = -np.inf                                # all -inf
    q[4, :, 2] = np.nan
    q[5, :, 1] = np.nan
    q[5, :, 3] = np.nan                           # the first NaN wins
    q[6, :, 0] = np.inf
    q[6, :, 4 % A] = np.nan                       # a NaN beats +inf
    return q


def test_restatement_greedy_equals_torch_max():
    from mapfx import rng
    rs = np.random.RandomState(5)
    rows, N, A = 64, 7, 5
    q = _special_q(rs, rows, N, A)
    avail = (rs.random_sample((rows, N, A)) < 0.6).astype(np.int32)
    avail[8] = 0                                  # nothing available
    avail[4, :, 2] = 1                            # the NaNs of rows 4 .. 6 stay visible
    avail[5] = 1
    avail[6] = 1
    avail[9] = 1
    ids = np.arange(rows)
    tq, ta = torch.from_numpy(q), torch.from_numpy(avail)
    for av_np, av_t in ((avail, ta), (None, torch.ones_like(ta))):
        masked = tq.clone()
        masked[av_t == 0.0] = -float("inf")
        ref = masked.max(dim=2)[1].numpy()
        for eps_q, greedy in ((0, False), (2 ** 32, True), (2 ** 31, True)):
            got = rng.select_actions(11, ids, 3, q, av_np, eps_q=eps_q, mode="epsilon_greedy",
                                     greedy_only=greedy)
            assert got.dtype == np.int64 and np.array_equal(got, ref), (eps_q, greedy)
        masked = tq.clone()
        masked[av_t == 0.0] = 0.0
        ref = masked.max(dim=2)[1].numpy()
        got = rng.select_actions(11, ids, 3, q, av_np, mode="multinomial", greedy_only=True)
        assert np.array_equal(got, ref)
    # the stated indices themselves
    assert rng.greedy_index(np.float32([[-np.inf] * 5, [1, 2, 2, 0, 2], [0, np.nan, 9, np.nan, 1]])).tolist() \
        == [0, 1, 1]
    # s not a finite number above 0: the multinomial falls back to greedy(p)
    p = np.zeros((3, 1, 5), np.float32)
    p[1, 0] = [0.1, np.inf, 0.2, 0, 0]
    p[2, 0] = [0.5, np.nan, 0.2, 0, 0]
    assert rng.select_actions(1, [0, 1, 2], 0, p, mode="multinomial").reshape(-1).tolist() == [0, 1, 1]


ROWS, N_AG, A5 = 4096, 16, 5


def _masks():
    m = (np.random.RandomState(2024).random_sample((ROWS, N_AG, A5)) < 0.5).astype(np.int32)
    m[..., 4] = 1                                 # stay is always available
    return m


def _within(count, n, p, what):
    """|count - n p| <= 5 sd of Binomial(n, p): a condition, not a measurement."""
    sd = np.sqrt(n * p * (1 - p))
    assert abs(count - n * p) <= 5 * sd, (what, count, n * p, sd)


def test_restatement_epsilon_greedy_distribution():
    from mapfx import rng
    m = _masks()
    n_av = m.sum(-1)
    ids = np.arange(ROWS)
    # two Q tables whose greedy actions differ wherever an agent has two available actions
    # (stay against the lowest other one): the two selections agree exactly where the agent
    # explored, since the random branch does not read Q
    q_stay = np.zeros((ROWS, N_AG, A5), np.float32)
    q_stay[..., 4] = 1.0
    q_low = np.zeros((ROWS, N_AG, A5), np.float32)
    q_low[..., :4] = np.arange(4, 0, -1, dtype=np.float32)
    two = n_av >= 2
    for eps in (0.05, 0.5):
        eps_q = int(round(eps * 2 ** 32))
        explored = total = 0
        for seed in (12345, 99):
            for t in range(8):
                a1 = rng.select_actions(seed, ids, t, q_stay, m, eps_q=eps_q)
                a2 = rng.select_actions(seed, ids, t, q_low, m, eps_q=eps_q)
                assert (np.take_along_axis(m, a1[..., None], -1) == 1).all()   # never an unavailable one
                assert (np.take_along_axis(m, a2[..., None], -1) == 1).all()
                explored += int((a1 == a2)[two].sum())
                total += int(two.sum())
        _within(explored, total, eps, "explore fraction at eps %g" % eps)
    # eps = 1: every draw is the random branch; uniform over the available actions per n
    cells = np.zeros((6, 5), np.int64)            # [n][rank of the action among the available]
    per_n = np.zeros(6, np.int64)
    rank = np.cumsum(m, -1) - 1
    for seed in (12345, 99):
        for t in range(8):
            a = rng.select_actions(seed, ids, t, q_stay, m, eps_q=2 ** 32)
            assert (np.take_along_axis(m, a[..., None], -1) == 1).all()
            r = np.take_along_axis(rank, a[..., None], -1)[..., 0]
            np.add.at(cells, (n_av, r), 1)
            np.add.at(per_n, n_av, 1)
    for n in range(1, 6):
        assert per_n[n] > 0
        assert cells[n, n:].sum() == 0
        if n == 1:
            assert cells[1, 0] == per_n[1]
            continue
        for j in range(n):
            _within(cells[n, j], per_n[n], 1.0 / n, "uniform cell n=%d j=%d" % (n, j))
    # greedy_only and eps_q = 0 never explore
    for kw in (dict(eps_q=0), dict(eps_q=2 ** 32, greedy_only=True)):
        assert (rng.select_actions(12345, ids, 0, q_stay, m, **kw) == 4).all()


def test_restatement_multinomial_distribution():
    from mapfx import rng
    p = np.float32([0.1, 0.3, 0.0, 0.4, 0.2])     # action 2 has p = 0, action 3 is masked
    mask = np.int32([1, 1, 1, 0, 1])
    q = np.broadcast_to(p, (ROWS, N_AG, A5)).copy()
    m = np.broadcast_to(mask, (ROWS, N_AG, A5)).copy()
    ids = np.arange(ROWS)
    counts = np.zeros(5, np.int64)
    for seed in (12345, 99):
        for t in range(4):
            a = rng.select_actions(seed, ids, t, q, m, mode="multinomial")
            counts += np.bincount(a.reshape(-1), minlength=5)
    total = int(counts.sum())
    assert counts[2] == 0 and counts[3] == 0
    eff = np.where(mask != 0, p, 0).astype(np.float64)
    for i in (0, 1, 4):
        _within(counts[i], total, eff[i] / eff.sum(), "multinomial action %d" % i)
    # test_greedy: greedy(p) with the masked zero taking part
    assert (rng.select_actions(1, ids, 0, q, m, mode="multinomial", greedy_only=True) == 1).all()


def test_select_actions_abi_refusals():
    """Every refusal comes before any launch: this test has no device, where a launch returns
    MAPFX_EHIP (-2), not MAPFX_EINVAL (-1)."""
    from mapfx import lib
    from mapfx._abi import SelArgs
    qbuf = (ctypes.c_float * 64)()
    abuf = (ctypes.c_int64 * 64)()
    vbuf = (ctypes.c_int32 * 64)()
    q, act, av = (ctypes.addressof(b) for b in (qbuf, abuf, vbuf))

    def call(**kw):
        a = SelArgs(rows=2, N=3, A=5, q=q, q_sr=15, avail=None, avail_sr=0, avail_form=0, env_ids=None,
                    env_offset=0, seed=1, eps_q=2 ** 31, t=0, mode=0, greedy_only=0, actions=act,
                    actions_sr=3)
        for k, v in kw.items():
            setattr(a, k, v)
        return lib.mapfx_select_actions(ctypes.byref(a), None), lib.mapfx_last_error()

    assert lib.mapfx_select_actions(None, None) == -1 and b"NULL args" in lib.mapfx_last_error()
    for kw, what in (({"q": None}, b"NULL q"), ({"actions": None}, b"NULL q / actions"),
                     ({"rows": -1}, b"rows < 0"), ({"N": 0}, b"N < 1"),
                     ({"A": 0}, b"A not in 1..9"), ({"A": 10}, b"A not in 1..9"),
                     ({"rows": 1 << 30, "N": 2}, b"below 2^31"),
                     ({"mode": 2}, b"unknown mode"), ({"mode": -1}, b"unknown mode"),
                     ({"avail_form": 2}, b"unknown avail_form"),
                     ({"eps_q": 2 ** 32 + 1}, b"eps_q above 2^32"),
                     ({"q_sr": 14}, b"q row stride"),
                     ({"avail": av, "avail_sr": 14}, b"avail row stride"),
                     ({"avail": av, "avail_form": 1, "avail_sr": 2}, b"avail row stride"),
                     ({"actions_sr": 2}, b"actions row stride")):
        rc, msg = call(**kw)
        assert rc == -1 and what in msg, (kw, rc, msg)
    assert call(rows=0)[0] == 0
    assert call(rows=0, q=None, actions=None)[0] == 0
    assert call(rows=0, A=10)[0] == -1            # an empty call is still checked
