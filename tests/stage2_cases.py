"""Seeded stage-2 inputs shared by tests/test_stage2_ref.py and the GPU shape tests."""
import numpy as np


def panel(rows, D, S, seed, absent=0.05, null=0.02, nan=0.01):
    """[rows][D][S] factor values and states: column scales 1e-3 / 1 / 1e5, 30 % integer
    ties, NULL, NaN, +-inf entries, a constant column (3), a trend column 1e6 + 0.25 d
    drifting away from its first value (5) and one 1e15 outlier that leaves the window
    (day 20 of column 6); ``absent`` / ``null`` / ``nan`` of the entries ABSENT / NULL /
    NaN, half and a fifth of ``nan`` +inf and -inf (long windows need low rates to keep any
    window free of them).  Every row has its own seed, so
    no two rows, stock blocks or day segments hold the same values."""
    val = np.empty((rows, D, S))
    state = np.empty((rows, D, S), np.uint8)
    for r in range(rows):
        rng = np.random.default_rng([seed, r])
        v = rng.normal(size=(D, S)) * rng.choice([1e-3, 1.0, 1e5], size=(1, S))
        ties = rng.random((D, S)) < 0.3
        v[ties] = np.round(v[ties])
        st = np.full((D, S), 2, np.uint8)
        st[rng.random((D, S)) < absent] = 0
        st[rng.random((D, S)) < null] = 1
        v[rng.random((D, S)) < nan] = np.nan
        v[rng.random((D, S)) < nan / 2] = np.inf
        v[rng.random((D, S)) < nan / 5] = -np.inf
        if S > 3:
            v[:, 3] = 1.25 + r
        if S > 5:
            v[:, 5] = 1e6 * (r + 1) + 0.25 * np.arange(D)
        if S > 6 and D > 20:
            v[20, 6] = 1e15
            st[20, 6] = 2
        val[r], state[r] = v, st
    return val, state


def ragged_tail(state):
    """In the last row's last stock block: a 40-day suspension, a stock listed late and a
    stock present only every 9th day (the last three stocks; fewer when S < 3)."""
    D, S = state.shape[1:]
    r = state.shape[0] - 1
    if S >= 1:
        state[r, :, S - 1] = 0
        state[r, ::9, S - 1] = 2
    if S >= 2:
        state[r, : (3 * D) // 5, S - 2] = 0
    if S >= 3:
        state[r, D // 4: D // 4 + 40, S - 3] = 0
    return state
