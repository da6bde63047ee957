"""Crafted stage-3 days shared by the GPU tests of the cross-sectional rank and z-score
(test_gpu_parity.py, test_gpu_stage3_shapes.py)."""
import numpy as np

ABSENT, NULLV, VALUE = 0, 1, 2


def rank_distribution_days(S, rng):
    """(val [8][S], state [8][S]): the distributions that defeat a one-level histogram: one
    dominant exact tie (1.0) among near values, two tie groups one ulp apart, a dense
    cluster with far outliers (lognormal sigma 6), a range of a few denormals, only
    infinities and zeros of both signs, integer-valued days (heavy ties everywhere), a
    day of one value, a day of 70 % zeros among tiny values; 2 % NaN, 3 % NULL, 3 % ABSENT."""
    D = 8
    val = np.empty((D, S))
    val[0] = np.where(rng.random(S) < 0.5, 1.0, 1.0 + rng.integers(-30, 30, S) * 1e-3)
    val[1] = np.where(rng.random(S) < 0.4, 0.5, np.nextafter(0.5, 1.0))
    m = rng.random(S) < 0.2
    val[1, m] = 0.5 + rng.normal(size=int(m.sum())) * 1e-9
    val[2] = rng.lognormal(0.0, 6.0, S) * rng.choice([-1.0, 1.0], S)
    val[3] = rng.integers(0, 9, S) * 5e-324
    val[4] = rng.choice([np.inf, -np.inf, 0.0, -0.0, 1.0], S)
    val[5] = rng.integers(-3, 4, S).astype(float)
    val[6] = 3.25
    val[7] = np.where(rng.random(S) < 0.7, 0.0, rng.normal(size=S) * 1e-12)
    val[rng.random(val.shape) < 0.02] = np.nan
    state = np.full(val.shape, VALUE, np.uint8)
    state[rng.random(val.shape) < 0.03] = NULLV
    state[rng.random(val.shape) < 0.03] = ABSENT
    return val, state


HANDOVER_RUN = 300  # consecutive doubles of the hand-over day (> XR_MAXO = XD_MAXO = 48)


def handover_day(S, rng):
    """A day the bucketed rank kernels cannot keep: HANDOVER_RUN consecutive doubles stepped
    up from 1.0 among magnitudes spread log-uniformly over 1e-300 .. 1e300 of both signs.
    Linear buckets over +-1e300 put every small value into one bucket; buckets linear in the
    IEEE bits are binades wide, and a bucket's equal sub-ranges still are 2^40 ulps wide: the
    run shares one level-2 bucket under both schemes, with 299 keys that differ from the
    bucket's reference."""
    assert S >= HANDOVER_RUN + 50
    val = 10.0 ** rng.uniform(-300.0, 300.0, S) * rng.choice([-1.0, 1.0], S)
    pos = rng.choice(S, HANDOVER_RUN, replace=False)
    val[pos] = 1.0 + np.arange(HANDOVER_RUN) * 2.0 ** -52  # nextafter steps from 1.0
    state = np.full(S, VALUE, np.uint8)
    return val, state


def pattern_days(S, seed, handover=True):
    """(val [P][S], state [P][S], names, index of the hand-over day or None): the eight rank
    distributions, a continuous normal day, an all-ABSENT and an all-NULL day, a day of one
    included value, a day of two, and the hand-over day."""
    rng = np.random.default_rng(seed)
    v8, s8 = rank_distribution_days(S, rng)
    names = ["tie1", "ulp-ties", "lognormal6", "denormals", "inf-zero", "integers", "constant", "zeros-tiny"]
    vals, states = list(v8), list(s8)

    def add(name, v, s):
        names.append(name)
        vals.append(np.asarray(v, np.float64))
        states.append(np.asarray(s, np.uint8))

    v = rng.normal(size=S)
    s = np.full(S, VALUE, np.uint8)
    s[rng.random(S) < 0.02] = NULLV
    s[rng.random(S) < 0.02] = ABSENT
    add("normal", v, s)
    add("all-absent", rng.normal(size=S), np.full(S, ABSENT, np.uint8))
    add("all-null", rng.normal(size=S), np.full(S, NULLV, np.uint8))
    # one / two included values among ABSENT, NULL and VALUE-NaN stocks
    for k, name in ((1, "one-value"), (2, "two-values")):
        v = rng.normal(size=S)
        s = rng.choice(np.array([ABSENT, NULLV, VALUE], np.uint8), S)
        v[s == VALUE] = np.nan
        keep = rng.choice(S, min(k, S), replace=False)
        s[keep] = VALUE
        v[keep] = rng.normal(size=keep.size)
        add(name, v, s)
    hand = None
    if handover:
        hand = len(names)
        add("hand-over", *handover_day(S, rng))
    return np.stack(vals), np.stack(states), names, hand
