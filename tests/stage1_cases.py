"""The panel of the stage-1 bound tests (tests/test_stage1_ref.py on the CPU,
tests/test_gpu_stage1_bounds.py on the GPU): D = 2, S = 161, i.e. 322 stock-days in the
flattened sd = d * S + s order of the serial kernels -- five full 64-lane pair blocks plus a
2-lane tail, one 256-lane block plus a 66-lane tail for set H and the non-pair kernels, a block
across the day boundary (161 is a multiple of neither 64 nor 4), and with stock-days 0..63
all-present or suspended a wholly dense wave (the full-wave walk) next to ragged ones.

Every stock-day is (price kind, volume kind, presence kind), seeded, on the 0.01 tick, fp32
prices (volume f64: counts beyond fp32's integers), absent bars NaN.  The kinds are the days
on which a walk that lost its shift, accumulated in f32 or took an f32 quotient goes wrong:
see PRICE, VOLUME and PRESENCE below.  `spec(sd)` names a stock-day's kinds.
"""
import numpy as np

D, S, T = 2, 161, 240
TICK = 0.01
SEED = 20260301


def _walk(rng, p0, step=3, lo=None, hi=None):
    """Closes on the tick from p0 (in ticks), steps in [-step, step], reflected into [lo, hi]."""
    c = np.empty(T, np.int64)
    p = p0
    for t in range(T):
        p += int(rng.integers(-step, step + 1))
        if lo is not None and p < lo:
            p = 2 * lo - p
        if hi is not None and p > hi:
            p = 2 * hi - p
        c[t] = p
    return c


def _ohlc(rng, c, p0, wick=2):
    """open = previous close, high / low within `wick` ticks beyond max / min(open, close)."""
    o = np.concatenate([[p0], c[:-1]])
    h = np.maximum(o, c) + rng.integers(0, wick + 1, T)
    lo = np.maximum(np.minimum(o, c) - rng.integers(0, wick + 1, T), 1)
    return o, h, lo, c


def _plain(rng):
    p0 = int(rng.integers(500, 10000))
    return _ohlc(rng, _walk(rng, p0, 3, lo=100), p0)


def _hi2000(rng):          # closes 1999.90..1999.93: level 2000, 3-tick range
    return _ohlc(rng, _walk(rng, 199991, 1, 199990, 199993), 199991)


def _hi500(rng):           # closes 499.90..499.95
    return _ohlc(rng, _walk(rng, 49992, 2, 49990, 49995), 49992)


def _penny(rng):           # 1.00..1.05
    c = _walk(rng, 102, 1, 100, 105)
    o = np.concatenate([[102], c[:-1]])
    return o, np.minimum(np.maximum(o, c) + rng.integers(0, 2, T), 105), np.maximum(np.minimum(o, c) - rng.integers(0, 2, T), 100), c


def _ramp(rng):            # +10 % over the day, local variation 1-2 ticks
    p0 = int(rng.integers(800, 3000))
    c = np.rint(p0 * (1.0 + 0.1 * np.arange(1, T + 1) / T)).astype(np.int64) + rng.integers(0, 2, T)
    return _ohlc(rng, c, p0, wick=1)


def _stretch(L):
    def f(rng):            # a moving day whose low, then high, stays put for exactly L bars
        o, h, lo, c = _plain(rng)
        a, b = 20, 130
        lo[a:a + L] = lo[a:a + L].min() - 1
        lo[a - 1] = lo[a] - 1
        lo[a + L] = lo[a] - 1 if lo[a + L] == lo[a] else lo[a + L]
        h[b:b + L] = h[b:b + L].max() + 1
        h[b - 1] = h[b] + 1
        h[b + L] = h[b] + 1 if h[b + L] == h[b] else h[b + L]
        return o, h, np.maximum(lo, 1), c
    return f


def _flat(rng):            # one price all day: every set constant
    p = np.full(T, int(rng.integers(100, 200000)), np.int64)
    return p, p.copy(), p.copy(), p.copy()


def _ret_all_but(ups, downs):
    def f(rng):            # close == open on every bar but `ups` up bars and `downs` down bars
        p = int(rng.integers(300, 150000))
        o = np.full(T, p, np.int64)
        c = o.copy()
        k = rng.choice(T, ups + downs, replace=False)
        c[k[:ups]] += 1
        c[k[ups:]] -= 1
        return o, np.maximum(o, c) + 1, np.minimum(o, c) - 1, c
    return f


def _flatgrid(rng):        # close == open at prices from the whole [1, 2000] grid; 40 bars move a tick
    o = rng.integers(100, 200001, T)
    c = o.copy()
    k = rng.choice(T, 40, replace=False)
    c[k] += rng.choice([-1, 1], 40)
    c = np.clip(c, 100, 200000)
    return o, np.maximum(o, c) + rng.integers(0, 3, T), np.maximum(np.minimum(o, c) - rng.integers(0, 3, T), 1), c


PRICE = {"plain": _plain, "hi2000": _hi2000, "hi500": _hi500, "penny": _penny, "ramp": _ramp,
         "stretch49": _stretch(49), "stretch50": _stretch(50), "stretch51": _stretch(51),
         "flat": _flat, "up0": _ret_all_but(0, 1), "up1": _ret_all_but(1, 0), "up2": _ret_all_but(2, 1),
         "down2": _ret_all_but(0, 2), "flatgrid": _flatgrid}


def _v_plain(rng):
    v = np.rint(np.exp(rng.normal(9.0, 1.0, T)) / 100.0) * 100.0
    v[rng.random(T) < 0.02] = 0.0
    return v


def _v_pm100(rng):         # 1,000,000 +- 100
    return 1e6 + rng.integers(-100, 101, T).astype(np.float64)


def _v_eq1(rng):           # all bars equal but one
    v = np.full(T, 1e6)
    v[int(rng.integers(1, T - 1))] += 100.0
    return v


def _v_odd(rng):           # odd counts above 2^24 (not fp32 integers)
    return 2.0 ** 24 + 1.0 + 2.0 * rng.integers(0, 50, T)


def _v_big(rng):           # one bar at the contract's maximum, mid-day
    v = _v_pm100(rng)
    v[121] = 2.0 ** 32 - 2.0
    return v


def _v_zero(rng):          # zero-volume bars interleaved
    v = _v_pm100(rng)
    v[rng.random(T) < 0.3] = 0.0
    v[::7] = 0.0
    return v


VOLUME = {"plain": _v_plain, "pm100": _v_pm100, "eq1": _v_eq1, "odd": _v_odd, "big": _v_big, "zero": _v_zero}


def _bars(*idx):
    m = np.zeros(T, bool)
    for i in idx:
        m[i] = True
    return m


PRESENCE = {
    "full": lambda rng: np.ones(T, bool),
    "suspended": lambda rng: np.zeros(T, bool),
    "nofirst": lambda rng: ~_bars(0),
    "nolast": lambda rng: ~_bars(T - 1),
    "no15": lambda rng: ~_bars(15),
    "no16": lambda rng: ~_bars(16),
    "upto15": lambda rng: _bars(slice(0, 16)),
    "from16": lambda rng: _bars(slice(16, T)),
    "alternate": lambda rng: _bars(slice(0, T, 2)),
    "run49": lambda rng: _bars(slice(100, 149)),
    "run50": lambda rng: _bars(slice(100, 150)),
    "run51": lambda rng: _bars(slice(100, 151)),
    "single": lambda rng: _bars(77),
    "two": lambda rng: _bars(3, 200),
    "quad": lambda rng: ~_bars(5),           # bars 0..3 an all-present quad, the next quad misses one
    "gap": lambda rng: ~_bars(slice(60, 131)),
    "holes": lambda rng: rng.random(T) >= 0.1,
}
_RAGGED = [k for k in PRESENCE if k not in ("full", "suspended")]
_PK, _VK = list(PRICE), list(VOLUME)
DENSE_SUSPENDED = (7, 40)


def spec(sd):
    """(price kind, volume kind, presence kind) of stock-day sd = d * S + s."""
    if sd < 64:
        pres = "suspended" if sd in DENSE_SUSPENDED else "full"
    else:
        j = sd - 64
        pres = "full" if j % 3 == 2 else _RAGGED[(j - j // 3) % len(_RAGGED)] if j % 41 else "suspended"
    return _PK[sd % len(_PK)], _VK[(sd // 2 + sd // len(_PK)) % len(_VK)], pres


def panel():
    """Host panel dict of mff.synth's layout (engine.validate_host_panel accepts it)."""
    o, h, lo, c = (np.full((D, S, T), np.nan, np.float32) for _ in range(4))
    v = np.full((D, S, T), np.nan, np.float64)
    present = np.zeros((D, S, T), bool)
    for sd in range(D * S):
        rng = np.random.default_rng([SEED, sd])
        pk, vk, rk = spec(sd)
        d, s = divmod(sd, S)
        m = PRESENCE[rk](rng)
        po, ph, pl, pc = PRICE[pk](rng)
        pv = VOLUME[vk](rng)
        for dst, src in ((o, po), (h, ph), (lo, pl), (c, pc)):
            dst[d, s, m] = (np.round(src[m] * TICK, 2)).astype(np.float32)
        v[d, s, m] = pv[m]
        present[d, s] = m
    codes = sorted(f"{i:06d}.SZ" for i in range(1, S + 1))
    return {"open": o, "high": h, "low": lo, "close": c, "volume": v, "present": present,
            "codes": codes, "dates": ["2020-01-02", "2020-01-03"]}
