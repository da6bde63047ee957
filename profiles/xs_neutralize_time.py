"""Time of engine.neutralize beside the two stage-3 yardsticks on the same tensors.

    python profiles/xs_neutralize_time.py [--rows 58 --days 2500 --stocks 5000 --industries 31]
Seeded heavy-tailed exposures (2 % NULL, 1 % ABSENT, a few NaN), 31 industries (3 % of
the stocks without one), ln-cap-like size covariate (2 % NULL), winsor = 3, standardise.
Device events around each call after a warm-up, median of --reps; algorithmic bytes are
9 B in + 9 B out per element for all three (the side inputs of neutralize are per day:
1 / rows of that).  Prints one JSON line.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "replication-of-minute-frequency-factor_amd"))
from mff import engine  # noqa: E402


def timed(fn, reps, warmup=2):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return float(np.median(ms)), float(np.min(ms)), float(np.max(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=58)
    ap.add_argument("--days", type=int, default=2500)
    ap.add_argument("--stocks", type=int, default=5000)
    ap.add_argument("--industries", type=int, default=31)
    ap.add_argument("--reps", type=int, default=7)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("xs_neutralize_time.py needs a GPU: a CPU run says nothing about kernel time")
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev)
    gen.manual_seed(20240501)
    R, D, S, G = a.rows, a.days, a.stocks, a.industries
    val = torch.empty((R, D, S), dtype=torch.float64, device=dev)
    state = torch.empty((R, D, S), dtype=torch.uint8, device=dev)
    for r in range(R):  # row by row: no second panel-sized temporary
        n = torch.randn((D, S), dtype=torch.float64, device=dev, generator=gen)
        w = torch.randn((D, S), dtype=torch.float64, device=dev, generator=gen)
        u = torch.rand((D, S), device=dev, generator=gen)
        val[r] = n * torch.exp(0.7 * w)  # heavy tails
        val[r][u > 0.999] = float("nan")
        state[r] = torch.where(u < 0.01, engine.ABSENT, torch.where(u < 0.03, engine.NULL, engine.VALUE)).to(torch.uint8)
    group = torch.randint(0, G, (D, S), device=dev, generator=gen, dtype=torch.int32)
    group[torch.rand((D, S), device=dev, generator=gen) < 0.03] = -1
    size = 23.0 + 1.5 * torch.randn((D, S), dtype=torch.float64, device=dev, generator=gen)
    size_state = torch.where(torch.rand((D, S), device=dev, generator=gen) < 0.02, engine.NULL,
                             engine.VALUE).to(torch.uint8)
    torch.cuda.synchronize()
    calls = {
        "neutralize": lambda: engine.neutralize(val, state, group, size, size_state, G=G, winsor=3.0),
        "neutralize_no_winsor": lambda: engine.neutralize(val, state, group, size, size_state, G=G, winsor=0.0),
        "neutralize_winsor_only": lambda: engine.neutralize(val, state, winsor=3.0),
        "neutralize_industry_only": lambda: engine.neutralize(val, state, group, G=G, winsor=0.0),
        "neutralize_size_only": lambda: engine.neutralize(val, state, None, size, size_state, winsor=0.0),
        "neutralize_standardize_only": lambda: engine.neutralize(val, state, winsor=0.0),
        "xs_z": lambda: engine.cross_section(val, state, "z"),
        "xs_rank": lambda: engine.cross_section(val, state, "rank"),
    }
    nbytes = 18 * val.numel()
    out = {"rows": R, "days": D, "stocks": S, "industries": G, "bytes": nbytes,
           "device": torch.cuda.get_device_name(0)}
    for name, fn in calls.items():
        med, lo, hi = timed(fn, a.reps)
        out[name] = {"ms": round(med, 3), "min_ms": round(lo, 3), "max_ms": round(hi, 3),
                     "TBps": round(nbytes / med / 1e9, 3)}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
