"""Time of the composite-factor calls (include/mff.h, mff_xs_comb_*) beside the per-factor IC
route they replace.

    python profiles/xs_combine_time.py [--reps 7] [--sizes 58x2500x5000,58x40x5000]
Not a test; run by hand on the GPU.  Per size (factors x days x stocks) one child process (its
own time limit; the run stops at the first child that fails) generates seeded exposures
(pairwise correlation 0.25, 0.05 % NULL per row, a few NaN) and a forward return with a planted
IC, and times in that one process, kernels only (device events around the calls after two
warm-up calls, median of --reps):
  batched      mff_xs_comb_moments + mff_xs_comb_finalize: every factor's z-score moments and
               Pearson IC in one pass (the return plane read once, no pair planes)
  per_factor   the route before: per factor mff_ic_pairs + mff_ic_moments + mff_ic_finalize
               (K round trips, each re-reading the return plane and writing a [2][D][S] pair plane)
  apply        mff_xs_comb_apply alone, against its bytes K D S 9 read + D S 9 written
  weights_*    mff_xs_comb_weights alone, per method (window 60, min_periods 20, horizon 5)
  combine      engine.factor_combine(method='icir') end to end
and checks once that the batched ICs agree with the per-factor ones within rtol = atol = 1e-9.
Floors at 8 TB/s: batched reads (K + 1) D S 9 B; per_factor reads 2 and writes 2 planes of 9 B
in the pair pass and reads the pair planes twice in the moment pass (k_ic_moments walks them
twice), 8 D S 9 B per factor.  Prints one JSON line.
"""
import argparse
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "replication-of-minute-frequency-factor_amd"))
sys.path.insert(0, HERE)

from xs_corr_time import timed  # noqa: E402

HBM_BPS = 8.0e12
CHILD_LIMIT_S = 420
H, W, M = 5, 60, 20


def one(K, D, S, reps):
    import torch

    from mff import _lib, engine
    if not torch.cuda.is_available():
        raise SystemExit("xs_combine_time.py needs a GPU: a CPU run says nothing about kernel time")
    dev = torch.device("cuda:0")
    lib = _lib.load()
    gen = torch.Generator(device=dev)
    gen.manual_seed(20240901)
    f64, u8, i32 = torch.float64, torch.uint8, torch.int32
    rnd = lambda: torch.randn((D, S), dtype=f64, device=dev, generator=gen)
    val = torch.empty((K, D, S), dtype=f64, device=dev)
    state = torch.empty((K, D, S), dtype=u8, device=dev)
    common = rnd()
    yv = 0.02 * rnd()
    for r in range(K):  # row by row: no second panel-sized temporary
        u = torch.rand((D, S), device=dev, generator=gen)
        own = rnd()
        yv += (0.02 * 0.1 / K ** 0.5) * own
        val[r] = 0.5 * common + 0.866 * own
        val[r][u > 0.9999] = float("nan")
        state[r] = torch.where(u < 0.0005, engine.NULL, engine.VALUE).to(u8)
    del common, own
    ys = torch.full((D, S), engine.VALUE, dtype=u8, device=dev)
    ys[max(D - H, 0):] = engine.NULL
    torch.cuda.synchronize()

    st = engine._stream(dev)
    P = lambda t_: t_.data_ptr()
    part = torch.empty((K, D, 9), dtype=f64, device=dev)
    zmom = torch.empty((K, D, 3), dtype=f64, device=dev)
    ic = torch.empty((K, D), dtype=f64, device=dev)
    npairs = torch.empty((K, D), dtype=i32, device=dev)
    wts = torch.empty((D, K), dtype=f64, device=dev)
    count = torch.empty((D, K), dtype=i32, device=dev)
    status = torch.empty(D, dtype=i32, device=dev)
    ov = torch.empty((D, S), dtype=f64, device=dev)
    os_ = torch.empty((D, S), dtype=u8, device=dev)
    pv = torch.empty((2, D, S), dtype=f64, device=dev)
    ps = torch.empty((2, D, S), dtype=u8, device=dev)
    part1 = torch.empty((D, 6), dtype=f64, device=dev)
    ic_old = torch.empty((K, D), dtype=f64, device=dev)

    def batched():
        _lib.check(lib.mff_xs_comb_moments(P(val), P(state), K, D, S, P(yv), P(ys), 1, P(part), st), "moments")
        _lib.check(lib.mff_xs_comb_finalize(P(part), 1, K, D, 0, P(zmom), P(ic), P(npairs), st), "finalize")

    def per_factor():
        for k in range(K):
            _lib.check(lib.mff_ic_pairs(P(val[k]), P(state[k]), P(yv), P(ys), D, S, P(pv), P(ps), st), "pairs")
            _lib.check(lib.mff_ic_moments(P(pv), P(ps), D, S, P(part1), st), "ic_moments")
            _lib.check(lib.mff_ic_finalize(P(part1), 1, D, P(ic_old[k]), st), "ic_finalize")

    def weights(method):
        def call():
            _lib.check(lib.mff_xs_comb_weights(P(ic), K, D, method, H, W, M, 0.5, P(wts), P(count), P(status), st),
                       "weights")
        return call

    def apply_():
        _lib.check(lib.mff_xs_comb_apply(P(val), P(state), K, D, S, P(zmom), P(wts), P(status), 1, P(ov), P(os_), st),
                   "apply")

    def combine():
        return engine.factor_combine(val, state, yv, ys, method="icir", future_days=H, window=W, min_periods=M)

    res = {"factors": K, "days": D, "stocks": S, "device": torch.cuda.get_device_name(0)}
    res["batched"] = timed(torch, batched, reps)
    res["per_factor"] = timed(torch, per_factor, max(3, reps // 2), warmup=1)
    res["batched_faster"] = res["batched"]["ms"] <= res["per_factor"]["ms"]
    res["speedup"] = round(res["per_factor"]["ms"] / res["batched"]["ms"], 2)
    fin = torch.isfinite(ic_old)
    res["ic_nan_pattern_equal"] = bool(torch.equal(fin, torch.isfinite(ic)))
    res["ic_vs_per_factor_max_abs"] = float((ic - ic_old)[fin].abs().max()) if bool(fin.any()) else None
    res["ic_within_tolerance"] = bool(torch.allclose(ic[fin], ic_old[fin], rtol=1e-9, atol=1e-9))
    for i, name in enumerate(engine.COMBINE_METHODS):
        res[f"weights_{name}"] = timed(torch, weights(i), reps)
    weights(2)()
    res["status0_days"] = int((status == 0).sum())
    res["apply"] = timed(torch, apply_, reps)
    apply_bytes = (K + 1) * D * S * 9
    res["apply_bytes"] = apply_bytes
    res["apply_TBps"] = round(apply_bytes / (res["apply"]["ms"] * 1e-3) / 1e12, 3)
    res["value_share"] = round(float((os_ == engine.VALUE).double().mean()), 4)
    res["combine"] = timed(torch, combine, max(3, reps // 2), warmup=1)
    res["floor_batched_ms"] = round((K + 1) * D * S * 9 / HBM_BPS * 1e3, 3)
    res["batched_TBps"] = round((K + 1) * D * S * 9 / (res["batched"]["ms"] * 1e-3) / 1e12, 3)
    res["floor_per_factor_ms"] = round(K * 8 * D * S * 9 / HBM_BPS * 1e3, 3)
    res["floor_apply_ms"] = round(apply_bytes / HBM_BPS * 1e3, 3)
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="58x2500x5000,58x40x5000")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--one", default=None, help="(child) factors x days x stocks")
    a = ap.parse_args()
    if a.one:
        K, D, S = (int(v) for v in a.one.split("x"))
        return one(K, D, S, a.reps)
    out = {"sizes": []}
    for size in a.sizes.split(","):
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", size, "--reps", str(a.reps)],
                           capture_output=True, text=True, timeout=CHILD_LIMIT_S)
        if r.returncode != 0:  # nothing more is started on the device after a failure
            print(json.dumps(out), flush=True)
            raise SystemExit(f"size {size} failed ({r.returncode}): {r.stderr[-800:]}")
        out["sizes"].append(json.loads(r.stdout.strip().splitlines()[-1]))
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
