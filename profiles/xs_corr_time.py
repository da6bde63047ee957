"""Time of engine.factor_corr + factor_corr_mean beside the same four products in torch.

    python profiles/xs_corr_time.py [--reps 7] [--sizes 58x2500x5000,116x2500x5000,58x20x5000]
Not a test; run by hand on the GPU.  Per size (rows x days x stocks) one child process (its
own time limit; the run stops at the first child that fails) generates seeded heavy-tailed
exposures (2 % NULL, 1 % ABSENT, a few NaN), and times in that one process, kernels only
(device events around the calls after a warm-up, median of --reps):
  hip        engine.factor_corr (centre + the four f64 MFMA sum planes + finalize) and
             engine.factor_corr_mean
  hip_sums   mff_xs_corr_sums alone (centre + planes)
  torch      the yardstick: the same centre, then Y, Y^2, M built with torch.where and the
             four products with torch.bmm in f64, in day batches that fit in memory
and checks once that the torch planes give the same correlations.  Floors: HBM =
rows * D * S * 9 B at 8 TB/s; f64 MFMA = the flop the kernels' MFMAs execute (rows padded to
64 per block, the symmetric halves they skip left out: executed_flop) at the rate a bare
MFMA loop reaches (profiles/ubench/mfma_f64_rate, built with
`hipcc --offload-arch=gfx950 -O3 profiles/ubench/mfma_f64_rate.hip -o profiles/ubench/mfma_f64_rate`;
"unmeasured" when the binary is not there).  Prints one JSON line.
"""
import argparse
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "replication-of-minute-frequency-factor_amd"))

HBM_BPS = 8.0e12
CHILD_LIMIT_S = 420
UBENCH = os.path.join(HERE, "ubench", "mfma_f64_rate")


def timed(torch, fn, reps, warmup=2):
    import numpy as np
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
    return {"ms": round(float(np.median(ms)), 3), "min_ms": round(float(np.min(ms)), 3),
            "max_ms": round(float(np.max(ms)), 3)}


def executed_flop(rows, D, S):
    """flop of the 16 x 16 x 4 MFMAs the kernels issue: per 64-row block pair and 4 stocks, 52
    tiles on a diagonal block (A and Q whole, P and n on or below the diagonal), 64 on a block
    below it, 32 on a block above it."""
    nb = (rows + 63) // 64
    off = nb * (nb - 1) // 2
    tiles = 52 * nb + 64 * off + 32 * off
    return tiles * 16 * 16 * S * D * 2


def one(rows, D, S, reps, mfma_tflops):
    import torch

    from mff import _lib, engine
    if not torch.cuda.is_available():
        raise SystemExit("xs_corr_time.py needs a GPU: a CPU run says nothing about kernel time")
    dev = torch.device("cuda:0")
    lib = _lib.load()
    gen = torch.Generator(device=dev)
    gen.manual_seed(20240601)
    val = torch.empty((rows, D, S), dtype=torch.float64, device=dev)
    state = torch.empty((rows, D, S), dtype=torch.uint8, device=dev)
    common = torch.randn((D, S), dtype=torch.float64, device=dev, generator=gen)
    for r in range(rows):  # row by row: no second panel-sized temporary
        n = torch.randn((D, S), dtype=torch.float64, device=dev, generator=gen)
        w = torch.randn((D, S), dtype=torch.float64, device=dev, generator=gen)
        u = torch.rand((D, S), device=dev, generator=gen)
        val[r] = (n + 0.5 * common) * torch.exp(0.7 * w)  # heavy tails, correlated rows
        val[r][u > 0.999] = float("nan")
        state[r] = torch.where(u < 0.01, engine.ABSENT, torch.where(u < 0.03, engine.NULL, engine.VALUE)).to(torch.uint8)
    del common
    torch.cuda.synchronize()

    ws = torch.empty(max(lib.mff_xs_corr_workspace_bytes(rows, D, S), 8), dtype=torch.uint8, device=dev)
    sums = torch.empty((D, 4, rows, rows), dtype=torch.float64, device=dev)
    st = engine._stream(dev)

    def hip():
        c, _ = engine.factor_corr(val, state)
        return engine.factor_corr_mean(c)

    def hip_sums():
        _lib.check(lib.mff_xs_corr_sums(val.data_ptr(), state.data_ptr(), rows, D, S, None, sums.data_ptr(),
                                        ws.data_ptr(), st), "mff_xs_corr_sums")

    nd_b = max(1, min(D, (2 << 30) // (rows * S * 8)))  # each derived panel of a batch <= 2 GiB
    planes = torch.empty((D, 4, rows, rows), dtype=torch.float64, device=dev)
    zero = torch.zeros((), dtype=torch.float64, device=dev)

    def torch_side():
        for d0 in range(0, D, nd_b):
            v = val[:, d0:d0 + nd_b].permute(1, 0, 2)
            u = (state[:, d0:d0 + nd_b].permute(1, 0, 2) == engine.VALUE) & torch.isfinite(v)
            M = u.to(torch.float64)
            c = torch.where(u, v, zero).sum(-1, keepdim=True) / M.sum(-1, keepdim=True).clamp(min=1.0)
            Y = torch.where(u, v - c, zero)
            Y2 = Y * Y
            MT = M.transpose(1, 2)
            out = planes[d0:d0 + nd_b]
            out[:, 0] = torch.bmm(M, MT)
            out[:, 1] = torch.bmm(Y, MT)
            out[:, 2] = torch.bmm(Y2, MT)
            out[:, 3] = torch.bmm(Y, Y.transpose(1, 2))

    res = {"rows": rows, "days": D, "stocks": S, "device": torch.cuda.get_device_name(0)}
    res["hip"] = timed(torch, hip, reps)
    res["hip_sums"] = timed(torch, hip_sums, reps)
    res["torch"] = timed(torch, torch_side, max(3, reps // 2), warmup=1)
    res["torch_day_batch"] = nd_b
    # the same numbers from both sides: correlations of the torch planes against the HIP ones
    corr_h, n_h = engine.factor_corr(val, state)
    corr_t = torch.empty_like(corr_h)
    n_t = torch.empty_like(n_h)
    _lib.check(lib.mff_xs_corr_finalize(planes.data_ptr(), 1, rows, D, 2, corr_t.data_ptr(), n_t.data_ptr(), st),
               "mff_xs_corr_finalize")
    torch.cuda.synchronize()
    ok = torch.isfinite(corr_h) & torch.isfinite(corr_t)
    res["torch_vs_hip_max_abs"] = float((corr_h - corr_t)[ok].abs().max())
    res["torch_vs_hip_n_equal"] = bool(torch.equal(n_h, n_t)) and bool(
        torch.equal(torch.isnan(corr_h), torch.isnan(corr_t)))
    res["hip_no_slower_than_torch"] = res["hip"]["ms"] <= res["torch"]["ms"]
    hbm_ms = rows * D * S * 9 / HBM_BPS * 1e3
    res["floor_hbm_ms"] = round(hbm_ms, 3)
    res["hip_fraction_of_hbm_floor"] = round(hbm_ms / res["hip"]["ms"], 3)
    res["executed_flop"] = executed_flop(rows, D, S)
    if mfma_tflops > 0:
        mfma_ms = res["executed_flop"] / (mfma_tflops * 1e12) * 1e3
        res["floor_mfma_ms"] = round(mfma_ms, 3)
        res["hip_fraction_of_mfma_floor"] = round(mfma_ms / res["hip"]["ms"], 3)
        res["hip_sums_fraction_of_mfma_floor"] = round(mfma_ms / res["hip_sums"]["ms"], 3)
        res["binding_floor"] = "f64 MFMA" if mfma_ms >= hbm_ms else "HBM"
    else:
        res["floor_mfma_ms"] = "unmeasured"
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="58x2500x5000,116x2500x5000,58x20x5000")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--one", default=None, help="(child) rows x days x stocks")
    ap.add_argument("--mfma-tflops", type=float, default=0.0, help="(child) measured f64 MFMA rate")
    a = ap.parse_args()
    if a.one:
        rows, D, S = (int(v) for v in a.one.split("x"))
        return one(rows, D, S, a.reps, a.mfma_tflops)
    out = {"mfma_f64": "unmeasured", "sizes": []}
    tflops = 0.0
    if os.path.exists(UBENCH):  # the bare MFMA loop, in a process and under a time limit of its own
        r = subprocess.run([UBENCH], capture_output=True, text=True, timeout=120)
        if r.returncode != 0:
            raise SystemExit(f"{UBENCH} failed ({r.returncode}): {r.stderr[-400:]}")
        out["mfma_f64"] = json.loads(r.stdout.strip().splitlines()[-1])
        tflops = max(out["mfma_f64"][k]["TFLOPs"] for k in ("waves_per_simd_1", "waves_per_simd_2"))
    for size in a.sizes.split(","):
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", size, "--reps", str(a.reps),
                            "--mfma-tflops", str(tflops)], capture_output=True, text=True, timeout=CHILD_LIMIT_S)
        if r.returncode != 0:  # nothing more is started on the device after a failure
            print(json.dumps(out), flush=True)
            raise SystemExit(f"size {size} failed ({r.returncode}): {r.stderr[-800:]}")
        out["sizes"].append(json.loads(r.stdout.strip().splitlines()[-1]))
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
