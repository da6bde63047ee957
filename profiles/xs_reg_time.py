"""Time of engine.factor_regress + factor_regress_mean beside a torch formulation of the same
definition (include/mff.h, mff_xs_reg_*).

    python profiles/xs_reg_time.py [--reps 7] [--sizes 58x2500x5000,58x20x5000] [--groups 31]
Not a test; run by hand on the GPU.  Per size (factors x days x stocks) one child process (its
own time limit; the run stops at the first child that fails) generates seeded exposures
(pairwise correlation 0.25, 0.05 % NULL per row, a few NaN), a regressand, 31 industries and
sqrt-cap weights, and times in that one process, kernels only (device events around the calls
after two warm-up calls, median of --reps):
  hip         engine.factor_regress (mask + group sums, means + f64 MFMA Gram, Cholesky solve)
              and engine.factor_regress_mean
  hip_groups / hip_gram / hip_solve   the three C calls alone
  torch       the yardstick: torch.where mask, index_add_ group means, one f64 bmm, batched
              torch.linalg.cholesky / cholesky_solve, in day batches that fit in memory
and checks once that the torch coefficients agree within the tests' rtol = atol = 1e-9.
Floors: HBM = two passes over the 9 B / element panel plus the side inputs (y 9 B, weight 9 B,
industry 4 B per stock-day) at 8 TB/s; f64 MFMA = the flop of the 16 x 16 x 4 MFMAs the Gram
kernel issues (the tiles on or below the block diagonal of the K + 1 columns padded to 16,
stocks padded to 32) at the rate a bare MFMA loop reaches (profiles/ubench/mfma_f64_rate, built
with `hipcc --offload-arch=gfx950 -O3 profiles/ubench/mfma_f64_rate.hip -o
profiles/ubench/mfma_f64_rate`; 67.7 TFLOP/s, the rate measured for DESIGN.md §10, when the
binary is not there).  Prints one JSON line.
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
MFMA_TFLOPS = 67.7
CHILD_LIMIT_S = 420
UBENCH = os.path.join(HERE, "ubench", "mfma_f64_rate")


def issued_flop(K, D, S, nsplit=1):
    nt = (K + 1 + 15) // 16
    tiles = nt * (nt + 1) // 2
    return tiles * 16 * 16 * 4 * 2 * (-(-S // 32) * 8) * D


def one(K, D, S, G, reps, mfma_tflops):
    import torch

    from mff import _lib, engine
    if not torch.cuda.is_available():
        raise SystemExit("xs_reg_time.py needs a GPU: a CPU run says nothing about kernel time")
    dev = torch.device("cuda:0")
    lib = _lib.load()
    gen = torch.Generator(device=dev)
    gen.manual_seed(20240901)
    f64 = torch.float64
    rnd = lambda: torch.randn((D, S), dtype=f64, device=dev, generator=gen)
    val = torch.empty((K, D, S), dtype=f64, device=dev)
    state = torch.empty((K, D, S), dtype=torch.uint8, device=dev)
    common = rnd()
    y = 0.5 * rnd()
    for r in range(K):  # row by row: no second panel-sized temporary
        u = torch.rand((D, S), device=dev, generator=gen)
        val[r] = 0.5 * common + 0.866 * rnd()
        y += val[r] * (0.1 * ((r % 7) - 3))
        val[r][u > 0.9999] = float("nan")
        state[r] = torch.where(u < 0.0005, engine.NULL, engine.VALUE).to(torch.uint8)
    del common
    ys = torch.full((D, S), engine.VALUE, dtype=torch.uint8, device=dev)
    w = torch.sqrt(torch.exp(3.0 + rnd()))
    ws = torch.full((D, S), engine.VALUE, dtype=torch.uint8, device=dev)
    grp = torch.randint(0, G, (D, S), device=dev, generator=gen).to(torch.int32)
    torch.cuda.synchronize()

    C = K + 1
    st = engine._stream(dev)
    nsplit = engine.reg_splits(D, S)
    wsp = torch.empty(lib.mff_xs_reg_workspace_bytes(K, D, S, G), dtype=torch.uint8, device=dev)
    gsums = torch.empty((nsplit, D, G + 1, K + 3), dtype=f64, device=dev)
    gram = torch.empty((nsplit, D, C, C), dtype=f64, device=dev)
    outs = [torch.empty((D, K), dtype=f64, device=dev) for _ in range(2)] + [torch.empty(D, dtype=f64, device=dev)] + \
        [torch.empty(D, dtype=torch.int32, device=dev) for _ in range(3)]

    def hip():
        return engine.factor_regress_mean(engine.factor_regress(val, state, y, ys, w, ws, grp, G=G))

    def hip_groups():
        _lib.check(lib.mff_xs_reg_groups(val.data_ptr(), state.data_ptr(), K, D, S, y.data_ptr(), ys.data_ptr(),
                                         w.data_ptr(), ws.data_ptr(), grp.data_ptr(), G, nsplit, gsums.data_ptr(),
                                         wsp.data_ptr(), st), "groups")

    def hip_gram():
        _lib.check(lib.mff_xs_reg_gram(val.data_ptr(), K, D, S, y.data_ptr(), w.data_ptr(), G, gsums.data_ptr(), nsplit,
                                       nsplit, gram.data_ptr(), wsp.data_ptr(), st), "gram")

    def hip_solve():
        _lib.check(lib.mff_xs_reg_solve(gram.data_ptr(), nsplit, K, D, 0, *[o.data_ptr() for o in outs],
                                        wsp.data_ptr(), st), "solve")

    nd_b = max(1, min(D, (1 << 30) // (C * S * 8)))  # each derived panel of a batch <= 1 GiB
    beta_t = torch.empty((D, K), dtype=f64, device=dev)
    zero = torch.zeros((), dtype=f64, device=dev)

    def torch_side():
        for d0 in range(0, D, nd_b):
            d1 = min(D, d0 + nd_b)
            nd = d1 - d0
            v = val[:, d0:d1].permute(1, 0, 2)
            wb, gb = w[d0:d1], grp[d0:d1].to(torch.int64)
            u = ((state[:, d0:d1].permute(1, 0, 2) == engine.VALUE) & torch.isfinite(v)).all(dim=1)
            u &= (ys[d0:d1] == engine.VALUE) & torch.isfinite(y[d0:d1])
            u &= (ws[d0:d1] == engine.VALUE) & torch.isfinite(wb) & (wb > 0) & (gb >= 0) & (gb < G)
            c = torch.where(u[:, None], torch.cat([v, y[d0:d1, None]], dim=1), zero)      # [nd][C][S]
            wu = torch.where(u, wb, zero)
            idx = (torch.arange(nd, device=dev)[:, None] * G + gb.clamp(0, G - 1)).reshape(-1)
            sums = torch.zeros((nd * G, C), dtype=f64, device=dev)
            sums.index_add_(0, idx, (c * wu[:, None]).permute(0, 2, 1).reshape(-1, C))
            W = torch.zeros(nd * G, dtype=f64, device=dev).index_add_(0, idx, wu.reshape(-1))
            mean = sums / W.clamp(min=1e-300)[:, None]
            ct = torch.where(u[:, None], c - mean[idx].reshape(nd, S, C).permute(0, 2, 1), zero)
            gr = torch.bmm(ct * wu[:, None], ct.transpose(1, 2))
            M, b = gr[:, :K, :K], gr[:, :K, K]
            sc = torch.rsqrt(torch.diagonal(M, dim1=1, dim2=2))
            L = torch.linalg.cholesky(M * sc[:, :, None] * sc[:, None, :])
            beta_t[d0:d1] = torch.cholesky_solve((b * sc)[:, :, None], L)[:, :, 0] * sc

    res = {"factors": K, "days": D, "stocks": S, "industries": G, "splits": nsplit,
           "device": torch.cuda.get_device_name(0)}
    res["hip"] = timed(torch, hip, reps)
    res["hip_groups"] = timed(torch, hip_groups, reps)
    res["hip_gram"] = timed(torch, hip_gram, reps)
    res["hip_solve"] = timed(torch, hip_solve, reps)
    res["torch"] = timed(torch, torch_side, max(3, reps // 2), warmup=1)
    res["torch_day_batch"] = nd_b
    r = engine.factor_regress(val, state, y, ys, w, ws, grp, G=G)
    torch.cuda.synchronize()
    res["status0_days"] = int((r.status == 0).sum())
    ok = (r.status == 0)[:, None].expand_as(r.beta)
    res["torch_vs_hip_beta_max_abs"] = float((r.beta - beta_t)[ok].abs().max())
    res["torch_beta_within_tolerance"] = bool(torch.allclose(r.beta[ok], beta_t[ok], rtol=1e-9, atol=1e-9))
    res["hip_faster_than_torch"] = res["hip"]["ms"] <= res["torch"]["ms"]
    hbm_ms = (2 * K * D * S * 9 + 2 * D * S * (9 + 9 + 4)) / HBM_BPS * 1e3
    res["floor_hbm_ms"] = round(hbm_ms, 3)
    res["issued_flop"] = issued_flop(K, D, S)
    res["mfma_tflops_used"] = mfma_tflops
    res["floor_mfma_ms"] = round(res["issued_flop"] / (mfma_tflops * 1e12) * 1e3, 3)
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="58x2500x5000,58x20x5000")
    ap.add_argument("--groups", type=int, default=31)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--one", default=None, help="(child) factors x days x stocks")
    ap.add_argument("--mfma-tflops", type=float, default=MFMA_TFLOPS, help="(child) f64 MFMA rate")
    a = ap.parse_args()
    if a.one:
        K, D, S = (int(v) for v in a.one.split("x"))
        return one(K, D, S, a.groups, a.reps, a.mfma_tflops)
    out = {"mfma_f64": f"unmeasured here: {MFMA_TFLOPS} TFLOP/s assumed", "sizes": []}
    tflops = MFMA_TFLOPS
    if os.path.exists(UBENCH):  # the bare MFMA loop, in a process and under a time limit of its own
        r = subprocess.run([UBENCH], capture_output=True, text=True, timeout=120)
        if r.returncode != 0:
            raise SystemExit(f"{UBENCH} failed ({r.returncode}): {r.stderr[-400:]}")
        out["mfma_f64"] = json.loads(r.stdout.strip().splitlines()[-1])
        tflops = max(out["mfma_f64"][k]["TFLOPs"] for k in ("waves_per_simd_1", "waves_per_simd_2"))
    for size in a.sizes.split(","):
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", size, "--reps", str(a.reps),
                            "--groups", str(a.groups), "--mfma-tflops", str(tflops)], capture_output=True, text=True,
                           timeout=CHILD_LIMIT_S)
        if r.returncode != 0:  # nothing more is started on the device after a failure
            print(json.dumps(out), flush=True)
            raise SystemExit(f"size {size} failed ({r.returncode}): {r.stderr[-800:]}")
        out["sizes"].append(json.loads(r.stdout.strip().splitlines()[-1]))
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
