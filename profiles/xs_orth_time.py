"""Time of engine.factor_orthogonalize beside a torch formulation of the same definition
(include/mff.h, mff_xs_orth_*).

    python profiles/xs_orth_time.py [--reps 7] [--sizes 58x2500x5000,58x20x5000] [--method symmetric]
Not a test; run by hand on the GPU.  Per size (factors x days x stocks) one child process (its
own time limit; the run stops at the first child that fails) generates seeded exposures
(pairwise correlation 0.25, 0.05 % NULL per row, a few NaN) and times in that one process,
kernels only (device events around the calls after two warm-up calls, median of --reps):
  hip         engine.factor_orthogonalize (mask + sums, f64 MFMA Gram, Jacobi solve, MFMA apply)
  hip_sums / hip_gram / hip_solve / hip_apply   the four C calls alone
  torch       the yardstick: torch mask, means, one f64 bmm, batched torch.linalg.eigh and
              V diag(l^-1/2) V^T (symmetric) or batched eigvalsh + cholesky + triangular solve
              (schmidt: the definition reports the eigenvalues for either method), one f64 bmm
              for the apply, in day batches that fit in memory
and checks once that the torch outputs agree within the tests' rtol = atol = 1e-9.
Floors: HBM = the mask pass reads 9 B per element, the Gram pass 8 B, the apply pass reads 9 B
and writes 9 B, at 8 TB/s; f64 MFMA = the flop of the 16 x 16 x 4 MFMAs the Gram and apply
kernels issue at the rate a bare MFMA loop reaches (profiles/ubench/mfma_f64_rate, see
profiles/xs_reg_time.py; 67.7 TFLOP/s, the rate measured for DESIGN.md §10, when the binary is
not there).  Prints one JSON line.
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


def issued_flop(K, D, S):
    nt = (K + 15) // 16
    per_mfma = 16 * 16 * 4 * 2
    gram = nt * (nt + 1) // 2 * per_mfma * (-(-S // 32) * 8) * D
    apply_ = nt * 2 * (-(-K // 4)) * per_mfma * (-(-S // 32)) * D
    return gram + apply_


def one(K, D, S, method, reps, mfma_tflops):
    import torch

    from mff import _lib, engine
    if not torch.cuda.is_available():
        raise SystemExit("xs_orth_time.py needs a GPU: a CPU run says nothing about kernel time")
    dev = torch.device("cuda:0")
    lib = _lib.load()
    gen = torch.Generator(device=dev)
    gen.manual_seed(20240901)
    f64 = torch.float64
    rnd = lambda: torch.randn((D, S), dtype=f64, device=dev, generator=gen)
    val = torch.empty((K, D, S), dtype=f64, device=dev)
    state = torch.empty((K, D, S), dtype=torch.uint8, device=dev)
    common = rnd()
    for r in range(K):  # row by row: no second panel-sized temporary
        u = torch.rand((D, S), device=dev, generator=gen)
        val[r] = 0.5 * common + 0.866 * rnd()
        val[r][u > 0.9999] = float("nan")
        state[r] = torch.where(u < 0.0005, engine.NULL, engine.VALUE).to(torch.uint8)
    del common
    torch.cuda.synchronize()

    st = engine._stream(dev)
    m = engine.ORTH_METHODS.index(method)
    nsplit = engine.reg_splits(D, S)
    wsp = torch.empty(lib.mff_xs_orth_workspace_bytes(K, D, S), dtype=torch.uint8, device=dev)
    sums = torch.empty((nsplit, D, 2 * K + 1), dtype=f64, device=dev)
    gram = torch.empty((nsplit, D, K, K), dtype=f64, device=dev)
    tr = torch.empty((D, K, K), dtype=f64, device=dev)
    eig, keep = (torch.empty((D, K), dtype=f64, device=dev) for _ in range(2))
    n, status = (torch.empty(D, dtype=torch.int32, device=dev) for _ in range(2))
    ov, os_ = torch.empty_like(val), torch.empty_like(state)

    def hip():
        return engine.factor_orthogonalize(val, state, method=method)

    def hip_sums():
        _lib.check(lib.mff_xs_orth_sums(val.data_ptr(), state.data_ptr(), K, D, S, nsplit, sums.data_ptr(),
                                        wsp.data_ptr(), st), "sums")

    def hip_gram():
        _lib.check(lib.mff_xs_orth_gram(val.data_ptr(), K, D, S, sums.data_ptr(), nsplit, nsplit, gram.data_ptr(),
                                        wsp.data_ptr(), st), "gram")

    def hip_solve():
        _lib.check(lib.mff_xs_orth_solve(gram.data_ptr(), nsplit, K, D, m, 0, tr.data_ptr(), eig.data_ptr(),
                                         keep.data_ptr(), n.data_ptr(), status.data_ptr(), wsp.data_ptr(), st), "solve")

    def hip_apply():
        _lib.check(lib.mff_xs_orth_apply(val.data_ptr(), state.data_ptr(), K, D, S, status.data_ptr(), ov.data_ptr(),
                                         os_.data_ptr(), wsp.data_ptr(), st), "apply")

    nd_b = max(1, min(D, (1 << 30) // (K * S * 8)))  # each derived panel of a batch <= 1 GiB
    out_t = torch.empty((K, D, S), dtype=f64, device=dev)
    lam_t = torch.empty((D, K), dtype=f64, device=dev)
    zero = torch.zeros((), dtype=f64, device=dev)

    def torch_side():
        for d0 in range(0, D, nd_b):
            d1 = min(D, d0 + nd_b)
            v = val[:, d0:d1].permute(1, 0, 2)                                     # [nd][K][S]
            u = ((state[:, d0:d1].permute(1, 0, 2) == engine.VALUE) & torch.isfinite(v)).all(dim=1)
            cnt = u.sum(dim=1).to(f64)
            x0 = torch.where(u[:, None], v, zero)
            c = torch.where(u[:, None], x0 - (x0.sum(dim=2) / cnt[:, None])[:, :, None], zero)
            M = torch.bmm(c, c.transpose(1, 2))
            dg = torch.diagonal(M, dim1=1, dim2=2)
            isd = torch.rsqrt(dg)
            R = M * isd[:, :, None] * isd[:, None, :]
            if method == "symmetric":
                lam, V = torch.linalg.eigh(R)
                lam_t[d0:d1] = lam
                T =torch.bmm(V * torch.rsqrt(lam)[:, None, :], V.transpose(1, 2))
            else:
                lam_t[d0:d1] = torch.linalg.eigvalsh(R)  # the definition's eig / singular rule, either method
                L = torch.linalg.cholesky(R)
                eye = torch.eye(K, dtype=f64, device=dev).expand(d1 - d0, K, K)
                T = torch.linalg.solve_triangular(L, eye, upper=False).transpose(1, 2)
            Tp = T * (isd * torch.sqrt(cnt - 1.0)[:, None])[:, :, None]
            out_t[:, d0:d1] = torch.bmm(Tp.transpose(1, 2), c).permute(1, 0, 2)

    res = {"factors": K, "days": D, "stocks": S, "method": method, "splits": nsplit,
           "device": torch.cuda.get_device_name(0)}
    res["hip"] = timed(torch, hip, reps)
    res["hip_sums"] = timed(torch, hip_sums, reps)
    res["hip_gram"] = timed(torch, hip_gram, reps)
    res["hip_solve"] = timed(torch, hip_solve, reps)
    res["hip_apply"] = timed(torch, hip_apply, reps)
    res["torch"] = timed(torch, torch_side, max(3, reps // 2), warmup=1)
    res["torch_day_batch"] = nd_b
    r = engine.factor_orthogonalize(val, state, method=method)
    torch.cuda.synchronize()
    res["status0_days"] = int((r.status == 0).sum())
    res["eig_min"] = float(r.eig[r.status == 0][:, 0].min())
    ok = (r.state == engine.VALUE) & (r.status == 0)[None, :, None]
    res["torch_vs_hip_max_abs"] = float((r.val - out_t)[ok].abs().max())
    res["torch_within_tolerance"] = bool(torch.allclose(r.val[ok], out_t[ok], rtol=1e-9, atol=1e-9))
    res["torch_vs_hip_eig_max_abs"] = float((r.eig - lam_t).abs().max())
    res["hip_faster_than_torch"] = res["hip"]["ms"] <= res["torch"]["ms"]
    res["floor_hbm_ms"] = round(K * D * S * (9 + 8 + 9 + 9) / HBM_BPS * 1e3, 3)
    res["issued_flop"] = issued_flop(K, D, S)
    res["mfma_tflops_used"] = mfma_tflops
    res["floor_mfma_ms"] = round(res["issued_flop"] / (mfma_tflops * 1e12) * 1e3, 3)
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="58x2500x5000,58x20x5000")
    ap.add_argument("--method", default="symmetric", choices=("symmetric", "schmidt"))
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--one", default=None, help="(child) factors x days x stocks")
    ap.add_argument("--mfma-tflops", type=float, default=MFMA_TFLOPS, help="(child) f64 MFMA rate")
    a = ap.parse_args()
    if a.one:
        K, D, S = (int(v) for v in a.one.split("x"))
        return one(K, D, S, a.method, a.reps, a.mfma_tflops)
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
                            "--method", a.method, "--mfma-tflops", str(tflops)], capture_output=True, text=True,
                           timeout=CHILD_LIMIT_S)
        if r.returncode != 0:  # nothing more is started on the device after a failure
            print(json.dumps(out), flush=True)
            raise SystemExit(f"size {size} failed ({r.returncode}): {r.stderr[-800:]}")
        out["sizes"].append(json.loads(r.stdout.strip().splitlines()[-1]))
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
