"""bench.py's command line: the plain run, --full and --dump-outputs.

The plain run prints the headline line and nothing that takes a run of its own;
--dump-outputs writes the last timed step's outputs (a fixed sample where they exceed the
budget) so that two builds can be compared output for output."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")
FILES = ("val", "nonfinite", "state", "factor_ids", "sample_day", "sample_stock")


def expected(v, s):
    """val.npy and nonfinite.npy of the pass output (v, s) at the dumped positions."""
    v = np.where(s == 2, v, 0.0)
    kind = np.where(np.isnan(v), 1, np.where(np.isposinf(v), 2, np.where(np.isneginf(v), 3, 0)))
    return np.where(kind == 0, v, 0.0), kind.astype(np.float32)


def test_measurements_beyond_the_steps_need_full():
    for flag in ("--kernel-times", "--null-only"):
        r = subprocess.run([sys.executable, BENCH, "--no-extras", flag], capture_output=True, text=True)
        assert r.returncode == 2 and "--full" in r.stderr, (flag, r.returncode, r.stderr)


def test_dump_holds_finite_numbers_only(tmp_path):
    """NaN and +-inf are values the pass may return: val.npy holds 0.0 there (as it does
    where state is not VALUE) and nonfinite.npy says which; host tensors, no GPU."""
    import torch
    import bench

    nan, inf = float("nan"), float("inf")
    v = np.array([[[1.5, nan, inf], [-inf, -2.0, nan]],
                  [[nan, 0.0, -inf], [inf, 3.0, 4.0]]])  # [2 factors][2 days][3 stocks]
    s = np.array([[[2, 2, 2], [2, 2, 1]],
                  [[0, 2, 2], [1, 2, 2]]], dtype=np.uint8)
    bench.dump_outputs(str(tmp_path), (torch.from_numpy(v), torch.from_numpy(s), [3, 9]), 0, 0, 1)
    got = {f: np.load(tmp_path / (f + ".npy")) for f in FILES}
    assert all(np.isfinite(a).all() for a in got.values())
    assert np.array_equal(got["val"], [[1.5, 0, 0, 0, -2.0, 0], [0, 0.0, 0, 0, 3.0, 4.0]])
    assert np.array_equal(got["nonfinite"], [[0, 1, 2, 3, 0, 0], [0, 0, 3, 0, 0, 0]])
    assert np.array_equal(got["state"], s.reshape(2, 6)) and got["state"].dtype == np.float32
    assert np.array_equal(got["factor_ids"], [3, 9])
    assert np.array_equal(got["sample_day"], [0, 0, 0, 1, 1, 1])
    assert np.array_equal(got["sample_stock"], [0, 1, 2, 0, 1, 2])


@pytest.mark.gpu
def test_plain_run_line_and_dump(tmp_path):
    import torch
    from mff import engine, synth

    S, D = 96, 6
    out = tmp_path / "dump"
    r = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--steps", "2", "--warmup", "1",
                        "--stocks", str(S), "--days", str(D), "--dump-outputs", str(out)],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    res = json.loads(lines[0])
    assert res["steps"] == 2 and res["warmup"] == 1 and res["ms_per_step"] > 0
    assert res["unit"] == "stock-days/s" and res["higher_is_better"] is True and res["dtype"] == "f64"
    assert res["value"] == pytest.approx(S * D / (res["ms_per_step"] * 1e-3))
    # nothing beyond the timed steps
    assert res["cpu_baseline"] is None and res["extras"] == {} and res["roofline"]["kernels"] is None
    assert sorted(os.listdir(out)) == sorted(f + ".npy" for f in FILES)
    got = {f: np.load(out / (f + ".npy")) for f in FILES}
    assert all(a.dtype in (np.float32, np.float64) and np.isfinite(a).all() for a in got.values())
    # the same seeded panel in this process: the dump is the pass's output, bit for bit
    dev = torch.device("cuda:0")
    bars, mask = synth.make_panel_device(S, D, dev, config=4, seed_offset=0)
    val, state, ids = engine.compute_factors(engine.DevicePanel(bars, mask, stocks_total=S))
    torch.cuda.synchronize()
    v, s = val.cpu().numpy().reshape(58, -1), state.cpu().numpy().reshape(58, -1)
    assert got["val"].shape == got["state"].shape == (58, S * D)  # small enough: no sampling
    assert np.array_equal(got["state"], s.astype(np.float32))
    assert (s == 2).any()
    ev, ek = expected(v, s)
    assert np.array_equal(got["val"], ev) and np.array_equal(got["nonfinite"], ek)
    assert np.array_equal(got["factor_ids"], np.asarray(ids, dtype=np.float64))
    assert np.array_equal(got["sample_day"] * S + got["sample_stock"], np.arange(S * D))


@pytest.mark.gpu
def test_dump_sample_is_fixed_and_within_budget(tmp_path, monkeypatch):
    import torch
    import bench
    from mff import engine, synth

    S, D = 40, 5
    dev = torch.device("cuda:0")
    bars, mask = synth.make_panel_device(S, D, dev, config=4, seed_offset=0)
    out = engine.compute_factors(engine.DevicePanel(bars, mask, stocks_total=S))
    torch.cuda.synchronize()
    assert bench.DUMP_BUDGET_BYTES <= 64_000_000
    budget = 50 * (58 * 16 + 16) + 58 * 8  # 50 of the 200 stock-days and the factor ids
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", budget)
    s0 = 7  # a shard that starts at stock 7 of the whole panel
    bench.dump_outputs(str(tmp_path / "a"), out, s0, 0, 1)
    bench.dump_outputs(str(tmp_path / "b"), out, s0, 0, 1)
    a = {f: np.load(tmp_path / "a" / (f + ".npy")) for f in FILES}
    b = {f: np.load(tmp_path / "b" / (f + ".npy")) for f in FILES}
    assert all(np.array_equal(a[f], b[f]) and np.isfinite(a[f]).all() for f in FILES)
    assert sum(x.nbytes for x in a.values()) == budget  # everything written counts
    day, stock = a["sample_day"].astype(int), a["sample_stock"].astype(int) - s0
    assert day.shape == (50,) and len(set(zip(day, stock))) == 50
    assert (0 <= day).all() and (day < D).all() and (0 <= stock).all() and (stock < S).all()
    v, s = out[0].cpu().numpy()[:, day, stock], out[1].cpu().numpy()[:, day, stock]
    assert np.array_equal(a["state"], s.astype(np.float32))
    ev, ek = expected(v, s)
    assert np.array_equal(a["val"], ev) and np.array_equal(a["nonfinite"], ek)
