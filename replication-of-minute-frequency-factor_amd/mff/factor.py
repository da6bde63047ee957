"""`Factor` and `MinFreqFactor`: the reference's user surface (Factor.py,
MinuteFrequentFactorCICC.py) over the HIP engine.

Kept: constructor arguments, attribute names (factor_name, factor_exposure, IC, ICIR,
rank_IC, rank_ICIR), method names and arguments, output column names, error messages
and the incremental-update / atomic-persistence behaviour.  Changed: frames are pandas
(pyarrow-backed float columns keep polars' null vs NaN) because polars is not part of
this stack; the hard-coded Windows data paths (FA:49,70; MF:64,68) are defaults that
environment variables (MFF_PV_PATH, MFF_EXPOSURE_DIR, MFF_KLINE_DIR) or arguments
override.

Device work:
  cal_exposure_by_min_data(cal_xxx)  -> ingest + stage-1 kernels over day-file batches
  cal_final_exposure(N, m, 'days')   -> stage-2 rolling kernel
  cal_final_exposure(f, m, 'calendar') -> calendar resampling kernel
  ic_test                            -> future-return, IC pair / rank / moment kernels
  group_test                         -> qcut / period / reduce kernels
  portfolio_test / portfolio_tests   -> qcut + daily portfolio kernels (mff_pf_*)
coverage is a host group-by count.
"""
from __future__ import annotations

import os
import tempfile
import warnings
from typing import Literal, Optional

import numpy as np

from . import _timing, catalog, frames

_PV_PATH = os.environ.get("MFF_PV_PATH", r"D:\QuantData\Price_Volume.parquet")
_EXPOSURE_DIR = os.environ.get("MFF_EXPOSURE_DIR", r"D:\QuantData\MinuteFreqFactor")
_KLINE_DIR = os.environ.get("MFF_KLINE_DIR", r"D:\QuantData\KLine_cleaned")


def _pd():
    import pandas as pd
    return pd


def _plt():
    try:
        import matplotlib.pyplot as plt
        return plt
    except ImportError:
        warnings.warn("matplotlib is not installed; plot_out ignored")
        return None


def _float_values(col):
    """(values f64 with NaN for null, isnull mask)."""
    pd = _pd()
    if isinstance(col.dtype, pd.ArrowDtype):
        arr = col.array._pa_array.combine_chunks()
        isnull = np.asarray(arr.is_null().to_numpy(zero_copy_only=False), dtype=bool)
        x = np.asarray(arr.fill_null(np.nan).to_numpy(zero_copy_only=False), dtype=np.float64)
        return x, isnull
    x = np.asarray(col.to_numpy(dtype=np.float64, na_value=np.nan))
    return x, np.asarray(col.isna().to_numpy())


class Factor:
    """Factor.py:7-350."""

    COLUMN_DICT = {  # CSMAR daily price-volume columns (Factor.py:32-47)
        "Trddt": "date", "Stkcd": "code", "Opnprc": "open", "Hiprc": "high", "Loprc": "low",
        "Clsprc": "close", "Dnshrtrd": "volume", "Dnvaltrd": "amount", "ChangeRatio": "pct_change",
        "Dsmvosd": "cmc", "Dsmvtll": "tmc", "Adjprcwd": "close_adjust", "LimitDown": "limit_down",
        "LimitUp": "limit_up",
    }

    def __init__(self, factor_name: str, factor_exposure=None):
        self.factor_name = factor_name
        self.factor_exposure = factor_exposure
        self.IC = None
        self.ICIR = None
        self.rank_IC = None
        self.rank_ICIR = None

    # ------------------------------------------------------------------ IO
    @staticmethod
    def _read_daily_pv_data(column_need=None, path: Optional[str] = None):
        """Factor.py:21-62: CSMAR daily PV parquet, columns renamed, Trddt parsed."""
        import pyarrow.parquet as pq

        pd = _pd()
        df = pq.read_table(path or _PV_PATH).to_pandas()
        df = df.rename(columns=Factor.COLUMN_DICT)
        df["date"] = pd.to_datetime(df["date"], format="%Y-%m-%d").dt.date
        if column_need is None:
            column_need = list(Factor.COLUMN_DICT.values())
        return df[[c for c in column_need if c in df.columns]]

    def to_parquet(self, path: str = None):
        """Factor.py:64-90: write through a temp file in the target dir, then rename."""
        import pyarrow as pa
        import pyarrow.parquet as pq

        if path is None:
            path = _EXPOSURE_DIR
        if not path.endswith(".parquet"):
            path = os.path.join(path, f"{self.factor_name}.parquet")
        temp_dir = os.path.dirname(path) or "."
        with tempfile.NamedTemporaryFile(dir=temp_dir, delete=False, suffix=".parquet") as tmp:
            temp_path = tmp.name
        try:
            pq.write_table(pa.Table.from_pandas(self.factor_exposure, preserve_index=False), temp_path)
            os.replace(temp_path, path)
        except Exception:
            if os.path.exists(temp_path):
                os.remove(temp_path)
            raise

    # ------------------------------------------------------------------ evaluation
    def _valid_exposure(self):
        """filter(~is_nan()) (FA:100-101, 167-168): drops NaN and null rows."""
        df = self.factor_exposure
        x, isnull = _float_values(df[self.factor_name])
        keep = ~isnull & ~np.isnan(x)
        out = df.loc[keep, ["code", "date"]].copy()
        out[self.factor_name] = x[keep]
        return out

    def coverage(self, plot_out=True, return_df=False):
        """Factor.py:92-125: per-date count of non-NaN exposures."""
        v = self._valid_exposure()
        cov = v.groupby("date")[self.factor_name].count().sort_index().reset_index()
        if plot_out:
            plt = _plt()
            if plt is not None:
                plt.figure(figsize=(12, 8))
                plt.bar(cov["date"], cov[self.factor_name], color="tab:blue", alpha=0.6,
                        label=f"{self.factor_name} coverage")
                plt.xticks(rotation=45)
                plt.grid(True, linestyle="--", alpha=0.7)
                plt.legend(loc="best")
                plt.title("coverage plot")
                plt.tight_layout()
                plt.show()
        return cov if return_df else None

    def ic_test(self, future_days: int = 5, plot_out: bool = True, plot_variable: str = "IC",
                return_df: bool = False, pv_data=None, device=None):
        """Factor.py:127-229 on the GPU: future N-day compounded return per code
        (mff_future_return, FA:142-162), per-date Pearson IC and Spearman rank IC of the
        non-null, non-NaN exposure against it (mff_ic_pairs / mff_xs_rank / mff_ic_moments,
        FA:163-183), dates with a NaN IC dropped (FA:184-186); IC, rank_IC, ICIR, rank_ICIR."""
        import torch

        from . import engine
        from .factors import _device

        pd = _pd()
        pv = pv_data if pv_data is not None else self._read_daily_pv_data(["code", "date", "pct_change"])
        ex = self.factor_exposure
        codes, dates = frames.universe(ex, pv)
        dev = _device(device)
        xv, xs, _, _ = frames.from_long(ex, self.factor_name, codes=codes, dates=dates)
        pv_v, pv_s, _, _ = frames.from_long(pv, "pct_change", codes=codes, dates=dates)
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        fv, fs = engine.future_return(t(pv_v), t(pv_s), future_days)
        ic, ric = engine.ic_series(t(xv), t(xs), fv, fs)
        ic, ric = ic.cpu().numpy(), ric.cpu().numpy()
        keep = ~np.isnan(ic)
        ic_df = pd.DataFrame({"date": np.asarray(dates, dtype=object)[keep], "IC": ic[keep],
                              "rank_IC": ric[keep]}).reset_index(drop=True)
        self.IC = float(ic_df["IC"].mean())
        self.rank_IC = float(ic_df["rank_IC"].mean())
        self.ICIR = self.IC / float(ic_df["IC"].std())
        self.rank_ICIR = self.rank_IC / float(ic_df["rank_IC"].std())
        if plot_out:
            plt = _plt()
            if plt is not None:
                fig, ax1 = plt.subplots(figsize=(12, 6))
                ax1.bar(ic_df["date"], ic_df[plot_variable], color="tab:blue", alpha=0.6, width=1.0)
                ax2 = ax1.twinx()
                ax2.plot(ic_df["date"], ic_df[plot_variable].cumsum(), color="tab:red",
                         linewidth=2.0, label=f"cum {plot_variable}")
                plt.title(f"{plot_variable} plot")
                plt.tight_layout()
                plt.show()
        return ic_df if return_df else None

    def group_test(self, frequency: Literal["weekly", "monthly", "quarterly", "yearly"] = "monthly",
                   weight_param: Literal["tmc", "cmc", None] = None, group_num: int = 5,
                   plot_out: bool = True, return_df: bool = False, pv_data=None, device=None):
        """Factor.py:231-350 on the GPU: per-date quantile groups (mff_bt_qcut), per
        rebalancing period compounding with the previous period's group / weight
        (mff_bt_periods), per (period, group) equal or tmc/cmc-weighted mean return
        (mff_bt_reduce / mff_bt_finalize).  Rows: [date (period right edge), group,
        pct_change] sorted by (date, group)."""
        import torch

        from . import engine
        from .factors import _device

        pd = _pd()
        if weight_param not in (None, "tmc", "cmc"):
            raise ValueError(f"weight_param must be 'tmc', 'cmc' or None, got {weight_param!r}")
        pv = pv_data if pv_data is not None else self._read_daily_pv_data(
            ["code", "date", "pct_change", "tmc", "cmc"])
        ex = self.factor_exposure
        codes, dates = frames.universe(ex)
        pv = pv[frames.rows_in(pv, codes, dates)]
        period_of, labels = rebalance_periods(dates, frequency)
        dev = _device(device)
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        xv, xs, _, _ = frames.from_long(ex, self.factor_name, codes=codes, dates=dates)
        pc_v, pc_s, _, _ = frames.from_long(pv, "pct_change", codes=codes, dates=dates)
        wv = ws = None
        if weight_param is not None:
            w_v, w_s, _, _ = frames.from_long(pv, weight_param, codes=codes, dates=dates)
            wv, ws = t(w_v), t(w_s)
        ret, present = engine.group_returns(t(xv), t(xs), t(pc_v), t(pc_s),
                                            t(period_of.astype(np.int32)), len(labels), group_num,
                                            wv, ws)
        ret, present = ret.cpu().numpy(), present.cpu().numpy().astype(bool)
        p_idx, g_idx = np.nonzero(present)
        group_df = pd.DataFrame({"date": np.asarray(labels, dtype=object)[p_idx],
                                 "group": [f"group_{g + 1}" for g in g_idx],
                                 "pct_change": ret[p_idx, g_idx]})
        group_df = group_df.sort_values(["date", "group"]).reset_index(drop=True)
        if plot_out:
            plt = _plt()
            if plt is not None:
                plt.figure(figsize=(12, 8))
                for grp, g in group_df.groupby("group"):
                    plt.plot(g["date"], (g["pct_change"] + 1).cumprod(), label=grp, linewidth=2)
                plt.legend(loc="best")
                plt.title("group return", fontsize=16)
                plt.tight_layout()
                plt.show()
        return group_df if return_df else None

    def portfolio_test(self, frequency: Literal["weekly", "monthly", "quarterly", "yearly"] = "monthly",
                       weight_param: Literal["tmc", "cmc", None] = None, group_num: int = 5, cost: float = 0.0,
                       annual_days: int = 252, return_daily: bool = False, pv_data=None, device=None,
                       plot_out: bool = True, return_df: bool = False):
        """:func:`portfolio_tests` of this factor alone (arguments as there): the daily NAV of
        the group_test portfolios and of group_G minus group_1, turnover and summary statistics
        net of ``cost``.  The frames come without the ``factor`` column; ``plot_out`` draws the
        NAV curves.  Returns None unless ``return_df``."""
        out = portfolio_tests([self], frequency=frequency, weight_param=weight_param, group_num=group_num,
                              cost=cost, annual_days=annual_days, return_daily=return_daily or plot_out,
                              pv_data=pv_data, device=device)
        summary, daily, periods = out if isinstance(out, tuple) else (out, None, None)
        if plot_out:
            plt = _plt()
            if plt is not None:
                plt.figure(figsize=(12, 8))
                for pn, g in daily.groupby("portfolio", sort=False):
                    plt.plot(g["date"], g["nav"], label=pn, linewidth=2)
                plt.legend(loc="best")
                plt.title("portfolio NAV", fontsize=16)
                plt.tight_layout()
                plt.show()
        if not return_df:
            return None
        summary = summary.drop(columns="factor")
        if not return_daily:
            return summary
        return summary, daily.drop(columns="factor"), periods.drop(columns="factor")

    def neutralize(self, industry=None, size: Literal["cmc", "tmc", None] = "cmc", winsor: float = 3.0,
                   standardize: bool = True, pv_data=None, device=None) -> "Factor":
        """Per-date preprocessing ahead of ic_test / group_test, on the GPU
        (mff_xs_neutralize, include/mff.h): MAD winsorisation (``winsor`` x 1.4826 x MAD
        around the median; <= 0: off), OLS residual on industry dummies and ln(market cap),
        z-score (ddof=1).  No reference counterpart: Factor.py tests raw exposures.

        ``industry``: None, or a long frame [code, industry] (one label per code) or
        [code, date, industry]; labels of any hashable dtype, a null label = no industry.
        ``size``: 'cmc', 'tmc' or None, read from ``pv_data`` (default: the daily
        price-volume file); a null, non-finite or <= 0 cap is a missing covariate.
        A stock-day with a finite exposure but no industry or no covariate comes out null.

        Returns a new object of the same class named ``f"{factor_name}_neu"`` whose
        factor_exposure holds [code, date, <that name>]; this object is left untouched."""
        import torch

        from . import engine
        from .factors import _device

        pd = _pd()
        if size not in (None, "tmc", "cmc"):
            raise ValueError(f"size must be 'tmc', 'cmc' or None, got {size!r}")
        if isinstance(winsor, bool) or not isinstance(winsor, (int, float)) or np.isnan(winsor):
            raise ValueError(f"winsor must be a number (<= 0: no winsorisation), got {winsor!r}")
        ex = self.factor_exposure
        codes, dates = frames.universe(ex)
        D, S = len(dates), len(codes)
        grp, G = _industry_ids(industry, codes, dates)
        dev = _device(device)
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        zv = zs = None
        if size is not None:
            pv = pv_data if pv_data is not None else self._read_daily_pv_data(["code", "date", size])
            if size not in pv.columns:
                raise ValueError(f"pv_data has no column {size!r}")
            pv = pv[frames.rows_in(pv, codes, dates)]
            c_v, c_s, _, _ = frames.from_long(pv, size, codes=codes, dates=dates)
            cap, cst = t(c_v), t(c_s)
            ok = (cst == engine.VALUE) & torch.isfinite(cap) & (cap > 0)
            zv = torch.where(ok, torch.log(torch.where(ok, cap, torch.ones_like(cap))), torch.zeros_like(cap))
            zs = torch.where(ok, cst, torch.where(cst == engine.ABSENT, cst, torch.full_like(cst, engine.NULL)))
        xv, xs, _, _ = frames.from_long(ex, self.factor_name, codes=codes, dates=dates)
        ov, os_ = engine.neutralize(t(xv[None]), t(xs[None]), None if grp is None else t(grp), zv, zs, G=G,
                                    winsor=float(winsor), standardize=bool(standardize))
        torch.cuda.synchronize(dev)
        name = f"{self.factor_name}_neu"
        return type(self)(name, frames.to_long(ov[0].cpu().numpy(), os_[0].cpu().numpy(), codes, dates, name))

    def corr_with(self, others, **kw):
        """The row of this factor in :func:`factor_correlation` of ``[self, *others]``
        (``others``: a Factor, a sequence of them or a mapping name -> Factor; keywords
        as there): a pandas Series indexed by the others' names -- with
        ``return_daily=True`` also the daily long frame restricted to this factor's pairs."""
        if isinstance(others, Factor):
            others = [others]
        if isinstance(others, dict):
            if self.factor_name in others:
                raise ValueError(f"duplicate factor name {self.factor_name!r}")
            group = {self.factor_name: self, **others}
        else:
            group = [self] + list(others)
        out = factor_correlation(group, **kw)
        mean, daily = out if isinstance(out, tuple) else (out, None)
        row = mean.loc[self.factor_name].drop(self.factor_name)
        if daily is None:
            return row
        mine = (daily["factor_a"] == self.factor_name) | (daily["factor_b"] == self.factor_name)
        return row, daily[mine].reset_index(drop=True)

    def return_with(self, others, **kw):
        """The row of this factor in :func:`factor_returns` of ``[self, *others]`` (``others``:
        a Factor, a sequence of them or a mapping name -> Factor; keywords as there): a pandas
        Series of the aggregate columns -- with ``return_daily`` / ``return_residual`` the
        extras follow, the daily long frame restricted to this factor."""
        if isinstance(others, Factor):
            others = [others]
        if isinstance(others, dict):
            if self.factor_name in others:
                raise ValueError(f"duplicate factor name {self.factor_name!r}")
            group = {self.factor_name: self, **others}
        else:
            group = [self] + list(others)
        out = factor_returns(group, **kw)
        if not isinstance(out, tuple):
            return out.loc[self.factor_name]
        extras = list(out[1:])
        if kw.get("return_daily"):
            extras[0] = extras[0][extras[0]["factor"] == self.factor_name].reset_index(drop=True)
        return (out[0].loc[self.factor_name], *extras)

    def orthogonal_to(self, others, **kw) -> "Factor":
        """This factor with the others taken out: the last output of the Gram-Schmidt
        :func:`orthogonalize` of ``[*others, self]`` (``others``: a Factor, a sequence of them
        or a mapping name -> Factor; keywords as there, ``method`` excepted), a new object of
        this class named ``f"{factor_name}_orth"``."""
        if "method" in kw or "return_info" in kw:
            raise ValueError("orthogonal_to is Gram-Schmidt and returns the factor alone")
        if isinstance(others, Factor):
            others = [others]
        if isinstance(others, dict):
            if self.factor_name in others:
                raise ValueError(f"duplicate factor name {self.factor_name!r}")
            group = {**others, self.factor_name: self}
        else:
            group = list(others) + [self]
        out = orthogonalize(group, method="schmidt", **kw)
        return out[self.factor_name]

    def combine_with(self, others, **kw):
        """:func:`combine` of ``[self, *others]`` (``others``: a Factor, a sequence of them or a
        mapping name -> Factor; keywords as there): the composite :class:`Factor`, with
        ``return_info`` followed by the weights and IC frames."""
        if isinstance(others, Factor):
            others = [others]
        if isinstance(others, dict):
            if self.factor_name in others:
                raise ValueError(f"duplicate factor name {self.factor_name!r}")
            group = {self.factor_name: self, **others}
        else:
            group = [self] + list(others)
        return combine(group, **kw)


def _industry_ids(industry, codes, dates):
    """``industry`` (None, or a long frame [code, industry] / [code, date, industry]; labels of
    any hashable dtype, a null label = no industry) -> (int32 ids [D][S] with -1 = none, the
    number of labels G), or (None, None).  Shared by Factor.neutralize and factor_returns."""
    from . import engine

    pd = _pd()
    if industry is None:
        return None, None
    D, S = len(dates), len(codes)
    cols = list(getattr(industry, "columns", []))
    if "code" not in cols or "industry" not in cols:
        raise ValueError("industry must be a frame with columns [code, industry] or "
                         "[code, date, industry]")
    ids, labels = pd.factorize(industry["industry"])  # a null label: -1
    G = max(len(labels), 1)
    if G > engine.NEUTRALIZE_MAX_GROUPS:
        raise ValueError(f"industry holds {G} distinct labels, more than the "
                         f"{engine.NEUTRALIZE_MAX_GROUPS} the kernel takes")
    ids = np.asarray(ids, dtype=np.int64)
    code_pos = pd.Index(codes).get_indexer(industry["code"].astype(str))
    grp = np.full((D, S), -1, dtype=np.int32)
    if "date" in cols:
        day_pos = pd.Index(dates).get_indexer([frames._as_date(d) for d in industry["date"]])
        ok = (code_pos >= 0) & (day_pos >= 0)
        grp[day_pos[ok], code_pos[ok]] = ids[ok]
    else:
        ok = code_pos >= 0
        if len(np.unique(code_pos[ok])) != int(ok.sum()):
            raise ValueError("industry without a date column must hold one row per code")
        grp[:, code_pos[ok]] = ids[ok][None, :]
    return grp, G


def _named_factors(factors, what):
    """A sequence of Factor objects or a mapping name -> Factor -> (names, objects);
    duplicate names raise ValueError."""
    if isinstance(factors, dict):
        names, objs = [str(k) for k in factors.keys()], list(factors.values())
    else:
        objs = list(factors)
        names = [f.factor_name for f in objs]
    if not objs:
        raise ValueError(f"{what} needs at least one factor")
    seen = set()
    for nm in names:
        if nm in seen:
            raise ValueError(f"duplicate factor name {nm!r}")
        seen.add(nm)
    return names, objs


def factor_returns(factors, future_days: int = 1, industry=None, weight: Literal["cmc", "tmc", None] = None,
                   min_obs: Optional[int] = None, return_daily: bool = False, return_residual: bool = False,
                   pv_data=None, device=None):
    """Per-date cross-sectional regression of the forward return on several factors at once
    (Fama-MacBeth / pure factor returns) on the GPU (mff_xs_reg_*, include/mff.h): weighted
    least squares of the ``future_days`` compounded return on industry dummies and every
    factor's exposure over the codes where all of them hold a finite value, then the time
    aggregate of the coefficients.  No reference counterpart: Factor.py never regresses.

    ``factors``: a sequence of :class:`Factor` or a mapping name -> Factor (duplicate names
    raise ValueError); the universe is the union of their codes and dates and ``pv_data``
    (default: the daily price-volume file; columns code, date, pct_change and the weight
    column).  ``industry``: as in :meth:`Factor.neutralize` (None: a plain intercept).
    ``weight``: None, or 'cmc' / 'tmc' for w = sqrt(cap); a null, non-finite or <= 0 cap
    means no weight (the stock-day drops out).  ``min_obs``: fewer usable codes on a date
    give no result for it (None: 0, only the degrees-of-freedom rule applies).

    Returns a DataFrame indexed by factor name with the columns days, mean, std, t_fm,
    mean_abs_t, share_abs_t_gt_2, mean_r2, mean_n.  With ``return_daily=True`` also a long
    frame [date, factor, ret, t] of the dates with a result, sorted by (date, factor in the
    order given), and a per-date frame [date, n, dof, r2, status]; with
    ``return_residual=True`` also a :class:`Factor` named "specific_return" holding the
    residual.  The extras follow the aggregate in that order, as a tuple."""
    import torch

    from . import engine
    from .factors import _device

    pd = _pd()
    if weight not in (None, "tmc", "cmc"):
        raise ValueError(f"weight must be 'tmc', 'cmc' or None, got {weight!r}")
    if min_obs is None:
        min_obs = 0
    if isinstance(min_obs, bool) or not isinstance(min_obs, (int, np.integer)) or min_obs < 0:
        raise ValueError(f"min_obs must be an integer >= 0, got {min_obs!r}")
    names, objs = _named_factors(factors, "factor_returns")
    need = ["code", "date", "pct_change"] + ([weight] if weight else [])
    pv = pv_data if pv_data is not None else Factor._read_daily_pv_data(need)
    for c in need:
        if c not in pv.columns:
            raise ValueError(f"pv_data has no column {c!r}")
    exposures = [f.factor_exposure for f in objs]
    codes, dates = frames.universe(*exposures, pv)
    K, D, S = len(objs), len(dates), len(codes)
    grp, G = _industry_ids(industry, codes, dates)
    val = np.zeros((K, D, S), dtype=np.float64)
    state = np.zeros((K, D, S), dtype=np.uint8)
    for i, (f, ex) in enumerate(zip(objs, exposures)):
        val[i], state[i], _, _ = frames.from_long(ex, f.factor_name, codes=codes, dates=dates)
    dev = _device(device)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    pc_v, pc_s, _, _ = frames.from_long(pv, "pct_change", codes=codes, dates=dates)
    yv, ys = engine.future_return(t(pc_v), t(pc_s), future_days)
    wv = ws = None
    if weight is not None:
        c_v, c_s, _, _ = frames.from_long(pv, weight, codes=codes, dates=dates)
        cap, cst = t(c_v), t(c_s)
        ok = (cst == engine.VALUE) & torch.isfinite(cap) & (cap > 0)
        wv = torch.where(ok, torch.sqrt(torch.where(ok, cap, torch.ones_like(cap))), torch.zeros_like(cap))
        ws = torch.where(ok, cst, torch.where(cst == engine.ABSENT, cst, torch.full_like(cst, engine.NULL)))
    res = engine.factor_regress(t(val), t(state), yv, ys, wv, ws, None if grp is None else t(grp), G=G,
                                min_obs=int(min_obs), residual=bool(return_residual))
    agg, overall = engine.factor_regress_mean(res)
    torch.cuda.synchronize(dev)
    out = pd.DataFrame(agg.cpu().numpy(), index=list(names), columns=list(engine.REG_AGG_COLUMNS))
    out["days"] = out["days"].astype(np.int64)
    ov = overall.cpu().numpy()
    out["mean_r2"], out["mean_n"] = ov[0], ov[1]
    extras = []
    if return_daily:
        status = res.status.cpu().numpy()
        beta, tst = res.beta.cpu().numpy(), res.tstat.cpu().numpy()
        d_idx = np.nonzero(status == 0)[0]
        dd = np.asarray(dates, dtype=object)
        daily = pd.DataFrame({"date": np.repeat(dd[d_idx], K), "factor": np.tile(np.asarray(names, dtype=object), len(d_idx)),
                              "ret": beta[d_idx].reshape(-1), "t": tst[d_idx].reshape(-1)})
        per_date = pd.DataFrame({"date": dd, "n": res.n.cpu().numpy(), "dof": res.dof.cpu().numpy(),
                                 "r2": res.r2.cpu().numpy(), "status": status})
        extras += [daily, per_date]
    if return_residual:
        extras.append(Factor("specific_return", frames.to_long(res.resid_val.cpu().numpy(), res.resid_state.cpu().numpy(),
                                                               codes, dates, "specific_return")))
    return (out, *extras) if extras else out


def orthogonalize(factors, method: str = "symmetric", min_obs: Optional[int] = None, return_info: bool = False,
                  device=None):
    """Per-date orthogonalisation of several factors' exposures on the GPU (mff_xs_orth_*,
    include/mff.h): over the codes of a date where all of them hold a finite value the
    exposures are standardised and mapped to as many mutually uncorrelated unit-variance
    columns.  No reference counterpart: Factor.py never combines factors.

    ``factors``: a sequence of :class:`Factor` or a mapping name -> Factor (duplicate names
    raise ValueError), aligned on the union of their codes and dates.  ``method``:
    'symmetric' (Loewdin: the orthonormal set closest to the standardised inputs, no factor
    preferred) or 'schmidt' (Gram-Schmidt in the order given: each factor with the earlier
    ones taken out).  ``min_obs``: fewer usable codes on a date (or fewer than the number of
    factors + 1) give no result for it (None: 0).  A stock-day with a value but outside the
    usable set, or on a date without a result, comes out null.

    Returns ``{name: Factor}`` in input order, each object of its input's class, named
    ``f"{name}_orth"`` and holding [code, date, <that name>]; the inputs are untouched.  With
    ``return_info=True`` also a per-date frame [date, n, status, eig_min, eig_max, cond]
    (eigenvalues of the date's correlation matrix) and a frame indexed by factor name with
    days, mean_keep, min_keep over the dates with a result (keep = the correlation of the
    output with its input), as a tuple."""
    import torch

    from . import engine
    from .factors import _device

    pd = _pd()
    if method not in engine.ORTH_METHODS:
        raise ValueError(f"method must be one of {engine.ORTH_METHODS}, got {method!r}")
    if min_obs is None:
        min_obs = 0
    if isinstance(min_obs, bool) or not isinstance(min_obs, (int, np.integer)) or min_obs < 0:
        raise ValueError(f"min_obs must be an integer >= 0, got {min_obs!r}")
    names, objs = _named_factors(factors, "orthogonalize")
    exposures = [f.factor_exposure for f in objs]
    codes, dates = frames.universe(*exposures)
    K, D, S = len(objs), len(dates), len(codes)
    val = np.zeros((K, D, S), dtype=np.float64)
    state = np.zeros((K, D, S), dtype=np.uint8)
    for i, (f, ex) in enumerate(zip(objs, exposures)):
        val[i], state[i], _, _ = frames.from_long(ex, f.factor_name, codes=codes, dates=dates)
    dev = _device(device)
    res = engine.factor_orthogonalize(torch.from_numpy(val).to(dev), torch.from_numpy(state).to(dev), method=method,
                                      min_obs=int(min_obs))
    torch.cuda.synchronize(dev)
    ov, os_ = res.val.cpu().numpy(), res.state.cpu().numpy()
    out = {}
    for i, (nm, f) in enumerate(zip(names, objs)):
        new = f"{nm}_orth"
        out[nm] = type(f)(new, frames.to_long(ov[i], os_[i], codes, dates, new))
    if not return_info:
        return out
    status, eig, keep = res.status.cpu().numpy(), res.eig.cpu().numpy(), res.keep.cpu().numpy()
    per_date = pd.DataFrame({"date": np.asarray(dates, dtype=object), "n": res.n.cpu().numpy(), "status": status,
                             "eig_min": eig[:, 0], "eig_max": eig[:, -1], "cond": eig[:, -1] / eig[:, 0]})
    ok = keep[status == 0]
    days = len(ok)
    per_factor = pd.DataFrame({"days": np.full(K, days, dtype=np.int64),
                               "mean_keep": ok.mean(axis=0) if days else np.full(K, np.nan),
                               "min_keep": ok.min(axis=0) if days else np.full(K, np.nan)}, index=list(names))
    return out, per_date, per_factor


def combine(factors, method: str = "icir", future_days: int = 5, window: int = 60, min_periods: int = 20,
            ic: str = "pearson", shrink: float = 0.5, min_factors: int = 1, name: str = "composite",
            return_info: bool = False, pv_data=None, device=None):
    """One composite factor from several factors' exposures on the GPU (mff_xs_comb_*,
    include/mff.h): per date every factor's cross-sectional z-score, weighted and summed per
    code over the factors that code has (at least ``min_factors`` of them, else null; the
    weights are renormalised over those).  No reference counterpart: Factor.py never combines
    factors.

    ``method``: 'equal'; 'ic' (the factor's mean IC against the ``future_days`` compounded
    return over the trailing ``window`` dates whose horizon has closed -- no look-ahead);
    'icir' (mean / std of those ICs); 'max_icir' (Sigma_s^-1 mu of the factors' IC means and
    covariance over the dates where all have an IC, the off-diagonal shrunk by ``shrink`` in
    [0, 1]).  A factor with fewer than ``min_periods`` ICs in the window gets weight 0; a date
    where none qualifies, or whose covariance is singular, has no composite.  ``ic``:
    'pearson' or 'rank'.

    ``factors``: a sequence of :class:`Factor` or a mapping name -> Factor (duplicate names
    raise ValueError); the universe is the union of their codes and dates and, unless
    ``method='equal'`` (which reads no ``pv_data``), of ``pv_data`` (default: the daily
    price-volume file; columns code, date, pct_change).

    Returns a :class:`Factor` named ``name`` holding [code, date, ``name``]; the inputs are
    untouched.  With ``return_info=True`` also a weights frame [date, status, <one column per
    factor>] and an IC frame [date, <one column per factor>], as a tuple."""
    import torch

    from . import engine
    from .factors import _device

    pd = _pd()
    if method not in engine.COMBINE_METHODS:
        raise ValueError(f"method must be one of {engine.COMBINE_METHODS}, got {method!r}")
    if ic not in engine.COMBINE_IC:
        raise ValueError(f"ic must be one of {engine.COMBINE_IC}, got {ic!r}")
    for what, v, lo in (("future_days", future_days, 1), ("window", window, 1), ("min_periods", min_periods, 1),
                        ("min_factors", min_factors, 1)):
        engine._int_arg(what, v, lo)
    if isinstance(shrink, bool) or not isinstance(shrink, (int, float, np.integer, np.floating)) \
            or not 0.0 <= float(shrink) <= 1.0:
        raise ValueError(f"shrink must be a number in [0, 1], got {shrink!r}")
    if not isinstance(name, str) or not name:
        raise ValueError(f"name must be a non-empty string, got {name!r}")
    names, objs = _named_factors(factors, "combine")
    if return_info and {"date", "status"} & set(names):
        raise ValueError("a factor named 'date' or 'status' collides with the columns of the info frames")
    if min_factors > len(objs):
        raise ValueError(f"min_factors must be at most the number of factors {len(objs)}, got {min_factors!r}")
    if len(objs) > engine.COMBINE_MAX_FACTORS:
        raise ValueError(f"combine takes at most {engine.COMBINE_MAX_FACTORS} factors, got {len(objs)}")
    exposures = [f.factor_exposure for f in objs]
    pv = None
    if method != "equal":
        need = ["code", "date", "pct_change"]
        pv = pv_data if pv_data is not None else Factor._read_daily_pv_data(need)
        for c in need:
            if c not in pv.columns:
                raise ValueError(f"pv_data has no column {c!r}")
    codes, dates = frames.universe(*exposures, pv) if pv is not None else frames.universe(*exposures)
    K, D, S = len(objs), len(dates), len(codes)
    val = np.zeros((K, D, S), dtype=np.float64)
    state = np.zeros((K, D, S), dtype=np.uint8)
    for i, (f, ex) in enumerate(zip(objs, exposures)):
        val[i], state[i], _, _ = frames.from_long(ex, f.factor_name, codes=codes, dates=dates)
    dev = _device(device)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    yv = ys = None
    if pv is not None:
        pc_v, pc_s, _, _ = frames.from_long(pv, "pct_change", codes=codes, dates=dates)
        yv, ys = engine.future_return(t(pc_v), t(pc_s), future_days)
    res = engine.factor_combine(t(val), t(state), yv, ys, method=method, future_days=int(future_days),
                                window=int(window), min_periods=int(min_periods), ic=ic, shrink=float(shrink),
                                min_factors=int(min_factors))
    torch.cuda.synchronize(dev)
    out = Factor(name, frames.to_long(res.val.cpu().numpy(), res.state.cpu().numpy(), codes, dates, name))
    if not return_info:
        return out
    dd = np.asarray(dates, dtype=object)
    w, icv = res.weights.cpu().numpy(), res.ic.cpu().numpy()
    wf = pd.DataFrame({"date": dd, "status": res.status.cpu().numpy(), **{nm: w[:, k] for k, nm in enumerate(names)}})
    icf = pd.DataFrame({"date": dd, **{nm: icv[k] for k, nm in enumerate(names)}})
    return out, wf, icf


def factor_correlation(factors, method: str = "pearson", min_pairs: int = 2, return_daily: bool = False,
                       device=None):
    """Cross-sectional correlation matrix of several factors' exposures on the GPU
    (mff_xs_corr_*, include/mff.h): per date the pairwise-complete Pearson correlation of
    every pair over the codes where both hold a finite value, then the mean over the dates
    where it is defined.  No reference counterpart: Factor.py never relates two factors.

    ``factors``: a sequence of :class:`Factor` objects or a mapping name -> Factor (the
    mapping's keys name the rows); duplicate names raise ValueError.  The exposures are
    aligned on the union of their codes and dates; a stock-day missing from a factor's frame
    is absent for that factor.  ``method``: 'pearson' or 'spearman' (each factor ranked per
    date over its own finite values; the ranks are not recomputed per pair, which equals
    ``pandas.corr(method='spearman')`` when the factors share their coverage).
    ``min_pairs`` >= 2: fewer common codes on a date give NaN for that date.

    Returns the F x F pandas DataFrame of the time means (index and columns = the names);
    with ``return_daily=True`` also a long frame [date, factor_a, factor_b, corr, n] of the
    upper triangle (in the order of ``factors``) including the diagonal, rows with n >= 1
    only, sorted by (date, factor_a, factor_b)."""
    import torch

    from . import engine
    from .factors import _device

    pd = _pd()
    if method not in engine.CORR_METHODS:
        raise ValueError(f"method must be one of {engine.CORR_METHODS}, got {method!r}")
    if isinstance(min_pairs, bool) or not isinstance(min_pairs, (int, np.integer)) or min_pairs < 2:
        raise ValueError(f"min_pairs must be an integer >= 2, got {min_pairs!r}")
    if isinstance(factors, dict):
        names, objs = [str(k) for k in factors.keys()], list(factors.values())
    else:
        objs = list(factors)
        names = [f.factor_name for f in objs]
    if not objs:
        raise ValueError("factor_correlation needs at least one factor")
    seen = set()
    for nm in names:
        if nm in seen:
            raise ValueError(f"duplicate factor name {nm!r}")
        seen.add(nm)
    exposures = [f.factor_exposure for f in objs]
    codes, dates = frames.universe(*exposures)
    F, D, S = len(objs), len(dates), len(codes)
    val = np.zeros((F, D, S), dtype=np.float64)
    state = np.zeros((F, D, S), dtype=np.uint8)
    for i, (f, ex) in enumerate(zip(objs, exposures)):
        val[i], state[i], _, _ = frames.from_long(ex, f.factor_name, codes=codes, dates=dates)
    dev = _device(device)
    corr, n = engine.factor_corr(torch.from_numpy(val).to(dev), torch.from_numpy(state).to(dev), method=method,
                                 min_pairs=int(min_pairs))
    mean, _ = engine.factor_corr_mean(corr)
    torch.cuda.synchronize(dev)
    out = pd.DataFrame(mean.cpu().numpy(), index=list(names), columns=list(names))
    if not return_daily:
        return out
    corr, n = corr.cpu().numpy(), n.cpu().numpy()
    iu, ju = np.triu_indices(F)
    keep = n[:, iu, ju] >= 1                      # [D][pairs]
    d_idx, p_idx = np.nonzero(keep)
    nm = np.asarray(names, dtype=object)
    daily = pd.DataFrame({"date": np.asarray(dates, dtype=object)[d_idx],
                          "factor_a": nm[iu[p_idx]], "factor_b": nm[ju[p_idx]],
                          "corr": corr[d_idx, iu[p_idx], ju[p_idx]],
                          "n": n[d_idx, iu[p_idx], ju[p_idx]]})
    return out, daily.sort_values(["date", "factor_a", "factor_b"], kind="stable").reset_index(drop=True)


PORTFOLIO_SUMMARY = ("days", "total_return", "annual_return", "annual_vol", "sharpe", "max_drawdown",
                     "mean_turnover", "total_cost")


def _series_summary(ret_net, traded, present, cost, annual_days):
    """Summary columns of one portfolio: ret_net [n] daily, traded / present [periods of the window]."""
    n = len(ret_net)
    nav = np.cumprod(1.0 + ret_net)
    out = dict.fromkeys(PORTFOLIO_SUMMARY, np.nan)
    out["days"] = n
    out["total_cost"] = float(np.sum(cost * traded))
    out["mean_turnover"] = float(np.mean(traded[present] / 2.0)) if present.any() else np.nan
    if n == 0:
        return out
    out["total_return"] = float(nav[-1] - 1.0)
    out["annual_return"] = float(nav[-1] ** (annual_days / n) - 1.0)
    if n >= 2:
        sd = float(np.std(ret_net, ddof=1))
        out["annual_vol"] = sd * np.sqrt(annual_days)
        if sd > 0:
            out["sharpe"] = float(np.mean(ret_net)) / sd * np.sqrt(annual_days)
    peak = np.maximum.accumulate(np.concatenate([[1.0], nav]))[1:]  # the running maximum starts at 1
    out["max_drawdown"] = float(np.max(1.0 - nav / peak))
    return out


def portfolio_statistics(ret, count, traded, period_of, cost: float = 0.0, annual_days: int = 252):
    """Host side of :func:`portfolio_tests` for one factor, numpy f64: ret [D][G], count [P][G],
    traded [P][G] (engine.group_portfolios) -> a dict with

    * ``names``: group_1..group_G and, when G >= 2, long_short (group_G minus group_1);
    * ``d0`` / ``p0``: the window starts on the first date of the first period with a present
      cell (count > 0) and runs to the last date; d0 = D, p0 = P when no cell is present;
    * ``ret`` / ``ret_net`` / ``nav`` [names][D - d0]: ret_net = (1 + ret)(1 - cost traded(p)) - 1
      on the first date of period p, else ret; long_short: ret_G - ret_1 less cost (traded_G +
      traded_1) on a period's first date; nav = cumprod(1 + ret_net);
    * ``traded`` [names][P - p0] (long_short: the sum of its legs), ``present`` likewise
      (long_short: either leg);
    * ``summary``: one dict of PORTFOLIO_SUMMARY per name: annual_return =
      nav_last^(annual_days / days) - 1, annual_vol = std(ddof=1) sqrt(annual_days), sharpe =
      mean / std sqrt(annual_days) (NaN when days < 2 or std = 0), max_drawdown against the
      running maximum starting at 1, mean_turnover = mean of traded / 2 over the present
      periods, total_cost = sum of cost traded."""
    ret = np.asarray(ret, dtype=np.float64)
    count, traded = np.asarray(count), np.asarray(traded, dtype=np.float64)
    period_of = np.asarray(period_of, dtype=np.int64)
    D, G = ret.shape
    P = count.shape[0]
    pres = count > 0
    held = np.flatnonzero(pres.any(axis=1))
    p0 = int(held[0]) if held.size else P
    d0 = int(np.searchsorted(period_of, p0, side="left"))
    per = period_of[d0:]
    first = np.ones(D - d0, dtype=bool)
    first[1:] = per[1:] != per[:-1]
    names = [f"group_{g + 1}" for g in range(G)]
    r = ret[d0:].T.copy()                                   # [G][n]
    charge = np.where(first[None, :], cost * traded[per].T, 0.0)
    rn = (1.0 + r) * (1.0 - charge) - 1.0
    tr, pr = traded[p0:].T.copy(), pres[p0:].T.copy()
    if G >= 2:
        names.append("long_short")
        ls = r[G - 1] - r[0]
        r = np.vstack([r, ls])
        rn = np.vstack([rn, ls - (charge[G - 1] + charge[0])])
        tr = np.vstack([tr, tr[G - 1] + tr[0]])
        pr = np.vstack([pr, pr[G - 1] | pr[0]])
    nav = np.cumprod(1.0 + rn, axis=1)
    summary = [_series_summary(rn[i], tr[i], pr[i], cost, annual_days) for i in range(len(names))]
    return {"names": names, "d0": d0, "p0": p0, "ret": r, "ret_net": rn, "nav": nav, "traded": tr,
            "present": pr, "summary": summary}


def portfolio_tests(factors, frequency: Literal["weekly", "monthly", "quarterly", "yearly"] = "monthly",
                    weight_param: Literal["tmc", "cmc", None] = None, group_num: int = 5, cost: float = 0.0,
                    annual_days: int = 252, return_daily: bool = False, pv_data=None, device=None):
    """Daily back-test of the ``group_num`` quantile portfolios of several factors at once on
    the GPU (mff_pf_*, include/mff.h): the groups of :meth:`Factor.group_test`, held with
    drifting weights between the rebalances of ``frequency``, give a daily return per group,
    the top-minus-bottom portfolio and the turnover of every rebalance; the host turns them into
    series net of ``cost`` (a rate in [0, 1) per unit traded, both sides counted) and summary
    statistics (:func:`portfolio_statistics`).  Compounded over a period the daily return is
    group_test's number.  No reference counterpart: Factor.py stops at one return per period.

    ``factors``: a sequence of :class:`Factor` or a mapping name -> Factor (duplicate names
    raise ValueError), aligned on the union of their codes and dates; ``pv_data`` (default: the
    daily price-volume file) gives pct_change and the ``weight_param`` column.  Many factors run
    through the device in chunks of at most engine.PORTFOLIO_BYTES of planes.

    Returns a long frame [factor, portfolio, days, total_return, annual_return, annual_vol,
    sharpe, max_drawdown, mean_turnover, total_cost] with portfolios group_1..group_G and (G >= 2)
    long_short.  With ``return_daily=True`` also [date, factor, portfolio, ret, ret_net, nav] and
    [date (period right edge), factor, group, count, turnover, cost] (turnover = traded / 2,
    cost = ``cost`` x traded), both from the first period in which a group holds a stock."""
    import torch

    from . import engine
    from .factors import _device

    pd = _pd()
    if weight_param not in (None, "tmc", "cmc"):
        raise ValueError(f"weight_param must be 'tmc', 'cmc' or None, got {weight_param!r}")
    G = engine._int_arg("group_num", group_num, 1)
    if G > engine.PORTFOLIO_MAX_GROUPS:
        raise ValueError(f"group_num must be at most {engine.PORTFOLIO_MAX_GROUPS}, got {group_num!r}")
    annual_days = engine._int_arg("annual_days", annual_days, 1)
    if isinstance(cost, bool) or not isinstance(cost, (int, float, np.integer, np.floating)) \
            or not 0.0 <= float(cost) < 1.0:
        raise ValueError(f"cost must be a number in [0, 1), got {cost!r}")
    cost = float(cost)
    names, objs = _named_factors(factors, "portfolio_tests")
    need = ["code", "date", "pct_change"] + ([weight_param] if weight_param else [])
    pv = pv_data if pv_data is not None else Factor._read_daily_pv_data(need)
    for c in need:
        if c not in pv.columns:
            raise ValueError(f"pv_data has no column {c!r}")
    exposures = [f.factor_exposure for f in objs]
    codes, dates = frames.universe(*exposures)
    pv = pv[frames.rows_in(pv, codes, dates)]
    period_of, labels = rebalance_periods(dates, frequency)
    K, D, S, P = len(objs), len(dates), len(codes), len(labels)
    dev = _device(device)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    pc_v, pc_s, _, _ = frames.from_long(pv, "pct_change", codes=codes, dates=dates)
    pcv, pcs = t(pc_v), t(pc_s)
    wv = ws = None
    if weight_param is not None:
        w_v, w_s, _, _ = frames.from_long(pv, weight_param, codes=codes, dates=dates)
        wv, ws = t(w_v), t(w_s)
    per_d = t(period_of.astype(np.int32))
    kc = max(1, engine.PORTFOLIO_BYTES // max(1, D * S * 10 + P * S * 17))
    ret = np.zeros((K, D, G))
    count = np.zeros((K, P, G), dtype=np.int32)
    traded = np.zeros((K, P, G))
    for k0 in range(0, K, kc):
        k1 = min(K, k0 + kc)
        val = np.zeros((k1 - k0, D, S), dtype=np.float64)
        state = np.zeros((k1 - k0, D, S), dtype=np.uint8)
        for i in range(k0, k1):
            val[i - k0], state[i - k0], _, _ = frames.from_long(exposures[i], objs[i].factor_name, codes=codes,
                                                                 dates=dates)
        res = engine.group_portfolios(t(val), t(state), pcv, pcs, per_d, P, G, wv, ws)
        torch.cuda.synchronize(dev)
        ret[k0:k1], count[k0:k1], traded[k0:k1] = (res.ret.cpu().numpy(), res.count.cpu().numpy(),
                                                  res.traded.cpu().numpy())
    dd, ll = np.asarray(dates, dtype=object), np.asarray(labels, dtype=object)
    rows, daily, periods = [], [], []
    for k, nm in enumerate(names):
        st = portfolio_statistics(ret[k], count[k], traded[k], period_of, cost, annual_days)
        for i, pn in enumerate(st["names"]):
            rows.append({"factor": nm, "portfolio": pn, **st["summary"][i]})
        if return_daily:
            d0, p0 = st["d0"], st["p0"]
            for i, pn in enumerate(st["names"]):
                daily.append(pd.DataFrame({"date": dd[d0:], "factor": nm, "portfolio": pn, "ret": st["ret"][i],
                                           "ret_net": st["ret_net"][i], "nav": st["nav"][i]}))
            for g in range(G):
                periods.append(pd.DataFrame({"date": ll[p0:], "factor": nm, "group": f"group_{g + 1}",
                                             "count": count[k, p0:, g], "turnover": traded[k, p0:, g] / 2.0,
                                             "cost": cost * traded[k, p0:, g]}))
    out = pd.DataFrame(rows, columns=["factor", "portfolio", *PORTFOLIO_SUMMARY])
    if not return_daily:
        return out
    daily_df = pd.concat(daily, ignore_index=True) if daily else pd.DataFrame(
        columns=["date", "factor", "portfolio", "ret", "ret_net", "nav"])
    period_df = pd.concat(periods, ignore_index=True) if periods else pd.DataFrame(
        columns=["date", "factor", "group", "count", "turnover", "cost"])
    return out, daily_df, period_df


def rebalance_periods(dates, frequency: str):
    """group_by_dynamic(every=1w/1mo/1q/1y, label='right') windows (Factor.py:249-256,
    295-297) of sorted dates -> (period index per date, right-edge label per period)."""
    pd = _pd()
    freq = {"weekly": "W-SUN", "monthly": "M", "quarterly": "Q", "yearly": "Y"}.get(frequency)
    if freq is None:
        raise ValueError(f"Unsupported frequency: {frequency}")
    per = pd.to_datetime(pd.Series(list(dates))).dt.to_period(freq)
    codes, uniq = pd.factorize(per, sort=True)
    labels = [(u.end_time.normalize() + pd.Timedelta(days=1)).date() for u in uniq]
    return np.asarray(codes, dtype=np.int64), labels


def calendar_windows(dates, frequency: str):
    """group_by_dynamic(every='1w'/'1mo') windows with polars' defaults (closed='left',
    label='left', windows truncated to Monday / the 1st) over sorted dates ->
    (period_start int32 [P+1]: first date index of each window, then len(dates); the
    windows' left-edge labels)."""
    pd = _pd()
    freq = {"weekly": "W-SUN", "monthly": "M"}.get(frequency)
    if freq is None:
        raise ValueError(f"Unsupported frequency for calendar: {frequency}")
    per = pd.to_datetime(pd.Series(list(dates))).dt.to_period(freq)
    codes, uniq = pd.factorize(per, sort=True)
    codes = np.asarray(codes)
    if np.any(np.diff(codes) < 0):
        raise ValueError("dates must be sorted")
    start = np.searchsorted(codes, np.arange(len(uniq)), side="left")
    pstart = np.append(start, len(dates)).astype(np.int32)
    return pstart, [u.start_time.date() for u in uniq]


class MinFreqFactor(Factor):
    """MinuteFrequentFactorCICC.py:8-245."""

    def __init__(self, factor_name, factor_exposure=None):
        super().__init__(factor_name, factor_exposure)

    @staticmethod
    def _read_day_file(path):
        import pyarrow.parquet as pq
        return pq.read_table(path)

    @staticmethod
    def _process_single_file(file_name, folder_path, calculate_method):
        """MF:17-25: a host callable on one day file; errors print and skip the day."""
        try:
            file_path = os.path.join(folder_path, file_name)
            return calculate_method(MinFreqFactor._read_day_file(file_path).to_pandas())
        except Exception as e:
            print(f"处理文件 {file_name} 时出错: {str(e)}")
            return None

    @staticmethod
    def _read_exposure(factor_name: str, path: Optional[str], default_path: str):
        """MF:27-48."""
        import pyarrow.parquet as pq

        if path is None:
            path = default_path
        if path.endswith(".parquet"):
            return pq.read_table(path).to_pandas(types_mapper=_arrow_float_mapper)
        if os.path.isdir(path) and f"{factor_name}.parquet" in os.listdir(path):
            return pq.read_table(os.path.join(path, f"{factor_name}.parquet")).to_pandas(
                types_mapper=_arrow_float_mapper)
        return None

    def cal_exposure_by_min_data(self, calculate_method, path: str = None, n_jobs: int = None,
                                 folder_path: Optional[str] = None, batch_days: int = 64,
                                 device=None, strict: bool = False):
        """MF:50-112: compute the exposure from per-day minute files, updating an
        existing exposure incrementally (only dates after its max date).

        `calculate_method` is one of the mff ``cal_*`` functions (or a factor name): the
        day files are read in batches of `batch_days`, turned into one dense panel and
        run through the stage-1 kernel (every factor at once; the batch's results are kept
        in a host cache keyed by the files' path / size / mtime, so the next factor over
        the same files costs no re-read and no re-ingest, see :func:`result_cache_info`).
        A day file that cannot be read or breaks the input contract is reported with the
        reference's message and dropped, the other days of its batch unaffected
        (MF:18-25, 95); ``strict=True`` raises instead, naming the file.  Any other
        callable runs per file on the host exactly as the reference does (joblib process
        pool, errors print and skip)."""
        factor_exposure = self._read_exposure(
            factor_name=self.factor_name,
            default_path=os.path.join(_EXPOSURE_DIR, "CICC Factor"), path=path)
        folder_path = folder_path or _KLINE_DIR
        files = _pending_files(folder_path, factor_exposure)

        name = getattr(calculate_method, "_mff_factor", None)
        if isinstance(calculate_method, str):
            name = calculate_method[4:] if calculate_method.startswith("cal_") else calculate_method
        valid, gpu = [], False
        if files:
            if name is not None and name in catalog.ID:
                valid = _gpu_batches(files, folder_path, [name], batch_days, device, strict)[name]
                gpu = True
            else:
                from joblib import Parallel, delayed

                results = Parallel(n_jobs=-1 if n_jobs is None else n_jobs)(
                    delayed(self._process_single_file)(f, folder_path, calculate_method)
                    for f in files)
                valid = [r for r in results if r is not None]
        self.factor_exposure = _merge(factor_exposure, valid, presorted=gpu)

    @classmethod
    def cal_exposures_by_min_data(cls, calculate_methods=None, path: str = None,
                                  folder_path: Optional[str] = None, batch_days: int = 64,
                                  device=None, strict: bool = False):
        """Many factors over the same day files in ONE read / ingest / stage-1 pass per
        batch (the reference re-reads every file per factor, MF:87-94): returns
        {name: MinFreqFactor} with each factor's exposure updated exactly as
        ``cal_exposure_by_min_data`` would (its own stored exposure and resume date).
        calculate_methods: mff ``cal_*`` functions or names (default: all 58)."""
        names = []
        for m in (catalog.NAMES if calculate_methods is None else calculate_methods):
            nm = m if isinstance(m, str) else getattr(m, "_mff_factor", None)
            if nm is None:
                raise ValueError(f"{m!r} is not an mff cal_* function")
            nm = nm[4:] if nm.startswith("cal_") else nm
            if nm not in catalog.ID:
                raise ValueError(f"unknown factor {nm!r}")
            names.append(nm)
        folder_path = folder_path or _KLINE_DIR
        out, groups = {}, {}
        for nm in names:
            f = cls(nm)
            ex = f._read_exposure(factor_name=nm, default_path=os.path.join(_EXPOSURE_DIR, "CICC Factor"),
                                  path=path)
            out[nm] = (f, ex)
            groups.setdefault(tuple(_pending_files(folder_path, ex)), []).append(nm)
        for files, grp in groups.items():
            res = _gpu_batches(list(files), folder_path, grp, batch_days, device, strict) if files else {}
            for nm in grp:
                f, ex = out[nm]
                f.factor_exposure = _merge(ex, res.get(nm, []), presorted=True)
        return {nm: out[nm][0] for nm in names}

    def cal_final_exposure(self, frequency, method: str, mode: str = "calendar", pool="full"):
        """MF:114-245.  mode='days': per-code rolling over present rows on the GPU
        (stage 2).  mode='calendar': per code and calendar window (weekly: Monday-based
        weeks, monthly: calendar months; polars group_by_dynamic defaults closed='left',
        label='left') the last value / mean / (last - mean) / std / std (ddof=1) of the
        window's rows on the GPU (mff_calendar).  The reference raises inside polars there
        (group_by_dynamic without index_column, MF:145-178): this is the build's
        definition of the intended operation, argument checks as MF:131-140."""
        if mode == "calendar":
            if frequency not in ("weekly", "monthly"):
                raise ValueError(f"Unsupported frequency for calendar: {frequency}")
            if pool != "full":
                raise ValueError(f"不支持的股票池: {pool}")
            if method not in ("o", "m", "z", "std"):
                raise ValueError("Unknown method")
            import torch

            from . import engine
            from .factors import _device

            name = f"{frequency}_{self.factor_name}_{method}"  # MF:141
            val, state, codes, dates = frames.from_long(self.factor_exposure, self.factor_name)
            pstart, labels = calendar_windows(dates, frequency)
            dev = _device(None)
            ov, os_ = engine.calendar(torch.from_numpy(val).to(dev), torch.from_numpy(state).to(dev),
                                      torch.from_numpy(pstart).to(dev), method)
            torch.cuda.synchronize(dev)
            return frames.to_long(ov.cpu().numpy(), os_.cpu().numpy(), codes, labels, name)
        if mode != "days":
            raise ValueError(f"Unknown mode: {mode}")
        if not isinstance(frequency, int):
            raise ValueError(f"Unsupported frequency for days: {frequency}")
        if method not in ("o", "m", "z", "std"):
            raise ValueError("Unknown method")
        import torch

        from . import engine
        from .factors import _device

        name = f"{self.factor_name}_{frequency}_{method}"
        with _timing.phase("from_long"):
            val, state, codes, dates = frames.from_long(self.factor_exposure, self.factor_name)
        with _timing.phase("H2D + stage 2 + D2H"):
            dev = _device(None)
            v = torch.from_numpy(val[None]).to(dev)
            s = torch.from_numpy(state[None]).to(dev)
            ov, os_ = engine.rolling(v, s, frequency, method)
            torch.cuda.synchronize(dev)
            ov, os_ = ov[0].cpu().numpy(), os_[0].cpu().numpy()
        with _timing.phase("to_long"):
            return frames.to_long(ov, os_, codes, dates, name)


def _pending_files(folder_path, factor_exposure):
    """Day files of the folder (YYYYMMDD*.parquet, MF:68-78) after the exposure's max
    date (MF:79-81), sorted."""
    pd = _pd()
    file_names = sorted(f for f in os.listdir(folder_path) if f.endswith(".parquet"))
    index = pd.DataFrame({"file_name": file_names})
    index["date"] = pd.to_datetime(index["file_name"].str[:8], format="%Y%m%d").dt.date
    if factor_exposure is not None:
        end_date = frames.universe(factor_exposure)[1][-1]
        index = index[index["date"] > end_date]
    return index["file_name"].tolist()


def _ordered(frames_):
    """True if consecutive frames, each in (date, code) order (frames.to_long of the
    sorted universes), hold strictly increasing dates: their concatenation is sorted."""
    for a, b in zip(frames_, frames_[1:]):
        if len(a) and len(b) and not a["date"].iloc[-1] < b["date"].iloc[0]:
            return False
    return True


def _merge(factor_exposure, valid, presorted=False):
    """MF:97-110: old exposure + new rows, sorted [date, code].  presorted: `valid` are
    the GPU batches' frames (each already in (date, code) order), so without an old
    exposure the sort is skipped when the batches' dates do not overlap."""
    pd = _pd()
    with _timing.phase("merge + sort"):
        if factor_exposure is None:
            if not valid:
                return None
            if presorted and _ordered(valid):
                return valid[0] if len(valid) == 1 else pd.concat(valid, ignore_index=True)
            return _sort(pd.concat(valid, ignore_index=True))
        if valid:
            return _sort(pd.concat([factor_exposure] + valid, ignore_index=True))
        return factor_exposure


# ---------------------------------------------------------------- day-file batch results
# Dense stage-1 results of every factor per day-file batch, keyed by the batch's files
# (absolute path, size, mtime): a notebook running the 58 cal_* one after another over
# the same folder reads and ingests every file once.  Only batches read and computed without
# any error are cached (a read failure may be transient: the next call retries the
# files).  Entries are added while they fit MFF_RESULT_CACHE_BYTES (default 4 GiB; 0
# disables) and never evicted by a later insert (a scan longer than the cache keeps its
# head cached instead of thrashing); clear_result_cache() frees it.
_RESULTS: "OrderedDict" = None
_RESULTS_BYTES = 0


def clear_result_cache() -> None:
    global _RESULTS, _RESULTS_BYTES
    _RESULTS, _RESULTS_BYTES = None, 0


def result_cache_info() -> dict:
    return {"batches": 0 if _RESULTS is None else len(_RESULTS), "bytes": _RESULTS_BYTES,
            "cap": _cache_cap()}


def _cache_cap() -> int:
    return int(os.environ.get("MFF_RESULT_CACHE_BYTES", str(4 << 30)))


def _batch_key(folder_path, files, device):
    try:
        key = []
        for f in files:
            p = os.path.abspath(os.path.join(folder_path, f))
            st = os.stat(p)
            key.append((p, st.st_size, st.st_mtime_ns))
        return (str(device),) + tuple(key)
    except OSError:
        return None


def _batch_results(files, folder_path, device):
    """((val [58][D][S], state, codes, dates), {file name: error}, {file name: (factor names,
    error)}) of one batch of day files (all 58 factors, per-day semantics), from the cache
    or computed.  The third dict: files on which only those factors' calls fail (T2: the
    five OLS calls on a decreasing minute_in_trade, CM:114-118; their rows are ABSENT)."""
    global _RESULTS, _RESULTS_BYTES
    from collections import OrderedDict

    from .factors import compute_dense
    from .ingest import NoTables

    key = _batch_key(folder_path, files, device)
    if key is not None and _RESULTS is not None and key in _RESULTS:
        return _RESULTS[key]
    # the day files go to the ingest as paths: its host threads read (parquet, the code
    # column from the files' dictionary pages) and encode them while earlier files move
    # to the device; a file that cannot be read is reported like any other bad file
    paths = [os.path.join(folder_path, f) for f in files]
    errors, res, partial = {}, None, {}
    try:  # one reference call per file (per-day semantics); a bad file drops its day only
        v, s, _, codes, dates, dropped, part = compute_dense(paths, None, device, per_day=True, skip_bad=True)
        res = (v, s, codes, dates)
        partial = {files[k]: x for k, x in sorted(part.items())}
    except NoTables as e:
        dropped = e.dropped
    errors.update({files[k]: msg for k, msg in dropped.items()})
    out = (res, dict(sorted(errors.items())), partial)
    nbytes = 0 if res is None else res[0].nbytes + res[1].nbytes
    if key is not None and not errors and res is not None and _RESULTS_BYTES + nbytes <= _cache_cap():
        if _RESULTS is None:
            _RESULTS = OrderedDict()
        _RESULTS[key] = out
        _RESULTS_BYTES += nbytes
    return out


def _gpu_batches(files, folder_path, names, batch_days, device, strict=False):
    """{name: [long frames of each batch]} over the day files, batch_days at a time."""
    out = {nm: [] for nm in names}
    for b0 in range(0, len(files), batch_days):
        res, errors, partial = _batch_results(files[b0:b0 + batch_days], folder_path, device)
        errors = dict(errors)  # (the cached entry stays as it is)
        for f, (fns, msg) in partial.items():  # only those calls fail on the file (MF:20-25)
            errors.update({f: msg for nm in names if nm in fns})
        errors = dict(sorted(errors.items()))
        for f, msg in errors.items():
            if strict:
                raise ValueError(f"{f}: {msg}")
            print(f"处理文件 {f} 时出错: {msg}")
        if res is None:
            continue
        v, s, codes, dates = res
        with _timing.phase("to_long"):
            for nm in names:
                i = catalog.ID[nm]
                out[nm].append(frames.to_long(v[i], s[i], codes, dates, nm,
                                              first="date" if nm == "shape_skratio" else "code"))
    return out


def _arrow_float_mapper(t):
    import pandas as pd
    import pyarrow as pa

    return pd.ArrowDtype(pa.float64()) if pa.types.is_floating(t) else None


def _sort(df):
    return df.sort_values(["date", "code"], kind="stable").reset_index(drop=True)
