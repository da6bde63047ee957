"""mff — MI355X-native CICC minute-frequency factor engine.

Host-side mirror of the reference interface (C-X-Lu/Replication-of-Minute-Frequency-Factor)
over libmff.so (hand-written HIP for gfx950):

* :mod:`mff.factors`  — the 58 ``cal_*`` drop-in functions (MinuteFrequentFactorCalculateMethodsCICC.py)
* :mod:`mff.factor`   — ``Factor`` / ``MinFreqFactor`` (Factor.py, MinuteFrequentFactorCICC.py)
* :mod:`mff.engine`   — dense-panel device API (stage 1 / 2 / 3)
* :mod:`mff.dist`     — one process per GPU, stock-sharded, RCCL collectives
"""
from . import catalog  # noqa: F401

__version__ = "0.1.0"

__all__ = ["catalog", "combine", "factor_correlation", "factor_returns", "orthogonalize", "portfolio_tests"]


def __getattr__(name):
    # mff.factor_correlation / mff.factor_returns / mff.orthogonalize / mff.combine /
    # mff.portfolio_tests, resolved on first use
    # (mff.factor pulls in pandas-side helpers)
    if name == "factor_correlation":
        from .factor import factor_correlation
        return factor_correlation
    if name == "factor_returns":
        from .factor import factor_returns
        return factor_returns
    if name == "orthogonalize":
        from .factor import orthogonalize
        return orthogonalize
    if name == "combine":
        from .factor import combine
        return combine
    if name == "portfolio_tests":
        from .factor import portfolio_tests
        return portfolio_tests
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
