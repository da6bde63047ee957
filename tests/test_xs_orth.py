"""tests/xs_orth_ref.py (the numpy restatement of the per-day factor orthogonalisation,
include/mff.h mff_xs_orth_*) pinned on the CPU against independent second routes (the polar
factor of the thin SVD for the symmetric method, sign-fixed numpy.linalg.qr for
Gram-Schmidt), closed forms for one and two factors, and hand-made degenerate days.  The
binding of the C entry points and their argument checks are tested too, so this file fails
without the feature."""
import numpy as np
import pytest

import xs_orth_ref as ref
from xs_orth_ref import ABSENT, NULL, VALUE

TOL = dict(rtol=1e-11, atol=1e-11)
ENTRY_POINTS = ("mff_xs_orth_max_factors", "mff_xs_orth_workspace_bytes", "mff_xs_orth_sums", "mff_xs_orth_gram",
                "mff_xs_orth_solve", "mff_xs_orth_apply")


def _day(seed, n, K):
    rng = np.random.default_rng(seed)
    return 0.5 * rng.standard_normal((n, 1)) + np.sqrt(0.75) * rng.standard_normal((n, K)) + rng.standard_normal(K)


def _dense(X):
    n, K = X.shape
    return X.T[:, None, :].copy(), np.full((K, 1, n), VALUE, np.uint8)


def test_library_binds_the_orthogonalisation_entry_points():
    from mff import _lib
    for name in ENTRY_POINTS:
        assert name in _lib.SIGNATURES
    lib = _lib.load()
    for name in ENTRY_POINTS:
        assert hasattr(lib, name)
    assert lib.mff_xs_orth_max_factors() == 64
    assert lib.mff_xs_orth_workspace_bytes(0, 1, 1) == 0 and lib.mff_xs_orth_workspace_bytes(3, 2, 100) >= 2 * 100
    import mff
    from mff import engine
    assert "orthogonalize" in mff.__all__
    assert engine.ORTH_METHODS == ref.METHODS
    assert engine.OrthResult._fields == ("val", "state", "transform", "eig", "keep", "n", "status")


def test_c_abi_argument_checks():
    """Bad arguments return a negative code before anything touches a device."""
    from mff import _lib
    lib = _lib.load()
    fake = 4096  # never dereferenced: every call fails its checks first
    sums = lambda K=2, D=1, S=8, ns=1: lib.mff_xs_orth_sums(fake, fake, K, D, S, ns, fake, fake, None)
    gram = lambda K=2, D=1, S=8, R=1, ns=1: lib.mff_xs_orth_gram(fake, K, D, S, fake, R, ns, fake, fake, None)
    solve = lambda P=1, K=2, D=1, m=0, mo=0: lib.mff_xs_orth_solve(fake, P, K, D, m, mo, fake, fake, fake, fake, fake,
                                                                   fake, None)
    apply_ = lambda K=2, D=1, S=8: lib.mff_xs_orth_apply(fake, fake, K, D, S, fake, fake, fake, fake, None)
    for call, kw, word in ((sums, dict(K=0), b"K=0"), (sums, dict(K=65), b"K=65"), (sums, dict(D=-1), b"D=-1"),
                           (sums, dict(S=-1), b"S=-1"), (sums, dict(ns=0), b"nsplit=0"),
                           (gram, dict(K=0), b"K=0"), (gram, dict(K=65), b"K=65"), (gram, dict(R=0), b"R=0"),
                           (gram, dict(ns=0), b"nsplit=0"), (gram, dict(S=-2), b"S=-2"),
                           (solve, dict(P=0), b"P=0"), (solve, dict(K=65), b"K=65"), (solve, dict(m=2), b"method=2"),
                           (solve, dict(m=-1), b"method=-1"), (solve, dict(mo=-1), b"min_obs=-1"),
                           (solve, dict(D=-1), b"D=-1"),
                           (apply_, dict(K=0), b"K=0"), (apply_, dict(K=65), b"K=65"), (apply_, dict(S=-1), b"S=-1")):
        rc = call(**kw)
        assert rc < 0 and word in lib.mff_last_error(), (kw, lib.mff_last_error())
        with pytest.raises(_lib.MffError):
            _lib.check(rc, "mff_xs_orth")
    # nothing to do
    assert sums(D=0) == 0 and gram(D=0) == 0 and solve(D=0) == 0 and apply_(D=0) == 0 and apply_(S=0) == 0


@pytest.mark.parametrize("K,n", [(1, 50), (2, 40), (5, 300), (16, 400), (58, 500)])
def test_symmetric_is_the_polar_factor(K, n):
    """The Loewdin set of the standardised columns z is sqrt(n - 1) times the orthogonal polar
    factor P Q^T of z = P S Q^T."""
    X = _day(10 + K, n, K)
    r = ref.orth_day(X, "symmetric")
    assert r["status"] == 0 and r["cond"] < 1e3
    c = X - X.mean(axis=0)
    z = c / c.std(axis=0, ddof=1)
    P, _, Qt = np.linalg.svd(z, full_matrices=False)
    np.testing.assert_allclose(r["out"], np.sqrt(n - 1) * P @ Qt, **TOL)
    assert np.array_equal(np.argsort(r["eig"], kind="stable"), np.arange(K))
    np.testing.assert_allclose(r["keep"], [np.corrcoef(r["out"][:, j], X[:, j])[0, 1] for j in range(K)], **TOL)
    np.testing.assert_allclose(np.cov(r["out"].T, ddof=1).reshape(K, K), np.eye(K), **TOL)


@pytest.mark.parametrize("K,n", [(1, 50), (2, 40), (5, 300), (16, 400), (58, 500)])
def test_schmidt_is_the_sign_fixed_qr(K, n):
    X = _day(20 + K, n, K)
    r = ref.orth_day(X, "schmidt")
    assert r["status"] == 0
    c = X - X.mean(axis=0)
    z = c / c.std(axis=0, ddof=1)
    Q, Rr = np.linalg.qr(z)
    Q = Q * np.sign(np.diag(Rr))
    np.testing.assert_allclose(r["out"], np.sqrt(n - 1) * Q, **TOL)
    assert (r["T"][np.tril_indices(K, -1)] == 0).all()
    np.testing.assert_allclose(r["out"][:, 0], z[:, 0], **TOL)
    np.testing.assert_allclose(r["keep"], [np.corrcoef(r["out"][:, j], X[:, j])[0, 1] for j in range(K)], **TOL)
    if K > 1:   # the last column: the standardised OLS residual on an intercept and the rows before it
        Z = np.concatenate([np.ones((n, 1)), X[:, :-1]], axis=1)
        e = X[:, -1] - Z @ np.linalg.lstsq(Z, X[:, -1], rcond=None)[0]
        np.testing.assert_allclose(r["out"][:, -1], e / e.std(ddof=1), rtol=1e-9, atol=1e-9)
    sym = ref.orth_day(X, "symmetric")
    np.testing.assert_allclose(r["eig"], sym["eig"], **TOL)   # the eigenvalues do not depend on the method


def test_one_and_two_factor_identities():
    X = _day(3, 80, 1)
    for method in ref.METHODS:
        r = ref.orth_day(X, method)
        np.testing.assert_allclose(r["out"][:, 0], (X[:, 0] - X[:, 0].mean()) / X[:, 0].std(ddof=1), **TOL)
        assert r["T"].tolist() == [[1.0]] and r["keep"].tolist() == [1.0] and r["eig"].tolist() == [1.0]
    X = _day(4, 200, 2)
    rho = np.corrcoef(X.T)[0, 1]
    assert 0.1 < abs(rho) < 0.9
    s = np.sqrt(1.0 - rho * rho)
    np.testing.assert_allclose(ref.orth_day(X, "symmetric")["keep"], np.full(2, np.sqrt((1.0 + s) / 2.0)), **TOL)
    np.testing.assert_allclose(ref.orth_day(X, "schmidt")["keep"], [1.0, s], **TOL)
    np.testing.assert_allclose(ref.orth_day(X, "schmidt")["eig"], [1.0 - abs(rho), 1.0 + abs(rho)], **TOL)


@pytest.mark.parametrize("method", ref.METHODS)
def test_status_rules(method):
    K = 4
    X = _day(5, 60, K)
    for n, status in ((K, 1), (K + 1, 0), (60, 0)):
        r = ref.orthogonalize(*_dense(X[:n]), method=method)
        assert r["n"][0] == n and r["status"][0] == status
        assert np.isnan(r["T"]).all() == (status != 0) and np.isnan(r["eig"]).all() == (status != 0)
    assert ref.orthogonalize(*_dense(X), method=method, min_obs=60)["status"][0] == 0
    r = ref.orthogonalize(*_dense(X), method=method, min_obs=61)
    assert r["status"][0] == 1 and r["n"][0] == 60 and (r["state"] == NULL).all() and (r["val"] == 0).all()
    const, dup, comb = X.copy(), X.copy(), X.copy()
    const[:, 1] = 2.5
    dup[:, 3] = dup[:, 0]
    comb[:, 2] = comb[:, 0] + comb[:, 1]
    for bad in (const, dup, comb):
        r = ref.orthogonalize(*_dense(bad), method=method)
        assert r["status"][0] == 2 and r["n"][0] == 60
        assert np.isnan(r["T"]).all() and np.isnan(r["eig"]).all() and np.isnan(r["keep"]).all()
        assert (r["state"] == NULL).all() and (r["val"] == 0).all()


def test_states_and_listwise_set():
    X = _day(6, 30, 3)
    x, xs = _dense(X)
    xs[0, 0, 0] = ABSENT
    xs[1, 0, 1] = NULL
    x[2, 0, 2] = np.nan
    x[0, 0, 3] = -np.inf
    r = ref.orthogonalize(x, xs)
    assert r["n"][0] == 26 and r["status"][0] == 0
    assert r["state"][:, 0, :5].tolist() == [[ABSENT, NULL, NULL, NULL, VALUE], [NULL, NULL, NULL, NULL, VALUE],
                                             [NULL, NULL, NULL, NULL, VALUE]]
    assert (r["val"][:, 0, :4] == 0).all()
    alone = ref.orth_day(X[4:])
    np.testing.assert_allclose(r["val"][:, 0, 4:].T, alone["out"], **TOL)
    np.testing.assert_allclose(r["T"][0], alone["T"], **TOL)
