"""CPU tests of the loop-point calls (srukf_get_landmark_record / srukf_insert_landmarks): the library exports them, the header declares them,
Filter binds them, and the numpy restatement (tests/np_loop.py) that the GPU tests hold the device to is right: S66^T S66 = P66 and
P' = Pi (P (+) S66_0^T S66_0 (+) ...) Pi^T."""
import os
import re

import numpy as np
import pytest
from scipy.linalg import block_diag

import np_loop as LP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("srukf_get_landmark_record", "srukf_insert_landmarks")


def _spd(rng, n, cond=1e4):
    Q, _ = np.linalg.qr(rng.normal(size=(n, n)))
    return (Q * np.geomspace(1.0, 1.0 / cond, n)) @ Q.T


def _upper_factor(rng, n):
    S = np.triu(rng.normal(size=(n, n)))
    S[np.diag_indices(n)] = np.abs(S[np.diag_indices(n)]) + 0.5
    return S


def test_library_exports_and_header_declares_the_loop_calls(pkg):
    lib = pkg.srukf.load_library()
    txt = open(os.path.join(ROOT, "include", "srukf.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for name in NEW:
        assert hasattr(lib, name), name
        assert re.search(r"\bint\s+" + name + r"\s*\(", txt), name
        assert name in pkg.srukf.EXPORTS


def test_filter_has_the_methods(pkg):
    for m in ("get_landmark_record", "insert_landmarks"):
        assert callable(getattr(pkg.srukf.Filter, m, None)), m


@pytest.mark.parametrize("seed", range(6))
def test_chol6_factors_the_block(seed):
    rng = np.random.default_rng(seed)
    P = _spd(rng, 6, cond=10.0 ** (seed + 1))
    S = LP.chol6(P)
    assert np.all(np.tril(S, -1) == 0.0) and np.all(np.diag(S) > 0)
    np.testing.assert_allclose(S.T @ S, P, rtol=0, atol=1e-14 * np.abs(P).max() * 10 ** seed)
    np.testing.assert_allclose(S, np.linalg.cholesky(P).T, rtol=1e-8 * 10 ** seed, atol=1e-14)


def test_chol6_clamps_null_pivots_to_epsilon():
    P = np.zeros((6, 6))
    P[:3, :3] = np.diag([4.0, 9.0, 1.0])            # rank 3: the other three pivots are exactly 0
    S = LP.chol6(P, eps=1e-13)
    np.testing.assert_array_equal(np.diag(S), [2.0, 3.0, 1.0] + [np.sqrt(1e-13)] * 3)
    np.testing.assert_array_equal(S[:3, 3:], 0.0)


@pytest.mark.parametrize("N,k_new,L", [(0, 0, 1), (0, 0, 3), (5, 0, 2), (8, 3, 1), (8, 3, 3), (12, 12, 2)])
def test_place_is_the_permuted_direct_sum(N, k_new, L):
    rng = np.random.default_rng(100 * N + 10 * k_new + L)
    n = 6 * N + 4
    X, S = rng.normal(size=n), _upper_factor(rng, n)
    X6 = rng.normal(size=(L, 6))
    S66 = np.stack([_upper_factor(rng, 6) for _ in range(L)])
    X2, S2 = LP.place(X, S, k_new, X6, S66)
    assert X2.shape == (n + 6 * L,) and np.all(np.tril(S2, -1) == 0.0)
    Pi = LP.perm_matrix(N, k_new, L)
    np.testing.assert_array_equal(X2, Pi @ np.concatenate([X, X6.ravel()]))
    P = S.T @ S
    direct = block_diag(P, *[s.T @ s for s in S66])
    np.testing.assert_allclose(S2.T @ S2, Pi @ direct @ Pi.T, rtol=0, atol=1e-12 * np.abs(direct).max())
    # the armed landmarks and the robot block stay last, the new ones sit right in front of them
    p6 = 6 * (N - k_new)
    np.testing.assert_array_equal(X2[-(6 * k_new + 4):], X[p6:])
    np.testing.assert_array_equal(X2[p6:p6 + 6 * L], X6.ravel())
    np.testing.assert_array_equal(S2[:p6, p6:p6 + 6 * L], 0.0)
    np.testing.assert_array_equal(S2[p6:p6 + 6 * L, p6 + 6 * L:], 0.0)
