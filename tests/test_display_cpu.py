"""tests/np_display.py (the restatement of get3DdisplayInformation, calculateEigenvaluesAndEigenvectors and matrix2Quaternion, SLAM.cpp:2791-2948, that the GPU
tests hold k_lm_ellipsoid to bit for bit) against numpy and against the outcomes the reference's code fixes for special inputs.  No GPU.

BOUND: V diag(values) V^T reconstructs the input, and the values equal numpy.linalg.eigvalsh's as sets, to 1e-12 of the largest absolute entry (largest absolute
difference / largest absolute entry).  3 x 3 in fp64, at most 271 plane rotations (ten at most over these inputs), each a handful of roundings of 1.1e-16, and a
stopping rule that leaves off-diagonal entries below EPSILON = 1e-13 ABSOLUTE: the inputs therefore have their largest eigenvalue in [1, 100] (the stopping rule
knows no scale; a matrix of entries ~1e-6 is "diagonal" to it at a relative 1e-7)."""
import math

import numpy as np
import pytest

import np_display as D

EPS = 1e-13                                                      # srukf_params.epsilon's default (EPSILON, SLAM.cpp:44)
BOUND = 1e-12
I3 = [1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0]
# a rank-one v v^T whose Jacobi iteration leaves a negative rounding residue on the diagonal (found by running the restatement over seeded draws)
RANK_ONE_V = [0.345584192064786, 0.8216181435011584, 0.33043707618338714]


def spd(seed):
    """Seeded symmetric positive definite 3 x 3: random orthogonal basis, the largest eigenvalue in [1, 100], the others down to 1e-6 (condition number up to 1e8)."""
    rng = np.random.default_rng(seed)
    Q, _ = np.linalg.qr(rng.standard_normal((3, 3)))
    lam = 10.0 ** rng.uniform(-6.0, 2.0, 3)
    lam[rng.integers(3)] = 10.0 ** rng.uniform(0.0, 2.0)
    A = (Q * lam) @ Q.T
    return 0.5 * (A + A.T)


def quat_to_matrix(q):
    r, x, y, z = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * r), 2 * (x * z + y * r)],
                     [2 * (x * y + z * r), 1 - 2 * (x * x + z * z), 2 * (y * z - x * r)],
                     [2 * (x * z - y * r), 2 * (y * z + x * r), 1 - 2 * (x * x + y * y)]])


def check_decomposition(A):
    values, V, rot = D.jacobi3(A.ravel().tolist(), EPS)
    Vm, scale = np.array(V).reshape(3, 3), np.abs(A).max()
    assert 0 <= rot <= 271
    rec = np.abs(Vm @ np.diag(values) @ Vm.T - A).max() / scale
    eig = np.abs(np.sort(values) - np.linalg.eigvalsh(A)).max() / scale
    orth = np.abs(Vm.T @ Vm - np.eye(3)).max()
    assert rec <= BOUND and eig <= BOUND and orth <= BOUND, (rec, eig, orth, rot)
    return rec, eig, rot


def test_seeded_spd_reconstruction_and_eigenvalues():
    worst_rec = worst_eig = 0.0
    conds, rots = [], []
    for seed in range(200):
        A = spd(seed)
        lam = np.linalg.eigvalsh(A)
        conds.append(lam[-1] / lam[0])
        rec, eig, rot = check_decomposition(A)
        worst_rec, worst_eig = max(worst_rec, rec), max(worst_eig, eig)
        rots.append(rot)
    print(f"200 SPD inputs: cond {min(conds):.2e} .. {max(conds):.2e}, rotations {min(rots)} .. {max(rots)}, worst reconstruction {worst_rec:.2e}, eigenvalues {worst_eig:.2e}")
    assert max(conds) > 1e7 and max(conds) <= 1e8 * (1 + 1e-6)


def test_trace_branch_is_the_only_one_jacobi_reaches_over_the_seeded_inputs():
    """The accumulated V of the 200 inputs has a positive trace every time (so has every one of 10^5 such draws and of 6 * 10^4 targeted ones — no
    seed is kept for the GPU test; the other three branches are reached through matrix2quaternion directly, below)."""
    for seed in range(200):
        _, V, _ = D.jacobi3(spd(seed).ravel().tolist(), EPS)
        assert D.quaternion_branch(V) == 0


def test_diagonal_input_needs_no_rotation():
    axis, sigma, rot = D.ellipsoid([4.0, 0.0, 0.0, 0.0, 9.0, 0.0, 0.0, 0.0, 0.25], EPS)
    values, V, _ = D.jacobi3([4.0, 0.0, 0.0, 0.0, 9.0, 0.0, 0.0, 0.0, 0.25], EPS)
    assert rot == 0 and V == I3 and axis == [1.0, 0.0, 0.0, 0.0] and sigma == [2.0, 3.0, 0.5] and values == [4.0, 9.0, 0.25]
    # off-diagonals below EPSILON count as zero: nothing is rotated, the diagonal is taken as it stands
    _, _, rot = D.ellipsoid([4.0, 9e-14, 0.0, 9e-14, 9.0, -9e-14, 0.0, -9e-14, 0.25], EPS)
    assert rot == 0


def first_pivots(cov, k=1):
    trace = []
    D.jacobi3(cov, EPS, trace)
    return trace[:k]


def test_equal_off_diagonals_the_first_in_scan_order_wins():
    # scan order (1,0), (2,0), (2,1) with a strict >
    assert first_pivots([2.0, 0.5, 0.5, 0.5, 3.0, 0.5, 0.5, 0.5, 4.0]) == [(1, 0)]
    assert first_pivots([2.0, 0.5, -0.5, 0.5, 3.0, 0.5, -0.5, 0.5, 4.0]) == [(1, 0)]            # (magnitudes)
    assert first_pivots([2.0, 0.25, 0.5, 0.25, 3.0, -0.5, 0.5, -0.5, 4.0]) == [(2, 0)]
    assert first_pivots([2.0, 0.25, 0.5, 0.25, 3.0, 0.75, 0.5, 0.75, 4.0]) == [(2, 1)]
    # only the entries BELOW the diagonal are scanned: a large entry above it is not a pivot
    assert first_pivots([2.0, 9.0, 0.0, 0.125, 3.0, 0.0, 0.25, 0.0, 4.0]) == [(2, 0)]
    check_decomposition(np.array([2.0, 0.5, 0.5, 0.5, 3.0, 0.5, 0.5, 0.5, 4.0]).reshape(3, 3))


def test_sign_flip_when_aqq_is_below_app():
    """p = 1, q = 0: y = (a00 - a11) / 2.  y < 0 flips omega, so sin(phi) takes the sign of -x = a10 instead of x: either way the larger diagonal entry stays where
    the larger one was (the rotation angle stays within 45 degrees)."""
    for a00, a11, sn_sign in ((1.0, 2.0, 1.0), (2.0, 1.0, -1.0)):
        values, V, rot = D.jacobi3([a00, 0.5, 0.0, 0.5, a11, 0.0, 0.0, 0.0, 3.0], EPS)
        lo, hi = 1.5 - math.sqrt(0.5), 1.5 + math.sqrt(0.5)
        assert rot == 1                                          # one rotation annihilates the only off-diagonal pair exactly (it is set to 0.0)
        assert V[1] != 0.0 and math.copysign(1.0, V[1]) == sn_sign and V[3] == -V[1] and V[0] == V[4] and V[8] == 1.0      # V[0][1] = sin(phi), V[1][0] = -sin(phi)
        assert abs(V[1]) < math.sqrt(0.5)
        want = [lo, hi, 3.0] if a00 < a11 else [hi, lo, 3.0]
        assert max(abs(v - w) for v, w in zip(values, want)) < 1e-15
    # negative off-diagonal: the mirror images
    _, V, _ = D.jacobi3([1.0, -0.5, 0.0, -0.5, 2.0, 0.0, 0.0, 0.0, 3.0], EPS)
    assert V[1] < 0.0


def test_nan_input_returns_at_once():
    n = float("nan")
    # a NaN below the diagonal never wins the pivot scan: with nothing else off the diagonal the iteration stops in its first pass
    axis, sigma, rot = D.ellipsoid([1.0, n, 0.0, n, 2.0, 0.0, 0.0, 0.0, 3.0], EPS)
    assert rot == 0 and axis == [1.0, 0.0, 0.0, 0.0] and sigma == [1.0, math.sqrt(2.0), math.sqrt(3.0)]
    axis, sigma, rot = D.ellipsoid([n] * 9, EPS)
    assert rot == 0 and axis == [1.0, 0.0, 0.0, 0.0] and all(s != s for s in sigma)
    # ... and the other entries are still rotated away (the NaN entry sits in column 0 of row 2: the rotation in the (2, 1) plane turns it into row 1's too)
    axis, sigma, rot = D.ellipsoid([1.0, 0.1, 0.0, 0.1, 2.0, 0.2, n, 0.2, 3.0], EPS)
    assert rot == 1 and sigma[0] == 1.0 and all(s == s for s in sigma) and all(a == a for a in axis)
    # a NaN on the diagonal of the pivot's plane poisons the rotation; the iteration still ends (every off-diagonal it leaves is 0 or NaN)
    axis, sigma, rot = D.ellipsoid([n, 0.5, 0.0, 0.5, 2.0, 0.0, 0.0, 0.0, 3.0], EPS)
    assert rot == 1 and all(a != a for a in axis) and sigma[0] != sigma[0] and sigma[1] != sigma[1] and sigma[2] == math.sqrt(3.0)


def test_rank_one_input_may_leave_a_negative_eigenvalue():
    """v v^T: two eigenvalues are zero up to rounding, and rounding may leave one of them below zero — sigma is NaN there, as on the host (sqrt of a negative).
    For this v it is position 2 (-2.8e-17); position 0 comes out as exactly 0."""
    A = np.outer(RANK_ONE_V, RANK_ONE_V)
    values, V, rot = D.jacobi3(A.ravel().tolist(), EPS)
    axis, sigma, rot2 = D.ellipsoid(A.ravel().tolist(), EPS)
    assert rot == rot2 == 2
    assert values[0] == 0.0 and -1e-16 < values[2] < 0.0 and abs(values[1] - float(np.dot(RANK_ONE_V, RANK_ONE_V))) < 1e-15
    assert sigma[0] == 0.0 and sigma[2] != sigma[2] and sigma[1] == math.sqrt(values[1])
    assert all(a == a for a in axis) and abs(math.sqrt(sum(a * a for a in axis)) - 1.0) < 1e-15
    check_decomposition(A)


def rotation(axis, angle):
    a = np.asarray(axis, dtype=float); a /= np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + math.sin(angle) * K + (1 - math.cos(angle)) * (K @ K)


@pytest.mark.parametrize("branch,axis,angle", [(0, (1.0, 2.0, 3.0), 0.7), (0, (0.0, 0.0, 1.0), 1.5),
                                               (1, (1.0, 0.1, -0.2), 2.9), (2, (0.1, 1.0, 0.2), 3.0), (3, (-0.2, 0.1, 1.0), 2.8),
                                               (1, (1.0, 0.0, 0.0), math.pi), (2, (0.0, 1.0, 0.0), math.pi), (3, (0.0, 0.0, 1.0), math.pi)])
def test_quaternion_branches(branch, axis, angle):
    """Each of matrix2Quaternion's four branches, with the reference's element pairing: the trace branch takes (m23 - m32, m31 - m13, m12 - m21), which is the
    quaternion of the TRANSPOSE; the three others pair their off-diagonal sums symmetrically and take r from (m32 - m23, m13 - m31, m21 - m12): the matrix itself."""
    R = rotation(axis, angle)
    V = R.ravel().tolist()
    assert D.quaternion_branch(V) == branch
    q = D.matrix2quaternion(V)
    assert abs(math.sqrt(sum(v * v for v in q)) - 1.0) < 1e-14
    want = R.T if branch == 0 else R
    assert np.abs(quat_to_matrix(q) - want).max() < 1e-13
    assert q[branch] > 0.0                                       # the branch's own component is the square root: r, x, y or z
