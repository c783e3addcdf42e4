"""get3DdisplayInformation, calculateEigenvaluesAndEigenvectors and matrix2Quaternion (SLAM.cpp:2791-2948) restated on Python floats (IEEE binary64, every
operation rounded once, no contraction): what k_lm_ellipsoid and the host facade compute, bit for bit.

The iteration limit is the facade's: at most 30 n^2 + 1 passes (each pass either stops or rotates), rot = -1 when it runs out."""
import math

NAN = float("nan")


def _sqrt(x):
    """C's sqrt: NaN for a negative or NaN argument (math.sqrt raises), -0.0 for -0.0."""
    if x != x or x < 0.0:
        return NAN
    return math.sqrt(x)


def _div(a, b):
    """C's a / b for finite-or-not binary64 operands (Python raises on a zero divisor)."""
    if b == 0.0 and b == b:
        if a != a or a == 0.0:
            return NAN
        return math.copysign(math.inf, a) * math.copysign(1.0, b)
    return a / b


def jacobi3(cov, eps, trace=None):
    """cov: 9 floats (row-major 3 x 3, all nine entries are used; trace: a list that receives the pivot (p, q) of every rotation).  Returns (values[3] = the diagonal as the rotations left it, V[9] row-major with the
    eigenvector of values[j] in column j, rot = plane rotations applied or -1)."""
    n = 3
    A = [float(v) for v in cov]
    V = [1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0]
    rot = -1
    for it in range(30 * n * n + 1):
        p = q = -1
        big = 0.0
        for i in range(1, n):
            for j in range(i):
                if abs(A[n * i + j]) > big:                    # strict: the first largest in scan order wins, a NaN never does
                    big = abs(A[n * i + j]); p = i; q = j
        if big < eps or p < 0:
            rot = it
            break
        if trace is not None:
            trace.append((p, q))
        x = -A[n * p + q]
        y = 0.5 * (A[n * q + q] - A[n * p + p])
        omega = _div(x, _sqrt(x * x + y * y))
        if y < 0.0:
            omega = -omega
        sn = _div(omega, _sqrt(2.0 * (1.0 + _sqrt(1.0 - omega * omega))))
        cn = _sqrt(1.0 - sn * sn)
        app, aqq, apq = A[n * p + p], A[n * q + q], A[n * p + q]
        A[n * p + p] = app * cn * cn + aqq * sn * sn + apq * omega
        A[n * q + q] = app * sn * sn + aqq * cn * cn - apq * omega
        A[n * p + q] = 0.0
        A[n * q + p] = 0.0
        for j in range(n):
            if j != p and j != q:
                ap, aq = A[n * p + j], A[n * q + j]
                A[n * p + j] = ap * cn + aq * sn
                A[n * q + j] = -ap * sn + aq * cn
        for i in range(n):
            if i != p and i != q:
                ap, aq = A[n * i + p], A[n * i + q]
                A[n * i + p] = ap * cn + aq * sn
                A[n * i + q] = -ap * sn + aq * cn
        for i in range(n):
            vp, vq = V[n * i + p], V[n * i + q]
            V[n * i + p] = vp * cn + vq * sn
            V[n * i + q] = -vp * sn + vq * cn
    return [A[0], A[4], A[8]], V, rot


def quaternion_branch(V):
    """Which of matrix2Quaternion's four branches V takes: 0 trace, 1 m11, 2 m22, 3 m33."""
    m11, m22, m33 = V[0], V[4], V[8]
    if m11 + m22 + m33 > 0.0:
        return 0
    if m11 > m22 and m11 > m33:
        return 1
    return 2 if m22 > m33 else 3


def matrix2quaternion(V):
    """(r, x, y, z) of the rotation matrix V[9], element pairing as in the reference."""
    m11, m12, m13, m21, m22, m23, m31, m32, m33 = [float(v) for v in V]
    tr = m11 + m22 + m33
    if tr > 0.0:
        t = _div(0.5, _sqrt(tr + 1))
        return [_div(0.25, t), (m23 - m32) * t, (m31 - m13) * t, (m12 - m21) * t]
    if m11 > m22 and m11 > m33:
        t = 2.0 * _sqrt(1.0 + m11 - m22 - m33)
        return [_div(m32 - m23, t), 0.25 * t, _div(m12 + m21, t), _div(m13 + m31, t)]
    if m22 > m33:
        t = 2.0 * _sqrt(1.0 + m22 - m11 - m33)
        return [_div(m13 - m31, t), _div(m12 + m21, t), 0.25 * t, _div(m23 + m32, t)]
    t = 2.0 * _sqrt(1.0 + m33 - m11 - m22)
    return [_div(m21 - m12, t), _div(m13 + m31, t), _div(m23 + m32, t), 0.25 * t]


def ellipsoid(cov, eps):
    """(axis[4] = (r, x, y, z), sigma[3], rot) of one 3 x 3 covariance."""
    values, V, rot = jacobi3(cov, eps)
    return matrix2quaternion(V), [_sqrt(v) for v in values], rot
