"""numpy restatement of the loop-point calls (include/srukf.h: srukf_get_landmark_record / srukf_insert_landmarks).

chol6: the record's factor of a landmark's marginal 6x6 block, in the order the device computes it (scalar fp64, no contraction): the GPU tests
hold srukf_get_landmark_record to it bit for bit.  place: where srukf_insert_landmarks puts L landmarks (copies only, no arithmetic)."""
import math

import numpy as np


def chol6(P66, eps=1e-13):
    """Upper S with S^T S = P66: d_j = max(eps, P_jj - sum_{m<j} S_mj^2), S_jj = sqrt(d_j), S_ji = (P_ji - sum_{m<j} S_mj S_mi) / S_jj (i > j),
    sums in ascending m, zeros below the diagonal."""
    P = [[float(v) for v in row] for row in np.asarray(P66, dtype=np.float64)]
    S = [[0.0] * 6 for _ in range(6)]
    for j in range(6):
        s = 0.0
        for m in range(j):
            s += S[m][j] * S[m][j]
        d = P[j][j] - s
        d = d if d > eps else eps
        sjj = math.sqrt(d)
        S[j][j] = sjj
        for i in range(j + 1, 6):
            q = 0.0
            for m in range(j):
                q += S[m][j] * S[m][i]
            S[j][i] = (P[j][i] - q) / sjj
    return np.array(S, dtype=np.float64)


def index_map(N, k_new, L):
    """src[r'] for every state index r' of the grown state (n' = 6 (N + L) + 4): the old index, or -1 for the rows of the new landmarks, which sit
    at landmark positions [N - k_new, N - k_new + L)."""
    p6, L6, n2 = 6 * (N - k_new), 6 * L, 6 * (N + L) + 4
    r = np.arange(n2)
    return np.where(r < p6, r, np.where(r < p6 + L6, -1, r - L6))


def place(X, S, k_new, X6, S66):
    """(X', S') of srukf_insert_landmarks: old rows / columns at their new indices, S66[j] on the diagonal block of new landmark j, zero elsewhere."""
    X = np.asarray(X, dtype=np.float64)
    S = np.asarray(S, dtype=np.float64)
    X6 = np.asarray(X6, dtype=np.float64).reshape(-1, 6)
    S66 = np.asarray(S66, dtype=np.float64).reshape(-1, 6, 6)
    N, L = (X.shape[0] - 4) // 6, X6.shape[0]
    src = index_map(N, k_new, L)
    n2 = src.shape[0]
    old = np.nonzero(src >= 0)[0]
    X2 = np.zeros(n2)
    X2[old] = X[src[old]]
    S2 = np.zeros((n2, n2))
    S2[np.ix_(old, old)] = S[np.ix_(src[old], src[old])]
    p6 = 6 * (N - k_new)
    for j in range(L):
        a = p6 + 6 * j
        X2[a:a + 6] = X6[j]
        S2[a:a + 6, a:a + 6] = S66[j]
    return X2, S2


def perm_matrix(N, k_new, L):
    """Pi with X' = Pi (X (+) X6_0 (+) ...): the grown state's row r' takes row src[r'] of the stacked [old state | new landmarks]."""
    src = index_map(N, k_new, L)
    n, n2 = 6 * N + 4, src.shape[0]
    Pi = np.zeros((n2, n2))
    new = np.nonzero(src < 0)[0]
    for r in range(n2):
        Pi[r, src[r] if src[r] >= 0 else n + int(np.searchsorted(new, r))] = 1.0
    return Pi
