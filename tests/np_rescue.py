"""numpy restatement of the rescue gate's rule (srukf_rescue_gate / srukf_images_rescue_gate), given the measurement prediction from the posterior.

A frame has candidates when n_active >= 2 and 0 < n_low < n_active (CSLAM::rescueHighInnovationInliers' condition); its candidates are the landmarks in A
(matched and visible) that are no low-innovation inliers.  A candidate is rescued when it is visible from the posterior, Si'[0] != 0, Si'[3] != 0 and
y = Si'^-T (z - h'), formed by forward substitution, has y0^2 + y1^2 < chi2 — strictly (dataAssociation's gate, SLAM.cpp:1977).
"""
import numpy as np

CHI2 = 5.99146454710798                                          # CHI2INV_TABLE(0, 2)
CANDIDATE, RESCUED = 1, 2


def frame_has_candidates(active, low):
    active, low = np.asarray(active) != 0, np.asarray(low) != 0
    n_active, n_low = int(active.sum()), int((active & low).sum())
    return n_active >= 2 and 0 < n_low < n_active


def gate(z, active, low, h2, Si2, vis2, chi2=CHI2):
    """flags[N] (bit 0 candidate, bit 1 rescued) and dist[N] = y0^2 + y1^2 (0 where the test was not formed).  Si2: [N][4] or [N][2][2], upper triangular."""
    z, h2 = np.asarray(z, dtype=np.float64).reshape(-1, 2), np.asarray(h2, dtype=np.float64).reshape(-1, 2)
    Si2 = np.asarray(Si2, dtype=np.float64).reshape(-1, 4)
    active, low, vis2 = np.asarray(active) != 0, np.asarray(low) != 0, np.asarray(vis2) != 0
    N = len(active)
    flags, dist = np.zeros(N, dtype=np.int32), np.zeros(N)
    if not frame_has_candidates(active, low):
        return flags, dist
    for k in range(N):
        if not active[k] or low[k]:
            continue
        flags[k] = CANDIDATE
        s00, s01, s11 = Si2[k, 0], Si2[k, 1], Si2[k, 3]
        if not vis2[k] or s00 == 0.0 or s11 == 0.0:
            continue
        v0, v1 = z[k, 0] - h2[k, 0], z[k, 1] - h2[k, 1]
        y0 = v0 / s00
        y1 = (v1 - s01 * y0) / s11
        dist[k] = y0 * y0 + y1 * y1
        if dist[k] < chi2:
            flags[k] |= RESCUED
    return flags, dist
