"""Generates the golden fixtures in tests/golden/ from the CPU oracle (oracle/srukf_oracle.c).

The reference ships no golden vectors for this path and cannot be compiled here,
so these vectors pin the ORACLE (and, through it, the HIP path) against regressions; the oracle
itself is cross-checked against the independent numpy restatement in tests/np_filter.py and
cv-monoslam_amd/synth.py.  Run from the repo root:  python tests/golden/make_golden.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402
from oracle import oracle as O  # noqa: E402

pkg = ge.load_package()
synth = pkg.synth
OUT = os.path.dirname(os.path.abspath(__file__))


def g1_weights():
    rows = []
    for wt in (0, 1, 2):
        for Na in (9, 129, 309, 1209, 3009):
            w = O.sample_parameter(Na, wt)
            rows.append([wt, Na] + [w[k] for k in ("wm0", "wc0", "wi", "wi_sr", "gamma", "wm0_sr", "wc0_sr")])
    return np.array(rows)


def g2_projection():
    p = synth.default_params()
    rng = np.random.default_rng(11)
    sc = synth.make_scene(24, 1, seed=5, p=synth.scene_params())
    feat = sc["truth"].copy()
    feat[:, :3] = rng.normal(0, 0.02, (24, 3))
    pos = rng.normal(0, 0.05, (24, 3))
    psi = rng.normal(0, 0.4, 24)
    err = rng.normal(0, 2.0, (24, 2))
    # force the special branches: Hlr.z == 0, outside the 10-px border, far outside the image
    feat[0, 2] = 0.0; feat[0, 3] = np.pi / 2; feat[0, 4] = 0.0; pos[0, 2] = 0.0   # cos(phi)cos(theta)/rho ~ 6e-17 != 0: stays a huge ratio
    feat[1, 3] = 1.2                                                               # projects outside -> zeroed by the border test
    feat[2, 4] = -1.3
    feat[3, 5] = 1e-3                                                              # very far point
    uv = O.project(p, feat, pos, psi, err, early_exit=0)
    return dict(feat=feat, pos=pos, psi=psi, err=err, uv=uv)


def g3_gmw():
    rng = np.random.default_rng(3)
    out = {}
    A = rng.normal(size=(8, 8)); spd = A @ A.T + 0.5 * np.eye(8)
    B = rng.integers(-3, 4, size=(10, 4)).astype(float); psd = B @ B.T   # integer entries: null pivots ~1e-16 -> EPSILON clamp
    C = rng.normal(size=(6, 6)); ind = C + C.T
    for name, G in (("spd", spd), ("psd", psd), ("ind", ind)):
        S, D, L, ce, ct = O.gmw(G)
        out[name + "_G"], out[name + "_S"], out[name + "_D"], out[name + "_L"] = G, S, D, L
        out[name + "_clamps"] = np.array([ce, ct])
    return out


def g4_joint_init():
    p = synth.default_params()
    out = {}
    for K in (1, 2, 8):
        sc = synth.make_scene(K, 1, seed=20 + K, p=synth.scene_params())
        X, S = O.joint_init(p, np.zeros(4), np.diag([.02, .02, .005, .02]), sc["uv0"])
        out[f"K{K}_uv"], out[f"K{K}_X"], out[f"K{K}_S"] = sc["uv0"], X, S
    return out


def g5_frame():
    p = synth.scene_params()
    N = 8
    sc = synth.make_scene(N, 1, seed=31, p=p)
    o = O.Oracle(N, p); o.set_state(sc["X0"], sc["S0"])
    out = dict(X0=sc["X0"], S0=sc["S0"], odo=sc["odo"], z=sc["z"], matched=sc["matched"])
    o.predict_motion(sc["odo"][0], sc["odo"][1])
    out["X_motion"], S = o.get_state(); out["P_motion"] = S.T @ S
    h, Si, vis = o.predict_measurement()
    out["h"], out["Si"], out["vis"] = h, Si, vis
    o.update(sc["z"][0], sc["matched"][0], 1, 0, 0)
    out["X_post"], S = o.get_state(); out["P_post"] = S.T @ S
    return out


def g6_trajectory():
    p = synth.scene_params()
    N, F = 20, 50
    sc = synth.make_scene(N, F, seed=42, p=p)
    o = O.Oracle(N, p); o.set_state(sc["X0"], sc["S0"])
    traj_seq = o.run_frames(sc["odo"], sc["z"], sc["matched"], O.Oracle.SEQUENTIAL)
    Xs, Ss = o.get_state()
    o2 = O.Oracle(N, p); o2.set_state(sc["X0"], sc["S0"])
    traj_bat = o2.run_frames(sc["odo"], sc["z"], sc["matched"], O.Oracle.BATCHED)
    return dict(N=N, F=F, seed=42, traj_sequential=traj_seq, traj_batched=traj_bat, X_final=Xs, P_final_diag=np.diag(Ss.T @ Ss),
                clamps_seq=np.array(list(o.clamp_stats().values())), clamps_bat=np.array(list(o2.clamp_stats().values())))


def g7_sequential(N, F, seed):
    """The reference's own structure (2M refactors per frame, SLAM.cpp:2066-2095, 2116-2154) at the benchmark sizes: what the
    BATCHED device path (one refactor per frame) is held to.  N = 200: one frame is ~3 minutes of single-thread CPU.
    The full P (11.6 MB at N = 200) is not stored: the state, diag P, the robot columns of P, every landmark's 6 x 6 block
    and P V for 16 seeded +-1 probe vectors are (an error matrix E shows in E V with |E V| >= |E|max for almost every V)."""
    p = synth.scene_params()
    sc = synth.make_scene(N, F, seed=seed, p=p)
    o = O.Oracle(N, p); o.set_state(sc["X0"], sc["S0"])
    traj = o.run_frames(sc["odo"], sc["z"], sc["matched"], O.Oracle.SEQUENTIAL)
    X, S = o.get_state()
    P = S.T @ S
    n = 6 * N + 4
    V = np.random.default_rng(700 + N).choice([-1.0, 1.0], size=(n, 16))
    blocks = np.stack([P[6 * k:6 * k + 6, 6 * k:6 * k + 6] for k in range(N)])
    return dict(N=N, F=F, seed=seed, traj=traj, X=X, P_diag=np.diag(P).copy(), P_robot_cols=P[:, n - 4:].copy(), P_blocks=blocks, V=V, PV=P @ V,
                P_absmax=np.abs(P).max(), clamps=np.array(list(o.clamp_stats().values())))


def g8_match_pattern(N, F, seed):
    """Association outcome of the g8 sequence: every frame a third of the landmarks unmatched (which third rotates), frame 7 with NO match at all
    (KalmanUpdate returns at once, SLAM.cpp:2050-2051), frame 19 with a single match."""
    rng = np.random.default_rng(seed)
    m = np.ones((F, N), dtype=np.int32)
    for t in range(F):
        m[t, rng.permutation(N)[:N // 3]] = 0
    m[7] = 0
    m[19] = 0; m[19, 5] = 1
    return m


def g8_batched(N=200, F=40, seed=81):
    """A multi-frame pin of the path the benchmark times: 40 consecutive frames at N = 200 through the oracle in BATCHED mode (one refactor per frame — held to the
    reference's SEQUENTIAL structure by g7 / test_g7_batched_equals_sequential_at_benchmark_sizes), partial / empty / single-match frames included.
    ~2 s of single-thread CPU per frame.  Stored: the association pattern, the trajectory, and of the final state X, diag P, the robot columns of P, every
    landmark's 6 x 6 block and P V for 16 seeded +-1 probe vectors."""
    p = synth.scene_params()
    sc = synth.make_scene(N, F, seed=seed, p=p)
    matched = g8_match_pattern(N, F, seed)
    o = O.Oracle(N, p); o.set_state(sc["X0"], sc["S0"])
    traj = o.run_frames(sc["odo"], sc["z"], matched, O.Oracle.BATCHED)
    X, S = o.get_state()
    P = S.T @ S
    n = 6 * N + 4
    V = np.random.default_rng(800 + N).choice([-1.0, 1.0], size=(n, 16))
    blocks = np.stack([P[6 * k:6 * k + 6, 6 * k:6 * k + 6] for k in range(N)])
    return dict(N=N, F=F, seed=seed, matched=matched.astype(np.int8), traj=traj, X=X, P_diag=np.diag(P).copy(), P_robot_cols=P[:, n - 4:].copy(), P_blocks=blocks,
                V=V, PV=P @ V, P_absmax=np.abs(P).max(), clamps=np.array(list(o.clamp_stats().values())))


def multi_frame_pin(N, F, seed, storage="f64", empty=None, single=None, exact_means=False):
    """F consecutive BATCHED oracle frames at a size whose launch plan differs from N = 200's (g9: N = 500 — split form, fused tail on the permuted operands, split-K
    k_syrk; g10: N = 800 — more tiles than the memory-tile form can own), with a third of the landmarks unmatched per frame, optionally one frame without a match and
    one with a single match.  storage = "f32" (BASELINE configs[4]): the state that lives from frame to frame is float — X and S are rounded to float before the first
    frame and after every frame, exactly what srukf_set_storage(SRUKF_STORAGE_F32) keeps, and the trajectory row is read from the rounded state.
    ~30 s (N = 500) / ~2.5 min (N = 800) of single-thread CPU per frame.  Stored like g7 / g8.  exact_means: the oracle's weighted means in binary128 (Oracle.set_exact_means;
    g9 f64: the reference's running sum for h is off by ~4e-8 px at N = 500, which moves the weakly observed rows of X by ~1e-9 — as much as the fixture's bound)."""
    p = synth.scene_params()
    sc = synth.make_scene(N, F, seed=seed, p=p)
    rng = np.random.default_rng(seed)
    matched = np.ones((F, N), dtype=np.int32)
    for t in range(F):
        matched[t, rng.permutation(N)[:N // 3]] = 0
    if empty is not None:
        matched[empty] = 0
    if single is not None:
        matched[single] = 0; matched[single, 5] = 1
    f32 = storage == "f32"
    rnd = (lambda a: a.astype(np.float32).astype(np.float64)) if f32 else (lambda a: a)
    n = 6 * N + 4
    o = O.Oracle(N, p); o.set_state(rnd(sc["X0"]), rnd(np.triu(sc["S0"])))
    o.set_exact_means(exact_means)
    traj = np.zeros((F, 8))
    for t in range(F):
        tr = o.run_frames(sc["odo"][t:t + 2], sc["z"][t:t + 1], matched[t:t + 1], O.Oracle.BATCHED)
        X, S = o.get_state()
        if f32:
            X, S = rnd(X), rnd(np.triu(S))
            o.set_state(X, S)
            Pr = S[:, n - 4:n - 2].T @ S[:, n - 4:n - 2]
            traj[t, :4] = X[n - 4:]; traj[t, 4:] = Pr.ravel()
        else:
            traj[t] = tr[0]
    X, S = o.get_state()
    P = S.T @ S
    V = np.random.default_rng(900 + N).choice([-1.0, 1.0], size=(n, 16))
    blocks = np.stack([P[6 * k:6 * k + 6, 6 * k:6 * k + 6] for k in range(N)])
    # |S|^T |S| of the final state on the stored entries: the scale of one float ulp per entry of S in P (fp32 storage bounds are relative to it)
    A = np.abs(S)
    AV = A.T @ (A @ np.ones((n, 1)))
    return dict(N=N, F=F, seed=seed, storage=storage, matched=matched.astype(np.int8), traj=traj, X=X, P_diag=np.diag(P).copy(), P_robot_cols=P[:, n - 4:].copy(), P_blocks=blocks,
                V=V, PV=P @ V, P_absmax=np.abs(P).max(), absS_diag=np.einsum("ki,ki->i", A, A), absS_rowsum=AV.ravel(), clamps=np.array(list(o.clamp_stats().values())))


def g11_recover_scene(N=200, F=4, seed=1, obs_seeds=(300, 301)):
    """The INPUTS of test_gpu_parity_r4.test_batched_filters_recover_from_flagged_frames (shipped a1..a4 = 8, N = 200, one map, one sequence of measurement noise per
    filter), stored rather than regenerated: the joint initialisation's QR (numpy -> OpenBLAS) rounds differently with the BLAS thread count and kernels of the machine,
    and the filter of that test diverges, so a scene that differs in the last bits moves its distance to the oracle by more than the test's tolerance."""
    p = synth.default_params()
    scs = [synth.make_scene(N, F, seed=seed, p=p, obs_seed=o) for o in obs_seeds]
    return dict(N=N, F=F, seed=seed, obs_seeds=np.array(obs_seeds), X0=scs[0]["X0"], S0=scs[0]["S0"], odo=scs[0]["odo"],
                z=np.stack([sc["z"] for sc in scs]), matched=np.stack([sc["matched"] for sc in scs]).astype(np.int8))


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "g9":
        # separate (slow) target:  python tests/golden/make_golden.py g9 [f64|f32]   (N = 500, 8 frames: ~4 min each)
        for st in (sys.argv[2:] or ["f64", "f32"]):
            np.savez_compressed(os.path.join(OUT, f"g9_batched_n500_{st}.npz"), **multi_frame_pin(500, 8, 91, st, empty=3, single=5, exact_means=(st == "f64")))
        sys.exit(0)
    if len(sys.argv) > 1 and sys.argv[1] == "g10":
        # separate (slow) target:  python tests/golden/make_golden.py g10   (N = 800, 2 frames: ~5 min)
        np.savez_compressed(os.path.join(OUT, "g10_batched_n800.npz"), **multi_frame_pin(800, 2, 101, "f64"))
        sys.exit(0)
    if len(sys.argv) > 1 and sys.argv[1] == "g11":
        # inputs only (no oracle run):  python tests/golden/make_golden.py g11
        np.savez_compressed(os.path.join(OUT, "g11_recover_scene_n200.npz"), **g11_recover_scene())
        sys.exit(0)
    if len(sys.argv) > 1 and sys.argv[1] == "g8":
        # separate (slow) target:  python tests/golden/make_golden.py g8
        np.savez_compressed(os.path.join(OUT, "g8_batched_n200.npz"), **g8_batched())
        sys.exit(0)
    if len(sys.argv) > 1 and sys.argv[1] == "g7":
        # separate (slow) target:  python tests/golden/make_golden.py g7 [n50|n200]
        which = sys.argv[2:] or ["n50", "n200"]
        if "n50" in which:
            np.savez_compressed(os.path.join(OUT, "g7_sequential_n50.npz"), **g7_sequential(50, 2, 71))
        if "n200" in which:
            np.savez_compressed(os.path.join(OUT, "g7_sequential_n200.npz"), **g7_sequential(200, 1, 72))
        sys.exit(0)
    np.savez_compressed(os.path.join(OUT, "g1_weights.npz"), table=g1_weights())
    np.savez_compressed(os.path.join(OUT, "g2_projection.npz"), **g2_projection())
    np.savez_compressed(os.path.join(OUT, "g3_gmw.npz"), **g3_gmw())
    np.savez_compressed(os.path.join(OUT, "g4_joint_init.npz"), **g4_joint_init())
    np.savez_compressed(os.path.join(OUT, "g5_frame_n8.npz"), **g5_frame())
    np.savez_compressed(os.path.join(OUT, "g6_trajectory_n20.npz"), **g6_trajectory())
    for f in sorted(os.listdir(OUT)):
        if f.endswith(".npz"):
            print(f, os.path.getsize(os.path.join(OUT, f)))
