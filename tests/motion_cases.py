"""Inputs for the motion-step tests (test_motion_cpu.py, test_gpu_motion.py): odometry pairs off the figure-8, robot blocks of S that make the 4x4 Gram
Cholesky of the device's motion step work for its living, and three-frame odometry sequences for whole frames.  A table like tests/cameras.py.

ODOMETRY   name -> (odo_prev, odo_cur).  The robot pose (x, y, theta) of the state is set to odo_prev before the step (place()), z is left as it is.
           The control is what SLAM.cpp:1446-1458 makes of the pair, quirks included (np_motion.control):
             figure8        the suite's usual source, as the control case
             still_0        nothing moves at heading 0: atan2(0, 0) - 0, so Ut and Mt are exactly zero and every sigma point of a null direction IS the centre
             still_1p2      nothing moves at heading 1.2: rot1 = atan2(0, 0) - 1.2 = -1.2, rot2 = +1.2, and Mt != 0 although nothing moved
             turn           0.3 rad on the spot
             reverse        1 cm backwards: rot1 = pi, Mt[0] = a1 pi^2 (the filter diverges behind it: a motion-step case only)
             wrap           forward across +pi: the heading arrives wrapped at -3.14 from 3.13, so rot2 is about -2 pi, with its noise (reproduce, do not repair)
             heading_40     a heading that was never wrapped: |rot1|, |rot2| of about 38 and sincos arguments of 40
             step_6cm       6 cm and 0.1 rad in one frame
             translated     1 cm forward from (50, -30) at heading 2.5: the weighted mean cancels L terms of size |wm0| |x| down to x
BLOCKS     name -> how the robot part of S is changed (the landmark rows of the robot columns included where the case needs it):
             after_frame    the state one ordinary frame leaves: the robot z pivot is already sqrt(epsilon) there
             z_zero         row and column of z exactly zero: G[2][2] = 0, the `raa > 0 ? v / raa : 0` branch of motion_finish
             xy_dependent   the y column of S is 0.7 times the x column (x and y perfectly correlated): with nothing moving, dsum = G[1][1] - R[0][1]^2 cancels to
                            rounding noise of either sign: the sqrt(fmax(dsum, 0)) branch
             theta_1e-12    heading standard deviation 1e-12
             fresh_S0       the joint-initialised start state itself (null rows exactly zero, robot block diagonal)
SEQUENCES  name -> three odometry steps behind one ordinary figure-8 frame, for whole frames: the oracle stays clean on them (no theta clamp) at N = 21 and 43.
TRANSLATION  the shift of the translated scene: the same map, robot and truth moved by (50, -30) m, S unchanged."""
import numpy as np

SEED = 5
TRANSLATION = np.array([50.0, -30.0])


def _forward(prev, dist, mid_heading, new_heading):
    x, y, th = prev
    return np.array([x + dist * np.cos(mid_heading), y + dist * np.sin(mid_heading), new_heading])


def odometry(synth, name):
    """(odo_prev, odo_cur) of the named case"""
    base = np.array([0.25, -0.125, 0.0])
    if name == "figure8":
        odo = synth.figure8_odometry(2)
        return odo[1].copy(), odo[2].copy()
    if name == "still_0":
        return base.copy(), base.copy()
    if name == "still_1p2":
        prev = base + [0, 0, 1.2]
        return prev, prev.copy()
    if name == "turn":
        prev = base + [0, 0, 0.4]
        return prev, prev + [0, 0, 0.3]
    if name == "reverse":
        prev = base + [0, 0, -0.3]
        return prev, _forward(prev, -0.01, -0.3, -0.3)
    if name == "wrap":
        prev = base + [0, 0, 3.13]
        return prev, _forward(prev, 0.01, 3.135, -3.14)
    if name == "heading_40":
        prev = base + [0, 0, 40.0]
        return prev, _forward(prev, 0.01, 40.005, 40.01)
    if name == "step_6cm":
        prev = base + [0, 0, 0.4]
        return prev, _forward(prev, 0.06, 0.45, 0.5)
    if name == "translated":
        prev = np.array([TRANSLATION[0], TRANSLATION[1], 2.5])
        return prev, _forward(prev, 0.01, 2.51, 2.52)
    raise KeyError(name)


ODOMETRY = ("figure8", "still_0", "still_1p2", "turn", "reverse", "wrap", "heading_40", "step_6cm", "translated")
BLOCKS = ("after_frame", "z_zero", "xy_dependent", "theta_1e-12", "fresh_S0")
DEGENERATE = ("z_zero", "xy_dependent", "theta_1e-12")


def place(X, odo_prev):
    """the state's robot pose set to the odometry pose (z stays)"""
    X = np.array(X, dtype=np.float64)
    n = X.shape[0]
    X[n - 4], X[n - 3], X[n - 1] = odo_prev[0], odo_prev[1], odo_prev[2]
    return X


def block(name, S):
    """the named robot block applied to a copy of the upper-triangular factor S (after_frame / fresh_S0: which state the caller passes)"""
    S = np.triu(np.array(S, dtype=np.float64))
    n = S.shape[0]
    if name in ("after_frame", "fresh_S0"):
        return S
    if name == "z_zero":
        S[:, n - 2] = 0.0
        S[n - 2, :] = 0.0
    elif name == "xy_dependent":
        S[:, n - 3] = 0.7 * S[:, n - 4]                      # (row n-3 is zero in column n-4: its own pivot becomes exactly zero)
    elif name == "theta_1e-12":
        S[:, n - 1] = 0.0
        S[n - 1, n - 1] = 1e-12
    else:
        raise KeyError(name)
    return S


def scene(synth, N, F=4):
    return synth.make_scene(N, F, seed=SEED, p=synth.scene_params())


# ---- whole frames ----------------------------------------------------------------------------------------------------------------------------------------

SEQUENCES = ("standstill", "stop_and_go", "turn_on_the_spot", "step_6cm")


def sequence(synth, sc, name, shift=(0.0, 0.0)):
    """One ordinary figure-8 frame, then three frames of the named kind: (odo (5, 3), z (4, 2N), matched (4, N)).  The measurements are the scene's own model of
    the true landmarks from the odometry poses plus the scene's pixel noise; `shift` moves the odometry (the measurements do not change: the map moves with it)."""
    N, p = sc["N"], sc["params"]
    odo = np.zeros((5, 3))
    odo[:2] = sc["odo"][:2]
    for t in range(1, 4):
        x, y, th = odo[t]
        if name == "standstill":
            odo[t + 1] = odo[t]
        elif name == "stop_and_go":
            odo[t + 1] = odo[t] if t == 2 else _forward(odo[t], 0.01, th + 0.01, th + 0.02)
        elif name == "turn_on_the_spot":
            odo[t + 1] = (x, y, th + 0.3)
        elif name == "step_6cm":
            odo[t + 1] = _forward(odo[t], 0.06, th + 0.05, th + 0.1)
        else:
            raise KeyError(name)
    rng = np.random.default_rng(SEED + 101)
    z = np.zeros((4, 2 * N))
    z[0] = sc["z"][0]
    for t in range(1, 4):
        x, y, th = odo[t + 1]
        uv = synth.project(sc["truth"], np.broadcast_to([x, y, 0.0], (N, 3)), np.full(N, th), np.zeros((N, 2)), p, iters=12)
        z[t] = (uv + rng.normal(0, 0.5, (N, 2))).ravel()
    odo = odo + [shift[0], shift[1], 0.0]
    return odo, z, np.ones((4, N), dtype=np.int32)


def translate_state(X, shift):
    """the state of the translated scene: every landmark's anchor and the robot moved by `shift` (x, y)"""
    X = np.array(X, dtype=np.float64)
    n = X.shape[0]
    X[0:n - 4:6] += shift[0]
    X[1:n - 4:6] += shift[1]
    X[n - 4] += shift[0]
    X[n - 3] += shift[1]
    return X


def standstill_in_front(synth, sc, X1, odo_prev, odo_cur):
    """For the form of the motion step that needs a complete frame in front of it (the frame tail prepares the next step, and a frame without matches has no tail):
    the scene moved so that the robot of the state X1 (one ordinary frame behind the origin) stands at odo_prev, heading included, and a standstill frame there
    with measurements of the true landmarks.  -> (X, the pair moved likewise, z of the standstill frame)"""
    N, p = sc["N"], sc["params"]
    n = X1.shape[0]
    X = translate_state(X1, odo_prev[:2])
    X[n - 1] = odo_prev[2]
    at = np.array([sc["odo"][1][0], sc["odo"][1][1], 0.0])       # where the ordinary frame has left the robot, before the move
    prev, cur = np.asarray(odo_prev) + at, np.asarray(odo_cur) + at
    truth = sc["truth"].copy()
    truth[:, 0] += odo_prev[0]
    truth[:, 1] += odo_prev[1]
    uv = synth.project(truth, np.broadcast_to([prev[0], prev[1], 0.0], (N, 3)), np.full(N, prev[2]), np.zeros((N, 2)), p, iters=12)
    z = (uv + np.random.default_rng(SEED + 202).normal(0, 0.5, (N, 2))).ravel()
    return X, prev, cur, z
