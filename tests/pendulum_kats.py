"""Pendulum known answers written out by hand from gym's published PendulumEnv.step (g = 10, m = l = 1, dt = 0.05,
max_speed = 8, max_torque = 2), with no dependence on the oracle's restatement:

    u      = clip(act, -2, 2)
    cost   = angle_normalize(th)^2 + 0.1 thdot^2 + 0.001 u^2,   angle_normalize(x) = ((x + pi) mod 2 pi) - pi
    thdot' = thdot + (-3g/(2l) sin(th + pi) + 3/(m l^2) u) dt  =  thdot + 0.75 sin(th) + 0.15 u
    v0 (gym 0.10.5, Pendulum-v0): th' = th + thdot' dt, THEN thdot' = clip(thdot', -8, 8)   (theta integrates the unclipped velocity)
    v1 (Pendulum-v1):             thdot' = clip(thdot', -8, 8), THEN th' = th + thdot' dt
    reward = -cost

Each row: (th, thdot, act,  th' v0, thdot' v0,  th' v1, thdot' v1,  reward)."""
import numpy as np

PI = 3.141592653589793
HALF_PI = 1.5707963267948966
PI_SQ = 9.869604401089358            # pi^2
HALF_PI_SQ = 2.4674011002723395      # (pi/2)^2

PENDULUM_KATS = np.array([
    # upright at rest, no torque: nothing moves, nothing costs
    (0.0, 0.0, 0.0,  0.0, 0.0,  0.0, 0.0,  0.0),
    # horizontal at rest: thdot' = 0.75 sin(pi/2) = 0.75, th' = pi/2 + 0.75 * 0.05, cost = (pi/2)^2
    (HALF_PI, 0.0, 0.0,  HALF_PI + 0.0375, 0.75,  HALF_PI + 0.0375, 0.75,  -HALF_PI_SQ),
    (-HALF_PI, 0.0, 0.0,  -HALF_PI - 0.0375, -0.75,  -HALF_PI - 0.0375, -0.75,  -HALF_PI_SQ),
    # angle_normalize in the cost: +-pi, 3 pi and -3 pi are all the angle +-pi (cost pi^2); sin = 0, so nothing moves
    (PI, 0.0, 0.0,  PI, 0.0,  PI, 0.0,  -PI_SQ),
    (-PI, 0.0, 0.0,  -PI, 0.0,  -PI, 0.0,  -PI_SQ),
    (3 * PI, 0.0, 0.0,  3 * PI, 0.0,  3 * PI, 0.0,  -PI_SQ),
    (-3 * PI, 0.0, 0.0,  -3 * PI, 0.0,  -3 * PI, 0.0,  -PI_SQ),
    # |thdot'| > 8: 7.9 + 0.75 + 0.15 * 2 = 8.95.  v0: th' = pi/2 + 8.95 * 0.05 = pi/2 + 0.4475 and thdot' = 8;
    # v1: thdot' = 8 first, th' = pi/2 + 0.4.  cost = (pi/2)^2 + 0.1 * 7.9^2 + 0.001 * 4 = (pi/2)^2 + 6.245
    (HALF_PI, 7.9, 2.0,  HALF_PI + 0.4475, 8.0,  HALF_PI + 0.4, 8.0,  -(HALF_PI_SQ + 6.245)),
    (-HALF_PI, -7.9, -2.0,  -HALF_PI - 0.4475, -8.0,  -HALF_PI - 0.4, -8.0,  -(HALF_PI_SQ + 6.245)),
    # |act| > 2 is clipped in the dynamics (thdot' = 0.15 * 2 = 0.3, not 0.75) AND in the cost (0.001 * 4, not 0.025)
    (0.0, 0.0, 5.0,  0.015, 0.3,  0.015, 0.3,  -0.004),
    (0.0, 0.0, -5.0,  -0.015, -0.3,  -0.015, -0.3,  -0.004),
])
