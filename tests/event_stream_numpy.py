"""Yardstick of the time-stamped event streams: written from the model's statement, not from the library.  A per-event scalar
recipe on Python floats (IEEE float64, one rounding per operation, nothing fused).

Model.  The sensor is the one of tests/event_sim_numpy.py (`Sensor.visit` is its closed form and stays the source of the counts
and of L_ref).  An interval [t_a, t_b] is visited at sub-steps s = 1..K.  With L_prev the level seen at sub-step s - 1 (for
s = 1 the previous frame's level), L_s this sub-step's level and R the value of L_ref before the update, the n events the pixel
fires at s are k = 1..n:

    X_k = R + k * C_pos (positive) or R - k * C_neg (negative): the product, then the sum
    f_k = (X_k - L_prev) / (L_s - L_prev), then limited to [0, 1]: below 0 or not a number gives 0, above 1 gives 1
    t_k = t_a + (((s - 1) + f_k) / K) * (t_b - t_a)

Order: row-major pixels, within a pixel sub-step by sub-step and k ascending.

Accumulation: np.add.at; event t goes to bin b where edges[b] < t <= edges[b+1]; an event with x >= W or y >= H is dropped
and counted as `sensor` whatever its time, another one outside every bin (or with t not a number) is dropped and counted as
`time`; p != 0 is positive; uint8 output saturated at 255."""
import math

import numpy as np

from tests import event_sim_numpy as Y


def event_time(R, k, c, up, L_prev, L_s, s, K, t_a, t_b):
    """(t_k, f_k before the limit, L_s - L_prev) of one event, scalars"""
    step = k * c
    X = R + step if up else R - step
    num, den = X - L_prev, L_s - L_prev
    if den == 0.0:
        raw = math.nan if (num == 0.0 or math.isnan(num)) else math.copysign(math.inf, num) * math.copysign(1.0, den)
    else:
        raw = num / den
    f = raw
    if not f >= 0.0:
        f = 0.0
    if f > 1.0:
        f = 1.0
    u = (float(s - 1) + f) / float(K)
    return t_a + u * (t_b - t_a), raw, den


def step_levels(sensor, levels, t_a, t_b):
    """One interval over the K + 1 level images `levels` ([K+1] of float64 [H,W]; levels[0] is the previous frame's): advances
    `sensor` (Y.Sensor) exactly as K calls of Sensor.visit do and returns a dict: events (uint8 [H,W,2]), t, x, y, p (the
    stream, pixel-major), per event also raw_f (f before the limit), den (L_s - L_prev) and c (its threshold), total ([H,W]
    int64, the unsaturated events per pixel), ref (L_ref after the interval) and K."""
    K = len(levels) - 1
    H, W = sensor.ref.shape
    sensor.begin()
    per_step = []
    for s in range(1, K + 1):
        R, pos0, neg0 = sensor.ref.copy(), sensor.pos.copy(), sensor.neg.copy()
        sensor.visit(levels[s])
        per_step.append((R, sensor.pos - pos0, sensor.neg - neg0))
    rows = []
    for y in range(H):
        for x in range(W):
            for s in range(1, K + 1):
                R, n_pos, n_neg = per_step[s - 1]
                up = n_pos[y, x] > 0
                n = int(n_pos[y, x] if up else n_neg[y, x])
                if n == 0:
                    continue
                c = float(sensor.c_pos[y, x] if up else sensor.c_neg[y, x])
                r, lp, ls = float(R[y, x]), float(levels[s - 1][y, x]), float(levels[s][y, x])
                for k in range(1, n + 1):
                    t, raw, den = event_time(r, float(k), c, up, lp, ls, s, K, t_a, t_b)
                    rows.append((t, x, y, 1 if up else 0, raw, den, c))
    a = np.array(rows, dtype=np.float64).reshape(-1, 7)
    return dict(events=sensor.events(), t=a[:, 0].copy(), x=a[:, 1].astype(np.uint16), y=a[:, 2].astype(np.uint16),
                p=a[:, 3].astype(np.uint8), raw_f=a[:, 4].copy(), den=a[:, 5].copy(), c=a[:, 6].copy(),
                total=(sensor.pos + sensor.neg).astype(np.int64), ref=sensor.ref.copy(), K=K)


def image_levels(prev, cur, K, eps):
    """the K + 1 levels of the image route: L_a, then L_a + (s / K) * (L_b - L_a)"""
    la, lb = Y.level_of_image(prev, eps), Y.level_of_image(cur, eps)
    delta = lb - la
    return [la] + [la + (float(s) / float(K)) * delta for s in range(1, K + 1)]


def scene_levels(room, poses, cam, eps):
    """the K + 1 levels of the analytic route: the room rendered at `poses` ([K+1,3|4,4], the previous frame's first)"""
    return [Y.level_of_color(Y.render(room, pose, cam)['color'], eps) for pose in poses]


def accumulate(t, x, y, p, edges, H, W):
    """(counts uint8 [B,H,W,2], unsaturated int64 [B,H,W,2], dropped_time, dropped_sensor)"""
    edges = [float(e) for e in edges]
    B = len(edges) - 1
    full = np.zeros((B, H, W, 2), dtype=np.int64)
    bins, ys, xs, ps = [], [], [], []
    dropped_time = dropped_sensor = 0
    for tt, xx, yy, pp in zip(np.asarray(t).tolist(), np.asarray(x).tolist(), np.asarray(y).tolist(), np.asarray(p).tolist()):
        if xx >= W or yy >= H:
            dropped_sensor += 1
            continue
        b = next((j for j in range(B) if edges[j] < tt <= edges[j + 1]), None)
        if b is None:
            dropped_time += 1
            continue
        bins.append(b), ys.append(yy), xs.append(xx), ps.append(1 if pp else 0)
    np.add.at(full, (np.array(bins, dtype=np.int64), np.array(ys, dtype=np.int64), np.array(xs, dtype=np.int64),
                     np.array(ps, dtype=np.int64)), 1)
    return np.where(full > 255, 255, full).astype(np.uint8), full, dropped_time, dropped_sensor
