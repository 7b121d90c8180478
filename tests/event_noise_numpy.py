"""Yardstick of the noisy event sensor: written from the model's statement, not from the library.  A per-event scalar recipe
on Python floats (IEEE float64, one rounding per operation, nothing fused) and a Philox4x32-10 on Python ints.  It builds on
tests/event_sim_numpy.py (the level images) and tests/event_stream_numpy.py (`event_time`, the time of a crossing).

Model.  State per pixel: L_ref and t_last, the time of the pixel's last emitted event (-inf after a reset).  Parameters:
refractory rho (s), leak rate lambda (Hz), shot rate r (Hz per pixel and polarity), seed (64 bits), and the index of the
interval since the reset.  An interval [t_a, t_b] has K sub-steps, delta = (t_b - t_a) / K, g = lambda * delta, q = r * delta.
Per pixel with flat index o, at sub-step s = 1..K, in this order:

  1 leak, if lambda > 0: L_ref = L_ref - g * C_pos (the product, then the difference)
  2 signal candidates: with R = L_ref and d = L_s - R:  d >= C_pos: n = floor(d / C_pos) positive ones, L_ref = R + n * C_pos;
    else -d >= C_neg: n = floor(-d / C_neg) negative ones, L_ref = R - n * C_neg.  Candidate k = 1..n has the time
    `event_stream_numpy.event_time` gives it (X_k = R +- k C, f_k limited to [0, 1], t_k = t_a + (((s - 1) + f_k) / K)(t_b - t_a))
  3 shot-noise candidates, if r > 0: one Philox4x32-10 block w0..w3 with key (seed & 0xffffffff, seed >> 32) and counter
    (o, interval, s, 0); u(w) = (w + 0.5) * 2^-32.  A negative candidate exists iff u(w0) < q, at f = u(w1); a positive one
    iff u(w2) < q, at f = u(w3); t = t_a + (((s - 1) + f) / K) * (t_b - t_a).  They do not move L_ref.
  4 merge: signal candidates in the order k = 1..n, noise candidates in ascending t (on equal t the negative one first); the
    next noise candidate leaves before the next signal candidate iff its t is smaller (on equal t signal comes first)
  5 refractory filter in merged order: emitted iff t - t_last >= rho; an emitted candidate sets t_last = t

Output per interval: the uint8 (-, +) image of emitted events saturated at 255, L_ref, t_last, and the emitted events
pixel-major.  Every candidate is also recorded with what became of it, for the conditions of tests/event_noise_cases.py."""
import math

import numpy as np

from tests import event_sim_numpy as Y
from tests import event_stream_numpy as YS

M32 = 0xFFFFFFFF


def philox4x32(counter, key, rounds=10):
    """the block of four 32-bit words: counter a 4-tuple, key a 2-tuple of Python ints"""
    c0, c1, c2, c3 = (int(v) & M32 for v in counter)
    k0, k1 = (int(v) & M32 for v in key)
    for _ in range(rounds):
        p0, p1 = 0xD2511F53 * c0, 0xCD9E8D57 * c2
        c0, c1, c2, c3 = ((p1 >> 32) ^ c1 ^ k0) & M32, p1 & M32, ((p0 >> 32) ^ c3 ^ k1) & M32, p0 & M32
        k0, k1 = (k0 + 0x9E3779B9) & M32, (k1 + 0xBB67AE85) & M32
    return c0, c1, c2, c3


def uniform(w):
    return (float(w) + 0.5) * 2.0 ** -32


def noise_time(f, s, K, t_a, t_b):
    u = (float(s - 1) + f) / float(K)
    return t_a + u * (t_b - t_a)


class NoisySensor:
    """L_ref, t_last and the thresholds of one case; `interval` counts the steps since the start"""

    def __init__(self, first_level, c_pos, c_neg, refractory=0.0, leak_rate=0.0, shot_rate=0.0, seed=0):
        self.ref = np.array(first_level, dtype=np.float64, copy=True)
        self.t_last = np.full(self.ref.shape, -np.inf)
        self.c_pos = np.broadcast_to(np.asarray(c_pos, dtype=np.float64), self.ref.shape)
        self.c_neg = np.broadcast_to(np.asarray(c_neg, dtype=np.float64), self.ref.shape)
        self.rho, self.lam, self.r, self.seed = float(refractory), float(leak_rate), float(shot_rate), int(seed)
        self.interval = 0


def step_levels(sensor, levels, t_a, t_b):
    """One interval over the K + 1 level images `levels` (levels[0] the previous frame's).  Advances `sensor` and returns a
    dict: events (uint8 [H,W,2]), t, x, y, p (emitted, pixel-major), per emitted event also den (L_s - L_prev) and c (its
    threshold) -- inf and 0 for a noise event, whose time no level enters -- and noise (bool); total ([H,W] int64 emitted per
    pixel), ref, t_last, K, margin ([H,W]: the smallest distance of d / C from an event boundary over the sub-steps,
    `event_sim_numpy.count_margin`) and `candidates`: one row per candidate (flat pixel, s, t, p, kind (0 signal, 1 noise),
    emitted (0 / 1), t_last before it, den, c, den and c of the event that set that t_last, f before the limit (0.5 for a
    noise candidate), and that f of the event that set t_last)."""
    K = len(levels) - 1
    H, W = sensor.ref.shape
    delta = (t_b - t_a) / K
    g, q = sensor.lam * delta, sensor.r * delta
    assert q <= 1.0
    key = (sensor.seed & M32, sensor.seed >> 32)
    neg_img, pos_img = np.zeros((H, W), dtype=np.int64), np.zeros((H, W), dtype=np.int64)
    lv = [np.asarray(v, dtype=np.float64) for v in levels]
    rows, cand = [], []
    margin = np.full((H, W), np.inf)
    if not hasattr(sensor, 'last_den'):
        sensor.last_den, sensor.last_c, sensor.last_raw = np.full((H, W), np.inf), np.zeros((H, W)), np.full((H, W), 0.5)
    for y in range(H):
        for x in range(W):
            o = y * W + x
            ref, t_last = float(sensor.ref[y, x]), float(sensor.t_last[y, x])
            cp, cn = float(sensor.c_pos[y, x]), float(sensor.c_neg[y, x])
            last_den, last_c, last_raw = float(sensor.last_den[y, x]), float(sensor.last_c[y, x]), float(sensor.last_raw[y, x])
            for s in range(1, K + 1):
                lp, ls = float(lv[s - 1][y, x]), float(lv[s][y, x])
                if sensor.lam > 0.0:
                    leak = g * cp
                    ref = ref - leak
                R = ref
                d = ls - R
                margin[y, x] = min(margin[y, x], float(Y.count_margin(np.float64(d), np.float64(cp), np.float64(cn))))
                signal = []
                if d >= cp:
                    n, up, c = math.floor(d / cp), True, cp
                    ref = R + n * cp
                elif -d >= cn:
                    n, up, c = math.floor(-d / cn), False, cn
                    ref = R - n * cn
                else:
                    n, up, c = 0, True, cp
                for k in range(1, int(n) + 1):
                    t, raw, den = YS.event_time(R, float(k), c, up, lp, ls, s, K, t_a, t_b)
                    signal.append((t, 1 if up else 0, 0, den, c, raw))
                noise = []
                if sensor.r > 0.0:
                    w = philox4x32((o, sensor.interval, s, 0), key)
                    if uniform(w[0]) < q:
                        noise.append((noise_time(uniform(w[1]), s, K, t_a, t_b), 0, 1, math.inf, 0.0, 0.5))
                    if uniform(w[2]) < q:
                        noise.append((noise_time(uniform(w[3]), s, K, t_a, t_b), 1, 1, math.inf, 0.0, 0.5))
                    noise.sort(key=lambda e: e[0])                   # stable: on equal t the negative one stays first
                merged, i, j = [], 0, 0
                while i < len(signal) or j < len(noise):
                    if j < len(noise) and (i == len(signal) or noise[j][0] < signal[i][0]):
                        merged.append(noise[j])
                        j += 1
                    else:
                        merged.append(signal[i])
                        i += 1
                for t, p, kind, den, c, raw in merged:
                    emitted = t - t_last >= sensor.rho
                    cand.append((o, s, t, p, kind, 1 if emitted else 0, t_last, den, c, last_den, last_c, raw, last_raw))
                    if emitted:
                        t_last, last_den, last_c, last_raw = t, den, c, raw
                        rows.append((t, x, y, p, den, c, kind))
                        if p:
                            pos_img[y, x] += 1
                        else:
                            neg_img[y, x] += 1
            sensor.ref[y, x], sensor.t_last[y, x] = ref, t_last
            sensor.last_den[y, x], sensor.last_c[y, x], sensor.last_raw[y, x] = last_den, last_c, last_raw
    sensor.interval += 1
    a = np.array(rows, dtype=np.float64).reshape(-1, 7)
    events = np.stack([np.minimum(neg_img, 255), np.minimum(pos_img, 255)], axis=-1).astype(np.uint8)
    return dict(events=events, t=a[:, 0].copy(), x=a[:, 1].astype(np.uint16), y=a[:, 2].astype(np.uint16), p=a[:, 3].astype(np.uint8),
                den=a[:, 4].copy(), c=a[:, 5].copy(), noise=a[:, 6] > 0, total=neg_img + pos_img, ref=sensor.ref.copy(),
                t_last=sensor.t_last.copy(), K=K, margin=margin,
                candidates=np.array(cand, dtype=np.float64).reshape(-1, 13))
