"""Yardstick of the event-stream filter: written from the model's statement in include/enslam_hip.h, not from the library.  A
per-event scalar state machine on Python floats (IEEE float64: comparisons and one subtraction) with plain dicts and lists
per pixel; nothing is vectorised and nothing is shared with event_filter.filter_numpy.

Model.  Stream of N events i = 0..N-1 (t, x, y, p); sensor H x W, flat index o = y W + x.  State per pixel, -inf after a
reset: t_last (the time of the last event that passed the refractory stage) and t_seen (the largest time of the pixel's
events that passed stages 0 and 1).  One call filters one chunk; every event gets the first class that applies:

  stage 0   SENSOR (1): x >= W or y >= H.  TIME (2): t is NaN, +inf or -inf.  HOT (3): hot_mask[o] != 0.  Else live.
  stage 1   the live events of a pixel in the order (t, i): passes iff t - t_last[o] >= rho, then t_last[o] = t; otherwise
            REFRACTORY (4).  The events that passed are S.
  stage 2   only with support: an S-event at (x, y, t) is kept iff for one of the up to eight pixels (x + dx, y + dy) inside
            the sensor, (dx, dy) != (0, 0), a time t' exists with t' <= t and t - t' <= dt, where t' is the time of an S-event
            of that pixel in this chunk or that pixel's t_seen from before the call; otherwise UNSUPPORTED (5).  t - t' falls
            as t' grows, so of a neighbour's S times only the largest one <= t is tested (bisect on its ascending list).
  after     t_seen[o] = max(t_seen[o], the largest S time at o)

Output: the events of class 0 in stream order, the classes, the counters, the two states."""
import bisect
import math

KEPT, SENSOR, TIME, HOT, REFRACTORY, UNSUPPORTED = range(6)
NAMES = ('kept', 'sensor', 'time', 'hot', 'refractory', 'unsupported')


class FilterState:
    """t_last and t_seen as dicts by flat pixel index; a missing key is -inf"""

    def __init__(self, H, W):
        self.H, self.W = int(H), int(W)
        self.t_last, self.t_seen = {}, {}

    def plane(self, which):
        """the state as a list of H rows of W floats"""
        d = self.t_last if which == 't_last' else self.t_seen
        return [[d.get(y * self.W + x, -math.inf) for x in range(self.W)] for y in range(self.H)]


def filter_chunk(state, t, x, y, p, rho, support, dt, hot_mask=None):
    """One call.  t, x, y, p: sequences of Python numbers; hot_mask: None or H rows of W values.  Advances `state` and returns
    a dict: classes (list of N ints), kept (list of the stream positions of class 0, ascending), counters (dict), and
    reached_support / removed_support, reached_refractory / removed_refractory (for the conditions of the cases)."""
    H, W = state.H, state.W
    N = len(t)
    classes = [KEPT] * N
    runs = {}                                                   # flat pixel -> [(t, i)] of its live events
    for i in range(N):
        xi, yi, ti = int(x[i]), int(y[i]), float(t[i])
        if xi >= W or yi >= H:
            classes[i] = SENSOR
        elif math.isnan(ti) or math.isinf(ti):
            classes[i] = TIME
        elif hot_mask is not None and hot_mask[yi][xi] != 0:
            classes[i] = HOT
        else:
            runs.setdefault(yi * W + xi, []).append((ti, i))
    passed = {}                                                 # flat pixel -> ascending S times; and their stream positions
    s_events = []
    reached_refractory = removed_refractory = 0
    for o, run in runs.items():
        run.sort()                                              # by (t, i)
        t_last = state.t_last.get(o, -math.inf)
        for ti, i in run:
            reached_refractory += 1
            if ti - t_last >= rho:
                t_last = ti
                passed.setdefault(o, []).append(ti)
                s_events.append((i, o, ti))
            else:
                classes[i] = REFRACTORY
                removed_refractory += 1
        state.t_last[o] = t_last
    removed_support = 0
    if support:
        for i, o, ti in s_events:
            yi, xi = divmod(o, W)
            ok = False
            for dy in (-1, 0, 1):
                for dx in (-1, 0, 1):
                    ny, nx = yi + dy, xi + dx
                    if (dy == 0 and dx == 0) or ny < 0 or ny >= H or nx < 0 or nx >= W:
                        continue
                    q = ny * W + nx
                    times = passed.get(q, [])
                    k = bisect.bisect_right(times, ti)          # times[k - 1] is the largest one <= ti
                    if k > 0 and ti - times[k - 1] <= dt:
                        ok = True
                    seen = state.t_seen.get(q, -math.inf)       # the value from before this call: updated below
                    if seen <= ti and ti - seen <= dt:
                        ok = True
            if not ok:
                classes[i] = UNSUPPORTED
                removed_support += 1
    for o, times in passed.items():
        state.t_seen[o] = max(state.t_seen.get(o, -math.inf), times[-1])
    counters = dict(n_in=N)
    for k in range(1, 6):
        counters[NAMES[k]] = sum(1 for c in classes if c == k)
    kept = [i for i in range(N) if classes[i] == KEPT]
    counters['n_out'] = len(kept)
    return dict(classes=classes, kept=kept, counters=counters, reached_refractory=reached_refractory,
                removed_refractory=removed_refractory, reached_support=len(s_events) if support else 0,
                removed_support=removed_support)
