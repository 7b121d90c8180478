"""Yardstick of the event-camera simulator: float64 numpy written from the model's statement, not from the library.

Model.  Y = (0.299 R + 0.587 G) + 0.114 B of values in [0, 1] (a grey image is its own Y); L = log(Y + eps).  One reference
level per pixel, L_ref: L of the first frame, then carried.  An interval is visited at K sub-steps s = 1..K; at each, with
d = L - L_ref:  d >= C_pos: n = floor(d / C_pos), pos += n, L_ref += n * C_pos;  else -d >= C_neg: n = floor(-d / C_neg),
neg += n, L_ref -= n * C_neg.  Counts leave as uint8 (-, +) saturated at 255; L_ref moves by the unsaturated n.

Every product and sum is its own numpy operation in the order written here ("scalar order": numpy never fuses them, and
the arrays only run the same scalar recipe on every pixel at once).  Grey images go through a 256-entry table of
log(v / 255 + eps); everything else calls np.log / np.sin on float64.

For the analytic route the yardstick also reports, per interval and pixel, how close the pixel came to a decision that an
ulp of sin / log could turn (`count_margin`, and `geo` of `render`)."""
import numpy as np


def table(eps):
    return np.log(np.arange(256, dtype=np.float64) / 255.0 + eps)


def level_of_image(img, eps):
    """L float64 [H,W] of a decoded uint8 image [H,W] or [H,W,3]"""
    img = np.asarray(img)
    assert img.dtype == np.uint8
    if img.ndim == 2:
        return table(eps)[img]
    r, g, b = (img[:, :, c].astype(np.float64) / 255.0 for c in range(3))
    y = 0.299 * r
    y = y + 0.587 * g
    y = y + 0.114 * b
    return np.log(y + eps)


class Sensor:
    """The sensor state of one case: L_ref plus the thresholds (scalars or [H,W] arrays)."""

    def __init__(self, first_level, c_pos, c_neg):
        self.ref = np.array(first_level, dtype=np.float64, copy=True)
        self.c_pos = np.broadcast_to(np.asarray(c_pos, dtype=np.float64), self.ref.shape)
        self.c_neg = np.broadcast_to(np.asarray(c_neg, dtype=np.float64), self.ref.shape)

    def begin(self):
        self.pos = np.zeros(self.ref.shape, dtype=np.float64)
        self.neg = np.zeros(self.ref.shape, dtype=np.float64)

    def visit(self, level):
        """one sub-step; returns the distance of d / C from the nearest event boundary (see `count_margin`)"""
        flat_ref, flat_pos, flat_neg = self.ref.reshape(-1), self.pos.reshape(-1), self.neg.reshape(-1)
        cp, cn, lv = self.c_pos.reshape(-1), self.c_neg.reshape(-1), np.asarray(level, dtype=np.float64).reshape(-1)
        d = lv - flat_ref
        margin = count_margin(d, cp, cn)
        rising = np.nonzero(d >= cp)[0]
        falling = np.nonzero(~(d >= cp) & (-d >= cn))[0]
        n = np.floor(d[rising] / cp[rising])
        flat_pos[rising] = flat_pos[rising] + n
        flat_ref[rising] = flat_ref[rising] + n * cp[rising]
        n = np.floor(-d[falling] / cn[falling])
        flat_neg[falling] = flat_neg[falling] + n
        flat_ref[falling] = flat_ref[falling] - n * cn[falling]
        return margin.reshape(self.ref.shape)

    def events(self):
        out = np.zeros(self.ref.shape + (2,), dtype=np.uint8)
        out[..., 0] = np.where(self.neg > 255.0, 255.0, self.neg)
        out[..., 1] = np.where(self.pos > 255.0, 255.0, self.pos)
        return out


def count_margin(d, cp, cn):
    """Per pixel: with q = d / C of the polarity d points to, the distance of q from the nearest integer at or above 1 -- from
    1 itself while q is below it.  A perturbation of L smaller than margin * C cannot change the count of this sub-step."""
    q = np.where(d >= 0.0, d / cp, -d / cn)
    nearest = np.maximum(np.rint(q), 1.0)
    return np.abs(q - nearest)


def step_images(sensor, prev, cur, K, eps):
    """One interval of the image route: events uint8 [H,W,2]; sensor.ref is advanced."""
    la, lb = level_of_image(prev, eps), level_of_image(cur, eps)
    delta = lb - la
    sensor.begin()
    for s in range(1, K + 1):
        frac = float(s) / float(K)
        sensor.visit(la + frac * delta)
    return sensor.events()


# ---- the analytic room ------------------------------------------------------------------------------------------------------
class Room:
    """Plain float64 arrays of a synthetic.BoxRoom (the yardstick takes numbers, not the library's object)."""

    def __init__(self, box_room):
        self.lo, self.hi = box_room.room_lo.numpy().copy(), box_room.room_hi.numpy().copy()
        self.blo = None if box_room.box_lo is None else box_room.box_lo.numpy().copy()
        self.bhi = None if box_room.box_hi is None else box_room.box_hi.numpy().copy()
        self.freq, self.phase = box_room.freq.numpy().copy(), box_room.phase.numpy().copy()


def render(room, pose, cam):
    """One view, step by step as BoxRoom.render / intersect / color_at: dict with color [H,W,3], t [H,W] (float64), on_box
    [H,W] and geo [H,W], the smallest relative gap among the decisions t1 vs t2, t1 vs 0, t1 vs t_wall (inf without a box)."""
    H, W = cam['H'], cam['W']
    pose = np.asarray(pose, dtype=np.float64)
    col_idx, row_idx = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    dx = (col_idx - cam['cx']) / cam['fx']
    dy = -(row_idx - cam['cy']) / cam['fy']
    dz = -np.ones((H, W))
    d, o = [], []
    for a in range(3):
        v = dx * pose[a, 0]
        v = v + dy * pose[a, 1]
        v = v + dz * pose[a, 2]
        d.append(v)
        o.append(pose[a, 3])
    safe = [np.where(np.abs(v) < 1e-12, 1e-12, v) for v in d]
    t_wall = np.full((H, W), np.inf)
    for a in range(3):
        t_wall = np.minimum(t_wall, np.maximum((room.lo[a] - o[a]) / safe[a], (room.hi[a] - o[a]) / safe[a]))
    t, on_box, geo = t_wall, np.zeros((H, W), dtype=bool), np.full((H, W), np.inf)
    if room.blo is not None:
        t1, t2 = np.full((H, W), -np.inf), np.full((H, W), np.inf)
        for a in range(3):
            ta, tb = (room.blo[a] - o[a]) / safe[a], (room.bhi[a] - o[a]) / safe[a]
            t1 = np.maximum(t1, np.minimum(ta, tb))
            t2 = np.minimum(t2, np.maximum(ta, tb))
        on_box = (t1 < t2) & (t1 > 0) & (t1 < t_wall)
        t = np.where(on_box, t1, t_wall)
        scale = np.maximum(np.maximum(np.abs(t1), np.abs(t2)), np.abs(t_wall))
        geo = np.minimum(np.minimum(np.abs(t1 - t2), np.abs(t1)), np.abs(t1 - t_wall)) / scale
    p = [o[a] + d[a] * t for a in range(3)]
    color = np.zeros((H, W, 3))
    for c in range(3):
        arg = p[0] * room.freq[c, 0]
        arg = arg + p[1] * room.freq[c, 1]
        arg = arg + p[2] * room.freq[c, 2]
        arg = arg + room.phase[c]
        color[:, :, c] = 0.5 + 0.45 * np.sin(arg)
    return dict(color=color, t=t, on_box=on_box, geo=geo)


def level_of_color(color, eps):
    y = 0.299 * color[:, :, 0]
    y = y + 0.587 * color[:, :, 1]
    y = y + 0.114 * color[:, :, 2]
    return np.log(y + eps)


def step_scene(sensor, room, poses, cam, eps):
    """One interval of the analytic route over the K poses `poses` ([K,3|4,4], the last is the frame): dict with events,
    color / depth (float32) / on_box of the last pose, and the two margins as [H,W] minima over the sub-steps: count (of
    d / C, `count_margin`) and geo (of the geometric decisions)."""
    sensor.begin()
    count = np.full(sensor.ref.shape, np.inf)
    geo = np.full(sensor.ref.shape, np.inf)
    view = None
    for pose in poses:
        view = render(room, pose, cam)
        count = np.minimum(count, sensor.visit(level_of_color(view['color'], eps)))
        geo = np.minimum(geo, view['geo'])
    return dict(events=sensor.events(), color=view['color'], depth=view['t'].astype(np.float32), on_box=view['on_box'],
                count_margin=count, geo_margin=geo)


def first_scene_level(room, pose, cam, eps):
    return level_of_color(render(room, pose, cam)['color'], eps)
