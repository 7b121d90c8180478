"""Event-camera simulator: a contrast-threshold sensor in the style of ESIM / vid2e, the source of the event images that the
`*_event` readers, the event network's trainer and the tracker's event term consume.

The model (include/enslam_hip.h repeats it; csrc/event_sim.hip runs it), all in float64:

    luminance   Y = (0.299 R + 0.587 G) + 0.114 B of values in [0, 1]; a grey image is its own Y
    level       L = log(Y + eps), eps = 1e-3
    state       one reference level per pixel, L_ref [H,W]: L of the first frame (which emits no events), then carried from
                interval to interval
    interval    frame k -> frame k+1 is visited at K sub-steps s = 1..K (default 8), the last one being frame k+1; at each,
                per pixel, with d = L - L_ref:
                    d >= C_pos:        n = floor(d / C_pos),  pos += n,  L_ref += n * C_pos
                    else -d >= C_neg:  n = floor(-d / C_neg), neg += n,  L_ref -= n * C_neg
                This closed form is the definition (a loop that fires one event at a time rounds differently).
    output      uint8 [H,W,2] = (-, +), the writers' order, saturated at 255; L_ref moves by the unsaturated n
    thresholds  scalars (default 0.2) or, with sigma_c > 0, per-pixel maps drawn ONCE per simulator from a seeded CPU generator:
                C * (1 + sigma_c * randn), clamped to at least 0.01

Two routes to L at a sub-step:

    images    any recorded sequence: two decoded uint8 images; L of a grey value from a 256-entry table, of an RGB pixel from
              its three bytes / 255.; sub-step s sees L_a + (s / K) * (L_b - L_a), in this operation order
    scene     synthetic.BoxRoom: the room is rendered at K poses between the two frames' (`interpolate_poses`: translation
              linear, rotation by quaternion slerp), exactly as BoxRoom.render does it

On a HIP device both run as one launch per interval (functional.event_sim_images / event_sim_boxroom).  On the CPU the same
methods run a numpy route of the same definition, operation for operation, so sequences can be written without a GPU.  The
two agree bit for bit wherever no transcendental function of the device decides (grey images, or `host_log=True`); the
device's log and sin are an ulp or two from numpy's, which moves a count only where d / C sits that close to an integer.

Time stamps (`stamps=(t_a, t_b)` on step_images / step_scene; csrc/event_stream.hip; include/enslam_hip.h states it too).
The counts and L_ref stay those of the closed form above.  At sub-step s let L_prev be the level seen at sub-step s - 1 (for
s = 1 the previous frame's level: L_a of the images route, the room rendered at the previous frame's pose), L_s this
sub-step's level and R the value of L_ref before the update.  The n events the pixel fires there are k = 1..n:

    X_k = R + k * C_pos (positive) or R - k * C_neg (negative), the product, then the sum
    f_k = (X_k - L_prev) / (L_s - L_prev), then limited to [0, 1] (below 0 or not a number: 0; above 1: 1)
    t_k = t_a + (((s - 1) + f_k) / K) * (t_b - t_a), in exactly this operation order

Linear level-crossing interpolation, as ESIM does it.  The limit is needed: over the image cases of tests/event_sim_cases.py
f reaches 1 + 2.2e-16 at one event and drops to 1.5e-16 at another, whose t_k rounds to t_a.  The stream leaves in
pixel-major order (row-major pixels, time-ordered within a pixel) as an event_stream.EventStream.

Sensor noise (`EventSimulator(..., noise=EventNoise(...))`; csrc/event_noise.hip; include/enslam_hip.h states it too).  Opt-in:
without a noise object everything above is untouched.  New state beside L_ref: t_last float64 [H,W], the time of the pixel's
last emitted event, -inf after `reset`.  Parameters: refractory rho >= 0 (s), leak_rate lambda >= 0 (Hz), shot_rate r >= 0 (Hz
per pixel and polarity), seed (uint64); the simulator counts the intervals since `reset` and passes the index along -- no
generator state is stored.  With delta = (t_b - t_a) / K the host computes g = lambda * delta and q = r * delta (q > 1 is
refused: raise K).  Per pixel with flat index o, at sub-step s = 1..K, in this order:

    1 leak (v2e's rule), if lambda > 0: L_ref = L_ref - g * C_pos, the product, then the difference; under constant light
      this yields positive events at lambda Hz
    2 signal candidates, exactly the time-stamped events above: R = L_ref, the closed form moves L_ref and gives n
      candidates of one polarity with X_k, f_k limited to [0, 1] and t_k in the operation order above
    3 shot-noise candidates, if r > 0: one Philox4x32-10 block (w0..w3) with key (seed & 0xffffffff, seed >> 32) and counter
      (o, interval, s, 0); u(w) = (w + 0.5) * 2^-32 (exact); a negative candidate exists iff u(w0) < q, at f = u(w1), a
      positive one iff u(w2) < q, at f = u(w3); both at t = t_a + (((s - 1) + f) / K) * (t_b - t_a); they do not move L_ref
    4 merge: the signal candidates in the order k = 1..n and the noise candidates in ascending t (on equal t the negative
      one first), two-way: the next noise candidate leaves before the next signal candidate iff its t is smaller
    5 refractory filter (ESIM's rule) in merged order: a candidate is emitted iff t - t_last >= rho (always for
      t_last = -inf) and then sets t_last = t; a suppressed signal candidate has still moved L_ref

The event image counts EMITTED events (saturated at 255); the stream holds them pixel-major, in merged order within a pixel.
With rho = lambda = r = 0 image, L_ref and stream equal the noise-free ones bit for bit.  On the device a sub-step walks at most
65536 signal candidates of a pixel; an interval beyond that is refused by the stream call (include/enslam_hip.h).  A stream
binned by frame times (event_stream.accumulate, tools/events_to_frames.py) returns these images, with one exception: a leak
event of a pixel whose level does not move has f = 0, at the first sub-step it carries the frame time t_a itself, and the
accumulator's rule gives an event on an edge to the frame before.

Not modelled: bandwidth-limited pixels, intensity-dependent noise rates, a reference level held in reset during
the refractory period, learned frame interpolation."""
import numpy as np
import torch

from ._lib import EnslamError

C_MIN = 0.01                        # floor of a per-pixel threshold


def grey_table(eps=1e-3):
    """log(v / 255 + eps) of the 256 grey values, float64: the table both routes read grey images through."""
    return np.log(np.arange(256, dtype=np.float64) / 255.0 + eps)


def luminance(rgb):
    """Y float64 [...] of float64 [...,3] values, summed in the model's order."""
    return (0.299 * rgb[..., 0] + 0.587 * rgb[..., 1]) + 0.114 * rgb[..., 2]


def log_intensity(image, eps=1e-3):
    """L float64 [H,W] of a decoded uint8 image: [H,W] / [H,W,1] (grey, through `grey_table`) or [H,W,3] (bytes / 255.)."""
    a = np.asarray(image)
    if a.ndim == 3 and a.shape[2] == 1:
        a = a[:, :, 0]
    if a.dtype != np.uint8 or a.ndim not in (2, 3) or (a.ndim == 3 and a.shape[2] != 3):
        raise EnslamError(f"event simulator: an image must be uint8 [H,W], [H,W,1] or [H,W,3] (got {a.dtype} {a.shape})")
    if a.ndim == 2:
        return grey_table(eps)[a]
    return np.log(luminance(a.astype(np.float64) / 255.0) + eps)


def sensor_update(L, ref, pos, neg, c_pos, c_neg):
    """The per-pixel update at one sub-step, in place on the float64 arrays ref, pos, neg (counts are kept unsaturated)."""
    d = L - ref
    up = d >= c_pos
    down = ~up & (-d >= c_neg)
    n_up = np.floor(d / c_pos)
    n_down = np.floor(-d / c_neg)
    pos[...] = np.where(up, pos + n_up, pos)
    neg[...] = np.where(down, neg + n_down, neg)
    ref[...] = np.where(up, ref + n_up * c_pos, np.where(down, ref - n_down * c_neg, ref))


def saturate(neg, pos):
    """uint8 [H,W,2] = (-, +) of two float64 count arrays"""
    return np.stack([np.minimum(neg, 255.0), np.minimum(pos, 255.0)], axis=-1).astype(np.uint8)


def stream_substep(s, K, t_a, t_b, R, n_pos, n_neg, c_pos, c_neg, L_prev, L):
    """The time-stamped events of sub-step s (1-based) of K, numpy route of the model above: R is L_ref before the update,
    n_pos / n_neg the counts the update added (float64 [H,W]), L_prev and L the levels at the previous and at this sub-step.
    Returns (pixel int64 [n], t float64 [n], p uint8 [n]) in pixel order, k ascending within a pixel."""
    shape = R.shape
    n = (n_pos + n_neg).reshape(-1)
    idx = np.nonzero(n > 0)[0]
    reps = n[idx].astype(np.int64)
    pix = np.repeat(idx, reps)
    first = np.cumsum(reps) - reps
    k = (np.arange(pix.size, dtype=np.int64) - np.repeat(first, reps) + 1).astype(np.float64)
    up = (n_pos.reshape(-1) > 0)[pix]
    cp = np.broadcast_to(np.asarray(c_pos, dtype=np.float64), shape).reshape(-1)[pix]
    cn = np.broadcast_to(np.asarray(c_neg, dtype=np.float64), shape).reshape(-1)[pix]
    step = k * np.where(up, cp, cn)
    r = R.reshape(-1)[pix]
    X = np.where(up, r + step, r - step)
    lp = L_prev.reshape(-1)[pix]
    with np.errstate(divide='ignore', invalid='ignore'):
        f = (X - lp) / (L.reshape(-1)[pix] - lp)
    f = np.where(f >= 0.0, f, 0.0)
    f = np.where(f > 1.0, 1.0, f)
    u = ((s - 1) + f) / K
    return pix, t_a + u * (t_b - t_a), up.astype(np.uint8)


def _stream_of(parts, W, device='cpu'):
    """EventStream of per-sub-step (pixel, t, p) lists: a stable sort by pixel keeps the sub-step order within a pixel"""
    from .event_stream import EventStream
    pix = np.concatenate([q[0] for q in parts]) if parts else np.zeros(0, dtype=np.int64)
    t = np.concatenate([q[1] for q in parts]) if parts else np.zeros(0)
    p = np.concatenate([q[2] for q in parts]) if parts else np.zeros(0, dtype=np.uint8)
    order = np.argsort(pix, kind='stable')
    pix = pix[order]
    return EventStream(t[order], (pix % W).astype(np.uint16), (pix // W).astype(np.uint16), p[order]).to(device)


class EventNoise:
    """Refractory period, leak and shot noise of an EventSimulator (the module docstring holds the model).  refractory in
    seconds, leak_rate in Hz, shot_rate in Hz per pixel and polarity, seed uint64."""

    def __init__(self, refractory=0.0, leak_rate=0.0, shot_rate=0.0, seed=0):
        self.refractory, self.leak_rate, self.shot_rate, self.seed = float(refractory), float(leak_rate), float(shot_rate), int(seed)
        for name in ('refractory', 'leak_rate', 'shot_rate'):
            v = getattr(self, name)
            if not (v >= 0.0 and v < float('inf')):
                raise EnslamError(f"EventNoise: {name} must be finite and not negative (got {v})")
        if not 0 <= self.seed < 2 ** 64:
            raise EnslamError(f"EventNoise: seed must fit uint64 (got {seed})")

    def params(self, interval):
        return dict(refractory=self.refractory, leak_rate=self.leak_rate, shot_rate=self.shot_rate, seed=self.seed, interval=interval)

    def __repr__(self):
        return (f"EventNoise(refractory={self.refractory}, leak_rate={self.leak_rate}, shot_rate={self.shot_rate}, "
                f"seed={self.seed})")


_PHILOX_M0, _PHILOX_M1, _PHILOX_W0, _PHILOX_W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85


def philox4x32(counter, key):
    """Philox4x32-10 on arrays: counter = four and key = two uint64 arrays (or ints) of 32-bit values; returns the four words
    of the block as uint64 arrays holding 32-bit values."""
    m32 = np.uint64(0xFFFFFFFF)
    c = [np.asarray(v, dtype=np.uint64) & m32 for v in counter]
    k = [np.asarray(v, dtype=np.uint64) & m32 for v in key]
    for _ in range(10):
        p0, p1 = np.uint64(_PHILOX_M0) * c[0], np.uint64(_PHILOX_M1) * c[2]     # 32 x 32 bits: exact in uint64
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k[0], p1 & m32, (p0 >> np.uint64(32)) ^ c[3] ^ k[1], p0 & m32]
        k = [(k[0] + np.uint64(_PHILOX_W0)) & m32, (k[1] + np.uint64(_PHILOX_W1)) & m32]
    return c


def _uniform(w):
    return (w.astype(np.float64) + 0.5) * (1.0 / 4294967296.0)


def _running_max(t, pix):
    """per run of equal `pix` (sorted), the running maximum of t: the key that keeps a run in its own order in a merge"""
    out = t.copy()
    if out.size < 2:
        return out
    same = np.concatenate([[False], pix[1:] == pix[:-1]])
    while True:
        before = np.concatenate([out[:1], out[:-1]])
        bad = same & (before > out)
        if not bad.any():
            return out
        out[bad] = before[bad]


def noisy_substep(s, K, t_a, t_b, ref, t_last, neg, pos, c_pos, c_neg, L_prev, L, noise, interval):
    """Sub-step s (1-based) of K of the noisy sensor, numpy route of the model above, in place on the float64 [H,W] arrays ref,
    t_last and the emitted counts neg / pos.  Returns (pixel int64 [n], t float64 [n], p uint8 [n]) of the emitted events in
    pixel order, merged order within a pixel."""
    H, W = ref.shape
    delta = (t_b - t_a) / K
    g, q = noise.leak_rate * delta, noise.shot_rate * delta
    cp = np.broadcast_to(np.asarray(c_pos, dtype=np.float64), ref.shape)
    if noise.leak_rate > 0.0:
        ref[...] = ref - g * cp
    R, n_pos, n_neg = ref.copy(), np.zeros_like(ref), np.zeros_like(ref)
    sensor_update(L, ref, n_pos, n_neg, c_pos, c_neg)
    pix, t, p = stream_substep(s, K, t_a, t_b, R, n_pos, n_neg, c_pos, c_neg, L_prev, L)
    key, cls = _running_max(t, pix), np.zeros(pix.size, dtype=np.int64)
    if noise.shot_rate > 0.0:
        o = np.arange(H * W, dtype=np.uint64)
        w = philox4x32((o, np.uint64(interval), np.uint64(s), np.uint64(0)), (noise.seed & 0xFFFFFFFF, noise.seed >> 32))
        for exists, frac, polarity in ((w[0], w[1], 0), (w[2], w[3], 1)):
            idx = np.nonzero(_uniform(exists) < q)[0]
            u = ((s - 1) + _uniform(frac[idx])) / K
            tn = t_a + u * (t_b - t_a)
            pix, t, key = np.concatenate([pix, idx]), np.concatenate([t, tn]), np.concatenate([key, tn])
            p = np.concatenate([p, np.full(idx.size, polarity, dtype=np.uint8)])
            cls = np.concatenate([cls, np.full(idx.size, 1 + polarity, dtype=np.int64)])
    order = np.lexsort((np.arange(pix.size), cls, key, pix))
    pix, t, p = pix[order], t[order], p[order]
    # the refractory filter is sequential within a pixel: rank j of every pixel's run at once
    count = np.bincount(pix, minlength=H * W)
    start = np.cumsum(count) - count
    keep = np.zeros(pix.size, dtype=bool)
    last, rho = t_last.reshape(-1), noise.refractory
    live = np.nonzero(count > 0)[0]
    j = 0
    while live.size:
        at = start[live] + j
        ok = t[at] - last[live] >= rho
        keep[at[ok]] = True
        last[live[ok]] = t[at[ok]]
        j += 1
        live = live[count[live] > j]
    pix, t, p = pix[keep], t[keep], p[keep]
    pos += np.bincount(pix[p == 1], minlength=H * W).reshape(H, W)
    neg += np.bincount(pix[p == 0], minlength=H * W).reshape(H, W)
    return pix, t, p


def _stamps(stamps):
    try:
        t_a, t_b = (float(v) for v in stamps)
    except (TypeError, ValueError):
        raise EnslamError("EventSimulator: stamps must be the pair (t_a, t_b) of the interval's frame times") from None
    if not (t_a <= t_b and abs(t_a) < float('inf') and abs(t_b) < float('inf')):
        raise EnslamError(f"EventSimulator: stamps must be finite with t_a <= t_b (got {t_a}, {t_b})")
    return t_a, t_b


def render_boxroom(room, c2w, cam):
    """synthetic.BoxRoom.render in numpy with every sum written out in a fixed order -- the order of csrc/event_sim.hip:
    (color float64 [H,W,3], t float64 [H,W]) of the view c2w ([3|4,4] float64)."""
    H, W, fx, fy, cx, cy = (cam[k] for k in ('H', 'W', 'fx', 'fy', 'cx', 'cy'))
    P = np.asarray(c2w, dtype=np.float64)
    i, j = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    dirs = ((i - cx) / fx, -(j - cy) / fy, -np.ones_like(i))
    d = [(dirs[0] * P[a, 0] + dirs[1] * P[a, 1]) + dirs[2] * P[a, 2] for a in range(3)]
    o = [P[a, 3] for a in range(3)]
    dc = [np.where(np.abs(v) < 1e-12, 1e-12, v) for v in d]
    lo, hi = room.room_lo.numpy(), room.room_hi.numpy()
    t = None
    for a in range(3):
        far = np.maximum((lo[a] - o[a]) / dc[a], (hi[a] - o[a]) / dc[a])
        t = far if t is None else np.minimum(t, far)
    if room.box_lo is not None:
        blo, bhi = room.box_lo.numpy(), room.box_hi.numpy()
        t1 = t2 = None
        for a in range(3):
            u, v = (blo[a] - o[a]) / dc[a], (bhi[a] - o[a]) / dc[a]
            near, far = np.minimum(u, v), np.maximum(u, v)
            t1 = near if t1 is None else np.maximum(t1, near)
            t2 = far if t2 is None else np.minimum(t2, far)
        t = np.where((t1 < t2) & (t1 > 0) & (t1 < t), t1, t)
    p = [o[a] + d[a] * t for a in range(3)]
    f, ph = room.freq.numpy(), room.phase.numpy()
    col = [0.5 + 0.45 * np.sin(((p[0] * f[c, 0] + p[1] * f[c, 1]) + p[2] * f[c, 2]) + ph[c]) for c in range(3)]
    return np.stack(col, axis=-1), t


def interpolate_poses(c2w_a, c2w_b, K):
    """The K poses s = 1..K of an interval, float64 [K,4,4]: translation a + (s / K) * (b - a), rotation by quaternion slerp
    of the two rotations along the shorter arc; the pose of s = K is c2w_b itself.  Host arithmetic (numpy float64)."""
    from .datasets import matrix_quaternion, quaternion_matrix
    A, B = (np.asarray(torch.as_tensor(m).double().numpy() if torch.is_tensor(m) else m, dtype=np.float64) for m in (c2w_a, c2w_b))
    if K < 1:
        raise EnslamError(f"interpolate_poses: K must be at least 1 (got {K})")
    qa, qb = matrix_quaternion(A[:3, :3]), matrix_quaternion(B[:3, :3])
    qa, qb = qa / np.linalg.norm(qa), qb / np.linalg.norm(qb)
    dot = float(np.dot(qa, qb))
    if dot < 0.0:
        qb, dot = -qb, -dot
    theta = float(np.arccos(min(dot, 1.0)))
    out = np.zeros((K, 4, 4), dtype=np.float64)
    out[:, 3, 3] = 1.0
    for s in range(1, K + 1):
        if s == K:
            out[s - 1, :3, :] = B[:3, :]
            continue
        u = s / K
        if theta < 1e-8:                                            # sin(theta) ~ theta: the chord is the arc
            q = qa + u * (qb - qa)
        else:
            q = (np.sin((1.0 - u) * theta) * qa + np.sin(u * theta) * qb) / np.sin(theta)
        out[s - 1, :3, :3] = quaternion_matrix(q)
        out[s - 1, :3, 3] = A[:3, 3] + u * (B[:3, 3] - A[:3, 3])
    return out


class EventSimulator:
    """One simulated sensor of H x W pixels: thresholds, sub-step count and the carried state.

        sim = EventSimulator(H, W, device='cuda:0')
        sim.reset(first_image)                              # or sim.reset((room, c2w, cam))
        events = sim.step_images(prev_image, cur_image)     # uint8 [H,W,2] = (-, +) on `device`
        events = sim.step_scene(room, c2w_prev, c2w_cur, cam)

    device: a HIP device runs csrc/event_sim.hip, 'cpu' the numpy route of the same definition.
    noise: an EventNoise switches to the noisy sensor (csrc/event_noise.hip): every step then needs `stamps`, and
    `stream=False` on a step returns the image alone (one launch on the device)."""

    def __init__(self, H, W, c_pos=0.2, c_neg=0.2, sigma_c=0.0, substeps=8, eps=1e-3, seed=0, device='cuda:0', noise=None):
        self.H, self.W, self.substeps, self.eps = int(H), int(W), int(substeps), float(eps)
        self.c_pos, self.c_neg, self.sigma_c, self.seed = float(c_pos), float(c_neg), float(sigma_c), int(seed)
        self.device = torch.device(device)
        if self.H <= 0 or self.W <= 0 or self.substeps < 1:
            raise EnslamError(f"EventSimulator: H, W and substeps must be positive (got {H}, {W}, {substeps})")
        if not (self.c_pos > 0 and self.c_neg > 0 and self.eps > 0 and self.sigma_c >= 0):
            raise EnslamError("EventSimulator: c_pos, c_neg and eps must be positive, sigma_c not negative")
        if self.device.type == 'cuda':
            from . import functional as EF
            from . import _lib as L
            kmax = L.lib().enslam_event_sim_max_substeps()
            if self.substeps > kmax:
                raise EnslamError(f"EventSimulator: at most {kmax} sub-steps on the device (got {substeps})")
            self._EF = EF
        self.c_pos_map = self.c_neg_map = None
        if self.sigma_c > 0:
            rng = np.random.default_rng(self.seed)
            maps = [np.maximum(c * (1.0 + self.sigma_c * rng.standard_normal((self.H, self.W))), C_MIN) for c in (self.c_pos, self.c_neg)]
            self.c_pos_map, self.c_neg_map = (torch.from_numpy(m).to(self.device) for m in maps)
        self._lut = torch.from_numpy(grey_table(self.eps)).to(self.device)
        self._ref = None
        if noise is not None and not isinstance(noise, EventNoise):
            raise EnslamError(f"EventSimulator: noise must be an EventNoise (got {type(noise).__name__})")
        self.noise, self._t_last, self._interval = noise, None, 0

    # ---- state -------------------------------------------------------------------------------------------------------------
    @property
    def state(self):
        """L_ref, float64 [H,W] on the simulator's device (None before `reset`); the live tensor, updated in place."""
        return self._ref

    @property
    def last_event_time(self):
        """t_last, float64 [H,W] on the simulator's device: the time of every pixel's last emitted event, -inf where there was
        none since `reset` (None without a noise object or before `reset`); the live tensor."""
        return self._t_last

    @property
    def on_device(self):
        return self.device.type == 'cuda'

    def _need_state(self):
        if self._ref is None:
            raise EnslamError("EventSimulator: reset() with the first frame before the first step")

    def _thresholds(self):
        """(c_pos, c_neg) for the numpy route: the maps where there are any"""
        return (self.c_pos if self.c_pos_map is None else self.c_pos_map.numpy(),
                self.c_neg if self.c_neg_map is None else self.c_neg_map.numpy())

    def _kw(self):
        return dict(eps=self.eps, c_pos=self.c_pos, c_neg=self.c_neg, c_pos_map=self.c_pos_map, c_neg_map=self.c_neg_map)

    def _image(self, image):
        """a decoded image as the kernel takes it: uint8 [H,W] or [H,W,3] on the device"""
        t = image if torch.is_tensor(image) else torch.from_numpy(np.ascontiguousarray(image))
        if t.dim() == 3 and t.shape[2] == 1:
            t = t[:, :, 0]
        if t.dtype != torch.uint8 or tuple(t.shape[:2]) != (self.H, self.W):
            raise EnslamError(f"EventSimulator: an image must be uint8 [{self.H},{self.W}] or [{self.H},{self.W},3] (got {t.dtype} "
                              f"{tuple(t.shape)})")
        return t.to(self.device).contiguous()

    def _host_level(self, image):
        a = image.cpu().numpy() if torch.is_tensor(image) else np.asarray(image)
        if a.dtype != np.uint8 or tuple(a.shape[:2]) != (self.H, self.W):
            raise EnslamError(f"EventSimulator: an image must be uint8 [{self.H},{self.W}] or [{self.H},{self.W},3] (got {a.dtype} "
                              f"{a.shape})")
        return log_intensity(a, self.eps)

    def _check_cam(self, cam):
        if int(cam['H']) != self.H or int(cam['W']) != self.W:
            raise EnslamError(f"EventSimulator: the camera is {cam['H']} x {cam['W']}, the sensor {self.H} x {self.W}")

    # ---- the first frame ---------------------------------------------------------------------------------------------------
    def reset(self, first, host_log=False):
        """State := L of the first frame, which emits no events.  first: a decoded image, or (room, c2w, cam)."""
        scene = isinstance(first, (tuple, list)) and len(first) == 3 and hasattr(first[0], 'room_lo')
        if scene:
            self._check_cam(first[2])
        if self.noise is not None:
            self._t_last = torch.full((self.H, self.W), float('-inf'), dtype=torch.float64, device=self.device)
            self._interval = 0
        if not self.on_device:
            if scene:
                room, c2w, cam = first
                L = np.log(luminance(render_boxroom(room, _pose64(c2w), cam)[0]) + self.eps)
            else:
                L = self._host_level(first)
            self._ref = torch.from_numpy(np.ascontiguousarray(L))
            return self
        self._ref = torch.empty((self.H, self.W), dtype=torch.float64, device=self.device)
        if scene:
            room, c2w, cam = first
            self._EF.event_sim_boxroom(room, _pose64(c2w)[None], cam, self._ref, init=True, **self._kw())
        elif host_log:
            self._ref.copy_(torch.from_numpy(self._host_level(first)))
        else:
            img = self._image(first)
            self._EF.event_sim_images(img, img, self._ref, substeps=1, lut=self._lut, init=True, **self._kw())
        return self

    # ---- one interval ------------------------------------------------------------------------------------------------------
    def _interval_stamps(self, stamps, what, want_frame=False):
        """the interval's stamps, checked: None without noise means the count image alone"""
        if want_frame and (self.noise is not None or stamps is not None):
            raise EnslamError("EventSimulator.step_scene: stamps and want_frame are not combined")
        if self.noise is None:
            return None if stamps is None else _stamps(stamps)
        if stamps is None:
            raise EnslamError(f"EventSimulator.{what}: a simulator with noise needs stamps = (t_a, t_b): the refractory period and "
                              "the rates are in seconds")
        stamps = _stamps(stamps)
        q = self.noise.shot_rate * ((stamps[1] - stamps[0]) / self.substeps)
        if q > 1.0:
            raise EnslamError(f"EventSimulator.{what}: shot_rate * sub-step length is {q} > 1: raise the number of sub-steps")
        if self._interval >= 2 ** 32:
            raise EnslamError("EventSimulator: the interval counter is uint32; reset() the simulator")
        return stamps

    def _step(self, source, stamps, stream):
        """One interval from its level source -- on the device (route, the leading arguments of functional.event_*_<route>,
        keywords), on the CPU ('numpy', then the arguments of `_walk`) -- through the frame, the stream or the noisy pass."""
        route, head, kw = source[0], source[1], source[2]
        if route == 'numpy':
            return self._walk(*source[1:], stamps, stream)
        if self.noise is not None:
            out = getattr(self._EF, 'event_noisy_' + route)(*head, self._ref, self._t_last, stamps, self.noise.params(self._interval),
                                                            stream=stream, **kw, **self._kw())
            self._interval += 1
            return self._with_stream(out) if stream else out
        if stamps is not None:
            return self._with_stream(getattr(self._EF, 'event_stream_' + route)(*head, self._ref, stamps, **kw, **self._kw()))
        return getattr(self._EF, 'event_sim_' + route)(*head, self._ref, **kw, **self._kw())

    def _walk(self, levels, first, frame, stamps, stream):
        """The numpy route of all three passes: one walk over the sub-steps' level images.  first: the level before the first
        (stamps only); frame: None, or where [colour, ray parameter] of the last sub-step are once `levels` is used up."""
        ref = self._ref.numpy()
        pos, neg = np.zeros_like(ref), np.zeros_like(ref)
        cp, cn = self._thresholds()
        K, parts, L_before = self.substeps, [], first
        for s, L in enumerate(levels, start=1):
            if self.noise is not None:
                parts.append(noisy_substep(s, K, stamps[0], stamps[1], ref, self._t_last.numpy(), neg, pos, cp, cn, L_before, L,
                                           self.noise, self._interval))
            elif stamps is None:
                sensor_update(L, ref, pos, neg, cp, cn)
            else:
                R, pos0, neg0 = ref.copy(), pos.copy(), neg.copy()
                sensor_update(L, ref, pos, neg, cp, cn)
                parts.append(stream_substep(s, K, stamps[0], stamps[1], R, pos - pos0, neg - neg0, cp, cn, L_before, L))
            L_before = L
        if self.noise is not None:
            self._interval += 1
        events = torch.from_numpy(saturate(neg, pos))
        if frame is not None:
            return events, torch.from_numpy(frame[0]), torch.from_numpy(frame[1].astype(np.float32))
        if stamps is None or (self.noise is not None and not stream):
            return events
        return events, _stream_of(parts, self.W)

    def step_images(self, prev, cur, host_log=False, stamps=None, stream=True):
        """Events uint8 [H,W,2] = (-, +) between two decoded images (numpy arrays, or tensors on the device).  host_log: on a
        device, take the two level images from the host (numpy's log) instead of the kernel's -- bit-equal to the CPU route
        for RGB images too, at the price of two float64 uploads.  stamps = (t_a, t_b), the times of the two frames: returns
        (events, EventStream) -- the same image and state, and the time-stamped events in pixel-major order.  With a noise object
        stamps are required; stream=False then returns the image alone."""
        self._need_state()
        stamps = self._interval_stamps(stamps, 'step_images')
        K = self.substeps
        if not self.on_device:
            La, Lb = self._host_level(prev), self._host_level(cur)
            dL = Lb - La
            source = ('numpy', (La + (s / K) * dL for s in range(1, K + 1)), La, None)
        elif host_log:
            levels = tuple(torch.from_numpy(self._host_level(im)).to(self.device) for im in (prev, cur))
            source = ('images', (None, None), dict(substeps=K, levels=levels))
        else:
            a, b = self._image(prev), self._image(cur)
            if a.shape != b.shape:
                raise EnslamError(f"EventSimulator: the two images differ in shape ({tuple(a.shape)}, {tuple(b.shape)})")
            source = ('images', (a, b), dict(substeps=K, lut=self._lut))
        return self._step(source, stamps, stream)

    @staticmethod
    def _with_stream(out):
        from .event_stream import EventStream
        events, arrays = out
        return events, EventStream(*arrays)

    def step_scene(self, room, c2w_prev, c2w_cur, cam, want_frame=False, stamps=None, stream=True):
        """Events of the interval between two views of `room`; with want_frame also (color float64 [H,W,3], depth float32
        [H,W]) of c2w_cur, what room.render(c2w_cur, cam) returns.  stamps = (t_a, t_b), the times of the two views: returns
        (events, EventStream) -- the room is then rendered at c2w_prev as well, for the level the first sub-step starts from
        (want_frame is not combined with it)."""
        self._need_state()
        self._check_cam(cam)
        poses = interpolate_poses(_pose64(c2w_prev), _pose64(c2w_cur), self.substeps)
        stamps = self._interval_stamps(stamps, 'step_scene', want_frame)
        first = None
        if stamps is not None:                                      # the previous frame's pose, for the level before sub-step 1
            first = np.eye(4, dtype=np.float64)
            first[:3, :] = _pose64(c2w_prev)[:3, :]
        if self.on_device:
            source = ('boxroom', (room, poses if first is None else np.concatenate([first[None], poses], axis=0), cam),
                      dict(want_frame=want_frame) if stamps is None else {})
        else:
            frame = [None, None]

            def level(P):
                frame[:] = render_boxroom(room, P, cam)
                return np.log(luminance(frame[0]) + self.eps)
            source = ('numpy', (level(P) for P in poses), None if first is None else level(first), frame if want_frame else None)
        return self._step(source, stamps, stream)


def _pose64(c2w):
    return (c2w.detach().cpu().double().numpy() if torch.is_tensor(c2w) else np.asarray(c2w, dtype=np.float64))
