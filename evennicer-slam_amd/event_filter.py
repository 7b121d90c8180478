"""Event-stream denoising: what sits between a stream (event_stream.EventStream) and the accumulator.

    EventFilter      hot-pixel mask, refractory filter and background-activity (neighbour-support) filter with carried state;
                     one call filters one chunk: csrc/event_filter.hip on a HIP device, numpy (`filter_numpy`) on the CPU
    filter_stream    the one-shot form
    hot_pixels       learns the hot-pixel mask of a stream from its per-pixel event counts
    filter_numpy     the CPU route on numpy arrays

Model (include/enslam_hip.h holds it in full).  State per pixel, -inf after a reset: t_last, the time of the last event that
passed the refractory stage; t_seen, the largest time of the events that passed stages 0 and 1.  Every event gets the first
class that applies (CLASSES; 0 = kept):
    stage 0  SENSOR: x >= W or y >= H.  TIME: t not finite.  HOT: hot_mask set.  Otherwise the event is live.
    stage 1  refractory, ESIM's rule and the simulator's expression: the live events of a pixel in the order (t, stream
             position); an event passes iff t - t_last >= rho and then sets t_last = t, else it is REFRACTORY.
    stage 2  support, only with support_dt: an event that passed stage 1 is kept iff one of its up to eight spatial neighbours
             has a time t' <= t with t - t' <= dt, t' being the time of one of that neighbour's events that passed stage 1 in
             this chunk or its carried t_seen; else UNSUPPORTED.  Non-recursive: an UNSUPPORTED event still supports others.
All arithmetic is float64 comparisons and one subtraction, so both routes give the same bits.  Chunks must ascend in time:
the smallest live time of a call must not lie before the largest live time since the reset (EnslamError otherwise).  Chunked
filtering equals the one-call result whenever no time value is shared across a chunk boundary; an event at exactly the
boundary time in the earlier chunk whose only support is an equal-time event of the later chunk is UNSUPPORTED."""
import math

import numpy as np
import torch

from ._lib import EnslamError
from .event_stream import EventStream

CLASSES = ('kept', 'sensor', 'time', 'hot', 'refractory', 'unsupported')
KEPT, SENSOR, TIME, HOT, REFRACTORY, UNSUPPORTED = range(6)
COUNTERS = ('n_in', 'sensor', 'time', 'hot', 'refractory', 'unsupported', 'n_out')
_NEIGHBOURS = tuple((dy, dx) for dy in (-1, 0, 1) for dx in (-1, 0, 1) if (dy, dx) != (0, 0))


def _sensor(what, H, W):
    H, W = int(H), int(W)
    if H <= 0 or W <= 0 or H > 65536 or W > 65536 or H * W > (1 << 28):
        raise EnslamError(f"{what}: the sensor must have 1..65536 rows and columns and at most 2^28 pixels (got {H} x {W})")
    return H, W


def _classify_numpy(t, x, y, H, W, hot_mask):
    """stage 0 on numpy arrays: (cls uint8 [N], pix int64 [N] with -1 outside the sensor)"""
    x, y = x.astype(np.int64), y.astype(np.int64)
    inside = (x < W) & (y < H)
    pix = np.where(inside, y * W + x, -1)
    cls = np.zeros(t.shape[0], dtype=np.uint8)
    cls[~inside] = SENSOR
    cls[inside & ~np.isfinite(t)] = TIME
    if hot_mask is not None:
        hot = np.zeros(t.shape[0], dtype=bool)
        hot[inside] = np.asarray(hot_mask).reshape(-1)[pix[inside]] != 0
        cls[(cls == KEPT) & hot] = HOT
    return cls, pix


def filter_numpy(t, x, y, p, H, W, t_last, t_seen, refractory=0.0, support_dt=None, hot_mask=None):
    """The CPU route of one filter call on numpy arrays: returns (cls uint8 [N], keep bool [N]) and updates t_last and t_seen
    (float64 [H,W]) in place.  Vectorised: round k walks the k-th live event of every pixel that has one, the support stage is
    one vectorised binary search per neighbour."""
    rho = float(refractory)
    cls, pix = _classify_numpy(t, x, y, H, W, hot_mask)
    tl, ts = t_last.reshape(-1), t_seen.reshape(-1)
    live = np.flatnonzero(cls == KEPT)
    order = live[np.lexsort((t[live], pix[live]))]              # by (pixel, t, stream position): lexsort is stable
    po, to = pix[order], t[order]
    counts = np.bincount(po, minlength=H * W)
    starts = np.concatenate([[0], np.cumsum(counts)])
    by_len = np.argsort(-counts, kind='stable')                 # pixels, longest run first
    lens = counts[by_len]
    passed = np.zeros(order.shape[0], dtype=bool)
    for k in range(int(lens[0]) if lens.size else 0):
        m = int(np.searchsorted(-lens, -k, side='left'))        # the pixels with more than k live events
        px = by_len[:m]
        at = starts[px] + k
        tv = to[at]
        ok = tv - tl[px] >= rho
        tl[px[ok]] = tv[ok]
        passed[at] = ok
    cls[order[~passed]] = REFRACTORY
    s_order, s_pix, s_t = order[passed], po[passed], to[passed]
    s_counts = np.bincount(s_pix, minlength=H * W)
    s_starts = np.concatenate([[0], np.cumsum(s_counts)])
    if support_dt is not None and s_order.size:
        dt = float(support_dt)
        sy, sx = s_pix // W, s_pix % W
        supported = np.zeros(s_order.shape[0], dtype=bool)
        for dy, dx in _NEIGHBOURS:
            ny, nx = sy + dy, sx + dx
            valid = (ny >= 0) & (ny < H) & (nx >= 0) & (nx < W)
            q = np.where(valid, ny * W + nx, 0)
            lo, hi = s_starts[q].copy(), s_starts[q + 1].copy()
            first = lo.copy()
            while True:                                         # lo: one past the neighbour's last time <= t
                open_ = lo < hi
                if not open_.any():
                    break
                mid = (lo + hi) >> 1
                go = open_ & (s_t[np.minimum(mid, s_t.shape[0] - 1)] <= s_t)
                lo = np.where(go, mid + 1, lo)
                hi = np.where(open_ & ~go, mid, hi)
            found = valid & (lo > first)
            with np.errstate(invalid='ignore'):
                in_chunk = found & (s_t - s_t[np.maximum(lo - 1, 0)] <= dt)
                carried = valid & (ts[q] <= s_t) & (s_t - ts[q] <= dt)
            supported |= in_chunk | carried
        cls[s_order[~supported]] = UNSUPPORTED
    has = s_counts > 0
    ts[has] = np.maximum(ts[has], s_t[s_starts[1:][has] - 1])
    return cls, cls == KEPT


def _counters(cls):
    n = np.bincount(cls, minlength=len(CLASSES))
    out = dict(n_in=int(cls.shape[0]))
    out.update({name: int(n[k]) for k, name in enumerate(CLASSES) if k})
    out['n_out'] = int(n[KEPT])
    return out


class EventFilter:
    """The three filters with their carried state.  H, W: the sensor; refractory: rho >= 0 in seconds; support_dt: None
    switches the support stage off, a value >= 0 is its window in seconds; hot_mask: bool or uint8 [H,W] or None.  The state
    tensors `t_last` and `t_seen` (float64 [H,W] on `device`) are attributes; `reset()` sets them to -inf.

    filt(stream, return_classes=False) -> (EventStream of the kept events in stream order, stats[, classes]) filters one chunk;
    the stream must live on the filter's device and is left untouched.  stats: dict of COUNTERS; classes: uint8 [N]."""

    def __init__(self, H, W, refractory=0.0, support_dt=None, hot_mask=None, device='cpu'):
        self.H, self.W = _sensor("EventFilter", H, W)
        self.refractory = float(refractory)
        self.support_dt = None if support_dt is None else float(support_dt)
        if not (0.0 <= self.refractory < math.inf) or (self.support_dt is not None and not (0.0 <= self.support_dt < math.inf)):
            raise EnslamError(f"EventFilter: refractory and support_dt must be finite and not negative (got {refractory}, {support_dt})")
        self.device = torch.device(device)
        self.hot_mask = None
        if hot_mask is not None:
            m = torch.as_tensor(hot_mask)
            if tuple(m.shape) != (self.H, self.W):
                raise EnslamError(f"EventFilter: hot_mask must be [{self.H},{self.W}] (got {tuple(m.shape)})")
            self.hot_mask = (m != 0).to(torch.uint8).to(self.device).contiguous()
        self.last_path = None               # the ordering path of the last device call (functional.event_filter_order)
        self.reset()

    def reset(self):
        self.t_last = torch.full((self.H, self.W), -math.inf, dtype=torch.float64, device=self.device)
        self.t_seen = torch.full((self.H, self.W), -math.inf, dtype=torch.float64, device=self.device)
        self.t_max = -math.inf              # the largest live time since the reset

    def _check_order(self, t_min, t_max):
        if t_min < self.t_max:
            raise EnslamError(f"EventFilter: chunks must ascend in time (this chunk's smallest live time {t_min!r} lies before "
                              f"{self.t_max!r}, the largest so far); reset() starts a new stream")
        self.t_max = max(self.t_max, t_max)

    def __call__(self, stream, return_classes=False, mark=None):
        if stream.device != self.device:
            raise EnslamError(f"EventFilter: the stream is on {stream.device}, the filter on {self.device}")
        if self.device.type == 'cuda':
            from . import functional as EF
            t, x, y, p = stream.arrays()
            cls, pix, counts, flags = EF.event_pixel_counts(t, x, y, p, self.H, self.W, self.hot_mask)
            if mark is not None:
                mark('classify')
            live_t = t[cls == 0]
            if live_t.numel():
                self._check_order(float(live_t.min()), float(live_t.max()))
            order, starts, self.last_path = EF.event_filter_order(t, cls, pix, counts, flags, self.hot_mask)
            if mark is not None:
                mark('order')
            out, _ = EF.event_filter_stages(t, x, y, p, self.H, self.W, cls, pix, order, starts, self.t_last, self.t_seen,
                                            self.refractory, self.support_dt, mark)
            kept, stats = EventStream(*out), EF.event_class_counters(cls)
        else:
            t, x, y, p = stream.numpy()
            mask = None if self.hot_mask is None else self.hot_mask.numpy()
            live = _classify_numpy(t, x, y, self.H, self.W, mask)[0] == KEPT
            if live.any():
                self._check_order(float(t[live].min()), float(t[live].max()))
            cls, keep = filter_numpy(t, x, y, p, self.H, self.W, self.t_last.numpy(), self.t_seen.numpy(), self.refractory,
                                     self.support_dt, mask)
            kept, stats = EventStream(t[keep], x[keep], y[keep], p[keep]), _counters(cls)
            cls = torch.from_numpy(cls)
        return (kept, stats, cls) if return_classes else (kept, stats)


def filter_stream(stream, H, W, refractory=0.0, support_dt=None, hot_mask=None, return_classes=False):
    """One-shot: a fresh EventFilter on the stream's device applied to the whole stream."""
    return EventFilter(H, W, refractory, support_dt, hot_mask, device=stream.device)(stream, return_classes=return_classes)


def pixel_counts(stream, H, W):
    """int64 [H,W] on the stream's device: per pixel the number of events that are neither outside the sensor nor without a
    finite time."""
    H, W = _sensor("pixel_counts", H, W)
    if stream.device.type == 'cuda':
        from . import functional as EF
        return EF.event_pixel_counts(*stream.arrays(), H, W)[2].to(torch.int64)
    t, x, y, _ = stream.numpy()
    cls, pix = _classify_numpy(t, x, y, H, W, None)
    return torch.from_numpy(np.bincount(pix[cls == KEPT], minlength=H * W).reshape(H, W).astype(np.int64))


def hot_pixels(stream, H, W, max_events=None, rate=None):
    """(mask bool [H,W], counts int64 [H,W]) on the stream's device: a pixel is hot iff it has more than max_events events
    (`pixel_counts`).  rate (Hz) is a convenience: max_events = floor(rate * (t_max - t_min)) over the stream's finite times.
    Exactly one of max_events and rate is given."""
    if (max_events is None) == (rate is None):
        raise EnslamError("hot_pixels: give max_events or rate, one of them")
    counts = pixel_counts(stream, H, W)
    if max_events is None:
        if not (0.0 <= float(rate) < math.inf):
            raise EnslamError(f"hot_pixels: rate must be finite and not negative (got {rate})")
        finite = stream.t[torch.isfinite(stream.t)]
        span = float(finite.max()) - float(finite.min()) if finite.numel() else 0.0
        max_events = int(math.floor(float(rate) * span))
    if int(max_events) < 0:
        raise EnslamError(f"hot_pixels: max_events must not be negative (got {max_events})")
    return counts > int(max_events), counts


def filter_from_options(stream, H, W, refractory=None, support_dt=None, hot_rate=None, hot_max=None):
    """What tools/events_to_frames.py and the `data.event_filter` mapping of the readers do: with hot_rate or hot_max the mask
    is learned from the whole stream first, then the stream is filtered in one call.  Returns (EventStream, stats)."""
    if hot_rate is not None and hot_max is not None:
        raise EnslamError("event filter: give hot_rate or hot_max, not both")
    mask = None
    if hot_rate is not None or hot_max is not None:
        mask = hot_pixels(stream, H, W, max_events=None if hot_max is None else int(hot_max), rate=hot_rate)[0]
    return filter_stream(stream, H, W, 0.0 if refractory is None else float(refractory), support_dt, mask)
