"""Time-stamped event streams: what an event camera produces, (t, x, y, polarity) per event.

    EventStream          the four arrays (t float64 seconds, x, y uint16, p uint8 with 1 = positive) as torch tensors on one
                         device; `time_sorted()`, `.npz` save / load
    read_events_txt      the RPG / DAVIS text layout: one event per line `t x y p`, t in seconds, p in {0, 1}; read in chunks
    write_events_txt
    accumulate           bins a stream into count images uint8 [B,H,W,2] = (-, +), what the `*_event` readers and writers use:
                         csrc/event_stream.hip on a HIP device (functional.event_accumulate), np.add.at under the same rule
                         on the CPU, so that sequences can be prepared without a GPU
    frame_edges          bin edges from frame times: every gap-th frame, each kept interval split into `density` equal parts

Bin rule (include/enslam_hip.h): event t goes to bin b where edges[b] < t <= edges[b+1] -- an event at a frame's own time
belongs to the interval that ends there.  Events with x >= W or y >= H are dropped and counted as `sensor`; the others outside
every bin as `time`.  The sums are integer sums: the result does not depend on the order of the stream.

The simulator side (event_sim.EventSimulator.step_images / step_scene with `stamps`) returns streams in pixel-major order:
row-major pixels, time-ordered within a pixel.  `time_sorted()` is a stable sort on t, so ties keep the pixel order."""
import numpy as np
import torch

from ._lib import EnslamError

_DTYPES = (('t', torch.float64), ('x', torch.uint16), ('y', torch.uint16), ('p', torch.uint8))


def _take(a, order):
    """a[order] for the stream dtypes (uint16 is indexed through its int16 view: the bits are what moves)"""
    if a.dtype == torch.uint16:
        return a.view(torch.int16)[order].view(torch.uint16)
    return a[order]


class EventStream:
    """N events as four tensors on one device: t float64 [N] seconds, x, y uint16 [N], p uint8 [N] (1 = positive)."""

    def __init__(self, t, x, y, p):
        arrays = []
        for (name, dtype), a in zip(_DTYPES, (t, x, y, p)):
            a = a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(np.asarray(a)))
            if a.dtype != dtype:
                if name != 't' and a.numel() and (int(a.min()) < 0 or int(a.max()) > (1 if name == 'p' else 65535)):
                    raise EnslamError(f"EventStream: {name} does not fit its range")
                a = a.to(torch.int32).to(dtype) if name != 't' else a.to(dtype)
            arrays.append(a.contiguous())
        self.t, self.x, self.y, self.p = arrays
        if any(a.dim() != 1 or a.shape != self.t.shape or a.device != self.t.device for a in arrays):
            raise EnslamError("EventStream: t, x, y, p must be one-dimensional, of one length and on one device")

    def __len__(self):
        return int(self.t.shape[0])

    @property
    def device(self):
        return self.t.device

    def arrays(self):
        return self.t, self.x, self.y, self.p

    def to(self, device):
        return EventStream(*(a.to(device) for a in self.arrays()))

    def numpy(self):
        """(t, x, y, p) as numpy arrays"""
        return tuple(a.cpu().numpy() for a in self.arrays())

    def take(self, order):
        order = torch.as_tensor(order, device=self.device)
        return EventStream(*(_take(a, order) for a in self.arrays()))

    def time_sorted(self):
        """The stream in time order: a stable sort on t, so events of one time keep their order."""
        if len(self) == 0:
            return self
        return self.take(torch.sort(self.t, stable=True).indices)

    @staticmethod
    def empty(device='cpu'):
        return EventStream(*(torch.empty(0, dtype=d, device=device) for _, d in _DTYPES))

    @staticmethod
    def concatenate(streams):
        streams = list(streams)
        if not streams:
            return EventStream.empty()
        return EventStream(*(torch.cat([getattr(s, n) for s in streams]) for n, _ in _DTYPES))

    def save(self, path):
        """One .npz with the arrays t, x, y, p."""
        t, x, y, p = self.numpy()
        with open(path, 'wb') as f:
            np.savez(f, t=t, x=x, y=y, p=p)

    @staticmethod
    def load(path, device='cpu'):
        with np.load(path) as z:
            return EventStream(z['t'], z['x'], z['y'], z['p']).to(device)


def read_events_txt(path, chunk=1 << 20, device='cpu'):
    """The RPG / DAVIS `events.txt`: one event per line `t x y p` (t seconds, p 0 or 1); empty lines and lines that start with
    '#' are skipped.  The file is parsed `chunk` lines at a time, so the text is never held whole."""
    parts = []

    def flush(rows):
        if rows:
            a = np.array(rows, dtype=np.float64)
            if a.ndim != 2 or a.shape[1] != 4:
                raise EnslamError(f"{path}: every event line holds four fields `t x y p`")
            xy, pol = a[:, 1:3], a[:, 3]
            if (xy < 0).any() or (xy > 65535).any() or (xy != np.rint(xy)).any() or ((pol != 0) & (pol != 1)).any():
                raise EnslamError(f"{path}: x and y must be integers in 0..65535 and p 0 or 1")
            parts.append(EventStream(a[:, 0].copy(), xy[:, 0].astype(np.uint16), xy[:, 1].astype(np.uint16), pol.astype(np.uint8)))

    rows = []
    with open(path, 'r') as f:
        for line in f:
            s = line.strip()
            if not s or s[0] == '#':
                continue
            fields = s.split()
            if len(fields) != 4:
                raise EnslamError(f"{path}: every event line holds four fields `t x y p` (got {s!r})")
            rows.append([float(v) for v in fields])             # float() reads back what repr() wrote, bit for bit
            if len(rows) >= chunk:
                flush(rows)
                rows = []
    flush(rows)
    return EventStream.concatenate(parts).to(device)


def write_events_txt(path, stream, chunk=1 << 20):
    """One line `t x y p` per event; t as repr(float), the shortest text that reads back to the same float64."""
    t, x, y, p = stream.numpy()
    with open(path, 'w') as f:
        for i in range(0, len(t), chunk):
            f.write(''.join(f"{tt!r} {xx} {yy} {pp}\n" for tt, xx, yy, pp in
                            zip(t[i:i + chunk].tolist(), x[i:i + chunk].tolist(), y[i:i + chunk].tolist(), p[i:i + chunk].tolist())))


def load_stream(path, device='cpu'):
    """A stream from `.npz` (EventStream.save) or, any other name, from the text layout."""
    return EventStream.load(path, device) if str(path).endswith('.npz') else read_events_txt(path, device=device)


def read_stamps(path):
    """Frame times, float64 [n]: the first field of every line that is neither empty nor a '#' comment (the `images.txt` of
    the RPG / DAVIS recordings, TUM's rgb.txt, or a plain list of numbers)."""
    out = []
    with open(path, 'r') as f:
        for line in f:
            s = line.strip()
            if s and s[0] != '#':
                out.append(float(s.replace(',', ' ').split()[0]))
    return np.array(out, dtype=np.float64)


def frame_edges(stamps, gap=1, density=1):
    """Bin edges float64 from frame times: the frames 0, gap, 2 gap, ... are kept and each kept interval [a, b] is split into
    `density` equal parts a + (j / density) * (b - a), j = 0..density - 1, the last edge being the last kept frame's time
    itself.  (n_kept - 1) * density bins: what RPG_event (density 1) and RPG_event_dense expect for n_kept images."""
    s = np.asarray(stamps, dtype=np.float64).reshape(-1)
    gap, density = int(gap), int(density)
    if gap < 1 or density < 1:
        raise EnslamError(f"frame_edges: gap and density must be at least 1 (got {gap}, {density})")
    kept = s[::gap]
    if kept.size < 2:
        raise EnslamError(f"frame_edges: {s.size} frame times at gap {gap} leave fewer than two frames")
    if not bool(np.all(kept[:-1] <= kept[1:])):
        raise EnslamError("frame_edges: the frame times must be ascending")
    edges = []
    for a, b in zip(kept[:-1].tolist(), kept[1:].tolist()):
        edges.extend(a + (j / density) * (b - a) for j in range(density))
    edges.append(float(kept[-1]))
    return np.array(edges, dtype=np.float64)


def accumulate_numpy(t, x, y, p, edges, H, W):
    """The CPU route of `accumulate` on numpy arrays: (counts uint8 [B,H,W,2], unsaturated int64 [B,H,W,2], (time, sensor))."""
    e = np.asarray(edges, dtype=np.float64)
    B = e.size - 1
    full = np.zeros((B, H, W, 2), dtype=np.int64)
    x, y = x.astype(np.int64), y.astype(np.int64)
    inside = (x < W) & (y < H)
    b = np.searchsorted(e, t, side='left') - 1              # edges[b] < t <= edges[b+1]
    timed = (b >= 0) & (b < B) & ~np.isnan(t)
    keep = inside & timed
    np.add.at(full, (b[keep], y[keep], x[keep], (p[keep] != 0).astype(np.int64)), 1)
    return np.minimum(full, 255).astype(np.uint8), full, (int((inside & ~timed).sum()), int((~inside).sum()))


def accumulate(stream, edges, H, W, want_unsaturated=False, with_dropped=False):
    """Count images of a stream: uint8 [B,H,W,2] = (-, +) saturated at 255 on the stream's device, B = len(edges) - 1, under
    the bin rule of this module.  A stream on a HIP device runs the kernel, one on the CPU numpy.  want_unsaturated: also the
    unsaturated counts (uint32 on a device, int64 on the CPU); with_dropped: also the pair (dropped by time, dropped by
    sensor).  Returns counts, or the tuple (counts[, unsaturated][, dropped])."""
    e = np.asarray(edges.cpu() if torch.is_tensor(edges) else edges, dtype=np.float64).reshape(-1)
    H, W = int(H), int(W)
    if e.size < 2 or H <= 0 or W <= 0:
        raise EnslamError(f"accumulate: at least two edges and a sensor with pixels (got {e.size} edges, {H} x {W})")
    if not bool(np.all(e[:-1] <= e[1:])):
        raise EnslamError("accumulate: edges must be ascending and hold no NaN")
    if stream.device.type == 'cuda':
        from . import functional as EF
        out = EF.event_accumulate(*stream.arrays(), e, H, W, want_unsaturated=want_unsaturated)
        counts, dropped, full = out[0], out[1], (out[2] if want_unsaturated else None)
    else:
        counts, full, dropped = accumulate_numpy(*stream.numpy(), e, H, W)
        counts, full = torch.from_numpy(counts), torch.from_numpy(full)
    res = (counts,) + ((full,) if want_unsaturated else ()) + ((dropped,) if with_dropped else ())
    return res[0] if len(res) == 1 else res
