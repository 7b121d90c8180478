"""Dataset readers of the run harness: the reference's `Replica` / `Replica_event` layouts
(src/utils/datasets.py:51-216) read with PIL + numpy instead of cv2 (absent from the image).

    <input_folder>/results/frame*.jpg   colour
    <input_folder>/results/depth*.png   16-bit depth, metres = value / cam.png_depth_scale
    <input_folder>/traj.txt             one row-major 4x4 camera-to-world per line (OpenCV axes; y and z columns flipped
                                        on load, :133-134)
    <event_folder>/*frame*.png          integrated events between frame i-1 and i: RGB png, channels (0, -, +)

Same item tuples, dtypes and conventions as the reference: colour float64 [H,W,3] in [0,1] (`cv2.imread / 255.`),
depth float32 [H,W] * scale, events uint8 [H,W,2] = (-, +) with an all-zero image for frame 0, mask int64 [H,W], pose
float32 [4,4] with the translation scaled IN PLACE on every access (the reference does the same, :112-113).

`RPG` / `RPG_event` (src/utils/datasets.py:218-319; BASELINE config 5's sequence format): grey-scale frames
`results/frame*`, 16-bit depth `results/depth*`, event pngs `<event_folder>/*.png` with channels (+, -, 0), and a lens
model (`cam.distortion` = k1, k2, p1, p2, k3, k4, k5, k6 of OpenCV) that the reference removes from the colour and event images
-- not from the depth -- with `cv2.undistort(img, K, dist)` (:85-88, :262-266).  `undistort()` below restates that call in
numpy: the inverse map of OpenCV's pinhole + rational-radial + tangential model evaluated per destination pixel, bilinear
sampling with a zero border.  cv2 interpolates 8-bit images in fixed point (1/32 pixel, 15-bit weights); this version
interpolates in float64 and rounds once, so single pixels may differ from cv2's by one grey level.  cv2 is absent from the
image, so that last level is "parity unpinned"; the geometry is pinned by a distort -> undistort round trip
(tests/test_harness_cpu.py).

Further layouts of the reference's `dataset_dict` (src/utils/datasets.py:321-606): `RPG_event_dense` (`data.density` event
frames per image interval, poses from traj_density{d}.txt), `TUM_RGBD` (rgb.txt / depth.txt / groundtruth.txt associated by
nearest time stamp), `ScanNet` (frames/{color,depth,pose}, numeric file order) and `Azure` (scene/trajectory.log).  `CoFusion`
is not built: its depth is OpenEXR and no EXR decoder is installed.

`data.event_stream` + `data.frame_stamps` (opt-in, the three `*_event` readers): the event image of a frame is accumulated from a
time-stamped stream (event_stream.accumulate) between the frame times instead of read from `<event_folder>`, and built as the
uint8 array the png would decode to; see `BaseDataset._init_event_stream`.

`data.prepare` (attribute `prepare`): 'host' (default) prepares a frame with numpy / torch on the CPU as described above and
uploads the result; 'device' uploads the RAW decoded arrays and prepares them in one launch of csrc/frame_prep.hip
(functional.frame_prepare) -- the same stages in the same order and precision, an eighth of the upload."""
import glob
import os

import numpy as np
import torch
import torch.nn.functional as F


def _imread_rgb(path):
    from PIL import Image
    with Image.open(path) as im:
        return np.array(im.convert("RGB"))


def _imread_depth(path):
    from PIL import Image
    with Image.open(path) as im:
        return np.array(im)                                     # 16-bit png ('I;16') -> uint16 / int32


def _resize_bilinear(img, size_hw):
    """cv2.resize(img, (W, H)) default INTER_LINEAR (half-pixel centres, no antialiasing) for float or uint8 HxWxC."""
    if img.shape[0] == size_hw[0] and img.shape[1] == size_hw[1]:
        return img
    t = torch.from_numpy(np.ascontiguousarray(img)).double().permute(2, 0, 1)[None]
    out = F.interpolate(t, size=size_hw, mode='bilinear', align_corners=False)[0].permute(1, 2, 0).numpy()
    return out if img.dtype.kind == 'f' else np.clip(np.rint(out), 0, 255).astype(img.dtype)


def get_dataset(cfg, args, scale, device='cuda:0'):
    return dataset_dict[cfg['dataset']](cfg, args, scale, device=device)


class BaseDataset(torch.utils.data.Dataset):
    def __init__(self, cfg, args, scale, device='cuda:0'):
        super().__init__()
        self.name = cfg['dataset']
        self.device = device
        self.scale = scale
        cam = cfg['cam']
        self.png_depth_scale = cam['png_depth_scale']
        self.H, self.W, self.fx, self.fy, self.cx, self.cy = cam['H'], cam['W'], cam['fx'], cam['fy'], cam['cx'], cam['cy']
        self.distortion = np.asarray(cam['distortion'], dtype=np.float64) if cam.get('distortion') is not None else None
        self.crop_size = cam.get('crop_size')
        self.input_folder = cfg['data']['input_folder'] if getattr(args, 'input_folder', None) is None else args.input_folder
        self.crop_edge = cam['crop_edge']
        self.prepare = cfg['data'].get('prepare', 'host')

    def __len__(self):
        return self.n_img

    def _on_device(self):
        """True for prepare == 'device'; that route exists on a HIP device only."""
        if self.prepare not in ('host', 'device'):
            raise ValueError(f"data.prepare must be 'host' or 'device' (got {self.prepare!r})")
        if self.prepare == 'device' and torch.device(self.device).type != 'cuda':
            from ._lib import EnslamError
            raise EnslamError(f"data.prepare = 'device' prepares frames with the HIP kernel and needs a HIP device (the dataset's "
                              f"device is {self.device!r}); use prepare = 'host' there")
        return self.prepare == 'device'

    def _prepare_device(self, color, depth, event=None, events=False, event_order='replica', undistort_events=False):
        from . import functional as EF
        return EF.frame_prepare(color, depth, event, events=events, K=(self.fx, self.fy, self.cx, self.cy),
                                distortion=self.distortion, png_depth_scale=self.png_depth_scale, scale=self.scale,
                                crop_size=self.crop_size, crop_edge=self.crop_edge, event_order=event_order,
                                undistort_events=undistort_events, device=self.device)

    def _init_event_stream(self, cfg, density=1):
        """The opt-in keys `data.event_stream` (a stream: `.npz` of event_stream.EventStream.save, or the text layout `t x y p`)
        and `data.frame_stamps` (a text file whose first field per non-comment line is a frame time).  With both set the
        event image of an item is accumulated from the stream (event_stream.accumulate: the HIP kernel on a HIP device,
        numpy on the CPU) instead of read from a png; it is built as the uint8 [H,W,3] array the png would decode to, at the
        size of the raw colour frame, so everything behind the decode is shared.  Returns False when neither key is set.
        `data.event_filter` (opt-in, honoured only together with these two): a mapping with any of the keys refractory,
        support_dt (seconds), hot_rate (Hz) and hot_max (events); the time-sorted stream is denoised once
        (event_filter.filter_from_options) before it is cut into frames, and the counters are kept in `event_filter_stats`."""
        path, stamps = cfg['data'].get('event_stream'), cfg['data'].get('frame_stamps')
        self._stream = None
        if path is None and stamps is None:
            return False
        if path is None or stamps is None:
            raise ValueError("data.event_stream and data.frame_stamps come together")
        from . import event_stream as ES
        times = ES.read_stamps(stamps)
        assert len(times) >= self.n_img, "Number of frame stamps is below that of GT images!"
        self._edges = ES.frame_edges(times[:self.n_img], 1, density)
        dev = self.device if torch.device(self.device).type == 'cuda' else 'cpu'
        self._stream = ES.load_stream(path, device=dev).time_sorted()
        self.event_filter_stats = None
        opts = cfg['data'].get('event_filter')
        if opts is not None:                                        # opt-in: denoise the stream once, before the cuts are taken
            unknown = set(opts) - {'refractory', 'support_dt', 'hot_rate', 'hot_max'}
            if unknown:
                raise ValueError(f"data.event_filter: unknown keys {sorted(unknown)} (refractory, support_dt, hot_rate, hot_max)")
            from . import event_filter as EFI
            from PIL import Image
            with Image.open(self.color_paths[0]) as im:
                W, H = im.size
            self._stream, self.event_filter_stats = EFI.filter_from_options(self._stream, H, W, **opts)
        # events of bin b are the slice [cuts[b], cuts[b + 1]) of the sorted stream: edges[b] < t <= edges[b + 1]
        self._cuts = torch.searchsorted(self._stream.t, torch.from_numpy(self._edges).to(dev), right=True).tolist()
        self.event_paths = None
        self.n_event = len(self._edges) - 1
        return True

    def event_slice(self, index):
        """(stream, t0, t1): the events of item `index` >= 1 as an event_stream.EventStream on the stream's device (the
        dataset's, when that is a HIP device), and the two frame times that bound them: t0 < t <= t1, the bin rule of
        `_init_event_stream`.  Needs data.event_stream and data.frame_stamps."""
        if getattr(self, '_stream', None) is None:
            raise ValueError("event_slice needs the time-stamped events of data.event_stream and data.frame_stamps")
        if not 1 <= index < len(self._cuts):
            raise IndexError(f"event_slice: item {index} has no event interval (1..{len(self._cuts) - 1})")
        from . import event_stream as ES
        i0, i1 = self._cuts[index - 1], self._cuts[index]
        part = ES.EventStream(*(a[i0:i1] for a in self._stream.arrays()))
        return part, float(self._edges[index - 1]), float(self._edges[index])

    def _event_image(self, index, order):
        """uint8 [H,W,3]: the decoded event png of item `index` >= 1, or the same array accumulated from the stream;
        order 'replica' = channels (0, -, +), 'rpg' = (+, -, 0)."""
        if self._stream is None:
            return _imread_rgb(self.event_paths[index - 1])
        from . import event_stream as ES
        from PIL import Image
        with Image.open(self.color_paths[0]) as im:
            W, H = im.size
        i0, i1 = self._cuts[index - 1], self._cuts[index]
        part = ES.EventStream(*(a[i0:i1] for a in self._stream.arrays()))
        ev = ES.accumulate(part, self._edges[index - 1:index + 1], H, W)[0].cpu().numpy()
        rgb = np.zeros((H, W, 3), dtype=np.uint8)
        if order == 'replica':
            rgb[..., 1:] = ev
        else:
            rgb[..., 0], rgb[..., 1] = ev[..., 1], ev[..., 0]
        return rgb

    def _color_depth(self, index):
        color = _imread_rgb(self.color_paths[index])
        if self.distortion is not None:                             # only the colour image, not the depth (:84-88)
            color = undistort(color, (self.fx, self.fy, self.cx, self.cy), self.distortion)
        color = color / 255.
        depth = _imread_depth(self.depth_paths[index]).astype(np.float32) / self.png_depth_scale
        H, W = depth.shape
        color = torch.from_numpy(_resize_bilinear(color, (H, W)))
        depth = torch.from_numpy(depth) * self.scale
        return color, depth

    def _crop(self, color, depth, event=None):
        if self.crop_size is not None:                              # :95-103 ("actually is resize")
            color = F.interpolate(color.permute(2, 0, 1)[None], self.crop_size, mode='bilinear', align_corners=True)[0]
            depth = F.interpolate(depth[None, None], self.crop_size, mode='nearest')[0, 0]
            color = color.permute(1, 2, 0).contiguous()
            if event is not None:
                event = F.interpolate(event.permute(2, 0, 1)[None].float(), self.crop_size, mode='bilinear', align_corners=True)[0]
                event = event.permute(1, 2, 0).contiguous()
        e = self.crop_edge
        if e > 0:
            color, depth = color[e:-e, e:-e], depth[e:-e, e:-e]
            if event is not None:
                event = event[e:-e, e:-e]
        return color, depth, event

    def _pose(self, index):
        pose = self.poses[index]
        pose[:3, 3] *= self.scale
        return pose

    def __getitem__(self, index):
        if self._on_device():
            color, depth = self._prepare_device(_imread_rgb(self.color_paths[index]), _imread_depth(self.depth_paths[index]))
            return index, color, depth, self._pose(index).to(self.device)
        color, depth = self._color_depth(index)
        color, depth, _ = self._crop(color, depth)
        return index, color.to(self.device), depth.to(self.device), self._pose(index).to(self.device)


class Replica(BaseDataset):
    def __init__(self, cfg, args, scale, device='cuda:0'):
        super().__init__(cfg, args, scale, device)
        self.color_paths = sorted(glob.glob(f'{self.input_folder}/results/frame*.jpg'))
        self.depth_paths = sorted(glob.glob(f'{self.input_folder}/results/depth*.png'))
        self.n_img = len(self.color_paths)
        self.load_poses(f'{self.input_folder}/traj.txt')

    def load_poses(self, path):
        self.poses = []
        with open(path, "r") as f:
            lines = f.readlines()
        for i in range(self.n_img):
            c2w = np.array(list(map(float, lines[i].split()))).reshape(4, 4)
            c2w[:3, 1] *= -1
            c2w[:3, 2] *= -1
            self.poses.append(torch.from_numpy(c2w).float())


class Replica_event(Replica):
    def __init__(self, cfg, args, scale, device='cuda:0'):
        super().__init__(cfg, args, scale, device)
        if not self._init_event_stream(cfg):
            self.event_folder = cfg['data']['event_folder'] if getattr(args, 'event_folder', None) is None else args.event_folder
            self.event_paths = sorted(glob.glob(f'{self.event_folder}/*frame*.png'))
            self.n_event = len(self.event_paths)
        assert self.n_event == self.n_img - 1, "Number of GT events does not match that of GT images!"

    def __getitem__(self, index):
        if self._on_device():                                       # the event image keeps its lens model here (as below)
            event = self._event_image(index, 'replica') if index >= 1 else None
            color, depth, event, mask = self._prepare_device(_imread_rgb(self.color_paths[index]),
                                                             _imread_depth(self.depth_paths[index]), event, events=True)
            return index, color, depth, event, mask, self._pose(index).to(self.device)
        color, depth = self._color_depth(index)
        H, W = depth.shape
        if index >= 1:
            event = self._event_image(index, 'replica')             # png (0, -, +)
        else:
            event = np.zeros((H, W, 3), dtype=np.uint8)             # all black for the first frame
        event = torch.from_numpy(_resize_bilinear(event, (H, W)))
        color, depth, event = self._crop(color, depth, event)
        event = event[:, :, 1:]                                     # (-, +)
        mask = torch.any(event != 0, dim=-1) * 1
        return (index, color.to(self.device), depth.to(self.device), event.to(self.device), mask.to(self.device),
                self._pose(index).to(self.device))


def distort_points(x, y, dist):
    """OpenCV's lens model on normalised image coordinates: (x, y) -> (x_d, y_d) with dist = (k1, k2, p1, p2[, k3[, k4, k5, k6]])."""
    d = np.zeros(8, dtype=np.float64)
    d[:min(len(dist), 8)] = np.asarray(dist, dtype=np.float64)[:8]
    k1, k2, p1, p2, k3, k4, k5, k6 = d
    r2 = x * x + y * y
    radial = (1 + r2 * (k1 + r2 * (k2 + r2 * k3))) / (1 + r2 * (k4 + r2 * (k5 + r2 * k6)))
    xd = x * radial + 2 * p1 * x * y + p2 * (r2 + 2 * x * x)
    yd = y * radial + p1 * (r2 + 2 * y * y) + 2 * p2 * x * y
    return xd, yd


def undistort(img, K, dist):
    """`cv2.undistort(img, K, dist)` (new camera matrix = K) for an HxW or HxWxC array: every destination pixel (u, v) reads
    the source at the DISTORTED position of its ray -- u' = fx x_d + cx, v' = fy y_d + cy with (x_d, y_d) =
    distort_points((u - cx) / fx, (v - cy) / fy) -- by bilinear interpolation, zeros outside the image.  uint8 in -> uint8 out
    (rounded once), float in -> float64 out."""
    fx, fy, cx, cy = K
    a = np.asarray(img)
    H, W = a.shape[:2]
    u, v = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    xd, yd = distort_points((u - cx) / fx, (v - cy) / fy, dist)
    mx, my = fx * xd + cx, fy * yd + cy
    x0, y0 = np.floor(mx).astype(np.int64), np.floor(my).astype(np.int64)
    ax, ay = mx - x0, my - y0
    src = a.reshape(H, W, -1).astype(np.float64)

    def tap(yy, xx):
        ok = (yy >= 0) & (yy < H) & (xx >= 0) & (xx < W)
        return src[np.clip(yy, 0, H - 1), np.clip(xx, 0, W - 1)] * ok[..., None]

    out = ((1 - ay) * (1 - ax))[..., None] * tap(y0, x0) + ((1 - ay) * ax)[..., None] * tap(y0, x0 + 1) + \
          (ay * (1 - ax))[..., None] * tap(y0 + 1, x0) + (ay * ax)[..., None] * tap(y0 + 1, x0 + 1)
    out = out.reshape(a.shape)
    return np.clip(np.rint(out), 0, 255).astype(np.uint8) if a.dtype == np.uint8 else out


class RPG(BaseDataset):
    """src/utils/datasets.py:218-240: the Replica layout with any image extension."""

    def __init__(self, cfg, args, scale, device='cuda:0'):
        super().__init__(cfg, args, scale, device)
        self.color_paths = sorted(glob.glob(f'{self.input_folder}/results/frame*'))
        self.depth_paths = sorted(glob.glob(f'{self.input_folder}/results/depth*'))
        self.n_img = len(self.color_paths)
        Replica.load_poses(self, f'{self.input_folder}/traj.txt')


class RPG_event(RPG):
    """src/utils/datasets.py:242-319: grey-scale frames (read as grey, replicated to three channels), event pngs with channels
    (+, -, 0) handed out as (-, +) like Replica_event, the lens model removed from colour and events."""

    def __init__(self, cfg, args, scale, device='cuda:0'):
        super().__init__(cfg, args, scale, device)
        if not self._init_event_stream(cfg):
            self.event_folder = cfg['data']['event_folder'] if getattr(args, 'event_folder', None) is None else args.event_folder
            self.event_paths = sorted(glob.glob(f'{self.event_folder}/*.png'))
            self.n_event = len(self.event_paths)
        assert self.n_event == self.n_img - 1, "Number of GT events does not match that of GT images!"

    def __getitem__(self, index):
        return self._frame(index, index)

    def _frame(self, index, image):
        """Item `index`: events of interval index - 1, colour and depth of image number `image`."""
        from PIL import Image
        with Image.open(self.color_paths[image]) as im:
            grey = np.array(im.convert('L'))                        # cv2.IMREAD_GRAYSCALE, then GRAY2BGR (:252-253)
        if self._on_device():
            event = self._event_image(index, 'rpg') if index >= 1 else None
            color, depth, event, mask = self._prepare_device(grey, _imread_depth(self.depth_paths[image]), event, events=True,
                                                             event_order='rpg', undistort_events=True)
            return index, color, depth, event, mask, self._pose(index).to(self.device)
        color = np.repeat(grey[:, :, None], 3, axis=2)
        depth = _imread_depth(self.depth_paths[image]).astype(np.float32) / self.png_depth_scale
        event = self._event_image(index, 'rpg') if index >= 1 else np.zeros_like(color)            # RGB = (+, -, 0)
        if self.distortion is not None:                             # colour and events, not the depth (:262-266)
            K = (self.fx, self.fy, self.cx, self.cy)
            color, event = undistort(color, K, self.distortion), undistort(event, K, self.distortion)
        H, W = depth.shape
        color = torch.from_numpy(_resize_bilinear(color / 255., (H, W)))
        depth = torch.from_numpy(depth) * self.scale
        event = torch.from_numpy(_resize_bilinear(event, (H, W)))
        color, depth, event = self._crop(color, depth, event)
        event = event[:, :, :-1]                                    # (+, -)
        event = event[:, :, [1, 0]]                                 # (-, +) as in Replica_event (:309-310)
        mask = torch.any(event != 0, dim=-1) * 1
        return (index, color.to(self.device), depth.to(self.device), event.to(self.device), mask.to(self.device),
                self._pose(index).to(self.device))


class RPG_event_dense(RPG):
    """src/utils/datasets.py:321-423: `RPG_event` with `data.density` event frames per image interval.  Item i carries the
    events of interval i - 1 and the pose of line i of traj_density{density}.txt; its colour and depth are those of image
    i // density (meant to be used where i % density == 0, a placeholder in between)."""

    def __init__(self, cfg, args, scale, device='cuda:0'):
        super().__init__(cfg, args, scale, device)
        self.density = int(cfg['data']['density'])
        if not self._init_event_stream(cfg, self.density):
            self.event_folder = cfg['data']['event_folder'] if getattr(args, 'event_folder', None) is None else args.event_folder
            self.event_paths = sorted(glob.glob(f'{self.event_folder}/*.png'))
            self.n_event = len(self.event_paths)
        assert self.n_event == (self.n_img - 1) * self.density, "Number of GT events does not match that of GT images!"
        with open(f'{self.input_folder}/traj_density{self.density}.txt', "r") as f:
            lines = f.readlines()
        assert len(lines) == self.n_event + 1, "Number of GT events does not match that of GT poses!"
        self.poses = []                                             # one per event frame, in place of traj.txt's
        for line in lines:
            c2w = np.array(line.split(), dtype=np.float64).reshape(4, 4)
            c2w[:3, 1] *= -1
            c2w[:3, 2] *= -1
            self.poses.append(torch.from_numpy(c2w).float())

    _frame = RPG_event._frame

    def __len__(self):
        return self.n_event + 1

    def __getitem__(self, index):
        return self._frame(index, index // self.density)


class Azure(BaseDataset):
    """src/utils/datasets.py:425-463: color/*.jpg, depth/*.png and scene/trajectory.log -- records of five lines, a header
    (source, target, fitness) and the four rows of a camera-to-world matrix; identity poses when the file is absent."""

    def __init__(self, cfg, args, scale, device='cuda:0'):
        super().__init__(cfg, args, scale, device)
        self.color_paths = sorted(glob.glob(os.path.join(self.input_folder, 'color', '*.jpg')))
        self.depth_paths = sorted(glob.glob(os.path.join(self.input_folder, 'depth', '*.png')))
        self.n_img = len(self.color_paths)
        self.load_poses(os.path.join(self.input_folder, 'scene', 'trajectory.log'))

    def load_poses(self, path):
        self.poses = []
        if not os.path.exists(path):
            self.poses = [torch.eye(4) for _ in range(self.n_img)]
            return
        with open(path) as f:
            lines = f.readlines()
        for i in range(0, len(lines) - 4, 5):
            c2w = np.array(' '.join(lines[i + 1:i + 5]).split(), dtype=np.float64).reshape(4, 4)
            c2w[:3, 1] *= -1
            c2w[:3, 2] *= -1
            self.poses.append(torch.from_numpy(c2w).float())


def _numbered(pattern):
    """files matching `pattern` in the order of the integer their name starts with (2.jpg before 10.jpg)"""
    return sorted(glob.glob(pattern), key=lambda x: int(os.path.splitext(os.path.basename(x))[0]))


class ScanNet(BaseDataset):
    """src/utils/datasets.py:466-493: frames/color/<n>.jpg, frames/depth/<n>.png, frames/pose/<n>.txt (a 4x4 per file)."""

    def __init__(self, cfg, args, scale, device='cuda:0'):
        super().__init__(cfg, args, scale, device)
        self.input_folder = os.path.join(self.input_folder, 'frames')
        self.color_paths = _numbered(os.path.join(self.input_folder, 'color', '*.jpg'))
        self.depth_paths = _numbered(os.path.join(self.input_folder, 'depth', '*.png'))
        self.n_img = len(self.color_paths)
        self.poses = []
        for path in _numbered(os.path.join(self.input_folder, 'pose', '*.txt')):
            with open(path, "r") as f:
                c2w = np.array(f.read().split(), dtype=np.float64).reshape(4, 4)
            c2w[:3, 1] *= -1
            c2w[:3, 2] *= -1
            self.poses.append(torch.from_numpy(c2w).float())


def quaternion_matrix(q):
    """3x3 rotation of the quaternion (x, y, z, w), normalised first (scipy's Rotation.from_quat(q).as_matrix())."""
    x, y, z, w = np.asarray(q, dtype=np.float64) / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def matrix_quaternion(R):
    """(x, y, z, w), w >= 0, of a 3x3 rotation: the inverse of `quaternion_matrix` (the sequence writers)."""
    R = np.asarray(R, dtype=np.float64)
    d = np.array([R[0, 0] - R[1, 1] - R[2, 2], R[1, 1] - R[0, 0] - R[2, 2], R[2, 2] - R[0, 0] - R[1, 1],
                  R[0, 0] + R[1, 1] + R[2, 2]])                     # 4 q_i^2 - 1
    k = int(np.argmax(d))                                           # the largest component: safe to divide by
    q = np.zeros(4)
    q[k] = np.sqrt(1 + d[k]) / 2
    prod = {(0, 1): R[0, 1] + R[1, 0], (0, 2): R[0, 2] + R[2, 0], (1, 2): R[1, 2] + R[2, 1],
            (0, 3): R[2, 1] - R[1, 2], (1, 3): R[0, 2] - R[2, 0], (2, 3): R[1, 0] - R[0, 1]}      # 4 q_i q_j
    for i in range(4):
        if i != k:
            q[i] = prod[(min(i, k), max(i, k))] / (4 * q[k])
    return q if q[3] >= 0 else -q


class TUM_RGBD(BaseDataset):
    """src/utils/datasets.py:519-606: rgb.txt and depth.txt (time stamp, file), groundtruth.txt or pose.txt (time stamp, t,
    q_xyzw; its first line is skipped as in the reference).  Every colour stamp takes the depth and the pose nearest in time
    and is dropped unless both lie within max_dt = 0.08 s; the survivors are thinned so that consecutive frames are more than
    1 / frame_rate = 1 / 32 s apart; poses are relative to the first kept frame."""

    def __init__(self, cfg, args, scale, device='cuda:0'):
        super().__init__(cfg, args, scale, device)
        self.color_paths, self.depth_paths, self.poses = self.loadtum(self.input_folder, frame_rate=32)
        self.n_img = len(self.color_paths)

    @staticmethod
    def parse_list(path, skiprows=0):
        """rows of a space-separated list as strings; '#' starts a comment (np.loadtxt(dtype=str) of the reference)"""
        with open(path) as f:
            lines = f.readlines()[skiprows:]
        rows = [ln.split('#', 1)[0].split() for ln in lines]
        return np.array([r for r in rows if r], dtype=str)

    @staticmethod
    def associate_frames(t_image, t_depth, t_pose, max_dt=0.08):
        out = []
        for i, t in enumerate(t_image):
            j, k = int(np.argmin(np.abs(t_depth - t))), int(np.argmin(np.abs(t_pose - t)))
            if np.abs(t_depth[j] - t) < max_dt and np.abs(t_pose[k] - t) < max_dt:
                out.append((i, j, k))
        return out

    def loadtum(self, root, frame_rate=-1):
        pose_list = os.path.join(root, 'groundtruth.txt')
        if not os.path.isfile(pose_list):
            pose_list = os.path.join(root, 'pose.txt')
        images, depths = self.parse_list(os.path.join(root, 'rgb.txt')), self.parse_list(os.path.join(root, 'depth.txt'))
        pose_rows = self.parse_list(pose_list, skiprows=1)
        t_image, t_depth = images[:, 0].astype(np.float64), depths[:, 0].astype(np.float64)
        t_pose, vecs = pose_rows[:, 0].astype(np.float64), pose_rows[:, 1:].astype(np.float64)
        assoc = self.associate_frames(t_image, t_depth, t_pose)
        keep = [0]
        for a in range(1, len(assoc)):
            if t_image[assoc[a][0]] - t_image[assoc[keep[-1]][0]] > 1.0 / frame_rate:
                keep.append(a)
        color_paths, depth_paths, poses, first_inv = [], [], [], None
        for a in keep:
            i, j, k = assoc[a]
            color_paths.append(os.path.join(root, images[i, 1]))
            depth_paths.append(os.path.join(root, depths[j, 1]))
            c2w = np.eye(4)
            c2w[:3, :3], c2w[:3, 3] = quaternion_matrix(vecs[k, 3:]), vecs[k, :3]
            if first_inv is None:
                first_inv, c2w = np.linalg.inv(c2w), np.eye(4)
            else:
                c2w = first_inv @ c2w
            c2w[:3, 1] *= -1
            c2w[:3, 2] *= -1
            poses.append(torch.from_numpy(c2w).float())
        return color_paths, depth_paths, poses


dataset_dict = {"replica": Replica, "replica_event": Replica_event, "rpg": RPG, "rpg_event": RPG_event,
                "rpg_event_dense": RPG_event_dense, "tumrgbd": TUM_RGBD, "scannet": ScanNet, "azure": Azure}


def write_rpg_event_sequence(root, frames, poses, png_depth_scale, events):
    """Write a sequence in the RPG_event layout (tests): frames = list of (grey uint8 [H,W], depth float32 [H,W] metres),
    events = list (n-1) of uint8 [H,W,2] (-, +); written as png (+, -, 0).  Returns (input_folder, event_folder)."""
    from PIL import Image
    inp, evf = os.path.join(root, 'seq'), os.path.join(root, 'seq_events')
    os.makedirs(os.path.join(inp, 'results'), exist_ok=True)
    os.makedirs(evf, exist_ok=True)
    with open(os.path.join(inp, 'traj.txt'), 'w') as f:
        for i, ((grey, depth), pose) in enumerate(zip(frames, poses)):
            Image.fromarray(np.asarray(grey, dtype=np.uint8), 'L').save(os.path.join(inp, 'results', f'frame{i:06d}.png'))
            d16 = np.clip(np.rint(np.asarray(depth, dtype=np.float64) * png_depth_scale), 0, 65535).astype(np.uint16)
            Image.fromarray(d16).save(os.path.join(inp, 'results', f'depth{i:06d}.png'))
            p = np.array(pose, dtype=np.float64).reshape(4, 4).copy()
            p[:3, 1] *= -1
            p[:3, 2] *= -1
            f.write(' '.join(repr(float(v)) for v in p.reshape(-1)) + '\n')
    for i, ev in enumerate(events):
        save_event_image(evf, i + 1, ev, 'rpg_event')
    return inp, evf


def write_replica_event_sequence(root, frames, poses, png_depth_scale, events=None):
    """Write a sequence in the layout above (synthetic data for tests and the harness's smoke run).
    frames: list of (color float [H,W,3] in [0,1], depth float32 [H,W] metres); poses: list of [4,4] camera-to-world IN THE
    READER'S convention (the y / z column flip of load_poses is undone here); events: list (n-1) of uint8 [H,W,2] (-, +).
    Colour is written as PNG-quality JPEG (quality 100, no chroma subsampling).  Returns (input_folder, event_folder)."""
    from PIL import Image
    inp, evf = os.path.join(root, 'seq'), os.path.join(root, 'seq_events')
    os.makedirs(os.path.join(inp, 'results'), exist_ok=True)
    os.makedirs(evf, exist_ok=True)
    with open(os.path.join(inp, 'traj.txt'), 'w') as f:
        for i, ((color, depth), pose) in enumerate(zip(frames, poses)):
            c8 = np.clip(np.rint(np.asarray(color, dtype=np.float64) * 255.), 0, 255).astype(np.uint8)
            Image.fromarray(c8, 'RGB').save(os.path.join(inp, 'results', f'frame{i:06d}.jpg'), quality=100, subsampling=0)
            d16 = np.clip(np.rint(np.asarray(depth, dtype=np.float64) * png_depth_scale), 0, 65535).astype(np.uint16)
            Image.fromarray(d16).save(os.path.join(inp, 'results', f'depth{i:06d}.png'))
            p = np.array(pose, dtype=np.float64).reshape(4, 4).copy()
            p[:3, 1] *= -1
            p[:3, 2] *= -1
            f.write(' '.join(repr(float(v)) for v in p.reshape(-1)) + '\n')
    if events is not None:
        for i, ev in enumerate(events):
            save_event_image(evf, i + 1, ev, 'replica_event')
    return inp, evf


def save_event_image(folder, number, ev, layout='replica_event'):
    """One event image uint8 [H,W,2] = (-, +) as the png the `layout` reader expects, named and ordered as the sequence
    writers above do: 'replica_event' event_frame{number:06d}.png with channels (0, -, +), 'rpg_event' event{number:06d}.png
    with (+, -, 0).  `number` is the frame the interval ends at (1 for the first image).  Returns the path."""
    from PIL import Image
    ev = np.asarray(ev, dtype=np.uint8)
    rgb = np.zeros(ev.shape[:2] + (3,), dtype=np.uint8)
    if layout == 'replica_event':
        rgb[..., 1:] = ev
        path = os.path.join(folder, f'event_frame{number:06d}.png')
    elif layout == 'rpg_event':
        rgb[..., 0], rgb[..., 1] = ev[..., 1], ev[..., 0]
        path = os.path.join(folder, f'event{number:06d}.png')
    else:
        raise ValueError(f"save_event_image: layout must be 'replica_event' or 'rpg_event' (got {layout!r})")
    Image.fromarray(rgb, 'RGB').save(path)
    return path


def _color_u8(color):
    a = np.asarray(color)
    return a if a.dtype == np.uint8 else np.clip(np.rint(a.astype(np.float64) * 255.), 0, 255).astype(np.uint8)


def _depth_u16(depth, png_depth_scale):
    return np.clip(np.rint(np.asarray(depth, dtype=np.float64) * png_depth_scale), 0, 65535).astype(np.uint16)


def _opencv_pose(pose):
    """a camera-to-world in the readers' convention -> the file's (the y / z column flip undone)"""
    p = np.array(pose, dtype=np.float64).reshape(4, 4).copy()
    p[:3, 1] *= -1
    p[:3, 2] *= -1
    return p


def _save_color(c8, path):
    from PIL import Image
    im = Image.fromarray(c8, 'RGB') if c8.ndim == 3 else Image.fromarray(c8, 'L')
    if path.endswith('.jpg'):
        im.save(path, quality=100, subsampling=0)
    else:
        im.save(path)


def write_rpg_event_dense_sequence(root, frames, poses, png_depth_scale, events, density):
    """The RPG_event_dense layout: `write_rpg_event_sequence` with len(events) = (len(frames) - 1) * density event pngs and
    len(events) + 1 poses (one per event frame, the readers' convention) in traj_density{density}.txt.  traj.txt holds the
    poses of the images (every density-th).  Returns (input_folder, event_folder)."""
    assert len(events) == (len(frames) - 1) * density and len(poses) == len(events) + 1
    inp, evf = write_rpg_event_sequence(root, frames, poses[::density], png_depth_scale, events)
    with open(os.path.join(inp, f'traj_density{density}.txt'), 'w') as f:
        for pose in poses:
            f.write(' '.join(repr(float(v)) for v in _opencv_pose(pose).reshape(-1)) + '\n')
    return inp, evf


def write_tum_sequence(root, frames, poses, png_depth_scale, stamps=None, depth_stamps=None, pose_stamps=None,
                       pose_file='groundtruth.txt'):
    """The TUM RGB-D layout: rgb/<stamp>.png, depth/<stamp>.png, rgb.txt, depth.txt and `pose_file` (stamp tx ty tz qx qy qz
    qw), each list under the three comment lines of the original files.  frames: list of (colour, depth metres); poses:
    camera-to-world in the readers' convention, one per entry of pose_stamps (default: one per frame at the colour stamps;
    TUM_RGBD hands them out relative to the first kept frame).  stamps / depth_stamps: seconds, default 0.1 s apart /
    the colour stamps; an entry of None in depth_stamps leaves that depth image out.  Returns the input folder."""
    from PIL import Image
    inp = os.path.join(root, 'seq')
    os.makedirs(os.path.join(inp, 'rgb'), exist_ok=True)
    os.makedirs(os.path.join(inp, 'depth'), exist_ok=True)
    stamps = [1.0 + 0.1 * i for i in range(len(frames))] if stamps is None else list(stamps)
    depth_stamps = stamps if depth_stamps is None else list(depth_stamps)
    pose_stamps = stamps if pose_stamps is None else list(pose_stamps)
    head = '# {}\n# file: synthetic\n# {}\n'
    with open(os.path.join(inp, 'rgb.txt'), 'w') as fc, open(os.path.join(inp, 'depth.txt'), 'w') as fd:
        fc.write(head.format('color images', 'timestamp filename'))
        fd.write(head.format('depth maps', 'timestamp filename'))
        for (color, depth), tc, td in zip(frames, stamps, depth_stamps):
            _save_color(_color_u8(color), os.path.join(inp, 'rgb', f'{tc:.6f}.png'))
            fc.write(f'{tc:.6f} rgb/{tc:.6f}.png\n')
            if td is not None:
                Image.fromarray(_depth_u16(depth, png_depth_scale)).save(os.path.join(inp, 'depth', f'{td:.6f}.png'))
                fd.write(f'{td:.6f} depth/{td:.6f}.png\n')
    with open(os.path.join(inp, pose_file), 'w') as f:
        f.write(head.format('ground truth trajectory', 'timestamp tx ty tz qx qy qz qw'))
        for pose, t in zip(poses, pose_stamps):
            p = _opencv_pose(pose)
            f.write(f'{t:.6f} ' + ' '.join(repr(float(v)) for v in list(p[:3, 3]) + list(matrix_quaternion(p[:3, :3]))) + '\n')
    return inp


def write_scannet_sequence(root, frames, poses, png_depth_scale, numbers=None):
    """The ScanNet layout: frames/color/<n>.jpg, frames/depth/<n>.png, frames/pose/<n>.txt with n = numbers[i] (default i, no
    zero padding: the reader orders by the integer).  The colour may be larger than the depth.  Returns the input folder."""
    from PIL import Image
    inp = os.path.join(root, 'seq')
    for sub in ('color', 'depth', 'pose'):
        os.makedirs(os.path.join(inp, 'frames', sub), exist_ok=True)
    numbers = list(range(len(frames))) if numbers is None else list(numbers)
    for n, (color, depth), pose in zip(numbers, frames, poses):
        _save_color(_color_u8(color), os.path.join(inp, 'frames', 'color', f'{n}.jpg'))
        Image.fromarray(_depth_u16(depth, png_depth_scale)).save(os.path.join(inp, 'frames', 'depth', f'{n}.png'))
        with open(os.path.join(inp, 'frames', 'pose', f'{n}.txt'), 'w') as f:
            for row in _opencv_pose(pose):
                f.write(' '.join(repr(float(v)) for v in row) + '\n')
    return inp


def write_azure_sequence(root, frames, poses, png_depth_scale):
    """The Azure layout: color/<i>.jpg, depth/<i>.png and, unless poses is None, scene/trajectory.log in five-line records.
    Returns the input folder."""
    from PIL import Image
    inp = os.path.join(root, 'seq')
    for sub in ('color', 'depth'):
        os.makedirs(os.path.join(inp, sub), exist_ok=True)
    for i, (color, depth) in enumerate(frames):
        _save_color(_color_u8(color), os.path.join(inp, 'color', f'{i:06d}.jpg'))
        Image.fromarray(_depth_u16(depth, png_depth_scale)).save(os.path.join(inp, 'depth', f'{i:06d}.png'))
    if poses is not None:
        os.makedirs(os.path.join(inp, 'scene'), exist_ok=True)
        with open(os.path.join(inp, 'scene', 'trajectory.log'), 'w') as f:
            for i, pose in enumerate(poses):
                f.write(f'{i} {i} {i + 1}\n')
                for row in _opencv_pose(pose):
                    f.write(' '.join(repr(float(v)) for v in row) + '\n')
    return inp
