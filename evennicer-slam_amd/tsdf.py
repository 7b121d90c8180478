"""Block-sparse TSDF fusion of depth frames under given poses on the HIP device (csrc/tsdf.hip): what the reference does with
Open3D's ScalableTSDFVolume in Mesher.get_bound_from_frames (src/utils/Mesher.py:214-279), and the classical fused-depth
mesh of a sequence (tools/tsdf_fuse.py).

Blocks ("units", Open3D's term) of 16^3 voxels are anchored at the world origin and found through a dense int32 table over an
integer unit box; the kernels touch, integrate and extract (enslam_hip.h has the arithmetic), this module holds the arrays
and does the allocation: `nonzero` of the newly stamped absent units, then growth of the arrays.  As in Open3D, a frame
integrates only into the blocks it touches itself; blocks opened by earlier frames are left alone.

Differences from Open3D's volume: the voxel geometry is evaluated per voxel in float64 (Open3D
steps the camera point incrementally in float32); the mesh comes out in a fixed order, bit-identical across runs and
independent of the order in which frames opened the blocks; the volume is bounded by its table, sized from the frames
(`for_frames`) -- a depth pixel whose units fall outside is ignored and counted."""
import numpy as np
import torch

from . import functional as EF

BLOCK = 16
MAX_TABLE = 1 << 27
MAX_UNIT = 1 << 26


def _pose44(c2w):
    m = np.eye(4)
    c = c2w.detach().cpu().numpy() if torch.is_tensor(c2w) else np.asarray(c2w)
    m[:c.shape[0]] = c.astype(np.float64)
    return m


def ray_length_table(cam):
    """float64 numpy [H,W]: sqrt(1 + ((u - cx) / fx)^2 + ((v - cy) / fy)^2), the factor between a pixel's depth and the distance
    along its ray."""
    a = (np.arange(int(cam['W']), dtype=np.float64) - float(cam['cx'])) / float(cam['fx'])
    b = (np.arange(int(cam['H']), dtype=np.float64) - float(cam['cy'])) / float(cam['fy'])
    return np.sqrt((1.0 + (a * a)[None, :]) + (b * b)[:, None])


class TSDFVolume:
    """TSDFVolume(voxel_length, sdf_trunc, lo, hi, cam, color=True, depth_sampling_stride=4, device='cuda:0')

    lo, hi   world corners of the volume, snapped outward to whole units of 16 * voxel_length
    cam      mapping with H, W, fx, fy, cx, cy (one camera per volume)
    """

    def __init__(self, voxel_length, sdf_trunc, lo, hi, cam, color=True, depth_sampling_stride=4, device='cuda:0'):
        self.voxel_length, self.sdf_trunc = float(voxel_length), float(sdf_trunc)
        self.unit_length = BLOCK * self.voxel_length
        if not (self.voxel_length > 0 and self.sdf_trunc > 0):
            raise ValueError(f"voxel_length and sdf_trunc must be positive (got {voxel_length}, {sdf_trunc})")
        if self.sdf_trunc > self.unit_length:
            raise ValueError(f"sdf_trunc {self.sdf_trunc} exceeds one unit of 16 voxels ({self.unit_length}): a depth pixel would "
                             "touch more than three units per axis")
        if int(depth_sampling_stride) < 1:
            raise ValueError(f"depth_sampling_stride must be at least 1 (got {depth_sampling_stride})")
        lo, hi = np.asarray(lo, np.float64).reshape(3), np.asarray(hi, np.float64).reshape(3)
        if not (np.isfinite(lo).all() and np.isfinite(hi).all() and (hi >= lo).all()):
            raise ValueError(f"the box [{lo.tolist()}, {hi.tolist()}] is not a finite box with hi >= lo")
        ulo, uhi = np.floor(lo / self.unit_length), np.floor(hi / self.unit_length)
        nu = uhi - ulo + 1
        if float(np.prod(nu)) > MAX_TABLE or np.abs(ulo).max() > MAX_UNIT or np.abs(uhi).max() >= MAX_UNIT:
            raise ValueError(f"the box [{lo.tolist()}, {hi.tolist()}] needs a block table of {[int(n) for n in nu]} units of "
                             f"{self.unit_length} m (more than 2^27 entries, or beyond unit index 2^26): a stray far depth pixel?")
        if torch.device(device).type != 'cuda':
            raise NotImplementedError("TSDFVolume needs a HIP device (csrc/tsdf.hip)")
        self.device = torch.device(device)
        self.cam = {k: cam[k] for k in ('H', 'W', 'fx', 'fy', 'cx', 'cy')}
        self.stride = int(depth_sampling_stride)
        self.unit_lo = [int(x) for x in ulo]
        self.nu = [int(x) for x in nu]
        n = self.nu[0] * self.nu[1] * self.nu[2]
        self.table = torch.full((n,), -1, dtype=torch.int32, device=self.device)
        self.stamps = torch.zeros(n, dtype=torch.int32, device=self.device)
        self.frames = 0
        self.n_blocks = 0
        self.has_color = bool(color)
        self._tsdf = torch.zeros((0, BLOCK ** 3), dtype=torch.float32, device=self.device)
        self._weight = torch.zeros((0, BLOCK ** 3), dtype=torch.float32, device=self.device)
        self._color = torch.zeros((0, BLOCK ** 3, 3), dtype=torch.float32, device=self.device) if color else None
        self.mult = torch.from_numpy(ray_length_table(self.cam)).to(self.device)
        self._stats = []            # per frame: (blocks, touched, device tensor of outside partials, device tensor of voxel counts)
        self.profile = None         # a list: integrate() appends four device events per frame (start, touch, allocation, kernel)

    # ------------------------------------------------------------------ views
    @property
    def tsdf(self):
        """float32 [blocks,16,16,16] (a view; z fastest inside a block)."""
        return self._tsdf[:self.n_blocks].view(-1, BLOCK, BLOCK, BLOCK)

    @property
    def weight(self):
        return self._weight[:self.n_blocks].view(-1, BLOCK, BLOCK, BLOCK)

    @property
    def color(self):
        return self._color[:self.n_blocks].view(-1, BLOCK, BLOCK, BLOCK, 3) if self.has_color else None

    @property
    def stats(self):
        """dict(blocks, bytes, frames=[dict(blocks, touched, touched_outside, integrated_voxels)]); reading it synchronises."""
        frames = [dict(blocks=b, touched=t, touched_outside=int(o.sum()), integrated_voxels=int(c.sum()) if c is not None else 0)
                  for b, t, o, c in self._stats]
        per_block = BLOCK ** 3 * 4 * (2 + (3 if self.has_color else 0))
        return dict(blocks=self.n_blocks, bytes=self.n_blocks * per_block + 8 * self.table.numel(), frames=frames)

    def block_units(self):
        """int64 device tensor [blocks,3]: the world unit index of every block, by block id."""
        idx = torch.nonzero(self.table >= 0).reshape(-1)
        ids = self.table[idx].long()
        u = torch.stack([idx // (self.nu[1] * self.nu[2]), (idx // self.nu[2]) % self.nu[1], idx % self.nu[2]], 1)
        out = torch.empty_like(u)
        out[ids] = u + torch.tensor(self.unit_lo, device=self.device)
        return out

    # ------------------------------------------------------------------ integration
    def _grow(self, need):
        cap = self._tsdf.shape[0]
        if need <= cap:
            return
        new = max(need, 2 * cap, 64)

        def grown(a):
            b = torch.zeros((new,) + tuple(a.shape[1:]), dtype=a.dtype, device=a.device)
            b[:self.n_blocks] = a[:self.n_blocks]
            return b
        self._tsdf, self._weight = grown(self._tsdf), grown(self._weight)
        if self.has_color:
            self._color = grown(self._color)

    def integrate(self, depth, color, c2w):
        """Fuse one frame: depth float32 [H,W] (0 = no measurement), color [H,W,3] in [0,1] or None, c2w [3|4,4] camera-to-world
        in the reference's axes (x right, y up, looking along -z: the est_c2w of a keyframe)."""
        H, W = int(self.cam['H']), int(self.cam['W'])
        depth = torch.as_tensor(depth).to(self.device).detach()
        if tuple(depth.shape) != (H, W):
            raise ValueError(f"depth must be [{H},{W}] (got {tuple(depth.shape)})")
        depth = depth.float().contiguous()
        if self.has_color:
            if color is None:
                raise ValueError("this volume fuses colour: integrate() needs a colour image (or build it with color=False)")
            color = torch.as_tensor(color).to(self.device).detach()
            if tuple(color.shape) != (H, W, 3):
                raise ValueError(f"color must be [{H},{W},3] (got {tuple(color.shape)})")
            color = color.float().contiguous()
        else:
            color = None
        c2w = _pose44(c2w)
        w2c = np.linalg.inv(c2w)
        self.frames += 1
        marks = []

        def mark():
            if self.profile is not None:
                marks.append(torch.cuda.Event(enable_timing=True))
                marks[-1].record()
        mark()
        outside = EF.tsdf_touch(depth, c2w, self.cam, self.stride, self.sdf_trunc, self.voxel_length, self.unit_lo, self.nu,
                                self.frames, self.stamps)
        mark()
        idx = torch.nonzero(self.stamps == self.frames).reshape(-1)         # ascending table index
        new = idx[self.table[idx] < 0]
        if new.numel():
            self._grow(self.n_blocks + int(new.numel()))
            self.table[new] = torch.arange(self.n_blocks, self.n_blocks + int(new.numel()), dtype=torch.int32, device=self.device)
            self.n_blocks += int(new.numel())
        counts = None
        touched_block, touched_index = self.table[idx].contiguous(), idx.int()
        mark()
        if idx.numel():
            counts = EF.tsdf_integrate(depth, color, self.mult, w2c, self.cam, self.voxel_length, self.sdf_trunc, self.unit_lo,
                                       self.nu, touched_block, touched_index, self.n_blocks, self._tsdf, self._weight, self._color)
        mark()
        if self.profile is not None:
            self.profile.append(marks)
        self._stats.append((self.n_blocks, int(idx.numel()), outside, counts))

    def extract_mesh(self):
        """(vertices float64 [V,3], faces int32 [F,3], colors uint8 [V,3] or None) on the device: marching cubes on the zero
        level, normals towards free space; empty tensors when there is no surface."""
        idx = torch.nonzero(self.table >= 0).reshape(-1)                    # ascending table index
        return EF.tsdf_mesh(self.table, self.unit_lo, self.nu, self.n_blocks, self.table[idx].contiguous(), idx.int(), self._tsdf,
                            self._weight, self._color, self.voxel_length)

    # ------------------------------------------------------------------ from frames
    @staticmethod
    def frames_box(frames, cam, device):
        """(lo, hi) float64 numpy [3]: extent of the frames' back-projected valid depth pixels (min / max on the device)."""
        H, W = int(cam['H']), int(cam['W'])
        j, i = torch.meshgrid(torch.arange(H, dtype=torch.float64, device=device), torch.arange(W, dtype=torch.float64, device=device),
                              indexing='ij')
        dirs = torch.stack([(i - cam['cx']) / cam['fx'], -(j - cam['cy']) / cam['fy'], -torch.ones_like(i)], -1)
        lo = torch.full((3,), float('inf'), dtype=torch.float64, device=device)
        hi = -lo
        for f in frames:
            d = torch.as_tensor(f['depth']).to(device).double().reshape(H, W)
            c2w = torch.from_numpy(_pose44(f['est_c2w'] if 'est_c2w' in f else f['c2w'])).to(device)
            ok = d > 0
            if not bool(ok.any()):
                continue
            p = (dirs[ok] * d[ok][:, None]) @ c2w[:3, :3].T + c2w[:3, 3]
            lo, hi = torch.minimum(lo, p.min(0).values), torch.maximum(hi, p.max(0).values)
        return lo.cpu().numpy(), hi.cpu().numpy()

    @classmethod
    def for_frames(cls, frames, cam, voxel_length, sdf_trunc, color=True, depth_sampling_stride=4, device='cuda:0'):
        """A volume sized from the frames' back-projected valid depth pixels +- sdf_trunc, with all of them integrated.
        frames: mappings with `depth`, `est_c2w` (or `c2w`) and, for color=True, `color` -- a keyframe_dict."""
        if torch.device(device).type != 'cuda':
            raise NotImplementedError("TSDFVolume needs a HIP device (csrc/tsdf.hip)")
        frames = list(frames)
        lo, hi = cls.frames_box(frames, cam, device)
        if not np.isfinite(lo).all():
            lo, hi = np.zeros(3), np.zeros(3)               # no valid depth anywhere: one empty unit
        vol = cls(voxel_length, sdf_trunc, lo - float(sdf_trunc), hi + float(sdf_trunc), cam, color=color,
                  depth_sampling_stride=depth_sampling_stride, device=device)
        for f in frames:
            vol.integrate(f['depth'], f.get('color') if color else None, f['est_c2w'] if 'est_c2w' in f else f['c2w'])
        return vol
