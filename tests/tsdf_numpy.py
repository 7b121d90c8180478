"""numpy restatement of the block-sparse TSDF volume (csrc/tsdf.hip, tsdf.py): the oracle of its tests (a plain helper
module, not a conftest).  It restates the published algorithm -- Open3D's ScalableTSDFVolume / UniformTSDFVolume integration
with the depth-to-distance multiplier, and marching cubes on the zero level -- with the arithmetic and the output order
include/enslam_hip.h writes down, on DENSE arrays over the whole unit table: no block lists, no tiles, no prefix sums.

  units      16^3 voxels, anchored at the world origin: unit = floor(p / (16 * voxel_length)) per axis; the table covers the
             integer unit box [unit_lo, unit_lo + nu), z fastest
  touch      every pixel on rows / columns 0, stride, 2 stride, ... with depth > 0: world point P in float64
             (mesher.backprojected_points' expression, the sums in a fixed order), every unit from floor((P - trunc) / L) to
             floor((P + trunc) / L) per axis
  integrate  the voxels of the units this frame touched (units opened earlier and not touched now are left alone)
  extract    vertices by (unit's table index, voxel in lattice order, axis), faces by (cell, case-table order)
"""
import numpy as np

from tests.mc_numpy import _C0, _COUNT, _EDGES

BS = 16


def mult_table(cam):
    """float64 [H,W]: length of the un-normalised pixel ray, sqrt(1 + ((u - cx) / fx)^2 + ((v - cy) / fy)^2)."""
    a = (np.arange(cam['W'], dtype=np.float64) - float(cam['cx'])) / float(cam['fx'])
    b = (np.arange(cam['H'], dtype=np.float64) - float(cam['cy'])) / float(cam['fy'])
    return np.sqrt((1.0 + (a * a)[None, :]) + (b * b)[:, None])


def pose44(c2w):
    m = np.eye(4)
    c = np.asarray(c2w, dtype=np.float64)
    m[:c.shape[0]] = c
    return m


class Volume:
    def __init__(self, voxel_length, sdf_trunc, lo, hi, cam, color=True, stride=4):
        self.vl, self.trunc, self.stride = float(voxel_length), float(sdf_trunc), int(stride)
        self.L = 16.0 * self.vl
        assert self.trunc <= self.L
        self.cam = cam
        self.unit_lo = np.floor(np.asarray(lo, np.float64) / self.L).astype(np.int64)
        self.nu = np.floor(np.asarray(hi, np.float64) / self.L).astype(np.int64) - self.unit_lo + 1
        D = tuple(int(n) * BS for n in self.nu)
        self.allocated = np.zeros(tuple(int(n) for n in self.nu), bool)      # per unit
        self.tsdf = np.zeros(D, np.float32)
        self.weight = np.zeros(D, np.float32)
        self.color = np.zeros(D + (3,), np.float32) if color else None
        self.mult = mult_table(cam)
        self.stats = []

    # ------------------------------------------------------------------ touch
    def touch(self, depth, c2w):
        """(bool [nu] of the units this frame touches, number of sampled pixels with a unit outside the table)."""
        cam, s = self.cam, self.stride
        c2w = pose44(c2w)
        jj, ii = np.meshgrid(np.arange(0, cam['H'], s), np.arange(0, cam['W'], s), indexing='ij')
        d = np.asarray(depth, np.float32)[jj, ii].astype(np.float64)
        ok = d > 0
        jj, ii, d = jj[ok].astype(np.float64), ii[ok].astype(np.float64), d[ok]
        c = [(ii - cam['cx']) / cam['fx'] * d, -(jj - cam['cy']) / cam['fy'] * d, -d]
        P = np.stack([((c[0] * c2w[k, 0] + c[1] * c2w[k, 1]) + c[2] * c2w[k, 2]) + c2w[k, 3] for k in range(3)], 1)
        ulo = np.floor((P - self.trunc) / self.L)
        uhi = np.floor((P + self.trunc) / self.L)
        touched = np.zeros(self.allocated.shape, bool)
        outside = np.zeros(P.shape[0], bool)
        lo, nu = self.unit_lo.astype(np.float64), self.nu.astype(np.float64)
        for dx in range(3):
            for dy in range(3):
                for dz in range(3):
                    u = ulo + np.array([dx, dy, dz], np.float64)
                    live = (u <= uhi).all(axis=1)
                    inside = ((u >= lo) & (u < lo + nu)).all(axis=1)
                    outside |= live & ~inside
                    k = (u[live & inside] - lo).astype(np.int64)
                    touched[k[:, 0], k[:, 1], k[:, 2]] = True
        return touched, int(outside.sum())

    # ------------------------------------------------------------------ integrate
    def integrate(self, depth, color, c2w):
        cam = self.cam
        H, W, fx, fy, cx, cy = (cam[k] for k in ('H', 'W', 'fx', 'fy', 'cx', 'cy'))
        depth = np.asarray(depth, np.float32)
        touched, outside = self.touch(depth, c2w)
        self.allocated |= touched
        w2c = np.linalg.inv(pose44(c2w))
        vox = np.repeat(np.repeat(np.repeat(touched, BS, 0), BS, 1), BS, 2)
        ix, iy, iz = np.nonzero(vox)
        g = np.stack([ix, iy, iz], 1) + self.unit_lo * BS
        ctr = (g.astype(np.float64) + 0.5) * self.vl
        p = [((w2c[k, 0] * ctr[:, 0] + w2c[k, 1] * ctr[:, 1]) + w2c[k, 2] * ctr[:, 2]) + w2c[k, 3] for k in range(3)]
        zc = -p[2]
        with np.errstate(divide='ignore', invalid='ignore'):
            uf = (p[0] * fx / zc + cx) + 0.5
            vf = ((-p[1]) * fy / zc + cy) + 0.5
        ok = (zc > 0) & (uf >= 1e-4) & (uf < W - 1e-4) & (vf >= 1e-4) & (vf < H - 1e-4)
        u = np.where(ok, uf, 0).astype(np.int64)
        v = np.where(ok, vf, 0).astype(np.int64)
        d = depth[v, u].astype(np.float64)
        ok &= d > 0
        sdf = (d - zc) * self.mult[v, u]
        skipped = ok & (sdf <= -self.trunc)
        ok &= ~skipped
        t = np.minimum(1.0, sdf / self.trunc).astype(np.float32)
        sel = (ix[ok], iy[ok], iz[ok])
        w = self.weight[sel]
        one = np.float32(1.0)
        self.tsdf[sel] = (self.tsdf[sel] * w + t[ok]) / (w + one)
        if self.color is not None:
            col = np.asarray(color, np.float32)[v[ok], u[ok]]
            self.color[sel] = (self.color[sel] * w[:, None] + col) / (w[:, None] + one)
        self.weight[sel] = w + one
        self.stats.append(dict(blocks=int(self.allocated.sum()), touched=int(touched.sum()), touched_outside=outside,
                               integrated_voxels=int(ok.sum()), clipped=int((ok & (sdf >= self.trunc)).sum()),
                               skipped_behind=int(skipped.sum())))

    # ------------------------------------------------------------------ views the tests compare with
    def units(self):
        """Allocated units as a set of (ux, uy, uz) world unit indices."""
        return {tuple(int(x) for x in (np.array(k) + self.unit_lo)) for k in zip(*np.nonzero(self.allocated))}

    def block(self, unit):
        """(tsdf [16,16,16], weight [16,16,16], color [16,16,16,3] or None) of a world unit index."""
        k = (np.asarray(unit) - self.unit_lo) * BS
        s = tuple(slice(int(a), int(a) + BS) for a in k)
        return self.tsdf[s], self.weight[s], (self.color[s] if self.color is not None else None)

    # ------------------------------------------------------------------ extraction
    def cells(self):
        """(valid bool [D], neg bool [D], cell_valid bool [D], case int64 [D]): a cell is named by its lowest corner."""
        valid = self.weight > 0
        neg = self.tsdf < 0
        D = valid.shape
        cv = np.zeros(D, bool)
        case = np.zeros(D, np.int64)
        core = np.ones(tuple(n - 1 for n in D), bool)
        cs = np.zeros(core.shape, np.int64)
        for c in range(8):
            dx, dy, dz = c & 1, (c >> 1) & 1, (c >> 2) & 1
            s = (slice(dx, D[0] - 1 + dx), slice(dy, D[1] - 1 + dy), slice(dz, D[2] - 1 + dz))
            core &= valid[s]
            cs += neg[s].astype(np.int64) << c
        cv[:-1, :-1, :-1] = core
        case[:-1, :-1, :-1] = np.where(core, cs, 0)
        return valid, neg, cv, case

    def edge_masks(self):
        """(crossing [3] of bool [D]: the +a edge of the voxel changes sign between two observed voxels,
            vertex [3] of bool [D]: ... and one of the up to four cells sharing it is valid)."""
        valid, neg, cv, _ = self.cells()
        D = valid.shape
        pad = np.zeros(tuple(n + 1 for n in D), bool)
        pad[1:, 1:, 1:] = cv                                    # pad[x+1, y+1, z+1] = cv[x, y, z]; index 0 = cell -1 (absent)
        crossing, vertex = [], []
        for a in range(3):
            lo, hi = [slice(None)] * 3, [slice(None)] * 3
            lo[a], hi[a] = slice(0, -1), slice(1, None)
            m = np.zeros(D, bool)
            m[tuple(lo)] = valid[tuple(lo)] & valid[tuple(hi)] & (neg[tuple(lo)] != neg[tuple(hi)])
            b, c = [x for x in range(3) if x != a]
            share = np.zeros(D, bool)
            for db in (0, 1):
                for dc in (0, 1):
                    s = [slice(1, None)] * 3
                    s[b] = slice(1 - db, D[b] + 1 - db)
                    s[c] = slice(1 - dc, D[c] + 1 - dc)
                    share |= pad[tuple(s)]
            crossing.append(m)
            vertex.append(m & share)
        return crossing, vertex

    def _order_key(self, ix, iy, iz):
        """Rank of a dense voxel in the output order: (table index of its unit, lattice index inside the unit)."""
        nu = self.nu
        t = ((ix // BS) * nu[1] + (iy // BS)) * nu[2] + (iz // BS)
        loc = ((ix % BS) * BS + (iy % BS)) * BS + (iz % BS)
        return t * BS ** 3 + loc

    def extract_mesh(self):
        """(vertices float64 [V,3], faces int32 [F,3], colors uint8 [V,3] or None)."""
        _, _, cv, case = self.cells()
        _, vertex = self.edge_masks()
        D = self.weight.shape
        t64 = self.tsdf.astype(np.float64)
        # vertices: sort (voxel order key, axis)
        vx, vy, vz, va = [], [], [], []
        for a in range(3):
            x, y, z = np.nonzero(vertex[a])
            vx.append(x), vy.append(y), vz.append(z), va.append(np.full(x.shape, a, np.int64))
        vx, vy, vz, va = (np.concatenate(q) for q in (vx, vy, vz, va))
        order = np.argsort(self._order_key(vx, vy, vz) * 3 + va, kind='stable')
        vx, vy, vz, va = vx[order], vy[order], vz[order], va[order]
        vid = np.full(D + (3,), -1, np.int64)
        vid[vx, vy, vz, va] = np.arange(vx.size)
        idx = np.stack([vx, vy, vz], 1)
        nb = idx.copy()
        nb[np.arange(vx.size), va] += 1
        ta = t64[vx, vy, vz]
        tb = t64[nb[:, 0], nb[:, 1], nb[:, 2]]
        frac = ta / (ta - tb)
        verts = ((idx + self.unit_lo * BS).astype(np.float64) + 0.5) * self.vl
        verts[np.arange(vx.size), va] += frac * self.vl
        colors = None
        if self.color is not None:
            ca = self.color[vx, vy, vz].astype(np.float64)
            cb = self.color[nb[:, 0], nb[:, 1], nb[:, 2]].astype(np.float64)
            col = ca + frac[:, None] * (cb - ca)
            colors = np.floor(np.clip(col, 0.0, 1.0) * 255.0 + 0.5).astype(np.uint8)
        # faces: cells in voxel order, the case table's triangles in table order
        cx, cy, cz = np.nonzero(cv & (_COUNT[case] > 0))
        order = np.argsort(self._order_key(cx, cy, cz), kind='stable')
        cx, cy, cz = cx[order], cy[order], cz[order]
        cs = case[cx, cy, cz]
        nt = _COUNT[cs]
        cell = np.repeat(np.arange(cs.size), nt)
        k = np.arange(cell.size) - np.repeat(np.cumsum(nt) - nt, nt)
        faces = np.empty((cell.size, 3), np.int64)
        for j in range(3):
            e = _EDGES[cs[cell], 3 * k + j]
            c0 = _C0[e]
            faces[:, j] = vid[cx[cell] + (c0 & 1), cy[cell] + ((c0 >> 1) & 1), cz[cell] + ((c0 >> 2) & 1), e >> 2]
        assert (faces >= 0).all()
        return verts, faces.astype(np.int32), colors
