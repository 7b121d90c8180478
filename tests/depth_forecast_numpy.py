"""Yardstick of the depth forecast (enslam_depth_forecast), written from the header of csrc/depth_forecast.hip: one source
pixel at a time in Python floats (IEEE float64, one operation per expression node, nothing fused), a dict as the z-buffer and
numpy.float32 for the one rounding.  Slow and obvious on purpose; the device kernel and the numpy route of
functional.depth_forecast are held to its bits."""
import math
import struct

import numpy as np


def spacing(n_src, n_dst):
    return (n_src - 1) / (n_dst - 1) if n_dst > 1 else 1.0


def f32_bits(x):
    return struct.unpack('<I', struct.pack('<f', x))[0]


def project(d, j, i, cam, M, z_near):
    """(u, v, z32) of source pixel (j, i) with depth d, or None when it is no point / not kept."""
    fx, fy, cx, cy = cam['fx'], cam['fy'], cam['cx'], cam['cy']
    d = float(d)
    if not (d > 0.0) or not math.isfinite(d):
        return None
    px = (i - cx) / fx
    py = -(j - cy) / fy
    p = (d * px, d * py, -d)
    q = [((float(M[r][0]) * p[0] + float(M[r][1]) * p[1]) + float(M[r][2]) * p[2]) + float(M[r][3]) for r in range(3)]
    z = -q[2]
    if not (z > z_near):
        return None
    with np.errstate(over='ignore'):
        z32 = np.float32(z)
    if not np.isfinite(z32):
        return None
    u = cx + fx * (q[0] / z)
    v = cy - fy * (q[1] / z)
    return u, v, z32


def vote_target(u, v, sx, sy, Ho, Wo, radius):
    """The target pixel (jo, io) the position (u, v) votes for, or None."""
    if not (math.isfinite(u) and math.isfinite(v)):
        return None
    fi = math.floor(u / sx + 0.5)
    fj = math.floor(v / sy + 0.5)
    if not (0 <= fi <= Wo - 1) or not (0 <= fj <= Ho - 1):
        return None
    if not (abs(u - fi * sx) <= radius) or not (abs(v - fj * sy) <= radius):
        return None
    return fj, fi


def votes(depth, cam, M, Ho, Wo, radius, z_near):
    """dict (jo, io) -> list of float32 depths voted for the pixel, in source order."""
    H, W = depth.shape
    sx, sy = spacing(W, Wo), spacing(H, Ho)
    out = {}
    for j in range(H):
        for i in range(W):
            r = project(depth[j, i], j, i, cam, M, float(z_near))
            if r is None:
                continue
            t = vote_target(r[0], r[1], sx, sy, Ho, Wo, float(radius))
            if t is not None:
                out.setdefault(t, []).append(r[2])
    return out


def forecast(depth, cam, M, Ho, Wo, radius, z_near, fill):
    """float32 [Ho,Wo]: the forecast image of the model."""
    zbuf = {}
    for t, zs in votes(depth, cam, M, Ho, Wo, radius, z_near).items():
        zbuf[t] = min(zs, key=lambda z: f32_bits(float(z)))         # unsigned integer minimum on the bit patterns
    out = np.zeros((Ho, Wo), dtype=np.float32)
    for (jo, io), z in zbuf.items():
        out[jo, io] = z
    if fill:
        for jo in range(Ho):
            for io in range(Wo):
                if (jo, io) in zbuf:
                    continue
                near = [zbuf[(jo + dj, io + di)] for dj in (-1, 0, 1) for di in (-1, 0, 1) if (jo + dj, io + di) in zbuf]
                if near:
                    out[jo, io] = max(near, key=lambda z: f32_bits(float(z)))
    return out
