"""Cull a mesh by a trajectory (the reference's src/tools/cull_mesh.py): the faces all of whose vertices lie outside every
camera's frustum are dropped; the vertices (and their colours) stay.

    python tools/cull_mesh.py --input_mesh in.ply --traj traj.txt --output_mesh out.ply [--device cuda:0]

The trajectory file holds one camera-to-world matrix per line, 16 floats, row-major; the y and z columns are negated as the
reference's loader does.  The camera defaults are the reference's Replica values."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402


def load_poses(path):
    """float32 [n,4,4] camera-to-world matrices of a trajectory file in this project's axes (the camera looks down -z): the
    file's y and z camera axes point the other way, so those two columns change sign.  Float32, as the reference keeps them."""
    poses = np.loadtxt(path, dtype=np.float64, ndmin=2).reshape(-1, 4, 4)
    poses[:, :3, 1:3] = -poses[:, :3, 1:3]
    return poses.astype(np.float32)


def main():
    ap = argparse.ArgumentParser(description="Drop the faces of a mesh that no camera of a trajectory can see.")
    ap.add_argument('--input_mesh', type=str, required=True, help='PLY file to read')
    ap.add_argument('--traj', type=str, required=True, help='text file, one row-major 4x4 camera-to-world matrix per line')
    ap.add_argument('--output_mesh', type=str, required=True, help='PLY file to write')
    for name, default in (('H', 680), ('W', 1200)):
        ap.add_argument(f'--{name}', type=int, default=default)
    for name, default in (('fx', 600.0), ('fy', 600.0), ('cx', 599.5), ('cy', 339.5)):
        ap.add_argument(f'--{name}', type=float, default=default)
    ap.add_argument('--device', type=str, default='cuda:0')
    args = ap.parse_args()
    from evennicer_slam_amd import eval_recon as R
    from evennicer_slam_amd.mesher import write_ply
    v, f, colors = R.load_mesh(args.input_mesh)
    cam = dict(H=args.H, W=args.W, fx=args.fx, fy=args.fy, cx=args.cx, cy=args.cy)
    kept = R.cull_mesh(v, f, list(load_poses(args.traj)), cam, device=args.device)
    write_ply(args.output_mesh, v, kept, colors)
    print(f"{len(f) - len(kept)} of {len(f)} faces culled")


if __name__ == '__main__':
    main()
