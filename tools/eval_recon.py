"""Reconstruction metrics of a mesh against its ground truth (the reference's src/tools/eval_recon.py): accuracy, completion
and completion ratio of 200 000 surface samples each (-3d), and the depth L1 of 1 000 random 500 x 500 views (-2d), after
the ICP alignment of the reconstructed mesh's vertices onto the ground truth's.  Prints one JSON line.

    python tools/eval_recon.py --rec_mesh rec.ply --gt_mesh gt.ply -3d -2d [--seed 0] [--no-align] [--device cuda:0]

-2d reads the points no view may see from <gt_mesh without .ply>_pc_unseen.npy, as the reference does.  The camera origins
are drawn from the AXIS-ALIGNED bounding box of the ground-truth mesh with the reference's shrink factors (extents x (0.3,
0.7, 0.7), lifted 0.4 along z); the reference fits an oriented box instead.  The depth renderer's near plane is 0 (the
reference's renderer derives one from the scene's bounding box); its far plane is the reference's 20."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description="Score a reconstructed mesh against its ground truth; prints one JSON line.")
    ap.add_argument('--rec_mesh', type=str, required=True, help='PLY file of the reconstruction')
    ap.add_argument('--gt_mesh', type=str, required=True, help='PLY file of the ground truth')
    ap.add_argument('-2d', '--metric_2d', action='store_true', help='depth L1 over random views (needs a HIP device; the camera '
                    'origins come from the axis-aligned box of the ground truth with the reference\'s shrink factors, not '
                    'from an oriented box)')
    ap.add_argument('-3d', '--metric_3d', action='store_true', help='accuracy, completion and completion ratio of surface samples')
    ap.add_argument('--seed', type=int, default=0, help='seed of the surface samples and of the views')
    ap.add_argument('--no-align', dest='align', action='store_false', help='skip the ICP alignment')
    ap.add_argument('--n_imgs', type=int, default=1000)
    ap.add_argument('--device', type=str, default='cuda:0')
    args = ap.parse_args()
    from evennicer_slam_amd import eval_recon as R
    rec, gt = R.load_mesh(args.rec_mesh), R.load_mesh(args.gt_mesh)
    out = {}
    if args.metric_3d:
        m = R.calc_3d_metric(rec, gt, align=args.align, seed=args.seed, device=args.device)
        out.update(accuracy_cm=m['accuracy'], completion_cm=m['completion'], completion_ratio_percent=m['completion_ratio'],
                   transform=np.asarray(m['transform']).tolist(), icp=m['icp'])
    if args.metric_2d:
        unseen = np.load(os.path.splitext(args.gt_mesh)[0] + '_pc_unseen.npy')
        extents, transform = R.view_box(gt[0])
        m = R.calc_2d_metric(rec, gt, unseen, extents, transform, align=args.align, n_imgs=args.n_imgs, seed=args.seed,
                             device=args.device)
        out.update(depth_l1_cm=m['depth_l1'], views=args.n_imgs, view_candidates=m['candidates'], views_rejected=m['rejected'])
    print(json.dumps(out))


if __name__ == '__main__':
    main()
