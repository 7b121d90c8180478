"""Replay a finished SLAM run from its output folder, headless (the reference's visualizer.py): the newest checkpoint's
estimated and ground-truth trajectories, the per-frame meshes mesh/{i:05d}_mesh.ply and a camera frustum moving along both
trajectories, rendered on the device one image per frame (evennicer_slam_amd.viz, csrc/scene_raster.hip).

    python tools/visualizer.py CONFIG [--output DIR] [--input_folder DIR] [--nice | --imap] [--save_rendering] [--no_gt_traj]
                                      [--default-config YAML] [--height 1080] [--width 1920] [--device cuda:0]

With --save_rendering the frames are written to OUTPUT/tmp_rendering/{n:06d}.jpg; they are the product: no video is
encoded, the ffmpeg line that makes one is printed.  --vis_input_frame (the reference's OpenCV window with the input
frames) is accepted and ignored.  The reference's YAML files are not part of this repository: --default-config names the
root of a configuration chain that names no parent (the reference passes configs/nice_slam.yaml or configs/imap.yaml)."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main(argv=None, frontend=None):
    """frontend: the class to draw with (default viz.SLAMFrontend).  Returns the number of frames rendered."""
    ap = argparse.ArgumentParser(description='Arguments to visualize the SLAM process.')
    ap.add_argument('config', type=str, help='Path to config file.')
    ap.add_argument('--input_folder', type=str, help='input folder; only the input-frame window of the reference reads it')
    ap.add_argument('--output', type=str, help='output folder, this has higher priority than the one in the config file')
    nice = ap.add_mutually_exclusive_group(required=False)
    nice.add_argument('--nice', dest='nice', action='store_true')
    nice.add_argument('--imap', dest='nice', action='store_false')
    ap.set_defaults(nice=True)
    ap.add_argument('--save_rendering', action='store_true', help='write every frame to OUTPUT/tmp_rendering')
    ap.add_argument('--vis_input_frame', action='store_true', help='accepted and ignored: there is no window')
    ap.add_argument('--no_gt_traj', action='store_true', help='do not draw the ground-truth trajectory')
    ap.add_argument('--default-config', default=None)
    ap.add_argument('--height', type=int, default=1080)
    ap.add_argument('--width', type=int, default=1920)
    ap.add_argument('--device', default='cuda:0')
    args = ap.parse_args(argv)

    import torch
    from evennicer_slam_amd.config import load_config
    from evennicer_slam_amd.eval_ate import latest_checkpoint
    if frontend is None:
        from evennicer_slam_amd.viz import SLAMFrontend as frontend

    cfg = load_config(args.config, args.default_config)
    scale = cfg['scale']
    output = cfg['data']['output'] if args.output is None else args.output
    if args.vis_input_frame:
        print('--vis_input_frame: there is no window to show the input frames in; ignored')
    ckpt_path = latest_checkpoint(f'{output}/ckpts')
    if ckpt_path is None:
        raise SystemExit(f'no checkpoint under {output}/ckpts')
    print('Get ckpt :', ckpt_path)
    ckpt = torch.load(ckpt_path, map_location=torch.device('cpu'), weights_only=False)
    estimate_c2w_list, gt_c2w_list, N = ckpt['estimate_c2w_list'], ckpt['gt_c2w_list'], ckpt['idx']
    estimate_c2w_list[:, :3, 3] /= scale
    gt_c2w_list[:, :3, 3] /= scale
    estimate_c2w_list = estimate_c2w_list.cpu().numpy()
    gt_c2w_list = gt_c2w_list.cpu().numpy()

    front = frontend(output, init_pose=estimate_c2w_list[0], cam_scale=0.3, save_rendering=args.save_rendering, near=0,
                     estimate_c2w_list=estimate_c2w_list, gt_c2w_list=gt_c2w_list, H=args.height, W=args.width,
                     device=args.device).start()
    for i in range(0, N + 1):
        meshfile = f'{output}/mesh/{i:05d}_mesh.ply'
        if os.path.isfile(meshfile):
            front.update_mesh(meshfile)
        front.update_pose(1, estimate_c2w_list[i], gt=False)
        if not args.no_gt_traj:
            front.update_pose(1, gt_c2w_list[i], gt=True)
        if i % 10 == 0:
            front.update_cam_trajectory(i, gt=False)
            if not args.no_gt_traj:
                front.update_cam_trajectory(i, gt=True)
        front.render()
    front.join()
    if args.save_rendering:
        print(f"{N + 1} frames in {output}/tmp_rendering; for a video:\n"
              f"ffmpeg -f image2 -r 30 -pattern_type glob -i '{output}/tmp_rendering/*.jpg' -y {output}/vis.mp4")
    return N + 1


if __name__ == '__main__':
    main()
