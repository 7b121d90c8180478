#!/usr/bin/env python3
"""Golden fixture for the iMAP mode (configs/imap.yaml): tests/golden/tiny_imap.npz.

Runs the reference on the CPU with the recipe of make_golden.py: its configuration loader over configs/imap.yaml with the
tiny scene's bound, its `config.get_model(cfg, nice=False)` decoder (seeded; biases perturbed so that no term is
identically zero) and its `Renderer` with slam.nice False.  Records
  * the decoder's state dict as names, shapes and SHA-256 digests of its float32 bytes (sd_names, sd_shape_*,
    sd_sha256), with the seeds that rebuild it (torch.manual_seed(seed) + get_model, then the bias perturbation drawn from
    a generator seeded with bias_seed): the tests rebuild the weights and check the digests instead of storing 0.9 MB;
  * `Renderer.eval_points` on points inside and outside the bound (ep_*);
  * `render_batch_ray` on the 64 rays of tiny_scene.npz (zero-depth band, rays that leave the bound) with N_importance 0
    and 12: depth, var, rgb, and the gradients of the mapper's iMAP loss (Mapper.py:555-570: L1 depth on gt_depth > 0
    + w_color_loss * L1 colour + 0.0005 * sum |sigma| of `regulation`) with respect to the decoder's parameters and to
    rays_o / rays_d (i{0,12}_*); of each [256, K] weight's gradient only the rows GRAD_ROWS (every eighth) are kept;
  * `regulation`'s torch.rand draw (reg_t_rand), its sigma and the gradient of sum |sigma| alone (reg_*).
Only build-container infrastructure: nothing under tests/, bench.py or smoke() imports this file."""
import hashlib
import os
import sys
import types

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as MG  # noqa: E402

import numpy as np  # noqa: E402
import torch  # noqa: E402

SEED = 1234
BIAS_SEED = 1235
W_COLOR = 0.05                     # configs/imap.yaml mapping.w_color_loss
GRAD_ROWS = np.arange(0, 256, 8)                           # rows kept of the [256, K] weights' gradients (size)


def grad_rows(name, g):
    return g[GRAD_ROWS] if name.startswith('pts_linears.') and name.endswith('weight') else g


def imap_cfg(n_importance):
    cfg = MG.config.load_config('configs/Replica/room0.yaml', 'configs/imap.yaml')
    tiny = MG.tiny_cfg()
    cfg['mapping']['bound'] = tiny['mapping']['bound']
    cfg['grid_len'].update(tiny['grid_len'])
    cfg['rendering']['N_importance'] = n_importance
    return cfg


def build_decoder(cfg):
    torch.manual_seed(SEED)
    model = MG.config.get_model(cfg, nice=False)
    g = torch.Generator().manual_seed(BIAS_SEED)
    with torch.no_grad():
        for name, p in model.named_parameters():
            if name.endswith('bias'):
                p.add_(torch.randn(p.shape, generator=g) * 0.05)
    return model


def make_renderer(cfg, bound, cam):
    slam = types.SimpleNamespace(nice=False, bound=bound, **cam)
    return MG.Renderer(cfg, None, slam)


def main():
    torch.set_num_threads(8)
    s = dict(np.load(os.path.join(HERE, 'tiny_scene.npz')))
    cam = dict(H=48, W=64, fx=50.0, fy=50.0, cx=31.5, cy=23.5)
    out = {}
    ro0, rd0 = torch.from_numpy(s['rays_o']), torch.from_numpy(s['rays_d'])
    gd, gc = torch.from_numpy(s['gt_depth']), torch.from_numpy(s['gt_color'])
    N = ro0.shape[0]
    for k in ('rays_o', 'rays_d', 'gt_depth', 'gt_color', 'cam'):
        out[k] = s[k]

    for n_imp in (0, 12):
        cfg = imap_cfg(n_imp)
        bound = MG.ref_bound(cfg)
        model = build_decoder(cfg)
        renderer = make_renderer(cfg, bound, cam)
        assert renderer.perturb == 0 and renderer.N_surface == 0 and not renderer.occupancy
        if n_imp == 12:
            out['bound'] = bound.numpy()
            out['N_samples'] = np.array(cfg['rendering']['N_samples'])
            out['w_color'] = np.array(W_COLOR)
            out['bias_seed'] = np.array(BIAS_SEED)
            out['seed'] = np.array(SEED)
            sd = model.state_dict()
            out['sd_names'] = np.array(list(sd))
            out['sd_sha256'] = np.array([hashlib.sha256(v.numpy().astype('<f4').tobytes()).hexdigest() for v in sd.values()])
            for k, v in sd.items():
                out['sd_shape_' + k] = np.array(v.shape, dtype=np.int64)
            out['grad_rows'] = GRAD_ROWS
            # eval_points: a lattice over the bound enlarged by 15 %, so that some points fall outside
            g = torch.Generator().manual_seed(3)
            lo, hi = bound[:, 0], bound[:, 1]
            mid, half = (lo + hi) / 2, (hi - lo) / 2 * 1.15
            pts = (mid + (torch.rand(700, 3, generator=g, dtype=torch.float64) * 2 - 1) * half)
            pts[:4] = bound[:, 0]                              # exactly on the bound: outside (strict)
            with torch.no_grad():
                raw = renderer.eval_points(pts, model, None, 'color', 'cpu')
            out['ep_pts'], out['ep_raw'] = pts.numpy(), raw.numpy()
            print('eval_points outside', int((raw[:, 3] == 100).sum()), 'of', pts.shape[0])

        ro, rd = ro0.clone().requires_grad_(True), rd0.clone().requires_grad_(True)
        depth, var, color = renderer.render_batch_ray(None, model, rd, ro, 'cpu', 'color', gt_depth=gd)
        m = gd > 0
        loss = torch.abs(gd[m] - depth[m]).sum() + W_COLOR * torch.abs(gc - color).sum()
        torch.manual_seed(11)
        t_rand = torch.rand((N, renderer.N_samples))
        torch.manual_seed(11)
        sigma = renderer.regulation(None, model, rd, ro, gd, 'cpu', 'color')
        loss = loss + 0.0005 * torch.abs(sigma).sum()
        loss.backward()
        p = f'i{n_imp}_'
        out[p + 'depth'], out[p + 'var'], out[p + 'color'] = depth.detach().numpy(), var.detach().numpy(), color.detach().numpy()
        out[p + 'loss'] = loss.detach().numpy()
        out[p + 'g_rays_o'], out[p + 'g_rays_d'] = ro.grad.numpy(), rd.grad.numpy()
        for k, v in model.named_parameters():
            out[p + 'g_' + k] = grad_rows(k, v.grad.numpy())
        if n_imp == 12:
            out['reg_t_rand'] = t_rand.numpy()
            out['reg_sigma'] = sigma.detach().numpy()
            model.zero_grad()
            torch.manual_seed(11)
            torch.abs(renderer.regulation(None, model, rd0, ro0, gd, 'cpu', 'color')).sum().backward()
            for k, v in model.named_parameters():
                out['reg_g_' + k] = grad_rows(k, v.grad.numpy())
        print('N_importance', n_imp, 'loss', loss.item(), 'depth[:3]', out[p + 'depth'][:3])
    path = os.path.join(HERE, 'tiny_imap.npz')
    np.savez_compressed(path, **out)
    print('bytes', os.path.getsize(path))


if __name__ == '__main__':
    main()
