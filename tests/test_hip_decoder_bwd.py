"""-m gpu: the NICE decoder backward (decoder_bwd_kernel, decoder_bwd_split_kernel, decoder_bwd_light_kernel, grid_bwd_kernel,
the two-kernel and deferred-scatter forms) against the float64 yardstick of tests/decoder_bwd_numpy.py, elementwise, through
the C ABI by hand: enslam_render_fwd fills the activation workspace, then the backward entry points run on a d_raw the test
chooses.  Cases, fragility rule and the bar: tests/decoder_bwd_cases.py (|device - yardstick| <= 8 * e_rel * A[element],
e_rel the float32 CPU oracle's own worst error per tensor family; exactly 0 where A == 0).  Every route is checked against
the yardstick, never against another route.  Every output buffer has GUARD sentinel rows behind it.
Run with -s to see the worst |error| / (e_rel * A) per family of every case.

Measured on the MI355X (bar 8; grids / rays_o / rays_d / weights / biases, worst over all routes and shapes): coarse 3.3 / 2.0 /
1.5 / 1.4 / 2.1, middle 5.0 / 3.2 / 2.8 / 1.2 / 3.4, fine 3.7 / 1.4 / 2.0 / 1.6 / 2.7, colour 5.3 / 2.2 / 6.7 / 1.6 / 6.3."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import decoder_bwd_cases as BC
from tests import decoder_cases as DC
from tests.test_hip_decoder_fwd import GUARD, SENTINEL, scene_struct

pytestmark = pytest.mark.gpu

STAGES = BC.STAGES
XYZ_STAGES = ('middle', 'fine', 'color')
ALL_SHAPES = [(n, s) for n in BC.SHAPES_N for s in BC.SHAPES_S]
MULTI = ('W+1', 64)                                       # N = workgroup count + 1: several rounds per role, the last one ragged
FEW_SHAPES = list(BC.LISTED_SHAPES) + [MULTI]
ROW = 32                                                  # floats of a sentinel row behind the flat buffers
DEFER = os.environ.get('ENSLAM_DEFER_SCATTER', '0')[:1] in ('1', '2')
GRID_KIND = {'grid_coarse': 0, 'grid_middle': 1, 'grid_fine': 2, 'grid_color': 3}
ROUTES = {'recompute': dict(workspace=None), 'saved_handoff': dict(workspace='full', handoff=True),
          'saved_inline': dict(workspace='full')}


def _id(stage, shape, *more):
    n, s = shape
    return '-'.join([stage, 'multiround' if n == 'W+1' else f'N{n}', f'S{s}'] + [str(m) for m in more]) + '-'


@pytest.fixture(scope='module')
def dev():
    import evennicer_slam_amd as E
    import evennicer_slam_amd.functional as EF
    from tests.hip_util import DEV, model_from_state
    bound = torch.from_numpy(DC.scene()[2].copy())
    models = {'generic': model_from_state(DC.state_arrays('generic'), bound)}
    grids = {k: torch.from_numpy(v.copy()).to(DEV) for k, v in DC.scene()[1].items()}
    lib = E._lib.lib()
    W = int(lib.enslam_bwd_max_workgroups())
    assert W >= 1
    return dict(E=E, EF=EF, L=E._lib, lib=lib, DEV=DEV, bound=bound, coarse_bound=bound * 2, models=models, grids=grids, W=W)


def the_case(dev, stage, shape, listed=False):
    n, s = shape
    c = BC.case(stage, dev['W'] + 1 if n == 'W+1' else n, s, listed)
    BC.check_case(c)
    return c


def param_names(L, kind):
    dec = L.MLP_NAMES[kind]
    names = [f'{dec}.pts_linears.{i}.{w}' for i in range(5) for w in ('weight', 'bias')]
    if kind != L.MLP_COARSE:
        names += [f'{dec}.fc_c.{i}.{w}' for i in range(5) for w in ('weight', 'bias')]
    names += [f'{dec}.output_linear.weight', f'{dec}.output_linear.bias']
    return names + ([f'{dec}.embedder._B'] if kind != L.MLP_COARSE else [])


def guarded(dev, n, fill=0.0):
    """flat float32 buffer of n floats holding `fill`, GUARD sentinel rows behind it"""
    buf = torch.full((n + GUARD * ROW,), SENTINEL, dtype=torch.float32, device=dev['DEV'])
    buf[:n] = fill
    return buf


def guard_intact(buf, n, what, label):
    tail = buf[n:]
    if not bool((tail == SENTINEL).all()):
        at = int((tail != SENTINEL).nonzero()[0])
        raise AssertionError(f"{label}: {what}: float {at} behind the buffer's end was written ({float(tail[at])!r})")


class Run:
    """one backward through the C ABI.  workspace: None (recompute), 'full' or 'light'; handoff: dgrid_ws given (then the ray
    gradients come from enslam_ray_grad_bwd, or from the finish launch with finish=True); grids / params: the names / kinds
    that get an accumulator (None: all of the stage); rays: g_rays_o / g_rays_d wanted; scale: *d_raw_scale; listed: the case's
    work list is passed; partials: grad_partial buffers for the decoders with parameter gradients; calls: how many times the
    backward runs into the same accumulators"""

    def __init__(self, dev, c, workspace=None, handoff=False, grids=None, params=None, rays=True, scale=None, listed=False,
                 partials=False, finish=False, calls=1, label=''):
        EF, L, lib = dev['EF'], dev['L'], dev['lib']
        P, st, D = EF._ptr, EF._stream(), dev['DEV']
        self.dev, self.c, self.label = dev, c, label
        stage, N, S = c.stage, c.N, c.S
        sid = L.STAGE[stage]
        kinds = L.STAGE_KINDS[stage]
        self.kinds = kinds
        ro, rd, z = (torch.from_numpy(a.copy()).to(D) for a in (c.ro, c.rd, c.z))
        d_raw = torch.from_numpy(c.d_raw.copy()).to(D)
        sc, keep = scene_struct(dev, 'generic', stage)
        saved = workspace is not None and stage != 'coarse'
        light = int(workspace == 'light')
        act = None
        if saved:
            act = torch.empty(lib.enslam_activation_floats(sid, N, S, light), dtype=torch.float32, device=D)
            depth, var = (torch.empty(N, dtype=torch.float64, device=D) for _ in range(2))
            rgb = torch.empty((N, 3), dtype=torch.float32, device=D)
            raw = torch.empty((N * S, 4), dtype=torch.float32, device=D)
            L.check(lib.enslam_render_fwd(sid, N, S, P(ro), P(rd), P(z), ctypes.byref(sc), P(depth), P(var), P(rgb), P(raw), P(act), light, st),
                    "enslam_render_fwd")
        # the hand-off starts as NaN: a kernel that reads a tile nobody wrote there shows in the ray gradients
        dgw = torch.full((lib.enslam_grid_handoff_floats(sid, N, S),), float('nan'), dtype=torch.float32, device=D) if handoff and saved else None
        grid_names = [L.GRID_NAMES[k] for k in kinds] if grids is None else list(grids)
        par_kinds = list(kinds) if params is None else list(params)
        gg, gpk, gpart = (L.Grid * 4)(), (ctypes.c_void_p * 4)(), (ctypes.c_void_p * 4)()
        self.vm, self.packed, self.part = {}, {}, {}
        for k in kinds:
            name = L.GRID_NAMES[k]
            dims = tuple(int(v) for v in dev['grids'][name].shape[2:])
            gg[k].D, gg[k].H, gg[k].W = dims
            if name in grid_names:
                self.vm[name] = guarded(dev, int(np.prod(dims)) * 32)
                gg[k].data = self.vm[name].data_ptr()
            if k in par_kinds:
                # with partial images the accumulator must still be given and must stay unwritten: it holds sentinels
                self.packed[k] = guarded(dev, lib.enslam_packed_grad_floats(k), SENTINEL if partials else 0.0)
                gpk[k] = self.packed[k].data_ptr()
                if partials:
                    self.part[k] = guarded(dev, lib.enslam_bwd_partial_floats(k), float('nan'))
                    gpart[k] = self.part[k].data_ptr()
        self.g_ro = guarded(dev, 3 * N) if rays else None
        self.g_rd = guarded(dev, 3 * N) if rays else None
        work = wcount = None
        if listed:
            assert c.work is not None
            n_tiles = N * (S // 16)
            work = torch.full((n_tiles + GUARD,), -1, dtype=torch.int32, device=D)     # (an id read past the count would be -1)
            work[:len(c.work)] = torch.from_numpy(c.work.copy()).to(D)
            wcount = torch.tensor([len(c.work)], dtype=torch.int32, device=D)
        dscale = None if scale is None else torch.tensor([scale], dtype=torch.float64, device=D)
        for _ in range(calls):
            if partials:
                L.check(lib.enslam_decoder_bwd_partials(sid, N, S, P(ro), P(rd), P(z), ctypes.byref(sc), P(d_raw), P(dscale), P(act), light,
                                                        P(dgw), gg, gpk, gpart, P(self.g_ro), P(self.g_rd), P(work), P(wcount), st),
                        "enslam_decoder_bwd_partials")
            elif listed or scale is not None:
                L.check(lib.enslam_decoder_bwd_scaled(sid, N, S, P(ro), P(rd), P(z), ctypes.byref(sc), P(d_raw), P(dscale), P(act), light,
                                                      P(dgw), gg, gpk, P(self.g_ro), P(self.g_rd), P(work), P(wcount), st),
                        "enslam_decoder_bwd_scaled")
            else:
                L.check(lib.enslam_decoder_bwd(sid, N, S, P(ro), P(rd), P(z), ctypes.byref(sc), P(d_raw), P(act), light, P(dgw), gg, gpk,
                                               P(self.g_ro), P(self.g_rd), st), "enslam_decoder_bwd")
            if dgw is not None and rays and not finish:
                L.check(lib.enslam_ray_grad_bwd(sid, N, S, P(ro), P(rd), P(z), ctypes.byref(sc), P(dgw), P(self.g_ro), P(self.g_rd), st),
                        "enslam_ray_grad_bwd")
        self.finished = None
        if finish:
            self.finished = self._finish(sid, N, S, ro, rd, z, sc, dgw if rays else None, work, wcount, partials)
        torch.cuda.synchronize()
        del keep

    def _outs(self, k):
        shapes = [self.c_shapes(n) for n in param_names(self.dev['L'], k)]
        return [torch.zeros(s, dtype=torch.float32, device=self.dev['DEV']) for s in shapes]

    def c_shapes(self, name):
        return DC.scene()[0][name].shape

    def _finish(self, sid, N, S, ro, rd, z, sc, dgw, work, wcount, partials):
        """enslam_step_finish_partials with n_conv = 0: the ray-gradient role on the hand-off and, with partial images, the sum of
        the rows while it unpacks"""
        dev = self.dev
        EF, L, lib = dev['EF'], dev['L'], dev['lib']
        P, st = EF._ptr, EF._stream()
        ks = sorted(self.part) if partials else []
        n = len(ks)
        kind_arr, pk_arr, part_arr = (ctypes.c_int32 * max(n, 1))(), (ctypes.c_void_p * max(n, 1))(), (ctypes.c_void_p * max(n, 1))()
        structs, outs = (L.MlpParams * max(n, 1))(), {}
        for j, k in enumerate(ks):
            outs[k] = self._outs(k)
            kind_arr[j], pk_arr[j], part_arr[j] = k, self.packed[k].data_ptr(), self.part[k].data_ptr()
            structs[j] = EF._fill_params_struct(k, outs[k])
        L.check(lib.enslam_step_finish_partials(0, None, None, None, None, None, n, kind_arr if n else None, pk_arr if n else None,
                                                part_arr if n else None, structs if n else None, sid, N, S, P(ro), P(rd), P(z),
                                                ctypes.byref(sc), P(dgw), P(self.g_ro), P(self.g_rd), P(work), P(wcount), st),
                "enslam_step_finish_partials")
        return outs

    def unpack(self, k, packed):
        EF, L, lib = self.dev['EF'], self.dev['L'], self.dev['lib']
        outs = self._outs(k)
        L.check(lib.enslam_unpack_mlp_grads(k, EF._ptr(packed), ctypes.byref(EF._fill_params_struct(k, outs)), EF._stream()),
                "enslam_unpack_mlp_grads")
        torch.cuda.synchronize()
        return outs

    def _named(self, k, outs):
        return {n: o.cpu().numpy().astype(np.float64) for n, o in zip(param_names(self.dev['L'], k), outs)}

    def results(self, params_from='packed'):
        """{name: float64 host array in the yardstick's shape}; checks every guard on the way"""
        lib, N = self.dev['lib'], self.c.N
        out = {}
        if self.g_ro is not None:
            for name, buf in (('rays_o', self.g_ro), ('rays_d', self.g_rd)):
                guard_intact(buf, 3 * N, name, self.label)
                out[name] = buf[:3 * N].view(N, 3).cpu().numpy().astype(np.float64)
        for name, buf in self.vm.items():
            n = buf.numel() - GUARD * ROW
            guard_intact(buf, n, name + ' (voxel-major)', self.label)
            out[name] = np.ascontiguousarray(buf[:n].view(-1, 32).cpu().numpy().astype(np.float64).T)
        for k, buf in self.packed.items():
            n = lib.enslam_packed_grad_floats(k)
            guard_intact(buf, n, f'packed gradient of decoder {k}', self.label)
            if k in self.part:
                guard_intact(self.part[k], lib.enslam_bwd_partial_floats(k), f'partial images of decoder {k}', self.label)
                assert bool((buf[:n] == SENTINEL).all()), f"{self.label}: grad_packed of decoder {k} was written although partial images were given"
            if params_from == 'packed':
                out.update(self._named(k, self.unpack(k, buf[:n])))
            elif params_from == 'rows':
                out.update(self._named(k, self.unpack(k, self.row_sum(k))))
            else:
                out.update(self._named(k, self.finished[k]))
        return out

    def row_sum(self, k):
        """float64 host sum of the rows of decoder k's partial buffer, as a float32 device image"""
        lib, W = self.dev['lib'], self.dev['W']
        gf = lib.enslam_packed_grad_floats(k)
        host = self.part[k][:lib.enslam_bwd_partial_floats(k)].cpu()
        rows = int(host[:1].view(torch.int32)[0])
        assert 1 <= rows <= W, f"{self.label}: header of decoder {k}'s partial buffer says {rows} rows; at most {W} workgroups"
        body = host[16:16 + rows * gf].view(rows, gf).numpy().astype(np.float64)
        assert np.isfinite(body).all(), f"{self.label}: a row of decoder {k}'s partial buffer was left unwritten"
        return torch.from_numpy(body.sum(axis=0).astype(np.float32)).to(self.dev['DEV'])


def check(c, got, label, factor=1.0, handoff=False):
    """every tensor of `got` against factor * yardstick; prints the worst ratio per family"""
    erel = c.erel
    assert got, label
    worst = {}
    for name, val in got.items():
        fam = BC.family_of(name)
        worst[fam] = max(worst.get(fam, 0.0), BC.worst_ratio(name, val, c.g[name] * factor, c.A[name] * abs(factor), erel[fam]))
    print(f"{label}: worst |error| / (e_rel * A): " + ", ".join(f"{k} {v:.2f}" for k, v in worst.items()))
    for name, val in got.items():
        extra = BC.DEFER_FLUSH * c.dC_max * abs(factor) if DEFER and handoff and name.startswith('grid_') else 0.0
        BC.assert_within_bar(name, val, c.g[name] * factor, c.A[name] * abs(factor), erel[BC.family_of(name)], label, extra_abs=extra)


# ------------------------------------------------------------------------------------------------ routes 1-3
@pytest.mark.parametrize("route", list(ROUTES))
@pytest.mark.parametrize("stage,shape", [(st, sh) for st in STAGES for sh in ALL_SHAPES + [MULTI]],
                         ids=[_id(st, sh) for st in STAGES for sh in ALL_SHAPES + [MULTI]])
def test_route(dev, stage, shape, route):
    """recompute (act_ws NULL), saved with hand-off + enslam_ray_grad_bwd, saved with in-kernel ray gradients: all gradients"""
    c = the_case(dev, stage, shape)
    label = f"stage {stage}, N {c.N}, S {c.S}, route {route}"
    r = Run(dev, c, label=label, **ROUTES[route])
    got = r.results()
    assert set(got) == set(c.g)
    check(c, got, label, handoff=bool(ROUTES[route].get('handoff')))


@pytest.mark.parametrize("stage", STAGES)
def test_route_adds_into_its_accumulators(dev, stage):
    """two calls into the same zeroed accumulators: twice the yardstick, within the bar"""
    c = the_case(dev, stage, (65, 48))
    for route in ROUTES:
        label = f"stage {stage}, N 65, S 48, route {route}, called twice"
        check(c, Run(dev, c, calls=2, label=label, **ROUTES[route]).results(), label, factor=2.0, handoff=bool(ROUTES[route].get('handoff')))


# ------------------------------------------------------------------------------------------------ routes 4-6
@pytest.mark.parametrize("stage,shape", [(st, sh) for st in XYZ_STAGES for sh in FEW_SHAPES],
                         ids=[_id(st, sh, 'light') for st in XYZ_STAGES for sh in FEW_SHAPES])
def test_light_route(dev, stage, shape):
    """light workspace, no parameter gradients: grid and ray gradients from decoder_bwd_light_kernel"""
    c = the_case(dev, stage, shape)
    label = f"stage {stage}, N {c.N}, S {c.S}, light"
    got = Run(dev, c, workspace='light', params=(), label=label).results()
    assert set(got) == {k for k in c.g if 'decoder' not in k}
    check(c, got, label)


@pytest.mark.parametrize("shape", FEW_SHAPES, ids=[_id('color', sh, 'mix') for sh in FEW_SHAPES])
def test_mappers_mix(dev, shape):
    """colour stage, full workspace, parameter gradients for the colour decoder only: the middle and fine roles run in the light
    kernel, the colour role in the persistent one, in the same call"""
    c = the_case(dev, 'color', shape)
    label = f"stage color, N {c.N}, S {c.S}, mapper's mix"
    got = Run(dev, c, workspace='full', handoff=True, params=(3,), label=label).results()
    assert set(got) == {k for k in c.g if 'decoder' not in k or k.startswith('color_decoder')}
    check(c, got, label, handoff=True)


@pytest.mark.parametrize("which", ['rays_only', 'one_grid', 'params_only'])
@pytest.mark.parametrize("stage,shape", [(st, sh) for st in STAGES for sh in FEW_SHAPES],
                         ids=[_id(st, sh) for st in STAGES for sh in FEW_SHAPES])
def test_only_some_outputs_wanted(dev, stage, shape, which):
    """the gradients that are asked for do not depend on the ones that are not"""
    c = the_case(dev, stage, shape)
    label = f"stage {stage}, N {c.N}, S {c.S}, {which}"
    L = dev['L']
    last_grid = L.GRID_NAMES[L.STAGE_KINDS[stage][-1]]
    kw = {'rays_only': dict(workspace='light', grids=(), params=()),                    # the tracker
          'one_grid': dict(workspace='full', grids=(last_grid,), params=(), rays=False),
          'params_only': dict(workspace='full', grids=(), rays=False)}[which]
    got = Run(dev, c, label=label, **kw).results()
    want = {'rays_only': {'rays_o', 'rays_d'}, 'one_grid': {last_grid}, 'params_only': {k for k in c.g if 'decoder' in k}}[which]
    assert set(got) == want
    check(c, got, label)


# ------------------------------------------------------------------------------------------------ route 7
@pytest.mark.parametrize("rays_by", ['inline', 'finish'])
@pytest.mark.parametrize("stage,shape", [(st, sh) for st in STAGES for sh in FEW_SHAPES],
                         ids=[_id(st, sh, 'listed') for st in STAGES for sh in FEW_SHAPES])
def test_work_list_and_scale(dev, stage, shape, rays_by):
    """enslam_decoder_bwd_scaled with the test's own work list and d_raw_scale = 0.5 (exact): half the yardstick; the ray
    gradients in the kernel, or by enslam_step_finish_partials given the same list"""
    c = the_case(dev, stage, shape, listed=True)
    label = f"stage {stage}, N {c.N}, S {c.S}, work list of {len(c.work)} of {c.N * c.S // 16} tiles, scale 0.5, rays {rays_by}"
    finish = rays_by == 'finish'
    got = Run(dev, c, workspace='full', handoff=finish, finish=finish, scale=0.5, listed=True, label=label).results()
    assert set(got) == set(c.g)
    check(c, got, label, factor=0.5, handoff=finish)


# ------------------------------------------------------------------------------------------------ route 8
@pytest.mark.parametrize("stage,shape", [(st, sh) for st in STAGES for sh in FEW_SHAPES],
                         ids=[_id(st, sh, 'partials') for st in STAGES for sh in FEW_SHAPES])
def test_partial_images(dev, stage, shape):
    """enslam_decoder_bwd_partials: at most W rows; their float64 host sum, unpacked, meets the bar; so do the same buffers through
    enslam_step_finish_partials; grad_packed of those decoders stays unwritten"""
    c = the_case(dev, stage, shape)
    label = f"stage {stage}, N {c.N}, S {c.S}, partial images"
    r = Run(dev, c, workspace='full', handoff=True, partials=True, finish=True, label=label)
    by_rows = r.results(params_from='rows')
    assert set(by_rows) == set(c.g)
    check(c, by_rows, label + ", host sum of the rows", handoff=True)
    check(c, {k: v for k, v in r.results(params_from='finish').items() if 'decoder' in k}, label + ", finish launch", handoff=True)


# ------------------------------------------------------------------------------------------------ route 9
@pytest.mark.parametrize("env", ['ENS_BWD2=1', 'ENSLAM_DEFER_SCATTER=1', 'ENS_SPLIT=0'])
def test_opt_in_form(env):
    """the switches are read once per process: this file's saved-route cases in a child pytest under each of them (the deferred
    scatter with the added term of decoder_bwd_cases.DEFER_FLUSH)"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    name, value = env.split('=')
    select = "test_route and saved and (N3- or N65- or multiround) and (S16- or S48- or multiround)"
    r = subprocess.run([sys.executable, '-m', 'pytest', '-q', '-x', '-p', 'no:cacheprovider', 'tests/test_hip_decoder_bwd.py', '-k', select],
                       cwd=root, env=dict(os.environ, **{name: value}), capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert ' passed' in r.stdout and 'failed' not in r.stdout
