"""No GPU: the sparse RGB-D schedule of the run harness (slam.frame_plan, slam.schedule_settings), the camera learning rates of
`tracking.seperate_LR` and the tools' flags.

The tables are written by hand from the reference tracker's lines (src/Tracker.py): rgbd = (idx % rgbd_every_frame == 0) (:357);
a tracked frame's events join the sum before its iterations (:351); after a frame with idx % every_frame == 0 its colour becomes
pre_gt_color and the sum restarts (:462-466); frame 0 is not tracked and starts the sum at zero (:304-311).  `map` is the
harness's rule: frame 0, every every_frame-th frame and the last one."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (n, every_frame, rgbd_every_frame) -> per frame (rgbd, anchor, integrate, map, reset)
T, F = True, False
REFERENCE = {
    (1, 5, 5): [(T, None, (), T, T)],
    (7, 1, 1): [(T, None, (), T, T), (T, 0, (1,), T, T), (T, 1, (2,), T, T), (T, 2, (3,), T, T), (T, 3, (4,), T, T),
                (T, 4, (5,), T, T), (T, 5, (6,), T, T)],
    (12, 5, 5): [(T, None, (), T, T),
                 (F, 0, (1,), F, F), (F, 0, (1, 2), F, F), (F, 0, (1, 2, 3), F, F), (F, 0, (1, 2, 3, 4), F, F),
                 (T, 0, (1, 2, 3, 4, 5), T, T),
                 (F, 5, (6,), F, F), (F, 5, (6, 7), F, F), (F, 5, (6, 7, 8), F, F), (F, 5, (6, 7, 8, 9), F, F),
                 (T, 5, (6, 7, 8, 9, 10), T, T),
                 (F, 10, (11,), T, F)],                                     # the last frame: mapped, no RGB-D, no restart
    (12, 3, 3): [(T, None, (), T, T),
                 (F, 0, (1,), F, F), (F, 0, (1, 2), F, F), (T, 0, (1, 2, 3), T, T),
                 (F, 3, (4,), F, F), (F, 3, (4, 5), F, F), (T, 3, (4, 5, 6), T, T),
                 (F, 6, (7,), F, F), (F, 6, (7, 8), F, F), (T, 6, (7, 8, 9), T, T),
                 (F, 9, (10,), F, F), (F, 9, (10, 11), T, F)],
    # the rpg.yaml shape: mapping frames 0, 3, 6, 9 and RGB-D frames 0, 5 differ
    (10, 3, 5): [(T, None, (), T, T),
                 (F, 0, (1,), F, F), (F, 0, (1, 2), F, F), (F, 0, (1, 2, 3), T, T),
                 (F, 3, (4,), F, F), (T, 3, (4, 5), F, F), (F, 3, (4, 5, 6), T, T),
                 (F, 6, (7,), F, F), (F, 6, (7, 8), F, F), (F, 6, (7, 8, 9), T, T)],
}


def dense_table(n, every):
    """today's behaviour: RGB-D and the frame's own events on every frame, the previous frame's colour"""
    return [(True, i - 1 if i else None, (i,) if i else (), i == 0 or i % every == 0 or i == n - 1, True) for i in range(n)]


@pytest.mark.parametrize('shape', sorted(REFERENCE))
def test_frame_plan_reference_against_hand_tables(shape):
    from evennicer_slam_amd.slam import FrameStep, frame_plan
    plan = frame_plan(*shape, 'reference')
    assert plan == [FrameStep(*row) for row in REFERENCE[shape]]
    assert [tuple(s) for s in plan] == REFERENCE[shape]
    s = plan[-1]
    assert (s.rgbd, s.anchor, s.integrate, s.map, s.reset) == REFERENCE[shape][-1]       # the fields by name


@pytest.mark.parametrize('shape', sorted(REFERENCE))
def test_frame_plan_dense_is_todays_plan(shape):
    from evennicer_slam_amd.slam import frame_plan
    n, every, rgbd_every = shape
    want = dense_table(n, every)
    assert [tuple(s) for s in frame_plan(n, every, rgbd_every, 'dense')] == want
    assert [tuple(s) for s in frame_plan(n, every, 1, 'dense')] == want                  # rgbd_every_frame is ignored
    assert [tuple(s) for s in frame_plan(n, every)] == want                              # and 'dense' is the default


def test_frame_plan_refuses_nonsense():
    from evennicer_slam_amd.slam import frame_plan
    with pytest.raises(ValueError):
        frame_plan(5, 2, 2, 'sparse')
    with pytest.raises(ValueError):
        frame_plan(5, 0, 1, 'reference')
    with pytest.raises(ValueError):
        frame_plan(5, 2, 0, 'reference')
    assert frame_plan(0, 2, 2, 'reference') == []


def _cfg(every, **event):
    return {'mapping': {'every_frame': every}, 'event': dict(event)}


def test_schedule_settings_defaults_and_refusals(tmp_path):
    from evennicer_slam_amd.slam import SLAM, schedule_settings
    assert schedule_settings({'mapping': {'every_frame': 5}}) == ('dense', 1, 'measured')
    assert schedule_settings(_cfg(5, rgbd_every_frame=5)) == ('dense', 5, 'measured')     # the key alone changes nothing
    assert schedule_settings(_cfg(10, schedule='reference', rgbd_every_frame=5, depth_on_event_frames='forecast')) == \
        ('reference', 5, 'forecast')
    assert schedule_settings(_cfg(3, schedule='reference', rgbd_every_frame=5)) == ('reference', 5, 'measured')   # rpg.yaml
    assert schedule_settings(_cfg(3, schedule='dense', rgbd_every_frame=5, depth_on_event_frames='none'))[0] == 'dense'
    for mode in ('forecast', 'none'):
        bad = _cfg(3, schedule='reference', rgbd_every_frame=5, depth_on_event_frames=mode)
        with pytest.raises(ValueError) as err:
            schedule_settings(bad)
        assert 'mapping.every_frame' in str(err.value) and 'event.rgbd_every_frame' in str(err.value)
        with pytest.raises(ValueError) as err:                                              # SLAM.__init__, before anything is built
            SLAM(bad, [], str(tmp_path / 'out'), device='cpu')
        assert 'mapping.every_frame' in str(err.value) and 'event.rgbd_every_frame' in str(err.value)
    with pytest.raises(ValueError):
        schedule_settings(_cfg(3, schedule='every_fifth'))
    with pytest.raises(ValueError):
        schedule_settings(_cfg(3, depth_on_event_frames='ground_truth'))


def test_seperate_lr_produces_the_two_rates():
    from evennicer_slam_amd.tracker import camera_learning_rates
    assert camera_learning_rates({'lr': 0.001}) == (0.001, 0.001)
    assert camera_learning_rates({'lr': 0.001, 'seperate_LR': False}) == (0.001, 0.001)
    quat, trans = camera_learning_rates({'lr': 0.001, 'seperate_LR': True})
    assert trans == 0.001 and quat == 0.2 * 0.001                                          # Tracker.py:335-336


def _tool(name):
    import importlib.util
    spec = importlib.util.spec_from_file_location('tool_' + name, os.path.join(ROOT, 'tools', name + '.py'))
    mod = importlib.util.module_from_spec(spec)
    argv = sys.argv
    sys.argv = [name]
    try:
        spec.loader.exec_module(mod)
    finally:
        sys.argv = argv
    return mod


def test_tool_flags_parse():
    import argparse
    R = _tool('run_slam')
    ap = argparse.ArgumentParser()
    R.add_schedule_arguments(ap)
    args = ap.parse_args(['--schedule', 'reference', '--rgbd-every', '5', '--depth-on-event-frames', 'forecast'])
    cfg = R.apply_schedule_arguments({'event': {'schedule': 'dense', 'rgbd_every_frame': 2, 'blur': True}}, args)
    assert cfg['event'] == {'schedule': 'reference', 'rgbd_every_frame': 5, 'depth_on_event_frames': 'forecast', 'blur': True}
    cfg = R.apply_schedule_arguments({'event': {'rgbd_every_frame': 5}}, ap.parse_args([]))
    assert cfg['event'] == {'rgbd_every_frame': 5}                                         # no flag: the configuration stands
    with pytest.raises(SystemExit):
        ap.parse_args(['--schedule', 'sparse'])
    S = _tool('run_synthetic_slam')
    n, kw = S.parse_args(['12', '--events', 'simulate', '--event-predictor', 'model', '--schedule', 'reference', '--rgbd-every', '5',
                          '--depth-on-event-frames', 'none', '--no-events'])
    assert n == 12 and kw['schedule'] == 'reference' and kw['rgbd_every'] == 5 and kw['depth_on_event_frames'] == 'none'
    assert kw['no_events'] is True and kw['events'] == 'simulate' and kw['event_predictor'] == 'model'
    assert S.schedule_overrides({'blur': True}, 'reference', 5, 'forecast') == \
        {'blur': True, 'schedule': 'reference', 'rgbd_every_frame': 5, 'depth_on_event_frames': 'forecast'}
    assert S.schedule_overrides({'schedule': 'reference'}) == {'schedule': 'reference'}
    with pytest.raises(SystemExit):
        S.parse_args(['--depth-on-event-frames', 'gt'])
    n, kw = S.parse_args([])
    assert n == 30 and 'schedule' not in kw and kw['no_events'] is False
