"""Host side of pose2sim_amd.trc_gaitevents against the goldens recorded from the reference (tests/golden/gait_units.npz):
the list logic and the report with the recorded frame lists fed in, the arguments, the appended file, the error types the
host decides, and the whole utility with the scipy restatement of the engine (tests/gait_scipy.py) in the GPU's place."""
import json

import numpy as np
import pytest

import gait_scipy as gs
from pose2sim_amd import trc as p2s_trc
from pose2sim_amd import trc_gaitevents as tg

G, CASES = gs.load_golden()
BY_NAME = {c['name']: c for c in CASES}
GOOD = [c['name'] for c in CASES if not c['error']]
BAD = [c['name'] for c in CASES if c['error']]
ERRORS = {'IndexError': IndexError, 'ValueError': ValueError, 'KeyError': KeyError}


def same_result(res, recorded):
    """Equal values AND equal text: the times are floats whose repr is printed."""
    return json.dumps([[list(v) for v in half] for half in res]) == json.dumps(recorded)


def test_goldens_cover_what_they_should():
    assert len(GOOD) >= 40 and len(BAD) >= 15
    assert {BY_NAME[n]['error'] for n in BAD} == set(ERRORS)
    for method in tg.METHODS:
        for motion in ('gait', 'sprint', ''):
            assert any(BY_NAME[n]['args'].get('method') == method and BY_NAME[n]['args'].get('motion_type') == motion for n in GOOD)
    # the cleaning does real work: more events dropped than the four the ends account for
    assert sum(sum(len(a) - len(b) for a, b in zip(BY_NAME[n]['raw_frames'], BY_NAME[n]['result'][1])) > 4 for n in GOOD) >= 3


@pytest.mark.parametrize('name', GOOD)
def test_cleaning_and_report_from_the_recorded_frames(name, tmp_path, capsys):
    case = BY_NAME[name]
    path = gs.write_trial(G, case['trial'], tmp_path)
    cfg = tg.resolve_args(dict(case['args'], trc_path=path, plot=False))
    time_col = p2s_trc.read_trc(path)[2]
    for line in tg._head_lines(cfg):
        print(line)
    res = tg.events_from_frames(cfg, path, time_col, case['raw_frames'])
    assert same_result(res, case['result'])
    assert capsys.readouterr().out == case['console']
    assert open(tmp_path / cfg['output_file']).read() == case['file']


@pytest.mark.parametrize('name', GOOD + BAD)
def test_utility_with_the_scipy_engine(name, tmp_path, capsys):
    case = BY_NAME[name]
    path = gs.write_trial(G, case['trial'], tmp_path)
    args = dict(case['args'], trc_path=path, plot=False, engine=gs.ScipyGaitEngine())
    if case['error']:
        with pytest.raises(ERRORS[case['error']]) as info:
            tg.trc_gaitevents_func(**args)
        assert type(info.value) is ERRORS[case['error']]
        assert not (tmp_path / 'gaitevents.txt').exists()            # no partial file
    else:
        assert same_result(tg.trc_gaitevents_func(**args), case['result'])
        assert open(tmp_path / 'gaitevents.txt').read() == case['file']
    assert capsys.readouterr().out == case['console']


def test_the_output_file_is_appended_to(tmp_path, capsys):
    a, b = BY_NAME['walk_m-forward_coordinates-gait'], BY_NAME['walk_m-height_coordinates-sprint']
    path = gs.write_trial(G, 'walk_m', tmp_path)
    for case in (a, b, a):
        tg.trc_gaitevents_func(trc_path=path, engine=gs.ScipyGaitEngine(), **case['args'])
    assert open(tmp_path / 'gaitevents.txt', 'rb').read() == (a['file'] + b['file'] + a['file']).encode()
    other = tmp_path / 'events.log'
    tg.trc_gaitevents_func(trc_path=path, engine=gs.ScipyGaitEngine(), output_file='events.log', **a['args'])
    assert other.read_text() == a['file']
    tg.trc_gaitevents_func(trc_path=path, engine=gs.ScipyGaitEngine(), output_file='none.log', save_output=False, **a['args'])
    assert not (tmp_path / 'none.log').exists()


def test_batch_reports_in_order_and_raises_at_the_failing_file(tmp_path, capsys):
    ok, bad = BY_NAME['walk_m-height_coordinates-gait'], BY_NAME['short-height_coordinates-sprint']
    first = gs.write_trial(G, 'walk_m', tmp_path, 'a')
    second = gs.write_trial(G, 'short', tmp_path, 'b')
    third = gs.write_trial(G, 'walk_m', tmp_path, 'c')
    args = dict(ok['args'], engine=gs.ScipyGaitEngine())
    with pytest.raises(ValueError):
        tg.trc_gaitevents_batch([first, second, third], **args)
    assert capsys.readouterr().out == ok['console'] + bad['console'].replace('sprint', 'gait')
    assert open(tmp_path / 'gaitevents.txt').read() == ok['file'].replace('walk_m.trc', 'a.trc')
    res = tg.trc_gaitevents_batch([first, third], **args)
    assert len(res) == 2 and all(same_result(r, ok['result']) for r in res)
    assert capsys.readouterr().out == ok['console'] * 2


def test_defaults_and_direction_parsing():
    cfg = tg.resolve_args({'trc_path': 'x.trc'})
    assert cfg == {'trc_path': 'x.trc', 'method': 'height_coordinates', 'gait_direction': (1, 'X'), 'up_direction': (1, 'Y'),
                   'forward_velocity_threshold': 1, 'height_threshold': 6, 'motion_type': 'gait', 'sacrum_marker': 'Hip',
                   'right_heel_marker': 'RHeel', 'right_toe_marker': 'RBigToe', 'left_heel_marker': 'LHeel',
                   'left_toe_marker': 'LBigToe', 'cut_off_frequency': 10, 'plot': True, 'save_output': True,
                   'output_file': 'gaitevents.txt'}
    for text, want in (('X', (1, 'X')), ('-X', (-1, 'X')), ('+Z', (1, 'Z')), ('-Y', (-1, 'Y'))):
        assert tg.resolve_args({'gait_direction': text, 'up_direction': text})['gait_direction'] == want
        assert tg.resolve_args({'gait_direction': text, 'up_direction': text})['up_direction'] == want
    assert tg.resolve_args({'motion_type': ''})['motion_type'] == ''            # '' is a value, not a missing one
    assert tg.resolve_args({'save_output': 'False'})['save_output'] == 'False'  # truthy, as on the reference's command line
    with pytest.raises(ValueError, match='Method must be'):
        tg.resolve_args({'method': 'heights'})
    with pytest.raises(ValueError):
        tg.resolve_args({'gait_direction': 'xX'})                               # int('x1')


def test_command_line_defaults(monkeypatch, tmp_path):
    seen = {}
    monkeypatch.setattr(tg, 'trc_gaitevents_func', lambda **a: seen.update(a))
    monkeypatch.setattr('sys.argv', ['trc_gaitevents', '-i', 'f.trc', '-g=-Z', '-H', '4.5', '--save_output', 'False'])
    tg.main()
    assert seen == {'trc_path': 'f.trc', 'gait_direction': '-Z', 'up_direction': 'Y', 'method': 'height_coordinates',
                    'forward_velocity_threshold': 1, 'height_threshold': 4.5, 'motion_type': 'gait', 'sacrum_marker': 'Hip',
                    'right_heel_marker': 'RHeel', 'right_toe_marker': 'RBigToe', 'left_heel_marker': 'LHeel',
                    'left_toe_marker': 'LBigToe', 'cut_off_frequency': 10, 'plot': True, 'save_output': 'False',
                    'output_file': 'gaitevents.txt'}


def test_alternate_lists_examples():
    a, b = [1, 4, 7, 10], [2, 3, 5, 6, 8, 9]
    assert tg.alternate_lists(a, b, strategy='first') == [[1, 4, 7, 10], [2, 5, 8]]
    assert tg.alternate_lists(a, b, strategy='last') == [[1, 4, 7, 10], [3, 6, 9]]
    assert tg.alternate_lists([5, 6], [1, 2, 7]) == [[6], [7]]                  # what precedes list 0's first value is dropped
    assert tg.alternate_lists([], [1, 2]) == [[], []]
    with pytest.raises(UnboundLocalError):
        tg.alternate_lists([-1.0, 2.0], [0.5], strategy='last')
    assert tg.alternate_lists([-1.0, 2.0], [0.5], strategy='first') == [[2.0], []]


def test_start_end_true_seq_contract():
    assert tg.start_end_true_seq(np.array([4, 9]), np.array([2, 6]), True) == ([4, 9], [2, 6])
    assert tg.start_end_true_seq([], [], False) == ([], [])                     # never below the threshold
    with pytest.raises(IndexError):
        tg.start_end_true_seq([], [], True)                                     # always below it
    # the restatement and the reference's pandas code agree on every pattern of 6 samples
    for bits in range(64):
        sig = np.array([0.0 if bits >> k & 1 else 2.0 for k in range(6)])
        low = sig < 1.0
        edges = np.flatnonzero(low[1:] != low[:-1]) + 1
        on = [int(i) for i in edges if low[i]]
        off = [int(i) - 1 for i in edges if not low[i]]
        if low.all():
            with pytest.raises(IndexError):
                gs.runs_of(sig, 1.0)
            with pytest.raises(IndexError):
                tg.start_end_true_seq(on, off, bool(low[0]))
        else:
            assert tg.start_end_true_seq(on, off, bool(low[0])) == gs.runs_of(sig, 1.0)


def test_without_a_gpu_the_module_raises(tmp_path):
    from pose2sim_amd import _lib
    if _lib.device_count() > 0:
        return                                                                  # the GPU tests cover the other side
    path = gs.write_trial(G, 'walk_m', tmp_path)
    with pytest.raises(_lib.P2sError, match='no HIP device'):
        tg.trc_gaitevents_func(trc_path=path)
    assert not (tmp_path / 'gaitevents.txt').exists()
