"""The timeline kernels on the MI355X, through the C-ABI: Engine.timeline_rows against the NumPy mirror
(tests/timeline_numpy.py) element for element on the smallest shapes at which the scan and the scatter can go wrong, the
utility against the goldens recorded from the reference, and several folders in one call against the host path's bytes.
There is no tolerance: every integer and every copied double must be equal.  Every test prints its figures before it
asserts."""
import os

import numpy as np
import pytest

import timeline_numpy as tn
from pose2sim_amd import confidence_timeline as ct
from test_timeline_host import ALL, gold, run_case, write_folder  # noqa: F401

pytestmark = pytest.mark.gpu

# One call: cameras of 1, 255, 256, 257 and 513 files (one tile of 256, its edge, two tiles and one file), a camera without
# files between two others, lists of at most 1, 2 and 7 entries, each entry valid with probability 1 / 2 (so that entry 0 is
# often invalid where a later one is valid) and one file in ten empty; a camera none of whose entries is valid, and one
# whose files list nobody.
N_FILES = (1, 255, 0, 256, 257, 513, 300, 40)
MOST = (1, 2, 5, 7, 1, 7, 3, 0)
P_VALID = (1.0, 0.5, 0.5, 0.5, 0.5, 0.5, 0.0, 0.5)


@pytest.fixture(scope='module')
def engine():
    from pose2sim_amd.engine import Engine
    return Engine(0)


@pytest.mark.parametrize('K', (1, 4, 26))
def test_rows_and_series_equal_the_mirror(engine, K, capsys):
    case = tn.seeded_case(N_FILES, MOST, K, seed=K, p_valid=P_VALID)
    want = tn.timeline_rows(*case)
    got = engine.timeline_rows(*case)
    again = engine.timeline_rows(*case)
    with capsys.disabled():
        print(f'timeline K = {K}: {len(case[2])} listed persons, {int(case[2].sum())} valid; rows per camera {np.diff(got["row_off"]).tolist()} '
              f'(mirror {np.diff(want["row_off"]).tolist()}); longest lists {got["n_people"].tolist()}; series entries {int(got["series_off"][-1])} '
              f'(mirror {int(want["series_off"][-1])}); kernels {engine.timeline_kernel_ms():.3f} ms')
    first = [case[2][case[1][f]] for f in range(case[0][-1]) if case[1][f + 1] - case[1][f] > 1]
    assert list(want['n_people']) == [m if F else 0 for F, m in zip(N_FILES, MOST)] and not all(first) and want['row_off'][7] == want['row_off'][6]    # what the comment claims
    tn.assert_same(got, want, K)
    for key in tn.OUTPUTS:
        assert got[key].tobytes() == again[key].tobytes(), key        # two runs, the same bytes


def test_single_cameras_at_the_tile_edges(engine, capsys):
    """Every length alone in a call: the camera's offsets start at 0 and the tile count is the camera's own."""
    for F in (1, 255, 256, 257, 513):
        case = tn.seeded_case((F,), (2,), 4, seed=F)
        got, want = engine.timeline_rows(*case), tn.timeline_rows(*case)
        with capsys.disabled():
            print(f'timeline {F} files: {len(got["frame"])} rows (mirror {len(want["frame"])}), series {np.diff(got["series_off"]).tolist()}')
        tn.assert_same(got, want, F)


def test_calls_without_rows(engine):
    for case in (tn.seeded_case((0,), (0,), 2, seed=1), tn.seeded_case((0, 0), (0, 0), 1, seed=2), tn.seeded_case((300, 0, 2), (3, 0, 1), 3, seed=3, p_valid=0.0)):
        got = engine.timeline_rows(*case)
        tn.assert_same(got, tn.timeline_rows(*case))
        assert len(got['frame']) == 0 and not got['row_off'].any() and not got['series_off'].any()


def test_kernel_time_needs_a_call():
    from pose2sim_amd._lib import P2sError
    from pose2sim_amd.engine import Engine
    fresh = Engine(0)
    with pytest.raises(P2sError, match='p2s_timeline_rows_host has not run on this context'):
        fresh.timeline_kernel_ms()
    fresh.timeline_rows(*tn.seeded_case((3,), (2,), 2, seed=4))
    assert fresh.timeline_kernel_ms() >= 0.0


@pytest.mark.parametrize('name', ALL)
def test_utility_on_the_gpu_writes_the_recorded_bytes(gold, engine, tmp_path, name, capsys):   # noqa: F811
    run_case(gold, name, str(tmp_path), engine, capsys)


def test_two_folders_in_one_call_equal_the_host_path(engine, tmp_path, capsys):
    root = str(tmp_path)
    dirs = [write_folder(os.path.join(root, f'cam{c}_json'), 20 + c, n_files=9 + 4 * c, most=4) for c in range(2)]
    names = ['Nose', 'Neck', 'RShoulder', 'LShoulder']
    device = ct.confidence_timelines(dirs, names, [os.path.join(root, f'gpu{c}') for c in range(2)], engine=engine)
    host = ct.confidence_timelines(dirs, names, [os.path.join(root, f'host{c}') for c in range(2)], engine=tn.HostTimelineEngine())
    for c in range(2):
        with open(os.path.join(root, f'gpu{c}', 'confidence_timeline.csv'), 'rb') as a, open(os.path.join(root, f'host{c}', 'confidence_timeline.csv'), 'rb') as b:
            data = a.read()
            with capsys.disabled():
                print(f'folder {c}: {len(data)} bytes of CSV, {len(device[c]["frame"])} rows, series {list(device[c]["series"])[:3]} ...')
            assert data == b.read() and len(device[c]['frame']) > 0
        assert list(device[c]['series']) == list(host[c]['series'])
        for key in host[c]['series']:
            assert tn.same(device[c]['series'][key][0], host[c]['series'][key][0]) and tn.same(device[c]['series'][key][1], host[c]['series'][key][1]), key
