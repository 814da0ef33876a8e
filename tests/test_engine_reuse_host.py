"""No entry point outside the engine-reuse test: every function of include/p2s.h that takes a context is either driven by a
stage of tests/engine_reuse_cases.py -- and so runs on a shared, poisoned engine in tests/test_engine_reuse_gpu.py -- or
stands in the table below with the reason why it takes no staging buffer worth the run.  A stage that is merged without
joining the list fails here, without a GPU."""
import os
import re

from engine_reuse_cases import STAGE_ENTRY

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

EXEMPT = {
    # the context itself: no staging slot, no kernel of a stage
    'p2s_destroy': 'frees the context',
    'p2s_set_stream': 'setter',
    'p2s_synchronize': 'waits for the stream',
    'p2s_set_calibration': 'setter: buffers of its own, owned by the calibration',
    'p2s_set_tuning': 'setter',
    'p2s_get_tri_stats': 'query: counters of their own on the context',
    'p2s_get_assoc_stats': 'query: counters of their own on the context',
    'p2s_timing_begin': 'records an event',
    'p2s_timing_end': 'query: the time between two events',
    # device operands are the caller's; the kernels behind them run through the *_host stages
    'p2s_triangulate_device': '_device: called by p2s_triangulate_host, which every triangulate stage drives',
    'p2s_associate_device': '_device: called by p2s_associate_host',
    'p2s_associate_single_device': '_device: called by p2s_associate_single_host',
    'p2s_track_persons_device': '_device: the kernel of p2s_track_persons_host; its one slot holds the frame offsets, uploaded whole',
    # the last call's kernel time, kept on the host
    **{f'p2s_{stage}_kernel_ms': 'query: *_kernel_ms' for stage in ('reproject', 'jitter', 'confidence', 'id_switch', 'track_select', 'track_persons',
                                                                     'gait', 'measure', 'gaps', 'timeline', 'refine', 'relpose')},
}


def context_entry_points():
    txt = open(os.path.join(ROOT, 'include', 'p2s.h')).read()
    txt = re.sub(r'/\*.*?\*/', '', txt, flags=re.S)
    return sorted(set(re.findall(r'\b(p2s_[a-z_0-9]+)\s*\(\s*p2s_ctx\s*\*(?!\*)', txt)))


def test_every_context_entry_point_has_a_stage_or_a_reason():
    entries = context_entry_points()
    assert len(entries) >= 55 and 'p2s_triangulate_host' in entries and 'p2s_create' not in entries
    staged = set(STAGE_ENTRY.values())
    missing = [e for e in entries if e not in staged and e not in EXEMPT]
    assert missing == [], 'add a stage to tests/engine_reuse_cases.py (or a reason to EXEMPT)'
    assert sorted(staged & set(EXEMPT)) == []                         # a stage is no exemption
    assert sorted((staged | set(EXEMPT)) - set(entries)) == []        # and both tables name what the header declares
    assert all(reason for reason in EXEMPT.values())


def test_the_exempt_table_holds_no_host_entry_point():
    """What takes host arrays stages them: *_host and the three gap entry points are never exempt."""
    host = [e for e in context_entry_points() if e.endswith('_host') or e in ('p2s_interpolate_gaps', 'p2s_fill_gaps', 'p2s_gap_runs')]
    assert len(host) >= 30 and [e for e in host if e in EXEMPT] == []


def test_the_stage_list_is_the_table():
    """stages() builds exactly the stages STAGE_ENTRY names, at both sizes (the inputs are host arrays: no GPU)."""
    from engine_reuse_cases import LARGE, SMALL, stages
    for size in (SMALL, LARGE):
        names = [name for name, _ in stages(size)]
        assert len(names) == len(set(names)) and set(names) == set(STAGE_ENTRY), set(names) ^ set(STAGE_ENTRY)
