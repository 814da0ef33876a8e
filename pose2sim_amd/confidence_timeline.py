"""Keypoint confidence timeline: mirror of Pose2Sim/Utilities/confidence_timeline.py.

One row per (frame, listed person, keypoint) with the detector's confidence, written as confidence_timeline.csv, and the
same confidences grouped per (keypoint, person) -- what the reference scatter-plots against the frame number.  Where
pose_confidence_analyze says how often a keypoint's confidence is low, this says when, and for which listed person.

The JSON files of all folders are parsed in one batch by the native ingest (JsonBatch) and the confidences of the
resolved keypoints gathered there; the rows, their order and the series come from one call of the HIP engine for all
folders (Engine.timeline_rows, csrc/p2s_timeline.hip), and the CSV from the native writer (engine.write_timeline_csv):
csv.writer's bytes, repr() floats.  There is no NumPy path and no second writer.

Kept from the reference, each recorded in tests/golden/timeline_units.npz: files are sorted(glob('*.json')), an empty
folder raises FileNotFoundError before the names are looked at; an unknown name raises ValueError with the sorted list of
names before the output folder exists; a name given twice yields its rows once, where it first stood, while the
'Keypoints:' line prints the names as given; the frame is the file's position in the listing, and a file that does not
decode as JSON is skipped with a warning on stderr while the files after it keep their positions; the person is the
position in the file's 'people' list, every entry counted; an entry without 'pose_keypoints_2d', or with fewer than 78
numbers, yields no rows; a longer list is cut to 26 keypoints; a file without 'people' holds nobody; 'people': null
raises TypeError and a top level that is no object AttributeError, after the folder was made and the first lines
printed.  The PNG is not drawn and its line not printed: the series it is drawn from are in the returned dictionary.
`thresholds` only draws lines on that plot: it is accepted and ignored.

Outside what the native parser tells apart, refused with ValueError naming the file before anything is written: a file
that cannot be read at all (or is not UTF-8), a 'people' value that is neither a list nor null, a person that is not an
object, a 'pose_keypoints_2d' that is not a list, a keypoint list holding anything but numbers.
"""
import argparse
import os
import sys
import time
from glob import glob

import numpy as np

from . import _lib
from .keypoint_jitter_analyze import KEYPOINT_NAMES

HALPE_26_INDICES = {name: i for i, name in enumerate(KEYPOINT_NAMES)}     # the reference's table: HALPE_26 in JSON order
N_KEYPOINTS = 26
DEFAULT_KEYPOINTS = 'Nose,Neck,RShoulder,LShoulder'
GATHER_ROWS = 1 << 16                            # persons per gather call: bounds the [rows][78] table it returns


class _Folder:
    """What one folder brings to the engine call, and what the report needs once the rows are back."""

    def __init__(self, json_dir, keypoint_names):
        self.json_dir = json_dir
        self.names_given = list(keypoint_names)
        self.files = sorted(glob(os.path.join(json_dir, '*.json')))
        if not self.files:
            raise FileNotFoundError(f'No JSON files found in {json_dir}')
        target = {}
        for name in keypoint_names:
            if name not in HALPE_26_INDICES:
                available = ', '.join(sorted(HALPE_26_INDICES.keys()))
                raise ValueError(f'Unknown keypoint: {name}. Available: {available}')
            target[name] = HALPE_26_INDICES[name]
        if not target:
            raise ValueError('at least one keypoint name is required')
        self.names, self.index = list(target), np.fromiter(target.values(), dtype=np.int64)
        self.skipped, self.error, self.n_files = [], None, len(self.files)


def _refuse(path, what):
    raise ValueError(f'{path} {what}')


def _screen(folders, batch):
    """What the parsed files hold beyond persons with lists of numbers: refuses what the parser cannot tell apart, notes
    the files the reference skips and the first file of every folder it raises on (only the files before it count).
    -> valid [N]: the person's list holds at least 78 numbers."""
    counts, lengths = batch.counts, batch.person_lengths
    flags = batch.person_flags() if len(lengths) else np.zeros(0, dtype=np.int32)
    kinds = batch.person_ids()[1] if (counts == _lib.P2S_JSON_NO_PEOPLE_LIST).any() else None
    paths = [f for fd in folders for f in fd.files]
    for i in np.flatnonzero(counts == _lib.P2S_JSON_UNREADABLE):
        try:
            with open(paths[i]) as fh:
                fh.read()
        except (OSError, UnicodeDecodeError):
            _refuse(paths[i], 'cannot be read')
    if kinds is not None:
        for i in np.flatnonzero(kinds == _lib.P2S_JSON_DOC_PEOPLE_OTHER):
            _refuse(paths[i], "does not hold a 'people' list")
    long_enough = lengths >= 3 * N_KEYPOINTS
    bad = ((flags & (_lib.P2S_JSON_PERSON_NOT_OBJECT | _lib.P2S_JSON_PERSON_BAD_LIST)) != 0) | (lengths == _lib.P2S_JSON_PERSON_NOT_NUMERIC) \
        | (long_enough & ((flags & (_lib.P2S_JSON_PERSON_HAS_NULL | _lib.P2S_JSON_PERSON_HAS_BOOL)) != 0))
    if bad.any():
        i = int(np.searchsorted(batch.person_base, np.flatnonzero(bad)[0], side='right')) - 1
        _refuse(paths[i], 'does not hold OpenPose people with lists of numbers')
    first = 0
    for fd in folders:
        for j in range(fd.n_files):
            i = first + j
            if counts[i] == _lib.P2S_JSON_UNREADABLE:
                fd.skipped.append(j)
            elif counts[i] == _lib.P2S_JSON_NO_PEOPLE_LIST and kinds[i] != _lib.P2S_JSON_DOC_NO_PEOPLE_KEY:
                fd.error = (TypeError("'NoneType' object is not iterable") if kinds[i] == _lib.P2S_JSON_DOC_PEOPLE_NULL else
                            AttributeError(f"'{_lib.P2S_JSON_DOC_TYPES[int(kinds[i])]}' object has no attribute 'get'"))
                fd.n_files = j                                        # the reference stops here
                break
        first += len(fd.files)
    return long_enough


def _gather(batch, valid, index):
    """-> conf [N][K]: the confidences of the keypoints `index` of every valid person; rows of the others stay 0."""
    conf = np.zeros((len(valid), len(index)))
    rows = np.flatnonzero(valid)
    file_of = np.searchsorted(batch.person_base, rows, side='right') - 1
    person_of = (rows - batch.person_base[file_of]).astype(np.int32)
    for a in range(0, len(rows), GATHER_ROWS):
        values, _ = batch.gather_people(file_of[a:a + GATHER_ROWS], person_of[a:a + GATHER_ROWS], 3 * N_KEYPOINTS)
        conf[rows[a:a + GATHER_ROWS]] = values[:, 3 * index + 2]
    return conf


def _series(names, res, c):
    """The reference's `grouped` of camera c: {(name, person): (frames, confidences)}, keys in the order of their first row."""
    people_off = np.concatenate([[0], np.cumsum(res['n_people'])])
    off, frames = res['series_off'], res['series_frame']
    present = [(int(frames[off[q]]), q) for q in range(int(people_off[c]), int(people_off[c + 1])) if off[q + 1] > off[q]]
    out = {}
    for _, q in sorted(present):
        for k, name in enumerate(names):
            out[(name, q - int(people_off[c]))] = (frames[off[q]:off[q + 1]], res['series_conf'][k, off[q]:off[q + 1]])
    return out


def confidence_timelines(json_dirs, keypoint_names, output_dirs=None, engine=None):
    """process() for several camera folders with one parse and one engine call.  output_dirs: one folder per entry of
    json_dirs, or None: nothing is written or printed, the data is returned.  -> a list of process()'s dictionaries.
    engine: an Engine (default: Engine(0))."""
    from .engine import write_timeline_csv
    from .ingest import JsonBatch
    t_start = time.time()
    json_dirs = list(json_dirs)
    if output_dirs is not None and len(output_dirs) != len(json_dirs):
        raise ValueError('one output folder per input folder is required')
    folders = [_Folder(d, keypoint_names) for d in json_dirs]
    if not folders:
        return []
    names, index = folders[0].names, folders[0].index
    with JsonBatch([f for fd in folders for f in fd.files]) as batch:
        valid = _screen(folders, batch)
        person_base = batch.person_base.copy()
        first = 0
        for fd in folders:                                            # the files from a folder's raising one on hold nobody
            lo, hi = person_base[first + fd.n_files], person_base[first + len(fd.files)]
            valid[lo:hi] = False
            first += len(fd.files)
        conf = _gather(batch, valid, index)
    if engine is None:
        from .engine import Engine
        engine = Engine(0)
    file_off = np.concatenate([[0], np.cumsum([len(fd.files) for fd in folders])])
    res = engine.timeline_rows(file_off, person_base, valid, conf)
    out = []
    for c, fd in enumerate(folders):
        output_dir = None if output_dirs is None else output_dirs[c]
        if output_dir is not None:
            os.makedirs(output_dir, exist_ok=True)
            print(f'JSON files: {len(fd.files)}')
            print(f'Keypoints: {", ".join(fd.names_given)}')
            print(f'Output: {output_dir}')
        for j in fd.skipped:
            if j < fd.n_files:
                print(f'Warning: JSON parse error, skipping: {fd.files[j]}', file=sys.stderr)
        if fd.error is not None:
            raise fd.error
        a, b = res['row_off'][c], res['row_off'][c + 1]
        data = {'frame': res['frame'][a:b], 'person': res['person'][a:b], 'keypoint': res['slot'][a:b], 'confidence': res['confidence'][a:b],
                'names': list(names), 'series': _series(names, res, c)}
        if output_dir is not None:
            csv_path = os.path.join(output_dir, 'confidence_timeline.csv')
            write_timeline_csv(csv_path, data['frame'], data['person'], data['keypoint'], data['confidence'], names)
            print(f'Done. {len(fd.files)} frames, {b - a} data points in {time.time() - t_start:.1f}s.')
            print(f'  CSV: {csv_path}')
        out.append(data)
    return out


def process(json_dir, keypoint_names, output_dir, thresholds, engine=None):
    """The reference's process(): confidence_timeline.csv in output_dir, the reference's lines printed (without the PNG's).
    thresholds is accepted and ignored: it only draws lines on the plot.  -> what the reference plots: {'frame', 'person',
    'keypoint', 'confidence': the CSV's columns as arrays, 'keypoint' as an index into 'names'; 'names': the resolved
    keypoint names; 'series': {(name, person): (frames, confidences)}, the reference's `grouped`}."""
    return confidence_timelines([json_dir], keypoint_names, [output_dir], engine=engine)[0]


def main():
    '''CLI entry point.'''
    parser = argparse.ArgumentParser(
        description='Plot keypoint confidence timeline from JSON files.')
    parser.add_argument('-j', '--json_dir', required=True,
                        help='Input JSON directory')
    parser.add_argument('-k', '--keypoints', default=DEFAULT_KEYPOINTS,
                        help=f'Keypoint names, comma-separated (default: {DEFAULT_KEYPOINTS})')
    parser.add_argument('-o', '--output', default=None,
                        help='Output directory (default: {json_dir}_conf_timeline)')
    parser.add_argument('-t', '--threshold', default=None,
                        help='Threshold lines, comma-separated (e.g., 0.3,0.5). Default: none; accepted, no plot is drawn')
    args = parser.parse_args()

    json_dir = args.json_dir
    if not os.path.isdir(json_dir):
        print(f'Error: Input directory not found: {json_dir}', file=sys.stderr)
        sys.exit(1)

    keypoint_names = [k.strip() for k in args.keypoints.split(',')]
    output_dir = json_dir.rstrip('/') + '_conf_timeline' if args.output is None else args.output

    thresholds = None
    if args.threshold:
        try:
            thresholds = [float(t.strip()) for t in args.threshold.split(',')]
        except ValueError:
            print(f'Error: Invalid threshold value: {args.threshold}', file=sys.stderr)
            sys.exit(1)

    process(json_dir, keypoint_names, output_dir, thresholds)


if __name__ == '__main__':
    main()
