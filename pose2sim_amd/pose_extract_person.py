"""Primary-person extraction: mirror of Pose2Sim/Utilities/pose_extract_person.py.

Walks a camera's OpenPose files, keeps in every frame the one person that follows the previous choice (the closest to it
over the keypoints valid in both; without an earlier choice, or when nobody shares a keypoint with it, the person with the
most confident keypoints) and writes a single-person folder that personAssociation and triangulation take as it is.

    python -m pose2sim_amd.pose_extract_person -i <json folder> [-o <folder>]

The files are parsed in one batch by the native ingest, the selection of every frame of every folder comes from one call of
the HIP engine (Engine.track_select, csrc/p2s_extract.hip: a prefix scan over per-frame transition maps, not a loop over
the frames) and the documents are written by the native writer on host threads, byte for byte json.dump's text: an
all-integer list stays a list of integers, one float makes all of them floats.  There is no NumPy path: without the
library or a GPU it raises.  extract_persons() takes several folders -- a session's cameras -- through the same single call.

Kept from the reference, each recorded in tests/golden/extract_units.npz: the three printed lines and the warning on stderr
for a file json.load cannot decode (written as an empty document, the previous choice kept); any other exception of
open + json.load; TypeError for "people": null, NumPy's reshape ValueError for a list longer than 78 numbers, AttributeError
for a top level or a person that is not an object -- each after the files before it have been written; main() creates the
output folder, process() does not.  No progress bar is drawn.  The rare file that is not a plain list of persons is handed
to Python's own open + json.load and to the reference's statements, so that whatever they raise is raised here.

Outside the reference's contract, refused with ValueError naming the file before anything is written: a keypoint list
holding strings, nulls, booleans or nested values, and an all-integer list with an integer beyond +-2^53 (int64 is the
reference's limit; float64, which carries the numbers here, holds every integer up to 2^53).
"""
import argparse
import json
import os
import sys
import time
from glob import glob

import numpy as np

from . import _lib

N_KPTS = 26
CONF_THRESHOLD = 0.1


def _reference_candidates(path):
    """The reference's own statements on one file, up to the number of candidates: raises what they raise."""
    with open(path) as fp:
        data = json.load(fp)
    n = 0
    for person in data.get('people', []):
        kps = person.get('pose_keypoints_2d', [])
        if len(kps) < N_KPTS * 3:
            continue
        kp = np.array(kps).reshape(N_KPTS, 3)
        n += int(np.sum((kp[:, 2] > CONF_THRESHOLD) & ~np.isnan(kp[:, 0])) >= 1)
    return n


def extract_persons(input_dirs, output_dirs=None, engine=None):
    """process() for several folders at once: one parse, one selection call for all of them, one batch of writes; the
    folders are reported in order.  output_dirs: one per input folder, used as they are; None = '<input>_person', created.
    engine: an Engine (default: Engine(0)).  -> per folder (n_frames, n_empty, n_multi)."""
    from .ingest import JsonBatch, write_person_files
    input_dirs = [os.fspath(d) for d in input_dirs]
    if not input_dirs:
        raise ValueError('no input folder')
    if output_dirs is None:
        output_dirs = [d.rstrip('/') + '_person' for d in input_dirs]
        for d in output_dirs:
            os.makedirs(d, exist_ok=True)
    output_dirs = [os.fspath(d) for d in output_dirs]
    if len(output_dirs) != len(input_dirs):
        raise ValueError('one output folder per input folder is required')
    t_start = time.time()
    folders = []
    for d in input_dirs:
        files = sorted(glob(os.path.join(d, '*.json')))
        if not files:
            raise FileNotFoundError(f'No JSON files found in {d}')
        folders.append(files)
    paths = [f for files in folders for f in files]
    first = np.concatenate([[0], np.cumsum([len(files) for files in folders])])      # [D + 1] every folder's first file
    need = 3 * N_KPTS
    with JsonBatch(paths) as batch:
        counts, base = batch.counts, batch.person_base
        lengths, flags = batch.person_lengths, batch.person_flags()
        file_of = np.repeat(np.arange(len(paths)), np.maximum(counts, 0))
        L = _lib
        refused = ((lengths == L.P2S_JSON_PERSON_NOT_NUMERIC) | ((flags & (L.P2S_JSON_PERSON_HAS_NULL | L.P2S_JSON_PERSON_HAS_BOOL)) != 0)
                   | ((flags & L.P2S_JSON_PERSON_ALL_INTS) != 0) & ((flags & L.P2S_JSON_PERSON_BIG_INT) != 0))
        if refused.any():
            raise ValueError(f'{paths[file_of[np.flatnonzero(refused)[0]]]} holds a keypoint list that is not a list of numbers within +-2^53')
        # files that are not a plain list of persons go through Python, in order, until one of them raises
        odd_person = ((flags & (L.P2S_JSON_PERSON_NOT_OBJECT | L.P2S_JSON_PERSON_BAD_LIST)) != 0) | (lengths > need)
        odd = counts < 0
        odd[file_of[odd_person]] = True
        undecodable, stop, error = [], len(paths), None
        for i in np.flatnonzero(odd).tolist():
            try:
                if _reference_candidates(paths[i]) > 0:
                    raise ValueError(f'{paths[i]} does not hold OpenPose people as the native parser reads them')
            except json.JSONDecodeError:
                undecodable.append(i)
            except Exception as e:
                stop, error = i, e
                break
        D = int(np.searchsorted(first, stop, side='right')) if error is not None else len(folders)   # folders begun
        staged = (lengths == need) & ~odd[file_of] & (file_of < stop)
        rows = np.flatnonzero(staged)
        persons, _ = batch.gather_people(file_of[rows], (rows - base[file_of[rows]]).astype(np.int32), need)
    ints = (flags[rows] & _lib.P2S_JSON_PERSON_ALL_INTS) != 0
    per_file = np.bincount(file_of[rows], minlength=len(paths))
    off = np.concatenate([[0], np.cumsum(per_file)])                                  # [files + 1] first staged person
    if engine is None:
        from .engine import Engine
        engine = Engine(0)
    cameras = [(persons[off[first[d]]:off[first[d + 1]]], off[first[d]:first[d + 1] + 1] - off[first[d]]) for d in range(D)]
    res = engine.track_select(cameras, N_KPTS, CONF_THRESHOLD)
    n_write = min(stop, int(first[D]))
    chosen = np.concatenate(res['chosen'])[:n_write].astype(np.int64)
    n_cand = np.concatenate(res['n_candidates'])[:n_write]
    picked = off[:n_write] + np.maximum(chosen, 0)                                    # a row of `persons` where chosen >= 0
    selecting = chosen >= 0
    kind = np.zeros(n_write, dtype=np.int8)
    kind[selecting] = np.where(ints[picked[selecting]], 2, 1)                         # an int64 array is written back as integers
    values = np.zeros((n_write, need))
    values[selecting] = persons[picked[selecting]].reshape(-1, need)
    out_paths = [os.path.join(output_dirs[d], os.path.basename(f)) for d in range(D) for f in folders[d]][:n_write]
    written = write_person_files(out_paths, values, kind, N_KPTS)
    if not written.all():
        i = int(np.flatnonzero(~written)[0])
        open(out_paths[i], 'w').close()                                               # raises what the reference's open raises
        raise OSError(f'{out_paths[i]} could not be written')
    report = []
    for d in range(D):
        lo, hi = int(first[d]), min(int(first[d + 1]), n_write)
        for i in undecodable:
            if lo <= i < hi:
                print(f'Warning: JSON parse error, skipping: {paths[i]}', file=sys.stderr)
        if error is not None and d == D - 1:
            raise error
        n_frames, n_empty, n_multi = hi - lo, int((chosen[lo:hi] < 0).sum()), int((n_cand[lo:hi] >= 2).sum())
        print(f'Done. {n_frames} frames processed in {time.time() - t_start:.1f}s.')
        print(f'  Empty: {n_empty} ({n_empty/n_frames*100:.1f}%)')
        print(f'  Multi-person: {n_multi} ({n_multi/n_frames*100:.1f}%)')
        report.append((n_frames, n_empty, n_multi))
    return report


def process(input_dir, output_dir, engine=None):
    """Process all JSON files of input_dir: extract the primary person and write to output_dir (which must exist)."""
    extract_persons([input_dir], [output_dir], engine=engine)


def main():
    parser = argparse.ArgumentParser(description='Extract the primary person from multi-person OpenPose JSON files.')
    parser.add_argument('-i', '--input', required=True, help='Input JSON directory')
    parser.add_argument('-o', '--output', default=None, help='Output JSON directory (default: {input}_person)')
    args = parser.parse_args()
    input_dir = args.input
    if not os.path.isdir(input_dir):
        print(f'Error: Input directory not found: {input_dir}', file=sys.stderr)
        sys.exit(1)
    output_dir = input_dir.rstrip('/') + '_person' if args.output is None else args.output
    os.makedirs(output_dir, exist_ok=True)
    process(input_dir, output_dir)


if __name__ == '__main__':
    main()
