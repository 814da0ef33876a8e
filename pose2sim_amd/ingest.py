"""Batch OpenPose-JSON ingest through the native parser (csrc/p2s_ingest.cpp, include/p2s.h).

One parse of every file of a trial on host threads instead of the reference's json.load per (frame,
camera, person) (triangulation.py:607-653, :77-90; personAssociation.py:260-274).  The numbers are the
ones Python's float() would produce (correctly rounded), a file is unreadable exactly when json.load
would raise.
"""
import ctypes as C

import numpy as np

from . import _lib
from .engine import _entry
from ._lib import (P2S_F32, P2S_F64, P2S_JSON_NO_PEOPLE_LIST, P2S_JSON_PERSON_NO_LIST,  # noqa: F401
                   P2S_JSON_PERSON_NOT_NUMERIC, P2S_JSON_UNREADABLE)


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None and a.size else None


class JsonBatch:
    """Parsed files; paths[i] = '' or None means "no file for this slot" (reads as unreadable)."""

    def __init__(self, paths, n_threads=0):
        self._lib = _lib.load()
        enc = [(p or '').encode() if not isinstance(p, bytes) else p for p in paths]
        self.n_files = len(enc)
        offsets = np.zeros(self.n_files + 1, dtype=np.int64)
        if enc:
            np.cumsum(np.fromiter((len(e) for e in enc), dtype=np.int64, count=len(enc)), out=offsets[1:])
        blob = b''.join(enc)
        h = C.c_void_p()
        _lib.check(self._lib.p2s_json_parse(blob, _ptr(offsets), self.n_files, int(n_threads), C.byref(h)))
        self._h = h
        self.counts = np.zeros(self.n_files, dtype=np.int32)
        self.person_base = np.zeros(self.n_files + 1, dtype=np.int64)
        _lib.check(self._lib.p2s_json_people_counts(self._h, _ptr(self.counts), self.person_base.ctypes.data_as(C.c_void_p)))
        self._lengths = None

    def close(self):
        if getattr(self, '_h', None):
            self._lib.p2s_json_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    @property
    def person_lengths(self):
        """Per person (file-major): len(pose_keypoints_2d) or a P2S_JSON_PERSON_* code."""
        if self._lengths is None:
            self._lengths = np.zeros(int(self.person_base[-1]), dtype=np.int32)
            if self._lengths.size:
                _lib.check(self._lib.p2s_json_person_lengths(self._h, _ptr(self._lengths)))
        return self._lengths

    def person_flags(self):
        """Per person (file-major): _lib.P2S_JSON_PERSON_* bits -- every number of the list an integer token, a null, a
        boolean, an integer beyond +-2^53, the person not an object, the list not an array (p2s_json_person_flags)."""
        fn = _entry(self._lib, 'p2s_json_person_flags')
        flags = np.zeros(int(self.person_base[-1]), dtype=np.int32)
        if flags.size:
            _lib.check(fn(self._h, _ptr(flags)))
        return flags

    def person_ids(self):
        """-> (ids, file_kind): ids, per person (file-major), the raw JSON text of its "person_id" value as bytes, None for
        a person without the key; file_kind [n_files] P2S_JSON_DOC_*: what `counts` does not tell apart about a file without
        a person list (see p2s_json_person_ids)."""
        fn = _entry(self._lib, 'p2s_json_person_ids')
        offsets = np.zeros(int(self.person_base[-1]) + 1, dtype=np.int64)
        kinds = np.zeros(self.n_files, dtype=np.int32)
        _lib.check(fn(self._h, _ptr(offsets), None, 0, _ptr(kinds)))
        text = C.create_string_buffer(max(int(offsets[-1]), 1))
        _lib.check(fn(self._h, _ptr(offsets), text, int(offsets[-1]), None))
        raw = text.raw
        return [raw[a:b] if b > a else None for a, b in zip(offsets[:-1].tolist(), offsets[1:].tolist())], kinds

    def gather_keypoints(self, keypoint_ids, max_persons, file_offsets, person_stride, out):
        """out: preallocated float32 / float64 array; see p2s_json_gather_keypoints.  -> n_inexact."""
        ids = np.ascontiguousarray(keypoint_ids, dtype=np.int32)
        file_offsets = np.ascontiguousarray(file_offsets, dtype=np.int64)
        if file_offsets.shape != (self.n_files,):
            raise ValueError('one offset per parsed file is required')
        dtype = P2S_F32 if out.dtype == np.float32 else P2S_F64
        if out.dtype not in (np.float32, np.float64) or not out.flags.c_contiguous:
            raise ValueError('out must be a C-contiguous float32 / float64 array')
        top = int(file_offsets.max(initial=-1))
        if top >= 0 and top + (max_persons - 1) * person_stride + 3 * len(ids) > out.size:
            raise ValueError('offsets reach beyond the output array')
        bad = C.c_int64(0)
        _lib.check(self._lib.p2s_json_gather_keypoints(self._h, _ptr(ids), len(ids), int(max_persons),
                                                       file_offsets.ctypes.data_as(C.c_void_p), int(person_stride), dtype,
                                                       out.ctypes.data_as(C.c_void_p), C.byref(bad)))
        return bad.value

    def gather_people(self, file_index, person_index, n_values, dtype=np.float64):
        file_index = np.ascontiguousarray(file_index, dtype=np.int64)
        person_index = np.ascontiguousarray(person_index, dtype=np.int32)
        out = np.empty((len(file_index), int(n_values)), dtype=dtype)
        bad = C.c_int64(0)
        _lib.check(self._lib.p2s_json_gather_people(self._h, _ptr(file_index), _ptr(person_index), len(file_index),
                                                    int(n_values), P2S_F32 if out.dtype == np.float32 else P2S_F64,
                                                    _ptr(out), C.byref(bad)))
        return out, bad.value

    def gather_largest_person(self, keypoint_ids, likelihood_threshold):
        """convert_json2pandas (synchronization.py:1185-1250) for every file: (x, y, likelihood) [n_files][n_ids][3] of
        the person with the largest bounding box, NaN below the threshold or where the reference's try block raises."""
        ids = np.ascontiguousarray(keypoint_ids, dtype=np.int32)
        out = np.empty((self.n_files, len(ids), 3), dtype=np.float64)
        _lib.check(self._lib.p2s_json_gather_largest_person(self._h, _ptr(ids), len(ids), float(likelihood_threshold),
                                                            _ptr(out)))
        return out

    def select_tracked_person(self, n_kpts=26, conf_threshold=0.1):
        """load_keypoints_series / _select_person (Utilities/keypoint_jitter_analyze.py:50-140) over the files in order:
        -> (series [n_files][n_kpts][3], status [n_files] P2S_TRACK_*, detail [n_files]); see p2s_json_select_tracked_person."""
        fn = _entry(self._lib, 'p2s_json_select_tracked_person')
        out = np.empty((self.n_files, int(n_kpts), 3), dtype=np.float64)
        status = np.zeros(self.n_files, dtype=np.int32)
        detail = np.zeros(self.n_files, dtype=np.int32)
        _lib.check(fn(self._h, int(n_kpts), float(conf_threshold), _ptr(out), _ptr(status), _ptr(detail)))
        return out, status, detail


def copy_files(pairs, n_threads=0):
    """shutil.copy(src, dst) for every (src, dst) pair on host threads (p2s_copy_files); raises OSError on a failure."""
    lib = _lib.load()
    enc_s = [s.encode() for s, _ in pairs]
    enc_d = [d.encode() for _, d in pairs]
    off_s = np.zeros(len(pairs) + 1, dtype=np.int64); off_d = np.zeros(len(pairs) + 1, dtype=np.int64)
    if pairs:
        np.cumsum([len(e) for e in enc_s], out=off_s[1:]); np.cumsum([len(e) for e in enc_d], out=off_d[1:])
    rc = lib.p2s_copy_files(b''.join(enc_s), off_s.ctypes.data_as(C.c_void_p), b''.join(enc_d), off_d.ctypes.data_as(C.c_void_p),
                            len(pairs), int(n_threads), None)
    if rc != 0:
        raise OSError(lib.p2s_last_error().decode())


def write_person_files(paths, values, kind, n_kpts=26, n_threads=0):
    """The single-person documents of Utilities/pose_extract_person.py, byte for byte json.dump's text, on host threads
    (p2s_write_person_files): kind[i] 0 = no person, 1 = values[i] ([3 * n_kpts]) as repr() floats, 2 = as integers.
    -> written [n_files] bool: False where the file could not be created or written."""
    lib = _lib.load()
    fn = _entry(lib, 'p2s_write_person_files')
    enc = [p.encode() if not isinstance(p, bytes) else p for p in paths]
    off = np.zeros(len(enc) + 1, dtype=np.int64)
    if enc:
        np.cumsum([len(e) for e in enc], out=off[1:])
    values = np.ascontiguousarray(values, dtype=np.float64).reshape(len(enc), 3 * int(n_kpts))
    kind = np.ascontiguousarray(kind, dtype=np.int8).reshape(len(enc))
    written = np.zeros(len(enc), dtype=np.int8)
    _lib.check(fn(b''.join(enc), off.ctypes.data_as(C.c_void_p), len(enc), _ptr(values), _ptr(kind), int(n_kpts), int(n_threads), _ptr(written)))
    return written.astype(bool)
