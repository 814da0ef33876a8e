"""The fixture under the association kernels' hard-frame tests (tests/assoc_hard.py), checked on the CPU: the generators
deliver what they claim at every shape the GPU tests use, the oracle is well conditioned on those frames (so that 1e-9 is
a fair bar for a kernel), most of them are still non-binary after 20 passes, and the oracle alone meets the cap on frames
left out of the proposal comparison."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import assoc_hard as ah  # noqa: E402
from oracle import association_ref as ar  # noqa: E402


def _claims(frames, info, Kj, need_blank=True):
    """What every call of hard_frames must hold; -> the detections per frame."""
    kinds = set()
    zero_lik = ghosts = blanks = 0
    for per_cam, tags in zip(frames, info):
        rows = [np.asarray(k).reshape(Kj, 3) for people in per_cam for k in people]
        assert len(rows) == len(tags)
        blank = [bool(np.isnan(k).all()) for k in rows]
        assert blank == [t == 'blank' for t in tags] and sum(blank) <= 1          # never two blank persons in a frame
        blanks += sum(blank)
        ghosts += tags.count('ghost')
        for k in rows:
            nan = np.isnan(k)
            kinds |= {tuple(np.flatnonzero(j)) for j in nan if j.any()}
            zero_lik += int((k[:, 2] == 0).sum())
            assert not (k[:, 2] < 0).any()
        for people in per_cam:                                                      # no identical detections in a camera
            assert not any(np.array_equal(a, b, equal_nan=True) for i, a in enumerate(people) for b in people[:i])
    assert kinds == set(ah.NAN_KINDS), kinds                                        # NaN joints of all four kinds, no other
    assert zero_lik > 0 and ghosts > 0 and (blanks > 0 or not need_blank)
    N = [len(t) for t in info]
    assert any(n % 2 for n in N)                                                    # an odd order
    assert any(n > 0 and sum(len(p) > 0 for p in per_cam) == 1 for n, per_cam in zip(N, frames))   # one camera only
    return N


@pytest.mark.parametrize('Kj', ah.KJ_ALL)
def test_affinity_frames_hold_what_they_claim(Kj):
    """Every call of the affinity test: all four NaN kinds, zero likelihoods, ghosts, a blank person but never two in a
    frame, an odd N, a single-camera frame, N from 1 up to a largest frame inside the call's class."""
    for f64 in ((False, True) if Kj in ah.KJ_F64 else (False,)):
        for k, (C, Pn, lo, hi) in enumerate(ah.SIZE_CLASSES):
            thr = ah.affinity_thr(ah.KJ_ALL.index(Kj), k)
            frames, cams, info = ah.hard_frames_with_info(C, Pn, Kj, ah.AFFINITY_FRAMES, ah.affinity_seed(Kj, k), hi,
                                                          recon_case=ah.RECON_THRS.index(thr), f64=f64, spread=True)
            N = _claims(frames, info, Kj)
            assert lo <= max(N) <= hi and min(N) == 1, (Kj, k, N)
            flat = np.concatenate([k for per_cam in frames for p in per_cam for k in p])
            flat = flat[~np.isnan(flat)]
            assert (flat.astype(np.float32).astype(np.float64) == flat).all() != f64  # on / off the float32 grid


def test_affinity_frames_reach_every_chunk_size():
    """The ray stage takes Kc joints at a time, Kc from N and the padded order: over the calls of the affinity test the
    chunk holds all joints with room to spare, exactly all joints, fewer, and a last chunk of one joint -- in the
    symmetric forms and in the general form."""
    seen = {(form, what): False for form in ('sym16', 'sym32', 'general') for what in ('>', '==', '<', 'last1')}
    for Kj in ah.KJ_ALL:
        for k, (C, Pn, lo, hi) in enumerate(ah.SIZE_CLASSES):
            thr = ah.affinity_thr(ah.KJ_ALL.index(Kj), k)
            _, _, info = ah.hard_frames_with_info(C, Pn, Kj, ah.AFFINITY_FRAMES, ah.affinity_seed(Kj, k), hi,
                                                  recon_case=ah.RECON_THRS.index(thr), spread=True)
            N = [len(t) for t in info]
            n_max = max(2, (max(N) + 1) & ~1)
            for n in N:
                for form, (raw, kc) in zip((('sym16' if n_max <= 16 else 'sym32', 'general') if n_max <= 32 else ('general',)),
                                           _raw_and_clamped(n, n_max, Kj)):
                    seen[form, '>'] |= raw > Kj
                    seen[form, '=='] |= raw == Kj
                    seen[form, '<'] |= raw < Kj
                    seen[form, 'last1'] |= kc < Kj and Kj % kc == 1
    assert all(seen.values()), [k for k, v in seen.items() if not v]


def _raw_and_clamped(N, n_max, Kj):
    out = []
    if n_max <= 32:
        R, L = (16, 8) if n_max <= 16 else (32, 4)
        out.append((R * (R + L // 2) + R * (R + 1) // 2 - R) // (7 * N))
    out.append(3 * n_max * n_max // (7 * N))
    return [(raw, max(1, min(raw, Kj))) for raw in out]


@pytest.mark.parametrize('Kj, C, n_per_cam', [(26, 3, 2), (26, 8, 4), (133, 3, 2), (133, 8, 4)])
def test_one_hot_frames_hold_what_they_claim(Kj, C, n_per_cam):
    """One live joint per frame, no NaN, no identical detections; and the references the GPU test takes (the oracle's
    rays evaluated joint by joint, each distinct joint once) are bit for bit the oracle's plain ones."""
    frames, cams, refs = ah.one_hot_call(Kj, C, n_per_cam)
    assert len(frames) == Kj
    for j, per_cam in enumerate(frames):
        assert [len(p) for p in per_cam] == [n_per_cam] * C
        for people in per_cam:
            for k in people:
                k = k.reshape(Kj, 3)
                assert not np.isnan(k).any()
                assert 0.3 <= k[j, 2] <= 1.0 and (np.delete(k[:, 2], j) == 0).all()
            assert not any(np.array_equal(a, b) for i, a in enumerate(people) for b in people[:i])
    cal = ah.cal_of(cams)
    for f in (range(Kj) if Kj == 26 else (0, 7, 66, 132)):
        cum = ah.cum_of(frames[f])
        assert np.array_equal(refs[f], ar.match_svt(ar.affinity_matrix(frames[f], cal, cum, 0.1), cum, max_iter=0))


@pytest.mark.parametrize('shape', range(len(ah.HARD_SHAPES)))
def test_hard_frames_and_the_oracle_on_them(shape):
    """Per hard shape: the generator's claims; the oracle's sensitivity to a symmetric 1e-12 perturbation of the affinity
    after 0, 1, 3, 5 and 20 passes at most 1e-10 (10 x under the kernels' bar of 1e-9: the frames are well conditioned,
    the bar is fair); at least half of the frames still non-binary after 20 passes (the 20-pass comparison is on
    continuous values); the proposal margin rule leaves out at most 1 frame in 20."""
    C, Pn, Kj, n_cap, thr = ah.HARD_SHAPES[shape]
    frames, cams, info = ah.hard_frames_with_info(C, Pn, Kj, ah.HARD_FRAMES, ah.HARD_SEEDS[shape], n_cap)
    N = _claims(frames, info, Kj)
    assert max(N) <= n_cap and max(N) > (0, 16, 32)[(16, 32, 48).index(n_cap)], N        # the kernel the shape is meant for
    for per_cam in frames:      # at most one detection per frame without a single live joint (it has affinity 1 with all)
        assert sum(bool((np.isnan(k.reshape(Kj, 3)).any(axis=1) | (k[2::3] == 0)).all()) for p in per_cam for k in p) <= 1
    _, _, _, affinity, refs = ah.hard_call(shape, False)
    rng = np.random.default_rng(500 + shape)
    worst = dict.fromkeys((0, 1, 3, 5, 20), 0.0)
    non_binary = left_out = 0
    for per_cam, A, ref in zip(frames, affinity, refs):
        cum = ah.cum_of(per_cam)
        assert not np.isnan(A).any()
        E = rng.normal(0, 1e-12, A.shape)
        E = (E + E.T) / 2
        for it in worst:
            worst[it] = max(worst[it], float(np.abs(ar.match_svt(A + E, cum, max_iter=it) - ref[it][0]).max()))
        X = ref[20][0]
        non_binary += bool(((X > 1e-6) & (X < 1 - 1e-6)).any())
        left_out += not ah.proposals_decided(X, cum)
    print(f'hard shape {ah.HARD_SHAPES[shape]}: N {min(N)}..{max(N)}; oracle sensitivity to 1e-12 after ' +
          ', '.join(f'{it} passes {d:.1e}' for it, d in worst.items()) +
          f'; non-binary after 20 passes {non_binary}/{len(frames)}; left out of the proposal comparison {left_out}/{len(frames)}')
    assert max(worst.values()) <= 1e-10, worst
    assert 2 * non_binary >= len(frames)
    assert 20 * left_out <= len(frames)


def test_the_pass_counter_counts_the_oracles_passes():
    """match_svt_counted returns match_svt's own result, leaves the oracle as it found it, and counts an early break."""
    _, _, _, affinity, refs = ah.hard_call(0, False)
    frames, _ = ah.hard_frames(*ah.HARD_SHAPES[0][:3], ah.HARD_FRAMES, ah.HARD_SEEDS[0], ah.HARD_SHAPES[0][3])
    svt = ar.singular_value_threshold
    for per_cam, A, ref in zip(frames, affinity, refs):
        cum = ah.cum_of(per_cam)
        for it in (0, 3):
            assert np.array_equal(ref[it][0], ar.match_svt(A, cum, max_iter=it)) and ref[it][1] <= it
    assert ar.singular_value_threshold is svt
    cum = np.array([0, 1, 2])
    X, passes = ah.match_svt_counted(np.array([[0.0, 1.0], [1.0, 0.0]]), cum, 20)          # two detections that match
    assert 1 <= passes < 20 and np.array_equal(X, ar.match_svt(np.array([[0.0, 1.0], [1.0, 0.0]]), cum))
