"""A moving and zooming rig for the tests of triangulation with per-frame cameras: synth.make_cameras' ring, every camera
with its own pan, tilt and position drift and a focal length that swings by +-20 % over the frames, the observations
contaminated as synth.make_observations contaminates them, and the calibration as a per-frame TOML (matrix [F][3][3],
rotation and translation [F][3], the layout Utilities/reproj_from_trc_calib.py:86-141 reads).  NumPy only."""
import numpy as np

from pose2sim_amd import cvmath, synth


def _rot_x(a):
    return np.array([[1.0, 0.0, 0.0], [0.0, np.cos(a), -np.sin(a)], [0.0, np.sin(a), np.cos(a)]])


def _rot_y(a):
    return np.array([[np.cos(a), 0.0, np.sin(a)], [0.0, 1.0, 0.0], [-np.sin(a), 0.0, np.cos(a)]])


def make_rig(C, F, seed=0, static=()):
    """-> dict: P [F][C][3][4], K [F][C][3][3], R_mat [F][C][3][3], T [F][C][3], S [C][2], names.  Cameras listed in
    `static` keep frame 0's pose and focal length."""
    cams = synth.make_cameras(C, seed=seed)
    rng = np.random.default_rng(seed + 3000)
    t = np.arange(F) / max(F - 1, 1)
    rig = {'P': np.empty((F, C, 3, 4)), 'K': np.empty((F, C, 3, 3)), 'R_mat': np.empty((F, C, 3, 3)), 'T': np.empty((F, C, 3)),
           'S': np.array(cams['S']), 'names': cams['names'], 'static': tuple(static)}
    for c in range(C):
        R0, K0 = cams['R_mat'][c], cams['K'][c]
        pos0 = -R0.T @ cams['T'][c]
        pan = np.radians(rng.uniform(2.0, 5.0)) * np.sin(2 * np.pi * rng.uniform(0.5, 1.5) * t + rng.uniform(0, 2 * np.pi))
        tilt = np.radians(rng.uniform(1.0, 3.0)) * np.sin(2 * np.pi * rng.uniform(0.5, 1.5) * t + rng.uniform(0, 2 * np.pi))
        drift = rng.uniform(-0.4, 0.4, 3)[None, :] * t[:, None]                      # metres, along a line
        zoom = 1.0 + 0.2 * np.sin(2 * np.pi * t + rng.uniform(0, 2 * np.pi))        # +-20 %
        for f in range(F):
            g = 0 if c in static else f
            R = _rot_x(tilt[g] - tilt[0]) @ _rot_y(pan[g] - pan[0]) @ R0
            K = K0.copy()
            K[0, 0] *= zoom[g]
            K[1, 1] *= zoom[g]
            T = -R @ (pos0 + drift[g])
            rig['K'][f, c], rig['R_mat'][f, c], rig['T'][f, c] = K, R, T
            rig['P'][f, c] = np.hstack([K, np.zeros((3, 1))]) @ np.vstack([np.hstack([R, T.reshape(3, 1)]), [0, 0, 0, 1.0]])
    return rig


def make_observations(Q3d, P, seed=0, dtype=np.float32, noise_px=1.5, p_lowlik=0.05, p_outlier=0.03, p_missing_cam=0.01):
    """synth.make_observations through one projection matrix per (frame, camera): Q3d [F][Pn][K][3], P [F][C][3][4] ->
    xyl [F][Pn][C][K][3]."""
    rng = np.random.default_rng(seed + 2000)
    F, Pn, K, _ = Q3d.shape
    C = P.shape[1]
    xyl = np.empty((F, Pn, C, K, 3), dtype=dtype)
    Xh = np.concatenate([Q3d, np.ones((F, Pn, K, 1))], axis=-1)
    for c in range(C):
        h = np.einsum('fij,fpkj->fpki', P[:, c], Xh)
        uv = h[..., :2] / h[..., 2:3]
        uv = uv + rng.normal(0, noise_px, uv.shape)
        out = rng.random((F, Pn, K)) < p_outlier
        uv = uv + out[..., None] * rng.normal(0, 60.0, uv.shape)
        lik = rng.uniform(0.3, 1.0, (F, Pn, K))
        low = rng.random((F, Pn, K)) < p_lowlik
        lik = np.where(low, rng.uniform(0.0, 0.3, (F, Pn, K)), lik)
        xyl[:, :, c, :, 0] = uv[..., 0]
        xyl[:, :, c, :, 1] = uv[..., 1]
        xyl[:, :, c, :, 2] = lik
        miss = rng.random((F, Pn)) < p_missing_cam
        xyl[:, :, c][miss] = np.nan
    return xyl


def make_workload(F, C, K, Pn=1, seed=0, dtype=np.float32, **contamination):
    """One workload on the moving rig: dict(xyl [F][Pn][C][K][3], P [F][C][3][4], Q3d, rig)."""
    rig = make_rig(C, F, seed=seed)
    Q3d = synth.make_points3d(F, Pn, K, seed=seed)
    return {'xyl': make_observations(Q3d, rig['P'], seed=seed, dtype=dtype, **contamination), 'P': rig['P'], 'Q3d': Q3d, 'rig': rig}


def _rows(a):
    return '[ ' + ', '.join('[ ' + ', '.join(repr(float(v)) for v in row) + ']' for row in a) + ']'


def write_toml(path, rig, frames=None):
    """The rig as a calibration file.  A camera of rig['static'] is written as a static table (frame 0), the others with
    one matrix, rotation and translation per frame; frames = {camera: count} cuts a camera's tables short."""
    F, C = rig['P'].shape[:2]
    with open(path, 'w') as fh:
        for c in range(C):
            n = (frames or {}).get(c, F)
            fh.write(f'[{rig["names"][c]}]\nname = "{rig["names"][c]}"\n')
            fh.write(f'size = [ {float(rig["S"][c][0])!r}, {float(rig["S"][c][1])!r}]\n')
            if c in rig['static']:
                fh.write(f'matrix = {_rows(rig["K"][0, c])}\n')
                fh.write('distortions = [ 0.0, 0.0, 0.0, 0.0]\n')
                fh.write(f'rotation = {_rows([cvmath.rodrigues_inv(rig["R_mat"][0, c])])[2:-1]}\n')
                fh.write(f'translation = {_rows([rig["T"][0, c]])[2:-1]}\n')
            else:
                fh.write('matrix = [ ' + ', '.join(_rows(rig['K'][f, c]) for f in range(n)) + ']\n')
                fh.write('distortions = [ 0.0, 0.0, 0.0, 0.0]\n')
                fh.write(f'rotation = {_rows([cvmath.rodrigues_inv(rig["R_mat"][f, c]) for f in range(n)])}\n')
                fh.write(f'translation = {_rows(rig["T"][:n, c])}\n')
            fh.write('fisheye = false\n\n')
        fh.write('[metadata]\nadjusted = false\nerror = 0.0\n')
