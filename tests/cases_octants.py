"""
The RPC chain in every octant of the globe: placements and helpers shared by the host test (test_octants_cases_host.py), which
pins the construction on the CPU oracle, and the GPU tests (test_gpu_octants.py), which hold the device to the oracle in the moved
frames.

Both shipped RPCs sit at LAT_OFF 11.02 N, LONG_OFF -72.71: every ECEF point they see has x > 0, y < 0, z > 0 and |y| > |x|.  The
chain has two exact symmetries.  For an RPC r, a longitude shift dlon and a flag mirror, the moved RPC has lon_offset + dlon and,
if mirror, -lat_offset and the coefficients of the monomials odd in P negated (the normalised latitude changes sign and every
monomial keeps its value).  The moved points are the original ones rotated about Z by dlon, z negated if mirror: they have the
longitude lon + dlon and the latitude -lat, so the moved RPC projects them to the same pixels.  dlon is a multiple of 90 degrees:
the rotation is a signed permutation of x and y and the moved points are exact.
"""
import os

import numpy as np

from satba import synth
from satba.rpc_model import RPCModel

# (dlon [deg], mirror), the original first: LONG_OFF -72.7, 17.3, 107.3, -162.7 and LAT_OFF +-11.02
PLACEMENTS = [(0.0, False), (90.0, False), (180.0, False), (-90.0, False), (0.0, True), (90.0, True), (180.0, True), (-90.0, True)]
ORIGINAL = PLACEMENTS[0]
# what a placement promises of every point of its scenes: sign of x, sign of y, |y| > |x| per longitude shift (cos and sin of
# -72.7, 17.3, 107.3 and -162.7 degrees); the sign of z is -1 if mirror
LON_SIGNS = {0.0: (1, -1, True), 90.0: (1, 1, False), 180.0: (-1, 1, True), -90.0: (-1, -1, False)}
# RPC00B order of satba/rpc_model.py: P, LP, PH, PLH, L2P, P3, PH2
ODD_IN_P = (2, 4, 6, 10, 14, 15, 16)
MARGIN = 20.0  # as cases_camapprox.MARGIN: room for another libm

# Distances of the oracle to itself between the original and a moved frame, the largest over the eight placements on the pinned
# seed (test_octants_cases_host.py prints them per placement); the host test asserts MARGIN x these.
# Measured per longitude shift 0 / +90 / +180 / -90 (the mirror changes none of them but the localisation: its signs round alike).
PROJ_CHAIN_PX = 6.642e-9  # (c) the two oracle Jacobian functions, moved RPC at moved points against the original: 0 / 2.213e-9 / 2.215e-9 / 6.642e-9 px
PROJ_BA_PX = 6.584e-9     # (c) ba_oracle.project_rpc in float64, the same: 0 / 2.215e-9 / 4.429e-9 / 6.584e-9 px
JAC_REL = 1.042e-14       # (d) D @ G taken back through the move, relative to its largest entry: 0 / 3.498e-15 / 3.537e-15 / 1.042e-14
FUN_PX = 8.774e-9         # (e) ba_oracle.fun in float64 on the moved 4-camera scene, R and R + T: 0 / 3.318e-9 / 4.429e-9 / 8.774e-9 px
# (f) T._Rpc(moved).eval_rpc against the moved angles.  Not mirrored 0 / 7.1e-15 / 0 / 2.8e-14 deg in longitude and 0 in latitude;
# mirrored 1.027e-11 deg and 2.435e-12 deg at every shift (the iteration starts at -delta in the normalised latitude, which the
# mirror turns into +delta: another path to the same root, stopped by the same threshold)
LOC_LON_DEG = 1.027e-11
LOC_LAT_DEG = 2.435e-12


def placement_id(placement):
    return "lon{:+d}{}".format(int(placement[0]), "_south" if placement[1] else "_north")


def promised_signs(placement):
    """(sign of x, sign of y, sign of z, |y| > |x|)"""
    sx, sy, steep = LON_SIGNS[placement[0]]
    return sx, sy, -1 if placement[1] else 1, steep


def frame(dlon, mirror):
    """M (3, 3) with X' = M X: the rotation about Z by dlon, a multiple of 90 degrees (entries 0 and +-1), then z -> -z if mirror"""
    k = int(round(dlon / 90.0))
    assert k * 90.0 == dlon, dlon
    c, s = ((1.0, 0.0), (0.0, 1.0), (-1.0, 0.0), (0.0, -1.0))[k % 4]
    return np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, -1.0 if mirror else 1.0]])


def moved_points(X, dlon, mirror):
    return np.asarray(X, dtype=np.float64) @ frame(dlon, mirror).T


def original_points(X, dlon, mirror):
    """inverse of moved_points"""
    return np.asarray(X, dtype=np.float64) @ frame(dlon, mirror)


def original_jacobian(J, dlon, mirror):
    """d(.)/dX of the original frame from d(.)/dX' (..., 3) of the moved frame"""
    return np.asarray(J, dtype=np.float64) @ frame(dlon, mirror)


def moved_rpc(r, dlon, mirror):
    m = r.copy()
    m.lon_offset = r.lon_offset + dlon
    if mirror:
        m.lat_offset = -r.lat_offset
        for attr in ("row_num", "row_den", "col_num", "col_den"):
            c = list(getattr(r, attr))
            for k in ODD_IN_P:
                c[k] = -c[k]
            setattr(m, attr, c)
    return m


def rpcs(dlon, mirror):
    """the two shipped RPCs, moved"""
    return [moved_rpc(RPCModel.from_file(f), dlon, mirror) for f in synth.default_rpc_files()]


def moved_files(tmp_dir, dlon, mirror):
    """writes the two shipped RPCs, moved, into tmp_dir; the paths in the order of synth.default_rpc_files()"""
    out = []
    for f, r in zip(synth.default_rpc_files(), rpcs(dlon, mirror)):
        out.append(os.path.join(str(tmp_dir), os.path.basename(f)))
        r.write_to_file(out[-1])
    return out


def scene(placement, tmp_dir, n_cam, n_pts, opp, seed, **kw):
    """a scene drawn in the placement's own frame, around the moved RPC files"""
    return synth.make_rpc_scene(n_cam, n_pts, opp, seed=seed, rpc_files=moved_files(tmp_dir, *placement), **kw)


def moved_scene(scene0, dlon, mirror):
    """scene0, drawn in the original frame, taken to a placement: the same random draws, the same observations"""
    d = dict(scene0.__dict__)
    d["cameras"] = [moved_rpc(r, dlon, mirror) for r in scene0.cameras]
    d["cameras_true"] = d["cameras"]
    d["pts3d"], d["pts3d_true"] = moved_points(scene0.pts3d, dlon, mirror), moved_points(scene0.pts3d_true, dlon, mirror)
    d["camera_centers"] = [moved_points(c, dlon, mirror) for c in scene0.camera_centers]
    return synth.Scene(**d)


def moved_variables(v, n_cam, n_params, dlon, mirror):
    """the variable vector [cameras (n_cam, n_params = 3 or 6: Euler angles, T), points] in the moved frame.  Only corrections that
    turn about Z map onto Euler angles again (R = Rz Ry Rx commutes with the move when the first two angles are zero)"""
    v = np.array(v, dtype=np.float64)
    cam = v[: n_cam * n_params].reshape(n_cam, n_params)
    assert not cam[:, :2].any()
    if n_params == 6:
        cam[:, 3:6] = moved_points(cam[:, 3:6], dlon, mirror)
    v[n_cam * n_params:] = moved_points(v[n_cam * n_params:].reshape(-1, 3), dlon, mirror).ravel()
    return v
