"""-m gpu: MultiColSLAM::CreateNewMapPoints<KF, MP> of the C++ facade (include/mcs/mcs_facade.hpp) compiled with g++ and run end to end
(tests/cpp/facade_driver_newpoints.cpp): on one scene of tests/newpoints_model.py it reproduces the Python front end's outputs, which equal the model's."""
import importlib
import os
import subprocess

import numpy as np
import pytest

import newpoints_model as M
import newpoints_pack as P

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class MapPoint:
    def __init__(self, X):
        self.X = np.asarray(X, np.float64)

    def GetWorldPos(self):
        return self.X


def frontend_keyframe(FE, kf):
    """a frontend.cMultiKeyFrame holding the arrays of a model keyframe (no extraction)"""
    models = [FE.cCamModelGeneral_.from_dict(c) for c in kf.cams]
    out = FE.cMultiKeyFrame.__new__(FE.cMultiKeyFrame)
    out.camSystem = FE.cMultiCamSys_(models, M_c=kf.M_c, M_t=kf.M_t)
    out.mvKeys, out.mvKeysRays, out.keypoint_to_cam = kf.keys, kf.rays, kf.cam
    out._d, out._m = kf.desc, kf.desc
    out.mvpMapPoints = [MapPoint(kf.mp_pos[i]) if kf.has_mp[i] else None for i in range(kf.n)]
    return out


def test_cpp_facade_create_new_map_points(tmp_path):
    import gpu_common as G
    FE = importlib.import_module("multicol-slam_amd.frontend")
    exe = tmp_path / "facade_driver_newpoints"
    lib_dir = os.path.join(ROOT, "multicol-slam_amd")
    subprocess.check_call(["g++", "-O1", "-std=c++14", "-Wall", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "facade_driver_newpoints.cpp"), "-o", str(exe), "-L" + lib_dir, "-lmcs_hip", "-Wl,-rpath," + lib_dir])
    kf1, nb = M.make_scene(21, nr_cams=3, n_points=700, n_neigh=6)
    want, v1 = M.create_new_map_points(kf1, nb)
    assert M.scene_conditions(want)["near"] == 0 and M.scene_conditions(want)["accepted"] >= 100
    # the Python front end over keyframe objects
    kfs = [frontend_keyframe(FE, k) for k in [kf1] + nb]
    assert np.array_equal(kfs[0].camSystem.MtMc_inv[1], kf1.MtMc_inv[1])   # the front end's rig arithmetic is the model's
    fe, fv1 = FE.CreateNewMapPoints(kfs[0], kfs[1:], ctx=G.ctx())
    for s, (g, w) in enumerate(zip(fe, want)):
        g = dict(g, acc_x3D=g["x3D"], x3D=g["x3D_all"], median=g["medianDepth"])
        P.compare(g, w, "front end, neighbour %d" % s)
        assert g["median"] == kfs[1 + s].ComputeSceneMedianDepth(2)
    assert np.array_equal(fv1, v1)
    # the C++ facade on the same scene
    fin, fout = tmp_path / "in.bin", tmp_path / "out.bin"
    dim = kf1.desc.shape[1]
    with open(fin, "wb") as f:
        f.write(np.array([kf1.nr, 1 + len(nb), dim], np.int32).tobytes())
        for c in range(kf1.nr):
            f.write(bytes(G.mcs.make_ocam(kf1.cams[c])) + np.asarray(kf1.M_c[c], np.float64).tobytes())
        for k in [kf1] + nb:
            f.write(np.asarray(k.M_t, np.float64).tobytes() + np.array([k.n], np.int32).tobytes())
            f.write(np.ascontiguousarray(k.keys).tobytes() + k.cam.tobytes() + k.rays.tobytes() + k.desc.tobytes())
            f.write(k.has_mp.astype(np.uint8).tobytes() + k.mp_pos.tobytes())
    subprocess.check_call([str(exe), str(fin), str(fout)])
    buf = open(fout, "rb").read()
    off, n1 = 0, kf1.n
    for s, g in enumerate(fe):
        nacc, nm, fb, sk = np.frombuffer(buf, np.int32, 4, off).tolist()
        bl, md = np.frombuffer(buf, np.float64, 2, off + 16)
        off += 32
        m12 = np.frombuffer(buf, np.int32, n1, off)
        vd = np.frombuffer(buf, np.int32, n1, off + 4 * n1)
        off += 8 * n1
        rec = np.frombuffer(buf, np.dtype([("i1", "<i4"), ("i2", "<i4"), ("x", "<f8", 3)]), nacc, off)
        off += 32 * nacc
        assert (nm, fb, bool(sk)) == (g["nmatches"], g["fallbacks"], g["skipped"]), s
        assert P.same_bits([bl, md], [g["baseline"], g["medianDepth"]])
        assert np.array_equal(m12, g["match12"]) and np.array_equal(vd, g["verdict"])
        assert np.array_equal(rec["i1"], g["idx1"]) and np.array_equal(rec["i2"], g["idx2"]) and P.same_bits(rec["x"], g["x3D"])
    assert np.array_equal(np.frombuffer(buf, np.uint8, n1, off).astype(bool), fv1) and off + n1 == len(buf)
