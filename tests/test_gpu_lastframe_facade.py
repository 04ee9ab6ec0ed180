"""-m gpu: the frame-to-frame searches above the C ABI — frontend.TrackWithMotionModelSearch / TrackPreviousFrameWindowSearch (host and device kind) and
MultiColSLAM::SearchByProjectionLastFrame<FR, MP> / WindowSearchFrames<FR, MP> of the C++ facade compiled with g++ (tests/cpp/facade_driver_lastframe.cpp) —
against the oracle on the pairs of tests/lastframe_scene.py: return value and the map point every feature of the searched frame holds afterwards."""
import importlib
import os
import subprocess

import numpy as np
import pytest

import lastframe_scene as LS

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FM = LS.FM
INT_MAX = 2**31 - 1


def rig_motion(nr):
    """M_c / M_t behind frustum_model.make_rig(cams, 1)"""
    M_t = FM.small_motion(0.2, -0.3, 0.1, [0.01, 0.0, 0.02])
    M_c = []
    for c in range(nr):
        Mc = FM.rot_y(360.0 / nr * c)
        Mc[:3, 3] = [0.1 * np.cos(c * 2.1), 0.02 * c, 0.1 * np.sin(c * 2.1)]
        M_c.append(Mc)
    return M_c, M_t


def frontend_frame(FE, S, part, held, outlier=None):
    """a frontend.cMultiFrame holding the arrays of one frame of a pair (no extraction); the pair's rig arithmetic must be the front end's"""
    synth = importlib.import_module("multicol-slam_amd.synth")
    rig, F = S["rig"], S[part]
    nr = S["cur"]["nr"]
    models = [FE.cCamModelGeneral_.from_dict(c, synth.mirror_mask(c)) for c in rig["cams"]]
    M_c, M_t = rig_motion(nr)
    out = FE.cMultiFrame.__new__(FE.cMultiFrame)
    out.camSystem = FE.cMultiCamSys_(models, M_c, M_t)
    for c in range(nr):
        assert np.array_equal(out.camSystem.MtMc[c], rig["MtMc"][c]) and np.array_equal(out.camSystem.MtMc_inv[c], rig["MtMc_inv"][c])
    dim = S["dim"]
    mask = F["mask"] if F["mask"] is not None else np.zeros((F["n"], dim), np.uint8)
    out.mvKeys, out.keypoint_to_cam, out.totalN, out.mnId = F["keys"], F["cam"], F["n"], 1
    out.mDescriptors = [F["desc"][F["cam"] == c] for c in range(nr)]
    out.mDescriptorMasks = [mask[F["cam"] == c] for c in range(nr)]
    out.descDimension = dim
    out.mnMaxX, out.mnMaxY, out.mvScaleFactors = S["cur"]["width"].tolist(), S["cur"]["height"].tolist(), S["cur"]["scales"].tolist()
    out.mvpMapPoints = [None if k < 0 else int(k) for k in held]
    if outlier is not None:
        out.mvbOutlier = np.asarray(outlier, np.uint8)
    return out


def held_after(S, window, ori, lo=0, hi=INT_MAX):
    if window:
        e = LS.expected_window(S, ori, min_level=lo, max_level=hi)
        return e["nmatches"], e["points2"]
    e = LS.expected_last(S, ori)
    return e["nmatches"], e["cur_points"]


# (2, 6): the octave filters TrackPreviousFrame's first call switches on, through both layers; asymmetric, so that a swapped pair shows
@pytest.mark.parametrize("name,window,lo,hi", [("3x401", False, 0, INT_MAX), ("8x256", False, 0, INT_MAX), ("3x401", True, 0, INT_MAX), ("8x256", True, 0, INT_MAX),
                                               ("3x401", True, 2, 6)])
def test_front_end_and_cpp_facade_match_the_oracle(tmp_path, name, window, lo, hi):
    import gpu_common as G
    FE = importlib.import_module("multicol-slam_amd.frontend")
    S = LS.make_pair(window=window, **LS.SCENES[name])
    La, Cu, T, rig = S["last"], S["cur"], S["pts"], S["rig"]
    nr, dim, masks = Cu["nr"], S["dim"], S["masks"]
    pts = dict(pos=T["pos"], flags=T["flags"])
    # ---- the Python front end, both kinds
    for ori in (0, 1):
        want_n, want_held = held_after(S, window, ori, lo, hi)
        for device in (False, True):
            Last = frontend_frame(FE, S, "last", La["points"], La["outlier"])
            Cur = frontend_frame(FE, S, "cur", S["cur_points"])
            if window:
                r = FE.TrackPreviousFrameWindowSearch(Last, Cur, pts, LS.WINDOW, lo, hi, 0.8, dim, masks, bool(ori), device, G.ctx())
                assert np.array_equal(r["match21"], LS.expected_window(S, ori, min_level=lo, max_level=hi)["match21"]) and np.array_equal(r["points2"], want_held)
            else:
                r = FE.TrackWithMotionModelSearch(Cur, Last, pts, LS.TH, dim, masks, bool(ori), device, G.ctx())
                e = LS.expected_last(S, ori)
                assert np.array_equal(r["match_cur"], e["match_cur"]) and np.array_equal(r["assigned"], e["assigned"]) and np.array_equal(r["cur_points"], want_held)
            assert r["nmatches"] == want_n, (ori, device)
            got = np.array([-1 if m is None else m for m in Cur.mvpMapPoints])
            assert np.array_equal(got, want_held), (ori, device)       # (a dropped match was free on entry: -1 either way)
    # ---- the C++ facade on the same pair
    exe = tmp_path / "facade_driver_lastframe"
    lib_dir = os.path.join(ROOT, "multicol-slam_amd")
    subprocess.check_call(["g++", "-O1", "-std=c++14", "-Wall", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "facade_driver_lastframe.cpp"), "-o", str(exe), "-L" + lib_dir, "-lmcs_hip", "-Wl,-rpath," + lib_dir])
    M_c, M_t = rig_motion(nr)
    zeros = np.zeros((La["n"], dim), np.uint8)
    for ori in (0, 1):
        fin, fout = tmp_path / ("in%d.bin" % ori), tmp_path / ("out%d.bin" % ori)
        with open(fin, "wb") as f:
            f.write(np.array([nr, dim, len(Cu["scales"]), 1, masks, ori, window, LS.WINDOW, lo, hi], np.int32).tobytes())
            f.write(np.array([LS.TH, 0.8], np.float64).tobytes())
            for c in range(nr):
                f.write(bytes(G.mcs.make_ocam(rig["cams"][c])) + np.asarray(M_c[c], np.float64).tobytes())
                f.write(np.ascontiguousarray(rig["masks"][c], np.uint8).tobytes())
            f.write(np.asarray(M_t, np.float64).tobytes() + np.ascontiguousarray(Cu["scales"], np.float64).tobytes())
            f.write(np.array([T["n"]], np.int32).tobytes())
            for i in range(T["n"]):
                f.write(T["pos"][i].tobytes() + np.array([T["flags"][i] & 1], np.int32).tobytes())
            for F, held, out in ((La, La["points"], La["outlier"]), (Cu, S["cur_points"], np.zeros(Cu["n"], np.uint8))):
                f.write(np.array([F["n"]], np.int32).tobytes() + np.ascontiguousarray(F["keys"]).tobytes() + F["cam"].astype(np.int32).tobytes())
                f.write(F["desc"].tobytes() + (F["mask"] if F["mask"] is not None else zeros).tobytes())
                f.write(np.ascontiguousarray(held, np.int32).tobytes() + np.ascontiguousarray(out, np.uint8).tobytes())
        subprocess.check_call([str(exe), str(fin), str(fout)])
        buf = open(fout, "rb").read()
        want_n, want_held = held_after(S, window, ori, lo, hi)
        assert len(buf) == 4 + 4 * Cu["n"]
        assert int(np.frombuffer(buf, np.int32, 1, 0)[0]) == want_n, ori
        got = np.frombuffer(buf, np.int32, Cu["n"], 4)
        assert np.array_equal(got, want_held), ori
