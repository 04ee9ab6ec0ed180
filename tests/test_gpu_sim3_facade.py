"""-m gpu: MultiColSLAM::cSim3Solver of the C++ facade (include/mcs/mcs_facade.hpp) compiled with g++ and run end to end
(tests/cpp/facade_driver_sim3.cpp) against the model of tests/sim3_model.py: every iterate(50) call of a loop-closer run and the estimate."""
import os
import subprocess

import numpy as np
import pytest

import sim3_model as M

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cpp_facade_sim3_solver(tmp_path):
    import gpu_common as G
    exe = tmp_path / "facade_driver_sim3"
    lib_dir = os.path.join(ROOT, "multicol-slam_amd")
    subprocess.check_call(["g++", "-O1", "-std=c++14", "-Wall", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "facade_driver_sim3.cpp"),
                           "-o", str(exe), "-L" + lib_dir, "-lmcs_hip", "-Wl,-rpath," + lib_dir])
    cams = G.cams3()
    M_c = M.rig_poses(3)
    rng = np.random.default_rng(31)
    pair = M.make_pair(rng, M_c, 400, inlier_frac=0.3)
    sig = M.level_sigma2()
    oct_ = np.array([[sig.index(v) for v in row] for row in pair["sigma2"]], np.int32)
    seed = 123456789
    fin, fout = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(fin, "wb") as f:
        f.write(np.array([3, len(pair["index1"]), pair["mN1"]], np.int32).tobytes() + np.array([seed], np.uint64).tobytes())
        for c in range(3):
            f.write(bytes(G.mcs.make_ocam(cams[c])) + np.asarray(M_c[c], np.float64).tobytes())
        f.write(np.array(sig, np.float64).tobytes())
        for Mt in pair["Mt"]:
            f.write(np.asarray(Mt, np.float64).tobytes())
        for i, i1 in enumerate(pair["index1"]):
            f.write(np.array([i1], np.int32).tobytes())
            for s in range(2):
                f.write(pair["Xw"][i, s].astype(np.float64).tobytes() + np.array([pair["cam"][i, s], oct_[i, s]], np.int32).tobytes())
    subprocess.check_call([str(exe), str(fin), str(fout)])
    buf = open(fout, "rb").read()
    m = M.model_of(pair, cams, M_c)
    m.SetRansacParameters(0.98, 15, 300)
    dr = M.generated_draws(seed, 0, len(pair["index1"]))
    off, calls = 0, 0
    while True:
        ok, nomore, ni = np.frombuffer(buf, np.int32, 3, off).tolist()
        vb = np.frombuffer(buf, np.uint8, pair["mN1"], off + 12).astype(bool)
        T = np.frombuffer(buf, np.float64, 16, off + 12 + pair["mN1"]).reshape(4, 4)
        off += 12 + pair["mN1"] + 128
        e = m.iterate(50, dr)
        assert (bool(ok), bool(nomore), ni) == (e[0], e[1], e[3]) and np.array_equal(vb, e[2]), calls
        if ok:
            assert np.allclose(T, e[4], rtol=1e-9, atol=1e-9)
        calls += 1
        if ok or nomore:
            break
    R = np.frombuffer(buf, np.float64, 9, off).reshape(3, 3)
    t = np.frombuffer(buf, np.float64, 3, off + 72)
    s = np.frombuffer(buf, np.float64, 1, off + 96)[0]
    assert np.allclose(R, m.best["R"], rtol=1e-9, atol=1e-9) and np.allclose(t, m.best["t"], rtol=1e-9, atol=1e-9) and abs(s - m.best["s"]) <= 1e-9 * abs(s)
    assert off + 104 == len(buf) and ok
