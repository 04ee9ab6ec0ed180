"""-m gpu: MultiColSLAM::cMultiKeyFrameDatabase of the C++ facade (include/mcs/mcs_facade.hpp) compiled with g++ and run end to end
(tests/cpp/facade_driver_kfdb.cpp) against the model of tests/kfdb_model.py."""
import os
import subprocess

import numpy as np
import pytest

import kfdb_model as M

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cpp_facade_keyframe_database(tmp_path):
    exe = tmp_path / "facade_driver_kfdb"
    lib_dir = os.path.join(ROOT, "multicol-slam_amd")
    subprocess.check_call(["g++", "-O1", "-std=c++14", "-Wall", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "facade_driver_kfdb.cpp"),
                           "-o", str(exe), "-L" + lib_dir, "-lmcs_hip", "-Wl,-rpath," + lib_dir])
    rng = np.random.default_rng(21)
    n_words, nkf, nq = 6999, 128, 6
    p = 1.0 / (np.arange(n_words) + 10.0) ** 1.1
    p /= p.sum()
    bows = []
    for _ in range(nkf + nq):
        w = np.unique(rng.choice(n_words, int(rng.integers(100, 600)), p=p)).astype(np.int32)
        v = rng.random(len(w)) + 0.01
        bows.append((w, v / v.sum()))
    covis = [[int(x) for x in rng.choice(nkf, int(rng.integers(0, 11)), replace=False) if x != i] for i in range(nkf)]
    kfs = [M.KF(i + 1, list(zip(bows[i][0].tolist(), bows[i][1].tolist()))) for i in range(nkf)]
    for i in range(nkf):
        kfs[i].neighbours = [kfs[j] for j in covis[i]]
    fin, fout = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(fin, "wb") as f:
        f.write(np.array([nkf, nq, n_words], np.int32).tobytes())
        for i in range(nkf + nq):
            w, v = bows[i]
            f.write(np.array([i + 1 if i < nkf else 5000 + i], np.int64).tobytes())
            f.write(np.array([len(w)], np.int32).tobytes() + w.tobytes() + v.astype(np.float64).tobytes())
            if i < nkf:
                f.write(np.array([len(covis[i])], np.int32).tobytes() + (np.array(covis[i], np.int64) + 1).tobytes())
    subprocess.check_call([str(exe), str(fin), str(fout)])
    buf = open(fout, "rb").read()
    off = [0]

    def ids():
        n = int(np.frombuffer(buf, np.int32, 1, off[0])[0])
        a = np.frombuffer(buf, np.int64, n, off[0] + 4).tolist()
        off[0] += 4 + 8 * n
        return a

    db = M.Database(n_words)
    for k in kfs:
        db.add(k)
    qb = [list(zip(bows[nkf + q][0].tolist(), bows[nkf + q][1].tolist())) for q in range(nq)]
    total = 0
    for q in range(nq):
        e = [k.mnId for k in db.DetectRelocalisationCandidates(5000 + nkf + q, qb[q])]
        assert ids() == e
        total += len(e)
    for q in range(nq):
        assert ids() == [k.mnId for k in db.DetectRelocalisationCandidates(5000 + nkf + q + 1000000, qb[q])]
    for i in range(4):
        assert ids() == [k.mnId for k in db.DetectLoopCandidates(kfs[i], 0.0, kfs[i].neighbours)]
    s = np.frombuffer(buf, np.float64, nkf, off[0])
    assert s.tolist() == [M.l1_score(qb[0], k.bow) for k in kfs] and total > 0
