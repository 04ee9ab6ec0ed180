"""CPU checks of the Sim3 RANSAC (src/cSim3Solver.cpp): the model's known answers, its Jacobi restatement against LAPACK, the draw generator and
the C ABI exports (version 10)."""
import importlib
import os
import subprocess

import numpy as np
import pytest

import sim3_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["mcs_sim3_create", "mcs_sim3_destroy", "mcs_sim3_set_ransac_parameters", "mcs_sim3_iterate", "mcs_sim3_best", "mcs_sim3_info",
         "mcs_sim3_hypotheses", "mcs_sim3_draw"]


@pytest.fixture(scope="module")
def pkg():
    import __graft_entry__ as ge
    ge.build()
    return importlib.import_module("multicol-slam_amd")


def rot(rng):
    return M.random_pose(rng)[:3, :3]


def test_noise_free_sim3_is_recovered():
    rng = np.random.default_rng(1)
    for _ in range(50):
        R, s, t = rot(rng), float(rng.uniform(0.3, 3.0)), rng.normal(0, 2, 3)
        P2 = rng.normal(0, 3, (3, 3))             # one point per column
        P1 = s * (R @ P2) + t[:, None]
        h = M.compute_t(P1.tolist(), P2.tolist())
        assert abs(h["s"] - s) < 1e-12 * s
        assert np.abs(h["R"] - R).max() < 1e-12 and np.abs(h["t"] - t).max() < 1e-11
        T12, T21 = h["T12"], h["T21"]
        assert np.abs(T12 @ T21 - np.eye(4)).max() < 1e-12


def test_iteration_counts():
    want = {15: 1, 16: 3, 20: 8, 30: 30, 50: 143, 100: 300, 12281: 300, 12282: 1, 16000: 1}
    assert {n: M.ransac_max_its(0.98, 15, 300, n) for n in want} == want
    assert M.ransac_max_its(0.99, 6, 300, 6) == 1 and M.ransac_max_its(0.98, 15, 0, 100) == 1   # max(1, ...)


def test_truncated_thresholds():
    assert [M.max_error(v) for v in M.level_sigma2()] == [9, 13, 19, 27, 39, 57, 82, 118]
    assert [M.max_error(1.2 ** (2 * o)) for o in range(8)] == [9, 13, 19, 27, 39, 57, 82, 118]


def test_jacobi_against_lapack():
    rng = np.random.default_rng(2)
    for _ in range(300):
        A = rng.normal(size=(4, 4)) * 10.0 ** rng.integers(-3, 4)
        A = A + A.T
        W, V = M.jacobi_eigen(A.tolist())
        ew, ev = np.linalg.eigh(A)
        assert np.allclose(W, ew[::-1], rtol=0, atol=1e-12 * np.abs(ew).max())
        assert all(W[i] >= W[i + 1] for i in range(3))
        V = np.array(V)
        assert np.allclose(V @ V.T, np.eye(4), atol=1e-12)
        assert np.allclose(V @ A @ V.T, np.diag(W), atol=1e-11 * np.abs(ew).max())
        # the top eigenvector, up to sign, where it is unique
        if ew[3] - ew[2] > 1e-6 * np.abs(ew).max():
            v, e = V[0], ev[:, 3]
            assert min(np.abs(v - e).max(), np.abs(v + e).max()) < 1e-9


def test_draws_hand_values(pkg):
    # splitmix64 seeded at 0: the first outputs are 0xE220A8397B1DCDAF, 0x6E789E6AA1B965F4, 0x06C45D188009454F
    assert [M.draw(0, 0, 0, j, 1 << 32) for j in range(3)] == [0xE220A839, 0x6E789E6A, 0x06C45D18]
    assert M.draw(0, 0, 0, 0, 1000) == 883 and M.draw(0, 1, 0, 0, 1 << 32) == M.draw(0x9E3779B97F4A7C15 << 32 & ((1 << 64) - 1), 0, 0, 0, 1 << 32)
    L = pkg.lib()
    rng = np.random.default_rng(3)
    for _ in range(2000):
        seed, s, k, j, n = int(rng.integers(0, 1 << 63)), int(rng.integers(0, 40)), int(rng.integers(0, 300)), int(rng.integers(0, 3)), int(rng.integers(1, 20000))
        assert L.mcs_sim3_draw(seed, s, k, j, n) == M.draw(seed, s, k, j, n)
    assert L.mcs_sim3_draw(0, 0, 0, 3, 10) == -1


def test_duplicate_draw_gives_nan_and_the_zero_update():
    import gpu_common  # noqa: F401  (sys.path / package import like the other CPU tests of the model)
    cams = gpu_common.cams3()
    M_c = M.rig_poses(3)
    rng = np.random.default_rng(4)
    pair = M.make_pair(rng, M_c, 20, inlier_frac=1.0)
    pair["Xw"][19] = pair["Xw"][18]          # two correspondences with the same points
    pair["cam"][19] = pair["cam"][18]
    m = M.model_of(pair, cams, M_c)
    m.SetRansacParameters(0.98, 15, 300)
    # randi = N-1 twice: the second read finds the stale N-1 past the popped end, the third the value moved into slot N-1
    picks, h = m.hypothesis(0, M.table_draws([[19, 19, 19]]))
    assert picks == [19, 19, 18]
    assert np.isnan(h["T12"][:3]).all()
    ok, nomore, vb, n, T, _ = m.iterate(1, M.table_draws([[19, 19, 19]] * 300))
    assert not ok and not nomore and n == 0 and not vb.any() and T is None
    assert m.mnBestInliers == 0 and np.isnan(m.best["R"]).all()   # 0 >= 0: the NaN hypothesis became the best one


def test_iterate_chunks_equal_one_call():
    import gpu_common
    cams = gpu_common.cams3()
    M_c = M.rig_poses(3)
    rng = np.random.default_rng(5)
    pair = M.make_pair(rng, M_c, 60, inlier_frac=0.35)
    dr = M.generated_draws(7, 0, 60)

    def run(sizes):
        m = M.model_of(pair, cams, M_c)
        m.SetRansacParameters(0.98, 15, 300)
        out = []
        for n in sizes:
            ok, nomore, vb, ni, T, _ = m.iterate(n, dr)
            out.append((ok, nomore, vb.tolist(), ni, None if T is None else T.tolist(), m.mnIterations))
        return out, m
    one, m1 = run([300])
    chunks, m5 = run([5] * 60)
    it = one[0][5]
    k = next(i for i, c in enumerate(chunks) if c[0] or c[1])
    assert chunks[k][:5] == one[0][:5] and chunks[k][5] == it
    assert all(not c[0] and not c[1] for c in chunks[:k])
    # bNoMore exactly when a call ends without success with the budget spent; a success returns at once and the next call resumes after it
    assert all(c[1] == (not c[0] and c[5] >= m5.mRansacMaxIts) for c in chunks)
    assert all(chunks[i + 1][5] >= chunks[i][5] for i in range(len(chunks) - 1))
    assert M.ransac_max_its(0.98, 15, 300, 60) == m1.mRansacMaxIts


def test_library_exports_the_sim3_solver(pkg):
    L = pkg.lib()
    for n in NAMES:
        assert hasattr(L, n), n
        assert n in pkg._capi.EXPORTS, n
    assert L.mcs_abi_version() == 10


def test_sim3_without_context_fails_loudly(pkg):
    import ctypes as C
    h = C.c_void_p()
    oc = pkg._capi.Ocam()
    with pytest.raises(pkg.McsError):
        pkg.check(pkg.lib().mcs_sim3_create(None, 1, None, C.byref(oc), 0, None, None, None, None, None, None, None, None, None, None, None, 0, None, C.byref(h)))
    with pytest.raises(pkg.McsError):
        pkg.check(pkg.lib().mcs_sim3_iterate(None, None, None, None, None, None, None))


def test_facade_sim3_solver_compiles(tmp_path):
    src = tmp_path / "sim3.cpp"
    src.write_text('#include "mcs/mcs_facade.hpp"\n'
                   '#include <unordered_map>\n'
                   'struct MP; struct KP { int octave; };\n'
                   'struct KF { MultiColSLAM::cMultiCamSys_ camSystem; std::unordered_map<size_t, int> keypoint_to_cam; std::vector<MP*> mp; std::vector<KP> kps;\n'
                   '  std::vector<MP*> GetMapPointMatches() { return mp; } const KP& GetKeyPoint(int i) const { return kps[i]; }\n'
                   '  double GetSigma2(int l) const { return 1.0 + l; } };\n'
                   'struct MP { double X[3]; bool isBad() { return false; } std::vector<size_t> GetIndexInKeyFrame(KF*) { return {0}; }\n'
                   '  MultiColSLAM::Vec3d GetWorldPos() { return MultiColSLAM::Vec3d{{X[0], X[1], X[2]}}; } };\n'
                   'void use(MultiColSLAM::Context& c, KF* a, KF* b, const std::vector<MP*>& m) {\n'
                   '  MultiColSLAM::cSim3Solver<KF, MP> s(c, a, b, m, &a->camSystem);\n'
                   '  s.SetRansacParameters(0.98, 15, 300); bool noMore; std::vector<bool> vb; int n; MultiColSLAM::Matx44d T{};\n'
                   '  bool ok = s.iterate(50, noMore, vb, n, T); ok = s.find(vb, n, T);\n'
                   '  std::array<double, 9> R = s.GetEstimatedRotation(); MultiColSLAM::Vec3d t = s.GetEstimatedTranslation(); double sc = s.GetEstimatedScale();\n'
                   '  (void)ok; (void)R; (void)t; (void)sc; }\n')
    subprocess.check_call(["g++", "-std=c++14", "-Wall", "-Werror", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), str(src)])
