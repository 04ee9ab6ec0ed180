"""CPU: tests/mappoint_model.py — the statement of cMapPoint::UpdateNormalAndDepth / ComputeDistinctiveDescriptors that tests/test_gpu_mappoints.py holds
mcs_covis_update_points to — checked four ways:
  (a) against an independent numpy statement (incidence matrix, explicit ordered sums, brute-force medians);
  (b) against the REFERENCE's own code where the existing wrappers of oracle/_ref expose it: rs_fuse_probes' GetMin/MaxDistanceInvariance of single-observer
      points and rs_distinctive's chosen descriptor of one keyframe's observations (skipped where oracle/_ref is not built);
  (c) every case of tests/mappoint_cases.py does what it is there for, asserted from the model's own decisions;
  (d) the header declares the two entry points and the built library exports them."""
import importlib
import os

import numpy as np
import pytest

import covis_model as M
import mappoint_cases as MC
import mappoint_model as MM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_SO = os.path.join(ROOT, "oracle", "_ref", "libmcs_ref.so")
needs_ref = pytest.mark.skipif(not os.path.exists(REF_SO), reason="oracle/_ref not built (needs the reference checkout)")


# ---------------------------------------------------------------------------------------------- (a) an independent statement
def random_map_store(seed, n_kf=9, n_feat=30, n_points=60, dim=32, masks=True):
    rng = np.random.default_rng(seed)
    ms = MM.MapStore(M.random_store(seed, n_kf, n_feat, n_points))
    for k in sorted(ms.s.rows):
        ms.set_octaves(k, rng.integers(0, MC.NLEVELS, n_feat))
        ms.set_descriptors(k, rng.integers(0, 256, (n_feat, dim), dtype=np.uint8), rng.integers(0, 256, (n_feat, dim), dtype=np.uint8) if masks else None)
    ms.s.kf_bad[sorted(ms.s.rows)[2]] = True
    return ms, rng


def numpy_statement(ms, p, pos, ref, with_masks):
    """-> (normal, min, max, N, chosen (kf, feat)) of a point that is not bad, from the incidence matrix"""
    kids = sorted(ms.s.rows)
    n_feat = max(len(ms.s.rows[k]) for k in kids)
    inc = np.zeros((len(kids), n_feat), bool)
    for a, k in enumerate(kids):
        inc[a, :len(ms.s.rows[k])] = np.array(ms.s.rows[k]) == p
    T = np.array([ms.s.t[k] for k in kids], np.float64)
    s = np.zeros(3)
    n = 0
    with np.errstate(all="ignore"):
        for a in np.flatnonzero(inc.any(axis=1)):                                # ascending slot order, one term per keyframe
            d = np.asarray(pos, np.float64) - T[a]
            s = s + d * (1.0 / np.sqrt(((0.0 + d[0] * d[0]) + d[1] * d[1]) + d[2] * d[2]))
            n += 1
        normal = s * (np.float64(1.0) / np.float64(n))
    r = kids.index(ref)
    level = int(ms.octaves[ref][int(np.flatnonzero(inc[r])[0])]) if inc[r].any() else 1
    d = np.asarray(pos, np.float64) - T[r]
    dist = np.sqrt(((0.0 + d[0] * d[0]) + d[1] * d[1]) + d[2] * d[2])
    sf = np.float64(MC.SCALES[level])
    mn, mx = ((1.0 / sf) * dist) / sf, (sf * dist) * np.float64(MC.SCALES[MC.NLEVELS - 1 - level])
    rows = [(kids[a], int(f)) for a, f in zip(*np.nonzero(inc)) if not ms.s.kf_bad[kids[a]]]      # row-major: ascending slot, ascending feature
    best = None
    if rows:
        best, best_median = 0, None
        if len(rows) > 2:
            for i in range(len(rows) - 1):
                dists = sorted(MM.distance(ms.desc[rows[i][0]][rows[i][1]], ms.desc[rows[j][0]][rows[j][1]],
                                           ms.mask[rows[i][0]][rows[i][1]] if with_masks else None, ms.mask[rows[j][0]][rows[j][1]] if with_masks else None)
                               for j in range(i + 1, len(rows)))
                med = dists[len(dists) // 2]
                if best_median is None or med < best_median:
                    best, best_median = i, med
        best = rows[best]
    return normal, mn, mx, len(rows), best


@pytest.mark.parametrize("masks", [True, False])
def test_model_against_an_independent_statement(masks):
    ms, rng = random_map_store(5 + int(masks), masks=masks)
    pts = [p for p in range(60) if p not in ms.s.pt_bad]
    pos = rng.normal(0, 3, (len(pts), 3))
    ref = [sorted(ms.s.rows)[int(j)] for j in rng.integers(0, len(ms.s.rows), len(pts))]
    got = MM.update_points(ms, pts, pos, ref, MC.SCALES, np.zeros((len(pts), 32), np.uint8), np.zeros((len(pts), 32), np.uint8) if masks else None)
    assert (got["status"] == 0).all() and (got["n_desc"] > 2).sum() > 20 and (got["n_desc"] == 0).any()
    for i, p in enumerate(pts):
        normal, mn, mx, N, best = numpy_statement(ms, p, pos[i], ref[i], masks)
        assert got["normal"][i].tobytes() == normal.tobytes(), p
        assert got["min_dist"][i] == mn and got["max_dist"][i] == mx and got["min_inv"][i] == 0.8 * mn and got["max_inv"][i] == 1.2 * mx
        assert got["n_desc"][i] == N
        if N:
            assert (got["best_kf"][i], got["best_feat"][i]) == best
            assert np.array_equal(got["desc"][i], ms.desc[best[0]][best[1]])
            assert not masks or np.array_equal(got["mask"][i], ms.mask[best[0]][best[1]])
        else:
            assert got["best_kf"][i] == -1 and not got["desc"][i].any()


def test_distance_matrix_is_the_pairwise_distance():
    rng = np.random.default_rng(2)
    for dim in (16, 32, 64):
        D, Mk = rng.integers(0, 256, (9, dim), dtype=np.uint8), rng.integers(0, 256, (9, dim), dtype=np.uint8)
        for masks in (None, Mk):
            X = MM.distance_matrix(D, masks)
            for i in range(9):
                for j in range(9):
                    assert X[i, j] == MM.distance(D[i], D[j], None if masks is None else Mk[i], None if masks is None else Mk[j])


# ---------------------------------------------------------------------------------------------- (b) the reference's own code
def motion(rz_deg, t):
    a = np.deg2rad(rz_deg)
    Mt = np.eye(4)
    Mt[:3, :3] = [[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]]
    Mt[:3, 3] = t
    return Mt


@pytest.fixture(scope="module")
def ref_scene(tmp_path_factory):
    import ref_scene as RS
    import test_io_formats as T
    import vocab_synth
    synth = importlib.import_module("multicol-slam_amd.synth")
    io = importlib.import_module("multicol-slam_amd.io")
    voc_path = str(tmp_path_factory.mktemp("voc") / "voc.yml")
    vocab_synth.write_vocabulary(voc_path, k=9, L=5, seed=3)
    cams = synth.lafida_cameras()
    masks = [np.ascontiguousarray(synth.mirror_mask(c)) for c in cams]
    S = RS.RefScene(cams, masks, [io.cayley2hom(c) for c in T.CAYLEY], voc_path, nfeatures=400, do_dBrief=1, learnMasks=1)
    poses = [motion(0.3, [0.05, 0.02, -0.03]), motion(0.7, [0.07, 0.01, -0.015])]
    frames = [S.frame(S.add_frame(synth.synth_multiframe(f, cams), 0.04 * f, poses[f])) for f in range(2)]
    kS = S.make_keyframe(0)
    S.set_mappoints(False, 1, np.zeros(frames[1]["n"], np.uint8), base=0, ref_kf=kS)
    kT = S.make_keyframe(1)
    _, dbl = S.frame_extra(0)
    yield dict(S=S, fr=frames, poses=poses, kS=kS, kT=kT, scales=dbl[1:1 + 8].copy())
    S.close()


def one_keyframe_model(fr, row, t):
    ms = MM.MapStore()
    ms.set_keyframe(1, row)
    ms.s.t[1] = tuple(float(v) for v in t)
    ms.set_octaves(1, fr["keys"]["octave"])
    ms.set_descriptors(1, fr["desc"], fr["mask"])
    return ms


@needs_ref
def test_depth_range_of_single_observer_points_is_the_references(ref_scene):
    """cMapPoint::UpdateNormalAndDepth -> GetMinDistanceInvariance / GetMaxDistanceInvariance through rs_fuse_probes, bit for bit (no Vec division involved)"""
    sc = ref_scene
    S, fr = sc["S"], sc["fr"][0]
    rng = np.random.default_rng(8)
    feat = np.sort(rng.choice(fr["n"], 60, replace=False)).astype(np.int32)
    pos = np.ascontiguousarray(rng.normal(0, 4, (60, 3)))
    best, mm = np.zeros((60, 3), np.int32), np.zeros((60, 2))
    assert S.L.rs_fuse_probes(S.h, sc["kT"], sc["kS"], feat.ctypes.data, pos.ctypes.data, 60, 3.0, best.ctypes.data, mm.ctypes.data) == 0
    row = np.full(fr["n"], -1, np.int64)
    row[feat] = np.arange(60)
    ms = one_keyframe_model(fr, row, sc["poses"][0][:3, 3])
    assert np.array_equal(sc["scales"], MC.SCALES)
    got = MM.update_points(ms, np.arange(60), pos, [1] * 60, sc["scales"])
    assert (got["status"] == 0).all() and len(set(fr["keys"]["octave"][feat].tolist())) > 3
    assert got["min_inv"].tobytes() == mm[:, 0].tobytes() and got["max_inv"].tobytes() == mm[:, 1].tobytes()


@needs_ref
def test_chosen_descriptor_of_one_keyframes_observations_is_the_references(ref_scene):
    sc = ref_scene
    S, fr = sc["S"], sc["fr"][0]
    rng = np.random.default_rng(4)
    for n in (1, 2, 3, 4, 7, 12, 25):
        idx = np.sort(rng.choice(fr["n"], n, replace=False)).astype(np.int32)
        d, m = np.zeros(32, np.uint8), np.zeros(32, np.uint8)
        assert S.L.rs_distinctive(S.h, sc["kS"], idx.ctypes.data, n, d.ctypes.data, m.ctypes.data) == 0
        row = np.full(fr["n"], -1, np.int64)
        row[idx] = 0
        got = MM.compute_distinctive_descriptors(one_keyframe_model(fr, row, (0, 0, 0)), 0)
        assert got["n_desc"] == n and got["best_kf"] == 1 and got["best_feat"] in idx
        assert np.array_equal(got["desc"], d) and np.array_equal(got["mask"], m), n


# ---------------------------------------------------------------------------------------------- (c) the cases do their job
@pytest.mark.parametrize("masks", [False, True])
@pytest.mark.parametrize("dim", [16, 32, 64])
def test_small_cases_reach_every_status_and_quirk(dim, masks):
    MC.assert_small_case_does_its_job(MC.small_case(dim, masks))


@pytest.mark.parametrize("S", sorted(MC.SEG_LENGTHS))
def test_segment_cases_have_their_lengths_and_show_the_order_of_the_sum(S):
    MC.assert_segment_case_does_its_job(MC.segment_case(S))


def test_list_case():
    MC.assert_list_case_does_its_job(MC.list_case())


def test_out_of_range_and_repeated_ids_in_the_model():
    c = MC.small_case(32, True)
    ids, pos, ref = c.call
    call = (list(ids) + [MC.SMALL_MAX_PTS + 5, -1, MC.P_N3], np.vstack([pos, pos[[0, 1, 5]]]), list(ref) + [MC.A, MC.A, MC.A])
    w = MC.run_model(c, MC.model_of(c), call, max_points=MC.SMALL_MAX_PTS)
    assert w["status"][-3:].tolist() == [1, 1, 0] and w["normal"][-3].tolist() == [MM.SENTINEL["normal"]] * 3
    # the copy of P_N3 has another position and another reference keyframe: its own normal and depth, the same descriptor
    assert w["normal"][-1].tobytes() != w["normal"][MC.P_N3].tobytes() and np.array_equal(w["desc"][-1], w["desc"][MC.P_N3])


# ---------------------------------------------------------------------------------------------- (d) header and library
NAMES = ["mcs_covis_set_keyframe_descriptors", "mcs_covis_update_points"]


def test_header_declares_and_library_exports_the_two_entry_points():
    import __graft_entry__ as ge
    ge.build()
    pkg = importlib.import_module("multicol-slam_amd")
    hdr = open(os.path.join(ROOT, "include", "mcs_c.h")).read()
    L = pkg.lib()
    for n in NAMES:
        assert ("int %s(" % n) in hdr, n
        assert hasattr(L, n), "libmcs_hip.so does not export %s" % n
        assert n in pkg._capi.EXPORTS, "_capi.EXPORTS does not list %s" % n
    assert "src/cMapPoint.cpp:449-492" in hdr and "src/cMapPoint.cpp:294-388" in hdr


def test_facade_use_compiles(tmp_path):
    import subprocess
    src = tmp_path / "mappoints_use.cpp"
    src.write_text('#include "mcs/mcs_facade.hpp"\n'
                   'struct KF { long unsigned int mnId; };\n'
                   'int use(MultiColSLAM::Context& c) {\n'
                   '  MultiColSLAM::cCovisibility<KF> s(c, 8, 16, 100);\n'
                   '  KF a{1};\n'
                   '  s.SetKeyFrame(&a, {0, 1, 2, -1});\n'
                   '  std::vector<uint8_t> d(4 * 32), m(4 * 32), pd(2 * 32), pm(2 * 32);\n'
                   '  s.SetDescriptors(&a, d.data(), m.data(), 32, 4);\n'
                   '  auto r = s.UpdateMapPoints({0, 1}, {0, 0, 1, 0, 1, 0}, {&a, &a}, {1.0, 1.2, 1.44}, pd.data(), pm.data());\n'
                   '  auto q = s.UpdateMapPoints({0, 1}, {0, 0, 1, 0, 1, 0}, {&a, &a}, {1.0, 1.2, 1.44});\n'
                   '  return (int)r.status.size() + (int)q.mNormalVector.size() + (r.bestKF[0] ? 1 : 0) + s.descriptorSize();\n'
                   '}\n')
    subprocess.check_call(["g++", "-std=c++14", "-Wall", "-Werror", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), str(src)])
