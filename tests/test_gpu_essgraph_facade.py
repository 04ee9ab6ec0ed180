"""-m gpu: frontend.OptimizeEssentialGraph on stand-in keyframes and map points built from the scenes of tests/essgraph_scenes.py, with a bad keyframe (no
vertex; the edges that name it are left out) and a point corrected by the current keyframe (its reference is mnCorrectedReference).  The wrapper builds the
vertex list, the Shoemake quaternions, the edge list in the reference's order and the point references itself; they equal, to the bit, the lists the test
derives from the scene with the model's own conversion, and its result equals the raw call on those arrays to the bit.  SetPose and SetWorldPos receive the
outputs.  MultiColSLAM::cOptimizer::OptimizeEssentialGraph of include/mcs/mcs_facade.hpp (tests/cpp/facade_driver_essgraph.cpp) runs on the same stand-ins,
written to a scene file: it builds the lists itself, applies the results to its objects, and every pose SetPose received, every point position and the
diagnostics equal the frontend's to the bit.  With a store given, the store is refreshed from the call: what UpdateMapPoints returns equals a refresh fed by
hand from the raw call's outputs, and the normals are those of the NEW positions seen from the NEW camera centres."""
import importlib
import os
import signal
import subprocess

import numpy as np
import pytest

import essgraph_model as M
import essgraph_scenes as S

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = tmp_path_factory.mktemp("facade_eg") / "facade_driver_essgraph"
    lib_dir = os.path.join(ROOT, "multicol-slam_amd")
    subprocess.check_call(["g++", "-O1", "-std=c++14", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "facade_driver_essgraph.cpp"), "-o", str(exe), "-L" + lib_dir, "-lmcs_hip", "-Wl,-rpath," + lib_dir])
    return exe


@pytest.fixture(scope="module")
def env():
    import gpu_common as G
    return dict(pkg=G.mcs, ctx=G.ctx(), FE=importlib.import_module("multicol-slam_amd.frontend"))


@pytest.fixture(autouse=True)
def _time_limit():
    signal.signal(signal.SIGALRM, signal.SIG_DFL)
    signal.alarm(120)
    yield
    signal.alarm(0)


class KF:
    def __init__(self, mnId, pose_inv, bad=False):
        self.mnId, self.pose_inv, self.bad = mnId, pose_inv, bad
        self.parent, self.loop, self.cov, self.weight, self.pose = None, [], [], {}, None
        self.mvScaleFactors = 1.2 ** np.arange(8)

    def isBad(self):
        return self.bad

    def GetPoseInverse(self):
        return self.pose_inv

    def GetParent(self):
        return self.parent

    def GetLoopEdges(self):
        return set(self.loop)

    def GetCovisiblesByWeight(self, w):
        return [k for k in self.cov if self.weight.get(k.mnId, 0) >= w]

    def GetWeight(self, k):
        return self.weight.get(k.mnId, 0)

    def SetPose(self, Mx):
        self.pose = np.asarray(Mx).copy()

    def __hash__(self):
        return self.mnId


class MP:
    def __init__(self, pos, ref, bad=False):
        self.pos, self.mpRefKF, self.bad, self.mnCorrectedByKF, self.mnCorrectedReference = np.asarray(pos).copy(), ref, bad, -1, -1

    def isBad(self):
        return self.bad

    def GetWorldPos(self):
        return self.pos

    def SetWorldPos(self, X):
        self.pos = np.asarray(X).copy()

    def GetReferenceKeyFrame(self):
        return self.mpRefKF


class Map:
    def __init__(self, kfs, mps):
        self.kfs, self.mps = kfs, mps

    def GetAllKeyFrames(self):
        return list(reversed(self.kfs))                          # in no particular order: the wrapper sorts by mnId

    def GetAllMapPoints(self):
        return list(self.mps)


def stand_ins(name):
    """the scene as objects, mnId = 2 * index, plus bad keyframe mnId 5 (parent of keyframe 6, covisible with keyframe 8, in the loop connections of the
    current keyframe) and, per point of reference -1, a point whose reference keyframe IS the bad one; point 1 is corrected by the current keyframe"""
    pr = S.build(name)
    K = len(pr.Scw)
    kfs = []
    for k in range(K):
        Minv = np.eye(4)
        src = pr.Snc[k] if pr.has_nc[k] else pr.Scw[k]
        Minv[:3, :3] = M.quat_to_mat(src[:4]).reshape(3, 3)
        Minv[:3, 3] = src[4:7]
        kfs.append(KF(2 * k, Minv))
    badkf = KF(5, np.eye(4), bad=True)
    cur, loop = kfs[K - 1], kfs[int(np.nonzero(pr.fixed)[0][0])]
    conns = {}
    for e in range(len(pr.edge_i)):
        a, b = kfs[pr.edge_i[e]], kfs[pr.edge_j[e]]
        if pr.edge_kind[e] == 0:
            conns.setdefault(a, set()).add(b)
            a.weight[b.mnId] = 150 if a is not cur else 3       # the pair (current, loop) passes whatever its weight (:362-365)
        elif a.parent is None and b.mnId == a.mnId - 2:
            a.parent = b
        else:
            a.cov.append(b)
            a.weight[b.mnId] = 120
    kfs[4].cov.append(badkf), kfs[4].weight.__setitem__(5, 200)
    kfs[1].cov.append(kfs[0]), kfs[1].weight.__setitem__(0, 99)  # below minNumFeat: no edge
    conns.setdefault(cur, set()).add(badkf), cur.weight.__setitem__(5, 500)
    conns[cur].add(kfs[1]), cur.weight.__setitem__(2, 99)        # a loop connection below minNumFeat that is not (current, loop): no edge
    mps = [MP(pr.pos[p], kfs[pr.pt_ref[p]] if pr.pt_ref[p] >= 0 else badkf) for p in range(len(pr.pos))]
    mps[1].mnCorrectedByKF, mps[1].mnCorrectedReference = cur.mnId, kfs[2].mnId
    mps.insert(3, MP([9.0, 9.0, 9.0], kfs[0], bad=True))        # a bad point: not part of the call
    corrected = {kfs[k]: pr.Scw[k].copy() for k in range(K) if pr.has_nc[k]}
    noncorr = {kfs[k]: pr.Snc[k].copy() for k in range(K) if pr.has_nc[k]}
    allk = kfs[:3] + [badkf] + kfs[3:]
    # what the wrapper has to arrive at: the vertices' Sim3 through the model's Shoemake conversion of the same matrices
    Scw = pr.Scw.copy()
    for k in range(K):
        if not pr.has_nc[k]:
            Scw[k] = M.sim3_vec(M.sim3_from_rts(kfs[k].pose_inv[:3, :3].reshape(9), kfs[k].pose_inv[:3, 3], 1.0))
    ref = pr.pt_ref.copy()
    ref[1] = 2
    want = M.Problem(Scw, np.where(pr.has_nc[:, None] != 0, pr.Snc, 0.0), pr.has_nc, pr.fixed, pr.edge_i, pr.edge_j, pr.edge_kind, pr.pos, ref)
    return Map(allk, mps), loop, cur, noncorr, corrected, conns, kfs, want


@pytest.mark.parametrize("device", [False, True])
@pytest.mark.parametrize("name", ["fixed_mid", "dup"])
def test_frontend_builds_the_lists_and_equals_the_raw_call(env, name, device):
    FE, pkg, ctx = env["FE"], env["pkg"], env["ctx"]
    pMap, loop, cur, noncorr, corrected, conns, kfs, want = stand_ins(name)
    got_kfs, got_pts, arrays = FE._essential_graph_lists(pMap, loop, cur, noncorr, corrected, conns)
    assert [k.mnId for k in got_kfs] == [k.mnId for k in kfs] and len(got_pts) == len(want.pos)
    built = M.Problem(*arrays)
    for a, b, what in zip(built.arrays(), want.arrays(), ("Scw", "Snc", "has_nc", "fixed", "edge_i", "edge_j", "edge_kind", "pos", "pt_ref")):
        assert a.tobytes() == b.tobytes(), what
    r = FE.OptimizeEssentialGraph(pMap, loop, cur, noncorr, corrected, conns, device=device, ctx=ctx)
    raw = S.run_library(pkg, ctx, want, device)
    assert r["status"] == raw["status"] == M.EG_OK and r["diag"].tobytes() == raw["diag"].tobytes()
    for k in S.FIELDS:
        assert r[k].tobytes() == raw[k].tobytes(), k
    for i, k in enumerate(kfs):
        assert np.array_equal(k.pose, raw["pose"][i].reshape(4, 4))
    assert pMap.kfs[3].pose is None                              # the bad keyframe
    live = [mp for mp in pMap.mps if not mp.bad]
    for p, mp in enumerate(live):
        assert np.array_equal(mp.pos, raw["pos"][p])
        if want.pt_ref[p] < 0:
            assert np.array_equal(mp.pos, want.pos[p])
        elif want.fixed[want.pt_ref[p]]:                         # through the fixed vertex and back: rounding only
            assert np.abs(mp.pos - want.pos[p]).max() <= 1e-12
        else:
            assert not np.array_equal(mp.pos, want.pos[p])
    assert np.array_equal(pMap.mps[3].pos, [9.0, 9.0, 9.0])
    m = M.optimize(want)
    assert S.rel(raw["pos"][1], m.pos[1]) <= 1e-4 and want.pt_ref[1] == 2   # the point corrected by the current keyframe moved with keyframe mnId 4


def scene_file(path, pMap, loop, cur, noncorr, corrected, conns):
    """the stand-ins as tests/cpp/facade_driver_essgraph.cpp reads them; repr() of a float reads back to the same double"""
    kfs = pMap.GetAllKeyFrames()
    at = {id(k): i for i, k in enumerate(kfs)}
    f = lambda vs: " ".join(repr(float(v)) for v in np.asarray(vs, np.float64).reshape(-1))   # noqa: E731
    out = [str(len(kfs))]
    for k in kfs:
        out.append("%d %d %s" % (k.mnId, int(k.bad), f(k.pose_inv)))
        out.append(str(-1 if k.parent is None else at[id(k.parent)]))
        out.append(" ".join([str(len(k.loop))] + [str(at[id(l)]) for l in k.loop]))
        out.append(" ".join([str(len(k.cov))] + [str(at[id(c)]) for c in k.cov]))
        by_id = {q.mnId: q for q in kfs}
        out.append(" ".join([str(len(k.weight))] + ["%d %d" % (at[id(by_id[m])], w) for m, w in k.weight.items()]))
    out.append("%d %d" % (at[id(loop)], at[id(cur)]))
    for table in (corrected, noncorr):
        out.append(str(len(table)))
        out += ["%d %s" % (at[id(k)], f(v)) for k, v in table.items()]
    out.append(str(len(conns)))
    out += [" ".join([str(at[id(k)]), str(len(c))] + [str(at[id(q)]) for q in c]) for k, c in conns.items()]
    out.append(str(len(pMap.mps)))
    out += ["%s %d %d %d %d" % (f(mp.pos), int(mp.bad), at[id(mp.mpRefKF)], mp.mnCorrectedByKF, mp.mnCorrectedReference) for mp in pMap.mps]
    path.write_text("\n".join(out) + "\n")
    return kfs


@pytest.mark.parametrize("name", ["fixed_mid", "dup"])
def test_facade_equals_the_frontend_bit_for_bit(env, driver, tmp_path, name):
    FE, ctx = env["FE"], env["ctx"]
    args = stand_ins(name)[:6]
    pMap = args[0]
    order = scene_file(tmp_path / "scene.txt", *args)          # before the frontend moves anything
    lines = subprocess.check_output([str(driver), str(tmp_path / "scene.txt")], timeout=100).decode().splitlines()
    r = FE.OptimizeEssentialGraph(*args, device=False, ctx=ctx)
    head = [int(v) for v in lines[0].split()]
    d = r["diag"]
    assert head == [r["status"], int(d["iters"]), int(d["stop"])] + d["trials"].tolist() and r["status"] == M.EG_OK and d["iters"] >= 2
    for k, row in zip(order, lines[1:1 + len(order)]):
        v = row.split()
        assert (v[0] == "1") == (k.pose is not None) == (not k.bad), k.mnId
        if k.pose is not None:
            assert np.array([float.fromhex(x) for x in v[1:]]).tobytes() == np.ascontiguousarray(k.pose, np.float64).tobytes(), k.mnId
    got = np.array([[float.fromhex(x) for x in row.split()] for row in lines[1 + len(order):]])
    assert len(got) == len(pMap.mps) and got.tobytes() == np.array([mp.pos for mp in pMap.mps], np.float64).tobytes()
    assert np.array_equal(got[3], [9.0, 9.0, 9.0])               # the bad point: not part of the call


def test_with_a_store_the_poses_and_points_are_refreshed(env):
    FE, pkg, ctx = env["FE"], env["pkg"], env["ctx"]

    def scene():
        pMap, loop, cur, noncorr, corrected, conns, kfs, want = stand_ins("fixed_mid")
        live = [mp for mp in pMap.mps if not mp.bad]
        for p, mp in enumerate(live):                            # the store refreshes a point from its reference keyframe: none may be the bad one
            mp.mnId = p
            if mp.mpRefKF.bad:
                mp.mpRefKF = kfs[0]
        store = FE.cCovisibility(16, 128, len(live) + 1, ctx=ctx)
        for k in kfs:
            store.SetKeyFrame(k, [mp.mnId for mp in live if mp.mpRefKF is k])
        return (pMap, loop, cur, noncorr, corrected, conns), kfs, live, store

    args, kfs, live, store = scene()
    before = np.array([mp.pos for mp in live])
    r = FE.OptimizeEssentialGraph(*args, device=True, store=store, ctx=ctx)
    assert r["status"] == 0 and [mp.mnId for mp in r["updated"]] == [mp.mnId for mp in live]      # every point has a vertex behind it here
    up = r["update"]
    assert (up["status"][:len(live)] == 0).all()
    # by hand, from the raw call's outputs on a store of its own
    args2, kfs2, live2, store2 = scene()
    raw = FE.OptimizeEssentialGraph(*args2, device=True, ctx=ctx)
    assert "update" not in raw and raw["pos"].tobytes() == r["pos"].tobytes()
    store2.SetPose(kfs2, ts=raw["kf_t"])
    want = store2.UpdateMapPoints(live2, raw["pos"], [mp.mpRefKF for mp in live2], args2[2].mvScaleFactors)
    for k in ("normal", "min_dist", "max_dist", "status"):
        assert up[k].tobytes() == want[k].tobytes(), k
    # a point sits in its reference keyframe's row alone: its normal is the unit vector from that keyframe's NEW centre to its NEW position
    ref = np.array([[k.mnId for k in kfs].index(mp.mpRefKF.mnId) for mp in live])
    v = r["pos"] - r["kf_t"][ref]
    assert np.abs(up["normal"][:len(live)] - v / np.linalg.norm(v, axis=1)[:, None]).max() <= 1e-12
    old = before - r["kf_t"][ref]
    assert np.abs(up["normal"][:len(live)] - old / np.linalg.norm(old, axis=1)[:, None]).max() > 1e-6    # not the positions it came in with
