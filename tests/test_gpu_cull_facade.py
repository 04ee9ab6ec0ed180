"""-m gpu: frontend.cCovisibility.SetOctaves / KeyFrameCulling / Observations / MapPointCulling on a small synthetic map of frontend.cMultiKeyFrame objects
against tests/cull_model.py, host-kind and device-kind variants; the bodies of cLocalMapping::KeyFrameCulling / MapPointCulling as INTEGRATION.md writes them."""
import importlib

import numpy as np
import pytest

import covis_model as M
import cull_model as CM

pytestmark = pytest.mark.gpu


class MapPoint:
    def __init__(self, mnId, found, visible, first):
        self.mnId, self.mnFound, self.mnVisible, self.mnFirstKFid = mnId, found, visible, first


def synthetic_map(FE, pkg, seed):
    """keyframe objects (mnId, mvpMapPoints of MapPoint objects / None, mvKeys with the octaves) of a cull_model.random_cull_store"""
    st, octs = CM.random_cull_store(seed, 24, 60)
    rng = np.random.default_rng(seed)
    pts = {}
    for k in sorted(st.rows):                                                      # a point's first keyframe is the first that holds it
        for p in st.rows[k]:
            if p >= 0 and int(p) not in pts:
                pts[int(p)] = MapPoint(int(p), int(rng.integers(0, 9)), int(rng.integers(0, 9)), k)
    kfs = []
    for k in sorted(st.rows):
        kf = FE.cMultiKeyFrame.__new__(FE.cMultiKeyFrame)
        kf.mnId = k
        kf.mvKeys = np.zeros(len(st.rows[k]), pkg._capi.KP_DTYPE)
        kf.mvKeys["octave"] = octs[k]
        kf.mvpMapPoints = [None if p < 0 else pts[int(p)] for p in st.rows[k]]
        kf.mbNotErase = bool(rng.random() < 0.15)
        kfs.append(kf)
    return st, octs, kfs, pts


@pytest.mark.parametrize("device", [False, True])
def test_local_mapping_culling_steps(device):
    import gpu_common as G
    pkg = G.mcs
    FE = importlib.import_module("multicol-slam_amd.frontend")
    st, octs, kfs, pts = synthetic_map(FE, pkg, 9)
    n_pts = max(pts) + 1
    store = FE.cCovisibility(len(kfs), 60, n_pts, ctx=G.ctx())
    for kf in kfs:
        store.SetKeyFrame(kf)
        store.SetOctaves(kf, device=device)                                        # default: the keyframe's keypoints
    every = sorted(pts)
    assert store.Observations(every, device=device) == CM.observations(st, every)
    # ---- MapPointCulling: mlpRecentAddedMapPoints = the points first seen by the later half of the keyframes
    by_id = {kf.mnId: kf for kf in kfs}
    cur = by_id[max(sorted(st.rows), key=lambda k: len(M.update_connections(st, k)["ordered"] or []))]   # the keyframe with the longest covisible list
    recent = [pts[p] for p in every if pts[p].mnFirstKFid >= kfs[-12].mnId]
    want = CM.map_point_culling(st, cur.mnId, [m.mnId for m in recent], [m.mnFound for m in recent], [m.mnVisible for m in recent], [m.mnFirstKFid for m in recent])
    verdicts, remaining = store.MapPointCulling(cur, recent, [m.mnFound for m in recent], [m.mnVisible for m in recent], [m.mnFirstKFid for m in recent],
                                                device=device)
    assert verdicts == want["verdict"] and [m.mnId for m in remaining] == want["remaining"] and len(set(want["verdict"])) >= 3
    model = want["store"]
    # ---- KeyFrameCulling over the covisible list in the order UpdateConnections gives it
    order = store.UpdateConnections([cur])[0]["ordered"]
    assert len(order) >= 6
    local = [by_id[k] for k in order]
    want = CM.keyframe_culling(model, octs, order, [kf.mbNotErase for kf in local])
    CM.not_vacuous(want)
    got = store.KeyFrameCulling(local, device=device)                              # not_erase: the keyframes' mbNotErase
    assert got["verdict"] == want["verdict"] and got["n_mps"] == want["n_mps"] and got["n_redundant"] == want["n_redundant"]
    assert [kf.mnId for kf in got["culled"]] == want["culled"] and [kf.mnId for kf in got["to_be_erased"]] == want["to_be_erased"]
    assert got["bad_points"] == want["bad_points"] and got["n_bad_points"] == len(want["bad_points"])
    for kf in got["culled"]:                                                       # the caller's part: SetBadFlag's bookkeeping, then the store
        store.EraseKeyFrame(kf)
    model = CM.erase_culled(want["store"], want["culled"])
    assert store.Observations(every, device=device) == CM.observations(model, every)
    assert store.size() == len(kfs) - len(want["culled"])
    # a cap below the number of bad points cuts the list, not the count
    st2, octs2, kfs2, pts2 = synthetic_map(FE, pkg, 9)
    store2 = FE.cCovisibility(len(kfs2), 60, n_pts, ctx=G.ctx())
    for kf in kfs2:
        store2.SetKeyFrame(kf)
        store2.SetOctaves(kf, kf.mvKeys["octave"])
    ids2 = [kf.mnId for kf in kfs2]
    w2 = CM.keyframe_culling(st2, octs2, ids2)
    g2 = store2.KeyFrameCulling(ids2, not_erase=[0] * len(ids2), cap=2, device=device)
    assert len(w2["bad_points"]) > 2 and g2["n_bad_points"] == len(w2["bad_points"]) and g2["bad_points"] == w2["bad_points"][:2] and g2["verdict"] == w2["verdict"]
