"""Plain-Python restatement of the three reference functions behind mcs_covis_*:
    cTracking::UpdateReferenceKeyFrames   src/cTracking.cpp:1051-1123
    cTracking::UpdateReferencePoints      src/cTracking.cpp:1024-1049
    cMultiKeyFrame::UpdateConnections     src/cMultiKeyFrame.cpp:406-500 (the counting and the ordering; AddConnection / parent bookkeeping stay with the caller)
Statement by statement, with the reference's line numbers.  Where the reference has maps keyed by cMultiKeyFrame* (iterated in address order) the model has
dicts keyed by mnId iterated in ascending order: "as if keyframes were allocated at ascending addresses" (DESIGN.md section 7).

The store's stated assumption: map point p is observed by exactly those live keyframes whose row holds p — GetObservations() below."""
import math

import numpy as np


class Store:
    """what the reference keeps on its keyframes and map points, as far as the three functions read it"""

    def __init__(self):
        self.rows = {}      # mnId -> list of point ids (-1 = NULL): mvpMapPoints
        self.t = {}         # mnId -> Hom2T(GetPose())
        self.kf_bad = {}    # mnId -> cMultiKeyFrame::isBad()
        self.pt_bad = set()  # cMapPoint::isBad()
        self.holes = 0      # erased keyframes (slots the device store keeps)

    def set_keyframe(self, kid, points):
        if kid not in self.rows:
            assert not self.rows or kid > max(self.rows), "nNextId++"
            self.t[kid], self.kf_bad[kid] = (0.0, 0.0, 0.0), False
        self.rows[kid] = [int(p) for p in points]

    def erase(self, kid):
        del self.rows[kid], self.t[kid], self.kf_bad[kid]
        self.holes += 1

    def observations(self, p):
        """cMapPoint::GetObservations(): map<cMultiKeyFrame*, vector<size_t>> — one key per keyframe, however many features hold the point"""
        return [k for k in sorted(self.rows) if p in self.rows[k]]

    def observers(self):
        """point -> observing keyframes in id order, built once (observations() for every point at a time)"""
        obs = {}
        for k in sorted(self.rows):
            for p in dict.fromkeys(self.rows[k]):
                if p >= 0:
                    obs.setdefault(p, []).append(k)
        return obs


def update_reference_keyframes(store, frame_points, frame_t, obs=None):
    """-> (frame_points after the call, local_kfs, weights, dists, ref_kf or -1)"""
    obs = store.observers() if obs is None else obs
    fp = [int(p) for p in frame_points]
    counter = {}                                                  # :1055
    for i in range(len(fp)):                                      # :1056
        if fp[i] >= 0:                                            # :1058
            p = fp[i]
            if p not in store.pt_bad:                             # :1061
                for k in obs.get(p, []):                          # :1063-1066
                    counter[k] = counter.get(k, 0) + 1            # :1068
            else:
                fp[i] = -1                                        # :1074
    mx, kfmax = 0, -1                                             # :1079-1080; the reference then assigns NULL to mpReferenceKF
    kfs, ws, ds = [], [], []
    for k in sorted(counter):                                     # :1089, address order -> id order
        c = counter[k]
        if c > 4:                                                 # :1098
            if store.kf_bad[k]:                                   # :1100
                continue
            if c > mx:                                            # :1103
                mx, kfmax = c, k
            d = [float(frame_t[j]) - float(store.t[k][j]) for j in range(3)]
            s = 0.0
            for j in range(3):                                    # cv::norm: sqrt(((0 + dx^2) + dy^2) + dz^2)
                s = s + d[j] * d[j]
            ws.append(c); kfs.append(k); ds.append(math.sqrt(s))  # :1112-1115
    return fp, kfs, ws, ds, kfmax


def update_reference_points(store, local_kfs):
    """-> mvpLocalMapPoints as ids"""
    out, marked = [], set()                                       # :1026; mnTrackReferenceForFrame == mCurrentFrame.mnId
    for k in local_kfs:                                           # :1028
        for p in store.rows[k]:                                   # :1034
            if p < 0:                                             # :1038
                continue
            if p in marked:                                       # :1040
                continue
            if p not in store.pt_bad:                             # :1042
                out.append(p)                                     # :1044
                marked.add(p)                                     # :1045
    return out


def update_reference(store, frame_points, frame_t, obs=None):
    fp, kfs, ws, ds, ref = update_reference_keyframes(store, frame_points, frame_t, obs)
    return dict(frame_points=fp, local_kfs=kfs, weights=ws, dists=ds, ref_kf=ref, local_points=update_reference_points(store, kfs))


def update_connections(store, kid, obs=None, th=30):
    """-> dict(counter={mnId: count}, ordered=[mnIds] or None (unchanged), weights=[...] or None)"""
    obs = store.observers() if obs is None else obs
    counter = {}                                                  # :408
    for p in store.rows[kid]:                                     # :419
        if p < 0:                                                 # :424
            continue
        if p in store.pt_bad:                                     # :427
            continue
        for k in obs.get(p, []):                                  # :430-433
            if k == kid:                                          # :435
                continue
            counter[k] = counter.get(k, 0) + 1                    # :439
    if not counter:                                               # :443
        return dict(counter=counter, ordered=None, weights=None)
    nmax, kfmax = 0, None                                         # :448-449
    pairs = []
    for k in sorted(counter):                                     # :454, address order -> id order
        if counter[k] > nmax:                                     # :457
            nmax, kfmax = counter[k], k
        if counter[k] >= th:                                      # :462
            pairs.append((counter[k], k))
    if not pairs:                                                 # :469
        pairs.append((nmax, kfmax))
    pairs.sort()                                                  # :475, pair<int, cMultiKeyFrame*>: by weight, then address -> id
    kfs, ws = [], []
    for w, k in pairs:                                            # :478-482 push_front
        kfs.insert(0, k); ws.insert(0, w)
    return dict(counter=counter, ordered=kfs, weights=ws)


def random_store(seed, n_kf, n_feat, n_points, bad_frac=0.05, repeat_frac=0.10):
    """a store whose keyframes see overlapping windows of the points (so that counts spread around both thresholds), with repeats inside rows"""
    rng = np.random.default_rng(seed)
    st = Store()
    win = max(1, min(n_points, 2 * n_feat))
    for k in range(n_kf):
        lo = 0 if n_kf == 1 else int(round((n_points - win) * k / (n_kf - 1)))
        row = rng.integers(lo, lo + win, n_feat)
        row[rng.random(n_feat) < 0.3] = -1
        rep = np.flatnonzero(rng.random(n_feat) < repeat_frac)
        if len(rep):
            row[rep] = row[rng.integers(0, n_feat, len(rep))]
        st.set_keyframe(3 * k + 1, row)
        st.t[3 * k + 1] = tuple(float(v) for v in rng.normal(0, 2, 3))
    st.pt_bad = set(int(p) for p in np.flatnonzero(rng.random(n_points) < bad_frac))
    return st


_P30, _P31 = list(range(30)), list(range(31))
# the stores and voters of tests/test_covis_cpu.py, one per quirk: (name, rows, bad points, bad keyframes, poses, frame rows, query keyframes)
HAND_CASES = [
    ("voter_twice", {1: [0, 1, 2]}, [], [], {}, [[0, 0, 1, 1, 2], [0, 1, 2, -1, -1]], [1]),
    ("voter_twice_kf", {1: [0, 0, 0], 2: [0]}, [], [], {}, [[0, 0, 0, 0, 0]], [1, 2]),
    ("keyframe_once", {1: [0, 0, 0, 0, 0, 1]}, [], [], {}, [[0, 1], [0, 0, 0, 1, 1]], [1]),
    ("keyframe_once_kf", {1: [7], 2: [7, 7, 7]}, [], [], {}, [[7]], [1, 2]),
    ("bad_voter", {1: [0, 1, 2, 3, 4, 5]}, [5], [], {}, [[0, 1, 2, 3, 5, -1, 5], [0, 1, 2, 3, 4, 5]], [1]),
    ("bad_voter_kf", {1: [0, 5], 2: [0, 5]}, [5], [], {}, [[5, 5, 5, 5, 5]], [1, 2]),
    ("local_4_5", {1: [0, 1, 2, 3], 2: [0, 1, 2, 3, 4]}, [], [], {}, [[0, 1, 2, 3, 4]], [1, 2]),
    ("conn_29_30", {1: _P30, 2: _P30[:29], 3: _P30}, [], [], {}, [_P30], [1, 2, 3]),
    ("ref_tie", {4: [0, 1, 2, 3, 4], 9: [0, 1, 2, 3, 4], 11: [0, 1, 2, 3, 4, 5]}, [], [], {}, [[0, 1, 2, 3, 4], [0, 1, 2, 3, 4, 5], [0, 1]], [4, 9, 11]),
    ("fallback_max", {1: [0, 1, 2, 3], 2: [0, 1], 3: [2, 3], 4: [9]}, [], [], {}, [[0, 1, 2, 3]], [1, 2, 3, 4]),
    ("empty_counter", {1: [0, 1], 2: [2, 3], 3: [-1, -1]}, [], [], {}, [[-1, -1]], [1, 2, 3]),
    ("equal_weights", {1: _P31, 2: _P31[:30], 5: _P31, 7: _P31[:30], 8: _P31[1:]}, [], [], {}, [_P31], [1, 2, 5, 7, 8]),
    ("first_occurrence", {1: [5, 3, -1, 5, 1, 0, 2], 2: [9, 3, 8, 0, 1, 2, 7, 5]}, [], [], {}, [[0, 1, 2, 3, 5]], [1, 2]),
    ("bad_keyframe", {1: _P30, 2: _P30, 3: _P30[:6]}, [], [2], {}, [_P30[:6]], [1, 2, 3]),
    ("bad_keyframe_ref", {1: _P30[:5], 2: _P30[:6]}, [], [2], {}, [_P30[:6]], [1, 2]),
    ("distance", {1: [0, 1, 2, 3, 4]}, [], [], {1: (0.1, 0.2, 0.3)}, [[0, 1, 2, 3, 4]], [1]),
]
