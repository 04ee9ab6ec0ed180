"""Plain-Python restatement of the two reference functions behind mcs_covis_update_points:
    cMapPoint::UpdateNormalAndDepth             src/cMapPoint.cpp:449-492
    cMapPoint::ComputeDistinctiveDescriptors    src/cMapPoint.cpp:294-388 (median(): include/misc.h:95-104)
over a covis_model.Store, statement by statement with the reference's line numbers.  MapStore holds a Store (composition: covis_model.py stays as it is) plus
what the two functions read beyond the rows: octaves, descriptor (and mask) rows, and — per call — the points' positions and reference keyframes.

The store's assumptions (DESIGN.md sections 4h, 4i, 7): point p is observed by exactly the live keyframes whose row holds p; a keyframe's observations of a
point are its features in ascending index; std::map<cMultiKeyFrame*, ...> is iterated in ascending mnId.

Every floating-point step is an np.float64 operation in the reference's order (OpenCV 3.x: cv::norm = sqrt(((0 + x^2) + y^2) + z^2); Vec / double and
Vec / int multiply by 1. / alpha), so the device is compared by bytes."""
import numpy as np

import covis_model as M

F = np.float64


class MapStore:
    """a covis_model.Store and, per keyframe, octaves / descriptors / masks in feature order"""

    def __init__(self, store=None):
        self.s = store if store is not None else M.Store()
        self.octaves = {}     # mnId -> [octave per feature]; absent: never set (level 0)
        self.desc = {}        # mnId -> uint8 [n][dim]
        self.mask = {}        # mnId -> uint8 [n][dim] (only when the store has masks)
        self.dim, self.masks = None, None

    # ---- what the device store does with the extra rows
    def set_keyframe(self, kid, points):
        if kid in self.s.rows and len(self.s.rows[kid]) != len(points):
            self.octaves.pop(kid, None); self.desc.pop(kid, None); self.mask.pop(kid, None)
        self.s.set_keyframe(kid, points)

    def set_octaves(self, kid, octs):
        assert len(octs) == len(self.s.rows[kid])
        self.octaves[kid] = [int(o) for o in octs]

    def set_descriptors(self, kid, desc, mask=None):
        desc = np.ascontiguousarray(desc, np.uint8).reshape(len(self.s.rows[kid]), -1)
        if self.dim is None:
            self.dim, self.masks = desc.shape[1], mask is not None
        assert desc.shape[1] == self.dim and (mask is not None) == self.masks
        self.desc[kid] = desc
        if mask is not None:
            self.mask[kid] = np.ascontiguousarray(mask, np.uint8).reshape(desc.shape)

    def erase(self, kid):
        self.s.erase(kid)
        self.octaves.pop(kid, None); self.desc.pop(kid, None); self.mask.pop(kid, None)

    def observations(self, p):
        """mObservations of point p: {keyframe: [features]} — keyframes ascending, features ascending"""
        out = {}
        for k in sorted(self.s.rows):
            idx = [i for i, q in enumerate(self.s.rows[k]) if q == p]
            if idx:
                out[k] = idx
        return out

    def observation_table(self):
        """point -> observations(point), for every point at once"""
        tab = {}
        for k in sorted(self.s.rows):
            for i, q in enumerate(self.s.rows[k]):
                if q >= 0:
                    tab.setdefault(q, {}).setdefault(k, []).append(i)
        return tab


def cv_norm(v):
    s = F(0.0)
    for x in v:                                                   # normL2Sqr: s += v * v from 0, then sqrt
        s = s + x * x
    return np.sqrt(s)


def update_normal_and_depth(ms, p, pos, ref_kf, scale_factors, obs=None):
    """-> (status, None) or (0, dict(normal, min_dist, max_dist, min_inv, max_inv, n, level))"""
    nlevels = len(scale_factors)
    sf = [F(x) for x in scale_factors]
    if p in ms.s.pt_bad:                                          # :457
        return 1, None
    if ref_kf not in ms.s.rows:                                   # pRefKF is an object the store no longer has
        return 2, None
    observations = ms.observations(p) if obs is None else obs.get(p, {})   # :459
    Pos = [F(x) for x in pos]                                     # :461
    with np.errstate(all="ignore"):
        normal = [F(0.0), F(0.0), F(0.0)]                         # :464
        n = 0                                                     # :465
        for k in observations:                                    # :466, ascending mnId; no isBad() here
            Owi = [F(x) for x in ms.s.t[k]]                       # :470
            normali = [Pos[j] - Owi[j] for j in range(3)]         # :471
            ia = F(1.0) / cv_norm(normali)                        # Vec / double: a * (1. / alpha)
            normal = [normal[j] + normali[j] * ia for j in range(3)]   # :472
            n += 1                                                # :473
        PC = [Pos[j] - F(ms.s.t[ref_kf][j]) for j in range(3)]    # :476
        dist = cv_norm(PC)                                        # :477
        level = 1                                                 # :479
        if observations.get(ref_kf):                              # :480 (operator[] default-constructs an empty vector)
            level = ms.octaves[ref_kf][observations[ref_kf][0]] if ref_kf in ms.octaves else 0   # :481
        if not 0 <= level < nlevels:                              # mvScaleFactors[level]: out of bounds in the reference
            return 3, None
        scaleFactor = sf[level]                                   # :482
        levelScaleFactor = sf[level]                              # :483
        mn = (F(1.0) / scaleFactor) * dist / levelScaleFactor     # :488
        mx = scaleFactor * dist * sf[nlevels - 1 - level]         # :489
        ia = F(1.0) / F(n)                                        # :490, Vec / int
        normal = [x * ia for x in normal]
        return 0, dict(normal=normal, min_dist=mn, max_dist=mx, min_inv=F(0.8) * mn, max_inv=F(1.2) * mx, n=n, level=level)


_POP = np.array([bin(i).count("1") for i in range(256)], np.int64)


def distance(a, b, ma=None, mb=None):
    """DescriptorDistance64 / DescriptorDistance64Masked (src/cORBmatcher.cpp:2452-2474)"""
    x = a ^ b
    if ma is None:
        return int(_POP[x].sum())
    return int(_POP[x & ma].sum() + _POP[x & mb].sum()) // 2


def distance_matrix(D, Mk=None):
    """distance() for every pair of rows at once (the matrix of :339-359): popcounts as products of the unpacked bits, exact in float32 (<= 512 per entry)"""
    a = np.unpackbits(D, axis=1).astype(np.float32)
    if Mk is None:
        x = a @ (1 - a).T
        return (x + x.T).astype(np.int64)
    m = np.unpackbits(Mk, axis=1).astype(np.float32)
    left = (m * a) @ (1 - a).T + (m * (1 - a)) @ a.T              # left[i][j] = popcount((d_i ^ d_j) & mask_i)
    return (left + left.T).astype(np.int64) // 2


def collect_rows(ms, p, obs=None):
    """:312-330 -> [(keyframe, feature)] of vDescriptors, in push_back order"""
    observations = ms.observations(p) if obs is None else obs.get(p, {})
    rows = []
    for k in observations:                                        # :314
        if not ms.s.kf_bad[k]:                                    # :319
            for l in observations[k]:                             # :321
                rows.append((k, l))                               # :325-327
    return rows


def compute_distinctive_descriptors(ms, p, obs=None):
    """-> None (bad point: :304) or dict(n_desc, best_kf, best_feat, desc, mask); N == 0: best_* -1 and desc None (the old one stays, :309-310 / :332-333)"""
    if p in ms.s.pt_bad:                                          # :304
        return None
    rows = collect_rows(ms, p, obs)
    N = len(rows)                                                 # :336
    if N == 0:
        return dict(n_desc=0, best_kf=-1, best_feat=-1, desc=None, mask=None)
    D = [ms.desc[k][l] for k, l in rows]
    Mk = [ms.mask[k][l] for k, l in rows] if ms.masks else None
    BestMedian, BestIdx = 2**31 - 1, 0                            # :362-363
    if N > 2:                                                     # :364
        Distances = distance_matrix(np.stack(D), np.stack(Mk) if Mk else None)   # :339-359
        for i in range(N - 1):                                    # :366
            vDists = Distances[i, i + 1:]                         # :369-370
            medianV = int(np.sort(vDists)[len(vDists) // 2])      # nth_element at size / 2
            if medianV < BestMedian:                              # :373
                BestMedian, BestIdx = medianV, i
    k, l = rows[BestIdx]
    return dict(n_desc=N, best_kf=k, best_feat=l, desc=D[BestIdx].copy(), mask=Mk[BestIdx].copy() if Mk else None)   # :384-386


SENTINEL = dict(normal=-7.5, min_dist=-7.5, max_dist=-7.5, min_inv=-7.5, max_inv=-7.5, n_desc=-77, best_kf=-77, best_feat=-77, status=-77)
DESC_OUTPUTS = ("desc", "mask", "n_desc", "best_kf", "best_feat")


def update_points(ms, ids, pos, ref_kf, scale_factors, desc=None, mask=None, max_points=None):
    """mcs_covis_update_points on the model: every output starts from its sentinel (desc / mask: from the arrays given) and an entry whose status is not 0
    keeps it.  max_points: an id outside [0, max_points) reads status 1 (device kind).  -> dict of arrays, list-indexed"""
    n = len(ids)
    out = dict(normal=np.full((n, 3), SENTINEL["normal"]), status=np.full(n, SENTINEL["status"], np.int32))
    for k in ("min_dist", "max_dist", "min_inv", "max_inv"):
        out[k] = np.full(n, SENTINEL[k])
    if desc is not None:
        out.update(desc=np.array(desc, np.uint8).reshape(n, -1).copy(), n_desc=np.full(n, SENTINEL["n_desc"], np.int32),
                   best_kf=np.full(n, SENTINEL["best_kf"], np.int64), best_feat=np.full(n, SENTINEL["best_feat"], np.int32))
        if mask is not None:
            out["mask"] = np.array(mask, np.uint8).reshape(out["desc"].shape).copy()
    obs = ms.observation_table()
    for i, p in enumerate(int(q) for q in ids):
        if max_points is not None and not 0 <= p < max_points:
            out["status"][i] = 1
            continue
        st, r = update_normal_and_depth(ms, p, pos[i], int(ref_kf[i]), scale_factors, obs)
        out["status"][i] = st
        if st:
            continue
        out["normal"][i] = r["normal"]
        for k in ("min_dist", "max_dist", "min_inv", "max_inv"):
            out[k][i] = r[k]
        if desc is not None:
            d = compute_distinctive_descriptors(ms, p, obs)
            out["n_desc"][i], out["best_kf"][i], out["best_feat"][i] = d["n_desc"], d["best_kf"], d["best_feat"]
            if d["desc"] is not None:
                out["desc"][i] = d["desc"]
                if "mask" in out and d["mask"] is not None:
                    out["mask"][i] = d["mask"]
    return out
