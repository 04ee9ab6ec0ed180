"""Hostile keyframes for the CreateNewMapPoints chain (csrc/mcs_newpoints.hip): the table of cases that tests/test_newpoints_hostile_cpu.py (the model alone: every
condition a case is there for) and tests/test_gpu_hostile_newpoints.py (device == model, doubles bit for bit) both walk.  Plain module: numpy, the model of
tests/newpoints_model.py and the CPU oracle, nothing of the device.

  1  median depth and the gate   k_np_median's rank selection under ties, NaN, infinities, at every tile boundary; the gate at the double 0.01 and its neighbours
  2  rigs of 16, 17, 32 cameras  k_np_setup's loop over nrCams^2 essential matrices beyond its first trip of 256
  3  compaction                  k_np_compact at the wave and chunk boundaries, with every accept pattern
  4  exact thresholds            cosParallax == cosThresh, dist == maxDIST, cosParallax == 0, dist == 0
  5  camera models               np_world_to_cam under polynomial degrees 1 .. MCS_MAX_POLY, affine terms, a principal point outside the image
  6  guards and staging          entries outside their arrays, a repeated first keyframe, masked descriptors"""
import importlib
import math

import numpy as np

import hostile_cameras as HC
import hostile_sim3 as T
import newpoints_model as M
import oracle_lib as O

synth = importlib.import_module("multicol-slam_amd.synth")
INT_MIN, INT_MAX = -2 ** 31, 2 ** 31 - 1
NAN, INF = float("nan"), float("inf")
_CACHE = {}


def _once(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def chain_model(key, kf1, nb, **kw):
    """the model's run of a chain case, computed once and left unchanged -> (per neighbour dicts, final valid1)"""
    def make():
        with np.errstate(all="ignore"):
            return M.create_new_map_points(kf1, nb, **kw)
    return _once(("model", key), make)


def pair_model(key, pairs, matches, **kw):
    """... and of the pairs of a mcs_triangulate_matches case"""
    def make():
        with np.errstate(all="ignore"):
            return [M.triangulate_matches(a, b, m, **kw) for (a, b), m in zip(pairs, matches)]
    return _once(("pairs", key), make)


def lafida0():
    return synth.lafida_cameras()[0]


def translation(t):
    P = np.eye(4)
    P[:3, 3] = t
    return P


def observe(cams, M_c, M_t, X, cam):
    """exact keypoints (the oracle's projection) and unit rays (camera frame) of world points X [m, 3] seen by cameras cam [m] of the rig at M_t"""
    kf = M.KF(cams, M_c, M_t, np.zeros(0, O.KP_DTYPE), np.zeros(0, np.int32), np.zeros((0, 3)), np.zeros((0, 32), np.uint8), None, np.zeros(0, bool), np.zeros((0, 3)))
    X, cam = np.asarray(X, np.float64).reshape(-1, 3), np.asarray(cam, np.int32)
    uv, _ = O.world_to_cam(kf.MtMc_inv.reshape(-1, 16), cams, None, X, cam)
    Xc = np.einsum("mij,mj->mi", kf.MtMc_inv[cam][:, :3, :3], X) + kf.MtMc_inv[cam][:, :3, 3]
    return uv, Xc / np.linalg.norm(Xc, axis=1)[:, None]


def keyframe(cams, M_c, M_t, uv, cam, rays, desc=None, mask=None):
    """a keyframe none of whose features holds a map point"""
    n = len(uv)
    keys = np.zeros(n, O.KP_DTYPE)
    if n:
        keys["x"], keys["y"] = np.asarray(uv)[:, 0], np.asarray(uv)[:, 1]
    keys["size"], keys["response"], keys["class_id"] = 31.0, 50.0, -1
    desc = np.zeros((n, 32), np.uint8) if desc is None else desc
    return M.KF(cams, M_c, M_t, keys, np.asarray(cam, np.int32).reshape(n), np.asarray(rays, np.float64).reshape(n, 3), desc, mask, np.zeros(n, bool), np.zeros((n, 3)))


def view(M_t, X, desc=None):
    """the one-camera rig (camera = rig frame, LaFiDa camera 0) at M_t observing the world points X"""
    cams, M_c = [lafida0()], [np.eye(4)]
    uv, rays = observe(cams, M_c, M_t, X, np.zeros(len(X), np.int32))
    return keyframe(cams, M_c, M_t, uv, np.zeros(len(X), np.int32), rays, desc)


def clone(kf, **changes):
    """a copy of a keyframe with some of its fields replaced (poses and cameras stay)"""
    f = dict(keys=kf.keys.copy(), cam=kf.cam.copy(), rays=kf.rays.copy(), desc=kf.desc.copy(), mask=None if kf.mask is None else kf.mask.copy(),
             has_mp=kf.has_mp.copy(), mp_pos=kf.mp_pos.copy(), cams=kf.cams)
    f.update(changes)
    out = M.KF(f["cams"], kf.M_c, kf.M_t, f["keys"], f["cam"], f["rays"], f["desc"], f["mask"], f["has_mp"], f["mp_pos"])
    out.mp = kf.mp
    return out


# ---- 1: median depth and the gate --------------------------------------------------------------------------------------------------------------------------
# The neighbours are one-camera rigs translated by (tx, 0, tz) with integer tz: row 2 of MtMc_inv is (0, 0, 1, -tz), so the map point (x, y, d + tz) has the depth
# d exactly (d and tz are small dyadic numbers), and the baseline to the current keyframe at the origin is sqrt(tx^2 + tz^2).
MEDIAN_COUNTS = (1, 2, 3, 4, 255, 256, 257, 511, 512, 513, 1025)
MEDIAN_PATTERNS = ("distinct", "equal", "tie", "negative", "zero", "zero_at_kf1", "inf", "nan_minor", "nan_major")
POINTS = [(-0.6 + 0.25 * (i % 6) + 0.03125 * (i // 6), 0.5 - 0.2 * (i % 5), 4.0 + 0.5 * (i % 7)) for i in range(18)]   # the current keyframe sees all of them
SEEN = 6                                                                                                                  # ... neighbour k six, from 3 k on
POINT_DESC = np.random.default_rng(77).integers(0, 256, (len(POINTS), 32), dtype=np.uint8)
TILE = 256   # k_np_median stages the depths 256 at a time


def rank(n):
    return (n - 1) // 2   # vDepths[(vDepths.size() - 1) / 2]


def expected_median(depths):
    """the ascending sort with every NaN behind every number, by hand (not np.sort)"""
    d = [float(v) for v in depths]
    s = sorted(v for v in d if not math.isnan(v)) + [NAN] * sum(math.isnan(v) for v in d)
    return s[rank(len(d))]


def expected_skip(baseline, median):
    """ratioBaselineDepth < 0.01 as an IEEE comparison: false for a NaN ratio (0 / 0, x / NaN), true for a negative one"""
    if math.isnan(median) or (baseline == 0.0 and median == 0.0):
        return False
    return (math.copysign(INF, median) if median == 0.0 else baseline / median) < 0.01


def tie_depths(n):
    """a run of equal depths that holds the wanted rank and lies across array index 255 / 256 (in the middle of a shorter array); distinct depths around it"""
    L, r = min(n, 12), rank(n)
    start = TILE - L // 2 if n > TILE else (n - L) // 2
    L = min(n, start + L) - start                             # (n = 257: the run ends with the array, seven long)
    below = max(0, min(r - L // 2, n - L))                    # depths smaller than the run's: the run takes ranks below .. below + L - 1
    others = [6.0 + k for k in range(n - L - below)][::-1] + [1.0 + k / 1024.0 for k in range(below)][::-1]
    d = others[:start] + [5.0] * L + others[start:]
    assert len(d) == n and below <= r < below + L
    return np.array(d), (start, start + L)


def median_depths(pattern, n):
    """-> (depths [n] as the kernel is to compute them, tx, tz, positions x that carry an infinity (the depth is then 0 * inf = NaN))"""
    r, i = rank(n), np.arange(n)
    desc = (n - i).astype(np.float64)                         # n .. 1
    none = np.zeros(n, bool)
    if pattern == "distinct":
        return desc, 1.0, 1, none                             # median r + 1: gated from 1 / (r + 1) < 0.01 on
    if pattern == "equal":
        return np.full(n, 7.0), 1.0, -2, none
    if pattern == "tie":
        return tie_depths(n)[0], 0.03125, 2, none             # sqrt(0.03125^2 + 2^2) / 5 > 0.01: only the gate cases decide closely
    if pattern == "negative":                                 # r + 1 negative depths, the rest positive, the positive ones first
        return np.array([3.0 + k for k in range(n - r - 1)] + [-0.5 * (k + 1) for k in range(r + 1)]), 1.0, 0, none
    if pattern in ("zero", "zero_at_kf1"):                    # r negative depths, up to three zeros, the rest positive; descending
        nz = min(3, n - r)
        d = np.array([2.0 + k for k in range(n - r - nz)][::-1] + [0.0] * nz + [-1.0 - k for k in range(r)])
        return (d, 1.0, 3, none) if pattern == "zero" else (d, 0.0, 0, none)
    if pattern == "inf":
        d = desc.copy()
        d[0] = INF
        if n >= 4:
            d[n // 2] = INF
        return d, 1.0, 1, none
    if pattern == "nan_minor":                                # every third depth NaN: a NaN z and an infinite x in turn
        bad = (i % 3 == 1)
    elif pattern == "nan_major":
        bad = (i % 3 != 1) | (n <= 2)
    else:
        raise KeyError(pattern)
    d, infx = desc.copy(), none.copy()
    k = np.flatnonzero(bad)
    d[k] = NAN
    infx[k[1::2]] = True
    return d, 1.0, 1, infx


def depth_neighbour(depths, tx, tz, infx=None, mp_cam=None, k=0):
    sel = [(3 * k + j) % len(POINTS) for j in range(SEEN)]
    kf = view(translation([tx, 0.0, float(tz)]), [POINTS[j] for j in sel], POINT_DESC[sel])
    n = len(depths)
    i = np.arange(n)
    pos = np.stack([(i % 5) - 2.0, (i % 3) - 1.0, np.asarray(depths, np.float64) + float(tz)], axis=1)
    if infx is not None and infx.any():
        pos[infx, 0] = INF * np.where(i[infx] % 2 == 0, 1.0, -1.0)
        pos[infx, 2] = 1.0                                    # (a finite z: the NaN comes from 0 * inf alone)
    kf.mp = (pos, np.zeros(n, np.int32) if mp_cam is None else np.asarray(mp_cam, np.int32))
    return kf


def current_keyframe():
    return view(np.eye(4), POINTS, POINT_DESC)


def median_neighbour(pattern, n, k=0):
    d, tx, tz, infx = median_depths(pattern, n)
    kf = depth_neighbour(d, tx, tz, infx, k=k)
    med = expected_median(d)
    return kf, dict(label="%s n=%d" % (pattern, n), median=med, skipped=expected_skip(math.sqrt(tx * tx + tz * tz), med), n_mp=n)


# baseline / median == the double 0.01 and its two neighbours: searched (find_gate_triple) and kept.  (median, (baseline below, at, above))
GATE_TRIPLES = ((100.0, (float.fromhex("0x1.fffffffffffffp-1"), 1.0, float.fromhex("0x1.0000000000001p+0"))),
                (12.5, (float.fromhex("0x1.fffffffffffffp-4"), 0.125, float.fromhex("0x1.0000000000001p-3"))))


def find_gate_triple(median):
    """the baselines nearest to 0.01 * median whose quotient by the median is nextafter(0.01, 0), 0.01 and nextafter(0.01, 1)"""
    want = (np.nextafter(0.01, 0.0), np.float64(0.01), np.nextafter(0.01, 1.0))
    b0 = np.float64(0.01) * np.float64(median)
    cand = [b0]
    for _ in range(64):
        cand = [np.nextafter(cand[0], 0.0)] + cand + [np.nextafter(cand[-1], INF)]
    out = []
    for w in want:
        hits = [float(b) for b in cand if b / np.float64(median) == w]
        out.append(min(hits, key=lambda b: abs(b - float(b0))))
    return tuple(out)


def gate_neighbours():
    """six neighbours: per triple below (gated), at and above 0.01 (not gated).  Three map points around the median; the baseline lies along x"""
    out = []
    for med, bs in GATE_TRIPLES:
        for b, name in zip(bs, ("below", "at", "above")):
            kf = depth_neighbour([med + 1.0, med, med - 1.0], b, 0, k=len(out))
            out.append((kf, dict(label="gate %s 0.01, median %g" % (name, med), median=med, skipped=name == "below", n_mp=3)))
    return out


MIXED = (("tie", 1025), ("distinct", 3), ("nan_minor", 513), ("equal", 1), ("negative", 512), ("zero", 2), ("inf", 257), ("tie", 4), ("nan_major", 256), ("distinct", 255))


def median_calls():
    """name -> (current keyframe, [neighbours], [expectations]): one call per count with every pattern, one with lengths going up and down (the depth scratch
    is reused in stream order: a shorter neighbour behind a longer one), one with the gate triples"""
    def make():
        calls = {}
        for n in MEDIAN_COUNTS:
            calls["n%d" % n] = [median_neighbour(p, n, k) for k, p in enumerate(MEDIAN_PATTERNS)]
        calls["mixed"] = [median_neighbour(p, n, k) for k, (p, n) in enumerate(MIXED)]
        calls["gate"] = gate_neighbours()
        return {k: (current_keyframe(), [x[0] for x in v], [x[1] for x in v]) for k, v in calls.items()}
    return _once("median", make)


OUTSIDE_CAMS = (-1, 1, INT_MAX, INT_MIN)   # map point cameras outside the one-camera rig


def outside_camera_call():
    """device kind only (host kind refuses it): every third map point names a camera outside the rig -> a NaN depth, as nan_minor's"""
    def make():
        nb, exp = [], []
        for n in (3, 257, 1025):
            d, tx, tz, _ = median_depths("distinct", n)
            i = np.arange(n)
            cam = np.where(i % 3 == 1, np.array(OUTSIDE_CAMS)[(i // 3) % 4], 0)
            nb.append(depth_neighbour(d, tx, tz, None, cam, k=len(nb)))
            med = expected_median(np.where(i % 3 == 1, NAN, d))
            exp.append(dict(label="outside cameras n=%d" % n, median=med, skipped=expected_skip(math.sqrt(tx * tx + tz * tz), med), n_mp=n))
        return current_keyframe(), nb, exp
    return _once("outside", make)


# ---- 2: essential matrices beyond 256 pairs ----------------------------------------------------------------------------------------------------------------
RIG_SIZES = (16, 17, 32)
SETUP_TRIP = 256   # k_np_setup forms matrix t = threadIdx.x, threadIdx.x + 256, ...


def rig_scene(nr):
    return _once(("rig", nr), lambda: M.make_scene(seed=40 + nr, nr_cams=nr, n_points=25 * nr, n_neigh=2, clutter=4, gated=-1))


def search_with_later_blocks_zeroed(kf1, valid1, kf2, E, check_ori):
    E = E.copy()
    E[SETUP_TRIP:] = 0.0
    return M.oracle_search(kf1, valid1, kf2, E, check_ori)


# ---- 3: compaction ---------------------------------------------------------------------------------------------------------------------------------------------
COMPACT_N1 = (0, 1, 63, 64, 65, 1023, 1024, 1025, 2049)
COMPACT_PATTERNS = ("all", "none", "first", "last", "i1024", "second", "every65")


def accept_pattern(name, n1):
    """-> bool [n1], or None where the pattern has no row to name"""
    a, i = np.zeros(n1, bool), np.arange(n1)
    if name == "all":
        a[:] = True
    elif name == "first" or name == "last" or name == "i1024":
        k = dict(first=0, last=n1 - 1, i1024=1024)[name]
        if not 0 <= k < n1:
            return None
        a[k] = True
    elif name == "second":
        a = i % 2 == 1
    elif name == "every65":
        a = i % 65 == 64
    return a


def compact_pairs(n1):
    """[(pattern, kf1, kf2, match12, accept)]: row i of keyframe 1 observes its own world point, which feature n1 - 1 - i of keyframe 2 observes too (accepted);
    a rejected row carries its partner's ray instead (parallel rays: stopped at the parallax check, as in test_degenerate_pairs_on_the_device)"""
    def make():
        i = np.arange(n1)
        X = np.stack([0.3 + (i % 97) / 128.0, 0.2 - (i % 89) / 128.0, 4.0 + (i % 13) / 8.0], axis=1).reshape(n1, 3)
        a = view(np.eye(4), X)
        b = view(translation([1.0, 0.0, 0.0]), X[::-1])
        m12 = (n1 - 1 - i).astype(np.int32)
        out = []
        for name in COMPACT_PATTERNS:
            acc = accept_pattern(name, n1)
            if acc is None:
                continue
            rays = a.rays.copy()
            rays[~acc] = b.rays[m12[~acc]]
            out.append((name, clone(a, rays=rays), b, m12, acc))
        return out
    return _once(("compact", n1), make)


# ---- 4: exact thresholds -------------------------------------------------------------------------------------------------------------------------------------
def threshold_pair():
    """one accepted pair -> (kf1, kf2, match12)"""
    X = [[0.3, 0.2, 4.0]]
    return view(np.eye(4), X), view(translation([1.0, 0.0, 0.0]), X), np.array([0], np.int32)


QUARTER_Y = np.array([[0.0, 0.0, -1.0], [0.0, 1.0, 0.0], [1.0, 0.0, 0.0]])   # camera z axis = world -x, camera x axis = world +z


def _rig_at(M_c, R, t, key_of_X):
    """a one-camera rig with rotation R, centre t and camera pose M_c in the rig; one feature looking along the camera's axis, keypoint = projection of X"""
    M_t = np.eye(4)
    M_t[:3, :3], M_t[:3, 3] = R, t
    cams = [lafida0()]
    uv, _ = observe(cams, [M_c], M_t, [key_of_X], [0])
    return keyframe(cams, [M_c], M_t, uv, [0], [[0.0, 0.0, 1.0]])


def exact_pairs():
    """integer poses, axis-aligned rays: every product and sum up to x3D and the distances is exact.  -> [(label, kf1, kf2)], one feature each, match12 = [0]
      orthogonal  the rays meet at (0, 0, 2) under exactly 90 degrees: cosParallax == 0.0, not < 0
      on centre   the cameras sit one unit behind their rig centres; the rays meet in keyframe 1's rig centre: dist1 == 0
      in camera   the rays meet in keyframe 2's camera centre (camera = rig frame): z == 0 there"""
    behind = translation([0.0, 0.0, -1.0])
    out = [("orthogonal", _rig_at(np.eye(4), np.eye(3), [0.0, 0.0, 0.0], [0.0, 0.0, 2.0]), _rig_at(np.eye(4), QUARTER_Y, [2.0, 0.0, 2.0], [0.0, 0.0, 2.0])),
           ("on centre", _rig_at(behind, np.eye(3), [0.0, 0.0, 0.0], [0.0, 0.0, 0.0]), _rig_at(behind, QUARTER_Y, [2.0, 0.0, 0.0], [0.0, 0.0, 0.0]))]
    a = _rig_at(np.eye(4), np.eye(3), [0.0, 0.0, 0.0], [0.0, 0.0, 2.0])
    b = _rig_at(np.eye(4), np.eye(3), [0.0, 0.0, 2.0], [0.0, 0.0, 3.0])
    out.append(("in camera", a, clone(b, rays=np.array([[1.0, 0.0, 0.0]]))))
    return out


# ---- 5: camera models in the projection ----------------------------------------------------------------------------------------------------------------------
CAM_W, CAM_H = T.PROJ_W, T.PROJ_H
INVP_PAD = 1.0e3   # written behind invP_deg into the library's camera struct: must never be read


def _outside(cam, c, d, e, u0, v0):
    return dict(cam, c=c, d=d, e=e, u0=u0, v0=v0)


def camera_rigs():
    """name -> three cameras (hostile_cameras' table at 400 x 300, hostile_sim3's two polynomial lengths)"""
    def make():
        base = [HC.camera(n, CAM_W, CAM_H) for n in HC.CONTROLS]
        return {
            "degrees 16+1+12": [dict(T._max_poly(base[0])), dict(T._one_coefficient(base[1]), invP_pad=INVP_PAD), dict(base[2], invP_pad=INVP_PAD)],
            "degrees 1+6+16": [dict(T._one_coefficient(base[0]), invP_pad=-INVP_PAD), dict(HC.camera("short", CAM_W, CAM_H), invP_pad=INVP_PAD),
                               dict(T._max_poly(base[2]))],
            "affine": [HC.camera("s160", CAM_W, CAM_H), HC.camera("shear", CAM_W, CAM_H), HC.camera("shrink", CAM_W, CAM_H)],
            "corners": [HC.camera("corner160", CAM_W, CAM_H), HC.camera("corner_br", CAM_W, CAM_H), HC.camera("flipped", CAM_W, CAM_H)],
            "outside": [_outside(base[0], 1.15, 0.1, -0.1, -40.0, -30.0), _outside(base[1], 1.0, 0.0, 0.0, CAM_W + 25.0, CAM_H / 2.0),
                        _outside(base[2], 0.9, -0.2, 0.3, CAM_W / 2.0, CAM_H + 60.0)],
        }
    return _once("camera_rigs", make)


def camera_scene(name):
    rigs = camera_rigs()
    return _once(("cam", name), lambda: M.make_scene(seed=60 + list(rigs).index(name), nr_cams=3, n_points=900, n_neigh=3, clutter=20, cams=rigs[name]))


def plain_cameras(cams):
    """what a kernel would see that ignored the coefficients past the calibrations' twelve and a camera's affine terms: c = 1, d = e = 0, the centre in the image centre"""
    return [dict(c, invP=list(c["invP"])[:12], c=1.0, d=0.0, e=0.0, u0=CAM_W / 2.0, v0=CAM_H / 2.0) for c in cams]


def padded_cameras(cams):
    """what a kernel would see that read all MCS_MAX_POLY coefficients of the struct whatever the degree says"""
    return [dict(c, invP=list(c["invP"]) + [c["invP_pad"]] * (16 - len(c["invP"]))) if "invP_pad" in c else c for c in cams]


def with_cameras(kf, cams):
    return clone(kf, cams=cams)


def bad_degree_scene(deg):
    """the first neighbour's camera 1 declares invP_deg = deg"""
    kf1, nb = camera_scene("affine")
    cams = [dict(c) for c in nb[0].cams]
    cams[1] = dict(cams[1], invP_deg=deg)
    return kf1, [with_cameras(nb[0], cams)] + nb[1:]


# ---- 6: guards and staging ---------------------------------------------------------------------------------------------------------------------------------------
def guard_scene():
    """-> (kf1, [two neighbours], [their matches, every neighbour searched on its own])"""
    def make():
        kf1, nb = M.make_scene(seed=71, nr_cams=3, n_points=900, n_neigh=2, clutter=20, gated=-1)
        return kf1, nb, [M.oracle_search(kf1, ~kf1.has_mp, kf2, M.essential_matrices(kf1, kf2), False) for kf2 in nb]
    return _once("guard", make)


def guard_inputs():
    """-> dict: the clean pair (kf1, kf2, match12) and what the bad inputs are made of.
      bad_match   row -> entry outside [0, kf2.n) on rows that held a match
      bad_cam1    features of keyframe 1 (matched ones) -> camera -1 / nr_cams
      bad_cam2    features of keyframe 2 (partners of matched rows) -> camera -1 / nr_cams"""
    kf1, nb, matches = guard_scene()
    kf2, m12 = nb[0], matches[0]
    rows = np.flatnonzero(m12 >= 0)
    assert len(rows) >= 40
    pick = rows[::max(1, len(rows) // 16)][:12]
    bad_match = {int(r): v for r, v in zip(pick[:4], (-7, INT_MIN, kf2.n, INT_MAX))}
    bad_cam1 = {int(r): v for r, v in zip(pick[4:8], (-1, kf1.nr, -1, kf1.nr))}
    bad_cam2 = {int(m12[r]): v for r, v in zip(pick[8:12], (-1, kf2.nr, kf2.nr, -1))}
    return dict(kf1=kf1, kf2=kf2, match12=m12, bad_match=bad_match, bad_cam1=bad_cam1, bad_cam2=bad_cam2)


def guarded(g, match=True, cam1=True, cam2=True):
    """-> (kf1, kf2, match12 as handed to the library, match12 as the model is to see it: -1 on every row a guard stops)"""
    kf1, kf2, m_in = g["kf1"], g["kf2"], g["match12"].copy()
    m_want = g["match12"].copy()
    if match:
        for r, v in g["bad_match"].items():
            m_in[r], m_want[r] = v, -1
    if cam1:
        c = kf1.cam.copy()
        for r, v in g["bad_cam1"].items():
            c[r], m_want[r] = v, -1
        kf1 = clone(kf1, cam=c)
    if cam2:
        c = kf2.cam.copy()
        for j, v in g["bad_cam2"].items():
            c[j] = v
            m_want[g["match12"] == j] = -1
        kf2 = clone(kf2, cam=c)
    return kf1, kf2, m_in, m_want


def aba_pairs():
    """first keyframes A, B, A: B has A's size and other contents (A's features in reverse order) -> ([(kf1, kf2)], [match12])"""
    A, nb, matches = guard_scene()
    B = clone(A, keys=A.keys[::-1].copy(), cam=A.cam[::-1].copy(), rays=A.rays[::-1].copy(), desc=A.desc[::-1].copy(), has_mp=A.has_mp[::-1].copy(),
              mp_pos=A.mp_pos[::-1].copy())
    mB = M.oracle_search(B, ~B.has_mp, nb[1], M.essential_matrices(B, nb[1]), False)
    return [(A, nb[0]), (B, nb[1]), (A, nb[1])], [matches[0], mB, matches[1]]


def masked_scene():
    """the guard scene with descriptor masks on every keyframe (about one bit in eight masked out).  Every fifth feature of a neighbour has the first ten
    bytes of its descriptor inverted and masked out: found with the masks, lost (80 bits apart) without them -> (kf1, neighbours)"""
    def make():
        kf1, nb, _ = guard_scene()
        rng = np.random.default_rng(72)

        def masked(kf, invert):
            m, d = np.zeros(kf.desc.shape, np.uint8), kf.desc.copy()
            for _ in range(3):
                m |= rng.integers(0, 256, kf.desc.shape, dtype=np.uint8)
            if invert:
                d[::5, :10] ^= np.uint8(255)
                m[::5, :10] = 0
            else:   # the masked distance is the mean of the two sides' counts: the current keyframe masks three bits in four of those bytes
                m[:, :10] &= rng.integers(0, 256, (kf.n, 10), dtype=np.uint8) & rng.integers(0, 256, (kf.n, 10), dtype=np.uint8)
            return clone(kf, desc=d, mask=m)
        return masked(kf1, False), [masked(k, True) for k in nb]
    return _once("masked", make)


def without_masks(kf):
    return clone(kf, mask=None)


def empty_current_keyframe():
    """n1 = 0"""
    return view(np.eye(4), np.zeros((0, 3)), np.zeros((0, 32), np.uint8))


def featureless_neighbour():
    """no feature, three map points"""
    kf = view(translation([1.0, 0.0, 0.0]), np.zeros((0, 3)), np.zeros((0, 32), np.uint8))
    kf.mp = (np.array([[0.0, 0.0, 3.0], [1.0, 0.0, 5.0], [0.0, 1.0, 4.0]]), np.zeros(3, np.int32))
    return kf
